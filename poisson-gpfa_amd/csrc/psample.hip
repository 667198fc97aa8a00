// libpgpfa_hip.so - psample.hip (one translation unit of the C-ABI library; shared declarations: ctx.h): joint posterior samples of the latents and
// posterior-predictive spike counts (pgpfa_posterior_sample); importance weights of the Laplace posterior's draws (pgpfa_importance_weights)
#include "query.h"
#include "model.h"
#include "sample.h"
#include "psample.h"
#include "impw.h"

using namespace pgpfa;

namespace {

constexpr int GEMM_COL_SLACK = 128;                          // the GEMM stages whole column tiles of its second operand: columns past N are read, never used

struct SampleArgs {
  const std::vector<int>* trials;     // trial of every list position
  int S; unsigned long long seed;
  const double* noise_in; double* noise_out; double* X; uint16_t* Y; int32_t* count_sum;
  bool lowrank;                       // engine the call's noise dimension was sized for
  int nz;
  // step 6, pgpfa_importance_weights (all NULL: not asked for - the call path is the one it was): per list position
  double* log_ratio; double* ess; double* log_w;
  const char* entry;                  // the entry point, for its messages (NULL: pgpfa_posterior_sample)
};

// the positions `pos` of the list (one snapshot, one kind of posterior), under that snapshot's parameters
int sample_group(pgpfa_ctx* c, const SampleArgs& a, const std::vector<int>& pos, bool dual) {
  CHK(ready_root(c, dual));
  const int n = c->n, q = c->q, p = c->p, T = c->T, S = a.S, nz = a.nz;
  const bool lr = c->plan_lowrank;
  const int t_first = (*a.trials)[pos[0]];
  if (lr != a.lowrank)
    return fail("the posterior of trial %d takes the %s covariance engine, the noise of this call was sized for the %s one: sample those trials in a call of their own",
                t_first, lr ? "low-rank" : "dense", a.lowrank ? "low-rank" : "dense");
  const int rz = lr ? c->rtot : 0, rpad = c->rpad, npad = c->npad;
  if (rz > nz - n && (a.noise_in || a.noise_out))          // (without noise arrays every group simply uses its own system's rows)
    return fail("the posterior of trial %d was computed under timescales whose low-rank system has %d rows, the noise of this call has %d (the rank under the current "
                "parameters): set the parameters of that E-step before sampling it", t_first, rz, nz - n);
  const bool want_counts = a.Y || a.count_sum;
  const bool want_weights = a.log_ratio || a.ess || a.log_w;
  const char* entry = a.entry ? a.entry : "pgpfa_posterior_sample";
  const int ntile = (T + 15) / 16;                             // bin tiles of impw_kernel

  // chunks of the group: device staging per trial (noise, U, trajectories, count planes)
  const size_t ldz = lr ? (size_t)rpad : (size_t)npad;       // leading dimension of the GEMM's noise operand (z2 panel / dense z), zero below the rows in use
  const size_t per_trial = (size_t)S * (((lr ? 2 * ldz + n : ldz) + n) * sizeof(double) + (a.Y ? (size_t)q * T * sizeof(uint16_t) : 0) + (want_counts ? (size_t)q * sizeof(int) : 0) +
                                              (want_weights ? (size_t)(ntile + 1) * sizeof(double) : 0));
  const int chunk = query_chunk(pos.size(), c->sample_chunk, per_trial, (size_t)c->B);
  if ((long long)chunk * S > (1LL << 30)) return fail("%s: %d samples of %d trials exceed one chunk's columns", entry, S, chunk);
  if (want_weights && (chunk > 65535 || (S + IMPW_NS - 1) / IMPW_NS > 65535))
    return fail("%s: %d samples of %d trials per chunk exceed the weight kernel's grid (65535 trials, %d samples)", entry, S, chunk, 65535 * IMPW_NS);

  DevBufs dev(entry);
  double *dX = nullptr, *dZ1 = nullptr, *dZ = nullptr, *dU = nullptr;
  uint16_t* dY = nullptr;
  int *dCs = nullptr, *dOver = nullptr, *dBad = nullptr;
  double *dPart = nullptr, *dLw = nullptr, *dLr = nullptr, *dEss = nullptr;
  const size_t cols = (size_t)chunk * S;
  CHK(dev.get(&dX, cols * n));
  CHK(dev.get(&dZ, (cols + GEMM_COL_SLACK) * ldz));
  HIPC(hipMemsetAsync(dZ, 0, (cols + GEMM_COL_SLACK) * ldz * sizeof(double), c->st));      // rows past the ones in use stay zero for the whole call
  if (lr) {
    CHK(dev.get(&dZ1, cols * n));
    CHK(dev.get(&dU, (cols + GEMM_COL_SLACK) * ldz));
    HIPC(hipMemsetAsync(dU, 0, (cols + GEMM_COL_SLACK) * ldz * sizeof(double), c->st));
  }
  if (a.Y) CHK(dev.get(&dY, cols * q * T));
  if (want_counts) { CHK(dev.get(&dCs, cols * q)); CHK(dev.get(&dOver, (size_t)chunk)); }
  if (want_weights) {
    CHK(dev.get(&dPart, cols * ntile)); CHK(dev.get(&dLw, cols));
    CHK(dev.get(&dLr, (size_t)chunk)); CHK(dev.get(&dEss, (size_t)chunk)); CHK(dev.get(&dBad, (size_t)chunk));
  }
  const int zused = lr ? rz : n;                               // rows of dZ a draw fills: z2, or the dense z
  const size_t zoff = lr ? (size_t)n : 0;                      // where they sit in a draw's nz normals

  std::vector<int> over(chunk), bad(want_weights ? chunk : 0), tos;
  std::vector<double> lr_h(want_weights ? chunk : 0), ess_h(want_weights ? chunk : 0);
  const size_t m = (size_t)q * T;
  for (size_t c0 = 0; c0 < pos.size(); c0 += chunk) {
    const int nb = (int)std::min<size_t>((size_t)chunk, pos.size() - c0);
    tos.assign(nb, 0);
    for (int s = 0; s < nb; ++s) tos[s] = (*a.trials)[pos[c0 + s]];
    // curvature blocks of the slots, as the blocks rebuilt on demand form them (cov.hip), then steps a - b of the covariance pass
    CHK(resident_curvature(c, tos, dual, "posterior", [&](double scale) { return posterior_factor_only(c, nb, scale); }));

    // 1. the normals: copied in, or drawn
    if (a.noise_in) {
      for (int s = 0; s < nb; ++s) {
        const double* src = a.noise_in + (size_t)pos[c0 + s] * S * nz;
        if (lr) HIPC(hipMemcpy2DAsync(dZ1 + (size_t)s * S * n, (size_t)n * sizeof(double), src, (size_t)nz * sizeof(double), (size_t)n * sizeof(double), S, hipMemcpyHostToDevice, c->st));
        if (zused > 0)
          HIPC(hipMemcpy2DAsync(dZ + (size_t)s * S * ldz, ldz * sizeof(double), src + zoff, (size_t)nz * sizeof(double), (size_t)zused * sizeof(double), S, hipMemcpyHostToDevice, c->st));
      }
    } else {
      if (lr) {
        const int nblk = (n + 511) / 512;
        hipLaunchKernelGGL(psample_noise_kernel, dim3((unsigned)S * nblk, nb), dim3(256), 0, c->st, dZ1, (long long)n, n, S, nblk, a.seed, PS_STREAM_Z1, c->trial_of_slot);
      }
      if (zused > 0) {
        const int nblk = (zused + 511) / 512;
        hipLaunchKernelGGL(psample_noise_kernel, dim3((unsigned)S * nblk, nb), dim3(256), 0, c->st, dZ, (long long)ldz, zused, S, nblk, a.seed, lr ? PS_STREAM_Z2 : PS_STREAM_Z1,
                           c->trial_of_slot);
      }
      HIPC(hipGetLastError());
    }
    if (lr) {
      // 2. U = L^-T Z2 per slot, then Yv_k = F_k U_k per latent over the S columns of every slot: the library's GEMM.  L^-T is upper triangular: tile row
      //    ti starts its k loop at its first row (KF_BEGIN_ROW), which skips the zero half in 64-row steps and keeps the launch off the split-K path - the
      //    number of k parts there follows the number of tiles, i.e. the chunk and the sample count, and the bits of a draw must not.  The products with F
      //    stay off it the same way (a one-level batch declared as the low half of a two-level one).
      GemmP u{};
      u.A = c->ws.Mt; u.sA = c->ws.sM; u.lda = rpad;
      u.B = dZ; u.sB = (long long)S * ldz; u.ldb = (int)ldz;
      u.C = dU; u.sC = (long long)S * ldz; u.ldc = (int)ldz;
      u.M = rpad; u.N = S; u.K = rpad; u.alpha = 1.0; u.beta = 0.0;
      u.slots = c->ident; u.nbatch = nb; u.mode = GEMM_FULL; u.kflags = KF_BEGIN_ROW;
      CHK(gemm(c, true, u));
      for (int k = 0; k < p; ++k) {
        GemmP g{};
        g.A = c->Flr + (size_t)k * c->Tp * c->Tp; g.sA = 0; g.lda = c->Tp;
        g.B = dU + c->roff[k]; g.sB = (long long)S * ldz; g.ldb = (int)ldz;
        g.C = dX + (size_t)k * T; g.sC = (long long)S * n; g.ldc = n;
        g.M = T; g.N = S; g.K = c->rk[k]; g.alpha = 1.0; g.beta = 0.0;
        g.slots = c->ident; g.nbatch = nb; g.nb_lo = nb; g.mode = GEMM_FULL; g.kflags = 0;
        CHK(gemm(c, true, g));
      }
      // 3. x = m + G yv + sqrt(eps) chol(G) z1, in place
      PsMixP mx{};
      mx.X = dX; mx.Z1 = dZ1; mx.G = c->Gbin; mx.Xmode = c->Xmode; mx.trial_of_slot = c->trial_of_slot;
      mx.S = S; mx.p = p; mx.T = T; mx.sqrt_eps = std::sqrt(c->eps);
      int rc = 0;
      dispatch_pw(p, [&](auto pw) {
        constexpr int PW = decltype(pw)::value;
        const size_t lds = psample_mix_lds(PW);
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&psample_mix_kernel<PW>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) { rc = 1; return; }
        hipLaunchKernelGGL(psample_mix_kernel<PW>, dim3((T + psample_bt(PW) - 1) / psample_bt(PW), nb), dim3(256), lds, c->st, mx);
      });
      if (rc) { (void)hipGetLastError(); return fail("%s: the mixing kernel's LDS size was refused", entry); }
    } else {
      // 5. dense engine: X = m + L^-T Z
      GemmP g{};
      g.A = c->ws.Mt; g.sA = c->ws.sM; g.lda = c->ld;
      g.B = dZ; g.sB = (long long)S * ldz; g.ldb = (int)ldz;
      g.C = dX; g.sC = (long long)S * n; g.ldc = n;
      g.M = n; g.N = S; g.K = npad; g.alpha = 1.0; g.beta = 0.0;
      g.slots = c->ident; g.nbatch = nb; g.mode = GEMM_FULL; g.kflags = KF_BEGIN_ROW;
      CHK(gemm(c, true, g));
      const int nblk = (n + 255) / 256;
      hipLaunchKernelGGL(psample_add_mean_kernel, dim3((unsigned)S * nblk, nb), dim3(256), 0, c->st, dX, c->Xmode, n, S, nblk, c->trial_of_slot);
    }
    HIPC(hipGetLastError());
    // 4. predictive counts
    if (want_counts) {
      HIPC(hipMemsetAsync(dOver, 0, sizeof(int) * nb, c->st));
      PsCountP cp{};
      cp.X = dX; cp.C = c->C; cp.d = c->d; cp.len = c->live.lengths(); cp.trial_of_slot = c->trial_of_slot;
      cp.Y = dY; cp.csum = a.count_sum ? dCs : nullptr; cp.over = dOver;
      cp.S = S; cp.q = q; cp.p = p; cp.T = T; cp.seed = a.seed;
      hipLaunchKernelGGL(psample_counts_kernel, dim3((unsigned)S, nb), dim3(256), 0, c->st, cp);
      HIPC(hipGetLastError());
      HIPC(hipMemcpyAsync(over.data(), dOver, sizeof(int) * nb, hipMemcpyDeviceToHost, c->st));
    }
    // 6. importance weights of the draws (impw.h): partial sums per (slot, draw, bin tile), then the tiles of a draw and the draws of a slot in order
    if (want_weights) {
      ImpwP ip{};
      ip.X = dX; ip.Xmode = c->Xmode; ip.C = c->C; ip.d = c->d; ip.trial_of_slot = c->trial_of_slot; ip.part = dPart;
      ip.S = S; ip.q = q; ip.p = p; ip.T = T; ip.ntile = ntile;
      c->live.fill(ip);
      const dim3 grid((unsigned)ntile, (unsigned)((S + IMPW_NS - 1) / IMPW_NS), (unsigned)nb);
      dispatch_obs(c->live.state(), [&](auto ob) { hipLaunchKernelGGL((impw_kernel<decltype(ob)::value>), grid, dim3(256), impw_lds(p), c->st, ip); });
      HIPC(hipGetLastError());
      hipLaunchKernelGGL(impw_reduce_kernel, dim3((unsigned)nb), dim3(256), 0, c->st, dPart, S, ntile, dLw, dLr, dEss, dBad);
      HIPC(hipGetLastError());
      HIPC(hipMemcpyAsync(bad.data(), dBad, sizeof(int) * nb, hipMemcpyDeviceToHost, c->st));
      HIPC(hipMemcpyAsync(lr_h.data(), dLr, sizeof(double) * nb, hipMemcpyDeviceToHost, c->st));
      HIPC(hipMemcpyAsync(ess_h.data(), dEss, sizeof(double) * nb, hipMemcpyDeviceToHost, c->st));
      if (a.log_w)
        for (int s = 0; s < nb; ++s)
          HIPC(hipMemcpyAsync(a.log_w + (size_t)pos[c0 + s] * S, dLw + (size_t)s * S, (size_t)S * sizeof(double), hipMemcpyDeviceToHost, c->st));
    }
    // results of the chunk, by list position
    for (int s = 0; s < nb; ++s) {
      const size_t ps = (size_t)pos[c0 + s];
      if (a.X) HIPC(hipMemcpyAsync(a.X + ps * S * n, dX + (size_t)s * S * n, (size_t)S * n * sizeof(double), hipMemcpyDeviceToHost, c->st));
      if (a.Y) HIPC(hipMemcpyAsync(a.Y + ps * S * m, dY + (size_t)s * S * m, (size_t)S * m * sizeof(uint16_t), hipMemcpyDeviceToHost, c->st));
      if (a.count_sum) HIPC(hipMemcpyAsync(a.count_sum + ps * S * q, dCs + (size_t)s * S * q, (size_t)S * q * sizeof(int), hipMemcpyDeviceToHost, c->st));
      if (a.noise_out) {
        double* dst = a.noise_out + ps * S * nz;
        if (lr) HIPC(hipMemcpy2DAsync(dst, (size_t)nz * sizeof(double), dZ1 + (size_t)s * S * n, (size_t)n * sizeof(double), (size_t)n * sizeof(double), S, hipMemcpyDeviceToHost, c->st));
        if (zused > 0)
          HIPC(hipMemcpy2DAsync(dst + zoff, (size_t)nz * sizeof(double), dZ + (size_t)s * S * ldz, ldz * sizeof(double), (size_t)zused * sizeof(double), S, hipMemcpyDeviceToHost, c->st));
      }
    }
    HIPC(hipStreamSynchronize(c->st));                         // the staging is reused by the next chunk
    HIPC(hipGetLastError());
    if (a.noise_out && (int)zoff + zused < nz)                // normals of the call's z2 this snapshot's smaller system has no row for: not used, reported as zeros
      for (int s = 0; s < nb; ++s)
        for (int j = 0; j < S; ++j) {
          double* dst = a.noise_out + ((size_t)pos[c0 + s] * S + j) * nz;
          std::fill(dst + zoff + zused, dst + nz, 0.0);
        }
    if (want_weights)
      for (int s = 0; s < nb; ++s) {
        if (bad[s]) return fail("%s: a log weight of trial %d is not a number: its mode, its draws or the parameters of its E-step are not finite", entry, tos[s]);
        if (a.log_ratio) a.log_ratio[pos[c0 + s]] = lr_h[s];
        if (a.ess) a.ess[pos[c0 + s]] = ess_h[s];
      }
    if (want_counts)
      for (int s = 0; s < nb; ++s)
        if (over[s]) return fail("a predictive count of trial %d exceeds 65535: the rates exp(d + C x) of its draws do not fit the uint16 output", tos[s]);
  }
  return 0;
}

}  // namespace

int pgpfa_posterior_sample(pgpfa_ctx* c, int n, const int32_t* idx, int n_samples, unsigned long long seed, const double* noise_in, double* noise_out, double* X,
                           uint16_t* Y, int32_t* count_sum) {
  if (!c) return fail("null context");
  if (n_samples < 1) return fail("pgpfa_posterior_sample: n_samples = %d, at least one draw per trial is needed", n_samples);
  if (!noise_out && !X && !Y && !count_sum) return fail("pgpfa_posterior_sample: no output asked for (noise_out, X, Y and count_sum are all NULL)");
  if (!c->have_params) return fail("set_params has not been called");
  if ((Y || count_sum) && !c->have_counts)
    return fail("spike counts have not been uploaded: predictive counts stop at every trial's own length, which is unknown without the counts table");
  if (c->tau_inflight) return fail("a timescale pass is in flight (pgpfa_mstep_tau_costgrad_multi_begin): collect it first");
  HIPC(hipSetDevice(c->device));
  Trials tr;
  CHK(resolve_trials(c, n, idx, &tr));
  CHK(require_resident(c, tr.v, RESIDENT_SAMPLABLE));
  SampleArgs a{};
  a.trials = &tr.v; a.S = n_samples; a.seed = seed; a.noise_in = noise_in; a.noise_out = noise_out; a.X = X; a.Y = Y; a.count_sum = count_sum;
  // engine and noise dimension under the current parameters (info key "sample_noise_dim"); variational trials follow option dual_lowrank
  bool any_laplace = false;
  for (int t : tr.v) any_laplace = any_laplace || !c->trial_dual[t];
  a.lowrank = want_lowrank(c) && (any_laplace || c->dual_lowrank);
  a.nz = c->n + (a.lowrank ? c->rtot : 0);
  return for_snapshot_groups(c, tr.v, [&](const std::vector<int>& pos, bool dual) { return sample_group(c, a, pos, dual); });
}

int pgpfa_importance_weights(pgpfa_ctx* c, int n, const int32_t* idx, int n_samples, unsigned long long seed, double* log_ratio, double* ess, double* log_w) {
  if (!c) return fail("null context");
  if (n_samples < 1) return fail("pgpfa_importance_weights: n_samples = %d, at least one draw per trial is needed", n_samples);
  if (!log_ratio && !ess && !log_w) return fail("pgpfa_importance_weights: no output asked for (log_ratio, ess and log_w are all NULL)");
  if (!c->have_params) return fail("set_params has not been called");
  if (!c->have_counts)
    return fail("spike counts have not been uploaded: the weights sum over every trial's live entries, which are unknown without the counts table");
  if (c->tau_inflight) return fail("a timescale pass is in flight (pgpfa_mstep_tau_costgrad_multi_begin): collect it first");
  HIPC(hipSetDevice(c->device));
  Trials tr;
  CHK(resolve_trials(c, n, idx, &tr));
  CHK(require_resident(c, tr.v, RESIDENT_SAMPLABLE));
  for (int t : tr.v)
    if (c->trial_dual[t])
      return fail("pgpfa_importance_weights: the posterior of trial %d is variational (pgpfa_dual_finalize): the identity behind the weights is the Laplace "
                  "approximation's - the Gaussian at a stationary mode with the Hessian as precision - and does not hold for it", t);
  SampleArgs a{};
  a.trials = &tr.v; a.S = n_samples; a.seed = seed; a.log_ratio = log_ratio; a.ess = ess; a.log_w = log_w; a.entry = "pgpfa_importance_weights";
  a.lowrank = want_lowrank(c);                                 // (every listed trial is a Laplace one: the engine of pgpfa_posterior_sample's draws)
  a.nz = c->n + (a.lowrank ? c->rtot : 0);
  return for_snapshot_groups(c, tr.v, [&](const std::vector<int>& pos, bool dual) { return sample_group(c, a, pos, dual); });
}
