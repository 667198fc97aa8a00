// libpgpfa_hip.so - covat.hip (one translation unit of the C-ABI library; shared declarations: ctx.h): the cross-latent posterior covariance and the
// log-rate moments at arbitrary time points (pgpfa_posterior_cov_at)
#include "ctx.h"
#include "interp.h"
#include "covat.h"

using namespace pgpfa;

namespace {

struct CovAtArgs {
  const std::vector<int>* trials;     // trial of every list position
  int S; const double* times; bool per_trial;
  double *mean, *cov, *eta, *var;
};

// the positions `pos` of the list (one snapshot, one kind of posterior), under that snapshot's parameters
int covat_group(pgpfa_ctx* c, const CovAtArgs& a, const std::vector<int>& pos, bool dual) {
  // (rates_kernel gathers both planes whichever of eta / var it stores)
  const bool want_rates = a.eta || a.var, want_cov = a.cov || want_rates, want_mean = a.mean || want_rates;
  if (want_cov) {
    CHK(ready_estep(c, dual ? c->dual_lowrank : true));
    if (dual) CHK(ensure_lambda(c));
  }
  const int p = c->p, q = c->q, T = c->T, S = a.S, pp = p * p;
  const bool lr = want_cov && c->plan_lowrank;
  const int T16 = round_up(T, 16), Spad = round_up(S, 16);
  const int N = (int)pos.size();
  std::vector<int> tos(N);
  for (int i = 0; i < N; ++i) tos[i] = (*a.trials)[pos[i]];

  // blocks of query times and chunks of the group: the right-hand sides of a block (p per time, rows_stage doubles each) and the planes of a chunk are
  // staged on the device
  const int rpad = lr ? c->rpad : 0, npad = c->npad;
  const size_t rows_stage = !want_cov ? 0 : (lr ? (size_t)p * T16 + 2 * (size_t)rpad : (size_t)npad);
  int SB = Spad;
  if (c->covat_block > 0) SB = std::min(Spad, round_up(c->covat_block, 16));
  else if (want_cov) {
    const size_t fit = QUERY_STAGE_BYTES / 8 / (rows_stage * p * sizeof(double));       // times per block that leave room for eight trials in a chunk
    SB = (int)std::min<size_t>((size_t)Spad, std::max<size_t>(16, fit / 16 * 16));
  }
  const size_t CC = (size_t)p * SB;
  const size_t slab = (size_t)p * T16 * Spad;
  const size_t planes = (want_mean ? (size_t)p * Spad : 0) + (want_cov ? (size_t)Spad * pp : 0) + ((a.eta ? 1 : 0) + (a.var ? 1 : 0)) * (size_t)q * Spad;
  const size_t per_trial = (rows_stage * CC + planes + (a.per_trial ? 2 * slab + S : 0)) * sizeof(double);
  const int chunk = query_chunk((size_t)N, c->covat_chunk, per_trial, want_cov ? (size_t)c->B : 0);
  const int grids = a.per_trial ? chunk : 1;

  DevBufs dev("pgpfa_posterior_cov_at");
  double *d_times = nullptr, *d_kx = nullptr, *d_A = nullptr, *d_mean = nullptr, *d_cov = nullptr, *d_eta = nullptr, *d_var = nullptr;
  double *d_V = nullptr, *d_W = nullptr, *d_Q = nullptr;
  int* d_trial = nullptr;
  CHK(dev.get(&d_times, (size_t)grids * S));
  CHK(dev.get(&d_kx, (size_t)grids * slab + GEMM_ROW_SLACK));
  CHK(dev.get(&d_A, (size_t)grids * slab + GEMM_ROW_SLACK));
  CHK(dev.get(&d_trial, (size_t)N));
  if (want_mean) CHK(dev.get(&d_mean, (size_t)chunk * p * Spad));
  if (want_cov) CHK(dev.get(&d_cov, (size_t)chunk * Spad * pp));
  if (a.eta) CHK(dev.get(&d_eta, (size_t)chunk * q * Spad));
  if (a.var) CHK(dev.get(&d_var, (size_t)chunk * q * Spad));
  HIPC(hipMemsetAsync(d_kx, 0, ((size_t)grids * slab + GEMM_ROW_SLACK) * sizeof(double), c->st));
  HIPC(hipMemsetAsync(d_A, 0, ((size_t)grids * slab + GEMM_ROW_SLACK) * sizeof(double), c->st));     // rows t >= T stay zero for the whole call
  const size_t q_rows = lr ? (size_t)rpad : (size_t)npad;
  if (want_cov) {
    CHK(dev.get(&d_Q, (size_t)chunk * q_rows * CC));
    HIPC(hipMemsetAsync(d_Q, 0, (size_t)chunk * q_rows * CC * sizeof(double), c->st));               // dense engine: the rows no product writes stay zero
    if (lr) {
      CHK(dev.get(&d_V, (size_t)chunk * p * T16 * CC + GEMM_ROW_SLACK));
      CHK(dev.get(&d_W, (size_t)chunk * rpad * CC + GEMM_ROW_SLACK));
      HIPC(hipMemsetAsync(d_V, 0, ((size_t)chunk * p * T16 * CC + GEMM_ROW_SLACK) * sizeof(double), c->st));   // rows t >= T stay zero for the whole call
      HIPC(hipMemsetAsync(d_W, 0, ((size_t)chunk * rpad * CC + GEMM_ROW_SLACK) * sizeof(double), c->st));      // so do the rank rows no latent owns
    }
  }
  HIPC(hipMemcpyAsync(d_trial, tos.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice, c->st));
  if (!a.per_trial) {
    HIPC(hipMemcpyAsync(d_times, a.times, (size_t)S * sizeof(double), hipMemcpyHostToDevice, c->st));
    CHK(interp_weights(c, d_times, 1, S, Spad, T16, d_kx, d_A));   // once per snapshot group, not per trial
  }
  const size_t expand_lds = (size_t)(pp + p) / 2 * COVAT_BT * sizeof(double);
  if (lr && expand_lds > ((size_t)48 << 10))
    HIPC(hipFuncSetAttribute(reinterpret_cast<const void*>(covat_expand_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)expand_lds));

  InterpP k{};
  k.Xmode = c->Xmode; k.A = d_A; k.kx = d_kx; k.mean = d_mean;
  k.sG = a.per_trial ? (long long)slab : 0;
  k.p = p; k.T = T; k.T4 = round_up(T, 4); k.T16 = T16; k.Spad = Spad;
  CovAtP g{};
  g.A = d_A; g.kx = d_kx; g.G = lr ? c->Gbin : nullptr; g.V = d_V; g.Q = d_Q; g.cov = d_cov;
  g.sG = k.sG; g.sQ = (long long)(q_rows * CC);
  g.p = p; g.T = T; g.T16 = T16; g.Spad = Spad; g.SB = SB; g.eps = c->eps;
  std::vector<double> h_times;
  std::vector<int> chunk_trials;
  for (int c0 = 0; c0 < N; c0 += chunk) {
    const int nc = std::min(chunk, N - c0);
    if (want_cov) {
      // curvature blocks and the factor of the chunk's slots, as the joint sampler forms them (psample.hip) - with every product on one k loop
      chunk_trials.assign(tos.begin() + c0, tos.begin() + c0 + nc);
      NoSplitK one_k_loop(c);
      CHK(resident_curvature(c, chunk_trials, dual, "posterior", [&](double scale) { return posterior_factor_only(c, nc, scale); }));
    }
    if (a.per_trial) {
      h_times.resize((size_t)nc * S);
      for (int i = 0; i < nc; ++i) std::copy(a.times + (size_t)pos[c0 + i] * S, a.times + (size_t)(pos[c0 + i] + 1) * S, h_times.begin() + (size_t)i * S);
      HIPC(hipMemcpyAsync(d_times, h_times.data(), h_times.size() * sizeof(double), hipMemcpyHostToDevice, c->st));
      CHK(interp_weights(c, d_times, nc, S, Spad, T16, d_kx, d_A));
    }
    k.ptrial = d_trial + c0;
    if (want_mean) hipLaunchKernelGGL(interp_mean_kernel, dim3((Spad + 255) / 256, p, nc), dim3(256), 0, c->st, k);
    HIPC(hipGetLastError());
    for (int s0 = 0; want_cov && s0 < Spad; s0 += SB) {
      const int nsb = std::min(SB, Spad - s0);
      g.s0 = s0; g.nsb = nsb;
      // The products below stay off the split-K path - a fixed 64-tile and a one-level batch declared as the low half of a two-level one -: the number
      // of k parts there follows the number of tiles, i.e. the chunk and the block, and the bits of a trial's covariance must not.
      if (lr) {
        hipLaunchKernelGGL(covat_expand_kernel, dim3((T + COVAT_BT - 1) / COVAT_BT, nc), dim3(256), expand_lds, c->st, g);
        HIPC(hipGetLastError());
        // W^T = V_j^T F_j per latent: the rr[j] rank rows the latent owns (columns of F_j past its rank are zero)
        for (int j = 0; j < p; ++j) {
          GemmP f{};
          f.A = d_V + (size_t)j * T16 * CC; f.sA = (long long)((size_t)p * T16 * CC); f.lda = (int)CC;
          f.B = c->Flr + (size_t)j * c->Tp * c->Tp; f.sB = 0; f.ldb = c->Tp;
          f.C = d_W + (size_t)c->roff[j] * CC; f.sC = (long long)((size_t)rpad * CC); f.ldc = (int)CC;
          f.M = (int)CC; f.N = c->rr[j]; f.K = T16; f.alpha = 1.0; f.beta = 0.0;
          f.slots = c->ident; f.nbatch = nc; f.nb_lo = nc; f.mode = GEMM_FULL; f.kflags = 0; f.bm = 64;
          CHK(gemm(c, true, f));
        }
        // Q^T = W^T L^-T (the triangle is the second operand's: no k range of the kernel's follows it)
        GemmP u{};
        u.A = d_W; u.sA = (long long)((size_t)rpad * CC); u.lda = (int)CC;
        u.B = c->ws.Mt; u.sB = c->ws.sM; u.ldb = rpad;
        u.C = d_Q; u.sC = g.sQ; u.ldc = (int)CC;
        u.M = (int)CC; u.N = rpad; u.K = rpad; u.alpha = 1.0; u.beta = 0.0;
        u.slots = c->ident; u.nbatch = nc; u.nb_lo = nc; u.mode = GEMM_FULL; u.kflags = 0; u.bm = 64;
        CHK(gemm(c, true, u));
        g.rows = round_up(c->rtot, COVAT_IC);
      } else {
        // Q_k^T = a_k^T (rows k T .. of L^-T): only latent k's rows multiply a_k.  The k loop runs over T16 rows from r0 = min(k T, npad - T16) on -
        // the rows before k T meet the zero rows t >= T of latent k - 1's weights - and the columns before r0 are zero (L^-T is upper triangular).
        for (int kk = 0; kk < p; ++kk) {
          const int r0 = std::min(kk * T, npad - T16), shift = kk * T - r0, j0 = r0 / 64 * 64;
          GemmP e{};
          e.A = d_A + (size_t)kk * T16 * Spad + s0 - (size_t)shift * Spad; e.sA = a.per_trial ? (long long)slab : 0; e.lda = Spad;
          e.B = c->ws.Mt + r0 + (size_t)j0 * c->ld; e.sB = c->ws.sM; e.ldb = c->ld;
          e.C = d_Q + (size_t)j0 * CC + (size_t)kk * SB; e.sC = g.sQ; e.ldc = (int)CC;
          e.M = nsb; e.N = npad - j0; e.K = T16; e.alpha = 1.0; e.beta = 0.0;
          e.slots = c->ident; e.nbatch = nc; e.nb_lo = nc; e.mode = GEMM_FULL; e.kflags = 0; e.bm = 64;
          CHK(gemm(c, true, e));
        }
        g.rows = round_up(c->n, COVAT_IC);
      }
      // (pgpfa_create holds p <= 32: the two forms cover every context)
      if (p <= 16) hipLaunchKernelGGL(covat_gram_kernel<1>, dim3(nsb / 16, nc), dim3(256), 0, c->st, g);
      else hipLaunchKernelGGL(covat_gram_kernel<2>, dim3(nsb / 16, nc), dim3(256), 0, c->st, g);
      HIPC(hipGetLastError());
    }
    if (want_rates) CHK(rates_staged_planes(c, "pgpfa_posterior_cov_at", d_mean, d_cov, Spad, nc, d_eta, d_var));
    // results of the chunk, by list position
    for (int i = 0; i < nc; ++i) {
      const size_t ps = (size_t)pos[c0 + i];
      const size_t row = (size_t)S * sizeof(double), prow = (size_t)Spad * sizeof(double);
      if (a.mean) HIPC(hipMemcpy2DAsync(a.mean + ps * p * S, row, d_mean + (size_t)i * p * Spad, prow, row, p, hipMemcpyDeviceToHost, c->st));
      if (a.cov) HIPC(hipMemcpyAsync(a.cov + ps * S * pp, d_cov + (size_t)i * Spad * pp, (size_t)S * pp * sizeof(double), hipMemcpyDeviceToHost, c->st));
      if (a.eta) HIPC(hipMemcpy2DAsync(a.eta + ps * q * S, row, d_eta + (size_t)i * q * Spad, prow, row, q, hipMemcpyDeviceToHost, c->st));
      if (a.var) HIPC(hipMemcpy2DAsync(a.var + ps * q * S, row, d_var + (size_t)i * q * Spad, prow, row, q, hipMemcpyDeviceToHost, c->st));
    }
    HIPC(hipStreamSynchronize(c->st));                         // the staging is reused by the next chunk
    HIPC(hipGetLastError());
  }
  return 0;
}

}  // namespace

int pgpfa_posterior_cov_at(pgpfa_ctx* c, int n, const int32_t* idx, int S, const double* times_ms, int per_trial, double* mean, double* cov, double* eta,
                           double* var) {
  if (!c) return fail("null context");
  if (S < 1) return fail("pgpfa_posterior_cov_at: S = %d, at least one query time is needed", S);
  if (!mean && !cov && !eta && !var) return fail("pgpfa_posterior_cov_at: no output asked for (mean, cov, eta and var are all NULL)");
  if (!times_ms) return fail("pgpfa_posterior_cov_at: times_ms is NULL");
  Trials tr;
  CHK(resolve_trials(c, n, idx, &tr));
  const int N = (int)tr.v.size();
  for (int i = 0; i < (per_trial ? N : 1); ++i)
    for (int s = 0; s < S; ++s)
      if (!std::isfinite(times_ms[(size_t)i * S + s])) {
        if (per_trial) return fail("pgpfa_posterior_cov_at: query time %d of list entry %d (trial %d) is not finite", s, i, tr.v[i]);
        return fail("pgpfa_posterior_cov_at: query time %d is not finite", s);
      }
  if (!c->have_params) return fail("set_params has not been called");
  if (c->tau_inflight) return fail("a timescale pass is in flight (pgpfa_mstep_tau_costgrad_multi_begin): collect it first");
  HIPC(hipSetDevice(c->device));
  // the sampler's predicate (RESIDENT_SAMPLABLE), with texts of this call's own for the two ways a trial misses it
  for (int t : tr.v) {
    if (c->trial_snap[t] >= 0) continue;
    if (c->mode_serial[t] < 0 && !c->vsmgp_ok[t])
      return fail("no posterior for trial %d: no E-step has written one since its counts were uploaded", t);
    return fail("the posterior of trial %d was uploaded with pgpfa_set_posterior: only its blocks are known, it has no square root, and the cross-latent "
                "covariance needs one (a posterior an E-step or pgpfa_dual_finalize of this context wrote)", t);
  }
  CHK(require_resident(c, tr.v, RESIDENT_SAMPLABLE));
  for (int t : tr.v)
    if (c->trial_dual[t] && c->live.length(t) < c->T)
      return fail("the variational posterior of trial %d covers %d of %d bins: its jitter comes from the trial's own %d-bin Gram inverse, so the padded grid "
                  "does not carry its prior conditional; pgpfa_posterior_cov_at refuses rather than approximates", t, c->live.length(t), c->T, c->live.length(t));
  CovAtArgs a{};
  a.trials = &tr.v; a.S = S; a.times = times_ms; a.per_trial = per_trial != 0; a.mean = mean; a.cov = cov; a.eta = eta; a.var = var;
  return for_snapshot_groups(c, tr.v, [&](const std::vector<int>& pos, bool dual) { return covat_group(c, a, pos, dual); });
}
