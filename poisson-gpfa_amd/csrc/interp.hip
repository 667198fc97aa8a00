// libpgpfa_hip.so - interp.hip (one translation unit of the C-ABI library; shared declarations: ctx.h, query.h): the latent posterior at arbitrary time
// points (pgpfa_posterior_at)
#include "query.h"
#include "interp.h"

using namespace pgpfa;

int interp_weights(pgpfa_ctx* c, const double* d_times, int grids, int S, int Spad, int T16, double* kx, double* A) {
  const int p = c->p, T = c->T;
  hipLaunchKernelGGL(interp_cross_kernel, dim3(T16, p, grids), dim3(256), 0, c->st, d_times, c->tau, c->bin, c->eps, T, T16, S, Spad, p, kx);
  HIPC(hipGetLastError());
  return interp_solve(c, kx, grids, Spad, T16, A);
}

int interp_solve(pgpfa_ctx* c, const double* rhs, int grids, int Spad, int T16, double* A) {
  const int p = c->p, T = c->T;
  // A[t][s] = sum_u Kinv[t][u] kx[u][s]: column-major C (Spad x T, ld Spad) = kx (Spad x T16) Kinv^T.  Kinv is the identity in its padding and the
  // rows u >= T of kx are zero.  The batch is declared as the low half of a two-level one (latents below, grids above) and the tile is fixed, which
  // keeps the launch off the split-K path: the bits of a trial's weights must not follow the number of grids in a chunk.
  const long long slab = (long long)T16 * Spad;
  GemmP g{};
  g.A = rhs; g.sA = slab; g.lda = Spad;
  g.B = c->Kinv; g.sB = (long long)c->Tp * c->Tp; g.ldb = c->Tp;
  g.C = A; g.sC = slab; g.ldc = Spad;
  g.M = Spad; g.N = T; g.K = T16; g.alpha = 1.0; g.beta = 0.0;
  g.slots = nullptr; g.nb_lo = p; g.nbatch = p * grids; g.sA_hi = (long long)p * slab; g.sB_hi = 0; g.sC_hi = (long long)p * slab;
  g.mode = GEMM_FULL; g.kflags = 0; g.bm = 64;
  return gemm(c, false, g);
}

int interp_blocks_resident(pgpfa_ctx* c, DevBufs& dev, MarkKeeper& keep, const std::vector<int>& tos) {
  const int p = c->p, T = c->T;
  CHK(ensure_vsmgp_buffer(c));
  // blocks rebuilt on demand under the sum-only plan (same snapshot, so no parameter switch).  The rebuild also rewrites post_vsm of those trials
  // - by another kernel than the sum-only E-step, so not to the bit: their post_vsm is set aside and put back, and so are the resident marks
  std::vector<int> rebuilt;
  for (int t : tos) {
    keep.saved.emplace_back(t, c->vsmgp_ok[t]);
    if (!c->vsmgp_ok[t] && std::find(rebuilt.begin(), rebuilt.end(), t) == rebuilt.end()) rebuilt.push_back(t);
  }
  if (!rebuilt.empty()) {
    const size_t lv = (size_t)T * p * p;
    double* d_vsm = nullptr;
    CHK(dev.get(&d_vsm, rebuilt.size() * lv));
    for (size_t i = 0; i < rebuilt.size(); ++i)
      HIPC(hipMemcpyAsync(d_vsm + i * lv, c->vsm + (size_t)rebuilt[i] * lv, lv * sizeof(double), hipMemcpyDeviceToDevice, c->st));
    const int rc = ensure_trial_vsmgp(c, tos);
    for (size_t i = 0; i < rebuilt.size(); ++i)
      HIPC(hipMemcpyAsync(c->vsm + (size_t)rebuilt[i] * lv, d_vsm + i * lv, lv * sizeof(double), hipMemcpyDeviceToDevice, c->st));
    CHK(rc);
  }
  return 0;
}

namespace {

struct AtArgs {
  const std::vector<int>* trials;     // trial of every list position
  int S; const double* times; bool per_trial;
  double* mean; double* var;
};

// the positions `pos` of the list (one snapshot, one kind of posterior), under that snapshot's parameters
int at_group(pgpfa_ctx* c, const AtArgs& a, const std::vector<int>& pos) {
  const int p = c->p, T = c->T, S = a.S;
  const int T4 = round_up(T, 4), T16 = round_up(T, 16), Spad = round_up(S, 16), VS = interp_row_stride(T4);
  const size_t lds = ((size_t)16 * VS + std::min(Spad, INTERP_SBLK)) * sizeof(double);
  if (a.var && lds > QUERY_LDS_MAX) return fail("pgpfa_posterior_at: a row panel of %d bins does not fit the LDS of a compute unit (%zu bytes)", T, lds);
  const int N = (int)pos.size();
  const std::vector<int> tos = group_trials(*a.trials, pos);

  DevBufs dev("pgpfa_posterior_at");
  MarkKeeper keep{c, {}};
  if (a.var) CHK(interp_blocks_resident(c, dev, keep, tos));

  // chunks of the group: device staging per trial (per-trial cross Grams, weights, results)
  const size_t slab = (size_t)p * T16 * Spad;
  const size_t per_trial = ((a.mean ? 1 : 0) + (a.var ? 1 : 0)) * (size_t)p * Spad * sizeof(double) + (a.per_trial ? (2 * slab + S) * sizeof(double) : 0);
  const int chunk = query_chunk((size_t)N, c->interp_chunk, per_trial);
  const int grids = a.per_trial ? chunk : 1;

  TimeGrids tg{c, a.times, S};
  double *d_kx = nullptr, *d_A = nullptr, *d_mean = nullptr, *d_var = nullptr;
  int* d_trial = nullptr;
  CHK(tg.alloc(dev, grids));
  CHK(weight_slabs(c, dev, (size_t)grids * slab + GEMM_ROW_SLACK, &d_kx, &d_A));
  CHK(dev.get(&d_trial, (size_t)N));
  if (a.mean) CHK(dev.get(&d_mean, (size_t)chunk * p * Spad));
  if (a.var) CHK(dev.get(&d_var, (size_t)chunk * p * Spad));
  HIPC(hipMemcpyAsync(d_trial, tos.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice, c->st));
  if (!a.per_trial) {
    CHK(tg.upload_shared());
    CHK(interp_weights(c, tg.d, 1, S, Spad, T16, d_kx, d_A));   // once per snapshot group, not per trial
  }
  if (a.var) CHK(lds_opt_in(reinterpret_cast<const void*>(interp_var_kernel), lds));

  InterpP k{};
  k.vsmgp = c->vsmgp; k.Xmode = c->Xmode; k.A = d_A; k.kx = d_kx; k.mean = d_mean; k.var = d_var;
  k.sG = a.per_trial ? (long long)slab : 0;
  k.p = p; k.T = T; k.T4 = T4; k.T16 = T16; k.Spad = Spad; k.VS = VS;
  for (int c0 = 0; c0 < N; c0 += chunk) {
    const int nc = std::min(chunk, N - c0);
    if (a.per_trial) {
      CHK(tg.upload_listed(pos.data() + c0, nc));
      CHK(interp_weights(c, tg.d, nc, S, Spad, T16, d_kx, d_A));
    }
    k.ptrial = d_trial + c0;
    if (a.mean) hipLaunchKernelGGL(interp_mean_kernel, dim3((Spad + 255) / 256, p, nc), dim3(256), 0, c->st, k);
    if (a.var) hipLaunchKernelGGL(interp_var_kernel, dim3((Spad + INTERP_SBLK - 1) / INTERP_SBLK, p, nc), dim3(256), lds, c->st, k);
    HIPC(hipGetLastError());
    // results of the chunk, by list position
    for (int i = 0; i < nc; ++i) {
      const size_t ps = (size_t)pos[c0 + i];
      if (a.mean) CHK(download_plane(c, a.mean + ps * p * S, d_mean + (size_t)i * p * Spad, p, S, Spad));
      if (a.var) CHK(download_plane(c, a.var + ps * p * S, d_var + (size_t)i * p * Spad, p, S, Spad));
    }
    HIPC(hipStreamSynchronize(c->st));                         // the staging is reused by the next chunk
    HIPC(hipGetLastError());
  }
  return 0;
}

}  // namespace

int pgpfa_posterior_at(pgpfa_ctx* c, int n, const int32_t* idx, int S, const double* times_ms, int per_trial, double* mean, double* var) {
  if (!c) return fail("null context");
  if (S < 1) return fail("pgpfa_posterior_at: S = %d, at least one query time is needed", S);
  if (!mean && !var) return fail("pgpfa_posterior_at: no output asked for (mean and var are both NULL)");
  if (!times_ms) return fail("pgpfa_posterior_at: times_ms is NULL");
  Trials tr;
  CHK(resolve_trials(c, n, idx, &tr));
  CHK(check_query_times("pgpfa_posterior_at", times_ms, S, per_trial != 0, tr.v));
  CHK(query_gate(c, "pgpfa_posterior_at", tr.v));
  AtArgs a{};
  a.trials = &tr.v; a.S = S; a.times = times_ms; a.per_trial = per_trial != 0; a.mean = mean; a.var = var;
  return for_snapshot_groups(c, tr.v, [&](const std::vector<int>& pos, bool) { return at_group(c, a, pos); });
}
