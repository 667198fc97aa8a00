// libpgpfa_hip.so - covat.hip (one translation unit of the C-ABI library; shared declarations: ctx.h, query.h): the cross-latent posterior covariance and
// the log-rate moments at arbitrary time points (pgpfa_posterior_cov_at)
#include "query.h"
#include "interp.h"
#include "covat.h"

using namespace pgpfa;

namespace {

static_assert(COVAT_IC == 8, "covat_gram_kernel steps through the rows of Q that RootStage::rows counts");

struct CovAtArgs {
  const std::vector<int>* trials;     // trial of every list position
  int S; const double* times; bool per_trial;
  double *mean, *cov, *eta, *var;
};

// the positions `pos` of the list (one snapshot, one kind of posterior), under that snapshot's parameters
int covat_group(pgpfa_ctx* c, const CovAtArgs& a, const std::vector<int>& pos, bool dual) {
  // (rates_kernel gathers both planes whichever of eta / var it stores)
  const bool want_rates = a.eta || a.var, want_cov = a.cov || want_rates, want_mean = a.mean || want_rates;
  if (want_cov) CHK(ready_root(c, dual));
  const int p = c->p, q = c->q, T = c->T, S = a.S, pp = p * p;
  const bool lr = want_cov && c->plan_lowrank;
  const int T16 = round_up(T, 16), Spad = round_up(S, 16);
  const int N = (int)pos.size();
  const std::vector<int> tos = group_trials(*a.trials, pos);

  // blocks of query times and chunks of the group: the right-hand sides of a block (p per time, rows_stage doubles each) and the planes of a chunk are
  // staged on the device
  const int npad = c->npad;
  RootStage root(c, lr);
  const size_t rows_stage = !want_cov ? 0 : (lr ? (size_t)p * T16 + 2 * root.q_rows : root.q_rows);
  const int SB = want_cov ? plan::query_block_cols(c->covat_block, Spad, rows_stage * p * sizeof(double), QUERY_STAGE_BYTES) : Spad;
  const size_t CC = (size_t)p * SB;
  const size_t slab = (size_t)p * T16 * Spad;
  const size_t planes = (want_mean ? (size_t)p * Spad : 0) + (want_cov ? (size_t)Spad * pp : 0) + ((a.eta ? 1 : 0) + (a.var ? 1 : 0)) * (size_t)q * Spad;
  const size_t per_trial = (rows_stage * CC + planes + (a.per_trial ? 2 * slab + S : 0)) * sizeof(double);
  const int chunk = query_chunk((size_t)N, c->covat_chunk, per_trial, want_cov ? (size_t)c->B : 0);
  const int grids = a.per_trial ? chunk : 1;

  DevBufs dev("pgpfa_posterior_cov_at");
  TimeGrids tg{c, a.times, S};
  double *d_kx = nullptr, *d_A = nullptr, *d_mean = nullptr, *d_cov = nullptr, *d_eta = nullptr, *d_var = nullptr;
  int* d_trial = nullptr;
  CHK(tg.alloc(dev, grids));
  CHK(weight_slabs(c, dev, (size_t)grids * slab + GEMM_ROW_SLACK, &d_kx, &d_A));
  CHK(dev.get(&d_trial, (size_t)N));
  if (want_mean) CHK(dev.get(&d_mean, (size_t)chunk * p * Spad));
  if (want_cov) CHK(dev.get(&d_cov, (size_t)chunk * Spad * pp));
  if (a.eta) CHK(dev.get(&d_eta, (size_t)chunk * q * Spad));
  if (a.var) CHK(dev.get(&d_var, (size_t)chunk * q * Spad));
  if (want_cov) CHK(root.alloc(dev, CC, chunk));
  HIPC(hipMemcpyAsync(d_trial, tos.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice, c->st));
  if (!a.per_trial) {
    CHK(tg.upload_shared());
    CHK(interp_weights(c, tg.d, 1, S, Spad, T16, d_kx, d_A));   // once per snapshot group, not per trial
  }
  const size_t expand_lds = (size_t)(pp + p) / 2 * COVAT_BT * sizeof(double);
  if (lr) CHK(lds_opt_in(reinterpret_cast<const void*>(covat_expand_kernel), expand_lds));

  InterpP k{};
  k.Xmode = c->Xmode; k.A = d_A; k.kx = d_kx; k.mean = d_mean;
  k.sG = a.per_trial ? (long long)slab : 0;
  k.p = p; k.T = T; k.T4 = round_up(T, 4); k.T16 = T16; k.Spad = Spad;
  CovAtP g{};
  g.A = d_A; g.kx = d_kx; g.G = lr ? c->Gbin : nullptr; g.V = root.V; g.Q = root.Q; g.cov = d_cov;
  g.sG = k.sG; g.sQ = root.sQ(); g.rows = root.rows;
  g.p = p; g.T = T; g.T16 = T16; g.Spad = Spad; g.SB = SB; g.eps = c->eps;
  for (int c0 = 0; c0 < N; c0 += chunk) {
    const int nc = std::min(chunk, N - c0);
    if (want_cov) CHK(root.factor(tos, c0, nc, dual));
    if (a.per_trial) {
      CHK(tg.upload_listed(pos.data() + c0, nc));
      CHK(interp_weights(c, tg.d, nc, S, Spad, T16, d_kx, d_A));
    }
    k.ptrial = d_trial + c0;
    if (want_mean) hipLaunchKernelGGL(interp_mean_kernel, dim3((Spad + 255) / 256, p, nc), dim3(256), 0, c->st, k);
    HIPC(hipGetLastError());
    for (int s0 = 0; want_cov && s0 < Spad; s0 += SB) {
      const int nsb = std::min(SB, Spad - s0);
      g.s0 = s0; g.nsb = nsb;
      if (lr) {
        hipLaunchKernelGGL(covat_expand_kernel, dim3((T + COVAT_BT - 1) / COVAT_BT, nc), dim3(256), expand_lds, c->st, g);
        HIPC(hipGetLastError());
        CHK(root.products(nc, 0, (int)CC));
      } else {
        // Q_k^T = a_k^T (rows k T .. of L^-T): only latent k's rows multiply a_k.  The k loop runs over T16 rows from r0 = min(k T, npad - T16) on -
        // the rows before k T meet the zero rows t >= T of latent k - 1's weights - and the columns before r0 are zero (L^-T is upper triangular).
        for (int kk = 0; kk < p; ++kk) {
          const int r0 = std::min(kk * T, npad - T16), shift = kk * T - r0, j0 = r0 / 64 * 64;
          GemmP e = root.batch(nc);
          e.A = d_A + (size_t)kk * T16 * Spad + s0 - (size_t)shift * Spad; e.sA = a.per_trial ? (long long)slab : 0; e.lda = Spad;
          e.B = c->ws.Mt + r0 + (size_t)j0 * c->ld; e.sB = c->ws.sM; e.ldb = c->ld;
          e.C = root.Q + (size_t)j0 * CC + (size_t)kk * SB; e.sC = g.sQ; e.ldc = (int)CC;
          e.M = nsb; e.N = npad - j0; e.K = T16;
          CHK(gemm(c, true, e));
        }
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
      if (a.mean) CHK(download_plane(c, a.mean + ps * p * S, d_mean + (size_t)i * p * Spad, p, S, Spad));
      if (a.cov) HIPC(hipMemcpyAsync(a.cov + ps * S * pp, d_cov + (size_t)i * Spad * pp, (size_t)S * pp * sizeof(double), hipMemcpyDeviceToHost, c->st));
      if (a.eta) CHK(download_plane(c, a.eta + ps * q * S, d_eta + (size_t)i * q * Spad, q, S, Spad));
      if (a.var) CHK(download_plane(c, a.var + ps * q * S, d_var + (size_t)i * q * Spad, q, S, Spad));
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
  CHK(check_query_times("pgpfa_posterior_cov_at", times_ms, S, per_trial != 0, tr.v));
  CHK(query_gate(c, "pgpfa_posterior_cov_at", tr.v, "the cross-latent covariance"));
  CovAtArgs a{};
  a.trials = &tr.v; a.S = S; a.times = times_ms; a.per_trial = per_trial != 0; a.mean = mean; a.cov = cov; a.eta = eta; a.var = var;
  return for_snapshot_groups(c, tr.v, [&](const std::vector<int>& pos, bool dual) { return covat_group(c, a, pos, dual); });
}
