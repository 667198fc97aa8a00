// libpgpfa_hip.so - pfunc.hip (one translation unit of the C-ABI library; shared declarations: ctx.h, query.h): the joint posterior of linear functionals of a
// trial's latents - epoch means, contrasts, projections (pgpfa_posterior_functionals)
#include "query.h"
#include "pfunc.h"

using namespace pgpfa;

namespace {

struct PFuncArgs {
  const std::vector<int>* trials;     // trial of every list position
  int J; const double* weights; bool per_trial;
  double *mean, *var, *cov;
};

// the positions `pos` of the list (one snapshot, one kind of posterior), under that snapshot's parameters
int pfunc_group(pgpfa_ctx* c, const PFuncArgs& a, const std::vector<int>& pos, bool dual) {
  const bool want_root = a.var || a.cov, want_cov = a.cov != nullptr;
  if (want_root) CHK(ready_root(c, dual));
  const int p = c->p, T = c->T, J = a.J;
  const bool lr = want_root && c->plan_lowrank;
  const int T16 = round_up(T, 16), Jpad = round_up(J, 16);
  const int N = (int)pos.size();
  const std::vector<int> tos = group_trials(*a.trials, pos);

  // The functionals go through the root in blocks of JB columns.  With the J x J plane asked for the staging holds all Jpad columns of a trial - every
  // pair of columns meets in the Gram - and a block is a column range of it; without, the staging is one block wide and is reused block after block.
  const int npad = c->npad;
  RootStage root(c, lr);
  const size_t urows = lr ? (size_t)p * T16 : (size_t)npad;                   // rows of the staged weights
  const size_t q_rows = want_root ? root.q_rows : 0;
  const size_t rows_stage = urows + (lr ? (size_t)p * T16 + 2 * q_rows : q_rows);
  const int JB = plan::query_block_cols(c->func_block, Jpad, rows_stage * sizeof(double), QUERY_STAGE_BYTES);
  const int JW = want_cov ? Jpad : JB;
  const bool restage = !want_cov && JB < Jpad;                                  // the weights of every block are staged when its turn comes
  const size_t planes = (a.mean ? (size_t)J : 0) + (want_root ? (size_t)J : 0) + (want_cov ? (size_t)J * J : 0);
  const size_t trial_bytes = (rows_stage * JW + planes) * sizeof(double);       // (shared weights are staged once: counted with every trial, the bound holds a fortiori)
  const int chunk = query_chunk((size_t)N, c->func_chunk, trial_bytes, want_root ? (size_t)c->B : 0);
  const int sets = a.per_trial ? chunk : 1;

  DevBufs dev("pgpfa_posterior_functionals");
  double *d_U = nullptr, *d_mean = nullptr, *d_var = nullptr, *d_cov = nullptr;
  int* d_trial = nullptr;
  const size_t u_len = (size_t)sets * urows * JW + GEMM_ROW_SLACK;
  CHK(dev.get(&d_U, u_len));
  CHK(dev.get(&d_trial, (size_t)N));
  if (a.mean) CHK(dev.get(&d_mean, (size_t)chunk * J));
  if (want_root) CHK(dev.get(&d_var, (size_t)chunk * J));
  if (want_cov) CHK(dev.get(&d_cov, (size_t)chunk * J * J));
  HIPC(hipMemsetAsync(d_U, 0, u_len * sizeof(double), c->st));
  if (want_root) CHK(root.alloc(dev, (size_t)JW, chunk));
  HIPC(hipMemcpyAsync(d_trial, tos.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice, c->st));
  const size_t expand_lds = (size_t)(p * p + p) / 2 * PFUNC_BT * sizeof(double);
  if (lr) CHK(lds_opt_in(reinterpret_cast<const void*>(pfunc_expand_kernel), expand_lds));

  // The columns jb0 .. jb0 + nj of the weights of `nsets` list positions, transposed into the staging at column col0: [J][p][T] -> [row][JW], every
  // other entry of the image zero.  The image is rebuilt on the host, so the stream is drained before it is touched again.
  std::vector<double> h_U;
  const int lrow = lr ? T16 : T;
  auto stage = [&](const int* positions, int nsets, int jb0, int nj, int col0) -> int {
    HIPC(hipStreamSynchronize(c->st));
    h_U.assign((size_t)nsets * urows * JW, 0.0);
    for (int i = 0; i < nsets; ++i) {
      const double* w = a.weights + (positions ? (size_t)positions[i] * J * p * T : 0);
      double* img = h_U.data() + (size_t)i * urows * JW + col0;
      for (int j = jb0; j < std::min(jb0 + nj, J); ++j)
        for (int k = 0; k < p; ++k)
          for (int t = 0; t < T; ++t) img[((size_t)k * lrow + t) * JW + (j - jb0)] = w[((size_t)j * p + k) * T + t];
    }
    HIPC(hipMemcpyAsync(d_U, h_U.data(), h_U.size() * sizeof(double), hipMemcpyHostToDevice, c->st));
    return 0;
  };
  if (!a.per_trial && !restage) CHK(stage(nullptr, 1, 0, Jpad, 0));            // once per snapshot group, not per trial

  PFuncP g{};
  g.U = d_U; g.Xmode = c->Xmode; g.G = lr ? c->Gbin : nullptr; g.V = root.V; g.Q = root.Q; g.mean = d_mean; g.var = d_var; g.cov = d_cov;
  g.sU = a.per_trial ? (long long)(urows * JW) : 0; g.sQ = root.sQ();
  g.rows = want_root ? root.rows : 0; g.erows = lr ? p * T16 : 0; g.lrow = lrow;
  g.p = p; g.T = T; g.T16 = T16; g.JW = JW; g.J = J; g.eps = c->eps;
  for (int c0 = 0; c0 < N; c0 += chunk) {
    const int nc = std::min(chunk, N - c0);
    if (want_root) CHK(root.factor(tos, c0, nc, dual));
    g.ptrial = d_trial + c0;
    if (a.per_trial && !restage) CHK(stage(pos.data() + c0, nc, 0, Jpad, 0));
    for (int jb0 = 0; jb0 < Jpad; jb0 += JB) {
      const int nj = std::min(JB, Jpad - jb0), col0 = want_cov ? jb0 : 0;
      if (restage) CHK(stage(a.per_trial ? pos.data() + c0 : nullptr, a.per_trial ? nc : 1, jb0, nj, 0));
      g.j0 = col0; g.nj = nj; g.jout = jb0;
      if (a.mean) hipLaunchKernelGGL(pfunc_mean_kernel, dim3((nj + 255) / 256, nc), dim3(256), 0, c->st, g);
      HIPC(hipGetLastError());
      if (!want_root) continue;
      if (lr) {
        hipLaunchKernelGGL(pfunc_expand_kernel, dim3((T + PFUNC_BT - 1) / PFUNC_BT, nc), dim3(256), expand_lds, c->st, g);
        HIPC(hipGetLastError());
        CHK(root.products(nc, (size_t)col0, nj));
      } else {
        // Q^T = U^T L^-T: one product over all npad rows (rows >= p T of U are zero)
        GemmP e = root.batch(nc);
        e.A = d_U + col0; e.sA = g.sU; e.lda = JW;
        e.B = c->ws.Mt; e.sB = c->ws.sM; e.ldb = c->ld;
        e.C = root.Q + col0; e.sC = g.sQ; e.ldc = JW;
        e.M = nj; e.N = npad; e.K = npad;
        CHK(gemm(c, true, e));
      }
      if (!want_cov) {
        hipLaunchKernelGGL(pfunc_gram_kernel<true>, dim3(nj / 16, 1, nc), dim3(256), 0, c->st, g);
        HIPC(hipGetLastError());
      }
    }
    if (want_cov) {
      g.j0 = 0; g.nj = Jpad; g.jout = 0;
      hipLaunchKernelGGL(pfunc_gram_kernel<false>, dim3(Jpad / 16, Jpad / 16, nc), dim3(256), 0, c->st, g);
      HIPC(hipGetLastError());
    }
    // results of the chunk, by list position
    for (int i = 0; i < nc; ++i) {
      const size_t ps = (size_t)pos[c0 + i];
      if (a.mean) HIPC(hipMemcpyAsync(a.mean + ps * J, d_mean + (size_t)i * J, (size_t)J * sizeof(double), hipMemcpyDeviceToHost, c->st));
      if (a.var) HIPC(hipMemcpyAsync(a.var + ps * J, d_var + (size_t)i * J, (size_t)J * sizeof(double), hipMemcpyDeviceToHost, c->st));
      if (a.cov) HIPC(hipMemcpyAsync(a.cov + ps * J * J, d_cov + (size_t)i * J * J, (size_t)J * J * sizeof(double), hipMemcpyDeviceToHost, c->st));
    }
    HIPC(hipStreamSynchronize(c->st));                         // the staging is reused by the next chunk
    HIPC(hipGetLastError());
  }
  return 0;
}

}  // namespace

int pgpfa_posterior_functionals(pgpfa_ctx* c, int n, const int32_t* idx, int J, const double* weights, int per_trial, double* mean, double* var, double* cov) {
  if (!c) return fail("null context");
  if (J < 1) return fail("pgpfa_posterior_functionals: J = %d, at least one functional is needed", J);
  if (!mean && !var && !cov) return fail("pgpfa_posterior_functionals: no output asked for (mean, var and cov are all NULL)");
  if (!weights) return fail("pgpfa_posterior_functionals: weights is NULL");
  if (cov && J > PFUNC_JMAX)
    return fail("pgpfa_posterior_functionals: J = %d with cov asked for, the J x J plane is given for at most %d functionals (var alone has no limit)", J, PFUNC_JMAX);
  Trials tr;
  CHK(resolve_trials(c, n, idx, &tr));
  const int N = (int)tr.v.size();
  const size_t pT = (size_t)c->p * c->T;
  for (int i = 0; i < (per_trial ? N : 1); ++i)
    for (int j = 0; j < J; ++j)
      for (size_t e = 0; e < pT; ++e)
        if (!std::isfinite(weights[((size_t)i * J + j) * pT + e])) {
          const int k = (int)(e / c->T), t = (int)(e % c->T);
          if (per_trial) return fail("pgpfa_posterior_functionals: the weight of functional %d at latent %d, bin %d of list entry %d (trial %d) is not finite", j, k, t, i, tr.v[i]);
          return fail("pgpfa_posterior_functionals: the weight of functional %d at latent %d, bin %d is not finite", j, k, t);
        }
  CHK(query_gate(c, "pgpfa_posterior_functionals", tr.v, "the covariance of a functional"));
  PFuncArgs a{};
  a.trials = &tr.v; a.J = J; a.weights = weights; a.per_trial = per_trial != 0; a.mean = mean; a.var = var; a.cov = cov;
  return for_snapshot_groups(c, tr.v, [&](const std::vector<int>& pos, bool dual) { return pfunc_group(c, a, pos, dual); });
}
