// libpgpfa_hip.so - query.hip (one translation unit of the C-ABI library; shared declarations: ctx.h, query.h): what the posterior queries share on the
// host - no kernel is launched here and no kernel header included
#include "query.h"

using namespace pgpfa;

int for_snapshot_groups(pgpfa_ctx* c, const std::vector<int>& trials, const std::function<int(const std::vector<int>& positions, bool dual)>& fn) {
  std::map<std::pair<int, int>, std::vector<int>> groups;
  for (size_t i = 0; i < trials.size(); ++i) groups[std::make_pair(c->trial_snap[trials[i]], (int)c->trial_dual[trials[i]])].push_back((int)i);
  for (auto& kv : groups) {
    const std::vector<int>& pos = kv.second;
    const bool dual = kv.first.second != 0;
    CHK(with_snapshot(c, kv.first.first, [&]() { return fn(pos, dual); }));
  }
  return 0;
}

int require_resident(const pgpfa_ctx* c, const std::vector<int>& trials, ResidentKind kind) {
  for (int t : trials) {
    if (kind == RESIDENT_BLOCKS && c->mode_serial[t] < 0 && c->trial_snap[t] < 0 && !c->vsmgp_ok[t])
      return fail("no posterior for trial %d: neither an E-step nor pgpfa_set_posterior has written one since its counts were uploaded", t);
    if (kind == RESIDENT_SAMPLABLE && (c->trial_snap[t] < 0 || (c->trial_dual[t] && !c->lam_keep)))
      return fail("no posterior to sample for trial %d: no E-step has written one since its counts were uploaded (a posterior given by pgpfa_set_posterior "
                  "cannot be sampled, only its blocks are known)", t);
  }
  return 0;
}

int query_gate(pgpfa_ctx* c, const char* entry, const std::vector<int>& trials, const char* root_need) {
  if (!c->have_params) return fail("set_params has not been called");
  if (c->tau_inflight) return fail("a timescale pass is in flight (pgpfa_mstep_tau_costgrad_multi_begin): collect it first");
  HIPC(hipSetDevice(c->device));
  if (root_need) for (int t : trials) {
    if (c->trial_snap[t] >= 0) continue;
    if (c->mode_serial[t] < 0 && !c->vsmgp_ok[t])
      return fail("no posterior for trial %d: no E-step has written one since its counts were uploaded", t);
    return fail("the posterior of trial %d was uploaded with pgpfa_set_posterior: only its blocks are known, it has no square root, and %s needs one (a "
                "posterior an E-step or pgpfa_dual_finalize of this context wrote)", t, root_need);
  }
  CHK(require_resident(c, trials, root_need ? RESIDENT_SAMPLABLE : RESIDENT_BLOCKS));
  for (int t : trials)
    if (c->trial_dual[t] && c->live.length(t) < c->T)
      return fail("the variational posterior of trial %d covers %d of %d bins: its jitter comes from the trial's own %d-bin Gram inverse, so the padded grid "
                  "does not carry its prior conditional; %s refuses rather than approximates", t, c->live.length(t), c->T, c->live.length(t), entry);
  return 0;
}

int check_query_times(const char* entry, const double* times, int S, bool per_trial, const std::vector<int>& trials) {
  for (size_t i = 0; i < (per_trial ? trials.size() : 1); ++i)
    for (int s = 0; s < S; ++s)
      if (!std::isfinite(times[i * S + s])) {
        if (per_trial) return fail("%s: query time %d of list entry %d (trial %d) is not finite", entry, s, (int)i, trials[i]);
        return fail("%s: query time %d is not finite", entry, s);
      }
  return 0;
}

std::vector<int> group_trials(const std::vector<int>& trials, const std::vector<int>& pos) {
  std::vector<int> tos(pos.size());
  for (size_t i = 0; i < pos.size(); ++i) tos[i] = trials[pos[i]];
  return tos;
}

int ready_root(pgpfa_ctx* c, bool dual) {
  CHK(ready_estep(c, dual ? c->dual_lowrank : true));
  return dual ? ensure_lambda(c) : 0;
}

int lds_opt_in(const void* kernel, size_t lds) {
  if (lds > ((size_t)48 << 10)) HIPC(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  return 0;
}

int download_plane(pgpfa_ctx* c, double* host, const double* dev, int rows, int S, int Spad) {
  HIPC(hipMemcpy2DAsync(host, (size_t)S * sizeof(double), dev, (size_t)Spad * sizeof(double), (size_t)S * sizeof(double), rows, hipMemcpyDeviceToHost, c->st));
  return 0;
}

int TimeGrids::upload_shared() {
  HIPC(hipMemcpyAsync(d, times, (size_t)S * sizeof(double), hipMemcpyHostToDevice, c->st));
  return 0;
}

int TimeGrids::upload_listed(const int* pos, int nc) {
  h.resize((size_t)nc * S);
  for (int i = 0; i < nc; ++i) std::copy(times + (size_t)pos[i] * S, times + (size_t)(pos[i] + 1) * S, h.begin() + (size_t)i * S);
  HIPC(hipMemcpyAsync(d, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, c->st));
  return 0;
}

int weight_slabs(pgpfa_ctx* c, DevBufs& dev, size_t len, double** kx, double** A) {
  CHK(dev.get(kx, len));
  CHK(dev.get(A, len));
  HIPC(hipMemsetAsync(*kx, 0, len * sizeof(double), c->st));
  HIPC(hipMemsetAsync(*A, 0, len * sizeof(double), c->st));
  return 0;
}

int RootStage::alloc(DevBufs& dev, size_t col_stride, int chunk) {
  CW = col_stride;
  CHK(dev.get(&Q, (size_t)chunk * q_rows * CW));
  HIPC(hipMemsetAsync(Q, 0, (size_t)chunk * q_rows * CW * sizeof(double), c->st));                   // dense engine: the rows no product writes stay zero
  if (!lr) return 0;
  const size_t v_len = (size_t)chunk * c->p * round_up(c->T, 16) * CW + GEMM_ROW_SLACK, w_len = (size_t)chunk * c->rpad * CW + GEMM_ROW_SLACK;
  CHK(dev.get(&V, v_len));
  CHK(dev.get(&W, w_len));
  HIPC(hipMemsetAsync(V, 0, v_len * sizeof(double), c->st));                                        // rows t >= T stay zero for the whole call
  HIPC(hipMemsetAsync(W, 0, w_len * sizeof(double), c->st));                                        // so do the rank rows no latent owns
  return 0;
}

int RootStage::factor(const std::vector<int>& tos, int c0, int nc, bool dual) {
  const std::vector<int> chunk_trials(tos.begin() + c0, tos.begin() + c0 + nc);
  NoSplitK one_k_loop(c);
  return resident_curvature(c, chunk_trials, dual, "posterior", [&](double scale) { return posterior_factor_only(c, nc, scale); });
}

GemmP RootStage::batch(int nc) const {
  GemmP g{};
  g.alpha = 1.0; g.beta = 0.0; g.slots = c->ident; g.nbatch = nc; g.nb_lo = nc; g.mode = GEMM_FULL; g.kflags = 0; g.bm = 64;
  return g;
}

int RootStage::products(int nc, size_t col0, int ncols) {
  const int T16 = round_up(c->T, 16), rpad = c->rpad;
  // W^T = V_k^T F_k per latent: the rr[k] rank rows the latent owns (columns of F_k past its rank are zero)
  for (int k = 0; k < c->p; ++k) {
    GemmP f = batch(nc);
    f.A = V + (size_t)k * T16 * CW + col0; f.sA = (long long)((size_t)c->p * T16 * CW); f.lda = (int)CW;
    f.B = c->Flr + (size_t)k * c->Tp * c->Tp; f.sB = 0; f.ldb = c->Tp;
    f.C = W + (size_t)c->roff[k] * CW + col0; f.sC = (long long)((size_t)rpad * CW); f.ldc = (int)CW;
    f.M = ncols; f.N = c->rr[k]; f.K = T16;
    CHK(gemm(c, true, f));
  }
  // Q^T = W^T L^-T (the triangle is the second operand's: no k range of the kernel's follows it)
  GemmP u = batch(nc);
  u.A = W + col0; u.sA = (long long)((size_t)rpad * CW); u.lda = (int)CW;
  u.B = c->ws.Mt; u.sB = c->ws.sM; u.ldb = rpad;
  u.C = Q + col0; u.sC = sQ(); u.ldc = (int)CW;
  u.M = ncols; u.N = rpad; u.K = rpad;
  return gemm(c, true, u);
}
