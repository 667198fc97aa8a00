// libpgpfa_hip.so - velat.hip (one translation unit of the C-ABI library; shared declarations: ctx.h, query.h): value and velocity of every latent at
// arbitrary time points, with their joint 2 x 2 posterior (pgpfa_posterior_velocity_at)
#include "query.h"
#include "interp.h"
#include "velat.h"

using namespace pgpfa;

namespace {

struct VelArgs {
  const std::vector<int>* trials;     // trial of every list position
  int S; const double* times; bool per_trial;
  double* out[5];                     // mean, var, vel, vel_var, cross
};
enum { O_MEAN, O_VAR, O_VEL, O_VELVAR, O_CROSS, O_COUNT };

// the positions `pos` of the list (one snapshot, one kind of posterior), under that snapshot's parameters
int velat_group(pgpfa_ctx* c, const VelArgs& a, const std::vector<int>& pos) {
  const int p = c->p, T = c->T, S = a.S;
  const int T4 = round_up(T, 4), T16 = round_up(T, 16), Spad = round_up(S, 16), VS = interp_row_stride(T4);
  const bool joint = a.out[O_VAR] || a.out[O_VELVAR] || a.out[O_CROSS];       // the pass over V: all three forms or none
  const bool need_A = a.out[O_MEAN] || joint, need_B = a.out[O_VEL] || joint;
  // the time block: as many query times as leave room for the panel, halved from VELAT_SBLK down to one tile (no output depends on it)
  int sblk = VELAT_SBLK;
  while (sblk > 16 && ((size_t)16 * VS + (size_t)3 * std::min(Spad, sblk)) * sizeof(double) > QUERY_LDS_MAX) sblk /= 2;
  const size_t lds = ((size_t)16 * VS + (size_t)3 * std::min(Spad, sblk)) * sizeof(double);
  if (joint && lds > QUERY_LDS_MAX)
    return fail("pgpfa_posterior_velocity_at: a row panel of %d bins does not fit the LDS of a compute unit (%zu bytes)", T, lds);
  const int N = (int)pos.size();
  const std::vector<int> tos = group_trials(*a.trials, pos);

  DevBufs dev("pgpfa_posterior_velocity_at");
  MarkKeeper keep{c, {}};
  if (joint) CHK(interp_blocks_resident(c, dev, keep, tos));

  // chunks of the group: device staging per trial (per-trial cross Grams, weights, results)
  const size_t slab = (size_t)p * T16 * Spad;
  int nout = 0;
  for (int o = 0; o < O_COUNT; ++o) nout += a.out[o] ? 1 : 0;
  const int nslab = 2 * ((need_A ? 1 : 0) + (need_B ? 1 : 0));
  const size_t per_trial = (size_t)nout * p * Spad * sizeof(double) + (a.per_trial ? (nslab * slab + S) * sizeof(double) : 0);
  const int chunk = query_chunk((size_t)N, c->velat_chunk, per_trial);
  const int grids = a.per_trial ? chunk : 1;
  const size_t wlen = (size_t)grids * slab + GEMM_ROW_SLACK;

  TimeGrids tg{c, a.times, S};
  double *d_kx = nullptr, *d_A = nullptr, *d_kd = nullptr, *d_B = nullptr, *d_out[O_COUNT] = {};
  int* d_trial = nullptr;
  CHK(tg.alloc(dev, grids));
  CHK(dev.get(&d_trial, (size_t)N));
  if (need_A) CHK(weight_slabs(c, dev, wlen, &d_kx, &d_A));
  if (need_B) CHK(weight_slabs(c, dev, wlen, &d_kd, &d_B));
  for (int o = 0; o < O_COUNT; ++o)
    if (a.out[o]) CHK(dev.get(&d_out[o], (size_t)chunk * p * Spad));
  HIPC(hipMemcpyAsync(d_trial, tos.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice, c->st));

  // kx, A and kd, B of `ng` grids whose times are in tg.d
  auto weights = [&](int ng) -> int {
    if (need_A) CHK(interp_weights(c, tg.d, ng, S, Spad, T16, d_kx, d_A));
    if (need_B) {
      hipLaunchKernelGGL(velat_cross_kernel, dim3(T16, p, ng), dim3(256), 0, c->st, tg.d, c->tau, c->bin, c->eps, T, T16, S, Spad, p, d_kd);
      HIPC(hipGetLastError());
      CHK(interp_solve(c, d_kd, ng, Spad, T16, d_B));
    }
    return 0;
  };
  if (!a.per_trial) {
    CHK(tg.upload_shared());
    CHK(weights(1));                                          // once per snapshot group, not per trial
  }
  if (joint) CHK(lds_opt_in(reinterpret_cast<const void*>(velat_joint_kernel), lds));

  const long long sG = a.per_trial ? (long long)slab : 0;
  InterpP km{};                                               // interp_mean_kernel on A (mean) and on B (vel)
  km.Xmode = c->Xmode; km.sG = sG; km.p = p; km.T = T; km.T4 = T4; km.T16 = T16; km.Spad = Spad; km.VS = VS;
  VelatP k{};
  k.vsmgp = c->vsmgp; k.A = d_A; k.B = d_B; k.kx = d_kx; k.kd = d_kd; k.tau = c->tau; k.eps = c->eps;
  k.var = d_out[O_VAR]; k.vel_var = d_out[O_VELVAR]; k.cross = d_out[O_CROSS];
  k.sG = sG; k.p = p; k.T = T; k.T4 = T4; k.T16 = T16; k.Spad = Spad; k.VS = VS; k.sblk = sblk;
  for (int c0 = 0; c0 < N; c0 += chunk) {
    const int nc = std::min(chunk, N - c0);
    if (a.per_trial) {
      CHK(tg.upload_listed(pos.data() + c0, nc));
      CHK(weights(nc));
    }
    km.ptrial = k.ptrial = d_trial + c0;
    if (a.out[O_MEAN]) {
      km.A = d_A; km.mean = d_out[O_MEAN];
      hipLaunchKernelGGL(interp_mean_kernel, dim3((Spad + 255) / 256, p, nc), dim3(256), 0, c->st, km);
    }
    if (a.out[O_VEL]) {
      km.A = d_B; km.mean = d_out[O_VEL];
      hipLaunchKernelGGL(interp_mean_kernel, dim3((Spad + 255) / 256, p, nc), dim3(256), 0, c->st, km);
    }
    if (joint) hipLaunchKernelGGL(velat_joint_kernel, dim3((Spad + sblk - 1) / sblk, p, nc), dim3(256), lds, c->st, k);
    HIPC(hipGetLastError());
    // results of the chunk, by list position
    for (int i = 0; i < nc; ++i) {
      const size_t ps = (size_t)pos[c0 + i];
      for (int o = 0; o < O_COUNT; ++o)
        if (a.out[o]) CHK(download_plane(c, a.out[o] + ps * p * S, d_out[o] + (size_t)i * p * Spad, p, S, Spad));
    }
    HIPC(hipStreamSynchronize(c->st));                         // the staging is reused by the next chunk
    HIPC(hipGetLastError());
  }
  return 0;
}

}  // namespace

int pgpfa_posterior_velocity_at(pgpfa_ctx* c, int n, const int32_t* idx, int S, const double* times_ms, int per_trial, double* mean, double* var, double* vel,
                                double* vel_var, double* cross) {
  if (!c) return fail("null context");
  if (S < 1) return fail("pgpfa_posterior_velocity_at: S = %d, at least one query time is needed", S);
  if (!mean && !var && !vel && !vel_var && !cross) return fail("pgpfa_posterior_velocity_at: no output asked for (mean, var, vel, vel_var and cross are all NULL)");
  if (!times_ms) return fail("pgpfa_posterior_velocity_at: times_ms is NULL");
  Trials tr;
  CHK(resolve_trials(c, n, idx, &tr));
  CHK(check_query_times("pgpfa_posterior_velocity_at", times_ms, S, per_trial != 0, tr.v));
  CHK(query_gate(c, "pgpfa_posterior_velocity_at", tr.v));
  VelArgs a{};
  a.trials = &tr.v; a.S = S; a.times = times_ms; a.per_trial = per_trial != 0;
  a.out[O_MEAN] = mean; a.out[O_VAR] = var; a.out[O_VEL] = vel; a.out[O_VELVAR] = vel_var; a.out[O_CROSS] = cross;
  return for_snapshot_groups(c, tr.v, [&](const std::vector<int>& pos, bool) { return velat_group(c, a, pos); });
}
