// libpgpfa_hip.so - rates.hip (one translation unit of the C-ABI library; shared declarations: ctx.h): posterior firing rates
#include "ctx.h"
#include "rates.h"

using namespace pgpfa;

namespace {

// bins per workgroup tile: the largest of 64 / 32 / 16 whose LDS image (4 KS rows of rates_row_stride(BT) doubles) stays within 64 KiB - two workgroups
// per CU -, else 16: 70 KiB at 32 latents, one workgroup per CU
int rates_nbt(int KS) {
  for (int nbt : {4, 2}) if ((size_t)4 * KS * rates_row_stride(16 * nbt) * sizeof(double) <= ((size_t)64 << 10)) return nbt;
  return 1;
}

template <int NBT>
int rates_launch(pgpfa_ctx* c, const RatesP& a, bool grouped, int items, size_t lds) {
  const int ntile = a.qpad / 16;
  const dim3 grid(a.nbt, grouped ? (ntile + 3) / 4 : 1, items);
  auto run = [&](auto kern) -> int {
    if (lds > ((size_t)48 << 10)) HIPC(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, c->st, a);
    return 0;
  };
  if (grouped) return run(rates_kernel<NBT, true>);
  return run(rates_kernel<NBT, false>);
}

}  // namespace

// Host side of the group table: positions of every group in list order, as CSR (start[g] .. start[g + 1] into pos).  first / last bound the positions
// taken (a chunk of the list).  Exported for the host tests: no device is touched.
extern "C" int pgpfa_rates_group_csr(int n, const int32_t* group, int n_groups, int first, int last, int32_t* start /* [n_groups + 1] */, int32_t* pos /* [last - first] */) {
  if (!group || !start || !pos || n < 0 || n_groups < 0 || first < 0 || last > n || first > last) return fail("pgpfa_rates_group_csr: invalid argument");
  for (int i = first; i < last; ++i)
    if (group[i] < 0 || group[i] >= n_groups) return fail("group id %d of list entry %d is outside 0..%d", (int)group[i], i, n_groups - 1);
  std::vector<int> cnt(n_groups + 1, 0);
  for (int i = first; i < last; ++i) ++cnt[group[i] + 1];
  for (int g = 0; g < n_groups; ++g) cnt[g + 1] += cnt[g];
  for (int g = 0; g <= n_groups; ++g) start[g] = cnt[g];
  for (int i = first; i < last; ++i) pos[cnt[group[i]]++] = i;          // (stable: list order inside a group)
  return 0;
}

int pgpfa_posterior_rates(pgpfa_ctx* c, int n, const int32_t* idx, const int32_t* group, int n_groups, double* eta, double* var, double* ell,
                          double* group_sum, int32_t* group_count) {
  if (!c) return fail("null context");
  if (!eta && !var && !ell && !group_sum && !group_count) return fail("pgpfa_posterior_rates: no output asked for");
  if (!c->have_params) return fail("set_params has not been called");
  if (ell && !c->have_counts) return fail("spike counts have not been uploaded: the expected log likelihood reads them");
  if ((group_sum || group_count) && !group) return fail("pgpfa_posterior_rates: a group output needs the trial -> group table");
  if (group && n_groups < 1) return fail("pgpfa_posterior_rates: n_groups = %d with a group table", n_groups);
  HIPC(hipSetDevice(c->device));
  Trials tr;
  CHK(resolve_trials(c, n, idx, &tr));
  const int N = (int)tr.v.size(), q = c->q, p = c->p, T = c->T;
  CHK(require_resident(c, tr.v, RESIDENT_BLOCKS));
  if (group)
    for (int i = 0; i < N; ++i)
      if (group[i] < 0 || group[i] >= n_groups) return fail("group id %d of list entry %d (trial %d) is outside 0..%d", (int)group[i], i, tr.v[i], n_groups - 1);

  if (group_count) {                                          // integers of the two host tables
    std::fill(group_count, group_count + (size_t)n_groups * T, 0);
    for (int i = 0; i < N; ++i) {
      const int Tr = c->live.length(tr.v[i]);
      for (int t = 0; t < Tr; ++t) ++group_count[(size_t)group[i] * T + t];
    }
  }
  if (!eta && !var && !ell && !group_sum) return 0;

  const int P4 = round_up(p, 4), NP4 = round_up(p * (p + 1) / 2, 4), KS = (P4 + NP4) / 4, qpad = round_up(q, 16);
  const int nbt_w = rates_nbt(KS), BT = 16 * nbt_w, nbt = (T + BT - 1) / BT;
  const size_t lds = (size_t)4 * KS * rates_row_stride(BT) * sizeof(double) + (size_t)p * p * sizeof(int);
  // the table of this parameter set (its own buffer, kept with the context)
  if (!c->rates_tbl) {
    if (c->arena_mode) return fail("internal: pgpfa_posterior_rates inside a workspace plan");
    CHK(dmalloc(c, &c->rates_tbl, (size_t)KS * qpad * 4));
    c->rates_tbl_params = -1.0;
  }
  if (c->rates_tbl_params != c->info["set_params_calls"]) {
    hipLaunchKernelGGL(rates_table_kernel, dim3(qpad / 16), dim3(64), 0, c->st, c->C, q, p, P4, KS, qpad, c->rates_tbl);
    HIPC(hipGetLastError());
    c->rates_tbl_params = c->info["set_params_calls"];
  }

  // chunks of the list: the per-trial planes of a chunk are staged on the device
  const size_t plane = (size_t)q * T * sizeof(double);
  const size_t per_trial = ((eta ? 1 : 0) + (var ? 1 : 0)) * plane + (ell ? (size_t)(nbt + 1) * q * sizeof(double) : 0);
  const int chunk = query_chunk((size_t)N, c->rates_chunk, per_trial);

  DevBufs dev("pgpfa_posterior_rates");
  int *d_trial = nullptr, *d_start = nullptr, *d_pos = nullptr;
  double *d_eta = nullptr, *d_var = nullptr, *d_ellp = nullptr, *d_ell = nullptr, *d_gsum = nullptr;
  CHK(dev.get(&d_trial, (size_t)N));
  if (eta) CHK(dev.get(&d_eta, (size_t)chunk * q * T));
  if (var) CHK(dev.get(&d_var, (size_t)chunk * q * T));
  if (ell) { CHK(dev.get(&d_ellp, (size_t)chunk * nbt * q)); CHK(dev.get(&d_ell, (size_t)chunk * q)); }
  const bool grouped = group_sum != nullptr;
  const int nchunks = (N + chunk - 1) / chunk;
  std::vector<int> h_start, h_pos;
  if (grouped) {
    CHK(dev.get(&d_gsum, (size_t)n_groups * q * T));
    HIPC(hipMemsetAsync(d_gsum, 0, (size_t)n_groups * q * T * sizeof(double), c->st));
    h_start.resize((size_t)nchunks * (n_groups + 1));
    h_pos.resize(N);
    for (int ci = 0; ci < nchunks; ++ci) {
      const int c0 = ci * chunk, c1 = std::min(N, c0 + chunk);
      int32_t* st = h_start.data() + (size_t)ci * (n_groups + 1);
      CHK(pgpfa_rates_group_csr(N, group, n_groups, c0, c1, st, h_pos.data() + c0));
      for (int g = 0; g <= n_groups; ++g) st[g] += c0;         // (offsets into the one position array of the call)
    }
    CHK(dev.get(&d_start, h_start.size()));
    CHK(dev.get(&d_pos, (size_t)N));
    HIPC(hipMemcpyAsync(d_start, h_start.data(), h_start.size() * sizeof(int), hipMemcpyHostToDevice, c->st));
    HIPC(hipMemcpyAsync(d_pos, h_pos.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice, c->st));
  }
  HIPC(hipMemcpyAsync(d_trial, tr.v.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice, c->st));

  RatesP a{};
  a.Xmode = c->Xmode; a.vsm = c->vsm; a.tbl = c->rates_tbl; a.d = c->d; a.Y = c->Y; a.Yhi = c->Yhi; a.len = c->live.lengths();
  a.ptrial = d_trial; a.ipos = d_pos;
  a.eta = d_eta; a.var = d_var; a.ellp = d_ellp; a.gsum = d_gsum;
  a.q = q; a.p = p; a.T = T; a.P4 = P4; a.KS = KS; a.qpad = qpad; a.nbt = nbt;
  for (int ci = 0; ci < nchunks; ++ci) {
    const int c0 = ci * chunk, nc = std::min(N, c0 + chunk) - c0;
    a.c0 = c0;
    a.istart = grouped ? d_start + (size_t)ci * (n_groups + 1) : nullptr;
    const int items = grouped ? n_groups : nc;
    // (without a table item z of the launch is position c0 + z: the kernel adds c0 to the item)
    switch (nbt_w) {
      case 4: CHK(rates_launch<4>(c, a, grouped, items, lds)); break;
      case 2: CHK(rates_launch<2>(c, a, grouped, items, lds)); break;
      default: CHK(rates_launch<1>(c, a, grouped, items, lds)); break;
    }
    HIPC(hipGetLastError());
    if (ell) hipLaunchKernelGGL(rates_ell_kernel, dim3((q + 255) / 256, nc), dim3(256), 0, c->st, d_ellp, q, nbt, d_ell);
    if (eta) HIPC(hipMemcpyAsync(eta + (size_t)c0 * q * T, d_eta, (size_t)nc * plane, hipMemcpyDeviceToHost, c->st));
    if (var) HIPC(hipMemcpyAsync(var + (size_t)c0 * q * T, d_var, (size_t)nc * plane, hipMemcpyDeviceToHost, c->st));
    if (ell) HIPC(hipMemcpyAsync(ell + (size_t)c0 * q, d_ell, (size_t)nc * q * sizeof(double), hipMemcpyDeviceToHost, c->st));
    if (eta || var || ell) HIPC(hipStreamSynchronize(c->st));      // the staging is reused by the next chunk
    HIPC(hipGetLastError());
  }
  if (grouped) HIPC(hipMemcpyAsync(group_sum, d_gsum, (size_t)n_groups * q * T * sizeof(double), hipMemcpyDeviceToHost, c->st));
  HIPC(hipStreamSynchronize(c->st));
  HIPC(hipGetLastError());
  return 0;
}
