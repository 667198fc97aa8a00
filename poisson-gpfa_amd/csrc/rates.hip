// libpgpfa_hip.so - rates.hip (one translation unit of the C-ABI library; shared declarations: ctx.h): posterior firing rates
#include "query.h"
#include "rates.h"
#include "counts.h"

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

// ---- what pgpfa_posterior_rates and pgpfa_posterior_counts share: eta / var of a chunk of the list staged on the device by rates_kernel ----------
struct RatesGeom { int P4, KS, qpad, nbt_w, nbt; size_t lds; };

RatesGeom rates_geom(const pgpfa_ctx* c) {
  const int p = c->p;
  RatesGeom g{};
  const int NP4 = round_up(p * (p + 1) / 2, 4);
  g.P4 = round_up(p, 4); g.KS = (g.P4 + NP4) / 4; g.qpad = round_up(c->q, 16);
  g.nbt_w = rates_nbt(g.KS);
  const int BT = 16 * g.nbt_w;
  g.nbt = (c->T + BT - 1) / BT;
  g.lds = (size_t)4 * g.KS * rates_row_stride(BT) * sizeof(double) + (size_t)p * p * sizeof(int);
  return g;
}

// the table of this parameter set (its own buffer, kept with the context)
int rates_table(pgpfa_ctx* c, const RatesGeom& g, const char* entry) {
  if (!c->rates_tbl) {
    if (c->arena_mode) return fail("internal: %s inside a workspace plan", entry);
    CHK(dmalloc(c, &c->rates_tbl, (size_t)g.KS * g.qpad * 4));
    c->rates_tbl_params = -1.0;
  }
  if (c->rates_tbl_params != c->info["set_params_calls"]) {
    hipLaunchKernelGGL(rates_table_kernel, dim3(g.qpad / 16), dim3(64), 0, c->st, c->C, c->q, c->p, g.P4, g.KS, g.qpad, c->rates_tbl);
    HIPC(hipGetLastError());
    c->rates_tbl_params = c->info["set_params_calls"];
  }
  return 0;
}

// the arguments of rates_kernel that do not depend on the call's outputs or chunk
RatesP rates_args(const pgpfa_ctx* c, const RatesGeom& g, const int* d_trial) {
  RatesP a{};
  a.Xmode = c->Xmode; a.vsm = c->vsm; a.tbl = c->rates_tbl; a.d = c->d; a.Y = c->Y; a.Yhi = c->Yhi; a.len = c->live.lengths();
  a.ptrial = d_trial;
  a.q = c->q; a.p = c->p; a.T = c->T; a.P4 = g.P4; a.KS = g.KS; a.qpad = g.qpad; a.nbt = g.nbt;
  return a;
}

int rates_launch_chunk(pgpfa_ctx* c, const RatesP& a, const RatesGeom& g, bool grouped, int items) {
  switch (g.nbt_w) {
    case 4: CHK(rates_launch<4>(c, a, grouped, items, g.lds)); break;
    case 2: CHK(rates_launch<2>(c, a, grouped, items, g.lds)); break;
    default: CHK(rates_launch<1>(c, a, grouped, items, g.lds)); break;
  }
  HIPC(hipGetLastError());
  return 0;
}

}  // namespace

// eta / var of `nslots` staged planes - mean [nslots][p][Tplane], cov [nslots][Tplane][p][p], device - into eta / var [nslots][q][Tplane] (either may be
// NULL): rates_kernel with the planes in place of Xmode / vsm, Tplane bins, every bin live, slot z the item z (pgpfa_posterior_cov_at, covat.hip)
int rates_staged_planes(pgpfa_ctx* c, const char* entry, const double* mean, const double* cov, int Tplane, int nslots, double* eta, double* var) {
  RatesGeom geo = rates_geom(c);
  geo.nbt = (Tplane + 16 * geo.nbt_w - 1) / (16 * geo.nbt_w);
  CHK(rates_table(c, geo, entry));
  RatesP a = rates_args(c, geo, c->ident);
  a.Xmode = mean; a.vsm = cov; a.len = nullptr; a.T = Tplane;
  a.eta = eta; a.var = var; a.c0 = 0;
  return rates_launch_chunk(c, a, geo, false, nslots);
}

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
  const int N = (int)tr.v.size(), q = c->q, T = c->T;
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

  const RatesGeom geo = rates_geom(c);
  const int nbt = geo.nbt;
  CHK(rates_table(c, geo, "pgpfa_posterior_rates"));

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

  RatesP a = rates_args(c, geo, d_trial);
  a.ipos = d_pos;
  a.eta = d_eta; a.var = d_var; a.ellp = d_ellp; a.gsum = d_gsum;
  for (int ci = 0; ci < nchunks; ++ci) {
    const int c0 = ci * chunk, nc = std::min(N, c0 + chunk) - c0;
    a.c0 = c0;
    a.istart = grouped ? d_start + (size_t)ci * (n_groups + 1) : nullptr;
    const int items = grouped ? n_groups : nc;
    // (without a table item z of the launch is position c0 + z: the kernel adds c0 to the item)
    CHK(rates_launch_chunk(c, a, geo, grouped, items));
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

namespace {

// ---- predictive counts -----------------------------------------------------------------------------------------------------------------------
// Nodes and log weights of the Q-node Gauss-Hermite rule (weight e^{-x^2}), what numpy.polynomial.hermite.hermgauss returns: the roots of H_Q as the
// eigenvalues of the Jacobi matrix (zero diagonal, off-diagonal sqrt(i / 2)) by bisection on its Sturm count, two Newton steps on the orthonormal
// recurrence, w = 1 / (Q pt_{Q-1}(x)^2).  The positive half is computed and mirrored.  out: [2][Q], x ascending | log w.
void gauss_hermite(int Q, double* out) {
  auto below = [&](double x) {                               // roots below x
    int cnt = 0;
    double d = -x;
    if (d < 0.0) ++cnt;
    for (int i = 1; i < Q; ++i) {
      if (d == 0.0) d = 1e-300;
      d = -x - 0.5 * i / d;
      if (d < 0.0) ++cnt;
    }
    return cnt;
  };
  auto ortho = [&](double x, double* pm1) {                  // pt_Q(x), pt_{Q-1}(x)
    double p0 = 0.7511255444649425, p1 = 0.0;                // pi^(-1/4)
    for (int j = 0; j < Q; ++j) {
      const double p2 = p1;
      p1 = p0;
      p0 = x * std::sqrt(2.0 / (j + 1)) * p1 - std::sqrt((double)j / (j + 1)) * p2;
    }
    *pm1 = p1;
    return p0;
  };
  const double R = std::sqrt(2.0 * Q + 1.0);
  for (int i = Q / 2; i < Q; ++i) {                          // root i (ascending) is >= 0
    double x = 0.0, pm1 = 0.0;
    if (!(Q % 2 == 1 && i == Q / 2)) {
      double lo = 0.0, hi = R;
      for (int it = 0; it < 80; ++it) {
        const double mid = 0.5 * (lo + hi);
        if (below(mid) > i) hi = mid; else lo = mid;
      }
      x = 0.5 * (lo + hi);
      for (int it = 0; it < 2; ++it) {
        const double pq = ortho(x, &pm1);
        x -= pq / (std::sqrt(2.0 * Q) * pm1);
      }
    }
    ortho(x, &pm1);
    const double lw = -std::log((double)Q) - 2.0 * std::log(std::fabs(pm1));
    out[i] = x; out[Q - 1 - i] = -x;
    out[Q + i] = lw; out[Q + Q - 1 - i] = lw;
  }
}

int counts_nodes(pgpfa_ctx* c, const char* entry) {
  if (!c->counts_nodes) {
    if (c->arena_mode) return fail("internal: %s inside a workspace plan", entry);
    CHK(dmalloc(c, &c->counts_nodes, (size_t)2 * 64));
    c->counts_nodes_Q = 0;
  }
  if (c->counts_nodes_Q != c->counts_Q) {
    std::vector<double> h((size_t)2 * c->counts_Q);
    gauss_hermite(c->counts_Q, h.data());
    HIPC(hipMemcpyAsync(c->counts_nodes, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, c->st));
    HIPC(hipStreamSynchronize(c->st));                       // (h leaves scope)
    c->counts_nodes_Q = c->counts_Q;
  }
  return 0;
}

struct CountsOut { double* logp; double* pmf; int32_t* lower; int32_t* upper; double* pmean; double* pvar; };

// the argument checks of the two entry points, in one place
int counts_check(const char* entry, const CountsOut& o, int K, double level, int k_cap) {
  if (!o.logp && !o.pmf && !o.lower && !o.upper && !o.pmean && !o.pvar) return fail("%s: no output asked for", entry);
  if (o.pmf && (K < 1 || K > 1024)) return fail("%s: K = %d, pmf holds 1 .. 1024 counts per entry", entry, K);
  if ((o.lower || o.upper) && !(level > 0.0 && level < 1.0)) return fail("%s: level = %g must lie strictly between 0 and 1", entry, level);
  if ((o.lower || o.upper) && (k_cap < 0 || k_cap > 65535)) return fail("%s: k_cap = %d is outside 0 .. 65535", entry, k_cap);
  return 0;
}

int counts_check_range(const char* entry, const int32_t* counts, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (counts[i] < 0 || counts[i] > 65535) return fail("%s: count %d of entry %zu is outside 0 .. 65535", entry, (int)counts[i], i);
  return 0;
}

// device outputs of one chunk of `cap` entries, the launch on `ne` of them and the copies to host offset `e0`; *saturated grows by the chunk's count
struct CountsDev {
  double *logp = nullptr, *pmf = nullptr, *pmean = nullptr, *pvar = nullptr;
  int32_t *lower = nullptr, *upper = nullptr, *sat = nullptr, *counts = nullptr;
  std::vector<int32_t> h_sat;
};

size_t counts_bytes_per_entry(const CountsOut& o, bool counts_given, int K) {
  return (counts_given ? 4 : 0) + (o.logp ? 8 : 0) + (o.pmf ? (size_t)8 * K : 0) + (o.lower ? 4 : 0) + (o.upper ? 4 : 0) + (o.pmean ? 8 : 0) + (o.pvar ? 8 : 0);
}

int counts_alloc(DevBufs& dev, CountsDev* d, const CountsOut& o, bool counts_given, int K, size_t cap) {
  if (counts_given) CHK(dev.get(&d->counts, cap));
  if (o.logp) CHK(dev.get(&d->logp, cap));
  if (o.pmf) CHK(dev.get(&d->pmf, cap * K));
  if (o.lower) CHK(dev.get(&d->lower, cap));
  if (o.upper) CHK(dev.get(&d->upper, cap));
  if (o.pmean) CHK(dev.get(&d->pmean, cap));
  if (o.pvar) CHK(dev.get(&d->pvar, cap));
  if (o.lower || o.upper) { CHK(dev.get(&d->sat, (cap + 63) / 64)); d->h_sat.resize((cap + 63) / 64); }
  return 0;
}

// a: m, v, the tables and c0 set by the caller.  Ends with the stream synchronised: the staging is reused by the next chunk.
int counts_run(pgpfa_ctx* c, CountsP a, CountsDev& d, const CountsOut& o, const int32_t* counts, size_t e0, size_t ne, int K, double level, int k_cap,
               long long* saturated) {
  const size_t nblk = (ne + 63) / 64;
  if (counts) HIPC(hipMemcpyAsync(d.counts, counts + e0, ne * sizeof(int32_t), hipMemcpyHostToDevice, c->st));
  a.counts = counts ? d.counts : nullptr;
  a.nodes = c->counts_nodes; a.Q = c->counts_nodes_Q;
  a.logp = d.logp; a.pmf = d.pmf; a.lower = d.lower; a.upper = d.upper; a.pmean = d.pmean; a.pvar = d.pvar; a.sat = d.sat;
  a.n = (long long)ne; a.K = K; a.k_cap = k_cap; a.p_lo = 0.5 * (1.0 - level); a.p_hi = 0.5 * (1.0 + level);
  hipLaunchKernelGGL(counts_kernel, dim3((unsigned)nblk), dim3(64), 0, c->st, a);
  HIPC(hipGetLastError());
  if (o.logp) HIPC(hipMemcpyAsync(o.logp + e0, d.logp, ne * sizeof(double), hipMemcpyDeviceToHost, c->st));
  if (o.pmf) HIPC(hipMemcpyAsync(o.pmf + e0 * K, d.pmf, ne * K * sizeof(double), hipMemcpyDeviceToHost, c->st));
  if (o.lower) HIPC(hipMemcpyAsync(o.lower + e0, d.lower, ne * sizeof(int32_t), hipMemcpyDeviceToHost, c->st));
  if (o.upper) HIPC(hipMemcpyAsync(o.upper + e0, d.upper, ne * sizeof(int32_t), hipMemcpyDeviceToHost, c->st));
  if (o.pmean) HIPC(hipMemcpyAsync(o.pmean + e0, d.pmean, ne * sizeof(double), hipMemcpyDeviceToHost, c->st));
  if (o.pvar) HIPC(hipMemcpyAsync(o.pvar + e0, d.pvar, ne * sizeof(double), hipMemcpyDeviceToHost, c->st));
  if (d.sat) HIPC(hipMemcpyAsync(d.h_sat.data(), d.sat, nblk * sizeof(int32_t), hipMemcpyDeviceToHost, c->st));
  HIPC(hipStreamSynchronize(c->st));
  HIPC(hipGetLastError());
  if (d.sat) for (size_t b = 0; b < nblk; ++b) *saturated += d.h_sat[b];
  return 0;
}

}  // namespace

int pgpfa_count_probabilities(pgpfa_ctx* c, long long n_entries, const double* m, const double* v, const int32_t* counts, int K, double level, int k_cap,
                              double* logp, double* pmf, int32_t* lower, int32_t* upper, double* pmean, double* pvar) {
  const char* entry = "pgpfa_count_probabilities";
  if (!c) return fail("null context");
  const CountsOut o{logp, pmf, lower, upper, pmean, pvar};
  CHK(counts_check(entry, o, K, level, k_cap));
  if (n_entries < 1 || !m || !v) return fail("%s: invalid argument", entry);
  if (logp && !counts) return fail("%s: logp needs the count of every entry", entry);
  const size_t n = (size_t)n_entries;
  if (counts && logp) CHK(counts_check_range(entry, counts, n));
  HIPC(hipSetDevice(c->device));
  CHK(counts_nodes(c, entry));
  // chunks of entries (whole workgroups): the staging of a chunk stays within the bound of the queries
  const size_t per_entry = 16 + counts_bytes_per_entry(o, counts && logp, K);
  const size_t cap = std::min(n, std::max<size_t>(64, QUERY_STAGE_BYTES / per_entry / 64 * 64));
  DevBufs dev(entry);
  CountsDev d;
  double *d_m = nullptr, *d_v = nullptr;
  CHK(dev.get(&d_m, cap));
  CHK(dev.get(&d_v, cap));
  CHK(counts_alloc(dev, &d, o, counts && logp, K, cap));
  long long saturated = 0;
  for (size_t e0 = 0; e0 < n; e0 += cap) {
    const size_t ne = std::min(n, e0 + cap) - e0;
    HIPC(hipMemcpyAsync(d_m, m + e0, ne * sizeof(double), hipMemcpyHostToDevice, c->st));
    HIPC(hipMemcpyAsync(d_v, v + e0, ne * sizeof(double), hipMemcpyHostToDevice, c->st));
    CountsP a{};
    a.m = d_m; a.v = d_v;
    CHK(counts_run(c, a, d, o, logp ? counts : nullptr, e0, ne, K, level, k_cap, &saturated));
  }
  c->info["counts_saturated"] = (double)saturated;
  return 0;
}

int pgpfa_posterior_counts(pgpfa_ctx* c, int n, const int32_t* idx, const int32_t* counts, int K, double level, int k_cap,
                           double* logp, double* pmf, int32_t* lower, int32_t* upper, double* pmean, double* pvar) {
  const char* entry = "pgpfa_posterior_counts";
  if (!c) return fail("null context");
  const CountsOut o{logp, pmf, lower, upper, pmean, pvar};
  CHK(counts_check(entry, o, K, level, k_cap));
  if (!c->have_params) return fail("set_params has not been called");
  if (logp && !counts && !c->have_counts) return fail("spike counts have not been uploaded: logp without a counts array reads them");
  if (logp && !counts && c->live.words())
    return fail("%s: logp at the resident counts is not available under a per-bin table: the resident counts at entries that were not recorded are "
                "placeholders (pass the counts)", entry);
  HIPC(hipSetDevice(c->device));
  Trials tr;
  CHK(resolve_trials(c, n, idx, &tr));
  const int N = (int)tr.v.size(), q = c->q, T = c->T;
  CHK(require_resident(c, tr.v, RESIDENT_BLOCKS));
  const size_t qT = (size_t)q * T;
  if (counts && logp) CHK(counts_check_range(entry, counts, (size_t)N * qT));

  const RatesGeom geo = rates_geom(c);
  CHK(rates_table(c, geo, entry));
  CHK(counts_nodes(c, entry));
  const size_t per_trial = qT * (16 + counts_bytes_per_entry(o, counts && logp, K));
  const int chunk = query_chunk((size_t)N, c->counts_chunk, per_trial);

  DevBufs dev(entry);
  CountsDev d;
  int* d_trial = nullptr;
  double *d_eta = nullptr, *d_var = nullptr;
  CHK(dev.get(&d_trial, (size_t)N));
  CHK(dev.get(&d_eta, (size_t)chunk * qT));
  CHK(dev.get(&d_var, (size_t)chunk * qT));
  CHK(counts_alloc(dev, &d, o, counts && logp, K, (size_t)chunk * qT));
  HIPC(hipMemcpyAsync(d_trial, tr.v.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice, c->st));

  RatesP ra = rates_args(c, geo, d_trial);
  ra.eta = d_eta; ra.var = d_var;
  CountsP a{};
  a.m = d_eta; a.v = d_var; a.Y = c->Y; a.Yhi = c->Yhi; a.len = c->live.lengths(); a.ptrial = d_trial; a.q = q; a.T = T;
  long long saturated = 0;
  for (int c0 = 0; c0 < N; c0 += chunk) {
    const int nc = std::min(N, c0 + chunk) - c0;
    ra.c0 = c0;
    CHK(rates_launch_chunk(c, ra, geo, false, nc));          // eta, var of the chunk: staged, never copied to the host
    a.c0 = c0;
    CHK(counts_run(c, a, d, o, logp ? counts : nullptr, (size_t)c0 * qT, (size_t)nc * qT, K, level, k_cap, &saturated));
  }
  c->info["counts_saturated"] = (double)saturated;
  return 0;
}
