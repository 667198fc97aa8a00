// Importance weights of the Laplace posterior's own draws (pgpfa_importance_weights): for x_s = x* + delta_s ~ N(x*, H^-1) of a trial,
//   log p(y, x_s) - log N(x_s; x*, H^-1) = log Z_Laplace + log w_s,
//   log w_s = - sum_{(n,t) live} lambda*_nt phi(a_snt),   lambda*_nt = exp(d_n + c_n . x*_t),  a_snt = c_n . delta_st,  phi(a) = e^a - 1 - a - a^2 / 2
// The prior is quadratic and cancels against the Gaussian; its first-order rest cancels the likelihood's gradient at a stationary mode, counts
// included - so the sum is likelihood-local: no K^-1, no counts, no pT x pT object.  A residual gradient g at x* would add
// - g . delta_s, which is ignored.
// impw_kernel forms the partial sums per (slot, sample, tile of 16 bins) on v_mfma_f64_16x16x4_f64 with the maps of psample_counts_kernel
// (psample.h); impw_reduce_kernel adds the tiles of a draw in tile order and forms the per-slot log mean weight and effective sample size.  No
// atomics: log w of draw s is a pure function of (trajectory, parameters, live tables) - no list position, chunk or sample count enters.
#pragma once

namespace pgpfa {

constexpr int IMPW_NS = 8;                                    // draws a workgroup carries through one walk of the neuron tiles

struct ImpwP {
  const double* X;         // [nslots][S][p][T]: the draws the sampler left
  const double* Xmode;     // [R][p][T]
  const double* C;         // [q][p]
  const double* d;         // [q]
  const int* len;          // [R] or NULL (LiveTables::fill)
  const uint8_t* obs;      // OBS == 1: [R][q] bytes; OBS == 2: the bit words of the per-bin table (bin_words, model.h); else not read
  const int* trial_of_slot;
  double* part;            // [nslots][S][ntile]: sum over the tile's live entries of lambda* phi(a)
  int S, q, p, T, ntile;
};

// phi(a) = e^a - 1 - a - a^2 / 2 (expm1: the leading cancellation is done inside the library function).  +inf when e^a overflows.
__device__ __forceinline__ double impw_phi(double a) { return (expm1(a) - a) - 0.5 * a * a; }

// dynamic LDS of impw_kernel: the draws' deviations from the mode for the tile, [NS][4 KS][16], and the waves' sums [4][NS]
__host__ __device__ constexpr size_t impw_lds(int p) { return ((size_t)IMPW_NS * ((p + 3) / 4) * 64 + 4 * IMPW_NS) * sizeof(double); }

// grid = (ntile, ceil(S / NS), nslots), block = 256, dynamic LDS impw_lds(p).  A workgroup owns 16 bins of a slot and NS consecutive draws.
// Operand maps of psample_counts_kernel: first operand of lane (l15, l4) = C[n0 + l15][4 ks + l4], second = z[4 ks + l4][t0 + l15], accumulator
// register r = neuron n0 + 4 r + l4, bin t0 + l15.  Wave w takes the neuron tiles w, w + 4, ...: per tile it keeps the loading fragments in
// registers, forms h* = C x* + d and lambda* = exp(h*) ONCE (second operand: the mode's fragment, in registers for the whole walk) and then runs the
// NS draws against it - second operand delta = x_s - x* from LDS, written there once per workgroup straight from the trajectory with the bins along
// the lanes (a lane's read address is its lane index: no bank conflict) - applying lambda* phi(a) on the accumulator registers.
// Entries that are not live - padded bins, unobserved rows, dead entries of a per-bin table, rows past q, bins past T - are selected out, never
// multiplied out: whatever C, d hold there, they add exactly 0.  Sums: lanes by butterfly, then the four waves in order.
template <int OBS>
__global__ __launch_bounds__(256) void impw_kernel(ImpwP a) {
  constexpr int NS = IMPW_NS;
  extern __shared__ double impw_sm[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, l4 = lane >> 4;
  const int q = a.q, p = a.p, T = a.T, KS = (p + 3) >> 2;
  double* dl = impw_sm;                                       // [NS][4 KS][16]
  double* red = impw_sm + (size_t)NS * KS * 64;               // [4][NS]
  const int tile = blockIdx.x, s0 = blockIdx.y * NS, slot = blockIdx.z;
  const int t0 = tile * 16, t = t0 + l15;
  const int trial = a.trial_of_slot[slot];
  const int Tr = a.len ? a.len[trial] : T;
  const int ns = min(NS, a.S - s0);
  double* out = a.part + ((size_t)slot * a.S + s0) * a.ntile + tile;
  if (t0 >= Tr) {                                             // (uniform over the workgroup) a tile of padded bins: no entry is live
    if (threadIdx.x < ns) out[(size_t)threadIdx.x * a.ntile] = 0.0;
    return;
  }
  const double* xm_g = a.Xmode + (size_t)trial * p * T;
  // delta of the workgroup's draws: element e = (u, k, b), b fastest - 16 consecutive bins of one latent per 16 lanes
  for (int e = threadIdx.x; e < NS * KS * 64; e += 256) {
    const int b = e & 15, k = (e >> 4) % (4 * KS), u = (e >> 4) / (4 * KS);
    double v = 0.0;
    if (u < ns && k < p && t0 + b < T) {
      const size_t o = (size_t)k * T + t0 + b;
      v = a.X[((size_t)slot * a.S + s0 + u) * p * T + o] - xm_g[o];
    }
    dl[e] = v;
  }
  double xm[8];
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) {
    const int k = 4 * ks + l4;
    xm[ks] = (ks < KS && k < p && t < T) ? xm_g[(size_t)k * T + t] : 0.0;
  }
  __syncthreads();

  const uint8_t* ob = OBS == 1 ? a.obs + (size_t)trial * q : nullptr;
  const int nw = (T + 63) >> 6;
  const unsigned long long* bw = OBS == 2 ? reinterpret_cast<const unsigned long long*>(a.obs) + (size_t)trial * (q + 1) * nw + (t0 >> 6) : nullptr;
  double sum[NS];
#pragma unroll
  for (int u = 0; u < NS; ++u) sum[u] = 0.0;
  for (int n0 = wave * 16; n0 < q; n0 += 64) {
    double cf[8];
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      const int k = 4 * ks + l4;
      cf[ks] = (ks < KS && k < p && n0 + l15 < q) ? a.C[(size_t)(n0 + l15) * p + k] : 0.0;
    }
    double4_t h = double4_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int ks = 0; ks < 8; ++ks)
      if (ks < KS) h = __builtin_amdgcn_mfma_f64_16x16x4f64(cf[ks], xm[ks], h, 0, 0, 0);
    double lam[4];
    bool live[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = n0 + 4 * r + l4;
      const int nc = n < q ? n : q - 1;                        // (clamped: the loads below stay inside the tables)
      bool lv = n < q && t < Tr;
      if constexpr (OBS == 1) lv = lv && ob[nc] != 0;
      if constexpr (OBS == 2) lv = lv && ((bw[(size_t)nc * nw] >> (t0 & 63)) >> l15 & 1ull) != 0;
      live[r] = lv;
      lam[r] = lv ? exp(h[r] + a.d[nc]) : 0.0;
    }
    bool any = live[0] || live[1] || live[2] || live[3];
    if (!__any(any)) continue;                                 // (uniform over the wave) a neuron tile without a live entry in these bins
#pragma unroll
    for (int u = 0; u < NS; ++u) {
      if (u < ns) {                                            // (uniform)
        double4_t acc = double4_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int ks = 0; ks < 8; ++ks)
          if (ks < KS) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(cf[ks], dl[(u * 4 * KS + 4 * ks + l4) * 16 + l15], acc, 0, 0, 0);
        double v = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) v += live[r] ? lam[r] * impw_phi(acc[r]) : 0.0;
        sum[u] += v;
      }
    }
  }
#pragma unroll
  for (int u = 0; u < NS; ++u) {
    double v = sum[u];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if (lane == 0) red[wave * NS + u] = v;
  }
  __syncthreads();
  if (threadIdx.x < ns) {
    const int u = threadIdx.x;
    out[(size_t)u * a.ntile] = ((red[u] + red[NS + u]) + red[2 * NS + u]) + red[3 * NS + u];
  }
}

// log_w[slot][s] = - (sum of the draw's tiles, in tile order); then per slot, by one thread and with the draws in index order,
//   log_ratio = m + log((1 / S) sum_s exp(log w_s - m)),  m = max_s log w_s        ess = (sum_s e_s)^2 / sum_s e_s^2,  e_s = exp(log w_s - m)
// (every weight zero: log_ratio = -inf, ess = 0).  bad[slot] is set when a log weight is NaN.  grid = nslots, block = 256.
inline __global__ __launch_bounds__(256) void impw_reduce_kernel(const double* __restrict__ part, int S, int ntile, double* log_w,
                                                                 double* __restrict__ log_ratio, double* __restrict__ ess, int* __restrict__ bad) {
  const int slot = blockIdx.x;
  double* lw = log_w + (size_t)slot * S;
  for (int s = threadIdx.x; s < S; s += 256) {
    const double* ps = part + ((size_t)slot * S + s) * ntile;
    double v = 0.0;
    for (int i = 0; i < ntile; ++i) v += ps[i];
    lw[s] = -v;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double m = -INFINITY;
  bool nan = false;
  for (int s = 0; s < S; ++s) {
    const double v = lw[s];
    nan = nan || v != v;
    m = v > m ? v : m;
  }
  double s1 = 0.0, s2 = 0.0;
  if (m > -INFINITY)
    for (int s = 0; s < S; ++s) {
      const double e = exp(lw[s] - m);
      s1 += e;
      s2 += e * e;
    }
  log_ratio[slot] = m > -INFINITY ? m + log(s1 / (double)S) : -INFINITY;
  ess[slot] = s2 > 0.0 ? s1 * s1 / s2 : 0.0;
  bad[slot] = nan ? 1 : 0;
}

}  // namespace pgpfa
