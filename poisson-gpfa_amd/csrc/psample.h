// Joint posterior samples (pgpfa_posterior_sample): draws x ~ N(m, Sigma) of whole trajectories from a square root of Sigma that the covariance
// engines build anyway, and posterior-predictive spike counts y ~ Poisson(exp(d + C x)) of every draw.
//   low-rank engine   Sigma = eps G + (G F L^-T)(G F L^-T)^T  (G = (I + eps W)^-1 per bin, B = I + F^T Wt F = L L^T), so
//                     x = m + G (F (L^-T z2)) + sqrt(eps) chol(G) z1     with z1 (p T) and z2 (rtot) standard normal
//   dense engine      H = L L^T, x = m + L^-T z
// The two products U = L^-T Z2 and Yv = F U are the library's batched GEMM (psample.hip); the kernels here draw the normals, mix the bins
// (psample_mix_kernel), add the mean (dense engine) and turn trajectories into counts (psample_counts_kernel).
// Normals: Philox4x32-10 of sample.h, counter (element pair, trial, sample, stream) with stream 4 = z1 and 5 = z2 (pgpfa_generate uses 1..3), key = seed: a
// normal is a pure function of (seed, trial, sample, element, stream) - no list position, chunk, launch geometry or sample count enters.
// Counts: poisson_draw of sample.h under a key derived per sample (a Philox output of (sample, stream 6) under the seed), counters (trial, neuron, bin).
#pragma once

namespace pgpfa {

constexpr unsigned PS_STREAM_Z1 = 4u, PS_STREAM_Z2 = 5u, PS_STREAM_KEY = 6u;

// Z[(slot * S + s) * ldz + e] for e < len: grid = (S nblk, nslots) with nblk = ceil(len / 512), block = 256.  A thread draws one pair (both halves of a
// Box-Muller transform) for the elements 2 j, 2 j + 1.
inline __global__ __launch_bounds__(256) void psample_noise_kernel(double* __restrict__ Z, long long ldz, int len, int S, int nblk, unsigned long long seed,
                                                                   unsigned stream, const int* __restrict__ trial_of_slot) {
  const unsigned s = blockIdx.x / nblk;
  const int j = (blockIdx.x - s * nblk) * 256 + threadIdx.x;
  if (2 * j >= len) return;
  const unsigned trial = (unsigned)trial_of_slot[blockIdx.y];
  const Philox rng{(unsigned)seed, (unsigned)(seed >> 32)};
  unsigned w[4];
  rng((unsigned)j, trial, s, stream, w);
  double a, b;
  normal2(w, a, b);
  double* z = Z + ((size_t)blockIdx.y * S + s) * ldz;
  z[2 * j] = a;
  if (2 * j + 1 < len) z[2 * j + 1] = b;
}

// bins per workgroup tile of the mixing kernel: the packed triangles of G_t and R_t = chol(G_t) of a tile live in LDS as [pair][bin] (2 NP BT doubles,
// NP = PW (PW + 1) / 2): 64 bins up to 10 latents (55 KiB), 32 up to 16 (68 KiB), 16 beyond (20: 53 KiB, 32: 132 KiB of the CU's 160)
__host__ __device__ constexpr int psample_bt(int pw) { return pw <= 10 ? 64 : (pw <= 16 ? 32 : 16); }
// samples a lane carries through one read of the triangles (the LDS reads are what the kernel issues most of)
__host__ __device__ constexpr int psample_ns(int pw) { return pw <= 16 ? 2 : 1; }
__host__ __device__ constexpr size_t psample_mix_lds(int pw) { return (size_t)2 * (pw * (pw + 1) / 2) * psample_bt(pw) * sizeof(double); }

struct PsMixP {
  double* X;               // [nslots][S][p][T]: Yv = F U on entry, the draws on exit (in place: a lane reads its p values before it stores them)
  const double* Z1;        // [nslots][S][p][T]
  const double* G;         // [nslots][T][p][p] per-bin blocks (c->Gbin), symmetric
  const double* Xmode;     // [R][p][T]
  const int* trial_of_slot;
  int S, p, T;
  double sqrt_eps;
};

// x[k][t] = m[k][t] + sum_j G_t[k][j] yv[j][t] + sqrt(eps) sum_{j <= k} R_t[k][j] z1[j][t].   grid = (ceil(T / BT), nslots), block = 256, dynamic LDS.
// A lane owns one bin of the tile (lane % BT) and walks the samples lane / BT, + 256 / BT, ...: loads and stores run along t (contiguous), the triangle
// reads of the lanes of a wave hit consecutive banks ([pair][bin]) or one address (lanes of the same bin).  R_t is formed once per (slot, bin), by the
// first BT threads, one bin each, in LDS.
template <int PW>
__global__ __launch_bounds__(256) void psample_mix_kernel(PsMixP a) {
  constexpr int BT = psample_bt(PW), NS = psample_ns(PW), NP = PW * (PW + 1) / 2, LANES = 256 / BT;
  extern __shared__ double ps_sm[];
  double* Gs = ps_sm;                   // [NP][BT], pair (i >= j) at i (i + 1) / 2 + j
  double* Rs = ps_sm + (size_t)NP * BT;
  const int tid = threadIdx.x, p = a.p, T = a.T, pp = p * p;
  const int slot = blockIdx.y, t0 = blockIdx.x * BT, nb = min(BT, T - t0);
  const double* Gg = a.G + ((size_t)slot * T + t0) * pp;
  for (int e = tid; e < nb * pp; e += 256) {
    const int b = e / pp, r = e - b * pp, i = r / p, j = r - i * p;
    if (i >= j) Gs[(i * (i + 1) / 2 + j) * BT + b] = Gg[e];
  }
  __syncthreads();
  if (tid < nb) {
    const int b = tid;
    for (int j = 0; j < p; ++j) {
      double dj = Gs[(j * (j + 1) / 2 + j) * BT + b];
      for (int k = 0; k < j; ++k) { const double v = Rs[(j * (j + 1) / 2 + k) * BT + b]; dj -= v * v; }
      dj = sqrt(fmax(dj, 0.0));
      Rs[(j * (j + 1) / 2 + j) * BT + b] = dj;
      const double inv = dj > 0.0 ? 1.0 / dj : 0.0;
      for (int i = j + 1; i < p; ++i) {
        double v = Gs[(i * (i + 1) / 2 + j) * BT + b];
        for (int k = 0; k < j; ++k) v -= Rs[(i * (i + 1) / 2 + k) * BT + b] * Rs[(j * (j + 1) / 2 + k) * BT + b];
        Rs[(i * (i + 1) / 2 + j) * BT + b] = v * inv;
      }
    }
  }
  __syncthreads();
  const int b = tid % BT, sl = tid / BT;
  if (b >= nb) return;                                        // (no barrier below)
  const size_t n = (size_t)p * T;
  const double* m = a.Xmode + (size_t)a.trial_of_slot[slot] * n + t0 + b;
  double mk[PW];
#pragma unroll
  for (int k = 0; k < PW; ++k) mk[k] = k < p ? m[(size_t)k * T] : 0.0;
  for (int s0 = sl * NS; s0 < a.S; s0 += LANES * NS) {
    double y[NS][PW], z[NS][PW];
#pragma unroll
    for (int u = 0; u < NS; ++u) {
      const bool live = s0 + u < a.S;
      const size_t o = ((size_t)slot * a.S + (live ? s0 + u : s0)) * n + t0 + b;
#pragma unroll
      for (int k = 0; k < PW; ++k) {
        y[u][k] = (k < p) ? a.X[o + (size_t)k * T] : 0.0;
        z[u][k] = (k < p) ? a.Z1[o + (size_t)k * T] : 0.0;
      }
    }
#pragma unroll
    for (int i = 0; i < PW; ++i) {
      if (i < p) {
        double ag[NS], ar[NS];
#pragma unroll
        for (int u = 0; u < NS; ++u) { ag[u] = 0.0; ar[u] = 0.0; }
#pragma unroll
        for (int j = 0; j < PW; ++j) {
          if (j < p) {
            const int pr = (i >= j) ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i;
            const double g = Gs[pr * BT + b];
#pragma unroll
            for (int u = 0; u < NS; ++u) ag[u] += g * y[u][j];
            if (j <= i) {
              const double r = Rs[pr * BT + b];
#pragma unroll
              for (int u = 0; u < NS; ++u) ar[u] += r * z[u][j];
            }
          }
        }
#pragma unroll
        for (int u = 0; u < NS; ++u)
          if (s0 + u < a.S) a.X[((size_t)slot * a.S + s0 + u) * n + (size_t)i * T + t0 + b] = mk[i] + (ag[u] + a.sqrt_eps * ar[u]);
      }
    }
  }
}

// dense engine: X[slot][s][.] += m of the slot's trial.  grid = (S nblk, nslots) with nblk = ceil(n / 256), block = 256
inline __global__ __launch_bounds__(256) void psample_add_mean_kernel(double* __restrict__ X, const double* __restrict__ Xmode, int n, int S, int nblk,
                                                                      const int* __restrict__ trial_of_slot) {
  const int s = blockIdx.x / nblk;
  const int e = (blockIdx.x - s * nblk) * 256 + threadIdx.x;
  if (e >= n) return;
  const size_t o = ((size_t)blockIdx.y * S + s) * n + e;
  X[o] = Xmode[(size_t)trial_of_slot[blockIdx.y] * n + e] + X[o];
}

struct PsCountP {
  const double* X;         // [nslots][S][p][T]
  const double* C;         // [q][p]
  const double* d;         // [q]
  const int* len;          // [R] bins of every trial, NULL: T
  const int* trial_of_slot;
  uint16_t* Y;             // [nslots][S][q][T] or NULL
  int* csum;               // [nslots][S][q] or NULL
  int* over;               // [nslots]: set when a draw of the slot exceeds 65535
  int S, q, p, T;
  unsigned long long seed;
};

// eta = d + C x on v_mfma_f64_16x16x4_f64 with the maps of rates_kernel (rates.h): first operand of lane (l15, l4) = C[n0 + l15][4 ks + l4], second =
// x[4 ks + l4][t0 + l15], accumulator register r = neuron n0 + 4 r + l4, bin t0 + l15 - so the second operand and the uint16 stores run along the bins.
// grid = (S, nslots), block = 256: wave w of the workgroup of (sample, slot) takes the neuron tiles w, w + 4, ... and walks the bin tiles of each; the
// per-(sample, neuron) sums stay in its registers over that walk and are reduced over the 16 bin lanes at its end (integers: exact, no atomics).
// The loading fragments of a neuron tile (KS = ceil(p / 4) <= 8 doubles per lane) stay in registers over the walk.
inline __global__ __launch_bounds__(256) void psample_counts_kernel(PsCountP a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, l4 = lane >> 4;
  const int q = a.q, p = a.p, T = a.T, KS = (p + 3) >> 2;
  const unsigned s = blockIdx.x;
  const int slot = blockIdx.y;
  const unsigned trial = (unsigned)a.trial_of_slot[slot];
  const int Tr = a.len ? a.len[trial] : T;
  const Philox base{(unsigned)a.seed, (unsigned)(a.seed >> 32)};
  unsigned kw[4];
  base(s, 0u, 0u, PS_STREAM_KEY, kw);
  const Philox rng{kw[0], kw[1]};
  const double* x = a.X + ((size_t)slot * a.S + s) * p * T;
  const size_t orow = ((size_t)slot * a.S + s) * q;
  bool over = false;
  for (int n0 = wave * 16; n0 < q; n0 += 64) {
    double cf[8];
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      const int k = 4 * ks + l4;
      cf[ks] = (ks < KS && k < p && n0 + l15 < q) ? a.C[(size_t)(n0 + l15) * p + k] : 0.0;
    }
    double dn[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) dn[r] = (n0 + 4 * r + l4 < q) ? a.d[n0 + 4 * r + l4] : 0.0;
    int sum[4] = {0, 0, 0, 0};
    for (int t0 = 0; t0 < T; t0 += 16) {
      const int t = t0 + l15;
      if (t0 >= Tr) {                                          // (wave-uniform) padded bins: zero counts, nothing drawn
        if (a.Y && t < T) {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (n0 + 4 * r + l4 < q) a.Y[(orow + n0 + 4 * r + l4) * T + t] = 0;
        }
        continue;
      }
      double4_t acc = double4_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) {
        if (ks < KS) {                                         // (uniform)
          const int k = 4 * ks + l4;
          const double xv = (k < p && t < T) ? x[(size_t)k * T + t] : 0.0;
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(cf[ks], xv, acc, 0, 0, 0);
        }
      }
      // (one copy of the sampler's code: the four accumulator registers go through it in a rolled loop, picked by compares)
      double lam[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) lam[r] = (n0 + 4 * r + l4 < q && t < Tr) ? exp(acc[r] + dn[r]) : -1.0;      // (-1: no draw)
      unsigned v4[4] = {0u, 0u, 0u, 0u};
#pragma nounroll
      for (int r = 0; r < 4; ++r) {
        const double l = r == 0 ? lam[0] : (r == 1 ? lam[1] : (r == 2 ? lam[2] : lam[3]));
        unsigned v = 0u;
        if (l > 1.0e9 || l != l) {                             // (far beyond the output's range, infinite or NaN: nothing the sampler's integer result could hold)
          over = true; v = 65535u;
        } else if (l >= 0.0) {
          v = poisson_draw(l, rng, trial, (unsigned)(n0 + 4 * r + l4) * 65536u + (unsigned)t);
          if (v > 65535u) { over = true; v = 65535u; }
        }
        v4[0] = r == 0 ? v : v4[0]; v4[1] = r == 1 ? v : v4[1]; v4[2] = r == 2 ? v : v4[2]; v4[3] = r == 3 ? v : v4[3];
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + 4 * r + l4;
        sum[r] += (int)v4[r];
        if (a.Y && n < q && t < T) a.Y[(orow + n) * T + t] = (uint16_t)v4[r];
      }
    }
    if (a.csum) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int v = sum[r];
        for (int off = 8; off > 0; off >>= 1) v += __shfl_xor(v, off);
        const int n = n0 + 4 * r + l4;
        if (l15 == 0 && n < q) a.csum[orow + n] = v;
      }
    }
  }
  if (over) a.over[slot] = 1;                                  // (every writer stores the same value)
}

}  // namespace pgpfa
