// Cross-latent posterior covariance at arbitrary time points (pgpfa_posterior_cov_at).  With a_k(s) = K_k^-1 kx_k(s) the interpolation weights of
// interp.h and Sigma = M M^T the trial's p T x p T posterior covariance,
//   Cov(x(s))[k][l] = a_k(s)^T Sigma_kl a_l(s) + delta_kl (1 - a_k(s) . kx_k(s)) = q_k(s) . q_l(s) + ...,      q_k(s) = M^T e_{k,s}
// where e_{k,s} holds a_k(s) in latent k's block and zeros elsewhere.
//   dense engine      M = L^-T of the Hessian:  q_k(s) = L^-1 e_{k,s}                                          (rows k T .. of L^-T against a_k: GEMM)
//   low-rank engine   Sigma = eps G + (G F L^-T)(G F L^-T)^T:  q_k(s) = L^-1 F^T (G e_{k,s}),  plus  eps sum_t a_k[t] a_l[t] G_t[k][l]
//                     V = G e_{k,s} by covat_expand_kernel, F^T V and the product with L^-T by the library's GEMM (covat.hip)
// Layout of one block of SB query times (SB a multiple of 16): a right-hand side is column c = k SB + s of CC = p SB, contiguous, so that the GEMMs
// take V, F^T V and Q with the right-hand sides as their row index:
//   V [slot][p][T16][CC]    V[j][t][c] = G_t[j][k] a_k[t][s]         (rows t >= T zero)
//   Q [slot][rows][CC]      Q[i][c]    = q_k(s)[i]
// covat_gram_kernel: a workgroup owns one slot and 16 consecutive query times, wave w the times 4 w .. 4 w + 3.  It walks the rows of Q in steps of 8;
// a step (8 rows x p latents x 16 times) is staged once in LDS as [row][latent][time] and every wave forms, per time, the p x p Gram of its p vectors
// with v_mfma_f64_16x16x4_f64: first operand Q[i + l4][16 a + l15], second Q[i + l4][16 b + l15], so that accumulator register r of lane (l15, l4)
// holds Cov[16 a + 4 r + l4][16 b + l15] - the map of interp_var_kernel and rates_kernel.  One tile (a, b) = (0, 0) up to 16 latents, the lower three
// of the 2 x 2 up to 32.  The rows are walked in one order by one wave per time: no atomics, no partial sums.
// LDS: time stride 1, latent stride 17, row stride RS = 16 mod 32 doubles: the 32 lanes of a half wave (l15 = 0 .. 15, l4 in {0, 1} or {2, 3}) read
// words 17 l15 + 16 l4 mod 32 - all 32 double-wide banks once.
// Behind the walk the two terms no Gram holds are added, both in one fixed order: a_k . kx_k per (latent, time) by a wave per latent (four bin groups, two shuffles), and - low-rank
// engine - eps sum_t a_k[t] a_l[t] G_t[k][l] straight into the accumulators, the weights of 8 bins at a time staged in the same LDS image (the reads of
// a lane are words 17 k + u, one address per row group, and 17 l15 + u: no conflict), G_t[k][l] from L2.  The epilogue clamps the diagonal at 0 and writes
// both triangles from the lower one's accumulator.
#pragma once

namespace pgpfa {

constexpr int COVAT_BT = 16;                      // bins per workgroup of covat_expand_kernel
constexpr int COVAT_IC = 8;                       // rows of Q per LDS step of covat_gram_kernel
__host__ __device__ constexpr int covat_row_stride(int nt) { return nt == 1 ? 16 * 17 : 32 * 17 + 16; }

struct CovAtP {
  const double* A;         // [grid][p][T16][Spad] weights
  const double* kx;        // [grid][p][T16][Spad] cross Gram
  const double* G;         // [nslots][T][p][p] per-bin blocks (c->Gbin), symmetric; NULL: dense engine
  double* V;               // [nslots][p][T16][CC] (expand)
  const double* Q;         // [nslots][rows][CC]
  double* cov;             // [nslots][Spad][p][p]
  long long sG;            // doubles between the grids of consecutive slots (0: one grid shared by all)
  long long sQ;            // doubles between the Q planes of consecutive slots
  int rows;                // rows of Q that can hold something, a multiple of COVAT_IC
  int p, T, T16, Spad, SB, s0, nsb;     // block: SB columns per latent in the staging, query times s0 .. s0 + nsb (nsb a multiple of 16)
  double eps;
};

// V of one block.  grid = (ceil(T / COVAT_BT), nslots), block = 256, dynamic LDS: the packed lower triangles of G_t of the tile's bins as [pair][bin]
// (pair (i >= j) at i (i + 1) / 2 + j).  Wave w takes the rows (latent j, bin b) w, w + 4, ... and its lanes run along the right-hand sides: stores
// and the reads of A are contiguous, the triangle reads of a wave hit at most CC / SB addresses.  Columns past the block's times are written as zeros.
inline __global__ __launch_bounds__(256) void covat_expand_kernel(CovAtP a) {
  extern __shared__ double covat_sm[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int p = a.p, T = a.T, pp = p * p, SB = a.SB, CC = p * SB;
  const int slot = blockIdx.y, t0 = blockIdx.x * COVAT_BT, nb = min(COVAT_BT, T - t0);
  const double* Gg = a.G + ((size_t)slot * T + t0) * pp;
  for (int e = tid; e < nb * pp; e += 256) {
    const int b = e / pp, r = e - b * pp, i = r / p, j = r - i * p;
    if (i >= j) covat_sm[(i * (i + 1) / 2 + j) * COVAT_BT + b] = Gg[e];
  }
  __syncthreads();
  const double* A = a.A + (size_t)slot * a.sG;
  double* V = a.V + (size_t)slot * p * a.T16 * CC;
  for (int row = wave; row < p * nb; row += 4) {
    const int j = row / nb, b = row - j * nb, t = t0 + b;
    double* dst = V + ((size_t)j * a.T16 + t) * CC;
    for (int c = lane; c < CC; c += 64) {
      const int k = c / SB, s = c - k * SB;
      const int pr = (j >= k) ? j * (j + 1) / 2 + k : k * (k + 1) / 2 + j;
      double v = 0.0;
      if (s < a.nsb) v = covat_sm[pr * COVAT_BT + b] * A[((size_t)k * a.T16 + t) * a.Spad + a.s0 + s];
      dst[c] = v;
    }
  }
}

// grid = (nsb / 16, nslots), block = 256 (four waves).  NT = 1: up to 16 latents, NT = 2: up to 32.
template <int NT>
__global__ __launch_bounds__(256) void covat_gram_kernel(CovAtP a) {
  constexpr int RS = covat_row_stride(NT), NTILE = NT == 1 ? 1 : 3;
  __shared__ double qs[COVAT_IC * RS];
  __shared__ double dsum[16 * NT * 16];                       // a_k . kx_k of the workgroup's (latent, time) entries
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
  const int p = a.p, T = a.T, pp = p * p, SB = a.SB, CC = p * SB;
  const int slot = blockIdx.y, sl0 = blockIdx.x * 16;       // first time of the workgroup, within the block
  const double* Q = a.Q + (size_t)slot * a.sQ + sl0;
  for (int e = tid; e < COVAT_IC * RS; e += 256) qs[e] = 0.0;           // latents >= p stay zero
  double4_t acc[4][NTILE];
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int x = 0; x < NTILE; ++x) acc[u][x] = double4_t{0.0, 0.0, 0.0, 0.0};
  const int cnt = COVAT_IC * p * 16;
  for (int i0 = 0; i0 < a.rows; i0 += COVAT_IC) {
    __syncthreads();                                         // the step before has been read (first trip: the image is cleared)
    for (int e = tid; e < cnt; e += 256) {
      const int s = e & 15, ik = e >> 4, i = ik / p, k = ik - i * p;
      qs[i * RS + k * 17 + s] = Q[(size_t)(i0 + i) * CC + (size_t)k * SB + s];
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < COVAT_IC; kk += 4) {
      const double* qr = qs + (kk + l4) * RS + l15 * 17 + 4 * wave;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const double q0 = qr[u];
        acc[u][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(q0, q0, acc[u][0], 0, 0, 0);
        if constexpr (NT == 2) {
          const double q1 = qr[16 * 17 + u];
          acc[u][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(q1, q0, acc[u][1], 0, 0, 0);
          acc[u][2] = __builtin_amdgcn_mfma_f64_16x16x4f64(q1, q1, acc[u][2], 0, 0, 0);
        }
      }
    }
  }
  // the two terms no Gram holds.  s16: first of the workgroup's 16 times on the padded grid (the block's times are whole 16-groups of it)
  const int s16 = a.s0 + sl0;
  const double* A = a.A + (size_t)slot * a.sG + s16;
  const double* KX = a.kx + (size_t)slot * a.sG + s16;
  // a_k . kx_k per (latent, time): wave w takes the latents w, w + 4, ..., its 16 lanes l15 run along the times and its four row groups l4 take the
  // bins l4, l4 + 4, ... in order; the four partial sums are added by two shuffles (one fixed order) and the p x 16 sums of the workgroup go to LDS
  for (int k = wave; k < p; k += 4) {
    const double* ak = A + (size_t)k * a.T16 * a.Spad + l15;
    const double* kk_ = KX + (size_t)k * a.T16 * a.Spad + l15;
    double d = 0.0;
    for (int t = l4; t < T; t += 4) d += ak[(size_t)t * a.Spad] * kk_[(size_t)t * a.Spad];
    d += __shfl_xor(d, 16);
    d += __shfl_xor(d, 32);
    if (l4 == 0) dsum[k * 16 + l15] = d;
  }
  // eps sum_t a_k[t] a_l[t] G_t[k][l] (low-rank engine), in bin order, into the accumulators: the weights of 8 bins at a time go through the LDS
  // image of the walk above (rows t >= T of A are zero), G_t[k][l] comes from L2 - a row of it per 16 lanes
  if (a.G) {
    bool ok[NTILE][4];
    int kl[NTILE][4];
#pragma unroll
    for (int x = 0; x < NTILE; ++x)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int k = 16 * (x == 0 ? 0 : 1) + 4 * r + l4, l = 16 * (x == 2 ? 1 : 0) + l15;
        ok[x][r] = k < p && l <= k;
        kl[x][r] = ok[x][r] ? k * p + l : 0;
      }
    const double* Gs = a.G + (size_t)slot * T * pp;
    for (int t0 = 0; t0 < a.T16; t0 += COVAT_IC) {
      __syncthreads();                                       // the step before has been read (first trip: the last rows of Q)
      for (int e = tid; e < cnt; e += 256) {
        const int s = e & 15, ik = e >> 4, i = ik / p, k = ik - i * p;
        qs[i * RS + k * 17 + s] = A[((size_t)k * a.T16 + t0 + i) * a.Spad + s];
      }
      __syncthreads();
#pragma unroll 1                                             // (unrolled, the G loads of all 8 bins are hoisted and the 32-latent form spills)
      for (int i = 0; i < COVAT_IC; ++i) {
        const int t = t0 + i;
        const double* row = qs + i * RS + 4 * wave;
#pragma unroll
        for (int x = 0; x < NTILE; ++x)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int k = 16 * (x == 0 ? 0 : 1) + 4 * r + l4, l = 16 * (x == 2 ? 1 : 0) + l15;
            const double g = (ok[x][r] && t < T) ? a.eps * Gs[(size_t)t * pp + kl[x][r]] : 0.0;
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[u][x][r] += g * (row[k * 17 + u] * row[l * 17 + u]);
          }
      }
    }
  }
  __syncthreads();                                           // dsum is complete
  // entry (k, l <= k) of every time of the wave: the diagonal gets the prior conditional and is clamped, both triangles are written from this value
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    double* out = a.cov + ((size_t)slot * a.Spad + s16 + 4 * wave + u) * pp;
#pragma unroll
    for (int x = 0; x < NTILE; ++x) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int k = 16 * (x == 0 ? 0 : 1) + 4 * r + l4, l = 16 * (x == 2 ? 1 : 0) + l15;
        if (k >= p || l > k) continue;
        double v = acc[u][x][r];
        if (k == l) v = fmax(v + (1.0 - dsum[k * 16 + 4 * wave + u]), 0.0);
        out[k * p + l] = v;
        out[l * p + k] = v;
      }
    }
  }
}

}  // namespace pgpfa
