// Latent posterior at arbitrary time points (pgpfa_posterior_at): the GP posterior N(m, Sigma) over the T grid times t_j = j bin extends to any
// time s by the prior conditional.  Per latent k, with K_k the Gram matrix of gram_tau_kernel (model.h) and V_k the trial's T x T block of latent k:
//   kx_k(s)[j] = (1 - eps) exp(-1/2 (s - j bin)^2 / (1000 tau_k)^2) + eps [s == j bin]       (interp_cross_kernel)
//   a_k(s)     = K_k^-1 kx_k(s)                                                              (the library's batched GEMM, gemm.h)
//   mean_k(s)  = a_k(s) . m_k                                                                (interp_mean_kernel)
//   var_k(s)   = 1 - a_k(s) . kx_k(s) + a_k(s)^T V_k a_k(s), stored as max(., 0)             (interp_var_kernel)
// Layout: kx and the weights A are [grid][p][T16][Spad] - query times contiguous, Spad = S rounded up to 16, T16 = T rounded up to 16, zero in
// every row >= T and every column >= S - so that neither the products nor the fold below need an edge case.
//
// interp_var_kernel: a workgroup owns one (trial, latent) and up to INTERP_SBLK query times.  It walks the T16 / 16 row panels of V_k; a panel (16
// rows, T4 = T rounded up to 4 columns, zero past T both ways) is staged ONCE in LDS and serves every 16-column tile of query times: wave w takes the
// tiles w, w + 4, ... and forms B = V_panel A_tile (16 x 16) with T4 / 4 v_mfma_f64_16x16x4_f64 - first operand V[t0 + l15][u + l4] from LDS, second
// A[u + l4][s0 + l15] from L2 - so that accumulator register r of lane (l15, l4) holds B[t0 + 4 r + l4][s0 + l15].  The tile is folded at once:
//   sum_r A[t][s] (B[t][s] - kx[t][s]),  t = t0 + 4 r + l4,
// summed over the four row groups l4 by two shuffles and added to the tile's 16 running sums in LDS (a tile belongs to one wave: no race, fixed
// order).  No T x S intermediate exists and V, the only T^2 stream, is read from HBM once per INTERP_SBLK query times.
// LDS row stride VS = 2 mod 32 doubles: the 32 lanes of a half wave read rows l15 at columns u + {0, 1} (or {2, 3}), i.e. words 2 l15 + {0, 1} mod
// 32 - all 64 banks once.
#pragma once

namespace pgpfa {

constexpr int INTERP_SBLK = 2048;                 // query times per workgroup of interp_var_kernel (16 KiB of running sums)

__host__ __device__ constexpr int interp_row_stride(int T4) { return T4 + ((2 - T4 % 32) + 32) % 32; }

struct InterpP {
  const double* vsmgp;     // [R][p][T][T]
  const double* Xmode;     // [R][p][T]
  const double* A;         // [grid][p][T16][Spad] weights
  const double* kx;        // [grid][p][T16][Spad] cross Gram
  const int* ptrial;       // trial of every item of the launch
  double* mean;            // [items][p][Spad] or NULL
  double* var;             // [items][p][Spad] or NULL
  long long sG;            // doubles between the grids of consecutive items (0: one grid shared by all)
  int p, T, T4, T16, Spad, VS;
};

// grid = (T16, p, grids), block = 256: one row j of kx.  times: [grids][S] ms from the trial's first bin
inline __global__ __launch_bounds__(256) void interp_cross_kernel(const double* __restrict__ times, const double* __restrict__ tau, double bin, double eps, int T,
                                                                  int T16, int S, int Spad, int p, double* __restrict__ kx) {
  const int j = blockIdx.x, k = blockIdx.y;
  const size_t g = blockIdx.z;
  const double den = (tau[k] * 1000.0) * (tau[k] * 1000.0);
  const double tj = (double)j * bin;
  double* row = kx + ((g * p + k) * T16 + j) * (size_t)Spad;
  for (int s = threadIdx.x; s < Spad; s += 256) {
    double v = 0.0;
    if (j < T && s < S) {
      const double ts = times[g * S + s];
      const double dt = ts - tj;                             // (at a grid time this is gram_tau_kernel's i bin - j bin, to the bit)
      v = (1.0 - eps) * exp(-0.5 * ((dt * dt) / den));
      if (ts == tj) v += eps;
    }
    row[s] = v;
  }
}

// grid = (ceil(Spad / 256), p, items), block = 256: mean[item][k][s] = sum_t m[t] A[t][s], in bin order
inline __global__ __launch_bounds__(256) void interp_mean_kernel(InterpP a) {
  const int s = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
  const size_t item = blockIdx.z;
  if (s >= a.Spad) return;
  const size_t r = a.ptrial[item];
  const double* m = a.Xmode + (r * a.p + k) * (size_t)a.T;
  const double* A = a.A + item * (size_t)a.sG + (size_t)k * a.T16 * a.Spad + s;
  double acc = 0.0;
  for (int t = 0; t < a.T; ++t) acc += m[t] * A[(size_t)t * a.Spad];
  a.mean[(item * a.p + k) * (size_t)a.Spad + s] = acc;
}

// grid = (ceil(Spad / INTERP_SBLK), p, items), block = 256 (four waves); dynamic LDS: 16 VS doubles (row panel) + min(Spad, INTERP_SBLK) (running sums)
inline __global__ __launch_bounds__(256) void interp_var_kernel(InterpP a) {
  extern __shared__ double interp_sm[];
  double* vp = interp_sm;
  double* sums = interp_sm + 16 * a.VS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
  const int k = blockIdx.y, T = a.T, T4 = a.T4, Spad = a.Spad, VS = a.VS;
  const size_t item = blockIdx.z;
  const size_t r = a.ptrial[item];
  const int s_begin = blockIdx.x * INTERP_SBLK, ncols = min(INTERP_SBLK, Spad - s_begin), ntile = ncols >> 4;
  const double* V = a.vsmgp + (r * a.p + k) * (size_t)T * T;
  const size_t goff = item * (size_t)a.sG + (size_t)k * a.T16 * Spad + s_begin;
  const double* A = a.A + goff;
  const double* KX = a.kx + goff;
  for (int e = tid; e < ncols; e += 256) sums[e] = 0.0;
  const int srow = tid >> 4, scol = tid & 15;                // staging: thread -> (panel row, column mod 16)
  for (int t0 = 0; t0 < a.T16; t0 += 16) {
    __syncthreads();                                         // the panel before has been read (first trip: the sums are cleared)
    {
      const int t = t0 + srow;
      const double* src = V + (size_t)t * T;
      for (int col = scol; col < T4; col += 16) vp[srow * VS + col] = (t < T && col < T) ? src[col] : 0.0;
    }
    __syncthreads();
    for (int tile = wave; tile < ntile; tile += 4) {
      double4_t acc = double4_t{0.0, 0.0, 0.0, 0.0};
      const double* ap = A + (size_t)l4 * Spad + tile * 16 + l15;
      const double* vq = vp + l15 * VS + l4;
#pragma unroll 4
      for (int u = 0; u < T4; u += 4) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(vq[u], ap[(size_t)u * Spad], acc, 0, 0, 0);
      double f = 0.0;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const size_t o = (size_t)(t0 + 4 * rr + l4) * Spad + tile * 16 + l15;
        f += A[o] * (acc[rr] - KX[o]);
      }
      f += __shfl_xor(f, 16);
      f += __shfl_xor(f, 32);
      if (l4 == 0) sums[tile * 16 + l15] += f;
    }
  }
  __syncthreads();
  for (int e = tid; e < ncols; e += 256) a.var[(item * a.p + k) * (size_t)Spad + s_begin + e] = fmax(1.0 + sums[e], 0.0);
}

}  // namespace pgpfa
