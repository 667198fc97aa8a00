// Latent velocities at arbitrary time points (pgpfa_posterior_velocity_at): under the prior the time derivative of latent k at s is jointly Gaussian
// with the grid values, so its posterior follows by the prior conditional of interp.h with the cross Gram differentiated.  Per latent k, with K_k,
// m_k, V_k and kx_k(s) as there, l_k = 1000 tau_k ms:
//   kd_k(s)[j] = -1000 (s - j bin) / l_k^2 (1 - eps) exp(-1/2 (s - j bin)^2 / l_k^2)   = Cov(xdot_k(s), x_k(j bin)), per SECOND   (velat_cross_kernel)
//   a = K_k^-1 kx,  b = K_k^-1 kd                                                         (the library's batched GEMM: interp_solve)
//   mean = a . m_k,  vel = b . m_k                                                        (interp_mean_kernel on A / B)
//   var     = 1       - a . kx + a^T V_k a                                                (velat_joint_kernel, the three of them in one pass over V_k)
//   vel_var = kappa_k - b . kd + b^T V_k b,   kappa_k = (1 - eps) / tau_k^2
//   cross   =         - a . kd + a^T V_k b    = Cov(x_k(s), xdot_k(s)), 0 under the prior
// The velocity is that of the smooth component: the white eps part has no derivative, so kd carries no nugget term even at a grid time.
// Layout: kd and B as kx and A, [grid][p][T16][Spad], zero in every row >= T and every column >= S.
//
// velat_joint_kernel: interp_var_kernel with two right-hand sides.  A workgroup owns one (trial, latent) and up to `sblk` query times; it walks the
// T16 / 16 row panels of V_k, each staged ONCE in LDS (row stride interp_row_stride: conflict-free), and wave w takes the 16-column tiles w, w + 4,
// ...: per step of four bins ONE LDS fragment V[t0 + l15][u + l4] feeds two v_mfma_f64_16x16x4_f64, with A[u + l4][s0 + l15] and B[u + l4][s0 + l15]
// from L2, so that register r of lane (l15, l4) holds (V A)[t0 + 4 r + l4][s0 + l15] and (V B)[same].  The three folds
//   sum_r A (VA - kx),   sum_r B (VB - kd),   sum_r A (VB - kd),     t = t0 + 4 r + l4,
// are summed over the four row groups l4 by two shuffles and added to the tile's running sums in LDS (three planes of sblk doubles; a tile belongs to
// one wave: no race, fixed order, no atomics).  No T x S intermediate exists and V, the only T^2 stream, is read once per sblk query times for all
// three quadratic forms.  All three sums are always formed; only the planes asked for are stored, so a plane's bits do not follow the request.
#pragma once

namespace pgpfa {

constexpr int VELAT_SBLK = 1024;                  // query times per workgroup of velat_joint_kernel at most (24 KiB of running sums); a multiple of 16

struct VelatP {
  const double* vsmgp;     // [R][p][T][T]
  const double* A;         // [grid][p][T16][Spad] weights of the value
  const double* B;         // [grid][p][T16][Spad] weights of the velocity
  const double* kx;        // [grid][p][T16][Spad] cross Gram
  const double* kd;        // [grid][p][T16][Spad] its derivative in s, per second
  const double* tau;       // [p] s
  const int* ptrial;       // trial of every item of the launch
  double* var;             // [items][p][Spad] or NULL
  double* vel_var;         // [items][p][Spad] or NULL
  double* cross;           // [items][p][Spad] or NULL
  double eps;
  long long sG;            // doubles between the grids of consecutive items (0: one grid shared by all)
  int p, T, T4, T16, Spad, VS, sblk;
};

// grid = (T16, p, grids), block = 256: one row j of kd.  times: [grids][S] ms from the trial's first bin
inline __global__ __launch_bounds__(256) void velat_cross_kernel(const double* __restrict__ times, const double* __restrict__ tau, double bin, double eps, int T,
                                                                 int T16, int S, int Spad, int p, double* __restrict__ kd) {
  const int j = blockIdx.x, k = blockIdx.y;
  const size_t g = blockIdx.z;
  const double den = (tau[k] * 1000.0) * (tau[k] * 1000.0);
  const double tj = (double)j * bin;
  double* row = kd + ((g * p + k) * T16 + j) * (size_t)Spad;
  for (int s = threadIdx.x; s < Spad; s += 256) {
    double v = 0.0;
    if (j < T && s < S) {
      const double ts = times[g * S + s];
      const double dt = ts - tj;                             // (as interp_cross_kernel forms it)
      v = -1000.0 * dt / den * ((1.0 - eps) * exp(-0.5 * ((dt * dt) / den)));
    }
    row[s] = v;
  }
}

// grid = (ceil(Spad / sblk), p, items), block = 256 (four waves); dynamic LDS: 16 VS doubles (row panel) + 3 min(Spad, sblk) (running sums)
inline __global__ __launch_bounds__(256) void velat_joint_kernel(VelatP a) {
  extern __shared__ double velat_sm[];
  double* vp = velat_sm;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
  const int k = blockIdx.y, T = a.T, T4 = a.T4, Spad = a.Spad, VS = a.VS;
  const size_t item = blockIdx.z;
  const size_t r = a.ptrial[item];
  const int s_begin = blockIdx.x * a.sblk, ncols = min(a.sblk, Spad - s_begin), ntile = ncols >> 4;
  double* sums = velat_sm + 16 * VS;                         // planes: value, velocity, cross; ncols doubles each
  const double* V = a.vsmgp + (r * a.p + k) * (size_t)T * T;
  const size_t goff = item * (size_t)a.sG + (size_t)k * a.T16 * Spad + s_begin;
  const double* A = a.A + goff;
  const double* B = a.B + goff;
  const double* KX = a.kx + goff;
  const double* KD = a.kd + goff;
  for (int e = tid; e < 3 * ncols; e += 256) sums[e] = 0.0;
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
      double4_t va = double4_t{0.0, 0.0, 0.0, 0.0}, vb = double4_t{0.0, 0.0, 0.0, 0.0};
      const size_t c0 = (size_t)l4 * Spad + tile * 16 + l15;
      const double* ap = A + c0;
      const double* bp = B + c0;
      const double* vq = vp + l15 * VS + l4;
#pragma unroll 4
      for (int u = 0; u < T4; u += 4) {
        const double v = vq[u];                              // one fragment of V, two products
        va = __builtin_amdgcn_mfma_f64_16x16x4f64(v, ap[(size_t)u * Spad], va, 0, 0, 0);
        vb = __builtin_amdgcn_mfma_f64_16x16x4f64(v, bp[(size_t)u * Spad], vb, 0, 0, 0);
      }
      double f0 = 0.0, f1 = 0.0, f2 = 0.0;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const size_t o = (size_t)(t0 + 4 * rr + l4) * Spad + tile * 16 + l15;
        const double av = A[o], bv = B[o], rb = vb[rr] - KD[o];
        f0 += av * (va[rr] - KX[o]);
        f1 += bv * rb;
        f2 += av * rb;
      }
      f0 += __shfl_xor(f0, 16); f1 += __shfl_xor(f1, 16); f2 += __shfl_xor(f2, 16);
      f0 += __shfl_xor(f0, 32); f1 += __shfl_xor(f1, 32); f2 += __shfl_xor(f2, 32);
      if (l4 == 0) {
        const int e = tile * 16 + l15;
        sums[e] += f0;
        sums[ncols + e] += f1;
        sums[2 * ncols + e] += f2;
      }
    }
  }
  __syncthreads();
  const double kappa = (1.0 - a.eps) / (a.tau[k] * a.tau[k]);
  const size_t out = (item * a.p + k) * (size_t)Spad + s_begin;
  for (int e = tid; e < ncols; e += 256) {
    if (a.var) a.var[out + e] = fmax(1.0 + sums[e], 0.0);
    if (a.vel_var) a.vel_var[out + e] = fmax(kappa + sums[ncols + e], 0.0);
    if (a.cross) a.cross[out + e] = sums[2 * ncols + e];
  }
}

}  // namespace pgpfa
