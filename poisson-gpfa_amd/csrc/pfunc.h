// Posterior of linear functionals of a trial's latents (pgpfa_posterior_functionals).  With m the resident posterior mean [p][T], Sigma = M M^T the
// trial's p T x p T posterior covariance and U = (u_1 .. u_J) the weight vectors, each laid out [p][T],
//   mean[j] = u_j . m,      cov[j][l] = u_j^T Sigma u_l = (M^T U)^T (M^T U)
//   dense engine      M = L^-T of the Hessian:  Q = L^-1 U,  cov = Q^T Q                                       (one GEMM against the L^-T slab)
//   low-rank engine   Sigma = eps G + (G F L^-T)(G F L^-T)^T:  V = G U (per bin: the p x p block times the p weights of that bin; pfunc_expand_kernel),
//                     Q = L^-1 F^T V (the library's GEMM, per latent and then against L^-T; pfunc.hip),  cov = Q^T Q + eps U^T V
// Sigma is never formed.  Layout: the functionals are the contiguous index everywhere, JW doubles per row (a multiple of 16; columns >= J are zero),
// so that the GEMMs take U, V, F^T V and Q with the functionals as their row index:
//   U [slot or shared][rows][JW]   low-rank engine: row k T16 + t (rows t >= T zero); dense engine: row k T + t, npad rows (rows >= p T zero)
//   V [slot][p][T16][JW]           V[l][t][j] = sum_k G_t[l][k] U[k][t][j]
//   Q [slot][rows][JW]             Q[r][j] = (M^T u_j)[r]
// pfunc_gram_kernel: a workgroup owns one slot and one 16 x 16 tile (jt >= lt) of the J x J plane.  The k index - the rows of Q, then under the
// low-rank engine the p T16 rows of U and V - is long and the tile small, so the rows are dealt to the four waves in groups of four (wave w takes rows
// 16 i + 4 w .. + 3) and every wave runs v_mfma_f64_16x16x4_f64 on its share: first operand X[r + l4][16 jt + l15], second Y[r + l4][16 lt + l15], so
// that accumulator register x of lane (l15, l4) holds C[16 jt + 4 x + l4][16 lt + l15].  The four partial tiles are added through LDS in wave order by
// wave 0: no atomics, one fixed order.  Only the entries with j >= l are stored, each to both triangles; the diagonal is clamped at 0.  DIAG: the
// diagonal tiles alone, storing var and no plane - the same instructions on the same operands, so var has the bits of the plane's diagonal.
#pragma once

namespace pgpfa {

constexpr int PFUNC_BT = 16;                      // bins per workgroup of pfunc_expand_kernel
constexpr int PFUNC_JMAX = 1024;                  // most functionals of a call that asks for the J x J plane

struct PFuncP {
  const double* U;         // staged weights
  const double* Xmode;     // [R][p][T] resident posterior means
  const int* ptrial;       // trial of every slot
  const double* G;         // [nslots][T][p][p] per-bin blocks (c->Gbin), symmetric; NULL: dense engine
  double* V;               // [nslots][p][T16][JW] (expand)
  const double* Q;         // [nslots][rows][JW]
  double *mean, *var;      // [nslots][J]
  double* cov;             // [nslots][J][J]
  long long sU;            // doubles between the weights of consecutive slots (0: one set shared by all)
  long long sQ;            // doubles between the Q planes of consecutive slots
  int rows;                // rows of Q that can hold something, a multiple of 4
  int erows;               // rows of U and V under the low-rank engine (p T16)
  int lrow;                // rows of U between consecutive latents (T16 or T)
  int p, T, T16, JW, J;
  int j0, nj;              // columns of the staging the launch works on (nj a multiple of 16)
  int jout;                // functional that column j0 holds
  double eps;
};

// V of the columns j0 .. j0 + nj.  grid = (ceil(T / PFUNC_BT), nslots), block = 256, dynamic LDS: the packed lower triangles of G_t of the tile's bins
// as [pair][bin] (pair (i >= k) at i (i + 1) / 2 + k).  Wave w takes the rows (latent l, bin b) w, w + 4, ... and its lanes run along the functionals:
// stores and the reads of U are contiguous, the triangle reads of a wave hit one address.  The sum over k runs in latent order.
inline __global__ __launch_bounds__(256) void pfunc_expand_kernel(PFuncP a) {
  extern __shared__ double pfunc_sm[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int p = a.p, T = a.T, pp = p * p, JW = a.JW;
  const int slot = blockIdx.y, t0 = blockIdx.x * PFUNC_BT, nb = min(PFUNC_BT, T - t0);
  const double* Gg = a.G + ((size_t)slot * T + t0) * pp;
  for (int e = tid; e < nb * pp; e += 256) {
    const int b = e / pp, r = e - b * pp, i = r / p, k = r - i * p;
    if (i >= k) pfunc_sm[(i * (i + 1) / 2 + k) * PFUNC_BT + b] = Gg[e];
  }
  __syncthreads();
  const double* U = a.U + (size_t)slot * a.sU + a.j0;
  double* V = a.V + (size_t)slot * p * a.T16 * JW + a.j0;
  for (int row = wave; row < p * nb; row += 4) {
    const int l = row / nb, b = row - l * nb, t = t0 + b;
    double* dst = V + ((size_t)l * a.T16 + t) * JW;
    for (int c = lane; c < a.nj; c += 64) {
      double v = 0.0;
      for (int k = 0; k < p; ++k) {
        const int pr = (l >= k) ? l * (l + 1) / 2 + k : k * (k + 1) / 2 + l;
        v += pfunc_sm[pr * PFUNC_BT + b] * U[((size_t)k * a.T16 + t) * JW + c];
      }
      dst[c] = v;
    }
  }
}

// grid = (ceil(nj / 256), nslots), block = 256: mean[slot][j] = sum_k sum_t m_k[t] u_j[k][t], in latent and then bin order
inline __global__ __launch_bounds__(256) void pfunc_mean_kernel(PFuncP a) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  const size_t slot = blockIdx.y;
  const int j = a.jout + c;
  if (c >= a.nj || j >= a.J) return;
  const size_t r = a.ptrial[slot];
  const double* m = a.Xmode + r * a.p * (size_t)a.T;
  const double* U = a.U + slot * (size_t)a.sU + a.j0 + c;
  double acc = 0.0;
  for (int k = 0; k < a.p; ++k)
    for (int t = 0; t < a.T; ++t) acc += m[(size_t)k * a.T + t] * U[((size_t)k * a.lrow + t) * a.JW];
  a.mean[slot * a.J + j] = acc;
}

// grid = (nj / 16, DIAG ? 1 : nj / 16, nslots), block = 256 (four waves)
template <bool DIAG>
__global__ __launch_bounds__(256) void pfunc_gram_kernel(PFuncP a) {
  __shared__ double part[3 * 256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
  const int jt = blockIdx.x, lt = DIAG ? jt : (int)blockIdx.y;
  if (lt > jt) return;                                       // (the whole workgroup: the mirror tile writes these entries)
  const size_t slot = blockIdx.z;
  const int JW = a.JW, ca = a.j0 + 16 * jt + l15, cb = a.j0 + 16 * lt + l15;
  double4_t acc = double4_t{0.0, 0.0, 0.0, 0.0};
  const double* Q = a.Q + slot * (size_t)a.sQ;
  for (int r = 4 * wave + l4; r < a.rows; r += 16) {        // (rows is a multiple of 4: the trip count is the wave's)
    const double* q = Q + (size_t)r * JW;
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(q[ca], q[cb], acc, 0, 0, 0);
  }
  if (a.G) {                                                 // eps U^T V, behind the rows of Q in the same accumulator
    const double* U = a.U + slot * (size_t)a.sU;
    const double* V = a.V + slot * (size_t)a.erows * JW;
    for (int r = 4 * wave + l4; r < a.erows; r += 16)
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a.eps * V[(size_t)r * JW + ca], U[(size_t)r * JW + cb], acc, 0, 0, 0);
  }
  if (wave > 0) {
#pragma unroll
    for (int x = 0; x < 4; ++x) part[(wave - 1) * 256 + x * 64 + lane] = acc[x];
  }
  __syncthreads();
  if (wave > 0) return;
#pragma unroll
  for (int w = 0; w < 3; ++w)
#pragma unroll
    for (int x = 0; x < 4; ++x) acc[x] += part[w * 256 + x * 64 + lane];
  const int J = a.J;
#pragma unroll
  for (int x = 0; x < 4; ++x) {
    const int j = a.jout + 16 * jt + 4 * x + l4, l = a.jout + 16 * lt + l15;
    if (j >= J || l > j) continue;
    double v = acc[x];
    if (j == l) {
      v = fmax(v, 0.0);
      if (a.var) a.var[slot * J + j] = v;
    }
    if constexpr (!DIAG) {
      double* out = a.cov + slot * (size_t)J * J;
      out[(size_t)j * J + l] = v;
      out[(size_t)l * J + j] = v;
    }
  }
}

}  // namespace pgpfa
