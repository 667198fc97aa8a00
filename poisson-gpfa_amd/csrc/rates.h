// Posterior firing rates (pgpfa_posterior_rates): per (trial, neuron, bin) the posterior mean and variance of the log rate under the resident
// Gaussian posterior, the expected Poisson log likelihood and per-group sums of the posterior mean rate.
//   eta[n][t] = d_n + c_n . m_t                      (the log rate exp(C x + d) of util.py:289-334 is taken at, here at the posterior mean)
//   var[n][t] = c_n^T Sigma_t c_n                    (twice the v of inference.py:215-219)
//   rate      = exp(eta + var / 2)
// Both are ONE contraction of length KK = P4 + NP4 per (neuron, bin): a table row of neuron n
//   TBL[n] = [ c_n (p, padded to P4) | (2 - delta_ij) c_ni c_nj for i <= j (NP = p (p + 1) / 2, padded to NP4) ]
// against a bin column
//   COL[t] = [ m_t | Sigma_t[i][j] for i <= j ]
// where the first P4 rows feed the accumulator of eta and the rest the accumulator of var (P4, NP4: multiples of four, so that no k step of
// v_mfma_f64_16x16x4 straddles the two).  Tile: 16 neurons (first operand) x 16 bins (second operand) per wave and instruction, so that the
// accumulator register r of lane (l15, l4) holds neuron 4 r + l4, bin l15: stores run along the bins, contiguous in eta / var / group_sum.
// The bin columns of a tile of BT = 16 NBT bins are gathered ONCE per (trial, bin tile) into LDS - the means from Xmode (latent-major, bins
// contiguous), the pairs from vsm (bin-major, p^2 contiguous: the tile is one contiguous run) - and serve every neuron tile of the workgroup;
// the table fragments come from L2 (the table is q x KK doubles).  LDS row stride S = 16 mod 32 doubles (16, 48, 80): the two rows k, k + 1 that one half
// wave of a ds_read_b64 touches then fall into disjoint halves of the 64 banks.
#pragma once

namespace pgpfa {

struct RatesP {
  const double* Xmode;     // [R][p][T]
  const double* vsm;       // [R][T][p][p]
  const double* tbl;       // [KS][qpad][4]
  const double* d;         // [q]
  const uint8_t* Y;        // [R][q][T] (read for ell only)
  const uint8_t* Yhi;      // high bytes or NULL
  const int* len;          // [R] bins of every trial, NULL: T
  const int* ptrial;       // trial of every position of the call's list
  const int* istart;       // CSR over the items of this launch: positions of item z are ipos[istart[z] .. istart[z + 1]); NULL: item z is position c0 + z
  const int* ipos;
  int c0;                  // first position of the chunk: per-trial outputs are indexed by position - c0
  double* eta;             // [chunk][q][T] or NULL
  double* var;             // [chunk][q][T] or NULL
  double* ellp;            // [chunk][nbt][q] partial sums over the bins of a tile, or NULL
  double* gsum;            // [items][q][T] or NULL (GROUP kernels only): read at the start, stored at the end
  int q, p, T, P4, KS, qpad, nbt;
};

// LDS row stride (doubles) of a tile of bt bins: bt rounded up to 16 mod 32 - 16, 48, 80
__host__ __device__ constexpr int rates_row_stride(int bt) { return (bt % 32 == 16) ? bt : bt + 16; }

// count of entry i: low byte, and the plane of high bytes while the tensor holds a count above 255 (a wave-uniform branch; as count_at of model.h)
__device__ __forceinline__ unsigned rates_count_at(const uint8_t* __restrict__ Y, const uint8_t* __restrict__ Yhi, size_t i) {
  unsigned v = Y[i];
  if (Yhi) v |= (unsigned)Yhi[i] << 8;
  return v;
}

// grid = (qpad / 16), block = 64: the table of one parameter set
inline __global__ __launch_bounds__(64) void rates_table_kernel(const double* __restrict__ C, int q, int p, int P4, int KS, int qpad, double* __restrict__ tbl) {
  const int n = blockIdx.x * 16 + (threadIdx.x & 15);
  const int np = p * (p + 1) / 2;
  for (int k = threadIdx.x >> 4; k < 4 * KS; k += 4) {
    double v = 0.0;
    if (n < q) {
      if (k < p) v = C[(size_t)n * p + k];
      else if (k >= P4 && k < P4 + np) {
        int c = k - P4, i = 0;                               // pairs i <= j, row-major: row i holds p - i of them
        while (c >= p - i) { c -= p - i; ++i; }
        const int j = i + c;
        v = (i == j ? 1.0 : 2.0) * C[(size_t)n * p + i] * C[(size_t)n * p + j];
      }
    }
    tbl[((size_t)(k >> 2) * qpad + n) * 4 + (k & 3)] = v;
  }
}

// grid = (bin tiles, neuron blocks, items), block = 256 (four waves).  Wave w of neuron block y takes the neuron tiles y * 4 + w, + 4 gridDim.y, ...
// GROUP: the item is a group of positions whose rates are summed; the host launches one neuron tile per wave (gridDim.y = ceil(tiles / 4)) so that the
// sums of the walk stay in registers.  dynamic LDS: 4 KS rows of S doubles, then p^2 ints (row of the pair (i, j), -1 below the diagonal).
template <int NBT, bool GROUP>
__global__ __launch_bounds__(256) void rates_kernel(RatesP a) {
  constexpr int BT = 16 * NBT, S = rates_row_stride(BT);
  extern __shared__ double rates_sm[];
  double* col = rates_sm;
  int* pmap = reinterpret_cast<int*>(rates_sm + (size_t)4 * a.KS * S);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
  const int q = a.q, p = a.p, T = a.T, pp = p * p, KS = a.KS, KSM = a.P4 >> 2;
  const int bt = blockIdx.x, t0 = bt * BT, nb = min(BT, T - t0);
  const int item = blockIdx.z;
  const int l0 = a.istart ? a.istart[item] : item, l1 = a.istart ? a.istart[item + 1] : item + 1;
  if (l0 >= l1) return;                                      // (an empty group keeps what its accumulator tile holds)
  const int ntile = a.qpad >> 4;
  const bool planes = a.eta || a.var || a.ellp;

  // rows and bins no trial writes stay zero: padding rows meet zero table entries, padding bins are never stored
  for (int e = tid; e < 4 * KS * S; e += 256) col[e] = 0.0;
  for (int e = tid; e < pp; e += 256) {
    const int i = e / p, j = e - i * p;
    pmap[e] = (i <= j) ? a.P4 + i * p - (i * (i - 1)) / 2 + (j - i) : -1;
  }
  const float inv_pp = 1.0f / (float)pp;

  double4_t gs[NBT];
  const int gt = blockIdx.y * 4 + wave;                      // GROUP: the wave's one neuron tile
  if constexpr (GROUP) {
#pragma unroll
    for (int s = 0; s < NBT; ++s)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = gt * 16 + 4 * r + l4, t = t0 + 16 * s + l15;
        gs[s][r] = (a.gsum && gt < ntile && n < q && t < T) ? a.gsum[((size_t)item * q + n) * T + t] : 0.0;
      }
  }

  for (int l = l0; l < l1; ++l) {
    const int pos = a.istart ? a.ipos[l] : a.c0 + l;
    const size_t r_ = a.ptrial[pos];
    const int Tr = a.len ? a.len[r_] : T;
    if (!planes && t0 >= Tr) continue;                       // (uniform over the workgroup) nothing of this tile enters a group sum
    const size_t lp = (size_t)(pos - a.c0);
    __syncthreads();                                         // the previous trial's column has been read
    for (int e = tid; e < p * BT; e += 256) {
      const int k = e / BT, tl = e - k * BT;
      if (tl < nb) col[k * S + tl] = a.Xmode[(r_ * p + k) * T + t0 + tl];
    }
    {
      const double* src = a.vsm + (r_ * T + t0) * (size_t)pp;
      const int cnt = nb * pp;
      for (int e = tid; e < cnt; e += 256) {
        const int tl = (int)(((float)e + 0.5f) * inv_pp);    // e / pp: (e + 1/2) / pp is at least 1 / (2 pp) away from an integer, e < 2^16
        const int row = pmap[e - tl * pp];
        const double v = src[e];
        if (row >= 0) col[row * S + tl] = v;
      }
    }
    __syncthreads();
    for (int nt = gt; nt < ntile; nt += 4 * gridDim.y) {
      const int n0 = nt * 16;
      double4_t accE[NBT], accV[NBT];
#pragma unroll
      for (int s = 0; s < NBT; ++s) { accE[s] = double4_t{0.0, 0.0, 0.0, 0.0}; accV[s] = double4_t{0.0, 0.0, 0.0, 0.0}; }
      const double* tb = a.tbl + ((size_t)n0 + l15) * 4 + l4;
      const double* cb = col + l4 * S + l15;
      for (int ks = 0; ks < KSM; ++ks) {
        const double av = tb[(size_t)ks * a.qpad * 4];
#pragma unroll
        for (int s = 0; s < NBT; ++s) accE[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, cb[ks * 4 * S + 16 * s], accE[s], 0, 0, 0);
      }
      for (int ks = KSM; ks < KS; ++ks) {
        const double av = tb[(size_t)ks * a.qpad * 4];
#pragma unroll
        for (int s = 0; s < NBT; ++s) accV[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, cb[ks * 4 * S + 16 * s], accV[s], 0, 0, 0);
      }
      double el[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + 4 * r + l4;
        const double dn = (n < q) ? a.d[n] : 0.0;
#pragma unroll
        for (int s = 0; s < NBT; ++s) {
          const int t = t0 + 16 * s + l15;
          const bool live = n < q && t < T;
          const double e_ = accE[s][r] + dn, v_ = fmax(accV[s][r], 0.0);
          const size_t o = (lp * q + n) * T + t;
          if (a.eta && live) a.eta[o] = e_;
          if (a.var && live) a.var[o] = v_;
          if (a.ellp || GROUP) {
            const bool in = live && t < Tr;                  // padded bins: no likelihood term, no group member
            const double rate = in ? exp(e_ + 0.5 * v_) : 0.0;
            if (a.ellp && in) el[r] += (double)rates_count_at(a.Y, a.Yhi, (r_ * q + n) * T + t) * e_ - rate;
            if constexpr (GROUP) gs[s][r] += rate;
          }
        }
      }
      if (a.ellp) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          double v = el[r];
          for (int off = 8; off > 0; off >>= 1) v += __shfl_xor(v, off);       // over the 16 bins of a row group, fixed order
          const int n = n0 + 4 * r + l4;
          if (l15 == 0 && n < q) a.ellp[(lp * a.nbt + bt) * q + n] = v;
        }
      }
      if constexpr (GROUP) break;                            // one tile per wave
    }
  }
  if constexpr (GROUP) {
    if (a.gsum && gt < ntile) {
#pragma unroll
      for (int s = 0; s < NBT; ++s)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int n = gt * 16 + 4 * r + l4, t = t0 + 16 * s + l15;
          if (n < q && t < T) a.gsum[((size_t)item * q + n) * T + t] = gs[s][r];
        }
    }
  }
}

// ell[pos][n] = sum over the bin tiles, in tile order.  grid = (ceil(q / 256), chunk), block = 256
inline __global__ __launch_bounds__(256) void rates_ell_kernel(const double* __restrict__ ellp, int q, int nbt, double* __restrict__ ell) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  const size_t lp = blockIdx.y;
  if (n >= q) return;
  double s = 0.0;
  for (int b = 0; b < nbt; ++b) s += ellp[(lp * nbt + b) * q + n];
  ell[lp * q + n] = s;
}

}  // namespace pgpfa
