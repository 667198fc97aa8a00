// Posterior-predictive spike counts (pgpfa_count_probabilities, pgpfa_posterior_counts): per entry, from the two moments m = eta, v = var of the log
// rate, the Poisson-lognormal mixture
//   P(y = k) = int Poisson(k; e^eta) N(eta; m, v) d eta
// by a Q-node Gauss-Hermite rule centred on the integrand's MODE (a rule around m is useless once k is far from e^m).  Everything is written in the
// scaled deviation u = (eta - m) / v, so that eta - m is never formed by subtraction and v = 0 is an ordinary input (the Poisson pmf at e^m):
//   g(u)     = k (m + v u) - exp(m + v u) - v u^2 / 2 - lgamma(k + 1)            the log integrand, strictly concave
//   Newton   u += (k - lam - u) / (1 + v lam),  lam = exp(m + v u)                  from u = 0 (or the mode of k - 1: modes rise with k); a step that
//                                                                                   would raise eta by more than 1 is cut to 1; at most COUNTS_NEWTON steps
//   nodes    eta_q = m + v u* + s x_q,  s = sqrt(2 v / (1 + v lam*))                curvature h = lam* + 1 / v
//   a_q      = (k - u*) s x_q - lam* (exp(s x_q) - 1) + x_q^2 v lam* / (1 + v lam*) + log w_q          = g(eta_q) - g* + x_q^2 + log w_q
//   log P    = g* - 1/2 log(pi (1 + v lam*)) + log sum_q exp(a_q)
// a_q is bounded above by a small constant (w_q e^{x_q^2} is) and the central nodes give a sum of order 1: no overflow, no underflow, for any k.
// Cost per evaluation: up to COUNTS_NEWTON + 2 Q FP64 exponentials (about 4 + 2 Q with a warm start) - the kernel is bound by the FP64 vector pipe,
// not by memory: 20 bytes in and 8 out per at least 2 Q exponentials.
//
// Layout: one lane per entry, 64 entries - one wave - per workgroup.  m, v, the counts and every per-entry output are then coalesced, lane i at
// base + i (the programming guide's "Global memory coalescing"); the nodes are read at a wave-uniform index from a kernel-argument pointer, i.e. by
// scalar loads, and cost no vector register or LDS traffic.  pmf has k fastest, so a lane's own values are K doubles apart: the walk over k stages
// COUNTS_KT = 16 values per lane in LDS (row stride 17 doubles: a half wave that reads two rows of 16 doubles with ds_read_b64 touches the dwords
// 2 kk and 34 + 2 kk, 32 distinct banks of the 64; the column writes, one per 2 Q exponentials, meet two ways at worst) and the wave stores the tile
// with consecutive lanes on consecutive k - runs of 128 bytes per entry, one contiguous run of the whole tile when K <= 16.  One wave per workgroup keeps the
// barriers of that staging to the wave and lets a wave whose lanes have all finished their walk leave; occupancy comes from many small
// workgroups (the grid has n / 64 of them), not from wide ones.  No atomics: the saturated entries of a workgroup are counted by a ballot and
// written to the workgroup's own slot.
// Bits: every output of an entry is a function of (m, v, count, K, level, k_cap, nodes) alone - logp is computed from a cold start by code that does
// not look at the other output pointers, and the walk over k is the same chain k = 0, 1, ... whether it feeds pmf, the quantiles or both.
#pragma once

namespace pgpfa {

constexpr int COUNTS_NEWTON = 40;        // cap on the Newton steps of one mode search (the grid of the tests needs at most 17 from a cold start)
constexpr int COUNTS_KT = 16;            // k values per lane staged in LDS before a pmf store
constexpr int COUNTS_KS = COUNTS_KT + 1; // LDS row stride (doubles)

struct CountsP {
  const double* m;          // [n] posterior mean of the log rate
  const double* v;          // [n] its variance (>= 0)
  const int32_t* counts;    // [n] count of every entry (logp), or NULL: the resident counts Y / Yhi
  const uint8_t* Y;         // [R][q][T] resident counts (read only when counts is NULL and logp is asked for)
  const uint8_t* Yhi;
  const int* len;           // [R] bins of every trial or NULL; read only with ptrial
  const int* ptrial;        // trial of every position of the call's list, or NULL: plain entries, none of them padding
  const double* nodes;      // [2][Q]: x_q, log w_q
  double* logp;             // [n] or NULL
  double* pmf;              // [n][K] or NULL
  int32_t* lower;           // [n] or NULL
  int32_t* upper;           // [n] or NULL
  double* pmean;            // [n] or NULL
  double* pvar;             // [n] or NULL
  int32_t* sat;             // [gridDim.x] entries of the workgroup whose upper quantile lies beyond k_cap (written when upper is asked for)
  long long n;              // entries of this launch
  int c0, q, T;             // with ptrial: entry e is (position c0 + e / (q T), neuron, bin e % T)
  int Q, K, k_cap;
  double p_lo, p_hi;        // (1 - level) / 2, (1 + level) / 2
};

// One Newton search for the mode of g in u, started at u.  Returns u*, with lam* = exp(m + v u*) in *lam_out.
__device__ __forceinline__ double counts_mode(double m, double v, double k, double u, double* lam_out) {
  double lam = exp(m + v * u);
  for (int it = 0; it < COUNTS_NEWTON; ++it) {
    double du = (k - lam - u) / (1.0 + v * lam);
    if (v * du > 1.0) du = 1.0 / v;
    u += du;
    lam = exp(m + v * u);
    if (!(fabs(v * du) > 1e-12)) break;
  }
  *lam_out = lam;
  return u;
}

// log P(y = k) by the rule centred at u (the mode, with lam = exp(m + v u))
__device__ __forceinline__ double counts_logp_at(double m, double v, double k, double u, double lam, const double* __restrict__ nodes, int Q) {
  const double vl = v * lam, r = 1.0 / (1.0 + vl);
  const double s = sqrt(2.0 * v * r), c = vl * r, ku = k - u;
  double sum = 0.0;
#pragma unroll 2
  for (int j = 0; j < Q; ++j) {
    const double x = nodes[j], lw = nodes[Q + j];
    const double d = s * x;
    sum += exp(ku * d - lam * (exp(d) - 1.0) + (x * x) * c + lw);
  }
  const double gs = k * (m + v * u) - lam - 0.5 * v * (u * u) - lgamma(k + 1.0);
  return gs - 0.5 * (1.1447298858494002 + log1p(vl)) + log(sum);        // log pi
}

// grid = ceil(n / 64), block = 64
inline __global__ __launch_bounds__(64) void counts_kernel(CountsP a) {
  __shared__ double tile[64 * COUNTS_KS];
  const int lane = threadIdx.x;
  const long long e0 = (long long)blockIdx.x * 64, e = e0 + lane;
  const bool inside = e < a.n;
  const double qnan = __builtin_nan("");

  double m = 0.0, v = 0.0;
  bool live = inside;
  size_t yi = 0;                                             // index of the entry in the resident counts
  if (inside) {
    m = a.m[e];
    v = a.v[e];
    if (a.ptrial) {
      const long long qT = (long long)a.q * a.T;
      const long long lp = e / qT, nt = e - lp * qT;
      const int t = (int)(nt % a.T);
      const size_t r_ = (size_t)a.ptrial[a.c0 + lp];
      live = t < (a.len ? a.len[r_] : a.T);
      yi = r_ * (size_t)qT + (size_t)nt;
    }
    live = live && v >= 0.0 && fabs(m) < 1e300 && v < 1e300;   // (NaN or infinite moments: no prediction)
  }

  if (a.pmean || a.pvar) {
    const double mu = exp(m + 0.5 * v);
    if (a.pmean && inside) a.pmean[e] = live ? mu : qnan;
    if (a.pvar && inside) a.pvar[e] = live ? mu + (mu * mu) * expm1(v) : qnan;
  }

  if (a.logp && inside) {
    double out = qnan;
    if (live) {
      const double k = a.counts ? (double)a.counts[e] : (double)rates_count_at(a.Y, a.Yhi, yi);
      double lam;
      const double u = counts_mode(m, v, k, 0.0, &lam);
      out = counts_logp_at(m, v, k, u, lam, a.nodes, a.Q);
    }
    a.logp[e] = out;
  }

  const bool bands = a.lower || a.upper;
  if (!a.pmf && !bands) return;                              // (uniform)

  // the walk over k = 0, 1, ...: pmf needs k < K of every lane, the quantiles k up to the lane's upper quantile, k_cap at the most
  const int K = a.pmf ? a.K : 0;
  const int kend = max(K - 1, bands ? a.k_cap : -1);         // last k any lane can need
  int lo = -1, up = -1;
  bool walking = bands && live;                              // this lane still looks for its upper quantile
  double u = 0.0, cdf = 0.0;
  const int ne = (int)min((long long)64, a.n - e0);         // entries of this workgroup
  for (int k0 = 0; k0 <= kend; k0 += COUNTS_KT) {
    if (k0 >= K && !__any(walking)) break;                   // (uniform over the wave = the workgroup)
    const int kt = min(COUNTS_KT, kend + 1 - k0);
    for (int kk = 0; kk < kt; ++kk) {
      const int k = k0 + kk;
      double p = qnan;
      const bool quant = walking && k <= a.k_cap;
      if (live && (k < K || quant)) {
        double lam;
        u = counts_mode(m, v, (double)k, u, &lam);
        p = exp(counts_logp_at(m, v, (double)k, u, lam, a.nodes, a.Q));
        if (quant) {
          cdf += p;
          if (lo < 0 && cdf >= a.p_lo) lo = k;
          if (cdf >= a.p_hi) { up = k; walking = false; }
        }
      }
      if (k0 < K) tile[lane * COUNTS_KS + kk] = p;
    }
    if (k0 < K) {                                            // (uniform) store the tile: consecutive lanes on consecutive k
      const int kw = min(COUNTS_KT, K - k0);
      __syncthreads();
      for (int f = lane; f < ne * kw; f += 64) {
        const int el = f / kw, kk = f - el * kw;
        a.pmf[(size_t)(e0 + el) * K + k0 + kk] = tile[el * COUNTS_KS + kk];
      }
      __syncthreads();                                       // the tile is reused by the next 16 values
    }
  }
  if (bands) {
    const bool saturated = walking;                          // live, and the upper quantile was not reached at k_cap
    if (saturated) { up = a.k_cap; if (lo < 0) lo = a.k_cap; }
    if (a.lower && inside) a.lower[e] = live ? lo : -1;
    if (a.upper && inside) a.upper[e] = live ? up : -1;
    const unsigned long long b = __ballot(saturated);
    if (lane == 0 && a.sat) a.sat[blockIdx.x] = (int32_t)__popcll(b);
  }
}

}  // namespace pgpfa
