// libpgpfa_hip.so - cov.hip (one translation unit of the C-ABI library; shared declarations: ctx.h)
#include "query.h"
#include "model.h"
#include "split.h"
#include "ytmix.h"
#include "hook.h"

using namespace pgpfa;

// post_vsm[t] = Gram of the rows (., t) of the panel Mt (ncol columns, column stride ld) for ns slots: matrix-core kernel beyond 10
// latents, vector kernel up to 10.  (f32: the panel is single precision)
template <typename TIN>
void launch_post_vsm(pgpfa_ctx* c, const TIN* Mt, long long sM, int ncol, int ns, int full_range, const int* roff = nullptr, int ts = 0) {
  const int T = c->T, p = c->p;
  if (ts <= 0) ts = T;                                       // row stride between latents in the panel
  if (p > 10 && c->vsm_mfma) {
    const int CB = post_vsm_mfma_cb(p, sizeof(TIN) == 4);
    if (p <= 20 && c->vsm_b4) {                              // four latents x four bins per 4 x 4 x 4 block product
      constexpr int VW = 16 / (int)sizeof(TIN);
      const bool vec = c->vsm_b4 >= 2 && T % VW == 0 && ts % VW == 0 && c->ld % VW == 0 && sM % VW == 0 && (((size_t)Mt) & 15) == 0;
      auto go = [&](auto nbk, auto vv) {
        constexpr int NBK = decltype(nbk)::value;
        constexpr bool VEC = decltype(vv)::value;
        const size_t lds4 = (size_t)CB * post_vsm_b4_cs(p, VEC) * sizeof(TIN);
        constexpr int BINS = VEC ? 64 : 32;
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&post_vsm_b4_kernel<NBK, TIN, VEC>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds4);
        hipLaunchKernelGGL((post_vsm_b4_kernel<NBK, TIN, VEC>), dim3((T + BINS - 1) / BINS, ns), dim3(512), lds4, c->st, Mt, sM, c->ld, ncol, T, p, c->vsm,
                           c->ident, c->trial_of_slot, full_range, CB, roff, (int)GBN, ts);
      };
      auto gov = [&](auto nbk) { if (vec) go(nbk, std::true_type{}); else go(nbk, std::false_type{}); };
      if (p <= 12) gov(std::integral_constant<int, 3>{}); else if (p <= 16) gov(std::integral_constant<int, 4>{}); else gov(std::integral_constant<int, 5>{});
      return;
    }
    const size_t lds = (size_t)CB * p * 33 * sizeof(TIN);
    if (p <= 16)
      hipLaunchKernelGGL((post_vsm_mfma_kernel<1, TIN>), dim3((T + 31) / 32, ns), dim3(512), lds, c->st, Mt, sM, c->ld, ncol, T, p, c->vsm, c->ident,
                         c->trial_of_slot, full_range, CB, roff, (int)GBN, ts);
    else
      hipLaunchKernelGGL((post_vsm_mfma_kernel<2, TIN>), dim3((T + 31) / 32, ns), dim3(512), lds, c->st, Mt, sM, c->ld, ncol, T, p, c->vsm, c->ident,
                         c->trial_of_slot, full_range, CB, roff, (int)GBN, ts);
    return;
  }
  const int KY = post_vsm_rows(p);
  dispatch_pmax(p, [&](auto pm) {
    hipLaunchKernelGGL((post_vsm_kernel<decltype(pm)::value, TIN>), dim3((T + 63) / 64, ns), dim3(64, KY), 0, c->st, Mt, sM, c->ld, ncol, T, p, c->vsm,
                       c->ident, c->trial_of_slot, full_range, ts);
  });
}


int post_vsm_from_mt(pgpfa_ctx* c, int nslots) {
  launch_post_vsm(c, (const double*)c->ws.Mt, (long long)c->ws.sM, c->npad, nslots, 0);
  HIPC(hipGetLastError());
  return 0;
}

// The GEMM addresses A, B and C with one slot index; post_vsmGP is indexed by trial, so the slot
// result goes through a slot-indexed staging slab and is scattered afterwards.
__global__ void scatter_vsmgp_kernel(const double* __restrict__ src, long long sSrc, double* __restrict__ dst, int T, int p, int k,
                                     const int* __restrict__ trial_of_slot) {
  const int slot = blockIdx.y;
  const size_t r = trial_of_slot[slot];
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < (size_t)T * T) {
    const size_t a = e % T, b = e / T;                 // column-major (a,b); only a >= b was computed
    dst[(r * p + k) * T * T + e] = (a >= b) ? src[(size_t)slot * sSrc + e] : src[(size_t)slot * sSrc + a * T + b];
  }
}


int ensure_mt_clean(pgpfa_ctx* c) {
  if (!c->mt_dirty) return 0;
  HIPC(hipMemsetAsync(c->ws.Mt, 0, (size_t)c->ws.sM * c->B * sizeof(double), c->st));
  c->mt_dirty = false;
  return 0;
}

// Per-trial T x T blocks live in an allocation of their own, freed only with the context: allocated lazily (often in the
// middle of an E-step, i.e. after the workspace mark), it must not be swept up by free_workspace on a re-plan.
int ensure_vsmgp_buffer(pgpfa_ctx* c) {
  if (c->vsmgp) return 0;
  const size_t bytes = (size_t)c->R * c->p * c->T * c->T * sizeof(double);
  void* ptr = nullptr;
  hipError_t e = hipMalloc(&ptr, bytes);
  if (e != hipSuccess) { (void)hipGetLastError(); return fail("hipMalloc(%zu bytes) for the per-trial post_vsmGP blocks failed: %s", bytes, hipGetErrorString(e)); }
  e = hipMemsetAsync(ptr, 0, bytes, c->st);
  if (e != hipSuccess) { hipFree(ptr); return fail("hipMemset failed: %s", hipGetErrorString(e)); }
  c->vsmgp = reinterpret_cast<double*>(ptr);
  c->bytes += bytes;
  return 0;
}

// Buffers of the Laplace log evidence (option laplace_evidence): the per-bin log-dets of the low-rank engine (shared with the dual path, which
// allocates it in ensure_lambda) and the per-slot result.  Workspace allocations: a re-plan frees them with the rest.
int ensure_evidence_buffers(pgpfa_ctx* c) {
  if (!c->ldet_buf) CHK(dmalloc(c, &c->ldet_buf, (size_t)c->B * c->T + 16));
  if (!c->evid_ld) CHK(dmalloc(c, &c->evid_ld, (size_t)c->B));
  return 0;
}

static int posterior_blocks_dense(pgpfa_ctx* c, int nb, double diag_scale, bool want_vsmgp, double* ld_dev) {
  const int T = c->T, p = c->p;
  c->info["last_cov_f32"] = 0.0;                             // (option laplace_f32 is the low-rank engine's)
  CHK(ensure_mt_clean(c));
  c->last_cov_lowrank = false;
  CHK(assemble(c, c->ident, nb, diag_scale, diag_scale != 1.0 && dual_jitter_per_trial(c)));   // (a scale other than 1: dual_dense_scale ran on these slots)
  CHK(factor(c, c->ws, c->ident, nb));
  // log det H + sum_k log det K_k of the log evidence: from the factor, before the staging of post_vsmGP reuses its slab
  if (ld_dev) {
    double ldk = 0.0;
    for (double v : c->logdetK) ldk += v;
    hipLaunchKernelGGL(evidence_logdet_kernel, dim3(nb), dim3(256), 0, c->st, (const double*)nullptr, 0, c->ws.H, (long long)c->ws.sH, c->ld, c->npad, ldk, ld_dev);
  }
  CHK(inverse_t(c, c->ws, c->ident, nb));
  if (want_vsmgp) {
    CHK(ensure_vsmgp_buffer(c));
    for (int k = 0; k < p; ++k) {
      const int kal = (k * T) / 16 * 16;
      GemmP g{};
      g.A = c->ws.Mt + (size_t)kal * c->ld + (size_t)k * T; g.sA = c->ws.sM; g.lda = c->ld;
      g.B = g.A; g.sB = c->ws.sM; g.ldb = c->ld;
      g.C = c->ws.H; g.sC = c->ws.sH; g.ldc = T;        // slot-indexed staging: the factor slab is free now
      g.M = T; g.N = T; g.K = c->npad - kal; g.alpha = 1.0; g.beta = 0.0;
      // lower tiles only (the scatter mirrors them); Mt is upper triangular, so tile (ti,tj) starts its k range
      // at max(ti,tj)*128 relative to the first column kept (kal <= k*T)
      g.slots = c->ident; g.nbatch = nb; g.mode = GEMM_LOWER; g.kflags = KF_BEGIN_MAXRC;
      CHK(gemm(c, false, g));
      hipLaunchKernelGGL(scatter_vsmgp_kernel, dim3((unsigned)(((size_t)T * T + 255) / 256), nb), dim3(256), 0, c->st, c->ws.H, c->ws.sH, c->vsmgp,
                         T, p, k, c->trial_of_slot);
    }
  }
  prof_begin(c, TAG_VSM, (double)nb * c->npad * c->npad * p);
  launch_post_vsm(c, (const double*)c->ws.Mt, (long long)c->ws.sM, c->npad, nb, 0);
  prof_end(c);
  HIPC(hipGetLastError());
  return 0;
}


constexpr int SPLIT_NS = 256;     // groups of the S sums of the split form (a partition of their own: S_k costs r_k^2 per group, not r_k T)

// Step 2 of the split form (accumulate_split; also behind pgpfa_test_split_syrk): the full-width term on the FP16 matrix cores,
//   part[(k * ngroups + g)][T x T] = sum over the slots of group g and the columns b < ract of D_k[:, b] D_k[:, b]^T   (lower 64 x 64 wave tiles),
// D_k[t, b] = D[slot * sD + (k * Ts + t) + b * ldd].  sps_req = 0: groups of max(1, ceil(nb / PACC_SPLITS)) slots.  tile_req is option syrk_tile; the
// 256 x 256 kernel runs where T spans more than one such tile and the 16-byte loads of the fast path are allowed.
static int split_syrk_launch(pgpfa_ctx* c, const float* D, long long sD, int ldd, int Ts, int T, int p, int ract, int nb, int sps_req, int tile_req, double* part,
                             int* tile_used, int* sps_out, int* ngroups_out) {
  const int sps = sps_req > 0 ? sps_req : std::max(1, (nb + PACC_SPLITS - 1) / PACC_SPLITS);
  const int ngroups = (nb + sps - 1) / sps;
  SyrkF16Args a{};
  a.D = D; a.sD = sD; a.ldd = ldd; a.ts = Ts; a.part = part;
  a.T = T; a.p = p; a.ract = ract; a.nslots = nb; a.sps = sps; a.ngroups = ngroups;
  a.dbg = c->syrk_dbg;
  // 256 x 256 tiles (half the reads of D per output) where T spans more than one of them and the 16-byte loads of the fast path are allowed
  const int t256 = (T + 255) / 256;
  const bool big = tile_req >= 256 && T > 256 && (Ts & 3) == 0 && (ldd & 3) == 0 && t256 * 256 <= Ts && (((size_t)D) & 15) == 0 && (sD & 3) == 0;
  a.tiles = big ? t256 : (T + 127) / 128; a.ntiles = a.tiles * (a.tiles + 1) / 2;
  const long long blocks = (long long)a.ntiles * ngroups * p;
  prof_begin(c, TAG_VSM, 3.0 * (double)nb * ract * T * T * p);
  if (big) {
    const size_t lds = (size_t)4 * 2 * 256 * 32 * sizeof(_Float16);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&syrk256_f16x2_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(syrk256_f16x2_kernel, dim3((unsigned)blocks), dim3(512), lds, c->st, a);
  } else {
    hipLaunchKernelGGL(syrk_f16x2_kernel, dim3((unsigned)blocks), dim3(256), 0, c->st, a);
  }
  prof_end(c);
  *tile_used = big ? 256 : 128;
  *sps_out = sps;
  *ngroups_out = ngroups;
  return 0;
}

// Step 3 of the split form for one latent (accumulate_split; also behind pgpfa_test_split_latent_sums):
//   Ssum (rk x rk, full) = sum over the slots of A_s A_s^T,   Xsum (rk x T, ld = rk) = sum over the slots of A_s D_s^T,
// A_s[i][b] = A0[s * sM + i + b * lda] (FP64, kw columns), D_s[b][t] = Dk[s * sD + b * ldd + t] (single precision).  Both as segmented-K products over
// groups of slots - S in SPLIT_NS groups, X in groups of sps slots, through cross_term_kernel in launches of 128 rows when `cross` is set and the shapes allow -
// reduced by sum_groups_kernel.  Spart holds ceil(nb / spsS) * rk^2 doubles, Xpart ceil(nb / sps) * rk * T.
static int split_latent_sums(pgpfa_ctx* c, const double* A0, long long sM, int lda, const float* Dk, long long sD, int ldd, int rk, int kw, int T, int nb, int sps,
                             bool cross, double* Spart, double* Xpart, double* Ssum, double* Xsum, int* cross_used) {
  const int ngroups = (nb + sps - 1) / sps;
  const int spsS = std::max(1, (nb + SPLIT_NS - 1) / SPLIT_NS);
  auto seg = [&](int sper, bool is_x, double* out) -> int {                   // groups of `sper` slots (the last one may be short)
    const int nfull = nb / sper, rem = nb - nfull * sper;
    for (int part = 0; part < 2; ++part) {
      const int first = part ? nfull * sper : 0, per = part ? rem : sper, ng = part ? (rem ? 1 : 0) : nfull;
      if (ng == 0 || per == 0) continue;
      GemmP g{};
      g.A = A0 + (size_t)first * sM; g.sA = (long long)per * sM; g.lda = lda;
      g.kseg = kw; g.sAseg = sM;
      g.K = per * kw; g.alpha = 1.0; g.beta = 0.0; g.slots = nullptr; g.nbatch = ng; g.kflags = 0; g.bm = 64;
      g.M = rk;
      if (is_x) {
        g.B = reinterpret_cast<const double*>(Dk + (size_t)first * sD);
        g.sB = (long long)per * sD; g.ldb = ldd; g.sBseg = sD; g.b_f32 = 1;
        g.N = T; g.mode = GEMM_FULL;
        g.C = out + (size_t)(part ? nfull : 0) * rk * T; g.sC = (long long)rk * T; g.ldc = rk;
      } else {
        g.B = g.A; g.sB = g.sA; g.ldb = lda; g.sBseg = sM;
        g.N = rk; g.mode = GEMM_LOWER;
        g.C = out + (size_t)(part ? nfull : 0) * rk * rk; g.sC = (long long)rk * rk; g.ldc = rk;
      }
      CHK(gemm(c, false, g));
    }
    return 0;
  };
  CHK(seg(spsS, false, Spart));
  // (the S sums stay with the general kernel: through cross_term_kernel<.., double, true> - lower 16 x 16 tiles only - they ran no faster)
  const bool use_cross = cross && c->mfma && rk % 16 == 0 && kw % 16 == 0;
  if (use_cross) {
    // the cross term with (up to 128) rows of the latent in one workgroup (split.h): no padded row tiles on the matrix cores
    for (int row0 = 0; row0 < rk; row0 += 128) {
      CrossArgs ca{};
      ca.A = A0; ca.sM = sM; ca.lda = lda;
      ca.D = Dk; ca.sD = sD; ca.ldd = ldd;
      ca.C = Xpart; ca.sC = (long long)rk * T;
      ca.rk = std::min(128, rk - row0); ca.T = T; ca.kw = kw; ca.nslots = nb; ca.sps = sps;
      ca.row0 = row0; ca.ldc = rk;
      prof_begin(c, TAG_GEMM, 2.0 * (double)nb * ca.rk * (double)kw * T);
      cross_term_launch<float, false>(ca, dim3((T + 63) / 64, ngroups), c->st);
      prof_end(c);
    }
    HIPC(hipGetLastError());
  } else {
    CHK(seg(sps, true, Xpart));
  }
  const int ngS = (nb + spsS - 1) / spsS;
  hipLaunchKernelGGL(sum_groups_kernel, dim3((unsigned)(((size_t)rk * rk + 63) / 64)), dim3(256), 0, c->st, Spart, ngS, rk, rk, 32, Ssum);
  hipLaunchKernelGGL(sum_groups_kernel, dim3((unsigned)(((size_t)rk * T + 63) / 64)), dim3(256), 0, c->st, Xpart, ngroups, rk, T, 0, Xsum);
  *cross_used = use_cross ? 1 : 0;
  return 0;
}

// B = I + F^T Wt F (ctx.h).  The shared preconditioner's one slot gives the grid (npairs, (1 + AB_SLOTS - 1) / AB_SLOTS) = (npairs, 1) it has always had.
// The two launches from explicit arguments (assemble_rxr passes the context's, pgpfa_test_assemble_b buffers and tables of its own): Bm with slot
// stride sB and leading dimension rpad, L and blk_lat / blk_col from the rank tables, F the slabs [p][Tf][Tf].
template <typename TB>
void assemble_rxr_launch(TB* Bm, long long sB, int rpad, int rtot, int nact, const BLayout& L, const TB* F, int Tf, int T, int p, const int* blk_lat,
                         const int* blk_col, const double* Wt, long long sW, const int* slots, int nb, hipStream_t st) {
  hipLaunchKernelGGL(assemble_b_kernel_t<TB>, dim3(L.npairs, (nb + AB_SLOTS - 1) / AB_SLOTS), dim3(256), 0, st, Bm, sB, rpad, L.nblk64, F, Tf, T, p,
                     blk_lat, blk_col, Wt, sW, slots, nb, L.cmap);
  if (L.cmap && rpad > rtot)
    hipLaunchKernelGGL(pad_identity_kernel<TB>, dim3((rpad + 3) / 4, nb), dim3(256), 0, st, Bm, sB, rpad, rtot, rpad, nact, (int)NB, slots);
}

template <typename TB>
int assemble_rxr(pgpfa_ctx* c, const CholWS& view, int nb, const TB* F, const double* Wt, long long sW, const int* slots) {
  TB* Bm = reinterpret_cast<TB*>(view.H);                  // (a single-precision view carries its strides in floats)
  assemble_rxr_launch<TB>(Bm, view.sH, c->rpad, c->rtot, view.nact, b_layout(c), F, c->Tp, c->T, c->p, c->d_blk_lat, c->d_blk_col, Wt, sW, slots, nb, c->st);
  HIPC(hipGetLastError());
  return 0;
}
template int assemble_rxr<double>(pgpfa_ctx*, const CholWS&, int, const double*, const double*, long long, const int*);
template int assemble_rxr<float>(pgpfa_ctx*, const CholWS&, int, const float*, const double*, long long, const int*);

namespace {

// Clear the L^-T slabs of `w` (T = float: the slabs viewed as floats), then L^-T.  The slab holds whatever its last use left - another rank layout, the
// factor of a dense pass -: all of it is cleared, or, with lower_ctile > 0 (FP64; every consumer starts at the latent's own columns), only the strictly
// lower entries of the p rectangles they read.
template <typename T>
int clear_and_invert(pgpfa_ctx* c, const CholWS& w, int nb, int lower_ctile = 0) {
  const int rpad = c->rpad;
  constexpr bool f32 = sizeof(T) == 4;
  if constexpr (f32)
    hipLaunchKernelGGL(fill_slabs_f32_kernel, dim3((unsigned)(((size_t)rpad * rpad + 1023) / 1024), nb), dim3(256), 0, c->st, reinterpret_cast<float*>(w.Mt), w.sM,
                       (size_t)rpad * rpad, 0.0f);
  else if (lower_ctile > 0)
    hipLaunchKernelGGL(clear_lower_reads_kernel, dim3(c->p, nb), dim3(256), 0, c->st, w.Mt, w.sM, rpad, c->d_roff, lower_ctile, c->ident);
  else
    hipLaunchKernelGGL(fill_slabs_kernel, dim3((unsigned)(((size_t)rpad * rpad + 1023) / 1024), nb), dim3(256), 0, c->st, w.Mt, w.sM, (size_t)rpad * rpad, 0.0);
  return inverse_t(c, w, c->ident, nb, f32);
}

// What one low-rank covariance pass derives from its arguments, the options and the plan, once per call.
struct CovPass {
  int nb;
  bool want_vsmgp, accumulate;
  int ract;                        // columns of Yt that are not identically zero (rpad rounds to 128 for the factor)
  long long sW;
  // sum-only accumulation by the split form (split.h)?  Decided by the relative size of the mixing correction of this chunk, max_t eps ||Wt_t||_inf,
  // measured with the per-bin blocks and read back just before the mixing pass (info key "last_eps_wt_norm")
  // (want_vsmgp passes run the FP64 engine whatever dual_f32 says - it only concerns the dual's evaluations - and under laplace_f32 everything the
  //  split form touches is FP64 as well, so the split form does not ask)
  bool split_candidate;
  unsigned* norm_bits;             // (scratch word: the inner solves are over)
  // Mixed precision (option dual_f32, dual-variational evaluations only): B, its Cholesky factor, L^-T and Yt = F L^-T - the O(T r^2) and
  // O(r^3) parts - run on the FP32 matrix cores (twice the FP64 rate, half the bytes); log det and the per-bin covariance blocks are
  // accumulated in FP64 from the single-precision factors.  (dual_f32 = 2: B is still assembled in FP64 and rounded once.)
  // Option laplace_f32 (want_vsmgp passes: the Laplace E-step and the blocks rebuilt on demand): the same single-precision B, factor and L^-T; L^-T is then
  // widened into the FP64 slab (widen_upper_f64_kernel) and everything from Yt on is the FP64 path, unchanged.  A chunk with a non-positive pivot in
  // the single-precision factorisation is redone in FP64.
  int f32_mode;
  bool f32, lap32;
  // Yt = F L^-T: L^-T is upper triangular, so the rows of Yt that belong to latent k vanish left of column roff[k].  When the consumer knows
  // the same offsets and takes those entries as zeros without reading them (the mixing pass up to 16 latents, the matrix-core post_vsm
  // beyond 10) the product skips the whole 128-column tiles left of it: ~45 % of the flops and stores.
  bool skip_zero_cols;
  // granularity of that skipping: the mixing passes take any multiple of 16 (the ranks are padded to 16, so exactly the zero columns are left
  // out: 128-column tiles kept 64 of them per latent on average - 18 % of the product and of the pass at config 3), the matrix-core post_vsm whole
  // 128-column tiles
  int ctile;
  // rows (k, t) of the Yt slab sit at k * Ts + t with Ts = T rounded up to 16 when the slab is tall enough: the 64-bin runs of the mixing pass and
  // the product's stores then start on 128-byte lines (at T = 500 every run straddled one: 1.4x the bytes fetched, PMC)
  int Ts;
  CholWS lw;                       // the dense engine's slabs as scratch, ld = rpad: B / L, then Yt in the H slabs, L^-T in the Mt slabs
  CholWS lwf;                      // single-precision views: B / L in the Mt slabs, L^-T and Yt in the H slabs
  float* Ytf;                      // Yt (float, n x ract, ld = c->ld) behind L^-T in the same slab
};

CovPass cov_pass(const pgpfa_ctx* c, int nb, bool want_vsmgp, bool accumulate, bool allow_lap32) {
  const int T = c->T, p = c->p;
  CovPass P{};
  P.nb = nb; P.want_vsmgp = want_vsmgp; P.accumulate = accumulate;
  P.ract = round_up(c->rtot, 16);
  P.sW = (long long)T * p * p;
  P.split_candidate = want_vsmgp && accumulate && c->split_cov && c->mfma && (p <= 16 || (p <= 20 && c->mix_wide));
  P.norm_bits = reinterpret_cast<unsigned*>(c->pcg_ratio);
  P.f32_mode = want_vsmgp ? (allow_lap32 ? c->laplace_f32 : 0) : c->dual_f32;
  P.f32 = P.f32_mode != 0;
  P.lap32 = P.f32 && want_vsmgp;
  P.skip_zero_cols = want_vsmgp ? p <= 16 : (p > 10 && c->vsm_mfma);
  P.ctile = (want_vsmgp && p <= 16) ? 16 : (int)GBN;
  P.Ts = (c->slab_row_align && p * round_up(T, 16) <= c->ld) ? round_up(T, 16) : T;
  P.lw = lowrank_view(c, c->ws);
  P.lwf = P.lw;
  if (P.f32) {
    P.lwf.H = P.lw.Mt; P.lwf.sH = 2 * P.lw.sM;
    P.lwf.Mt = P.lw.H; P.lwf.sM = 2 * P.lw.sH;
    P.lwf.sD = 2 * P.lw.sD; P.lwf.sP = 2 * P.lw.sP;
    P.Ytf = reinterpret_cast<float*>(P.lw.H) + (size_t)c->rpad * c->rpad;
  }
  return P;
}

// ---- the split form of the sum-only output (split.h): Pacc[k] += sum over the chunk's slots of Y~_k Y~_k^T + eps diag(G_t[k][k]) from L^-T (lw.Mt),
// Yt (lw.H) and the per-bin blocks G (c->Gbin), without the full-width FP64 product.  Also writes post_vsm.

// scratch: S parts [NS][r_k^2] | X parts [NG][r_k T] | Ssum | Xsum | Z | T1 [p][T^2] | Xfull [p][T^2]; a latent's padded rank r_k can reach
// T rounded up to 16, so the first five are laid out in units of tq = round_up(T, 16)^2
struct SplitScratch {
  double *Spart, *Xpart, *Ssum, *Xsum, *Zb, *T1, *Xfull;
  float* D;                        // the correction eps Wt Yt, behind Yt in every slot's slab
  long long sD;                    // slab stride in floats
  int ldd;
};

int split_scratch(pgpfa_ctx* c, const CholWS& lw, SplitScratch* s) {
  const int T = c->T, p = c->p;
  const size_t tt = (size_t)T * T;
  constexpr int NS = SPLIT_NS, NG = PACC_SPLITS + 1;
  const size_t tq = (size_t)round_up(T, 16) * round_up(T, 16);
  if (!c->split_buf) {
    const size_t len = ((size_t)NS + NG + 3) * tq + 2 * (size_t)p * tt + 1024;
    if (hipMalloc((void**)&c->split_buf, len * sizeof(double)) != hipSuccess) { (void)hipGetLastError(); c->split_buf = nullptr; return fail("out of device memory for the split accumulation (%zu bytes)", len * sizeof(double)); }
    c->bytes += len * sizeof(double);
  }
  s->Spart = c->split_buf;
  s->Xpart = s->Spart + (size_t)NS * tq;
  s->Ssum = s->Xpart + (size_t)NG * tq;
  s->Xsum = s->Ssum + tq;
  s->Zb = s->Xsum + tq;
  s->T1 = s->Zb + tq;
  s->Xfull = s->T1 + (size_t)p * tt;
  s->D = reinterpret_cast<float*>(lw.H + (size_t)c->ld * c->rpad);
  s->sD = 2 * (long long)lw.sH;
  s->ldd = c->ld;
  return 0;
}

// 1. mixing pass: post_vsm and the correction D = eps Wt Yt (single precision); Yt itself stays.  Returns the info key "last_mix_form": which of the
// kernels ran (4: with the product, ytmix.h - Yt was not formed; 5: mix_vsm_wide2; 3 / 2 / 1: mix_slot3 / 2 / 1; 0: mix_vsm_split).
int mix_split(pgpfa_ctx* c, const CovPass& P, const SplitScratch& s, bool fused) {
  const int T = c->T, p = c->p, Tp = c->Tp, rpad = c->rpad, nb = P.nb, ract = P.ract, Ts = P.Ts, ctile = P.ctile, ldd = s.ldd;
  const long long sW = P.sW, sD = s.sD;
  const CholWS& lw = P.lw;
  float* D = s.D;
  int mix_form = 0;
  double mix_cols = 0.0;                                   // columns of Yt a latent's rows really hold: left of its first column tile nothing was written
  for (int k = 0; k < p; ++k) mix_cols += std::max(0, ract - (ctile > 0 ? (c->roff[k] / ctile) * ctile : 0));
  // (bytes: the columns of Yt that hold something read once in FP64; D - dense, the mixing couples the latents - written once in FP32)
  if (fused) {
    // Yt was not formed: product and mixing in one kernel.  Work recorded: its FLOPs - products 2 T (ract^2 / 2 + 8 ract) over the
    // triangular panels in 16-column blocks, mixing 2 p^2 + p (p + 1) per (bin, column); info key "last_yt_mix_fused" tells the reader of
    // prof_mix_flops that these are flops, not the bytes of the stand-alone pass.
    prof_begin(c, TAG_MIX, (double)nb * T * ((double)ract * ract + 16.0 * ract + (double)ract * (2.0 * p * p + p * (p + 1.0))));
    dispatch_pw(p, [&](auto pw) {
      constexpr int PW = decltype(pw)::value;
      if constexpr (PW <= 10) {
        YtMixArgs a{};
        a.F = c->Flr; a.Tp = Tp; a.Mts = lw.Mt; a.sM = (long long)lw.sM; a.rpad = rpad;
        a.D = D; a.sD = sD; a.ldd = ldd; a.G = c->Gbin; a.sG = sW;
        a.T = T; a.p = p; a.ract = ract; a.nbx = (T + YTM_BINS - 1) / YTM_BINS; a.nslots = nb; a.eps = c->eps;
        a.vsm = c->vsm; a.slots = c->ident; a.trial_of_slot = c->trial_of_slot; a.ts = Ts; a.dbg = c->yt_mix_dbg;
        const BLayout L = b_layout(c);
        a.roff = L.roff_padded; a.cmap = L.cmap; a.nrtab = L.nrtab;
        a.ncmap = L.ncmap_rows;
        if (ytmix_lds(PW) + (size_t)a.ncmap * sizeof(int) > (size_t)160 * 1024) a.ncmap = 0;     // (the kernel then reads the map from memory)
        const size_t lds = ytmix_lds(PW) + (size_t)a.ncmap * sizeof(int);
        a.zero16 = c->zero16;
        // (the DMA form reads the row map from its LDS copy only, and moves 16 bytes from 16-byte aligned addresses: even strides, an aligned slab)
        const bool dma = c->yt_mix_dma && c->zero16 && (!a.cmap || a.ncmap > 0) && rpad % 2 == 0 && lw.sM % 2 == 0 && (reinterpret_cast<uintptr_t>(lw.Mt) & 15) == 0;
        auto launch = [&](auto kern) {
          (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
          hipLaunchKernelGGL(kern, dim3((unsigned)(a.nbx * nb)), dim3(YTM_THREADS), lds, c->st, a);
        };
        if (dma) launch(&yt_mix_kernel<PW, true>); else launch(&yt_mix_kernel<PW, false>);
      }
    });
    prof_end(c);
    mix_form = 4;
  } else {
  prof_begin(c, TAG_MIX, (double)nb * T * (mix_cols * 8.0 + (double)p * ract * 4.0));
  mix_form = p > 16 ? 5 : 0;
  if (p > 16)                                               // (17..20 latents: split_candidate admits no others beyond 16)
    hipLaunchKernelGGL((mix_vsm_wide2_kernel<20, true>), dim3((T + 63) / 64, nb), dim3(256), 0, c->st, lw.H, (long long)lw.sH, c->ld, c->Gbin, sW, T, p, ract, c->eps,
                       c->vsm, c->ident, c->trial_of_slot, Ts, c->sink, D, sD, ldd);
  else
  dispatch_pw(p, [&](auto pw) {
    constexpr int PW = decltype(pw)::value;
    if constexpr (PW <= 10) {
      if (c->mix_slot >= 3 && p == PW && ract % 4 == 0) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&mix_slot3_kernel<PW, 128, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)mix_slot_lds(PW, 128));
        hipLaunchKernelGGL((mix_slot3_kernel<PW, 128, 2>), dim3((T + 127) / 128, nb), dim3(256), mix_slot_lds(PW, 128), c->st, (const double*)lw.H, (long long)lw.sH, c->ld, D, sD, ldd,
                           c->Gbin, sW, T, ract, c->eps, c->vsm, c->ident, c->trial_of_slot, c->d_roff, ctile, Ts);
        mix_form = 3;
        return;
      }
      if (c->mix_slot >= 2 && p == PW && ract % 4 == 0) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&mix_slot2_kernel<PW, 256, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)mix_slot_lds(PW, 256));
        hipLaunchKernelGGL((mix_slot2_kernel<PW, 256, 2>), dim3((T + 255) / 256, nb), dim3(256), mix_slot_lds(PW, 256), c->st, (const double*)lw.H, (long long)lw.sH, c->ld, D, sD, ldd,
                           c->Gbin, sW, T, ract, c->eps, c->vsm, c->ident, c->trial_of_slot, c->d_roff, ctile, Ts);
        mix_form = 2;
        return;
      }
      if (c->mix_slot) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&mix_slot_kernel<PW, 256, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)mix_slot_lds(PW, 256));
        hipLaunchKernelGGL((mix_slot_kernel<PW, 256, 2>), dim3((T + 255) / 256, nb), dim3(256), mix_slot_lds(PW, 256), c->st, (const double*)lw.H, (long long)lw.sH, c->ld, D, sD, ldd,
                           c->Gbin, sW, T, p, ract, c->eps, c->vsm, c->ident, c->trial_of_slot, c->d_roff, ctile, Ts);
        mix_form = 1;
        return;
      }
    }
    if constexpr (PW <= 16)
      hipLaunchKernelGGL(mix_vsm_split_kernel<PW>, dim3((T + 63) / 64, nb), dim3(256), 0, c->st, (const double*)lw.H, (long long)lw.sH, c->ld, D, sD, ldd,
                         c->Gbin, sW, T, p, ract, c->eps, c->vsm, c->ident, c->trial_of_slot, c->d_roff, ctile, Ts);
  });
  prof_end(c);
  }
  return mix_form;
}

// 3. per latent: S_k = sum_r A A^T (r_k x r_k), X_k = sum_r A D_k^T (r_k x T) with A = rows of latent k of L^-T right of column
//    roff_k (it is upper triangular), both as segmented-K products over groups of slots (split_latent_sums); then T1 = F S F^T and Xfull = F X
int split_latent_terms(pgpfa_ctx* c, const CovPass& P, const SplitScratch& s, int sps, bool* cross_ran_out) {
  const int T = c->T, p = c->p, Tp = c->Tp, rpad = c->rpad, nb = P.nb, ract = P.ract, Ts = P.Ts, ldd = s.ldd;
  const size_t tt = (size_t)T * T;
  const long long sD = s.sD;
  const CholWS& lw = P.lw;
  float* D = s.D;
  double *Spart = s.Spart, *Xpart = s.Xpart, *Ssum = s.Ssum, *Xsum = s.Xsum, *Zb = s.Zb, *T1 = s.T1, *Xfull = s.Xfull;
  bool cross_ran = false;
  for (int k = 0; k < p; ++k) {
    // (compact rank offsets: the rk rows taken from r0 on end in the next latent's first rows - they meet zero columns of F_k in T1 and Xfull
    //  below - and the columns start at r0 rounded down to 16, so that their count stays a multiple of 16: the entries left of r0 are below the
    //  diagonal of L^-T, i.e. zeros)
    const int rk = c->rk[k], r0 = c->roff[k] & ~15;
    const int rrow = c->roff[k];
    const int kw = ract - r0;                                                   // columns of A that are not identically zero
    if (kw <= 0 || rk <= 0) {
      HIPC(hipMemsetAsync(T1 + (size_t)k * tt, 0, tt * sizeof(double), c->st));
      HIPC(hipMemsetAsync(Xfull + (size_t)k * tt, 0, tt * sizeof(double), c->st));
      continue;
    }
    const double* A0 = lw.Mt + rrow + (size_t)r0 * rpad;
    int cross_used = 0;
    CHK(split_latent_sums(c, A0, (long long)lw.sM, rpad, D + (size_t)k * Ts + (size_t)r0 * ldd, sD, ldd, rk, kw, T, nb, sps, c->cross_kernel, Spart, Xpart, Ssum, Xsum,
                          &cross_used));
    cross_ran = cross_ran || cross_used != 0;
    const double* Fk = c->Flr + (size_t)k * Tp * Tp;
    GemmP z{};                                                                  // Z = F_k S_k   (T x r_k)
    z.A = Fk; z.lda = Tp; z.B = Ssum; z.ldb = rk; z.C = Zb; z.ldc = T;
    z.M = T; z.N = rk; z.K = rk; z.alpha = 1.0; z.beta = 0.0; z.nbatch = 1; z.mode = GEMM_FULL;
    CHK(gemm(c, true, z));
    GemmP t1 = z;                                                               // T1 = Z F_k^T  (T x T)
    t1.A = Zb; t1.lda = T; t1.B = Fk; t1.ldb = Tp; t1.C = T1 + (size_t)k * tt; t1.ldc = T; t1.N = T;
    CHK(gemm(c, false, t1));
    GemmP xf = z;                                                               // Xfull = F_k X_k  (T x T)
    xf.B = Xsum; xf.ldb = rk; xf.C = Xfull + (size_t)k * tt; xf.ldc = T; xf.N = T;
    CHK(gemm(c, true, xf));
  }
  *cross_ran_out = cross_ran;
  return 0;
}

int accumulate_split(pgpfa_ctx* c, const CovPass& P, bool fused) {
  const int T = c->T, p = c->p;
  SplitScratch s{};
  CHK(split_scratch(c, P.lw, &s));
  c->info["last_mix_form"] = (double)mix_split(c, P, s, fused);
  // 2. the full-width term on the FP16 matrix cores: partial sums per (latent, group of slots) into c->ppart
  int sps = 0, ngroups = 0, tile_used = 0;
  CHK(split_syrk_launch(c, s.D, s.sD, s.ldd, P.Ts, T, p, P.ract, P.nb, 0, c->syrk_tile, c->ppart, &tile_used, &sps, &ngroups));
  c->info["last_syrk_tile"] = (double)tile_used;
  c->info["last_split_sps"] = (double)sps;
  bool cross_ran = false;
  CHK(split_latent_terms(c, P, s, sps, &cross_ran));
  c->info["last_cross_kernel"] = cross_ran ? 1.0 : 0.0;
  // 4. Pacc += eps diag + T1 - Xfull - Xfull^T + sum of the FP16 partial sums
  const int nt64 = (T + PACC_TS - 1) / PACC_TS;
  hipLaunchKernelGGL(pacc_split_reduce_kernel, dim3(nt64 * (nt64 + 1) / 2, p), dim3(256), 0, c->st, s.T1, s.Xfull, c->ppart, ngroups, c->Gbin, P.sW, P.nb, c->eps, T, c->Tp,
                     p, c->Pacc);
  HIPC(hipGetLastError());
  c->pacc_used = true;
  return 0;
}

// ---- the phases of the low-rank covariance pass, in the order posterior_blocks_lowrank_impl calls them ---------------------------------------------

// a. per-bin blocks G = (I + eps W)^-1, Wt = W G [, their log-dets]; and what the split form's verdict will need, max and mean square over the chunk's
//    bins of eps ||Wt_t||_inf
int blocks_and_norm(pgpfa_ctx* c, const CovPass& P, double* ldet) {
  CHK(bin_blocks(c, c->W, P.sW, c->Gbin, c->Wt, P.sW, P.nb, ldet));
  if (P.split_candidate || c->measure_mix) {
    HIPC(hipMemsetAsync(P.norm_bits, 0, 4 * sizeof(unsigned), c->st));
    const long long nblk = (long long)P.nb * c->T;
    hipLaunchKernelGGL(block_norm_max_kernel, dim3((unsigned)std::min<long long>((nblk * c->p + 255) / 256, 2048)), dim3(256), 0, c->st, c->Wt, nblk, c->p, c->eps,
                       P.norm_bits, reinterpret_cast<double*>(P.norm_bits + 2));
  }
  return 0;
}

// the single-precision copy of the low-rank factors, allocated on first use and converted again after every build_lowrank
int ensure_f32_factors(pgpfa_ctx* c) {
  const size_t nf = (size_t)c->Tp * c->Tp * c->p;
  if (!c->Flr32) {
    if (hipMalloc((void**)&c->Flr32, (nf + 256 * (size_t)c->Tp) * sizeof(float)) != hipSuccess) { (void)hipGetLastError(); return fail("out of device memory for the single-precision factors"); }
    c->flr32_valid = false;
  }
  if (!c->flr32_valid) {
    hipLaunchKernelGGL(cvt_f32_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, c->st, c->Flr, c->Flr32, nf);
    c->flr32_valid = true;
  }
  return 0;
}

// b. B = I + F^T Wt F into the factor slabs viewed with ld = rpad - in FP64, in FP32 (f32_mode 1), or in FP64 and rounded once (2) - and its factor
// (compact rank offsets: the tiles of B are walked in the padded index space - rtot16 rows - and stored through cmap; build_lowrank)
int assemble_and_factor(pgpfa_ctx* c, const CovPass& P) {
  const int rpad = c->rpad, nb = P.nb;
  HIPC(hipMemsetAsync(c->ws.info, 0, sizeof(int) * nb, c->st));
  if (P.f32_mode == 1) CHK(assemble_rxr<float>(c, P.lwf, nb, c->Flr32, c->Wt, P.sW, c->ident));
  else CHK(assemble_rxr<double>(c, P.lw, nb, c->Flr, c->Wt, P.sW, c->ident));
  if (!P.f32) return factor(c, P.lw, c->ident, nb);
  if (P.f32_mode != 1)
    hipLaunchKernelGGL(cvt_lower_f32_kernel, dim3((unsigned)(((size_t)rpad * rpad + 1023) / 1024), nb), dim3(256), 0, c->st, P.lw.H, P.lw.sH,
                       reinterpret_cast<float*>(P.lwf.H), P.lwf.sH, rpad);
  c->mt_dirty = true;
  // (laplace_f32: the diagonal blocks of the factorisation in FP64 registers over the single-precision slab - their 127 rank-1 steps in float cost
  //  6 x the error of the rest, and the kernel is latency-bound either way; the dual's dual_f32 keeps its arithmetic)
  return factor(c, P.lwf, c->ident, nb, true, P.lap32);
}

// log-determinants from the factor, before anything reuses its slab: ld_dev on the device, logdet_out through two read-backs (see the pass below)
int log_determinants(pgpfa_ctx* c, const CovPass& P, double* logdet_out, double* ld_dev) {
  const int T = c->T, rpad = c->rpad, nb = P.nb;
  const CholWS &lw = P.lw, &lwf = P.lwf;
  if (ld_dev) {
    if (P.f32) return fail("internal: log evidence requested from a single-precision factor");
    hipLaunchKernelGGL(evidence_logdet_kernel, dim3(nb), dim3(256), 0, c->st, (const double*)c->ldet_buf, T, lw.H, (long long)lw.sH, rpad, rpad, 0.0, ld_dev);
  }
  if (logdet_out) {
    std::vector<double> a(nb), b2(nb);
    hipLaunchKernelGGL(sum_rows_kernel, dim3(nb), dim3(256), 0, c->st, c->ldet_buf, T, c->sc_f);
    CHK(download(c, a.data(), c->sc_f, nb));
    if (P.f32)
      hipLaunchKernelGGL(logdet_batch_f32_kernel, dim3(nb), dim3(256), 0, c->st, reinterpret_cast<const float*>(lwf.H), (long long)lwf.sH, rpad, rpad,
                         c->sc_f);
    else
      hipLaunchKernelGGL(logdet_batch_kernel, dim3(nb), dim3(256), 0, c->st, lw.H, (long long)lw.sH, rpad, rpad, c->sc_f);
    CHK(download(c, b2.data(), c->sc_f, nb));
    double ldk = 0.0;
    for (double v : c->logdetK) ldk += v;
    for (int s2 = 0; s2 < nb; ++s2) logdet_out[s2] = -ldk + a[s2] + b2[s2];
  }
  return 0;
}

// c. Yt = F L^-T per latent (T x ract, ld = c->ld, rows (k, .) at k * Ts), in the element type of its three operands; column tiles left of roff[k]
// skipped under skip_zero_cols.  FP64: from the Mt slabs into the factor slab (the factor itself is dead now).
template <typename T>
int yt_product(pgpfa_ctx* c, const CovPass& P, const T* F, const T* Linv, long long sL, T* Yt, long long sY) {
  const int Tp = c->Tp, rpad = c->rpad;
  for (int k = 0; k < c->p; ++k) {
    const int c0 = P.skip_zero_cols ? (c->roff[k] / P.ctile) * P.ctile : 0;
    if (c0 >= P.ract) continue;
    GemmP g{};
    g.A = reinterpret_cast<const double*>(F + (size_t)k * Tp * Tp); g.sA = 0; g.lda = Tp;
    g.B = reinterpret_cast<const double*>(Linv + c->roff[k] + (size_t)c0 * rpad); g.sB = sL; g.ldb = rpad;     // rows roff[k].. of L^-T, K x N column-major
    g.C = reinterpret_cast<double*>(Yt + (size_t)k * P.Ts + (size_t)c0 * c->ld); g.sC = sY; g.ldc = c->ld;
    g.M = c->T; g.N = P.ract - c0; g.K = c->rk[k]; g.alpha = 1.0; g.beta = 0.0;
    g.slots = c->ident; g.nbatch = P.nb; g.mode = GEMM_FULL; g.kflags = 0;
    CHK(gemm(c, true, g, sizeof(T) == 4));
  }
  return 0;
}

// d. post_vsm[t] = eps G_t + G_t (Y_t^T Y_t) G_t from the Yt panel
template <typename TY>
int vsm_from_yt(pgpfa_ctx* c, const CovPass& P, const TY* Yt, long long sY) {
  const int T = c->T, p = c->p, nb = P.nb;
  const long long sW = P.sW;
  prof_begin(c, TAG_VSM, (double)nb * c->n * c->rpad * p);
  launch_post_vsm(c, Yt, sY, P.ract, nb, 1, P.skip_zero_cols ? c->d_roff : nullptr, P.Ts);
  prof_end(c);
  dispatch_pw(p, [&](auto pw) {
    constexpr int PW = decltype(pw)::value;
    if constexpr (PW <= 16) {
      constexpr int BT = 256 / PW;
      hipLaunchKernelGGL(vsm_finish_kernel<PW>, dim3((T + BT - 1) / BT, nb), dim3(256), 0, c->st, c->vsm, c->Gbin, sW, T, p, c->eps, c->ident,
                         c->trial_of_slot);
    } else {
      const int bins = wide_bins(p) / 2;                 // two staged blocks per bin
      hipLaunchKernelGGL(vsm_finish_wide_kernel, dim3((T + bins - 1) / bins, nb), dim3(bins * 32), wide_lds_bytes(p, bins, 2), c->st, c->vsm,
                         c->Gbin, sW, T, p, c->eps, c->ident, c->trial_of_slot, bins);
    }
  });
  return 0;
}

// The rest of a dual evaluation under dual_f32: L^-T, Yt and post_vsm from the single-precision factor.
int dual_f32_tail(pgpfa_ctx* c, const CovPass& P) {
  CHK(clear_and_invert<float>(c, P.lwf, P.nb));
  CHK(yt_product<float>(c, P, c->Flr32, reinterpret_cast<const float*>(P.lwf.Mt), P.lwf.sM, P.Ytf, P.lwf.sM));
  if (c->p > WIDE_MAX) return fail("low-rank covariance engine supports up to %d latents (p=%d)", WIDE_MAX, c->p);
  CHK(vsm_from_yt<float>(c, P, P.Ytf, P.lwf.sM));
  HIPC(hipGetLastError());
  return 0;
}

// L^-T under laplace_f32: in single precision into the H slabs (float view, cleared first as for the dual), then widened into the Mt slabs - the
// single-precision factor there is dead - before anything writes Yt or D into the H slabs.  The widening writes the zeros the FP64 path's clears would have
// left.  *redo: a pivot of the single-precision factorisation was not positive.
int lap32_inverse(pgpfa_ctx* c, const CovPass& P, bool* redo) {
  const int p = c->p, rpad = c->rpad, nb = P.nb, ctile = P.ctile;
  const CholWS &lw = P.lw, &lwf = P.lwf;
  CHK(clear_and_invert<float>(c, lwf, nb));
  const int full = (P.skip_zero_cols && c->mt_fill) ? 0 : 1;
  const bool vec = lw.sM % 2 == 0 && lw.sH % 2 == 0 && (reinterpret_cast<uintptr_t>(lw.Mt) & 15) == 0 && (reinterpret_cast<uintptr_t>(lw.H) & 15) == 0;
  prof_begin(c, TAG_MIX, (double)nb * rpad * lw.nact * 6.0);          // (bytes, roughly: the upper triangle read in FP32 and written in FP64)
  if (vec)
    hipLaunchKernelGGL(widen_upper_f64_kernel<true>, dim3((lw.nact + 3) / 4, nb), dim3(256), 0, c->st, reinterpret_cast<const float*>(lwf.Mt), (long long)lwf.sM,
                       lw.Mt, (long long)lw.sM, rpad, lw.nact, c->d_roff, p, ctile, full);
  else
    hipLaunchKernelGGL(widen_upper_f64_kernel<false>, dim3((lw.nact + 3) / 4, nb), dim3(256), 0, c->st, reinterpret_cast<const float*>(lwf.Mt), (long long)lwf.sM,
                       lw.Mt, (long long)lw.sM, rpad, lw.nact, c->d_roff, p, ctile, full);
  prof_end(c);
  HIPC(hipGetLastError());
  // B >= I in exact arithmetic, so a bad pivot needs cond(B) r 6e-8 of order one; the chunk is then redone through the FP64 path as a whole.  (The
  // host waits for the factorisation here; where the fused pass runs it would wait for the split form's verdict a few lines on anyway.)
  std::vector<int> pivot(nb, 0);
  CHK(dl_enqueue(c, pivot.data(), c->ws.info, sizeof(int) * nb));
  CHK(dl_flush(c));
  *redo = std::any_of(pivot.begin(), pivot.end(), [](int v) { return v != 0; });
  if (*redo) c->info["last_cov_f32_fallbacks"] += 1.0;
  return 0;
}

// The split form's verdict: the relative size of the mixing correction, measured when the chunk's blocks were formed.  The host waits for it.
int split_verdict(pgpfa_ctx* c, const CovPass& P, bool* split) {
  *split = false;
  if (!(P.split_candidate || c->measure_mix)) return 0;
  unsigned hw[4] = {0u, 0u, 0u, 0u};
  CHK(dl_enqueue(c, hw, P.norm_bits, 4 * sizeof(unsigned)));
  CHK(dl_flush(c));
  float hv;
  double hsq;
  std::memcpy(&hv, &hw[0], sizeof(float));
  std::memcpy(&hsq, &hw[2], sizeof(double));
  const double rms = std::sqrt(hsq / std::max(1.0, (double)P.nb * c->T));
  c->info["last_eps_wt_norm"] = std::max(c->info["last_eps_wt_norm"], (double)hv);
  c->info["last_eps_wt_rms"] = std::max(c->info["last_eps_wt_rms"], rms);
  // (the precision of the split form follows the root mean square of the correction; the maximum only has to stay a contraction)
  *split = P.split_candidate && std::isfinite(hv) && std::isfinite(rms) && rms <= c->split_max_norm && (double)hv <= 0.9;
  return 0;
}

// d+e. one pass over Yt: post_vsm[t] = eps G_t + sum_b (G_t y_b)(G_t y_b)^T, and Yt is mixed in place (y <- G_t y) so that
//      rows (k,.) of the slab become Ymix_k, the GEMM operand of post_vsmGP_k = eps diag(G_t[k][k]) + Ymix_k Ymix_k^T
int mix_in_place(pgpfa_ctx* c, const CovPass& P) {
  const int T = c->T, p = c->p, nb = P.nb, ract = P.ract, ctile = P.ctile, Ts = P.Ts;
  const long long sW = P.sW;
  const CholWS& lw = P.lw;
  prof_begin(c, TAG_MIX, (double)nb * c->n * ract * 16.0);           // (bytes: Yt read and written in place)
  dispatch_pw(p, [&](auto pw) {
    constexpr int PW = decltype(pw)::value;
    if constexpr (PW <= 16) {
      hipLaunchKernelGGL(mix_vsm_kernel<PW>, dim3((T + 63) / 64, nb), dim3(256), 0, c->st, lw.H, lw.sH, c->ld, c->Gbin, sW, T, p, ract, c->eps,
                         c->vsm, c->ident, c->trial_of_slot, c->d_roff, ctile, Ts);
    } else if (c->mix_wide && p <= 20) {
      hipLaunchKernelGGL((mix_vsm_wide2_kernel<20, false>), dim3((T + 63) / 64, nb), dim3(256), 0, c->st, lw.H, (long long)lw.sH, c->ld, c->Gbin, sW, T, p, ract, c->eps,
                         c->vsm, c->ident, c->trial_of_slot, Ts, c->sink, (float*)nullptr, 0LL, 0);
    } else {
      const int bins = wide_bins(p);
      hipLaunchKernelGGL(mix_vsm_wide_kernel, dim3((T + bins - 1) / bins, nb), dim3(bins * 32), wide_lds_bytes(p, bins, 1), c->st, lw.H, lw.sH,
                         c->ld, c->Gbin, sW, T, p, ract, c->eps, c->vsm, c->ident, c->trial_of_slot, bins, Ts);
    }
  });
  prof_end(c);
  return 0;
}

// sum-only output: Pacc[k] += sum over the chunk's slots of Ymix_k Ymix_k^T as ONE split-K product per launch -
// batch = (latent, group of `sps` consecutive slots), the K dimension walks the rpad-wide panels of the
// group's slabs - followed by a reduction of the partial products (+ the eps G_t[k][k] diagonals)
int pacc_sum(pgpfa_ctx* c, const CovPass& P) {
  const int T = c->T, p = c->p, nb = P.nb, ract = P.ract;
  const CholWS& lw = P.lw;
  const int sps = std::max(1, (nb + PACC_SPLITS - 1) / PACC_SPLITS);
  const int nfull = nb / sps, rem = nb - nfull * sps, nsplit = nfull + (rem ? 1 : 0);
  auto launch = [&](int first_slot, int slots_per, int ngroups, int part_first) -> int {
    GemmP g{};
    g.A = lw.H + (size_t)first_slot * lw.sH; g.sA = (long long)slots_per * lw.sH; g.lda = c->ld;
    g.B = g.A; g.sB = g.sA; g.ldb = c->ld;
    g.C = c->ppart + (size_t)part_first * T * T; g.sC = (long long)T * T; g.ldc = T;
    g.M = T; g.N = T; g.K = slots_per * ract; g.alpha = 1.0; g.beta = 0.0;
    g.slots = nullptr; g.nb_lo = ngroups; g.nbatch = ngroups * p;
    g.sA_hi = P.Ts; g.sB_hi = P.Ts; g.sC_hi = (long long)nsplit * T * T;
    g.kseg = ract; g.sAseg = lw.sH; g.sBseg = lw.sH;    // ract columns of each slab, slabs sH apart
    g.mode = GEMM_LOWER; g.kflags = 0;
    return gemm(c, false, g);
  };
  if (nfull) CHK(launch(0, sps, nfull, 0));
  if (rem) CHK(launch(nfull * sps, rem, 1, nfull));
  hipLaunchKernelGGL(pacc_reduce_kernel, dim3(T, p), dim3(128), 0, c->st, c->ppart, nsplit, c->Gbin, P.sW, nb, c->eps, T, c->Tp, p, c->Pacc);
  c->pacc_used = true;
  return 0;
}

// per-trial output: post_vsmGP_k of every slot from the mixed panel, through a staging block behind Yt
int trial_blocks(pgpfa_ctx* c, const CovPass& P) {
  const int T = c->T, p = c->p, rpad = c->rpad, nb = P.nb;
  const CholWS& lw = P.lw;
  CHK(ensure_vsmgp_buffer(c));
  const size_t off_stage = (size_t)c->ld * rpad + (size_t)c->Tp * rpad;
  for (int k = 0; k < p; ++k) {
    GemmP g{};
    g.A = lw.H + (size_t)k * P.Ts; g.sA = lw.sH; g.lda = c->ld;
    g.B = g.A; g.sB = lw.sH; g.ldb = c->ld;
    g.C = lw.H + off_stage; g.sC = lw.sH; g.ldc = T;
    g.M = T; g.N = T; g.K = P.ract; g.alpha = 1.0; g.beta = 0.0;
    g.slots = c->ident; g.nbatch = nb; g.mode = GEMM_LOWER; g.kflags = 0;
    CHK(gemm(c, false, g));
    hipLaunchKernelGGL(scatter_vsmgp_lr_kernel, dim3((unsigned)(((size_t)T * T + 255) / 256), nb), dim3(256), 0, c->st, lw.H + off_stage, lw.sH, T,
                       c->vsmgp, T, p, k, c->Gbin, P.sW, c->eps, c->trial_of_slot);
  }
  return 0;
}

}  // namespace

// Covariance blocks through the low-rank form of the prior (see model.h): per slot an r x r SPD system
// B = I + F^T Wt F instead of the n x n Hessian.  Uses the dense engine's slabs as scratch (ld = rpad views).  The phases, in DESIGN section 3's order:
// logdet_out (optional, host, nb entries): log det of the posterior precision K^-1 + scatter(W) of every slot,
//   = -sum_k log det K_k + sum_t log det(I + eps W_t) + log det(I + F^T Wt F)   (Sylvester; K_k = eps I + F_k F_k^T)
// (allow_lap32 = false: the FP64 pass that redoes a chunk whose single-precision factorisation failed under option laplace_f32)
// ld_dev (optional, device, nb entries; the Laplace log evidence): log det of the posterior precision + sum_k log det K_k = the last two terms above,
//   reduced per slot by one kernel behind the factorisation; nothing is read back here.  FP64 factor only: the E-step refuses it under laplace_f32.
static int posterior_blocks_lowrank_impl(pgpfa_ctx* c, int nb, bool want_vsmgp, bool accumulate, double* logdet_out, bool allow_lap32, double* ld_dev) {
  c->last_cov_lowrank = true;
  const CovPass P = cov_pass(c, nb, want_vsmgp, accumulate, allow_lap32);
  CHK(blocks_and_norm(c, P, (logdet_out || ld_dev) ? c->ldet_buf : nullptr));                  // a.
  c->info["last_cov_f32"] = P.lap32 ? 1.0 : 0.0;
  if (P.f32) CHK(ensure_f32_factors(c));
  CHK(assemble_and_factor(c, P));                                                               // b.
  CHK(log_determinants(c, P, logdet_out, ld_dev));
  c->mt_dirty = true;
  if (P.f32 && !P.lap32) return dual_f32_tail(c, P);
  if (P.lap32) {
    bool redo = false;
    CHK(lap32_inverse(c, P, &redo));
    if (redo) return posterior_blocks_lowrank_impl(c, nb, want_vsmgp, accumulate, logdet_out, false, ld_dev);
  } else {
    CHK(clear_and_invert<double>(c, P.lw, nb, (P.skip_zero_cols && c->mt_fill) ? P.ctile : 0));
  }
  if (c->p > WIDE_MAX) return fail("low-rank covariance engine supports up to %d latents (p=%d)", WIDE_MAX, c->p);
  // c. Yt = F L^-T.  Under the split form Yt has one consumer, the mixing pass: up to 10 latents the two run as one kernel (ytmix.h) and Yt is never
  // written.  That needs the verdict before the product is queued instead of behind it (the host then waits for the factorisation: one launch gap per chunk).
  // (compact offsets: the last column block of Yt is partly padding - identity columns of L^-T meeting no row of F: zeros)
  const bool fuse_candidate = P.split_candidate && c->yt_mix && c->mfma && c->p <= 10 && (P.ract == c->rtot || (c->rank_compact && P.ract <= P.lw.nact));
  bool split = false;
  if (fuse_candidate) CHK(split_verdict(c, P, &split));
  const bool fused = fuse_candidate && split;
  c->info["last_yt_mix_fused"] = fused ? 1.0 : 0.0;
  if (!fused) CHK(yt_product<double>(c, P, c->Flr, P.lw.Mt, P.lw.sM, P.lw.H, P.lw.sH));
  if (!fuse_candidate) CHK(split_verdict(c, P, &split));
  c->info["last_split_cov"] = split ? 1.0 : 0.0;
  if (!split) for (const char* key : {"last_syrk_tile", "last_split_sps", "last_cross_kernel", "last_mix_form"}) c->info[key] = 0.0;
  // d, e. post_vsm and the T x T output: summed by the split form, or summed / per trial from the panel mixed in place; post_vsm alone for the dual
  if (!want_vsmgp) CHK(vsm_from_yt<double>(c, P, P.lw.H, P.lw.sH));
  else if (split) CHK(accumulate_split(c, P, fused));
  else {
    CHK(mix_in_place(c, P));
    CHK(accumulate ? pacc_sum(c, P) : trial_blocks(c, P));
  }
  HIPC(hipGetLastError());
  return 0;
}

int posterior_blocks_lowrank(pgpfa_ctx* c, int nb, bool want_vsmgp, bool accumulate, double* logdet_out, double* ld_dev) {
  return posterior_blocks_lowrank_impl(c, nb, want_vsmgp, accumulate, logdet_out, true, ld_dev);
}

int posterior_blocks(pgpfa_ctx* c, int nb, double diag_scale, bool want_vsmgp, bool accumulate, double* ld_dev) {
  if (c->plan_lowrank) {
    if (diag_scale != 1.0) return fail("internal: jittered covariance requested under the low-rank workspace plan");
    return posterior_blocks_lowrank(c, nb, want_vsmgp, accumulate, nullptr, ld_dev);
  }
  return posterior_blocks_dense(c, nb, diag_scale, want_vsmgp, ld_dev);
}


// Steps a - b of the covariance passes alone, for pgpfa_posterior_sample (psample.hip): from the curvature blocks c->W of the slots [0, nb) to L^-T, in
// FP64 whatever laplace_f32 / dual_f32 say.  Low-rank plan: G_t into c->Gbin, and L^-T of B = I + F^T Wt F (rpad x rpad, ld = rpad, upper triangular,
// the rest of the square cleared) into the Mt slabs.  Dense plan: L^-T of the Hessian (npad x npad, ld = c->ld) into the Mt slabs.  No posterior output
// and no info key is written; the caller clears and reads ws.info.
int posterior_factor_only(pgpfa_ctx* c, int nb, double diag_scale) {
  if (!c->plan_lowrank) {
    CHK(ensure_mt_clean(c));
    CHK(assemble(c, c->ident, nb, diag_scale, diag_scale != 1.0 && dual_jitter_per_trial(c)));   // (a scale other than 1: dual_dense_scale ran on these slots)
    CHK(factor(c, c->ws, c->ident, nb));
    CHK(inverse_t(c, c->ws, c->ident, nb));
    HIPC(hipGetLastError());
    return 0;
  }
  if (diag_scale != 1.0) return fail("internal: jittered factor requested under the low-rank workspace plan");
  if (c->p > WIDE_MAX) return fail("low-rank covariance engine supports up to %d latents (p=%d)", WIDE_MAX, c->p);
  const long long sW = (long long)c->T * c->p * c->p;
  CHK(bin_blocks(c, c->W, sW, c->Gbin, c->Wt, sW, nb, nullptr));
  const CholWS lw = lowrank_view(c, c->ws);
  CHK(assemble_rxr<double>(c, lw, nb, c->Flr, c->Wt, sW, c->ident));
  CHK(factor(c, lw, c->ident, nb));
  c->mt_dirty = true;
  CHK(clear_and_invert<double>(c, lw, nb));
  HIPC(hipGetLastError());
  return 0;
}

static int get_rows(pgpfa_ctx* c, int n, const int32_t* idx, const double* src, size_t len, double* out) {
  if (!c || !out) return fail("null argument");
  HIPC(hipSetDevice(c->device));
  Trials tr;
  CHK(resolve_trials(c, n, idx, &tr));
  for (size_t i = 0; i < tr.v.size(); ++i)
    CHK(dl_enqueue(c, out + i * len, src + (size_t)tr.v[i] * len, len * sizeof(double)));
  CHK(dl_flush(c));
  return 0;
}
int pgpfa_get_post_mean(pgpfa_ctx* c, int n, const int32_t* idx, double* out) { return get_rows(c, n, idx, c ? c->Xmode : nullptr, c ? (size_t)c->n : 0, out); }
int pgpfa_get_post_vsm(pgpfa_ctx* c, int n, const int32_t* idx, double* out) {
  return get_rows(c, n, idx, c ? c->vsm : nullptr, c ? (size_t)c->T * c->p * c->p : 0, out);
}

// Rebuild the per-trial T x T blocks of trials whose last E-step ran sum-only: covariance blocks at the resident
// modes, under the parameters of that E-step (restored around the call when an M-step has moved on since).

// The curvature of one chunk of them (ctx.h; shared with pgpfa_posterior_sample).
// (dual: the trials' posterior is the dual-variational one - curvature blocks W_t = C^T diag(lambda_t) C from the kept lambda, with the
// reference's jitter, instead of the Laplace curvature at the mode)
int resident_curvature(pgpfa_ctx* c, const std::vector<int>& tos, bool dual, const char* where, const std::function<int(double diag_scale)>& finish) {
  const int nb = (int)tos.size();
  const size_t m = (size_t)c->q * c->T;
  CHK(upload_list(c, c->trial_of_slot, tos));
  HIPC(hipMemsetAsync(c->ws.info, 0, sizeof(int) * nb, c->st));
  double scale = 1.0;
  if (dual) {
    for (int s = 0; s < nb; ++s)
      HIPC(hipMemcpyAsync(c->lamd + (size_t)s * m, c->lam_keep + (size_t)tos[s] * m, m * sizeof(double), hipMemcpyDeviceToDevice, c->st));
    std::vector<double> sB, sD, vKv;
    CHK(dual_common(c, nb, &sB, &sD, &vKv));
    if (c->plan_lowrank) CHK(dual_jitter(c, nb));
    else CHK(dual_dense_scale(c, nb, &scale));
  } else {
    hipLaunchKernelGGL(gather_rows_kernel, dim3((c->n + 255) / 256, nb), dim3(256), 0, c->st, c->Xmode, c->n, c->Xc, (long long)c->ld,
                       c->trial_of_slot, 0);
    CHK(poisson(c, c->ident, nb, c->Xc, c->Gl, c->W, c->sc_f, 1));
  }
  CHK(finish(scale));
  std::vector<int> info(nb);
  CHK(dl_enqueue(c, info.data(), c->ws.info, sizeof(int) * nb));
  CHK(dl_flush(c));
  for (int s = 0; s < nb; ++s)
    if (info[s] != 0) return fail("posterior precision of trial %d is not positive definite at the resident %s", tos[s], where);
  return 0;
}

static int materialize_impl(pgpfa_ctx* c, const std::vector<int>& need, bool dual) {
  CHK(ready_estep(c, dual ? c->dual_lowrank : true));
  if (dual) CHK(ensure_lambda(c));
  const int N = (int)need.size();
  for (int c0 = 0; c0 < N; c0 += c->B) {
    const int nb = std::min(c->B, N - c0);
    const std::vector<int> tos(need.begin() + c0, need.begin() + c0 + nb);
    CHK(resident_curvature(c, tos, dual, "mode", [&](double scale) { return posterior_blocks(c, nb, scale, true, false); }));
    for (int t : tos) c->vsmgp_ok[t] = 1;
  }
  return 0;
}

int ensure_trial_vsmgp(pgpfa_ctx* c, const std::vector<int>& trials) {
  // trials whose blocks are not resident, each once, rebuilt under the E-step (parameter snapshot) that produced their posterior
  std::vector<int> need;
  for (int t : trials) {
    if (c->vsmgp_ok[t]) continue;
    if (c->trial_snap[t] < 0) return fail("post_vsmGP of trial %d is not resident: no E-step or pgpfa_set_posterior produced it", t);
    if (std::find(need.begin(), need.end(), t) == need.end()) need.push_back(t);
  }
  return for_snapshot_groups(c, need, [&](const std::vector<int>& pos, bool dual) {
    std::vector<int> v;
    for (int i : pos) v.push_back(need[i]);
    return materialize_impl(c, v, dual);
  });
}

int pgpfa_get_post_vsmgp(pgpfa_ctx* c, int n, const int32_t* idx, double* out) {
  if (!c || !out) return fail("null argument");
  HIPC(hipSetDevice(c->device));
  Trials tr;
  CHK(resolve_trials(c, n, idx, &tr));
  CHK(ensure_vsmgp_buffer(c));
  CHK(ensure_trial_vsmgp(c, tr.v));
  const size_t len = (size_t)c->T * c->T * c->p;
  double* tmp = nullptr;
  HIPC(hipMalloc((void**)&tmp, len * sizeof(double)));
  for (size_t i = 0; i < tr.v.size(); ++i) {
    hipLaunchKernelGGL(vsmgp_to_ref_kernel, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, c->st, c->vsmgp + (size_t)tr.v[i] * len, tmp, c->T, c->p);
    hipMemcpyAsync(out + i * len, tmp, len * sizeof(double), hipMemcpyDeviceToHost, c->st);
    hipStreamSynchronize(c->st);
  }
  hipFree(tmp);
  HIPC(hipGetLastError());
  return 0;
}

static int post_cov_impl(pgpfa_ctx* c, int trial, double* out) {
  CHK(ready(c));
  std::vector<int> tr{trial};
  CHK(upload_list(c, c->trial_of_slot, tr));
  HIPC(hipMemsetAsync(c->ws.info, 0, sizeof(int), c->st));
  hipLaunchKernelGGL(gather_rows_kernel, dim3((c->n + 255) / 256, 1), dim3(256), 0, c->st, c->Xmode, c->n, c->Xc, (long long)c->ld, c->trial_of_slot, 0);
  CHK(poisson(c, c->ident, 1, c->Xc, c->Gl, c->W, c->sc_f, 1));
  CHK(ensure_mt_clean(c));
  CHK(assemble(c, c->ident, 1));
  CHK(factor(c, c->ws, c->ident, 1));
  CHK(inverse_t(c, c->ws, c->ident, 1));
  GemmP g{};
  g.A = c->ws.Mt; g.sA = c->ws.sM; g.lda = c->ld;
  g.B = c->ws.Mt; g.sB = c->ws.sM; g.ldb = c->ld;
  g.C = c->ws.H; g.sC = c->ws.sH; g.ldc = c->ld;
  g.M = c->npad; g.N = c->npad; g.K = c->npad; g.alpha = 1.0; g.beta = 0.0;
  g.slots = c->ident; g.nbatch = 1; g.mode = GEMM_FULL; g.kflags = KF_BEGIN_MAXRC;
  CHK(gemm(c, false, g));
  HIPC(hipMemcpy2DAsync(out, (size_t)c->n * sizeof(double), c->ws.H, (size_t)c->ld * sizeof(double), (size_t)c->n * sizeof(double), c->n,
                        hipMemcpyDeviceToHost, c->st));
  HIPC(hipStreamSynchronize(c->st));
  return 0;
}

// Dense posterior covariance of one trial at its resident mode, under the parameters of the E-step that produced that mode (they are
// restored around the call when later calls have moved the context on).
int pgpfa_get_post_cov(pgpfa_ctx* c, int trial, double* out) {
  if (!c || !out) return fail("null argument");
  if (trial < 0 || trial >= c->R) return fail("trial %d out of range", trial);
  if (!c->have_params) return fail("set_params has not been called");
  return with_snapshot(c, c->trial_snap[trial], [&]() { return (c->trial_dual[trial] && c->lam_keep) ? post_cov_dual_impl(c, trial, out) : post_cov_impl(c, trial, out); });
}

int pgpfa_set_posterior(pgpfa_ctx* c, int n, const int32_t* idx, const double* post_mean, const double* post_vsm, const double* post_vsmgp) {
  if (!c || !post_mean || !post_vsm) return fail("null argument");
  HIPC(hipSetDevice(c->device));
  Trials tr;
  CHK(resolve_trials(c, n, idx, &tr, true));
  const size_t lm = c->n, lv = (size_t)c->T * c->p * c->p, lg = (size_t)c->T * c->T * c->p;
  double* tmp = nullptr;
  if (post_vsmgp) CHK(ensure_vsmgp_buffer(c));
  if (post_vsmgp) HIPC(hipMalloc((void**)&tmp, lg * sizeof(double)));
  for (size_t i = 0; i < tr.v.size(); ++i) {
    const size_t r = tr.v[i];
    hipMemcpyAsync(c->Xmode + r * lm, post_mean + i * lm, lm * sizeof(double), hipMemcpyHostToDevice, c->st);
    hipMemcpyAsync(c->vsm + r * lv, post_vsm + i * lv, lv * sizeof(double), hipMemcpyHostToDevice, c->st);
    if (post_vsmgp) {
      hipMemcpyAsync(tmp, post_vsmgp + i * lg, lg * sizeof(double), hipMemcpyHostToDevice, c->st);
      hipLaunchKernelGGL(vsmgp_from_ref_kernel, dim3((unsigned)((lg + 255) / 256)), dim3(256), 0, c->st, tmp, c->vsmgp + r * lg, c->T, c->p);
      hipStreamSynchronize(c->st);
    }
  }
  hipStreamSynchronize(c->st);
  if (tmp) hipFree(tmp);
  HIPC(hipGetLastError());
  for (int t : tr.v) { c->vsmgp_ok[t] = 1; c->mode_serial[t] = -10; c->trial_snap[t] = -1; c->trial_dual[t] = 0; }   // whatever the caller provided (or left) is the resident value
  return remember_trials(c, tr.v);
}



// ---- test hooks: steps 2 and 3 of the split covariance sum on caller data, through the launch code above ------------------------------
// (device buffers, prefilled outputs and the band behind them: hook.h)
using namespace hook;

int pgpfa_test_split_syrk(pgpfa_ctx* c, int nslots, int T, int p, int ract, int ldd, int ts, int sps, int tile, const float* D, double* part, int* tile_used,
                          int* ngroups) {
  if (!c || !D || !part || !tile_used || !ngroups) return fail("null argument");
  if (nslots < 1 || T < 1 || p < 1 || ract < 1 || sps < 0) return fail("invalid sizes");
  if (ts < T) return fail("latent stride ts = %d below T = %d", ts, T);
  if ((long long)ldd < (long long)p * ts) return fail("column stride ldd = %d below p ts = %lld", ldd, (long long)p * ts);
  if (tile != 128 && tile != 256) return fail("tile must be 128 or 256");
  const int ract_alloc = round_up(ract, 32);
  const size_t slot = (size_t)ract_alloc * ldd;
  if (slot * sizeof(float) >= ((size_t)1 << 31)) return fail("a slot of D exceeds the 32-bit offsets of the buffer loads");
  const int sps_eff = sps > 0 ? sps : std::max(1, (nslots + PACC_SPLITS - 1) / PACC_SPLITS);
  const int ng = (nslots + sps_eff - 1) / sps_eff;
  const size_t np = (size_t)p * ng * T * T;
  HIPC(hipSetDevice(c->device));
  HIPC(hipStreamSynchronize(c->st));
  HookBuffers hb;
  float* dD = nullptr;
  double* dpart = nullptr;
  CHK(hb.get(&dD, slot * nslots, 1024));
  HIPC(hipMemcpy(dD, D, slot * nslots * sizeof(float), hipMemcpyHostToDevice));
  CHK(hook_output(hb, &dpart, part, np));
  int sps_used = 0;
  CHK(split_syrk_launch(c, dD, (long long)slot, ldd, ts, T, p, ract, nslots, sps, tile, dpart, tile_used, &sps_used, ngroups));
  HIPC(hipGetLastError());
  HIPC(hipStreamSynchronize(c->st));
  return hook_collect("pgpfa_test_split_syrk", dpart, part, np);
}

int pgpfa_test_split_latent_sums(pgpfa_ctx* c, int nslots, int rk, int kw, int T, int lda, long long sM, int row_off, int ldd, long long sD, int sps, int cross_kernel,
                                 const double* A, const float* D, double* Ssum, double* Xsum) {
  if (!c || !A || !D || !Ssum || !Xsum) return fail("null argument");
  if (nslots < 1 || T < 1 || rk < 1 || kw < 1 || sps < 0 || row_off < 0) return fail("invalid sizes");
  if (rk % 16 != 0) return fail("rk = %d is no multiple of 16", rk);
  if (kw % 16 != 0) return fail("kw = %d is no multiple of 16", kw);
  if (lda < row_off + rk) return fail("lda = %d below row_off + rk = %d", lda, row_off + rk);
  if (ldd < T) return fail("ldd = %d below T = %d", ldd, T);
  if (sM < (long long)kw * lda || sD < (long long)kw * ldd) return fail("slot strides below kw columns");
  if (!c->mfma) return fail("the split form runs on the matrix cores (use_mfma = 1)");
  const int sps_eff = sps > 0 ? sps : std::max(1, (nslots + PACC_SPLITS - 1) / PACC_SPLITS);
  const int ng = (nslots + sps_eff - 1) / sps_eff;
  const int spsS = std::max(1, (nslots + SPLIT_NS - 1) / SPLIT_NS), ngS = (nslots + spsS - 1) / spsS;
  HIPC(hipSetDevice(c->device));
  HIPC(hipStreamSynchronize(c->st));
  HookBuffers hb;
  double *dA = nullptr, *dSp = nullptr, *dXp = nullptr, *dS = nullptr, *dX = nullptr;
  float* dD = nullptr;
  CHK(hb.get(&dA, (size_t)sM * nslots, 4096));
  CHK(hb.get(&dD, (size_t)sD * nslots, 4096));
  CHK(hb.get(&dSp, (size_t)ngS * rk * rk, 1024));
  CHK(hb.get(&dXp, (size_t)ng * rk * T, 1024));
  HIPC(hipMemcpy(dA, A, (size_t)sM * nslots * sizeof(double), hipMemcpyHostToDevice));
  HIPC(hipMemcpy(dD, D, (size_t)sD * nslots * sizeof(float), hipMemcpyHostToDevice));
  CHK(hook_output(hb, &dS, Ssum, (size_t)rk * rk));
  CHK(hook_output(hb, &dX, Xsum, (size_t)rk * T));
  int cross_used = 0;
  CHK(split_latent_sums(c, dA + row_off, sM, lda, dD, sD, ldd, rk, kw, T, nslots, sps_eff, cross_kernel != 0, dSp, dXp, dS, dX, &cross_used));
  HIPC(hipGetLastError());
  HIPC(hipStreamSynchronize(c->st));
  if ((cross_kernel != 0) != (cross_used != 0)) return fail("internal: the cross term did not take the requested form");
  CHK(hook_collect("pgpfa_test_split_latent_sums (S)", dS, Ssum, (size_t)rk * rk));
  return hook_collect("pgpfa_test_split_latent_sums (X)", dX, Xsum, (size_t)rk * T);
}

// ---- test hook: B = I + F^T Wt F on caller data, through rank_layout, b_layout_of and assemble_rxr_launch ------------------------------------------
// What the kernels read past their logical inputs (assemble_b_kernel_t walks the bins in chunks of 32, a thread per bin of the chunk):
//  * F: rows up to round_up(T, 32) - 1 of every column [0, rk_l) of a latent's slab - unguarded loads, met by weights that the guard `bin < T` made
//    zero.  With Tf >= round_up(T, 32) (refused otherwise) and rk_l <= round_up(T, 16) <= Tf (a rank above T is refused) they stay inside the slab;
//    the slabs still get 128 elements of `fill` behind them.  Rows [T, Tf) of a column hold what the caller put there: any FINITE value.
//  * Wt: bins < T of the listed slots only (guarded), block (la, lb) of the p x p matrix of a bin; nothing behind it.  128 elements of `fill` behind it.
//  * the tables: blk_lat / blk_col entries [0, 4 nblk64), cmap entries [0, 64 nblk64) - both at most round_up(rtot16, 128), their lengths.
// What they write: assemble_b_kernel_t entries (row >= col) < rtot of the compact space (without cmap: < rpad), pad_identity_kernel rows [rtot, rpad).
namespace {
int asmb_refuse(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  (void)fail("pgpfa_test_assemble_b refuses: %s", buf);
  return code;
}
}  // namespace

int pgpfa_test_assemble_b(pgpfa_ctx* c, int p, int T, int Tf, const int32_t* ranks, int gran, int f32, int nslots, int nlist, const int32_t* list, long long sW,
                          double fill, const double* F, const double* Wt, void* B, int rpad_expected, int32_t* geom, int tab_cap, int32_t* blk_lat,
                          int32_t* blk_col, int32_t* cmap, int32_t* ntab) {
  if (!c || !ranks || !list || !F || !Wt || !B || !geom || !blk_lat || !blk_col || !cmap || !ntab) return asmb_refuse(PGPFA_ASMB_BAD_ARG, "null argument");
  if (p < 1 || p > 32 || T < 1 || nslots < 1 || nlist < 1 || tab_cap < 1) return asmb_refuse(PGPFA_ASMB_BAD_ARG, "invalid sizes");
  if (gran != 4 && gran != 8 && gran != 16) return asmb_refuse(PGPFA_ASMB_BAD_ARG, "rank granularity %d (4, 8 or 16)", gran);
  if (Tf < round_up(T, AB_TK) || Tf > 4096)
    return asmb_refuse(PGPFA_ASMB_REFUSED_TF, "slab size Tf = %d below round_up(T, %d) = %d (the bins are read in whole chunks), or above 4096", Tf, AB_TK, round_up(T, AB_TK));
  for (int k = 0; k < p; ++k)
    if (ranks[k] < 1 || ranks[k] > T) return asmb_refuse(PGPFA_ASMB_REFUSED_RANK, "rank %d of latent %d outside 1..T = %d", ranks[k], k, T);
  {
    std::vector<char> seen(nslots, 0);
    for (int i = 0; i < nlist; ++i) {
      if (list[i] < 0 || list[i] >= nslots) return asmb_refuse(PGPFA_ASMB_REFUSED_LIST, "slot list entry %d = %d outside the %d slots", i, list[i], nslots);
      if (seen[list[i]]) return asmb_refuse(PGPFA_ASMB_REFUSED_LIST, "slot list names slot %d twice", list[i]);
      seen[list[i]] = 1;
    }
  }
  const long long wbin = (long long)T * p * p;
  if (sW == 0 ? nslots != 1 : sW < wbin)
    return asmb_refuse(PGPFA_ASMB_REFUSED_STRIDE, "weight stride sW = %lld below T p^2 = %lld (0: one shared slot, with nslots = 1)", sW, wbin);
  std::vector<int> r(ranks, ranks + p);
  const RankLayout rl = rank_layout(p, r.data(), gran, true);
  if (rl.bad_pair >= 0) return fail("rank tables: padded rows %d, %d are no pair the panel staging can move whole", rl.bad_pair, rl.bad_pair + 1);
  if (rl.rpad != rpad_expected) return asmb_refuse(PGPFA_ASMB_BAD_ARG, "the output was sized for rpad = %d, the rank tables give %d", rpad_expected, rl.rpad);
  if ((int)rl.blk_lat.size() > tab_cap || (int)rl.cmap.size() > tab_cap) return asmb_refuse(PGPFA_ASMB_BAD_ARG, "tables exceed tab_cap = %d", tab_cap);
  const int rpad = rl.rpad, nact = round_up(rl.rtot, 64);        // (nact: lowrank_view)
  // (the tiles walked must lie inside the tables and the output)
  const int n64 = rl.rank_compact ? round_up(rl.rtot16, 64) / 64 : rpad / 64;
  if (4 * n64 > (int)rl.blk_lat.size() || (rl.rank_compact && 64 * n64 > (int)rl.cmap.size()) || (!rl.rank_compact && 64 * n64 > rpad))
    return fail("internal: the rank tables are shorter than the tiles the assembly walks");

  HIPC(hipSetDevice(c->device));
  HIPC(hipStreamSynchronize(c->st));
  HookBuffers hb;
  constexpr size_t SLACK = 128;
  auto input = [&](double** dev, const double* host, size_t count) -> int {
    CHK(hb.get(dev, count + SLACK, 0));
    const std::vector<double> h(SLACK, fill);
    HIPC(hipMemcpy(*dev, host, count * sizeof(double), hipMemcpyHostToDevice));
    HIPC(hipMemcpy(*dev + count, h.data(), SLACK * sizeof(double), hipMemcpyHostToDevice));
    return 0;
  };
  auto ints = [&](int** dev, const std::vector<int>& v) -> int {
    CHK(hb.get(dev, std::max<size_t>(v.size(), 1), 0));
    if (!v.empty()) HIPC(hipMemcpy(*dev, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice));
    return 0;
  };
  double *dF = nullptr, *dWt = nullptr;
  float* dF32 = nullptr;
  int *d_lat = nullptr, *d_col = nullptr, *d_cmap = nullptr, *d_roff = nullptr, *d_nrtab = nullptr, *d_list = nullptr;
  const size_t nf = (size_t)p * Tf * Tf;
  CHK(input(&dF, F, nf));
  CHK(input(&dWt, Wt, sW == 0 ? (size_t)wbin : (size_t)nslots * sW));
  CHK(ints(&d_lat, rl.blk_lat));
  CHK(ints(&d_col, rl.blk_col));
  CHK(ints(&d_roff, rl.rank_compact ? rl.roff16 : rl.roff));
  if (rl.rank_compact) { CHK(ints(&d_cmap, rl.cmap)); CHK(ints(&d_nrtab, rl.nrtab)); }
  CHK(ints(&d_list, std::vector<int>(list, list + nlist)));
  if (f32) {
    // the single-precision copy of the slabs, as ensure_f32_factors makes it (the slack too)
    CHK(hb.get(&dF32, nf + SLACK, 0));
    HIPC(hipDeviceSynchronize());
    hipLaunchKernelGGL(cvt_f32_kernel, dim3((unsigned)((nf + SLACK + 255) / 256)), dim3(256), 0, c->st, dF, dF32, nf + SLACK);
    HIPC(hipGetLastError());
  }
  void* dB = nullptr;
  const size_t bbytes = (size_t)nslots * rpad * rpad * (f32 ? sizeof(float) : sizeof(double));
  CHK(hook_output_bytes(hb, &dB, B, bbytes));
  HIPC(hipDeviceSynchronize());
  const BLayout L = b_layout_of(rl.rank_compact, rl.rtot16, rpad, d_cmap, d_roff, d_nrtab);
  const long long sB = (long long)rpad * rpad;
  if (f32) assemble_rxr_launch<float>(static_cast<float*>(dB), sB, rpad, rl.rtot, nact, L, dF32, Tf, T, p, d_lat, d_col, dWt, sW, d_list, nlist, c->st);
  else assemble_rxr_launch<double>(static_cast<double*>(dB), sB, rpad, rl.rtot, nact, L, dF, Tf, T, p, d_lat, d_col, dWt, sW, d_list, nlist, c->st);
  HIPC(hipGetLastError());
  HIPC(hipStreamSynchronize(c->st));
  for (int k = 0; k < p; ++k) { geom[k] = rl.rr[k]; geom[p + k] = rl.rk[k]; }
  for (int k = 0; k <= p; ++k) { geom[2 * p + k] = rl.roff[k]; geom[3 * p + 1 + k] = rl.roff16[k]; }
  int32_t* g = geom + 4 * p + 2;
  g[0] = rl.rtot; g[1] = rl.rtot16; g[2] = rpad; g[3] = rl.rank_compact ? 1 : 0; g[4] = L.nblk64; g[5] = L.npairs; g[6] = nact;
  std::copy(rl.blk_lat.begin(), rl.blk_lat.end(), blk_lat);
  std::copy(rl.blk_col.begin(), rl.blk_col.end(), blk_col);
  std::copy(rl.cmap.begin(), rl.cmap.end(), cmap);
  ntab[0] = (int)rl.blk_lat.size(); ntab[1] = (int)rl.cmap.size();
  return hook_collect_bytes("pgpfa_test_assemble_b", dB, B, bbytes);
}
