/*
 * pgpfa.h - C-ABI of libpgpfa_hip.so: the MI355X (gfx950) implementation of the
 * Poisson-GPFA EM hot path.
 *
 * The reference (mackelab/poisson-gpfa) is pure Python and has no FFI; the boundary it
 * exposes is the call surface of funs/inference.py, funs/learning.py and funs/engine.py.
 * Every entry point below names the reference function (file:line under the reference
 * tree) whose arithmetic it replaces.  The host mirror of that call surface lives in
 * poisson-gpfa_amd/funs/ and binds these symbols with ctypes.
 *
 * Conventions
 *   - plain pointers and sizes only; all host arrays are caller-owned, C-contiguous.
 *   - every function returns 0 on success, non-zero on failure; pgpfa_last_error()
 *     returns the message of the last failure on the calling thread.
 *   - doubles everywhere (the reference computes in float64); spike counts are packed
 *     to uint8 on upload (counts above 255 are rejected).
 *   - one context = one GPU = one host thread at a time; no callbacks into the caller.
 *   - trial index lists are int32, relative to the count tensor uploaded into the
 *     context; a NULL list means "all trials".
 *   - sizes: q neurons (ydim), p latents (xdim), T bins, R trials, n = p*T.
 *   - vector layouts are the reference's: xbar[k*T+t] = X[k][t] (inference.py:129),
 *     vecCd = [C[:,0],...,C[:,p-1], d] (util.py:560-574).
 */
#ifndef PGPFA_H
#define PGPFA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pgpfa_ctx pgpfa_ctx;

/* ---- library ------------------------------------------------------------------ */
const char* pgpfa_last_error(void);
int pgpfa_version(void);
int pgpfa_device_count(int* count);

/* ---- context ------------------------------------------------------------------ */
/* One fit = one context: sizes of experiment.data (engine.py:131-135), binSize in ms. */
int pgpfa_create(pgpfa_ctx** out, int device, int q, int p, int T, int R, double bin_ms);
int pgpfa_destroy(pgpfa_ctx* ctx);
/* Options: "newton_xtol" (1e-5), "newton_max_iter" (50), "use_mfma" (1),
 * "chunk_trials" (0 = auto), "eps_noise" (1e-3, util.py:599), "chord" (1: reuse the first factor for
 * chord steps), "chord_xtol" (1e-9), "chord_rho" (0.6), "chord_max_step" (1.0), "profile" (0; 1 = HIP events around
 * every tagged launch, 2 = around GEMM launches and the one mixing (tag "mix") launch of an E-step only; sums are read with pgpfa_get_info "prof_<family>_ms|_flops|_launches", the longest
 * single launch with "_max_ms|_max_flops"), "profile_pause" (1: stop recording without touching the sums, 0: go on - an event pair costs
 * ~10 us of device time per launch, so a caller that wants rates over a long region samples it),
 * "shared_pcg" (1: phase-1 Newton with the shared preconditioner), "shared_min" (16), "pcg_inner" (16: cap on
 * the inner PCG iterations of one outer Newton iteration), "pcg_eta0" (1e-2: relative residual of the first inner solve;
 * later ones adapt to the predicted error), "splitk_target" (1280: thin GEMMs are cut along k until about this many
 * workgroups are in flight),
 * "pcg_outer_max" (12), "cov_mode" (0 auto, 1 dense, 2 low-rank covariance engine), "lowrank_tol" (1e-10: stopping residual of the pivoted Cholesky behind the low-rank form K = eps I + F F^T; the covariance blocks
 * come out accurate to ~2x this value - measured against the reference at config 3 - the modes and the objective do not depend on it;
 * 1e-13 makes the form exact to rounding at ~10 % more rank),
 * "keep_trial_vsmgp" (0: the low-rank engine accumulates sum_r post_vsmGP_r for the tau M-step and rebuilds
 * per-trial T x T blocks only when pgpfa_get_post_vsmgp asks for them; 1: store them in every E-step),
 * "dual_lowrank" (1: the dual-variational entry points use the low-rank engine when it pays - log det through the r x r system; the
 * reference's 1e-6 diagonal jitter, inference.py:190, is carried by the per-bin blocks, so both engines evaluate the reference's
 * function; 0: always the dense engine),
 * "dual_f32" (0; 1: with dual_lowrank, the r x r system B = I + F^T Wt F, its factorisation, its inverse and the Yt product run in single
 * precision on the FP32 matrix cores, log det / covariance blocks / gradient accumulated in FP64: the mixed-precision form BASELINE
 * config 5 asks for; 2: the same with B assembled in FP64 and rounded once),
 * "laplace_f32" (0 - the default: the FP64 engine, the same instructions and bits as without the option; 1: in the passes of the low-rank engine that
 * produce post_vsmGP or its sum - the covariance phase of pgpfa_estep_laplace, sum-only or with "keep_trial_vsmgp", and the per-trial blocks
 * rebuilt on demand - B = I + F^T Wt F is assembled from single-precision factors, factorised and inverted on the FP32 matrix cores (the 128-wide
 * diagonal blocks of the factorisation in FP64 registers over the single-precision slab, rounded once); L^-T is
 * then widened to FP64 and everything behind it - the Yt product or the fused pass, the mixing, the split sums, post_vsm, post_vsmGP, PautoSum -
 * is the FP64 path, unchanged; 2: the same with B assembled in FP64 and rounded once; any other value fails.  The mode search and the objective
 * do not depend on it (bit-identical); the split verdict, the fused / unfused choice and the workspace plan come out the same.  A chunk whose
 * single-precision factorisation meets a non-positive pivot is redone in FP64 as a whole - info "last_cov_f32_fallbacks" - never an error.  The
 * dense engine ignores the option and "dual_f32" keeps its meaning for the dual's evaluations.  Measured error of the covariance outputs
 * against a dense FP64 inverse: docs/history/laplace_f32.md),
 * "laplace_evidence" (0 - the default: nothing is launched or allocated for it, every output keeps its bits; 1: pgpfa_estep_laplace also produces the
 * Laplace approximation of every processed trial's log evidence, see pgpfa_get_log_evidence - one reduction kernel per chunk behind the covariance
 * phase's factorisation, read back with the pivots, no further host wait; any other value fails.  With "laplace_f32" != 0 pgpfa_estep_laplace fails:
 * the log-determinant is taken from the FP64 factor only),
 * "dual_masked" (0 - the default: every pgpfa_dual_* entry point refuses while per-trial bin counts or an observation table are set, and launches,
 * allocations and bits are those of a library without the option; 1: pgpfa_dual_fixed_point, pgpfa_dual_lbfgs, pgpfa_dual_costgrad_batch,
 * pgpfa_dual_costgrad, pgpfa_dual_finalize, pgpfa_get_dual_lambda, post_cov of a variational trial and the blocks rebuilt on demand for rates and
 * samples accept both tables; with no table set the code path is the default one, bit for bit; any other value fails.  An entry (n, t) of trial r is
 * live when t < T_r and the neuron is observed on the trial.  Dual variables keep their padded [q*T] layout: lambda is exactly 0, rho = log lambda
 * comes back as 0 and gradients are exactly 0 at entries that are not live, and whatever the caller passes there is ignored.  Every result is that
 * of the reference's functions (inference.py:188-256) on the trial's reduced problem - rows of unobserved neurons deleted, bins cut to T_r - including
 * the 1e-6 jitter, which for a trial of T_r < T bins is taken from the T_r-bin Gram inverse and put on the bins t < T_r only, and the log-determinant
 * of the dual cost, corrected by sum_k (log det K_{k,T} - log det K_{k,T_r}); the tables behind both come from one kernel per
 * set of timescales, launched on the first such call while a length table is set.  pgpfa_dual_post_mean, pgpfa_dual_post_cov, pgpfa_loo_predict and
 * pgpfa_generate keep refusing),
 * "pcg_fused" (1: inner PCG iterations without host round trips, pcg.h), "pcg_w32" (1: packed FP32 curvature blocks in the PCG
 * Hessian-vector product), "cd_mfma" (1: (C,d) sweep on the matrix cores, mstep.h), "cd_hess_mfma" (1: the Newton pass
 * of the (C,d) M-step - cost, gradient, per-neuron Hessians - on the matrix cores up to 10 latents; 0: the vector kernel), "vsm_mfma" (1: beyond 10 latents the per-bin
 * covariance blocks are Gram products on the matrix cores - post_vsm_mfma_kernel, model.h; 0: vector kernel),
 * "extrapolate_start" (1: a warm-started E-step begins at m + beta (m - m_prev) for trials whose two previous
 * E-steps are resident), "extrapolate_beta" (1.0), "extrapolate_guard" (3.0, round 6: that extrapolation is only used while the parameter step
 * between the last two Laplace E-steps - info "last_param_step_prev" - was at most this many times the step being taken - "last_param_step";
 * behind a JUMP of the parameters the difference of the two previous modes is the jump's effect, not a trend; 0: no test),
 * "start_guard" (1, round 6: a warm start whose objective is above that of x = 0 - the resident mode belongs to other loadings - restarts at
 * zero; info "last_cold_restarts"),
 * "pcg_form" (2, round 5: as 1 with the solve's private vectors on line-aligned latent rows (T rounded up to 16 doubles), one start kernel for gradient / residual /
 * first per-bin application, the closing of a step inside kernel A of the next one and one upload per solve - needs "thin_products";
 * 1: a step of the host-free inner iteration is two tile-parallel kernels - the one-reduction (Chronopoulos-Gear) form of
 * PCG - plus the three preconditioner products, the prior mat-vec gone from the loop through Kt^-1 z = r - Wb z, pcg.h; up to 10 latents, needs "pcg_w32" and
 * "pcg_retire"; 0: the split kernels of round 3 with K^-1 p as a product),
 * "pcg_vec32" (1, with "pcg_form" 2: the vectors of an inner solve that carry no accumulated state - z, s, p, q and the preconditioner's t / y -
 * are stored in single precision, x, r, every product and dot stay FP64: a slot-step moves 13.8 n-vector equivalents instead of 19.8; 0: all FP64),
 * "pcg_rx32" (1, round 6, with "pcg_vec32", up to 10 latents: the residual r and the step x of an inner solve are stored in single precision as
 * well - every product, dot and update still in FP64 from the widened values; the step is widened into the caller's FP64 vector once per solve),
 * "pcg_adapt" (1: the launches of a step of that iteration are sized by the live count the device last mirrored to the host - it only falls during a
 * solve - and the per-bin kernels take 16 / 8 / 4 slots per workgroup above 640 / 320 / below; 0: sized by the solve's first count, 16 slots),
 * "pcg_xcd" (1: the two per-bin kernels of that step map workgroup ids so that the bin tiles of a slot group run on one XCD - they share the
 * boundary lines of rows that are not line-aligned and the slot's scalars in one L2; 0: bin tile = fast grid index),
 * "pcg_retire" (1: every slot of the inner PCG has its own forcing term and leaves the iteration when it reaches it - device-side
 * live list, pcg.h; 0: one common forcing term), "pcg_trace" (0; 1: one stderr line per inner solve),
 * "time_newton" (0; 1: HIP events around the inner solves -> info "last_newton_solve_ms" / "last_newton_solve_bytes"),
 * "small_tile_below" (2^30: products with fewer 128 x 128 tiles than this run on 64 x 64 workgroup tiles - i.e. all; 0: never),
 * "f32_tile64" (1: the single-precision products of the mixed-precision dual evaluation run on 64 x 64 workgroup tiles like the FP64 ones; 0: 128 x 128 only),
 * "splitk_below64" (400: products on 64 x 64 tiles are cut along k only below this many tiles),
 * "copy_kernels" (1: read-backs and uploads up to 256 KB move through host-mapped staging memory as one-workgroup kernels, and a flush is a
 * kernel that raises a sequence number the host spins on - no hipMemcpyAsync / hipStreamSynchronize on those paths; 0: the runtime's copies),
 * "poisson_tiles" (2, round 5: 16-bin tiles per wave of the matrix-core Poisson pass up to 10 latents - the table fragments of a neuron tile, read from
 * L2, serve that many tiles; 1: one tile per wave),
 * "vsm_b4" (2, round 5; 1: the same with 32 bins per workgroup and scalar loads: the per-bin covariance blocks post_vsm for 11..20 latents on the 4 x 4 x 4 block shape of the FP64 matrix cores - four bins per
 * instruction, instructions over the lower pairs of four-latent blocks: 15 x 19 cycles per four bins and four columns at 20 latents against 12 x 68 on
 * the 16 x 16 x 4 shape padded to 32 rows; 0: that form),
 * "pivchol_pairs" (1, round 5: beyond 256 bins the pivoted Cholesky of the Gram matrices runs with two bins per row thread and four column groups -
 * half the dependent memory round trips per step, the pivot search on the diagonal while it is in registers; same pivots; 0: rbf_pivchol_kernel),
 * "yt_mix" (1, round 5: under the split covariance form and up to 10 latents the product Yt = F L^-T and the mixing pass run as ONE kernel - tiles of all
 * latents on the FP64 matrix cores, mixed in registers, only the correction D and post_vsm leave the chip; Yt is never written; 0: product, then mixing pass),
 * "yt_mix_dbg" (0; bit mask for timing experiments on that kernel - 1 no loads of F, 2 no products, 4 no mixing, 8 no stores of D, 16 no panel staging, 32 no
 * barriers, 64 no panel loads: the results are WRONG when it is set; tools/ab_opts.sh only),
 * "yt_mix_dma" (1: that kernel stages the panels of L^-T by LDS-DMA, global_load_lds_dwordx4, one chunk ahead of the products that read them - no
 * staging registers, no LDS writes, same bits; 0: through registers behind the products.  A row map too long for LDS runs the register form),
 * "syrk_tile" (256, round 5: 256 x 256 workgroup tiles in the FP16 term of the split covariance sum where there are more than 256 bins and the strides
 * allow 16-byte loads - every output then costs half the reads of the correction D; 128: the 128 x 128 kernel),
 * "syrk_dbg" (0; bit mask for timing experiments on syrk_f16x2_kernel - 1 no conversions, 2 no products, 8 no barriers: the results are WRONG when it is
 * set; tools/ab_opts.sh only),
 * "mix_slot" (3, round 5: as 2 with a workgroup of 128 bins x 2 column halves - both halves read one G_t image of 56 KB, two workgroups = two waves per SIMD on a CU -
 * the halves' pair sums meet through LDS at the end; 2: as 1 with the next pair of columns requested before this pair's arithmetic - two register sets, no branch in the loop - where
 * p is a template width and the rank a multiple of 4, else 1; 1: the mixing pass of that split form with a thread per bin and a workgroup per (slot, 256 bins) that walks whole columns of
 * the slab - contiguous 2-KB runs instead of 512-byte pieces, no LDS; up to 10 latents; 0: mix_vsm_split_kernel, 64 bins x 4 columns),
 * "thin_products" (2: the three products of the low-rank preconditioner application - the block-diagonal F^T t and F v, and Sb u - as kernels of
 * their own that feed the matrix cores straight from global memory, csrc/thin.h; 1: the two block-diagonal ones only; 0: products of the general
 * GEMM kernel, block-sparse and with split-K),
 * "overlap_factors" (1: in pgpfa_set_params the pivoted Cholesky of the Gram matrices runs on a side stream next to the Gram inverses; 0: one stream),
 * "mt_fill" (1: before a slot's L^-T is formed in the low-rank covariance engine only the entries its consumers read below the diagonal are cleared -
 * the strictly lower part of p rectangles of r_k rows - where every consumer starts at the latent's own columns; 0: the whole rpad x rpad slab),
 * "mix_wide" (1: the in-place mixing pass y <- G_t y of the full-width covariance product at 17..20 latents with the lanes along the bins - 64 bins x 4 waves
 * per workgroup, G_t's rows in registers, y and G_t y exchanged through LDS, csrc/model.h mix_vsm_wide2_kernel; 0: mix_vsm_wide_kernel, lanes along the latents),
 * "cross_kernel" (1: the cross term of that split form in a kernel with all rows of a latent in one workgroup, 128 rows per
 * launch; 0: through the general GEMM kernel),
 * "split_cov" (1: the sum over trials of the T x T covariance blocks by the exact split form of csrc/split.h (up to 20 latents; 17..20 need "mix_wide") - FP64 cross term, FP16
 * two-half product for the second-order term - while the root mean square of eps ||Wt_t|| stays below "split_max_norm" (0.07);
 * 0: always the full-width FP64 product), "measure_mix" (0; 1: measure eps ||Wt_t|| in every covariance pass, also where the split form is not a candidate -> info
 * "last_eps_wt_norm" / "last_eps_wt_rms": the maximum over the chunks of the LAST pgpfa_estep_laplace / pgpfa_dual_finalize call of the
 * largest and of the root-mean-square value over (trial, bin); reset at the start of those calls),
 * "workspace_headroom" (2.0: a low-rank workspace plan leaves room for the ranks to grow by this factor before it is re-made),
 * "workspace_grow_budget_ms" (200, round 6: a RE-plan stops mapping memory into the arena after this long once the chunk has what
 * "workspace_grow_floor_slots" (128) slots need, and runs the E-step in balanced chunks of the slots that fit - mapping pages another process has
 * just released costs up to 40 ms per GB on this stack; the first plan of a context is not bounded; 0: no limit),
 * "rank_gran" (4 - the default -, 8 or 16, round 6; also the environment variable PGPFA_RANK_GRAN at pgpfa_create: the ranks of the latents' low-rank factors are
 * rounded up to this many columns in the r x r system of the low-rank engine, in L^-T and in the columns of Yt / D - 4 and 8: COMPACT offsets, the
 * products with F_k still take the rank rounded up to 16 rows and meet zero columns of F_k; needs "thin_products" 2, falls back to 16 otherwise),
 * "workspace_pool" (1: a new context attaches the arena - address range and mapped memory - a closed context of the process left behind; 0: it
 * reserves and maps its own; before the first E-step),
 * "workspace_vmm" (1: the chunk workspace is a reserved address range that grows by mapping memory; 0: plain allocations; before
 * the first E-step), "workspace_granule_mb" (1024: size of the mapped chunks),
 * "chord_max" (most chord steps of the per-trial fallback Newton on one factor), "slab_row_align" (1: rows of latent k of the low-rank
 * slab start on 128-byte lines), "dual_gemm" (1: the neuron contractions of the dual evaluation as GEMMs against a pair / loading table),
 * "cd_debug" (0; measurement only: bit switches that drop the exp / the products / the staging of the (C,d) kernels, tools/cd_probe.py),
 * "rates_chunk_trials" (0 - the default: pgpfa_posterior_rates walks its trial list in chunks sized so that the device staging of the per-trial planes
 * it was asked for stays within 256 MiB; > 0: that many trials per chunk.  No output depends on it, bit for bit - the group sums are carried from
 * chunk to chunk in list order; it exists for the tests of exactly that),
 * "sample_chunk_trials" (0 - the default: pgpfa_posterior_sample walks its list in chunks whose device staging stays within 256 MiB; > 0: that many
 * trials per chunk.  No output depends on it, bit for bit; it exists for the test of exactly that),
 * "interp_chunk_trials" (0 - the default: pgpfa_posterior_at walks its list in chunks whose device staging stays within 256 MiB; > 0: that many
 * trials per chunk.  No output depends on it, bit for bit; it exists for the test of exactly that),
 * "velat_chunk_trials" (0 - the default; the same for pgpfa_posterior_velocity_at),
 * "covat_chunk_trials" (0 - the default; the same for pgpfa_posterior_cov_at), "covat_block_times" (0 - the default: pgpfa_posterior_cov_at walks
 * its query times in blocks sized so that the right-hand sides of a block stay within that bound; > 0: that many times per block, rounded up to 16.
 * No output depends on it, bit for bit),
 * "func_chunk_trials" (0 - the default; the same for pgpfa_posterior_functionals), "func_block_cols" (0 - the default: pgpfa_posterior_functionals
 * pushes its functionals through the square root in blocks sized so that the staging of a block stays within that bound; > 0: that many functionals
 * per block, a multiple of 16.  No output depends on it, bit for bit),
 * "counts_chunk_trials" (0 - the default; the same for pgpfa_posterior_counts), "counts_nodes" (32: nodes of the Gauss-Hermite rule of
 * pgpfa_count_probabilities / pgpfa_posterior_counts, 8 .. 64; the rule's error falls with it and the cost grows in proportion). */
int pgpfa_set_option(pgpfa_ctx* ctx, const char* key, double value);
/* Options that pgpfa_set_params builds from - "eps_noise" (Gram matrices, their inverses, the low-rank factors), "lowrank_tol" (the low-rank
 * factors), "rank_gran", "thin_products" and "use_mfma" (the rank tables: compact offsets need both) - re-run it with the stored parameters
 * when they change after it, so an option set before or after pgpfa_set_params gives the same numbers. */
/* Info: "sample_noise_dim" (normals per draw of the next pgpfa_posterior_sample), "chunk_trials", "plan_lowrank", "n_pad", "lowrank_rtot" (total rank of the r x r system), "lowrank_rtot16" (the same with every
 * latent's rank rounded up to 16: roff16[p], the rows the products with F take), "lowrank_compact" (1: compact rank offsets are live,
 * "rank_gran" 4 or 8 - lowrank_rtot < lowrank_rtot16 when they save rows), "last_estep_ms", "last_newton_factorizations",
 * "last_newton_solves", "last_pcg_iterations", "last_shared_factorizations", "last_cov_lowrank",
 * "last_dense_retries", "hbm_bytes_allocated", "hbm_bytes_free" / "hbm_bytes_total" (hipMemGetInfo of the context's device, now), "n_trials_global", "prof_<tag>_{ms,flops,launches}" (tags gemm, potrf, solve, poisson, assemble, vsm, cd, mix; "prof_mix_flops" counts BYTES for the stand-alone mixing
 * passes and FLOPs - products + mixing - when "last_yt_mix_fused" is 1), "counts_two_bytes",
 * "arena_bytes", "last_split_cov"; the path the split form of the last covariance pass took (set by every pass of the low-rank engine, as "last_split_cov";
 * all 0 when the split form did not run): "last_syrk_tile" (128 or 256: the kernel of the FP16 term), "last_split_sps" (slots per group of its partial
 * sums), "last_cross_kernel" (1: cross_term_kernel, 0: the segmented-K GEMM), "last_mix_form" (the mixing pass: 0 mix_vsm_split_kernel, 1 / 2 / 3
 * mix_slot_kernel / mix_slot2_kernel / mix_slot3_kernel, 4 the fused yt_mix_kernel, 5 mix_vsm_wide2_kernel); "last_yt_mix_fused" (1 when the last covariance pass ran product and mixing as one kernel), "last_cov_f32" (1 when the last covariance pass ran the
 * single-precision r x r phase of "laplace_f32", else 0: set by every pass, as "last_split_cov"), "last_cov_f32_fallbacks" (chunks of the last
 * pgpfa_estep_laplace call redone in FP64 after a non-positive pivot of the single-precision factorisation; reset at the start of that call),
 * "last_log_evidence_sum" (sum of the Laplace log evidence, pgpfa_get_log_evidence, over the trials of the last pgpfa_estep_laplace call; 0 when
 * "laplace_evidence" was off),
 * "last_eps_wt_norm", "last_eps_wt_rms", "last_newton_solve_ms", "last_newton_solve_bytes",
 * "last_newton_solve_bytes_moved" (what the step's kernels really move: with "pcg_vec32" five of its vectors are single precision),
 * "last_newton_solve_bytes_survey" (the same slot-iterations priced at q T + 8 (2 p T + T p^2) bytes each: SURVEY 8(d)'s B_E per pass per trial),
 * "arena_vmm_failed" (1 once the virtual-memory arena fell back to plain allocations), "last_newton_max_iter", "last_dual_evaluations",
 * "last_loo_unconverged"; round 6, diagnostics of the last pgpfa_estep_laplace call: "last_param_step" / "last_param_step_prev" (relative
 * displacement of the parameters between consecutive Laplace E-steps: the largest of |dC| / |C|, |dd| / |d|, |d log tau|; -1: unknown),
 * "last_cold_restarts", "last_retry_ms" (time of the dense retry pass), "last_fallback_no_descent" / "last_fallback_line_search" /
 * "last_fallback_outer_cap" (slots the shared-preconditioner Newton phase gave up on, by reason); of the context: "plans" and "plan_ms_total"
 * (workspace plans made and their time), "arena_grow_ms_total" (of it: mapping memory), "set_params_calls"; "trial_lengths_set" (1 while
 * pgpfa_set_trial_lengths has given the trials bin counts of their own, 0 when every trial has T bins); "observed_set" (1 while pgpfa_set_observed has marked (trial, neuron) pairs as not recorded, else 0);
 * "observed_bins_set" (1 while pgpfa_set_observed_bins has given the context a per-bin table, else 0);
 * "last_cd_unobserved_neurons" (neurons without an observed trial in the list of the last (C,d) M-step pass). */
int pgpfa_get_info(pgpfa_ctx* ctx, const char* key, double* value);

/* ---- data ---------------------------------------------------------------------- */
/* experiment.data[r]['Y'] for all r, as one [R][q][T] tensor (inference.py:96-97).  The reference keeps counts as float64 / int64 of
 * any size (util.py:741,750); here any non-negative integer up to 65535 is accepted (one byte per entry resident, a second plane of
 * high bytes only while some count exceeds 255 - info key "counts_two_bytes"). */
int pgpfa_upload_counts_f64(pgpfa_ctx* ctx, const double* Y);
int pgpfa_upload_counts_u8(pgpfa_ctx* ctx, const uint8_t* Y);
int pgpfa_upload_counts_u16(pgpfa_ctx* ctx, const uint16_t* Y);
/* Trials of unequal length: len[R], the number of bins T_r (1 <= T_r <= T) of every trial; NULL: every trial has T bins again.  Called after
 * the counts are uploaded, which stay one zero-padded [R][q][T] tensor: the call fails, naming the trial, on a length outside 1..T or on a
 * non-zero count at a padded bin t >= T_r.  Uploading counts again drops the table.  Padded bins carry no likelihood term: no rate, no count, no
 * contribution to the Laplace objective, its gradient and curvature blocks, or to any sum of the (C,d) M-step; the GP prior still spans all T
 * bins of every trial, so the posterior over the first T_r bins is that of the T_r-bin problem (a GP is consistent under marginalisation), the
 * padded bins hold the prior conditional and the objective at the mode is the same number.  Posterior getters and pgpfa_set_posterior keep
 * their padded [T] layouts; PautoSum and the timescale cost are those of the padded problem; pgpfa_count_moments counts sum_r T_r samples.  The
 * dual-variational entry points, pgpfa_loo_predict and pgpfa_generate do not know the lengths and fail while a table is set (info key
 * "trial_lengths_set"). */
int pgpfa_set_trial_lengths(pgpfa_ctx* ctx, const int32_t* len /* [R], NULL: all T */);
/* Neurons unobserved on some trials (sessions that share only part of their population): obs[R][q], non-zero = neuron n was recorded on trial r;
 * NULL: every neuron is observed on every trial again (drops the table).  Called after the counts are uploaded.  The call fails, naming the first
 * offender, when a trial has no observed neuron, a neuron is observed on no trial, or a count at an unobserved (trial, neuron) row is non-zero; counts
 * uploaded while a table is set are checked again.  An unobserved pair carries no likelihood term: the Laplace posterior, objective and evidence of
 * trial r are those of the model with only the observed rows of C, d and Y; the (C,d) M-step sums run over observed pairs (and keep the 1/numTrials
 * of the reference); the timescale M-step is untouched.  A neuron without an observed trial in the list of an M-step pass has zero gradient, Hessian and
 * step (only a prior moves it).  With no table every kernel takes the branch it took before.  The dual-variational entry points, pgpfa_loo_predict and
 * pgpfa_generate do not know the table and fail while it is set (info key "observed_set"). */
int pgpfa_set_observed(pgpfa_ctx* ctx, const uint8_t* obs /* [R][q], non-zero = observed; NULL: all observed, drops the table */);
/* Single entries not recorded (a channel that drops out for part of a trial, a blanked artifact, speckled hold-out): live[R][q][T], non-zero = entry
 * (r, n, t) was recorded; NULL drops the table.  Called after the counts are uploaded.  The table composes with pgpfa_set_trial_lengths and
 * pgpfa_set_observed by AND, in any order of the three calls: an entry is live when t < T_r, obs[r][n] is set and live[r][n][t] is.  Trial r's
 * likelihood is the sum over its live entries of exp(h_nt) - y_nt h_nt; the prior is unchanged, so posterior, objective and evidence are those of the
 * model marginalised over the dead entries, and the (C,d) M-step sums run over live entries.  The call (and a later call of the other two setters
 * while a table is set) fails, naming the first offender, when a trial is left without a live entry, a neuron has no live entry on any trial, or a
 * count at a dead entry is non-zero; counts uploaded while a table is set are checked again.  Setting or dropping the table supersedes resident
 * posteriors.  A table that marks every entry live computes what no table computes, through other kernel instantiations.  The dual-variational
 * entry points (also under the option dual_masked), pgpfa_loo_predict and pgpfa_generate do not know the table and fail while it is set (info key
 * "observed_bins_set"). */
int pgpfa_set_observed_bins(pgpfa_ctx* ctx, const uint8_t* live /* [R][q][T], non-zero = recorded; NULL drops the table */);
/* resident counts of the listed trials (idx NULL: all) as uint16 [n][q][T] */
int pgpfa_get_counts_u16(pgpfa_ctx* ctx, int n, const int32_t* idx, uint16_t* out);
/* params = {'C': [q][p], 'd': [q], 'tau': [p] seconds} (engine.py:40-44).  Builds the p Gram
 * matrices (util.makeK_big, util.py:599-619) and their inverses (inference.py:82) on device. */
int pgpfa_set_params(pgpfa_ctx* ctx, const double* C, const double* d, const double* tau_s);
int pgpfa_get_gram(pgpfa_ctx* ctx, double* K /* [p][T][T] */);
int pgpfa_get_gram_inverse(pgpfa_ctx* ctx, double* Kinv /* [p][T][T] */);

/* ---- Laplace callbacks (inference.py:12-65) -------------------------------------- */
/* negLogPosteriorUnNorm and _grad at caller-supplied points X[n][p][T] for trials idx[n]. */
int pgpfa_laplace_eval(pgpfa_ctx* ctx, int n, const int32_t* idx, const double* X,
                       double* f /* [n] */, double* grad /* [n][p][T] or NULL */);
/* negLogPosteriorUnNorm_hess for one trial, dense [pT][pT] latent-major. */
int pgpfa_laplace_hessian(pgpfa_ctx* ctx, int trial, const double* X, double* H);

/* ---- Laplace E-step (inference.laplace, inference.py:67-185) ---------------------- */
/* Mode finding + posterior covariance blocks for the listed trials.  warm_start = 1
 * starts from the modes resident in the context (prevOptimRes, inference.py:99-102), 0 from
 * zeros, 2 per trial from its resident mode if an earlier E-step produced one and from zeros
 * otherwise (minibatches that revisit trials).  obj_sum = sum over the listed trials of the objective at the
 * mode (the reference returns -obj_sum/numTrials, inference.py:175,183).
 * iters/status (may be NULL): Cholesky factorizations per trial (Newton + the final one at the
 * mode), status 0 = converged. */
int pgpfa_estep_laplace(pgpfa_ctx* ctx, int n, const int32_t* idx, int warm_start,
                        double* obj_sum, int32_t* iters, int32_t* status);
int pgpfa_set_modes(pgpfa_ctx* ctx, int n, const int32_t* idx, const double* X /* [n][p][T] */);
int pgpfa_get_post_mean(pgpfa_ctx* ctx, int n, const int32_t* idx, double* out /* [n][p][T] */);
int pgpfa_get_post_vsm(pgpfa_ctx* ctx, int n, const int32_t* idx, double* out /* [n][T][p][p] */);
/* post_vsmGP in the reference's (T,T,p) layout (inference.py:164-167). */
int pgpfa_get_post_vsmgp(pgpfa_ctx* ctx, int n, const int32_t* idx, double* out /* [n][T][T][p] */);
/* post_cov of one trial, recomputed on demand (inference.py:130-131,161-162). */
int pgpfa_get_post_cov(pgpfa_ctx* ctx, int trial, double* out /* [pT][pT] */);
/* Laplace approximation of the log evidence of the listed trials (idx NULL: all), one double each:
 *   log Z_r = -f_r(x*_r) - 1/2 (log det H_r(x*_r) + sum_k log det K_k)
 * with f_r = negLogPosteriorUnNorm (inference.py:12-32), H_r its Hessian (inference.py:50-65) and x*_r the mode the E-step returned
 * (post_cov = H_r^-1, inference.py:130-131).  Normalisation: the reference's - f_r drops sum log y!, so log Z_r does too; the 2 pi factors of the
 * prior and of the Laplace integral cancel.  Padded bins of a trial shorter than T (pgpfa_set_trial_lengths) change nothing: the value is that of
 * the trial's own T_r-bin model.  Produced by pgpfa_estep_laplace while option "laplace_evidence" is 1, under both covariance engines; a
 * trial's value stays valid as long as the posterior it belongs to is the resident one - a later E-step over the trial with the option off,
 * pgpfa_dual_finalize, pgpfa_set_posterior, pgpfa_set_modes or new counts supersede it.  Fails, naming the first such trial, when a listed trial has no valid value. */
int pgpfa_get_log_evidence(pgpfa_ctx* ctx, int n, const int32_t* idx, double* out /* [n] */);
/* Upload E-step results produced elsewhere (e.g. a reference infRes dict) for the M-step. */
int pgpfa_set_posterior(pgpfa_ctx* ctx, int n, const int32_t* idx, const double* post_mean,
                        const double* post_vsm, const double* post_vsmgp /* [n][T][T][p] */);

/* ---- posterior firing rates --------------------------------------------------------------- */
/* What the resident posterior of the listed trials (idx NULL: all; a trial may be listed more than once) says about the firing rates
 *   lambda_n(t) = exp(d_n + c_n . x_t)
 * under the parameters of the last pgpfa_set_params - the posterior being whatever is resident for the trial: the Laplace one, the variational
 * one after pgpfa_dual_finalize, or one uploaded with pgpfa_set_posterior.  With m_t = post_mean[:, t] and Sigma_t = post_vsm[t]:
 *   eta[i][n][t] = d_n + sum_k C_nk m_kt                  posterior mean of the log rate (the argument of exp(C x + d), util.py:289-334, which the
 *                                                         reference only ever evaluates at a mode and without a variance)
 *   var[i][n][t] = sum_ab C_na Sigma_t[a][b] C_nb         its posterior variance, stored as max(., 0) (twice the v = 1/2 diag(C Sigma C^T) of
 *                                                         inference.py:215-219, which the variational fixed point computes and never hands out)
 *   rate         = exp(eta + var / 2)                     posterior mean of the rate, spikes per bin; the central credible band of the rate at
 *                                                         level L is exp(eta -+ z_L sqrt(var)) - the caller forms both from eta and var
 *   ell[i][n]    = sum_{t < T_r} (y_nt eta - rate)        expected Poisson log likelihood per trial and neuron without sum log y!, as the reference
 *                                                         drops it (inference.py:12-32); reads the resident counts, both byte planes
 *   group_sum[g][n][t] = sum_{i: group[i] = g, t < T_r} rate[i][n][t],   group_count[g][t] = #{i: group[i] = g, t < T_r}
 * for a trial -> group table group[n] with ids 0..n_groups-1 (experimental conditions: the mean rate of a condition is group_sum / group_count; a
 * group without trials gives zeros and a count of 0, a trial listed twice counts twice).  Every output may be NULL; with only group outputs asked for
 * no per-trial [q][T] plane is written to memory at all.  No floating-point atomics: a workgroup owns a (group, neuron tile, bin tile), walks the
 * group's trials in list order and carries its sums in registers, so group_sum is reproducible from run to run and does not depend on how the list
 * is cut into chunks (option "rates_chunk_trials").  Trials of unequal length (pgpfa_set_trial_lengths): ell, group_sum and group_count stop at
 * T_r; eta and var are written for all T bins - the padded bins hold the prior conditional, so there they are the forecast of the log rate.
 * Fails, naming the trial, when a listed trial has no posterior - no E-step, pgpfa_dual_finalize or pgpfa_set_posterior has written one since its
 * counts were uploaded -; when a group id is outside 0..n_groups-1; when a group output is asked for without the table.  Touches no E-step or M-step
 * state: the workspace plan, the arena, the per-trial serials and snapshots and every sum an M-step reads are what they were. */
int pgpfa_posterior_rates(pgpfa_ctx* ctx, int n, const int32_t* idx /* NULL: all */,
                          const int32_t* group /* [n], 0..n_groups-1, or NULL */, int n_groups,
                          double* eta /* [n][q][T] */, double* var /* [n][q][T] */, double* ell /* [n][q] */,
                          double* group_sum /* [n_groups][q][T] */, int32_t* group_count /* [n_groups][T] */);

/* Joint posterior samples of the latents and posterior-predictive spike counts.  X[i][s] is draw s from the Gaussian posterior N(m_r, Sigma_r) resident
 * for trial r = idx[i], under the parameters of the E-step that produced it (restored around the call when the context has moved on): the covariance is
 * the one pgpfa_get_post_cov returns for that trial - for a Laplace trial the inverse Hessian at the resident mode, for a trial whose posterior came from
 * pgpfa_dual_finalize the VIPostCov of the kept lambda with the reference's jitter.  The pT x pT matrix is never formed: the draw is a square root of
 * Sigma applied to standard normals,
 *   low-rank engine   x = m + G F L^-T z2 + sqrt(eps) chol(G) z1     (G = (I + eps W)^-1 per bin, B = I + F^T Wt F = L L^T)
 *   dense engine      x = m + L^-T z                                  (H = L L^T)
 * with nz normals per draw: nz = p T + lowrank_rtot under the low-rank engine - z1 latent-major [p][T], then z2 in the compact rank order - and p T
 * under the dense one (info key "sample_noise_dim": the nz of the next call; the engine follows the plan as for every covariance pass, option
 * "cov_mode", and "dual_lowrank" for variational trials).  noise_in given: X - m is a deterministic linear function of it.  noise_in NULL: the normals
 * are drawn on the device, each a pure function of (seed, trial id, sample index, element, stream) - Philox4x32-10 with streams 4 (z1) and 5 (z2), apart
 * from the 1..3 of pgpfa_generate - so sample s is the same whether 8 or 4096 are asked for, wherever the trial stands in the list and however the list
 * is chunked; a trial listed twice gets the same draws twice.  noise_out receives exactly the normals that were used.
 *   Y[i][s][n][t] ~ Poisson(exp(d_n + c_n . x_t)) for t < T_r, 0 at padded bins, keyed by (seed, trial, sample, neuron, bin);
 *   count_sum[i][s][n] = sum_{t < T_r} Y (integers; with only count_sum asked for no [q][T] plane is written to memory).
 * Trials of unequal length: X covers all T bins, the padded ones are draws of the forecast (W is zero there).  The pass is FP64 whatever
 * "laplace_f32" says.  noise_in / noise_out are sized by the current parameters: when a trial's posterior was computed under timescales whose
 * low-rank system has fewer rows the last entries of z2 are not used (noise_out reports zeros there); when it has more a call with noise arrays
 * fails (set those parameters first) - without noise arrays every trial simply uses its own system.
 * Fails, naming what is wrong: n_samples < 1; every output NULL; set_params not called; Y or count_sum without a counts table (the trial lengths are
 * unknown); a trial without such a posterior - no E-step since its counts were uploaded, or one given by pgpfa_set_posterior, of which only blocks are
 * known -, naming the trial; a draw above 65535, naming the trial; an asynchronous timescale pass in flight.
 * Leaves untouched: post_mean, post_vsm, post_vsmGP and their resident marks, the sums pgpfa_mstep_precomp reads, mode serials, snapshots, log
 * evidence and the resident counts.  Uses the chunk workspace as pgpfa_get_post_cov does. */
int pgpfa_posterior_sample(pgpfa_ctx* ctx, int n, const int32_t* idx /* NULL: all; repeats allowed */,
                           int n_samples, unsigned long long seed,
                           const double* noise_in  /* [n][S][nz] or NULL: drawn on the device */,
                           double*       noise_out /* [n][S][nz] or NULL: the normals that were used */,
                           double*   X         /* [n][S][p][T] or NULL */,
                           uint16_t* Y         /* [n][S][q][T] or NULL */,
                           int32_t*  count_sum /* [n][S][q]    or NULL */);

/* Importance weights of the Laplace posterior's own draws: how far the Gaussian at the mode is from the true posterior of a trial, and the correction
 * of its log evidence.  With f = negLogPosteriorUnNorm (inference.py:12-32), x* the resident mode of trial r = idx[i], H the Hessian there and
 * x_s = x* + delta_s draw s of pgpfa_posterior_sample under `seed` - bit for bit the X[i][s] that call returns for the same (seed, trial, s) -,
 *   log p(y, x_s) - log N(x_s; x*, H^-1) = log Z_Laplace + log w_s,        log w_s = - [ f(x_s) - f(x*) - 1/2 delta_s^T H delta_s ].
 * The prior is quadratic and cancels; at a stationary mode what is left of it cancels the first-order likelihood term, counts included, so that
 *   log_w[i][s]  = - sum_{(n,t) live} lambda*_nt phi(c_n . delta_st),   lambda*_nt = exp(d_n + c_n . x*_t),   phi(a) = e^a - 1 - a - a^2 / 2
 *   log_ratio[i] = log (1/S) sum_s w_s        log Z_Laplace + log_ratio estimates the trial's true log evidence: (1/S) sum_s w_s is unbiased for
 *                                              Z / Z_Laplace (log Z_Laplace: pgpfa_get_log_evidence, same normalisation)
 *   ess[i]       = (sum_s w_s)^2 / sum_s w_s^2 effective sample size, 1 .. S: near S where the Laplace posterior can be trusted
 * and the w_s, self-normalised, turn the draws of pgpfa_posterior_sample with the same seed into an importance sampler of the true posterior.  The
 * only approximation is that the gradient g at x* is zero: a residual one adds - g . delta_s to log w_s, which is ignored (the E-step's stopping
 * rule bounds it).  The sum runs over the entries that carry a likelihood term under the three missing-data tables; every other entry adds exactly
 * 0, whatever C and d hold there.  K is the prior the covariance engine in use is exact for - the sum needs no K^-1, no counts and no pT x pT
 * object: one pass over the draws on the FP64 matrix cores (csrc/impw.h) behind the sampler, whose engine follows the plan as there; the list is
 * walked in chunks (option "sample_chunk_trials") and no X plane goes to the host.  No floating-point atomics: the tiles of a draw and the draws of
 * a trial are added in index order (log_ratio max-shifted), so log_w[i][s] is a function of the draw and the trial alone - the trial's position in the
 * list, the chunks and n_samples enter no sum -, and log_ratio and ess depend on n_samples besides; a trial listed twice gets the same numbers twice.  An overflowing e^a gives
 * log_w = -inf (weight 0).
 * Fails, naming what is wrong: n_samples < 1; every output NULL; set_params not called; no counts table; an asynchronous timescale pass in flight;
 * a trial without a posterior that can be sampled (as pgpfa_posterior_sample), naming the trial; a trial whose posterior is variational
 * (pgpfa_dual_finalize), naming the trial - the identity is the Laplace approximation's -; a log weight that is NaN, naming the trial.
 * Leaves untouched what pgpfa_posterior_sample leaves untouched. */
int pgpfa_importance_weights(pgpfa_ctx* ctx, int n, const int32_t* idx /* NULL: all; repeats allowed */,
                             int n_samples, unsigned long long seed,
                             double* log_ratio /* [n]    log mean_s w_s, or NULL */,
                             double* ess       /* [n]    or NULL */,
                             double* log_w     /* [n][S] or NULL */);

/* The latent posterior at arbitrary time points.  The Gaussian posterior N(m, Sigma) over the T grid times t_j = j bin_ms resident for trial
 * r = idx[i] - the posterior being whatever is resident for the trial, as pgpfa_posterior_rates defines it - extends to any time s (ms from the
 * trial's first bin) by the prior conditional of the GP.  Per latent k, with K_k the Gram matrix of pgpfa_get_gram and V_k = post_vsmGP[:, :, k]:
 *   kx_k(s)[j]    = (1 - eps) exp(-1/2 (s - j bin)^2 / (1000 tau_k)^2) + eps [s == j bin]      (the white-noise term only AT a grid time)
 *   a_k(s)        = K_k^-1 kx_k(s)
 *   mean[i][k][s] = a_k(s) . m_k
 *   var[i][k][s]  = 1 - a_k(s) . kx_k(s) + a_k(s)^T V_k a_k(s),  stored as max(., 0)
 * At a grid time this is post_mean[k][j] and post_vsmGP[j][j][k]; off the grid it is the marginal of the model extended by s as a bin without a
 * likelihood term; far from the trial mean -> 0 and var -> 1, the prior.  times_ms: any finite doubles - negative or beyond the last bin
 * (extrapolation), unsorted, repeated -, one grid [S] for all listed trials or, with per_trial != 0, one grid [n][S] per list entry (event
 * alignment: event_ms[r] + lags).  Trials of unequal length: the padded bins hold the prior conditional, so interpolating from all T bins equals
 * interpolating the trial's own T_r-bin posterior from its own grid.  Only the marginals per latent are given: the cross-latent covariance at s
 * needs the off-diagonal T x T blocks of Sigma, which are not resident.
 * The posterior of an E-step is evaluated under the timescales of that E-step (restored around the call when the context has moved on, per
 * (snapshot, kind of posterior) group as pgpfa_posterior_sample does); one uploaded with pgpfa_set_posterior under the current parameters.  Under
 * the sum-only plan ("keep_trial_vsmgp" 0) the blocks of the listed trials are rebuilt on demand, as pgpfa_get_post_vsmgp does.
 * A trial's result does not depend on its position in the list, on which other trials are listed or on how the list is cut into chunks (option
 * "interp_chunk_trials"), bit for bit; a trial listed twice gives the same numbers twice.  No floating-point atomics.
 * Fails, naming what is wrong: S < 1; both outputs NULL; a time that is not finite, naming its position; set_params not called; a trial without a
 * posterior - no E-step, pgpfa_dual_finalize or pgpfa_set_posterior has written one since its counts were uploaded -, naming the trial; a
 * variational posterior of a trial shorter than T (its jitter comes from the trial's own T_r-bin Gram inverse, for which the padded-grid identity
 * is not established: refused rather than approximated); an asynchronous timescale pass in flight.
 * Leaves untouched: post_mean, post_vsm, post_vsmGP and their resident marks, the sums pgpfa_mstep_precomp reads, mode serials, snapshots, log
 * evidence, the resident counts and the three missing-data tables.  Uses the chunk workspace as pgpfa_get_post_vsmgp does when blocks are rebuilt. */
int pgpfa_posterior_at(pgpfa_ctx* ctx, int n, const int32_t* idx /* NULL: all; repeats allowed */,
                       int S, const double* times_ms /* [S], or [n][S] when per_trial != 0 */, int per_trial,
                       double* mean /* [n][p][S] or NULL */, double* var /* [n][p][S] or NULL */);

/* Cross-latent posterior covariance and log-rate moments at arbitrary time points: what pgpfa_posterior_at leaves out.  With a_k(s) = K_k^-1 kx_k(s)
 * as there and Sigma the trial's p T x p T posterior covariance (the layout of pgpfa_get_post_cov),
 *   cov(s)[k][l] = a_k(s)^T Sigma_kl a_l(s) + delta_kl (1 - a_k(s) . kx_k(s))
 * - at a grid time post_vsm of that bin, on the diagonal the var of pgpfa_posterior_at - and per neuron n the Gaussian log rate at s:
 *   eta[n][s] = d_n + c_n . mean(s),   var[n][s] = c_n^T cov(s) c_n                (rate, bands: as for pgpfa_posterior_rates)
 * Sigma is never formed: the call builds the square root pgpfa_posterior_sample draws from (dense engine: L^-T of the Hessian; low-rank engine:
 * eps G + (G F L^-T)(G F L^-T)^T), pushes the p weight vectors of every time through it with the library's GEMM and takes their p x p Gram on the
 * FP64 matrix cores (csrc/covat.h).  times_ms and per_trial mean what they mean for pgpfa_posterior_at; so do the parameter snapshots, trials of
 * unequal length (times behind T_r: the forecast) and the missing-data tables.
 * A trial's result does not depend on its position in the list, on which other trials are listed, on how the list is cut into chunks or the query
 * times into blocks (options "covat_chunk_trials", "covat_block_times"), or on which other outputs are asked for, bit for bit; cov is symmetric to
 * the bit, its diagonal and var are clamped at 0.  No floating-point atomics.
 * Fails, naming what is wrong: S < 1; all four outputs NULL; times_ms NULL; a time that is not finite, naming its position (before any device
 * call); set_params not called; an asynchronous timescale pass in flight; a trial without a posterior, naming the trial; a posterior uploaded with
 * pgpfa_set_posterior (only its blocks are known: it has no square root); a variational posterior of a trial shorter than T.
 * Leaves untouched what pgpfa_posterior_sample leaves untouched: post_mean, post_vsm, post_vsmGP and their resident marks, the sums
 * pgpfa_mstep_precomp reads, mode serials, snapshots, log evidence, the resident counts and the three missing-data tables.  Uses the chunk workspace. */
int pgpfa_posterior_cov_at(pgpfa_ctx* ctx, int n, const int32_t* idx /* NULL: all; repeats allowed */,
                           int S, const double* times_ms /* [S], or [n][S] when per_trial != 0 */, int per_trial,
                           double* mean /* [n][p][S] or NULL */, double* cov /* [n][S][p][p] or NULL */,
                           double* eta /* [n][q][S] or NULL */, double* var /* [n][q][S] or NULL */);

/* Joint posterior of linear functionals of a trial's latents: epoch means, contrasts between epochs, projections of a whole trajectory onto a
 * decoding axis or a temporal template, window-averaged log rates - the questions that span time, which need the covariance BETWEEN bins.  With m
 * the resident posterior mean of trial r = idx[i] laid out [p][T], Sigma its p T x p T covariance (the layout of pgpfa_get_post_cov) and J weight
 * vectors u_j laid out [p][T],
 *   mean[i][j]   = u_j . m
 *   cov[i][j][l] = u_j^T Sigma u_l,      var[i][j] = cov[i][j][j]
 * Sigma is never formed: the call builds the square root M (Sigma = M M^T) that pgpfa_posterior_sample draws from and pgpfa_posterior_cov_at uses -
 * G, F and L as in the comments above those two -, pushes the weights through it and takes the Gram of the results on the FP64 matrix cores
 * (csrc/pfunc.h):
 *   dense engine      Sigma = L^-T L^-1                               Q = L^-1 U                cov = Q^T Q
 *   low-rank engine   Sigma = eps G + (G F L^-T)(G F L^-T)^T          V = G U,  Q = L^-1 F^T V  cov = Q^T Q + eps U^T V
 * in FP64 whatever "laplace_f32" says.  The engine follows the plan, the parameter snapshots and the three missing-data tables as those two calls do.
 * A trial shorter than T needs nothing special: its padded bins hold the GP forecast under the square root, so weights there give the forecast's
 * contribution.  weights: one set [J][p][T] for all listed trials or, with per_trial != 0, one set [n][J][p][T] per list entry (windows aligned
 * to an event that falls at another bin in every trial).  With cov asked for J <= 1024; without it any J, walked in blocks, and no J x J plane
 * is formed.
 * A trial's result does not depend on its position in the list, on which other trials are listed, on how the list is cut into chunks or the
 * functionals into blocks (options "func_chunk_trials", "func_block_cols"), on shared against per-trial weights, or on which other outputs are asked
 * for, bit for bit; a trial listed twice gives the same numbers twice; cov is symmetric to the bit, var has the bits of its diagonal, both clamped
 * at 0.  No floating-point atomics.
 * Fails, naming what is wrong: J < 1; all three outputs NULL; weights NULL; a weight that is not finite, naming functional, latent and bin (and the
 * list entry when per_trial; before any device call); cov with J > 1024; set_params not called; an asynchronous timescale pass in flight; a trial
 * without a posterior, naming the trial; a posterior uploaded with pgpfa_set_posterior (only its blocks are known: it has no square root); a
 * variational posterior of a trial shorter than T.
 * Leaves untouched what pgpfa_posterior_sample leaves untouched.  Uses the chunk workspace when var or cov is asked for. */
int pgpfa_posterior_functionals(pgpfa_ctx* ctx, int n, const int32_t* idx /* NULL: all; repeats allowed */,
                                int J, const double* weights /* [J][p][T], or [n][J][p][T] when per_trial != 0 */, int per_trial,
                                double* mean /* [n][J] or NULL */, double* var /* [n][J] or NULL */, double* cov /* [n][J][J] or NULL */);

/* Value and velocity of every latent at arbitrary time points, with their joint 2 x 2 posterior per latent.  Under the prior the time derivative
 * xdot_k(s) is jointly Gaussian with the grid values, so its posterior follows by the prior conditional of pgpfa_posterior_at with the cross Gram
 * differentiated.  With kx_k(s), a_k(s), m_k, V_k as there, l_k = 1000 tau_k ms:
 *   kd_k(s)[j]       = -1000 (s - j bin) / l_k^2 (1 - eps) exp(-1/2 (s - j bin)^2 / l_k^2)      (Cov(xdot_k(s), x_k(j bin)), per SECOND)
 *   b_k(s)           = K_k^-1 kd_k(s),   kappa_k = (1 - eps) / tau_k^2                            (the prior variance of the velocity, 1/s^2)
 *   mean[i][k][s]    = a . m_k                          vel[i][k][s]     = b . m_k
 *   var[i][k][s]     = 1 - a . kx + a^T V_k a           vel_var[i][k][s] = kappa_k - b . kd + b^T V_k b         (both stored as max(., 0))
 *   cross[i][k][s]   =   - a . kd + a^T V_k b           (the posterior Cov(x_k(s), xdot_k(s)); 0 under the prior)
 * The velocity is that of the smooth component of the latent - the white eps part has no derivative, so kd has no nugget term even at a grid time -
 * in latent units per second.  mean has the bits of pgpfa_posterior_at.  var, vel_var and cross come from ONE pass over the T x T blocks, on the FP64
 * matrix cores (csrc/velat.h).  Far from the trial vel -> 0, cross -> 0, var -> 1, vel_var -> kappa_k.  times_ms, per_trial, parameter snapshots,
 * uploaded posteriors, trials of unequal length and the sum-only plan: as for pgpfa_posterior_at.
 * A plane's bits do not depend on which other planes are asked for, on the trial's position in the list, on which other trials are listed, on how
 * the list is cut into chunks (option "velat_chunk_trials") or on shared against per-trial grids, given the same blocks: under the sum-only plan
 * every call rebuilds the blocks of its list, and the last bits of a rebuilt block follow the number of trials rebuilt together, as for
 * pgpfa_posterior_at (var, vel_var and cross then move in the last digits with the SET of listed trials; mean and vel never).  No floating-point atomics.
 * Not given: the cross-latent covariance of the velocities (hence velocities in orthonormalised coordinates and the variance of the speed),
 * derivatives of firing rates, sharded sessions.
 * Fails and leaves untouched what pgpfa_posterior_at does, in the same words under this entry point's name; all five outputs NULL is refused. */
int pgpfa_posterior_velocity_at(pgpfa_ctx* ctx, int n, const int32_t* idx /* NULL: all; repeats allowed */,
                                int S, const double* times_ms /* [S], or [n][S] when per_trial != 0 */, int per_trial,
                                double* mean /* [n][p][S] or NULL */, double* var /* [n][p][S] or NULL */, double* vel /* [n][p][S] or NULL */,
                                double* vel_var /* [n][p][S] or NULL */, double* cross /* [n][p][S] or NULL */);

/* Posterior-predictive spike counts from the two moments of the log rate.  The reference has no counterpart: it stops at the latent posterior, and
 * its only count-like outputs are exp(C x + d) at a held-out mode (util.py:289-334).  With eta ~ N(m, v) the count of an entry is the
 * Poisson-lognormal mixture
 *   P(y = k) = int Poisson(k; e^eta) N(eta; m, v) d eta          (no closed form; mean mu = exp(m + v / 2), variance mu + mu^2 (e^v - 1))
 * evaluated in FP64 by a Gauss-Hermite rule of "counts_nodes" nodes (option; 32, allowed 8 .. 64; nodes and weights are computed on the host and
 * uploaded once per context and node count) centred on the mode of the integrand and scaled by its curvature there - found by Newton from m, at
 * most 40 steps, warm-started from the mode of k - 1 when k is walked - and written in (eta - m) / v throughout, so that v = 0 is an ordinary input
 * (the Poisson pmf at e^m) and v -> 0 approaches it smoothly (csrc/counts.h).  Per entry i, every output optional:
 *   logp[i]     = log P(y = counts[i]), counts in 0 .. 65535
 *   pmf[i][k]   = P(y = k), k = 0 .. K - 1 (k fastest), 1 <= K <= 1024
 *   lower[i], upper[i] = the smallest k with CDF(k) >= (1 - level) / 2 and with CDF(k) >= (1 + level) / 2, 0 < level < 1; the walk over k stops at
 *                 k_cap (0 .. 65535): an entry whose upper quantile lies beyond gets k_cap (lower too if it lies beyond), and the number of such
 *                 entries of the LAST call is info "counts_saturated"
 *   pmean[i], pvar[i]  = mu and mu + mu^2 expm1(v), counts per bin
 * An entry whose moments are not finite or whose v is negative gets NaN (lower, upper: -1).  An entry's outputs are functions of its own inputs and
 * of K, level, k_cap and the node count alone, bit for bit: not of its position, of the other entries, of how the entries are cut into chunks, or
 * of which other outputs are asked for.  No atomics.  Needs a context for its device and stream only: no counts, parameters or posterior.
 * Fails, naming what is wrong: every output NULL; K, level or k_cap outside their ranges (each checked only when an output reads it); logp
 * without counts; a count outside 0 .. 65535. */
int pgpfa_count_probabilities(pgpfa_ctx* ctx, long long n_entries, const double* m /* [n_entries] */, const double* v /* [n_entries] */,
                              const int32_t* counts /* [n_entries], or NULL without logp */, int K, double level, int k_cap,
                              double* logp /* [n_entries] */, double* pmf /* [n_entries][K] */, int32_t* lower, int32_t* upper /* [n_entries] */,
                              double* pmean, double* pvar /* [n_entries] */);
/* The same per (trial, neuron, bin) of the listed trials under their resident posterior (the reference has no counterpart): m = eta and v = var of
 * pgpfa_posterior_rates, staged on the device per chunk of the list by that entry point's kernel and never copied to the host, then the kernel of
 * pgpfa_count_probabilities on the staged planes.  Every output is [n][q][T] (pmf [n][q][T][K]).  counts: a host array [n][q][T] (0 .. 65535), or
 * NULL for the resident counts, both byte planes.  Entries behind a trial's T_r (pgpfa_set_trial_lengths) are written as NaN (lower, upper: -1) and
 * are not counted in "counts_saturated"; an unobserved neuron (pgpfa_set_observed) or entry (pgpfa_set_observed_bins) has a posterior of its log
 * rate like any other and gets the model's prediction.  A trial's result does not depend on its position in the list, on the other trials, on the
 * chunking (option "counts_chunk_trials", as "rates_chunk_trials") or on the outputs asked for, bit for bit; a trial listed twice gives the same
 * numbers twice.  Fails as pgpfa_posterior_rates does and in its order - set_params not called, the trial list, a trial without a posterior -, and
 * before those: logp with counts NULL while no counts are uploaded, or while a per-bin table is set (the resident counts at entries that were not
 * recorded are placeholders: pass the counts).  Touches no E-step or M-step state, as pgpfa_posterior_rates. */
int pgpfa_posterior_counts(pgpfa_ctx* ctx, int n, const int32_t* idx /* NULL: all; repeats allowed */,
                           const int32_t* counts /* [n][q][T] or NULL: the resident counts */, int K, double level, int k_cap,
                           double* logp, double* pmf, int32_t* lower, int32_t* upper, double* pmean, double* pvar);

/* ---- M-step ----------------------------------------------------------------------- */
/* MStepObservationCost(_grad) (learning.py:20-91) over the trials of the last E-step /
 * pgpfa_set_posterior call; with prior_center != NULL adds |v-center|^2 * inv_s2 / 2 and its
 * gradient ('useDiag' prior of learning.py:445-534).  Multi-GPU: all-reduced over ranks. */
int pgpfa_mstep_cd_costgrad(pgpfa_ctx* ctx, const double* vecCd, const double* prior_center,
                            double inv_s2, double* cost, double* grad /* [q*(p+1)] */);
/* Device Newton solver for the same cost (separable over neurons: q convex problems of dimension p+1):
 * one pass returns the per-neuron costs at vecCd, the Newton steps delta[(p+1)*q] (vecCd layout) and the
 * Newton decrements dec[q]; pgpfa_mstep_cd_cost_per_neuron evaluates trial points for the line search. */
int pgpfa_mstep_cd_newton_pass(pgpfa_ctx* ctx, const double* vecCd, const double* prior_center, double inv_s2,
                               double* cost_n /* [q] */, double* delta /* [q*(p+1)] */, double* dec /* [q] */);
/* Chord pass: cost and gradient at vecCd (one cheap sweep), step from the per-neuron Hessians of the last
 * pgpfa_mstep_cd_newton_pass (also across EM iterations: they stay SPD, the step stays a descent direction).
 * The trial lists of the two passes need not have the same length: the gradient is the mean over the trials of THIS
 * pass, the Hessians the mean over the trials of that Newton pass (its all-reduced count is kept with its sums), so
 * delta = -(H_A / n_A)^-1 (g_B / n_B) and dec = -g . delta. */
int pgpfa_mstep_cd_chord_pass(pgpfa_ctx* ctx, const double* vecCd, const double* prior_center, double inv_s2,
                              double* cost_n /* [q] */, double* delta /* [q*(p+1)] */, double* dec /* [q] */);
int pgpfa_mstep_cd_cost_per_neuron(pgpfa_ctx* ctx, const double* vecCd, const double* prior_center, double inv_s2,
                                   double* cost_n /* [q] */);
/* makePrecomp (learning.py:145-173): PautoSum[p][T][T] over the same trials (all-reduced). */
int pgpfa_mstep_precomp(pgpfa_ctx* ctx, double* num_trials);
int pgpfa_get_pautosum(pgpfa_ctx* ctx, double* out /* [p][T][T] */);
/* MStepGPtimescaleCost(_grad) (learning.py:175-255) for latent k at log-gamma = logp. */
int pgpfa_mstep_tau_costgrad(pgpfa_ctx* ctx, int k, double logp, double* cost, double* grad);
/* The same for all p latents at once (one batched factorisation): logp[p] -> cost[p], grad[p]. */
int pgpfa_mstep_tau_costgrad_batch(pgpfa_ctx* ctx, const double* logp, double* cost, double* grad);
/* m (1..4) candidate points per latent in one batched pass, candidate-major: logp[m][p] -> cost[m][p], grad[m][p].
 * The pass is a latency-bound chain of small launches, so 4 candidates cost about as much as 1; the host-side
 * root finder of learnGPparams brackets and interpolates with them instead of stepping serially. */
int pgpfa_mstep_tau_costgrad_multi(pgpfa_ctx* ctx, int m, const double* logp, double* cost, double* grad);
/* The same pass in two halves (round 6): _begin enqueues it on the context's side stream and returns at once, _end waits for it and returns
 * cost[m][p], grad[m][p] - the same bits as the call above.  Between the two the caller may run the (C,d) passes of the same M-step (learning.py:
 * 93-141 and 257-293 are independent problems; the reference solves them one after the other); one pass in flight per context, every other
 * timescale / precomp / E-step entry point - pgpfa_mstep_tau_costgrad for a single latent among them, it shares the pass's scratch -
 * fails while one is, and leaves the pass intact. */
int pgpfa_mstep_tau_costgrad_multi_begin(pgpfa_ctx* ctx, int m, const double* logp);
int pgpfa_mstep_tau_costgrad_multi_end(pgpfa_ctx* ctx, double* cost, double* grad);

/* ---- count moments (util.py:523-533 Poisson-PCA initialiser; engine.py:487-492 diagnostics) ---- */
/* Exact integer moments of the resident counts over all (trial, bin) samples of the listed trials:
 * sum[i] = sum y_i, cross[i][j] = sum y_i y_j, n_samples = trials * T - the sum of the listed trials' lengths under
 * pgpfa_set_trial_lengths - (np.mean / np.cov of the raster follow). */
int pgpfa_count_moments(pgpfa_ctx* ctx, int n, const int32_t* idx, int64_t* sum /* [q] */, int64_t* cross /* [q][q] */,
                        int64_t* n_samples);

/* ---- synthetic population (util.dataset, util.py:705-750) ------------------------------------------ */
/* Draws x_k ~ N(0, K(tau_k)) and y_nt ~ Poisson(exp(c_n . x_t + d_n)) for the listed trials (NULL: all) under the parameters of
 * pgpfa_set_params, from a counter-based generator keyed by `seed` (NOT NumPy's stream).  The counts replace those trials in
 * the resident tensor; X_out[n][p][T] / Y_out[n][q][T] (either may be NULL) receive copies. */
int pgpfa_generate(pgpfa_ctx* ctx, unsigned long long seed, int n, const int32_t* idx, double* X_out, uint8_t* Y_out);

/* ---- leave-one-neuron-out prediction (util.py:289-334, engine.py:599-644) ----------- */
/* For each listed trial (idx NULL: all R) and each neuron nn: the Laplace mode of the latents given the other
 * q-1 neurons (cold start), then y_pred[(trial, nn)][t] = exp(C[nn] . x_t + d[nn]); err_sum = sum of squared
 * differences to the held-out counts.  The R*q mode searches run batched on the E-step machinery. */
int pgpfa_loo_predict(pgpfa_ctx* ctx, int n, const int32_t* idx, double* y_pred /* [n][q][T] */, double* err_sum);

/* ---- dual variational E-step (inference.py:188-432) -------------------------------- */
/* dualProblem and dualProblem_grad for one trial at lambda[q*T] (structured: never forms
 * C_big or diag(lambda)).  pgpfa_dual_costgrad, pgpfa_dual_costgrad_batch, pgpfa_dual_post_mean and pgpfa_dual_post_cov
 * refuse a lambda that is not finite (the first two also one that is not positive) at a live entry on the host, before
 * anything is uploaded or launched, naming the trial and the entry.  The check runs right behind the argument and trial-list
 * checks and ahead of the state checks, so a call that is also made too early (no counts, no parameters) or lists a trial
 * twice reports its lambda first; it reads only the caller's array and the host copies of the live tables. */
int pgpfa_dual_costgrad(pgpfa_ctx* ctx, int trial, const double* lam, double* cost,
                        double* grad /* [q*T] or NULL */);
/* The same for a list of distinct trials at once, each at its own lambda: lam[n][q*T] -> cost[n], grad[n][q*T]
 * (or NULL).  The dense factorisations of a chunk of trials are batched; inference.dualVariational drives the
 * reference's per-trial L-BFGS-B runs concurrently so that one round of their requests is one call. */
int pgpfa_dual_costgrad_batch(pgpfa_ctx* ctx, int n, const int32_t* idx, const double* lam, double* cost, double* grad);
/* The whole dual optimisation of the listed distinct trials on the device: one L-BFGS run (10 correction pairs, Armijo
 * backtracking) per trial in rho = log(lambda) - the unconstrained form of the reference's optimizeLogLambda path
 * (inference.py:222-256, 391-396) - all runs of a chunk in lockstep, every iteration one batched dual evaluation.
 * Stops per trial on scipy's L-BFGS-B criteria (relative decrease <= factr * 2.2e-16, or max |gradient| <= pgtol).
 * rho[n][q*T]: start in, optimum out; fopt[n]: dual optimum (inference.py:325/397); iters[n] may be NULL. */
int pgpfa_dual_lbfgs(pgpfa_ctx* ctx, int n, const int32_t* idx, double* rho, int max_iter, double factr, double pgtol,
                     double* fopt, int32_t* iters);
/* The optimum of the same dual problem by a fixed point instead of a quasi-Newton run in lambda.  At the optimum of the reference's dual
 * (zero of dualProblem_grad, inference.py:215-219)  log lambda = d + C m + v  with  m = -K C_big (lambda - y)  (VIPostMean, :193) and
 * v = 1/2 diag(C Sigma C^T)  (VIPostCov with its 1e-6 jitter, :188-191).  Given v, m is the mode of the Laplace objective with the log
 * rates shifted by v (the batched Newton-PCG of pgpfa_estep_laplace, warm-started) and lambda = exp(C m + d + v); given lambda, v follows
 * from the per-bin covariance blocks.  The map v -> v contracts by about half the largest posterior variance of a log rate per pass
 * (a digit or more), so a trial needs ~5-10 covariance passes where L-BFGS in rho = log lambda needs thousands of evaluations.
 * Stops per trial when max |v_new - v| <= tol - exactly the max-norm of dualProblem_grad at the returned lambda.
 * rho[n][q*T] (may be NULL with start = 0 / 3: nothing read, nothing written): log lambda - read as the start (start = 1, 2), written with the
 * optimum; start: 0 cold, lambda = 0.5 everywhere (the reference's start, inference.py:302), 1 rho is the start and the mode search begins at
 * zero, 2 rho is a previous optimum and the mode search begins at its variational mean, 3 the same from the optimum resident on the device; fopt[n]: dual cost at the optimum (inference.py:196-213); outer[n] (may be NULL):
 * passes used; vstatus[n]: 0 converged, 1 pass cap reached, 2 not contracting (hand the trial to pgpfa_dual_lbfgs from the rho returned);
 * lam_out[n][q*T] (may be NULL): the optimal lambda itself (exp and log of the q T entries run on the device).  The optimum also stays on the
 * device: pgpfa_dual_finalize with lam = NULL takes it from there. */
int pgpfa_dual_fixed_point(pgpfa_ctx* ctx, int n, const int32_t* idx, double* rho, int start, int max_outer, double tol, double* fopt,
                           int32_t* outer, int32_t* vstatus, double* lam_out);
/* The dual variables resident for the listed trials (the optimum of the last pgpfa_dual_fixed_point, or what pgpfa_dual_finalize was given):
 * out[n][q*T]. */
int pgpfa_get_dual_lambda(pgpfa_ctx* ctx, int n, const int32_t* idx, double* out);
/* VIPostMean (inference.py:193-194): mean[p*T] = -K_big C_big (lambda - ybar) for one trial, latent-major. */
int pgpfa_dual_post_mean(pgpfa_ctx* ctx, int trial, const double* lam, double* mean);
/* VIPostCov (inference.py:188-191) for one trial, dense [pT][pT] latent-major: prec = K_big^-1 + C_big diag(lambda) C_big^T
 * (may be NULL) and cov = (prec + 1e-6 diag(diag(prec)))^-1. */
int pgpfa_dual_post_cov(pgpfa_ctx* ctx, int trial, const double* lam, double* cov, double* prec);
/* VIPostMean / VIPostCov blocks at lambda for the listed trials; fills the same posterior
 * slots as the Laplace E-step and returns sum of negLogPosteriorUnNorm at the VI mean. */
int pgpfa_dual_finalize(pgpfa_ctx* ctx, int n, const int32_t* idx, const double* lam /* [n][q*T]; NULL: the optimum pgpfa_dual_fixed_point left
                        on the device for these trials */, double* nlp_sum);

/* ---- multi-GPU (trial sharding; RCCL over xGMI) -------------------------------------- */
int pgpfa_comm_unique_id(char* id128 /* 128 bytes */);
int pgpfa_comm_init(pgpfa_ctx* ctx, const char* id128, int rank, int nranks);
int pgpfa_comm_allreduce_host(pgpfa_ctx* ctx, double* buf, int count);
/* One line about this rank's communicator for start-up logs: "rank r/n device d pci <bus id> comm_ranks m comm_device d" (comm_ranks = ncclCommCount:
 * the number of ranks RCCL itself saw); without a communicator "rank 0/1 device d pci <bus id> comm none".  buf is NUL-terminated. */
int pgpfa_comm_describe(pgpfa_ctx* ctx, char* buf, int len);

/* ---- test / bench hooks ---------------------------------------------------------------- */
/* Batched SPD factor (+ optional inverse) of caller matrices through the production kernels:
 * A[batch][n][n] symmetric in, Cholesky factor L (lower, row-major) out; inv (may be NULL)
 * receives A^-1.  Used by the parity tests and by bench.py's roofline leg. */
int pgpfa_test_potrf(pgpfa_ctx* ctx, int batch, int n, const double* A, double* L, double* inv);
/* C = alpha*A*B^T + beta*C, column-major, through the production MFMA GEMM (use_mfma=1) or
 * the scalar check kernel (use_mfma=0). */
int pgpfa_test_gemm_nt(pgpfa_ctx* ctx, int M, int N, int K, double alpha, const double* A,
                       const double* B, double beta, double* C);
/* The same with B given as K x N column-major (C = alpha*A*B + beta*C): the multi-RHS sweep form. */
int pgpfa_test_gemm_nn(pgpfa_ctx* ctx, int M, int N, int K, double alpha, const double* A,
                       const double* B, double beta, double* C);
/* The same two products through the single-precision instantiation of the MFMA kernel (v_mfma_f32_16x16x4_f32; operands are
 * rounded to float on the way in, C comes back widened): the GEMM of the mixed-precision dual evaluation ("dual_f32"). */
int pgpfa_test_gemm_nt_f32(pgpfa_ctx* ctx, int M, int N, int K, double alpha, const double* A,
                           const double* B, double beta, double* C);
int pgpfa_test_gemm_nn_f32(pgpfa_ctx* ctx, int M, int N, int K, double alpha, const double* A,
                           const double* B, double beta, double* C);
/* The two kernel stages of the split covariance sum (csrc/split.h) on caller data, through the launch code of the E-step; the hooks allocate device
 * buffers of their own.  Every output buffer is uploaded before the launch, so entries no kernel stores come back as the caller left them, and the hooks
 * fail when a kernel wrote behind an output.
 * pgpfa_test_split_syrk: the single-precision term on the FP16 matrix cores.  D is float [nslots][round_up(ract, 32) * ldd], laid out as the E-step lays it
 * out: D_k[t, b] of a slot at (k * ts + t) + b * ldd, ts >= T, ldd >= p * ts (neither has to be a multiple of 4: the kernel then takes its slow loads);
 * columns b >= ract, rows t in [T, ts) and the floats between p * ts and ldd must not reach the result.  sps = 0: groups of max(1, ceil(nslots / 64)) slots,
 * the E-step's rule; sps > 0: groups of sps slots.  tile is option "syrk_tile" (128 or 256); *tile_used is the kernel that ran (256 only where T > 256,
 * round_up(T, 256) <= ts and ts, ldd are multiples of 4).  part comes back as [p][*ngroups][T][T], column-major, of which the entries (i, j) with i >= j hold
 * sum over the group's slots and b < ract of D_k[i, b] D_k[j, b] (entries above the diagonal are written in whole 64 x 64 blocks that meet it, or not at all). */
int pgpfa_test_split_syrk(pgpfa_ctx* ctx, int nslots, int T, int p, int ract, int ldd, int ts, int sps, int tile, const float* D, double* part, int* tile_used,
                          int* ngroups);
/* pgpfa_test_split_latent_sums: one latent's S = sum_s A_s A_s^T (rk x rk, full after the mirror) and X = sum_s A_s D_s^T (rk x T), both column-major with
 * leading dimension rk.  A_s[i][b] = A[s * sM + row_off + i + b * lda] (FP64; rk, kw multiples of 16, lda >= row_off + rk, sM >= kw * lda),
 * D_s[b][t] = D[s * sD + b * ldd + t] (float; ldd >= T, sD >= kw * ldd).  cross_kernel 1: X through cross_term_kernel in launches of 128 rows, 0: through
 * the segmented-K GEMM (option "cross_kernel").  Groups as in the E-step: X in groups of sps slots (0: its rule, as above), S in at most 256 groups. */
int pgpfa_test_split_latent_sums(pgpfa_ctx* ctx, int nslots, int rk, int kw, int T, int lda, long long sM, int row_off, int ldd, long long sD, int sps,
                                 int cross_kernel, const double* A, const float* D, double* Ssum, double* Xsum);
/* pgpfa_test_thin: the three block-diagonal products of the low-rank preconditioner y = F Sb F^T t (csrc/thin.h) on caller data, through the table builder
 * of the rank tables (thin_tables) and the launch code of the inner solve (thin_launch_ft / _s / _f); device buffers of its own, the context only lends its
 * stream.  kind: PGPFA_THIN_FT u = F^T t, PGPFA_THIN_S v = Sb u, PGPFA_THIN_F y = F v, PGPFA_THIN_APPLY the three in that order through two intermediates.
 * Geometry by the rule of the rank tables: rr_l = round_up(ranks[l], gran) (gran 4, 8 or 16), rk_l = round_up(rr_l, 16), roff_l = sum of rr before l,
 * rtot = roff_p, rpad = round_up(max(rtot, max_l roff_l + rk_l), 128); they come back in geom = [rr (p), rk (p), roff (p + 1), rtot, rpad], the work tables in
 * tab_ft / tab_f / tab_s (four ints per entry, at most tab_cap ints each) and their entry counts in ntab[3].
 * F: slabs [p][Tf][Tf], element (t, j) of latent l at l Tf Tf + j Tf + t; columns [ranks[l], rk_l) must hold zeros, rows t >= T may hold anything.  The
 *   transposed copy FT (ld rpad) is built from F by build_fbig_kernel, as the rank tables' owner builds it, over a buffer that holds `fill` where production
 *   has zeros (outside every latent's own rr rows).  Sb: [rpad][rpad], element (m, k) at k rpad + m, read for m, k < rtot.
 * n-vectors (input of FT, output of F): one column per slot, latent l at rows l Tx + (0..T), Tx >= T; doubles, or floats with vec_f32 (FT, F, APPLY).
 * rank-space vectors (output of FT, both of S, input of F): doubles, rows [0, rtot) of a column that holds at least rpad.
 * X: input [nslots][ldx], Y: output [nslots][ldy] (elements of their storage type), uploaded before the launch - what no kernel stores comes back as it
 *   went in - with a band of 1024 doubles behind it, and behind the intermediates of APPLY (leading dimension max(ldx, ldy), prefilled with `fill`); the
 *   call fails if a band changed.  Every input has 128 elements of `fill` behind it.
 * cols (may be NULL: identity): ncols slot numbers; live: device-side count of the leading list entries in use (-1: none); stop: value of the device
 *   stop flag (-1: no flag).
 * Impossible geometry is refused before anything is allocated or launched, with a code of its own (the text is in pgpfa_last_error). */
enum {
  PGPFA_THIN_FT = 0, PGPFA_THIN_S = 1, PGPFA_THIN_F = 2, PGPFA_THIN_APPLY = 3
};
enum {
  PGPFA_THIN_BAD_ARG = 100,       /* null pointer, unknown kind or granularity, sizes below 1, Tf below T or no multiple of 4 */
  PGPFA_THIN_REFUSED_T = 101,     /* T < 4 */
  PGPFA_THIN_REFUSED_RANK = 102,  /* a rank or the rank total no multiple of 4, rk above Tf */
  PGPFA_THIN_REFUSED_TX = 103,    /* Tx < T, or Tx % 4 where T % 4 == 0 */
  PGPFA_THIN_REFUSED_LD = 104,    /* ldx / ldy below the rows read or written, or no multiple of 4 */
  PGPFA_THIN_REFUSED_RPAD = 105,  /* rpad above the leading dimension of a rank-space vector */
  PGPFA_THIN_REFUSED_COLS = 106,  /* list entry outside the slots, or a slot twice; without a list, more columns than slots */
  PGPFA_THIN_REFUSED_LIVE = 107   /* live count above ncols */
};
int pgpfa_test_thin(pgpfa_ctx* ctx, int kind, int p, int T, int Tf, const int32_t* ranks, int gran, long long ldx, long long ldy, int Tx, int vec_f32,
                    int nslots, int ncols, const int32_t* cols, int live, int stop, double fill, const double* F, const double* Sb, const void* X, void* Y,
                    int32_t* geom /* [3 p + 3] */, int tab_cap, int32_t* tab_ft, int32_t* tab_f, int32_t* tab_s, int32_t* ntab /* [3] */);
/* pgpfa_test_pivchol: the pivoted Cholesky of (1 - eps) RBF_k, k < p (rbf_pivchol_kernel<256,1>, <512,2>, rbf_pivchol2_kernel<256,4>) for caller
 * timescales tau[p] (seconds; bin in milliseconds), through the three-way choice of the engine (pivchol_launch): up to 256 bins the first form, beyond
 * them the third with `pairs` (and an even Tf), else the second.  Slabs of its own, prefilled with `fill`, the band of 1024 doubles behind them and behind
 * the ranks; the context only lends its stream.  F: [p][Tf][Tf] out, element (t, j) of latent k at k Tf Tf + j Tf + t; rank[p] out; *form out: 0, 1, 2 in
 * the order above.  Impossible geometry is refused before anything is allocated or launched, with a code of its own. */
enum {
  PGPFA_PIVCHOL_BAD_ARG = 120,      /* null pointer, p outside 1..32, Tf above 4096, bin or a timescale not positive */
  PGPFA_PIVCHOL_REFUSED_T = 121,    /* T < 1 */
  PGPFA_PIVCHOL_REFUSED_TF = 122,   /* Tf < T */
  PGPFA_PIVCHOL_REFUSED_ODD = 123,  /* pairs with an odd Tf */
  PGPFA_PIVCHOL_REFUSED_LDS = 124   /* dynamic LDS above 64 KiB, what a launch may ask for without opting in */
};
int pgpfa_test_pivchol(pgpfa_ctx* ctx, int p, int T, int Tf, const double* tau, double bin, double eps, double tol, int pairs, double fill, double* F,
                       int32_t* rank, int32_t* form);
/* pgpfa_test_bin_blocks: G_t = (I + eps W_t)^-1, Wt_t = W_t G_t and log det(I + eps W_t) of the listed slots (bin_blocks_reg_kernel up to 10 latents,
 * bin_blocks_coop_kernel up to 32) on caller data, through the launch code of the engine (bin_blocks_launch); device buffers of its own, the context only
 * lends its stream.  W: [nslots][sW], bin t of slot s at s sW + t p p, row-major p x p, symmetric positive semi-definite; sW = 0: one shared slot
 * (nslots must be 1; sO alike).  list: nlist slot numbers.  G, Wt: [nslots][sO] out, uploaded before the launch - what no kernel stores comes back as it
 * went in -; ldet (may be NULL: not computed): [nlist][T], indexed by LIST POSITION.  A band of 1024 doubles sits behind each; the call fails if one
 * changed.  W has 128 elements of `fill` behind it.  *per_block out: matrices per workgroup of the form that ran.
 * Impossible geometry is refused before anything is allocated or launched, with a code of its own. */
enum {
  PGPFA_BINB_BAD_ARG = 130,         /* null pointer, sizes below 1 */
  PGPFA_BINB_REFUSED_P = 131,       /* p above 32 */
  PGPFA_BINB_REFUSED_LIST = 132,    /* list entry outside the slots, or a slot twice */
  PGPFA_BINB_REFUSED_STRIDE = 133   /* sW or sO below T p^2 (0 with more than one slot) */
};
int pgpfa_test_bin_blocks(pgpfa_ctx* ctx, int p, int T, double eps, int nslots, int nlist, const int32_t* list, long long sW, long long sO, double fill,
                          const double* W, double* G, double* Wt, double* ldet, int32_t* per_block);
/* pgpfa_test_assemble_b: B = I + F^T Wt F of the low-rank engine (assemble_b_kernel_t<double | float> and pad_identity_kernel) on caller data, through the
 * rank tables' builder (rank_layout, b_layout_of) and the launch code of the covariance pass (assemble_rxr_launch); device buffers of its own, the context
 * only lends its stream.  Geometry by the rule of the rank tables (see pgpfa_test_thin); it comes back in
 * geom = [rr (p), rk (p), roff (p + 1), roff16 (p + 1), rtot, rtot16, rpad, compact, nblk64, npairs, nact], the tables in blk_lat / blk_col (ntab[0] entries)
 * and cmap (ntab[1] entries; none with gran 16), at most tab_cap ints each.
 * F: slabs [p][Tf][Tf], element (t, j) of latent l at l Tf Tf + j Tf + t; columns [ranks[l], rk_l) must hold zeros, rows t >= T any finite value (they are
 *   read up to round_up(T, 32) - 1 and meet zero weights).  With f32 the slabs are converted by cvt_f32_kernel, as the covariance pass converts them.
 * Wt: [nslots][sW] doubles, bin t of slot s at s sW + t p p, entry (ka, kb) at ka p + kb, symmetric per bin (the kernel's contract); sW = 0: one shared
 *   slot (nslots must be 1).  Only the listed slots are read.
 * list: nlist slot numbers; B: [nslots][rpad][rpad] doubles (floats with f32), entry (row, col) of a slot at col rpad + row, uploaded before the launch -
 *   what no kernel stores comes back as it went in - with a band of 1024 doubles behind it; the call fails if the band changed.  rpad_expected: the rpad
 *   the caller sized B for.  F and Wt have 128 elements of `fill` behind them.
 * Impossible geometry is refused before anything is allocated or launched, with a code of its own (the text is in pgpfa_last_error). */
enum {
  PGPFA_ASMB_BAD_ARG = 110,         /* null pointer, sizes below 1, p above 32, unknown granularity, rpad_expected or tab_cap that do not fit */
  PGPFA_ASMB_REFUSED_TF = 111,      /* Tf below round_up(T, 32) */
  PGPFA_ASMB_REFUSED_RANK = 112,    /* a rank outside 1..T */
  PGPFA_ASMB_REFUSED_LIST = 113,    /* list entry outside the slots, or a slot twice */
  PGPFA_ASMB_REFUSED_STRIDE = 114   /* sW below T p^2 (sW = 0 with more than one slot) */
};
int pgpfa_test_assemble_b(pgpfa_ctx* ctx, int p, int T, int Tf, const int32_t* ranks, int gran, int f32, int nslots, int nlist, const int32_t* list,
                          long long sW, double fill, const double* F, const double* Wt, void* B, int rpad_expected, int32_t* geom /* [4 p + 9] */,
                          int tab_cap, int32_t* blk_lat, int32_t* blk_col, int32_t* cmap, int32_t* ntab /* [2] */);
/* Times `reps` launches of the dominant kernel (batched trailing SYRK update, K=512) with HIP
 * events on the context stream; returns average ms per launch and the flops of one launch. */
int pgpfa_bench_syrk(pgpfa_ctx* ctx, int batch, int n, int k, int reps, double* ms_per_launch,
                     double* flops_per_launch);
/* GEMM launches since option "profile" was switched on, grouped by operand shape (text, one line per shape: launches, total ms, algorithmic
 * GFLOP, TFLOP/s; longest total first).  Returns the bytes the full report needs incl. the terminator; writes at most len. */
int pgpfa_gemm_shape_report(pgpfa_ctx* ctx, char* buf, int len);
/* Phase timings of the 128 x 128 diagonal-block kernel (chol.h): phases 0 = load/store only, 1 = + Cholesky steps, 3 = + inverse; + 4 (5, 7): the
 * round-1 form of the Cholesky steps (a row and 32 columns per thread) instead of the 4 x 8 register blocks. */
int pgpfa_bench_potrf_diag(pgpfa_ctx* ctx, int batch, int reps, int phases, double* us_per_launch);
/* Sustained v_mfma_f64_16x16x4_f64 rate of the device (register-only loop): the practical MFMA
 * ceiling under the clock the chip holds, reported next to the datasheet peak. */
int pgpfa_bench_mfma_peak(pgpfa_ctx* ctx, int iters, double* tflops);
/* The host half of pgpfa_posterior_rates' group table, no device and no context: the list positions first..last-1 of every group in list order as
 * CSR - positions of group g are pos[start[g] .. start[g + 1]), pos holding last - first entries.  Fails on a group id outside 0..n_groups-1. */
int pgpfa_rates_group_csr(int n, const int32_t* group /* [n] */, int n_groups, int first, int last, int32_t* start /* [n_groups + 1] */,
                          int32_t* pos /* [last - first] */);

#ifdef __cplusplus
}
#endif
#endif /* PGPFA_H */
