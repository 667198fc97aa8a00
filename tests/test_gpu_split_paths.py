"""Every path of the split covariance sum end to end against a dense FP64 inverse (oracle.laplace_cov_at at the device's own modes), with the
tolerances and helpers of tests/test_gpu_dense_covariance.py: mode gradient <= 1e-6 first, then the post_vsm blocks of a few trials 1e-8 (per bin
1e-6), PautoSum over all trials 1e-9 and its covariance part 1e-8.

The counts are drawn from the model at rates high enough that the measured rms of eps ||Wt|| lies between 0.02 and 0.06 (the split form's guard
is 0.07): the single-precision correction D and with it the FP16 and cross terms are as heavy as the split form admits.  Every case asserts that
range, that the split form ran, and the four info keys that name the path it took (last_syrk_tile, last_split_sps, last_cross_kernel,
last_mix_form): a case that meant one path and got another fails.  p T <= 1100 and R <= 70 keep the dense inversions to a few seconds.

What the tolerance of the covariance part has to hold besides the device's arithmetic: the engine replaces the RBF part of every prior Gram matrix by
its pivoted Cholesky factors, stopped when the largest remaining diagonal entry is <= lowrank_tol (1e-10, absolute, against a prior variance of 1).
The residual dK moves the posterior covariance by (I + K W)^-1 dK (I + W K)^-1, up to 1e-10 per entry, whatever the rates; the raised rates of these
cases shrink the posterior covariance itself to 6e-3 .. 4e-2, so that share can reach 1e-8 of it without any kernel being wrong (at the bench's rates
it stays below 1e-9).  truncation_share() computes it in numpy, with no device code; tests/test_cpu_split_kernels.py asserts that it takes at most half
of the 1e-8 in every case, which leaves the other half to the device.  It is why tiles_256 has timescales of 5 and 15 bins: short timescales keep the
posterior variance largest at given rates (with 15 and 50 bins that share alone is 1.2e-8, and the device, split form or FP64 product alike, returns
1.17e-8)."""
import time

import numpy as np
import pytest

from oracle import pgpfa_oracle as orc
from test_gpu_dense_covariance import _check_pautosum, _dense, _max_grad

pytestmark = pytest.mark.gpu

PATH_KEYS = ('last_syrk_tile', 'last_split_sps', 'last_cross_kernel', 'last_mix_form')


def loud_problem(q, p, T, R, tau, d0, seed):
    """Parameters with the given timescales and offsets d0 + 0.3 N(0, 1), counts drawn from the model (as _edge_problem of
    test_gpu_dense_covariance.py draws them)."""
    rng = np.random.default_rng(seed)
    tau = np.asarray(tau, dtype=np.float64)
    par = {'C': 0.4 * rng.standard_normal((q, p)) / np.sqrt(p), 'd': d0 + 0.3 * rng.standard_normal(q), 'tau': tau}
    L = np.linalg.cholesky(orc.make_K(tau, T, 10.0))
    Ys, Xs = [], []
    for _ in range(R):
        X = np.einsum('kts,ks->kt', L, rng.standard_normal((p, T)))
        Xs.append(X)
        Ys.append(np.minimum(rng.poisson(np.exp(par['C'] @ X + par['d'][:, None])), 60000).astype(np.uint16))
    return par, Ys, Xs


def taus(p, full_rank=()):
    """timescales of 15 .. 50 bins; of one bin (full rank) for the latents listed"""
    t = np.linspace(0.15, 0.5, p) if p > 1 else np.array([0.3])
    for k in full_rank:
        t[k] = 0.01
    return t


# name: (q, p, T, R, timescales, offset d0, [(options, expected path), ...]); the runs of a case share the data; every run finds its own modes
CASES = {
    # groups of two slots, the last group ragged (67 = 33 x 2 + 1); then the same with the cross term through the segmented-K GEMM
    'groups_of_two': (30, 3, 130, 67, taus(3), 2.2, [
        ({}, dict(last_syrk_tile=128, last_split_sps=2, last_cross_kernel=1, last_mix_form=4)),
        ({'cross_kernel': 0}, dict(last_syrk_tile=128, last_split_sps=2, last_cross_kernel=0, last_mix_form=4))]),
    # 256 x 256 tiles with groups of two; then 128 x 128 tiles forced (timescales of 5 and 15 bins: see the module's docstring; the first latent's
    # rank of about 240 also takes two row launches of cross_term_kernel at T = 500)
    'tiles_256': (40, 2, 500, 67, np.array([0.05, 0.15]), 1.7, [
        ({}, dict(last_syrk_tile=256, last_split_sps=2, last_cross_kernel=1, last_mix_form=4)),
        ({'syrk_tile': 128}, dict(last_syrk_tile=128, last_split_sps=2, last_cross_kernel=1, last_mix_form=4))]),
    # latent stride T = 203 (slab_row_align 0): no multiple of 4, the 128-tile kernel takes its slow loads in every tile
    'unaligned_stride': (30, 3, 203, 8, taus(3), 2.3, [
        ({'slab_row_align': 0}, dict(last_syrk_tile=128, last_split_sps=1, last_cross_kernel=1, last_mix_form=4))]),
    # the stand-alone mixing passes: p = 7 is no template width (dispatch_pw: 8), so mix_slot 2 and 3 fall back to mix_slot_kernel as cov.hip documents
    'mix_p7': (40, 7, 150, 6, taus(7), 2.5, [
        ({'yt_mix': 0, 'mix_slot': m}, dict(last_syrk_tile=128, last_split_sps=1, last_cross_kernel=1, last_mix_form=f)) for m, f in ((0, 0), (1, 1), (2, 1), (3, 1))]),
    # at template widths every form runs: p = 8 (two 128-bin blocks of mix_slot3) and p = 4 with T = 260 (two 256-bin blocks of mix_slot / mix_slot2,
    # three of mix_slot3, five 64-bin blocks of mix_vsm_split)
    'mix_p8': (40, 8, 130, 6, taus(8), 2.9, [
        ({'yt_mix': 0, 'mix_slot': m}, dict(last_syrk_tile=128, last_split_sps=1, last_cross_kernel=1, last_mix_form=m)) for m in (0, 1, 2, 3)]),
    'mix_p4': (40, 4, 260, 6, taus(4), 2.0, [
        ({'yt_mix': 0, 'mix_slot': m}, dict(last_syrk_tile=128, last_split_sps=1, last_cross_kernel=1, last_mix_form=m)) for m in (0, 1, 2, 3)]),
    # 11 .. 16 latents: mix_vsm_split_kernel<12> and <16> with masked rows
    'p11': (40, 11, 90, 6, taus(11), 2.8, [({}, dict(last_syrk_tile=128, last_split_sps=1, last_cross_kernel=1, last_mix_form=0))]),
    'p13': (40, 13, 80, 6, taus(13), 2.85, [({}, dict(last_syrk_tile=128, last_split_sps=1, last_cross_kernel=1, last_mix_form=0))]),
    # a latent with a timescale of one bin: full rank 150 (160 rows padded), two row launches of cross_term_kernel
    'full_rank_latent': (30, 3, 150, 6, taus(3, full_rank=(1,)), 2.6, [
        ({}, dict(last_syrk_tile=128, last_split_sps=1, last_cross_kernel=1, last_mix_form=4))]),
}


LOWRANK_TOL = 1e-10        # the engine's default stop of the pivoted Cholesky (option lowrank_tol)


def pivoted_cholesky_residual(G, tol):
    """G - F F^T and the rank of the pivoted Cholesky factor F of G, stopped when the largest remaining diagonal entry is <= tol"""
    T = len(G)
    d = np.diag(G).copy()
    F = np.zeros((T, 0))
    while F.shape[1] < T:
        j = int(np.argmax(d))
        if not d[j] > tol:
            break
        col = (G[:, j] - F @ F[j]) / np.sqrt(d[j])
        F = np.column_stack([F, col])
        d -= col ** 2
        d[j] = 0.0
    return G - F @ F.T, F.shape[1]


def truncation_share(name, trials=2):
    """What the truncated prior factors alone do to the covariance part of PautoSum, as _check_pautosum measures it (largest error over a latent's
    largest entry), in plain numpy: (I + K W)^-1 dK (I + W K)^-1 summed over the first `trials` trials of the case, against the sum of their exact
    posterior covariances, with W at the latents the counts were drawn from (the modes lie near them).  Returns the share per latent and the ranks."""
    q, p, T, R, tau, d0, _ = CASES[name]
    par, _, Xs = loud_problem(q, p, T, R, tau, d0, seed=q * 1000 + p * 100 + T)
    K = orc.make_K(par['tau'], T, 10.0)
    dK, ranks = np.zeros((p * T, p * T)), []
    for k in range(p):
        res, r = pivoted_cholesky_residual((K[k] - orc.EPS_NOISE * np.eye(T)) / (1.0 - orc.EPS_NOISE), LOWRANK_TOL)
        dK[k * T:(k + 1) * T, k * T:(k + 1) * T] = (1.0 - orc.EPS_NOISE) * res
        ranks.append(r)
    Kb = orc.make_K_big(K)
    S, E = np.zeros((p, T, T)), np.zeros((p, T, T))
    for X in Xs[:trials]:
        Wt = np.einsum('qk,qt,ql->tkl', par['C'], np.exp(par['C'] @ X + par['d'][:, None]), par['C'])
        W = np.zeros((p * T, p * T))
        for k in range(p):
            for l in range(p):
                W[k * T + np.arange(T), l * T + np.arange(T)] = Wt[:, k, l]
        A = np.linalg.solve(np.eye(p * T) + Kb @ W, np.eye(p * T))
        Sig, dS = A @ Kb, A @ dK @ A.T
        for k in range(p):
            S[k] += Sig[k * T:(k + 1) * T, k * T:(k + 1) * T]
            E[k] += dS[k * T:(k + 1) * T, k * T:(k + 1) * T]
    return np.max(np.abs(E), axis=(1, 2)) / np.max(np.abs(S), axis=(1, 2)), ranks


def _check_vsm(tag, r, vsm, ref_vsm):
    """post_vsm of one trial with the tolerances of _check_blocks (test_gpu_dense_covariance.py): 1e-8 of the trial's largest block entry, 1e-6 of every
    bin's own largest entry.  (The per-trial T x T blocks are not an output of the sum-only pass: PautoSum below is what the split form produces.)"""
    err = np.abs(vsm - ref_vsm)
    e_vsm = np.max(err) / np.max(np.abs(ref_vsm))
    e_bin = np.max(np.max(err, axis=(1, 2)) / np.max(np.abs(ref_vsm), axis=(1, 2)))
    print('%s trial %4d: post_vsm %.2e (worst bin %.2e)' % (tag, r, e_vsm, e_bin))
    assert e_vsm <= 1e-8 and e_bin <= 1e-6


@pytest.mark.parametrize('name', list(CASES))
def test_split_path_against_dense_fp64(name):
    from funs import _hip
    q, p, T, R, tau, d0, runs = CASES[name]
    assert p * T <= 1100 and R <= 70
    par, Ys, _ = loud_problem(q, p, T, R, tau, d0, seed=q * 1000 + p * 100 + T)
    Y = np.stack(Ys)
    Kinv = np.linalg.inv(orc.make_K(par['tau'], T, 10.0))
    sidx = np.array(sorted({0, 1, R // 2, R - 2, R - 1}), dtype=np.int32)[:4] if R > 8 else np.array([0, R - 1], dtype=np.int32)
    t_dense, n_dense, dense = 0.0, 0, None
    t_start = time.time()
    for opts, expect in runs:
        tag = '%s %s' % (name, opts if opts else 'defaults')
        ctx = _hip.Context(q, p, T, R, 10.0)
        try:
            ctx.upload_counts(Y)
            ctx.set_option('cov_mode', 2)
            ctx.set_option('measure_mix', 1)
            for k, v in opts.items():
                ctx.set_option(k, v)
            ctx.set_params(par['C'], par['d'], par['tau'])
            _, _, st = ctx.estep_laplace()
            assert np.all(st == 0)
            got = {k: ctx.info(k) for k in PATH_KEYS + ('last_split_cov', 'last_eps_wt_rms', 'last_yt_mix_fused', 'lowrank_rtot', 'chunk_trials')}
            print('%s: %s' % (tag, ', '.join('%s %g' % kv for kv in got.items())))
            assert got['last_split_cov'] == 1.0
            assert 0.02 <= got['last_eps_wt_rms'] <= 0.06
            for k, v in expect.items():
                assert got[k] == float(v), (k, got[k], v)
            if name == 'full_rank_latent':
                assert got['lowrank_rtot'] >= 150 + 2 * 16       # the full-rank latent's 150 rows: cross_term_kernel runs rows 0 .. 127 and 128 .. 159
            assert ctx.mstep_precomp() == float(R)
            P = ctx.pautosum().copy()
            pm = ctx.post_mean()
            vsm_dev = ctx.post_vsm(sidx)
        finally:
            ctx.close()
        if dense is None or not np.array_equal(dense[0], pm):        # (the options of a case touch the covariance pass only: the modes are the same bits)
            t1 = time.time()
            dense = (pm,) + _dense(par, pm, T)
            t_dense += time.time() - t1
            n_dense += R
        _, ref_vsm, ref_gp = dense
        for i, r in enumerate(sidx):
            assert _max_grad(Ys[r], par['C'], par['d'], Kinv, pm[r]) <= 1e-6
            _check_vsm(tag, r, vsm_dev[i], ref_vsm[r])
        _check_pautosum(tag + ':', P, pm, ref_gp)
    print('%s: %.1f s, of which %d dense inversions %.1f s' % (name, time.time() - t_start, n_dense, t_dense))
