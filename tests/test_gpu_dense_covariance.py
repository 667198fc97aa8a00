"""The covariance engine against a plain dense FP64 inverse (oracle.laplace_cov_at: the p T x p T Hessian of inference.py:50-65 inverted
by LAPACK, blocks of inference.py:164-172) at the DEVICE's own modes, where the headline number is measured:

* A - the bench's operating point: batch EM at 200 x 10 x 500 x 1024 from the Poisson-PCA start, the fourth E-step (rank total 448 in compact
  offsets, 480 rounded to 16 - measured -, the fused yt_mix pass writing D in FP32, the FP16 split form of the sum over trials,
  sum_groups_kernel over 16-slot groups);
* B - the plateau: 48 trials at the generating parameters (rank total 1068);
* C - compact-offset edges (p T just below a multiple of 128, T % 4 != 0, a full-rank LAST latent) against the oracle's exact Laplace;
* D - options set AFTER pgpfa_set_params give the numbers of the same options set before it.

Every test prints the errors it measured."""
import time

import numpy as np
import pytest

from oracle import pgpfa_oracle as orc

pytestmark = pytest.mark.gpu

EPS = orc.EPS_NOISE
SLOT_POSITIONS = [0, 7, 8, 15, 16, 511, 512, 1016, 1023]     # XCD groups of 8, split groups of 16, the last group of a 1024-slot chunk


def _wt_norms(C, d, pm):
    """max over the bins of eps ||W_t||_2, W_t = C^T diag(exp(C m_t + d)) C, for every trial (the size of the correction the FP32 / FP16
    parts of the split covariance form carry)"""
    q, p = C.shape
    CC = (C[:, :, None] * C[:, None, :]).reshape(q, p * p)
    out = np.empty(len(pm))
    for r, m in enumerate(pm):
        W = (np.exp(C @ m + d[:, None]).T @ CC).reshape(-1, p, p)
        out[r] = EPS * np.max(np.linalg.eigvalsh(W)[:, -1])
    return out


def _max_grad(Y, C, d, Kinv, X):
    return float(np.max(np.abs(orc.nlp_grad(X, Y.astype(np.float64), C, d, Kinv))))


def _check_blocks(tag, r, vsm, gp, ref_vsm, ref_gp):
    """post_vsm: 1e-8 of the trial's largest block entry and 1e-6 of every bin's own largest entry (a wrong bin, a wrong tail tile);
    post_vsmGP: 1e-8 of every latent block's largest entry.  Returns the three errors."""
    err = np.abs(vsm - ref_vsm)
    e_vsm = np.max(err) / np.max(np.abs(ref_vsm))
    e_bin = np.max(np.max(err, axis=(1, 2)) / np.max(np.abs(ref_vsm), axis=(1, 2)))
    e_gp = np.max(np.max(np.abs(gp - ref_gp), axis=(0, 1)) / np.max(np.abs(ref_gp), axis=(0, 1)))
    print('%s trial %4d: post_vsm %.2e (worst bin %.2e), post_vsmGP %.2e' % (tag, r, e_vsm, e_bin, e_gp))
    assert e_vsm <= 1e-8 and e_bin <= 1e-6 and e_gp <= 1e-8
    return np.array([e_vsm, e_bin, e_gp])


def _check_pautosum(tag, P, pm, gps):
    """P (p,T,T) against sum_r (Sigma_kk,r + m_r m_r^T) with the dense blocks gps (R,T,T,p) at the device modes pm: 1e-9 of every latent's
    largest entry; and the covariance part alone (m m^T dominates PautoSum and could hide an error) to 1e-8 of ITS largest entry per latent."""
    M = np.einsum('rkt,rks->kts', pm, pm)
    S = np.sum(gps, axis=0).transpose(2, 0, 1)
    ref = S + M
    assert P.shape == ref.shape
    e_all = np.max(np.max(np.abs(P - ref), axis=(1, 2)) / np.max(np.abs(ref), axis=(1, 2)))
    e_cov = np.max(np.max(np.abs((P - M) - S), axis=(1, 2)) / np.max(np.abs(S), axis=(1, 2)))
    print('%s PautoSum over %d trials vs dense: %.2e of each latent\'s largest entry, covariance part %.2e' % (tag, len(pm), e_all, e_cov))
    assert e_all <= 1e-9 and e_cov <= 1e-8


def _dense(par, pm, T):
    """dense FP64 post_vsm (R,T,p,p) and post_vsmGP (R,T,T,p) at the modes pm"""
    out = [orc.laplace_cov_at(m, par['C'], par['d'], par['tau'], T, 10.0) for m in pm]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


@pytest.mark.timeout(1200)
def test_bench_operating_point_against_dense_fp64():
    """Test A.  The loop of test_gpu_round6's bench-workload test (bench.synth_shard(..., 12, 0), np.random.seed(0) Poisson-PCA start,
    4 x (inference.laplace with prevOptimRes, updateParams 'newton')); the fourth E-step (extrapolated warm start) is checked against dense
    FP64 at the device's modes after a guard that it took the bench's path: low-rank plan and covariance, split form, fused yt_mix, compact
    offsets that save rows, one chunk of 1024 slots, no dense retry.  Blocks of about 12 trials: slot positions 0, 7, 8, 15, 16, 511, 512,
    1016, 1023, the two largest max_t eps ||W_t|| and the fewest spikes, each at a mode with max |gradient| <= 1e-6.  Then PautoSum: the
    M-step's over 1024 trials is the sum of the ones over a 40-trial subset A that holds the sampled trials (sum_groups_kernel runs its
    8-wide loop and its tail) and over its 984-trial complement (62 split groups of 16 slots), and P_A matches dense.
    Measured: blocks 3.3e-10 (per bin 9.8e-10, post_vsmGP 4.5e-10), PautoSum 7.4e-12 (covariance part 3.7e-10), P_A + P_B 4.3e-13."""
    import bench
    import funs
    from funs import _session
    q, p, T, R = 200, 10, 500, 1024
    _session.drop_sessions()
    true, Ys = bench.synth_shard(q, p, T, R, 12, 0)
    exp = bench.Shard(Ys, 10.0)
    np.random.seed(0)
    params = {k: np.real(np.asarray(v)).astype(np.float64) for k, v in funs.util.initializeParams(p, q, exp).items()}
    t0 = time.time()
    optim = None
    for it in range(4):
        infRes, nll, optim = funs.inference.laplace(exp, params, prevOptimRes=optim)
        ctx = infRes.session.ctx
        assert np.all(infRes.newton_status == 0)
        if it < 3:
            params, _ = funs.learning.updateParams(params, infRes, exp, CdOptimMethod='newton')
    par = params                                                   # the parameters of the E-step under test
    flags = {k: ctx.info(k) for k in ('plan_lowrank', 'last_cov_lowrank', 'last_split_cov', 'last_yt_mix_fused', 'chunk_trials', 'last_dense_retries',
                                       'lowrank_compact', 'lowrank_rtot', 'lowrank_rtot16')}
    print('iteration 3 path: %s' % ', '.join('%s %g' % kv for kv in flags.items()))
    assert flags['plan_lowrank'] == 1.0 and flags['last_cov_lowrank'] == 1.0 and flags['last_split_cov'] == 1.0 and flags['last_yt_mix_fused'] == 1.0
    assert flags['chunk_trials'] == float(R) and flags['last_dense_retries'] == 0.0
    assert flags['lowrank_compact'] == 1.0 and flags['lowrank_rtot'] < flags['lowrank_rtot16']
    all_idx = np.arange(R, dtype=np.int32)
    pm_all = ctx.post_mean(all_idx)
    nspk = np.array([int(np.sum(y)) for y in Ys])
    wt = _wt_norms(par['C'], par['d'], pm_all)
    extra = []
    for r in [int(x) for x in np.argsort(-wt)[:2]] + [int(np.argmin(nspk))]:
        if r not in SLOT_POSITIONS and r not in extra:
            extra.append(r)
    sample = sorted(SLOT_POSITIONS + extra)
    print('sampled trials %s; max_t eps ||W_t|| from %.4f to %.4f (largest: trials %s), fewest spikes %d (trial %d)'
          % (sample, wt.min(), wt.max(), [int(x) for x in np.argsort(-wt)[:2]], nspk.min(), int(np.argmin(nspk))))
    sidx = np.array(sample, dtype=np.int32)
    vsm_dev = ctx.post_vsm(sidx)
    gp_dev = np.stack([infRes['post_vsmGP'][int(r)] for r in sidx])
    # the PautoSum the M-step of this iteration uses
    funs.learning.updateParams(par, infRes, exp, CdOptimMethod='newton')
    P_all = ctx.pautosum().copy()
    t_gpu = time.time() - t0
    Kinv = np.linalg.inv(orc.make_K(par['tau'], T, 10.0))
    t1 = time.time()
    ref_vsm, ref_gp = _dense(par, pm_all[sidx], T)
    t_dense = time.time() - t1
    worst = np.zeros(3)
    for i, r in enumerate(sidx):
        g = _max_grad(Ys[r], par['C'], par['d'], Kinv, pm_all[r])
        assert g <= 1e-6, (r, g)
        worst = np.maximum(worst, _check_blocks('bench point', r, vsm_dev[i], gp_dev[i], ref_vsm[i], ref_gp[i]))
    # PautoSum of the same parameters over A (40 trials) and its complement B (984)
    t0 = time.time()
    ctx.set_params(par['C'], par['d'], par['tau'])
    others = [int(r) for r in np.linspace(0, R - 1, 64).astype(int) if int(r) not in sample]
    A = np.array(sorted(sample + others[:40 - len(sample)]), dtype=np.int32)
    B = np.setdiff1d(all_idx, A).astype(np.int32)
    assert len(A) == 40 and len(B) == 984
    out = {}
    for tag, idx in (('A', A), ('B', B)):
        _, _, st = ctx.estep_laplace(idx, warm_start=True)
        assert np.all(st == 0)
        assert ctx.mstep_precomp() == float(len(idx))
        out[tag] = (ctx.pautosum().copy(), ctx.post_mean(idx))
    t_gpu += time.time() - t0
    e_sum = np.max(np.max(np.abs(out['A'][0] + out['B'][0] - P_all), axis=(1, 2)) / np.max(np.abs(P_all), axis=(1, 2)))
    print('P_A + P_B vs the M-step\'s P_all: %.2e of each latent\'s largest entry' % e_sum)
    assert e_sum <= 1e-8
    t1 = time.time()
    _, gpA = _dense(par, out['A'][1], T)
    t_dense += time.time() - t1
    _check_pautosum('bench point, subset A:', out['A'][0], out['A'][1], gpA)
    print('bench point: worst post_vsm %.2e, per bin %.2e, post_vsmGP %.2e; GPU part %.1f s, %d dense inversions %.1f s'
          % (worst[0], worst[1], worst[2], t_gpu, len(sidx) + len(A), t_dense))
    _session.drop_sessions()


@pytest.mark.timeout(1200)
def test_plateau_ranks_against_dense_fp64():
    """Test B.  A fresh context with the first 48 trials of the bench's data at the generating parameters (rank ~1070) and default options:
    low-rank plan, compact offsets, rank >= 1000, every status 0; blocks of 6 trials and PautoSum over all 48 against dense FP64 at the
    device modes with the tolerances of test A.  Prints whether the split form and the fused pass ran and the measured rms of eps ||W_t||
    (both ran at these rates: rms 0.0127 against the split form's bound of 0.07).  Measured: post_vsm 5.7e-10, post_vsmGP 4.1e-9 of a latent
    block's largest entry - the low-rank factors stop at a residual of 1e-10 (option lowrank_tol) and the plateau's ranks are the largest -
    PautoSum 6.7e-11, covariance part 4.0e-9."""
    import bench
    from funs import _hip
    q, p, T, R = 200, 10, 500, 48
    true, Ys = bench.synth_shard(q, p, T, 1024, 12, 0)
    Ys = Ys[:R]
    par = {k: np.asarray(v, dtype=np.float64) for k, v in true.items()}
    ctx = _hip.Context(q, p, T, R, 10.0)
    try:
        ctx.upload_counts(np.stack(Ys))
        ctx.set_option('measure_mix', 1)
        ctx.set_params(par['C'], par['d'], par['tau'])
        t0 = time.time()
        _, _, st = ctx.estep_laplace()
        assert np.all(st == 0)
        flags = {k: ctx.info(k) for k in ('plan_lowrank', 'last_cov_lowrank', 'lowrank_compact', 'lowrank_rtot', 'lowrank_rtot16', 'last_split_cov',
                                           'last_yt_mix_fused', 'last_eps_wt_rms', 'last_eps_wt_norm', 'last_dense_retries')}
        print('plateau path: %s' % ', '.join('%s %g' % kv for kv in flags.items()))
        assert flags['plan_lowrank'] == 1.0 and flags['last_cov_lowrank'] == 1.0 and flags['lowrank_compact'] == 1.0
        assert flags['lowrank_rtot'] >= 1000 and flags['lowrank_rtot'] < flags['lowrank_rtot16']
        assert ctx.mstep_precomp() == float(R)
        P = ctx.pautosum().copy()
        pm = ctx.post_mean()
        sidx = np.array([0, 7, 8, 15, 16, 47], dtype=np.int32)
        vsm_dev = ctx.post_vsm(sidx)
        gp_dev = ctx.post_vsmgp(sidx)
        t_gpu = time.time() - t0
    finally:
        ctx.close()
    Kinv = np.linalg.inv(orc.make_K(par['tau'], T, 10.0))
    t1 = time.time()
    ref_vsm, ref_gp = _dense(par, pm, T)
    t_dense = time.time() - t1
    for i, r in enumerate(sidx):
        assert _max_grad(Ys[r], par['C'], par['d'], Kinv, pm[r]) <= 1e-6
        _check_blocks('plateau', r, vsm_dev[i], gp_dev[i], ref_vsm[r], ref_gp[r])
    _check_pautosum('plateau:', P, pm, ref_gp)
    print('plateau: GPU part %.1f s, %d dense inversions %.1f s' % (t_gpu, R, t_dense))


def _edge_problem(q, p, T, R, rng):
    """Timescales of one bin (full rank) on every third latent and on the LAST one, long ones (15-50 bins) on the others; counts drawn
    from the model."""
    tau = 0.15 + 0.35 * rng.random(p)
    tau[1::3] = 0.01
    tau[-1] = 0.01
    par = {'C': 0.4 * rng.standard_normal((q, p)) / np.sqrt(p), 'd': -0.5 + 0.3 * rng.standard_normal(q), 'tau': tau}
    L = np.linalg.cholesky(orc.make_K(tau, T, 10.0))
    Ys = []
    for _ in range(R):
        X = np.einsum('kts,ks->kt', L, rng.standard_normal((p, T)))
        Ys.append(rng.poisson(np.exp(par['C'] @ X + par['d'][:, None])).astype(np.uint8))
    return par, Ys


@pytest.mark.parametrize('shape', [(30, 7, 73), (25, 5, 51), (20, 3, 85)])
@pytest.mark.parametrize('cov_mode', [2, 0])
def test_compact_offset_edges_against_the_oracle(shape, cov_mode):
    """Test C.  p T just below a multiple of 128 (511, 255, 255), T % 4 != 0 (a tail tile of 1 or 3 bins), full-rank latents with a
    timescale of one bin next to long ones, the LAST latent full rank (its rank rounded to 16 reaches past the compact rank total), 4 trials:
    modes, post_vsm, per-trial post_vsmGP against the oracle's exact Laplace (polished Newton, inverse of the dense Hessian) and PautoSum
    against orc.make_precomp, 1e-8 of the largest entry.  These shapes sit where want_lowrank and rpad <= ld meet: cov_mode 2 must run the
    low-rank engine with compact offsets; cov_mode 0 picks an engine by cost (printed)."""
    from funs import _hip
    q, p, T = shape
    R = 4
    par, Ys = _edge_problem(q, p, T, R, np.random.default_rng(q * 100 + T))
    ref, _, _ = orc.laplace([y.astype(np.float64) for y in Ys], par, 10.0, mode='exact', return_cov=False)
    Pref, _ = orc.make_precomp(ref)
    ctx = _hip.Context(q, p, T, R, 10.0)
    try:
        ctx.upload_counts(np.stack(Ys))
        ctx.set_option('cov_mode', cov_mode)
        ctx.set_params(par['C'], par['d'], par['tau'])
        _, _, st = ctx.estep_laplace()
        assert np.all(st == 0) and ctx.info('last_dense_retries') == 0.0
        plan = {k: ctx.info(k) for k in ('plan_lowrank', 'last_cov_lowrank', 'lowrank_compact', 'lowrank_rtot', 'lowrank_rtot16')}
        assert ctx.mstep_precomp() == float(R)
        pm, vsm, gp, P = ctx.post_mean(), ctx.post_vsm(), ctx.post_vsmgp(), ctx.pautosum()
    finally:
        ctx.close()

    def rel(a, b):
        return np.max(np.abs(a - b)) / np.max(np.abs(b))
    e = (np.max(np.abs(pm - np.stack(ref['post_mean']))), rel(vsm, np.stack(ref['post_vsm'])), rel(gp, np.stack(ref['post_vsmGP'])), rel(P, Pref))
    print('%s cov_mode %d: %s; modes %.2e, post_vsm %.2e, post_vsmGP %.2e, PautoSum %.2e'
          % (shape, cov_mode, ', '.join('%s %g' % kv for kv in plan.items()), *e))
    if cov_mode == 2:
        assert plan['plan_lowrank'] == 1.0 and plan['lowrank_compact'] == 1.0
    assert e[0] <= 1e-8 and max(e[1:]) <= 1e-8


@pytest.mark.parametrize('shape', [(40, 7, 70, 6), (200, 10, 500, 32)])
@pytest.mark.parametrize('opt', [('use_mfma', 1, 0), ('use_mfma', 0, 1), ('eps_noise', EPS, 1e-2), ('thin_products', 2, 0), ('rank_gran', 16, 4)],
                         ids=['use_mfma_1to0', 'use_mfma_0to1', 'eps_noise', 'thin_products_2to0', 'rank_gran_16to4'])
def test_option_set_after_set_params_changes_nothing(shape, opt):
    """Test D.  An option that pgpfa_set_params builds from (the rank tables: use_mfma, thin_products, rank_gran; the Gram matrices and the
    low-rank factors: eps_noise), set from `old` to `new` AFTER set_params, against a context where `new` was set BEFORE it (low-rank
    engine, cov_mode 2): the same plan, objective, modes, post_vsm and PautoSum to 1e-10 relative.  The call may raise HipBackendError
    instead; it must never return other numbers silently (before the fix, use_mfma 1 -> 0 sent the compact rank tables through the general
    GEMM, and eps_noise changed the E-step's per-bin arithmetic but not the Gram matrices and low-rank factors it goes with)."""
    from funs import _hip
    key, old, new = opt
    q, p, T, R = shape
    rng = np.random.default_rng(q * 1000 + p)
    _, Ys, _ = orc.synth_dataset(q, p, T, R, seed=p, dOffset=0.0)
    Y = np.stack(Ys).astype(np.uint8)
    par = {'C': 0.3 * rng.standard_normal((q, p)) / np.sqrt(max(1, p / 4)), 'd': np.log(Y.mean(axis=(0, 2)) + 0.1), 'tau': 0.05 + 0.3 * rng.random(p)}
    out = {}
    for after in (False, True):
        ctx = _hip.Context(q, p, T, R, 10.0)
        try:
            ctx.upload_counts(Y)
            ctx.set_option('cov_mode', 2)
            ctx.set_option(key, old if after else new)
            ctx.set_params(par['C'], par['d'], par['tau'])
            try:
                if after:
                    ctx.set_option(key, new)
                obj, _, st = ctx.estep_laplace()
            except _hip.HipBackendError as exc:
                assert after
                print('%s %s %g -> %g after set_params raised: %s' % (shape, key, old, new, exc))
                return
            assert np.all(st == 0)
            ctx.mstep_precomp()
            out[after] = (obj, ctx.post_mean(), ctx.post_vsm(), ctx.pautosum(), ctx.info('plan_lowrank'), ctx.info('lowrank_rtot'))
        finally:
            ctx.close()
    a, b = out[True], out[False]
    e = (abs(a[0] - b[0]) / abs(b[0]),) + tuple(np.max(np.abs(x - y)) / np.max(np.abs(y)) for x, y in zip(a[1:4], b[1:4]))
    print('%s %s %g -> %g after set_params: plan low-rank %g / %g, rank %g / %g; objective %.2e, modes %.2e, post_vsm %.2e, PautoSum %.2e'
          % (shape, key, old, new, a[4], b[4], a[5], b[5], *e))
    assert a[4] == b[4] and a[5] == b[5]
    assert max(e) <= 1e-10
