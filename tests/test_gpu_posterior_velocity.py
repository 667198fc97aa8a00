"""Value and velocity of every latent at arbitrary time points, with their joint 2 x 2 posterior (pgpfa_posterior_velocity_at,
Context.posterior_velocity_at, util.posteriorVelocityAt):

    kd_k(s)[j] = -1000 (s - j bin) / l_k^2 (1 - eps) exp(-(s - j bin)^2 / (2 l_k^2)),   b = K_k^-1 kd,   kappa_k = (1 - eps) / tau_k^2
    vel = b . m_k,   vel_var = kappa_k - b . kd + b^T V_k b,   cross = -a . kd + a^T V_k b          (mean, var: those of pgpfa_posterior_at)

8 trials, both covariance engines and the sum-only plan of the low-rank one.  Errors are relative to max|m| (mean), max|vel_ref| (vel), 1 (var),
kappa_k (vel_var) and sqrt(kappa_k) (cross).  Tolerances: 1e-9 against numpy_velocity (test_cpu_posterior_velocity.py) on the downloaded post_mean /
post_vsmGP - its two evaluation orders differ by 8.5e-13 at most, ten times which stays below 1e-9; 1e-8 against independent dense FP64 models
(the project's tolerance for modes and blocks against dense FP64); 1e-12 in the far field; the central differences of ctx.posterior_at means use
the step and the limit test_cpu_posterior_velocity.py fixed on the CPU.  Every test prints its figures before it asserts."""
import numpy as np
import pytest

from conftest import Experiment
from oracle import pgpfa_oracle as orc
from test_cpu_posterior_samples import problem
from test_cpu_posterior_velocity import DEVICE_KEYS, FD_H_MS, FD_LIMIT_MEAN, kappa, numpy_velocity, off_grid_times
from test_gpu_posterior_at import CONFIG_IDS, CONFIGS, SHAPES, _var_problem, make_ctx, make_times

pytestmark = pytest.mark.gpu

BIN_MS = 10.0
R8 = 8
IDS = ['q%d-p%d-T%d' % s for s in SHAPES]
S_VALUES = (1, 17, 65, 257)
TOL_SAME, TOL_DENSE, TOL_FAR = 1e-9, 1e-8, 1e-12
ALL = DEVICE_KEYS


def tag(config):
    return CONFIG_IDS[CONFIGS.index(config)]


def same_bits(a, b, keys=None):
    return all(np.array_equal(a[k], b[k]) for k in (keys or a))


def errors(got, ref, tau, m_scale):
    """largest error of every plane of one trial (got, ref: dicts of (p, S)), in the units of the docstring above"""
    kap = kappa(tau)[:, None]
    scale = {'mean': m_scale, 'var': 1.0, 'vel': float(np.max(np.abs(ref['vel']))), 'vel_var': kap, 'cross': np.sqrt(kap)}
    return {k: float(np.max(np.abs(got[k] - ref[k]) / scale[k])) for k in ALL}


def worst(list_of_errors):
    return {k: max(e[k] for e in list_of_errors) for k in ALL}


def fmt(e):
    return ', '.join('%s %.2e' % (k, e[k]) for k in ALL)


def sblk_of(T):
    """query times per workgroup of velat_joint_kernel (csrc/velat.hip: halved from 1024 while panel and sums exceed 160 KiB of LDS)"""
    T4 = (T + 3) // 4 * 4
    VS = T4 + ((2 - T4 % 32) + 32) % 32
    sblk = 1024
    while sblk > 16 and (16 * VS + 3 * sblk) * 8 > 160 * 1024:
        sblk //= 2
    return sblk


# ---- 1. same inputs in plain FP64; the far field; the joint is a covariance; each plane alone -----------------------------------------------------
@pytest.mark.parametrize('config', CONFIGS, ids=CONFIG_IDS)
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_same_inputs_in_plain_fp64_the_far_field_and_each_plane_alone(shape, config):
    q, p, T = shape
    ctx, par, _, _ = make_ctx(shape, config)
    try:
        tau = par['tau']
        kap = kappa(tau)[None, :, None]
        m, V = ctx.post_mean().reshape(R8, p, T), ctx.post_vsmgp()
        m_scale = float(np.max(np.abs(m)))
        s_values = S_VALUES + ((sblk_of(T) + 17,) if shape == (20, 1, 21) else ())      # one tile and one time into the second time block
        for S in s_values:
            s, far = make_times(T, S, tau, 0)
            got = ctx.posterior_velocity_at(s, want=ALL)
            assert all(got[k].shape == (R8, p, S) for k in ALL)
            e = worst([errors({k: got[k][r] for k in ALL}, numpy_velocity(tau, m[r], V[r], s), tau, m_scale) for r in range(R8)])
            e_far = max(float(np.max(np.abs(got['vel'][:, :, far]), initial=0.0)), float(np.max(np.abs(got['cross'][:, :, far]), initial=0.0)),
                        float(np.max(np.abs(got['var'][:, :, far] - 1.0), initial=0.0)), float(np.max(np.abs(got['vel_var'][:, :, far] / kap - 1.0), initial=0.0)))
            det = float(np.min((got['var'] * got['vel_var'] - got['cross'] ** 2) / kap))
            at = ctx.posterior_at(s)
            e_at = float(np.max(np.abs(got['var'] - at['var'])))
            print('q=%d p=%d T=%d %s S=%d: %s (limit %.0e); far field %.2e (limit %.0e); smallest var vel_var - cross^2 %.2e of kappa; var against '
                  'posterior_at %.2e, mean the same bits: %s' % (q, p, T, tag(config), S, fmt(e), TOL_SAME, e_far, TOL_FAR, det, e_at, np.array_equal(got['mean'], at['mean'])))
            assert max(e.values()) <= TOL_SAME and e_far <= TOL_FAR
            assert np.all(got['var'] >= 0.0) and np.all(got['vel_var'] >= 0.0) and det >= -1e-9
            assert np.array_equal(got['mean'], at['mean']) and e_at <= TOL_SAME
            # each output asked for alone: the same bits
            for k in ALL:
                alone = ctx.posterior_velocity_at(s, want=(k,))
                assert list(alone) == [k] and np.array_equal(alone[k], got[k]), k
    finally:
        ctx.close()


# ---- 2. the velocity against central differences of posterior_at means: independent of the derivative formula on the device --------------------------
@pytest.mark.parametrize('config', CONFIGS, ids=CONFIG_IDS)
@pytest.mark.parametrize('shape', [SHAPES[0], SHAPES[4]], ids=[IDS[0], IDS[4]])
def test_the_velocity_is_the_central_difference_of_posterior_at_means(shape, config):
    q, p, T = shape
    ctx, par, _, _ = make_ctx(shape, config)
    try:
        s = off_grid_times(T, 40, 23)
        vel = ctx.posterior_velocity_at(s, want=('vel',))['vel']
        up, dn = ctx.posterior_at(s + FD_H_MS, want=('mean',))['mean'], ctx.posterior_at(s - FD_H_MS, want=('mean',))['mean']
        fd = (up - dn) / (2.0 * FD_H_MS) * 1000.0
        err = float(np.max(np.abs(vel - fd)) / np.max(np.abs(vel)))
        print('q=%d p=%d T=%d %s: vel against central differences of posterior_at means at h = %.2f ms: %.2e of max|vel| (limit %.1e)'
              % (q, p, T, tag(config), FD_H_MS, err, FD_LIMIT_MEAN))
        assert err <= FD_LIMIT_MEAN
    finally:
        ctx.close()


# ---- 3. ragged trials and both observation tables ---------------------------------------------------------------------------------------------------
def own_grid_velocity(par, mode, live, L, s):
    """numpy_velocity on the trial's own L-bin dense posterior (likelihood terms at its live entries only) at the device's mode: the construction of
    own_grid_reference in test_gpu_posterior_at.py"""
    C, d = np.asarray(par['C']), np.asarray(par['d']).reshape(-1)
    p = C.shape[1]
    X = np.ascontiguousarray(mode[:, :L])
    e = np.exp(C @ X + d[:, None]) * live[:, :L]
    W = np.einsum('nk,nt,nl->tkl', C, e, C)
    Kinv = np.linalg.inv(orc.make_K(par['tau'], L, BIN_MS))
    H = np.zeros((p, L, p, L))
    ar = np.arange(L)
    for k in range(p):
        H[k, :, k, :] += Kinv[k]
        for l in range(p):
            H[k, ar, l, ar] += W[:, k, l]
    V, _ = orc.marginal_blocks(np.linalg.inv(H.reshape(p * L, p * L)), p, L)
    return numpy_velocity(par['tau'], X, V, s)


@pytest.mark.parametrize('config', CONFIGS, ids=CONFIG_IDS)
@pytest.mark.parametrize('shape', SHAPES[:2], ids=IDS[:2])
def test_ragged_trials_under_both_observation_tables_use_their_own_posterior(shape, config):
    q, p, T = shape
    lens = np.array([T, T - 1, 17, 16, T, 40, T - 7, 33], dtype=np.int32)
    rng = np.random.default_rng(7)
    observed = np.ones((R8, q), dtype=np.uint8)
    observed[1, :5] = 0
    observed[2, q - 4:] = 0
    observed[6, 3::4] = 0
    bins = (rng.random((R8, q, T)) > 0.15).astype(np.uint8)
    bins[0] = 1
    ctx, par, _, live = make_ctx(shape, config, lens=lens, observed=observed, bins=bins)
    try:
        m = ctx.post_mean().reshape(R8, p, T)
        s, _ = make_times(T, 65, par['tau'], 2)
        trials = np.array([0, 1, 2, 3, 6], dtype=np.int32)
        # on top: query times inside [T_r bin, T bin) of the short trials and grid times at padded bins
        s = np.concatenate([s, [16.5 * BIN_MS, 17.0 * BIN_MS, 20.0 * BIN_MS, (T - 1.5) * BIN_MS, (T - 1.0) * BIN_MS, 0.5 * (17 + T) * BIN_MS]])
        got = ctx.posterior_velocity_at(s, trials, want=ALL)
        for i, r in enumerate(trials):
            ref = own_grid_velocity(par, m[r], live[r], int(lens[r]), s)
            e = errors({k: got[k][i] for k in ALL}, ref, par['tau'], float(np.max(np.abs(m[r]))))
            print('q=%d p=%d T=%d %s trial %d (%d bins): own-grid posterior, %s (limit %.0e)' % (q, p, T, tag(config), r, lens[r], fmt(e), TOL_DENSE))
            assert max(e.values()) <= TOL_DENSE
    finally:
        ctx.close()


# ---- 4. variational posteriors ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('engine', [1, 2], ids=['dense', 'lowrank'])
@pytest.mark.parametrize('which', ['var_toy', 'q40-p10-T64'])
def test_variational_posterior_against_the_oracle_at_the_kept_lambda(which, engine):
    from funs import _hip
    par, Y, binSize = _var_problem(which)
    assert binSize == BIN_MS
    R, q, T = Y.shape
    p = par['C'].shape[1]
    C_big, _ = orc.make_Cd_big(par['C'], par['d'], T)
    K_big = orc.make_K_big(orc.make_K(par['tau'], T, binSize))
    Kinv_big = np.linalg.inv(K_big)
    ctx = _hip.Context(q, p, T, R, binSize)
    try:
        ctx.upload_counts(Y.astype(np.uint16 if Y.max() > 255 else np.uint8))
        ctx.set_option('cov_mode', engine)
        ctx.set_option('dual_lowrank', int(engine == 2))
        ctx.set_params(par['C'], par['d'], par['tau'])
        _, _, _, status, lam = ctx.dual_fixed_point(None, None, want_lam=True)
        assert np.all(status == 0), status
        ctx.dual_finalize(None, None)
        s, _ = make_times(T, 65, par['tau'], 4)
        got = ctx.posterior_velocity_at(s, want=ALL)
        for r in range(R):
            Sigma, _ = orc.vi_post_cov(Kinv_big, C_big, lam[r])
            mean = orc.vi_post_mean(K_big, C_big, Y[r].reshape(-1).astype(np.float64), lam[r]).reshape(p, T)
            V, _ = orc.marginal_blocks(Sigma, p, T)
            e = errors({k: got[k][r] for k in ALL}, numpy_velocity(par['tau'], mean, V, s), par['tau'], float(np.max(np.abs(mean))))
            print('%s engine %d trial %d: VIPostMean / VIPostCov at the kept lambda, %s (limit %.0e)' % (which, engine, r, fmt(e), TOL_DENSE))
            assert max(e.values()) <= TOL_DENSE
    finally:
        ctx.close()


def test_a_variational_posterior_of_a_short_trial_is_refused():
    from funs import _hip
    shape = (20, 3, 40)
    q, p, T = shape
    par, Y, _ = problem(shape, R=3)
    lens = np.array([T, 23, T], dtype=np.int32)
    Y = Y * (np.arange(T)[None, None, :] < lens[:, None, None])
    ctx = _hip.Context(q, p, T, 3, BIN_MS)
    try:
        ctx.upload_counts(Y.astype(np.uint8))
        ctx.set_trial_lengths(lens)
        ctx.set_option('dual_masked', 1)
        ctx.set_params(par['C'], par['d'], par['tau'])
        _, _, _, status = ctx.dual_fixed_point(None, None)
        assert np.all(status == 0), status
        ctx.dual_finalize(None, None)
        with pytest.raises(_hip.HipBackendError, match='variational posterior of trial 1 covers 23 of 40 bins.*pgpfa_posterior_velocity_at refuses'):
            ctx.posterior_velocity_at(np.zeros(3))
        assert ctx.posterior_velocity_at(np.zeros(3), np.array([0, 2], dtype=np.int32))['vel'].shape == (2, p, 3)      # the full-length ones are served
    finally:
        ctx.close()


# ---- 5. an uploaded posterior -----------------------------------------------------------------------------------------------------------------------
def test_an_uploaded_posterior_is_evaluated_under_the_current_parameters():
    from funs import _hip
    q, p, T, R = 9, 4, 37, 3
    rng = np.random.default_rng(11)
    tau = np.array([0.05, 0.08, 0.11, 0.2])
    K = orc.make_K(tau, T, BIN_MS)
    m = np.stack([np.stack([np.linalg.cholesky(K[k]) @ rng.standard_normal(T) for k in range(p)]) for _ in range(R)])
    V = np.empty((R, T, T, p))
    for r in range(R):
        for k in range(p):
            V[r, :, :, k] = np.linalg.inv(np.linalg.inv(K[k]) + np.diag(rng.uniform(0.1, 2.0, T)))
    vsm = np.zeros((R, T, p, p))
    for k in range(p):
        vsm[:, :, k, k] = np.diagonal(V[:, :, :, k], axis1=1, axis2=2)
    ctx = _hip.Context(q, p, T, R, BIN_MS)
    try:
        ctx.set_params(rng.standard_normal((q, p)), np.zeros(q), tau)
        with pytest.raises(_hip.HipBackendError, match='no posterior for trial 0'):
            ctx.posterior_velocity_at(np.zeros(3))
        ctx.set_posterior(None, m, vsm, V)
        s, _ = make_times(T, 65, tau, 5)
        for scale_tau in (1.0, 1.4):                                  # ... whatever they are when the call is made
            ctx.set_params(rng.standard_normal((q, p)), np.zeros(q), tau * scale_tau)
            got = ctx.posterior_velocity_at(s, np.array([2, 0], dtype=np.int32), want=ALL)
            for i, r in enumerate((2, 0)):
                e = errors({k: got[k][i] for k in ALL}, numpy_velocity(tau * scale_tau, m[r], V[r], s), tau * scale_tau, float(np.max(np.abs(m[r]))))
                print('uploaded posterior, tau x %.1f, trial %d: %s (limit %.0e)' % (scale_tau, r, fmt(e), TOL_SAME))
                assert max(e.values()) <= TOL_SAME
    finally:
        ctx.close()


# ---- 6. bits do not depend on the call ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('config', CONFIGS, ids=CONFIG_IDS)
@pytest.mark.parametrize('shape', [SHAPES[0], SHAPES[5]], ids=[IDS[0], IDS[5]])
def test_per_trial_grids_lists_and_chunks_give_the_same_bits(shape, config):
    q, p, T = shape
    ctx, par, _, _ = make_ctx(shape, config)
    try:
        S = 65
        grids = np.stack([make_times(T, S, par['tau'], 10 + r)[0] for r in range(R8)])
        per = ctx.posterior_velocity_at(grids, want=ALL)
        # one grid per trial against the same grid shared by the same list: the same bits per (trial, times)
        rows = [bool(all(np.array_equal(ctx.posterior_velocity_at(grids[r], want=ALL)[k][r], per[k][r]) for k in ALL)) for r in range(R8)]
        # ... and against a list of that trial alone.  mean and vel read no block.  var, vel_var and cross read post_vsmGP: the same bits where the
        # blocks are resident; under the sum-only plan every call rebuilds the blocks of ITS list (ensure_trial_vsmgp, as for pgpfa_posterior_at and
        # pgpfa_get_post_vsmgp), and the last bits of a rebuilt block follow the number of trials rebuilt together (test_gpu_posterior_at.py measures
        # 6.7e-16 in var for the same comparison), so there the inputs differ and the limit is the "same inputs" one
        kap = kappa(par['tau'])[:, None]
        worst_alone = dict.fromkeys(ALL, 0.0)
        for r in range(R8):
            one = ctx.posterior_velocity_at(grids[r], np.array([r], dtype=np.int32), want=ALL)
            for k, scale in (('mean', 1.0), ('var', 1.0), ('vel', 1.0), ('vel_var', kap), ('cross', np.sqrt(kap))):
                worst_alone[k] = max(worst_alone[k], float(np.max(np.abs(one[k][0] - per[k][r]) / scale)))
        print('q=%d p=%d T=%d %s: (n, S) call against the shared grid over the same list, same bits %s; against a list of the trial alone, largest '
              'difference %s' % (q, p, T, tag(config), rows, fmt(worst_alone)))
        assert all(rows)
        assert worst_alone['mean'] == 0.0 and worst_alone['vel'] == 0.0
        assert all(worst_alone[k] <= (0.0 if config[1] else TOL_SAME) for k in ('var', 'vel_var', 'cross'))
        shared = ctx.posterior_velocity_at(grids[0], want=ALL)
        order = np.array([6, 2, 2, 7, 0, 5, 1, 3, 4, 2], dtype=np.int32)     # permuted, trial 2 three times
        seen = []
        for chunk in (1, 3, 0):
            ctx.set_option('velat_chunk_trials', chunk)
            a = ctx.posterior_velocity_at(grids, want=ALL)
            b = ctx.posterior_velocity_at(grids[order], order, want=ALL)
            c = ctx.posterior_velocity_at(grids[0], order, want=ALL)
            seen.append((chunk, same_bits(a, per), all(np.array_equal(b[k], per[k][order]) for k in ALL), all(np.array_equal(c[k], shared[k][order]) for k in ALL)))
        print('q=%d p=%d T=%d %s: (velat_chunk_trials, all trials, permuted list with repeats, shared grid) %s' % (q, p, T, tag(config), seen))
        assert all(x[1] and x[2] and x[3] for x in seen)
    finally:
        ctx.close()


@pytest.mark.parametrize('config', CONFIGS, ids=CONFIG_IDS)
def test_a_list_across_two_parameter_snapshots_gives_the_bits_of_one_call_per_trial(config):
    """four trials, {0, 1} through an E-step at parameters A and {2, 3} through one at B (C, d and every timescale differ): one call over
    [3, 0, 2, 1, 0] walks two snapshot groups and scatters by list position (the construction of test_gpu_posterior_at.py)"""
    from funs import _hip
    shape = SHAPES[4]
    q, p, T = shape
    par, Y, _ = problem(shape, R=4)
    mixed = np.array([3, 0, 2, 1, 0], dtype=np.int32)
    s = np.array([0.0, 3.7, 10.0, T - 1.0, T + 2.5]) * BIN_MS
    ctx = _hip.Context(q, p, T, 4, BIN_MS)
    try:
        ctx.upload_counts(Y.astype(np.uint16 if Y.max() > 255 else np.uint8))
        ctx.set_option('cov_mode', config[0])
        ctx.set_option('keep_trial_vsmgp', config[1])
        ctx.set_params(par['C'], par['d'], par['tau'])
        _, _, status = ctx.estep_laplace(np.array([0, 1], dtype=np.int32))
        assert np.all(status == 0), status
        tau_b = par['tau'] * np.linspace(0.85, 0.95, p)
        ctx.set_params(par['C'] * 1.05 + 0.01, par['d'] + 0.1, tau_b)
        _, _, status = ctx.estep_laplace(np.array([2, 3], dtype=np.int32))
        assert np.all(status == 0), status
        before = [ctx.post_mean(), ctx.post_vsm(), ctx.gram()]
        one = ctx.posterior_velocity_at(s, mixed, want=ALL)
        after = [ctx.post_mean(), ctx.post_vsm(), ctx.gram()]
        same = [bool(same_bits(ctx.posterior_velocity_at(s, mixed[i:i + 1], want=ALL), {k: one[k][i:i + 1] for k in ALL})) for i in range(mixed.size)]
        kept = [bool(np.array_equal(a, b)) for a, b in zip(before, after)]
        # each group under its own timescales: far away vel_var is the kappa of the trial's own E-step
        far = ctx.posterior_velocity_at(np.array([-1.0e6]), mixed, want=('vel_var',))['vel_var'][:, :, 0]
        e_far = max(float(np.max(np.abs(far[i] / kappa(tau_b if mixed[i] >= 2 else par['tau']) - 1.0))) for i in range(mixed.size))
        print('%s: list %s against one call per entry %s; post_mean, post_vsm, Gram unchanged %s; far-field vel_var against the own kappa %.2e'
              % (tag(config), mixed.tolist(), same, kept, e_far))
        assert all(same) and all(kept) and e_far <= TOL_FAR
        assert same_bits({k: one[k][1] for k in ALL}, {k: one[k][4] for k in ALL})
    finally:
        ctx.close()


# ---- 7. no state is touched -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('config', CONFIGS, ids=CONFIG_IDS)
def test_no_state_is_touched(config):
    """Two contexts through the same E-step; one makes the call (twice), the other never does.  What follows is the same to the bit: posterior_at,
    post_mean, post_vsm, then the download of post_vsmGP - which under the sum-only plan rebuilds the blocks of the trials whose mark is not set and
    rewrites their post_vsm by another kernel, so post_vsm read AFTER it shows whether the call left a mark behind - and post_vsm again."""
    shape = SHAPES[0]
    q, p, T = shape
    s, _ = make_times(T, 65, np.array([0.15]), 3)
    pick = np.array([0, 3], dtype=np.int32)
    state = {}
    for call in (True, False):
        ctx, par, _, _ = make_ctx(shape, config)
        try:
            if call:
                at_before = ctx.posterior_at(s)
                first = ctx.posterior_velocity_at(s, want=ALL)
                again = ctx.posterior_velocity_at(s, want=ALL)
                assert same_bits(first, again)
                at_after = ctx.posterior_at(s)
                assert same_bits(at_before, at_after)
            at = ctx.posterior_at(s)
            state[call] = [at['mean'], at['var'], ctx.post_mean(), ctx.post_vsm(), ctx.post_vsmgp(pick), ctx.post_vsm(), ctx.gram()]
        finally:
            ctx.close()
    same = [bool(np.array_equal(a, b)) for a, b in zip(state[True], state[False])]
    print('%s: bit-identical to a context that never made the call (posterior_at mean / var, post_mean, post_vsm, post_vsmGP of two trials, post_vsm after '
          'that download, Gram): %s' % (tag(config), same))
    assert all(same)


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_names_what_is_wrong():
    from funs import _hip
    shape = (20, 3, 40)
    q, p, T = shape
    par, Y, _ = problem(shape, R=4)
    ctx = _hip.Context(q, p, T, 4, BIN_MS)
    try:
        ctx.upload_counts(Y.astype(np.uint8))
        with pytest.raises(_hip.HipBackendError, match='set_params has not been called'):
            ctx.posterior_velocity_at(np.zeros(3))
        ctx.set_params(par['C'], par['d'], par['tau'])
        with pytest.raises(_hip.HipBackendError, match='no posterior for trial 0'):
            ctx.posterior_velocity_at(np.zeros(3))
        ctx.estep_laplace(np.array([0, 1, 2], dtype=np.int32))
        with pytest.raises(_hip.HipBackendError, match='no posterior for trial 3'):
            ctx.posterior_velocity_at(np.zeros(3))
        idx = np.array([2, 0], dtype=np.int32)
        assert ctx.posterior_velocity_at(np.zeros(3), idx)['vel'].shape == (2, p, 3)
        with pytest.raises(_hip.HipBackendError, match='pgpfa_posterior_velocity_at: S = 0'):
            ctx.posterior_velocity_at(np.zeros(0), idx)
        t = np.zeros(3)
        assert ctx.lib.pgpfa_posterior_velocity_at(ctx.h, 2, _hip.iptr(idx), 3, _hip.dptr(t), 0, None, None, None, None, None) != 0
        assert 'no output asked for' in ctx.lib.pgpfa_last_error().decode()
        out = np.zeros((2, p, 3))
        assert ctx.lib.pgpfa_posterior_velocity_at(ctx.h, 2, _hip.iptr(idx), 3, None, 0, None, None, _hip.dptr(out), None, None) != 0
        assert 'times_ms is NULL' in ctx.lib.pgpfa_last_error().decode()
        with pytest.raises(_hip.HipBackendError, match='pgpfa_posterior_velocity_at: query time 1 is not finite'):
            ctx.posterior_velocity_at(np.array([0.0, np.nan, 1.0]), idx)
        grids = np.zeros((2, 3))
        grids[1, 2] = np.inf
        with pytest.raises(_hip.HipBackendError, match=r'query time 2 of list entry 1 \(trial 0\) is not finite'):
            ctx.posterior_velocity_at(grids, idx)
        with pytest.raises(ValueError, match='times must have shape'):
            ctx.posterior_velocity_at(np.zeros((3, 3)), idx)
        with pytest.raises(ValueError, match='unknown output'):
            ctx.posterior_velocity_at(np.zeros(3), idx, want=('vel', 'cov'))
        with pytest.raises(_hip.HipBackendError, match='velat_chunk_trials'):
            ctx.set_option('velat_chunk_trials', -1)
        # an asynchronous timescale pass in flight
        ctx.mstep_precomp()
        Q = np.log(1.0 / (par['tau'] * 100.0) ** 2)[None, :] + np.array([0.0, 0.1])[:, None]
        ctx.mstep_tau_costgrad_multi_begin(Q)
        with pytest.raises(_hip.HipBackendError, match='timescale pass is in flight'):
            ctx.posterior_velocity_at(np.zeros(3), idx)
        ctx.mstep_tau_costgrad_multi_end()
        assert ctx.posterior_velocity_at(np.zeros(3), idx, want=('cross',))['cross'].shape == (2, p, 3)
        # counts uploaded after the E-step: the posterior is gone
        ctx.upload_counts(Y.astype(np.uint8))
        with pytest.raises(_hip.HipBackendError, match='no posterior for trial 2'):
            ctx.posterior_velocity_at(np.zeros(3), idx)
    finally:
        ctx.close()


# ---- 9. the Python surface --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def funs_mod():
    import funs
    from funs import _session
    _session.drop_sessions()
    yield funs
    _session.drop_sessions()


def test_util_posterior_velocity_at_with_conditions_on_a_ragged_config1_experiment(funs_mod):
    util, inference = funs_mod.util, funs_mod.inference
    shape = SHAPES[0]
    q, p, T = shape
    par, Y, _ = problem(shape, R=R8)
    lens = np.array([T, T - 1, 17, 16, T, 40, T - 7, 33])
    exp = Experiment([Y[r][:, :lens[r]].astype(np.float64) for r in range(R8)], BIN_MS)
    params = {k: np.array(v, dtype=np.float64) for k, v in par.items()}
    infRes, _ = inference.laplace(exp, {k: v.copy() for k, v in params.items()}, returnOptimRes=False)
    s, _ = make_times(T, 65, par['tau'], 6)
    s = np.concatenate([s, [0.0, 150.0, 160.0, 160.0 + 1e-9, (T - 1) * BIN_MS]])
    cond = np.array([4, 9, 4, 9, 4, 4, 9, 9])
    keys = ('vel', 'var', 'lower', 'upper', 'value', 'value_var', 'cross', 'speed2')
    out = util.posteriorVelocityAt(params, exp, s, infRes=infRes, conditions=cond, level=0.9, want=keys)
    assert all(out[k].shape == (R8, p, s.size) for k in keys[:-1]) and out['speed2'].shape == (R8, s.size)
    assert np.array_equal(out['times'], s) and out['condition_labels'].tolist() == [4, 9]
    # the device planes against each trial's own-grid dense model
    live = np.ones((q, T))
    name = {'vel': 'vel', 'var': 'vel_var', 'value': 'mean', 'value_var': 'var', 'cross': 'cross'}
    for r in range(R8):
        mode = np.zeros((p, T))
        mode[:, :lens[r]] = np.asarray(infRes['post_mean'][r])[:, :lens[r]]
        ref = own_grid_velocity(par, mode, live, int(lens[r]), s)
        e = errors({name[k]: out[k][r] for k in name}, ref, par['tau'], float(np.max(np.abs(mode))))
        print('util.posteriorVelocityAt on ragged config 1, trial %d (%d bins): %s (limit %.0e)' % (r, lens[r], fmt(e), TOL_DENSE))
        assert max(e.values()) <= TOL_DENSE
    # the host arithmetic against numpy on the call's own device outputs: 1e-12 of the sums of absolute terms
    z = util._band_z(0.9)
    sd = np.sqrt(out['var'])
    e_band = max(float(np.max(np.abs(out['lower'] - (out['vel'] - z * sd)) / (np.abs(out['vel']) + z * sd))),
                 float(np.max(np.abs(out['upper'] - (out['vel'] + z * sd)) / (np.abs(out['vel']) + z * sd))))
    terms = out['vel'] ** 2 + out['var']
    e_speed = float(np.max(np.abs(out['speed2'] - terms.sum(axis=1)) / terms.sum(axis=1)))
    inside = (s[None, :] >= 0.0) & (s[None, :] <= ((lens - 1) * BIN_MS)[:, None])
    e_cond = 0.0
    for g, label in enumerate((4, 9)):
        members = np.flatnonzero(cond == label)
        count = inside[members].sum(axis=0)
        assert np.array_equal(out['condition_count'][g], count)
        total = (out['vel'][members] * inside[members][:, None, :]).sum(axis=0)
        absum = (np.abs(out['vel'][members]) * inside[members][:, None, :]).sum(axis=0)
        want = np.where(count[None, :] > 0, total / np.maximum(count, 1)[None, :], 0.0)
        e_cond = max(e_cond, float(np.max(np.abs(out['condition_mean'][g] - want) / np.maximum(absum / np.maximum(count, 1)[None, :], 1e-300))))
        assert np.all(out['condition_mean'][g][:, count == 0] == 0.0)
    print('band %.2e, speed2 %.2e, condition means %.2e of the sums of absolute terms (limit 1e-12)' % (e_band, e_speed, e_cond))
    assert e_band <= 1e-12 and e_speed <= 1e-12 and e_cond <= 1e-12
    assert out['condition_count'][:, list(s).index(160.0)].tolist() == [4, 3] and out['condition_count'][:, list(s).index(160.0 + 1e-9)].tolist() == [3, 3]


def test_fit_posterior_velocity_at_after_a_two_iteration_fit(funs_mod):
    shape = SHAPES[0]
    q, p, T = shape
    par, Y, _ = problem(shape, R=R8)
    exp = Experiment([Y[r].astype(np.float64) for r in range(R8)], BIN_MS)
    init = {k: np.array(v, dtype=np.float64) for k, v in par.items()}
    fit = funs_mod.engine.PPGPFAfit(exp, initParams=init, EMmode='Batch', maxEMiter=2, CdOptimMethod='newton', quiet=True)
    fine = np.arange(0.0, (T - 2) * BIN_MS + 1e-9, BIN_MS / 4.0) + 1.0          # off the grid, inside every trial's span
    out = fit.posteriorVelocityAt(times=fine, conditions=np.arange(R8) % 2, want=('vel', 'lower', 'upper', 'value', 'speed2'))
    assert fit.velocitiesAt is out and out['vel'].shape == (R8, p, fine.size) and out['condition_mean'].shape == (2, p, fine.size)
    assert np.all(out['lower'] <= out['vel']) and np.all(out['vel'] <= out['upper']) and np.all(out['speed2'] >= (out['vel'] ** 2).sum(axis=1))
    assert np.array_equal(out['condition_count'], np.full((2, fine.size), R8 // 2))
    # the velocity is the slope of the value the same call returns, at the fitted timescales: central differences over the 2.5 ms spacing
    # (error about (h / l)^2 / 6 with l >= 60 ms at the start of the fit: well under 1e-2)
    slope = (out['value'][:, :, 2:] - out['value'][:, :, :-2]) / (2.0 * BIN_MS / 4.0) * 1000.0
    err = float(np.max(np.abs(slope - out['vel'][:, :, 1:-1])) / np.max(np.abs(out['vel'])))
    print('PPGPFAfit.posteriorVelocityAt: vel against the slope of value over 2.5 ms %.2e of max|vel| (limit 1e-2)' % err)
    assert err <= 1e-2
    for g in range(2):
        assert np.allclose(out['condition_mean'][g], out['vel'][g::2].mean(axis=0), rtol=1e-12, atol=1e-15)
