"""Joint posterior samples and posterior-predictive counts (pgpfa_posterior_sample, Context.posterior_sample):

    x = m + M z,  M M^T = Sigma,  y ~ Poisson(exp(d + C x))

with M = [sqrt(eps) chol(G) | G F L^-T] under the low-rank covariance engine and M = L^-T under the dense one.  R = 3 trials, the list [2, 0], four
shapes on the seams of the kernels, both engines.  Feeding the identity as noise returns M itself, so M M^T is compared with the numpy inverse of the
oracle's Hessian at the device's mode at the project's 1e-8; the statistical tests use sampling-theory bounds at 6 standard
errors under a fixed seed.  Every test prints its figures before it asserts; the yardstick functions come from test_cpu_posterior_samples.py."""
import ctypes as ct

import numpy as np
import pytest

from conftest import load_golden
from oracle import pgpfa_oracle as orc
from test_cpu_posterior_samples import BIN_MS, SHAPES, problem

pytestmark = pytest.mark.gpu

IDS = ['q%d-p%d-T%d' % s for s in SHAPES]
ENGINES = [1, 2]
ENGINE_IDS = ['dense', 'lowrank']
LIST = np.array([2, 0], dtype=np.int32)
RAGGED = {SHAPES[0]: (24, 17, 9), SHAPES[1]: (40, 33, 16)}
COV_TOL = 1e-8            # post_cov against the oracle: DESIGN.md section 2, docs/history/unequal_trials.md
S_STAT = 4096


def make_ctx(shape, engine, lens=None, d_offset=-1.0, evidence=False):
    """context of the 3-trial problem after one Laplace E-step under the given engine"""
    from funs import _hip
    q, p, T = shape
    par, Y, _ = problem(shape, d_offset=d_offset)
    if lens is not None:
        Y = Y * (np.arange(T)[None, None, :] < np.asarray(lens)[:, None, None])
    ctx = _hip.Context(q, p, T, 3, BIN_MS)
    ctx.upload_counts(Y.astype(np.uint16 if Y.max() > 255 else np.uint8))
    ctx.set_option('cov_mode', engine)
    if evidence:
        ctx.set_option('laplace_evidence', 1)
    ctx.set_params(par['C'], par['d'], par['tau'])
    if lens is not None:
        ctx.set_trial_lengths(np.asarray(lens, dtype=np.int32))
    _, _, status = ctx.estep_laplace()
    assert np.all(status == 0), status
    assert ctx.info('plan_lowrank') == float(engine == 2)
    nz = int(ctx.info('sample_noise_dim'))
    assert nz == p * T + (int(ctx.info('lowrank_rtot')) if engine == 2 else 0)
    return ctx, par, Y


def oracle_cov(par, mode, length):
    """numpy inverse of the oracle's Hessian at `mode` cut to `length` bins: the recipe of orc.laplace_cov_at, whole matrix"""
    C, d = np.asarray(par['C'], dtype=np.float64), np.asarray(par['d'], dtype=np.float64).reshape(-1)
    Kinv = np.linalg.inv(orc.make_K(par['tau'], length, BIN_MS))
    return np.linalg.inv(orc.nlp_hess(np.ascontiguousarray(mode[:, :length]), None, C, d, Kinv))


def roots(ctx, idx):
    """M of every listed trial ([p T] x nz) by feeding the nz x nz identity as noise, and nz"""
    nz = int(ctx.info('sample_noise_dim'))
    noise = np.ascontiguousarray(np.broadcast_to(np.eye(nz), (len(idx), nz, nz)))
    X = ctx.posterior_sample(idx, n_samples=nz, noise=noise)['x']
    m = ctx.post_mean()
    return [(X[i].reshape(nz, -1) - m[t].reshape(1, -1)).T for i, t in enumerate(idx)], nz


# ---- 1. exact square root --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('engine', ENGINES, ids=ENGINE_IDS)
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_identity_noise_returns_a_square_root_of_the_oracle_covariance(shape, engine):
    q, p, T = shape
    ctx, par, _ = make_ctx(shape, engine)
    try:
        Ms, nz = roots(ctx, LIST)
        m = ctx.post_mean()
        for M, t in zip(Ms, LIST):
            Sigma = oracle_cov(par, m[t], T)
            err = float(np.max(np.abs(M @ M.T - Sigma)) / np.max(np.abs(Sigma)))
            print('q=%d p=%d T=%d engine %d trial %d: nz = %d, max|M M^T - Sigma| = %.2e of max|Sigma| (limit %.0e)' % (q, p, T, engine, t, nz, err, COV_TOL))
            assert err <= COV_TOL
        zero = ctx.posterior_sample(LIST, n_samples=2, noise=np.zeros((2, 2, nz)))['x']
        assert np.array_equal(zero[0][0], m[2]) and np.array_equal(zero[0][1], m[2]) and np.array_equal(zero[1][1], m[0])
    finally:
        ctx.close()


# ---- 2. ragged trials ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('engine', ENGINES, ids=ENGINE_IDS)
@pytest.mark.parametrize('shape', [SHAPES[0], SHAPES[1]], ids=IDS[:2])
def test_ragged_trials_sample_the_truncated_model_and_stop_their_counts(shape, engine):
    q, p, T = shape
    lens = RAGGED[shape]
    ctx, par, _ = make_ctx(shape, engine, lens=lens)
    try:
        Ms, nz = roots(ctx, LIST)
        m = ctx.post_mean()
        for M, t in zip(Ms, LIST):
            L = lens[t]
            S = (M @ M.T).reshape(p, T, p, T)[:, :L][:, :, :, :L].reshape(p * L, p * L)
            Sigma = oracle_cov(par, m[t], L)
            err = float(np.max(np.abs(S - Sigma)) / np.max(np.abs(Sigma)))
            print('q=%d p=%d T=%d engine %d trial %d (%d of %d bins): first T_r bins %.2e of max|Sigma| (limit %.0e)' % (q, p, T, engine, t, L, T, err, COV_TOL))
            assert err <= COV_TOL
        out = ctx.posterior_sample(LIST, n_samples=5, seed=3, want=('y', 'count_sum'))
        for i, t in enumerate(LIST):
            assert not out['y'][i][:, :, lens[t]:].any()
            assert out['y'][i][:, :, :lens[t]].any()
        assert np.array_equal(out['count_sum'], out['y'].sum(axis=-1, dtype=np.int64))
    finally:
        ctx.close()


# ---- 3. variational posterior ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('engine', ENGINES, ids=ENGINE_IDS)
def test_variational_posterior_is_sampled_with_the_reference_jitter(engine):
    from funs import _hip
    g = load_golden('var_toy.npz')
    Y = g['Y'][:3]
    R, q, T = Y.shape
    par = {'C': g['init_C'], 'd': g['init_d'], 'tau': g['init_tau']}
    p = par['C'].shape[1]
    binSize = float(g['binSize'])
    C_big, _ = orc.make_Cd_big(par['C'], par['d'], T)
    Kinv_big = np.linalg.inv(orc.make_K_big(orc.make_K(par['tau'], T, binSize)))
    ctx = _hip.Context(q, p, T, R, binSize)
    try:
        ctx.upload_counts(Y)
        ctx.set_option('cov_mode', engine)
        ctx.set_option('dual_lowrank', int(engine == 2))
        ctx.set_params(par['C'], par['d'], par['tau'])
        _, _, _, status, lam = ctx.dual_fixed_point(None, None, want_lam=True)
        assert np.all(status == 0), status
        ctx.dual_finalize(None, None)
        Ms, nz = roots(ctx, LIST)
        for M, t in zip(Ms, LIST):
            dev = ctx.post_cov(int(t))
            ref, _ = orc.vi_post_cov(Kinv_big, C_big, lam[t])
            e_dev = float(np.max(np.abs(M @ M.T - dev)) / np.max(np.abs(dev)))
            e_ref = float(np.max(np.abs(M @ M.T - ref)) / np.max(np.abs(ref)))
            print('variational, engine %d trial %d: nz = %d, M M^T against post_cov %.2e, against orc.vi_post_cov %.2e (limit %.0e)' % (engine, t, nz, e_dev, e_ref, COV_TOL))
            assert e_dev <= COV_TOL and e_ref <= COV_TOL
    finally:
        ctx.close()


# ---- 4. device noise is the same map -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('engine', ENGINES, ids=ENGINE_IDS)
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_device_noise_is_a_pure_function_of_seed_trial_and_sample(shape, engine):
    ctx, par, _ = make_ctx(shape, engine)
    try:
        a = ctx.posterior_sample(LIST, n_samples=32, seed=7, want=('x', 'noise', 'y', 'count_sum'))
        again = ctx.posterior_sample(LIST, n_samples=32, noise=a['noise'], want=('x',))
        assert np.array_equal(again['x'], a['x'])                                       # the drawn normals fed back: the same linear map
        short = ctx.posterior_sample(LIST, n_samples=8, seed=7, want=('x', 'noise', 'y', 'count_sum'))
        for k in ('x', 'noise', 'y', 'count_sum'):
            assert np.array_equal(short[k], a[k][:, :8]), k                             # sample s does not know how many were asked for
        same = ctx.posterior_sample(LIST, n_samples=32, seed=7, want=('x', 'y'))
        assert np.array_equal(same['x'], a['x']) and np.array_equal(same['y'], a['y'])
        other = ctx.posterior_sample(LIST, n_samples=32, seed=8, want=('x', 'y'))
        assert not np.array_equal(other['x'], a['x']) and not np.array_equal(other['y'], a['y'])
        ctx.set_option('sample_chunk_trials', 1)
        chunked = ctx.posterior_sample(LIST, n_samples=32, seed=7, want=('x', 'noise', 'y', 'count_sum'))
        ctx.set_option('sample_chunk_trials', 0)
        for k in ('x', 'noise', 'y', 'count_sum'):
            assert np.array_equal(chunked[k], a[k]), k
        wide = ctx.posterior_sample(np.array([0, 1, 2, 0], dtype=np.int32), n_samples=32, seed=7, want=('x', 'y'))
        for k in ('x', 'y'):                                                            # whatever else is listed, and wherever the trial stands
            assert np.array_equal(wide[k][0], a[k][1]) and np.array_equal(wide[k][3], a[k][1]) and np.array_equal(wide[k][2], a[k][0]), k
        assert not np.array_equal(a['x'][0], a['x'][1]) and not np.array_equal(a['noise'][0], a['noise'][1])
        assert not np.array_equal(a['noise'][0][0], a['noise'][0][1])
    finally:
        ctx.close()


# ---- 5, 6, 8. the normals are normal; the draws have the posterior's moments; the rates agree with posterior_rates ---------------------------------------
@pytest.mark.parametrize('engine', ENGINES, ids=ENGINE_IDS)
def test_moments_of_4096_draws(engine):
    shape = SHAPES[0]
    q, p, T = shape
    ctx, par, _ = make_ctx(shape, engine)
    try:
        S = S_STAT
        out = ctx.posterior_sample(LIST, n_samples=S, seed=20261, want=('x', 'noise'))
        z = out['noise']
        nz = z.shape[2]
        N = z.size
        mean, var, m4 = float(z.mean()), float(z.var()), float(np.mean(z ** 4))
        print('engine %d: %d normals, mean %.2e (limit %.2e), variance - 1 %.2e (limit %.2e), fourth moment - 3 %.2e (limit %.2e)'
              % (engine, N, mean, 6 / np.sqrt(N), var - 1, 6 * np.sqrt(2 / N), m4 - 3, 6 * np.sqrt(96 / N)))
        assert abs(mean) <= 6 / np.sqrt(N) and abs(var - 1) <= 6 * np.sqrt(2 / N) and abs(m4 - 3) <= 6 * np.sqrt(96 / N)
        for i in range(2):
            corr = np.corrcoef(z[i].T)
            off = float(np.max(np.abs(corr - np.diag(np.diag(corr)))))
            print('engine %d trial %d: largest off-diagonal correlation of the %d x %d matrix %.4f (limit %.4f)' % (engine, LIST[i], nz, nz, off, 6 / np.sqrt(S)))
            assert off <= 6 / np.sqrt(S)
        m = ctx.post_mean()
        C, d = par['C'], par['d']
        rates = ctx.posterior_rates(LIST, want=('eta', 'var'))
        for i, t in enumerate(LIST):
            Sigma = oracle_cov(par, m[t], T)
            x = out['x'][i].reshape(S, p * T)
            dg = np.diag(Sigma)
            z_mean = float(np.max(np.abs(x.mean(axis=0) - m[t].reshape(-1)) / np.sqrt(dg / S)))
            xc = x - m[t].reshape(1, -1)
            z_cov = float(np.max(np.abs(xc.T @ xc / S - Sigma) / np.sqrt((np.outer(dg, dg) + Sigma ** 2) / S)))
            print('engine %d trial %d: worst z-score of the %d sample means %.2f, of the %d covariance entries %.2f (limit 6)' % (engine, t, p * T, z_mean, (p * T) ** 2, z_cov))
            assert z_mean <= 6.0 and z_cov <= 6.0
            lam = np.exp(d[None, :, None] + np.einsum('nk,skt->snt', C, out['x'][i]))
            eta, v = rates['eta'][i], rates['var'][i]
            se = np.sqrt((np.exp(v) - 1.0) * np.exp(2.0 * eta + v) / S)
            z_rate = float(np.max(np.abs(lam.mean(axis=0) - np.exp(eta + 0.5 * v)) / se))
            print('engine %d trial %d: Monte-Carlo mean rate against exp(eta + var / 2), worst z-score over %d (neuron, bin) %.2f (limit 6)' % (engine, t, q * T, z_rate))
            assert z_rate <= 6.0
    finally:
        ctx.close()


# ---- 7. predictive counts ---------------------------------------------------------------------------------------------------------------------------------
def check_counts(tag, par, out):
    C, d = par['C'], par['d']
    lam = np.exp(d[None, None, :, None] + np.einsum('nk,iskt->isnt', C, out['x']))
    Y = out['y'].astype(np.float64)
    assert out['y'].dtype == np.uint16 and out['count_sum'].dtype == np.int32
    assert np.array_equal(out['count_sum'], out['y'].sum(axis=-1, dtype=np.int64))
    N = Y.size
    z_sum = float((Y - lam).sum() / np.sqrt(lam.sum()))
    disp = float(np.mean((Y - lam) ** 2 / lam))
    lim = 6 * np.sqrt((2 + np.mean(1 / lam)) / N)
    print('%s: %d counts, largest %d, mean rate %.3g; sum(Y - lam) / sqrt(sum lam) = %.2f (limit 6), dispersion - 1 = %.2e (limit %.2e)'
          % (tag, N, out['y'].max(), lam.mean(), z_sum, disp - 1, lim))
    assert abs(z_sum) <= 6.0 and abs(disp - 1) <= lim


@pytest.mark.parametrize('engine', ENGINES, ids=ENGINE_IDS)
@pytest.mark.parametrize('shape', [SHAPES[0], SHAPES[1]], ids=IDS[:2])
def test_predictive_counts_are_poisson_of_the_drawn_rates(shape, engine):
    ctx, par, _ = make_ctx(shape, engine)
    try:
        out = ctx.posterior_sample(LIST, n_samples=256, seed=5, want=('x', 'y', 'count_sum'))
        check_counts('q=%d p=%d T=%d engine %d' % (shape + (engine,)), par, out)
        only = ctx.posterior_sample(LIST, n_samples=256, seed=5, want=('count_sum',))            # no [q][T] plane is written
        assert sorted(only) == ['count_sum'] and np.array_equal(only['count_sum'], out['count_sum'])
    finally:
        ctx.close()


def test_counts_above_255_come_back_in_uint16():
    """d raised to log 400: rates of several hundred per bin, the sampler's transformed-rejection branch, two-byte counts"""
    ctx, par, Y = make_ctx(SHAPES[0], 2, d_offset=float(np.log(400.0)))
    try:
        assert Y.max() > 255
        out = ctx.posterior_sample(LIST, n_samples=256, seed=9, want=('x', 'y', 'count_sum'))
        assert out['y'].max() > 255
        check_counts('d = log 400', par, out)
    finally:
        ctx.close()


def test_a_count_above_65535_fails_naming_the_trial():
    """a variational posterior at a fixed lambda under offsets of 12.5: rates of 2.7e5 exp(C x) do not fit the output"""
    from funs import _hip
    q, p, T = SHAPES[0]
    par, Y, _ = problem(SHAPES[0])
    ctx = _hip.Context(q, p, T, 3, BIN_MS)
    try:
        ctx.upload_counts(Y.astype(np.uint8))
        ctx.set_params(par['C'], np.full(q, 12.5), par['tau'])
        ctx.dual_finalize(LIST, np.full((2, q * T), 0.5))
        with pytest.raises(_hip.HipBackendError, match=r'trial (2|0) exceeds 65535'):
            ctx.posterior_sample(LIST, n_samples=4, want=('y',))
        x = ctx.posterior_sample(LIST, n_samples=4, want=('x',))['x']                           # the trajectories themselves are fine
        assert np.all(np.isfinite(x))
    finally:
        ctx.close()


# ---- 9. nothing else moved ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('engine', ENGINES, ids=ENGINE_IDS)
def test_sampling_leaves_the_resident_state_alone(engine):
    shape = SHAPES[0]
    q, p, T = shape
    ctx, par, _ = make_ctx(shape, engine, evidence=True)
    try:
        before_move = ctx.posterior_sample(LIST, n_samples=16, seed=1, want=('x', 'y'))
        ctx.mstep_precomp()
        # an M-step has moved the parameters on: the draws must still be those of the E-step's own parameters (the snapshot path; shorter
        # timescales, so that the low-rank system of the new parameters has at least the snapshot's rows and the noise can be handed out)
        C2, d2, tau2 = par['C'] * 1.05 + 0.01, par['d'] + 0.1, par['tau'] * 0.9
        ctx.set_params(C2, d2, tau2)
        v = orc.cd_to_vec(C2, d2)

        def state():
            cost, grad = ctx.mstep_cd_costgrad(v)
            return {'post_mean': ctx.post_mean(), 'post_vsm': ctx.post_vsm(), 'post_vsmgp': ctx.post_vsmgp(), 'pautosum': ctx.pautosum(),
                    'cd_cost': np.array(cost), 'cd_grad': grad, 'log_evidence': ctx.log_evidence()}
        ctx.post_vsmgp()                     # (under the sum-only plan the first request rebuilds the blocks: before the comparison, not inside it)
        s0 = state()
        nz_now = int(ctx.info('sample_noise_dim'))
        after_move = ctx.posterior_sample(LIST, n_samples=16, seed=1, want=('x', 'y', 'count_sum', 'noise'))
        s1 = state()
        for k in s0:
            assert np.array_equal(s0[k], s1[k]), k
        assert after_move['noise'].shape[2] == nz_now
        assert np.array_equal(after_move['x'], before_move['x']) and np.array_equal(after_move['y'], before_move['y'])
        par_now = {k: ctx.info(k) for k in ('plan_lowrank', 'lowrank_rtot')}
        print('engine %d: state bit-identical around a sampling call under a parameter snapshot (plan %s)' % (engine, par_now))
    finally:
        ctx.close()


@pytest.mark.parametrize('engine', ENGINES, ids=ENGINE_IDS)
def test_a_list_across_two_parameter_snapshots_gives_the_bits_of_one_call_per_trial(engine):
    """four trials, {0, 1} through an E-step at parameters A and {2, 3} through one at B (C, d and every timescale differ): one call over
    [3, 0, 2, 1, 0] walks two snapshot groups and scatters by list position"""
    from funs import _hip
    shape = SHAPES[0]
    q, p, T = shape
    par, Y, _ = problem(shape, R=4)
    mixed = np.array([3, 0, 2, 1, 0], dtype=np.int32)
    ctx = _hip.Context(q, p, T, 4, BIN_MS)
    try:
        ctx.upload_counts(Y.astype(np.uint16 if Y.max() > 255 else np.uint8))
        ctx.set_option('cov_mode', engine)
        ctx.set_params(par['C'], par['d'], par['tau'])
        _, _, status = ctx.estep_laplace(np.array([0, 1], dtype=np.int32))
        assert np.all(status == 0), status
        ctx.set_params(par['C'] * 1.05 + 0.01, par['d'] + 0.1, par['tau'] * np.linspace(0.85, 0.95, p))
        _, _, status = ctx.estep_laplace(np.array([2, 3], dtype=np.int32))
        assert np.all(status == 0), status
        assert ctx.info('plan_lowrank') == float(engine == 2)
        before = [ctx.post_mean(), ctx.post_vsm(), ctx.gram()]
        one = ctx.posterior_sample(mixed, n_samples=4, seed=11, want=('x',))['x']
        after = [ctx.post_mean(), ctx.post_vsm(), ctx.gram()]
        same = [bool(np.array_equal(one[i], ctx.posterior_sample(mixed[i:i + 1], n_samples=4, seed=11, want=('x',))['x'][0])) for i in range(mixed.size)]
        kept = [bool(np.array_equal(a, b)) for a, b in zip(before, after)]
        print('engine %d: list %s against one call per entry %s; post_mean, post_vsm, Gram unchanged %s' % (engine, mixed.tolist(), same, kept))
        assert all(same)
        assert np.array_equal(one[1], one[4])
        assert all(kept)
    finally:
        ctx.close()


# ---- 10. errors --------------------------------------------------------------------------------------------------------------------------------------------
def raw_call(ctx, n_samples=2, want_x=True, want_y=False, idx=LIST):
    """the C entry point without the binding's own checks -> (return code, message)"""
    from funs import _hip
    ii = np.ascontiguousarray(idx, dtype=np.int32)
    X = np.empty((len(ii), max(n_samples, 1), ctx.p, ctx.T))
    Y = np.empty((len(ii), max(n_samples, 1), ctx.q, ctx.T), dtype=np.uint16)
    rc = ctx.lib.pgpfa_posterior_sample(ctx.h, len(ii), _hip.iptr(ii), int(n_samples), ct.c_ulonglong(0), None, None, _hip.dptr(X) if want_x else None,
                                        Y.ctypes.data_as(ct.POINTER(ct.c_uint16)) if want_y else None, None)
    return rc, ctx.lib.pgpfa_last_error().decode()


def test_argument_errors_name_what_is_wrong():
    from funs import _hip
    shape = SHAPES[0]
    q, p, T = shape
    ctx, par, Y = make_ctx(shape, 2)
    try:
        rc, msg = raw_call(ctx, n_samples=0)
        assert rc != 0 and 'n_samples = 0' in msg
        rc, msg = raw_call(ctx, want_x=False)
        assert rc != 0 and 'no output asked for' in msg
        with pytest.raises(ValueError, match='n_samples'):
            ctx.posterior_sample(LIST, n_samples=0)
        with pytest.raises(ValueError, match='unknown output'):
            ctx.posterior_sample(LIST, want=('x', 'rate'))
        with pytest.raises(ValueError, match='noise must have shape'):
            ctx.posterior_sample(LIST, n_samples=2, noise=np.zeros((2, 2, 5)))
        # an uploaded posterior: only its blocks are known
        ctx.set_posterior(np.array([1], dtype=np.int32), ctx.post_mean([1]), ctx.post_vsm([1]))
        with pytest.raises(_hip.HipBackendError, match='no posterior to sample for trial 1'):
            ctx.posterior_sample(np.array([0, 1], dtype=np.int32))
        assert ctx.posterior_sample(LIST)['x'].shape == (2, 1, p, T)                             # the others still have theirs
        # new counts: no E-step since
        ctx.upload_counts(Y.astype(np.uint8))
        with pytest.raises(_hip.HipBackendError, match='no posterior to sample for trial 2'):
            ctx.posterior_sample(LIST)
    finally:
        ctx.close()
    fresh = _hip.Context(q, p, T, 3, BIN_MS)
    try:
        fresh.upload_counts(Y.astype(np.uint8))
        rc, msg = raw_call(fresh)
        assert rc != 0 and 'set_params has not been called' in msg
    finally:
        fresh.close()
    fresh = _hip.Context(q, p, T, 3, BIN_MS)
    try:
        fresh.set_params(par['C'], par['d'], par['tau'])
        rc, msg = raw_call(fresh, want_y=True)
        assert rc != 0 and 'spike counts have not been uploaded' in msg and 'length' in msg
    finally:
        fresh.close()
