"""Host side of the cross-latent covariance at arbitrary time points, without a GPU: header, binding and library agree on pgpfa_posterior_cov_at,
the unit is part of the build, the numpy restatement the GPU tests hold the device to

    Cov(x(s))[k][l] = a_k(s)^T Sigma_kl a_l(s) + delta_kl (1 - a_k(s) . kx_k(s)),   a_k(s) = K_k^-1 kx_k(s)

is itself checked - against the dense FP64 model extended by the query times as bins without a likelihood term, against the block diagonal of Sigma at
grid times and against the identity in the far field - and what util.posteriorRatesAt / util.posteriorAt(want=('cov',)) do around the device call.

The restatement's two evaluation orders (np.linalg.solve against an explicit inverse of K) differ by 5.5e-13 of the largest entry at most at the two
shapes below (printed by the test); ten times that stays below 1e-9, which is therefore the "same inputs" tolerance of test_gpu_posterior_cov_at.py,
as in test_gpu_posterior_at.py.  Every test prints its figures before it asserts."""
import ctypes as ct
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from oracle import pgpfa_oracle as orc
from test_cpu_posterior_at import _fake
from test_cpu_posterior_samples import curvature_blocks, dense_precision, problem

BIN_MS = 10.0
EPS = orc.EPS_NOISE
TOL_SAME, TOL_DENSE, TOL_FAR = 1e-9, 1e-8, 1e-12


# ---- the yardstick -------------------------------------------------------------------------------------------------------------------------------
def cross(tau_k, s, L):
    """kx (L, S) of one latent between the grid times j bin, j < L, and the query times s (as in test_gpu_posterior_at.py)"""
    tg = np.arange(L, dtype=np.float64) * BIN_MS
    dt = s[None, :] - tg[:, None]
    return (1.0 - EPS) * np.exp(-0.5 * ((dt * dt) / (tau_k * 1000.0) ** 2)) + EPS * (s[None, :] == tg[:, None])


def numpy_cov_at(tau, Sigma, s, explicit_inverse=False):
    """Cov(x(s)) (S, p, p) by the formula above from the p T x p T covariance Sigma (latent-major, the layout of post_cov)"""
    tau = np.asarray(tau, dtype=np.float64).reshape(-1)
    p = tau.size
    T = Sigma.shape[0] // p
    K = orc.make_K(tau, T, BIN_MS)
    kx = [cross(tau[k], s, T) for k in range(p)]
    a = [np.linalg.inv(K[k]) @ kx[k] if explicit_inverse else np.linalg.solve(K[k], kx[k]) for k in range(p)]
    cov = np.empty((s.size, p, p))
    for k in range(p):
        for l in range(p):
            cov[:, k, l] = ((Sigma[k * T:(k + 1) * T, l * T:(l + 1) * T] @ a[l]) * a[k]).sum(axis=0)
        cov[:, k, k] += 1.0 - (a[k] * kx[k]).sum(axis=0)
    return cov


def extended_blocks(tau, W, s, T):
    """The dense FP64 model over the grid AND the distinct off-grid query times (bins without a likelihood term), with the curvature blocks W (T, p, p)
    at the grid bins: the p x p blocks (S, p, p) of the inverse extended Hessian at the query times - the construction of augmented_reference in
    test_gpu_posterior_at.py, returning blocks instead of the diagonal.  A query time ON the grid reads the grid's own bin."""
    tau = np.asarray(tau, dtype=np.float64).reshape(-1)
    p = tau.size
    tg = np.arange(T) * BIN_MS
    on = np.isin(s, tg)
    extra = np.unique(s[~on])
    tt = np.concatenate([tg, extra])
    n = tt.size
    dt = tt[:, None] - tt[None, :]
    H = np.zeros((p, n, p, n))
    ar = np.arange(T)
    for k in range(p):
        H[k, :, k, :] += np.linalg.inv((1.0 - EPS) * np.exp(-0.5 * ((dt * dt) / (tau[k] * 1000.0) ** 2)) + EPS * np.eye(n))
        for l in range(p):
            H[k, ar, l, ar] += W[:, k, l]
    Sig = np.linalg.inv(H.reshape(p * n, p * n)).reshape(p, n, p, n)
    col = np.where(on, np.searchsorted(tg, s).clip(0, T - 1), T + np.searchsorted(extra, s).clip(0, max(extra.size - 1, 0)))
    return np.stack([Sig[:, c, :, c] for c in col])


def query_times(T, tau, seed):
    """off-grid draws over [-2 bin, (T + 1) bin], a few grid times, and two times 50 max(tau) beyond the ends; returns (times, positions of the far ones)"""
    rng = np.random.default_rng(seed)
    far = 50.0 * 1000.0 * float(np.max(tau))
    s = np.concatenate([rng.uniform(-2 * BIN_MS, (T + 1) * BIN_MS, 24), np.array([0.0, 7.0, T - 1.0]) * BIN_MS, [-far, (T - 1) * BIN_MS + far]])
    return s, np.array([s.size - 2, s.size - 1])


@pytest.fixture(scope='module')
def hip():
    import __graft_entry__ as ge
    ge.build()
    from funs import _hip
    return _hip


# ---- prototype -----------------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_the_new_entry_point(hip):
    lib = hip.load_library()
    header = open(os.path.join(ROOT, 'include', 'pgpfa.h')).read()
    bare = re.sub(r'/\*.*?\*/', ' ', header, flags=re.S)              # (the declaration without its comments)
    assert re.search(r'int\s+pgpfa_posterior_cov_at\s*\(\s*pgpfa_ctx\s*\*\s*ctx\s*,\s*int\s+n\s*,\s*const\s+int32_t\s*\*\s*idx\s*,\s*int\s+S\s*,\s*const\s+double\s*\*\s*'
                     r'times_ms\s*,\s*int\s+per_trial\s*,\s*double\s*\*\s*mean\s*,\s*double\s*\*\s*cov\s*,\s*double\s*\*\s*eta\s*,\s*double\s*\*\s*var\s*\)\s*;', bare)
    assert 'pgpfa_posterior_cov_at' in hip.EXPORTED_SYMBOLS and hasattr(lib, 'pgpfa_posterior_cov_at')
    c_double_p, c_int32_p = ct.POINTER(ct.c_double), ct.POINTER(ct.c_int32)
    assert list(lib.pgpfa_posterior_cov_at.argtypes) == [ct.c_void_p, ct.c_int, c_int32_p, ct.c_int, c_double_p, ct.c_int] + [c_double_p] * 4
    assert '"covat_chunk_trials"' in header and '"covat_block_times"' in header
    assert hasattr(hip.Context, 'posterior_cov_at')
    from funs import engine, util
    assert callable(util.posteriorRatesAt) and callable(engine.PPGPFAfit.posteriorRatesAt)


def test_the_unit_is_part_of_the_build():
    import __graft_entry__ as ge
    assert 'covat' in ge.UNITS
    assert os.path.exists(os.path.join(ge.CSRC, 'covat.hip')) and os.path.exists(os.path.join(ge.CSRC, 'covat.h'))


def test_null_context_is_refused_without_a_device(hip):
    lib = hip.load_library()
    t = np.zeros(1)
    out = np.zeros(1)
    assert lib.pgpfa_posterior_cov_at(None, 1, None, 1, hip.dptr(t), 0, hip.dptr(out), None, None, None) != 0
    assert 'null context' in lib.pgpfa_last_error().decode()


# ---- the restatement against independent constructions --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(30, 3, 100), (12, 2, 21)], ids=['q30-p3-T100', 'q12-p2-T21'])
def test_the_numpy_restatement_against_the_extended_model_the_grid_and_the_far_field(shape):
    q, p, T = shape
    par, _, X = problem(shape, R=1)
    W = curvature_blocks(X[0], par['C'], par['d'])
    Sigma = np.linalg.inv(dense_precision(W, par['tau'], T, BIN_MS))
    s, far = query_times(T, par['tau'], 5)
    near = np.setdiff1d(np.arange(s.size), far)
    cov = numpy_cov_at(par['tau'], Sigma, s)
    # its own error: the extended model
    ref = extended_blocks(par['tau'], W, s[near], T)
    e_ext = float(np.max(np.abs(cov[near] - ref)) / np.max(np.abs(ref)))
    # the spread of its two evaluation orders
    spread = float(np.max(np.abs(cov - numpy_cov_at(par['tau'], Sigma, s, explicit_inverse=True))) / np.max(np.abs(cov)))
    # grid times: the block diagonal of Sigma
    grid = numpy_cov_at(par['tau'], Sigma, np.arange(T) * BIN_MS)
    _, vsm = orc.marginal_blocks(Sigma, p, T)
    e_grid = float(np.max(np.abs(grid - vsm)) / np.max(np.abs(vsm)))
    e_far = float(np.max(np.abs(cov[far] - np.eye(p)[None])))
    e_sym = float(np.max(np.abs(cov - cov.transpose(0, 2, 1))))
    print('q=%d p=%d T=%d: restatement against the extended model %.2e relative (limit %.0e); solve against explicit inverse %.2e of the largest entry '
          '(ten times that against the same-inputs tolerance %.0e); grid blocks %.2e (limit %.0e); far field %.2e (limit %.0e); asymmetry %.2e'
          % (q, p, T, e_ext, TOL_DENSE, spread, TOL_SAME, e_grid, TOL_SAME, e_far, TOL_FAR, e_sym))
    assert e_ext <= TOL_DENSE
    assert 10.0 * spread <= TOL_SAME
    assert e_grid <= TOL_SAME
    assert e_far <= TOL_FAR
    assert e_sym <= 1e-12


# ---- util around a fake device -------------------------------------------------------------------------------------------------------------------
def _fake_cov(monkeypatch, lens, **kw):
    """the fake session of test_cpu_posterior_at.py whose context also answers posterior_cov_at in closed form: mean as its posterior_at,
    cov = (0.25 + (s / 1000)^2) I, eta = -1 + sum_k mean_k, var = p (0.25 + (s / 1000)^2)  (C = ones, d = -1 there)"""
    sess, exp, params, res, touched = _fake(monkeypatch, lens, **kw)
    ctx = sess.ctx
    ctx.cov_calls = []

    def posterior_cov_at(times, idx=None, want=('mean', 'cov')):
        tt = np.asarray(times, dtype=np.float64)
        ctx.cov_calls.append((tt.shape, tuple(want)))
        n, q = len(idx), sess.q
        s = np.broadcast_to(tt, (n, tt.shape[-1]))
        mean = (np.asarray(idx)[:, None, None] + 1.0) * (np.arange(ctx.p)[None, :, None] + 1.0) * s[:, None, :] / 100.0
        v = 0.25 + (s / 1000.0) ** 2
        made = {'mean': mean, 'cov': v[:, :, None, None] * np.eye(ctx.p)[None, None],
                'eta': np.broadcast_to(-1.0 + mean.sum(axis=1)[:, None, :], (n, q, s.shape[1])).copy(),
                'var': np.broadcast_to(ctx.p * v[:, None, :], (n, q, s.shape[1])).copy()}
        return {k: made[k] for k in want}
    ctx.posterior_cov_at = posterior_cov_at
    return sess, exp, params, res, touched


def test_posterior_rates_at_units_bands_and_condition_means(monkeypatch):
    from funs import util
    lens, bin_ms = [8, 3, 5, 8], 20.0
    sess, exp, params, res, _ = _fake_cov(monkeypatch, lens, bin_ms=bin_ms)
    times = np.array([0.0, 33.3, 40.0, 40.0 + 1e-9, 140.0])
    out = util.posteriorRatesAt(params, exp, times, infRes=res, conditions=[1, 1, 0, 0], level=0.9, want=('rate', 'lower', 'upper', 'median', 'eta', 'var'))
    assert sess.ctx.cov_calls[-1] == ((5,), ('eta', 'var')) and sess.ctx.calls == []
    assert out['rate'].shape == (4, 3, 5) and np.array_equal(out['times'], times) and out['condition_labels'].tolist() == [0, 1]
    z, per_s = util._band_z(0.9), 1000.0 / bin_ms
    assert np.array_equal(out['rate'], np.exp(out['eta'] + 0.5 * out['var']) * per_s) and np.array_equal(out['median'], np.exp(out['eta']) * per_s)
    assert np.array_equal(out['lower'], np.exp(out['eta'] - z * np.sqrt(out['var'])) * per_s)
    assert np.array_equal(out['upper'], np.exp(out['eta'] + z * np.sqrt(out['var'])) * per_s)
    span = (np.asarray(lens) - 1) * bin_ms
    inside = (times[None, :] >= 0.0) & (times[None, :] <= span[:, None])
    assert out['condition_count'].tolist() == [inside[[2, 3]].sum(axis=0).tolist(), inside[[0, 1]].sum(axis=0).tolist()]
    for g, members in ((0, [2, 3]), (1, [0, 1])):
        for j in range(times.size):
            who = [i for i in members if inside[i, j]]
            ref = sum(out['rate'][i][:, j] for i in who) / len(who) if who else np.zeros(3)
            assert np.allclose(out['condition_mean'][g][:, j], ref, rtol=1e-15, atol=0.0)
    # want=() with conditions: the averages alone; per-trial grids
    per = util.posteriorRatesAt(params, exp, np.tile(times, (4, 1)), infRes=res, conditions=[1, 1, 0, 0], want=())
    assert sorted(per) == ['condition_count', 'condition_labels', 'condition_mean', 'times'] and sess.ctx.cov_calls[-1] == ((4, 5), ('eta', 'var'))
    assert np.array_equal(per['condition_mean'], out['condition_mean'])


def test_posterior_rates_at_argument_checks_need_no_device(monkeypatch):
    from funs import util
    sess, exp, params, res, touched = _fake_cov(monkeypatch, [8, 8, 8])
    with pytest.raises(ValueError, match=r'times: entry \(2,\) is not finite'):
        util.posteriorRatesAt(params, exp, np.array([0.0, 1.0, np.nan]), infRes=res)
    grid = np.zeros((3, 4))
    grid[1, 3] = np.inf
    with pytest.raises(ValueError, match=r'times: entry \(1, 3\) is not finite'):
        util.posteriorRatesAt(params, exp, grid, infRes=res)
    with pytest.raises(ValueError, match='unknown key'):
        util.posteriorRatesAt(params, exp, np.zeros(2), infRes=res, want=('rate', 'ell'))
    for bad in (np.zeros((3, 2, 2)), np.zeros(0), np.zeros((3, 0)), 5.0):
        with pytest.raises(ValueError, match='times'):
            util.posteriorRatesAt(params, exp, bad, infRes=res)
    with pytest.raises(ValueError, match='nothing asked for'):
        util.posteriorRatesAt(params, exp, np.zeros(2), infRes=res, want=())
    with pytest.raises(ValueError, match='level'):
        util.posteriorRatesAt(params, exp, np.zeros(2), infRes=res, level=0.0)
    assert touched == []                                           # not even the session was looked up
    with pytest.raises(ValueError, match='times'):
        util.posteriorRatesAt(params, exp, np.zeros((2, 4)), infRes=res)                 # two grids for three listed trials
    with pytest.raises(ValueError, match='one label per listed trial'):
        util.posteriorRatesAt(params, exp, np.zeros(2), infRes=res, conditions=[0, 1])
    with pytest.raises(ValueError, match='not a device-backed result'):
        util.posteriorRatesAt(params, exp, np.zeros(2), infRes={'post_mean': []})
    assert sess.ctx.cov_calls == [] and sess.ctx.calls == []


def test_posterior_at_with_cov_in_want(monkeypatch):
    from funs import util
    sess, exp, params, res, touched = _fake_cov(monkeypatch, [8, 8, 8])
    times = np.array([-5.0, 0.0, 33.3])
    both = util.posteriorAt(params, exp, times, infRes=res, want=('mean', 'cov'))
    assert both['cov'].shape == (3, 3, 2, 2) and both['mean'].shape == (3, 2, 3)
    # the mean still comes from posterior_at, asked exactly as without 'cov'; the covariance from the new call, alone
    assert sess.ctx.calls[-1] == ((3,), ('mean',)) and sess.ctx.cov_calls[-1] == ((3,), ('cov',))
    plain = util.posteriorAt(params, exp, times, infRes=res, want=('mean',))
    assert np.array_equal(plain['mean'], both['mean']) and len(sess.ctx.cov_calls) == 1
    n_at = len(sess.ctx.calls)
    only = util.posteriorAt(params, exp, times, infRes=res, want=('cov',))
    assert sorted(only) == ['cov', 'times'] and len(sess.ctx.calls) == n_at            # posterior_at is not called for the covariance alone
    with pytest.raises(ValueError, match='unknown key'):
        util.posteriorAt(params, exp, times, infRes=res, want=('cov', 'rate'))
    with pytest.raises(ValueError, match=r'times: entry \(1,\) is not finite'):
        util.posteriorAt(params, exp, np.array([0.0, np.inf]), infRes=res, want=('cov',))
    with pytest.raises(ValueError, match='times'):
        util.posteriorAt(params, exp, np.zeros((2, 4)), infRes=res, want=('cov',))
