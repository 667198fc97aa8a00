"""Host side of the latent velocities at arbitrary time points (pgpfa_posterior_velocity_at), without a GPU:

* header, binding and built library agree on the entry point and the option key, the unit is part of the build, a null context is refused;
* what util.posteriorVelocityAt does around the device call, on the fake session of test_cpu_posterior_at.py whose context answers in closed form;
* the numpy restatement numpy_velocity - the yardstick of test_gpu_posterior_velocity.py - is pinned by central differences of the dense posterior
  (which know the kernel's values only, not its derivative) at off-grid times, on a dense Laplace posterior built in numpy at 30 x 3 x 100 and
  20 x 1 x 21: see test_numpy_velocity_is_pinned_by_central_differences for the figures.

Every test prints its figures before it asserts."""
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
DEVICE_KEYS = ('mean', 'var', 'vel', 'vel_var', 'cross')
FD_SHAPES = [(30, 3, 100), (20, 1, 21)]
FD_H_MS = 0.05                      # step of the central differences the GPU test repeats through ctx.posterior_at
# Limits of the central-difference checks: ten times what the pinned seeds give (the docstring of the test below has the measured values)
FD_LIMIT_MEAN = 4.0e-6             # |vel - FD of the mean| / max|vel| at h = FD_H_MS
FD_LIMIT_VELVAR = 5.0e-6           # of kappa
FD_LIMIT_CROSS = 1.0e-6            # of sqrt(kappa)


# ---- the yardstick -------------------------------------------------------------------------------------------------------------------------------
def smooth_cross(tau_k, s, L):
    """(L, S): covariance of the SMOOTH component of one latent at the times s with the grid values j bin, j < L (kx without its nugget term)"""
    dt = s[None, :] - (np.arange(L, dtype=np.float64) * BIN_MS)[:, None]
    return (1.0 - EPS) * np.exp(-0.5 * ((dt * dt) / (tau_k * 1000.0) ** 2))


def cross_gram(tau_k, s, L):
    """kx (L, S) of one latent: the smooth part plus eps where a query time IS a grid time"""
    tg = np.arange(L, dtype=np.float64) * BIN_MS
    return smooth_cross(tau_k, s, L) + EPS * (s[None, :] == tg[:, None])


def cross_gram_dot(tau_k, s, L):
    """kd (L, S): d/ds of the smooth part, per SECOND"""
    dt = s[None, :] - (np.arange(L, dtype=np.float64) * BIN_MS)[:, None]
    den = (tau_k * 1000.0) ** 2
    return -1000.0 * dt / den * ((1.0 - EPS) * np.exp(-0.5 * ((dt * dt) / den)))


def kappa(tau):
    return (1.0 - EPS) / (np.asarray(tau, dtype=np.float64) ** 2)


def numpy_velocity(tau, m, V, s, explicit_inverse=False):
    """mean, var, vel, vel_var, cross (each (p, S)) by the formulas of include/pgpfa.h from m (p, L) and the blocks V (L, L, p), through
    np.linalg.solve (explicit_inverse: through np.linalg.inv instead, the other evaluation order)"""
    p, L = m.shape
    s = np.asarray(s, dtype=np.float64)
    K = orc.make_K(tau, L, BIN_MS)
    out = {k: np.empty((p, s.size)) for k in DEVICE_KEYS}
    for k in range(p):
        kx, kd = cross_gram(tau[k], s, L), cross_gram_dot(tau[k], s, L)
        if explicit_inverse:
            Ki = np.linalg.inv(K[k])
            a, b = Ki @ kx, Ki @ kd
        else:
            a, b = np.linalg.solve(K[k], kx), np.linalg.solve(K[k], kd)
        Va, Vb = V[:, :, k] @ a, V[:, :, k] @ b
        out['mean'][k] = a.T @ m[k]
        out['vel'][k] = b.T @ m[k]
        out['var'][k] = np.maximum(1.0 - (a * kx).sum(axis=0) + (a * Va).sum(axis=0), 0.0)
        out['vel_var'][k] = np.maximum(kappa(tau[k]) - (b * kd).sum(axis=0) + (b * Vb).sum(axis=0), 0.0)
        out['cross'][k] = -(a * kd).sum(axis=0) + (a * Vb).sum(axis=0)
    return out


def dense_laplace_posterior(shape, seed=0):
    """tau, m (p, T), V (T, T, p) of one trial: the polished Laplace mode of the problem of test_cpu_posterior_samples.py and the diagonal blocks
    of the plain dense inverse of its Hessian"""
    q, p, T = shape
    par, Y, _ = problem(shape, seed=seed, R=1)
    Kinv = np.linalg.inv(orc.make_K(par['tau'], T, BIN_MS))
    m, _, _ = orc.newton_mode(Y[0].astype(np.float64), par['C'], par['d'], Kinv)
    H = dense_precision(curvature_blocks(m, par['C'], par['d']), par['tau'], T, BIN_MS)
    V, _ = orc.marginal_blocks(np.linalg.inv(H), p, T)
    return par['tau'], m, V


def central_differences(tau, m, V, s, h):
    """vel, vel_var, cross (p, S) at OFF-grid times s by central differences with step h ms of the dense posterior of the smooth component: its mean
    g(s)^T K^-1 m and its cross-time covariance C(s, s') = k(s - s') - g(s)^T K^-1 g(s') + g(s)^T K^-1 V K^-1 g(s'), g the smooth cross Gram.  Only
    values of the kernel enter, never its derivative.  C is bilinear in g, so the second difference is formed on g first (the same number with
    less cancellation) and the prior part 2 (k(0) - k(2h)) through expm1."""
    p, L = m.shape
    K = orc.make_K(tau, L, BIN_MS)
    vel, vel_var, cross = (np.empty((p, s.size)) for _ in range(3))
    for k in range(p):
        g0 = smooth_cross(tau[k], s, L)
        dg = (smooth_cross(tau[k], s + h, L) - smooth_cross(tau[k], s - h, L)) / (2.0 * h) * 1000.0         # per second
        a0, ad = np.linalg.solve(K[k], g0), np.linalg.solve(K[k], dg)
        vel[k] = ad.T @ m[k]
        prior = -2.0 * (1.0 - EPS) * np.expm1(-0.5 * (2.0 * h) ** 2 / (tau[k] * 1000.0) ** 2) / (2.0 * h) ** 2 * 1.0e6
        vel_var[k] = prior - (ad * dg).sum(axis=0) + (ad * (V[:, :, k] @ ad)).sum(axis=0)
        cross[k] = -(a0 * dg).sum(axis=0) + (a0 * (V[:, :, k] @ ad)).sum(axis=0)        # (the prior part k(h) - k(-h) is 0)
    return vel, vel_var, cross


def off_grid_times(T, n, seed):
    """n seeded times over [-2 bin, (T + 1) bin], none within 0.2 bin of a grid time (so that s +- h stays off the grid as well)"""
    rng = np.random.default_rng(seed)
    j = rng.integers(-2, T + 1, n)
    return (j + rng.uniform(0.2, 0.8, n)) * BIN_MS


@pytest.mark.parametrize('shape', FD_SHAPES, ids=['q%d-p%d-T%d' % s for s in FD_SHAPES])
def test_numpy_velocity_is_pinned_by_central_differences(shape):
    """Measured with the pinned seeds (relative to max|vel|, kappa_k, sqrt(kappa_k)):
      30 x 3 x 100: mean 1.53e-6 / 1.53e-8 / 1.72e-10 at h = 0.1 / 0.01 / 0.001 ms (ratios 100, 89: at the last step rounding begins to show);
                    at h = 0.05 ms mean 3.83e-7, vel_var 4.61e-7, cross 8.53e-8
      20 x 1 x 21:  mean 1.32e-6 / 1.32e-8 / 1.98e-10 (ratios 100, 67); at h = 0.05 ms mean 3.30e-7, vel_var 1.91e-7, cross 3.77e-8
    The limits FD_LIMIT_* above are ten times the larger of the two shapes, rounded up.  solve against the explicit inverse: at most 8.5e-13 in
    every output at both shapes (relative to max|m|, 1, max|vel|, kappa, sqrt(kappa)); ten times that stays under 1e-9, so 1e-9 is the "same
    inputs" tolerance of test_gpu_posterior_velocity.py.  The posterior correlation of value and velocity reaches 0.77 / 0.88."""
    q, p, T = shape
    tau, m, V = dense_laplace_posterior(shape)
    s = off_grid_times(T, 40, 17)
    ref = numpy_velocity(tau, m, V, s)
    kap = kappa(tau)[:, None]
    scale_v = float(np.max(np.abs(ref['vel'])))
    e_mean = []
    for h in (0.1, 0.01, 0.001):
        fd_vel, _, _ = central_differences(tau, m, V, s, h)
        e_mean.append(float(np.max(np.abs(fd_vel - ref['vel'])) / scale_v))
    ratios = [e_mean[0] / e_mean[1], e_mean[1] / e_mean[2]]
    fd_vel, fd_vv, fd_cr = central_differences(tau, m, V, s, FD_H_MS)
    e_m = float(np.max(np.abs(fd_vel - ref['vel'])) / scale_v)
    e_vv = float(np.max(np.abs(fd_vv - ref['vel_var']) / kap))
    e_cr = float(np.max(np.abs(fd_cr - ref['cross']) / np.sqrt(kap)))
    rho = ref['cross'] / np.sqrt(ref['var'] * ref['vel_var'])
    print('q=%d p=%d T=%d: mean against central differences at h = 0.1 / 0.01 / 0.001 ms: %.2e %.2e %.2e of max|vel| (ratios %.1f %.1f); at h = %.2f ms: '
          'mean %.2e (limit %.1e), vel_var %.2e of kappa (limit %.1e), cross %.2e of sqrt(kappa) (limit %.1e); largest |corr(value, velocity)| %.2f'
          % (q, p, T, e_mean[0], e_mean[1], e_mean[2], ratios[0], ratios[1], FD_H_MS, e_m, FD_LIMIT_MEAN, e_vv, FD_LIMIT_VELVAR, e_cr, FD_LIMIT_CROSS,
             float(np.max(np.abs(rho)))))
    inv = numpy_velocity(tau, m, V, s, explicit_inverse=True)
    scales = {'mean': float(np.max(np.abs(m))), 'var': 1.0, 'vel': scale_v, 'vel_var': kap, 'cross': np.sqrt(kap)}
    spread = {k: float(np.max(np.abs(inv[k] - ref[k]) / scales[k])) for k in DEVICE_KEYS}
    print('q=%d p=%d T=%d: np.linalg.solve against the explicit inverse: %s' % (q, p, T, ', '.join('%s %.1e' % kv for kv in spread.items())))
    assert all(30.0 <= r <= 300.0 for r in ratios), ratios
    assert e_m <= FD_LIMIT_MEAN and e_vv <= FD_LIMIT_VELVAR and e_cr <= FD_LIMIT_CROSS
    assert 10.0 * max(spread.values()) < 1e-9
    # the joint is a covariance, and its far field is the prior
    assert np.all(ref['var'] * ref['vel_var'] - ref['cross'] ** 2 >= -1e-9 * kap)
    far = numpy_velocity(tau, m, V, np.array([-50.0e3 * tau.max(), (T - 1) * BIN_MS + 50.0e3 * tau.max()]))
    assert np.all(far['vel'] == 0.0) and np.all(far['cross'] == 0.0) and np.all(far['var'] == 1.0) and np.array_equal(far['vel_var'], np.broadcast_to(kap, (p, 2)))


# ---- header, binding, library, build ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def hip():
    import __graft_entry__ as ge
    ge.build()
    from funs import _hip
    return _hip


def test_header_binding_and_library_agree_on_the_new_entry_point(hip):
    lib = hip.load_library()
    header = open(os.path.join(ROOT, 'include', 'pgpfa.h')).read()
    bare = re.sub(r'/\*.*?\*/', ' ', header, flags=re.S)              # (the declaration without its comments)
    dbl = r'\s*,\s*double\s*\*\s*'
    assert re.search(r'int\s+pgpfa_posterior_velocity_at\s*\(\s*pgpfa_ctx\s*\*\s*ctx\s*,\s*int\s+n\s*,\s*const\s+int32_t\s*\*\s*idx\s*,\s*int\s+S\s*,\s*const\s+double\s*\*\s*'
                     r'times_ms\s*,\s*int\s+per_trial' + dbl + 'mean' + dbl + 'var' + dbl + 'vel' + dbl + 'vel_var' + dbl + r'cross\s*\)\s*;', bare)
    assert 'pgpfa_posterior_velocity_at' in hip.EXPORTED_SYMBOLS and hasattr(lib, 'pgpfa_posterior_velocity_at')
    c_double_p, c_int32_p = ct.POINTER(ct.c_double), ct.POINTER(ct.c_int32)
    assert list(lib.pgpfa_posterior_velocity_at.argtypes) == [ct.c_void_p, ct.c_int, c_int32_p, ct.c_int, c_double_p, ct.c_int] + [c_double_p] * 5
    assert '"velat_chunk_trials"' in header
    assert hasattr(hip.Context, 'posterior_velocity_at')
    from funs import engine, util
    assert callable(util.posteriorVelocityAt) and callable(engine.PPGPFAfit.posteriorVelocityAt)


def test_the_unit_is_part_of_the_build():
    import __graft_entry__ as ge
    assert 'velat' in ge.UNITS
    assert os.path.exists(os.path.join(ge.CSRC, 'velat.hip')) and os.path.exists(os.path.join(ge.CSRC, 'velat.h'))


def test_null_context_is_refused_without_a_device(hip):
    lib = hip.load_library()
    t, out = np.zeros(1), np.zeros(1)
    assert lib.pgpfa_posterior_velocity_at(None, 1, None, 1, hip.dptr(t), 0, None, None, hip.dptr(out), None, None) != 0
    assert 'null context' in lib.pgpfa_last_error().decode()


# ---- util.posteriorVelocityAt around a fake device ---------------------------------------------------------------------------------------------------
def _fake_velocity(monkeypatch, lens, **kw):
    """the fake session of test_cpu_posterior_at.py whose context also answers posterior_velocity_at in closed form: with g = (trial + 1) (latent + 1),
    mean = g s / 100, vel = g / 10 - s / 50, var = 0.25 + (s / 1000)^2, vel_var = 4 + latent + (s / 500)^2, cross = 0.1 - s / 1e4"""
    sess, exp, params, res, touched = _fake(monkeypatch, lens, **kw)
    ctx = sess.ctx
    ctx.vcalls = []

    def posterior_velocity_at(times, idx=None, want=('mean', 'vel')):
        tt = np.asarray(times, dtype=np.float64)
        ctx.vcalls.append((tt.shape, tuple(want)))
        n = len(idx)
        s = np.broadcast_to(tt, (n, tt.shape[-1]))[:, None, :]
        g = (np.asarray(idx)[:, None, None] + 1.0) * (np.arange(ctx.p)[None, :, None] + 1.0)
        full = {'mean': g * s / 100.0, 'vel': g / 10.0 - s / 50.0, 'var': 0.25 + (s / 1000.0) ** 2 + 0.0 * g,
                'vel_var': 4.0 + np.arange(ctx.p)[None, :, None] + (s / 500.0) ** 2 + 0.0 * g, 'cross': 0.1 - s / 1.0e4 + 0.0 * g}
        return {k: np.ascontiguousarray(full[k]) for k in DEVICE_KEYS if k in want}
    ctx.posterior_velocity_at = posterior_velocity_at
    return sess, exp, params, res, touched


def test_shapes_keys_and_what_the_device_is_asked_for(monkeypatch):
    from funs import util
    sess, exp, params, res, _ = _fake_velocity(monkeypatch, [8, 8, 8])
    times = np.array([-5.0, 0.0, 33.3, 140.0, 33.3])
    out = util.posteriorVelocityAt(params, exp, times, infRes=res)
    assert sorted(out) == ['lower', 'times', 'upper', 'vel'] and out['vel'].shape == (3, 2, 5) and np.array_equal(out['times'], times)
    assert sess.ctx.vcalls[-1] == ((5,), ('vel', 'vel_var')) and sess.ctx.calls == []
    assert np.array_equal(out['vel'][2, 1], 3.0 * 2.0 / 10.0 - times / 50.0)
    allk = util.posteriorVelocityAt(params, exp, times, infRes=res, want=('vel', 'var', 'lower', 'upper', 'value', 'value_var', 'cross', 'speed2'))
    assert sess.ctx.vcalls[-1] == ((5,), DEVICE_KEYS)
    assert all(allk[k].shape == (3, 2, 5) for k in ('vel', 'var', 'lower', 'upper', 'value', 'value_var', 'cross')) and allk['speed2'].shape == (3, 5)
    assert np.array_equal(allk['value'][1, 0], 2.0 * times / 100.0) and np.array_equal(allk['var'][0, 1], 5.0 + (times / 500.0) ** 2)
    assert np.array_equal(allk['value_var'][0, 0], 0.25 + (times / 1000.0) ** 2) and np.array_equal(allk['cross'][2, 1], 0.1 - times / 1.0e4)
    # one grid per trial; only what is needed is asked of the device
    event, lags = np.array([40.0, 60.0]), np.array([-20.0, 0.0, 20.0, 40.0])
    per = util.posteriorVelocityAt(params, exp, event[:, None] + lags[None, :], infRes=res, trials=[2, 0], want=('vel',))
    assert per['vel'].shape == (2, 2, 4) and per['times'].shape == (2, 4) and sess.ctx.vcalls[-1] == ((2, 4), ('vel',))
    assert np.array_equal(per['vel'][0, 0], 3.0 / 10.0 - (40.0 + lags) / 50.0) and np.array_equal(per['vel'][1, 1], 2.0 / 10.0 - (60.0 + lags) / 50.0)
    util.posteriorVelocityAt(params, exp, times, infRes=res, want=('cross', 'value'))
    assert sess.ctx.vcalls[-1] == ((5,), ('mean', 'cross'))
    util.posteriorVelocityAt(params, exp, times, infRes=res, want=('var',))
    assert sess.ctx.vcalls[-1] == ((5,), ('vel_var',))


def test_shape_errors_unknown_keys_and_an_empty_request(monkeypatch):
    from funs import util
    sess, exp, params, res, _ = _fake_velocity(monkeypatch, [8, 8, 8])
    for bad in (np.zeros((2, 4)), np.zeros((3, 2, 2)), np.zeros(0), np.zeros((3, 0)), 5.0):
        with pytest.raises(ValueError, match='times'):
            util.posteriorVelocityAt(params, exp, bad, infRes=res)
    with pytest.raises(ValueError, match='times'):
        util.posteriorVelocityAt(params, exp, np.zeros((3, 4)), infRes=res, trials=[0, 1])     # three grids for two listed trials
    with pytest.raises(ValueError, match='unknown key'):
        util.posteriorVelocityAt(params, exp, np.zeros(2), infRes=res, want=('vel', 'mean'))
    with pytest.raises(ValueError, match='nothing asked for'):
        util.posteriorVelocityAt(params, exp, np.zeros(2), infRes=res, want=())
    with pytest.raises(ValueError, match='level'):
        util.posteriorVelocityAt(params, exp, np.zeros(2), infRes=res, level=1.0)
    with pytest.raises(ValueError, match='one label per listed trial'):
        util.posteriorVelocityAt(params, exp, np.zeros(2), infRes=res, conditions=[0, 1])
    with pytest.raises(ValueError, match='not a device-backed result'):
        util.posteriorVelocityAt(params, exp, np.zeros(2), infRes={'post_mean': []})
    assert sess.ctx.vcalls == [] and sess.ctx.calls == []


def test_a_time_that_is_not_finite_is_refused_before_any_device_call(monkeypatch):
    from funs import util
    sess, exp, params, res, touched = _fake_velocity(monkeypatch, [8, 8, 8])
    with pytest.raises(ValueError, match=r'times: entry \(2,\) is not finite'):
        util.posteriorVelocityAt(params, exp, np.array([0.0, 1.0, np.nan]), infRes=res)
    grid = np.zeros((3, 4))
    grid[1, 3] = np.inf
    with pytest.raises(ValueError, match=r'times: entry \(1, 3\) is not finite'):
        util.posteriorVelocityAt(params, exp, grid, infRes=res)
    assert touched == [] and sess.ctx.vcalls == []                  # not even the session was looked up


def test_band_and_speed2_arithmetic(monkeypatch):
    from funs import util
    sess, exp, params, res, _ = _fake_velocity(monkeypatch, [8, 8])
    times = np.array([0.0, 70.0, 500.0])
    out = util.posteriorVelocityAt(params, exp, times, infRes=res, level=0.9, want=('vel', 'var', 'lower', 'upper', 'speed2'))
    z = util._band_z(0.9)
    assert np.array_equal(out['lower'], out['vel'] - z * np.sqrt(out['var'])) and np.array_equal(out['upper'], out['vel'] + z * np.sqrt(out['var']))
    assert np.allclose(out['upper'][:, 1] - out['lower'][:, 1], 2.0 * z * np.sqrt(5.0 + (times / 500.0) ** 2)[None, :], rtol=1e-14)
    assert out['speed2'].shape == (2, 3)
    for i in range(2):
        want = sum(((i + 1.0) * (k + 1.0) / 10.0 - times / 50.0) ** 2 + 4.0 + k + (times / 500.0) ** 2 for k in range(2))
        assert np.allclose(out['speed2'][i], want, rtol=1e-15, atol=0.0)
    dflt = util.posteriorVelocityAt(params, exp, times, infRes=res)
    assert np.allclose(dflt['upper'] - dflt['vel'], 1.959963984540054 * np.sqrt(out['var']), rtol=1e-12)


def test_condition_means_of_the_velocity_over_ragged_spans(monkeypatch):
    from funs import util
    lens, bin_ms = [8, 3, 5, 8, 4], 20.0
    sess, exp, params, res, _ = _fake_velocity(monkeypatch, lens, bin_ms=bin_ms)
    tiny = 1e-9
    times = np.array([-tiny, 0.0, 40.0, 40.0 + tiny, 60.0, 60.0 + tiny, 80.0, 80.0 + tiny, 140.0, 140.0 + tiny, 10.0])
    cond = [7, 7, 3, 7, 3]
    out = util.posteriorVelocityAt(params, exp, times, infRes=res, conditions=cond, want=('vel',))
    assert out['condition_labels'].tolist() == [3, 7]
    span = (np.asarray(lens) - 1) * bin_ms
    inside = (times[None, :] >= 0.0) & (times[None, :] <= span[:, None])
    assert out['condition_count'].tolist() == [inside[[2, 4]].sum(axis=0).tolist(), inside[[0, 1, 3]].sum(axis=0).tolist()]
    assert out['condition_count'][1].tolist() == [0, 3, 3, 2, 2, 2, 2, 2, 2, 0, 3]
    for g, members in ((0, [2, 4]), (1, [0, 1, 3])):
        for j in range(times.size):
            who = [i for i in members if inside[i, j]]
            ref = sum(out['vel'][i][:, j] for i in who) / len(who) if who else np.zeros(2)
            assert np.allclose(out['condition_mean'][g][:, j], ref, rtol=1e-15, atol=0.0)
    assert np.all(out['condition_mean'][:, :, 0] == 0.0)
    # want=() with conditions asks the device for the velocity alone
    per = util.posteriorVelocityAt(params, exp, np.tile(times, (5, 1)), infRes=res, conditions=cond, want=())
    assert sorted(per) == ['condition_count', 'condition_labels', 'condition_mean', 'times'] and sess.ctx.vcalls[-1] == ((5, 11), ('vel',))
    assert np.array_equal(per['condition_mean'], out['condition_mean'])
