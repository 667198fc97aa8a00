"""Host side of the posterior of linear functionals of the latents (pgpfa_posterior_functionals), without a GPU: header, binding and library agree on
the entry point, the unit is part of the build, the numpy restatement the GPU tests hold the device to

    Cov(U^T x) = (M^T U)^T (M^T U),   Sigma = M M^T        (low-rank root: Q^T Q + eps U^T V with V = G U, Q = L^-1 F^T V)

is itself checked against U^T inv(H) U by both square roots, and what util.posteriorEpochs / util.posteriorFunctionals do around the device call:
window weights, alignment, refusals, bands, contrasts and condition means on a fake context.

The spread of the restatement - the largest difference between any of its forms and U^T inv(H) U, of the largest entry of |U|^T |Sigma| |U| - is
printed by the test; the limits of test_gpu_posterior_functionals.py (1e-9 on the engine's own inputs, 1e-8 for the low-rank root against the exact
dense inverse) must be at least ten times it, which the test asserts.  Every test prints its figures before it asserts."""
import ctypes as ct
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from oracle import pgpfa_oracle as orc
from test_cpu_posterior_at import _fake
from test_cpu_posterior_samples import curvature_blocks, dense_precision, lowrank_factors, problem, sqrt_dense, sqrt_lowrank

BIN_MS = 10.0
EPS = orc.EPS_NOISE
TOL_SAME, TOL_DENSE = 1e-9, 1e-8


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
    assert re.search(r'int\s+pgpfa_posterior_functionals\s*\(\s*pgpfa_ctx\s*\*\s*ctx\s*,\s*int\s+n\s*,\s*const\s+int32_t\s*\*\s*idx\s*,\s*int\s+J\s*,\s*const\s+double\s*\*\s*'
                     r'weights\s*,\s*int\s+per_trial\s*,\s*double\s*\*\s*mean\s*,\s*double\s*\*\s*var\s*,\s*double\s*\*\s*cov\s*\)\s*;', bare)
    assert 'pgpfa_posterior_functionals' in hip.EXPORTED_SYMBOLS and hasattr(lib, 'pgpfa_posterior_functionals')
    c_double_p, c_int32_p = ct.POINTER(ct.c_double), ct.POINTER(ct.c_int32)
    assert list(lib.pgpfa_posterior_functionals.argtypes) == [ct.c_void_p, ct.c_int, c_int32_p, ct.c_int, c_double_p, ct.c_int] + [c_double_p] * 3
    assert '"func_chunk_trials"' in header and '"func_block_cols"' in header
    assert hasattr(hip.Context, 'posterior_functionals')
    from funs import engine, util
    assert callable(util.posteriorFunctionals) and callable(util.posteriorEpochs)
    assert callable(engine.PPGPFAfit.posteriorFunctionals) and callable(engine.PPGPFAfit.posteriorEpochs)


def test_the_unit_is_part_of_the_build():
    import __graft_entry__ as ge
    assert 'pfunc' in ge.UNITS
    assert os.path.exists(os.path.join(ge.CSRC, 'pfunc.hip')) and os.path.exists(os.path.join(ge.CSRC, 'pfunc.h'))


def test_null_context_is_refused_without_a_device(hip):
    lib = hip.load_library()
    w = np.zeros(1)
    out = np.zeros(1)
    assert lib.pgpfa_posterior_functionals(None, 1, None, 1, hip.dptr(w), 0, hip.dptr(out), None, None) != 0
    assert 'null context' in lib.pgpfa_last_error().decode()


# ---- the restatement against U^T inv(H) U ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(30, 3, 100), (12, 2, 21)], ids=['q30-p3-T100', 'q12-p2-T21'])
def test_the_numpy_restatement_by_both_roots_against_the_dense_inverse(shape):
    q, p, T = shape
    par, _, X = problem(shape, R=1)
    W = curvature_blocks(X[0], par['C'], par['d'])
    H = dense_precision(W, par['tau'], T, BIN_MS)
    Sigma = np.linalg.inv(0.5 * (H + H.T))
    rng = np.random.default_rng(3)
    J = 17
    U = rng.standard_normal((J, p, T))
    U[J - 4:] = 0.0
    for j in range(J - 4, J):                                          # four sparse windows
        U[j, j % p, 3 * (j - J + 5):3 * (j - J + 5) + 5] = 0.2
    Uf = U.reshape(J, p * T).T                                         # (p T, J), latent-major rows
    ref = Uf.T @ Sigma @ Uf
    scale = float(np.max(np.abs(Uf).T @ np.abs(Sigma) @ np.abs(Uf)))
    Qd = sqrt_dense(H).T @ Uf
    e_dense = float(np.max(np.abs(Qd.T @ Qd - ref)) / scale)
    # low-rank root, whole: M = [sqrt(eps) chol(G) | G F L^-T]
    F = lowrank_factors(par['tau'], T, BIN_MS)
    M = sqrt_lowrank(W, F)
    Ql = M.T @ Uf
    e_lr = float(np.max(np.abs(Ql.T @ Ql - ref)) / scale)
    # ... and split the way the device walks it: V = G U per bin, Q = (G F L^-T)^T U = L^-1 F^T V, cov = Q^T Q + eps U^T V
    G = np.linalg.inv(np.eye(p)[None] + EPS * W)
    G = 0.5 * (G + G.transpose(0, 2, 1))
    V = np.einsum('tlk,jkt->jlt', G, U).reshape(J, p * T).T
    Q = M[:, p * T:].T @ Uf
    split = Q.T @ Q + EPS * (Uf.T @ V)
    e_split = float(np.max(np.abs(split - ref)) / scale)
    e_forms = float(np.max(np.abs(split - Ql.T @ Ql)) / scale)
    spread_same, spread_lr = max(e_dense, e_forms), max(e_lr, e_split)
    print('q=%d p=%d T=%d: (M^T U)^T (M^T U) against U^T inv(H) U, of the largest entry of |U|^T |Sigma| |U|: dense root %.2e, low-rank root %.2e, its split '
          'form Q^T Q + eps U^T V %.2e; the two low-rank forms against each other %.2e.  Spread on the same inputs %.2e (ten times that against %.0e), of the '
          'low-rank root against the exact inverse %.2e (ten times that against %.0e)' % (q, p, T, e_dense, e_lr, e_split, e_forms, spread_same, TOL_SAME, spread_lr, TOL_DENSE))
    assert 10.0 * spread_same <= TOL_SAME
    assert 10.0 * spread_lr <= TOL_DENSE


# ---- posteriorEpochs: the windows ----------------------------------------------------------------------------------------------------------------
def test_epoch_windows_membership_at_the_edges_and_alignment():
    from funs import util
    T, lens, pos = 12, np.array([12, 12, 9]), np.array([0, 1, 2])
    W = util._epoch_windows([(20.0, 50.0), (0.0, 10.0), (19.999, 50.001), (100.0, 120.0)], BIN_MS, T, lens[:2], pos[:2], None, False)
    assert W.shape == (4, T)
    member = [np.flatnonzero(W[e]).tolist() for e in range(4)]
    assert member == [[2, 3, 4], [0], [2, 3, 4, 5], [10, 11]]           # start <= j bin < stop: the start bin is in, the stop bin is out
    for e in range(4):
        assert np.array_equal(W[e][member[e]], np.full(len(member[e]), 1.0 / len(member[e])))
    # a bin size that is no binary fraction: membership by the comparison j * binSize itself
    W3 = util._epoch_windows([(0.3, 0.9)], 0.1, T, lens[:2], pos[:2], None, False)
    tj = np.arange(T) * 0.1
    assert np.flatnonzero(W3[0]).tolist() == np.flatnonzero((tj >= 0.3) & (tj < 0.9)).tolist()
    # alignment: one shift per listed trial
    Wa = util._epoch_windows([(-20.0, 10.0), (0.0, 30.0)], BIN_MS, T, lens, pos, [30.0, 55.0, 40.0], False)
    assert Wa.shape == (3, 2, T)
    assert [np.flatnonzero(Wa[i, e]).tolist() for i in range(3) for e in range(2)] == [[1, 2, 3], [3, 4, 5], [4, 5, 6], [6, 7, 8], [2, 3, 4], [4, 5, 6]]
    assert np.allclose(Wa.sum(axis=2), 1.0, rtol=1e-15, atol=0.0)
    # functionals of the latent vector: window e on latent k alone
    Uf = util._latent_functionals(Wa, 2)
    assert Uf.shape == (3, 4, 2, T)
    assert np.array_equal(Uf[1, 2, 0], Wa[1, 1]) and np.array_equal(Uf[1, 3, 1], Wa[1, 1]) and not Uf[1, 2, 1].any() and not Uf[1, 3, 0].any()


def test_epoch_window_refusals():
    from funs import util
    T, lens, pos = 12, np.array([12, 9]), np.array([4, 7])
    with pytest.raises(ValueError, match=r'window 1, \[31, 39\) ms, holds no bin'):
        util._epoch_windows([(0.0, 10.0), (31.0, 39.0)], BIN_MS, T, lens, pos, None, True)
    with pytest.raises(ValueError, match='window 0.*holds no bin'):
        util._epoch_windows([(30.0, 30.0)], BIN_MS, T, lens, pos, None, True)
    with pytest.raises(ValueError, match=r'window 0, bins -1 \.\. 2, leaves the grid \[0, 12\)'):
        util._epoch_windows([(-10.0, 30.0)], BIN_MS, T, lens, pos, None, True)
    with pytest.raises(ValueError, match=r'window 1, bins 10 \.\. 12, leaves the grid'):
        util._epoch_windows([(0.0, 10.0), (100.0, 130.0)], BIN_MS, T, lens, pos, None, True)
    with pytest.raises(ValueError, match=r'window 0, bins 7 \.\. 9, passes the 9 bins of trial 7 \(list entry 1\); forecast=True'):
        util._epoch_windows([(70.0, 100.0)], BIN_MS, T, lens, pos, None, False)
    assert util._epoch_windows([(70.0, 100.0)], BIN_MS, T, lens, pos, None, True).shape == (1, T)
    assert util._epoch_windows([(60.0, 90.0)], BIN_MS, T, lens, pos, None, False).shape == (1, T)          # bins 6 .. 8: inside
    with pytest.raises(ValueError, match=r'window 0 of list entry 1 \(trial 7, aligned to 50 ms\), bins 10 \.\. 12, leaves the grid'):
        util._epoch_windows([(50.0, 80.0)], BIN_MS, T, lens, pos, [0.0, 50.0], True)
    with pytest.raises(ValueError, match=r'passes the 9 bins of trial 7 \(list entry 1\)'):
        util._epoch_windows([(50.0, 80.0)], BIN_MS, T, lens, pos, [0.0, 20.0], False)
    with pytest.raises(ValueError, match='align: one event time in ms per listed trial expected'):
        util._epoch_windows([(50.0, 80.0)], BIN_MS, T, lens, pos, [0.0], False)
    with pytest.raises(ValueError, match='align: the event time of list entry 1 is not finite'):
        util._epoch_windows([(50.0, 80.0)], BIN_MS, T, lens, pos, [0.0, np.nan], False)
    for bad in ([], [(1.0, 2.0, 3.0)], [1.0, 2.0]):
        with pytest.raises(ValueError, match='epochs: a list of'):
            util._epoch_windows(bad, BIN_MS, T, lens, pos, None, False)
    with pytest.raises(ValueError, match='epochs: window 1 is not finite'):
        util._epoch_windows([(0.0, 10.0), (0.0, np.inf)], BIN_MS, T, lens, pos, None, False)


# ---- util around a fake device -------------------------------------------------------------------------------------------------------------------
def _fake_func(monkeypatch, lens, **kw):
    """the fake session of test_cpu_posterior_at.py whose context answers posterior_functionals from a fixed mean and covariance per trial:
    m_r[k][t] = (r + 1) (k + 1) t / 10, Sigma_r = (r + 1) (A A^T + I), A seeded"""
    sess, exp, params, res, touched = _fake(monkeypatch, lens, **kw)
    ctx, T, p = sess.ctx, sess.T, sess.p
    rng = np.random.default_rng(5)
    A = rng.standard_normal((p * T, p * T)) / np.sqrt(p * T)
    base = A @ A.T + np.eye(p * T)
    ctx.func_calls = []
    ctx.m = lambda r: (r + 1.0) * (np.arange(p)[:, None] + 1.0) * np.arange(T)[None, :] / 10.0
    ctx.Sigma = lambda r: (r + 1.0) * base

    def posterior_functionals(weights, trials=None, want=('mean', 'var')):
        ww = np.asarray(weights, dtype=np.float64)
        ctx.func_calls.append((ww.shape, tuple(want)))
        n = len(trials)
        sets = np.broadcast_to(ww, (n,) + ww.shape[-3:]).reshape(n, ww.shape[-3], p * T)
        mean = np.stack([sets[i] @ ctx.m(int(r)).reshape(-1) for i, r in enumerate(trials)])
        cov = np.stack([sets[i] @ ctx.Sigma(int(r)) @ sets[i].T for i, r in enumerate(trials)])
        made = {'mean': mean, 'var': np.diagonal(cov, axis1=1, axis2=2).copy(), 'cov': cov}
        return {k: made[k] for k in want}
    ctx.posterior_functionals = posterior_functionals
    return sess, exp, params, res, touched


def test_posterior_epochs_bands_contrasts_eta_and_condition_means(monkeypatch):
    from funs import util
    lens = [8, 8, 6, 8]
    sess, exp, params, res, _ = _fake_func(monkeypatch, lens, bin_ms=20.0)
    params['C'] = np.random.default_rng(1).standard_normal((3, 2))
    params['d'] = np.array([-1.0, 0.5, 0.25])
    epochs, contrasts, cond = [(0.0, 40.0), (60.0, 120.0)], [(0, 1), (1, 0)], [7, 3, 7, 3]
    keys = ('mean', 'var', 'lower', 'upper', 'cov', 'contrast', 'contrastVar', 'contrastLower', 'contrastUpper', 'eta', 'etaVar', 'etaLower', 'etaUpper')
    out = util.posteriorEpochs(params, exp, epochs, infRes=res, contrasts=contrasts, conditions=cond, level=0.9, want=keys)
    ctx, T, p, q, E = sess.ctx, 8, 2, 3, 2
    # two device calls: the latents with the contrasts behind them (mean, var and the plane), the log rates without a plane
    assert ctx.func_calls == [((E * p + 2 * p, p, T), ('mean', 'var', 'cov')),((E * q, p, T), ('mean', 'var'))]
    z = util._band_z(0.9)
    w = np.zeros((E, T))
    w[0, 0:2], w[1, 3:6] = 0.5, 1.0 / 3.0
    for r in range(4):
        m, S = ctx.m(r), ctx.Sigma(r).reshape(p, T, p, T)
        mean = m @ w.T                                                   # (p, E)
        assert np.allclose(out['mean'][r], mean.T, rtol=1e-14, atol=0.0)
        cov = np.einsum('et,ktls,fs->ekfl', w, S, w).reshape(E * p, E * p)
        assert np.allclose(out['cov'][r], cov, rtol=1e-12, atol=1e-15)
        assert np.allclose(out['var'][r].reshape(-1), np.diag(cov), rtol=1e-12, atol=0.0)
        for i, (a, b) in enumerate(contrasts):
            assert np.allclose(out['contrast'][r, i], mean[:, b] - mean[:, a], rtol=1e-12, atol=1e-15)
            cv = np.array([cov[a * p + k, a * p + k] + cov[b * p + k, b * p + k] - 2.0 * cov[a * p + k, b * p + k] for k in range(p)])
            assert np.allclose(out['contrastVar'][r, i], cv, rtol=1e-11, atol=0.0)
        for e in range(E):
            assert np.allclose(out['eta'][r, e], params['d'] + params['C'] @ mean[:, e], rtol=1e-12, atol=1e-15)
            blk = cov[e * p:(e + 1) * p, e * p:(e + 1) * p]
            assert np.allclose(out['etaVar'][r, e], np.einsum('ni,ij,nj->n', params['C'], blk, params['C']), rtol=1e-11, atol=0.0)
    assert np.array_equal(out['lower'], out['mean'] - z * np.sqrt(out['var'])) and np.array_equal(out['upper'], out['mean'] + z * np.sqrt(out['var']))
    assert np.array_equal(out['contrastLower'], out['contrast'] - z * np.sqrt(out['contrastVar']))
    assert np.array_equal(out['contrastUpper'], out['contrast'] + z * np.sqrt(out['contrastVar']))
    assert np.array_equal(out['etaLower'], out['eta'] - z * np.sqrt(out['etaVar'])) and np.array_equal(out['etaUpper'], out['eta'] + z * np.sqrt(out['etaVar']))
    assert np.array_equal(out['contrast'][:, 0], -out['contrast'][:, 1]) and np.allclose(out['contrastVar'][:, 0], out['contrastVar'][:, 1], rtol=1e-12)
    assert out['condition_labels'].tolist() == [3, 7] and out['condition_count'].tolist() == [2, 2]
    assert np.allclose(out['condition_mean'][0], out['mean'][[1, 3]].mean(axis=0), rtol=1e-14) and np.allclose(out['condition_mean'][1], out['mean'][[0, 2]].mean(axis=0), rtol=1e-14)
    assert np.allclose(out['condition_contrast'][1], out['contrast'][[0, 2]].mean(axis=0), rtol=1e-14)
    # the defaults: contrasts add their three keys; only what is needed is asked of the device
    ctx.func_calls.clear()
    dflt = util.posteriorEpochs(params, exp, epochs, infRes=res, contrasts=contrasts)
    assert sorted(dflt) == ['contrast', 'contrastLower', 'contrastUpper', 'lower', 'mean', 'upper'] and ctx.func_calls == [((E * p + 2 * p, p, T), ('mean', 'var'))]
    only = util.posteriorEpochs(params, exp, epochs, infRes=res, trials=[3, 0], align=[20.0, 0.0], want=('eta',))
    assert ctx.func_calls[-1] == ((2, E * q, p, T), ('mean',)) and only['eta'].shape == (2, E, q)
    w3 = np.zeros(T)
    w3[1:3] = 0.5                                                        # trial 3: window 0 shifted by one bin
    assert np.allclose(only['eta'][0, 0], params['d'] + params['C'] @ (ctx.m(3) @ w3), rtol=1e-12, atol=1e-15)
    assert np.array_equal(only['eta'][1], out['eta'][0])
    avg = util.posteriorEpochs(params, exp, epochs, infRes=res, conditions=cond, want=())
    assert sorted(avg) == ['condition_count', 'condition_labels', 'condition_mean'] and np.array_equal(avg['condition_mean'], out['condition_mean'])


def test_posterior_epochs_argument_checks_need_no_device(monkeypatch):
    from funs import util
    sess, exp, params, res, touched = _fake_func(monkeypatch, [8, 5, 8])
    with pytest.raises(ValueError, match='holds no bin'):
        util.posteriorEpochs(params, exp, [(21.0, 39.0)], infRes=res)
    with pytest.raises(ValueError, match='leaves the grid'):
        util.posteriorEpochs(params, exp, [(100.0, 200.0)], infRes=res)
    with pytest.raises(ValueError, match=r'passes the 5 bins of trial 1 \(list entry 1\)'):
        util.posteriorEpochs(params, exp, [(80.0, 120.0)], infRes=res)
    with pytest.raises(ValueError, match=r'passes the 5 bins of trial 1 \(list entry 0\)'):
        util.posteriorEpochs(params, exp, [(80.0, 120.0)], infRes=res, trials=[1, 0])
    with pytest.raises(ValueError, match=r'contrasts: \(0, 2\) names an epoch outside 0 \.\. 1'):
        util.posteriorEpochs(params, exp, [(0.0, 40.0), (40.0, 80.0)], infRes=res, contrasts=[(0, 1), (0, 2)])
    with pytest.raises(ValueError, match=r'contrasts: \(-1, 0\) names an epoch'):
        util.posteriorEpochs(params, exp, [(0.0, 40.0), (40.0, 80.0)], infRes=res, contrasts=[(-1, 0)])
    with pytest.raises(ValueError, match='contrasts: a list of'):
        util.posteriorEpochs(params, exp, [(0.0, 40.0)], infRes=res, contrasts=[(0, 0, 0)])
    with pytest.raises(ValueError, match='needs contrasts'):
        util.posteriorEpochs(params, exp, [(0.0, 40.0)], infRes=res, want=('contrast',))
    with pytest.raises(ValueError, match='unknown key'):
        util.posteriorEpochs(params, exp, [(0.0, 40.0)], infRes=res, want=('mean', 'rate'))
    with pytest.raises(ValueError, match='level'):
        util.posteriorEpochs(params, exp, [(0.0, 40.0)], infRes=res, level=1.0)
    with pytest.raises(ValueError, match='nothing asked for'):
        util.posteriorEpochs(params, exp, [(0.0, 40.0)], infRes=res, want=())
    with pytest.raises(ValueError, match='one label per listed trial'):
        util.posteriorEpochs(params, exp, [(0.0, 40.0)], infRes=res, conditions=[0, 1])
    with pytest.raises(ValueError, match='align: one event time'):
        util.posteriorEpochs(params, exp, [(0.0, 40.0)], infRes=res, align=[0.0, 0.0])
    with pytest.raises(ValueError, match='trials: positions'):
        util.posteriorEpochs(params, exp, [(0.0, 40.0)], infRes=res, trials=[0, 3])
    assert touched == [] and sess.ctx.func_calls == []                 # not even the session was looked up
    assert util.posteriorEpochs(params, exp, [(80.0, 120.0)], infRes=res, forecast=True)['mean'].shape == (3, 1, 2)
    with pytest.raises(ValueError, match='not a device-backed result'):
        util.posteriorEpochs(params, exp, [(0.0, 40.0)], infRes={'post_mean': []})
    sess.comm_ready = True
    with pytest.raises(NotImplementedError, match='posteriorEpochs does not support sharded sessions'):
        util.posteriorEpochs(params, exp, [(0.0, 40.0)], infRes=res)
    with pytest.raises(NotImplementedError, match='posteriorFunctionals does not support sharded sessions'):
        util.posteriorFunctionals(params, exp, np.zeros((1, 2, 8)), infRes=res)


def test_posterior_functionals_keys_and_argument_checks(monkeypatch):
    from funs import util
    sess, exp, params, res, touched = _fake_func(monkeypatch, [8, 8, 8])
    U = np.random.default_rng(2).standard_normal((5, 2, 8))
    out = util.posteriorFunctionals(params, exp, U, infRes=res, level=0.8, want=('mean', 'var', 'sd', 'lower', 'upper', 'cov'))
    assert sess.ctx.func_calls[-1] == ((5, 2, 8), ('mean', 'var', 'cov')) and out['cov'].shape == (3, 5, 5)
    z = util._band_z(0.8)
    assert np.array_equal(out['sd'], np.sqrt(out['var'])) and np.array_equal(out['lower'], out['mean'] - z * out['sd']) and np.array_equal(out['upper'], out['mean'] + z * out['sd'])
    util.posteriorFunctionals(params, exp, U, infRes=res, want=('sd',))
    assert sess.ctx.func_calls[-1] == ((5, 2, 8), ('var',))                                 # no mean, no plane
    per = util.posteriorFunctionals(params, exp, np.stack([U, 2.0 * U]), infRes=res, trials=[2, 0], want=('mean',))
    assert sess.ctx.func_calls[-1] == ((2, 5, 2, 8), ('mean',)) and np.allclose(per['mean'][1], 2.0 * out['mean'][0], rtol=1e-14)
    n_calls, n_touched = len(sess.ctx.func_calls), len(touched)
    bad = U.copy()
    bad[4, 1, 6] = np.nan
    with pytest.raises(ValueError, match=r'weights: entry \(4, 1, 6\) is not finite'):
        util.posteriorFunctionals(params, exp, bad, infRes=res)
    with pytest.raises(ValueError, match='unknown key'):
        util.posteriorFunctionals(params, exp, U, infRes=res, want=('mean', 'rate'))
    with pytest.raises(ValueError, match='nothing asked for'):
        util.posteriorFunctionals(params, exp, U, infRes=res, want=())
    with pytest.raises(ValueError, match='level'):
        util.posteriorFunctionals(params, exp, U, infRes=res, level=0.0)
    for shape in ((2, 8), (0, 2, 8), (1, 1, 5, 2, 8)):
        with pytest.raises(ValueError, match='weights: shape'):
            util.posteriorFunctionals(params, exp, np.zeros(shape), infRes=res)
    assert len(touched) == n_touched                                   # not even the session was looked up
    for shape in ((5, 2, 7), (5, 3, 8), (2, 5, 2, 8)):
        with pytest.raises(ValueError, match='weights:.*expected'):
            util.posteriorFunctionals(params, exp, np.zeros(shape), infRes=res)
    assert len(sess.ctx.func_calls) == n_calls
