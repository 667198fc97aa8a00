"""Per-bin observation masks (pgpfa_set_observed_bins, experiment.data[r]['observedBins']), the part that needs no GPU.

The oracle cannot take an entry mask, so this file carries the yardstick of test_gpu_observed_bins.py: a structured numpy restatement of the
Laplace problem in which only live entries carry a likelihood term - objective sum_live (exp h - y h) + prior, gradient, Hessian with
W_t = sum_{n live at t} e_nt c_n c_n^T - a dense Newton on it and the posterior blocks from the inverse Hessian.  The first test pins that
restatement to the oracle's big-matrix forms with the columns of dead entries deleted.  The rest is the host side: the table of
_session._stack_observed_bins, the zero-filled resident copy, ValueError before any upload, live_mask, the count moments, the speckled subset,
the binding.  Every test prints the figure it measured before it asserts."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, Experiment, load_golden
from oracle import pgpfa_oracle as orc

BIN_MS = 10.0


# ---- the yardstick: the Laplace problem over live entries, plain FP64 numpy ---------------------------------------------------------------------
def masked_nlp(X, Y, live, C, d, Kinv):
    """sum over live entries of exp(h) - y h, plus the prior 1/2 sum_k x_k^T K_k^-1 x_k; h = C X + d"""
    h = C @ X + d[:, None]
    return float(np.where(live, np.exp(h) - np.where(live, Y, 0.0) * h, 0.0).sum() + 0.5 * np.einsum('kt,kts,ks->', X, Kinv, X))


def masked_grad(X, Y, live, C, d, Kinv):
    """(p, T): C^T [live (exp(h) - y)] + K_k^-1 x_k"""
    h = C @ X + d[:, None]
    return C.T @ np.where(live, np.exp(h) - np.where(live, Y, 0.0), 0.0) + np.einsum('kts,ks->kt', Kinv, X)


def masked_hess(X, live, C, d, Kinv):
    """dense, latent-major: H[(k,t),(l,s)] = [t == s] W_t[k,l] + [k == l] K_k^-1[t,s], W_t = sum_{n live at t} e_nt c_n c_n^T"""
    p, T = X.shape
    e = np.where(live, np.exp(C @ X + d[:, None]), 0.0)
    W = np.einsum('nk,nt,nl->tkl', C, e, C)
    H = np.zeros((p, T, p, T))
    ar = np.arange(T)
    for k in range(p):
        H[k, :, k, :] += Kinv[k]
        for l in range(p):
            H[k, ar, l, ar] += W[:, k, l]
    return H.reshape(p * T, p * T)


def masked_laplace(Y, live, params, bin_ms=BIN_MS, gtol=1e-10):
    """Dense Newton (halving line search) from x = 0 on the model with only the live entries of Y (q, T), to a gradient max-norm of gtol at most.
    Returns a dict: post_mean (p, T), post_vsm (T, p, p), post_vsmGP (T, T, p), nlp (the objective at the mode), logZ (the Laplace log
    evidence -nlp - (log det H + log det K) / 2), grad (the gradient max-norm reached)."""
    C, d = np.asarray(params['C'], dtype=np.float64), np.asarray(params['d'], dtype=np.float64).reshape(-1)
    live = np.asarray(live, dtype=bool)
    Y = np.where(live, np.asarray(Y, dtype=np.float64), 0.0)
    p, T = C.shape[1], Y.shape[1]
    K = orc.make_K(params['tau'], T, bin_ms)
    Kinv = np.linalg.inv(K)
    X = np.zeros((p, T))
    f = masked_nlp(X, Y, live, C, d, Kinv)
    for _ in range(100):
        g = masked_grad(X, Y, live, C, d, Kinv)
        if np.max(np.abs(g)) <= gtol:
            break
        step = -np.linalg.solve(masked_hess(X, live, C, d, Kinv), g.reshape(-1)).reshape(p, T)
        a = 1.0
        while True:
            f_new = masked_nlp(X + a * step, Y, live, C, d, Kinv)
            # (close to the mode the decrease of f drowns in its rounding: a step that shrinks the gradient is accepted as well)
            if f_new <= f + 1e-4 * a * float(np.sum(g * step)) or a < 1e-10 or \
                    np.max(np.abs(masked_grad(X + a * step, Y, live, C, d, Kinv))) < 0.5 * np.max(np.abs(g)):
                break
            a *= 0.5
        X, f = X + a * step, f_new
    g = float(np.max(np.abs(masked_grad(X, Y, live, C, d, Kinv))))
    assert g <= gtol, 'the reference Newton stopped at a gradient of %.2e' % g
    H = masked_hess(X, live, C, d, Kinv)
    vsmGP, vsm = orc.marginal_blocks(np.linalg.inv(H), p, T)
    sign, ldH = np.linalg.slogdet(H)
    ldK = sum(np.linalg.slogdet(K[k])[1] for k in range(p))
    assert sign == 1.0
    return {'post_mean': X, 'post_vsm': vsm, 'post_vsmGP': vsmGP, 'nlp': masked_nlp(X, Y, live, C, d, Kinv), 'logZ': -f - 0.5 * (ldH + ldK), 'grad': g}


def pattern_masks(R, q, T, seed=0):
    """(R, q, T) booleans, True = live: the eight patterns in turn over the trials.  1 all live | 2 a seeded 20 % speckle | 3 neurons {0, 15, 16,
    q-1} x bins {0, 15, 16, 63, 64, T-1} dead (those that exist) | 4 neuron 3 dead on the whole trial, neuron 17 on bins [16, 32) | 5 every neuron
    dead on the second 64-bin block (T > 64) or on [16, 32) | 6 the single live entry (17, 33) | 7 a checkerboard, (n + t) even live | 8 t < T/2 and
    n even live (what lengths plus 'observed' can express)."""
    assert R >= 8 and q > 17 and T > 33
    n, t = np.arange(q)[:, None], np.arange(T)[None, :]
    rng = np.random.default_rng(seed + 1000 * q + T)
    rows = [np.ones((q, T), bool), rng.random((q, T)) >= 0.2,
            ~(np.isin(n, [0, 15, 16, q - 1]) & np.isin(t, [b for b in (0, 15, 16, 63, 64, T - 1) if b < T])),
            ~((n == 3) | ((n == 17) & (t >= 16) & (t < 32))),
            np.broadcast_to(~((t >= 64) & (t < 128)) if T > 64 else ~((t >= 16) & (t < 32)), (q, T)),
            (n == 17) & (t == 33), (n + t) % 2 == 0, (t < T // 2) & (n % 2 == 0)]
    live = np.stack([np.array(rows[r % 8]) for r in range(R)])
    assert live.any(axis=(1, 2)).all() and live.any(axis=(0, 2)).all()
    return live


# ---- 1. the restatement against the oracle's big-matrix forms ----------------------------------------------------------------------------------
def test_restatement_equals_the_oracle_with_dead_columns_deleted():
    """Config 1's shape (30 x 3 x 100), a 20 % speckle plus a dead window: orc.nlp_big / nlp_big_grad / nlp_big_hess with the columns n T + t of
    C_big and the matching entries of d_big and ybar deleted, at two random x.  Plain FP64 re-orderings of the same sums: objective 1e-13,
    gradient and Hessian 1e-12 relative."""
    g = load_golden('c1_dataset.npz')
    C, d, tau = g['init_C'].astype(np.float64), g['init_d'].astype(np.float64).reshape(-1), g['init_tau']
    Y = g['Y'][0].astype(np.float64)
    q, T = Y.shape
    p = C.shape[1]
    rng = np.random.default_rng(7)
    live = rng.random((q, T)) >= 0.2
    live[4, 10:40] = False
    K = orc.make_K(tau, T, BIN_MS)
    Kinv = np.linalg.inv(K)
    K_bigInv = orc.make_K_big(Kinv)
    C_big, d_big = orc.make_Cd_big(C, d, T)
    keep = live.reshape(-1)                                    # column n T + t
    Cb, db, yb = C_big[:, keep], d_big[keep], Y.reshape(-1)[keep]
    for trial in range(2):
        X = 0.5 * rng.standard_normal((p, T))
        x = X.reshape(-1)
        f_ref, g_ref, H_ref = orc.nlp_big(x, yb, Cb, db, K_bigInv), orc.nlp_big_grad(x, yb, Cb, db, K_bigInv), orc.nlp_big_hess(x, yb, Cb, db, K_bigInv)
        e_f = abs(masked_nlp(X, Y, live, C, d, Kinv) - f_ref) / abs(f_ref)
        e_g = float(np.max(np.abs(masked_grad(X, Y, live, C, d, Kinv).reshape(-1) - g_ref)) / np.max(np.abs(g_ref)))
        e_h = float(np.max(np.abs(masked_hess(X, live, C, d, Kinv) - H_ref)) / np.max(np.abs(H_ref)))
        print('restatement against the oracle, x %d: objective %.2e (1e-13), gradient %.2e (1e-12), Hessian %.2e (1e-12); %d of %d entries live'
              % (trial, e_f, e_g, e_h, int(keep.sum()), keep.size))
        assert e_f <= 1e-13 and e_g <= 1e-12 and e_h <= 1e-12


def test_reference_newton_reaches_its_gradient_limit():
    """masked_laplace on a small trial: gradient at most 1e-10, blocks symmetric, and with every entry live it is the oracle's exact Laplace"""
    params, Ys, _ = orc.synth_dataset(18, 2, 40, 1, seed=3)
    live = pattern_masks(8, 18, 40)[1]
    res = masked_laplace(Ys[0], live, params)
    ref, nll, _ = orc.laplace([np.asarray(Ys[0], dtype=np.float64)], params, BIN_MS, mode='exact', return_cov=False)
    full = masked_laplace(Ys[0], np.ones_like(live), params)
    e_m = float(np.max(np.abs(full['post_mean'] - ref['post_mean'][0])))
    e_v = float(np.max(np.abs(full['post_vsm'] - ref['post_vsm'][0])) / np.max(np.abs(ref['post_vsm'][0])))
    print('reference Newton: gradient %.2e (speckle), %.2e (all live); all live against orc.laplace: modes %.2e, post_vsm %.2e, objective %.2e'
          % (res['grad'], full['grad'], e_m, e_v, abs(full['nlp'] + nll) / abs(nll)))
    assert res['grad'] <= 1e-10 and e_m <= 1e-9 and e_v <= 1e-9 and abs(full['nlp'] + nll) <= 1e-10 * abs(nll)     # (orc.laplace returns minus the objective)
    assert np.allclose(res['post_vsm'], res['post_vsm'].transpose(0, 2, 1), atol=1e-14)


def test_patterns_keep_every_trial_and_neuron_alive():
    for q, T in ((30, 100), (40, 176), (35, 64), (50, 48)):
        live = pattern_masks(8, q, T)
        assert live.shape == (8, q, T) and live[0].all() and live[5].sum() == 1 and live[5, 17, 33]
        assert 0.15 < 1.0 - live[1].mean() < 0.25 and not live[3, 3].any() and not live[3, 17, 16:32].any() and live[3, 17, 32]


# ---- 2. host-side stacking and validation ---------------------------------------------------------------------------------------------------------
def _experiment(seed=0, q=5, lens=(8, 8, 8, 8), bins=None, observed=None):
    rng = np.random.default_rng(seed)
    exp = Experiment([rng.poisson(1.5, size=(q, L)).astype(np.float64) for L in lens], 10.0)
    for r, b in (bins or {}).items():
        exp.data[r]['observedBins'] = np.asarray(b)
    for r, o in (observed or {}).items():
        exp.data[r]['observed'] = np.asarray(o)
    return exp


def test_no_key_means_no_table_and_the_plain_stack():
    from funs import _session
    exp = _experiment()
    assert _session._stack_observed_bins(exp) is None
    Y, lens = _session._stack_counts(exp)
    assert np.array_equal(Y, np.stack([tr['Y'] for tr in exp.data]).astype(np.uint8)) and lens.tolist() == [8, 8, 8, 8]


def test_table_stacking_and_zero_filling():
    """trials without the key are fully recorded inside their own bins; the resident copy holds zeros at dead entries (NaN accepted there and
    nowhere else), the caller's arrays stay as they were; behind a shorter trial's bins the stacked table is False"""
    from funs import _session
    b1 = np.ones((5, 5), dtype=bool)
    b1[2, 1:4] = False
    b3 = np.ones((5, 6), dtype=int)
    b3[0, 0] = 0
    b3[4, 5] = 0
    exp = _experiment(lens=(8, 5, 8, 6), bins={1: b1, 3: b3})
    exp.data[1]['Y'][2, 2] = np.nan
    before = [tr['Y'].copy() for tr in exp.data]
    table = _session._stack_observed_bins(exp)
    assert table.dtype == bool and table.shape == (4, 5, 8)
    assert table[0].all() and table[2].all() and np.array_equal(table[1, :, :5], b1) and not table[1, :, 5:].any()
    assert np.array_equal(table[3, :, :6], b3 != 0) and not table[3, :, 6:].any()
    Y, lens = _session._stack_counts(exp)
    assert Y.shape == (4, 5, 8) and Y.dtype == np.uint8 and lens.tolist() == [8, 5, 8, 6]
    for r, y in enumerate(before):
        assert np.array_equal(exp.data[r]['Y'], y, equal_nan=True)
        L = y.shape[1]
        assert np.array_equal(Y[r, :, :L], np.where(table[r, :, :L], y, 0.0)) and not Y[r, :, L:].any()
    exp.data[1]['Y'][0, 0] = np.nan                           # a live entry: the stack stays float64, which the C-ABI rejects with the reason
    Y, _ = _session._stack_counts(exp)
    assert Y.dtype == np.float64 and np.isnan(Y[1, 0, 0])
    print('dead entries: %d of %d inside the trials' % (int((~table).sum() - 5 * 3 - 5 * 2), 5 * (8 + 5 + 8 + 6)))


def test_invalid_tables_raise_value_error_before_any_upload(monkeypatch):
    from funs import _hip, _session, inference

    def no_context(*a, **k):
        raise AssertionError('a device context was created for an invalid experiment')
    monkeypatch.setattr(_hip, 'Context', no_context)
    params = {'C': np.zeros((5, 2)), 'd': np.zeros(5), 'tau': np.ones(2) * 0.1}
    with pytest.raises(ValueError, match=r"trial 1: 'observedBins' must have the shape of 'Y', \(ydim, T\) = \(5, 8\)"):
        inference.laplace(_experiment(bins={1: np.ones((5, 7))}), dict(params))
    with pytest.raises(ValueError, match='trial 2 has no live entry'):
        inference.laplace(_experiment(bins={2: np.zeros((5, 8))}), dict(params))
    never = np.ones((5, 8), dtype=bool)
    never[3] = False
    with pytest.raises(ValueError, match='neuron 3 has no live entry on any trial'):
        _session.session_for(_experiment(bins={r: never for r in range(4)}), 2)
    # together with 'observed': the bin table leaves trial 0 only neuron 1, which 'observed' hides
    only1 = np.zeros((5, 8), dtype=bool)
    only1[1] = True
    with pytest.raises(ValueError, match='trial 0 has no live entry'):
        _session.session_for(_experiment(bins={0: only1}, observed={0: [1, 0, 1, 1, 1]}), 2)
    with pytest.raises(ValueError, match=r'shape \(trials, ydim, T\) = \(4, 5, 8\)'):
        _session.compose_observed_bins(np.ones((4, 5, 7)), None, None, 4, 5, 8)


class _FakeContext:
    calls = []

    def __init__(self, *a, **k):
        type(self).calls.append(('create',))

    def upload_counts(self, Y):
        type(self).calls.append(('counts', Y.copy()))

    def set_trial_lengths(self, lens):
        type(self).calls.append(('lengths', np.array(lens)))

    def set_observed(self, table):
        type(self).calls.append(('observed', np.array(table)))

    def set_observed_bins(self, table):
        type(self).calls.append(('bins', None if table is None else np.array(table)))


def test_an_all_true_table_is_dropped_and_a_real_one_is_passed_on(monkeypatch):
    """A table that marks every entry inside the lengths and 'observed' as recorded sets nothing (as Session.__init__ drops an all-true
    'observed'); one with a dead entry reaches the context after the counts, as (R, q, T) booleans"""
    from funs import _hip, _session
    monkeypatch.setattr(_hip, 'Context', _FakeContext)
    monkeypatch.setattr(_session.WORLD, 'enabled', False)
    _FakeContext.calls = []
    exp = _experiment(lens=(8, 5, 8, 6), bins={1: np.ones((5, 5)), 2: np.ones((5, 8), dtype=bool)}, observed={0: [1, 1, 0, 1, 1]})
    sess, _ = _session.session_for(exp, 2)
    kinds = [c[0] for c in _FakeContext.calls]
    assert kinds == ['create', 'counts', 'lengths', 'observed'] and sess.observed_bins is None and sess.live_mask([0]).sum() == 4 * 8
    _FakeContext.calls = []
    b = np.ones((5, 8), dtype=bool)
    b[2, 3] = False
    exp = _experiment(bins={2: b})
    sess, _ = _session.session_for(exp, 2)
    kinds = [c[0] for c in _FakeContext.calls]
    assert kinds == ['create', 'counts', 'bins'] and sess.observed_bins.shape == (4, 5, 8) and sess.observed_bins.sum() == 4 * 5 * 8 - 1
    assert _FakeContext.calls[1][1][2, 2, 3] == 0 and np.array_equal(_FakeContext.calls[2][1], sess.observed_bins)


def test_session_keeps_its_positional_signature():
    import inspect
    from funs import _session
    assert list(inspect.signature(_session.Session.__init__).parameters) == ['self', 'Y', 'p', 'bin_ms', 'lengths', 'observed']
    assert list(inspect.signature(_session.Session.set_observed_bins).parameters) == ['self', 'table']


def _fake_session(R, q, T, lengths=None, observed=None, bins=None):
    from funs import _session
    sess = object.__new__(_session.Session)
    sess.R, sess.q, sess.T, sess.p = R, q, T, 2
    sess.lengths, sess.observed, sess.observed_bins = lengths, observed, bins
    return sess


def test_live_mask_composes_the_three_tables():
    rng = np.random.default_rng(1)
    R, q, T = 4, 5, 9
    lens = np.array([9, 4, 9, 7], dtype=np.int32)
    obs = np.ones((R, q), dtype=bool)
    obs[2, 1] = False
    bins = rng.random((R, q, T)) > 0.3
    sess = _fake_session(R, q, T, lens, obs, bins)
    want = bins & obs[:, :, None] & (np.arange(T)[None, None, :] < lens[:, None, None])
    got = sess.live_mask([3, 1])
    assert got.shape == (2, q * T) and np.array_equal(got.reshape(2, q, T), want[[3, 1]]) and np.array_equal(sess.live_entries(), want)
    assert np.array_equal(_fake_session(R, q, T, None, None, bins).live_mask([0, 1, 2, 3]).reshape(R, q, T), bins)
    assert _fake_session(R, q, T).live_mask([0]) is None and _fake_session(R, q, T).live_entries().all()
    plain = object.__new__(type(sess))                     # a session object made without __init__ (the fakes of the other CPU tests)
    plain.lengths, plain.R, plain.q, plain.T = None, R, q, T
    assert plain.live_mask([0]) is None


def test_refusals_name_the_per_bin_table():
    from funs import _session
    bins = np.ones((3, 4, 6), dtype=bool)
    bins[1, 2, 3] = False
    sess = _fake_session(3, 4, 6, bins=bins)
    with pytest.raises(NotImplementedError, match='per-bin'):
        sess.refuse_tables('dualVariational')
    with pytest.raises(NotImplementedError, match='per-bin'):
        sess.refuse_tables('dualVariational', allow=('lengths', 'observed'))
    sess.refuse_tables('dualVariational', allow=('observed_bins',))
    sess.observed_bins = None
    sess.refuse_tables('dualVariational')
    object.__new__(_session.Session).refuse_tables('anything')


# ---- 3. moments, hold-out subset ------------------------------------------------------------------------------------------------------------------
def test_count_moments_under_a_bin_table_against_a_brute_force_loop():
    """util._live_moments on exact integer sums of a zero-filled raster against loops over the entries: n_i live entries, n_ij co-live entries,
    mean_i = s_i / n_i, cov_ij = (S_ij - s_i s_j n_ij / (n_i n_j)) / (n_ij - 1), 0 where n_ij < 2; cov_ii is np.var(ddof=1) over the neuron's live
    samples.  1e-12 relative: the sums are exact integers, the formula a handful of FP64 operations."""
    from funs import util
    rng = np.random.default_rng(5)
    R, q, T = 5, 6, 11
    live = rng.random((R, q, T)) > 0.35
    live[:, 5] = False
    live[2, 5, 4] = True                                    # neuron 5: a single live entry
    Y = np.where(live, rng.poisson(2.0, size=(R, q, T)), 0).astype(np.float64)
    s, S = Y.sum(axis=(0, 2)), np.einsum('rit,rjt->ij', Y, Y)
    mean, cov = util._live_moments(s, S, live)
    worst = 0.0
    for i in range(q):
        n_i = sum(1 for r in range(R) for t in range(T) if live[r, i, t])
        own = np.array([Y[r, i, t] for r in range(R) for t in range(T) if live[r, i, t]])
        assert mean[i] == own.sum() / n_i
        if n_i >= 2:
            worst = max(worst, abs(cov[i, i] - np.var(own, ddof=1)) / np.var(own, ddof=1))
        for j in range(q):
            n_j = sum(1 for r in range(R) for t in range(T) if live[r, j, t])
            n_ij = sum(1 for r in range(R) for t in range(T) if live[r, i, t] and live[r, j, t])
            if n_ij < 2:
                assert cov[i, j] == 0.0
                continue
            S_ij = sum(Y[r, i, t] * Y[r, j, t] for r in range(R) for t in range(T) if live[r, i, t] and live[r, j, t])
            assert S_ij == S[i, j]                           # (dead entries hold zeros: the device's sums are the co-live sums)
            restated = (S_ij - s[i] * s[j] * n_ij / (n_i * n_j)) / (n_ij - 1)
            worst = max(worst, abs(cov[i, j] - restated) / max(abs(restated), 1.0))
    print('count moments under a bin table: worst relative deviation %.2e; cov[5,5] = %g (one sample)' % (worst, cov[5, 5]))
    assert worst <= 1e-12 and cov[5, 5] == 0.0 and np.array_equal(cov, cov.T)
    # a table that only whole (trial, neuron) rows and tails: the formulas of _observed_moments
    obs = rng.random((R, q)) > 0.3
    obs[0] = True
    lens = np.array([11, 6, 11, 9, 3])
    whole = obs[:, :, None] & (np.arange(T)[None, None, :] < lens[:, None, None])
    Yw = np.where(whole, Y, 0.0)
    sw, Sw = Yw.sum(axis=(0, 2)), np.einsum('rit,rjt->ij', Yw, Yw)
    m1, c1 = util._live_moments(sw, Sw, whole)
    m2, c2 = util._observed_moments(sw, Sw, obs, lens, T, np.arange(R))
    assert np.array_equal(m1, m2) and np.array_equal(c1, c2)


def test_the_held_out_subset_does_not_depend_on_the_width():
    """speckledHoldout is a function of the experiment and the seed: the same arrays on every call (what crossValidation hands every width),
    another seed gives another subset, entries the experiment did not record are never chosen, the fraction is about the one asked for"""
    from funs import util
    b = np.ones((5, 40), dtype=bool)
    b[1, 5:30] = False
    exp = _experiment(q=5, lens=(40, 40, 33, 40), bins={2: b[:, :33], 3: b}, observed={0: [1, 1, 1, 0, 1]})
    a1, a2, other = util.speckledHoldout(exp, 0.1, seed=4), util.speckledHoldout(exp, 0.1, seed=4), util.speckledHoldout(exp, 0.1, seed=5)
    assert all(np.array_equal(x, y) for x, y in zip(a1, a2)) and not all(np.array_equal(x, y) for x, y in zip(a1, other))
    assert [x.shape for x in a1] == [(5, 40), (5, 40), (5, 33), (5, 40)] and all(x.dtype == bool for x in a1)
    assert not a1[0][3].any() and not a1[2][1, 5:30].any() and not a1[3][1, 5:30].any()
    frac = sum(int(x.sum()) for x in a1) / float(5 * 153)
    print('speckled subset: %.3f of the entries at holdoutFraction = 0.1' % frac)
    assert 0.04 < frac < 0.16
    hidden = util._with_hidden_entries(exp, a1)
    assert hidden is not exp and 'observedBins' not in exp.data[0] and np.array_equal(hidden.data[3]['observedBins'], b & ~a1[3])
    assert np.array_equal(hidden.data[0]['observedBins'], ~a1[0]) and hidden.data[0]['Y'] is exp.data[0]['Y']
    with pytest.raises(ValueError, match='holdoutFraction'):
        util.speckledHoldout(exp, 1.0)


def test_score_entries_is_the_null_model_of_co_smoothing():
    """_score_entries against the formula written out: per neuron, lbar over ITS scored entries"""
    from funs import util
    rng = np.random.default_rng(2)
    y = [rng.poisson(1.0, size=(3, 7)).astype(np.float64) for _ in range(2)]
    lam = [rng.uniform(0.3, 2.0, size=(3, 7)) for _ in range(2)]
    sc = [rng.random((3, 7)) > 0.4 for _ in range(2)]
    total, per, n = util._score_entries(y, lam, sc)
    ll, spikes = np.zeros(3), np.zeros(3)
    for i in range(3):
        ys = np.concatenate([a[i][m[i]] for a, m in zip(y, sc)])
        ls = np.concatenate([a[i][m[i]] for a, m in zip(lam, sc)])
        lbar = ys.mean()
        ll[i] = np.sum(ys * np.log(ls) - ls) - np.sum(ys * np.log(lbar) - lbar)
        spikes[i] = ys.sum()
    assert n == sum(int(m.sum()) for m in sc)
    assert abs(total - ll.sum() / (np.log(2) * spikes.sum())) <= 1e-13 and np.max(np.abs(per - ll / (np.log(2) * spikes))) <= 1e-13


# ---- 4. the binding --------------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_pgpfa_set_observed_bins():
    import __graft_entry__ as ge
    ge.build()
    from funs import _hip, _session, util
    lib = _hip.load_library()
    header = open(os.path.join(ROOT, 'include', 'pgpfa.h')).read()
    assert re.search(r'int\s+pgpfa_set_observed_bins\s*\(\s*pgpfa_ctx\s*\*\s*ctx\s*,\s*const\s+uint8_t\s*\*\s*live', header)
    assert 'pgpfa_set_observed_bins' in _hip.EXPORTED_SYMBOLS and hasattr(lib, 'pgpfa_set_observed_bins')
    assert '"observed_bins_set"' in header
    assert hasattr(_hip.Context, 'set_observed_bins') and hasattr(_session.Session, 'refuse_tables') and hasattr(util, 'binHoldout')
