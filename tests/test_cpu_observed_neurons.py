"""Host side of neurons unobserved on some trials, without a GPU: the observation table of _session._stack_observed, the zero-filled resident
copy of _session._stack_counts (NaN accepted in unobserved rows and nowhere else), the ValueError cases that must stop an experiment before
anything is uploaded, the count moments under a table, the refusals, and the C-ABI declaration of pgpfa_set_observed.
Every test prints the figure it measured before it asserts."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, Experiment


def _experiment(seed=0, q=5, lens=(8, 8, 8, 8), observed=None):
    rng = np.random.default_rng(seed)
    exp = Experiment([rng.poisson(1.5, size=(q, L)).astype(np.float64) for L in lens], 10.0)
    for r, o in (observed or {}).items():
        exp.data[r]['observed'] = np.asarray(o)
    return exp


def test_no_key_means_no_table_and_the_plain_stack():
    """absent from every trial: no table, and _stack_counts returns what it returned before (the equal path)"""
    from funs import _session
    exp = _experiment()
    assert _session._stack_observed(exp) is None
    Y, lens = _session._stack_counts(exp)
    assert np.array_equal(Y, np.stack([tr['Y'] for tr in exp.data]).astype(np.uint8)) and lens.tolist() == [8, 8, 8, 8]


def test_table_stacking_and_zero_filling():
    """trials without the key are fully observed; the resident copy holds zeros at unobserved rows, the caller's arrays stay as they were;
    together with ragged lengths the padding and the rows are both zero"""
    from funs import _session
    obs = {1: [1, 0, 1, 1, 0], 3: np.array([False, True, True, True, True])}
    exp = _experiment(lens=(8, 5, 8, 6), observed=obs)
    before = [tr['Y'].copy() for tr in exp.data]
    table = _session._stack_observed(exp)
    assert table.dtype == bool and table.shape == (4, 5)
    assert table.tolist() == [[True] * 5, [True, False, True, True, False], [True] * 5, [False, True, True, True, True]]
    Y, lens = _session._stack_counts(exp)
    assert Y.shape == (4, 5, 8) and Y.dtype == np.uint8 and lens.tolist() == [8, 5, 8, 6]
    for r, y in enumerate(before):
        assert np.array_equal(exp.data[r]['Y'], y)
        want = np.where(table[r][:, None], y, 0.0)
        assert np.array_equal(Y[r, :, :y.shape[1]], want) and not Y[r, :, y.shape[1]:].any()
    print('unobserved pairs: %d, counts zero-filled: %d' % (int((~table).sum()), int(sum(before[r][~table[r]].sum() for r in range(4)))))


def test_nan_is_accepted_in_unobserved_rows_only():
    from funs import _session
    exp = _experiment(observed={2: [1, 1, 0, 1, 1]})
    exp.data[2]['Y'][2, :] = np.nan
    Y, _ = _session._stack_counts(exp)
    assert Y.dtype == np.uint8 and not Y[2, 2].any()
    exp.data[2]['Y'][3, 4] = np.nan                        # an observed row: the stack stays float64, which the C-ABI rejects with the reason
    Y, _ = _session._stack_counts(exp)
    assert Y.dtype == np.float64 and np.isnan(Y[2, 3, 4])


def test_invalid_tables_raise_value_error_before_any_upload(monkeypatch):
    """a wrong shape, a trial without an observed neuron, a neuron never observed: ValueError from the host - no context is created"""
    from funs import _hip, _session, inference

    def no_context(*a, **k):
        raise AssertionError('a device context was created for an invalid experiment')
    monkeypatch.setattr(_hip, 'Context', no_context)
    params = {'C': np.zeros((5, 2)), 'd': np.zeros(5), 'tau': np.ones(2) * 0.1}
    with pytest.raises(ValueError, match=r"trial 1: 'observed' must have shape \(ydim,\) = \(5,\)"):
        inference.laplace(_experiment(observed={1: [1, 0, 1]}), dict(params))
    with pytest.raises(ValueError, match='trial 2 has no observed neuron'):
        inference.laplace(_experiment(observed={2: [0, 0, 0, 0, 0]}), dict(params))
    never = {r: [1, 1, 1, 0, 1] for r in range(4)}
    with pytest.raises(ValueError, match='neuron 3 is observed on no trial'):
        _session.session_for(_experiment(observed=never), 2)
    with pytest.raises(ValueError, match=r'shape \(trials, ydim\) = \(4, 5\)'):
        _session.check_observed(np.ones((4, 4)), 4, 5)


def test_session_keeps_its_positional_signature():
    import inspect
    from funs import _session
    assert list(inspect.signature(_session.Session.__init__).parameters) == ['self', 'Y', 'p', 'bin_ms', 'lengths', 'observed']


def _fake_session(observed, lengths, T):
    from funs import _session
    sess = object.__new__(_session.Session)
    sess.R, sess.q, sess.T, sess.p = observed.shape[0], observed.shape[1], T, 2
    sess.lengths = lengths
    sess.observed = observed
    return sess


def test_refusals_name_the_unobserved_neurons():
    from funs import _session
    table = np.ones((3, 4), dtype=bool)
    table[1, 2] = False
    sess = _fake_session(table, None, 6)
    with pytest.raises(NotImplementedError, match='unobserved neurons'):
        sess.refuse_tables('dualVariational')
    with pytest.raises(NotImplementedError, match='unobserved neurons'):
        sess.refuse_tables('dualVariational', allow=('lengths', 'observed_bins'))
    sess.refuse_tables('dualVariational', allow=('observed',))
    sess.observed = None
    sess.refuse_tables('dualVariational')
    plain = object.__new__(_session.Session)               # a session object made without __init__ (the fakes of the other CPU tests)
    plain.refuse_tables('anything')


def test_count_moments_under_a_table():
    """util._observed_moments on exact integer sums of a zero-filled raster.  mean_i = s_i / n_i is np.mean over the neuron's own samples;
    cov_ii is np.var(ddof=1) over them; for a pair with the SAME observation pattern cov_ij is np.cov on the co-observed samples (the formula
    centres a pair at the neurons' overall means, so for pairs with different patterns it is np.cov only up to the difference of the overall
    and the co-observed means: those are held to the formula restated entry by entry); cov_ij = 0 where fewer than 2 samples are co-observed.
    Tolerance 1e-12 relative: the sums are exact integers, the formula is a handful of FP64 operations."""
    from funs import util
    rng = np.random.default_rng(3)
    R, q, T = 6, 6, 9
    lens = np.array([9, 5, 9, 7, 9, 1], dtype=np.int32)
    table = np.ones((R, q), dtype=bool)
    table[1, [0, 1]] = False                               # neurons 0 and 1 share a pattern
    table[3, [0, 1, 4]] = False
    table[0:5, 5] = False                                  # neuron 5: observed on trial 5 only (1 bin): n_55 = 1 < 2
    table[5, 4] = False
    Y = np.zeros((R, q, T))
    for r in range(R):
        Y[r, :, :lens[r]] = rng.poisson(2.0, size=(q, lens[r]))
        Y[r, ~table[r]] = 0
    s = Y.sum(axis=(0, 2))
    S = np.einsum('rit,rjt->ij', Y, Y)
    mean, cov = util._observed_moments(s, S, table, lens, T, np.arange(R))
    worst = 0.0
    samples = lambda i, j: np.concatenate([Y[r, [i, j], :lens[r]] for r in range(R) if table[r, i] and table[r, j]] or [np.zeros((2, 0))], axis=1)
    for i in range(q):
        own = samples(i, i)[0]
        assert mean[i] == own.sum() / own.size
        if own.size >= 2:
            worst = max(worst, abs(cov[i, i] - np.var(own, ddof=1)) / np.var(own, ddof=1))
        for j in range(q):
            co = samples(i, j)
            n_ij = co.shape[1]
            if n_ij < 2:
                assert cov[i, j] == 0.0
                continue
            n_i, n_j = samples(i, i).shape[1], samples(j, j).shape[1]
            restated = (S[i, j] - s[i] * s[j] * n_ij / (n_i * n_j)) / (n_ij - 1)
            worst = max(worst, abs(cov[i, j] - restated) / max(abs(restated), 1.0))
            if np.array_equal(table[:, i], table[:, j]):
                ref = np.cov(co)[0, 1]
                worst = max(worst, abs(cov[i, j] - ref) / max(abs(ref), 1.0))
    print('count moments under a table: worst relative deviation %.2e; cov[5,5] = %g (one sample)' % (worst, cov[5, 5]))
    assert worst <= 1e-12 and cov[5, 5] == 0.0 and np.array_equal(cov, cov.T)
    # everything observed: the formula is the plain one
    full = np.ones((R, q), dtype=bool)
    Yf = rng.poisson(2.0, size=(R, q, T)).astype(np.float64)
    sf, Sf = Yf.sum(axis=(0, 2)), np.einsum('rit,rjt->ij', Yf, Yf)
    m2, c2 = util._observed_moments(sf, Sf, full, None, T, np.arange(R))
    raster = Yf.transpose(1, 0, 2).reshape(q, -1)
    assert np.allclose(m2, raster.mean(axis=1), rtol=1e-14) and np.allclose(c2, np.cov(raster), rtol=1e-12, atol=1e-14)


def test_header_binding_and_library_agree_on_pgpfa_set_observed():
    import __graft_entry__ as ge
    ge.build()
    from funs import _hip
    lib = _hip.load_library()
    header = open(os.path.join(ROOT, 'include', 'pgpfa.h')).read()
    assert re.search(r'int\s+pgpfa_set_observed\s*\(\s*pgpfa_ctx\s*\*\s*ctx\s*,\s*const\s+uint8_t\s*\*\s*obs', header)
    assert 'pgpfa_set_observed' in _hip.EXPORTED_SYMBOLS and hasattr(lib, 'pgpfa_set_observed')
    assert '"observed_set"' in header and '"last_cd_unobserved_neurons"' in header
    assert hasattr(_hip.Context, 'set_observed')
