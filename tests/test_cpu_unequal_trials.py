"""Host side of trials of unequal length, without a GPU: the padding and lengths of _session._stack_counts, the cut of the lazy infRes /
lapOptimRes entries to a trial's own bins (on a fake context), the ValueError cases that must stop an experiment before anything is uploaded,
and the C-ABI declaration of pgpfa_set_trial_lengths."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, Experiment


def _ragged(seed=0, q=4, lens=(10, 5, 7, 10)):
    rng = np.random.default_rng(seed)
    return [rng.poisson(1.5, size=(q, L)).astype(np.float64) for L in lens]


def test_stack_counts_pads_with_zeros_and_returns_the_lengths():
    from funs import _session
    Ys = _ragged()
    Y, lens = _session._stack_counts(Experiment(Ys, 10.0))
    assert Y.shape == (4, 4, 10) and Y.dtype == np.uint8
    assert lens.dtype == np.int32 and lens.tolist() == [10, 5, 7, 10]
    for r, y in enumerate(Ys):
        assert np.array_equal(Y[r, :, :y.shape[1]], y) and not Y[r, :, y.shape[1]:].any()
    # counts above 255 still choose the two-byte form, non-integers still go to the C-ABI as float64 (which rejects them with the reason)
    Ys[1][0, 0] = 300
    assert _session._stack_counts(Experiment(Ys, 10.0))[0].dtype == np.uint16
    Ys[1][0, 0] = 0.5
    assert _session._stack_counts(Experiment(Ys, 10.0))[0].dtype == np.float64


def test_stack_counts_of_equal_trials_is_the_plain_stack():
    from funs import _session
    Ys = _ragged(lens=(9, 9, 9))
    Y, lens = _session._stack_counts(Experiment(Ys, 10.0))
    assert np.array_equal(Y, np.stack(Ys).astype(np.uint8)) and Y.dtype == np.uint8 and lens.tolist() == [9, 9, 9]


def test_invalid_experiments_raise_value_error_before_any_upload(monkeypatch):
    """a trial without bins, trials with different numbers of neurons: ValueError from the host - no context is created (the constructor
    would raise HipBackendError on a machine without a GPU, or upload on one with)"""
    from funs import _hip, _session, inference

    def no_context(*a, **k):
        raise AssertionError('a device context was created for an invalid experiment')
    monkeypatch.setattr(_hip, 'Context', no_context)
    params = {'C': np.zeros((4, 2)), 'd': np.zeros(4), 'tau': np.ones(2) * 0.1}
    empty = _ragged()
    empty[2] = np.zeros((4, 0))
    with pytest.raises(ValueError, match='trial 2 has no bins'):
        inference.laplace(Experiment(empty, 10.0), dict(params))
    mixed = _ragged()
    mixed[1] = np.zeros((5, 5))
    with pytest.raises(ValueError, match='trial 1 has 5 neurons'):
        _session.session_for(Experiment(mixed, 10.0), 2)
    flat = _ragged()
    flat[3] = np.zeros(10)
    with pytest.raises(ValueError, match='trial 3'):
        _session.session_for(Experiment(flat, 10.0), 2)


class _FakeCtx:
    """padded device results with recognisable entries: value = 1000 trial + position"""

    def __init__(self, R, p, T):
        self.R, self.p, self.T = R, p, T

    def post_mean(self, idx):
        return np.stack([1000.0 * t + np.arange(self.p * self.T, dtype=np.float64).reshape(self.p, self.T) for t in idx])

    def post_vsm(self, idx):
        return np.stack([1000.0 * t + np.arange(self.T * self.p * self.p, dtype=np.float64).reshape(self.T, self.p, self.p) for t in idx])

    def post_vsmgp(self, idx):
        return np.stack([1000.0 * t + np.arange(self.T * self.T * self.p, dtype=np.float64).reshape(self.T, self.T, self.p) for t in idx])

    def post_cov(self, trial):
        n = self.p * self.T
        return 1000.0 * trial + np.arange(n * n, dtype=np.float64).reshape(n, n)


def _fake_session(lens, p, T):
    from funs import _session
    sess = object.__new__(_session.Session)
    sess.R, sess.q, sess.T, sess.p = len(lens), 3, T, p
    sess.lengths = None if lens is None or all(v == T for v in lens) else np.asarray(lens, dtype=np.int32)
    sess.ctx = _FakeCtx(sess.R, p, T)
    sess.post_stamp = sess.mode_stamp = 1
    sess.trial_stamp = np.ones(sess.R, dtype=np.int64)
    return sess


@pytest.mark.parametrize('bulk', [False, True], ids=['lazy', 'materialize'])
def test_lazy_entries_are_cut_to_the_trials_own_bins(bulk):
    from funs import _session
    p, T, lens = 2, 6, [6, 3, 5, 4]
    sess = _fake_session(lens, p, T)
    tid = np.array([2, 1, 0], dtype=np.int32)                      # a minibatch: entry i belongs to trial tid[i]
    res = _session.DeviceInfRes(sess, tid, (0, 3))
    if bulk:
        res.materialize(('post_mean', 'post_vsm', 'post_vsmGP'))
    opt = _session.DeviceOptimRes(sess, tid)
    for i, t in enumerate(tid):
        L = lens[t]
        m, v, g, c = res['post_mean'][i], res['post_vsm'][i], res['post_vsmGP'][i], res['post_cov'][i]
        assert m.shape == (p, L) and v.shape == (L, p, p) and g.shape == (L, L, p) and c.shape == (p * L, p * L)
        assert np.array_equal(m, sess.ctx.post_mean([t])[0][:, :L])
        assert np.array_equal(v, sess.ctx.post_vsm([t])[0][:L])
        assert np.array_equal(g, sess.ctx.post_vsmgp([t])[0][:L, :L])
        full = sess.ctx.post_cov(t).reshape(p, T, p, T)
        assert np.array_equal(c, full[:, :L, :, :L].reshape(p * L, p * L))
        assert opt[i].shape == (p * L,) and np.array_equal(opt[i], m.reshape(-1))


def test_equal_trials_get_the_device_arrays_unchanged():
    from funs import _session
    sess = _fake_session([6, 6, 6], 2, 6)
    assert sess.lengths is None
    res = _session.DeviceInfRes(sess, np.arange(3, dtype=np.int32), (0, 3))
    assert res['post_mean'][1].shape == (2, 6) and res['post_cov'][2].shape == (12, 12) and res['post_vsmGP'][0].shape == (6, 6, 2)
    sess.refuse_tables('anything')                                  # no table, no refusal


def test_host_modes_of_a_trials_own_length_are_padded_with_zeros():
    p, T, lens = 2, 6, [6, 3, 5]
    sess = _fake_session(lens, p, T)
    rows = [np.arange(1, p * L + 1, dtype=np.float64) for L in lens]
    X = sess.pad_modes([0, 1, 2], rows).reshape(3, p, T)
    for r, L in enumerate(lens):
        assert np.array_equal(X[r, :, :L], rows[r].reshape(p, L)) and not X[r, :, L:].any()
    # an entry may also come padded already; any other size is refused
    assert np.array_equal(sess.pad_modes([1], [np.ones(p * T)]), np.ones((1, p * T)))
    with pytest.raises(ValueError, match='trial 1 has 3 bins'):
        sess.pad_modes([1], [np.ones(p * 4)])
    with pytest.raises(NotImplementedError, match='trials of unequal length'):
        sess.refuse_tables('dualVariational')
    with pytest.raises(NotImplementedError, match='trials of unequal length'):
        sess.refuse_tables('dualVariational', allow=('observed', 'observed_bins'))
    sess.refuse_tables('dualVariational', allow=('lengths',))


def test_header_binding_and_library_agree_on_the_new_entry_point():
    import __graft_entry__ as ge
    ge.build()
    from funs import _hip
    lib = _hip.load_library()
    header = open(os.path.join(ROOT, 'include', 'pgpfa.h')).read()
    assert re.search(r'int\s+pgpfa_set_trial_lengths\s*\(\s*pgpfa_ctx\s*\*\s*ctx\s*,\s*const\s+int32_t\s*\*\s*len', header)
    assert 'pgpfa_set_trial_lengths' in _hip.EXPORTED_SYMBOLS and hasattr(lib, 'pgpfa_set_trial_lengths')
    assert '"trial_lengths_set"' in header
    assert hasattr(_hip.Context, 'set_trial_lengths')
