"""Host side of the latent posterior at arbitrary time points, without a GPU: header, binding and library agree on pgpfa_posterior_at, the unit is
part of the build, and what util.posteriorAt does around the device call - one grid or one per trial, the shape errors, a time that is not finite
refused before anything reaches the device, the band, condition means over trials of unequal length with the inside-span rule - on a fake session
whose context answers with numbers that are easy to recompute."""
import ctypes as ct
import os
import re

import numpy as np
import pytest

from conftest import ROOT, Experiment


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
    assert re.search(r'int\s+pgpfa_posterior_at\s*\(\s*pgpfa_ctx\s*\*\s*ctx\s*,\s*int\s+n\s*,\s*const\s+int32_t\s*\*\s*idx\s*,\s*int\s+S\s*,\s*const\s+double\s*\*\s*times_ms'
                     r'\s*,\s*int\s+per_trial\s*,\s*double\s*\*\s*mean\s*,\s*double\s*\*\s*var\s*\)\s*;', bare)
    assert 'pgpfa_posterior_at' in hip.EXPORTED_SYMBOLS and hasattr(lib, 'pgpfa_posterior_at')
    c_double_p, c_int32_p = ct.POINTER(ct.c_double), ct.POINTER(ct.c_int32)
    assert list(lib.pgpfa_posterior_at.argtypes) == [ct.c_void_p, ct.c_int, c_int32_p, ct.c_int, c_double_p, ct.c_int, c_double_p, c_double_p]
    assert '"interp_chunk_trials"' in header
    assert hasattr(hip.Context, 'posterior_at')
    from funs import engine, util
    assert callable(util.posteriorAt) and callable(engine.PPGPFAfit.posteriorAt)


def test_the_unit_is_part_of_the_build():
    import __graft_entry__ as ge
    assert 'interp' in ge.UNITS
    assert os.path.exists(os.path.join(ge.CSRC, 'interp.hip')) and os.path.exists(os.path.join(ge.CSRC, 'interp.h'))


def test_null_context_is_refused_without_a_device(hip):
    lib = hip.load_library()
    t = np.zeros(1)
    out = np.zeros(1)
    assert lib.pgpfa_posterior_at(None, 1, None, 1, hip.dptr(t), 0, hip.dptr(out), None) != 0
    assert 'null context' in lib.pgpfa_last_error().decode()


# ---- util.posteriorAt around a fake device -------------------------------------------------------------------------------------------------------
class _FakeCtx:
    """posterior_at with a closed form in place of the GP algebra: mean = (trial + 1) * (latent + 1) * s / 100, var = 0.25 + (s / 1000)^2"""

    def __init__(self, p):
        self.p = p
        self.calls = []

    def posterior_at(self, times, idx=None, want=('mean', 'var')):
        tt = np.asarray(times, dtype=np.float64)
        self.calls.append((tt.shape, tuple(want)))
        n = len(idx)
        s = np.broadcast_to(tt, (n, tt.shape[-1]))
        mean = (np.asarray(idx)[:, None, None] + 1.0) * (np.arange(self.p)[None, :, None] + 1.0) * s[:, None, :] / 100.0
        var = np.broadcast_to(0.25 + (s[:, None, :] / 1000.0) ** 2, mean.shape).copy()
        return {k: v for k, v in (('mean', mean), ('var', var)) if k in want}


def _fake(monkeypatch, lens, T=8, q=3, p=2, bin_ms=20.0):
    from funs import _session
    R = len(lens)
    sess = object.__new__(_session.Session)
    sess.R, sess.q, sess.T, sess.p = R, q, T, p
    sess.lengths = None if all(v == T for v in lens) else np.asarray(lens, dtype=np.int32)
    sess.ctx = _FakeCtx(p)
    sess.post_stamp = sess.mode_stamp = 1
    sess.trial_stamp = np.ones(R, dtype=np.int64)
    sess.comm_ready = False
    sess.set_params = lambda params: None
    touched = []

    def session_for(experiment, xdim):
        touched.append(1)
        return sess, np.arange(R, dtype=np.int32)
    monkeypatch.setattr(_session, 'session_for', session_for)
    exp = Experiment([np.zeros((q, L)) for L in lens], bin_ms)
    params = {'C': np.ones((q, p)), 'd': -np.ones(q), 'tau': np.full(p, 0.1)}
    return sess, exp, params, _session.DeviceInfRes(sess, np.arange(R, dtype=np.int32), (0, R)), touched


def test_one_grid_for_all_trials_and_one_grid_per_trial(monkeypatch):
    from funs import util
    sess, exp, params, res, _ = _fake(monkeypatch, [8, 8, 8])
    times = np.array([-5.0, 0.0, 33.3, 140.0, 33.3])
    out = util.posteriorAt(params, exp, times, infRes=res, want=('mean', 'var'))
    assert sorted(out) == ['mean', 'times', 'var'] and out['mean'].shape == (3, 2, 5) and np.array_equal(out['times'], times)
    assert np.array_equal(out['mean'][2, 1], 3.0 * 2.0 * times / 100.0)
    assert sess.ctx.calls[-1] == ((5,), ('mean', 'var'))
    # event alignment: event_ms[r] + lags
    event, lags = np.array([40.0, 60.0]), np.array([-20.0, 0.0, 20.0, 40.0])
    per = util.posteriorAt(params, exp, event[:, None] + lags[None, :], infRes=res, trials=[2, 0], want=('mean',))
    assert per['mean'].shape == (2, 2, 4) and per['times'].shape == (2, 4) and sess.ctx.calls[-1] == ((2, 4), ('mean',))
    assert np.array_equal(per['mean'][0, 0], 3.0 * (40.0 + lags) / 100.0) and np.array_equal(per['mean'][1, 0], 1.0 * (60.0 + lags) / 100.0)
    # only the variance asked for: the device is not asked for the mean
    util.posteriorAt(params, exp, times, infRes=res, want=('var',))
    assert sess.ctx.calls[-1] == ((5,), ('var',))


def test_shape_errors_unknown_keys_and_an_empty_request(monkeypatch):
    from funs import util
    sess, exp, params, res, _ = _fake(monkeypatch, [8, 8, 8])
    for bad in (np.zeros((2, 4)), np.zeros((3, 2, 2)), np.zeros(0), np.zeros((3, 0)), 5.0):
        with pytest.raises(ValueError, match='times'):
            util.posteriorAt(params, exp, bad, infRes=res)
    with pytest.raises(ValueError, match='times'):
        util.posteriorAt(params, exp, np.zeros((3, 4)), infRes=res, trials=[0, 1])     # three grids for two listed trials
    with pytest.raises(ValueError, match='unknown key'):
        util.posteriorAt(params, exp, np.zeros(2), infRes=res, want=('mean', 'rate'))
    with pytest.raises(ValueError, match='nothing asked for'):
        util.posteriorAt(params, exp, np.zeros(2), infRes=res, want=())
    with pytest.raises(ValueError, match='level'):
        util.posteriorAt(params, exp, np.zeros(2), infRes=res, level=1.0)
    with pytest.raises(ValueError, match='one label per listed trial'):
        util.posteriorAt(params, exp, np.zeros(2), infRes=res, conditions=[0, 1])
    with pytest.raises(ValueError, match='not a device-backed result'):
        util.posteriorAt(params, exp, np.zeros(2), infRes={'post_mean': []})
    sess.post_stamp += 1
    sess.trial_stamp[1] = sess.post_stamp
    with pytest.raises(ValueError, match='superseded.*trial 1'):
        util.posteriorAt(params, exp, np.zeros(2), infRes=res)
    assert sess.ctx.calls == []


def test_a_time_that_is_not_finite_is_refused_before_any_device_call(monkeypatch):
    from funs import util
    sess, exp, params, res, touched = _fake(monkeypatch, [8, 8, 8])
    with pytest.raises(ValueError, match=r'times: entry \(2,\) is not finite'):
        util.posteriorAt(params, exp, np.array([0.0, 1.0, np.nan]), infRes=res)
    grid = np.zeros((3, 4))
    grid[1, 3] = np.inf
    with pytest.raises(ValueError, match=r'times: entry \(1, 3\) is not finite'):
        util.posteriorAt(params, exp, grid, infRes=res)
    assert touched == [] and sess.ctx.calls == []                  # not even the session was looked up


def test_band_arithmetic(monkeypatch):
    from funs import util
    sess, exp, params, res, _ = _fake(monkeypatch, [8, 8])
    times = np.array([0.0, 70.0, 500.0])
    out = util.posteriorAt(params, exp, times, infRes=res, level=0.9, want=('mean', 'var', 'lower', 'upper'))
    z = util._band_z(0.9)
    assert np.array_equal(out['lower'], out['mean'] - z * np.sqrt(out['var'])) and np.array_equal(out['upper'], out['mean'] + z * np.sqrt(out['var']))
    assert np.allclose(out['upper'] - out['lower'], 2.0 * z * np.sqrt(0.25 + (times / 1000.0) ** 2)[None, None, :], rtol=1e-14)
    dflt = util.posteriorAt(params, exp, times, infRes=res)
    assert sorted(dflt) == ['lower', 'mean', 'times', 'upper']
    assert np.allclose(dflt['upper'] - dflt['mean'], 1.959963984540054 * np.sqrt(out['var']), rtol=1e-12)


def test_condition_means_over_ragged_lengths_and_the_inside_span_rule(monkeypatch):
    from funs import util
    lens, bin_ms = [8, 3, 5, 8, 4], 20.0
    sess, exp, params, res, _ = _fake(monkeypatch, lens, bin_ms=bin_ms)
    tiny = 1e-9
    # s = 0 and just before it; the last bins (T_r - 1) bin of the lengths 3, 4, 5, 8 and just behind each
    times = np.array([-tiny, 0.0, 40.0, 40.0 + tiny, 60.0, 60.0 + tiny, 80.0, 80.0 + tiny, 140.0, 140.0 + tiny, 10.0])
    cond = [7, 7, 3, 7, 3]                                              # label 3: trials 2, 4; label 7: trials 0, 1, 3; label 5 below: nobody
    out = util.posteriorAt(params, exp, times, infRes=res, conditions=cond, want=('mean',))
    assert out['condition_labels'].tolist() == [3, 7]
    span = (np.asarray(lens) - 1) * bin_ms
    inside = (times[None, :] >= 0.0) & (times[None, :] <= span[:, None])
    assert out['condition_count'].dtype == np.int32
    assert out['condition_count'].tolist() == [inside[[2, 4]].sum(axis=0).tolist(), inside[[0, 1, 3]].sum(axis=0).tolist()]
    assert out['condition_count'][1].tolist() == [0, 3, 3, 2, 2, 2, 2, 2, 2, 0, 3]
    assert out['condition_count'][0].tolist() == [0, 2, 2, 2, 2, 1, 1, 0, 0, 0, 2]
    for g, members in ((0, [2, 4]), (1, [0, 1, 3])):
        for j in range(times.size):
            who = [i for i in members if inside[i, j]]
            ref = sum(out['mean'][i][:, j] for i in who) / len(who) if who else np.zeros(2)
            assert np.allclose(out['condition_mean'][g][:, j], ref, rtol=1e-15, atol=0.0)
    assert np.all(out['condition_mean'][:, :, 0] == 0.0) and np.all(out['condition_mean'][1][:, 9] == 0.0)      # nobody there: 0 and a count of 0
    # per-trial grids: the rule follows every trial's own times; want=() asks the device for the mean alone
    grids = np.tile(times, (5, 1))
    grids[1] += 1.0
    per = util.posteriorAt(params, exp, grids, infRes=res, conditions=cond, want=())
    assert sorted(per) == ['condition_count', 'condition_labels', 'condition_mean', 'times'] and sess.ctx.calls[-1] == ((5, 11), ('mean',))
    ins2 = (grids >= 0.0) & (grids <= span[:, None])
    assert per['condition_count'].tolist() == [ins2[[2, 4]].sum(axis=0).tolist(), ins2[[0, 1, 3]].sum(axis=0).tolist()]


def test_an_empty_group_gives_zeros_and_a_count_of_zero():
    from funs import util
    mean = np.arange(2 * 2 * 3, dtype=np.float64).reshape(2, 2, 3) + 1.0
    cm, cnt = util._condition_means_at(mean, np.array([0.0, 10.0, 20.0]), np.array([0, 2]), 3, [20.0, 10.0])
    assert cnt.tolist() == [[1, 1, 1], [0, 0, 0], [1, 1, 0]]
    assert np.array_equal(cm[0], mean[0]) and np.all(cm[1] == 0.0)
    assert np.array_equal(cm[2][:, :2], mean[1][:, :2]) and np.all(cm[2][:, 2] == 0.0)
    # a trial listed twice counts twice, in list order
    cm, cnt = util._condition_means_at(np.stack([mean[0], mean[0]]), np.array([0.0, 10.0, 20.0]), np.array([0, 0]), 1, [20.0, 20.0])
    assert cnt.tolist() == [[2, 2, 2]] and np.array_equal(cm[0], mean[0])
