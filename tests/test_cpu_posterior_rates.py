"""Host side of the posterior firing rates, without a GPU: the CSR form of the trial -> group table (pgpfa_rates_group_csr: what the device walks),
the label -> group mapping, the z of a credible level, and what util.posteriorRates does around the device call - units, band, cutting to a
trial's own bins, condition means, the refusals - on a fake session whose context computes eta / var / sums in numpy."""
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


def test_header_binding_and_library_agree_on_the_new_entry_points(hip):
    lib = hip.load_library()
    header = open(os.path.join(ROOT, 'include', 'pgpfa.h')).read()
    assert re.search(r'int\s+pgpfa_posterior_rates\s*\(\s*pgpfa_ctx\s*\*\s*ctx\s*,\s*int\s+n\s*,\s*const\s+int32_t\s*\*\s*idx', header)
    for name in ('pgpfa_posterior_rates', 'pgpfa_rates_group_csr'):
        assert name in hip.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert '"rates_chunk_trials"' in header
    assert hasattr(hip.Context, 'posterior_rates')
    from funs import engine, util
    assert callable(util.posteriorRates) and callable(engine.PPGPFAfit.posteriorRates)


def test_group_csr_lists_every_group_in_list_order(hip):
    rng = np.random.default_rng(3)
    for n, G in ((1, 1), (6, 4), (37, 5), (200, 9)):
        group = rng.integers(0, G, size=n).astype(np.int32)
        group[group == G - 1] = 0                                   # the last group is empty
        start, pos = hip.rates_group_csr(group, G)
        assert start.shape == (G + 1,) and start[0] == 0 and start[-1] == n and np.all(np.diff(start) >= 0)
        assert sorted(pos.tolist()) == list(range(n))
        for g in range(G):
            assert pos[start[g]:start[g + 1]].tolist() == np.flatnonzero(group == g).tolist()
        assert start[G - 1] == start[G] or G == 1
        # a chunk of the list: positions first..last-1 only, still global positions, still in list order
        first, last = n // 3, n - n // 4
        start_c, pos_c = hip.rates_group_csr(group, G, first, last)
        assert start_c[-1] == last - first
        for g in range(G):
            assert pos_c[start_c[g]:start_c[g + 1]].tolist() == [i for i in range(first, last) if group[i] == g]


def test_group_csr_refuses_ids_out_of_range(hip):
    for bad in ([0, 4, 1], [0, -1, 1]):
        with pytest.raises(hip.HipBackendError, match='group id'):
            hip.rates_group_csr(bad, 4)


def test_labels_become_dense_group_ids():
    from funs import util
    labels, group = util._condition_groups([7, -2, 7, 40, -2, 7], 6)
    assert labels.tolist() == [-2, 7, 40] and group.tolist() == [1, 0, 1, 2, 0, 1] and group.dtype == np.int32
    labels, group = util._condition_groups(np.array([3.0, 1.0]), 2)         # integer-valued floats are labels too
    assert labels.tolist() == [1, 3] and group.tolist() == [1, 0]
    with pytest.raises(ValueError, match='one label per listed trial'):
        util._condition_groups([1, 2, 3], 4)
    with pytest.raises(ValueError, match='integer labels'):
        util._condition_groups([0.5, 1.0], 2)


def test_z_of_a_credible_level():
    from funs import util
    # P(|N(0,1)| <= z) = level: tabulated quantiles of the normal distribution
    for level, z in ((0.95, 1.959963984540054), (0.5, 0.6744897501960817), (0.99, 2.5758293035489004), (0.6826894921370859, 1.0)):
        assert abs(util._band_z(level) - z) <= 1e-12
    for bad in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError, match='level'):
            util._band_z(bad)


# ---- util.posteriorRates around a fake device ---------------------------------------------------------------------------------------------------
class _FakeCtx:
    """posterior_rates in numpy from a stored synthetic posterior; records what it was asked for"""

    def __init__(self, C, d, mean, vsm, lens):
        self.C, self.d, self.mean, self.vsm, self.lens = C, d, mean, vsm, lens
        self.q, self.T = C.shape[0], mean.shape[2]
        self.asked = []

    def posterior_rates(self, idx, group=None, n_groups=0, want=('eta', 'var')):
        self.asked.append(tuple(want))
        eta = self.d[None, :, None] + np.einsum('nk,rkt->rnt', self.C, self.mean[idx])
        var = np.einsum('ni,rtij,nj->rnt', self.C, self.vsm[idx], self.C)
        live = np.arange(self.T)[None, :] < self.lens[idx][:, None]
        rate = np.exp(eta + 0.5 * var) * live[:, None, :]
        out = {'eta': eta, 'var': var, 'ell': np.zeros((len(idx), self.q))}
        if group is not None:
            out['group_sum'] = np.stack([rate[group == g].sum(axis=0) for g in range(n_groups)])
            out['group_count'] = np.stack([live[group == g].sum(axis=0) for g in range(n_groups)]).astype(np.int32)
        return {k: out[k] for k in want}


def _fake(monkeypatch, lens, T=8, q=3, p=2, comm_ready=False):
    from funs import _session
    rng = np.random.default_rng(5)
    R = len(lens)
    A = rng.standard_normal((R, T, p, p))
    sess = object.__new__(_session.Session)
    sess.R, sess.q, sess.T, sess.p = R, q, T, p
    sess.lengths = None if all(v == T for v in lens) else np.asarray(lens, dtype=np.int32)
    sess.ctx = _FakeCtx(rng.standard_normal((q, p)) / np.sqrt(p), -np.ones(q), 0.5 * rng.standard_normal((R, p, T)),
                        0.05 * A @ A.transpose(0, 1, 3, 2) + 0.01 * np.eye(p), np.asarray(lens))
    sess.post_stamp = sess.mode_stamp = 1
    sess.trial_stamp = np.ones(R, dtype=np.int64)
    sess.comm_ready = comm_ready
    sess.set_params = lambda params: None
    monkeypatch.setattr(_session, 'session_for', lambda experiment, xdim: (sess, np.arange(R, dtype=np.int32)))
    exp = Experiment([np.zeros((q, L)) for L in lens], 20.0)
    params = {'C': sess.ctx.C, 'd': sess.ctx.d, 'tau': np.full(p, 0.1)}
    return sess, exp, params, _session.DeviceInfRes(sess, np.arange(R, dtype=np.int32), (0, R))


def test_units_band_and_condition_means_on_equal_trials(monkeypatch):
    from funs import util
    sess, exp, params, res = _fake(monkeypatch, [8, 8, 8, 8, 8])
    cond = [5, 2, 5, 5, 2]
    out = util.posteriorRates(params, exp, infRes=res, conditions=cond, level=0.9, want=('rate', 'lower', 'upper', 'median', 'eta', 'var'))
    ref = sess.ctx.posterior_rates(np.arange(5))
    per_s = 1000.0 / 20.0                                             # 20 ms bins
    z = util._band_z(0.9)
    assert np.array_equal(out['eta'], ref['eta']) and np.array_equal(out['var'], ref['var']) and out['rate'].shape == (5, 3, 8)
    assert np.allclose(out['rate'], np.exp(ref['eta'] + 0.5 * ref['var']) * per_s, rtol=1e-15)
    assert np.allclose(out['median'], np.exp(ref['eta']) * per_s, rtol=1e-15)
    assert np.allclose(out['upper'], np.exp(ref['eta'] + z * np.sqrt(ref['var'])) * per_s, rtol=1e-15)
    assert np.all(out['lower'] <= out['median']) and np.all(out['median'] <= out['rate']) and np.all(out['rate'] <= out['upper'])
    assert out['condition_labels'].tolist() == [2, 5] and out['condition_count'].tolist() == [[2] * 8, [3] * 8]
    assert np.allclose(out['condition_mean'][0], out['rate'][[1, 4]].mean(axis=0), rtol=1e-14)
    assert np.allclose(out['condition_mean'][1], out['rate'][[0, 2, 3]].mean(axis=0), rtol=1e-14)


def test_cut_to_the_trials_own_bins_unless_forecast(monkeypatch):
    from funs import util
    lens = [8, 3, 5, 8]
    sess, exp, params, res = _fake(monkeypatch, lens)
    out = util.posteriorRates(params, exp, infRes=res, conditions=[0, 0, 1, 0])
    assert isinstance(out['rate'], list) and [a.shape for a in out['rate']] == [(3, L) for L in lens]
    full = util.posteriorRates(params, exp, infRes=res, forecast=True)
    assert isinstance(full['rate'], np.ndarray) and full['rate'].shape == (4, 3, 8)
    for i, L in enumerate(lens):
        assert np.array_equal(out['rate'][i], full['rate'][i][:, :L]) and np.array_equal(out['upper'][i], full['upper'][i][:, :L])
    # a bin only trial 2 of condition 1 reaches / nobody of a condition reaches: count and NaN
    assert out['condition_count'].tolist() == [[3, 3, 3, 2, 2, 2, 2, 2], [1, 1, 1, 1, 1, 0, 0, 0]]
    assert np.all(np.isnan(out['condition_mean'][1][:, 5:])) and not np.any(np.isnan(out['condition_mean'][1][:, :5]))
    assert np.allclose(out['condition_mean'][0][:, 4], (full['rate'][0][:, 4] + full['rate'][3][:, 4]) / 2, rtol=1e-14)
    # a sub-list of trials with one length: one array again
    sub = util.posteriorRates(params, exp, infRes=res, trials=[1, 1])
    assert isinstance(sub['rate'], np.ndarray) and sub['rate'].shape == (2, 3, 3)


def test_condition_means_alone_ask_the_device_for_no_plane(monkeypatch):
    from funs import util
    sess, exp, params, res = _fake(monkeypatch, [8, 8, 8])
    out = util.posteriorRates(params, exp, infRes=res, conditions=[1, 1, 0], want=())
    assert sorted(out) == ['condition_count', 'condition_labels', 'condition_mean']
    assert sess.ctx.asked == [('group_sum', 'group_count')]
    out = util.posteriorRates(params, exp, infRes=res, want=('ell',))
    assert sorted(out) == ['ell'] and sess.ctx.asked[-1] == ('ell',)
    with pytest.raises(ValueError, match='nothing asked for'):
        util.posteriorRates(params, exp, infRes=res, want=())
    with pytest.raises(ValueError, match='unknown key'):
        util.posteriorRates(params, exp, infRes=res, want=('rates',))


def test_superseded_foreign_and_sharded_are_refused(monkeypatch):
    from funs import util
    sess, exp, params, res = _fake(monkeypatch, [8, 8, 8])
    sess.post_stamp += 1
    sess.trial_stamp[1] = sess.post_stamp                             # a later E-step went over trial 1
    with pytest.raises(ValueError, match='superseded.*trial 1'):
        util.posteriorRates(params, exp, infRes=res)
    assert util.posteriorRates(params, exp, infRes=res, trials=[0, 2])['rate'].shape == (2, 3, 8)     # the others are still the resident ones
    with pytest.raises(ValueError, match="not a device-backed result"):
        util.posteriorRates(params, exp, infRes={'post_mean': [], 'post_vsm': []})
    other, _, _, res_other = _fake(monkeypatch, [8, 8, 8])
    with pytest.raises(ValueError, match="not a device-backed result"):
        util.posteriorRates(params, exp, infRes=res)                  # (res belongs to the first session)
    other.comm_ready = True
    with pytest.raises(NotImplementedError, match='posteriorRates'):
        util.posteriorRates(params, exp, infRes=res_other)
