"""Posterior-predictive spike counts without a GPU (pgpfa_count_probabilities / pgpfa_posterior_counts, util.posteriorCounts, the predictive hold-out
scores).  This file holds the numpy restatement of the device's rule (csrc/counts.h) that the GPU tests compare against:

    P(y = k) = int Poisson(k; e^eta) N(eta; m, v) d eta,  by Q Gauss-Hermite nodes centred on the mode of the integrand, in u = (eta - m) / v.

The restatement is checked here against a fine reference - a trapezoid of 200 001 points over +-40 Laplace widths around the mode - on
    m in {-6,-3,-1,0,1,2,3,4.5} x v in {1e-8,1e-4,1e-2,0.1,0.5,1,2,4} x k in {0,1,2,3,5,8,13,21,40,80,200,1000}       (full grid)
and on the part of it with v <= 1 and k <= 80 (restricted grid).  Measured worst |delta log P| of the restatement (this file, numpy 1.x, x86-64):

    Q     full grid    restricted grid
    16    9.13e-05     1.73e-07
    24    2.12e-05     2.27e-09
    32    3.78e-06     9.17e-11
    48    2.57e-07     1.88e-11

(the full grid's worst entries have v = 4, where the integrand is furthest from a Gaussian).  The asserted bounds at Q = 32 are twice the measured
values: 7.6e-6 and 1.9e-10; the error must fall from each Q to the next.  The reference itself: halving its step changes log P by
less than 1e-12 on the grid (the trapezoid converges geometrically for an analytic integrand that decays at both ends)."""
import ctypes as ct
import os
import re

import numpy as np
import pytest
from numpy.polynomial.hermite import hermgauss
from scipy.special import gammaln

from conftest import ROOT, Experiment

NEWTON_MAX = 40
LOG_PI = float(np.log(np.pi))
GRID_M = (-6.0, -3.0, -1.0, 0.0, 1.0, 2.0, 3.0, 4.5)
GRID_V = (1e-8, 1e-4, 1e-2, 0.1, 0.5, 1.0, 2.0, 4.0)
GRID_K = (0, 1, 2, 3, 5, 8, 13, 21, 40, 80, 200, 1000)
TOL_RULE_FULL, TOL_RULE_RESTRICTED = 7.6e-6, 1.9e-10       # twice the measured 3.78e-6 and 9.17e-11 (table above)


# ---- the rule of csrc/counts.h in numpy ------------------------------------------------------------------------------------------------------------
def rule_nodes(Q):
    x, w = hermgauss(Q)
    return x, np.log(w)


def rule_mode(m, v, k, u0):
    """Newton for the mode of the log integrand in u = (eta - m) / v from u0, step by step as counts_mode: -> (u, lam = exp(m + v u))"""
    m, v, k, u = np.broadcast_arrays(np.asarray(m, float), np.asarray(v, float), np.asarray(k, float), np.asarray(u0, float))
    u = u.copy()
    lam = np.exp(m + v * u)
    active = np.ones(u.shape, bool)
    for _ in range(NEWTON_MAX):
        du = (k - lam - u) / (1.0 + v * lam)
        with np.errstate(divide='ignore'):
            du = np.where(v * du > 1.0, 1.0 / v, du)
        du = np.where(active, du, 0.0)
        u = u + du
        lam = np.where(active, np.exp(m + v * u), lam)
        active = active & (np.abs(v * du) > 1e-12)
        if not active.any():
            break
    return u, lam


def rule_logp_at(m, v, k, u, lam, Q):
    x, lw = rule_nodes(Q)
    m, v, k = np.asarray(m, float), np.asarray(v, float), np.asarray(k, float)
    vl = v * lam
    r = 1.0 / (1.0 + vl)
    s, c, ku = np.sqrt(2.0 * v * r), vl * r, k - u
    total = np.zeros(np.broadcast(m, v, k).shape)
    for j in range(Q):
        d = s * x[j]
        total = total + np.exp(ku * d - lam * (np.exp(d) - 1.0) + (x[j] * x[j]) * c + lw[j])
    gs = k * (m + v * u) - lam - 0.5 * v * (u * u) - gammaln(k + 1.0)
    return gs - 0.5 * (LOG_PI + np.log1p(vl)) + np.log(total)


def rule_logp(m, v, k, Q=32):
    """log P(y = k) from a cold start, as the device computes 'logp'"""
    u, lam = rule_mode(m, v, k, 0.0)
    return rule_logp_at(m, v, k, u, lam, Q)


def rule_pmf(m, v, K, Q=32):
    """P(y = k), k = 0 .. K - 1 (last axis), by the walk of the device: the mode of k is searched from the mode of k - 1"""
    m, v = np.broadcast_arrays(np.asarray(m, float), np.asarray(v, float))
    out = np.empty(m.shape + (K,))
    u = np.zeros(m.shape)
    for k in range(K):
        u, lam = rule_mode(m, v, float(k), u)
        out[..., k] = np.exp(rule_logp_at(m, v, float(k), u, lam, Q))
    return out


def rule_band(pmf, level, k_cap):
    """(lower, upper, saturated) from a walked pmf that covers k = 0 .. k_cap at least: the smallest k with CDF(k) >= (1 -+ level) / 2, the sums
    in the order of k; an entry that has not reached its upper quantile at k_cap gets k_cap"""
    cdf = np.cumsum(pmf[..., :k_cap + 1], axis=-1)
    p_lo, p_hi = 0.5 * (1.0 - level), 0.5 * (1.0 + level)

    def first(p):
        hit = cdf >= p
        return np.where(hit.any(axis=-1), hit.argmax(axis=-1), k_cap).astype(np.int32)
    saturated = ~(cdf >= p_hi).any(axis=-1)
    return first(p_lo), first(p_hi), saturated


# ---- the fine reference ----------------------------------------------------------------------------------------------------------------------------
def fine_logp(m, v, k, points=200001, widths=40.0):
    """log P(y = k) of one entry (v > 0) by a trapezoid over +-`widths` Laplace widths around the mode of the integrand, in delta = eta - m"""
    u, lam = rule_mode(m, v, float(k), 0.0)
    u, lam = float(u), float(lam)
    dstar, h = v * u, lam + 1.0 / v
    t = np.linspace(-widths, widths, points) / np.sqrt(h)
    delta = dstar + t
    g = k * (m + delta) - np.exp(m + delta) - delta * delta / (2.0 * v)
    gs = k * (m + dstar) - lam - dstar * dstar / (2.0 * v)
    f = np.exp(g - gs)
    integral = (f.sum() - 0.5 * (f[0] + f[-1])) * (t[1] - t[0])
    return gs - gammaln(k + 1.0) + np.log(integral) - 0.5 * np.log(2.0 * np.pi * v)


_GRID = {}


def full_grid():
    """(m, v, k, fine reference) over the full grid, flat; computed once per process"""
    if not _GRID:
        mm, vv, kk = (a.reshape(-1) for a in np.meshgrid(GRID_M, GRID_V, np.asarray(GRID_K, float), indexing='ij'))
        _GRID['g'] = (mm, vv, kk, np.array([fine_logp(a, b, c) for a, b, c in zip(mm, vv, kk)]))
    return _GRID['g']


def rule_errors(Q):
    mm, vv, kk, ref = full_grid()
    err = np.abs(rule_logp(mm, vv, kk, Q) - ref)
    restricted = (vv <= 1.0) & (kk <= 80)
    return float(err.max()), float(err[restricted].max())


# ---- the rule against the fine reference -----------------------------------------------------------------------------------------------------------
def test_the_rule_against_the_fine_reference_on_both_grids():
    full, restricted = rule_errors(32)
    print('Q = 32: worst |delta log P| %.2e on the full grid (limit %.1e), %.2e on the restricted grid (limit %.1e)'
          % (full, TOL_RULE_FULL, restricted, TOL_RULE_RESTRICTED))
    assert full <= TOL_RULE_FULL and restricted <= TOL_RULE_RESTRICTED


def test_the_error_of_the_rule_falls_with_the_node_count():
    errs = [rule_errors(Q) for Q in (16, 24, 32, 48)]
    print('worst |delta log P| (full, restricted) at Q = 16, 24, 32, 48: ' + ', '.join('(%.2e, %.2e)' % e for e in errs))
    for a, b in zip(errs, errs[1:]):
        assert b[0] < a[0] and b[1] < a[1]


def test_newton_from_the_mean_stays_far_below_the_cap_on_the_grid():
    """the cap of 40 on the device leaves room: the cold search on the full grid takes 18 steps at the most, the confirming one included"""
    mm, vv, kk, _ = full_grid()
    u = np.zeros(mm.shape)
    lam = np.exp(mm)
    steps = np.zeros(mm.shape, int)
    active = np.ones(mm.shape, bool)
    for _ in range(NEWTON_MAX):
        du = (kk - lam - u) / (1.0 + vv * lam)
        du = np.where(vv * du > 1.0, 1.0 / vv, du)
        du = np.where(active, du, 0.0)
        u, steps = u + du, steps + active
        lam = np.exp(mm + vv * u)
        active &= np.abs(vv * du) > 1e-12
    print('most Newton steps from a cold start on the grid: %d' % steps.max())
    assert not active.any() and steps.max() <= NEWTON_MAX // 2


# ---- identities that need no reference -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('m', [-3.0, 0.0, 1.0])
@pytest.mark.parametrize('v', [0.0, 1e-3, 0.1, 0.5])
def test_the_pmf_sums_to_one_and_has_the_closed_form_moments(m, v):
    K = 256
    pmf = rule_pmf(m, v, K)
    k = np.arange(K, dtype=float)
    mu = np.exp(m + 0.5 * v)
    var = mu + mu * mu * np.expm1(v)
    s0, s1 = pmf.sum(), (k * pmf).sum()
    s2 = (k * k * pmf).sum() - s1 * s1
    print('m = %g, v = %g: sum - 1 = %.2e, mean rel %.2e, var rel %.2e (limit 1e-6)' % (m, v, s0 - 1.0, s1 / mu - 1.0, s2 / var - 1.0))
    assert abs(s0 - 1.0) <= 1e-6 and abs(s1 / mu - 1.0) <= 1e-6 and abs(s2 / var - 1.0) <= 1e-6


@pytest.mark.parametrize('v', [0.0, 1e-12])
def test_no_variance_gives_the_poisson_log_pmf(v):
    """the test that catches a cancellation in eta - m.  To first order in v the mixture is Poisson(k; lam) (1 + v ((k - lam)^2 - lam) / 2), lam = e^m:
    at v = 1e-12 that is the Poisson pmf to 1e-10 while |k - lam| <= 8 (3.2e-11), and with the term every k of the list agrees to 1e-10"""
    from scipy.stats import poisson
    mm, kk = (a.reshape(-1) for a in np.meshgrid([-3.0, 0.0, 1.0], [0.0, 1.0, 2.0, 5.0, 8.0, 13.0, 40.0], indexing='ij'))
    lam = np.exp(mm)
    near = kk <= 8.0
    for Q in (8, 32, 64):
        got = rule_logp(mm, v, kk, Q)
        err = np.abs(got - poisson.logpmf(kk, lam))[near]
        err1 = np.abs(got - poisson.logpmf(kk, lam) - np.log1p(0.5 * v * ((kk - lam) ** 2 - lam)))
        print('v = %g, Q = %d: worst |log P - Poisson log pmf| %.2e for k <= 8, %.2e for k <= 40 with the first-order term (limit 1e-10)'
              % (v, Q, err.max(), err1.max()))
        assert err.max() <= 1e-10 and err1.max() <= 1e-10
    walked = np.log(rule_pmf(np.array([-3.0, 0.0, 1.0]), v, 14))
    ref = poisson.logpmf(np.arange(14)[None, :], np.exp(np.array([-3.0, 0.0, 1.0]))[:, None])
    assert np.max(np.abs(walked - ref)) <= 1e-10


def test_the_walk_and_the_cold_start_agree():
    """a warm start moves the centre of the rule by less than the Newton tolerance: pmf[k] and exp(logp at k) differ by rounding"""
    mm, vv = (a.reshape(-1) for a in np.meshgrid(GRID_M, GRID_V, indexing='ij'))
    walked = np.log(rule_pmf(mm, vv, 41))
    for k in (0, 1, 5, 40):
        assert np.max(np.abs(walked[:, k] - rule_logp(mm, vv, float(k)))) <= 1e-10


# ---- quantiles and saturation ----------------------------------------------------------------------------------------------------------------------
def test_quantiles_against_the_cumulative_sum_of_the_fine_reference():
    """lower / upper of the rule's walk against the quantiles of the cumulative sum of the FINE pmf, where the fine CDF is not within 1e-5 of the
    level's two probabilities (there the rule's error of 3.8e-6 may move a quantile by one)"""
    checked = 0
    for m, v in ((-1.0, 0.5), (1.0, 0.1), (2.0, 1.0), (0.0, 2.0)):
        K = 400
        fine = np.exp(np.array([fine_logp(m, v, k, points=20001) for k in range(K)]))
        cdf = np.cumsum(fine)
        pmf = rule_pmf(m, v, K)
        for level in (1e-6, 0.5, 0.95, 0.999, 1.0 - 1e-6):
            p_lo, p_hi = 0.5 * (1.0 - level), 0.5 * (1.0 + level)
            lo, up, sat = rule_band(pmf, level, K - 1)
            if np.min(np.abs(cdf - p_lo)) > 1e-5:
                assert lo == np.argmax(cdf >= p_lo)
                checked += 1
            if np.min(np.abs(cdf - p_hi)) > 1e-5 and cdf[-1] >= p_hi:
                assert up == np.argmax(cdf >= p_hi) and not sat
                checked += 1
            assert 0 <= lo <= up
    assert checked >= 30
    lo, up, _ = rule_band(rule_pmf(1.0, 0.1, 60), 1e-9, 59)            # a level near 0: both ends at the median
    assert lo == up


def test_saturation_at_a_cap_of_three():
    m = np.array([-3.0, 0.0, 1.0, 3.0])
    pmf = rule_pmf(m, 0.5, 4)
    lo, up, sat = rule_band(pmf, 0.95, 3)
    cdf3 = pmf.sum(axis=-1)
    print('CDF(3) = %s -> upper %s, saturated %s' % (cdf3, up, sat))
    assert sat.tolist() == (cdf3 < 0.975).tolist() == [False, True, True, True]
    assert up.tolist()[1:] == [3, 3, 3] and lo.tolist()[3] == 3 and lo.tolist()[:3] == [0, 0, 0] and up.tolist()[0] == 1 - int(pmf[0, 0] >= 0.975)


# ---- the predictive score --------------------------------------------------------------------------------------------------------------------------
def test_predictive_bits_per_spike_is_its_formula():
    from math import lgamma, log
    from funs import util
    rng = np.random.default_rng(5)
    truth = [rng.poisson(1.5, (3, 6)).astype(float), rng.poisson(1.5, (3, 4)).astype(float)]
    truth[0][2] = 0.0
    truth[1][2] = 0.0                                                  # a row without a spike
    logp = [-rng.uniform(0.2, 3.0, (3, 6)), -rng.uniform(0.2, 3.0, (3, 4))]
    scored = [rng.random((3, 6)) < 0.7, rng.random((3, 4)) < 0.7]
    logp[0][~scored[0]] = np.nan                                       # what is not scored may hold anything
    total, per_row = util._score_predictive(truth, logp, scored)
    num, den = np.zeros(3), np.zeros(3)
    for n in range(3):
        ys = [y[n, t] for y, sc in zip(truth, scored) for t in range(y.shape[1]) if sc[n, t]]
        lps = [lp[n, t] for lp, sc in zip(logp, scored) for t in range(lp.shape[1]) if sc[n, t]]
        lbar = sum(ys) / len(ys)
        for y, lp in zip(ys, lps):
            null = (y * log(lbar) if y > 0 else 0.0) - lbar - lgamma(y + 1.0)
            num[n] += lp - null
        den[n] = sum(ys)
    assert np.allclose(per_row[:2], num[:2] / (np.log(2.0) * den[:2]), rtol=1e-13) and np.isnan(per_row[2])
    assert np.isclose(total, num.sum() / (np.log(2.0) * den.sum()), rtol=1e-13)
    keys = util._predictive_keys(truth, logp, scored)
    assert sorted(keys) == ['bitsPerSpikePredictive', 'bitsPerSpikePredictivePerNeuron', 'logPredictive'] and keys['bitsPerSpikePredictive'] == total
    assert all(np.array_equal(np.isnan(a), ~sc) for a, sc in zip(keys['logPredictive'], scored))


# ---- refusals before any device call ---------------------------------------------------------------------------------------------------------------
def _untouchable(monkeypatch):
    from funs import _session
    touched = []
    monkeypatch.setattr(_session, 'session_for', lambda experiment, xdim: touched.append(1))
    exp = Experiment([np.zeros((3, L)) for L in (8, 5, 8)], 20.0)
    params = {'C': np.ones((3, 2)), 'd': -np.ones(3), 'tau': np.full(2, 0.1)}
    return exp, params, touched


def test_argument_refusals_fire_before_the_session_is_looked_up(monkeypatch):
    from funs import util
    exp, params, touched = _untouchable(monkeypatch)
    with pytest.raises(ValueError, match='unknown key'):
        util.posteriorCounts(params, exp, want=('logp', 'rate'))
    with pytest.raises(ValueError, match='nothing asked for'):
        util.posteriorCounts(params, exp, want=())
    for level in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError, match='level'):
            util.posteriorCounts(params, exp, level=level, want=('lower',))
    with pytest.raises(ValueError, match='maxCount'):
        util.posteriorCounts(params, exp, maxCount=-1, want=('upper',))
    with pytest.raises(ValueError, match='maxCount'):
        util.posteriorCounts(params, exp, want=('pmf',))
    with pytest.raises(ValueError, match='maxCount'):
        util.posteriorCounts(params, exp, maxCount=1024, want=('pmf',))
    with pytest.raises(ValueError, match='one .* array per listed trial'):
        util.posteriorCounts(params, exp, counts=[np.zeros((3, 8))])
    with pytest.raises(ValueError, match=r'counts\[1\] must have shape \(ydim, T_r\) = \(3, 5\)'):
        util.posteriorCounts(params, exp, counts=[np.zeros((3, 8)), np.zeros((3, 8)), np.zeros((3, 8))])
    with pytest.raises(ValueError, match=r'counts\[0\]: integers'):
        util.posteriorCounts(params, exp, trials=[2], counts=[np.full((3, 8), -1)])
    with pytest.raises(ValueError, match=r'counts\[0\]: integers'):
        util.posteriorCounts(params, exp, trials=[2], counts=[np.full((3, 8), 0.5)])
    assert touched == []


def test_the_predictive_keyword_of_the_scores(monkeypatch):
    """predictive=True hands _predicted_without_hidden the true counts at the scored entries and zeros elsewhere, and adds its three keys; the
    default changes neither the call nor the keys"""
    from funs import util
    rng = np.random.default_rng(2)
    lens = (8, 5, 8)
    exp = Experiment([rng.poisson(1.0, (3, L)).astype(float) for L in lens], 20.0)
    params = {'C': np.ones((3, 2)), 'd': -np.ones(3), 'tau': np.full(2, 0.1)}
    seen = []

    def fake(what, params_, experiment, Yt, len_t, masked, bins_t, rows=slice(None), counts_at=None):
        seen.append(counts_at)
        n = Yt.shape[0] - 1
        nrows = np.zeros(Yt.shape[1])[rows].size
        lam = [np.full((nrows, int(len_t[i])), 0.7) for i in range(n)]
        logp = None if counts_at is None else [-(1.0 + counts_at[i][rows][:, :int(len_t[i])].astype(float)) for i in range(n)]
        return lam, logp
    monkeypatch.setattr(util, '_predicted_without_hidden', fake)
    hide = [rng.random((3, L)) < 0.4 for L in lens]
    plain = util.binHoldout(params, exp, hide)
    assert seen[-1] is None and sorted(plain) == ['bitsPerSpike', 'bitsPerSpikePerNeuron', 'nScored', 'rate']
    pred = util.binHoldout(params, exp, hide, predictive=True)
    at = seen[-1]
    assert at.dtype == np.int32 and at.shape == (4, 3, 8) and not at[3].any()
    for i, L in enumerate(lens):
        assert np.array_equal(at[i][:, :L], np.where(hide[i], exp.data[i]['Y'], 0)) and not at[i][:, L:].any()
    assert sorted(pred) == sorted(list(plain) + ['bitsPerSpikePredictive', 'bitsPerSpikePredictivePerNeuron', 'logPredictive'])
    assert pred['bitsPerSpike'] == plain['bitsPerSpike'] and pred['nScored'] == plain['nScored']
    truth = [tr['Y'] for tr in exp.data]
    assert pred['bitsPerSpikePredictive'] == util._score_predictive(truth, [-(1.0 + np.where(h, y, 0)) for h, y in zip(hide, truth)], hide)[0]
    co_plain = util.coSmoothing(params, exp, [1])
    assert seen[-1] is None and sorted(co_plain) == ['bitsPerSpike', 'bitsPerSpikePerNeuron', 'heldOut', 'rate']
    co = util.coSmoothing(params, exp, [1], predictive=True)
    at = seen[-1]
    assert not at[:, [0, 2]].any() and all(np.array_equal(at[i, 1, :L], exp.data[i]['Y'][1]) for i, L in enumerate(lens))
    assert co['logPredictive'][1].shape == (1, 5) and np.isfinite(co['bitsPerSpikePredictive'])
    with pytest.raises(ValueError, match="score='speckled'"):
        util.crossValidation(exp, numTrainingTrials=2, numTestTrials=1, maxXdim=1, score='evidence', predictive=True)


# ---- symbols ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def hip():
    import __graft_entry__ as ge
    ge.build()
    from funs import _hip
    return _hip


def test_header_binding_and_library_agree_on_the_two_entry_points(hip):
    lib = hip.load_library()
    header = open(os.path.join(ROOT, 'include', 'pgpfa.h')).read()
    bare = re.sub(r'/\*.*?\*/', ' ', header, flags=re.S)
    outs = (r'\s*,\s*int\s+K\s*,\s*double\s+level\s*,\s*int\s+k_cap\s*,\s*double\s*\*\s*logp\s*,\s*double\s*\*\s*pmf\s*,\s*int32_t\s*\*\s*lower\s*,\s*int32_t\s*\*\s*upper'
            r'\s*,\s*double\s*\*\s*pmean\s*,\s*double\s*\*\s*pvar\s*\)\s*;')
    assert re.search(r'int\s+pgpfa_count_probabilities\s*\(\s*pgpfa_ctx\s*\*\s*ctx\s*,\s*long\s+long\s+n_entries\s*,\s*const\s+double\s*\*\s*m\s*,\s*const\s+double\s*\*\s*v'
                     r'\s*,\s*const\s+int32_t\s*\*\s*counts' + outs, bare)
    assert re.search(r'int\s+pgpfa_posterior_counts\s*\(\s*pgpfa_ctx\s*\*\s*ctx\s*,\s*int\s+n\s*,\s*const\s+int32_t\s*\*\s*idx\s*,\s*const\s+int32_t\s*\*\s*counts' + outs, bare)
    c_double_p, c_int32_p = ct.POINTER(ct.c_double), ct.POINTER(ct.c_int32)
    tail = [c_int32_p, ct.c_int, ct.c_double, ct.c_int, c_double_p, c_double_p, c_int32_p, c_int32_p, c_double_p, c_double_p]
    for name, head in (('pgpfa_count_probabilities', [ct.c_void_p, ct.c_longlong, c_double_p, c_double_p]), ('pgpfa_posterior_counts', [ct.c_void_p, ct.c_int, c_int32_p])):
        assert name in hip.EXPORTED_SYMBOLS and name in hip._SIGNATURES and hasattr(lib, name)
        assert list(getattr(lib, name).argtypes) == head + tail
    assert '"counts_chunk_trials"' in header and '"counts_nodes"' in header and '"counts_saturated"' in header
    assert hasattr(hip.Context, 'count_probabilities') and hasattr(hip.Context, 'posterior_counts')
    from funs import engine, util
    assert callable(util.posteriorCounts) and callable(engine.PPGPFAfit.posteriorCounts)
    import __graft_entry__ as ge
    assert os.path.exists(os.path.join(ge.CSRC, 'counts.h')) and 'counts.h' in open(os.path.join(ge.CSRC, 'rates.hip')).read()


def test_null_context_and_bad_arguments_are_refused_without_a_device(hip):
    lib = hip.load_library()
    z = np.zeros(1)
    assert lib.pgpfa_count_probabilities(None, 1, hip.dptr(z), hip.dptr(z), None, 1, 0.95, 10, None, None, None, None, hip.dptr(z), None) != 0
    assert 'null context' in lib.pgpfa_last_error().decode()
    assert lib.pgpfa_posterior_counts(None, 1, None, None, 1, 0.95, 10, None, None, None, None, hip.dptr(z), None) != 0
    assert 'null context' in lib.pgpfa_last_error().decode()
    with pytest.raises(ValueError, match='unknown output'):
        hip.Context._count_outputs(None, (1,), None, 1, 0.95, 1, ('logp', 'rate'))
    with pytest.raises(ValueError, match='counts must have shape'):
        hip.Context._count_outputs(None, (2, 3), np.zeros((3, 2)), 1, 0.95, 1, ('logp',))
