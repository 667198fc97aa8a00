"""Posterior-predictive spike counts on the device (pgpfa_count_probabilities, pgpfa_posterior_counts, util.posteriorCounts and the predictive hold-out
scores) against the numpy restatement of the same rule in test_cpu_posterior_counts.py, which that file checks against a fine
reference.  Device against restatement is rounding only - the same nodes, the same Newton steps, the same sums in the same order - so it has its own
tolerance, far below the rule's error (3.8e-6 at 32 nodes).  Measured on one MI355X over the full grid of the CPU file plus v = 0 (864 entries) and
the walks below: worst |delta log P| 3.64e-12 (logp: at m = -6, v = 1e-8, k = 1000, where log P = -11 900 is a sum of k eta = -6000 and lgamma(1001) =
5912 - one unit in the last place of those is 9e-13, and the two lgamma and exp implementations round them differently), worst relative pmf error
1.14e-13 (K = 64 and 65, pmf down to 1e-256: the same effect at |log P| = 590); at the shapes of the resident tests 1.2e-13 and 9.9e-14.  TOL_LOGP and
TOL_PMF are ten times the measured figures.  Every test prints its figures before it asserts."""
import numpy as np
import pytest

from conftest import Experiment
from test_cpu_posterior_counts import GRID_K, GRID_M, GRID_V, rule_band, rule_logp, rule_pmf
from test_cpu_posterior_samples import BIN_MS, problem

pytestmark = pytest.mark.gpu

TOL_LOGP, TOL_PMF = 3.7e-11, 1.2e-12     # ten times the measured 3.64e-12 and 1.14e-13 (above)
ALL = ('logp', 'pmf', 'lower', 'upper', 'pmean', 'pvar')
CASES = [((5, 3, 24), 7), ((17, 1, 21), 20)]              # ((neurons, latents, bins), trials)
CASE_IDS = ['7x3x24-q5', '20x1x21-q17']
ENGINES = [1, 2]
ENGINE_IDS = ['dense', 'lowrank']
LIST = np.array([3, 0, 2, 1, 0], dtype=np.int32)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == 'f')


def worst(dev, ref):
    """(worst |delta log P|, worst relative pmf error) of a dict of device outputs against (logp, pmf) of the restatement; None where not there"""
    e_l = float(np.max(np.abs(dev['logp'] - ref[0]))) if 'logp' in dev else 0.0
    e_p = float(np.max(np.abs(dev['pmf'] - ref[1]) / ref[1])) if 'pmf' in dev else 0.0
    return e_l, e_p


def check_band(tag, dev, pmf_ref, level, k_cap, saturated_info=None):
    """lower / upper / saturation against the restatement's walk, except where its CDF comes within 1e-9 of one of the two probabilities"""
    lo, up, sat = rule_band(pmf_ref, level, k_cap)
    cdf = np.cumsum(pmf_ref[..., :k_cap + 1], axis=-1)
    clear = (np.min(np.abs(cdf - 0.5 * (1.0 - level)), axis=-1) > 1e-9) & (np.min(np.abs(cdf - 0.5 * (1.0 + level)), axis=-1) > 1e-9)
    print('%s: %d of %d entries compared, %d saturated at k_cap = %d' % (tag, clear.sum(), clear.size, sat.sum(), k_cap))
    assert clear.mean() > 0.99
    assert np.array_equal(dev['lower'][clear], lo[clear]) and np.array_equal(dev['upper'][clear], up[clear])
    if saturated_info is not None and clear.all():
        assert saturated_info == sat.sum()


@pytest.fixture(scope='module')
def plain_ctx():
    from funs import _hip
    ctx = _hip.Context(5, 3, 24, 1, BIN_MS)                # (a device and a stream: no counts, parameters or posterior)
    yield ctx
    ctx.close()


@pytest.fixture(scope='module')
def grid():
    """the full grid of the CPU file plus v = 0, flat, with the restatement's logp"""
    mm, vv, kk = (a.reshape(-1) for a in np.meshgrid(GRID_M, (0.0,) + GRID_V, np.asarray(GRID_K, float), indexing='ij'))
    return mm, vv, kk.astype(np.int32), rule_logp(mm, vv, kk)


# ---- 1. the kernel on known moments -----------------------------------------------------------------------------------------------------------------
def test_logp_on_the_full_grid_and_the_same_bits_whatever_else_is_asked_for(plain_ctx, grid):
    mm, vv, kk, ref = grid
    got = plain_ctx.count_probabilities(mm, vv, counts=kk, want=['logp'])['logp']
    err = np.abs(got - ref)
    i = int(np.argmax(err))
    print('logp, %d entries: worst |delta log P| %.2e at m = %g, v = %g, k = %d (limit %.1e)' % (mm.size, err[i], mm[i], vv[i], kk[i], TOL_LOGP))
    assert err[i] <= TOL_LOGP
    more = plain_ctx.count_probabilities(mm, vv, counts=kk, K=5, level=0.9, k_cap=40, want=ALL)
    assert same(more['logp'], got)
    assert same(plain_ctx.count_probabilities(mm, vv, counts=kk, K=64, want=['logp', 'pmf'])['logp'], got)
    mu = np.exp(mm + 0.5 * vv)
    assert np.allclose(more['pmean'], mu, rtol=1e-14) and np.allclose(more['pvar'], mu + mu * mu * np.expm1(vv), rtol=1e-13)


@pytest.mark.parametrize('n', [1, 63, 64, 65, 257])
def test_entry_counts_around_the_workgroup_size(plain_ctx, grid, n):
    mm, vv, kk, ref = grid
    pick = (np.arange(n) * 7) % mm.size                      # a spread of the grid; k up to 1000 among them
    whole = plain_ctx.count_probabilities(mm, vv, counts=kk, K=5, level=0.95, k_cap=30, want=ALL)
    part = plain_ctx.count_probabilities(mm[pick], vv[pick], counts=kk[pick], K=5, level=0.95, k_cap=30, want=ALL)
    for key in ALL:
        assert same(part[key], whole[key][pick]), key          # an entry's bits do not depend on the list
    pmf = rule_pmf(mm[pick], vv[pick], 31)
    e_l, e_p = worst(part, (ref[pick], pmf[:, :5]))
    print('n = %d: worst |delta log P| %.2e, worst relative pmf error %.2e (limits %.1e, %.1e)' % (n, e_l, e_p, TOL_LOGP, TOL_PMF))
    assert e_l <= TOL_LOGP and e_p <= TOL_PMF
    check_band('n = %d' % n, part, pmf, 0.95, 30, plain_ctx.info('counts_saturated'))


@pytest.mark.parametrize('K', [1, 5, 64, 65])
def test_pmf_widths_around_the_staging_tile(plain_ctx, K):
    mm, vv = (a.reshape(-1) for a in np.meshgrid(GRID_M, (0.0,) + GRID_V, indexing='ij'))          # 72 entries: two workgroups, the second short
    got = plain_ctx.count_probabilities(mm, vv, K=K, want=['pmf'])['pmf']
    ref = rule_pmf(mm, vv, K)
    assert got.shape == (72, K)
    rel = np.abs(got - ref) / ref
    print('K = %d: worst relative pmf error %.2e (limit %.1e); smallest pmf %.1e' % (K, rel.max(), TOL_PMF, ref.min()))
    assert rel.max() <= TOL_PMF
    both = plain_ctx.count_probabilities(mm, vv, K=K, level=0.5, k_cap=7, want=['pmf', 'lower', 'upper'])
    assert same(both['pmf'], got)                             # the walk is the same chain with and without the quantiles
    alone = plain_ctx.count_probabilities(mm, vv, level=0.5, k_cap=7, want=['lower', 'upper'])
    assert same(alone['lower'], both['lower']) and same(alone['upper'], both['upper'])


def test_quantiles_saturation_and_levels_near_zero_and_one(plain_ctx):
    mm, vv = (a.reshape(-1) for a in np.meshgrid(GRID_M, (0.0,) + GRID_V, indexing='ij'))
    pmf = rule_pmf(mm, vv, 301)
    for level, k_cap in ((0.95, 300), (1e-6, 300), (1.0 - 1e-6, 300), (0.95, 3), (0.95, 0)):
        got = plain_ctx.count_probabilities(mm, vv, level=level, k_cap=k_cap, want=['lower', 'upper'])
        check_band('level %g' % level, got, pmf, level, k_cap, plain_ctx.info('counts_saturated'))
        assert np.all(got['lower'] <= got['upper']) and got['upper'].max() <= k_cap
    assert plain_ctx.info('counts_saturated') > 0              # (k_cap = 0: every entry whose P(0) is below 0.975)


def test_moments_that_are_not_finite_give_nan_and_refusals_name_the_argument(plain_ctx):
    from funs import _hip
    m = np.array([0.0, np.nan, 0.0, np.inf, 0.5])
    v = np.array([0.1, 0.1, -1.0, 0.1, 0.2])
    got = plain_ctx.count_probabilities(m, v, counts=np.ones(5, np.int32), K=3, level=0.9, k_cap=9, want=ALL)
    bad = np.array([False, True, True, True, False])
    for key in ('logp', 'pmean', 'pvar'):
        assert np.array_equal(np.isnan(got[key]), bad), key
    assert np.array_equal(np.isnan(got['pmf']).all(axis=1), bad) and np.array_equal(np.isnan(got['pmf']).any(axis=1), bad)
    assert np.array_equal(got['lower'] == -1, bad) and np.array_equal(got['upper'] == -1, bad)
    for kw, text in ((dict(K=0, want=['pmf']), 'K = 0'), (dict(K=1025, want=['pmf']), 'K = 1025'), (dict(level=1.0, want=['upper']), 'level'),
                     (dict(k_cap=-1, want=['lower']), 'k_cap'), (dict(want=['logp']), 'logp needs the count'),
                     (dict(counts=np.full(5, -1, np.int32), want=['logp']), 'count -1 of entry 0'), (dict(counts=np.full(5, 65536, np.int32), want=['logp']), 'outside')):
        with pytest.raises(_hip.HipBackendError, match=text):
            plain_ctx.count_probabilities(m, v, **kw)
    with pytest.raises(_hip.HipBackendError, match='counts_nodes'):
        plain_ctx.set_option('counts_nodes', 7)


def test_the_node_count_is_an_option(plain_ctx, grid):
    mm, vv, kk, _ = grid
    try:
        for Q in (8, 48, 64):
            plain_ctx.set_option('counts_nodes', Q)
            err = np.max(np.abs(plain_ctx.count_probabilities(mm, vv, counts=kk, want=['logp'])['logp'] - rule_logp(mm, vv, kk.astype(float), Q)))
            print('Q = %d: worst |delta log P| against the restatement at the same Q %.2e (limit %.1e)' % (Q, err, TOL_LOGP))
            assert err <= TOL_LOGP
    finally:
        plain_ctx.set_option('counts_nodes', 32)


# ---- 2. the resident posterior ------------------------------------------------------------------------------------------------------------------------
def make_ctx(shape, R, engine, kind='laplace', lens=None, observed=None, bins=None):
    """context of the R-trial problem after one Laplace E-step, or after the variational fixed point and its finalize"""
    from funs import _hip
    q, p, T = shape
    par, Y, _ = problem(shape, R=R)
    live = np.ones((R, q, T), bool)
    if lens is not None:
        live &= np.arange(T)[None, None, :] < np.asarray(lens)[:, None, None]
    if observed is not None:
        live &= np.asarray(observed, bool)[:, :, None]
    if bins is not None:
        live &= np.asarray(bins, bool)
    Y = Y * live
    ctx = _hip.Context(q, p, T, R, BIN_MS)
    ctx.upload_counts(Y.astype(np.uint16 if Y.max() > 255 else np.uint8))
    ctx.set_option('cov_mode', engine)
    if kind == 'variational':
        ctx.set_option('dual_lowrank', int(engine == 2))
    ctx.set_params(par['C'], par['d'], par['tau'])
    if lens is not None:
        ctx.set_trial_lengths(np.asarray(lens, dtype=np.int32))
    if observed is not None:
        ctx.set_observed(observed)
    if bins is not None:
        ctx.set_observed_bins(bins)
    if kind == 'variational':
        status = ctx.dual_fixed_point(None, None)[3]
        assert np.all(status != 2), status
        ctx.dual_finalize(None, None)
    else:
        _, _, status = ctx.estep_laplace()
        assert np.all(status == 0), status
    return ctx, par, Y


def reference(eta, var, counts, K, level, k_cap):
    pmf = rule_pmf(eta, var, max(K, k_cap + 1))
    mu = np.exp(eta + 0.5 * var)
    return {'logp': rule_logp(eta, var, counts.astype(float)), 'pmf': pmf, 'pmean': mu, 'pvar': mu + mu * mu * np.expm1(var)}


@pytest.mark.parametrize('kind', ['laplace', 'variational'])
@pytest.mark.parametrize('engine', ENGINES, ids=ENGINE_IDS)
@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_resident_posterior_against_the_rule_on_its_own_moments(case, engine, kind):
    (q, p, T), R = case
    ctx, par, Y = make_ctx((q, p, T), R, engine, kind)
    try:
        before = (ctx.post_mean(), ctx.post_vsm(), ctx.posterior_rates(LIST))
        K, level, k_cap = 12, 0.95, 50
        got = ctx.posterior_counts(LIST, K=K, level=level, k_cap=k_cap, want=ALL)
        sat = ctx.info('counts_saturated')
        assert got['logp'].shape == (5, q, T) and got['pmf'].shape == (5, q, T, K) and got['lower'].dtype == np.int32
        eta, var = before[2]['eta'], before[2]['var']
        ref = reference(eta, var, Y[LIST], K, level, k_cap)
        e_l, e_p = worst(got, (ref['logp'], ref['pmf'][..., :K]))
        print('%s %s %s: worst |delta log P| %.2e, worst relative pmf error %.2e (limits %.1e, %.1e); var up to %.2f'
              % (CASE_IDS[CASES.index(case)], ENGINE_IDS[engine - 1], kind, e_l, e_p, TOL_LOGP, TOL_PMF, var.max()))
        assert e_l <= TOL_LOGP and e_p <= TOL_PMF
        assert np.allclose(got['pmean'], ref['pmean'], rtol=1e-14) and np.allclose(got['pvar'], ref['pvar'], rtol=1e-13)
        check_band('band', got, ref['pmf'], level, k_cap, sat)
        # a list with repeats against one call per trial, and the two entries of trial 0
        for i, t in enumerate(LIST):
            one = ctx.posterior_counts(np.array([t], dtype=np.int32), K=K, level=level, k_cap=k_cap, want=ALL)
            for key in ALL:
                assert same(one[key][0], got[key][i]), (key, i)
        for key in ALL:
            assert same(got[key][1], got[key][4]), key
        # chunks, the counts given, single outputs
        for chunk in (1, 2, 3, 0):
            ctx.set_option('counts_chunk_trials', chunk)
            again = ctx.posterior_counts(LIST, K=K, level=level, k_cap=k_cap, want=ALL)
            for key in ALL:
                assert same(again[key], got[key]), (key, chunk)
        given = ctx.posterior_counts(LIST, counts=Y[LIST].astype(np.int32), want=['logp'])
        assert same(given['logp'], got['logp'])
        assert same(ctx.posterior_counts(LIST, K=K, want=['pmf'])['pmf'], got['pmf'])
        # the resident state and the rates are what they were
        after = (ctx.post_mean(), ctx.post_vsm(), ctx.posterior_rates(LIST))
        assert same(after[0], before[0]) and same(after[1], before[1])
        assert same(after[2]['eta'], eta) and same(after[2]['var'], var)
    finally:
        ctx.close()


def test_refusals_of_the_resident_query_and_their_order():
    from funs import _hip
    q, p, T = 5, 3, 24
    par, Y, _ = problem((q, p, T), R=3)
    ctx = _hip.Context(q, p, T, 3, BIN_MS)
    try:
        assert ctx.lib.pgpfa_posterior_counts(ctx.h, 3, None, None, 1, 0.95, 10, None, None, None, None, None, None) != 0
        assert 'no output asked for' in ctx.lib.pgpfa_last_error().decode()
        with pytest.raises(_hip.HipBackendError, match='set_params has not been called'):
            ctx.posterior_counts(want=['pmean'])
        ctx.set_params(par['C'], par['d'], par['tau'])
        with pytest.raises(_hip.HipBackendError, match='spike counts have not been uploaded'):
            ctx.posterior_counts(want=['logp'])
        ctx.upload_counts(Y.astype(np.uint8))
        with pytest.raises(_hip.HipBackendError, match='trial index 7 out of range'):
            ctx.posterior_counts(np.array([7], dtype=np.int32), want=['pmean'])
        with pytest.raises(_hip.HipBackendError, match='trial 1'):
            ctx.posterior_counts(np.array([1], dtype=np.int32), want=['pmean'])      # no posterior yet
        ctx.estep_laplace()
        with pytest.raises(_hip.HipBackendError, match='count 70000'):
            ctx.posterior_counts(counts=np.full((3, q, T), 70000, np.int32), want=['logp'])
        assert ctx.posterior_counts(want=['pmean'])['pmean'].shape == (3, q, T)
    finally:
        ctx.close()


# ---- 3. ragged trials ---------------------------------------------------------------------------------------------------------------------------------
def test_ragged_trials_padding_cut_planes_and_forecast():
    from funs import util
    shape, lens = (5, 3, 24), (24, 17, 9, 24)
    q, p, T = shape
    ctx, par, Y = make_ctx(shape, 4, 1, lens=lens)
    try:
        got = ctx.posterior_counts(K=4, level=0.9, k_cap=40, want=ALL)
        pad = np.broadcast_to(np.arange(T)[None, None, :] >= np.asarray(lens)[:, None, None], (4, q, T))
        for key in ('logp', 'pmean', 'pvar'):
            assert np.array_equal(np.isnan(got[key]), pad), key
        assert np.array_equal(np.isnan(got['pmf']).all(axis=-1), pad) and np.array_equal(np.isnan(got['pmf']).any(axis=-1), pad)
        assert np.array_equal(got['lower'] == -1, pad) and np.array_equal(got['upper'] == -1, pad)
        rates = ctx.posterior_rates()
    finally:
        ctx.close()
    exp = Experiment([Y[r][:, :L] for r, L in enumerate(lens)], BIN_MS)
    out = util.posteriorCounts(par, exp, maxCount=3, level=0.9, want=('logp', 'pmf', 'lower', 'upper', 'mean', 'var', 'saturated'))
    assert isinstance(out['logp'], list) and [a.shape for a in out['logp']] == [(q, L) for L in lens] and out['pmf'][2].shape == (q, 9, 4)
    assert all(np.isfinite(a).all() for a in out['logp'] + out['mean'] + out['var']) and all((a >= 0).all() for a in out['lower'])
    assert isinstance(out['saturated'], int) and out['saturated'] == sum(int((np.cumsum(a, axis=-1)[..., -1] < 0.95).sum()) for a in out['pmf']) > 0
    assert all(np.array_equal(np.cumsum(a, axis=-1)[..., -1] < 0.95, (u == 3) & (np.cumsum(a, axis=-1)[..., -1] < 0.95)) for a, u in zip(out['pmf'], out['upper']))
    for r, L in enumerate(lens):                             # (the session's E-step is the context's: the same problem)
        assert np.max(np.abs(out['logp'][r] - rule_logp(rates['eta'][r][:, :L], rates['var'][r][:, :L], Y[r][:, :L].astype(float)))) <= 1e-6
    fc = util.posteriorCounts(par, exp, maxCount=3, level=0.9, forecast=True, want=('logp', 'pmf', 'mean', 'upper'))
    assert fc['logp'].shape == (4, q, T) and fc['pmf'].shape == (4, q, T, 4)
    assert np.array_equal(np.isnan(fc['logp']), pad) and np.isfinite(fc['pmf']).all() and np.isfinite(fc['mean']).all() and (fc['upper'] >= 0).all()
    for r, L in enumerate(lens):
        assert same(fc['pmf'][r][:, :L], out['pmf'][r]) and same(fc['logp'][r][:, :L], out['logp'][r])      # in front of T_r: the same bits
    fr = util.posteriorRates(par, exp, forecast=True, want=('eta', 'var'))
    assert np.max(np.abs(fc['pmf'] - rule_pmf(fr['eta'], fr['var'], 4)) / fc['pmf']) <= TOL_PMF
    assert np.allclose(fc['mean'], np.exp(fr['eta'] + 0.5 * fr['var']), rtol=1e-14)


# ---- 4. observation tables ----------------------------------------------------------------------------------------------------------------------------
def test_an_unobserved_neuron_gets_a_prediction_and_no_logp():
    from funs import util
    q, p, T = 5, 3, 24
    par, Y, _ = problem((q, p, T), R=3)
    observed = np.ones((3, q), bool)
    observed[1, 2] = False
    exp = Experiment([Y[r] * observed[r][:, None] for r in range(3)], BIN_MS)
    for r in range(3):
        exp.data[r]['observed'] = observed[r]
    out = util.posteriorCounts(par, exp, maxCount=5, want=('logp', 'pmf', 'mean', 'upper'))
    assert np.array_equal(np.isnan(out['logp']), np.broadcast_to(~observed[:, :, None], (3, q, T)))
    assert np.isfinite(out['pmf']).all() and np.isfinite(out['mean']).all() and (out['upper'] >= 0).all()
    truth = [Y[r] for r in range(3)]
    with_counts = util.posteriorCounts(par, exp, counts=truth, want=('logp',))
    assert np.isfinite(with_counts['logp']).all()
    assert same(with_counts['logp'][observed], out['logp'][observed])


def test_under_a_per_bin_table_logp_needs_the_counts():
    from funs import _hip, util
    q, p, T = 5, 3, 24
    rng = np.random.default_rng(3)
    bins = rng.random((3, q, T)) > 0.2
    ctx, par, Y = make_ctx((q, p, T), 3, 1, bins=bins)
    try:
        with pytest.raises(_hip.HipBackendError, match='per-bin table'):
            ctx.posterior_counts(want=['logp'])
        got = ctx.posterior_counts(counts=Y.astype(np.int32), K=3, want=['logp', 'pmf', 'pmean'])
        rates = ctx.posterior_rates()
        assert np.isfinite(got['logp']).all() and np.isfinite(got['pmf']).all()
        assert np.max(np.abs(got['logp'] - rule_logp(rates['eta'], rates['var'], Y.astype(float)))) <= TOL_LOGP
    finally:
        ctx.close()
    exp = Experiment([Y[r] for r in range(3)], BIN_MS)
    for r in range(3):
        exp.data[r]['observedBins'] = bins[r]
    with pytest.raises(ValueError, match="'logp' needs counts= under a per-bin table"):
        util.posteriorCounts(par, exp)
    out = util.posteriorCounts(par, exp, counts=[Y[r] for r in range(3)], maxCount=2, want=('logp', 'pmf'))
    assert np.isfinite(out['logp']).all() and out['pmf'].shape == (3, q, T, 3)


# ---- 5. the hold-out scores ---------------------------------------------------------------------------------------------------------------------------
RAGGED6 = (24, 17, 24, 9, 20, 13)


@pytest.fixture(scope='module')
def ragged6():
    shape = (6, 2, 24)
    par, Y, _ = problem(shape, R=6, d_offset=0.0)
    return par, Experiment([Y[r][:, :L] for r, L in enumerate(RAGGED6)], BIN_MS), [Y[r][:, :L].astype(float) for r, L in enumerate(RAGGED6)]


def check_scores(tag, pred, plain, hidden_exp, par, truth, scored, rows):
    """the new keys against the formula on the moments of an equivalent masked E-step (util.posteriorRates on an experiment that hides the same entries:
    the same model, the modes to the Newton tolerance); the old keys bit for bit"""
    from funs import util
    for key in plain:
        a, b = plain[key], pred[key]
        assert all(same(x, y) for x, y in zip(a, b)) if isinstance(a, list) else same(np.asarray(a), np.asarray(b)), key
    mv = util.posteriorRates(par, hidden_exp, trials=np.arange(len(truth)), want=('eta', 'var'))
    logp = [rule_logp(mv['eta'][i][rows], mv['var'][i][rows], np.where(sc, y, 0.0)) for i, (y, sc) in enumerate(zip(truth, scored))]
    worst_lp = max(float(np.max(np.abs(np.where(sc, a - b, 0.0)))) for a, b, sc in zip(pred['logPredictive'], logp, scored))
    total, per_row = util._score_predictive(truth, logp, scored)
    print('%s: logPredictive against the rule on an equivalent E-step %.2e (limit 1e-6); bits per spike %.6f against %.6f, plug-in %.6f'
          % (tag, worst_lp, pred['bitsPerSpikePredictive'], total, pred['bitsPerSpike']))
    assert worst_lp <= 1e-6 and abs(pred['bitsPerSpikePredictive'] - total) <= 1e-6
    assert np.allclose(pred['bitsPerSpikePredictivePerNeuron'], per_row, rtol=0, atol=1e-6, equal_nan=True)
    assert all(np.array_equal(np.isnan(a), ~sc) for a, sc in zip(pred['logPredictive'], scored))
    assert same(np.asarray(util._score_predictive(truth, pred['logPredictive'], scored)[0]), np.asarray(pred['bitsPerSpikePredictive']))


def test_bin_holdout_with_the_predictive_score(ragged6):
    from funs import util
    par, exp, truth = ragged6
    hide = util.speckledHoldout(exp, 0.2, seed=4)
    plain = util.binHoldout(par, exp, hide)
    pred = util.binHoldout(par, exp, hide, predictive=True)
    assert sorted(pred) == sorted(list(plain) + ['bitsPerSpikePredictive', 'bitsPerSpikePredictivePerNeuron', 'logPredictive'])
    check_scores('binHoldout', pred, plain, util._with_hidden_entries(exp, hide), par, truth, hide, slice(None))


def test_co_smoothing_with_the_predictive_score(ragged6):
    from funs import util
    par, exp, truth = ragged6
    held = np.array([1, 4])
    plain = util.coSmoothing(par, exp, held)
    pred = util.coSmoothing(par, exp, held, predictive=True)
    assert sorted(pred) == sorted(list(plain) + ['bitsPerSpikePredictive', 'bitsPerSpikePredictivePerNeuron', 'logPredictive'])
    observed = np.ones(6, bool)
    observed[held] = False
    # (a neuron hidden on every trial is observed nowhere, which a session refuses: one silent, fully observed trial behind the six, as coSmoothing adds)
    hidden = Experiment([tr['Y'] * observed[:, None] for tr in exp.data] + [np.zeros((6, 24))], BIN_MS)
    for tr in hidden.data[:6]:
        tr['observed'] = observed
    hidden.data[6]['observed'] = np.ones(6, bool)
    scored = [np.ones((2, L), bool) for L in RAGGED6]
    check_scores('coSmoothing', pred, plain, hidden, par, [y[held] for y in truth], scored, held)


def test_cross_validation_passes_the_keyword_on(ragged6):
    from funs import util
    _, exp, _ = ragged6
    cv = util.crossValidation(exp, numTrainingTrials=5, numTestTrials=1, maxXdim=2, maxEMiter=2, score='speckled', predictive=True, seed=1)
    scored_set, _ = util.splitTrainingTestDataset(exp, 5, 1)
    assert len(cv.errs) == 2 and np.all(np.isfinite(cv.errs))
    for err, fit in zip(cv.errs, cv.fits):
        both = util.binHoldout(fit.optimParams, scored_set, cv.heldOut, predictive=True)
        assert err == -both['bitsPerSpikePredictive'] and err != -both['bitsPerSpike']
    assert cv.optimXdim == int(np.argmin(cv.errs)) + 1


# ---- 6. against the sampler ---------------------------------------------------------------------------------------------------------------------------
def test_frequencies_of_20000_predictive_draws_lie_within_five_standard_errors():
    S = 20000
    ctx, par, Y = make_ctx((5, 3, 24), 3, 1)
    try:
        one = np.array([1], dtype=np.int32)
        pmf = ctx.posterior_counts(one, K=4, want=['pmf'])['pmf'][0]              # (q, T, 4)
        y = ctx.posterior_sample(one, n_samples=S, seed=11, want=['y'])['y'][0]    # (S, q, T)
    finally:
        ctx.close()
    freq = np.stack([(y == k).mean(axis=0) for k in range(4)], axis=-1)
    z = (freq - pmf) / np.sqrt(pmf * (1.0 - pmf) / S)
    print('%d entries x 4 counts: worst |z| %.2f (limit 5), pmf from %.1e to %.2f' % (pmf.shape[0] * pmf.shape[1], np.abs(z).max(), pmf.min(), pmf.max()))
    assert np.all(np.abs(z) <= 5.0)
