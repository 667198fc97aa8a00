"""Posterior firing rates (pgpfa_posterior_rates, Context.posterior_rates, util.posteriorRates, PPGPFAfit.posteriorRates):

    eta = d_n + c_n . m_t,  var = c_n^T Sigma_t c_n,  rate = exp(eta + var / 2),  ell = sum_{t < T_r} y eta - rate,  group sums of the rate.

Part 1 puts synthetic posteriors on the device with set_posterior (no E-step) at shapes on the seams of the kernel's tiles - 16 neurons x 16
bins per wave, 64 / 32 / 16 bins per workgroup at p <= 12 / <= 16 / above, four neuron tiles per workgroup - and compares with plain FP64 numpy.
Tolerances are derived, not measured: a contraction of K <= 560 FP64 terms is off by at most K 2^-53 = 6e-14 of the sum of its absolute terms A;
eta and var are held to 1e-12 A (a margin of 16), ell to 1e-11 sum_t (|y eta| + rate), group sums to 1e-12 of their largest entry.
Part 2 runs real E-steps: the rates against numpy on the device's own posterior (same tolerances) and against the oracle's posterior, where the
E-step's stated 1e-8 on modes and blocks is propagated through |C|.  Every test prints its figures before it asserts."""
import numpy as np
import pytest

from conftest import Experiment, load_golden
from oracle import pgpfa_oracle as orc
from test_gpu_unequal_trials import BIN_MS, _estep_case, _estep_problem, cov_mode, cut, funs_mod, rel  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

SHAPES = [(17, 1, 16, 3), (30, 3, 57, 5), (35, 10, 129, 4), (40, 12, 64, 4), (50, 20, 48, 3), (33, 32, 33, 2)]
IDS = ['q%d-p%d-T%d-R%d' % s for s in SHAPES]
ESTEP_TOL = 1e-8          # modes (absolute) and covariance blocks (of their largest entry): the E-step's own tolerance against the oracle


# ---- synthetic posteriors and their numpy rates -------------------------------------------------------------------------------------------------
def numpy_rates(C, d, mean, vsm):
    """eta, var [R][q][T] and the sums of absolute terms A_eta, A_var the tolerances scale with"""
    eta = d[None, :, None] + np.einsum('nk,rkt->rnt', C, mean)
    var = np.einsum('ni,rtij,nj->rnt', C, vsm, C)
    a_eta = np.abs(d)[None, :, None] + np.einsum('nk,rkt->rnt', np.abs(C), np.abs(mean))
    a_var = np.einsum('ni,rtij,nj->rnt', np.abs(C), np.abs(vsm), np.abs(C))
    return eta, var, a_eta, a_var


def numpy_ell(Y, eta, var, lens):
    """ell [R][q] and the scale sum_t (|y eta| + rate) of its tolerance"""
    live = (np.arange(eta.shape[2])[None, :] < np.asarray(lens)[:, None])[:, None, :]
    rate = np.exp(eta + 0.5 * var)
    return ((Y * eta - rate) * live).sum(axis=2), ((np.abs(Y * eta) + rate) * live).sum(axis=2)


def numpy_groups(eta, var, lens, idx, group, G):
    T = eta.shape[2]
    gs, gc = np.zeros((G,) + eta.shape[1:]), np.zeros((G, T), dtype=np.int32)
    for r, g in zip(idx, group):
        L = int(lens[r])
        gs[g][:, :L] += np.exp(eta[r][:, :L] + 0.5 * var[r][:, :L])
        gc[g][:L] += 1
    return gs, gc


_synth_cache = {}


def _synth(shape):
    """C ~ N(0,1)/sqrt(p), d = -1, post_mean ~ 0.5 N(0,1), Sigma_t = 0.05 A A^T + 0.01 I, counts Poisson of the implied rate; cut lengths with
    T_0 = T, T_1 = 1 and one inside a bin tile.  The (30, 3, 57, 5) case carries a count of 300.  Computed once, shared, never written to."""
    if shape not in _synth_cache:
        q, p, T, R = shape
        rng = np.random.default_rng(1000 * q + p)
        C = rng.standard_normal((q, p)) / np.sqrt(p)
        d = -np.ones(q)
        mean = 0.5 * rng.standard_normal((R, p, T))
        A = rng.standard_normal((R, T, p, p))
        vsm = 0.05 * A @ A.transpose(0, 1, 3, 2) + 0.01 * np.eye(p)
        eta, var, a_eta, a_var = numpy_rates(C, d, mean, vsm)
        Y = rng.poisson(np.exp(eta + 0.5 * var)).astype(np.uint16)
        if shape == SHAPES[1]:
            Y[2, 4, 9] = 300
        lens = np.full(R, T, dtype=np.int32)
        lens[1] = 1
        if R > 2:
            lens[2] = min(T, 16 * (T // 32) + 5)                     # inside a tile of 16 bins (and of the workgroup's 32 / 64)
        if R > 3:
            lens[3:] = rng.integers(2, T + 1, size=R - 3)
        Ycut = Y * (np.arange(T)[None, None, :] < lens[:, None, None])
        out = dict(C=C, d=d, mean=mean, vsm=vsm, eta=eta, var=var, a_eta=a_eta, a_var=a_var, Y=Y, Ycut=Ycut.astype(np.uint16), lens=lens,
                   tau=np.linspace(0.08, 0.3, p))
        for v in out.values():
            v.setflags(write=False)
        _synth_cache[shape] = out
    return _synth_cache[shape]


def _synth_context(shape, ragged=False, full_table=False):
    from funs import _hip
    q, p, T, R = shape
    s = _synth(shape)
    ctx = _hip.Context(q, p, T, R, BIN_MS)
    ctx.upload_counts(np.array(s['Ycut'] if ragged else s['Y']))
    ctx.set_params(s['C'], s['d'], s['tau'])
    if ragged or full_table:
        ctx.set_trial_lengths(s['lens'] if ragged else np.full(R, T, dtype=np.int32))
    ctx.set_posterior(None, s['mean'], s['vsm'])                      # (behind the lengths: a new table drops what was resident)
    return ctx, s


def _group_setup(R):
    """list with trial 1 twice, labels interleaved over groups 0 and 2, group 3 with a single entry, group 1 empty"""
    idx = np.array(list(range(R)) + [1], dtype=np.int32)
    group = np.array([0 if i % 2 == 0 else 2 for i in range(R + 1)], dtype=np.int32)
    group[1] = 3
    return idx, group, 4


ALL = ('eta', 'var', 'ell', 'group_sum', 'group_count')


def check_planes(tag, got, eta, var, a_eta, a_var):
    e_eta, e_var = float(np.max(np.abs(got['eta'] - eta) / a_eta)), float(np.max(np.abs(got['var'] - var) / a_var))
    print('%s: eta %.2e of A, var %.2e of A (limit 1e-12), smallest var %.3e' % (tag, e_eta, e_var, got['var'].min()))
    assert e_eta <= 1e-12 and e_var <= 1e-12
    assert np.all(got['var'] >= 0.0)


# ---- 1. synthetic posteriors against numpy ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ragged', [False, True], ids=['equal', 'cut'])
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_all_outputs_against_numpy(shape, ragged):
    """eta, var, ell, group_sum and group_count of one call: every bin of eta / var (padded ones included), ell and the groups up to T_r"""
    q, p, T, R = shape
    ctx, s = _synth_context(shape, ragged)
    try:
        idx, group, G = _group_setup(R)
        got = ctx.posterior_rates(idx, group=group, n_groups=G, want=ALL)
        assert ctx.info('counts_two_bytes') == float(shape == SHAPES[1])
        lens = s['lens'] if ragged else np.full(R, T)
        tag = 'q=%d p=%d T=%d R=%d %s' % (q, p, T, R, 'cut' if ragged else 'equal')
        check_planes(tag, got, s['eta'][idx], s['var'][idx], s['a_eta'][idx], s['a_var'][idx])
        ell, scale = numpy_ell(np.asarray(s['Ycut'] if ragged else s['Y'], dtype=np.float64), s['eta'], s['var'], lens)
        e_ell = float(np.max(np.abs(got['ell'] - ell[idx]) / scale[idx]))
        gs, gc = numpy_groups(s['eta'], s['var'], lens, idx, group, G)
        e_gs = float(np.max(np.abs(got['group_sum'] - gs)) / np.max(np.abs(gs)))
        print('%s: ell %.2e of its scale (limit 1e-11), group_sum %.2e of its maximum (limit 1e-12)' % (tag, e_ell, e_gs))
        assert e_ell <= 1e-11 and e_gs <= 1e-12
        assert got['group_count'].dtype == np.int32 and np.array_equal(got['group_count'], gc)
        assert not got['group_sum'][1].any() and not got['group_count'][1].any()             # the empty group
        assert np.array_equal(got['group_count'][3], (np.arange(T) < lens[1]).astype(np.int32))   # the group of one entry
    finally:
        ctx.close()


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_chunks_null_outputs_and_runs_give_the_same_bits(shape):
    """rates_chunk_trials 1, 2 and 0, a second run, and every output asked for alone: bit-identical to the one call with all outputs"""
    q, p, T, R = shape
    ctx, s = _synth_context(shape, ragged=True)
    try:
        idx, group, G = _group_setup(R)
        base = ctx.posterior_rates(idx, group=group, n_groups=G, want=ALL)
        for chunk in (1, 2, 0, 0):
            ctx.set_option('rates_chunk_trials', chunk)
            got = ctx.posterior_rates(idx, group=group, n_groups=G, want=ALL)
            for k in ALL:
                assert np.array_equal(got[k], base[k]), (chunk, k)
        for chunk in (2, 0):
            ctx.set_option('rates_chunk_trials', chunk)
            for k in ALL:
                one = ctx.posterior_rates(idx, group=group, n_groups=G, want=(k,))
                assert list(one) == [k] and np.array_equal(one[k], base[k]), (chunk, k)
            # per-trial outputs do not need the table
            for k in ('eta', 'var', 'ell'):
                assert np.array_equal(ctx.posterior_rates(idx, want=(k,))[k], base[k]), (chunk, k)
        with pytest.raises(Exception, match='rates_chunk_trials'):
            ctx.set_option('rates_chunk_trials', -1)
    finally:
        ctx.close()


@pytest.mark.parametrize('shape', [SHAPES[1], SHAPES[2]], ids=[IDS[1], IDS[2]])
def test_a_table_of_full_lengths_changes_no_bit(shape):
    q, p, T, R = shape
    idx, group, G = _group_setup(R)
    got = []
    for full_table in (False, True):
        ctx, _ = _synth_context(shape, full_table=full_table)
        try:
            assert ctx.info('trial_lengths_set') == float(full_table)
            got.append(ctx.posterior_rates(idx, group=group, n_groups=G, want=ALL))
        finally:
            ctx.close()
    for k in ALL:
        assert np.array_equal(got[0][k], got[1][k]), k


def test_refusals():
    from funs import _hip
    shape = SHAPES[1]
    q, p, T, R = shape
    s = _synth(shape)
    ctx = _hip.Context(q, p, T, R, BIN_MS)
    try:
        ctx.upload_counts(np.array(s['Y']))
        ctx.set_params(s['C'], s['d'], s['tau'])
        with pytest.raises(_hip.HipBackendError, match='no posterior for trial 0'):
            ctx.posterior_rates()
        ctx.set_posterior(np.array([0, 2], dtype=np.int32), s['mean'][[0, 2]], s['vsm'][[0, 2]])
        with pytest.raises(_hip.HipBackendError, match='no posterior for trial 3'):
            ctx.posterior_rates(np.array([2, 0, 3, 1], dtype=np.int32))
        two = np.array([2, 0], dtype=np.int32)
        assert ctx.posterior_rates(two)['eta'].shape == (2, q, T)
        for bad in ([0, 2], [-1, 0]):
            with pytest.raises(_hip.HipBackendError, match='group id'):
                ctx.posterior_rates(two, group=np.array(bad, dtype=np.int32), n_groups=2, want=('group_sum',))
        for k in ('group_sum', 'group_count'):
            with pytest.raises(_hip.HipBackendError, match='needs the trial -> group table'):
                ctx.posterior_rates(two, want=(k,))
        with pytest.raises(_hip.HipBackendError, match='no output'):
            ctx.posterior_rates(two, want=())
        ctx.upload_counts(np.array(s['Y']))                             # new counts: the posterior of every trial is gone
        with pytest.raises(_hip.HipBackendError, match='no posterior for trial 2'):
            ctx.posterior_rates(two)
    finally:
        ctx.close()


# ---- 2. end to end: Laplace ----------------------------------------------------------------------------------------------------------------------
_equal_cache = {}


def _c1_oracle(ragged):
    """(params, trials, lengths, T, oracle posterior per trial - of the truncated trials where ragged, with post_cov)"""
    if ragged:
        params, Yr, lens, T, ref, _ = _estep_case('c1')
        return params, Yr, lens, T, ref
    if 'c1' not in _equal_cache:
        params, Ys, T = _estep_problem('c1')
        ref, _, _ = orc.laplace(Ys, params, BIN_MS, mode='exact', return_cov=False)
        _equal_cache['c1'] = (params, Ys, np.full(len(Ys), T, dtype=np.int32), T, ref)
    return _equal_cache['c1']


def _c1_context(engine, ragged):
    from funs import _hip
    params, Yr, lens, T, ref = _c1_oracle(ragged)
    Y = np.zeros((len(Yr), Yr[0].shape[0], T), dtype=np.uint8)
    for r, y in enumerate(Yr):
        Y[r, :, :y.shape[1]] = y
    ctx = _hip.Context(Y.shape[1], params['C'].shape[1], T, len(Yr), BIN_MS)
    ctx.upload_counts(Y)
    ctx.set_option('cov_mode', engine)
    ctx.set_params(params['C'], params['d'], params['tau'])
    if ragged:
        ctx.set_trial_lengths(lens)
    _, _, status = ctx.estep_laplace()
    assert np.all(status == 0) and ctx.info('last_cov_lowrank') == float(engine == 2)
    return ctx, params, Y, lens, T, ref


@pytest.mark.parametrize('engine', [1, 2], ids=['dense', 'lowrank'])
@pytest.mark.parametrize('ragged', [False, True], ids=['equal', 'cut'])
def test_laplace_rates_on_config1(engine, ragged):
    """estep_laplace, then rates: against numpy on the device's own post_mean / post_vsm at the rounding tolerances, and against numpy on the
    oracle's posterior of the (truncated) trials, where a mode off by 1e-8 moves eta by at most 1e-8 sum_k |C_nk| and blocks off by 1e-8 of
    their largest entry move var by at most 1e-8 max|Sigma| (sum_k |C_nk|)^2 (plus the rounding terms)."""
    ctx, params, Y, lens, T, ref = _c1_context(engine, ragged)
    try:
        C, d = np.asarray(params['C'], dtype=np.float64), np.asarray(params['d'], dtype=np.float64).reshape(-1)
        got = ctx.posterior_rates(want=('eta', 'var', 'ell'))
        eta, var, a_eta, a_var = numpy_rates(C, d, ctx.post_mean(), ctx.post_vsm())
        tag = 'config 1 %s, engine %d' % ('cut' if ragged else 'equal', engine)
        check_planes(tag + ', device posterior', got, eta, var, a_eta, a_var)
        ell, scale = numpy_ell(Y.astype(np.float64), eta, var, lens)
        e_ell = float(np.max(np.abs(got['ell'] - ell) / scale))
        c1n = np.abs(C).sum(axis=1)                                    # sum_k |C_nk|
        worst = [0.0, 0.0]
        for r in range(len(lens)):
            L = int(lens[r])
            m, S = np.asarray(ref['post_mean'][r]), np.asarray(ref['post_vsm'][r])
            e_o, v_o, ae, av = numpy_rates(C, d, m[None], S[None])
            tol_eta = ESTEP_TOL * c1n[:, None] + 1e-12 * ae[0]
            tol_var = ESTEP_TOL * np.max(np.abs(S)) * (c1n ** 2)[:, None] + 1e-12 * av[0]
            worst[0] = max(worst[0], float(np.max(np.abs(got['eta'][r][:, :L] - e_o[0]) / tol_eta)))
            worst[1] = max(worst[1], float(np.max(np.abs(got['var'][r][:, :L] - v_o[0]) / tol_var)))
        print('%s: ell %.2e of its scale (limit 1e-11); against the oracle eta %.3f and var %.3f of the propagated bound' % (tag, e_ell, worst[0], worst[1]))
        assert e_ell <= 1e-11 and worst[0] <= 1.0 and worst[1] <= 1.0
    finally:
        ctx.close()


@pytest.mark.parametrize('engine', [1, 2], ids=['dense', 'lowrank'])
def test_padded_bins_hold_the_forecast(engine):
    """Behind a trial's length the posterior is the GP conditional on the trial's own bins: with A_k = K_PL K_LL^-1 of latent k (dense numpy),
    mean_P = A_k m_L and Sigma_PP[i][j] = delta_ij (K_PP - A_i K_LP) + A_i Sigma_LL[i][j] A_j^T, Sigma_LL the oracle's posterior covariance of the
    truncated trial.  eta and var of the padded bins against numpy on these, at the propagated E-step tolerance of the test above."""
    ctx, params, Y, lens, T, ref = _c1_context(engine, True)
    try:
        C, d = np.asarray(params['C'], dtype=np.float64), np.asarray(params['d'], dtype=np.float64).reshape(-1)
        p = C.shape[1]
        K = orc.make_K(params['tau'], T, BIN_MS)
        got = ctx.posterior_rates(want=('eta', 'var'))
        c1n = np.abs(C).sum(axis=1)
        worst, n_checked = [0.0, 0.0], 0
        for r in np.flatnonzero(lens < T)[:6]:
            L, P = int(lens[r]), T - int(lens[r])
            A = np.stack([np.linalg.solve(K[k][:L, :L], K[k][:L, L:]).T for k in range(p)])          # [p][P][L]
            mean_P = np.einsum('kpl,kl->kp', A, np.asarray(ref['post_mean'][r]))
            cov = np.asarray(ref['post_cov'][r]).reshape(p, L, p, L)
            S = np.einsum('ipl,iljm,jpm->pij', A, cov, A)                                             # [P][p][p]
            for k in range(p):
                S[:, k, k] += np.diag(K[k][L:, L:] - A[k] @ K[k][:L, L:])
            e_o, v_o, ae, av = numpy_rates(C, d, mean_P[None], S[None])
            tol_eta = ESTEP_TOL * c1n[:, None] + 1e-12 * ae[0]
            tol_var = ESTEP_TOL * max(np.max(np.abs(S)), np.max(np.abs(ref['post_vsm'][r]))) * (c1n ** 2)[:, None] + 1e-12 * av[0]
            worst[0] = max(worst[0], float(np.max(np.abs(got['eta'][r][:, L:] - e_o[0]) / tol_eta)))
            worst[1] = max(worst[1], float(np.max(np.abs(got['var'][r][:, L:] - v_o[0]) / tol_var)))
            n_checked += P
        print('engine %d: %d padded bins, eta %.3f and var %.3f of the propagated bound' % (engine, n_checked, worst[0], worst[1]))
        assert n_checked > 0 and worst[0] <= 1.0 and worst[1] <= 1.0
    finally:
        ctx.close()


# ---- 3. end to end: variational --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('engine', [1, 2], ids=['dense', 'lowrank'])
def test_variational_rates_are_the_reference_dual_gradient(engine):
    """After dual_finalize(idx, lam) at an arbitrary positive lam the resident posterior is VIPostMean / VIPostCov at lam, and the reference's dual
    gradient (inference.py:215-219) is exactly log lam - (eta + var / 2).  Against orc.dual_grad (dense numpy, jitter included) at 1e-8 of its
    largest entry: the tolerance test_gpu_parity.py holds pgpfa_dual_costgrad_batch's gradient to against the same oracle function."""
    from funs import _hip
    g = load_golden('var_toy.npz')
    Y = g['Y']
    R, q, T = Y.shape
    par = {'C': g['init_C'], 'd': g['init_d'], 'tau': g['init_tau']}
    p = par['C'].shape[1]
    K_big = orc.make_K_big(orc.make_K(par['tau'], T, float(g['binSize'])))
    C_big, d_big = orc.make_Cd_big(par['C'], par['d'], T)
    Kinv_big = np.linalg.inv(K_big)
    idx = np.array([3, 0, 7], dtype=np.int32)
    lam = 0.2 + np.random.default_rng(2).random((3, q * T))
    ctx = _hip.Context(q, p, T, R, float(g['binSize']))
    try:
        ctx.upload_counts(Y)
        ctx.set_option('cov_mode', engine)
        ctx.set_option('dual_lowrank', int(engine == 2))
        ctx.set_params(par['C'], par['d'], par['tau'])
        ctx.dual_finalize(idx, lam)
        got = ctx.posterior_rates(idx)
        for i, tr in enumerate(idx):
            ref = orc.dual_grad(lam[i], Y[tr].reshape(-1).astype(np.float64), C_big, K_big, Kinv_big, d_big)
            dev = np.log(lam[i]) - (got['eta'][i] + 0.5 * got['var'][i]).reshape(-1)
            err = rel(dev, ref)
            print('engine %d, trial %d: log lam - (eta + var / 2) against the dual gradient %.2e (limit 1e-8)' % (engine, tr, err))
            assert err <= 1e-8
    finally:
        ctx.close()


# ---- 4. the Python surface --------------------------------------------------------------------------------------------------------------------------
def _c1_init():
    g = load_golden('c1_dataset.npz')
    return [g['Y'][r].astype(np.float64) for r in range(g['Y'].shape[0])], {'C': g['init_C'].copy(), 'd': g['init_d'].copy(), 'tau': g['init_tau'].copy()}


def test_util_posterior_rates_on_config1(funs_mod):
    from funs import _session
    _session.drop_sessions()
    Ys, params = _c1_init()
    exp = Experiment(Ys, BIN_MS)
    util, inference = funs_mod.util, funs_mod.inference
    cond = np.arange(len(Ys)) % 3 + 10
    keys = ('rate', 'lower', 'upper', 'median', 'eta', 'var', 'ell')
    own = util.posteriorRates(params, exp, conditions=cond, want=keys)                    # runs its own E-step
    infRes, _ = inference.laplace(exp, {k: v.copy() for k, v in params.items()}, returnOptimRes=False)
    out = util.posteriorRates(params, exp, infRes=infRes, conditions=cond, want=keys)      # the resident posterior of that one
    C, d = params['C'], params['d']
    m, S = np.stack([infRes['post_mean'][r] for r in range(len(Ys))]), np.stack([infRes['post_vsm'][r] for r in range(len(Ys))])
    eta, var, a_eta, a_var = numpy_rates(C, d, m, S)
    check_planes('util.posteriorRates, config 1', out, eta, var, a_eta, a_var)
    assert np.array_equal(own['eta'], out['eta']) or np.max(np.abs(own['eta'] - out['eta'])) <= 2 * ESTEP_TOL * np.abs(C).sum(axis=1).max()
    per_s = 1000.0 / BIN_MS                                                               # spikes per second
    assert np.allclose(out['rate'], np.exp(eta + 0.5 * var) * per_s, rtol=1e-12) and out['rate'].shape == (20, 30, 100)
    mean_count = np.mean(Ys)
    assert mean_count * per_s / 3.0 < out['rate'].mean() < 3.0 * mean_count * per_s       # the scale of the data, in Hz
    assert np.all(out['lower'] <= out['median']) and np.all(out['median'] <= out['rate']) and np.all(out['rate'] <= out['upper'])
    assert out['condition_labels'].tolist() == [10, 11, 12] and np.array_equal(out['condition_count'], np.stack([np.full(100, (cond == c).sum()) for c in (10, 11, 12)]))
    for gi, c in enumerate((10, 11, 12)):
        assert rel(out['condition_mean'][gi], out['rate'][cond == c].mean(axis=0)) <= 1e-12
    assert out['ell'].shape == (20, 30)
    only = util.posteriorRates(params, exp, infRes=infRes, conditions=cond, want=())
    assert sorted(only) == ['condition_count', 'condition_labels', 'condition_mean'] and np.array_equal(only['condition_mean'], out['condition_mean'])
    sub = util.posteriorRates(params, exp, infRes=infRes, trials=[4, 4, 17], want=('rate',))
    assert np.array_equal(sub['rate'], out['rate'][[4, 4, 17]])
    inference.laplace(exp, {k: v.copy() for k, v in params.items()}, returnOptimRes=False)
    with pytest.raises(ValueError, match='superseded'):
        util.posteriorRates(params, exp, infRes=infRes)
    _session.drop_sessions()


def test_fit_posterior_rates_on_cut_config1(funs_mod):
    from funs import _session
    _session.drop_sessions()
    Ys, params = _c1_init()
    lens = np.full(len(Ys), 100)
    lens[[1, 5, 6, 12]] = [50, 57, 83, 64]
    exp = Experiment(cut(Ys, lens), BIN_MS)
    fit = funs_mod.engine.PPGPFAfit(exp, initParams=params, EMmode='Batch', maxEMiter=2, CdOptimMethod='newton', quiet=True)
    out = fit.posteriorRates(conditions=np.arange(20) // 10, want=('rate', 'lower', 'upper'))
    assert fit.rates is out and isinstance(out['rate'], list) and [a.shape for a in out['rate']] == [(30, int(L)) for L in lens]
    assert fit.infRes['post_mean'][3].shape == (3, 100)                                   # kept on the host before the E-step superseded it
    full = fit.posteriorRates(forecast=True, want=('rate',))
    assert isinstance(full['rate'], np.ndarray) and full['rate'].shape == (20, 30, 100)
    for r in (0, 1, 12):
        assert np.allclose(out['rate'][r], full['rate'][r][:, :lens[r]], rtol=1e-6)         # (two E-steps from different starts)
        assert np.all(out['lower'][r] <= out['rate'][r]) and np.all(out['rate'][r] <= out['upper'][r])
    assert out['condition_count'][0].tolist() == [10] * 50 + [9] * 7 + [8] * 26 + [7] * 17 and out['condition_count'][1].tolist() == [10] * 64 + [9] * 36
    mean0 = np.mean([out['rate'][r][:, 60] for r in range(10) if lens[r] > 60], axis=0)
    assert rel(out['condition_mean'][0][:, 60], mean0) <= 1e-12
    _session.drop_sessions()
