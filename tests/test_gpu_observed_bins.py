"""Per-bin observation masks in the Laplace EM path (pgpfa_set_observed_bins, experiment.data[r]['observedBins']).

An entry (trial, neuron, bin) that is not live carries no likelihood term; the prior is unchanged, so posterior, objective and evidence of a
trial are those of the model marginalised over its dead entries.  The oracle cannot take an entry mask: the yardstick of every E-step check is
the numpy restatement of test_cpu_observed_bins.py (masked_laplace: dense Newton to a gradient of 1e-10, blocks from the inverse Hessian), which
that file pins to the oracle's big-matrix forms.  The (C,d) passes are held to plain FP64 numpy summed over live entries.  Eight trials per
shape take the eight patterns of pattern_masks in turn (all live | 20 % speckle | seam neurons x seam bins | a whole row and a 16-bin window |
a whole 64-bin block | one live entry | checkerboard | what lengths + 'observed' express); the shapes cross 16-neuron tiles, 16-bin tiles,
64-bin words and the four (C,d) tile widths.

Tolerances are the project's own (test_gpu_observed_neurons.py): modes 1e-8, covariance blocks 1e-8 relative, nPLL 1e-9 relative, evidence
1e-9, (C,d) cost 1e-10, gradient, steps and decrements 1e-9.  Every test prints the figures it measured before it asserts."""
import numpy as np
import pytest

from conftest import Experiment, load_golden
from oracle import pgpfa_oracle as orc
import test_cpu_observed_bins as ob
import test_gpu_mstep_dense as dense
from test_gpu_unequal_trials import BIN_MS, _estep_problem, cov_mode, funs_mod, ragged_lengths, rel  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

INV_S2 = dense.INV_S2
R8 = 8


@pytest.fixture(scope='module', autouse=True)
def _leave_nothing_behind():
    yield
    import gc
    from funs import _session
    _session.drop_sessions()
    _cases.clear()
    _cd_cache.clear()
    gc.collect()


# ---- problems and references: computed once, shared, never written to ---------------------------------------------------------------------------
def _problem(name):
    """(params, 8 equal-length trials, T): config 1's first 8 trials, or the synthetic sets of the other files with 8 trials"""
    if name == 'c1':
        params, Ys, T = _estep_problem('c1')
        return params, Ys[:R8], T
    q, p, T = {'p10': (40, 10, 176), 'p12': (35, 12, 64), 'p20': (50, 20, 48)}[name]
    params, Ys, _ = orc.synth_dataset(q, p, T, R8, seed=31 + p)
    return params, Ys, T


_cases = {}


def _case(name, ragged=False):
    """params, trials (cut where ragged), the bin table (R, q, T), lengths, 'observed' (R, q) or None, T, the references per trial.  ragged: trials
    cut to lengths in T/2..T AND an 'observed' table that hides neuron 1 on trial 1 and neurons 5, 20 on trial 6, on top of the patterns."""
    if (name, ragged) not in _cases:
        params, Ys, T = _problem(name)
        q = Ys[0].shape[0]
        bins = ob.pattern_masks(R8, q, T)
        lens = np.full(R8, T, dtype=np.int32)
        observed = None
        if ragged:
            lens = ragged_lengths(R8, T, seed=len(name) + T, n_distinct=4)
            lens[5] = T                                              # (the single live entry (17, 33) of trial 5 stays inside its trial)
            observed = np.ones((R8, q), dtype=bool)
            observed[1, 1] = False
            observed[6, [5, 20]] = False
        Yr = [np.ascontiguousarray(np.asarray(y, dtype=np.float64)[:, :L]) for y, L in zip(Ys, lens)]
        live = [bins[r, :, :L] & (True if observed is None else observed[r][:, None]) for r, L in enumerate(lens)]
        assert all(l.any() for l in live)
        ref = [ob.masked_laplace(Yr[r], live[r], params) for r in range(R8)]
        _cases[(name, ragged)] = (params, Yr, bins, lens, observed, T, live, ref)
    return _cases[(name, ragged)]


def bins_experiment(Yr, bins, observed=None, nan=False):
    """Experiment whose trials carry 'observedBins' (cut to their own bins) and 'observed'; the counts at dead entries are left in place (the
    session must ignore them) or set to NaN"""
    exp = Experiment(Yr, BIN_MS)
    for r, tr in enumerate(exp.data):
        L = tr['Y'].shape[1]
        tr['observedBins'] = bins[r, :, :L].copy()
        if observed is not None:
            tr['observed'] = observed[r].copy()
        if nan:
            tr['Y'] = tr['Y'].copy()
            tr['Y'][~tr['observedBins']] = np.nan
    return exp


def padded_counts(Yr, live, T):
    Y = np.zeros((len(Yr), Yr[0].shape[0], T), dtype=np.uint8)
    for r, y in enumerate(Yr):
        Y[r, :, :y.shape[1]] = np.where(live[r], y, 0)
    return Y


def _compare_posterior(tag, infRes, optim, ref, lens, p, nll, trials=None):
    e_m = e_v = e_g = 0.0
    trials = range(len(lens)) if trials is None else trials
    for r in trials:
        L = int(lens[r])
        m, v, gp = infRes['post_mean'][r], infRes['post_vsm'][r], infRes['post_vsmGP'][r]
        assert m.shape == (p, L) and v.shape == (L, p, p) and gp.shape == (L, L, p) and np.array_equal(optim[r], m.reshape(-1))
        e_m = max(e_m, float(np.max(np.abs(m - ref[r]['post_mean']))))
        e_v = max(e_v, rel(v, ref[r]['post_vsm']))
        e_g = max(e_g, rel(gp, ref[r]['post_vsmGP']))
    nll_ref = -float(np.mean([ref[r]['nlp'] for r in trials]))      # (inference.laplace returns minus the mean objective)
    e_f = abs(nll - nll_ref) / abs(nll_ref)
    print('%s: modes %.2e, post_vsm %.2e, post_vsmGP %.2e, nPLL %.2e' % (tag, e_m, e_v, e_g, e_f))
    assert e_m <= 1e-8 and e_v <= 1e-8 and e_g <= 1e-8 and e_f <= 1e-9


# ---- 1. E-step against numpy on the reduced model -----------------------------------------------------------------------------------------------
@pytest.mark.timeout(900)
@pytest.mark.parametrize('cov_mode', [1, 2], indirect=True, ids=['dense', 'lowrank'])
@pytest.mark.parametrize('name', ['c1', 'p10', 'p12', 'p20'])
def test_estep_against_numpy_on_the_live_entries(funs_mod, name, cov_mode):
    """inference.laplace on an experiment with 'observedBins', cold start, under both covariance engines: post_mean 1e-8, post_vsm and post_vsmGP
    1e-8 relative, nPLL 1e-9 relative against masked_laplace per trial.  The dead entries of 'Y' hold NaN: nothing may read them."""
    params, Yr, bins, lens, observed, T, live, ref = _case(name)
    p = params['C'].shape[1]
    exp = bins_experiment(Yr, bins, nan=True)
    infRes, nll, optim = funs_mod.inference.laplace(exp, {k: v.copy() for k, v in params.items()})
    ctx = infRes.session.ctx
    assert ctx.info('observed_bins_set') == 1.0 and ctx.info('observed_set') == 0.0 and ctx.info('trial_lengths_set') == 0.0
    assert np.all(infRes.newton_status == 0) and ctx.info('last_cov_lowrank') == float(cov_mode == 2)
    _compare_posterior('%s, engine %d, cold start' % (name, cov_mode), infRes, optim, ref, lens, p, nll)
    infRes, nll, optim = funs_mod.inference.laplace(exp, {k: v.copy() for k, v in params.items()}, prevOptimRes=optim)
    _compare_posterior('%s, engine %d, resident start' % (name, cov_mode), infRes, optim, ref, lens, p, nll)


@pytest.mark.parametrize('cov_mode', [1, 2], indirect=True, ids=['dense', 'lowrank'])
@pytest.mark.parametrize('name,option', [('p20', 'dual_gemm'), ('p10', 'use_mfma')])
def test_vector_poisson_pass_against_numpy(name, option, cov_mode):
    """poisson_pass_kernel under the same yardstick, at the C-ABI and under both covariance engines: option dual_gemm = 0 selects it at 20 latents,
    use_mfma = 0 (set before the parameters) at 10.  Modes 1e-8, blocks 1e-8, objective 1e-9 relative, cold start."""
    from funs import _hip
    params, Yr, bins, lens, observed, T, live, ref = _case(name)
    q, p = Yr[0].shape[0], params['C'].shape[1]
    total = sum(r['nlp'] for r in ref)
    ctx = _hip.Context(q, p, T, R8, BIN_MS)
    try:
        ctx.upload_counts(padded_counts(Yr, live, T))
        ctx.set_option(option, 0)
        ctx.set_option('cov_mode', cov_mode)
        ctx.set_params(params['C'], params['d'], params['tau'])
        ctx.set_observed_bins(bins)
        obj, _, st = ctx.estep_laplace(warm_start=False)
        assert np.all(st == 0) and ctx.info('last_cov_lowrank') == float(cov_mode == 2)
        M, V, G = ctx.post_mean(), ctx.post_vsm(), ctx.post_vsmgp()
        e_m = max(float(np.max(np.abs(M[r] - ref[r]['post_mean']))) for r in range(R8))
        e_v = max(rel(V[r], ref[r]['post_vsm']) for r in range(R8))
        e_g = max(rel(G[r], ref[r]['post_vsmGP']) for r in range(R8))
        e_f = abs(obj - total) / abs(total)
        print('%s, vector Poisson pass (%s = 0), engine %d: modes %.2e, post_vsm %.2e, post_vsmGP %.2e, objective %.2e' % (name, option, cov_mode, e_m, e_v, e_g, e_f))
        assert e_m <= 1e-8 and e_v <= 1e-8 and e_g <= 1e-8 and e_f <= 1e-9
    finally:
        ctx.close()


@pytest.mark.timeout(900)
@pytest.mark.parametrize('cov_mode', [1, 2], indirect=True, ids=['dense', 'lowrank'])
@pytest.mark.parametrize('name', ['c1', 'p10'])
def test_table_together_with_lengths_and_observed(funs_mod, name, cov_mode):
    """Trials cut to lengths in T/2..T, rows hidden by 'observed' AND the bin patterns: numpy on the model with the three tables folded together"""
    params, Yr, bins, lens, observed, T, live, ref = _case(name, ragged=True)
    p = params['C'].shape[1]
    exp = bins_experiment(Yr, bins, observed)
    infRes, nll, optim = funs_mod.inference.laplace(exp, {k: v.copy() for k, v in params.items()})
    ctx = infRes.session.ctx
    assert ctx.info('observed_bins_set') == 1.0 and ctx.info('observed_set') == 1.0 and ctx.info('trial_lengths_set') == 1.0
    assert np.all(infRes.newton_status == 0)
    _compare_posterior('%s with lengths and observed, engine %d' % (name, cov_mode), infRes, optim, ref, lens, p, nll)


@pytest.mark.parametrize('cov_mode', [1, 2], indirect=True, ids=['dense', 'lowrank'])
def test_the_expressible_pattern_against_the_lengths_and_observed_path(funs_mod, cov_mode):
    """Pattern 8 (t < T/2 and n even live) on trials 1..7 of config 1 (trial 0 stays whole: every neuron needs a live entry somewhere), once as
    'observedBins' and once as trials cut to T/2 bins with 'observed': the first T/2 bins of the padded posterior are the posterior of the cut
    model (the GP prior is consistent under marginalisation) - modes 1e-8, blocks 1e-8 relative, nPLL 1e-9 relative between the two paths."""
    from funs import _session
    params, Ys, T = _problem('c1')
    q, p = Ys[0].shape[0], params['C'].shape[1]
    lens = np.array([T] + [T // 2] * (R8 - 1))
    pat = ob.pattern_masks(R8, q, T)[7]
    a_exp = bins_experiment(Ys, np.stack([np.ones_like(pat)] + [pat] * (R8 - 1)))
    a, nll_a, _ = funs_mod.inference.laplace(a_exp, {k: v.copy() for k, v in params.items()})
    assert a.session.ctx.info('observed_bins_set') == 1.0 and a.session.ctx.info('trial_lengths_set') == 0.0
    got = [(np.array(a['post_mean'][r]), np.array(a['post_vsm'][r]), np.array(a['post_vsmGP'][r])) for r in range(R8)]
    _session.drop_sessions(a_exp)
    b_exp = Experiment([np.ascontiguousarray(y[:, :L]) for y, L in zip(Ys, lens)], BIN_MS)
    for tr in b_exp.data[1:]:
        tr['observed'] = np.arange(q) % 2 == 0
    b, nll_b, _ = funs_mod.inference.laplace(b_exp, {k: v.copy() for k, v in params.items()})
    ctx = b.session.ctx
    assert ctx.info('observed_bins_set') == 0.0 and ctx.info('observed_set') == 1.0 and ctx.info('trial_lengths_set') == 1.0
    e_m = max(float(np.max(np.abs(got[r][0][:, :L] - b['post_mean'][r]))) for r, L in enumerate(lens))
    e_v = max(rel(got[r][1][:L], b['post_vsm'][r]) for r, L in enumerate(lens))
    e_g = max(rel(got[r][2][:L, :L], b['post_vsmGP'][r]) for r, L in enumerate(lens))
    e_f = abs(nll_a - nll_b) / abs(nll_b)
    print('pattern 8 as a bin table against lengths + observed, engine %d: modes %.2e, post_vsm %.2e, post_vsmGP %.2e, nPLL %.2e' % (cov_mode, e_m, e_v, e_g, e_f))
    assert e_m <= 1e-8 and e_v <= 1e-8 and e_g <= 1e-8 and e_f <= 1e-9


# ---- 2. the evidence --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cov_mode', [1, 2], indirect=True, ids=['dense', 'lowrank'])
@pytest.mark.parametrize('name,ragged', [('c1', False), ('p10', False), ('c1', True)], ids=['c1', 'p10', 'c1-ragged'])
def test_log_evidence_with_a_bin_table(funs_mod, name, ragged, cov_mode):
    """LAPLACE_EVIDENCE: log Z_r to 1e-9 relative against -f - (log det H + log det K) / 2 of the reduced model in numpy"""
    params, Yr, bins, lens, observed, T, live, ref = _case(name, ragged)
    want = np.array([r['logZ'] for r in ref])
    old = funs_mod.inference.LAPLACE_EVIDENCE
    funs_mod.inference.LAPLACE_EVIDENCE = True
    try:
        infRes, _, _ = funs_mod.inference.laplace(bins_experiment(Yr, bins, observed), {k: v.copy() for k, v in params.items()})
    finally:
        funs_mod.inference.LAPLACE_EVIDENCE = old
    assert infRes.session.ctx.info('observed_bins_set') == 1.0 and np.all(infRes.newton_status == 0)
    e_z = float(np.max(np.abs(infRes.log_evidence - want) / np.abs(want)))
    e_m = abs(infRes.mean_log_evidence - want.mean()) / abs(want.mean())
    print('%s%s, engine %d: log Z per trial %.2e, mean %.2e (mean log Z %.6f)' % (name, ' ragged' if ragged else '', cov_mode, e_z, e_m, want.mean()))
    assert e_z <= 1e-9 and e_m <= 1e-9


# ---- 3. the (C,d) passes -----------------------------------------------------------------------------------------------------------------------------
CD_CASES = {'p3': (30, 3, 100), 'p10': (40, 10, 176), 'p12': (35, 12, 64), 'p20': (50, 20, 48), 'p27': (50, 27, 70)}
CD_RUNS = [('p3', 'default'), ('p3', 'vector'), ('p10', 'default'), ('p10', 'vector'), ('p12', 'default'), ('p20', 'default'), ('p27', 'default')]
_cd_cache = {}


def _live_sums(vec, pr, live, trials=None, want_hess=True):
    """dense._cd_sums restated over live entries: per neuron, summed over the listed trials, cost -(y hh - yhat), its size, gradient
    yhat w - y [m, 1] and Hessian yhat (w w^T + [V, 0; 0, 0]) with every term multiplied by the entry's live bit"""
    q, p, T, R = pr['dims']
    D = p + 1
    vv = np.asarray(vec, dtype=np.float64).reshape(D, q)
    Cn, dn = np.ascontiguousarray(vv[:p].T), vv[p]
    cost, size, g, H = np.zeros(q), np.zeros(q), np.zeros((q, D)), np.zeros((q, D, D))
    for r in (range(R) if trials is None else trials):
        lv = live[r].astype(np.float64)                                       # (q, T); zero behind the trial's length
        mt, vt = pr['M'][r].T, pr['V'][r]                                     # (T, p), (T, p, p)
        yy = pr['Y'][r].astype(np.float64) * lv
        Vc = np.einsum('tkl,nl->ntk', vt, Cn)
        hh = dn[:, None] + Cn @ mt.T
        yh = np.exp(hh + 0.5 * np.einsum('ntk,nk->nt', Vc, Cn)) * lv
        w = np.concatenate([mt[None] + Vc, np.ones((q, T, 1))], axis=2)
        cost -= np.sum(yy * hh - yh, axis=1)
        size += np.sum(np.abs(yy * hh) + yh, axis=1)
        g += np.einsum('nt,nti->ni', yh, w)
        g[:, :p] -= yy @ mt
        g[:, p] -= yy.sum(axis=1)
        if want_hess:
            H += np.matmul((w * yh[:, :, None]).transpose(0, 2, 1), w)
            H[:, :p, :p] += np.einsum('nt,tkl->nkl', yh, vt)
    return cost, size, g, H


def _cd_case(name, ragged):
    if (name, ragged) not in _cd_cache:
        _cd_cache.clear()
        q, p, T = CD_CASES[name]
        pr = dense._cd_problem(q, p, T, R8, seed=77 + 3 * q + T)
        bins = ob.pattern_masks(R8, q, T)
        lens = np.full(R8, T, dtype=np.int32)
        if ragged:
            lens = ragged_lengths(R8, T, seed=R8 + T, n_distinct=4)
            lens[5] = T
        live = bins & (np.arange(T)[None, None, :] < lens[:, None, None])
        assert live.any(axis=(1, 2)).all() and live.sum(axis=(0, 2)).min() > 4 * (p + 1)
        s0 = _live_sums(pr['v0'], pr, live)
        v1 = pr['v0'] + 0.3 * dense._step(*dense._with_prior(pr['v0'], s0, R8, None)[2:])[0].T.reshape(-1)
        s1 = _live_sums(v1, pr, live, want_hess=False)
        _cd_cache[(name, ragged)] = (pr, bins, lens, live, v1, s0, s1)
    return _cd_cache[(name, ragged)]


def _cd_context(pr, bins, lens, live, form):
    """counts zero at dead entries; the posterior NaN at padded bins (whatever read them would show)"""
    from funs import _hip
    q, p, T, R = pr['dims']
    Y = np.where(live, pr['Y'], 0)
    M, V = pr['M'].copy(), pr['V'].copy()
    for r, L in enumerate(lens):
        M[r, :, L:] = np.nan
        V[r, L:] = np.nan
    ctx = _hip.Context(q, p, T, R, BIN_MS)
    try:
        ctx.upload_counts(Y if Y.max() > 255 else Y.astype(np.uint8))
        for key in (('cd_mfma', 'cd_hess_mfma') if form == 'vector' else ()):
            ctx.set_option(key, 0)
        ctx.set_params(pr['C'], pr['d'], pr['tau_s'])
        ctx.set_observed_bins(bins)                                   # (before the lengths: the order of the calls must not matter)
        if np.any(lens != T):
            ctx.set_trial_lengths(lens)
    except Exception:
        ctx.close()
        raise
    return ctx, M, V


@pytest.mark.timeout(900)
@pytest.mark.parametrize('prior', [False, True], ids=['plain', 'prior'])
@pytest.mark.parametrize('ragged', [False, True], ids=['equal', 'ragged'])
@pytest.mark.parametrize('name,form', CD_RUNS, ids=['%s-%s' % r for r in CD_RUNS])
def test_cd_passes_with_a_bin_table(name, form, ragged, prior):
    """A synthetic posterior through pgpfa_set_posterior, the eight patterns, without and with per-trial lengths: costgrad, Newton pass (the
    Hessian rows), chord pass and per-neuron cost against plain FP64 numpy summed over live entries: cost 1e-10, gradient, steps and decrements
    1e-9, in the matrix-core and vector forms of widths 3 and 10, the vector forms of 12, 20 and 27."""
    pr, bins, lens, live, v1, s0, s1 = _cd_case(name, ragged)
    center = pr['center'] if prior else None
    ref0, ref1 = dense._with_prior(pr['v0'], s0, R8, center), dense._with_prior(v1, s1, R8, center)
    tag = 'bin table %s %s %s%s%s' % (name, pr['dims'], form, ' ragged' if ragged else '', ' with prior' if prior else '')
    ctx, M, V = _cd_context(pr, bins, lens, live, form)
    try:
        ctx.set_posterior(None, M, V)
        dense._compare_entry_points(tag, ctx, pr['v0'], v1, center, ref0, ref1)
        assert ctx.info('last_cd_unobserved_neurons') == 0.0 and ctx.info('observed_bins_set') == 1.0
    finally:
        ctx.close()


@pytest.mark.parametrize('name,form', [('p10', 'default'), ('p10', 'vector'), ('p12', 'default'), ('p20', 'default')],
                         ids=['p10-default', 'p10-vector', 'p12-default', 'p20-default'])
def test_a_neuron_without_a_live_entry_in_the_list(name, form):
    """An M-step over a list of trials on none of which neuron 20 has a live entry (an online minibatch): its gradient, Newton step, chord step and
    decrement are EXACTLY zero, last_cd_unobserved_neurons = 1; every other neuron is held to numpy over the list (1e-9)."""
    pr, bins, lens, live, _, _, _ = _cd_case(name, False)
    q, p, T, R = pr['dims']
    tb = bins.copy()
    tb[:, 20] = False
    tb[0, 20, 5:9] = True                                            # live on four bins of trial 0 only, which the list leaves out
    lst = np.array([5, 2, 7, 1, 4], dtype=np.int32)
    ctx, M, V = _cd_context(pr, tb, lens, tb, form)
    try:
        ctx.set_posterior(lst, M[lst], V[lst])
        s0 = _live_sums(pr['v0'], pr, tb, trials=lst)
        others = np.arange(q) != 20
        cost_r, _, g_r, H_r = dense._with_prior(pr['v0'], s0, len(lst), None)
        cost, grad = ctx.mstep_cd_costgrad(pr['v0'])
        cost_n, delta, dec = ctx.mstep_cd_newton_pass(pr['v0'])
        assert ctx.info('last_cd_unobserved_neurons') == 1.0
        _, delta_c, dec_c = ctx.mstep_cd_chord_pass(pr['v0'])
        g20, d20, c20 = grad.reshape(p + 1, q)[:, 20], delta.reshape(p + 1, q)[:, 20], delta_c.reshape(p + 1, q)[:, 20]
        d_ref, _ = dense._step(g_r[others], H_r[others])
        e_g = dense._rows(grad.reshape(p + 1, q)[:, others], g_r[others])
        e_d = dense._rows(delta.reshape(p + 1, q)[:, others], d_ref)
        print('%s %s: neuron 20: max |gradient| %.3e, |Newton step| %.3e, |chord step| %.3e, decrement %.3e; the others: gradient %.2e, step %.2e'
              % (name, form, np.max(np.abs(g20)), np.max(np.abs(d20)), np.max(np.abs(c20)), dec[20], e_g, e_d))
        assert e_g <= 1e-9 and e_d <= 1e-9 and np.all(np.isfinite(delta)) and np.all(np.isfinite(delta_c))
        assert not g20.any() and not d20.any() and not c20.any() and dec[20] == 0.0 and dec_c[20] == 0.0 and cost_n[20] == 0.0
    finally:
        ctx.close()


# ---- 4. exactness -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('q,p,T,R', [(30, 3, 100, 8), (40, 10, 176, 4), (50, 20, 48, 4)], ids=['p3', 'p10', 'p20'])
def test_a_table_of_all_ones_changes_no_bit(q, p, T, R):
    """pgpfa_set_observed_bins with every byte set against no call: bit-identical objective, modes, blocks, PautoSum, (C,d) cost, gradient and
    Newton step, count moments"""
    from funs import _hip
    params, Ys, _ = orc.synth_dataset(q, p, T, R, seed=9 + p)
    Y = np.stack(Ys).astype(np.uint8)
    got = []
    for with_table in (False, True):
        ctx = _hip.Context(q, p, T, R, BIN_MS)
        try:
            ctx.upload_counts(Y)
            ctx.set_params(params['C'], params['d'], params['tau'])
            if with_table:
                ctx.set_observed_bins(np.ones((R, q, T), dtype=np.uint8))
            assert ctx.info('observed_bins_set') == float(with_table)
            obj, _, st = ctx.estep_laplace()
            obj2, _, st2 = ctx.estep_laplace(warm_start=True)
            assert np.all(st == 0) and np.all(st2 == 0)
            ctx.mstep_precomp()
            v0 = orc.cd_to_vec(params['C'], params['d'])
            mom = ctx.count_moments()
            got.append([np.array([obj, obj2]), ctx.post_mean(), ctx.post_vsm(), ctx.post_vsmgp(), ctx.pautosum(), *ctx.mstep_cd_costgrad(v0),
                        *ctx.mstep_cd_newton_pass(v0), np.array(mom[0]), np.array(mom[1]), np.array(mom[2])])
        finally:
            ctx.close()
    same = [np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(*got)]
    print('p = %d: bit-identical with a bin table of ones: %s' % (p, same))
    assert all(same)


@pytest.mark.parametrize('name,options', [('c1', ()), ('p10', ()), ('p10', (('use_mfma', 0),)), ('p12', ()), ('p20', ()), ('p20', (('dual_gemm', 0),))],
                         ids=['c1', 'p10', 'p10-vector', 'p12', 'p20', 'p20-vector'])
def test_parameters_of_a_dead_neuron_change_no_bit(name, options):
    """C[n], d[n] of a neuron dead on every listed trial do not enter the E-step over the list: objective, modes, blocks and post_vsmGP are
    bit-identical after they are replaced by other (large) values"""
    from funs import _hip
    params, Yr, bins, lens, observed, T, live, ref = _case(name)
    q, p = Yr[0].shape[0], params['C'].shape[1]
    tb = bins.copy()
    n = q - 2
    tb[[1, 2, 6], n] = False
    lst = np.array([2, 6, 1], dtype=np.int32)
    got = []
    for moved in (False, True):
        C, d = params['C'].copy(), np.asarray(params['d'], dtype=np.float64).reshape(-1).copy()
        if moved:
            C[n] = 3.0 - 2.0 * C[n]
            d[n] = d[n] + 5.0
        ctx = _hip.Context(q, p, T, R8, BIN_MS)
        try:
            ctx.upload_counts(padded_counts(Yr, tb, T))
            for key, value in options:
                ctx.set_option(key, value)
            ctx.set_params(C, d, params['tau'])
            ctx.set_observed_bins(tb)
            obj, _, st = ctx.estep_laplace(lst)
            assert np.all(st == 0)
            got.append([np.array([obj]), ctx.post_mean(lst), ctx.post_vsm(lst), ctx.post_vsmgp(lst)])
        finally:
            ctx.close()
    same = [np.array_equal(a, b) for a, b in zip(*got)]
    print('%s %s: objective, modes, post_vsm, post_vsmGP bit-identical: %s' % (name, dict(options), same))
    assert all(same)


def test_counts_poked_into_dead_entries_change_no_bit(funs_mod):
    """The caller's Y at dead entries is ignored: the session zero-fills its resident copy.  Two experiments that differ only there give the same bits."""
    from funs import _session
    _session.drop_sessions()
    params, Yr, bins, lens, observed, T, live, ref = _case('c1')
    got = []
    for poke in (False, True):
        exp = bins_experiment(Yr, bins)
        if poke:
            for r, tr in enumerate(exp.data):
                tr['Y'] = np.where(bins[r], tr['Y'], tr['Y'] + 3.0 + r)
        infRes, nll, _ = funs_mod.inference.laplace(exp, {k: v.copy() for k, v in params.items()})
        got.append([np.array([nll])] + [np.array(infRes[k][r]) for k in ('post_mean', 'post_vsm', 'post_vsmGP') for r in range(R8)])
        _session.drop_sessions(exp)
    same = all(np.array_equal(a, b) for a, b in zip(*got))
    print('counts poked into %d dead entries: bit-identical %s' % (int((~bins).sum()), same))
    assert same


# ---- 5. EM end to end on config 1 with a 20 % speckle ----------------------------------------------------------------------------------------------
def speckled_config1():
    g = load_golden('c1_dataset.npz')
    Ys = [g['Y'][r].astype(np.float64) for r in range(g['Y'].shape[0])]
    R, (q, T) = len(Ys), Ys[0].shape
    live = np.random.default_rng(20).random((R, q, T)) >= 0.2
    assert live.any(axis=(1, 2)).all() and live.any(axis=(0, 2)).all()
    return g, Ys, live


def cd_grad_live(vec, Ys, pm, pv, live, p, q):
    """gradient of the (C,d) cost summed over live entries, with the reference's 1 / numTrials, in the vecCd layout"""
    pr = {'dims': (q, p, Ys[0].shape[1], len(Ys)), 'M': np.stack(pm), 'V': np.stack(pv), 'Y': np.stack(Ys)}
    return _live_sums(vec, pr, live, want_hess=False)[2].T.reshape(-1) / len(Ys)


def _stationarity(par, Ys, live, pm):
    Kinv = np.linalg.inv(orc.make_K(par['tau'], Ys[0].shape[1], BIN_MS))
    d = np.asarray(par['d'], dtype=np.float64).reshape(-1)
    return max(float(np.max(np.abs(ob.masked_grad(X, np.where(l, Y, 0.0), l, par['C'], d, Kinv)))) for Y, l, X in zip(Ys, live, pm))


def numpy_initialize(Ys, live, p):
    """the initialiser restated: n_i live entries per neuron, n_ij co-live entries per pair, then the reference's Poisson-PCA"""
    Z = np.stack([np.where(l, y, 0.0) for y, l in zip(Ys, live)])
    s, S = Z.sum(axis=(0, 2)), np.einsum('rit,rjt->ij', Z, Z)
    L = live.astype(np.float64)
    n_i, n_ij = L.sum(axis=(0, 2)), np.einsum('rit,rjt->ij', L, L)
    with np.errstate(invalid='ignore', divide='ignore'):
        mean = np.where(n_i > 0, s / n_i, 0.0)
        cov = np.where(n_ij >= 2, (S - np.outer(s, s) * n_ij / np.outer(n_i, n_i)) / (n_ij - 1.0), 0.0)
    mean = mean + 1e-10
    outer = np.outer(mean, mean)
    lamb = np.log(np.abs(cov + outer - np.diag(mean))) - np.log(outer)
    evals, evecs = np.linalg.eig(lamb)
    return evecs[:, np.argsort(evals)[::-1]][:, :p], np.log(mean)


@pytest.mark.timeout(900)
def test_batch_em_on_speckled_config1(funs_mod):
    """initializeParams equals its numpy restatement with n_i and n_ij bit for bit; three batch-EM iterations (CdOptimMethod='newton'): every mode
    stationary for its reduced problem (1e-6), the new (C,d) zero the numpy gradient over live entries (2e-6), the new timescales orc.tau_grad on
    PautoSum (1e-6 R = 2e-5) - the limits of test_batch_em_on_stitched_config1."""
    from funs import _session
    _session.drop_sessions()
    _, Ys, live = speckled_config1()
    R, q, p = len(Ys), Ys[0].shape[0], 3
    exp = bins_experiment(Ys, live)
    np.random.seed(5)
    init = funs_mod.util.initializeParams(p, q, exp)
    C_ref, d_ref = numpy_initialize(Ys, live, p)
    same = np.array_equal(np.asarray(init['C']), C_ref) and np.array_equal(np.asarray(init['d']), d_ref)
    print('initializeParams against its numpy restatement: bit for bit %s (max |dC| %.2e, |dd| %.2e)'
          % (same, np.max(np.abs(np.asarray(init['C']) - C_ref)), np.max(np.abs(np.asarray(init['d']) - d_ref))))
    assert same
    params = {k: np.real(np.asarray(v)).astype(np.float64) for k, v in init.items()}
    optim = None
    for it in range(3):
        infRes, nll, optim = funs_mod.inference.laplace(exp, params, prevOptimRes=optim)
        assert np.all(infRes.newton_status == 0) and infRes.session.ctx.info('observed_bins_set') == 1.0
        pm = [np.array(infRes['post_mean'][r]) for r in range(R)]
        pv = [np.array(infRes['post_vsm'][r]) for r in range(R)]
        new, _ = funs_mod.learning.updateParams(params, infRes, exp, CdOptimMethod='newton')
        P = infRes.session.ctx.pautosum()
        worst = _stationarity(params, Ys, live, pm)
        g_cd = float(np.max(np.abs(cd_grad_live(orc.cd_to_vec(new['C'], new['d']), Ys, pm, pv, live, p, q))))
        logp = np.log(1.0 / (new['tau'] * 1000.0 / BIN_MS) ** 2)
        g_tau = max(abs(orc.tau_grad(logp[k], P[k], R)[0]) for k in range(p))
        print('batch EM iteration %d: nPLL %.6f, worst |grad| of a mode %.2e, |(C,d) gradient| %.2e, |timescale gradient| %.2e' % (it, nll, worst, g_cd, g_tau))
        assert worst <= 1e-6 and g_cd <= 2e-6 and g_tau <= 1e-6 * R
        params = new
    _session.drop_sessions()


@pytest.mark.timeout(900)
def test_online_diag_em_on_speckled_config1(funs_mod):
    """Three stochastic-EM iterations with the 'diag' prior on minibatches of 6 (the parent's resident counts and table): every mode stationary
    (1e-6), the new (C,d) zero the regularised gradient over the minibatch's live entries (2e-6), the new timescales the reference's regularised
    timescale gradient (1e-6 batch)."""
    from funs import _session
    _session.drop_sessions()
    g, Ys, live = speckled_config1()
    R, q, p, batch = len(Ys), Ys[0].shape[0], 3, 6
    exp = bins_experiment(Ys, live)
    params = {'C': g['init_C'].copy(), 'd': g['init_d'].copy(), 'tau': g['init_tau'].copy()}
    np.random.seed(11)
    prior = np.diag(np.ones(q * (p + 1)))
    for n in range(3):
        sz = 1.0 / (n + 1) ** 0.75
        sub = funs_mod.util.subsampleTrials(exp, batch)
        idx = np.asarray(sub.batchTrIdx)
        infRes, nll, _ = funs_mod.inference.laplace(sub, params, prevOptimRes='resident')
        assert infRes.session is _session.session_for(exp, p)[0] and infRes.session.ctx.info('observed_bins_set') == 1.0
        Yb, lb = [Ys[i] for i in idx], live[idx]
        pm = [np.array(infRes['post_mean'][j]) for j in range(batch)]
        pv = [np.array(infRes['post_vsm'][j]) for j in range(batch)]
        new, _, prior = funs_mod.learning.updateParamsWithPrior(params, infRes, sub, 'newton', 'lockstep', sz, sz, prior, covOpts='useDiag')
        assert infRes.session.ctx.info('last_cd_unobserved_neurons') == 0.0
        P = infRes.session.ctx.pautosum()
        worst = _stationarity(params, Yb, lb, pm)
        old_vec, new_vec = orc.cd_to_vec(params['C'], params['d']), orc.cd_to_vec(new['C'], new['d'])
        g_cd = float(np.max(np.abs(cd_grad_live(new_vec, Yb, pm, pv, lb, p, q) - prior @ (new_vec - old_vec))))
        logp = np.log(1.0 / (new['tau'] * 1000.0 / BIN_MS) ** 2)
        g_tau = max(abs(orc.tau_grad_prior(logp[k], P[k], batch, BIN_MS, params['tau'][k], sz)[0]) for k in range(p))
        print('online EM iteration %d (trials %s): worst |grad| of a mode %.2e, |(C,d) gradient| %.2e, |timescale gradient| %.2e'
              % (n, idx.tolist(), worst, g_cd, g_tau))
        assert worst <= 1e-6 and g_cd <= 2e-6 and g_tau <= 1e-6 * batch
        params = new
    _session.drop_sessions()


def test_fit_object_on_a_speckled_experiment(funs_mod):
    """engine.PPGPFAfit in Batch mode with trackEvidence and emTol, in Online mode, crossValidation(score='evidence') and coSmoothing on the
    speckled experiment: finite likelihoods, evidences, parameters and scores; trajectories extract."""
    from funs import _session
    _session.drop_sessions()
    g, Ys, live = speckled_config1()
    exp = bins_experiment(Ys, live)
    init = {'C': g['init_C'].copy(), 'd': g['init_d'].copy(), 'tau': g['init_tau'].copy()}
    fit = funs_mod.engine.PPGPFAfit(exp, initParams={k: v.copy() for k, v in init.items()}, EMmode='Batch', maxEMiter=3, CdOptimMethod='newton', quiet=True,
                                    trackEvidence=True, emTol=1e-12)
    print('batch fit: nPLL %s, mean log evidence %s' % (np.round(fit.posteriorLikelihood, 4).tolist(), np.round(fit.logEvidence, 4).tolist()))
    assert np.all(np.isfinite(fit.posteriorLikelihood)) and len(fit.logEvidence) == 3 and np.all(np.isfinite(fit.logEvidence))
    assert all(np.all(np.isfinite(fit.optimParams[k])) for k in ('C', 'd', 'tau')) and np.all(np.isfinite(fit.sampleMeanSpikeCounts))
    fit.extractTrajectories()
    np.random.seed(3)
    fit = funs_mod.engine.PPGPFAfit(exp, initParams={k: v.copy() for k, v in init.items()}, EMmode='Online', maxEMiter=2, batchSize=5,
                                    onlineParamUpdateMethod='diag', quiet=True, trackEvidence=True)
    assert np.all(np.isfinite(fit.posteriorLikelihood)) and all(np.all(np.isfinite(fit.optimParams[k])) for k in ('C', 'd', 'tau'))
    np.random.seed(4)
    half = bins_experiment(Ys[:10], live[:10])
    cv = funs_mod.util.crossValidation(half, numTrainingTrials=8, numTestTrials=2, maxXdim=2, maxEMiter=2, score='evidence')
    co = funs_mod.util.coSmoothing(init, half, [3, 17], trials=[0, 1, 2])
    print('crossValidation(score=evidence) on a speckled experiment: %s; coSmoothing %.5f bits per spike' % (np.round(cv.errs, 5).tolist(), co['bitsPerSpike']))
    assert np.all(np.isfinite(cv.errs)) and np.isfinite(co['bitsPerSpike']) and co['rate'][0].shape == (2, Ys[0].shape[1])
    _session.drop_sessions()


# ---- 6. binHoldout and the speckled score ----------------------------------------------------------------------------------------------------------
def test_bin_holdout_against_numpy(funs_mod):
    """util.binHoldout on the first 8 trials of config 1, 10 % of the entries held out on top of a table that already hides a window (neuron 4,
    bins 10..39 of trial 2), against the same score from the numpy posterior of the reduced model.  Tolerance: the bound that
    test_co_smoothing_against_the_oracle propagates from the 1e-8 on modes and blocks - a relative rate error delta_n = 1e-8 sum_k |C_nk| +
    1e-8 max|Sigma| (sum_k |C_nk|)^2 / 2 and a score error of at most sum (y + lam) delta_n / (log 2 sum y) over the scored entries.  The
    experiment's session, table and resident posterior stay as they were; held-out entries the experiment itself hid are not scored."""
    from funs import _session
    _session.drop_sessions()
    params, Ys, T = _problem('c1')
    q, p = Ys[0].shape[0], 3
    own = np.ones((R8, q, T), dtype=bool)
    own[2, 4, 10:40] = False
    exp = bins_experiment(Ys, own)
    infRes, _, _ = funs_mod.inference.laplace(exp, {k: v.copy() for k, v in params.items()})
    sess = infRes.session
    before = (sess.observed_bins.copy(), sess.post_stamp, np.array(infRes['post_mean'][2]))
    held = list(np.random.default_rng(8).random((R8, q, T)) < 0.1)
    held[2][4, 20:30] = True                                         # ten entries the experiment itself hides: held out, not scored
    out = funs_mod.util.binHoldout(params, exp, held)
    assert np.array_equal(sess.observed_bins, before[0]) and sess.post_stamp == before[1] and sess.ctx.info('observed_bins_set') == 1.0
    assert np.array_equal(sess.ctx.post_mean(np.array([2], dtype=np.int32))[0], before[2])
    C, d = params['C'], params['d'].reshape(-1)
    c1n = np.abs(C).sum(axis=1)
    lam, delta, scored = [], [], []
    for r in range(R8):
        res = ob.masked_laplace(Ys[r], own[r] & ~held[r], params)
        m, S = res['post_mean'], res['post_vsm']
        lam.append(np.exp(C @ m + d[:, None] + 0.5 * np.einsum('nk,tkl,nl->nt', C, S, C)))
        delta.append(1e-8 * c1n + 0.5 * 1e-8 * np.max(np.abs(S)) * c1n ** 2 + 1e-12)
        scored.append(held[r] & own[r])
    lam, delta, scored = np.stack(lam), np.stack(delta), np.stack(scored)
    y = np.stack(Ys) * scored
    n_sc = scored.sum(axis=(0, 2))
    lbar = y.sum(axis=(0, 2)) / n_sc
    ll = ((y * np.log(lam) - lam) - (y * np.log(lbar)[None, :, None] - lbar[None, :, None])) * scored
    score_ref = ll.sum() / (np.log(2.0) * y.sum())
    per_neuron_ref = ll.sum(axis=(0, 2)) / (np.log(2.0) * y.sum(axis=(0, 2)))
    bound = float(np.sum((y + lam) * delta[:, :, None] * scored) / (np.log(2.0) * y.sum()))
    per_s = 1000.0 / BIN_MS
    e_rate = max(float(np.max(np.abs(out['rate'][r] / per_s - lam[r]) / (lam[r] * delta[r][:, None]))) for r in range(R8))
    e_score = abs(out['bitsPerSpike'] - score_ref)
    print('binHoldout: %.6f bits per spike (numpy %.6f), difference %.2e (bound %.2e); rates %.3f of their propagated bound; %d entries scored of %d held out'
          % (out['bitsPerSpike'], score_ref, e_score, bound, e_rate, out['nScored'], int(sum(h.sum() for h in held))))
    assert e_rate <= 1.0 and e_score <= bound
    ok = y.sum(axis=(0, 2)) > 0
    assert np.max(np.abs(out['bitsPerSpikePerNeuron'][ok] - per_neuron_ref[ok])) <= 10 * bound * y.sum() / y.sum(axis=(0, 2))[ok].min()
    hidden_twice = int((np.stack(held) & ~own).sum())                 # held out AND hidden by the experiment itself: the ten set above and the draws in the window
    assert hidden_twice >= 10 and out['nScored'] == int(scored.sum()) == int(sum(h.sum() for h in held)) - hidden_twice
    assert len(out['rate']) == R8 and out['rate'][0].shape == (q, T) and all(np.all(np.isfinite(x)) for x in out['rate'])
    _session.drop_sessions()


def test_cross_validation_with_the_speckled_score(funs_mod):
    """crossValidation(score='speckled', maxXdim=2, maxEMiter=2) on config 1: errs equal -binHoldout(...)['bitsPerSpike'] recomputed by hand with
    the same seed, the held-out subset is the same for every width, and a second run gives the same numbers."""
    from funs import _session
    _session.drop_sessions()
    g = load_golden('c1_dataset.npz')
    Ys = [g['Y'][r].astype(np.float64) for r in range(g['Y'].shape[0])]
    runs = []
    for _ in range(2):
        np.random.seed(6)
        cv = funs_mod.util.crossValidation(Experiment(Ys, BIN_MS), numTrainingTrials=8, numTestTrials=2, maxXdim=2, maxEMiter=2, score='speckled',
                                           holdoutFraction=0.1, seed=3)
        runs.append(cv)
        _session.drop_sessions()
    cv = runs[0]
    train = Experiment(Ys[:8], BIN_MS)
    held = funs_mod.util.speckledHoldout(train, 0.1, seed=3)
    assert all(np.array_equal(a, b) for a, b in zip(held, cv.heldOut))
    by_hand = [-funs_mod.util.binHoldout(fit.optimParams, train, held)['bitsPerSpike'] for fit in cv.fits]
    print('crossValidation(score=speckled): errs %s, by hand %s, second run %s, optimXdim %d' % (cv.errs, by_hand, runs[1].errs, cv.optimXdim))
    assert cv.errs == by_hand and runs[1].errs == cv.errs and np.all(np.isfinite(cv.errs)) and cv.optimXdim == int(np.argmin(cv.errs)) + 1
    with pytest.raises(ValueError, match='laplace'):
        funs_mod.util.crossValidation(train, 6, 2, maxXdim=1, inferenceMethod='variational', score='speckled')
    _session.drop_sessions()


# ---- 7. rates and samples ---------------------------------------------------------------------------------------------------------------------------
def test_posterior_rates_and_samples_cover_dead_entries(funs_mod):
    """posteriorRates over every entry: eta and var against numpy on the device's own posterior (1e-12 of their sums of absolute terms), finite
    rates and bands at dead entries, condition averages over all trials; 'ell' raises ValueError; posteriorSamples draws counts everywhere."""
    from funs import _session
    _session.drop_sessions()
    params, Yr, bins, lens, observed, T, live, ref = _case('c1')
    q, p = Yr[0].shape[0], 3
    exp = bins_experiment(Yr, bins)
    par = {k: v.copy() for k, v in params.items()}
    infRes, _, _ = funs_mod.inference.laplace(exp, par)
    out = funs_mod.util.posteriorRates(par, exp, infRes=infRes, conditions=[0, 1] * 4, want=('rate', 'eta', 'var', 'lower', 'upper'))
    C, d = params['C'], params['d'].reshape(-1)
    e_eta = e_var = 0.0
    for r in range(R8):
        m, S = infRes['post_mean'][r], infRes['post_vsm'][r]
        e_eta = max(e_eta, float(np.max(np.abs(out['eta'][r] - (C @ m + d[:, None])) / (np.abs(C) @ np.abs(m) + np.abs(d)[:, None]))))
        e_var = max(e_var, float(np.max(np.abs(out['var'][r] - np.einsum('nk,tkl,nl->nt', C, S, C)) / np.einsum('nk,tkl,nl->nt', np.abs(C), np.abs(S), np.abs(C)))))
    print('rates under a bin table: eta %.2e, var %.2e of their scales (limit 1e-12); %d dead entries covered' % (e_eta, e_var, int((~bins).sum())))
    assert e_eta <= 1e-12 and e_var <= 1e-12
    assert out['rate'].shape == (R8, q, T) and np.all(np.isfinite(out['rate'])) and np.all(out['lower'] <= out['rate']) and np.all(out['rate'] <= out['upper'])
    assert out['condition_mean'].shape == (2, q, T) and np.all(np.isfinite(out['condition_mean'])) and np.all(out['condition_count'] == 4)
    with pytest.raises(ValueError, match="'ell'"):
        funs_mod.util.posteriorRates(par, exp, infRes=infRes, want=('rate', 'ell'))
    smp = funs_mod.util.posteriorSamples(par, exp, infRes=infRes, trials=[0, 5, 3], nSamples=4, seed=1, want=('x', 'y'))
    assert smp['x'].shape == (3, 4, p, T) and smp['y'].shape == (3, 4, q, T) and np.all(np.isfinite(smp['x']))
    _session.drop_sessions()


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(funs_mod):
    from funs import _hip, _session
    _session.drop_sessions()
    params, Yr, bins, lens, observed, T, live, ref = _case('c1')
    q, p = Yr[0].shape[0], 3
    exp = bins_experiment(Yr, bins)
    par = lambda: {k: v.copy() for k, v in params.items()}
    calls = [lambda: funs_mod.inference.dualVariational(exp, par()), lambda: funs_mod.util.leaveOneOutPrediction(par(), exp),
             lambda: funs_mod.mcmc.PosteriorMCMC(exp, par(), 2, 0), lambda: funs_mod.mcmc.PosteriorMCMC_batch(exp, par(), 2, [0, 1], [1, 2])]
    for call in calls:
        with pytest.raises(NotImplementedError, match='per-bin'):
            call()
    old = funs_mod.inference.DUAL_MASKED
    funs_mod.inference.DUAL_MASKED = True
    try:
        with pytest.raises(NotImplementedError, match='per-bin'):
            funs_mod.inference.dualVariational(exp, par())
    finally:
        funs_mod.inference.DUAL_MASKED = old
    host = {'post_mean': [np.zeros((p, T))] * R8, 'post_vsm': [np.zeros((T, p, p))] * R8, 'post_vsmGP': [np.zeros((T, T, p))] * R8}
    with pytest.raises(NotImplementedError, match='per-bin'):
        funs_mod.learning.MStepObservationCost(orc.cd_to_vec(params['C'], params['d']), p, q, exp, host)
    _session.drop_sessions()
    Y = padded_counts(Yr, live, T)
    ctx = _hip.Context(q, p, T, R8, BIN_MS)
    try:
        ctx.upload_counts(Y)
        ctx.set_params(params['C'], params['d'], params['tau'])
        tb = bins.copy()
        tb[4] = False
        with pytest.raises(_hip.HipBackendError, match='trial 4 has no live entry'):
            ctx.set_observed_bins(tb)
        tb = bins.copy()
        tb[:, 7] = False
        with pytest.raises(_hip.HipBackendError, match='neuron 7 has no live entry'):
            ctx.set_observed_bins(tb)
        with pytest.raises(ValueError, match='shape'):
            ctx.set_observed_bins(bins[:, :, :-1])
        assert ctx.info('observed_bins_set') == 0.0
        Yb = Y.copy()
        Yb[5, 3, 40] = 2                                               # trial 5 has the single live entry (17, 33)
        Yb[5, 9, 0] = 1
        ctx.upload_counts(Yb)
        with pytest.raises(_hip.HipBackendError, match='trial 5: 2 non-zero counts at entries the per-bin table marks as not recorded'):
            ctx.set_observed_bins(bins)
        assert ctx.info('observed_bins_set') == 0.0
        ctx.upload_counts(Y)
        ctx.set_observed_bins(bins)
        assert ctx.info('observed_bins_set') == 1.0
        # the other two tables compose by AND in any order: lengths that leave trial 5 without its live entry are refused, the table stays
        short = np.full(R8, T, dtype=np.int32)
        short[5] = 20
        with pytest.raises(_hip.HipBackendError, match='trial 5 has no live entry'):
            ctx.set_trial_lengths(short)
        assert ctx.info('trial_lengths_set') == 0.0 and ctx.info('observed_bins_set') == 1.0
        hide = np.ones((R8, q), dtype=np.uint8)
        hide[5, 17] = 0
        with pytest.raises(_hip.HipBackendError, match='trial 5 has no live entry'):
            ctx.set_observed(hide)
        assert ctx.info('observed_set') == 0.0
        lam = np.full((1, q * T), 0.5)
        idx = np.zeros(1, dtype=np.int32)
        for masked in (0, 1):
            ctx.set_option('dual_masked', masked)
            for call in (lambda: ctx.dual_costgrad(0, lam[0]), lambda: ctx.dual_costgrad_batch(idx, lam), lambda: ctx.dual_lbfgs(idx, np.log(lam)),
                         lambda: ctx.dual_fixed_point(idx), lambda: ctx.dual_finalize(idx, lam), lambda: ctx.dual_post_mean(0, lam[0]),
                         lambda: ctx.dual_post_cov(0, lam[0]), lambda: ctx.loo_predict(idx), lambda: ctx.generate(1)):
                with pytest.raises(_hip.HipBackendError, match='per-bin'):
                    call()
        ctx.set_option('dual_masked', 0)
        # counts uploaded while a table is set are checked again; the table stays; NULL drops it
        with pytest.raises(_hip.HipBackendError, match='trial 5: 2 non-zero counts at entries the per-bin table marks as not recorded'):
            ctx.upload_counts(Yb)
        ctx.upload_counts(Y)
        assert ctx.info('observed_bins_set') == 1.0
        obj, _, st = ctx.estep_laplace()
        assert np.all(st == 0) and np.isfinite(obj)
        ctx.set_observed_bins(None)
        assert ctx.info('observed_bins_set') == 0.0
    finally:
        ctx.close()


def test_the_order_of_the_three_calls_does_not_matter():
    """lengths, 'observed' and the bin table set in two different orders: bit-identical objective, modes and blocks; dropping the lengths while
    the bin table stays equals never having set them"""
    from funs import _hip
    params, Yr, bins, lens, observed, T, live, ref = _case('c1', ragged=True)
    q, p = Yr[0].shape[0], 3
    Y = padded_counts(Yr, live, T)
    got = []
    for order in ('lob', 'bol'):
        ctx = _hip.Context(q, p, T, R8, BIN_MS)
        try:
            ctx.upload_counts(Y)
            ctx.set_params(params['C'], params['d'], params['tau'])
            for step in order:
                {'l': lambda: ctx.set_trial_lengths(lens), 'o': lambda: ctx.set_observed(observed), 'b': lambda: ctx.set_observed_bins(bins)}[step]()
            obj, _, st = ctx.estep_laplace()
            assert np.all(st == 0)
            got.append([np.array([obj]), ctx.post_mean(), ctx.post_vsm()])
            if order == 'bol':
                ctx.set_trial_lengths(None)
                ctx.set_observed(None)
                obj, _, _ = ctx.estep_laplace()
                dropped = [np.array([obj]), ctx.post_mean(), ctx.post_vsm()]
        finally:
            ctx.close()
    ctx = _hip.Context(q, p, T, R8, BIN_MS)
    try:
        ctx.upload_counts(Y)
        ctx.set_params(params['C'], params['d'], params['tau'])
        ctx.set_observed_bins(bins)
        obj, _, _ = ctx.estep_laplace()
        only = [np.array([obj]), ctx.post_mean(), ctx.post_vsm()]
    finally:
        ctx.close()
    same = [np.array_equal(a, b) for a, b in zip(*got)]
    same2 = [np.array_equal(a, b) for a, b in zip(dropped, only)]
    print('orders l-o-b and b-o-l bit-identical: %s; lengths and observed dropped against never set: %s' % (same, same2))
    assert all(same) and all(same2)


def test_an_upload_that_drops_the_lengths_rebuilds_the_bin_words_without_them():
    """upload, lengths, bin table, the same counts again: the upload drops the lengths, and the bin words - built with the lengths folded in - must
    lose them too: objective, modes and blocks bit-identical to a context that only ever had the bin table.  (Before the tables had one owner the words
    kept the lengths while every reader of the length table saw T bins.)"""
    from funs import _hip
    params, Yr, bins, lens, observed, T, live, ref = _case('c1', ragged=True)
    q, p = Yr[0].shape[0], 3
    Y = padded_counts(Yr, live, T)
    got = []
    for with_lengths in (True, False):
        ctx = _hip.Context(q, p, T, R8, BIN_MS)
        try:
            ctx.upload_counts(Y)
            ctx.set_params(params['C'], params['d'], params['tau'])
            if with_lengths:
                ctx.set_trial_lengths(lens)
            ctx.set_observed_bins(bins)
            if with_lengths:
                ctx.upload_counts(Y)
            assert ctx.info('trial_lengths_set') == 0.0 and ctx.info('observed_bins_set') == 1.0
            obj, _, st = ctx.estep_laplace()
            assert np.all(st == 0)
            got.append([np.array([obj]), ctx.post_mean(), ctx.post_vsm()])
        finally:
            ctx.close()
    same = [np.array_equal(a, b) for a, b in zip(*got)]
    print('re-upload under lengths + bin table against the bin table alone, bit-identical (objective, post_mean, post_vsm): %s' % same)
    assert all(same)
