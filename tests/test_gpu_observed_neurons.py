"""Laplace EM with neurons unobserved on some trials (pgpfa_set_observed, experiment.data[r]['observed']).

An unobserved (trial, neuron) pair carries no likelihood term: the Laplace posterior, objective and evidence of trial r are those of the model
with only the observed rows of C, d and Y.  The yardstick of every E-step check below is therefore orc.laplace(mode='exact') on each trial
with the unobserved rows of Y, C and d DELETED (and the bins cut where lengths differ too); the (C,d) passes are held to plain FP64 numpy summed
over the observed pairs.  The shapes are those of test_gpu_unequal_trials.py (config 1; 40 x 10 x 176: poisson_mfma_kernel<10, 2>; 35 x 12 x 64:
the one-tile matrix-core form; 50 x 20 x 48: the GEMM form), the patterns hit the tile seams:

    trial 0 fully observed | one trial lacks neurons {0, 15, 16, q-1} | one has the single neuron 17 | one only neurons 0..15 (the first matrix-core
    tile) | one only the neurons behind the vector kernel's 32-neuron chunk | one every second neuron

(config 1 has 30 neurons, none behind neuron 31: its fifth pattern is 'only neurons >= 16', behind the first matrix-core tile; its 20 trials
take the six patterns in turn).

Tolerances are the project's own for the same kernels (test_gpu_unequal_trials.py): modes 1e-8, covariance blocks 1e-8
relative, objective / nPLL 1e-9 relative, evidence 1e-9, (C,d) cost 1e-10, gradient and steps 1e-9.  Every test prints the figures it measured
before it asserts."""
import numpy as np
import pytest

from conftest import Experiment, load_golden
from oracle import pgpfa_oracle as orc
import test_gpu_mstep_dense as dense
from test_gpu_laplace_evidence import numpy_log_evidence
from test_gpu_unequal_trials import BIN_MS, _estep_problem, cov_mode, funs_mod, ragged_lengths, rel  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

INV_S2 = dense.INV_S2


@pytest.fixture(scope='module', autouse=True)
def _leave_nothing_behind():
    """after the last test of this file: no session, context or cached reference of it stays alive for the files that follow"""
    yield
    import gc
    from funs import _session
    _session.drop_sessions()
    _cases.clear()
    _cd_cache.clear()
    gc.collect()


# ---- tables ------------------------------------------------------------------------------------------------------------------------------------
def seam_table(R, q):
    """(R, q) booleans: the six patterns of the header, in turn over the trials"""
    n = np.arange(q)
    behind = n >= (32 if q > 32 else 16)
    rows = [np.ones(q, bool), ~np.isin(n, [0, 15, 16, q - 1]), n == 17, n < 16, behind, n % 2 == 0]
    table = np.stack([rows[r % 6] for r in range(R)])
    assert table.any(axis=1).all() and table.any(axis=0).all() and R >= 6
    return table


def observed_experiment(Ys, table, nan=False):
    """Experiment whose trials carry 'observed'; the counts of unobserved rows are left in place (the session must ignore them) or set to NaN"""
    exp = Experiment(Ys, BIN_MS)
    for r, tr in enumerate(exp.data):
        tr['observed'] = table[r].copy()
        if nan:
            tr['Y'] = tr['Y'].copy()
            tr['Y'][~table[r]] = np.nan
    return exp


def reduced(params, o):
    return {'C': params['C'][o], 'd': np.asarray(params['d']).reshape(-1)[o], 'tau': params['tau']}


def oracle_reduced(Ys, table, params, cov_trials=()):
    """orc.laplace(mode='exact') per trial on the observed rows -> per-trial lists, sum of the objectives"""
    out = {k: [None] * len(Ys) for k in ('post_mean', 'post_vsm', 'post_vsmGP', 'post_cov')}
    total = 0.0
    for r, Y in enumerate(Ys):
        o = table[r]
        res, nll, _ = orc.laplace([np.asarray(Y, dtype=np.float64)[o]], reduced(params, o), BIN_MS, mode='exact', return_cov=(r in cov_trials))
        total += -nll
        for k in out:
            if k in res:
                out[k][r] = res[k][0]
    return out, total


_cases = {}


def _case(name, ragged=False):
    """(params, trials (cut where ragged), table, lengths, T, oracle posteriors, oracle objective sum): computed once, shared, never written to"""
    if (name, ragged) not in _cases:
        params, Ys, T = _estep_problem(name)
        R, q = len(Ys), Ys[0].shape[0]
        table = seam_table(R, q)
        lens = ragged_lengths(R, T, seed=len(name) + T, n_distinct=5 if name == 'c1' else 4) if ragged else np.full(R, T, dtype=np.int32)
        Yr = [np.ascontiguousarray(np.asarray(y, dtype=np.float64)[:, :L]) for y, L in zip(Ys, lens)]
        single = [r for r in range(R) if table[r].sum() == 1][:1] if name == 'c1' else []
        ref, total = oracle_reduced(Yr, table, params, cov_trials=single)
        _cases[(name, ragged)] = (params, Yr, table, lens, T, ref, total)
    return _cases[(name, ragged)]


def padded_counts(Yr, table, T):
    Y = np.zeros((len(Yr), Yr[0].shape[0], T), dtype=np.uint8)
    for r, y in enumerate(Yr):
        Y[r, :, :y.shape[1]] = np.where(table[r][:, None], y, 0)
    return Y


def _compare_posterior(tag, infRes, optim, ref, lens, p, nll, nll_ref):
    e_m = e_v = e_g = 0.0
    for r in range(len(lens)):
        L = int(lens[r])
        m, v, gp = infRes['post_mean'][r], infRes['post_vsm'][r], infRes['post_vsmGP'][r]
        assert m.shape == (p, L) and v.shape == (L, p, p) and gp.shape == (L, L, p) and np.array_equal(optim[r], m.reshape(-1))
        e_m = max(e_m, float(np.max(np.abs(m - ref['post_mean'][r]))))
        e_v = max(e_v, rel(v, ref['post_vsm'][r]))
        e_g = max(e_g, rel(gp, ref['post_vsmGP'][r]))
    e_f = abs(nll - nll_ref) / abs(nll_ref)
    print('%s: modes %.2e, post_vsm %.2e, post_vsmGP %.2e, nPLL %.2e' % (tag, e_m, e_v, e_g, e_f))
    assert e_m <= 1e-8 and e_v <= 1e-8 and e_g <= 1e-8 and e_f <= 1e-9


# ---- 1. E-step against the oracle on the observed rows ------------------------------------------------------------------------------------------
@pytest.mark.timeout(900)
@pytest.mark.parametrize('cov_mode', [1, 2], indirect=True, ids=['dense', 'lowrank'])
@pytest.mark.parametrize('name', ['c1', 'p10', 'p12', 'p20'])
def test_estep_against_the_oracle_on_the_observed_rows(funs_mod, name, cov_mode):
    """inference.laplace on an experiment with 'observed' rows, cold, from the resident modes and from host copies of lapOptimRes, under both
    covariance engines: post_mean 1e-8, post_vsm and post_vsmGP 1e-8 relative, nPLL 1e-9 relative against the oracle on the reduced model of
    every trial; config 1 also post_cov of the single-neuron trial.  The unobserved rows of 'Y' hold NaN: nothing may read them."""
    params, Yr, table, lens, T, ref, total = _case(name)
    R, p = len(Yr), params['C'].shape[1]
    exp = observed_experiment(Yr, table, nan=True)
    optim = host_copy = None
    for start in ('cold', 'resident', 'host'):
        prev = {'cold': None, 'resident': optim, 'host': host_copy}[start]
        infRes, nll, optim = funs_mod.inference.laplace(exp, {k: v.copy() for k, v in params.items()}, prevOptimRes=prev)
        sess = infRes.session
        assert sess.ctx.info('observed_set') == 1.0 and sess.ctx.info('trial_lengths_set') == 0.0 and np.all(infRes.newton_status == 0)
        assert sess.ctx.info('last_cov_lowrank') == float(cov_mode == 2)
        _compare_posterior('%s, engine %d, %s start' % (name, cov_mode, start), infRes, optim, ref, lens, p, nll, -total / R)
        if start == 'cold':
            host_copy = [np.array(optim[r]) for r in range(R)]
            if name == 'c1':
                r = [i for i in range(R) if table[i].sum() == 1][0]
                e_c = rel(infRes['post_cov'][r], ref['post_cov'][r])
                print('%s, engine %d: post_cov of the single-neuron trial %d: %.2e' % (name, cov_mode, r, e_c))
                assert e_c <= 1e-8


# ---- 2. the vector Poisson pass ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,option', [('p20', 'dual_gemm'), ('p10', 'use_mfma')])
def test_vector_poisson_pass_against_the_oracle(name, option):
    """poisson_pass_kernel under the same yardstick, at the C-ABI: option dual_gemm = 0 selects it at 20 latents, use_mfma = 0 (set before the
    parameters) at 10.  Modes 1e-8, objective 1e-9 relative, cold and warm."""
    from funs import _hip
    params, Yr, table, lens, T, ref, total = _case(name)
    R, q, p = len(Yr), Yr[0].shape[0], params['C'].shape[1]
    ctx = _hip.Context(q, p, T, R, BIN_MS)
    try:
        ctx.upload_counts(padded_counts(Yr, table, T))
        ctx.set_option(option, 0)
        ctx.set_params(params['C'], params['d'], params['tau'])
        ctx.set_observed(table)
        for warm in (False, True):
            obj, _, st = ctx.estep_laplace(warm_start=warm)
            assert np.all(st == 0)
            M = ctx.post_mean()
            e_m = max(float(np.max(np.abs(M[r] - ref['post_mean'][r]))) for r in range(R))
            e_f = abs(obj - total) / abs(total)
            print('%s, vector Poisson pass (%s = 0), %s: modes %.2e, objective %.2e' % (name, option, 'warm' if warm else 'cold', e_m, e_f))
            assert e_m <= 1e-8 and e_f <= 1e-9
    finally:
        ctx.close()


# ---- 3. the table together with ragged lengths ---------------------------------------------------------------------------------------------------
@pytest.mark.timeout(900)
@pytest.mark.parametrize('cov_mode', [1, 2], indirect=True, ids=['dense', 'lowrank'])
@pytest.mark.parametrize('name', ['c1', 'p10'])
def test_table_together_with_ragged_lengths(funs_mod, name, cov_mode):
    """Trials cut to lengths in T/2..T AND rows unobserved: the oracle on the rows deleted and the bins cut."""
    params, Yr, table, lens, T, ref, total = _case(name, ragged=True)
    R, p = len(Yr), params['C'].shape[1]
    exp = observed_experiment(Yr, table)
    optim = None
    for start in ('cold', 'resident'):
        infRes, nll, optim = funs_mod.inference.laplace(exp, {k: v.copy() for k, v in params.items()}, prevOptimRes=optim)
        ctx = infRes.session.ctx
        assert ctx.info('observed_set') == 1.0 and ctx.info('trial_lengths_set') == 1.0 and np.all(infRes.newton_status == 0)
        _compare_posterior('%s ragged, engine %d, %s start' % (name, cov_mode, start), infRes, optim, ref, lens, p, nll, -total / R)


# ---- 4. the evidence -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cov_mode', [1, 2], indirect=True, ids=['dense', 'lowrank'])
@pytest.mark.parametrize('name,ragged', [('c1', False), ('p10', False), ('c1', True)], ids=['c1', 'p10', 'c1-ragged'])
def test_log_evidence_with_a_table(funs_mod, name, ragged, cov_mode):
    """LAPLACE_EVIDENCE: log Z_r to 1e-9 relative against the plain-numpy formula of test_gpu_laplace_evidence.py on the reduced model of each trial"""
    params, Yr, table, lens, T, _, _ = _case(name, ragged)
    ref = np.array([numpy_log_evidence([Yr[r][table[r]]], reduced(params, table[r]))[0] for r in range(len(Yr))])
    old = funs_mod.inference.LAPLACE_EVIDENCE
    funs_mod.inference.LAPLACE_EVIDENCE = True
    try:
        infRes, _, _ = funs_mod.inference.laplace(observed_experiment(Yr, table), {k: v.copy() for k, v in params.items()})
    finally:
        funs_mod.inference.LAPLACE_EVIDENCE = old
    assert infRes.session.ctx.info('observed_set') == 1.0 and np.all(infRes.newton_status == 0)
    e_z = float(np.max(np.abs(infRes.log_evidence - ref) / np.abs(ref)))
    e_m = abs(infRes.mean_log_evidence - ref.mean()) / abs(ref.mean())
    print('%s%s, engine %d: log Z per trial %.2e, mean %.2e (mean log Z %.6f)' % (name, ' ragged' if ragged else '', cov_mode, e_z, e_m, ref.mean()))
    assert e_z <= 1e-9 and e_m <= 1e-9


# ---- 5. the (C,d) passes ------------------------------------------------------------------------------------------------------------------------------
CD_CASES = {
    'items':  (200, 10, 500, 64),     # 512 / 1024 (trial, bin tile) items on 256 / 128 workgroups: the stride loop, the prefetch of a following item
    'p10':    (60, 10, 150, 12),
    'p12':    (60, 12, 150, 12),      # vector sweep, mstep_cd_hess_kernel
    'p20':    (70, 20, 100, 12),      # mstep_cd_hess_rows_kernel, 4 row groups
    'p27':    (50, 27, 70, 12),       # mstep_cd_hess_rows_kernel, 8 row groups
}
CD_RUNS = [('items', 'default'), ('p10', 'default'), ('p10', 'vector'), ('p12', 'default'), ('p20', 'default'), ('p27', 'default')]
_cd_cache = {}


def _masked_sums(vec, pr, lens, table, want_hess=True):
    """dense._cd_sums per trial over its own bins, the rows of unobserved neurons dropped, summed over the trials"""
    out = None
    for r, L in enumerate(lens):
        s = dense._cd_sums(vec, pr['M'][r:r + 1, :, :L], pr['V'][r:r + 1, :L], pr['Y'][r:r + 1, :, :L], want_hess=want_hess)
        o = table[r].astype(np.float64)
        s = [a * o.reshape((-1,) + (1,) * (a.ndim - 1)) for a in s]
        out = s if out is None else [a + b for a, b in zip(out, s)]
    return tuple(out)


def _cd_case(name, ragged):
    """problem, table, lengths and the FP64 sums over observed pairs at v0 and v1: once per (case, lengths), shared by forms and prior settings"""
    if (name, ragged) not in _cd_cache:
        _cd_cache.clear()
        q, p, T, R = CD_CASES[name]
        pr = dense._cd_problem(q, p, T, R, seed=77 + 3 * q + T)
        table = seam_table(R, q)
        lens = ragged_lengths(R, T, seed=R + T, n_distinct=6) if ragged else np.full(R, T, dtype=np.int32)
        s0 = _masked_sums(pr['v0'], pr, lens, table)
        v1 = pr['v0'] + 0.3 * dense._step(*dense._with_prior(pr['v0'], s0, R, None)[2:])[0].T.reshape(-1)
        s1 = _masked_sums(v1, pr, lens, table, want_hess=False)
        _cd_cache[(name, ragged)] = (pr, table, lens, v1, s0, s1)
    return _cd_cache[(name, ragged)]


def _cd_context(pr, table, lens, form):
    """counts zero at padded bins and unobserved rows; the posterior NaN at padded bins (whatever read them would show)"""
    from funs import _hip
    q, p, T, R = pr['dims']
    Y = pr['Y'].copy()
    M, V = pr['M'].copy(), pr['V'].copy()
    for r, L in enumerate(lens):
        Y[r, :, L:] = 0
        Y[r, ~table[r]] = 0
        M[r, :, L:] = np.nan
        V[r, L:] = np.nan
    ctx = _hip.Context(q, p, T, R, BIN_MS)
    try:
        ctx.upload_counts(Y if Y.max() > 255 else Y.astype(np.uint8))
        for key in (('cd_mfma', 'cd_hess_mfma') if form == 'vector' else ()):
            ctx.set_option(key, 0)
        ctx.set_params(pr['C'], pr['d'], pr['tau_s'])
        if np.any(lens != T):
            ctx.set_trial_lengths(lens)
        ctx.set_observed(table)
    except Exception:
        ctx.close()
        raise
    return ctx, M, V


@pytest.mark.timeout(900)
@pytest.mark.parametrize('prior', [False, True], ids=['plain', 'prior'])
@pytest.mark.parametrize('ragged', [False, True], ids=['equal', 'ragged'])
@pytest.mark.parametrize('name,form', CD_RUNS, ids=['%s-%s' % r for r in CD_RUNS])
def test_cd_passes_with_a_table(name, form, ragged, prior):
    """A synthetic posterior through pgpfa_set_posterior, a table of the seam patterns, without and with per-trial lengths: costgrad, Newton pass,
    chord pass and per-neuron cost against plain FP64 numpy summed over the observed (trial, neuron) pairs (and the bins t < T_r), per neuron as
    test_gpu_mstep_dense.py does: cost 1e-10, gradient, steps and decrements 1e-9; every kernel form that test_cd_passes_on_ragged_posteriors runs
    plus 27 latents (mstep_cd_hess_rows_kernel with 8 row groups).  form 'vector': options cd_mfma = cd_hess_mfma = 0."""
    pr, table, lens, v1, s0, s1 = _cd_case(name, ragged)
    q, p, T, R = pr['dims']
    center = pr['center'] if prior else None
    ref0, ref1 = dense._with_prior(pr['v0'], s0, R, center), dense._with_prior(v1, s1, R, center)
    tag = 'table %s %s %s%s%s' % (name, pr['dims'], form, ' ragged' if ragged else '', ' with prior' if prior else '')
    ctx, M, V = _cd_context(pr, table, lens, form)
    try:
        ctx.set_posterior(None, M, V)
        dense._compare_entry_points(tag, ctx, pr['v0'], v1, center, ref0, ref1)
        assert ctx.info('last_cd_unobserved_neurons') == 0.0 and ctx.info('observed_set') == 1.0
    finally:
        ctx.close()


@pytest.mark.parametrize('name,form', [('p10', 'default'), ('p10', 'vector'), ('p12', 'default'), ('p20', 'default')],
                         ids=['p10-default', 'p10-vector', 'p12-default', 'p20-default'])
def test_a_neuron_without_an_observed_trial_in_the_list(name, form):
    """An M-step over a list of trials none of which observes neuron 20 (an online minibatch): its gradient, Newton step, chord step and decrement
    are EXACTLY zero without a prior, last_cd_unobserved_neurons = 1, every other neuron is held to numpy over the list (1e-9); with a prior
    only the prior acts on it: gradient inv_s2 (v - center), Newton step center - v (1e-12: a (p+1)-dim solve with inv_s2 I)."""
    pr, table, lens, _, _, _ = _cd_case(name, False)
    q, p, T, R = pr['dims']
    tb = table.copy()
    tb[:, 20] = False
    tb[0, 20] = True                                                 # observed on trial 0 only, which the list leaves out
    lst = np.array([5, 2, 7, 1, 9, 4], dtype=np.int32)
    ctx, M, V = _cd_context(pr, tb, lens, form)
    try:
        ctx.set_posterior(lst, M[lst], V[lst])
        sub = {'M': pr['M'][lst], 'V': pr['V'][lst], 'Y': pr['Y'][lst]}
        s0 = _masked_sums(pr['v0'], sub, lens[lst], tb[lst])
        others = np.arange(q) != 20
        for center in (None, pr['center']):
            kw = {} if center is None else {'prior_center': center, 'inv_s2': INV_S2}
            cost_r, _, g_r, H_r = dense._with_prior(pr['v0'], s0, len(lst), center)
            cost, grad = ctx.mstep_cd_costgrad(pr['v0'], **kw)
            cost_n, delta, dec = ctx.mstep_cd_newton_pass(pr['v0'], **kw)
            assert ctx.info('last_cd_unobserved_neurons') == 1.0
            _, delta_c, dec_c = ctx.mstep_cd_chord_pass(pr['v0'], **kw)
            g20, d20, c20 = grad.reshape(p + 1, q)[:, 20], delta.reshape(p + 1, q)[:, 20], delta_c.reshape(p + 1, q)[:, 20]
            d_ref, dec_ref = dense._step(g_r[others], H_r[others])
            e_g = dense._rows(grad.reshape(p + 1, q)[:, others], g_r[others])
            e_d = dense._rows(delta.reshape(p + 1, q)[:, others], d_ref)
            print('%s %s%s: neuron 20: max |gradient| %.3e, |Newton step| %.3e, |chord step| %.3e, decrement %.3e; the others: gradient %.2e, step %.2e'
                  % (name, form, '' if center is None else ' with prior', np.max(np.abs(g20)), np.max(np.abs(d20)), np.max(np.abs(c20)), dec[20], e_g, e_d))
            assert e_g <= 1e-9 and e_d <= 1e-9 and np.all(np.isfinite(delta)) and np.all(np.isfinite(delta_c))
            if center is None:
                assert not g20.any() and not d20.any() and not c20.any() and dec[20] == 0.0 and dec_c[20] == 0.0 and cost_n[20] == 0.0
            else:
                dv = (pr['v0'] - center).reshape(p + 1, q)[:, 20]
                assert np.max(np.abs(g20 - INV_S2 * dv)) <= 1e-12 * np.max(np.abs(INV_S2 * dv)) and np.max(np.abs(d20 + dv)) <= 1e-12 * np.max(np.abs(dv))
                assert np.max(np.abs(d20)) > 0.0
    finally:
        ctx.close()


# ---- 6. invariance ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,options', [('c1', ()), ('p10', ()), ('p10', (('use_mfma', 0),)), ('p12', ()), ('p20', ()), ('p20', (('dual_gemm', 0),))],
                         ids=['c1', 'p10', 'p10-vector', 'p12', 'p20', 'p20-vector'])
def test_parameters_of_an_unobserved_neuron_change_no_bit(name, options):
    """C[n], d[n] of a neuron unobserved on every listed trial do not enter the E-step over the list: objective, modes, blocks and post_vsmGP are
    bit-identical after they are replaced by other (large) values."""
    from funs import _hip
    params, Yr, table, lens, T, _, _ = _case(name)
    R, q, p = len(Yr), Yr[0].shape[0], params['C'].shape[1]
    lst = np.array([3, 1], dtype=np.int32)                            # 'only neurons 0..15' and 'lacks {0, 15, 16, q-1}': both lack the last neuron
    n = q - 1
    assert not table[lst, n].any() and table[0, n]
    got = []
    for moved in (False, True):
        C, d = params['C'].copy(), np.asarray(params['d'], dtype=np.float64).reshape(-1).copy()
        if moved:
            C[n] = 3.0 - 2.0 * C[n]
            d[n] = d[n] + 5.0
        ctx = _hip.Context(q, p, T, R, BIN_MS)
        try:
            ctx.upload_counts(padded_counts(Yr, table, T))
            for key, value in options:
                ctx.set_option(key, value)
            ctx.set_params(C, d, params['tau'])
            ctx.set_observed(table)
            obj, _, st = ctx.estep_laplace(lst)
            assert np.all(st == 0)
            got.append([np.array([obj]), ctx.post_mean(lst), ctx.post_vsm(lst), ctx.post_vsmgp(lst)])
        finally:
            ctx.close()
    same = [np.array_equal(a, b) for a, b in zip(*got)]
    print('%s %s: objective, modes, post_vsm, post_vsmGP bit-identical: %s' % (name, dict(options), same))
    assert all(same)


# ---- 7. a table of all ones -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('q,p,T,R', [(30, 3, 100, 8), (40, 10, 176, 4), (50, 20, 48, 4)], ids=['p3', 'p10', 'p20'])
def test_a_table_of_all_ones_changes_no_bit(q, p, T, R):
    """pgpfa_set_observed with every byte set against no call: bit-identical objective, modes, blocks, PautoSum, (C,d) cost, gradient and Newton
    step, count moments (as test_all_lengths_equal_to_T_changes_no_bit)."""
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
                ctx.set_observed(np.ones((R, q), dtype=np.uint8))
            assert ctx.info('observed_set') == float(with_table)
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
    print('p = %d: bit-identical with a table of ones: %s' % (p, same))
    assert all(same)


# ---- 8. EM end to end on config 1 stitched from two sessions ---------------------------------------------------------------------------------------
def stitched_config1():
    g = load_golden('c1_dataset.npz')
    Ys = [g['Y'][r].astype(np.float64) for r in range(g['Y'].shape[0])]
    R, q = len(Ys), Ys[0].shape[0]
    n = np.arange(q)
    table = np.stack([(n < -(-2 * q // 3)) if r < R // 2 else (n >= q // 3) for r in range(R)])
    return g, Ys, table


def cd_grad_observed(vec, Ys, pm, pv, table, p, q):
    """orc.mstep_cd_grad with the sums over observed (trial, neuron) pairs only; the reference's 1 / numTrials stays"""
    C, d = orc.vec_to_cd(vec, p, q)
    dC, dd = np.zeros((q, p)), np.zeros(q)
    for Y, m, V, o in zip(Ys, pm, pv, table):
        _, a, b = orc.mstep_cd_terms(orc.cd_to_vec(C[o], d[o]), [np.asarray(Y, dtype=np.float64)[o]], [m], [V], p, int(o.sum()))
        dC[o] += a
        dd[o] += b
    return -orc.cd_to_vec(dC, dd) / len(Ys)


def _stationarity(par, Ys, table, pm):
    """max |gradient of the reduced log-posterior| over the trials at the device's modes (the criterion of the ragged tests)"""
    worst = 0.0
    kinv = {}
    for Y, o, X in zip(Ys, table, pm):
        L = X.shape[1]
        if L not in kinv:
            kinv[L] = np.linalg.inv(orc.make_K(par['tau'], L, BIN_MS))
        worst = max(worst, float(np.max(np.abs(orc.nlp_grad(X, np.asarray(Y, dtype=np.float64)[o], par['C'][o], par['d'].reshape(-1)[o], kinv[L])))))
    return worst


def numpy_initialize(Ys, table, p):
    """the initialiser's moments restated: per-neuron and co-observed sample counts from the table, then the reference's Poisson-PCA"""
    T = Ys[0].shape[1]
    Z = np.stack([np.where(o[:, None], y, 0.0) for y, o in zip(Ys, table)])
    s, S = Z.sum(axis=(0, 2)), np.einsum('rit,rjt->ij', Z, Z)
    O = table.astype(np.float64)
    n_i, n_ij = O.sum(axis=0) * T, O.T @ O * T
    mean = s / n_i + 1e-10
    with np.errstate(invalid='ignore', divide='ignore'):
        cov = np.where(n_ij >= 2, (S - np.outer(s, s) * n_ij / np.outer(n_i, n_i)) / (n_ij - 1.0), 0.0)
    outer = np.outer(mean, mean)
    lamb = np.log(np.abs(cov + outer - np.diag(mean))) - np.log(outer)
    evals, evecs = np.linalg.eig(lamb)
    return evecs[:, np.argsort(evals)[::-1]][:, :p], np.log(mean)


@pytest.mark.timeout(900)
def test_batch_em_on_stitched_config1(funs_mod):
    """Config 1 as two sessions: the first half of the trials observes neurons 0..19, the second 10..29.  initializeParams equals its numpy
    restatement to 1e-10 (columns up to LAPACK's sign); three batch-EM iterations (CdOptimMethod='newton'): every mode is stationary for its
    reduced problem (1e-6), the new (C,d) zero the oracle's gradient summed over observed pairs (2e-6), the new timescales orc.tau_grad on
    PautoSum (1e-6 R) - the criteria of test_batch_em_on_ragged_config1."""
    from funs import _session
    _session.drop_sessions()
    _, Ys, table = stitched_config1()
    R, q, p = len(Ys), Ys[0].shape[0], 3
    exp = observed_experiment(Ys, table)
    np.random.seed(5)
    init = funs_mod.util.initializeParams(p, q, exp)
    C_ref, d_ref = numpy_initialize(Ys, table, p)
    Cd, Cr = np.real(init['C']), np.real(C_ref)
    sign = np.sign(np.sum(Cd * Cr, axis=0))
    errs = {'C': float(np.max(np.abs(Cd * sign - Cr))), 'd': float(np.max(np.abs(init['d'] - d_ref)))}
    print('initializeParams against its numpy restatement: %s (column signs %s)' % (errs, sign.tolist()))
    assert np.all(np.abs(sign) == 1.0) and max(errs.values()) <= 1e-10
    params = {k: np.real(np.asarray(v)).astype(np.float64) for k, v in init.items()}
    optim = None
    for it in range(3):
        infRes, nll, optim = funs_mod.inference.laplace(exp, params, prevOptimRes=optim)
        assert np.all(infRes.newton_status == 0) and infRes.session.ctx.info('observed_set') == 1.0
        pm = [np.array(infRes['post_mean'][r]) for r in range(R)]
        pv = [np.array(infRes['post_vsm'][r]) for r in range(R)]
        new, _ = funs_mod.learning.updateParams(params, infRes, exp, CdOptimMethod='newton')
        P = infRes.session.ctx.pautosum()
        worst = _stationarity(params, Ys, table, pm)
        g_cd = float(np.max(np.abs(cd_grad_observed(orc.cd_to_vec(new['C'], new['d']), Ys, pm, pv, table, p, q))))
        logp = np.log(1.0 / (new['tau'] * 1000.0 / BIN_MS) ** 2)
        g_tau = max(abs(orc.tau_grad(logp[k], P[k], R)[0]) for k in range(p))
        print('batch EM iteration %d: nPLL %.6f, worst |grad| of a mode %.2e, |(C,d) gradient| %.2e, |timescale gradient| %.2e' % (it, nll, worst, g_cd, g_tau))
        assert worst <= 1e-6 and g_cd <= 2e-6 and g_tau <= 1e-6 * R
        params = new
    _session.drop_sessions()


@pytest.mark.timeout(900)
def test_online_diag_em_on_stitched_config1(funs_mod):
    """Three stochastic-EM iterations with the 'diag' prior on minibatches of 6 (the parent's resident counts and table): every mode stationary
    for its reduced trial (1e-6), the new (C,d) zero the regularised gradient over the minibatch's observed pairs (2e-6), the new timescales the
    reference's regularised timescale gradient (1e-6 batch) - the criteria of test_online_diag_em_on_ragged_config1."""
    from funs import _session
    _session.drop_sessions()
    g, Ys, table = stitched_config1()
    R, q, p, batch = len(Ys), Ys[0].shape[0], 3, 6
    exp = observed_experiment(Ys, table)
    params = {'C': g['init_C'].copy(), 'd': g['init_d'].copy(), 'tau': g['init_tau'].copy()}
    np.random.seed(11)
    prior = np.diag(np.ones(q * (p + 1)))
    for n in range(3):
        sz = 1.0 / (n + 1) ** 0.75
        sub = funs_mod.util.subsampleTrials(exp, batch)
        idx = np.asarray(sub.batchTrIdx)
        infRes, nll, _ = funs_mod.inference.laplace(sub, params, prevOptimRes='resident')
        assert infRes.session is _session.session_for(exp, p)[0] and infRes.session.ctx.info('observed_set') == 1.0
        Yb, tb = [Ys[i] for i in idx], table[idx]
        pm = [np.array(infRes['post_mean'][j]) for j in range(batch)]
        pv = [np.array(infRes['post_vsm'][j]) for j in range(batch)]
        new, _, prior = funs_mod.learning.updateParamsWithPrior(params, infRes, sub, 'newton', 'lockstep', sz, sz, prior, covOpts='useDiag')
        missing = int(infRes.session.ctx.info('last_cd_unobserved_neurons'))
        assert missing == int((~tb.any(axis=0)).sum())
        P = infRes.session.ctx.pautosum()
        worst = _stationarity(params, Yb, tb, pm)
        old_vec, new_vec = orc.cd_to_vec(params['C'], params['d']), orc.cd_to_vec(new['C'], new['d'])
        g_cd = float(np.max(np.abs(cd_grad_observed(new_vec, Yb, pm, pv, tb, p, q) - prior @ (new_vec - old_vec))))
        logp = np.log(1.0 / (new['tau'] * 1000.0 / BIN_MS) ** 2)
        g_tau = max(abs(orc.tau_grad_prior(logp[k], P[k], batch, BIN_MS, params['tau'][k], sz)[0]) for k in range(p))
        print('online EM iteration %d (trials %s, %d neurons without an observed trial): worst |grad| of a mode %.2e, |(C,d) gradient| %.2e, '
              '|timescale gradient| %.2e' % (n, idx.tolist(), missing, worst, g_cd, g_tau))
        assert worst <= 1e-6 and g_cd <= 2e-6 and g_tau <= 1e-6 * batch
        params = new
    _session.drop_sessions()


def test_fit_object_on_a_stitched_experiment(funs_mod):
    """engine.PPGPFAfit in Batch mode with trackEvidence and emTol, in Online mode, and crossValidation(score='evidence'), on the stitched
    experiment: finite likelihoods, evidences and parameters; trajectories extract."""
    from funs import _session
    _session.drop_sessions()
    g, Ys, table = stitched_config1()
    exp = observed_experiment(Ys, table)
    init = {'C': g['init_C'].copy(), 'd': g['init_d'].copy(), 'tau': g['init_tau'].copy()}
    fit = funs_mod.engine.PPGPFAfit(exp, initParams={k: v.copy() for k, v in init.items()}, EMmode='Batch', maxEMiter=3, CdOptimMethod='newton', quiet=True,
                                    trackEvidence=True, emTol=1e-12)
    print('batch fit: nPLL %s, mean log evidence %s' % (np.round(fit.posteriorLikelihood, 4).tolist(), np.round(fit.logEvidence, 4).tolist()))
    assert np.all(np.isfinite(fit.posteriorLikelihood)) and len(fit.logEvidence) == 3 and np.all(np.isfinite(fit.logEvidence))
    assert all(np.all(np.isfinite(fit.optimParams[k])) for k in ('C', 'd', 'tau'))
    fit.extractTrajectories()
    for method in ('diag', 'hess', 'grad'):
        np.random.seed(3)
        fit = funs_mod.engine.PPGPFAfit(exp, initParams={k: v.copy() for k, v in init.items()}, EMmode='Online', maxEMiter=2, batchSize=5,
                                        onlineParamUpdateMethod=method, quiet=True, trackEvidence=True)
        assert np.all(np.isfinite(fit.posteriorLikelihood)) and all(np.all(np.isfinite(fit.optimParams[k])) for k in ('C', 'd', 'tau')), method
    np.random.seed(4)
    half = observed_experiment(Ys, table)
    half.data = [half.data[i] for i in (0, 1, 2, 3, 10, 11, 12, 13, 4, 14)]              # training: 8 trials of both sessions; test: one of each
    half.numTrials = len(half.data)
    cv = funs_mod.util.crossValidation(half, numTrainingTrials=8, numTestTrials=2, maxXdim=2, maxEMiter=2, score='evidence')
    print('crossValidation(score=evidence) on a stitched experiment: %s' % np.round(cv.errs, 5).tolist())
    assert np.all(np.isfinite(cv.errs))
    _session.drop_sessions()


# ---- 9. rates, samples, co-smoothing -------------------------------------------------------------------------------------------------------------------
def test_posterior_rates_and_samples_cover_unobserved_neurons(funs_mod):
    """posteriorRates over all neurons: the rate of an unobserved neuron is the documented exp(eta + var / 2) on the returned planes, with eta and
    var against numpy on the device's own posterior (1e-12 of their sums of absolute terms, as test_gpu_posterior_rates.py); ell is NaN exactly at
    the unobserved pairs; posteriorSamples runs and draws counts for every neuron."""
    from funs import _session
    _session.drop_sessions()
    params, Yr, table, lens, T, _, _ = _case('c1')
    R, q, p = len(Yr), Yr[0].shape[0], 3
    exp = observed_experiment(Yr, table)
    par = {k: v.copy() for k, v in params.items()}
    infRes, _, _ = funs_mod.inference.laplace(exp, par)
    out = funs_mod.util.posteriorRates(par, exp, infRes=infRes, want=('rate', 'eta', 'var', 'ell', 'lower', 'upper'))
    per_s = 1000.0 / BIN_MS
    C, d = params['C'], params['d'].reshape(-1)
    e_eta = e_var = 0.0
    for r in range(R):
        m, S = infRes['post_mean'][r], infRes['post_vsm'][r]
        eta = C @ m + d[:, None]
        var = np.einsum('nk,tkl,nl->nt', C, S, C)
        a_eta = np.abs(C) @ np.abs(m) + np.abs(d)[:, None]
        a_var = np.einsum('nk,tkl,nl->nt', np.abs(C), np.abs(S), np.abs(C))
        e_eta = max(e_eta, float(np.max(np.abs(out['eta'][r] - eta) / a_eta)))
        e_var = max(e_var, float(np.max(np.abs(out['var'][r] - var) / a_var)))
    e_rate = rel(out['rate'], np.exp(out['eta'] + 0.5 * out['var']) * per_s)
    print('rates under a table: eta %.2e, var %.2e of their scales (limit 1e-12), rate against exp(eta + var / 2): %.2e; NaN ell entries %d of %d unobserved pairs'
          % (e_eta, e_var, e_rate, int(np.isnan(out['ell']).sum()), int((~table).sum())))
    assert e_eta <= 1e-12 and e_var <= 1e-12 and e_rate <= 1e-12
    assert out['rate'].shape == (R, q, T) and np.all(np.isfinite(out['rate'])) and np.all(out['lower'] <= out['rate']) and np.all(out['rate'] <= out['upper'])
    assert np.array_equal(np.isnan(out['ell']), ~table)
    smp = funs_mod.util.posteriorSamples(par, exp, infRes=infRes, trials=[0, 2, 3], nSamples=4, seed=1, want=('x', 'y'))
    assert smp['x'].shape == (3, 4, p, T) and smp['y'].shape == (3, 4, q, T) and np.all(np.isfinite(smp['x']))
    _session.drop_sessions()


def test_co_smoothing_against_the_oracle(funs_mod):
    """util.coSmoothing(held-out neurons 3, 17, 18, 25 on every trial of config 1, on top of a table that already hides neuron 5 on trial 2 and the
    held-out neuron 17 on trial 4) against the same score computed in numpy from the oracle's posterior of the reduced model.  The rate tolerance
    of test_gpu_posterior_rates.py - the E-step's 1e-8 on modes and blocks propagated through |C|: |d eta| <= 1e-8 sum_k |C_nk|, |d var| <= 1e-8
    max|Sigma| (sum_k |C_nk|)^2 - gives a relative rate error delta_n = |d eta| + |d var| / 2 and a score error of at most
    sum (y + lam) delta_n / (log 2 sum y).  The experiment's session, its table and its resident posterior stay as they were."""
    from funs import _session
    _session.drop_sessions()
    g = load_golden('c1_dataset.npz')
    Ys = [g['Y'][r].astype(np.float64) for r in range(g['Y'].shape[0])]
    R, q, p = len(Ys), Ys[0].shape[0], 3
    params = {'C': g['init_C'].copy(), 'd': g['init_d'].copy(), 'tau': g['init_tau'].copy()}
    own = np.ones((R, q), dtype=bool)
    own[2, 5] = False
    own[4, 17] = False
    exp = observed_experiment(Ys, own)
    infRes, _, _ = funs_mod.inference.laplace(exp, {k: v.copy() for k, v in params.items()})
    sess = infRes.session
    before = (sess.observed.copy(), sess.post_stamp, np.array(infRes['post_mean'][4]))
    held = np.array([3, 17, 18, 25])
    out = funs_mod.util.coSmoothing(params, exp, held)
    assert np.array_equal(sess.observed, before[0]) and sess.post_stamp == before[1] and sess.ctx.info('observed_set') == 1.0
    assert np.array_equal(sess.ctx.post_mean(np.array([4], dtype=np.int32))[0], before[2])
    # the oracle: posterior of every trial without the held-out neurons (and without what the experiment itself hides), then the same score
    masked = own.copy()
    masked[:, held] = False
    ref, _ = oracle_reduced(Ys, masked, params)
    C, d = params['C'][held], params['d'].reshape(-1)[held]
    c1n = np.abs(C).sum(axis=1)
    lam, delta = [], []
    for r in range(R):
        m, S = ref['post_mean'][r], ref['post_vsm'][r]
        lam.append(np.exp(C @ m + d[:, None] + 0.5 * np.einsum('nk,tkl,nl->nt', C, S, C)))
        delta.append(1e-8 * c1n + 0.5 * 1e-8 * np.max(np.abs(S)) * c1n ** 2 + 1e-12)
    lam = np.stack(lam)
    scored = own[:, held]                                                # (R, 4): the pairs the experiment observed
    y = np.stack([Y[held] for Y in Ys]) * scored[:, :, None]
    bins = scored.sum(axis=0) * Ys[0].shape[1]
    lbar = y.sum(axis=(0, 2)) / bins
    ll = ((y * np.log(lam) - lam) - (y * np.log(lbar)[None, :, None] - lbar[None, :, None])) * scored[:, :, None]
    score_ref = ll.sum() / (np.log(2.0) * y.sum())
    per_neuron_ref = ll.sum(axis=(0, 2)) / (np.log(2.0) * y.sum(axis=(0, 2)))
    bound = float(np.sum((y + lam) * np.stack(delta)[:, :, None] * scored[:, :, None]) / (np.log(2.0) * y.sum()))
    per_s = 1000.0 / BIN_MS
    e_rate = max(float(np.max(np.abs(out['rate'][r] / per_s - lam[r]) / (lam[r] * delta[r][:, None]))) for r in range(R))
    e_score = abs(out['bitsPerSpike'] - score_ref)
    print('coSmoothing: %.6f bits per spike (oracle %.6f), difference %.2e (bound %.2e); rates %.3f of their propagated bound; per neuron %s'
          % (out['bitsPerSpike'], score_ref, e_score, bound, e_rate, np.round(out['bitsPerSpikePerNeuron'], 4).tolist()))
    assert e_rate <= 1.0 and e_score <= bound
    assert np.max(np.abs(out['bitsPerSpikePerNeuron'] - per_neuron_ref)) <= 10 * bound and np.array_equal(out['heldOut'], held)
    assert len(out['rate']) == R and out['rate'][0].shape == (4, Ys[0].shape[1])
    _session.drop_sessions()


# ---- 10. refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals(funs_mod):
    from funs import _hip, _session
    _session.drop_sessions()
    params, Yr, table, lens, T, _, _ = _case('c1')
    R, q, p = len(Yr), Yr[0].shape[0], 3
    exp = observed_experiment(Yr, table)
    par = lambda: {k: v.copy() for k, v in params.items()}
    for call in (lambda: funs_mod.inference.dualVariational(exp, par()), lambda: funs_mod.util.leaveOneOutPrediction(par(), exp),
                 lambda: funs_mod.mcmc.PosteriorMCMC(exp, par(), 2, 0), lambda: funs_mod.mcmc.PosteriorMCMC_batch(exp, par(), 2, [0, 1], [1, 2])):
        with pytest.raises(NotImplementedError, match='unobserved neurons'):
            call()
    host = {'post_mean': [np.zeros((p, T))] * R, 'post_vsm': [np.zeros((T, p, p))] * R, 'post_vsmGP': [np.zeros((T, T, p))] * R}
    with pytest.raises(NotImplementedError, match='unobserved neurons'):
        funs_mod.learning.MStepObservationCost(orc.cd_to_vec(params['C'], params['d']), p, q, exp, host)
    _session.drop_sessions()
    Y = padded_counts(Yr, table, T)
    ctx = _hip.Context(q, p, T, R, BIN_MS)
    try:
        ctx.upload_counts(Y)
        ctx.set_params(params['C'], params['d'], params['tau'])
        tb = table.copy()
        tb[4] = False
        with pytest.raises(_hip.HipBackendError, match='trial 4 has no observed neuron'):
            ctx.set_observed(tb)
        tb = table.copy()
        tb[:, 7] = False
        with pytest.raises(_hip.HipBackendError, match='neuron 7 is observed on no trial'):
            ctx.set_observed(tb)
        with pytest.raises(ValueError, match='shape'):
            ctx.set_observed(table[:, :-1])
        Yb = Y.copy()
        Yb[2, 3, 40] = 2                                               # trial 2 observes neuron 17 only
        Yb[2, 9, 0] = 1
        ctx.upload_counts(Yb)
        with pytest.raises(_hip.HipBackendError, match='trial 2: 2 non-zero counts at unobserved neurons'):
            ctx.set_observed(table)
        assert ctx.info('observed_set') == 0.0
        ctx.upload_counts(Y)
        ctx.set_observed(table)
        assert ctx.info('observed_set') == 1.0
        lam = np.full((1, q * T), 0.5)
        idx = np.zeros(1, dtype=np.int32)
        for call in (lambda: ctx.dual_costgrad(0, lam[0]), lambda: ctx.dual_costgrad_batch(idx, lam), lambda: ctx.dual_lbfgs(idx, np.log(lam)),
                     lambda: ctx.dual_fixed_point(idx), lambda: ctx.dual_finalize(idx, lam), lambda: ctx.dual_post_mean(0, lam[0]),
                     lambda: ctx.dual_post_cov(0, lam[0]), lambda: ctx.loo_predict(idx), lambda: ctx.generate(1)):
            with pytest.raises(_hip.HipBackendError, match='unobserved neurons'):
                call()
        # counts uploaded while a table is set are checked again; the table stays; NULL drops it
        with pytest.raises(_hip.HipBackendError, match='trial 2: 2 non-zero counts at unobserved neurons'):
            ctx.upload_counts(Yb)
        ctx.upload_counts(Y)
        assert ctx.info('observed_set') == 1.0
        obj, _, st = ctx.estep_laplace()
        assert np.all(st == 0) and np.isfinite(obj)
        ctx.set_observed(None)
        assert ctx.info('observed_set') == 0.0
    finally:
        ctx.close()
