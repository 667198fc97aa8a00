"""Option laplace_f32: the r x r phase of the low-rank covariance engine (B = I + F^T Wt F, its Cholesky factor, L^-T) in single precision for
the Laplace E-step, everything behind L^-T in FP64.

Cases (all cov_mode 2; synthetic ones are orc.synth_dataset(q, p, T, R, seed) at the generating parameters):
  c1    config 1, 30 x 3 x 100, first 6 trials, the data set's initial parameters
  p10   40 x 10 x 176, seed 41: the 10-wide fused kernel, two bin blocks per slot  (also with rank_gran 16 and with keep_trial_vsmgp 1)
  p9    33 x 9 x 203, seed 42: 9 latents in the 10-wide instantiation, T no multiple of 16
  p12   35 x 12 x 64, seed 43: unfused, p <= 16
  p20   50 x 20 x 48, seed 51: the wide path

Yardstick: the dense FP64 inverse of orc.nlp_hess at the device's own modes (orc.laplace_cov_at), computed once per case - the modes do not
depend on the option (test b).  Errors are max |error| over the largest entry of post_vsm, of the per-trial post_vsmGP and of PautoSum.
Caps: FP64 run 1e-8 (the project's), laplace_f32 = 2: 2e-6, laplace_f32 = 1: 5e-6 - about 15 x the worst figures of a numpy float32 emulation
of the r x r phase at these shapes and seeds (1.2e-7 / 3.5e-7), the margin being for the device's blocked factorisation, its order of sums and
the truncated low-rank factors.  Every test prints what it measured; the figures are recorded in docs/history/laplace_f32.md.

Measured on an MI355X (worst over post_vsm / post_vsmGP / PautoSum): FP64 run 1.0e-10 ... 3.8e-10; laplace_f32 = 2: c1 1.2e-7, p10 3.8e-7, p9 3.1e-7,
p12 2.3e-7, p20 1.83e-6, p10 with rank_gran 16 3.1e-7; laplace_f32 = 1: c1 6.5e-7, p10 1.9e-6, p9 7.6e-7, p12 1.7e-6, p20 3.75e-6."""
import os

import numpy as np
import pytest

from conftest import load_golden
from oracle import pgpfa_oracle as orc

pytestmark = pytest.mark.gpu

BIN_MS = 10.0
CAP = {0: 1e-8, 1: 5e-6, 2: 2e-6}
SYNTH = {'p10': (40, 10, 176, 6, 41), 'p9': (33, 9, 203, 5, 42), 'p12': (35, 12, 64, 6, 43), 'p20': (50, 20, 48, 6, 51)}
# (case, extra options set before set_params)
VARIANTS = {'c1': ('c1', {}), 'p10': ('p10', {}), 'p9': ('p9', {}), 'p12': ('p12', {}), 'p20': ('p20', {}),
            'p10_gran16': ('p10', {'rank_gran': 16}), 'p10_keep': ('p10', {'keep_trial_vsmgp': 1})}
FLAG_KEYS = ('last_yt_mix_fused', 'last_split_cov', 'plan_lowrank', 'lowrank_rtot')

_problems, _runs, _refs = {}, {}, {}


def _problem(case):
    """(params, Y (R, q, T) uint8, second parameter set: new timescales and loadings)"""
    if case not in _problems:
        if case == 'c1':
            g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'c1_dataset.npz'))
            par = {'C': g['init_C'].astype(np.float64), 'd': g['init_d'].astype(np.float64), 'tau': g['init_tau'].astype(np.float64).reshape(-1)}
            Y = np.asarray(g['Y'][:6])
        else:
            q, p, T, R, seed = SYNTH[case]
            par, Ys, _ = orc.synth_dataset(q, p, T, R, seed)
            Y = np.stack(Ys)
        assert Y.max() <= 255
        par2 = {'C': 1.05 * par['C'], 'd': par['d'] + 0.02, 'tau': 1.3 * par['tau']}
        _problems[case] = (par, Y.astype(np.uint8), par2)
    return _problems[case]


def _collect(ctx, obj, iters, status):
    """everything the tests compare after one E-step; the flags are read before anything rebuilds per-trial blocks"""
    out = {'obj': obj, 'iters': iters.copy(), 'status': status.copy()}
    out['flags'] = {k: ctx.info(k) for k in FLAG_KEYS}
    out['cov_f32'] = ctx.info('last_cov_f32')
    out['fallbacks'] = ctx.info('last_cov_f32_fallbacks')
    assert ctx.mstep_precomp() == float(ctx.R)
    out['P'] = ctx.pautosum().copy()
    out['pm'], out['vsm'] = ctx.post_mean(), ctx.post_vsm()
    out['gp'] = ctx.post_vsmgp()
    return out


def _context(case, opts, f32, cov_mode=2):
    from funs import _hip
    par, Y, _ = _problem(case)
    R, q, T = Y.shape
    ctx = _hip.Context(q, par['C'].shape[1], T, R, BIN_MS)
    ctx.upload_counts(Y)
    ctx.set_option('cov_mode', cov_mode)
    for k, v in opts.items():
        ctx.set_option(k, v)
    if f32 is not None:
        ctx.set_option('laplace_f32', f32)
    ctx.set_params(par['C'], par['d'], par['tau'])
    return ctx


def _run(variant, f32):
    """cold E-step at the case's parameters, then a warm-started one at the second parameter set, in one context"""
    key = (variant, f32)
    if key not in _runs:
        case, opts = VARIANTS[variant]
        par2 = _problem(case)[2]
        ctx = _context(case, opts, f32)
        try:
            cold = _collect(ctx, *ctx.estep_laplace())
            ctx.set_params(par2['C'], par2['d'], par2['tau'])
            warm = _collect(ctx, *ctx.estep_laplace(warm_start=True))
        finally:
            ctx.close()
        assert np.all(cold['status'] == 0) and np.all(warm['status'] == 0)
        _runs[key] = (cold, warm)
    return _runs[key]


def _dense(case, step):
    """dense FP64 post_vsm (R,T,p,p), post_vsmGP (R,T,T,p) and PautoSum (p,T,T) at the device's modes of the FP64 run"""
    key = (case, step)
    if key not in _refs:
        par = _problem(case)[2 if step else 0]
        pm = _run(case, 0)[step]['pm']
        T = pm.shape[2]
        out = [orc.laplace_cov_at(m, par['C'], par['d'], par['tau'], T, BIN_MS) for m in pm]
        vsm, gp = np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
        P = np.sum(gp, axis=0).transpose(2, 0, 1) + np.einsum('rkt,rks->kts', pm, pm)
        for a in (vsm, gp, P):
            a.setflags(write=False)
        _refs[key] = (vsm, gp, P)
    return _refs[key]


def _errors(res, ref):
    def rel(a, b):
        return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
    gp_trial = max(rel(a, b) for a, b in zip(res['gp'], ref[1]))
    return rel(res['vsm'], ref[0]), gp_trial, rel(res['P'], ref[2])


def _check(tag, res, ref, f32):
    assert np.all(np.isfinite(res['vsm'])) and np.all(np.isfinite(res['gp'])) and np.all(np.isfinite(res['P']))
    e = _errors(res, ref)
    print('%s laplace_f32 %d: post_vsm %.2e, post_vsmGP %.2e (worst trial), PautoSum %.2e (cap %.0e); fallbacks %g'
          % (tag, f32, e[0], e[1], e[2], CAP[f32], res['fallbacks']))
    assert max(e) <= CAP[f32], (tag, f32, e)


# ---- a. the option and its bookkeeping -----------------------------------------------------------------------------------------------------
def test_option_values():
    """0, 1 and 2 are accepted, 3 fails with a message (on a library without the option the first call fails: unknown option)"""
    from funs import _hip
    ctx = _hip.Context(8, 2, 16, 1, BIN_MS)
    try:
        for v in (0, 1, 2):
            ctx.set_option('laplace_f32', v)
        with pytest.raises(_hip.HipBackendError, match='laplace_f32'):
            ctx.set_option('laplace_f32', 3)
        assert ctx.info('last_cov_f32') == 0.0 and ctx.info('last_cov_f32_fallbacks') == 0.0
    finally:
        ctx.close()


@pytest.mark.parametrize('variant', list(VARIANTS))
def test_bookkeeping(variant):
    """last_cov_f32 says which form ran; the split verdict, the fused / unfused choice, the plan and the rank total are those of the FP64 run"""
    base = _run(variant, 0)
    for step in (0, 1):
        assert base[step]['cov_f32'] == 0.0 and base[step]['fallbacks'] == 0.0
        assert base[step]['flags']['plan_lowrank'] == 1.0
    for f32 in (1, 2):
        run = _run(variant, f32)
        for step in (0, 1):
            print('%s step %d laplace_f32 %d: %s, fallbacks %g' % (variant, step, f32, run[step]['flags'], run[step]['fallbacks']))
            assert run[step]['cov_f32'] == 1.0
            assert run[step]['flags'] == base[step]['flags']


def test_dense_engine_ignores_the_option():
    """cov_mode 1 with the option set: the dense engine runs in FP64 and says so"""
    case, opts = VARIANTS['c1']
    par = _problem(case)[0]
    ctx = _context(case, opts, 1, cov_mode=1)
    try:
        res = _collect(ctx, *ctx.estep_laplace())
    finally:
        ctx.close()
    assert np.all(res['status'] == 0) and res['flags']['plan_lowrank'] == 0.0 and res['cov_f32'] == 0.0
    T = res['pm'].shape[2]
    out = [orc.laplace_cov_at(m, par['C'], par['d'], par['tau'], T, BIN_MS) for m in res['pm']]
    gp = np.stack([o[1] for o in out])
    P = np.sum(gp, axis=0).transpose(2, 0, 1) + np.einsum('rkt,rks->kts', res['pm'], res['pm'])
    _check('c1 dense engine', res, (np.stack([o[0] for o in out]), gp, P), 0)


# ---- b. phase 1 is untouched ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('variant', list(VARIANTS))
def test_mode_search_bit_identical(variant):
    base = _run(variant, 0)
    for f32 in (1, 2):
        run = _run(variant, f32)
        for step, name in ((0, 'cold'), (1, 'warm, new parameters')):
            for k in ('obj', 'pm', 'iters', 'status'):
                assert np.array_equal(run[step][k], base[step][k]), (variant, f32, name, k)


# ---- c. blocks by value --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('variant', list(VARIANTS))
@pytest.mark.parametrize('f32', [0, 2, 1])
def test_blocks_against_dense_fp64(variant, f32):
    case = VARIANTS[variant][0]
    res = _run(variant, f32)[0]
    if variant != case:                                      # (rank_gran 16 / per-trial blocks kept: the same modes, so the same yardstick)
        assert np.max(np.abs(res['pm'] - _run(case, 0)[0]['pm'])) <= 1e-9
    _check(variant, res, _dense(case, 0), f32)


# ---- d. no state leaks ---------------------------------------------------------------------------------------------------------------------
def test_option_switched_off_leaves_nothing():
    """option 1, E-step, option 0, E-step in one context: the second is the E-step of a context that never heard of the option, bit for bit"""
    base = _run('p10', 0)[0]
    ctx = _context('p10', {}, 1)
    try:
        first = _collect(ctx, *ctx.estep_laplace())
        ctx.set_option('laplace_f32', 0)
        second = _collect(ctx, *ctx.estep_laplace())
    finally:
        ctx.close()
    assert first['cov_f32'] == 1.0 and second['cov_f32'] == 0.0
    for k in ('obj', 'vsm', 'P', 'gp', 'pm'):
        assert np.array_equal(second[k], base[k]), k


def test_option_switched_on_later():
    """the reverse order: FP64 E-step, then option 1 (and 2) in the same context"""
    ref = _dense('p10', 0)
    ctx = _context('p10', {}, None)
    try:
        first = _collect(ctx, *ctx.estep_laplace())
        assert first['cov_f32'] == 0.0
        assert np.array_equal(first['vsm'], _run('p10', 0)[0]['vsm'])
        for f32 in (1, 2):
            ctx.set_option('laplace_f32', f32)
            res = _collect(ctx, *ctx.estep_laplace())
            assert res['cov_f32'] == 1.0
            _check('p10 after an FP64 E-step', res, ref, f32)
    finally:
        ctx.close()


@pytest.mark.parametrize('f32', [2, 1])
def test_new_timescales_between_mixed_esteps(f32):
    """set_params with new timescales between two mixed E-steps (the single-precision factors must follow): the second keeps the caps"""
    res = _run('p10', f32)[1]
    _check('p10 second E-step, new timescales', _run('p10', 0)[1], _dense('p10', 1), 0)
    _check('p10 second E-step, new timescales', res, _dense('p10', 1), f32)


# ---- e. EM, end to end ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(600)
def test_batch_em_with_the_option(c1, c1_experiment):
    """five batch EM iterations on config 1 through the low-rank engine with LAPLACE_F32 = True against the exactly converged EM path
    (c1_em_exact.npz), with the tolerances test_gpu_parity.py::test_batch_em_vs_reference holds the FP64 run to; dualVariational in the same
    session afterwards runs its covariance passes in FP64"""
    import funs
    from funs import _session

    def rel(a, b):
        return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))
    ex = load_golden('c1_em_exact.npz')
    old = (funs.inference.COV_MODE, funs.inference.LAPLACE_F32)
    _session.drop_sessions()
    try:
        funs.inference.COV_MODE, funs.inference.LAPLACE_F32 = 2, True
        init = {k: v.copy() for k, v in c1['init'].items()}
        fit = funs.engine.PPGPFAfit(c1_experiment, initParams=init, inferenceMethod='laplace', EMmode='Batch', maxEMiter=5, quiet=True)
        nll = np.asarray(fit.posteriorLikelihood)
        e_nll = float(np.max(np.abs(nll - ex['nll'])))
        e_par = [max(rel(fit.paramSeq[i][k], ex['seq_' + k][i]) for i in range(1, 6)) for k in ('C', 'd', 'tau')]
        print('batch EM with LAPLACE_F32: nPLL %.2e (5e-5), C %.2e, d %.2e (1e-4), tau %.2e (1e-5)' % (e_nll, *e_par))
        params = {k: np.asarray(v, dtype=np.float64).copy() for k, v in fit.paramSeq[5].items()}
        infRes, _, _ = funs.inference.laplace(c1_experiment, params)
        ctx = infRes.session.ctx
        assert ctx.info('plan_lowrank') == 1.0 and ctx.info('last_cov_f32') == 1.0
        assert e_nll <= 5e-5 and e_par[0] <= 1e-4 and e_par[1] <= 1e-4 and e_par[2] <= 1e-5
        vi = funs.inference.dualVariational(c1_experiment, params)
        assert vi[0].session.ctx is ctx
        assert ctx.info('last_cov_f32') == 0.0
    finally:
        funs.inference.COV_MODE, funs.inference.LAPLACE_F32 = old
        _session.drop_sessions()
