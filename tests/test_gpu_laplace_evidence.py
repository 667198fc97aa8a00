"""Laplace log evidence per trial (C-ABI option laplace_evidence, inference.LAPLACE_EVIDENCE):

    log Z_r = -f_r(x*_r) - 1/2 (log det H_r(x*_r) + sum_k log det K_k)

in the reference's normalisation (sum log y! dropped).  The yardstick is plain FP64 numpy from the oracle's functions: the polished mode of
orc.newton_mode on the trial - cut to its own length where lengths differ -, orc.nlp there, np.linalg.slogdet of orc.nlp_hess and of the Gram
matrices of orc.make_K.  Every log Z_r and every mean of them is held to 1e-9 relative, the tolerance of the two scalars of the same make-up
(nPLL: test_gpu_unequal_trials.py; the dual cost, which carries the same log-det through both engines: test_gpu_round3.py, test_gpu_round4.py).
Every test prints the figure it measured before it asserts."""
import numpy as np
import pytest

from conftest import Experiment, load_golden
from oracle import pgpfa_oracle as orc
from test_gpu_unequal_trials import BIN_MS, _estep_problem, cov_mode, cut, funs_mod, ragged_lengths  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

TOL = 1e-9
CASES = ['c1', 'p10', 'p12', 'p20']


# ---- the yardstick -----------------------------------------------------------------------------------------------------------------------------
_prior_cache = {}


def _prior(tau, L):
    """(K_k^-1 of the L-bin model, sum_k log det K_k)"""
    key = (np.asarray(tau, dtype=np.float64).tobytes(), int(L))
    if key not in _prior_cache:
        K = orc.make_K(tau, int(L), BIN_MS)
        _prior_cache[key] = (np.linalg.inv(K), float(sum(np.linalg.slogdet(K[k])[1] for k in range(K.shape[0]))))
    return _prior_cache[key]


def numpy_log_evidence(Ys, params):
    """log Z of every trial, each in the model of its own length"""
    C, d = np.asarray(params['C'], dtype=np.float64), np.asarray(params['d'], dtype=np.float64).reshape(-1)
    out = np.empty(len(Ys))
    for r, Y in enumerate(Ys):
        Y = np.asarray(Y, dtype=np.float64)
        Kinv, ldK = _prior(params['tau'], Y.shape[1])
        X, _, _ = orc.newton_mode(Y, C, d, Kinv)
        sign, ldH = np.linalg.slogdet(orc.nlp_hess(X, Y, C, d, Kinv))
        assert sign == 1.0
        out[r] = -orc.nlp(X, Y, C, d, Kinv) - 0.5 * (ldH + ldK)
    return out


_ref_cache = {}


def _case(name, ragged):
    """(params, trials - cut where ragged -, lengths, T, numpy's log Z per trial): computed once, shared, never written to"""
    if (name, ragged) not in _ref_cache:
        params, Ys, T = _estep_problem(name)
        lens = ragged_lengths(len(Ys), T, seed=len(name) + T, n_distinct=5 if name == 'c1' else 4) if ragged else np.full(len(Ys), T, dtype=np.int32)
        Yr = cut(Ys, lens)
        ref = numpy_log_evidence(Yr, params)
        ref.setflags(write=False)
        _ref_cache[(name, ragged)] = (params, Yr, lens, T, ref)
    return _ref_cache[(name, ragged)]


def rel_each(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.abs(b)))


@pytest.fixture()
def evidence_on(funs_mod):
    old = funs_mod.inference.LAPLACE_EVIDENCE
    funs_mod.inference.LAPLACE_EVIDENCE = True
    yield
    funs_mod.inference.LAPLACE_EVIDENCE = old


def _padded_counts(Yr, T):
    Y = np.zeros((len(Yr), Yr[0].shape[0], T), dtype=np.uint8)
    for r, y in enumerate(Yr):
        Y[r, :, :y.shape[1]] = y
    return Y


def _context(name, engine, ragged=False, options=()):
    from funs import _hip
    params, Yr, lens, T, ref = _case(name, ragged)
    ctx = _hip.Context(Yr[0].shape[0], params['C'].shape[1], T, len(Yr), BIN_MS)
    ctx.upload_counts(_padded_counts(Yr, T))
    ctx.set_option('cov_mode', engine)
    for key, value in options:
        ctx.set_option(key, value)
    ctx.set_params(params['C'], params['d'], params['tau'])
    if ragged:
        ctx.set_trial_lengths(lens)
    return ctx, ref


# ---- 1. per trial, both engines ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cov_mode', [1, 2], indirect=True, ids=['dense', 'lowrank'])
@pytest.mark.parametrize('ragged', [False, True], ids=['equal', 'ragged'])
@pytest.mark.parametrize('name', CASES)
def test_log_evidence_per_trial(funs_mod, evidence_on, name, ragged, cov_mode):
    """inference.laplace with LAPLACE_EVIDENCE on, cold and from the resident modes: infRes.log_evidence[r] and mean_log_evidence against numpy,
    1e-9 relative; Context.log_evidence() hands out the same array bit for bit."""
    params, Yr, lens, T, ref = _case(name, ragged)
    exp = Experiment(Yr, BIN_MS)
    optim = None
    for start in ('cold', 'resident'):
        infRes, _, optim = funs_mod.inference.laplace(exp, {k: v.copy() for k, v in params.items()}, prevOptimRes=optim)
        ctx = infRes.session.ctx
        assert np.all(infRes.newton_status == 0) and ctx.info('last_cov_lowrank') == float(cov_mode == 2)
        assert ctx.info('trial_lengths_set') == float(ragged)
        z = infRes.log_evidence
        assert isinstance(z, np.ndarray) and z.dtype == np.float64 and z.shape == (len(Yr),)
        e_z, e_m = rel_each(z, ref), abs(infRes.mean_log_evidence - ref.mean()) / abs(ref.mean())
        print('%s %s, engine %d, %s start: log Z per trial %.2e, mean %.2e (mean log Z %.6f)' % (name, 'ragged' if ragged else 'equal', cov_mode, start, e_z, e_m, ref.mean()))
        assert e_z <= TOL and e_m <= TOL
        assert np.array_equal(ctx.log_evidence(), z)
        e_s = abs(ctx.info('last_log_evidence_sum') - ref.sum()) / abs(ref.sum())
        assert e_s <= TOL


def test_switch_off_leaves_no_evidence(funs_mod):
    params, Yr, _, _, _ = _case('c1', False)
    from funs import _session
    _session.drop_sessions()
    assert funs_mod.inference.LAPLACE_EVIDENCE is False
    infRes, _, _ = funs_mod.inference.laplace(Experiment(Yr, BIN_MS), {k: v.copy() for k, v in params.items()})
    assert infRes.log_evidence is None and infRes.mean_log_evidence is None
    _session.drop_sessions()


# ---- 2. chunks and trial lists ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('engine', [1, 2], ids=['dense', 'lowrank'])
def test_chunks_and_trial_lists(engine):
    """Config 1 with chunk_trials = 6: an E-step over an unsorted, non-contiguous list of 7 trials (two chunks) gives those 7 values to 1e-9 and
    none for the other trials; one over all 20 trials (four chunks, the last one partly filled) all 20; one with the option off afterwards
    invalidates every value."""
    from funs import _hip
    ctx, ref = _context('c1', engine, options=(('chunk_trials', 6), ('laplace_evidence', 1)))
    try:
        R = ref.size
        idx = np.array([13, 2, 17, 5, 19, 0, 8], dtype=np.int32)
        _, _, st = ctx.estep_laplace(idx)
        assert np.all(st == 0) and ctx.info('chunk_trials') == 6.0
        e_list = rel_each(ctx.log_evidence(idx), ref[idx])
        print('engine %d, list %s in chunks of 6: log Z %.2e' % (engine, idx.tolist(), e_list))
        assert e_list <= TOL
        for t in sorted(set(range(R)) - set(idx.tolist())):
            with pytest.raises(_hip.HipBackendError, match='log evidence'):
                ctx.log_evidence(np.array([5, t], dtype=np.int32))
        with pytest.raises(_hip.HipBackendError, match='log evidence'):
            ctx.log_evidence()
        _, _, st = ctx.estep_laplace()
        assert np.all(st == 0)
        e_all = rel_each(ctx.log_evidence(), ref)
        e_sum = abs(ctx.info('last_log_evidence_sum') - ref.sum()) / abs(ref.sum())
        print('engine %d, all %d trials in chunks of 6: log Z %.2e, sum %.2e' % (engine, R, e_all, e_sum))
        assert e_all <= TOL and e_sum <= TOL
        ctx.set_option('laplace_evidence', 0)
        ctx.estep_laplace(warm_start=True)
        assert ctx.info('last_log_evidence_sum') == 0.0
        for t in range(R):
            with pytest.raises(_hip.HipBackendError, match='log evidence'):
                ctx.log_evidence(np.array([t], dtype=np.int32))
    finally:
        ctx.close()


def test_what_supersedes_the_posterior_invalidates_the_evidence():
    """set_posterior, set_modes and new counts take the value of the trials they touch; the others keep theirs."""
    from funs import _hip
    ctx, ref = _context('c1', 2, options=(('laplace_evidence', 1),))
    try:
        ctx.estep_laplace()
        z = ctx.log_evidence()
        one, two = np.array([4], dtype=np.int32), np.array([7], dtype=np.int32)
        ctx.set_posterior(one, ctx.post_mean(one), ctx.post_vsm(one))
        ctx.set_modes(two, ctx.post_mean(two))
        for t in (4, 7):
            with pytest.raises(_hip.HipBackendError, match='no log evidence for trial %d' % t):
                ctx.log_evidence(np.array([t], dtype=np.int32))
        with pytest.raises(_hip.HipBackendError, match='no log evidence for trial 4'):       # (the first such trial of the list is named)
            ctx.log_evidence()
        keep = np.array([t for t in range(ref.size) if t not in (4, 7)], dtype=np.int32)
        assert np.array_equal(ctx.log_evidence(keep), z[keep])
        ctx.upload_counts(_padded_counts(_case('c1', False)[1], ctx.T))
        with pytest.raises(_hip.HipBackendError, match='no log evidence for trial 0'):
            ctx.log_evidence()
    finally:
        ctx.close()


# ---- 3. the option changes no other bit ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('engine', [1, 2], ids=['dense', 'lowrank'])
@pytest.mark.parametrize('name', ['c1', 'p10'])
def test_option_changes_no_other_bit(name, engine):
    """One context each way, same starts (cold, then warm): objective, post_mean, post_vsm, PautoSum and the factorisation counts are equal bit
    for bit; last_log_evidence_sum is 0 with the option off."""
    got = []
    for on in (0, 1):
        ctx, ref = _context(name, engine, options=(('laplace_evidence', on),))
        try:
            obj, it, st = ctx.estep_laplace()
            obj2, it2, st2 = ctx.estep_laplace(warm_start=True)
            assert np.all(st == 0) and np.all(st2 == 0)
            ctx.mstep_precomp()
            s = ctx.info('last_log_evidence_sum')
            assert (abs(s - ref.sum()) <= TOL * abs(ref.sum())) if on else (s == 0.0)
            got.append([np.array([obj, obj2]), ctx.post_mean(), ctx.post_vsm(), ctx.pautosum(), it, it2])
        finally:
            ctx.close()
    for a, b in zip(*got):
        assert np.array_equal(np.asarray(a), np.asarray(b))


# ---- 4. refused combination ---------------------------------------------------------------------------------------------------------------------
def test_evidence_with_laplace_f32_is_refused():
    from funs import _hip
    ctx, ref = _context('c1', 2)
    try:
        ctx.set_option('laplace_f32', 1)
        ctx.estep_laplace()
        assert ctx.info('last_cov_f32') == 1.0
        ctx.set_option('laplace_evidence', 1)
        with pytest.raises(_hip.HipBackendError, match='laplace_evidence.*laplace_f32'):
            ctx.estep_laplace()
        ctx.set_option('laplace_f32', 0)
        ctx.estep_laplace()
        assert rel_each(ctx.log_evidence(), ref) <= TOL
        with pytest.raises(_hip.HipBackendError, match='laplace_evidence is 0 or 1'):
            ctx.set_option('laplace_evidence', 2)
    finally:
        ctx.close()


# ---- 5. the fit object ---------------------------------------------------------------------------------------------------------------------------
def _c1_fit(funs_mod, **kw):
    from funs import _session
    _session.drop_sessions()
    g = load_golden('c1_dataset.npz')
    Ys = [g['Y'][r].astype(np.float64) for r in range(g['Y'].shape[0])]
    init = {'C': g['init_C'].copy(), 'd': g['init_d'].copy(), 'tau': g['init_tau'].copy()}
    args = dict(EMmode='Batch', maxEMiter=5, CdOptimMethod='newton', quiet=True)
    args.update(kw)
    return funs_mod.engine.PPGPFAfit(Experiment(Ys, BIN_MS), initParams=init, **args), Ys


def test_fit_tracks_the_evidence(funs_mod):
    """Config 1, Batch, CdOptimMethod='newton', 5 iterations with trackEvidence: logEvidence[i] is numpy's mean log Z at paramSeq[i] (1e-9);
    posteriorLikelihood and paramSeq are those of the same fit without the keyword, bit for bit; the module switch is restored."""
    plain, _ = _c1_fit(funs_mod)
    fit, Ys = _c1_fit(funs_mod, trackEvidence=True)
    assert funs_mod.inference.LAPLACE_EVIDENCE is False and not hasattr(plain, 'logEvidence')
    assert len(fit.logEvidence) == 5 and fit.emIterations == 5 and plain.emIterations == 5
    for i in range(5):
        want = numpy_log_evidence(Ys, fit.paramSeq[i]).mean()
        err = abs(fit.logEvidence[i] - want) / abs(want)
        print('EM iteration %d: mean log evidence %.6f, numpy %.6f, difference %.2e' % (i, fit.logEvidence[i], want, err))
        assert err <= TOL
    assert np.array_equal(np.asarray(fit.posteriorLikelihood), np.asarray(plain.posteriorLikelihood))
    assert len(fit.paramSeq) == len(plain.paramSeq) == 6
    for a, b in zip(fit.paramSeq, plain.paramSeq):
        assert all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in ('C', 'd', 'tau'))


def test_fit_stops_by_the_evidence(funs_mod):
    """emTol = 1.0 ends the fit as early as the rule allows, after iteration 1."""
    fit, _ = _c1_fit(funs_mod, emTol=1.0)
    print('emTol = 1.0: %d iterations, log evidence %s' % (fit.emIterations, fit.logEvidence))
    assert fit.emIterations == 2 and len(fit.posteriorLikelihood) == len(fit.logEvidence) == 2
    assert len(fit.paramSeq) == 3 and fit.tauSeq.shape == (3, 2) and fit.maxEMiter == 5
    assert fit.expectedSpikeCountsEst.shape == (30, 2) and len(fit.learningDetails) == 2
    # a tolerance nothing meets runs all iterations
    fit, _ = _c1_fit(funs_mod, emTol=1e-300, maxEMiter=3)
    assert fit.emIterations == 3 and len(fit.logEvidence) == 3
    with pytest.raises(ValueError, match='emTol'):
        _c1_fit(funs_mod, EMmode='Online', emTol=1e-3)
    with pytest.raises(ValueError, match='emTol'):
        _c1_fit(funs_mod, emTol=-1.0)


def test_variational_fit_stops_by_the_bound(funs_mod):
    from funs import _session
    _session.drop_sessions()
    g = load_golden('var_toy.npz')
    Ys = [g['Y'][r].astype(float) for r in range(g['Y'].shape[0])]
    init = {'C': g['init_C'].copy(), 'd': g['init_d'].copy(), 'tau': g['init_tau'].copy()}
    fit = funs_mod.engine.PPGPFAfit(Experiment(Ys, float(g['binSize'])), initParams=init, inferenceMethod='variational', EMmode='Batch', maxEMiter=5,
                                    quiet=True, emTol=1.0)
    print('variational, emTol = 1.0: %d iterations, bound %s' % (fit.emIterations, fit.variationalLowerBound))
    assert fit.emIterations == 2 and len(fit.variationalLowerBound) == 2 and len(fit.paramSeq) == 3 and fit.maxEMiter == 5
    assert not hasattr(fit, 'logEvidence')
    _session.drop_sessions()


# ---- 6. cross-validation by the evidence ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ragged', [False, True], ids=['equal', 'ragged'])
def test_cross_validation_by_the_evidence(funs_mod, ragged):
    """Config 1 data, 10 training and 4 test trials, xdim 1..3, two EM iterations: errs[i] = - sum log Z / sum T of numpy at fits[i].optimParams on
    the test trials (1e-9), optimXdim the arg-min.  With the test trials cut to unequal lengths too: the leave-one-out score refuses those."""
    from funs import _session
    _session.drop_sessions()
    g = load_golden('c1_dataset.npz')
    Ys = [g['Y'][r].astype(np.float64) for r in range(g['Y'].shape[0])]
    if ragged:
        lens = np.full(len(Ys), Ys[0].shape[1])
        lens[10:14] = [100, 50, 57, 83]
        Ys = cut(Ys, lens)
    exp = Experiment(Ys, BIN_MS)
    np.random.seed(2)
    cv = funs_mod.util.crossValidation(exp, numTrainingTrials=10, numTestTrials=4, maxXdim=3, maxEMiter=2, score='evidence')
    assert funs_mod.inference.LAPLACE_EVIDENCE is False and len(cv.errs) == 3
    test = Ys[10:14]
    bins = sum(y.shape[1] for y in test)
    for i, fit in enumerate(cv.fits):
        par = {k: np.real(np.asarray(v)).astype(np.float64) for k, v in fit.optimParams.items()}
        want = -numpy_log_evidence(test, par).sum() / bins
        err = abs(cv.errs[i] - want) / abs(want)
        print('%s test trials, xdim %d: score %.8f, numpy %.8f, difference %.2e' % ('ragged' if ragged else 'equal', i + 1, cv.errs[i], want, err))
        assert err <= TOL
    assert cv.optimXdim == int(np.argmin(cv.errs)) + 1
    if ragged:
        with pytest.raises(NotImplementedError, match='trials of unequal length'):
            funs_mod.util.crossValidation(exp, numTrainingTrials=10, numTestTrials=4, maxXdim=1, maxEMiter=1)
    with pytest.raises(ValueError, match='evidence'):
        funs_mod.util.crossValidation(exp, numTrainingTrials=10, numTestTrials=4, maxXdim=1, maxEMiter=1, inferenceMethod='variational', score='evidence')
    _session.drop_sessions()
