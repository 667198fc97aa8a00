"""Laplace EM over trials of unequal length (pad and mask: pgpfa_set_trial_lengths; DESIGN.md sections 3, 4 and 8).

A context keeps T = max_r T_r; bins t >= T_r of trial r carry no likelihood term, the GP prior spans all T bins.  A GP is consistent under
marginalisation, so the Laplace posterior over the first T_r bins of the padded problem IS the posterior of the T_r-bin problem and the
objective at the mode is the same number: the yardstick of every E-step check below is the oracle run on the TRUNCATED trials, one length
group at a time.  Ragged sets are made by cutting trials of equal-length data (a prefix of a GP sample is a sample of the shorter model);
lengths lie in T/2..T and always hold a full-length trial, one at T/2 and one that is no multiple of 16.

Tolerances are those of the equal-length path (test_gpu_mstep_dense.py): modes 1e-8, covariance blocks 1e-8 relative,
objective 1e-9 relative, PautoSum 1e-9, (C,d) cost 1e-10 / gradient and steps 1e-9, timescale gradient 1e-8 of the larger of its two terms.
Every test prints the figures it measured before it asserts."""
import numpy as np
import pytest

from conftest import Experiment, load_golden
from oracle import pgpfa_oracle as orc
import test_gpu_mstep_dense as dense

pytestmark = pytest.mark.gpu

BIN_MS = 10.0
INV_S2 = dense.INV_S2


# ---- ragged data ---------------------------------------------------------------------------------------------------------------------------
def ragged_lengths(R, T, seed, n_distinct=5):
    """R lengths out of n_distinct values in T/2..T: T, T/2, one that is no multiple of 16, the others drawn; trial 0 is full length"""
    rng = np.random.default_rng(seed)
    odd = T // 2 + 7 if (T // 2 + 7) % 16 else T // 2 + 9
    vals = [T, T // 2, odd]
    while len(vals) < n_distinct:
        v = int(rng.integers(T // 2, T + 1))
        if v not in vals:
            vals.append(v)
    lens = np.array([vals[i % len(vals)] for i in range(R)])
    lens[1:] = rng.permutation(lens[1:])
    assert lens[0] == T and T // 2 in lens and any(v % 16 for v in lens) and lens.min() >= T // 2
    return lens.astype(np.int32)


def cut(Ys, lens):
    return [np.ascontiguousarray(np.asarray(y, dtype=np.float64)[:, :L]) for y, L in zip(Ys, lens)]


def oracle_by_length(Ys, lens, params, return_cov=False):
    """orc.laplace(mode='exact') on the truncated trials of every distinct length -> per-trial lists in trial order, sum of the objectives"""
    R = len(Ys)
    out = {k: [None] * R for k in ('post_mean', 'post_vsm', 'post_vsmGP', 'post_cov')}
    total = 0.0
    for L in sorted(set(int(v) for v in lens)):
        idx = [r for r in range(R) if lens[r] == L]
        res, nll, _ = orc.laplace([Ys[r] for r in idx], params, BIN_MS, mode='exact', return_cov=return_cov)
        total += -nll * len(idx)
        for j, r in enumerate(idx):
            for k in out:
                if k in res:
                    out[k][r] = res[k][j]
    return out, total


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


@pytest.fixture(scope='module')
def funs_mod():
    import funs
    return funs


@pytest.fixture()
def cov_mode(funs_mod, request):
    from funs import _session
    old = funs_mod.inference.COV_MODE
    _session.drop_sessions()
    funs_mod.inference.COV_MODE = request.param
    yield request.param
    funs_mod.inference.COV_MODE = old
    _session.drop_sessions()


def _estep_problem(name):
    """(params, equal-length trials, T): config 1 (p = 3), or small synthetic sets; p = 10 has T > 128, so that poisson_mfma_kernel<10, 2> runs
    with whole workgroups, waves and single tiles past a trial's length; p = 12 the one-tile matrix-core form; p = 20 the GEMM form (rates_wide_kernel)"""
    if name == 'c1':
        g = load_golden('c1_dataset.npz')
        Ys = [g['Y'][r].astype(np.float64) for r in range(g['Y'].shape[0])]
        return {'C': g['init_C'].copy(), 'd': g['init_d'].copy(), 'tau': g['init_tau'].copy()}, Ys, Ys[0].shape[1]
    q, p, T, R = {'p10': (40, 10, 176, 6), 'p12': (35, 12, 64, 6), 'p20': (50, 20, 48, 6)}[name]
    params, Ys, _ = orc.synth_dataset(q, p, T, R, seed=31 + p)
    return params, Ys, T


ESTEP_CASES = ['c1', 'p10', 'p12', 'p20']
_oracle_cache = {}


def _estep_case(name):
    if name not in _oracle_cache:
        params, Ys, T = _estep_problem(name)
        lens = ragged_lengths(len(Ys), T, seed=len(name) + T, n_distinct=5 if name == 'c1' else 4)
        Yr = cut(Ys, lens)
        ref, total = oracle_by_length(Yr, lens, params, return_cov=(name == 'c1'))
        _oracle_cache[name] = (params, Yr, lens, T, ref, total)
    return _oracle_cache[name]


# ---- 1. E-step against the oracle, per length ----------------------------------------------------------------------------------------------
@pytest.mark.timeout(900)
@pytest.mark.parametrize('cov_mode', [1, 2], indirect=True, ids=['dense', 'lowrank'])
@pytest.mark.parametrize('name', ESTEP_CASES)
def test_estep_against_the_oracle_per_length(funs_mod, name, cov_mode):
    """inference.laplace on a ragged experiment, cold, warm from the resident modes and warm from host copies of lapOptimRes (xdim * T_r values
    each), under both covariance engines: post_mean (p, T_r) 1e-8, post_vsm (T_r, p, p) and post_vsmGP (T_r, T_r, p) 1e-8 relative, nPLL 1e-9
    relative against orc.laplace(mode='exact') on the truncated trials of each length; config 1 also post_cov (p T_r x p T_r) 1e-8 relative."""
    params, Yr, lens, T, ref, total = _estep_case(name)
    R, p = len(Yr), params['C'].shape[1]
    exp = Experiment(Yr, BIN_MS)
    nll_ref = -total / R
    optim = None
    host_copy = None
    for start in ('cold', 'resident', 'host'):
        prev = {'cold': None, 'resident': optim, 'host': host_copy}[start]
        infRes, nll, optim = funs_mod.inference.laplace(exp, {k: v.copy() for k, v in params.items()}, prevOptimRes=prev)
        sess = infRes.session
        if start == 'resident':
            infRes.materialize(('post_mean', 'post_vsm', 'post_vsmGP'))       # (the bulk download hands out the same cut entries)
        assert sess.T == T and sess.ctx.info('trial_lengths_set') == 1.0 and np.all(infRes.newton_status == 0)
        e_m = e_v = e_g = 0.0
        for r in range(R):
            L = int(lens[r])
            m, v, gp = infRes['post_mean'][r], infRes['post_vsm'][r], infRes['post_vsmGP'][r]
            assert m.shape == (p, L) and v.shape == (L, p, p) and gp.shape == (L, L, p) and optim[r].shape == (p * L,)
            assert np.array_equal(optim[r], m.reshape(-1))
            e_m = max(e_m, float(np.max(np.abs(m - ref['post_mean'][r]))))
            e_v = max(e_v, rel(v, ref['post_vsm'][r]))
            e_g = max(e_g, rel(gp, ref['post_vsmGP'][r]))
        e_f = abs(nll - nll_ref) / abs(nll_ref)
        print('%s, engine %d, %s start: modes %.2e, post_vsm %.2e, post_vsmGP %.2e, nPLL %.2e (lengths %s)'
              % (name, cov_mode, start, e_m, e_v, e_g, e_f, sorted(set(lens.tolist()))))
        assert e_m <= 1e-8 and e_v <= 1e-8 and e_g <= 1e-8 and e_f <= 1e-9
        if start == 'cold':
            host_copy = [np.array(optim[r]) for r in range(R)]
            if name == 'c1':
                r = int(np.argmin(lens))
                cov = infRes['post_cov'][r]
                assert cov.shape == (p * lens[r], p * lens[r])
                e_c = rel(cov, ref['post_cov'][r])
                print('%s, engine %d: post_cov of trial %d (%d bins) %.2e' % (name, cov_mode, r, lens[r], e_c))
                assert e_c <= 1e-8


@pytest.mark.parametrize('name', ['p20'])
def test_vector_poisson_pass_against_the_oracle(name):
    """poisson_pass_kernel (the vector form, which option dual_gemm = 0 selects at 20 latents) on the ragged set of the test above, at the
    C-ABI: modes 1e-8 and objective 1e-9 relative against the oracle per length, cold and warm."""
    from funs import _hip
    params, Yr, lens, T, ref, total = _estep_case(name)
    R, q, p = len(Yr), Yr[0].shape[0], params['C'].shape[1]
    Y = np.zeros((R, q, T), dtype=np.uint8)
    for r, y in enumerate(Yr):
        Y[r, :, :y.shape[1]] = y
    ctx = _hip.Context(q, p, T, R, BIN_MS)
    try:
        ctx.upload_counts(Y)
        ctx.set_option('dual_gemm', 0)
        ctx.set_params(params['C'], params['d'], params['tau'])
        ctx.set_trial_lengths(lens)
        for warm in (False, True):
            obj, _, st = ctx.estep_laplace(warm_start=warm)
            assert np.all(st == 0)
            M = ctx.post_mean()
            e_m = max(float(np.max(np.abs(M[r, :, :lens[r]] - ref['post_mean'][r]))) for r in range(R))
            e_f = abs(obj - total) / abs(total)
            print('%s, vector Poisson pass, %s: modes %.2e, objective %.2e' % (name, 'warm' if warm else 'cold', e_m, e_f))
            assert e_m <= 1e-8 and e_f <= 1e-9
    finally:
        ctx.close()


# ---- 2. PautoSum against a dense inverse ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cov_mode', [1, 2], indirect=True, ids=['dense', 'lowrank'])
def test_pautosum_against_a_dense_inverse(funs_mod, cov_mode):
    """The whole padded PautoSum of ragged config 1, 1e-9 relative: per trial numpy inverts blockdiag(K_T^-1) + W_t [t < T_r] at the device's
    mode (all T bins: the padded ones hold the prior conditional) and sums Sigma_kk + m m^T over the trials."""
    params, Yr, lens, T, _, _ = _estep_case('c1')
    R, p = len(Yr), params['C'].shape[1]
    exp = Experiment(Yr, BIN_MS)
    infRes, _, _ = funs_mod.inference.laplace(exp, {k: v.copy() for k, v in params.items()})
    ctx = infRes.session.ctx
    assert ctx.mstep_precomp() == float(R)
    P = ctx.pautosum()
    M = ctx.post_mean(np.arange(R, dtype=np.int32))                  # padded (R, p, T)
    Kinv = np.linalg.inv(orc.make_K(params['tau'], T, BIN_MS))
    C, d = params['C'], params['d'].reshape(-1)
    P_ref = np.zeros((p, T, T))
    ar = np.arange(T)
    for r in range(R):
        W = orc.poisson_blocks(M[r], C, d) * (ar < lens[r])[:, None, None]
        H = np.zeros((p, T, p, T))
        for k in range(p):
            H[k, :, k, :] += Kinv[k]
            for l in range(p):
                H[k, ar, l, ar] += W[:, k, l]
        S = np.linalg.inv(H.reshape(p * T, p * T))
        for k in range(p):
            P_ref[k] += S[k * T:(k + 1) * T, k * T:(k + 1) * T] + np.outer(M[r, k], M[r, k])
    e = rel(P, P_ref)
    print('PautoSum of ragged config 1, engine %d: %.2e' % (cov_mode, e))
    assert e <= 1e-9


# ---- 3. (C,d) passes by value ----------------------------------------------------------------------------------------------------------------
CD_CASES = {
    'items':  (200, 10, 500, 64),     # 512 / 1024 (trial, bin tile) items on 256 / 128 workgroups: the stride loop, the prefetch of a following item
    'p10':    (60, 10, 150, 12),
    'p12':    (60, 12, 150, 12),      # vector sweep, mstep_cd_hess_kernel
    'p20':    (70, 20, 100, 12),      # mstep_cd_hess_rows_kernel, 4 row groups
}
CD_RUNS = [('items', 'default'), ('p10', 'default'), ('p10', 'vector'), ('p12', 'default'), ('p20', 'default')]


def _ragged_sums(vec, pr, lens, want_hess=True):
    out = None
    for r, L in enumerate(lens):
        s = dense._cd_sums(vec, pr['M'][r:r + 1, :, :L], pr['V'][r:r + 1, :L], pr['Y'][r:r + 1, :, :L], want_hess=want_hess)
        out = list(s) if out is None else [a + b for a, b in zip(out, s)]
    return tuple(out)


@pytest.mark.timeout(900)
@pytest.mark.parametrize('prior', [False, True], ids=['plain', 'prior'])
@pytest.mark.parametrize('name,form', CD_RUNS, ids=['%s-%s' % r for r in CD_RUNS])
def test_cd_passes_on_ragged_posteriors(name, form, prior):
    """A ragged synthetic posterior through pgpfa_set_posterior (padded arrays whose padded bins hold NaN: whatever read them would show), the
    counts zero-padded.  costgrad against orc.mstep_cd_cost / _grad (and the _prior forms) on the ragged lists: cost 1e-10, gradient 1e-9; every
    entry point (costgrad, Newton pass, chord pass, per-neuron cost) against plain FP64 numpy over the bins t < T_r, as test_gpu_mstep_dense.py
    does for equal trials: steps and decrements 1e-9.  form 'vector': options cd_mfma = cd_hess_mfma = 0."""
    q, p, T, R = CD_CASES[name]
    pr = dense._cd_problem(q, p, T, R, seed=77 + 3 * q + T)
    lens = ragged_lengths(R, T, seed=R + T, n_distinct=6)
    center = pr['center'] if prior else None
    Y = pr['Y'].copy()
    M, V = pr['M'].copy(), pr['V'].copy()
    for r, L in enumerate(lens):
        Y[r, :, L:] = 0
        M[r, :, L:] = np.nan
        V[r, L:] = np.nan
    s0 = _ragged_sums(pr['v0'], pr, lens)
    v1 = pr['v0'] + 0.3 * dense._step(*dense._with_prior(pr['v0'], s0, R, None)[2:])[0].T.reshape(-1)
    s1 = _ragged_sums(v1, pr, lens, want_hess=False)
    ref0, ref1 = dense._with_prior(pr['v0'], s0, R, center), dense._with_prior(v1, s1, R, center)
    tag = 'ragged %s %s %s%s' % (name, (q, p, T, R), form, ' with prior' if prior else '')
    from funs import _hip
    ctx = _hip.Context(q, p, T, R, BIN_MS)
    try:
        ctx.upload_counts(Y if Y.max() > 255 else Y.astype(np.uint8))
        for key in (('cd_mfma', 'cd_hess_mfma') if form == 'vector' else ()):
            ctx.set_option(key, 0)
        ctx.set_params(pr['C'], pr['d'], pr['tau_s'])
        ctx.set_trial_lengths(lens)
        ctx.set_posterior(None, M, V)
        dense._compare_entry_points(tag, ctx, pr['v0'], v1, center, ref0, ref1)
        # the oracle on the ragged lists
        Ys = [Y[r, :, :L].astype(np.float64) for r, L in enumerate(lens)]
        pm = [pr['M'][r, :, :L] for r, L in enumerate(lens)]
        pv = [pr['V'][r, :L] for r, L in enumerate(lens)]
        kw = {} if center is None else {'prior_center': center, 'inv_s2': INV_S2}
        cost, grad = ctx.mstep_cd_costgrad(pr['v0'], **kw)
        if prior:
            inv_prior = -INV_S2 * np.eye(q * (p + 1))
            c_ref = orc.mstep_cd_cost_prior(pr['v0'], center, inv_prior, Ys, pm, pv, p, q)
            g_ref = orc.mstep_cd_grad_prior(pr['v0'], center, inv_prior, Ys, pm, pv, p, q)
        else:
            c_ref = orc.mstep_cd_cost(pr['v0'], Ys, pm, pv, p, q)
            g_ref = orc.mstep_cd_grad(pr['v0'], Ys, pm, pv, p, q)
        e_c = abs(cost - c_ref) / ref0[1].sum()
        e_g = dense._rows(grad, g_ref.reshape(p + 1, q).T)
        print('%s: against the oracle on the ragged lists: cost %.2e, gradient %.2e' % (tag, e_c, e_g))
        assert e_c <= 1e-10 and e_g <= 1e-9
    finally:
        ctx.close()


# ---- 4. timescale identity -------------------------------------------------------------------------------------------------------------------
def test_timescale_gradient_is_that_of_the_per_length_cost(funs_mod):
    """At the parameters of the E-step the gradient of the padded timescale cost (pgpfa_mstep_tau_costgrad on the T x T PautoSum) equals
    sum_L orc.tau_grad(pv, P_L, R_L) with P_L from the oracle's truncated posteriors (Fisher identity): 1e-8 of the larger of the gradient's
    two terms."""
    from funs import _session
    _session.drop_sessions()
    params, Yr, lens, T, ref, _ = _estep_case('c1')
    R, p = len(Yr), params['C'].shape[1]
    exp = Experiment(Yr, BIN_MS)
    infRes, _, _ = funs_mod.inference.laplace(exp, {k: v.copy() for k, v in params.items()})
    ctx = infRes.session.ctx
    ctx.mstep_precomp()
    logp = np.log(1.0 / (params['tau'] * 1000.0 / BIN_MS) ** 2)
    worst = 0.0
    for k in range(p):
        g_dev = ctx.mstep_tau_costgrad(k, logp[k])[1]
        g_ref, a_sum, b_sum = 0.0, 0.0, 0.0
        for L in sorted(set(lens.tolist())):
            idx = [r for r in range(R) if lens[r] == L]
            P_L, n_L = orc.make_precomp({'post_mean': [ref['post_mean'][r] for r in idx], 'post_vsmGP': [ref['post_vsmGP'][r] for r in idx]})
            g_ref += orc.tau_grad(logp[k], P_L[k], n_L)[0]
            K, dK = orc._tau_pieces(logp[k], L, orc.EPS_NOISE)
            Ki = np.linalg.inv(K)
            KiM = Ki @ dK
            a_sum += -0.5 * n_L * np.trace(KiM) * np.exp(logp[k])
            b_sum += 0.5 * np.sum((KiM @ Ki) * P_L[k].T) * np.exp(logp[k])
        err = abs(g_dev - g_ref) / max(abs(a_sum), abs(b_sum))
        print('latent %d: padded gradient %.6e, per-length gradient %.6e, difference %.2e of the larger term' % (k, g_dev, g_ref, err))
        worst = max(worst, err)
    assert worst <= 1e-8
    _session.drop_sessions()


# ---- 5. EM end to end on ragged config 1 -----------------------------------------------------------------------------------------------------
def _stationarity(par, Yr, pm):
    """max |gradient of the T_r-bin log-posterior| over the trials at the cut modes"""
    worst = 0.0
    kinv = {}
    for Y, X in zip(Yr, pm):
        L = Y.shape[1]
        if L not in kinv:
            kinv[L] = np.linalg.inv(orc.make_K(par['tau'], L, BIN_MS))
        worst = max(worst, float(np.max(np.abs(orc.nlp_grad(X, Y, par['C'], par['d'].reshape(-1), kinv[L])))))
    return worst


@pytest.mark.timeout(900)
def test_batch_em_on_ragged_config1(funs_mod):
    """Three batch-EM iterations (CdOptimMethod='newton') from initializeParams, which equals orc.initialize_params on the ragged trials to 1e-10
    (loading columns up to the sign LAPACK leaves open): every mode is stationary for the truncated
    problem (<= 1e-6), the new (C,d) zero the oracle's gradient on the ragged lists (2e-6, as the bench-workload test), the new timescales zero
    orc.tau_grad on the padded PautoSum (1e-6 R)."""
    from funs import _session
    _session.drop_sessions()
    _, Yr, lens, T, _, _ = _estep_case('c1')
    R, q, p = len(Yr), Yr[0].shape[0], 3
    exp = Experiment(Yr, BIN_MS)
    np.random.seed(5)
    init = funs_mod.util.initializeParams(p, q, exp)
    ref_init = orc.initialize_params(Yr, p, seed=5)
    # (a column of C is an eigenvector from LAPACK's dgeev, whose sign the routine leaves open: the device's exact integer moments and np.cov
    # differ in the last bits - 2e-15 of the covariance here - and that flips the third column.  Columns are compared up to that sign.)
    Cd, Cr = np.real(init['C']), np.real(ref_init['C'])
    sign = np.sign(np.sum(Cd * Cr, axis=0))
    errs = {'C': float(np.max(np.abs(Cd * sign - Cr))), 'd': float(np.max(np.abs(init['d'] - ref_init['d']))),
            'tau': float(np.max(np.abs(init['tau'] - ref_init['tau'])))}
    print('initializeParams against the oracle on the ragged trials: %s (column signs %s)' % (errs, sign.tolist()))
    assert np.all(np.abs(sign) == 1.0) and max(errs.values()) <= 1e-10
    params = {k: np.real(np.asarray(v)).astype(np.float64) for k, v in init.items()}
    optim = None
    for it in range(3):
        infRes, nll, optim = funs_mod.inference.laplace(exp, params, prevOptimRes=optim)
        assert np.all(infRes.newton_status == 0)
        pm = [np.array(infRes['post_mean'][r]) for r in range(R)]
        pv = [np.array(infRes['post_vsm'][r]) for r in range(R)]
        new, _ = funs_mod.learning.updateParams(params, infRes, exp, CdOptimMethod='newton')
        P = infRes.session.ctx.pautosum()
        worst = _stationarity(params, Yr, pm)
        g_cd = float(np.max(np.abs(orc.mstep_cd_grad(orc.cd_to_vec(new['C'], new['d']), Yr, pm, pv, p, q))))
        logp = np.log(1.0 / (new['tau'] * 1000.0 / BIN_MS) ** 2)
        g_tau = max(abs(orc.tau_grad(logp[k], P[k], R)[0]) for k in range(p))
        print('batch EM iteration %d: nPLL %.6f, worst |grad| of a mode %.2e, |(C,d) gradient| %.2e, |timescale gradient| %.2e' % (it, nll, worst, g_cd, g_tau))
        assert worst <= 1e-6 and g_cd <= 2e-6 and g_tau <= 1e-6 * R
        params = new
    _session.drop_sessions()


@pytest.mark.timeout(900)
def test_online_diag_em_on_ragged_config1(funs_mod):
    """Three stochastic-EM iterations with the 'diag' prior (minibatches of 6 reuse the parent's resident counts and length table): the
    minibatch index stream is the reference's (np.random.choice on the global stream), every mode of the minibatch is stationary for its
    truncated trial (1e-6), the new (C,d) zero the oracle's regularised gradient on the ragged minibatch (2e-6) and the new timescales the
    reference's regularised timescale gradient on the padded PautoSum (1e-6 batch)."""
    from funs import _session
    _session.drop_sessions()
    g = load_golden('c1_dataset.npz')
    _, Yr, lens, T, _, _ = _estep_case('c1')
    R, q, p, batch = len(Yr), Yr[0].shape[0], 3, 6
    exp = Experiment(Yr, BIN_MS)
    params = {'C': g['init_C'].copy(), 'd': g['init_d'].copy(), 'tau': g['init_tau'].copy()}
    np.random.seed(11)
    state = np.random.get_state()
    prior = np.diag(np.ones(q * (p + 1)))
    for n in range(3):
        sz = 1.0 / (n + 1) ** 0.75
        np.random.set_state(state)
        idx_ref = orc.subsample_trials(R, batch)
        np.random.set_state(state)
        sub = funs_mod.util.subsampleTrials(exp, batch)
        state = np.random.get_state()
        assert np.array_equal(sub.batchTrIdx, idx_ref)
        infRes, nll, _ = funs_mod.inference.laplace(sub, params, prevOptimRes='resident')
        assert infRes.session is _session.session_for(exp, p)[0]
        Yb = [Yr[i] for i in idx_ref]
        pm = [np.array(infRes['post_mean'][j]) for j in range(batch)]
        pv = [np.array(infRes['post_vsm'][j]) for j in range(batch)]
        assert all(pm[j].shape == (p, lens[i]) for j, i in enumerate(idx_ref))
        new, _, prior = funs_mod.learning.updateParamsWithPrior(params, infRes, sub, 'newton', 'lockstep', sz, sz, prior, covOpts='useDiag')
        P = infRes.session.ctx.pautosum()
        worst = _stationarity(params, Yb, pm)
        old_vec = orc.cd_to_vec(params['C'], params['d'])
        g_cd = float(np.max(np.abs(orc.mstep_cd_grad_prior(orc.cd_to_vec(new['C'], new['d']), old_vec, prior, Yb, pm, pv, p, q))))
        logp = np.log(1.0 / (new['tau'] * 1000.0 / BIN_MS) ** 2)
        g_tau = max(abs(orc.tau_grad_prior(logp[k], P[k], batch, BIN_MS, params['tau'][k], sz)[0]) for k in range(p))
        print('online EM iteration %d (trials %s): worst |grad| of a mode %.2e, |(C,d) gradient| %.2e, |timescale gradient| %.2e'
              % (n, idx_ref.tolist(), worst, g_cd, g_tau))
        assert worst <= 1e-6 and g_cd <= 2e-6 and g_tau <= 1e-6 * batch
        params = new
    _session.drop_sessions()


def test_fit_object_on_a_ragged_experiment(funs_mod):
    """engine.PPGPFAfit in Batch and in Online mode with every update method: T is the longest trial, the expected spike counts are taken over
    the mean trial length, countMoments counts sum_r T_r samples, x_tilde is a list of (xdim, T_r) arrays."""
    from funs import _session
    _session.drop_sessions()
    g = load_golden('c1_dataset.npz')
    _, Yr, lens, T, _, _ = _estep_case('c1')
    exp = Experiment(Yr, BIN_MS)
    init = {'C': g['init_C'].copy(), 'd': g['init_d'].copy(), 'tau': g['init_tau'].copy()}
    mean, cov, totals, ns = funs_mod.util.countMoments(exp, 3)
    raster = np.concatenate(Yr, axis=1)
    assert ns == int(lens.sum()) and np.array_equal(totals, raster.sum(axis=1))
    assert np.allclose(mean, raster.mean(axis=1), rtol=1e-13, atol=0) and np.allclose(cov, np.cov(raster), rtol=1e-10, atol=1e-14)
    fit = funs_mod.engine.PPGPFAfit(exp, initParams={k: v.copy() for k, v in init.items()}, EMmode='Batch', maxEMiter=2, CdOptimMethod='newton', quiet=True)
    assert fit.T == T and fit.meanT == float(np.mean(lens)) and np.all(np.isfinite(fit.posteriorLikelihood))
    C = fit.paramSeq[0]['C']
    assert np.allclose(fit.expectedSpikeCountsEst[:, 0], np.mean(lens) * np.exp(0.5 * np.sum(C * C, axis=1) + fit.paramSeq[0]['d']), rtol=1e-13)
    fit.extractTrajectories()
    fit.orthonormalizeTrajectories()
    assert isinstance(fit.x_tilde, list) and [x.shape for x in fit.x_tilde] == [(3, int(L)) for L in lens]
    for method in ('diag', 'hess', 'grad', 'balancingGamma', 'sequentialAverage', 'fullyUpdateAll'):
        np.random.seed(3)
        fit = funs_mod.engine.PPGPFAfit(exp, initParams={k: v.copy() for k, v in init.items()}, EMmode='Online', maxEMiter=2, batchSize=5,
                                        onlineParamUpdateMethod=method, quiet=True)
        assert np.all(np.isfinite(fit.posteriorLikelihood)) and all(np.all(np.isfinite(fit.optimParams[k])) for k in ('C', 'd', 'tau')), method
    _session.drop_sessions()


# ---- 6. no change for equal trials -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('q,p,T,R', [(30, 3, 100, 8), (40, 10, 176, 4), (50, 20, 48, 4)], ids=['p3', 'p10', 'p20'])
def test_all_lengths_equal_to_T_changes_no_bit(q, p, T, R):
    """pgpfa_set_trial_lengths with every length T against no call: bit-identical objective, modes, blocks, PautoSum and (C,d) sums (cost,
    gradient, Newton step)."""
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
                ctx.set_trial_lengths(np.full(R, T))
            assert ctx.info('trial_lengths_set') == float(with_table)
            obj, _, st = ctx.estep_laplace()
            obj2, _, st2 = ctx.estep_laplace(warm_start=True)
            assert np.all(st == 0) and np.all(st2 == 0)
            ctx.mstep_precomp()
            v0 = orc.cd_to_vec(params['C'], params['d'])
            got.append([np.array([obj, obj2]), ctx.post_mean(), ctx.post_vsm(), ctx.post_vsmgp(), ctx.pautosum(), *ctx.mstep_cd_costgrad(v0),
                        *ctx.mstep_cd_newton_pass(v0), np.array(ctx.count_moments()[2])])
        finally:
            ctx.close()
    for a, b in zip(*got):
        assert np.array_equal(np.asarray(a), np.asarray(b))


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_entry_points_that_do_not_know_the_lengths_refuse(funs_mod):
    from funs import _hip, _session
    _session.drop_sessions()
    params, Yr, lens, T, _, _ = _estep_case('c1')
    R, q, p = len(Yr), Yr[0].shape[0], 3
    exp = Experiment(Yr, BIN_MS)
    par = lambda: {k: v.copy() for k, v in params.items()}
    for call in (lambda: funs_mod.inference.dualVariational(exp, par()), lambda: funs_mod.util.leaveOneOutPrediction(par(), exp),
                 lambda: funs_mod.mcmc.PosteriorMCMC(exp, par(), 2, 0), lambda: funs_mod.mcmc.PosteriorMCMC_batch(exp, par(), 2, [0, 1], [1, 2])):
        with pytest.raises(NotImplementedError, match='trials of unequal length'):
            call()
    _session.drop_sessions()
    Y = np.zeros((R, q, T), dtype=np.uint8)
    for r, y in enumerate(Yr):
        Y[r, :, :y.shape[1]] = y
    ctx = _hip.Context(q, p, T, R, BIN_MS)
    try:
        ctx.upload_counts(Y)
        ctx.set_params(params['C'], params['d'], params['tau'])
        for bad in (0, T + 1):
            ln = lens.copy()
            ln[3] = bad
            with pytest.raises(_hip.HipBackendError, match='trial 3: length'):
                ctx.set_trial_lengths(ln)
        short = int(np.argmin(lens))
        Yb = Y.copy()
        Yb[short, 5, lens[short]] = 2                                  # the first padded bin of the shortest trial
        ctx.upload_counts(Yb)
        with pytest.raises(_hip.HipBackendError, match='trial %d: 1 non-zero counts at padded bins' % short):
            ctx.set_trial_lengths(lens)
        assert ctx.info('trial_lengths_set') == 0.0
        ctx.upload_counts(Y)
        ctx.set_trial_lengths(lens)
        assert ctx.info('trial_lengths_set') == 1.0
        lam = np.full((1, q * T), 0.5)
        idx = np.zeros(1, dtype=np.int32)
        for call in (lambda: ctx.dual_costgrad(0, lam[0]), lambda: ctx.dual_costgrad_batch(idx, lam), lambda: ctx.dual_lbfgs(idx, np.log(lam)),
                     lambda: ctx.dual_fixed_point(idx), lambda: ctx.dual_finalize(idx, lam), lambda: ctx.dual_post_mean(0, lam[0]),
                     lambda: ctx.dual_post_cov(0, lam[0]), lambda: ctx.loo_predict(idx), lambda: ctx.generate(1)):
            with pytest.raises(_hip.HipBackendError, match='trials of unequal length'):
                call()
        # uploading counts again drops the table; NULL drops it too
        ctx.set_trial_lengths(None)
        assert ctx.info('trial_lengths_set') == 0.0
        ctx.set_trial_lengths(lens)
        ctx.upload_counts(Y)
        assert ctx.info('trial_lengths_set') == 0.0
    finally:
        ctx.close()
