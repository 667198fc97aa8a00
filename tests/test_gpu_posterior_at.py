"""The latent posterior at arbitrary time points (pgpfa_posterior_at, Context.posterior_at, util.posteriorAt):

    kx_k(s)[j] = (1 - eps) exp(-1/2 (s - j bin)^2 / (1000 tau_k)^2) + eps [s == j bin],   a_k(s) = K_k^-1 kx_k(s)
    mean_k(s)  = a_k(s) . m_k,   var_k(s) = 1 - a_k(s) . kx_k(s) + a_k(s)^T V_k a_k(s)

8 trials at six shapes, both covariance engines and the sum-only plan of the low-rank one (blocks rebuilt on demand), S in {1, 15, 16, 17, 64, 65, 257}.
Tolerances: 1e-9 against the same formulas in numpy on the downloaded post_mean / post_vsmGP (mean relative to max|m|, var absolute - the prior
variance is 1): rounding amplified by cond(K) <= T / eps gives about 1e-10, and the restatement's own two evaluation orders (np.linalg.solve
against an explicit inverse) differ by 2.4e-11 (mean) / 8.8e-13 (var) at these shapes, ten times which stays below 1e-9.  1e-8 against
independent dense FP64 models (the project's tolerance for modes and blocks against dense FP64, docs/history/observed_bins.md).  1e-12 in the far
field.  Every test prints its figures before it asserts."""
import numpy as np
import pytest

from conftest import Experiment, load_golden
from oracle import pgpfa_oracle as orc
from test_cpu_posterior_samples import problem

pytestmark = pytest.mark.gpu

BIN_MS = 10.0
EPS = orc.EPS_NOISE
R8 = 8
SHAPES = [(30, 3, 100), (40, 10, 176), (35, 12, 64), (50, 20, 48), (20, 1, 21), (40, 32, 24)]
IDS = ['q%d-p%d-T%d' % s for s in SHAPES]
CONFIGS = [(1, 1), (2, 1), (2, 0)]                       # (cov_mode, keep_trial_vsmgp)
CONFIG_IDS = ['dense', 'lowrank', 'lowrank-sumonly']
S_VALUES = (1, 15, 16, 17, 64, 65, 257)
TOL_SAME, TOL_DENSE, TOL_FAR = 1e-9, 1e-8, 1e-12


# ---- the yardstick -------------------------------------------------------------------------------------------------------------------------------
def cross(tau_k, s, L):
    """kx (L, S) of one latent between the grid times j bin, j < L, and the query times s"""
    tg = np.arange(L, dtype=np.float64) * BIN_MS
    dt = s[None, :] - tg[:, None]
    return (1.0 - EPS) * np.exp(-0.5 * ((dt * dt) / (tau_k * 1000.0) ** 2)) + EPS * (s[None, :] == tg[:, None])


def numpy_at(tau, m, V, s):
    """mean, var (p, S) by the formulas above from m (p, L) and the blocks V (L, L, p), through np.linalg.solve"""
    p, L = m.shape
    K = orc.make_K(tau, L, BIN_MS)
    mean, var = np.empty((p, s.size)), np.empty((p, s.size))
    for k in range(p):
        kx = cross(tau[k], s, L)
        a = np.linalg.solve(K[k], kx)
        mean[k] = a.T @ m[k]
        var[k] = np.maximum(1.0 - (a * kx).sum(axis=0) + (a * (V[:, :, k] @ a)).sum(axis=0), 0.0)
    return mean, var


def make_times(T, S, tau, seed):
    """One grid of S query times: seeded uniform draws over [-2 bin, (T + 1) bin], the grid times {0, 15, 16, T - 1} bin exactly, one time
    50 max(tau) beyond each end and one duplicated time, shuffled.  (S = 1 holds one time only: a uniform draw.)  Returns the times and the positions
    of the two distant ones."""
    rng = np.random.default_rng(1000 * T + S + seed)
    if S < 8:
        return rng.uniform(-2 * BIN_MS, (T + 1) * BIN_MS, S), np.zeros(0, dtype=np.int64)
    far = 50.0 * 1000.0 * float(np.max(tau))
    draws = rng.uniform(-2 * BIN_MS, (T + 1) * BIN_MS, S - 7)
    t = np.concatenate([np.array([0.0, 15.0, 16.0, T - 1.0]) * BIN_MS, [-far, (T - 1) * BIN_MS + far], draws[:1], draws])
    order = rng.permutation(S)
    t = t[order]
    return np.ascontiguousarray(t), np.flatnonzero(np.isin(order, (4, 5)))


def make_ctx(shape, config, lens=None, observed=None, bins=None, evidence=False, R=R8, seed=0):
    """context of the R-trial problem after one Laplace E-step"""
    from funs import _hip
    q, p, T = shape
    par, Y, _ = problem(shape, seed=seed, R=R)
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
    ctx.set_option('cov_mode', config[0])
    ctx.set_option('keep_trial_vsmgp', config[1])
    if evidence:
        ctx.set_option('laplace_evidence', 1)
    ctx.set_params(par['C'], par['d'], par['tau'])
    if lens is not None:
        ctx.set_trial_lengths(np.asarray(lens, dtype=np.int32))
    if observed is not None:
        ctx.set_observed(observed)
    if bins is not None:
        ctx.set_observed_bins(bins)
    _, _, status = ctx.estep_laplace()
    assert np.all(status == 0), status
    if lens is None and observed is None and bins is None:        # (under a table the plan is the library's choice)
        assert ctx.info('plan_lowrank') == float(config[0] == 2)
    return ctx, par, Y, live


def errors(got, ref_mean, ref_var, scale):
    return float(np.max(np.abs(got['mean'] - ref_mean)) / scale), float(np.max(np.abs(got['var'] - ref_var)))


# ---- 1, 3, 4. same inputs in plain FP64; the grid identity; the far field ---------------------------------------------------------------------------
@pytest.mark.parametrize('config', CONFIGS, ids=CONFIG_IDS)
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_same_inputs_in_plain_fp64_the_grid_identity_and_the_far_field(shape, config):
    q, p, T = shape
    ctx, par, _, _ = make_ctx(shape, config)
    try:
        m, V = ctx.post_mean().reshape(R8, p, T), ctx.post_vsmgp()
        scale = float(np.max(np.abs(m)))
        for S in S_VALUES:
            s, far = make_times(T, S, par['tau'], 0)
            got = ctx.posterior_at(s)
            assert got['mean'].shape == (R8, p, S) and got['var'].shape == (R8, p, S)
            ref = [numpy_at(par['tau'], m[r], V[r], s) for r in range(R8)]
            e_m, e_v = errors(got, np.stack([a for a, _ in ref]), np.stack([b for _, b in ref]), scale)
            e_far = max(float(np.max(np.abs(got['mean'][:, :, far]), initial=0.0)), float(np.max(np.abs(got['var'][:, :, far] - 1.0), initial=0.0)))
            print('q=%d p=%d T=%d %s S=%d: mean %.2e of max|m|, var %.2e (limit %.0e); far field %.2e (limit %.0e)'
                  % (q, p, T, CONFIG_IDS[CONFIGS.index(config)], S, e_m, e_v, TOL_SAME, e_far, TOL_FAR))
            assert e_m <= TOL_SAME and e_v <= TOL_SAME and e_far <= TOL_FAR
            assert np.all(got['var'] >= 0.0)
            # each output asked for alone: the same bits
            assert np.array_equal(ctx.posterior_at(s, want=('mean',))['mean'], got['mean']) and np.array_equal(ctx.posterior_at(s, want=('var',))['var'], got['var'])
        grid = ctx.posterior_at(np.arange(T) * BIN_MS)
        e_m = float(np.max(np.abs(grid['mean'] - m)) / scale)
        e_v = float(np.max(np.abs(grid['var'] - np.stack([np.diagonal(V[r], axis1=0, axis2=1) for r in range(R8)]))))
        print('q=%d p=%d T=%d %s grid identity: mean %.2e of max|m|, var %.2e (limit %.0e)' % (q, p, T, CONFIG_IDS[CONFIGS.index(config)], e_m, e_v, TOL_SAME))
        assert e_m <= TOL_SAME and e_v <= TOL_SAME
    finally:
        ctx.close()


# ---- 2. the model extended by the query times as bins without a likelihood term -----------------------------------------------------------------------
def augmented_reference(par, mode, s, T, big):
    """Dense FP64 model over the grid AND the distinct off-grid query times (bins without a likelihood term), at the GP-extended mode: returns
    (mean (p, S), var (p, S)).  The variance is the diagonal of the inverse Hessian; the mean at the extra bins solves the extra rows of the gradient,
    K_aug^-1 x = 0 there, for x given the device's mode on the grid - the precision form of the conditional, not the K^-1 kx the device evaluates.
    A query time ON the grid is that bin itself (the extended Gram matrix would be singular): it reads the grid's own entry.  big: the Hessian through
    orc.nlp_big_hess (the reference's conventions, dense C_big), checked against the structured assembly used at the larger shape."""
    C, d, tau = np.asarray(par['C']), np.asarray(par['d']).reshape(-1), np.asarray(par['tau'])
    p = C.shape[1]
    tg = np.arange(T) * BIN_MS
    on = np.isin(s, tg)
    extra = np.unique(s[~on])
    tt = np.concatenate([tg, extra])
    n = tt.size
    dt = tt[:, None] - tt[None, :]
    Kinv = np.stack([np.linalg.inv((1.0 - EPS) * np.exp(-0.5 * ((dt * dt) / (tau[k] * 1000.0) ** 2)) + EPS * np.eye(n)) for k in range(p)])
    x = np.zeros((p, n))
    x[:, :T] = mode
    for k in range(p):
        x[k, T:] = -np.linalg.solve(Kinv[k][T:, T:], Kinv[k][T:, :T] @ mode[k])
    W = orc.poisson_blocks(mode, C, d)
    H = np.zeros((p, n, p, n))
    ar = np.arange(T)
    for k in range(p):
        H[k, :, k, :] += Kinv[k]
        for l in range(p):
            H[k, ar, l, ar] += W[:, k, l]
    H = H.reshape(p * n, p * n)
    if big:
        C_big = np.zeros((p, n, C.shape[0], T))
        for k in range(p):
            C_big[k, ar, :, ar] = C[:, k][None, :]
        Hb = orc.nlp_big_hess(x.reshape(-1), None, C_big.reshape(p * n, -1), np.kron(d, np.ones(T)), orc.make_K_big(Kinv))
        assert np.max(np.abs(Hb - H)) <= 1e-12 * np.max(np.abs(H))
        H = Hb
    var = np.diag(np.linalg.inv(H)).reshape(p, n)
    col = np.where(on, np.searchsorted(tg, s).clip(0, T - 1), T + np.searchsorted(extra, s).clip(0, max(extra.size - 1, 0)))
    return x[:, col], var[:, col]


@pytest.mark.parametrize('config', CONFIGS, ids=CONFIG_IDS)
@pytest.mark.parametrize('shape', SHAPES[:2], ids=IDS[:2])
def test_off_the_grid_it_is_the_marginal_of_the_model_extended_by_the_query_times(shape, config):
    q, p, T = shape
    ctx, par, _, _ = make_ctx(shape, config)
    try:
        m = ctx.post_mean().reshape(R8, p, T)
        s, far = make_times(T, 65, par['tau'], 1)
        near = np.setdiff1d(np.arange(65), far)                         # (the two distant times are the far-field test's: 50 tau away the extension is the prior)
        trials = np.array([5, 0], dtype=np.int32)
        got = ctx.posterior_at(s[near], trials)
        for i, r in enumerate(trials):
            ref_m, ref_v = augmented_reference(par, m[r], s[near], T, big=(shape == SHAPES[0]))
            e_m = float(np.max(np.abs(got['mean'][i] - ref_m)) / np.max(np.abs(ref_m)))
            e_v = float(np.max(np.abs(got['var'][i] - ref_v)) / np.max(np.abs(ref_v)))
            print('q=%d p=%d T=%d %s trial %d: extended model, mean %.2e var %.2e relative (limit %.0e)' % (q, p, T, CONFIG_IDS[CONFIGS.index(config)], r, e_m, e_v, TOL_DENSE))
            assert e_m <= TOL_DENSE and e_v <= TOL_DENSE
    finally:
        ctx.close()


# ---- 5. ragged trials and both observation tables ---------------------------------------------------------------------------------------------------
def own_grid_reference(par, mode, live, L, s):
    """the trial's own L-bin dense posterior (likelihood terms at its live entries only) at the device's mode, interpolated from its own grid"""
    C, d = np.asarray(par['C']), np.asarray(par['d']).reshape(-1)
    p = C.shape[1]
    X = np.ascontiguousarray(mode[:, :L])
    e = np.exp(C @ X + d[:, None]) * live[:, :L]
    W = np.einsum('nk,nt,nl->tkl', C, e, C)
    Kinv = np.linalg.inv(orc.make_K(par['tau'], L, BIN_MS))
    H = np.zeros((p, L, p, L))
    ar = np.arange(L)
    for k in range(p):
        H[k, :, k, :] += Kinv[k]
        for l in range(p):
            H[k, ar, l, ar] += W[:, k, l]
    V, _ = orc.marginal_blocks(np.linalg.inv(H.reshape(p * L, p * L)), p, L)
    return numpy_at(par['tau'], X, V, s)


@pytest.mark.parametrize('config', CONFIGS, ids=CONFIG_IDS)
@pytest.mark.parametrize('shape', SHAPES[:2], ids=IDS[:2])
def test_ragged_trials_under_both_observation_tables_interpolate_their_own_posterior(shape, config):
    q, p, T = shape
    lens = np.array([T, T - 1, 17, 16, T, 40, T - 7, 33], dtype=np.int32)
    rng = np.random.default_rng(7)
    observed = np.ones((R8, q), dtype=np.uint8)
    observed[1, :5] = 0
    observed[2, q - 4:] = 0
    observed[6, 3::4] = 0
    bins = (rng.random((R8, q, T)) > 0.15).astype(np.uint8)
    bins[0] = 1
    ctx, par, _, live = make_ctx(shape, config, lens=lens, observed=observed, bins=bins)
    try:
        m = ctx.post_mean().reshape(R8, p, T)
        s, _ = make_times(T, 65, par['tau'], 2)
        trials = np.array([0, 1, 2, 3, 6], dtype=np.int32)
        # on top: query times inside [T_r bin, T bin) of the short trials and grid times at padded bins
        s = np.concatenate([s, [16.5 * BIN_MS, 17.0 * BIN_MS, 20.0 * BIN_MS, (T - 1.5) * BIN_MS, (T - 1.0) * BIN_MS, 0.5 * (17 + T) * BIN_MS]])
        got = ctx.posterior_at(s, trials)
        for i, r in enumerate(trials):
            ref_m, ref_v = own_grid_reference(par, m[r], live[r], int(lens[r]), s)
            e_m = float(np.max(np.abs(got['mean'][i] - ref_m)) / np.max(np.abs(m[r])))
            e_v = float(np.max(np.abs(got['var'][i] - ref_v)))
            print('q=%d p=%d T=%d %s trial %d (%d bins): own-grid posterior, mean %.2e of max|m|, var %.2e (limit %.0e)'
                  % (q, p, T, CONFIG_IDS[CONFIGS.index(config)], r, lens[r], e_m, e_v, TOL_DENSE))
            assert e_m <= TOL_DENSE and e_v <= TOL_DENSE
    finally:
        ctx.close()


# ---- 6. per-trial grids; nothing depends on the list -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('config', CONFIGS, ids=CONFIG_IDS)
@pytest.mark.parametrize('shape', [SHAPES[0], SHAPES[5]], ids=[IDS[0], IDS[5]])
def test_per_trial_grids_and_results_that_do_not_depend_on_the_list(shape, config):
    q, p, T = shape
    ctx, par, _, _ = make_ctx(shape, config)
    try:
        scale = float(np.max(np.abs(ctx.post_mean())))
        for S in (17, 65):
            grids = np.stack([make_times(T, S, par['tau'], 10 + r)[0] for r in range(R8)])
            per = ctx.posterior_at(grids)
            e_m = e_v = 0.0
            for r in range(R8):
                one = ctx.posterior_at(grids[r], np.array([r], dtype=np.int32))
                e_m = max(e_m, float(np.max(np.abs(per['mean'][r] - one['mean'][0])) / scale))
                e_v = max(e_v, float(np.max(np.abs(per['var'][r] - one['var'][0]))))
            print('q=%d p=%d T=%d %s S=%d: (n, S) call against n shared-grid calls, mean %.2e var %.2e (limit %.0e)'
                  % (q, p, T, CONFIG_IDS[CONFIGS.index(config)], S, e_m, e_v, TOL_SAME))
            assert e_m <= TOL_SAME and e_v <= TOL_SAME
            again = ctx.posterior_at(grids)
            assert np.array_equal(again['mean'], per['mean']) and np.array_equal(again['var'], per['var'])
            shared = ctx.posterior_at(grids[0])
            order = np.array([6, 2, 2, 7, 0, 5, 1, 3, 4, 2], dtype=np.int32)     # permuted, trial 2 three times
            for chunk in (1, 3, 0):
                ctx.set_option('interp_chunk_trials', chunk)
                a = ctx.posterior_at(grids)
                b = ctx.posterior_at(grids[order], order)
                c = ctx.posterior_at(grids[0], order)
                assert np.array_equal(a['mean'], per['mean']) and np.array_equal(a['var'], per['var'])
                assert np.array_equal(b['mean'], per['mean'][order]) and np.array_equal(b['var'], per['var'][order])
                assert np.array_equal(c['mean'], shared['mean'][order]) and np.array_equal(c['var'], shared['var'][order])
    finally:
        ctx.close()


# ---- 7. the snapshot of the E-step; nothing else moves ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('config', CONFIGS, ids=CONFIG_IDS)
def test_the_estep_timescales_are_used_and_no_state_is_touched(config):
    shape = SHAPES[0]
    q, p, T = shape
    s, _ = make_times(T, 65, np.array([0.15]), 3)
    state = {}
    for call in (True, False):
        ctx, par, _, _ = make_ctx(shape, config, evidence=True)
        try:
            if call:
                before = ctx.posterior_at(s)
            ctx.set_params(par['C'], par['d'], par['tau'] * np.linspace(1.3, 0.7, p))
            if call:
                after = ctx.posterior_at(s)
                assert np.array_equal(after['mean'], before['mean']) and np.array_equal(after['var'], before['var'])
            ctx.mstep_precomp()
            out = [ctx.pautosum(), ctx.post_mean(), ctx.post_vsm(), ctx.post_vsmgp(), ctx.log_evidence()]
            obj, _, status = ctx.estep_laplace(warm_start=True)
            assert np.all(status == 0)
            state[call] = out + [np.array([obj]), ctx.post_mean()]
        finally:
            ctx.close()
    same = [bool(np.array_equal(a, b)) for a, b in zip(state[True], state[False])]
    print('%s: bit-identical to a context that never made the call (PautoSum, post_mean, post_vsm, post_vsmGP, log evidence, warm objective, its modes): %s'
          % (CONFIG_IDS[CONFIGS.index(config)], same))
    assert all(same)


@pytest.mark.parametrize('config', CONFIGS, ids=CONFIG_IDS)
def test_a_list_across_two_parameter_snapshots_gives_the_bits_of_one_call_per_trial(config):
    """four trials, {0, 1} through an E-step at parameters A and {2, 3} through one at B (C, d and every timescale differ): one call over
    [3, 0, 2, 1, 0] walks two snapshot groups and scatters by list position"""
    from funs import _hip
    shape = SHAPES[4]                                    # (the smallest)
    q, p, T = shape
    par, Y, _ = problem(shape, R=4)
    mixed = np.array([3, 0, 2, 1, 0], dtype=np.int32)
    s = np.array([0.0, 3.7, 10.0, T - 1.0, T + 2.5]) * BIN_MS      # on the grid, off it, beyond the last bin
    ctx = _hip.Context(q, p, T, 4, BIN_MS)
    try:
        ctx.upload_counts(Y.astype(np.uint16 if Y.max() > 255 else np.uint8))
        ctx.set_option('cov_mode', config[0])
        ctx.set_option('keep_trial_vsmgp', config[1])
        ctx.set_params(par['C'], par['d'], par['tau'])
        _, _, status = ctx.estep_laplace(np.array([0, 1], dtype=np.int32))
        assert np.all(status == 0), status
        ctx.set_params(par['C'] * 1.05 + 0.01, par['d'] + 0.1, par['tau'] * np.linspace(0.85, 0.95, p))
        _, _, status = ctx.estep_laplace(np.array([2, 3], dtype=np.int32))
        assert np.all(status == 0), status
        assert ctx.info('plan_lowrank') == float(config[0] == 2)
        before = [ctx.post_mean(), ctx.post_vsm(), ctx.gram()]
        one = ctx.posterior_at(s, mixed)
        after = [ctx.post_mean(), ctx.post_vsm(), ctx.gram()]
        same = []
        for i in range(mixed.size):
            single = ctx.posterior_at(s, mixed[i:i + 1])
            same.append(bool(np.array_equal(one['mean'][i], single['mean'][0]) and np.array_equal(one['var'][i], single['var'][0])))
        kept = [bool(np.array_equal(a, b)) for a, b in zip(before, after)]
        print('%s: list %s against one call per entry %s; post_mean, post_vsm, Gram unchanged %s' % (CONFIG_IDS[CONFIGS.index(config)], mixed.tolist(), same, kept))
        assert all(same)
        assert np.array_equal(one['mean'][1], one['mean'][4]) and np.array_equal(one['var'][1], one['var'][4])
        assert all(kept)
    finally:
        ctx.close()


# ---- 8. variational and uploaded posteriors --------------------------------------------------------------------------------------------------------
def _var_problem(which):
    if which == 'var_toy':
        g = load_golden('var_toy.npz')
        return {'C': g['init_C'], 'd': g['init_d'], 'tau': g['init_tau']}, g['Y'][:3], float(g['binSize'])
    par, Y, _ = problem((40, 10, 64), R=3)
    return par, Y, BIN_MS


@pytest.mark.parametrize('engine', [1, 2], ids=['dense', 'lowrank'])
@pytest.mark.parametrize('which', ['var_toy', 'q40-p10-T64'])
def test_variational_posterior_against_the_oracle_at_the_kept_lambda(which, engine):
    from funs import _hip
    par, Y, binSize = _var_problem(which)
    assert binSize == BIN_MS
    R, q, T = Y.shape
    p = par['C'].shape[1]
    C_big, _ = orc.make_Cd_big(par['C'], par['d'], T)
    K_big = orc.make_K_big(orc.make_K(par['tau'], T, binSize))
    Kinv_big = np.linalg.inv(K_big)
    ctx = _hip.Context(q, p, T, R, binSize)
    try:
        ctx.upload_counts(Y.astype(np.uint16 if Y.max() > 255 else np.uint8))
        ctx.set_option('cov_mode', engine)
        ctx.set_option('dual_lowrank', int(engine == 2))
        ctx.set_params(par['C'], par['d'], par['tau'])
        _, _, _, status, lam = ctx.dual_fixed_point(None, None, want_lam=True)
        assert np.all(status == 0), status
        ctx.dual_finalize(None, None)
        s, _ = make_times(T, 65, par['tau'], 4)
        got = ctx.posterior_at(s)
        for r in range(R):
            Sigma, _ = orc.vi_post_cov(Kinv_big, C_big, lam[r])
            mean = orc.vi_post_mean(K_big, C_big, Y[r].reshape(-1).astype(np.float64), lam[r]).reshape(p, T)
            V, _ = orc.marginal_blocks(Sigma, p, T)
            ref_m, ref_v = numpy_at(par['tau'], mean, V, s)
            e_m = float(np.max(np.abs(got['mean'][r] - ref_m)) / np.max(np.abs(mean)))
            e_v = float(np.max(np.abs(got['var'][r] - ref_v)))
            print('%s engine %d trial %d: VIPostMean / VIPostCov at the kept lambda, mean %.2e of max|m|, var %.2e (limit %.0e)' % (which, engine, r, e_m, e_v, TOL_DENSE))
            assert e_m <= TOL_DENSE and e_v <= TOL_DENSE
    finally:
        ctx.close()


def test_an_uploaded_posterior_is_evaluated_under_the_current_parameters():
    from funs import _hip
    q, p, T, R = 9, 4, 37, 3
    rng = np.random.default_rng(11)
    tau = np.array([0.05, 0.08, 0.11, 0.2])
    K = orc.make_K(tau, T, BIN_MS)
    m = np.stack([np.stack([np.linalg.cholesky(K[k]) @ rng.standard_normal(T) for k in range(p)]) for _ in range(R)])
    V = np.empty((R, T, T, p))
    for r in range(R):
        for k in range(p):
            V[r, :, :, k] = np.linalg.inv(np.linalg.inv(K[k]) + np.diag(rng.uniform(0.1, 2.0, T)))
    vsm = np.zeros((R, T, p, p))
    for k in range(p):
        vsm[:, :, k, k] = np.diagonal(V[:, :, :, k], axis1=1, axis2=2)
    ctx = _hip.Context(q, p, T, R, BIN_MS)
    try:
        ctx.set_params(rng.standard_normal((q, p)), np.zeros(q), tau)
        with pytest.raises(_hip.HipBackendError, match='no posterior for trial 0'):
            ctx.posterior_at(np.zeros(3))
        ctx.set_posterior(None, m, vsm, V)
        s, _ = make_times(T, 65, tau, 5)
        for scale_tau in (1.0, 1.4):                                  # ... whatever they are when the call is made
            ctx.set_params(rng.standard_normal((q, p)), np.zeros(q), tau * scale_tau)
            got = ctx.posterior_at(s, np.array([2, 0], dtype=np.int32))
            for i, r in enumerate((2, 0)):
                ref_m, ref_v = numpy_at(tau * scale_tau, m[r], V[r], s)
                e_m, e_v = float(np.max(np.abs(got['mean'][i] - ref_m)) / np.max(np.abs(m[r]))), float(np.max(np.abs(got['var'][i] - ref_v)))
                print('uploaded posterior, tau x %.1f, trial %d: mean %.2e of max|m|, var %.2e (limit %.0e)' % (scale_tau, r, e_m, e_v, TOL_SAME))
                assert e_m <= TOL_SAME and e_v <= TOL_SAME
    finally:
        ctx.close()


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_names_what_is_wrong():
    from funs import _hip
    shape = (20, 3, 40)
    q, p, T = shape
    par, Y, _ = problem(shape, R=4)
    ctx = _hip.Context(q, p, T, 4, BIN_MS)
    try:
        ctx.upload_counts(Y.astype(np.uint8))
        with pytest.raises(_hip.HipBackendError, match='set_params has not been called'):
            ctx.posterior_at(np.zeros(3))
        ctx.set_params(par['C'], par['d'], par['tau'])
        with pytest.raises(_hip.HipBackendError, match='no posterior for trial 0'):
            ctx.posterior_at(np.zeros(3))
        ctx.estep_laplace(np.array([0, 1, 2], dtype=np.int32))
        with pytest.raises(_hip.HipBackendError, match='no posterior for trial 3'):
            ctx.posterior_at(np.zeros(3))
        idx = np.array([2, 0], dtype=np.int32)
        assert ctx.posterior_at(np.zeros(3), idx)['mean'].shape == (2, p, 3)
        with pytest.raises(_hip.HipBackendError, match='S = 0'):
            ctx.posterior_at(np.zeros(0), idx)
        t = np.zeros(3)
        assert ctx.lib.pgpfa_posterior_at(ctx.h, 2, _hip.iptr(idx), 3, _hip.dptr(t), 0, None, None) != 0
        assert 'no output asked for' in ctx.lib.pgpfa_last_error().decode()
        with pytest.raises(_hip.HipBackendError, match='query time 1 is not finite'):
            ctx.posterior_at(np.array([0.0, np.nan, 1.0]), idx)
        grids = np.zeros((2, 3))
        grids[1, 2] = np.inf
        with pytest.raises(_hip.HipBackendError, match=r'query time 2 of list entry 1 \(trial 0\) is not finite'):
            ctx.posterior_at(grids, idx)
        with pytest.raises(ValueError, match='times must have shape'):
            ctx.posterior_at(np.zeros((3, 3)), idx)
        with pytest.raises(ValueError, match='unknown output'):
            ctx.posterior_at(np.zeros(3), idx, want=('mean', 'cov'))
        # an asynchronous timescale pass in flight
        ctx.mstep_precomp()
        Q = np.log(1.0 / (par['tau'] * 100.0) ** 2)[None, :] + np.array([0.0, 0.1])[:, None]
        ctx.mstep_tau_costgrad_multi_begin(Q)
        with pytest.raises(_hip.HipBackendError, match='timescale pass is in flight'):
            ctx.posterior_at(np.zeros(3), idx)
        ctx.mstep_tau_costgrad_multi_end()
        assert ctx.posterior_at(np.zeros(3), idx)['var'].shape == (2, p, 3)
        # counts uploaded after the E-step: the posterior is gone
        ctx.upload_counts(Y.astype(np.uint8))
        with pytest.raises(_hip.HipBackendError, match='no posterior for trial 2'):
            ctx.posterior_at(np.zeros(3), idx)
    finally:
        ctx.close()


def test_a_variational_posterior_of_a_short_trial_is_refused():
    from funs import _hip
    shape = (20, 3, 40)
    q, p, T = shape
    par, Y, _ = problem(shape, R=3)
    lens = np.array([T, 23, T], dtype=np.int32)
    Y = Y * (np.arange(T)[None, None, :] < lens[:, None, None])
    ctx = _hip.Context(q, p, T, 3, BIN_MS)
    try:
        ctx.upload_counts(Y.astype(np.uint8))
        ctx.set_trial_lengths(lens)
        ctx.set_option('dual_masked', 1)
        ctx.set_params(par['C'], par['d'], par['tau'])
        _, _, _, status = ctx.dual_fixed_point(None, None)
        assert np.all(status == 0), status
        ctx.dual_finalize(None, None)
        with pytest.raises(_hip.HipBackendError, match='variational posterior of trial 1 covers 23 of 40 bins'):
            ctx.posterior_at(np.zeros(3))
        assert ctx.posterior_at(np.zeros(3), np.array([0, 2], dtype=np.int32))['mean'].shape == (2, p, 3)      # the full-length ones are served
    finally:
        ctx.close()


# ---- 10. the Python surface -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def funs_mod():
    import funs
    from funs import _session
    _session.drop_sessions()
    yield funs
    _session.drop_sessions()


def test_util_posterior_at_with_conditions_on_a_ragged_config1_experiment(funs_mod):
    util, inference = funs_mod.util, funs_mod.inference
    shape = SHAPES[0]
    q, p, T = shape
    par, Y, _ = problem(shape, R=R8)
    lens = np.array([T, T - 1, 17, 16, T, 40, T - 7, 33])
    exp = Experiment([Y[r][:, :lens[r]].astype(np.float64) for r in range(R8)], BIN_MS)
    params = {k: np.array(v, dtype=np.float64) for k, v in par.items()}
    infRes, _ = inference.laplace(exp, {k: v.copy() for k, v in params.items()}, returnOptimRes=False)
    s, _ = make_times(T, 65, par['tau'], 6)
    s = np.concatenate([s, [0.0, 150.0, 160.0, 160.0 + 1e-9, (T - 1) * BIN_MS]])
    cond = np.array([4, 9, 4, 9, 4, 4, 9, 9])
    out = util.posteriorAt(params, exp, s, infRes=infRes, conditions=cond, level=0.9, want=('mean', 'var', 'lower', 'upper'))
    assert out['mean'].shape == (R8, p, s.size) and np.array_equal(out['times'], s) and out['condition_labels'].tolist() == [4, 9]
    live = np.ones((q, T))
    ref = []
    for r in range(R8):
        mode = np.zeros((p, T))
        mode[:, :lens[r]] = np.asarray(infRes['post_mean'][r])[:, :lens[r]]
        ref.append(own_grid_reference(par, mode, live, int(lens[r]), s))
    ref_m, ref_v = np.stack([a for a, _ in ref]), np.stack([b for _, b in ref])
    e_m, e_v = float(np.max(np.abs(out['mean'] - ref_m)) / np.max(np.abs(ref_m))), float(np.max(np.abs(out['var'] - ref_v)))
    print('util.posteriorAt on ragged config 1: mean %.2e of max|m|, var %.2e (limit %.0e)' % (e_m, e_v, TOL_DENSE))
    assert e_m <= TOL_DENSE and e_v <= TOL_DENSE
    z = util._band_z(0.9)
    assert np.array_equal(out['lower'], out['mean'] - z * np.sqrt(out['var'])) and np.array_equal(out['upper'], out['mean'] + z * np.sqrt(out['var']))
    # the host formula on the numpy means: a trial enters at s only inside its own recorded span
    inside = (s[None, :] >= 0.0) & (s[None, :] <= ((lens - 1) * BIN_MS)[:, None])
    for g, label in enumerate((4, 9)):
        members = np.flatnonzero(cond == label)
        count = inside[members].sum(axis=0)
        assert np.array_equal(out['condition_count'][g], count)
        total = (ref_m[members] * inside[members][:, None, :]).sum(axis=0)
        want = np.where(count[None, :] > 0, total / np.maximum(count, 1)[None, :], 0.0)
        err = float(np.max(np.abs(out['condition_mean'][g] - want)) / np.max(np.abs(ref_m)))
        print('condition %d: mean on the common axis %.2e of max|m| (limit %.0e)' % (label, err, TOL_DENSE))
        assert err <= TOL_DENSE
        assert np.all(out['condition_mean'][g][:, count == 0] == 0.0)
    assert out['condition_count'][:, list(s).index(160.0)].tolist() == [4, 3] and out['condition_count'][:, list(s).index(160.0 + 1e-9)].tolist() == [3, 3]
    # event alignment: one grid per trial equals the shared call where the grids agree
    lags = np.arange(-3, 4) * 7.5
    event = np.array([300.0, 120.0, 80.0, 95.0, 500.0, 210.0, 640.0, 100.0])
    per = util.posteriorAt(params, exp, event[:, None] + lags[None, :], infRes=infRes, want=('mean',))
    one = util.posteriorAt(params, exp, event[2] + lags, infRes=infRes, trials=[2], want=('mean',))
    assert per['mean'].shape == (R8, p, 7) and float(np.max(np.abs(per['mean'][2] - one['mean'][0]))) <= TOL_SAME * np.max(np.abs(ref_m))


def test_fit_posterior_at_after_a_two_iteration_fit(funs_mod):
    shape = SHAPES[0]
    q, p, T = shape
    par, Y, _ = problem(shape, R=R8)
    exp = Experiment([Y[r].astype(np.float64) for r in range(R8)], BIN_MS)
    init = {k: np.array(v, dtype=np.float64) for k, v in par.items()}
    fit = funs_mod.engine.PPGPFAfit(exp, initParams=init, EMmode='Batch', maxEMiter=2, CdOptimMethod='newton', quiet=True)
    fine = np.arange(0.0, (T - 1) * BIN_MS + 1e-9, BIN_MS / 4.0)
    out = fit.posteriorAt(times=fine, conditions=np.arange(R8) % 2, want=('mean', 'lower', 'upper'))
    assert fit.trajectoriesAt is out and out['mean'].shape == (R8, p, fine.size) and out['condition_mean'].shape == (2, p, fine.size)
    assert np.all(out['lower'] <= out['mean']) and np.all(out['mean'] <= out['upper'])
    assert np.array_equal(out['condition_count'], np.full((2, fine.size), R8 // 2))
    assert fit.infRes['post_mean'][3].shape == (p, T)                  # kept on the host before the E-step superseded it
    # on the grid the upsampled trajectory passes through the posterior mean of the E-step that util.posteriorAt ran
    from funs import _session
    sess, _ = _session.session_for(exp, p)
    pm = sess.ctx.post_mean().reshape(R8, p, T)
    assert float(np.max(np.abs(out['mean'][:, :, ::4] - pm))) <= TOL_SAME * np.max(np.abs(pm))
    for g in range(2):
        assert np.allclose(out['condition_mean'][g], out['mean'][g::2].mean(axis=0), rtol=1e-12, atol=1e-15)
