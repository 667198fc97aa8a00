"""Importance-sampled log evidence and weights from the Laplace posterior (pgpfa_importance_weights, Context.importance_weights,
util.importanceEvidence):

    log w_s = - sum_{(n,t) live} lambda*_nt phi(c_n . delta_st),   log_ratio = log mean_s w_s,   ess = (sum w)^2 / sum w^2

for the draws x_s = x* + delta_s of pgpfa_posterior_sample under the same seed.  The yardstick is the numpy restatement of
test_cpu_importance_evidence.py (which that file pins to the oracle's dense definition) evaluated at the device's own draws and mode; it needs no
K, so it is the same under both covariance engines.  Eight trials per shape; the shapes sit on the seams of the kernel: neuron tiles of 16, bin
tiles of 16, a single latent, a bin count below one tile and one past four.  Tolerances are the issue's: log_w 1e-9 max(1, sum lambda* (e^a + 1
+ |a| + a^2 / 2)) per draw, log_ratio 1e-9 absolute (the project's for a log evidence), ess 1e-9 relative.  The truth test integrates a
4-dimensional posterior by a tensor Gauss-Hermite rule.  Every test prints its figures before it asserts."""
import ctypes as ct

import numpy as np
import pytest

from conftest import Experiment, load_golden
from oracle import pgpfa_oracle as orc
from test_cpu_importance_evidence import log_ratio_ess, log_ratio_se, log_weights, small_masks
from test_cpu_posterior_samples import BIN_MS, problem

pytestmark = pytest.mark.gpu

SHAPES = [(7, 3, 24), (18, 10, 40), (9, 12, 20), (12, 20, 17),        # the sampler's own shapes
          (16, 3, 24), (17, 3, 24), (33, 10, 24),                     # neuron tiles of 16: exactly one, one more row, two and one row
          (12, 1, 4), (9, 3, 65)]                                     # bin tiles of 16: a quarter of one, four and one bin
IDS = ['q%d-p%d-T%d' % s for s in SHAPES]
ENGINES = [1, 2]
ENGINE_IDS = ['dense', 'lowrank']
NO_LOWRANK = set()                     # shapes at which option cov_mode = 2 still plans the dense engine (core.hip: want_lowrank); checked below
R8 = 8
LIST = np.array([2, 0, 7, 5, 3, 1, 6, 4, 2], dtype=np.int32)
VARIANTS = ['plain', 'ragged', 'observed', 'bins']
ALL = ('log_ratio', 'ess', 'log_w')
TOL = 1e-9


@pytest.fixture(scope='module', autouse=True)
def _leave_nothing_behind():
    yield
    import gc
    from funs import _session
    _session.drop_sessions()
    _cases.clear()
    gc.collect()


# ---- problems: computed once, shared, never written to -------------------------------------------------------------------------------------------
_cases = {}


def case(shape, variant):
    """(params, counts [8][q][T] zero at dead entries, live [8][q][T], lengths or None, 'observed' [8][q] or None, per-bin table or None)"""
    if (shape, variant) not in _cases:
        q, p, T = shape
        par, Y, _ = problem(shape, R=R8, d_offset=float(np.log(400.0)) if variant == 'big' else -1.0)
        lens = obs = bins = None
        live = np.ones((R8, q, T), bool)
        if variant == 'ragged':
            lens = np.array([T, T - 1, max(1, T // 2), 1, max(1, T - 16), min(T, 16), min(T, 17), max(1, T // 3)], dtype=np.int32)
            live = np.broadcast_to(np.arange(T)[None, None, :] < lens[:, None, None], (R8, q, T)).copy()
        elif variant == 'observed':
            obs = np.random.default_rng(q + T).random((R8, q)) > 0.3
            obs[:, 0], obs[:, 1] = True, False
            obs[4, 1] = True                                    # (neuron 1 is dead on every trial but 4: the library refuses a neuron observed nowhere)
            live = np.broadcast_to(obs[:, :, None], (R8, q, T)).copy()
        elif variant == 'bins':
            bins = small_masks(R8, q, T)
            live = bins.copy()
        Y = Y * live
        if variant == 'big':
            assert Y.max() > 255
        _cases[(shape, variant)] = (par, Y, live, lens, obs, bins)
    return _cases[(shape, variant)]


def open_ctx(shape, variant, engine, par=None, evidence=False, trials=None):
    """context of the 8-trial problem after one Laplace E-step (over `trials`; None: all) under option cov_mode = engine -> (ctx, params, live,
    low-rank engine planned)"""
    from funs import _hip
    q, p, T = shape
    par0, Y, live, lens, obs, bins = case(shape, variant)
    par = par0 if par is None else par
    ctx = _hip.Context(q, p, T, R8, BIN_MS)
    try:
        ctx.upload_counts(Y.astype(np.uint16 if Y.max() > 255 else np.uint8))
        ctx.set_option('cov_mode', engine)
        if evidence:
            ctx.set_option('laplace_evidence', 1)
        ctx.set_params(par['C'], par['d'], par['tau'])
        if lens is not None:
            ctx.set_trial_lengths(lens)
        if obs is not None:
            ctx.set_observed(obs)
        if bins is not None:
            ctx.set_observed_bins(bins)
        _, _, status = ctx.estep_laplace(trials)
        assert np.all(status == 0), status
        lowrank = ctx.info('plan_lowrank') == 1.0
        assert lowrank == (engine == 2 and shape not in NO_LOWRANK), 'cov_mode %d at %s plans low-rank = %s' % (engine, shape, lowrank)
    except BaseException:
        ctx.close()
        raise
    return ctx, par, live, lowrank


def check_against_restatement(tag, ctx, par, live, idx, S, seed):
    """device log_w / log_ratio / ess of `idx` against the restatement at the device's own draws -> worst errors in units of their tolerances"""
    X = ctx.posterior_sample(idx, n_samples=S, seed=seed)['x']
    out = ctx.importance_weights(idx, n_samples=S, seed=seed, want=ALL)
    assert out['log_w'].shape == (len(idx), S) and out['log_ratio'].shape == (len(idx),) and out['ess'].shape == (len(idx),)
    m = ctx.post_mean()
    e_w = e_r = e_e = 0.0
    for i, t in enumerate(idx):
        lw, scale = log_weights(par['C'], par['d'], m[t], X[i], live[t], with_scale=True)
        lr, ess = log_ratio_ess(lw)
        e_w = max(e_w, float(np.max(np.abs(out['log_w'][i] - lw) / (TOL * np.maximum(1.0, scale)))))
        e_r = max(e_r, abs(out['log_ratio'][i] - lr) / TOL)
        e_e = max(e_e, abs(out['ess'][i] - ess) / (TOL * ess))
    print('%s, S = %d: log_w in [%.3g, %.3g], ess / S in [%.3f, %.3f]; errors in units of the tolerance: log_w %.2e, log_ratio %.2e, ess %.2e'
          % (tag, S, out['log_w'].min(), out['log_w'].max(), out['ess'].min() / S, out['ess'].max() / S, e_w, e_r, e_e))
    assert np.all(np.isfinite(out['log_w'])) and np.all(out['ess'] >= 1.0 - 1e-12) and np.all(out['ess'] <= S * (1.0 + 1e-12))
    assert e_w <= 1.0 and e_r <= 1.0 and e_e <= 1.0
    return out


# ---- 1. against the restatement, same draws --------------------------------------------------------------------------------------------------------
SHAPE_ENGINES = [(s, e) for s in SHAPES for e in ENGINES if not (e == 2 and s in NO_LOWRANK)]


@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('shape,engine', SHAPE_ENGINES, ids=['q%d-p%d-T%d-%s' % (s + (ENGINE_IDS[e - 1],)) for s, e in SHAPE_ENGINES])
def test_weights_against_the_restatement_at_the_same_draws(shape, engine, variant):
    ctx, par, live, lowrank = open_ctx(shape, variant, engine)
    try:
        for S in (1, 5, 64):
            check_against_restatement('q=%d p=%d T=%d %s, %s engine' % (shape + (variant, 'low-rank' if lowrank else 'dense')), ctx, par, live, LIST, S, seed=7)
    finally:
        ctx.close()


@pytest.mark.parametrize('engine', ENGINES, ids=ENGINE_IDS)
@pytest.mark.parametrize('shape', [SHAPES[0], SHAPES[5]], ids=[IDS[0], IDS[5]])
def test_counts_above_255(shape, engine):
    """d raised to log 400: rates of several hundred per bin, two-byte counts, sums of lambda* phi(a) four orders larger"""
    ctx, par, live, lowrank = open_ctx(shape, 'big', engine)
    try:
        for S in (1, 5, 64):
            check_against_restatement('q=%d p=%d T=%d d = log 400, engine %d' % (shape + (engine,)), ctx, par, live, LIST, S, seed=7)
    finally:
        ctx.close()


@pytest.mark.parametrize('variant', ['observed', 'bins'])
@pytest.mark.parametrize('engine', ENGINES, ids=ENGINE_IDS)
@pytest.mark.parametrize('shape', [SHAPES[5], SHAPES[6]], ids=[IDS[5], IDS[6]])
def test_dead_entries_contribute_exactly_zero(shape, engine, variant):
    """C[n], d[n] of a neuron that is dead on every listed trial set to 1e3 (exp overflows): no bit of any output may change.  'observed': neuron
    1, every trial but 4, which is not listed and not in the E-step; per-bin table: neuron 3 on trial 3 (pattern 4), the list is that trial."""
    idx = LIST[LIST != 4] if variant == 'observed' else np.array([3, 3], dtype=np.int32)
    n_dead = 1 if variant == 'observed' else 3
    outs = []
    for huge in (False, True):
        par = {k: np.array(v, dtype=np.float64) for k, v in case(shape, variant)[0].items()}
        if huge:
            par['C'][n_dead], par['d'][n_dead] = 1e3, 1e3
        ctx, _, live, _ = open_ctx(shape, variant, engine, par=par, trials=np.unique(idx).astype(np.int32))
        try:
            assert not live[idx][:, n_dead].any()
            outs.append((ctx.post_mean(idx), ctx.importance_weights(idx, n_samples=16, seed=5, want=ALL)))
        finally:
            ctx.close()
    (m0, a), (m1, b) = outs
    same = {k: bool(np.array_equal(a[k], b[k])) for k in ALL}
    print('q=%d p=%d T=%d engine %d %s: modes equal %s, outputs equal %s' % (shape + (engine, variant, np.array_equal(m0, m1), same)))
    assert np.array_equal(m0, m1) and all(same.values()) and np.all(np.isfinite(a['log_w']))


# ---- 2. reproducibility ------------------------------------------------------------------------------------------------------------------------------
# (The weights are a pure function of the draws, so what this checks end to end is the sampler's contract plus the kernels' own.  At q18-p10-T40
# under the DENSE engine - n_pad = 512, a chunk workspace of 8 slots - the sampler itself does not keep it: the draws of a trial differ in the last
# bit (up to 9e-16) between a chunk of 8 trials and a chunk of 1, because the factorization's GEMMs pick their tiles and k parts by the batch size
# (linalg.hip: gemm - the likely cause).  Nothing on that path is new; docs/history/importance_evidence.md.  That shape therefore runs
# here under the low-rank engine only, the dense engine at q33-p10-T24.)
REPRO = [(SHAPES[1], 2), (SHAPES[6], 1), (SHAPES[6], 2)]


@pytest.mark.parametrize('shape,engine', REPRO, ids=['q%d-p%d-T%d-%s' % (s + (ENGINE_IDS[e - 1],)) for s, e in REPRO])
def test_a_weight_is_a_pure_function_of_seed_trial_and_sample(shape, engine):
    ctx, par, live, _ = open_ctx(shape, 'bins', engine)
    try:
        a = ctx.importance_weights(LIST, n_samples=64, seed=7, want=ALL)
        same = ctx.importance_weights(LIST, n_samples=64, seed=7, want=ALL)
        x = ctx.posterior_sample(LIST, n_samples=64, seed=7)['x']
        print('q=%d p=%d T=%d engine %d: a trial listed twice - draws equal %s, log_w equal %s (largest difference %.1e), log_ratio %s, ess %s'
              % (shape + (engine, np.array_equal(x[0], x[8]), np.array_equal(a['log_w'][0], a['log_w'][8]), np.max(np.abs(a['log_w'][0] - a['log_w'][8])),
                          a['log_ratio'][0] == a['log_ratio'][8], a['ess'][0] == a['ess'][8])))
        for k in ALL:
            assert np.array_equal(same[k], a[k]), k                                    # the same call twice
            assert np.array_equal(a[k][0], a[k][8]), k                                 # a trial listed twice
        perm = np.array([8, 3, 0, 5, 1, 7, 2, 6, 4])
        other = ctx.importance_weights(LIST[perm], n_samples=64, seed=7, want=ALL)
        for k in ALL:
            assert np.array_equal(other[k], a[k][perm]), k                             # another list order
        single = ctx.importance_weights(LIST[4:5], n_samples=64, seed=7, want=ALL)
        for k in ALL:
            assert np.array_equal(single[k][0], a[k][4]), k                            # whatever else is listed
        ctx.set_option('sample_chunk_trials', 1)
        chunked = ctx.importance_weights(LIST, n_samples=64, seed=7, want=ALL)
        ctx.set_option('sample_chunk_trials', 0)
        for k in ALL:
            assert np.array_equal(chunked[k], a[k]), k
        short = ctx.importance_weights(LIST, n_samples=8, seed=7, want=('log_w',))
        assert np.array_equal(short['log_w'], a['log_w'][:, :8])                       # draw s does not know how many were asked for
        only = ctx.importance_weights(LIST, n_samples=64, seed=7, want=('ess',))
        assert sorted(only) == ['ess'] and np.array_equal(only['ess'], a['ess'])
        new = ctx.importance_weights(LIST, n_samples=64, seed=8, want=('log_w',))
        assert not np.array_equal(new['log_w'], a['log_w'])
    finally:
        ctx.close()


# ---- 3. nothing else moves ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('engine', ENGINES, ids=ENGINE_IDS)
def test_the_call_leaves_the_resident_state_alone(engine):
    shape = SHAPES[0]
    ctx, par, live, _ = open_ctx(shape, 'plain', engine, evidence=True)
    try:
        before_move = ctx.importance_weights(LIST, n_samples=16, seed=1, want=ALL)
        ctx.mstep_precomp()
        # an M-step has moved the parameters on: the weights must still be those of the E-step's own parameters (the snapshot path)
        C2, d2, tau2 = par['C'] * 1.05 + 0.01, par['d'] + 0.1, par['tau'] * 0.9
        ctx.set_params(C2, d2, tau2)
        v = orc.cd_to_vec(C2, d2)

        def state():
            cost, grad = ctx.mstep_cd_costgrad(v)
            return {'post_mean': ctx.post_mean(), 'post_vsm': ctx.post_vsm(), 'post_vsmgp': ctx.post_vsmgp(), 'pautosum': ctx.pautosum(),
                    'cd_cost': np.array(cost), 'cd_grad': grad, 'log_evidence': ctx.log_evidence(),
                    'sample': ctx.posterior_sample(LIST, n_samples=16, seed=1, want=('x',))['x']}
        ctx.post_vsmgp()                     # (under the sum-only plan the first request rebuilds the blocks: before the comparison, not inside it)
        s0 = state()
        after_move = ctx.importance_weights(LIST, n_samples=16, seed=1, want=ALL)
        s1 = state()
        for k in s0:
            assert np.array_equal(s0[k], s1[k]), k
        for k in ALL:
            assert np.array_equal(after_move[k], before_move[k]), k
        # and they are the weights of the draws the sampler hands out now
        m = ctx.post_mean()
        lw, scale = log_weights(par['C'], par['d'], m[2], s1['sample'][0], live[2], with_scale=True)
        assert np.all(np.abs(after_move['log_w'][0] - lw) <= TOL * np.maximum(1.0, scale))
        print('engine %d: state bit-identical around a weights call under a parameter snapshot' % engine)
    finally:
        ctx.close()


# ---- 4. truth by quadrature --------------------------------------------------------------------------------------------------------------------------
QUAD_SHAPE = (12, 1, 4)
QUAD_SEED = 100
QUAD_S = 4096


def quad_problem(seed=QUAD_SEED):
    """p = 1, T = 4, q = 12 at low rates: C ~ N(0, 1.5^2), d = -2.5, timescale 5 bins; the counts of one trajectory drawn from the prior"""
    q, p, T = QUAD_SHAPE
    rng = np.random.default_rng(seed)
    C = 1.5 * rng.standard_normal((q, p))
    d = np.full(q, -2.5)
    tau = np.array([5.0 * BIN_MS / 1000.0])
    x = np.linalg.cholesky(orc.make_K(tau, T, BIN_MS)[0]) @ rng.standard_normal(T)
    Y = rng.poisson(np.exp(C @ x[None] + d[:, None]))
    return {'C': C, 'd': d, 'tau': tau}, Y


def quad_laplace(par, K, Y):
    """(x* polished, f(x*), M = L^-T with H = L L^T, log Z_Laplace) in numpy under the Gram matrix K [1][T][T]"""
    C, d, Yf = par['C'], par['d'], Y.astype(np.float64)
    Kinv = np.linalg.inv(K)
    xs, f0, _ = orc.newton_mode(Yf, C, d, Kinv, xtol=1e-13)
    H = orc.nlp_hess(xs, Yf, C, d, Kinv)
    L = np.linalg.cholesky(0.5 * (H + H.T))
    M = np.linalg.solve(L, np.eye(H.shape[0])).T
    log_z = -f0 - 0.5 * (2.0 * np.log(np.diag(L)).sum() + np.linalg.slogdet(K[0])[1])
    return xs, f0, M, float(log_z)


def quad_correction(par, K, Y, nodes):
    """log Z - log Z_Laplace = log E_u exp(-[f(x* + M u) - f(x*) - |u|^2 / 2]), u ~ N(0, I_4), by the tensor Gauss-Hermite rule with `nodes` per
    dimension in the whitened coordinates of the Laplace posterior"""
    C, d, Yf = par['C'], par['d'], Y.astype(np.float64)
    T = Y.shape[1]
    Kinv = np.linalg.inv(K)
    xs, f0, M, _ = quad_laplace(par, K, Y)
    z, w = np.polynomial.hermite_e.hermegauss(nodes)
    lw1 = np.log(w) - 0.5 * np.log(2.0 * np.pi)
    rest = np.stack(np.meshgrid(*([z] * (T - 1)), indexing='ij'), -1).reshape(-1, T - 1)
    rest_lw = sum(np.meshgrid(*([lw1] * (T - 1)), indexing='ij')).reshape(-1)
    parts = []
    for z0, l0 in zip(z, lw1):                                   # (one slab of the grid per node of the first coordinate)
        U = np.concatenate([np.full((rest.shape[0], 1), z0), rest], axis=1)
        X = xs.reshape(-1)[None] + U @ M.T
        h = d[None, :, None] + C[None, :, 0, None] * X[:, None, :]
        f = np.exp(h).sum((1, 2)) - (Yf[None] * h).sum((1, 2)) + 0.5 * np.einsum('st,tu,su->s', X, Kinv[0], X)
        parts.append(-(f - f0) + 0.5 * (U * U).sum(1) + rest_lw + l0)
    e = np.concatenate(parts)
    m = e.max()
    return float(m + np.log(np.exp(e - m).sum()))


def quad_conditions(par, K, Y):
    """the two conditions of the truth test, host only: the rule with 16 and with 32 nodes per dimension agrees to 1e-6, and the correction is at
    least ten standard errors of a 4096-draw estimate (numpy draws from the numpy Laplace posterior) -> (correction, that standard error)"""
    c12, c24 = quad_correction(par, K, Y, 16), quad_correction(par, K, Y, 32)
    xs, _, M, _ = quad_laplace(par, K, Y)
    rng = np.random.default_rng(1)
    X = xs[None] + (rng.standard_normal((QUAD_S, xs.size)) @ M.T).reshape(QUAD_S, 1, -1)
    se = log_ratio_se(log_weights(par['C'], par['d'], xs, X))
    print('quadrature: correction %.7f (16 nodes), %.7f (32 nodes), difference %.1e (limit 1e-6); numpy se at S = %d: %.5f, |correction| / se = %.1f (at least 10)'
          % (c12, c24, abs(c12 - c24), QUAD_S, se, abs(c24) / se))
    assert abs(c12 - c24) <= 1e-6 and abs(c24) >= 10.0 * se
    return c24, se


def test_corrected_evidence_meets_the_quadrature_value_and_laplace_alone_does_not():
    from funs import _hip
    q, p, T = QUAD_SHAPE
    par, Y = quad_problem()
    ctx = _hip.Context(q, p, T, 1, BIN_MS)
    try:
        ctx.upload_counts(Y.astype(np.uint8)[None])
        ctx.set_option('laplace_evidence', 1)
        ctx.set_params(par['C'], par['d'], par['tau'])
        K = ctx.gram()                                           # the library's own Gram matrix
        corr, _ = quad_conditions(par, K, Y)                     # (host only, before any device output is looked at)
        _, _, _, log_z_np = quad_laplace(par, K, Y)
        _, _, status = ctx.estep_laplace()
        assert np.all(status == 0), status
        log_z = float(ctx.log_evidence()[0])
        out = ctx.importance_weights(None, n_samples=QUAD_S, seed=0, want=ALL)
        se = log_ratio_se(out['log_w'][0])
        truth = log_z_np + corr
        z = (log_z + out['log_ratio'][0] - truth) / se
        z_laplace = (log_z - truth) / se
        print('T = %d: log Z by quadrature %.6f, Laplace %.6f (numpy %.6f), log_ratio %.6f, se %.5f, ess / S %.3f; z-score of the corrected value %.2f '
              '(limit 5), of Laplace alone %.2f' % (T, truth, log_z, log_z_np, out['log_ratio'][0], se, out['ess'][0] / QUAD_S, z, z_laplace))
        assert abs(log_z - log_z_np) <= TOL
        assert abs(z) <= 5.0
        assert abs(z_laplace) > 5.0
    finally:
        ctx.close()


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------------------
def raw_call(ctx, n_samples=2, outputs=True, idx=LIST[:2]):
    """the C entry point without the binding's own checks -> (return code, message)"""
    from funs import _hip
    ii = np.ascontiguousarray(idx, dtype=np.int32)
    lr = np.empty(len(ii))
    rc = ctx.lib.pgpfa_importance_weights(ctx.h, len(ii), _hip.iptr(ii), int(n_samples), ct.c_ulonglong(0), _hip.dptr(lr) if outputs else None, None, None)
    return rc, ctx.lib.pgpfa_last_error().decode()


def test_refusals_name_what_is_wrong():
    from funs import _hip
    shape = SHAPES[0]
    q, p, T = shape
    ctx, par, live, _ = open_ctx(shape, 'plain', 2)
    try:
        rc, msg = raw_call(ctx, n_samples=0)
        assert rc != 0 and 'n_samples = 0' in msg
        rc, msg = raw_call(ctx, outputs=False)
        assert rc != 0 and 'no output asked for' in msg and 'log_ratio' in msg
        with pytest.raises(ValueError, match='n_samples'):
            ctx.importance_weights(LIST, n_samples=0)
        with pytest.raises(ValueError, match='unknown output'):
            ctx.importance_weights(LIST, want=('log_ratio', 'x'))
        with pytest.raises(ValueError, match='no output asked for'):
            ctx.importance_weights(LIST, want=())
        # a variational posterior: the identity is Laplace's
        ctx.dual_finalize(np.array([5], dtype=np.int32), np.full((1, q * T), 0.5))
        with pytest.raises(_hip.HipBackendError, match=r'trial 5 is variational.*Laplace'):
            ctx.importance_weights(LIST)
        assert ctx.importance_weights(np.array([2, 0], dtype=np.int32))['ess'].shape == (2,)       # the others still have theirs
        # an uploaded posterior: only its blocks are known
        ctx.set_posterior(np.array([1], dtype=np.int32), ctx.post_mean([1]), ctx.post_vsm([1]))
        with pytest.raises(_hip.HipBackendError, match='no posterior to sample for trial 1'):
            ctx.importance_weights(np.array([0, 1], dtype=np.int32))
    finally:
        ctx.close()
    Y = case(shape, 'plain')[1]
    fresh = _hip.Context(q, p, T, R8, BIN_MS)
    try:
        fresh.upload_counts(Y.astype(np.uint8))
        rc, msg = raw_call(fresh)
        assert rc != 0 and 'set_params has not been called' in msg
        fresh.set_params(par['C'], par['d'], par['tau'])
        rc, msg = raw_call(fresh)                                                                    # no E-step yet
        assert rc != 0 and 'no posterior to sample for trial 2' in msg
    finally:
        fresh.close()
    fresh = _hip.Context(q, p, T, R8, BIN_MS)
    try:
        fresh.set_params(par['C'], par['d'], par['tau'])
        rc, msg = raw_call(fresh)
        assert rc != 0 and 'spike counts have not been uploaded' in msg
    finally:
        fresh.close()


# ---- 6. Python layer ---------------------------------------------------------------------------------------------------------------------------------
def _c1(n):
    g = load_golden('c1_dataset.npz')
    Ys = [g['Y'][r].astype(np.float64) for r in range(n)]
    return {'C': g['init_C'].astype(np.float64), 'd': g['init_d'].astype(np.float64), 'tau': g['init_tau'].astype(np.float64)}, Ys, float(g['binSize'])


def test_importance_evidence_is_the_laplace_value_plus_the_log_ratio():
    import funs
    from funs import _hip, _session
    _session.drop_sessions()
    par, Ys, bin_ms = _c1(6)
    exp = Experiment(Ys, bin_ms)
    keys = ('logEvidence', 'laplace', 'logRatio', 'ess', 'logWeights')
    trials = [4, 0, 2, 4]
    res = funs.util.importanceEvidence(par, exp, trials=trials, nSamples=64, seed=3, want=keys)
    assert funs.inference.LAPLACE_EVIDENCE is False and sorted(res) == sorted(keys)
    sess, trial_idx = _session.session_for(exp, par['C'].shape[1])
    idx = np.ascontiguousarray(trial_idx[trials], dtype=np.int32)
    le = sess.ctx.log_evidence(idx)
    iw = sess.ctx.importance_weights(idx, n_samples=64, seed=3, want=ALL)
    assert np.array_equal(res['logEvidence'], le + iw['log_ratio']) and np.array_equal(res['laplace'], le)
    assert np.array_equal(res['logRatio'], iw['log_ratio']) and np.array_equal(res['ess'], iw['ess']) and np.array_equal(res['logWeights'], iw['log_w'])
    assert np.array_equal(res['logEvidence'][0], res['logEvidence'][3])
    default = funs.util.importanceEvidence(par, exp)
    assert sorted(default) == ['ess', 'logEvidence'] and default['ess'].shape == (6,)
    print('config 1, 6 trials: log Z_Laplace %s, correction %s, ess / 256 %s' % (np.round(le, 3), np.round(iw['log_ratio'], 4), np.round(default['ess'] / 256, 3)))
    # the weights of the draws posteriorSamples returns, same seed
    infRes, _, _ = funs.inference.laplace(exp, {k: v.copy() for k, v in par.items()})
    smp = funs.util.posteriorSamples(par, exp, infRes=infRes, trials=trials, nSamples=16, seed=3, want=('x', 'logWeights'))
    m = sess.ctx.post_mean(idx)
    assert smp['x'].shape == (4, 16) + m.shape[1:] and smp['logWeights'].shape == (4, 16)
    for i in range(len(trials)):
        lw, scale = log_weights(par['C'], par['d'], m[i], smp['x'][i], with_scale=True)
        assert np.all(np.abs(smp['logWeights'][i] - lw) <= TOL * np.maximum(1.0, scale))
    assert np.array_equal(smp['logWeights'], sess.ctx.importance_weights(idx, n_samples=16, seed=3, want=('log_w',))['log_w'])
    # an E-step that left no evidence: the library's error comes through
    with pytest.raises(_hip.HipBackendError, match='no log evidence for trial'):
        funs.util.importanceEvidence(par, exp, infRes=infRes)
    with pytest.raises(ValueError, match='unknown key'):
        funs.util.importanceEvidence(par, exp, want=('logZ',))
    with pytest.raises(ValueError, match='nSamples'):
        funs.util.importanceEvidence(par, exp, nSamples=0)
    _session.drop_sessions()


def test_cross_validation_by_the_corrected_evidence():
    import funs
    from funs import _session
    _session.drop_sessions()
    par, Ys, bin_ms = _c1(14)
    exp = Experiment(Ys, bin_ms)
    kw = dict(numTrainingTrials=10, numTestTrials=4, maxEMiter=2, score='evidence')
    np.random.seed(2)
    plain = funs.util.crossValidation(exp, maxXdim=1, **kw)
    np.random.seed(2)
    none = funs.util.crossValidation(exp, maxXdim=1, importance=None, **kw)
    assert plain.errs == none.errs and none.importance is None                                   # today's score, bit for bit
    np.random.seed(2)
    cv = funs.util.crossValidation(exp, maxXdim=2, importance=64, **kw)
    assert funs.inference.LAPLACE_EVIDENCE is False and len(cv.errs) == 2 and cv.importance == 64
    assert cv.errs[0] != plain.errs[0]
    test = Experiment(Ys[10:14], bin_ms)
    bins = sum(y.shape[1] for y in Ys[10:14])
    for i, fit in enumerate(cv.fits):
        _session.drop_sessions()
        funs.inference.LAPLACE_EVIDENCE = True
        try:
            infRes, _ = funs.inference.laplace(test, dict(fit.optimParams), returnOptimRes=False)
        finally:
            funs.inference.LAPLACE_EVIDENCE = False
        lr = infRes.session.ctx.importance_weights(None, n_samples=64, seed=0, want=('log_ratio',))['log_ratio']
        by_hand = -float(np.sum(infRes.log_evidence + lr)) / bins
        print('xdim %d: score %.10f, by hand %.10f, Laplace part %.10f' % (i + 1, cv.errs[i], by_hand, -float(np.sum(infRes.log_evidence)) / bins))
        assert cv.errs[i] == by_hand
    assert cv.optimXdim == int(np.argmin(cv.errs)) + 1
    got = cv.fits[0].importanceEvidence(nSamples=8, trials=[0, 1])
    assert sorted(got) == ['ess', 'logEvidence'] and got['ess'].shape == (2,) and cv.fits[0].importance is got
    with pytest.raises(ValueError, match="score='evidence'"):
        funs.util.crossValidation(exp, maxXdim=1, importance=8, numTrainingTrials=10, numTestTrials=4, maxEMiter=1)
    with pytest.raises(ValueError, match='importance = 0'):
        funs.util.crossValidation(exp, maxXdim=1, importance=0, **kw)
    _session.drop_sessions()
