"""The joint posterior of linear functionals of a trial's latents (pgpfa_posterior_functionals, Context.posterior_functionals,
util.posteriorFunctionals, util.posteriorEpochs):

    mean[j] = u_j . m,      cov[j][l] = u_j^T Sigma u_l,      var[j] = cov[j][j]

8 trials, both covariance engines and the sum-only plan of the low-rank one.  The error of a covariance is measured against the largest entry of
|U|^T |Sigma| |U| (the sums of absolute terms), that of a mean against |U| . |m|.  Limits: 1e-9 on the engine's own inputs - the dense engine
against the inverse of the dense Hessian at the device's mode, by numpy and by the downloaded post_cov (which is the dense engine's inverse whatever
the plan) -, 1e-8 for the low-rank engine against those exact dense inverses (its factors are truncated at lowrank_tol) and for every engine against
the independent dense models (ragged trials, the oracle's VIPostCov): the limits of test_gpu_posterior_cov_at.py for the same root through the same
products.  The numpy restatement's own spread is 2.0e-15 on the same inputs and 1.3e-13 for the low-rank root against the exact inverse
(test_cpu_posterior_functionals.py), more than ten times under both.  Reductions to the other queries, which hold the low-rank engine to its own
inputs: 1e-9 of the largest entry.  Results that must not depend on the call are compared with array_equal.  Every test prints its figures before
it asserts."""
import numpy as np
import pytest

from conftest import Experiment
from oracle import pgpfa_oracle as orc
from test_cpu_posterior_samples import problem
from test_gpu_posterior_at import CONFIG_IDS, CONFIGS, make_ctx
from test_gpu_posterior_cov_at import own_grid_covariance

pytestmark = pytest.mark.gpu

BIN_MS = 10.0
R8 = 8
SHAPES = [(20, 1, 21), (30, 3, 100), (40, 10, 176), (40, 32, 24)]
IDS = ['q%d-p%d-T%d' % s for s in SHAPES]
J_VALUES = (1, 16, 17, 65)
TOL_SAME, TOL_DENSE, TOL_ARITH = 1e-9, 1e-8, 1e-12
ALL = ('mean', 'var', 'cov')


def tag(config):
    return CONFIG_IDS[CONFIGS.index(config)]


def dense_weights(J, p, T, seed):
    return np.random.default_rng(1000 * T + 10 * J + seed).standard_normal((J, p, T))


def window_weights(J, p, T, seed):
    """sparse windows: functional j averages one latent over a short run of bins, with a sign"""
    rng = np.random.default_rng(77 * T + J + seed)
    U = np.zeros((J, p, T))
    for j in range(J):
        a = int(rng.integers(0, T))
        b = int(rng.integers(a + 1, min(a + 9, T) + 1))
        U[j, int(rng.integers(0, p)), a:b] = (1.0 if j % 3 else -1.0) / (b - a)
    return U


def numpy_functionals(U, m, Sigma):
    """mean (J), cov (J, J) and the scales their errors are measured against, from U (J, p, T), m (p, T) and Sigma (p T, p T)"""
    Uf = U.reshape(U.shape[0], -1)
    cov = Uf @ Sigma @ Uf.T
    return Uf @ m.reshape(-1), 0.5 * (cov + cov.T), float(np.max(np.abs(Uf) @ np.abs(m.reshape(-1)))), float(np.max(np.abs(Uf) @ np.abs(Sigma) @ np.abs(Uf).T))


def errs(got, i, U, m, Sigma):
    mean, cov, s_m, s_c = numpy_functionals(U, m, Sigma)
    out = {}
    if 'mean' in got:
        out['mean'] = float(np.max(np.abs(got['mean'][i] - mean)) / s_m)
    if 'cov' in got:
        out['cov'] = float(np.max(np.abs(got['cov'][i] - cov)) / s_c)
    if 'var' in got:
        out['var'] = float(np.max(np.abs(got['var'][i] - np.diag(cov))) / s_c)
    return out


def same_bits(a, b, keys=None):
    return all(np.array_equal(a[k], b[k]) for k in (keys or a))


# ---- 1. plain FP64 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('config', CONFIGS, ids=CONFIG_IDS)
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_against_plain_fp64_symmetry_definiteness_and_each_output_alone(shape, config):
    q, p, T = shape
    ctx, par, _, live = make_ctx(shape, config)
    try:
        m = ctx.post_mean()
        trials = np.array([5, 0], dtype=np.int32)
        own = [ctx.post_cov(r) for r in trials]                                            # the dense engine's inverse of the Hessian, whatever the plan
        exact = [own_grid_covariance(par, m[r], live[r], T) for r in trials]              # numpy's inverse of the dense Hessian at the device's mode
        tol = TOL_SAME if config[0] == 1 else TOL_DENSE              # the low-rank root against an exact dense inverse: both references are one
        cases = [(J, 'dense', dense_weights(J, p, T, 0)) for J in J_VALUES] + [(17, 'windows', window_weights(17, p, T, 0))]
        for J, kind, U in cases:
            got = ctx.posterior_functionals(U, trials, want=ALL)
            assert got['mean'].shape == (2, J) and got['var'].shape == (2, J) and got['cov'].shape == (2, J, J)
            e_own = [errs(got, i, U, m[r], own[i]) for i, r in enumerate(trials)]
            e_exact = [errs(got, i, U, m[r], exact[i]) for i, r in enumerate(trials)]
            ev = np.linalg.eigvalsh(got['cov'])
            e_eig = float(np.min(ev[:, 0] / ev[:, -1]))
            worst_own = max(max(e.values()) for e in e_own)
            worst_exact = max(max(e.values()) for e in e_exact)
            print('q=%d p=%d T=%d %s J=%d %s weights: against post_cov %.2e, against the dense inverse in numpy %.2e of the sums of absolute terms (limit %.0e); '
                  'smallest / largest eigenvalue %.2e (limit -1e-12)' % (q, p, T, tag(config), J, kind, worst_own, worst_exact, tol, e_eig))
            assert worst_own <= tol and worst_exact <= tol
            assert np.array_equal(got['cov'], got['cov'].transpose(0, 2, 1))
            assert e_eig >= -1e-12
            assert np.array_equal(got['var'], np.diagonal(got['cov'], axis1=1, axis2=2)) and np.all(got['var'] >= 0.0)
            if J == 17:                                              # each output asked for alone: the same bits; var alone takes the diagonal-only form
                for k in ALL:
                    assert np.array_equal(ctx.posterior_functionals(U, trials, want=(k,))[k], got[k]), k
                assert same_bits(ctx.posterior_functionals(U, trials, want=('mean', 'var')), got, ('mean', 'var'))
    finally:
        ctx.close()


# ---- 2. reductions to the existing queries ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('config', CONFIGS, ids=CONFIG_IDS)
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_one_hot_weights_give_post_vsm_and_post_vsmgp(shape, config):
    q, p, T = shape
    ctx, par, _, _ = make_ctx(shape, config)
    try:
        trials = np.array([2, 7], dtype=np.int32)
        t0, t1, k0 = T // 3, T - 1, p - 1
        U = np.zeros((p + 2, p, T))
        U[np.arange(p), np.arange(p), t0] = 1.0                      # all latents at bin t0
        U[p, k0, t0] = 1.0                                          # latent k0 at two bins
        U[p + 1, k0, t1] = 1.0
        got = ctx.posterior_functionals(U, trials, want=ALL)
        blocks = ctx.post_vsmgp(trials)                              # (under the sum-only plan this rebuilds the blocks)
        vsm, m = ctx.post_vsm(trials), ctx.post_mean(trials)
        e_vsm = float(np.max(np.abs(got['cov'][:, :p, :p] - vsm[:, t0])) / np.max(np.abs(vsm)))
        gp = np.stack([blocks[:, t0, t0, k0], blocks[:, t0, t1, k0], blocks[:, t1, t1, k0]])
        mine = np.stack([got['cov'][:, p, p], got['cov'][:, p, p + 1], got['cov'][:, p + 1, p + 1]])
        e_gp = float(np.max(np.abs(mine - gp)) / np.max(np.abs(blocks)))
        exact_mean = bool(np.array_equal(got['mean'][:, :p], m[:, :, t0]) and np.array_equal(got['mean'][:, p + 1], m[:, k0, t1]))
        print('q=%d p=%d T=%d %s: one-hot weights, cov against post_vsm[%d] %.2e, against post_vsmGP[%d][%d][%d] %.2e of the largest entry (limit %.0e); '
              'mean is post_mean to the bit: %s' % (q, p, T, tag(config), t0, e_vsm, t0, t1, k0, e_gp, TOL_SAME, exact_mean))
        assert e_vsm <= TOL_SAME and e_gp <= TOL_SAME and exact_mean
    finally:
        ctx.close()


# ---- 3. ragged trials and both observation tables ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('config', CONFIGS, ids=CONFIG_IDS)
def test_ragged_trials_under_both_observation_tables_and_the_forecast(config):
    shape = SHAPES[1]
    q, p, T = shape
    lens = np.array([100, 73, 100, 41, 88, 64, 100, 17], dtype=np.int32)
    rng = np.random.default_rng(7)
    observed = np.ones((R8, q), dtype=np.uint8)
    observed[1, :5] = 0
    observed[2, q - 4:] = 0
    observed[6, 3::4] = 0
    bins = (rng.random((R8, q, T)) > 0.2).astype(np.uint8)
    bins[0] = 1
    ctx, par, _, live = make_ctx(shape, config, lens=lens, observed=observed, bins=bins)
    try:
        m = ctx.post_mean()
        J = 17
        U = np.stack([np.concatenate([dense_weights(J - 4, p, T, r), window_weights(4, p, T, r)]) for r in range(R8)])
        inside = U * (np.arange(T)[None, None, None, :] < lens[:, None, None, None])
        got_in, got_all = ctx.posterior_functionals(inside, want=ALL), ctx.posterior_functionals(U, want=ALL)
        worst_in = worst_all = 0.0
        for r in range(R8):
            L = int(lens[r])
            e_in = errs(got_in, r, inside[r][:, :, :L], m[r][:, :L], own_grid_covariance(par, m[r], live[r], L))     # the trial's own T_r-bin model
            e_all = errs(got_all, r, U[r], m[r], own_grid_covariance(par, m[r], live[r], T))                         # the model extended by the padded bins
            worst_in, worst_all = max(worst_in, max(e_in.values())), max(worst_all, max(e_all.values()))
            print('%s trial %d (%d bins): weights inside T_r against the own-grid model %s; reaching into the padded bins against the extended model %s '
                  '(limit %.0e)' % (tag(config), r, L, {k: '%.2e' % v for k, v in e_in.items()}, {k: '%.2e' % v for k, v in e_all.items()}, TOL_DENSE))
        assert worst_in <= TOL_DENSE and worst_all <= TOL_DENSE
        # one-hot weights at a padded bin of a short trial: posterior_cov_at and posterior_at at that grid time
        short, t_pad = np.array([7, 3], dtype=np.int32), 60
        hot = np.zeros((p, p, T))
        hot[np.arange(p), np.arange(p), t_pad] = 1.0
        mine = ctx.posterior_functionals(hot, short, want=('mean', 'cov'))
        at = ctx.posterior_cov_at(np.array([t_pad * BIN_MS]), short, want=('cov',))['cov'][:, 0]
        at_mean = ctx.posterior_at(np.array([t_pad * BIN_MS]), short, want=('mean',))['mean'][:, :, 0]
        e_cov = float(np.max(np.abs(mine['cov'] - at)) / np.max(np.abs(at)))
        e_mean = float(np.max(np.abs(mine['mean'] - at_mean)) / np.max(np.abs(m)))
        print('%s: one-hot at padded bin %d of trials %s: cov against posterior_cov_at %.2e, mean against posterior_at %.2e (limit %.0e)'
              % (tag(config), t_pad, short.tolist(), e_cov, e_mean, TOL_SAME))
        assert e_cov <= TOL_SAME and e_mean <= TOL_SAME
    finally:
        ctx.close()


# ---- 4. variational posteriors ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('engine', [1, 2], ids=['dense', 'lowrank'])
@pytest.mark.parametrize('which', ['var_toy', 'q40-p10-T64'])
def test_variational_posterior_against_the_oracle_at_the_kept_lambda(which, engine):
    from funs import _hip
    from test_gpu_posterior_at import _var_problem
    par, Y, binSize = _var_problem(which)
    assert binSize == BIN_MS
    R, q, T = Y.shape
    p = par['C'].shape[1]
    C_big, _ = orc.make_Cd_big(par['C'], par['d'], T)
    Kinv_big = np.linalg.inv(orc.make_K_big(orc.make_K(par['tau'], T, binSize)))
    ctx = _hip.Context(q, p, T, R, binSize)
    try:
        ctx.upload_counts(Y.astype(np.uint16 if Y.max() > 255 else np.uint8))
        ctx.set_option('cov_mode', engine)
        ctx.set_option('dual_lowrank', int(engine == 2))
        ctx.set_params(par['C'], par['d'], par['tau'])
        _, _, _, status, lam = ctx.dual_fixed_point(None, None, want_lam=True)
        assert np.all(status == 0), status
        ctx.dual_finalize(None, None)
        U = np.concatenate([dense_weights(13, p, T, 4), window_weights(4, p, T, 4)])
        got = ctx.posterior_functionals(U, want=ALL)
        m = ctx.post_mean()
        worst = 0.0
        for r in range(R):
            Sigma, _ = orc.vi_post_cov(Kinv_big, C_big, lam[r])
            e = errs(got, r, U, m[r], Sigma)
            worst = max(worst, max(e.values()))
            print('%s engine %d trial %d: VIPostCov at the kept lambda %s (limit %.0e)' % (which, engine, r, {k: '%.2e' % v for k, v in e.items()}, TOL_DENSE))
        assert worst <= TOL_DENSE
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
        U = dense_weights(3, p, T, 0)
        with pytest.raises(_hip.HipBackendError, match='variational posterior of trial 1 covers 23 of 40 bins.*pgpfa_posterior_functionals refuses'):
            ctx.posterior_functionals(U)
        assert ctx.posterior_functionals(U, np.array([0, 2], dtype=np.int32), want=('cov',))['cov'].shape == (2, 3, 3)      # the full-length ones are served
    finally:
        ctx.close()


# ---- 5. bits do not depend on the call ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('config', CONFIGS, ids=CONFIG_IDS)
@pytest.mark.parametrize('shape', [SHAPES[1], SHAPES[3]], ids=[IDS[1], IDS[3]])
def test_per_trial_weights_lists_chunks_and_blocks_give_the_same_bits(shape, config):
    q, p, T = shape
    ctx, par, _, _ = make_ctx(shape, config, R=4)
    try:
        J = 65
        sets = np.stack([dense_weights(J, p, T, 10 + r) for r in range(4)])
        per = ctx.posterior_functionals(sets, want=ALL)
        singles = [bool(same_bits(ctx.posterior_functionals(sets[r], np.array([r], dtype=np.int32), want=ALL), {k: per[k][r:r + 1] for k in ALL})) for r in range(4)]
        print('q=%d p=%d T=%d %s: (n, J, p, T) call against one shared-weights call per trial, same bits %s' % (q, p, T, tag(config), singles))
        assert all(singles)
        shared = ctx.posterior_functionals(sets[0], want=ALL)
        diag = ctx.posterior_functionals(sets[0], want=('mean', 'var'))
        assert same_bits(diag, shared, ('mean', 'var'))
        order = np.array([3, 0, 2, 1, 0], dtype=np.int32)
        seen = []
        for chunk, block in ((1, 0), (3, 0), (0, 16), (0, 32), (3, 16), (0, 0)):
            ctx.set_option('func_chunk_trials', chunk)
            ctx.set_option('func_block_cols', block)
            a = ctx.posterior_functionals(sets, want=ALL)
            b = ctx.posterior_functionals(sets[order], order, want=ALL)
            c = ctx.posterior_functionals(sets[0], order, want=ALL)
            d = ctx.posterior_functionals(sets[0], order, want=('mean', 'var'))          # the diagonal-only form, its staging one block wide
            seen.append((chunk, block, same_bits(a, per), all(np.array_equal(b[k], per[k][order]) for k in ALL),
                         all(np.array_equal(c[k], shared[k][order]) for k in ALL), all(np.array_equal(d[k], shared[k][order]) for k in ('mean', 'var'))))
        print('q=%d p=%d T=%d %s: (func_chunk_trials, func_block_cols, all trials, list %s per trial, shared weights, var alone) %s'
              % (q, p, T, tag(config), order.tolist(), seen))
        assert all(all(x[2:]) for x in seen)
        assert np.array_equal(b['cov'][1], b['cov'][4])               # trial 0, listed twice
    finally:
        ctx.close()


@pytest.mark.parametrize('config', CONFIGS, ids=CONFIG_IDS)
def test_a_list_across_two_parameter_snapshots_gives_the_bits_of_one_call_per_trial(config):
    """four trials, {0, 1} through an E-step at parameters A and {2, 3} through one at B: one call over [3, 0, 2, 1, 0] walks two snapshot groups and
    scatters by list position (the construction of test_gpu_posterior_cov_at.py)"""
    from funs import _hip
    shape = SHAPES[0]
    q, p, T = shape
    par, Y, _ = problem(shape, R=4)
    mixed = np.array([3, 0, 2, 1, 0], dtype=np.int32)
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
        sets = np.stack([dense_weights(17, p, T, 20 + i) for i in range(mixed.size)])
        before = [ctx.post_mean(), ctx.post_vsm(), ctx.gram()]
        one = ctx.posterior_functionals(sets, mixed, want=ALL)
        after = [ctx.post_mean(), ctx.post_vsm(), ctx.gram()]
        same = [bool(same_bits(ctx.posterior_functionals(sets[i], mixed[i:i + 1], want=ALL), {k: one[k][i:i + 1] for k in ALL})) for i in range(mixed.size)]
        kept = [bool(np.array_equal(a, b)) for a, b in zip(before, after)]
        # the two groups were evaluated under their own parameters: trial 3 against the covariance of its own E-step
        e3 = errs(one, 0, sets[0], before[0][3], ctx.post_cov(3))
        tol = TOL_SAME if config[0] == 1 else TOL_DENSE              # (post_cov is the dense engine's inverse, whatever the plan)
        print('%s: list %s against one call per entry %s; post_mean, post_vsm, Gram unchanged %s; trial 3 against its own post_cov %s (limit %.0e)'
              % (tag(config), mixed.tolist(), same, kept, {k: '%.2e' % v for k, v in e3.items()}, tol))
        assert all(same) and all(kept) and max(e3.values()) <= tol
    finally:
        ctx.close()


# ---- 6. no state is touched -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('config', CONFIGS, ids=CONFIG_IDS)
def test_no_state_is_touched(config):
    shape = SHAPES[1]
    q, p, T = shape
    ctx, par, _, _ = make_ctx(shape, config, evidence=True)
    try:
        U = dense_weights(17, p, T, 3)
        pick = np.array([0, 3], dtype=np.int32)

        def state():
            blocks = ctx.post_vsmgp(pick)        # (first: under the sum-only plan this download rebuilds the blocks and rewrites post_vsm of these trials)
            return [ctx.post_mean(), ctx.post_vsm(), blocks, ctx.gram(), ctx.log_evidence()]
        before = state()
        first = ctx.posterior_functionals(U, want=ALL)
        after = state()
        again = ctx.posterior_functionals(U, want=ALL)
        same = [bool(np.array_equal(a, b)) for a, b in zip(before, after)]
        print('%s: post_mean, post_vsm, post_vsmGP, Gram, log evidence unchanged by the call: %s; the call repeats its bits: %s' % (tag(config), same, same_bits(first, again)))
        assert all(same) and same_bits(first, again)
    finally:
        ctx.close()


# ---- 7. refusals and the limit on J -------------------------------------------------------------------------------------------------------------------
def test_every_refusal_names_what_is_wrong_and_var_walks_past_the_limit_of_cov():
    from funs import _hip
    shape = (20, 3, 40)
    q, p, T = shape
    par, Y, _ = problem(shape, R=4)
    ctx = _hip.Context(q, p, T, 4, BIN_MS)
    try:
        ctx.upload_counts(Y.astype(np.uint8))
        U = dense_weights(3, p, T, 0)
        with pytest.raises(_hip.HipBackendError, match='set_params has not been called'):
            ctx.posterior_functionals(U)
        # a weight that is not finite is refused before the parameters are even looked at: no device call has been made
        bad = U.copy()
        bad[2, 1, 7] = np.nan
        with pytest.raises(_hip.HipBackendError, match='weight of functional 2 at latent 1, bin 7 is not finite'):
            ctx.posterior_functionals(bad)
        ctx.set_params(par['C'], par['d'], par['tau'])
        with pytest.raises(_hip.HipBackendError, match='no posterior for trial 0'):
            ctx.posterior_functionals(U)
        ctx.estep_laplace(np.array([0, 1, 2], dtype=np.int32))
        with pytest.raises(_hip.HipBackendError, match='no posterior for trial 3'):
            ctx.posterior_functionals(U)
        idx = np.array([2, 0], dtype=np.int32)
        assert ctx.posterior_functionals(U, idx, want=('cov',))['cov'].shape == (2, 3, 3)
        with pytest.raises(_hip.HipBackendError, match='J = 0'):
            ctx.posterior_functionals(np.zeros((0, p, T)), idx)
        out = np.zeros(2 * 3)
        assert ctx.lib.pgpfa_posterior_functionals(ctx.h, 2, _hip.iptr(idx), 3, _hip.dptr(U), 0, None, None, None) != 0
        assert 'no output asked for' in ctx.lib.pgpfa_last_error().decode()
        assert ctx.lib.pgpfa_posterior_functionals(ctx.h, 2, _hip.iptr(idx), 3, None, 0, _hip.dptr(out), None, None) != 0
        assert 'weights is NULL' in ctx.lib.pgpfa_last_error().decode()
        assert ctx.lib.pgpfa_posterior_functionals(None, 2, _hip.iptr(idx), 3, _hip.dptr(U), 0, _hip.dptr(out), None, None) != 0
        assert 'null context' in ctx.lib.pgpfa_last_error().decode()
        sets = np.stack([U, U])
        sets[1, 0, 2, 39] = np.inf
        with pytest.raises(_hip.HipBackendError, match=r'weight of functional 0 at latent 2, bin 39 of list entry 1 \(trial 0\) is not finite'):
            ctx.posterior_functionals(sets, idx)
        with pytest.raises(ValueError, match='weights must have shape'):
            ctx.posterior_functionals(np.zeros((3, 3, p, T)), idx)
        with pytest.raises(ValueError, match='weights must have shape'):
            ctx.posterior_functionals(np.zeros((3, p, T + 1)), idx)
        with pytest.raises(ValueError, match='unknown output'):
            ctx.posterior_functionals(U, idx, want=('mean', 'rate'))
        with pytest.raises(ValueError, match='no output asked for'):
            ctx.posterior_functionals(U, idx, want=())
        for key, value in (('func_chunk_trials', -1), ('func_block_cols', 24), ('func_block_cols', -16)):
            with pytest.raises(_hip.HipBackendError, match=key):
                ctx.set_option(key, value)
        # the J x J plane is given up to 1024 functionals; var alone walks any J in blocks
        big = dense_weights(1040, p, T, 1)
        with pytest.raises(_hip.HipBackendError, match='J = 1025 with cov asked for.*at most 1024'):
            ctx.posterior_functionals(big[:1025], idx, want=('cov',))
        ctx.set_option('func_block_cols', 256)                       # (five blocks, the last one short)
        walked = ctx.posterior_functionals(big, idx, want=('mean', 'var'))
        ctx.set_option('func_block_cols', 0)
        whole = ctx.posterior_functionals(big, idx, want=('mean', 'var'))
        m = ctx.post_mean()
        e = [errs(walked, i, big, m[r], ctx.post_cov(r)) for i, r in enumerate(idx)]
        head = ctx.posterior_functionals(big[:1024], idx, want=('cov',))['cov']
        tol = TOL_DENSE if ctx.info('plan_lowrank') else TOL_SAME     # (post_cov is the dense engine's inverse, whatever the plan)
        print('J = 1040, var and mean alone: against numpy on post_cov %s (limit %.0e); blocks of 256 against one block, same bits %s; the first 1024 against '
              "the diagonal of their plane, same bits %s" % (e, tol, same_bits(walked, whole), np.array_equal(np.diagonal(head, axis1=1, axis2=2), whole['var'][:, :1024])))
        assert max(max(x.values()) for x in e) <= tol and same_bits(walked, whole)
        assert np.array_equal(np.diagonal(head, axis1=1, axis2=2), whole['var'][:, :1024])
        # an uploaded posterior has blocks, no square root
        ctx.set_posterior(np.array([3], dtype=np.int32), np.zeros((1, p, T)), np.tile(np.eye(p), (1, T, 1, 1)), np.tile(np.eye(T)[:, :, None], (1, 1, 1, p)))
        with pytest.raises(_hip.HipBackendError, match='posterior of trial 3 was uploaded.*no square root'):
            ctx.posterior_functionals(U, np.array([0, 3], dtype=np.int32))
        # an asynchronous timescale pass in flight
        ctx.mstep_precomp()
        Q = np.log(1.0 / (par['tau'] * 100.0) ** 2)[None, :] + np.array([0.0, 0.1])[:, None]
        ctx.mstep_tau_costgrad_multi_begin(Q)
        with pytest.raises(_hip.HipBackendError, match='timescale pass is in flight'):
            ctx.posterior_functionals(U, idx)
        ctx.mstep_tau_costgrad_multi_end()
        assert ctx.posterior_functionals(U, idx, want=('var',))['var'].shape == (2, 3)
        # counts uploaded after the E-step: the posterior is gone
        ctx.upload_counts(Y.astype(np.uint8))
        with pytest.raises(_hip.HipBackendError, match='no posterior for trial 2'):
            ctx.posterior_functionals(U, idx)
    finally:
        ctx.close()


# ---- 8. the Python surface ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def funs_mod():
    import funs
    from funs import _session
    _session.drop_sessions()
    yield funs
    _session.drop_sessions()


def test_util_posterior_epochs_with_align_contrasts_and_conditions_on_a_ragged_config1_experiment(funs_mod):
    util, inference = funs_mod.util, funs_mod.inference
    shape = (30, 3, 100)
    q, p, T = shape
    R = 6
    par, Y, _ = problem(shape, R=R)
    lens = np.array([T, T - 1, 60, 70, T, 80])
    exp = Experiment([Y[r][:, :lens[r]].astype(np.float64) for r in range(R)], BIN_MS)
    params = {k: np.array(v, dtype=np.float64) for k, v in par.items()}
    infRes, _ = inference.laplace(exp, {k: v.copy() for k, v in params.items()}, returnOptimRes=False)
    epochs = [(-200.0, -100.0), (0.0, 150.0), (150.0, 155.0)]             # relative to the event: 10, 15 and 1 bins
    event = np.array([300.0, 250.0, 200.0, 400.0, 500.0, 380.0])
    contrasts = [(0, 1), (1, 2)]
    cond = np.array([4, 9, 4, 9, 4, 9])
    keys = ('mean', 'var', 'lower', 'upper', 'cov', 'contrast', 'contrastVar', 'contrastLower', 'contrastUpper', 'eta', 'etaVar', 'etaLower', 'etaUpper')
    out = util.posteriorEpochs(params, exp, epochs, infRes=infRes, align=event, contrasts=contrasts, conditions=cond, level=0.9, want=keys)
    E, nC = len(epochs), len(contrasts)
    assert out['mean'].shape == (R, E, p) and out['cov'].shape == (R, E * p, E * p) and out['contrast'].shape == (R, nC, p) and out['eta'].shape == (R, E, q)
    z = util._band_z(0.9)
    cov = out['cov'].reshape(R, E, p, E, p)
    var = np.stack([[np.diag(cov[r, e, :, e, :]) for e in range(E)] for r in range(R)])
    assert np.array_equal(out['var'], var)
    assert np.array_equal(out['lower'], out['mean'] - z * np.sqrt(out['var'])) and np.array_equal(out['upper'], out['mean'] + z * np.sqrt(out['var']))
    # the means are those of the windows, straight from the resident posterior mean
    sess, _ = funs_mod._session.session_for(exp, p)
    m = sess.ctx.post_mean()
    worst = 0.0
    for r in range(R):
        for e, (a, b) in enumerate(epochs):
            tj = np.arange(T) * BIN_MS
            inb = (tj >= a + event[r]) & (tj < b + event[r])
            assert inb.sum() == (10, 15, 1)[e]
            worst = max(worst, float(np.max(np.abs(out['mean'][r, e] - m[r][:, inb].mean(axis=1)) / np.abs(m[r][:, inb]).mean(axis=1))))
    # contrasts and eta from the call's own mean and cov
    C, d = params['C'], params['d'].reshape(-1)
    e_c = e_cv = e_eta = e_ev = 0.0
    for r in range(R):
        for i, (a, b) in enumerate(contrasts):
            ref = out['mean'][r, b] - out['mean'][r, a]
            e_c = max(e_c, float(np.max(np.abs(out['contrast'][r, i] - ref) / (np.abs(out['mean'][r, b]) + np.abs(out['mean'][r, a])))))
            vab = np.array([cov[r, a, k, a, k] + cov[r, b, k, b, k] - 2.0 * cov[r, a, k, b, k] for k in range(p)])
            aab = np.array([cov[r, a, k, a, k] + cov[r, b, k, b, k] + 2.0 * abs(cov[r, a, k, b, k]) for k in range(p)])
            e_cv = max(e_cv, float(np.max(np.abs(out['contrastVar'][r, i] - vab) / aab)))
        for e in range(E):
            eta = d + C @ out['mean'][r, e]
            e_eta = max(e_eta, float(np.max(np.abs(out['eta'][r, e] - eta) / (np.abs(d) + np.abs(C) @ np.abs(out['mean'][r, e])))))
            blk = cov[r, e, :, e, :]
            ev = np.einsum('ni,ij,nj->n', C, blk, C)
            e_ev = max(e_ev, float(np.max(np.abs(out['etaVar'][r, e] - ev) / np.einsum('ni,ij,nj->n', np.abs(C), np.abs(blk), np.abs(C)))))
    print('util.posteriorEpochs on ragged config 1: epoch means against window means of post_mean %.2e; contrast %.2e, its variance %.2e, eta %.2e, its '
          'variance %.2e against numpy on the call\'s own mean / cov, of the sums of absolute terms (limit %.0e)' % (worst, e_c, e_cv, e_eta, e_ev, TOL_ARITH))
    assert max(worst, e_c, e_cv, e_eta, e_ev) <= TOL_ARITH
    assert np.array_equal(out['contrastLower'], out['contrast'] - z * np.sqrt(out['contrastVar']))
    assert np.array_equal(out['contrastUpper'], out['contrast'] + z * np.sqrt(out['contrastVar']))
    assert np.array_equal(out['etaLower'], out['eta'] - z * np.sqrt(out['etaVar'])) and np.array_equal(out['etaUpper'], out['eta'] + z * np.sqrt(out['etaVar']))
    assert out['condition_labels'].tolist() == [4, 9] and out['condition_count'].tolist() == [3, 3]
    for g, label in enumerate((4, 9)):
        members = np.flatnonzero(cond == label)
        assert np.allclose(out['condition_mean'][g], out['mean'][members].mean(axis=0), rtol=1e-13, atol=0.0)
        assert np.allclose(out['condition_contrast'][g], out['contrast'][members].mean(axis=0), rtol=1e-13, atol=0.0)
    # a window that passes a trial's own bins is refused by name unless forecast=True
    with pytest.raises(ValueError, match=r'passes the 60 bins of trial 2'):
        util.posteriorEpochs(params, exp, [(0.0, 450.0)], infRes=infRes, align=event)
    fc = util.posteriorEpochs(params, exp, [(0.0, 450.0)], infRes=infRes, align=event[[2]], forecast=True, trials=[2], want=('mean', 'var'))
    assert fc['mean'].shape == (1, 1, p) and np.all(fc['var'] > 0.0)
    # posteriorFunctionals: the same numbers from explicit weights
    W = util._epoch_windows(epochs, BIN_MS, T, lens, np.arange(R), event, False)
    direct = util.posteriorFunctionals(params, exp, util._latent_functionals(W, p), infRes=infRes, level=0.9, want=('mean', 'sd', 'lower', 'upper', 'cov'))
    assert np.array_equal(direct['mean'].reshape(R, E, p), out['mean']) and np.array_equal(direct['cov'], out['cov'])
    assert np.array_equal(direct['lower'], direct['mean'] - z * direct['sd'])


def test_fit_posterior_epochs_after_a_two_iteration_fit(funs_mod):
    shape = (30, 3, 100)
    q, p, T = shape
    par, Y, _ = problem(shape, R=R8)
    exp = Experiment([Y[r].astype(np.float64) for r in range(R8)], BIN_MS)
    init = {k: np.array(v, dtype=np.float64) for k, v in par.items()}
    fit = funs_mod.engine.PPGPFAfit(exp, initParams=init, EMmode='Batch', maxEMiter=2, CdOptimMethod='newton', quiet=True)
    out = fit.posteriorEpochs(epochs=[(0.0, 200.0), (500.0, 990.0)], contrasts=[(0, 1)], conditions=np.arange(R8) % 2)
    assert fit.epochs is out and out['mean'].shape == (R8, 2, p) and out['contrast'].shape == (R8, 1, p) and out['condition_mean'].shape == (2, 2, p)
    assert np.all(out['lower'] <= out['mean']) and np.all(out['mean'] <= out['upper']) and np.all(out['contrastLower'] <= out['contrastUpper'])
    assert fit.infRes['post_mean'][3].shape == (p, T)                  # kept on the host before the E-step superseded it
    from funs import _session
    sess, _ = _session.session_for(exp, p)
    m = sess.ctx.post_mean()
    err = float(np.max(np.abs(out['mean'][:, 0] - m[:, :, :20].mean(axis=2)) / np.abs(m[:, :, :20]).mean(axis=2)))
    print('PPGPFAfit.posteriorEpochs: epoch means against window means of the resident post_mean %.2e (limit %.0e)' % (err, TOL_ARITH))
    assert err <= TOL_ARITH
    fun = fit.posteriorFunctionals(weights=np.ones((1, p, T)) / (p * T), want=('mean', 'var'))
    assert fit.functionals is fun and fun['mean'].shape == (R8, 1) and np.all(fun['var'] > 0.0)
