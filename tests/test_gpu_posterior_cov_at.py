"""The cross-latent posterior covariance and the log-rate moments at arbitrary time points (pgpfa_posterior_cov_at, Context.posterior_cov_at,
util.posteriorRatesAt, util.posteriorAt(want=('cov',))):

    Cov(x(s))[k][l] = a_k(s)^T Sigma_kl a_l(s) + delta_kl (1 - a_k(s) . kx_k(s)),   a_k(s) = K_k^-1 kx_k(s)
    eta_n(s) = d_n + c_n . mean(s),   var_n(s) = c_n^T Cov(x(s)) c_n

8 trials, both covariance engines and the sum-only plan of the low-rank one.  Tolerances: 1e-9 of the largest entry against the same formula in numpy
on the downloaded post_cov (the restatement's two evaluation orders differ by 5.5e-13, test_cpu_posterior_cov_at.py: ten times that stays below 1e-9,
the "same inputs" tolerance of test_gpu_posterior_at.py); the same against post_vsm, posterior_at and posterior_rates on the grid, which go through
other kernels; 1e-8 against independent dense FP64 models (TOL_DENSE, the project's tolerance for blocks against dense FP64); 1e-12 in the far field;
1e-12 of the sums of absolute terms for eta / var against numpy on the call's own mean and cov (the bound of test_gpu_posterior_rates.py: the same
kernel).  Results that must not depend on the call are compared with array_equal.  Every test prints its figures before it asserts."""
import numpy as np
import pytest

from conftest import Experiment
from oracle import pgpfa_oracle as orc
from test_cpu_posterior_cov_at import extended_blocks, numpy_cov_at
from test_cpu_posterior_samples import problem
from test_gpu_posterior_at import CONFIG_IDS, CONFIGS, cross, make_ctx, make_times

pytestmark = pytest.mark.gpu

BIN_MS = 10.0
R8 = 8
SHAPES = [(20, 1, 21), (30, 3, 100), (40, 10, 176), (35, 12, 64), (50, 20, 48), (40, 32, 24)]
IDS = ['q%d-p%d-T%d' % s for s in SHAPES]
S_VALUES = (1, 16, 17, 65)
TOL_SAME, TOL_DENSE, TOL_FAR, TOL_RATES = 1e-9, 1e-8, 1e-12, 1e-12
ALL = ('mean', 'cov', 'eta', 'var')


def tag(config):
    return CONFIG_IDS[CONFIGS.index(config)]


def numpy_mean_at(tau, m, s):
    """mean (p, S) = a_k(s) . m_k from m (p, L), through np.linalg.solve"""
    p, L = m.shape
    K = orc.make_K(tau, L, BIN_MS)
    return np.stack([np.linalg.solve(K[k], cross(tau[k], s, L)).T @ m[k] for k in range(p)])


def numpy_rates_at(C, d, mean, cov):
    """eta, var (n, q, S) from mean (n, p, S) and cov (n, S, p, p), and the sums of absolute terms their tolerance scales with"""
    eta = d[None, :, None] + np.einsum('nk,rks->rns', C, mean)
    var = np.einsum('ni,rsij,nj->rns', C, cov, C)
    a_eta = np.abs(d)[None, :, None] + np.einsum('nk,rks->rns', np.abs(C), np.abs(mean))
    a_var = np.einsum('ni,rsij,nj->rns', np.abs(C), np.abs(cov), np.abs(C))
    return eta, var, a_eta, a_var


def rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def same_bits(a, b, keys=None):
    return all(np.array_equal(a[k], b[k]) for k in (keys or a))


# ---- 1. same inputs in plain FP64 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('config', CONFIGS, ids=CONFIG_IDS)
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_same_inputs_in_plain_fp64_symmetry_definiteness_and_the_far_field(shape, config):
    q, p, T = shape
    ctx, par, _, _ = make_ctx(shape, config)
    try:
        m = ctx.post_mean().reshape(R8, p, T)
        scale_m = float(np.max(np.abs(m)))
        grids = {S: make_times(T, S, par['tau'], 0) for S in S_VALUES}
        s_all = np.concatenate([grids[S][0] for S in S_VALUES])
        ref_cov = np.stack([numpy_cov_at(par['tau'], ctx.post_cov(r), s_all) for r in range(R8)])          # computed once, sliced per S
        ref_mean = np.stack([numpy_mean_at(par['tau'], m[r], s_all) for r in range(R8)])
        at = 0
        for S in S_VALUES:
            s, far = grids[S]
            rc, rm = ref_cov[:, at:at + S], ref_mean[:, :, at:at + S]
            at += S
            ctx.set_option('covat_block_times', 0)
            got = ctx.posterior_cov_at(s, want=ALL)
            ctx.set_option('covat_block_times', 16)
            blocked = ctx.posterior_cov_at(s, want=ALL)
            ctx.set_option('covat_block_times', 0)
            assert got['mean'].shape == (R8, p, S) and got['cov'].shape == (R8, S, p, p) and got['eta'].shape == (R8, q, S) and got['var'].shape == (R8, q, S)
            e_c, e_m = rel(got['cov'], rc), float(np.max(np.abs(got['mean'] - rm)) / scale_m)
            ev = np.linalg.eigvalsh(got['cov'])
            e_eig = float(np.min(ev[..., 0] / ev[..., -1]))
            e_far = float(np.max(np.abs(got['cov'][:, far] - np.eye(p)), initial=0.0))
            print('q=%d p=%d T=%d %s S=%d: cov %.2e of the largest entry, mean %.2e of max|m| (limit %.0e); smallest / largest eigenvalue %.2e (limit -1e-12); '
                  'far field %.2e (limit %.0e); blocks of 16 times the same bits: %s'
                  % (q, p, T, tag(config), S, e_c, e_m, TOL_SAME, e_eig, e_far, TOL_FAR, same_bits(got, blocked)))
            assert e_c <= TOL_SAME and e_m <= TOL_SAME
            assert np.array_equal(got['cov'], got['cov'].transpose(0, 1, 3, 2))
            assert e_eig >= -1e-12
            assert e_far <= TOL_FAR
            assert same_bits(got, blocked)
            if S == 17:                                          # each output asked for alone: the same bits
                for k in ALL:
                    assert np.array_equal(ctx.posterior_cov_at(s, want=(k,))[k], got[k]), k
    finally:
        ctx.close()


# ---- 2. the grid identity and consistency with the other queries -----------------------------------------------------------------------------------
@pytest.mark.parametrize('config', CONFIGS, ids=CONFIG_IDS)
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_on_the_grid_it_is_post_vsm_and_agrees_with_posterior_at_and_posterior_rates(shape, config):
    q, p, T = shape
    ctx, par, _, _ = make_ctx(shape, config)
    try:
        grid = np.arange(T) * BIN_MS
        got = ctx.posterior_cov_at(grid, want=ALL)
        vsm = ctx.post_vsm().reshape(R8, T, p, p)
        e_vsm = rel(got['cov'], vsm)
        s, _ = make_times(T, 65, par['tau'], 1)
        off = ctx.posterior_cov_at(s, want=('mean', 'cov'))
        at = ctx.posterior_at(s)
        e_diag = float(np.max(np.abs(np.diagonal(off['cov'], axis1=2, axis2=3).transpose(0, 2, 1) - at['var'])) / np.max(np.abs(off['cov'])))
        e_mean = float(np.max(np.abs(off['mean'] - at['mean'])) / np.max(np.abs(at['mean'])))
        rates = ctx.posterior_rates(want=('eta', 'var'))
        e_eta, e_var = rel(got['eta'], rates['eta']), rel(got['var'], rates['var'])
        print('q=%d p=%d T=%d %s: cov on the grid against post_vsm %.2e; diagonal against posterior_at var %.2e, mean %.2e; eta %.2e and var %.2e against '
              'posterior_rates - of the largest entry (limit %.0e)' % (q, p, T, tag(config), e_vsm, e_diag, e_mean, e_eta, e_var, TOL_SAME))
        assert max(e_vsm, e_diag, e_mean, e_eta, e_var) <= TOL_SAME
    finally:
        ctx.close()


# ---- 3. the independent dense model ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('config', CONFIGS, ids=CONFIG_IDS)
@pytest.mark.parametrize('shape', SHAPES[1:3], ids=IDS[1:3])
def test_off_the_grid_it_is_the_block_of_the_model_extended_by_the_query_times(shape, config):
    q, p, T = shape
    ctx, par, _, _ = make_ctx(shape, config)
    try:
        m = ctx.post_mean().reshape(R8, p, T)
        s, far = make_times(T, 65, par['tau'], 1)
        near = np.setdiff1d(np.arange(65), far)
        trials = np.array([5, 0], dtype=np.int32)
        got = ctx.posterior_cov_at(s[near], trials, want=('cov',))
        for i, r in enumerate(trials):
            W = orc.poisson_blocks(m[r], np.asarray(par['C']), np.asarray(par['d']).reshape(-1))
            err = rel(got['cov'][i], extended_blocks(par['tau'], W, s[near], T))
            print('q=%d p=%d T=%d %s trial %d: extended model, cov %.2e relative (limit %.0e)' % (q, p, T, tag(config), r, err, TOL_DENSE))
            assert err <= TOL_DENSE
    finally:
        ctx.close()


# ---- 4. rates -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('config', CONFIGS, ids=CONFIG_IDS)
@pytest.mark.parametrize('shape', [SHAPES[0], SHAPES[3], SHAPES[4]], ids=[IDS[0], IDS[3], IDS[4]])
def test_eta_and_var_are_the_contractions_of_the_calls_own_mean_and_cov(shape, config):
    q, p, T = shape
    ctx, par, _, _ = make_ctx(shape, config)
    try:
        for S in (17, 65):
            s, _ = make_times(T, S, par['tau'], 2)
            got = ctx.posterior_cov_at(s, want=ALL)
            eta, var, a_eta, a_var = numpy_rates_at(np.asarray(par['C']), np.asarray(par['d']).reshape(-1), got['mean'], got['cov'])
            e_eta, e_var = float(np.max(np.abs(got['eta'] - eta) / a_eta)), float(np.max(np.abs(got['var'] - np.maximum(var, 0.0)) / a_var))
            print('q=%d p=%d T=%d %s S=%d: eta %.2e, var %.2e of the sums of absolute terms (limit %.0e); smallest var %.3e'
                  % (q, p, T, tag(config), S, e_eta, e_var, TOL_RATES, float(got['var'].min())))
            assert e_eta <= TOL_RATES and e_var <= TOL_RATES
            assert np.all(got['var'] >= 0.0)
    finally:
        ctx.close()


# ---- 5. ragged trials and both observation tables ---------------------------------------------------------------------------------------------------
def own_grid_covariance(par, mode, live, L):
    """the trial's own L-bin dense posterior covariance (likelihood terms at its live entries only) at the device's mode"""
    C, d = np.asarray(par['C']), np.asarray(par['d']).reshape(-1)
    p = C.shape[1]
    e = np.exp(C @ mode[:, :L] + d[:, None]) * live[:, :L]
    W = np.einsum('nk,nt,nl->tkl', C, e, C)
    Kinv = np.linalg.inv(orc.make_K(par['tau'], L, BIN_MS))
    H = np.zeros((p, L, p, L))
    ar = np.arange(L)
    for k in range(p):
        H[k, :, k, :] += Kinv[k]
        for l in range(p):
            H[k, ar, l, ar] += W[:, k, l]
    return np.linalg.inv(H.reshape(p * L, p * L))


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
        m = ctx.post_mean().reshape(R8, p, T)
        s, _ = make_times(T, 65, par['tau'], 2)
        # on top: query times behind T_r of the short trials and grid times at padded bins
        s = np.concatenate([s, [17.5 * BIN_MS, 18.0 * BIN_MS, 41.0 * BIN_MS, 64.5 * BIN_MS, 73.0 * BIN_MS, (T - 1.5) * BIN_MS, 0.5 * (17 + T) * BIN_MS]])
        got = ctx.posterior_cov_at(s, want=('cov',))
        worst = 0.0
        for r in range(R8):
            ref = numpy_cov_at(par['tau'], own_grid_covariance(par, m[r], live[r], int(lens[r])), s)
            err = rel(got['cov'][r], ref)
            worst = max(worst, err)
            print('%s trial %d (%d bins): own-grid posterior, cov %.2e relative (limit %.0e)' % (tag(config), r, lens[r], err, TOL_DENSE))
        assert worst <= TOL_DENSE
        grid = ctx.posterior_cov_at(np.arange(T) * BIN_MS, want=('eta', 'var'))
        rates = ctx.posterior_rates(want=('eta', 'var'))
        behind = np.arange(T)[None, :] >= lens[:, None]
        e_eta = float(np.max(np.abs(grid['eta'] - rates['eta'])[np.broadcast_to(behind[:, None, :], grid['eta'].shape)]) / np.max(np.abs(rates['eta'])))
        e_var = float(np.max(np.abs(grid['var'] - rates['var'])[np.broadcast_to(behind[:, None, :], grid['var'].shape)]) / np.max(np.abs(rates['var'])))
        print('%s: behind T_r, eta %.2e and var %.2e against posterior_rates (the forecast), of the largest entry (limit %.0e)' % (tag(config), e_eta, e_var, TOL_SAME))
        assert e_eta <= TOL_SAME and e_var <= TOL_SAME
    finally:
        ctx.close()


# ---- 6. variational posteriors ----------------------------------------------------------------------------------------------------------------------
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
        s, _ = make_times(T, 65, par['tau'], 4)
        got = ctx.posterior_cov_at(s, want=('cov',))
        worst = 0.0
        for r in range(R):
            Sigma, _ = orc.vi_post_cov(Kinv_big, C_big, lam[r])
            err = rel(got['cov'][r], numpy_cov_at(par['tau'], Sigma, s))
            worst = max(worst, err)
            print('%s engine %d trial %d: VIPostCov at the kept lambda, cov %.2e relative (limit %.0e)' % (which, engine, r, err, TOL_DENSE))
        assert worst <= TOL_DENSE
    finally:
        ctx.close()


# ---- 7. bits do not depend on the call ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('config', CONFIGS, ids=CONFIG_IDS)
@pytest.mark.parametrize('shape', [SHAPES[1], SHAPES[5]], ids=[IDS[1], IDS[5]])
def test_per_trial_grids_lists_chunks_and_blocks_give_the_same_bits(shape, config):
    q, p, T = shape
    ctx, par, _, _ = make_ctx(shape, config)
    try:
        S = 65
        grids = np.stack([make_times(T, S, par['tau'], 10 + r)[0] for r in range(R8)])
        per = ctx.posterior_cov_at(grids, want=ALL)
        singles = [bool(same_bits(ctx.posterior_cov_at(grids[r], np.array([r], dtype=np.int32), want=ALL), {k: per[k][r:r + 1] for k in ALL})) for r in range(R8)]
        print('q=%d p=%d T=%d %s: (n, S) call against one shared-grid call per trial, same bits %s' % (q, p, T, tag(config), singles))
        assert all(singles)
        shared = ctx.posterior_cov_at(grids[0], want=ALL)
        order = np.array([6, 2, 2, 7, 0, 5, 1, 3, 4, 2], dtype=np.int32)     # permuted, trial 2 three times
        seen = []
        for chunk, block in ((1, 0), (3, 0), (0, 16), (0, 32), (3, 16), (0, 0)):
            ctx.set_option('covat_chunk_trials', chunk)
            ctx.set_option('covat_block_times', block)
            a = ctx.posterior_cov_at(grids, want=ALL)
            b = ctx.posterior_cov_at(grids[order], order, want=ALL)
            c = ctx.posterior_cov_at(grids[0], order, want=ALL)
            seen.append((chunk, block, same_bits(a, per), all(np.array_equal(b[k], per[k][order]) for k in ALL), all(np.array_equal(c[k], shared[k][order]) for k in ALL)))
        print('q=%d p=%d T=%d %s: (covat_chunk_trials, covat_block_times, all trials, permuted list with repeats, shared grid) %s' % (q, p, T, tag(config), seen))
        assert all(x[2] and x[3] and x[4] for x in seen)
    finally:
        ctx.close()


@pytest.mark.parametrize('config', CONFIGS, ids=CONFIG_IDS)
def test_a_list_across_two_parameter_snapshots_gives_the_bits_of_one_call_per_trial(config):
    """four trials, {0, 1} through an E-step at parameters A and {2, 3} through one at B (C, d and every timescale differ): one call over
    [3, 0, 2, 1, 0] walks two snapshot groups and scatters by list position (the construction of test_gpu_posterior_at.py)"""
    from funs import _hip
    shape = SHAPES[0]
    q, p, T = shape
    par, Y, _ = problem(shape, R=4)
    mixed = np.array([3, 0, 2, 1, 0], dtype=np.int32)
    s = np.array([0.0, 3.7, 10.0, T - 1.0, T + 2.5]) * BIN_MS
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
        before = [ctx.post_mean(), ctx.post_vsm(), ctx.gram()]
        one = ctx.posterior_cov_at(s, mixed, want=ALL)
        after = [ctx.post_mean(), ctx.post_vsm(), ctx.gram()]
        same = [bool(same_bits(ctx.posterior_cov_at(s, mixed[i:i + 1], want=ALL), {k: one[k][i:i + 1] for k in ALL})) for i in range(mixed.size)]
        kept = [bool(np.array_equal(a, b)) for a, b in zip(before, after)]
        # the two groups were evaluated under their own parameters: eta of trial 3 follows the second C and d
        eta3 = (par['d'] + 0.1)[:, None] + (par['C'] * 1.05 + 0.01) @ one['mean'][0]
        e3 = float(np.max(np.abs(one['eta'][0] - eta3)))
        print('%s: list %s against one call per entry %s; post_mean, post_vsm, Gram unchanged %s; eta of trial 3 under its own C, d %.2e' % (tag(config), mixed.tolist(), same, kept, e3))
        assert all(same) and all(kept)
        assert same_bits({k: one[k][1] for k in ALL}, {k: one[k][4] for k in ALL})
        assert e3 <= 1e-12 * (np.abs(par['d']).max() + 1.0 + np.abs(par['C']).sum(axis=1).max() * np.abs(one['mean']).max())
    finally:
        ctx.close()


# ---- 8. no state is touched -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('config', CONFIGS, ids=CONFIG_IDS)
def test_no_state_is_touched(config):
    shape = SHAPES[1]
    q, p, T = shape
    ctx, par, _, _ = make_ctx(shape, config)
    try:
        s, _ = make_times(T, 65, par['tau'], 3)
        pick = np.array([0, 3], dtype=np.int32)

        def state():
            blocks = ctx.post_vsmgp(pick)        # (first: under the sum-only plan this download rebuilds the blocks and rewrites post_vsm of these trials)
            at, smp = ctx.posterior_at(s), ctx.posterior_sample(pick, n_samples=3, seed=5, want=('x',))
            return [ctx.post_mean(), ctx.post_vsm(), blocks, ctx.gram(), at['mean'], at['var'], smp['x']]
        before = state()
        first = ctx.posterior_cov_at(s, want=ALL)
        after = state()
        again = ctx.posterior_cov_at(s, want=ALL)
        same = [bool(np.array_equal(a, b)) for a, b in zip(before, after)]
        print('%s: post_mean, post_vsm, post_vsmGP, Gram, posterior_at mean / var, posterior_sample x unchanged by the call: %s; the call repeats its bits: %s'
              % (tag(config), same, same_bits(first, again)))
        assert all(same) and same_bits(first, again)
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
            ctx.posterior_cov_at(np.zeros(3))
        # a time that is not finite is refused before the parameters are even looked at: no device call has been made
        with pytest.raises(_hip.HipBackendError, match='query time 1 is not finite'):
            ctx.posterior_cov_at(np.array([0.0, np.nan, 1.0]))
        ctx.set_params(par['C'], par['d'], par['tau'])
        with pytest.raises(_hip.HipBackendError, match='no posterior for trial 0'):
            ctx.posterior_cov_at(np.zeros(3))
        ctx.estep_laplace(np.array([0, 1, 2], dtype=np.int32))
        with pytest.raises(_hip.HipBackendError, match='no posterior for trial 3'):
            ctx.posterior_cov_at(np.zeros(3))
        idx = np.array([2, 0], dtype=np.int32)
        assert ctx.posterior_cov_at(np.zeros(3), idx)['cov'].shape == (2, 3, p, p)
        with pytest.raises(_hip.HipBackendError, match='S = 0'):
            ctx.posterior_cov_at(np.zeros(0), idx)
        t = np.zeros(3)
        out = np.zeros(2 * p * 3)
        assert ctx.lib.pgpfa_posterior_cov_at(ctx.h, 2, _hip.iptr(idx), 3, _hip.dptr(t), 0, None, None, None, None) != 0
        assert 'no output asked for' in ctx.lib.pgpfa_last_error().decode()
        assert ctx.lib.pgpfa_posterior_cov_at(ctx.h, 2, _hip.iptr(idx), 3, None, 0, _hip.dptr(out), None, None, None) != 0
        assert 'times_ms is NULL' in ctx.lib.pgpfa_last_error().decode()
        grids = np.zeros((2, 3))
        grids[1, 2] = np.inf
        with pytest.raises(_hip.HipBackendError, match=r'query time 2 of list entry 1 \(trial 0\) is not finite'):
            ctx.posterior_cov_at(grids, idx)
        with pytest.raises(ValueError, match='times must have shape'):
            ctx.posterior_cov_at(np.zeros((3, 3)), idx)
        with pytest.raises(ValueError, match='unknown output'):
            ctx.posterior_cov_at(np.zeros(3), idx, want=('mean', 'rate'))
        with pytest.raises(ValueError, match='no output asked for'):
            ctx.posterior_cov_at(np.zeros(3), idx, want=())
        # an uploaded posterior has blocks, no square root
        ctx.set_posterior(np.array([3], dtype=np.int32), np.zeros((1, p, T)), np.tile(np.eye(p), (1, T, 1, 1)), np.tile(np.eye(T)[:, :, None], (1, 1, 1, p)))
        assert ctx.posterior_at(np.zeros(3), np.array([3], dtype=np.int32))['var'].shape == (1, p, 3)
        with pytest.raises(_hip.HipBackendError, match='posterior of trial 3 was uploaded.*no square root'):
            ctx.posterior_cov_at(np.zeros(3), np.array([0, 3], dtype=np.int32))
        # an asynchronous timescale pass in flight
        ctx.mstep_precomp()
        Q = np.log(1.0 / (par['tau'] * 100.0) ** 2)[None, :] + np.array([0.0, 0.1])[:, None]
        ctx.mstep_tau_costgrad_multi_begin(Q)
        with pytest.raises(_hip.HipBackendError, match='timescale pass is in flight'):
            ctx.posterior_cov_at(np.zeros(3), idx)
        ctx.mstep_tau_costgrad_multi_end()
        assert ctx.posterior_cov_at(np.zeros(3), idx, want=('var',))['var'].shape == (2, q, 3)
        # counts uploaded after the E-step: the posterior is gone
        ctx.upload_counts(Y.astype(np.uint8))
        with pytest.raises(_hip.HipBackendError, match='no posterior for trial 2'):
            ctx.posterior_cov_at(np.zeros(3), idx)
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
            ctx.posterior_cov_at(np.zeros(3))
        assert ctx.posterior_cov_at(np.zeros(3), np.array([0, 2], dtype=np.int32))['cov'].shape == (2, 3, p, p)      # the full-length ones are served
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


def test_util_posterior_rates_at_with_conditions_on_a_ragged_config1_experiment(funs_mod):
    util, inference = funs_mod.util, funs_mod.inference
    shape = (30, 3, 100)
    q, p, T = shape
    R = 6
    par, Y, _ = problem(shape, R=R)
    lens = np.array([T, T - 1, 17, 16, T, 40])
    exp = Experiment([Y[r][:, :lens[r]].astype(np.float64) for r in range(R)], BIN_MS)
    params = {k: np.array(v, dtype=np.float64) for k, v in par.items()}
    infRes, _ = inference.laplace(exp, {k: v.copy() for k, v in params.items()}, returnOptimRes=False)
    lags = np.arange(-3, 4) * 7.5
    event = np.array([300.0, 120.0, 150.0, 5.0, 500.0, 380.0])            # trials 2, 3 and 5 leave their recorded span at some lags
    grids = event[:, None] + lags[None, :]
    cond = np.array([4, 9, 4, 9, 4, 9])
    out = util.posteriorRatesAt(params, exp, grids, infRes=infRes, conditions=cond, level=0.9, want=('rate', 'lower', 'upper', 'median', 'eta', 'var'))
    lat = util.posteriorAt(params, exp, grids, infRes=infRes, want=('mean', 'cov'))
    plain = util.posteriorAt(params, exp, grids, infRes=infRes, want=('mean',))
    assert lat['cov'].shape == (R, lags.size, p, p) and out['rate'].shape == (R, q, lags.size) and out['condition_labels'].tolist() == [4, 9]
    assert np.array_equal(lat['mean'], plain['mean'])                        # the same mean bits with and without 'cov' in want
    eta, var, a_eta, a_var = numpy_rates_at(params['C'], params['d'].reshape(-1), lat['mean'], lat['cov'])
    # (the mean of posteriorAt comes from pgpfa_posterior_at's launch, eta from the new call's own: same kernel, same inputs)
    e_eta, e_var = float(np.max(np.abs(out['eta'] - eta) / a_eta)), float(np.max(np.abs(out['var'] - np.maximum(var, 0.0)) / a_var))
    print('util.posteriorRatesAt on ragged config 1: eta %.2e, var %.2e of the sums of absolute terms (limit %.0e)' % (e_eta, e_var, TOL_RATES))
    assert e_eta <= TOL_RATES and e_var <= TOL_RATES
    z, per_s = util._band_z(0.9), 1000.0 / BIN_MS
    assert np.array_equal(out['rate'], np.exp(out['eta'] + 0.5 * out['var']) * per_s) and np.array_equal(out['median'], np.exp(out['eta']) * per_s)
    assert np.array_equal(out['lower'], np.exp(out['eta'] - z * np.sqrt(out['var'])) * per_s)
    assert np.array_equal(out['upper'], np.exp(out['eta'] + z * np.sqrt(out['var'])) * per_s)
    inside = (grids >= 0.0) & (grids <= ((lens - 1) * BIN_MS)[:, None])
    for g, label in enumerate((4, 9)):
        members = np.flatnonzero(cond == label)
        count = inside[members].sum(axis=0)
        assert np.array_equal(out['condition_count'][g], count)
        total = (out['rate'][members] * inside[members][:, None, :]).sum(axis=0)
        want = np.where(count[None, :] > 0, total / np.maximum(count, 1)[None, :], 0.0)
        assert np.allclose(out['condition_mean'][g], want, rtol=1e-14, atol=0.0)
    assert 0 < inside.sum() < inside.size                                    # some trials are outside their span at some lags


def test_fit_posterior_rates_at_after_a_two_iteration_fit(funs_mod):
    shape = (30, 3, 100)
    q, p, T = shape
    par, Y, _ = problem(shape, R=R8)
    exp = Experiment([Y[r].astype(np.float64) for r in range(R8)], BIN_MS)
    init = {k: np.array(v, dtype=np.float64) for k, v in par.items()}
    fit = funs_mod.engine.PPGPFAfit(exp, initParams=init, EMmode='Batch', maxEMiter=2, CdOptimMethod='newton', quiet=True)
    fine = np.arange(0.0, (T - 1) * BIN_MS + 1e-9, BIN_MS / 4.0)
    out = fit.posteriorRatesAt(times=fine, conditions=np.arange(R8) % 2)
    assert fit.ratesAt is out and out['rate'].shape == (R8, q, fine.size) and out['condition_mean'].shape == (2, q, fine.size)
    assert np.all(out['lower'] <= out['rate']) and np.all(out['lower'] <= out['upper'])
    assert np.array_equal(out['condition_count'], np.full((2, fine.size), R8 // 2))
    assert fit.infRes['post_mean'][3].shape == (p, T)                  # kept on the host before the E-step superseded it
    # on the grid the finely sampled rate passes through the rates of the posterior that util.posteriorRatesAt's E-step left resident
    from funs import _session
    sess, _ = _session.session_for(exp, p)
    dev = sess.ctx.posterior_rates(want=('eta', 'var'))
    on = np.exp(dev['eta'] + 0.5 * dev['var']) * (1000.0 / BIN_MS)
    err = float(np.max(np.abs(out['rate'][:, :, ::4] - on)) / np.max(np.abs(on)))
    print('PPGPFAfit.posteriorRatesAt: rate on the grid against posterior_rates %.2e of the largest (limit %.0e)' % (err, TOL_SAME))
    assert err <= TOL_SAME
    for g in range(2):
        assert np.allclose(out['condition_mean'][g], out['rate'][g::2].mean(axis=0), rtol=1e-12, atol=0.0)
