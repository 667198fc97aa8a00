"""Dual-variational E-step and EM on trials of unequal length and with unobserved neurons (inference.DUAL_MASKED, C-ABI option dual_masked;
DESIGN.md section 3).

Yardstick: the reference's own functions as the oracle restates them - orc.dual_cost, orc.dual_grad, orc.vi_post_mean, orc.vi_post_cov +
orc.marginal_blocks - applied to every trial's REDUCED problem: rows of Y, C and d deleted for unobserved neurons, bins cut to T_r.  (At 40 x 10 x 176
orc.dual_grad's three-operand einsum takes a minute per trial; `dual_grad_blas` below is the same formula with the quadratic term as one BLAS
product, and every config-1 check asserts that the two agree to 1e-13 before it uses it.)

Tolerances (the project's own for this path): max |dual_grad| at the returned lambda <= 1e-7, dual cost 1e-8 relative, post_mean
1e-9, post_vsm / post_vsmGP / post_cov 1e-7 of their largest entry.  No test may pass by handing a trial back: every fixed-point status is 0 and every
pass count is at most DUAL_FP_MAX_PASSES.  Every test prints the figures it measured before it asserts."""
import numpy as np
import pytest

from conftest import Experiment, load_golden
from oracle import pgpfa_oracle as orc

pytestmark = pytest.mark.gpu

BIN_MS = 10.0
TOL_GRAD, TOL_COST, TOL_MEAN, TOL_COV = 1e-7, 1e-8, 1e-9, 1e-7


@pytest.fixture(scope='module')
def funs_mod():
    import funs
    return funs


@pytest.fixture(scope='module', autouse=True)
def _leave_nothing_behind():
    yield
    import gc
    from funs import _session
    _session.drop_sessions()
    _problems.clear()
    gc.collect()


@pytest.fixture()
def masked(funs_mod):
    """DUAL_MASKED on, the low-rank engine selectable at any size (COV_MODE = 2; DUAL_LOWRANK then picks the engine); everything restored afterwards"""
    from funs import _session
    inf = funs_mod.inference
    old = (inf.DUAL_MASKED, inf.COV_MODE, inf.DUAL_LOWRANK, inf.DUAL_SOLVER)
    _session.drop_sessions()
    inf.DUAL_MASKED, inf.COV_MODE = True, 2
    yield inf
    inf.DUAL_MASKED, inf.COV_MODE, inf.DUAL_LOWRANK, inf.DUAL_SOLVER = old
    _session.drop_sessions()


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------------
def seam_table(R, q):
    """the observation patterns of test_gpu_observed_neurons.py that the issue names: fully observed | lacking {0, 15, 16, q-1} | a single neuron |
    every second neuron, in turn over the trials"""
    n = np.arange(q)
    rows = [np.ones(q, bool), ~np.isin(n, [0, 15, 16, q - 1]), n == 17, n % 2 == 0]
    return np.stack([rows[r % 4] for r in range(R)])


def c1_problem(R=8):
    g = load_golden('c1_dataset.npz')
    Ys = [g['Y'][r].astype(np.float64) for r in range(R)]
    params = {'C': g['init_C'].copy(), 'd': g['init_d'].copy(), 'tau': g['init_tau'].copy()}
    T = Ys[0].shape[1]
    lens = np.array([T, 50, 73, 1, 99, 64, 87, 51][:R], dtype=np.int32)      # 50 .. 100, one trial at T, one of a single bin
    return params, Ys, T, lens


def synth_problem(q, p, T, lens):
    params, Ys, _ = orc.synth_dataset(q, p, T, len(lens), seed=31 + p)
    return params, [np.asarray(y, dtype=np.float64) for y in Ys], T, np.asarray(lens, dtype=np.int32)


def experiment(Ys, lens=None, table=None):
    Yr = [y[:, :int(L)] for y, L in zip(Ys, lens)] if lens is not None else Ys
    exp = Experiment(Yr, BIN_MS)
    if table is not None:
        for r, tr in enumerate(exp.data):
            tr['observed'] = table[r].copy()
            tr['Y'] = tr['Y'].copy()
            tr['Y'][~table[r]] = np.nan                                    # nothing may read the unobserved rows
    return exp


_problems = {}


def reduced_problem(key, params, Y, o, L):
    """(ybar, C_big, K_big, Kinv_big, d_big) of the reference for one trial's reduced problem; computed once per key, never written to"""
    if key not in _problems:
        C, d = params['C'][o], np.asarray(params['d']).reshape(-1)[o]
        C_big, d_big = orc.make_Cd_big(C, d, L)
        K = orc.make_K(params['tau'], L, BIN_MS)
        K_big = orc.make_K_big(K)
        Kinv_big = orc.make_K_big(np.stack([np.linalg.inv(k) for k in K]))
        _problems[key] = (np.ascontiguousarray(Y[o][:, :L]).reshape(-1), C_big, K_big, Kinv_big, d_big)
    return _problems[key]


def dual_grad_blas(lam, ybar, C_big, K_big, Kinv_big, d_big):
    """orc.dual_grad with 'im,ij,jm->m' as one matrix product and a row-wise dot"""
    S, _ = orc.vi_post_cov(Kinv_big, C_big, lam)
    quad = np.einsum('im,im->m', C_big, S @ C_big)
    return C_big.T @ (K_big @ (C_big @ (lam - ybar))) - d_big + np.log(lam) - 0.5 * quad


def check_optimum(tag, case, params, Ys, lens, table, T, infRes, optim, vlb, sess, log=False, cov_trial=None, use_orc_grad=False, tol_grad=TOL_GRAD):
    """every figure of the issue's table for one dualVariational result; returns the per-trial oracle costs at the returned lambda"""
    R, q, p = len(Ys), Ys[0].shape[0], params['C'].shape[1]
    e_g = e_c = e_m = e_v = e_gp = e_cc = 0.0
    costs = np.zeros(R)
    lam_pad = np.zeros((R, q * T))
    for r in range(R):
        L, o = int(lens[r]), (table[r] if table is not None else np.ones(q, bool))
        x = np.asarray(optim[r], dtype=np.float64)
        assert x.shape == (q * T,)
        live = np.zeros((q, T), bool)
        live[o, :L] = True
        assert np.all(x.reshape(q, T)[~live] == 0.0), '%s: trial %d has non-zero dual variables at entries that are not live' % (tag, r)
        lam = np.exp(x.reshape(q, T)[o][:, :L].reshape(-1)) if log else x.reshape(q, T)[o][:, :L].reshape(-1)
        assert np.all(lam > 0.0)
        lam_pad[r] = np.where(live, np.exp(x.reshape(q, T)) if log else x.reshape(q, T), 0.0).reshape(-1)
        pr = reduced_problem((case, r, L, o.tobytes()), params, Ys[r], o, L)
        g = dual_grad_blas(lam, *pr)
        if use_orc_grad:
            assert np.max(np.abs(g - orc.dual_grad(lam, *pr))) <= 1e-13 * max(1.0, np.max(np.abs(g)))
        e_g = max(e_g, float(np.max(np.abs(g))))
        costs[r] = orc.dual_cost(lam, *pr)
        S, _ = orc.vi_post_cov(pr[3], pr[1], lam)
        gp_ref, v_ref = orc.marginal_blocks(S, p, L)
        m, v, gp = infRes['post_mean'][r], infRes['post_vsm'][r], infRes['post_vsmGP'][r]
        assert m.shape == (p, L) and v.shape == (L, p, p) and gp.shape == (L, L, p)
        e_m = max(e_m, float(np.max(np.abs(m.reshape(-1) - orc.vi_post_mean(pr[2], pr[1], pr[0], lam)))))
        e_v, e_gp = max(e_v, rel(v, v_ref)), max(e_gp, rel(gp, gp_ref))
        if r == cov_trial:
            pc = infRes['post_cov'][r]
            assert pc.shape == (p * L, p * L)
            e_cc = rel(pc, S)
    # the cost of every trial at the returned lambda, through the batched evaluation, and the mean the call returned
    cb, _ = sess.ctx.dual_costgrad_batch(infRes.trial_idx, lam_pad, want_grad=False)
    e_c = float(np.max(np.abs(cb - costs) / np.abs(costs)))
    e_mean = abs(vlb - costs.mean()) / abs(costs.mean())
    print('%s: max |dual_grad| %.2e, cost %.2e (mean %.2e), post_mean %.2e, post_vsm %.2e, post_vsmGP %.2e, post_cov %.2e'
          % (tag, e_g, e_c, e_mean, e_m, e_v, e_gp, e_cc))
    assert e_g <= tol_grad and e_c <= TOL_COST and e_mean <= TOL_COST and e_m <= TOL_MEAN and e_v <= TOL_COV and e_gp <= TOL_COV and e_cc <= TOL_COV
    return costs


def check_contracted(inf, infRes):
    print('    fixed-point passes %s, status %s' % (infRes.dual_iterations.tolist(), infRes.dual_status.tolist()))
    assert np.all(infRes.dual_status == 0) and np.all(infRes.dual_iterations <= inf.DUAL_FP_MAX_PASSES)


def copy_params(params):
    return {k: np.array(v, copy=True) for k, v in params.items()}


# ---- 1. config 1, both engines, the tables one by one and together ---------------------------------------------------------------------------
@pytest.mark.parametrize('lowrank', [0, 1], ids=['dense', 'lowrank'])
@pytest.mark.parametrize('tables', ['lengths', 'observed', 'both'])
def test_config1_against_the_reference_on_the_reduced_trials(masked, tables, lowrank):
    params, Ys, T, lens = c1_problem()
    q = Ys[0].shape[0]
    table = seam_table(len(Ys), q) if tables != 'lengths' else None
    if tables == 'observed':
        lens = np.full(len(Ys), T, dtype=np.int32)
    masked.DUAL_LOWRANK = bool(lowrank)
    exp = experiment(Ys, lens, table)
    infRes, nll, vlb, optim = masked.dualVariational(exp, copy_params(params))
    sess = infRes.session
    assert sess.ctx.info('plan_lowrank') == float(lowrank)
    assert sess.ctx.info('trial_lengths_set') == float(tables != 'observed') and sess.ctx.info('observed_set') == float(tables != 'lengths')
    check_contracted(masked, infRes)
    check_optimum('config 1, %s, engine %d' % (tables, lowrank), 'c1', params, Ys, lens, table, T, infRes, optim, vlb, sess,
                  cov_trial=2, use_orc_grad=True)


# ---- 2. tile seams -----------------------------------------------------------------------------------------------------------------------------
SEAMS = {'p10': (40, 10, 176, [1, 63, 64, 65, 128, 176]), 'p20': (50, 20, 48, [1, 31, 32, 33, 48])}


@pytest.mark.timeout(600)
@pytest.mark.parametrize('name,vector', [('p10', False), ('p20', False), ('p10', True)], ids=['p10', 'p20-wide', 'p10-vector'])
def test_lengths_across_the_tile_seams(masked, name, vector):
    """40 x 10 x 176 with lengths {1, 63, 64, 65, 128, 176} (dual_pre_kernel's 64-bin tile, dual_unpack_w_kernel's 32-bin tile, the GEMM's 128-row
    tile) and 50 x 20 x 48 with {1, 31, 32, 33, 48} (the wide form: rates_wide_kernel and the GEMMs against the pair table); once the vector forms
    (dual_gemm = 0, use_mfma = 0) on the first shape.  Both tables are set."""
    q, p, T, lens = SEAMS[name]
    params, Ys, T, lens = synth_problem(q, p, T, lens)
    table = seam_table(len(Ys), q)
    masked.DUAL_LOWRANK = True
    exp = experiment(Ys, lens, table)
    if vector:
        from funs import _session
        sess, _ = _session.session_for(exp, p)
        sess.ctx.set_option('dual_gemm', 0)
        sess.ctx.set_option('use_mfma', 0)
    infRes, nll, vlb, optim = masked.dualVariational(exp, copy_params(params))
    check_contracted(masked, infRes)
    check_optimum('%s%s' % (name, ', vector forms' if vector else ''), name, params, Ys, lens, table, T, infRes, optim, vlb, infRes.session)


# ---- 3. the other solvers ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(900)
@pytest.mark.parametrize('solver', ['device', 'scipy'])
def test_other_solvers_on_config1_with_both_tables(masked, solver):
    """DUAL_SOLVER 'device' (lockstep L-BFGS in rho) and 'scipy' on config 1 with both tables: the cost the call returns is orc.dual_cost at the
    returned lambda (1e-8), and it lies within the reference's own L-BFGS stop - factr = 1e7: a relative decrease of 1e7 * eps = 2.2e-9 per step,
    held here as |f - f*| <= 1e-6 max(|f*|, 1) as test_gpu_parity.py holds the same solvers - of the fixed point's optimum."""
    params, Ys, T, lens = c1_problem(R=4)
    table = seam_table(len(Ys), Ys[0].shape[0])
    masked.DUAL_LOWRANK = True
    exp = experiment(Ys, lens, table)
    infRes, _, vlb_fp, optim = masked.dualVariational(exp, copy_params(params))
    check_contracted(masked, infRes)
    f_star = check_optimum('fixed point', 'c1', params, Ys, lens, table, T, infRes, optim, vlb_fp, infRes.session)
    masked.DUAL_SOLVER = solver
    infRes, _, vlb, optim = masked.dualVariational(exp, copy_params(params))
    # (an L-BFGS optimum is stationary to its own stop only: the gradient bound of the fixed point does not apply, everything else does)
    f = check_optimum(solver, 'c1', params, Ys, lens, table, T, infRes, optim, vlb, infRes.session, tol_grad=np.inf)
    gap = np.abs(f - f_star) / np.maximum(np.abs(f_star), 1.0)
    print('%s: distance to the fixed point\'s optimum %s' % (solver, gap.tolist()))
    assert np.all(f >= f_star - 1e-8 * np.maximum(np.abs(f_star), 1.0)) and np.all(gap <= 1e-6)


# ---- 4. cost and gradient away from the optimum --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lowrank', [0, 1], ids=['dense', 'lowrank'])
def test_costgrad_batch_at_a_random_lambda(funs_mod, lowrank):
    """pgpfa_dual_costgrad_batch at a random positive lambda with both tables: cost 1e-8 relative, gradient 1e-8 of its largest entry at live entries
    and exactly 0 elsewhere; what the caller passes at entries that are not live (NaN here) is ignored."""
    from funs import _hip
    params, Ys, T, lens = c1_problem(R=6)
    R, q = len(Ys), Ys[0].shape[0]
    table = seam_table(R, q)
    Y = np.zeros((R, q, T), dtype=np.uint8)
    for r in range(R):
        Y[r, table[r], :lens[r]] = Ys[r][table[r], :lens[r]]
    ctx = _hip.Context(q, 3, T, R, BIN_MS)
    try:
        ctx.upload_counts(Y)
        ctx.set_trial_lengths(lens)
        ctx.set_observed(table)
        ctx.set_option('cov_mode', 2)
        ctx.set_option('dual_lowrank', lowrank)
        ctx.set_params(params['C'], params['d'], params['tau'])
        lam = 0.2 + np.random.default_rng(5).random((R, q * T))
        with pytest.raises(_hip.HipBackendError):
            ctx.dual_costgrad_batch(None, lam)                             # the option is off: refused
        ctx.set_option('dual_masked', 1)
        live = np.zeros((R, q, T), bool)
        for r in range(R):
            live[r, table[r], :lens[r]] = True
        lam_in = np.where(live.reshape(R, -1), lam, np.nan)
        cost, grad = ctx.dual_costgrad_batch(None, lam_in)
        assert ctx.info('plan_lowrank') == float(lowrank)
        e_c = e_g = 0.0
        for r in range(R):
            L, o = int(lens[r]), table[r]
            pr = reduced_problem(('c1', r, L, o.tobytes()), params, Ys[r], o, L)
            lr = lam[r].reshape(q, T)[o][:, :L].reshape(-1)
            g_ref = orc.dual_grad(lr, *pr)
            e_c = max(e_c, abs(cost[r] - orc.dual_cost(lr, *pr)) / abs(orc.dual_cost(lr, *pr)))
            e_g = max(e_g, rel(grad[r].reshape(q, T)[o][:, :L].reshape(-1), g_ref))
            assert np.all(grad[r].reshape(q, T)[~live[r]] == 0.0)
            c1_, g1_ = ctx.dual_costgrad(r, lam_in[r])                     # (one trial: routed through the batched path while a table is set)
            assert c1_ == cost[r] and np.array_equal(g1_, grad[r])
        print('costgrad_batch, engine %d: cost %.2e, gradient %.2e' % (lowrank, e_c, e_g))
        assert e_c <= 1e-8 and e_g <= 1e-8
    finally:
        ctx.close()


# ---- 5. bit identity -----------------------------------------------------------------------------------------------------------------------------
def _run_ctx(ctx, R, want_pauto=True):
    rho, fopt, outer, status, lam = ctx.dual_fixed_point(None, max_outer=40, tol=1e-8, want_lam=True)
    ctx.dual_finalize(None, None)
    out = [lam, fopt, outer, status, ctx.post_mean(), ctx.post_vsm(), ctx.post_vsmgp()]
    if want_pauto:
        ctx.mstep_precomp()
        out.append(ctx.pautosum())
    return out


def _same_bits(a, b):
    same = [bool(np.array_equal(x, y)) for x, y in zip(a, b)]
    print('    bit-identical (lambda, cost, passes, status, post_mean, post_vsm, post_vsmGP[, PautoSum]): %s' % same)
    return all(same)


@pytest.mark.parametrize('lowrank', [0, 1], ids=['dense', 'lowrank'])
def test_no_table_and_full_tables_change_no_bit(funs_mod, lowrank):
    """The flag on with no table equals the flag off; an observation table of all ones changes no bit of lambda, cost, blocks or PautoSum under both
    engines; a length table of all T changes none under the low-rank engine; C[n] and d[n] of a neuron that no listed trial observes change none."""
    from funs import _hip
    g = load_golden('c1_dataset.npz')
    R, q, T = 6, 30, 100
    Y = np.ascontiguousarray(g['Y'][:R]).astype(np.uint8)
    C, d, tau = g['init_C'].copy(), g['init_d'].copy(), g['init_tau'].copy()

    def run(masked_opt, lengths=None, observed=None, Yin=Y, Cin=C, din=d):
        ctx = _hip.Context(q, 3, T, R, BIN_MS)
        try:
            ctx.upload_counts(Yin)
            if lengths is not None:
                ctx.set_trial_lengths(lengths)
            if observed is not None:
                ctx.set_observed(observed)
            ctx.set_option('cov_mode', 2)
            ctx.set_option('dual_lowrank', lowrank)
            ctx.set_option('keep_trial_vsmgp', 1)
            ctx.set_option('dual_masked', masked_opt)
            ctx.set_params(Cin, din, tau)
            out = _run_ctx(ctx, R)
            assert ctx.info('plan_lowrank') == float(lowrank) and np.all(out[3] == 0)
            return out
        finally:
            ctx.close()

    base = run(0)
    assert _same_bits(base, run(1)), 'the flag alone changed bits'
    assert _same_bits(base, run(1, observed=np.ones((R, q), bool))), 'an observation table of all ones changed bits'
    if lowrank:
        assert _same_bits(base, run(1, lengths=np.full(R, T, dtype=np.int32))), 'a length table of all T changed bits'
    # a neuron that no trial of the list observes (the table needs it observed somewhere: trial R - 1 keeps it and stays out of the list)
    table = np.ones((R, q), bool)
    table[:R - 1, 7] = False
    Y0 = Y.copy()
    Y0[:R - 1, 7] = 0
    C2, d2 = C.copy(), d.copy()
    C2[7] += 3.0
    d2[7] -= 2.0
    outs = []
    for Cin, din in ((C, d), (C2, d2)):
        ctx = _hip.Context(q, 3, T, R, BIN_MS)
        try:
            ctx.upload_counts(Y0)
            ctx.set_observed(table)
            ctx.set_option('cov_mode', 2)
            ctx.set_option('dual_lowrank', lowrank)
            ctx.set_option('keep_trial_vsmgp', 1)
            ctx.set_option('dual_masked', 1)
            ctx.set_params(Cin, din, tau)
            idx = np.arange(R - 1, dtype=np.int32)
            rho, fopt, outer, status, lam = ctx.dual_fixed_point(idx, max_outer=40, tol=1e-8, want_lam=True)
            ctx.dual_finalize(idx, None)
            outs.append([lam, fopt, outer, status, ctx.post_mean(idx), ctx.post_vsm(idx), ctx.post_vsmgp(idx)])
        finally:
            ctx.close()
    assert _same_bits(*outs), 'parameters of a neuron that no listed trial observes changed bits'


# ---- 6. warm start ---------------------------------------------------------------------------------------------------------------------------------
def test_warm_start_from_the_returned_optimum(masked):
    """a second call with the returned varOptimRes - resident, and as host arrays in lambda and in rho - converges in one pass to the same optimum"""
    params, Ys, T, lens = c1_problem(R=6)
    table = seam_table(len(Ys), Ys[0].shape[0])
    masked.DUAL_LOWRANK = True
    exp = experiment(Ys, lens, table)
    infRes, nll, vlb, optim = masked.dualVariational(exp, copy_params(params))
    check_contracted(masked, infRes)
    host = [np.array(optim[r]) for r in range(len(Ys))]
    for tag, prev, log in (('resident', optim, False), ('host', host, False)):
        ir, nll_w, vlb_w, opt_w = masked.dualVariational(exp, copy_params(params), prevOptimRes=prev)
        check_contracted(masked, ir)
        e = max(rel(opt_w[r], host[r]) for r in range(len(Ys)))
        print('warm start (%s): passes %s, lambda %.2e, cost %.2e' % (tag, ir.dual_iterations.tolist(), e, abs(vlb_w - vlb) / abs(vlb)))
        assert np.all(ir.dual_iterations <= 1) and e <= 1e-8 and abs(vlb_w - vlb) <= 1e-8 * abs(vlb) and abs(nll_w - nll) <= 1e-8 * abs(nll)
        optim = opt_w
    # the log-lambda variant: rho is 0 where lambda is 0, and comes back as a warm start too
    ir, _, vlb_l, opt_l = masked.dualVariational(exp, copy_params(params), optimizeLogLambda=True, prevOptimRes=[np.where(h > 0, np.log(np.where(h > 0, h, 1.0)), 0.0) for h in host])
    check_contracted(masked, ir)
    assert np.all(ir.dual_iterations <= 1) and abs(vlb_l - vlb) <= 1e-8 * abs(vlb)
    for r in range(len(Ys)):
        assert np.all(np.isfinite(opt_l[r])) and np.all(opt_l[r][host[r] == 0.0] == 0.0)


# ---- 7. EM -----------------------------------------------------------------------------------------------------------------------------------------
def cd_grad_observed(vec, Ys, pm, pv, table, p, q):
    """orc.mstep_cd_grad with the sums over observed (trial, neuron) pairs only, as test_gpu_observed_neurons.py takes it; the reference's 1 / numTrials stays"""
    C, d = orc.vec_to_cd(vec, p, q)
    dC, dd = np.zeros((q, p)), np.zeros(q)
    for Y, m, V, o in zip(Ys, pm, pv, table):
        _, a, b = orc.mstep_cd_terms(orc.cd_to_vec(C[o], d[o]), [np.asarray(Y, dtype=np.float64)[o]], [m], [V], p, int(o.sum()))
        dC[o] += a
        dd[o] += b
    return -orc.cd_to_vec(dC, dd) / len(Ys)


@pytest.mark.timeout(900)
def test_variational_em_on_two_stitched_sessions(masked, funs_mod):
    """PPGPFAfit(inferenceMethod='variational', maxEMiter=3, CdOptimMethod='newton') on config 1 stitched from two sessions (neurons 0..19 and 10..29)
    with ragged lengths: after the last M-step the oracle's (C,d) gradient over observed pairs at the variational posterior is <= 2e-6 and the
    timescale gradient on PautoSum <= 2e-5 = 1e-6 R (the limits test_gpu_observed_neurons.py holds the Laplace EM to); posteriorRates and
    posteriorSamples run on the fit's posterior, and the rate of an observed neuron equals numpy on the downloaded posterior (1e-9)."""
    g = load_golden('c1_dataset.npz')
    Ys = [g['Y'][r].astype(np.float64) for r in range(g['Y'].shape[0])]
    R, (q, T) = len(Ys), Ys[0].shape
    n = np.arange(q)
    table = np.stack([(n < 20) if r < R // 2 else (n >= 10) for r in range(R)])
    lens = np.array([T, 50, 73, 99, 64, 87, 51, 100, 66, 58, 91, 77, 83, 95, 60, 100, 55, 70, 89, 62][:R], dtype=np.int32)
    init = {'C': g['init_C'].copy(), 'd': g['init_d'].copy(), 'tau': g['init_tau'].copy()}
    exp = experiment(Ys, lens, table)
    masked.DUAL_LOWRANK = True
    fit = funs_mod.engine.PPGPFAfit(exp, initParams=copy_params(init), inferenceMethod='variational', EMmode='Batch', maxEMiter=3, CdOptimMethod='newton',
                                    quiet=True)
    new, prev, infRes = fit.optimParams, fit.paramSeq[-2], fit.infRes
    p = new['C'].shape[1]
    check_contracted(masked, infRes)
    assert infRes.session.ctx.info('trial_lengths_set') == 1.0 and infRes.session.ctx.info('observed_set') == 1.0
    Yr = [np.where(table[r][:, None], Ys[r][:, :lens[r]], 0.0) for r in range(R)]
    pm = [np.array(infRes['post_mean'][r]) for r in range(R)]
    pv = [np.array(infRes['post_vsm'][r]) for r in range(R)]
    P = infRes.session.ctx.pautosum()
    g_cd = float(np.max(np.abs(cd_grad_observed(orc.cd_to_vec(new['C'], np.asarray(new['d']).reshape(-1)), Yr, pm, pv, table, p, q))))
    logp = np.log(1.0 / (np.asarray(new['tau']).reshape(-1) * 1000.0 / BIN_MS) ** 2)
    g_tau = max(abs(orc.tau_grad(logp[k], P[k], R)[0]) for k in range(p))
    print('variational EM, 3 iterations: |(C,d) gradient| %.2e, |timescale gradient| %.2e, lower bound %s'
          % (g_cd, g_tau, np.asarray(fit.variationalLowerBound).tolist()))
    assert g_cd <= 2e-6 and g_tau <= 2e-5
    rates = funs_mod.util.posteriorRates(copy_params(prev), exp, infRes=infRes, want=('rate',))
    e_r = 0.0
    dprev = np.asarray(prev['d']).reshape(-1)
    for r in range(R):
        o = table[r]
        eta = prev['C'][o] @ pm[r] + dprev[o][:, None]
        var = np.einsum('nk,tkl,nl->nt', prev['C'][o], pv[r], prev['C'][o])
        e_r = max(e_r, rel(np.asarray(rates['rate'][r])[o], np.exp(eta + 0.5 * var) * 1000.0 / BIN_MS))
    print('posterior rates of the observed neurons against numpy on the downloaded posterior: %.2e' % e_r)
    assert e_r <= 1e-9
    smp = funs_mod.util.posteriorSamples(copy_params(prev), exp, infRes=infRes, nSamples=4, seed=1, want=('x',))
    assert len(smp['x']) == R and all(np.all(np.isfinite(np.asarray(x))) for x in smp['x'])
    # online EM on the same experiment runs too
    fit2 = funs_mod.engine.PPGPFAfit(exp, initParams=copy_params(init), inferenceMethod='variational', EMmode='Online', maxEMiter=2, batchSize=4, quiet=True)
    assert all(np.all(np.isfinite(np.asarray(fit2.optimParams[k]))) for k in ('C', 'd', 'tau'))


# ---- the refusals stay while the flag is off -----------------------------------------------------------------------------------------------------------
def test_refused_while_the_flag_is_off(funs_mod):
    from funs import _session
    assert funs_mod.inference.DUAL_MASKED is False
    params, Ys, T, lens = c1_problem(R=4)
    _session.drop_sessions()
    try:
        with pytest.raises(NotImplementedError):
            funs_mod.inference.dualVariational(experiment(Ys, lens), copy_params(params))
        with pytest.raises(NotImplementedError):
            funs_mod.inference.dualVariational(experiment(Ys, None, seam_table(4, 30)), copy_params(params))
    finally:
        _session.drop_sessions()
