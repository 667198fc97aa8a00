"""Pin the CPU oracle (oracle/pgpfa_oracle.py) against golden vectors captured from the
real reference (tests/golden/make_golden.py).  CPU only.  Tolerances follow SURVEY.md 8c."""
import numpy as np
import pytest

from conftest import load_golden
from oracle import pgpfa_oracle as orc


def rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(1e-300, np.max(np.abs(b)))


def test_gram_matches_reference_bitwise(c1):
    g = load_golden('c1_callbacks.npz')
    K = orc.make_K(c1['init_tau'], 100, c1['binSize'])
    assert np.max(np.abs(K - g['K'])) <= 1e-15


def test_vec_layout(c1):
    g = load_golden('c1_callbacks.npz')
    v = orc.cd_to_vec(c1['init_C'], c1['init_d'])
    assert np.array_equal(v, g['vecCd0'])
    C, d = orc.vec_to_cd(v, 3, 30)
    assert np.array_equal(C, c1['init_C']) and np.array_equal(d, c1['init_d'])


def test_callbacks_structured_and_big(c1):
    g = load_golden('c1_callbacks.npz')
    p, q, T = 3, 30, 100
    C, d = c1['init_C'], c1['init_d']
    K = orc.make_K(c1['init_tau'], T, c1['binSize'])
    Kb = orc.make_K_big(K)
    Kbi = np.linalg.inv(Kb)
    Cb, db = orc.make_Cd_big(C, d, T)
    x = g['xprobe']
    y = c1['Ys'][0].reshape(-1)
    # faithful big-matrix form: same arithmetic as the reference (summation order differs: 1e-10)
    assert abs(orc.nlp_big(x, y, Cb, db, Kbi) - g['f']) <= 1e-10 * abs(g['f'])
    assert rel(orc.nlp_big_grad(x, y, Cb, db, Kbi), g['g']) <= 1e-10
    assert rel(orc.nlp_big_hess(x, y, Cb, db, Kbi), g['H']) <= 1e-10
    # structured form (what the HIP kernels are diffed against): 1e-9 rel, SURVEY 8c
    Kinv = np.linalg.inv(K)
    X = x.reshape(p, T)
    assert abs(orc.nlp(X, c1['Ys'][0], C, d, Kinv) - g['f']) <= 1e-9 * abs(g['f'])
    assert rel(orc.nlp_grad(X, c1['Ys'][0], C, d, Kinv).reshape(-1), g['g']) <= 1e-9
    assert rel(orc.nlp_hess(X, c1['Ys'][0], C, d, Kinv), g['H']) <= 1e-9


def test_laplace_faithful_and_exact(c1):
    g = load_golden('c1_laplace.npz')
    Ys = c1['Ys'][:4]
    res, nll, opt = orc.laplace(Ys, c1['init'], c1['binSize'], mode='faithful')
    # same scipy driver, same callbacks -> same early-stopped answer up to rounding
    for r in range(4):
        assert np.max(np.abs(res['post_mean'][r] - g['post_mean'][r])) <= 1e-6
        assert rel(res['post_vsm'][r], g['post_vsm'][r]) <= 1e-6
    assert rel(res['post_cov'][0], g['post_cov_trial0']) <= 1e-6
    assert rel(res['post_vsmGP'][0], g['post_vsmGP_trial0']) <= 1e-6
    # exact mode vs the polished modes (Newton on the reference's own callbacks): 1e-8
    rese, nlle, _ = orc.laplace(Ys, c1['init'], c1['binSize'], mode='exact')
    for r in range(4):
        assert np.max(np.abs(rese['post_mean'][r].reshape(-1) - g['polished'][r])) <= 1e-8
        # raw oracle slack (reference stops early): SURVEY 8c, max|dx| <= 5e-3
        assert np.max(np.abs(rese['post_mean'][r] - g['post_mean'][r])) <= 5e-3
        d = [np.diag(rese['post_vsmGP'][r][:, :, k]) for k in range(3)]
        assert rel(np.stack(d), g['post_vsmGP_diag'][r]) <= 1e-3


def test_laplace_nll_all_trials(c1):
    g = load_golden('c1_laplace.npz')
    res, nll, _ = orc.laplace(c1['Ys'], c1['init'], c1['binSize'], mode='exact', return_cov=False)
    assert abs(nll - float(g['nll'])) <= 1e-4                       # SURVEY 8c |dnll| <= 1e-4
    P, R = orc.make_precomp(res)
    assert R == 20 and rel(P, g['PautoSum']) <= 1e-3


def test_mstep_cd_cost_grad(c1):
    g = load_golden('c1_mstep.npz')
    lap = load_golden('c1_laplace.npz')
    pm = [lap['post_mean'][r] for r in range(20)]
    pv = [lap['post_vsm'][r] for r in range(20)]
    args = (c1['Ys'], pm, pv, 3, 30)
    for v, c, gr in ((g['v0'], g['cost0'], g['grad0']), (g['v1'], g['cost1'], g['grad1'])):
        assert abs(orc.mstep_cd_cost(v, *args) - c) <= 1e-10 * abs(c)
        assert rel(orc.mstep_cd_grad(v, *args), gr) <= 1e-10
    inv_prior = -np.eye(g['v0'].size) / float(g['prior_step']) ** 2
    assert abs(orc.mstep_cd_cost_prior(g['v1'], g['v0'], inv_prior, *args) - g['costp']) <= 1e-10 * abs(g['costp'])
    assert rel(orc.mstep_cd_grad_prior(g['v1'], g['v0'], inv_prior, *args), g['gradp']) <= 1e-10


def _golden_infres():
    lap = load_golden('c1_laplace.npz')
    return lap


def test_tau_cost_grad(c1):
    g = load_golden('c1_mstep.npz')
    P = load_golden('c1_laplace.npz')['PautoSum']
    for k in range(3):
        for j, pv in enumerate(g['pprobe']):
            assert abs(orc.tau_cost(pv, P[k], 20) - g['tcost'][k, j]) <= 1e-9 * abs(g['tcost'][k, j])
            assert abs(orc.tau_grad(pv, P[k], 20)[0] - g['tgrad'][k, j]) <= 1e-8 * max(1.0, abs(g['tgrad'][k, j]))
            cp = orc.tau_cost_prior(pv, P[k], 20, c1['binSize'], c1['init_tau'][k], float(g['tau_prior_step']))
            gp = orc.tau_grad_prior(pv, P[k], 20, c1['binSize'], c1['init_tau'][k], float(g['tau_prior_step']))
            assert abs(cp - g['tcostp'][k, j]) <= 1e-9 * abs(g['tcostp'][k, j])
            assert abs(gp[0] - g['tgradp'][k, j]) <= 1e-8 * max(1.0, abs(g['tgradp'][k, j]))


def test_mstep_results_from_golden_estep(c1):
    """learnLTparams (TNC) and learnGPparams (BFGS) on the reference's own E-step output."""
    g = load_golden('c1_mstep.npz')
    res, _, _ = orc.laplace(c1['Ys'], c1['init'], c1['binSize'], mode='faithful', return_cov=False)
    C, d, cost, out = orc.learn_cd(c1['init'], c1['Ys'], res, 'TNC')
    v = orc.cd_to_vec(C, d)
    assert np.max(np.abs(v - orc.cd_to_vec(g['newC'], g['newd']))) <= 1e-4       # raw oracle slack
    assert np.max(np.abs(v - g['tight_vec'])) <= 1e-3
    tau, det = orc.learn_tau(c1['init'], res, c1['binSize'])
    assert np.max(np.abs(np.log(tau) - np.log(g['newTau']))) <= 1e-5


@pytest.mark.timeout(600)
def test_full_batch_em_matches_reference(c1):
    g = load_golden('c1_em_batch.npz')
    fit = orc.fit_batch(c1['Ys'], c1['init'], c1['binSize'], 3, 'TNC', mode='faithful')
    assert np.max(np.abs(np.asarray(fit['nll']) - g['nll'][:3])) <= 1e-3
    for i in range(1, 4):
        assert rel(fit['paramSeq'][i]['C'], g['seq_C'][i]) <= 1e-3
        assert rel(fit['paramSeq'][i]['tau'], g['seq_tau'][i]) <= 1e-3


def test_online_em_indices_and_values(c1):
    g = load_golden('c1_em_online.npz')
    np.random.seed(1)
    fit = orc.fit_online_diag(c1['Ys'], c1['init'], c1['binSize'], 4, 5, 'TNC', 'TNC', mode='faithful')
    assert np.array_equal(np.stack(fit['batchTrIdx']), g['batchTrIdx'])
    assert np.max(np.abs(np.asarray(fit['nll']) - g['nll'])) <= 1e-3
    assert rel(fit['paramSeq'][-1]['C'], g['seq_C'][-1]) <= 1e-3
    assert rel(fit['paramSeq'][-1]['tau'], g['seq_tau'][-1]) <= 2e-3


def test_variational_callbacks_and_estep():
    g = load_golden('var_toy.npz')
    Ys = [g['Y'][r].astype(float) for r in range(g['Y'].shape[0])]
    params = {'C': g['init_C'], 'd': g['init_d'], 'tau': g['init_tau']}
    T, q = 50, 20
    Cb, db = orc.make_Cd_big(params['C'], params['d'], T)
    Kb = orc.make_K_big(orc.make_K(params['tau'], T, float(g['binSize'])))
    Kbi = np.linalg.inv(Kb)
    yb = Ys[0].reshape(-1)
    assert abs(orc.dual_cost(g['lam_probe'], yb, Cb, Kb, Kbi, db) - g['dual_cost']) <= 1e-9 * abs(g['dual_cost'])
    assert rel(orc.dual_grad(g['lam_probe'], yb, Cb, Kb, Kbi, db), g['dual_grad']) <= 1e-9
    res, nll, vlb, opt = orc.dual_variational(Ys[:2], params, float(g['binSize']))
    for r in range(2):
        assert np.max(np.abs(res['post_mean'][r] - g['estep_post_mean'][r])) <= 1e-4
        assert rel(res['post_vsm'][r], g['estep_post_vsm'][r]) <= 1e-4


def test_c2_spot_exact_vs_reference():
    g = load_golden('c2_spot.npz')
    Ys = [g['Y'][r].astype(float) for r in range(1)]
    params = {'C': g['init_C'], 'd': g['init_d'], 'tau': g['init_tau']}
    res, nll, _ = orc.laplace(Ys, params, float(g['binSize']), mode='exact', return_cov=False)
    assert np.max(np.abs(res['post_mean'][0] - g['post_mean'][0])) <= 5e-3
    assert rel(res['post_vsm'][0], g['post_vsm'][0]) <= 1e-3


def test_leave_one_out_prediction_vs_reference(c1):
    """8f row 2: the oracle's faithful restatement against util.leaveOneOutPrediction itself (same fmin_ncg calls),
    and the exact-mode variant within the reference's early-stopping slack."""
    g = load_golden('c1_loo.npz')
    Ys = c1['Ys'][:2]
    pred, err = orc.leave_one_out_prediction(Ys, c1['init'], c1['binSize'], mode='faithful')
    # (same solver calls; the truncated-CG path amplifies the rounding differences of the Hessian products to ~1e-8)
    assert np.max(np.abs(pred - g['y_pred_mode'][:2])) <= 1e-6
    assert abs(err - 0) > 0
    pred_x, err_x = orc.leave_one_out_prediction(Ys[:1], c1['init'], c1['binSize'], mode='exact')
    assert np.max(np.abs(pred_x[0] - g['y_pred_mode'][0]) / g['y_pred_mode'][0]) <= 2e-2


def test_oracle_at_config3_dimensions_vs_reference_spot():
    """c3_spot.npz (tests/golden/make_golden_c3.py): one trial at 200 neurons x 10 latents x 500 bins pushed through the real
    reference's inference.laplace (~5 min there), then polished on the reference's own callbacks.  The oracle's structured exact
    mode must land on the polished mode (1e-9) with its covariance blocks (1e-10 rel), and within the reference's own
    early-stopping slack of the raw answer (measured 2.7e-5 / 3.4e-7)."""
    g = load_golden('c3_spot.npz')
    par = {'C': g['init_C'], 'd': g['init_d'], 'tau': g['init_tau']}
    res, nll, _ = orc.laplace([g['Y'][0].astype(float)], par, float(g['binSize']), mode='exact', return_cov=False)
    assert float(g['polished_grad_max']) <= 1e-10
    assert np.max(np.abs(res['post_mean'][0].reshape(-1) - g['polished'])) <= 1e-9
    assert abs(-nll - float(g['polished_f'])) <= 1e-12 * abs(float(g['polished_f']))
    assert rel(res['post_vsm'][0], g['polished_vsm']) <= 1e-10
    G = res['post_vsmGP'][0]
    assert rel(np.stack([np.diag(G[:, :, k]) for k in range(10)]), g['polished_vsmGP_diag']) <= 1e-10
    assert rel(G[::50, :, :], g['polished_vsmGP_rows']) <= 1e-10
    # the reference's raw output (scipy Newton-CG stopped at xtol 1e-5 on the mean |step|)
    assert np.max(np.abs(res['post_mean'][0] - g['post_mean'])) <= 5e-3
    assert abs(nll - float(g['nll'])) <= 1e-4
    assert rel(res['post_vsm'][0], g['post_vsm']) <= 1e-5


def test_oracle_with_counts_above_255():
    """Counts above one byte (tests/golden/c1_highcount.npz, captured from the reference): the oracle's callbacks, exact modes,
    (C,d) cost / gradient and dual callbacks against the reference's values."""
    g = load_golden('c1_highcount.npz')
    c1 = load_golden('c1_dataset.npz')
    Ys = [g['Y'][r].astype(float) for r in range(3)]
    par = {'C': c1['init_C'], 'd': c1['init_d'], 'tau': c1['init_tau']}
    q, p, T = 30, 3, 100
    K = orc.make_K(par['tau'], T, float(c1['binSize']))
    K_big = orc.make_K_big(K)
    Kinv_big = np.linalg.inv(K_big)
    C_big, d_big = orc.make_Cd_big(par['C'], par['d'], T)
    ybar = Ys[0].reshape(-1)
    assert abs(orc.nlp_big(g['xprobe'], ybar, C_big, d_big, Kinv_big) - float(g['f'])) <= 1e-12 * abs(float(g['f']))
    assert np.max(np.abs(orc.nlp_big_grad(g['xprobe'], ybar, C_big, d_big, Kinv_big) - g['g'])) <= 1e-10 * np.max(np.abs(g['g']))
    res, nll, _ = orc.laplace(Ys, par, float(c1['binSize']), mode='exact', return_cov=False)
    assert np.max(np.abs(np.stack(res['post_mean']).reshape(3, -1) - g['polished'])) <= 1e-9
    assert np.max(np.abs(np.stack(res['post_vsm']) - g['post_vsm_polished'])) <= 1e-9 * np.max(np.abs(g['post_vsm_polished']))
    ref_res = {'post_mean': list(g['post_mean']), 'post_vsm': list(g['post_vsm'])}
    assert abs(orc.mstep_cd_cost(g['v1'], Ys, ref_res['post_mean'], ref_res['post_vsm'], p, q) - float(g['cost1'])) <= 1e-12 * abs(float(g['cost1']))
    assert np.max(np.abs(orc.mstep_cd_grad(g['v1'], Ys, ref_res['post_mean'], ref_res['post_vsm'], p, q) - g['grad1'])) <= 1e-11 * np.max(np.abs(g['grad1']))
    assert abs(orc.dual_cost(g['lam'], ybar, C_big, K_big, Kinv_big, d_big) - float(g['dual_cost'])) <= 1e-10 * abs(float(g['dual_cost']))
    assert np.max(np.abs(orc.dual_grad(g['lam'], ybar, C_big, K_big, Kinv_big, d_big) - g['dual_grad'])) <= 1e-9 * np.max(np.abs(g['dual_grad']))


def test_laplace_cov_at_a_given_mode_vs_reference():
    """orc.laplace_cov_at - the dense FP64 yardstick (dpotrf / dpotri of the full p T x p T Hessian) that the GPU tests
    compare the covariance engine with at the DEVICE's modes - against the reference's own inverse (inference.py:130-172)
    at the reference's modes: c3_spot.npz's polished mode (200 x 10 x 500) and c1_laplace.npz's raw modes of all 20
    trials, blocks and PautoSum (learning.py:145-173) to 1e-10 of the largest entry."""
    g = load_golden('c3_spot.npz')
    p, T = 10, 500
    vsm, G = orc.laplace_cov_at(g['polished'].reshape(p, T), g['init_C'], g['init_d'], g['init_tau'], T, float(g['binSize']))
    e = (rel(vsm, g['polished_vsm']), rel(np.stack([np.diag(G[:, :, k]) for k in range(p)]), g['polished_vsmGP_diag']),
         rel(G[::50, :, :], g['polished_vsmGP_rows']))
    print('c3 polished: post_vsm %.2e, post_vsmGP diagonal %.2e, rows %.2e' % e)
    assert max(e) <= 1e-10
    c1 = load_golden('c1_dataset.npz')
    lap = load_golden('c1_laplace.npz')
    p, T = 3, 100
    P = np.zeros((p, T, T))
    worst = 0.0
    for r in range(lap['post_mean'].shape[0]):
        m = lap['post_mean'][r]
        vsm, G = orc.laplace_cov_at(m, c1['init_C'], c1['init_d'], c1['init_tau'], T, float(c1['binSize']))
        worst = max(worst, rel(vsm, lap['post_vsm'][r]))
        if r == 0:
            e0 = rel(G, lap['post_vsmGP_trial0'])
        for k in range(p):
            P[k] += G[:, :, k] + np.outer(m[k], m[k])
    eP = rel(P, lap['PautoSum'])
    print('c1 raw modes: post_vsm %.2e (worst of 20 trials), post_vsmGP trial 0 %.2e, PautoSum %.2e' % (worst, e0, eP))
    assert worst <= 1e-10 and e0 <= 1e-10 and eP <= 1e-10
