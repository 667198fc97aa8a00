"""The M-step kernels against plain FP64 numpy at the sizes where their loops run: a synthetic posterior goes in through Context.set_posterior
(no E-step: a failure points at the M-step alone) and every entry point is compared with a restatement of learning.py:20-91 / :175-255.

* A - the (C,d) passes (pgpfa_mstep_cd_costgrad, _newton_pass, _chord_pass, _cost_per_neuron) with MORE (trial, bin tile) items than
  workgroups, so that the stride loop, the prefetch of a following item and the (trial, tile) carry of the matrix-core forms run against
  a reference: the bench's 200 x 10 x 500 with 256 trials (8 / 32 items per workgroup), grids that are no multiple of the tiles per trial,
  tail tiles, counts above 255, template widths above p, a single latent, the vector kernels of 11..32 latents with 1 / 2 / 4 / 8 Hessian
  row groups, the vector kernels up to 10 latents (options cd_mfma = cd_hess_mfma = 0), without and with the prior.  Errors are taken PER
  NEURON (max_i |x_ni - ref_ni| / max_i |ref_ni|, then the largest over the neurons): a loud neuron must not hide a quiet one; a neuron's
  cost against its unsigned size sum (|y hh| + yhat) / R.
* A' - unsorted, non-contiguous trial lists beside trials whose posterior is NaN; the chord pass after the trial count changed.
* B - the timescale pass (pgpfa_mstep_tau_costgrad, _batch, _multi, _multi_begin / _end) at 500 bins x 10 latents (40 matrices padded to
  512, four 128-blocks), at exact multiples of the block, at 80 and 128 matrices in a batch and at a single one; every candidate of every
  latent at its own timescale, against orc.tau_cost / orc.tau_grad.  The gradient error is measured against the larger of its two terms,
  the cost error against R/2 |log det K| + 1/2 tr(K^-1 P): at a root the two gradient terms cancel and the cost changes sign along a scan.

Tolerances are those of the existing tests of the same quantities (test_mstep_many_neurons, test_cd_newton_pass_matrix_core_form,
test_mstep_tau_costgrad_vs_golden).  Every test prints the errors it measured."""
import time

import numpy as np
import pytest

from oracle import pgpfa_oracle as orc

pytestmark = pytest.mark.gpu

EPS = orc.EPS_NOISE
BIN_MS = 10.0
INV_S2 = 4.0
TOL = {'costgrad cost': 1e-10, 'costgrad grad': 1e-9, 'cost_n': 1e-11, 'delta': 1e-9, 'dec': 1e-9, 'sum of cost_n': 1e-12}
# 'sum of cost_n': pgpfa_mstep_cd_cost_per_neuron and pgpfa_mstep_cd_costgrad sum the same q per-neuron FP64 numbers; the two orders differ by at
# most q eps = 200 x 1.1e-16 = 2.2e-14 of the unsigned size

# (q, p, T, R) -> what the launch code makes of it (cd_sweep: 64 bins per item on min(items, max(64, 512 / groups)) workgroups, groups of 8 neuron
# tiles; Newton pass: 32 bins per item on at most 128 workgroups; vector kernels: 32 / 16 / 8 bins per item at widths 12-16 / 20 / 32)
CD_CASES = {
    'bench':    (200, 10, 500, 256),   # 2048 / 4096 items on 256 / 128 workgroups, 13 neuron tiles in groups of 7 and 6, the last tile half full
    'carry':    (200, 10, 301, 70),    # 350 / 700 items on 256 / 128 workgroups, 256 % 5 and 128 % 10 != 0, tail tile of 45 bins, counts above 255
    'narrow':   (77, 7, 333, 100),     # p below its template width, one group, 600 items on 512 workgroups (512 % 6), 1100 on 128 (128 % 11)
    'groups54': (130, 3, 203, 150),    # 9 neuron tiles in groups of 5 and 4, T % 4 = 3
    'single':   (17, 1, 150, 80),      # one latent, two neuron tiles
    'wide12':   (60, 12, 150, 40),     # vector sweep and mstep_cd_hess_kernel, 200 items on 160 / 128 workgroup rows
    'wide16':   (70, 16, 132, 40),     # mstep_cd_hess_rows_kernel with 2 row groups
    'wide20':   (90, 20, 100, 40),     # 4 row groups, 280 items
    'wide27':   (50, 27, 70, 40),      # 8 row groups, 360 items
}
CD_RUNS = [(name, 'default') for name in CD_CASES] + [('carry', 'vector'), ('narrow', 'vector')]


# ---- part A: synthetic posterior and the numpy reference ---------------------------------------------------------------------------------
def _rbf(tau_bins, T):
    idx = np.arange(T, dtype=np.float64)
    return (1.0 - EPS) * np.exp(-0.5 * (idx[:, None] - idx[None, :]) ** 2 / tau_bins ** 2) + EPS * np.eye(T)


def _cd_problem(q, p, T, R, seed, plant=False):
    """C = 0.4 randn / sqrt(p), rates log-uniform in [0.02, 2] per bin, means sqrt(0.7) L_k z with timescales log-uniform in [3, 60] bins,
    post_vsm[r][t] = 0.3 (A A^T / p + 0.1 I) (symmetric), counts Poisson from exp(C m + d + c^T V c / 2); plant: counts above 255 in a few
    entries of the first and of the last neuron tile (first, middle and last bins: the tail tile too)."""
    rng = np.random.default_rng(seed)
    C = 0.4 * rng.standard_normal((q, p)) / np.sqrt(p)
    d = rng.uniform(np.log(0.02), np.log(2.0), q)                      # log of the rate per bin
    tau = np.exp(rng.uniform(np.log(3.0), np.log(60.0), p))
    L = [np.linalg.cholesky(_rbf(t, T)) for t in tau]
    M = np.stack([np.stack([np.sqrt(0.7) * L[k] @ rng.standard_normal(T) for k in range(p)]) for _ in range(R)])        # (R,p,T)
    A = rng.standard_normal((R, T, p, p))
    V = 0.3 * (A @ A.transpose(0, 1, 3, 2) / p + 0.1 * np.eye(p))                                                         # (R,T,p,p)
    del A
    Y = np.empty((R, q, T), dtype=np.uint16)
    for r in range(R):
        h = C @ M[r] + d[:, None] + 0.5 * np.einsum('nk,tkl,nl->nt', C, V[r], C)
        Y[r] = rng.poisson(np.exp(h))
    if plant:
        for r, n, t, y in ((0, 0, 0, 256), (R - 1, 15, T - 1, 300), (R // 2, 3, T // 2, 1000), (1, q - 1, T - 1, 511), (R - 1, q - 8, 0, 260),
                           (R - 2, q - 3, T - 14, 777)):
            Y[r, n, t] = y
    v0 = orc.cd_to_vec(C, d) + 0.01 * rng.standard_normal(q * (p + 1))
    center = v0 - 0.05 * rng.standard_normal(q * (p + 1))
    return {'dims': (q, p, T, R), 'C': C, 'd': d, 'tau_s': tau * BIN_MS / 1000.0, 'M': M, 'V': V, 'Y': Y, 'v0': v0, 'center': center}


def _cd_sums(vec, M, V, Y, want_hess=True, chunk=8):
    """Per neuron, summed over the trials given and all bins, FP64: cost -(y hh - yhat), its unsigned size |y hh| + yhat, gradient
    yhat w - y [m, 1] (q, p+1), Hessian yhat w w^T + [yhat V, 0; 0, 0] (q, p+1, p+1); hh = d_n + c_n.m_t, yhat = exp(hh + c_n^T V_t c_n / 2),
    w = [m_t + V_t c_n, 1].  Not divided by the trial count."""
    R, p, T = M.shape
    q = Y.shape[1]
    D = p + 1
    vv = np.asarray(vec, dtype=np.float64).reshape(D, q)
    Cn, dn = np.ascontiguousarray(vv[:p].T), vv[p]
    cost, size, g, H = np.zeros(q), np.zeros(q), np.zeros((q, D)), np.zeros((q, D, D))
    for r0 in range(0, R, chunk):
        mt = M[r0:r0 + chunk].transpose(0, 2, 1).reshape(-1, p)              # (X,p), X = trials of the chunk x bins
        vt = V[r0:r0 + chunk].reshape(-1, p, p)                              # (X,p,p)
        yy = Y[r0:r0 + chunk].astype(np.float64).transpose(1, 0, 2).reshape(q, -1)
        Vc = np.einsum('xkl,nl->nxk', vt, Cn)                                # (q,X,p)
        hh = dn[:, None] + Cn @ mt.T                                         # (q,X)
        yh = np.exp(hh + 0.5 * np.einsum('nxk,nk->nx', Vc, Cn))
        w = np.concatenate([mt[None] + Vc, np.ones((q, mt.shape[0], 1))], axis=2)
        cost -= np.sum(yy * hh - yh, axis=1)
        size += np.sum(np.abs(yy * hh) + yh, axis=1)
        g += np.einsum('nx,nxi->ni', yh, w)
        g[:, :p] -= yy @ mt
        g[:, p] -= yy.sum(axis=1)
        if want_hess:
            H += np.matmul((w * yh[:, :, None]).transpose(0, 2, 1), w)
            H[:, :p, :p] += np.einsum('nx,xkl->nkl', yh, vt)
    return cost, size, g, H


def _with_prior(vec, sums, ntr, center):
    """means over ntr trials of the sums above, plus the prior inv_s2 / 2 |v_n - center_n|^2 where center is given: cost_n, size_n, g, H"""
    cost, size, g, H = sums
    q, D = g.shape
    cost, size, g, H = cost / ntr, size / ntr, g / ntr, H / ntr
    if center is not None:
        dv = (np.asarray(vec) - center).reshape(D, q).T
        pr = 0.5 * INV_S2 * np.sum(dv * dv, axis=1)
        cost, size, g, H = cost + pr, size + pr, g + INV_S2 * dv, H + INV_S2 * np.eye(D)
    return cost, size, g, H


def _step(g, H):
    delta = -np.linalg.solve(H, g[:, :, None])[:, :, 0]
    return delta, -np.einsum('ni,ni->n', g, delta)


def _rows(x, ref):
    """largest over the neurons of max_i |x_ni - ref_ni| / max_i |ref_ni|; x in the vecCd layout (p+1, q), ref (q, p+1)"""
    x = np.asarray(x).reshape(ref.shape[1], ref.shape[0]).T
    return float(np.max(np.max(np.abs(x - ref), axis=1) / np.max(np.abs(ref), axis=1)))


def _each(x, ref, size=None):
    return float(np.max(np.abs(np.asarray(x) - ref) / (np.abs(ref) if size is None else size)))


def _check_inputs(tag, Y, H0, gs):
    """the conditions that keep a comparison from being vacuous, on the reference side"""
    rate = Y.mean(axis=(0, 2))
    cond = np.array([np.linalg.cond(h) for h in H0])
    gmin = min(float(np.min(np.max(np.abs(g), axis=1))) for g in gs)
    print('%s inputs: mean counts per bin %.3f-%.3f, largest count %d, Hessian condition numbers <= %.1f, smallest max_i |g_ni| %.3f'
          % (tag, rate.min(), rate.max(), int(Y.max()), cond.max(), gmin))
    assert rate.min() >= 0.01 and cond.max() <= 1e4 and gmin >= 1e-3


def _report(tag, errs):
    print('%s: %s' % (tag, ', '.join('%s %.2e' % (k, e) for k, e, _ in errs)))
    bad = [(k, e, tol) for k, e, tol in errs if not e <= tol]
    assert not bad, '%s: %s' % (tag, ', '.join('%s %.2e > %.0e' % b for b in bad))


def _compare_entry_points(tag, ctx, v0, v1, center, ref0, ref1, ref_chord=None):
    """All four entry points against the reference: ref0 / ref1 = (cost_n, size_n, g, H) at v0 / v1 (H at v1 unused); the chord pass at v1
    follows the Newton pass at v0 and uses ITS Hessians (ref_chord: another Hessian set to use instead of ref0's)."""
    kw = {} if center is None else {'prior_center': center, 'inv_s2': INV_S2}
    errs = []
    cost, grad = ctx.mstep_cd_costgrad(v0, **kw)
    assert np.isfinite(cost) and np.all(np.isfinite(grad))
    errs.append(('costgrad cost', abs(cost - ref0[0].sum()) / ref0[1].sum(), TOL['costgrad cost']))
    errs.append(('costgrad grad', _rows(grad, ref0[2]), TOL['costgrad grad']))
    cost_n, delta, dec = ctx.mstep_cd_newton_pass(v0, **kw)
    assert np.all(np.isfinite(cost_n)) and np.all(np.isfinite(delta)) and np.all(np.isfinite(dec))
    d_ref, dec_ref = _step(ref0[2], ref0[3])
    errs.append(('newton cost_n', _each(cost_n, ref0[0], ref0[1]), TOL['cost_n']))
    errs.append(('newton delta', _rows(delta, d_ref), TOL['delta']))
    errs.append(('newton dec', _each(dec, dec_ref), TOL['dec']))
    cost_n, delta, dec = ctx.mstep_cd_chord_pass(v1, **kw)
    assert np.all(np.isfinite(cost_n)) and np.all(np.isfinite(delta)) and np.all(np.isfinite(dec))
    d_ref, dec_ref = _step(ref1[2], ref0[3] if ref_chord is None else ref_chord)
    errs.append(('chord cost_n', _each(cost_n, ref1[0], ref1[1]), TOL['cost_n']))
    errs.append(('chord delta', _rows(delta, d_ref), TOL['delta']))
    errs.append(('chord dec', _each(dec, dec_ref), TOL['dec']))
    cost_n = ctx.mstep_cd_cost_per_neuron(v1, **kw)
    cost, grad = ctx.mstep_cd_costgrad(v1, **kw)
    errs.append(('cost_per_neuron', _each(cost_n, ref1[0], ref1[1]), TOL['cost_n']))
    errs.append(('its sum vs costgrad', abs(cost_n.sum() - cost) / ref1[1].sum(), TOL['sum of cost_n']))
    errs.append(('costgrad cost at v1', abs(cost - ref1[0].sum()) / ref1[1].sum(), TOL['costgrad cost']))
    errs.append(('costgrad grad at v1', _rows(grad, ref1[2]), TOL['costgrad grad']))
    _report(tag, errs)
    return errs


_cd_cache = {}


def _cd_case(name):
    """problem and reference sums of a case, computed once and shared by its tests (one case resident at a time)"""
    if name not in _cd_cache:
        _cd_cache.clear()
        q, p, T, R = CD_CASES[name]
        t0 = time.time()
        pr = _cd_problem(q, p, T, R, seed=1000 + 7 * q + T, plant=(name == 'carry'))
        s0 = _cd_sums(pr['v0'], pr['M'], pr['V'], pr['Y'])
        delta0, _ = _step(*_with_prior(pr['v0'], s0, R, None)[2:])
        pr['v1'] = pr['v0'] + 0.3 * delta0.T.reshape(-1)
        s1 = _cd_sums(pr['v1'], pr['M'], pr['V'], pr['Y'], want_hess=False)
        pr['sums'] = (s0, s1)
        print('%s %s: problem and FP64 reference at two points in %.1f s' % (name, (q, p, T, R), time.time() - t0))
        _cd_cache[name] = pr
    return _cd_cache[name]


def _context(pr, options=()):
    from funs import _hip
    q, p, T, R = pr['dims']
    ctx = _hip.Context(q, p, T, R, BIN_MS)
    try:
        Y = pr['Y']
        ctx.upload_counts(Y if Y.max() > 255 else Y.astype(np.uint8))
        for key, value in options:
            ctx.set_option(key, value)
        ctx.set_params(pr['C'], pr['d'], pr['tau_s'])
    except Exception:
        ctx.close()
        raise
    return ctx


@pytest.mark.timeout(1200)
@pytest.mark.parametrize('prior', [False, True], ids=['plain', 'prior'])
@pytest.mark.parametrize('name,form', CD_RUNS, ids=['%s-%s' % r for r in CD_RUNS])
def test_cd_passes_against_numpy(name, form, prior):
    """Part A.  costgrad (cost, gradient), newton_pass (cost_n, delta, dec) at v0 = vec(C, d) + 0.01 randn, chord_pass (cost_n, delta, dec with
    the Hessians of v0) and cost_per_neuron at v1 = v0 + 0.3 delta_ref(v0), without and with the prior (center = v0 - 0.05 randn, inv_s2 = 4),
    per neuron: costgrad cost 1e-10, gradient 1e-9, per-neuron cost 1e-11, delta and dec 1e-9.  form 'vector': options cd_mfma = 0 and
    cd_hess_mfma = 0, the vector kernels up to 10 latents against the same reference.
    Measured (worst case; at the bench's dimensions): costgrad cost 3.8e-16, gradient 7.1e-14 (3.1e-14), per-neuron cost 6.8e-16, Newton delta
    4.1e-14 (1.4e-14), dec 4.5e-14 (5.4e-15), chord delta 7.5e-14 (3.2e-14), dec 7.1e-14 (1.5e-14); docs/history/mstep_dense_tests.md."""
    pr = _cd_case(name)
    q, p, T, R = pr['dims']
    center = pr['center'] if prior else None
    ref0 = _with_prior(pr['v0'], pr['sums'][0], R, center)
    ref1 = _with_prior(pr['v1'], pr['sums'][1], R, center)
    tag = '%s %s %s%s' % (name, pr['dims'], form, ' with prior' if prior else '')
    _check_inputs(tag, pr['Y'], ref0[3], (ref0[2], ref1[2]))
    if name == 'carry':
        assert pr['Y'].max() > 255
    ctx = _context(pr, (('cd_mfma', 0), ('cd_hess_mfma', 0)) if form == 'vector' else ())
    try:
        if name == 'carry':
            assert ctx.info('counts_two_bytes') == 1.0
        ctx.set_posterior(None, pr['M'], pr['V'])
        _compare_entry_points(tag, ctx, pr['v0'], pr['v1'], center, ref0, ref1)
    finally:
        ctx.close()


@pytest.mark.parametrize('prior', [False, True], ids=['plain', 'prior'])
def test_cd_passes_over_an_unsorted_trial_list(prior):
    """Part A'.  48 trials at 77 x 7 x 333: the posterior of all 48 set to NaN, then set for a list of 29 trials, unsorted and non-contiguous.
    Every entry point returns finite values equal to the reference over exactly those 29: nothing outside the list is read (290 / 319 items
    on 290 / 128 workgroups).  Tolerances of part A.
    Measured: costgrad gradient 4.2e-14, per-neuron cost 5.2e-16, Newton delta 3.0e-14, chord delta 4.5e-14, dec 2.2e-14."""
    q, p, T, R = 77, 7, 333, 48
    pr = _cd_problem(q, p, T, R, seed=4848)
    rng = np.random.default_rng(29)
    lst = rng.permutation(R)[:29].astype(np.int32)
    assert np.any(np.diff(lst) < 0) and len(set(np.diff(np.sort(lst)))) > 1
    M, V, Y = pr['M'][lst], pr['V'][lst], pr['Y'][lst]
    center = pr['center'] if prior else None
    s0 = _cd_sums(pr['v0'], M, V, Y)
    v1 = pr['v0'] + 0.3 * _step(*_with_prior(pr['v0'], s0, len(lst), None)[2:])[0].T.reshape(-1)
    s1 = _cd_sums(v1, M, V, Y, want_hess=False)
    ref0, ref1 = _with_prior(pr['v0'], s0, len(lst), center), _with_prior(v1, s1, len(lst), center)
    tag = 'list of 29 out of 48%s' % (' with prior' if prior else '')
    _check_inputs(tag, Y, ref0[3], (ref0[2], ref1[2]))
    ctx = _context(pr)
    try:
        ctx.set_posterior(None, np.full_like(pr['M'], np.nan), np.full_like(pr['V'], np.nan))
        ctx.set_posterior(lst, M, V)
        _compare_entry_points(tag, ctx, pr['v0'], v1, center, ref0, ref1)
    finally:
        ctx.close()


@pytest.mark.parametrize('prior', [False, True], ids=['plain', 'prior'])
def test_chord_pass_after_the_trial_count_changed(prior):
    """Part A'.  Newton pass over 40 trials at v0, set_posterior over 24 OTHER trials, chord pass at v1: the step is
    -(H_40(v0) / 40)^-1 (g_24(v1) / 24) - every mean over its own count - and dec = g^T H^-1 g likewise; cost_n over the 24 (64 trials at
    77 x 7 x 333).  Before the fix the Hessian sums of the 40 were divided by 24: steps 0.6 times too short.  Tolerances of part A.
    Measured: Newton delta 3.4e-14, dec 1.3e-14, chord delta 6.2e-14, dec 2.7e-14, per-neuron cost 4.2e-16."""
    q, p, T, R = 77, 7, 333, 64
    pr = _cd_problem(q, p, T, R, seed=6424)
    rng = np.random.default_rng(40)
    perm = rng.permutation(R).astype(np.int32)
    la, lb = perm[:40], perm[40:]
    center = pr['center'] if prior else None
    sa = _cd_sums(pr['v0'], pr['M'][la], pr['V'][la], pr['Y'][la])
    refa = _with_prior(pr['v0'], sa, 40, center)
    v1 = pr['v0'] + 0.3 * _step(*_with_prior(pr['v0'], sa, 40, None)[2:])[0].T.reshape(-1)
    sb = _cd_sums(v1, pr['M'][lb], pr['V'][lb], pr['Y'][lb], want_hess=False)
    refb = _with_prior(v1, sb, 24, center)
    tag = 'Newton over 40 trials, chord over 24 others%s' % (' with prior' if prior else '')
    _check_inputs(tag, pr['Y'], refa[3], (refa[2], refb[2]))
    ctx = _context(pr)
    try:
        kw = {} if center is None else {'prior_center': center, 'inv_s2': INV_S2}
        ctx.set_posterior(la, pr['M'][la], pr['V'][la])
        cost_n, delta, dec = ctx.mstep_cd_newton_pass(pr['v0'], **kw)
        d_ref, dec_ref = _step(refa[2], refa[3])
        errs = [('newton cost_n', _each(cost_n, refa[0], refa[1]), TOL['cost_n']), ('newton delta', _rows(delta, d_ref), TOL['delta']),
                ('newton dec', _each(dec, dec_ref), TOL['dec'])]
        ctx.set_posterior(lb, pr['M'][lb], pr['V'][lb])
        cost_n, delta, dec = ctx.mstep_cd_chord_pass(v1, **kw)
        d_ref, dec_ref = _step(refb[2], refa[3])
        errs += [('chord cost_n', _each(cost_n, refb[0], refb[1]), TOL['cost_n']), ('chord delta', _rows(delta, d_ref), TOL['delta']),
                 ('chord dec', _each(dec, dec_ref), TOL['dec'])]
        # a second chord pass finds the same Hessians and the same count behind them
        cost_n2, delta2, dec2 = ctx.mstep_cd_chord_pass(v1, **kw)
        assert np.array_equal(cost_n, cost_n2) and np.array_equal(delta, delta2) and np.array_equal(dec, dec2)
        _report(tag, errs)
    finally:
        ctx.close()


# ---- part B: the timescale pass ---------------------------------------------------------------------------------------------------------------
TAU_SHAPES = [(10, 500), (10, 301), (3, 203), (5, 128), (2, 129), (20, 130), (32, 64), (1, 17)]
SCALES = (0.25, 0.7, 1.0, 1.4, 4.0)


def _tau_problem(p, T, seed):
    q, R = 4, 3
    rng = np.random.default_rng(seed)
    hi = max(1.0, T / 8.0)
    tau = np.exp(rng.uniform(0.0, np.log(hi), p))                   # bins
    tau[0] = 1.0
    tau[-1] = hi
    K = np.stack([_rbf(t, T) for t in tau])
    L = np.linalg.cholesky(K)
    M = np.stack([np.stack([np.sqrt(0.7) * L[k] @ rng.standard_normal(T) for k in range(p)]) for _ in range(R)])        # (R,p,T)
    G = np.stack([0.3 * K.transpose(1, 2, 0)] * R)                                                                        # (R,T,T,p)
    V = np.stack([np.stack([0.3 * np.eye(p)] * T)] * R)
    C = 0.4 * rng.standard_normal((q, p)) / np.sqrt(p)
    d = np.full(q, -1.0)
    Y = rng.poisson(np.exp(np.einsum('nk,rkt->rnt', C, M) + d[None, :, None])).astype(np.uint8)
    logp = np.array([[-2.0 * np.log(tau[k] * SCALES[(j + k) % 5]) for k in range(p)] for j in range(5)])                # candidate-major
    return {'q': q, 'R': R, 'tau': tau, 'M': M, 'G': G, 'V': V, 'C': C, 'd': d, 'Y': Y, 'logp': logp}


def _tau_reference(logp, P, R):
    """orc.tau_cost / orc.tau_grad entry by entry, the two terms of the gradient a = -R/2 tr(K^-1 M) gamma and b = 1/2 tr(K^-1 M K^-1 P) gamma,
    the unsigned size of the cost R/2 |log det K| + 1/2 tr(K^-1 P) and cond(K)"""
    m, p = logp.shape
    T = P.shape[1]
    out = {k: np.empty((m, p)) for k in ('cost', 'grad', 'gsize', 'csize', 'cond')}
    for j in range(m):
        for k in range(p):
            pv = logp[j, k]
            out['cost'][j, k] = orc.tau_cost(pv, P[k], R)
            out['grad'][j, k] = orc.tau_grad(pv, P[k], R)[0]
            K, dK = orc._tau_pieces(pv, T, EPS)
            np.linalg.cholesky(K)
            Ki = np.linalg.inv(K)
            KiM = Ki @ dK
            a = -0.5 * R * np.trace(KiM) * np.exp(pv)
            b = 0.5 * np.sum((KiM @ Ki) * P[k].T) * np.exp(pv)
            out['gsize'][j, k] = max(abs(a), abs(b))
            out['csize'][j, k] = 0.5 * R * abs(np.linalg.slogdet(K)[1]) + 0.5 * np.sum(Ki * P[k])
            out['cond'][j, k] = np.linalg.cond(K)
    return out


@pytest.mark.timeout(1200)
@pytest.mark.parametrize('p,T', TAU_SHAPES, ids=['%dx%d' % s for s in TAU_SHAPES])
def test_timescale_pass_against_numpy(p, T):
    """Part B.  q = 4, R = 3, posterior through set_posterior with post_vsmGP = 0.3 K(tau_k) per latent and means drawn from K(tau_k); tau_k
    log-uniform between 1 bin and T / 8, the first latent at 1 bin, the last at T / 8.  mstep_precomp returns 3 and PautoSum equals
    orc.make_precomp to 1e-12.  Candidate j of latent k at tau_k s[(j + k) % 5], s = (0.25, 0.7, 1, 1.4, 4): no two entries of a pass share a
    value.  m = 1..4: _multi entry by entry (cost 1e-9 of R/2 |log det K| + 1/2 tr(K^-1 P), gradient 1e-8 of the larger of its two terms),
    _batch == row 0, the single-latent entry point at every (j, k), _multi_begin / _end the bits of _multi, m = 5 refused; while a pass is in
    flight mstep_precomp, _multi and the single-latent entry point raise and the pass is still collected with the right bits.
    Measured: cost 2.9e-12 (10 x 301), gradient 8.5e-12 (10 x 500, single-latent entry point); PautoSum 3.1e-16.  Before sum_part_batch_kernel
    was launched over all queries, the passes with more than 64 of them (20 x 130 at m = 4, 32 x 64 at m = 3, 4) returned stale traces: cost
    errors of 23 and 1.4e4 on this scale."""
    from funs import _hip
    pr = _tau_problem(p, T, seed=100 * p + T)
    R = pr['R']
    P_ref, n_ref = orc.make_precomp({'post_mean': list(pr['M']), 'post_vsmGP': list(pr['G'])})
    ref = _tau_reference(pr['logp'][:4], P_ref, R)
    tag = 'timescale pass %d latents x %d bins' % (p, T)
    print('%s: timescales %.2f-%.2f bins, probes %.2f-%.2f bins, cond(K) <= %.1e'
          % (tag, pr['tau'].min(), pr['tau'].max(), np.exp(-0.5 * pr['logp'][:4].max()), np.exp(-0.5 * pr['logp'][:4].min()), ref['cond'].max()))
    assert ref['cond'].max() <= 1e7 and len(np.unique(pr['logp'][:4])) == 4 * p
    ctx = _hip.Context(pr['q'], p, T, R, BIN_MS)
    try:
        ctx.upload_counts(pr['Y'])
        ctx.set_params(pr['C'], pr['d'], pr['tau'] * BIN_MS / 1000.0)
        ctx.set_posterior(None, pr['M'], pr['V'], pr['G'])
        assert ctx.mstep_precomp() == 3.0 and n_ref == 3
        e_p = np.max(np.abs(ctx.pautosum() - P_ref)) / np.max(np.abs(P_ref))
        print('%s: PautoSum %.2e' % (tag, e_p))
        assert e_p <= 1e-12
        errs, out = [], {}
        for m in (1, 2, 3, 4):
            Q = pr['logp'][:m]
            cost, grad = ctx.mstep_tau_costgrad_multi(Q)
            assert cost.shape == (m, p) and np.all(np.isfinite(cost)) and np.all(np.isfinite(grad))
            errs.append(('multi m=%d cost' % m, float(np.max(np.abs(cost - ref['cost'][:m]) / ref['csize'][:m])), 1e-9))
            errs.append(('multi m=%d grad' % m, float(np.max(np.abs(grad - ref['grad'][:m]) / ref['gsize'][:m])), 1e-8))
            ctx.mstep_tau_costgrad_multi_begin(Q)
            c2, g2 = ctx.mstep_tau_costgrad_multi_end()
            assert np.array_equal(cost, c2) and np.array_equal(grad, g2), 'begin / end differs from multi at m=%d' % m
            out[m] = (cost, grad)
        cb, gb = ctx.mstep_tau_costgrad_batch(pr['logp'][0])
        assert np.array_equal(cb, out[1][0][0]) and np.array_equal(gb, out[1][1][0])
        errs.append(('batch cost', float(np.max(np.abs(cb - ref['cost'][0]) / ref['csize'][0])), 1e-9))
        errs.append(('batch grad', float(np.max(np.abs(gb - ref['grad'][0]) / ref['gsize'][0])), 1e-8))
        one = np.array([[ctx.mstep_tau_costgrad(k, pr['logp'][j, k]) for k in range(p)] for j in range(4)])               # (4, p, 2)
        assert np.all(np.isfinite(one))
        errs.append(('single cost', float(np.max(np.abs(one[:, :, 0] - ref['cost']) / ref['csize'])), 1e-9))
        errs.append(('single grad', float(np.max(np.abs(one[:, :, 1] - ref['grad']) / ref['gsize'])), 1e-8))
        with pytest.raises(_hip.HipBackendError):
            ctx.mstep_tau_costgrad_multi(pr['logp'][:5])
        with pytest.raises(_hip.HipBackendError):
            ctx.mstep_tau_costgrad_multi_begin(pr['logp'][:5])
        # while a pass is in flight the other timescale / precomp entry points fail and leave it alone
        ctx.mstep_tau_costgrad_multi_begin(pr['logp'][:4])
        try:
            with pytest.raises(_hip.HipBackendError):
                ctx.mstep_precomp()
            with pytest.raises(_hip.HipBackendError):
                ctx.mstep_tau_costgrad_multi(pr['logp'][:2])
            with pytest.raises(_hip.HipBackendError):
                ctx.mstep_tau_costgrad(0, pr['logp'][0, 0])
        finally:
            c2, g2 = ctx.mstep_tau_costgrad_multi_end()
        assert np.array_equal(out[4][0], c2) and np.array_equal(out[4][1], g2)
        _report(tag, errs)
    finally:
        ctx.close()
