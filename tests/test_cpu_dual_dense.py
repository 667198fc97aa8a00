"""The bounds of tests/test_gpu_dual_dense.py can be met and have teeth, shown without a GPU on the very inputs the GPU test uses.

* `mirror`, a float64 numpy restatement of the GEMM form of the dual evaluation (the pair / loading table with its npd padding, pair order
  a (a + 1) / 2 + b, Sp with the weights 1 and 2, partial sums per 64-bin tile, the jitter), meets every bound of sections A to D against the longdouble
  reference, with ratio at most 1, at every case.
* The same with one fault misses a bound by a factor of 1000 or more in every case in which the fault is defined (`fault_defined`):
    pair_shift    the pair index one too far, in both transposes                              two latents or more
    weight_one    off-diagonal weight 1 in Sp where dual_pack_sigma_kernel owes 2             two latents or more
    lost_neuron   the last neuron with n % 4 == 3 never visited by dual_pre_kernel's wave 3   four neurons or more
    sd_tail       the tile tail t >= 64 floor(T / 64) dropped from sum lambda (log lambda - 1) T no multiple of 64
    unpack_tail   the tail of the last transpose tile of dual_unpack_w_kernel left unstored    T no multiple of its tile (32 / 16 / 8 bins)
    pack_tail     the same in dual_pack_sigma_kernel                                          T no multiple of its tile (32 / 16 / 8 / 4 bins)
    no_jitter     the 1e-6 relative jitter on the diagonal left out
    alpha_plus    alpha = +1/2 in the gradient's product with the pair table
    hi_ignored    the second count plane not read                                             the case with counts above 255
    finish_twice  log lambda - d added twice
* Section D's bound is at most 1e-3 of the median variance term 1/2 c_n^T Sigma_t c_n in every case, so a variance term 0.1 % wrong fails.
* FP64 numpy's own error in the log-determinant and in the Sigma_t blocks, against a longdouble evaluation (Gram inverses, precision, Cholesky factor and
  inverse in longdouble, vectorised by column), at the cases with n = p T <= 400: the model behind tau_logdet of the dense engine."""
import numpy as np
import pytest

import test_gpu_dual_dense as gk

LD = np.longdouble


def trials_of(c):
    return c['idx'][:2]                                   # (two trials of a case show what all of them show: the inputs are drawn alike)


@pytest.mark.parametrize('c', gk.CASES, ids=gk.CASE_IDS)
def test_mirror_meets_every_bound_and_the_gradient_bound_sees_the_variance_term(c):
    for trial in trials_of(c):
        ref = gk.reference(c, trial)
        out = gk.mirror(c, trial)
        r = gk.ratios_of(ref, out)
        e_sig = gk.rel(out['Sig'], ref['Sig'])
        var, _ = gk.var_term(ref, ref['Sig'])
        med = float(np.median(np.abs(var)))
        sens = float(np.max(gk.bound_d(ref, ref['Sig']))) / med
        print('%s trial %d: mirror A %.3g, B %.3g, C %.3g, D %.3g, Sigma %.2e; largest D bound / median variance term (%.3g) = %.2e'
              % (c['name'], trial, r['A'], r['B'], r['C'], r['D'], e_sig, med, sens))
        assert max(r.values()) <= 1.0, r
        assert e_sig <= gk.TOL_SIGMA
        assert sens <= 1e-3


@pytest.mark.parametrize('c', gk.CASES, ids=gk.CASE_IDS)
def test_every_fault_misses_a_bound_by_a_factor_of_1000(c):
    trial = c['idx'][0]
    ref = gk.reference(c, trial)
    line = []
    for fault in gk.FAULTS:
        if not gk.fault_defined(c, fault):
            line.append('%s -' % fault)
            continue
        r = gk.ratios_of(ref, gk.mirror(c, trial, fault=fault))
        line.append('%s %.1e (%s)' % (fault, max(r.values()), max(r, key=r.get)))
        assert max(r.values()) >= 1000.0, (fault, r)
    print('%s: %s' % (c['name'], ', '.join(line)))


def test_every_fault_is_exercised():
    for fault in gk.FAULTS:
        n = sum(gk.fault_defined(c, fault) for c in gk.CASES)
        print('%s: defined on %d of %d cases' % (fault, n, len(gk.CASES)))
        assert n >= (1 if fault == 'hi_ignored' else 15)


def test_the_cases_sit_on_the_seams():
    by = lambda k, **fix: {c[k] for c in gk.CASES if all(c[f] == v for f, v in fix.items())}
    assert {1, 33, 63, 64, 65, 127, 128, 129, 200} <= by('T', p=3, q=21)
    assert {3, 15, 16, 17, 50, 130} <= by('q', p=3, T=70)
    assert {1, 2, 5, 15, 16, 20, 21, 22, 30, 31, 32} <= by('p', T=40, q=37)
    assert {1, 2, 3} <= {len(c['idx']) for c in gk.CASES} and any(c['idx'] == (4, 0, 2) and c['R'] == 5 for c in gk.CASES)
    assert [gk.unpack_tile_bins(p) for p in (20, 21, 29, 30, 32)] == [32, 16, 16, 8, 8]
    assert [gk.pack_tile_bins(p) for p in (15, 16, 21, 22, 30, 31)] == [32, 16, 16, 8, 8, 4]
    assert all((p * (p + 1) // 2) % 16 == 0 for p in (31, 32)) and all((p * (p + 1) // 2) % 16 for p in (1, 2, 5, 15, 16, 20, 21, 22, 30))
    assert all(c['p'] * c['T'] <= 1500 for c in gk.CASES)
    for c in gk.CASES:
        g = gk.inputs(c)
        assert g['lam'].min() >= 1e-4 and (g['lam'].size < 500 or (g['lam'].max() > 50.0 and g['lam'].min() < 1e-3))   # (T = 1 draws 21 rates only)
        assert np.any(g['d'] > 0) and np.any(g['d'] < 0) and np.any(np.all(g['C'] == 0, axis=1)) and (c['p'] < 3 or np.any(np.all(g['C'] == 0, axis=0)))
        assert c['p'] == 1 or (g['tau'].min() == pytest.approx(0.03) and g['tau'].max() == pytest.approx(0.6))
        assert (g['Y'].max() > 255) == c['hi']
        lmy = g['lam'] - g['Y']
        assert np.any(lmy > 0) and np.any(lmy < 0)                                  # lambda - y cancels in the sums
    m = gk.masked_problem('both')
    assert tuple(m['lens']) == (1, 63, 64, 65, 130) and m['T'] == 130 and np.all(m['Y'][~m['live']] == 0) and m['rows'][4].all()


# ---- FP64 numpy against longdouble -----------------------------------------------------------------------------------------------------------------------
def ld_cholesky(A):
    """lower Cholesky factor in longdouble, one column at a time"""
    L = np.array(A, dtype=LD)
    for j in range(L.shape[0]):
        if j:
            L[j:, j] -= L[j:, :j] @ L[j, :j]
        L[j, j] = np.sqrt(L[j, j])
        L[j + 1:, j] /= L[j, j]
    return np.tril(L)


def ld_lower_inverse(L):
    n = L.shape[0]
    X = np.zeros_like(L)
    for i in range(n):
        row = -(L[i, :i] @ X[:i]) if i else np.zeros(n, dtype=LD)
        row[i] += 1
        X[i] = row / L[i, i]
    return X


SMALL = [c for c in gk.CASES if c['p'] * c['T'] <= 400]


@pytest.mark.parametrize('c', SMALL, ids=[c['name'] for c in SMALL])
def test_numpy_logdet_and_sigma_against_longdouble(c):
    trial = c['idx'][0]
    ref = gk.reference(c, trial)
    p, T, n = c['p'], c['T'], c['p'] * c['T']
    P = np.zeros((n, n), dtype=LD)
    for k in range(p):
        Li = ld_lower_inverse(ld_cholesky(ref['K'][k]))
        P[k * T:(k + 1) * T, k * T:(k + 1) * T] = Li.T @ Li
    t = np.arange(T)
    for k in range(p):
        for l in range(p):
            P[k * T + t, l * T + t] += ref['W'][:, k, l]
    P[np.arange(n), np.arange(n)] *= 1 + LD(gk.JIT)
    L = ld_cholesky(P)
    logdet = 2 * np.sum(np.log(np.diag(L)))
    Li = ld_lower_inverse(L)
    Sig = gk.blocks_of(Li.T @ Li, p, T)
    e_ld = float(abs(ref['logdet'] - logdet))
    e_sig = float(np.max(np.abs(ref['Sig'] - Sig)) / np.max(np.abs(Sig)))
    rho = e_ld / (gk.U * abs(float(logdet)))
    print('%s: n = %d, logdet %.3f, FP64 numpy off by %.2e = %.3g u |logdet| (model %g), Sigma blocks off by %.2e of the largest entry'
          % (c['name'], n, float(logdet), e_ld, rho, gk.NP_LOGDET_RHO, e_sig))
    assert rho <= gk.NP_LOGDET_RHO
    assert e_sig <= 1e-3 * gk.TOL_SIGMA                 # the yardstick of the 1e-8 tie is itself right to 1e-11
