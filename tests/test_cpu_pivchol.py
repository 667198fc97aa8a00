"""The checks of tests/test_gpu_pivchol.py have teeth on the very cases the GPU test uses: without a GPU, a float64 numpy implementation of the kernels'
algorithm passes them, and the same implementation with any one fault misses one of them by more than a factor of 1000 in every case in which the fault
is defined.  (The mutants are judged in float64 - their errors are 1000 bounds or more, the evaluation's own rounding is about one; the right
implementation is judged in longdouble as the device is.)

The faults:
* drop_first / drop_mid / drop_last   in column 1, r / 2, r - 1 the dot product of ONE bin loses its term with the largest |F[t, m] F[piv, m]| (t not the
                    pivot).  That magnitude is the error it leaves in R[piv, t].  Defined where it exceeds 1000 b and bin t is not chosen as a pivot
                    later on (a later pivot at t makes row t of R exact again: the factor is then another correct one)
* double_tail       the last, partly filled block of 8 columns is summed twice, in every step
* keep_dpiv         d[piv] is not cleared: it keeps the value it was chosen for, and the same bin is chosen again
* stop_early / stop_late   the loop stops one column early / runs one column past the stop.  Defined where the diagonal entry that decides is more than
                    1000 b away from tol (early: what is left behind above tol; late: what was taken below it), late also only below full rank
* rows_kept         rows [T, Tf) are not cleared.  Defined where Tf > T"""
import numpy as np
import pytest

import test_gpu_pivchol as gk

FAULTS = ('drop_first', 'drop_mid', 'drop_last', 'double_tail', 'keep_dpiv', 'stop_early', 'stop_late', 'rows_kept')
CASES = [(c, k) for c in gk.LAUNCHES for k in range(len(c['taus']))]
IDS = ['%s_k%d' % (c['name'], k) for c, k in CASES]


def pivchol_f64(T, Tf, tau, tol, fault=None, rank=None, drop_at=None):
    """the algorithm of rbf_pivchol_kernel in float64: (slab (Tf, Tf) [column, bin], rank, pivots, info).  rank: stop after that many columns whatever
    the diagonal says (the stop faults); drop_at: the column in which one term is lost"""
    slab = np.full((Tf, Tf), gk.POISON)
    slab[:, :T] = 0.0
    if fault != 'rows_kept':
        slab[:, T:] = 0.0
    d = np.full(T, 1.0 - gk.EPS)
    t = np.arange(T, dtype=np.float64) * gk.BIN_MS
    den = (tau * 1000.0) * (tau * 1000.0)
    pivots, info = [], dict(magnitude=0.0, row=-1, decided=None)
    j = 0
    while j < min(T, Tf):
        piv = int(np.argmax(d))                         # largest remaining diagonal entry, lowest index on ties
        dp = d[piv]
        if rank is None and not dp > tol:
            break
        if rank is not None and (j >= rank or not dp > 0.0):
            break
        frow = slab[:j, piv].copy()
        tot = slab[:j, :T].T @ frow
        if drop_at is not None and j == drop_at and j > 0:
            terms = np.abs(slab[:j, :T] * frow[:, None])            # (j, T)
            terms[:, piv] = 0.0
            m, row = np.unravel_index(int(np.argmax(terms)), terms.shape)
            tot[row] -= slab[m, row] * frow[m]
            info['magnitude'], info['row'] = float(terms[m, row]), int(row)
        if fault == 'double_tail' and j % 8:
            m0 = j // 8 * 8
            tot = tot + slab[m0:j, :T].T @ frow[m0:]
        dt = t - t[piv]
        v = ((1.0 - gk.EPS) * np.exp(-0.5 * ((dt * dt) / den)) - tot) * (1.0 / np.sqrt(dp))
        slab[j, :T] = v
        keep = d[piv]
        d = d - v * v
        d[piv] = keep if fault == 'keep_dpiv' else 0.0
        pivots.append(piv)
        j += 1
    info['next'] = float(np.max(d)) if T else 0.0       # the diagonal entry that would be taken next
    return slab, j, pivots, info


_right = {}


def right(c, k):
    key = (c['name'], k)
    if key not in _right:
        _right[key] = pivchol_f64(c['T'], c['Tf'], c['taus'][k], c['tol'])
    return _right[key]


def mutant(c, k, fault):
    """(defined, worst check of the mutant as a fraction of what it allows) - defined: the fault is one the checks can be asked to see in this case
    (module docstring); b is the mutant's own, as in the checks"""
    T, Tf, tau, tol = c['T'], c['Tf'], c['taus'][k], c['tol']
    _, r0, _, info0 = right(c, k)

    def judge(slab, r):
        res = gk.check_factor(slab, r, T, tau, tol, dtype=np.float64)
        return res['b'], gk.worst(res)

    if fault.startswith('drop_'):
        at = {'drop_first': 1, 'drop_mid': r0 // 2, 'drop_last': r0 - 1}[fault]
        if at < 1:
            return False, 0.0
        slab, r, piv, info = pivchol_f64(T, Tf, tau, tol, drop_at=at)
        b, w = judge(slab, r)
        return info['magnitude'] > 1000 * b and info['row'] not in piv[at + 1:], w
    if fault == 'stop_early':
        if r0 < 2:
            return False, 0.0
        slab, r, piv, info = pivchol_f64(T, Tf, tau, tol, rank=r0 - 1)
        b, w = judge(slab, r)
        return info['next'] - tol > 1000 * b, w
    if fault == 'stop_late':
        if r0 >= T:
            return False, 0.0
        slab, r, piv, info = pivchol_f64(T, Tf, tau, tol, rank=r0 + 1)
        b, w = judge(slab, r)
        return r == r0 + 1 and tol - info0['next'] > 1000 * b, w
    if (fault == 'rows_kept' and Tf == T) or (fault in ('double_tail', 'keep_dpiv') and r0 < 2):
        return False, 0.0
    slab, r, piv, info = pivchol_f64(T, Tf, tau, tol, fault=fault)
    return True, judge(slab, r)[1]


_judged = {}


def judged(c, k, fault):
    """mutant(c, k, fault), computed once"""
    key = (c['name'], k, fault)
    if key not in _judged:
        _judged[key] = mutant(c, k, fault)
    return _judged[key]


@pytest.mark.parametrize('c,k', CASES, ids=IDS)
def test_checks_separate_the_mutants(c, k):
    T, tau, tol = c['T'], c['taus'][k], c['tol']
    slab, r, _, _ = right(c, k)
    res = gk.check_factor(slab, r, T, tau, tol)
    line = ['%s latent %d: rank %d, b %.3g, right: %.3g' % (c['name'], k, r, res['b'], gk.worst(res))]
    assert gk.worst(res) <= 1.0, res
    for fault in FAULTS:
        ok, ratio = judged(c, k, fault)
        if not ok:
            line.append('%s -' % fault)
            continue
        line.append('%s %.2e' % (fault, ratio))
        assert ratio > 1000.0, (fault, ratio)
    print(', '.join(line))


def test_every_fault_is_exercised():
    for fault in FAULTS:
        n = sum(judged(c, k, fault)[0] for c, k in CASES)
        print('%s: defined on %d of %d cases' % (fault, n, len(CASES)))
        assert n >= 10
