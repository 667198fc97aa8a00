"""The bound of tests/test_gpu_thin_kernels.py - 1.01 K 2^-53 sum |f| |x| per entry, composed over the stages of apply - has teeth on the very inputs the
GPU test uses: without a GPU, the longdouble reference with any one of four faults must miss the bound by more than a factor of 1000, and every bound is
below 1e-3 of the smallest product term (0.25), so a single lost or doubled term is always seen.

The faults (`fault` of test_gpu_thin_kernels.reference):
* drop_run     one 4-bin run of one latent never summed (F v: one run of four rank columns; Sb u: four rows of Sb)
* shift_group  one row group reads its factor rows 4 further on (F v: the vector rows of one latent read 4 further on)
* rk_rows      the difference between rr and rk ignored: F^T t stores rk rows per latent - zeros over the first rows of the next latent, whose real
               values the rows [rr, rk) are - and F v takes its vector rows from offsets that count rk rows per latent.  Defined where a latent that
               is not the last has rk > rr (compact offsets)
* swap_cols    the first two list columns stored into each other's slot.  Defined where at least two columns are stored"""
import numpy as np
import pytest

import test_gpu_thin_kernels as gk

FAULTS = ('drop_run', 'shift_group', 'rk_rows', 'swap_cols')


def defined(c, fault):
    g = gk.thin_input(c)
    live = len(g['listed']) if c['live'] is None else c['live']
    if c['stop'] == 1 or live == 0:
        return False                                   # nothing is stored: nothing to get wrong
    if fault == 'swap_cols':
        return live >= 2
    if fault == 'rk_rows':
        return c['kind'] != 's' and any(g['rk'][l] > g['rr'][l] for l in range(g['p'] - 1))
    return True


@pytest.mark.parametrize('c', gk.CASES, ids=gk.CASE_IDS)
def test_bound_separates_the_mutants(c):
    g = gk.thin_input(c)
    # the generator's contract: magnitudes in [0.5, 1.5] wherever a value is real, zeros in the slab columns [rank, rk), poison elsewhere
    for l in range(g['p']):
        real = g['F'][l, :g['ranks'][l], :g['T']]
        assert np.all((np.abs(real) >= 0.5) & (np.abs(real) <= 1.5))
        assert np.all(g['F'][l, g['ranks'][l]:g['rk'][l], :g['T']] == 0.0)
        assert np.all(g['F'][l, :, g['T']:] == gk.POISON) and np.all(g['F'][l, g['rk'][l]:, :] == gk.POISON)
    assert np.all(g['Y0'] == gk.POISON)
    unlisted = [s for s in range(c['nslots']) if s not in g['listed']]
    assert np.all(g['X'][unlisted] == gk.POISON)
    x = np.abs(g['X'][g['listed']].astype(np.float64))
    assert np.all((x == gk.POISON) | ((x >= 0.5 - 1e-7) & (x <= 1.5 + 1e-7)))
    assert np.allclose(g['Sb'][:g['rtot'], :g['rtot']], g['Sb'][:g['rtot'], :g['rtot']].T, rtol=0, atol=0)

    ref, bound, written = gk.reference(c)
    if np.any(written):
        assert np.all(ref[written] != gk.POISON)
        assert float(np.max(bound[written])) < 1e-3 * 0.25, float(np.max(bound[written]))
        assert gk.worst_ratio(ref, ref, bound, written) == 0.0
    line = ['%s: largest bound %.3e' % (c['name'], float(np.max(bound)))]
    for fault in FAULTS:
        if not defined(c, fault):
            line.append('%s -' % fault)
            continue
        mut, _, wm = gk.reference(c, fault=fault)
        assert np.array_equal(wm, written)
        ratio = gk.worst_ratio(mut, ref, bound, written)
        line.append('%s %.2e' % (fault, ratio))
        assert ratio > 1000.0, (fault, ratio)
    print(', '.join(line))


def test_every_fault_is_exercised():
    for fault in FAULTS:
        n = sum(defined(c, fault) for c in gk.CASES)
        print('%s: defined on %d of %d cases' % (fault, n, len(gk.CASES)))
        assert n >= 10
    for kind in ('ft', 'f', 'apply'):
        assert any(defined(c, 'rk_rows') for c in gk.CASES if c['kind'] == kind)
