"""The bound of tests/test_gpu_bin_blocks.py - 4 times the error of a float64 mirror of the kernel, per case and quantity - has teeth on the very inputs
the GPU test uses: without a GPU, the longdouble reference with any one of five faults must miss it by more than a factor of 1000 in every case in which
the fault is defined.

The faults (`fault` of test_gpu_bin_blocks.blocks / expected):
* eps_missing     eps left out of one entry: A[0][0] = 1 + W[0][0]
* uninverted_col  G from the un-inverted factor in one column (column 0 of L^-1 is column 0 of L).  Defined for two latents or more (with one, at
                  eps ||W|| = 0.01, L and its inverse are both 1 to within the fault's reach - and p = 1 has no such case)
* nonsym_g        Wt = G W^T with a G that is not symmetric (one off-diagonal entry doubled).  Defined for two latents or more
* log_pivot       the log of the pivot instead of its square.  Defined where ldet is requested
* tail_unstored   the last item of a partly filled workgroup not stored.  Defined where the item count is no multiple of the workgroup's"""
import numpy as np
import pytest

import test_gpu_bin_blocks as gk


def defined(c, fault):
    g = gk.blocks_input(c)
    if fault in ('uninverted_col', 'nonsym_g'):
        return g['p'] >= 2
    if fault == 'log_pivot':
        return c['want_ldet']
    if fault == 'tail_unstored':
        return g['items'] % g['pb'] != 0
    return True


@pytest.mark.parametrize('c', gk.CASES, ids=gk.CASE_IDS)
def test_bound_separates_the_mutants(c):
    g = gk.blocks_input(c)
    p, T = g['p'], g['T']
    # the generator's contract: symmetric, positive semi-definite, eps ||W|| as the case says; poison in unlisted slots and behind the strides
    for i, s in enumerate(c['slots']):
        M = g['W'][s, :g['run']].reshape(T, p, p)
        assert np.array_equal(M, g['Wl'][i]) and np.array_equal(M, np.transpose(M, (0, 2, 1)))
        ev = np.linalg.eigvalsh(M)
        assert np.all(ev[:, 0] > -1e-9 * ev[:, -1]) and np.allclose(gk.EPS * ev[:, -1], c['scale'], rtol=1e-9)
    unlisted = [s for s in range(c['nslots']) if s not in c['slots']]
    assert np.all(g['W'][unlisted] == gk.POISON) and np.all(g['W'][:, g['run']:] == gk.POISON)
    assert np.all(g['G0'] == gk.POISON) and np.all(g['Wt0'] == gk.POISON)

    ref = gk.expected(c)
    mir = gk.mirror_buffers(c)
    em = gk.errors(mir, ref)
    assert all(e > 0.0 for e in em[:2]) and max(gk.ratios(em, em)) == 0.25
    # the mirror is the kernel's algorithm: it is right to a few units of rounding of the largest entry times the condition of I + eps W
    cond = 1.0 + c['scale']
    assert em[0] < 1e-13 * cond and em[1] < 1e-13 * cond * c['scale'] / gk.EPS and em[2] < 1e-13 * p
    line = ['%s: mirror error G %.3g, Wt %.3g, ldet %.3g' % (c['name'], em[0], em[1], em[2])]
    for fault in gk.FAULTS:
        if not defined(c, fault):
            line.append('%s -' % fault)
            continue
        mut = gk.expected(c, fault=fault)
        if not c['want_ldet']:
            mut, refq = mut[:2], ref[:2]
        else:
            refq = ref
        with np.errstate(invalid='ignore'):
            err = gk.errors(mut, refq)
        err = [np.inf if np.isnan(e) else e for e in err]
        ratio = max(gk.ratios(err, em))
        line.append('%s %.2e' % (fault, ratio))
        assert ratio > 1000.0, (fault, ratio)
    print(', '.join(line))


def test_every_fault_is_exercised():
    for fault in gk.FAULTS:
        n = sum(defined(c, fault) for c in gk.CASES)
        print('%s: defined on %d of %d cases' % (fault, n, len(gk.CASES)))
        assert n >= 10


def test_the_cases_the_kernels_need_are_there():
    ps = {c['p'] for c in gk.CASES}
    assert {1, 2, 3, 5, 6, 7, 9, 10, 11, 16, 17, 20, 24, 25, 32} <= ps
    reg = {len(c['slots']) * c['T'] for c in gk.CASES if c['p'] <= 10}
    assert {1, 31, 32, 33, 70} <= reg
    for p in (11, 16, 17, 20, 24, 25, 32):              # an odd count and a partly filled last workgroup, under the workgroup size the launcher picks
        mine = [len(c['slots']) * c['T'] for c in gk.CASES if c['p'] == p]
        assert any(n % 2 == 1 for n in mine) and any(n % gk.per_block(p) for n in mine)
    assert [gk.per_block(p) for p in (11, 16, 17, 20, 24, 25, 32)] == [8, 8, 8, 6, 4, 4, 2]
    for form in (lambda p: p <= 10, lambda p: p > 10):
        mine = [c for c in gk.CASES if form(c['p'])]
        assert {c['scale'] for c in mine} == set(gk.SCALES)
        assert any(c['shared'] for c in mine) and any(not c['want_ldet'] for c in mine) and any(len(c['slots']) < c['nslots'] for c in mine)
