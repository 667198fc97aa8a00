"""The bound of tests/test_gpu_assemble_b.py - 1.01 (T + 2) u sum |f||w||f| per entry - has teeth on the very inputs the GPU test uses: without a GPU, the
longdouble reference with any one of five faults must miss the bound by more than a factor of 1000 in every case in which the fault is defined.

The faults (`fault` of test_gpu_assemble_b.reference):
* drop_run         one 4-bin run of the row side of latent 0 never summed
* neighbour_pair   the weight block of the last latent's diagonal pair taken from the neighbouring pair (p - 1, p - 2).  Defined for two latents or more
* cmap_shift       cmap off by one 4-row run for the last latent: its rows and columns stored 4 further on.  Defined under compact offsets (gran 4, 8)
* second_slot      the second slot of a workgroup reads the first slot's weights.  Defined where two slots or more are listed
* identity_padded  the identity added where the padded index of a real row says, not at its compact place.  Defined under compact offsets where a
                   latent that is not the last has rk > rr (else the two spaces are one)
The sixth fault of the float form - weights not rounded to float32 - cannot be separated by this bound, and no bound of this kind can: it moves a term by
at most 2^-24 of its magnitude, the bound allows (T + 2) 2^-24 of it.  test_unrounded_weights_stay_inside_the_bound records that."""
import numpy as np
import pytest

import test_gpu_assemble_b as gk


def defined(c, fault):
    g = gk.assemble_input(c)
    if fault == 'neighbour_pair':
        return g['p'] >= 2
    if fault == 'cmap_shift':
        return g['compact']
    if fault == 'second_slot':
        return len(c['slots']) >= 2
    if fault == 'identity_padded':
        if not (g['compact'] and any(g['rk'][l] > g['rr'][l] for l in range(g['p'] - 1))):
            return False
        # the fault moves a 1: it can be 1000 bounds only where the bound of a diagonal entry is below 1e-3 - in float, 1.01 (T + 2) 2^-24 sum f^2 |w|
        # passes that near T = 115 (every FP64 case and every float case up to T = 100 is in; the float twin at T = 140 is not)
        return not c['f32'] or diagonal_bound(c) < 1e-3
    return True


def diagonal_bound(c):
    ref, bound, written = gk.reference(c)
    return max(float(np.max(np.diagonal(bound[s]))) for s in c['slots'])


@pytest.mark.parametrize('c', gk.CASES, ids=gk.CASE_IDS)
def test_bound_separates_the_mutants(c):
    g = gk.assemble_input(c)
    # the generator's contract: magnitudes in [0.5, 1.5] wherever a value is real, zeros in the slab columns [rank, rk), poison elsewhere, Wt symmetric
    T, p = g['T'], g['p']
    for l in range(p):
        real = g['F'][l, :g['ranks'][l], :T]
        assert np.all((np.abs(real) >= 0.5) & (np.abs(real) <= 1.5))
        assert np.all(g['F'][l, g['ranks'][l]:g['rk'][l], :T] == 0.0)
        assert np.all(g['F'][l, :, T:] == gk.POISON) and np.all(g['F'][l, g['rk'][l]:, :] == gk.POISON)
    assert np.all(g['B0'] == gk.POISON)
    if not c['shared']:
        unlisted = [s for s in range(c['nslots']) if s not in c['slots']]
        assert np.all(g['Wt'][unlisted] == gk.POISON) and np.all(g['Wt'][:, g['wbin']:] == gk.POISON)
    for s in c['slots']:
        W = (g['Wt'].reshape(-1)[:g['wbin']] if c['shared'] else g['Wt'][s, :g['wbin']]).reshape(T, p, p)
        assert np.array_equal(W, np.transpose(W, (0, 2, 1))) and np.all((np.abs(W) >= 0.5) & (np.abs(W) <= 1.5))

    ref, bound, written = gk.reference(c)
    assert np.all(ref[written] != gk.POISON) and np.all(ref[~written] == gk.POISON)
    # one lost term (0.125 at least) is 1000 bounds or more; in float 50: its worst case 1.01 (T + 2) 2^-24 T 1.5^3 + 2^-24 (1 + 3.375 T) is 2.1e-3 at T = 100
    limit = gk.SMALLEST_TERM / 50 if c['f32'] else 1e-3 * gk.SMALLEST_TERM
    assert float(np.max(bound[written])) < limit, float(np.max(bound[written]))
    assert gk.worst_ratio(ref, ref, bound, written) == 0.0
    line = ['%s: largest bound %.3e' % (c['name'], float(np.max(bound)))]
    for fault in gk.FAULTS:
        if not defined(c, fault):
            line.append('%s -' % fault)
            continue
        mut, _, wm = gk.reference(c, fault=fault)
        assert np.array_equal(wm, written)
        ratio = gk.worst_ratio(mut, ref, bound, written)
        line.append('%s %.2e' % (fault, ratio))
        assert ratio > 1000.0, (fault, ratio)
    print(', '.join(line))


@pytest.mark.parametrize('c', [c for c in gk.CASES if c['f32']], ids=[c['name'] for c in gk.CASES if c['f32']])
def test_unrounded_weights_stay_inside_the_bound(c):
    """weights not rounded to float32: at most 1 / (T + 2) of the bound, by arithmetic - the bound cannot see this fault"""
    ref, bound, written = gk.reference(c)
    mut, _, _ = gk.reference(c, unrounded_weights=True)
    ratio = gk.worst_ratio(mut, ref, bound, written)
    print('%s: weights not rounded, worst / bound %.3g' % (c['name'], ratio))
    assert 0.0 < ratio <= 1.0 / (c['T'] + 2)


def test_every_fault_is_exercised():
    for fault in gk.FAULTS:
        n = sum(defined(c, fault) for c in gk.CASES)
        print('%s: defined on %d of %d cases' % (fault, n, len(gk.CASES)))
        assert n >= 10


def test_the_cases_the_kernel_needs_are_there():
    """every bin count of the list, every rank list under every granularity, float twins, a slot list, the shared slot, 10 and 20 latents"""
    names = set(gk.CASE_IDS)
    for T in gk.BIN_T:
        for f32 in (False, True):
            assert gk.case(T, (20, 4, 68), nslots=2, f32=f32)['name'] in names
    for i, r in enumerate(gk.RANKS + ((8, 70),)):
        T = 70 if r == (8, 70) else gk.rank_T(i, r)
        for gran in (4, 8, 16):
            assert gk.case(T, r, gran, nslots=2)['name'] in names
        assert gk.case(T, r, 4, nslots=2, f32=True)['name'] in names
    assert sorted({len(c['slots']) for c in gk.CASES}) == [1, 2, 3]
    assert any(c['shared'] for c in gk.CASES) and any(c['nslots'] == 7 for c in gk.CASES)
    assert {10, 20} <= {len(c['ranks']) for c in gk.CASES}
