"""The bound of tests/test_gpu_split_kernels.py for the FP16 term of the split covariance sum - 4 x the error of a numpy emulation of the documented
arithmetic - separates right from wrong on the very inputs the GPU test uses: without a GPU, the emulation with one half product lost, with hi x hi
only, and with one column of one slot lost must each exceed that bound by more than a factor of 10.

And the problems of tests/test_gpu_split_paths.py leave the device its share of that file's tolerance: the truncation of the prior's low-rank factors,
which the dense reference does not have, takes at most half of the 1e-8 allowed to the covariance part of PautoSum."""
import numpy as np
import pytest

import test_gpu_split_kernels as gk
import test_gpu_split_paths as gp


@pytest.mark.parametrize('case', gk.SYRK_CASES, ids=gk.SYRK_IDS)
def test_emulation_bound_separates_the_mutants(case):
    buf, valid = gk.syrk_input(case)
    T, ts, ract, p = case['T'], case['ts'], case['ract'], case['p']
    # the generator's contract: magnitudes, and poison in every float the sums must not see
    assert np.max(np.abs(valid)) <= 0.3 < 1.0
    seen = np.zeros(buf.shape, dtype=bool)
    for k in range(p):
        seen[:, :ract, k * ts:k * ts + T] = True
    assert np.all(buf[~seen] == gk.POISON) and not np.any(buf[seen] == gk.POISON)
    ref, e_emu, bound = gk.syrk_reference_and_bound(case)
    spe, _ = gk.groups_of(case['nslots'], case['sps'])
    errs = {m: gk.syrk_error(case, gk.emulate_syrk(valid, spe, mutant=m), ref) for m in ('drop_lh', 'hh_only', 'drop_column')}
    print('%s: emulation %.3e (bound %.3e); one half product lost %.3e, hi x hi only %.3e, one column lost %.3e'
          % (case['name'], e_emu, bound, errs['drop_lh'], errs['hh_only'], errs['drop_column']))
    assert 0.0 < e_emu <= 1e-6
    for m, e in errs.items():
        assert e > 10.0 * bound, (m, e, bound)


@pytest.mark.parametrize('name', list(gp.CASES))
def test_path_problems_leave_the_device_half_of_the_tolerance(name):
    share, ranks = gp.truncation_share(name)
    print('%s: ranks %s, truncation of the prior factors / largest covariance entry, per latent: %s' % (name, ranks, ' '.join('%.2e' % s for s in share)))
    assert np.all(share > 0.0) and np.max(share) <= 5e-9
