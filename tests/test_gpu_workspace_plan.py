"""Slots per chunk of the workspace plan (csrc/workspace.hip: ensure_workspace; the rule: csrc/plan.h: slot_count) as a context reports them, at
shapes that come nowhere near the memory budget: option chunk_trials alone binds.  A Laplace E-step over all trials of a small context; info
'chunk_trials' is the plan's slot count - 48 of 100 trials round to three balanced chunks of 40, 20 to groups of 8 (16), 12 stays (below 16 nothing
is rounded), 0 takes the whole list; 64 of 130 trials make three chunks of 48.  A second identical E-step keeps the plan (info 'plans' stays 1).
The memory-bound paths are those of test_gpu_round3.py (test_workspace_grows_with_the_ranks), test_gpu_round5.py and test_gpu_round6.py."""
import numpy as np
import pytest

from funs import _hip
from test_cpu_posterior_samples import BIN_MS, problem

pytestmark = pytest.mark.gpu

Q, P, T = 8, 2, 20
CASES = [(100, 48, 40), (100, 20, 16), (100, 12, 12), (100, 0, 100), (130, 64, 48)]      # trials, option chunk_trials, slots per chunk

_problems = {}


def _problem(R):
    if R not in _problems:
        _problems[R] = problem((Q, P, T), R=R)[:2]
    return _problems[R]


@pytest.mark.parametrize('R,option,slots', CASES, ids=['R%d-opt%d' % c[:2] for c in CASES])
def test_chunk_trials_option_sets_the_slot_count(R, option, slots):
    par, Y = _problem(R)
    ctx = _hip.Context(Q, P, T, R, BIN_MS)
    try:
        ctx.upload_counts(Y)
        ctx.set_params(par['C'], par['d'], par['tau'])
        ctx.set_option('chunk_trials', option)
        _, _, status = ctx.estep_laplace()
        chunk, plans = ctx.info('chunk_trials'), ctx.info('plans')
        _, _, status2 = ctx.estep_laplace()
        print('R %d, chunk_trials %d: %d slots per chunk, %d plan(s), %d after a second E-step' % (R, option, chunk, plans, ctx.info('plans')))
        assert np.all(status == 0) and np.all(status2 == 0)
        assert chunk == float(slots) and ctx.info('chunk_trials') == float(slots)
        assert plans == 1.0 and ctx.info('plans') == 1.0
    finally:
        ctx.close()
