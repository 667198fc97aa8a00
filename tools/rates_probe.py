"""Posterior rates at the bench's dimensions, 200 neurons x 10 latents x 500 bins, on a synthetic posterior uploaded with set_posterior (argv: trials
[wall]).  Without `wall`: two passes of pgpfa_posterior_rates with all outputs (8 groups), with the group outputs only and with eta + var only - run it
under `rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o r -- python3 tools/rates_probe.py 1024` and read the rates_* rows of the kernel
trace in start order (tools/gemm_by_grid.py groups them by grid).  With `wall`: the wall time of util.posteriorRates(want=(), conditions=...) against the
numpy route it replaces - post_mean / post_vsm to the host, einsum per (trial, neuron, bin), mean per condition - and their difference."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'poisson-gpfa_amd')]
from funs import _hip, _session, util   # noqa: E402

R = int(sys.argv[1])
wall = len(sys.argv) > 2
q, p, T, G = 200, 10, 500, 8
rng = np.random.default_rng(1)
R0 = min(R, 64)
C = rng.standard_normal((q, p)) / np.sqrt(p)
d = -np.ones(q)
mean0 = 0.5 * rng.standard_normal((R0, p, T))
A = rng.standard_normal((R0, T, p, p))
vsm0 = 0.05 * A @ A.transpose(0, 1, 3, 2) + 0.01 * np.eye(p)
rep = (R + R0 - 1) // R0
mean, vsm = np.tile(mean0, (rep, 1, 1))[:R], np.tile(vsm0, (rep, 1, 1, 1))[:R]
eta0 = d[None, :, None] + np.einsum('nk,rkt->rnt', C, mean0)
Y0 = rng.poisson(np.exp(eta0)).astype(np.uint8)
Y = np.tile(Y0, (rep, 1, 1))[:R]
group = (np.arange(R) % G).astype(np.int32)

if not wall:
    ctx = _hip.Context(q, p, T, R, 10.0)
    ctx.upload_counts(Y)
    ctx.set_params(C, d, np.linspace(0.1, 0.3, p))
    ctx.set_posterior(None, mean, vsm)
    for rep_ in range(2):
        t0 = time.time()
        ctx.posterior_rates(None, group=group, n_groups=G, want=('eta', 'var', 'ell', 'group_sum', 'group_count'))
        t1 = time.time()
        ctx.posterior_rates(None, group=group, n_groups=G, want=('group_sum', 'group_count'))
        t2 = time.time()
        ctx.posterior_rates(None, want=('eta', 'var'))
        t3 = time.time()
        print('R=%d pass %d: all outputs %.1f ms wall, group outputs only %.2f ms wall, eta+var without table %.1f ms wall' % (R, rep_, 1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t3 - t2)), flush=True)
    ctx.close()
else:
    class Exp:
        pass
    exp = Exp()
    exp.data = [{'Y': Y[r]} for r in range(R)]
    exp.binSize, exp.trialDur, exp.numTrials, exp.ydim, exp.T = 10.0, 5000.0, R, q, T
    params = {'C': C, 'd': d, 'tau': np.linspace(0.1, 0.3, p)}
    sess, idx = _session.session_for(exp, p)
    sess.set_params(params)
    sess.ctx.set_posterior(None, mean, vsm)
    sess.mark_written(idx)
    res = _session.DeviceInfRes(sess, idx, (0, R))
    for rep_ in range(3):
        t0 = time.time()
        out = util.posteriorRates(params, exp, infRes=res, conditions=group, want=())
        t1 = time.time()
        # the route it replaces: post_vsm and post_mean to the host, einsum per (trial, neuron, bin), mean per condition
        cm = np.zeros((G, q, T))
        for c0 in range(0, R, 64):
            sl = np.arange(c0, min(R, c0 + 64), dtype=np.int32)
            m_, v_ = sess.ctx.post_mean(sl), sess.ctx.post_vsm(sl)
            e_ = d[None, :, None] + np.einsum('nk,rkt->rnt', C, m_)
            s_ = np.einsum('ni,rtij,nj->rnt', C, v_, C, optimize=True)
            rate = np.exp(e_ + 0.5 * s_)
            for g in range(G):
                cm[g] += rate[group[sl] == g].sum(axis=0)
        cm = cm / np.bincount(group, minlength=G)[:, None, None] * 100.0
        t2 = time.time()
        err = np.max(np.abs(cm - out['condition_mean'])) / np.max(np.abs(cm))
        print('R=%d pass %d: util.posteriorRates(want=(), conditions) %.1f ms (of it set_params: see below), numpy route %.0f ms, difference %.1e' % (R, rep_, 1e3 * (t1 - t0), 1e3 * (t2 - t1), err), flush=True)
    t0 = time.time(); sess.set_params(params); t1 = time.time()
    print('R=%d: sess.set_params alone %.1f ms' % (R, 1e3 * (t1 - t0)))
    _session.drop_sessions()
