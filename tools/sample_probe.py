"""Joint posterior samples at the bench's dimensions, 200 neurons x 10 latents x 500 bins, 64 draws per trial (argv: mode trials).

kernels  one Laplace E-step over `trials` trials, then two passes of pgpfa_posterior_sample (x and count_sum).  Run it under
         `rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o s -- python3 tools/sample_probe.py kernels 64` and read the phases off the
         kernel rows: bin_blocks / assemble_b / potrf / trsm rows = factor, the GEMM rows with M = rpad = U, with M = 500 = F U, psample_mix_kernel,
         psample_counts_kernel, psample_noise_kernel.
wall     util.posteriorSamples(nSamples=64) over `trials` trials of an experiment (x; then count_sum alone), wall time per call.
old      the route without the entry point: pgpfa_get_post_cov per trial, numpy.linalg.cholesky on the host, 64 draws - for as many trials as a
         minute allows.  Uses nothing this entry point added, so the same file times the route on an older checkout."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'poisson-gpfa_amd')]
from funs import _hip   # noqa: E402

mode, R = sys.argv[1], int(sys.argv[2])
q, p, T, S, BIN = 200, 10, 500, 64, 10.0
rng = np.random.default_rng(1)
C = rng.standard_normal((q, p)) / np.sqrt(p)
d = -np.ones(q)
tau = np.linspace(0.1, 0.3, p)
t = np.arange(T) * BIN
R0 = min(R, 16)
X0 = np.empty((R0, p, T))
for k in range(p):
    K = np.exp(-0.5 * (t[:, None] - t[None, :]) ** 2 / (1000.0 * tau[k]) ** 2) + 1e-3 * np.eye(T)
    X0[:, k] = (np.linalg.cholesky(K) @ rng.standard_normal((T, R0))).T
Y0 = rng.poisson(np.exp(np.einsum('nk,rkt->rnt', C, X0) + d[None, :, None])).astype(np.uint8)
Y = np.tile(Y0, ((R + R0 - 1) // R0, 1, 1))[:R]

if mode == 'wall':
    from funs import _session, inference, util

    class Exp:
        pass
    exp = Exp()
    exp.data = [{'Y': Y[r].astype(np.float64)} for r in range(R)]
    exp.binSize, exp.trialDur, exp.numTrials, exp.ydim, exp.T = BIN, T * BIN, R, q, T
    params = {'C': C, 'd': d, 'tau': tau}
    t0 = time.time()
    infRes, _ = inference.laplace(exp, {k: v.copy() for k, v in params.items()}, returnOptimRes=False)
    print('R=%d: inference.laplace %.2f s' % (R, time.time() - t0), flush=True)
    for rep in range(3):
        t0 = time.time()
        out = util.posteriorSamples(params, exp, infRes=infRes, nSamples=S, seed=rep, want=('x',))
        t1 = time.time()
        cs = util.posteriorSamples(params, exp, infRes=infRes, nSamples=S, seed=rep, want=('count_sum',))
        t2 = time.time()
        print('R=%d pass %d: util.posteriorSamples(nSamples=%d) x %.3f s (%.2f ms per trial, %.0f MB to the host), count_sum alone %.3f s'
              % (R, rep, S, t1 - t0, 1e3 * (t1 - t0) / R, out['x'].nbytes / 1e6, t2 - t1), flush=True)
    _session.drop_sessions()
    sys.exit(0)

ctx = _hip.Context(q, p, T, R, BIN)
ctx.upload_counts(Y)
ctx.set_params(C, d, tau)
t0 = time.time()
_, _, status = ctx.estep_laplace()
print('R=%d: estep_laplace %.2f s, status %s, plan_lowrank %d, rank %d' % (R, time.time() - t0, np.unique(status), ctx.info('plan_lowrank'), ctx.info('lowrank_rtot')), flush=True)
if mode == 'kernels':
    for rep in range(2):
        t0 = time.time()
        out = ctx.posterior_sample(None, n_samples=S, seed=rep, want=('x', 'count_sum'))
        print('R=%d pass %d: posterior_sample(x, count_sum) %.3f s wall' % (R, rep, time.time() - t0), flush=True)
else:
    m = ctx.post_mean()
    t_start, done = time.time(), 0
    while done < R and time.time() - t_start < 60.0:
        t0 = time.time()
        Sigma = ctx.post_cov(done)
        t1 = time.time()
        L = np.linalg.cholesky(0.5 * (Sigma + Sigma.T))
        t2 = time.time()
        x = m[done].reshape(-1, 1) + L @ rng.standard_normal((p * T, S))
        t3 = time.time()
        done += 1
        print('trial %d: post_cov %.2f s, host Cholesky %.2f s, %d draws %.3f s' % (done - 1, t1 - t0, t2 - t1, S, t3 - t2), flush=True)
    print('R=%d: %d trials in %.1f s: %.2f s per trial by post_cov + numpy.linalg.cholesky' % (R, done, time.time() - t_start, (time.time() - t_start) / max(done, 1)), flush=True)
ctx.close()
