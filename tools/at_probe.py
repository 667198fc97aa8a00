"""The latent posterior at arbitrary time points at the bench's dimensions, 200 neurons x 10 latents x 500 bins (argv: trials S; default 64 500):
one Laplace E-step over `trials` trials with the per-trial blocks kept (keep_trial_vsmgp 1, so that the call times the entry point and not the
rebuild of the blocks), then pgpfa_posterior_at for a shared grid of S times, wall time per call, next to the 2 R p T^2 S flops of the variance
contraction and the R p T^2 doubles of V it reads; then once with the mean alone and once with one grid per trial (docs/history/posterior_at.md)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'poisson-gpfa_amd')]
from funs import _hip   # noqa: E402

R = int(sys.argv[1]) if len(sys.argv) > 1 else 64
S = int(sys.argv[2]) if len(sys.argv) > 2 else 500
q, p, T, BIN = 200, 10, 500, 10.0
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

ctx = _hip.Context(q, p, T, R, BIN)
ctx.upload_counts(Y)
ctx.set_option('keep_trial_vsmgp', 1)
ctx.set_params(C, d, tau)
t0 = time.time()
_, _, status = ctx.estep_laplace()
print('R=%d: estep_laplace %.2f s, status %s, plan_lowrank %d' % (R, time.time() - t0, np.unique(status), ctx.info('plan_lowrank')), flush=True)
times = np.sort(rng.uniform(-2 * BIN, (T + 1) * BIN, S))
flops, nbytes = 2.0 * R * p * T * T * S, 8.0 * R * p * T * T
for rep in range(4):
    t0 = time.time()
    out = ctx.posterior_at(times)
    dt = time.time() - t0
    print('R=%d S=%d pass %d: posterior_at(mean, var) %.1f ms wall: %.3g flops -> %.2f TFLOP/s, %.3g bytes of V -> %.0f GB/s'
          % (R, S, rep, 1e3 * dt, flops, flops / dt / 1e12, nbytes, nbytes / dt / 1e9), flush=True)
t0 = time.time()
ctx.posterior_at(times, want=('mean',))
print('R=%d S=%d: mean alone %.1f ms wall' % (R, S, 1e3 * (time.time() - t0)), flush=True)
t0 = time.time()
ctx.posterior_at(times[None, :] + rng.uniform(-50.0, 50.0, R)[:, None])
print('R=%d S=%d: one grid per trial %.1f ms wall' % (R, S, 1e3 * (time.time() - t0)), flush=True)
ctx.close()
