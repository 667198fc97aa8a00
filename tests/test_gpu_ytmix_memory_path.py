"""The memory path of yt_mix_kernel (ytmix.h) changes no bit: with every option that picks an alternative form of it set to 0 - the form of the
commit before it - an E-step gives `np.array_equal` post_vsm, PautoSum and per-trial post_vsmGP blocks.

Options under test (OPTIONS): yt_mix_dma (the panels of L^-T staged by LDS-DMA a chunk ahead of the products; 0: through registers behind them).
Each alone and all together against all at 0.  (Storing D several bins per lane was measured slower in both of its forms and is not in the code:
docs/history.)

Shapes: the bench's dimensions at 32 trials after two EM iterations (ranks no multiples of 16, a rank total above 256: blocks with more than one
panel chunk; the compact path and the fused kernel asserted); the same with rank_gran = 16 (no row map); 7 and 9 latents (the 8- and 10-wide
instantiations with empty latents) at T = 203 (no multiple of 4 or 16: a quad of bins that straddles T, a clamped last bin)."""
import itertools

import numpy as np
import pytest

from oracle import pgpfa_oracle as orc

pytestmark = pytest.mark.gpu

OPTIONS = ('yt_mix_dma',)


def _settings():
    """all at 0 first (the reference), then each option alone, then all together"""
    out = [dict.fromkeys(OPTIONS, 0)]
    for o in OPTIONS:
        out.append({k: int(k == o) for k in OPTIONS})
    if len(OPTIONS) > 1:
        out.append(dict.fromkeys(OPTIONS, 1))
    return out


def _estep(Y, par, opts, extra):
    from funs import _hip
    R, q, T = Y.shape
    p = par['C'].shape[1]
    ctx = _hip.Context(q, p, T, R, 10.0)
    try:
        ctx.upload_counts(Y)
        ctx.set_option('cov_mode', 2)
        for k, v in itertools.chain(extra.items(), opts.items()):
            ctx.set_option(k, v)
        ctx.set_params(par['C'], par['d'], par['tau'])
        _, _, st = ctx.estep_laplace()
        assert np.all(st == 0)
        ctx.mstep_precomp()
        res = [ctx.post_vsm().copy(), ctx.pautosum().copy()]
        # (the path of the pass that summed PautoSum: read before the per-trial blocks are asked for - they come from a pass of their own)
        flags = {k: ctx.info(k) for k in ('plan_lowrank', 'last_yt_mix_fused', 'lowrank_compact', 'lowrank_rtot', 'lowrank_rtot16', 'last_dense_retries')}
        res.append(ctx.post_vsmgp(np.arange(min(R, 3), dtype=np.int32)).copy())
    finally:
        ctx.close()
    return res, flags


def _compare(tag, Y, par, extra, compact):
    ref = None
    for opts in _settings():
        res, flags = _estep(Y, par, opts, extra)
        print('%s %s: %s' % (tag, opts, ', '.join('%s %g' % kv for kv in flags.items())))
        assert flags['plan_lowrank'] == 1.0 and flags['last_yt_mix_fused'] == 1.0 and flags['last_dense_retries'] == 0.0
        assert flags['lowrank_compact'] == (1.0 if compact else 0.0)
        if ref is None:
            ref = res
            assert all(np.all(np.isfinite(x)) for x in ref)
            continue
        for name, a, b in zip(('post_vsm', 'PautoSum', 'post_vsmGP'), res, ref):
            same = np.array_equal(a, b)
            print('  %s: %s (max |difference| %.3e)' % (name, 'identical' if same else 'DIFFERS', np.max(np.abs(a - b))))
            assert same, (tag, opts, name)
    return flags


@pytest.fixture(scope='module')
def bench_point():
    """the bench's dimensions at 32 trials: the parameters after two EM iterations from the Poisson-PCA start"""
    import bench
    import funs.inference
    import funs.learning
    import funs.util
    q, p, T, R = 200, 10, 500, 32
    _, Ys = bench.synth_shard(q, p, T, R, 12, 0)
    exp = bench.Shard(Ys, 10.0)
    np.random.seed(0)
    params = {k: np.real(np.asarray(v)).astype(np.float64) for k, v in funs.util.initializeParams(p, q, exp).items()}
    optim = None
    for _ in range(2):
        infRes, _, optim = funs.inference.laplace(exp, params, prevOptimRes=optim)
        params, _ = funs.learning.updateParams(params, infRes, exp, CdOptimMethod='newton')
    return np.stack(Ys).astype(np.uint8), {k: np.array(params[k], dtype=np.float64) for k in ('C', 'd', 'tau')}


@pytest.mark.timeout(300)
@pytest.mark.parametrize('gran', [4, 16])
def test_bench_dimensions(bench_point, gran):
    Y, par = bench_point
    flags = _compare('200 x 10 x 500 x 32, rank_gran %d' % gran, Y, par, {'rank_gran': gran}, compact=(gran == 4))
    assert flags['lowrank_rtot'] > 256            # a block of more than one panel chunk
    if gran == 4:
        assert flags['lowrank_rtot'] < flags['lowrank_rtot16']      # ranks that are no multiples of 16: rows that go through the map


@pytest.mark.timeout(300)
@pytest.mark.parametrize('shape', [(40, 7, 203, 6), (33, 9, 203, 5)])
def test_empty_latents_and_ragged_bins(shape):
    q, p, T, R = shape
    rng = np.random.default_rng(q * 1000 + p)
    _, Ys, _ = orc.synth_dataset(q, p, T, R, seed=p, dOffset=0.0)
    Y = np.stack(Ys).astype(np.uint8)
    par = {'C': 0.3 * rng.standard_normal((q, p)) / np.sqrt(max(1, p / 4)), 'd': np.log(Y.mean(axis=(0, 2)) + 0.1), 'tau': 0.05 + 0.3 * rng.random(p)}
    _compare('%d x %d x %d x %d' % shape, Y, par, {}, compact=True)
