"""The kernels of the split covariance sum (csrc/split.h) on known inputs, through the E-step's own launch code (pgpfa_test_split_syrk,
pgpfa_test_split_latent_sums), against plain FP64 numpy.

* FP16 term (syrk_f16x2_kernel - fast and slow loads - and syrk256_f16x2_kernel): the reference is the FP64 product of the float32 inputs; the bound
  is 4 x the error that `emulate_syrk` - a numpy emulation of the documented arithmetic: scale by 2^11, hi = fp16(x), lo = fp16(x - hi), the products
  hh + hl + lh accumulated in FP32 in 32-column steps - makes on the same input against the same product (the factor 4 covers the accumulation order
  inside the matrix instruction, which is not specified).  tests/test_cpu_split_kernels.py shows without a GPU that this bound separates the kernel
  from three wrong ones (a half product lost, hi x hi only, one column lost) on exactly these inputs.
* latent sums (segmented-K GemmP products, cross_term_kernel, sum_groups_kernel): rel <= 1e-13 K, K = sps kw, the GEMM rule of test_gpu_kernels.py.

Every float of an input buffer that the sums must not see holds the poison value 7.0; outputs are prefilled with a sentinel and followed by a
sentinel band.  Every test prints what it measured."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

POISON = 7.0
SENTINEL = -3.0e33
BAND = 512
SCALE = 2048.0          # SPLIT_SCALE of split.h
KS = 32                 # columns per step of the FP16 kernels
PACC_SPLITS = 64


def round_up(a, b):
    return (a + b - 1) // b * b


def groups_of(nslots, sps):
    """(slots per group, groups) of the E-step's partition; sps = 0: its rule"""
    spe = sps if sps > 0 else max(1, (nslots + PACC_SPLITS - 1) // PACC_SPLITS)
    return spe, (nslots + spe - 1) // spe


# ---- FP16 term ---------------------------------------------------------------------------------------------------------------------------------
def _case(name, T, ts, ract, nslots, sps, p, tile, used, ldd_gap=0, spread=False):
    return dict(name=name, T=T, ts=ts, ldd=p * ts + ldd_gap, ract=ract, nslots=nslots, sps=sps, p=p, tile=tile, used=used, spread=spread)


SYRK_CASES = [
    # one step, dead waves (T < 128)
    _case('T64_p1', 64, 112, 16, 1, 1, 1, 128, 128),
    _case('T100_p3', 100, 112, 16, 1, 1, 3, 128, 128),
    _case('T64_p3', 64, 112, 16, 1, 1, 3, 128, 128),
    _case('T100_p1', 100, 112, 16, 1, 1, 1, 128, 128),
    # half-empty second step, odd / even number of steps (1, 3, 2, 6)
    _case('T130_r16_n1', 130, 144, 16, 1, 1, 3, 128, 128),
    _case('T130_r16_n3', 130, 144, 16, 3, 3, 3, 128, 128),
    _case('T130_r48_n1', 130, 144, 48, 1, 1, 3, 128, 128),
    _case('T130_r48_n3', 130, 144, 48, 3, 3, 3, 128, 128),
    # the load cursor crosses slots; ragged last group
    _case('T130_groups_of_2', 130, 144, 48, 5, 2, 3, 128, 128),
    # the E-step's rule above PACC_SPLITS: groups of 2, 34 groups, the last with one slot; 102 batch entries, no multiple of 8
    _case('T130_67_slots', 130, 144, 48, 67, 0, 3, 128, 128),
    # fast and slow tiles in one launch (i0 + 128 > ts)
    _case('T200_fast_and_slow', 200, 208, 48, 5, 2, 2, 128, 128),
    # slow loads everywhere: ts, ldd no multiples of 4
    _case('T203_slow', 203, 203, 48, 5, 2, 2, 128, 128, ldd_gap=1),
    # 256 kernel: 2 tiles ragged; 3 tiles exact and ragged
    _case('T500_256', 500, 512, 48, 5, 2, 3, 256, 256),
    _case('T768_256', 768, 768, 32, 3, 3, 1, 256, 256),
    _case('T520_256', 520, 768, 32, 3, 3, 1, 256, 256),
    # 256 refused by the stride rule (round_up(T, 256) > ts); 128 forced where 256 is allowed
    _case('T300_256_refused', 300, 304, 48, 3, 2, 2, 256, 128),
    _case('T500_128_forced', 500, 512, 48, 5, 2, 3, 128, 128),
    # per-row magnitudes spread over 1e-7 .. 0.1, error normalised by the latent's largest entry
    _case('T130_row_spread', 130, 144, 48, 5, 2, 3, 128, 128, spread=True),
]
SYRK_IDS = [c['name'] for c in SYRK_CASES]

_inputs = {}


def syrk_input(case):
    """(buffer float32 (nslots, round_up(ract, 32), ldd), valid float32 (nslots, ract, p, T)): seeded entries of magnitude 1e-3 .. 0.3, one scale per
    slot (spread: one scale per row, 1e-7 .. 0.1), poison in every float the sums must not see - columns >= ract, rows [T, ts), the gap behind p ts.
    Computed once per case and shared; callers must not write to it."""
    T, ts, ldd, ract, nslots, p = (case[k] for k in ('T', 'ts', 'ldd', 'ract', 'nslots', 'p'))
    key = (T, ts, ldd, ract, nslots, p, int(case['spread']))          # (the two T = 500 cases: the same data through both kernels)
    if key in _inputs:
        return _inputs[key]
    rng = np.random.default_rng(list(key))
    buf = np.full((nslots, round_up(ract, KS), ldd), POISON, dtype=np.float32)
    sign = np.where(rng.random((nslots, ract, p, T)) < 0.5, -1.0, 1.0)
    if case['spread']:
        mag = 10.0 ** rng.uniform(-7.0, -1.0, size=(1, 1, p, T)) * rng.uniform(0.5, 1.0, size=(nslots, ract, p, T))
    else:
        mag = rng.uniform(5e-3, 0.3, size=(nslots, 1, 1, 1)) * rng.uniform(0.2, 1.0, size=(nslots, ract, p, T))
    valid = (sign * mag).astype(np.float32)
    assert np.max(np.abs(valid)) <= 0.3 and (case['spread'] or np.min(np.abs(valid)) >= 1e-3)
    for k in range(p):
        buf[:, :ract, k * ts:k * ts + T] = valid[:, :, k, :]
    _inputs[key] = (buf, valid)
    return _inputs[key]


def syrk_reference(valid):
    """(p, T, T) FP64: sum over slots and columns of D_k[:, b] D_k[:, b]^T from the float32 inputs"""
    v = valid.astype(np.float64)
    return np.einsum('sbki,sbkj->kij', v, v, optimize=True)


def emulate_syrk(valid, sps, mutant=None):
    """The documented arithmetic of the FP16 kernels in numpy: x = 2^11 d (float32), hi = fp16(x), lo = fp16(x - hi); per group of sps slots a float32
    accumulator takes, per 32-column step, the products hi hi^T, lo hi^T, hi lo^T, each a float32 matrix product over the step's columns (a product of
    two halves is exact in float32: all rounding is in the float32 additions); the group results, scaled back in FP64, are summed in FP64.
    Returns (p, T, T).
    mutant: 'drop_lh' leaves the third product out, 'hh_only' the second and third, 'drop_column' skips column 0 of the slot with the largest entries."""
    nslots, ract, p, T = valid.shape
    x = (valid * np.float32(SCALE)).astype(np.float32)
    hi = x.astype(np.float16)
    lo = (x - hi.astype(np.float32)).astype(np.float16)
    hi, lo = hi.astype(np.float32), lo.astype(np.float32)
    if mutant == 'drop_column':
        s = int(np.argmax(np.max(np.abs(valid), axis=(1, 2, 3))))
        hi[s, 0] = 0.0
        lo[s, 0] = 0.0
    out = np.zeros((p, T, T))
    for k in range(p):
        for g0 in range(0, nslots, sps):
            acc = np.zeros((T, T), dtype=np.float32)
            for s in range(g0, min(nslots, g0 + sps)):
                for c0 in range(0, ract, KS):
                    h, l = hi[s, c0:c0 + KS, k, :], lo[s, c0:c0 + KS, k, :]
                    terms = [(h, h)] if mutant == 'hh_only' else [(h, h), (l, h)] if mutant == 'drop_lh' else [(h, h), (l, h), (h, l)]
                    for u, v in terms:
                        acc += u.T @ v
            out[k] += acc.astype(np.float64) / (SCALE * SCALE)
    return out


def syrk_error(case, res, ref):
    """largest error over the stored region i >= j and the latents: per entry relative to sqrt(ref_ii ref_jj); spread case: to the latent's largest entry"""
    T = ref.shape[1]
    low = np.tril(np.ones((T, T), dtype=bool))
    worst = 0.0
    for k in range(ref.shape[0]):
        if case['spread']:
            den = np.max(np.abs(ref[k]))
        else:
            dg = np.sqrt(np.diag(ref[k]))
            den = np.outer(dg, dg)
        worst = max(worst, float(np.max((np.abs(res[k] - ref[k]) / den)[low])))
    return worst


_refs = {}


def syrk_reference_and_bound(case):
    """(reference, emulation error, bound = 4 x emulation error), computed once per case"""
    spe, _ = groups_of(case['nslots'], case['sps'])
    key = tuple(case[k] for k in ('T', 'ts', 'ldd', 'ract', 'nslots', 'p', 'spread')) + (spe,)
    if key not in _refs:
        _, valid = syrk_input(case)
        ref = syrk_reference(valid)
        e_emu = syrk_error(case, emulate_syrk(valid, spe), ref)
        _refs[key] = (ref, e_emu, 4.0 * e_emu)
    return _refs[key]


@pytest.fixture(scope='module')
def ctx():
    from funs import _hip
    c = _hip.Context(7, 2, 20, 2, 10.0)
    yield c
    c.close()


_syrk_results = {}


@pytest.mark.parametrize('case', SYRK_CASES, ids=SYRK_IDS)
def test_fp16_term_against_the_fp64_product(ctx, case):
    T, p = case['T'], case['p']
    buf, valid = syrk_input(case)
    ref, e_emu, bound = syrk_reference_and_bound(case)
    spe, ng = groups_of(case['nslots'], case['sps'])
    part, tile_used, ngroups, tail = ctx.test_split_syrk(buf.reshape(case['nslots'], -1), T, p, case['ract'], case['ldd'], case['ts'], sps=case['sps'],
                                                         tile=case['tile'], fill=SENTINEL, band=BAND)
    assert tile_used == case['used'] and ngroups == ng and part.shape == (p, ng, T, T)
    assert np.all(tail == SENTINEL)
    low = np.tril(np.ones((T, T), dtype=bool))
    stored = part.transpose(0, 1, 3, 2)                    # [k, g, i, j]
    assert not np.any(stored[:, :, low] == SENTINEL), 'an entry of the stored region i >= j was not written'
    res = np.where(low, np.sum(np.where(stored == SENTINEL, 0.0, stored), axis=1), 0.0)
    e_ker = syrk_error(case, res, ref)
    print('%s: tile %d, %d groups of %d; kernel %.3e, emulation %.3e, ratio %.2f (bound 4)' % (case['name'], tile_used, ngroups, spe, e_ker, e_emu, e_ker / e_emu))
    _syrk_results[case['name']] = res
    assert e_ker <= bound
    if case['name'] == 'T500_128_forced' and 'T500_256' in _syrk_results:
        a, b = res, _syrk_results['T500_256']
        dg = np.sqrt(np.stack([np.diag(r) for r in ref]))
        print('T = 500: 128-tile and 256-tile results differ by %.3e of sqrt(ref_ii ref_jj)' % np.max(np.abs(a - b) / (dg[:, :, None] * dg[:, None, :])))


@pytest.mark.parametrize('bad', [dict(ts=63), dict(ldd=3 * 112 - 1), dict(tile=64)], ids=['ts_below_T', 'ldd_below_p_ts', 'tile_64'])
def test_fp16_hook_refuses_impossible_geometry(ctx, bad):
    from funs import _hip
    g = dict(T=64, p=3, ract=16, ldd=3 * 112, ts=112, tile=128)
    g.update(bad)
    D = np.zeros((1, 32 * g['ldd']), dtype=np.float32)
    with pytest.raises(_hip.HipBackendError):
        ctx.test_split_syrk(D, g['T'], g['p'], g['ract'], g['ldd'], g['ts'], sps=1, tile=g['tile'])


# ---- latent sums -------------------------------------------------------------------------------------------------------------------------------
# (rk, kw, T, row_off, (nslots, sps)): every value of the issue's lists appears; each combination runs with cross_kernel 1 and 0.  rk 144 and 256 take two
# launches of cross_term_kernel (row0 = 128); T = 70 and 130 leave a ragged last 64-column block and dead waves; 67 slots reach the 8-wide loop of
# sum_groups_kernel and its tail for S (67 groups) and X (34 groups).
SUMS_CASES = [
    (16, 16, 64, 0, (1, 1)), (48, 64, 70, 4, (5, 2)), (128, 16, 130, 12, (67, 0)), (144, 64, 64, 4, (5, 2)), (256, 16, 70, 12, (1, 1)),
    (256, 64, 130, 0, (5, 2)), (144, 16, 130, 0, (67, 0)), (48, 16, 130, 12, (1, 1)), (16, 64, 70, 4, (67, 0)), (128, 64, 64, 0, (5, 2)),
]

_sums_inputs = {}


def sums_input(rk, kw, T, row_off, nslots):
    """A float64 (nslots, kw lda + 8) and D float32 (nslots, kw ldd + 4), poison outside the rk rows / T rows / kw columns; the FP64 references."""
    key = (rk, kw, T, row_off, nslots)
    if key not in _sums_inputs:
        rng = np.random.default_rng(list(key))
        lda, ldd = rk + row_off + 20, T + 9
        A = np.full((nslots, kw * lda + 8), POISON)
        D = np.full((nslots, kw * ldd + 4), POISON, dtype=np.float32)
        a = rng.standard_normal((nslots, kw, rk))
        sign = np.where(rng.random((nslots, kw, T)) < 0.5, -1.0, 1.0)
        d = (sign * rng.uniform(5e-3, 0.3, size=(nslots, 1, 1)) * rng.uniform(0.2, 1.0, size=(nslots, kw, T))).astype(np.float32)
        A[:, :kw * lda].reshape(nslots, kw, lda)[:, :, row_off:row_off + rk] = a
        D[:, :kw * ldd].reshape(nslots, kw, ldd)[:, :, :T] = d
        S = np.einsum('sbi,sbj->ij', a, a, optimize=True)
        X = np.einsum('sbi,sbt->it', a, d.astype(np.float64), optimize=True)
        _sums_inputs[key] = (A, D, lda, ldd, S, X)
    return _sums_inputs[key]


def rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(1e-300, np.max(np.abs(b)))


@pytest.mark.parametrize('cross', [1, 0], ids=['cross_kernel', 'gemm'])
@pytest.mark.parametrize('rk,kw,T,row_off,slots', SUMS_CASES)
def test_latent_sums_against_fp64(ctx, rk, kw, T, row_off, slots, cross):
    nslots, sps = slots
    A, D, lda, ldd, S_ref, X_ref = sums_input(rk, kw, T, row_off, nslots)
    assert lda > rk + row_off
    spe, ng = groups_of(nslots, sps)
    S, X, tails = ctx.test_split_latent_sums(A, D, rk, kw, T, lda, row_off, ldd, sps=sps, cross_kernel=cross, fill=SENTINEL, band=BAND)
    assert np.all(tails[0] == SENTINEL) and np.all(tails[1] == SENTINEL)
    assert not np.any(S == SENTINEL) and not np.any(X == SENTINEL)
    K = spe * kw
    e_s, e_x = rel(S.T, S_ref), rel(X.T, X_ref)
    print('rk %d kw %d T %d row_off %d, %d slots in %d groups of %d, cross_kernel %d: S %.2e, X %.2e (allowed %.1e)' % (rk, kw, T, row_off, nslots, ng, spe, cross, e_s, e_x, 1e-13 * K))
    assert e_s <= 1e-13 * K and e_x <= 1e-13 * K
    blk = np.arange(rk) // 32                              # above the diagonal blocks: the mirror of the lower 32 x 32 blocks, bit for bit
    off = blk[:, None] != blk[None, :]
    assert np.array_equal(S[off], S.T[off])


@pytest.mark.parametrize('bad', [dict(rk=24), dict(kw=24), dict(lda=40), dict(ldd=60)], ids=['rk_24', 'kw_24', 'lda_small', 'ldd_below_T'])
def test_latent_sums_hook_refuses_impossible_geometry(ctx, bad):
    from funs import _hip
    g = dict(rk=48, kw=32, T=64, lda=64, ldd=64)
    g.update(bad)
    A = np.zeros((1, 64 * 64))
    D = np.zeros((1, 64 * 64), dtype=np.float32)
    with pytest.raises(_hip.HipBackendError):
        ctx.test_split_latent_sums(A, D, g['rk'], g['kw'], g['T'], g['lda'], 4, g['ldd'], sps=1, cross_kernel=1)
