"""B = I + F^T Wt F of the low-rank engine (csrc/model.h: assemble_b_kernel_t<double | float> and pad_identity_kernel) on known inputs, through the builder
of the rank tables and the launch code of the covariance pass (pgpfa_test_assemble_b), against numpy.longdouble.

Reference: B[a, b] = delta_ab + sum_t F_ka[t, a] Wt_t[ka, kb] F_kb[t, b], placed by a layout this file derives from the ranks on its own (`layout`); the
tables the hook used are asserted equal to it.  Inputs are seeded, magnitudes uniform in [0.5, 1.5] with random signs, Wt symmetric per bin (the kernel's
contract: it reads block (row latent, column latent) and feeds it to the column side).  The poison value 7.0 sits in slab rows [T, Tf), in slab columns
>= rk, behind every stride of Wt, in Wt of every slot that is not listed, in the 128 elements behind both inputs (the hook's `fill`) and in the whole
output.  Slab columns [rank, rk) are zero by contract.

Bound, derived: T accumulations with one rounding each, one rounding of the product F * w formed in registers, one of the added identity:
|got - exact| <= 1.01 (T + 2) u sum_t |f||w||f|, u = 2^-53.  float: F and Wt are rounded to float32 first (as the kernel loads them), u = 2^-24, plus
2^-24 |ref|.  Entries whose terms are all exact zeros (rows of a latent past its rank, identity rows) have bound 0 and must come back exact.
tests/test_cpu_assemble_b.py shows without a GPU that this bound separates wrong kernels from the right one on exactly these inputs.

Every case asserts the written set: the lower triangle of [0, rtot)^2 of the compact space plus what pad_identity_kernel owes (rows [rtot, rpad), lower,
below nact everywhere and beyond it inside the row's own 128-block); under gran 16 (no cmap) the whole lower triangle of rpad.  Every other entry - the
strict upper triangle, every unlisted slot - still holds the poison.  Every test prints what it measured."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

POISON = 7.0
U53 = 2.0 ** -53
U24 = 2.0 ** -24
LD = np.longdouble
SMALLEST_TERM = 0.125                                   # 0.5^3


def round_up(a, b):
    return (a + b - 1) // b * b


def layout(ranks, gran):
    """the rank tables of the r x r system from the ranks, restated from the description in build_lowrank (compact offsets for gran 4 and 8)"""
    p = len(ranks)
    rr = [round_up(max(r, 1), gran) for r in ranks]
    rk = [round_up(r, 16) for r in rr]
    roff, roff16 = [0], [0]
    for k in range(p):
        roff.append(roff[-1] + rr[k])
        roff16.append(roff16[-1] + rk[k])
    rtot, rtot16 = roff[-1], roff16[-1]
    rpad = round_up(max(rtot, max(roff[k] + rk[k] for k in range(p))), 128)
    n16 = round_up(rtot16, 128)
    blk_lat, blk_col = [-1] * (n16 // 16), [0] * (n16 // 16)
    cmap = [-1] * n16
    for k in range(p):
        for b in range(roff16[k] // 16, roff16[k + 1] // 16):
            blk_lat[b], blk_col[b] = k, 16 * b - roff16[k]
        for j in range(rr[k]):
            cmap[roff16[k] + j] = roff[k] + j
    compact = gran != 16
    n64 = round_up(rtot16, 64) // 64 if compact else rpad // 64
    return dict(p=p, rr=rr, rk=rk, roff=roff, roff16=roff16, rtot=rtot, rtot16=rtot16, rpad=rpad, compact=compact, blk_lat=blk_lat, blk_col=blk_col,
                cmap=cmap if compact else [], nact=round_up(rtot, 64), nblk64=n64, npairs=n64 * (n64 + 1) // 2)


SCRAMBLED_3_OF_7 = (5, 0, 3)


def case(T, ranks, gran=4, nslots=1, slots=None, shared=False, f32=False):
    ranks = tuple(min(r, T) for r in ranks)             # (a rank cannot exceed the number of bins: the hook refuses it)
    name = 'T%d_r%s_g%d' % (T, 'x'.join(map(str, ranks)) if len(ranks) < 6 else '%dx%d' % (ranks[0], len(ranks)), gran)
    if slots is not None:
        name += '_list%dof%d' % (len(slots), nslots)
    elif nslots != 1:
        name += '_n%d' % nslots
    if shared:
        name += '_shared'
    if f32:
        name += '_f32'
    return dict(name=name, T=T, ranks=ranks, gran=gran, nslots=nslots, slots=tuple(range(nslots)) if slots is None else tuple(slots), shared=shared, f32=f32)


BIN_T = (1, 5, 31, 32, 33, 64, 70, 100)
RANKS = ((4,), (132,), (60, 64), (20, 4, 68), (132, 8, 60), (16, 16, 16, 16, 16))


def rank_T(i, r):
    """T = 70 and 100 in turn; 140 where a rank of 132 needs that many bins (a rank above T is refused)"""
    return 140 if max(r) > 100 else (100, 70)[i % 2]


def _cases():
    out = []
    for f32 in (False, True):
        out += [case(T, (20, 4, 68), nslots=2, f32=f32) for T in BIN_T]                 # bins: one chunk and its tails, two and three chunks, a fourth
        for i, r in enumerate(RANKS):
            out.append(case(rank_T(i, r), r, 4, nslots=2, f32=f32))
        out.append(case(70, (8, 70), 4, nslots=2, f32=f32))                              # a full-rank last latent
    for gran in (8, 16):
        for i, r in enumerate(RANKS):
            out.append(case(rank_T(i, r), r, gran, nslots=2))
        out.append(case(70, (8, 70), gran, nslots=2))
    out += [case(70, (4,) * 10), case(70, (4,) * 20)]                                    # the p x p stride of Wt; five 64-blocks
    out += [case(70, (20, 4, 68), nslots=n) for n in (1, 3)]                             # a workgroup with one slot alone / a full one and a half one
    out.append(case(70, (20, 4, 68), nslots=7, slots=SCRAMBLED_3_OF_7))
    out.append(case(70, (20, 4, 68), shared=True))                                       # sW = 0: the shared preconditioner's call
    out.append(case(140, (132, 8, 60), 16, shared=True))
    return list({c['name']: c for c in out}.values())


CASES = _cases()
CASE_IDS = [c['name'] for c in CASES]

_inputs = {}


def assemble_input(c):
    """Inputs of a case, computed once and shared (callers must not write to them): the layout, F (p, Tf, Tf) [latent, column, bin], Wt (nslots, sW) - or
    (T p p,) for the shared slot -, sW as passed to the hook, B0 the poisoned output (nslots, rpad, rpad)"""
    key = c['name']
    if key in _inputs:
        return _inputs[key]
    T, ranks, nslots = c['T'], c['ranks'], c['nslots']
    g = layout(ranks, c['gran'])
    p = g['p']
    rng = np.random.default_rng([T, c['gran'], nslots, int(c['f32']), int(c['shared']), len(c['slots'])] + list(ranks))

    def rnd(*shape):
        return rng.uniform(0.5, 1.5, size=shape) * np.where(rng.random(shape) < 0.5, -1.0, 1.0)

    Tf = round_up(T, 32) + 2
    F = np.full((p, Tf, Tf), POISON)
    for l in range(p):
        F[l, :g['rk'][l], :T] = 0.0
        F[l, :ranks[l], :T] = rnd(ranks[l], T)
    wbin = T * p * p
    if c['shared']:
        assert nslots == 1
        sW, Wt = 0, np.empty((1, wbin))
    else:
        sW = wbin + 3
        Wt = np.full((nslots, sW), POISON)
    for s in c['slots']:
        up = np.triu(rnd(T, p, p))
        Wt[s, :wbin] = (up + np.transpose(np.triu(up, 1), (0, 2, 1))).reshape(-1)
    if c['shared']:
        Wt = Wt.reshape(-1)
    g.update(T=T, Tf=Tf, ranks=ranks, F=F, Wt=Wt, sW=sW, wbin=wbin, B0=np.full((nslots, g['rpad'], g['rpad']), POISON, dtype=np.float32 if c['f32'] else np.float64))
    _inputs[key] = g
    return g


# ---- reference and bound ---------------------------------------------------------------------------------------------------------------------------
FAULTS = ('drop_run', 'neighbour_pair', 'cmap_shift', 'second_slot', 'identity_padded')


def written_mask(g):
    """[row, col]: what the two kernels store, for every listed slot alike"""
    rtot, rpad, nact = g['rtot'], g['rpad'], g['nact']
    row, col = np.meshgrid(np.arange(rpad), np.arange(rpad), indexing='ij')
    low = row >= col
    if not g['compact']:
        return low
    pad = (row >= rtot) & ((row < nact) | (col >= row // 128 * 128))
    return low & (((row < rtot) & (col < rtot)) | pad)


def slot_matrix(c, g, s, fault=None, unrounded_weights=False):
    """(M, bound) of slot s in the compact space, [row, col], all of [0, rtot)^2 (the caller keeps the lower triangle)"""
    T, p, rtot = g['T'], g['p'], g['rtot']
    u = U24 if c['f32'] else U53
    W = (g['Wt'].reshape(-1)[:g['wbin']] if c['shared'] else g['Wt'][s, :g['wbin']]).reshape(T, p, p)
    A = [g['F'][l, :g['rr'][l], :T] for l in range(p)]
    if c['f32']:
        A = [a.astype(np.float32).astype(np.float64) for a in A]
        if not unrounded_weights:
            W = W.astype(np.float32).astype(np.float64)
    M = np.zeros((rtot, rtot), dtype=LD)
    S = np.zeros((rtot, rtot))
    for a in range(p):
        Aa = A[a].astype(LD)
        if fault == 'drop_run' and a == 0:              # one 4-bin run of the row side of latent 0 never summed
            Aa = Aa.copy()
            t0 = 4 * (T // 8)
            Aa[:, t0:t0 + 4] = 0.0
        for b in range(a + 1):
            w = W[:, a, b]
            if fault == 'neighbour_pair' and a == p - 1 and b == p - 1:      # the weight block of the neighbouring latent pair
                w = W[:, a, b - 1]
            ra, rb = slice(g['roff'][a], g['roff'][a + 1]), slice(g['roff'][b], g['roff'][b + 1])
            M[ra, rb] = (Aa * w.astype(LD)) @ A[b].astype(LD).T
            S[ra, rb] = (np.abs(A[a]) * np.abs(w)) @ np.abs(A[b]).T
    d = np.arange(rtot)
    if fault == 'identity_padded':                      # the 1 stored where the PADDED index of a real row says, not at its compact place
        real = [i for i, v in enumerate(g['cmap']) if v >= 0 and i < rtot]
        M[real, real] += 1.0
    else:
        M[d, d] += 1.0
    bound = 1.01 * (T + 2) * u * S
    if c['f32']:
        bound = bound + U24 * np.abs(M).astype(np.float64)
    if fault == 'cmap_shift':                           # the last latent stored one 4-row run further on; what falls out of [0, rtot) is lost
        idx = np.arange(rtot)
        idx[g['roff'][p - 1]:] += 4
        keep = idx < rtot
        Mm = np.full((rtot, rtot), LD(POISON))
        Mm[np.ix_(idx[keep], idx[keep])] = M[np.ix_(keep, keep)]
        M = Mm
    return M, bound


def reference(c, fault=None, unrounded_weights=False):
    """(ref, bound, written), (nslots, rpad, rpad) indexed [slot, row, col]: the exact result in longdouble, the bound on |got - ref| (float64), which
    entries the contract says are stored.  Entries not written hold POISON in ref.  fault: None or one of FAULTS (tests/test_cpu_assemble_b.py)."""
    g = assemble_input(c)
    nslots, rtot, rpad = c['nslots'], g['rtot'], g['rpad']
    ref = np.full((nslots, rpad, rpad), LD(POISON))
    bound = np.zeros((nslots, rpad, rpad))
    written = np.zeros((nslots, rpad, rpad), dtype=bool)
    wm = written_mask(g)
    eye = np.eye(rpad, dtype=LD)
    for i, s in enumerate(c['slots']):
        src = c['slots'][i - 1] if (fault == 'second_slot' and i % 2 == 1) else s       # the second slot of a workgroup reads the first one's weights
        M, b = slot_matrix(c, g, src, None if fault == 'second_slot' else fault, unrounded_weights)
        full, fb = eye.copy(), np.zeros((rpad, rpad))
        full[:rtot, :rtot], fb[:rtot, :rtot] = M, b
        ref[s][wm], bound[s][wm], written[s] = full[wm], fb[wm], wm
    return ref, bound, written


def worst_ratio(got, ref, bound, written):
    """largest |got - ref| / bound over the written entries (an entry with bound 0 must be exact: inf otherwise)"""
    d = np.abs(got[written].astype(LD) - ref[written])
    b = bound[written]
    if d.size == 0:
        return 0.0
    with np.errstate(divide='ignore', invalid='ignore'):
        q = np.where(d == 0, 0.0, np.where(b > 0, d / np.where(b > 0, b, 1), np.inf))
    return float(np.max(q))


# ---- GPU --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def ctx():
    from funs import _hip
    c = _hip.Context(4, 2, 8, 1, 10.0)                  # (no parameters, no counts: the hook only borrows the stream)
    yield c
    c.close()


def run(ctx, c, slots=None, Wt=None):
    g = assemble_input(c)
    got, info = ctx.test_assemble_b(g['T'], g['Tf'], g['ranks'], c['gran'], g['F'], g['Wt'] if Wt is None else Wt, g['B0'], slots=c['slots'] if slots is None else slots,
                                    sW=g['sW'], f32=c['f32'], fill=POISON)
    return np.transpose(got, (0, 2, 1)), info           # [slot, row, col]


def check_tables(info, g):
    for k in ('rr', 'rk', 'roff', 'roff16', 'blk_lat', 'blk_col', 'cmap'):
        assert list(info[k]) == list(g[k]), k
    for k in ('rtot', 'rtot16', 'rpad', 'compact', 'nblk64', 'npairs', 'nact'):
        assert info[k] == g[k], k


@pytest.mark.parametrize('c', CASES, ids=CASE_IDS)
def test_assembly_against_longdouble(ctx, c):
    g = assemble_input(c)
    got, info = run(ctx, c)
    check_tables(info, g)
    ref, bound, written = reference(c)
    ratio = worst_ratio(got, ref, bound, written)
    print('%s: rtot %d, rpad %d, %d entries written, worst |got - ref| / bound %.3g' % (c['name'], g['rtot'], g['rpad'], int(np.sum(written)), ratio))
    assert np.any(written)
    assert not np.any(got[written] == POISON), 'an entry the contract says is written still holds the poison'
    assert np.all(got[~written] == POISON), 'an entry outside the contract was stored'
    assert ratio <= 1.0, ratio


def test_result_of_a_slot_does_not_depend_on_the_launch(ctx):
    """slot 5 alone, first of two, second of two (the same workgroup), third of three (a workgroup of its own): the same bits"""
    base = case(70, (20, 4, 68), nslots=7, slots=SCRAMBLED_3_OF_7)
    g = assemble_input(base)
    Wt = g['Wt'].copy()
    Wt[[1, 2, 4, 6]] = Wt[0]                            # every slot readable
    ref, bound, written = reference(base)
    results = {}
    for slots in ((5,), (5, 2), (2, 5), (0, 2, 5)):
        got, _ = run(ctx, base, slots=slots, Wt=Wt)
        assert not np.any(got[5][written[5]] == POISON)
        for s in range(7):
            if s not in slots:
                assert np.all(got[s] == POISON)
        results[slots] = got[5][written[5]].copy()
    first = results[(5,)]
    assert worst_ratio(first, ref[5][written[5]], bound[5][written[5]], np.ones(first.shape, dtype=bool)) <= 1.0
    for slots, r in results.items():
        assert np.array_equal(r.view(np.uint64), first.view(np.uint64)), slots


REFUSALS = [
    ('Tf below round_up(T, 32)', 'Tf', dict(Tf=95)),
    ('Tf below T', 'Tf', dict(Tf=64)),
    ('rank above T', 'rank', dict(ranks=(20, 4, 71))),
    ('rank 0', 'rank', dict(ranks=(20, 0, 68))),
    ('list entry outside the slots', 'list', dict(slots=(0, 3))),
    ('negative list entry', 'list', dict(slots=(-1, 1))),
    ('slot listed twice', 'list', dict(slots=(1, 0, 1))),
    ('weight stride below T p^2', 'stride', dict(sW=70 * 9 - 1)),
    ('shared weights with two slots', 'stride', dict(sW=0)),
    ('granularity 5', 'bad_arg', dict(gran=5)),
    ('output sized for another rpad', 'bad_arg', dict(rpad=256)),
]


@pytest.mark.parametrize('what,refusal,over', REFUSALS, ids=[r[0].replace(' ', '_') for r in REFUSALS])
def test_impossible_geometry_is_refused(ctx, what, refusal, over):
    """refused by a return code of its own, before anything is allocated or launched"""
    from funs import _hip
    geo = dict(T=70, Tf=96, ranks=(20, 4, 68), gran=4, slots=(0, 1, 2), sW=70 * 9, rpad=128)
    geo.update(over)
    F = np.zeros((3, geo['Tf'], geo['Tf']))
    Wt = np.zeros((3, max(geo['sW'], 70 * 9)))
    B = np.full((3, geo['rpad'], geo['rpad']), POISON)
    with pytest.raises(_hip.HipBackendError) as e:
        ctx.test_assemble_b(geo['T'], geo['Tf'], geo['ranks'], geo['gran'], F, Wt, B, slots=geo['slots'], sW=geo['sW'], fill=POISON)
    print('%s: rc %d, "%s"' % (what, e.value.rc, e.value))
    assert e.value.refusal == refusal, (e.value.rc, str(e.value))
    assert e.value.rc == {v: k for k, v in ctx.ASMB_REFUSALS.items()}[refusal]


LAYOUT_GEOMETRIES = [(ranks, gran) for ranks in ((1,), (4,), (20,), (132,), (200,), (60, 64), (20, 4, 68), (132, 8, 60), (64, 80, 4), (3, 17, 5), (128, 192, 196),
                                                 (16,) * 5, (4,) * 10, (4,) * 20, (12, 4, 4, 4, 28, 52), (8, 200), (1, 1, 1), (13, 7), (36, 36, 36, 36), (124, 4),
                                                 (4, 124), (60, 4, 60, 4), (100, 100, 100, 100, 100), (9,) * 7, (48, 16, 80), (2,) * 32, (68, 60), (7, 130, 11),
                                                 (44, 44, 44), (24, 40, 56, 72), (5,), (127,), (129,), (33, 31))
                     for gran in (4, 8, 16)]


def test_tables_describe_the_layout(ctx):
    """the tables the hook used (returned by it), over 102 geometries, one launch on one slot each: cmap is a monotone bijection from the real padded rows
    onto [0, rtot), 16-blocks never straddle a latent, row pairs can be moved whole (the check of the rank tables' owner)"""
    assert len(LAYOUT_GEOMETRIES) >= 100
    for ranks, gran in LAYOUT_GEOMETRIES:
        g = layout(ranks, gran)
        p, T = len(ranks), max(max(ranks), 4)
        Tf = round_up(T, 32)
        _, info = ctx.test_assemble_b(T, Tf, ranks, gran, np.zeros((p, Tf, Tf)), np.zeros((1, T * p * p)), np.zeros((1, g['rpad'], g['rpad'])))
        check_tables(info, g)
        rr, rk, roff, roff16, rtot, rtot16 = list(info['rr']), list(info['rk']), list(info['roff']), list(info['roff16']), info['rtot'], info['rtot16']
        assert all(r % gran == 0 and r >= q for r, q in zip(rr, ranks)) and rk == [round_up(r, 16) for r in rr]
        assert roff == list(np.concatenate([[0], np.cumsum(rr)])) and roff16 == list(np.concatenate([[0], np.cumsum(rk)]))
        assert info['rpad'] % 128 == 0 and info['rpad'] >= max(rtot, max(roff[k] + rk[k] for k in range(p)))
        lat, col = info['blk_lat'], info['blk_col']
        assert len(lat) * 16 == round_up(rtot16, 128) and len(lat) >= 4 * info['nblk64']
        for b in range(len(lat)):                       # a 16-block belongs to one latent as a whole, or lies behind the last
            inside = [k for k in range(p) if roff16[k] <= 16 * b < roff16[k + 1]]
            assert (lat[b] == -1 and not inside and 16 * b >= rtot16) or (inside == [lat[b]] and 16 * b + 16 <= roff16[lat[b] + 1] and col[b] == 16 * b - roff16[lat[b]])
        assert info['compact'] == (gran != 16)
        if gran == 16:
            assert len(info['cmap']) == 0 and roff == roff16 and info['nblk64'] * 64 == info['rpad']
            continue
        cmap = info['cmap']
        assert len(cmap) == round_up(rtot16, 128) and len(cmap) >= 64 * info['nblk64'] >= rtot16
        real = [i for i in range(len(cmap)) if cmap[i] >= 0]
        assert [cmap[i] for i in real] == list(range(rtot))                  # monotone, onto [0, rtot), one to one
        assert real == [roff16[k] + j for k in range(p) for j in range(rr[k])]
        for i in range(0, len(cmap) - 1, 2):
            assert (cmap[i] < 0 and cmap[i + 1] < 0) or (cmap[i] >= 0 and cmap[i] % 2 == 0 and cmap[i + 1] == cmap[i] + 1)
