"""The thin products of the low-rank preconditioner y = F Sb F^T t (csrc/thin.h: thin_ft_kernel for u = F^T t and v = Sb u, thin_f_kernel for y = F v)
on known inputs, through the table builder of the rank tables and the launch code of the inner solve (pgpfa_test_thin), against numpy.longdouble.

Inputs are seeded, magnitudes uniform in [0.5, 1.5] with random signs (every product term is at least 0.25 in magnitude); float-typed vectors are rounded to
float32 before the reference sees them.  The poison value 7.0 sits wherever the header of thin.h says the result does not depend on the value: FT outside
each latent's own rr rows, slab rows t >= T and slab columns >= rk, vector rows [T, Tx) and past the last latent, rank-space rows >= rtot (for apply also
rows [rtot, rpad) of the intermediates), every column of a slot that is not in the list, the 128 elements behind every input, and the whole output.  Slab
columns [rank, rk) are zero by contract; the vector rows they meet are the next latent's real values (compact offsets).

Bound, derived: a sum of K terms accumulated with one rounding per step is within  1.01 K 2^-53 sum |f| |x|  of the exact sum, entry by entry; K = T for
ft, rk_l for f, rtot for s; apply composes the three (the error of a stage enters the next through |Sb| and |F|); float output adds 2^-24 |ref|.
tests/test_cpu_thin_kernels.py shows without a GPU that this bound separates four wrong kernels from the right one on exactly these inputs.

Every case asserts: every entry the contract says is written differs from the poison, every other entry still holds it, the band behind the output is
intact (the hook fails otherwise).  Every test prints what it measured (worst |got - ref| / bound)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

POISON = 7.0
U53 = 2.0 ** -53
U24 = 2.0 ** -24
LD = np.longdouble


def round_up(a, b):
    return (a + b - 1) // b * b


def geometry(ranks, gran):
    """rank tables by the rule of build_lowrank: (rr, rk, roff, rtot, rpad)"""
    rr = [round_up(max(r, 1), gran) for r in ranks]
    rk = [round_up(r, 16) for r in rr]
    roff = [0]
    for r in rr:
        roff.append(roff[-1] + r)
    extent = max(o + k for o, k in zip(roff, rk))
    return rr, rk, roff, roff[-1], round_up(max(roff[-1], extent), 128)


def expected_tables(T, ranks, gran):
    """the three work tables, restated from the description in build_lowrank / thin.h"""
    rr, rk, roff, rtot, _ = geometry(ranks, gran)
    ft, f, s = [], [], []
    for l in range(len(ranks)):
        ngr, runs = (rr[l] + 63) // 64, rr[l] // 4
        sizes = [4 * (runs // ngr + (1 if i < runs % ngr else 0)) for i in range(ngr)]
        ft += [(l, sum(sizes[:i]), sizes[i], roff[l]) for i in range(ngr)]
        f += [(l, t0, rk[l], roff[l]) for t0 in range(0, T, 256)]
    s = [(0, m0, min(64, rtot - m0), 0) for m0 in range(0, rtot, 64)]
    return np.array(ft).reshape(-1, 4), np.array(f).reshape(-1, 4), np.array(s).reshape(-1, 4)


SCRAMBLED_17_OF_40 = [23, 5, 38, 0, 17, 31, 9, 2, 36, 14, 27, 39, 7, 20, 11, 33, 4]


def case(kind, T, ranks, gran=4, ncols=5, cols=None, nslots=None, live=None, stop=None, f32=False, pad16=False):
    ranks = tuple(ranks)
    name = '%s_T%d_r%s_g%d' % (kind, T, 'x'.join(map(str, ranks)), gran)
    if cols is not None:
        name += '_list%dof%d' % (len(cols), nslots)
    elif ncols != 5:
        name += '_n%d' % ncols
    if live is not None:
        name += '_live%d' % live
    if stop is not None:
        name += '_stop%d' % stop
    if f32:
        name += '_f32'
    return dict(name=name, kind=kind, T=T, ranks=ranks, gran=gran, ncols=len(cols) if cols is not None else ncols, cols=None if cols is None else tuple(cols),
                nslots=nslots if nslots is not None else ncols, live=live, stop=stop, f32=f32, Tx=round_up(T, 16) if pad16 else T)


BIN_T_FT = [4, 5, 16, 17, 63, 64, 100, 127, 130, 131, 260]
BIN_T_F = [4, 5, 63, 64, 65, 100, 255, 256, 257, 260]
RANKS = [4, 8, 16, 20, 60, 64, 68, 80, 132]


def _rank_cases():
    out = []
    for kind in ('ft', 'f'):
        for gran in (4, 8, 16):
            for i, r in enumerate(RANKS):
                out.append(case(kind, 100, (r,), gran))                                             # p = 1: T % 4 == 0
                out.append(case(kind, 70, (r, 4, RANKS[(i + 3) % len(RANKS)]), gran))               # p = 3: T % 4 != 0, a 4-row latent in the middle
            out.append(case(kind, 70, (20, 4, 68), gran))
            out.append(case(kind, 100, (132, 8, 60), gran))
    return out


def _column_cases():
    out = []
    for kind in ('ft', 'f'):
        for n in (1, 15, 16, 17, 33):
            out.append(case(kind, 100, (20, 4, 68), ncols=n))
        out.append(case(kind, 100, (20, 4, 68), cols=SCRAMBLED_17_OF_40, nslots=40))
        for live in (0, 5, 16, 17):
            out.append(case(kind, 100, (20, 4, 68), cols=SCRAMBLED_17_OF_40, nslots=40, live=live))
        out.append(case(kind, 100, (20, 4, 68), cols=SCRAMBLED_17_OF_40, nslots=40, live=17, stop=1))
        out.append(case(kind, 100, (20, 4, 68), cols=SCRAMBLED_17_OF_40, nslots=40, live=17, stop=0))
    return out


CASES = (
    # ft, bins: one k-block with seven idle waves, both VEC4 forms, uneven wave shares, an odd THIN_KB tail at 260
    [case('ft', T, (20,), ncols=17) for T in BIN_T_FT] + [case('ft', T, (20, 4, 68), ncols=17) for T in (5, 64, 131, 260)]
    # f, bins: a wave with no bins, a second 256-bin group, both store forms
    + [case('f', T, (20, 4, 68), ncols=17) for T in BIN_T_F]
    # ranks: a single partial tile, exactly 64, 40 + 40, 3 x 44; compact offsets with gran 4 and 8
    + _rank_cases()
    + _column_cases()
    # float storage of the n-vectors in the inner solve's private layout
    + [case(kind, T, (20, 4, 68), ncols=17, f32=True, pad16=True) for kind in ('ft', 'f') for T in (100, 130)]
    + [case('s', 8, (r,), ncols=17) for r in (4, 28, 64, 92, 200)]
    + [case('apply', 100, (20, 4, 68), 4, ncols=17), case('apply', 131, (60, 64), 16, cols=SCRAMBLED_17_OF_40, nslots=40, live=17),
       case('apply', 260, (132, 8, 60), 4, ncols=17)]
)
CASES = list({c['name']: c for c in CASES}.values())       # (the groups above overlap in a few cases: each once)
CASE_IDS = [c['name'] for c in CASES]

_inputs = {}


def thin_input(c):
    """Inputs of a case, computed once and shared (callers must not write to them): dict with the geometry, F (p, Tf, Tf) [latent, column, bin],
    Sb (rpad, rpad) [k, m] symmetric, X (nslots, ld) in its storage type, Y0 the poisoned output buffer, and `listed`: the slots of the list in order."""
    key = (c['kind'], c['T'], c['ranks'], c['gran'], c['ncols'], c['cols'], c['nslots'], c['f32'], c['Tx'])
    if key in _inputs:
        return _inputs[key]
    kind, T, Tx, ranks, p, nslots = c['kind'], c['T'], c['Tx'], c['ranks'], len(c['ranks']), c['nslots']
    rr, rk, roff, rtot, rpad = geometry(ranks, c['gran'])
    rng = np.random.default_rng([sum(ord(ch) for ch in kind), T, Tx, c['gran'], c['ncols'], nslots, int(c['f32'])] + list(ranks))

    def rnd(*shape):
        return rng.uniform(0.5, 1.5, size=shape) * np.where(rng.random(shape) < 0.5, -1.0, 1.0)

    Tf = round_up(max(T, max(rk)), 4) + 4
    nrows = (p - 1) * Tx + T
    ld = max(round_up(nrows, 4), rpad) + 4
    F = np.full((p, Tf, Tf), POISON)
    for l in range(p):
        F[l, :rk[l], :T] = 0.0
        F[l, :ranks[l], :T] = rnd(ranks[l], T)
    up = np.triu(rnd(rpad, rpad))
    Sb = np.full((rpad, rpad), POISON)
    Sb[:rtot, :rtot] = (up + np.triu(up, 1).T)[:rtot, :rtot]
    listed = list(c['cols']) if c['cols'] is not None else list(range(c['ncols']))
    n_in = kind in ('ft', 'apply')                      # the input is an n-vector
    n_out = kind in ('f', 'apply')
    X = np.full((nslots, ld), POISON, dtype=np.float32 if (c['f32'] and n_in) else np.float64)
    for s in listed:
        if n_in:
            for l in range(p):
                X[s, l * Tx:l * Tx + T] = rnd(T)
        else:
            X[s, :rtot] = rnd(rtot)
    Y0 = np.full((nslots, ld), POISON, dtype=np.float32 if (c['f32'] and n_out) else np.float64)
    _inputs[key] = dict(T=T, Tx=Tx, Tf=Tf, p=p, ranks=ranks, rr=rr, rk=rk, roff=roff, rtot=rtot, rpad=rpad, ld=ld, F=F, Sb=Sb, X=X, Y0=Y0, listed=listed,
                        tables=expected_tables(T, ranks, c['gran']))
    return _inputs[key]


# ---- reference and bound in numpy.longdouble --------------------------------------------------------------------------------------------------
# Every stage returns (exact result, bound on |computed - exact|) for all slots, given its input and a bound on the input's own error.
# fault: None, or one of the wrong kernels of tests/test_cpu_thin_kernels.py.
def stage_ft(g, x, ex, fault=None):
    """u[s, roff_l + j] = sum_t F_l[t, j] x[s, l Tx + t], j < rr_l"""
    T, Tx, p = g['T'], g['Tx'], g['p']
    u = np.zeros((x.shape[0], g['rtot']), dtype=LD)
    b = np.zeros_like(u)
    for l in range(p):
        cols = np.arange(g['rr'][l])
        if fault == 'shift_group' and l == p - 1:       # the last row group of the last latent reads the factor rows 4 further on
            _, m0, rows, _ = g['tables'][0][-1]
            cols[m0:m0 + rows] += 4
        A = g['F'][l][cols, :T].astype(LD)              # (rr, T)
        if fault == 'drop_run' and l == 0:              # one 4-bin run of one latent never summed
            t0 = 4 * (T // 8)
            A[:, t0:t0 + 4] = 0.0
        xs, es = x[:, l * Tx:l * Tx + T], ex[:, l * Tx:l * Tx + T]
        u[:, g['roff'][l]:g['roff'][l] + g['rr'][l]] = xs @ A.T
        b[:, g['roff'][l]:g['roff'][l] + g['rr'][l]] = es @ np.abs(A).T + 1.01 * T * U53 * ((np.abs(xs) + es) @ np.abs(A).T)
    if fault == 'rk_rows':                              # a latent stores rk rows, not rr: zeros over the next latent's first rows
        for l in range(p - 1):
            u[:, g['roff'][l] + g['rr'][l]:g['roff'][l] + g['rk'][l]] = 0.0
    return u, b


def stage_s(g, u, eu, fault=None):
    """v[s, m] = sum_k Sb[m, k] u[s, k], k, m < rtot"""
    rtot = g['rtot']
    S = g['Sb'][:rtot, :rtot].astype(LD)                # [k, m]
    if fault == 'drop_run':
        k0 = 4 * (rtot // 8)
        S[k0:k0 + 4, :] = 0.0
    if fault == 'shift_group':
        _, m0, rows, _ = g['tables'][2][-1]
        S[:, m0:m0 + rows] = g['Sb'][:rtot, m0 + 4:m0 + rows + 4]
    return u @ S, eu @ np.abs(S) + 1.01 * rtot * U53 * ((np.abs(u) + eu) @ np.abs(S))


def stage_f(g, v, ev, fault=None):
    """y[s, l Tx + t] = sum_j F_l[t, j] v[s, roff_l + j], j < rk_l (columns [rank_l, rk_l) of F_l are zero; v there is the next latent's).
    v, ev: (slots, >= roff_l + rk_l + 4) - the rank-space rows as the device buffer holds them"""
    T, Tx, p = g['T'], g['Tx'], g['p']
    y = np.zeros((v.shape[0], (p - 1) * Tx + T), dtype=LD)
    b = np.zeros_like(y)
    r16 = 0
    for l in range(p):
        rk = g['rk'][l]
        A = g['F'][l][:rk, :T].astype(LD)               # (rk, T)
        if fault == 'drop_run' and l == 0:              # one run of four rank columns never summed
            A[0:4, :] = 0.0
        r0 = g['roff'][l]
        if fault == 'shift_group' and l == p - 1:       # the vector rows read 4 further on
            r0 += 4
        if fault == 'rk_rows':                          # offsets that count rk rows per latent, not rr
            r0 = r16
        r16 += rk
        vs, es = v[:, r0:r0 + rk], ev[:, r0:r0 + rk]
        y[:, l * Tx:l * Tx + T] = vs @ A
        b[:, l * Tx:l * Tx + T] = es @ np.abs(A) + 1.01 * rk * U53 * ((np.abs(vs) + es) @ np.abs(A))
    return y, b


def reference(c, fault=None):
    """(ref, bound, written): the exact result in the layout of the output buffer, longdouble (nslots, ld); the bound on |got - ref|; which entries the
    contract says are stored.  Entries not written hold POISON in ref.
    fault (see tests/test_cpu_thin_kernels.py): 'drop_run', 'shift_group', 'rk_rows', 'swap_cols'"""
    g = thin_input(c)
    kind, T, Tx, p, rtot, ld, nslots = c['kind'], g['T'], g['Tx'], g['p'], g['rtot'], g['ld'], c['nslots']
    x = g['X'].astype(LD)
    zero = np.zeros_like(x)
    kf = None if fault == 'swap_cols' else fault
    if kind == 'ft':
        r, b = stage_ft(g, x, zero, kf)
    elif kind == 's':
        r, b = stage_s(g, x[:, :rtot], zero[:, :rtot], kf)
    elif kind == 'f':
        r, b = stage_f(g, x, zero, kf)
    else:
        u, bu = stage_ft(g, x, zero, kf)
        v, bv = stage_s(g, u, bu)
        # (rows [rtot, rpad) of the intermediate hold the poison; they meet zero columns of the last slab)
        vfull = np.full((nslots, ld), LD(POISON))
        vfull[:, :rtot] = v
        bfull = np.zeros((nslots, ld), dtype=LD)
        bfull[:, :rtot] = bv
        r, b = stage_f(g, vfull, bfull)
    if c['f32'] and kind in ('f', 'apply'):
        b = b + U24 * np.abs(r)
    live = len(g['listed']) if c['live'] is None else c['live']
    stored = [] if c['stop'] == 1 else g['listed'][:live]
    if fault == 'swap_cols':                            # the first two columns of the list stored into each other's slot
        r, b = r.copy(), b.copy()
        r[[stored[0], stored[1]]] = r[[stored[1], stored[0]]]
    ref = np.full((nslots, ld), LD(POISON))
    bound = np.zeros((nslots, ld), dtype=LD)
    written = np.zeros((nslots, ld), dtype=bool)
    for s in stored:
        if kind in ('ft', 's'):
            rows = np.arange(rtot)
        else:
            rows = np.concatenate([l * Tx + np.arange(T) for l in range(p)])
        ref[s, rows], bound[s, rows], written[s, rows] = r[s, rows], b[s, rows], True
    return ref, bound, written


def worst_ratio(got, ref, bound, written):
    """largest |got - ref| / bound over the written entries (an entry with bound 0 must be exact: inf otherwise; 0.0 if nothing is written)"""
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


def run(ctx, c, **over):
    g = thin_input(c)
    kw = dict(Tx=g['Tx'], F=g['F'], Sb=g['Sb'], f32=c['f32'], cols=c['cols'], ncols=c['ncols'], live=c['live'], stop=c['stop'], fill=POISON)
    kw.update(over)
    return ctx.test_thin(c['kind'], g['T'], g['Tf'], g['ranks'], c['gran'], g['X'], g['Y0'], **kw)


@pytest.mark.parametrize('c', CASES, ids=CASE_IDS)
def test_thin_product_against_longdouble(ctx, c):
    g = thin_input(c)
    got, info = run(ctx, c)
    ref, bound, written = reference(c)
    assert info['rtot'] == g['rtot'] and info['rpad'] == g['rpad'] and list(info['rr']) == g['rr'] and list(info['rk']) == g['rk'] and list(info['roff']) == g['roff']
    for have, want in zip((info['ft'], info['f'], info['s']), g['tables']):
        assert np.array_equal(have, want)
    ratio = worst_ratio(got, ref, bound, written)
    print('%s: %d entries written, worst |got - ref| / bound %.3g' % (c['name'], int(np.sum(written)), ratio))
    assert not np.any(got[written] == POISON), 'an entry the contract says is written still holds the poison'
    assert np.all(got[~written] == POISON), 'an entry outside the contract was stored'
    assert c['stop'] == 1 or c['live'] == 0 or np.any(written)
    assert ratio <= 1.0, ratio


@pytest.mark.parametrize('c', [c for c in CASES if c['kind'] == 'apply'], ids=[n for n in CASE_IDS if n.startswith('apply')])
def test_apply_is_symmetric(ctx, c):
    """Sb is symmetric, so F Sb F^T is: t^T (apply s) = s^T (apply t), to the bounds of the two results"""
    g = thin_input(c)
    got, _ = run(ctx, c)
    ref, bound, written = reference(c)
    i, j = g['listed'][0], g['listed'][1]
    rows = written[i]
    t, s = g['X'][i, rows].astype(LD), g['X'][j, rows].astype(LD)
    a, b = np.sum(t * got[j, rows].astype(LD)), np.sum(s * got[i, rows].astype(LD))
    allowed = np.sum(np.abs(t) * bound[j, rows]) + np.sum(np.abs(s) * bound[i, rows])
    print('%s: t^T M s = %.17g, s^T M t = %.17g, difference / bound %.3g' % (c['name'], float(a), float(b), float(abs(a - b) / allowed)))
    assert abs(a - b) <= allowed


@pytest.mark.parametrize('kind', ['ft', 'f'])
def test_result_of_a_slot_does_not_depend_on_the_launch(ctx, kind):
    """thin.h: "the result does not depend on the launch" - slot 11 at list position 0 and at position 20, under live counts 5 and 17, and with the
    identity list: the same bits"""
    base = case(kind, 100, (20, 4, 68), cols=SCRAMBLED_17_OF_40, nslots=40)
    g = thin_input(base)
    slot = 11
    assert slot in g['listed']
    others = [s for s in range(40) if s != slot]
    X = g['X'].copy()
    X[others] = np.where(X[others] == POISON, np.roll(X[g['listed'][0]], 1)[None, :], X[others])          # every slot readable: finite values everywhere
    rows = reference(base)[2][slot]
    results = {}
    for name, cols, live in (('position 0, live 17', [slot] + others[:20], 17), ('position 20', others[:20] + [slot], None), ('position 0, live 5', [slot] + others[:20], 5),
                             ('position 4, live 5', others[:4] + [slot] + others[4:20], 5), ('identity', None, None)):
        got, _ = ctx.test_thin(kind, g['T'], g['Tf'], g['ranks'], 4, X, g['Y0'], Tx=g['Tx'], F=g['F'], cols=cols, ncols=40 if cols is None else len(cols),
                               live=live, fill=POISON)
        assert not np.any(got[slot, rows] == POISON) and np.all(got[slot, ~rows] == POISON)
        results[name] = got[slot, rows].copy()
    first = results['position 0, live 17']
    ref = reference(base)
    assert worst_ratio(first, ref[0][slot, rows], ref[1][slot, rows], np.ones(first.shape, dtype=bool)) <= 1.0
    for name, r in results.items():
        assert np.array_equal(r.view(np.uint64), first.view(np.uint64)), name


REFUSALS = [
    # (what, expected refusal, kind, overrides of the geometry of a good case)
    ('T below 4', 'T', 'ft', dict(T=3)),
    ('rank no multiple of 4', 'rank', 'ft', dict(ranks=(20, 6, 68))),
    ('rank columns beyond the slab', 'rank', 'f', dict(ranks=(20, 4, 132))),
    ('Tx below T', 'Tx', 'ft', dict(Tx=96)),
    ('Tx % 4 with VEC4', 'Tx', 'f', dict(Tx=102)),
    ('ldx below the rows read', 'ld', 'ft', dict(ldx=296)),
    ('ldy below the rows written', 'ld', 'f', dict(ldy=296)),
    ('ldy below rtot', 'ld', 'ft', dict(ldy=88)),
    ('ld no multiple of 4', 'ld', 'ft', dict(ldx=302)),
    ('rpad above ld', 'rpad', 'ft', dict(ldy=124)),
    ('rpad above ld (input of F v)', 'rpad', 'f', dict(ldx=124)),
    ('rpad above ld (Sb u)', 'rpad', 's', dict(ldx=124)),
    ('list entry outside the slots', 'cols', 'ft', dict(cols=[0, 1, 5])),
    ('negative list entry', 'cols', 'f', dict(cols=[0, -1, 2])),
    ('slot listed twice', 'cols', 'ft', dict(cols=[0, 3, 1, 3])),
    ('more columns than slots', 'cols', 'ft', dict(ncols=6)),
    ('live count above ncols', 'live', 'ft', dict(cols=[0, 1, 2], live=4)),
    ('live count above ncols (identity)', 'live', 'f', dict(live=6)),
]


@pytest.mark.parametrize('what,refusal,kind,over', REFUSALS, ids=[r[0].replace(' ', '_') for r in REFUSALS])
def test_impossible_geometry_is_refused(ctx, what, refusal, kind, over):
    """refused by a return code of its own, before anything is allocated or launched"""
    from funs import _hip
    geo = dict(T=100, ranks=(20, 4, 68), Tx=100, ldx=300 if kind == 'ft' else 128, ldy=128 if kind in ('ft', 's') else 300, cols=None, ncols=None, live=None)
    geo.update(over)
    Tf = 104
    F = np.zeros((len(geo['ranks']), Tf, Tf))
    Sb = np.zeros((128, 128))
    X = np.ones((5, geo['ldx']))
    Y = np.full((5, geo['ldy']), POISON)
    with pytest.raises(_hip.HipBackendError) as e:
        ctx.test_thin(kind, geo['T'], Tf, geo['ranks'], 4, X, Y, Tx=geo['Tx'], F=F, Sb=Sb if kind == 's' else None, cols=geo['cols'], ncols=geo['ncols'], live=geo['live'], fill=POISON)
    print('%s: rc %d, "%s"' % (what, e.value.rc, e.value))
    assert e.value.refusal == refusal, (e.value.rc, str(e.value))
    assert e.value.rc == {v: k for k, v in ctx.THIN_REFUSALS.items()}[refusal]


TABLE_GEOMETRIES = [(T, ranks, gran) for T in (4, 100, 256, 257, 260, 700) for ranks in ((20,), (20, 4, 68), (132, 8, 60), (64, 80, 4), (200,), (128, 192, 196)) for gran in (4, 8, 16)]


def test_tables_partition_the_work(ctx):
    """the tables the hook used (returned by it), for the geometries of the cases above and a few larger ones - each from one launch on one column"""
    seen = set()
    for T, ranks, gran in TABLE_GEOMETRIES:
        _, _, _, _, rpad = geometry(ranks, gran)
        Tf = round_up(max(T, round_up(max(ranks), 16)), 4)
        ld = max(round_up(len(ranks) * T, 4), rpad)
        _, info = ctx.test_thin('ft', T, Tf, ranks, gran, np.ones((1, ld)), np.zeros((1, ld)), F=np.zeros((len(ranks), Tf, Tf)))
        rr, rk, roff, rtot = list(info['rr']), list(info['rk']), list(info['roff']), info['rtot']
        assert all(r % gran == 0 and r >= q for r, q in zip(rr, ranks)) and rk == [round_up(r, 16) for r in rr] and roff == list(np.concatenate([[0], np.cumsum(rr)]))
        for l in range(len(ranks)):
            grp = info['ft'][info['ft'][:, 0] == l]
            assert np.all(grp[:, 3] == roff[l])
            # the groups of a latent cover [0, rr) exactly once, in multiples of 4 up to 64 that differ by at most 4
            assert grp[0, 1] == 0 and np.all(grp[1:, 1] == grp[:-1, 1] + grp[:-1, 2]) and grp[-1, 1] + grp[-1, 2] == rr[l]
            assert np.all(grp[:, 2] % 4 == 0) and np.all(grp[:, 2] >= 4) and np.all(grp[:, 2] <= 64)
            assert np.max(grp[:, 2]) - np.min(grp[:, 2]) <= 4
            assert len(grp) == (rr[l] + 63) // 64
            seen.add(tuple(grp[:, 2]))
            fl = info['f'][info['f'][:, 0] == l]
            assert list(fl[:, 1]) == list(range(0, T, 256)) and np.all(fl[:, 2] == round_up(rr[l], 16)) and np.all(fl[:, 3] == roff[l])
        assert len(info['ft']) == sum((r + 63) // 64 for r in rr) and len(info['f']) == len(ranks) * ((T + 255) // 256)
        s = info['s']
        assert np.all(s[:, 0] == 0) and np.all(s[:, 3] == 0) and list(s[:, 1]) == list(range(0, rtot, 64)) and s[-1, 1] + s[-1, 2] == rtot and np.all(s[:-1, 2] == 64)
    assert (40, 40) in seen and (44, 44, 44) in seen and (48, 44, 44) in seen and (64,) in seen and (20,) in seen and (52, 48, 48, 48) in seen
