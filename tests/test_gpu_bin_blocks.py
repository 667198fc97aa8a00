"""The per-bin blocks of the low-rank engine (csrc/model.h: bin_blocks_reg_kernel<PW> up to 10 latents, bin_blocks_coop_kernel<PM> for 11..32):
G_t = (I + eps W_t)^-1, Wt_t = W_t G_t and log det(I + eps W_t), through the launch code of the engine (pgpfa_test_bin_blocks), against numpy.longdouble.

Reference: Cholesky, triangular inverse, L^-T L^-1, W G and the sum of the logs of the squared pivots, in longdouble, vectorised over the items.
Input: W = C^T diag(w) C (symmetric positive semi-definite) scaled so that eps ||W||_2 is 0.01, 1 or 30.
Bound: `mirror` is a float64 numpy restatement of the register kernel's algorithm in its order of operations; its error against the reference is
measured per case and quantity (the largest |.| over the matrices of the case, for G, Wt and ldet each), and the device must stay within 4 times that:
the factor covers fused multiply-adds, the device's log / sqrt / division and the other summation order of the cooperative form.
tests/test_cpu_bin_blocks.py shows without a GPU that this bound separates wrong kernels from the right one on exactly these inputs.

Poison 7.0: W of every slot that is not listed, behind every stride, the 128 elements behind W (the hook's `fill`), and all three outputs - what the
kernels do not store must come back as it went in: unlisted slots, the stride slack, and ldet is indexed by list position.
Every test prints what it measured."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

POISON = 7.0
LD = np.longdouble
EPS = 1e-3
SCALES = (0.01, 1.0, 30.0)
REG_MPB = 32                                            # matrices per workgroup of the register form


def coop_doubles(p):
    """bin_blocks_coop_doubles of model.h"""
    return 2 * p * (p | 1) + p * p


def per_block(p):
    """matrices per workgroup: 32 in the register form; in the cooperative form two per wave, as many waves as 64 KB of LDS hold, four at most"""
    if p <= 10:
        return REG_MPB
    return 2 * max(1, min(4, (64 * 1024) // (2 * coop_doubles(p) * 8)))


SCRAMBLED_3_OF_7 = (5, 0, 3)


def case(p, T, nslots=1, scale=1.0, slots=None, shared=False, want_ldet=True):
    name = 'p%d_T%d_n%d_s%g' % (p, T, nslots, scale)
    if slots is not None:
        name += '_list%dof%d' % (len(slots), nslots)
    if shared:
        name += '_shared'
    if not want_ldet:
        name += '_noldet'
    return dict(name=name, p=p, T=T, nslots=nslots, scale=scale, slots=tuple(range(nslots)) if slots is None else tuple(slots), shared=shared, want_ldet=want_ldet)


def _cases():
    out = []
    for i, p in enumerate((1, 2, 3, 5, 6, 7, 9, 10)):                                    # register form: 70 items = two full workgroups and 6
        out.append(case(p, 35, 2, SCALES[i % 3]))
    out += [case(5, 1, 1, 0.01), case(5, 31, 1, 30.0), case(5, 16, 2, 1.0), case(5, 11, 3, 0.01),          # 1, 31, 32, 33 items
            case(7, 33, 1, 30.0), case(9, 31, 1, 1.0), case(10, 11, 3, 0.01), case(2, 32, 1, 30.0)]          # the padded widths at the tails
    for i, p in enumerate((11, 16, 17, 20, 24, 25, 32)):                                 # cooperative form: an odd count, a partly filled last workgroup
        out.append(case(p, 2 * per_block(p) + 1, 1, SCALES[i % 3]))
    out += [case(11, 35, 2, 30.0), case(20, 8, 2, 0.01), case(32, 4, 1, 1.0), case(17, 3, 3, 30.0), case(25, 7, 2, 0.01)]
    out += [case(5, 11, 7, 1.0, slots=SCRAMBLED_3_OF_7), case(17, 5, 7, 1.0, slots=SCRAMBLED_3_OF_7)]
    out += [case(3, 33, 1, 1.0, shared=True), case(16, 9, 1, 30.0, shared=True)]
    out += [case(6, 33, 1, 30.0, want_ldet=False), case(24, 5, 1, 1.0, want_ldet=False)]
    return list({c['name']: c for c in out}.values())


CASES = _cases()
CASE_IDS = [c['name'] for c in CASES]

_inputs = {}


def blocks_input(c):
    """Inputs of a case, computed once and shared (callers must not write to them): W (nslots, sW) - (1, T p p) for the shared slot -, the strides as
    passed to the hook, the poisoned outputs G0 / Wt0, and Wl (list position, T, p, p): the matrices of the items in item order"""
    if c['name'] in _inputs:
        return _inputs[c['name']]
    p, T, nslots = c['p'], c['T'], c['nslots']
    rng = np.random.default_rng([p, T, nslots, int(c['scale'] * 100), len(c['slots']), int(c['shared'])])
    run = T * p * p
    sW, sO = (0, 0) if c['shared'] else (run + 3, run + 5)
    W = np.full((nslots, run + (0 if c['shared'] else 3)), POISON)
    Wl = np.empty((len(c['slots']), T, p, p))
    for i, s in enumerate(c['slots']):
        C = rng.standard_normal((T, 2 * p, p))
        w = rng.uniform(0.5, 1.5, size=(T, 2 * p))
        M = np.einsum('tqi,tq,tqj->tij', C, w, C)
        M = 0.5 * (M + np.transpose(M, (0, 2, 1)))
        M *= (c['scale'] / EPS / np.linalg.norm(M, 2, axis=(1, 2)))[:, None, None]
        Wl[i] = M
        W[s, :run] = M.reshape(-1)
    out0 = np.full((nslots, run + (0 if c['shared'] else 5)), POISON)
    _inputs[c['name']] = dict(p=p, T=T, run=run, sW=sW, sO=sO, W=W, Wl=Wl, G0=out0, Wt0=out0.copy(), pb=per_block(p), items=len(c['slots']) * T)
    return _inputs[c['name']]


# ---- the algorithm, vectorised over the items: W (n, p, p) -> G, Wt (n, p, p), ldet (n,) ---------------------------------------------------------------
FAULTS = ('eps_missing', 'uninverted_col', 'nonsym_g', 'log_pivot', 'tail_unstored')


def blocks(W, dtype, kernel_order, fault=None):
    """kernel_order: every sum in the order of bin_blocks_reg_kernel, log of the pivot before its root (the float64 mirror); otherwise the plain
    reference: products as matrix products, the logs of the squared pivots"""
    W = W.astype(dtype)
    n, p, _ = W.shape
    A = dtype(EPS) * W
    A[:, np.arange(p), np.arange(p)] += dtype(1.0)
    if fault == 'eps_missing':                          # eps left out of one entry
        A[:, 0, 0] = dtype(1.0) + W[:, 0, 0]
    L = np.zeros_like(A)
    ldet = np.zeros(n, dtype=dtype)
    for j in range(p):
        dj = A[:, j, j].copy()
        for m in range(j):
            dj = dj - L[:, j, m] * L[:, j, m]
        if kernel_order:
            ldet = ldet + np.log(dj)
        dj = np.sqrt(dj)
        L[:, j, j] = dj
        for i in range(j + 1, p):
            v = A[:, i, j].copy()
            for m in range(j):
                v = v - L[:, i, m] * L[:, j, m]
            L[:, i, j] = v / dj
    d = L[:, np.arange(p), np.arange(p)]
    if not kernel_order:
        ldet = np.sum(np.log(d if fault == 'log_pivot' else d * d), axis=1)
    Li = L.copy()                                       # inverted in place, column by column: column j reads entries that are still un-inverted
    for j in range(p):
        Li[:, j, j] = dtype(1.0) / Li[:, j, j]
        for i in range(j + 1, p):
            v = np.zeros(n, dtype=dtype)
            for m in range(j, i):
                v = v - Li[:, i, m] * Li[:, m, j]
            Li[:, i, j] = v / Li[:, i, i]
    if fault == 'uninverted_col':                       # G from the un-inverted factor in one column
        Li[:, :, 0] = L[:, :, 0]
    if kernel_order:
        G = np.zeros_like(A)
        for i in range(p):
            for j in range(i + 1):
                v = np.zeros(n, dtype=dtype)
                for m in range(i, p):
                    v = v + Li[:, m, i] * Li[:, m, j]
                G[:, i, j] = v
                G[:, j, i] = v
        Wt = np.zeros_like(A)
        for m in range(p):
            Wt = Wt + W[:, :, m, None] * G[:, m, None, :]
    else:
        G = np.einsum('nmi,nmj->nij', Li, Li)
        if fault == 'nonsym_g':                         # Wt = G W^T with a G that is not symmetric
            Gn = G.copy()
            Gn[:, 0, p - 1] *= 2
            Wt = np.einsum('nim,njm->nij', Gn, W)
        else:
            Wt = np.einsum('nim,nmj->nij', W, G)
    return G, Wt, ldet


def mirror(Wl):
    n = Wl.shape[0] * Wl.shape[1]
    return blocks(Wl.reshape(n, Wl.shape[2], Wl.shape[3]), np.float64, True)


def expected(c, fault=None):
    """(G, Wt, ldet) as the output buffers should come back, longdouble, POISON where nothing is stored; ldet (list positions, T)"""
    g = blocks_input(c)
    p, T, run = g['p'], g['T'], g['run']
    n = g['items']
    G, Wt, ldet = blocks(g['Wl'].reshape(n, p, p), LD, False, fault)
    G, Wt, ldet = G.copy(), Wt.copy(), ldet.copy()
    if fault == 'tail_unstored':                        # the last item of a partly filled workgroup not stored
        G[-1], Wt[-1], ldet[-1] = POISON, POISON, POISON
    Gb, Wb = np.full(g['G0'].shape, LD(POISON)), np.full(g['G0'].shape, LD(POISON))
    for i, s in enumerate(c['slots']):
        Gb[s, :run] = G[i * T:(i + 1) * T].reshape(-1)
        Wb[s, :run] = Wt[i * T:(i + 1) * T].reshape(-1)
    return Gb, Wb, ldet.reshape(len(c['slots']), T)


def mirror_buffers(c):
    g = blocks_input(c)
    p, T, run = g['p'], g['T'], g['run']
    G, Wt, ldet = mirror(g['Wl'])
    Gb, Wb = np.full(g['G0'].shape, POISON), np.full(g['G0'].shape, POISON)
    for i, s in enumerate(c['slots']):
        Gb[s, :run] = G[i * T:(i + 1) * T].reshape(-1)
        Wb[s, :run] = Wt[i * T:(i + 1) * T].reshape(-1)
    return Gb, Wb, ldet.reshape(len(c['slots']), T)


def errors(got, ref):
    """largest |got - ref| per quantity (G, Wt, ldet); ldet None: not requested"""
    return [float(np.max(np.abs(a.astype(LD) - b))) if a is not None else 0.0 for a, b in zip(got, ref)]


def ratios(err, err_mirror):
    """error / (4 x the mirror's error) per quantity; an error where the mirror has none: inf"""
    return [0.0 if e == 0.0 else (e / (4.0 * m) if m > 0.0 else np.inf) for e, m in zip(err, err_mirror)]


# ---- GPU --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def ctx():
    from funs import _hip
    c = _hip.Context(4, 2, 8, 1, 10.0)                  # (no parameters, no counts: the hook only borrows the stream)
    yield c
    c.close()


@pytest.mark.parametrize('c', CASES, ids=CASE_IDS)
def test_blocks_against_longdouble(ctx, c):
    g = blocks_input(c)
    p, T, run = g['p'], g['T'], g['run']
    G, Wt, ldet, pb = ctx.test_bin_blocks(p, T, EPS, g['W'], g['G0'], g['Wt0'], slots=c['slots'], sW=g['sW'], sO=g['sO'], want_ldet=c['want_ldet'], ldet_fill=POISON,
                                          fill=POISON)
    assert pb == g['pb']
    ref = expected(c)
    mir = mirror_buffers(c)
    if not c['want_ldet']:
        assert ldet is None
        ref, mir = ref[:2] + (None,), mir[:2] + (None,)
    em = errors(mir, [r if r is not None else None for r in ref])
    ed = errors((G, Wt, ldet), ref)
    rt = ratios(ed, em)
    print('%s: %d items, %d per workgroup; G device %.3g mirror %.3g, Wt device %.3g mirror %.3g, ldet device %.3g mirror %.3g; device / (4 mirror) %.3g %.3g %.3g'
          % (c['name'], g['items'], pb, ed[0], em[0], ed[1], em[1], ed[2], em[2], rt[0], rt[1], rt[2]))
    # what is not stored comes back as it went in: unlisted slots, the stride slack (the reference holds the poison there)
    stored = ref[0] != POISON
    assert np.all(G[~stored] == POISON) and np.all(Wt[~stored] == POISON)
    assert not np.any(G[stored] == POISON) and not np.any(Wt[stored] == POISON)
    if ldet is not None:
        assert not np.any(ldet == POISON)
    assert max(rt) <= 1.0, rt
    # symmetric to the bound: each of the two entries is within it of a symmetric reference
    for X, e in ((G, em[0]), (Wt, em[1])):
        for s in c['slots']:
            M = X[s, :run].reshape(T, p, p)
            assert float(np.max(np.abs(M - np.transpose(M, (0, 2, 1))))) <= 2 * 4 * e


REFUSALS = [
    ('p above 32', 'p', dict(p=33)),
    ('list entry outside the slots', 'list', dict(slots=(0, 3))),
    ('negative list entry', 'list', dict(slots=(-1,))),
    ('slot listed twice', 'list', dict(slots=(2, 0, 2))),
    ('sW below T p^2', 'stride', dict(sW=5 * 9 - 1)),
    ('sO below T p^2', 'stride', dict(sO=5 * 9 - 1)),
    ('shared input with three slots', 'stride', dict(sW=0)),
]


@pytest.mark.parametrize('what,refusal,over', REFUSALS, ids=[r[0].replace(' ', '_') for r in REFUSALS])
def test_impossible_geometry_is_refused(ctx, what, refusal, over):
    from funs import _hip
    geo = dict(p=3, T=5, slots=(0, 1, 2), sW=45, sO=45)
    geo.update(over)
    n = 5 * geo['p'] ** 2
    with pytest.raises(_hip.HipBackendError) as e:
        ctx.test_bin_blocks(geo['p'], geo['T'], EPS, np.zeros((3, n)), np.zeros((3, n)), np.zeros((3, n)), slots=geo['slots'], sW=geo['sW'], sO=geo['sO'])
    print('%s: rc %d, "%s"' % (what, e.value.rc, e.value))
    assert e.value.refusal == refusal, (e.value.rc, str(e.value))
    assert e.value.rc == {v: k for k, v in ctx.BINB_REFUSALS.items()}[refusal]
