"""The pivoted Cholesky of the RBF part (csrc/model.h: rbf_pivchol_kernel<256,1>, <512,2>, rbf_pivchol2_kernel<256,4>) through the three-way choice of the
engine (pgpfa_test_pivchol), checked for what ANY correct greedy pivoted Cholesky satisfies - pivots may differ from a reference's at near-ties (the
residual diagonal is symmetric about the middle of the trial), so no reference factor is compared.

All checks in numpy.longdouble, from the device's F and K~ = (1 - eps) RBF built by the kernel's own formula.  With u = 2^-53, r the returned rank,
A = |K~| + |F||F|^T, b = (r + 4) u max(A), p_j = argmax_t |F[t, j]| (a pivot entry is the largest of its column), R = K~ - F F^T:
 1. contract: rows >= T and columns >= r of every Tf x Tf slab are exactly 0, no prefill survives, r <= T
 2. pivot rows are exact to rounding: max_t |R[p_j, t]| <= b for every j - independent of tol; it sees one lost or doubled term of a step's dot product
 3. stopped neither early nor late: max diag(R) <= tol + b; unless r == T, the largest residual diagonal with the last column removed is > tol - b
 4. greedy: for every j, the residual diagonal from the columns < j at p_j is within 2 b of its maximum
 5. R is small everywhere: max |R| <= tol + b
tests/test_cpu_pivchol.py shows without a GPU that these checks separate wrong kernels from a float64 implementation of the algorithm on these cases.
Every test prints what it measured: each check as a fraction of what it allows."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

POISON = 7.0
U53 = 2.0 ** -53
LD = np.longdouble
BIN_MS = 10.0
EPS = 1e-3
TOLS = (1e-10, 1e-13)
NS = {'256_1': 1, '512_2': 2, 'pairs': 4}


def round_up(a, b):
    return (a + b - 1) // b * b


def launch(form, T, taus, tol, wide):
    """one launch: p = len(taus) latents.  wide: slabs of round_up(T, 64) rows as the engine has them, else the tightest the form takes"""
    pairs = form == 'pairs'
    Tf = round_up(T, 64) if wide else (T + T % 2 if pairs else T)
    return dict(name='%s_T%d_tau%s_tol%g_Tf%d' % (form, T, 'x'.join('%g' % t for t in taus), tol, Tf), form=form, T=T, Tf=Tf, taus=tuple(taus), tol=tol, pairs=pairs)


# timescales per bin count, sized so that r T^2 <= 5e7 (the longdouble products have no BLAS); tau = 0.003 s: full rank, every start a tie
FORM_CASES = {
    '256_1': [(1, (0.07,)), (5, (0.02,)), (64, (0.02,)), (100, (0.1,)), (130, (0.003,)), (255, (0.6, 0.07, 0.02)), (256, (0.07, 0.02))],
    '512_2': [(257, (0.6, 0.07, 0.02)), (257, (0.003,)), (512, (0.6, 0.1)), (513, (0.6, 0.1)), (700, (0.6, 0.2))],
    'pairs': [(257, (0.6, 0.07, 0.02)), (301, (0.6, 0.07, 0.003)), (258, (0.07,)), (511, (0.1,)), (512, (0.6, 0.1)), (513, (0.6, 0.1)), (700, (0.6, 0.2)),
              (1025, (1.0,))],
}
LAUNCHES = [launch(form, T, taus, tol, wide=(tol == TOLS[0])) for form in ('256_1', '512_2', 'pairs') for T, taus in FORM_CASES[form] for tol in TOLS]
LAUNCH_IDS = [c['name'] for c in LAUNCHES]


def kernel_matrix(T, tau, dtype=LD):
    """K~ = (1 - eps) exp(-0.5 dt^2 / den) by the kernel's own formula: dt and den formed in float64 as the kernel forms them"""
    t = np.arange(T, dtype=np.float64) * BIN_MS
    dt = t[:, None] - t[None, :]
    den = (tau * 1000.0) * (tau * 1000.0)
    return dtype(1.0 - EPS) * np.exp(dtype(-0.5) * ((dt * dt) / den).astype(dtype))


def check_factor(slab, r, T, tau, tol, fill=POISON, dtype=LD):
    """slab (Tf, Tf) [column, bin], rank r.  Returns dict: b, and every check as the fraction of what it allows (<= 1 passes; inf: contract broken)."""
    out = dict(b=0.0, contract=0.0, pivot_rows=0.0, stop_late=0.0, stop_early=0.0, greedy=0.0, residual=0.0)
    if not (0 <= r <= T) or np.any(slab[r:, :] != 0.0) or np.any(slab[:, T:] != 0.0) or np.any(slab == fill):
        out['contract'] = np.inf
        return out
    F = slab[:r, :T].T.astype(dtype)                    # (T, r)
    K = kernel_matrix(T, tau, dtype)
    A = np.abs(K).astype(np.float64) + np.abs(slab[:r, :T].T) @ np.abs(slab[:r, :T])
    b = (r + 4) * U53 * float(np.max(A))
    out['b'] = b
    R = K - F @ F.T
    dR = np.diagonal(R)
    out['residual'] = float((np.max(np.abs(R)) - tol) / b)
    out['stop_late'] = float((np.max(dR) - tol) / b)
    if r > 0:
        piv = np.argmax(np.abs(F), axis=0)
        out['pivot_rows'] = float(np.max(np.abs(R[piv, :])) / b)
        if r < T:                                       # with the last column removed something above tol must have been left
            out['stop_early'] = float((tol - np.max(dR + F[:, -1] ** 2)) / b)
        # residual diagonal before column j: diag(K~) - sum_{m < j} F[:, m]^2
        D = np.diagonal(K)[:, None] - np.concatenate([np.zeros((T, 1), dtype=dtype), np.cumsum(F[:, :-1] ** 2, axis=1)], axis=1)
        out['greedy'] = float(np.max(np.max(D, axis=0) - D[piv, np.arange(r)]) / (2 * b))
    elif T > 0:
        out['stop_early'] = float((tol - np.max(dR)) / b)
    return out


CHECKS = ('contract', 'pivot_rows', 'stop_late', 'stop_early', 'greedy', 'residual')


def worst(res):
    return max(res[k] for k in CHECKS)


# ---- GPU --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def ctx():
    from funs import _hip
    c = _hip.Context(4, 2, 8, 1, 10.0)                  # (no parameters, no counts: the hook only borrows the stream)
    yield c
    c.close()


_ranks = {}


@pytest.mark.parametrize('c', LAUNCHES, ids=LAUNCH_IDS)
def test_factor_is_a_greedy_pivoted_cholesky(ctx, c):
    F, ranks, form = ctx.test_pivchol(c['T'], c['Tf'], c['taus'], BIN_MS, EPS, c['tol'], pairs=c['pairs'], fill=POISON)
    assert form == c['form']
    _ranks[c['name']] = [int(r) for r in ranks]
    for k, tau in enumerate(c['taus']):
        r = int(ranks[k])
        assert r * c['T'] ** 2 <= 5e7, 'the case is too large for its longdouble products'
        res = check_factor(F[k], r, c['T'], tau, c['tol'])
        print('%s latent %d: rank %d, b %.3g, %s' % (c['name'], k, r, res['b'], ', '.join('%s %.3g' % (n, res[n]) for n in CHECKS)))
        assert 1 <= r <= c['T']
        for n in CHECKS:
            assert res[n] <= 1.0, (n, res[n])
        if tau == 0.003:
            assert r == c['T']                          # full rank: the loop ends on rmax


def test_ranks_cross_the_block_sizes_and_the_two_long_forms_agree(ctx):
    """every form meets ranks beyond 8 and 64 and beyond a multiple of 8 NS plus a partly filled block (every column count below the rank is a step);
    one full-rank case per form; the two forms beyond 256 bins return equal ranks wherever both ran"""
    for c in LAUNCHES:
        if c['name'] not in _ranks:
            _, ranks, _ = ctx.test_pivchol(c['T'], c['Tf'], c['taus'], BIN_MS, EPS, c['tol'], pairs=c['pairs'], fill=POISON)
            _ranks[c['name']] = [int(r) for r in ranks]
    for form in NS:
        mine = [(c, _ranks[c['name']]) for c in LAUNCHES if c['form'] == form]
        top = max(max(r) for _, r in mine)
        print('%s: largest rank %d' % (form, top))
        assert top > 64 + 8 * NS[form] + 1
        assert any(r == c['T'] and c['T'] > 8 for c, rs in mine for r in rs)
        assert any(1 < r <= 8 for _, rs in mine for r in rs) or form != '256_1'
    shared = 0
    for a in LAUNCHES:
        for b in LAUNCHES:
            if a['form'] == '512_2' and b['form'] == 'pairs' and (a['T'], a['taus'], a['tol']) == (b['T'], b['taus'], b['tol']):
                assert _ranks[a['name']] == _ranks[b['name']], (a['name'], _ranks[a['name']], _ranks[b['name']])
                shared += 1
    assert shared >= 8


REFUSALS = [
    ('Tf below T', 'Tf', dict(Tf=299)),
    ('odd Tf with pairs', 'odd', dict(Tf=301)),
    ('T below 1', 'T', dict(T=0)),
    ('LDS above a launch', 'lds', dict(T=2800, Tf=2816, pairs=False)),
    ('LDS above a launch (pairs)', 'lds', dict(T=1700, Tf=1700)),
    ('timescale 0', 'bad_arg', dict(taus=(0.1, 0.0))),
]


@pytest.mark.parametrize('what,refusal,over', REFUSALS, ids=[r[0].replace(' ', '_').replace('(', '').replace(')', '') for r in REFUSALS])
def test_impossible_geometry_is_refused(ctx, what, refusal, over):
    from funs import _hip
    geo = dict(T=300, Tf=320, taus=(0.1,), pairs=True)
    geo.update(over)
    with pytest.raises(_hip.HipBackendError) as e:
        ctx.test_pivchol(geo['T'], geo['Tf'], geo['taus'], BIN_MS, EPS, 1e-10, pairs=geo['pairs'], fill=POISON)
    print('%s: rc %d, "%s"' % (what, e.value.rc, e.value))
    assert e.value.refusal == refusal, (e.value.rc, str(e.value))
    assert e.value.rc == {v: k for k, v in ctx.PIVCHOL_REFUSALS.items()}[refusal]
