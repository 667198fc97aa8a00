"""The dual-variational evaluation term by term against numpy.longdouble: csrc/dual.h (the GEMM form: dual_table_kernel, dual_pre_kernel, the two
products against the pair / loading table, dual_unpack_w_kernel, dual_pack_sigma_kernel, dual_jitter_kernel, dual_grad_finish_kernel, and under option
dual_masked dual_jitter_len_kernel, trunc_prior_kernel, dual_live_mask_kernel), the host flow of csrc/dual.hip (dual_common, dual_gradient,
dual_eval_slots) and the vector forms of model.h (dual_prep_kernel, dual_grad_kernel, dual_grad_batch_kernel), through the public entry points only:
dual_post_mean (= -K v), dual_post_cov(prec) (= K^-1 + scatter(W_t): every entry of W_t), dual_costgrad(_batch), and post_vsm, which hands back the
Sigma_t blocks the gradient was formed from.

Reference (`reference`): lmy = lambda - y, V = C^T lmy, K V (K from orc.make_K), sB = sum d_n lmy, sD = sum lambda (log lambda - 1), 1/2 v^T K v,
W_t = C^T diag(lambda_t) C and C_big^T K v in longdouble, each with its unsigned size - the same sum over the absolute values of its terms.  The jittered
precision, its inverse and the log-determinant come from FP64 numpy (orc.vi_post_cov, slogdet as orc.dual_cost takes it).

Bounds, u = 2^-53, each 1.01 N u (unsigned size) - they hold for any order of summation:
  A  post_mean            N = q + T + 4            size |K| (|C|^T |lmy|)
  B  prec, same bin       N = q + 3                size sum_n |c_na c_nb| lambda; the diagonal adds one rounding of the sum with the device's own K^-1
     prec, elsewhere      the bits of gram_inverse within a latent, exactly 0 across latents; prec exactly symmetric; cov 1e-8 rel of orc.vi_post_cov
  C  cost                 N = q + T + 8            size of 1/2 vKv, sB, sD, plus tau_logdet / 2 (below)
  D  gradient, per entry  1.01 u [(q + T + p + 6) |C|^T |K| |V| + (p^2 + 4) 1/2 sum |c| |Sigma^dev| |c| + 2 |log lambda| + |d|] against
                          g_ref = C_big^T K v - d + log lambda - 1/2 c_n^T Sigma_t^dev c_n in longdouble, Sigma^dev = post_vsm after the call, itself tied
                          to dense numpy at 1e-8 relative (the engines' own criterion)
An entry whose terms are all exact zeros (the zero row and the zero column of C) has bound 0 and must come back exact.

tau_logdet.  Dense engine: LOGDET_MULT = 8 times FP64 numpy's own error in that log-determinant, which tests/test_cpu_dual_dense.py measures against a
longdouble evaluation (Gram inverses, precision, Cholesky factor, all in longdouble) at the cases with n = p T <= 400.  That error does not grow with n:
it comes from inverting the Gram matrices (condition 1e4 .. 1e6) and sits at 0.6 .. 51 u |logdet| from n = 3 to n = 640, so the model is
NP_LOGDET_RHO u |logdet| with NP_LOGDET_RHO = 64, asserted there.  Low-rank engine: 1e-9 |logdet| (low-rank against dense).

Forms: every case runs in the GEMM form and with dual_gemm = 0 (the vector kernels); every case with one trial also through single-trial dual_costgrad
(dense engine, dual_grad_kernel); the cases marked `lowrank` also under cov_mode 2 / dual_lowrank 1 (plan_lowrank asserted) with section D unchanged.
tests/test_cpu_dual_dense.py shows without a GPU that `mirror` - a float64 numpy restatement of the GEMM form - meets every bound on exactly these inputs
and that ten single faults miss them by a factor of 1000 or more.  Every test prints what it measured."""
import numpy as np
import pytest

from oracle import pgpfa_oracle as orc

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = 2.0 ** -53
BIN_MS = 10.0
JIT = 1e-6
LOGDET_MULT = 8.0           # the dense engine's log-determinant may miss FP64 numpy's by this many times numpy's own error (blocked factor, other order)
NP_LOGDET_RHO = 64.0        # FP64 numpy's log-determinant is within NP_LOGDET_RHO u |logdet| of the longdouble one: measured in test_cpu_dual_dense.py (largest 51)
TOL_SIGMA = 1e-8            # covariance blocks against dense numpy, relative to the largest entry
TOL_LOGDET_LOWRANK = 1e-9   # low-rank engine against dense
TOL_COST_MASKED = 1e-8      # the dual cost under a length table (tests/test_gpu_variational_missing.py)


def round_up(a, b):
    return (a + b - 1) // b * b


def unpack_tile_bins(p):
    """dual_tile_bins(np) of dual.h: bins per LDS tile of dual_unpack_w_kernel"""
    n, per = 32, p * (p + 1) // 2
    while n > 1 and per * (n + 1) * 8 > 60000:
        n >>= 1
    return n


def pack_tile_bins(p):
    """bins per LDS tile of dual_pack_sigma_kernel (dual_gradient)"""
    n = 32
    while n > 1 and n * (p * p + 1) * 8 > 60000:
        n >>= 1
    return n


# ---- cases: the smallest shapes on each seam ------------------------------------------------------------------------------------------------------------
def case(name, q, p, T, R=1, idx=None, hi=False, lowrank=False, why=''):
    return dict(name=name, q=q, p=p, T=T, R=R, idx=tuple(range(R)) if idx is None else tuple(idx), hi=hi, lowrank=lowrank, why=why)


def _cases():
    out = []
    why_T = {1: 'one bin: a single lane of dual_pre_kernel, K = [1]',
             33: 'one bin into the second 32-bin tile of both transposes',
             63: 'dual_pre_kernel: one lane short of its 64-bin tile', 64: 'dual_pre_kernel: exactly one 64-bin tile, no tail anywhere',
             65: 'dual_pre_kernel: a second tile of one bin (two partial sums per slot)',
             127: 'general GEMM, M = T: one row short of its 128-row tile', 128: 'general GEMM: exactly one 128-row tile',
             129: 'general GEMM: a second 128-row block of one row', 200: 'four 64-bin tiles, two 128-row blocks, seven 32-bin transpose tiles'}
    for T in (1, 33, 63, 64, 65, 127, 128, 129, 200):
        out.append(case('T%d' % T, 21, 3, T, lowrank=T >= 127, why=why_T[T]))
    why_q = {3: 'fewer neurons than waves in the 4-wave interleave; qpad - q = 13 rows of the next slot under zero table rows',
             15: 'q = qpad - 1: one row of the next slot in the Lambda^T operand', 16: 'q = qpad: the operand ends at the slot',
             17: 'qpad = 32: 15 rows of the next slot', 50: 'wave 3 of the interleave ends one neuron early (n = 47)',
             130: 'two 128-row blocks of the table: N = q of the gradient products crosses 128'}
    for q in (3, 15, 16, 17, 50, 130):                   # two trials: the operand of slot 0 runs into slot 1
        out.append(case('q%d' % q, q, 3, 70, R=2, lowrank=q in (17, 130), why=why_q[q]))
    why_p = {1: 'one pair, npd = 16: fifteen zero columns of Sp', 2: 'three pairs; the weights 1, 2, 1',
             5: '15 pairs: N one short of 16', 15: 'dual_pack_sigma_kernel: the last width with 32-bin tiles; 120 pairs',
             16: 'pack tile 32 -> 16 bins; K = round_up(p, 16) = p columns of KD', 20: 'dual_unpack_w_kernel: the last width with 32-bin tiles',
             21: 'unpack tile 32 -> 16 bins; the last width with 16-bin pack tiles', 22: 'pack tile 16 -> 8 bins',
             30: 'unpack tile 16 -> 8 bins; the last width with 8-bin pack tiles', 31: 'pack tile 8 -> 4 bins; 496 pairs, a multiple of 16',
             32: '528 pairs, a multiple of 16; K = 32 columns of KD'}
    for p in (1, 2, 5, 15, 16, 20, 21, 22, 30, 31, 32):
        out.append(case('p%d' % p, 37, p, 40, lowrank=p in (5, 16, 21, 32), why=why_p[p]))
    out.append(case('slots3', 21, 3, 70, R=3, why='three slots in one launch'))
    out.append(case('list3of5', 21, 3, 70, R=5, idx=(4, 0, 2), why='3 of 5 trials out of order: trial_of_slot is no identity'))
    out.append(case('hi', 21, 3, 65, R=2, hi=True, why='counts above 255: the second count plane'))
    return out


CASES = _cases()
CASE_IDS = [c['name'] for c in CASES]
LOWRANK_CASES = [c for c in CASES if c['lowrank']]
MASKED_T, MASKED_LENS = 130, (1, 63, 64, 65, 130)

_inputs, _refs = {}, {}


def make_inputs(q, p, T, R, hi=False, tag=0):
    """C with one all-zero row (and, from three latents on, one all-zero column), d of both signs, timescales spread over 0.03 .. 0.6 s, lambda log-uniform
    over 1e-4 .. 1e2 and Poisson counts at those rates, so that lambda - y cancels"""
    rng = np.random.default_rng([q, p, T, R, int(hi), tag])
    C = 0.35 * rng.standard_normal((q, p)) / np.sqrt(p)
    C[q // 2] = 0.0
    if p >= 3:
        C[:, p // 2] = 0.0
    d = rng.uniform(-1.5, 1.0, q)
    d[0], d[-1] = -0.7, 0.4
    tau = rng.permutation(np.geomspace(0.03, 0.6, p)) if p > 1 else np.array([0.13])
    lam = 10.0 ** rng.uniform(-4.0, 2.0, (R, q, T))
    Y = np.minimum(rng.poisson(lam), 255).astype(np.uint16)
    if hi:
        flat = rng.choice(R * q * T, 40, replace=False)
        big = rng.integers(256, 1500, 40)
        Y.reshape(-1)[flat] = big
        lam.reshape(-1)[flat] = big * (1.0 + 1e-3 * rng.standard_normal(40))
    return dict(q=q, p=p, T=T, R=R, C=C, d=d, tau=tau, lam=lam, Y=Y)


def inputs(c):
    """the inputs of a case, computed once; callers must not write to them"""
    if c['name'] not in _inputs:
        _inputs[c['name']] = make_inputs(c['q'], c['p'], c['T'], c['R'], c['hi'])
    return _inputs[c['name']]


# ---- the longdouble reference ---------------------------------------------------------------------------------------------------------------------------
def blocks_of(S, p, T):
    """Sigma_t[k][l] = S[(k, t), (l, t)] of a latent-major (p T) x (p T) matrix -> (T, p, p)"""
    return np.ascontiguousarray(np.einsum('ktlt->tkl', S.reshape(p, T, p, T)))


def reference_of(C, d, tau, lam, y):
    """every term of the dual evaluation of one trial (lam, y: (q, T)) and its unsigned size in longdouble; the jittered precision's inverse and
    log-determinant in FP64 numpy"""
    q, p = C.shape
    T = lam.shape[1]
    Cl, dl, ll, yl = C.astype(LD), d.astype(LD), lam.astype(LD), y.astype(LD)
    K = orc.make_K(tau, T, BIN_MS)
    Kl = K.astype(LD)
    lmy = ll - yl
    V, aV = Cl.T @ lmy, np.abs(Cl).T @ np.abs(lmy)                                   # (p, T)
    KV = np.einsum('kts,ks->kt', Kl, V)
    aKV = np.einsum('kts,ks->kt', np.abs(Kl), aV)
    logl = np.log(ll)
    W = np.einsum('na,nb,nt->tab', Cl, Cl, ll)
    aW = np.einsum('na,nb,nt->tab', np.abs(Cl), np.abs(Cl), ll)
    r = dict(q=q, p=p, T=T, C=Cl, d=dl, lam=ll, logl=logl, K=K, lmy=lmy, V=V, aV=aV, KV=KV, aKV=aKV, W=W, aW=aW,
             sB=np.sum(dl[:, None] * lmy), asB=np.sum(np.abs(dl)[:, None] * np.abs(lmy)),
             sD=np.sum(ll * (logl - 1)), asD=np.sum(np.abs(ll * (logl - 1))),
             hvKv=np.sum(V * KV) / 2, ahvKv=np.sum(aV * aKV) / 2, CKV=Cl @ KV, aCKV=np.abs(Cl) @ aKV)
    Kinv = np.stack([np.linalg.inv(k) for k in K])
    C_big, _ = orc.make_Cd_big(C, d, T)
    S, P = orc.vi_post_cov(orc.make_K_big(Kinv), C_big, lam.reshape(-1))
    sign, ld = np.linalg.slogdet(S)                                                  # (as orc.dual_cost takes it: + ld / 2)
    assert sign == 1.0
    r.update(S=S, Sig=blocks_of(S, p, T), logdet=-ld, n=p * T)
    r['cost_head'] = r['hvKv'] - r['sB'] + r['sD']
    r['cost'] = r['cost_head'] - LD(r['logdet']) / 2
    r['acost'] = r['ahvKv'] + r['asB'] + r['asD']
    return r


def reference(c, trial):
    key = (c['name'], trial)
    if key not in _refs:
        g = inputs(c)
        _refs[key] = reference_of(g['C'], g['d'], g['tau'], g['lam'][trial], g['Y'][trial])
    return _refs[key]


def tau_logdet(ref, lowrank=False):
    """what the log-determinant may miss FP64 numpy's by (see the module's docstring)"""
    if lowrank:
        return TOL_LOGDET_LOWRANK * abs(ref['logdet'])
    return LOGDET_MULT * NP_LOGDET_RHO * U * abs(ref['logdet'])


def worst(err, bound):
    """largest err / bound; an entry with bound 0 must be exact (inf otherwise)"""
    err, bound = np.asarray(err, dtype=LD), np.asarray(bound, dtype=LD)
    zero = bound == 0
    if np.any(err[zero] != 0) or not np.all(np.isfinite(err.astype(np.float64))):
        return np.inf
    if np.all(zero):
        return 0.0
    return float(np.max(err[~zero] / bound[~zero]))


def ratio_a(ref, post_mean):
    q, p, T = ref['q'], ref['p'], ref['T']
    got = np.asarray(post_mean, dtype=LD).reshape(p, T)
    return worst(np.abs(got + ref['KV']), 1.01 * (q + T + 4) * U * ref['aKV'])


def ratio_b_w(ref, W):
    """W (T, p, p) against C^T diag(lambda_t) C"""
    return worst(np.abs(np.asarray(W, dtype=LD) - ref['W']), 1.01 * (ref['q'] + 3) * U * ref['aW'])


def bound_c(ref, lowrank=False):
    return float(1.01 * (ref['q'] + ref['T'] + 8) * U * ref['acost']) + 0.5 * tau_logdet(ref, lowrank)


def ratio_c(ref, cost, lowrank=False):
    r = float(abs(LD(cost) - ref['cost'])) / bound_c(ref, lowrank)
    return r if np.isfinite(r) else np.inf


def var_term(ref, Sig):
    """1/2 c_n^T Sigma_t c_n and its unsigned size, (q, T), from blocks Sig (T, p, p)"""
    Sl = np.asarray(Sig, dtype=LD)
    return np.einsum('na,tab,nb->nt', ref['C'], Sl, ref['C']) / 2, np.einsum('na,tab,nb->nt', np.abs(ref['C']), np.abs(Sl), np.abs(ref['C'])) / 2


def bound_d(ref, Sig):
    q, p, T = ref['q'], ref['p'], ref['T']
    _, av = var_term(ref, Sig)
    return 1.01 * U * ((q + T + p + 6) * ref['aCKV'] + (p * p + 4) * av + 2 * np.abs(ref['logl']) + np.abs(ref['d'])[:, None])


def ratio_d(ref, grad, Sig, rows=None):
    """the gradient against the longdouble gradient formed with the blocks Sig it was formed from (rows: only these neurons)"""
    v, _ = var_term(ref, Sig)
    g_ref = ref['CKV'] - ref['d'][:, None] + ref['logl'] - v
    err, bound = np.abs(np.asarray(grad, dtype=LD).reshape(ref['q'], ref['T']) - g_ref), bound_d(ref, Sig)
    return worst(err, bound) if rows is None else worst(err[rows], bound[rows])


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


# ---- the GEMM form in float64 numpy, and the same with one fault ------------------------------------------------------------------------------------------
FAULTS = ('pair_shift', 'weight_one', 'lost_neuron', 'sd_tail', 'unpack_tail', 'pack_tail', 'no_jitter', 'alpha_plus', 'hi_ignored', 'finish_twice')
_posteriors = {}


def fault_defined(c, fault):
    q, p, T = c['q'], c['p'], c['T']
    return {'pair_shift': p >= 2, 'weight_one': p >= 2, 'lost_neuron': q >= 4, 'sd_tail': T % 64 != 0, 'unpack_tail': T % unpack_tile_bins(p) != 0,
            'pack_tail': T % pack_tile_bins(p) != 0, 'hi_ignored': c['hi']}.get(fault, True)


def mirror(c, trial, fault=None):
    """The GEMM form of dual_common / dual_eval_slots / dual_gradient for one trial in float64 numpy: the pair / loading table with its npd padding and
    zero rows up to qpad, pair order a (a + 1) / 2 + b, Lambda^T read with K = qpad (the rows behind q hold the next slot's finite values), partial sums
    per 64-bin tile, the jitter on the diagonal, Sp with the weights 1 and 2, alpha = -1/2, KD with K = round_up(p, 16) columns, log lambda - d at the end.
    fault: one of FAULTS - what a wrong kernel would do."""
    g = inputs(c)
    q, p, T, C, d = g['q'], g['p'], g['T'], g['C'], g['d']
    lam, Yc = g['lam'][trial], g['Y'][trial]
    qpad, npair, p16 = round_up(q, 16), p * (p + 1) // 2, round_up(p, 16)
    npd = round_up(npair, 16)
    ia, ib = np.tril_indices(p)                                                      # pair c = a (a + 1) / 2 + b, a >= b
    tbl = np.zeros((qpad, npd + p16))
    tbl[:q, :npair] = C[:, ia] * C[:, ib]
    tbl[:q, npd:npd + p] = C
    y = (Yc & 255).astype(np.float64) + (0.0 if fault == 'hi_ignored' else 256.0 * (Yc >> 8))
    lmy = lam - y
    term_d = lam * (np.log(lam) - 1.0)
    term_b = d[:, None] * lmy
    if fault == 'lost_neuron':                           # the last neuron of wave 3 never visited: its lmy stays what the buffer held, its terms are not summed
        n3 = max(n for n in range(q) if n % 4 == 3)
        lmy, term_d, term_b = lmy.copy(), term_d.copy(), term_b.copy()
        lmy[n3] = term_d[n3] = term_b[n3] = 0.0
    sB = sD = 0.0
    for t0 in range(0, T, 64):
        sB += term_b[:, t0:t0 + 64].sum()
        if not (fault == 'sd_tail' and t0 == 64 * (T // 64)):
            sD += term_d[:, t0:t0 + 64].sum()
    next_slot = np.full((qpad - q, T), 3.0)
    Wp = np.vstack([lam, next_slot]).T @ tbl[:, :npair]                              # (T, pairs)
    V = (np.vstack([lmy, -next_slot]).T @ tbl[:, npd:npd + p]).T                     # (p, T)
    shift = (lambda i: np.minimum(i + 1, npair - 1)) if fault == 'pair_shift' else (lambda i: i)
    a, b = np.meshgrid(np.arange(p), np.arange(p), indexing='ij')
    hi_, lo_ = np.maximum(a, b), np.minimum(a, b)
    W = Wp[:, shift(hi_ * (hi_ + 1) // 2 + lo_)]                                     # dual_unpack_w_kernel
    if fault == 'unpack_tail':
        W[unpack_tile_bins(p) * (T // unpack_tile_bins(p)):] = 0.0
    K = orc.make_K(g['tau'], T, BIN_MS)
    KV = np.einsum('kts,ks->kt', K, V)
    vKv = float(np.sum(V * KV))
    key = (c['name'], trial, fault if fault in ('pair_shift', 'unpack_tail', 'no_jitter') else None)
    if key not in _posteriors:
        # (symmetric Gram inverses, as the device's L^-T L^-1 are: a Cholesky factor reads one triangle only, and the two triangles of numpy's inverse
        #  differ by cond(K) u |K^-1| - worth 7e-9 of the log-determinant at T = 63, a thousand times the error of either evaluation)
        P = orc.make_K_big(np.stack([0.5 * (ki + ki.T) for ki in (np.linalg.inv(k) for k in K)]))
        for k in range(p):
            for l in range(p):
                P[k * T + np.arange(T), l * T + np.arange(T)] += W[:, k, l]
        if fault != 'no_jitter':
            P[np.arange(p * T), np.arange(p * T)] *= 1.0 + JIT
        try:
            Lc = np.linalg.cholesky(P)
            _posteriors[key] = (2.0 * np.sum(np.log(np.diag(Lc))), blocks_of(np.linalg.inv(P), p, T))
        except np.linalg.LinAlgError:                    # (a fault can cost the precision its definiteness: the device call would fail, the ratios are inf)
            _posteriors[key] = (np.nan, np.full((T, p, p), np.nan))
    logdet, Sig = _posteriors[key]
    cost = 0.5 * vKv - sB - 0.5 * logdet + sD
    w = np.ones(npair) if fault == 'weight_one' else np.where(ia == ib, 1.0, 2.0)
    Sp = np.zeros((T, npd))
    Sp[:, :npair] = Sig[:, ia[shift(np.arange(npair))], ib[shift(np.arange(npair))]] * w   # dual_pack_sigma_kernel
    if fault == 'pack_tail':
        Sp[pack_tile_bins(p) * (T // pack_tile_bins(p)):] = 0.0
    G = (0.5 if fault == 'alpha_plus' else -0.5) * (Sp @ tbl[:, :npd].T)             # (T, qpad)
    KD = np.zeros((T, p16))
    KD[:, :p] = KV.T
    G += KD @ tbl[:, npd:npd + p16].T
    grad = G[:, :q].T + (2.0 if fault == 'finish_twice' else 1.0) * (np.log(lam) - d[:, None])
    return dict(post_mean=-KV.reshape(-1), W=W, cost=cost, grad=grad, Sig=Sig, logdet=logdet)


def ratios_of(ref, out, lowrank=False):
    """sections A, B (W), C, D of one evaluation (device or mirror)"""
    return dict(A=ratio_a(ref, out['post_mean']), B=ratio_b_w(ref, out['W']), C=ratio_c(ref, out['cost'], lowrank), D=ratio_d(ref, out['grad'], out['Sig']))


# ---- the device -----------------------------------------------------------------------------------------------------------------------------------------
def open_context(g, lowrank=False, gemm=True):
    from funs import _hip
    ctx = _hip.Context(g['q'], g['p'], g['T'], g['R'], BIN_MS)
    try:
        ctx.upload_counts(g['Y'] if g['Y'].max() > 255 else g['Y'].astype(np.uint8))
        ctx.set_option('cov_mode', 2 if lowrank else 1)
        ctx.set_option('dual_lowrank', int(lowrank))
        ctx.set_option('dual_gemm', int(gemm))
        ctx.set_params(g['C'], g['d'], g['tau'])
    except Exception:
        ctx.close()
        raise
    return ctx


@pytest.mark.parametrize('c', CASES, ids=CASE_IDS)
def test_sections_a_b_post_mean_and_every_entry_of_the_precision(c):
    g = inputs(c)
    q, p, T = g['q'], g['p'], g['T']
    trial = c['idx'][0]
    ref = reference(c, trial)
    lam = g['lam'][trial]
    ctx = open_context(g)
    try:
        Kinv = ctx.gram_inverse()
        line = []
        for gemm in (1, 0):
            ctx.set_option('dual_gemm', gemm)
            ra = ratio_a(ref, ctx.dual_post_mean(trial, lam))
            cov, prec = ctx.dual_post_cov(trial, lam)
            P4 = prec.reshape(p, T, p, T)
            W = blocks_of(prec, p, T)                                                # same bin: W_t, on its diagonal plus (K_k^-1)_tt
            kd = np.stack([np.diag(Kinv[k]) for k in range(p)], axis=1)              # (T, p)
            off = ~np.eye(p, dtype=bool)
            rb = worst(np.abs(W.astype(LD) - ref['W'])[:, off], (1.01 * (q + 3) * U * ref['aW'])[:, off]) if p > 1 else 0.0
            dg = np.arange(p)
            want = kd.astype(LD) + ref['W'][:, dg, dg]
            rdiag = worst(np.abs(W[:, dg, dg].astype(LD) - want), 1.01 * (q + 3) * U * ref['aW'][:, dg, dg] + U * np.abs(want))
            same_latent = all(np.array_equal(P4[k, :, k, :][~np.eye(T, dtype=bool)], Kinv[k][~np.eye(T, dtype=bool)]) for k in range(p))
            across = P4.copy()
            across[np.arange(p), :, np.arange(p), :] = 0.0                           # what is left: different latents ...
            t = np.arange(T)
            across[:, t, :, t] = 0.0                                                 # ... at different bins
            e_cov = rel(cov, ref['S'])
            line.append('%s form: A %.3g, B off-diagonal %.3g, diagonal %.3g, cov %.2e' % ('GEMM' if gemm else 'vector', ra, rb, rdiag, e_cov))
            assert ra <= 1.0 and rb <= 1.0 and rdiag <= 1.0, line[-1]
            assert same_latent and not np.any(across) and np.array_equal(prec, prec.T)
            assert e_cov <= TOL_SIGMA, line[-1]
        print('%s (%s): %s' % (c['name'], c['why'], '; '.join(line)))
    finally:
        ctx.close()


def evaluate(ctx, g, idx, single=False):
    """cost, gradient and the blocks the gradient was formed from, per listed trial"""
    idx = np.asarray(idx, dtype=np.int32)
    if single:
        cost, grad = ctx.dual_costgrad(int(idx[0]), g['lam'][idx[0]])
        cost, grad = np.array([cost]), grad[None]
    else:
        cost, grad = ctx.dual_costgrad_batch(idx, g['lam'][idx])
    return cost, grad, ctx.post_vsm(idx)


def check_c_d(c, g, tag, idx, cost, grad, Sig, lowrank=False):
    worst_c = worst_d = worst_z = worst_s = worst_l = 0.0
    zero_row = np.all(g['C'] == 0, axis=1)                # (there the gradient is log lambda - d alone: the entries with the least room)
    for i, trial in enumerate(idx):
        ref = reference(c, trial)
        worst_c = max(worst_c, ratio_c(ref, cost[i], lowrank))
        worst_d = max(worst_d, ratio_d(ref, grad[i], Sig[i]))
        worst_z = max(worst_z, ratio_d(ref, grad[i], Sig[i], rows=zero_row))
        worst_s = max(worst_s, rel(Sig[i], ref['Sig']))
        # what the cost says about the log-determinant alone, as a fraction of tau_logdet (the other terms taken from the reference)
        worst_l = max(worst_l, float(abs(-2 * (LD(cost[i]) - ref['cost_head']) - LD(ref['logdet']))) / tau_logdet(ref, lowrank))
    msg = ('%s %s: C %.3g (the log-determinant alone: %.3g of tau_logdet), D %.3g (zero row of C: %.3g), Sigma against dense numpy %.2e'
           % (c['name'], tag, worst_c, worst_l, worst_d, worst_z, worst_s))
    print(msg)
    assert worst_c <= 1.0 and worst_d <= 1.0 and worst_s <= TOL_SIGMA, msg


@pytest.mark.parametrize('c', CASES, ids=CASE_IDS)
def test_sections_c_d_cost_and_gradient_dense_engine(c):
    g = inputs(c)
    ctx = open_context(g)
    try:
        for gemm in (1, 0):
            ctx.set_option('dual_gemm', gemm)
            check_c_d(c, g, 'dense, %s form, batch' % ('GEMM' if gemm else 'vector'), c['idx'], *evaluate(ctx, g, c['idx']))
            if c['R'] == 1:
                check_c_d(c, g, 'dense, %s form, single-trial entry' % ('GEMM' if gemm else 'vector'), c['idx'], *evaluate(ctx, g, c['idx'], single=True))
        assert ctx.info('plan_lowrank') == 0.0
    finally:
        ctx.close()


@pytest.mark.parametrize('c', LOWRANK_CASES, ids=[c['name'] for c in LOWRANK_CASES])
def test_sections_c_d_cost_and_gradient_lowrank_engine(c):
    g = inputs(c)
    ctx = open_context(g, lowrank=True)
    try:
        for gemm in (1, 0):
            ctx.set_option('dual_gemm', gemm)
            out = evaluate(ctx, g, c['idx'])
            assert ctx.info('plan_lowrank') == 1.0
            check_c_d(c, g, 'low-rank, %s form' % ('GEMM' if gemm else 'vector'), c['idx'], *out, lowrank=True)
    finally:
        ctx.close()


# ---- E: the result of a trial does not depend on the launch ----------------------------------------------------------------------------------------------
def test_section_e_a_trial_keeps_its_bits_whatever_the_launch():
    """q = 21 (qpad - q = 11 rows of the next slot under zero table rows): trial 3 alone in a fresh context, first of three, last of three, and alone again
    after a three-trial call has left another trial's lambda in slot 1; then 3 of 5 trials out of order against the trials one by one"""
    c = next(c for c in CASES if c['name'] == 'list3of5')
    g = inputs(c)
    r = 3

    def one(ctx, idx):
        idx = np.asarray(idx, dtype=np.int32)
        cost, grad = ctx.dual_costgrad_batch(idx, g['lam'][idx])
        return cost, grad

    got = []
    ctx = open_context(g)
    try:
        cost, grad = one(ctx, [r])
        got.append((cost[0], grad[0], ctx.dual_post_mean(r, g['lam'][r])))
    finally:
        ctx.close()
    ctx = open_context(g)
    try:
        cost, grad = one(ctx, [r, 0, 4])
        got.append((cost[0], grad[0], ctx.dual_post_mean(r, g['lam'][r])))
        cost, grad = one(ctx, [1, 2, r])
        got.append((cost[2], grad[2], ctx.dual_post_mean(r, g['lam'][r])))
        one(ctx, [0, 4, 2])                                                          # slot 1 keeps the lambda of trial 4
        cost, grad = one(ctx, [r])
        got.append((cost[0], grad[0], ctx.dual_post_mean(r, g['lam'][r])))
        mixed = one(ctx, list(c['idx']))
        singles = [one(ctx, [t]) for t in c['idx']]
    finally:
        ctx.close()
    same = [all(np.array_equal(a, b) for a, b in zip(got[0], other)) for other in got[1:]]
    same_list = all(mixed[0][i] == s[0][0] and np.array_equal(mixed[1][i], s[1][0]) for i, s in enumerate(singles))
    print('trial %d alone / first of three / last of three / alone behind a three-trial call: same bits %s; list %s against one by one: %s'
          % (r, same, list(c['idx']), same_list))
    assert all(same) and same_list


# ---- G: masked forms --------------------------------------------------------------------------------------------------------------------------------------
def masked_problem(tables):
    """five trials of 130 bins, 21 neurons, 3 latents: lengths 1, 63, 64, 65, 130 and / or an observed-rows table; counts are zero where nothing is live"""
    key = 'masked_' + tables
    if key not in _inputs:
        g = dict(make_inputs(21, 3, MASKED_T, 5, tag=7))
        q, T, R = g['q'], g['T'], g['R']
        lens = np.array(MASKED_LENS if tables != 'rows' else (T,) * R, dtype=np.int32)
        n = np.arange(q)
        rows = np.stack([~np.isin(n, [0, 15, 16, q - 1]), n % 2 == 0, np.ones(q, bool), n == 17, np.ones(q, bool)]) if tables != 'lengths' else np.ones((R, q), bool)
        live = rows[:, :, None] & (np.arange(T)[None, None, :] < lens[:, None, None])
        g['Y'] = np.where(live, g['Y'], 0).astype(np.uint16)
        g.update(lens=lens, rows=rows, live=live, tables=tables)
        _inputs[key] = g
    return _inputs[key]


def masked_reference(g, trial):
    key = ('masked_' + g['tables'], trial)
    if key not in _refs:
        o, L = g['rows'][trial], int(g['lens'][trial])
        _refs[key] = reference_of(g['C'][o], g['d'][o], g['tau'], g['lam'][trial][o][:, :L], g['Y'][trial][o][:, :L])
    return _refs[key]


@pytest.mark.parametrize('lowrank', [0, 1], ids=['dense', 'lowrank'])
@pytest.mark.parametrize('tables', ['lengths', 'rows', 'both'])
def test_section_g_masked_forms_against_the_truncated_trials(tables, lowrank):
    """Option dual_masked with a length table, an observed-rows table, or both, lengths 1, 63, 64, 65 and T = 130 in one call, in the GEMM form and the
    vector form: the cost at 1e-8 relative of the truncated trial's (live neurons only, jitter included: the length table changes the log-determinant too,
    by trunc_logdet_correction, so no section C bound is claimed), section D's bound at the live entries, exact zeros at the others - whatever the caller
    passed there -, and a trial of full length with every neuron observed returns the bits it returns with no table set.

    lmy cannot be read through any entry point.  What guards it at the entries that are not live is the gradient: exactly 0 there, and inside section D's
    bound at every live entry, where V = C^T lmy enters through C_big^T K v with a bound of a few hundred u - a stray lmy of any size at a dead entry of
    an observed neuron's padded bins moves K v at the live bins by that size times |c| K.  The cost at 1e-8 relative would not see a tiny one.

    That last assertion found the one fault of this file: in the dense engine under a length table a full-length trial's gradient moved by 1.2e-16 of its
    largest entry, because its jitter was rounded into W (dual_jitter_len_kernel) and not into the assembled diagonal as with no table.  The dense engine
    now jitters only the shorter trials in W and scales the diagonal of the others behind the assembly (dual_diag_scale_full_kernel, assemble)."""
    g = masked_problem(tables)
    q, T, R = g['q'], g['T'], g['R']
    idx = np.arange(R, dtype=np.int32)
    full = 4                                                                         # length T and every row observed under all three tables
    lam_in = np.where(g['live'], g['lam'], -7.0)                                     # entries that are not live: ignored on input
    moved = []
    ctx = open_context(g, lowrank=bool(lowrank))
    try:
        for gemm in (1, 0):
            ctx.set_option('dual_gemm', gemm)
            ctx.set_option('dual_masked', 0)
            ctx.set_trial_lengths(None)
            ctx.set_observed(None)
            cost0, grad0 = ctx.dual_costgrad_batch(idx, g['lam'])
            ctx.set_option('dual_masked', 1)
            if tables != 'rows':
                ctx.set_trial_lengths(g['lens'])
            if tables != 'lengths':
                ctx.set_observed(g['rows'])
            cost, grad = ctx.dual_costgrad_batch(idx, lam_in)
            assert ctx.info('plan_lowrank') == float(lowrank)
            Sig = ctx.post_vsm(idx)
            e_c = r_d = e_s = 0.0
            for r in range(R):
                ref = masked_reference(g, r)
                o, L = g['rows'][r], int(g['lens'][r])
                e_c = max(e_c, float(abs(LD(cost[r]) - ref['cost']) / abs(ref['cost'])))
                gr = grad[r].reshape(q, T)
                r_d = max(r_d, ratio_d(ref, gr[o][:, :L], Sig[r][:L]))
                e_s = max(e_s, rel(Sig[r][:L], ref['Sig']))
                assert np.all(gr[~g['live'][r]] == 0.0), 'trial %d: the gradient is not 0 at an entry that is not live' % r
            same = cost[full] == cost0[full] and np.array_equal(grad[full], grad0[full])
            msg = ('%s, %s engine, %s form: cost %.2e of 1e-8, D at live entries %.3g, Sigma %.2e, full trial keeps its bits: %s (cost moves by %.2e '
                   'relative, gradient by %.2e of its largest entry)'
                   % (tables, 'low-rank' if lowrank else 'dense', 'GEMM' if gemm else 'vector', e_c, r_d, e_s, same,
                      abs(cost[full] - cost0[full]) / abs(cost0[full]), rel(grad[full], grad0[full])))
            print(msg)
            assert e_c <= TOL_COST_MASKED and r_d <= 1.0 and e_s <= TOL_SIGMA, msg
            if not same:
                moved.append(msg)
    finally:
        ctx.close()
    assert not moved, moved


def test_the_assembly_is_timed_with_and_without_a_length_table():
    """Option profile: every assembly of the dense engine opens and closes one record of its own (prof_assemble_*), also when a length table adds the
    pass over the diagonal of the full-length slots to it.  A record that is never closed is dropped or, worse, closed by a stale event: the count then
    stays behind or the time comes out negative."""
    g = masked_problem('lengths')
    idx = np.arange(g['R'], dtype=np.int32)
    ctx = open_context(g)
    try:
        ctx.set_option('profile', 1)
        ctx.dual_costgrad_batch(idx, g['lam'])
        n1, ms1 = ctx.info('prof_assemble_launches'), ctx.info('prof_assemble_ms')
        ctx.set_option('dual_masked', 1)
        ctx.set_trial_lengths(g['lens'])
        ctx.dual_costgrad_batch(idx, g['lam'])
        n2, ms2 = ctx.info('prof_assemble_launches'), ctx.info('prof_assemble_ms')
        ctx.set_option('profile', 0)
        print('assemblies timed: %d in %.4f ms with no table, %d in %.4f ms more under a length table' % (n1, ms1, n2 - n1, ms2 - ms1))
        assert n1 >= 1 and n2 - n1 == n1                  # (the same chunks both times: as many assemblies)
        assert 0.0 < ms1 < 100.0 and 0.0 < ms2 - ms1 < 100.0
    finally:
        ctx.close()


# ---- validation: a lambda that is not finite is refused on the host ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bad', [np.inf, np.nan, -np.inf], ids=['inf', 'nan', '-inf'])
def test_a_lambda_that_is_not_finite_is_refused_naming_trial_and_entry(bad):
    """Nothing that is not finite is launched: every call below must fail on the host.  The entry sits in neuron row 2 of trial 2 = slot 1: one of the
    qpad - q rows that the Lambda^T operand of slot 0 reads against zero table rows, where an Inf used to turn into NaN in the curvature of trial 0."""
    from funs import _hip
    c = next(c for c in CASES if c['name'] == 'slots3')
    g = inputs(c)
    T = g['T']
    lam = g['lam'].copy()
    e = 2 * T + 5
    lam[2].reshape(-1)[e] = bad
    named = r'\(trial 2, entry %d = ' % e
    ctx = open_context(g)
    try:
        with pytest.raises(_hip.HipBackendError, match='pgpfa_dual_costgrad_batch: lambda must be finite ' + named):
            ctx.dual_costgrad_batch(np.array([0, 2], dtype=np.int32), lam[[0, 2]])
        with pytest.raises(_hip.HipBackendError, match='pgpfa_dual_costgrad: lambda must be finite ' + named):
            ctx.dual_costgrad(2, lam[2])
        with pytest.raises(_hip.HipBackendError, match='pgpfa_dual_post_mean: lambda must be finite ' + named):
            ctx.dual_post_mean(2, lam[2])
        with pytest.raises(_hip.HipBackendError, match='pgpfa_dual_post_cov: lambda must be finite ' + named):
            ctx.dual_post_cov(2, lam[2])
        with pytest.raises(_hip.HipBackendError, match=r'lambda must be positive \(trial 1, entry 0 = '):
            zero = g['lam'].copy()
            zero[1, 0, 0] = 0.0
            ctx.dual_costgrad_batch(np.array([0, 1], dtype=np.int32), zero[[0, 1]])
        cost, _ = ctx.dual_costgrad_batch(np.array([0, 2], dtype=np.int32), g['lam'][[0, 2]])      # the context is as good as before
        assert np.all(np.isfinite(cost))
    finally:
        ctx.close()


def test_an_entry_that_is_not_live_may_hold_anything_under_dual_masked():
    g = masked_problem('both')
    idx = np.arange(g['R'], dtype=np.int32)
    ctx = open_context(g)
    try:
        ctx.set_option('dual_masked', 1)
        ctx.set_trial_lengths(g['lens'])
        ctx.set_observed(g['rows'])
        want = ctx.dual_costgrad_batch(idx, np.where(g['live'], g['lam'], 1.0))
        dead = np.argwhere(~g['live'])
        fill = np.where(np.arange(len(dead)) % 3 == 0, np.inf, np.where(np.arange(len(dead)) % 3 == 1, np.nan, -1.0))
        lam = g['lam'].copy()
        lam[tuple(dead.T)] = fill
        got = ctx.dual_costgrad_batch(idx, lam)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        from funs import _hip
        r, n, t = np.argwhere(g['live'])[-1]
        lam[r, n, t] = np.inf
        with pytest.raises(_hip.HipBackendError, match=r'lambda must be finite \(trial %d, entry %d = ' % (r, n * g['T'] + t)):
            ctx.dual_costgrad_batch(idx, lam)
    finally:
        ctx.close()
