"""The Poisson pass - rates exp(C x + d [+ off]), the likelihood part of the objective, its gradient and the per-bin curvature blocks
W_t = C^T diag(lambda_t) C - and the leave-one-neuron-out search against plain FP64 numpy at the bench's dimensions and at the seams of
every kernel form: poisson_mfma_kernel<PW,2> (up to 10 latents, 128 bins per workgroup), poisson_mfma_kernel<PW,1> (11..16 latents), the
GEMM form (17..32 latents: rates_wide_kernel, two products, dual_unpack_w_kernel) and the vector form poisson_pass_kernel<PMAX>, with their
option branches (held-out neuron, log-rate offsets and rate output, per-trial lengths, the second count plane).

* A - pgpfa_laplace_eval / pgpfa_laplace_hessian at the caller's points: GP draws x_k = chol(K_k) z, so that the log rates span several units.
* B - pgpfa_get_gram / pgpfa_get_gram_inverse at 500 and 333 bins.
* C - pgpfa_loo_predict against orc.newton_mode on the problem with the neuron's row deleted.
* D - pgpfa_dual_fixed_point / pgpfa_dual_finalize (offsets and the rate output) against the dense dual of one trial.

Error measures.  "Unsigned size" of an entry: the sum of the absolute values of the terms it sums, with h = C x + d, lambda = exp(h), |.|
entrywise and Kd the inverse Gram matrices the DEVICE holds (pgpfa_get_gram_inverse; with cond(K) near 1e5 two correct inverses differ by
1e-11, more than the tolerance - the inverse itself is test B's business):

  objective      f = sum lambda - sum y h + 1/2 sum_k x_k^T Kd_k x_k         size: sum lambda + sum y |h| + 1/2 sum_k |x_k|^T |Kd_k| |x_k|
  gradient       g = C^T (lambda - y) + [Kd_k^T x_k]_k                       size: |C|^T (lambda + y) + [|Kd_k|^T |x_k|]_k
  curvature      W_t = C^T diag(lambda_t) C                                  size: |C|^T diag(lambda_t) |C|
  dense Hessian  H[(k,t),(l,s)] = [k = l] Kd_k[t][s] + [t = s] W_t[k][l]     size: [k = l] |Kd_k[t][s]| + [t = s] size(W_t[k][l])

(the device's prior mat-vec runs down the columns of its K^-1 slabs, i.e. applies the transpose of what the getter returns; the asymmetry of
that matrix is printed).  "sharp" error: max over the entries of |device - numpy| / size, tolerance SHARP = 1e-12.  A sum of N terms that
each carry a few roundings and an exp of an argument below 10 in size is off by at most about (N + 100) 2^-53 of its unsigned size: 9e-14 at
N = q + T = 700, 6e-13 for the objective's longest chain T + p T; 1e-12 sits above both and a thousand times above what FP64 numpy itself
shows against numpy.longdouble (re-measured and printed by the bench case).  Entries of H off its pattern (different bins AND different
latents) must be exactly zero.  "worst bin": max over the bins t of (largest error of an entry of H that holds W_t) / (largest |entry| of
W_t), held to 1e-9 - a wrong tail tile cannot hide behind the largest entry of the matrix.  "project criteria" (DESIGN.md section 2), with
numpy's own inverse of orc.make_K: objective 1e-10 relative, gradient and Hessian 1e-9 of their largest entry.

Which form ran.  With option profile = 1 the GEMM form shows product launches inside the call (prof_gemm_launches) and every other form shows
none; the test asserts that.  Beyond 16 latents dual_gemm = 0 and use_mfma = 0 both end in poisson_pass_kernel<PMAX> (one kernel: there is
nothing to tell apart); up to 16 latents the library offers no way to tell poisson_mfma_kernel from the vector kernel after the fact
(prof_poisson_launches counts either), so those cases rest on the option alone.

Every test prints the errors it measured; docs/history/poisson_pass_dense_tests.md holds them."""
import time

import numpy as np
import pytest

from oracle import pgpfa_oracle as orc

pytestmark = pytest.mark.gpu

BIN = 10.0
SHARP = 1e-12
R_EVAL, CHUNK = 6, 4
EVAL_LIST = [5, 0, 3, 3, 1, 0, 2, 5, 4, 1, 3]                # 11 entries over chunks of 4 slots (4 + 4 + 3), trials repeated; every entry is checked


def rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(1e-300, np.max(np.abs(b)))


def _ratio(err, size):
    """largest err / size over the entries; an entry of size zero (no term at all: a bin behind a trial's length) must be exactly zero"""
    err, size = np.asarray(err, dtype=np.float64), np.asarray(size, dtype=np.float64)
    ok = size > 0
    assert np.all(err[~ok] == 0.0)
    return float(np.max(err[ok] / size[ok])) if np.any(ok) else 0.0


def _gp_draws(tau, T, n, rng):
    """n points [p][T] with x_k = chol(K_k) z"""
    L = np.linalg.cholesky(orc.make_K(tau, T, BIN))
    return np.einsum('kts,nks->nkt', L, rng.standard_normal((n, len(tau), T)))


def _params(kind, q, p, T, seed):
    """'bench': the generating parameters of the bench's workload; otherwise the same distributions from a Generator, the loadings scaled by
    sqrt(10 / p) beyond 10 latents (log rates keep the bench's spread), and for 'linspace' the timescales of the config-5 tests"""
    if kind == 'bench':
        import bench
        true, _ = bench.synth_shard(q, p, T, 0, 12, 0)
        return true['C'], true['d'], true['tau']
    rng = np.random.default_rng(seed)
    C = (rng.random((q, p)) - 0.5) * min(1.0, np.sqrt(10.0 / p))
    d = -2.0 * rng.random(q) - 1.0
    tau = rng.random(p) + 0.01 if kind == 'gen' else np.linspace(0.1, 0.5, p)
    return C, d, tau


def _counts(C, d, tau, T, R, rng, high=False, dtype=None):
    """counts drawn from the model at latents of their own; high: 1 % of the entries replaced by counts of 256..1000 (one of exactly 1000)"""
    X = _gp_draws(tau, T, R, rng)
    Y = rng.poisson(np.exp(np.einsum('qk,rkt->rqt', C, X) + d[None, :, None]))
    if high:
        m = rng.random(Y.shape) < 0.01
        Y[m] = rng.integers(256, 1001, size=int(m.sum()))
        Y[R - 1, C.shape[0] - 1, T - 1] = 1000
        return Y.astype(np.uint16)
    if dtype is not None:
        return np.minimum(Y, 60000).astype(dtype)
    return np.minimum(Y, 255).astype(np.uint8)


def _pass_reference(C, d, Kd, X, Y, Tl=None, dt=np.float64):
    """objective, gradient [p][T] and curvature blocks [T][p][p] of one point with their unsigned sizes, in the precision dt.
    Tl: bins t >= Tl carry no likelihood term (pgpfa_set_trial_lengths)."""
    C, d, Kd, X, Y = (np.asarray(a, dtype=dt) for a in (C, d, Kd, X, Y))
    q, p = C.shape
    T = X.shape[1]
    h = C @ X + d[:, None]
    lam = np.exp(h)
    if Tl is not None:
        lam[:, Tl:] = 0
        h = h.copy()
        h[:, Tl:] = 0
    Ca, Xa, Ka = np.abs(C), np.abs(X), np.abs(Kd)
    KX = np.stack([Kd[k].T @ X[k] for k in range(p)])
    KXa = np.stack([Ka[k].T @ Xa[k] for k in range(p)])
    f = lam.sum() - (Y * h).sum() + (X * KX).sum() / 2
    fs = lam.sum() + (Y * np.abs(h)).sum() + (Xa * KXa).sum() / 2
    g = C.T @ (lam - Y) + KX
    gs = Ca.T @ (lam + Y) + KXa
    CC = (C[:, :, None] * C[:, None, :]).reshape(q, p * p)
    W = (lam.T @ CC).reshape(T, p, p)
    Ws = (lam.T @ np.abs(CC)).reshape(T, p, p)
    return dict(f=f, fs=fs, g=g, gs=gs, W=W, Ws=Ws, lam=lam)


def _check_hessian(H, Kd, Knp, ref, p, T):
    """The dense Hessian of one point against ref (a _pass_reference): returns (entries off the pattern that are not zero, sharp error,
    worst-bin error, error against numpy's own inverse relative to the largest entry)."""
    H4 = H.reshape(p, T, p, T)
    ar = np.arange(T)
    W, Ws = ref['W'], ref['Ws']
    nonzero, sharp, e_np, hmax = 0, 0.0, 0.0, 0.0
    ebin = np.zeros(T)
    for k in range(p):
        for l in range(p):
            B = H4[k, :, l, :]
            if k != l:
                nonzero += int(np.count_nonzero(B)) - int(np.count_nonzero(B[ar, ar]))
                err = np.abs(B[ar, ar] - W[:, k, l])
                sharp = max(sharp, _ratio(err, Ws[:, k, l]))
                e_np = max(e_np, float(err.max()))
            else:
                want = Kd[k].copy()
                want[ar, ar] += W[:, k, k]
                size = np.abs(Kd[k])
                size[ar, ar] += Ws[:, k, k]
                err_full = np.abs(B - want)
                sharp = max(sharp, _ratio(err_full, size))
                err = err_full[ar, ar]
                want_np = Knp[k].copy()
                want_np[ar, ar] += W[:, k, k]
                e_np = max(e_np, float(np.max(np.abs(B - want_np))))
                hmax = max(hmax, float(np.max(np.abs(want_np))))
            ebin = np.maximum(ebin, err)
    worst_bin = _ratio(ebin, np.max(np.abs(W), axis=(1, 2)))
    return nonzero, sharp, worst_bin, e_np / hmax


# ---------------------------------------------------------------------------------------------------------------
# A: evaluation at the caller's points
# ---------------------------------------------------------------------------------------------------------------
# (id, parameters, q, p, T, counts, options, form, per-trial lengths)
_WIDE_FORMS = [('gemm', {}), ('dual_gemm0', {'dual_gemm': 0}), ('use_mfma0', {'use_mfma': 0})]
EVAL_CASES = [
    ('bench_200x10x500', 'bench', 200, 10, 500, 'u8', {}, 'mfma', False),
    ('bench_200x10x500_counts_to_1000', 'bench', 200, 10, 500, 'high', {}, 'mfma', False),
    ('bench_200x10x500_rates_in_the_hundreds', 'loud', 200, 10, 500, 'u16', {}, 'mfma', False),
    ('77x7x333', 'gen', 77, 7, 333, 'u8', {}, 'mfma', False),
    ('77x7x333_vector', 'gen', 77, 7, 333, 'u8', {'use_mfma': 0}, 'vector', False),
    ('77x7x333_lengths', 'gen', 77, 7, 333, 'u8', {}, 'mfma', True),
    ('130x3x203', 'gen', 130, 3, 203, 'u8', {}, 'mfma', False),
    ('17x1x150', 'gen', 17, 1, 150, 'u8', {}, 'mfma', False),
    ('61x10x128', 'gen', 61, 10, 128, 'u8', {}, 'mfma', False),
    ('61x10x129', 'gen', 61, 10, 129, 'high', {}, 'mfma', False),
    ('61x10x257', 'gen', 61, 10, 257, 'u8', {}, 'mfma', False),
    ('61x10x257_lengths', 'gen', 61, 10, 257, 'u8', {}, 'mfma', True),
    ('90x12x203', 'gen', 90, 12, 203, 'u8', {}, 'mfma', False),
    ('90x14x203', 'gen', 90, 14, 203, 'high', {}, 'mfma', False),
    ('90x16x203', 'gen', 90, 16, 203, 'u8', {}, 'mfma', False),
    ('90x14x203_lengths', 'gen', 90, 14, 203, 'u8', {}, 'mfma', True),
]
for _q, _p in ((70, 17), (70, 20), (70, 27), (70, 32), (64, 20)):
    for _form, _opts in _WIDE_FORMS:
        EVAL_CASES.append(('%dx%dx150_%s' % (_q, _p, _form), 'gen', _q, _p, 150, 'high' if _p == 27 else 'u8', _opts, 'gemm' if _form == 'gemm' else 'vector', False))
EVAL_CASES.append(('70x20x150_gemm_lengths', 'gen', 70, 20, 150, 'u8', {}, 'gemm', True))


def _longdouble_self_check(C, d, Kd, X, Y):
    """numpy's own error: the FP64 reference against the same expressions in numpy.longdouble, in the sharp measure"""
    a = _pass_reference(C, d, Kd, X, Y)
    b = _pass_reference(C, d, Kd, X, Y, dt=np.longdouble)
    return (float(abs(a['f'] - b['f']) / b['fs']), float(np.max(np.abs(a['g'] - b['g']) / b['gs'])), float(np.max(np.abs(a['W'] - b['W']) / b['Ws'])))


@pytest.mark.timeout(600)
@pytest.mark.parametrize('case', EVAL_CASES, ids=[c[0] for c in EVAL_CASES])
def test_eval_and_hessian_against_numpy(case):
    """Test A.  A context of 6 trials with a chunk of 4 slots (option chunk_trials); pgpfa_laplace_eval over a list of 11 entries with repeated
    trials (chunks of 4, 4 and 3 slots), every entry at a GP draw of its own, and pgpfa_laplace_hessian at two of them; objective, every
    gradient entry and every curvature entry to 1e-12 of their unsigned size, the Hessian's pattern exactly, the worst bin, the project's
    criteria with numpy's own K^-1, and the form that ran (module docstring).  At three cases the file's own restatement (_pass_reference, which
    also yields the unsigned sizes) is tied to orc.nlp, orc.nlp_grad and orc.poisson_blocks to 1e-14 of those sizes.  'lengths': per-trial bin counts, one of them a multiple of 16,
    one below the first 16-bin tile's end, one equal to T.  Measured errors: docs/history/poisson_pass_dense_tests.md."""
    from funs import _hip
    tag, kind, q, p, T, counts, opts, form, lengths = case
    rng = np.random.default_rng(1000 * q + 10 * p + T)
    C, d, tau = _params('bench' if kind == 'loud' else kind, q, p, T, q + p + T)
    if kind == 'loud':
        d = d + 6.5                                                # rates in the hundreds per bin; log rates stay below 10
    Y = _counts(C, d, tau, T, R_EVAL, rng, high=(counts == 'high'), dtype=np.uint16 if counts == 'u16' else None)
    lens = None
    if lengths:
        lens = np.array([T, 5, T - 1, (T // 2) // 16 * 16, T - 17, 64 + 3], dtype=np.int32)
        for r in range(R_EVAL):
            Y[r, :, lens[r]:] = 0
    X = _gp_draws(tau, T, len(EVAL_LIST), rng)
    lst = np.array(EVAL_LIST, dtype=np.int32)
    h_probe = [(3, 2), (R_EVAL - 1, len(EVAL_LIST) - 4)]          # (trial, point): the Hessian call takes any point for any trial
    ctx = _hip.Context(q, p, T, R_EVAL, BIN)
    try:
        ctx.set_option('chunk_trials', CHUNK)
        for k, v in opts.items():
            ctx.set_option(k, v)
        ctx.upload_counts(Y)
        assert ctx.info('counts_two_bytes') == float(Y.max() > 255)
        if lens is not None:
            ctx.set_trial_lengths(lens)
        ctx.set_params(C, d, tau)
        Kd = ctx.gram_inverse()
        ctx.set_option('profile', 1)
        f, g = ctx.laplace_eval(lst, X)
        gemm_eval = ctx.info('prof_gemm_launches')
        assert ctx.info('chunk_trials') == float(CHUNK)
        Hs = [ctx.laplace_hessian(r, X[i]) for r, i in h_probe]
        gemm_hess = ctx.info('prof_gemm_launches') - gemm_eval
        poisson_launches = ctx.info('prof_poisson_launches')
    finally:
        ctx.close()
    if form == 'gemm':
        assert gemm_eval > 0 and gemm_hess > 0, (gemm_eval, gemm_hess)
    else:
        assert gemm_eval == 0 and gemm_hess == 0, (gemm_eval, gemm_hess)
    assert poisson_launches == 3 + len(h_probe)
    Knp = np.linalg.inv(orc.make_K(tau, T, BIN))
    asym = np.max(np.abs(Kd - Kd.transpose(0, 2, 1))) / np.max(np.abs(Kd))
    e_f = e_g = e_fp = e_gp = 0.0
    hrange = [np.inf, -np.inf]
    for i, r in enumerate(lst):
        Tl = None if lens is None else int(lens[r])
        Yr = Y[r].astype(np.float64)
        ref = _pass_reference(C, d, Kd, X[i], Yr, Tl)
        assert np.all(np.isfinite(g[i])) and np.isfinite(f[i])
        e_f = max(e_f, abs(f[i] - ref['f']) / ref['fs'])
        e_g = max(e_g, _ratio(np.abs(g[i] - ref['g']), ref['gs']))
        hh = C @ X[i] + d[:, None]
        hrange = [min(hrange[0], hh.min()), max(hrange[1], hh.max())]
        # the project's criteria, numpy's own inverse (the padded bins of a shortened trial carry the prior alone)
        lam = ref['lam']
        f_np = lam.sum() - (Yr * np.where(lam > 0, hh, 0.0)).sum() + 0.5 * np.einsum('kt,kts,ks->', X[i], Knp, X[i])
        g_np = C.T @ (lam - Yr) + np.einsum('kts,ks->kt', Knp, X[i])
        e_fp = max(e_fp, abs(f[i] - f_np) / abs(f_np))
        e_gp = max(e_gp, float(np.max(np.abs(g[i] - g_np)) / np.max(np.abs(g_np))))
    nz = 0
    e_h = e_bin = e_hp = 0.0
    for (r, i), H in zip(h_probe, Hs):
        Tl = None if lens is None else int(lens[r])
        ref = _pass_reference(C, d, Kd, X[i], Y[r].astype(np.float64), Tl)
        a, b, c_, e = _check_hessian(H, Kd, Knp, ref, p, T)
        nz, e_h, e_bin, e_hp = nz + a, max(e_h, b), max(e_bin, c_), max(e_hp, e)
    print('%s [%s]: log rates %.1f .. %.1f, counts up to %d, products in eval / hessian %d / %d; sharp: objective %.2e, gradient %.2e, curvature %.2e '
          '(worst bin %.2e, %d entries off the pattern); project criteria: objective %.2e, gradient %.2e, Hessian %.2e; asymmetry of the device K^-1 %.2e'
          % (tag, form, hrange[0], hrange[1], Y.max(), gemm_eval, gemm_hess, e_f, e_g, e_h, e_bin, nz, e_fp, e_gp, e_hp, asym))
    if tag in ('bench_200x10x500', '90x14x203', '70x32x150_gemm'):
        # the file's own restatement against the oracle's structured functions at this point (the device K^-1 is symmetrised for them: orc applies
        # it untransposed); both are FP64 numpy, so they agree to a few roundings of the unsigned sizes
        i = len(lst) - 1
        Yr, Ks = Y[lst[i]].astype(np.float64), 0.5 * (Kd + Kd.transpose(0, 2, 1))
        ref = _pass_reference(C, d, Ks, X[i], Yr)
        o = (abs(orc.nlp(X[i], Yr, C, d, Ks) - ref['f']) / ref['fs'], _ratio(np.abs(orc.nlp_grad(X[i], Yr, C, d, Ks) - ref['g']), ref['gs']),
             _ratio(np.abs(orc.poisson_blocks(X[i], C, d) - ref['W']), ref['Ws']))
        print('%s: _pass_reference against orc.nlp / orc.nlp_grad / orc.poisson_blocks: %.2e / %.2e / %.2e' % (tag, o[0], o[1], o[2]))
        assert max(o) <= 1e-14
    if tag == 'bench_200x10x500':
        t0 = time.time()
        s = _longdouble_self_check(C, d, Kd, X[0], Y[lst[0]].astype(np.float64))
        print('%s: FP64 numpy against numpy.longdouble (eps %.1e): objective %.2e, gradient %.2e, curvature %.2e (%.1f s)'
              % (tag, np.finfo(np.longdouble).eps, s[0], s[1], s[2], time.time() - t0))
        assert max(s) <= 1e-13                                 # (a device error above 1e-13 is a finding: the yardstick must sit below that)
    assert nz == 0
    assert e_f <= SHARP and e_g <= SHARP and e_h <= SHARP
    assert e_bin <= 1e-9
    assert e_fp <= 1e-10 and e_gp <= 1e-9 and e_hp <= 1e-9


# ---------------------------------------------------------------------------------------------------------------
# B: Gram matrices and their inverses at the bench's bin counts
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T', [500, 333])
@pytest.mark.parametrize('which', ['bench', 'linspace'])
def test_gram_and_inverse_at_bench_bin_counts(which, T):
    """Test B.  pgpfa_get_gram against orc.make_K entry by entry: the kernel evaluates the expression in make_K's order and the two exp
    differ by a few units in the last place, so 1e-15 of every entry (4.5 ulp; entries in the subnormal range, below 1e-300, are left out of
    the relative figure).  pgpfa_get_gram_inverse: the residual max |K^-1 K - I| (product in FP64 numpy) against the same figure of
    np.linalg.inv(K), measured here; the device may exceed it by a factor of 10 - both are backward-stable factorisations of one matrix, and
    the device's blocked order differs."""
    from funs import _hip
    p, q = 10, 8
    tau = _params('bench', 200, p, 16, 0)[2] if which == 'bench' else np.linspace(0.1, 0.5, p)
    ctx = _hip.Context(q, p, T, 1, BIN)
    try:
        rng = np.random.default_rng(T)
        ctx.set_params(rng.standard_normal((q, p)), rng.standard_normal(q), tau)
        Kdev, Kinv = ctx.gram(), ctx.gram_inverse()
    finally:
        ctx.close()
    K = orc.make_K(tau, T, BIN)
    e_gram = float(np.max(np.abs(Kdev - K) / np.maximum(np.abs(K), 1e-285)))
    assert np.all(np.abs(Kdev - K) <= 1e-15 * np.abs(K) + 1e-300)
    eye = np.eye(T)
    res_dev = np.array([np.max(np.abs(Kinv[k] @ K[k] - eye)) for k in range(p)])
    res_np = np.array([np.max(np.abs(np.linalg.inv(K[k]) @ K[k] - eye)) for k in range(p)])
    cond = np.array([np.linalg.cond(K[k]) for k in range(p)])
    print('%s timescales, %d bins: Gram entries %.2e; cond(K) up to %.1e; residual |K^-1 K - I|: device %.2e, numpy %.2e (per latent, device / numpy: %s)'
          % (which, T, e_gram, cond.max(), res_dev.max(), res_np.max(), ' '.join('%.2f' % x for x in res_dev / res_np)))
    assert res_dev.max() <= 10.0 * res_np.max()


# ---------------------------------------------------------------------------------------------------------------
# C: the held-out neuron
# ---------------------------------------------------------------------------------------------------------------
_LOO_REFS = {}


def _loo_problem(q, p, T, R, high):
    rng = np.random.default_rng(7 * q + 3 * p + T)
    C, d, tau = _params('gen', q, p, T, q * p + T)
    if high:
        d = d.copy()
        d[7] = np.log(300.0)                                      # counts of 200 .. 400 per bin on neuron 7: the second plane
    Y = _counts(C, d, tau, T, R, rng, dtype=np.uint16 if high else None)
    return C, d, tau, Y


def _loo_reference(Y, C, d, Kinv, neurons, x_full):
    """rates of the held-out neurons at the polished mode of the problem with their row deleted (orc.newton_mode, warm-started from the mode
    of the full problem: the mode of a strictly convex problem does not depend on the start)"""
    out, its = {}, []
    Yf = Y.astype(np.float64)
    for n in neurons:
        X, _, it = orc.newton_mode(np.delete(Yf, n, 0), np.delete(C, n, 0), np.delete(d, n, 0), Kinv, x0=x_full)
        out[n] = np.exp(C[n] @ X + d[n])
        its.append(it)
    return out, its


def _item_errors(pred, ref):
    return np.array([np.max(np.abs(pred[n] - ref[n])) / np.max(np.abs(ref[n])) for n in sorted(ref)])


LOO_SHAPES = [(48, 10, 130, 2, False), (40, 4, 150, 2, False), (40, 4, 150, 1, True), (45, 12, 100, 1, False), (40, 16, 100, 1, False), (40, 20, 64, 1, False)]


@pytest.mark.timeout(900)
@pytest.mark.parametrize('cov_mode', [1, 2])
@pytest.mark.parametrize('shape', LOO_SHAPES, ids=['%dx%dx%d_%dtrials%s' % (s[0], s[1], s[2], s[3], '_counts_above_255' if s[4] else '') for s in LOO_SHAPES])
def test_loo_all_neurons_against_dense_newton(shape, cov_mode):
    """Test C, every neuron of every listed trial: poisson_mfma_kernel<PW,2> and <PW,1> under a mask with the held-out neuron in every neuron
    tile (48 x 10, 45 x 12, 40 x 16: three tiles of 16, the last ragged or full), the vector kernel under a mask beyond 16 latents (40 x 20:
    the GEMM form is switched off while a mask is active), one shape with counts of 200..400 on a held-out neuron (loo_predict_kernel's
    second plane), under both workspace plans (asserted: plan_lowrank follows cov_mode).  Predicted rates of every item to 1e-7 of the item's largest rate (the project's LOO criterion
    asks 1e-7 of the largest rate of all); err_sum = sum (y - y_pred)^2 from the returned rates to 1e-12; every item converged.  On the way:
    a Laplace E-step before the prediction pass and the same one after it return the same bits, and the posterior getters return the same
    bits right after the pass."""
    from funs import _hip
    q, p, T, ntr, high = shape
    R = 5
    C, d, tau, Y = _loo_problem(q, p, T, R, high)
    trials = [3, 1][:ntr]
    key = shape
    if key not in _LOO_REFS:
        t0 = time.time()
        Kinv = np.linalg.inv(orc.make_K(tau, T, BIN))
        refs, its = [], []
        for r in trials:
            xf, _, it0 = orc.newton_mode(Y[r].astype(np.float64), C, d, Kinv)
            rr, it = _loo_reference(Y[r], C, d, Kinv, range(q), xf)
            refs.append(rr)
            its += it
        _LOO_REFS[key] = (refs, max(its), time.time() - t0)
    refs, it_max, t_ref = _LOO_REFS[key]
    idx = np.array(trials, dtype=np.int32)
    eidx = np.array([0, 3, 4], dtype=np.int32)
    ctx = _hip.Context(q, p, T, R, BIN)
    try:
        ctx.upload_counts(Y)
        assert ctx.info('counts_two_bytes') == float(high)
        ctx.set_option('cov_mode', cov_mode)
        ctx.set_params(C, d, tau)
        obj0, it0, st0 = ctx.estep_laplace(eidx)
        assert np.all(st0 == 0)
        pm0, vsm0 = ctx.post_mean(eidx).copy(), ctx.post_vsm(eidx).copy()
        pred, err = ctx.loo_predict(idx)
        assert ctx.info('last_loo_unconverged') == 0
        plan = ctx.info('plan_lowrank')
        same_mid = np.array_equal(ctx.post_mean(eidx), pm0) and np.array_equal(ctx.post_vsm(eidx), vsm0)
        obj1, it1, st1 = ctx.estep_laplace(eidx)
        same_after = obj1 == obj0 and np.array_equal(it1, it0) and np.array_equal(st1, st0) and np.array_equal(ctx.post_mean(eidx), pm0) \
            and np.array_equal(ctx.post_vsm(eidx), vsm0)
    finally:
        ctx.close()
    assert plan == float(cov_mode == 2), plan                 # (cov_mode 2 falls back to the dense plan silently where the ranks do not fit)
    assert pred.shape == (ntr, q, T) and np.all(np.isfinite(pred)) and np.all(pred > 0)
    e_items = np.concatenate([_item_errors(pred[i], refs[i]) for i in range(ntr)])
    err_np = float(np.sum((Y[idx].astype(np.float64) - pred) ** 2))
    e_all = max(rel(pred[i], np.stack([refs[i][n] for n in range(q)])) for i in range(ntr))
    print('%s cov_mode %d (low-rank plan %g): %d items, worst item %.2e (neuron %d), of the largest rate of all %.2e, err_sum %.2e; counts up to %d; '
          'posterior untouched %s, E-step repeats its bits %s; references: at most %d Newton iterations, %.1f s'
          % (shape[:3], cov_mode, plan, len(e_items), e_items.max(), int(np.argmax(e_items)) % q, e_all, abs(err - err_np) / err_np, Y.max(),
             same_mid, same_after, it_max, t_ref))
    assert e_items.max() <= 1e-7
    assert abs(err - err_np) <= 1e-12 * err_np
    assert same_mid and same_after


@pytest.mark.timeout(1200)
def test_loo_at_bench_dimensions():
    """Test C at 200 x 10 x 500: a context of 64 trials, all 200 neurons of trials 37 and 5 - 400 items in chunks of 64 slots, so that a
    trial's items neither fill whole chunks nor start on a chunk boundary (asserted), under the low-rank plan the bench runs (asserted).  Exact references (orc.newton_mode on the 199-neuron
    problem, warm-started from the trial's full mode) for the held-out neurons 0, 15, 16, 191, 192, 199 of trial 37 - the first and last of
    the first, second and last (half-full) neuron tiles - and 16, 199 of trial 5: 1e-7 of the item's largest rate.  Leaving out one neuron
    moves the prediction by a few per cent (printed): an ignored mask sits 5 orders of magnitude above the tolerance.  For all 400 items:
    finite positive rates, err_sum = sum (y - y_pred)^2 recomputed from the returned rates to 1e-12, last_loo_unconverged = 0."""
    import bench
    from funs import _hip
    q, p, T, R = 200, 10, 500, 64
    true, Ys = bench.synth_shard(q, p, T, R, 12, 0)
    C, d, tau = true['C'], true['d'], true['tau']
    Y = np.stack(Ys)
    trials = [37, 5]
    exact = {37: [0, 15, 16, 191, 192, 199], 5: [16, 199]}
    ctx = _hip.Context(q, p, T, R, BIN)
    try:
        ctx.upload_counts(Y)
        ctx.set_params(C, d, tau)
        t0 = time.time()
        pred, err = ctx.loo_predict(np.array(trials, dtype=np.int32))
        t_gpu = time.time() - t0
        bad = ctx.info('last_loo_unconverged')
        chunk = int(ctx.info('chunk_trials'))
        plan = ctx.info('plan_lowrank')
    finally:
        ctx.close()
    assert chunk < q and q % chunk != 0, chunk
    assert plan == 1.0                                        # the bench's own plan
    assert bad == 0
    assert pred.shape == (2, q, T) and np.all(np.isfinite(pred)) and np.all(pred > 0)
    err_np = float(np.sum((Y[trials].astype(np.float64) - pred) ** 2))
    Kinv = np.linalg.inv(orc.make_K(tau, T, BIN))
    t0 = time.time()
    worst, moved, its = 0.0, [], []
    for i, r in enumerate(trials):
        xf, _, it0 = orc.newton_mode(Y[r].astype(np.float64), C, d, Kinv)
        refs, it = _loo_reference(Y[r], C, d, Kinv, exact[r], xf)
        its += [it0] + it
        e = _item_errors(pred[i], refs)
        for n, en in zip(sorted(refs), e):
            full = np.exp(C[n] @ xf + d[n])
            moved.append(np.max(np.abs(refs[n] - full) / full))
            print('bench LOO trial %d neuron %3d: %.2e of the largest rate; leaving it out moves its rate by up to %.1f %%' % (r, n, en, 100 * moved[-1]))
        worst = max(worst, e.max())
    print('bench LOO: chunk of %d slots (low-rank plan %g), 400 items in %.1f s; worst exact item %.2e; err_sum %.2e; mask moves the rates by %.1f .. %.1f %%; '
          'references: Newton iterations %s, %.1f s' % (chunk, plan, t_gpu, worst, abs(err - err_np) / err_np, 100 * min(moved), 100 * max(moved), its, time.time() - t0))
    assert worst <= 1e-7
    assert abs(err - err_np) <= 1e-12 * err_np


# ---------------------------------------------------------------------------------------------------------------
# D: offsets and the rate output
# ---------------------------------------------------------------------------------------------------------------
DUAL_CASES = [('200x10x500', 'bench', 200, 10, 500, {}), ('90x14x203', 'gen', 90, 14, 203, {}), ('60x20x150_vector', 'gen', 60, 20, 150, {'dual_gemm': 0})]


@pytest.mark.timeout(1200)
@pytest.mark.parametrize('case', DUAL_CASES, ids=[c[0] for c in DUAL_CASES])
def test_fixed_point_offsets_and_rate_output_against_dense_dual(case):
    """Test D.  pgpfa_dual_fixed_point from the cold start on 3 of 4 trials, low-rank plan (the default at these sizes, asserted): every Poisson pass of it adds the offsets 1/2 c_n^T Sigma_t c_n to
    the log rate (a.off) and writes the rates (a.lam_out) - poisson_mfma_kernel<PW,2> at 10 latents (two bin tiles per wave, 4 workgroups
    along the bins), <PW,1> at 14, the vector kernel at 20 with dual_gemm = 0.  At the returned lambda, per trial on the dense matrices
    (_dense_dual_reference of test_gpu_round3: p T <= 5000): the reference's dual gradient vanishes to 1e-7 in the max-norm (the solver stops
    at 1e-8 in the offsets, which IS that max-norm), fopt is the dense dual cost to 1e-9 relative, lam_out = exp(rho) to 1e-15 of its largest
    entry, and post_mean after pgpfa_dual_finalize equals -K C_big (lambda - y) in structured numpy to 1e-9."""
    from funs import _hip
    from test_gpu_round3 import _dense_dual_reference
    tag, kind, q, p, T, opts = case
    R = 4
    rng = np.random.default_rng(q + p + T)
    C, d, tau = _params(kind, q, p, T, 3 * q + p)
    Y = _counts(C, d, tau, T, R, rng)
    idx = np.array([2, 0, 3], dtype=np.int32)
    ctx = _hip.Context(q, p, T, R, BIN)
    try:
        ctx.upload_counts(Y)
        for k, v in opts.items():
            ctx.set_option(k, v)
        ctx.set_params(C, d, tau)
        t0 = time.time()
        rho, fopt, passes, status, lam = ctx.dual_fixed_point(idx, None, want_lam=True)
        t_gpu = time.time() - t0
        plan = ctx.info('plan_lowrank')
        ctx.dual_finalize(idx, None)
        pm = ctx.post_mean(idx)
    finally:
        ctx.close()
    assert plan == 1.0, plan                                  # the plan all three sizes take by default
    assert np.all(status == 0), (status, passes)
    e_lam = np.max(np.abs(lam - np.exp(rho))) / np.max(lam)
    K = orc.make_K(tau, T, BIN)
    t0 = time.time()
    e_grad = e_cost = e_mean = e_mean_dense = 0.0
    for i, r in enumerate(idx):
        y = Y[r].astype(np.float64)
        cost, grad, mean, _ = _dense_dual_reference(C, d, tau, y.reshape(-1), lam[i], T, BIN)
        e_grad = max(e_grad, float(np.max(np.abs(grad))))
        e_cost = max(e_cost, abs(fopt[i] - cost) / abs(cost))
        v = C.T @ (lam[i].reshape(q, T) - y)
        e_mean = max(e_mean, rel(pm[i], -np.einsum('kts,ks->kt', K, v)))
        e_mean_dense = max(e_mean_dense, rel(pm[i], mean))
    print('%s (low-rank plan %g): passes %s in %.1f s; max |dual gradient| %.2e, fopt %.2e, lam_out vs exp(rho) %.2e, post_mean %.2e; dense references %.1f s'
          % (tag, plan, passes.tolist(), t_gpu, e_grad, e_cost, e_lam, e_mean, time.time() - t0))
    assert e_grad <= 1e-7
    assert e_cost <= 1e-9
    assert e_lam <= 1e-15
    assert e_mean <= 1e-9 and e_mean_dense <= 1e-9
