"""Host side of the importance-sampled log evidence (pgpfa_importance_weights, util.importanceEvidence), without a GPU:

* the numpy restatement of what the device computes from (C, d, x*, draws, live mask),

      log w_s = - sum_{(n,t) live} lambda*_nt phi(c_n . delta_st),  lambda* = exp(d + C x*),  phi(a) = e^a - 1 - a - a^2 / 2,
      log_ratio = logmeanexp_s log w_s,   ess = (sum w)^2 / sum w^2;

  the GPU tests import these functions as their yardstick;
* the identity behind it, pinned to the dense definition with the oracle's objective, gradient and Hessian at a Newton-polished mode: for every draw
  log p(y, x_s) - log N(x_s; x*, H^-1) - log Z_Laplace - log w_s = - g . delta_s up to rounding, g the gradient left at the mode;
* header, binding and Python layer carry the new entry points."""
import inspect
import os
import re

import numpy as np

from conftest import ROOT, load_golden
from oracle import pgpfa_oracle as orc

BIN_MS = 10.0


# ---- the yardstick -------------------------------------------------------------------------------------------------------------------------------
def phi(a):
    """e^a - 1 - a - a^2 / 2 (>= 0 for a >= 0, the sign of a^3 near 0); +inf where e^a overflows"""
    with np.errstate(over='ignore'):
        return (np.expm1(a) - a) - 0.5 * a * a


def log_weights(C, d, xstar, X, live=None, with_scale=False):
    """log w_s [S] of the draws X [S][p][T] around the mode xstar [p][T]; live: (q, T) booleans (None: all).  Entries that are not live are
    selected out, never multiplied out.  with_scale: also sum over the live entries of lambda* (e^a + 1 + |a| + a^2 / 2), the magnitude of the
    terms that cancel inside phi - what a rounding bound of log w_s scales with."""
    C, d = np.asarray(C, dtype=np.float64), np.asarray(d, dtype=np.float64).reshape(-1)
    xstar, X = np.asarray(xstar, dtype=np.float64), np.asarray(X, dtype=np.float64)
    live = np.ones((C.shape[0], xstar.shape[1]), bool) if live is None else np.asarray(live, dtype=bool)
    with np.errstate(over='ignore', invalid='ignore'):
        lam = np.exp(d[:, None] + C @ xstar)
        a = np.einsum('nk,skt->snt', C, X - xstar[None])
        lw = -np.where(live[None], lam[None] * phi(a), 0.0).sum(axis=(1, 2))
        if not with_scale:
            return lw
        scale = np.where(live[None], lam[None] * (np.exp(a) + 1.0 + np.abs(a) + 0.5 * a * a), 0.0).sum(axis=(1, 2))
    return lw, scale


def log_ratio_ess(lw):
    """(log mean_s w_s, (sum w)^2 / sum w^2) of log weights [S], max-shifted, the draws in index order; every weight zero: (-inf, 0)"""
    lw = np.asarray(lw, dtype=np.float64)
    m = float(np.max(lw))
    if m == -np.inf:
        return -np.inf, 0.0
    s1 = s2 = 0.0
    for v in lw:
        e = float(np.exp(v - m))
        s1 += e
        s2 += e * e
    return m + float(np.log(s1 / lw.size)), s1 * s1 / s2


def log_ratio_se(lw):
    """standard error of log mean_s w_s by the delta method: std(w) / (sqrt(S) mean(w))"""
    w = np.exp(np.asarray(lw, dtype=np.float64) - np.max(lw))
    return float(np.std(w, ddof=1) / (np.sqrt(w.size) * np.mean(w)))


def small_masks(R, q, T, seed=0):
    """(R, q, T) booleans, True = live: the eight patterns of the per-bin tests (test_cpu_observed_bins.pattern_masks) restated for shapes down to a
    few neurons and bins, in turn over the trials.  1 all live | 2 a seeded 20 % speckle | 3 neurons {0, 15, 16, q-1} x bins {0, 15, 16, 63, 64,
    T-1} dead (those that exist) | 4 neuron 3 (or the last) dead on the whole trial, neuron 17 (or the first) on bins [16, 32) (or the first half)
    | 5 every neuron dead on the second 64-bin block (T > 64), on [16, 32) (T > 32) or on the second half | 6 a single live entry, (17, 33) or
    the last that exists | 7 a checkerboard, (n + t) even live | 8 t < T/2 and n even live (what lengths plus 'observed' can express)."""
    n, t = np.arange(q)[:, None], np.arange(T)[None, :]
    rng = np.random.default_rng(seed + 1000 * q + T)
    n3, n17 = min(3, q - 1), (17 if q > 17 else 0)
    win = ((t >= 16) & (t < 32)) if T > 32 else (t >= T // 2)
    block = ((t >= 64) & (t < 128)) if T > 64 else win
    rows = [np.ones((q, T), bool), rng.random((q, T)) >= 0.2,
            ~(np.isin(n, [0, 15, 16, q - 1]) & np.isin(t, [0, 15, 16, 63, 64, T - 1])),
            ~((n == n3) | ((n == n17) & (win if T > 32 else (t < T // 2)))),
            np.broadcast_to(~block, (q, T)),
            (n == min(17, q - 1)) & (t == min(33, T - 1)), (n + t) % 2 == 0, (t < max(T // 2, 1)) & (n % 2 == 0)]
    live = np.stack([np.array(rows[r % 8]) for r in range(R)])
    assert live.any(axis=(1, 2)).all()
    return live


# ---- 1. the restatement is the dense definition ---------------------------------------------------------------------------------------------------
def _polished_mode(ybar, Cb, db, K_bigInv, n):
    """Newton on the oracle's big-matrix objective from zero, backtracking on the objective, until the step is below 1e-12"""
    x = np.zeros(n)
    f = orc.nlp_big(x, ybar, Cb, db, K_bigInv)
    for _ in range(100):
        g = orc.nlp_big_grad(x, ybar, Cb, db, K_bigInv)
        step = -np.linalg.solve(orc.nlp_big_hess(x, ybar, Cb, db, K_bigInv), g)
        a = 1.0
        while a > 1e-10:
            fn = orc.nlp_big(x + a * step, ybar, Cb, db, K_bigInv)
            if np.isfinite(fn) and fn <= f + 1e-12 * (1.0 + abs(f)):
                break
            a *= 0.5
        x, f = x + a * step, fn
        if a * np.max(np.abs(step)) < 1e-12:
            break
    return x


def _identity_case(tag, live, S=16):
    g = load_golden('c1_dataset.npz')
    C, d, tau = g['init_C'].astype(np.float64), g['init_d'].astype(np.float64).reshape(-1), g['init_tau']
    Y = g['Y'][0].astype(np.float64)
    q, T = Y.shape
    p = C.shape[1]
    n = p * T
    live = np.ones((q, T), bool) if live is None else live
    K_bigInv = orc.make_K_big(np.linalg.inv(orc.make_K(tau, T, float(g['binSize']))))
    C_big, d_big = orc.make_Cd_big(C, d, T)
    keep = live.reshape(-1)                                    # column n T + t: the oracle on the model with the dead entries deleted
    Cb, db, yb = C_big[:, keep], d_big[keep], Y.reshape(-1)[keep]
    f = lambda x: orc.nlp_big(x, yb, Cb, db, K_bigInv)
    xs = _polished_mode(yb, Cb, db, K_bigInv, n)
    grad = orc.nlp_big_grad(xs, yb, Cb, db, K_bigInv)
    H = orc.nlp_big_hess(xs, yb, Cb, db, K_bigInv)
    H = 0.5 * (H + H.T)
    L = np.linalg.cholesky(H)
    logdet = 2.0 * float(np.log(np.diag(L)).sum())
    rng = np.random.default_rng(11)
    delta = np.linalg.solve(L.T, rng.standard_normal((n, S))).T            # delta_s ~ N(0, H^-1)
    lw = log_weights(C, d, xs.reshape(p, T), (xs[None] + delta).reshape(S, p, T), live)
    log_z = -f(xs) - 0.5 * logdet + 0.5 * n * np.log(2.0 * np.pi)           # Laplace: exp(-f(x*)) (2 pi)^(n/2) det(H)^(-1/2)
    g1 = float(np.abs(grad).sum())
    worst = 0.0
    for s in range(S):
        fx = f(xs + delta[s])
        log_joint = -fx                                                      # log p(y, x_s), the reference's normalisation
        log_gauss = -0.5 * float(delta[s] @ H @ delta[s]) + 0.5 * logdet - 0.5 * n * np.log(2.0 * np.pi)
        gap = abs(log_joint - log_gauss - log_z - lw[s])
        bound = g1 * float(np.max(np.abs(delta[s]))) + 1e-9 * max(1.0, abs(fx))
        worst = max(worst, gap / bound)
        assert gap <= bound, (tag, s, gap, bound)
    lr, ess = log_ratio_ess(lw)
    print('%s: |g|_1 = %.2e, %d draws, log w in [%.3f, %.3f], worst gap / bound %.2e; log_ratio %.4f, ess %.1f of %d'
          % (tag, g1, S, lw.min(), lw.max(), worst, lr, ess, S))
    assert 1.0 <= ess <= S + 1e-9 and np.all(np.isfinite(lw))


def test_identity_against_the_oracle_at_config_1():
    _identity_case('config 1, all live', None)


def test_identity_against_the_oracle_under_an_entry_mask():
    g = load_golden('c1_dataset.npz')
    q, T = g['Y'][0].shape
    live = np.random.default_rng(7).random((q, T)) >= 0.2
    live[4, 10:40] = False
    live[:, 90:] = False                                        # (a ragged end)
    live[9] = False                                             # (an unobserved row)
    _identity_case('config 1, 20 % speckle + window + ragged end + dead row', live)


def test_restatement_edge_cases():
    rng = np.random.default_rng(3)
    q, p, T, S = 5, 2, 6, 4
    C, d, xs = rng.standard_normal((q, p)), rng.standard_normal(q), rng.standard_normal((p, T))
    X = xs[None] + 0.3 * rng.standard_normal((S, p, T))
    live = rng.random((q, T)) > 0.3
    live[2] = False
    lw = log_weights(C, d, xs, X, live)
    C2, d2 = C.copy(), d.copy()
    C2[2], d2[2] = 1e300, 1e300                                 # a dead row: whatever it holds, exactly 0
    assert np.array_equal(log_weights(C2, d2, xs, X, live), lw)
    assert np.array_equal(log_weights(C, d, xs, xs[None], live), np.zeros(1))          # the mode itself has weight 1
    Xo = X.copy()
    Xo[1] += 1e4                                                # an overflowing e^a: weight 0, no NaN
    lwo = log_weights(C, d, xs, Xo, np.ones((q, T), bool))
    assert lwo[1] == -np.inf and np.isfinite(lwo[[0, 2, 3]]).all()
    lr, ess = log_ratio_ess(lwo)
    assert np.isfinite(lr) and 1.0 <= ess <= 3.0 + 1e-12
    assert log_ratio_ess(np.full(3, -np.inf)) == (-np.inf, 0.0)
    lr1, ess1 = log_ratio_ess(lw[:1])
    assert lr1 == lw[0] and ess1 == 1.0
    a = np.array([-1e-3, 1e-3, 0.5, -0.5])
    assert np.allclose(phi(a), a ** 3 / 6 + a ** 4 / 24 + a ** 5 / 120 + a ** 6 / 720 + a ** 7 / 5040, rtol=1e-4, atol=0)
    m = small_masks(8, 7, 24)
    assert m.shape == (8, 7, 24) and m[5].sum() == 1 and m[0].all() and not m[3][3].any()


# ---- 2. interface ------------------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_python_layer_carry_the_entry_points():
    import ctypes as ct
    from funs import _hip, engine, util
    with open(os.path.join(ROOT, 'include', 'pgpfa.h')) as fh:
        header = fh.read()
    m = re.search(r'int pgpfa_importance_weights\((.*?)\);', header, flags=re.S)
    assert m, 'include/pgpfa.h does not declare pgpfa_importance_weights'
    args = re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S)
    names = [a.split()[-1].lstrip('*') for a in args.split(',')]
    assert names == ['ctx', 'n', 'idx', 'n_samples', 'seed', 'log_ratio', 'ess', 'log_w'], names
    assert 'unsigned long long seed' in args and args.count('double*') == 3
    dp = _hip.c_double_p
    assert _hip._SIGNATURES['pgpfa_importance_weights'] == [ct.c_void_p, ct.c_int, _hip.c_int32_p, ct.c_int, ct.c_ulonglong, dp, dp, dp]
    assert 'pgpfa_importance_weights' in _hip.EXPORTED_SYMBOLS
    sig = inspect.signature(_hip.Context.importance_weights)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[1:]] == [('idx', None), ('n_samples', 256), ('seed', 0), ('want', ('log_ratio', 'ess'))]
    sig = inspect.signature(util.importanceEvidence)
    assert list(sig.parameters) == ['params', 'experiment', 'infRes', 'trials', 'nSamples', 'seed', 'want']
    assert sig.parameters['nSamples'].default == 256 and sig.parameters['want'].default == ('logEvidence', 'ess')
    assert callable(engine.PPGPFAfit.importanceEvidence)
    assert inspect.signature(util.crossValidation.__init__).parameters['importance'].default is None
    assert 'logWeights' in util._SAMPLE_KEYS
    if os.path.exists(_hip.LIB_PATH):
        assert hasattr(_hip.load_library(), 'pgpfa_importance_weights')
