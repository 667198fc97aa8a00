"""Host side of the joint posterior samples (pgpfa_posterior_sample), without a GPU:

* the numpy restatement of the two square roots the device applies to standard normals - the dense one, M = L^-T with H = L L^T, and the low-rank
  one, M = [sqrt(eps) chol(G) | G F L^-T] - satisfies M M^T = Sigma against a plain dense inverse; the GPU tests import
  these functions as their yardstick;
* what util.posteriorSamples does around the device call (argument checks, trial list, cutting ragged trials) on a fake session;
* header, binding and built library agree on the new entry point, option key and info key."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, Experiment
from oracle import pgpfa_oracle as orc

BIN_MS = 10.0
SHAPES = [(7, 3, 24), (18, 10, 40), (9, 12, 20), (12, 20, 17)]           # (q, p, T): the shapes of the GPU tests


# ---- the yardstick -------------------------------------------------------------------------------------------------------------------------------
def problem(shape, seed=0, R=3, d_offset=-1.0):
    """parameters, counts [R][q][T] and smooth trajectories [R][p][T] at a shape; timescales of 6 - 15 bins, so that the low-rank system stays
    well below p T rows"""
    q, p, T = shape
    rng = np.random.default_rng(100 * q + 10 * p + T + seed)
    C = rng.standard_normal((q, p)) / np.sqrt(p)
    d = np.full(q, d_offset) + 0.3 * rng.standard_normal(q)
    tau = np.linspace(0.06, 0.15, p)
    K = orc.make_K(tau, T, BIN_MS)
    X = np.stack([np.stack([np.linalg.cholesky(K[k]) @ rng.standard_normal(T) for k in range(p)]) for _ in range(R)])
    Y = rng.poisson(np.exp(np.einsum('nk,rkt->rnt', C, X) + d[None, :, None]))
    return {'C': C, 'd': d, 'tau': tau}, Y, X


def curvature_blocks(X, C, d, length=None):
    """W[t] = C^T diag(exp(d + C x_t)) C of the Laplace posterior at X (p, T); zero behind `length` (padded bins carry no likelihood term)"""
    W = orc.poisson_blocks(np.asarray(X, dtype=np.float64), np.asarray(C, dtype=np.float64), np.asarray(d, dtype=np.float64).reshape(-1))
    if length is not None:
        W[int(length):] = 0.0
    return W


def dense_precision(W, tau, T, binSize):
    """H[(k,t),(l,s)] = [t == s] W[t][k][l] + [k == l] K_k^-1[t][s], latent-major (orc.nlp_hess with the blocks given)"""
    p = W.shape[1]
    Kinv = np.linalg.inv(orc.make_K(tau, T, binSize))
    H = np.zeros((p, T, p, T))
    ar = np.arange(T)
    for k in range(p):
        H[k, :, k, :] += Kinv[k]
        for l in range(p):
            H[k, ar, l, ar] += W[:, k, l]
    return H.reshape(p * T, p * T)


def sqrt_dense(H):
    """M (n x n) with x = m + M z: H = L L^T, M = L^-T.  (np.linalg.inv leaves K^-1, and so H, unsymmetric in the last digits and the factorization
    reads one triangle: the mean of the two is factored)"""
    L = np.linalg.cholesky(0.5 * (H + H.T))
    return np.linalg.solve(L, np.eye(H.shape[0])).T


def lowrank_factors(tau, T, binSize, eps=orc.EPS_NOISE, tol=1e-13):
    """F (p T x r, block diagonal, latent-major rows) with K_k = eps I + F_k F_k^T up to `tol` of the largest eigenvalue"""
    K = orc.make_K(tau, T, binSize, eps)
    blocks = []
    for k in range(K.shape[0]):
        lam, V = np.linalg.eigh(K[k] - eps * np.eye(T))
        keep = lam > tol * lam.max()
        blocks.append(V[:, keep] * np.sqrt(lam[keep]))
    r = sum(b.shape[1] for b in blocks)
    F = np.zeros((K.shape[0] * T, r))
    c0 = 0
    for k, b in enumerate(blocks):
        F[k * T:(k + 1) * T, c0:c0 + b.shape[1]] = b
        c0 += b.shape[1]
    return F


def scatter_bins(blocks):
    """[T][p][p] per-bin blocks -> (p T x p T), latent-major"""
    T, p, _ = blocks.shape
    out = np.zeros((p, T, p, T))
    ar = np.arange(T)
    for k in range(p):
        for l in range(p):
            out[k, ar, l, ar] = blocks[:, k, l]
    return out.reshape(p * T, p * T)


def sqrt_lowrank(W, F, eps=orc.EPS_NOISE):
    """M (n x (n + r)) = [sqrt(eps) chol(G) | G F L^-T] with G_t = (I + eps W_t)^-1, Wt = W G, B = I + F^T Wt F = L L^T: the draw is
    x = m + M [z1; z2], z1 latent-major"""
    T, p, _ = W.shape
    G = np.linalg.inv(np.eye(p)[None] + eps * W)
    G = 0.5 * (G + G.transpose(0, 2, 1))
    Rb = np.linalg.cholesky(G)
    Gf = scatter_bins(G)
    B = np.eye(F.shape[1]) + F.T @ (scatter_bins(W @ G) @ F)
    B = 0.5 * (B + B.T)
    L = np.linalg.cholesky(B)
    U = np.linalg.solve(L, np.eye(L.shape[0])).T
    return np.hstack([np.sqrt(eps) * scatter_bins(Rb), Gf @ (F @ U)])


@pytest.mark.parametrize('shape', [SHAPES[0], SHAPES[2]], ids=['q7-p3-T24', 'q9-p12-T20'])
def test_both_square_roots_reproduce_the_dense_inverse(shape):
    """M M^T against np.linalg.inv of the precision.  Dense: the precision is the oracle's Hessian.  Low-rank: the precision is K~^-1 + W with
    K~ = eps I + F F^T built from the same F, so the identity Sigma = eps G + G F B^-1 F^T G is checked exactly; against the oracle's own Hessian
    the truncation of F at 1e-13 of its largest eigenvalue adds at most cond(H) 1e-13.  Tolerance: an inverse or a triangular solve in FP64 is off by
    about cond(H) 2^-53 relative to its largest entry (Higham, Accuracy and Stability, ch. 14); both sides of each comparison carry one, and 8 cond(H)
    2^-53 leaves a factor of four for the dimension-dependent constant.  cond(H) is printed."""
    q, p, T = shape
    par, Y, X = problem(shape)
    W = curvature_blocks(X[0], par['C'], par['d'])
    H = dense_precision(W, par['tau'], T, BIN_MS)
    assert np.max(np.abs(H - orc.nlp_hess(X[0], None, par['C'], par['d'], np.linalg.inv(orc.make_K(par['tau'], T, BIN_MS))))) == 0.0
    Sigma = np.linalg.inv(0.5 * (H + H.T))
    M = sqrt_dense(H)
    e_dense = np.max(np.abs(M @ M.T - Sigma)) / np.max(np.abs(Sigma))
    F = lowrank_factors(par['tau'], T, BIN_MS)
    assert F.shape[1] < p * T
    Kt = orc.EPS_NOISE * np.eye(p * T) + F @ F.T
    Sigma_lr = np.linalg.inv(np.linalg.inv(Kt) + scatter_bins(W))
    M2 = sqrt_lowrank(W, F)
    assert M2.shape == (p * T, p * T + F.shape[1])
    e_lr = np.max(np.abs(M2 @ M2.T - Sigma_lr)) / np.max(np.abs(Sigma_lr))
    e_cross = np.max(np.abs(M2 @ M2.T - Sigma)) / np.max(np.abs(Sigma))
    tol = 8.0 * np.linalg.cond(H) * 2.0 ** -53
    print('cond(H) %.2e, tolerance %.2e' % (np.linalg.cond(H), tol))
    print('q=%d p=%d T=%d: dense root %.2e, low-rank root %.2e of its own precision (rank %d of %d), %.2e of the oracle Hessian' % (q, p, T, e_dense, e_lr, F.shape[1], p * T, e_cross))
    assert tol < 1e-8 and e_dense <= tol and e_lr <= tol and e_cross <= tol + np.linalg.cond(H) * 1e-13


def test_padded_bins_of_the_square_root_are_the_prior_conditional():
    """With W zero behind T_r the first T_r bins of the draw are those of the T_r-bin model: the leading block of Sigma equals the covariance of the
    truncated trial"""
    q, p, T = SHAPES[0]
    par, Y, X = problem(SHAPES[0])
    L = 17
    H = dense_precision(curvature_blocks(X[1], par['C'], par['d'], L), par['tau'], T, BIN_MS)
    M = sqrt_dense(H)
    S = (M @ M.T).reshape(p, T, p, T)[:, :L][:, :, :, :L].reshape(p * L, p * L)
    H_cut = dense_precision(curvature_blocks(X[1][:, :L], par['C'], par['d']), par['tau'], L, BIN_MS)
    S_cut = np.linalg.inv(0.5 * (H_cut + H_cut.T))
    assert np.max(np.abs(S - S_cut)) <= 8.0 * np.linalg.cond(H) * 2.0 ** -53 * np.max(np.abs(S_cut))           # (as in the test above)


# ---- header, binding, library ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def hip():
    import __graft_entry__ as ge
    ge.build()
    from funs import _hip
    return _hip


def test_header_binding_and_library_agree_on_the_new_entry_point(hip):
    lib = hip.load_library()
    header = open(os.path.join(ROOT, 'include', 'pgpfa.h')).read()
    assert re.search(r'int\s+pgpfa_posterior_sample\s*\(\s*pgpfa_ctx\s*\*\s*ctx\s*,\s*int\s+n\s*,\s*const\s+int32_t\s*\*\s*idx[\s\S]{0,80}?int\s+n_samples\s*,\s*unsigned\s+long\s+long\s+seed', header)
    assert 'pgpfa_posterior_sample' in hip.EXPORTED_SYMBOLS and hasattr(lib, 'pgpfa_posterior_sample')
    assert '"sample_chunk_trials"' in header and '"sample_noise_dim"' in header
    assert hasattr(hip.Context, 'posterior_sample')
    import __graft_entry__ as ge
    assert 'psample' in ge.UNITS
    from funs import engine, util
    assert callable(util.posteriorSamples) and callable(engine.PPGPFAfit.posteriorSamples)


# ---- util.posteriorSamples around a fake device ---------------------------------------------------------------------------------------------------------
class _FakeCtx:
    def __init__(self, q, p, T):
        self.q, self.p, self.T = q, p, T
        self.calls = []

    def posterior_sample(self, idx, n_samples=1, seed=0, noise=None, want=('x',)):
        self.calls.append((np.asarray(idx).tolist(), n_samples, seed, tuple(want)))
        n = len(idx)
        full = {'x': np.arange(n * n_samples * self.p * self.T, dtype=np.float64).reshape(n, n_samples, self.p, self.T),
                'y': np.ones((n, n_samples, self.q, self.T), dtype=np.uint16), 'count_sum': np.zeros((n, n_samples, self.q), dtype=np.int32),
                'noise': np.zeros((n, n_samples, self.p * self.T))}
        return {k: full[k] for k in want}


def _fake(monkeypatch, lens, T=8, q=3, p=2, comm_ready=False):
    from funs import _session
    R = len(lens)
    sess = object.__new__(_session.Session)
    sess.R, sess.q, sess.T, sess.p = R, q, T, p
    sess.lengths = None if all(v == T for v in lens) else np.asarray(lens, dtype=np.int32)
    sess.ctx = _FakeCtx(q, p, T)
    sess.post_stamp = sess.mode_stamp = 1
    sess.trial_stamp = np.ones(R, dtype=np.int64)
    sess.comm_ready = comm_ready
    monkeypatch.setattr(_session, 'session_for', lambda experiment, xdim: (sess, np.arange(R, dtype=np.int32)))
    exp = Experiment([np.zeros((q, L)) for L in lens], 20.0)
    params = {'C': np.zeros((q, p)), 'd': np.zeros(q), 'tau': np.full(p, 0.1)}
    return sess, exp, params, _session.DeviceInfRes(sess, np.arange(R, dtype=np.int32), (0, R))


def test_util_posterior_samples_passes_the_list_and_cuts_ragged_trials(monkeypatch):
    from funs import util
    sess, exp, params, res = _fake(monkeypatch, [8, 5, 8, 3])
    out = util.posteriorSamples(params, exp, infRes=res, trials=[3, 1, 1, 0], nSamples=6, seed=11, want=('x', 'y', 'count_sum'))
    assert sess.ctx.calls == [([3, 1, 1, 0], 6, 11, ('x', 'y', 'count_sum'))]
    assert sorted(out) == ['count_sum', 'x', 'y']
    assert [a.shape for a in out['x']] == [(6, 2, 3), (6, 2, 5), (6, 2, 5), (6, 2, 8)]
    assert [a.shape for a in out['y']] == [(6, 3, 3), (6, 3, 5), (6, 3, 5), (6, 3, 8)]
    assert out['count_sum'].shape == (4, 6, 3)
    full = sess.ctx.posterior_sample([3, 1, 1, 0], 6)['x']
    assert np.array_equal(out['x'][1], full[1][:, :, :5])
    sess2, exp2, params2, res2 = _fake(monkeypatch, [8, 8])
    out2 = util.posteriorSamples(params2, exp2, infRes=res2)                  # equal lengths: arrays, all trials, the defaults
    assert isinstance(out2['x'], np.ndarray) and out2['x'].shape == (2, 100, 2, 8) and sess2.ctx.calls[0][1:] == (100, 0, ('x',))


def test_util_posterior_samples_refuses_bad_arguments(monkeypatch):
    from funs import util
    sess, exp, params, res = _fake(monkeypatch, [8, 8, 8])
    with pytest.raises(ValueError, match='unknown key'):
        util.posteriorSamples(params, exp, infRes=res, want=('x', 'rate'))
    with pytest.raises(ValueError, match='nothing asked for'):
        util.posteriorSamples(params, exp, infRes=res, want=())
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError, match='nSamples'):
            util.posteriorSamples(params, exp, infRes=res, nSamples=bad)
    with pytest.raises(ValueError, match='empty trial list'):
        util.posteriorSamples(params, exp, infRes=res, trials=[])
    with pytest.raises(ValueError, match='not a device-backed result'):
        util.posteriorSamples(params, exp, infRes={'post_mean': []})
    sess.trial_stamp[1] = 2                                                   # a later E-step went over trial 1
    with pytest.raises(ValueError, match='superseded'):
        util.posteriorSamples(params, exp, infRes=res)
    assert sess.ctx.calls == []
    sess3, exp3, params3, res3 = _fake(monkeypatch, [8, 8], comm_ready=True)
    with pytest.raises(NotImplementedError, match='sharded'):
        util.posteriorSamples(params3, exp3, infRes=res3)
