"""E-step entry points with the reference's call surface (funs/inference.py of
mackelab/poisson-gpfa), executed by hand-written HIP kernels on MI355X.

    laplace(experiment, params, prevOptimRes=None, returnOptimRes=True, verbose=False,
            optimMethod='Newton-CG')                         # reference inference.py:67-185
    negLogPosteriorUnNorm / _grad / _hess                     # reference inference.py:12-65

The three callbacks keep the reference's positional signature (xbar, ybar, C_big, d_big,
K_bigInv, xdim, ydim) but are also offered in the structured form the device evaluates
(`laplace_objective`), because the Kronecker "big" matrices are never formed here.
"""
import numpy as np

from . import _hip
from ._session import DeviceDualOptimRes, DeviceInfRes, DeviceOptimRes, log_live, session_for

# covariance engine of every context this module creates: None = the library's choice (low-rank when it pays), 1 = dense, 2 = low-rank
# (tests pin one or the other; results agree to the low-rank tolerance)
COV_MODE = None

STATUS_TEXT = {0: 'converged', 1: 'iteration limit reached', 2: 'line search failed', 3: 'Hessian not positive definite',
               4: 'left unfinished by the shared-preconditioner iteration'}


class LaplaceConvergenceWarning(RuntimeWarning):
    """Some trials stopped at the Newton iteration limit: their modes are the last iterates, not converged ones."""


def _check_newton_status(status, first_trial=0, sess=None):
    """The reference ignores scipy's Newton-CG status (inference.py:127-129) - its failures are merely imprecise modes.
    Here status 2 / 3 mean that no acceptable step exists or that the posterior precision is not positive definite at
    the iterate (NaN / overflowing rates): such a trial's mode and covariance blocks are not a posterior and must not
    be summed into the M-step statistics, so they raise; the iteration limit (1) only warns.

    With trials sharded over ranks the verdict is COLLECTIVE: every rank contributes (failed, slow, first failing global
    trial) to one all-reduce and then all ranks raise (or warn) together with the same message - a rank that left on its
    own would leave the others blocked in the next collective."""
    status = np.asarray(status)
    bad = np.flatnonzero((status == 2) | (status == 3) | (status == 4))
    slow = np.flatnonzero(status == 1)
    size = sess.size if sess is not None else 1
    rank = sess.rank if sess is not None else 0
    # slots [0, size): first failing trial + 1 of each rank (0: none); [size, 2 size): its status; then the counts; same for `slow`
    msg = np.zeros(3 * size + 2)
    if bad.size:
        msg[rank] = first_trial + int(bad[0]) + 1
        msg[size + rank] = int(status[bad[0]])
    if slow.size:
        msg[2 * size + rank] = first_trial + int(slow[0]) + 1
    msg[3 * size] = bad.size
    msg[3 * size + 1] = slow.size
    if sess is not None and size > 1:
        msg = np.asarray(sess.allreduce(msg))
    n_bad, n_slow = int(round(msg[3 * size])), int(round(msg[3 * size + 1]))
    if n_bad:
        owner = int(np.flatnonzero(msg[:size] > 0)[0])
        first = int(round(msg[owner])) - 1
        raise _hip.HipBackendError('Laplace mode search failed for %d trial(s), first: trial %d%s (%s); parameters probably '
                                   'give non-finite rates' % (n_bad, first, ' on rank %d' % owner if size > 1 else '',
                                                              STATUS_TEXT.get(int(round(msg[size + owner])), '?')))
    if n_slow:
        import warnings
        owner = int(np.flatnonzero(msg[2 * size:3 * size] > 0)[0])
        warnings.warn('Laplace mode search hit the iteration limit for %d trial(s), first: trial %d; their modes are not '
                      'converged' % (n_slow, int(round(msg[2 * size + owner])) - 1), LaplaceConvergenceWarning, stacklevel=3)


def _prepare(experiment, params):
    C = np.asarray(params['C'], dtype=np.float64)
    ydim, xdim = C.shape
    # the reference flattens tau in place inside util.makeK_big (util.py:602); keep that side effect
    params['tau'] = np.ndarray.flatten(np.asarray(params['tau'], dtype=np.float64))
    sess, trial_idx = session_for(experiment, xdim)
    if sess.q != ydim:
        raise ValueError("params['C'] has %d rows but the experiment has %d neurons" % (ydim, sess.q))
    if COV_MODE is not None:
        sess.ctx.set_option('cov_mode', COV_MODE)
    sess.set_params(params)
    return sess, trial_idx


def laplace(experiment, params, prevOptimRes=None, returnOptimRes=True, verbose=False, optimMethod='Newton-CG'):
    """Laplace approximation of every trial's latent posterior (reference inference.py:67-185).

    Returns (infRes, -mean objective at the modes[, lapOptimRes]) exactly like the reference.  The
    mode search is a batched inexact Newton iteration on the GPU (shared-preconditioner PCG),
    run until the predicted error of the mode is below 1e-9 (far tighter than the reference's scipy Newton-CG
    stop, xtol=1e-5 on the mean |step|); `optimMethod` is accepted for signature compatibility only.  infRes
    entries are lazy device-backed sequences; 'post_cov' and 'post_vsmGP' are rebuilt on access.
    prevOptimRes: the previous call's lapOptimRes (or host arrays) as in the reference; additionally the string
    'resident' starts every trial from the mode an earlier E-step left on the device, if any (minibatch EM).
    Trials may differ in length (experiment.data[r]['Y'] of shape (ydim, T_r)): entries of trial r then have T_r bins, lapOptimRes[r]
    xdim*T_r values, and bins past T_r carry no likelihood term on the device.
    Neurons may be unobserved on some trials (experiment.data[r]['observed'], an optional boolean (ydim,)): trial r's posterior is then that of
    the model with only its observed rows of C, d and Y; the values of 'Y' in unobserved rows are ignored (NaN is accepted there).
    Single entries may be missing (experiment.data[r]['observedBins'], an optional boolean (ydim, T_r), True = recorded; ANDed with the other
    two): an entry that is not recorded carries no likelihood term, its value in 'Y' is ignored (NaN is accepted there).
    """
    sess, trial_idx = _prepare(experiment, params)
    sess.ctx.set_option('laplace_f32', int(LAPLACE_F32))      # (True is 1; LAPLACE_F32 is defined next to DUAL_F32 below)
    evidence = bool(LAPLACE_EVIDENCE)
    sess.ctx.set_option('laplace_evidence', int(evidence))
    n_all = len(trial_idx)
    # default: every rank holds the same experiment and takes a contiguous slice of its trials;
    # experiment._pgpfa_local_shard = True says this rank's experiment already IS its shard
    local_shard = bool(getattr(experiment, '_pgpfa_local_shard', False))
    lo, hi = (0, n_all) if local_shard else sess.local_slice(n_all)
    mine = trial_idx[lo:hi]
    warm = False
    if isinstance(prevOptimRes, str):
        if prevOptimRes != 'resident':
            raise ValueError("prevOptimRes: expected a sequence of modes or 'resident'")
        warm = 'resident'
    elif prevOptimRes is not None:
        resident = (isinstance(prevOptimRes, DeviceOptimRes) and prevOptimRes.session is sess
                    and prevOptimRes.stamp == sess.mode_stamp and np.array_equal(prevOptimRes.trial_idx, mine))
        if not resident:
            if len(prevOptimRes) == n_all:
                X = sess.pad_modes(mine, [prevOptimRes[i] for i in range(lo, hi)])
            elif len(prevOptimRes) == len(mine):
                X = sess.pad_modes(mine, list(prevOptimRes))
            else:
                raise ValueError('prevOptimRes has %d entries for %d trials' % (len(prevOptimRes), n_all))
            if len(mine):
                sess.ctx.set_modes(mine, X)
        warm = True
    if len(mine):
        obj, iters, status = sess.ctx.estep_laplace(mine, warm_start=warm)
    else:
        obj, iters, status = 0.0, np.zeros(0, np.int32), np.zeros(0, np.int32)
    sess.mark_written(mine)
    _check_newton_status(status, lo, sess)
    if verbose:
        for i, (it, st) in enumerate(zip(iters, status)):
            print('laplace inference trajectory of trial %d: %d Newton factorizations, %s' % (lo + i + 1, it, STATUS_TEXT.get(int(st), '?')))
    log_z = sess.ctx.log_evidence(mine) if (evidence and len(mine)) else np.zeros(0)
    # (the evidence rides in the all-reduce of the objective: one collective per E-step either way)
    tot = sess.allreduce(np.array([obj, float(len(mine))] + ([float(np.sum(log_z))] if evidence else [])))
    post_lik = tot[0] / tot[1]
    infRes = DeviceInfRes(sess, mine, (lo, hi))
    infRes.newton_iters = iters
    infRes.newton_status = status
    # LAPLACE_EVIDENCE: log Z_r of this rank's trials in the order of infRes, and the mean over the trials of all ranks; None while it is off
    infRes.log_evidence = log_z if evidence else None
    infRes.mean_log_evidence = float(tot[2] / tot[1]) if evidence else None
    if returnOptimRes:
        return infRes, -post_lik, DeviceOptimRes(sess, mine)
    return infRes, -post_lik


# ------------------------------------------------------------------------------------------------
# callbacks (reference inference.py:12-65) - structured form
# ------------------------------------------------------------------------------------------------
def laplace_objective(experiment, params, X, trials=None, grad=True):
    """negLogPosteriorUnNorm (and _grad) at latent trajectories X[n][xdim][T] for the given trials."""
    sess, trial_idx = _prepare(experiment, params)
    idx = trial_idx if trials is None else trial_idx[np.asarray(trials)]
    return sess.ctx.laplace_eval(idx, X, want_grad=grad)


def laplace_hessian(experiment, params, X, trial=0):
    """negLogPosteriorUnNorm_hess for one trial: dense (xdim*T, xdim*T), latent-major."""
    sess, trial_idx = _prepare(experiment, params)
    return sess.ctx.laplace_hessian(int(trial_idx[trial]), X)


# ------------------------------------------------------------------------------------------------
# callbacks by the reference's names and positional signatures (inference.py:12-65, 188-256)
# ------------------------------------------------------------------------------------------------
# The reference's callers hand these functions the Kronecker "big" matrices (mcmc.py:25, util.py:319-326).  The device
# never forms them: the small factors they were built from are read back out of their structure - C[n][k] =
# C_big[k*T][n*T], d[n] = d_big[n*T] (util.py:594-597); K_big / K_bigInv are block diagonal with one RBF Gram matrix
# (or its inverse) per latent, whose timescale in bins and noise level follow from two entries of a block
# (util.py:599-619) - and checked against the matrices handed in; anything that is not such a structure raises.
_BIG_CACHE = []          # [(C_big, d_big, Kmat, which, ybar bytes, ctx)] most recent first; arrays held so that ids stay valid
_BIG_CACHE_MAX = 4


def _unkron(C_big, d_big, ydim):
    C_big = np.asarray(C_big, dtype=np.float64)
    d_big = np.ndarray.flatten(np.asarray(d_big, dtype=np.float64))
    T = int(len(d_big) // ydim)
    if T < 1 or len(d_big) != ydim * T or C_big.ndim != 2 or C_big.shape[1] != ydim * T or C_big.shape[0] % T:
        raise ValueError('C_big / d_big do not have the shapes of util.makeCd_big (xdim*T, ydim*T) / (ydim*T,)')
    xdim = C_big.shape[0] // T
    C = np.ascontiguousarray(C_big[::T, ::T].T)                      # (ydim, xdim)
    d = np.ascontiguousarray(d_big[::T])
    # check of the Kronecker structure: every entry when the matrix is small (up to 2^22 entries), else a 4096-entry spot check (the
    # full comparison would cost as much as the product the device avoids) - a C_big that deviates from kron(C, I) in a few entries
    # (a masked neuron, time-varying loadings) can slip through the spot check and is then evaluated as the structured model
    rng = np.random.RandomState(0)
    if C_big.size <= (1 << 22):
        rows, cols = np.divmod(np.arange(C_big.size), C_big.shape[1])
    else:
        rows, cols = rng.randint(0, C_big.shape[0], 4096), rng.randint(0, C_big.shape[1], 4096)
    want = np.where(rows % T == cols % T, C[cols // T, rows // T], 0.0)
    if not np.allclose(C_big[rows, cols], want, rtol=0, atol=1e-12 * (1.0 + np.abs(C).max())) or \
            not np.allclose(d_big.reshape(ydim, T), d[:, None], rtol=0, atol=1e-12 * (1.0 + np.abs(d).max())):
        raise ValueError('C_big / d_big are not Kronecker expansions of (C, d) (util.makeCd_big); only that structure is evaluated')
    return C, d, xdim, T


def _rbf_params(Kmat, xdim, T, inverse):
    """(tau in bins, eps) per latent from the diagonal blocks of K_big (or K_bigInv), validated entry by entry."""
    Kmat = np.asarray(Kmat, dtype=np.float64)
    if Kmat.shape != (xdim * T, xdim * T):
        raise ValueError('K_big / K_bigInv must be (xdim*T, xdim*T)')
    taus, epss = [], []
    lag2 = (np.arange(T)[:, None] - np.arange(T)[None, :]) ** 2
    for k in range(xdim):
        blk = Kmat[k * T:(k + 1) * T, k * T:(k + 1) * T]
        K = np.linalg.inv(blk) if inverse else blk
        k1 = K[0, 1] if T > 1 else 0.999
        k2 = K[0, 2] if T > 2 else 0.0
        if k1 > 1e-200 and k2 > 1e-200 and k2 < k1:
            gamma = (np.log(k1) - np.log(k2)) / 1.5
            one_m_eps = np.exp(np.log(k1) + 0.5 * gamma)
        else:                                          # very short timescale: the second lag underflows; reference noise level
            one_m_eps = 0.999
            gamma = -2.0 * np.log(max(k1, 1e-300) / one_m_eps) if k1 > 0 else 1e3
        if abs((1.0 - one_m_eps) - 1e-3) < 1e-7:
            one_m_eps = 0.999                          # the reference's constant (util.py:599): drop the rounding of the read-back
        # refine gamma over all usable lags of the first row (entries read back from an inverse carry ~cond * 1e-16 of noise;
        # lag j determines gamma with that noise divided by j^2)
        row = K[0, 1:]
        lags = np.arange(1, T, dtype=np.float64)
        use = row > 1e-3
        if np.count_nonzero(use) >= 1:
            est = -2.0 * (np.log(row[use]) - np.log(one_m_eps)) / lags[use] ** 2
            w = (row[use] * lags[use] ** 2) ** 2
            gamma = float(np.sum(w * est) / np.sum(w))
        eps = 1.0 - one_m_eps
        model = one_m_eps * np.exp(-0.5 * gamma * lag2) + eps * np.eye(T)
        scale = np.abs(K).max()
        if not (gamma > 0 and 0 < eps < 1) or not np.allclose(K, model, rtol=0, atol=1e-6 * scale):
            raise ValueError('block %d of K_big%s is not an RBF Gram matrix of util.makeK_big; only that structure is evaluated'
                             % (k, 'Inv' if inverse else ''))
        taus.append(1.0 / np.sqrt(gamma))
        epss.append(eps)
    off = Kmat.copy()
    for k in range(xdim):
        off[k * T:(k + 1) * T, k * T:(k + 1) * T] = 0.0
    if np.abs(off).max() > 1e-9 * np.abs(Kmat).max():
        raise ValueError('K_big%s is not block diagonal over latents' % ('Inv' if inverse else ''))
    if max(epss) - min(epss) > 1e-6:
        raise ValueError('latents with different noise levels are not supported')
    return np.asarray(taus), float(np.mean(epss))


def _fingerprint(C_big, d_big, Kmat, T):
    """Cheap content key of the big matrices, O(q p + p T): the entries the small factors are read from (every T-th row / column
    of C_big and d_big, the first row of every diagonal block of K_big).  A caller that refills preallocated big matrices in
    place between EM iterations keeps their identity but not this key."""
    C_big, d_big, Kmat = np.asarray(C_big), np.asarray(d_big), np.asarray(Kmat)
    n = Kmat.shape[0]
    rows = [Kmat[k, k:min(k + T, n)] for k in range(0, n, T)]
    return (C_big[::T, ::T].tobytes(), np.ndarray.flatten(d_big)[::T].tobytes(), np.concatenate(rows).tobytes())


def _big_context(ybar, C_big, d_big, Kmat, ydim, inverse):
    """One-trial device context for the big-matrix callbacks, cached on the identity of the matrices AND a content
    fingerprint of the entries the small factors are recovered from."""
    ybar = np.ndarray.flatten(np.asarray(ybar, dtype=np.float64))
    for i, ent in enumerate(_BIG_CACHE):
        if ent[0] is C_big and ent[1] is d_big and ent[2] is Kmat and ent[3] == inverse:
            if ent[6] != _fingerprint(C_big, d_big, Kmat, ent[5].T):
                _BIG_CACHE.pop(i)[5].close()               # refilled in place: rebuild below
                break
            if ent[4] != ybar.tobytes():
                ent[5].upload_counts(ybar.reshape(1, ent[5].q, ent[5].T))
                ent[4] = ybar.tobytes()
            if i:
                _BIG_CACHE.insert(0, _BIG_CACHE.pop(i))
            return ent[5]
    C, d, xdim, T = _unkron(C_big, d_big, ydim)
    tau_bins, eps = _rbf_params(Kmat, xdim, T, inverse)
    if len(ybar) != ydim * T:
        raise ValueError('ybar must have ydim*T entries')
    bin_ms = 10.0
    ctx = _hip.Context(ydim, xdim, T, 1, bin_ms)
    ctx.set_option('eps_noise', eps)
    if COV_MODE is not None:
        ctx.set_option('cov_mode', COV_MODE)
    ctx.upload_counts(ybar.reshape(1, ydim, T))
    ctx.set_params(C, d, tau_bins * bin_ms / 1000.0)
    _BIG_CACHE.insert(0, [C_big, d_big, Kmat, inverse, ybar.tobytes(), ctx, _fingerprint(C_big, d_big, Kmat, T)])
    while len(_BIG_CACHE) > _BIG_CACHE_MAX:
        _BIG_CACHE.pop()[5].close()
    return ctx


def negLogPosteriorUnNorm(xbar, ybar, C_big, d_big, K_bigInv, xdim, ydim):
    """reference inference.py:12-32, evaluated on the device in structured form."""
    ctx = _big_context(ybar, C_big, d_big, K_bigInv, ydim, True)
    f, _ = ctx.laplace_eval(np.zeros(1, np.int32), np.ndarray.flatten(np.asarray(xbar, dtype=np.float64))[None, :], want_grad=False)
    return float(f[0])


def negLogPosteriorUnNorm_grad(xbar, ybar, C_big, d_big, K_bigInv, xdim, ydim):
    """reference inference.py:34-48"""
    ctx = _big_context(ybar, C_big, d_big, K_bigInv, ydim, True)
    _, g = ctx.laplace_eval(np.zeros(1, np.int32), np.ndarray.flatten(np.asarray(xbar, dtype=np.float64))[None, :], want_grad=True)
    return g.reshape(-1)


def negLogPosteriorUnNorm_hess(xbar, ybar, C_big, d_big, K_bigInv, xdim, ydim):
    """reference inference.py:50-65: dense (xdim*T, xdim*T)"""
    ctx = _big_context(ybar, C_big, d_big, K_bigInv, ydim, True)
    return ctx.laplace_hessian(0, np.ndarray.flatten(np.asarray(xbar, dtype=np.float64)))


def _infer_T(C_big):
    """T from the Kronecker structure of C_big = kron(C, I_T).T: entry (k*T+t, n*T+t') is non-zero only for t == t', so T
    divides column - row of every non-zero entry (the dual callbacks do not receive xdim / ydim).  A loading matrix with exact
    zeros can make the gcd a multiple of T; _unkron's structure check then rejects the matrices (pass dense loadings, or use
    the structured entry points, which take T explicitly)."""
    C_big = np.asarray(C_big)
    rows = np.unique(np.linspace(0, C_big.shape[0] - 1, 8).astype(int))
    g = 0
    for r in rows:
        nz = np.flatnonzero(C_big[r])
        if len(nz):
            g = int(np.gcd.reduce(np.append(np.abs(nz - r), g)))
    T = g if g > 0 else C_big.shape[1]
    if C_big.shape[0] % T or C_big.shape[1] % T:
        raise ValueError('C_big is not a Kronecker expansion of util.makeCd_big')
    return T


_ZERO_D = {}


def _zero_d_big(m):
    """stand-in d_big (same object every time, so that the context cache hits) for callbacks that do not take one"""
    if m not in _ZERO_D:
        _ZERO_D[m] = np.zeros(m)
    return _ZERO_D[m]


def _dual_ctx(ybar, C_big, K_big, d_big):
    m = np.asarray(C_big).shape[1]
    return _big_context(ybar, C_big, d_big, K_big, m // _infer_T(C_big), False)


def VIPostCov(K_bigInv, C_big, lamb):
    """reference inference.py:188-191 -> (postCovariance, postPrecision), dense; the covariance carries the reference's
    1e-6 relative jitter on the diagonal of the precision."""
    m = np.asarray(C_big).shape[1]
    ctx = _big_context(np.zeros(m), C_big, _zero_d_big(m), K_bigInv, m // _infer_T(C_big), True)
    return ctx.dual_post_cov(0, lamb, want_prec=True)


def VIPostMean(K_big, C_big, y_bar, lamb):
    """reference inference.py:193-194: -K_big C_big (lamb - y_bar)"""
    m = np.asarray(C_big).shape[1]
    ctx = _big_context(y_bar, C_big, _zero_d_big(m), K_big, m // _infer_T(C_big), False)
    return ctx.dual_post_mean(0, lamb)


def dualProblem(lamb, ybar, C_big, K_big, K_bigInv, d_big):
    """reference inference.py:196-213"""
    ctx = _dual_ctx(ybar, C_big, K_big, d_big)
    return ctx.dual_costgrad(0, lamb, want_grad=False)[0]


def dualProblem_grad(lamb, ybar, C_big, K_big, K_bigInv, d_big):
    """reference inference.py:215-219"""
    ctx = _dual_ctx(ybar, C_big, K_big, d_big)
    return ctx.dual_costgrad(0, lamb, want_grad=True)[1]


def dualProblemRho(rho, ybar, C_big, K_big, K_bigInv, d_big):
    """reference inference.py:222-247"""
    return dualProblem(np.exp(np.asarray(rho, dtype=np.float64)), ybar, C_big, K_big, K_bigInv, d_big)


def dualProblemRho_grad(rho, ybar, C_big, K_big, K_bigInv, d_big):
    """reference inference.py:249-256"""
    lam = np.exp(np.asarray(rho, dtype=np.float64))
    return dualProblem_grad(lam, ybar, C_big, K_big, K_bigInv, d_big) * lam


# 'device': the dual optimisations of all trials run as lockstep L-BFGS on the GPU (pgpfa_dual_lbfgs); 'scipy': the
# reference's per-trial scipy L-BFGS-B calls (same options), driven concurrently with batched device evaluations;
# 'fixedpoint': the optimum of the same dual through the fixed point of its stationarity conditions (pgpfa_dual_fixed_point: the Laplace
# Newton-PCG with variance offsets in a loop with the covariance blocks) - the zero of the reference's dual gradient to DUAL_FP_TOL
# in a handful of passes, where either L-BFGS stops on its decrease test after thousands of evaluations
DUAL_SOLVER = 'fixedpoint'
# passes / tolerance of DUAL_SOLVER = 'fixedpoint' (the tolerance is the max-norm of the reference's dual gradient at the returned lambda IN THE
# ARITHMETIC OF THE EVALUATION: with DUAL_F32 the covariance blocks behind the offsets carry single-precision rounding, and the same lambda
# evaluated in FP64 has a gradient of ~1e-7 (config 5, 256 trials: 1.2e-7) - the tests hold the mixed run to 1e-5, the FP64 run to 1e-6)
DUAL_FP_MAX_PASSES = 40
DUAL_FP_TOL = 1e-8
# evaluate the dual through the low-rank covariance engine when that pays (large xdim*T); the reference's 1e-6 diagonal jitter
# (inference.py:190) enters as a diagonal addition to the per-bin curvature blocks, so both engines evaluate the reference's function
DUAL_LOWRANK = True
# with DUAL_LOWRANK: factorisation of the r x r system, its inverse and the Yt product of every dual evaluation in single precision
# on the FP32 matrix cores, log det / covariance blocks / gradient accumulated in FP64 (BASELINE config 5 asks for fp32)
DUAL_F32 = False
# Laplace E-step under the low-rank covariance engine: the r x r system B = I + F^T Wt F of every trial, its Cholesky factor and L^-T in single
# precision on the FP32 matrix cores (C-ABI option laplace_f32).  L^-T is widened to FP64 right behind the inverse and everything after it - the
# Yt product, the mixing pass, the sums over trials, post_vsm / post_vsmGP / PautoSum - is the FP64 arithmetic of the default path; the mode
# search and the objective are not touched (bit-identical).  False / 0: off; True / 1: B assembled in FP32 from single-precision factors;
# 2: B assembled in FP64 and rounded once.  Measured error of the covariance outputs against dense FP64: docs/history/laplace_f32.md.  A chunk
# whose single-precision factorisation meets a non-positive pivot is redone in FP64 (info key last_cov_f32_fallbacks).  The dense engine
# ignores the flag; laplace() sends it on every call, dualVariational always runs its own covariance passes without it.
LAPLACE_F32 = False
# Laplace approximation of every trial's log evidence, log Z_r = -f_r(x*_r) - 1/2 (log det H_r(x*_r) + sum_k log det K_k) in the reference's
# normalisation (sum log y! dropped), computed next to the covariance blocks of the E-step (C-ABI option laplace_evidence).
# True: laplace() returns it as infRes.log_evidence (this rank's trials) and infRes.mean_log_evidence (mean over all ranks' trials); False:
# both are None and the E-step is the default one, bit for bit.  Not available together with LAPLACE_F32 (the call fails).  laplace() sends it
# on every call; engine.PPGPFAfit(trackEvidence=True) and util.crossValidation(score='evidence') switch it on around their own E-steps.
LAPLACE_EVIDENCE = False
# dualVariational on trials of unequal length (experiment.data[r]['Y'] of shape (ydim, T_r)) and / or with neurons unobserved on some trials
# (experiment.data[r]['observed']) - C-ABI option dual_masked, sent on every call.  False: such experiments are refused, as every pgpfa_dual_*
# entry point refuses them.  True: every trial's optimum, cost, posterior mean and covariance are those of the reference's functions on the trial's
# reduced problem (unobserved rows of Y, C, d deleted, bins cut to T_r), jitter included; varOptimRes entries keep their
# padded (ydim*T,) layout with zeros at entries without a likelihood term, and are accepted back as prevOptimRes.  Without a table the flag
# changes nothing, bit for bit.
DUAL_MASKED = False


class _ConcurrentProblems:
    """n independent optimisations, one Python thread each, whose cost/gradient requests are gathered into one batched
    device evaluation per round.  Every optimiser sees exactly the call sequence it would see running alone."""

    def __init__(self, n, evaluate_batch):
        import threading
        self._threading = threading
        self.n = n
        self.evaluate_batch = evaluate_batch          # (positions, [x...]) -> [(cost, grad)...]
        self.cond = threading.Condition()
        self.pending, self.results = {}, {}
        self.active = set(range(n))
        self.generation = 0
        self.error = None
        self.rounds = 0

    def _flush(self):                                 # lock held by the caller
        which = sorted(self.pending)
        try:
            res = self.evaluate_batch(which, [self.pending[i] for i in which])
            self.results = dict(zip(which, res))
        except Exception as exc:                      # hand the failure to every waiting optimiser
            self.error = exc
            self.results = {}
        self.pending = {}
        self.rounds += 1
        self.generation += 1
        self.cond.notify_all()

    def request(self, idx, x):
        with self.cond:
            self.pending[idx] = x
            gen = self.generation
            if len(self.pending) == len(self.active):
                self._flush()
            else:
                while self.generation == gen:
                    self.cond.wait()
            if self.error is not None:
                raise self.error
            return self.results[idx]

    def run(self, solve_one):
        out = [None] * self.n

        def worker(idx):
            try:
                out[idx] = solve_one(idx, lambda x: self.request(idx, x))
            except Exception as exc:
                out[idx] = exc
            finally:
                with self.cond:
                    self.active.discard(idx)
                    if self.pending and len(self.pending) == len(self.active):
                        self._flush()
        import sys
        threads = [self._threading.Thread(target=worker, args=(i,)) for i in range(self.n)]
        # many runnable threads hand the interpreter lock around once per switch interval (5 ms by default): with dozens of
        # optimisers that, not the device, would set the time of a round
        interval = sys.getswitchinterval()
        sys.setswitchinterval(1e-4)
        try:
            for t in threads:
                t.start()
            for t in threads:
                t.join()
        finally:
            sys.setswitchinterval(interval)
        for r in out:
            if isinstance(r, Exception):
                raise r
        return out


def dualVariational(experiment, params, optimizeLogLambda=False, prevOptimRes=None, returnOptimRes=True, verbose=False):
    """Dual variational E-step (reference inference.py:259-432).

    Per trial the dual objective over lambda in R^{ydim*T} (inference.py:196-219; log-lambda variant
    :222-256) is minimised by the same scipy L-BFGS-B calls as the reference (bounds lambda >= 1e-10,
    factr=1e7, start 0.5; or unbounded in rho = log lambda from 0); every cost/gradient evaluation runs on
    the GPU in structured form: W_t = C^T diag(lambda_t) C, one Cholesky of the (xdim*T)^2 precision for the
    log-determinant, its inverse's per-bin blocks for c_n^T Sigma_t c_n - C_big and diag(lambda) are never formed.
    Returns (infRes, -mean negLogPosterior at the VI means, mean dual optimum[, varOptimRes]).
    With DUAL_MASKED set, trials may differ in length and neurons may be unobserved on some trials, as in laplace(): infRes entries of trial r have
    T_r bins, and varOptimRes[r] stays a padded (ydim*T,) array (T: the longest trial) with zeros at entries without a likelihood term.
    """
    import scipy.optimize as op
    sess, trial_idx = _prepare(experiment, params)
    masked = bool(DUAL_MASKED)
    sess.refuse_tables('dualVariational', allow=('lengths', 'observed'))     # (a per-bin table is outside DUAL_MASKED too)
    if not masked:
        sess.refuse_tables('dualVariational')
    sess.ctx.set_option('dual_masked', int(masked))
    n_all = len(trial_idx)
    local_shard = bool(getattr(experiment, '_pgpfa_local_shard', False))
    lo, hi = (0, n_all) if local_shard else sess.local_slice(n_all)
    mine = trial_idx[lo:hi]
    m = sess.q * sess.T
    ctx = sess.ctx
    # DUAL_MASKED with a table set: which entries of the padded dual variables have a likelihood term (None: all).  The device ignores whatever
    # the others hold on input and keeps lambda = 0 there; on the host they are 0 in lambda and in rho
    live = sess.live_mask(mine) if masked else None
    # DUAL_LOWRANK: the dual is evaluated through the low-rank covariance engine when that pays (large xdim*T), with the
    # reference's 1e-6 diagonal jitter (inference.py:190) carried by the per-bin blocks; otherwise the dense engine
    ctx.set_option('dual_lowrank', 1 if DUAL_LOWRANK else 0)
    ctx.set_option('dual_f32', 1 if (DUAL_SOLVER in ('device', 'fixedpoint') and DUAL_LOWRANK and DUAL_F32) else 0)
    ctx.set_option('laplace_f32', 0)                           # pgpfa_dual_finalize's blocks stay FP64 whatever LAPLACE_F32 says
    if DUAL_SOLVER in ('device', 'fixedpoint') and len(mine):
        # on the device, in rho = log(lambda); same optimum as either of the reference's variants
        def prev_rho():
            prev = np.stack([np.asarray(prevOptimRes[j] if len(prevOptimRes) == len(mine) else prevOptimRes[lo + j], dtype=np.float64)
                             for j in range(len(mine))])
            if live is not None:
                return np.where(live, prev if optimizeLogLambda else np.log(np.maximum(prev, 1e-300)), 0.0)
            return prev if optimizeLogLambda else np.log(np.maximum(prev, 1e-300))
        lam_all = None
        if DUAL_SOLVER == 'fixedpoint':
            # the optimum through the variance fixed point (pgpfa_dual_fixed_point): a handful of covariance passes per trial; a trial
            # whose map does not contract (log-rate variances of order one) or that runs out of passes goes to L-BFGS from where it stopped.
            # Cold start: the reference's lambda = 0.5 (inference.py:302) - rho = 0 of the log-lambda variant is lambda = 1: both are starts of
            # one strictly convex problem and the fixed point lands on its optimum from either.  exp / log of the q T entries run on the
            # device and the optimum stays there for the finalize call.
            # The optimum also stays on the device as the returned varOptimRes (a lazy list: an entry is downloaded when it is read), and handed
            # back as prevOptimRes of the next call it is a warm start that moves no bytes.
            resident = (isinstance(prevOptimRes, DeviceDualOptimRes) and prevOptimRes.session is sess and prevOptimRes.stamp == sess.mode_stamp
                        and np.array_equal(prevOptimRes.trial_idx, mine))
            res = ctx.dual_fixed_point(mine, None if (prevOptimRes is None or resident) else prev_rho(), max_outer=DUAL_FP_MAX_PASSES, tol=DUAL_FP_TOL,
                                       warm=prevOptimRes is not None, resident=resident, want_rho=False)
            fopt, iters, vstat = res[1:4]
            fp_status = np.array(vstat, copy=True)           # (before the handed-back trials are finished below)
            bad = np.nonzero(vstat != 0)[0]
            if len(bad):
                # (rare: bring the whole optimum to the host, finish the handed-back trials there, finalize from the host copy)
                lam_all = ctx.dual_lambda(mine)
                rho_b, fopt_b, it_b = ctx.dual_lbfgs(mine[bad], log_live(lam_all[bad]))
                lam_all[bad], fopt[bad] = (np.exp(rho_b) if live is None else np.where(live[bad], np.exp(rho_b), 0.0)), fopt_b
                iters[bad] += it_b
            nlp = ctx.dual_finalize(mine, lam_all)           # (None: the optimum the fixed point left on the device)
            sess.mark_written(mine)
            sess.mark_dual_written(mine)
            optim = DeviceDualOptimRes(sess, mine, optimizeLogLambda)
            tot = sess.allreduce(np.array([nlp, float(np.sum(fopt)), float(len(mine))]))
            infRes = DeviceInfRes(sess, mine, (lo, hi))
            infRes.dual_iterations = iters
            # status of the fixed point per trial: 0 converged, 1 pass cap, 2 not contracting (1 and 2 were finished by L-BFGS above)
            infRes.dual_status = fp_status
            if returnOptimRes:
                return infRes, -tot[0] / tot[2], tot[1] / tot[2], optim
            return infRes, -tot[0] / tot[2], tot[1] / tot[2]
        else:
            if prevOptimRes is None:
                rho0 = np.zeros((len(mine), m)) if optimizeLogLambda else np.full((len(mine), m), np.log(0.5))
            else:
                rho0 = prev_rho()
            if live is not None:
                rho0 = np.where(live, rho0, 0.0)                # (the lockstep L-BFGS never moves them: zero gradient)
            rho, fopt, iters = ctx.dual_lbfgs(mine, rho0)
            lam_all = np.exp(rho) if live is None else np.where(live, np.exp(rho), 0.0)
            optim = list(rho) if optimizeLogLambda else list(lam_all)
            nlp = ctx.dual_finalize(mine, lam_all)
        sess.mark_written(mine)
        sess.mark_dual_written(mine)
        tot = sess.allreduce(np.array([nlp, float(np.sum(fopt)), float(len(mine))]))
        infRes = DeviceInfRes(sess, mine, (lo, hi))
        infRes.dual_iterations = iters
        if returnOptimRes:
            return infRes, -tot[0] / tot[2], tot[1] / tot[2], optim
        return infRes, -tot[0] / tot[2], tot[1] / tot[2]
    # DUAL_SOLVER == 'scipy':
    # The reference solves the trials one after the other (inference.py:300-397), each with its own scipy L-BFGS-B run.
    # Here every trial still gets exactly that run (same calls, same options, same start), but the runs execute
    # concurrently - one Python thread per trial - and each round of their cost/gradient requests is served by ONE
    # batched device evaluation (pgpfa_dual_costgrad_batch), instead of one dense factorisation at a time.
    starts = []
    for j in range(len(mine)):
        if prevOptimRes is None:
            starts.append(np.zeros(m) if optimizeLogLambda else np.zeros(m) + 0.5)
        else:
            starts.append(np.asarray(prevOptimRes[j] if len(prevOptimRes) == len(mine) else prevOptimRes[lo + j], dtype=np.float64))

    def evaluate_batch(which, xs):
        """which: positions in `mine`; xs: their optimiser variables -> list of (cost, grad in the optimiser's variable)"""
        X = np.stack(xs)
        lam = np.exp(X) if optimizeLogLambda else X
        cost, grad = ctx.dual_costgrad_batch(mine[np.asarray(which)], lam)
        if optimizeLogLambda:
            grad = grad * lam
        return [(float(cost[i]), grad[i]) for i in range(len(which))]

    def solve_one(j, evaluate):
        if verbose:
            print('dual variational inference trajectory of trial %d...' % (lo + j + 1))
        cache = {}

        def cached(x):
            key = x.tobytes()
            if cache.get('k') != key:
                cache['k'], cache['v'] = key, evaluate(np.array(x, dtype=np.float64))
            return cache['v']
        if optimizeLogLambda:
            return op.fmin_l_bfgs_b(func=lambda x: cached(x)[0], x0=starts[j], fprime=lambda x: cached(x)[1], disp=False)
        return op.fmin_l_bfgs_b(func=lambda x: cached(x)[0], x0=starts[j], fprime=lambda x: cached(x)[1], approx_grad=False,
                                bounds=[(1e-10, None)] * m, factr=1e7, disp=False)

    outs = _ConcurrentProblems(len(mine), evaluate_batch).run(solve_one) if len(mine) else []
    if live is not None:
        # entries without a likelihood term kept their start value through the run (the device ignores them and returns a zero gradient there);
        # the returned varOptimRes holds 0 there, in lambda and in rho
        optim = [np.where(live[j], out[0], 0.0) for j, out in enumerate(outs)]
        lams = [np.where(live[j], np.exp(out[0]) if optimizeLogLambda else out[0], 0.0) for j, out in enumerate(outs)]
    else:
        optim = [out[0] for out in outs]
        lams = [np.exp(out[0]) if optimizeLogLambda else out[0] for out in outs]
    vlb = float(sum(out[1] for out in outs))
    nlp = ctx.dual_finalize(mine, np.stack(lams)) if len(mine) else 0.0
    sess.mark_written(mine)
    sess.mark_dual_written(mine)
    tot = sess.allreduce(np.array([nlp, vlb, float(len(mine))]))
    infRes = DeviceInfRes(sess, mine, (lo, hi))
    if returnOptimRes:
        return infRes, -tot[0] / tot[2], tot[1] / tot[2], optim
    return infRes, -tot[0] / tot[2], tot[1] / tot[2]
