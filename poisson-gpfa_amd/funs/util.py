"""Host utilities on either side of the hot path, with the names of the reference's funs/util.py:
vec layout helpers, the builders (Gram matrices come from the device kernel), trial subsampling with
the reference's RNG stream, the synthetic population generator and the Poisson-PCA initialiser.
Plotting, CRCNS/Matlab loaders and cross-validation helpers of the reference are outside the hot
path and are not provided."""
import copy
import sys

import numpy as np

from . import _hip


class Printer:
    """One-line progress output (reference util.py:121-128)."""

    def __init__(self, data):
        sys.stdout.write('\r\x1b[K' + str(data))
        sys.stdout.flush()

    @staticmethod
    def stdout(message):
        sys.stdout.write(message)
        sys.stdout.write('\b' * len(message))


# -- vec(C, d) layout (reference util.py:560-592) ----------------------------------------------------
def CdtoVecCd(C, d):
    C = np.asarray(C, dtype=np.float64)
    d = np.asarray(d, dtype=np.float64).reshape(-1)
    return np.concatenate((C.T.ravel(), d))


def vecCdtoCd(vecCd, xdim, ydim):
    m = np.asarray(vecCd, dtype=np.float64).reshape(xdim + 1, ydim)
    return m[:xdim].T, m[xdim]


# -- builders (reference util.py:594-619) ---------------------------------------------------------------
def makeCd_big(params, T):
    """Kronecker expansion of (C, d).  Only for small diagnostics: the device path never forms it."""
    C_big = np.kron(params['C'], np.eye(T)).T
    d_big = np.kron(np.ndarray.flatten(np.asarray(params['d'])), np.ones(T)).T
    return C_big, d_big


def makeK_big(params, trialDur, binSize, epsNoise=0.001):
    """Per-latent RBF Gram matrices K (xdim,T,T) from the device kernel, and their block-diagonal K_big."""
    ydim, xdim = np.shape(params['C'])
    params['tau'] = np.ndarray.flatten(np.asarray(params['tau'], dtype=np.float64))
    T = int(trialDur / binSize)
    ctx = _hip.Context(ydim, xdim, T, 1, float(binSize))
    try:
        ctx.set_option('eps_noise', epsNoise)
        ctx.set_params(np.asarray(params['C'], dtype=np.float64), np.zeros(ydim), params['tau'])
        K = ctx.gram()
    finally:
        ctx.close()
    K_big = np.zeros((xdim * T, xdim * T))
    for xd in range(xdim):
        K_big[xd * T:(xd + 1) * T, xd * T:(xd + 1) * T] = K[xd]
    return K_big, K


# -- finite-difference Jacobian (reference util.py:377-434) -------------------------------------------------
def approx_jacobian(x, func, epsilon, *args):
    """Jacobian of the vector function func at x by the reference's fourth-order central differences,
    J[:, i] = (-f(x+2h) + 8 f(x+h) - 8 f(x-h) + f(x-2h)) / (12 h_i), with its step rule: h = epsilon / 2 (a scalar epsilon for
    every coordinate) or, for epsilon None, EPS^(1/3) * max(|x|, 0.1) / 2 (statsmodels' _get_epsilon with s = 3)."""
    x0 = np.atleast_1d(np.asarray(x, dtype=np.float64))
    n = x0.size
    if epsilon is None:
        h = np.finfo(float).eps ** (1.0 / 3.0) * np.maximum(np.abs(x0), 0.1)
    elif np.isscalar(epsilon):
        h = np.full(n, float(epsilon))
    else:
        h = np.asarray(epsilon, dtype=np.float64)
    h = h / 2.0
    f0 = np.asarray(func(x0, *args))
    jac = np.zeros((f0.size, n))
    for i in range(n):
        dx = np.zeros(n)
        dx[i] = h[i]
        jac[:, i] = (-np.asarray(func(x0 + 2 * dx, *args)) + 8 * np.asarray(func(x0 + dx, *args))
                     - 8 * np.asarray(func(x0 - dx, *args)) + np.asarray(func(x0 - 2 * dx, *args))) / (12 * h[i])
    return jac


# -- leave-one-neuron-out prediction (reference util.py:289-334) --------------------------------------------
def leaveOneOutPrediction(params, experiment):
    """For every trial and neuron: posterior mode of the latents given all OTHER neurons, then the held-out neuron's
    predicted rate exp(c_n x + d_n) per bin.  Returns (y_pred_mode[numTrials][ydim][T], pred_err_mode) like the
    reference; the numTrials*ydim mode searches run batched on the device (the reference solves them one by one
    with fmin_ncg from a cold start, to a looser tolerance)."""
    from . import _session
    xdim = np.shape(params['C'])[1]
    sess, trial_idx = _session.session_for(experiment, xdim)
    sess.refuse_tables('leaveOneOutPrediction')
    lo, hi = (0, len(trial_idx)) if getattr(experiment, '_pgpfa_local_shard', False) else sess.local_slice(len(trial_idx))
    sess.set_params(params)
    y_loc, err_loc = sess.ctx.loo_predict(trial_idx[lo:hi])
    unconverged = int(sess.ctx.info('last_loo_unconverged'))
    if unconverged:
        import warnings
        warnings.warn('leaveOneOutPrediction: %d of %d held-out mode searches did not converge; their predictions come from '
                      'the last iterate' % (unconverged, (hi - lo) * sess.q), RuntimeWarning, stacklevel=2)
    if sess.comm_ready and not getattr(experiment, '_pgpfa_local_shard', False):
        y_pred = np.zeros((len(trial_idx), sess.q, sess.T))
        y_pred[lo:hi] = y_loc
        y_pred = sess.allreduce(y_pred)
        err = float(sess.allreduce(np.array([err_loc]))[0])
        return y_pred, err
    return y_loc, float(err_loc)


# -- posterior firing rates ---------------------------------------------------------------------------------
_RATE_KEYS = ('rate', 'lower', 'upper', 'median', 'eta', 'var', 'ell')


def _band_z(level):
    """z of the central credible band at `level`: P(|N(0,1)| <= z) = level."""
    from statistics import NormalDist
    level = float(level)
    if not 0.0 < level < 1.0:
        raise ValueError('level must lie strictly between 0 and 1, got %r' % (level,))
    return NormalDist().inv_cdf(0.5 * (1.0 + level))


def _condition_groups(conditions, n):
    """One integer label per listed trial -> (sorted distinct labels, group id 0..G-1 of every listed trial)."""
    lab = np.asarray(conditions)
    if lab.shape != (n,):
        raise ValueError('conditions: one label per listed trial expected (%d), got shape %s' % (n, lab.shape))
    if not np.issubdtype(lab.dtype, np.integer):
        if not np.all(lab == np.floor(lab)):
            raise ValueError('conditions must be integer labels')
        lab = lab.astype(np.int64)
    labels, group = np.unique(lab, return_inverse=True)
    return labels, group.reshape(-1).astype(np.int32)


def _cut_planes(sess, idx, arr, forecast):
    """Per-trial planes arr[n][ydim][T] of the session's trials idx as the caller sees them: each cut to the trial's own T_r bins unless
    `forecast`; one array when the shapes agree, else a list of (ydim, T_r) arrays (as orthonormalizeTrajectories returns x_tilde)."""
    if forecast or sess.lengths is None:
        return arr
    lens = [int(sess.lengths[int(t)]) for t in idx]
    if all(L == sess.T for L in lens):
        return arr
    out = [np.ascontiguousarray(arr[i][:, :L]) for i, L in enumerate(lens)]
    return np.stack(out) if len(set(lens)) == 1 else out


def _resident_posterior(what, params, experiment, infRes, trials, set_params):
    """The front end of the queries on a resident posterior (posteriorRates, posteriorSamples, posteriorAt = `what`): the experiment's session and the
    session's indices of the listed trials (positions in experiment.data; None: all; repeats allowed), once a posterior is resident for them.
    infRes None: one Laplace E-step at `params` over the experiment.  A DeviceInfRes of this session whose entries are still the resident ones: that
    posterior, with `params` set as the current parameters if `set_params`.  Anything else raises ValueError; a sharded session NotImplementedError."""
    from . import _session, inference
    sess, trial_idx = _session.session_for(experiment, np.shape(params['C'])[1])
    if sess.comm_ready:
        raise NotImplementedError('%s does not support sharded sessions: every rank holds the posterior of its own trials only' % what)
    pos = np.arange(len(trial_idx)) if trials is None else np.asarray(trials, dtype=np.int64).reshape(-1)
    idx = np.ascontiguousarray(trial_idx[pos], dtype=np.int32)
    if idx.size == 0:
        raise ValueError('empty trial list')
    if infRes is None:
        inference.laplace(experiment, copy.copy(params), returnOptimRes=False)
        return sess, idx
    if not isinstance(infRes, _session.DeviceInfRes) or infRes.session is not sess:
        raise ValueError("infRes is not a device-backed result of this experiment's session: pass infRes=None to run an E-step")
    covered = set(infRes.trial_idx.tolist())
    stale = [int(t) for t in idx if sess.trial_stamp[int(t)] != infRes.stamp or int(t) not in covered]
    if stale:
        raise ValueError('infRes is superseded (or never covered) for trial %d: a later E-step has overwritten its posterior on the device' % stale[0])
    if set_params:
        sess.set_params({'C': params['C'], 'd': params['d'], 'tau': np.ndarray.flatten(np.asarray(params['tau'], dtype=np.float64))})
    return sess, idx


def posteriorRates(params, experiment, infRes=None, trials=None, conditions=None, level=0.95, forecast=False, want=('rate', 'lower', 'upper')):
    """Denoised single-trial firing rates lambda_n(t) = exp(d_n + c_n . x_t) under the posterior of the latents, with a credible band, and
    their averages over the trials of every experimental condition.  The reference stops at the latent posterior; its only rate-like
    outputs are exp(C x + d) at a held-out mode (util.py:289-334) and a per-neuron scalar from the parameters.  Everything per (trial,
    neuron, bin) is computed on the device from the resident posterior (pgpfa_posterior_rates); post_vsm never comes to the host.

    infRes None: one Laplace E-step at `params` over the experiment first.  A DeviceInfRes of this experiment's session whose entries are
    still the resident ones (inference.laplace, dualVariational): that posterior, with `params` set as the parameters.  Anything else -
    superseded by a later E-step, of another session, host arrays - raises ValueError.
    trials: positions in experiment.data (None: all; repeats allowed).  conditions: one integer label per listed trial.
    want: any of 'rate' (posterior mean exp(eta + var/2)), 'lower' / 'upper' (the central `level` band exp(eta -+ z sqrt(var))), 'median'
    (exp(eta)) - all four in spikes per SECOND -, 'eta' / 'var' (posterior mean and variance of the log rate per bin) and 'ell' ([n][ydim]:
    expected Poisson log likelihood sum_t y eta - rate, without sum log y!; NaN where the neuron was not observed on the trial - the planes cover
    all neurons there: an unobserved neuron's rate is the model's prediction from the observed ones).  Per-trial entries are [n][ydim][T]; with trials of unequal
    length each is cut to its T_r bins - a list of (ydim, T_r) arrays - unless forecast=True, which keeps all T bins: behind T_r the
    posterior is the GP's prediction from the trial's own bins.  With `conditions` the dict also holds 'condition_mean' [G][ydim][T] in
    spikes per second (the mean over the condition's trials that have the bin; NaN where none has), 'condition_count' [G][T] and
    'condition_labels' [G]; with want=() only these come back and no per-trial plane leaves the device.
    Under a per-bin table (experiment.data[r]['observedBins']) the planes and the condition averages cover every entry - an entry that was not
    recorded gets the model's prediction - and 'ell' raises ValueError: the resident counts at such entries are placeholders."""
    from . import _session
    want = tuple(want)
    unknown = [k for k in want if k not in _RATE_KEYS]
    if unknown:
        raise ValueError('want: unknown key(s) %s; known: %s' % (unknown, list(_RATE_KEYS)))
    z = _band_z(level)
    if 'ell' in want and getattr(_session.session_for(experiment, np.shape(params['C'])[1])[0], 'observed_bins', None) is not None:
        raise ValueError("want: 'ell' is not available under a per-bin table ('observedBins'): the resident counts at entries that were not "
                         'recorded are placeholders')
    sess, idx = _resident_posterior('posteriorRates', params, experiment, infRes, trials, set_params=True)
    planes = any(k in want for k in ('rate', 'lower', 'upper', 'median', 'eta', 'var'))
    ask = (['eta', 'var'] if planes else []) + (['ell'] if 'ell' in want else [])
    group, labels = None, None
    if conditions is not None:
        labels, group = _condition_groups(conditions, idx.size)
        ask += ['group_sum', 'group_count']
    if not ask:
        raise ValueError('nothing asked for: want is empty and there are no conditions')
    dev = sess.ctx.posterior_rates(idx, group=group, n_groups=0 if labels is None else len(labels), want=ask)
    per_s = 1000.0 / float(experiment.binSize)
    out = {}
    if planes:
        eta, var = dev['eta'], dev['var']
        sd = np.sqrt(var) if ('lower' in want or 'upper' in want) else None
        made = {'eta': lambda: eta, 'var': lambda: var, 'median': lambda: np.exp(eta) * per_s, 'rate': lambda: np.exp(eta + 0.5 * var) * per_s,
                'lower': lambda: np.exp(eta - z * sd) * per_s, 'upper': lambda: np.exp(eta + z * sd) * per_s}
        for k in want:
            if k in made:
                out[k] = _cut_planes(sess, idx, made[k](), forecast)
    if 'ell' in want:
        out['ell'] = dev['ell']
        observed = getattr(sess, 'observed', None)
        if observed is not None:                       # no counts, no likelihood: an unobserved (trial, neuron) pair has no ell
            out['ell'] = np.where(observed[idx], out['ell'], np.nan)
    if labels is not None:
        cnt = dev['group_count']
        with np.errstate(invalid='ignore', divide='ignore'):
            out['condition_mean'] = np.where(cnt[:, None, :] > 0, dev['group_sum'] / cnt[:, None, :], np.nan) * per_s
        out['condition_count'] = cnt
        out['condition_labels'] = labels
    return out


# -- posterior-predictive spike counts -------------------------------------------------------------------------
_COUNT_KEYS = ('logp', 'pmf', 'lower', 'upper', 'mean', 'var', 'saturated')
_COUNT_DEVICE = {'logp': 'logp', 'pmf': 'pmf', 'lower': 'lower', 'upper': 'upper', 'mean': 'pmean', 'var': 'pvar', 'saturated': 'upper'}
MAX_COUNT = 65535                                          # largest count a bin can hold on the device (two byte planes)


def _listed_counts(counts, experiment, pos, ydim, T):
    """The caller's counts - one (ydim, T_r) array per listed trial - as one int32 (n, ydim, T) array, zeros behind T_r.  Shapes and values are
    checked against the experiment: no device is touched."""
    if len(counts) != len(pos):
        raise ValueError('counts: one (ydim, T_r) array per listed trial expected (%d trials, %d arrays)' % (len(pos), len(counts)))
    out = np.zeros((len(pos), ydim, T), dtype=np.int32)
    for i, (r, y) in enumerate(zip(pos, counts)):
        y = np.asarray(y)
        L = int(np.shape(experiment.data[int(r)]['Y'])[1])
        if y.shape != (ydim, L):
            raise ValueError('counts[%d] must have shape (ydim, T_r) = (%d, %d), got %s' % (i, ydim, L, y.shape))
        if not np.all((y >= 0) & (y <= MAX_COUNT) & (y == np.floor(y))):
            raise ValueError('counts[%d]: integers in 0..%d expected' % (i, MAX_COUNT))
        out[i, :, :L] = y
    return out


def posteriorCounts(params, experiment, infRes=None, trials=None, counts=None, maxCount=None, level=0.95, forecast=False, want=('logp',)):
    """What the fitted model predicts for the spike COUNT of every (trial, neuron, bin): with the log rate eta ~ N(eta, var) of posteriorRates the
    count is the Poisson-lognormal mixture P(y = k) = int Poisson(k; e^eta) N(eta; m, v) d eta - over-dispersed, variance mu + mu^2 (e^v - 1), and
    far from Poisson(mu) where the posterior is wide: held-out neurons, hidden entries, forecast bins.  The reference has no counterpart.  Computed
    on the device from the resident posterior (pgpfa_posterior_counts: a mode-centred Gauss-Hermite rule in FP64; eta and var never come to the host).

    infRes, trials: as posteriorRates.  counts: one (ydim, T_r) array of integers per listed trial - the counts 'logp' is taken at -, or None for
    the experiment's own.  maxCount: 'pmf' covers k = 0..maxCount (needed for 'pmf', at most 1023), and the walk of the band stops there (None:
    at 65535).  want: any of
      'logp'   log P(y) at the count of every entry; NaN where the experiment did not observe the neuron on the trial and counts is None,
      'pmf'    [n][ydim][T][maxCount + 1],
      'lower', 'upper'   the central `level` predictive interval in counts (integers): the smallest k with CDF(k) >= (1 -+ level) / 2; an entry
               whose upper quantile lies beyond maxCount gets maxCount,
      'saturated'   how many entries that happened to (an int; computes 'upper'),
      'mean', 'var'   mu = exp(eta + var / 2) and mu + mu^2 (e^var - 1): counts per BIN, not per second.
    Per-trial entries are [n][ydim][T]; with trials of unequal length each is cut to its T_r bins - a list - unless forecast=True, which keeps all T
    bins: behind T_r they carry the prediction from the trial's own bins, and 'logp' is NaN there.  Under a per-bin table ('observedBins') every
    entry gets a prediction; 'logp' with counts=None raises ValueError there (the resident counts at entries that were not recorded are placeholders)."""
    from . import _session
    want = tuple(want)
    unknown = [k for k in want if k not in _COUNT_KEYS]
    if unknown:
        raise ValueError('want: unknown key(s) %s; known: %s' % (unknown, list(_COUNT_KEYS)))
    if not want:
        raise ValueError('nothing asked for: want is empty')
    _band_z(level)                                       # (its check of level)
    if maxCount is not None and (int(maxCount) != maxCount or not 0 <= int(maxCount) <= MAX_COUNT):
        raise ValueError('maxCount must be an integer in 0..%d, got %r' % (MAX_COUNT, maxCount))
    if 'pmf' in want and (maxCount is None or int(maxCount) > 1023):
        raise ValueError("want: 'pmf' needs maxCount (at most 1023): it covers k = 0..maxCount")
    ydim = np.shape(params['C'])[0]
    pos = np.arange(len(experiment.data)) if trials is None else np.asarray(trials, dtype=np.int64).reshape(-1)
    T_all = max(int(np.shape(tr['Y'])[1]) for tr in experiment.data)
    given = None if counts is None else _listed_counts(counts, experiment, pos, ydim, T_all)      # (checked before any device call)
    if 'logp' in want and counts is None and getattr(_session.session_for(experiment, np.shape(params['C'])[1])[0], 'observed_bins', None) is not None:
        raise ValueError("want: 'logp' needs counts= under a per-bin table ('observedBins'): the resident counts at entries that were not "
                         'recorded are placeholders')
    sess, idx = _resident_posterior('posteriorCounts', params, experiment, infRes, trials, set_params=True)
    if given is not None and given.shape[2] != sess.T:
        given = _listed_counts(counts, experiment, pos, ydim, sess.T)
    ask = sorted({_COUNT_DEVICE[k] for k in want})
    K = 1 if maxCount is None else int(maxCount) + 1
    k_cap = MAX_COUNT if maxCount is None else int(maxCount)
    ragged = sess.lengths is not None
    if forecast and ragged:
        # behind T_r the library writes padding: the forecast goes through the moments, which cover all T bins
        mv = sess.ctx.posterior_rates(idx, group=None, n_groups=0, want=['eta', 'var'])
        at = given
        if 'logp' in want and at is None:
            at = _listed_counts([experiment.data[int(r)]['Y'] for r in pos], experiment, pos, ydim, sess.T)
        dev = sess.ctx.count_probabilities(mv['eta'], mv['var'], counts=at if 'logp' in want else None, K=K, level=level, k_cap=k_cap, want=ask)
        if 'logp' in dev:
            beyond = np.arange(sess.T)[None, :] >= sess.lengths[idx][:, None]
            dev['logp'] = np.where(beyond[:, None, :], np.nan, dev['logp'])
    else:
        dev = sess.ctx.posterior_counts(idx, counts=given if 'logp' in want else None, K=K, level=level, k_cap=k_cap, want=ask)
    saturated = int(sess.ctx.info('counts_saturated')) if 'upper' in ask else 0
    if 'logp' in dev and counts is None:
        observed = getattr(sess, 'observed', None)
        if observed is not None:                           # no counts, nothing to take the probability of
            dev['logp'] = np.where(observed[idx][:, :, None], dev['logp'], np.nan)
    out = {}
    for k in want:
        out[k] = saturated if k == 'saturated' else _cut_planes(sess, idx, dev[_COUNT_DEVICE[k]], forecast)
    return out


def _score_predictive(truth, logp, scored):
    """Bits per spike of the predictive distribution over single entries: truth, logp (log P(y) of the model at the true count) and scored are lists
    of (rows, T_r) arrays, one per trial.  Per row n: sum over its scored entries of log P(y) - log Poisson(y; lbar_n), lbar_n the mean count of row n
    over its scored entries as in _score_entries, both terms WITH - log y!; divided by log 2 times the spikes scored.  Returns (total, per row -
    NaN for a row without a scored spike)."""
    from math import lgamma
    rows = truth[0].shape[0]
    tot_y, tot_n = np.zeros(rows), np.zeros(rows)
    for y, sc in zip(truth, scored):
        tot_y += np.where(sc, y, 0.0).sum(axis=1)
        tot_n += sc.sum(axis=1)
    with np.errstate(invalid='ignore', divide='ignore'):
        lbar = np.where(tot_n > 0, tot_y / tot_n, 0.0)
    lfact = np.vectorize(lambda k: lgamma(k + 1.0), otypes=[np.float64])
    ll, spikes = np.zeros(rows), np.zeros(rows)
    for y, lp, sc in zip(truth, logp, scored):
        y = np.where(sc, y, 0.0)
        with np.errstate(invalid='ignore', divide='ignore'):
            null = np.where(y > 0, y * np.log(lbar)[:, None], 0.0) - lbar[:, None] - lfact(y)
        ll += np.where(sc, np.where(sc, lp, 0.0) - null, 0.0).sum(axis=1)
        spikes += y.sum(axis=1)
    with np.errstate(invalid='ignore', divide='ignore'):
        per_row = np.where(spikes > 0, ll / (np.log(2.0) * spikes), np.nan)
        total = float(ll.sum() / (np.log(2.0) * spikes.sum())) if spikes.sum() > 0 else float('nan')
    return total, per_row


def _predictive_keys(truth, logp, scored):
    """The keys predictive=True adds to the dict of coSmoothing / binHoldout"""
    total, per_row = _score_predictive(truth, logp, scored)
    return {'logPredictive': [np.where(sc, lp, np.nan) for lp, sc in zip(logp, scored)], 'bitsPerSpikePredictive': total,
            'bitsPerSpikePredictivePerNeuron': per_row}


_SAMPLE_KEYS = ('x', 'y', 'count_sum', 'noise', 'logWeights')


def posteriorSamples(params, experiment, infRes=None, trials=None, nSamples=100, seed=0, want=('x',)):
    """Joint draws of whole latent trajectories from the posterior of every listed trial, and posterior-predictive spike counts of every draw.
    The reference hands out the marginals of the posterior only; whatever depends on the joint uncertainty of a trajectory - a peak time, a
    path length, a band for a time-integrated rate, Fano factors of predicted counts, over-dispersed starts for funs.mcmc - needs draws.  They
    are made on the device from a square root of the posterior covariance the covariance pass builds anyway (pgpfa_posterior_sample); the
    (xdim T) x (xdim T) matrix is never formed.

    infRes None: one Laplace E-step at `params` over the experiment first.  A DeviceInfRes of this experiment's session whose entries are still
    the resident ones (inference.laplace, dualVariational): that posterior, under the parameters of the E-step that produced it.  Anything else
    raises ValueError.  trials: positions in experiment.data (None: all; repeats allowed - a repeated trial gets the same draws).
    want: any of 'x' [n][nSamples][xdim][T], 'y' [n][nSamples][ydim][T] (uint16: y ~ Poisson(exp(d + C x)) per bin), 'count_sum'
    [n][nSamples][ydim] (the counts of a draw summed over the trial's bins) and 'noise' (the standard normals used).  With trials of unequal
    length 'x' and 'y' are lists of arrays cut to each trial's own T_r bins.  Draw s of a trial is a pure function of (seed, trial, s).
    'logWeights' [n][nSamples] (Laplace posteriors only): the log importance weights of exactly these draws (importanceEvidence, same seed) -
    exp(logWeights), normalised per trial, re-weights any function of 'x' from the Laplace posterior to the true one."""
    want = tuple(want)
    unknown = [k for k in want if k not in _SAMPLE_KEYS]
    if unknown:
        raise ValueError('want: unknown key(s) %s; known: %s' % (unknown, list(_SAMPLE_KEYS)))
    if not want:
        raise ValueError('nothing asked for: want is empty')
    if int(nSamples) != nSamples or int(nSamples) < 1:
        raise ValueError('nSamples = %r: a count of draws per trial, at least 1' % (nSamples,))
    sess, idx = _resident_posterior('posteriorSamples', params, experiment, infRes, trials, set_params=False)
    dev = {}
    if any(k != 'logWeights' for k in want):
        dev = sess.ctx.posterior_sample(idx, n_samples=int(nSamples), seed=int(seed), want=tuple(k for k in want if k != 'logWeights'))
    if 'logWeights' in want:
        dev['logWeights'] = sess.ctx.importance_weights(idx, n_samples=int(nSamples), seed=int(seed), want=('log_w',))['log_w']
    out = {}
    for k in want:
        arr = dev[k]
        if k in ('x', 'y') and sess.lengths is not None:
            lens = [int(sess.lengths[int(t)]) for t in idx]
            if any(L != sess.T for L in lens):
                arr = [np.ascontiguousarray(arr[i][:, :, :L]) for i, L in enumerate(lens)]
        out[k] = arr
    return out


_AT_KEYS = ('mean', 'var', 'lower', 'upper', 'cov')


def _condition_means_at(mean, times, group, n_groups, spans):
    """Condition averages of per-trial trajectories on a common axis, on the host and in list order (so the result is reproducible):
    trial i enters group[i]'s average at query time s only where 0 <= s <= spans[i], its own recorded span.  mean: (n, xdim, S); times: (S,)
    or (n, S).  Returns (condition_mean (G, xdim, S) - 0 where no trial has the time -, condition_count (G, S))."""
    n, xdim, S = mean.shape
    tt = np.broadcast_to(times, (n, S))
    total = np.zeros((n_groups, xdim, S))
    count = np.zeros((n_groups, S), dtype=np.int32)
    for i in range(n):
        inside = (tt[i] >= 0.0) & (tt[i] <= spans[i])
        total[group[i]] += np.where(inside[None, :], mean[i], 0.0)
        count[group[i]] += inside
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(count[:, None, :] > 0, total / count[:, None, :], 0.0), count


def posteriorAt(params, experiment, times, infRes=None, trials=None, conditions=None, level=0.95, want=('mean', 'lower', 'upper')):
    """The latent trajectories of the listed trials at arbitrary time points, with a credible band: the GP posterior over the bin grid extended
    to any time by the prior conditional (pgpfa_posterior_at; the reference hands the posterior out on the grid only).  Three uses: a trajectory
    aligned to an event that falls at another time in every trial, a finely sampled trajectory for a figure, and condition means on a common axis
    over trials of unequal length.  post_vsmGP never comes to the host.

    times: ms from a trial's first bin (bin j sits at j * binSize), any finite values - before the first or beyond the last bin extrapolates, far
    away gives the prior (mean 0, variance 1).  A 1-D array is one grid for all listed trials; a 2-D (n, S) array gives every listed trial its own
    grid (event alignment: event_ms[r] + lags).
    infRes None: one Laplace E-step at `params` over the experiment first.  A DeviceInfRes of this experiment's session whose entries are still
    the resident ones: that posterior, evaluated under the timescales of the E-step that produced it.  Anything else raises ValueError.
    trials: positions in experiment.data (None: all; repeats allowed).  conditions: one integer label per listed trial.
    want: any of 'mean', 'var' (marginal posterior mean and variance of every latent), 'lower' / 'upper' (mean -+ z sqrt(var), the central
    `level` band) - (n, xdim, S) arrays - and 'cov', the joint (xdim, xdim) covariance of the latents at every time, (n, S, xdim, xdim)
    (pgpfa_posterior_cov_at; it needs a posterior an E-step of this session wrote).  Returns a dict of the asked keys plus 'times'; with
    `conditions` also 'condition_mean' (G, xdim, S) - the mean over the condition's trials of the posterior mean, a trial entering at s only
    inside its own recorded span 0 <= s <= (T_r - 1) binSize; 0 where no trial has the time -, 'condition_count' (G, S) and
    'condition_labels' (G)."""
    from . import _session, inference
    want = tuple(want)
    unknown = [k for k in want if k not in _AT_KEYS]
    if unknown:
        raise ValueError('want: unknown key(s) %s; known: %s' % (unknown, list(_AT_KEYS)))
    z = _band_z(level)
    tt = np.asarray(times, dtype=np.float64)
    tt = np.ascontiguousarray(tt) if tt.ndim else tt            # (ascontiguousarray would turn a scalar into a grid of one time)
    if tt.ndim not in (1, 2) or tt.shape[-1] < 1:
        raise ValueError('times: shape (S,) or (n, S) with S >= 1 expected, got %s' % (tt.shape,))
    if not np.all(np.isfinite(tt)):                    # (before the session is touched: nothing reaches the device)
        raise ValueError('times: entry %s is not finite' % (tuple(int(i) for i in np.argwhere(~np.isfinite(tt))[0]),))
    sess, idx = _resident_posterior('posteriorAt', params, experiment, infRes, trials, set_params=True)
    if tt.ndim == 2 and tt.shape[0] != idx.size:
        raise ValueError('times: one grid per listed trial expected, (%d, S), got %s' % (idx.size, tt.shape))
    labels, group = (None, None) if conditions is None else _condition_groups(conditions, idx.size)
    if not want and labels is None:
        raise ValueError('nothing asked for: want is empty and there are no conditions')
    need_var = any(k in want for k in ('var', 'lower', 'upper'))
    need_mean = labels is not None or any(k in want for k in ('mean', 'lower', 'upper'))
    dev = {}
    if need_mean or need_var:
        dev = sess.ctx.posterior_at(tt, idx, want=(('mean',) if need_mean else ()) + (('var',) if need_var else ()))
    if 'cov' in want:
        dev['cov'] = sess.ctx.posterior_cov_at(tt, idx, want=('cov',))['cov']
    out = {'times': tt}
    sd = np.sqrt(dev['var']) if ('lower' in want or 'upper' in want) else None
    made = {'mean': lambda: dev['mean'], 'var': lambda: dev['var'], 'lower': lambda: dev['mean'] - z * sd, 'upper': lambda: dev['mean'] + z * sd,
            'cov': lambda: dev['cov']}
    for k in want:
        out[k] = made[k]()
    if labels is not None:
        binSize = float(experiment.binSize)
        spans = [((sess.T if sess.lengths is None else int(sess.lengths[int(t)])) - 1) * binSize for t in idx]
        out['condition_mean'], out['condition_count'] = _condition_means_at(dev['mean'], tt, group, len(labels), spans)
        out['condition_labels'] = labels
    return out


_VEL_AT_KEYS = ('vel', 'var', 'lower', 'upper', 'value', 'value_var', 'cross', 'speed2')


def posteriorVelocityAt(params, experiment, times, infRes=None, trials=None, conditions=None, level=0.95, want=('vel', 'lower', 'upper')):
    """The time derivative of the latent trajectories of the listed trials at arbitrary time points, with a credible band, jointly with the value:
    phase portraits (x_k, xdot_k), speed profiles around an event, condition-averaged velocities on a common axis.  The GP gives the derivative
    exactly - xdot_k(s) is jointly Gaussian with the grid values under the prior - so nothing is differenced (pgpfa_posterior_velocity_at).  The
    velocity is that of the smooth component of the latent, in latent units per SECOND.

    times, infRes, trials, conditions: as for posteriorAt.
    want: any of 'vel', 'var' (posterior mean and variance of the velocity of every latent), 'lower' / 'upper' (vel -+ z sqrt(var), the central
    `level` band), 'value' / 'value_var' (mean and variance of the latent itself: the 'mean' / 'var' of posteriorAt), 'cross' (the posterior
    covariance of value and velocity of the same latent) - (n, xdim, S) arrays - and 'speed2' (n, S): sum_k (vel_k^2 + var_k), the posterior
    expectation of the squared speed in the model's latent coordinates.  Returns a dict of the asked keys plus 'times'; with `conditions` also
    'condition_mean' (G, xdim, S) - the mean of 'vel' over the condition's trials, a trial entering at s only inside its own recorded span -,
    'condition_count' (G, S) and 'condition_labels' (G).
    Not given: the covariance of the velocities ACROSS latents - hence velocities in orthonormalised coordinates and the variance of the speed -,
    derivatives of firing rates, sharded sessions."""
    want = tuple(want)
    unknown = [k for k in want if k not in _VEL_AT_KEYS]
    if unknown:
        raise ValueError('want: unknown key(s) %s; known: %s' % (unknown, list(_VEL_AT_KEYS)))
    z = _band_z(level)
    tt = np.asarray(times, dtype=np.float64)
    tt = np.ascontiguousarray(tt) if tt.ndim else tt
    if tt.ndim not in (1, 2) or tt.shape[-1] < 1:
        raise ValueError('times: shape (S,) or (n, S) with S >= 1 expected, got %s' % (tt.shape,))
    if not np.all(np.isfinite(tt)):                    # (before the session is touched: nothing reaches the device)
        raise ValueError('times: entry %s is not finite' % (tuple(int(i) for i in np.argwhere(~np.isfinite(tt))[0]),))
    if not want and conditions is None:
        raise ValueError('nothing asked for: want is empty and there are no conditions')
    sess, idx = _resident_posterior('posteriorVelocityAt', params, experiment, infRes, trials, set_params=True)
    if tt.ndim == 2 and tt.shape[0] != idx.size:
        raise ValueError('times: one grid per listed trial expected, (%d, S), got %s' % (idx.size, tt.shape))
    labels, group = (None, None) if conditions is None else _condition_groups(conditions, idx.size)
    needs = {'vel': labels is not None or any(k in want for k in ('vel', 'lower', 'upper', 'speed2')),
             'vel_var': any(k in want for k in ('var', 'lower', 'upper', 'speed2')),
             'mean': 'value' in want, 'var': 'value_var' in want, 'cross': 'cross' in want}
    dev = sess.ctx.posterior_velocity_at(tt, idx, want=tuple(k for k in ('mean', 'var', 'vel', 'vel_var', 'cross') if needs[k]))
    sd = np.sqrt(dev['vel_var']) if ('lower' in want or 'upper' in want) else None
    made = {'vel': lambda: dev['vel'], 'var': lambda: dev['vel_var'], 'lower': lambda: dev['vel'] - z * sd, 'upper': lambda: dev['vel'] + z * sd,
            'value': lambda: dev['mean'], 'value_var': lambda: dev['var'], 'cross': lambda: dev['cross'],
            'speed2': lambda: (dev['vel'] * dev['vel'] + dev['vel_var']).sum(axis=1)}
    out = {'times': tt}
    for k in want:
        out[k] = made[k]()
    if labels is not None:
        binSize = float(experiment.binSize)
        spans = [((sess.T if sess.lengths is None else int(sess.lengths[int(t)])) - 1) * binSize for t in idx]
        out['condition_mean'], out['condition_count'] = _condition_means_at(dev['vel'], tt, group, len(labels), spans)
        out['condition_labels'] = labels
    return out


_RATE_AT_KEYS = ('rate', 'lower', 'upper', 'median', 'eta', 'var')


def posteriorRatesAt(params, experiment, times, infRes=None, trials=None, conditions=None, level=0.95, want=('rate', 'lower', 'upper')):
    """Single-trial firing rates of the listed trials at arbitrary time points, with a credible band, and their condition averages on a common
    axis: posteriorRates off the bin grid.  The log rate of neuron n at time s is Gaussian with eta = d_n + c_n . mean(s) and var = c_n^T
    Cov(x(s)) c_n, where mean(s) and the joint covariance Cov(x(s)) of the latents are those of posteriorAt (pgpfa_posterior_cov_at); neither the
    covariance nor post_vsmGP comes to the host.

    times, infRes, trials, conditions: as for posteriorAt; the posterior has to be one an E-step of this session wrote, and C, d and the
    timescales are those of that E-step (restored around the call when the session has moved on).
    want: any of 'rate' (exp(eta + var/2)), 'lower' / 'upper' (the central `level` band exp(eta -+ z sqrt(var))), 'median' (exp(eta)) - in spikes
    per SECOND, the definitions of posteriorRates - and 'eta' / 'var'.  Returns a dict of the asked keys as (n, ydim, S) arrays plus 'times'; with
    `conditions` also 'condition_mean' (G, ydim, S) - the mean of 'rate' over the condition's trials, a trial entering at s only inside its own
    recorded span 0 <= s <= (T_r - 1) binSize; 0 where no trial has the time -, 'condition_count' (G, S) and 'condition_labels' (G)."""
    want = tuple(want)
    unknown = [k for k in want if k not in _RATE_AT_KEYS]
    if unknown:
        raise ValueError('want: unknown key(s) %s; known: %s' % (unknown, list(_RATE_AT_KEYS)))
    z = _band_z(level)
    tt = np.asarray(times, dtype=np.float64)
    tt = np.ascontiguousarray(tt) if tt.ndim else tt
    if tt.ndim not in (1, 2) or tt.shape[-1] < 1:
        raise ValueError('times: shape (S,) or (n, S) with S >= 1 expected, got %s' % (tt.shape,))
    if not np.all(np.isfinite(tt)):                    # (before the session is touched: nothing reaches the device)
        raise ValueError('times: entry %s is not finite' % (tuple(int(i) for i in np.argwhere(~np.isfinite(tt))[0]),))
    if not want and conditions is None:
        raise ValueError('nothing asked for: want is empty and there are no conditions')
    sess, idx = _resident_posterior('posteriorRatesAt', params, experiment, infRes, trials, set_params=True)
    if tt.ndim == 2 and tt.shape[0] != idx.size:
        raise ValueError('times: one grid per listed trial expected, (%d, S), got %s' % (idx.size, tt.shape))
    labels, group = (None, None) if conditions is None else _condition_groups(conditions, idx.size)
    dev = sess.ctx.posterior_cov_at(tt, idx, want=('eta', 'var'))
    eta, var = dev['eta'], dev['var']
    per_s = 1000.0 / float(experiment.binSize)
    sd = np.sqrt(var) if ('lower' in want or 'upper' in want) else None
    made = {'eta': lambda: eta, 'var': lambda: var, 'median': lambda: np.exp(eta) * per_s, 'rate': lambda: np.exp(eta + 0.5 * var) * per_s,
            'lower': lambda: np.exp(eta - z * sd) * per_s, 'upper': lambda: np.exp(eta + z * sd) * per_s}
    out = {'times': tt}
    for k in want:
        out[k] = made[k]()
    if labels is not None:
        binSize = float(experiment.binSize)
        spans = [((sess.T if sess.lengths is None else int(sess.lengths[int(t)])) - 1) * binSize for t in idx]
        rate = out['rate'] if 'rate' in out else made['rate']()
        out['condition_mean'], out['condition_count'] = _condition_means_at(rate, tt, group, len(labels), spans)
        out['condition_labels'] = labels
    return out


# -- linear functionals of the latents: epoch means, contrasts, projections ------------------------------------
_FUNC_KEYS = ('mean', 'var', 'sd', 'lower', 'upper', 'cov')


def posteriorFunctionals(params, experiment, weights, infRes=None, trials=None, level=0.95, want=('mean', 'lower', 'upper')):
    """The joint posterior of linear functionals u_j . x of the latents of the listed trials: the mean of a latent over an epoch, a contrast
    between two epochs, the projection of a whole trajectory onto a decoding axis or a temporal template.  Exact - no samples - and without the
    p T x p T covariance of a trial ever being formed (pgpfa_posterior_functionals): Cov(U^T x) = (M^T U)^T (M^T U) from the square root M the
    sampler draws from.

    weights: (J, xdim, T) - one set for all listed trials - or (n, J, xdim, T), one set per listed trial; T is the session's bin count (the
    longest trial).  Behind a shorter trial's own T_r bins the posterior is the GP's forecast, and weights there count it in.
    infRes, trials: as for posteriorAt; the posterior has to be one an E-step of this session wrote.
    want: any of 'mean', 'var', 'sd', 'lower' / 'upper' (mean -+ z sd, the central `level` band) - (n, J) arrays - and 'cov', the joint (n, J, J)
    covariance of the functionals (J <= 1024; without it J is not limited and no J x J plane is formed).  Returns a dict of the asked keys."""
    want = tuple(want)
    unknown = [k for k in want if k not in _FUNC_KEYS]
    if unknown:
        raise ValueError('want: unknown key(s) %s; known: %s' % (unknown, list(_FUNC_KEYS)))
    if not want:
        raise ValueError('nothing asked for: want is empty')
    z = _band_z(level)
    ww = np.ascontiguousarray(weights, dtype=np.float64)
    if ww.ndim not in (3, 4) or ww.shape[-3] < 1:
        raise ValueError('weights: shape (J, xdim, T) or (n, J, xdim, T) with J >= 1 expected, got %s' % (ww.shape,))
    if not np.all(np.isfinite(ww)):                    # (before the session is touched: nothing reaches the device)
        raise ValueError('weights: entry %s is not finite' % (tuple(int(i) for i in np.argwhere(~np.isfinite(ww))[0]),))
    sess, idx = _resident_posterior('posteriorFunctionals', params, experiment, infRes, trials, set_params=True)
    xdim = int(np.shape(params['C'])[1])
    if ww.shape[-2:] != (xdim, sess.T) or (ww.ndim == 4 and ww.shape[0] != idx.size):
        raise ValueError('weights: (J, %d, %d) or one set per listed trial, (%d, J, %d, %d), expected, got %s'
                         % (xdim, sess.T, idx.size, xdim, sess.T, ww.shape))
    return _functional_bands(sess.ctx, ww, idx, z, want)


def _functional_bands(ctx, ww, idx, z, want):
    """The asked keys of _FUNC_KEYS from one device call that asks for exactly what they need."""
    need_var = any(k in want for k in ('var', 'sd', 'lower', 'upper'))
    need_mean = any(k in want for k in ('mean', 'lower', 'upper'))
    ask = (('mean',) if need_mean else ()) + (('var',) if need_var else ()) + (('cov',) if 'cov' in want else ())
    dev = ctx.posterior_functionals(ww, idx, want=ask)
    sd = np.sqrt(dev['var']) if any(k in want for k in ('sd', 'lower', 'upper')) else None
    made = {'mean': lambda: dev['mean'], 'var': lambda: dev['var'], 'sd': lambda: sd, 'lower': lambda: dev['mean'] - z * sd,
            'upper': lambda: dev['mean'] + z * sd, 'cov': lambda: dev['cov']}
    return {k: made[k]() for k in want}


_EPOCH_KEYS = ('mean', 'var', 'lower', 'upper', 'cov', 'contrast', 'contrastVar', 'contrastLower', 'contrastUpper', 'eta', 'etaVar', 'etaLower', 'etaUpper')


def _experiment_bins(experiment):
    """(T, lengths): the bin count of the experiment's session - the longest trial of the experiment, or of the one it was sub-sampled from - and
    the bin count of every trial of experiment.data.  Host arithmetic only."""
    root = getattr(experiment, '_pgpfa_parent', None) if hasattr(experiment, 'batchTrIdx') else None
    root = experiment if root is None else root
    T = max(int(np.shape(tr['Y'])[1]) for tr in root.data)
    return T, np.array([int(np.shape(tr['Y'])[1]) for tr in experiment.data], dtype=np.int64)


def _epoch_bins(start, stop, binSize):
    """The grid bins j (any integer) with start <= j binSize < stop, by exactly that comparison."""
    jj = np.arange(int(np.floor(start / binSize)) - 1, int(np.ceil(stop / binSize)) + 2, dtype=np.int64)
    tj = jj * binSize
    return jj[(tj >= start) & (tj < stop)]


def _epoch_windows(epochs, binSize, T, lengths, pos, align, forecast):
    """Window weights of posteriorEpochs: (E, T) without `align`, (n, E, T) with - uniform 1 / |B| over the bins B of every window, 0 elsewhere.
    lengths: bin count of every listed trial; pos: its position in experiment.data (for the messages).  Raises ValueError on an epoch that is not
    a (start, stop) pair of finite numbers, an empty window, one that leaves [0, T) and - unless `forecast` - one that passes a listed trial's
    own length."""
    ep = np.asarray(epochs, dtype=np.float64)
    if ep.ndim != 2 or ep.shape[1] != 2 or ep.shape[0] < 1:
        raise ValueError('epochs: a list of (start_ms, stop_ms) pairs expected, got shape %s' % (ep.shape,))
    if not np.all(np.isfinite(ep)):
        raise ValueError('epochs: window %d is not finite' % int(np.argwhere(~np.isfinite(ep))[0][0]))
    n, E = len(lengths), ep.shape[0]
    shift = None
    if align is not None:
        shift = np.asarray(align, dtype=np.float64).reshape(-1)
        if shift.shape != (n,):
            raise ValueError('align: one event time in ms per listed trial expected (%d), got %d' % (n, shift.size))
        if not np.all(np.isfinite(shift)):
            raise ValueError('align: the event time of list entry %d is not finite' % int(np.argwhere(~np.isfinite(shift))[0][0]))
    W = np.zeros((n if shift is not None else 1, E, T))
    for i in range(W.shape[0]):
        off = 0.0 if shift is None else float(shift[i])
        who = '' if shift is None else ' of list entry %d (trial %d, aligned to %g ms)' % (i, int(pos[i]), off)
        for e in range(E):
            bins = _epoch_bins(ep[e, 0] + off, ep[e, 1] + off, binSize)
            if bins.size == 0:
                raise ValueError('epochs: window %d%s, [%g, %g) ms, holds no bin (bin j sits at j * %g ms)' % (e, who, ep[e, 0] + off, ep[e, 1] + off, binSize))
            if bins[0] < 0 or bins[-1] >= T:
                raise ValueError('epochs: window %d%s, bins %d .. %d, leaves the grid [0, %d)' % (e, who, bins[0], bins[-1], T))
            if not forecast:
                short = [j for j in (range(n) if shift is None else [i]) if bins[-1] >= lengths[j]]
                if short:
                    raise ValueError('epochs: window %d, bins %d .. %d, passes the %d bins of trial %d (list entry %d); forecast=True takes the '
                                     "GP's forecast there" % (e, bins[0], bins[-1], lengths[short[0]], int(pos[short[0]]), short[0]))
            W[i, e, bins] = 1.0 / bins.size
    return W if shift is not None else W[0]


def _latent_functionals(W, xdim):
    """Window weights (..., E, T) as functionals of the latent vector, one per (window, latent): (..., E * xdim, xdim, T), window-major."""
    eye = np.eye(xdim)
    U = W[..., :, None, None, :] * eye[:, :, None]                     # (..., E, xdim, xdim, T)
    return np.ascontiguousarray(U.reshape(W.shape[:-2] + (W.shape[-2] * xdim, xdim, W.shape[-1])))


def posteriorEpochs(params, experiment, epochs, infRes=None, trials=None, align=None, contrasts=None, conditions=None, level=0.95, forecast=False,
                    want=('mean', 'lower', 'upper')):
    """The mean of every latent over task epochs, with credible bands that account for the correlation between bins, the change between two
    epochs, and the window-averaged log rate of every neuron: exact posteriors of linear functionals (posteriorFunctionals).

    epochs: a list of (start_ms, stop_ms); the weights of an epoch are uniform 1 / |B| over the grid bins j with start <= j * binSize < stop.
    align: one event time in ms per listed trial; the windows are then shifted by it, trial by trial.  contrasts: a list of (a, b) epoch indices,
    for xbar(b) - xbar(a) per latent - functionals of their own, so the band carries the correlation between the two epochs.
    conditions: one integer label per listed trial.  forecast: allow a window to pass a trial's own T_r bins, where the posterior is the GP's
    forecast.  infRes, trials: as for posteriorFunctionals.
    want: any of 'mean', 'var', 'lower', 'upper' - (n, E, xdim) - 'cov', the joint (n, E * xdim, E * xdim) covariance of the epoch means
    (epoch-major), 'eta', 'etaVar', 'etaLower', 'etaUpper' - (n, E, ydim): the window-averaged log rate d_i + c_i . xbar of every neuron, by the
    call's diagonal-only path, so no plane over the E * ydim functionals is formed - and, with `contrasts`, 'contrast', 'contrastVar',
    'contrastLower', 'contrastUpper', (n, len(contrasts), xdim); `contrasts` alone adds the three keys 'contrast', 'contrastLower' and
    'contrastUpper' to want.  With `conditions` the dict also holds 'condition_mean' (G, E, xdim), 'condition_contrast' (G, len(contrasts),
    xdim) when there are contrasts, 'condition_count' (G) and 'condition_labels' (G): the plain means over a condition's listed trials.
    Raises ValueError before anything reaches the device on an empty window, a window that leaves [0, T), one that passes a trial's own length
    while forecast=False (naming the trial), and on contrast indices out of range."""
    want = tuple(want)
    unknown = [k for k in want if k not in _EPOCH_KEYS]
    if unknown:
        raise ValueError('want: unknown key(s) %s; known: %s' % (unknown, list(_EPOCH_KEYS)))
    z = _band_z(level)
    T, all_lengths = _experiment_bins(experiment)
    pos = np.arange(len(experiment.data)) if trials is None else np.asarray(trials, dtype=np.int64).reshape(-1)
    if pos.size == 0:
        raise ValueError('empty trial list')
    if np.any(pos < 0) or np.any(pos >= len(experiment.data)):
        raise ValueError('trials: positions in experiment.data expected (0 .. %d)' % (len(experiment.data) - 1))
    binSize = float(experiment.binSize)
    W = _epoch_windows(epochs, binSize, T, all_lengths[pos], pos, align, forecast)
    E = W.shape[-2]
    pairs = np.zeros((0, 2), dtype=np.int64)
    if contrasts is not None:
        cc = np.asarray(contrasts)
        if cc.ndim != 2 or cc.shape[1] != 2 or cc.shape[0] < 1 or not np.issubdtype(cc.dtype, np.integer):
            raise ValueError('contrasts: a list of (a, b) epoch indices expected')
        pairs = cc.astype(np.int64)
        if np.any(pairs < 0) or np.any(pairs >= E):
            bad = pairs[np.argwhere((pairs < 0) | (pairs >= E))[0][0]]
            raise ValueError('contrasts: (%d, %d) names an epoch outside 0 .. %d' % (bad[0], bad[1], E - 1))
        want = want + tuple(k for k in ('contrast', 'contrastLower', 'contrastUpper') if k not in want)
    elif any(k.startswith('contrast') for k in want):
        raise ValueError("want: %s needs contrasts=[(a, b), ...]" % [k for k in want if k.startswith('contrast')])
    if not want and conditions is None:
        raise ValueError('nothing asked for: want is empty and there are no conditions')
    labels, group = (None, None) if conditions is None else _condition_groups(conditions, pos.size)
    sess, idx = _resident_posterior('posteriorEpochs', params, experiment, infRes, trials, set_params=True)
    if sess.T != T:
        raise ValueError('the session holds %d bins, the experiment %d' % (sess.T, T))
    C = np.asarray(params['C'], dtype=np.float64)
    d = np.asarray(params['d'], dtype=np.float64).reshape(-1)
    ydim, xdim = C.shape
    nC = pairs.shape[0]
    out = {}
    # epoch means and contrasts: one call, the contrasts behind the epochs
    lat_keys = {'mean': 'mean', 'var': 'var', 'lower': 'lower', 'upper': 'upper', 'cov': 'cov', 'contrast': 'mean', 'contrastVar': 'var',
                'contrastLower': 'lower', 'contrastUpper': 'upper'}
    ask = tuple(sorted(set(lat_keys[k] for k in want if k in lat_keys) | ({'mean'} if labels is not None else set())))
    if ask:
        Wall = W if nC == 0 else np.concatenate([W, W[..., pairs[:, 1], :] - W[..., pairs[:, 0], :]], axis=-2)
        got = _functional_bands(sess.ctx, _latent_functionals(Wall, xdim), idx, z, ask)
        n = idx.size
        for k in want:
            if k == 'cov':
                out[k] = np.ascontiguousarray(got['cov'][:, :E * xdim, :E * xdim])
            elif k in lat_keys:
                full = got[lat_keys[k]].reshape(n, E + nC, xdim)
                out[k] = np.ascontiguousarray(full[:, E:] if k.startswith('contrast') else full[:, :E])
        if labels is not None:
            full = got['mean'].reshape(n, E + nC, xdim)
            cnt = np.bincount(group, minlength=len(labels))
            tot = np.zeros((len(labels), E + nC, xdim))
            for i in range(n):                                         # in list order: reproducible
                tot[group[i]] += full[i]
            avg = tot / cnt[:, None, None]
            out['condition_mean'] = avg[:, :E]
            if nC:
                out['condition_contrast'] = avg[:, E:]
            out['condition_count'] = cnt
            out['condition_labels'] = labels
    # window-averaged log rates: E * ydim functionals with weights C[i, k] / |B|, variances alone
    eta_keys = {'eta': 'mean', 'etaVar': 'var', 'etaLower': 'lower', 'etaUpper': 'upper'}
    ask = tuple(sorted(set(eta_keys[k] for k in want if k in eta_keys)))
    if ask:
        U = W[..., :, None, None, :] * C[:, :, None]                   # (..., E, ydim, xdim, T)
        U = np.ascontiguousarray(U.reshape(W.shape[:-2] + (E * ydim, xdim, T)))
        need_var = any(k in ask for k in ('var', 'lower', 'upper'))
        need_mean = any(k in ask for k in ('mean', 'lower', 'upper'))
        got = sess.ctx.posterior_functionals(U, idx, want=(('mean',) if need_mean else ()) + (('var',) if need_var else ()))
        eta = got['mean'].reshape(idx.size, E, ydim) + d[None, None, :] if need_mean else None
        var = got['var'].reshape(idx.size, E, ydim) if need_var else None
        sd = np.sqrt(var) if ('lower' in ask or 'upper' in ask) else None
        made = {'eta': lambda: eta, 'etaVar': lambda: var, 'etaLower': lambda: eta - z * sd, 'etaUpper': lambda: eta + z * sd}
        for k in want:
            if k in eta_keys:
                out[k] = made[k]()
    return out


# -- co-smoothing: held-out neurons predicted from the others -------------------------------------------------
def coSmoothing(params, experiment, heldOut, trials=None, predictive=False):
    """Predict the neurons `heldOut` on the listed trials from the trials' other neurons and score the prediction: the held-out neurons are
    marked unobserved on those trials (on top of experiment.data[r]['observed']), ONE Laplace E-step gives the posterior of the latents
    without them, and their rate is the posterior mean rate exp(eta + var / 2) that posteriorRates documents.  No ydim mode searches per
    trial, as leaveOneOutPrediction runs them.

    Runs on a context of its own that holds the listed trials (and one silent, fully observed trial that no E-step touches: a neuron
    masked on every listed trial is otherwise observed nowhere, which the observation table refuses), so the experiment, its session, the
    session's table and its resident posterior stay as they were.

    trials: positions in experiment.data (None: all).  Returns a dict: 'rate' - a list with one (len(heldOut), T_r) array per listed trial, in
    spikes per second; 'bitsPerSpike' - sum over the scored (trial, neuron, bin) of [y log lam - lam] - [y log lbar_n - lbar_n], divided by
    log 2 times the spikes scored, lam the predicted count per bin, lbar_n the mean count per bin of neuron n over its scored bins;
    'bitsPerSpikePerNeuron' [len(heldOut)] (NaN for a neuron without a scored spike).  A (trial, neuron) pair is scored when the experiment
    itself observed the neuron on that trial: the score is computed on the host from the rate plane and the caller's true counts.
    predictive=True adds the proper score: 'logPredictive' - one (len(heldOut), T_r) array per trial, log P(y) of the true count under the
    predictive distribution of posteriorCounts, NaN where the entry is not scored -, 'bitsPerSpikePredictive' - sum over the scored entries of
    log P(y) - log Poisson(y; lbar_n), both with - log y!, divided by log 2 times the spikes scored - and 'bitsPerSpikePredictivePerNeuron'."""
    from . import _session
    C = np.asarray(params['C'], dtype=np.float64)
    ydim, xdim = C.shape
    held = np.unique(np.asarray(heldOut, dtype=np.int64).reshape(-1))
    if held.size == 0 or held[0] < 0 or held[-1] >= ydim:
        raise ValueError('heldOut: neuron indices in 0..%d expected' % (ydim - 1))
    if WORLD_sharded():
        raise NotImplementedError('coSmoothing does not support sharded sessions yet')
    n_all = len(experiment.data)
    pos = np.arange(n_all) if trials is None else np.asarray(trials, dtype=np.int64).reshape(-1)
    if pos.size == 0:
        raise ValueError('empty trial list')
    table = _session._stack_observed(experiment)
    own_bins = _session._stack_observed_bins(experiment)    # (per-bin table of the experiment, or None: ANDed with the mask of the held-out neurons)
    Y, lengths = _session._stack_counts(experiment)
    if Y.shape[1] != ydim:
        raise ValueError("params['C'] has %d rows but the experiment has %d neurons" % (ydim, Y.shape[1]))
    own = np.ones((n_all, ydim), dtype=bool) if table is None else table
    n = pos.size
    bins_t = None
    if own_bins is not None:
        bins_t = np.ones((n + 1,) + own_bins.shape[1:], dtype=bool)
        bins_t[:n] = own_bins[pos]
        bins_t[:n, held] = True                          # (whole rows are masked by the observation table below; their bits do not matter)
    masked = np.ones((n + 1, ydim), dtype=bool)
    masked[:n] = own[pos]
    masked[:n, held] = False
    empty = np.flatnonzero(~masked[:n].any(axis=1))
    if empty.size:
        raise ValueError('trial %d has no observed neuron left once the held-out ones are masked' % int(pos[empty[0]]))
    Yt = np.zeros((n + 1,) + Y.shape[1:], dtype=Y.dtype)
    Yt[:n] = Y[pos]
    Yt[:n, held] = 0
    len_t = np.concatenate([np.asarray(lengths, dtype=np.int32)[pos], [Y.shape[2]]]).astype(np.int32)
    at = None
    if predictive:                                       # the true counts of the held-out neurons where they are scored, 0 elsewhere
        at = np.zeros(Yt.shape, dtype=np.int32)
        keep = own[pos][:, held][:, :, None] if own_bins is None else own[pos][:, held][:, :, None] & own_bins[pos][:, held]
        at[:n, held] = np.where(keep, Y[pos][:, held], 0)
    lam, logp = _predicted_without_hidden('coSmoothing', params, experiment, Yt, len_t, masked, bins_t, held, at)      # [n] of (held, T_r)
    per_s = 1000.0 / float(experiment.binSize)
    rates = [lm * per_s for lm in lam]
    # the score, on the host: the caller's true counts at the entries the experiment itself recorded
    scored = [np.broadcast_to(own[int(r)][held][:, None], lm.shape) if own_bins is None else own[int(r)][held][:, None] & own_bins[int(r)][held][:, :lm.shape[1]]
              for r, lm in zip(pos, lam)]
    truth = [np.asarray(experiment.data[int(r)]['Y'], dtype=np.float64)[held] for r in pos]
    total, per_neuron, _ = _score_entries(truth, lam, scored)
    out = {'rate': rates, 'bitsPerSpike': total, 'bitsPerSpikePerNeuron': per_neuron, 'heldOut': held}
    if predictive:
        out.update(_predictive_keys(truth, logp, scored))
    return out


def _predicted_without_hidden(what, params, experiment, Yt, len_t, masked, bins_t, rows=slice(None), counts_at=None):
    """The prediction step of the hold-out scores (coSmoothing, binHoldout = `what`, the prefix of a failure): a context of its own over the n listed
    trials plus one silent, fully observed trial - counts Yt (n + 1, ydim, T) with the hidden entries zeroed, lengths len_t, observation table
    masked (n + 1, ydim), per-bin table bins_t (n + 1, ydim, T) or None (checked against the other two before the context exists) -, ONE cold Laplace
    E-step over the n trials and the posterior mean count per bin exp(eta + var / 2) of the neurons `rows`.  The context is closed on every way
    out.  counts_at (n + 1, ydim, T) int32 or None: the counts at which the predictive log probability of every entry is also taken (the private
    context holds zeros at the hidden entries, so the query is given the caller's).  Returns (one (rows, T_r) array per listed trial, the same of
    log P or None)."""
    from . import _session
    n, ydim, T = Yt.shape[0] - 1, Yt.shape[1], Yt.shape[2]
    if bins_t is not None:
        bins_t = _session.compose_observed_bins(bins_t, len_t, masked, n + 1, ydim, T)
    sess = _session.Session(Yt, np.shape(params['C'])[1], float(experiment.binSize), len_t, masked)
    try:
        sess._install_observed_bins(bins_t)
        sess.set_params({'C': np.asarray(params['C'], dtype=np.float64), 'd': params['d'], 'tau': np.ndarray.flatten(np.asarray(params['tau'], dtype=np.float64))})
        idx = np.arange(n, dtype=np.int32)
        _, _, status = sess.ctx.estep_laplace(idx, warm_start=False)
        if np.any(status > 1):
            raise _hip.HipBackendError('%s: the Laplace mode search failed for %d trial(s)' % (what, int(np.sum(status > 1))))
        dev = sess.ctx.posterior_rates(idx, group=None, n_groups=0, want=['eta', 'var'])
        lam = np.exp(dev['eta'][:, rows] + 0.5 * dev['var'][:, rows])
        logp = None
        if counts_at is not None:
            logp = sess.ctx.posterior_counts(idx, counts=counts_at[:n], want=['logp'])['logp'][:, rows]
    finally:
        sess.ctx.close()
    cut = lambda a: [a[i, :, :int(len_t[i])] for i in range(n)]
    return cut(lam), (None if logp is None else cut(logp))


def _score_entries(truth, lam, scored):
    """Bits per spike over single entries: truth, lam (predicted counts per bin) and scored (booleans) are lists of (rows, T_r) arrays, one per
    trial.  Per row n: sum over its scored entries of [y log lam - lam] - [y log lbar_n - lbar_n], lbar_n the mean count of row n over its scored
    entries - the null model of coSmoothing, per entry.  Returns (total, per row (NaN for a row without a scored spike), entries scored)."""
    rows = truth[0].shape[0]
    tot_y, tot_n = np.zeros(rows), np.zeros(rows)
    for y, sc in zip(truth, scored):
        tot_y += np.where(sc, y, 0.0).sum(axis=1)
        tot_n += sc.sum(axis=1)
    with np.errstate(invalid='ignore', divide='ignore'):
        lbar = np.where(tot_n > 0, tot_y / tot_n, 0.0)
    ll, spikes = np.zeros(rows), np.zeros(rows)
    for y, lm, sc in zip(truth, lam, scored):
        y = np.where(sc, y, 0.0)                         # (NaN in the caller's counts is accepted where nothing is scored)
        with np.errstate(invalid='ignore', divide='ignore'):
            null = np.where(y > 0, y * np.log(lbar)[:, None], 0.0) - lbar[:, None]
        model = y * np.log(lm) - lm
        ll += np.where(sc, model - null, 0.0).sum(axis=1)
        spikes += y.sum(axis=1)
    with np.errstate(invalid='ignore', divide='ignore'):
        per_row = np.where(spikes > 0, ll / (np.log(2.0) * spikes), np.nan)
        total = float(ll.sum() / (np.log(2.0) * spikes.sum())) if spikes.sum() > 0 else float('nan')
    return total, per_row, int(tot_n.sum())


def binHoldout(params, experiment, heldOut, trials=None, predictive=False):
    """Predict single (neuron, bin) entries of the listed trials from everything else and score the prediction: the per-entry sibling of
    coSmoothing ("speckled" hold-out).  heldOut: one boolean (ydim, T_r) array per listed trial, True = hide and score.  The hidden entries are
    marked as not recorded (on top of the experiment's own lengths, 'observed' and 'observedBins'), ONE Laplace E-step gives the posterior of
    the latents without them, and an entry's predicted rate is the posterior mean rate exp(eta + var / 2) that posteriorRates documents.

    Runs on a context of its own that holds the listed trials and one silent, fully observed trial that no E-step touches (coSmoothing), so the
    experiment, its session, the session's tables and its resident posterior stay as they were.

    trials: positions in experiment.data (None: all).  Returns a dict: 'rate' - one (ydim, T_r) array per listed trial, spikes per second,
    every entry; 'bitsPerSpike' and 'bitsPerSpikePerNeuron' [ydim] as coSmoothing defines them, over the entries that are held out AND were
    live in the experiment (the null model is each neuron's mean count over its scored entries); 'nScored' - how many those are.
    predictive=True adds 'logPredictive', 'bitsPerSpikePredictive' and 'bitsPerSpikePredictivePerNeuron' as coSmoothing defines them."""
    from . import _session
    C = np.asarray(params['C'], dtype=np.float64)
    ydim, xdim = C.shape
    if WORLD_sharded():
        raise NotImplementedError('binHoldout does not support sharded sessions yet')
    n_all = len(experiment.data)
    pos = np.arange(n_all) if trials is None else np.asarray(trials, dtype=np.int64).reshape(-1)
    if pos.size == 0:
        raise ValueError('empty trial list')
    if len(heldOut) != pos.size:
        raise ValueError('heldOut: one boolean (ydim, T_r) array per listed trial expected (%d trials, %d arrays)' % (pos.size, len(heldOut)))
    table = _session._stack_observed(experiment)
    own_bins = _session._stack_observed_bins(experiment)
    Y, lengths = _session._stack_counts(experiment)
    if Y.shape[1] != ydim:
        raise ValueError("params['C'] has %d rows but the experiment has %d neurons" % (ydim, Y.shape[1]))
    T = Y.shape[2]
    lengths = np.asarray(lengths, dtype=np.int32)
    n = pos.size
    # the entries the experiment itself has a likelihood term for
    own_live = (np.arange(T)[None, None, :] < lengths[pos][:, None, None]) & np.ones((n, ydim, T), dtype=bool)
    if table is not None:
        own_live &= table[pos][:, :, None]
    if own_bins is not None:
        own_live &= own_bins[pos]
    hide = np.zeros((n, ydim, T), dtype=bool)
    for i, h in enumerate(heldOut):
        h = np.asarray(h)
        L = int(lengths[pos[i]])
        if h.shape != (ydim, L):
            raise ValueError('heldOut[%d] must have shape (ydim, T_r) = (%d, %d), got %s' % (i, ydim, L, h.shape))
        hide[i, :, :L] = h != 0
    bins_t = np.ones((n + 1, ydim, T), dtype=bool)
    bins_t[:n] = own_live & ~hide
    empty = np.flatnonzero(~bins_t[:n].any(axis=(1, 2)))
    if empty.size:
        raise ValueError('trial %d has no live entry left once the held-out ones are hidden' % int(pos[empty[0]]))
    masked = np.ones((n + 1, ydim), dtype=bool)
    if table is not None:
        masked[:n] = table[pos]
    Yt = np.zeros((n + 1,) + Y.shape[1:], dtype=Y.dtype)
    Yt[:n] = np.where(bins_t[:n], Y[pos], 0)
    len_t = np.concatenate([lengths[pos], [T]]).astype(np.int32)
    at = None
    if predictive:                                       # the true counts at the scored entries, 0 elsewhere
        at = np.zeros(Yt.shape, dtype=np.int32)
        at[:n] = np.where(hide & own_live, Y[pos], 0)
    lam, logp = _predicted_without_hidden('binHoldout', params, experiment, Yt, len_t, masked, bins_t, counts_at=at)      # [n] of (ydim, T_r)
    per_s = 1000.0 / float(experiment.binSize)
    scored = [(hide[i] & own_live[i])[:, :int(len_t[i])] for i in range(n)]
    truth = [np.asarray(experiment.data[int(r)]['Y'], dtype=np.float64) for r in pos]
    total, per_neuron, n_scored = _score_entries(truth, lam, scored)
    out = {'rate': [lm * per_s for lm in lam], 'bitsPerSpike': total, 'bitsPerSpikePerNeuron': per_neuron, 'nScored': n_scored}
    if predictive:
        out.update(_predictive_keys(truth, logp, scored))
    return out


def speckledHoldout(experiment, holdoutFraction=0.1, seed=0):
    """A seeded random subset of the experiment's live entries: one boolean (ydim, T_r) array per trial, True = held out.  Every entry is drawn
    with probability holdoutFraction from numpy.random.default_rng(seed), trial after trial; entries the experiment did not record are never
    chosen.  The subset depends on the experiment and the seed only - not on a latent width."""
    from . import _session
    if not 0.0 < float(holdoutFraction) < 1.0:
        raise ValueError('holdoutFraction must lie strictly between 0 and 1')
    rng = np.random.default_rng(seed)
    table = _session._stack_observed(experiment)
    own_bins = _session._stack_observed_bins(experiment)
    out = []
    for r, tr in enumerate(experiment.data):
        shape = np.asarray(tr['Y']).shape
        live = np.ones(shape, dtype=bool)
        if table is not None:
            live &= table[r][:, None]
        if own_bins is not None:
            live &= own_bins[r][:, :shape[1]]
        out.append((rng.random(shape) < float(holdoutFraction)) & live)
    return out


def _with_hidden_entries(experiment, heldOut):
    """A shallow copy of the experiment whose trials carry 'observedBins' = their own table AND NOT heldOut (a data set of its own on the device)."""
    from . import _session
    own_bins = _session._stack_observed_bins(experiment)
    hidden = copy.copy(experiment)
    hidden.__dict__.pop('_pgpfa_parent', None)
    hidden.__dict__.pop('batchTrIdx', None)
    hidden.data = []
    for r, (tr, h) in enumerate(zip(experiment.data, heldOut)):
        tr = dict(tr)
        keep = ~np.asarray(h, dtype=bool)
        if own_bins is not None:
            keep &= own_bins[r][:, :keep.shape[1]]
        tr['observedBins'] = keep
        hidden.data.append(tr)
    return hidden


def WORLD_sharded():
    from . import _session
    return bool(_session.WORLD.enabled)


# -- latent-dimensionality cross-validation (reference util.py:180-275) -------------------------------------
def splitTrainingTestDataset(experiment, numTrainingTrials, numTestTrials):
    """First numTrainingTrials trials / the numTestTrials after them, as shallow copies (reference util.py:263-275)."""
    if numTestTrials + numTrainingTrials > experiment.numTrials:
        print('Error: Number of training trials and test trials must sum to less than the number of available trials.')
    trainingSet, testSet = copy.copy(experiment), copy.copy(experiment)
    trainingSet.data = experiment.data[:numTrainingTrials]
    trainingSet.numTrials = numTrainingTrials
    testSet.data = experiment.data[numTrainingTrials:numTrainingTrials + numTestTrials]
    testSet.numTrials = numTestTrials
    for part in (trainingSet, testSet):                   # the copies are data sets of their own on the device
        part.__dict__.pop('_pgpfa_parent', None)
        part.__dict__.pop('batchTrIdx', None)
    return trainingSet, testSet


def negLogEvidencePerBin(params, experiment):
    """- sum_r log Z_r / sum_r T_r over the experiment's trials: one Laplace E-step at `params` with inference.LAPLACE_EVIDENCE on (the
    switch is restored).  Trials may differ in length."""
    from . import inference
    switch = inference.LAPLACE_EVIDENCE
    inference.LAPLACE_EVIDENCE = True
    try:
        infRes, _ = inference.laplace(experiment, copy.copy(params), returnOptimRes=False)
    finally:
        inference.LAPLACE_EVIDENCE = switch
    bins = sum(int(np.shape(tr['Y'])[1]) for tr in experiment.data)
    return -float(infRes.mean_log_evidence) * len(experiment.data) / bins


_IMPORTANCE_KEYS = ('logEvidence', 'laplace', 'logRatio', 'ess', 'logWeights')


def importanceEvidence(params, experiment, infRes=None, trials=None, nSamples=256, seed=0, want=('logEvidence', 'ess')):
    """The Laplace log evidence of every listed trial corrected by importance sampling from the Laplace posterior itself, and how far that
    Gaussian is from the trial's true posterior.  With w_s the importance weights of nSamples draws (pgpfa_importance_weights; the draws are
    those of posteriorSamples under the same seed and never leave the device):
      'logEvidence' [n]  log Z_Laplace + log mean_s w_s - mean_s w_s is an unbiased estimator of Z / Z_Laplace, so this estimates the trial's
                         true log marginal likelihood (normalisation of the Laplace value: sum log y! dropped)
      'laplace'     [n]  log Z_Laplace itself          'logRatio' [n]  the correction, log mean_s w_s
      'ess'         [n]  effective sample size (sum w)^2 / sum w^2, between 1 and nSamples: near nSamples where Laplace can be trusted
      'logWeights'  [n][nSamples]  log w_s (with posteriorSamples(..., seed=seed): a self-normalised importance sampler of the true posterior)
    The dict holds the keys of `want`.  infRes None: one Laplace E-step at `params` over the experiment with inference.LAPLACE_EVIDENCE on (the
    switch is restored).  A DeviceInfRes of this experiment's session whose entries are still the resident ones: that posterior - it must come
    from a Laplace E-step that computed the evidence, the library's error comes through otherwise.  trials: positions in experiment.data (None:
    all; repeats allowed).  The weights assume a stationary mode; nothing here acts on a low ess - it is reported."""
    from . import inference
    want = tuple(want)
    unknown = [k for k in want if k not in _IMPORTANCE_KEYS]
    if unknown:
        raise ValueError('want: unknown key(s) %s; known: %s' % (unknown, list(_IMPORTANCE_KEYS)))
    if not want:
        raise ValueError('nothing asked for: want is empty')
    if int(nSamples) != nSamples or int(nSamples) < 1:
        raise ValueError('nSamples = %r: a count of draws per trial, at least 1' % (nSamples,))
    switch = inference.LAPLACE_EVIDENCE
    if infRes is None:
        inference.LAPLACE_EVIDENCE = True
    try:
        sess, idx = _resident_posterior('importanceEvidence', params, experiment, infRes, trials, set_params=False)
    finally:
        inference.LAPLACE_EVIDENCE = switch
    laplace = sess.ctx.log_evidence(idx)
    dev = sess.ctx.importance_weights(idx, n_samples=int(nSamples), seed=int(seed), want=('log_ratio', 'ess') + (('log_w',) if 'logWeights' in want else ()))
    full = {'logEvidence': laplace + dev['log_ratio'], 'laplace': laplace, 'logRatio': dev['log_ratio'], 'ess': dev['ess'], 'logWeights': dev.get('log_w')}
    return {k: full[k] for k in want}


def negLogImportanceEvidencePerBin(params, experiment, nSamples, seed=0):
    """- sum_r (log Z_Laplace,r + logRatio_r) / sum_r T_r over the experiment's trials: negLogEvidencePerBin with every trial's log evidence
    corrected by importanceEvidence(nSamples, seed) - one Laplace E-step at `params` and one pass of weights."""
    res = importanceEvidence(params, experiment, nSamples=nSamples, seed=seed, want=('logEvidence',))
    bins = sum(int(np.shape(tr['Y'])[1]) for tr in experiment.data)
    return -float(np.sum(res['logEvidence'])) / bins


class crossValidation:
    """reference util.py:180-249: for xdim = 1..maxXdim fit on the training split and score the leave-one-neuron-out
    prediction error on the test split; optimXdim is the arg-min.  learningMethod: 'batch', 'diag', 'hess' or 'grad'.
    score='evidence' (an addition; Laplace only) scores a fit by ONE Laplace E-step of its parameters on the test split instead of the
    numTestTrials * ydim held-out mode searches: errs[i] = - sum_r log Z_r / sum_r T_r, the negative Laplace log evidence per bin (lower is
    better, so optimXdim stays the arg-min).  It also takes test trials of unequal length, which the leave-one-out score refuses.
    importance=S (with score='evidence'; None - the default - is the Laplace score itself) corrects every test trial's log evidence by
    importance sampling with S draws under `seed` (importanceEvidence): errs[i] = - sum_r (log Z_Laplace,r + logRatio_r) / sum_r T_r.
    score='speckled' (an addition; Laplace only) hides a seeded random subset of the TRAINING trials' live entries (speckledHoldout: each with
    probability holdoutFraction, numpy.random.default_rng(seed), the same subset for every width), fits on the rest and scores the fit by
    binHoldout at the hidden entries: errs[i] = - bitsPerSpike (lower is better); the test split is not used.  predictive=True (with
    score='speckled') scores by the predictive distribution of the counts instead: errs[i] = - bitsPerSpikePredictive."""

    def __init__(self, experiment, numTrainingTrials=10, numTestTrials=2, maxXdim=6, maxEMiter=3, batchSize=5,
                 inferenceMethod='laplace', learningMethod='batch', quiet=True, score='loo', holdoutFraction=0.1, seed=0, predictive=False, importance=None):
        from . import engine
        if learningMethod not in ('batch', 'diag', 'hess', 'grad'):
            raise ValueError("learningMethod must be 'batch', 'diag', 'hess' or 'grad'")
        if score not in ('loo', 'evidence', 'speckled'):
            raise ValueError("score must be 'loo' or 'evidence', or 'speckled' (hold-out of single entries of the training trials)")
        if score == 'evidence' and inferenceMethod != 'laplace':
            raise ValueError("score='evidence' is the Laplace log evidence: it needs inferenceMethod='laplace'")
        if score == 'speckled' and inferenceMethod != 'laplace':
            raise ValueError("score='speckled' fits and scores under a per-bin table: it needs inferenceMethod='laplace'")
        if predictive and score != 'speckled':
            raise ValueError("predictive=True is the predictive score of binHoldout: it needs score='speckled'")
        if importance is not None and score != 'evidence':
            raise ValueError("importance=S corrects the Laplace log evidence: it needs score='evidence'")
        if importance is not None and (int(importance) != importance or int(importance) < 1):
            raise ValueError('importance = %r: a count of draws per trial, at least 1 (None: the Laplace score)' % (importance,))
        trainingSet, testSet = splitTrainingTestDataset(experiment, numTrainingTrials, numTestTrials)
        if score == 'speckled':
            scoredSet = trainingSet                       # (the hidden entries are scored against the training trials' true counts)
            self.heldOut = speckledHoldout(scoredSet, holdoutFraction, seed)
            trainingSet = _with_hidden_entries(scoredSet, self.heldOut)
        self.errs, self.fits = [], []
        for xdimFit in range(1, maxXdim + 1):
            initParams = initializeParams(xdimFit, trainingSet.ydim, trainingSet)
            if learningMethod == 'batch':
                fit = engine.PPGPFAfit(experiment=trainingSet, initParams=initParams, inferenceMethod=inferenceMethod,
                                       EMmode='Batch', maxEMiter=maxEMiter, quiet=quiet)
            else:
                fit = engine.PPGPFAfit(experiment=trainingSet, initParams=initParams, inferenceMethod=inferenceMethod,
                                       EMmode='Online', onlineParamUpdateMethod=learningMethod, maxEMiter=maxEMiter,
                                       batchSize=batchSize, quiet=quiet)
            if score == 'speckled':
                predErr = -binHoldout(fit.optimParams, scoredSet, self.heldOut, predictive=predictive)['bitsPerSpikePredictive' if predictive else 'bitsPerSpike']
            elif score == 'evidence':
                predErr = (negLogEvidencePerBin(fit.optimParams, testSet) if importance is None
                           else negLogImportanceEvidencePerBin(fit.optimParams, testSet, int(importance), seed))
            else:
                _, predErr = leaveOneOutPrediction(fit.optimParams, testSet)
            self.errs.append(predErr)
            self.fits.append(fit)
        self.inferenceMethod, self.learningMethod, self.score, self.importance = inferenceMethod, learningMethod, score, importance
        self.optimXdim = int(np.argmin(self.errs)) + 1
        self.maxXdim = maxXdim


# -- minibatches (reference util.py:449-473) ---------------------------------------------------------------
def subsampleTrials(experiment, batchSize):
    """Same draw from the global legacy RNG as the reference (np.random.choice without replacement);
    the returned shallow copy remembers its parent so the device keeps using the resident counts."""
    numTrials = len(experiment.data)
    batchTrIdx = np.random.choice(numTrials, batchSize, replace=False)
    sub = copy.copy(experiment)
    sub.data = [experiment.data[i] for i in batchTrIdx]
    sub.numTrials = batchSize
    sub.batchTrIdx = batchTrIdx
    sub._pgpfa_parent = getattr(experiment, '_pgpfa_parent', experiment)
    if hasattr(experiment, 'batchTrIdx') and getattr(experiment, '_pgpfa_parent', None) is not None:
        sub.batchTrIdx = np.asarray(experiment.batchTrIdx)[batchTrIdx]
    return sub


def seenTrials(experiment, seenIdx):
    idx = np.asarray(seenIdx).flatten()
    seen = copy.copy(experiment)
    seen.data = [experiment.data[i] for i in idx]
    seen.numTrials = len(seen.data)
    return seen


# -- synthetic population (distributions of reference util.py:705-750) ---------------------------------------
class dataset:
    """Trials of population spike counts sampled from  x_k ~ GP(0, K(tau_k)),  y ~ Poisson(exp(Cx+d)).

    Attributes as in the reference: data (list of {'X','Y'}), xdim, ydim, T, trialDur, binSize, numTrials,
    seed, params.  `sampler='reference'` reproduces the reference's global-RNG stream bit for bit: the
    reference calls np.random.multivariate_normal on the (xdim*T)^2 covariance once per trial (util.py:738-741),
    which repeats the same SVD of K_big every time; here the SVD is taken once and each trial is the same
    standard_normal draw times the same sqrt(s) * v matrix - identical bits, without the per-trial
    (xdim*T)^3 (minutes per trial at config 3).  `sampler='cholesky'` draws the same distributions per latent
    through T x T factors from numpy's Generator (no (xdim*T)^2 matrix at all).  `sampler='device'` draws every trial on the
    GPU from a counter-based generator: 1024 config-3 trials in well under a second.
    """

    def __init__(self, trialDur=1000, binSize=10, drawSameX=False, numTrials=20, xdim=3, ydim=30, seed=12, dOffset=-1,
                 fixTau=False, fixedTau=None, params=None, model='pgpfa', sampler='reference', verbose=False):
        if model != 'pgpfa':
            raise NotImplementedError("only model='pgpfa' is on the hot path")
        self.trialDur, self.binSize, self.drawSameX = trialDur, binSize, drawSameX
        self.numTrials, self.xdim, self.ydim, self.seed = numTrials, xdim, ydim, seed
        self.T = int(trialDur / binSize)
        T = self.T
        np.random.seed(seed)
        if params is None:
            params = {'C': np.random.rand(ydim, xdim) - 0.5,
                      'd': np.random.rand(ydim) * (-2) + dOffset,
                      'tau': np.abs(np.random.rand(xdim)) + 0.01}
            if fixTau:
                params['tau'] = np.asarray(fixedTau, dtype=np.float64)
        self.params = params
        tau = np.asarray(params['tau'], dtype=np.float64).reshape(-1)
        t = np.arange(T, dtype=np.float64) * binSize
        dsq = (t[:, None] - t[None, :]) ** 2
        K = np.stack([0.999 * np.exp(-0.5 * (dsq / (tk * 1000.0) ** 2)) + 0.001 * np.eye(T) for tk in tau])
        offset = np.asarray(params['d'], dtype=np.float64)[:, None]
        data = []
        if sampler == 'reference':
            K_big = np.zeros((xdim * T, xdim * T))
            for k in range(xdim):
                K_big[k * T:(k + 1) * T, k * T:(k + 1) * T] = K[k]
            _, sv, vt = np.linalg.svd(K_big)                       # what legacy multivariate_normal factors cov with
            mix = np.sqrt(sv)[:, None] * vt
            mean = np.zeros(T * xdim)

            def draw():
                x = np.dot(np.random.standard_normal((1, T * xdim)).reshape(-1, T * xdim), mix)
                x += mean
                return np.reshape(x, [xdim, T])
            pois = lambda lam: np.random.poisson(lam=lam)
        elif sampler == 'cholesky':
            rng = np.random.default_rng(seed)
            Lk = np.linalg.cholesky(K)
            draw = lambda: np.einsum('kts,ks->kt', Lk, rng.standard_normal((xdim, T)))
            pois = lambda lam: rng.poisson(lam)
        elif sampler == 'device':
            # all trials on the GPU (pgpfa_generate): latents through the resident low-rank form of the Gram matrices, counts by a
            # counter-based generator keyed by `seed` - same distributions, NOT NumPy's stream (no fixture depends on this one)
            if drawSameX:
                raise NotImplementedError("drawSameX needs sampler='reference' or 'cholesky'")
            ctx = _hip.Context(ydim, xdim, T, numTrials, float(binSize))
            try:
                ctx.set_params(np.asarray(params['C'], dtype=np.float64), offset[:, 0], tau)
                Xd, Yd = ctx.generate(seed)
            finally:
                ctx.close()
            self.data = [{'X': Xd[i], 'Y': Yd[i]} for i in range(numTrials)]
            return
        else:
            raise ValueError("sampler must be 'reference', 'cholesky' or 'device'")
        X0 = draw() if drawSameX else None
        for i in range(numTrials):
            X = X0 if drawSameX else draw()
            data.append({'X': X, 'Y': pois(np.exp(params['C'] @ X + offset))})
            if verbose:
                Printer('Sampling trial %d ...' % (i + 1))
        self.data = data

    def getAllRaster(self):
        self.all_raster = np.concatenate([tr['Y'] for tr in self.data], axis=1)
        return self.all_raster

    def getAvgFiringRate(self):
        self.avgFR = float(np.mean(self.getAllRaster()) / self.binSize * 1000.0)
        return self.avgFR


def countMoments(experiment, xdim):
    """Mean and covariance of the spike counts over all (trial, bin) samples - np.mean / np.cov of the concatenated
    raster (reference util.py:523-533, engine.py:487-492) - from the device's exact integer sums of the resident
    count tensor; the raster is never formed on the host.  Returns (mean[q], cov[q][q], per-neuron totals, samples).
    Trials of unequal length: the samples are the sum of the trials' own bin counts (their padding is no sample)."""
    from . import _session
    sess, trial_idx = _session.session_for(experiment, xdim)
    local = getattr(experiment, '_pgpfa_local_shard', False)
    lo, hi = (0, len(trial_idx)) if local else sess.local_slice(len(trial_idx))
    s, S, ns = sess.ctx.count_moments(trial_idx[lo:hi])
    s, S, ns = s.astype(np.float64), S.astype(np.float64), float(ns)      # exact: all sums are far below 2^53
    if sess.comm_ready:
        red = sess.allreduce(np.concatenate([s, S.reshape(-1), [ns]]))
        s, S, ns = red[:s.size], red[s.size:-1].reshape(S.shape), float(red[-1])
    if getattr(sess, 'observed_bins', None) is not None:   # (per-bin table: live and co-live entries, counted on the host from the boolean table)
        mean, cov = _live_moments(s, S, sess.live_entries()[np.asarray(trial_idx, dtype=np.int64)])
        return mean, cov, s, int(ns)
    observed = getattr(sess, 'observed', None)
    if observed is not None:
        mean, cov = _observed_moments(s, S, observed, sess.lengths, sess.T, trial_idx)
        return mean, cov, s, int(ns)
    mean = s / ns
    cov = (S - np.outer(s, s) / ns) / (ns - 1.0)
    return mean, cov, s, int(ns)


def observedTrialCounts(experiment, xdim):
    """Per neuron, the number of the experiment's trials that observed it (experiment.data[r]['observed']); the trial count where no table is set.
    Under a per-bin table ('observedBins') a trial counts by the fraction of its T_r bins that are live for the neuron: sum_r n_live[r][i] / T_r."""
    from . import _session
    sess, trial_idx = _session.session_for(experiment, xdim)
    if getattr(sess, 'observed_bins', None) is not None:
        idx = np.asarray(trial_idx, dtype=np.int64)
        Tr = np.full(len(idx), float(sess.T)) if sess.lengths is None else np.asarray(sess.lengths, dtype=np.float64)[idx]
        return (sess.live_entries()[idx].sum(axis=2) / Tr[:, None]).sum(axis=0)
    observed = getattr(sess, 'observed', None)
    if observed is None:
        return float(len(trial_idx))
    return observed[np.asarray(trial_idx, dtype=np.int64)].sum(axis=0).astype(np.float64)


def _live_moments(s, S, live):
    """Count moments under a per-bin table: the formulas of _observed_moments with n_i = live entries of neuron i and n_ij = entries at which both
    neurons of a pair are live, over the boolean table live[n][q][T] of the listed trials (lengths and the observation table folded in)."""
    L = np.asarray(live, dtype=np.float64)
    n_i = L.sum(axis=(0, 2))
    n_ij = np.einsum('rit,rjt->ij', L, L)
    with np.errstate(invalid='ignore', divide='ignore'):
        mean = np.where(n_i > 0, s / n_i, 0.0)
        cov = (S - np.outer(s, s) * n_ij / np.outer(n_i, n_i)) / (n_ij - 1.0)
    return mean, np.where(n_ij >= 2, cov, 0.0)


def _observed_moments(s, S, observed, lengths, T, trial_idx):
    """Count moments under an observation table (host arithmetic on the device's integer sums s[q], S[q][q] over the listed trials, whose rows of
    unobserved neurons are zero): n_i = sum_r O[r][i] T_r samples of neuron i, n_ij = sum_r O[r][i] O[r][j] T_r co-observed samples of a pair;
    mean_i = s_i / n_i, cov_ij = (S_ij - s_i s_j n_ij / (n_i n_j)) / (n_ij - 1), and cov_ij = 0 where n_ij < 2 (the initialiser then treats the
    pair as uncorrelated).  A neuron without a sample among the listed trials has mean 0."""
    idx = np.asarray(trial_idx, dtype=np.int64)
    O = np.asarray(observed)[idx].astype(np.float64)
    Tr = np.full(len(idx), float(T)) if lengths is None else np.asarray(lengths, dtype=np.float64)[idx]
    n_i = O.T @ Tr
    n_ij = (O * Tr[:, None]).T @ O
    with np.errstate(invalid='ignore', divide='ignore'):
        mean = np.where(n_i > 0, s / n_i, 0.0)
        cov = (S - np.outer(s, s) * n_ij / np.outer(n_i, n_i)) / (n_ij - 1.0)
    return mean, np.where(n_ij >= 2, cov, 0.0)


def getMeanCovYfromParams(params, experiment=None):
    """Mean and second moment of the counts implied by the parameters under a unit-variance latent (reference
    util.py:24-39): E[y] = exp(diag(CC^T)/2 + d), E[y_i y_j] = E[y_i]E[y_j]exp(CC^T_ij/2) (+ E[y_i] on the diagonal)."""
    C = np.asarray(params['C'], dtype=np.float64)
    lamb = C @ C.T
    E_y = np.exp(0.5 * np.diag(lamb) + np.asarray(params['d'], dtype=np.float64).reshape(-1))
    E_yy = np.outer(E_y, E_y) * np.exp(0.5 * lamb)
    E_yy[np.diag_indices_from(E_yy)] += E_y
    return E_y, E_yy


def JSLogdetDiv(X, Y):
    """reference util.py:21-22"""
    return np.log(np.linalg.det((X + Y) / 2)) - 0.5 * np.log(np.linalg.det(X.dot(Y)))


def initializeParams(xdim, ydim, experiment=None):
    """Poisson-PCA initialiser (reference util.py:505-558): moment-matched log-rate covariance ->
    leading eigenvectors -> C; d = log mean rate; tau ~ U(0.1, 0.6) s from the global RNG.  The count moments come
    from the device (countMoments); the ydim x ydim eigen-decomposition stays on the host like the reference's."""
    if experiment is None:
        return {'C': np.random.rand(ydim, xdim) * 2 - 1, 'd': np.random.randn(ydim) * 2 - 2, 'tau': np.random.rand(xdim) * 0.5}
    meanY, covY, _, _ = countMoments(experiment, xdim)
    meanY = meanY + 1e-10
    outer = np.outer(meanY, meanY)
    lamb = np.log(np.abs(covY + outer - np.diag(meanY))) - np.log(outer)
    evals, evecs = np.linalg.eig(lamb)
    order = np.argsort(evals)[::-1]
    return {'C': evecs[:, order][:, :xdim], 'd': np.log(meanY), 'tau': np.random.rand(xdim) * 0.5 + 0.1}


def subspaceAngle(F, G):
    """Largest principal angle between the column spaces of F and G (reference util.py:338-367),
    columns scaled by their maximum entry first as the reference does."""
    F = np.array(F, dtype=np.float64)
    G = np.array(G, dtype=np.float64)
    F = F / np.max(F, axis=0)
    G = G / np.max(G, axis=0)
    QF, _ = np.linalg.qr(F)
    QG, _ = np.linalg.qr(G)
    s = np.linalg.svd(QF.T @ QG, compute_uv=False)
    return float(np.max(np.arccos(np.minimum(s, 1.0))))
