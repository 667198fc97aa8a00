"""Device sessions: one per (experiment, xdim).  Keeps the spike-count tensor, the modes and the
posterior blocks resident in HBM between E-step and M-step calls, and hands lazy views back to
callers that still want the reference's list-of-arrays ``infRes``.

Trial sharding (multi-GPU): when the process was launched one-rank-per-GPU (RANK / WORLD_SIZE /
LOCAL_RANK in the environment, as torch.distributed.run sets them) every rank holds the full
count tensor (uint8, small) and processes a contiguous slice of each trial list; M-step sufficient
statistics are summed with an RCCL all-reduce inside the C-ABI.
"""
import os
import time
import weakref

import numpy as np

from . import _hip


# ----------------------------------------------------------------------------------------------
# process-wide communicator description (rank, world size, unique id exchange)
# ----------------------------------------------------------------------------------------------
class _stdout_to_stderr:
    """RCCL prints a version banner on the process's stdout (file descriptor 1) when the first communicator comes
    up; callers that emit machine-readable output on stdout (bench.py: one JSON line) must not see it there."""

    def __enter__(self):
        import sys
        sys.stdout.flush()
        self._saved = os.dup(1)
        os.dup2(2, 1)
        return self

    def __exit__(self, *exc):
        os.dup2(self._saved, 1)
        os.close(self._saved)
        return False


_PROCESS_START = time.time()


class phase_deadline:
    """Watchdog around a start-up phase that can block for ever inside the library (ncclCommInitRank and the first collective have no
    timeout: one rank that never joins holds all the others).  A helper thread waits for the phase to end; when the deadline passes
    first it writes one line to stderr and ends THIS process with a non-zero status (os._exit: the main thread is stuck in a native
    call and cannot be interrupted; nothing is re-executed) - the launcher then sees a failed rank with a message instead of a job that
    hangs until somebody's outer limit kills it without one."""

    def __init__(self, what, seconds, rank=0, exit_code=13):
        self.what, self.seconds, self.rank, self.exit_code = what, float(seconds), rank, exit_code
        import threading
        self._done = threading.Event()
        self._thread = threading.Thread(target=self._watch, daemon=True)

    def _watch(self):
        if not self._done.wait(self.seconds):
            import sys
            try:
                sys.stderr.write('pgpfa: rank %d: %s did not finish within %.0f s (another rank never joined, or RCCL could not reach it); '
                                 'exiting with status %d\n' % (self.rank, self.what, self.seconds, self.exit_code))
                sys.stderr.flush()
            finally:
                os._exit(self.exit_code)

    def __enter__(self):
        self._thread.start()
        return self

    def __exit__(self, *exc):
        self._done.set()
        return False


class _World:
    def __init__(self):
        self.rank = int(os.environ.get('RANK', '0'))
        self.size = int(os.environ.get('WORLD_SIZE', '1'))
        self.local_rank = int(os.environ.get('LOCAL_RANK', str(self.rank)))
        # PGPFA_FORCE_COMM=1 builds the RCCL communicator even for a single rank (exercises the same code path)
        self.enabled = (self.size > 1 or os.environ.get('PGPFA_FORCE_COMM', '0') == '1') and \
            os.environ.get('PGPFA_DISABLE_COMM', '0') != '1'
        self._serial = 0
        if self.enabled:
            # single-node job: keep RCCL's bootstrap on loopback and off InfiniBand probing (both can stall in
            # containers without a routable interface); explicit user settings win
            os.environ.setdefault('NCCL_SOCKET_IFNAME', 'lo')
            os.environ.setdefault('NCCL_IB_DISABLE', '1')
            os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')

    def device(self):
        return self.local_rank if self.enabled else int(os.environ.get('PGPFA_DEVICE', '0'))

    def exchange_unique_id(self):
        """Rendezvous of this single-node job through files; returns (RCCL unique id, path of the id file).

        Rank 0 removes whatever an earlier attempt left under the same key, creates the unique id and publishes it; every
        other rank reads it and acknowledges WITH ITS CONTENT; rank 0 waits until every acknowledgement carries the id it
        published (an acknowledgement of an older id is not one) and only then publishes the go-ahead, again with the id.
        A non-zero rank never trusts a single read: it keeps re-reading the id file, acknowledges again when the id
        changed under it (it had read a leftover before rank 0 replaced it), and leaves only when the go-ahead carries the
        id it holds - a leftover go-ahead of another attempt is waited out, not an error.  Nobody enters ncclCommInitRank
        (which blocks without a timeout until every rank has joined) before every rank is known to be alive and to hold
        the same id: a rank that died at start-up (bad device, out of memory while creating its context) or was never
        started makes every other rank raise after PGPFA_RDZV_TIMEOUT seconds (default 300) - a non-zero exit of the whole
        job instead of a hang.  File names are keyed by MASTER_PORT, the launcher's run id, its restart count
        (TORCHELASTIC_RESTART_COUNT: a restarted worker group is another attempt) and pid (shared parent of all ranks)
        and a per-process serial.  A file older than this process by more than the timeout cannot belong to this attempt
        (rank 0 gives up that long after publishing) and is ignored.
        Every rank's acknowledgement also carries a random 16-byte nonce of ITS process, and the go-ahead repeats the nonces of
        all ranks next to the id: a non-zero rank leaves only on a go-ahead that holds its own nonce, so the complete leftovers
        of a crashed earlier run under the same key (id file + matching go-ahead: the key repeats when the same shell reruns
        the job on the same port) cannot send it into ncclCommInitRank with a dead id before rank 0 has cleaned up."""
        self._serial += 1
        base = os.environ.get('PGPFA_RDZV_DIR', '/tmp')
        key = 'pgpfa_uid_%s_%s_%s_%d_%d' % (os.environ.get('MASTER_PORT', '0'), os.environ.get('TORCHELASTIC_RUN_ID', 'none'),
                                           os.environ.get('TORCHELASTIC_RESTART_COUNT', '0'), os.getppid(), self._serial)
        path = os.path.join(base, key)
        timeout = float(os.environ.get('PGPFA_RDZV_TIMEOUT', '300'))
        deadline = time.time() + timeout

        def publish(name, payload):
            tmp = name + '.tmp.%d' % os.getpid()
            with open(tmp, 'wb') as fh:
                fh.write(payload)
            os.replace(tmp, name)

        def read_fresh(name):
            """Content of a file that can belong to this attempt, else None."""
            try:
                if os.path.getmtime(name) < _PROCESS_START - timeout - 5.0:
                    return None
                with open(name, 'rb') as fh:
                    return fh.read()
            except OSError:
                return None

        def timed_out(what, names):
            return _hip.HipBackendError('rendezvous of rank %d timed out after %.0f s waiting for %s (%s): a rank died at start-up or was '
                                        'never launched' % (self.rank, timeout, what, ', '.join(os.path.basename(m) for m in names)))
        acks = [path + '.ack.%d' % r for r in range(1, self.size)]
        nonce = os.urandom(16)
        if self.rank == 0:
            for stale in [path, path + '.go'] + acks:
                try:
                    os.remove(stale)
                except OSError:
                    pass
            uid = _hip.comm_unique_id()
            publish(path, uid)
            while True:
                got = [read_fresh(nm) for nm in acks]
                missing = [nm for nm, a in zip(acks, got) if a is None or len(a) != 144 or a[:128] != uid]
                if not missing:
                    break
                if time.time() >= deadline:
                    try:
                        os.remove(path)
                    except OSError:
                        pass
                    raise timed_out('the acknowledgement of every rank', missing)
                time.sleep(0.01)
            publish(path + '.go', uid + b''.join(a[128:] for a in got))
            for nm in acks:
                try:
                    os.remove(nm)
                except OSError:
                    pass
            return uid, path
        held = None
        while True:
            uid = read_fresh(path)
            if uid is not None and len(uid) == 128:
                if uid != held:
                    publish(path + '.ack.%d' % self.rank, uid + nonce)
                    held = uid
                go = read_fresh(path + '.go')
                if go is not None and len(go) == 128 + 16 * (self.size - 1) and go[:128] == held and \
                        go[128 + 16 * (self.rank - 1):128 + 16 * self.rank] == nonce:
                    # the go-ahead is written after every rank acknowledged THIS id, and it names this process: not a leftover
                    return held, path
            if time.time() >= deadline:
                raise timed_out("rank 0's unique id" if held is None else "rank 0's go-ahead", [path if held is None else path + '.go'])
            time.sleep(0.01)


WORLD = _World()


def cleanup_rendezvous(path):
    """After the first collective (which every rank has passed) rank 0 removes the rendezvous files."""
    if WORLD.rank == 0:
        for name in (path, path + '.go'):
            try:
                os.remove(name)
            except OSError:
                pass


def shard_slice(n_items, rank, size):
    """Contiguous block partition of range(n_items): the first (n_items % size) ranks get one more."""
    base, rem = divmod(n_items, size)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


# ----------------------------------------------------------------------------------------------
# lazy, device-backed sequences (duck-type the reference's per-trial lists)
# ----------------------------------------------------------------------------------------------
class LazyTrialList:
    """Behaves like the reference's list of per-trial arrays; entry i is fetched from HBM on first use."""

    def __init__(self, n, fetch):
        self._n = n
        self._fetch = fetch
        self._cache = {}

    def __len__(self):
        return self._n

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(self._n))]
        if i < 0:
            i += self._n
        if not 0 <= i < self._n:
            raise IndexError(i)
        if i not in self._cache:
            self._cache[i] = self._fetch(i)
        return self._cache[i]

    def __iter__(self):
        return (self[i] for i in range(self._n))


class DeviceInfRes(dict):
    """infRes dict of inference.laplace / dualVariational (inference.py:176-180) whose four entries
    are lazy views of device-resident results.  Carries the session and the trial list so that
    learning.updateParams* can run the M-step without the data ever leaving HBM."""

    # Laplace log evidence of the trials of this rank (float64 array, order of the entries) and its mean over all ranks' trials: host values that
    # inference.laplace sets while inference.LAPLACE_EVIDENCE is on; None otherwise
    log_evidence = None
    mean_log_evidence = None

    def __init__(self, session, trial_idx, local_pos):
        super().__init__()
        self.session = session
        self.trial_idx = np.asarray(trial_idx, dtype=np.int32)       # trials this rank processed
        self.stamp = session.post_stamp
        ctx = session.ctx
        n = len(self.trial_idx)
        tid = self.trial_idx
        self.local_positions = local_pos                              # positions in the caller's trial list
        # (trials of unequal length: the device keeps every trial padded to the longest; an entry is cut to the trial's own bins)
        cut = session.cut
        self['post_mean'] = LazyTrialList(n, lambda i: self._fresh(i, 'post_mean') and cut('post_mean', tid[i], ctx.post_mean(tid[i:i + 1])[0]))
        self['post_vsm'] = LazyTrialList(n, lambda i: self._fresh(i, 'post_vsm') and cut('post_vsm', tid[i], ctx.post_vsm(tid[i:i + 1])[0]))
        self['post_vsmGP'] = LazyTrialList(n, lambda i: self._fresh(i, 'post_vsmGP') and cut('post_vsmGP', tid[i], ctx.post_vsmgp(tid[i:i + 1])[0]))
        self['post_cov'] = LazyTrialList(n, lambda i: self._fresh(i, 'post_cov') and cut('post_cov', tid[i], ctx.post_cov(int(tid[i]))))

    def _fresh(self, i, what):
        """The reference returns immutable per-trial arrays; here entry i is a view of device memory that the next
        E-step touching the same trial overwrites in place.  Reading it afterwards must fail, not return the newer
        posterior under the old name (entries already fetched, or snapshotted with materialize(), stay valid)."""
        if self.session.trial_stamp[self.trial_idx[i]] != self.stamp:
            raise _hip.HipBackendError("infRes['%s'][%d] belongs to a superseded E-step: trial %d has been overwritten on the "
                                       'device by a later one (call infRes.materialize() before running it to keep a host copy)'
                                       % (what, i, int(self.trial_idx[i])))
        return True

    def materialize(self, keys=('post_mean', 'post_vsm')):
        """Snapshot the listed entries to host arrays (bulk download) so that they survive later E-steps on the same
        session, like the reference's per-trial arrays do."""
        n = len(self.trial_idx)
        if n == 0:
            return self
        fetch = {'post_mean': self.session.ctx.post_mean, 'post_vsm': self.session.ctx.post_vsm, 'post_vsmGP': self.session.ctx.post_vsmgp}
        for key in keys:
            lst = self[key]
            missing = [i for i in range(n) if i not in lst._cache]
            if not missing:
                continue
            for i in missing:
                self._fresh(i, key)
            step = max(1, (1 << 28) // max(1, {'post_mean': self.session.p * self.session.T, 'post_vsm': self.session.T * self.session.p ** 2,
                                               'post_vsmGP': self.session.T ** 2 * self.session.p}[key] * 8))
            for c0 in range(0, len(missing), step):
                part = missing[c0:c0 + step]
                arr = fetch[key](self.trial_idx[part])
                for j, i in enumerate(part):
                    lst._cache[i] = self.session.cut(key, self.trial_idx[i], arr[j]).copy()
        return self

    def host_bytes(self, keys=('post_mean', 'post_vsm')):
        per = {'post_mean': self.session.p * self.session.T, 'post_vsm': self.session.T * self.session.p ** 2,
               'post_vsmGP': self.session.T ** 2 * self.session.p}
        return 8 * len(self.trial_idx) * sum(per[k] for k in keys)


class DeviceOptimRes(LazyTrialList):
    """lapOptimRes (inference.py:92,127): the modes, flattened; resident on device for warm starts."""

    def __init__(self, session, trial_idx):
        tid = np.asarray(trial_idx, dtype=np.int32)
        ctx = session.ctx
        super().__init__(len(tid), lambda i: self._fresh(i) and session.cut('post_mean', tid[i], ctx.post_mean(tid[i:i + 1])[0]).reshape(-1))
        self.session = session
        self.trial_idx = tid
        self.stamp = session.mode_stamp
        self.post_stamp = session.post_stamp

    def _fresh(self, i):
        if self.session.trial_stamp[self.trial_idx[i]] != self.post_stamp:
            raise _hip.HipBackendError('lapOptimRes[%d] belongs to a superseded E-step: the mode of trial %d has been overwritten '
                                       'on the device by a later one' % (i, int(self.trial_idx[i])))
        return True


def log_live(lam):
    """log of dual variables in their padded layout: entries that are not live hold lambda = 0 (inference.DUAL_MASKED) and come back as rho = 0."""
    lam = np.asarray(lam, dtype=np.float64)
    if np.all(lam > 0.0):
        return np.log(lam)
    live = lam > 0.0
    return np.where(live, np.log(np.where(live, lam, 1.0)), 0.0)


class DeviceDualOptimRes(LazyTrialList):
    """varOptimRes of inference.dualVariational (inference.py:326 / 398: the optimal lambda, or rho = log lambda, per trial) left on the
    device: an entry is downloaded when it is read, and handed back as prevOptimRes of the next call on the same trials it is a warm start that
    moves no bytes (at config 5 a trial's entry is 4 MB: 1 GB per 256 trials each way).  Like the lazy infRes entries it is a VIEW: the next
    variational E-step on a trial overwrites its lambda in place, and reading the entry afterwards raises instead of returning the newer
    optimum under the old name (entries already read, or snapshotted with materialize(), stay valid)."""

    def __init__(self, session, trial_idx, log):
        tid = np.asarray(trial_idx, dtype=np.int32)
        ctx = session.ctx
        super().__init__(len(tid), lambda i: self._fresh(i) and (log_live(ctx.dual_lambda(tid[i:i + 1])[0]) if log else ctx.dual_lambda(tid[i:i + 1])[0]))
        self.session = session
        self.trial_idx = tid
        self.log = bool(log)
        self.stamp = session.mode_stamp
        self.dual_stamp = session.dual_stamp

    def _fresh(self, i):
        if self.session.dual_trial_stamp[self.trial_idx[i]] != self.dual_stamp:
            raise _hip.HipBackendError('varOptimRes[%d] belongs to a superseded variational E-step: the dual variables of trial %d have been '
                                       'overwritten on the device by a later one (call materialize() on the list before running it to keep a '
                                       'host copy)' % (i, int(self.trial_idx[i])))
        return True

    def materialize(self):
        """Host copies of every entry not read yet (one bulk download per 256 MB)."""
        missing = [i for i in range(len(self)) if i not in self._cache]
        if not missing:
            return self
        for i in missing:
            self._fresh(i)
        step = max(1, (1 << 28) // max(1, self.session.q * self.session.T * 8))
        for c0 in range(0, len(missing), step):
            part = missing[c0:c0 + step]
            lam = self.session.ctx.dual_lambda(self.trial_idx[part])
            for j, i in enumerate(part):
                self._cache[i] = log_live(lam[j]) if self.log else lam[j].copy()
        return self


# ----------------------------------------------------------------------------------------------
class Session:
    lengths = observed = observed_bins = None                # no table set (what a session object made without __init__ sees too)

    def __init__(self, Y, p, bin_ms, lengths=None, observed=None):
        R, q, T = Y.shape
        self.R, self.q, self.T, self.p = R, q, T, p
        # per-trial bin counts, or None when every trial has T bins (then nothing below differs from a context without the table)
        self.lengths = None
        if lengths is not None and np.any(np.asarray(lengths) != T):
            self.lengths = np.asarray(lengths, dtype=np.int32).reshape(-1)
            if self.lengths.shape != (R,):
                raise ValueError('one length per trial expected')
        # observation table (R, q) of booleans, or None when every neuron was recorded on every trial (then no table is set: the equal path)
        self.observed = None
        if observed is not None and not np.all(observed):
            self.observed = check_observed(observed, R, q)
        self.observed_bins = None                            # per-bin table (R, q, T) of booleans: set_observed_bins
        self.ctx = _hip.Context(q, p, T, R, bin_ms, device=WORLD.device())
        self.ctx.upload_counts(Y)
        if self.lengths is not None:
            self.ctx.set_trial_lengths(self.lengths)
        if self.observed is not None:
            self.ctx.set_observed(self.observed)
        self.post_stamp = 0
        self.mode_stamp = 0
        self.trial_stamp = np.zeros(R, dtype=np.int64)      # post_stamp of the E-step that last wrote each trial's posterior
        self.dual_stamp = 0
        self.dual_trial_stamp = np.zeros(R, dtype=np.int64)  # dual_stamp of the variational E-step that last wrote each trial's dual variables
        self.rank, self.size = 0, 1
        self.comm_ready = False
        if WORLD.enabled:
            import sys
            limit = float(os.environ.get('PGPFA_COMM_TIMEOUT', '300'))
            with _stdout_to_stderr():
                uid, path = WORLD.exchange_unique_id()
                # (every rank is known to be alive and to hold this id; what can still block is RCCL itself: bounded by a watchdog)
                with phase_deadline('pgpfa_comm_init (ncclCommInitRank)', limit, WORLD.rank):
                    self.ctx.comm_init(uid, WORLD.rank, WORLD.size)
                self.rank, self.size = WORLD.rank, WORLD.size
                self.comm_ready = True
                # first collective doubles as the barrier after which rank 0 may remove the file
                with phase_deadline('the first all-reduce', limit, WORLD.rank):
                    ones = self.ctx.allreduce_host(np.ones(1))
                # one line per rank for the launcher's log: which device, which PCI function, how many ranks RCCL itself saw
                sys.stderr.write('pgpfa: %s first_allreduce_sum %g\n' % (self.ctx.comm_describe(), float(ones[0])))
                sys.stderr.flush()
                if int(round(float(ones[0]))) != WORLD.size:
                    raise _hip.HipBackendError('first all-reduce over %d ranks summed to %g' % (WORLD.size, float(ones[0])))
            cleanup_rendezvous(path)

    def set_params(self, params):
        self.ctx.set_params(params['C'], params['d'], params['tau'])

    def set_observed_bins(self, table):
        """Give the session a per-bin table (R, q, T) of booleans, True = recorded, on top of its lengths and observation table (None drops it).  A
        table that marks every entry inside those two as recorded is dropped here: no table is set and the path is that of the other two alone.
        Resident posteriors are superseded, as by any change of the data.  ValueError for a wrong shape or a trial / neuron left without a live
        entry, before anything reaches the device."""
        if table is not None:
            table = compose_observed_bins(table, self.lengths, self.observed, self.R, self.q, self.T)
        self._install_observed_bins(table)

    def _install_observed_bins(self, table):
        """set_observed_bins for a table that compose_observed_bins has returned already (session_for checks it before anything is uploaded)."""
        if table is None and self.observed_bins is None:
            return
        if table is not None and self.comm_ready:
            # (the moments all-reduce s and S over the ranks, the live and co-live counts would have to follow)
            raise NotImplementedError('a per-bin observation table is not supported on a sharded session yet')
        self.ctx.set_observed_bins(table)
        self.observed_bins = table
        self.mark_written(np.arange(self.R))

    def cut(self, key, trial, arr):
        """The padded device entry `arr` of `trial` restricted to the trial's own T_r bins: post_mean (p, T_r), post_vsm (T_r, p, p),
        post_vsmGP (T_r, T_r, p), post_cov the p T_r x p T_r sub-matrix (latent-major).  Equal trials: `arr` itself."""
        if self.lengths is None:
            return arr
        L = int(self.lengths[int(trial)])
        if L == self.T:
            return arr
        if key == 'post_mean':
            return np.ascontiguousarray(arr[:, :L])
        if key == 'post_vsm':
            return np.ascontiguousarray(arr[:L])
        if key == 'post_vsmGP':
            return np.ascontiguousarray(arr[:L, :L])
        if key == 'post_cov':
            keep = (np.arange(self.p)[:, None] * self.T + np.arange(L)[None, :]).reshape(-1)
            return np.ascontiguousarray(arr[np.ix_(keep, keep)])
        raise KeyError(key)

    def pad_modes(self, trials, rows):
        """Host modes of the listed trials as one (n, p*T) array.  With trials of unequal length an entry may have the trial's own
        p*T_r values (what lapOptimRes returns): its padded bins start at zero."""
        if self.lengths is None:
            return np.stack([np.asarray(x, dtype=np.float64).reshape(-1) for x in rows])
        X = np.zeros((len(rows), self.p, self.T))
        for j, (t, x) in enumerate(zip(trials, rows)):
            x = np.asarray(x, dtype=np.float64).reshape(-1)
            L = int(self.lengths[int(t)])
            if x.size == self.p * L:
                X[j, :, :L] = x.reshape(self.p, L)
            elif x.size == self.p * self.T:
                X[j] = x.reshape(self.p, self.T)
            else:
                raise ValueError('prevOptimRes entry %d has %d values; trial %d has %d bins (xdim*T_r = %d)' % (j, x.size, int(t), L, self.p * L))
        return X.reshape(len(rows), -1)

    def live_mask(self, trials):
        """Boolean (n, q*T) array over the padded dual variables of the listed trials: True where entry (neuron, bin) has a likelihood term - the bin
        lies inside the trial's own T_r bins and the neuron was recorded on the trial.  None when no table is set (every entry is live)."""
        if self.lengths is None and self.observed is None and self.observed_bins is None:
            return None
        trials = np.asarray(trials, dtype=np.int64)
        live = _inside(None if self.lengths is None else self.lengths[trials], None if self.observed is None else self.observed[trials],
                       len(trials), self.q, self.T)
        if self.observed_bins is not None:
            live &= self.observed_bins[trials]
        return live.reshape(len(trials), -1)

    def live_entries(self):
        """Boolean (R, q, T) array of the entries that carry a likelihood term: lengths, observation table and per-bin table by AND."""
        live = self.live_mask(np.arange(self.R))
        return np.ones((self.R, self.q, self.T), dtype=bool) if live is None else live.reshape(self.R, self.q, self.T)

    def refuse_tables(self, what, allow=()):
        """Entry points must not run on a table they do not know as if its padding, zero-filled rows or zero-filled entries were data.  allow: the
        tables `what` understands, of 'lengths', 'observed', 'observed_bins'."""
        if self.lengths is not None and 'lengths' not in allow:
            raise NotImplementedError('%s does not support trials of unequal length yet (this experiment has %d..%d bins per trial); '
                                      'only the Laplace EM path does' % (what, int(self.lengths.min()), int(self.lengths.max())))
        if self.observed is not None and 'observed' not in allow:
            raise NotImplementedError('%s does not support unobserved neurons yet (this experiment has %d unobserved (trial, neuron) pairs); '
                                      'only the Laplace EM path does' % (what, int((~self.observed).sum())))
        if self.observed_bins is not None and 'observed_bins' not in allow:
            raise NotImplementedError('%s does not support a per-bin observation table yet (this experiment has %d entries marked as not recorded by '
                                      "'observedBins'); only the Laplace EM path does" % (what, int((~self.observed_bins).sum())))

    def mark_dual_written(self, trial_idx):
        """A variational E-step has just overwritten the resident dual variables of these trials."""
        self.dual_stamp += 1
        self.dual_trial_stamp[np.asarray(trial_idx, dtype=np.int64)] = self.dual_stamp

    def mark_written(self, trial_idx):
        """An E-step (or an uploaded posterior) has just overwritten the device state of these trials."""
        self.post_stamp += 1
        self.mode_stamp += 1
        self.trial_stamp[np.asarray(trial_idx, dtype=np.int64)] = self.post_stamp

    def local_slice(self, n_items):
        return shard_slice(n_items, self.rank, self.size)

    def allreduce(self, arr):
        return self.ctx.allreduce_host(arr) if self.comm_ready else np.asarray(arr, dtype=np.float64)


_sessions = weakref.WeakKeyDictionary()


def check_observed(observed, R, q):
    """The observation table as a boolean (R, q) array; ValueError on a wrong shape, a trial without an observed neuron or a neuron that no
    trial observes (nothing has been uploaded yet when this runs)."""
    ob = np.asarray(observed)
    if ob.shape != (R, q):
        raise ValueError('observation table must have shape (trials, ydim) = (%d, %d), got %s' % (R, q, ob.shape))
    ob = ob != 0
    empty = np.flatnonzero(~ob.any(axis=1))
    if empty.size:
        raise ValueError('trial %d has no observed neuron' % int(empty[0]))
    never = np.flatnonzero(~ob.any(axis=0))
    if never.size:
        raise ValueError('neuron %d is observed on no trial' % int(never[0]))
    return np.ascontiguousarray(ob)


def _inside(lengths, observed, R, q, T):
    """Boolean (R, q, T) array: True at the bins inside the trials' lengths (None: all T) of the neurons the observation table (None: all) records."""
    live = np.ones((R, q, T), dtype=bool)
    if lengths is not None:
        live &= (np.arange(T)[None, :] < np.asarray(lengths).reshape(-1)[:, None])[:, None, :]
    if observed is not None:
        live &= np.asarray(observed, dtype=bool)[:, :, None]
    return live


def compose_observed_bins(table, lengths, observed, R, q, T):
    """The per-bin table as a contiguous boolean (R, q, T) array, or None when it marks every entry inside the lengths (may be None) and the
    observation table (may be None) as recorded.  ValueError for a wrong shape, and for a trial or a neuron that the three tables together leave
    without a live entry (nothing has been uploaded yet when this runs)."""
    ob = np.asarray(table)
    if ob.shape != (R, q, T):
        raise ValueError('per-bin table must have shape (trials, ydim, T) = (%d, %d, %d), got %s' % (R, q, T, ob.shape))
    ob = ob != 0
    base = _inside(lengths, observed, R, q, T)
    if np.all(ob[base]):
        return None
    live = ob & base
    empty = np.flatnonzero(~live.any(axis=(1, 2)))
    if empty.size:
        raise ValueError('trial %d has no live entry: every (neuron, bin) of it is marked as not recorded' % int(empty[0]))
    never = np.flatnonzero(~live.any(axis=(0, 2)))
    if never.size:
        raise ValueError('neuron %d has no live entry on any trial' % int(never[0]))
    return np.ascontiguousarray(ob)


def _stack_observed_bins(experiment):
    """Per-bin table (R, ydim, T) of experiment.data, booleans, T the longest trial: trial r holds data[r]['observedBins'] (ydim, T_r), all True for
    a trial without the key and False behind a shorter trial's own bins; None when no trial carries the key.  ValueError for a wrong shape."""
    rows = [tr.get('observedBins') if hasattr(tr, 'get') else None for tr in experiment.data]
    if all(o is None for o in rows):
        return None
    shapes = [np.asarray(tr['Y']).shape for tr in experiment.data]
    q, T = shapes[0][0], max(sh[1] for sh in shapes if len(sh) == 2)
    table = np.zeros((len(rows), q, T), dtype=bool)
    for r, o in enumerate(rows):
        if len(shapes[r]) != 2:
            continue                                     # (reported by _stack_counts)
        if o is None:
            table[r, :, :shapes[r][1]] = True
            continue
        o = np.asarray(o)
        if o.shape != tuple(shapes[r]):
            raise ValueError("trial %d: 'observedBins' must have the shape of 'Y', (ydim, T) = %s, got %s" % (r, tuple(shapes[r]), o.shape))
        table[r, :, :shapes[r][1]] = o != 0
    return table


def _stack_observed(experiment):
    """Observation table (R, ydim) of experiment.data, booleans: row r is data[r]['observed'] (all True for a trial without the key), or None
    when no trial carries the key.  Raises ValueError for a wrong shape, a trial without an observed neuron or a neuron never observed."""
    rows = [tr.get('observed') if hasattr(tr, 'get') else None for tr in experiment.data]
    if all(o is None for o in rows):
        return None
    q = np.asarray(experiment.data[0]['Y']).shape[0]
    table = np.ones((len(rows), q), dtype=bool)
    for r, o in enumerate(rows):
        if o is None:
            continue
        o = np.asarray(o)
        if o.shape != (q,):
            raise ValueError("trial %d: 'observed' must have shape (ydim,) = (%d,), got %s" % (r, q, o.shape))
        table[r] = o != 0
    return check_observed(table, len(rows), q)


def _observed_filled(tr, y):
    """y with the rows that data[r]['observed'] marks as not recorded, and the entries that data[r]['observedBins'] marks so, set to zero (a copy; NaN
    is accepted there only)."""
    b = tr.get('observedBins') if hasattr(tr, 'get') else None
    if b is not None:
        b = np.asarray(b)
        if b.shape == y.shape and not np.all(b != 0):    # (a wrong shape is reported by _stack_observed_bins)
            y = np.array(y, copy=True)
            y[b == 0] = 0
    o = tr.get('observed') if hasattr(tr, 'get') else None
    if o is None:
        return y
    o = np.asarray(o)
    if o.shape != (y.shape[0],) or np.all(o != 0):
        return y                                         # (a wrong shape is reported by _stack_observed)
    y = np.array(y, copy=True)
    y[o == 0] = 0
    return y


def _stack_counts(experiment):
    """(counts [R][q][T], lengths [R]) of experiment.data: T is the longest trial, shorter trials are padded with zeros behind their
    own T_r bins.  Raises ValueError for a trial without bins or trials with different numbers of neurons."""
    trials = [np.asarray(tr['Y']) for tr in experiment.data]
    for r, y in enumerate(trials):
        if y.ndim == 2:
            trials[r] = y = _observed_filled(experiment.data[r], y)      # the resident copy holds zeros where a neuron was not recorded
        if y.ndim != 2:
            raise ValueError("trial %d: 'Y' must be (ydim, T), got shape %s" % (r, y.shape))
        if y.shape[0] != trials[0].shape[0]:
            raise ValueError('trial %d has %d neurons, trial 0 has %d' % (r, y.shape[0], trials[0].shape[0]))
        if y.shape[1] < 1:
            raise ValueError('trial %d has no bins' % r)
    lengths = np.asarray([y.shape[1] for y in trials], dtype=np.int32)
    if np.all(lengths == lengths[0]):
        Y = np.stack(trials)
    else:
        Y = np.zeros((len(trials), trials[0].shape[0], int(lengths.max())), dtype=np.result_type(*trials))
        for r, y in enumerate(trials):
            Y[r, :, :y.shape[1]] = y
    return _pack_counts(Y), lengths


def _pack_counts(Y):
    if Y.min() >= 0 and Y.max() <= 65535 and np.all(Y == np.floor(Y)):
        return Y.astype(np.uint8 if Y.max() <= 255 else np.uint16)
    return Y.astype(np.float64)            # (the C-ABI rejects it with the reason)


def session_for(experiment, p):
    """Return (session, trial indices of `experiment` inside the session's count tensor).

    Sub-sampled experiments produced by funs.util.subsampleTrials carry `_pgpfa_parent` and
    `batchTrIdx`, so minibatches reuse the parent's resident tensor instead of re-uploading."""
    parent = getattr(experiment, '_pgpfa_parent', None)
    if parent is not None and hasattr(experiment, 'batchTrIdx'):
        sess, _ = session_for(parent, p)
        return sess, np.asarray(experiment.batchTrIdx, dtype=np.int32)
    per_exp = _sessions.get(experiment)
    if per_exp is None:
        per_exp = {}
        _sessions[experiment] = per_exp
    n_trials = len(experiment.data)
    sess = per_exp.get(p)
    if sess is None or sess.R != n_trials:
        observed = _stack_observed(experiment)            # (before anything is uploaded: a bad table raises ValueError here)
        bins = _stack_observed_bins(experiment)
        Y, lengths = _stack_counts(experiment)
        if bins is not None:                              # (still before anything is uploaded)
            bins = compose_observed_bins(bins, lengths if np.any(lengths != Y.shape[2]) else None, observed, Y.shape[0], Y.shape[1], Y.shape[2])
        sess = Session(Y, p, float(experiment.binSize), lengths, observed)
        sess._install_observed_bins(bins)
        per_exp[p] = sess
    return sess, np.arange(n_trials, dtype=np.int32)


def drop_sessions(experiment=None):
    """Free device memory held for `experiment` (or for every experiment)."""
    if experiment is None:
        for per_exp in list(_sessions.values()):
            for s in per_exp.values():
                s.ctx.close()
        _sessions.clear()
    elif experiment in _sessions:
        for s in _sessions[experiment].values():
            s.ctx.close()
        del _sessions[experiment]
