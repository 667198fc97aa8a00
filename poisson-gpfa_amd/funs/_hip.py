"""ctypes binding of libpgpfa_hip.so (C-ABI declared in include/pgpfa.h).

The product path has NO CPU fallback: if the shared library is missing, or no MI355X is
visible, every compute entry point raises.  Build the library with
``python -c "import __graft_entry__ as g; g.build()"`` (hipcc --offload-arch=gfx950).
"""
import ctypes as ct
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), 'libpgpfa_hip.so')

c_double_p = ct.POINTER(ct.c_double)
c_int32_p = ct.POINTER(ct.c_int32)
c_uint8_p = ct.POINTER(ct.c_uint8)
c_int64_p = ct.POINTER(ct.c_int64)

# name -> (argtypes); every function returns int except where noted
_SIGNATURES = {
    'pgpfa_version': [],
    'pgpfa_device_count': [ct.POINTER(ct.c_int)],
    'pgpfa_create': [ct.POINTER(ct.c_void_p), ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_double],
    'pgpfa_destroy': [ct.c_void_p],
    'pgpfa_set_option': [ct.c_void_p, ct.c_char_p, ct.c_double],
    'pgpfa_get_info': [ct.c_void_p, ct.c_char_p, c_double_p],
    'pgpfa_upload_counts_f64': [ct.c_void_p, c_double_p],
    'pgpfa_upload_counts_u8': [ct.c_void_p, c_uint8_p],
    'pgpfa_upload_counts_u16': [ct.c_void_p, ct.POINTER(ct.c_uint16)],
    'pgpfa_set_trial_lengths': [ct.c_void_p, c_int32_p],
    'pgpfa_set_observed': [ct.c_void_p, c_uint8_p],
    'pgpfa_set_observed_bins': [ct.c_void_p, c_uint8_p],
    'pgpfa_get_counts_u16': [ct.c_void_p, ct.c_int, c_int32_p, ct.POINTER(ct.c_uint16)],
    'pgpfa_set_params': [ct.c_void_p, c_double_p, c_double_p, c_double_p],
    'pgpfa_get_gram': [ct.c_void_p, c_double_p],
    'pgpfa_get_gram_inverse': [ct.c_void_p, c_double_p],
    'pgpfa_laplace_eval': [ct.c_void_p, ct.c_int, c_int32_p, c_double_p, c_double_p, c_double_p],
    'pgpfa_laplace_hessian': [ct.c_void_p, ct.c_int, c_double_p, c_double_p],
    'pgpfa_estep_laplace': [ct.c_void_p, ct.c_int, c_int32_p, ct.c_int, c_double_p, c_int32_p, c_int32_p],
    'pgpfa_set_modes': [ct.c_void_p, ct.c_int, c_int32_p, c_double_p],
    'pgpfa_get_post_mean': [ct.c_void_p, ct.c_int, c_int32_p, c_double_p],
    'pgpfa_get_post_vsm': [ct.c_void_p, ct.c_int, c_int32_p, c_double_p],
    'pgpfa_get_post_vsmgp': [ct.c_void_p, ct.c_int, c_int32_p, c_double_p],
    'pgpfa_get_post_cov': [ct.c_void_p, ct.c_int, c_double_p],
    'pgpfa_get_log_evidence': [ct.c_void_p, ct.c_int, c_int32_p, c_double_p],
    'pgpfa_set_posterior': [ct.c_void_p, ct.c_int, c_int32_p, c_double_p, c_double_p, c_double_p],
    'pgpfa_posterior_rates': [ct.c_void_p, ct.c_int, c_int32_p, c_int32_p, ct.c_int, c_double_p, c_double_p, c_double_p, c_double_p, c_int32_p],
    'pgpfa_posterior_sample': [ct.c_void_p, ct.c_int, c_int32_p, ct.c_int, ct.c_ulonglong, c_double_p, c_double_p, c_double_p, ct.POINTER(ct.c_uint16), c_int32_p],
    'pgpfa_importance_weights': [ct.c_void_p, ct.c_int, c_int32_p, ct.c_int, ct.c_ulonglong, c_double_p, c_double_p, c_double_p],
    'pgpfa_posterior_at': [ct.c_void_p, ct.c_int, c_int32_p, ct.c_int, c_double_p, ct.c_int, c_double_p, c_double_p],
    'pgpfa_posterior_cov_at': [ct.c_void_p, ct.c_int, c_int32_p, ct.c_int, c_double_p, ct.c_int, c_double_p, c_double_p, c_double_p, c_double_p],
    'pgpfa_posterior_velocity_at': [ct.c_void_p, ct.c_int, c_int32_p, ct.c_int, c_double_p, ct.c_int] + [c_double_p] * 5,
    'pgpfa_posterior_functionals': [ct.c_void_p, ct.c_int, c_int32_p, ct.c_int, c_double_p, ct.c_int] + [c_double_p] * 3,
    'pgpfa_count_probabilities': [ct.c_void_p, ct.c_longlong, c_double_p, c_double_p, c_int32_p, ct.c_int, ct.c_double, ct.c_int, c_double_p, c_double_p, c_int32_p,
                                  c_int32_p, c_double_p, c_double_p],
    'pgpfa_posterior_counts': [ct.c_void_p, ct.c_int, c_int32_p, c_int32_p, ct.c_int, ct.c_double, ct.c_int, c_double_p, c_double_p, c_int32_p, c_int32_p,
                               c_double_p, c_double_p],
    'pgpfa_rates_group_csr': [ct.c_int, c_int32_p, ct.c_int, ct.c_int, ct.c_int, c_int32_p, c_int32_p],
    'pgpfa_mstep_cd_costgrad': [ct.c_void_p, c_double_p, c_double_p, ct.c_double, c_double_p, c_double_p],
    'pgpfa_mstep_cd_newton_pass': [ct.c_void_p, c_double_p, c_double_p, ct.c_double, c_double_p, c_double_p, c_double_p],
    'pgpfa_mstep_cd_chord_pass': [ct.c_void_p, c_double_p, c_double_p, ct.c_double, c_double_p, c_double_p, c_double_p],
    'pgpfa_mstep_cd_cost_per_neuron': [ct.c_void_p, c_double_p, c_double_p, ct.c_double, c_double_p],
    'pgpfa_mstep_precomp': [ct.c_void_p, c_double_p],
    'pgpfa_get_pautosum': [ct.c_void_p, c_double_p],
    'pgpfa_mstep_tau_costgrad': [ct.c_void_p, ct.c_int, ct.c_double, c_double_p, c_double_p],
    'pgpfa_mstep_tau_costgrad_batch': [ct.c_void_p, c_double_p, c_double_p, c_double_p],
    'pgpfa_mstep_tau_costgrad_multi': [ct.c_void_p, ct.c_int, c_double_p, c_double_p, c_double_p],
    'pgpfa_mstep_tau_costgrad_multi_begin': [ct.c_void_p, ct.c_int, c_double_p],
    'pgpfa_mstep_tau_costgrad_multi_end': [ct.c_void_p, c_double_p, c_double_p],
    'pgpfa_generate': [ct.c_void_p, ct.c_ulonglong, ct.c_int, c_int32_p, c_double_p, c_uint8_p],
    'pgpfa_loo_predict': [ct.c_void_p, ct.c_int, c_int32_p, c_double_p, c_double_p],
    'pgpfa_count_moments': [ct.c_void_p, ct.c_int, c_int32_p, c_int64_p, c_int64_p, c_int64_p],
    'pgpfa_dual_costgrad': [ct.c_void_p, ct.c_int, c_double_p, c_double_p, c_double_p],
    'pgpfa_dual_costgrad_batch': [ct.c_void_p, ct.c_int, c_int32_p, c_double_p, c_double_p, c_double_p],
    'pgpfa_dual_lbfgs': [ct.c_void_p, ct.c_int, c_int32_p, c_double_p, ct.c_int, ct.c_double, ct.c_double, c_double_p, c_int32_p],
    'pgpfa_get_dual_lambda': [ct.c_void_p, ct.c_int, c_int32_p, c_double_p],
    'pgpfa_dual_fixed_point': [ct.c_void_p, ct.c_int, c_int32_p, c_double_p, ct.c_int, ct.c_int, ct.c_double, c_double_p, c_int32_p, c_int32_p, c_double_p],
    'pgpfa_dual_finalize': [ct.c_void_p, ct.c_int, c_int32_p, c_double_p, c_double_p],
    'pgpfa_dual_post_mean': [ct.c_void_p, ct.c_int, c_double_p, c_double_p],
    'pgpfa_dual_post_cov': [ct.c_void_p, ct.c_int, c_double_p, c_double_p, c_double_p],
    'pgpfa_comm_unique_id': [ct.c_char_p],
    'pgpfa_comm_init': [ct.c_void_p, ct.c_char_p, ct.c_int, ct.c_int],
    'pgpfa_comm_allreduce_host': [ct.c_void_p, c_double_p, ct.c_int],
    'pgpfa_comm_describe': [ct.c_void_p, ct.c_char_p, ct.c_int],
    'pgpfa_test_potrf': [ct.c_void_p, ct.c_int, ct.c_int, c_double_p, c_double_p, c_double_p],
    'pgpfa_test_gemm_nt': [ct.c_void_p, ct.c_int, ct.c_int, ct.c_int, ct.c_double, c_double_p, c_double_p, ct.c_double, c_double_p],
    'pgpfa_test_gemm_nn': [ct.c_void_p, ct.c_int, ct.c_int, ct.c_int, ct.c_double, c_double_p, c_double_p, ct.c_double, c_double_p],
    'pgpfa_test_gemm_nt_f32': [ct.c_void_p, ct.c_int, ct.c_int, ct.c_int, ct.c_double, c_double_p, c_double_p, ct.c_double, c_double_p],
    'pgpfa_test_gemm_nn_f32': [ct.c_void_p, ct.c_int, ct.c_int, ct.c_int, ct.c_double, c_double_p, c_double_p, ct.c_double, c_double_p],
    'pgpfa_test_split_syrk': [ct.c_void_p, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.POINTER(ct.c_float), c_double_p,
                              ct.POINTER(ct.c_int), ct.POINTER(ct.c_int)],
    'pgpfa_test_split_latent_sums': [ct.c_void_p, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_longlong, ct.c_int, ct.c_int, ct.c_longlong, ct.c_int, ct.c_int,
                                     c_double_p, ct.POINTER(ct.c_float), c_double_p, c_double_p],
    'pgpfa_test_thin': [ct.c_void_p, ct.c_int, ct.c_int, ct.c_int, ct.c_int, c_int32_p, ct.c_int, ct.c_longlong, ct.c_longlong, ct.c_int, ct.c_int, ct.c_int,
                        ct.c_int, c_int32_p, ct.c_int, ct.c_int, ct.c_double, c_double_p, c_double_p, ct.c_void_p, ct.c_void_p, c_int32_p, ct.c_int,
                        c_int32_p, c_int32_p, c_int32_p, c_int32_p],
    'pgpfa_test_pivchol': [ct.c_void_p, ct.c_int, ct.c_int, ct.c_int, c_double_p, ct.c_double, ct.c_double, ct.c_double, ct.c_int, ct.c_double, c_double_p,
                           c_int32_p, c_int32_p],
    'pgpfa_test_bin_blocks': [ct.c_void_p, ct.c_int, ct.c_int, ct.c_double, ct.c_int, ct.c_int, c_int32_p, ct.c_longlong, ct.c_longlong, ct.c_double, c_double_p,
                              c_double_p, c_double_p, c_double_p, c_int32_p],
    'pgpfa_test_assemble_b': [ct.c_void_p, ct.c_int, ct.c_int, ct.c_int, c_int32_p, ct.c_int, ct.c_int, ct.c_int, ct.c_int, c_int32_p, ct.c_longlong, ct.c_double,
                              c_double_p, c_double_p, ct.c_void_p, ct.c_int, c_int32_p, ct.c_int, c_int32_p, c_int32_p, c_int32_p, c_int32_p],
    'pgpfa_bench_syrk': [ct.c_void_p, ct.c_int, ct.c_int, ct.c_int, ct.c_int, c_double_p, c_double_p],
    'pgpfa_bench_potrf_diag': [ct.c_void_p, ct.c_int, ct.c_int, ct.c_int, c_double_p],
    'pgpfa_gemm_shape_report': [ct.c_void_p, ct.c_char_p, ct.c_int],
    'pgpfa_bench_mfma_peak': [ct.c_void_p, ct.c_int, c_double_p],
}
EXPORTED_SYMBOLS = sorted(list(_SIGNATURES) + ['pgpfa_last_error'])

_lib = None


class HipBackendError(RuntimeError):
    """Raised when the HIP library is missing, no GPU is visible, or a C-ABI call fails."""


def load_library():
    """Load libpgpfa_hip.so and attach prototypes.  Works without a GPU (symbols only)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipBackendError(
            'libpgpfa_hip.so not found at %s - build it with __graft_entry__.build(); '
            'this package has no CPU fallback' % LIB_PATH)
    lib = ct.CDLL(LIB_PATH)
    for name, argtypes in _SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = ct.c_int
    lib.pgpfa_last_error.argtypes = []
    lib.pgpfa_last_error.restype = ct.c_char_p
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        raise HipBackendError(load_library().pgpfa_last_error().decode('utf-8', 'replace'))


def _check_outputs(want, known, may_be_empty=False):
    """the `want` of a posterior query: only known output names, and at least one"""
    unknown = set(want) - set(known)
    if unknown:
        raise ValueError('unknown output(s) %s' % sorted(unknown))
    if not want and not may_be_empty:
        raise ValueError('no output asked for')


COUNT_OUTPUTS = ('logp', 'pmf', 'lower', 'upper', 'pmean', 'pvar')      # of count_probabilities / posterior_counts, in the order of the C prototypes


def rates_group_csr(group, n_groups, first=0, last=None):
    """(start[n_groups + 1], pos[last - first]): the list positions first..last-1 of every group, in list order (pgpfa_rates_group_csr; host only)."""
    gg = np.ascontiguousarray(group, dtype=np.int32).reshape(-1)
    last = gg.size if last is None else int(last)
    start = np.zeros(int(n_groups) + 1, dtype=np.int32)
    pos = np.zeros(max(last - int(first), 0), dtype=np.int32)
    check(load_library().pgpfa_rates_group_csr(gg.size, iptr(gg), int(n_groups), int(first), last, iptr(start), iptr(pos)))
    return start, pos


def device_count():
    n = ct.c_int(0)
    rc = load_library().pgpfa_device_count(ct.byref(n))
    return n.value if rc == 0 else 0


def dptr(a):
    return a.ctypes.data_as(c_double_p)


def iptr(a):
    return None if a is None else a.ctypes.data_as(c_int32_p)


def as_f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def as_idx(idx):
    if idx is None:
        return None
    return np.ascontiguousarray(idx, dtype=np.int32)


class Context:
    """Thin RAII wrapper over pgpfa_ctx."""

    def __init__(self, q, p, T, R, bin_ms, device=0):
        lib = load_library()
        if device_count() < 1:
            raise HipBackendError('no HIP device visible: the Poisson-GPFA hot path runs on MI355X only '
                                  '(there is no CPU fallback)')
        self.lib = lib
        self.q, self.p, self.T, self.R = int(q), int(p), int(T), int(R)
        self.n = self.p * self.T
        h = ct.c_void_p()
        check(lib.pgpfa_create(ct.byref(h), int(device), self.q, self.p, self.T, self.R, float(bin_ms)))
        self.h = h

    def close(self):
        if getattr(self, 'h', None):
            self.lib.pgpfa_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- options / info --------------------------------------------------------------
    def set_option(self, key, value):
        check(self.lib.pgpfa_set_option(self.h, key.encode(), float(value)))

    def info(self, key):
        v = ct.c_double(0.0)
        check(self.lib.pgpfa_get_info(self.h, key.encode(), ct.byref(v)))
        return v.value

    # -- data ---------------------------------------------------------------------------
    def upload_counts(self, Y):
        Y = np.asarray(Y)
        if Y.shape != (self.R, self.q, self.T):
            raise ValueError('counts must have shape (R,q,T)=%s, got %s' % ((self.R, self.q, self.T), Y.shape))
        if Y.dtype == np.uint8:
            Y = np.ascontiguousarray(Y)
            check(self.lib.pgpfa_upload_counts_u8(self.h, Y.ctypes.data_as(c_uint8_p)))
        elif Y.dtype == np.uint16:
            Y = np.ascontiguousarray(Y)
            check(self.lib.pgpfa_upload_counts_u16(self.h, Y.ctypes.data_as(ct.POINTER(ct.c_uint16))))
        else:
            Y = as_f64(Y)
            check(self.lib.pgpfa_upload_counts_f64(self.h, dptr(Y)))

    def set_trial_lengths(self, lengths):
        """Per-trial bin counts T_r (1..T) of the zero-padded resident counts; None: every trial has T bins again.  Bins t >= T_r of trial r
        then carry no likelihood term (pgpfa_set_trial_lengths); getters keep their padded shapes."""
        if lengths is None:
            check(self.lib.pgpfa_set_trial_lengths(self.h, None))
            return
        ln = np.ascontiguousarray(lengths, dtype=np.int32).reshape(-1)
        if ln.shape != (self.R,):
            raise ValueError('one length per trial expected (R=%d), got %d' % (self.R, ln.size))
        check(self.lib.pgpfa_set_trial_lengths(self.h, iptr(ln)))

    def set_observed(self, observed):
        """Observation table (R, q): non-zero = neuron n was recorded on trial r; None: every neuron on every trial again.  Unobserved (trial, neuron)
        pairs then carry no likelihood term (pgpfa_set_observed); their resident counts must be zero."""
        if observed is None:
            check(self.lib.pgpfa_set_observed(self.h, None))
            return
        ob = np.ascontiguousarray(np.asarray(observed) != 0, dtype=np.uint8)
        if ob.shape != (self.R, self.q):
            raise ValueError('observation table must have shape (R,q)=%s, got %s' % ((self.R, self.q), ob.shape))
        check(self.lib.pgpfa_set_observed(self.h, ob.ctypes.data_as(c_uint8_p)))

    def set_observed_bins(self, live):
        """Per-bin table (R, q, T): non-zero = entry (trial, neuron, bin) was recorded; None drops the table.  Composes with the trial lengths and the
        observation table by AND; entries that are not live carry no likelihood term (pgpfa_set_observed_bins); their resident counts must be zero."""
        if live is None:
            check(self.lib.pgpfa_set_observed_bins(self.h, None))
            return
        lv = np.ascontiguousarray(np.asarray(live) != 0, dtype=np.uint8)
        if lv.shape != (self.R, self.q, self.T):
            raise ValueError('per-bin table must have shape (R,q,T)=%s, got %s' % ((self.R, self.q, self.T), lv.shape))
        check(self.lib.pgpfa_set_observed_bins(self.h, lv.ctypes.data_as(c_uint8_p)))

    def set_params(self, C, d, tau):
        C, d, tau = as_f64(C), as_f64(d).reshape(-1), as_f64(tau).reshape(-1)
        if C.shape != (self.q, self.p) or d.shape != (self.q,) or tau.shape != (self.p,):
            raise ValueError('parameter shapes do not match the context (q=%d, p=%d)' % (self.q, self.p))
        check(self.lib.pgpfa_set_params(self.h, dptr(C), dptr(d), dptr(tau)))

    def gram(self):
        K = np.empty((self.p, self.T, self.T))
        check(self.lib.pgpfa_get_gram(self.h, dptr(K)))
        return K

    def gram_inverse(self):
        K = np.empty((self.p, self.T, self.T))
        check(self.lib.pgpfa_get_gram_inverse(self.h, dptr(K)))
        return K

    # -- Laplace ---------------------------------------------------------------------------
    def _n_idx(self, idx):
        return (self.R, None) if idx is None else (len(idx), as_idx(idx))

    def laplace_eval(self, idx, X, want_grad=True):
        n, ii = self._n_idx(idx)
        X = as_f64(X).reshape(n, self.n)
        f = np.empty(n)
        g = np.empty((n, self.p, self.T)) if want_grad else None
        check(self.lib.pgpfa_laplace_eval(self.h, n, iptr(ii), dptr(X), dptr(f), dptr(g) if want_grad else None))
        return f, g

    def laplace_hessian(self, trial, X):
        X = as_f64(X).reshape(self.n)
        H = np.empty((self.n, self.n))
        check(self.lib.pgpfa_laplace_hessian(self.h, int(trial), dptr(X), dptr(H)))
        return H

    def estep_laplace(self, idx=None, warm_start=False):
        n, ii = self._n_idx(idx)
        obj = ct.c_double(0.0)
        iters = np.zeros(n, dtype=np.int32)
        status = np.zeros(n, dtype=np.int32)
        warm = 2 if warm_start == 'resident' else (1 if warm_start else 0)
        check(self.lib.pgpfa_estep_laplace(self.h, n, iptr(ii), warm, ct.byref(obj), iptr(iters), iptr(status)))
        return obj.value, iters, status

    def count_moments(self, idx=None):
        """Exact integer moments of the resident counts over the listed trials:
        (sum[q], cross[q][q], n_samples) with sum_i = sum y_i, cross_ij = sum y_i y_j over all (trial, bin) samples."""
        n, ii = self._n_idx(idx)
        s = np.zeros(self.q, dtype=np.int64)
        S = np.zeros((self.q, self.q), dtype=np.int64)
        ns = ct.c_int64(0)
        check(self.lib.pgpfa_count_moments(self.h, n, iptr(ii), s.ctypes.data_as(c_int64_p), S.ctypes.data_as(c_int64_p), ct.byref(ns)))
        return s, S, int(ns.value)

    def generate(self, seed, idx=None, want_x=True, want_y=True):
        """Sample latents and counts of the listed trials on the device (they replace the resident counts) -> (X, Y) copies."""
        n, ii = self._n_idx(idx)
        X = np.empty((n, self.p, self.T)) if want_x else None
        check(self.lib.pgpfa_generate(self.h, int(seed), n, iptr(ii), dptr(X) if want_x else None, None))
        Y = self.counts(idx) if want_y else None
        return X, Y

    def counts(self, idx=None):
        """Resident counts of the listed trials: uint8 [n][q][T], or uint16 when some resident count exceeds 255."""
        n, ii = self._n_idx(idx)
        Y = np.empty((n, self.q, self.T), dtype=np.uint16)
        check(self.lib.pgpfa_get_counts_u16(self.h, n, iptr(ii), Y.ctypes.data_as(ct.POINTER(ct.c_uint16))))
        return Y if self.info('counts_two_bytes') else Y.astype(np.uint8)

    def loo_predict(self, idx=None):
        """Leave-one-neuron-out prediction for the listed trials -> (y_pred[n][q][T], summed squared error)."""
        n, ii = self._n_idx(idx)
        out = np.empty((n, self.q, self.T))
        err = ct.c_double(0.0)
        check(self.lib.pgpfa_loo_predict(self.h, n, iptr(ii), dptr(out), ct.byref(err)))
        return out, err.value

    def set_modes(self, idx, X):
        n, ii = self._n_idx(idx)
        X = as_f64(X).reshape(n, self.n)
        check(self.lib.pgpfa_set_modes(self.h, n, iptr(ii), dptr(X)))

    def post_mean(self, idx=None):
        n, ii = self._n_idx(idx)
        out = np.empty((n, self.p, self.T))
        check(self.lib.pgpfa_get_post_mean(self.h, n, iptr(ii), dptr(out)))
        return out

    def log_evidence(self, idx=None):
        """Laplace log evidence log Z_r of the listed trials (all: None), float64 [n]: what the last estep_laplace over them left while option
        'laplace_evidence' was 1 (include/pgpfa.h: pgpfa_get_log_evidence).  Raises HipBackendError for a trial without a valid value."""
        n, ii = self._n_idx(idx)
        out = np.empty(n)
        check(self.lib.pgpfa_get_log_evidence(self.h, n, iptr(ii), dptr(out)))
        return out

    def post_vsm(self, idx=None):
        n, ii = self._n_idx(idx)
        out = np.empty((n, self.T, self.p, self.p))
        check(self.lib.pgpfa_get_post_vsm(self.h, n, iptr(ii), dptr(out)))
        return out

    def post_vsmgp(self, idx=None):
        n, ii = self._n_idx(idx)
        out = np.empty((n, self.T, self.T, self.p))
        check(self.lib.pgpfa_get_post_vsmgp(self.h, n, iptr(ii), dptr(out)))
        return out

    def post_cov(self, trial):
        out = np.empty((self.n, self.n))
        check(self.lib.pgpfa_get_post_cov(self.h, int(trial), dptr(out)))
        return out

    def set_posterior(self, idx, post_mean, post_vsm, post_vsmgp=None):
        n, ii = self._n_idx(idx)
        m = as_f64(post_mean).reshape(n, self.n)
        v = as_f64(post_vsm).reshape(n, self.T * self.p * self.p)
        g = None if post_vsmgp is None else as_f64(post_vsmgp).reshape(n, self.T * self.T * self.p)
        check(self.lib.pgpfa_set_posterior(self.h, n, iptr(ii), dptr(m), dptr(v), None if g is None else dptr(g)))

    def posterior_rates(self, idx=None, group=None, n_groups=0, want=('eta', 'var')):
        """Posterior log-rate moments of the listed trials under the resident posterior and parameters (include/pgpfa.h: pgpfa_posterior_rates).
        want: any of 'eta' [n][q][T], 'var' [n][q][T], 'ell' [n][q], 'group_sum' [n_groups][q][T], 'group_count' [n_groups][T] (int32); group: one
        id in 0..n_groups-1 per listed trial.  Returns a dict of exactly the arrays asked for; nothing else is computed or moved."""
        n, ii = self._n_idx(idx)
        _check_outputs(want, ('eta', 'var', 'ell', 'group_sum', 'group_count'), may_be_empty=True)      # (the library refuses an empty request itself)
        gg = None
        if group is not None:
            gg = np.ascontiguousarray(group, dtype=np.int32).reshape(-1)
            if gg.shape != (n,):
                raise ValueError('one group id per listed trial expected (%d), got %d' % (n, gg.size))
        shapes = {'eta': (n, self.q, self.T), 'var': (n, self.q, self.T), 'ell': (n, self.q), 'group_sum': (int(n_groups), self.q, self.T)}
        out = {k: np.empty(shapes[k]) for k in shapes if k in want}
        if 'group_count' in want:
            out['group_count'] = np.empty((int(n_groups), self.T), dtype=np.int32)
        ptr = lambda k: dptr(out[k]) if k in out else None
        check(self.lib.pgpfa_posterior_rates(self.h, n, iptr(ii), iptr(gg), int(n_groups), ptr('eta'), ptr('var'), ptr('ell'), ptr('group_sum'),
                                             iptr(out.get('group_count'))))
        return out

    def posterior_sample(self, idx=None, n_samples=1, seed=0, noise=None, want=('x',)):
        """Joint draws from the resident posterior of the listed trials (repeats allowed) and posterior-predictive counts (include/pgpfa.h:
        pgpfa_posterior_sample).  want: any of 'x' [n][S][p][T], 'y' [n][S][q][T] (uint16), 'count_sum' [n][S][q] (int32), 'noise' [n][S][nz] - the
        standard normals that were used, nz = info('sample_noise_dim').  noise: those normals given by the caller ([n][S][nz]) instead of drawn on the
        device from `seed`.  Returns a dict of exactly the arrays asked for."""
        n, ii = self._n_idx(idx)
        S = int(n_samples)
        _check_outputs(want, ('x', 'y', 'count_sum', 'noise'), may_be_empty=S < 1)
        if S < 1:
            raise ValueError('n_samples = %d: at least one draw per trial is needed' % S)
        zin = None
        nz = None
        if noise is not None or 'noise' in want:
            nz = int(self.info('sample_noise_dim'))
        if noise is not None:
            zin = as_f64(noise)
            if zin.shape != (n, S, nz):
                raise ValueError('noise must have shape (n, n_samples, nz) = %s, got %s' % ((n, S, nz), zin.shape))
        shapes = {'x': ((n, S, self.p, self.T), np.float64), 'y': ((n, S, self.q, self.T), np.uint16), 'count_sum': ((n, S, self.q), np.int32),
                  'noise': ((n, S, nz), np.float64)}
        out = {k: np.empty(shapes[k][0], dtype=shapes[k][1]) for k in shapes if k in want}
        y = out.get('y')
        check(self.lib.pgpfa_posterior_sample(self.h, n, iptr(ii), S, ct.c_ulonglong(int(seed) & 0xFFFFFFFFFFFFFFFF), None if zin is None else dptr(zin),
                                              dptr(out['noise']) if 'noise' in out else None, dptr(out['x']) if 'x' in out else None,
                                              None if y is None else y.ctypes.data_as(ct.POINTER(ct.c_uint16)), iptr(out.get('count_sum'))))
        return out

    def importance_weights(self, idx=None, n_samples=256, seed=0, want=('log_ratio', 'ess')):
        """Importance weights of the Laplace posterior's own draws for the listed trials (repeats allowed; include/pgpfa.h:
        pgpfa_importance_weights).  want: any of 'log_ratio' [n] - log of the mean weight, the correction log Z - log Z_Laplace of the trial's log
        evidence -, 'ess' [n] - the effective sample size - and 'log_w' [n][S], the log weight of draw s of posterior_sample under the same seed.
        Returns a dict of exactly the arrays asked for; the draws themselves stay on the device."""
        n, ii = self._n_idx(idx)
        S = int(n_samples)
        _check_outputs(want, ('log_ratio', 'ess', 'log_w'), may_be_empty=S < 1)
        if S < 1:
            raise ValueError('n_samples = %d: at least one draw per trial is needed' % S)
        shapes = {'log_ratio': (n,), 'ess': (n,), 'log_w': (n, S)}
        out = {k: np.empty(shapes[k]) for k in shapes if k in want}
        ptr = lambda k: dptr(out[k]) if k in out else None
        check(self.lib.pgpfa_importance_weights(self.h, n, iptr(ii), S, ct.c_ulonglong(int(seed) & 0xFFFFFFFFFFFFFFFF), ptr('log_ratio'), ptr('ess'), ptr('log_w')))
        return out

    def posterior_at(self, times, idx=None, want=('mean', 'var')):
        """Marginal posterior of every latent of the listed trials (repeats allowed) at arbitrary times in ms from the trial's first bin
        (include/pgpfa.h: pgpfa_posterior_at).  times: (S,) - one grid for all listed trials - or (n, S), one grid per list entry.  want: 'mean'
        and / or 'var', each [n][p][S].  Returns a dict of exactly the arrays asked for."""
        n, ii = self._n_idx(idx)
        _check_outputs(want, ('mean', 'var'))
        tt = as_f64(times)
        if tt.ndim == 1:
            per_trial = 0
        elif tt.ndim == 2 and tt.shape[0] == n:
            per_trial = 1
        else:
            raise ValueError('times must have shape (S,) or (n, S) = (%d, S), got %s' % (n, tt.shape))
        S = tt.shape[-1]
        out = {k: np.empty((n, self.p, S)) for k in ('mean', 'var') if k in want}
        check(self.lib.pgpfa_posterior_at(self.h, n, iptr(ii), S, dptr(tt), per_trial, dptr(out['mean']) if 'mean' in out else None,
                                          dptr(out['var']) if 'var' in out else None))
        return out

    def posterior_cov_at(self, times, idx=None, want=('mean', 'cov')):
        """Joint posterior of the latents of the listed trials (repeats allowed) at arbitrary times, and the log-rate moments there (include/pgpfa.h:
        pgpfa_posterior_cov_at).  times: as for posterior_at.  want: any of 'mean' [n][p][S], 'cov' [n][S][p][p], 'eta' [n][q][S], 'var' [n][q][S].
        Returns a dict of exactly the arrays asked for."""
        n, ii = self._n_idx(idx)
        _check_outputs(want, ('mean', 'cov', 'eta', 'var'))
        tt = as_f64(times)
        if tt.ndim == 1:
            per_trial = 0
        elif tt.ndim == 2 and tt.shape[0] == n:
            per_trial = 1
        else:
            raise ValueError('times must have shape (S,) or (n, S) = (%d, S), got %s' % (n, tt.shape))
        S = tt.shape[-1]
        shapes = {'mean': (n, self.p, S), 'cov': (n, S, self.p, self.p), 'eta': (n, self.q, S), 'var': (n, self.q, S)}
        out = {k: np.empty(shapes[k]) for k in shapes if k in want}
        ptr = lambda k: dptr(out[k]) if k in out else None
        check(self.lib.pgpfa_posterior_cov_at(self.h, n, iptr(ii), S, dptr(tt), per_trial, ptr('mean'), ptr('cov'), ptr('eta'), ptr('var')))
        return out

    def posterior_velocity_at(self, times, idx=None, want=('mean', 'vel')):
        """Value and velocity of every latent of the listed trials (repeats allowed) at arbitrary times, with their joint 2 x 2 posterior per latent
        (include/pgpfa.h: pgpfa_posterior_velocity_at).  times: as for posterior_at.  want: any of 'mean', 'var' (of the value), 'vel', 'vel_var'
        (latent units per second, and its square) and 'cross' (Cov(value, velocity)), each [n][p][S].  Returns a dict of exactly the arrays asked for."""
        n, ii = self._n_idx(idx)
        keys = ('mean', 'var', 'vel', 'vel_var', 'cross')
        _check_outputs(want, keys)
        tt = as_f64(times)
        if tt.ndim == 1:
            per_trial = 0
        elif tt.ndim == 2 and tt.shape[0] == n:
            per_trial = 1
        else:
            raise ValueError('times must have shape (S,) or (n, S) = (%d, S), got %s' % (n, tt.shape))
        S = tt.shape[-1]
        out = {k: np.empty((n, self.p, S)) for k in keys if k in want}
        check(self.lib.pgpfa_posterior_velocity_at(self.h, n, iptr(ii), S, dptr(tt), per_trial, *[dptr(out[k]) if k in out else None for k in keys]))
        return out

    def posterior_functionals(self, weights, trials=None, want=('mean', 'var')):
        """Joint posterior of linear functionals u_j . x of the latents of the listed trials (repeats allowed; include/pgpfa.h:
        pgpfa_posterior_functionals).  weights: (J, p, T) - one set for all listed trials - or (n, J, p, T), one set per list entry.  want: any of
        'mean' [n][J], 'var' [n][J] and 'cov' [n][J][J] (J <= 1024).  Returns a dict of exactly the arrays asked for."""
        n, ii = self._n_idx(trials)
        _check_outputs(want, ('mean', 'var', 'cov'))
        ww = as_f64(weights)
        if ww.ndim == 3 and ww.shape[1:] == (self.p, self.T):
            per_trial = 0
        elif ww.ndim == 4 and ww.shape[0] == n and ww.shape[2:] == (self.p, self.T):
            per_trial = 1
        else:
            raise ValueError('weights must have shape (J, p, T) = (J, %d, %d) or (n, J, p, T) = (%d, J, %d, %d), got %s'
                             % (self.p, self.T, n, self.p, self.T, ww.shape))
        J = ww.shape[-3]
        shapes = {'mean': (n, J), 'var': (n, J), 'cov': (n, J, J)}
        out = {k: np.empty(shapes[k]) for k in shapes if k in want}
        ptr = lambda k: dptr(out[k]) if k in out else None
        check(self.lib.pgpfa_posterior_functionals(self.h, n, iptr(ii), J, dptr(ww), per_trial, ptr('mean'), ptr('var'), ptr('cov')))
        return out

    def _count_outputs(self, shape, counts, K, level, k_cap, want):
        """The output arrays of the two predictive-count calls and their pointers in the order of the C prototypes (None where not asked for)."""
        _check_outputs(want, COUNT_OUTPUTS)
        cc = None
        if counts is not None:
            cc = np.ascontiguousarray(counts, dtype=np.int32)
            if cc.shape != shape:
                raise ValueError('counts must have shape %s, got %s' % (shape, cc.shape))
        kinds = {'logp': (shape, np.float64), 'pmf': (shape + (int(K),), np.float64), 'lower': (shape, np.int32), 'upper': (shape, np.int32),
                 'pmean': (shape, np.float64), 'pvar': (shape, np.float64)}
        out = {k: np.empty(kinds[k][0], dtype=kinds[k][1]) for k in COUNT_OUTPUTS if k in want}
        ptrs = [None if k not in out else (iptr(out[k]) if k in ('lower', 'upper') else dptr(out[k])) for k in COUNT_OUTPUTS]
        return cc, out, (iptr(cc), int(K), float(level), int(k_cap)) + tuple(ptrs)

    def count_probabilities(self, m, v, counts=None, K=1, level=0.95, k_cap=65535, want=('logp',)):
        """Posterior-predictive count probabilities of entries with log-rate moments m, v (any shape, the same for both; include/pgpfa.h:
        pgpfa_count_probabilities).  want: any of 'logp' (needs counts, int32 of m's shape), 'pmf' (m's shape + (K,)), 'lower' / 'upper' (int32, the
        central `level` interval, walked up to k_cap; info('counts_saturated') counts the entries it cut), 'pmean', 'pvar'.  Returns a dict of exactly
        the arrays asked for."""
        mm, vv = as_f64(m), as_f64(v)
        if mm.shape != vv.shape:
            raise ValueError('m and v must have the same shape, got %s and %s' % (mm.shape, vv.shape))
        cc, out, args = self._count_outputs(mm.shape, counts, K, level, k_cap, want)
        check(self.lib.pgpfa_count_probabilities(self.h, mm.size, dptr(mm), dptr(vv), *args))
        return out

    def posterior_counts(self, idx=None, counts=None, K=1, level=0.95, k_cap=65535, want=('logp',)):
        """The same per (trial, neuron, bin) of the listed trials (repeats allowed) under their resident posterior (include/pgpfa.h:
        pgpfa_posterior_counts): every output [n][q][T], 'pmf' [n][q][T][K].  counts: int32 [n][q][T], or None for the resident counts.  Bins behind
        a trial's own length come back as NaN (lower, upper: -1)."""
        n, ii = self._n_idx(idx)
        cc, out, args = self._count_outputs((n, self.q, self.T), counts, K, level, k_cap, want)
        check(self.lib.pgpfa_posterior_counts(self.h, n, iptr(ii), *args))
        return out

    # -- dual variational ---------------------------------------------------------------------
    def dual_costgrad(self, trial, lam, want_grad=True):
        lam = as_f64(lam).reshape(-1)
        cost = ct.c_double(0.0)
        grad = np.empty(self.q * self.T) if want_grad else None
        check(self.lib.pgpfa_dual_costgrad(self.h, int(trial), dptr(lam), ct.byref(cost), dptr(grad) if want_grad else None))
        return cost.value, grad

    def dual_post_mean(self, trial, lam):
        lam = as_f64(lam).reshape(-1)
        out = np.empty(self.n)
        check(self.lib.pgpfa_dual_post_mean(self.h, int(trial), dptr(lam), dptr(out)))
        return out

    def dual_post_cov(self, trial, lam, want_prec=True):
        lam = as_f64(lam).reshape(-1)
        cov = np.empty((self.n, self.n))
        prec = np.empty((self.n, self.n)) if want_prec else None
        check(self.lib.pgpfa_dual_post_cov(self.h, int(trial), dptr(lam), dptr(cov), dptr(prec) if want_prec else None))
        return cov, prec

    def dual_costgrad_batch(self, idx, lam, want_grad=True):
        """Dual cost (and gradient) of the listed distinct trials, each at its own lambda: lam[n][q*T] -> cost[n], grad[n][q*T]."""
        n, ii = self._n_idx(idx)
        lam = as_f64(lam).reshape(n, self.q * self.T)
        cost = np.empty(n)
        grad = np.empty((n, self.q * self.T)) if want_grad else None
        check(self.lib.pgpfa_dual_costgrad_batch(self.h, n, iptr(ii), dptr(lam), dptr(cost), dptr(grad) if want_grad else None))
        return cost, grad

    def dual_lbfgs(self, idx, rho0, max_iter=15000, factr=1e7, pgtol=1e-5):
        """Device L-BFGS on the dual in rho = log(lambda) for the listed trials -> (rho_opt[n][q*T], dual optimum[n], iterations[n])."""
        n, ii = self._n_idx(idx)
        rho = np.array(as_f64(rho0).reshape(n, self.q * self.T), copy=True)
        fopt = np.empty(n)
        iters = np.zeros(n, dtype=np.int32)
        check(self.lib.pgpfa_dual_lbfgs(self.h, n, iptr(ii), dptr(rho), int(max_iter), float(factr), float(pgtol), dptr(fopt), iptr(iters)))
        return rho, fopt, iters

    def dual_fixed_point(self, idx, rho0=None, max_outer=40, tol=1e-8, warm=False, want_lam=False, want_rho=True, resident=False):
        """Optimum of the dual by the variance fixed point (pgpfa_dual_fixed_point) -> (rho_opt[n][q*T] or None, dual optimum[n], passes[n],
        status[n]: 0 converged, 1 pass cap, 2 not contracting[, lambda_opt[n][q*T] with want_lam]).  rho0 = None: the reference's cold start
        lambda = 0.5; warm: rho0 is a previous optimum; resident: the start is the optimum resident on the device (nothing uploaded).  The
        optimum stays on the device: dual_finalize(idx, None) takes it from there, dual_lambda(idx) reads it."""
        n, ii = self._n_idx(idx)
        m = self.q * self.T
        if resident:
            rho, start = (np.empty((n, m)) if want_rho else None), 3
        elif rho0 is None:
            rho, start = (np.empty((n, m)) if want_rho else None), 0
        else:
            rho, start = np.array(as_f64(rho0).reshape(n, m), copy=True), (2 if warm else 1)
        fopt = np.empty(n)
        outer = np.zeros(n, dtype=np.int32)
        status = np.zeros(n, dtype=np.int32)
        lam = np.empty((n, m)) if want_lam else None
        check(self.lib.pgpfa_dual_fixed_point(self.h, n, iptr(ii), dptr(rho) if rho is not None else None, start, int(max_outer), float(tol), dptr(fopt),
                                              iptr(outer), iptr(status), dptr(lam) if want_lam else None))
        return (rho, fopt, outer, status, lam) if want_lam else (rho, fopt, outer, status)

    def dual_lambda(self, idx=None):
        """The dual variables resident for the listed trials: [n][q*T]."""
        n, ii = self._n_idx(idx)
        out = np.empty((n, self.q * self.T))
        check(self.lib.pgpfa_get_dual_lambda(self.h, n, iptr(ii), dptr(out)))
        return out

    def dual_finalize(self, idx, lam):
        """lam = None: the optimum the last dual_fixed_point left on the device for these trials."""
        n, ii = self._n_idx(idx)
        tot = ct.c_double(0.0)
        if lam is None:
            check(self.lib.pgpfa_dual_finalize(self.h, n, iptr(ii), None, ct.byref(tot)))
            return tot.value
        lam = as_f64(lam).reshape(n, self.q * self.T)
        check(self.lib.pgpfa_dual_finalize(self.h, n, iptr(ii), dptr(lam), ct.byref(tot)))
        return tot.value

    # -- M-step --------------------------------------------------------------------------------
    def mstep_cd_costgrad(self, vec, prior_center=None, inv_s2=0.0):
        vec = as_f64(vec).reshape(-1)
        cost = ct.c_double(0.0)
        grad = np.empty(self.q * (self.p + 1))
        pc = None if prior_center is None else as_f64(prior_center).reshape(-1)
        check(self.lib.pgpfa_mstep_cd_costgrad(self.h, dptr(vec), None if pc is None else dptr(pc), float(inv_s2),
                                               ct.byref(cost), dptr(grad)))
        return cost.value, grad

    def mstep_cd_newton_pass(self, vec, prior_center=None, inv_s2=0.0):
        vec = as_f64(vec).reshape(-1)
        pc = None if prior_center is None else as_f64(prior_center).reshape(-1)
        cost_n, dec = np.empty(self.q), np.empty(self.q)
        delta = np.empty(self.q * (self.p + 1))
        check(self.lib.pgpfa_mstep_cd_newton_pass(self.h, dptr(vec), None if pc is None else dptr(pc), float(inv_s2),
                                                  dptr(cost_n), dptr(delta), dptr(dec)))
        return cost_n, delta, dec

    def mstep_cd_chord_pass(self, vec, prior_center=None, inv_s2=0.0):
        """cost_n, Newton-like step and decrement at vec with the Hessians of the last mstep_cd_newton_pass."""
        vec = as_f64(vec).reshape(-1)
        pc = None if prior_center is None else as_f64(prior_center).reshape(-1)
        cost_n, dec = np.empty(self.q), np.empty(self.q)
        delta = np.empty(self.q * (self.p + 1))
        check(self.lib.pgpfa_mstep_cd_chord_pass(self.h, dptr(vec), None if pc is None else dptr(pc), float(inv_s2),
                                                 dptr(cost_n), dptr(delta), dptr(dec)))
        return cost_n, delta, dec

    def mstep_cd_cost_per_neuron(self, vec, prior_center=None, inv_s2=0.0):
        vec = as_f64(vec).reshape(-1)
        pc = None if prior_center is None else as_f64(prior_center).reshape(-1)
        cost_n = np.empty(self.q)
        check(self.lib.pgpfa_mstep_cd_cost_per_neuron(self.h, dptr(vec), None if pc is None else dptr(pc), float(inv_s2), dptr(cost_n)))
        return cost_n

    def mstep_precomp(self):
        n = ct.c_double(0.0)
        check(self.lib.pgpfa_mstep_precomp(self.h, ct.byref(n)))
        return n.value

    def pautosum(self):
        out = np.empty((self.p, self.T, self.T))
        check(self.lib.pgpfa_get_pautosum(self.h, dptr(out)))
        return out

    def mstep_tau_costgrad(self, k, logp):
        cost, grad = ct.c_double(0.0), ct.c_double(0.0)
        check(self.lib.pgpfa_mstep_tau_costgrad(self.h, int(k), float(logp), ct.byref(cost), ct.byref(grad)))
        return cost.value, grad.value

    def mstep_tau_costgrad_batch(self, logp):
        logp = as_f64(logp).reshape(-1)
        cost, grad = np.empty(self.p), np.empty(self.p)
        check(self.lib.pgpfa_mstep_tau_costgrad_batch(self.h, dptr(logp), dptr(cost), dptr(grad)))
        return cost, grad

    def mstep_tau_costgrad_multi(self, logp):
        """logp[m][p] (m <= 4 candidate points per latent) -> cost[m][p], grad[m][p] in one batched pass."""
        logp = as_f64(logp).reshape(-1, self.p)
        m = logp.shape[0]
        cost, grad = np.empty((m, self.p)), np.empty((m, self.p))
        check(self.lib.pgpfa_mstep_tau_costgrad_multi(self.h, int(m), dptr(logp), dptr(cost), dptr(grad)))
        return cost, grad

    def mstep_tau_costgrad_multi_begin(self, logp):
        """Enqueue the batched pass on the side stream and return; collect with mstep_tau_costgrad_multi_end()."""
        logp = as_f64(logp).reshape(-1, self.p)
        check(self.lib.pgpfa_mstep_tau_costgrad_multi_begin(self.h, int(logp.shape[0]), dptr(logp)))
        self._tau_m = logp.shape[0]

    def mstep_tau_costgrad_multi_end(self):
        m = self._tau_m
        cost, grad = np.empty((m, self.p)), np.empty((m, self.p))
        check(self.lib.pgpfa_mstep_tau_costgrad_multi_end(self.h, dptr(cost), dptr(grad)))
        return cost, grad

    # -- comm --------------------------------------------------------------------------------------
    def comm_init(self, uid, rank, nranks):
        warm_rccl_image()
        check(self.lib.pgpfa_comm_init(self.h, uid, int(rank), int(nranks)))

    def comm_describe(self):
        """One line about this rank's communicator (device, PCI bus id, the rank count RCCL itself reports)."""
        buf = ct.create_string_buffer(256)
        check(self.lib.pgpfa_comm_describe(self.h, buf, 256))
        return buf.value.decode('utf-8', 'replace')

    def allreduce_host(self, arr):
        a = as_f64(arr).reshape(-1).copy()
        check(self.lib.pgpfa_comm_allreduce_host(self.h, dptr(a), a.size))
        return a.reshape(np.shape(arr))

    # -- test hooks ----------------------------------------------------------------------------------
    def test_potrf(self, A, want_inverse=True):
        A = as_f64(A)
        if A.ndim == 2:
            A = A[None]
        b, n, _ = A.shape
        L = np.empty_like(A)
        inv = np.empty_like(A) if want_inverse else None
        check(self.lib.pgpfa_test_potrf(self.h, b, n, dptr(A), dptr(L), dptr(inv) if want_inverse else None))
        return L, inv

    def test_gemm_nt(self, A, B, C=None, alpha=1.0, beta=0.0, f32=False):
        """C = alpha*A@B.T + beta*C with A (M,K), B (N,K) given row-major; passed column-major.  f32: single-precision MFMA kernel."""
        A, B = as_f64(A), as_f64(B)
        M, K = A.shape
        N = B.shape[0]
        Ccm = np.zeros((N, M)) if C is None else as_f64(np.asarray(C).T)     # column-major (M,N) == row-major (N,M)
        Acm, Bcm = as_f64(A.T), as_f64(B.T)                                   # column-major (M,K) == row-major (K,M)
        fn = self.lib.pgpfa_test_gemm_nt_f32 if f32 else self.lib.pgpfa_test_gemm_nt
        check(fn(self.h, M, N, K, float(alpha), dptr(Acm), dptr(Bcm), float(beta), dptr(Ccm)))
        return Ccm.T.copy()

    def test_gemm_nn(self, A, B, C=None, alpha=1.0, beta=0.0, f32=False):
        """C = alpha*A@B + beta*C with A (M,K), B (K,N) row-major in; B is passed K x N column-major."""
        A, B = as_f64(A), as_f64(B)
        M, K = A.shape
        N = B.shape[1]
        Ccm = np.zeros((N, M)) if C is None else as_f64(np.asarray(C).T)
        Acm, Bcm = as_f64(A.T), as_f64(B.T)                # (K,N) column-major == (N,K) row-major buffer
        fn = self.lib.pgpfa_test_gemm_nn_f32 if f32 else self.lib.pgpfa_test_gemm_nn
        check(fn(self.h, M, N, K, float(alpha), dptr(Acm), dptr(Bcm), float(beta), dptr(Ccm)))
        return Ccm.T.copy()

    def test_split_syrk(self, D, T, p, ract, ldd, ts, sps=0, tile=256, fill=0.0, band=0):
        """The FP16 term of the split covariance sum (pgpfa_test_split_syrk) on D, float32 (nslots, round_up(ract, 32) * ldd).  Returns (part, tile_used,
        ngroups, tail): part (p, ngroups, T, T) indexed [k, g, j, i] - column-major (i, j) blocks - prefilled with `fill`, so entries no kernel stored
        keep it; tail: `band` doubles behind the output buffer, prefilled alike."""
        D = np.ascontiguousarray(D, dtype=np.float32)
        nslots = D.shape[0]
        assert D.ndim == 2 and D.shape[1] == (int(ract) + 31) // 32 * 32 * int(ldd)
        spe = int(sps) if sps > 0 else max(1, (nslots + 63) // 64)
        ng = (nslots + spe - 1) // spe
        n = p * ng * T * T
        buf = np.full(n + int(band), float(fill))
        tile_used, ngroups = ct.c_int(0), ct.c_int(0)
        check(self.lib.pgpfa_test_split_syrk(self.h, nslots, int(T), int(p), int(ract), int(ldd), int(ts), int(sps), int(tile),
                                             D.ctypes.data_as(ct.POINTER(ct.c_float)), dptr(buf), ct.byref(tile_used), ct.byref(ngroups)))
        assert ngroups.value == ng
        return buf[:n].reshape(p, ng, T, T), tile_used.value, ngroups.value, buf[n:]

    def test_split_latent_sums(self, A, D, rk, kw, T, lda, row_off, ldd, sps=0, cross_kernel=1, fill=0.0, band=0):
        """One latent's sums of the split form (pgpfa_test_split_latent_sums): A float64 (nslots, sM), D float32 (nslots, sD).  Returns (S, X, tails):
        S[j, i] = sum_s (A_s A_s^T)[i, j] (rk, rk), X[t, i] = sum_s (A_s D_s^T)[i, t] (T, rk) - the column-major results - and the `band` doubles behind each."""
        A = as_f64(A)
        D = np.ascontiguousarray(D, dtype=np.float32)
        nslots = A.shape[0]
        assert A.ndim == 2 and D.ndim == 2 and D.shape[0] == nslots
        S = np.full(rk * rk + int(band), float(fill))
        X = np.full(rk * T + int(band), float(fill))
        check(self.lib.pgpfa_test_split_latent_sums(self.h, nslots, int(rk), int(kw), int(T), int(lda), A.shape[1], int(row_off), int(ldd), D.shape[1], int(sps),
                                                    int(cross_kernel), dptr(A), D.ctypes.data_as(ct.POINTER(ct.c_float)), dptr(S), dptr(X)))
        return S[:rk * rk].reshape(rk, rk), X[:rk * T].reshape(T, rk), (S[rk * rk:], X[rk * T:])

    THIN_KINDS = {'ft': 0, 's': 1, 'f': 2, 'apply': 3}
    THIN_REFUSALS = {100: 'bad_arg', 101: 'T', 102: 'rank', 103: 'Tx', 104: 'ld', 105: 'rpad', 106: 'cols', 107: 'live'}      # PGPFA_THIN_* of pgpfa.h

    def test_thin(self, kind, T, Tf, ranks, gran, X, Y, Tx=None, F=None, Sb=None, f32=False, cols=None, ncols=None, live=None, stop=None, fill=0.0):
        """The thin products of the low-rank preconditioner (pgpfa_test_thin) on caller data: kind 'ft' (u = F^T t), 's' (v = Sb u), 'f' (y = F v) or
        'apply' (the three in a row).  X (nslots, ldx) input and Y (nslots, ldy) output buffer with the caller's prefill, one row per slot; n-vectors
        (input of 'ft' / 'apply', output of 'f' / 'apply') are float32 with f32, everything else float64.  F (p, Tf, Tf) indexed [latent, column, bin],
        Sb (rpad, rpad) indexed [k, m].  cols: slot list (None: identity over ncols slots), live: device-side live count, stop: stop flag value.
        Returns (Y as the device left it, info): info holds rr, rk, roff, rtot, rpad and the tables ft, f, s as (entries, 4) arrays.
        A refused geometry raises HipBackendError with .rc (the return code) and .refusal (its name in THIN_REFUSALS)."""
        ranks = np.ascontiguousarray(ranks, dtype=np.int32)
        p = len(ranks)
        k = self.THIN_KINDS[kind]
        xt = np.float32 if f32 and kind in ('ft', 'apply') else np.float64
        yt = np.float32 if f32 and kind in ('f', 'apply') else np.float64
        X = np.ascontiguousarray(X, dtype=xt)
        out = np.array(Y, dtype=yt, order='C', copy=True)
        assert X.ndim == 2 and out.ndim == 2 and X.shape[0] == out.shape[0]
        nslots = X.shape[0]
        cl = None if cols is None else np.ascontiguousarray(cols, dtype=np.int32)
        nc = int(ncols) if ncols is not None else (nslots if cl is None else len(cl))
        assert cl is None or len(cl) == nc
        Fp = None
        if F is not None:
            F = as_f64(F)
            assert F.shape == (p, int(Tf), int(Tf))
            Fp = dptr(F)
        geom = np.zeros(3 * p + 3, dtype=np.int32)
        cap = 4 * (p * (16 + (max(int(T), 1) + 255) // 256) + 1024)
        tabs = [np.zeros(cap, dtype=np.int32) for _ in range(3)]
        ntab = np.zeros(3, dtype=np.int32)
        Sp = None
        if Sb is not None:
            Sb = as_f64(Sb)
            if int(gran) in (4, 8, 16) and np.all(ranks >= 1):                 # (else the hook refuses before it reads anything)
                rr = (ranks + int(gran) - 1) // int(gran) * int(gran)
                roff = np.concatenate([[0], np.cumsum(rr)])
                rpad = (max(int(roff[-1]), int(np.max(roff[:-1] + (rr + 15) // 16 * 16))) + 127) // 128 * 128
                assert Sb.shape == (rpad, rpad), (Sb.shape, rpad)
            Sp = dptr(Sb)
        rc = self.lib.pgpfa_test_thin(self.h, k, p, int(T), int(Tf), iptr(ranks), int(gran), X.shape[1], out.shape[1], int(T if Tx is None else Tx), int(bool(f32)),
                                      nslots, nc, iptr(cl), -1 if live is None else int(live), -1 if stop is None else int(stop), float(fill), Fp, Sp,
                                      X.ctypes.data_as(ct.c_void_p), out.ctypes.data_as(ct.c_void_p), iptr(geom), cap, iptr(tabs[0]), iptr(tabs[1]), iptr(tabs[2]),
                                      iptr(ntab))
        if rc != 0:
            err = HipBackendError(self.lib.pgpfa_last_error().decode('utf-8', 'replace'))
            err.rc = rc
            err.refusal = self.THIN_REFUSALS.get(rc)
            raise err
        info = dict(rr=geom[:p].copy(), rk=geom[p:2 * p].copy(), roff=geom[2 * p:3 * p + 1].copy(), rtot=int(geom[3 * p + 1]), rpad=int(geom[3 * p + 2]),
                    ft=tabs[0][:4 * ntab[0]].reshape(-1, 4).copy(), f=tabs[1][:4 * ntab[1]].reshape(-1, 4).copy(), s=tabs[2][:4 * ntab[2]].reshape(-1, 4).copy())
        return out, info

    PIVCHOL_REFUSALS = {120: 'bad_arg', 121: 'T', 122: 'Tf', 123: 'odd', 124: 'lds'}      # PGPFA_PIVCHOL_* of pgpfa.h
    PIVCHOL_FORMS = ('256_1', '512_2', 'pairs')

    def test_pivchol(self, T, Tf, tau, bin_ms, eps, tol, pairs=True, fill=0.0):
        """The pivoted Cholesky of (1 - eps) RBF for the timescales tau (seconds) on slabs prefilled with `fill` (pgpfa_test_pivchol).
        Returns (F (p, Tf, Tf) indexed [latent, column, bin], ranks (p,), form - one of PIVCHOL_FORMS).
        A refused geometry raises HipBackendError with .rc and .refusal (its name in PIVCHOL_REFUSALS)."""
        tau = as_f64(np.atleast_1d(tau))
        p = len(tau)
        ok = 0 < int(Tf) <= 4096
        F = np.empty((p, int(Tf), int(Tf)) if ok else (1,))
        rank = np.zeros(p, dtype=np.int32)
        form = np.zeros(1, dtype=np.int32)
        rc = self.lib.pgpfa_test_pivchol(self.h, p, int(T), int(Tf), dptr(tau), float(bin_ms), float(eps), float(tol), int(bool(pairs)), float(fill), dptr(F),
                                         iptr(rank), iptr(form))
        if rc != 0:
            err = HipBackendError(self.lib.pgpfa_last_error().decode('utf-8', 'replace'))
            err.rc = rc
            err.refusal = self.PIVCHOL_REFUSALS.get(rc)
            raise err
        return F, rank, self.PIVCHOL_FORMS[int(form[0])]

    BINB_REFUSALS = {130: 'bad_arg', 131: 'p', 132: 'list', 133: 'stride'}      # PGPFA_BINB_* of pgpfa.h

    def test_bin_blocks(self, p, T, eps, W, G, Wt, slots=None, sW=None, sO=None, want_ldet=True, ldet_fill=0.0, fill=0.0):
        """The per-bin blocks G = (I + eps W)^-1, Wt = W G, log det(I + eps W) (pgpfa_test_bin_blocks) on caller data.  W (nslots, sW) float64, bin t of a
        slot at t p p (row-major p x p); G, Wt (nslots, sO): the output buffers with the caller's prefill; slots: the slot list (None: all, in order).
        sW / sO default to the row lengths; 0: one shared slot.  Returns (G, Wt, ldet (len(slots), T) or None - prefilled with ldet_fill -, per_block).
        A refused geometry raises HipBackendError with .rc and .refusal (its name in BINB_REFUSALS)."""
        W = as_f64(np.atleast_2d(W))
        Go = np.array(np.atleast_2d(G), dtype=np.float64, order='C', copy=True)
        Wo = np.array(np.atleast_2d(Wt), dtype=np.float64, order='C', copy=True)
        nslots = Go.shape[0]
        assert W.shape[0] == nslots and Wo.shape == Go.shape
        sl = np.ascontiguousarray(np.arange(nslots) if slots is None else slots, dtype=np.int32)
        ld = np.full((len(sl), max(int(T), 1)), float(ldet_fill)) if want_ldet else None
        per_block = np.zeros(1, dtype=np.int32)
        rc = self.lib.pgpfa_test_bin_blocks(self.h, int(p), int(T), float(eps), nslots, len(sl), iptr(sl), int(W.shape[1] if sW is None else sW),
                                            int(Go.shape[1] if sO is None else sO), float(fill), dptr(W), dptr(Go), dptr(Wo), dptr(ld) if want_ldet else None,
                                            iptr(per_block))
        if rc != 0:
            err = HipBackendError(self.lib.pgpfa_last_error().decode('utf-8', 'replace'))
            err.rc = rc
            err.refusal = self.BINB_REFUSALS.get(rc)
            raise err
        return Go, Wo, ld, int(per_block[0])

    ASMB_REFUSALS = {110: 'bad_arg', 111: 'Tf', 112: 'rank', 113: 'list', 114: 'stride'}      # PGPFA_ASMB_* of pgpfa.h

    def test_assemble_b(self, T, Tf, ranks, gran, F, Wt, B, slots=None, sW=None, f32=False, fill=0.0):
        """B = I + F^T Wt F of the low-rank engine (pgpfa_test_assemble_b) on caller data.  F (p, Tf, Tf) indexed [latent, column, bin]; Wt (nslots, sW)
        float64, bin t of a slot at t p p, or (T p p,) / (1, T p p) with sW = 0 (one shared slot); B (nslots, rpad, rpad) indexed [slot, column, row], the
        output buffer with the caller's prefill, float32 with f32.  slots: the slot list (None: all, in order).
        Returns (B as the device left it, info): info holds rr, rk, roff, roff16, rtot, rtot16, rpad, compact, nblk64, npairs, nact, blk_lat, blk_col, cmap.
        A refused geometry raises HipBackendError with .rc and .refusal (its name in ASMB_REFUSALS)."""
        ranks = np.ascontiguousarray(ranks, dtype=np.int32)
        p = len(ranks)
        F = as_f64(F)
        assert F.shape == (p, int(Tf), int(Tf))
        out = np.array(B, dtype=np.float32 if f32 else np.float64, order='C', copy=True)
        assert out.ndim == 3 and out.shape[1] == out.shape[2]
        nslots = out.shape[0]
        Wt = as_f64(Wt)
        if sW is None:
            sW = Wt.shape[1] if Wt.ndim == 2 else 0
        assert Wt.size >= (int(sW) * nslots if sW else 1)
        sl = np.ascontiguousarray(np.arange(nslots) if slots is None else slots, dtype=np.int32)
        geom = np.zeros(4 * p + 9, dtype=np.int32)
        cap = 16 * (16 * p + 256) + 1024
        tabs = [np.zeros(cap, dtype=np.int32) for _ in range(3)]
        ntab = np.zeros(2, dtype=np.int32)
        rc = self.lib.pgpfa_test_assemble_b(self.h, p, int(T), int(Tf), iptr(ranks), int(gran), int(bool(f32)), nslots, len(sl), iptr(sl), int(sW), float(fill),
                                            dptr(F), dptr(Wt), out.ctypes.data_as(ct.c_void_p), out.shape[1], iptr(geom), cap, iptr(tabs[0]), iptr(tabs[1]),
                                            iptr(tabs[2]), iptr(ntab))
        if rc != 0:
            err = HipBackendError(self.lib.pgpfa_last_error().decode('utf-8', 'replace'))
            err.rc = rc
            err.refusal = self.ASMB_REFUSALS.get(rc)
            raise err
        g = geom[4 * p + 2:]
        info = dict(rr=geom[:p].copy(), rk=geom[p:2 * p].copy(), roff=geom[2 * p:3 * p + 1].copy(), roff16=geom[3 * p + 1:4 * p + 2].copy(), rtot=int(g[0]),
                    rtot16=int(g[1]), rpad=int(g[2]), compact=bool(g[3]), nblk64=int(g[4]), npairs=int(g[5]), nact=int(g[6]),
                    blk_lat=tabs[0][:ntab[0]].copy(), blk_col=tabs[1][:ntab[0]].copy(), cmap=tabs[2][:ntab[1]].copy())
        return out, info

    def bench_mfma_peak(self, iters=20000):
        tf = ct.c_double(0.0)
        check(self.lib.pgpfa_bench_mfma_peak(self.h, int(iters), ct.byref(tf)))
        return tf.value

    def gemm_shape_report(self):
        """Text table of the GEMM launches timed since set_option('profile', 1 | 2), grouped by operand shape."""
        need = self.lib.pgpfa_gemm_shape_report(self.h, None, 0)
        if need < 0:
            check(1)
        buf = ct.create_string_buffer(max(need, 1))
        self.lib.pgpfa_gemm_shape_report(self.h, buf, need)
        return buf.value.decode()

    def bench_potrf_diag(self, batch, reps=50, phases=3):
        us = ct.c_double()
        check(self.lib.pgpfa_bench_potrf_diag(self.h, int(batch), int(reps), int(phases), ct.byref(us)))
        return us.value

    def bench_syrk(self, batch, n, k, reps):
        ms, fl = ct.c_double(0.0), ct.c_double(0.0)
        check(self.lib.pgpfa_bench_syrk(self.h, int(batch), int(n), int(k), int(reps), ct.byref(ms), ct.byref(fl)))
        return ms.value, fl.value


_rccl_warmed = False


def warm_rccl_image():
    """RCCL's shared object carries ~0.5 GB of device code that ncclCommInitRank loads through page faults; on a
    machine whose image has not been read yet that takes minutes.  One sequential read beforehand makes the first
    communicator come up in seconds (no-op cost when the file is already cached)."""
    global _rccl_warmed
    if _rccl_warmed:
        return
    _rccl_warmed = True
    try:
        path = None
        with open('/proc/self/maps') as fh:
            for line in fh:
                if 'librccl.so' in line:
                    path = line.split()[-1]
                    break
        if path is None:
            return
        with open(path, 'rb', buffering=0) as fh:
            while fh.read(16 << 20):
                pass
    except OSError:
        pass


def comm_unique_id():
    load_library()
    warm_rccl_image()
    buf = ct.create_string_buffer(128)
    check(load_library().pgpfa_comm_unique_id(buf))
    return buf.raw
