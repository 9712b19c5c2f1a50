"""ctypes binding of libnmgp_hip.so (the C ABI declared in include/nmgp.h).

The product path has NO CPU fallback: if the shared object is missing, cannot be loaded, or no MI355X is
visible, every compute entry raises.  Only ``load(require_gpu=False)`` is allowed without a GPU and only
resolves symbols (used by the CPU test-suite to check the ABI surface).
"""
from __future__ import annotations

import ctypes
import os
import threading

import numpy as np

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG, "libnmgp_hip.so")

c_double_p = ctypes.POINTER(ctypes.c_double)
c_ll_p = ctypes.POINTER(ctypes.c_longlong)
c_void_pp = ctypes.POINTER(ctypes.c_void_p)
I, D, P, V = ctypes.c_int, ctypes.c_double, c_double_p, ctypes.c_void_p

NUM_NAN = 1 << 20
NUM_EIG = (1 << 20) + 1
HAD_ADAM_HIST_MAX = 1 << 24          # NMGP_HAD_ADAM_HIST_MAX: values of one nmgp_had_subjects_adam call's history (tests compare the two)
STAGES = ["cov", "chol", "solve", "reduce", "prior", "inverse", "adjoint", "eig", "kronmv", "syrk"]

# name -> (restype, argtypes); must list every function declared in include/nmgp.h
SIGNATURES = {
    "nmgp_ctx_create": (I, [I, c_void_pp]),
    "nmgp_ctx_destroy": (I, [V]),
    "nmgp_last_error": (ctypes.c_char_p, [V]),
    "nmgp_version": (I, []),
    "nmgp_build_id": (ctypes.c_char_p, []),
    "nmgp_sync": (I, [V]),
    "nmgp_device_count": (I, []),
    "nmgp_set_data": (I, [V, P, P, I, I]),
    "nmgp_logpos_svc": (I, [V, P, P, I, P, P]),
    "nmgp_svc_set_pars": (I, [V, P]),
    "nmgp_svc_pars_dev": (V, [V]),
    "nmgp_svc_grad_dev": (V, [V]),
    "nmgp_svc_eval_resident": (I, [V, P, I, I]),
    "nmgp_svc_fetch": (I, [V, P, P]),
    "nmgp_svc_batch_alloc": (I, [V, I]),
    "nmgp_svc_batch_set_pars": (I, [V, P]),
    "nmgp_svc_batch_set_subjects": (I, [V, P, P]),
    "nmgp_svc_batch_pars_dev": (V, [V]),
    "nmgp_svc_batch_eval": (I, [V, P, I, I]),
    "nmgp_svc_batch_fetch_grad": (I, [V, P]),
    "nmgp_svc_batch_grad_dev": (V, [V]),
    "nmgp_svc_batch_fetch": (I, [V, P, ctypes.POINTER(ctypes.c_int)]),
    "nmgp_svc_batch_set_subjects_chains": (I, [V, P, P, I]),
    "nmgp_svc_batch_traj_begin": (I, [V]),
    "nmgp_svc_batch_traj_set_mass": (I, [V, I, P]),
    "nmgp_svc_batch_traj": (I, [V, P, I, D, I, P, P, P, P, ctypes.POINTER(ctypes.c_int)]),
    "nmgp_svc_batch_traj_set_mass_chol": (I, [V, I, P]),
    "nmgp_svc_batch_traj_z": (I, [V, P, I, D, I, P, P, P, P, ctypes.POINTER(ctypes.c_int)]),
    "nmgp_svc_batch_traj_commit": (I, [V, ctypes.POINTER(ctypes.c_int)]),
    "nmgp_svc_batch_traj_set_mass_prior": (I, [V, P, I, P, P]),
    "nmgp_svc_batch_prior_apply": (I, [V, P, I, P, P]),
    "nmgp_sep_prior_apply": (I, [V, P, I, I, P, P]),
    "nmgp_svc_batch_adam_begin": (I, [V]),
    "nmgp_svc_batch_adam_step": (I, [V, P, I, D, D, D, D, P, ctypes.POINTER(ctypes.c_int)]),
    "nmgp_svc_batch_get_pars": (I, [V, P]),
    "nmgp_svc_covariance": (I, [V, P, P]),
    "nmgp_logpos_sep": (I, [V, P, P, I, P, P]),
    "nmgp_logpos_sta": (I, [V, P, P, I, P, P]),
    "nmgp_sep_batch_eval": (I, [V, P, I, P, I, P, P, ctypes.POINTER(ctypes.c_int)]),
    "nmgp_sep_batch_set_subjects_chains": (I, [V, P, P, I, I]),
    "nmgp_sep_batch_clear_subjects": (I, [V]),
    "nmgp_sta_batch_eval": (I, [V, P, I, P, I, P, P, ctypes.POINTER(ctypes.c_int)]),
    "nmgp_pairwise_distances": (I, [V, P, I, P, I, I, P]),
    "nmgp_rbf_cov": (I, [V, P, I, P, I, I, D, D, P]),
    "nmgp_nonstat_rbf_cov": (I, [V, P, P, P, I, P, P, P, I, I, P]),
    "nmgp_kron_product": (I, [V, P, I, I, P, I, I, P]),
    "nmgp_kron_mv": (I, [V, P, I, I, P, I, I, P, P]),
    "nmgp_mvn_logpdf": (I, [V, P, P, D, P, I, P]),
    "nmgp_mvn_logpdf_kron": (I, [V, P, P, P, I, P, I, D, P]),
    "nmgp_mvn_logpdf_dense": (I, [V, P, P, P, I, P, I, D, P]),
    "nmgp_kron_inv_logdet": (I, [V, D, P, I, P, I, P, P]),
    "nmgp_cholesky": (I, [V, P, I, P, P, P, I]),
    "nmgp_cholesky_batch": (I, [V, P, I, I, P, I, I, I, I, P, P, P, P, ctypes.POINTER(ctypes.c_int)]),
    "nmgp_predict_svc": (I, [V, P, P, P, I, P, P, P]),
    "nmgp_predict_sep": (I, [V, P, P, P, I, P, P]),
    "nmgp_predict_sta": (I, [V, P, P, I, P, P]),
    "nmgp_had_set_data": (I, [V, P, ctypes.POINTER(ctypes.c_int), P, I, I]),
    "nmgp_had_batch_eval": (I, [V, P, I, P, I, P, P, ctypes.POINTER(ctypes.c_int)]),
    "nmgp_had_covariance": (I, [V, P, P]),
    "nmgp_predict_had": (I, [V, P, P, P, I, P, P, P]),
    "nmgp_had_set_subjects": (I, [V, P, ctypes.POINTER(ctypes.c_int), P, ctypes.POINTER(ctypes.c_int), I, I, I]),
    "nmgp_had_clear_subjects": (I, [V]),
    "nmgp_had_subjects_eval": (I, [V, P, I, I, P, I, P, P, ctypes.POINTER(ctypes.c_int)]),
    "nmgp_hads_subjects_eval": (I, [V, P, I, I, P, I, P, P, ctypes.POINTER(ctypes.c_int)]),
    "nmgp_hadst_subjects_eval": (I, [V, P, I, I, P, I, P, P, ctypes.POINTER(ctypes.c_int)]),
    "nmgp_had_subjects_traj_begin": (I, [V, I, P, I, I, P, I, P, ctypes.POINTER(ctypes.c_int)]),
    "nmgp_had_subjects_traj_set_mass": (I, [V, I, P]),
    "nmgp_had_subjects_traj": (I, [V, P, I, P, P, P, P, P, ctypes.POINTER(ctypes.c_int)]),
    "nmgp_had_subjects_traj_commit": (I, [V, ctypes.POINTER(ctypes.c_int)]),
    "nmgp_had_subjects_traj_end": (I, [V]),
    "nmgp_had_subjects_adam_begin": (I, [V, I, P, I, I, P, I]),
    "nmgp_had_subjects_adam": (I, [V, I, D, D, D, D, P, ctypes.POINTER(ctypes.c_int)]),
    "nmgp_had_subjects_adam_get_pars": (I, [V, P]),
    "nmgp_had_subjects_adam_end": (I, [V]),
    "nmgp_had_subjects_prior_apply": (I, [V, I, P, I, P, I, I, P]),
    "nmgp_predsample_had_subjects": (I, [V, P, I, I, P, P, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), I, P, P, P, P, P,
                                         ctypes.POINTER(ctypes.c_int)]),
    "nmgp_predsample_hads_subjects": (I, [V, P, I, I, P, P, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), I, P, P, P, P, P,
                                          ctypes.POINTER(ctypes.c_int)]),
    "nmgp_predict_hadst_subjects": (I, [V, P, I, I, P, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), I, P, P,
                                        ctypes.POINTER(ctypes.c_int)]),
    "nmgp_hads_batch_eval": (I, [V, P, I, P, I, P, P, ctypes.POINTER(ctypes.c_int)]),
    "nmgp_hads_covariance": (I, [V, P, P]),
    "nmgp_predict_hads": (I, [V, P, P, P, I, P, P, P]),
    "nmgp_hadst_batch_eval": (I, [V, P, I, P, I, P, P, ctypes.POINTER(ctypes.c_int)]),
    "nmgp_hadst_covariance": (I, [V, P, P]),
    "nmgp_predict_hadst": (I, [V, P, I, P, ctypes.POINTER(ctypes.c_int), I, P, P, ctypes.POINTER(ctypes.c_int)]),
    "nmgp_predsample_svc": (I, [V, P, I, P, P, I, I, P, P, P, P, P, ctypes.POINTER(ctypes.c_int)]),
    "nmgp_predsample_sep": (I, [V, P, I, P, P, I, I, P, P, P, P, P, ctypes.POINTER(ctypes.c_int)]),
    "nmgp_predsample_sta": (I, [V, P, I, P, I, P, P, ctypes.POINTER(ctypes.c_int)]),
    "nmgp_predsample_hads": (I, [V, P, I, P, P, ctypes.POINTER(ctypes.c_int), I, P, P, P, P, P, ctypes.POINTER(ctypes.c_int)]),
    "nmgp_predsample_had": (I, [V, P, I, P, P, ctypes.POINTER(ctypes.c_int), I, P, P, P, P, P, ctypes.POINTER(ctypes.c_int)]),
    "nmgp_profile_enable": (I, [V, I]),
    "nmgp_profile_read": (I, [V, P, c_ll_p]),
    "nmgp_profile_reset": (I, [V]),
    "nmgp_profile_read_work": (I, [V, P, c_ll_p, P, P]),
    "nmgp_last_sep_attempts": (I, [V]),
    "nmgp_measure_hbm_gbs": (I, [V, ctypes.c_longlong, I, P]),
    "nmgp_measure_hbm_rates": (I, [V, ctypes.c_longlong, I, P]),
    "nmgp_measure_dgemm_tflops": (I, [V, I, I, P]),
}

_lib = None
_lock = threading.Lock()


class NmgpError(RuntimeError):
    """API misuse or HIP runtime failure reported by libnmgp_hip.so (negative return code)."""


class NmgpNumericalError(RuntimeError):
    """Numerical failure (positive return code): covariance not positive definite, NaN, eigensolver."""

    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


def load(require_gpu=True):
    """Load the shared object and bind every symbol of the ABI.  Raises if it is absent: there is no fallback."""
    global _lib
    # torch bundles its own ROCm runtime (libamdhip64 / rocBLAS / rocSOLVER with the same sonames as /opt/rocm).
    # Two HIP runtimes in one process crash, so torch must be loaded FIRST: libnmgp_hip.so then binds to the copies
    # already in the process.  (A pure C/C++ host links /opt/rocm directly; see INTEGRATION.md.)
    import torch  # noqa: F401
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise NmgpError(
                    "libnmgp_hip.so is missing (%s). Build it with `python -m "
                    "nonstationary_multivariate_gaussian_process_amd.build` (needs hipcc); this package has no CPU "
                    "fallback." % LIB_PATH)
            lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
            for name, (res, args) in SIGNATURES.items():
                fn = getattr(lib, name)        # AttributeError if the .so does not export it
                fn.restype = res
                fn.argtypes = args
            # provenance: the shared object must be the build of THIS tree (sources + headers + flags), not a stale one
            from . import build as _build
            have, want = lib.nmgp_build_id().decode(), _build.tree_id()
            if have != want:
                raise NmgpError("libnmgp_hip.so is stale: it was built from tree %s..., the sources beside it hash to %s... "
                                "Rebuild with `python -m nonstationary_multivariate_gaussian_process_amd.build`." % (have[:16], want[:16]))
            _lib = lib
    if require_gpu and _lib.nmgp_device_count() <= 0:
        raise NmgpError("no HIP device is visible: the MI355X path cannot run (and there is no CPU fallback)")
    return _lib


def build_id():
    """The loaded library's build id (== build.tree_id() of the tree, or load() would have refused it)."""
    return load(require_gpu=False).nmgp_build_id().decode()


def as_f64(a):
    """Contiguous float64 ndarray view/copy of array-like or CPU torch tensor."""
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


def ptr(a):
    return a.ctypes.data_as(c_double_p) if a is not None else None


class Context:
    """One nmgp_ctx: one GPU, one stream, one resident subject.  Not thread-safe."""

    def __init__(self, device=None):
        self.lib = load(require_gpu=True)
        if device is None:
            device = default_device()
        self.device = int(device)
        h = ctypes.c_void_p()
        rc = self.lib.nmgp_ctx_create(self.device, ctypes.byref(h))
        self.h = h
        if rc != 0:
            msg = self.lib.nmgp_last_error(h).decode() if h else "nmgp_ctx_create failed"
            raise NmgpError("nmgp_ctx_create(device=%d) -> %d: %s" % (self.device, rc, msg))
        self.N = self.M = self.T = 0
        self._data_key = None
        self._cohort = None              # (S, Nmax, M) of the Hadamard cohort, while one is set

    def close(self):
        if getattr(self, "h", None):
            self.lib.nmgp_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- error mapping --------------------------------------------------------------------------
    def check(self, rc):
        if rc == 0:
            return
        msg = self.lib.nmgp_last_error(self.h).decode()
        if rc > 0:
            raise NmgpNumericalError(rc, msg)
        raise NmgpError("libnmgp_hip error %d: %s" % (rc, msg))

    # -- data -----------------------------------------------------------------------------------
    def set_data(self, x, Y):
        x = as_f64(x).reshape(-1)
        Y = as_f64(Y)
        if Y.ndim != 2 or Y.shape[0] != x.shape[0]:
            raise NmgpError("Y must be [N, M] with N == len(x); got Y%s x%s" % (Y.shape, x.shape))
        key = ("complete", x.shape, Y.shape, hash(x.tobytes()), hash(Y.tobytes()))
        if key == self._data_key:
            self.sep_batch_clear_subjects()      # (the upload, which would drop a separable subject set, is skipped)
            return
        self.check(self.lib.nmgp_set_data(self.h, ptr(x), ptr(Y), Y.shape[0], Y.shape[1]))
        self.N, self.M = Y.shape
        self.T = self.M * (self.M + 1) // 2
        self._data_key = key

    def sync(self):
        self.check(self.lib.nmgp_sync(self.h))

    # -- nonseparable ---------------------------------------------------------------------------
    def logpos_svc(self, pars, hyper, prior=True, want_grad=False):
        pars = as_f64(pars).reshape(-1)
        P_ = self.N * (1 + self.T) + 1
        if pars.shape[0] != P_:
            raise NmgpError("parameter vector has length %d, expected N(1+T)+1 = %d" % (pars.shape[0], P_))
        hyper = as_f64(hyper)
        out = np.empty(5)
        grad = np.empty(P_) if want_grad else None
        self.check(self.lib.nmgp_logpos_svc(self.h, ptr(pars), ptr(hyper), int(bool(prior)), ptr(out), ptr(grad)))
        return out, grad

    def svc_set_pars(self, pars):
        pars = as_f64(pars).reshape(-1)
        if pars.shape[0] != self.N * (1 + self.T) + 1:
            raise NmgpError("bad parameter vector length %d" % pars.shape[0])
        self.check(self.lib.nmgp_svc_set_pars(self.h, ptr(pars)))
        self.sync()      # the host buffer may be a temporary

    def svc_eval_resident(self, hyper, prior=True, want_grad=False):
        hyper = as_f64(hyper)
        self.check(self.lib.nmgp_svc_eval_resident(self.h, ptr(hyper), int(bool(prior)), int(bool(want_grad))))

    def svc_fetch(self, want_grad=False):
        out = np.empty(5)
        grad = np.empty(self.N * (1 + self.T) + 1) if want_grad else None
        self.check(self.lib.nmgp_svc_fetch(self.h, ptr(out), ptr(grad)))
        return out, grad

    # -- batched chains ---------------------------------------------------------------------------
    def svc_batch_alloc(self, B):
        self.check(self.lib.nmgp_svc_batch_alloc(self.h, int(B)))
        self.B = int(B)

    def svc_batch_set_pars(self, pars):
        pars = as_f64(pars)
        P_ = self.N * (1 + self.T) + 1
        if pars.shape != (self.B, P_):
            raise NmgpError("batched parameters must be [B=%d, P=%d], got %s" % (self.B, P_, pars.shape))
        self.check(self.lib.nmgp_svc_batch_set_pars(self.h, ptr(pars)))
        self.sync()

    def svc_batch_set_subjects(self, xs, Ys, chains_per_subject=1):
        """The batch holds S = B / chains_per_subject subjects: xs [S, N], Ys [S, N, M] (same N, M as set_data); batch element
        b = s * chains_per_subject + k is chain k of subject s.  With the default of 1 every batch element is its own subject."""
        xs, Ys = as_f64(xs), as_f64(Ys)
        k = int(chains_per_subject)
        if k < 1 or self.B % k:
            raise NmgpError("the batch size %d is not a multiple of chains_per_subject = %d" % (self.B, k))
        S = self.B // k
        if xs.shape != (S, self.N) or Ys.shape != (S, self.N, self.M):
            raise NmgpError("subjects must be xs [S=%d, N=%d], Ys [S, N, M=%d]; got %s, %s"
                            % (S, self.N, self.M, xs.shape, Ys.shape))
        self.check(self.lib.nmgp_svc_batch_set_subjects_chains(self.h, ptr(xs), ptr(Ys), k))

    def svc_batch_eval(self, hyper, prior=True, want_grad=False):
        hyper = as_f64(hyper)
        self.check(self.lib.nmgp_svc_batch_eval(self.h, ptr(hyper), int(bool(prior)), int(bool(want_grad))))

    def svc_batch_fetch_grad(self):
        grad = np.empty((self.B, self.N * (1 + self.T) + 1))
        self.check(self.lib.nmgp_svc_batch_fetch_grad(self.h, ptr(grad)))
        return grad

    def svc_batch_fetch(self):
        out = np.empty((self.B, 5))
        status = np.zeros(self.B, dtype=np.int32)
        self.check(self.lib.nmgp_svc_batch_fetch(self.h, ptr(out), status.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return out, status

    # -- device-resident leapfrog trajectories of the batch (HMC) ---------------------------------
    def svc_batch_traj_begin(self):
        """After set_pars + batch_eval(want_grad=True) at the start positions: positions and gradients become the state
        the trajectories start from."""
        self.check(self.lib.nmgp_svc_batch_traj_begin(self.h))

    def svc_batch_traj_set_mass(self, minv=None):
        """Mass matrix of the device-resident trajectories: None (identity), diag(M^-1) [P] or dense M^-1 [P, P]."""
        if minv is None:
            self.check(self.lib.nmgp_svc_batch_traj_set_mass(self.h, 0, None))
            return
        minv = as_f64(minv)
        P = self.N * (1 + self.T) + 1
        if minv.shape == (P,):
            kind = 1
        elif minv.shape == (P, P):
            kind = 2
        else:
            raise ValueError("minv must be [P] or [P, P] with P = %d" % P)
        self.check(self.lib.nmgp_svc_batch_traj_set_mass(self.h, kind, ptr(minv)))

    def svc_batch_traj_set_mass_chol(self, mchol):
        """chol(M) of the mass matrix set by svc_batch_traj_set_mass: sqrt(diag M) [P] or a square root R [P, P] with R R^T = M
        (NumPy row-major; np.linalg.cholesky(M), or e.g. L^-T when M^-1 = L L^T is what one has) -- lets svc_batch_traj_z draw
        the momenta p = R z on the device."""
        mchol = as_f64(mchol)
        P = self.N * (1 + self.T) + 1
        if mchol.shape == (P,):
            self.check(self.lib.nmgp_svc_batch_traj_set_mass_chol(self.h, 1, ptr(mchol)))
        elif mchol.shape == (P, P):
            mt = np.ascontiguousarray(mchol.T)                   # column-major R == row-major of its transpose
            self.check(self.lib.nmgp_svc_batch_traj_set_mass_chol(self.h, 2, ptr(mt)))
        else:
            raise ValueError("mchol must be [P] or [P, P] with P = %d" % P)

    def svc_batch_traj_set_mass_prior(self, hyper, U=None, lam=None):
        """The prior-factor metric M^-1 = L_blk (I + U diag(lam) U^T)^-1 L_blk^T of the trajectories (nmgp.h): L_blk from the cached
        GP-prior factors named by hyper [8]; U [r, P] (one subject) or [S, r, P], lam [r] / [S, r] >= 0 the optional low-rank
        correction in whitened coordinates (drivers.prior_lowrank_metric builds it)."""
        hyper = as_f64(hyper)
        if U is None:
            self.check(self.lib.nmgp_svc_batch_traj_set_mass_prior(self.h, ptr(hyper), 0, None, None))
            return
        U, lam = as_f64(U), as_f64(lam)
        P_ = self.N * (1 + self.T) + 1
        if U.ndim == 2:
            U, lam = U[None], lam.reshape(1, -1)
        if U.ndim != 3 or U.shape[2] != P_ or lam.shape != U.shape[:2]:
            raise NmgpError("U must be [S, r, P=%d] with lam [S, r]; got %s, %s" % (P_, U.shape, lam.shape))
        U, lam = np.ascontiguousarray(U), np.ascontiguousarray(lam)
        self.check(self.lib.nmgp_svc_batch_traj_set_mass_prior(self.h, ptr(hyper), int(U.shape[1]), ptr(U), ptr(lam)))

    def svc_batch_prior_apply(self, hyper, v, trans=False):
        """L_blk v (trans=False) or L_blk^T v (trans=True) for B parameter-shaped vectors v [B, P]: the change of coordinates of the
        prior-factor metric (L_blk = blockdiag of the GP-prior Cholesky factors, 1 for the noise parameter)."""
        hyper, v = as_f64(hyper), as_f64(v)
        P_ = self.N * (1 + self.T) + 1
        if v.shape != (self.B, P_):
            raise NmgpError("v must be [B=%d, P=%d], got %s" % (self.B, P_, v.shape))
        out = np.empty_like(v)
        self.check(self.lib.nmgp_svc_batch_prior_apply(self.h, ptr(hyper), int(bool(trans)), ptr(v), ptr(out)))
        return out

    def sep_prior_apply(self, hyper, v, trans=False):
        """L_blk v / L_blk^T v for B vectors v [B, 2N+T+1] of the SEPARABLE parameter layout: L_blk = blockdiag(chol Sigma_l,
        chol Sigma_sigma, c I_T, 1) from the cached GP-prior factors named by hyper [9]."""
        hyper, v = as_f64(hyper), as_f64(v)
        P_ = 2 * self.N + self.T + 1
        if v.ndim != 2 or v.shape[1] != P_:
            raise NmgpError("v must be [B, 2N+T+1 = %d], got %s" % (P_, v.shape))
        out = np.empty_like(v)
        self.check(self.lib.nmgp_sep_prior_apply(self.h, ptr(hyper), int(bool(trans)), int(v.shape[0]), ptr(v), ptr(out)))
        return out

    def svc_batch_traj_z(self, hyper, prior, eps, nsteps, z):
        """One leapfrog trajectory per chain with momenta p0 = chol(M) z formed on the device from the standard normals z [B, P]:
        returns the end point q1 [B, P], the kinetic energy there kin1 [B] = 1/2 p1^T M^-1 p1, the potential U1 [B] (inf for failed
        chains) and failed [B] (bool)."""
        hyper, z = as_f64(hyper), as_f64(z)
        P_ = self.N * (1 + self.T) + 1
        if z.shape != (self.B, P_):
            raise NmgpError("z must be [B=%d, P=%d], got %s" % (self.B, P_, z.shape))
        q1, kin1, U1 = np.empty((self.B, P_)), np.empty(self.B), np.empty(self.B)
        failed = np.zeros(self.B, dtype=np.int32)
        self.check(self.lib.nmgp_svc_batch_traj_z(self.h, ptr(hyper), int(bool(prior)), float(eps), int(nsteps), ptr(z),
                                                  ptr(q1), ptr(kin1), ptr(U1),
                                                  failed.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return q1, kin1, U1, failed.astype(bool)

    def svc_batch_traj(self, hyper, prior, eps, nsteps, p0):
        """One leapfrog trajectory per chain from the resident state with momenta p0 [B, P]: returns the end point
        (q1, p1 [B, P]), the potential there U1 [B] (inf for failed chains) and failed [B] (bool)."""
        hyper, p0 = as_f64(hyper), as_f64(p0)
        P_ = self.N * (1 + self.T) + 1
        if p0.shape != (self.B, P_):
            raise NmgpError("momenta must be [B=%d, P=%d], got %s" % (self.B, P_, p0.shape))
        q1, p1, U1 = np.empty((self.B, P_)), np.empty((self.B, P_)), np.empty(self.B)
        failed = np.zeros(self.B, dtype=np.int32)
        self.check(self.lib.nmgp_svc_batch_traj(self.h, ptr(hyper), int(bool(prior)), float(eps), int(nsteps), ptr(p0),
                                                ptr(q1), ptr(p1), ptr(U1),
                                                failed.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return q1, p1, U1, failed.astype(bool)

    def svc_batch_traj_commit(self, accept):
        acc = np.ascontiguousarray(np.asarray(accept).astype(np.int32))
        if acc.shape != (self.B,):
            raise NmgpError("accept must be [B=%d]" % self.B)
        self.check(self.lib.nmgp_svc_batch_traj_commit(self.h, acc.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))

    # -- device-resident Adam over the batch (MAP) ------------------------------------------------
    def svc_batch_adam_begin(self):
        self.check(self.lib.nmgp_svc_batch_adam_begin(self.h))

    def svc_batch_adam_step(self, hyper, prior, lr, beta1=0.9, beta2=0.999, eps=1e-8):
        """One Adam iteration of every batch element on the device: returns the verbose tuples [B, 5] at the parameters the
        iteration started from and alive [B] (bool)."""
        hyper = as_f64(hyper)
        out = np.empty((self.B, 5))
        alive = np.zeros(self.B, dtype=np.int32)
        self.check(self.lib.nmgp_svc_batch_adam_step(self.h, ptr(hyper), int(bool(prior)), float(lr), float(beta1),
                                                     float(beta2), float(eps), ptr(out),
                                                     alive.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return out, alive.astype(bool)

    def svc_batch_get_pars(self):
        pars = np.empty((self.B, self.N * (1 + self.T) + 1))
        self.check(self.lib.nmgp_svc_batch_get_pars(self.h, ptr(pars)))
        return pars

    def svc_covariance(self, pars):
        pars = as_f64(pars).reshape(-1)
        n = self.N * self.M
        out = np.empty((n, n))
        self.check(self.lib.nmgp_svc_covariance(self.h, ptr(pars), ptr(out)))
        return out

    # -- separable / stationary -------------------------------------------------------------------
    def logpos_sep(self, pars, hyper, prior=True, want_grad=False):
        pars = as_f64(pars).reshape(-1)
        P_ = 2 * self.N + self.T + 1
        if pars.shape[0] != P_:
            raise NmgpError("parameter vector has length %d, expected 2N+T+1 = %d" % (pars.shape[0], P_))
        hyper = as_f64(hyper)
        out = np.empty(6)
        grad = np.empty(P_) if want_grad else None
        self.check(self.lib.nmgp_logpos_sep(self.h, ptr(pars), ptr(hyper), int(bool(prior)), ptr(out), ptr(grad)))
        return out, grad

    def sep_batch_eval(self, pars, hyper, prior=True, want_grad=False):
        """B chains of the separable model in one launch sequence: pars [B, 2N+T+1] -> (out [B, 6], grad [B, P] or None,
        status [B]: 0 exact, 1..3 jitter retries needed, negative = numerical failure even so (row NaN))."""
        pars = as_f64(pars)
        P_ = 2 * self.N + self.T + 1
        if pars.ndim != 2 or pars.shape[1] != P_:
            raise NmgpError("parameters must be [B, 2N+T+1 = %d], got %s" % (P_, pars.shape))
        hyper = as_f64(hyper)
        B = pars.shape[0]
        out = np.empty((B, 6))
        grad = np.empty((B, P_)) if want_grad else None
        status = np.zeros(B, dtype=np.int32)
        self.check(self.lib.nmgp_sep_batch_eval(self.h, ptr(pars), B, ptr(hyper), int(bool(prior)), ptr(out), ptr(grad),
                                                status.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return out, grad, status

    def sep_batch_set_subjects(self, xs, Ys, chains_per_subject=1):
        """S subjects of the separable model for ``sep_batch_eval``: xs [S, N], Ys [S, N, M] (N, M of ``set_data``).  While the set is
        active ``sep_batch_eval`` takes pars [S * chains_per_subject, 2N+T+1], row s * chains_per_subject + k being chain k of subject
        s.  ``sep_batch_clear_subjects``, ``set_data`` and ``had_set_data`` end it; every other entry keeps using the resident
        subject."""
        xs, Ys = as_f64(xs), as_f64(Ys)
        if xs.ndim != 2 or Ys.ndim != 3 or Ys.shape[0] != xs.shape[0]:
            raise NmgpError("subjects must be xs [S, N], Ys [S, N, M]; got %s, %s" % (xs.shape, Ys.shape))
        if self.N and (xs.shape[1] != self.N or Ys.shape[1:] != (self.N, self.M)):
            raise NmgpError("subjects must be xs [S, N=%d], Ys [S, N, M=%d]; got %s, %s" % (self.N, self.M, xs.shape, Ys.shape))
        self.check(self.lib.nmgp_sep_batch_set_subjects_chains(self.h, ptr(xs), ptr(Ys), xs.shape[0], int(chains_per_subject)))

    def sep_batch_clear_subjects(self):
        self.check(self.lib.nmgp_sep_batch_clear_subjects(self.h))

    def logpos_sta(self, pars, hyper, prior=True, want_grad=False):
        pars = as_f64(pars).reshape(-1)
        P_ = self.T + 3
        if pars.shape[0] != P_:
            raise NmgpError("parameter vector has length %d, expected T+3 = %d" % (pars.shape[0], P_))
        hyper = as_f64(hyper)
        out = np.empty(5)
        grad = np.empty(P_) if want_grad else None
        self.check(self.lib.nmgp_logpos_sta(self.h, ptr(pars), ptr(hyper), int(bool(prior)), ptr(out), ptr(grad)))
        return out, grad

    def sta_batch_eval(self, pars, hyper, prior=True, want_grad=False):
        """B chains of the stationary (LMC) model in one launch sequence: pars [B, T+3] (or one vector [T+3]) -> (out [B, 5] as
        ``logpos_sta``, grad [B, T+3] or None, status [B]: 0 exact, 1..3 jitter retries needed, negative = numerical failure even so
        (row NaN, gradient row zero)).  A chain's bits do not depend on B.  While a subject set is active (``sta_batch_set_subjects``)
        row s * chains_per_subject + k is chain k of subject s."""
        pars = as_f64(pars)
        P_ = self.T + 3
        if pars.ndim == 1:
            pars = pars.reshape(1, -1)
        if pars.ndim != 2 or pars.shape[1] != P_:
            raise NmgpError("parameters must be [B, T+3 = %d], got %s" % (P_, pars.shape))
        hyper = as_f64(hyper)
        if hyper.size != 5:
            raise NmgpError("the stationary model takes 5 hyper-parameters, got %d" % hyper.size)
        B = pars.shape[0]
        out = np.empty((B, 5))
        grad = np.empty((B, P_)) if want_grad else None
        status = np.zeros(B, dtype=np.int32)
        self.check(self.lib.nmgp_sta_batch_eval(self.h, ptr(pars), B, ptr(hyper), int(bool(prior)), ptr(out), ptr(grad),
                                                status.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return out, grad, status

    def sta_batch_set_subjects(self, xs, Ys, chains_per_subject=1):
        """Alias of ``sep_batch_set_subjects``: the stationary and the separable batched entries share ONE subject set (xs [S, N],
        Ys [S, N, M]); the stationary model has no GP priors, so nothing per subject is factored for it."""
        self.sep_batch_set_subjects(xs, Ys, chains_per_subject)

    def sta_batch_clear_subjects(self):
        """Alias of ``sep_batch_clear_subjects``."""
        self.sep_batch_clear_subjects()

    # -- primitives -----------------------------------------------------------------------------
    def pairwise_distances(self, x1, x2=None):
        x1 = as_f64(x1)
        x2a = None if x2 is None else as_f64(x2)
        n1, d = x1.shape
        n2 = n1 if x2a is None else x2a.shape[0]
        out = np.empty((n1, n2))
        self.check(self.lib.nmgp_pairwise_distances(self.h, ptr(x1), n1, ptr(x2a), n2, d, ptr(out)))
        return out

    def rbf_cov(self, x1, x2=None, alpha=1.0, beta=1.0):
        x1 = as_f64(x1)
        x2a = None if x2 is None else as_f64(x2)
        n1, d = x1.shape
        n2 = n1 if x2a is None else x2a.shape[0]
        out = np.empty((n1, n2))
        self.check(self.lib.nmgp_rbf_cov(self.h, ptr(x1), n1, ptr(x2a), n2, d, float(alpha), float(beta), ptr(out)))
        return out

    def nonstat_rbf_cov(self, x1, s1=None, l1=None, x2=None, s2=None, l2=None):
        x1 = as_f64(x1)
        n1, d = x1.shape
        s1a = None if s1 is None else as_f64(s1).reshape(-1)
        l1a = None if l1 is None else as_f64(l1).reshape(-1)
        x2a = None if x2 is None else as_f64(x2)
        s2a = None if (x2 is None or s2 is None) else as_f64(s2).reshape(-1)
        l2a = None if (x2 is None or l2 is None) else as_f64(l2).reshape(-1)
        n2 = n1 if x2a is None else x2a.shape[0]
        out = np.empty((n1, n2))
        self.check(self.lib.nmgp_nonstat_rbf_cov(self.h, ptr(x1), ptr(s1a), ptr(l1a), n1, ptr(x2a), ptr(s2a), ptr(l2a),
                                                 n2, d, ptr(out)))
        return out

    def kron_product(self, a, b):
        a, b = as_f64(a), as_f64(b)
        out = np.empty((a.shape[0] * b.shape[0], a.shape[1] * b.shape[1]))
        self.check(self.lib.nmgp_kron_product(self.h, ptr(a), a.shape[0], a.shape[1], ptr(b), b.shape[0], b.shape[1],
                                              ptr(out)))
        return out

    def kron_mv(self, B, K, y):
        B, K, y = as_f64(B), as_f64(K), as_f64(y).reshape(-1)
        if y.shape[0] != B.shape[1] * K.shape[1]:
            raise NmgpError("kron_mv: y has length %d, expected %d" % (y.shape[0], B.shape[1] * K.shape[1]))
        out = np.empty(B.shape[0] * K.shape[0])
        self.check(self.lib.nmgp_kron_mv(self.h, ptr(B), B.shape[0], B.shape[1], ptr(K), K.shape[0], K.shape[1], ptr(y),
                                         ptr(out)))
        return out

    def mvn_logpdf(self, y, mu, logdet, inv):
        y, inv = as_f64(y).reshape(-1), as_f64(inv)
        mua = None if mu is None else as_f64(mu).reshape(-1)
        out = np.empty(1)
        self.check(self.lib.nmgp_mvn_logpdf(self.h, ptr(y), ptr(mua), float(logdet), ptr(inv), y.shape[0], ptr(out)))
        return float(out[0])

    def mvn_logpdf_kron(self, y, mu, B, K, sigma2, dense=False):
        y, B, K = as_f64(y).reshape(-1), as_f64(B), as_f64(K)
        mua = None if mu is None else as_f64(mu).reshape(-1)
        out = np.empty(1)
        fn = self.lib.nmgp_mvn_logpdf_dense if dense else self.lib.nmgp_mvn_logpdf_kron
        self.check(fn(self.h, ptr(y), ptr(mua), ptr(B), B.shape[0], ptr(K), K.shape[0], float(sigma2), ptr(out)))
        return float(out[0])

    def kron_inv_logdet(self, sigma2, B, K, want_inv=True):
        B, K = as_f64(B), as_f64(K)
        n = B.shape[0] * K.shape[0]
        inv = np.empty((n, n)) if want_inv else None
        ld = np.empty(1)
        self.check(self.lib.nmgp_kron_inv_logdet(self.h, float(sigma2), ptr(B), B.shape[0], ptr(K), K.shape[0], ptr(inv),
                                                 ptr(ld)))
        return inv, float(ld[0])

    def cholesky(self, A, rhs=None, algo=1):
        """Lower Cholesky factor of the SPD matrix A (and L^-1 rhs when rhs is given)."""
        A = as_f64(A)
        n = A.shape[0]
        rhsa = None if rhs is None else as_f64(rhs).reshape(-1)
        out = np.empty((n, n))
        z = np.empty(n) if rhsa is not None else None
        self.check(self.lib.nmgp_cholesky(self.h, ptr(A), n, ptr(rhsa), ptr(out), ptr(z), int(algo)))
        L = np.tril(out.T)           # the library's column-major lower triangle == row-major upper
        return (L, z) if rhsa is not None else L

    def cholesky_batch(self, A, rows=None, want_xtri=False, want_inv=0, precise=False):
        """The batched custom factorisation on caller-supplied matrices, laid out and launched as the batched objectives do it.
        A [B, n, n] symmetric (only the triangle ``cholesky`` reads is uploaded), rows [B, extra, n] dense rows carried below each
        matrix.  Returns (L, R, X, Sinv, status) in the orientation of ``cholesky``: L [B, n, n] lower factors, R [B, extra, n] =
        rows L^-T (None without rows), X [B, n, n] = L^-T with want_xtri (only its upper triangle is promised: left of the diagonal
        it holds whatever the device buffer held), Sinv [B, n, n] = -X X^T with want_inv (1: lower triangle, the rest zero; 2: both
        triangles), status [B] (0, or the first leading minor that is not positive definite: such a matrix does not raise)."""
        A = as_f64(A)
        if A.ndim != 3 or A.shape[1] != A.shape[2]:
            raise NmgpError("A must be [B, n, n]")
        B, n = A.shape[0], A.shape[1]
        ra = None if rows is None else as_f64(rows)
        if ra is not None and (ra.ndim != 3 or ra.shape[0] != B or ra.shape[2] != n):
            raise NmgpError("rows must be [B=%d, extra, n=%d]" % (B, n))
        if ra is not None and ra.shape[1] == 0:
            ra = None
        extra = 0 if ra is None else ra.shape[1]
        L = np.empty((B, n, n))
        R = None if ra is None else np.empty((B, extra, n))
        X = np.empty((B, n, n)) if want_xtri else None
        Sinv = np.empty((B, n, n)) if want_inv else None
        status = np.zeros(B, dtype=np.int32)
        self.check(self.lib.nmgp_cholesky_batch(self.h, ptr(A), n, B, ptr(ra), extra, int(bool(want_xtri)), int(want_inv),
                                                int(bool(precise)), ptr(L), ptr(R), ptr(X), ptr(Sinv),
                                                status.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        # the library's column-major matrices are the row-major transposes
        L = np.ascontiguousarray(L.transpose(0, 2, 1))
        if X is not None:
            X = np.ascontiguousarray(X.transpose(0, 2, 1))
        if Sinv is not None:
            Sinv = np.ascontiguousarray(Sinv.transpose(0, 2, 1))
            if int(want_inv) == 1:
                Sinv = np.tril(Sinv)          # the other triangle is not written
        return L, R, X, Sinv, status

    # -- prediction -----------------------------------------------------------------------------
    def predict_svc(self, pars, hyper, xs):
        pars, hyper, xs = as_f64(pars).reshape(-1), as_f64(hyper), as_f64(xs).reshape(-1)
        S = xs.shape[0]
        mean, var, Ls = np.empty((S, self.M)), np.empty((S, self.M)), np.empty((S, self.T))
        self.check(self.lib.nmgp_predict_svc(self.h, ptr(pars), ptr(hyper), ptr(xs), S, ptr(mean), ptr(var), ptr(Ls)))
        return mean, var, Ls

    def predict_sep(self, pars, hyper, xs):
        pars, hyper, xs = as_f64(pars).reshape(-1), as_f64(hyper), as_f64(xs).reshape(-1)
        S = xs.shape[0]
        mean, var = np.empty((S, self.M)), np.empty((S, self.M))
        self.check(self.lib.nmgp_predict_sep(self.h, ptr(pars), ptr(hyper), ptr(xs), S, ptr(mean), ptr(var)))
        return mean, var

    def predict_sta(self, pars, xs):
        pars, xs = as_f64(pars).reshape(-1), as_f64(xs).reshape(-1)
        S = xs.shape[0]
        mean, var = np.empty((S, self.M)), np.empty((S, self.M))
        self.check(self.lib.nmgp_predict_sta(self.h, ptr(pars), ptr(xs), S, ptr(mean), ptr(var)))
        return mean, var

    def predsample_svc(self, pars_hist, hyper, xs, z=None, star=None, constrained=True):
        """Posterior-draw prediction: H parameter vectors pars_hist [H, P] of the resident subject at the new inputs xs [S].
        z [H, S, 1+T]: standard normals of the latent regression (None: the conditional means); star [H, S, 1+T]: starred values
        (tilde_l*, the T slots of L*) to use instead of regressing (z must then be None).  constrained=True is the `predsample`
        family's regression on the constrained L_vecs, False the `predmap_*_sampling` family's on uL_vecs (nmgp.h).
        Returns (mean [H, S, M], var [H, S, M], star [H, S, 1+T], status [H]); a draw with non-zero status has NaN rows."""
        pars = as_f64(pars_hist)
        if pars.ndim == 1:
            pars = pars[None]
        P_ = self.N * (1 + self.T) + 1
        if pars.ndim != 2 or pars.shape[1] != P_:
            raise NmgpError("draws must be [H, P=%d], got %s" % (P_, pars.shape))
        hyper, xs = as_f64(hyper), as_f64(xs).reshape(-1)
        H, S = pars.shape[0], xs.shape[0]
        if z is not None and star is not None:
            raise NmgpError("star= replaces the regression: z must be None")
        za = sa = None
        for name, a in (("z", z), ("star", star)):
            if a is not None:
                a = as_f64(a)
                if a.shape != (H, S, 1 + self.T):
                    raise NmgpError("%s must be [H=%d, S=%d, 1+T=%d], got %s" % (name, H, S, 1 + self.T, a.shape))
                if name == "z":
                    za = a
                else:
                    sa = a
        mean, var = np.empty((H, S, self.M)), np.empty((H, S, self.M))
        star_out = np.empty((H, S, 1 + self.T))
        status = np.zeros(H, dtype=np.int32)
        self.check(self.lib.nmgp_predsample_svc(self.h, ptr(pars), H, ptr(hyper), ptr(xs), S, int(bool(constrained)), ptr(za),
                                                ptr(sa), ptr(mean), ptr(var), ptr(star_out),
                                                status.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return mean, var, star_out, status

    def predsample_sep(self, pars_hist, hyper, xs, z=None, star=None, kss_jitter=True):
        """Posterior-draw prediction of the SEPARABLE model: pars_hist [H, 2N+T+1] of the resident subject at the new inputs xs [S].
        z [H, S, 2]: standard normals of the latent regression of (tilde_l*, tilde_sigma*) (None: the conditional means); star
        [H, S, 2]: starred values to use instead of regressing (z must then be None).  kss_jitter=True is the `predsample` family's
        a2 = B_mm (sigma*^2 + 1e-6), False the `predmap_sampling` family's B_mm sigma*^2 (nmgp.h).
        Returns (mean [H, S, M], var [H, S, M], star [H, S, 2], status [H]); a draw with non-zero status has NaN rows."""
        pars = as_f64(pars_hist)
        if pars.ndim == 1:
            pars = pars[None]
        P_ = 2 * self.N + self.T + 1
        if pars.ndim != 2 or pars.shape[1] != P_:
            raise NmgpError("draws must be [H, P=%d], got %s" % (P_, pars.shape))
        hyper, xs = as_f64(hyper), as_f64(xs).reshape(-1)
        H, S = pars.shape[0], xs.shape[0]
        if z is not None and star is not None:
            raise NmgpError("star= replaces the regression: z must be None")
        za = sa = None
        for name, a in (("z", z), ("star", star)):
            if a is not None:
                a = as_f64(a)
                if a.shape != (H, S, 2):
                    raise NmgpError("%s must be [H=%d, S=%d, 2], got %s" % (name, H, S, a.shape))
                if name == "z":
                    za = a
                else:
                    sa = a
        mean, var = np.empty((H, S, self.M)), np.empty((H, S, self.M))
        star_out = np.empty((H, S, 2))
        status = np.zeros(H, dtype=np.int32)
        self.check(self.lib.nmgp_predsample_sep(self.h, ptr(pars), H, ptr(hyper), ptr(xs), S, int(bool(kss_jitter)), ptr(za),
                                                ptr(sa), ptr(mean), ptr(var), ptr(star_out),
                                                status.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return mean, var, star_out, status

    def predsample_sta(self, pars_hist, xs):
        """Posterior-draw prediction of the STATIONARY model: pars_hist [H, T+3] at xs [S] (nothing is regressed, so there is no
        noise to inject).  Returns (mean [H, S, M], var [H, S, M], status [H])."""
        pars = as_f64(pars_hist)
        if pars.ndim == 1:
            pars = pars[None]
        if pars.ndim != 2 or pars.shape[1] != self.T + 3:
            raise NmgpError("draws must be [H, P=%d], got %s" % (self.T + 3, pars.shape))
        xs = as_f64(xs).reshape(-1)
        H, S = pars.shape[0], xs.shape[0]
        mean, var = np.empty((H, S, self.M)), np.empty((H, S, self.M))
        status = np.zeros(H, dtype=np.int32)
        self.check(self.lib.nmgp_predsample_sta(self.h, ptr(pars), H, ptr(xs), S, ptr(mean), ptr(var),
                                                status.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return mean, var, status

    # -- Hadamard form of the nonseparable model (irregularly observed outputs) -------------------
    def had_set_data(self, x, indx, y, M=None):
        """N single observations (x[i], indx[i], y[i]); M defaults to the number of distinct labels, as the reference infers it
        (logpos.py:579).  Replaces the resident subject: the complete-data entries raise until ``set_data`` is called again."""
        x, y = as_f64(x).reshape(-1), as_f64(y).reshape(-1)
        if hasattr(indx, "detach"):
            indx = indx.detach().cpu().numpy()
        indx = np.ascontiguousarray(np.asarray(indx).reshape(-1).astype(np.int32))
        if not (x.shape == y.shape == indx.shape):
            raise NmgpError("x, indx and y must have one length; got x%s indx%s y%s" % (x.shape, indx.shape, y.shape))
        M = int(np.unique(indx).shape[0]) if M is None else int(M)
        key = ("hadamard", M, x.shape, hash(x.tobytes()), hash(indx.tobytes()), hash(y.tobytes()))
        if key == self._data_key:
            self.sep_batch_clear_subjects()
            return
        self._data_key = None            # whatever was resident is gone even if the call fails
        self.check(self.lib.nmgp_had_set_data(self.h, ptr(x), indx.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), ptr(y),
                                              x.shape[0], M))
        self.N, self.M = x.shape[0], M
        self.T = M * (M + 1) // 2
        self._data_key = key

    def had_batch_eval(self, pars, hyper, prior=True, want_grad=False):
        """B parameter vectors of the resident Hadamard subject in one launch sequence: pars [B, N(1+T)+1] (or one vector) ->
        (out [B, 5], grad [B, P] or None, status [B]: 0, a leading-minor index or NUM_NAN; a failing chain has a NaN row and a
        zero gradient row)."""
        return self._had_eval(self.lib.nmgp_had_batch_eval, pars, self.N * (1 + self.T) + 1, 5, hyper, None, "N(1+T)+1", prior,
                              want_grad)

    def _had_eval(self, fn, pars, P_, width, hyper, n_hyper, what, prior, want_grad):
        """One batched evaluation entry of the three Hadamard models: pars [B, P_] (or one vector) -> (out [B, width], grad [B, P_]
        or None, status [B]).  ``what`` spells P_ in the error text; n_hyper=None: the length of hyper is not checked."""
        pars = as_f64(pars)
        if pars.ndim == 1:
            pars = pars[None]
        if pars.ndim != 2 or pars.shape[1] != P_:
            raise NmgpError("parameters must be [B, %s = %d], got %s" % (what, P_, pars.shape))
        hyper = as_f64(hyper)
        if n_hyper is not None:
            hyper = hyper.reshape(-1)
            if hyper.shape[0] != n_hyper:
                raise NmgpError("hyper must have %d entries, got %d" % (n_hyper, hyper.shape[0]))
        B = pars.shape[0]
        out = np.empty((B, width))
        grad = np.empty((B, P_)) if want_grad else None
        status = np.zeros(B, dtype=np.int32)
        self.check(fn(self.h, ptr(pars), B, ptr(hyper), int(bool(prior)), ptr(out), ptr(grad),
                      status.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return out, grad, status

    def _had_cov(self, fn, pars, P_, what):
        """One covariance entry of the three Hadamard models: the full symmetric [N, N] of one parameter vector of length P_;
        ``what`` is appended to the error text."""
        pars = as_f64(pars).reshape(-1)
        if pars.shape[0] != P_:
            raise NmgpError("bad parameter vector length %d%s" % (pars.shape[0], what))
        out = np.empty((self.N, self.N))
        self.check(fn(self.h, ptr(pars), ptr(out)))
        return out

    def had_covariance(self, pars):
        return self._had_cov(self.lib.nmgp_had_covariance, pars, self.N * (1 + self.T) + 1, "")

    # -- a cohort of ragged Hadamard subjects (independent of the resident subject) -----------------
    def had_set_subjects(self, xs, indxs, ys, M=None, Nmax=None):
        """S Hadamard subjects of ragged size for ``had_subjects_eval``: lists of per-subject arrays ``xs[s]``, ``indxs[s]``,
        ``ys[s]`` of length ``nobs[s]``.  ``M`` defaults to the number of distinct labels, which must be the same for all subjects;
        ``Nmax`` (the order every subject is padded to) defaults to ``max(nobs)``.  The set needs no resident subject, survives
        ``set_data`` / ``had_set_data``, and ends with ``had_clear_subjects``, the next ``had_set_subjects`` or the context."""
        xs = [as_f64(v).reshape(-1) for v in xs]
        ys = [as_f64(v).reshape(-1) for v in ys]
        labs = []
        for v in indxs:
            if hasattr(v, "detach"):
                v = v.detach().cpu().numpy()
            labs.append(np.asarray(v).reshape(-1).astype(np.int32))
        S = len(xs)
        if S < 1 or len(ys) != S or len(labs) != S:
            raise NmgpError("xs, indxs and ys must be lists of one positive length; got %d, %d, %d" % (S, len(labs), len(ys)))
        nobs = np.array([v.shape[0] for v in xs], dtype=np.int32)
        for s in range(S):
            if not (xs[s].shape == ys[s].shape == labs[s].shape):
                raise NmgpError("subject %d: x, indx and y must have one length; got x%s indx%s y%s"
                                % (s, xs[s].shape, labs[s].shape, ys[s].shape))
        if M is None:
            counts = sorted({int(np.unique(v).shape[0]) for v in labs})
            if len(counts) != 1:
                raise NmgpError("the subjects have different numbers of distinct labels %s: pass M" % counts)
            M = counts[0]
        M = int(M)
        Nmax = int(nobs.max()) if Nmax is None else int(Nmax)
        if nobs.max() > Nmax:
            raise NmgpError("a subject has %d observations, more than Nmax = %d" % (int(nobs.max()), Nmax))
        x2, y2 = np.zeros((S, max(Nmax, 1))), np.zeros((S, max(Nmax, 1)))
        i2 = np.zeros((S, max(Nmax, 1)), dtype=np.int32)
        for s in range(S):
            x2[s, :nobs[s]], y2[s, :nobs[s]], i2[s, :nobs[s]] = xs[s], ys[s], labs[s]
        self.had_set_subjects_padded(x2, i2, y2, nobs, M)

    def had_set_subjects_padded(self, x, indx, y, nobs, M):
        """The C entry as it is: x, indx (int32), y [S, Nmax] of which only the first nobs[s] entries of row s are read."""
        x, y = as_f64(x), as_f64(y)
        indx = np.ascontiguousarray(np.asarray(indx), dtype=np.int32)
        nobs = np.ascontiguousarray(np.asarray(nobs).reshape(-1), dtype=np.int32)
        if x.ndim != 2 or x.shape != y.shape or x.shape != indx.shape or nobs.shape[0] != x.shape[0]:
            raise NmgpError("x, indx, y must be [S, Nmax] and nobs [S]; got %s, %s, %s, %s" % (x.shape, indx.shape, y.shape, nobs.shape))
        ip = ctypes.POINTER(ctypes.c_int)
        # (a refused call leaves the previous set, and the shape recorded for it, in place)
        self.check(self.lib.nmgp_had_set_subjects(self.h, ptr(x), indx.ctypes.data_as(ip), ptr(y), nobs.ctypes.data_as(ip),
                                                  x.shape[0], x.shape[1], int(M)))
        self._cohort = (x.shape[0], x.shape[1], int(M))
        self._cohort_traj = None          # (a new set ends a begun trajectory and a begun optimiser)
        self._cohort_adam = None

    def had_clear_subjects(self):
        self.check(self.lib.nmgp_had_clear_subjects(self.h))
        self._cohort = None
        self._cohort_traj = None
        self._cohort_adam = None

    def had_subjects_eval(self, pars, hyper, prior=True, want_grad=False, chains_per_subject=1):
        """B = S * chains_per_subject chains of the cohort in one launch sequence: pars [B, Pmax = Nmax(1+T)+1] in the padded layout
        (``hadamard.cohort_pack``), row s * chains_per_subject + k being chain k of subject s -> (out [B, 5], grad [B, Pmax] or None
        with +0.0 in the padded slots, status [B] as ``had_batch_eval``).  Padded parameter slots are never read."""
        pars = as_f64(pars)
        if pars.ndim == 1:
            pars = pars[None]
        cohort = getattr(self, "_cohort", None)
        if cohort is not None:
            P_ = cohort[1] * (1 + cohort[2] * (cohort[2] + 1) // 2) + 1
            if pars.ndim != 2 or pars.shape[1] != P_:
                raise NmgpError("parameters must be [B, Nmax(1+T)+1 = %d], got %s" % (P_, pars.shape))
        elif pars.ndim != 2:
            raise NmgpError("parameters must be [B, Pmax], got %s" % (pars.shape,))
        hyper = as_f64(hyper)
        B, P_ = pars.shape
        out = np.empty((B, 5))
        grad = np.empty((B, P_)) if want_grad else None
        status = np.zeros(B, dtype=np.int32)
        self.check(self.lib.nmgp_had_subjects_eval(self.h, ptr(pars), B, int(chains_per_subject), ptr(hyper), int(bool(prior)),
                                                   ptr(out), ptr(grad), status.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return out, grad, status

    def _model_subjects_eval(self, fn, pars, hyper, prior, want_grad, chains_per_subject, width, plen, what):
        pars = as_f64(pars)
        if pars.ndim == 1:
            pars = pars[None]
        cohort = getattr(self, "_cohort", None)
        if pars.ndim != 2 or (cohort is not None and pars.shape[1] != plen(cohort[1], cohort[2] * (cohort[2] + 1) // 2)):
            raise NmgpError("parameters must be [B, %s%s], got %s"
                            % (what, "" if cohort is None else " = %d" % plen(cohort[1], cohort[2] * (cohort[2] + 1) // 2), pars.shape))
        hyper = as_f64(hyper)
        B, P_ = pars.shape
        out = np.empty((B, width))
        grad = np.empty((B, P_)) if want_grad else None
        status = np.zeros(B, dtype=np.int32)
        self.check(fn(self.h, ptr(pars), B, int(chains_per_subject), ptr(hyper), int(bool(prior)), ptr(out), ptr(grad),
                      status.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return out, grad, status

    def hads_subjects_eval(self, pars, hyper, prior=True, want_grad=False, chains_per_subject=1):
        """The cohort under the separable model: pars [B = S * chains_per_subject, Pmax = 2 Nmax + T + 1] in the padded layout
        (``hadamard_sep.cohort_pack``), hyper [9] as ``hads_batch_eval`` -> (out [B, 6], grad [B, Pmax] or None with +0.0 in the
        padded slots, status [B]).  Padded parameter slots are never read."""
        return self._model_subjects_eval(self.lib.nmgp_hads_subjects_eval, pars, hyper, prior, want_grad, chains_per_subject, 6,
                                         lambda N, T: 2 * N + T + 1, "2 Nmax + T + 1")

    def hadst_subjects_eval(self, pars, hyper, prior=True, want_grad=False, chains_per_subject=1):
        """The cohort under the stationary model: pars [B = S * chains_per_subject, T + 3] (no per-observation part, so no padded
        layout), hyper [5] as ``hadst_batch_eval`` -> (out [B, 5], grad [B, T + 3] or None, status [B])."""
        return self._model_subjects_eval(self.lib.nmgp_hadst_subjects_eval, pars, hyper, prior, want_grad, chains_per_subject, 5,
                                         lambda N, T: T + 3, "T + 3")

    # -- device-resident HMC trajectories of the cohort (one family for the three models) -----------
    # model name -> (NMGP_HAD_MODEL_*, entries of hyper, width of the tuple, length of a padded row and its name)
    _COHORT_TRAJ_MODELS = {
        "non": (0, 8, 5, lambda N, T: N * (1 + T) + 1, "Nmax(1+T)+1"),
        "sep": (1, 9, 6, lambda N, T: 2 * N + T + 1, "2 Nmax + T + 1"),
        "sta": (2, 5, 5, lambda N, T: T + 3, "T + 3"),
    }

    def _traj_rows(self, a, what):
        """[B, Pmax] of the begun trajectory; without one the C entry refuses the call (NMGP_E_STATE) before it reads anything"""
        a = as_f64(a)
        shape = getattr(self, "_cohort_traj", None)
        if a.ndim != 2 or (shape is not None and a.shape != shape):
            raise NmgpError("%s must be [B, Pmax]%s, got %s" % (what, "" if shape is None else " = [%d, %d]" % shape, a.shape))
        return a

    def had_subjects_traj_begin(self, model, pars, hyper, prior=True, chains_per_subject=1):
        """Starts the device-resident trajectories of the cohort at ``pars`` [B = S * chains_per_subject, Pmax] (the padded layout of
        the model's ``*_subjects_eval``; ``model`` is "non", "sep" or "sta") -> (out [B, W], status [B]) of that entry, bit for bit.
        Positions and gradients then stay on the device until ``had_subjects_traj_end``."""
        if model not in self._COHORT_TRAJ_MODELS:
            raise NmgpError("model must be one of 'non', 'sep', 'sta'; got %r" % (model,))
        code, nhyper, width, plen, what = self._COHORT_TRAJ_MODELS[model]
        pars = as_f64(pars)
        if pars.ndim == 1:
            pars = pars[None]
        cohort = getattr(self, "_cohort", None)
        if pars.ndim != 2 or (cohort is not None and pars.shape[1] != plen(cohort[1], cohort[2] * (cohort[2] + 1) // 2)):
            raise NmgpError("parameters must be [B, %s%s], got %s"
                            % (what, "" if cohort is None else " = %d" % plen(cohort[1], cohort[2] * (cohort[2] + 1) // 2), pars.shape))
        hyper = as_f64(hyper).reshape(-1)
        if hyper.shape[0] != nhyper:
            raise NmgpError("hyper must hold %d entries for model %r, got %d" % (nhyper, model, hyper.shape[0]))
        B = pars.shape[0]
        out = np.empty((B, width))
        status = np.zeros(B, dtype=np.int32)
        self._cohort_traj = None
        self.check(self.lib.nmgp_had_subjects_traj_begin(self.h, code, ptr(pars), B, int(chains_per_subject), ptr(hyper),
                                                         int(bool(prior)), ptr(out), status.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        self._cohort_traj = pars.shape
        return out, status

    def had_subjects_traj_set_mass(self, minv=None, prior=False):
        """None: identity; else diag(M^-1) per chain row [B, Pmax] in the padded layout (only the real slots are read; > 0 there).
        ``prior=True``: the prior-factor metric of the begun model and hyper-parameters (kind 2; not for the stationary model) --
        ``had_subjects_traj`` then takes and returns WHITENED momenta."""
        if prior:
            if minv is not None:
                raise NmgpError("prior=True takes no minv")
            self.check(self.lib.nmgp_had_subjects_traj_set_mass(self.h, 2, None))
            return
        if minv is None:
            self.check(self.lib.nmgp_had_subjects_traj_set_mass(self.h, 0, None))
            return
        minv = self._traj_rows(minv, "minv")
        self.check(self.lib.nmgp_had_subjects_traj_set_mass(self.h, 1, ptr(minv)))

    def had_subjects_traj(self, eps, nsteps, p0, want_p1=True, want_kin=False):
        """One leapfrog trajectory per chain from the resident state: step size ``eps[s]`` for the chains of subject s, momenta
        ``p0`` [B, Pmax] -> (q1 [B, Pmax], p1 [B, Pmax] or None, kin1 [B] or None, U1 [B] (inf for failed chains), failed [B] bool)."""
        p0 = self._traj_rows(p0, "momenta")
        B, P_ = p0.shape
        cohort = getattr(self, "_cohort", None)
        eps = as_f64(eps).reshape(-1)
        if cohort is not None and eps.shape[0] != cohort[0]:
            raise NmgpError("eps must hold one step size per subject (%d), got %d" % (cohort[0], eps.shape[0]))
        q1, U1 = np.empty((B, P_)), np.empty(B)
        p1 = np.empty((B, P_)) if want_p1 else None
        kin1 = np.empty(B) if want_kin else None
        failed = np.zeros(B, dtype=np.int32)
        self.check(self.lib.nmgp_had_subjects_traj(self.h, ptr(eps), int(nsteps), ptr(p0), ptr(q1), ptr(p1), ptr(kin1), ptr(U1),
                                                   failed.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return q1, p1, kin1, U1, failed.astype(bool)

    def had_subjects_prior_apply(self, model, hyper, v, trans=False, chains_per_subject=1):
        """``L_blk,s v`` (or ``L_blk,s^T v``) for the padded rows v [B = S * chains_per_subject, Pmax] of the set under ``model`` "non"
        or "sep": the block-diagonal of the set's cached GP-prior Cholesky factors of subject s (``nmgp_had_subjects_prior_apply``).
        Padded slots of v are never read; those of the result are +0.0."""
        if model not in self._COHORT_TRAJ_MODELS:
            raise NmgpError("model must be one of 'non', 'sep', 'sta'; got %r" % (model,))
        code, nhyper, _, plen, what = self._COHORT_TRAJ_MODELS[model]
        v = as_f64(v)
        if v.ndim == 1:
            v = v[None]
        cohort = getattr(self, "_cohort", None)
        if v.ndim != 2 or (cohort is not None and v.shape[1] != plen(cohort[1], cohort[2] * (cohort[2] + 1) // 2)):
            raise NmgpError("vectors must be [B, %s%s], got %s"
                            % (what, "" if cohort is None else " = %d" % plen(cohort[1], cohort[2] * (cohort[2] + 1) // 2), v.shape))
        hyper = as_f64(hyper).reshape(-1)
        if hyper.shape[0] != nhyper:
            raise NmgpError("hyper must hold %d entries for model %r, got %d" % (nhyper, model, hyper.shape[0]))
        out = np.empty_like(v)
        self.check(self.lib.nmgp_had_subjects_prior_apply(self.h, code, ptr(hyper), int(bool(trans)), ptr(v), int(v.shape[0]),
                                                          int(chains_per_subject), ptr(out)))
        return out

    def had_subjects_traj_commit(self, accept):
        acc = np.ascontiguousarray(np.asarray(accept).astype(np.int32))
        shape = getattr(self, "_cohort_traj", None)
        if acc.ndim != 1 or (shape is not None and acc.shape[0] != shape[0]):
            raise NmgpError("accept must be [B]%s, got %s" % ("" if shape is None else " = [%d]" % shape[0], acc.shape))
        self.check(self.lib.nmgp_had_subjects_traj_commit(self.h, acc.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))

    def had_subjects_traj_end(self):
        self.check(self.lib.nmgp_had_subjects_traj_end(self.h))
        self._cohort_traj = None

    # -- device-resident Adam of the cohort (one family for the three models, next to the trajectories) -----------
    def had_subjects_adam_begin(self, model, pars, hyper, prior=True, chains_per_subject=1):
        """Starts the device-resident optimiser of the cohort at ``pars`` [B = S * chains_per_subject, Pmax] (the padded layout of the
        model's ``*_subjects_eval``; ``model`` is "non", "sep" or "sta"): moments zero, every chain alive, t = 0; nothing is
        evaluated.  Parameters and moments then stay on the device until ``had_subjects_adam_end``."""
        if model not in self._COHORT_TRAJ_MODELS:
            raise NmgpError("model must be one of 'non', 'sep', 'sta'; got %r" % (model,))
        code, nhyper, width, plen, what = self._COHORT_TRAJ_MODELS[model]
        pars = as_f64(pars)
        if pars.ndim == 1:
            pars = pars[None]
        cohort = getattr(self, "_cohort", None)
        if pars.ndim != 2 or (cohort is not None and pars.shape[1] != plen(cohort[1], cohort[2] * (cohort[2] + 1) // 2)):
            raise NmgpError("parameters must be [B, %s%s], got %s"
                            % (what, "" if cohort is None else " = %d" % plen(cohort[1], cohort[2] * (cohort[2] + 1) // 2), pars.shape))
        hyper = as_f64(hyper).reshape(-1)
        if hyper.shape[0] != nhyper:
            raise NmgpError("hyper must hold %d entries for model %r, got %d" % (nhyper, model, hyper.shape[0]))
        # The recorded shape changes only when the library's state does.  A refusal (NMGP_E_SHAPE, NMGP_E_STATE, ...) leaves an
        # earlier run begun on the device, and its shape recorded here: the caller may go on with it.  A failure after the library
        # has dropped the earlier run (an allocation, the upload) leaves a shape nobody uses: the next call is refused before it writes.
        self.check(self.lib.nmgp_had_subjects_adam_begin(self.h, code, ptr(pars), pars.shape[0], int(chains_per_subject), ptr(hyper),
                                                         int(bool(prior))))
        self._cohort_adam = pars.shape + (width,)

    def had_subjects_adam(self, niters, lr, beta1=0.9, beta2=0.999, eps=1e-8):
        """``niters`` Adam iterations from the resident state with ONE synchronisation -> (out_hist [niters, B, W]: the verbose
        tuples at the parameters each iteration started from, NaN rows for chains that are no longer alive; alive [B] bool).  The
        iteration count behind the bias corrections persists across calls."""
        shape = getattr(self, "_cohort_adam", None)
        niters = int(niters)
        if shape is None:
            # no run known here: no buffer is handed over at all.  The entry checks the state first (NMGP_E_STATE), and were a run
            # begun behind this binding's back it would refuse the NULL pointers (NMGP_E_NULL) -- it cannot write either way
            hist = alive = ap = None
        else:
            # (niters < 1 is refused with NMGP_E_SHAPE before anything is written; the buffers are of the run's size all the same)
            hist, alive = np.empty((max(niters, 1), shape[0], shape[2])), np.zeros(shape[0], dtype=np.int32)
            ap = alive.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
        self.check(self.lib.nmgp_had_subjects_adam(self.h, niters, float(lr), float(beta1), float(beta2), float(eps), ptr(hist), ap))
        return hist, alive.astype(bool)

    def had_subjects_adam_get_pars(self):
        """The parameters [B, Pmax] as they stand on the device (padded slots as uploaded)."""
        shape = getattr(self, "_cohort_adam", None)
        pars = np.empty(shape[:2]) if shape is not None else None      # (no run known here: no buffer, as in had_subjects_adam)
        self.check(self.lib.nmgp_had_subjects_adam_get_pars(self.h, ptr(pars)))
        return pars

    def had_subjects_adam_end(self):
        self.check(self.lib.nmgp_had_subjects_adam_end(self.h))
        self._cohort_adam = None

    # the three cohort predictors as the binding sees them: C entry, entries of hyper (0: the entry takes no hyper, z or star and
    # returns no starred values), length of a parameter row and its name, starred values per draw and input and their name
    _COHORT_PREDICTORS = {
        "had": dict(entry="nmgp_predsample_had_subjects", nhyper=8, plen=lambda N, T: N * (1 + T) + 1, what="Nmax(1+T)+1",
                    width=lambda T: 1 + T, wname="1+T"),
        "sep": dict(entry="nmgp_predsample_hads_subjects", nhyper=9, plen=lambda N, T: 2 * N + T + 1, what="2 Nmax + T + 1",
                    width=lambda T: 2, wname="2"),
        "sta": dict(entry="nmgp_predict_hadst_subjects", nhyper=0, plen=lambda N, T: T + 3, what="T + 3", width=None, wname=None),
    }

    def _predict_subjects(self, model, pars, xs, hyper=None, indx_star=None, nstar=None, draws_per_subject=1, z=None, star=None):
        """The three cohort predictors' binding: shape checks against the set's (S, Nmax, M), the padded output arrays, the call."""
        d = self._COHORT_PREDICTORS[model]
        fn = getattr(self.lib, d["entry"])
        cohort = getattr(self, "_cohort", None)
        pars = as_f64(pars)
        if pars.ndim == 1:
            pars = pars[None]
        xs = as_f64(xs)
        if d["nhyper"]:
            hyper = as_f64(hyper).reshape(-1)
            if hyper.shape[0] != d["nhyper"]:
                raise NmgpError("hyper must have %d entries, got %d" % (d["nhyper"], hyper.shape[0]))
        H = int(draws_per_subject)
        if pars.ndim != 2 or xs.ndim != 2 or xs.shape[1] < 1 or H < 1:
            raise NmgpError("pars must be [B, Pmax], xs [S, Smax >= 1] and draws_per_subject >= 1; got %s, %s, %d"
                            % (pars.shape, xs.shape, H))
        S, Smax = xs.shape
        B = pars.shape[0]
        if cohort is not None:
            M = cohort[2]
            T = M * (M + 1) // 2
            P_ = d["plen"](cohort[1], T)
            if S != cohort[0] or B != S * H or pars.shape[1] != P_:
                raise NmgpError("pars must be [S * draws_per_subject = %d, %s = %d] and xs [S = %d, Smax]; got %s, %s"
                                % (cohort[0] * H, d["what"], P_, cohort[0], pars.shape, xs.shape))
        else:                            # (no set: the entry refuses the call; the shapes only have to be self-consistent)
            M, T = 1, None
        ipt = ctypes.POINTER(ctypes.c_int)
        ia = na = None
        if indx_star is not None:
            if hasattr(indx_star, "detach"):
                indx_star = indx_star.detach().cpu().numpy()
            ia = np.ascontiguousarray(np.asarray(indx_star), dtype=np.int32)
            if ia.shape != (S, Smax):
                raise NmgpError("indx_star must be [S=%d, Smax=%d], got %s" % (S, Smax, ia.shape))
        if nstar is not None:
            na = np.ascontiguousarray(np.asarray(nstar).reshape(-1), dtype=np.int32)
            if na.shape[0] != S:
                raise NmgpError("nstar must have one entry per subject (S=%d), got %d" % (S, na.shape[0]))
        shape = (B, Smax, M) if ia is None else (B, Smax)
        mean, var = np.empty(shape), np.empty(shape)
        status = np.zeros(B, dtype=np.int32)
        ii, ni = (None if a is None else a.ctypes.data_as(ipt) for a in (ia, na))
        if not d["nhyper"]:
            self.check(fn(self.h, ptr(pars), B, H, ptr(xs), ii, ni, Smax, ptr(mean), ptr(var), status.ctypes.data_as(ipt)))
            return mean, var, status
        if z is not None and star is not None:
            raise NmgpError("star= replaces the regression: z must be None")
        za, sa = (None if a is None else as_f64(a) for a in (z, star))
        W = None if T is None else d["width"](T)
        for name, a in (("z", za), ("star", sa)):
            if a is not None and (a.ndim != 3 or a.shape[:2] != (B, Smax) or (W is not None and a.shape[2] != W)):
                raise NmgpError("%s must be [B=%d, Smax=%d, %s], got %s" % (name, B, Smax, d["wname"], a.shape))
        if W is None:
            W = next((a.shape[2] for a in (za, sa) if a is not None), 2)
        star_out = np.empty((B, Smax, W))
        self.check(fn(self.h, ptr(pars), B, H, ptr(hyper), ptr(xs), ii, ni, Smax, ptr(za), ptr(sa), ptr(mean), ptr(var), ptr(star_out),
                      status.ctypes.data_as(ipt)))
        return mean, var, star_out, status

    def predsample_had_subjects(self, pars, hyper, xs, indx_star=None, nstar=None, draws_per_subject=1, z=None, star=None):
        """MAP and posterior-draw prediction for the cohort (``nmgp_predsample_had_subjects``), padded arrays as the C entry takes
        them: pars [B = S * draws_per_subject, Pmax] (row s * draws_per_subject + h = draw h of subject s), xs [S, Smax] of which
        the first nstar[s] entries of row s are read (nstar=None: all Smax), indx_star [S, Smax] or None (all M outputs per input),
        z / star [B, Smax, 1+T] as ``predsample_had``.  Returns (mean, var [B, Smax(, M)], star [B, Smax, 1+T], status [B]); padded
        new-input slots hold +0.0, a draw with non-zero status has NaN in its real slots.  ``hadamard.cohort_predict`` is the ragged
        form."""
        return self._predict_subjects("had", pars, xs, hyper=hyper, indx_star=indx_star, nstar=nstar,
                                      draws_per_subject=draws_per_subject, z=z, star=star)

    def predsample_hads_subjects(self, pars, hyper, xs, indx_star=None, nstar=None, draws_per_subject=1, z=None, star=None):
        """The cohort predictor under the separable model (``nmgp_predsample_hads_subjects``): pars [B, 2 Nmax + T + 1] in the padded
        layout of ``hads_subjects_eval`` (``hadamard_sep.cohort_pack``), hyper [9], z / star [B, Smax, 2] (tilde_l*, tilde_sigma*
        before exp) as ``predsample_hads``; everything else as ``predsample_had_subjects``.  Returns (mean, var [B, Smax(, M)],
        star [B, Smax, 2], status [B]).  ``hadamard_sep.cohort_predict`` is the ragged form."""
        return self._predict_subjects("sep", pars, xs, hyper=hyper, indx_star=indx_star, nstar=nstar,
                                      draws_per_subject=draws_per_subject, z=z, star=star)

    def predict_hadst_subjects(self, pars, xs, indx_star=None, nstar=None, draws_per_subject=1):
        """The cohort predictor under the stationary model (``nmgp_predict_hadst_subjects``): pars [B, T + 3] (draws_per_subject = 1:
        the MAP predictor; more: posterior draws), no hyper, z or starred values; xs, indx_star, nstar as
        ``predsample_had_subjects``.  Returns (mean, var [B, Smax(, M)], status [B]).  ``hadamard_sta.cohort_predict`` is the ragged
        form."""
        return self._predict_subjects("sta", pars, xs, indx_star=indx_star, nstar=nstar, draws_per_subject=draws_per_subject)

    def predict_had(self, pars, hyper, xs):
        """(mean [S, M], var [S, M], star [S, 1+T]) of the resident Hadamard subject at the new inputs xs."""
        pars, hyper, xs = as_f64(pars).reshape(-1), as_f64(hyper), as_f64(xs).reshape(-1)
        if pars.shape[0] != self.N * (1 + self.T) + 1:
            raise NmgpError("bad parameter vector length %d" % pars.shape[0])
        S = xs.shape[0]
        mean, var, star = np.empty((S, self.M)), np.empty((S, self.M)), np.empty((S, 1 + self.T))
        self.check(self.lib.nmgp_predict_had(self.h, ptr(pars), ptr(hyper), ptr(xs), S, ptr(mean), ptr(var), ptr(star)))
        return mean, var, star

    def predsample_had(self, pars_hist, hyper, xs, indx_star=None, z=None, star=None):
        """Posterior-draw and held-out prediction of the nonseparable HADAMARD model: pars_hist [H, N(1+T)+1] of the resident
        Hadamard subject at the new inputs xs [S].  indx_star=None: all M outputs at every input, moments [H, S, M]; indx_star [S]:
        output indx_star[s] only at xs[s] (held-out pairs), moments [H, S].  z [H, S, 1+T]: standard normals of the latent regression
        of (tilde_l*, the T raw slots of L*) (None: the conditional means); star [H, S, 1+T]: starred values to use instead of
        regressing (z must then be None).  Returns (mean, var, star [H, S, 1+T], status [H]); a draw with non-zero status has NaN
        rows."""
        pars = as_f64(pars_hist)
        if pars.ndim == 1:
            pars = pars[None]
        P_, W = self.N * (1 + self.T) + 1, 1 + self.T
        if pars.ndim != 2 or pars.shape[1] != P_:
            raise NmgpError("draws must be [H, N(1+T)+1 = %d], got %s" % (P_, pars.shape))
        hyper, xs = as_f64(hyper).reshape(-1), as_f64(xs).reshape(-1)
        if hyper.shape[0] != 8:
            raise NmgpError("hyper must have 8 entries, got %d" % hyper.shape[0])
        H, S = pars.shape[0], xs.shape[0]
        ia = None
        if indx_star is not None:
            if hasattr(indx_star, "detach"):
                indx_star = indx_star.detach().cpu().numpy()
            ia = np.ascontiguousarray(np.asarray(indx_star).reshape(-1).astype(np.int32))
            if ia.shape[0] != S:
                raise NmgpError("indx_star must have one label per new input (S=%d), got %d" % (S, ia.shape[0]))
        if z is not None and star is not None:
            raise NmgpError("star= replaces the regression: z must be None")
        za = sa = None
        for name, a in (("z", z), ("star", star)):
            if a is not None:
                a = as_f64(a)
                if a.shape != (H, S, W):
                    raise NmgpError("%s must be [H=%d, S=%d, 1+T=%d], got %s" % (name, H, S, W, a.shape))
                if name == "z":
                    za = a
                else:
                    sa = a
        shape = (H, S, self.M) if ia is None else (H, S)
        mean, var = np.empty(shape), np.empty(shape)
        star_out = np.empty((H, S, W))
        status = np.zeros(H, dtype=np.int32)
        ip = None if ia is None else ia.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
        self.check(self.lib.nmgp_predsample_had(self.h, ptr(pars), H, ptr(hyper), ptr(xs), ip, S, ptr(za), ptr(sa), ptr(mean),
                                                ptr(var), ptr(star_out), status.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return mean, var, star_out, status

    # -- Hadamard form of the separable model (the resident subject is had_set_data's) -------------
    def _hads_len(self):
        return 2 * self.N + self.T + 1

    def hads_batch_eval(self, pars, hyper, prior=True, want_grad=False):
        """B parameter vectors [tilde_l | tilde_sigma | L_vec | tilde_sigma2_err] of the resident Hadamard subject in one launch
        sequence: pars [B, 2N+T+1] (or one vector), hyper [9] -> (out [B, 6], grad [B, P] or None, status [B]: 0, a leading-minor
        index or NUM_NAN; a failing chain has a NaN row and a zero gradient row)."""
        return self._had_eval(self.lib.nmgp_hads_batch_eval, pars, self._hads_len(), 6, hyper, 9, "2N+T+1", prior, want_grad)

    def hads_covariance(self, pars):
        return self._had_cov(self.lib.nmgp_hads_covariance, pars, self._hads_len(), " (2N+T+1 = %d)" % self._hads_len())

    def predict_hads(self, pars, hyper, xs):
        """(mean [S, M], var [S, M], star [S, 2] = tilde_l*, tilde_sigma*) of the resident Hadamard subject at the new inputs xs."""
        pars, hyper, xs = as_f64(pars).reshape(-1), as_f64(hyper).reshape(-1), as_f64(xs).reshape(-1)
        if pars.shape[0] != self._hads_len():
            raise NmgpError("bad parameter vector length %d (2N+T+1 = %d)" % (pars.shape[0], self._hads_len()))
        if hyper.shape[0] != 9:
            raise NmgpError("hyper must have 9 entries, got %d" % hyper.shape[0])
        S = xs.shape[0]
        mean, var, star = np.empty((S, self.M)), np.empty((S, self.M)), np.empty((S, 2))
        self.check(self.lib.nmgp_predict_hads(self.h, ptr(pars), ptr(hyper), ptr(xs), S, ptr(mean), ptr(var), ptr(star)))
        return mean, var, star

    def predsample_hads(self, pars_hist, hyper, xs, indx_star=None, z=None, star=None):
        """Posterior-draw prediction of the separable HADAMARD model: pars_hist [H, 2N+T+1] of the resident Hadamard subject at the
        new inputs xs [S].  indx_star=None: all M outputs at every input, moments [H, S, M]; indx_star [S]: output indx_star[s] only
        at xs[s] (the reference's indexed family), moments [H, S].  z [H, S, 2]: standard normals of the latent regression of
        (tilde_l*, tilde_sigma*) (None: the conditional means); star [H, S, 2]: starred values to use instead of regressing (z must
        then be None).  Returns (mean, var, star [H, S, 2], status [H]); a draw with non-zero status has NaN rows."""
        pars = as_f64(pars_hist)
        if pars.ndim == 1:
            pars = pars[None]
        P_ = self._hads_len()
        if pars.ndim != 2 or pars.shape[1] != P_:
            raise NmgpError("draws must be [H, 2N+T+1 = %d], got %s" % (P_, pars.shape))
        hyper, xs = as_f64(hyper).reshape(-1), as_f64(xs).reshape(-1)
        if hyper.shape[0] != 9:
            raise NmgpError("hyper must have 9 entries, got %d" % hyper.shape[0])
        H, S = pars.shape[0], xs.shape[0]
        ia = None
        if indx_star is not None:
            if hasattr(indx_star, "detach"):
                indx_star = indx_star.detach().cpu().numpy()
            ia = np.ascontiguousarray(np.asarray(indx_star).reshape(-1).astype(np.int32))
            if ia.shape[0] != S:
                raise NmgpError("indx_star must have one label per new input (S=%d), got %d" % (S, ia.shape[0]))
        if z is not None and star is not None:
            raise NmgpError("star= replaces the regression: z must be None")
        za = sa = None
        for name, a in (("z", z), ("star", star)):
            if a is not None:
                a = as_f64(a)
                if a.shape != (H, S, 2):
                    raise NmgpError("%s must be [H=%d, S=%d, 2], got %s" % (name, H, S, a.shape))
                if name == "z":
                    za = a
                else:
                    sa = a
        shape = (H, S, self.M) if ia is None else (H, S)
        mean, var = np.empty(shape), np.empty(shape)
        star_out = np.empty((H, S, 2))
        status = np.zeros(H, dtype=np.int32)
        ip = None if ia is None else ia.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
        self.check(self.lib.nmgp_predsample_hads(self.h, ptr(pars), H, ptr(hyper), ptr(xs), ip, S, ptr(za), ptr(sa), ptr(mean),
                                                 ptr(var), ptr(star_out), status.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return mean, var, star_out, status

    # -- Hadamard form of the stationary model (the resident subject is had_set_data's) -------------
    def hadst_batch_eval(self, pars, hyper, prior=True, want_grad=False):
        """B parameter vectors [tilde_l, tilde_sigma, L_vec, tilde_sigma2_err] of the resident Hadamard subject in one launch
        sequence: pars [B, T+3] (or one vector), hyper [5] = (mu_tilde_l, sigma_tilde_l, a, b, c) -> (out [B, 5], grad [B, T+3] or
        None, status [B]: 0, a leading-minor index or NUM_NAN; a failing chain has a NaN row and a zero gradient row)."""
        return self._had_eval(self.lib.nmgp_hadst_batch_eval, pars, self.T + 3, 5, hyper, 5, "T+3", prior, want_grad)

    def hadst_covariance(self, pars):
        return self._had_cov(self.lib.nmgp_hadst_covariance, pars, self.T + 3, " (T+3 = %d)" % (self.T + 3))

    def predict_hadst(self, pars, xs, indx_star=None):
        """Prediction of the stationary HADAMARD model at the new inputs xs [S] under the parameter vectors pars [H, T+3] (one
        vector: the MAP predictor with H = 1; a chain of posterior draws otherwise).  indx_star=None: all M outputs at every input,
        moments [H, S, M]; indx_star [S]: output indx_star[s] only at xs[s], moments [H, S].  Returns (mean, var, status [H]); a draw
        with non-zero status has NaN rows."""
        pars = as_f64(pars)
        if pars.ndim == 1:
            pars = pars[None]
        if pars.ndim != 2 or pars.shape[1] != self.T + 3:
            raise NmgpError("parameters must be [H, T+3 = %d], got %s" % (self.T + 3, pars.shape))
        xs = as_f64(xs).reshape(-1)
        H, S = pars.shape[0], xs.shape[0]
        ia = None
        if indx_star is not None:
            if hasattr(indx_star, "detach"):
                indx_star = indx_star.detach().cpu().numpy()
            ia = np.ascontiguousarray(np.asarray(indx_star).reshape(-1).astype(np.int32))
            if ia.shape[0] != S:
                raise NmgpError("indx_star must have one label per new input (S=%d), got %d" % (S, ia.shape[0]))
        shape = (H, S, self.M) if ia is None else (H, S)
        mean, var = np.empty(shape), np.empty(shape)
        status = np.zeros(H, dtype=np.int32)
        ip = None if ia is None else ia.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
        self.check(self.lib.nmgp_predict_hadst(self.h, ptr(pars), H, ptr(xs), ip, S, ptr(mean), ptr(var),
                                               status.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return mean, var, status

    # -- measurement ----------------------------------------------------------------------------
    def profile_enable(self, on=True):
        self.check(self.lib.nmgp_profile_enable(self.h, int(on)))   # True/1 stage timers, 2 + per-launch SYRK timers

    def profile_reset(self):
        self.check(self.lib.nmgp_profile_reset(self.h))

    def profile_read(self):
        ms = np.zeros(len(STAGES))
        cnt = np.zeros(len(STAGES), dtype=np.int64)
        self.check(self.lib.nmgp_profile_read(self.h, ptr(ms), cnt.ctypes.data_as(c_ll_p)))
        return {s: (float(ms[k]), int(cnt[k])) for k, s in enumerate(STAGES)}

    def profile_read_work(self):
        """{stage: (ms, launches, algorithmic flop, algorithmic bytes)}; tracked for "syrk", 0 elsewhere."""
        ms = np.zeros(len(STAGES))
        cnt = np.zeros(len(STAGES), dtype=np.int64)
        work = np.zeros(len(STAGES))
        nbytes = np.zeros(len(STAGES))
        self.check(self.lib.nmgp_profile_read_work(self.h, ptr(ms), cnt.ctypes.data_as(c_ll_p), ptr(work), ptr(nbytes)))
        return {s: (float(ms[k]), int(cnt[k]), float(work[k]), float(nbytes[k])) for k, s in enumerate(STAGES)}

    def last_sep_attempts(self):
        """Jitter retries the last separable / stationary evaluation needed (0: the exact covariance was evaluated)."""
        return int(self.lib.nmgp_last_sep_attempts(self.h))

    def measure_hbm_gbs(self, nbytes=1 << 30, reps=10):
        out = np.empty(1)
        self.check(self.lib.nmgp_measure_hbm_gbs(self.h, int(nbytes), int(reps), ptr(out)))
        return float(out[0])

    def measure_hbm_rates(self, nbytes=1 << 30, reps=10):
        """{copy, read, write} GB/s of the library's flat streaming kernels (the HBM ceilings as measured in this run)."""
        out = np.empty(3)
        self.check(self.lib.nmgp_measure_hbm_rates(self.h, int(nbytes), int(reps), ptr(out)))
        return {"copy": float(out[0]), "read": float(out[1]), "write": float(out[2])}

    def measure_dgemm_tflops(self, n=4096, reps=5):
        out = np.empty(1)
        self.check(self.lib.nmgp_measure_dgemm_tflops(self.h, int(n), int(reps), ptr(out)))
        return float(out[0])


def default_device():
    """GPU ordinal for this process: NMGP_DEVICE, else LOCAL_RANK (one process per GPU), else 0."""
    for k in ("NMGP_DEVICE", "LOCAL_RANK"):
        v = os.environ.get(k)
        if v is not None and v != "":
            return int(v)
    return 0


_default_ctx = {}


def default_context(device=None):
    """Process-wide context used by the `Utility` mirror (created on first use)."""
    if device is None:
        device = default_device()
    ctx = _default_ctx.get(device)
    if ctx is None:
        ctx = Context(device)
        _default_ctx[device] = ctx
    return ctx
