"""Hadamard form of the stationary model (the LMC baseline) behind the reference's signatures: irregularly observed outputs.

The data are N single observations ``(x[i], indx[i], y[i])`` as in ``hadamard.py``.  The model has ONE ``B_f = L L^T`` and a
stationary RBF kernel: ``pars = [tilde_l, tilde_sigma, L_vec (T), tilde_sigma2_err]``, P = T+3 (``vec2pars_S``), no GP prior.
Served here:

* ``nlogpos_obj_hadamard_S`` / ``logpos_hadamard_S`` (reference ``Utility/logpos.py:662-716``): value and gradient from one device
  evaluation (``nmgp_hadst_batch_eval``), attached to autograd through one ``torch.autograd.Function``;
* ``point_predmap_S_hadamard`` / ``pointwise_predmap_S_hadamard`` (``Utility/prediction.py:1695-1740``): all grid points from one
  device call (``nmgp_predict_hadst``);
* ``indexed_predict`` (this package's own name): mean and std of ONE labelled output per held-out input.

Quirks of the reference that are kept:

* the verbose tuple has FIVE entries (NegLog, loglik, lp_tilde_l, lp_L_vec, lp_sigma2_err), and the three prior entries are
  reported whether or not ``Prior`` adds them;
* ``tilde_sigma`` has NO prior;
* ``Normal(mu_tilde_l, sigma_tilde_l)`` and ``Normal(0, c)`` round their Python-number arguments to float32, as torch does;
* ``L_vec`` enters ``vec2lowtriangle`` as it is (no exp on the diagonal slots);
* the inverse gamma on sigma2_err is the UNNORMALISED one (``inverse_gamma_logpdf_u``);
* the jitter of ``RBF_cov`` is multiplied by ``B_f[c_i, c_i]``, and the prior term of the predictive variance is
  ``B_f[m, m] (sigma^2 + 1e-6)`` while the cross-covariance carries no jitter.

Not served, on purpose: ``indexedpoint_predmap_S_hadamard`` / ``test_predmap_S_hadamard``.  Their variance is ``(A - B)[0, 0]``
with ``A = B_f kron k(x*, x*)``: output 0's prior variance for EVERY ``indx_star`` (the mean is right).  They keep resolving to
the user's checkout even with the switch set; ``indexed_predict`` computes the same mean and the variance with ``B_f[c*, c*]``.

``M`` is inferred from ``indx`` as the reference does (the number of distinct labels), so the labels must be 0 .. M-1 and each
must occur.  The reference forms S^-1 through ``inverse`` + ``logdet`` (objective) and ``symeig`` + a Cholesky of the dense
inverse per grid point (predictor); here it is the blocked Cholesky with riding rows, once for all grid points.

The names are opt-in behind the reference's module names: with ``NMGP_HADAMARD_STA=1`` in the environment ``Utility.logpos`` /
``Utility.prediction`` serve them; otherwise they keep resolving to the user's checkout (``NMGP_HADAMARD=1`` and
``NMGP_HADAMARD_SEP=1`` do not serve them).  Importing this module directly always works.
"""
import os

import numpy as np
import torch

from . import _lib
from .hadamard import _as_tensor, _bands, _cohort_predict, _f, _labels, _np, _objective

LOGPOS_NAMES = ("nlogpos_obj_hadamard_S", "logpos_hadamard_S")
PREDICTION_NAMES = ("point_predmap_S_hadamard", "pointwise_predmap_S_hadamard")


def enabled():
    """NMGP_HADAMARD_STA=1: ``Utility.logpos`` / ``Utility.prediction`` serve the names of this module."""
    return os.environ.get("NMGP_HADAMARD_STA", "") not in ("", "0")


_HadamardStaObjective = _objective(
    __name__, "_HadamardStaObjective", "hadst_batch_eval", "nlogpos_obj_hadamard_S",
    "Stationary model: forward(flags, hyper, x, indx, y, tilde_l, tilde_sigma, L_vec, tilde_sigma2_err) -> (res, loglik, "
    "lp_tilde_l, lp_L_vec, lp_sigma2_err).")


def nlogpos_obj_hadamard_S(pars, x, indx, y, mu_tilde_l, sigma_tilde_l, a=1, b=1, c=10, verbose=False, Prior=True):
    """Negative log posterior of the stationary Hadamard model on the flat parameter vector [tilde_l, tilde_sigma, L_vec,
    tilde_sigma2_err]; verbose=True returns the five-entry tuple (NegLog, loglik, lp_tilde_l, lp_L_vec, lp_sigma2_err).
    reference logpos.py:662-673."""
    M = torch.unique(indx).size(0)
    T = int(M * (M + 1) / 2)
    tilde_l, tilde_sigma, L_vec, tilde_sigma2_err = pars[0], pars[1], pars[2: 2 + T], pars[-1]
    if verbose:
        res, loglik, lp_l, lp_L, lp_s2 = logpos_hadamard_S(tilde_l, tilde_sigma, L_vec, tilde_sigma2_err, x, indx, y, mu_tilde_l,
                                                           sigma_tilde_l, a, b, c, verbose, Prior)
        return -res, loglik, lp_l, lp_L, lp_s2
    return -logpos_hadamard_S(tilde_l, tilde_sigma, L_vec, tilde_sigma2_err, x, indx, y, mu_tilde_l, sigma_tilde_l, a, b, c, verbose,
                              Prior)


def logpos_hadamard_S(tilde_l, tilde_sigma, L_vec, tilde_sigma2_err, x, indx, y, mu_tilde_l, sigma_tilde_l, a, b, c, verbose=False,
                      Prior=True):
    """Log joint posterior of the stationary Hadamard model; reference logpos.py:676-716.  One device evaluation: covariance
    K_x o B_f[indx, indx] + sigma2_err I of the N observations, blocked Cholesky, and -- when a parameter requires grad -- the
    analytic adjoint reduced to the T + 3 parameters on the device."""
    hyper = [_f(mu_tilde_l), _f(sigma_tilde_l), _f(a), _f(b), _f(c)]
    res = _HadamardStaObjective.apply((bool(Prior), torch.is_grad_enabled()), hyper, x, indx, y, _as_tensor(tilde_l),
                                      _as_tensor(tilde_sigma), _as_tensor(L_vec), _as_tensor(tilde_sigma2_err))
    return res if verbose else res[0]


def _moments(tilde_l, tilde_sigma, L_vec, tilde_sigma2_err, x, indx, y, xs, indx_star=None):
    c = _lib.default_context()
    c.had_set_data(_np(x).reshape(-1), _labels(indx), _np(y).reshape(-1))
    pars = np.concatenate([_np(tilde_l).reshape(-1), _np(tilde_sigma).reshape(-1), _np(L_vec).reshape(-1),
                           _np(tilde_sigma2_err).reshape(-1)])
    mean, var, status = c.predict_hadst(pars, _np(xs).reshape(-1), None if indx_star is None else _labels(indx_star))
    if status[0] != 0:
        # torch.cholesky raises on a covariance that is not positive definite (reference prediction.py:1717)
        raise RuntimeError("predmap_S_hadamard: the covariance is not positive definite or not finite (status %d)" % int(status[0]))
    return mean[0], var[0]


def _predict(tilde_l, tilde_sigma, L_vec, tilde_sigma2_err, x, indx, y, xs):
    return _bands(*_moments(tilde_l, tilde_sigma, L_vec, tilde_sigma2_err, x, indx, y, xs))


def point_predmap_S_hadamard(tilde_l, tilde_sigma, L_vec, tilde_sigma2_err, x, indx, y, x_star, *args, **kwargs):
    """[mu - 1.96 s, mu, mu + 1.96 s] of all M outputs at x_star ([3, M]); reference prediction.py:1695-1728."""
    return _predict(tilde_l, tilde_sigma, L_vec, tilde_sigma2_err, x, indx, y, x_star)[0]


def pointwise_predmap_S_hadamard(tilde_l, tilde_sigma, L_vec, tilde_sigma2_err, x, indx, y, grids, *args, **kwargs):
    """All grid points from one device call ([G, 3, M]); reference prediction.py:1730-1740."""
    return _predict(tilde_l, tilde_sigma, L_vec, tilde_sigma2_err, x, indx, y, grids)


def indexed_predict(tilde_l, tilde_sigma, L_vec, tilde_sigma2_err, x, indx, y, x_test, indx_test):
    """(mean [S], std [S]) of output ``indx_test[s]`` at ``x_test[s]``, the variance with ``B_f[c*, c*]``.  The reference's
    ``test_predmap_S_hadamard`` (prediction.py:1742-1792) returns the same mean, and this std at the label-0 points only (see the
    module docstring)."""
    mean, var = _moments(tilde_l, tilde_sigma, L_vec, tilde_sigma2_err, x, indx, y, x_test, indx_test)
    return (torch.from_numpy(np.ascontiguousarray(mean)).type(torch.DoubleTensor),
            torch.from_numpy(np.sqrt(var)).type(torch.DoubleTensor))


def cohort_predict(ctx, draws, xs, indx_star=None):
    """Prediction under the stationary model for the cohort ``ctx`` holds (``Context.had_set_subjects``), in ONE device call
    (``nmgp_predict_hadst_subjects``): ``draws[s]`` ``[H, T + 3]`` (or ``[T + 3]``: the MAP predictor; the same H for every subject),
    ``xs[s]`` ``[S_s]``, ``indx_star[s]`` ``[S_s]`` labels or None (all M outputs per input).  The model has no latent curve: no
    hyper, no normals, no starred values.  Returns per-subject ``(mean [H, S_s(, M)], var, status [H])``."""
    def rows_of(vs, H, Nmax, M, T):
        for s, v in enumerate(vs):
            if v.shape != (H, T + 3):
                raise _lib.NmgpError("hadamard_sta.cohort_predict: draws[%d] %s is not [H = %d, T + 3 = %d]" % (s, v.shape, H, T + 3))
        return np.concatenate(vs, axis=0)

    return _cohort_predict(ctx, "hadamard_sta.cohort_predict", lambda pars, x2, i2, nstar, H, z2, s2: ctx.predict_hadst_subjects(
        pars, x2, indx_star=i2, nstar=nstar, draws_per_subject=H), draws, xs, indx_star, None, None, rows_of, lambda T: 0)
