"""Hadamard form of the separable model behind the reference's signatures: irregularly observed outputs, one cross-output matrix.

The data are N single observations ``(x[i], indx[i], y[i])`` as in ``hadamard.py``.  Where that module's model gives every
observation its own lower triangle (P = N(1+T)+1), this one has ONE ``B_f = L L^T`` shared by all locations and a nonstationary
amplitude ``tilde_sigma``: ``pars = [tilde_l (N) | tilde_sigma (N) | L_vec (T) | tilde_sigma2_err]``, P = 2N+T+1.  Served here:

* ``nlogpos_obj_hadamard`` / ``logpos_hadamard`` (reference ``Utility/logpos.py:465-563``): value and gradient from one device
  evaluation (``nmgp_hads_batch_eval``), attached to autograd through one ``torch.autograd.Function``;
* ``point_predmap_hadamard`` / ``pointwise_predmap_hadmard`` (``Utility/prediction.py:710-808``; the second name is the
  reference's spelling, ``pointwise_predmap_hadamard`` is offered as an alias): all grid points from one device call
  (``nmgp_predict_hads``), nothing printed per grid point.

Quirks of the reference that are kept:

* the verbose tuple has SIX entries (NegLog, loglik, lp_tilde_l, lp_tilde_sigma, lp_L_vec, lp_sigma2_err);
* ``L_vec`` enters ``vec2lowtriangle`` as it is (no exp on the diagonal slots) and carries ``Normal(0, c)`` on every raw slot, with
  ``c`` rounded to float32 as torch does for a Python number;
* the inverse gamma on sigma2 is the UNNORMALISED one (``inverse_gamma_logpdf_u``);
* the prior term of the predictive variance is ``B_f[m, m] (sigma*^2 + 1e-6)``: the jitter of ``Nonstationary_RBF_cov`` sits inside
  it, while the cross-covariance carries none.

``M`` is inferred from ``indx`` as the reference does (the number of distinct labels), so the labels must be 0 .. M-1 and each
must occur.  The reference forms S^-1 of the predictor through ``symeig``; here it is the blocked Cholesky with riding rows.

The stationary ``*_hadamard_S`` names live in ``hadamard_sta.py`` behind ``NMGP_HADAMARD_STA=1``.
``indexedpoint_predmap_hadamard`` / ``test_predmap_hadamard`` and the ``predsample_hadamard`` families live in
``predsample_hadamard.py`` behind a switch of their own.

The names are opt-in behind the reference's module names: with ``NMGP_HADAMARD_SEP=1`` in the environment ``Utility.logpos`` /
``Utility.prediction`` serve them; otherwise they keep resolving to the user's checkout (``NMGP_HADAMARD=1`` alone does not serve
them).  Importing this module directly always works.
"""
import os

import numpy as np
import torch

from . import _lib
from .hadamard import _as_tensor, _bands, _cohort_predict, _f, _labels, _np, _objective

LOGPOS_NAMES = ("nlogpos_obj_hadamard", "logpos_hadamard")
PREDICTION_NAMES = ("point_predmap_hadamard", "pointwise_predmap_hadmard", "pointwise_predmap_hadamard")


def enabled():
    """NMGP_HADAMARD_SEP=1: ``Utility.logpos`` / ``Utility.prediction`` serve the names of this module."""
    return os.environ.get("NMGP_HADAMARD_SEP", "") not in ("", "0")


_HadamardSepObjective = _objective(
    __name__, "_HadamardSepObjective", "hads_batch_eval", "nlogpos_obj_hadamard",
    "Separable model: forward(flags, hyper, x, indx, y, tilde_l, tilde_sigma, L_vec, tilde_sigma2_err) -> (res, loglik, "
    "lp_tilde_l, lp_tilde_sigma, lp_L_vec, lp_sigma2_err).")


def nlogpos_obj_hadamard(pars, x, indx, y, mu_tilde_l=0., alpha_tilde_l=1., beta_tilde_l=1., mu_tilde_sigma=0., alpha_tilde_sigma=1.,
                         beta_tilde_sigma=1., a=1, b=1, c=10, verbose=False, Prior=True):
    """Negative log posterior of the separable Hadamard model on the flat parameter vector [tilde_l | tilde_sigma | L_vec |
    tilde_sigma2_err]; verbose=True returns the six-entry tuple (NegLog, loglik, lp_tilde_l, lp_tilde_sigma, lp_L_vec,
    lp_sigma2_err).  reference logpos.py:465-499."""
    N = y.size(0)
    M = torch.unique(indx).size(0)
    T = int(M * (M + 1) / 2)
    tilde_l, tilde_sigma, L_vec, tilde_sigma2_err = pars[:N], pars[N: 2 * N], pars[2 * N: 2 * N + T], pars[-1]
    if verbose:
        res, loglik, lp_l, lp_s, lp_L, lp_s2 = logpos_hadamard(tilde_l, tilde_sigma, L_vec, tilde_sigma2_err, x, indx, y, mu_tilde_l,
                                                               alpha_tilde_l, beta_tilde_l, mu_tilde_sigma, alpha_tilde_sigma,
                                                               beta_tilde_sigma, a, b, c, verbose, Prior)
        return -res, loglik, lp_l, lp_s, lp_L, lp_s2
    return -logpos_hadamard(tilde_l, tilde_sigma, L_vec, tilde_sigma2_err, x, indx, y, mu_tilde_l, alpha_tilde_l, beta_tilde_l,
                            mu_tilde_sigma, alpha_tilde_sigma, beta_tilde_sigma, a, b, c, verbose, Prior)


def logpos_hadamard(tilde_l, tilde_sigma, L_vec, tilde_sigma2_err, x, indx, y, mu_tilde_l, alpha_tilde_l, beta_tilde_l,
                    mu_tilde_sigma, alpha_tilde_sigma, beta_tilde_sigma, a, b, c, verbose=False, Prior=True):
    """Log joint posterior of the separable Hadamard model; reference logpos.py:502-563.  One device evaluation: covariance
    K_x o (R R^T) + sigma2 I of the N observations (R[i] = row indx[i] of the shared L), blocked Cholesky, cached-factor GP priors
    on tilde_l and tilde_sigma, and -- when a parameter requires grad -- the analytic adjoint."""
    hyper = [_f(mu_tilde_l), _f(alpha_tilde_l), _f(beta_tilde_l), _f(mu_tilde_sigma), _f(alpha_tilde_sigma), _f(beta_tilde_sigma),
             _f(a), _f(b), _f(c)]
    res = _HadamardSepObjective.apply((bool(Prior), torch.is_grad_enabled()), hyper, x, indx, y, _as_tensor(tilde_l),
                                      _as_tensor(tilde_sigma), _as_tensor(L_vec), _as_tensor(tilde_sigma2_err))
    return res if verbose else res[0]


def _predict(tilde_l, tilde_sigma, L_vec, tilde_sigma2_err, x, indx, y, xs, mu_tilde_l, alpha_tilde_l, beta_tilde_l, mu_tilde_sigma,
             alpha_tilde_sigma, beta_tilde_sigma):
    c = _lib.default_context()
    c.had_set_data(_np(x).reshape(-1), _labels(indx), _np(y).reshape(-1))
    hyper = [_f(mu_tilde_l), _f(alpha_tilde_l), _f(beta_tilde_l), _f(mu_tilde_sigma), _f(alpha_tilde_sigma), _f(beta_tilde_sigma),
             1.0, 1.0, 1.0]
    pars = np.concatenate([_np(tilde_l).reshape(-1), _np(tilde_sigma).reshape(-1), _np(L_vec).reshape(-1),
                           _np(tilde_sigma2_err).reshape(-1)])
    mean, var, _ = c.predict_hads(pars, hyper, _np(xs).reshape(-1))
    return _bands(mean, var)


def point_predmap_hadamard(tilde_l, tilde_sigma, L_vec, tilde_sigma2_err, x, indx, y, x_star, mu_tilde_l, alpha_tilde_l, beta_tilde_l,
                           mu_tilde_sigma, alpha_tilde_sigma, beta_tilde_sigma, *args, **kwargs):
    """[mu - 1.96 s, mu, mu + 1.96 s] of all M outputs at x_star ([3, M]); reference prediction.py:710-785."""
    return _predict(tilde_l, tilde_sigma, L_vec, tilde_sigma2_err, x, indx, y, x_star, mu_tilde_l, alpha_tilde_l, beta_tilde_l,
                    mu_tilde_sigma, alpha_tilde_sigma, beta_tilde_sigma)[0]


def pointwise_predmap_hadmard(tilde_l, tilde_sigma, L_vec, tilde_sigma2_err, x, indx, y, grids, mu_tilde_l, alpha_tilde_l,
                              beta_tilde_l, mu_tilde_sigma, alpha_tilde_sigma, beta_tilde_sigma, *args, **kwargs):
    """All grid points from one device call ([G, 3, M]); reference prediction.py:787-808 (its spelling of the name)."""
    return _predict(tilde_l, tilde_sigma, L_vec, tilde_sigma2_err, x, indx, y, grids, mu_tilde_l, alpha_tilde_l, beta_tilde_l,
                    mu_tilde_sigma, alpha_tilde_sigma, beta_tilde_sigma)


pointwise_predmap_hadamard = pointwise_predmap_hadmard


# ---- a cohort of ragged subjects: the padded parameter layout of nmgp_hads_subjects_eval ------------------------------------------------
def cohort_pack(vectors, nobs, M, Nmax=None, fill=0.0):
    """Reference-layout vectors of S ragged subjects -> the padded layout of ``Context.hads_subjects_eval``; the contract of
    ``hadamard.cohort_pack``.  ``vectors[s]`` is ``[k, P_s]`` (or ``[P_s]``: k = 1), ``P_s = 2 nobs[s] + T + 1``, the same k for every
    subject; the result is ``[S k, Pmax = 2 Nmax + T + 1]`` with row ``s k + j`` = vector j of subject s: its ``tilde_l`` in the first
    ``nobs[s]`` slots of the first block, its ``tilde_sigma`` in the first ``nobs[s]`` slots of the second, ``L_vec`` and
    ``tilde_sigma2_err`` in the last ``T + 1`` slots, ``fill`` in every padded slot (the device never reads those).  Parameters and
    gradients alike."""
    nobs = [int(n) for n in nobs]
    T = int(M) * (int(M) + 1) // 2
    Nmax = max(nobs) if Nmax is None else int(Nmax)
    if len(vectors) != len(nobs) or max(nobs) > Nmax:
        raise ValueError("%d vectors for %d subjects, or a subject larger than Nmax = %d" % (len(vectors), len(nobs), Nmax))
    vs = [np.atleast_2d(_np(v)) for v in vectors]
    k = vs[0].shape[0]
    out = np.full((len(nobs) * k, 2 * Nmax + T + 1), float(fill))
    for s, (v, n) in enumerate(zip(vs, nobs)):
        if v.shape != (k, 2 * n + T + 1):
            raise ValueError("subject %d: expected [%d, 2 nobs + T + 1 = %d], got %s" % (s, k, 2 * n + T + 1, v.shape))
        rows = out[s * k:(s + 1) * k]
        rows[:, :n] = v[:, :n]
        rows[:, Nmax:Nmax + n] = v[:, n:2 * n]
        rows[:, 2 * Nmax:] = v[:, 2 * n:]
    return out


def cohort_unpack(P, nobs, M, chains_per_subject=1):
    """The inverse of :func:`cohort_pack`: ``[S k, Pmax]`` -> a list of S arrays ``[k, P_s]`` (copies)."""
    P = np.atleast_2d(_np(P))
    nobs = [int(n) for n in nobs]
    T, k = int(M) * (int(M) + 1) // 2, int(chains_per_subject)
    Nmax, rem = divmod(P.shape[1] - T - 1, 2)
    if rem or Nmax < 0 or P.shape[0] != len(nobs) * k or max(nobs) > Nmax:
        raise ValueError("P %s does not fit %d subjects x %d chains of at most 2 Nmax + T + 1 slots, T = %d" % (P.shape, len(nobs), k, T))
    out = []
    for s, n in enumerate(nobs):
        rows = P[s * k:(s + 1) * k]
        out.append(np.concatenate([rows[:, :n], rows[:, Nmax:Nmax + n], rows[:, 2 * Nmax:]], axis=1))
    return out


def cohort_predict(ctx, draws, xs, hyper, indx_star=None, z=None, star=None):
    """MAP and posterior-draw prediction under the separable model for the cohort ``ctx`` holds (``Context.had_set_subjects``), in ONE
    device call (``nmgp_predsample_hads_subjects``); the contract of ``hadamard.cohort_predict`` with ``draws[s]``
    ``[H, 2 N_s + T + 1]``, ``hyper [9]`` and ``z[s]`` / ``star[s]`` ``[H, S_s, 2]`` (tilde_l*, tilde_sigma* before exp) as
    ``Context.predsample_hads`` takes them.  Returns per-subject ``(mean [H, S_s(, M)], var, star [H, S_s, 2], status [H])``."""
    def rows_of(vs, H, Nmax, M, T):
        nobs = []
        for s, v in enumerate(vs):
            n, rem = divmod(v.shape[1] - T - 1, 2)
            if rem or n < 1 or v.shape[0] != H:
                raise _lib.NmgpError("hadamard_sep.cohort_predict: draws[%d] %s is not [H = %d, 2 N_s + T + 1]" % (s, v.shape, H))
            nobs.append(n)
        return cohort_pack(vs, nobs, M, Nmax=Nmax)

    return _cohort_predict(ctx, "hadamard_sep.cohort_predict", lambda pars, x2, i2, nstar, H, z2, s2: ctx.predsample_hads_subjects(
        pars, hyper, x2, indx_star=i2, nstar=nstar, draws_per_subject=H, z=z2, star=s2), draws, xs, indx_star, z, star, rows_of,
        lambda T: 2)
