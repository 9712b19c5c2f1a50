"""Deterministic (MAP) prediction behind the reference's signatures (reference: Utility/prediction.py).

In scope: ``point_predmap_inhomogeneous`` (:912-988), ``pointwise_`` /
``test_predmap_inhomogeneous`` (:990-1036), ``point_predmap`` / ``pointwise_predmap`` / ``test_predmap`` (:337-458),
``pointwise_predmap_S`` / ``test_predmap_S`` (:1566-1638).  The reference rebuilds and eigendecomposes the full
MN x MN covariance for every grid point; here all grid points share ONE Cholesky factor on the GPU and the
cross-covariances are solved as one multi-right-hand-side triangular solve (nmgp_predict_*).
The nonseparable posterior-draw families (``*_predsample_inhomogeneous``, ``*_predmap_inhomogeneous_sampling``) live in
``nonstationary_multivariate_gaussian_process_amd.predsample`` (one batched device call for all draws and grid points) and are
served under this module's name only with ``NMGP_PREDSAMPLE=1`` in the environment: by default these names keep resolving to the
user's checkout, as every name outside the mirrored path does.  The separable and stationary posterior-draw families
(``*_predsample``, ``*_predmap_sampling``, ``*_predsample_S``) live in ``...predsample_sep`` under the same opt-in.
The MAP predictors of the Hadamard nonseparable model (irregularly observed outputs: ``point_`` / ``pointwise_predmap_SVC_hadamard``,
:1401-1478) live in ``...hadamard`` and are served under this module's name only with ``NMGP_HADAMARD=1``; those of the Hadamard
separable model (``point_predmap_hadamard`` / ``pointwise_predmap_hadmard``, :710-808) live in ``...hadamard_sep`` and are served only
with ``NMGP_HADAMARD_SEP=1``.  The posterior-draw families of the Hadamard separable model (``point_`` / ``pointwise_`` /
``indexedpoint_`` / ``test_predsample_hadamard``, :461-707) and the MAP forms of its indexed predictor
(``indexedpoint_predmap_hadamard`` / ``test_predmap_harmard``, :810-908, with ``test_predmap_hadamard`` as an alias) live in
``...predsample_hadamard`` and are served only with ``NMGP_PREDSAMPLE_HADAMARD=1``, a switch of its own: none of ``NMGP_HADAMARD``,
``NMGP_HADAMARD_SEP`` and ``NMGP_PREDSAMPLE`` serves them.  The MAP predictors of the Hadamard stationary model (``point_`` /
``pointwise_predmap_S_hadamard``, :1695-1740) live in ``...hadamard_sta`` and are served only with ``NMGP_HADAMARD_STA=1``.  The other
Hadamard names (``indexedpoint_`` / ``test_predmap_SVC_hadamard``, ``indexedpoint_predmap_S_hadamard`` / ``test_predmap_S_hadamard``)
keep resolving to the user's checkout whatever the switches: their variance takes output 0's prior variance for every label
(INTEGRATION.md); ``hadamard_sta.indexed_predict`` is the corrected stationary form.
"""
import numpy as np
import torch

from . import settings
from ._bridge import ctx, to_np, to_t


def _f(v):
    return float(v.detach()) if isinstance(v, torch.Tensor) else float(v)


def _percentiles(mean, var):
    sd = np.sqrt(var)
    return np.stack([mean - 1.96 * sd, mean, mean + 1.96 * sd], axis=1)          # [S, 3, M]


def _svc(tilde_l, uL_vecs, tilde_sigma2_err, Y, x, xs, hyper):
    c = ctx()
    c.set_data(x, Y)
    pars = np.concatenate([to_np(tilde_l).reshape(-1), to_np(uL_vecs).reshape(-1), to_np(tilde_sigma2_err).reshape(-1)])
    mean, var, Ls = c.predict_svc(pars, hyper, to_np(xs).reshape(-1))
    return to_t(_percentiles(mean, var)), to_t(Ls)


def point_predmap_inhomogeneous(tilde_l, uL_vecs, tilde_sigma2_err, Y, x, x_star, mu_tilde_l, alpha_tilde_l,
                                beta_tilde_l, mu_L, alpha_L, beta_L, *args, **kwargs):
    """Nonseparable model: [mu-1.96 s, mu, mu+1.96 s] ([3, M]) and the predicted L_vec ([T]) at x_star;
    reference prediction.py:912-988."""
    hyper = [_f(mu_tilde_l), _f(alpha_tilde_l), _f(beta_tilde_l), _f(mu_L), _f(alpha_L), _f(beta_L), 1.0, 1.0]
    pct, Ls = _svc(tilde_l, uL_vecs, tilde_sigma2_err, Y, x, x_star, hyper)
    return pct[0], Ls[0]


def pointwise_predmap_inhomogeneous(tilde_l, uL_vecs, tilde_sigma2_err, Y, x, grids, mu_tilde_l, alpha_tilde_l,
                                    beta_tilde_l, mu_L, alpha_L, beta_L, *args, **kwargs):
    """All grid points at once ([G, 3, M], [G, T]); reference prediction.py:990-1012."""
    hyper = [_f(mu_tilde_l), _f(alpha_tilde_l), _f(beta_tilde_l), _f(mu_L), _f(alpha_L), _f(beta_L), 1.0, 1.0]
    return _svc(tilde_l, uL_vecs, tilde_sigma2_err, Y, x, grids, hyper)


def test_predmap_inhomogeneous(tilde_l, L_vecs, tilde_sigma2_err, Y, x, x_test, mu_tilde_l, alpha_tilde_l, beta_tilde_l,
                               mu_L, alpha_L, beta_L, *args, **kwargs):
    """reference prediction.py:1014-1036 (same computation on test inputs)."""
    return pointwise_predmap_inhomogeneous(tilde_l, L_vecs, tilde_sigma2_err, Y, x, x_test, mu_tilde_l, alpha_tilde_l,
                                           beta_tilde_l, mu_L, alpha_L, beta_L)


def _sep(tilde_l, tilde_sigma, uL_vec, tilde_sigma2_err, Y, x, xs, hyper):
    c = ctx()
    c.set_data(x, Y)
    pars = np.concatenate([to_np(tilde_l).reshape(-1), to_np(tilde_sigma).reshape(-1), to_np(uL_vec).reshape(-1),
                           to_np(tilde_sigma2_err).reshape(-1)])
    mean, var = c.predict_sep(pars, hyper, to_np(xs).reshape(-1))
    return to_t(_percentiles(mean, var))


def point_predmap(tilde_l, tilde_sigma, uL_vec, tilde_sigma2_err, Y, x, x_star, mu_tilde_l, alpha_tilde_l, beta_tilde_l,
                  mu_tilde_sigma, alpha_tilde_sigma, beta_tilde_sigma, *args, **kwargs):
    """Separable model, one new input ([3, M]); reference prediction.py:337-408."""
    hyper = [_f(mu_tilde_l), _f(alpha_tilde_l), _f(beta_tilde_l), _f(mu_tilde_sigma), _f(alpha_tilde_sigma),
             _f(beta_tilde_sigma), 1.0, 1.0, 10.0]
    return _sep(tilde_l, tilde_sigma, uL_vec, tilde_sigma2_err, Y, x, x_star, hyper)[0]


def pointwise_predmap(tilde_l, tilde_sigma, uL_vec, tilde_sigma2_err, Y, x, grids, mu_tilde_l, alpha_tilde_l,
                      beta_tilde_l, mu_tilde_sigma, alpha_tilde_sigma, beta_tilde_sigma, *args, **kwargs):
    """[G, 3, M]; reference prediction.py:410-430."""
    hyper = [_f(mu_tilde_l), _f(alpha_tilde_l), _f(beta_tilde_l), _f(mu_tilde_sigma), _f(alpha_tilde_sigma),
             _f(beta_tilde_sigma), 1.0, 1.0, 10.0]
    return _sep(tilde_l, tilde_sigma, uL_vec, tilde_sigma2_err, Y, x, grids, hyper)


def test_predmap(tilde_l, tilde_sigma, uL_vec, tilde_sigma2_err, Y, x, x_test, mu_tilde_l, alpha_tilde_l, beta_tilde_l,
                 mu_tilde_sigma, alpha_tilde_sigma, beta_tilde_sigma, *args, **kwargs):
    """reference prediction.py:432-458."""
    return pointwise_predmap(tilde_l, tilde_sigma, uL_vec, tilde_sigma2_err, Y, x, x_test, mu_tilde_l, alpha_tilde_l,
                             beta_tilde_l, mu_tilde_sigma, alpha_tilde_sigma, beta_tilde_sigma)


def _sta(tilde_l, tilde_sigma, uL_vec, tilde_sigma2_err, Y, x, xs):
    c = ctx()
    c.set_data(x, Y)
    pars = np.concatenate([to_np(tilde_l).reshape(-1), to_np(tilde_sigma).reshape(-1), to_np(uL_vec).reshape(-1),
                           to_np(tilde_sigma2_err).reshape(-1)])
    return c.predict_sta(pars, to_np(xs).reshape(-1))


def pointwise_predmap_S(tilde_l, tilde_sigma, uL_vec, tilde_sigma2_err, Y, x, grids, *args, **kwargs):
    """Stationary model on a grid ([G, 3, M]); reference prediction.py:1566-1599."""
    mean, var = _sta(tilde_l, tilde_sigma, uL_vec, tilde_sigma2_err, Y, x, grids)
    return to_t(_percentiles(mean, var))


def test_predmap_S(tilde_l, tilde_sigma, uL_vec, tilde_sigma2_err, Y, x, test_x, *args, **kwargs):
    """Stationary model: (mean [S, M], std [S, M]); reference prediction.py:1601-1638."""
    mean, var = _sta(tilde_l, tilde_sigma, uL_vec, tilde_sigma2_err, Y, x, test_x)
    return to_t(mean), to_t(np.sqrt(var))


def __getattr__(name):
    """Names outside the mirrored path come from the user's reference checkout (Utility/_overlay.py)."""
    from .. import hadamard, hadamard_sep, hadamard_sta, predsample, predsample_hadamard, predsample_sep
    for mod in (hadamard, hadamard_sep, hadamard_sta):
        if name in mod.PREDICTION_NAMES and mod.enabled():
            return getattr(mod, name)
    if name in predsample_hadamard.NAMES and predsample_hadamard.enabled():
        return getattr(predsample_hadamard, name)
    for mod in (predsample, predsample_sep):
        if name in mod.NAMES and predsample.enabled():
            return getattr(mod, name)
    from . import _overlay
    return _overlay.module_getattr(__name__, name)
