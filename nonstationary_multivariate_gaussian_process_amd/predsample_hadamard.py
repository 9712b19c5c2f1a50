"""Posterior-draw prediction of the separable Hadamard model behind the reference's signatures (reference:
Utility/prediction.py:461-707 and :810-908).

The data are N single observations ``(x[i], indx[i], y[i])`` as in ``hadamard_sep.py``; a HISTORY of posterior draws
``(tilde_l_hist [H, N], tilde_sigma_hist [H, N], L_vec_hist [H, T], tilde_sigma2_err_hist [H])`` is turned into sampled y:

* ``point_`` / ``pointwise_predsample_hadamard`` (:461-583): all M outputs at a new input / on a grid -- ``[H, M]`` /
  ``[S, H, M]``;
* ``indexedpoint_`` / ``test_predsample_hadamard`` (:585-707): output ``indx_star`` only at ``x_star`` / at the held-out pairs
  ``(x_test[s], indx_test[s])`` -- ``[H]`` / ``[S_test, H]``;
* ``indexedpoint_predmap_hadamard`` / ``test_predmap_harmard`` (:810-908; the second name is the reference's spelling,
  ``test_predmap_hadamard`` is offered as an alias): the MAP forms of the indexed predictor, ONE parameter vector and no noise,
  ``[mean - 1.96 sd, mean, mean + 1.96 sd]`` as ``[3]`` / ``[S_test, 3]``.

Per draw and new input the unconstrained ``tilde_l`` and ``tilde_sigma`` are regressed onto the input under their RBF priors and
sampled; y is sampled from the draw's predictive distribution with variance ``B_f[m, m] (sigma*^2 + 1e-6) - |L_S^-1 k_f|^2 +
sigma2_err``.  The reference rebuilds and eigendecomposes the N x N covariance once per draw AND per new input, inverts it and runs
a Cholesky on the inverse.  The covariance depends on the draw only: here all points of all draws go through ONE call of
``nmgp_predsample_hads`` -- one factorisation per draw with y and the cross-covariance rows of all new inputs riding below it, the
draws batched on the device.  There is no ``N_sample`` argument (the reference has none); the four histories are zipped.  Nothing
is printed per grid point.

Randomness.  ``z=`` injects the standard normals in the reference's consumption order: point, draw, then ``tilde_l*``,
``tilde_sigma*`` and y -- ``[S, H, 2 + M]`` for the grid forms, ``[S, H, 3]`` for the indexed forms (``[1, H, ...]`` for the point
forms).  Without ``z=`` they are ONE ``torch.randn`` of that shape on the global generator, so ``torch.manual_seed`` reproduces a
run -- but not the reference's stream, which calls ``Normal.sample`` three times per (point, draw).

``M`` is inferred from ``indx`` as the reference does (the number of distinct labels), so the labels must be 0 .. M-1 and each
must occur.

The names are opt-in behind the reference's module name: with ``NMGP_PREDSAMPLE_HADAMARD=1`` in the environment
``Utility.prediction`` serves them; otherwise they keep resolving to the user's checkout (``NMGP_HADAMARD``, ``NMGP_HADAMARD_SEP``
and ``NMGP_PREDSAMPLE`` do not serve them).  Importing this module directly always works.
"""
import os

import numpy as np
import torch

from . import _lib
from .hadamard import _f, _labels, _np
from .predsample import _normals, sample_y

NAMES = ("point_predsample_hadamard", "pointwise_predsample_hadamard", "indexedpoint_predsample_hadamard",
         "test_predsample_hadamard", "indexedpoint_predmap_hadamard", "test_predmap_harmard", "test_predmap_hadamard")


def enabled():
    """NMGP_PREDSAMPLE_HADAMARD=1: ``Utility.prediction`` serves the names of this module."""
    return os.environ.get("NMGP_PREDSAMPLE_HADAMARD", "") not in ("", "0")


def _hyper(mu_tilde_l, alpha_tilde_l, beta_tilde_l, mu_tilde_sigma, alpha_tilde_sigma, beta_tilde_sigma):
    return np.array([_f(mu_tilde_l), _f(alpha_tilde_l), _f(beta_tilde_l), _f(mu_tilde_sigma), _f(alpha_tilde_sigma),
                     _f(beta_tilde_sigma), 1.0, 1.0, 1.0])


def _history(tilde_l_hist, tilde_sigma_hist, L_vec_hist, tilde_sigma2_err_hist):
    hs = [_np(tilde_l_hist), _np(tilde_sigma_hist), _np(L_vec_hist), _np(tilde_sigma2_err_hist).reshape(-1)]
    H = min(len(h) for h in hs)                            # the reference zips the four histories
    return np.concatenate([hs[0][:H].reshape(H, -1), hs[1][:H].reshape(H, -1), hs[2][:H].reshape(H, -1), hs[3][:H, None]], axis=1)


def _run(pars, x, indx, y, xs, indx_star, hyper, zlat, ctx=None):
    """pars [H, P], xs [S], zlat [S, H, 2] or None -> mean, var point-major ([S, H, M], or [S, H] with indx_star), status [H]."""
    c = ctx if ctx is not None else _lib.default_context()
    c.had_set_data(_np(x).reshape(-1), _labels(indx), _np(y).reshape(-1))
    z = None if zlat is None else np.ascontiguousarray(zlat.transpose(1, 0, 2))
    mean, var, _, status = c.predsample_hads(pars, hyper, xs, indx_star=indx_star, z=z)
    axes = (1, 0, 2) if indx_star is None else (1, 0)
    return mean.transpose(axes), var.transpose(axes), status


def _predsample(hist, x, indx, y, xs, indx_star, hyper, z):
    pars = _history(*hist)
    xs = _np(xs).reshape(-1)
    S, H = xs.shape[0], pars.shape[0]
    if indx_star is None:
        M = int(np.unique(_labels(indx)).shape[0])
        zz = _normals((S, H, 2 + M), z)
        mean, var, _ = _run(pars, x, indx, y, xs, None, hyper, zz[:, :, :2])
        ys = sample_y(mean, var, zz[:, :, 2:])                                     # [S, H, M]
    else:
        zz = _normals((S, H, 3), z)
        mean, var, _ = _run(pars, x, indx, y, xs, _labels(indx_star), hyper, zz[:, :, :2])
        ys = sample_y(mean, var, zz[:, :, 2])                                      # [S, H]
    return torch.from_numpy(np.ascontiguousarray(ys))


def point_predsample_hadamard(tilde_l_hist, tilde_sigma_hist, L_vec_hist, tilde_sigma2_err_hist, x, indx, y, x_star, mu_tilde_l,
                              alpha_tilde_l, beta_tilde_l, mu_tilde_sigma, alpha_tilde_sigma, beta_tilde_sigma, *args, z=None,
                              **kwargs):
    """Sampled y of all M outputs at x_star, one row per draw: 2d tensor [N_hist, M]; reference prediction.py:461-553.
    z: [1, N_hist, 2 + M] standard normals (module docstring)."""
    hyper = _hyper(mu_tilde_l, alpha_tilde_l, beta_tilde_l, mu_tilde_sigma, alpha_tilde_sigma, beta_tilde_sigma)
    return _predsample((tilde_l_hist, tilde_sigma_hist, L_vec_hist, tilde_sigma2_err_hist), x, indx, y, _np(x_star).reshape(1), None,
                       hyper, z)[0]


def pointwise_predsample_hadamard(tilde_l_hist, tilde_sigma_hist, L_vec_hist, tilde_sigma2_err_hist, x, indx, y, grids, mu_tilde_l,
                                  alpha_tilde_l, beta_tilde_l, mu_tilde_sigma, alpha_tilde_sigma, beta_tilde_sigma, *args, z=None,
                                  **kwargs):
    """Sampled y on a grid: 3d tensor [N_grid, N_hist, M]; reference prediction.py:555-583.  All grid points of all draws go
    through one call of the device entry.  z: [N_grid, N_hist, 2 + M]."""
    hyper = _hyper(mu_tilde_l, alpha_tilde_l, beta_tilde_l, mu_tilde_sigma, alpha_tilde_sigma, beta_tilde_sigma)
    return _predsample((tilde_l_hist, tilde_sigma_hist, L_vec_hist, tilde_sigma2_err_hist), x, indx, y, grids, None, hyper, z)


def indexedpoint_predsample_hadamard(tilde_l_hist, tilde_sigma_hist, L_vec_hist, tilde_sigma2_err_hist, x, indx, y, x_star, indx_star,
                                     mu_tilde_l, alpha_tilde_l, beta_tilde_l, mu_tilde_sigma, alpha_tilde_sigma, beta_tilde_sigma,
                                     *args, z=None, **kwargs):
    """Sampled y of output indx_star at x_star, one value per draw: 1d tensor [N_hist]; reference prediction.py:585-676.
    z: [1, N_hist, 3]."""
    hyper = _hyper(mu_tilde_l, alpha_tilde_l, beta_tilde_l, mu_tilde_sigma, alpha_tilde_sigma, beta_tilde_sigma)
    return _predsample((tilde_l_hist, tilde_sigma_hist, L_vec_hist, tilde_sigma2_err_hist), x, indx, y, _np(x_star).reshape(1),
                       np.asarray(_labels(indx_star)).reshape(1), hyper, z)[0]


def test_predsample_hadamard(tilde_l_hist, tilde_sigma_hist, L_vec_hist, tilde_sigma2_err_hist, x, indx, y, x_test, indx_test,
                             mu_tilde_l, alpha_tilde_l, beta_tilde_l, mu_tilde_sigma, alpha_tilde_sigma, beta_tilde_sigma, *args,
                             z=None, **kwargs):
    """Sampled y at the held-out pairs (x_test[s], indx_test[s]): 2d tensor [N_test, N_hist]; reference prediction.py:678-707.
    All pairs of all draws go through one call of the device entry.  z: [N_test, N_hist, 3]."""
    hyper = _hyper(mu_tilde_l, alpha_tilde_l, beta_tilde_l, mu_tilde_sigma, alpha_tilde_sigma, beta_tilde_sigma)
    return _predsample((tilde_l_hist, tilde_sigma_hist, L_vec_hist, tilde_sigma2_err_hist), x, indx, y, x_test,
                       np.asarray(_labels(indx_test)).reshape(-1), hyper, z)


test_predsample_hadamard.__test__ = False               # a reference signature, not a pytest test


def _predmap(tilde_l, tilde_sigma, L_vec, tilde_sigma2_err, x, indx, y, xs, indx_star, hyper):
    pars = np.concatenate([_np(tilde_l).reshape(-1), _np(tilde_sigma).reshape(-1), _np(L_vec).reshape(-1),
                           _np(tilde_sigma2_err).reshape(-1)])[None]
    mean, var, _ = _run(pars, x, indx, y, _np(xs).reshape(-1), np.asarray(_labels(indx_star)).reshape(-1), hyper, None)
    mean, sd = mean[:, 0], np.sqrt(var[:, 0])
    return torch.from_numpy(np.ascontiguousarray(np.stack([mean - 1.96 * sd, mean, mean + 1.96 * sd], axis=1)))    # [S, 3]


def indexedpoint_predmap_hadamard(tilde_l, tilde_sigma, L_vec, tilde_sigma2_err, x, indx, y, x_star, indx_star, mu_tilde_l,
                                  alpha_tilde_l, beta_tilde_l, mu_tilde_sigma, alpha_tilde_sigma, beta_tilde_sigma, *args, **kwargs):
    """[mu - 1.96 s, mu, mu + 1.96 s] of output indx_star at x_star from ONE parameter vector ([3]); reference
    prediction.py:810-885."""
    hyper = _hyper(mu_tilde_l, alpha_tilde_l, beta_tilde_l, mu_tilde_sigma, alpha_tilde_sigma, beta_tilde_sigma)
    return _predmap(tilde_l, tilde_sigma, L_vec, tilde_sigma2_err, x, indx, y, _np(x_star).reshape(1),
                    np.asarray(_labels(indx_star)).reshape(1), hyper)[0]


def test_predmap_harmard(tilde_l, tilde_sigma, L_vec, tilde_sigma2_err, x, indx, y, x_test, indx_test, mu_tilde_l, alpha_tilde_l,
                         beta_tilde_l, mu_tilde_sigma, alpha_tilde_sigma, beta_tilde_sigma, *args, **kwargs):
    """The same at the held-out pairs (x_test[s], indx_test[s]), all from one device call ([N_test, 3]); reference
    prediction.py:887-908 (its spelling of the name)."""
    hyper = _hyper(mu_tilde_l, alpha_tilde_l, beta_tilde_l, mu_tilde_sigma, alpha_tilde_sigma, beta_tilde_sigma)
    return _predmap(tilde_l, tilde_sigma, L_vec, tilde_sigma2_err, x, indx, y, x_test, indx_test, hyper)


test_predmap_harmard.__test__ = False
test_predmap_hadamard = test_predmap_harmard
