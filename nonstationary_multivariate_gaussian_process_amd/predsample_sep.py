"""Posterior-draw prediction of the separable and the stationary model behind the reference's signatures (reference:
Utility/prediction.py).

Three families, eight functions:

* ``point_`` / ``pointwise_`` / ``test_predsample`` (:34-186) work on a HISTORY of posterior draws of the separable model: per
  draw and new input the unconstrained ``tilde_l`` and ``tilde_sigma`` are regressed onto the input and sampled, and y is sampled
  from the draw's predictive distribution (``a2 = B_mm (sigma*^2 + 1e-6)``).
* ``point_`` / ``pointwise_`` / ``test_predmap_sampling`` (:189-334) work on ONE parameter vector and draw ``n_sample`` samples of
  the latent values and of y per new input (``a2 = B_mm sigma*^2``); they return (2.5 / 97.5 % quantiles, mean, std).
* ``pointwise_`` / ``test_predsample_S`` (:1640-1692) work on a history of the stationary model: nothing is regressed, ONE normal
  per (draw, grid point) is shared by the M outputs, and the result is draw-major ``[H, S, M]``.

The reference re-eigendecomposes the N x N ``K_x`` once per draw AND per grid point (the stationary functions invert the dense
MN x MN matrix per draw).  Here all grid points of all draws go through ONE call of ``nmgp_predsample_sep`` / ``_sta``: one batched
factorisation of the M blocks per draw (per parameter vector in the ``_sampling`` family, whose ``n_sample`` noise draws ride as
repeated grid points), draws batched on the device.  Nothing is printed per grid point.

Randomness, separable.  ``z=`` injects the standard normals in the reference's consumption order ``[S, H | n_sample, 2 + M]``
(grid point, draw, then tilde_l*, tilde_sigma*, the M outputs of y).  Without ``z=`` they are ONE ``torch.randn`` of that shape on
the global generator, so ``torch.manual_seed`` reproduces a run -- but not the reference's stream, which calls ``Normal.sample``
three times per (grid point, draw).

Randomness, stationary.  ``z=`` is ``[H, S]``.  Without it the numbers are ONE ``np.random.standard_normal((H, S))`` on NumPy's
global generator, which yields exactly the numbers of H S successive ``np.random.randn()`` calls: for this family
``np.random.seed`` reproduces the REFERENCE's own stream, and with it its samples.

These names are opt-in behind the reference's module name: with ``NMGP_PREDSAMPLE=1`` in the environment ``Utility.prediction``
serves them; otherwise they keep resolving to the user's checkout.  Importing this module directly always works.
"""
import numpy as np
import torch

from . import _lib
from .predsample import _f, _normals, _np, sample_y

NAMES = ("point_predsample", "pointwise_predsample", "test_predsample",
         "point_predmap_sampling", "pointwise_predmap_sampling", "test_predmap_sampling",
         "pointwise_predsample_S", "test_predsample_S")


def _hyper(mu_tilde_l, alpha_tilde_l, beta_tilde_l, mu_tilde_sigma, alpha_tilde_sigma, beta_tilde_sigma):
    return np.array([_f(mu_tilde_l), _f(alpha_tilde_l), _f(beta_tilde_l), _f(mu_tilde_sigma), _f(alpha_tilde_sigma),
                     _f(beta_tilde_sigma), 1.0, 1.0, 10.0])


def _run(pars, Y, x, xs, hyper, zlat, kss_jitter, ctx=None):
    """pars [H, P], xs [S], zlat [S, H, 2] -> mean, var [S, H, M], star [S, H, 2], status [H]."""
    c = ctx if ctx is not None else _lib.default_context()
    c.set_data(_np(x).reshape(-1), _np(Y))
    mean, var, star, status = c.predsample_sep(pars, hyper, xs, z=np.ascontiguousarray(zlat.transpose(1, 0, 2)),
                                               kss_jitter=kss_jitter)
    return mean.transpose(1, 0, 2), var.transpose(1, 0, 2), star.transpose(1, 0, 2), status


def _history(tilde_l_hist, tilde_sigma_hist, uL_vec_hist, tilde_sigma2_err_hist, N_sample):
    hs = [_np(tilde_l_hist), _np(tilde_sigma_hist), _np(uL_vec_hist), _np(tilde_sigma2_err_hist).reshape(-1)]
    if N_sample is not None:
        hs = [h[-N_sample:] for h in hs]                   # N_sample takes the LAST draws
    H = min(len(h) for h in hs)                            # the reference zips the four histories
    return np.concatenate([hs[0][:H].reshape(H, -1), hs[1][:H].reshape(H, -1), hs[2][:H].reshape(H, -1), hs[3][:H, None]], axis=1)


def _predsample(tilde_l_hist, tilde_sigma_hist, uL_vec_hist, tilde_sigma2_err_hist, Y, x, xs, hyper, N_sample, z):
    pars = _history(tilde_l_hist, tilde_sigma_hist, uL_vec_hist, tilde_sigma2_err_hist, N_sample)
    xs = _np(xs).reshape(-1)
    M = _np(Y).shape[1]
    zz = _normals((xs.shape[0], pars.shape[0], 2 + M), z)
    mean, var, _, _ = _run(pars, Y, x, xs, hyper, zz[:, :, :2], True)
    return sample_y(mean, var, zz[:, :, 2:])                                       # [S, H, M]


def point_predsample(tilde_l_hist, tilde_sigma_hist, uL_vec_hist, tilde_sigma2_err_hist, Y, x, x_star, mu_tilde_l, alpha_tilde_l,
                     beta_tilde_l, mu_tilde_sigma, alpha_tilde_sigma, beta_tilde_sigma, N_sample, *args, z=None, **kwargs):
    """Sampled y at x_star for the last N_sample draws: 2d tensor [N_hist, M]; reference prediction.py:34-131.
    z: [1, N_hist, 2 + M] standard normals (module docstring)."""
    hyper = _hyper(mu_tilde_l, alpha_tilde_l, beta_tilde_l, mu_tilde_sigma, alpha_tilde_sigma, beta_tilde_sigma)
    ys = _predsample(tilde_l_hist, tilde_sigma_hist, uL_vec_hist, tilde_sigma2_err_hist, Y, x, _np(x_star).reshape(1), hyper,
                     N_sample, z)
    return torch.from_numpy(np.ascontiguousarray(ys[0]))


def pointwise_predsample(tilde_l_hist, tilde_sigma_hist, uL_vec_hist, tilde_sigma2_err_hist, Y, x, grids, mu_tilde_l,
                         alpha_tilde_l, beta_tilde_l, mu_tilde_sigma, alpha_tilde_sigma, beta_tilde_sigma, N_sample, *args, z=None,
                         **kwargs):
    """Sampled y on a grid: NumPy array [N_grid, N_hist, M]; reference prediction.py:133-157.  All grid points of all draws go
    through one call of the device entry.  z: [N_grid, N_hist, 2 + M]."""
    hyper = _hyper(mu_tilde_l, alpha_tilde_l, beta_tilde_l, mu_tilde_sigma, alpha_tilde_sigma, beta_tilde_sigma)
    return np.ascontiguousarray(_predsample(tilde_l_hist, tilde_sigma_hist, uL_vec_hist, tilde_sigma2_err_hist, Y, x, grids, hyper,
                                            N_sample, z))


def test_predsample(tilde_l_hist, tilde_sigma_hist, uL_vec_hist, tilde_sigma2_err_hist, Y, x, x_test, mu_tilde_l, alpha_tilde_l,
                    beta_tilde_l, mu_tilde_sigma, alpha_tilde_sigma, beta_tilde_sigma, N_sample, *args, z=None, **kwargs):
    """The same at test inputs: NumPy array [N_test, N_hist, M]; reference prediction.py:159-186."""
    return pointwise_predsample(tilde_l_hist, tilde_sigma_hist, uL_vec_hist, tilde_sigma2_err_hist, Y, x, x_test, mu_tilde_l,
                                alpha_tilde_l, beta_tilde_l, mu_tilde_sigma, alpha_tilde_sigma, beta_tilde_sigma, N_sample, z=z)


test_predsample.__test__ = False                        # a reference signature, not a pytest test


def _sampling(n_sample, tilde_l, tilde_sigma, uL_vec, tilde_sigma2_err, Y, x, xs, hyper, z):
    """One parameter vector, n_sample noise draws per grid point: the grid is repeated n_sample times under ONE covariance."""
    pars = np.concatenate([_np(tilde_l).reshape(-1), _np(tilde_sigma).reshape(-1), _np(uL_vec).reshape(-1),
                           _np(tilde_sigma2_err).reshape(-1)])[None]
    xs = _np(xs).reshape(-1)
    S, n_sample = xs.shape[0], int(n_sample)
    M = _np(Y).shape[1]
    zz = _normals((S, n_sample, 2 + M), z)
    # entry layout: H = 1 draw, S n_sample inputs (grid point major, sample minor)
    mean, var, _, _ = _run(pars, Y, x, np.repeat(xs, n_sample), hyper, zz[:, :, :2].reshape(S * n_sample, 1, 2), False)
    ys = sample_y(mean.reshape(S, n_sample, M), var.reshape(S, n_sample, M), zz[:, :, 2:])
    return (np.percentile(ys, q=[2.5, 97.5], axis=1).transpose(1, 0, 2), np.mean(ys, axis=1), np.std(ys, axis=1))


def point_predmap_sampling(n_sample, tilde_l, tilde_sigma, uL_vec, tilde_sigma2_err, Y, x, x_star, mu_tilde_l, alpha_tilde_l,
                           beta_tilde_l, mu_tilde_sigma, alpha_tilde_sigma, beta_tilde_sigma, *args, z=None, **kwargs):
    """n_sample samples at x_star from one parameter vector; reference prediction.py:189-277.  Returns (2.5 / 97.5 % quantiles
    [2, M], mean [M], std [M]) of the sampled y.  z: [1, n_sample, 2 + M]."""
    hyper = _hyper(mu_tilde_l, alpha_tilde_l, beta_tilde_l, mu_tilde_sigma, alpha_tilde_sigma, beta_tilde_sigma)
    out = _sampling(n_sample, tilde_l, tilde_sigma, uL_vec, tilde_sigma2_err, Y, x, _np(x_star).reshape(1), hyper, z)
    return tuple(o[0] for o in out)


def pointwise_predmap_sampling(n_sample, tilde_l, tilde_sigma, uL_vec, tilde_sigma2_err, Y, x, grids, mu_tilde_l, alpha_tilde_l,
                               beta_tilde_l, mu_tilde_sigma, alpha_tilde_sigma, beta_tilde_sigma, *args, z=None, **kwargs):
    """The same on a grid; reference prediction.py:279-306: ([N_grid, 2, M], [N_grid, M], [N_grid, M]).
    z: [N_grid, n_sample, 2 + M]."""
    hyper = _hyper(mu_tilde_l, alpha_tilde_l, beta_tilde_l, mu_tilde_sigma, alpha_tilde_sigma, beta_tilde_sigma)
    return _sampling(n_sample, tilde_l, tilde_sigma, uL_vec, tilde_sigma2_err, Y, x, grids, hyper, z)


def test_predmap_sampling(n_sample, tilde_l, tilde_sigma, uL_vec, tilde_sigma2_err, Y, x, x_test, mu_tilde_l, alpha_tilde_l,
                          beta_tilde_l, mu_tilde_sigma, alpha_tilde_sigma, beta_tilde_sigma, *args, z=None, **kwargs):
    """The same at test inputs; reference prediction.py:308-334."""
    return pointwise_predmap_sampling(n_sample, tilde_l, tilde_sigma, uL_vec, tilde_sigma2_err, Y, x, x_test, mu_tilde_l,
                                      alpha_tilde_l, beta_tilde_l, mu_tilde_sigma, alpha_tilde_sigma, beta_tilde_sigma, z=z)


test_predmap_sampling.__test__ = False


def pointwise_predsample_S(tilde_ls, tilde_sigmas, uL_vecs, tilde_sigma2_errs, Y, x, grids, *args, z=None, **kwargs):
    """Stationary model, a history of draws on a grid: NumPy array [N_hist, N_grid, M] (draw-major, unlike the other families);
    reference prediction.py:1640-1665.  One normal per (draw, grid point) is shared by the M outputs.  z: [N_hist, N_grid];
    without it ``np.random.standard_normal((N_hist, N_grid))`` on NumPy's global generator -- the reference's own stream under
    ``np.random.seed`` (module docstring)."""
    pars = _history(tilde_ls, tilde_sigmas, uL_vecs, tilde_sigma2_errs, None)
    xs = _np(grids).reshape(-1)
    H, S = pars.shape[0], xs.shape[0]
    if z is None:
        zz = np.random.standard_normal((H, S))
    else:
        zz = _np(z)
        if zz.shape != (H, S):
            raise ValueError("z must have shape %s (draw, grid point), got %s" % ((H, S), zz.shape))
    c = _lib.default_context()
    c.set_data(_np(x).reshape(-1), _np(Y))
    mean, var, _ = c.predsample_sta(pars, xs)
    return mean + zz[:, :, None] * np.sqrt(var)


def test_predsample_S(tilde_ls, tilde_sigmas, uL_vecs, tilde_sigma2_errs, Y, x, test_x, *args, z=None, **kwargs):
    """The same at test inputs; reference prediction.py:1667-1692."""
    return pointwise_predsample_S(tilde_ls, tilde_sigmas, uL_vecs, tilde_sigma2_errs, Y, x, test_x, z=z)


test_predsample_S.__test__ = False
