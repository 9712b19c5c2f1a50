"""Posterior-draw prediction of the nonseparable model behind the reference's signatures (reference: Utility/prediction.py).

Two families, six functions:

* ``point_`` / ``pointwise_`` / ``test_predsample_inhomogeneous`` (:1265-1398) work on a HISTORY of posterior draws: per draw and
  new input the latent curves are regressed onto the input (on the constrained ``L_vecs``), sampled, and y is sampled from the
  draw's predictive distribution.
* ``point_`` / ``pointwise_`` / ``test_predmap_inhomogeneous_sampling`` (:1038-1262) work on ONE parameter vector and draw
  ``n_sample`` samples of the latent curves (regression on the unconstrained ``uL_vecs``) and of y per new input.

The reference rebuilds and eigendecomposes the MN x MN covariance once per draw AND per grid point.  Here all grid points of all
draws go through ONE call of ``nmgp_predsample_svc``: one factorisation per draw (per parameter vector in the ``_sampling``
family, whose ``n_sample`` noise draws ride as repeated grid points), draws batched on the device.

Randomness.  ``z=`` injects the standard normals in the reference's consumption order ``[S, H, 1 + T + M]`` (grid point, draw,
then tilde_l*, the T slots of L*, the M outputs of y; for ``pred_smoothness`` / ``pred_cov`` the last axis has only the 1 / T
numbers those modes consume).  Without ``z=`` they are ONE ``torch.randn`` of that shape on the global generator, so
``torch.manual_seed`` reproduces a run -- but NOT the reference's stream: the reference calls ``Normal.sample`` three times per
(grid point, draw) with 1, T and M numbers, the batched draw here takes all of them at once, so the same seed gives other numbers.

These names are opt-in behind the reference's module name: with ``NMGP_PREDSAMPLE=1`` in the environment
``Utility.prediction`` serves them; otherwise they keep resolving to the user's checkout.  Importing this module directly always
works.
"""
import os

import numpy as np
import torch

from . import _lib

NAMES = ("point_predsample_inhomogeneous", "pointwise_predsample_inhomogeneous", "test_predsample_inhomogeneous",
         "point_predmap_inhomogeneous_sampling", "pointwise_predmap_inhomogeneous_sampling",
         "test_predmap_inhomogeneous_sampling")


def enabled():
    """NMGP_PREDSAMPLE=1: ``Utility.prediction`` serves the names of this module."""
    return os.environ.get("NMGP_PREDSAMPLE", "") not in ("", "0")


def _f(v):
    return float(v.detach()) if isinstance(v, torch.Tensor) else float(v)


def _np(t):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(t, dtype=np.float64))


def _hyper(mu_tilde_l, alpha_tilde_l, beta_tilde_l, mu_L, alpha_L, beta_L):
    return np.array([_f(mu_tilde_l), _f(alpha_tilde_l), _f(beta_tilde_l), _f(mu_L), _f(alpha_L), _f(beta_L), 1.0, 1.0])


def _normals(shape, z):
    if z is None:
        return torch.randn(*shape, dtype=torch.float64).numpy()
    z = _np(z)
    if z.shape != tuple(shape):
        raise ValueError("z must have shape %s (grid point, draw, numbers consumed), got %s" % (tuple(shape), z.shape))
    return z


def sample_y(mean, var, zy):
    """y* = mean + sqrt(var) z_y (prediction.py:1346): formed on the host."""
    return mean + np.sqrt(var) * zy


def _run(pars, Y, x, xs, hyper, zlat, constrained, ctx=None):
    """pars [H, P], xs [S], zlat [S, H, 1+T] -> mean, var [S, H, M], star [S, H, 1+T], status [H]."""
    c = ctx if ctx is not None else _lib.default_context()
    c.set_data(_np(x).reshape(-1), _np(Y))
    mean, var, star, status = c.predsample_svc(pars, hyper, xs, z=np.ascontiguousarray(zlat.transpose(1, 0, 2)),
                                               constrained=constrained)
    return mean.transpose(1, 0, 2), var.transpose(1, 0, 2), star.transpose(1, 0, 2), status


def _history(tilde_l_hist, uL_vecs_hist, tilde_sigma2_err_hist, N_sample):
    tl, uL, ts = _np(tilde_l_hist), _np(uL_vecs_hist), _np(tilde_sigma2_err_hist).reshape(-1)
    tl, uL, ts = tl[-N_sample:], uL[-N_sample:], ts[-N_sample:]
    H = min(len(tl), len(uL), len(ts))                     # the reference zips the three histories
    return np.concatenate([tl[:H], uL[:H], ts[:H, None]], axis=1)


def _predsample(tilde_l_hist, uL_vecs_hist, tilde_sigma2_err_hist, Y, x, xs, hyper, N_sample, z):
    pars = _history(tilde_l_hist, uL_vecs_hist, tilde_sigma2_err_hist, N_sample)
    xs = _np(xs).reshape(-1)
    M = _np(Y).shape[1]
    T = M * (M + 1) // 2
    zz = _normals((xs.shape[0], pars.shape[0], 1 + T + M), z)
    mean, var, _, _ = _run(pars, Y, x, xs, hyper, zz[:, :, :1 + T], True)
    return sample_y(mean, var, zz[:, :, 1 + T:])                                   # [S, H, M]


def point_predsample_inhomogeneous(tilde_l_hist, uL_vecs_hist, tilde_sigma2_err_hist, Y, x, x_star, mu_tilde_l, alpha_tilde_l,
                                   beta_tilde_l, mu_L, alpha_L, beta_L, N_sample, *args, z=None, **kwargs):
    """Sampled y at x_star for the last N_sample draws: 2d tensor [N_hist, M]; reference prediction.py:1265-1357.
    z: [1, N_hist, 1 + T + M] standard normals (module docstring)."""
    hyper = _hyper(mu_tilde_l, alpha_tilde_l, beta_tilde_l, mu_L, alpha_L, beta_L)
    ys = _predsample(tilde_l_hist, uL_vecs_hist, tilde_sigma2_err_hist, Y, x, _np(x_star).reshape(1), hyper, N_sample, z)
    return torch.from_numpy(np.ascontiguousarray(ys[0]))


def pointwise_predsample_inhomogeneous(tilde_l_hist, uL_vecs_hist, tilde_sigma2_err_hist, Y, x, grids, mu_tilde_l, alpha_tilde_l,
                                       beta_tilde_l, mu_L, alpha_L, beta_L, N_sample, *args, z=None, **kwargs):
    """Sampled y on a grid: NumPy array [N_grid, N_hist, M]; reference prediction.py:1359-1378.  All grid points of all draws
    go through one call of the device entry.  z: [N_grid, N_hist, 1 + T + M]."""
    hyper = _hyper(mu_tilde_l, alpha_tilde_l, beta_tilde_l, mu_L, alpha_L, beta_L)
    return np.ascontiguousarray(_predsample(tilde_l_hist, uL_vecs_hist, tilde_sigma2_err_hist, Y, x, grids, hyper, N_sample, z))


def test_predsample_inhomogeneous(tilde_l_hist, uL_vecs_hist, tilde_sigma2_err_hist, Y, x, x_test, mu_tilde_l, alpha_tilde_l,
                                  beta_tilde_l, mu_L, alpha_L, beta_L, N_sample, *args, z=None, **kwargs):
    """The same at test inputs: NumPy array [N_test, N_hist, M]; reference prediction.py:1380-1398."""
    return pointwise_predsample_inhomogeneous(tilde_l_hist, uL_vecs_hist, tilde_sigma2_err_hist, Y, x, x_test, mu_tilde_l,
                                              alpha_tilde_l, beta_tilde_l, mu_L, alpha_L, beta_L, N_sample, z=z)


test_predsample_inhomogeneous.__test__ = False          # a reference signature, not a pytest test


def _sampling(n_sample, tilde_l, uL_vecs, tilde_sigma2_err, Y, x, xs, hyper, pred_smoothness, pred_cov, z):
    """One parameter vector, n_sample noise draws per grid point: the grid is repeated n_sample times under ONE covariance."""
    pars = np.concatenate([_np(tilde_l).reshape(-1), _np(uL_vecs).reshape(-1), _np(tilde_sigma2_err).reshape(-1)])[None]
    xs = _np(xs).reshape(-1)
    S, n_sample = xs.shape[0], int(n_sample)
    M = _np(Y).shape[1]
    T = M * (M + 1) // 2
    K = 1 if pred_smoothness else (T if pred_cov else 1 + T + M)
    zz = _normals((S, n_sample, K), z)
    zlat = np.zeros((S, n_sample, 1 + T))
    if pred_smoothness:
        zlat[:, :, :1] = zz
    elif pred_cov:
        zlat[:, :, 1:] = zz
    else:
        zlat = zz[:, :, :1 + T]
    # entry layout: H = 1 draw, S n_sample inputs (grid point major, sample minor)
    mean, var, star, _ = _run(pars, Y, x, np.repeat(xs, n_sample), hyper, zlat.reshape(S * n_sample, 1, 1 + T), False)
    star = star.reshape(S, n_sample, 1 + T)
    if pred_smoothness:
        return star[:, :, 0]                                                       # [S, n_sample]
    if pred_cov:
        Lf = np.zeros((S, n_sample, M, M))
        r, cidx = np.tril_indices(M)
        Lf[:, :, r, cidx] = star[:, :, 1:]
        return Lf                                                                  # [S, n_sample, M, M]
    ys = sample_y(mean.reshape(S, n_sample, M), var.reshape(S, n_sample, M), zz[:, :, 1 + T:])
    return (np.percentile(ys, q=[2.5, 97.5], axis=1).transpose(1, 0, 2), np.mean(ys, axis=1), np.std(ys, axis=1))


def point_predmap_inhomogeneous_sampling(n_sample, tilde_l, uL_vecs, tilde_sigma2_err, Y, x, x_star, mu_tilde_l, alpha_tilde_l,
                                         beta_tilde_l, mu_L, alpha_L, beta_L, pred_smoothness=False, pred_cov=False, *args,
                                         z=None, **kwargs):
    """n_sample samples at x_star from one parameter vector; reference prediction.py:1038-1192.  Returns the sampled tilde_l*
    [n_sample] (pred_smoothness), the sampled L* [n_sample, M, M] (pred_cov), else (2.5 / 97.5 % quantiles [2, M], mean [M],
    std [M]) of the sampled y.  z: [1, n_sample, 1 | T | 1 + T + M]."""
    hyper = _hyper(mu_tilde_l, alpha_tilde_l, beta_tilde_l, mu_L, alpha_L, beta_L)
    out = _sampling(n_sample, tilde_l, uL_vecs, tilde_sigma2_err, Y, x, _np(x_star).reshape(1), hyper, pred_smoothness, pred_cov, z)
    return tuple(o[0] for o in out) if isinstance(out, tuple) else out[0]


def pointwise_predmap_inhomogeneous_sampling(n_sample, tilde_l, uL_vecs, tilde_sigma2_err, Y, x, grids, mu_tilde_l, alpha_tilde_l,
                                             beta_tilde_l, mu_L, alpha_L, beta_L, pred_smoothness=False, pred_cov=False, *args,
                                             z=None, **kwargs):
    """The same on a grid; reference prediction.py:1194-1235: [N_grid, n_sample], [N_grid, n_sample, M, M], or
    ([N_grid, 2, M], [N_grid, M], [N_grid, M]).  z: [N_grid, n_sample, 1 | T | 1 + T + M]."""
    hyper = _hyper(mu_tilde_l, alpha_tilde_l, beta_tilde_l, mu_L, alpha_L, beta_L)
    return _sampling(n_sample, tilde_l, uL_vecs, tilde_sigma2_err, Y, x, grids, hyper, pred_smoothness, pred_cov, z)


def test_predmap_inhomogeneous_sampling(n_sample, tilde_l, uL_vecs, tilde_sigma2_err, Y, x, x_test, mu_tilde_l, alpha_tilde_l,
                                        beta_tilde_l, mu_L, alpha_L, beta_L, *args, z=None, **kwargs):
    """The same at test inputs (y only); reference prediction.py:1237-1262."""
    hyper = _hyper(mu_tilde_l, alpha_tilde_l, beta_tilde_l, mu_L, alpha_L, beta_L)
    return _sampling(n_sample, tilde_l, uL_vecs, tilde_sigma2_err, Y, x, x_test, hyper, False, False, z)


test_predmap_inhomogeneous_sampling.__test__ = False
