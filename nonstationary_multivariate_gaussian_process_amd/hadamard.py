"""Hadamard form of the nonseparable model behind the reference's signatures: irregularly observed outputs.

The data are N single observations ``(x[i], indx[i], y[i])``, ``indx[i]`` naming the output measured at ``x[i]`` (longitudinal
measurements where each output has its own time stamps), instead of a complete ``Y[N, M]``.  Served here:

* ``nlogpos_obj_hadamard_SVC`` / ``logpos_hadamard_SVC`` (reference ``Utility/logpos.py:566-659``): value and gradient from one
  device evaluation (``nmgp_had_batch_eval``), attached to autograd like ``logpos.nlogpos_obj_SVC``;
* ``point_predmap_SVC_hadamard`` / ``pointwise_predmap_SVC_hadamard`` (``Utility/prediction.py:1401-1478``): all grid points from
  one device call (``nmgp_predict_had``), nothing printed per grid point;
* ``generate_K_index_SVC_hadamard0`` (``logpos.py:121-124``) as a host helper.

``M`` is inferred from ``indx`` as the reference does (the number of distinct labels), so the labels must be 0 .. M-1 and each
must occur.  The parameter vector is ``[tilde_l (N) | L_vecs (N T) | tilde_sigma2_err]``; ``L_vecs`` enters ``vec2lowtriangle``
as it is (no exp on the diagonal slots).

Under this package's OWN names (the reference has none for them, so nothing is installed behind its module names):

* ``point_`` / ``pointwise_`` / ``indexedpoint_`` / ``test_predsample_SVC_hadamard``: sampled y from a HISTORY of posterior draws
  ``(tilde_l_hist [H, N], L_vecs_hist [H, N T], tilde_sigma2_err_hist [H])``, with the argument order of the reference's separable
  family (``prediction.py:461-707``) minus ``tilde_sigma_hist``: all M outputs at a new input / on a grid (``[H, M]`` /
  ``[S, H, M]``), or one labelled output per held-out pair (``[H]`` / ``[S_test, H]``).  All points of all draws go through ONE
  device call (``nmgp_predsample_had``);
* ``indexed_predict``: mean and variance of ONE labelled output per held-out input from one parameter vector -- the corrected
  form of the reference's ``test_predmap_SVC_hadamard``;
* ``cohort_pack`` / ``cohort_unpack`` / ``cohort_buckets``: host helpers of the cohort entry (``Context.had_set_subjects`` /
  ``had_subjects_eval``: S subjects of ragged size, padded to one order, S x k chains per launch sequence) -- the padded parameter
  layout and the grouping of subjects of similar size; ``drivers.HadamardCohortMAP`` is the MAP loop on top of them;
* ``cohort_predict`` (with ``cohort_pack_inputs`` / ``cohort_unpack_outputs``): MAP and posterior-draw prediction for the cohort at
  each subject's own new inputs, all subjects and draws in one device call (``nmgp_predsample_had_subjects``).

Not provided: ``indexedpoint_predmap_SVC_hadamard`` / ``test_predmap_SVC_hadamard`` themselves (their variance is output 0's for
every label; INTEGRATION.md says why).  The separable Hadamard model (``nlogpos_obj_hadamard``, ``point_predmap_hadamard``, ...) is
served by ``hadamard_sep.py``, the stationary one (``*_hadamard_S``, ``*_predmap_S_hadamard``) by ``hadamard_sta.py``, each under its
own opt-in.

The names are opt-in behind the reference's module names: with ``NMGP_HADAMARD=1`` in the environment ``Utility.logpos`` /
``Utility.prediction`` serve them; otherwise they keep resolving to the user's checkout.  Importing this module directly always
works.
"""
import os

import numpy as np
import torch

from . import _lib

LOGPOS_NAMES = ("nlogpos_obj_hadamard_SVC", "logpos_hadamard_SVC", "generate_K_index_SVC_hadamard0")
PREDICTION_NAMES = ("point_predmap_SVC_hadamard", "pointwise_predmap_SVC_hadamard")


def enabled():
    """NMGP_HADAMARD=1: ``Utility.logpos`` / ``Utility.prediction`` serve the names of this module."""
    return os.environ.get("NMGP_HADAMARD", "") not in ("", "0")


def _f(v):
    return float(v.detach()) if isinstance(v, torch.Tensor) else float(v)


def _np(t):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(t, dtype=np.float64))


def _labels(indx):
    if isinstance(indx, torch.Tensor):
        indx = indx.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(indx).reshape(-1).astype(np.int32))


def _as_tensor(v):
    return v if isinstance(v, torch.Tensor) else torch.tensor(float(v), dtype=torch.float64)


def generate_K_index_SVC_hadamard0(L_f_list, indexes):
    """R R^T with R[i] = row indexes[i] of L_f_list[i] ([N, N]); reference logpos.py:121-124.  (The device objective never
    materialises this matrix; the function is kept for callers that want it.)"""
    L = torch.stack([L_f[int(index), :] for L_f, index in zip(L_f_list, indexes)])
    return torch.mm(L, L.t())


def _bands(mean, var):
    """[mu - 1.96 s, mu, mu + 1.96 s] stacked on axis 1 ([S, 3, M]) as a double tensor."""
    sd = np.sqrt(var)
    pct = np.stack([mean - 1.96 * sd, mean, mean + 1.96 * sd], axis=1)
    return torch.from_numpy(np.ascontiguousarray(pct)).type(torch.DoubleTensor)


def _backward(fctx, gres, *unused):
    """The backward of every Hadamard objective: scatter d NegLog / d pars over the parameter pieces."""
    g = fctx.grad_np
    outs = [None] * 5          # the parameter pieces follow five non-tensor arguments
    if g is None:
        return tuple(outs + [None] * len(fctx.shapes))
    scale = -float(gres)          # grad_np is for NegLog = -res
    k = 0
    for shp in fctx.shapes:
        if shp is None:
            outs.append(None)
            k += 1
            continue
        cnt = int(np.prod(shp)) if len(shp) else 1
        outs.append(torch.from_numpy(g[k:k + cnt] * scale).type(torch.DoubleTensor).reshape(shp))
        k += cnt
    return tuple(outs)


def _objective(module, name, eval_method, what, doc):
    """The ``torch.autograd.Function`` of one Hadamard model: value + gradient from one C-ABI call, ``eval_method`` of
    ``_lib.Context``; ``what`` is the reference function its error speaks of, ``module`` the module that binds the class (its ``__module__``).  forward(flags, hyper, x, indx, y, *parameter pieces)
    -> (res, loglik, the model's prior terms ...), ``res`` the log posterior (NOT negated), the rest non-differentiable.  The
    gradient is computed in the forward call whenever a parameter requires grad and autograd is recording at the call site (see
    ``Utility.logpos._FusedObjective``)."""

    def forward(fctx, flags, hyper, x, indx, y, *pieces):
        prior, grad_mode = flags
        c = _lib.default_context()
        c.had_set_data(_np(x).reshape(-1), _labels(indx), _np(y).reshape(-1))
        flat = np.concatenate([_np(p).reshape(-1) for p in pieces])
        want_grad = bool(grad_mode) and any(isinstance(p, torch.Tensor) and p.requires_grad for p in pieces)
        out, grad, status = getattr(c, eval_method)(flat[None], hyper, prior, want_grad)
        if status[0] != 0:
            # torch.inverse raises on a singular covariance (reference logpos.py:528 / 623 / 690)
            raise RuntimeError("%s: the covariance is not positive definite or not finite (status %d)" % (what, int(status[0])))
        fctx.shapes = [tuple(p.shape) if isinstance(p, torch.Tensor) else None for p in pieces]
        fctx.grad_np = grad[0] if want_grad else None          # d NegLog / d pars
        res = [torch.tensor(-float(out[0, 0]), dtype=torch.float64)]
        res += [torch.tensor(float(v), dtype=torch.float64) for v in out[0, 1:]]
        fctx.mark_non_differentiable(*res[1:])
        return tuple(res)

    return type(name, (torch.autograd.Function,),
                {"forward": staticmethod(forward), "backward": staticmethod(_backward), "__doc__": doc, "__module__": module})


_HadamardObjective = _objective(
    __name__, "_HadamardObjective", "had_batch_eval", "nlogpos_obj_hadamard_SVC",
    "Nonseparable model: forward(flags, hyper, x, indx, y, tilde_l, L_vecs, tilde_sigma2_err) -> (res, loglik, lp_tilde_l, "
    "lp_L_vecs, lp_sigma2_err).")


def nlogpos_obj_hadamard_SVC(pars, x, indx, y, mu_tilde_l=0., alpha_tilde_l=1., beta_tilde_l=1., mu_L=0., alpha_L=1., beta_L=1.,
                             a=1, b=1, verbose=False, Prior=True):
    """Negative log posterior of the Hadamard nonseparable model on the flat parameter vector [tilde_l | L_vecs |
    tilde_sigma2_err]; verbose=True returns (NegLog, loglik, lp_tilde_l, lp_L_vecs, lp_sigma2_err).  reference logpos.py:566-585."""
    N = y.size(0)
    M = torch.unique(indx).size(0)
    T = int(M * (M + 1) / 2)
    tilde_l, L_vecs, tilde_sigma2_err = pars[:N], pars[N: N + N * T], pars[-1]
    if verbose:
        res, loglik, lp_l, lp_L, lp_s2 = logpos_hadamard_SVC(tilde_l, L_vecs, tilde_sigma2_err, x, indx, y, mu_tilde_l,
                                                             alpha_tilde_l, beta_tilde_l, mu_L, alpha_L, beta_L, a, b, verbose,
                                                             Prior)
        return -res, loglik, lp_l, lp_L, lp_s2
    return -logpos_hadamard_SVC(tilde_l, L_vecs, tilde_sigma2_err, x, indx, y, mu_tilde_l, alpha_tilde_l, beta_tilde_l, mu_L,
                                alpha_L, beta_L, a, b, verbose, Prior)


def logpos_hadamard_SVC(tilde_l, L_vecs, tilde_sigma2_err, x, indx, y, mu_tilde_l, alpha_tilde_l, beta_tilde_l, mu_L, alpha_L,
                        beta_L, a, b, verbose=False, Prior=True):
    """Log joint posterior of the Hadamard nonseparable model; reference logpos.py:588-659.  One device evaluation: covariance
    K_x o (R R^T) + sigma2 I of the N observations, blocked Cholesky, cached-factor GP priors on tilde_l and on the T raw
    L_vecs columns, and -- when a parameter requires grad -- the analytic adjoint."""
    hyper = [_f(mu_tilde_l), _f(alpha_tilde_l), _f(beta_tilde_l), _f(mu_L), _f(alpha_L), _f(beta_L), _f(a), _f(b)]
    res = _HadamardObjective.apply((bool(Prior), torch.is_grad_enabled()), hyper, x, indx, y, _as_tensor(tilde_l),
                                   _as_tensor(L_vecs), _as_tensor(tilde_sigma2_err))
    return res if verbose else res[0]


def _predict(tilde_l, L_vecs, tilde_sigma2_err, x, indx, y, xs, mu_tilde_l, alpha_tilde_l, beta_tilde_l, mu_L, alpha_L, beta_L):
    c = _lib.default_context()
    c.had_set_data(_np(x).reshape(-1), _labels(indx), _np(y).reshape(-1))
    hyper = [_f(mu_tilde_l), _f(alpha_tilde_l), _f(beta_tilde_l), _f(mu_L), _f(alpha_L), _f(beta_L), 1.0, 1.0]
    pars = np.concatenate([_np(tilde_l).reshape(-1), _np(L_vecs).reshape(-1), _np(tilde_sigma2_err).reshape(-1)])
    mean, var, _ = c.predict_had(pars, hyper, _np(xs).reshape(-1))
    return _bands(mean, var)


def point_predmap_SVC_hadamard(tilde_l, L_vecs, tilde_sigma2_err, x, indx, y, x_star, mu_tilde_l, alpha_tilde_l, beta_tilde_l,
                               mu_L, alpha_L, beta_L, *args, **kwargs):
    """[mu - 1.96 s, mu, mu + 1.96 s] of all M outputs at x_star ([3, M]); reference prediction.py:1401-1465."""
    return _predict(tilde_l, L_vecs, tilde_sigma2_err, x, indx, y, x_star, mu_tilde_l, alpha_tilde_l, beta_tilde_l, mu_L,
                    alpha_L, beta_L)[0]


def pointwise_predmap_SVC_hadamard(tilde_l, L_vecs, tilde_sigma2_err, x, indx, y, grids, *args, **kwargs):
    """All grid points from one device call ([G, 3, M]); reference prediction.py:1467-1478, which forwards ``*args, **kwargs``
    (the six GP-prior hyper-parameters, positionally or by keyword) to ``point_predmap_SVC_hadamard``."""
    names = ("mu_tilde_l", "alpha_tilde_l", "beta_tilde_l", "mu_L", "alpha_L", "beta_L")
    vals = list(args[:6])
    for k in names[len(vals):]:
        if k not in kwargs:
            raise TypeError("point_predmap_SVC_hadamard() missing required argument: %r" % k)
        vals.append(kwargs[k])
    return _predict(tilde_l, L_vecs, tilde_sigma2_err, x, indx, y, grids, *vals)


# ---- posterior-draw and held-out prediction: this package's own names (nmgp_predsample_had) --------------------------------------
def _hyper8(mu_tilde_l, alpha_tilde_l, beta_tilde_l, mu_L, alpha_L, beta_L):
    return np.array([_f(mu_tilde_l), _f(alpha_tilde_l), _f(beta_tilde_l), _f(mu_L), _f(alpha_L), _f(beta_L), 1.0, 1.0])


def _history(tilde_l_hist, L_vecs_hist, tilde_sigma2_err_hist):
    hs = [_np(tilde_l_hist), _np(L_vecs_hist), _np(tilde_sigma2_err_hist).reshape(-1)]
    H = min(len(h) for h in hs)                            # the histories are zipped, as the reference's separable family does
    return np.concatenate([hs[0][:H].reshape(H, -1), hs[1][:H].reshape(H, -1), hs[2][:H, None]], axis=1)


def _std_normals(shape, z, name):
    if z is None:
        return np.random.standard_normal(shape)
    z = _np(z)
    if z.shape != tuple(shape):
        raise ValueError("%s must have shape %s (new input, draw, numbers consumed), got %s" % (name, tuple(shape), z.shape))
    return z


def _predsample(hist, x, indx, y, xs, indx_star, hyper, z, zy):
    """Sampled y point-major: [S, H, M], or [S, H] with indx_star; ONE call of the device entry."""
    pars = _history(*hist)
    xs = _np(xs).reshape(-1)
    S, H = xs.shape[0], pars.shape[0]
    c = _lib.default_context()
    c.had_set_data(_np(x).reshape(-1), _labels(indx), _np(y).reshape(-1))
    M = int(np.unique(_labels(indx)).shape[0])
    T = M * (M + 1) // 2
    zl = _std_normals((S, H, 1 + T), z, "z")
    zy = _std_normals((S, H, M) if indx_star is None else (S, H), zy, "zy")
    mean, var, _, _ = c.predsample_had(pars, hyper, xs, indx_star=indx_star, z=np.ascontiguousarray(zl.transpose(1, 0, 2)))
    axes = (1, 0, 2) if indx_star is None else (1, 0)
    ys = mean.transpose(axes) + np.sqrt(var.transpose(axes)) * zy
    return torch.from_numpy(np.ascontiguousarray(ys))


def point_predsample_SVC_hadamard(tilde_l_hist, L_vecs_hist, tilde_sigma2_err_hist, x, indx, y, x_star, mu_tilde_l, alpha_tilde_l,
                                  beta_tilde_l, mu_L, alpha_L, beta_L, z=None, zy=None):
    """Sampled y of all M outputs at x_star, one row per draw: 2d tensor [H, M].  z [1, H, 1+T]: the standard normals of the latent
    regression (tilde_l*, the T slots of L*), zy [1, H, M]: those of y; both default to NumPy's global generator.  A draw whose
    covariance does not factor has a NaN row."""
    return _predsample((tilde_l_hist, L_vecs_hist, tilde_sigma2_err_hist), x, indx, y, _np(x_star).reshape(1), None,
                       _hyper8(mu_tilde_l, alpha_tilde_l, beta_tilde_l, mu_L, alpha_L, beta_L), z, zy)[0]


def pointwise_predsample_SVC_hadamard(tilde_l_hist, L_vecs_hist, tilde_sigma2_err_hist, x, indx, y, grids, mu_tilde_l, alpha_tilde_l,
                                      beta_tilde_l, mu_L, alpha_L, beta_L, z=None, zy=None):
    """Sampled y on a grid: 3d tensor [S, H, M]; all grid points of all draws go through one device call.  z [S, H, 1+T],
    zy [S, H, M]."""
    return _predsample((tilde_l_hist, L_vecs_hist, tilde_sigma2_err_hist), x, indx, y, grids, None,
                       _hyper8(mu_tilde_l, alpha_tilde_l, beta_tilde_l, mu_L, alpha_L, beta_L), z, zy)


def indexedpoint_predsample_SVC_hadamard(tilde_l_hist, L_vecs_hist, tilde_sigma2_err_hist, x, indx, y, x_star, indx_star, mu_tilde_l,
                                         alpha_tilde_l, beta_tilde_l, mu_L, alpha_L, beta_L, z=None, zy=None):
    """Sampled y of output indx_star at x_star, one value per draw: 1d tensor [H].  z [1, H, 1+T], zy [1, H]."""
    return _predsample((tilde_l_hist, L_vecs_hist, tilde_sigma2_err_hist), x, indx, y, _np(x_star).reshape(1),
                       _labels(indx_star).reshape(1), _hyper8(mu_tilde_l, alpha_tilde_l, beta_tilde_l, mu_L, alpha_L, beta_L), z,
                       zy)[0]


def test_predsample_SVC_hadamard(tilde_l_hist, L_vecs_hist, tilde_sigma2_err_hist, x, indx, y, x_test, indx_test, mu_tilde_l,
                                 alpha_tilde_l, beta_tilde_l, mu_L, alpha_L, beta_L, z=None, zy=None):
    """Sampled y at the held-out pairs (x_test[s], indx_test[s]): 2d tensor [S_test, H]; all pairs of all draws go through one device
    call.  z [S_test, H, 1+T], zy [S_test, H]."""
    return _predsample((tilde_l_hist, L_vecs_hist, tilde_sigma2_err_hist), x, indx, y, x_test, _labels(indx_test),
                       _hyper8(mu_tilde_l, alpha_tilde_l, beta_tilde_l, mu_L, alpha_L, beta_L), z, zy)


test_predsample_SVC_hadamard.__test__ = False           # a predictor of held-out ("test") pairs, not a pytest test


def indexed_predict(tilde_l, L_vecs, tilde_sigma2_err, x, indx, y, x_test, indx_test, **hyper):
    """(mean [S], var [S]) of output ``indx_test[s]`` at ``x_test[s]`` from ONE parameter vector (no noise: the conditional means
    of the starred values), the variance with ``(L* L*^T)[c*, c*]``; ``hyper``: the six GP-prior hyper-parameters by keyword
    (mu_tilde_l, alpha_tilde_l, beta_tilde_l, mu_L, alpha_L, beta_L).  The reference's ``test_predmap_SVC_hadamard``
    (prediction.py:1549-1561) returns the same mean, and this variance at the label-0 points only (see the module docstring)."""
    names = ("mu_tilde_l", "alpha_tilde_l", "beta_tilde_l", "mu_L", "alpha_L", "beta_L")
    missing = [k for k in names if k not in hyper]
    if missing:
        raise TypeError("indexed_predict() missing required keyword arguments: %s" % ", ".join(missing))
    c = _lib.default_context()
    c.had_set_data(_np(x).reshape(-1), _labels(indx), _np(y).reshape(-1))
    pars = np.concatenate([_np(tilde_l).reshape(-1), _np(L_vecs).reshape(-1), _np(tilde_sigma2_err).reshape(-1)])[None]
    mean, var, _, status = c.predsample_had(pars, _hyper8(*[hyper[k] for k in names]), _np(x_test).reshape(-1),
                                            indx_star=_labels(indx_test))
    if status[0] != 0:
        # torch.cholesky raises on a covariance that is not positive definite (reference prediction.py:1538)
        raise RuntimeError("indexed_predict: the covariance is not positive definite or not finite (status %d)" % int(status[0]))
    return (torch.from_numpy(np.ascontiguousarray(mean[0])).type(torch.DoubleTensor),
            torch.from_numpy(np.ascontiguousarray(var[0])).type(torch.DoubleTensor))


# ---- a cohort of ragged subjects: the padded parameter layout of nmgp_had_subjects_eval and the host-side bucketing ------------------
def _cohort_T(M):
    return int(M) * (int(M) + 1) // 2


def cohort_pack(vectors, nobs, M, Nmax=None, fill=0.0):
    """Reference-layout vectors of S ragged subjects -> the padded layout of ``Context.had_subjects_eval``.  ``vectors[s]`` is
    ``[k, P_s]`` (or ``[P_s]``: k = 1), ``P_s = nobs[s] (1 + T) + 1``, the same k for every subject; the result is
    ``[S k, Pmax = Nmax (1 + T) + 1]`` with row ``s k + j`` = vector j of subject s: its ``tilde_l`` in the first ``nobs[s]`` slots of
    the first block, its ``L_vecs`` in the first ``nobs[s] T`` slots of the second, ``tilde_sigma2_err`` in the last slot, ``fill``
    in every padded slot (the device never reads those).  Parameters and gradients alike."""
    nobs = [int(n) for n in nobs]
    T = _cohort_T(M)
    Nmax = max(nobs) if Nmax is None else int(Nmax)
    if len(vectors) != len(nobs) or max(nobs) > Nmax:
        raise ValueError("%d vectors for %d subjects, or a subject larger than Nmax = %d" % (len(vectors), len(nobs), Nmax))
    vs = [np.atleast_2d(_np(v)) for v in vectors]
    k = vs[0].shape[0]
    out = np.full((len(nobs) * k, Nmax * (1 + T) + 1), float(fill))
    for s, (v, n) in enumerate(zip(vs, nobs)):
        if v.shape != (k, n * (1 + T) + 1):
            raise ValueError("subject %d: expected [%d, nobs (1 + T) + 1 = %d], got %s" % (s, k, n * (1 + T) + 1, v.shape))
        rows = out[s * k:(s + 1) * k]
        rows[:, :n] = v[:, :n]
        rows[:, Nmax:Nmax + n * T] = v[:, n:n + n * T]
        rows[:, -1] = v[:, -1]
    return out


def cohort_unpack(P, nobs, M, chains_per_subject=1):
    """The inverse of :func:`cohort_pack`: ``[S k, Pmax]`` -> a list of S arrays ``[k, P_s]`` (copies)."""
    P = np.atleast_2d(_np(P))
    nobs = [int(n) for n in nobs]
    T, k = _cohort_T(M), int(chains_per_subject)
    Nmax, rem = divmod(P.shape[1] - 1, 1 + T)
    if rem or P.shape[0] != len(nobs) * k or max(nobs) > Nmax:
        raise ValueError("P %s does not fit %d subjects x %d chains of at most Nmax (1 + T) + 1 slots, T = %d" % (P.shape, len(nobs), k, T))
    out = []
    for s, n in enumerate(nobs):
        rows = P[s * k:(s + 1) * k]
        out.append(np.concatenate([rows[:, :n], rows[:, Nmax:Nmax + n * T], rows[:, -1:]], axis=1))
    return out


def cohort_buckets(nobs, max_flop_waste=0.5):
    """A deterministic partition of ``range(S)`` into sets for ``had_set_subjects``: a set of ``count`` subjects padded to its
    ``Nmax`` factors ``count * Nmax^3`` where the subjects need ``sum N_s^3``.  Subjects are sorted by size, descending (ties by
    index); a bucket opens at the largest remaining subject and takes the following ones while
    ``count * Nmax^3 <= (1 + max_flop_waste) * sum N_s^3`` holds.  ``max_flop_waste = 0`` gives buckets of equal sizes only.
    Returns a list of index arrays (each in that sorted order).

    The default 0.5 was not chosen from a measurement: fewer, larger batches amortise launch latency, padding costs flop, and where
    the two balance is unmeasured beyond the two points in the README (16 subjects of 512 .. 1024 observations: one set was faster
    than these buckets with one chain per subject, the buckets were faster with eight chains and gradients).
    ``tools/hadamard_cohort_bench.py`` reports one set against these buckets together with the flop ratio
    ``S Nmax^3 / sum N_s^3``, the figure a default should later be chosen from."""
    nobs = [int(n) for n in nobs]
    w = float(max_flop_waste)
    if w < 0.0 or any(n < 1 for n in nobs):
        raise ValueError("max_flop_waste must be >= 0 and every nobs positive")
    order = sorted(range(len(nobs)), key=lambda s: (-nobs[s], s))
    buckets, cur, nmax3, need = [], [], 0, 0
    for s in order:
        n3 = nobs[s] ** 3                              # (Python integers; both sides below are exact in double up to 2^53)
        if cur and (len(cur) + 1) * nmax3 <= (1.0 + w) * (need + n3):
            cur.append(s)
            need += n3
            continue
        if cur:
            buckets.append(np.array(cur, dtype=np.int64))
        cur, nmax3, need = [s], n3, n3
    if cur:
        buckets.append(np.array(cur, dtype=np.int64))
    return buckets


# ---- prediction for the cohort: the padded new-input arrays of nmgp_predsample_had_subjects ------------------------------------------
def cohort_pack_inputs(arrays, nstar=None, Smax=None, fill=0.0, dtype=np.float64):
    """Ragged per-subject new-input arrays -> one padded array.  ``arrays[s]`` is ``[S_s]`` (``xs``, ``indx_star``) -> ``[S, Smax]``;
    or ``[k, S_s, W]`` (``z``, ``star``; the same k and W for every subject) -> ``[S k, Smax, W]``, row ``s k + j`` = draw j of
    subject s.  ``Smax`` defaults to ``max(S_s)`` (at least 1: a cohort with nothing to predict still has one padded slot);
    ``fill`` goes into every padded slot (the device never reads those).  Returns ``(padded, nstar)``, nstar an int32 ``[S]``."""
    arrs = [_np(a) for a in arrays]
    if nstar is None:
        nstar = [a.shape[0] if a.ndim == 1 else a.shape[1] for a in arrs]
    nstar = np.asarray([int(n) for n in nstar], dtype=np.int32)
    Smax = max(1, int(nstar.max())) if Smax is None else int(Smax)
    if len(arrs) != nstar.shape[0] or len(arrs) < 1 or nstar.max() > Smax or Smax < 1:
        raise ValueError("%d arrays for %d subjects, or a subject with more new inputs than Smax = %d" % (len(arrs), nstar.shape[0], Smax))
    if arrs[0].ndim == 1:
        out = np.full((len(arrs), Smax), fill, dtype=dtype)
        for s, (a, n) in enumerate(zip(arrs, nstar)):
            if a.shape != (n,):
                raise ValueError("subject %d: expected [%d], got %s" % (s, n, a.shape))
            out[s, :n] = a
        return out, nstar
    k, W = arrs[0].shape[0], arrs[0].shape[2]
    out = np.full((len(arrs) * k, Smax, W), fill, dtype=dtype)
    for s, (a, n) in enumerate(zip(arrs, nstar)):
        if a.shape != (k, n, W):
            raise ValueError("subject %d: expected [%d, %d, %d], got %s" % (s, k, n, W, a.shape))
        out[s * k:(s + 1) * k, :n] = a
    return out, nstar


def cohort_unpack_outputs(A, nstar, draws_per_subject=1):
    """The inverse on the output side: ``[S k, Smax, ...]`` -> a list of S arrays ``[k, S_s, ...]`` (copies); a status vector
    ``[S k]`` -> a list of ``[k]``."""
    A, k = np.asarray(A), int(draws_per_subject)
    nstar = [int(n) for n in nstar]
    if A.shape[0] != len(nstar) * k or (A.ndim > 1 and max(nstar) > A.shape[1]):
        raise ValueError("array %s does not fit %d subjects x %d draws of at most Smax new inputs" % (A.shape, len(nstar), k))
    if A.ndim == 1:
        return [A[s * k:(s + 1) * k].copy() for s in range(len(nstar))]
    return [A[s * k:(s + 1) * k, :n].copy() for s, n in enumerate(nstar)]


def _cohort_predict(ctx, who, call, draws, xs, indx_star, z, star, rows_of, width):
    """The ragged-to-padded half the three models' ``cohort_predict`` share.  ``rows_of(vs, H, Nmax, M, T)`` checks the per-subject
    draws ``vs[s] [H, P_s]`` (the same H for every subject) and returns the entry's parameter rows; ``width(T)`` is the number of starred values per draw and input
    (0: the model has none); ``call(pars, x2, i2, nstar, H, z2, s2)`` is the device call on the padded arrays."""
    cohort = getattr(ctx, "_cohort", None)
    if cohort is None:
        raise _lib.NmgpError("%s: no cohort is set (Context.had_set_subjects)" % who)
    S, Nmax, M = cohort
    if not (len(draws) == len(xs) == S) or any(a is not None and len(a) != S for a in (indx_star, z, star)):
        raise _lib.NmgpError("%s: draws, xs (and indx_star, z, star) must be lists of one entry per subject (S = %d)" % (who, S))
    vs = [np.atleast_2d(_np(v)) for v in draws]
    T, H = _cohort_T(M), vs[0].shape[0]
    pars = rows_of(vs, H, Nmax, M, T)
    x2, nstar = cohort_pack_inputs([_np(v).reshape(-1) for v in xs])
    Smax, W = x2.shape[1], width(T)
    i2 = None if indx_star is None else cohort_pack_inputs([_np(v).reshape(-1) for v in indx_star], nstar, Smax, 0, np.int32)[0]
    z2, s2 = (None if a is None else cohort_pack_inputs([_np(v).reshape(H, int(n), W) for v, n in zip(a, nstar)], nstar, Smax)[0]
              for a in (z, star))
    return list(zip(*(cohort_unpack_outputs(a, nstar, H) for a in call(pars, x2, i2, nstar, H, z2, s2))))


def cohort_predict(ctx, draws, xs, hyper, indx_star=None, z=None, star=None):
    """MAP and posterior-draw prediction for the cohort ``ctx`` holds (``Context.had_set_subjects``) at each subject's OWN new
    inputs, in ONE device call (``nmgp_predsample_had_subjects``).  Ragged lists in the set's subject order: ``draws[s]`` ``[H, P_s]``
    (or ``[P_s]``: H = 1; the same H for every subject), ``xs[s]`` ``[S_s]`` (``S_s = 0`` allowed), ``indx_star[s]`` ``[S_s]`` labels
    (None: all M outputs per input), ``z[s]`` / ``star[s]`` ``[H, S_s, 1+T]`` as ``Context.predsample_had`` takes them.  Returns a list
    of per-subject ``(mean [H, S_s(, M)], var, star [H, S_s, 1+T], status [H])``; a draw with non-zero status has NaN moments."""
    def rows_of(vs, H, Nmax, M, T):
        nobs = []
        for s, v in enumerate(vs):
            n, rem = divmod(v.shape[1] - 1, 1 + T)
            if rem or v.shape[0] != H:
                raise _lib.NmgpError("cohort_predict: draws[%d] %s is not [H = %d, N_s (1 + T) + 1]" % (s, v.shape, H))
            nobs.append(n)
        return cohort_pack(vs, nobs, M, Nmax=Nmax)

    return _cohort_predict(ctx, "cohort_predict", lambda pars, x2, i2, nstar, H, z2, s2: ctx.predsample_had_subjects(
        pars, hyper, x2, indx_star=i2, nstar=nstar, draws_per_subject=H, z=z2, star=s2), draws, xs, indx_star, z, star, rows_of,
        lambda T: 1 + T)
