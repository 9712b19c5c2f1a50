"""Posterior-draw prediction without a GPU: a NumPy restatement of what the reference computes (prediction.py:1265-1398 and
:1038-1262, with their quirks) against the fixtures recorded from the reference (tests/golden/make_golden_predsample.py), the
pure-NumPy summary of ``drivers.posterior_predict``, and the opt-in name resolution of ``Utility.prediction``.

The restatement (``restate``) is also what the GPU tests compare the device entry with where no fixture exists.

Bars (the N = 512 prediction bars the project already uses): mean rtol 1e-5 / atol 1e-7, variance rtol 1e-5 / atol 1e-9, starred
values rtol 1e-6 / atol 1e-6 -- the last covers an LU against a Cholesky solve with the GP-prior covariance (condition number
~1e11), as in test_prediction_on_the_reference_grid."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from conftest import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JITTER = 1e-6
PRECISION = 1e-6
MEAN_TOL = dict(rtol=1e-5, atol=1e-7)
VAR_TOL = dict(rtol=1e-5, atol=1e-9)
STAR_TOL = dict(rtol=1e-6, atol=1e-6)


# ---- the restatement -----------------------------------------------------------------------------------------------
def rbf(x1, x2, alpha, beta):
    a, b = x1 / beta, x2 / beta
    dist = (a ** 2)[:, None] + (b ** 2)[None, :] - 2.0 * a[:, None] * b[None, :]
    return np.exp(-0.5 * dist) * alpha ** 2


def gibbs(x1, l1, x2, l2):
    dist = (x1 ** 2)[:, None] + (x2 ** 2)[None, :] - 2.0 * x1[:, None] * x2[None, :]
    A = (l1 ** 2)[:, None] + (l2 ** 2)[None, :]
    return np.sqrt(2.0 * l1[:, None] * l2[None, :] / A) * np.exp(-dist / A)


def diag_slots(M):
    return np.array([r * (r + 1) // 2 + r for r in range(M)])


def tril_from_vec(v, M):
    """v [..., T] (tril row-major slots) -> [..., M, M]"""
    L = np.zeros(v.shape[:-1] + (M, M))
    r, c = np.tril_indices(M)
    L[..., r, c] = v
    return L


def regression(x, xs, alpha, beta):
    """proj [N, S] = Sigma^-1 k (the reference's proj-first order) and the clipped conditional variances [S]."""
    Sig = rbf(x, x, alpha, beta) + JITTER * np.eye(len(x))
    k = rbf(x, xs, alpha, beta)
    proj = np.linalg.solve(Sig, k)
    cv = (alpha ** 2 + JITTER) - np.sum(proj * k, axis=0)
    return proj, np.where(cv < 0, PRECISION, cv)


def split_pars(p, N, M):
    T = M * (M + 1) // 2
    return p[:N], p[N:N + N * T].reshape(N, T), p[-1]


def restate(x, Y, pars, hyper, xs, z=None, constrained=True, star=None):
    """pars [H, P], xs [S], z [S, H, 1 + T] or None (zeros), star [S, H, 1 + T] or None (regress).
    Returns mean, var [S, H, M] and the starred values [S, H, 1 + T] as they enter exp() / vec2lowtriangle."""
    x, Y, pars, xs = (np.asarray(a, dtype=np.float64) for a in (x, Y, pars, xs))
    N, M = Y.shape
    T = M * (M + 1) // 2
    H, S = pars.shape[0], xs.shape[0]
    mu_l, al_l, be_l, mu_L, al_L, be_L = [float(v) for v in hyper[:6]]
    y = Y.T.reshape(-1)
    dg = diag_slots(M)
    if star is None:
        proj_l, cv_l = regression(x, xs, al_l, be_l)
        proj_L, cv_L = regression(x, xs, al_L, be_L)
        z = np.zeros((S, H, 1 + T)) if z is None else np.asarray(z, dtype=np.float64)
    mean, var, out_star = np.empty((S, H, M)), np.empty((S, H, M)), np.empty((S, H, 1 + T))
    for h in range(H):
        tl, uL, ts = split_pars(pars[h], N, M)
        Lv = uL.copy()
        Lv[:, dg] = np.exp(Lv[:, dg])                               # uLvecs2Lvecs
        if star is None:
            st = np.empty((S, 1 + T))
            st[:, 0] = mu_l + proj_l.T @ (tl - mu_l) + np.sqrt(cv_l) * z[:, h, 0]
            curve = Lv if constrained else uL                       # the predsample flavour regresses the CONSTRAINED L_vecs
            st[:, 1:] = mu_L + proj_L.T @ (curve - mu_L) + np.sqrt(cv_L)[:, None] * z[:, h, 1:]
            if not constrained:
                st[:, 1 + dg] = np.exp(st[:, 1 + dg])               # uLvec2Lvec after the noise
        else:
            st = np.asarray(star, dtype=np.float64)[:, h]
        out_star[:, h] = st
        ell, sig2 = np.exp(tl), np.exp(ts)
        Lf = tril_from_vec(Lv, M)                                   # [N, M, M]
        Kx = gibbs(x, ell, x, ell) + JITTER * np.eye(N)
        B = np.einsum("imr,jnr->minj", Lf, Lf)                      # (L_i L_j^T)[m, n] at [(m, i), (n, j)]
        Sigma = (B * Kx[None, :, None, :]).reshape(M * N, M * N) + sig2 * np.eye(M * N)
        Ls = tril_from_vec(st[:, 1:], M)                            # [S, M, M]
        kx = gibbs(x, ell, xs, np.exp(st[:, 0]))                    # [N, S]
        kf = np.einsum("is,imr,snr->misn", kx, Lf, Ls).reshape(M * N, S * M)
        sol = np.linalg.solve(Sigma, np.concatenate([y[:, None], kf], axis=1))
        mean[:, h] = (kf.T @ sol[:, 0]).reshape(S, M)
        v = (1.0 + JITTER) * np.einsum("smr,smr->sm", Ls, Ls) - np.sum(kf * sol[:, 1:], axis=0).reshape(S, M) + sig2
        var[:, h] = np.where(v <= 0, PRECISION, v)
    return mean, var, out_star


# ---- the restatement against the reference's recorded runs ---------------------------------------------------------------
def check_family(g, pars, z, loc, scale, constrained, M):
    T = M * (M + 1) // 2
    mean, var, star = restate(g["x"], g["Y"], pars, g["hyper"], g["xs"], z[:, :, :1 + T], constrained)
    want = loc[:, :, :1 + T] + scale[:, :, :1 + T] * z[:, :, :1 + T]       # the reference's sampled latent values
    if not constrained:
        want[:, :, 1 + diag_slots(M)] = np.exp(want[:, :, 1 + diag_slots(M)])
    np.testing.assert_allclose(star, want, **STAR_TOL)
    np.testing.assert_allclose(mean, loc[:, :, 1 + T:], **MEAN_TOL)
    np.testing.assert_allclose(var, scale[:, :, 1 + T:] ** 2, **VAR_TOL)
    return mean + np.sqrt(var) * z[:, :, 1 + T:]


@pytest.mark.parametrize("name", ["predsample_N64_M3", "predsample_N512_M3"])
def test_restatement_reproduces_the_predsample_family(name):
    g = golden(name)
    M = g["Y"].shape[1]
    ys = check_family(g, g["draws"], g["ps_z"], g["ps_loc"], g["ps_scale"], True, M)
    np.testing.assert_allclose(ys, g["ps_y"], **MEAN_TOL)


def test_restatement_reproduces_the_sampling_family():
    g = golden("predsample_N64_M3")
    M = g["Y"].shape[1]
    T = M * (M + 1) // 2
    n = int(g["sm_n_sample"])
    pars = np.repeat(g["sm_pars"][None], n, axis=0)                 # one parameter vector, n noise draws per grid point
    ys = check_family(g, pars, g["sm_z"], g["sm_loc"], g["sm_scale"], False, M)
    np.testing.assert_allclose(np.percentile(ys, q=[2.5, 97.5], axis=1).transpose(1, 0, 2), g["sm_q"], **MEAN_TOL)
    np.testing.assert_allclose(ys.mean(axis=1), g["sm_mean"], **MEAN_TOL)
    np.testing.assert_allclose(ys.std(axis=1), g["sm_std"], rtol=1e-5, atol=1e-7)
    z = np.zeros((len(g["xs"]), n, 1 + T))
    z[:, :, :1] = g["sm_z_smooth"]
    np.testing.assert_allclose(restate(g["x"], g["Y"], pars, g["hyper"], g["xs"], z, False)[2][:, :, 0], g["sm_tl"], **STAR_TOL)
    z = np.zeros((len(g["xs"]), n, 1 + T))
    z[:, :, 1:] = g["sm_z_cov"]
    star = restate(g["x"], g["Y"], pars, g["hyper"], g["xs"], z, False)[2]
    np.testing.assert_allclose(tril_from_vec(star[:, :, 1:], M), g["sm_Lf"], **STAR_TOL)


def test_fixtures_are_small_and_clip_free():
    for name in ("predsample_N64_M3", "predsample_N512_M3"):
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) < 1 << 20
        g = golden(name)
        T = g["Y"].shape[1] * (g["Y"].shape[1] + 1) // 2
        assert (g["ps_scale"][:, :, 1 + T:] ** 2).min() > 10 * PRECISION
        assert (g["ps_scale"][:, :, :1 + T] ** 2).min() > 1.0000001 * PRECISION


# ---- the summary of drivers.posterior_predict -----------------------------------------------------------------------------
def test_summary_is_the_hand_computed_mixture():
    from nonstationary_multivariate_gaussian_process_amd.drivers import summarize_posterior_predictive
    # 4 draws (one of them failed), S = 2, M = 1
    mean = np.array([[[1.0], [0.0]], [[3.0], [2.0]], [[np.nan], [np.nan]], [[2.0], [4.0]]])
    var = np.array([[[0.5], [1.0]], [[1.5], [1.0]], [[np.nan], [np.nan]], [[1.0], [4.0]]])
    ys = np.array([[[0.0], [1.0]], [[4.0], [2.0]], [[np.nan], [np.nan]], [[2.0], [9.0]]])
    tl = np.arange(8.0).reshape(4, 2)
    status = np.array([0, 0, 17, 0])
    s = summarize_posterior_predictive(mean, var, ys, tl, status)
    assert s["n_used"] == 3 and s["n_failed"] == 1 and s["status"].tolist() == [0, 0, 17, 0]
    np.testing.assert_allclose(s["mean"], [[2.0], [2.0]], rtol=0, atol=1e-15)
    # law of total variance: mean of the variances + (population) variance of the means
    np.testing.assert_allclose(s["var"], [[1.0 + 2.0 / 3.0], [2.0 + 8.0 / 3.0]], rtol=1e-15)
    np.testing.assert_allclose(s["quantiles"][1], [[2.0], [2.0]], rtol=0, atol=1e-15)          # medians of (0, 4, 2) and (1, 2, 9)
    np.testing.assert_allclose(s["quantiles"][0], [[0.1], [1.05]], rtol=1e-14)                 # 2.5 %: linear interpolation
    np.testing.assert_allclose(s["quantiles"][2], [[3.9], [8.65]], rtol=1e-14)
    assert s["tilde_l_star"].tolist() == [[0.0, 1.0], [2.0, 3.0], [6.0, 7.0]]
    with pytest.raises(RuntimeError, match="no posterior draw"):
        summarize_posterior_predictive(mean, var, ys, tl, np.array([1, 2, 3, 4]))


# ---- name resolution ---------------------------------------------------------------------------------------------
RESOLVE = textwrap.dedent('''
    import inspect, os, sys
    sys.dont_write_bytecode = True
    sys.path.insert(0, {root!r})
    import nonstationary_multivariate_gaussian_process_amd as nmgp_amd
    nmgp_amd.install_utility_alias(reference_utility_dir={refutil!r})
    from Utility import prediction
    pkg = os.path.join({root!r}, "nonstationary_multivariate_gaussian_process_amd")
    def where(obj):
        return os.path.dirname(os.path.abspath(inspect.getsourcefile(obj)))
    got = [where(getattr(prediction, n)) for n in ("pointwise_predsample_inhomogeneous", "test_predmap_inhomogeneous_sampling")]
    want = pkg if sys.argv[1] == "on" else {refutil!r}
    assert got == [want, want], (got, want)
    if sys.argv[1] == "on":
        for n in ("point_predsample_inhomogeneous", "test_predsample_inhomogeneous", "point_predmap_inhomogeneous_sampling",
                  "pointwise_predmap_inhomogeneous_sampling"):
            assert where(getattr(prediction, n)) == pkg, n
    assert where(prediction.pointwise_predmap_inhomogeneous) == os.path.join(pkg, "Utility")      # unchanged either way
    assert where(prediction.vec2pars) == {refutil!r}
    print("RESOLVE-OK", sys.argv[1])
''')


@pytest.mark.parametrize("mode", ["on", "off"])
def test_the_new_names_are_opt_in_behind_the_references_module(mode, tmp_path):
    util = tmp_path / "Utility"
    util.mkdir()
    (util / "__init__.py").write_text("")
    (util / "logpos.py").write_text("def nlogpos_obj_hadamard_SVC(*args):\n    return 0.0\n")
    (util / "prediction.py").write_text("".join("def %s(*args):\n    return args\n\n\n" % f for f in (
        "vec2pars", "pointwise_predsample_inhomogeneous", "test_predmap_inhomogeneous_sampling")))
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    env.pop("NMGP_REFERENCE_UTILITY", None)
    env.pop("NMGP_PREDSAMPLE", None)
    if mode == "on":
        env["NMGP_PREDSAMPLE"] = "1"
    r = subprocess.run([sys.executable, "-c", RESOLVE.format(root=ROOT, refutil=str(util)), mode], cwd=str(tmp_path), env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "RESOLVE-OK" in r.stdout, r.stdout + r.stderr


def test_module_signatures_follow_the_reference():
    import inspect
    from nonstationary_multivariate_gaussian_process_amd import predsample as ps
    hyp = ["mu_tilde_l", "alpha_tilde_l", "beta_tilde_l", "mu_L", "alpha_L", "beta_L"]
    hist = ["tilde_l_hist", "uL_vecs_hist", "tilde_sigma2_err_hist", "Y", "x"]
    one = ["n_sample", "tilde_l", "uL_vecs", "tilde_sigma2_err", "Y", "x"]
    want = {"point_predsample_inhomogeneous": hist + ["x_star"] + hyp + ["N_sample"],
            "pointwise_predsample_inhomogeneous": hist + ["grids"] + hyp + ["N_sample"],
            "test_predsample_inhomogeneous": hist + ["x_test"] + hyp + ["N_sample"],
            "point_predmap_inhomogeneous_sampling": one + ["x_star"] + hyp + ["pred_smoothness", "pred_cov"],
            "pointwise_predmap_inhomogeneous_sampling": one + ["grids"] + hyp + ["pred_smoothness", "pred_cov"],
            "test_predmap_inhomogeneous_sampling": one + ["x_test"] + hyp}
    assert sorted(want) == sorted(ps.NAMES)
    for name, names in want.items():
        prm = inspect.signature(getattr(ps, name)).parameters
        pos = [k for k, v in prm.items() if v.kind == v.POSITIONAL_OR_KEYWORD]
        assert pos == names, (name, pos)
        assert prm["z"].kind == prm["z"].KEYWORD_ONLY and prm["z"].default is None
        for k in ("pred_smoothness", "pred_cov"):
            if k in prm:
                assert prm[k].default is False
