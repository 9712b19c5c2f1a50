"""CPU-only checks of the posterior-draw prediction of the separable Hadamard model: a NumPy restatement of the reference's two
sampling forms (``point_predsample_hadamard`` prediction.py:461-553, all outputs at a new input; ``indexedpoint_predsample_hadamard``
:585-676, one output) held against the fixtures tests/golden/hps_*.npz that tests/golden/make_golden_predsample_hadamard.py
produced by running the reference with a recorded normal stream; the mirror's names, signatures and opt-in; the summary of [H, S]
moments.  tests/test_gpu_predsample_hadamard.py imports the restatement from here.

Bar of the restatement against the recorded runs: 1e-8 relative, element by element (conftest.relerr), on loc, scale and samples.
Both sides are float64 NumPy / torch on well-conditioned covariances (cond(S) <= 2e4); the GP-prior solves (cond ~ 1e8) enter
through the starred values only, where both sides use the same LU solve."""
import inspect
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
from scipy.linalg import cho_solve, cholesky, solve_triangular

from conftest import ROOT, golden, golden_names, relerr

CASES = golden_names("hps_N")
JITTER, PRECISION = 1e-6, 1e-6
RESTATE_TOL = 1e-8


# ---- the two sampling forms, restated -----------------------------------------------------------------------------------
def rbf(x1, x2, alpha, beta):
    a, b = x1 / beta, x2 / beta
    dist = (a ** 2)[:, None] + (b ** 2)[None, :] - 2.0 * a[:, None] * b[None, :]
    return np.exp(-0.5 * dist) * alpha ** 2


def gibbs(x1, s1, l1, x2, s2, l2):
    dist = (x1 ** 2)[:, None] + (x2 ** 2)[None, :] - 2.0 * x1[:, None] * x2[None, :]
    A = (l1 ** 2)[:, None] + (l2 ** 2)[None, :]
    return (s1[:, None] * s2[None, :]) * np.sqrt(2.0 * l1[:, None] * l2[None, :] / A) * np.exp(-dist / A)


def regression(x, xs, alpha, beta):
    """proj [N, S] = Sigma^-1 k (the reference's proj-first order, LU) and the clipped conditional variances [S]."""
    Sig = rbf(x, x, alpha, beta) + JITTER * np.eye(len(x))
    k = rbf(x, xs, alpha, beta)
    proj = np.linalg.solve(Sig, k)
    cv = (alpha ** 2 + JITTER) - np.sum(proj * k, axis=0)
    return proj, np.where(cv < 0, PRECISION, cv)


def tril(L_vec, M):
    L = np.zeros((M, M))
    L[np.tril_indices(M)] = L_vec                 # the slots as they are: no exp
    return L


def restate_hps(x, indx, y, draws, hyper, xs, z, indx_star=None):
    """draws [H, 2N+T+1], xs [S], z [S, H, 2 + K] (K = M, or 1 with indx_star [S]) in the reference's consumption order ->
    loc, scale, samples, each [S, H, 2 + K]: (tilde_l*, tilde_sigma*, y)."""
    x, y, xs = (np.asarray(v, dtype=np.float64) for v in (x, y, xs))
    indx = np.asarray(indx).astype(np.int64)
    N, M = x.shape[0], int(np.unique(indx).shape[0])
    T = M * (M + 1) // 2
    mu_l, al_l, be_l, mu_s, al_s, be_s = [float(v) for v in hyper[:6]]
    S, H = xs.shape[0], draws.shape[0]
    K = M if indx_star is None else 1
    proj_l, cv_l = regression(x, xs, al_l, be_l)
    proj_s, cv_s = regression(x, xs, al_s, be_s)
    loc, scale = np.zeros((S, H, 2 + K)), np.zeros((S, H, 2 + K))
    for h in range(H):
        p = draws[h]
        tl, ts, Lv, s2e = p[:N], p[N:2 * N], p[2 * N:2 * N + T], float(np.exp(p[-1]))
        ell, sig = np.exp(tl), np.exp(ts)
        B_f = tril(Lv, M) @ tril(Lv, M).T
        Kx = gibbs(x, sig, ell, x, sig, ell) + JITTER * np.eye(N)
        C = cholesky(Kx * B_f[indx][:, indx] + s2e * np.eye(N), lower=True)      # the reference goes through symeig
        alpha = cho_solve((C, True), y)
        loc[:, h, 0] = mu_l + proj_l.T @ (tl - mu_l)
        loc[:, h, 1] = mu_s + proj_s.T @ (ts - mu_s)
        scale[:, h, 0], scale[:, h, 1] = np.sqrt(cv_l), np.sqrt(cv_s)
        star = loc[:, h, :2] + scale[:, h, :2] * z[:, h, :2]
        for s in range(S):
            ls, ss = np.exp(star[s, 0]), np.exp(star[s, 1])
            kx = gibbs(x, sig, ell, xs[s:s + 1], np.array([ss]), np.array([ls]))[:, 0]      # no jitter on the cross term
            ms = np.arange(M) if indx_star is None else np.array([int(indx_star[s])])
            kf = kx[:, None] * B_f[indx][:, ms]                                            # [N, K]
            V = solve_triangular(C, kf, lower=True)
            var = B_f[ms, ms] * (ss * ss + JITTER) - (V * V).sum(0) + s2e                   # the jitter sits inside the prior term
            loc[s, h, 2:] = kf.T @ alpha
            scale[s, h, 2:] = np.sqrt(np.where(var <= 0, PRECISION, var))
    return loc, scale, loc + scale * z


def test_fixture_set_is_complete():
    assert CASES == ["hps_N200_M4", "hps_N77_M3"]
    for n, H in (("hps_N77_M3", 6), ("hps_N200_M4", 4)):
        g = golden(n)
        N, M = g["x"].shape[0], int(g["M"])
        h = golden("hsep" + n[3:])
        assert all(np.array_equal(g[k], h[k]) for k in ("x", "indx", "y", "hyper", "grids")) and np.array_equal(g["draws"][0], h["pars"])
        assert g["draws"].shape == (H, 2 * N + M * (M + 1) // 2 + 1) and g["grids"].shape == (9,)
        assert g["ps_z"].shape == g["ps_loc"].shape == g["ps_scale"].shape == (9, H, 2 + M) and g["ps_y"].shape == (9, H, M)
        St = g["x_test"].shape[0]
        assert 5 <= St <= 6 and sorted(np.unique(g["indx_test"]).tolist()) == list(range(M))
        assert g["ix_z"].shape == g["ix_loc"].shape == g["ix_scale"].shape == (St, H, 3) and g["ix_y"].shape == (St, H)
        assert g["map_pct"].shape == (St, 3)
        assert np.any(np.isin(g["grids"], g["x"])) and np.any(np.isin(g["x_test"], g["x"]))          # one observed x in each
        assert g["grids"].min() < g["x"].min() and g["grids"].max() > g["x"].max()
    assert int((golden("hps_N77_M3")["indx"] == 2).sum()) == 2                # the rare label: 2 observations of 77


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_recorded_runs(name):
    g = golden(name)
    loc, scale, ys = restate_hps(g["x"], g["indx"], g["y"], g["draws"], g["hyper"], g["grids"], g["ps_z"])
    errs = dict(loc=relerr(loc, g["ps_loc"]), scale=relerr(scale, g["ps_scale"]), y=relerr(ys[:, :, 2:], g["ps_y"]))
    iloc, iscale, iy = restate_hps(g["x"], g["indx"], g["y"], g["draws"], g["hyper"], g["x_test"], g["ix_z"], g["indx_test"])
    errs.update(ix_loc=relerr(iloc, g["ix_loc"]), ix_scale=relerr(iscale, g["ix_scale"]), ix_y=relerr(iy[:, :, 2], g["ix_y"]))
    # the MAP forms of the indexed predictor: draws[0], no noise
    mloc, mscale, _ = restate_hps(g["x"], g["indx"], g["y"], g["draws"][:1], g["hyper"], g["x_test"], np.zeros((len(g["x_test"]), 1, 3)),
                                  g["indx_test"])
    m, sd = mloc[:, 0, 2], mscale[:, 0, 2]
    errs["map_pct"] = relerr(np.stack([m - 1.96 * sd, m, m + 1.96 * sd], axis=1), g["map_pct"])
    print(name, errs)
    for k, e in errs.items():
        assert e < RESTATE_TOL, (name, k, e)
    # the indexed form is column indx* of the full form under the same starred values
    St = len(g["x_test"])
    zf = np.concatenate([g["ix_z"][:, :, :2], np.zeros((St, g["draws"].shape[0], int(g["M"])))], axis=2)
    floc, fscale, _ = restate_hps(g["x"], g["indx"], g["y"], g["draws"], g["hyper"], g["x_test"], zf)
    pick = 2 + g["indx_test"].astype(np.int64)
    assert relerr(floc[np.arange(St), :, pick], iloc[:, :, 2]) < 1e-12 and relerr(fscale[np.arange(St), :, pick], iscale[:, :, 2]) < 1e-12


# ---- names, signatures, opt-in -------------------------------------------------------------------------------------------
HYP = ["mu_tilde_l", "alpha_tilde_l", "beta_tilde_l", "mu_tilde_sigma", "alpha_tilde_sigma", "beta_tilde_sigma"]
HIST = ["tilde_l_hist", "tilde_sigma_hist", "L_vec_hist", "tilde_sigma2_err_hist", "x", "indx", "y"]
PIECES = ["tilde_l", "tilde_sigma", "L_vec", "tilde_sigma2_err", "x", "indx", "y"]
SIGNATURES = {                                      # the reference's positional parameters (prediction.py:461, :555, :585, :678, :810, :887)
    "point_predsample_hadamard": HIST + ["x_star"] + HYP,
    "pointwise_predsample_hadamard": HIST + ["grids"] + HYP,
    "indexedpoint_predsample_hadamard": HIST + ["x_star", "indx_star"] + HYP,
    "test_predsample_hadamard": HIST + ["x_test", "indx_test"] + HYP,
    "indexedpoint_predmap_hadamard": PIECES + ["x_star", "indx_star"] + HYP,
    "test_predmap_harmard": PIECES + ["x_test", "indx_test"] + HYP,
}
SAMPLING = [n for n in SIGNATURES if "predsample" in n]


def test_module_signatures_follow_the_reference():
    from nonstationary_multivariate_gaussian_process_amd import hadamard, hadamard_sep, predsample, predsample_hadamard as psh, predsample_sep
    for fn, params in SIGNATURES.items():
        sig = inspect.signature(getattr(psh, fn))
        extra = ("args", "kwargs", "z")
        assert [p for p in sig.parameters if p not in extra] == params, fn
        for k, p in sig.parameters.items():
            if k not in ("args", "kwargs"):
                assert p.default is (None if k == "z" else inspect.Parameter.empty), (fn, k)       # the reference has no defaults
        kinds = {k: p.kind for k, p in sig.parameters.items()}
        assert kinds["args"] == inspect.Parameter.VAR_POSITIONAL and kinds["kwargs"] == inspect.Parameter.VAR_KEYWORD
        assert ("z" in kinds) == (fn in SAMPLING)
        if fn in SAMPLING:
            assert kinds["z"] == inspect.Parameter.KEYWORD_ONLY
        assert "N_sample" not in kinds
    assert psh.test_predmap_hadamard is psh.test_predmap_harmard
    assert set(psh.NAMES) == set(SIGNATURES) | {"test_predmap_hadamard"}
    for fn in ("test_predsample_hadamard", "test_predmap_harmard", "test_predmap_hadamard"):
        assert getattr(psh, fn).__test__ is False
    # the other modules' tuples are not extended
    others = set(hadamard.PREDICTION_NAMES) | set(hadamard_sep.PREDICTION_NAMES) | set(predsample.NAMES) | set(predsample_sep.NAMES)
    assert not set(psh.NAMES) & others
    assert hadamard_sep.PREDICTION_NAMES == ("point_predmap_hadamard", "pointwise_predmap_hadmard", "pointwise_predmap_hadamard")


RESOLVE = textwrap.dedent('''
    import inspect, os, sys
    sys.path.insert(0, {root!r})
    import nonstationary_multivariate_gaussian_process_amd as nmgp_amd
    nmgp_amd.install_utility_alias(reference_utility_dir={refutil!r})
    from Utility import prediction
    pkg = os.path.join({root!r}, "nonstationary_multivariate_gaussian_process_amd")
    def where(obj):
        return os.path.dirname(os.path.abspath(inspect.getsourcefile(obj)))
    names = {names!r}
    want = pkg if sys.argv[1] == "on" else {refutil!r}
    served = [where(getattr(prediction, n)) for n in names]
    assert served == [want] * len(names), (served, want)
    if sys.argv[1] == "on":
        from nonstationary_multivariate_gaussian_process_amd import predsample_hadamard
        for n in names:
            assert getattr(prediction, n) is getattr(predsample_hadamard, n), n
        assert prediction.test_predmap_hadamard is predsample_hadamard.test_predmap_harmard
    # not this module's: the stationary variant keeps resolving to the checkout, the MAP predictor follows its own switch
    assert where(prediction.pointwise_predsample_hadamard_S) == {refutil!r}
    assert where(prediction.point_predmap_hadamard) == (pkg if sys.argv[1] == "NMGP_HADAMARD_SEP" else {refutil!r})
    assert where(prediction.point_predmap_inhomogeneous) == os.path.join(pkg, "Utility")      # unchanged either way
    print("RESOLVE-OK", sys.argv[1])
''')


@pytest.mark.parametrize("mode", ["on", "off", "NMGP_HADAMARD", "NMGP_HADAMARD_SEP", "NMGP_PREDSAMPLE"])
def test_the_names_are_opt_in_behind_a_switch_of_their_own(mode, tmp_path):
    """on: NMGP_PREDSAMPLE_HADAMARD=1 serves the seven names; off: nothing set; each of the other three switches alone does not."""
    from nonstationary_multivariate_gaussian_process_amd import predsample_hadamard as psh
    util = tmp_path / "Utility"
    util.mkdir()
    (util / "__init__.py").write_text("")
    stub = "def %s(*args):\n    return args\n\n\n"
    (util / "logpos.py").write_text(stub % "nlogpos_obj_hadamard")
    (util / "prediction.py").write_text("".join(stub % f for f in psh.NAMES + ("pointwise_predsample_hadamard_S", "point_predmap_hadamard")))
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    for k in ("NMGP_REFERENCE_UTILITY", "NMGP_HADAMARD", "NMGP_HADAMARD_SEP", "NMGP_PREDSAMPLE", "NMGP_PREDSAMPLE_HADAMARD"):
        env.pop(k, None)
    if mode == "on":
        env["NMGP_PREDSAMPLE_HADAMARD"] = "1"
    elif mode != "off":
        env[mode] = "1"
    r = subprocess.run([sys.executable, "-c", RESOLVE.format(root=ROOT, refutil=str(util), names=psh.NAMES), mode], cwd=str(tmp_path),
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "RESOLVE-OK" in r.stdout, r.stdout + r.stderr


def test_abi_declares_and_binds_the_entry():
    from nonstationary_multivariate_gaussian_process_amd import _lib, build, drivers
    header = open(os.path.join(ROOT, "include", "nmgp.h")).read()
    assert "nmgp_predsample_hads" in _lib.SIGNATURES and "int nmgp_predsample_hads(" in header
    assert len(_lib.SIGNATURES["nmgp_predsample_hads"][1]) == 13
    assert list(inspect.signature(_lib.Context.predsample_hads).parameters) == ["self", "pars_hist", "hyper", "xs", "indx_star", "z", "star"]
    assert "nmgp_predsample_hadamard.hip" in build.SOURCES
    sig = inspect.signature(drivers.posterior_predict_hadamard_sep)
    assert list(sig.parameters) == ["x", "indx", "y", "hyper_pars", "samples", "xs", "indx_star", "draws", "seed", "ctx"]
    assert [sig.parameters[k].default for k in ("indx_star", "draws", "seed", "ctx")] == [None, None, 0, None]


# ---- the summary ------------------------------------------------------------------------------------------------------------
def test_summary_takes_moments_without_an_output_axis():
    from nonstationary_multivariate_gaussian_process_amd.drivers import summarize_posterior_predictive
    rng = np.random.default_rng(3)
    H, S, M = 10, 7, 3
    status = np.zeros(H, dtype=np.int32)
    status[4] = 17
    ok = status == 0
    for shape in ((H, S), (H, S, M)):
        mean, var = rng.standard_normal(shape), rng.uniform(0.1, 2.0, shape)
        ys = mean + np.sqrt(var) * rng.standard_normal(shape)
        star = rng.standard_normal((H, S))
        mean[4] = var[4] = np.nan
        out = summarize_posterior_predictive(mean, var, ys, star, status)
        assert out["mean"].shape == out["var"].shape == shape[1:] and out["quantiles"].shape == (3,) + shape[1:]
        assert out["n_used"] == 9 and out["n_failed"] == 1 and out["status"].tolist() == status.tolist()
        np.testing.assert_allclose(out["mean"], mean[ok].mean(axis=0), rtol=1e-15)
        np.testing.assert_allclose(out["var"], var[ok].mean(axis=0) + mean[ok].var(axis=0), rtol=1e-15)
        np.testing.assert_allclose(out["quantiles"], np.percentile(ys[ok], [2.5, 50.0, 97.5], axis=0), rtol=1e-15)
        assert np.array_equal(out["tilde_l_star"], star[ok]) and np.all(np.isfinite(out["var"]))
