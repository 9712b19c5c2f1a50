"""Posterior-draw prediction of the separable and the stationary model without a GPU: a NumPy restatement of what the reference
computes (prediction.py:34-334 and :1640-1692, with their quirks) in the Cholesky block formulation of the device entry, against
the fixtures recorded from the reference (tests/golden/make_golden_predsample_sep.py); the signatures of ``predsample_sep``; the
opt-in name resolution of ``Utility.prediction``; the summary of ``drivers.posterior_predict_separable``.

``restate_sep`` / ``restate_sta`` are also what the GPU tests compare the device entries with where no fixture exists.
Bars: those of test_predsample_cpu.py."""
import inspect
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from conftest import golden
from test_predsample_cpu import JITTER, MEAN_TOL, PRECISION, STAR_TOL, VAR_TOL, gibbs, regression, rbf, tril_from_vec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ("predsample_sep_N64_M3", "predsample_sep_N512_M5")


# ---- the restatement -----------------------------------------------------------------------------------------------
def b_eig(uL, M):
    """B = L L^T from the unconstrained packed tril vector (exp on the diagonal slots) and its eigenpairs."""
    L = tril_from_vec(np.asarray(uL, dtype=np.float64), M)
    L[np.arange(M), np.arange(M)] = np.exp(np.diag(L))
    B = L @ L.T
    w, V = np.linalg.eigh(B)
    return B, w, V


def block_moments(Kx, kx, Y, B, w, V, sig2, kss, strict):
    """Sigma = B kron Kx + sig2 I in B's eigenbasis: M blocks w_p Kx + sig2 I, each factored once, the rotated data and the
    cross-covariance vectors kx [N, S] solved against the factor.  Returns mean, var [S, M]."""
    N, S = kx.shape
    M = B.shape[0]
    yt = Y @ V                                                      # [N, M]: column p = sum_m V[m, p] Y[:, m]
    mean, vf = np.zeros((S, M)), np.zeros((S, M))
    for p in range(M):
        Lp = np.linalg.cholesky(w[p] * Kx + sig2 * np.eye(N))
        sol = np.linalg.solve(Lp, np.concatenate([yt[:, p:p + 1], kx], axis=1))
        a, r = sol[:, 0], sol[:, 1:]
        am = w[p] * V[:, p]                                         # [M]
        mean += np.outer(r.T @ a, am)
        vf += np.outer(np.sum(r * r, axis=0), am ** 2)
    v = (kss[:, None] * np.diag(B)[None, :] - vf) + sig2
    return mean, np.where((v < 0) if strict else (v <= 0), PRECISION, v)


def restate_sep(x, Y, pars, hyper, xs, z=None, kss_jitter=True, star=None):
    """pars [H, 2N+T+1], xs [S], z [S, H, 2] or None (zeros), star [S, H, 2] or None (regress).
    Returns mean, var [S, H, M] and the starred values [S, H, 2] (tilde_l*, tilde_sigma*, before exp)."""
    x, Y, pars, xs = (np.asarray(a, dtype=np.float64) for a in (x, Y, pars, xs))
    N, M = Y.shape
    T = M * (M + 1) // 2
    H, S = pars.shape[0], xs.shape[0]
    mu_l, al_l, be_l, mu_s, al_s, be_s = [float(v) for v in hyper[:6]]
    if star is None:
        proj_l, cv_l = regression(x, xs, al_l, be_l)
        proj_s, cv_s = regression(x, xs, al_s, be_s)
        z = np.zeros((S, H, 2)) if z is None else np.asarray(z, dtype=np.float64)
    mean, var, out_star = np.empty((S, H, M)), np.empty((S, H, M)), np.empty((S, H, 2))
    for h in range(H):
        tl, ts, uL, tse = pars[h, :N], pars[h, N:2 * N], pars[h, 2 * N:2 * N + T], pars[h, -1]
        if star is None:
            st = np.stack([mu_l + proj_l.T @ (tl - mu_l) + np.sqrt(cv_l) * z[:, h, 0],
                           mu_s + proj_s.T @ (ts - mu_s) + np.sqrt(cv_s) * z[:, h, 1]], axis=1)
        else:
            st = np.asarray(star, dtype=np.float64)[:, h]
        out_star[:, h] = st
        ell, sig = np.exp(tl), np.exp(ts)
        ls, ss = np.exp(st[:, 0]), np.exp(st[:, 1])
        Kx = np.outer(sig, sig) * gibbs(x, ell, x, ell) + JITTER * np.eye(N)
        kx = sig[:, None] * ss[None, :] * gibbs(x, ell, xs, ls)
        B, w, V = b_eig(uL, M)
        kss = ss ** 2 + (JITTER if kss_jitter else 0.0)
        mean[:, h], var[:, h] = block_moments(Kx, kx, Y, B, w, V, np.exp(tse), kss, False)
    return mean, var, out_star


def restate_sta(x, Y, pars, xs):
    """pars [H, T+3], xs [S] -> mean, var [H, S, M] (draw-major, as the stationary functions return)."""
    x, Y, pars, xs = (np.asarray(a, dtype=np.float64) for a in (x, Y, pars, xs))
    N, M = Y.shape
    T = M * (M + 1) // 2
    H, S = pars.shape[0], xs.shape[0]
    mean, var = np.empty((H, S, M)), np.empty((H, S, M))
    for h in range(H):
        l0, sig0 = np.exp(pars[h, 0]), np.exp(pars[h, 1])
        Kx = rbf(x, x, sig0, l0) + JITTER * np.eye(N)
        B, w, V = b_eig(pars[h, 2:2 + T], M)
        mean[h], var[h] = block_moments(Kx, rbf(x, xs, sig0, l0), Y, B, w, V, np.exp(pars[h, -1]), np.full(S, sig0 ** 2), True)
    return mean, var


def relmax(a, b, floor=0.0):
    return float(np.max(np.abs(a - b) / (np.abs(b) + floor)))


# ---- the restatement against the reference's recorded runs ---------------------------------------------------------------
def check_family(g, pars, z, loc, scale, kss_jitter):
    mean, var, star = restate_sep(g["x"], g["Y"], pars, g["hyper"], g["xs"], z[:, :, :2], kss_jitter)
    want = loc[:, :, :2] + scale[:, :, :2] * z[:, :, :2]                  # the reference's sampled latent values
    print("restatement: mean", relmax(mean, loc[:, :, 2:], 1e-2), "var", relmax(var, scale[:, :, 2:] ** 2), "star abs",
          float(np.max(np.abs(star - want))))
    np.testing.assert_allclose(star, want, **STAR_TOL)
    np.testing.assert_allclose(mean, loc[:, :, 2:], **MEAN_TOL)
    np.testing.assert_allclose(var, scale[:, :, 2:] ** 2, **VAR_TOL)
    return mean + np.sqrt(var) * z[:, :, 2:]


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_reproduces_the_predsample_family(name):
    g = golden(name)
    ys = check_family(g, g["draws"], g["ps_z"], g["ps_loc"], g["ps_scale"], True)
    np.testing.assert_allclose(ys, g["ps_y"], **MEAN_TOL)
    # the fixture discriminates the quirk: without the jitter in a2 the variance misses the bar
    var = restate_sep(g["x"], g["Y"], g["draws"], g["hyper"], g["xs"], g["ps_z"][:, :, :2], False)[1]
    assert not np.allclose(var, g["ps_scale"][:, :, 2:] ** 2, **VAR_TOL)


def test_restatement_reproduces_the_sampling_family():
    g = golden("predsample_sep_N64_M3")
    n = int(g["sm_n_sample"])
    pars = np.repeat(g["sm_pars"][None], n, axis=0)                 # one parameter vector, n noise draws per grid point
    ys = check_family(g, pars, g["sm_z"], g["sm_loc"], g["sm_scale"], False)
    np.testing.assert_allclose(np.percentile(ys, q=[2.5, 97.5], axis=1).transpose(1, 0, 2), g["sm_q"], **MEAN_TOL)
    np.testing.assert_allclose(ys.mean(axis=1), g["sm_mean"], **MEAN_TOL)
    np.testing.assert_allclose(ys.std(axis=1), g["sm_std"], rtol=1e-5, atol=1e-7)
    var = restate_sep(g["x"], g["Y"], pars, g["hyper"], g["xs"], g["sm_z"][:, :, :2], True)[1]
    assert not np.allclose(var, g["sm_scale"][:, :, 2:] ** 2, **VAR_TOL)


def test_restatement_reproduces_the_stationary_family():
    g = golden("predsample_sep_N64_M3")
    mean, var = restate_sta(g["x"], g["Y"], g["sta_draws"], g["xs"])
    print("restatement (stationary): mean", relmax(mean, g["sta_mean"], 1e-2), "var", relmax(var, g["sta_sd"] ** 2))
    np.testing.assert_allclose(mean, g["sta_mean"], **MEAN_TOL)
    np.testing.assert_allclose(var, g["sta_sd"] ** 2, **VAR_TOL)
    np.testing.assert_allclose(mean + g["sta_z"][:, :, None] * np.sqrt(var), g["sta_y"], **MEAN_TOL)
    # np.random.standard_normal((H, S)) is the stream of H S successive np.random.randn() calls: the seeded run of the reference
    np.random.seed(int(g["sta_seed"]))
    zz = np.random.standard_normal(g["sta_z"].shape)
    np.testing.assert_allclose(mean + zz[:, :, None] * np.sqrt(var), g["sta_y_seeded"], **MEAN_TOL)


def test_fixtures_are_small_and_clip_free():
    for name in FIXTURES:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) < 1 << 20
        g = golden(name)
        assert (g["ps_scale"][:, :, 2:] ** 2).min() > 10 * PRECISION
        assert (g["ps_scale"][:, :, :2] ** 2).min() > 1.0000001 * PRECISION
    g = golden("predsample_sep_N64_M3")
    assert (g["sm_scale"][:, :, 2:] ** 2).min() > 10 * PRECISION and (g["sm_scale"][:, :, :2] ** 2).min() > 1.0000001 * PRECISION
    assert (g["sta_sd"] ** 2).min() > 10 * PRECISION and np.all(np.isfinite(g["sta_y"]))


# ---- signatures -----------------------------------------------------------------------------------------------------
def test_module_signatures_follow_the_reference():
    from nonstationary_multivariate_gaussian_process_amd import predsample as ps0
    from nonstationary_multivariate_gaussian_process_amd import predsample_sep as ps
    hyp = ["mu_tilde_l", "alpha_tilde_l", "beta_tilde_l", "mu_tilde_sigma", "alpha_tilde_sigma", "beta_tilde_sigma"]
    hist = ["tilde_l_hist", "tilde_sigma_hist", "uL_vec_hist", "tilde_sigma2_err_hist", "Y", "x"]
    one = ["n_sample", "tilde_l", "tilde_sigma", "uL_vec", "tilde_sigma2_err", "Y", "x"]
    sta = ["tilde_ls", "tilde_sigmas", "uL_vecs", "tilde_sigma2_errs", "Y", "x"]
    want = {"point_predsample": hist + ["x_star"] + hyp + ["N_sample"],
            "pointwise_predsample": hist + ["grids"] + hyp + ["N_sample"],
            "test_predsample": hist + ["x_test"] + hyp + ["N_sample"],
            "point_predmap_sampling": one + ["x_star"] + hyp,
            "pointwise_predmap_sampling": one + ["grids"] + hyp,
            "test_predmap_sampling": one + ["x_test"] + hyp,
            "pointwise_predsample_S": sta + ["grids"],
            "test_predsample_S": sta + ["test_x"]}
    assert sorted(want) == sorted(ps.NAMES)
    assert not set(ps.NAMES) & set(ps0.NAMES)
    for name, names in want.items():
        prm = inspect.signature(getattr(ps, name)).parameters
        pos = [k for k, v in prm.items() if v.kind == v.POSITIONAL_OR_KEYWORD]
        assert pos == names, (name, pos)
        assert prm["z"].kind == prm["z"].KEYWORD_ONLY and prm["z"].default is None
        assert any(v.kind == v.VAR_POSITIONAL for v in prm.values()) and any(v.kind == v.VAR_KEYWORD for v in prm.values())


# ---- name resolution ---------------------------------------------------------------------------------------------
RESOLVE = textwrap.dedent('''
    import inspect, os, sys
    sys.dont_write_bytecode = True
    sys.path.insert(0, {root!r})
    import nonstationary_multivariate_gaussian_process_amd as nmgp_amd
    nmgp_amd.install_utility_alias(reference_utility_dir={refutil!r})
    from Utility import prediction
    pkg = os.path.join({root!r}, "nonstationary_multivariate_gaussian_process_amd")
    names = {names!r}
    def where(obj):
        return os.path.dirname(os.path.abspath(inspect.getsourcefile(obj)))
    want = pkg if sys.argv[1] == "on" else {refutil!r}
    for n in names:
        assert where(getattr(prediction, n)) == want, (n, where(getattr(prediction, n)), want)
    assert where(prediction.pointwise_predmap) == os.path.join(pkg, "Utility")      # unchanged either way
    assert where(prediction.pointwise_predmap_S) == os.path.join(pkg, "Utility")
    assert where(prediction.vec2pars) == {refutil!r}
    print("RESOLVE-OK", sys.argv[1])
''')


@pytest.mark.parametrize("mode", ["on", "off"])
def test_the_new_names_are_opt_in_behind_the_references_module(mode, tmp_path):
    from nonstationary_multivariate_gaussian_process_amd import predsample_sep as ps
    util = tmp_path / "Utility"
    util.mkdir()
    (util / "__init__.py").write_text("")
    (util / "logpos.py").write_text("def nlogpos_obj_hadamard_SVC(*args):\n    return 0.0\n")
    (util / "prediction.py").write_text("".join("def %s(*args):\n    return args\n\n\n" % f for f in ("vec2pars",) + ps.NAMES))
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    env.pop("NMGP_REFERENCE_UTILITY", None)
    env.pop("NMGP_PREDSAMPLE", None)
    if mode == "on":
        env["NMGP_PREDSAMPLE"] = "1"
    r = subprocess.run([sys.executable, "-c", RESOLVE.format(root=ROOT, refutil=str(util), names=ps.NAMES), mode], cwd=str(tmp_path),
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "RESOLVE-OK" in r.stdout, r.stdout + r.stderr


# ---- the driver's summary ---------------------------------------------------------------------------------------------
class FakeContext:
    """Stands in for _lib.Context: returns synthetic moments, so that the driver's arithmetic is checked without a GPU."""

    def __init__(self, status, M):
        self.status = np.asarray(status, dtype=np.int32)
        self.M = M
        self.calls = []

    def set_data(self, x, Y):
        assert Y.shape[1] == self.M

    def predsample_sep(self, pars, hyper, xs, z=None, star=None, kss_jitter=True):
        H, S = pars.shape[0], xs.shape[0]
        self.calls.append((pars.copy(), np.asarray(hyper).copy(), z.copy(), kss_jitter))
        mean = pars[:, :1, None] + xs[None, :, None] + np.arange(self.M)[None, None, :]
        var = 0.5 + 0.1 * np.abs(pars[:, 1:2, None]) + 0.0 * mean
        bad = self.status[:H] != 0
        mean[bad] = var[bad] = np.nan
        return mean, var, 0.01 * z, self.status[:H]


def test_posterior_predict_separable_summarises_synthetic_moments():
    from nonstationary_multivariate_gaussian_process_amd import drivers, sim
    N, M, S = 4, 2, 3
    P = 2 * N + M * (M + 1) // 2 + 1
    samples = np.arange(5 * 2 * P, dtype=np.float64).reshape(5, 2, P) / 50.0          # [iters, chains, P]
    xs = np.array([0.1, 0.5, 0.9])
    status = np.zeros(10, dtype=np.int32)
    status[3] = 7
    fc = FakeContext(status, M)
    out = drivers.posterior_predict_separable(np.linspace(0, 1, N), np.zeros((N, M)), sim.HYPER_SEP, samples, xs, seed=4, ctx=fc)
    pars, hyper, z, kss = fc.calls[0]
    assert pars.shape == (10, P) and kss is True and z.shape == (10, S, 2)
    assert hyper.tolist() == [float(sim.HYPER_SEP[k]) for k in drivers.SEP_HYPER_KEYS]
    rng = np.random.default_rng(4)
    z0, zy = rng.standard_normal((10, S, 2)), rng.standard_normal((10, S, M))
    assert np.array_equal(z, z0)
    mean, var, star, _ = FakeContext(status, M).predsample_sep(pars, hyper, xs, z=z0)
    ok = status == 0
    assert out["n_used"] == 9 and out["n_failed"] == 1 and out["status"].tolist() == status.tolist()
    np.testing.assert_allclose(out["mean"], mean[ok].mean(axis=0), rtol=1e-15)
    np.testing.assert_allclose(out["var"], var[ok].mean(axis=0) + mean[ok].var(axis=0), rtol=1e-15)
    np.testing.assert_allclose(out["quantiles"], np.percentile((mean + np.sqrt(var) * zy)[ok], [2.5, 50.0, 97.5], axis=0), rtol=1e-15)
    assert np.array_equal(out["tilde_l_star"], star[ok][:, :, 0]) and np.array_equal(out["tilde_sigma_star"], star[ok][:, :, 1])
    assert out["tilde_sigma_star"].shape == (9, S)
    thin = drivers.posterior_predict_separable(np.linspace(0, 1, N), np.zeros((N, M)), sim.HYPER_SEP, samples, xs, draws=4, seed=4,
                                               ctx=FakeContext(np.zeros(10), M))
    assert thin["n_used"] == 4 and thin["tilde_sigma_star"].shape == (4, S)
