"""CPU-only checks of the Hadamard separable model (irregularly observed outputs, one shared cross-output matrix): a NumPy
restatement of the reference's ``logpos_hadamard`` / ``point_predmap_hadamard`` (logpos.py:502-563, prediction.py:710-785) with its
analytic adjoint, held against the fixtures tests/golden/hsep_*.npz that tests/golden/make_golden_hadamard_sep.py produced by
running the reference; the mirror's names, signatures and opt-in.  tests/test_gpu_hadamard_sep.py imports the restatement from here.

Bars of the restatement against the reference: the two GP priors' factors have cond ~ 1e8 (RBF + 1e-6 I with repeated time stamps),
so the reference's own prior terms and prior gradients carry ~1e8 x 1e-16; the likelihood (cond(S) <= 2e4) is good to 1e-10."""
import inspect
import math
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
from scipy.linalg import cho_solve, cholesky, solve_triangular

from conftest import ROOT, golden, golden_names, relerr, vec_relerr
from oracle import nmgp_oracle as oracle

CASES = [n for n in golden_names("hsep_N")]


# ---- the model, restated ------------------------------------------------------------------------------------------------
def hsep_split(pars, N, M):
    T = M * (M + 1) // 2
    assert pars.shape[0] == 2 * N + T + 1
    return pars[:N], pars[N:2 * N], pars[2 * N:2 * N + T], float(pars[-1])


def hsep_rows(L_vec, indx, M):
    """R [N, M]: row indx[i] of the ONE L = vec2lowtriangle(L_vec) (the slots as they are: no exp)."""
    return oracle.vec2lowtriangle(L_vec, M)[np.asarray(indx).astype(np.int64)]


def hsep_covariance(pars, x, indx, M, add_noise=True):
    """S = K_x o (R R^T) (+ sigma2 I), K_x the Gibbs kernel with amplitudes, carrying the 1e-6 jitter (logpos.py:517-528)."""
    x = np.asarray(x, dtype=np.float64)
    tl, ts, Lv, tse = hsep_split(np.asarray(pars, dtype=np.float64), x.shape[0], M)
    R = hsep_rows(Lv, indx, M)
    Kx = oracle.Nonstationary_RBF_cov(x.reshape(-1, 1), sigma1=np.exp(ts), ell1=np.exp(tl))
    S = Kx * (R @ R.T)
    return S + math.exp(tse) * np.eye(x.shape[0]) if add_noise else S


def hsep_prior_terms(pars, x, M, hyper):
    """(lp_tilde_l, lp_tilde_sigma, lp_L_vec, d (their sum) / d [tilde_l | tilde_sigma | L_vec])."""
    N = x.shape[0]
    tl, ts, Lv, _ = hsep_split(pars, N, M)
    mu_l, al_l, be_l, mu_s, al_s, be_s = [float(v) for v in hyper[:6]]
    c = float(hyper[8])
    X1 = x.reshape(-1, 1)
    lp_l, g_l = oracle.mvn_log_prob(tl, mu_l * np.ones(N), oracle.RBF_cov(X1, alpha=al_l, beta=be_l))
    lp_s, g_s = oracle.mvn_log_prob(ts, mu_s * np.ones(N), oracle.RBF_cov(X1, alpha=al_s, beta=be_s))
    lp_L = float(np.sum(oracle.normal_log_prob(Lv, 0.0, c)))
    var = float(np.float32(c) * np.float32(c))                 # torch rounds a Python-number scale to float32
    return lp_l, lp_s, lp_L, -np.concatenate([g_l, g_s, Lv / var])


def hsep_logpos(pars, x, indx, y, hyper, prior=True, grad=False):
    """The verbose tuple (NegLog, loglik, lp_tilde_l, lp_tilde_sigma, lp_L_vec, lp_sigma2_err) and, with grad, d NegLog / d pars."""
    pars, x, y = (np.asarray(v, dtype=np.float64) for v in (pars, x, y))
    indx = np.asarray(indx).astype(np.int64)
    N, M = x.shape[0], int(np.unique(indx).shape[0])
    T = M * (M + 1) // 2
    tl, ts, Lv, tse = hsep_split(pars, N, M)
    sigma2 = math.exp(tse)
    a, b = float(hyper[6]), float(hyper[7])
    S = hsep_covariance(pars, x, indx, M)
    C = cholesky(S, lower=True)
    z = solve_triangular(C, y, lower=True)
    loglik = -np.log(np.diag(C)).sum() - 0.5 * (z @ z)
    lp_l, lp_s, lp_L, g_prior = hsep_prior_terms(pars, x, M, hyper)
    lp_s2 = oracle.inverse_gamma_logpdf_u(sigma2, alpha=a, beta=b)       # unnormalised (logpos.py:555)
    res = loglik + ((lp_l + lp_s + lp_L + lp_s2 + tse) if prior else 0.0)
    out = np.array([-res, loglik, lp_l, lp_s, lp_L, lp_s2])
    if not grad:
        return out
    alpha = cho_solve((C, True), y)
    G = 0.5 * (np.outer(alpha, alpha) - cho_solve((C, True), np.eye(N)))
    R = hsep_rows(Lv, indx, M)
    ell, sig = np.exp(tl), np.exp(ts)
    D = oracle.pairwise_distances(x.reshape(-1, 1))
    A = (ell ** 2)[:, None] + (ell ** 2)[None, :]
    K0 = np.outer(sig, sig) * np.sqrt(2.0 * np.outer(ell, ell) / A) * np.exp(-D / A)
    Kx = K0 + 1e-6 * np.eye(N)
    V = 2.0 * G * K0 * (R @ R.T)
    g_s = V.sum(1)                                            # j = i included
    e2 = (ell ** 2)[:, None]
    W = V * (0.5 - e2 / A + 2.0 * e2 * D / (A * A))
    np.fill_diagonal(W, 0.0)
    dR = 2.0 * (G * Kx) @ R                                   # row components: sum_j 2 G_ij K_x[i, j] r_j
    g_L = np.zeros(T)
    for c in range(M):
        g_L[c * (c + 1) // 2: c * (c + 1) // 2 + c + 1] = dR[indx == c, :c + 1].sum(0)
    g = np.concatenate([W.sum(1), g_s, g_L, [sigma2 * np.trace(G)]])
    if prior:
        g[:-1] += g_prior
        g[-1] += (-a - 1.0) + b / sigma2 + 1.0
    return out, -g


def hsep_predict(pars, x, indx, y, hyper, xs):
    """[S, 3, M] percentiles at the new inputs xs, all M outputs (prediction.py:710-785), and the variances [S, M] before the
    clip.  S^-1 by Cholesky where the reference goes through symeig."""
    pars, x, y, xs = (np.asarray(v, dtype=np.float64) for v in (pars, x, y, xs))
    indx = np.asarray(indx).astype(np.int64)
    N, M = x.shape[0], int(np.unique(indx).shape[0])
    mu_l, al_l, be_l, mu_s, al_s, be_s = [float(v) for v in hyper[:6]]
    tl, ts, Lv, tse = hsep_split(pars, N, M)
    sigma2 = math.exp(tse)
    tl_star = oracle._gp_regress(x, xs, tl, mu_l, al_l, be_l)
    ts_star = oracle._gp_regress(x, xs, ts, mu_s, al_s, be_s)
    C = cholesky(hsep_covariance(pars, x, indx, M), lower=True)
    alpha = cho_solve((C, True), y)
    L = oracle.vec2lowtriangle(Lv, M)
    B_f = L @ L.T
    pct, raw = np.zeros((xs.shape[0], 3, M)), np.zeros((xs.shape[0], M))
    for s in range(xs.shape[0]):
        ss = math.exp(ts_star[s])
        kx = oracle.Nonstationary_RBF_cov(x.reshape(-1, 1), sigma1=np.exp(ts), ell1=np.exp(tl), X2=xs[s].reshape(1, 1),
                                          sigma2=np.array([ss]), ell2=np.array([math.exp(tl_star[s])]))[:, 0]
        kf = kx[:, None] * B_f[indx, :]                                    # [N, M]: no jitter on the cross term
        mean = kf.T @ alpha
        V = solve_triangular(C, kf, lower=True)
        raw[s] = np.diag(B_f) * (ss * ss + 1e-6) - (V * V).sum(0) + sigma2  # the jitter sits inside the prior term
        sd = np.sqrt(np.where(raw[s] <= 0, 1e-6, raw[s]))
        pct[s] = np.stack([mean - 1.96 * sd, mean, mean + 1.96 * sd])
    return pct, raw


# ---- the restatement meets every fixture ---------------------------------------------------------------------------------
def test_fixture_set_is_complete():
    assert CASES == ["hsep_N1100_M3", "hsep_N130_M8", "hsep_N16_M1", "hsep_N200_M4", "hsep_N77_M3"]
    for n in CASES + ["hsep_map_N77_M3"]:
        g = golden(n)
        N, M = g["x"].shape[0], int(g["M"])
        assert np.any(np.diff(np.sort(g["x"])) == 0), "no repeated time stamp in " + n
        assert sorted(np.unique(g["indx"]).tolist()) == list(range(M))
        assert M == 1 or 2 <= int((g["indx"] == M - 1).sum()) <= 3          # the last label is rare
        assert g["hyper"].shape == (9,) and g["pars" if "pars" in g else "pars0"].shape == (2 * N + M * (M + 1) // 2 + 1,)
        if "out" in g:
            assert g["out"].shape == (6,) and float(g["cond_S"]) < 1e6 and float(g["min_eig_K"]) > 0.0
    assert int((golden("hsep_N77_M3")["indx"] == 2).sum()) == 2              # the segmented reduction's two-member label


def _points(g):
    pts = [(g["pars"], int(g["prior"]), g["out"], g["grad"])]
    if "pars2" in g:
        pts.append((g["pars2"], int(g["prior2"]), g["out2"], g["grad2"]))
    return pts


@pytest.mark.parametrize("name", CASES)
def test_numpy_restatement_meets_the_reference(name):
    g = golden(name)
    for pars, prior, ref_out, ref_grad in _points(g):
        out, grad = hsep_logpos(pars, g["x"], g["indx"], g["y"], g["hyper"], prior=bool(prior), grad=True)
        e_lik, e_pos, e_g = relerr(out[1], ref_out[1]), relerr(out[0], ref_out[0]), vec_relerr(grad, ref_grad)
        e_L = relerr(out[4], ref_out[4])
        print(name, "prior", prior, "loglik", e_lik, "NegLog", e_pos, "grad", e_g, "lp_L_vec", e_L)
        assert e_lik < 1e-10
        assert e_g < 1e-8
        assert e_pos < 1e-6 and relerr(out[5], ref_out[5]) < 1e-12 and e_L < 1e-12
        assert relerr(out[2:4], ref_out[2:4]) < 1e-6
    assert "pars2" not in g or int(g["prior2"]) == 0


@pytest.mark.parametrize("name", ["hsep_N77_M3", "hsep_N200_M4"])
def test_numpy_prediction_meets_the_reference(name):
    g = golden(name)
    assert g["grids"].shape == (9,) and g["grids"][2] in g["x"] and (g["grids"] < g["x"].min()).sum() == 1 \
        and (g["grids"] > g["x"].max()).sum() == 1
    pct, raw = hsep_predict(g["pars"], g["x"], g["indx"], g["y"], g["hyper"], g["grids"])
    assert raw.min() > 1e-4                                   # no variance took the clip branch
    err = relerr(pct, g["pred"])
    print(name, "prediction", err)
    assert err < 1e-8


@pytest.mark.parametrize("name", ["hsep_N77_M3", "hsep_N200_M4"])
def test_numpy_covariance_meets_the_reference(name):
    g = golden(name)
    S = hsep_covariance(g["pars"], g["x"], g["indx"], int(g["M"]))
    np.testing.assert_allclose(S, g["Sigma"], rtol=1e-13, atol=1e-15)


def test_restated_adam_loop_follows_the_map_fixture():
    """The lock-step Adam driver on the NumPy restatement follows the reference's target_value_hist TEN times inside the bar the
    GPU driver is held to (first 20 steps, 1e-6 relative): the fixture is a trajectory a second implementation can reproduce."""
    from nonstationary_multivariate_gaussian_process_amd.drivers import LockStepMAP
    g = golden("hsep_map_N77_M3")
    assert g["target_value_hist"].shape == (30,) and float(g["lr"]) == 0.05

    class HostMAP(LockStepMAP):
        def value_and_grad(self, P):
            out, grad = hsep_logpos(P[0], g["x"], g["indx"], g["y"], g["hyper"], grad=True)
            return out[None], grad[None], np.zeros(1, dtype=np.int32)

    _, hist, alive = HostMAP(g["pars0"][None], lr=0.05).run(20)
    rel = np.abs(hist[:, 0] - g["target_value_hist"][:20]) / np.abs(g["target_value_hist"][:20])
    print("restated MAP trajectory", rel.max())
    assert alive.all() and rel.max() < 1e-7


# ---- names, signatures, opt-in -------------------------------------------------------------------------------------------
HYP = ["mu_tilde_l", "alpha_tilde_l", "beta_tilde_l", "mu_tilde_sigma", "alpha_tilde_sigma", "beta_tilde_sigma"]
PIECES = ["tilde_l", "tilde_sigma", "L_vec", "tilde_sigma2_err", "x", "indx", "y"]
SIGNATURES = {
    "nlogpos_obj_hadamard": ["pars", "x", "indx", "y"] + HYP + ["a", "b", "c", "verbose", "Prior"],
    "logpos_hadamard": PIECES + HYP + ["a", "b", "c", "verbose", "Prior"],
    "point_predmap_hadamard": PIECES + ["x_star"] + HYP,
    "pointwise_predmap_hadmard": PIECES + ["grids"] + HYP,
}
DEFAULTS = {
    "nlogpos_obj_hadamard": dict(mu_tilde_l=0., alpha_tilde_l=1., beta_tilde_l=1., mu_tilde_sigma=0., alpha_tilde_sigma=1.,
                                 beta_tilde_sigma=1., a=1, b=1, c=10, verbose=False, Prior=True),
    "logpos_hadamard": dict(verbose=False, Prior=True),
}


def test_module_signatures_follow_the_reference():
    from nonstationary_multivariate_gaussian_process_amd import hadamard, hadamard_sep
    for fn, params in SIGNATURES.items():
        sig = inspect.signature(getattr(hadamard_sep, fn))
        assert [p for p in sig.parameters if p not in ("args", "kwargs")] == params, fn
        for k, p in sig.parameters.items():
            want = DEFAULTS.get(fn, {}).get(k, inspect.Parameter.empty)
            if k not in ("args", "kwargs"):
                assert p.default == want, (fn, k)
    for fn in ("point_predmap_hadamard", "pointwise_predmap_hadmard"):
        kinds = [p.kind for p in inspect.signature(getattr(hadamard_sep, fn)).parameters.values()]
        assert inspect.Parameter.VAR_POSITIONAL in kinds and inspect.Parameter.VAR_KEYWORD in kinds
    assert hadamard_sep.pointwise_predmap_hadamard is hadamard_sep.pointwise_predmap_hadmard
    assert set(hadamard_sep.LOGPOS_NAMES + hadamard_sep.PREDICTION_NAMES) == set(SIGNATURES) | {"pointwise_predmap_hadamard"}
    # the nonseparable module's tuples are not extended
    assert not set(hadamard_sep.LOGPOS_NAMES + hadamard_sep.PREDICTION_NAMES) & set(hadamard.LOGPOS_NAMES + hadamard.PREDICTION_NAMES)


RESOLVE = textwrap.dedent('''
    import inspect, os, sys
    sys.path.insert(0, {root!r})
    import nonstationary_multivariate_gaussian_process_amd as nmgp_amd
    nmgp_amd.install_utility_alias(reference_utility_dir={refutil!r})
    from Utility import logpos, prediction
    pkg = os.path.join({root!r}, "nonstationary_multivariate_gaussian_process_amd")
    def where(obj):
        return os.path.dirname(os.path.abspath(inspect.getsourcefile(obj)))
    served = [where(logpos.nlogpos_obj_hadamard), where(logpos.logpos_hadamard), where(prediction.point_predmap_hadamard),
              where(prediction.pointwise_predmap_hadmard)]
    want = pkg if sys.argv[1] == "on" else {refutil!r}
    assert served == [want] * 4, (served, want)
    if sys.argv[1] == "on":
        from nonstationary_multivariate_gaussian_process_amd import hadamard_sep
        assert logpos.nlogpos_obj_hadamard is hadamard_sep.nlogpos_obj_hadamard
        assert prediction.pointwise_predmap_hadamard is hadamard_sep.pointwise_predmap_hadmard
    # never served by the mirror: they keep resolving to the checkout either way
    for n in ("indexedpoint_predmap_hadamard", "test_predmap_hadamard", "pointwise_predsample_hadamard"):
        assert where(getattr(prediction, n)) == {refutil!r}, n
    assert where(logpos.nlogpos_obj_hadamard_S) == {refutil!r}
    # the nonseparable Hadamard names follow their own switch
    want_svc = pkg if sys.argv[1] == "other" else {refutil!r}
    assert where(logpos.nlogpos_obj_hadamard_SVC) == want_svc
    assert where(logpos.nlogpos_obj_SVC) == os.path.join(pkg, "Utility")      # unchanged either way
    print("RESOLVE-OK", sys.argv[1])
''')


@pytest.mark.parametrize("mode", ["on", "off", "other"])
def test_the_names_are_opt_in_behind_the_references_modules(mode, tmp_path):
    """on: NMGP_HADAMARD_SEP=1 serves the four names; off: nothing set; other: NMGP_HADAMARD=1 alone does not serve them."""
    util = tmp_path / "Utility"
    util.mkdir()
    (util / "__init__.py").write_text("")
    stub = "def %s(*args):\n    return args\n\n\n"
    (util / "logpos.py").write_text("".join(stub % f for f in (
        "nlogpos_obj_hadamard", "logpos_hadamard", "nlogpos_obj_hadamard_S", "nlogpos_obj_hadamard_SVC")))
    (util / "prediction.py").write_text("".join(stub % f for f in (
        "point_predmap_hadamard", "pointwise_predmap_hadmard", "indexedpoint_predmap_hadamard", "test_predmap_hadamard",
        "pointwise_predsample_hadamard")))
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    for k in ("NMGP_REFERENCE_UTILITY", "NMGP_HADAMARD", "NMGP_HADAMARD_SEP"):
        env.pop(k, None)
    if mode == "on":
        env["NMGP_HADAMARD_SEP"] = "1"
    if mode == "other":
        env["NMGP_HADAMARD"] = "1"
    r = subprocess.run([sys.executable, "-c", RESOLVE.format(root=ROOT, refutil=str(util)), mode], cwd=str(tmp_path), env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "RESOLVE-OK" in r.stdout, r.stdout + r.stderr


def test_abi_declares_and_binds_the_three_entries():
    from nonstationary_multivariate_gaussian_process_amd import _lib, build
    names = {"nmgp_hads_batch_eval": "hads_batch_eval", "nmgp_hads_covariance": "hads_covariance", "nmgp_predict_hads": "predict_hads"}
    header = open(os.path.join(ROOT, "include", "nmgp.h")).read()
    for n, method in names.items():
        assert n in _lib.SIGNATURES and ("int %s(" % n) in header, n
        assert hasattr(_lib.Context, method)
    assert "nmgp_hadamard_sep.hip" in build.SOURCES and "nmgp_hadamard.hip" in build.SOURCES


def test_driver_classes_have_the_lockstep_parents():
    from nonstationary_multivariate_gaussian_process_amd import drivers
    assert issubclass(drivers.HadamardSepMAP, drivers.LockStepMAP) and issubclass(drivers.BatchedHMCHadamardSep, drivers.LockStepHMC)
    assert issubclass(drivers.HadamardSepMAP, drivers._HadamardSepSubject)
    assert issubclass(drivers.BatchedHMCHadamardSep, drivers._HadamardSepSubject)
    assert not issubclass(drivers.HadamardMAP, drivers._HadamardSepSubject)
    # the prior-factor metrics are refused as by the nonseparable pair (before anything touches a device)
    g = golden("hsep_N16_M1")
    for metric in (drivers.PriorMetric, drivers.SeparablePriorMetric):
        m = object.__new__(metric)
        m.P = g["pars"].shape[0]
        with pytest.raises(NotImplementedError):
            drivers.BatchedHMCHadamardSep(g["x"], g["indx"], g["y"], {}, g["pars"][None], M=m)
