"""CPU-only checks of the Hadamard nonseparable model (irregularly observed outputs): a NumPy restatement of the reference's
``logpos_hadamard_SVC`` / ``point_predmap_SVC_hadamard`` (logpos.py:588-659, prediction.py:1401-1465) with its analytic adjoint,
held against the fixtures tests/golden/had_*.npz that tests/golden/make_golden_hadamard.py produced by running the reference;
the mirror's names, signatures and opt-in.  tests/test_gpu_hadamard.py imports the restatement from here."""
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

CASES = [n for n in golden_names("had_N")]


# ---- the model, restated ------------------------------------------------------------------------------------------------
def had_rows(L_vecs, indx, M):
    """R [N, M]: row indx[i] of L_i = vec2lowtriangle(L_vecs[i]) (the slots as they are: no exp), zero-padded."""
    T = M * (M + 1) // 2
    Lv = np.asarray(L_vecs, dtype=np.float64).reshape(-1, T)
    R = np.zeros((Lv.shape[0], M))
    for i, c in enumerate(indx):
        R[i, :c + 1] = Lv[i, c * (c + 1) // 2: c * (c + 1) // 2 + c + 1]
    return R


def had_covariance(tilde_l, L_vecs, tse, x, indx, M, add_noise=True):
    """S = K_x o (R R^T) (+ sigma2 I), K_x the Gibbs kernel carrying the 1e-6 jitter (logpos.py:603-623)."""
    x = np.asarray(x, dtype=np.float64)
    R = had_rows(L_vecs, indx, M)
    Kx = oracle.Nonstationary_RBF_cov(x.reshape(-1, 1), ell1=np.exp(np.asarray(tilde_l, dtype=np.float64)))
    S = Kx * (R @ R.T)
    return S + math.exp(float(tse)) * np.eye(x.shape[0]) if add_noise else S


def had_prior_terms(pars, x, M, hyper):
    """(lp_tilde_l, lp_L_vecs, d lp / d [tilde_l | L_vecs]) of the two GP priors, applied to the raw L_vecs columns."""
    N = x.shape[0]
    T = M * (M + 1) // 2
    mu_l, al_l, be_l, mu_L, al_L, be_L = [float(v) for v in hyper[:6]]
    X1 = x.reshape(-1, 1)
    lp_l, g_l = oracle.mvn_log_prob(pars[:N], mu_l * np.ones(N), oracle.RBF_cov(X1, alpha=al_l, beta=be_l))
    Sig_L = oracle.RBF_cov(X1, alpha=al_L, beta=be_L)
    U = pars[N:N + N * T].reshape(N, T)
    lp_L, g_L = 0.0, np.zeros((N, T))
    for t in range(T):
        lp_t, g_t = oracle.mvn_log_prob(U[:, t], mu_L * np.ones(N), Sig_L)
        lp_L += lp_t
        g_L[:, t] = g_t
    return lp_l, lp_L, -np.concatenate([g_l, g_L.reshape(-1)])


def had_logpos(pars, x, indx, y, hyper, prior=True, grad=False):
    """The verbose tuple (NegLog, loglik, lp_tilde_l, lp_L_vecs, lp_sigma2_err) and, with grad, d NegLog / d pars."""
    pars, x, y = (np.asarray(v, dtype=np.float64) for v in (pars, x, y))
    indx = np.asarray(indx).astype(np.int64)
    N, M = x.shape[0], int(np.unique(indx).shape[0])
    T = M * (M + 1) // 2
    tl, tse = pars[:N], float(pars[-1])
    sigma2 = math.exp(tse)
    a, b = float(hyper[6]), float(hyper[7])
    S = had_covariance(tl, pars[N:N + N * T], tse, x, indx, M)
    C = cholesky(S, lower=True)
    z = solve_triangular(C, y, lower=True)
    loglik = -np.log(np.diag(C)).sum() - 0.5 * (z @ z)
    lp_l, lp_L, g_prior = had_prior_terms(pars, x, M, hyper)
    lp_s2 = oracle.inverse_gamma_logpdf_u(sigma2, alpha=a, beta=b)       # unnormalised here (logpos.py:650)
    res = loglik + ((lp_l + lp_L + lp_s2 + tse) if prior else 0.0)
    out = np.array([-res, loglik, lp_l, lp_L, lp_s2])
    if not grad:
        return out
    alpha = cho_solve((C, True), y)
    G = 0.5 * (np.outer(alpha, alpha) - cho_solve((C, True), np.eye(N)))
    R = had_rows(pars[N:N + N * T], indx, M)
    ell = np.exp(tl)
    D = oracle.pairwise_distances(x.reshape(-1, 1))
    A = (ell ** 2)[:, None] + (ell ** 2)[None, :]
    K0 = np.sqrt(2.0 * np.outer(ell, ell) / A) * np.exp(-D / A)
    Kx = K0 + 1e-6 * np.eye(N)
    dR = 2.0 * (G * Kx) @ R                                   # d loglik / d r_i = 2 sum_j G_ij K_x[i,j] r_j
    e2 = (ell ** 2)[:, None]
    W = 2.0 * G * K0 * (R @ R.T) * (0.5 - e2 / A + 2.0 * e2 * D / (A * A))
    np.fill_diagonal(W, 0.0)
    g_L = np.zeros((N, T))
    for i, c in enumerate(indx):
        g_L[i, c * (c + 1) // 2: c * (c + 1) // 2 + c + 1] = dR[i, :c + 1]
    g = np.concatenate([W.sum(1), g_L.reshape(-1), [sigma2 * np.trace(G)]])
    if prior:
        g[:-1] += g_prior
        g[-1] += (-a - 1.0) + b / sigma2 + 1.0
    return out, -g


def had_predict(pars, x, indx, y, hyper, xs):
    """[S, 3, M] percentiles at the new inputs xs, all M outputs (prediction.py:1401-1465), and the variances [S, M] before
    the clip."""
    pars, x, y, xs = (np.asarray(v, dtype=np.float64) for v in (pars, x, y, xs))
    indx = np.asarray(indx).astype(np.int64)
    N, M = x.shape[0], int(np.unique(indx).shape[0])
    T = M * (M + 1) // 2
    mu_l, al_l, be_l, mu_L, al_L, be_L = [float(v) for v in hyper[:6]]
    tl, Lv, tse = pars[:N], pars[N:N + N * T].reshape(N, T), float(pars[-1])
    sigma2 = math.exp(tse)
    tl_star = oracle._gp_regress(x, xs, tl, mu_l, al_l, be_l)
    L_star = np.stack([oracle._gp_regress(x, xs, Lv[:, t], mu_L, al_L, be_L) for t in range(T)], 1)      # raw: no exp
    C = cholesky(had_covariance(tl, Lv, tse, x, indx, M), lower=True)
    alpha = cho_solve((C, True), y)
    R = had_rows(Lv, indx, M)
    ell = np.exp(tl)
    r, c = oracle.tril_slots(M)
    pct, raw = np.zeros((xs.shape[0], 3, M)), np.zeros((xs.shape[0], M))
    for s in range(xs.shape[0]):
        kx = oracle.Nonstationary_RBF_cov(x.reshape(-1, 1), sigma1=np.ones(N), ell1=ell, X2=xs[s].reshape(1, 1),
                                          sigma2=np.ones(1), ell2=np.array([math.exp(tl_star[s])]))[:, 0]
        Ls = np.zeros((M, M))
        Ls[r, c] = L_star[s]
        kf = kx[:, None] * (R @ Ls.T)                                      # [N, M]
        mean = kf.T @ alpha
        V = solve_triangular(C, kf, lower=True)
        raw[s] = (1.0 + 1e-6) * np.diag(Ls @ Ls.T) - (V * V).sum(0) + sigma2
        sd = np.sqrt(np.where(raw[s] <= 0, 1e-6, raw[s]))
        pct[s] = np.stack([mean - 1.96 * sd, mean, mean + 1.96 * sd])
    return pct, raw


# ---- the restatement meets every fixture ---------------------------------------------------------------------------------
def test_fixture_set_is_complete():
    assert CASES == ["had_N1100_M3", "had_N130_M8", "had_N16_M1", "had_N200_M4", "had_N77_M3"]
    for n in CASES + ["had_map_N77_M3"]:
        g = golden(n)
        assert np.any(np.diff(np.sort(g["x"])) == 0), "no repeated time stamp in " + n
        M = int(g["M"])
        assert sorted(np.unique(g["indx"]).tolist()) == list(range(M))
        assert M == 1 or 2 <= int((g["indx"] == M - 1).sum()) <= 3          # the last label is rare


def _points(g):
    pts = [(g["pars"], int(g["prior"]), g["out"], g["grad"])]
    if "pars2" in g:
        pts.append((g["pars2"], int(g["prior2"]), g["out2"], g["grad2"]))
    return pts


@pytest.mark.parametrize("name", CASES)
def test_numpy_restatement_meets_the_reference(name):
    g = golden(name)
    for pars, prior, ref_out, ref_grad in _points(g):
        out, grad = had_logpos(pars, g["x"], g["indx"], g["y"], g["hyper"], prior=bool(prior), grad=True)
        e_lik, e_pos, e_g = relerr(out[1], ref_out[1]), relerr(out[0], ref_out[0]), vec_relerr(grad, ref_grad)
        print(name, "prior", prior, "loglik", e_lik, "NegLog", e_pos, "grad", e_g)
        assert e_lik < 1e-10
        assert e_g < 1e-8
        assert e_pos < 1e-6 and relerr(out[4], ref_out[4]) < 1e-12
    assert "pars2" not in g or int(g["prior2"]) == 0


@pytest.mark.parametrize("name", ["had_N77_M3", "had_N200_M4"])
def test_numpy_prediction_meets_the_reference(name):
    g = golden(name)
    assert g["grids"].shape == (9,) and g["grids"][2] in g["x"] and (g["grids"] < g["x"].min()).sum() == 1 \
        and (g["grids"] > g["x"].max()).sum() == 1
    pct, raw = had_predict(g["pars"], g["x"], g["indx"], g["y"], g["hyper"], g["grids"])
    assert raw.min() > 1e-4                                   # no variance took the clip branch
    err = relerr(pct, g["pred"])
    print(name, "prediction", err)
    assert err < 1e-8


@pytest.mark.parametrize("name", ["had_N77_M3", "had_N200_M4"])
def test_numpy_covariance_meets_the_reference_and_is_a_restriction_of_the_svc_covariance(name):
    g = golden(name)
    x, indx, pars = g["x"], g["indx"].astype(np.int64), g["pars"]
    N, M = x.shape[0], int(g["M"])
    T = M * (M + 1) // 2
    S = had_covariance(pars[:N], pars[N:N + N * T], pars[-1], x, indx, M)
    np.testing.assert_allclose(S, g["Sigma"], rtol=1e-13, atol=1e-15)
    # the SVC covariance restricted to the observed (output, input) pairs: rows / columns c_i N + i, for uL = Lvecs2uLvecs(L_vecs)
    uL = oracle.Lvecs2uLvecs(pars[N:N + N * T], N, M)
    full = oracle.svc_covariance(pars[:N], uL, pars[-1], x, M)
    sel = indx * N + np.arange(N)
    np.testing.assert_allclose(S, full[np.ix_(sel, sel)], rtol=1e-13, atol=1e-15)


def test_restated_adam_loop_follows_the_map_fixture():
    """The lock-step Adam driver on the NumPy restatement follows the reference's target_value_hist at the bar the GPU driver is
    held to (first 20 steps, 1e-6 relative): the fixture is a trajectory a second implementation can reproduce."""
    from nonstationary_multivariate_gaussian_process_amd.drivers import LockStepMAP
    g = golden("had_map_N77_M3")
    assert g["target_value_hist"].shape == (30,) and float(g["lr"]) == 0.2

    class HostMAP(LockStepMAP):
        def value_and_grad(self, P):
            out, grad = had_logpos(P[0], g["x"], g["indx"], g["y"], g["hyper"], grad=True)
            return out[None], grad[None], np.zeros(1, dtype=np.int32)

    _, hist, alive = HostMAP(g["pars0"][None], lr=0.2).run(20)
    rel = np.abs(hist[:, 0] - g["target_value_hist"][:20]) / np.abs(g["target_value_hist"][:20])
    print("restated MAP trajectory", rel.max())
    assert alive.all() and rel.max() < 1e-6


# ---- names, signatures, opt-in -------------------------------------------------------------------------------------------
HYP = ["mu_tilde_l", "alpha_tilde_l", "beta_tilde_l", "mu_L", "alpha_L", "beta_L"]
SIGNATURES = {
    "nlogpos_obj_hadamard_SVC": ["pars", "x", "indx", "y"] + HYP + ["a", "b", "verbose", "Prior"],
    "logpos_hadamard_SVC": ["tilde_l", "L_vecs", "tilde_sigma2_err", "x", "indx", "y"] + HYP + ["a", "b", "verbose", "Prior"],
    "point_predmap_SVC_hadamard": ["tilde_l", "L_vecs", "tilde_sigma2_err", "x", "indx", "y", "x_star"] + HYP,
    "pointwise_predmap_SVC_hadamard": ["tilde_l", "L_vecs", "tilde_sigma2_err", "x", "indx", "y", "grids"],
    "generate_K_index_SVC_hadamard0": ["L_f_list", "indexes"],
}
DEFAULTS = {
    "nlogpos_obj_hadamard_SVC": dict(mu_tilde_l=0., alpha_tilde_l=1., beta_tilde_l=1., mu_L=0., alpha_L=1., beta_L=1., a=1, b=1,
                                     verbose=False, Prior=True),
    "logpos_hadamard_SVC": dict(verbose=False, Prior=True),
}


def test_module_signatures_follow_the_reference():
    from nonstationary_multivariate_gaussian_process_amd import hadamard
    for fn, params in SIGNATURES.items():
        sig = inspect.signature(getattr(hadamard, fn))
        assert [p for p in sig.parameters if p not in ("args", "kwargs")] == params, fn
        for k, p in sig.parameters.items():
            want = DEFAULTS.get(fn, {}).get(k, inspect.Parameter.empty)
            if k not in ("args", "kwargs"):
                assert p.default == want, (fn, k)
    for fn in ("point_predmap_SVC_hadamard", "pointwise_predmap_SVC_hadamard"):
        kinds = [p.kind for p in inspect.signature(getattr(hadamard, fn)).parameters.values()]
        assert inspect.Parameter.VAR_POSITIONAL in kinds and inspect.Parameter.VAR_KEYWORD in kinds
    assert set(hadamard.LOGPOS_NAMES + hadamard.PREDICTION_NAMES) == set(SIGNATURES)


def test_host_helper_matches_its_definition():
    import torch
    from nonstationary_multivariate_gaussian_process_amd import hadamard
    from nonstationary_multivariate_gaussian_process_amd.Utility import utils
    g = golden("had_N77_M3")
    N, M, T = 77, 3, 6
    Lv = torch.from_numpy(g["pars"][N:N + N * T])
    L_f = [utils.vec2lowtriangle(Lv[n * T:(n + 1) * T], M) for n in range(N)]
    K = hadamard.generate_K_index_SVC_hadamard0(L_f, torch.from_numpy(g["indx"])).numpy()
    R = had_rows(g["pars"][N:N + N * T], g["indx"], M)
    np.testing.assert_allclose(K, R @ R.T, rtol=1e-14, atol=1e-16)


RESOLVE = textwrap.dedent('''
    import inspect, os, sys
    sys.path.insert(0, {root!r})
    import nonstationary_multivariate_gaussian_process_amd as nmgp_amd
    nmgp_amd.install_utility_alias(reference_utility_dir={refutil!r})
    from Utility import logpos, prediction
    pkg = os.path.join({root!r}, "nonstationary_multivariate_gaussian_process_amd")
    def where(obj):
        return os.path.dirname(os.path.abspath(inspect.getsourcefile(obj)))
    served = [where(logpos.nlogpos_obj_hadamard_SVC), where(logpos.logpos_hadamard_SVC),
              where(logpos.generate_K_index_SVC_hadamard0), where(prediction.point_predmap_SVC_hadamard),
              where(prediction.pointwise_predmap_SVC_hadamard)]
    want = pkg if sys.argv[1] == "on" else {refutil!r}
    assert served == [want] * 5, (served, want)
    if sys.argv[1] == "on":
        from nonstationary_multivariate_gaussian_process_amd import hadamard
        assert logpos.nlogpos_obj_hadamard_SVC is hadamard.nlogpos_obj_hadamard_SVC
    # never served by the mirror: they keep resolving to the checkout either way
    for n in ("indexedpoint_predmap_SVC_hadamard", "test_predmap_SVC_hadamard"):
        assert where(getattr(prediction, n)) == {refutil!r}, n
    assert where(logpos.nlogpos_obj_hadamard_S) == {refutil!r}
    assert where(logpos.nlogpos_obj_SVC) == os.path.join(pkg, "Utility")      # unchanged either way
    print("RESOLVE-OK", sys.argv[1])
''')


@pytest.mark.parametrize("mode", ["on", "off"])
def test_the_names_are_opt_in_behind_the_references_modules(mode, tmp_path):
    util = tmp_path / "Utility"
    util.mkdir()
    (util / "__init__.py").write_text("")
    stub = "def %s(*args):\n    return args\n\n\n"
    (util / "logpos.py").write_text("".join(stub % f for f in (
        "nlogpos_obj_hadamard_SVC", "logpos_hadamard_SVC", "generate_K_index_SVC_hadamard0", "nlogpos_obj_hadamard_S")))
    (util / "prediction.py").write_text("".join(stub % f for f in (
        "point_predmap_SVC_hadamard", "pointwise_predmap_SVC_hadamard", "indexedpoint_predmap_SVC_hadamard",
        "test_predmap_SVC_hadamard")))
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    env.pop("NMGP_REFERENCE_UTILITY", None)
    env.pop("NMGP_HADAMARD", None)
    if mode == "on":
        env["NMGP_HADAMARD"] = "1"
    r = subprocess.run([sys.executable, "-c", RESOLVE.format(root=ROOT, refutil=str(util)), mode], cwd=str(tmp_path), env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "RESOLVE-OK" in r.stdout, r.stdout + r.stderr


def test_abi_declares_and_binds_the_four_entries():
    from nonstationary_multivariate_gaussian_process_amd import _lib, build
    names = ["nmgp_had_set_data", "nmgp_had_batch_eval", "nmgp_had_covariance", "nmgp_predict_had"]
    header = open(os.path.join(ROOT, "include", "nmgp.h")).read()
    for n in names:
        assert n in _lib.SIGNATURES and ("int %s(" % n) in header, n
        assert hasattr(_lib.Context, n[len("nmgp_"):] if n != "nmgp_predict_had" else "predict_had")
    assert "nmgp_hadamard.hip" in build.SOURCES
    # the shared schedule and kernels: a header outside HEADERS is outside the build id, and a stale library would load
    assert "nmgp_hadamard_common.h" in [os.path.basename(h) for h in build.HEADERS]
    from nonstationary_multivariate_gaussian_process_amd import drivers
    assert issubclass(drivers.HadamardMAP, drivers.LockStepMAP) and issubclass(drivers.BatchedHMCHadamard, drivers.LockStepHMC)
