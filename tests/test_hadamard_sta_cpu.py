"""CPU-only checks of the Hadamard stationary model (irregularly observed outputs, the LMC baseline): a NumPy restatement of the
reference's ``logpos_hadamard_S`` / ``point_predmap_S_hadamard`` (logpos.py:676-716, prediction.py:1695-1728) with its analytic
adjoint reduced to the T + 3 parameters, held against the fixtures tests/golden/hsta_*.npz that
tests/golden/make_golden_hadamard_sta.py produced by running the reference; the mirror's names, signatures and opt-in.
tests/test_gpu_hadamard_sta.py imports the restatement from here.

Bars of the restatement against the reference: there is no GP prior, so every term is a closed form or hangs on S alone
(cond(S) <= 2e4: 1e4 x 1e-16 per solve; the reference goes through torch.inverse).  likelihood 1e-10, gradient 1e-8; the log
posterior at the project's 1e-6, because lp_tilde_l carries a float32 logarithm (see the test)."""
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

CASES = [n for n in golden_names("hsta_N")]


# ---- the model, restated ------------------------------------------------------------------------------------------------
def hsta_split(pars, M):
    T = M * (M + 1) // 2
    assert pars.shape[0] == T + 3
    return float(pars[0]), float(pars[1]), pars[2:2 + T], float(pars[-1])


def hsta_rows(L_vec, indx, M):
    """R [N, M]: row indx[i] of L = vec2lowtriangle(L_vec) (the slots as they are: no exp)."""
    return oracle.vec2lowtriangle(L_vec, M)[np.asarray(indx).astype(np.int64)]


def hsta_covariance(pars, x, indx, M, add_noise=True):
    """S = K_x o (R R^T) (+ sigma2_err I), K_x = RBF_cov(x; sigma, l) carrying the 1e-6 jitter (logpos.py:685-690)."""
    x = np.asarray(x, dtype=np.float64)
    tl, ts, Lv, tse = hsta_split(np.asarray(pars, dtype=np.float64), M)
    R = hsta_rows(Lv, indx, M)
    S = oracle.RBF_cov(x.reshape(-1, 1), alpha=math.exp(ts), beta=math.exp(tl)) * (R @ R.T)
    return S + math.exp(tse) * np.eye(x.shape[0]) if add_noise else S


def hsta_logpos(pars, x, indx, y, hyper, prior=True, grad=False):
    """The verbose tuple (NegLog, loglik, lp_tilde_l, lp_L_vec, lp_sigma2_err) and, with grad, d NegLog / d pars.  hyper =
    (mu_tilde_l, sigma_tilde_l, a, b, c)."""
    pars, x, y = (np.asarray(v, dtype=np.float64) for v in (pars, x, y))
    indx = np.asarray(indx).astype(np.int64)
    N, M = x.shape[0], int(np.unique(indx).shape[0])
    T = M * (M + 1) // 2
    tl, ts, Lv, tse = hsta_split(pars, M)
    mu_l, sd_l, a, b, c = [float(v) for v in hyper]
    sigma2 = math.exp(tse)
    C = cholesky(hsta_covariance(pars, x, indx, M), lower=True)
    z = solve_triangular(C, y, lower=True)
    loglik = -np.log(np.diag(C)).sum() - 0.5 * (z @ z)                 # no 2 pi term (distributions.multivariate_normal_logpdf)
    lp_l = float(oracle.normal_log_prob(tl, mu_l, sd_l))
    lp_L = float(np.sum(oracle.normal_log_prob(Lv, 0.0, c)))
    lp_s2 = oracle.inverse_gamma_logpdf_u(sigma2, alpha=a, beta=b)       # unnormalised (logpos.py:708)
    res = loglik + ((lp_l + lp_L + lp_s2 + tse) if prior else 0.0)        # tilde_sigma has no prior
    out = np.array([-res, loglik, lp_l, lp_L, lp_s2])
    if not grad:
        return out
    alpha = cho_solve((C, True), y)
    G = 0.5 * (np.outer(alpha, alpha) - cho_solve((C, True), np.eye(N)))
    R = hsta_rows(Lv, indx, M)
    D = oracle.pairwise_distances(x.reshape(-1, 1) / math.exp(tl))
    E = math.exp(ts) ** 2 * np.exp(-0.5 * D)
    V = G * (R @ R.T) * E
    W = (G * (E + 1e-6 * np.eye(N))) @ R                           # w_i[m] = sum_j G_ij (e_ij + jitter d_ij) r_j[m]
    g_L = np.zeros(T)
    for lab in range(M):
        g_L[lab * (lab + 1) // 2: lab * (lab + 1) // 2 + lab + 1] = 2.0 * W[indx == lab, :lab + 1].sum(0)
    g = np.concatenate([[(V * D).sum(), 2.0 * V.sum()], g_L, [sigma2 * np.trace(G)]])
    if prior:
        g[0] -= (tl - float(np.float32(mu_l))) / float(np.float32(sd_l) * np.float32(sd_l))     # torch rounds both to float32
        g[2:2 + T] -= Lv / float(np.float32(c) * np.float32(c))
        g[-1] += (-a - 1.0) + b / sigma2 + 1.0
    return out, -g


def hsta_moments(pars, x, indx, y, xs, indx_star=None):
    """(mean, raw variance before the clip) at the new inputs xs: [S, M] for all outputs (prediction.py:1695-1728), or [S] for the
    labelled output indx_star[s] with B_f[c*, c*] in the prior term.  S^-1 by Cholesky where the reference goes through symeig."""
    pars, x, y, xs = (np.asarray(v, dtype=np.float64) for v in (pars, x, y, xs))
    indx = np.asarray(indx).astype(np.int64)
    M = int(np.unique(indx).shape[0])
    tl, ts, Lv, tse = hsta_split(pars, M)
    C = cholesky(hsta_covariance(pars, x, indx, M), lower=True)
    alpha = cho_solve((C, True), y)
    L = oracle.vec2lowtriangle(Lv, M)
    B_f = L @ L.T
    kx = oracle.RBF_cov(x.reshape(-1, 1), xs.reshape(-1, 1), alpha=math.exp(ts), beta=math.exp(tl))      # [N, S]: no jitter
    kss = math.exp(ts) ** 2 + 1e-6                                     # the jitter sits inside the prior term
    if indx_star is None:
        kf = kx[:, :, None] * B_f[indx][:, None, :]                    # [N, S, M]
        bdiag = np.diag(B_f)[None, :]
    else:
        lab = np.asarray(indx_star).astype(np.int64)
        kf = kx * B_f[indx][:, lab]                                    # [N, S]
        bdiag = np.diag(B_f)[lab]
    flat = kf.reshape(x.shape[0], -1)
    mean = (flat.T @ alpha).reshape(kf.shape[1:])
    V = solve_triangular(C, flat, lower=True)
    raw = bdiag * kss - (V * V).sum(0).reshape(kf.shape[1:]) + math.exp(tse)
    return mean, raw


def hsta_predict(pars, x, indx, y, xs):
    """[S, 3, M] percentiles and the variances [S, M] before the clip."""
    mean, raw = hsta_moments(pars, x, indx, y, xs)
    sd = np.sqrt(np.where(raw <= 0, 1e-6, raw))
    return np.stack([mean - 1.96 * sd, mean, mean + 1.96 * sd], axis=1), raw


# ---- the restatement meets every fixture ---------------------------------------------------------------------------------
def test_fixture_set_is_complete():
    assert CASES == ["hsta_N1100_M3", "hsta_N130_M8", "hsta_N16_M1", "hsta_N200_M4", "hsta_N77_M3"]
    for n in CASES + ["hsta_map_N77_M3"]:
        g = golden(n)
        M = int(g["M"])
        assert np.any(np.diff(np.sort(g["x"])) == 0), "no repeated time stamp in " + n
        assert sorted(np.unique(g["indx"]).tolist()) == list(range(M))
        assert g["hyper"].shape == (5,) and g["pars" if "pars" in g else "pars0"].shape == (M * (M + 1) // 2 + 3,)
        assert float(g["hyper"][1]) != float(np.float32(g["hyper"][1]))      # sigma_tilde_l exercises the float32 rounding
        if "out" in g:
            assert g["out"].shape == (5,) and float(g["cond_S"]) < 1e6 and float(g["min_eig_K"]) > 0.0
        # the subjects are those of the had_* / hsep_* fixtures
        twin = golden(n.replace("hsta_", "hsep_"))
        for k in ("x", "indx", "y"):
            np.testing.assert_array_equal(g[k], twin[k])
    g = golden("hsta_N77_M3")
    assert int(g["prior2"]) == 0 and g["Sigma"].shape == (77, 77) and g["pred"].shape == (9, 3, 3)
    np.testing.assert_array_equal(g["indx_star"], np.arange(9) % 3)
    assert g["test_mean"].shape == g["test_std"].shape == (9,)
    assert golden("hsta_N200_M4")["pred"].shape == (9, 3, 4)


def _points(g):
    pts = [(g["pars"], int(g["prior"]), g["out"], g["grad"])]
    if "pars2" in g:
        pts.append((g["pars2"], int(g["prior2"]), g["out2"], g["grad2"]))
    return pts


@pytest.mark.parametrize("name", CASES)
def test_numpy_restatement_meets_the_reference(name):
    g = golden(name)
    for pars, prior, ref_out, ref_grad in _points(g):
        out, grad = hsta_logpos(pars, g["x"], g["indx"], g["y"], g["hyper"], prior=bool(prior), grad=True)
        e_lik, e_pos, e_g = relerr(out[1], ref_out[1]), relerr(out[0], ref_out[0]), vec_relerr(grad, ref_grad)
        print(name, "prior", prior, "loglik", e_lik, "NegLog", e_pos, "grad", e_g)
        assert e_lik < 1e-10
        assert e_g < 1e-8
        # lp_tilde_l holds log(float32(sigma_tilde_l)) computed IN float32: one unit in its last place is 6e-8 of it, and two
        # libraries' float32 logarithms may differ by that unit (0.7 is not a float32 number; c = 3 is, and log 3's neighbours agree)
        assert relerr(out[2], ref_out[2]) < 1e-6 and relerr(out[3], ref_out[3]) < 1e-12 and relerr(out[4], ref_out[4]) < 1e-12
        assert e_pos < 1e-6


@pytest.mark.parametrize("name", ["hsta_N77_M3", "hsta_N200_M4"])
def test_numpy_prediction_meets_the_reference(name):
    g = golden(name)
    assert g["grids"].shape == (9,) and g["grids"][2] in g["x"] and (g["grids"] < g["x"].min()).sum() == 1 \
        and (g["grids"] > g["x"].max()).sum() == 1
    pct, raw = hsta_predict(g["pars"], g["x"], g["indx"], g["y"], g["grids"])
    assert raw.min() > 1e-4                                   # no variance took the clip branch
    err = float(np.max(np.abs(pct - g["pred"]) / np.abs(g["pred"])))
    print(name, "prediction, element by element", err)
    assert err < 1e-8


def test_numpy_indexed_prediction_meets_the_reference_where_it_is_right():
    """test_predmap_S_hadamard: its mean for all labels; its std takes B_f[0, 0] for every label, so it is met at the label-0
    points only, and the indexed form is the column indx_star[s] of the full form."""
    g = golden("hsta_N77_M3")
    lab = g["indx_star"]
    mean, raw = hsta_moments(g["pars"], g["x"], g["indx"], g["y"], g["grids"], lab)
    e_mean = float(np.max(np.abs(mean - g["test_mean"]) / np.abs(g["test_mean"])))
    zero = lab == 0
    e_sd = float(np.max(np.abs(np.sqrt(raw[zero]) - g["test_std"][zero]) / g["test_std"][zero]))
    print("indexed mean", e_mean, "std at label 0", e_sd)
    assert e_mean < 1e-8 and e_sd < 1e-8 and zero.sum() == 3
    # ... and not at the others: the defect is in the fixture as the reference has it
    assert np.min(np.abs(np.sqrt(raw[~zero]) - g["test_std"][~zero]) / g["test_std"][~zero]) > 1e-3
    fm, fr = hsta_moments(g["pars"], g["x"], g["indx"], g["y"], g["grids"])
    np.testing.assert_allclose(mean, fm[np.arange(9), lab], rtol=1e-12)
    np.testing.assert_allclose(raw, fr[np.arange(9), lab], rtol=1e-12)


@pytest.mark.parametrize("name", ["hsta_N77_M3", "hsta_N200_M4"])
def test_numpy_covariance_meets_the_reference(name):
    g = golden(name)
    S = hsta_covariance(g["pars"], g["x"], g["indx"], int(g["M"]))
    np.testing.assert_allclose(S, g["Sigma"], rtol=1e-13, atol=1e-15)


def test_restated_adam_loop_follows_the_map_fixture():
    """The lock-step Adam driver on the NumPy restatement follows the reference's target_value_hist TEN times inside the bar the
    GPU driver is held to (first 20 steps, 1e-6 relative): the fixture is a trajectory a second implementation can reproduce."""
    from nonstationary_multivariate_gaussian_process_amd.drivers import LockStepMAP
    g = golden("hsta_map_N77_M3")
    assert g["target_value_hist"].shape == (30,) and float(g["lr"]) == 0.05

    class HostMAP(LockStepMAP):
        def value_and_grad(self, P):
            out, grad = hsta_logpos(P[0], g["x"], g["indx"], g["y"], g["hyper"], grad=True)
            return out[None], grad[None], np.zeros(1, dtype=np.int32)

    _, hist, alive = HostMAP(g["pars0"][None], lr=0.05).run(20)
    rel = np.abs(hist[:, 0] - g["target_value_hist"][:20]) / np.abs(g["target_value_hist"][:20])
    print("restated MAP trajectory", rel.max())
    assert alive.all() and rel.max() < 1e-7


# ---- names, signatures, opt-in -------------------------------------------------------------------------------------------
PIECES = ["tilde_l", "tilde_sigma", "L_vec", "tilde_sigma2_err", "x", "indx", "y"]
SIGNATURES = {
    "nlogpos_obj_hadamard_S": ["pars", "x", "indx", "y", "mu_tilde_l", "sigma_tilde_l", "a", "b", "c", "verbose", "Prior"],
    "logpos_hadamard_S": PIECES + ["mu_tilde_l", "sigma_tilde_l", "a", "b", "c", "verbose", "Prior"],
    "point_predmap_S_hadamard": PIECES + ["x_star"],
    "pointwise_predmap_S_hadamard": PIECES + ["grids"],
}
DEFAULTS = {
    "nlogpos_obj_hadamard_S": dict(a=1, b=1, c=10, verbose=False, Prior=True),
    "logpos_hadamard_S": dict(verbose=False, Prior=True),
}


def test_module_signatures_follow_the_reference():
    from nonstationary_multivariate_gaussian_process_amd import hadamard, hadamard_sep, hadamard_sta
    for fn, params in SIGNATURES.items():
        sig = inspect.signature(getattr(hadamard_sta, fn))
        assert [p for p in sig.parameters if p not in ("args", "kwargs")] == params, fn
        for k, p in sig.parameters.items():
            want = DEFAULTS.get(fn, {}).get(k, inspect.Parameter.empty)
            if k not in ("args", "kwargs"):
                assert p.default == want, (fn, k)
    for fn in ("point_predmap_S_hadamard", "pointwise_predmap_S_hadamard"):
        kinds = [p.kind for p in inspect.signature(getattr(hadamard_sta, fn)).parameters.values()]
        assert inspect.Parameter.VAR_POSITIONAL in kinds and inspect.Parameter.VAR_KEYWORD in kinds
    assert set(hadamard_sta.LOGPOS_NAMES + hadamard_sta.PREDICTION_NAMES) == set(SIGNATURES)
    assert list(inspect.signature(hadamard_sta.indexed_predict).parameters) == PIECES + ["x_test", "indx_test"]
    # the other two modules' tuples are not extended
    mine = set(hadamard_sta.LOGPOS_NAMES + hadamard_sta.PREDICTION_NAMES)
    for mod in (hadamard, hadamard_sep):
        assert not mine & set(mod.LOGPOS_NAMES + mod.PREDICTION_NAMES)


def _reference_module(name):
    """Source text of the module `name` of the reference checkout NMGP_REFERENCE_UTILITY names, else None."""
    base = os.environ.get("NMGP_REFERENCE_UTILITY", "")
    path = os.path.join(base, name + ".py") if base else ""
    return open(path).read() if path and os.path.exists(path) else None


def test_signatures_equal_the_checkouts_where_one_is_present():
    """Read from the checkout's source text (its modules need an old torch to import): parameter names, order and defaults."""
    import ast
    from nonstationary_multivariate_gaussian_process_amd import hadamard_sta
    seen = 0
    for modname, names in (("logpos", hadamard_sta.LOGPOS_NAMES), ("prediction", hadamard_sta.PREDICTION_NAMES)):
        src = _reference_module(modname)
        if src is None:
            continue
        defs = {n.name: n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef)}
        for fn in names:
            a = defs[fn].args
            ref_names = [p.arg for p in a.args]
            ref_defaults = [ast.literal_eval(d) for d in a.defaults]
            sig = inspect.signature(getattr(hadamard_sta, fn))
            mine = [p for p in sig.parameters.values() if p.kind == inspect.Parameter.POSITIONAL_OR_KEYWORD]
            assert [p.name for p in mine] == ref_names, fn
            assert [p.default for p in mine if p.default is not inspect.Parameter.empty] == ref_defaults, fn
            assert (a.vararg is not None) == any(p.kind == inspect.Parameter.VAR_POSITIONAL for p in sig.parameters.values()), fn
            seen += 1
    print("signatures compared against a checkout:", seen)


RESOLVE = textwrap.dedent('''
    import inspect, os, sys
    sys.path.insert(0, {root!r})
    import nonstationary_multivariate_gaussian_process_amd as nmgp_amd
    nmgp_amd.install_utility_alias(reference_utility_dir={refutil!r})
    from Utility import logpos, prediction
    pkg = os.path.join({root!r}, "nonstationary_multivariate_gaussian_process_amd")
    def where(obj):
        return os.path.dirname(os.path.abspath(inspect.getsourcefile(obj)))
    served = [where(logpos.nlogpos_obj_hadamard_S), where(logpos.logpos_hadamard_S), where(prediction.point_predmap_S_hadamard),
              where(prediction.pointwise_predmap_S_hadamard)]
    want = pkg if sys.argv[1] == "on" else {refutil!r}
    assert served == [want] * 4, (served, want)
    if sys.argv[1] == "on":
        from nonstationary_multivariate_gaussian_process_amd import hadamard_sta
        assert logpos.nlogpos_obj_hadamard_S is hadamard_sta.nlogpos_obj_hadamard_S
        assert prediction.pointwise_predmap_S_hadamard is hadamard_sta.pointwise_predmap_S_hadamard
    # never served by the mirror: the indexed pair keeps resolving to the checkout either way
    for n in ("indexedpoint_predmap_S_hadamard", "test_predmap_S_hadamard"):
        assert where(getattr(prediction, n)) == {refutil!r}, n
    # the other two Hadamard models follow their own switches
    want_svc = pkg if sys.argv[1] == "other" else {refutil!r}
    assert where(logpos.nlogpos_obj_hadamard_SVC) == want_svc
    want_sep = pkg if sys.argv[1] == "other" else {refutil!r}
    assert where(logpos.nlogpos_obj_hadamard) == want_sep
    assert where(logpos.nlogpos_obj_S) == os.path.join(pkg, "Utility")      # unchanged either way
    print("RESOLVE-OK", sys.argv[1])
''')


@pytest.mark.parametrize("mode", ["on", "off", "other"])
def test_the_names_are_opt_in_behind_the_references_modules(mode, tmp_path):
    """on: NMGP_HADAMARD_STA=1 serves the four names; off: nothing set; other: NMGP_HADAMARD=1 and NMGP_HADAMARD_SEP=1 together do
    not serve them."""
    util = tmp_path / "Utility"
    util.mkdir()
    (util / "__init__.py").write_text("")
    stub = "def %s(*args):\n    return args\n\n\n"
    (util / "logpos.py").write_text("".join(stub % f for f in (
        "nlogpos_obj_hadamard_S", "logpos_hadamard_S", "nlogpos_obj_hadamard", "nlogpos_obj_hadamard_SVC")))
    (util / "prediction.py").write_text("".join(stub % f for f in (
        "point_predmap_S_hadamard", "pointwise_predmap_S_hadamard", "indexedpoint_predmap_S_hadamard", "test_predmap_S_hadamard")))
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    for k in ("NMGP_REFERENCE_UTILITY", "NMGP_HADAMARD", "NMGP_HADAMARD_SEP", "NMGP_HADAMARD_STA", "NMGP_PREDSAMPLE_HADAMARD"):
        env.pop(k, None)
    if mode == "on":
        env["NMGP_HADAMARD_STA"] = "1"
    if mode == "other":
        env["NMGP_HADAMARD"] = "1"
        env["NMGP_HADAMARD_SEP"] = "1"
    r = subprocess.run([sys.executable, "-c", RESOLVE.format(root=ROOT, refutil=str(util)), mode], cwd=str(tmp_path), env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "RESOLVE-OK" in r.stdout, r.stdout + r.stderr


def test_abi_declares_and_binds_the_three_entries():
    from nonstationary_multivariate_gaussian_process_amd import _lib, build
    names = {"nmgp_hadst_batch_eval": "hadst_batch_eval", "nmgp_hadst_covariance": "hadst_covariance",
             "nmgp_predict_hadst": "predict_hadst"}
    header = open(os.path.join(ROOT, "include", "nmgp.h")).read()
    for n, method in names.items():
        assert n in _lib.SIGNATURES and ("int %s(" % n) in header, n
        assert hasattr(_lib.Context, method)
    assert "nmgp_hadamard_sta.hip" in build.SOURCES and "-ffp-contract=off" in build.CODEGEN_FLAGS


def test_driver_classes_have_the_lockstep_parents():
    from nonstationary_multivariate_gaussian_process_amd import drivers
    assert issubclass(drivers.HadamardStaMAP, drivers.LockStepMAP) and issubclass(drivers.BatchedHMCHadamardSta, drivers.LockStepHMC)
    assert issubclass(drivers.HadamardStaMAP, drivers._HadamardStaSubject)
    assert issubclass(drivers.BatchedHMCHadamardSta, drivers._HadamardStaSubject)
    assert not issubclass(drivers.HadamardSepMAP, drivers._HadamardStaSubject)
    assert drivers._HadamardStaSubject.HYPER_KEYS == ("mu_tilde_l", "sigma_tilde_l", "a", "b", "c")
    assert callable(drivers.posterior_predict_hadamard_sta)
    # the prior-factor metrics are refused as by the other two pairs (before anything touches a device)
    g = golden("hsta_N16_M1")
    for metric in (drivers.PriorMetric, drivers.SeparablePriorMetric):
        m = object.__new__(metric)
        m.P = g["pars"].shape[0]
        with pytest.raises(NotImplementedError):
            drivers.BatchedHMCHadamardSta(g["x"], g["indx"], g["y"], {}, g["pars"][None], M=m)
