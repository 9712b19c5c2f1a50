"""CPU-only checks of the posterior-draw / held-out prediction of the nonseparable Hadamard model: the NumPy restatement
(tests/predsample_had_cases.restate_hpn, which tests/test_gpu_predsample_had.py compares the device entry with) is held to what
exists -- the restated MAP predictor had_predict, the reference's recorded grids had_*["pred"], and the reference's held-out MAP
predictor recorded in tests/golden/hpn_N77_M3.npz (tests/golden/make_golden_predsample_had.py); the Python names, their shapes and
the ABI.

Bars: the ones tests/test_hadamard_cpu.py uses for had_predict against had_N77_M3["pred"]: 1e-8 relative element by element
(conftest.relerr), and no compared variance near the clip (raw variance > 1e-4 on the fixtures' grids)."""
import inspect
import os

import numpy as np
import pytest
import torch

import predsample_had_cases as pc
from conftest import ROOT, golden, relerr
from predsample_had_cases import restate_hpn
from test_hadamard_cpu import had_predict

RESTATE_TOL = 1e-8


def bands(mean, raw):
    sd = np.sqrt(np.where(raw <= 0, 1e-6, raw))
    return np.stack([mean - 1.96 * sd, mean, mean + 1.96 * sd], axis=1)            # [S, 3, M]


# ---- (a) z = 0, one draw, full form is the MAP predictor ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(5, 5, "unsorted"), (63, 2, "blocks"), "had_N77_M3"], ids=pc.parity_id)
def test_one_draw_without_noise_is_had_predict(case):
    c = pc.subject(case)
    xs, _ = pc.new_inputs(case)
    for h in (0, 1):
        pct, raw0 = had_predict(c["draws"][h], c["x"], c["indx"], c["y"], c["hyper"], xs)
        for z in (None, np.zeros((1, xs.shape[0], 1 + c["T"]))):
            mean, raw, star = restate_hpn(c["x"], c["indx"], c["y"], c["draws"][h], c["hyper"], xs, z)
            assert mean.shape == raw.shape == (1, xs.shape[0], c["M"]) and star.shape == (1, xs.shape[0], 1 + c["T"])
            assert relerr(mean[0], pct[:, 1]) < 1e-12 and relerr(raw[0], raw0) < 1e-12


# ---- (b) the reference's recorded grids ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pc.FIXTURES)
def test_restatement_meets_the_recorded_grids(name):
    g = golden(name)
    mean, raw, _ = restate_hpn(g["x"], g["indx"], g["y"], g["pars"], g["hyper"], g["grids"], None)
    assert raw.min() > 1e-4                                   # no variance took the clip branch
    err = relerr(bands(mean[0], raw[0]), g["pred"])
    print(name, "prediction", err)
    assert err < RESTATE_TOL


# ---- (c) the reference's held-out MAP predictor ---------------------------------------------------------------------------------------
def test_fixture_and_restatement_meet_the_references_held_out_predictor():
    g, h = golden("hpn_N77_M3"), golden("had_N77_M3")
    assert all(np.array_equal(g[k], h[k]) for k in ("x", "indx", "y", "pars", "hyper"))
    xt, lab = g["x_test"], g["indx_test"]
    assert xt.shape == lab.shape == g["mean"].shape == g["var"].shape == (12,)
    assert lab.tolist() == [0, 1, 2] * 4 and int(np.isin(xt, g["x"]).sum()) == 1
    assert (xt < g["x"].min()).sum() + (xt > g["x"].max()).sum() == 1
    zero = lab == 0
    assert zero.sum() >= 4
    mean, raw, _ = restate_hpn(g["x"], g["indx"], g["y"], g["pars"], g["hyper"], xt, None, lab)
    assert mean.shape == raw.shape == (1, 12)
    assert g["var"][zero].min() > 10 * 1e-6 and raw[0][zero].min() > 10 * 1e-6          # nowhere near the clip
    e_m, e_v = relerr(mean[0], g["mean"]), relerr(raw[0][zero], g["var"][zero])
    print("held-out: mean", e_m, "var at label 0", e_v)
    assert e_m < RESTATE_TOL and e_v < RESTATE_TOL
    # why the variance is compared at label 0 only: elsewhere the reference takes output 0's prior variance
    assert relerr(raw[0][~zero], g["var"][~zero]) > 1e-2 and np.all(raw[0][~zero] > 1e-4)


# ---- (d) indexed is the labelled column of the full form -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(8, 8, "interleaved"), (64, 5, "rare_last"), "had_N77_M3"], ids=pc.parity_id)
def test_indexed_form_is_the_labelled_column_of_the_full_form(case):
    e = pc.expected(case)
    S = e["xs"].shape[0]
    (fm, fv, fs), (im, iv, is_) = e["full"], e["ix"]
    assert np.array_equal(fs, is_) and len(set(e["lab"].tolist())) > 1
    assert relerr(im, fm[:, np.arange(S), e["lab"]]) < 1e-12 and relerr(iv, fv[:, np.arange(S), e["lab"]]) < 1e-12


# ---- (e) the noise of the latent regression ------------------------------------------------------------------------------------------
def test_normals_move_the_starred_values_by_the_conditional_standard_deviation():
    case = (63, 2, "blocks")
    c = pc.subject(case)
    xs = np.concatenate([pc.new_inputs(case)[0], c["x"][:3]])          # three more training inputs: conditional variances near 0
    S, T, h = xs.shape[0], c["T"], c["hyper"]
    z = np.random.default_rng(5).standard_normal((2, S, 1 + T))
    star0 = restate_hpn(c["x"], c["indx"], c["y"], c["draws"], h, xs, None)[2]
    star = restate_hpn(c["x"], c["indx"], c["y"], c["draws"], h, xs, z)[2]
    cv_l, cv_L = pc.cond_var(c["x"], xs, h[1], h[2]), pc.cond_var(c["x"], xs, h[4], h[5])
    assert np.all(cv_l > 0) and np.all(cv_L > 0) and cv_l.min() < 1e-4 * cv_l.max()
    sd = np.concatenate([np.sqrt(cv_l)[:, None], np.repeat(np.sqrt(cv_L)[:, None], T, axis=1)], axis=1)      # ONE cv per prior
    assert np.array_equal(star, star0 + sd[None] * z) and not np.array_equal(star, star0)
    # the same expression as the restatement of the complete-data entry (its own RBF, its own solve)
    from test_predsample_cpu import regression
    for (al, be), cv in (((h[1], h[2]), cv_l), ((h[4], h[5]), cv_L)):
        np.testing.assert_allclose(cv, regression(c["x"], xs, al, be)[1], rtol=1e-6, atol=1e-9)
    # the rule: strictly negative -> 1e-6 (0 stays 0)
    assert pc.clip_cv(np.array([-1e-9, 0.0, 1e-9])).tolist() == [1e-6, 0.0, 1e-9]


# ---- (f) the Python layer ----------------------------------------------------------------------------------------------------------------
def _fake_context(monkeypatch):
    """A Context that never opens a device: had_set_data keeps the subject, predsample_had is the restatement (clip applied, status 0)."""
    from nonstationary_multivariate_gaussian_process_amd import _lib
    calls = []

    def had_set_data(self, x, indx, y, M=None):
        self._subject = (np.array(x), np.array(indx), np.array(y))
        self.M = int(np.unique(indx).shape[0])
        self.N, self.T = len(x), self.M * (self.M + 1) // 2

    def predsample_had(self, pars_hist, hyper, xs, indx_star=None, z=None, star=None):
        x, indx, y = self._subject
        mean, raw, st = restate_hpn(x, indx, y, pars_hist, hyper, xs, z, indx_star)
        calls.append((np.atleast_2d(pars_hist).shape[0], len(xs)))
        return mean, np.where(raw <= 0, 1e-6, raw), st, np.zeros(mean.shape[0], dtype=np.int32)

    monkeypatch.setattr(_lib.Context, "had_set_data", had_set_data)
    monkeypatch.setattr(_lib.Context, "predsample_had", predsample_had)
    host = object.__new__(_lib.Context)
    monkeypatch.setattr(_lib, "default_context", lambda device=None: host)
    return host, calls


def test_python_names_shapes_and_one_device_call(monkeypatch):
    from nonstationary_multivariate_gaussian_process_amd import hadamard
    host, calls = _fake_context(monkeypatch)
    g = golden("hpn_N77_M3")
    N, M, T = 77, 3, 6
    t = torch.from_numpy
    H = 3
    d = np.stack([g["pars"] + 0.01 * k for k in range(H)])
    hist = (t(d[:, :N]), t(d[:, N:N + N * T]), t(d[:, -1]), t(g["x"]), t(g["indx"]), t(g["y"]))
    h = [float(v) for v in g["hyper"][:6]]
    xs, lab = g["x_test"][:5], g["indx_test"][:5]
    rng = np.random.default_rng(2)
    z, zy, zyi = rng.standard_normal((5, H, 1 + T)), rng.standard_normal((5, H, M)), rng.standard_normal((5, H))
    ys = hadamard.pointwise_predsample_SVC_hadamard(*hist, t(xs), *h, z=z, zy=zy)
    assert isinstance(ys, torch.Tensor) and ys.dtype == torch.float64 and tuple(ys.shape) == (5, H, M) and calls == [(H, 5)]
    one = hadamard.point_predsample_SVC_hadamard(*hist, t(xs[2:3])[0], *h, z=z[2:3], zy=zy[2:3])
    assert tuple(one.shape) == (H, M) and relerr(one.numpy(), ys[2].numpy()) < RESTATE_TOL      # another solve width: rounding
    yt = hadamard.test_predsample_SVC_hadamard(*hist, t(xs), t(lab), *h, z=z, zy=zyi)
    assert tuple(yt.shape) == (5, H) and calls[-1] == (H, 5) and len(calls) == 3
    one = hadamard.indexedpoint_predsample_SVC_hadamard(*hist, t(xs[3:4])[0], t(lab[3:4])[0], *h, z=z[3:4], zy=zyi[3:4])
    assert tuple(one.shape) == (H,) and relerr(one.numpy(), yt[3].numpy()) < RESTATE_TOL
    # sampled y = mean + sqrt(var) zy under the starred values z gives
    mean, raw, _ = restate_hpn(g["x"], g["indx"], g["y"], d, g["hyper"], xs, np.swapaxes(z, 0, 1), lab)
    assert relerr(yt.numpy(), (mean + np.sqrt(raw) * np.swapaxes(zyi, 0, 1)).T) < 1e-12
    # without z / zy: NumPy's global generator, so a seed reproduces the run
    np.random.seed(3)
    a = hadamard.test_predsample_SVC_hadamard(*hist, t(xs), t(lab), *h)
    np.random.seed(3)
    b = hadamard.test_predsample_SVC_hadamard(*hist, t(xs), t(lab), *h)
    assert torch.equal(a, b) and not torch.equal(a, yt)
    with pytest.raises(ValueError):
        hadamard.test_predsample_SVC_hadamard(*hist, t(xs), t(lab), *h, z=z[:, :, :2])
    # the corrected held-out MAP predictor: one draw, no noise; the reference's numbers where the reference is right
    names = ("mu_tilde_l", "alpha_tilde_l", "beta_tilde_l", "mu_L", "alpha_L", "beta_L")
    m, v = hadamard.indexed_predict(t(g["pars"][:N]), t(g["pars"][N:N + N * T]), t(g["pars"][-1:])[0], t(g["x"]), t(g["indx"]), t(g["y"]),
                                    t(g["x_test"]), t(g["indx_test"]), **dict(zip(names, h)))
    assert tuple(m.shape) == tuple(v.shape) == (12,) and m.dtype == v.dtype == torch.float64
    zero = g["indx_test"] == 0
    assert relerr(m.numpy(), g["mean"]) < RESTATE_TOL and relerr(v.numpy()[zero], g["var"][zero]) < RESTATE_TOL
    with pytest.raises(TypeError):
        hadamard.indexed_predict(*[None] * 8, mu_tilde_l=0.0)


def test_names_are_the_packages_own():
    from nonstationary_multivariate_gaussian_process_amd import hadamard
    HYP = ["mu_tilde_l", "alpha_tilde_l", "beta_tilde_l", "mu_L", "alpha_L", "beta_L"]
    HIST = ["tilde_l_hist", "L_vecs_hist", "tilde_sigma2_err_hist", "x", "indx", "y"]
    want = {"point_predsample_SVC_hadamard": HIST + ["x_star"] + HYP, "pointwise_predsample_SVC_hadamard": HIST + ["grids"] + HYP,
            "indexedpoint_predsample_SVC_hadamard": HIST + ["x_star", "indx_star"] + HYP,
            "test_predsample_SVC_hadamard": HIST + ["x_test", "indx_test"] + HYP}
    for fn, params in want.items():
        sig = inspect.signature(getattr(hadamard, fn))
        assert list(sig.parameters) == params + ["z", "zy"], fn
        assert sig.parameters["z"].default is None and sig.parameters["zy"].default is None
    assert hadamard.test_predsample_SVC_hadamard.__test__ is False
    assert list(inspect.signature(hadamard.indexed_predict).parameters) == ["tilde_l", "L_vecs", "tilde_sigma2_err", "x", "indx", "y",
                                                                            "x_test", "indx_test", "hyper"]
    # not installed under the reference's module names: the served set is what it was
    assert hadamard.PREDICTION_NAMES == ("point_predmap_SVC_hadamard", "pointwise_predmap_SVC_hadamard")
    assert not any("predsample" in n or n == "indexed_predict" for n in hadamard.LOGPOS_NAMES + hadamard.PREDICTION_NAMES)


def test_abi_declares_and_binds_the_entry():
    from nonstationary_multivariate_gaussian_process_amd import _lib, build, drivers
    header = open(os.path.join(ROOT, "include", "nmgp.h")).read()
    assert "nmgp_predsample_had" in _lib.SIGNATURES and "int nmgp_predsample_had(" in header
    assert len(_lib.SIGNATURES["nmgp_predsample_had"][1]) == 13
    assert _lib.SIGNATURES["nmgp_predsample_had"] == _lib.SIGNATURES["nmgp_predsample_hads"]
    assert list(inspect.signature(_lib.Context.predsample_had).parameters) == ["self", "pars_hist", "hyper", "xs", "indx_star", "z", "star"]
    assert "nmgp_predsample_had.hip" in build.SOURCES
    sig = inspect.signature(drivers.posterior_predict_hadamard)
    assert list(sig.parameters) == ["x", "indx", "y", "hyper_pars", "samples", "xs", "indx_star", "draws", "seed", "ctx"]
    assert [sig.parameters[k].default for k in ("indx_star", "draws", "seed", "ctx")] == [None, None, 0, None]


# ---- (g) the driver's correlation summary -------------------------------------------------------------------------------------------------
def test_correlation_quantiles_are_correlations():
    from nonstationary_multivariate_gaussian_process_amd import drivers
    rng = np.random.default_rng(6)
    H, S, M = 9, 4, 3
    L_star = rng.standard_normal((H, S, M * (M + 1) // 2))
    q = drivers.correlation_quantiles(L_star, M)
    assert q.shape == (3, S, M, M)
    np.testing.assert_allclose(np.einsum("qsmm->qsm", q), 1.0, rtol=0, atol=1e-14)
    assert np.all(q <= 1.0 + 1e-14) and np.all(q >= -1.0 - 1e-14) and np.all(np.diff(q, axis=0) >= 0)
    np.testing.assert_allclose(q, np.swapaxes(q, -1, -2), rtol=0, atol=1e-15)
    # one draw: the quantiles are that draw's cov2cor(L L^T)
    L = np.zeros((M, M))
    L[np.tril_indices(M)] = L_star[0, 0]
    B = L @ L.T
    d = np.sqrt(np.diag(B))
    np.testing.assert_allclose(drivers.correlation_quantiles(L_star[:1, :1], M)[1, 0], B / np.outer(d, d), rtol=1e-14)


def test_driver_summary_on_the_restatement(monkeypatch):
    from nonstationary_multivariate_gaussian_process_amd import drivers
    from conftest import SVC_KEYS, hyper_dict
    host, calls = _fake_context(monkeypatch)
    case = (8, 8, "interleaved")
    c = pc.subject(case)
    xs, lab = pc.new_inputs(case)
    S, M, T = xs.shape[0], c["M"], c["T"]
    samples = np.stack([c["draws"][k % 2] + 0.001 * k for k in range(6)])
    for ix in (None, lab):
        out = drivers.posterior_predict_hadamard(c["x"], c["indx"], c["y"], hyper_dict(c["hyper"], SVC_KEYS), samples, xs, indx_star=ix,
                                                 seed=4, ctx=host)
        shape = (S, M) if ix is None else (S,)
        assert out["n_used"] == 6 and out["n_failed"] == 0 and out["mean"].shape == out["var"].shape == shape
        assert out["L_star"].shape == (6, S, T) and out["corr_quantiles"].shape == (3, S, M, M) and out["tilde_l_star"].shape == (6, S)
        np.testing.assert_allclose(np.einsum("qsmm->qsm", out["corr_quantiles"]), 1.0, rtol=0, atol=1e-14)
        assert np.all(np.abs(out["corr_quantiles"]) <= 1.0 + 1e-14)
    assert calls == [(6, S), (6, S)]
