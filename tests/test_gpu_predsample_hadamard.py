"""Posterior-draw prediction of the separable Hadamard model on the GPU (nmgp_predsample_hads, predsample_hadamard.py,
drivers.posterior_predict_hadamard_sep) against the reference's recorded runs (tests/golden/hps_*.npz), the deterministic predictor
nmgp_predict_hads, and itself across forms (indexed against full), batch sizes and chunk sizes.

Bars.  Against the recorded runs: the project's standing prediction bar, 1e-5 relative element by element (conftest.relerr).
Against nmgp_predict_hads with one draw and no noise: mean, variance and starred values bit for bit -- every piece shares the
predictor's arithmetic, the factorisation included (both run the substitution-based panel kernels, whose bits do not depend on the
schedule the batch size selects).  Indexed against full under the same starred values: 1e-10 relative (whether it
is bit-identical is printed).  Batch against single calls, chunk against chunk: bit for bit."""
import numpy as np
import pytest
import torch

from conftest import SEP_KEYS, golden, hyper_dict, record_parity, relerr
from test_predsample_hadamard_cpu import CASES

pytestmark = pytest.mark.gpu

PRED_TOL = 1e-5


@pytest.fixture(scope="module")
def ctx():
    from nonstationary_multivariate_gaussian_process_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def resident(ctx, g):
    ctx.had_set_data(g["x"], g["indx"], g["y"])


def dm(a):
    """[S, H, ...] (the reference's point-major order) <-> [H, S, ...] (the entry's draw-major order)"""
    return np.ascontiguousarray(np.swapaxes(a, 0, 1))


def same_bits(a, b):
    return all(np.array_equal(u, v, equal_nan=True) for u, v in zip(a, b))


def smooth_chains(p0, x, N, T, B, amp=0.05):
    """test_gpu_hadamard_sep.smooth_chains"""
    out = []
    for k in range(B):
        p = p0.copy()
        p[:N] += amp * np.sin(3.0 * x + 0.4 + k)
        p[N:2 * N] += amp * np.cos(2.0 * x + 0.3 * k)
        p[2 * N:2 * N + T] += amp * np.sin(0.7 + k + np.arange(T))
        p[-1] += 0.01 * k
        out.append(p)
    return np.stack(out)


# ---- 1. the reference's recorded runs, both forms -------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_entry_and_names_reproduce_the_recorded_runs(ctx, name):
    from nonstationary_multivariate_gaussian_process_amd import predsample_hadamard as psh
    g = golden(name)
    N, M = g["x"].shape[0], int(g["M"])
    T = M * (M + 1) // 2
    H = g["draws"].shape[0]
    resident(ctx, g)
    errs = {}
    for tag, xs, lab, z, loc, scale, ys in (("ps", g["grids"], None, g["ps_z"], g["ps_loc"], g["ps_scale"], g["ps_y"]),
                                            ("ix", g["x_test"], g["indx_test"], g["ix_z"], g["ix_loc"], g["ix_scale"], g["ix_y"][:, :, None])):
        mean, var, star, status = ctx.predsample_hads(g["draws"], g["hyper"], xs, indx_star=lab, z=dm(z[:, :, :2]))
        assert status.tolist() == [0] * H and star.shape == (H, len(xs), 2)
        assert mean.shape == var.shape == ((H, len(xs), M) if lab is None else (H, len(xs)))
        mean, var = dm(mean).reshape(loc[:, :, 2:].shape), dm(var).reshape(loc[:, :, 2:].shape)
        _, _, star0, _ = ctx.predsample_hads(g["draws"], g["hyper"], xs, indx_star=lab)          # the conditional means
        errs.update({tag + "_mean": relerr(mean, loc[:, :, 2:]), tag + "_var": relerr(var, scale[:, :, 2:] ** 2),
                     tag + "_star": relerr(dm(star), loc[:, :, :2] + scale[:, :, :2] * z[:, :, :2]),
                     tag + "_star_mean": relerr(dm(star0), loc[:, :, :2]),
                     tag + "_y": relerr(mean + np.sqrt(var) * z[:, :, 2:], ys)})
    # the reference's names and shapes
    t = torch.from_numpy
    d = g["draws"]
    hist = (t(d[:, :N]), t(d[:, N:2 * N]), t(d[:, 2 * N:2 * N + T]), t(d[:, -1]), t(g["x"]), t(g["indx"]), t(g["y"]))
    h = [float(v) for v in g["hyper"][:6]]
    ys = psh.pointwise_predsample_hadamard(*hist, t(g["grids"]), *h, z=g["ps_z"])
    assert isinstance(ys, torch.Tensor) and tuple(ys.shape) == (9, H, M)
    errs["pointwise_predsample_hadamard"] = relerr(ys.numpy(), g["ps_y"])
    one = psh.point_predsample_hadamard(*hist, t(g["grids"][4:5])[0], *h, z=g["ps_z"][4:5])
    assert tuple(one.shape) == (H, M) and torch.equal(one, ys[4])
    St = len(g["x_test"])
    yt = psh.test_predsample_hadamard(*hist, t(g["x_test"]), t(g["indx_test"]), *h, z=g["ix_z"])
    assert isinstance(yt, torch.Tensor) and tuple(yt.shape) == (St, H)
    errs["test_predsample_hadamard"] = relerr(yt.numpy(), g["ix_y"])
    one = psh.indexedpoint_predsample_hadamard(*hist, t(g["x_test"][2:3])[0], t(g["indx_test"][2:3])[0], *h, z=g["ix_z"][2:3])
    assert tuple(one.shape) == (H,) and torch.equal(one, yt[2])
    # the MAP forms of the indexed predictor: one parameter vector, no noise
    pieces = (t(d[0, :N]), t(d[0, N:2 * N]), t(d[0, 2 * N:2 * N + T]), t(d[0, -1:])[0], t(g["x"]), t(g["indx"]), t(g["y"]))
    pct = psh.test_predmap_harmard(*pieces, t(g["x_test"]), t(g["indx_test"]), *h)
    assert tuple(pct.shape) == (St, 3) and pct.dtype == torch.float64
    errs["test_predmap_harmard"] = relerr(pct.numpy(), g["map_pct"])
    one = psh.indexedpoint_predmap_hadamard(*pieces, t(g["x_test"][2:3])[0], t(g["indx_test"][2:3])[0], *h)
    assert tuple(one.shape) == (3,) and torch.equal(one, pct[2])
    print(name, errs)
    record_parity(name, **{k: (e, PRED_TOL) for k, e in errs.items()})
    for k, e in errs.items():
        assert e < PRED_TOL, (name, k, e)
    # without z the numbers come from torch's global generator: a seed reproduces the run
    torch.manual_seed(11)
    a = psh.test_predsample_hadamard(*hist, t(g["x_test"]), t(g["indx_test"]), *h)
    torch.manual_seed(11)
    b = psh.test_predsample_hadamard(*hist, t(g["x_test"]), t(g["indx_test"]), *h)
    assert torch.equal(a, b) and not torch.equal(a, yt)


# ---- 2. one draw without noise is the deterministic predictor ------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_one_draw_without_noise_is_predict_hads(ctx, name):
    g = golden(name)
    resident(ctx, g)
    for k in (0, g["draws"].shape[0] - 1):
        m0, v0, s0 = ctx.predict_hads(g["draws"][k], g["hyper"], g["grids"])
        mean, var, star, status = ctx.predsample_hads(g["draws"][k], g["hyper"], g["grids"])
        assert status.tolist() == [0] and mean.shape == (1,) + m0.shape
        print(name, k, "against predict_hads: mean", relerr(mean[0], m0), "var", relerr(var[0], v0))
        assert np.array_equal(star[0], s0) and np.array_equal(mean[0], m0) and np.array_equal(var[0], v0)


# ---- 3. the indexed form against the full form ------------------------------------------------------------------------------------
def test_indexed_form_is_the_matching_column_of_the_full_form(ctx):
    """N = 77, M = 3: the full form slices at N / M = 25 grid points, so 30 points are two factorisations per draw there and one
    (30 <= N riding rows) in the indexed form."""
    g = golden("hps_N77_M3")
    resident(ctx, g)
    S, H, M = 30, 3, 3
    xs = np.linspace(-0.02, 1.02, S)
    lab = (np.arange(S) % M).astype(np.int32)
    assert S > 77 // M and sorted(set(lab.tolist())) == [0, 1, 2]
    z = np.random.default_rng(8).standard_normal((H, S, 2))
    mean, var, star, status = ctx.predsample_hads(g["draws"][:H], g["hyper"], xs, z=z)
    im, iv, istar, ist = ctx.predsample_hads(g["draws"][:H], g["hyper"], xs, indx_star=lab, star=star)
    assert status.tolist() == ist.tolist() == [0] * H and np.array_equal(istar, star) and im.shape == iv.shape == (H, S)
    fm, fv = mean[:, np.arange(S), lab], var[:, np.arange(S), lab]
    e_m, e_v = relerr(im, fm), relerr(iv, fv)
    print("indexed against full: mean", e_m, "var", e_v, "bit-identical", np.array_equal(im, fm) and np.array_equal(iv, fv))
    record_parity("hps_N77_M3/indexed_vs_full", mean=(e_m, 1e-10), var=(e_v, 1e-10))
    assert e_m < 1e-10 and e_v < 1e-10
    # regressing again with the same z gives the same starred values, hence the same numbers
    jm, jv, jstar, _ = ctx.predsample_hads(g["draws"][:H], g["hyper"], xs, indx_star=lab, z=z)
    assert np.array_equal(jstar, star) and np.array_equal(jm, im) and np.array_equal(jv, iv)
    from nonstationary_multivariate_gaussian_process_amd import _lib
    with pytest.raises(_lib.NmgpError):
        ctx.predsample_hads(g["draws"][:H], g["hyper"], xs, z=z, star=star)


# ---- 4. batch == single ---------------------------------------------------------------------------------------------------------------
def test_four_draws_give_the_bits_of_four_calls(ctx, monkeypatch):
    monkeypatch.delenv("NMGP_PREDSAMPLE_CHUNK", raising=False)
    g = golden("hps_N200_M4")
    resident(ctx, g)
    for xs, lab, z in ((g["grids"], None, g["ps_z"]), (g["x_test"], g["indx_test"], g["ix_z"])):
        z = dm(z[:, :, :2])
        big = ctx.predsample_hads(g["draws"], g["hyper"], xs, indx_star=lab, z=z)
        assert big[3].tolist() == [0] * 4
        for k in range(4):
            one = ctx.predsample_hads(g["draws"][k], g["hyper"], xs, indx_star=lab, z=z[k:k + 1])
            assert same_bits([a[k:k + 1] for a in big], one), k


def test_a_batch_gives_the_bits_of_smaller_batches_across_the_schedule_line(ctx, monkeypatch):
    """N = 1100: 8 draws are batch n = 8,800 <= 73,728, 72 draws in one chunk 79,200: the other side of the blocked Cholesky's
    schedule line.  The default chunking of 72 draws is 64 + 8; 30 + 30 + 12 and one chunk of 72 are run too."""
    monkeypatch.delenv("NMGP_PREDSAMPLE_CHUNK", raising=False)
    g = golden("hsep_N1100_M3")
    N, M = 1100, 3
    resident(ctx, g)
    draws = smooth_chains(g["pars"], g["x"], N, M * (M + 1) // 2, 72)
    xs = np.array([0.11, float(g["x"][N // 3]), 0.97])
    z = np.random.default_rng(9).standard_normal((72, 3, 2))
    small = [ctx.predsample_hads(draws[k:k + 8], g["hyper"], xs, z=z[k:k + 8]) for k in range(0, 72, 8)]
    small = [np.concatenate([s[i] for s in small]) for i in range(4)]
    assert small[3].tolist() == [0] * 72 and not np.array_equal(small[0][0], small[0][1])
    assert same_bits(ctx.predsample_hads(draws, g["hyper"], xs, z=z), small)
    for chunk in ("72", "30"):
        monkeypatch.setenv("NMGP_PREDSAMPLE_CHUNK", chunk)
        out = ctx.predsample_hads(draws, g["hyper"], xs, z=z)
        monkeypatch.delenv("NMGP_PREDSAMPLE_CHUNK")
        assert same_bits(out, small), chunk
    one = ctx.predsample_hads(draws[71], g["hyper"], xs, z=z[71:])
    assert same_bits([a[71:] for a in small], one)


# ---- 5. failure stays local -------------------------------------------------------------------------------------------------------------
def test_a_draw_that_is_not_finite_does_not_touch_its_neighbours(ctx):
    from nonstationary_multivariate_gaussian_process_amd import _lib
    g = golden("hps_N77_M3")
    resident(ctx, g)
    z = np.random.default_rng(10).standard_normal((3, 9, 2))
    bad = g["draws"][:3].copy()
    bad[1, 40] = np.nan
    for lab, xs in ((None, g["grids"]), (np.arange(9, dtype=np.int32) % 3, g["grids"])):
        mean, var, star, status = ctx.predsample_hads(bad, g["hyper"], xs, indx_star=lab, z=z)
        assert status.tolist() == [0, _lib.NUM_NAN, 0]
        assert np.all(np.isnan(mean[1])) and np.all(np.isnan(var[1]))
        clean = ctx.predsample_hads(bad[[0, 2]], g["hyper"], xs, indx_star=lab, z=z[[0, 2]])
        assert clean[3].tolist() == [0, 0] and np.all(np.isfinite(clean[0]))
        assert same_bits([a[[0, 2]] for a in (mean, var, star)], clean[:3])


# ---- 6. state ---------------------------------------------------------------------------------------------------------------------------
def test_state_and_argument_checks(ctx):
    from nonstationary_multivariate_gaussian_process_amd import _lib
    s = golden("svc_rngfree_N64_M3")
    g = golden("hps_N77_M3")
    ctx.set_data(s["x"], s["Y"])                                            # a complete-data subject is resident
    with pytest.raises(_lib.NmgpError, match="error -3"):                   # NMGP_E_STATE
        ctx.predsample_hads(np.zeros((1, 2 * 64 + 6 + 1)), g["hyper"], np.array([0.5]))
    resident(ctx, g)
    P = g["draws"][:2]
    before = ctx.hads_batch_eval(P, g["hyper"], want_grad=True)
    ctx.predsample_hads(g["draws"], g["hyper"], g["grids"])
    ctx.predsample_hads(g["draws"], g["hyper"], g["x_test"], indx_star=g["indx_test"])
    after = ctx.hads_batch_eval(P, g["hyper"], want_grad=True)
    assert before[2].tolist() == [0, 0] and same_bits(before, after)
    for lab in ([0, 1, 3], [0, -1, 2]):
        with pytest.raises(_lib.NmgpError, match="error -2"):               # NMGP_E_SHAPE: a label outside [0, M)
            ctx.predsample_hads(g["draws"], g["hyper"], g["grids"][:3], indx_star=lab)
    with pytest.raises(_lib.NmgpError):                                     # one label per new input
        ctx.predsample_hads(g["draws"], g["hyper"], g["grids"][:3], indx_star=[0, 1])
    with pytest.raises(_lib.NmgpError):                                     # the nonseparable layout's length is refused
        ctx.predsample_hads(np.zeros((1, 77 * 7 + 1)), g["hyper"], g["grids"])
    with pytest.raises(_lib.NmgpError):
        ctx.predsample_hads(g["draws"], g["hyper"], g["grids"], z=np.zeros((6, 9, 3)))
    # the entry still works after the refusals
    assert ctx.predsample_hads(g["draws"], g["hyper"], g["grids"])[3].tolist() == [0] * 6


# ---- 7. the driver -----------------------------------------------------------------------------------------------------------------------
def test_driver_summarises_twelve_draws_in_both_forms(ctx):
    from nonstationary_multivariate_gaussian_process_amd import drivers
    g = golden("hps_N77_M3")
    h = hyper_dict(g["hyper"], SEP_KEYS)
    N, M = 77, 3
    samples = smooth_chains(g["draws"][0], g["x"], N, 6, 24, 0.02).reshape(6, 4, -1)      # [iters, chains, P]
    used = samples.reshape(24, -1)[np.unique(np.round(np.linspace(0, 23, 12)).astype(int))]
    for xs, lab in ((g["grids"], None), (g["x_test"], g["indx_test"])):
        S = len(xs)
        a = drivers.posterior_predict_hadamard_sep(g["x"], g["indx"], g["y"], h, samples, xs, indx_star=lab, draws=12, seed=4, ctx=ctx)
        shape = (S, M) if lab is None else (S,)
        assert a["n_used"] == 12 and a["n_failed"] == 0 and a["mean"].shape == a["var"].shape == shape
        assert a["quantiles"].shape == (3,) + shape and a["tilde_l_star"].shape == a["tilde_sigma_star"].shape == (12, S)
        # total variance = mean of the per-draw variances + variance of the per-draw means, from the entry's own moments
        z = np.random.default_rng(4).standard_normal((12, S, 2))
        mean, var, star, _ = ctx.predsample_hads(used, g["hyper"], xs, indx_star=lab, z=z)
        np.testing.assert_allclose(a["mean"], mean.mean(axis=0), rtol=1e-13)
        np.testing.assert_allclose(a["var"], var.mean(axis=0) + mean.var(axis=0), rtol=1e-13)
        assert np.all(a["var"] >= var.mean(axis=0)) and np.array_equal(a["tilde_sigma_star"], star[:, :, 1])
        b = drivers.posterior_predict_hadamard_sep(g["x"], g["indx"], g["y"], h, samples, xs, indx_star=lab, draws=12, seed=4, ctx=ctx)
        assert all(np.array_equal(a[k], b[k]) for k in a if k not in ("n_used", "n_failed"))
        c = drivers.posterior_predict_hadamard_sep(g["x"], g["indx"], g["y"], h, samples, xs, indx_star=lab, draws=12, seed=5, ctx=ctx)
        assert not np.array_equal(a["quantiles"], c["quantiles"])
