"""Posterior-draw prediction on the GPU (nmgp_predsample_svc, predsample.py, drivers.posterior_predict) against the reference's
recorded runs (tests/golden/predsample_*.npz), the deterministic predictor, the NumPy restatement of test_predsample_cpu.py, and
itself across batch sizes, chunk sizes and grid slices.  Bars as in test_predsample_cpu.py; the bar against nmgp_predict_svc
(rtol 1e-9, atol 1e-11) is the one test_gpu_parity.py uses between the custom and the rocSOLVER schedules."""
import numpy as np
import pytest
import torch

from conftest import SVC_KEYS, golden, record_parity
from test_predsample_cpu import MEAN_TOL, STAR_TOL, VAR_TOL, diag_slots, restate

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from nonstationary_multivariate_gaussian_process_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def hm(a):
    """[S, H, ...] <-> [H, S, ...]"""
    return np.ascontiguousarray(np.swapaxes(a, 0, 1))


def maxrel(a, b, floor):
    return float(np.max(np.abs(a - b) / (np.abs(b) + floor)))


def smooth_draws(p0, x, N, T, H, amp=0.05):
    out = []
    for k in range(H):
        p = p0.copy()
        p[:N] += amp * np.sin(3.0 * x + 0.4 + k)
        p[N:N + N * T] += (amp * np.sin(3.0 * x[:, None] + 0.4 + k + np.arange(T)[None, :])).reshape(-1)
        p[-1] += 0.01 * k
        out.append(p)
    return np.stack(out)


def same_bits(a, b):
    return all(np.array_equal(u, v, equal_nan=True) for u, v in zip(a, b))


# ---- 1. the reference's recorded runs ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["predsample_N64_M3", "predsample_N512_M3"])
def test_entry_reproduces_the_references_moments_and_latent_samples(ctx, name):
    g = golden(name)
    M = g["Y"].shape[1]
    T = M * (M + 1) // 2
    ctx.set_data(g["x"], g["Y"])
    fams = [("ps", g["draws"], True)]
    if "sm_z" in g:
        fams.append(("sm", np.repeat(g["sm_pars"][None], int(g["sm_n_sample"]), axis=0), False))
    for fam, pars, constrained in fams:
        z, loc, scale = g[fam + "_z"], g[fam + "_loc"], g[fam + "_scale"]
        mean, var, star, status = ctx.predsample_svc(pars, g["hyper"], g["xs"], z=hm(z[:, :, :1 + T]), constrained=constrained)
        assert np.all(status == 0)
        mean, var, star = hm(mean), hm(var), hm(star)
        want = loc[:, :, :1 + T] + scale[:, :, :1 + T] * z[:, :, :1 + T]
        if not constrained:
            want[:, :, 1 + diag_slots(M)] = np.exp(want[:, :, 1 + diag_slots(M)])
        print(name, fam, "mean", maxrel(mean, loc[:, :, 1 + T:], 1e-2), "var", maxrel(var, scale[:, :, 1 + T:] ** 2, 0.0),
              "star abs", float(np.max(np.abs(star - want))))
        record_parity("%s_%s_entry" % (name, fam), mean=(maxrel(mean, loc[:, :, 1 + T:], 1e-2), 1e-5),
                      var=(maxrel(var, scale[:, :, 1 + T:] ** 2, 0.0), 1e-5), star_abs=(float(np.max(np.abs(star - want))), 1e-6))
        np.testing.assert_allclose(star, want, **STAR_TOL)
        np.testing.assert_allclose(mean, loc[:, :, 1 + T:], **MEAN_TOL)
        np.testing.assert_allclose(var, scale[:, :, 1 + T:] ** 2, **VAR_TOL)


def hist_args(g, N, T):
    t = torch.from_numpy
    d = g["draws"]
    return (t(d[:, :N].copy()), t(d[:, N:N + N * T].copy()), t(d[:, -1].copy()), t(g["Y"]), t(g["x"]))


@pytest.mark.parametrize("name", ["predsample_N64_M3", "predsample_N512_M3"])
def test_predsample_functions_return_the_references_samples(name):
    from nonstationary_multivariate_gaussian_process_amd import predsample as ps
    g = golden(name)
    N, M = g["Y"].shape
    T = M * (M + 1) // 2
    hv = [float(v) for v in g["hyper"][:6]]
    S, H = g["ps_y"].shape[:2]
    args = hist_args(g, N, T)
    ys = ps.pointwise_predsample_inhomogeneous(*args, torch.from_numpy(g["xs"]), *hv, N_sample=H, z=g["ps_z"])
    assert isinstance(ys, np.ndarray) and ys.shape == (S, H, M) and ys.dtype == np.float64
    record_parity(name + "_pointwise_samples", y=(maxrel(ys, g["ps_y"], 1e-2), 1e-5))
    np.testing.assert_allclose(ys, g["ps_y"], **MEAN_TOL)
    yt = ps.test_predsample_inhomogeneous(*args, torch.from_numpy(g["xs"]), *hv, H, z=g["ps_z"])
    assert np.array_equal(yt, ys)
    # N_sample takes the LAST draws of the history; the point function returns a tensor [N_hist, M]
    y1 = ps.point_predsample_inhomogeneous(*args, torch.tensor(g["xs"][2]), *hv, N_sample=4, z=g["ps_z"][2:3, -4:])
    assert isinstance(y1, torch.Tensor) and y1.dtype == torch.float64 and tuple(y1.shape) == (4, M)
    np.testing.assert_allclose(y1.numpy(), g["ps_y"][2, -4:], **MEAN_TOL)


def test_sampling_functions_return_the_references_summaries():
    from nonstationary_multivariate_gaussian_process_amd import predsample as ps
    g = golden("predsample_N64_M3")
    N, M = g["Y"].shape
    T = M * (M + 1) // 2
    t = torch.from_numpy
    p = g["sm_pars"]
    n = int(g["sm_n_sample"])
    S = len(g["xs"])
    hv = [float(v) for v in g["hyper"][:6]]
    args = (n, t(p[:N].copy()), t(p[N:N + N * T].copy()), t(p[-1:].copy())[0], t(g["Y"]), t(g["x"]))
    q, mean, std = ps.pointwise_predmap_inhomogeneous_sampling(*args, t(g["xs"]), *hv, z=g["sm_z"])
    assert q.shape == (S, 2, M) and mean.shape == (S, M) and std.shape == (S, M)
    record_parity("predsample_N64_M3_sampling_summaries", q=(maxrel(q, g["sm_q"], 1e-2), 1e-5), mean=(maxrel(mean, g["sm_mean"], 1e-2), 1e-5),
                  std=(maxrel(std, g["sm_std"], 0.0), 1e-5))
    np.testing.assert_allclose(q, g["sm_q"], **MEAN_TOL)
    np.testing.assert_allclose(mean, g["sm_mean"], **MEAN_TOL)
    np.testing.assert_allclose(std, g["sm_std"], **MEAN_TOL)
    qt = ps.test_predmap_inhomogeneous_sampling(*args, t(g["xs"]), *hv, z=g["sm_z"])
    assert same_bits(qt, (q, mean, std))
    tl = ps.pointwise_predmap_inhomogeneous_sampling(*args, t(g["xs"]), *hv, pred_smoothness=True, z=g["sm_z_smooth"])
    assert isinstance(tl, np.ndarray) and tl.shape == (S, n)
    np.testing.assert_allclose(tl, g["sm_tl"], **STAR_TOL)
    Lf = ps.pointwise_predmap_inhomogeneous_sampling(*args, t(g["xs"]), *hv, pred_cov=True, z=g["sm_z_cov"])
    assert Lf.shape == (S, n, M, M)
    np.testing.assert_allclose(Lf, g["sm_Lf"], **STAR_TOL)
    q1, m1, s1 = ps.point_predmap_inhomogeneous_sampling(*args, t(g["xs"])[3], *hv, z=g["sm_z"][3:4])
    assert q1.shape == (2, M) and m1.shape == (M,) and s1.shape == (M,)
    np.testing.assert_allclose(q1, g["sm_q"][3], **MEAN_TOL)
    assert ps.point_predmap_inhomogeneous_sampling(*args, t(g["xs"])[3], *hv, pred_smoothness=True, z=g["sm_z_smooth"][3:4]).shape == (n,)
    # without z the normals come from torch's global generator: a seed reproduces the run
    torch.manual_seed(5)
    a = ps.pointwise_predmap_inhomogeneous_sampling(*args, t(g["xs"]), *hv)
    torch.manual_seed(5)
    b = ps.pointwise_predmap_inhomogeneous_sampling(*args, t(g["xs"]), *hv)
    assert same_bits(a, b) and not np.array_equal(a[1], mean)


# ---- 2. no noise, one draw: the deterministic predictor ------------------------------------------------------------------
@pytest.mark.parametrize("name,xkey", [("pred_N64_M3", "xs"), ("pred_N512_M3_grid201", "grids")])
def test_without_noise_one_draw_is_the_deterministic_predictor(ctx, name, xkey):
    g = golden(name)
    xs = g[xkey]
    ctx.set_data(g["x"], g["Y"])
    m0, v0, L0 = ctx.predict_svc(g["svc_pars"], g["svc_hyper"], xs)
    mean, var, star, status = ctx.predsample_svc(g["svc_pars"], g["svc_hyper"], xs, constrained=False)
    assert status.tolist() == [0] and mean.shape == (1,) + m0.shape
    record_parity(name + "_predsample_vs_predict_svc", mean=(maxrel(mean[0], m0, 1e-2), 1e-9), var=(maxrel(var[0], v0, 0.0), 1e-9),
                  Lstar=(maxrel(star[0][:, 1:], L0, 1e-2), 1e-9))
    np.testing.assert_allclose(mean[0], m0, rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(var[0], v0, rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(star[0][:, 1:], L0, rtol=1e-9, atol=1e-11)
    # the caller's starred values: predict_svc's own Lstar and the regressed tilde_l*
    sin = np.concatenate([star[0][:, :1], L0], axis=1)[None]
    m2, v2, s2, st2 = ctx.predsample_svc(g["svc_pars"], g["svc_hyper"], xs, star=sin, constrained=False)
    assert st2.tolist() == [0] and np.array_equal(s2, sin)
    np.testing.assert_allclose(m2[0], m0, rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(v2[0], v0, rtol=1e-9, atol=1e-11)
    from nonstationary_multivariate_gaussian_process_amd import _lib
    with pytest.raises(_lib.NmgpError):
        ctx.predsample_svc(g["svc_pars"], g["svc_hyper"], xs, z=np.zeros_like(sin), star=sin)


# ---- 3. batch == single, on both sides of the factorisation's schedule line --------------------------------------------------
def test_a_batch_of_draws_gives_the_bits_of_single_draw_calls(ctx, monkeypatch):
    """N = 512, D = 3 (n = 1536): 8 draws factor in the latency schedule of the blocked Cholesky (batch n <= 73,728), 56 draws in
    the throughput schedule, with 63 cross-covariance rows riding below every matrix."""
    monkeypatch.delenv("NMGP_PREDSAMPLE_CHUNK", raising=False)
    g = golden("predsample_N512_M3")
    N, M = g["Y"].shape
    T = M * (M + 1) // 2
    H = 56
    draws = np.concatenate([smooth_draws(g["draws"][0], g["x"], N, T, 28, 0.01), smooth_draws(g["draws"][5], g["x"], N, T, 28, 0.02)])
    xs = np.linspace(0.0, 1.0, 201)[::10]
    z = np.random.default_rng(31).standard_normal((H, len(xs), 1 + T))
    ctx.set_data(g["x"], g["Y"])
    big = ctx.predsample_svc(draws, g["hyper"], xs, z=z)
    assert np.all(big[3] == 0)
    small = ctx.predsample_svc(draws[:8], g["hyper"], xs, z=z[:8])
    assert same_bits([a[:8] for a in big], small)
    for k in (0, 7, 8, 31, 55):
        one = ctx.predsample_svc(draws[k:k + 1], g["hyper"], xs, z=z[k:k + 1])
        assert same_bits([a[k:k + 1] for a in big], one), k
    monkeypatch.setenv("NMGP_PREDSAMPLE_CHUNK", "8")
    chunked = ctx.predsample_svc(draws, g["hyper"], xs, z=z)
    monkeypatch.delenv("NMGP_PREDSAMPLE_CHUNK")
    assert same_bits(big, chunked)
    pick = [3, 29, 55]
    mean, var, star = restate(g["x"], g["Y"], draws[pick], g["hyper"], xs, hm(z[pick]), True)
    np.testing.assert_allclose(big[2][pick], hm(star), **STAR_TOL)
    np.testing.assert_allclose(big[0][pick], hm(mean), **MEAN_TOL)
    np.testing.assert_allclose(big[1][pick], hm(var), **VAR_TOL)


# ---- 4. the headline size ------------------------------------------------------------------------------------------------
def test_headline_size_in_the_throughput_schedule_against_the_restatement(ctx):
    """N = 2048, D = 3: the 8 `pars_typical` positions of the sampler twice (16 draws of order 6144: throughput schedule), the
    201-point grid (603 riding rows), a fixed z; two draws x four grid points against the restatement (one 6144^2 solve each)."""
    from nonstationary_multivariate_gaussian_process_amd import sim
    N, M = 2048, 3
    T = M * (M + 1) // 2
    d = sim.simulate_nonseparable(N, M, seed=2222)
    draws = np.concatenate([golden("hmc_state_N2048_M3_seed2222")["pars_typical"]] * 2)
    hv = np.array([sim.HYPER_SVC[k] for k in SVC_KEYS])
    xs = np.linspace(0.0, 1.0, 201)
    z = np.random.default_rng(77).standard_normal((16, 201, 1 + T))
    z[8:] = z[:8]
    ctx.set_data(d["x"], d["Y"])
    mean, var, star, status = ctx.predsample_svc(draws, hv, xs, z=z)
    assert np.all(status == 0) and np.all(var > 0)
    assert same_bits([mean[:8], var[:8], star[:8]], [mean[8:], var[8:], star[8:]])
    dr, pick = [1, 14], np.array([5, 77, 100, 196])
    mo, vo, so = restate(d["x"], d["Y"], draws[dr], hv, xs[pick], hm(z[dr][:, pick]), True)
    gm, gv, gs = mean[dr][:, pick], var[dr][:, pick], star[dr][:, pick]
    print("headline: mean", maxrel(gm, hm(mo), 1e-2), "var", maxrel(gv, hm(vo), 0.0), "star abs", float(np.max(np.abs(gs - hm(so)))))
    record_parity("predsample_N2048_M3_grid201_restatement", mean=(maxrel(gm, hm(mo), 1e-2), 1e-5), var=(maxrel(gv, hm(vo), 0.0), 1e-5),
                  star_abs=float(np.max(np.abs(gs - hm(so)))))
    np.testing.assert_allclose(gm, hm(mo), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(gv, hm(vo), rtol=1e-5, atol=1e-9)


# ---- 5. more grid outputs than riding rows ---------------------------------------------------------------------------------
def test_grid_slices_against_the_restatement(ctx):
    g = golden("svc_rngfree_N16_M1")                       # n = 16 riding rows at most: S = 20 goes through in two slices
    N, M = g["Y"].shape
    T = M * (M + 1) // 2
    draws = smooth_draws(g["pars"], g["x"], N, T, 3)
    xs = np.linspace(0.03, 0.97, 20)
    z = np.random.default_rng(9).standard_normal((3, 20, 1 + T))
    ctx.set_data(g["x"], g["Y"])
    for constrained in (True, False):
        mean, var, star, status = ctx.predsample_svc(draws, g["hyper"], xs, z=z, constrained=constrained)
        mo, vo, so = restate(g["x"], g["Y"], draws, g["hyper"], xs, hm(z), constrained)
        assert np.all(status == 0)
        np.testing.assert_allclose(star, hm(so), **STAR_TOL)
        np.testing.assert_allclose(mean, hm(mo), **MEAN_TOL)
        np.testing.assert_allclose(var, hm(vo), **VAR_TOL)
        # slices do not change a grid point's bits
        head = ctx.predsample_svc(draws, g["hyper"], xs[:7], z=z[:, :7], constrained=constrained)
        assert same_bits([mean[:, :7], var[:, :7], star[:, :7]], head[:3])


def test_prediction_at_the_training_inputs(ctx):
    """test_predsample_inhomogeneous(..., x_test = x): S = N, as many riding rows as the matrix has (one slice)."""
    g = golden("predsample_N64_M3")
    N, M = g["Y"].shape
    T = M * (M + 1) // 2
    draws = g["draws"][:3]
    z = np.random.default_rng(13).standard_normal((3, N, 1 + T))
    ctx.set_data(g["x"], g["Y"])
    mean, var, star, status = ctx.predsample_svc(draws, g["hyper"], g["x"], z=z)
    mo, vo, so = restate(g["x"], g["Y"], draws, g["hyper"], g["x"], hm(z), True)
    assert np.all(status == 0)
    np.testing.assert_allclose(star, hm(so), **STAR_TOL)
    np.testing.assert_allclose(mean, hm(mo), **MEAN_TOL)
    np.testing.assert_allclose(var, hm(vo), **VAR_TOL)


# ---- 6. a draw that fails numerically ------------------------------------------------------------------------------------
def test_a_failing_draw_is_reported_and_leaves_the_others_alone(ctx):
    g = golden("predsample_N64_M3")
    N, M = g["Y"].shape
    T = M * (M + 1) // 2
    z = hm(g["ps_z"][:, :, :1 + T])
    bad = g["draws"].copy()
    bad[2, N + 5] = np.nan
    ctx.set_data(g["x"], g["Y"])
    good = ctx.predsample_svc(g["draws"], g["hyper"], g["xs"], z=z)
    mean, var, star, status = ctx.predsample_svc(bad, g["hyper"], g["xs"], z=z)       # returns: no exception
    assert status[2] != 0 and np.all(np.isnan(mean[2])) and np.all(np.isnan(var[2]))
    keep = [0, 1, 3, 4, 5]
    assert np.all(status[keep] == 0)
    assert same_bits([mean[keep], var[keep], star[keep]], [a[keep] for a in good[:3]])


# ---- 7. the batch's state --------------------------------------------------------------------------------------------------
def test_the_call_leaves_batched_evaluations_and_a_begun_trajectory_alone():
    """The entry has its own workspace: a batched evaluation after it repeats the one before it bit for bit, and a trajectory
    begun before it continues as if the call had not happened."""
    from nonstationary_multivariate_gaussian_process_amd import _lib
    g = golden("predsample_N64_M3")
    N, M = g["Y"].shape
    T = M * (M + 1) // 2
    B = 4
    pars = g["draws"][:B]
    p0 = np.random.default_rng(3).standard_normal(pars.shape)

    def run(with_prediction):
        c = _lib.Context(0)
        try:
            c.set_data(g["x"], g["Y"])
            c.svc_batch_alloc(B)
            c.svc_batch_set_pars(pars)
            c.svc_batch_eval(g["hyper"], True, False)
            v0 = c.svc_batch_fetch()
            c.svc_batch_eval(g["hyper"], True, True)
            v1, g1 = c.svc_batch_fetch(), c.svc_batch_fetch_grad()
            c.svc_batch_traj_begin()
            pred = c.predsample_svc(g["draws"], g["hyper"], g["xs"], z=hm(g["ps_z"][:, :, :1 + T])) if with_prediction else None
            gafter = c.svc_batch_fetch_grad()                       # the pending evaluation is still the batch's last one
            traj = c.svc_batch_traj(g["hyper"], True, 1e-4, 3, p0)
            c.svc_batch_set_pars(pars)
            c.svc_batch_eval(g["hyper"], True, False)
            w0 = c.svc_batch_fetch()
            c.svc_batch_eval(g["hyper"], True, True)
            w1, h1 = c.svc_batch_fetch(), c.svc_batch_fetch_grad()
        finally:
            c.close()
        assert same_bits(v0, w0) and same_bits(v1, w1) and np.array_equal(g1, h1) and np.array_equal(g1, gafter)
        return traj, pred

    t_plain, _ = run(False)
    t_pred, pred = run(True)
    assert np.all(pred[3] == 0)
    assert same_bits(t_plain, t_pred)


# ---- 8. the driver -----------------------------------------------------------------------------------------------------
def test_posterior_predict_on_the_fixture_draws(ctx):
    from nonstationary_multivariate_gaussian_process_amd import drivers, sim
    g = golden("predsample_N64_M3")
    N, M = g["Y"].shape
    h = dict(zip(SVC_KEYS, g["hyper"]))
    S = len(g["xs"])
    samples = g["draws"].reshape(3, 2, -1)                     # [iters, chains, P]
    a = drivers.posterior_predict(g["x"], g["Y"], h, samples, g["xs"], seed=4, ctx=ctx)
    assert a["mean"].shape == (S, M) and a["var"].shape == (S, M) and a["quantiles"].shape == (3, S, M)
    assert a["tilde_l_star"].shape == (6, S) and a["status"].tolist() == [0] * 6 and a["n_used"] == 6 and a["n_failed"] == 0
    assert np.all(a["quantiles"][0] <= a["quantiles"][1]) and np.all(a["quantiles"][1] <= a["quantiles"][2])
    # total variance = mean of the per-draw variances + variance of the per-draw means, from the entry's own moments
    z = np.random.default_rng(4).standard_normal((6, S, 1 + M * (M + 1) // 2))
    mean, var, _, _ = ctx.predsample_svc(g["draws"], g["hyper"], g["xs"], z=z)
    np.testing.assert_allclose(a["mean"], mean.mean(axis=0), rtol=1e-13)
    np.testing.assert_allclose(a["var"], var.mean(axis=0) + mean.var(axis=0), rtol=1e-13)
    assert np.all(a["var"] >= var.mean(axis=0))
    b = drivers.posterior_predict(g["x"], g["Y"], h, samples, g["xs"], seed=4, ctx=ctx)
    assert all(np.array_equal(a[k], b[k]) for k in ("mean", "var", "quantiles", "tilde_l_star"))
    c = drivers.posterior_predict(g["x"], g["Y"], h, samples, g["xs"], seed=5, ctx=ctx)
    assert not np.array_equal(a["quantiles"], c["quantiles"])
    thin = drivers.posterior_predict(g["x"], g["Y"], h, g["draws"], g["xs"], draws=3, seed=4, ctx=ctx)
    assert thin["n_used"] == 3 and thin["tilde_l_star"].shape == (3, S)
