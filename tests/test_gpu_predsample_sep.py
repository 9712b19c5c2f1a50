"""Posterior-draw prediction of the separable and the stationary model on the GPU (nmgp_predsample_sep / _sta, predsample_sep.py,
drivers.posterior_predict_separable) against the reference's recorded runs (tests/golden/predsample_sep_*.npz), the deterministic
predictors, the NumPy restatement of test_predsample_sep_cpu.py, and itself across batch sizes, chunk sizes and grid slices.
Bars as in test_predsample_cpu.py; the bar against nmgp_predict_sep / _sta (rtol 1e-9, atol 1e-11) is the one test_gpu_parity.py
uses between two device paths of the same arithmetic."""
import numpy as np
import pytest
import torch

from conftest import SEP_KEYS, golden, record_parity
from test_predsample_cpu import MEAN_TOL, STAR_TOL, VAR_TOL
from test_predsample_sep_cpu import restate_sep, restate_sta

pytestmark = pytest.mark.gpu
SAME = dict(rtol=1e-9, atol=1e-11)


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


def same_bits(a, b):
    return all(np.array_equal(u, v, equal_nan=True) for u, v in zip(a, b))


def sep_draws(p0, x, N, T, H, amp=0.05):
    out = []
    for k in range(H):
        p = p0.copy()
        p[:N] += amp * np.sin(3.0 * x + 0.4 + k)
        p[N:2 * N] += amp * np.sin(3.0 * x + 1.4 + k)
        p[2 * N:2 * N + T] += 0.4 * amp * np.cos(np.arange(T) + k)
        p[-1] += 0.01 * k
        out.append(p)
    return np.stack(out)


def sta_draws(p0, T, H):
    return np.stack([p0 + np.concatenate([[0.05 * np.sin(0.4 + k), 0.05 * np.sin(1.4 + k)], 0.02 * np.cos(np.arange(T) + k), [0.01 * k]])
                     for k in range(H)])


# ---- 1. the reference's recorded runs ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["predsample_sep_N64_M3", "predsample_sep_N512_M5"])
def test_entry_reproduces_the_references_moments_and_latent_samples(ctx, name):
    g = golden(name)
    ctx.set_data(g["x"], g["Y"])
    fams = [("ps", g["draws"], True)]
    if "sm_z" in g:
        fams.append(("sm", np.repeat(g["sm_pars"][None], int(g["sm_n_sample"]), axis=0), False))
    for fam, pars, kss_jitter in fams:
        z, loc, scale = g[fam + "_z"], g[fam + "_loc"], g[fam + "_scale"]
        mean, var, star, status = ctx.predsample_sep(pars, g["hyper"], g["xs"], z=hm(z[:, :, :2]), kss_jitter=kss_jitter)
        assert np.all(status == 0)
        mean, var, star = hm(mean), hm(var), hm(star)
        want = loc[:, :, :2] + scale[:, :, :2] * z[:, :, :2]
        em, ev, es = maxrel(mean, loc[:, :, 2:], 1e-2), maxrel(var, scale[:, :, 2:] ** 2, 0.0), float(np.max(np.abs(star - want)))
        print(name, fam, "mean", em, "var", ev, "star abs", es)
        record_parity("%s_%s_entry" % (name, fam), mean=(em, 1e-5), var=(ev, 1e-5), star_abs=(es, 1e-6))
        np.testing.assert_allclose(star, want, **STAR_TOL)
        np.testing.assert_allclose(mean, loc[:, :, 2:], **MEAN_TOL)
        np.testing.assert_allclose(var, scale[:, :, 2:] ** 2, **VAR_TOL)
        # the other family's a2 misses the bar: the fixture discriminates kss_jitter
        other = ctx.predsample_sep(pars, g["hyper"], g["xs"], z=hm(z[:, :, :2]), kss_jitter=not kss_jitter)[1]
        assert not np.allclose(hm(other), scale[:, :, 2:] ** 2, **VAR_TOL)


def test_stationary_entry_reproduces_the_references_moments(ctx):
    g = golden("predsample_sep_N64_M3")
    ctx.set_data(g["x"], g["Y"])
    mean, var, status = ctx.predsample_sta(g["sta_draws"], g["xs"])
    assert np.all(status == 0)
    em, ev = maxrel(mean, g["sta_mean"], 1e-2), maxrel(var, g["sta_sd"] ** 2, 0.0)
    print("stationary entry: mean", em, "var", ev)
    record_parity("predsample_sep_N64_M3_sta_entry", mean=(em, 1e-5), var=(ev, 1e-5))
    np.testing.assert_allclose(mean, g["sta_mean"], **MEAN_TOL)
    np.testing.assert_allclose(var, g["sta_sd"] ** 2, **VAR_TOL)


def hist_args(g, N, T):
    t = torch.from_numpy
    d = g["draws"]
    return (t(d[:, :N].copy()), t(d[:, N:2 * N].copy()), t(d[:, 2 * N:2 * N + T].copy()), t(d[:, -1].copy()), t(g["Y"]), t(g["x"]))


@pytest.mark.parametrize("name", ["predsample_sep_N64_M3", "predsample_sep_N512_M5"])
def test_predsample_functions_return_the_references_samples(name):
    from nonstationary_multivariate_gaussian_process_amd import predsample_sep as ps
    g = golden(name)
    N, M = g["Y"].shape
    T = M * (M + 1) // 2
    hv = [float(v) for v in g["hyper"][:6]]
    S, H = g["ps_y"].shape[:2]
    args = hist_args(g, N, T)
    ys = ps.pointwise_predsample(*args, torch.from_numpy(g["xs"]), *hv, N_sample=H, z=g["ps_z"])
    assert isinstance(ys, np.ndarray) and ys.shape == (S, H, M) and ys.dtype == np.float64
    record_parity(name + "_pointwise_samples", y=(maxrel(ys, g["ps_y"], 1e-2), 1e-5))
    np.testing.assert_allclose(ys, g["ps_y"], **MEAN_TOL)
    yt = ps.test_predsample(*args, torch.from_numpy(g["xs"]), *hv, H, z=g["ps_z"])
    assert np.array_equal(yt, ys)
    # N_sample takes the LAST draws of the history; the point function returns a tensor [N_hist, M]
    y1 = ps.point_predsample(*args, torch.tensor(g["xs"][2]), *hv, N_sample=4, z=g["ps_z"][2:3, -4:])
    assert isinstance(y1, torch.Tensor) and y1.dtype == torch.float64 and tuple(y1.shape) == (4, M)
    np.testing.assert_allclose(y1.numpy(), g["ps_y"][2, -4:], **MEAN_TOL)
    # the four histories are zipped: the shortest wins
    short = (args[0], args[1][:3], args[2], args[3]) + args[4:]
    y3 = ps.pointwise_predsample(*short, torch.from_numpy(g["xs"]), *hv, N_sample=H, z=g["ps_z"][:, :3])
    np.testing.assert_allclose(y3, g["ps_y"][:, :3], **MEAN_TOL)


def test_sampling_functions_return_the_references_summaries():
    from nonstationary_multivariate_gaussian_process_amd import predsample_sep as ps
    g = golden("predsample_sep_N64_M3")
    N, M = g["Y"].shape
    T = M * (M + 1) // 2
    t = torch.from_numpy
    p = g["sm_pars"]
    n = int(g["sm_n_sample"])
    S = len(g["xs"])
    hv = [float(v) for v in g["hyper"][:6]]
    args = (n, t(p[:N].copy()), t(p[N:2 * N].copy()), t(p[2 * N:2 * N + T].copy()), t(p[-1:].copy())[0], t(g["Y"]), t(g["x"]))
    q, mean, std = ps.pointwise_predmap_sampling(*args, t(g["xs"]), *hv, z=g["sm_z"])
    assert q.shape == (S, 2, M) and mean.shape == (S, M) and std.shape == (S, M)
    record_parity("predsample_sep_N64_M3_sampling_summaries", q=(maxrel(q, g["sm_q"], 1e-2), 1e-5),
                  mean=(maxrel(mean, g["sm_mean"], 1e-2), 1e-5), std=(maxrel(std, g["sm_std"], 0.0), 1e-5))
    np.testing.assert_allclose(q, g["sm_q"], **MEAN_TOL)
    np.testing.assert_allclose(mean, g["sm_mean"], **MEAN_TOL)
    np.testing.assert_allclose(std, g["sm_std"], **MEAN_TOL)
    qt = ps.test_predmap_sampling(*args, t(g["xs"]), *hv, z=g["sm_z"])
    assert same_bits(qt, (q, mean, std))
    q1, m1, s1 = ps.point_predmap_sampling(*args, t(g["xs"])[3], *hv, z=g["sm_z"][3:4])
    assert q1.shape == (2, M) and m1.shape == (M,) and s1.shape == (M,)
    np.testing.assert_allclose(q1, g["sm_q"][3], **MEAN_TOL)
    # without z the normals come from torch's global generator: a seed reproduces the run
    torch.manual_seed(5)
    a = ps.pointwise_predmap_sampling(*args, t(g["xs"]), *hv)
    torch.manual_seed(5)
    b = ps.pointwise_predmap_sampling(*args, t(g["xs"]), *hv)
    assert same_bits(a, b) and not np.array_equal(a[1], mean)


def test_stationary_functions_return_the_references_samples_also_under_numpys_seed():
    from nonstationary_multivariate_gaussian_process_amd import predsample_sep as ps
    g = golden("predsample_sep_N64_M3")
    M = g["Y"].shape[1]
    T = M * (M + 1) // 2
    t = torch.from_numpy
    d = g["sta_draws"]
    H, S = d.shape[0], len(g["xs"])
    args = (t(d[:, 0].copy()), t(d[:, 1].copy()), t(d[:, 2:2 + T].copy()), t(d[:, -1].copy()), t(g["Y"]), t(g["x"]), t(g["xs"]))
    ys = ps.pointwise_predsample_S(*args, z=g["sta_z"])
    assert isinstance(ys, np.ndarray) and ys.shape == (H, S, M) and ys.dtype == np.float64          # draw-major
    record_parity("predsample_sep_N64_M3_sta_samples", y=(maxrel(ys, g["sta_y"], 1e-2), 1e-5))
    np.testing.assert_allclose(ys, g["sta_y"], **MEAN_TOL)
    assert np.array_equal(ps.test_predsample_S(*args, z=g["sta_z"]), ys)
    # no z: NumPy's global generator, the reference's own stream
    np.random.seed(int(g["sta_seed"]))
    seeded = ps.test_predsample_S(*args)
    record_parity("predsample_sep_N64_M3_sta_seeded", y=(maxrel(seeded, g["sta_y_seeded"], 1e-2), 1e-5))
    np.testing.assert_allclose(seeded, g["sta_y_seeded"], **MEAN_TOL)
    # the histories are zipped
    short = (args[0][:2],) + args[1:]
    np.testing.assert_allclose(ps.pointwise_predsample_S(*short, z=g["sta_z"][:2]), g["sta_y"][:2], **MEAN_TOL)


# ---- 2. no noise, one draw: the deterministic predictors ------------------------------------------------------------------
@pytest.mark.parametrize("name,xkey,pre", [("pred_N64_M3", "xs", ""), ("pred_N512_M3_grid201", "grids", "sep_")])
def test_without_noise_one_draw_is_the_deterministic_predictor(ctx, name, xkey, pre):
    from nonstationary_multivariate_gaussian_process_amd import _lib
    g = golden(name)
    xs = g[xkey]
    ctx.set_data(g[pre + "x"], g[pre + "Y"])
    m0, v0 = ctx.predict_sep(g["sep_pars"], g["sep_hyper"], xs)
    mean, var, star, status = ctx.predsample_sep(g["sep_pars"], g["sep_hyper"], xs, kss_jitter=True)
    assert status.tolist() == [0] and mean.shape == (1,) + m0.shape and star.shape == (1, len(xs), 2)
    record_parity(name + "_predsample_vs_predict_sep", mean=(maxrel(mean[0], m0, 1e-2), 1e-9), var=(maxrel(var[0], v0, 0.0), 1e-9))
    np.testing.assert_allclose(mean[0], m0, **SAME)
    np.testing.assert_allclose(var[0], v0, **SAME)
    # star_in round-trips and reproduces the regression's result
    m2, v2, s2, st2 = ctx.predsample_sep(g["sep_pars"], g["sep_hyper"], xs, star=star, kss_jitter=True)
    assert st2.tolist() == [0] and np.array_equal(s2, star)
    assert np.array_equal(m2, mean) and np.array_equal(v2, var)
    with pytest.raises(_lib.NmgpError):
        ctx.predsample_sep(g["sep_pars"], g["sep_hyper"], xs, z=np.zeros_like(star), star=star)
    # the C entry's own check (NMGP_E_STATE), past the binding's
    import ctypes
    p, hy, x_ = (_lib.as_f64(a) for a in (g["sep_pars"], g["sep_hyper"], xs))
    rc = ctx.lib.nmgp_predsample_sep(ctx.h, _lib.ptr(p), 1, _lib.ptr(hy), _lib.ptr(x_), len(x_), 1, _lib.ptr(np.zeros_like(star)),
                                     _lib.ptr(star), _lib.ptr(np.empty_like(mean)), _lib.ptr(np.empty_like(var)), None,
                                     ctypes.POINTER(ctypes.c_int)())
    assert rc == -3


@pytest.mark.parametrize("name,xkey,pre", [("pred_N64_M3", "xs", ""), ("pred_N512_M3_grid201", "grids", "sta_")])
def test_one_stationary_draw_is_the_deterministic_predictor(ctx, name, xkey, pre):
    g = golden(name)
    xs = g[xkey]
    ctx.set_data(g[pre + "x"], g[pre + "Y"])
    m0, v0 = ctx.predict_sta(g["sta_pars"], xs)
    mean, var, status = ctx.predsample_sta(g["sta_pars"], xs)
    assert status.tolist() == [0]
    record_parity(name + "_predsample_vs_predict_sta", mean=(maxrel(mean[0], m0, 1e-2), 1e-9), var=(maxrel(var[0], v0, 0.0), 1e-9))
    np.testing.assert_allclose(mean[0], m0, **SAME)
    np.testing.assert_allclose(var[0], v0, **SAME)


# ---- 3. batch == single, on both sides of the factorisation's schedule line --------------------------------------------------
def test_a_batch_of_draws_gives_the_bits_of_single_draw_calls(ctx, monkeypatch):
    """N = 512, D = 5: 8 draws are 40 matrices (batch n = 20,480 <= 73,728: the latency schedule of the blocked Cholesky), 40 draws
    are 200 matrices (102,400: the throughput schedule), with 21 cross-covariance rows riding below every block."""
    monkeypatch.delenv("NMGP_PREDSAMPLE_CHUNK", raising=False)
    g = golden("predsample_sep_N512_M5")
    N, M = g["Y"].shape
    T = M * (M + 1) // 2
    H = 40
    draws = np.concatenate([sep_draws(g["draws"][0], g["x"], N, T, 20, 0.01), sep_draws(g["draws"][5], g["x"], N, T, 20, 0.02)])
    xs = np.linspace(0.0, 1.0, 201)[::10]
    z = np.random.default_rng(31).standard_normal((H, len(xs), 2))
    ctx.set_data(g["x"], g["Y"])
    big = ctx.predsample_sep(draws, g["hyper"], xs, z=z)
    assert np.all(big[3] == 0)
    small = ctx.predsample_sep(draws[:8], g["hyper"], xs, z=z[:8])
    assert same_bits([a[:8] for a in big], small)
    for k in (0, 7, 8, 23, 39):
        one = ctx.predsample_sep(draws[k:k + 1], g["hyper"], xs, z=z[k:k + 1])
        assert same_bits([a[k:k + 1] for a in big], one), k
    monkeypatch.setenv("NMGP_PREDSAMPLE_CHUNK", "8")
    chunked = ctx.predsample_sep(draws, g["hyper"], xs, z=z)
    monkeypatch.delenv("NMGP_PREDSAMPLE_CHUNK")
    assert same_bits(big, chunked)
    pick = [3, 21, 39]
    mean, var, star = restate_sep(g["x"], g["Y"], draws[pick], g["hyper"], xs, hm(z[pick]), True)
    np.testing.assert_allclose(big[2][pick], hm(star), **STAR_TOL)
    np.testing.assert_allclose(big[0][pick], hm(mean), **MEAN_TOL)
    np.testing.assert_allclose(big[1][pick], hm(var), **VAR_TOL)
    # the stationary entry: 40 draws against 8 and single ones
    sd = sta_draws(np.concatenate([[-1.0, 0.5], g["draws"][0][2 * N:]]), T, H)
    sbig = ctx.predsample_sta(sd, xs)
    assert np.all(sbig[2] == 0)
    assert same_bits([a[:8] for a in sbig], ctx.predsample_sta(sd[:8], xs))
    for k in (0, 13, 39):
        assert same_bits([a[k:k + 1] for a in sbig], ctx.predsample_sta(sd[k:k + 1], xs)), k
    mo, vo = restate_sta(g["x"], g["Y"], sd[[2, 38]], xs)
    np.testing.assert_allclose(sbig[0][[2, 38]], mo, **MEAN_TOL)
    np.testing.assert_allclose(sbig[1][[2, 38]], vo, **VAR_TOL)


# ---- 4. config 5's shape --------------------------------------------------------------------------------------------------
def test_config5_shape_against_the_restatement(ctx):
    """N = 4096, D = 5, the 201-point grid: 8 draws around sep_sim_N4096_M5's parameters, repeated twice (80 matrices of order
    4096 with 202 riding rows each); two draws x four grid points against the restatement."""
    g = golden("sep_sim_N4096_M5")
    N, M = g["Y"].shape
    T = M * (M + 1) // 2
    draws = np.concatenate([sep_draws(g["pars"], g["x"], N, T, 8, 0.02)] * 2)
    xs = np.linspace(0.0, 1.0, 201)
    z = np.random.default_rng(77).standard_normal((16, 201, 2))
    z[8:] = z[:8]
    ctx.set_data(g["x"], g["Y"])
    mean, var, star, status = ctx.predsample_sep(draws, g["hyper"], xs, z=z)
    assert np.all(status == 0) and np.all(var > 0)
    assert same_bits([mean[:8], var[:8], star[:8]], [mean[8:], var[8:], star[8:]])
    dr, pick = [1, 14], np.array([5, 77, 100, 196])
    mo, vo, so = restate_sep(g["x"], g["Y"], draws[dr], g["hyper"], xs[pick], hm(z[dr][:, pick]), True)
    gm, gv, gs = mean[dr][:, pick], var[dr][:, pick], star[dr][:, pick]
    em, ev, es = maxrel(gm, hm(mo), 1e-2), maxrel(gv, hm(vo), 0.0), float(np.max(np.abs(gs - hm(so))))
    print("config 5: mean", em, "var", ev, "star abs", es)
    record_parity("predsample_sep_N4096_M5_grid201_restatement", mean=(em, 1e-5), var=(ev, 1e-5), star_abs=es)
    np.testing.assert_allclose(gm, hm(mo), **MEAN_TOL)
    np.testing.assert_allclose(gv, hm(vo), **VAR_TOL)


# ---- 5. more grid points than riding rows ----------------------------------------------------------------------------------
def test_grid_slices_against_the_restatement(ctx):
    g = golden("sep_rngfree_N8_M3")                        # N - 2 = 6 riding rows at most: S = 20 goes through in four slices
    N, M = g["Y"].shape
    T = M * (M + 1) // 2
    draws = sep_draws(g["pars"], g["x"], N, T, 3)
    xs = np.linspace(0.03, 0.97, 20)
    z = np.random.default_rng(9).standard_normal((3, 20, 2))
    ctx.set_data(g["x"], g["Y"])
    for kss_jitter in (True, False):
        mean, var, star, status = ctx.predsample_sep(draws, g["hyper"], xs, z=z, kss_jitter=kss_jitter)
        mo, vo, so = restate_sep(g["x"], g["Y"], draws, g["hyper"], xs, hm(z), kss_jitter)
        assert np.all(status == 0)
        np.testing.assert_allclose(star, hm(so), **STAR_TOL)
        np.testing.assert_allclose(mean, hm(mo), **MEAN_TOL)
        np.testing.assert_allclose(var, hm(vo), **VAR_TOL)
        # slices do not change a grid point's bits
        head = ctx.predsample_sep(draws, g["hyper"], xs[:5], z=z[:, :5], kss_jitter=kss_jitter)
        assert same_bits([mean[:, :5], var[:, :5], star[:, :5]], head[:3])
    sd = sta_draws(np.concatenate([[-1.5, 0.2], g["pars"][2 * N:]]), T, 3)
    mean, var, status = ctx.predsample_sta(sd, xs)
    mo, vo = restate_sta(g["x"], g["Y"], sd, xs)
    assert np.all(status == 0)
    np.testing.assert_allclose(mean, mo, **MEAN_TOL)
    np.testing.assert_allclose(var, vo, **VAR_TOL)
    assert same_bits([mean[:, :5], var[:, :5]], ctx.predsample_sta(sd, xs[:5])[:2])


def test_prediction_at_the_training_inputs(ctx):
    """test_predsample(..., x_test = x): S = N = 64 against N - 2 riding rows, two slices."""
    g = golden("predsample_sep_N64_M3")
    N = g["Y"].shape[0]
    draws = g["draws"][:3]
    z = np.random.default_rng(13).standard_normal((3, N, 2))
    ctx.set_data(g["x"], g["Y"])
    mean, var, star, status = ctx.predsample_sep(draws, g["hyper"], g["x"], z=z)
    mo, vo, so = restate_sep(g["x"], g["Y"], draws, g["hyper"], g["x"], hm(z), True)
    assert np.all(status == 0)
    np.testing.assert_allclose(star, hm(so), **STAR_TOL)
    np.testing.assert_allclose(mean, hm(mo), **MEAN_TOL)
    np.testing.assert_allclose(var, hm(vo), **VAR_TOL)
    head = ctx.predsample_sep(draws, g["hyper"], g["x"][:9], z=z[:, :9])
    assert same_bits([mean[:, :9], var[:, :9], star[:, :9]], head[:3])
    ms, vs, st = ctx.predsample_sta(g["sta_draws"], g["x"])
    mo, vo = restate_sta(g["x"], g["Y"], g["sta_draws"], g["x"])
    assert np.all(st == 0)
    np.testing.assert_allclose(ms, mo, **MEAN_TOL)
    np.testing.assert_allclose(vs, vo, **VAR_TOL)


# ---- 6. a draw that fails numerically ------------------------------------------------------------------------------------
def test_a_failing_draw_is_reported_and_leaves_the_others_alone(ctx):
    g = golden("predsample_sep_N64_M3")
    N = g["Y"].shape[0]
    z = hm(g["ps_z"][:, :, :2])
    ctx.set_data(g["x"], g["Y"])
    good = ctx.predsample_sep(g["draws"], g["hyper"], g["xs"], z=z)
    keep = [0, 1, 3, 4, 5]
    for slot in (N + 5, 2 * N + 1):                             # a NaN in tilde_sigma, a NaN in uL_vec
        bad = g["draws"].copy()
        bad[2, slot] = np.nan
        mean, var, star, status = ctx.predsample_sep(bad, g["hyper"], g["xs"], z=z)       # returns: no exception
        assert status[2] != 0 and np.all(np.isnan(mean[2])) and np.all(np.isnan(var[2]))
        assert np.all(status[keep] == 0)
        assert same_bits([mean[keep], var[keep], star[keep]], [a[keep] for a in good[:3]])
    sgood = ctx.predsample_sta(g["sta_draws"], g["xs"])
    bad = g["sta_draws"].copy()
    bad[1, 0] = np.nan
    mean, var, status = ctx.predsample_sta(bad, g["xs"])
    assert status[1] != 0 and np.all(np.isnan(mean[1])) and np.all(np.isnan(var[1]))
    assert np.all(status[[0, 2, 3, 4]] == 0)
    assert same_bits([mean[[0, 2, 3, 4]], var[[0, 2, 3, 4]]], [a[[0, 2, 3, 4]] for a in sgood[:2]])


# ---- 7. the workspace is the entry's own -------------------------------------------------------------------------------------
def test_the_call_leaves_batched_evaluations_and_a_begun_trajectory_alone():
    """A separable batched evaluation after the call repeats the one before it bit for bit, and a nonseparable trajectory begun
    before it continues as if the call had not happened (the two fixtures share x and Y)."""
    from nonstationary_multivariate_gaussian_process_amd import _lib
    g = golden("predsample_sep_N64_M3")
    gs = golden("predsample_N64_M3")
    assert np.array_equal(g["x"], gs["x"]) and np.array_equal(g["Y"], gs["Y"])
    B = 4
    pars = gs["draws"][:B]
    p0 = np.random.default_rng(3).standard_normal(pars.shape)

    def run(with_prediction):
        c = _lib.Context(0)
        try:
            c.set_data(g["x"], g["Y"])
            e0 = c.sep_batch_eval(g["draws"], g["hyper"], True, True)
            c.svc_batch_alloc(B)
            c.svc_batch_set_pars(pars)
            c.svc_batch_eval(gs["hyper"], True, True)
            v1, g1 = c.svc_batch_fetch(), c.svc_batch_fetch_grad()
            c.svc_batch_traj_begin()
            pred = None
            if with_prediction:
                pred = (c.predsample_sep(g["draws"], g["hyper"], g["xs"], z=hm(g["ps_z"][:, :, :2])),
                        c.predsample_sta(g["sta_draws"], g["xs"]))
            gafter = c.svc_batch_fetch_grad()                       # the pending evaluation is still the batch's last one
            traj = c.svc_batch_traj(gs["hyper"], True, 1e-4, 3, p0)
            e1 = c.sep_batch_eval(g["draws"], g["hyper"], True, True)
        finally:
            c.close()
        assert same_bits(e0, e1) and np.array_equal(g1, gafter)
        return traj, e1, pred

    t_plain, e_plain, _ = run(False)
    t_pred, e_pred, pred = run(True)
    assert np.all(pred[0][3] == 0) and np.all(pred[1][2] == 0)
    assert same_bits(t_plain, t_pred) and same_bits(e_plain, e_pred)


# ---- 8. the driver -----------------------------------------------------------------------------------------------------
def test_posterior_predict_separable_on_the_fixture_draws(ctx):
    from nonstationary_multivariate_gaussian_process_amd import drivers
    g = golden("predsample_sep_N64_M3")
    M = g["Y"].shape[1]
    h = dict(zip(SEP_KEYS, g["hyper"]))
    S = len(g["xs"])
    samples = g["draws"].reshape(3, 2, -1)                     # [iters, chains, P]
    a = drivers.posterior_predict_separable(g["x"], g["Y"], h, samples, g["xs"], seed=4, ctx=ctx)
    assert a["mean"].shape == (S, M) and a["var"].shape == (S, M) and a["quantiles"].shape == (3, S, M)
    assert a["tilde_l_star"].shape == (6, S) and a["tilde_sigma_star"].shape == (6, S)
    assert a["status"].tolist() == [0] * 6 and a["n_used"] == 6 and a["n_failed"] == 0
    assert np.all(a["quantiles"][0] <= a["quantiles"][1]) and np.all(a["quantiles"][1] <= a["quantiles"][2])
    # total variance = mean of the per-draw variances + variance of the per-draw means, from the entry's own moments
    z = np.random.default_rng(4).standard_normal((6, S, 2))
    mean, var, star, _ = ctx.predsample_sep(g["draws"], g["hyper"], g["xs"], z=z)
    np.testing.assert_allclose(a["mean"], mean.mean(axis=0), rtol=1e-13)
    np.testing.assert_allclose(a["var"], var.mean(axis=0) + mean.var(axis=0), rtol=1e-13)
    assert np.all(a["var"] >= var.mean(axis=0))
    assert np.array_equal(a["tilde_l_star"], star[:, :, 0]) and np.array_equal(a["tilde_sigma_star"], star[:, :, 1])
    b = drivers.posterior_predict_separable(g["x"], g["Y"], h, samples, g["xs"], seed=4, ctx=ctx)
    assert all(np.array_equal(a[k], b[k]) for k in ("mean", "var", "quantiles", "tilde_l_star", "tilde_sigma_star"))
    c = drivers.posterior_predict_separable(g["x"], g["Y"], h, samples, g["xs"], seed=5, ctx=ctx)
    assert not np.array_equal(a["quantiles"], c["quantiles"])
    thin = drivers.posterior_predict_separable(g["x"], g["Y"], h, g["draws"], g["xs"], draws=3, seed=4, ctx=ctx)
    assert thin["n_used"] == 3 and thin["tilde_l_star"].shape == (3, S)
