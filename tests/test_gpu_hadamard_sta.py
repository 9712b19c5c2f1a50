"""The Hadamard stationary model on the GPU (nmgp_hadst_*, nmgp_predict_hadst, hadamard_sta.py, drivers.HadamardStaMAP /
BatchedHMCHadamardSta / posterior_predict_hadamard_sta) against the reference's recorded runs (tests/golden/hsta_*.npz), the
separable Hadamard entry with constant curves, and itself across batch sizes.  Bars: the project's standing ones (log posterior
1e-6 relative, likelihood 1e-9, gradient ||dg|| / ||g|| 1e-5, predictive mean and variance 1e-5 element by element, MAP
trajectory 1e-6).  The closed-form prior entries: 1e-12, except lp_tilde_l, which carries a float32 logarithm (1e-6, see
test_hadamard_sta_cpu.py)."""
import numpy as np
import pytest
import torch

from conftest import STA_KEYS, golden, hyper_dict, record_parity, relerr, vec_relerr
from test_hadamard_sta_cpu import CASES, _points, hsta_logpos

pytestmark = pytest.mark.gpu

VAL_TOL, LIK_TOL, GRAD_TOL, PRED_TOL = 1e-6, 1e-9, 1e-5, 1e-5


@pytest.fixture(scope="module")
def ctx():
    from nonstationary_multivariate_gaussian_process_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def resident(ctx, g):
    ctx.had_set_data(g["x"], g["indx"], g["y"])


def chains(p0, B, amp=0.05):
    """B parameter vectors around p0, all different."""
    k = np.arange(B)[:, None]
    P = p0[None] + amp * np.sin(0.7 + k + np.arange(p0.shape[0])[None])
    P[:, -1] = p0[-1] + 0.01 * k[:, 0]
    return np.ascontiguousarray(P)


def elem_relerr(a, b):
    """max |a - b| / |b|, element by element."""
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.abs(b)))


def same_bits(a, b):
    return all(np.array_equal(u, v) for u, v in zip(a, b))


def moments_of(pct):
    return pct[:, 1], ((pct[:, 2] - pct[:, 0]) / (2 * 1.96)) ** 2


# ---- 1. the reference's recorded runs ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_batch_entry_and_objective_reproduce_the_reference(ctx, name):
    from nonstationary_multivariate_gaussian_process_amd import hadamard_sta
    g = golden(name)
    resident(ctx, g)
    t = torch.from_numpy
    points = _points(g)
    # prior on AND off at every recorded point: the verbose tuple's prior entries are reported either way, so the other setting's
    # NegLog follows from the recorded one
    for k, (pars, prior, ref_out, ref_grad) in enumerate(points):
        out, grad, status = ctx.hadst_batch_eval(pars, g["hyper"], prior=bool(prior), want_grad=True)
        assert status.tolist() == [0] and out.shape == (1, 5) and grad.shape == (1, pars.shape[0])
        p = t(pars.copy()).requires_grad_(True)
        res = hadamard_sta.nlogpos_obj_hadamard_S(p, t(g["x"]), t(g["indx"]), t(g["y"]), **hyper_dict(g["hyper"], STA_KEYS),
                                                  verbose=True, Prior=bool(prior))
        assert len(res) == 5
        res[0].backward()
        via = np.array([float(v.detach()) for v in res])
        assert np.array_equal(via, out[0]) and np.array_equal(p.grad.numpy(), grad[0])       # one entry behind both
        errs = dict(logpos=(relerr(out[0, 0], ref_out[0]), VAL_TOL), loglik=(relerr(out[0, 1], ref_out[1]), LIK_TOL),
                    grad=(vec_relerr(grad[0], ref_grad), GRAD_TOL), lp_tilde_l=(relerr(out[0, 2], ref_out[2]), VAL_TOL),
                    lp_L_vec=(relerr(out[0, 3], ref_out[3]), 1e-12), lp_sigma2=(relerr(out[0, 4], ref_out[4]), 1e-12))
        print(name, k, {n: v[0] for n, v in errs.items()})
        record_parity("%s/point%d" % (name, k), **errs)
        for n, (e, tol) in errs.items():
            assert e < tol, (name, k, n, e)
        # the other setting of `prior`: the same tuple but NegLog, which moves by the recorded prior entries + the Jacobian
        other, gother, st = ctx.hadst_batch_eval(pars, g["hyper"], prior=not prior, want_grad=True)
        assert st.tolist() == [0] and np.array_equal(other[0, 1:], out[0, 1:])
        shift = float(ref_out[2] + ref_out[3] + ref_out[4] + pars[-1])
        want = ref_out[0] + shift if prior else ref_out[0] - shift
        e_o = relerr(other[0, 0], want)
        ref2 = hsta_logpos(pars, g["x"], g["indx"], g["y"], g["hyper"], prior=not prior, grad=True)
        e_g = vec_relerr(gother[0], ref2[1])
        record_parity("%s/point%d/prior_flipped" % (name, k), logpos=(e_o, VAL_TOL), grad_vs_restatement=(e_g, GRAD_TOL))
        assert e_o < VAL_TOL and e_g < GRAD_TOL, (name, k, e_o, e_g)
        # the non-verbose form and logpos_hadamard_S on the pieces
        T = pars.shape[0] - 3
        v = hadamard_sta.nlogpos_obj_hadamard_S(t(pars), t(g["x"]), t(g["indx"]), t(g["y"]), *[float(h) for h in g["hyper"]],
                                                Prior=bool(prior))
        lp = hadamard_sta.logpos_hadamard_S(t(pars)[0], t(pars)[1], t(pars)[2:2 + T], t(pars)[-1], t(g["x"]), t(g["indx"]), t(g["y"]),
                                            *[float(h) for h in g["hyper"]], Prior=bool(prior))
        assert float(v) == out[0, 0] and float(lp) == -out[0, 0]


# ---- 2. covariance ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hsta_N77_M3", "hsta_N200_M4"])
def test_covariance_reproduces_the_reference(ctx, name):
    g = golden(name)
    resident(ctx, g)
    S = ctx.hadst_covariance(g["pars"])
    assert np.array_equal(S, S.T)
    np.testing.assert_allclose(S, g["Sigma"], rtol=1e-13, atol=1e-15)
    record_parity(name + "/covariance", sigma=(relerr(S, g["Sigma"]), 1e-13))


# ---- 3. bits: batch == single, value-only == value + gradient, across the factorisation's schedule line ---------------------------
@pytest.mark.parametrize("name,B", [("hsta_N200_M4", 4), ("hsta_N1100_M3", 3)])
def test_a_batch_gives_the_bits_of_single_chain_calls(ctx, name, B):
    g = golden(name)
    resident(ctx, g)
    P = chains(g["pars"], B)
    out, grad, status = ctx.hadst_batch_eval(P, g["hyper"], want_grad=True)
    vout, vgrad, _ = ctx.hadst_batch_eval(P, g["hyper"], want_grad=False)
    assert np.all(status == 0) and vgrad is None and np.array_equal(out, vout)
    assert not np.array_equal(out[0], out[1])
    for k in range(B):
        o1, g1, s1 = ctx.hadst_batch_eval(P[k], g["hyper"], want_grad=True)
        assert np.array_equal(o1[0], out[k]) and np.array_equal(g1[0], grad[k]) and s1[0] == 0, k
        v1, _, _ = ctx.hadst_batch_eval(P[k], g["hyper"], want_grad=False)
        assert np.array_equal(v1[0], out[k]), k
    ref = hsta_logpos(P[B - 1], g["x"], g["indx"], g["y"], g["hyper"], grad=True)
    assert relerr(out[B - 1, 0], ref[0][0]) < VAL_TOL and vec_relerr(grad[B - 1], ref[1]) < GRAD_TOL


def test_the_first_chains_of_a_large_batch_equal_the_small_batch(ctx):
    """72 x 1100 = 79,200 lies beyond the blocked Cholesky's schedule line of 73,728; 4 x 1100 before it."""
    g = golden("hsta_N1100_M3")
    resident(ctx, g)
    P = chains(g["pars"], 72)
    big = ctx.hadst_batch_eval(P, g["hyper"], want_grad=True)
    small = ctx.hadst_batch_eval(P[:4], g["hyper"], want_grad=True)
    assert np.all(big[2] == 0)
    assert same_bits([a[:4] for a in big], small)


# ---- 4. failure stays local ---------------------------------------------------------------------------------------------------
def test_a_failing_chain_does_not_touch_its_neighbours(ctx):
    from nonstationary_multivariate_gaussian_process_amd import _lib
    g = golden("hsta_N77_M3")
    resident(ctx, g)
    P = chains(g["pars"], 3)
    clean, gclean, _ = ctx.hadst_batch_eval(P, g["hyper"], want_grad=True)
    bad = P.copy()
    bad[1, 3] = np.nan
    out, grad, status = ctx.hadst_batch_eval(bad, g["hyper"], want_grad=True)        # returns: the call itself does not fail
    assert status.tolist() == [0, _lib.NUM_NAN, 0]
    assert np.all(np.isnan(out[1])) and np.all(grad[1] == 0.0)
    for k in (0, 2):
        assert np.array_equal(out[k], clean[k]) and np.array_equal(grad[k], gclean[k])


# ---- 5. cross-check against the separable entry with constant curves, and interleaving ---------------------------------------------
def test_separable_entry_with_constant_curves_and_interleaving(ctx):
    g = golden("hsta_N1100_M3")
    hs = golden("hsep_N1100_M3")
    hd = golden("had_N1100_M3")
    N, M = 1100, 3
    T = M * (M + 1) // 2
    resident(ctx, g)
    p = chains(g["pars"], 2)[1]
    sta0 = ctx.hadst_batch_eval(p, g["hyper"], prior=False, want_grad=True)
    psep = np.concatenate([np.full(N, p[0]), np.full(N, p[1]), p[2:2 + T], p[-1:]])
    sep = ctx.hads_batch_eval(psep, hs["hyper"], prior=False, want_grad=True)
    assert sta0[2].tolist() == [0] and sep[2].tolist() == [0]
    e_lik = relerr(sta0[0][0, 1], sep[0][0, 1])
    gs = sep[1][0]
    folded = np.concatenate([[gs[:N].sum(), gs[N:2 * N].sum()], gs[2 * N:2 * N + T], gs[-1:]])
    e_g = vec_relerr(sta0[1][0], folded)
    e_slots = relerr(sta0[1][0], folded)
    print("against nmgp_hads_batch_eval with constant curves: loglik", e_lik, "gradient", e_g, "slot by slot", e_slots)
    record_parity("hsta_N1100_M3/constant_curves_vs_hads", loglik=(e_lik, LIK_TOL), grad=(e_g, GRAD_TOL), grad_slots=(e_slots, GRAD_TOL))
    assert e_lik < LIK_TOL and e_g < GRAD_TOL and e_slots < GRAD_TOL
    assert sta0[0][0, 0] == -sta0[0][0, 1]                  # prior = 0: NegLog is the negated likelihood
    # afterwards each entry reproduces its own earlier bits on the one resident subject
    had0 = ctx.had_batch_eval(hd["pars"], hd["hyper"], want_grad=True)
    sep0 = ctx.hads_batch_eval(hs["pars"], hs["hyper"], want_grad=True)
    sta1 = ctx.hadst_batch_eval(p, g["hyper"], prior=False, want_grad=True)
    pred0 = ctx.predict_hadst(p, np.array([0.2, 0.7]))
    had1 = ctx.had_batch_eval(hd["pars"], hd["hyper"], want_grad=True)
    sta2 = ctx.hadst_batch_eval(p, g["hyper"], prior=False, want_grad=True)
    sep1 = ctx.hads_batch_eval(hs["pars"], hs["hyper"], want_grad=True)
    pred1 = ctx.predict_hadst(p, np.array([0.2, 0.7]))
    assert same_bits(sta0, sta1) and same_bits(sta0, sta2) and same_bits(had0, had1) and same_bits(sep0, sep1)
    assert same_bits(pred0, pred1)


# ---- 6. prediction, full form ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hsta_N77_M3", "hsta_N200_M4"])
def test_prediction_reproduces_the_reference(ctx, name):
    from nonstationary_multivariate_gaussian_process_amd import hadamard_sta
    g = golden(name)
    M = int(g["M"])
    T = M * (M + 1) // 2
    resident(ctx, g)
    mean, var, status = ctx.predict_hadst(g["pars"], g["grids"])
    assert status.tolist() == [0] and mean.shape == var.shape == (1, 9, M)
    ref_mean, ref_var = moments_of(g["pred"])
    e_m, e_v = elem_relerr(mean[0], ref_mean), elem_relerr(var[0], ref_var)
    print(name, "prediction mean", e_m, "var", e_v)
    record_parity(name + "/predict", pred_mean=(e_m, PRED_TOL), pred_var=(e_v, PRED_TOL))
    assert e_m < PRED_TOL and e_v < PRED_TOL
    t = torch.from_numpy
    p = g["pars"]
    pieces = (t(p)[0], t(p)[1], t(p[2:2 + T]), t(p)[-1], t(g["x"]), t(g["indx"]), t(g["y"]))
    pct = hadamard_sta.pointwise_predmap_S_hadamard(*pieces, t(g["grids"]))
    e_p = elem_relerr(pct.numpy(), g["pred"])
    record_parity(name + "/pointwise_predmap_S_hadamard", percentiles=(e_p, PRED_TOL))
    assert tuple(pct.shape) == (9, 3, M) and e_p < PRED_TOL
    one = hadamard_sta.point_predmap_S_hadamard(*pieces, t(g["grids"][4:5])[0])
    assert tuple(one.shape) == (3, M) and torch.equal(one, pct[4])


def test_four_draws_give_the_bits_of_four_calls(ctx, monkeypatch):
    monkeypatch.delenv("NMGP_PREDSAMPLE_CHUNK", raising=False)
    g = golden("hsta_N200_M4")
    resident(ctx, g)
    draws = chains(g["pars"], 4)
    lab = np.arange(9) % 4
    for ix in (None, lab):
        big = ctx.predict_hadst(draws, g["grids"], indx_star=ix)
        assert big[2].tolist() == [0] * 4 and not np.array_equal(big[0][0], big[0][1])
        for k in range(4):
            assert same_bits([a[k:k + 1] for a in big], ctx.predict_hadst(draws[k], g["grids"], indx_star=ix)), k


def test_draws_give_the_same_bits_across_chunk_sizes_and_the_schedule_line(ctx, monkeypatch):
    """N = 1100: chunks of 8 draws are batch n = 8,800 <= 73,728, one chunk of 72 draws 79,200, the other side of the blocked
    Cholesky's schedule line."""
    g = golden("hsta_N1100_M3")
    resident(ctx, g)
    draws = chains(g["pars"], 72)
    xs = np.array([0.11, float(g["x"][1100 // 3]), 0.97])
    out = {}
    for chunk in ("8", "72"):
        monkeypatch.setenv("NMGP_PREDSAMPLE_CHUNK", chunk)
        out[chunk] = ctx.predict_hadst(draws, xs)
        monkeypatch.delenv("NMGP_PREDSAMPLE_CHUNK")
    assert out["8"][2].tolist() == [0] * 72 and same_bits(out["8"], out["72"])
    for k in (0, 71):
        assert same_bits([a[k:k + 1] for a in out["8"]], ctx.predict_hadst(draws[k], xs)), k
    m1, v1 = hsta_moments_at(g, draws[71], xs)
    assert elem_relerr(out["8"][0][71], m1) < PRED_TOL and elem_relerr(out["8"][1][71], v1) < PRED_TOL


def hsta_moments_at(g, pars, xs, lab=None):
    from test_hadamard_sta_cpu import hsta_moments
    return hsta_moments(pars, g["x"], g["indx"], g["y"], xs, lab)


def test_sixty_grid_points_in_three_slices_give_the_bits_of_one_point_calls(ctx):
    g = golden("hsta_N77_M3")                     # slices of 77 // 3 = 25 grid points: 25 + 25 + 10
    resident(ctx, g)
    xs = np.linspace(-0.02, 1.03, 60)
    mean, var, status = ctx.predict_hadst(g["pars"], xs)
    assert status.tolist() == [0] and mean.shape == (1, 60, 3)
    for s in range(60):
        m1, v1, _ = ctx.predict_hadst(g["pars"], xs[s:s + 1])
        assert np.array_equal(m1[0, 0], mean[0, s]) and np.array_equal(v1[0, 0], var[0, s]), s
    m_ref, v_ref = hsta_moments_at(g, g["pars"], xs)
    assert elem_relerr(mean[0], m_ref) < PRED_TOL and elem_relerr(var[0], v_ref) < PRED_TOL


# ---- 7. prediction, indexed form -----------------------------------------------------------------------------------------------------
def test_indexed_form(ctx):
    from nonstationary_multivariate_gaussian_process_amd import _lib, hadamard_sta
    g = golden("hsta_N77_M3")
    resident(ctx, g)
    lab = g["indx_star"]
    draws = np.concatenate([g["pars"][None], chains(g["pars"], 2)])
    mean, var, status = ctx.predict_hadst(draws, g["grids"], indx_star=lab)
    full_mean, full_var, _ = ctx.predict_hadst(draws, g["grids"])
    assert status.tolist() == [0] * 3 and mean.shape == var.shape == (3, 9)
    # [h, s] is bit for bit [h, s, indx_star[s]] of the full form
    assert np.array_equal(mean, full_mean[:, np.arange(9), lab]) and np.array_equal(var, full_var[:, np.arange(9), lab])
    # the reference's test_predmap_S_hadamard: its mean for all labels; its std is right at the label-0 points only
    e_m = elem_relerr(mean[0], g["test_mean"])
    zero = lab == 0
    e_s = elem_relerr(np.sqrt(var[0][zero]), g["test_std"][zero])
    print("indexed mean", e_m, "std at label 0", e_s)
    record_parity("hsta_N77_M3/indexed", pred_mean=(e_m, PRED_TOL), pred_std_label0=(e_s, PRED_TOL))
    assert e_m < PRED_TOL and e_s < PRED_TOL and zero.sum() == 3
    m_ref, v_ref = hsta_moments_at(g, g["pars"], g["grids"], lab)
    assert elem_relerr(var[0], v_ref) < PRED_TOL                        # B_f[c*, c*] at the other labels
    t = torch.from_numpy
    p = g["pars"]
    m_t, s_t = hadamard_sta.indexed_predict(t(p)[0], t(p)[1], t(p[2:8]), t(p)[-1], t(g["x"]), t(g["indx"]), t(g["y"]), t(g["grids"]),
                                            t(lab))
    assert np.array_equal(m_t.numpy(), mean[0]) and np.array_equal(s_t.numpy(), np.sqrt(var[0]))
    bad = lab.copy()
    bad[4] = 3                                                          # a label M
    with pytest.raises(_lib.NmgpError, match="error -2"):               # NMGP_E_SHAPE
        ctx.predict_hadst(g["pars"], g["grids"], indx_star=bad)


# ---- 8. state ------------------------------------------------------------------------------------------------------------------------
def test_a_complete_data_subject_is_refused(ctx):
    from nonstationary_multivariate_gaussian_process_amd import _lib
    s = golden("svc_rngfree_N64_M3")
    g = golden("hsta_N77_M3")
    ctx.set_data(s["x"], s["Y"])
    for call in (lambda: ctx.hadst_batch_eval(np.zeros((1, 9)), g["hyper"]),
                 lambda: ctx.hadst_covariance(np.zeros(9)),
                 lambda: ctx.predict_hadst(np.zeros(9), np.array([0.5]))):
        with pytest.raises(_lib.NmgpError, match="error -3"):               # NMGP_E_STATE
            call()
    resident(ctx, g)
    assert ctx.hadst_batch_eval(g["pars"], g["hyper"])[2].tolist() == [0]


# ---- 9. drivers ------------------------------------------------------------------------------------------------------------------------
def test_lockstep_map_follows_the_references_adam_trajectory(ctx):
    from nonstationary_multivariate_gaussian_process_amd.drivers import HadamardStaMAP
    g = golden("hsta_map_N77_M3")
    h = hyper_dict(g["hyper"], STA_KEYS)
    init = np.stack([g["pars0"], g["pars0"] + 0.01])
    m = HadamardStaMAP(g["x"], g["indx"], g["y"], h, init, lr=float(g["lr"]), ctx=ctx)
    pars, hist, alive = m.run(20)
    ref = g["target_value_hist"][:20]
    rel = np.abs(hist[:, 0] - ref) / np.abs(ref)
    print("MAP trajectory, first 20 steps", rel.max())
    record_parity("hsta_map_N77_M3", map_first20=(rel.max(), 1e-6))
    assert alive.all()
    assert rel.max() < 1e-6, rel


def test_batched_hmc_chain_reproduces_a_one_chain_run_under_a_dense_mass(ctx):
    from nonstationary_multivariate_gaussian_process_amd.drivers import BatchedHMCHadamardSta
    g = golden("hsta_N77_M3")
    h = hyper_dict(g["hyper"], STA_KEYS)
    P = g["pars"].shape[0]
    init = chains(g["pars"], 3, 0.01)
    A = np.random.default_rng(3).standard_normal((P, P))
    mass = 50.0 * (np.eye(P) + 0.05 * (A @ A.T))                       # dense, SPD
    kw = dict(step_size=5e-3, num_steps_in_leap=5, ctx=ctx, M=mass)
    s3 = BatchedHMCHadamardSta(g["x"], g["indx"], g["y"], h, init, seed=5, **kw)
    assert s3.mass_kind == 2
    samples, info = s3.run(5)
    assert samples.shape == (5, 3, P) and np.all(np.isfinite(info["energy_error"]))
    assert not np.array_equal(samples[-1], init)
    for b in range(3):
        one, _ = BatchedHMCHadamardSta(g["x"], g["indx"], g["y"], h, init[b:b + 1], seed=5 + b, **kw).run(5)
        assert np.array_equal(one[:, 0], samples[:, b]), b


def test_posterior_predict_returns_finite_bands_in_both_forms(ctx):
    from nonstationary_multivariate_gaussian_process_amd.drivers import posterior_predict_hadamard_sta
    g = golden("hsta_N77_M3")
    h = hyper_dict(g["hyper"], STA_KEYS)
    samples = chains(g["pars"], 12, 0.02).reshape(4, 3, -1)                    # [iters, chains, P]
    full = posterior_predict_hadamard_sta(g["x"], g["indx"], g["y"], h, samples, g["grids"], draws=6, seed=1, ctx=ctx)
    assert full["mean"].shape == full["var"].shape == (9, 3) and full["quantiles"].shape == (3, 9, 3)
    assert full["n_used"] == 6 and full["n_failed"] == 0 and full["tilde_l_star"].shape == (6, 9)
    ix = posterior_predict_hadamard_sta(g["x"], g["indx"], g["y"], h, samples, g["grids"], indx_star=g["indx_star"], seed=1, ctx=ctx)
    assert ix["mean"].shape == ix["var"].shape == (9,) and ix["quantiles"].shape == (3, 9) and ix["n_used"] == 12
    for out in (full, ix):
        assert all(np.all(np.isfinite(out[k])) for k in ("mean", "var", "quantiles")) and np.all(out["var"] > 0)
        assert np.all(out["quantiles"][0] <= out["quantiles"][1]) and np.all(out["quantiles"][1] <= out["quantiles"][2])
