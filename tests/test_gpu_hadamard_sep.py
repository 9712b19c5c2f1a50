"""The Hadamard separable model on the GPU (nmgp_hads_*, hadamard_sep.py, drivers.HadamardSepMAP / BatchedHMCHadamardSep) against the
reference's recorded runs (tests/golden/hsep_*.npz), the NumPy restatement of test_hadamard_sep_cpu.py, and itself across batch
sizes.  Bars: the project's standing ones (log posterior 1e-6 relative, likelihood 1e-9, gradient ||dg|| / ||g|| 1e-5, prediction
1e-5, lp_sigma2 1e-12, the GP-prior components on prior_component_err_on_the_logdet_scale)."""
import numpy as np
import pytest
import torch

from conftest import SEP_KEYS, golden, hyper_dict, prior_component_err_on_the_logdet_scale, record_parity, relerr, vec_relerr
from test_hadamard_sep_cpu import CASES, _points, hsep_logpos, hsep_prior_terms

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


def smooth_chains(p0, x, N, T, B, amp=0.05):
    out = []
    for k in range(B):
        p = p0.copy()
        p[:N] += amp * np.sin(3.0 * x + 0.4 + k)
        p[N:2 * N] += amp * np.cos(2.0 * x + 0.3 * k)
        p[2 * N:2 * N + T] += amp * np.sin(0.7 + k + np.arange(T))
        p[-1] += 0.01 * k
        out.append(p)
    return np.stack(out)


# ---- 1. the reference's recorded runs ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_batch_entry_and_objective_reproduce_the_reference(ctx, name):
    from nonstationary_multivariate_gaussian_process_amd import hadamard_sep
    g = golden(name)
    N = g["x"].shape[0]
    resident(ctx, g)
    for k, (pars, prior, ref_out, ref_grad) in enumerate(_points(g)):
        out, grad, status = ctx.hads_batch_eval(pars, g["hyper"], prior=bool(prior), want_grad=True)
        assert status.tolist() == [0] and out.shape == (1, 6)
        p = torch.from_numpy(pars.copy()).requires_grad_(True)
        res = hadamard_sep.nlogpos_obj_hadamard(p, torch.from_numpy(g["x"]), torch.from_numpy(g["indx"]), torch.from_numpy(g["y"]),
                                                **hyper_dict(g["hyper"], SEP_KEYS), verbose=True, Prior=bool(prior))
        assert len(res) == 6
        res[0].backward()
        via = np.array([float(v.detach()) for v in res])
        assert np.array_equal(via, out[0]) and np.array_equal(p.grad.numpy(), grad[0])       # one entry behind both
        errs = dict(logpos=(relerr(out[0, 0], ref_out[0]), VAL_TOL), loglik=(relerr(out[0, 1], ref_out[1]), LIK_TOL),
                    grad=(vec_relerr(grad[0], ref_grad), GRAD_TOL),
                    prior_component_err_on_the_logdet_scale=(prior_component_err_on_the_logdet_scale(out[0, 2:5], ref_out[2:5], N), VAL_TOL),
                    lp_sigma2=(relerr(out[0, 5], ref_out[5]), 1e-12))
        print(name, k, {n: v[0] for n, v in errs.items()})
        record_parity("%s/point%d" % (name, k), **errs)
        for n, (e, tol) in errs.items():
            assert e < tol, (name, k, n, e)


# ---- 2. covariance and prediction ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hsep_N77_M3", "hsep_N200_M4"])
def test_covariance_and_prediction_reproduce_the_reference(ctx, name):
    from nonstationary_multivariate_gaussian_process_amd import hadamard_sep
    g = golden(name)
    N, M = g["x"].shape[0], int(g["M"])
    T = M * (M + 1) // 2
    resident(ctx, g)
    S = ctx.hads_covariance(g["pars"])
    assert np.array_equal(S, S.T)
    np.testing.assert_allclose(S, g["Sigma"], rtol=1e-13, atol=1e-15)
    mean, var, star = ctx.predict_hads(g["pars"], g["hyper"], g["grids"])
    ref_mean = g["pred"][:, 1]
    ref_var = ((g["pred"][:, 2] - g["pred"][:, 0]) / (2 * 1.96)) ** 2
    e_m, e_v = relerr(mean, ref_mean), relerr(var, ref_var)
    print(name, "prediction mean", e_m, "var", e_v)
    record_parity(name + "/predict", pred_mean=(e_m, PRED_TOL), pred_var=(e_v, PRED_TOL))
    assert e_m < PRED_TOL and e_v < PRED_TOL
    assert star.shape == (9, 2) and np.all(np.isfinite(star))
    # the reference's names: all grid points from one call, and one point
    t = torch.from_numpy
    h = [float(v) for v in g["hyper"][:6]]
    p = g["pars"]
    pieces = (t(p[:N]), t(p[N:2 * N]), t(p[2 * N:2 * N + T]), t(p[-1:])[0], t(g["x"]), t(g["indx"]), t(g["y"]))
    pct = hadamard_sep.pointwise_predmap_hadmard(*pieces, t(g["grids"]), *h)
    e_p = relerr(pct.numpy(), g["pred"])
    record_parity(name + "/pointwise_predmap_hadmard", percentiles=(e_p, PRED_TOL))
    assert tuple(pct.shape) == (9, 3, M) and e_p < PRED_TOL
    one = hadamard_sep.point_predmap_hadamard(*pieces, t(g["grids"][4:5])[0], *h)
    assert tuple(one.shape) == (3, M) and torch.equal(one, pct[4])


# ---- 3. gradient pieces: the prior gradient and the label-segmented reduction -------------------------------------------------
def test_prior_gradient_and_label_segmented_reduction(ctx):
    g = golden("hsep_N77_M3")
    N, M = 77, 3
    T = M * (M + 1) // 2
    assert int((g["indx"] == M - 1).sum()) == 2             # the rare label has two members
    resident(ctx, g)
    pars = g["pars2"]
    _, g1, _ = ctx.hads_batch_eval(pars, g["hyper"], prior=True, want_grad=True)
    _, g0, _ = ctx.hads_batch_eval(pars, g["hyper"], prior=False, want_grad=True)
    _, _, _, dprior = hsep_prior_terms(pars, g["x"], M, g["hyper"])       # d (lp_l + lp_sigma + lp_L) / d [tilde_l | tilde_sigma | L_vec]
    a, b, s2 = float(g["hyper"][6]), float(g["hyper"][7]), float(np.exp(pars[-1]))
    want = -np.concatenate([dprior, [(-a - 1.0) + b / s2 + 1.0]])
    e = vec_relerr(g1[0] - g0[0], want)
    # the L_vec / c^2 part alone: T numbers of size 0.1 next to prior gradients of size 1e3, so measured on its own slots
    e_L = vec_relerr((g1[0] - g0[0])[2 * N:2 * N + T], want[2 * N:2 * N + T])
    e_s2 = relerr((g1[0] - g0[0])[-1], want[-1])
    # Prior=False: the L_vec gradient is the segmented sum of the likelihood's row components and nothing else
    e_seg = vec_relerr(g0[0][2 * N:2 * N + T], g["grad2"][2 * N:2 * N + T])
    print("prior gradient", e, "L_vec part", e_L, "sigma2 part", e_s2, "segmented L_vec gradient", e_seg)
    record_parity("hsep_N77_M3/prior_gradient", grad=(e, GRAD_TOL), grad_L_vec_prior=(e_L, GRAD_TOL), grad_sigma2_prior=(e_s2, GRAD_TOL),
                  grad_L_vec_segmented=(e_seg, GRAD_TOL))
    assert e < GRAD_TOL and e_L < GRAD_TOL and e_s2 < GRAD_TOL
    assert e_seg < GRAD_TOL
    assert vec_relerr(g0[0], g["grad2"]) < GRAD_TOL


# ---- 4. batch == single, value-only == value + gradient ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,B", [("hsep_N200_M4", 4), ("hsep_N1100_M3", 3)])
def test_a_batch_gives_the_bits_of_single_chain_calls(ctx, name, B):
    g = golden(name)
    N, M = g["x"].shape[0], int(g["M"])
    resident(ctx, g)
    P = smooth_chains(g["pars"], g["x"], N, M * (M + 1) // 2, B)
    out, grad, status = ctx.hads_batch_eval(P, g["hyper"], want_grad=True)
    vout, vgrad, _ = ctx.hads_batch_eval(P, g["hyper"], want_grad=False)
    assert np.all(status == 0) and vgrad is None and np.array_equal(out, vout)
    for k in range(B):
        o1, g1, s1 = ctx.hads_batch_eval(P[k], g["hyper"], want_grad=True)
        assert np.array_equal(o1[0], out[k]) and np.array_equal(g1[0], grad[k]) and s1[0] == 0, k
        v1, _, _ = ctx.hads_batch_eval(P[k], g["hyper"], want_grad=False)
        assert np.array_equal(v1[0], out[k]), k
    ref = hsep_logpos(P[B - 1], g["x"], g["indx"], g["y"], g["hyper"], grad=True)
    assert relerr(out[B - 1, 0], ref[0][0]) < VAL_TOL and vec_relerr(grad[B - 1], ref[1]) < GRAD_TOL


# ---- 5. failure stays local -------------------------------------------------------------------------------------------------------
def test_a_failing_chain_does_not_touch_its_neighbours(ctx):
    from nonstationary_multivariate_gaussian_process_amd import _lib
    g = golden("hsep_N77_M3")
    resident(ctx, g)
    P = smooth_chains(g["pars"], g["x"], 77, 6, 3)
    clean, gclean, _ = ctx.hads_batch_eval(P, g["hyper"], want_grad=True)
    bad = P.copy()
    bad[1, 40] = np.nan
    out, grad, status = ctx.hads_batch_eval(bad, g["hyper"], want_grad=True)
    assert status.tolist() == [0, _lib.NUM_NAN, 0]
    assert np.all(np.isnan(out[1])) and np.all(grad[1] == 0.0)
    for k in (0, 2):
        assert np.array_equal(out[k], clean[k]) and np.array_equal(grad[k], gclean[k])


# ---- 6. state -----------------------------------------------------------------------------------------------------------------------
def test_state_and_interleaving_with_the_nonseparable_entry(ctx):
    from nonstationary_multivariate_gaussian_process_amd import _lib
    s = golden("svc_rngfree_N64_M3")
    g = golden("hsep_N77_M3")
    h = golden("had_N77_M3")
    assert np.array_equal(g["x"], h["x"]) and np.array_equal(g["indx"], h["indx"]) and np.array_equal(g["y"], h["y"])
    ctx.set_data(s["x"], s["Y"])
    for call in (lambda: ctx.hads_batch_eval(np.zeros((1, 2 * 64 + 6 + 1)), g["hyper"]),
                 lambda: ctx.hads_covariance(np.zeros(2 * 64 + 6 + 1)),
                 lambda: ctx.predict_hads(np.zeros(2 * 64 + 6 + 1), g["hyper"], np.array([0.5]))):
        with pytest.raises(_lib.NmgpError, match="error -3"):               # NMGP_E_STATE
            call()
    resident(ctx, g)
    with pytest.raises(_lib.NmgpError):                                     # the nonseparable layout's length is refused
        ctx.hads_batch_eval(h["pars"], g["hyper"])
    sep0 = ctx.hads_batch_eval(g["pars"], g["hyper"], want_grad=True)
    svc0 = ctx.had_batch_eval(h["pars"], h["hyper"], want_grad=True)
    sep1 = ctx.hads_batch_eval(g["pars"], g["hyper"], want_grad=True)
    ctx.predict_hads(g["pars"], g["hyper"], g["grids"])
    svc1 = ctx.had_batch_eval(h["pars"], h["hyper"], want_grad=True)
    sep2 = ctx.hads_batch_eval(g["pars"], g["hyper"], want_grad=True)
    assert all(np.array_equal(a, b) for a, b in zip(sep0, sep1)) and all(np.array_equal(a, b) for a, b in zip(sep0, sep2))
    assert all(np.array_equal(a, b) for a, b in zip(svc0, svc1))
    assert sep0[0].shape == (1, 6) and svc0[0].shape == (1, 5)


# ---- 7, 8. drivers ---------------------------------------------------------------------------------------------------------------------
def test_lockstep_map_follows_the_references_adam_trajectory(ctx):
    from nonstationary_multivariate_gaussian_process_amd.drivers import HadamardSepMAP
    g = golden("hsep_map_N77_M3")
    h = hyper_dict(g["hyper"], SEP_KEYS)
    init = np.stack([g["pars0"], g["pars0"] + 0.01])
    m = HadamardSepMAP(g["x"], g["indx"], g["y"], h, init, lr=float(g["lr"]), ctx=ctx)
    pars, hist, alive = m.run(20)
    ref = g["target_value_hist"][:20]
    rel = np.abs(hist[:, 0] - ref) / np.abs(ref)
    print("MAP trajectory, first 20 steps", rel.max())
    record_parity("hsep_map_N77_M3", map_first20=(rel.max(), 1e-6))
    assert alive.all()
    assert rel.max() < 1e-6, rel


def test_batched_hmc_chain_reproduces_a_one_chain_run(ctx):
    from nonstationary_multivariate_gaussian_process_amd.drivers import BatchedHMCHadamardSep
    g = golden("hsep_N77_M3")
    h = hyper_dict(g["hyper"], SEP_KEYS)
    init = smooth_chains(g["pars"], g["x"], 77, 6, 3, 0.01)
    kw = dict(step_size=2e-4, num_steps_in_leap=5, ctx=ctx)
    samples, info = BatchedHMCHadamardSep(g["x"], g["indx"], g["y"], h, init, seed=5, **kw).run(3)
    assert samples.shape == (3, 3, init.shape[1]) and np.all(np.isfinite(info["energy_error"]))
    assert not np.array_equal(samples[-1], init)
    for b in range(3):
        one, _ = BatchedHMCHadamardSep(g["x"], g["indx"], g["y"], h, init[b:b + 1], seed=5 + b, **kw).run(3)
        assert np.array_equal(one[:, 0], samples[:, b]), b
