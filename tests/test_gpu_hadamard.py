"""The Hadamard nonseparable model on the GPU (nmgp_had_*, hadamard.py, drivers.HadamardMAP / BatchedHMCHadamard) against the
reference's recorded runs (tests/golden/had_*.npz), the NumPy restatement of test_hadamard_cpu.py, and itself across batch sizes.
Bars: the project's standing ones (log posterior 1e-6 relative, likelihood 1e-9, gradient ||dg|| / ||g|| 1e-5, prediction 1e-5)."""
import numpy as np
import pytest
import torch

from conftest import SVC_KEYS, golden, hyper_dict, prior_component_err_on_the_logdet_scale, record_parity, relerr, vec_relerr
from test_hadamard_cpu import CASES, _points, had_logpos, had_prior_terms

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
        p[N:N + N * T] += (amp * np.sin(3.0 * x[:, None] + 0.4 + k + np.arange(T)[None, :])).reshape(-1)
        p[-1] += 0.01 * k
        out.append(p)
    return np.stack(out)


# ---- 1. the reference's recorded runs ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_batch_entry_and_objective_reproduce_the_reference(ctx, name):
    from nonstationary_multivariate_gaussian_process_amd import hadamard
    g = golden(name)
    N = g["x"].shape[0]
    resident(ctx, g)
    for k, (pars, prior, ref_out, ref_grad) in enumerate(_points(g)):
        out, grad, status = ctx.had_batch_eval(pars, g["hyper"], prior=bool(prior), want_grad=True)
        assert status.tolist() == [0]
        p = torch.from_numpy(pars.copy()).requires_grad_(True)
        res = hadamard.nlogpos_obj_hadamard_SVC(p, torch.from_numpy(g["x"]), torch.from_numpy(g["indx"]), torch.from_numpy(g["y"]),
                                                **hyper_dict(g["hyper"], SVC_KEYS), verbose=True, Prior=bool(prior))
        res[0].backward()
        via = np.array([float(v.detach()) for v in res])
        assert np.array_equal(via, out[0]) and np.array_equal(p.grad.numpy(), grad[0])       # one entry behind both
        errs = dict(logpos=(relerr(out[0, 0], ref_out[0]), VAL_TOL), loglik=(relerr(out[0, 1], ref_out[1]), LIK_TOL),
                    grad=(vec_relerr(grad[0], ref_grad), GRAD_TOL),
                    prior_component_err_on_the_logdet_scale=(prior_component_err_on_the_logdet_scale(out[0, 2:4], ref_out[2:4], N), VAL_TOL),
                    lp_sigma2=(relerr(out[0, 4], ref_out[4]), 1e-12))
        print(name, k, {n: v[0] for n, v in errs.items()})
        record_parity("%s/point%d" % (name, k), **errs)
        for n, (e, tol) in errs.items():
            assert e < tol, (name, k, n, e)


@pytest.mark.parametrize("name", ["had_N77_M3", "had_N200_M4"])
def test_covariance_and_prediction_reproduce_the_reference(ctx, name):
    from nonstationary_multivariate_gaussian_process_amd import hadamard
    g = golden(name)
    N, M = g["x"].shape[0], int(g["M"])
    T = M * (M + 1) // 2
    resident(ctx, g)
    S = ctx.had_covariance(g["pars"])
    assert np.array_equal(S, S.T)
    np.testing.assert_allclose(S, g["Sigma"], rtol=1e-13, atol=1e-15)
    mean, var, star = ctx.predict_had(g["pars"], g["hyper"], g["grids"])
    ref_mean = g["pred"][:, 1]
    ref_var = ((g["pred"][:, 2] - g["pred"][:, 0]) / (2 * 1.96)) ** 2
    e_m, e_v = relerr(mean, ref_mean), relerr(var, ref_var)
    print(name, "prediction mean", e_m, "var", e_v)
    record_parity(name + "/predict", pred_mean=(e_m, PRED_TOL), pred_var=(e_v, PRED_TOL))
    assert e_m < PRED_TOL and e_v < PRED_TOL
    assert star.shape == (9, 1 + T) and np.all(np.isfinite(star))
    # the reference's names: all grid points from one call, and one point
    t = torch.from_numpy
    h = [float(v) for v in g["hyper"][:6]]
    p = g["pars"]
    pct = hadamard.pointwise_predmap_SVC_hadamard(t(p[:N]), t(p[N:N + N * T]), t(p[-1:])[0], t(g["x"]), t(g["indx"]), t(g["y"]),
                                                  t(g["grids"]), *h)
    assert tuple(pct.shape) == (9, 3, M) and relerr(pct.numpy(), g["pred"]) < PRED_TOL
    one = hadamard.point_predmap_SVC_hadamard(t(p[:N]), t(p[N:N + N * T]), t(p[-1:])[0], t(g["x"]), t(g["indx"]), t(g["y"]),
                                              t(g["grids"][4:5])[0], *h)
    assert tuple(one.shape) == (3, M) and torch.equal(one, pct[4])


# ---- 2. gradient scatter ----------------------------------------------------------------------------------------------------
def test_gradient_scatter_and_prior_gradient(ctx):
    g = golden("had_N77_M3")
    N, M = 77, 3
    T = M * (M + 1) // 2
    resident(ctx, g)
    pars = g["pars2"]
    _, g1, _ = ctx.had_batch_eval(pars, g["hyper"], prior=True, want_grad=True)
    _, g0, _ = ctx.had_batch_eval(pars, g["hyper"], prior=False, want_grad=True)
    _, _, dprior = had_prior_terms(pars, g["x"], M, g["hyper"])            # d (lp_l + lp_L) / d [tilde_l | L_vecs]
    a, b, s2 = float(g["hyper"][6]), float(g["hyper"][7]), float(np.exp(pars[-1]))
    want = -np.concatenate([dprior, [(-a - 1.0) + b / s2 + 1.0]])
    e = vec_relerr(g1[0] - g0[0], want)
    print("prior gradient", e)
    record_parity("had_N77_M3/prior_gradient", grad=(e, GRAD_TOL))
    assert e < GRAD_TOL
    # prior = 0: exactly the T - c_i - 1 slots outside row c_i of every observation are exactly 0.0, and no other
    L0 = g0[0][N:N + N * T].reshape(N, T)
    used = np.zeros((N, T), dtype=bool)
    for i, c in enumerate(g["indx"]):
        used[i, c * (c + 1) // 2: c * (c + 1) // 2 + c + 1] = True
    assert np.all(L0[~used] == 0.0) and np.all(L0[used] != 0.0)
    assert (~used).sum(1).tolist() == (T - g["indx"] - 1).tolist()
    assert vec_relerr(g0[0], g["grad2"]) < GRAD_TOL


# ---- 3. batch == single ------------------------------------------------------------------------------------------------------
def test_a_batch_gives_the_bits_of_single_chain_calls(ctx):
    g = golden("had_N200_M4")
    N, M = 200, 4
    resident(ctx, g)
    P = smooth_chains(g["pars"], g["x"], N, M * (M + 1) // 2, 4)
    out, grad, status = ctx.had_batch_eval(P, g["hyper"], want_grad=True)
    vout, _, _ = ctx.had_batch_eval(P, g["hyper"], want_grad=False)
    assert np.all(status == 0) and np.array_equal(out, vout)
    for k in range(4):
        o1, g1, s1 = ctx.had_batch_eval(P[k], g["hyper"], want_grad=True)
        assert np.array_equal(o1[0], out[k]) and np.array_equal(g1[0], grad[k]) and s1[0] == 0, k
    ref = had_logpos(P[3], g["x"], g["indx"], g["y"], g["hyper"], grad=True)
    assert relerr(out[3, 0], ref[0][0]) < VAL_TOL and vec_relerr(grad[3], ref[1]) < GRAD_TOL


def test_batch_bits_on_both_sides_of_the_factorisations_schedule_line(ctx):
    """N = 1536: 4 chains factor in the latency schedule of the blocked Cholesky (batch n <= 73,728), 52 chains in the throughput
    schedule.  Values AND gradients of the first 4 chains carry the same bits either way (the first run showed it: every
    kernel of the factorisation, of the inverse SYRK and of the adjoint sums in an order that does not depend on the batch)."""
    N, M = 1536, 3
    T = M * (M + 1) // 2
    rng = np.random.default_rng(1536)
    x = np.sort(np.concatenate([np.linspace(0.05, 0.95, N - 300), rng.choice(np.linspace(0.05, 0.95, N - 300), 300, replace=False)]))
    indx = rng.integers(0, M, N).astype(np.int32)
    y = np.sin(2.0 * np.pi * x * (indx + 1)) + 0.1 * indx
    p0 = np.concatenate([-2.5 + 0.5 * np.sin(3.0 * x), (0.6 + 0.2 * np.cos(2.0 * x[:, None] + np.arange(T)[None, :])).reshape(-1),
                         [np.log(1e-2)]])
    hyper = golden("had_N77_M3")["hyper"]
    P = smooth_chains(p0, x, N, T, 52, 0.02)
    ctx.had_set_data(x, indx, y)
    big_v, _, st = ctx.had_batch_eval(P, hyper, want_grad=False)
    assert np.all(st == 0)
    small_v, _, _ = ctx.had_batch_eval(P[:4], hyper, want_grad=False)
    assert np.array_equal(big_v[:4], small_v)
    big, gbig, _ = ctx.had_batch_eval(P, hyper, want_grad=True)
    small, gsmall, _ = ctx.had_batch_eval(P[:4], hyper, want_grad=True)
    e = max(vec_relerr(gbig[k], gsmall[k]) for k in range(4))
    print("gradient across the schedule line: bit-identical", np.array_equal(gbig[:4], gsmall), "measure", e)
    record_parity("had_N1536_M3/schedule_line", grad=(e, GRAD_TOL))
    assert np.array_equal(big[:4], small) and np.array_equal(big, big_v)
    assert np.array_equal(gbig[:4], gsmall)
    ref = had_logpos(P[51], x, indx, y, hyper, grad=True)
    assert relerr(big[51, 0], ref[0][0]) < VAL_TOL and relerr(big[51, 1], ref[0][1]) < LIK_TOL
    assert vec_relerr(gbig[51], ref[1]) < GRAD_TOL


# ---- 4. failure stays local, state ---------------------------------------------------------------------------------------------
def test_a_failing_chain_does_not_touch_its_neighbours(ctx):
    from nonstationary_multivariate_gaussian_process_amd import _lib
    g = golden("had_N77_M3")
    resident(ctx, g)
    P = smooth_chains(g["pars"], g["x"], 77, 6, 3)
    clean, gclean, _ = ctx.had_batch_eval(P, g["hyper"], want_grad=True)
    bad = P.copy()
    bad[1, 40] = np.nan
    out, grad, status = ctx.had_batch_eval(bad, g["hyper"], want_grad=True)
    assert status.tolist() == [0, _lib.NUM_NAN, 0]
    assert np.all(np.isnan(out[1])) and np.all(grad[1] == 0.0)
    for k in (0, 2):
        assert np.array_equal(out[k], clean[k]) and np.array_equal(grad[k], gclean[k])


def test_set_data_rejects_bad_labels(ctx):
    from nonstationary_multivariate_gaussian_process_amd import _lib
    x, y = np.linspace(0, 1, 6), np.zeros(6)
    for indx, M in (([0, 1, 3, 1, 0, 3], 3), ([0, 1, 1, 0, 1, 0], 3), ([0, -1, 1, 0, 1, 0], 2)):
        with pytest.raises(_lib.NmgpError, match="error -2"):           # NMGP_E_SHAPE
            ctx.had_set_data(x, np.array(indx), y, M=M)


def test_the_two_kinds_of_subject_exclude_each_other(ctx):
    from nonstationary_multivariate_gaussian_process_amd import _lib
    s = golden("svc_rngfree_N64_M3")
    g = golden("had_N77_M3")
    ctx.set_data(s["x"], s["Y"])
    out0, grad0 = ctx.logpos_svc(s["pars"], s["hyper"], want_grad=True)
    with pytest.raises(_lib.NmgpError, match="error -3"):               # NMGP_E_STATE
        ctx.had_batch_eval(np.zeros((1, 64 * 7 + 1)), g["hyper"])
    resident(ctx, g)
    had = ctx.had_batch_eval(g["pars"], g["hyper"], want_grad=True)
    ctx.predict_had(g["pars"], g["hyper"], g["grids"])
    with pytest.raises(_lib.NmgpError, match="error -3"):
        ctx.logpos_svc(np.zeros(77 * 7 + 1), s["hyper"])
    with pytest.raises(_lib.NmgpError, match="error -3"):
        ctx.predict_svc(np.zeros(77 * 7 + 1), s["hyper"], np.array([0.5]))
    ctx.set_data(s["x"], s["Y"])
    out1, grad1 = ctx.logpos_svc(s["pars"], s["hyper"], want_grad=True)
    assert np.array_equal(out0, out1) and np.array_equal(grad0, grad1)
    resident(ctx, g)
    again = ctx.had_batch_eval(g["pars"], g["hyper"], want_grad=True)
    assert all(np.array_equal(a, b) for a, b in zip(had, again))


# ---- 5. drivers --------------------------------------------------------------------------------------------------------------
def test_lockstep_map_follows_the_references_adam_trajectory(ctx):
    from nonstationary_multivariate_gaussian_process_amd.drivers import HadamardMAP
    g = golden("had_map_N77_M3")
    h = hyper_dict(g["hyper"], SVC_KEYS)
    init = np.stack([g["pars0"], g["pars0"] + 0.01])
    m = HadamardMAP(g["x"], g["indx"], g["y"], h, init, lr=float(g["lr"]), ctx=ctx)
    pars, hist, alive = m.run(int(g["steps"]))
    ref = g["target_value_hist"]
    rel = np.abs(hist[:, 0] - ref) / np.abs(ref)
    print("MAP trajectory, first 20 steps", rel[:20].max(), "all", rel.max())
    record_parity("had_map_N77_M3", map_first20=(rel[:20].max(), 1e-6))
    assert alive.all()
    assert rel[:20].max() < 1e-6, rel[:20]


def test_batched_hmc_chain_reproduces_a_one_chain_run(ctx):
    from nonstationary_multivariate_gaussian_process_amd.drivers import BatchedHMCHadamard
    g = golden("had_N77_M3")
    h = hyper_dict(g["hyper"], SVC_KEYS)
    init = smooth_chains(g["pars"], g["x"], 77, 6, 3, 0.01)
    kw = dict(step_size=2e-4, num_steps_in_leap=5, ctx=ctx)
    samples, info = BatchedHMCHadamard(g["x"], g["indx"], g["y"], h, init, seed=5, **kw).run(3)
    assert samples.shape == (3, 3, init.shape[1]) and np.all(np.isfinite(info["energy_error"]))
    assert not np.array_equal(samples[-1], init)
    for b in range(3):
        one, _ = BatchedHMCHadamard(g["x"], g["indx"], g["y"], h, init[b:b + 1], seed=5 + b, **kw).run(3)
        assert np.array_equal(one[:, 0], samples[:, b]), b
