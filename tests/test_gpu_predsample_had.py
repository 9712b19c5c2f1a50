"""Posterior-draw and held-out prediction of the nonseparable Hadamard model on the GPU (nmgp_predsample_had, hadamard.py's own names,
drivers.posterior_predict_hadamard) against the NumPy restatement tests/predsample_had_cases.restate_hpn (which
tests/test_predsample_had_cpu.py holds to the reference's recorded runs), the reference's held-out MAP predictor
(tests/golden/hpn_N77_M3.npz), the deterministic predictor nmgp_predict_had, and itself across forms, batch, chunk and slice sizes.

Bars.  Against the restatement and the reference: the project's standing prediction bars, mean and variance 1e-5 relative element by
element (conftest.relerr), starred values 1e-6 (an LU against a substitution solve with the GP-prior covariance).  Against
nmgp_predict_had with one draw and no noise: starred values bit for bit (the same regression), mean and variance 1e-5 -- not bit for
bit, because that entry factors with the default panel kernels and this one with the substitution-based ones.  Indexed against full
under the same starred values: 1e-10 relative.  Batch against single calls, chunk against chunk, slice against slice, poisoned
against repeated: bit for bit.

Shapes are tests/hadamard_cases.py's, the smallest that still reach each edge; every compared raw variance of the restatement exceeds
the draw's sigma2_err on the grids as they stand (asserted below), so the clip to 1e-6 plays no part and no grid had to be made denser."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import hadamard_cases as hc
import predsample_had_cases as pc
from conftest import ROOT, SVC_KEYS, golden, hyper_dict, record_parity, relerr

pytestmark = pytest.mark.gpu

PRED_TOL, STAR_TOL, FORM_TOL = 1e-5, 1e-6, 1e-10


@pytest.fixture(scope="module")
def ctx():
    from nonstationary_multivariate_gaussian_process_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def resident(ctx, c):
    ctx.had_set_data(c["x"], c["indx"], c["y"])


def same_bits(a, b):
    return all(np.array_equal(u, v, equal_nan=True) for u, v in zip(a, b))


def more_draws(c, H):
    """H draws on the segment through the subject's two (and beyond it): smooth, distinct, all factorable."""
    d = c["draws"]
    return np.stack([d[0] + 0.5 * k * (d[1] - d[0]) for k in range(H)])


def check_against_restatement(ctx, case, tag, e):
    c = pc.subject(case)
    S, M, T = e["xs"].shape[0], c["M"], c["T"]
    floor = pc.raw_variance_floor(e, case)
    errs = {}
    for form, lab in (("full", None), ("ix", e["lab"])):
        if form not in e:
            continue
        mean, var, star, status = ctx.predsample_had(c["draws"], c["hyper"], e["xs"], indx_star=lab, z=e["z"])
        assert status.tolist() == [0, 0] and star.shape == (2, S, 1 + T)
        assert mean.shape == var.shape == ((2, S, M) if lab is None else (2, S))
        rm, rv, rs = e[form]
        errs.update({form + "_mean": relerr(mean, rm), form + "_var": relerr(var, rv), form + "_star": relerr(star, rs)})
    print(tag, "raw variance / sigma2_err >=", floor, errs)
    record_parity(tag, **{k: (v, STAR_TOL if k.endswith("star") else PRED_TOL) for k, v in errs.items()})
    assert floor > 1.0, (tag, floor)
    for k, v in errs.items():
        assert v < (STAR_TOL if k.endswith("star") else PRED_TOL), (tag, k, v)


# ---- 1. parity with the restatement: M = 1 .. 8, tile edges, label layouts, both forms -------------------------------------------------
@pytest.mark.parametrize("case", pc.PARITY, ids=pc.parity_id)
def test_two_draws_under_fixed_normals_meet_the_restatement(ctx, case):
    resident(ctx, pc.subject(case))
    check_against_restatement(ctx, case, "hpn/" + pc.parity_id(case), pc.expected(case))


# ---- 2. slices wider than one 256-lane block of riding rows ----------------------------------------------------------------------------
def test_wide_slices_meet_the_restatement(ctx):
    c = pc.subject(pc.WIDE)
    assert (c["N"], c["M"]) == (321, 3)
    resident(ctx, c)
    check_against_restatement(ctx, pc.WIDE, "hpn/wide_full_S110", pc.expected(pc.WIDE, **pc.WIDE_FULL))           # 321 rows, then 3
    check_against_restatement(ctx, pc.WIDE, "hpn/wide_indexed_S330", pc.expected(pc.WIDE, **pc.WIDE_INDEXED))     # 321 rows, then 9


# ---- 3. bits ------------------------------------------------------------------------------------------------------------------------
def test_five_draws_give_the_bits_of_five_calls_whatever_the_chunking(ctx, monkeypatch):
    monkeypatch.delenv("NMGP_PREDSAMPLE_CHUNK", raising=False)
    case = "had_N77_M3"
    c = pc.subject(case)
    resident(ctx, c)
    draws = more_draws(c, 5)
    xs, lab = pc.new_inputs(case, 30)                                     # full form: slices of 25 and 5 inputs
    z = np.random.default_rng(12).standard_normal((5, 30, 1 + c["T"]))
    for ix in (None, lab):
        big = ctx.predsample_had(draws, c["hyper"], xs, indx_star=ix, z=z)
        assert big[3].tolist() == [0] * 5 and not np.array_equal(big[0][0], big[0][1])
        for k in range(5):
            one = ctx.predsample_had(draws[k], c["hyper"], xs, indx_star=ix, z=z[k:k + 1])
            assert same_bits([a[k:k + 1] for a in big], one), k
        monkeypatch.setenv("NMGP_PREDSAMPLE_CHUNK", "2")                  # chunks of 2, 2 and 1 draws
        chunked = ctx.predsample_had(draws, c["hyper"], xs, indx_star=ix, z=z)
        monkeypatch.delenv("NMGP_PREDSAMPLE_CHUNK")
        assert same_bits(big, chunked)


def test_a_grid_point_moved_to_another_slice_keeps_its_bits(ctx):
    case = "had_N77_M3"
    c = pc.subject(case)
    resident(ctx, c)
    xs, _ = pc.new_inputs(case, 30)                                       # slices of 77 // 3 = 25 inputs: 25 + 5
    z = pc.normals(case, 30)
    a = ctx.predsample_had(c["draws"], c["hyper"], xs, z=z)
    rev = np.arange(30)[::-1]                                             # points 0 .. 4 move to the second slice, 25 .. 29 to the first
    b = ctx.predsample_had(c["draws"], c["hyper"], xs[rev].copy(), z=np.ascontiguousarray(z[:, rev]))
    assert a[3].tolist() == b[3].tolist() == [0, 0]
    assert same_bits([v[:, rev] for v in b[:3]], a[:3])
    head = ctx.predsample_had(c["draws"], c["hyper"], xs[:7].copy(), z=np.ascontiguousarray(z[:, :7]))    # one short slice
    assert same_bits(head[:3], [v[:, :7] for v in a[:3]])


POISON_SNIPPET = r'''
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np
import predsample_had_cases as pc
from nonstationary_multivariate_gaussian_process_amd import _lib
ctx = _lib.Context(0)
n = 0
for case, S in (((5, 5, "unsorted"), None), ((65, 6, "rare_first"), None), ("had_N77_M3", 30)):
    c = pc.subject(case)
    ctx.had_set_data(c["x"], c["indx"], c["y"])
    xs, lab = pc.new_inputs(case, S)
    z = pc.normals(case, xs.shape[0])
    for ix in (None, lab):
        first = ctx.predsample_had(c["draws"], c["hyper"], xs, indx_star=ix, z=z)        # a fresh (or grown) workspace: poisoned
        again = ctx.predsample_had(c["draws"], c["hyper"], xs, indx_star=ix, z=z)        # the kept workspace: poisoned again
        fed = ctx.predsample_had(c["draws"], c["hyper"], xs, indx_star=ix, star=first[2])
        assert first[3].tolist() == [0, 0] and all(np.all(np.isfinite(a)) for a in first[:3]), (case, ix)
        assert all(np.array_equal(u, v) for u, v in zip(first, again)), (case, ix)
        assert all(np.array_equal(u, v) for u, v in zip(first, fed)), (case, ix)
        n += 1
ctx.close()
print("POISON_OK", n)
'''


def test_repeated_calls_under_poison_give_the_same_bits():
    """NMGP_POISON=1 (read once per process: a child) fills fresh buffers and the kept workspace with NaNs before every call: an
    element that no kernel wrote, or one read before it is written, shows up as a NaN or as a difference between the calls."""
    env = dict(os.environ)
    env["NMGP_POISON"] = "1"
    env.pop("NMGP_PREDSAMPLE_CHUNK", None)
    out = subprocess.run([sys.executable, "-c", POISON_SNIPPET % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}],
                         capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0 and "POISON_OK 6" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


def test_a_pending_batch_result_is_unchanged_by_a_prediction_in_between(ctx):
    case = "had_N77_M3"
    c = pc.subject(case)
    resident(ctx, c)
    xs, lab = pc.new_inputs(case)
    before = ctx.had_batch_eval(c["draws"], c["hyper"], want_grad=True)
    ctx.predsample_had(c["draws"], c["hyper"], xs, z=pc.normals(case, xs.shape[0]))
    ctx.predsample_had(c["draws"], c["hyper"], xs, indx_star=lab)
    after = ctx.had_batch_eval(c["draws"], c["hyper"], want_grad=True)
    assert before[2].tolist() == [0, 0] and same_bits(before, after)


# ---- 4. against the existing deterministic predictor ------------------------------------------------------------------------------------
def test_one_draw_without_noise_against_predict_had(ctx):
    g = golden("had_N77_M3")
    resident(ctx, g)
    m0, v0, s0 = ctx.predict_had(g["pars"], g["hyper"], g["grids"])
    mean, var, star, status = ctx.predsample_had(g["pars"], g["hyper"], g["grids"])
    assert status.tolist() == [0] and mean.shape == (1,) + m0.shape and star.shape == (1,) + s0.shape
    e_m, e_v = relerr(mean[0], m0), relerr(var[0], v0)
    print("against predict_had: mean", e_m, "var", e_v, "bit-identical", np.array_equal(mean[0], m0) and np.array_equal(var[0], v0))
    record_parity("hpn/had_N77_M3/vs_predict_had", mean=(e_m, PRED_TOL), var=(e_v, PRED_TOL))
    assert np.array_equal(star[0], s0)                      # the same regression: bit for bit
    assert e_m < PRED_TOL and e_v < PRED_TOL                # another panel kernel: rounding


# ---- 5. the indexed form against the full form -------------------------------------------------------------------------------------------
def test_indexed_form_is_the_matching_column_of_the_full_form(ctx):
    """N = 77, M = 3: the full form slices at 25 grid points, so 30 points are two factorisations per draw there and one (30 <= N
    riding rows) in the indexed form."""
    from nonstationary_multivariate_gaussian_process_amd import _lib
    case = "had_N77_M3"
    c = pc.subject(case)
    resident(ctx, c)
    S = 30
    xs, lab = pc.new_inputs(case, S)
    assert sorted(set(lab.tolist())) == [0, 1, 2]
    z = pc.normals(case, S)
    mean, var, star, status = ctx.predsample_had(c["draws"], c["hyper"], xs, z=z)
    im, iv, istar, ist = ctx.predsample_had(c["draws"], c["hyper"], xs, indx_star=lab, star=star)
    assert status.tolist() == ist.tolist() == [0, 0] and np.array_equal(istar, star) and im.shape == iv.shape == (2, S)
    fm, fv = mean[:, np.arange(S), lab], var[:, np.arange(S), lab]
    e_m, e_v = relerr(im, fm), relerr(iv, fv)
    print("indexed against full: mean", e_m, "var", e_v, "bit-identical", np.array_equal(im, fm) and np.array_equal(iv, fv))
    record_parity("hpn/had_N77_M3/indexed_vs_full", mean=(e_m, FORM_TOL), var=(e_v, FORM_TOL))
    assert e_m < FORM_TOL and e_v < FORM_TOL
    # regressing again with the same z gives the same starred values, hence the same numbers
    jm, jv, jstar, _ = ctx.predsample_had(c["draws"], c["hyper"], xs, indx_star=lab, z=z)
    assert np.array_equal(jstar, star) and np.array_equal(jm, im) and np.array_equal(jv, iv)


# ---- 6. the reference's held-out MAP predictor --------------------------------------------------------------------------------------------
def test_indexed_predict_meets_the_reference_where_the_reference_is_right():
    from nonstationary_multivariate_gaussian_process_amd import hadamard
    g = golden("hpn_N77_M3")
    N, T = 77, 6
    t = torch.from_numpy
    p = g["pars"]
    mean, var = hadamard.indexed_predict(t(p[:N]), t(p[N:N + N * T]), t(p[-1:])[0], t(g["x"]), t(g["indx"]), t(g["y"]), t(g["x_test"]),
                                         t(g["indx_test"]), **hyper_dict(g["hyper"][:6], SVC_KEYS[:6]))
    assert tuple(mean.shape) == tuple(var.shape) == (12,) and mean.dtype == var.dtype == torch.float64
    zero = g["indx_test"] == 0
    assert zero.sum() >= 4 and g["var"][zero].min() > 1e-5
    e_m, e_v = relerr(mean.numpy(), g["mean"]), relerr(var.numpy()[zero], g["var"][zero])
    print("against the reference's test_predmap_SVC_hadamard: mean", e_m, "var at label 0", e_v)
    record_parity("hpn_N77_M3/reference", mean=(e_m, PRED_TOL), var_label0=(e_v, PRED_TOL))
    assert e_m < PRED_TOL and e_v < PRED_TOL
    assert np.all(var.numpy()[~zero] > float(np.exp(p[-1])))          # the labelled output's own variance, above the noise floor


# ---- 7. failure stays local -----------------------------------------------------------------------------------------------------------------
def test_status_of_a_bad_draw_and_its_neighbours(ctx, monkeypatch):
    from nonstationary_multivariate_gaussian_process_amd import _lib
    monkeypatch.delenv("NMGP_PREDSAMPLE_CHUNK", raising=False)
    c = hc.build(hc.MINOR)
    resident(ctx, c)
    xs, hyper = c["xs"], c["hyper"]["had"]
    S, T = xs.shape[0], c["T"]
    lab = hc.grid_labels(S, c["M"], 2)                                      # M = 3: every label occurs
    z = np.random.default_rng(65).standard_normal((3, S, 1 + T))
    P = hc.minor_chains("had")
    nan = P[[0, 2, 0]].copy()
    nan[1, 40] = np.nan
    for ix in (None, lab):
        for draws, want in ((P, 3), (nan, _lib.NUM_NAN)):
            mean, var, star, status = ctx.predsample_had(draws, hyper, xs, indx_star=ix, z=z)
            print("predsample_had", "indexed" if ix is not None else "full", "status", status.tolist())
            assert status.tolist() == [0, want, 0]
            assert np.all(np.isnan(mean[1])) and np.all(np.isnan(var[1]))
            clean = ctx.predsample_had(draws[[0, 2]], hyper, xs, indx_star=ix, z=z[[0, 2]])
            assert clean[3].tolist() == [0, 0] and np.all(np.isfinite(clean[0])) and np.all(np.isfinite(clean[1]))
            assert same_bits([a[[0, 2]] for a in (mean, var, star)], clean[:3])


# ---- 8. state and arguments (argument checks: nothing reaches the device) -------------------------------------------------------------------
def test_state_and_argument_checks(ctx):
    from nonstationary_multivariate_gaussian_process_amd import _lib
    s = golden("svc_rngfree_N64_M3")
    g = golden("had_N77_M3")
    P = g["pars"][None]
    ctx.set_data(s["x"], s["Y"])                                            # a complete-data subject is resident
    with pytest.raises(_lib.NmgpError, match="error -3"):                   # NMGP_E_STATE
        ctx.predsample_had(np.zeros((1, 64 * 7 + 1)), g["hyper"], np.array([0.5]))
    resident(ctx, g)
    xs = g["grids"][:3]
    for lab in ([0, 1, 3], [0, -1, 2]):
        with pytest.raises(_lib.NmgpError, match="error -2"):               # NMGP_E_SHAPE: a label outside [0, M)
            ctx.predsample_had(P, g["hyper"], xs, indx_star=lab)
    z, star = np.zeros((1, 3, 7)), np.zeros((1, 3, 7))
    with pytest.raises(_lib.NmgpError):                                     # the binding refuses z with star ...
        ctx.predsample_had(P, g["hyper"], xs, z=z, star=star)
    ptr, ip = _lib.ptr, _lib.ctypes.POINTER(_lib.ctypes.c_int)
    mean, var, hy = np.empty((1, 3, 3)), np.empty((1, 3, 3)), _lib.as_f64(g["hyper"])
    rc = ctx.lib.nmgp_predsample_had(ctx.h, ptr(P), 1, ptr(hy), ptr(xs), None, 3, ptr(z), ptr(star), ptr(mean), ptr(var), None, None)
    assert rc == -3                                                         # ... and so does the entry: NMGP_E_STATE
    with pytest.raises(_lib.NmgpError):                                     # one label per new input
        ctx.predsample_had(P, g["hyper"], xs, indx_star=[0, 1])
    with pytest.raises(_lib.NmgpError):                                     # the separable layout's length is refused
        ctx.predsample_had(np.zeros((1, 2 * 77 + 6 + 1)), g["hyper"], xs)
    with pytest.raises(_lib.NmgpError):
        ctx.predsample_had(P, g["hyper"], xs, z=np.zeros((1, 3, 2)))
    # the entry still works after the refusals
    assert ctx.predsample_had(P, g["hyper"], xs)[3].tolist() == [0]


# ---- 9. the driver -----------------------------------------------------------------------------------------------------------------------------
def test_driver_summarises_six_draws_in_both_forms(ctx):
    from nonstationary_multivariate_gaussian_process_amd import drivers
    case = "had_N77_M3"
    c = pc.subject(case)
    h = hyper_dict(c["hyper"], SVC_KEYS)
    M, T = c["M"], c["T"]
    samples = more_draws(c, 6).reshape(3, 2, -1)                            # [iters, chains, P]
    used = samples.reshape(6, -1)
    g = golden("hpn_N77_M3")
    for xs, lab in ((pc.new_inputs(case)[0], None), (g["x_test"], g["indx_test"])):
        S = len(xs)
        a = drivers.posterior_predict_hadamard(c["x"], c["indx"], c["y"], h, samples, xs, indx_star=lab, seed=4, ctx=ctx)
        shape = (S, M) if lab is None else (S,)
        assert a["n_used"] == 6 and a["n_failed"] == 0 and a["mean"].shape == a["var"].shape == shape
        assert a["quantiles"].shape == (3,) + shape and a["tilde_l_star"].shape == (6, S)
        assert a["L_star"].shape == (6, S, T) and a["corr_quantiles"].shape == (3, S, M, M)
        # total variance = mean of the per-draw variances + variance of the per-draw means, from the entry's own moments
        z = np.random.default_rng(4).standard_normal((6, S, 1 + T))
        mean, var, star, _ = ctx.predsample_had(used, c["hyper"], xs, indx_star=lab, z=z)
        np.testing.assert_allclose(a["mean"], mean.mean(axis=0), rtol=1e-13)
        np.testing.assert_allclose(a["var"], var.mean(axis=0) + mean.var(axis=0), rtol=1e-13)
        assert np.all(a["var"] >= var.mean(axis=0)) and np.array_equal(a["L_star"], star[:, :, 1:])
        np.testing.assert_allclose(np.einsum("qsmm->qsm", a["corr_quantiles"]), 1.0, rtol=0, atol=1e-14)
        assert np.all(np.abs(a["corr_quantiles"]) <= 1.0 + 1e-14)
        b = drivers.posterior_predict_hadamard(c["x"], c["indx"], c["y"], h, samples, xs, indx_star=lab, seed=4, ctx=ctx)
        assert all(np.array_equal(a[k], b[k]) for k in a if k not in ("n_used", "n_failed"))
