"""GPU half of the Hadamard sweep: the three Hadamard models' objective, gradient and covariance entries (nmgp_had_*, nmgp_hads_*,
nmgp_hadst_*) and the four predictors (nmgp_predict_had, nmgp_predict_hads, nmgp_predict_hadst, nmgp_predsample_hads) against the NumPy
restatements, at the subjects of tests/hadamard_cases.py: every template instantiation M = 1..8 (3 and 4 through the fixtures' tests and
the wide case), N = M, the edges of the 64 x 64 tiles, contiguous / rare-first / rare-last / unsorted label layouts, more than 256
riding rows in one slice, and the leading-minor status.  tests/test_hadamard_sweep_cpu.py holds the restatements to central
differences at these very subjects and asserts cond(S) < 1e4 and that no predictive variance meets the clip.

Bars.  Covariance: rtol 1e-13, atol 1e-15, exactly symmetric (the bar of the fixtures' covariance tests).  Without the priors, and for
the stationary model (which has no GP prior) with them too: likelihood 1e-10 relative and gradient 1e-8 in ||dg|| / ||g||, the bars at
which test_numpy_restatement_meets_the_reference holds the restatements to the reference itself (cond(S) N eps ~ 1e-11 here).  With the
GP priors (factors of condition number up to 1e11): the project's standing bars -- log posterior 1e-6, likelihood 1e-9, gradient 1e-5,
the prior components 1e-6 on prior_component_err_on_the_logdet_scale, the inverse-gamma entry 1e-12.  The gradients also block by
block (tests/hadamard_cases.py, block_bar): every block at min(1e-8, max(100 d_cpu, N cond(S) eps)) where the whole vector is held to
1e-8, every block of the prior part g(prior) - g(no prior) at 1e-5 where it is held to 1e-5.  nmgp_predict_hadst (no prior
regression): mean and variance 1e-9 relative; the other predictors the standing 1e-5.  Value-only against value + gradient, a chain
alone against its row of the batch, H draws against H calls, and a batch split into chunks by NMGP_HAD_BATCH_SLAB_GB against the same
batch in one chunk: bit for bit."""
import functools

import numpy as np
import pytest

import hadamard_cases as hc
from conftest import prior_component_err_on_the_logdet_scale, record_parity, relerr, vec_relerr

pytestmark = pytest.mark.gpu

VAL_TOL, LIK_TOL, GRAD_TOL, PRED_TOL = 1e-6, 1e-9, 1e-5, 1e-5
LIK_TIGHT, GRAD_TIGHT, STA_PRED_TOL = 1e-10, 1e-8, 1e-9

EVAL = {"sta": "hadst_batch_eval", "sep": "hads_batch_eval", "had": "had_batch_eval"}
COV = {"sta": "hadst_covariance", "sep": "hads_covariance", "had": "had_covariance"}
WIDTH = {"sta": 5, "sep": 6, "had": 5}


@pytest.fixture(scope="module")
def ctx():
    from nonstationary_multivariate_gaussian_process_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def resident(ctx, c):
    ctx.had_set_data(c["x"], c["indx"], c["y"])
    assert (ctx.N, ctx.M) == (c["N"], c["M"])


def same_bits(a, b):
    return all(np.array_equal(u, v, equal_nan=True) for u, v in zip(a, b))


def name(model, case, quantity):
    return "hsweep/%s/%s/%s" % (model, hc.case_id(case), quantity)


def check(case_name, **errs):
    """print, record, then assert every (achieved, bar)"""
    print(case_name, {k: v[0] for k, v in errs.items()})
    record_parity(case_name, **errs)
    for k, (e, tol) in errs.items():
        assert e < tol, (case_name, k, e, tol)


def allclose_err(a, b, rtol, atol):
    """The measure numpy's allclose bounds by rtol: max |a - b| / (atol / rtol + |b|)."""
    return float(np.max(np.abs(a - b) / (atol / rtol + np.abs(b))))


def dm(a):
    """[S, H, ...] (the restatement's point-major order) <-> [H, S, ...] (the entries' draw-major order)"""
    return np.ascontiguousarray(np.swapaxes(a, 0, 1))


# ---- a. objective, gradient, covariance --------------------------------------------------------------------------------------------
def eval_errors(model, out, grad, ref_out, ref_grad, prior, N, M, block_bar=GRAD_TIGHT, without=None):
    """{quantity: (achieved, bar)} of one chain's verbose tuple and gradient against the restatement's.  Next to the whole-vector
    gradient error, block by block (tests/hadamard_cases.py): without the priors, and for the stationary model with them, every block
    "grad[block]" at `block_bar` = hc.block_bar(model, case, Nmax); with the GP priors every block "prior_grad[block]" of
    g(prior) - g(no prior) at GRAD_TOL, `without` = (the entry's gradient, the restatement's) of the same chain without the priors."""
    tight = model == "sta" or not prior
    if tight:
        blocks = hc.block_entries("grad", grad, ref_grad, model, N, M, min(block_bar, GRAD_TIGHT), hc.BLOCK_BARS)
    else:
        blocks = hc.block_entries("prior_grad", grad - without[0], ref_grad - without[1], model, N, M, GRAD_TOL)
    errs = eval_errors_whole(model, out, grad, ref_out, ref_grad, prior, N)
    errs.update(blocks)
    return errs


def eval_errors_whole(model, out, grad, ref_out, ref_grad, prior, N):
    tight = model == "sta" or not prior
    errs = dict(logpos=(relerr(out[0], ref_out[0]), LIK_TIGHT if not prior else VAL_TOL),
                loglik=(relerr(out[1], ref_out[1]), LIK_TIGHT if tight else LIK_TOL),
                grad=(vec_relerr(grad, ref_grad), GRAD_TIGHT if tight else GRAD_TOL))
    if model == "sta":            # closed forms; lp_tilde_l carries a float32 logarithm (test_hadamard_sta_cpu.py)
        errs.update(lp_tilde_l=(relerr(out[2], ref_out[2]), VAL_TOL), lp_L_vec=(relerr(out[3], ref_out[3]), 1e-12))
    else:
        k = WIDTH[model] - 1
        errs["prior_component_err_on_the_logdet_scale"] = (prior_component_err_on_the_logdet_scale(out[2:k], ref_out[2:k], N), VAL_TOL)
    errs["lp_sigma2"] = (relerr(out[-1], ref_out[-1]), 1e-12)
    return errs


@pytest.mark.parametrize("model", hc.MODELS)
@pytest.mark.parametrize("case", hc.CASES, ids=hc.case_id)
def test_objective_gradient_and_covariance_meet_the_restatement(ctx, case, model):
    c = hc.build(case)
    N, P = c["N"], c["pars"][model]
    resident(ctx, c)
    for k in (0, 1):
        S = getattr(ctx, COV[model])(P[k])
        ref = hc.ref_covariance(model, P[k], c)
        assert S.shape == (N, N) and np.array_equal(S, S.T)
        # (an entry is K_x[i, j] <r_i, r_j>: where the rows' products cancel, the absolute term is what holds)
        check(name(model, case, "covariance/chain%d" % k), sigma_rtol_1e13_atol_1e15=(allclose_err(S, ref, 1e-13, 1e-15), 1e-13))
        np.testing.assert_allclose(S, ref, rtol=1e-13, atol=1e-15)
    ev = getattr(ctx, EVAL[model])
    hyper = c["hyper"][model]
    plain = ev(P, hyper, prior=False, want_grad=True)[1]                 # (the prior part of a gradient is taken against it)
    for prior in (True, False):
        out, grad, status = ev(P, hyper, prior=prior, want_grad=True)
        assert status.tolist() == [0, 0] and out.shape == (2, WIDTH[model]) and grad.shape == P.shape
        assert not np.array_equal(out[0], out[1])
        if not prior:
            assert np.array_equal(out[:, 0], -out[:, 1])                 # NegLog is the negated likelihood
        for k in (0, 1):
            ref_out, ref_grad = hc.reference(model, case, k, prior)
            check(name(model, case, "eval_prior%d/chain%d" % (prior, k)),
                  **eval_errors(model, out[k], grad[k], ref_out, ref_grad, prior, N, c["M"], hc.block_bar(model, case),
                                without=(plain[k], hc.reference(model, case, k, False)[1])))
        # exactness: the value-only call, and each chain alone, return the bits of the batch
        vout, vgrad, vst = ev(P, hyper, prior=prior, want_grad=False)
        assert vgrad is None and vst.tolist() == [0, 0] and np.array_equal(vout, out)
        for k in (0, 1):
            o1, g1, s1 = ev(P[k], hyper, prior=prior, want_grad=True)
            assert s1.tolist() == [0] and np.array_equal(o1[0], out[k]) and np.array_equal(g1[0], grad[k]), k
            v1, _, _ = ev(P[k], hyper, prior=prior, want_grad=False)
            assert np.array_equal(v1[0], out[k]), k


# ---- b, c. the four predictors ---------------------------------------------------------------------------------------------------------
def run_predictors(ctx, case, full=None, indexed=None, tag=""):
    """All four predictors on the resident subject of `case` against the restatements' moments: `full` = hc.predictions(...) with the
    full-form references (None: skip the full forms), `indexed` likewise for the indexed forms (they may sit at other inputs)."""
    c = hc.build(case)
    M, T, P, hy = c["M"], c["T"], c["pars"], c["hyper"]
    if full is not None:
        xs, z = full["xs"], full["z"]
        S = xs.shape[0]
        # stationary: both chains as two draws of one call
        mean, var, status = ctx.predict_hadst(P["sta"], xs)
        assert status.tolist() == [0, 0] and mean.shape == var.shape == (2, S, M)
        for k in (0, 1):
            m_ref, v_ref = full["sta_full"][k]
            check(name("sta", case, tag + "predict_full/draw%d" % k), pred_mean=(relerr(mean[k], m_ref), STA_PRED_TOL),
                  pred_var=(relerr(var[k], v_ref), STA_PRED_TOL))
            assert same_bits([a[k:k + 1] for a in (mean, var, status)], ctx.predict_hadst(P["sta"][k], xs)), k
        # separable and nonseparable MAP predictors
        mean, var, star = ctx.predict_hads(P["sep"][0], hy["sep"], xs)
        assert mean.shape == var.shape == (S, M) and star.shape == (S, 2) and np.all(np.isfinite(star))
        check(name("sep", case, tag + "predict"), pred_mean=(relerr(mean, full["sep"][0]), PRED_TOL), pred_var=(relerr(var, full["sep"][1]), PRED_TOL))
        one = ctx.predsample_hads(P["sep"][0], hy["sep"], xs)                 # one draw, no noise, no labels: the bits of predict_hads
        assert one[3].tolist() == [0] and np.array_equal(one[0][0], mean) and np.array_equal(one[1][0], var) and np.array_equal(one[2][0], star)
        mean, var, star = ctx.predict_had(P["had"][0], hy["had"], xs)
        assert mean.shape == var.shape == (S, M) and star.shape == (S, 1 + T) and np.all(np.isfinite(star))
        check(name("had", case, tag + "predict"), pred_mean=(relerr(mean, full["had"][0]), PRED_TOL), pred_var=(relerr(var, full["had"][1]), PRED_TOL))
        # posterior draws of the separable model
        loc, scale = full["hps_full"]
        mean, var, star, status = ctx.predsample_hads(P["sep"], hy["sep"], xs, z=z)
        assert status.tolist() == [0, 0] and mean.shape == var.shape == (2, S, M) and star.shape == (2, S, 2)
        check(name("sep", case, tag + "predsample_full"), star=(relerr(dm(star), loc[:, :, :2] + scale[:, :, :2] * dm(z)), PRED_TOL),
              pred_mean=(relerr(dm(mean), loc[:, :, 2:]), PRED_TOL), pred_var=(relerr(dm(var), scale[:, :, 2:] ** 2), PRED_TOL))
    if indexed is not None:
        xs, lab, z = indexed["xs"], indexed["lab"], indexed["z"]
        S = xs.shape[0]
        mean, var, status = ctx.predict_hadst(P["sta"], xs, indx_star=lab)
        assert status.tolist() == [0, 0] and mean.shape == var.shape == (2, S)
        for k in (0, 1):
            m_ref, v_ref = indexed["sta_ix"][k]
            check(name("sta", case, tag + "predict_indexed/draw%d" % k), pred_mean=(relerr(mean[k], m_ref), STA_PRED_TOL),
                  pred_var=(relerr(var[k], v_ref), STA_PRED_TOL))
            assert same_bits([a[k:k + 1] for a in (mean, var, status)], ctx.predict_hadst(P["sta"][k], xs, indx_star=lab)), k
        loc, scale = indexed["hps_ix"]
        mean, var, star, status = ctx.predsample_hads(P["sep"], hy["sep"], xs, indx_star=lab, z=z)
        assert status.tolist() == [0, 0] and mean.shape == var.shape == (2, S) and star.shape == (2, S, 2)
        check(name("sep", case, tag + "predsample_indexed"), star=(relerr(dm(star), loc[:, :, :2] + scale[:, :, :2] * dm(z)), PRED_TOL),
              pred_mean=(relerr(dm(mean), loc[:, :, 2]), PRED_TOL), pred_var=(relerr(dm(var), scale[:, :, 2] ** 2), PRED_TOL))


@pytest.mark.parametrize("case", hc.CASES, ids=hc.case_id)
def test_the_four_predictors_meet_the_restatement(ctx, case, monkeypatch):
    monkeypatch.delenv("NMGP_PREDSAMPLE_CHUNK", raising=False)
    c = hc.build(case)
    resident(ctx, c)
    pred = hc.predictions(case)
    assert hc.raw_variance_floor(pred, c) > 1.0                   # (asserted per case in the CPU half: no variance meets the clip)
    run_predictors(ctx, case, full=pred, indexed=pred)


def test_slices_of_more_than_256_riding_rows(ctx, monkeypatch):
    """N = 321, M = 3.  Full form, 110 inputs: one slice of 107 inputs = 321 riding rows (cross-row blocks of 256 + 65), then a slice of
    3 inputs.  Indexed form, 330 inputs: a slice of 321 rows, then 9."""
    monkeypatch.delenv("NMGP_PREDSAMPLE_CHUNK", raising=False)
    case = hc.WIDE
    c = hc.build(case)
    resident(ctx, c)
    full, ix = hc.predictions(case, **hc.WIDE_FULL), hc.predictions(case, **hc.WIDE_INDEXED)
    run_predictors(ctx, case, full=full, indexed=ix, tag="wide_")
    # rows beyond index 256 of the first slice on their own: outputs k = s M + m >= 256 (full), inputs s >= 256 (indexed)
    mean, var, _ = ctx.predict_hadst(c["pars"]["sta"][0], full["xs"])
    m_ref, v_ref = full["sta_full"][0]
    far = slice(256, 321)
    check(name("sta", case, "wide_predict_full/rows_256_320"), pred_mean=(relerr(mean[0].reshape(-1)[far], m_ref.reshape(-1)[far]), STA_PRED_TOL),
          pred_var=(relerr(var[0].reshape(-1)[far], v_ref.reshape(-1)[far]), STA_PRED_TOL))
    mean, var, _ = ctx.predict_hadst(c["pars"]["sta"][0], ix["xs"], indx_star=ix["lab"])
    m_ref, v_ref = ix["sta_ix"][0]
    check(name("sta", case, "wide_predict_indexed/rows_256_320"), pred_mean=(relerr(mean[0][far], m_ref[far]), STA_PRED_TOL),
          pred_var=(relerr(var[0][far], v_ref[far]), STA_PRED_TOL))
    # three draws in chunks of two: the ragged chunk gives the bits of single-draw calls
    P = c["pars"]["sta"]
    draws = np.stack([P[0], P[1], 2.0 * P[1] - P[0]])
    for xs, lab in ((full["xs"], None), (ix["xs"], ix["lab"])):
        monkeypatch.setenv("NMGP_PREDSAMPLE_CHUNK", "2")
        big = ctx.predict_hadst(draws, xs, indx_star=lab)
        monkeypatch.delenv("NMGP_PREDSAMPLE_CHUNK")
        assert big[2].tolist() == [0, 0, 0] and not np.array_equal(big[0][1], big[0][2])
        for k in range(3):
            assert same_bits([a[k:k + 1] for a in big], ctx.predict_hadst(draws[k], xs, indx_star=lab)), k


# ---- d. the leading-minor status -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", hc.MODELS)
def test_a_zero_third_pivot_is_reported_as_leading_minor_three(ctx, model):
    """The header's `status = k > 0`: sigma2_err = exp(-800) = 0 and a zero row 2 of L make row / column 2 of S exactly 0 (finite
    inputs throughout), so the third pivot is exactly 0 and LAPACK's rule `pivot <= 0` names minor 3."""
    c = hc.build(hc.MINOR)
    resident(ctx, c)
    P = hc.minor_chains(model)
    ev = getattr(ctx, EVAL[model])
    hyper = c["hyper"][model]
    for prior in (True, False):
        clean = ev(P[[0, 2]], hyper, prior=prior, want_grad=True)
        assert clean[2].tolist() == [0, 0]
        out, grad, status = ev(P, hyper, prior=prior, want_grad=True)
        print(model, "prior", prior, "status", status.tolist())
        assert status.tolist() == [0, 3, 0]
        assert np.all(np.isnan(out[1])) and np.all(grad[1] == 0.0)
        assert np.array_equal(out[[0, 2]], clean[0]) and np.array_equal(grad[[0, 2]], clean[1])
        vout, _, vst = ev(P, hyper, prior=prior, want_grad=False)
        assert vst.tolist() == [0, 3, 0] and np.array_equal(vout, out, equal_nan=True)


def test_the_predictors_report_leading_minor_three_for_the_bad_draw_only(ctx, monkeypatch):
    monkeypatch.delenv("NMGP_PREDSAMPLE_CHUNK", raising=False)
    c = hc.build(hc.MINOR)
    resident(ctx, c)
    xs, lab = c["xs"], c["lab"]
    S, M = xs.shape[0], c["M"]
    z = np.random.default_rng(65).standard_normal((3, S, 2))
    P = hc.minor_chains("sta")
    for ix in (None, lab):
        mean, var, status = ctx.predict_hadst(P, xs, indx_star=ix)
        print("predict_hadst", "indexed" if ix is not None else "full", "status", status.tolist())
        assert status.tolist() == [0, 3, 0]
        assert np.all(np.isnan(mean[1])) and np.all(np.isnan(var[1]))
        clean = ctx.predict_hadst(P[[0, 2]], xs, indx_star=ix)
        assert clean[2].tolist() == [0, 0] and np.all(np.isfinite(clean[0])) and same_bits([a[[0, 2]] for a in (mean, var)], clean[:2])
    P = hc.minor_chains("sep")
    hyper = c["hyper"]["sep"]
    for ix in (None, lab):
        mean, var, star, status = ctx.predsample_hads(P, hyper, xs, indx_star=ix, z=z)
        print("predsample_hads", "indexed" if ix is not None else "full", "status", status.tolist())
        assert status.tolist() == [0, 3, 0]
        assert np.all(np.isnan(mean[1])) and np.all(np.isnan(var[1]))
        clean = ctx.predsample_hads(P[[0, 2]], hyper, xs, indx_star=ix, z=z[[0, 2]])
        assert clean[3].tolist() == [0, 0] and np.all(np.isfinite(clean[0]))
        assert same_bits([a[[0, 2]] for a in (mean, var, star)], clean[:3])


# ---- e. the workspace cap --------------------------------------------------------------------------------------------------------------
CAP_N, CAP_B = 3800, 3


@functools.lru_cache(maxsize=None)
def cap_subject():
    """N = 3800 evenly spaced inputs of ONE output (M = T = 1: the smallest parameter vectors) and three chains per model."""
    N = CAP_N
    x = np.linspace(0.05, 0.95, N)
    indx = np.zeros(N, dtype=np.int32)
    y = np.sin(6.0 * x) + 0.1 * np.random.default_rng(3801).standard_normal(N)
    P = hc.parameters(x, 1, np.ones(1))
    return dict(N=N, M=1, x=x, indx=indx, y=y, hyper=hc.hypers(), pars={m: np.stack([p[0], p[1], 2.0 * p[1] - p[0]]) for m, p in P.items()})


def chunks_under_cap(N, B, cap_gb):
    """Chunks of a value + gradient call of B chains as INTEGRATION.md states the workspace: (2N + 2) ld + N^2 doubles per chain, ld =
    the 2N + 2 rows rounded up to 16 and one column per observation, floor(cap / that) chains per chunk."""
    ld = (2 * N + 2 + 15) // 16 * 16
    per_chain = 8.0 * (ld * N + N * N)
    per_chunk = min(B, int(cap_gb * 1e9 // per_chain))
    assert per_chunk >= 1
    return -(-B // per_chunk)


@pytest.mark.parametrize("model", hc.MODELS)
def test_results_do_not_depend_on_the_workspace_cap(ctx, model, monkeypatch):
    """INTEGRATION.md on NMGP_HAD_BATCH_SLAB_GB: "results do not depend on it bit for bit".  Three chains with gradients at N = 3800
    need 0.35 GB each: under the smallest cap the library accepts (1 GB) they run as chunks of 2 + 1, under the default cap as one.
    N = 3800 is the smallest order (in steps of 100) at which three chains split.  For the models with GP priors prior = 0 and the
    first two columns only: above N = 3500 the prior solves go through the library's trsm, whose results are not promised to be
    independent of the batch."""
    c = cap_subject()
    assert chunks_under_cap(CAP_N, CAP_B, 1.0) == 2 and chunks_under_cap(CAP_N, CAP_B, 96.0) == 1
    assert chunks_under_cap(CAP_N, CAP_B, 1.0 / 1.05) == 2          # (the vectors and partial rows the formula leaves out: < 2 %)
    resident(ctx, c)
    ev = getattr(ctx, EVAL[model])
    P, hyper = c["pars"][model], c["hyper"][model]
    prior = model == "sta"
    monkeypatch.setenv("NMGP_HAD_BATCH_SLAB_GB", "1")
    out_c, grad_c, st_c = ev(P, hyper, prior=prior, want_grad=True)
    monkeypatch.delenv("NMGP_HAD_BATCH_SLAB_GB")
    out_1, grad_1, st_1 = ev(P, hyper, prior=prior, want_grad=True)
    vout, _, vst = ev(P, hyper, prior=prior, want_grad=False)
    print(model, "status", st_c.tolist(), st_1.tolist(), vst.tolist(), "neglog", out_1[:, 0].tolist())
    assert st_c.tolist() == st_1.tolist() == vst.tolist() == [0, 0, 0]
    assert np.all(np.isfinite(out_1[:, :2])) and np.all(np.isfinite(grad_1)) and len(set(out_1[:, 1].tolist())) == 3
    assert np.array_equal(out_c[:, :2], out_1[:, :2]) and np.array_equal(grad_c, grad_1)
    assert np.array_equal(vout[:, :2], out_1[:, :2])
