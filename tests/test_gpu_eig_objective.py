"""The separable and stationary objectives in the eigen formulation (NMGP_SEP=eig) on the GPU (run with -m gpu on an MI355X), M = 1 .. 8
around every ragged edge of its kernels: rocsolver_dsyevd, k_kron_mv, k_eig_reduce, k_colscale_d, k_sep_adjoint, k_sep_grad_sum,
k_sep_coreB, the host Jacobi and the rotation of coreB, the retry loop's add_diag.  Cases, chains and references come from
tests/eig_objective_cases.py, which tests/test_eig_objective_cpu.py checks: the CPU oracle where the case has one, the dense
restatement (np.longdouble while N M <= 1000) otherwise.  Two contexts live in this process, the default one (Cholesky formulation)
and one created under NMGP_SEP=eig.

What is measured, per chain (the measures of tests/test_gpu_objective_sweep.py):
  priors off   likelihood 1e-10 relative; the gradient block by block (tilde_l, tilde_sigma, uL_vec, sigma2) at 1e-8 each,
               ||d_b|| / max(||gref_b||, 1e-3 ||gref||) -- a failure names the chain (row) and the block; NegLog == -loglik
  priors on    the standing bars: NegLog 1e-6, likelihood 1e-9 and bit-equal to the priors-off call, the components 1e-6 (the GP-prior
               ones on the log det scale), the prior part of the gradient 1e-5 in ||.||
  bits         the prior components of the two formulations; a batch row and its single-chain call; the value-only and the
               value+gradient batch; a case after a larger and after a smaller one
Every achieved error is recorded (eig_objective/<model>_<case>/<entry>/prior<0|1>)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import eig_objective_cases as E
import objective_cases as OC
from conftest import ROOT, record_parity, relerr, vec_relerr
from test_gpu_objective_sweep import GRAD_TOL, LIK_TOL, VAL_TOL, hold_to_oracle

pytestmark = pytest.mark.gpu

SWEEP = "eig_objective"
CASES = E.all_cases()


def model_case_id(case):
    return "%s_%s" % (case[0], E.case_id(case[1:]))


def make_context(algo):
    """A context of its own formulation: NMGP_SEP is read when the context is created."""
    from nonstationary_multivariate_gaussian_process_amd import _lib
    old = os.environ.get("NMGP_SEP")
    os.environ["NMGP_SEP"] = algo
    try:
        return _lib.Context(0)
    finally:
        if old is None:
            os.environ.pop("NMGP_SEP", None)
        else:
            os.environ["NMGP_SEP"] = old


@pytest.fixture(scope="module")
def ctxs():
    c = {"eig": make_context("eig"), "chol": make_context("chol")}
    yield c
    for v in c.values():
        v.close()


# ---------------------------------------------------------------------------------------------------
# the entries and the measures (also run by the NMGP_POISON child, which imports this module)
# ---------------------------------------------------------------------------------------------------
def hold_sta_to_oracle(case, entry, layout, got, refs, rows=None, tag=None, bars=None):
    """hold_to_oracle for the stationary layout: four blocks, five components (none of them a GP prior).  tag, bars: the record's
    name and the table of block bars of another sweep (tests/test_gpu_sta_objective.py)."""
    model, N, M = layout
    (out0, g0), (out1, g1) = got[False], got[True]
    rows = range(len(refs)) if rows is None else rows
    e = dict(loglik=0.0, block=0.0, neglog=0.0, loglik1=0.0, rest=0.0, prior_grad=0.0)
    worst, bad = (0.0, "-", -1), []
    for j, b in enumerate(rows):
        (r0, gr0), (r1, gr1) = refs[j][False], refs[j][True]
        el = relerr(out0[b][1], r0[1])
        e["loglik"] = max(e["loglik"], el)
        if not el < E.LIK_TIGHT:
            bad.append("row %d: likelihood %.3g >= %.0e (%r, reference %r)" % (b, el, E.LIK_TIGHT, out0[b][1], r0[1]))
        if out0[b][0] != -out0[b][1]:
            bad.append("row %d: NegLog %r != -loglik %r without the priors" % (b, out0[b][0], out0[b][1]))
        eb, name = OC.block_errors(g0[b], gr0, layout)
        if not eb <= worst[0]:
            worst = (eb, name, b)
        for name, err, bar in OC.blocks_over_bar(g0[b], gr0, layout, E.GRAD_TIGHT, E.BLOCK_BARS if bars is None else bars):
            bad.append("row %d: gradient block %s %.3g >= %.0e" % (b, name, err, bar))
        errs = dict(neglog=(relerr(out1[b][0], r1[0]), VAL_TOL), loglik1=(relerr(out1[b][1], r1[1]), LIK_TOL),
                    rest=(relerr(out1[b][2:], r1[2:]), VAL_TOL), prior_grad=(vec_relerr(g1[b] - g0[b], gr1 - gr0), GRAD_TOL))
        for k, (err, bar) in errs.items():
            e[k] = max(e[k], err)
            if not err < bar:
                bad.append("row %d, priors on: %s %.3g >= %.0e (%r, reference %r)" % (b, k, err, bar, out1[b], r1))
        if out1[b][1] != out0[b][1]:
            bad.append("row %d: the likelihood changes with the prior flag: %r, %r" % (b, out1[b][1], out0[b][1]))
    e["block"] = worst[0]
    tag = "%s/%s_%s/%s" % (SWEEP, model, case, entry) if tag is None else tag
    print("%s: loglik %.3g worst block %.3g (%s, row %d) | priors on: neglog %.3g loglik %.3g rest %.3g prior grad %.3g"
          % (tag, e["loglik"], worst[0], worst[1], worst[2], e["neglog"], e["loglik1"], e["rest"], e["prior_grad"]))
    worst_bar = (E.BLOCK_BARS if bars is None else bars).get(tuple(layout) + (worst[1],), E.GRAD_TIGHT)       # the bar that block is held to
    record_parity(tag + "/prior0", loglik=(e["loglik"], E.LIK_TIGHT), worst_block=(e["block"], worst_bar))
    record_parity(tag + "/prior1", neglog=(e["neglog"], VAL_TOL), loglik=(e["loglik1"], LIK_TOL), other_components=(e["rest"], VAL_TOL),
                  prior_grad=(e["prior_grad"], GRAD_TOL))
    assert not bad, "%s:\n  " % tag + "\n  ".join(bad)
    return e


def hold(case, entry, got, ks):
    model, N, M = case
    refs = E.refs(model, N, M, ks)
    if model == "sep":
        return hold_to_oracle(E.case_id((N, M)), entry, case, got, refs, sweep=SWEEP, bars=E.BLOCK_BARS)
    return hold_sta_to_oracle(E.case_id((N, M)), entry, case, got, refs)


def resident(ctx, case):
    x, Y = E.subject(*case)
    ctx.set_data(x, Y)


def run_single(ctx, case, ks):
    """nmgp_logpos_sep / nmgp_logpos_sta on the chains ks: {prior: (out [len(ks), 6 | 5], grad [len(ks), P])}."""
    model, N, M = case
    resident(ctx, case)
    fn = ctx.logpos_sep if model == "sep" else ctx.logpos_sta
    got = {}
    for prior in (False, True):
        rows = [fn(E.chain(model, N, M, k), E.hyper_vec(model), prior=prior, want_grad=True) for k in ks]
        got[prior] = (np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]))
        assert ctx.last_sep_attempts() == 0
    return got


def run_batch(ctx, case):
    """nmgp_sep_batch_eval / nmgp_sta_batch_eval on chains 0 .. 2, with and without the gradient: ({prior: (out, grad)}, {prior: out})."""
    model, N, M = case
    resident(ctx, case)
    fn = ctx.sep_batch_eval if model == "sep" else ctx.sta_batch_eval
    pars = E.chains(model, N, M, E.BATCH)
    got, valued = {}, {}
    for prior in (False, True):
        out, grad, st = fn(pars, E.hyper_vec(model), prior, True)
        outv, gv, stv = fn(pars, E.hyper_vec(model), prior, False)
        assert gv is None and st.tolist() == [0] * E.BATCH and stv.tolist() == [0] * E.BATCH, (st, stv)
        got[prior], valued[prior] = (out, grad), outv
    return got, valued


def all_chains(case):
    return list(range(E.n_chains(case[0])))


def check_single(ctx, case):
    got = run_single(ctx, case, all_chains(case))
    hold(case, "single", got, all_chains(case))
    return got


def check_batch(ctx, case, single=None):
    """The batch of 3 against the references, against the single-chain calls (bit for bit) and against its value-only call."""
    got, valued = run_batch(ctx, case)
    hold(case, "batch%d_grad" % E.BATCH, got, list(range(E.BATCH)))
    single = run_single(ctx, case, list(range(E.BATCH))) if single is None else single
    for prior in (False, True):
        assert np.array_equal(got[prior][0], single[prior][0][:E.BATCH]), (case, prior, got[prior][0], single[prior][0])
        assert np.array_equal(got[prior][1], single[prior][1][:E.BATCH]), (case, prior)
        assert np.array_equal(valued[prior], got[prior][0]), (case, prior, valued[prior], got[prior][0])


_SINGLE = {}


def single_results(ctxs, algo, case):
    """run_single on every chain of the case in the context of formulation `algo`; evaluated once per module run, and held to
    nothing here: the tests that compare the formulations do not fail because a bar of 1. does."""
    if (algo, case) not in _SINGLE:
        _SINGLE[(algo, case)] = run_single(ctxs[algo], case, all_chains(case))
    return _SINGLE[(algo, case)]


# ---------------------------------------------------------------------------------------------------
# 1. the single-chain entries against the references
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=model_case_id)
def test_single_chain_entry_in_the_eigen_formulation(ctxs, case):
    hold(case, "single", single_results(ctxs, "eig", case), all_chains(case))


# ---------------------------------------------------------------------------------------------------
# 2., 3. against the default formulation
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=model_case_id)
def test_prior_parts_have_the_default_formulations_bits(ctxs, case):
    """The prior components are the same code on the same inputs in both formulations (nmgp_logpos_sep: the cached factors, the two
    solves queued by the g_before_sync hook from inside kron_loglik here and from inside kron_chol_loglik there)."""
    eig, chol = single_results(ctxs, "eig", case), single_results(ctxs, "chol", case)
    for prior in (False, True):
        assert np.array_equal(eig[prior][0][:, 2:], chol[prior][0][:, 2:]), (case, prior, eig[prior][0], chol[prior][0])


@pytest.mark.parametrize("case", CASES, ids=model_case_id)
def test_distance_between_the_two_formulations_is_recorded(ctxs, case):
    """No bar of its own: both formulations are held to the reference (here and in tests/test_gpu_objective_sweep.py)."""
    model, N, M = case
    eig, chol = single_results(ctxs, "eig", case), single_results(ctxs, "chol", case)
    el = max(relerr(a[1], b[1]) for a, b in zip(eig[False][0], chol[False][0]))
    eb = max(OC.block_errors(a, b, case) for a, b in zip(eig[False][1], chol[False][1]))
    print("%s/%s eig vs default: loglik %.3g worst block %.3g (%s)" % (SWEEP, model_case_id(case), el, eb[0], eb[1]))
    record_parity("%s/%s/single_vs_default/prior0" % (SWEEP, model_case_id(case)), loglik=el, worst_block=eb[0])
    assert np.isfinite(el) and np.isfinite(eb[0])


# ---------------------------------------------------------------------------------------------------
# 4. the batch entries fall back to the single-chain entry, chain by chain
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=model_case_id)
def test_batch_entries_in_the_eigen_formulation(ctxs, case):
    check_batch(ctxs["eig"], case)


# ---------------------------------------------------------------------------------------------------
# 5. degenerate B
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["eig", "chol"])
@pytest.mark.parametrize("shape", E.DEGENERATE_SHAPES, ids=E.case_id)
@pytest.mark.parametrize("model", ["sep", "sta"])
def test_degenerate_B_in_both_formulations(ctxs, model, shape, algo):
    """B = I (every eigenvalue equal: the Jacobi stops on its first sweep) and a B whose eigenvalues span twelve orders of
    magnitude; the default formulation builds its blocks from the same host Jacobi."""
    case = (model,) + shape
    got = run_single(ctxs[algo], case, list(E.DEGENERATE_KINDS))
    hold(case, "degenerate_%s" % algo, got, list(E.DEGENERATE_KINDS))


# ---------------------------------------------------------------------------------------------------
# 6. the retry
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["sep", "sta"])
def test_singular_covariance_is_retried_in_the_eigen_formulation(ctxs, model):
    """Attempt 0 gives log 0 and 0 / 0 in k_eig_reduce; attempt 1 (1e-6 on the diagonals of B, through the host Jacobi, and of K,
    through add_diag) must be the likelihood of that covariance.  In a batch the neighbours of the retried chain keep their bits."""
    ctx = ctxs["eig"]
    x, Y, good, bad = E.singular(model)
    ctx.set_data(x, Y)
    hv = E.hyper_vec(model)
    fn, fb = (ctx.logpos_sep, ctx.sep_batch_eval) if model == "sep" else (ctx.logpos_sta, ctx.sta_batch_eval)
    out, grad = fn(bad, hv, prior=False, want_grad=True)
    assert np.all(np.isfinite(out[:2])) and out[0] == -out[1] and np.all(np.isfinite(grad)), (out, grad)
    assert ctx.last_sep_attempts() == 1
    e = relerr(out[1], E.singular_ref(model))
    print("%s/%s_singular_retry: loglik %.3g" % (SWEEP, model, e))
    record_parity("%s/%s_singular_retry/single/prior0" % (SWEEP, model), loglik=(e, E.RETRY_TOL))
    assert e < E.RETRY_TOL, (out[1], E.singular_ref(model))
    out_g, grad_g, st_g = fb(good, hv, False, True)
    pars = good.copy()
    pars[1] = bad
    out_b, grad_b, st_b = fb(pars, hv, False, True)
    assert st_g.tolist() == [0, 0, 0] and st_b.tolist() == [0, 1, 0], (st_g, st_b)
    assert np.array_equal(out_b[[0, 2]], out_g[[0, 2]]) and np.array_equal(grad_b[[0, 2]], grad_g[[0, 2]])
    # (sigma2 = 0 leaves a NaN in the inverse-gamma component, which the entries report whatever the prior flag)
    assert np.array_equal(out_b[1], out, equal_nan=True) and np.array_equal(grad_b[1], grad)
    o, _ = fn(good[0], hv, prior=True, want_grad=False)      # a well-posed call afterwards
    assert ctx.last_sep_attempts() == 0 and np.all(np.isfinite(o))


# ---------------------------------------------------------------------------------------------------
# 7. call history
# ---------------------------------------------------------------------------------------------------
def test_a_case_has_the_same_bits_after_a_larger_and_after_a_smaller_one(ctxs):
    """From the largest case to the smallest and back: on the way down the scratch slots (SL_K3, SL_U, SL_PART) and d_K / d_K2 are
    larger than the case needs and hold the previous case's data."""
    ctx = ctxs["eig"]
    order = sorted(CASES, key=lambda c: (-c[1], -c[2], c[0]))
    passes = []
    for cases in (order, order[::-1]):
        res = {}
        for case in cases:
            ks = [0, E.n_chains(case[0]) - 1]
            res[case] = run_single(ctx, case, ks)
        passes.append(res)
    for case in order:
        for prior in (False, True):
            for j in (0, 1):
                assert np.array_equal(passes[0][case][prior][j], passes[1][case][prior][j]), (case, prior, j)


# ---------------------------------------------------------------------------------------------------
# 8. once more with every fresh buffer and scratch hand-out full of NaNs
# ---------------------------------------------------------------------------------------------------
POISON_SNIPPET = r'''
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import eig_objective_cases as E
import test_gpu_eig_objective as t
E.load_refs(%(refs)r)
ctx = t.make_context("eig")
n = 0
for case in t.CASES + t.CASES[::-1]:
    t.check_batch(ctx, case, t.check_single(ctx, case))
    n += 1
ctx.close()
print("POISON_OK", n)
'''


def test_eigen_sweep_under_poison(tmp_path):
    """NMGP_POISON=1 (read once per process: a child) fills fresh buffers and every scratch hand-out with NaNs: an element the
    formulation reads without having written it -- a pad slot of k_sep_adjoint's sU (0 x NaN), a partial past the ragged end, a
    beta = 0 product onto a fresh C -- shows up.  1. and 4. of every case, forwards then backwards, at the same bars.  The references
    go to the child in a file, so that they are computed once."""
    for case in CASES:
        E.refs(case[0], case[1], case[2], all_chains(case))
    path = str(tmp_path / "refs.npz")
    E.save_refs(path)
    env = dict(os.environ)
    env["NMGP_POISON"] = "1"
    out = subprocess.run([sys.executable, "-c", POISON_SNIPPET % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "refs": path}],
                         capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0 and "POISON_OK %d" % (2 * len(CASES)) in out.stdout, out.stdout[-4000:] + out.stderr[-4000:]
