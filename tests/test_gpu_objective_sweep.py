"""The complete-data objectives on the GPU (run with -m gpu on an MI355X), M = 1 .. 8 around the tile, block and panel edges: the
nonseparable entries nmgp_logpos_svc and nmgp_svc_batch_eval (value+gradient, value-only, subject sets, the throughput schedule) and
the separable nmgp_logpos_sep / nmgp_sep_batch_eval against the CPU oracle, which tests/test_objective_sweep_cpu.py holds to
np.longdouble on the same subjects and chains (tests/objective_cases.py).

What is measured, per chain:
  priors off   likelihood 1e-10 relative; the gradient block by block (tilde_l, every slot column of uL, the sigma2 entry) at 1e-8 each,
               ||d_b|| / max(||gref_b||, 1e-3 ||gref||) -- a failure names the chain and the block; NegLog == -loglik
  priors on    the standing bars: NegLog 1e-6, likelihood 1e-9 and bit-equal to the priors-off call, the GP-prior components 1e-6 on
               the log det scale, the other components 1e-6; the PRIOR PART of the gradient, g(prior) - g(no prior), both from the
               GPU, against the oracle's same difference at 1e-5 in ||.|| (the prior solve; conditioning-bound)
  value-only   `out` against the value+gradient call's: likelihood 1e-11, the tuple 1e-9 (the bars of tests/test_svc_schur.py)
Every achieved error is recorded (objective_sweep/<case>/<entry>/prior<0|1>)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import objective_cases as C
from conftest import ROOT, prior_component_err_on_the_logdet_scale, record_parity, relerr, vec_relerr

pytestmark = pytest.mark.gpu

VAL_TOL = 1e-6          # the standing bars of tests/test_gpu_parity.py
LIK_TOL = 1e-9
GRAD_TOL = 1e-5
VALUE_ONLY_LIK, VALUE_ONLY_OUT = 1e-11, 1e-9        # tests/test_svc_schur.py
SEP_VALUE_ONLY_LIK = 1e-10                          # nmgp_sep_batch_eval's standing bar (test_separable_chains_batched_...)


@pytest.fixture(scope="module")
def ctx():
    from nonstationary_multivariate_gaussian_process_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


# ---------------------------------------------------------------------------------------------------
# the measures (also run by the NMGP_POISON child, which imports this module)
# ---------------------------------------------------------------------------------------------------
def hold_to_oracle(case, entry, layout, got, refs, rows=None, sweep="objective_sweep", bars=None):
    """got[prior] = (out [B, 5 | 6], grad [B, P]) of one entry, priors off and on; refs[b][prior] = the oracle's (out, grad) of batch
    row b; rows: the batch rows to compare (all).  Records the achieved errors and fails with every miss named.  sweep, bars: the
    record's prefix and the block-bar table of another sweep that reuses the measure (tests/test_gpu_eig_objective.py)."""
    model, N, M = layout
    (out0, g0), (out1, g1) = got[False], got[True]
    rows = range(len(refs)) if rows is None else rows
    e = dict(loglik=0.0, block=0.0, neglog=0.0, loglik1=0.0, gp=0.0, rest=0.0, prior_grad=0.0)
    worst, bad = (0.0, "-", -1), []
    for j, b in enumerate(rows):
        (r0, gr0), (r1, gr1) = refs[j][False], refs[j][True]
        # priors off
        el = relerr(out0[b][1], r0[1])
        e["loglik"] = max(e["loglik"], el)
        if not el < C.LIK_TIGHT:
            bad.append("row %d: likelihood %.3g >= %.0e (%r, oracle %r)" % (b, el, C.LIK_TIGHT, out0[b][1], r0[1]))
        if out0[b][0] != -out0[b][1]:
            bad.append("row %d: NegLog %r != -loglik %r without the priors" % (b, out0[b][0], out0[b][1]))
        eb, name = C.block_errors(g0[b], gr0, layout)
        if not eb <= worst[0]:
            worst = (eb, name, b)
        for name, err, bar in C.blocks_over_bar(g0[b], gr0, layout, bars=bars):
            bad.append("row %d: gradient block %s %.3g >= %.0e" % (b, name, err, bar))
        # priors on
        errs = dict(neglog=(relerr(out1[b][0], r1[0]), VAL_TOL), loglik1=(relerr(out1[b][1], r1[1]), LIK_TOL),
                    gp=(prior_component_err_on_the_logdet_scale(out1[b][2:4], r1[2:4], N), VAL_TOL),
                    rest=(relerr(out1[b][4:], r1[4:]), VAL_TOL), prior_grad=(vec_relerr(g1[b] - g0[b], gr1 - gr0), GRAD_TOL))
        for k, (err, bar) in errs.items():
            e[k] = max(e[k], err)
            if not err < bar:
                bad.append("row %d, priors on: %s %.3g >= %.0e (%r, oracle %r)" % (b, k, err, bar, out1[b], r1))
        if out1[b][1] != out0[b][1]:
            bad.append("row %d: the likelihood changes with the prior flag: %r, %r" % (b, out1[b][1], out0[b][1]))
    e["block"] = worst[0]
    tag = "%s/%s_%s/%s" % (sweep, model, case, entry)
    print("%s: loglik %.3g worst block %.3g (%s, row %d) | priors on: neglog %.3g loglik %.3g gp %.3g rest %.3g prior grad %.3g"
          % (tag, e["loglik"], worst[0], worst[1], worst[2], e["neglog"], e["loglik1"], e["gp"], e["rest"], e["prior_grad"]))
    record_parity(tag + "/prior0", loglik=(e["loglik"], C.LIK_TIGHT), worst_block=(e["block"], C.GRAD_TIGHT))
    record_parity(tag + "/prior1", neglog=(e["neglog"], VAL_TOL), loglik=(e["loglik1"], LIK_TOL),
                  prior_components_on_the_logdet_scale=(e["gp"], VAL_TOL), other_components=(e["rest"], VAL_TOL),
                  prior_grad=(e["prior_grad"], GRAD_TOL))
    assert not bad, "%s:\n  " % tag + "\n  ".join(bad)
    return e


def hold_value_only(case, entry, model, valued, graded, rows=None, lik_bar=VALUE_ONLY_LIK):
    """valued[prior] = out [B, .] of the value-only call, graded[prior] = that of the value+gradient call."""
    bad = []
    for prior in (False, True):
        ov, og = np.asarray(valued[prior]), np.asarray(graded[prior])
        if rows is not None:
            ov, og = ov[list(rows)], og[list(rows)]
        el, eo = relerr(ov[:, 1], og[:, 1]), relerr(ov, og)
        tag = "objective_sweep/%s_%s/%s/prior%d" % (model, case, entry, prior)
        print("%s: value-only vs value+gradient: loglik %.3g out %.3g" % (tag, el, eo))
        record_parity(tag, loglik_vs_grad_call=(el, lik_bar), out_vs_grad_call=(eo, VALUE_ONLY_OUT))
        if not (el < lik_bar and eo < VALUE_ONLY_OUT):
            bad.append("%s: loglik %.3g (bar %.0e) out %.3g (bar %.0e)\n%r\n%r" % (tag, el, lik_bar, eo, VALUE_ONLY_OUT, ov, og))
        if not prior and not np.array_equal(ov[:, 0], -ov[:, 1]):
            bad.append("%s: NegLog != -loglik without the priors" % tag)
    assert not bad, "\n".join(bad)


def svc_refs(N, M, B, s=0):
    return [{p: C.oracle("svc", N, M, k, p, s) for p in (False, True)} for k in range(B)]


def svc_batch(ctx, pars, prior, want_grad):
    ctx.svc_batch_set_pars(pars)
    ctx.svc_batch_eval(C.HYPER_SVC_VEC, prior, want_grad)
    out, st = ctx.svc_batch_fetch()
    grad = ctx.svc_batch_fetch_grad() if want_grad else None
    assert st.tolist() == [0] * pars.shape[0], st
    assert np.all(np.isfinite(out)) and (grad is None or np.all(np.isfinite(grad)))
    return out, grad


def run_svc_single(ctx, case, entry="single"):
    """(a) nmgp_logpos_svc, chain 0."""
    N, M = case
    x, Y, _ = C.subject("svc", N, M)
    ctx.set_data(x, Y)
    got = {}
    for prior in (False, True):
        out, grad = ctx.logpos_svc(C.chain("svc", N, M, 0), C.HYPER_SVC_VEC, prior=prior, want_grad=True)
        got[prior] = (out[None], grad[None])
    return hold_to_oracle(C.case_id(case), entry, ("svc", N, M), got, svc_refs(N, M, 1))


def run_svc_batches(ctx, case, B):
    """(b) nmgp_svc_batch_eval with gradient, every chain against the oracle; (c) the value-only batch (structured for M >= 2, dense
    at M = 1) against (b)'s out."""
    N, M = case
    x, Y, _ = C.subject("svc", N, M)
    ctx.set_data(x, Y)
    ctx.svc_batch_alloc(B)
    pars = C.chains("svc", N, M, B)
    got = {prior: svc_batch(ctx, pars, prior, True) for prior in (False, True)}
    hold_to_oracle(C.case_id(case), "batch%d_grad" % B, ("svc", N, M), got, svc_refs(N, M, B))
    valued = {prior: svc_batch(ctx, pars, prior, False)[0] for prior in (False, True)}
    hold_value_only(C.case_id(case), "batch%d_value" % B, "svc", valued, {p: got[p][0] for p in got})


# ---------------------------------------------------------------------------------------------------
# nonseparable
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.SVC_CASES, ids=C.case_id)
def test_svc_single_chain_entry(ctx, case):
    run_svc_single(ctx, case)


@pytest.mark.parametrize("B", C.SVC_BATCHES)
@pytest.mark.parametrize("case", C.SVC_CASES, ids=C.case_id)
def test_svc_batch_with_gradient_and_value_only(ctx, case, B):
    run_svc_batches(ctx, case, B)


@pytest.mark.parametrize("case", C.SUBJECT_SET_CASES, ids=C.case_id)
def test_svc_subject_set(ctx, case):
    """(d) 3 distinct subjects x 2 chains in one launch sequence, every chain against the oracle of its own subject (own inputs, own
    prior factors: k_prior_trsv, whose row-pair tail odd N takes); then the resident subject alone answers as in (a)."""
    N, M = case
    S, k = C.SUBJECTS, C.CHAINS_PER_SUBJECT
    subs = [C.subject("svc", N, M, s) for s in range(S)]
    ctx.set_data(subs[1][0], subs[1][1])                # the resident subject, which the set overrides, is not subject 0
    ctx.svc_batch_alloc(S * k)
    ctx.svc_batch_set_subjects(np.stack([s[0] for s in subs]), np.stack([s[1] for s in subs]), k)
    pars = np.stack([C.chain("svc", N, M, j, s) for s in range(S) for j in range(k)])
    refs = [{p: C.oracle("svc", N, M, j, p, s) for p in (False, True)} for s in range(S) for j in range(k)]
    got = {prior: svc_batch(ctx, pars, prior, True) for prior in (False, True)}
    hold_to_oracle(C.case_id(case), "subjects%dx%d_grad" % (S, k), ("svc", N, M), got, refs)
    valued = {prior: svc_batch(ctx, pars, prior, False)[0] for prior in (False, True)}
    hold_value_only(C.case_id(case), "subjects%dx%d_value" % (S, k), "svc", valued, {p: got[p][0] for p in got})
    # chains of different subjects really see different data
    assert abs(got[False][0][0][1] - got[False][0][k][1]) > 1e-3 * abs(got[False][0][0][1])
    run_svc_single(ctx, case, "single_after_subjects")  # set_data drops the set and the batch: the resident path


def test_svc_throughput_schedule_line(ctx):
    """(e) 128 chains of n = 579: 74,112 rows in all, the throughput schedule on a ragged last block.  Chains 0, 64 and 127 against
    the oracle; every chain status 0 and finite (the batch-against-single tests of tests/test_gpu_parity.py own the rest)."""
    (N, M), B, rows = C.SCHEDULE_CASE, C.SCHEDULE_B, C.SCHEDULE_CHAINS
    assert B * N * M > 73728
    x, Y, _ = C.subject("svc", N, M)
    ctx.set_data(x, Y)
    ctx.svc_batch_alloc(B)
    pars = C.chains("svc", N, M, B)
    refs = [{p: C.oracle("svc", N, M, k, p) for p in (False, True)} for k in rows]
    got = {prior: svc_batch(ctx, pars, prior, True) for prior in (False, True)}
    hold_to_oracle(C.case_id((N, M)), "batch%d_grad" % B, ("svc", N, M), got, refs, rows)
    valued = {prior: svc_batch(ctx, pars, prior, False)[0] for prior in (False, True)}
    hold_value_only(C.case_id((N, M)), "batch%d_value" % B, "svc", valued, {p: got[p][0] for p in got}, rows)
    ctx.svc_batch_alloc(1)                              # release the batch buffers


# ---------------------------------------------------------------------------------------------------
# separable
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.SEP_CASES, ids=C.case_id)
def test_sep_single_chain_entry(ctx, case):
    N, M = case
    x, Y, _ = C.subject("sep", N, M)
    ctx.set_data(x, Y)
    got = {}
    for prior in (False, True):
        out, grad = ctx.logpos_sep(C.chain("sep", N, M, 0), C.HYPER_SEP_VEC, prior=prior, want_grad=True)
        got[prior] = (out[None], grad[None])
    hold_to_oracle(C.case_id(case), "single", ("sep", N, M), got, [{p: C.oracle("sep", N, M, 0, p) for p in (False, True)}])


@pytest.mark.parametrize("case", C.SEP_CASES, ids=C.case_id)
def test_sep_batch_with_gradient_and_value_only(ctx, case):
    N, M = case
    B = C.SEP_BATCH
    x, Y, _ = C.subject("sep", N, M)
    ctx.set_data(x, Y)
    pars = C.chains("sep", N, M, B)
    got, valued = {}, {}
    for prior in (False, True):
        out, grad, st = ctx.sep_batch_eval(pars, C.HYPER_SEP_VEC, prior, True)
        outv, _, stv = ctx.sep_batch_eval(pars, C.HYPER_SEP_VEC, prior, False)
        assert st.tolist() == [0] * B and stv.tolist() == [0] * B, (st, stv)
        got[prior], valued[prior] = (out, grad), outv
    hold_to_oracle(C.case_id(case), "batch%d_grad" % B, ("sep", N, M), got,
                   [{p: C.oracle("sep", N, M, k, p) for p in (False, True)} for k in range(B)])
    hold_value_only(C.case_id(case), "batch%d_value" % B, "sep", valued, {p: got[p][0] for p in got}, lik_bar=SEP_VALUE_ONLY_LIK)


# ---------------------------------------------------------------------------------------------------
# once more with every fresh buffer and scratch hand-out full of NaNs
# ---------------------------------------------------------------------------------------------------
POISON_SNIPPET = r'''
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import objective_cases as C
import test_gpu_objective_sweep as t
from nonstationary_multivariate_gaussian_process_amd import _lib
C.load_oracle(%(oracle)r)
ctx = _lib.Context(0)
n = 0
for case in C.SVC_CASES + C.SVC_CASES[::-1]:
    t.run_svc_single(ctx, case)
    for B in C.SVC_BATCHES:
        t.run_svc_batches(ctx, case, B)
    n += 1
ctx.close()
print("POISON_OK", n)
'''


def test_svc_sweep_under_poison(tmp_path):
    """NMGP_POISON=1 (read once per process: a child) fills fresh buffers and every scratch hand-out with NaNs: an element an entry
    reads without having written it -- the seeded band of L^-T, a block sum past the ragged end, a pad row -- shows up.  (a) - (c) of
    every nonseparable case, forwards then backwards so that the workspace shrinks as well as grows, at the same bars.  The oracle
    values go to the child in a file, so that they are computed once."""
    for N, M in C.SVC_CASES:
        svc_refs(N, M, max(C.SVC_BATCHES))
    path = str(tmp_path / "oracle.npz")
    C.save_oracle(path)
    env = dict(os.environ)
    env["NMGP_POISON"] = "1"
    out = subprocess.run([sys.executable, "-c", POISON_SNIPPET % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "oracle": path}],
                         capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0 and "POISON_OK %d" % (2 * len(C.SVC_CASES)) in out.stdout, out.stdout[-4000:] + out.stderr[-4000:]
