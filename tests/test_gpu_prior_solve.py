"""The GP-prior solves on the GPU (run with -m gpu on an MI355X): every site that solves op(L) X = R against the cached factors of
RBF(x; alpha, beta) + 1e-6 I, on every branch it can take -- the library's dtrsm in its plain, strided and per-subject forms and the
substitution kernel k_prior_trsv -- against the np.longdouble reference of tests/prior_solve_cases.py, on well-conditioned, fully
populated factors (kappa <= 3500), with the same pair of hyper-parameters for both factors and with different pairs.

Three contexts live in this process: `default`, `rocblas` (NMGP_PRIOR_SOLVE=rocblas: the library everywhere, which is also the code
every Hadamard entry runs beyond N = 3500) and `trsv` (substitution everywhere).  The variable is read when a context is created.

  A  logpos_svc and svc_batch_eval on the resident subject            default (library), trsv
  B  svc_batch_set_subjects, cps = 1 and 2, both sides of 32 columns   default, rocblas, trsv
  C  logpos_sep, sep_batch_eval, sep_batch_set_subjects                default, trsv; subjects: default, rocblas
  D  had_batch_eval and hads_batch_eval                                default (substitution), rocblas
  E  had_subjects_eval on a ragged cohort, in one chunk and in three   default
  P  the starred values of the predictors, z = None and z = 1          default, rocblas

Measured: the prior part of the gradient g(prior = 1) - g(prior = 0), block by block, and the two verbose prior components relative to
themselves; value-only calls: the components.  The bars are 50 x the float64 restatement's own worst error per table
(prior_solve_cases.BAR, held by tests/test_prior_solve_cpu.py), none above 1e-10.  Where the code promises bits they are checked: a
substitution-solved chain alone against its row of the batch, a multi-subject chain against the same subject resident under `trsv`.
Every row is recorded as prior_solve/<table>/<case>/<context>/<variant>/<entry>/<quantity> [branch]; the branch is looked up in
prior_solve_cases.branch_map by the first five, never written here."""
import os
import subprocess
import sys

import numpy as np
import pytest

import prior_solve_cases as C
from conftest import ROOT, record_parity

pytestmark = pytest.mark.gpu

ENV = "NMGP_PRIOR_SOLVE"
SLAB_ENV = "NMGP_HAD_BATCH_SLAB_GB"


def make_contexts():
    """The three contexts, each created with NMGP_PRIOR_SOLVE set for the duration of the constructor only"""
    from nonstationary_multivariate_gaussian_process_amd import _lib
    out = {}
    for name in C.CONTEXTS:
        old = os.environ.get(ENV)
        try:
            if name == "default":
                os.environ.pop(ENV, None)
            else:
                os.environ[ENV] = name
            out[name] = _lib.Context(0)
        finally:
            if old is None:
                os.environ.pop(ENV, None)
            else:
                os.environ[ENV] = old
    return out


@pytest.fixture(scope="module")
def ctxs():
    cs = make_contexts()
    yield cs
    for c in cs.values():
        c.close()


# ---------------------------------------------------------------------------------------------------
# the measure (also run by the NMGP_POISON child, which imports this module)
# ---------------------------------------------------------------------------------------------------
def case_name(key, what):
    """prior_solve/<table>/<case>/<context>/<variant>/<entry>/<what> [branch]: the branch is the map's for the key"""
    return "prior_solve/%s/%s [%s]" % ("/".join(key), what, C.branch_of(*key))


def hold(key, what, comps, dgrad, ref, layout, N, M, bad):
    """One entry's chains under BAR[table]: every gradient block (dgrad None: a value-only call) and both components; the worst block
    is named and everything recorded.  key = (table, case, context, variant, entry) of prior_solve_cases.branch_map."""
    table, tag = key[0], "/".join(key[1:]) + "/" + what
    bar = C.BAR[table]
    assert np.all(np.isfinite(comps)) and (dgrad is None or np.all(np.isfinite(dgrad))), "%s: a non-finite output" % tag
    errs = C.errors(comps, dgrad, ref, layout, N, M)
    blocks = {k: v for k, v in errs.items() if not k.startswith("component")}
    case = case_name(key, what)
    row = dict(component0=(errs["component0"], bar), component1=(errs["component1"], bar))
    if blocks:
        e, name = C.worst(blocks)
        row["worst_block"] = (e, bar)
        print("%s: worst block %.3g (%s), components %.3g %.3g, bar %.3g" % (case, e, name, errs["component0"], errs["component1"], bar))
    else:
        print("%s: components %.3g %.3g, bar %.3g" % (case, errs["component0"], errs["component1"], bar))
    record_parity(case, **row)
    for k, e in errs.items():
        if not e < bar:
            bad.append("%s %s: %.3g >= %.3g" % (case, k, e, bar))


def rows_ref(ref, rows):
    return dict(comps=ref["comps"][rows], grad=ref["grad"][rows])


def svc_batch(ctx, pars, hv, prior, want_grad):
    ctx.svc_batch_set_pars(pars)
    ctx.svc_batch_eval(hv, prior, want_grad)
    out, st = ctx.svc_batch_fetch()
    grad = ctx.svc_batch_fetch_grad() if want_grad else None
    assert st.tolist() == [0] * pars.shape[0], st
    return out, grad


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------------------
# A: the resident subject of the nonseparable model
# ---------------------------------------------------------------------------------------------------
def run_table_a(ctxs, case, variant):
    N, M = case
    x, Y = C.complete_subject(N, M)
    V = C.complete_chains("svc", N, M, 5)
    hv = C.hyper_vec("svc", variant)
    ref = C.prior_terms(x, "svc", M, V, variant)
    bad = []
    for context in ("default", "trsv"):
        ctx = ctxs[context]
        ctx.set_data(x, Y)
        tag = "N%d_M%d/%s/%s" % (N, M, context, variant)
        key = ("A", "N%d_M%d" % (N, M), context, variant, "single")
        o1, g1 = ctx.logpos_svc(V[0], hv, prior=True, want_grad=True)
        o0, g0 = ctx.logpos_svc(V[0], hv, prior=False, want_grad=True)
        hold(key, "grad", o1[2:4], g1 - g0, rows_ref(ref, [0]), "svc", N, M, bad)
        ov, _ = ctx.logpos_svc(V[0], hv, prior=True, want_grad=False)
        hold(key, "value", ov[2:4], None, rows_ref(ref, [0]), "svc", N, M, bad)
        outs = {}
        for B in C.BATCHES_A:
            key = key[:4] + ("batch%d" % B,)
            ctx.svc_batch_alloc(B)
            o1, g1 = svc_batch(ctx, V[:B], hv, True, True)
            o0, g0 = svc_batch(ctx, V[:B], hv, False, True)
            hold(key, "grad", o1[:, 2:4], g1 - g0, rows_ref(ref, slice(0, B)), "svc", N, M, bad)
            ov, _ = svc_batch(ctx, V[:B], hv, True, False)
            hold(key, "value", ov[:, 2:4], None, rows_ref(ref, slice(0, B)), "svc", N, M, bad)
            outs[B] = (o1, g1)
        if context == "trsv":
            # the copy of chain 0 in the batch of 5 shares every launch with chain 0: its whole row and gradient, the transposed
            # substitution included, to the bit (no bit promise is asserted for the library forms)
            if not (same_bytes(outs[5][0][4], outs[5][0][0]) and same_bytes(outs[5][1][4], outs[5][1][0])):
                bad.append("%s: the copy of chain 0 in the batch of 5 differs from chain 0 in bits" % tag)
            # a column's substitution does not depend on the columns next to it: chain 0 alone and in the batch of 5.  Only the
            # components are promised between batch sizes: the gradient row carries the likelihood part, whose factorisation
            # schedule changes with the batch (the one quantity that is the transposed solve alone is not returned)
            if not same_bytes(outs[1][0][0, 2:4], outs[5][0][0, 2:4]):
                bad.append("%s: the prior components of chain 0 alone and in the batch of 5 differ in bits" % tag)
    assert not bad, "table A:\n  " + "\n  ".join(bad)


@pytest.mark.parametrize("variant", C.VARIANTS)
@pytest.mark.parametrize("case", C.TABLE_A, ids=lambda c: "N%d_M%d" % c)
def test_table_a_resident_nonseparable(ctxs, case, variant):
    run_table_a(ctxs, case, variant)


# ---------------------------------------------------------------------------------------------------
# B: subject sets of the nonseparable model
# ---------------------------------------------------------------------------------------------------
def run_table_b(ctxs, case, variant):
    M, cps = case
    N, S = C.N_B, C.SUBJECTS
    B = S * cps
    subs = [C.complete_subject(N, M, s) for s in range(S)]
    xs, Ys = np.stack([s[0] for s in subs]), np.stack([s[1] for s in subs])
    chains = [C.complete_chains("svc", N, M, 2, s)[:cps] for s in range(S)]
    pars = np.concatenate(chains)
    hv = C.hyper_vec("svc", variant)
    refs = [C.prior_terms(xs[s], "svc", M, chains[s], variant) for s in range(S)]
    bad = []
    for context in C.CONTEXTS:
        ctx = ctxs[context]
        key = ("B", "M%d_cps%d" % (M, cps), context, variant, "set")
        ctx.set_data(xs[1], Ys[1])                      # the resident subject, which the set overrides, is not subject 0
        ctx.svc_batch_alloc(B)
        ctx.svc_batch_set_subjects(xs, Ys, cps)
        o1, g1 = svc_batch(ctx, pars, hv, True, True)
        o0, g0 = svc_batch(ctx, pars, hv, False, True)
        ov, _ = svc_batch(ctx, pars, hv, True, False)
        for s in range(S):
            rows = slice(s * cps, (s + 1) * cps)
            hold(key, "subject%d_grad" % s, o1[rows, 2:4], (g1 - g0)[rows], refs[s], "svc", N, M, bad)
            hold(key, "subject%d_value" % s, ov[rows, 2:4], None, refs[s], "svc", N, M, bad)
        if context == "trsv":
            # the same chain with its subject resident: the same substitution on the same factor, to the bit.  The components
            # only: the gradient row carries the likelihood part, for which the set and the resident subject promise no bits
            for s in (0, 2):
                ctx.set_data(xs[s], Ys[s])
                ctx.svc_batch_alloc(cps)
                r1, _ = svc_batch(ctx, chains[s], hv, True, True)
                if not same_bytes(r1[:, 2:4], o1[s * cps:(s + 1) * cps, 2:4]):
                    bad.append("M%d_cps%d/%s: subject %d in the set and resident differ in the bits of the prior components"
                               % (M, cps, variant, s))
    assert not bad, "table B:\n  " + "\n  ".join(bad)


@pytest.mark.parametrize("variant", C.VARIANTS)
@pytest.mark.parametrize("case", C.TABLE_B, ids=lambda c: "M%d_cps%d" % c)
def test_table_b_subject_sets(ctxs, case, variant):
    run_table_b(ctxs, case, variant)


# ---------------------------------------------------------------------------------------------------
# C: the separable model
# ---------------------------------------------------------------------------------------------------
def sep_batch(ctx, pars, hv, prior, want_grad):
    out, grad, st = ctx.sep_batch_eval(pars, hv, prior, want_grad)
    assert st.tolist() == [0] * pars.shape[0], st
    return out, grad


def run_table_c(ctxs, case, variant):
    N, M = case
    x, Y = C.complete_subject(N, M)
    V = C.complete_chains("sep", N, M, C.BATCH_C)
    hv = C.hyper_vec("sep", variant)
    ref = C.prior_terms(x, "sep", M, V, variant)
    bad = []
    for context in ("default", "trsv"):
        ctx = ctxs[context]
        ctx.set_data(x, Y)
        key = ("C", "N%d_M%d" % (N, M), context, variant, "single")
        o1, g1 = ctx.logpos_sep(V[0], hv, prior=True, want_grad=True)
        o0, g0 = ctx.logpos_sep(V[0], hv, prior=False, want_grad=True)
        hold(key, "grad", o1[2:4], g1 - g0, rows_ref(ref, [0]), "sep", N, M, bad)
        ov, _ = ctx.logpos_sep(V[0], hv, prior=True, want_grad=False)
        hold(key, "value", ov[2:4], None, rows_ref(ref, [0]), "sep", N, M, bad)
        key = key[:4] + ("batch%d" % C.BATCH_C,)
        o1, g1 = sep_batch(ctx, V, hv, True, True)
        o0, g0 = sep_batch(ctx, V, hv, False, True)
        hold(key, "grad", o1[:, 2:4], g1 - g0, ref, "sep", N, M, bad)
        ov, _ = sep_batch(ctx, V, hv, True, False)
        hold(key, "value", ov[:, 2:4], None, ref, "sep", N, M, bad)
    assert not bad, "table C:\n  " + "\n  ".join(bad)


def run_table_c_subjects(ctxs, case, variant):
    N, M = case
    S, cps = C.SUBJECTS, C.CPS_C
    subs = [C.complete_subject(N, M, s) for s in range(S)]
    xs, Ys = np.stack([s[0] for s in subs]), np.stack([s[1] for s in subs])
    chains = [C.complete_chains("sep", N, M, cps, s) for s in range(S)]
    pars = np.concatenate(chains)
    hv = C.hyper_vec("sep", variant)
    refs = [C.prior_terms(xs[s], "sep", M, chains[s], variant) for s in range(S)]
    bad = []
    for context in ("default", "rocblas"):
        ctx = ctxs[context]
        key = ("C", "subjects_N%d_M%d" % (N, M), context, variant, "set")
        ctx.set_data(xs[1], Ys[1])
        ctx.sep_batch_set_subjects(xs, Ys, cps)
        try:
            o1, g1 = sep_batch(ctx, pars, hv, True, True)
            o0, g0 = sep_batch(ctx, pars, hv, False, True)
            ov, _ = sep_batch(ctx, pars, hv, True, False)
        finally:
            ctx.sep_batch_clear_subjects()
        for s in range(S):
            rows = slice(s * cps, (s + 1) * cps)
            hold(key, "subject%d_grad" % s, o1[rows, 2:4], (g1 - g0)[rows], refs[s], "sep", N, M, bad)
            hold(key, "subject%d_value" % s, ov[rows, 2:4], None, refs[s], "sep", N, M, bad)
    assert not bad, "table C, subjects:\n  " + "\n  ".join(bad)


@pytest.mark.parametrize("variant", C.VARIANTS)
@pytest.mark.parametrize("case", C.TABLE_C, ids=lambda c: "N%d_M%d" % c)
def test_table_c_resident_separable(ctxs, case, variant):
    run_table_c(ctxs, case, variant)


@pytest.mark.parametrize("variant", C.VARIANTS)
@pytest.mark.parametrize("case", C.SUBJECT_CASES_C, ids=lambda c: "N%d_M%d" % c)
def test_table_c_separable_subject_sets(ctxs, case, variant):
    run_table_c_subjects(ctxs, case, variant)


# ---------------------------------------------------------------------------------------------------
# D: the Hadamard models
# ---------------------------------------------------------------------------------------------------
HAD_ENTRY = {"svc": "had_batch_eval", "sep": "hads_batch_eval"}


def run_table_d(ctxs, case, variant):
    N, M, layout = case
    h = C.hadamard_subject(N, M, layout)
    bad = []
    for context in ("default", "rocblas"):
        ctx = ctxs[context]
        ctx.had_set_data(h["x"], h["indx"], h["y"], M=M)
        for lay in ("svc", "sep"):
            ev = getattr(ctx, HAD_ENTRY[lay])
            V = h["chains"][lay]
            hv = C.hyper_vec(lay, variant)
            ref = C.prior_terms(h["x"], lay, M, V, variant)
            got = {}
            key = ("D", "N%d_M%d_%s" % (N, M, layout), context, variant, HAD_ENTRY[lay])
            for B in C.BATCHES_D:
                tag = "/".join(key) + "/batch%d" % B
                o1, g1, s1 = ev(V[:B], hv, prior=True, want_grad=True)
                o0, g0, s0 = ev(V[:B], hv, prior=False, want_grad=True)
                ov, _, sv = ev(V[:B], hv, prior=True, want_grad=False)
                assert s1.tolist() == s0.tolist() == sv.tolist() == [0] * B, (tag, s1, s0, sv)
                hold(key, "batch%d_grad" % B, o1[:, 2:4], g1 - g0, rows_ref(ref, slice(0, B)), lay, N, M, bad)
                hold(key, "batch%d_value" % B, ov[:, 2:4], None, rows_ref(ref, slice(0, B)), lay, N, M, bad)
                got[B] = (o1, g1)
            if context == "default":
                # by substitution a column's bits do not depend on how many chains share the launch
                if not (same_bytes(got[1][0][0], got[3][0][0]) and same_bytes(got[1][1][0], got[3][1][0])):
                    bad.append("N%d_M%d_%s/%s/%s: chain 0 alone differs in bits from its row of the batch" % (N, M, layout, variant, HAD_ENTRY[lay]))
    assert not bad, "table D:\n  " + "\n  ".join(bad)


@pytest.mark.parametrize("variant", C.VARIANTS)
@pytest.mark.parametrize("case", C.TABLE_D, ids=lambda c: "N%d_M%d_%s" % c)
def test_table_d_hadamard_models(ctxs, case, variant):
    run_table_d(ctxs, case, variant)


# ---------------------------------------------------------------------------------------------------
# E: a ragged cohort of Hadamard subjects
# ---------------------------------------------------------------------------------------------------
def run_table_e(ctxs, cps, variant):
    """cps = 1, 2: the cohort in one chunk.  cps = COHORT_SPLIT_CPS: the two chains of every subject tiled, under the smallest
    NMGP_HAD_BATCH_SLAB_GB (read at every call), which makes three whole-subject chunks starting at subjects 0, 1 and 2
    (prior_solve_cases.cohort_chunks): the factors and log-determinants of a chunk at s0 > 0."""
    from nonstationary_multivariate_gaussian_process_amd import hadamard
    ctx = ctxs["default"]
    subs = C.cohort()
    nobs, M = list(C.COHORT_NOBS), C.COHORT_M
    hv = C.hyper_vec("svc", variant)
    split = cps == C.COHORT_SPLIT_CPS
    own = [h["chains"]["svc"][:min(cps, 2)] for h in subs]
    pick = np.arange(cps) % 2 if split else np.arange(cps)                     # row j of a subject is its chain pick[j]
    pars = hadamard.cohort_pack([v[pick] for v in own], nobs, M)
    key = ("E", "cps%d" % cps, "default", variant, "cohort")
    bad = []
    old = os.environ.get(SLAB_ENV)
    ctx.had_set_subjects([h["x"] for h in subs], [h["indx"] for h in subs], [h["y"] for h in subs], M=M)
    try:
        if split:
            os.environ[SLAB_ENV] = "%g" % C.COHORT_SPLIT_CAP_GB
        o1, g1, s1 = ctx.had_subjects_eval(pars, hv, prior=True, want_grad=True, chains_per_subject=cps)
        o0, g0, s0 = ctx.had_subjects_eval(pars, hv, prior=False, want_grad=True, chains_per_subject=cps)
        ov, _, sv = ctx.had_subjects_eval(pars, hv, prior=True, want_grad=False, chains_per_subject=cps)
    finally:
        if old is None:
            os.environ.pop(SLAB_ENV, None)
        else:
            os.environ[SLAB_ENV] = old
        ctx.had_clear_subjects()
    assert not s1.any() and not s0.any() and not sv.any(), (s1, s0, sv)
    dg = hadamard.cohort_unpack(g1 - g0, nobs, M, cps)
    for s, h in enumerate(subs):
        rows = slice(s * cps, (s + 1) * cps)
        two = C.prior_terms(h["x"], "svc", M, own[s], variant)
        ref = dict(comps=two["comps"][pick], grad=two["grad"][pick])
        hold(key, "subject%d_N%d_grad" % (s, nobs[s]), o1[rows, 2:4], dg[s], ref, "svc", nobs[s], M, bad)
        hold(key, "subject%d_N%d_value" % (s, nobs[s]), ov[rows, 2:4], None, ref, "svc", nobs[s], M, bad)
        if split and not (same_bytes(o1[rows][2:], o1[rows][:-2]) and same_bytes(g1[rows][2:], g1[rows][:-2])):
            bad.append("cps%d/%s: the tiled copies of subject %d's chains differ in bits" % (cps, variant, s))
    assert not bad, "table E:\n  " + "\n  ".join(bad)


@pytest.mark.parametrize("variant", C.VARIANTS)
@pytest.mark.parametrize("cps", C.COHORT_CPS + (C.COHORT_SPLIT_CPS,))
def test_table_e_ragged_cohort(ctxs, cps, variant):
    run_table_e(ctxs, cps, variant)


# ---------------------------------------------------------------------------------------------------
# P: the projections of the predictors
# ---------------------------------------------------------------------------------------------------
def hold_star(key, got, ref, bad, what="star"):
    e = C.star_errors(got, ref)
    case = case_name(key, what)
    print("%s: %.3g, bar %.3g" % (case, e, C.BAR["P"]))
    record_parity(case, **{what: (e, C.BAR["P"])})
    if not e < C.BAR["P"]:
        bad.append("%s: %.3g >= %.3g" % (case, e, C.BAR["P"]))


def run_table_p(ctxs, case, variant):
    N, M = case
    T = C.n_slots(M)
    x, Y = C.complete_subject(N, M)
    xs = C.new_inputs(x)
    h = C.hadamard_subject(N, M, "unsorted")
    hxs = C.new_inputs(h["x"])
    dslots = np.cumsum(np.arange(1, M + 1)) - 1
    bad = []
    for context in ("default", "rocblas"):
        ctx = ctxs[context]

        def key(entry):
            return ("P", "N%d_M%d" % (N, M), context, variant, entry)
        # the complete-data models
        ctx.set_data(x, Y)
        V = C.complete_chains("svc", N, M, 2)
        hv = C.hyper_vec("svc", variant)
        ref = C.projection_terms(x, xs, "svc", M, V, variant, curve=C.constrained_curve(N, M))
        _, _, s0, st = ctx.predsample_svc(V, hv, xs, constrained=True)
        _, _, s1, st1 = ctx.predsample_svc(V, hv, xs, z=np.ones((2, C.S_NEW, 1 + T)), constrained=True)
        assert st.tolist() == st1.tolist() == [0, 0]
        hold_star(key("predsample_svc"), s0, ref["star"], bad)
        hold_star(key("predsample_svc"), s1 - s0, ref["sd"], bad, "sqrt_cv")
        raw = C.projection_terms(x, xs, "svc", M, V[:1], variant)["star"][:, :, 1:].copy()
        raw[:, :, dslots] = np.exp(raw[:, :, dslots])
        _, _, Ls = ctx.predict_svc(V[0], hv, xs)
        hold_star(key("predict_svc"), Ls[None], raw, bad)
        V = C.complete_chains("sep", N, M, 2)
        hv = C.hyper_vec("sep", variant)
        ref = C.projection_terms(x, xs, "sep", M, V, variant)
        _, _, s0, st = ctx.predsample_sep(V, hv, xs)
        _, _, s1, st1 = ctx.predsample_sep(V, hv, xs, z=np.ones((2, C.S_NEW, 2)))
        assert st.tolist() == st1.tolist() == [0, 0]
        hold_star(key("predsample_sep"), s0, ref["star"], bad)
        hold_star(key("predsample_sep"), s1 - s0, ref["sd"], bad, "sqrt_cv")
        # the Hadamard models
        ctx.had_set_data(h["x"], h["indx"], h["y"], M=M)
        for lay, ps, pm, width in (("svc", ctx.predsample_had, ctx.predict_had, 1 + T), ("sep", ctx.predsample_hads, ctx.predict_hads, 2)):
            V = h["chains"][lay][:2]
            hv = C.hyper_vec(lay, variant)
            ref = C.projection_terms(h["x"], hxs, lay, M, V, variant)
            _, _, s0, st = ps(V, hv, hxs)
            _, _, s1, st1 = ps(V, hv, hxs, z=np.ones((2, C.S_NEW, width)))
            assert st.tolist() == st1.tolist() == [0, 0]
            hold_star(key(ps.__name__), s0, ref["star"], bad)
            hold_star(key(ps.__name__), s1 - s0, ref["sd"], bad, "sqrt_cv")
            _, _, sm = pm(V[0], hv, hxs)
            hold_star(key(pm.__name__), sm[None], ref["star"][:1], bad)
    assert not bad, "table P:\n  " + "\n  ".join(bad)


@pytest.mark.parametrize("variant", C.VARIANTS)
@pytest.mark.parametrize("case", C.TABLE_P, ids=lambda c: "N%d_M%d" % c)
def test_table_p_projections(ctxs, case, variant):
    run_table_p(ctxs, case, variant)


# ---------------------------------------------------------------------------------------------------
# once more with every fresh buffer and scratch hand-out full of NaNs, forwards and backwards
# ---------------------------------------------------------------------------------------------------
def run_everything(ctxs, reverse=False):
    jobs = [(run_table_a, c) for c in C.TABLE_A] + [(run_table_b, c) for c in C.TABLE_B] + [(run_table_c, c) for c in C.TABLE_C]
    jobs += [(run_table_c_subjects, c) for c in C.SUBJECT_CASES_C] + [(run_table_d, c) for c in C.TABLE_D]
    jobs += [(run_table_e, c) for c in C.COHORT_CPS + (C.COHORT_SPLIT_CPS,)] + [(run_table_p, c) for c in C.TABLE_P]
    n = 0
    for fn, case in (jobs[::-1] if reverse else jobs):
        for variant in (C.VARIANTS[::-1] if reverse else C.VARIANTS):
            fn(ctxs, case, variant)
            n += 1
    return n


POISON_SNIPPET = r'''
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import test_gpu_prior_solve as t
ctxs = t.make_contexts()
n = t.run_everything(ctxs) + t.run_everything(ctxs, reverse=True)
for c in ctxs.values():
    c.close()
print("POISON_OK", n)
'''


def test_sweep_under_poison():
    """NMGP_POISON=1 (read once per process: a child) fills fresh buffers and every scratch hand-out with NaNs: an element a solve
    reads without its having been written -- a factor's padding, the pad of a right-hand side, a masked factor's tail -- shows up.
    Every table, forwards and then backwards so that the workspaces shrink as well as grow, at the same bars."""
    env = dict(os.environ)
    env["NMGP_POISON"] = "1"
    env.pop(ENV, None)
    env.pop(SLAB_ENV, None)
    out = subprocess.run([sys.executable, "-c", POISON_SNIPPET % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}],
                         capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    n = 2 * len(C.VARIANTS) * (len(C.TABLE_A) + len(C.TABLE_B) + len(C.TABLE_C) + len(C.SUBJECT_CASES_C) + len(C.TABLE_D)
                               + len(C.COHORT_CPS) + 1 + len(C.TABLE_P))
    assert out.returncode == 0 and "POISON_OK %d" % n in out.stdout, out.stdout[-4000:] + out.stderr[-4000:]
