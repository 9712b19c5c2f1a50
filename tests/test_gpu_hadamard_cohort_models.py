"""GPU half of the cohort tests of the separable ("sep") and stationary ("sta") Hadamard models: nmgp_hads_subjects_eval /
nmgp_hadst_subjects_eval on the set of nmgp_had_set_subjects against the NumPy restatements hadamard_cases.ref_logpos(model, ...) on
each subject ALONE, at the sets of tests/hadamard_cohort_cases.py; tests/test_hadamard_cohort_models_cpu.py checks the subjects'
preconditions and the padded formulations.  The file mirrors tests/test_gpu_hadamard_cohort.py.

Bars: eval_errors(model, ...) of tests/test_gpu_hadamard_sweep.py, the standing bars of the two models and the gradient block by block
(hadamard_cases.block_bar of the subject in its set; sep with the priors: the prior part at 1e-5).  Sets F - H (M = 4, 6, 7) run
everything sets A - E run; set I (Nmax = 1030) with one chain per subject, here and in "padding is inert".  Padding inert, a subject
alone against its rows of the set, value-only against value + gradient, chunked against unchunked, and a subject without padding
against the resident path (sta: everything; sep: the likelihood, and without priors NegLog and the gradient): bit for bit.  Drivers:
1e-6 relative on the log-posterior history, the standing bar between two evaluation paths."""
import os
import subprocess
import sys

import numpy as np
import pytest

import hadamard_cases as hc
import hadamard_cohort_cases as cc
import hadamard_cohort_model_cases as mc
from conftest import ROOT, prior_component_err_on_the_logdet_scale, record_parity, relerr
from test_gpu_hadamard_sweep import VAL_TOL, check, eval_errors, same_bits

pytestmark = pytest.mark.gpu

MODELS = mc.MODELS


@pytest.fixture(scope="module")
def ctx():
    from nonstationary_multivariate_gaussian_process_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def set_subjects(ctx, cases, Nmax=None):
    subs = cc.subjects(cases)
    ctx.had_set_subjects([c["x"] for c in subs], [c["indx"] for c in subs], [c["y"] for c in subs], M=cases[0][1], Nmax=Nmax)


def packed(model, cases, k, Nmax=None, fill=0.0):
    return mc.pack(model, mc.chains(model, cases, k), cc.nobs(cases), cases[0][1], Nmax=Nmax, fill=fill)


def entry(ctx, model):
    return getattr(ctx, mc.ENTRY[model])


def no_sign_bit_zeros(a):
    return np.all(a == 0.0) and not np.any(np.signbit(a))


def meets_the_restatement(model, out, grad, status, cases, k, prior, tag, Nmax, plain):
    """every chain's tuple and the real slots of its gradient against the restatement on the subject alone, the gradient block by
    block too (`plain`: the entry's gradient without the priors, which the prior part is taken against); padded slots +0.0"""
    S, M = len(cases), cases[0][1]
    assert status.tolist() == [0] * (S * k) and out.shape == (S * k, mc.WIDTH[model]) and grad.shape == (S * k, mc.plen(model, Nmax, M))
    pads = mc.padded_slots(model, cc.nobs(cases), M, Nmax, k)
    assert no_sign_bit_zeros(grad[pads])
    real, real_plain = mc.unpack(model, grad, cc.nobs(cases), M, k), mc.unpack(model, plain, cc.nobs(cases), M, k)
    for s, case in enumerate(cases):
        for j in range(k):
            ref_out, ref_grad = mc.reference(model, case, j, prior)
            check("hcohort_models/%s/%s/k%d/prior%d/%s/chain%d" % (model, tag, k, prior, hc.case_id(case), j),
                  **eval_errors(model, out[s * k + j], real[s][j], ref_out, ref_grad, prior, case[0], M, hc.block_bar(model, case, Nmax),
                                without=(real_plain[s][j], mc.reference(model, case, j, False)[1])))


def evaluate_set(ctx, model, cases, k, tag, Nmax=None):
    set_subjects(ctx, cases, Nmax)
    P = packed(model, cases, k, Nmax)
    res = {prior: entry(ctx, model)(P, mc.hyper_of(model, cases), prior=prior, want_grad=True, chains_per_subject=k) for prior in (True, False)}
    assert np.array_equal(res[False][0][:, 0], -res[False][0][:, 1])
    for prior in (True, False):
        meets_the_restatement(model, *res[prior], cases, k, prior, tag, max(cc.nobs(cases)) if Nmax is None else Nmax, res[False][1])


# ---- 1. against the restatement -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("name", sorted(cc.SETS))
def test_every_chain_of_the_set_meets_the_restatement_on_its_subject_alone(ctx, name, k, model):
    evaluate_set(ctx, model, cc.SETS[name], k, name)


@pytest.mark.parametrize("model", MODELS)
def test_set_I_meets_the_restatement_beyond_one_panel_and_one_trace_pass(ctx, model):
    """Nmax = 1030, one chain per subject (tests/hadamard_cohort_cases.py): the trace kernel's second pass for N_s = 1030 and 1025, two
    512-column panels, 2 Nmax + 2 = 2062 riding rows."""
    evaluate_set(ctx, model, cc.SET_I, 1, "I")


# ---- 2. padding is inert ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_padding_is_inert(ctx, model):
    padding_is_inert(ctx, model, cc.SET_A, 2)


@pytest.mark.parametrize("model", MODELS)
def test_padding_is_inert_in_set_I(ctx, model):
    padding_is_inert(ctx, model, cc.SET_I, 1)


def padding_is_inert(ctx, model, cases, k):
    from nonstationary_multivariate_gaussian_process_amd import _lib
    M, B = cases[0][1], len(cases) * k
    sizes, Nmax = cc.nobs(cases), max(cc.nobs(cases))
    subs = cc.subjects(cases)
    ev = entry(ctx, model)
    x, y, indx = np.zeros((len(cases), Nmax)), np.zeros((len(cases), Nmax)), np.zeros((len(cases), Nmax), dtype=np.int32)
    for s, c in enumerate(subs):
        x[s, :sizes[s]], y[s, :sizes[s]], indx[s, :sizes[s]] = c["x"], c["y"], c["indx"]
    ctx.had_set_subjects_padded(x, indx, y, sizes, M)
    hyper = mc.hyper_of(model, cases)
    clean = {prior: ev(packed(model, cases, k), hyper, prior=prior, want_grad=True, chains_per_subject=k) for prior in (True, False)}
    for s, n in enumerate(sizes):                       # poison in every padded slot of the data
        x[s, n:], y[s, n:] = np.nan, np.nan
        indx[s, n:] = np.where(np.arange(Nmax - n) % 2 == 0, -1, 99)
    ctx.had_set_subjects_padded(x, indx, y, sizes, M)
    pads = mc.padded_slots(model, sizes, M, Nmax, k)
    assert pads.sum() > 0 if model == "sep" else pads.sum() == 0
    for fill in (np.nan, 1e300):                        # ... and (sep) in every padded parameter slot
        P = packed(model, cases, k, fill=fill)
        assert np.all(P[pads] == fill) if np.isfinite(fill) else np.all(np.isnan(P[pads]))
        for prior in (True, False):
            got = ev(P, hyper, prior=prior, want_grad=True, chains_per_subject=k)
            assert got[2].tolist() == [0] * B and same_bits(got, clean[prior]), (fill, prior)
            assert no_sign_bit_zeros(got[1][pads])
            val = ev(P, hyper, prior=prior, want_grad=False, chains_per_subject=k)
            assert val[1] is None and np.array_equal(val[0], clean[prior][0]) and val[2].tolist() == got[2].tolist()
    # a NaN in a REAL slot is reported for that chain alone
    P = packed(model, cases, k, fill=np.nan)
    bad = 2 * k - 1                                     # the last chain of subject 1 (set A: 63 observations): tilde_l[1] / tilde_sigma
    assert sizes[1] < Nmax and (k, bad) in ((2, 3), (1, 1))
    P[bad, 1] = np.nan
    out, grad, status = ev(P, hyper, prior=True, want_grad=True, chains_per_subject=k)
    assert status.tolist() == [_lib.NUM_NAN if b == bad else 0 for b in range(B)] and np.all(np.isnan(out[bad])) and not np.any(grad[bad])
    keep = np.arange(B) != bad
    assert same_bits([out[keep], grad[keep]], [clean[True][0][keep], clean[True][1][keep]])


# ---- 3. no padding: the resident path's bits ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("name", ["E", "A"])
def test_a_subject_without_padding_gets_the_resident_paths_bits(ctx, name, model):
    cases, k = cc.SETS[name], 2
    M, Nmax = cases[0][1], max(cc.nobs(cases))
    set_subjects(ctx, cases)
    hyper = mc.hyper_of(model, cases)
    P = packed(model, cases, k)
    for prior in (False, True):
        out, grad, status = entry(ctx, model)(P, hyper, prior=prior, want_grad=True, chains_per_subject=k)
        real = mc.unpack(model, grad, cc.nobs(cases), M, k)
        full = [s for s, case in enumerate(cases) if case[0] == Nmax]
        assert full == ([0, 1] if name == "E" else [0])
        for s in full:
            c = hc.build(cases[s])
            ctx.had_set_data(c["x"], c["indx"], c["y"])                       # the resident subject: the set does not care
            r_out, r_grad, r_st = getattr(ctx, mc.RESIDENT[model])(c["pars"][model], hyper, prior=prior, want_grad=True)
            rows = slice(s * k, (s + 1) * k)
            assert r_st.tolist() == [0, 0] and status[rows].tolist() == [0, 0]
            assert np.array_equal(out[rows, 1], r_out[:, 1])                 # the likelihood entry: bit for bit
            if model == "sta":                                               # no prior factor from another factorisation
                assert np.array_equal(out[rows], r_out) and np.array_equal(real[s], r_grad)
            elif not prior:
                assert np.array_equal(out[rows, 0], r_out[:, 0]) and np.array_equal(real[s], r_grad)
            else:                                                            # the prior factors come from another factorisation call
                for j in range(k):
                    check("hcohort_models/sep/%s/vs_resident/%s/chain%d" % (name, hc.case_id(cases[s]), j),
                          logpos=(relerr(out[s * k + j, 0], r_out[j, 0]), VAL_TOL),
                          prior_component_err_on_the_logdet_scale=(prior_component_err_on_the_logdet_scale(out[s * k + j, 2:4], r_out[j, 2:4], Nmax), VAL_TOL),
                          lp_L_vec=(relerr(out[s * k + j, 4], r_out[j, 4]), 1e-12),
                          lp_sigma2=(relerr(out[s * k + j, 5], r_out[j, 5]), 1e-12))


# ---- 4. independence ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_a_subject_alone_gives_the_bits_of_its_rows_in_the_set(ctx, model):
    cases, k = cc.SET_A, 2
    hyper = mc.hyper_of(model, cases)
    ev = entry(ctx, model)
    set_subjects(ctx, cases)
    full = {prior: ev(packed(model, cases, k), hyper, prior=prior, want_grad=True, chains_per_subject=k) for prior in (True, False)}
    for prior in (True, False):
        val = ev(packed(model, cases, k), hyper, prior=prior, want_grad=False, chains_per_subject=k)
        assert val[1] is None and np.array_equal(val[0], full[prior][0]) and np.array_equal(val[2], full[prior][2])
    for s, case in enumerate(cases):
        set_subjects(ctx, [case], Nmax=128)
        for prior in (True, False):
            one = ev(packed(model, [case], k, Nmax=128), hyper, prior=prior, want_grad=True, chains_per_subject=k)
            assert one[2].tolist() == [0, 0] and same_bits(one, [a[s * k:(s + 1) * k] for a in full[prior]]), (case, prior)


@pytest.mark.parametrize("model", MODELS)
def test_a_larger_nmax_stays_within_the_bars(ctx, model):
    evaluate_set(ctx, model, cc.SET_A, 2, "A_Nmax130", Nmax=130)


def test_a_stationary_chain_does_not_see_another_subjects_data(ctx):
    """The stationary rows carry no subject of their own (plain [B, T + 3]): the subject of a row is its position alone.  Subject 1's
    data replaced by subject 4's first 63 observations: subject 1's rows change, every other row keeps its bits."""
    cases, k = cc.SET_A, 2
    hyper = mc.hyper_of("sta", cases)
    P = packed("sta", cases, k)
    set_subjects(ctx, cases)
    base = ctx.hadst_subjects_eval(P, hyper, want_grad=True, chains_per_subject=k)
    subs = [dict(x=c["x"], indx=c["indx"], y=c["y"]) for c in cc.subjects(cases)]
    n = subs[1]["x"].shape[0]
    subs[1] = dict(x=subs[4]["x"][:n], indx=subs[4]["indx"][:n], y=subs[4]["y"][:n])
    assert sorted(np.unique(subs[1]["indx"]).tolist()) == [0, 1]
    ctx.had_set_subjects([c["x"] for c in subs], [c["indx"] for c in subs], [c["y"] for c in subs], M=2)
    got = ctx.hadst_subjects_eval(P, hyper, want_grad=True, chains_per_subject=k)
    keep = np.ones(len(cases) * k, dtype=bool)
    keep[2:4] = False
    assert got[2].tolist() == [0] * 12 and same_bits([a[keep] for a in got], [a[keep] for a in base])
    assert not np.any(got[0][2:4, 1] == base[0][2:4, 1])


# ---- 5. chunking --------------------------------------------------------------------------------------------------------------------------
CHUNK_NOBS = [1024, 513, 1023, 64]


@pytest.mark.parametrize("model", MODELS)
def test_results_do_not_depend_on_the_chunking(ctx, model, monkeypatch):
    """M = 2, Nmax = 1024, with gradients: a chain needs about 26 MB (mc.workspace_per_chain, the formula of INTEGRATION.md), so the
    smallest cap (1 GB) holds 38 chains.  (a) four subjects with 16 chains each: chunks of two whole subjects; (b) the first two
    subjects with 48 chains each: parts of one subject's chains (38 + 10 each).  Under the default cap each is one chunk."""
    M, Nmax = 2, max(CHUNK_NOBS)
    subs, vecs = [], []
    for s, n in enumerate(CHUNK_NOBS):
        x, indx, y, L_vec = hc.subject(n, M, "interleaved", 3400 + s)
        subs.append((x, indx, y))
        vecs.append(hc.parameters(x, M, L_vec)[model])
    hyper = hc.hypers()[model]
    ev = entry(ctx, model)
    for S, cps in ((4, 16), (2, 48)):
        under, whole_n = mc.chunks_under_cap(model, Nmax, M, S, cps, 1.0), mc.chunks_under_cap(model, Nmax, M, S, cps, 96.0)
        print(model, "S", S, "cps", cps, "bytes per chain", mc.workspace_per_chain(model, Nmax, M), "chunks", under, whole_n)
        assert under >= 2 and whole_n == 1
        assert under == (2 if cps == 16 else 4)          # whole subjects / parts of one subject's chains
        ctx.had_set_subjects([s[0] for s in subs[:S]], [s[1] for s in subs[:S]], [s[2] for s in subs[:S]], M=M, Nmax=Nmax)
        # chain j of a subject: chain 0 moved towards chain 1 by j / cps (distinct, smooth, well conditioned)
        rows = [v[0][None] + (np.arange(cps) / cps)[:, None] * (v[1] - v[0])[None] for v in vecs[:S]]
        P = mc.pack(model, rows, CHUNK_NOBS[:S], M, Nmax=Nmax)
        monkeypatch.setenv("NMGP_HAD_BATCH_SLAB_GB", "1")
        chunked = ev(P, hyper, prior=True, want_grad=True, chains_per_subject=cps)
        monkeypatch.delenv("NMGP_HAD_BATCH_SLAB_GB")
        whole = ev(P, hyper, prior=True, want_grad=True, chains_per_subject=cps)
        print("status", sorted(set(chunked[2].tolist())), sorted(set(whole[2].tolist())), "neglog", whole[0][::cps, 0].tolist())
        assert whole[2].tolist() == [0] * (S * cps) and np.all(np.isfinite(whole[0])) and np.all(np.isfinite(whole[1]))
        assert len(set(whole[0][:, 1].tolist())) == S * cps and same_bits(chunked, whole)
        assert no_sign_bit_zeros(whole[1][mc.padded_slots(model, CHUNK_NOBS[:S], M, Nmax, cps)])
    ctx.had_clear_subjects()                             # (gives the prior factors back)


# ---- 6. status ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_a_failing_chain_is_reported_inside_its_own_subject(ctx, model):
    cases, k = cc.SET_C, 3
    assert cases[1] == hc.MINOR
    set_subjects(ctx, cases)
    hyper = mc.hyper_of(model, cases)
    sizes, M = cc.nobs(cases), 3
    ev = entry(ctx, model)

    def vectors(minor):
        return [minor if case == hc.MINOR else hc.build(case)["pars"][model][[0, 1, 0]] for case in cases]

    bad_rows = hc.minor_chains(model)                    # [good, bad, good] on MINOR
    good_rows = bad_rows.copy()
    good_rows[1] = bad_rows[2]
    for prior in (True, False):
        clean = ev(mc.pack(model, vectors(good_rows), sizes, M), hyper, prior=prior, want_grad=True, chains_per_subject=k)
        assert clean[2].tolist() == [0] * 12
        out, grad, status = ev(mc.pack(model, vectors(bad_rows), sizes, M), hyper, prior=prior, want_grad=True, chains_per_subject=k)
        print(model, "prior", prior, "status", status.tolist())
        assert status.tolist() == [0, 0, 0, 0, 3, 0] + [0] * 6
        assert np.all(np.isnan(out[4])) and np.all(grad[4] == 0.0)
        keep = np.arange(12) != 4
        assert same_bits([out[keep], grad[keep]], [clean[0][keep], clean[1][keep]])
        vout, _, vst = ev(mc.pack(model, vectors(bad_rows), sizes, M), hyper, prior=prior, want_grad=False, chains_per_subject=k)
        assert vst.tolist() == status.tolist() and np.array_equal(vout, out, equal_nan=True)


# ---- 7. refusals, each leaving the context usable -------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(ctx):
    from nonstationary_multivariate_gaussian_process_amd import _lib
    cases, M = cc.SET_D, 1
    hyper = {m: mc.hyper_of(m, cases) for m in MODELS}
    P = {m: packed(m, cases, 1) for m in MODELS}
    P_had, hyper_had = cc.pack(cc.chains(cases, 1), cc.nobs(cases), M), hc.build(cases[0])["hyper"]["had"]
    set_subjects(ctx, cases)
    # the three cohort entries interleaved on one set
    base = {m: entry(ctx, m)(P[m], hyper[m], want_grad=True) for m in MODELS}
    had = ctx.had_subjects_eval(P_had, hyper_had, want_grad=True)
    assert all(base[m][2].tolist() == [0, 0, 0] for m in MODELS) and had[2].tolist() == [0, 0, 0]

    def still_good():
        for m in MODELS:
            assert same_bits(entry(ctx, m)(P[m], hyper[m], want_grad=True), base[m])
        assert same_bits(ctx.had_subjects_eval(P_had, hyper_had, want_grad=True), had)

    still_good()
    for m in MODELS:
        with pytest.raises(_lib.NmgpError, match="error -2"):                   # B != S k
            entry(ctx, m)(P[m], hyper[m], want_grad=True, chains_per_subject=2)
        still_good()
        with pytest.raises(_lib.NmgpError, match="error -2"):
            entry(ctx, m)(P[m][:2], hyper[m], want_grad=True)
        still_good()
        with pytest.raises(_lib.NmgpError, match="error -2"):                   # chains_per_subject = 0
            entry(ctx, m)(P[m], hyper[m], want_grad=True, chains_per_subject=0)
        still_good()
    # the resident subject and the set do not see each other
    c = hc.build((63, 2, "blocks"))
    ctx.had_set_data(c["x"], c["indx"], c["y"])
    res = {m: getattr(ctx, mc.RESIDENT[m])(c["pars"][m], c["hyper"][m], want_grad=True) for m in MODELS}
    still_good()
    for m in MODELS:
        assert same_bits(getattr(ctx, mc.RESIDENT[m])(c["pars"][m], c["hyper"][m], want_grad=True), res[m])
    assert (ctx.N, ctx.M) == (63, 2)
    rng = np.random.default_rng(5)
    xs, Y = np.sort(rng.uniform(0.0, 1.0, 40)), rng.standard_normal((40, 2))
    ctx.set_data(xs, Y)
    pc = np.concatenate([-1.5 * np.ones(40), np.tile([0.0, 0.3, 0.0], 40), [-2.0]])
    svc = ctx.logpos_svc(pc, c["hyper"]["had"], want_grad=True)
    still_good()
    assert same_bits(ctx.logpos_svc(pc, c["hyper"]["had"], want_grad=True), svc) and np.all(np.isfinite(svc[0]))
    # without a set: after had_clear_subjects, and on a context that never had one
    ctx.had_clear_subjects()
    fresh = _lib.Context(0)
    try:
        for m in MODELS:
            with pytest.raises(_lib.NmgpError, match="error -3"):
                entry(ctx, m)(P[m], hyper[m], want_grad=True)
            with pytest.raises(_lib.NmgpError, match="error -3"):
                entry(fresh, m)(P[m], hyper[m], want_grad=True)
        set_subjects(fresh, cases)                       # ... and a set needs no resident subject
        for m in MODELS:
            assert same_bits(entry(fresh, m)(P[m], hyper[m], want_grad=True), base[m])
    finally:
        fresh.close()
    set_subjects(ctx, cases)
    still_good()


# ---- 8. poison ------------------------------------------------------------------------------------------------------------------------------
POISON_SNIPPET = r'''
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import hadamard_cohort_cases as cc
import test_gpu_hadamard_cohort_models as t
from nonstationary_multivariate_gaussian_process_amd import _lib
ctx = _lib.Context(0)
for model in t.MODELS:
    for name in ("A", "D", "F", "G", "H"):
        t.evaluate_set(ctx, model, cc.SETS[name], 2, "poison_" + name)      # a fresh (or grown) workspace: poisoned
        t.evaluate_set(ctx, model, cc.SETS[name], 2, "poison_" + name)      # the kept workspace: poisoned again
ctx.close()
print("POISON_OK")
'''


def test_sets_under_poison_meet_the_restatement():
    """NMGP_POISON=1 (read once per process: a fresh child, nothing preloaded) fills fresh buffers and the kept workspace with NaN before
    every call: the y row, ell, sig, Rv, a partial row or a prior column of a padded observation that nobody wrote would show up."""
    env = dict(os.environ)
    env["NMGP_POISON"] = "1"
    env.pop("NMGP_HAD_BATCH_SLAB_GB", None)
    out = subprocess.run([sys.executable, "-c", POISON_SNIPPET % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}],
                         capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0 and "POISON_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


# ---- 9. the drivers -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_cohort_map_follows_the_per_subject_map(ctx, model):
    """5 Adam iterations from chain 0 of every subject of set A: one set per bucket against HadamardSepMAP / HadamardStaMAP subject
    by subject; the achieved distance is recorded (profiles/parity_hadamard_cohort_models.json, hcohort_models/<model>/driver/*)."""
    from nonstationary_multivariate_gaussian_process_amd import _lib, drivers
    cases, iters = cc.SET_A, 5
    subs = cc.subjects(cases)
    keys = {"sep": drivers.SEP_HYPER_KEYS, "sta": drivers.STA_HYPER_KEYS}[model]
    one, cohort = {"sep": (drivers.HadamardSepMAP, drivers.HadamardSepCohortMAP), "sta": (drivers.HadamardStaMAP, drivers.HadamardStaCohortMAP)}[model]
    hyper_pars = dict(zip(keys, [float(v) for v in mc.hyper_of(model, cases)]))
    starts = mc.chains(model, cases, 1)
    ref_hist = np.zeros((iters, len(cases)))
    ref_pars = []
    for s, c in enumerate(subs):
        p, h, alive = one(c["x"], c["indx"], c["y"], hyper_pars, starts[s], ctx=ctx).run(iters)
        assert alive.tolist() == [True]
        ref_hist[:, s] = h[:, 0]
        ref_pars.append(p)
    ctxs = [_lib.Context(0) for _ in range(6)]
    try:
        for w, nb in ((0.0, 6), (0.5, 3)):
            m = cohort([(c["x"], c["indx"], c["y"]) for c in subs], hyper_pars, starts, max_flop_waste=w, ctxs=ctxs[:nb])
            assert len(m.buckets) == nb
            pars, hist, alive = m.run(iters)
            m.close()                                    # (contexts of the caller's: the sets are dropped, the contexts stay open)
            assert hist.shape == (iters, 6) and alive.tolist() == [True] * 6 and [p.shape for p in pars] == [v.shape for v in starts]
            per_step = np.max(np.abs(hist - ref_hist) / np.abs(ref_hist), axis=1)
            print(model, "max_flop_waste", w, "relative error of the history per step", per_step.tolist())
            record_parity("hcohort_models/%s/driver/max_flop_waste_%g" % (model, w), hist=(float(per_step.max()), VAL_TOL),
                          pars=float(max(relerr(p, q) for p, q in zip(pars, ref_pars))))
            assert per_step.max() < VAL_TOL, (w, per_step.tolist())
    finally:
        for c in ctxs:
            c.close()
