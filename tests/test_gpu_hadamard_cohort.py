"""GPU half of the Hadamard cohort tests: nmgp_had_set_subjects / nmgp_had_subjects_eval (ragged subjects padded to Nmax with decoupled
unit observations) against the NumPy restatement hadamard_cases.ref_logpos("had", ...) on each subject ALONE, at the sets of
tests/hadamard_cohort_cases.py; tests/test_hadamard_cohort_cpu.py checks the new subjects' preconditions and the padded formulation.

Bars: those of tests/test_gpu_hadamard_sweep.py for the model "had" (its eval_errors): without priors likelihood 1e-10 and gradient
1e-8; with priors 1e-6 / 1e-9 / 1e-5; prior components 1e-6 on the log-det scale; the inverse-gamma entry 1e-12; the gradient block by
block too, without the priors at hadamard_cases.block_bar of the subject in its set (min(1e-8, max(100 d_cpu, N_s cond(S) eps)), both
terms from the CPU half), the prior part g(prior) - g(no prior) at 1e-5.  Sets F - H (M = 4, 6, 7) run everything sets A - E run; set
I (Nmax = 1030) with one chain per subject against the restatement and in "padding is inert".  Padding inert, a
subject alone against its rows of the set, value-only against value + gradient, chunked against unchunked, and a subject without
padding against the resident path's likelihood: bit for bit.  Driver: 1e-6 relative on the log-posterior history, the standing bar
between two evaluation paths."""
import os
import subprocess
import sys

import numpy as np
import pytest

import hadamard_cases as hc
import hadamard_cohort_cases as cc
from conftest import ROOT, prior_component_err_on_the_logdet_scale, record_parity, relerr
from test_gpu_hadamard_sweep import VAL_TOL, check, eval_errors, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from nonstationary_multivariate_gaussian_process_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def set_subjects(ctx, cases, Nmax=None):
    subs = cc.subjects(cases)
    ctx.had_set_subjects([c["x"] for c in subs], [c["indx"] for c in subs], [c["y"] for c in subs], M=cases[0][1], Nmax=Nmax)


def packed(cases, k, Nmax=None, fill=0.0):
    return cc.pack(cc.chains(cases, k), cc.nobs(cases), cases[0][1], Nmax=Nmax, fill=fill)


def hyper_of(cases):
    return hc.build(cases[0])["hyper"]["had"]


def unpack(P, cases, k):
    from nonstationary_multivariate_gaussian_process_amd import hadamard
    return hadamard.cohort_unpack(P, cc.nobs(cases), cases[0][1], chains_per_subject=k)


def meets_the_restatement(out, grad, status, cases, k, prior, tag, plain):
    """every chain's tuple and the real slots of its gradient against the restatement on the subject alone, the gradient block by
    block too (`plain`: the entry's gradient without the priors, which the prior part is taken against); padded slots +0.0"""
    S, M = len(cases), cases[0][1]
    Nmax = (grad.shape[1] - 1) // (1 + hc.build(cases[0])["T"])
    assert status.tolist() == [0] * (S * k) and out.shape == (S * k, 5)
    pads = cc.padded_slots(cc.nobs(cases), M, Nmax, k)
    assert np.all(grad[pads] == 0.0) and not np.any(np.signbit(grad[pads]))
    real, real_plain = unpack(grad, cases, k), unpack(plain, cases, k)
    for s, case in enumerate(cases):
        for j in range(k):
            ref_out, ref_grad = cc.reference(case, j, prior)
            check("hcohort/%s/k%d/prior%d/%s/chain%d" % (tag, k, prior, hc.case_id(case), j),
                  **eval_errors("had", out[s * k + j], real[s][j], ref_out, ref_grad, prior, case[0], M, hc.block_bar("had", case, Nmax),
                                without=(real_plain[s][j], cc.reference(case, j, False)[1])))


def evaluate_set(ctx, cases, k, tag, Nmax=None):
    set_subjects(ctx, cases, Nmax)
    P = packed(cases, k, Nmax)
    res = {prior: ctx.had_subjects_eval(P, hyper_of(cases), prior=prior, want_grad=True, chains_per_subject=k) for prior in (True, False)}
    assert np.array_equal(res[False][0][:, 0], -res[False][0][:, 1])
    for prior in (True, False):
        meets_the_restatement(*res[prior], cases, k, prior, tag, res[False][1])


# ---- 1. against the restatement -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("name", sorted(cc.SETS))
def test_every_chain_of_the_set_meets_the_restatement_on_its_subject_alone(ctx, name, k):
    evaluate_set(ctx, cc.SETS[name], k, name)


def test_set_I_meets_the_restatement_beyond_one_panel_and_one_trace_pass(ctx):
    """Nmax = 1030, one chain per subject: N_s = 1030 and 1025 take k_hadc_trace's second pass and 513 and 640 do not, the factorisation
    runs two 512-column panels (the identity-padded tail of the short subjects in the second), 2 Nmax + 2 = 2062 riding rows."""
    evaluate_set(ctx, cc.SET_I, 1, "I")


# ---- 2. padding is inert ----------------------------------------------------------------------------------------------------------------
def test_padding_is_inert(ctx):
    padding_is_inert(ctx, cc.SET_A, 2)


def test_padding_is_inert_in_set_I(ctx):
    padding_is_inert(ctx, cc.SET_I, 1)


def padding_is_inert(ctx, cases, k):
    M, B = cases[0][1], len(cases) * k
    sizes, Nmax = cc.nobs(cases), max(cc.nobs(cases))
    subs = cc.subjects(cases)
    x, y, indx = np.zeros((len(cases), Nmax)), np.zeros((len(cases), Nmax)), np.zeros((len(cases), Nmax), dtype=np.int32)
    for s, c in enumerate(subs):
        x[s, :sizes[s]], y[s, :sizes[s]], indx[s, :sizes[s]] = c["x"], c["y"], c["indx"]
    ctx.had_set_subjects_padded(x, indx, y, sizes, M)
    hyper = hyper_of(cases)
    clean = {prior: ctx.had_subjects_eval(packed(cases, k), hyper, prior=prior, want_grad=True, chains_per_subject=k) for prior in (True, False)}
    for s, n in enumerate(sizes):                       # poison in every padded slot of the data
        x[s, n:], y[s, n:] = np.nan, np.nan
        indx[s, n:] = np.where(np.arange(Nmax - n) % 2 == 0, -1, 99)
    ctx.had_set_subjects_padded(x, indx, y, sizes, M)
    pads = cc.padded_slots(sizes, M, Nmax, k)
    assert pads.sum() > 0
    for fill in (np.nan, 1e300):
        P = packed(cases, k, fill=fill)
        assert np.all(P[pads] == fill) if np.isfinite(fill) else np.all(np.isnan(P[pads]))
        for prior in (True, False):
            got = ctx.had_subjects_eval(P, hyper, prior=prior, want_grad=True, chains_per_subject=k)
            assert got[2].tolist() == [0] * B and same_bits(got, clean[prior]), (fill, prior)
            assert np.all(got[1][pads] == 0.0) and not np.any(np.signbit(got[1][pads]))
            val = ctx.had_subjects_eval(P, hyper, prior=prior, want_grad=False, chains_per_subject=k)
            assert val[1] is None and np.array_equal(val[0], clean[prior][0]) and val[2].tolist() == got[2].tolist()
    # a NaN in a REAL slot is reported for that chain alone
    P = packed(cases, k, fill=np.nan)
    bad = 2 * k - 1                                     # the last chain of subject 1 (set A: 63 observations): tilde_l[1]
    assert sizes[1] < Nmax and (k, bad) in ((2, 3), (1, 1))
    P[bad, 1] = np.nan
    out, grad, status = ctx.had_subjects_eval(P, hyper, prior=True, want_grad=True, chains_per_subject=k)
    from nonstationary_multivariate_gaussian_process_amd import _lib
    assert status.tolist() == [_lib.NUM_NAN if b == bad else 0 for b in range(B)] and np.all(np.isnan(out[bad])) and not np.any(grad[bad])
    keep = np.arange(B) != bad
    assert same_bits([out[keep], grad[keep]], [clean[True][0][keep], clean[True][1][keep]])


# ---- 3. no padding: the resident path's likelihood, bit for bit --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["E", "A"])
def test_a_subject_without_padding_gets_the_resident_paths_bits(ctx, name):
    cases, k = cc.SETS[name], 2
    Nmax = max(cc.nobs(cases))
    set_subjects(ctx, cases)
    hyper = hyper_of(cases)
    P = packed(cases, k)
    for prior in (False, True):
        out, grad, status = ctx.had_subjects_eval(P, hyper, prior=prior, want_grad=True, chains_per_subject=k)
        real = unpack(grad, cases, k)
        full = [s for s, case in enumerate(cases) if case[0] == Nmax]
        assert full == ([0, 1] if name == "E" else [0])
        for s in full:
            c = hc.build(cases[s])
            ctx.had_set_data(c["x"], c["indx"], c["y"])                       # the resident subject: the set does not care
            r_out, r_grad, r_st = ctx.had_batch_eval(c["pars"]["had"], hyper, prior=prior, want_grad=True)
            rows = slice(s * k, (s + 1) * k)
            assert r_st.tolist() == [0, 0] and status[rows].tolist() == [0, 0]
            assert np.array_equal(out[rows, 1], r_out[:, 1])                 # the likelihood entry: bit for bit
            if not prior:
                assert np.array_equal(out[rows, 0], r_out[:, 0]) and np.array_equal(real[s], r_grad)
            else:                                                            # the prior factor comes from another factorisation call
                for j in range(k):
                    check("hcohort/%s/vs_resident/%s/chain%d" % (name, hc.case_id(cases[s]), j),
                          logpos=(relerr(out[s * k + j, 0], r_out[j, 0]), VAL_TOL),
                          prior_component_err_on_the_logdet_scale=(prior_component_err_on_the_logdet_scale(out[s * k + j, 2:4], r_out[j, 2:4], Nmax), VAL_TOL),
                          lp_sigma2=(relerr(out[s * k + j, 4], r_out[j, 4]), 1e-12))


# ---- 4. independence ------------------------------------------------------------------------------------------------------------------------
def test_a_subject_alone_gives_the_bits_of_its_rows_in_the_set(ctx):
    cases, k = cc.SET_A, 2
    hyper = hyper_of(cases)
    set_subjects(ctx, cases)
    full = {prior: ctx.had_subjects_eval(packed(cases, k), hyper, prior=prior, want_grad=True, chains_per_subject=k) for prior in (True, False)}
    for prior in (True, False):
        val = ctx.had_subjects_eval(packed(cases, k), hyper, prior=prior, want_grad=False, chains_per_subject=k)
        assert val[1] is None and np.array_equal(val[0], full[prior][0]) and np.array_equal(val[2], full[prior][2])
    for s, case in enumerate(cases):
        set_subjects(ctx, [case], Nmax=128)
        for prior in (True, False):
            one = ctx.had_subjects_eval(packed([case], k, Nmax=128), hyper, prior=prior, want_grad=True, chains_per_subject=k)
            assert one[2].tolist() == [0, 0] and same_bits(one, [a[s * k:(s + 1) * k] for a in full[prior]]), (case, prior)


def test_a_larger_nmax_stays_within_the_bars(ctx):
    evaluate_set(ctx, cc.SET_A, 2, "A_Nmax130", Nmax=130)


# ---- 5. chunking --------------------------------------------------------------------------------------------------------------------------
CHUNK_NMAX, CHUNK_NOBS = 3400, [3400, 1700, 3399, 64]


def chunks_under_cap(Nmax, B, cap_gb):
    """Chunks of a value + gradient call of B chains: (2 Nmax + 2) ld + Nmax^2 doubles per chain, ld = the 2 Nmax + 2
    rows rounded up to 16."""
    ld = (2 * Nmax + 2 + 15) // 16 * 16
    per_chunk = min(B, int(cap_gb * 1e9 // (8.0 * (ld * Nmax + Nmax * Nmax))))
    assert per_chunk >= 1
    return -(-B // per_chunk)


def test_results_do_not_depend_on_the_chunking(ctx, monkeypatch):
    """M = 2, Nmax = 3400 (next to the largest allowed order), four subjects with one chain each, with gradients: a chain needs about
    0.29 GB, so under the smallest cap (1 GB) the call runs as chunks of 3 + 1 subjects, under the default cap as one."""
    assert chunks_under_cap(CHUNK_NMAX, 4, 1.0) == 2 and chunks_under_cap(CHUNK_NMAX, 4, 1.0 / 1.05) == 2 and chunks_under_cap(CHUNK_NMAX, 4, 96.0) == 1
    subs, vecs = [], []
    for s, n in enumerate(CHUNK_NOBS):
        x, indx, y, L_vec = hc.subject(n, 2, "interleaved", 3400 + s)
        subs.append((x, indx, y))
        vecs.append(hc.parameters(x, 2, L_vec)["had"][:1])
    ctx.had_set_subjects([s[0] for s in subs], [s[1] for s in subs], [s[2] for s in subs], M=2)
    P = cc.pack(vecs, CHUNK_NOBS, 2)
    hyper = hc.hypers()["had"]
    monkeypatch.setenv("NMGP_HAD_BATCH_SLAB_GB", "1")
    chunked = ctx.had_subjects_eval(P, hyper, prior=True, want_grad=True)
    monkeypatch.delenv("NMGP_HAD_BATCH_SLAB_GB")
    whole = ctx.had_subjects_eval(P, hyper, prior=True, want_grad=True)
    print("status", chunked[2].tolist(), whole[2].tolist(), "neglog", whole[0][:, 0].tolist())
    assert whole[2].tolist() == [0, 0, 0, 0] and np.all(np.isfinite(whole[0])) and np.all(np.isfinite(whole[1]))
    assert len(set(whole[0][:, 1].tolist())) == 4 and same_bits(chunked, whole)
    pads = cc.padded_slots(CHUNK_NOBS, 2, CHUNK_NMAX)
    assert np.all(whole[1][pads] == 0.0) and not np.any(np.signbit(whole[1][pads]))
    ctx.had_clear_subjects()                             # (gives the 3400-order prior factors back)


# ---- 6. status ----------------------------------------------------------------------------------------------------------------------------
def test_a_failing_chain_is_reported_inside_its_own_subject(ctx):
    cases, k = cc.SET_C, 3
    assert cases[1] == hc.MINOR
    set_subjects(ctx, cases)
    hyper = hyper_of(cases)
    sizes, M = cc.nobs(cases), 3

    def vectors(minor):
        return [minor if case == hc.MINOR else hc.build(case)["pars"]["had"][[0, 1, 0]] for case in cases]

    bad_rows = hc.minor_chains("had")                    # [good, bad, good] on MINOR
    good_rows = bad_rows.copy()
    good_rows[1] = bad_rows[2]
    for prior in (True, False):
        clean = ctx.had_subjects_eval(cc.pack(vectors(good_rows), sizes, M), hyper, prior=prior, want_grad=True, chains_per_subject=k)
        assert clean[2].tolist() == [0] * 12
        out, grad, status = ctx.had_subjects_eval(cc.pack(vectors(bad_rows), sizes, M), hyper, prior=prior, want_grad=True, chains_per_subject=k)
        print("prior", prior, "status", status.tolist())
        assert status.tolist() == [0, 0, 0, 0, 3, 0] + [0] * 6
        assert np.all(np.isnan(out[4])) and np.all(grad[4] == 0.0)
        keep = np.arange(12) != 4
        assert same_bits([out[keep], grad[keep]], [clean[0][keep], clean[1][keep]])
        vout, _, vst = ctx.had_subjects_eval(cc.pack(vectors(bad_rows), sizes, M), hyper, prior=prior, want_grad=False, chains_per_subject=k)
        assert vst.tolist() == status.tolist() and np.array_equal(vout, out, equal_nan=True)


# ---- 7. refusals, each leaving the context usable -------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(ctx):
    from nonstationary_multivariate_gaussian_process_amd import _lib
    cases, M = cc.SET_D, 1
    hyper = hyper_of(cases)
    sizes, Nmax = cc.nobs(cases), 70
    P = packed(cases, 1)
    set_subjects(ctx, cases)
    base = ctx.had_subjects_eval(P, hyper, want_grad=True)
    assert base[2].tolist() == [0, 0, 0]

    def still_good():
        assert same_bits(ctx.had_subjects_eval(P, hyper, want_grad=True), base)

    x, y, indx = np.zeros((3, Nmax)), np.zeros((3, Nmax)), np.zeros((3, Nmax), dtype=np.int32)
    for s, c in enumerate(cc.subjects(cases)):
        x[s, :sizes[s]], y[s, :sizes[s]], indx[s, :sizes[s]] = c["x"], c["y"], c["indx"]
    two = np.where(np.arange(Nmax) % 2 == 0, 0, 1).astype(np.int32)[None].repeat(3, axis=0)
    lone = two.copy()
    lone[1, :sizes[1]] = 0                               # subject 1 misses label 1 among its real observations (its pads hold it)
    refused = [("nobs = 0", x, indx, y, [1, 0, 70], 1), ("nobs > Nmax", x, indx, y, [1, 2, 71], 1),
               ("nobs < M", x, two, y, [1, 2, 70], 2), ("a missing label", x, lone, y, [2, 2, 70], 2),
               ("M = 9", x, indx, y, sizes, 9), ("a label outside [0, M)", x, two, y, [2, 2, 70], 1),
               ("Nmax = 3501", np.zeros((1, 3501)), np.zeros((1, 3501), dtype=np.int32), np.zeros((1, 3501)), [3501], 1)]
    for what, xx, ii, yy, nn, mm in refused:
        with pytest.raises(_lib.NmgpError, match="error -2"):
            ctx.had_set_subjects_padded(xx, ii, yy, nn, mm)
        still_good()
    with pytest.raises(_lib.NmgpError, match="error -2"):                   # B != S k
        ctx.had_subjects_eval(P, hyper, want_grad=True, chains_per_subject=2)
    still_good()
    with pytest.raises(_lib.NmgpError, match="error -2"):
        ctx.had_subjects_eval(P[:2], hyper, want_grad=True)
    still_good()
    # the resident subject and the set do not see each other
    c = hc.build((63, 2, "blocks"))
    ctx.had_set_data(c["x"], c["indx"], c["y"])
    res = ctx.had_batch_eval(c["pars"]["had"], c["hyper"]["had"], want_grad=True)
    still_good()
    assert same_bits(ctx.had_batch_eval(c["pars"]["had"], c["hyper"]["had"], want_grad=True), res) and (ctx.N, ctx.M) == (63, 2)
    rng = np.random.default_rng(5)
    xs, Y = np.sort(rng.uniform(0.0, 1.0, 40)), rng.standard_normal((40, 2))
    ctx.set_data(xs, Y)
    pc = np.concatenate([-1.5 * np.ones(40), np.tile([0.0, 0.3, 0.0], 40), [-2.0]])
    svc = ctx.logpos_svc(pc, c["hyper"]["had"], want_grad=True)
    still_good()
    assert same_bits(ctx.logpos_svc(pc, c["hyper"]["had"], want_grad=True), svc) and np.all(np.isfinite(svc[0]))
    # without a set: after had_clear_subjects, and on a context that never had one
    ctx.had_clear_subjects()
    with pytest.raises(_lib.NmgpError, match="error -3"):
        ctx.had_subjects_eval(P, hyper, want_grad=True)
    fresh = _lib.Context(0)
    try:
        with pytest.raises(_lib.NmgpError, match="error -3"):
            fresh.had_subjects_eval(P, hyper, want_grad=True)
        set_subjects(fresh, cases)                       # ... and a set needs no resident subject
        assert same_bits(fresh.had_subjects_eval(P, hyper, want_grad=True), base)
    finally:
        fresh.close()
    set_subjects(ctx, cases)
    still_good()


# ---- 8. poison ------------------------------------------------------------------------------------------------------------------------------
POISON_SNIPPET = r'''
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import hadamard_cohort_cases as cc
import test_gpu_hadamard_cohort as t
from nonstationary_multivariate_gaussian_process_amd import _lib
ctx = _lib.Context(0)
for name in ("A", "D", "F", "G", "H"):
    t.evaluate_set(ctx, cc.SETS[name], 2, "poison_" + name)      # a fresh (or grown) workspace: poisoned
    t.evaluate_set(ctx, cc.SETS[name], 2, "poison_" + name)      # the kept workspace: poisoned again
ctx.close()
print("POISON_OK")
'''


def test_sets_under_poison_meet_the_restatement():
    """NMGP_POISON=1 (read once per process: a fresh child, nothing preloaded) fills fresh buffers and the kept workspace with NaN before
    every call: the y row, ell or Rv of a padded observation that nobody wrote would show up as a NaN."""
    env = dict(os.environ)
    env["NMGP_POISON"] = "1"
    env.pop("NMGP_HAD_BATCH_SLAB_GB", None)
    out = subprocess.run([sys.executable, "-c", POISON_SNIPPET % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}],
                         capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0 and "POISON_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


# ---- 9. the driver --------------------------------------------------------------------------------------------------------------------------
def test_cohort_map_follows_the_per_subject_map(ctx):
    """5 Adam iterations from chain 0 of every subject of set A: one set per bucket against HadamardMAP subject by subject.  Measured on
    the MI355X (profiles/parity_hadamard_cohort.json, hcohort/driver/*): the history agrees exactly at max_flop_waste = 0 and within
    2.2e-14 relative at 0.5 over the five steps."""
    from nonstationary_multivariate_gaussian_process_amd import _lib, drivers
    cases, iters = cc.SET_A, 5
    subs = cc.subjects(cases)
    hyper_pars = dict(zip(drivers.SVC_HYPER_KEYS, [float(v) for v in hyper_of(cases)]))
    starts = cc.chains(cases, 1)
    ref_hist = np.zeros((iters, len(cases)))
    ref_pars = []
    for s, c in enumerate(subs):
        p, h, alive = drivers.HadamardMAP(c["x"], c["indx"], c["y"], hyper_pars, starts[s], ctx=ctx).run(iters)
        assert alive.tolist() == [True]
        ref_hist[:, s] = h[:, 0]
        ref_pars.append(p)
    ctxs = [_lib.Context(0) for _ in range(6)]
    try:
        for w, nb in ((0.0, 6), (0.5, 3)):
            m = drivers.HadamardCohortMAP([(c["x"], c["indx"], c["y"]) for c in subs], hyper_pars, starts, max_flop_waste=w, ctxs=ctxs[:nb])
            assert len(m.buckets) == nb
            pars, hist, alive = m.run(iters)
            m.close()                                    # (contexts of the caller's: the sets are dropped, the contexts stay open)
            assert hist.shape == (iters, 6) and alive.tolist() == [True] * 6 and [p.shape for p in pars] == [v.shape for v in starts]
            per_step = np.max(np.abs(hist - ref_hist) / np.abs(ref_hist), axis=1)
            print("max_flop_waste", w, "relative error of the history per step", per_step.tolist())
            record_parity("hcohort/driver/max_flop_waste_%g" % w, hist=(float(per_step.max()), VAL_TOL),
                          pars=float(max(relerr(p, q) for p, q in zip(pars, ref_pars))))
            assert per_step.max() < VAL_TOL, (w, per_step.tolist())
    finally:
        for c in ctxs:
            c.close()
