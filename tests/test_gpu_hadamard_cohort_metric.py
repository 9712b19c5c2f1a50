"""GPU half of the prior-factor metric of the Hadamard cohort: nmgp_had_subjects_prior_apply, nmgp_had_subjects_traj_* under mass kind 2
(k_prior_trmm_coh, csrc/nmgp_metric.hip) and the cohort HMC drivers with mass="prior", on the ragged sets P, Q, R, E of
tests/hadamard_cohort_metric_cases.py (CPU half: tests/test_hadamard_cohort_metric_cpu.py, which measures the bars).

1. prior_apply, both orientations and models, k = 1 and 2: per block against the np.longdouble products within C.BAR["apply"], +0.0
   in every padded output slot; once under the golden ill-conditioned hyper-parameters, whole vector within metric_cases.ILL_BAR.
2. Bit for bit (prior_apply, trajectories of 1 and 3 steps): every subject alone in a set of one (at the set's Nmax, as the evaluation's
   own independence test), k = 1 against chain 0 of k = 2, Nmax + 37, a slab cap that splits the set (whole subjects / parts of one
   subject's chains), NaN / 1e300 / labels -1 and 99 in every padded slot, NMGP_POISON=1 in a child process.
3. One step: q1 - q0 and u1 per block against the longdouble reference fed with the entry's gradients; two steps as table D2 of the
   metric sweep; kin1 within math.fsum's summation bound.
4. Meaning: the device against the dense-mass leapfrog M^-1 = L_blk L_blk^T, p0 = L_blk^-T z in longdouble, in q1 - q0 and H1 - H0.
5. State and switching: kind 2 -> 0 -> 2, commit with rejections, a chain bad at the start, a chain pushed to a non-finite position,
   the refusals.
6. Drivers: the resident loop against the host loop, 3 iterations x 3 steps, sets P and Q, max_flop_waste 0 and 0.5.
7. The metric does its job (C.JOB_EPS, C.JOB_STEPS; see C.JOB_DIAGONAL for the subject whose L_blk is diagonal)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import hadamard_cases as hc
import hadamard_cohort_hmc_cases as hh
import hadamard_cohort_metric_cases as C
import metric_cases as mc
from conftest import ROOT, record_parity

pytestmark = pytest.mark.gpu
LD = mc.LD
NAMES = ("P", "Q", "R", "E")
STEPS = (1, 3)
E_SHAPE, E_STATE, E_UNSUPPORTED = -2, -3, -4          # include/nmgp.h


@pytest.fixture(scope="module")
def ctx():
    from nonstationary_multivariate_gaussian_process_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def evaluate(ctx, model, P, k, hyper=None):
    return getattr(ctx, hh.ENTRY[model])(P, C.HYPER[model] if hyper is None else hyper, True, True, k)


def subject_eval(ctx, model, name, k, s):
    """rows [k, P_s] of subject s -> (U [k], grad [k, P_s]) from the model's *_subjects_eval on the set that is on the context (the
    other subjects' rows at their start)"""
    base = C.chains(model, name, k)

    def f(q):
        rows = [np.asarray(q, dtype=np.float64) if j == s else b for j, b in enumerate(base)]
        out, g, status = evaluate(ctx, model, C.pack(model, name, rows), k)
        assert status.tolist() == [0] * len(status)
        return out[s * k:(s + 1) * k, 0], C.unpack(model, name, g, k)[s]

    return f


def traj(ctx, model, P, k, eps, nsteps, z, mass="prior", hyper=None):
    """begin at P, the mass, one trajectory: (out, status), (q1, u1, kin1, U1, failed)"""
    start = ctx.had_subjects_traj_begin(model, P, C.HYPER[model] if hyper is None else hyper, True, k)
    if mass == "prior":
        ctx.had_subjects_traj_set_mass(prior=True)
    else:
        ctx.had_subjects_traj_set_mass(mass)
    return start, ctx.had_subjects_traj(eps, nsteps, z, want_p1=True, want_kin=True)


def collect(ctx, model, name, k, Nmax=None, fill=0.0, only=None, padded_set=None):
    """everything test 2 compares, per subject in the reference layout: both products of C.vectors and, for 1 and 3 steps, q1, u1,
    kin1, U1, failed.  only: the subject alone in a set of one; padded_set: (x, indx, y) [S, Nmax] with their own padding"""
    sel = range(len(C.sizes(name))) if only is None else [only]
    if padded_set is not None:
        ctx.had_set_subjects_padded(*padded_set, C.sizes(name), C.n_labels(name))
    else:
        C.set_subjects(ctx, name, Nmax=Nmax, only=only)
    pk = lambda rows: C.pack(model, name, [rows[s] for s in sel], Nmax=Nmax, fill=fill, only=only)
    un = lambda A: C.unpack(model, name, A, k, only=only)
    V, Q = pk(C.vectors(model, name, k)), pk(C.chains(model, name, k))
    eps = C.eps_of(name)[list(sel)]
    res = {"apply0": un(ctx.had_subjects_prior_apply(model, C.HYPER[model], V, False, k)),
           "apply1": un(ctx.had_subjects_prior_apply(model, C.HYPER[model], V, True, k))}
    for nsteps in STEPS:
        _, (q1, u1, kin1, U1, failed) = traj(ctx, model, Q, k, eps, nsteps, V)
        assert not failed.any()
        res["q1_%d" % nsteps], res["u1_%d" % nsteps] = un(q1), un(u1)
        res["kin1_%d" % nsteps], res["U1_%d" % nsteps] = kin1.reshape(len(sel), k), U1.reshape(len(sel), k)
        if fill != 0.0:                              # padded slots of q1 come back as uploaded, those of u1 are +0.0
            pads = C.pads(model, name, k, Nmax=Nmax)
            assert np.array_equal(hh.bits(q1)[pads], hh.bits(Q)[pads]) and np.all(u1[pads] == 0.0) and not np.any(np.signbit(u1[pads]))
    ctx.had_subjects_traj_end()
    return res


def same(a, b, sa, sb, rows=slice(None), what=""):
    ok = True
    for key in a:
        x, y = np.asarray(a[key][sa])[rows], np.asarray(b[key][sb])[rows]
        same_bits = np.array_equal(hh.bits(x), hh.bits(y))
        if not same_bits:
            with np.errstate(invalid="ignore"):
                print(what, key, "subject", sa, "max |difference|", float(np.nanmax(np.abs(x - y))), "NaN", int(np.isnan(x).sum()))
        ok = ok and same_bits
    return ok


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("model", C.MODELS)
def test_prior_apply_against_the_longdouble_products(ctx, model, name):
    C.set_subjects(ctx, name)
    S, worst = len(C.sizes(name)), (0.0, "")
    for k in (1, 2):
        v = C.vectors(model, name, k)
        V = C.pack(model, name, v)
        pads = C.pads(model, name, k)
        for trans in (False, True):
            out = ctx.had_subjects_prior_apply(model, C.HYPER[model], V, trans, k)
            err, where = C.worst_block(model, name, C.unpack(model, name, out, k), [C.apply_rows(model, name, s, v[s], trans) for s in range(S)])
            print(model, name, "k", k, "trans", trans, "worst block error", err, where, "bar", C.BAR["apply"])
            worst = max(worst, (err, where))
            assert np.all(out[pads] == 0.0) and not np.any(np.signbit(out[pads]))
    record_parity("hcohort_metric/%s/%s/prior_apply" % (model, name), block=(worst[0], C.BAR["apply"]))
    assert worst[0] <= C.BAR["apply"], worst


@pytest.mark.parametrize("model", C.MODELS)
def test_prior_apply_under_the_golden_hyper_parameters(ctx, model):
    """kappa up to ~1e8: the factor itself is only defined to kappa eps, so the whole vector is held to metric_cases.ILL_BAR against
    NumPy's float64 factors, as tests/test_hmc_metric.py does for the resident metric"""
    name, k = "P", 2
    C.set_subjects(ctx, name)
    v = C.vectors(model, name, k)
    worst = 0.0
    for trans in (False, True):
        out = C.unpack(model, name, ctx.had_subjects_prior_apply(model, C.HYPER_ILL[model], C.pack(model, name, v), trans, k), k)
        for s in range(len(v)):
            ref = np.asarray(C.apply_rows(model, name, s, v[s], trans, "f64", ill=True), dtype=np.float64)
            err = float(np.linalg.norm(out[s] - ref) / np.linalg.norm(ref))
            print(model, "trans", trans, "subject", s, "whole-vector error", err)
            worst = max(worst, err)
    record_parity("hcohort_metric/%s/P/prior_apply_ill" % model, whole=(worst, mc.ILL_BAR))
    assert worst < mc.ILL_BAR


# ---- 2 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", C.MODELS)
def test_a_chain_depends_on_nothing_else(ctx, model):
    name = "P"
    sz = C.sizes(name)
    Nmax, S = max(sz), len(sz)
    full = collect(ctx, model, name, 2)
    ok = []
    for who in range(S):                               # every subject alone in a set of one at the set's Nmax (N_s = 129: three k tiles)
        ok.append(same(full, collect(ctx, model, name, 2, Nmax=Nmax, only=who), who, 0, what="alone"))
    one = collect(ctx, model, name, 1)
    ok += [same(full, one, s, s, slice(0, 1), what="k=1") for s in range(S)]
    wide = collect(ctx, model, name, 2, Nmax=Nmax + C.WIDE)
    ok += [same(full, wide, s, s, what="Nmax+37") for s in range(S)]
    assert all(ok), ok


@pytest.mark.parametrize("name", ("P", "Q"))
@pytest.mark.parametrize("model", C.MODELS)
def test_poisoned_pads_are_never_read(ctx, model, name):
    """NaN, 1e300 and the labels -1 / 99 in every padded slot of pars, p0, in and of the set's x / indx / y"""
    sz, k = C.sizes(name), 2
    Nmax, S = max(sz) + 5, len(sz)
    clean = collect(ctx, model, name, k, Nmax=Nmax)
    subs = C.subjects(name)
    for fill, label in ((np.nan, -1), (1e300, 99)):
        x2, y2 = np.full((S, Nmax), fill), np.full((S, Nmax), fill)
        i2 = np.full((S, Nmax), label, dtype=np.int32)
        for s, c in enumerate(subs):
            x2[s, :sz[s]], y2[s, :sz[s]], i2[s, :sz[s]] = c["x"], c["y"], c["indx"]
        pads = C.pads(model, name, k, Nmax=Nmax)
        V = C.pack(model, name, C.vectors(model, name, k), Nmax=Nmax, fill=fill)
        assert pads.any() and not np.any(np.isfinite(V[pads]) & (np.abs(V[pads]) < 1e299))
        got = collect(ctx, model, name, k, Nmax=Nmax, fill=fill, padded_set=(x2, i2, y2))
        out = ctx.had_subjects_prior_apply(model, C.HYPER[model], V, True, k)
        assert np.all(out[pads] == 0.0) and not np.any(np.signbit(out[pads]))
        assert all([same(clean, got, s, s, what="fill %r" % fill) for s in range(S)])
    ctx.had_clear_subjects()


def interpolated(model, name, cps, sel):
    """cps chains per subject between its chains 0 and 1, and as many momenta"""
    rows = [v[0][None] + (np.arange(cps) / cps)[:, None] * (v[1] - v[0])[None] for v in C.chains(model, name, 2)]
    z = [np.random.default_rng(C.P_SEED + s).standard_normal(r.shape) for s, r in enumerate(rows)]
    return [rows[s] for s in sel], [z[s] for s in sel]


@pytest.mark.parametrize("model", C.MODELS)
def test_trajectories_do_not_depend_on_the_chunking(ctx, model, monkeypatch):
    """Set R (Nmax = 193) under the smallest cap, 1 GB: (S, cps) = (3, 700) runs as chunks of whole subjects, (1, 2400) -- its largest
    subject alone -- as parts of one subject's chains; one chunk each under the default cap.  One and three steps."""
    name = "R"
    M, Nmax = C.n_labels(name), max(C.sizes(name))
    for sel, cps in (([0, 1, 2], 700), ([2], 2400)):
        S = len(sel)
        under, whole_n = hh.chunks_under_cap(model, Nmax, M, S, cps, 1.0), hh.chunks_under_cap(model, Nmax, M, S, cps, 96.0)
        print(model, "S", S, "cps", cps, "bytes per chain", hh.workspace_per_chain(model, Nmax, M), "chunks", under, whole_n)
        assert under >= 2 and whole_n == 1
        subs = [C.subjects(name)[s] for s in sel]
        ctx.had_set_subjects([c["x"] for c in subs], [c["indx"] for c in subs], [c["y"] for c in subs], M=M, Nmax=Nmax)
        rows, z = interpolated(model, name, cps, sel)
        sz = [C.sizes(name)[s] for s in sel]
        Q, Z = hh.pack(model, rows, sz, M, Nmax=Nmax), hh.pack(model, z, sz, M, Nmax=Nmax)
        eps = C.eps_of(name)[sel]
        for nsteps in STEPS:
            monkeypatch.setenv("NMGP_HAD_BATCH_SLAB_GB", "1")
            start_c, chunked = traj(ctx, model, Q, cps, eps, nsteps, Z)
            monkeypatch.delenv("NMGP_HAD_BATCH_SLAB_GB")
            start_w, whole = traj(ctx, model, Q, cps, eps, nsteps, Z)
            assert not whole[4].any() and np.all(np.isfinite(whole[3]))
            for a, b in zip(start_c + chunked, start_w + whole):
                assert np.array_equal(hh.bits(a) if a.dtype == np.float64 else a, hh.bits(b) if b.dtype == np.float64 else b)
    ctx.had_clear_subjects()


POISON_SNIPPET = r"""
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np
import hadamard_cohort_metric_cases as C
import test_gpu_hadamard_cohort_metric as t
from nonstationary_multivariate_gaussian_process_amd import _lib
ctx = _lib.Context(0)
out = {}
for model in C.MODELS:
    for name in ("P", "Q"):
        for key, per_subject in t.collect(ctx, model, name, 2).items():
            for s, a in enumerate(per_subject):
                out["%%s/%%s/%%s/%%d" %% (model, name, key, s)] = np.asarray(a)
ctx.close()
np.savez(%(path)r, **out)
print("POISON_OK")
"""


def test_poisoned_workspace(ctx, tmp_path):
    """NMGP_POISON=1 (read once per process: a fresh child, nothing preloaded) fills fresh buffers and the kept workspace with NaN before
    every call: a slot of the momentum, of a product's result or of the staging buffers that nobody wrote would change a bit of the
    products or of the trajectories on sets P and Q."""
    env = dict(os.environ)
    env["NMGP_POISON"] = "1"
    env.pop("NMGP_HAD_BATCH_SLAB_GB", None)
    path = str(tmp_path / "poisoned.npz")
    out = subprocess.run([sys.executable, "-c", POISON_SNIPPET % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "path": path}],
                         capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0 and "POISON_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    got = np.load(path)
    for model in C.MODELS:
        for name in ("P", "Q"):
            for key, per_subject in collect(ctx, model, name, 2).items():
                for s, a in enumerate(per_subject):
                    assert np.array_equal(hh.bits(np.asarray(a)), hh.bits(got["%s/%s/%s/%d" % (model, name, key, s)])), (model, name, key, s)


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("model", C.MODELS)
def test_one_step_against_the_longdouble_reference(ctx, model, name):
    k, S = 2, len(C.sizes(name))
    C.set_subjects(ctx, name)
    q0, z = C.chains(model, name, k), C.vectors(model, name, k)
    Q, Z, eps = C.pack(model, name, q0), C.pack(model, name, z), C.eps_of(name)
    out0, G0, status = evaluate(ctx, model, Q, k)
    assert status.tolist() == [0] * len(status)
    _, (q1, u1, kin1, U1, failed) = traj(ctx, model, Q, k, eps, 1, Z)
    ctx.had_subjects_traj_end()
    assert not failed.any()
    _, G1, _ = evaluate(ctx, model, q1, k)                                   # the gradient at the returned point: u1's second kick
    g0, g1, q1s, u1s = (C.unpack(model, name, a, k) for a in (G0, G1, q1, u1))
    disp, uref = [], []
    for s in range(S):
        pts, u = C.leapfrog_ld(model, name, s, q0[s], z[s], eps[s], 1, g0[s], lambda step, q, s=s: g1[s])
        disp.append(mc.displacement(pts))
        uref.append(u)
    eq, wq = C.worst_block(model, name, [np.asarray(a, dtype=LD) - np.asarray(b, dtype=LD) for a, b in zip(q1s, q0)], disp)
    eu, wu = C.worst_block(model, name, u1s, uref)
    print(model, name, "q1 - q0", eq, wq, "u1", eu, wu, "bar", C.BAR["traj"])
    mask, worst_k = ~C.pads(model, name, k), 0.0
    for r in range(Q.shape[0]):
        pr = u1[r][mask[r]]
        bound = (pr.shape[0] + 4) * 2.0 ** -53 * 0.5 * math.fsum(pr * pr)
        err = abs(kin1[r] - 0.5 * math.fsum(pr * pr))
        print("row", r, "kin1", kin1[r], "err", err, "bound", bound)
        worst_k = max(worst_k, err / bound)
    record_parity("hcohort_metric/%s/%s/one_step" % (model, name), displacement=(eq, C.BAR["traj"]), momentum=(eu, C.BAR["traj"]),
                  kinetic=(worst_k, 1.0))
    assert eq <= C.BAR["traj"] and eu <= C.BAR["traj"] and worst_k <= 1.0
    assert max(float(np.abs(np.asarray(a) - np.asarray(b)).max()) for a, b in zip(q1s, q0)) > 1e-8


@pytest.mark.parametrize("model", C.MODELS)
def test_two_steps_against_the_longdouble_reference(ctx, model):
    """Table D2's construction: the reference's middle point is rounded to float64 and its gradient taken from the evaluation entry
    (the device itself evaluated a point one rounding away: C.BAR["traj2"] holds the one-ulp sensitivity)."""
    name, k = "P", 2
    S = len(C.sizes(name))
    C.set_subjects(ctx, name)
    q0, z = C.chains(model, name, k), C.vectors(model, name, k)
    Q, Z, eps = C.pack(model, name, q0), C.pack(model, name, z), C.eps_of(name)
    g0 = C.unpack(model, name, evaluate(ctx, model, Q, k)[1], k)
    _, (q1, u1, kin1, U1, failed) = traj(ctx, model, Q, k, eps, 2, Z)
    ctx.had_subjects_traj_end()
    assert not failed.any()
    q1s, disp = C.unpack(model, name, q1, k), []
    for s in range(S):
        grad = subject_eval(ctx, model, name, k, s)
        pts, _ = C.leapfrog_ld(model, name, s, q0[s], z[s], eps[s], 2, g0[s], lambda step, q: grad(q)[1])
        disp.append(mc.displacement(pts))
    err, where = C.worst_block(model, name, [np.asarray(a, dtype=LD) - np.asarray(b, dtype=LD) for a, b in zip(q1s, q0)], disp)
    print(model, "two steps: q1 - q0", err, where, "bar", C.BAR["traj2"])
    record_parity("hcohort_metric/%s/P/two_steps" % model, displacement=(err, C.BAR["traj2"]))
    assert err <= C.BAR["traj2"]


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", C.MODELS)
def test_the_device_trajectory_is_the_dense_mass_leapfrog(ctx, model):
    name, k, nsteps = "P", 2, 2
    S = len(C.sizes(name))
    C.set_subjects(ctx, name)
    q0, z = C.chains(model, name, k), C.vectors(model, name, k)
    Q, Z, eps = C.pack(model, name, q0), C.pack(model, name, z), C.eps_of(name, C.MEANING_EPS0)
    out0, G0, _ = evaluate(ctx, model, Q, k)
    g0 = C.unpack(model, name, G0, k)
    (bout, _), (q1, u1, kin1, U1, failed) = traj(ctx, model, Q, k, eps, nsteps, Z)
    ctx.had_subjects_traj_end()
    assert not failed.any() and np.array_equal(hh.bits(bout), hh.bits(out0))
    mask = ~C.pads(model, name, k)
    K0 = np.array([0.5 * math.fsum(Z[r][mask[r]] ** 2) for r in range(Q.shape[0])], dtype=LD)
    dH = (np.asarray(U1, dtype=LD) + np.asarray(kin1, dtype=LD)) - (np.asarray(out0[:, 0], dtype=LD) + K0)
    q1s = C.unpack(model, name, q1, k)
    worst_q, worst_H = (0.0, ""), (0.0, "")
    for s in range(S):
        f = subject_eval(ctx, model, name, k, s)
        pts, Kd0, Kd1 = C.leapfrog_dense_ld(model, name, s, q0[s], z[s], eps[s], nsteps, g0[s], lambda step, q: f(q)[1])
        e, w = mc.block_errors(np.asarray(q1s[s], dtype=LD) - np.asarray(q0[s], dtype=LD), mc.displacement(pts), C.layout_of(model, name, s))
        ref = (np.asarray(f(pts[-1])[0], dtype=LD) + Kd1) - (np.asarray(out0[s * k:(s + 1) * k, 0], dtype=LD) + Kd0)
        eH = mc.scalar_error(dH[s * k:(s + 1) * k], ref)
        print(model, "subject", s, "q1 - q0", e, w, "dH", dH[s * k:(s + 1) * k], "dense", ref, "error", eH)
        worst_q, worst_H = max(worst_q, (e, "subject %d %s" % (s, w))), max(worst_H, (eH, "subject %d" % s))
    record_parity("hcohort_metric/%s/P/meaning" % model, displacement=(worst_q[0], C.BAR["meaning_q"]), energy=(worst_H[0], C.BAR["meaning_H"]))
    assert worst_q[0] <= C.BAR["meaning_q"], worst_q
    assert worst_H[0] <= C.BAR["meaning_H"], worst_H


# ---- 5 ----------------------------------------------------------------------------------------------------------------------------------
def bits_equal(a, b, mask, rows=slice(None)):
    """q1, u1 on the real slots, kin1, U1 and failed of two trajectory results"""
    return (all(hh.same_real_bits(x[rows], y[rows], mask[rows]) for x, y in zip(a[:2], b[:2]))
            and all(np.array_equal(hh.bits(x[rows]), hh.bits(y[rows])) for x, y in zip(a[2:4], b[2:4])) and np.array_equal(a[4][rows], b[4][rows]))


@pytest.mark.parametrize("model", C.MODELS)
def test_switching_the_mass_and_committing(ctx, model):
    name, k, nsteps = "P", 2, 2
    C.set_subjects(ctx, name)
    Q, Z, eps = C.pack(model, name, C.chains(model, name, k)), C.pack(model, name, C.vectors(model, name, k)), C.eps_of(name)
    Zb = C.pack(model, name, C.vectors(model, name, k, seed=C.P_SEED + 1000))
    mask = ~C.pads(model, name, k)
    B = Q.shape[0]
    _, first = traj(ctx, model, Q, k, eps, nsteps, Z)
    # kind 2 -> 0 -> 2 on ONE begun trajectory
    ctx.had_subjects_traj_commit(np.zeros(B, dtype=bool))
    ctx.had_subjects_traj_set_mass(None)
    ident = ctx.had_subjects_traj(eps * 1e-3, nsteps, Z, want_p1=True, want_kin=True)
    assert not ident[4].any() and not hh.same_real_bits(ident[0], first[0], mask)
    ctx.had_subjects_traj_commit(np.zeros(B, dtype=bool))
    ctx.had_subjects_traj_set_mass(prior=True)
    again = ctx.had_subjects_traj(eps, nsteps, Z, want_p1=True, want_kin=True)
    assert bits_equal(again, first, mask)
    # commit with rejections: position, gradient and flag of the rejected chains are restored
    accept = np.arange(B) % 2 == 0
    ctx.had_subjects_traj_commit(accept)
    repeat = ctx.had_subjects_traj(eps, nsteps, Z, want_p1=True, want_kin=True)
    assert bits_equal(repeat, first, mask, ~accept)
    ctx.had_subjects_traj_commit(np.zeros(B, dtype=bool))
    second = ctx.had_subjects_traj(eps, nsteps, Zb, want_p1=True, want_kin=True)
    _, fresh = traj(ctx, model, np.where(accept[:, None], first[0], Q), k, eps, nsteps, Zb)
    assert bits_equal(second, fresh, mask) and not second[4].any()
    assert not hh.same_real_bits(first[0], Q, mask)
    ctx.had_subjects_traj_end()


@pytest.mark.parametrize("model", C.MODELS)
def test_a_failure_stays_in_its_chain(ctx, model):
    name, k, nsteps = "P", 2, 2
    sz = C.sizes(name)
    C.set_subjects(ctx, name)
    Q, Z, eps = C.pack(model, name, C.chains(model, name, k)), C.pack(model, name, C.vectors(model, name, k)), C.eps_of(name)
    mask = ~C.pads(model, name, k)
    bad_row = 3 * k + 1                                                      # chain 1 of the subject with N_s = 65
    others = np.arange(Q.shape[0]) != bad_row
    _, base = traj(ctx, model, Q, k, eps, nsteps, Z)
    # (a) bad at the start: a NaN in a real slot of the second tile
    Qb = Q.copy()
    Qb[bad_row, 64] = np.nan
    assert mask[bad_row, 64]
    (_, status), dev = traj(ctx, model, Qb, k, eps, nsteps, Z)
    assert status[bad_row] != 0 and status[others].tolist() == [0] * int(others.sum())
    assert dev[4][bad_row] and np.isposinf(dev[3][bad_row]) and not dev[4][others].any()
    assert bits_equal(dev, base, mask, others)
    # (b) pushed to a non-finite position in the first drift: the subject's step size is huge and one whitened momentum is 1e300
    far = eps.copy()
    far[3] = 1e10
    Zp = Z.copy()
    Zp[bad_row, np.flatnonzero(mask[bad_row])[-1]] = 1e300
    _, base_far = traj(ctx, model, Q, k, far, nsteps, Z)
    _, dev = traj(ctx, model, Q, k, far, nsteps, Zp)
    assert dev[4][bad_row] and np.isposinf(dev[3][bad_row]) and not np.all(np.isfinite(dev[0][bad_row][mask[bad_row]]))
    other_subjects = np.repeat(np.arange(len(sz)) != 3, k)
    assert not dev[4][other_subjects].any() and np.all(np.isfinite(dev[3][other_subjects]))
    assert bits_equal(dev, base_far, mask, others)
    ctx.had_subjects_traj_end()


def test_refusals(ctx):
    from nonstationary_multivariate_gaussian_process_amd import _lib
    import hadamard_cohort_cases as cc
    name, k = "E", 1
    fresh = _lib.Context(0)
    try:
        v = C.pack("non", name, C.vectors("non", name, k))
        rc = fresh.lib.nmgp_had_subjects_prior_apply(fresh.h, 0, _lib.ptr(C.HYPER["non"]), 0, _lib.ptr(v), v.shape[0], k, _lib.ptr(np.empty_like(v)))
        assert rc == E_STATE                                       # no set
    finally:
        fresh.close()
    C.set_subjects(ctx, name)
    v = C.pack("non", name, C.vectors("non", name, k))
    out = np.empty_like(v)
    call = lambda model, B, cps: ctx.lib.nmgp_had_subjects_prior_apply(ctx.h, model, _lib.ptr(C.HYPER["sep"]), 0, _lib.ptr(v), B, cps, _lib.ptr(out))
    assert call(0, v.shape[0] + 1, k) == E_SHAPE and call(0, v.shape[0], 0) == E_SHAPE
    assert call(3, v.shape[0], k) == E_SHAPE and call(-1, v.shape[0], k) == E_SHAPE
    assert call(2, v.shape[0], k) == E_UNSUPPORTED
    good = ctx.had_subjects_prior_apply("non", C.HYPER["non"], v, False, k)   # the context stays usable
    # the trajectory's mass: kind 3, and kind 2 on the stationary model with kind 1 in force
    cases = cc.SET_D
    subs = cc.subjects(cases)
    ctx.had_set_subjects([c["x"] for c in subs], [c["indx"] for c in subs], [c["y"] for c in subs], M=cases[0][1])
    hyper, S = hh.hyper_of("sta", cases), len(cases)
    P = hh.pack("sta", hh.chains("sta", cases, 1), cc.nobs(cases), cases[0][1])
    p0 = hh.momenta("sta", cases, 1, 9100)
    minv = hh.pack("sta", [1.0 / m[None] for m in hh.diag_mass("sta", cases)], cc.nobs(cases), cases[0][1])
    ctx.had_subjects_traj_begin("sta", P, hyper, True, 1)
    ctx.had_subjects_traj_set_mass(minv)
    want = ctx.had_subjects_traj(hh.eps_of(S), 2, p0, want_p1=True, want_kin=True)
    ctx.had_subjects_traj_commit(np.zeros(S, dtype=bool))
    assert ctx.lib.nmgp_had_subjects_traj_set_mass(ctx.h, 2, None) == E_UNSUPPORTED
    assert ctx.lib.nmgp_had_subjects_traj_set_mass(ctx.h, 3, None) == E_SHAPE
    assert ctx.lib.nmgp_had_subjects_traj_set_mass(ctx.h, -1, None) == E_SHAPE
    got = ctx.had_subjects_traj(hh.eps_of(S), 2, p0, want_p1=True, want_kin=True)
    for a, b in zip(got, want):                                              # kind 1 is still in force
        assert np.array_equal(hh.bits(a) if a.dtype == np.float64 else a, hh.bits(b) if b.dtype == np.float64 else b)
    ctx.had_subjects_traj_end()
    C.set_subjects(ctx, name)
    assert np.array_equal(hh.bits(ctx.had_subjects_prior_apply("non", C.HYPER["non"], v, False, k)), hh.bits(good))


# ---- 6 ----------------------------------------------------------------------------------------------------------------------------------
DRIVER_BAR = C.BAR["traj2"]          # the sweep's bar on a displacement, with the one-ulp term of the evaluated middle points


@pytest.mark.parametrize("waste", (0.0, 0.5))
@pytest.mark.parametrize("name", ("P", "Q"))
@pytest.mark.parametrize("model", C.MODELS)
def test_the_resident_driver_against_the_host_loop(model, name, waste):
    """identical accept decisions (the CPU half shows that none of this seed's is within 1e-6 of its threshold), samples within the bar
    on the displacement from the start -- not bit for bit: NumPy's GEMM and the kernel's tiles sum a product in different orders"""
    from nonstationary_multivariate_gaussian_process_amd import drivers
    k, n, runs = 2, 3, {}
    for resident in (False, True):
        d = getattr(drivers, hh.DRIVER[model])(C.triples(name), C.hyper_dict(model), C.chains(model, name, k), step_size=C.DRIVER_EPS,
                                               num_steps_in_leap=3, seed=C.DRIVER_SEED, mass="prior", device_resident=resident,
                                               device_kinetic=resident, max_flop_waste=waste)
        try:
            runs[resident] = d.run(n)
        finally:
            d.close()
    (hs, hi), (rs, ri) = runs[False], runs[True]
    print(model, name, waste, "accept rates", hi["accept_rate"], ri["accept_rate"])
    assert np.array_equal(hi["accept_rate"], ri["accept_rate"]) and 0 < hi["accept_rate"].sum() < len(hi["accept_rate"])
    assert np.array_equal(np.isfinite(hi["energy_error"]), np.isfinite(ri["energy_error"]))
    worst = (0.0, "")
    for s, q0 in enumerate(C.chains(model, name, k)):
        for it in range(n):
            e, w = mc.block_errors(np.asarray(rs[s][it], dtype=LD) - q0, np.asarray(hs[s][it], dtype=LD) - q0, C.layout_of(model, name, s))
            worst = max(worst, (e, "subject %d iteration %d %s" % (s, it, w)))
    print("worst block error of the displacement from the start", worst, "bar", DRIVER_BAR)
    record_parity("hcohort_metric/%s/%s/driver/max_flop_waste_%g" % (model, name, waste), displacement=(worst[0], DRIVER_BAR))
    assert worst[0] <= DRIVER_BAR, worst


# ---- 7 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", C.MODELS)
def test_the_metric_does_its_job(model):
    from nonstationary_multivariate_gaussian_process_amd import drivers
    name, k, dH = "P", 2, {}
    for mass in ("prior", None):
        d = getattr(drivers, hh.DRIVER[model])(C.triples(name), C.hyper_dict(model, ill=True), C.prior_draw_chains(model, name, k),
                                               step_size=C.JOB_EPS, num_steps_in_leap=C.JOB_STEPS, seed=C.DRIVER_SEED, mass=mass,
                                               device_resident=True, max_flop_waste=1e9)
        try:
            dH[mass] = d.run(1)[1]["energy_error"][0]
        finally:
            d.close()
    print(model, "dH under the prior metric", dH["prior"], "under the identity", dH[None])
    diag = np.arange(dH[None].shape[0]) // k == C.JOB_DIAGONAL
    assert np.all(np.abs(dH["prior"]) < C.JOB_DH_PRIOR)
    assert np.all(np.isnan(dH[None][~diag]) | (np.abs(dH[None][~diag]) > C.JOB_DH_IDENTITY))
    assert np.all(np.abs(dH[None][diag]) < C.JOB_DH_PRIOR)
