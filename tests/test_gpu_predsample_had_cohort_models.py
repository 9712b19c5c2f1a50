"""MAP and posterior-draw prediction for a cohort of ragged Hadamard subjects under the separable ("sep": nmgp_predsample_hads_subjects,
hadamard_sep.cohort_predict, drivers.HadamardSepCohortMAP.predict, drivers.posterior_predict_hadamard_sep_cohort) and the stationary
model ("sta": nmgp_predict_hadst_subjects, hadamard_sta.cohort_predict, drivers.HadamardStaCohortMAP.predict,
drivers.posterior_predict_hadamard_sta_cohort) on the GPU: against the NumPy restatements of hadamard_cases.predictions on each
subject ALONE (tests/test_predsample_had_cohort_models_cpu.py holds the padding argument and the precondition of the bars), against
the resident entries nmgp_predsample_hads / nmgp_predict_hadst, and against itself across sets, batch, chunk and slice sizes.

Bars: separable mean and variance 1e-5 relative element by element, starred values 1e-6 (tests/test_gpu_predsample_had_cohort.py's);
stationary mean and variance 1e-9 (tests/test_gpu_hadamard_sweep.py's STA_PRED_TOL); indexed against full 1e-10; everything else bit
for bit.  All shapes are tests/hadamard_cohort_cases.SETS', the inputs each subject's own default grid (ragged within a set)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import hadamard_cases as hc
import hadamard_cohort_cases as cc
import hadamard_cohort_model_cases as mc
from conftest import ROOT, SEP_KEYS, STA_KEYS, hyper_dict, record_parity, relerr

pytestmark = pytest.mark.gpu

MODELS = ("sep", "sta")
PRED_TOL, STAR_TOL, STA_PRED_TOL, FORM_TOL = 1e-5, 1e-6, 1e-9, 1e-10
HYPER = hc.hypers()
KEYS = {"sep": SEP_KEYS, "sta": STA_KEYS}


@pytest.fixture(scope="module")
def ctx():
    from nonstationary_multivariate_gaussian_process_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def same_bits(a, b):
    return len(a) == len(b) and all(np.array_equal(u, v, equal_nan=True) for u, v in zip(a, b))


def all_same_bits(res_a, res_b):
    return len(res_a) == len(res_b) and all(same_bits(a, b) for a, b in zip(res_a, res_b))


def rows(res, sel):
    """the draws `sel` of every array of every subject's result"""
    return [[a[sel] for a in r] for r in res]


def set_subjects(ctx, cases, Nmax=None):
    subs = cc.subjects(cases)
    ctx.had_set_subjects([c["x"] for c in subs], [c["indx"] for c in subs], [c["y"] for c in subs], M=cases[0][1], Nmax=Nmax)


def pred(case, form):
    """the restatements of a subject alone in a form: at its default grid, but the slice wider than 256 riding rows for hc.WIDE"""
    if case == hc.WIDE:
        return hc.predictions(case, **(hc.WIDE_FULL if form == "full" else hc.WIDE_INDEXED))
    return hc.predictions(case)


def inputs(cases, form="full", S=None, step=3):
    """per-subject (xs, labels or None, z [2, S_s, 2]) lists; S: one grid size for every subject instead of the default grids"""
    xs, lab, z = [], [], []
    for case in cases:
        if S is None:
            e = pred(case, form)
            xs.append(e["xs"]), lab.append(e["lab"]), z.append(e["z"])
        else:
            c = hc.build(case)
            v = hc.grid(c["N"], c["M"], c["x"], S)
            xs.append(v), lab.append(hc.grid_labels(S, c["M"], step)), z.append(hc.normals(case, S))
    return xs, (lab if form == "ix" else None), z


def more_draws(model, case, H):
    """H draws on the segment through the subject's two (and beyond it): smooth, distinct, all factorable."""
    d = hc.build(case)["pars"][model]
    return np.stack([d[0] + 0.5 * k * (d[1] - d[0]) for k in range(H)])


def call(ctx, model, draws, xs, lab=None, z=None, star=None):
    """the model's ragged cohort predictor: per subject (mean, var[, star], status)"""
    from nonstationary_multivariate_gaussian_process_amd import hadamard_sep, hadamard_sta
    if model == "sep":
        return hadamard_sep.cohort_predict(ctx, draws, xs, HYPER["sep"], indx_star=lab, z=z, star=star)
    return hadamard_sta.cohort_predict(ctx, draws, xs, indx_star=lab)


def predict(ctx, model, cases, form="full", S=None, draws=None, z="fixed", star=None):
    xs, lab, zz = inputs(cases, form, S)
    draws = mc.chains(model, cases, 2) if draws is None else draws
    return call(ctx, model, draws, xs, lab, zz if z == "fixed" and star is None else (None if z == "fixed" else z), star)


def statuses(res):
    return [r[-1].tolist() for r in res]


# ---- 1. parity with the restatements on each subject alone ------------------------------------------------------------------------------
PARITY_SETS = {"A": cc.SET_A, "B": cc.SET_B, "C": [c for c in cc.SET_C if c != hc.MINOR], "D": cc.SET_D, "E": cc.SET_E,
               "F": cc.SET_F, "G": cc.SET_G, "H": cc.SET_H, "I": cc.SET_I}      # F - H: k_hadcs / k_hadcst_cross_rows<4, 6, 7>; I: Nmax = 1030


def reference(model, case, form):
    """(mean, var[, star]) [2, S(, M)] of the two draws from the restatement on the subject alone"""
    e = pred(case, form)
    if model == "sta":
        m = e["sta_full" if form == "full" else "sta_ix"]
        return np.stack([m[0][0], m[1][0]]), np.stack([m[0][1], m[1][1]])
    loc, scale = (np.swapaxes(a, 0, 1) for a in e["hps_full" if form == "full" else "hps_ix"])       # [H, S, 2 + K]
    star = loc[:, :, :2] + scale[:, :, :2] * e["z"]
    if form == "full":
        return loc[:, :, 2:], scale[:, :, 2:] ** 2, star
    return loc[:, :, 2], scale[:, :, 2] ** 2, star


@pytest.mark.parametrize("name", sorted(PARITY_SETS))
@pytest.mark.parametrize("model", MODELS)
def test_two_draws_per_subject_meet_the_restatement_on_the_subject_alone(ctx, model, name):
    from nonstationary_multivariate_gaussian_process_amd import hadamard
    cases = PARITY_SETS[name]
    worst = {}
    for form in ("full", "ix"):
        # through the binding on padded arrays with NaN (labels: 99) in every padded slot of the call and of the set: a kernel that
        # reads one cannot meet a bar
        raw, ns, _ = padded_call(ctx, model, cases, form, np.nan, 99, poison_set=True)
        res = list(zip(*(hadamard.cohort_unpack_outputs(a, ns, 2) for a in raw)))
        for case, r in zip(cases, res):
            c = hc.build(case)
            ref = reference(model, case, form)
            S = pred(case, form)["xs"].shape[0]
            assert r[-1].tolist() == [0, 0] and len(r) == len(ref) + 1
            assert r[0].shape == r[1].shape == ((2, S, c["M"]) if form == "full" else (2, S))
            assert model == "sta" or r[2].shape == (2, S, 2)
            errs = {k: relerr(a, b) for k, a, b in zip(("mean", "var", "star"), r[:-1], ref)}
            tol = {"mean": PRED_TOL, "var": PRED_TOL, "star": STAR_TOL} if model == "sep" else {"mean": STA_PRED_TOL, "var": STA_PRED_TOL}
            tag = "hpcohort_%s/%s/%s/%s" % (model, name, form, hc.case_id(case))
            print(tag, errs)
            record_parity(tag, **{k: (v, tol[k]) for k, v in errs.items()})
            for k, v in errs.items():
                worst[form + "_" + k] = max(worst.get(form + "_" + k, 0.0), v)
            for k, v in errs.items():
                assert v < tol[k], (tag, k, v)
    print("hpcohort_%s/%s worst" % (model, name), worst)


# ---- 2. padded slots ---------------------------------------------------------------------------------------------------------------------
def padded_call(ctx, model, cases, form, fill, lab_fill, star=None, nstar=None, poison_set=False):
    """the C entry through its binding on padded arrays whose padded slots hold `fill` (labels: `lab_fill`), the set's own pads
    included"""
    from nonstationary_multivariate_gaussian_process_amd import hadamard
    subs, M = cc.subjects(cases), cases[0][1]
    nobs = cc.nobs(cases)
    Nmax = max(nobs)
    xs, lab, z = inputs(cases, form)
    x2, y2 = np.full((len(cases), Nmax), fill if poison_set else 0.0), np.full((len(cases), Nmax), fill if poison_set else 0.0)
    i2 = np.full((len(cases), Nmax), lab_fill if poison_set else 0, dtype=np.int32)
    for s, c in enumerate(subs):
        x2[s, :nobs[s]], y2[s, :nobs[s]], i2[s, :nobs[s]] = c["x"], c["y"], c["indx"]
    ctx.had_set_subjects_padded(x2, i2, y2, nobs, M)
    own = [v.shape[0] for v in xs]
    ns = own if nstar is None else nstar
    Smax = max(own)
    xs2 = hadamard.cohort_pack_inputs([v[:n] for v, n in zip(xs, ns)], Smax=Smax, fill=fill)[0]
    l2 = None if lab is None else hadamard.cohort_pack_inputs([v[:n] for v, n in zip(lab, ns)], Smax=Smax, fill=lab_fill, dtype=np.int32)[0]
    pars = mc.pack(model, mc.chains(model, cases, 2), nobs, M, fill=fill)
    if model == "sta":
        return ctx.predict_hadst_subjects(pars, xs2, indx_star=l2, nstar=ns, draws_per_subject=2), ns, Smax
    z2 = hadamard.cohort_pack_inputs([v[:, :n] for v, n in zip(z, ns)], Smax=Smax, fill=fill)[0] if star is None else None
    s2 = None
    if star is not None:
        s2 = star.copy()
        for s, n in enumerate(ns):
            s2[2 * s:2 * s + 2, n:] = fill
    return ctx.predsample_hads_subjects(pars, HYPER["sep"], xs2, indx_star=l2, nstar=ns, draws_per_subject=2, z=z2, star=s2), ns, Smax


@pytest.mark.parametrize("form", ["full", "ix"])
@pytest.mark.parametrize("model", MODELS)
def test_poisoned_padded_slots_change_no_bit_and_padded_outputs_are_plus_zero(ctx, model, form):
    cases = cc.SET_A
    clean, ns, Smax = padded_call(ctx, model, cases, form, 0.0, 0)
    assert clean[-1].tolist() == [0] * 12 and Smax == 63 and min(ns) == 3
    if model == "sep":
        assert np.isnan(mc.pack("sep", mc.chains("sep", cases, 2), cc.nobs(cases), 2, fill=np.nan)).sum() > 0
    checked = []
    for fill, lab_fill in ((np.nan, 99), (1e300, -1)):
        dirty, _, _ = padded_call(ctx, model, cases, form, fill, lab_fill, poison_set=True)
        assert same_bits(clean, dirty), (fill, lab_fill)
        checked.append(dirty)
        if model == "sep":
            fed_clean, _, _ = padded_call(ctx, model, cases, form, 0.0, 0, star=clean[2])
            fed_dirty, _, _ = padded_call(ctx, model, cases, form, fill, lab_fill, star=clean[2], poison_set=True)
            assert same_bits(fed_clean, fed_dirty) and same_bits(fed_clean, clean)
            checked.append(fed_dirty)
    for s, n in enumerate(ns):
        for res in checked:
            for a in res[:-1]:
                pad, real = a[2 * s:2 * s + 2, n:], a[2 * s:2 * s + 2, :n]
                assert np.all(pad == 0.0) and not np.any(np.signbit(pad)) and np.all(np.isfinite(real))
    # a patient with nothing to predict: all-zero rows, status 0; the others keep their bits
    ns0 = list(ns)
    ns0[1] = 0
    zero, _, _ = padded_call(ctx, model, cases, form, np.nan, 99, nstar=ns0, poison_set=True)
    assert zero[-1].tolist() == [0] * 12
    for a, b in zip(zero[:-1], clean[:-1]):
        assert np.all(a[2:4] == 0.0) and not np.any(np.signbit(a[2:4]))
        keep = np.r_[0:2, 4:12]
        assert np.array_equal(a[keep], b[keep])


# ---- 3. - 6. bits ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_a_subject_alone_in_a_set_of_one_gives_the_bits_of_its_rows_in_the_set(ctx, model):
    cases = cc.SET_A
    for form in ("full", "ix"):
        set_subjects(ctx, cases)
        full = predict(ctx, model, cases, form)
        for s in (0, 1, 2, 4):                                             # N_s = Nmax, a mask inside a tile, N_s = M, one past an edge
            set_subjects(ctx, [cases[s]], Nmax=128)
            one = predict(ctx, model, [cases[s]], form)
            assert one[0][-1].tolist() == [0, 0] and same_bits(one[0], full[s]), (form, s)


@pytest.mark.parametrize("model", MODELS)
def test_five_draws_per_subject_give_the_bits_of_five_calls_whatever_the_chunking(ctx, model, monkeypatch):
    monkeypatch.delenv("NMGP_PREDSAMPLE_CHUNK", raising=False)
    cases = cc.SET_A
    set_subjects(ctx, cases)
    draws = [more_draws(model, c, 5) for c in cases]
    for form in ("full", "ix"):
        xs, lab, _ = inputs(cases, form)
        z = [np.random.default_rng(12 + s).standard_normal((5, v.shape[0], 2)) for s, v in enumerate(xs)] if model == "sep" else None
        sub = lambda k: None if z is None else [v[k] for v in z]
        big = call(ctx, model, draws, xs, lab, z)
        assert all(r[-1].tolist() == [0] * 5 for r in big) and not np.array_equal(big[0][0][0], big[0][0][1])
        for k in range(5):
            one = call(ctx, model, [d[k:k + 1] for d in draws], xs, lab, sub(slice(k, k + 1)))
            assert all_same_bits(rows(big, slice(k, k + 1)), one), (form, k)
        monkeypatch.setenv("NMGP_PREDSAMPLE_CHUNK", "2")                  # parts of ONE subject's draws: 2, 2 and 1
        split = call(ctx, model, draws, xs, lab, z)
        two = call(ctx, model, [d[:2] for d in draws], xs, lab, sub(slice(0, 2)))        # one whole subject per chunk
        monkeypatch.setenv("NMGP_PREDSAMPLE_CHUNK", "4")                  # two whole subjects per chunk
        four = call(ctx, model, [d[:2] for d in draws], xs, lab, sub(slice(0, 2)))
        monkeypatch.delenv("NMGP_PREDSAMPLE_CHUNK")
        assert all_same_bits(big, split)
        assert all_same_bits(rows(big, slice(0, 2)), two) and all_same_bits(two, four)


@pytest.mark.parametrize("model", MODELS)
def test_a_grid_point_moved_to_another_slice_keeps_its_bits(ctx, model):
    cases = PARITY_SETS["C"]                                               # Nmax = 321, M = 3: slices of 107 inputs (full), 321 (indexed)
    assert cases[0] == hc.WIDE
    set_subjects(ctx, cases)
    draws = mc.chains(model, cases, 2)
    for form, sizes in (("full", (110, 9, 3)), ("ix", (330, 9, 3))):
        got = [inputs([c], form, S=S, step=2) for c, S in zip(cases, sizes)]
        xs, z = [g[0][0] for g in got], [g[2][0] for g in got]
        lab = None if form == "full" else [g[1][0] for g in got]
        zz = z if model == "sep" else None
        a = call(ctx, model, draws, xs, lab, zz)
        rev = [np.arange(S)[::-1] for S in sizes]
        b = call(ctx, model, draws, [v[r].copy() for v, r in zip(xs, rev)], None if lab is None else [v[r].copy() for v, r in zip(lab, rev)],
                 None if zz is None else [np.ascontiguousarray(v[:, r]) for v, r in zip(z, rev)])
        for ra, rb, r in zip(a, b, rev):
            assert ra[-1].tolist() == rb[-1].tolist() == [0, 0] and same_bits([v[:, r] for v in rb[:-1]], ra[:-1]), form
        head = call(ctx, model, draws, [v[:3].copy() for v in xs], None if lab is None else [v[:3].copy() for v in lab],
                    None if zz is None else [np.ascontiguousarray(v[:, :3]) for v in z])
        for ra, rh in zip(a, head):
            assert same_bits(rh[:-1], [v[:, :3] for v in ra[:-1]]), form


@pytest.mark.parametrize("model", MODELS)
def test_indexed_form_is_the_labelled_column_of_the_full_form(ctx, model):
    cases = cc.SET_A
    set_subjects(ctx, cases)
    full = predict(ctx, model, cases, "full")
    ix = predict(ctx, model, cases, "ix", star=[r[2] for r in full] if model == "sep" else None)
    _, lab, _ = inputs(cases, "ix")
    e_m = e_v = 0.0
    for rf, ri, l in zip(full, ix, lab):
        S = l.shape[0]
        assert rf[-1].tolist() == ri[-1].tolist() == [0, 0] and ri[0].shape == ri[1].shape == (2, S)
        assert model == "sta" or np.array_equal(ri[2], rf[2])
        e_m = max(e_m, relerr(ri[0], rf[0][:, np.arange(S), l]))
        e_v = max(e_v, relerr(ri[1], rf[1][:, np.arange(S), l]))
    print(model, "indexed against full: mean", e_m, "var", e_v)
    record_parity("hpcohort_%s/A/indexed_vs_full" % model, mean=(e_m, FORM_TOL), var=(e_v, FORM_TOL))
    assert e_m < FORM_TOL and e_v < FORM_TOL


# ---- 7. against the resident entries ---------------------------------------------------------------------------------------------------------
def test_unpadded_subjects_give_the_stationary_resident_entry_its_bits(ctx):
    cases = cc.SET_E
    assert cc.nobs(cases) == [64, 64]
    for form in ("full", "ix"):
        set_subjects(ctx, cases)
        xs, lab, _ = inputs(cases, form)
        assert len({v.shape[0] for v in xs}) == 1                          # equal grids: nstar = Smax
        res = predict(ctx, "sta", cases, form)
        for s, case in enumerate(cases):
            c = hc.build(case)
            ctx.had_set_data(c["x"], c["indx"], c["y"])
            want = ctx.predict_hadst(c["pars"]["sta"], xs[s], indx_star=None if lab is None else lab[s])
            assert want[2].tolist() == [0, 0] and same_bits(res[s], want), (form, s)


def test_unpadded_subjects_give_the_separable_resident_entry_its_bits(ctx):
    cases = cc.SET_E
    hy = HYPER["sep"]
    for form in ("full", "ix"):
        set_subjects(ctx, cases)
        xs, lab, z = inputs(cases, form)
        assert len({v.shape[0] for v in xs}) == 1
        reg = predict(ctx, "sep", cases, form)
        fed = predict(ctx, "sep", cases, form, star=[r[2] for r in reg])
        d = 0.0
        for s, case in enumerate(cases):
            c = hc.build(case)
            ctx.had_set_data(c["x"], c["indx"], c["y"])
            l = None if lab is None else lab[s]
            r_fed = ctx.predsample_hads(c["pars"]["sep"], hy, xs[s], indx_star=l, star=reg[s][2])
            r_reg = ctx.predsample_hads(c["pars"]["sep"], hy, xs[s], indx_star=l, z=z[s])
            assert r_fed[3].tolist() == fed[s][3].tolist() == [0, 0]
            assert same_bits(fed[s], r_fed), (form, s)                     # under the same starred values: bit for bit
            assert same_bits(fed[s][:2], reg[s][:2])
            # with the regression on, the prior factors come from two factorisation calls: the distance is recorded
            d = max(d, relerr(reg[s][2], r_reg[2]))
            print("set E", form, hc.case_id(case), "star vs resident", relerr(reg[s][2], r_reg[2]), "bit-identical",
                  np.array_equal(reg[s][2], r_reg[2]), "mean", relerr(reg[s][0], r_reg[0]), "var", relerr(reg[s][1], r_reg[1]))
        record_parity("hpcohort_sep/E/%s/vs_resident" % form, star=(d, STAR_TOL))
        assert d < STAR_TOL


# ---- 8. failure stays local ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_status_of_a_bad_draw_and_every_other_subject(ctx, model, monkeypatch):
    from nonstationary_multivariate_gaussian_process_amd import _lib
    monkeypatch.delenv("NMGP_PREDSAMPLE_CHUNK", raising=False)
    cases = cc.SET_C
    k = cases.index(hc.MINOR)
    others = [c for c in cases if c != hc.MINOR]
    xs = [hc.build(c)["xs"] for c in cases]                                # short grids for all
    z = [np.random.default_rng(65 + s).standard_normal((3, v.shape[0], 2)) for s, v in enumerate(xs)] if model == "sep" else None
    lab = [hc.grid_labels(v.shape[0], 3, 2) for v in xs]
    P = hc.minor_chains(model)
    nan = P[[0, 2, 0]].copy()
    nan[1, 40 if model == "sep" else 0] = np.nan                           # a real slot: tilde_l[40] of 65, the one tilde_l
    keep = [s for s in range(len(cases)) if s != k]
    pick = lambda a: None if a is None else [a[s] for s in keep]
    for ix in (None, lab):
        for bad, want in ((P, 3), (nan, _lib.NUM_NAN)):
            draws = [bad if c == hc.MINOR else more_draws(model, c, 3) for c in cases]
            set_subjects(ctx, cases)
            res = call(ctx, model, draws, xs, ix, z)
            print(model, "indexed" if ix is not None else "full", "status", statuses(res))
            assert res[k][-1].tolist() == [0, want, 0]
            assert np.all(np.isnan(res[k][0][1])) and np.all(np.isnan(res[k][1][1]))
            assert np.all(np.isfinite(res[k][0][[0, 2]])) and np.all(np.isfinite(res[k][1][[0, 2]]))
            set_subjects(ctx, others, Nmax=max(cc.nobs(cases)))
            clean = call(ctx, model, [draws[s] for s in keep], [xs[s] for s in keep], pick(ix), pick(z))
            assert all(r[-1].tolist() == [0, 0, 0] for r in clean)
            assert all_same_bits([res[s] for s in keep], clean)
            # ... and the bad draw's neighbours: the bits of the call with a good draw in its place
            good = list(draws)
            good[k] = P[[0, 2, 2]] if bad is P else P[[0, 2, 0]]
            set_subjects(ctx, cases)
            ref = call(ctx, model, good, xs, ix, z)
            assert ref[k][-1].tolist() == [0, 0, 0] and same_bits([a[[0, 2]] for a in res[k][:2]], [a[[0, 2]] for a in ref[k][:2]])


# ---- 9. arguments and state ------------------------------------------------------------------------------------------------------------------------
def raw_call(ctx, model, pars, H, xs, lab=None, nstar=None, Smax=None, z=None, star=None):
    """the C entry as it is: its return code"""
    from nonstationary_multivariate_gaussian_process_amd import _lib
    ptr, ip = _lib.ptr, ctypes.POINTER(ctypes.c_int)
    B = pars.shape[0]
    Smax = xs.shape[1] if Smax is None else Smax
    out = np.empty((B, max(Smax, 1), 8)), np.empty((B, max(Smax, 1), 8)), np.empty((B, max(Smax, 1), 2))
    status = np.zeros(B, dtype=np.int32)
    lab = None if lab is None else np.ascontiguousarray(lab, dtype=np.int32)
    nstar = None if nstar is None else np.ascontiguousarray(nstar, dtype=np.int32)
    li, ni = (None if a is None else a.ctypes.data_as(ip) for a in (lab, nstar))
    if model == "sta":
        return ctx.lib.nmgp_predict_hadst_subjects(ctx.h, ptr(pars), B, H, ptr(xs), li, ni, Smax, ptr(out[0]), ptr(out[1]),
                                                   status.ctypes.data_as(ip))
    hy = _lib.as_f64(HYPER["sep"])
    return ctx.lib.nmgp_predsample_hads_subjects(ctx.h, ptr(pars), B, H, ptr(hy), ptr(xs), li, ni, Smax, ptr(z), ptr(star), ptr(out[0]),
                                                 ptr(out[1]), ptr(out[2]), status.ctypes.data_as(ip))


@pytest.mark.parametrize("model", MODELS)
def test_argument_and_state_checks(ctx, model, monkeypatch):
    from nonstationary_multivariate_gaussian_process_amd import _lib, hadamard
    cases = cc.SET_D                                                       # M = 1, nobs 1 / 2 / 70
    nobs, M = cc.nobs(cases), 1
    pars = mc.pack(model, mc.chains(model, cases, 2), nobs, M)
    grids = [hc.build(c)["xs"] for c in cases]
    xs = hadamard.cohort_pack_inputs(grids)[0]
    Smax = xs.shape[1]
    zz = np.zeros((6, Smax, 2))
    ctx.had_clear_subjects()
    assert raw_call(ctx, model, pars, 2, xs) == -3                         # NMGP_E_STATE: no set
    with pytest.raises(_lib.NmgpError):
        call(ctx, model, mc.chains(model, cases, 2), grids)
    set_subjects(ctx, cases)

    def works():
        return all(s == [0, 0] for s in statuses(predict(ctx, model, cases, "full")))

    assert works()
    if model == "sep":
        assert raw_call(ctx, model, pars, 2, xs, z=zz, star=zz) == -3 and works()    # NMGP_E_STATE: z with star_in
    assert raw_call(ctx, model, pars[:5], 2, xs) == -2 and works()         # NMGP_E_SHAPE: B != S * draws_per_subject
    assert raw_call(ctx, model, pars, 3, xs) == -2 and works()
    assert raw_call(ctx, model, pars, 0, xs) == -2 and works()             # draws_per_subject < 1
    assert raw_call(ctx, model, pars, 2, xs, Smax=0) == -2 and works()     # Smax < 1
    for bad in ([Smax + 1, 1, 1], [1, -1, 1]):                             # nstar outside [0, Smax]
        assert raw_call(ctx, model, pars, 2, xs, nstar=bad) == -2 and works()
    lab = np.zeros(xs.shape, dtype=np.int32)
    for v in (1, -1):                                                      # a real label outside [0, M)
        lab[1, 2] = v
        assert raw_call(ctx, model, pars, 2, xs, lab=lab, nstar=[3, 3, 3]) == -2 and works()
        assert raw_call(ctx, model, pars, 2, xs, lab=lab, nstar=[3, 2, 3]) == 0      # ... in a padded slot it is not read
    # nstar[s] = 0 for one and for all subjects
    for ns in ([3, 0, 3], [0, 0, 0]):
        assert raw_call(ctx, model, pars, 2, xs, nstar=ns) == 0 and works()
    empty = call(ctx, model, mc.chains(model, cases, 2), [np.zeros(0)] * 3)
    assert statuses(empty) == [[0, 0]] * 3 and all(r[0].shape == (2, 0, 1) for r in empty)
    if model == "sta":
        assert ctx.lib.nmgp_predict_hadst_subjects(None, None, 0, 0, None, None, None, 0, None, None, None) == -1
        assert ctx.lib.nmgp_predict_hadst_subjects(ctx.h, None, 6, 2, _lib.ptr(xs), None, None, Smax, None, None, None) == -1 and works()
        bad_kw = (dict(draws_per_subject=3), dict(nstar=[1, 1]), dict(indx_star=np.zeros((3, 2), dtype=np.int32)))
        binding = lambda p, **kw: ctx.predict_hadst_subjects(p, xs, **{"draws_per_subject": 2, **kw})
    else:
        assert ctx.lib.nmgp_predsample_hads_subjects(None, None, 0, 0, None, None, None, None, 0, *([None] * 6)) == -1
        assert ctx.lib.nmgp_predsample_hads_subjects(ctx.h, None, 6, 2, None, _lib.ptr(xs), None, None, Smax, None, None, None, None, None,
                                                     None) == -1 and works()   # NMGP_E_NULL
        bad_kw = (dict(draws_per_subject=3), dict(nstar=[1, 1]), dict(indx_star=np.zeros((3, 2), dtype=np.int32)), dict(z=zz, star=zz),
                  dict(z=np.zeros((6, Smax, 3))))
        binding = lambda p, **kw: ctx.predsample_hads_subjects(p, HYPER["sep"], xs, **{"draws_per_subject": 2, **kw})
    for kw in bad_kw:                                                      # the binding raises before the call
        with pytest.raises(_lib.NmgpError):
            binding(pars, **kw)
    with pytest.raises(_lib.NmgpError):
        binding(pars[:, :-1])
    assert works()
    monkeypatch.setenv("NMGP_CHOL", "rocsolver")                           # read when a context is created
    other = _lib.Context(0)
    try:
        set_subjects(other, cases)
        assert raw_call(other, model, pars, 2, xs) == -4                   # NMGP_E_UNSUPPORTED
    finally:
        other.close()


# ---- 10. nothing else is disturbed -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_the_resident_subject_the_cohort_evaluations_and_the_nonseparable_predictor_are_undisturbed(ctx, model):
    from nonstationary_multivariate_gaussian_process_amd import hadamard
    cases = cc.SET_A
    set_subjects(ctx, cases)
    g = hc.build((63, 2, "blocks"))
    ctx.had_set_data(g["x"], g["indx"], g["y"])
    nobs = cc.nobs(cases)
    resident = getattr(ctx, mc.RESIDENT[model])

    def evaluations():
        out = [ctx.had_subjects_eval(cc.pack(cc.chains(cases, 2), nobs, 2), HYPER["had"], want_grad=True, chains_per_subject=2)]
        out += [getattr(ctx, mc.ENTRY[m])(mc.pack(m, mc.chains(m, cases, 2), nobs, 2), HYPER[m], want_grad=True, chains_per_subject=2)
                for m in MODELS]
        out.append(resident(g["pars"][model], HYPER[model], want_grad=True))
        return out

    xs, lab, _ = inputs(cases, "ix")
    zn = [np.random.default_rng(7 + s).standard_normal((2, v.shape[0], 4)) for s, v in enumerate(xs)]
    non = lambda ix: hadamard.cohort_predict(ctx, cc.chains(cases, 2), xs, HYPER["had"], indx_star=ix, z=zn)
    before, n1, n2 = evaluations(), non(None), non(lab)
    p1 = predict(ctx, model, cases, "full")
    assert all_same_bits(n1, non(None))                                    # interleaved on the same set
    p2 = predict(ctx, model, cases, "ix")
    assert all_same_bits(n2, non(lab))
    assert ctx.N == 63 and ctx.M == 2
    after = evaluations()
    assert all(r[2].tolist() == [0] * len(r[2]) for r in before) and all_same_bits(before, after)
    # ... and the set's cached prior factors served all of them: the predictions repeat bit for bit
    assert all_same_bits(p1, predict(ctx, model, cases, "full")) and all_same_bits(p2, predict(ctx, model, cases, "ix"))


# ---- 11. NMGP_POISON -----------------------------------------------------------------------------------------------------------------------------------
POISON_SNIPPET = r'''
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np
import hadamard_cases as hc
import hadamard_cohort_cases as cc
from nonstationary_multivariate_gaussian_process_amd import _lib, hadamard_sep, hadamard_sta
ctx = _lib.Context(0)
hyper = hc.hypers()["sep"]
n = 0
for cases in (cc.SET_D, cc.SET_A, cc.SET_E, cc.SET_F, cc.SET_G, cc.SET_H):
    subs = cc.subjects(cases)
    ctx.had_set_subjects([c["x"] for c in subs], [c["indx"] for c in subs], [c["y"] for c in subs], M=cases[0][1])
    xs, lab = [c["xs"] for c in subs], [c["lab"] for c in subs]
    z = [hc.normals(case, v.shape[0]) for case, v in zip(cases, xs)]
    sep, sta = [c["pars"]["sep"] for c in subs], [c["pars"]["sta"] for c in subs]
    for ix in (None, lab):
        first = hadamard_sep.cohort_predict(ctx, sep, xs, hyper, indx_star=ix, z=z)     # a fresh (or grown) workspace: poisoned
        other = hadamard_sta.cohort_predict(ctx, sta, xs, indx_star=ix)                 # the kept workspace: poisoned again
        again = hadamard_sep.cohort_predict(ctx, sep, xs, hyper, indx_star=ix, z=z)
        fed = hadamard_sep.cohort_predict(ctx, sep, xs, hyper, indx_star=ix, star=[r[2] for r in first])
        twice = hadamard_sta.cohort_predict(ctx, sta, xs, indx_star=ix)
        for a, b, c, d, e in zip(first, again, fed, other, twice):
            assert a[3].tolist() == d[2].tolist() == [0, 0] and all(np.all(np.isfinite(v)) for v in a[:3] + d[:2]), (cases, ix)
            assert all(np.array_equal(u, v) for u, v in zip(a, b)), (cases, ix)
            assert all(np.array_equal(u, v) for u, v in zip(a, c)), (cases, ix)
            assert all(np.array_equal(u, v) for u, v in zip(d, e)), (cases, ix)
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
    assert out.returncode == 0 and "POISON_OK 12" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


# ---- 12. the drivers -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_cohort_map_predict_is_cohort_predict_with_one_draw_and_no_noise(ctx, model):
    from nonstationary_multivariate_gaussian_process_amd import drivers
    cases = cc.SET_A
    subs = cc.subjects(cases)
    h = hyper_dict(HYPER[model], KEYS[model])
    init = [c["pars"][model][:1] for c in subs]
    xs, lab, _ = inputs(cases, "ix")
    triples = [(c["x"], c["indx"], c["y"]) for c in subs]
    Driver = {"sep": drivers.HadamardSepCohortMAP, "sta": drivers.HadamardStaCohortMAP}[model]
    one = Driver(triples, h, init, max_flop_waste=1e9, ctxs=[ctx])
    try:
        assert len(one.buckets) == 1
        order = [int(s) for s in one.buckets[0]]
        for ix in (None, lab):
            got = one.predict(init, xs, indx_star=ix)
            want = call(ctx, model, [init[s] for s in order], [xs[s] for s in order], None if ix is None else [ix[s] for s in order])
            for s, w in zip(order, want):                                  # the same set: bit for bit
                assert len(got[s]) == len(w) and got[s][-1] == 0 and same_bits(got[s][:-1], [a[0] for a in w[:-1]]), s
    finally:
        one.close()
    m = Driver(triples, h, init, max_flop_waste=0.5)                       # several sets: results come back in the caller's order
    try:
        assert len(m.buckets) > 1
        tol = {"sep": (PRED_TOL, PRED_TOL, STAR_TOL), "sta": (STA_PRED_TOL, STA_PRED_TOL)}[model]
        for ix in (None, lab):
            got = m.predict(init, xs, indx_star=ix)
            set_subjects(ctx, cases)
            want = call(ctx, model, init, xs, ix)
            for s, (g, w) in enumerate(zip(got, want)):
                assert g[-1] == 0 and w[-1].tolist() == [0]
                # (another set, another Nmax, hence another blocking: each side is within its bar of the restatement, so the two are
                # within twice the bar of each other)
                for u, v, t in zip(g[:-1], w[:-1], tol):
                    assert relerr(u, v[0]) < 2 * t, (model, s)
    finally:
        m.close()


@pytest.mark.parametrize("model", MODELS)
def test_cohort_posterior_driver_gives_each_subject_the_single_subject_drivers_band(ctx, model):
    from nonstationary_multivariate_gaussian_process_amd import drivers, hadamard
    cases = cc.SET_B                                                       # M = 8
    subs = cc.subjects(cases)
    h = hyper_dict(HYPER[model], KEYS[model])
    samples = [more_draws(model, c, 6).reshape(3, 2, -1) for c in cases]   # [iters, chains, P_s]
    xs, lab, _ = inputs(cases, "ix")
    triples = [(c["x"], c["indx"], c["y"]) for c in subs]
    cohort, single = {"sep": (drivers.posterior_predict_hadamard_sep_cohort, drivers.posterior_predict_hadamard_sep),
                      "sta": (drivers.posterior_predict_hadamard_sta_cohort, drivers.posterior_predict_hadamard_sta)}[model]
    # the parity bars as they are: every draw's mean and variance of the two drivers within eps of each other, relative, element by
    # element; the summaries over the draws get the bound that follows from that
    eps = PRED_TOL if model == "sep" else STA_PRED_TOL
    order = [int(s) for s in hadamard.cohort_buckets(cc.nobs(cases), 1e9)[0]]
    Nmax = max(cc.nobs(cases))
    for ix in (None, lab):
        a = cohort(triples, h, samples, xs, indx_star=ix, seed=4, max_flop_waste=1e9, ctxs=[ctx])
        # the driver's normals (z first, then the y* normals, from default_rng(seed + s)) and its one call on the one bucket
        zs, zys = {}, {}
        for s in order:
            rng = np.random.default_rng(4 + s)
            zs[s] = rng.standard_normal((6, xs[s].shape[0], 2)) if model == "sep" else None
            zys[s] = rng.standard_normal((6, xs[s].shape[0]) + (() if ix is not None else (8,)))
        pick = lambda v: None if v is None else [v[k] for k in order]
        set_subjects(ctx, [cases[k] for k in order])
        res = call(ctx, model, [samples[k].reshape(6, -1) for k in order], [xs[k] for k in order], pick(ix),
                   pick(zs) if model == "sep" else None)
        for s, r in zip(order, res):
            x, indx, y = triples[s]
            d, S = a[s], xs[s].shape[0]
            w = single(x, indx, y, h, samples[s], xs[s], indx_star=None if ix is None else ix[s], seed=4 + s, ctx=ctx)
            assert d["n_used"] == w["n_used"] == 6 and d["n_failed"] == 0 and d["mean"].shape == ((S, 8) if ix is None else (S,))
            assert sorted(d) == sorted(w)
            mean, var, zy = r[0], r[1], zys[s]
            np.testing.assert_allclose(d["mean"], mean.mean(axis=0), rtol=1e-13)
            np.testing.assert_allclose(d["var"], var.mean(axis=0) + mean.var(axis=0), rtol=1e-13)
            # mean of the draws' means m_h (1 + delta_h), |delta_h| <= eps: moves by at most eps times the mean of their magnitudes
            assert np.all(np.abs(d["mean"] - w["mean"]) <= eps * np.abs(mean).mean(axis=0)), (model, s)
            # total variance = mean_h v_h + var_h(m_h).  The first term moves by at most eps mean_h v_h.  With e_h = m_h delta_h,
            # var(m + e) - var(m) = 2 cov(m, e) + var(e), |cov(m, e)| <= std(m) std(e), std(e)^2 <= mean(e^2) <= eps^2 mean(m^2)
            rms = np.sqrt((mean ** 2).mean(axis=0))
            bound = eps * var.mean(axis=0) + 2.0 * eps * mean.std(axis=0) * rms + eps ** 2 * rms ** 2
            assert np.all(np.abs(d["var"] - w["var"]) <= bound), (model, s)
            # a percentile is a convex combination of order statistics, which move by at most the largest move of a sample
            # y*_h = m_h + sqrt(v_h) zy_h: at most eps |m_h| + eps |zy_h| sqrt(v_h) (the square root halves a relative error)
            scale = (np.abs(mean) + np.abs(zy) * np.sqrt(var)).max(axis=0)
            assert np.all(np.abs(d["quantiles"] - w["quantiles"]) <= eps * scale[None]), (model, s)
            assert relerr(d["tilde_l_star"], w["tilde_l_star"]) < STAR_TOL
            if model == "sep":
                assert relerr(d["tilde_sigma_star"], w["tilde_sigma_star"]) < STAR_TOL
        # a subject's rows: the same bits in the cohort and in a cohort of itself padded to the same Nmax
        for s in (1, 2):
            set_subjects(ctx, [cases[s]], Nmax=Nmax)
            alone = call(ctx, model, [samples[s].reshape(6, -1)], [xs[s]], None if ix is None else [ix[s]],
                         [zs[s]] if model == "sep" else None)[0]
            assert same_bits(alone, res[order.index(s)]), (model, s)
    # the default buckets on contexts of its own: every draw of every subject is used, in the caller's order
    b = cohort(triples, h, samples, xs, indx_star=lab, seed=4)
    assert [d["n_used"] for d in b] == [6, 6, 6] and [d["mean"].shape for d in b] == [(v.shape[0],) for v in xs]
