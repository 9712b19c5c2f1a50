"""MAP and posterior-draw prediction for a cohort of ragged Hadamard subjects on the GPU (nmgp_predsample_had_subjects,
hadamard.cohort_predict, drivers.HadamardCohortMAP.predict, drivers.posterior_predict_hadamard_cohort) against the NumPy restatement
tests/predsample_had_cases.restate_hpn on each subject ALONE (tests/test_predsample_had_cohort_cpu.py holds the padding argument and
the precondition of the bars), against the resident entry nmgp_predsample_had, and against itself across sets, batch, chunk and slice
sizes.

Bars: mean and variance 1e-5 relative element by element, starred values 1e-6 (tests/test_gpu_predsample_had.py's PRED_TOL /
STAR_TOL); indexed against full under the same starred values 1e-10 (its FORM_TOL); everything else bit for bit.  All shapes are
tests/hadamard_cohort_cases.SETS', the inputs each subject's own default grid (3, 5, 11 and 63 points: ragged within a set)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import hadamard_cases as hc
import hadamard_cohort_cases as cc
import predsample_had_cases as pc
from conftest import ROOT, SVC_KEYS, hyper_dict, record_parity, relerr

pytestmark = pytest.mark.gpu

PRED_TOL, STAR_TOL, FORM_TOL = 1e-5, 1e-6, 1e-10
HYPER = hc.hypers()["had"]


@pytest.fixture(scope="module")
def ctx():
    from nonstationary_multivariate_gaussian_process_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def same_bits(a, b):
    return all(np.array_equal(u, v, equal_nan=True) for u, v in zip(a, b))


def all_same_bits(res_a, res_b):
    return len(res_a) == len(res_b) and all(same_bits(a, b) for a, b in zip(res_a, res_b))


def set_subjects(ctx, cases, Nmax=None):
    subs = cc.subjects(cases)
    ctx.had_set_subjects([c["x"] for c in subs], [c["indx"] for c in subs], [c["y"] for c in subs], M=cases[0][1], Nmax=Nmax)


def grid_kw(case, form):
    """the grid of a subject in a form: its default one, but the slice wider than 256 riding rows for hc.WIDE"""
    if case == pc.WIDE:
        return pc.WIDE_FULL if form == "full" else pc.WIDE_INDEXED
    return {}


def expected(case, form):
    return pc.expected(case, **grid_kw(case, form))


def more_draws(case, H):
    """H draws on the segment through the subject's two (and beyond it): smooth, distinct, all factorable."""
    d = pc.subject(case)["draws"]
    return np.stack([d[0] + 0.5 * k * (d[1] - d[0]) for k in range(H)])


def inputs(cases, form="full", S=None):
    """per-subject (xs, labels or None, z [2, S_s, 1+T]) lists; S: one grid size for every subject instead of the default grids"""
    xs, lab, z = [], [], []
    for case in cases:
        if S is None:
            e = expected(case, form)
            xs.append(e["xs"]), lab.append(e["lab"]), z.append(e["z"])
        else:
            x_, l_ = pc.new_inputs(case, S)
            xs.append(x_), lab.append(l_), z.append(pc.normals(case, S))
    return xs, (lab if form == "ix" else None), z


def predict(ctx, cases, form="full", S=None, draws=None, z="fixed", star=None):
    from nonstationary_multivariate_gaussian_process_amd import hadamard
    xs, lab, zz = inputs(cases, form, S)
    draws = [pc.subject(c)["draws"] for c in cases] if draws is None else draws
    return hadamard.cohort_predict(ctx, draws, xs, HYPER, indx_star=lab, z=zz if z == "fixed" else z, star=star)


# ---- 1. parity with the restatement on each subject alone ------------------------------------------------------------------------------
PARITY_SETS = {"A": cc.SET_A, "B": cc.SET_B, "C": [c for c in cc.SET_C if c != hc.MINOR], "D": cc.SET_D, "E": cc.SET_E,
               "F": cc.SET_F, "G": cc.SET_G, "H": cc.SET_H, "I": cc.SET_I}      # F - H: k_hadc_cross_rows<4, 6, 7>; I: Nmax = 1030


@pytest.mark.parametrize("name", sorted(PARITY_SETS))
def test_two_draws_per_subject_meet_the_restatement_on_the_subject_alone(ctx, name):
    cases = PARITY_SETS[name]
    if name == "A":
        assert cc.nobs(cases) == [128, 63, 2, 64, 65, 127]
        assert sorted({expected(c, "full")["xs"].shape[0] for c in cases}) == [3, 11, 63]
    set_subjects(ctx, cases)
    worst = {}
    for form in ("full", "ix"):
        res = predict(ctx, cases, form)
        for case, (mean, var, star, status) in zip(cases, res):
            c, e = pc.subject(case), expected(case, form)
            S = e["xs"].shape[0]
            floor = pc.raw_variance_floor({form: e[form]}, case)
            assert status.tolist() == [0, 0] and star.shape == (2, S, 1 + c["T"])
            assert mean.shape == var.shape == ((2, S, c["M"]) if form == "full" else (2, S))
            rm, rv, rs = e[form]
            errs = {"mean": relerr(mean, rm), "var": relerr(var, rv), "star": relerr(star, rs)}
            tag = "hpcohort/%s/%s/%s" % (name, form, hc.case_id(case))
            print(tag, "raw variance / sigma2_err >=", floor, errs)
            record_parity(tag, **{k: (v, STAR_TOL if k == "star" else PRED_TOL) for k, v in errs.items()})
            for k, v in errs.items():
                worst[form + "_" + k] = max(worst.get(form + "_" + k, 0.0), v)
            assert floor > 1.0, (tag, floor)
            for k, v in errs.items():
                assert v < (STAR_TOL if k == "star" else PRED_TOL), (tag, k, v)
    print("hpcohort/%s worst" % name, worst)


# ---- 2. padded slots ---------------------------------------------------------------------------------------------------------------------
def padded_call(ctx, cases, form, fill, lab_fill, star=None, nstar=None, poison_set=False, use_z=True):
    """the entry on padded arrays whose padded slots hold `fill` (labels: `lab_fill`), the set's own pads included"""
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
    z2 = hadamard.cohort_pack_inputs([v[:, :n] for v, n in zip(z, ns)], Smax=Smax, fill=fill)[0] if use_z and star is None else None
    s2 = None
    if star is not None:
        s2 = star.copy()
        for s, n in enumerate(ns):
            s2[2 * s:2 * s + 2, n:] = fill
    pars = cc.pack(cc.chains(cases, 2), nobs, M, fill=fill)
    return ctx.predsample_had_subjects(pars, HYPER, xs2, indx_star=l2, nstar=ns, draws_per_subject=2, z=z2, star=s2), ns, Smax


@pytest.mark.parametrize("form", ["full", "ix"])
def test_poisoned_padded_slots_change_no_bit_and_padded_outputs_are_plus_zero(ctx, form):
    cases = cc.SET_A
    clean, ns, Smax = padded_call(ctx, cases, form, 0.0, 0)
    assert clean[3].tolist() == [0] * 12 and Smax == 63 and min(ns) == 3
    dirty, _, _ = padded_call(ctx, cases, form, np.nan, 99, poison_set=True)
    assert same_bits(clean, dirty)
    fed_clean, _, _ = padded_call(ctx, cases, form, 0.0, 0, star=clean[2])
    fed_dirty, _, _ = padded_call(ctx, cases, form, np.nan, 99, star=clean[2], poison_set=True)
    assert same_bits(fed_clean, fed_dirty) and same_bits(fed_clean, clean)
    for s, n in enumerate(ns):
        for a in dirty[:3] + fed_dirty[:3]:
            pad, real = a[2 * s:2 * s + 2, n:], a[2 * s:2 * s + 2, :n]
            assert np.all(pad == 0.0) and not np.any(np.signbit(pad)) and np.all(np.isfinite(real))
    # a patient with nothing to predict: all-zero rows, status 0; the others keep their bits
    ns0 = list(ns)
    ns0[1] = 0
    zero, _, _ = padded_call(ctx, cases, form, np.nan, 99, nstar=ns0, poison_set=True)
    assert zero[3].tolist() == [0] * 12
    for a, b in zip(zero[:3], clean[:3]):
        assert np.all(a[2:4] == 0.0) and not np.any(np.signbit(a[2:4]))
        keep = np.r_[0:2, 4:12]
        assert np.array_equal(a[keep], b[keep])


# ---- 3. bits -------------------------------------------------------------------------------------------------------------------------------
def test_a_subject_alone_in_a_set_of_one_gives_the_bits_of_its_rows_in_the_set(ctx):
    cases = cc.SET_A
    for form in ("full", "ix"):
        set_subjects(ctx, cases)
        full = predict(ctx, cases, form)
        for s in (0, 1, 2, 4):                                             # N_s = Nmax, a mask inside a tile, N_s = M, one past an edge
            set_subjects(ctx, [cases[s]], Nmax=128)
            one = predict(ctx, [cases[s]], form)
            assert one[0][3].tolist() == [0, 0] and same_bits(one[0], full[s]), (form, s)


def test_five_draws_per_subject_give_the_bits_of_five_calls_whatever_the_chunking(ctx, monkeypatch):
    monkeypatch.delenv("NMGP_PREDSAMPLE_CHUNK", raising=False)
    cases = cc.SET_A
    set_subjects(ctx, cases)
    draws = [more_draws(c, 5) for c in cases]
    for form in ("full", "ix"):
        xs, _, _ = inputs(cases, form)
        T = pc.subject(cases[0])["T"]
        z = [np.random.default_rng(12 + s).standard_normal((5, v.shape[0], 1 + T)) for s, v in enumerate(xs)]
        big = predict(ctx, cases, form, draws=draws, z=z)
        assert all(r[3].tolist() == [0] * 5 for r in big) and not np.array_equal(big[0][0][0], big[0][0][1])
        for k in range(5):
            one = predict(ctx, cases, form, draws=[d[k:k + 1] for d in draws], z=[v[k:k + 1] for v in z])
            assert all_same_bits([[a[k:k + 1] for a in r] for r in big], one), (form, k)
        monkeypatch.setenv("NMGP_PREDSAMPLE_CHUNK", "2")                  # parts of ONE subject's draws: 2, 2 and 1
        split = predict(ctx, cases, form, draws=draws, z=z)
        two = predict(ctx, cases, form, draws=[d[:2] for d in draws], z=[v[:2] for v in z])        # one whole subject per chunk
        monkeypatch.setenv("NMGP_PREDSAMPLE_CHUNK", "4")                  # two whole subjects per chunk
        four = predict(ctx, cases, form, draws=[d[:2] for d in draws], z=[v[:2] for v in z])
        monkeypatch.delenv("NMGP_PREDSAMPLE_CHUNK")
        assert all_same_bits(big, split)
        assert all_same_bits([[a[:2] for a in r] for r in big], two) and all_same_bits(two, four)


def test_a_grid_point_moved_to_another_slice_keeps_its_bits(ctx):
    from nonstationary_multivariate_gaussian_process_amd import hadamard
    cases = cc.SET_E                                                       # Nmax = 64, M = 5: full-form slices of 12 inputs
    set_subjects(ctx, cases)
    sizes = (30, 17)                                                       # 12 + 12 + 6 and 12 + 5 inputs
    xs = [pc.new_inputs(c, S)[0] for c, S in zip(cases, sizes)]
    z = [pc.normals(c, S) for c, S in zip(cases, sizes)]
    draws = [pc.subject(c)["draws"] for c in cases]
    a = hadamard.cohort_predict(ctx, draws, xs, HYPER, z=z)
    rev = [np.arange(S)[::-1] for S in sizes]
    b = hadamard.cohort_predict(ctx, draws, [v[r].copy() for v, r in zip(xs, rev)], HYPER,
                                z=[np.ascontiguousarray(v[:, r]) for v, r in zip(z, rev)])
    for ra, rb, r in zip(a, b, rev):
        assert ra[3].tolist() == rb[3].tolist() == [0, 0] and same_bits([v[:, r] for v in rb[:3]], ra[:3])
    head = hadamard.cohort_predict(ctx, draws, [v[:7].copy() for v in xs], HYPER, z=[np.ascontiguousarray(v[:, :7]) for v in z])
    for ra, rh in zip(a, head):
        assert same_bits(rh[:3], [v[:, :7] for v in ra[:3]])


def test_indexed_form_is_the_labelled_column_of_the_full_form(ctx):
    cases = cc.SET_A
    set_subjects(ctx, cases)
    full = predict(ctx, cases, "full")
    ix = predict(ctx, cases, "ix", z=None, star=[r[2] for r in full])
    _, lab, _ = inputs(cases, "ix")
    e_m = e_v = 0.0
    for (mean, var, star, status), (im, iv, istar, ist), l in zip(full, ix, lab):
        S = l.shape[0]
        assert status.tolist() == ist.tolist() == [0, 0] and np.array_equal(istar, star) and im.shape == iv.shape == (2, S)
        e_m = max(e_m, relerr(im, mean[:, np.arange(S), l]))
        e_v = max(e_v, relerr(iv, var[:, np.arange(S), l]))
    print("indexed against full: mean", e_m, "var", e_v)
    record_parity("hpcohort/A/indexed_vs_full", mean=(e_m, FORM_TOL), var=(e_v, FORM_TOL))
    assert e_m < FORM_TOL and e_v < FORM_TOL


# ---- 4. against the resident entry ------------------------------------------------------------------------------------------------------------
def test_unpadded_subjects_give_the_resident_entry_its_bits(ctx):
    cases = cc.SET_E
    assert cc.nobs(cases) == [64, 64]
    for form in ("full", "ix"):
        set_subjects(ctx, cases)
        xs, lab, z = inputs(cases, form)
        assert len({v.shape[0] for v in xs}) == 1                          # equal grids: nstar = Smax
        reg = predict(ctx, cases, form)
        fed = predict(ctx, cases, form, z=None, star=[r[2] for r in reg])
        d = 0.0
        for s, case in enumerate(cases):
            c = pc.subject(case)
            ctx.had_set_data(c["x"], c["indx"], c["y"])
            l = None if lab is None else lab[s]
            r_fed = ctx.predsample_had(c["draws"], HYPER, xs[s], indx_star=l, star=reg[s][2])
            r_reg = ctx.predsample_had(c["draws"], HYPER, xs[s], indx_star=l, z=z[s])
            assert r_fed[3].tolist() == fed[s][3].tolist() == [0, 0]
            # under the same starred values: bit for bit
            assert np.array_equal(fed[s][0], r_fed[0]) and np.array_equal(fed[s][1], r_fed[1]) and np.array_equal(fed[s][2], r_fed[2])
            assert same_bits(fed[s][:2], reg[s][:2])
            # with the regression on, the prior factors come from two factorisation calls: the distance is recorded
            d = max(d, relerr(reg[s][2], r_reg[2]))
            print("set E", form, hc.case_id(case), "star vs resident", relerr(reg[s][2], r_reg[2]), "bit-identical",
                  np.array_equal(reg[s][2], r_reg[2]), "mean", relerr(reg[s][0], r_reg[0]), "var", relerr(reg[s][1], r_reg[1]))
        record_parity("hpcohort/E/%s/vs_resident" % form, star=(d, STAR_TOL))
        assert d < STAR_TOL


# ---- 5. failure stays local ----------------------------------------------------------------------------------------------------------------------
def test_status_of_a_bad_draw_and_every_other_subject(ctx, monkeypatch):
    from nonstationary_multivariate_gaussian_process_amd import _lib, hadamard
    monkeypatch.delenv("NMGP_PREDSAMPLE_CHUNK", raising=False)
    cases = cc.SET_C
    k = cases.index(hc.MINOR)
    others = [c for c in cases if c != hc.MINOR]
    xs = [pc.new_inputs(c)[0] for c in cases]                              # short grids for all
    T = pc.subject(cases[0])["T"]
    z = [np.random.default_rng(65 + s).standard_normal((3, v.shape[0], 1 + T)) for s, v in enumerate(xs)]
    lab = [hc.grid_labels(v.shape[0], 3, 2) for v in xs]
    P = hc.minor_chains("had")
    nan = P[[0, 2, 0]].copy()
    nan[1, 40] = np.nan
    keep = [s for s in range(len(cases)) if s != k]
    for ix in (None, lab):
        for bad, want in ((P, 3), (nan, _lib.NUM_NAN)):
            draws = [bad if c == hc.MINOR else more_draws(c, 3) for c in cases]
            set_subjects(ctx, cases)
            res = hadamard.cohort_predict(ctx, draws, xs, HYPER, indx_star=ix, z=z)
            print("cohort_predict", "indexed" if ix is not None else "full", "status", [r[3].tolist() for r in res])
            assert res[k][3].tolist() == [0, want, 0]
            assert np.all(np.isnan(res[k][0][1])) and np.all(np.isnan(res[k][1][1]))
            assert np.all(np.isfinite(res[k][0][[0, 2]])) and np.all(np.isfinite(res[k][1][[0, 2]]))
            set_subjects(ctx, others, Nmax=max(cc.nobs(cases)))
            clean = hadamard.cohort_predict(ctx, [draws[s] for s in keep], [xs[s] for s in keep], HYPER,
                                            indx_star=None if ix is None else [ix[s] for s in keep], z=[z[s] for s in keep])
            assert all(r[3].tolist() == [0, 0, 0] for r in clean)
            assert all_same_bits([res[s] for s in keep], clean)


# ---- 6. arguments and state ------------------------------------------------------------------------------------------------------------------------
def raw_call(ctx, pars, H, xs, lab=None, nstar=None, Smax=None, z=None, star=None, per=None):
    """the C entry as it is: its return code"""
    from nonstationary_multivariate_gaussian_process_amd import _lib
    ptr, ip = _lib.ptr, ctypes.POINTER(ctypes.c_int)
    B = pars.shape[0]
    Smax = xs.shape[1] if Smax is None else Smax
    out = np.empty((B, max(Smax, 1), 8)), np.empty((B, max(Smax, 1), 8)), np.empty((B, max(Smax, 1), 40))
    status = np.zeros(B, dtype=np.int32)
    hy = _lib.as_f64(HYPER)
    lab = None if lab is None else np.ascontiguousarray(lab, dtype=np.int32)
    nstar = None if nstar is None else np.ascontiguousarray(nstar, dtype=np.int32)
    return ctx.lib.nmgp_predsample_had_subjects(ctx.h, ptr(pars), B, H, ptr(hy), ptr(xs), None if lab is None else lab.ctypes.data_as(ip),
                                                None if nstar is None else nstar.ctypes.data_as(ip), Smax, ptr(z), ptr(star),
                                                ptr(out[0]), ptr(out[1]), ptr(out[2]), status.ctypes.data_as(ip))


def test_argument_and_state_checks(ctx, monkeypatch):
    from nonstationary_multivariate_gaussian_process_amd import _lib, hadamard
    cases = cc.SET_D                                                       # M = 1, nobs 1 / 2 / 70
    nobs, M = cc.nobs(cases), 1
    pars = cc.pack(cc.chains(cases, 2), nobs, M)
    xs = hadamard.cohort_pack_inputs([pc.new_inputs(c)[0] for c in cases])[0]
    Smax = xs.shape[1]
    zz = np.zeros((6, Smax, 2))
    ctx.had_clear_subjects()
    assert raw_call(ctx, pars, 2, xs) == -3                                # NMGP_E_STATE: no set
    with pytest.raises(_lib.NmgpError):
        hadamard.cohort_predict(ctx, cc.chains(cases, 2), [pc.new_inputs(c)[0] for c in cases], HYPER)
    set_subjects(ctx, cases)

    def works():
        r = predict(ctx, cases, "full")
        return all(v[3].tolist() == [0, 0] for v in r)

    assert works()
    assert raw_call(ctx, pars, 2, xs, z=zz, star=zz) == -3 and works()    # NMGP_E_STATE: z with star_in
    assert raw_call(ctx, pars[:5], 2, xs) == -2 and works()                # NMGP_E_SHAPE: B != S * draws_per_subject
    assert raw_call(ctx, pars, 3, xs) == -2 and works()
    assert raw_call(ctx, pars, 0, xs) == -2 and works()                    # draws_per_subject < 1
    assert raw_call(ctx, pars, 2, xs, Smax=0) == -2 and works()            # Smax < 1
    for bad in ([Smax + 1, 1, 1], [1, -1, 1]):                             # nstar outside [0, Smax]
        assert raw_call(ctx, pars, 2, xs, nstar=bad) == -2 and works()
    lab = np.zeros(xs.shape, dtype=np.int32)
    for v in (1, -1):                                                      # a real label outside [0, M)
        lab[1, 2] = v
        assert raw_call(ctx, pars, 2, xs, lab=lab, nstar=[3, 3, 3]) == -2 and works()
        assert raw_call(ctx, pars, 2, xs, lab=lab, nstar=[3, 2, 3]) == 0   # ... in a padded slot it is not read
    assert ctx.lib.nmgp_predsample_had_subjects(None, None, 0, 0, None, None, None, None, 0, *([None] * 6)) == -1
    assert ctx.lib.nmgp_predsample_had_subjects(ctx.h, None, 6, 2, None, _lib.ptr(xs), None, None, Smax, None, None, None, None, None,
                                                None) == -1 and works()   # NMGP_E_NULL
    # the binding raises before the call
    for kw in (dict(draws_per_subject=3), dict(nstar=[1, 1]), dict(indx_star=np.zeros((3, 2), dtype=np.int32)), dict(z=zz, star=zz),
               dict(z=np.zeros((6, Smax, 3)))):
        with pytest.raises(_lib.NmgpError):
            ctx.predsample_had_subjects(pars, HYPER, xs, **{"draws_per_subject": 2, **kw})
    with pytest.raises(_lib.NmgpError):
        ctx.predsample_had_subjects(pars[:, :-1], HYPER, xs, draws_per_subject=2)
    assert works()
    monkeypatch.setenv("NMGP_CHOL", "rocsolver")                           # read when a context is created
    other = _lib.Context(0)
    try:
        set_subjects(other, cases)
        assert raw_call(other, pars, 2, xs) == -4                          # NMGP_E_UNSUPPORTED
    finally:
        other.close()


def test_the_resident_subject_and_the_cohort_evaluation_are_unchanged_by_a_prediction_in_between(ctx):
    cases = cc.SET_A
    set_subjects(ctx, cases)
    g = pc.subject("had_N77_M3")
    ctx.had_set_data(g["x"], g["indx"], g["y"])
    P = cc.pack(cc.chains(cases, 2), cc.nobs(cases), 2)
    before = ctx.had_subjects_eval(P, HYPER, want_grad=True, chains_per_subject=2)
    res_before = ctx.had_batch_eval(g["draws"], g["hyper"], want_grad=True)
    p1 = predict(ctx, cases, "full")
    p2 = predict(ctx, cases, "ix")
    assert ctx.N == 77 and ctx.M == 3
    after = ctx.had_subjects_eval(P, HYPER, want_grad=True, chains_per_subject=2)
    res_after = ctx.had_batch_eval(g["draws"], g["hyper"], want_grad=True)
    assert before[2].tolist() == [0] * 12 and same_bits(before, after) and same_bits(res_before, res_after)
    # ... and the set's cached prior factors served both: the predictions repeat bit for bit
    assert all_same_bits(p1, predict(ctx, cases, "full")) and all_same_bits(p2, predict(ctx, cases, "ix"))


# ---- 7. NMGP_POISON ---------------------------------------------------------------------------------------------------------------------------------
POISON_SNIPPET = r'''
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np
import hadamard_cases as hc
import hadamard_cohort_cases as cc
import predsample_had_cases as pc
from nonstationary_multivariate_gaussian_process_amd import _lib, hadamard
ctx = _lib.Context(0)
hyper = hc.hypers()["had"]
n = 0
for cases in (cc.SET_D, cc.SET_A, cc.SET_E, cc.SET_F, cc.SET_G, cc.SET_H):
    subs = cc.subjects(cases)
    ctx.had_set_subjects([c["x"] for c in subs], [c["indx"] for c in subs], [c["y"] for c in subs], M=cases[0][1])
    draws = [pc.subject(c)["draws"] for c in cases]
    e = [pc.expected(c, indexed_only=True) for c in cases]
    xs, lab, z = [v["xs"] for v in e], [v["lab"] for v in e], [v["z"] for v in e]
    for ix in (None, lab):
        first = hadamard.cohort_predict(ctx, draws, xs, hyper, indx_star=ix, z=z)       # a fresh (or grown) workspace: poisoned
        again = hadamard.cohort_predict(ctx, draws, xs, hyper, indx_star=ix, z=z)       # the kept workspace: poisoned again
        fed = hadamard.cohort_predict(ctx, draws, xs, hyper, indx_star=ix, star=[r[2] for r in first])
        for a, b, c in zip(first, again, fed):
            assert a[3].tolist() == [0, 0] and all(np.all(np.isfinite(v)) for v in a[:3]), (cases, ix)
            assert all(np.array_equal(u, v) for u, v in zip(a, b)), (cases, ix)
            assert all(np.array_equal(u, v) for u, v in zip(a, c)), (cases, ix)
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


# ---- 8. the drivers ------------------------------------------------------------------------------------------------------------------------------------
def test_cohort_map_predict_is_cohort_predict_with_one_draw_and_no_noise(ctx):
    from nonstationary_multivariate_gaussian_process_amd import drivers, hadamard
    cases = cc.SET_A
    subs = cc.subjects(cases)
    h = hyper_dict(HYPER, SVC_KEYS)
    init = [c["pars"]["had"][:1] for c in subs]
    xs, lab, _ = inputs(cases, "ix")
    m = drivers.HadamardCohortMAP([(c["x"], c["indx"], c["y"]) for c in subs], h, init, max_flop_waste=0.5)
    try:
        assert len(m.buckets) > 1                                          # several sets: results come back in the caller's order
        for ix in (None, lab):
            got = m.predict(init, xs, indx_star=ix)
            set_subjects(ctx, cases)
            want = hadamard.cohort_predict(ctx, init, xs, HYPER, indx_star=ix)
            for s, (g, w) in enumerate(zip(got, want)):
                assert g[3] == 0 and w[3].tolist() == [0]
                # (another set, another Nmax, hence another blocking: each side is within its bar of the restatement, so the two are
                # within twice the bar of each other)
                assert relerr(g[0], w[0][0]) < 2 * PRED_TOL and relerr(g[1], w[1][0]) < 2 * PRED_TOL, s
                assert relerr(g[2], w[2][0]) < 2 * STAR_TOL, s
        one = drivers.HadamardCohortMAP([(c["x"], c["indx"], c["y"]) for c in subs], h, init, max_flop_waste=1e9, ctxs=[ctx])
        assert len(one.buckets) == 1
        order = [int(s) for s in one.buckets[0]]
        got = one.predict(init, xs, indx_star=lab)
        want = hadamard.cohort_predict(ctx, [init[s] for s in order], [xs[s] for s in order], HYPER, indx_star=[lab[s] for s in order])
        for s, w in zip(order, want):
            assert same_bits(got[s][:3], [w[0][0], w[1][0], w[2][0]]) and got[s][3] == 0       # the same set: bit for bit
        one.close()
    finally:
        m.close()


def test_cohort_driver_summarises_six_draws_per_subject_in_both_forms(ctx):
    from nonstationary_multivariate_gaussian_process_amd import drivers, hadamard
    cases = cc.SET_B                                                       # M = 8
    subs = cc.subjects(cases)
    h = hyper_dict(HYPER, SVC_KEYS)
    M, T = 8, 36
    samples = [more_draws(c, 6).reshape(3, 2, -1) for c in cases]          # [iters, chains, P_s]
    xs, lab, _ = inputs(cases, "ix")
    triples = [(c["x"], c["indx"], c["y"]) for c in subs]
    for ix in (None, lab):
        a = drivers.posterior_predict_hadamard_cohort(triples, h, samples, xs, indx_star=ix, seed=4, max_flop_waste=1e9, ctxs=[ctx])
        order = [int(s) for s in hadamard.cohort_buckets(cc.nobs(cases), 1e9)[0]]
        set_subjects(ctx, [cases[s] for s in order])
        z = {s: np.random.default_rng(4 + s).standard_normal((6, xs[s].shape[0], 1 + T)) for s in order}
        res = hadamard.cohort_predict(ctx, [samples[s].reshape(6, -1) for s in order], [xs[s] for s in order], HYPER,
                                      indx_star=None if ix is None else [ix[s] for s in order], z=[z[s] for s in order])
        for s, (mean, var, star, status) in zip(order, res):
            S, d = xs[s].shape[0], a[s]
            shape = (S, M) if ix is None else (S,)
            assert d["n_used"] == 6 and d["n_failed"] == 0 and d["mean"].shape == d["var"].shape == shape
            assert d["quantiles"].shape == (3,) + shape and d["tilde_l_star"].shape == (6, S)
            assert d["L_star"].shape == (6, S, T) and d["corr_quantiles"].shape == (3, S, M, M)
            np.testing.assert_allclose(d["mean"], mean.mean(axis=0), rtol=1e-13)
            np.testing.assert_allclose(d["var"], var.mean(axis=0) + mean.var(axis=0), rtol=1e-13)
            assert np.all(d["var"] >= var.mean(axis=0)) and np.array_equal(d["L_star"], star[:, :, 1:])
            np.testing.assert_allclose(np.einsum("qsmm->qsm", d["corr_quantiles"]), 1.0, rtol=0, atol=1e-14)
            assert np.all(np.abs(d["corr_quantiles"]) <= 1.0 + 1e-14)
    # the default buckets on contexts of its own: every draw of every subject is used, in the caller's order
    b = drivers.posterior_predict_hadamard_cohort(triples, h, samples, xs, indx_star=lab, seed=4)
    assert [d["n_used"] for d in b] == [6, 6, 6] and [d["mean"].shape for d in b] == [(v.shape[0],) for v in xs]
