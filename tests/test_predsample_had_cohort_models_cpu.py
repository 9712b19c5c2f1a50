"""CPU-only half of the cohort prediction tests of the separable and the stationary Hadamard model (nmgp_predsample_hads_subjects,
nmgp_predict_hadst_subjects; the GPU half is tests/test_gpu_predsample_had_cohort_models.py):

1. the precondition of the GPU half's bars: for every subject of sets A - E but hadamard_cases.MINOR, both models and both forms, the
   restatement's variance before the clip exceeds that chain's sigma2_err, so the clip to 1e-6 plays no part in any comparison;
2. the padding argument on the restatements: restate_hps (tests/test_predsample_hadamard_cpu.py) and hsta_moments
   (tests/test_hadamard_sta_cpu.py), unchanged, run on a subject PADDED in NumPy with decoupled unit observations (identity rows /
   columns in the covariance and in both GP-prior covariances, y = 0, zero cross-covariance rows, the padded parameter layout) give the
   subject-alone moments;
3. the surface: header, exported symbols, ctypes table, the four Python layers, and the pack / unpack helpers with width-2 starred
   arrays."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import hadamard_cases as hc
import hadamard_cohort_cases as cc
from conftest import ROOT, relerr
from oracle import nmgp_oracle as oracle

HEADER = os.path.join(ROOT, "include", "nmgp.h")
SEP, STA = "nmgp_predsample_hads_subjects", "nmgp_predict_hadst_subjects"
_D, _I = r"\s*const\s+double\s*\*\s*", r"\s*const\s+int\s*\*\s*"
DECL = {
    SEP: (r"int\s+" + SEP + r"\s*\(\s*nmgp_ctx\s*\*\s*\w*,\s*const\s+double\s*\*\s*pars,\s*int\s+B,\s*int\s+draws_per_subject,"
          r"\s*const\s+double\s+hyper\[9\]," + _D + r"xs," + _I + r"indx_star," + _I + r"nstar,\s*int\s+Smax," + _D + r"z," + _D +
          r"star_in,\s*double\s*\*\s*mean,\s*double\s*\*\s*var,\s*double\s*\*\s*star_out,\s*int\s*\*\s*status\s*\)\s*;"),
    STA: (r"int\s+" + STA + r"\s*\(\s*nmgp_ctx\s*\*\s*\w*,\s*const\s+double\s*\*\s*pars,\s*int\s+B,\s*int\s+draws_per_subject," + _D +
          r"xs," + _I + r"indx_star," + _I + r"nstar,\s*int\s+Smax,\s*double\s*\*\s*mean,\s*double\s*\*\s*var,\s*int\s*\*\s*status\s*\)\s*;"),
}


# ---- 1. the precondition of the bars --------------------------------------------------------------------------------------------------
def compared(case):
    """the restatements the GPU half compares a subject against: {form: predictions}"""
    if case == hc.WIDE:
        return {"full": hc.predictions(case, **hc.WIDE_FULL), "ix": hc.predictions(case, **hc.WIDE_INDEXED)}
    p = hc.predictions(case)
    return {"full": p, "ix": p}


def variance_floors(case):
    """{(model, form): min over the two chains and every compared output of (variance before the clip / sigma2_err of the chain)}"""
    c = hc.build(case)
    s2 = {m: np.exp(c["pars"][m][:, -1]) for m in ("sep", "sta")}
    out = {}
    for form, p in compared(case).items():
        sta = p["sta_full" if form == "full" else "sta_ix"]
        out["sta", form] = min(float(np.min(sta[k][1])) / s2["sta"][k] for k in (0, 1))
        # restate_hps returns the clipped scale: its square exceeds sigma2_err exactly when the variance before the clip does
        scale = p["hps_full" if form == "full" else "hps_ix"][1]
        out["sep", form] = min(float(np.min(scale[:, k, 2:] ** 2)) / s2["sep"][k] for k in (0, 1))
    return out


@pytest.mark.parametrize("name", sorted(cc.SETS))
def test_every_compared_variance_before_the_clip_exceeds_its_noise_floor(name):
    for case in cc.SETS[name]:
        if case == hc.MINOR:
            continue
        for key, floor in variance_floors(case).items():
            print(name, hc.case_id(case), key, "variance before the clip / sigma2_err >=", floor)
            assert floor > 1.0, (case, key, floor)


# ---- 2. the restatements on a padded subject --------------------------------------------------------------------------------------------
def padded_data(c, Nmax):
    pad = Nmax - c["N"]
    return (np.concatenate([c["x"], np.zeros(pad)]), np.concatenate([c["indx"], np.zeros(pad, dtype=c["indx"].dtype)]),
            np.concatenate([c["y"], np.zeros(pad)]))


def sep_padded(monkeypatch, c, Nmax, xs, z, lab):
    """restate_hps, unchanged, on the subject c padded to Nmax: the pieces it builds its matrices from are wrapped so that the padded
    observations are decoupled unit observations, as the device pads them."""
    import test_predsample_hadamard_cpu as tph
    from nonstationary_multivariate_gaussian_process_amd import hadamard_sep
    n = c["N"]
    rbf, gibbs, chol = tph.rbf, tph.gibbs, tph.cholesky

    def rbf_padded(x1, x2, alpha, beta):
        if x1.shape[0] != Nmax:
            return rbf(x1, x2, alpha, beta)
        if x2 is x1:                                                       # the prior covariance: identity block once the jitter is on
            out = (1.0 - tph.JITTER) * np.eye(Nmax)
            out[:n, :n] = rbf(x1[:n], x1[:n], alpha, beta)
            return out
        out = np.zeros((Nmax, x2.shape[0]))                                # zero right-hand sides
        out[:n] = rbf(x1[:n], x2, alpha, beta)
        return out

    def gibbs_padded(x1, s1, l1, x2, s2, l2):
        if x1.shape[0] != Nmax:
            return gibbs(x1, s1, l1, x2, s2, l2)
        if x2 is x1:
            out = np.zeros((Nmax, Nmax))
            out[:n, :n] = gibbs(x1[:n], s1[:n], l1[:n], x1[:n], s1[:n], l1[:n])
            return out
        out = np.zeros((Nmax, x2.shape[0]))                                # zero cross rows
        out[:n] = gibbs(x1[:n], s1[:n], l1[:n], x2, s2, l2)
        return out

    def chol_padded(A, lower=True):
        if A.shape[0] == Nmax:                                             # the padded part of the covariance: the identity
            A = A.copy()
            A[n:, :] = 0.0
            A[:, n:] = 0.0
            A[np.arange(n, Nmax), np.arange(n, Nmax)] = 1.0
        return chol(A, lower=lower)

    monkeypatch.setattr(tph, "rbf", rbf_padded)
    monkeypatch.setattr(tph, "gibbs", gibbs_padded)
    monkeypatch.setattr(tph, "cholesky", chol_padded)
    x, indx, y = padded_data(c, Nmax)
    draws = hadamard_sep.cohort_pack([c["pars"]["sep"]], [n], c["M"], Nmax=Nmax)
    try:
        return tph.restate_hps(x, indx, y, draws, c["hyper"]["sep"], xs, z, lab)[:2]
    finally:
        monkeypatch.undo()


def sta_padded(monkeypatch, c, Nmax, xs, lab, k):
    """hsta_moments, unchanged, on the padded subject: identity block in the covariance, zero cross rows"""
    import test_hadamard_sta_cpu as tst
    n = c["N"]
    rbf, cov = oracle.RBF_cov, tst.hsta_covariance

    def rbf_padded(X1, X2=None, alpha=1.0, beta=1.0):
        if X1.shape[0] != Nmax or X2 is None:
            return rbf(X1, X2, alpha=alpha, beta=beta)
        out = np.zeros((Nmax, np.asarray(X2).shape[0]))
        out[:n] = rbf(X1[:n], X2, alpha=alpha, beta=beta)
        return out

    def cov_padded(pars, x, indx, M):
        out = np.eye(Nmax)
        out[:n, :n] = cov(pars, x[:n], indx[:n], M)
        return out

    monkeypatch.setattr(oracle, "RBF_cov", rbf_padded)
    monkeypatch.setattr(tst, "hsta_covariance", cov_padded)
    x, indx, y = padded_data(c, Nmax)
    try:
        return tst.hsta_moments(c["pars"]["sta"][k], x, indx, y, xs, lab)
    finally:
        monkeypatch.undo()


def reordered(model, c, xs, z, lab):
    """the restatement on the same subject with its observations in reverse order: another evaluation order of the same numbers"""
    from test_hadamard_sta_cpu import hsta_moments
    from test_predsample_hadamard_cpu import restate_hps
    n = c["N"]
    r = np.arange(n)[::-1]
    if model == "sta":
        return [hsta_moments(c["pars"]["sta"][k], c["x"][r], c["indx"][r], c["y"][r], xs, lab) for k in (0, 1)]
    d = c["pars"]["sep"]
    draws = np.concatenate([d[:, :n][:, r], d[:, n:2 * n][:, r], d[:, 2 * n:]], axis=1)
    return restate_hps(c["x"][r], c["indx"][r], c["y"][r], draws, c["hyper"]["sep"], xs, z, lab)[:2]


@pytest.mark.parametrize("model", ["sep", "sta"])
@pytest.mark.parametrize("case", [c for c in cc.SET_A if c[0] >= 4] + [(130, 8, "unsorted")], ids=hc.case_id)
def test_the_restatement_on_a_padded_subject_agrees_with_the_subject_alone(monkeypatch, case, model):
    c, p = hc.build(case), hc.predictions(case)
    Nmax = 193 if c["M"] == 8 else 128                                     # the order its set pads it to
    xs, S, M = p["xs"], p["xs"].shape[0], c["M"]
    zs = np.swapaxes(p["z"], 0, 1)                                         # the restatement's order [S, H, 2]
    for form, lab in (("full", None), ("ix", p["lab"])):
        z = np.concatenate([zs, np.zeros((S, 2, M if lab is None else 1))], axis=2)
        if model == "sep":
            alone = p["hps_full" if form == "full" else "hps_ix"]
            padded = sep_padded(monkeypatch, c, Nmax, xs, z, lab)
            again = reordered("sep", c, xs, z, lab)
        else:
            alone = [a for k in (0, 1) for a in p["sta_full" if form == "full" else "sta_ix"][k]]
            padded = [a for k in (0, 1) for a in sta_padded(monkeypatch, c, Nmax, xs, lab, k)]
            again = [a for m in reordered("sta", c, xs, None, lab) for a in m]
        own = max(relerr(a, b) for a, b in zip(alone, again))
        got = max(relerr(a, b) for a, b in zip(alone, padded))
        print(model, hc.case_id(case), form, "two evaluation orders:", own, "padded against alone:", got)
        assert own > 0.0 or got == 0.0
        assert got <= 100.0 * own, (case, model, form, got, own)


# ---- 3. the surface -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", [SEP, STA])
def test_header_declares_the_entry(entry):
    src = re.sub(r"\s+,", ",", re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S))      # (a comment may stand before a comma)
    assert re.search(DECL[entry], src), "%s is not declared in nmgp.h with the documented signature" % entry


def test_library_exports_and_binding_carries_the_entries():
    from nonstationary_multivariate_gaussian_process_amd import build as b, _lib
    lib_path = b.build(verbose=False)
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib_path]).decode()
    exported = set(re.findall(r" T (nmgp_[a-z0-9_]+)", out))
    assert {SEP, STA, "nmgp_predsample_had_subjects"} <= exported
    I, V, P, IP = ctypes.c_int, ctypes.c_void_p, _lib.c_double_p, ctypes.POINTER(ctypes.c_int)
    sigs = {SEP: [V, P, I, I, P, P, IP, IP, I, P, P, P, P, P, IP], STA: [V, P, I, I, P, IP, IP, I, P, P, IP]}
    lib = _lib.load(require_gpu=False)
    for entry, sig in sigs.items():
        assert _lib.SIGNATURES[entry] == (I, sig) and getattr(lib, entry).argtypes == sig
    # no context: the entries refuse a NULL handle instead of touching it
    assert lib.nmgp_predsample_hads_subjects(None, None, 1, 1, None, None, None, None, 1, None, None, None, None, None, None) == -1
    assert lib.nmgp_predict_hadst_subjects(None, None, 1, 1, None, None, None, 1, None, None, None) == -1
    assert "nmgp_predsample_had_cohort.hip" in b.SOURCES


def test_python_layers_expose_the_cohort_prediction_of_both_models():
    from nonstationary_multivariate_gaussian_process_amd import _lib, drivers, hadamard_sep, hadamard_sta
    sig = inspect.signature(_lib.Context.predsample_hads_subjects)
    assert list(sig.parameters) == ["self", "pars", "hyper", "xs", "indx_star", "nstar", "draws_per_subject", "z", "star"]
    assert sig.parameters["draws_per_subject"].default == 1 and sig.parameters["nstar"].default is None
    sig = inspect.signature(_lib.Context.predict_hadst_subjects)
    assert list(sig.parameters) == ["self", "pars", "xs", "indx_star", "nstar", "draws_per_subject"]
    assert list(inspect.signature(hadamard_sep.cohort_predict).parameters) == ["ctx", "draws", "xs", "hyper", "indx_star", "z", "star"]
    assert list(inspect.signature(hadamard_sta.cohort_predict).parameters) == ["ctx", "draws", "xs", "indx_star"]
    for cls in (drivers.HadamardCohortMAP, drivers.HadamardSepCohortMAP, drivers.HadamardStaCohortMAP):
        assert list(inspect.signature(cls.predict).parameters) == ["self", "pars", "xs", "indx_star"]
        assert "No prediction" not in cls.__doc__
    want = ["subjects", "hyper_pars", "samples", "xs", "indx_star", "draws", "seed", "max_flop_waste", "ctxs"]
    for fn in (drivers.posterior_predict_hadamard_sep_cohort, drivers.posterior_predict_hadamard_sta_cohort,
               drivers.posterior_predict_hadamard_cohort):
        sig = inspect.signature(fn)
        assert list(sig.parameters) == want and sig.parameters["seed"].default == 0 and sig.parameters["max_flop_waste"].default == 0.5
    # nothing is installed under the reference's module names
    for mod in (hadamard_sep, hadamard_sta):
        assert not any("cohort" in n for n in mod.LOGPOS_NAMES + mod.PREDICTION_NAMES)
    # without a set the ragged forms refuse before any device call
    class NoSet:
        _cohort = None
    with pytest.raises(_lib.NmgpError):
        hadamard_sep.cohort_predict(NoSet(), [np.zeros(6)], [np.zeros(2)], np.zeros(9))
    with pytest.raises(_lib.NmgpError):
        hadamard_sta.cohort_predict(NoSet(), [np.zeros(4)], [np.zeros(2)])


def test_ragged_forms_pack_what_the_entries_take():
    """hadamard_sep / hadamard_sta.cohort_predict against a recording stand-in for the context: the padded arrays, the tables and
    the per-subject results, with width-2 starred arrays."""
    from nonstationary_multivariate_gaussian_process_amd import hadamard, hadamard_sep, hadamard_sta
    rng = np.random.default_rng(5)
    nobs, sizes, M, T, H = [4, 2, 3], [3, 0, 5], 2, 3, 2
    xs = [rng.standard_normal(n) for n in sizes]
    lab = [rng.integers(0, M, n).astype(np.int32) for n in sizes]
    z = [rng.standard_normal((H, n, 2)) for n in sizes]
    z2, nz = hadamard.cohort_pack_inputs(z, fill=np.nan)
    assert z2.shape == (3 * H, 5, 2) and nz.tolist() == sizes
    assert all(np.array_equal(a, b) for a, b in zip(hadamard.cohort_unpack_outputs(z2, nz, H), z))
    assert all(np.all(np.isnan(z2[s * H:(s + 1) * H, n:])) for s, n in enumerate(sizes))

    class Recorder:
        _cohort = (3, 4, M)

        def predsample_hads_subjects(self, pars, hyper, x2, indx_star=None, nstar=None, draws_per_subject=1, z=None, star=None):
            self.seen = dict(pars=pars, x2=x2, lab=indx_star, nstar=nstar, H=draws_per_subject, z=z, star=star)
            B, Smax = pars.shape[0], x2.shape[1]
            shape = (B, Smax) if indx_star is not None else (B, Smax, M)
            fill = np.arange(B, dtype=np.float64).reshape((B,) + (1,) * (len(shape) - 1))
            return np.zeros(shape) + fill, np.ones(shape) + fill, (z if z is not None else np.zeros((B, Smax, 2))), np.arange(B, dtype=np.int32)

        def predict_hadst_subjects(self, pars, x2, indx_star=None, nstar=None, draws_per_subject=1):
            r = self.predsample_hads_subjects(pars, None, x2, indx_star, nstar, draws_per_subject)
            return r[0], r[1], r[3]

    rec = Recorder()
    sep = [rng.standard_normal((H, 2 * n + T + 1)) for n in nobs]
    res = hadamard_sep.cohort_predict(rec, sep, xs, np.zeros(9), indx_star=lab, z=z)
    seen = rec.seen
    assert np.array_equal(seen["pars"], hadamard_sep.cohort_pack(sep, nobs, M, Nmax=4)) and seen["H"] == H
    assert seen["x2"].shape == (3, 5) and seen["nstar"].tolist() == sizes and seen["lab"].dtype == np.int32
    assert np.array_equal(seen["z"], hadamard.cohort_pack_inputs(z)[0]) and seen["star"] is None
    for s, (mean, var, star, status) in enumerate(res):
        assert mean.shape == var.shape == (H, sizes[s]) and star.shape == (H, sizes[s], 2) and status.tolist() == [2 * s, 2 * s + 1]
        assert np.array_equal(star, z[s]) and np.all(mean[1] == 2 * s + 1)
    fed = hadamard_sep.cohort_predict(rec, sep, xs, np.zeros(9), star=z)
    assert rec.seen["z"] is None and np.array_equal(rec.seen["star"], hadamard.cohort_pack_inputs(z)[0])
    assert [r[0].shape for r in fed] == [(H, n, M) for n in sizes]
    sta = [rng.standard_normal((H, T + 3)) for _ in nobs]
    res = hadamard_sta.cohort_predict(rec, sta, xs)
    assert np.array_equal(rec.seen["pars"], np.concatenate(sta)) and rec.seen["lab"] is None
    assert [len(r) for r in res] == [3, 3, 3] and [r[0].shape for r in res] == [(H, n, M) for n in sizes]
    assert [r[2].tolist() for r in res] == [[0, 1], [2, 3], [4, 5]]
    for bad in ([v[:, :-1] for v in sep], sep[:2]):
        with pytest.raises(Exception):
            hadamard_sep.cohort_predict(rec, bad, xs, np.zeros(9))
    with pytest.raises(Exception):
        hadamard_sta.cohort_predict(rec, [v[:, :-1] for v in sta], xs)
