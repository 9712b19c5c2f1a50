"""CPU-only half of the cohort prediction tests (nmgp_predsample_had_subjects; the GPU half is tests/test_gpu_predsample_had_cohort.py):

1. the padding argument on the host: tests/predsample_had_cases.restate_hpn run on a subject PADDED in NumPy (identity rows / columns
   in the covariance and in both GP-prior covariances, y = 0, zero cross rows, the padded parameter layout) agrees with restate_hpn on
   the subject alone at every real slot;
2. the pack / unpack helpers of the new-input arrays;
3. the precondition of the GPU half's bars: every compared raw variance of the restatement exceeds its draw's sigma2_err, so the clip
   to 1e-6 plays no part;
4. the ABI surface: header, exported symbol, ctypes table, Python layers."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import hadamard_cases as hc
import hadamard_cohort_cases as cc
import predsample_had_cases as pc
from conftest import ROOT, relerr
from oracle import nmgp_oracle as oracle

HEADER = os.path.join(ROOT, "include", "nmgp.h")
ENTRY = "nmgp_predsample_had_subjects"
DECL = (r"int\s+nmgp_predsample_had_subjects\s*\(\s*nmgp_ctx\s*\*\s*\w+,\s*const\s+double\s*\*\s*pars,\s*int\s+B,\s*int\s+draws_per_subject,"
        r"\s*const\s+double\s+hyper\[8\],\s*const\s+double\s*\*\s*xs,\s*const\s+int\s*\*\s*indx_star,\s*const\s+int\s*\*\s*nstar,"
        r"\s*int\s+Smax,\s*const\s+double\s*\*\s*z,\s*const\s+double\s*\*\s*star_in,\s*double\s*\*\s*mean,\s*double\s*\*\s*var,"
        r"\s*double\s*\*\s*star_out,\s*int\s*\*\s*status\s*\)\s*;")


# ---- 1. the restatement on a padded subject -------------------------------------------------------------------------------------------
def restate_padded(monkeypatch, c, Nmax, xs, z, lab):
    """restate_hpn, unchanged, on the subject c padded to Nmax: the pieces it builds its matrices from are wrapped so that the padded
    observations are decoupled unit observations, as the device pads them."""
    import test_hadamard_cpu as thc
    from nonstationary_multivariate_gaussian_process_amd import hadamard
    n, M = c["N"], c["M"]
    rbf, gibbs, cov = oracle.RBF_cov, oracle.Nonstationary_RBF_cov, thc.had_covariance

    def rbf_padded(X1, X2=None, alpha=1.0, beta=1.0):
        if X1.shape[0] != Nmax:
            return rbf(X1, X2, alpha=alpha, beta=beta)
        if X2 is None:                                                     # identity block
            out = np.eye(Nmax)
            out[:n, :n] = rbf(X1[:n], alpha=alpha, beta=beta)
            return out
        out = np.zeros((Nmax, np.asarray(X2).shape[0]))                    # zero right-hand sides
        out[:n] = rbf(X1[:n], X2, alpha=alpha, beta=beta)
        return out

    def gibbs_padded(X1, sigma1=None, ell1=None, X2=None, sigma2=None, ell2=None):
        if X2 is None or X1.shape[0] != Nmax:                              # (had_covariance's own call, on the real observations)
            return gibbs(X1, sigma1=sigma1, ell1=ell1, X2=X2, sigma2=sigma2, ell2=ell2)
        out = np.zeros((Nmax, X2.shape[0]))                                # zero cross rows
        out[:n] = gibbs(X1[:n], sigma1=sigma1[:n], ell1=ell1[:n], X2=X2, sigma2=sigma2, ell2=ell2)
        return out

    def cov_padded(tl, Lv, tse, x, indx, M_):
        out = np.eye(Nmax)
        out[:n, :n] = cov(tl[:n], Lv[:n], tse, x[:n], indx[:n], M_)
        return out

    monkeypatch.setattr(oracle, "RBF_cov", rbf_padded)
    monkeypatch.setattr(oracle, "Nonstationary_RBF_cov", gibbs_padded)
    monkeypatch.setattr(thc, "had_covariance", cov_padded)
    pad = Nmax - n
    x = np.concatenate([c["x"], np.zeros(pad)])
    y = np.concatenate([c["y"], np.zeros(pad)])
    indx = np.concatenate([c["indx"], np.zeros(pad, dtype=c["indx"].dtype)])
    draws = hadamard.cohort_pack([c["draws"]], [n], M, Nmax=Nmax)
    try:
        return pc.restate_hpn(x, indx, y, draws, c["hyper"], xs, z, lab)
    finally:
        monkeypatch.undo()


def reordered(c, xs, z, lab):
    """the restatement on the same subject with its observations in reverse order: another evaluation order of the same numbers"""
    n, T = c["N"], c["T"]
    r = np.arange(n)[::-1]
    d = c["draws"]
    draws = np.concatenate([d[:, :n][:, r], d[:, n:n + n * T].reshape(2, n, T)[:, r].reshape(2, -1), d[:, -1:]], axis=1)
    return pc.restate_hpn(c["x"][r], c["indx"][r], c["y"][r], draws, c["hyper"], xs, z, lab)


@pytest.mark.parametrize("case", [c for c in cc.SET_A if c[0] >= 4] + [(130, 8, "unsorted")], ids=hc.case_id)
def test_the_restatement_on_a_padded_subject_agrees_with_the_subject_alone(monkeypatch, case):
    c = pc.subject(case)
    e = pc.expected(case)
    Nmax = 193 if c["M"] == 8 else 128                                     # the order its set pads it to
    assert c["M"] >= 2                                                     # (restate_hpn infers M from the labels: pads carry label 0)
    for form, lab in (("full", None), ("ix", e["lab"])):
        alone = e[form]
        again = reordered(c, e["xs"], e["z"], lab)
        padded = restate_padded(monkeypatch, c, Nmax, e["xs"], e["z"], lab)
        own = max(relerr(a, b) for a, b in zip(alone, again))
        got = max(relerr(a, b) for a, b in zip(alone, padded))
        print(hc.case_id(case), form, "two evaluation orders:", own, "padded against alone:", got)
        assert own > 0.0 or got == 0.0
        assert got <= 100.0 * own, (case, form, got, own)


# ---- 2. the helpers of the new-input arrays --------------------------------------------------------------------------------------------
def test_input_helpers_round_trip_and_leave_the_fill_in_padded_slots():
    from nonstationary_multivariate_gaussian_process_amd import hadamard
    rng = np.random.default_rng(3)
    sizes, k, W = [4, 0, 7, 1], 3, 4
    xs = [rng.standard_normal(n) for n in sizes]
    lab = [rng.integers(0, 3, n).astype(np.int32) for n in sizes]
    z = [rng.standard_normal((k, n, W)) for n in sizes]
    x2, nstar = hadamard.cohort_pack_inputs(xs, fill=np.nan)
    assert x2.shape == (4, 7) and nstar.dtype == np.int32 and nstar.tolist() == sizes
    l2, _ = hadamard.cohort_pack_inputs(lab, fill=99, dtype=np.int32)
    z2, nz = hadamard.cohort_pack_inputs(z, fill=-7.0)
    assert l2.dtype == np.int32 and z2.shape == (4 * k, 7, W) and nz.tolist() == sizes
    for s, n in enumerate(sizes):
        assert np.array_equal(x2[s, :n], xs[s]) and np.all(np.isnan(x2[s, n:]))
        assert np.array_equal(l2[s, :n], lab[s]) and np.all(l2[s, n:] == 99)
        assert np.array_equal(z2[s * k:(s + 1) * k, :n], z[s]) and np.all(z2[s * k:(s + 1) * k, n:] == -7.0)
    for back, want in ((hadamard.cohort_unpack_outputs(x2[:, :, None], nstar), [v[None, :, None] for v in xs]),
                       (hadamard.cohort_unpack_outputs(z2, nstar, k), z)):
        assert all(np.array_equal(a, b) for a, b in zip(back, want))
    status = np.arange(4 * k)
    assert [v.tolist() for v in hadamard.cohort_unpack_outputs(status, nstar, k)] == [[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10, 11]]
    # a wider Smax, and nothing to predict at all
    assert hadamard.cohort_pack_inputs(xs, Smax=9)[0].shape == (4, 9)
    e2, n0 = hadamard.cohort_pack_inputs([np.zeros(0), np.zeros(0)])
    assert e2.shape == (2, 1) and n0.tolist() == [0, 0]
    with pytest.raises(ValueError):
        hadamard.cohort_pack_inputs(xs, Smax=5)
    with pytest.raises(ValueError):
        hadamard.cohort_pack_inputs(z, nstar=[4, 0, 6, 1])


# ---- 3. the precondition of the bars ------------------------------------------------------------------------------------------------------
def grids(case):
    return [dict(), pc.WIDE_FULL, pc.WIDE_INDEXED] if case == pc.WIDE else [dict()]


@pytest.mark.parametrize("name", sorted(cc.SETS))
def test_every_compared_raw_variance_exceeds_its_noise_floor(name):
    for case in cc.SETS[name]:
        if case == hc.MINOR:
            continue
        for kw in grids(case):
            floor = pc.raw_variance_floor(pc.expected(case, **kw), case)
            print(name, hc.case_id(case), kw, "raw variance / sigma2_err >=", floor)
            assert floor > 1.0, (case, kw, floor)


# ---- 4. the ABI surface ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(DECL, src), "%s is not declared in nmgp.h with the documented signature" % ENTRY


def test_library_exports_and_binding_carries_the_entry():
    from nonstationary_multivariate_gaussian_process_amd import build as b, _lib
    lib_path = b.build(verbose=False)
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib_path]).decode()
    assert ENTRY in set(re.findall(r" T (nmgp_[a-z0-9_]+)", out)), "%s is not exported by %s" % (ENTRY, lib_path)
    I, V, P, IP = ctypes.c_int, ctypes.c_void_p, _lib.c_double_p, ctypes.POINTER(ctypes.c_int)
    sig = [V, P, I, I, P, P, IP, IP, I, P, P, P, P, P, IP]
    assert _lib.SIGNATURES[ENTRY] == (I, sig)
    lib = _lib.load(require_gpu=False)
    assert lib.nmgp_predsample_had_subjects.argtypes == sig
    # no context: the entry refuses a NULL handle instead of touching it
    assert lib.nmgp_predsample_had_subjects(None, None, 1, 1, None, None, None, None, 1, None, None, None, None, None, None) == -1


def test_python_layers_expose_the_cohort_prediction():
    from nonstationary_multivariate_gaussian_process_amd import _lib, drivers, hadamard
    sig = inspect.signature(_lib.Context.predsample_had_subjects)
    assert list(sig.parameters) == ["self", "pars", "hyper", "xs", "indx_star", "nstar", "draws_per_subject", "z", "star"]
    assert sig.parameters["draws_per_subject"].default == 1 and sig.parameters["nstar"].default is None
    sig = inspect.signature(hadamard.cohort_predict)
    assert list(sig.parameters) == ["ctx", "draws", "xs", "hyper", "indx_star", "z", "star"]
    assert callable(hadamard.cohort_pack_inputs) and callable(hadamard.cohort_unpack_outputs)
    assert list(inspect.signature(drivers.HadamardCohortMAP.predict).parameters) == ["self", "pars", "xs", "indx_star"]
    sig = inspect.signature(drivers.posterior_predict_hadamard_cohort)
    assert list(sig.parameters) == ["subjects", "hyper_pars", "samples", "xs", "indx_star", "draws", "seed", "max_flop_waste", "ctxs"]
    assert sig.parameters["seed"].default == 0 and sig.parameters["max_flop_waste"].default == 0.5
    # nothing is installed under the reference's module names
    assert not any("cohort" in n for n in hadamard.LOGPOS_NAMES + hadamard.PREDICTION_NAMES)
