"""Fixture of tests/test_gpu_predsample_had_cohort_parent_bits.py: the bits of the nonseparable cohort predictor
(nmgp_predsample_had_subjects) on the subject sets of tests/hadamard_cohort_cases.py.

    python tools/make_predsample_had_cohort_fixture.py [out.npz, default tests/golden/predsample_had_cohort_parent_bits.npz]

runs every case on cuda:0 with the library of the tree it is started from, through Context.had_set_subjects and
Context.predsample_had_subjects only, and writes the SHA-256 (uint8 [32]) of the bytes of `mean`, `var`, `star` (float64) and `status`
(int32) of each call.  The committed fixture was written by the library of the commit BEFORE the entry's host function became the
schedule hadc_predict<Model> that the separable and the stationary cohort predictors share; the test requires the same digests of
every later library.  `--print` runs the cases and prints them as one JSON line instead (the test's child process under NMGP_POISON=1).

Cases: sets A, D, E and set A padded to Nmax = 192 ("A_nmax192": a whole padded tile), each subject at its own default grid
(predsample_had_cases.new_inputs: ragged within a set), two draws per subject, in the full ("full") and the indexed ("ix") form, five
calls each:
    z        the regression under the fixed normals predsample_had_cases.normals
    mean     z = NULL: the conditional means
    star     star_in = the starred values the call "z" returned (the regression skipped)
    chunk1   the call "z" under NMGP_PREDSAMPLE_CHUNK=1: every chunk a part of one subject's draws
    nan      the call "z" with a NaN in a real slot (tilde_l[0]) of draw 1 of the set's second subject: status NMGP_NUM_NAN and NaN
             moments for that draw, the other draws' bytes those of "z"
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

FIXTURE = os.path.join(ROOT, "tests", "golden", "predsample_had_cohort_parent_bits.npz")
CASES = ("A", "D", "E", "A_nmax192")
FORMS = ("full", "ix")
CALLS = ("z", "mean", "star", "chunk1", "nan")
WHAT = ("mean", "var", "star", "status")
NAN_ROW = 3                                  # draw 1 of subject 1


def case_keys():
    """every key of the fixture, "<case>/<form>/<call>/<mean | var | star | status>", in the order the cases run"""
    return ["%s/%s/%s/%s" % (case, form, call, what) for case in CASES for form in FORMS for call in CALLS for what in WHAT]


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8).copy()


def evaluate_all():
    """{key: digest} of every case, in one context"""
    import hadamard_cases as hc
    import hadamard_cohort_cases as cc
    import predsample_had_cases as pc
    from nonstationary_multivariate_gaussian_process_amd import _lib, hadamard
    old = os.environ.pop("NMGP_PREDSAMPLE_CHUNK", None)
    hyper = hc.hypers()["had"]
    ctx = _lib.Context(0)
    res = {}
    try:
        for case in CASES:
            cases = cc.SETS[case[0]]
            Nmax = 192 if case.endswith("nmax192") else max(cc.nobs(cases))
            subs, M = cc.subjects(cases), cases[0][1]
            ctx.had_set_subjects([c["x"] for c in subs], [c["indx"] for c in subs], [c["y"] for c in subs], M=M, Nmax=Nmax)
            pars = cc.pack(cc.chains(cases, 2), cc.nobs(cases), M, Nmax=Nmax)
            bad = pars.copy()
            bad[NAN_ROW, 0] = np.nan
            new = [pc.new_inputs(c) for c in cases]
            xs, nstar = hadamard.cohort_pack_inputs([v[0] for v in new])
            Smax = xs.shape[1]
            lab = hadamard.cohort_pack_inputs([v[1] for v in new], nstar, Smax, 0, np.int32)[0]
            z = hadamard.cohort_pack_inputs([pc.normals(c, int(n)) for c, n in zip(cases, nstar)], nstar, Smax)[0]
            for form in FORMS:
                kw = dict(indx_star=lab if form == "ix" else None, nstar=nstar, draws_per_subject=2)
                got = {"z": ctx.predsample_had_subjects(pars, hyper, xs, z=z, **kw),
                       "mean": ctx.predsample_had_subjects(pars, hyper, xs, **kw)}
                got["star"] = ctx.predsample_had_subjects(pars, hyper, xs, star=got["z"][2], **kw)
                os.environ["NMGP_PREDSAMPLE_CHUNK"] = "1"
                try:
                    got["chunk1"] = ctx.predsample_had_subjects(pars, hyper, xs, z=z, **kw)
                finally:
                    del os.environ["NMGP_PREDSAMPLE_CHUNK"]
                got["nan"] = ctx.predsample_had_subjects(bad, hyper, xs, z=z, **kw)
                B = pars.shape[0]
                for call in ("z", "mean", "star", "chunk1"):
                    assert got[call][3].tolist() == [0] * B and all(np.all(np.isfinite(a)) for a in got[call][:3]), (case, form, call)
                assert all(np.array_equal(a, b) for a, b in zip(got["z"], got["chunk1"])), (case, form)
                assert all(np.array_equal(a, b) for a, b in zip(got["z"], got["star"])), (case, form)
                keep = np.arange(B) != NAN_ROW
                n1 = int(nstar[1])
                assert got["nan"][3].tolist() == [0] * NAN_ROW + [_lib.NUM_NAN] + [0] * (B - NAN_ROW - 1), (case, form, got["nan"][3])
                assert np.all(np.isnan(got["nan"][0][NAN_ROW, :n1])) and np.all(np.isnan(got["nan"][1][NAN_ROW, :n1])), (case, form)
                assert all(np.array_equal(a[keep], b[keep]) for a, b in zip(got["nan"][:2], got["z"][:2])), (case, form)
                for call in CALLS:
                    for what, a in zip(WHAT, got[call]):
                        res["%s/%s/%s/%s" % (case, form, call, what)] = digest(a.astype(np.int32) if what == "status" else a)
        ctx.had_clear_subjects()
    finally:
        ctx.close()
        if old is not None:
            os.environ["NMGP_PREDSAMPLE_CHUNK"] = old
    assert list(res) == case_keys()
    return res


def main():
    res = evaluate_all()
    if "--print" in sys.argv:
        print(json.dumps({k: a.tobytes().hex() for k, a in res.items()}))
        return
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = args[0] if args else FIXTURE
    np.savez_compressed(path, **res)
    print("wrote", path, os.path.getsize(path), "bytes,", len(res), "digests")


if __name__ == "__main__":
    main()
