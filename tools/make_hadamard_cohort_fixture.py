"""Fixture of tests/test_gpu_hadamard_cohort_parent_bits.py: the bits of the three cohort evaluation entries (nmgp_had_subjects_eval,
nmgp_hads_subjects_eval, nmgp_hadst_subjects_eval) on the subject sets of tests/hadamard_cohort_cases.py, the smallest that reach every
mask position of the masked kernels.

    python tools/make_hadamard_cohort_fixture.py [out.npz, default tests/golden/hadamard_cohort_parent_bits.npz]

runs every case on cuda:0 with the library of the tree it is started from, through Context.had_set_subjects, had_subjects_eval,
hads_subjects_eval, hadst_subjects_eval and had_clear_subjects only, and writes `out`, `grad` (float64) and `status` (int32) of each
call.  The committed fixture was written by the library of the commit BEFORE the three entries came to share one chunk skeleton and
one masked Gibbs kernel pair; the test requires the same bytes of every later library.  `--print` runs the cases and prints them as
one JSON line instead (the test's child process under NMGP_POISON=1).

Cases, each for the three models ("had" nonseparable, "sep" separable, "sta" stationary):
    A2, B2, D2, E2   sets A, B, D, E with chains 0 and 1 of every subject, three calls each: priors + gradient ("pg"), no priors +
                     gradient ("ng"), priors, value only ("pv")
    A2_nmax192       set A padded to Nmax = 192: a whole padded tile (the "nothing real in the tile" branches), the same three calls
    A3_nan_real      set A, three chains per subject (0, 1, their midpoint), a NaN in a real slot of chain 1 of subject 1: the status
                     pattern, that chain's NaN row and zero gradient row; the other chains' bytes are those of the clean call
    A2_nan_pad       (had, sep) set A with NaN in every padded parameter slot: status 0, finite, the bytes of A2
    chunk            two subjects (1024 and 513 observations, M = 2, Nmax = 1024), 48 chains per subject, priors + gradient, under
                     NMGP_HAD_BATCH_SLAB_GB=1: four chunks, each a part of one subject's chains
Stored as the SHA-256 of the array's bytes (uint8 [32]) instead of the array: every array of `chunk`, and `grad` of B2 and A2_nan_pad
(the fixture stays small; A2_nan_pad's gradients are A2's, which are stored)."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

FIXTURE = os.path.join(ROOT, "tests", "golden", "hadamard_cohort_parent_bits.npz")
MODELS = ("had", "sep", "sta")
ENTRY = {"had": "had_subjects_eval", "sep": "hads_subjects_eval", "sta": "hadst_subjects_eval"}
MODES = {"pg": (True, True), "ng": (False, True), "pv": (True, False)}          # (prior, want_grad)
SET_CASES = ("A2", "B2", "D2", "E2", "A2_nmax192")
CHUNK_NOBS, CHUNK_CPS = [1024, 513], 48
DIGEST_ALL = ("chunk",)
DIGEST_GRAD = ("B2", "A2_nan_pad")


def case_keys():
    """every key of the fixture, "<case>/<model>/<mode>/<out | grad | status>", in the order the cases run"""
    keys = []
    for model in MODELS:
        for case in SET_CASES:
            for mode, (_, want_grad) in MODES.items():
                keys += ["%s/%s/%s/%s" % (case, model, mode, a) for a in (("out", "grad", "status") if want_grad else ("out", "status"))]
        keys += ["A3_nan_real/%s/pg/%s" % (model, a) for a in ("out", "grad", "status")]
        if model != "sta":
            keys += ["A2_nan_pad/%s/pg/%s" % (model, a) for a in ("out", "grad", "status")]
        keys += ["chunk/%s/pg/%s" % (model, a) for a in ("out", "grad", "status")]
    return keys


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8).copy()


def stored(key, a):
    case, _, _, what = key.split("/")
    a = np.ascontiguousarray(a)
    return digest(a) if case in DIGEST_ALL or (case in DIGEST_GRAD and what == "grad") else a


def pack(model, vectors, sizes, M, Nmax=None, fill=0.0):
    """the rows the model's cohort entry takes"""
    import hadamard_cohort_cases as cc
    import hadamard_cohort_model_cases as mc
    return cc.pack(vectors, sizes, M, Nmax=Nmax, fill=fill) if model == "had" else mc.pack(model, vectors, sizes, M, Nmax=Nmax, fill=fill)


def same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def evaluate_all():
    """{key: array or digest} of every case, in one context"""
    import hadamard_cases as hc
    import hadamard_cohort_cases as cc
    from nonstationary_multivariate_gaussian_process_amd import _lib
    old = os.environ.pop("NMGP_HAD_BATCH_SLAB_GB", None)
    ctx = _lib.Context(0)
    res = {}

    def put(case, model, mode, got):
        for what, a in zip(("out", "grad", "status"), got):
            if a is not None:
                key = "%s/%s/%s/%s" % (case, model, mode, what)
                res[key] = stored(key, a.astype(np.int32) if what == "status" else a)

    def set_subjects(cases, Nmax=None):
        subs = cc.subjects(cases)
        ctx.had_set_subjects([c["x"] for c in subs], [c["indx"] for c in subs], [c["y"] for c in subs], M=cases[0][1], Nmax=Nmax)

    try:
        for model in MODELS:
            ev = getattr(ctx, ENTRY[model])
            clean_A2 = None
            for case in SET_CASES:
                cases = cc.SETS[case[0]]
                Nmax = 192 if case.endswith("nmax192") else None
                sizes, M = cc.nobs(cases), cases[0][1]
                hyper = hc.build(cases[0])["hyper"][model]
                set_subjects(cases, Nmax)
                P = pack(model, [c["pars"][model][:2] for c in cc.subjects(cases)], sizes, M, Nmax=Nmax)
                for mode, (prior, want_grad) in MODES.items():
                    got = ev(P, hyper, prior=prior, want_grad=want_grad, chains_per_subject=2)
                    assert got[2].tolist() == [0] * (2 * len(cases)) and np.all(np.isfinite(got[0])), (case, model, mode, got[2])
                    assert not want_grad or np.all(np.isfinite(got[1])), (case, model, mode)
                    put(case, model, mode, got)
                    if case == "A2" and mode == "pg":
                        clean_A2 = got
            cases = cc.SET_A
            sizes, M, hyper = cc.nobs(cases), 2, hc.build(cases[0])["hyper"][model]
            set_subjects(cases)
            # a NaN in a real slot of chain 1 of subject 1 (63 observations): tilde_l[1] (the stationary model's one tilde_l)
            rows = [np.stack([v[0], v[1], 0.5 * (v[0] + v[1])]) for v in (c["pars"][model] for c in cc.subjects(cases))]
            clean = ev(pack(model, rows, sizes, M), hyper, prior=True, want_grad=True, chains_per_subject=3)
            assert clean[2].tolist() == [0] * 18
            rows[1] = rows[1].copy()
            rows[1][1, 0 if model == "sta" else 1] = np.nan
            got = ev(pack(model, rows, sizes, M), hyper, prior=True, want_grad=True, chains_per_subject=3)
            keep = np.arange(18) != 4
            assert got[2].tolist() == [0] * 4 + [_lib.NUM_NAN] + [0] * 13 and np.all(np.isnan(got[0][4])) and not np.any(got[1][4])
            assert same([a[keep] for a in got], [a[keep] for a in clean]), model
            put("A3_nan_real", model, "pg", got)
            if model != "sta":                                   # NaN in the padded slots only: inert
                P = pack(model, [c["pars"][model][:2] for c in cc.subjects(cases)], sizes, M, fill=np.nan)
                assert np.isnan(P).sum() > 0
                got = ev(P, hyper, prior=True, want_grad=True, chains_per_subject=2)
                assert got[2].tolist() == [0] * 12 and np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[1])) and same(got, clean_A2)
                put("A2_nan_pad", model, "pg", got)
            # the chunked call (tests/test_gpu_hadamard_cohort_models.py, test_results_do_not_depend_on_the_chunking, its second shape)
            M, Nmax = 2, max(CHUNK_NOBS)
            subs, rows = [], []
            for s, n in enumerate(CHUNK_NOBS):
                x, indx, y, L_vec = hc.subject(n, M, "interleaved", 3400 + s)
                subs.append((x, indx, y))
                v = hc.parameters(x, M, L_vec)[model]
                rows.append(v[0][None] + (np.arange(CHUNK_CPS) / CHUNK_CPS)[:, None] * (v[1] - v[0])[None])
            ctx.had_set_subjects([s[0] for s in subs], [s[1] for s in subs], [s[2] for s in subs], M=M, Nmax=Nmax)
            os.environ["NMGP_HAD_BATCH_SLAB_GB"] = "1"
            try:
                got = ev(pack(model, rows, CHUNK_NOBS, M, Nmax=Nmax), hc.hypers()[model], prior=True, want_grad=True,
                         chains_per_subject=CHUNK_CPS)
            finally:
                del os.environ["NMGP_HAD_BATCH_SLAB_GB"]
            assert got[2].tolist() == [0] * (2 * CHUNK_CPS) and np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[1])), model
            put("chunk", model, "pg", got)
            ctx.had_clear_subjects()                             # (gives the 1024-order prior factors back)
    finally:
        ctx.close()
        if old is not None:
            os.environ["NMGP_HAD_BATCH_SLAB_GB"] = old
    assert list(res) == case_keys()
    return res


def main():
    res = evaluate_all()
    if "--print" in sys.argv:
        print(json.dumps({k: [str(a.dtype), list(a.shape), a.tobytes().hex()] for k, a in res.items()}))
        return
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = args[0] if args else FIXTURE
    np.savez_compressed(path, **res)
    for k in res:
        print(k, res[k].shape, res[k].dtype, res[k].reshape(-1)[:2])
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
