"""Fixture of tests/test_gpu_schur_epilogue.py: the bits of the structured value path (k_syrk_schur's Sigma' epilogue) on the
smallest shapes that reach each path of that epilogue.

    python tools/make_schurepi_fixture.py [out.npz, default tests/golden/schurepi_parent_bits.npz]

runs one batched value evaluation per case on cuda:0 with the library of the tree it is started from and writes `out [B, 5]`
(float64) and `status [B]` (int32) of every case.  The committed fixture was written by the library of the commit BEFORE the
epilogue was reshaped; the test requires the same bytes of every later library.  `--print` runs the cases and prints them as one
JSON line instead (the test's child process under NMGP_POISON=1)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(ROOT, "tests", "golden", "schurepi_parent_bits.npz")
SVC_KEYS = ["mu_tilde_l", "alpha_tilde_l", "beta_tilde_l", "mu_L", "alpha_L", "beta_L", "a", "b"]

# (name, N, M, subjects, chains per subject): the path of the epilogue the case is the smallest to reach
CASES = (
    ("N128_M3_B2", 128, 3, 1, 2),        # one full diagonal tile
    ("N256_M3_B2", 256, 3, 1, 2),        # a full off-diagonal tile with its mirrored pass, two diagonal ones
    ("N257_M3_B3", 257, 3, 1, 3),        # one row past a tile edge
    ("N200_M3_B2", 200, 3, 1, 2),        # partial tiles on the masked path
    ("N384_M2_B2", 384, 2, 1, 2),        # M = 2: no mirrored pass
    ("N256_M4_B2", 256, 4, 1, 2),        # rolled loops, table path
    ("N160_M5_B2", 160, 5, 1, 2),        # no table, partial tile
    ("N256_M3_S2x2", 256, 3, 2, 2),      # the per-subject x / Y stride
)


def hyper():
    from nonstationary_multivariate_gaussian_process_amd import sim
    return [sim.HYPER_SVC[k] for k in SVC_KEYS]


def case_inputs(name):
    """Subjects (simulate_nonseparable, fixed seeds) and the chains' parameters (perturb of each subject's truth) of a case."""
    from nonstationary_multivariate_gaussian_process_amd import sim
    i, (_, N, M, S, K) = next((i, c) for i, c in enumerate(CASES) if c[0] == name)
    subs = [sim.simulate_nonseparable(N, M, seed=2100 + 10 * i + s) for s in range(S)]
    pars = np.stack([sim.perturb(d["pars_true"], 0.05, 0.2 + 0.11 * k) for d in subs for k in range(K)])
    return subs, pars, K


def evaluate(name, schur=None):
    """One batched value evaluation of case `name` in a fresh context (schur = 0: created under NMGP_SVC_SCHUR=0, the dense path):
    out [B, 5], status [B]."""
    from nonstationary_multivariate_gaussian_process_amd import _lib
    subs, pars, K = case_inputs(name)
    old = os.environ.get("NMGP_SVC_SCHUR")
    if schur is not None:
        os.environ["NMGP_SVC_SCHUR"] = str(schur)
    try:
        ctx = _lib.Context(0)
    finally:
        if schur is not None:
            if old is None:
                del os.environ["NMGP_SVC_SCHUR"]
            else:
                os.environ["NMGP_SVC_SCHUR"] = old
    try:
        ctx.set_data(subs[0]["x"], subs[0]["Y"])
        ctx.svc_batch_alloc(pars.shape[0])
        if len(subs) > 1:
            ctx.svc_batch_set_subjects(np.stack([d["x"] for d in subs]), np.stack([d["Y"] for d in subs]), K)
        ctx.svc_batch_set_pars(pars)
        ctx.svc_batch_eval(hyper(), True, want_grad=False)
        out, status = ctx.svc_batch_fetch()
    finally:
        ctx.close()
    return np.ascontiguousarray(out, dtype=np.float64), np.ascontiguousarray(status, dtype=np.int32)


def evaluate_all():
    res = {}
    for c in CASES:
        res[c[0] + "/out"], res[c[0] + "/status"] = evaluate(c[0])
    return res


def main():
    res = evaluate_all()
    if "--print" in sys.argv:
        print(json.dumps({k: [str(a.dtype), list(a.shape), a.tobytes().hex()] for k, a in res.items()}))
        return
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = args[0] if args else FIXTURE
    np.savez(path, **res)
    for k in sorted(res):
        print(k, res[k].shape, res[k].dtype, res[k].reshape(-1)[:2])
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
