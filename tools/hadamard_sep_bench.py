"""Hadamard separable objective on the subject and with the protocol of tools/hadamard_bench.py: N = 6144 single observations, M = 3.
    python tools/hadamard_sep_bench.py [--N 6144] [--B 1,16,64] [--reps 3] [--out FILE] [--no-cpu]
    python tools/hadamard_sep_bench.py --one-step 16      # a warm-up and ONE value+gradient step of 16 chains: the form to run
                                                          # under `rocprofv3 --kernel-trace --stats -- python3 tools/hadamard_sep_bench.py ...`
Times nmgp_hads_batch_eval (B chains in one launch sequence) for value and value+gradient against a loop of B single-chain calls,
alternating in one session.  One JSON line per (B, mode) with the fields of tools/hadamard_bench.py, so that the two tools' lines
from one session can be laid side by side (profiles/hadamard_sep_bench.jsonl holds both): the matrix order, the factorisation and
the inverse are the same, the separable model has 2 prior columns per chain where the nonseparable one has 1 + T."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from hadamard_bench import PEAK, subject  # noqa: E402  (the same x, indx, y and tilde_l)
from nonstationary_multivariate_gaussian_process_amd import _lib  # noqa: E402

HYPER = np.array([-2.4, 1.0, 0.05, 0.1, 1.5, 0.03, 2.0, 0.5, 3.0])       # the fixtures' (tests/golden/make_golden_hadamard_sep.py)


def start(N, M):
    x, indx, y, p_svc = subject(N, M)
    Lv = []
    for r in range(M):
        for c in range(r + 1):
            Lv.append(0.9 + 0.05 * r if c == r else 0.1 * (len(Lv) % 5 + 1) - 0.25)
    p0 = np.concatenate([p_svc[:N], 0.1 + 0.3 * np.cos(2.0 * np.pi * x), Lv, [np.log(1e-2)]])
    return x, indx, y, p0


def chains(p0, x, N, T, B):
    out = []
    for k in range(B):
        p = p0.copy()
        p[:N] += 0.02 * np.sin(3.0 * x + 0.4 + k)
        p[N:2 * N] += 0.02 * np.cos(2.0 * x + 0.3 * k)
        p[2 * N:2 * N + T] += 0.02 * np.sin(0.7 + k + np.arange(T))
        out.append(p)
    return np.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=6144)
    ap.add_argument("--M", type=int, default=3)
    ap.add_argument("--B", default="1,16,64")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--one-step", type=int, default=0)
    a = ap.parse_args()
    N, M = a.N, a.M
    T = M * (M + 1) // 2
    x, indx, y, p0 = start(N, M)
    c = _lib.Context(0)
    c.had_set_data(x, indx, y)
    if a.one_step:
        for _ in range(2):               # the first builds the prior factors and the workspace
            out, g, st = c.hads_batch_eval(chains(p0, x, N, T, a.one_step), HYPER, True, True)
        assert np.all(st == 0)
        print(json.dumps({"one_step_chains": a.one_step, "N": N, "M": M, "neglog0": float(out[0, 0])}), flush=True)
        c.close()
        return
    cpu = {}
    if not a.no_cpu:
        from test_hadamard_sep_cpu import hsep_logpos
        for mode, key in ((False, "value"), (True, "value_grad")):
            t0 = time.perf_counter()
            hsep_logpos(p0, x, indx, y, HYPER, grad=mode)
            cpu[key] = 1.0 / (time.perf_counter() - t0)
    lines = []
    for B in [int(v) for v in a.B.split(",")]:
        P = chains(p0, x, N, T, B)
        for mode, key, flop in ((False, "value", float(N) ** 3 / 3.0), (True, "value_grad", float(N) ** 3)):
            c.hads_batch_eval(P, HYPER, True, mode)                  # workspace of this B, prior factors
            c.hads_batch_eval(P[0], HYPER, True, mode)
            t_b, t_l, ok = [], [], True
            for _ in range(a.reps):
                t0 = time.perf_counter()
                out, g, st = c.hads_batch_eval(P, HYPER, True, mode)
                t_b.append(time.perf_counter() - t0)
                ok = ok and bool(np.all(st == 0))
                t0 = time.perf_counter()
                for k in range(B):
                    c.hads_batch_eval(P[k], HYPER, True, mode)
                t_l.append(time.perf_counter() - t0)
            tb, tl = float(np.median(t_b)), float(np.median(t_l))
            rec = {"what": "nmgp_hads_batch_eval against a loop of single-chain calls, N=%d observations, M=%d, host pointers in and out"
                           % (N, M), "B": B, "mode": key, "batch_evals_per_s": B / tb, "loop_evals_per_s": B / tl,
                   "batch_over_loop": tl / tb, "batch_ms_reps": [1e3 * t for t in t_b], "loop_ms_reps": [1e3 * t for t in t_l],
                   "roofline_frac_batch": B * flop / tb / PEAK, "roofline_frac_loop": B * flop / tl / PEAK,
                   "roofline_flop_per_eval": "N^3/3" if not mode else "N^3", "all_chains_ok": ok,
                   "cpu_numpy_restatement_evals_per_s": cpu.get(key), "library_build_id": _lib.build_id()}
            print(json.dumps(rec), flush=True)
            lines.append(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    c.close()


if __name__ == "__main__":
    main()
