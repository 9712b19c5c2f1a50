"""Hadamard nonseparable objective at the headline's matrix order: N = 6144 single observations, M = 3.
    python tools/hadamard_bench.py [--N 6144] [--B 1,16,64] [--reps 3] [--out profiles/hadamard_bench.jsonl] [--no-cpu]
    python tools/hadamard_bench.py --one-step 16          # a warm-up and ONE value+gradient step of 16 chains: the form to run
                                                          # under `rocprofv3 --kernel-trace --stats -- python3 tools/hadamard_bench.py ...`
                                                          # (tools/trace_summary.py <trace> k_had_grad_final cuts out the last step)
Times nmgp_had_batch_eval (B chains in one launch sequence) for value and value+gradient against a loop of B single-chain calls,
alternating in one session.  One JSON line per (B, mode): evals/s on both sides, the fraction of the FP64 matrix roofline on
N^3 / 3 (value) and N^3 (value+gradient), and the rate of the NumPy restatement (tests/test_hadamard_cpu.py) on the same host."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from nonstationary_multivariate_gaussian_process_amd import _lib  # noqa: E402

PEAK = 78.6e12          # FP64 matrix peak
HYPER = np.array([-2.4, 1.0, 0.05, 0.3, 1.5, 0.03, 2.0, 0.5])       # the fixtures' (tests/golden/make_golden_hadamard.py)


def subject(N, M, seed=0):
    rng = np.random.default_rng(seed)
    nu = N - N // 5
    base = np.linspace(0.05, 0.95, nu)
    x = np.sort(np.concatenate([base, rng.choice(base, N - nu, replace=False)]))
    indx = rng.integers(0, M, N).astype(np.int32)
    y = np.sin(2.0 * np.pi * x * (indx + 1)) + 0.1 * indx + 0.05 * rng.standard_normal(N)
    T = M * (M + 1) // 2
    p0 = np.concatenate([-2.5 + 0.5 * np.sin(3.0 * x), (0.6 + 0.2 * np.cos(2.0 * x[:, None] + np.arange(T)[None, :])).reshape(-1),
                         [np.log(1e-2)]])
    return x, indx, y, p0


def chains(p0, x, N, T, B):
    out = []
    for k in range(B):
        p = p0.copy()
        p[:N] += 0.02 * np.sin(3.0 * x + 0.4 + k)
        p[N:N + N * T] += (0.02 * np.sin(3.0 * x[:, None] + 0.4 + k + np.arange(T)[None, :])).reshape(-1)
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
    x, indx, y, p0 = subject(N, M)
    c = _lib.Context(0)
    c.had_set_data(x, indx, y)
    if a.one_step:
        for _ in range(2):               # the first builds the prior factors and the workspace
            out, g, st = c.had_batch_eval(chains(p0, x, N, T, a.one_step), HYPER, True, True)
        assert np.all(st == 0)
        print(json.dumps({"one_step_chains": a.one_step, "N": N, "M": M, "neglog0": float(out[0, 0])}), flush=True)
        c.close()
        return
    cpu = {}
    if not a.no_cpu:
        from test_hadamard_cpu import had_logpos
        for mode, key in ((False, "value"), (True, "value_grad")):
            t0 = time.perf_counter()
            had_logpos(p0, x, indx, y, HYPER, grad=mode)
            cpu[key] = 1.0 / (time.perf_counter() - t0)
    lines = []
    for B in [int(v) for v in a.B.split(",")]:
        P = chains(p0, x, N, T, B)
        for mode, key, flop in ((False, "value", float(N) ** 3 / 3.0), (True, "value_grad", float(N) ** 3)):
            c.had_batch_eval(P, HYPER, True, mode)                   # workspace of this B, prior factors
            c.had_batch_eval(P[0], HYPER, True, mode)
            t_b, t_l, ok = [], [], True
            for _ in range(a.reps):
                t0 = time.perf_counter()
                out, g, st = c.had_batch_eval(P, HYPER, True, mode)
                t_b.append(time.perf_counter() - t0)
                ok = ok and bool(np.all(st == 0))
                t0 = time.perf_counter()
                for k in range(B):
                    c.had_batch_eval(P[k], HYPER, True, mode)
                t_l.append(time.perf_counter() - t0)
            tb, tl = float(np.median(t_b)), float(np.median(t_l))
            rec = {"what": "nmgp_had_batch_eval against a loop of single-chain calls, N=%d observations, M=%d, host pointers in and out"
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
