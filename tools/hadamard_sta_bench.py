"""Hadamard stationary objective and predictor on the subject of tools/hadamard_bench.py: N = 6144 single observations, M = 3.
    python tools/hadamard_sta_bench.py [--N 6144] [--B 1,16,64] [--H 1,16,128] [--reps 3] [--out FILE]
    python tools/hadamard_sta_bench.py --one-step 16 [--entry hadst|hads]
        # a warm-up and ONE value+gradient step of 16 chains: the form to run under
        # `rocprofv3 --kernel-trace --stats -- python3 tools/hadamard_sta_bench.py --one-step 16`
Times nmgp_hadst_batch_eval (B chains in one launch sequence) for value and value+gradient, ALTERNATING in every repetition with the
two existing entries on the same resident subject: nmgp_had_batch_eval (nonseparable) and nmgp_hads_batch_eval (separable).  The
comparison is against those entries, never against the new code itself.  One JSON line per (B, mode): medians over the repetitions.
Then nmgp_predict_hadst on the 201-point grid at H draws in one call against a loop of single-draw calls (the loop is timed on at
most 16 draws and reported per draw).  The matrix order, the factorisation and the inverse are the same in all three models; the
stationary one has no GP prior and so no prior solve."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import hadamard_bench as hb  # noqa: E402  (the same x, indx, y; the nonseparable start and chains)
import hadamard_sep_bench as hsb  # noqa: E402  (the separable start and chains)
from nonstationary_multivariate_gaussian_process_amd import _lib  # noqa: E402

HYPER = np.array([-2.0, 0.7, 2.0, 0.5, 3.0])       # the fixtures' (tests/golden/make_golden_hadamard_sta.py)


def start(N, M):
    x, indx, y, p_sep = hsb.start(N, M)
    T = M * (M + 1) // 2
    return np.concatenate([[-2.3, 0.1], p_sep[2 * N:2 * N + T], [np.log(1e-2)]])


def chains(p0, B):
    k = np.arange(B)[:, None]
    P = p0[None] + 0.02 * np.sin(0.7 + k + np.arange(p0.shape[0])[None])
    P[:, -1] = p0[-1]
    return np.ascontiguousarray(P)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=6144)
    ap.add_argument("--M", type=int, default=3)
    ap.add_argument("--B", default="1,16,64")
    ap.add_argument("--H", default="1,16,128")
    ap.add_argument("--grid", type=int, default=201)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--one-step", type=int, default=0)
    ap.add_argument("--entry", default="hadst", choices=["hadst", "hads"])
    a = ap.parse_args()
    N, M = a.N, a.M
    T = M * (M + 1) // 2
    x, indx, y, p_svc = hb.subject(N, M)
    _, _, _, p_sep = hsb.start(N, M)
    p_sta = start(N, M)
    c = _lib.Context(0)
    c.had_set_data(x, indx, y)
    entries = {
        "had": lambda B, g: c.had_batch_eval(hb.chains(p_svc, x, N, T, B), hb.HYPER, True, g),
        "hads": lambda B, g: c.hads_batch_eval(hsb.chains(p_sep, x, N, T, B), hsb.HYPER, True, g),
        "hadst": lambda B, g: c.hadst_batch_eval(chains(p_sta, B), HYPER, True, g),
    }
    if a.one_step:
        for _ in range(2):               # the first builds the workspace (and the separable entry's prior factors)
            out, g, st = entries[a.entry](a.one_step, True)
        assert np.all(st == 0)
        print(json.dumps({"one_step_chains": a.one_step, "entry": a.entry, "N": N, "M": M, "neglog0": float(out[0, 0])}), flush=True)
        c.close()
        return
    lines = []

    def emit(rec):
        rec["library_build_id"] = _lib.build_id()
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))

    for B in [int(v) for v in a.B.split(",")]:
        pars = {"had": hb.chains(p_svc, x, N, T, B), "hads": hsb.chains(p_sep, x, N, T, B), "hadst": chains(p_sta, B)}
        calls = {"had": lambda g: c.had_batch_eval(pars["had"], hb.HYPER, True, g),
                 "hads": lambda g: c.hads_batch_eval(pars["hads"], hsb.HYPER, True, g),
                 "hadst": lambda g: c.hadst_batch_eval(pars["hadst"], HYPER, True, g)}
        for mode, key in ((False, "value"), (True, "value_grad")):
            for f in calls.values():                                   # workspace of this B, prior factors
                f(mode)
            times = {k: [] for k in calls}
            ok = True
            for _ in range(a.reps):
                for k, f in calls.items():                             # alternating within every repetition
                    t0 = time.perf_counter()
                    out, g, st = f(mode)
                    times[k].append(time.perf_counter() - t0)
                    ok = ok and bool(np.all(st == 0))
            med = {k: float(np.median(v)) for k, v in times.items()}
            emit({"what": "nmgp_hadst_batch_eval alternating with nmgp_had_batch_eval and nmgp_hads_batch_eval on one resident subject, "
                          "N=%d observations, M=%d, host pointers in and out; medians of %d" % (N, M, a.reps),
                  "B": B, "mode": key, "evals_per_s": {k: B / v for k, v in med.items()},
                  "ms_reps": {k: [1e3 * t for t in v] for k, v in times.items()},
                  "hadst_over_had": med["had"] / med["hadst"], "hadst_over_hads": med["hads"] / med["hadst"],
                  "roofline_frac_hadst": B * (float(N) ** 3 / (1.0 if mode else 3.0)) / med["hadst"] / hb.PEAK,
                  "roofline_flop_per_eval": "N^3" if mode else "N^3/3", "all_chains_ok": ok})
    xs = np.linspace(0.0, 1.0, a.grid)
    for H in [int(v) for v in a.H.split(",") if int(v) > 0]:
        draws = chains(p_sta, H)
        nl = min(H, 16)
        c.predict_hadst(draws, xs)                                     # workspace of this H
        c.predict_hadst(draws[0], xs)
        t_b, t_l, ok = [], [], True
        for _ in range(a.reps):
            t0 = time.perf_counter()
            mean, var, st = c.predict_hadst(draws, xs)
            t_b.append(time.perf_counter() - t0)
            ok = ok and bool(np.all(st == 0))
            t0 = time.perf_counter()
            for k in range(nl):
                c.predict_hadst(draws[k], xs)
            t_l.append(time.perf_counter() - t0)
        tb, tl = float(np.median(t_b)), float(np.median(t_l))
        emit({"what": "nmgp_predict_hadst, H draws in one call against a loop of single-draw calls (the loop timed on %d draws), N=%d, "
                      "M=%d, %d grid points, all outputs; medians of %d" % (nl, N, M, a.grid, a.reps),
              "H": H, "batch_ms_per_draw": 1e3 * tb / H, "loop_ms_per_draw": 1e3 * tl / nl, "batch_over_loop": (tl / nl) / (tb / H),
              "batch_ms_reps": [1e3 * t for t in t_b], "loop_ms_reps": [1e3 * t for t in t_l], "all_draws_ok": ok})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    c.close()


if __name__ == "__main__":
    main()
