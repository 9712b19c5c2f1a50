"""Posterior-draw and held-out prediction of the nonseparable Hadamard model on the subject of tools/hadamard_bench.py: N = 6144
single observations, M = 3, the reference's 201-point grid (all outputs) and 1536 held-out (x, label) pairs (the indexed form).
    python tools/predsample_had_bench.py [--N 6144] [--H 1,16,128] [--reps 3] [--grid 201] [--test 1536] [--form full,indexed]
                                         [--only-entry] [--out profiles/predsample_had_bench.jsonl]
Times, in one process and alternating, the entry (nmgp_predsample_had: all draws in one call) and what the library offered before
it: a loop of H nmgp_predict_had calls on the same draws (one parameter vector each, conditional means instead of samples; the loop
has no indexed form: for the held-out pairs it predicts all M outputs at the held-out inputs, of which a caller would keep one per
input).  Every shape is warmed up on both sides first; a call ends in the entry's own device synchronisation, so the host clock
around it is the call time.  One JSON line per form and H: ms per draw on both sides (median and every repetition), whether the
entry's per-draw median lies below the loop's by more than the spread of the repetitions of that run, the chunk size the entry
used, the library's build id.  The H = 16 line also carries the per-stage HIP-event read-out (nmgp_profile_enable(1)) of ONE more
call of the entry, made after the timed ones: where a call's time goes.  --out appends the lines to a file as well.  --only-entry
skips the loop and its warm-up."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from hadamard_bench import HYPER, chains, subject  # noqa: E402  (the same x, indx, y and starting point)
from nonstationary_multivariate_gaussian_process_amd import _lib  # noqa: E402
from predsample_hadamard_bench import chunk_size  # noqa: E402  (the entries share the chunking rule)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=6144)
    ap.add_argument("--M", type=int, default=3)
    ap.add_argument("--H", default="1,16,128")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--grid", type=int, default=201)
    ap.add_argument("--test", type=int, default=1536)
    ap.add_argument("--form", default="full,indexed")
    ap.add_argument("--only-entry", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    N, M = a.N, a.M
    T = M * (M + 1) // 2
    x, indx, y, p0 = subject(N, M)
    rng = np.random.default_rng(0)
    forms = {"full": (np.linspace(0.0, 1.0, a.grid), None),
             "indexed": (np.sort(rng.uniform(0.05, 0.95, a.test)), rng.integers(0, M, a.test).astype(np.int32))}
    c = _lib.Context(0)
    c.had_set_data(x, indx, y)
    for form in a.form.split(","):
        xs, lab = forms[form]
        S = xs.shape[0]
        E = min(S, N) if lab is not None else min(S, max(1, N // M)) * M
        for H in [int(v) for v in a.H.split(",")]:
            draws = chains(p0, x, N, T, H)
            z = rng.standard_normal((H, S, 1 + T))
            c.predsample_had(draws[:1], HYPER, xs, indx_star=lab, z=z[:1])           # prior factors
            if not a.only_entry:
                c.predsample_had(draws, HYPER, xs, indx_star=lab, z=z)               # workspace of this H
                c.predict_had(draws[0], HYPER, xs)
            t_new, t_loop, ok = [], [], True
            for _ in range(a.reps):
                t0 = time.perf_counter()
                _, var, _, status = c.predsample_had(draws, HYPER, xs, indx_star=lab, z=z)
                t_new.append((time.perf_counter() - t0) / H)
                ok = ok and bool(np.all(status == 0) and np.all(var > 0))
                if not a.only_entry:
                    t0 = time.perf_counter()
                    for h in range(H):
                        c.predict_had(draws[h], HYPER, xs)
                    t_loop.append((time.perf_counter() - t0) / H)
            rec = {"what": "nmgp_predsample_had (%s form) against a loop of nmgp_predict_had (all M outputs at every input), N=%d "
                           "observations, M=%d, %d new inputs, host pointers in and out" % (form, N, M, S), "form": form, "H": H,
                   "riding_rows_entry": 1 + E, "riding_rows_loop": 1 + min(S, max(1, N // M)) * M, "chunk": chunk_size(H, N, E),
                   "entry_ms_per_draw": 1e3 * float(np.median(t_new)), "entry_ms_per_draw_reps": [1e3 * t for t in t_new],
                   "all_draws_ok": ok, "library_build_id": _lib.build_id()}
            if t_loop:
                spread = 1e3 * max(max(t_new) - min(t_new), max(t_loop) - min(t_loop))
                gain = 1e3 * float(np.median(t_loop) - np.median(t_new))
                rec.update(loop_ms_per_draw=1e3 * float(np.median(t_loop)), loop_ms_per_draw_reps=[1e3 * t for t in t_loop],
                           loop_over_entry=float(np.median(t_loop) / np.median(t_new)), spread_ms=spread,
                           entry_faster_beyond_spread=bool(gain > spread), entry_not_slower_beyond_spread=bool(gain > -spread))
            if H == 16:
                c.profile_enable(1)
                c.profile_reset()
                t0 = time.perf_counter()
                c.predsample_had(draws, HYPER, xs, indx_star=lab, z=z)
                wall = 1e3 * (time.perf_counter() - t0)
                rec["stages_of_one_call_ms"] = {k: v[0] for k, v in c.profile_read().items() if v[1]}
                rec["stages_call_wall_ms"] = wall
                c.profile_enable(0)
            line = json.dumps(rec)
            print(line, flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")
    c.close()


if __name__ == "__main__":
    main()
