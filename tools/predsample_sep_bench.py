"""Posterior-draw prediction of the separable and the stationary model at config 5's shape: N = 4096, D = 5, the reference's
201-point grid, H draws around the parameters of tests/golden/sep_sim_N4096_M5.npz (stationary: around the simulator's).
    python tools/predsample_sep_bench.py [--H 1,8,32,128] [--reps 3] [--grid 201] [--model sep,sta] [--only-entry] [--out FILE]
Times, in one process and alternating, the entry (nmgp_predsample_sep / _sta: all draws in one call) and what the library offered
before it: a loop of H nmgp_predict_sep / _sta calls (one parameter vector each, conditional means instead of samples).  Every
shape is warmed up on both sides first.  One JSON line per model and H: ms per draw on both sides (median and every repetition),
whether the entry's per-draw median lies below the loop's by more than the spread of the repetitions of that run, the chunk size
the entry used, the library's build id.  --out appends the lines to a file as well.
--only-entry skips the loop and the warm-up of it: the form to run under `rocprofv3 --kernel-trace --stats` for one chunk."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nonstationary_multivariate_gaussian_process_amd import _lib, sim  # noqa: E402


def chunk_size(H, N, M, S):
    """The entry's rule (nmgp.h): NMGP_PREDSAMPLE_CHUNK, else what keeps the factorisation buffers below NMGP_PREDSAMPLE_SLAB_GB
    (default 16), at most 64."""
    B = int(os.environ.get("NMGP_PREDSAMPLE_CHUNK", "0") or 0)
    if B <= 0:
        ld = (N + 1 + min(S, max(1, N - 2)) + 15) // 16 * 16
        slab = max(1, int(os.environ.get("NMGP_PREDSAMPLE_SLAB_GB", "16") or 16)) * 2.0 ** 30
        B = int(min(64.0, slab / (8.0 * M * ld * N)))
    return max(1, min(B, H))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--H", default="1,8,32,128")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--grid", type=int, default=201)
    ap.add_argument("--model", default="sep,sta")
    ap.add_argument("--only-entry", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    g = np.load(os.path.join(ROOT, "tests", "golden", "sep_sim_N4096_M5.npz"))
    x, Y, p_sep, hv = g["x"], g["Y"], g["pars"], g["hyper"]
    N, M = Y.shape
    T = M * (M + 1) // 2
    p_sta = np.concatenate([[-1.0, 0.5], p_sep[2 * N:]])
    xs = np.linspace(0.0, 1.0, a.grid)
    c = _lib.Context(0)
    c.set_data(x, Y)
    rng = np.random.default_rng(0)
    sides = {"sep": (lambda d, z: c.predsample_sep(d, hv, xs, z=z)[1::2], lambda p: c.predict_sep(p, hv, xs), p_sep),
             "sta": (lambda d, z: c.predsample_sta(d, xs)[1:], lambda p: c.predict_sta(p, xs), p_sta)}
    for model in a.model.split(","):
        entry, single, p0 = sides[model]
        for H in [int(v) for v in a.H.split(",")]:
            draws = np.stack([p0 + 1e-3 * rng.standard_normal(p0.shape[0]) for _ in range(H)])
            z = rng.standard_normal((H, a.grid, 2))
            entry(draws[:1], z[:1])                                                 # prior factors
            if not a.only_entry:
                entry(draws, z)                                                     # workspace of this H
                single(draws[0])
            t_new, t_loop, ok = [], [], True
            for _ in range(a.reps):
                t0 = time.perf_counter()
                var, status = entry(draws, z)
                t_new.append((time.perf_counter() - t0) / H)
                ok = ok and bool(np.all(status == 0) and np.all(var > 0))
                if not a.only_entry:
                    t0 = time.perf_counter()
                    for h in range(H):
                        single(draws[h])
                    t_loop.append((time.perf_counter() - t0) / H)
            rec = {"what": "nmgp_predsample_%s against a loop of nmgp_predict_%s, N=%d, D=%d, %d grid points, host pointers in and out"
                           % (model, model, N, M, a.grid), "model": model, "H": H, "chunk": chunk_size(H, N, M, a.grid),
                   "entry_ms_per_draw": 1e3 * float(np.median(t_new)), "entry_ms_per_draw_reps": [1e3 * t for t in t_new],
                   "all_draws_ok": ok, "library_build_id": _lib.build_id()}
            if t_loop:
                spread = 1e3 * max(max(t_new) - min(t_new), max(t_loop) - min(t_loop))
                gain = 1e3 * float(np.median(t_loop) - np.median(t_new))
                rec.update(loop_ms_per_draw=1e3 * float(np.median(t_loop)), loop_ms_per_draw_reps=[1e3 * t for t in t_loop],
                           loop_over_entry=float(np.median(t_loop) / np.median(t_new)), spread_ms=spread,
                           entry_faster_beyond_spread=bool(gain > spread), entry_not_slower_beyond_spread=bool(gain > -spread))
            line = json.dumps(rec)
            print(line, flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")
    c.close()


if __name__ == "__main__":
    main()
