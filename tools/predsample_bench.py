"""Posterior-draw prediction at the headline size: N = 2048, D = 3, the reference's 201-point grid, H draws = the sampler's
`pars_typical` positions (tests/golden/hmc_state_N2048_M3_seed2222.npz) repeated with a small jitter.
    python tools/predsample_bench.py [--H 1,8,32,128] [--reps 3] [--grid 201] [--only-entry]
Times, in one process and alternating, nmgp_predsample_svc (all draws in one call) and what the library offered before it: a loop
of H nmgp_predict_svc calls (one parameter vector each, conditional means instead of samples).  One JSON line per H: ms per draw
on both sides (median and every repetition), the chunk size the entry used, the library's build id.
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

SVC_KEYS = ("mu_tilde_l", "alpha_tilde_l", "beta_tilde_l", "mu_L", "alpha_L", "beta_L", "a", "b")


def chunk_size(H, n, E):
    """The entry's rule (nmgp.h): NMGP_PREDSAMPLE_CHUNK, else what keeps the factorisation buffers below NMGP_PREDSAMPLE_SLAB_GB
    (default 16), at most 64."""
    B = int(os.environ.get("NMGP_PREDSAMPLE_CHUNK", "0") or 0)
    if B <= 0:
        ld = (n + 1 + E + 15) // 16 * 16
        slab = max(1, int(os.environ.get("NMGP_PREDSAMPLE_SLAB_GB", "16") or 16)) * 2.0 ** 30
        B = int(min(64.0, slab / (8.0 * ld * n)))
    return max(1, min(B, H))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--H", default="1,8,32,128")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--grid", type=int, default=201)
    ap.add_argument("--only-entry", action="store_true")
    a = ap.parse_args()
    N, M = 2048, 3
    T = M * (M + 1) // 2
    n = N * M
    d = sim.simulate_nonseparable(N, M, seed=2222)
    typical = np.load(os.path.join(ROOT, "tests", "golden", "hmc_state_N2048_M3_seed2222.npz"))["pars_typical"]
    hv = np.array([sim.HYPER_SVC[k] for k in SVC_KEYS])
    xs = np.linspace(0.0, 1.0, a.grid)
    c = _lib.Context(0)
    c.set_data(d["x"], d["Y"])
    rng = np.random.default_rng(0)
    for H in [int(v) for v in a.H.split(",")]:
        draws = np.stack([typical[k % len(typical)] + 1e-3 * rng.standard_normal(typical.shape[1]) for k in range(H)])
        z = rng.standard_normal((H, a.grid, 1 + T))
        c.predsample_svc(draws[:min(H, 2)], hv, xs, z=z[:min(H, 2)])            # prior factors
        if not a.only_entry:
            c.predsample_svc(draws, hv, xs, z=z)                                   # workspace of this H
            c.predict_svc(draws[0], hv, xs)
        t_new, t_loop, ok = [], [], True
        for _ in range(a.reps):
            t0 = time.perf_counter()
            mean, var, star, status = c.predsample_svc(draws, hv, xs, z=z)
            t_new.append((time.perf_counter() - t0) / H)
            ok = ok and bool(np.all(status == 0) and np.all(var > 0))
            if not a.only_entry:
                t0 = time.perf_counter()
                for h in range(H):
                    c.predict_svc(draws[h], hv, xs)
                t_loop.append((time.perf_counter() - t0) / H)
        rec = {"what": "nmgp_predsample_svc against a loop of nmgp_predict_svc, N=%d, D=%d, %d grid points, host pointers in and out"
                       % (N, M, a.grid), "H": H, "chunk": chunk_size(H, n, min(a.grid * M, n)),
               "entry_ms_per_draw": 1e3 * float(np.median(t_new)), "entry_ms_per_draw_reps": [1e3 * t for t in t_new],
               "all_draws_ok": ok, "library_build_id": _lib.build_id()}
        if t_loop:
            rec.update(loop_ms_per_draw=1e3 * float(np.median(t_loop)), loop_ms_per_draw_reps=[1e3 * t for t in t_loop],
                       loop_over_entry=float(np.median(t_loop) / np.median(t_new)))
        print(json.dumps(rec), flush=True)
    c.close()


if __name__ == "__main__":
    main()
