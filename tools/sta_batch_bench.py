"""Stationary (LMC) objective, B chains per launch sequence (nmgp_sta_batch_eval), against the two ways there were before it:
    python tools/sta_batch_bench.py [--out profiles/sta_batch_bench.jsonl] [--quick]
Two shapes: BASELINE config 5's (N = 4096, D = 5, one subject; 1 / 16 / 64 chains per call) and N = 1024, D = 5 with 8 subjects
(8 / 16 / 64 chains per call = 1 / 2 / 8 chains per subject: with a subject set a call carries every subject).  Per shape and chain
count, for value and value+gradient evaluations, three methods are timed in the same session, alternating, 3 repetitions each:
    sta_batch   nmgp_sta_batch_eval
    loop_sta    a loop over nmgp_logpos_sta, one parameter vector per call (with 8 subjects: nmgp_set_data per subject, then its chains)
    sep_batch   nmgp_sep_batch_eval with constant curves and prior = 0 (the same likelihood through the separable entry)
One JSON line per (shape, chains): the median evaluations / s of each method and mode, the three repetitions, and the stage read-out
(nmgp_profile_enable(1)) of one further sta_batch call made after the timed ones.  A time is a host clock around calls that end in a
stream synchronisation; every method is warmed up at every shape before its first timed call.  --quick: small shapes, to rehearse."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nonstationary_multivariate_gaussian_process_amd import _lib, sim  # noqa: E402

STA_KEYS = ("mu_tilde_l", "sigma_tilde_l", "a", "b", "c")
SEP_KEYS = ("mu_tilde_l", "alpha_tilde_l", "beta_tilde_l", "mu_tilde_sigma", "alpha_tilde_sigma", "beta_tilde_sigma", "a", "b", "c")
MIN_WINDOW_S = 0.25          # calls are repeated until a timed window is at least this long


def timed(call):
    """seconds per call: one call to size the window, then enough calls for MIN_WINDOW_S (at most 50)"""
    t0 = time.perf_counter()
    call()
    first = time.perf_counter() - t0
    n = int(min(50, max(1, np.ceil(MIN_WINDOW_S / max(first, 1e-6)))))
    if n == 1:
        return first
    t0 = time.perf_counter()
    for _ in range(n):
        call()
    return (time.perf_counter() - t0) / n


def bench_shape(ctx, N, M, S, chain_counts, out_f):
    subs = [sim.simulate_stationary(N, M, 8 + s) for s in range(S)]
    xs, Ys = np.stack([d["x"] for d in subs]), np.stack([d["Y"] for d in subs])
    hv = np.array([sim.HYPER_STA[k] for k in STA_KEYS])
    hs = np.array([sim.HYPER_SEP[k] for k in SEP_KEYS])
    for B in chain_counts:
        assert B % S == 0, "with %d subjects a call carries a multiple of %d chains" % (S, S)
        cps = B // S
        pars = np.stack([sim.perturb(subs[b // cps]["pars_true"], 0.05, 0.4 + 0.1 * b) for b in range(B)])
        sep = np.stack([np.concatenate([np.full(N, p[0]), np.full(N, p[1]), p[2:]]) for p in pars])

        def subjects_on():
            ctx.set_data(xs[0], Ys[0])
            if S > 1:
                ctx.sta_batch_set_subjects(xs, Ys, cps)       # (one set: the separable entry reads it too)

        def run_sta(grad):
            out, g, st = ctx.sta_batch_eval(pars, hv, True, grad)
            assert np.all(st == 0)

        def run_sep(grad):
            out, g, st = ctx.sep_batch_eval(sep, hs, False, grad)
            assert np.all(st == 0)

        def run_loop(grad):
            for s in range(S):
                if S > 1:
                    ctx.set_data(xs[s], Ys[s])
                for p in pars[s * cps:(s + 1) * cps]:
                    ctx.logpos_sta(p, hv, True, grad)

        rec = {"N": N, "M": M, "subjects": S, "chains": B, "window_s": MIN_WINDOW_S}
        for grad, key in ((False, "value"), (True, "value_grad")):
            reps = {"sta_batch": [], "loop_sta": [], "sep_batch": []}
            subjects_on()
            run_sta(grad), run_sep(grad)                      # warm-up at this shape (first use builds the separable prior factors)
            run_loop(grad)
            for _ in range(3):                                # alternating: a drift of the machine hits every method alike
                subjects_on()
                run_sta(grad), run_sep(grad)                  # (a fresh subject set: its separable prior factors are built here)
                reps["sta_batch"].append(B / timed(lambda: run_sta(grad)))
                reps["sep_batch"].append(B / timed(lambda: run_sep(grad)))
                reps["loop_sta"].append(B / timed(lambda: run_loop(grad)))
            subjects_on()
            ctx.profile_enable(True)
            ctx.profile_reset()
            run_sta(grad)
            stages = {k: round(v[0], 3) for k, v in ctx.profile_read().items() if v[1]}
            ctx.profile_enable(False)
            med = {k: float(np.median(v)) for k, v in reps.items()}
            rec[key] = {"evals_per_s": med, "evals_per_s_reps": reps, "sta_batch_over_loop_sta": med["sta_batch"] / med["loop_sta"],
                        "sta_batch_over_sep_batch": med["sta_batch"] / med["sep_batch"], "sta_batch_stage_ms_per_call": stages}
        line = json.dumps(rec)
        print(line, flush=True)
        out_f.write(line + "\n")
        out_f.flush()


def main(argv):
    out = os.path.join(ROOT, "profiles", "sta_batch_bench.jsonl")
    if "--out" in argv:
        out = argv[argv.index("--out") + 1]
    quick = "--quick" in argv
    ctx = _lib.Context(0)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        if quick:
            bench_shape(ctx, 96, 3, 1, [1, 4], f)
            bench_shape(ctx, 64, 3, 2, [2, 4], f)
        else:
            bench_shape(ctx, 4096, 5, 1, [1, 16, 64], f)
            bench_shape(ctx, 1024, 5, 8, [8, 16, 64], f)
    ctx.close()


if __name__ == "__main__":
    main(sys.argv[1:])
