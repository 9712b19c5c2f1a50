"""HMC for a cohort of RAGGED Hadamard subjects on one GPU: the device-resident trajectories (nmgp_had_subjects_traj_*,
drivers.HadamardCohortHMC / HadamardSepCohortHMC / HadamardStaCohortHMC with device_resident=True) against what there was before them,
    resident_set / resident_buckets   the resident loop on one set of all S subjects / on the default buckets (one context each),
    host_set / host_buckets           (i) the host lock-step loop over *_subjects_eval (device_resident=False): its device work is
                                      entirely the evaluation entries', the leapfrog is NumPy with an upload, a download and a
                                      synchronisation per chunk and step,
    per_subject                       (ii) one BatchedHMCHadamard* per subject on ONE context (a had_set_data per visit).
    python tools/hadamard_cohort_hmc_bench.py [--M 3] [--S 16] [--lo 512] [--hi 1024] [--seed 7] [--chains 1 8] [--L 20] [--reps 5]
                                              [--iters 2] [--models non sep sta] [--out profiles/hadamard_cohort_hmc_bench.jsonl]
The cohort is tools/hadamard_cohort_bench.py's (the same seed draws the same nobs and subjects).  Every arrangement is warmed up with
one iteration (prior factors, workspaces, first launches); then the arrangements alternate within a repetition in one process, a
repetition times `iters` HMC iterations of L leapfrog steps (per_subject: one iteration, it is the slow one), and the figures are
medians over the repetitions, with the range.  A run() ends in the trajectory's synchronisation (resident) or the last evaluation's
(host loops), so the host clock around it measures finished work.  One JSON line per (model, k): ms per HMC iteration of each
arrangement, the drivers' own timing split, the stage read-out of one resident trajectory call (nmgp_profile_enable(1), taken after
the timed repetitions), and the library's build id.

EXPECTATIONS, written before the first run (nothing here had been measured):
  * A cohort value+gradient sweep of this cohort takes 1.2-1.7 ms at k = 1 (README), so a step of the host loop at k = 1 is mostly
    round trips: the resident loop should gain MOST at k = 1, and most of all for the stationary model, whose rows are T + 3 = 9
    numbers and whose step is round trips and little else (its factorisations are the same size as the others', so "little else"
    means: no prior solves, a tiny gradient).
  * At k = 8 the evaluation's device time (8x the factorisations) should dominate both loops: a gain of a few percent at most.
  * The nonseparable rows are the widest (Nmax (1 + T) + 1 = 7169 doubles): the host loop's NumPy update and copies are largest there,
    so among the two GP-prior models the nonseparable one should gain more than the separable one.
  * Buckets against one set: as for the evaluation (README: 1.1-1.2x at k = 8, a loss at k = 1 where launches dominate); the resident
    loop does not change that picture.
  * per_subject should be several times slower than either cohort loop at k = 1 (the README's 8-37x per sweep, less the host
    leapfrog both sides pay).
AFTER the run (profiles/hadamard_cohort_hmc_bench.jsonl; host_set / resident_set at k = 1, k = 8): nonseparable 1.47x, 1.64x;
separable 1.10x, 1.12x; stationary 1.07x, 1.015x.  The resident loop was faster at every point.  "Most at k = 1 and for the stationary
model": NOT met -- the stationary model gained least (9-number rows: the host loop's share of its 1.1 ms step is about 0.07 ms), and
the nonseparable model gained more at k = 8 than at k = 1.  "A few percent at most at k = 8": met for the stationary model only; the
host loop's copies and NumPy update of [128, 7169] rows are over a third of its nonseparable step.  "Nonseparable more than separable":
met.  Buckets against one set: one set led at k = 1 (28.0 against 36.4 ms), within 5 % at k = 8.  per_subject: 9.3-9.8x at k = 1,
2.3-2.6x at k = 8 -- met.
NOT measured here: more than one GPU, step-size adaptation, mixing (this is time per iteration at a fixed small step, not effective
samples per second), any mass matrix (identity only), M other than --M."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nonstationary_multivariate_gaussian_process_amd import _lib, drivers, hadamard, sim  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--M", type=int, default=3)
ap.add_argument("--S", type=int, default=16)
ap.add_argument("--lo", type=int, default=512)
ap.add_argument("--hi", type=int, default=1024)
ap.add_argument("--seed", type=int, default=7)
ap.add_argument("--chains", type=int, nargs="+", default=[1, 8])
ap.add_argument("--L", type=int, default=20)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--iters", type=int, default=2)
ap.add_argument("--models", nargs="+", default=["non", "sep", "sta"])
ap.add_argument("--step", type=float, default=1e-4)
ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
a = ap.parse_args()
M, S = a.M, a.S
T = M * (M + 1) // 2
rng = np.random.default_rng(a.seed)
nobs = [int(n) for n in rng.integers(a.lo, a.hi + 1, size=S)]


def subject(n):
    """n single observations: sorted uniform inputs, interleaved labels, y = sin(6 x + label) + noise (hadamard_cohort_bench.py's)"""
    x = np.sort(rng.uniform(0.0, 1.0, n))
    indx = (np.arange(n) % M).astype(np.int32)
    return x, indx, np.sin(6.0 * x + indx) + 0.1 * rng.standard_normal(n)


def chain(model, x, j):
    """chain j of a subject: smooth curves, (rows of) I + a lower triangle, tilde_sigma2_err = -2"""
    L = np.eye(M) + np.tril(0.3 * np.sin(1.0 + np.arange(M * M).reshape(M, M)))
    Lv = L[np.tril_indices(M)]
    tl = -1.5 + 0.2 * np.sin(5.0 * x + 0.3 * j)
    if model == "non":
        return np.concatenate([tl, (Lv[None, :] * (1.0 + 0.1 * np.sin(3.0 * x + 0.2 * j))[:, None]).reshape(-1), [-2.0 + 0.01 * j]])
    if model == "sep":
        return np.concatenate([tl, 0.1 * np.cos(4.0 * x + 0.2 * j), Lv, [-2.0 + 0.01 * j]])
    return np.concatenate([[-1.5 + 0.01 * j, 0.1], Lv, [-2.0 + 0.01 * j]])


subs = [subject(n) for n in nobs]
HYPER = {"non": sim.HYPER_SVC, "sep": sim.HYPER_SEP, "sta": sim.HYPER_STA}
COHORT = {"non": drivers.HadamardCohortHMC, "sep": drivers.HadamardSepCohortHMC, "sta": drivers.HadamardStaCohortHMC}
SINGLE = {"non": drivers.BatchedHMCHadamard, "sep": drivers.BatchedHMCHadamardSep, "sta": drivers.BatchedHMCHadamardSta}
buckets = hadamard.cohort_buckets(nobs)
one_ctx = _lib.Context(0)


class PerSubject:
    """baseline (ii): one per-subject sampler after the other on one context"""

    def __init__(self, model, starts):
        self.s = [SINGLE[model](x, indx, y, HYPER[model], starts[i], step_size=a.step, num_steps_in_leap=a.L, seed=a.seed + i * len(starts[i]),
                                ctx=one_ctx) for i, (x, indx, y) in enumerate(subs)]

    def run(self, n):
        res = [s.run(n) for s in self.s]
        return [r[0] for r in res], {"accept_rate": np.concatenate([r[1]["accept_rate"] for r in res])}

    def close(self):
        pass


def stage_readout(d):
    """the stage timers of ONE resident trajectory call (all buckets of the driver)"""
    for ctx in d.ctxs:
        ctx.lib.nmgp_profile_reset(ctx.h)
        ctx.lib.nmgp_profile_enable(ctx.h, 1)
    d.run(1)
    out = {}
    for ctx in d.ctxs:
        ms = np.zeros(len(_lib.STAGES))
        cnt = np.zeros(len(_lib.STAGES), dtype=np.int64)
        ctx.lib.nmgp_profile_read(ctx.h, _lib.ptr(ms), cnt.ctypes.data_as(_lib.c_ll_p))
        ctx.lib.nmgp_profile_enable(ctx.h, 0)
        for name, t, n in zip(_lib.STAGES, ms, cnt):
            if n:
                out[name] = round(out.get(name, 0.0) + float(t), 3)
    return out


for model in a.models:
    for k in a.chains:
        starts = [np.stack([chain(model, d[0], j) for j in range(k)]) for d in subs]
        mk = lambda resident, waste: COHORT[model](subs, HYPER[model], starts, step_size=a.step, num_steps_in_leap=a.L, seed=a.seed,
                                                   device_resident=resident, max_flop_waste=waste)
        arr = {"resident_set": mk(True, 1e30), "resident_buckets": mk(True, 0.5), "host_set": mk(False, 1e30),
               "host_buckets": mk(False, 0.5), "per_subject": PerSubject(model, starts)}
        assert len(arr["resident_set"].buckets) == 1 and len(arr["resident_buckets"].buckets) == len(buckets)
        first = {}
        for name, d in arr.items():                      # warm-up, and: the arrangements compute the same chains
            samples, info = d.run(1)
            first[name] = samples
            assert np.all(np.isfinite(np.concatenate([v.reshape(-1) for v in samples]))), (model, k, name)
        for name in arr:
            for u, v in zip(first["host_set"], first[name]):
                assert np.allclose(u, v, rtol=1e-6, atol=1e-9), (model, k, name)
        same_bits = all(np.array_equal(u, v) for u, v in zip(first["host_set"], first["resident_set"]))
        times = {name: [] for name in arr}
        split = {name: [] for name in arr if name != "per_subject"}
        for rep in range(a.reps):
            for name, d in arr.items():
                n = 1 if name == "per_subject" else a.iters
                t0 = time.perf_counter()
                _, info = d.run(n)
                times[name].append((time.perf_counter() - t0) / n)
                if name in split:
                    split[name].append({key: info["timing"][key] / n for key in ("setup_seconds", "loop_seconds", "trajectory_call_seconds")})
        med = {name: float(np.median(t)) for name, t in times.items()}
        stages = stage_readout(arr["resident_set"])
        rec = {"model": model, "M": M, "subjects": S, "nobs": nobs, "seed": a.seed, "chains_per_subject": k, "L": a.L, "step": a.step,
               "reps": a.reps, "iters_per_rep": a.iters, "buckets": [[int(s) for s in idx] for idx in buckets],
               "ms_per_iteration": {n_: round(1e3 * t, 3) for n_, t in med.items()},
               "ms_per_iteration_range": {n_: [round(1e3 * min(ts), 3), round(1e3 * max(ts), 3)] for n_, ts in times.items()},
               "host_set_over_resident_set": round(med["host_set"] / med["resident_set"], 3),
               "host_buckets_over_resident_buckets": round(med["host_buckets"] / med["resident_buckets"], 3),
               "per_subject_over_resident_set": round(med["per_subject"] / med["resident_set"], 3),
               "resident_set_equals_host_set_bit_for_bit": bool(same_bits),
               "driver_timing_ms_per_iteration": {n_: {key: round(1e3 * float(np.median([s_[key] for s_ in ss])), 3) for key in ss[0]}
                                                  for n_, ss in split.items()},
               "stage_ms_of_one_resident_set_iteration": stages, "build_id": _lib.build_id()}
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        for d in arr.values():
            d.close()
