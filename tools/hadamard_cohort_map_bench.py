"""MAP by Adam for a cohort of RAGGED Hadamard subjects on one GPU: the device-resident optimiser (nmgp_had_subjects_adam_*,
drivers.HadamardCohortMAP / HadamardSepCohortMAP / HadamardStaCohortMAP with device_resident=True) against what there was before it,
    resident_set_1 / _10 / _50        the resident loop on one set of all S subjects at iters_per_call 1, 10 and 50,
    resident_buckets                  the resident loop on the default buckets (one context each) at iters_per_call 50,
    host_set / host_buckets           (i) the host lock-step loop over *_subjects_eval (device_resident=False): an upload of the
                                      parameter rows, a download of the gradient rows and a synchronisation per chunk and iteration,
                                      Adam's update of P, m and v in NumPy,
    per_subject                       (ii) one HadamardMAP / HadamardSepMAP / HadamardStaMAP per subject on ONE context (a
                                      had_set_data per visit).
    python tools/hadamard_cohort_map_bench.py [--M 3] [--S 16] [--lo 512] [--hi 1024] [--seed 7] [--chains 1 8] [--reps 5]
                                              [--iters 50] [--models non sep sta] [--out profiles/hadamard_cohort_map_bench.jsonl]
The cohort is tools/hadamard_cohort_bench.py's (the same seed draws the same nobs and subjects).  Every arrangement is warmed up with
two iterations (prior factors, workspaces, first launches); then the arrangements alternate within a repetition in one process, a
repetition times `iters` Adam iterations (per_subject: 5, it is the slow one), and the figures are medians over the repetitions, with
the range.  A run() ends in a synchronisation (the call's, the parameter fetch, or the last evaluation's), so the host clock around it
measures finished work.  One JSON line per (model, k): ms per Adam iteration of each arrangement, the stage read-out of one resident
block of `iters` iterations (nmgp_profile_enable(1), taken after the timed repetitions), and the library's build id.

EXPECTATIONS, written before the first run (nothing here had been measured; the HMC tool's figures for the same host work are known:
per 20 evaluations 41.0 against 28.0 ms at k = 1 and 228 against 139 ms at k = 8 for the nonseparable model):
  * The gain of resident_set_50 over host_set is LARGEST for the nonseparable model, whose rows are 7169 doubles wide.
  * The gain is a few percent at most for the stationary model (9-number rows).
  * The gain grows from iters_per_call 1 to 10 and flattens by 50.
AFTER the run: see profiles/hadamard_cohort_map_bench.jsonl and README ("Hadamard cohort MAP on the device"), where each expectation
is reported as met or not met.
NOT measured here: more than one GPU, convergence (this is time per iteration, not iterations to a tolerance), learning rates other
than --lr, M other than --M, cohorts that need more than one chunk."""
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
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--models", nargs="+", default=["non", "sep", "sta"])
ap.add_argument("--lr", type=float, default=1e-3)
ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
a = ap.parse_args()
M, S = a.M, a.S
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
COHORT = {"non": drivers.HadamardCohortMAP, "sep": drivers.HadamardSepCohortMAP, "sta": drivers.HadamardStaCohortMAP}
SINGLE = {"non": drivers.HadamardMAP, "sep": drivers.HadamardSepMAP, "sta": drivers.HadamardStaMAP}
buckets = hadamard.cohort_buckets(nobs)
one_ctx = _lib.Context(0)
PER_SUBJECT_ITERS = 5


class PerSubject:
    """baseline (ii): one per-subject optimiser after the other on one context"""

    def __init__(self, model, starts):
        self.s = [SINGLE[model](x, indx, y, HYPER[model], starts[i], lr=a.lr, ctx=one_ctx) for i, (x, indx, y) in enumerate(subs)]

    def run(self, n):
        res = [s.run(n) for s in self.s]
        return [r[0] for r in res], np.concatenate([r[1] for r in res], axis=1), np.concatenate([r[2] for r in res])

    def close(self):
        pass


class Resident:
    """one resident driver run at a given iters_per_call (the three settings share the driver, its contexts and its state)"""

    def __init__(self, d, per_call):
        self.d, self.per_call = d, per_call

    def run(self, n):
        self.d.iters_per_call = self.per_call
        return self.d.run(n)

    def close(self):
        pass


def stage_readout(d, n):
    """the stage timers of ONE resident block of n iterations (all buckets of the driver)"""
    for ctx in d.ctxs:
        ctx.lib.nmgp_profile_reset(ctx.h)
        ctx.lib.nmgp_profile_enable(ctx.h, 1)
    d.iters_per_call = n
    d.run(n)
    out = {}
    for ctx in d.ctxs:
        ms = np.zeros(len(_lib.STAGES))
        cnt = np.zeros(len(_lib.STAGES), dtype=np.int64)
        ctx.lib.nmgp_profile_read(ctx.h, _lib.ptr(ms), cnt.ctypes.data_as(_lib.c_ll_p))
        ctx.lib.nmgp_profile_enable(ctx.h, 0)
        for name, t, c in zip(_lib.STAGES, ms, cnt):
            if c:
                out[name] = round(out.get(name, 0.0) + float(t), 3)
    return out


for model in a.models:
    for k in a.chains:
        starts = [np.stack([chain(model, d[0], j) for j in range(k)]) for d in subs]
        mk = lambda resident, waste: COHORT[model](subs, HYPER[model], starts, lr=a.lr, chains_per_subject=k, max_flop_waste=waste,
                                                   device_resident=resident, iters_per_call=50)
        rset = mk(True, 1e30)
        own = [rset, mk(True, 0.5), mk(False, 1e30), mk(False, 0.5)]
        arr = {"resident_set_1": Resident(rset, 1), "resident_set_10": Resident(rset, 10), "resident_set_50": Resident(rset, 50),
               "resident_buckets": own[1], "host_set": own[2], "host_buckets": own[3], "per_subject": PerSubject(model, starts)}
        assert len(rset.buckets) == 1 and len(own[1].buckets) == len(buckets)
        first = {}
        for name in ("resident_set_50", "resident_buckets", "host_set", "host_buckets", "per_subject"):      # warm-up, and: the same chains
            pars, hist, alive = arr[name].run(2)
            first[name] = hist
            assert alive.all() and np.all(np.isfinite(hist)), (model, k, name)
        for name, h in first.items():
            assert np.allclose(h, first["host_set"], rtol=1e-6, atol=1e-9), (model, k, name)
        same_bits = bool(np.array_equal(first["host_set"], first["resident_set_50"]))
        times = {name: [] for name in arr}
        for rep in range(a.reps):
            for name, d in arr.items():
                n = PER_SUBJECT_ITERS if name == "per_subject" else a.iters
                t0 = time.perf_counter()
                d.run(n)
                times[name].append((time.perf_counter() - t0) / n)
        med = {name: float(np.median(t)) for name, t in times.items()}
        stages = stage_readout(rset, a.iters)
        rec = {"model": model, "M": M, "subjects": S, "nobs": nobs, "seed": a.seed, "chains_per_subject": k, "lr": a.lr, "reps": a.reps,
               "iters_per_rep": a.iters, "per_subject_iters_per_rep": PER_SUBJECT_ITERS,
               "buckets": [[int(s) for s in idx] for idx in buckets],
               "ms_per_iteration": {n_: round(1e3 * t, 4) for n_, t in med.items()},
               "ms_per_iteration_range": {n_: [round(1e3 * min(ts), 4), round(1e3 * max(ts), 4)] for n_, ts in times.items()},
               "host_set_over_resident_set": {str(c): round(med["host_set"] / med["resident_set_%d" % c], 3) for c in (1, 10, 50)},
               "host_buckets_over_resident_buckets": round(med["host_buckets"] / med["resident_buckets"], 3),
               "per_subject_over_resident_set_50": round(med["per_subject"] / med["resident_set_50"], 3),
               "resident_set_equals_host_set_bit_for_bit": same_bits,
               "stage_ms_of_one_resident_set_block": stages, "build_id": _lib.build_id()}
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        for d in own:
            d.close()
