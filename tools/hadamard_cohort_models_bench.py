"""Separable and stationary Hadamard models, a cohort of RAGGED subjects on one GPU: the subject set (nmgp_had_set_subjects, S * k chains
in ONE nmgp_hads_subjects_eval / nmgp_hadst_subjects_eval) against the loop over the existing entries,
    (i)  one set of all S subjects, padded to the largest,
    (ii) the buckets of hadamard.cohort_buckets at its default max_flop_waste, one context and one set per bucket,
    (a)  one context, a loop of had_set_data + hads_batch_eval / hadst_batch_eval (k chains) over the subjects -- the baseline (for the
         separable model the cached prior factors go with every had_set_data).
    python tools/hadamard_cohort_models_bench.py [--M 3] [--S 16] [--lo 512] [--hi 1024] [--seed 7] [--chains 1 8] [--reps 3]
                                                 [--sweeps 3] [--models sep sta] [--out profiles/hadamard_cohort_models_bench.jsonl]
The cohort is tools/hadamard_cohort_bench.py's (same seed, same draws of nobs and subjects).  One sweep evaluates all S * k chains once.
Every shape is warmed up first (prior factors, workspaces); then the arrangements alternate within a repetition (i, ii, a, i, ii, a,
...) in one process, a repetition times `sweeps` sweeps; medians and ranges over the repetitions.  One JSON line per (model, k, value |
value_grad), then one line per model with the stage read-out (nmgp_profile_enable(1)) of ONE 8-chain value + gradient call on the set.
NOT measured: a context per subject (arrangement b of the nonseparable tool), other M or size ranges, max_flop_waste other than the
default, more than one GPU, the MAP drivers end to end."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nonstationary_multivariate_gaussian_process_amd import _lib, drivers, hadamard, hadamard_sep, sim  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--M", type=int, default=3)
ap.add_argument("--S", type=int, default=16)
ap.add_argument("--lo", type=int, default=512)
ap.add_argument("--hi", type=int, default=1024)
ap.add_argument("--seed", type=int, default=7)
ap.add_argument("--chains", type=int, nargs="+", default=[1, 8])
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--sweeps", type=int, default=3)
ap.add_argument("--models", nargs="+", default=["sep", "sta"], choices=["sep", "sta"])
ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
a = ap.parse_args()
M, S = a.M, a.S
rng = np.random.default_rng(a.seed)
nobs = [int(n) for n in rng.integers(a.lo, a.hi + 1, size=S)]
HYPER = {"sep": np.array([float(sim.HYPER_SEP[k]) for k in drivers.SEP_HYPER_KEYS]),
         "sta": np.array([float(sim.HYPER_STA[k]) for k in drivers.STA_HYPER_KEYS])}
SET_EVAL = {"sep": "hads_subjects_eval", "sta": "hadst_subjects_eval"}
ONE_EVAL = {"sep": "hads_batch_eval", "sta": "hadst_batch_eval"}


def subject(n):
    """n single observations: sorted uniform inputs, interleaved labels, y = sin(6 x + label) + noise"""
    x = np.sort(rng.uniform(0.0, 1.0, n))
    indx = (np.arange(n) % M).astype(np.int32)
    return x, indx, np.sin(6.0 * x + indx) + 0.1 * rng.standard_normal(n)


def chain(model, x, j):
    """chain j of a subject: smooth curves (sep) / scalars (sta), L = I + a lower triangle, tilde_sigma2_err = -2"""
    L = np.eye(M) + np.tril(0.3 * np.sin(1.0 + np.arange(M * M).reshape(M, M)))
    Lv = L[np.tril_indices(M)] * (1.0 + 0.02 * j)
    if model == "sta":
        return np.concatenate([[-1.5 + 0.03 * j, 0.1 - 0.02 * j], Lv, [-2.0 + 0.01 * j]])
    return np.concatenate([-1.5 + 0.2 * np.sin(5.0 * x + 0.3 * j), 0.1 * np.cos(4.0 * x + 0.2 * j), Lv, [-2.0 + 0.01 * j]])


def pack(model, vecs, sizes):
    return np.concatenate(vecs, axis=0) if model == "sta" else hadamard_sep.cohort_pack(vecs, sizes, M)


subs = [subject(n) for n in nobs]
buckets = hadamard.cohort_buckets(nobs)
one = _lib.Context(0)                                  # (i), and the loop (a) on the same context: the set does not mind
per_bucket = [_lib.Context(0) for _ in buckets]        # (ii)
one.had_set_subjects([d[0] for d in subs], [d[1] for d in subs], [d[2] for d in subs], M=M)
for c, idx in zip(per_bucket, buckets):
    c.had_set_subjects([subs[s][0] for s in idx], [subs[s][1] for s in idx], [subs[s][2] for s in idx], M=M)
need = float(sum(n ** 3 for n in nobs))
ratio_one = S * max(nobs) ** 3 / need
ratio_buckets = sum(len(idx) * max(nobs[s] for s in idx) ** 3 for idx in buckets) / need


def sweep_set(model, vecs, k, grad):
    out, _, st = getattr(one, SET_EVAL[model])(pack(model, vecs, nobs), HYPER[model], True, grad, k)
    return out[:, 0], st


def sweep_buckets(model, vecs, k, grad):
    val, sts = np.zeros(S * k), np.zeros(S * k, dtype=np.int32)
    for c, idx in zip(per_bucket, buckets):
        out, _, st = getattr(c, SET_EVAL[model])(pack(model, [vecs[s] for s in idx], [nobs[s] for s in idx]), HYPER[model], True, grad, k)
        rows = (np.asarray(idx)[:, None] * k + np.arange(k)[None, :]).reshape(-1)
        val[rows], sts[rows] = out[:, 0], st
    return val, sts


def sweep_a(model, vecs, k, grad):
    outs, sts = [], []
    for d, v in zip(subs, vecs):
        one.had_set_data(*d)
        out, _, st = getattr(one, ONE_EVAL[model])(v, HYPER[model], True, grad)
        outs.append(out[:, 0]), sts.append(st)
    return np.concatenate(outs), np.concatenate(sts)


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


ARRANGEMENTS = (("set", sweep_set), ("buckets", sweep_buckets), ("a", sweep_a))
shapes = [(k, grad, key) for k in a.chains for grad, key in ((False, "value"), (True, "value_grad"))]
for model in a.models:
    vectors = {k: [np.stack([chain(model, d[0], j) for j in range(k)]) for d in subs] for k in a.chains}
    vals = {}
    for k, grad, key in shapes:                        # warm-up of every shape: prior factors, workspaces, first launches
        for name, fn in ARRANGEMENTS:
            v, st = fn(model, vectors[k], k, grad)
            assert np.all(st == 0), (model, name, k, key, st)
            vals[(k, key, name)] = v
        for name in ("buckets", "a"):                  # the arrangements compute the same cohort
            assert np.allclose(vals[(k, key, "set")], vals[(k, key, name)], rtol=1e-6, atol=0.0), (model, name, k, key)
    for k, grad, key in shapes:
        times = {name: [] for name, _ in ARRANGEMENTS}
        for rep in range(a.reps):
            for name, fn in ARRANGEMENTS:
                t0 = time.perf_counter()
                for _ in range(a.sweeps):
                    fn(model, vectors[k], k, grad)
                times[name].append((time.perf_counter() - t0) / a.sweeps)
        med = {name: float(np.median(t)) for name, t in times.items()}
        emit({"model": model, "M": M, "subjects": S, "nobs": nobs, "seed": a.seed, "chains_per_subject": k, "mode": key, "reps": a.reps,
              "sweeps_per_rep": a.sweeps, "buckets": [[int(s) for s in idx] for idx in buckets],
              "flop_ratio_one_set": round(ratio_one, 4), "flop_ratio_buckets": round(ratio_buckets, 4),
              "ms_per_sweep": {n_: round(1e3 * t, 3) for n_, t in med.items()},
              "ms_per_sweep_range": {n_: [round(1e3 * min(ts), 3), round(1e3 * max(ts), 3)] for n_, ts in times.items()},
              "ms_per_sweep_all_reps": {n_: [round(1e3 * t, 3) for t in ts] for n_, ts in times.items()},
              "set_vs_a_set_data_loop": round(med["a"] / med["set"], 3), "buckets_vs_set": round(med["set"] / med["buckets"], 3),
              "build_id": _lib.build_id()})
    # stage read-out of ONE 8-chain value + gradient call on the one set (the event timers serialise the prior stream: the stages'
    # sum is not the call's wall time)
    k = 8
    vec8 = [np.stack([chain(model, d[0], j) for j in range(k)]) for d in subs]
    sweep_set(model, vec8, k, True)
    one.profile_enable(1)
    one.profile_reset()
    t0 = time.perf_counter()
    sweep_set(model, vec8, k, True)
    wall = time.perf_counter() - t0
    stages = {s: {"ms": round(v[0], 3), "launches": v[1]} for s, v in one.profile_read().items() if v[1]}
    one.profile_enable(0)
    emit({"model": model, "stage_readout": "one set, %d chains per subject, value_grad" % k, "wall_ms_with_timers": round(1e3 * wall, 3),
          "stages": stages, "build_id": _lib.build_id()})
