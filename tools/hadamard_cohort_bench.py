"""Hadamard nonseparable model, a cohort of RAGGED subjects on one GPU: the subject set (nmgp_had_set_subjects: S subjects padded to
Nmax, S * k chains in ONE nmgp_had_subjects_eval) against what there was before it,
    (i)  one set of all S subjects, padded to the largest,
    (ii) the buckets of hadamard.cohort_buckets at its default max_flop_waste, one context and one set per bucket,
    (a)  one context, a loop of had_set_data + had_batch_eval(k chains) over the subjects (the cached prior factors go with every
         had_set_data),
    (b)  S contexts, each keeping its subject resident, evaluated one after the other.
    python tools/hadamard_cohort_bench.py [--M 3] [--S 16] [--lo 512] [--hi 1024] [--seed 7] [--chains 1 8] [--reps 3] [--sweeps 3]
                                          [--out profiles/hadamard_cohort_bench.jsonl]
nobs is drawn once from the seed, uniform in [lo, hi].  One sweep evaluates all S * k chains once.  Every shape is warmed up first (prior
factors, workspaces); then the arrangements alternate within a repetition (i, ii, a, b, i, ii, a, b, ...) in one process, a repetition
times `sweeps` sweeps, and the figures are medians over the repetitions.  One JSON line per (k, value | value_grad): ms per sweep of
each arrangement, the flop ratios S Nmax^3 / sum N_s^3 of (i) and of (ii), and the library's build id."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nonstationary_multivariate_gaussian_process_amd import _lib, hadamard, sim  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--M", type=int, default=3)
ap.add_argument("--S", type=int, default=16)
ap.add_argument("--lo", type=int, default=512)
ap.add_argument("--hi", type=int, default=1024)
ap.add_argument("--seed", type=int, default=7)
ap.add_argument("--chains", type=int, nargs="+", default=[1, 8])
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--sweeps", type=int, default=3)
ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
a = ap.parse_args()
M, S = a.M, a.S
T = M * (M + 1) // 2
rng = np.random.default_rng(a.seed)
nobs = [int(n) for n in rng.integers(a.lo, a.hi + 1, size=S)]
hv = [sim.HYPER_SVC[k] for k in ("mu_tilde_l", "alpha_tilde_l", "beta_tilde_l", "mu_L", "alpha_L", "beta_L", "a", "b")]


def subject(n):
    """n single observations: sorted uniform inputs, interleaved labels, y = sin(6 x + label) + noise"""
    x = np.sort(rng.uniform(0.0, 1.0, n))
    indx = (np.arange(n) % M).astype(np.int32)
    return x, indx, np.sin(6.0 * x + indx) + 0.1 * rng.standard_normal(n)


def chain(x, j):
    """chain j of a subject: smooth curves, rows of I + a lower triangle, tilde_sigma2_err = -2"""
    n = x.shape[0]
    L = np.eye(M) + np.tril(0.3 * np.sin(1.0 + np.arange(M * M).reshape(M, M)))
    Lv = L[np.tril_indices(M)][None, :] * (1.0 + 0.1 * np.sin(3.0 * x + 0.2 * j))[:, None]
    return np.concatenate([-1.5 + 0.2 * np.sin(5.0 * x + 0.3 * j), Lv.reshape(-1), [-2.0 + 0.01 * j]])


subs = [subject(n) for n in nobs]
buckets = hadamard.cohort_buckets(nobs)
one = _lib.Context(0)                                  # (i), and the loop (a) on the same context: the set does not mind
per_bucket = [_lib.Context(0) for _ in buckets]        # (ii)
many = [_lib.Context(0) for _ in range(S)]             # (b)
for c, d in zip(many, subs):
    c.had_set_data(*d)
one.had_set_subjects([d[0] for d in subs], [d[1] for d in subs], [d[2] for d in subs], M=M)
for c, idx in zip(per_bucket, buckets):
    c.had_set_subjects([subs[s][0] for s in idx], [subs[s][1] for s in idx], [subs[s][2] for s in idx], M=M)
need = float(sum(n ** 3 for n in nobs))
ratio_one = S * max(nobs) ** 3 / need
ratio_buckets = sum(len(idx) * max(nobs[s] for s in idx) ** 3 for idx in buckets) / need


def sweep_set(vecs, k, grad):
    out, _, st = one.had_subjects_eval(hadamard.cohort_pack(vecs, nobs, M), hv, True, grad, k)
    return out[:, 0], st


def sweep_buckets(vecs, k, grad):
    val, sts = np.zeros(S * k), np.zeros(S * k, dtype=np.int32)
    for c, idx in zip(per_bucket, buckets):
        out, _, st = c.had_subjects_eval(hadamard.cohort_pack([vecs[s] for s in idx], [nobs[s] for s in idx], M), hv, True, grad, k)
        rows = (np.asarray(idx)[:, None] * k + np.arange(k)[None, :]).reshape(-1)
        val[rows], sts[rows] = out[:, 0], st
    return val, sts


def sweep_a(vecs, k, grad):
    outs, sts = [], []
    for d, v in zip(subs, vecs):
        one.had_set_data(*d)
        out, _, st = one.had_batch_eval(v, hv, True, grad)
        outs.append(out[:, 0]), sts.append(st)
    return np.concatenate(outs), np.concatenate(sts)


def sweep_b(vecs, k, grad):
    outs, sts = [], []
    for c, v in zip(many, vecs):
        out, _, st = c.had_batch_eval(v, hv, True, grad)
        outs.append(out[:, 0]), sts.append(st)
    return np.concatenate(outs), np.concatenate(sts)


ARRANGEMENTS = (("set", sweep_set), ("buckets", sweep_buckets), ("a", sweep_a), ("b", sweep_b))
shapes = [(k, grad, key) for k in a.chains for grad, key in ((False, "value"), (True, "value_grad"))]
vectors = {k: [np.stack([chain(d[0], j) for j in range(k)]) for d in subs] for k in a.chains}
vals = {}
for k, grad, key in shapes:                            # warm-up of every shape: prior factors, workspaces, first launches
    for name, fn in ARRANGEMENTS:
        v, st = fn(vectors[k], k, grad)
        assert np.all(st == 0), (name, k, key, st)
        vals[(k, key, name)] = v
    for name in ("buckets", "a", "b"):                 # the four arrangements compute the same cohort
        assert np.allclose(vals[(k, key, "set")], vals[(k, key, name)], rtol=1e-6, atol=0.0), (name, k, key)
for k, grad, key in shapes:
    times = {name: [] for name, _ in ARRANGEMENTS}
    for rep in range(a.reps):
        for name, fn in ARRANGEMENTS:
            t0 = time.perf_counter()
            for _ in range(a.sweeps):
                fn(vectors[k], k, grad)
            times[name].append((time.perf_counter() - t0) / a.sweeps)
    med = {name: float(np.median(t)) for name, t in times.items()}
    rec = {"M": M, "subjects": S, "nobs": nobs, "seed": a.seed, "chains_per_subject": k, "mode": key, "reps": a.reps,
           "sweeps_per_rep": a.sweeps, "buckets": [[int(s) for s in idx] for idx in buckets],
           "flop_ratio_one_set": round(ratio_one, 4), "flop_ratio_buckets": round(ratio_buckets, 4),
           "ms_per_sweep": {n_: round(1e3 * t, 3) for n_, t in med.items()},
           "ms_per_sweep_all_reps": {n_: [round(1e3 * t, 3) for t in ts] for n_, ts in times.items()},
           "set_vs_a_set_data_loop": round(med["a"] / med["set"], 3), "set_vs_b_context_per_subject": round(med["b"] / med["set"], 3),
           "buckets_vs_set": round(med["set"] / med["buckets"], 3), "build_id": _lib.build_id()}
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
