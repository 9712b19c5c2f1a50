"""Separable and stationary Hadamard models, MAP and posterior-draw prediction for a cohort of RAGGED subjects on one GPU: the set
entries (nmgp_predsample_hads_subjects, nmgp_predict_hadst_subjects: S subjects x H draws at each subject's own new inputs in ONE call)
against what there was before them,
    (i)  one set of all S subjects, padded to the largest,
    (ii) the buckets of hadamard.cohort_buckets at max_flop_waste = 0.5, one context and one set per bucket,
    (c)  one context, a loop of had_set_data + predsample_hads / predict_hadst (H draws) over the subjects (for the separable model the
         cached prior factors go with every had_set_data: two prior factorisations and two projections per subject and visit; the
         stationary model has neither).
    python tools/predsample_had_cohort_models_bench.py [--models sep sta] [--M 3] [--S 16] [--lo 512] [--hi 1024] [--seed 7] [--H 1 16]
                                                       [--grid 201] [--reps 5] [--sweeps 20]
                                                       [--out profiles/predsample_had_cohort_models_bench.jsonl]
The cohort is tools/hadamard_cohort_bench.py's and tools/predsample_had_cohort_bench.py's (same seed, same draws of nobs and
subjects).  Full form: linspace(0, 1, grid) for every subject, all M outputs.  Indexed form: N_s / 4 held-out (x, label) pairs per
subject -- ragged new inputs.  H = 1 runs without noise (MAP), H > 1 with fixed normals (separable; the stationary model has none).
One sweep predicts for all S * H draws once, host packing included.  Every shape is warmed up first (prior factors, workspaces); then
the arrangements alternate within a repetition (i, ii, c, i, ii, c, ...) in one process, a repetition times `sweeps` sweeps; the figures
are medians over the repetitions, with the range.  One JSON line per (model, H, form), plus one line per model with the stage read-out
(nmgp_profile_enable(1)) of one set call at the largest H, full form.

Expectation, written before the first run.  The separable set gains over its loop about what the nonseparable set gained over its own
(profiles/predsample_had_cohort_bench.jsonl: 6.5x full / 5.6x indexed at H = 1, 2.3x / 2.5x at H = 16): the loop pays the same two
prior factorisations and projections per subject and visit, the set shares them, and the factorisations of the draws are the same
size.  The stationary set gains less over its loop: it has no prior factor and no projection to share, so what the set saves is the
loop's per-subject uploads, launches and synchronisations only, against the flop it wastes on padding (S Nmax^3 / sum N_s^3 of the
factorisation); at H = 16, where the factorisation dominates, it may not gain at all.  No ratio is a pass criterion."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nonstationary_multivariate_gaussian_process_amd import _lib, drivers, hadamard, hadamard_sep, hadamard_sta, sim  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--models", nargs="+", default=["sep", "sta"], choices=["sep", "sta"])
ap.add_argument("--M", type=int, default=3)
ap.add_argument("--S", type=int, default=16)
ap.add_argument("--lo", type=int, default=512)
ap.add_argument("--hi", type=int, default=1024)
ap.add_argument("--seed", type=int, default=7)
ap.add_argument("--H", type=int, nargs="+", default=[1, 16])
ap.add_argument("--grid", type=int, default=201)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--sweeps", type=int, default=20)
ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
a = ap.parse_args()
M, S = a.M, a.S
T = M * (M + 1) // 2
rng = np.random.default_rng(a.seed)
nobs = [int(n) for n in rng.integers(a.lo, a.hi + 1, size=S)]
hv = np.array([float(sim.HYPER_SEP[k]) for k in drivers.SEP_HYPER_KEYS])      # (the stationary predictor takes no hyper-parameters)


def subject(n):
    """n single observations: sorted uniform inputs, interleaved labels, y = sin(6 x + label) + noise"""
    x = np.sort(rng.uniform(0.0, 1.0, n))
    indx = (np.arange(n) % M).astype(np.int32)
    return x, indx, np.sin(6.0 * x + indx) + 0.1 * rng.standard_normal(n)


def draw(model, x, j):
    """draw j of a subject: smooth curves, the rows of I + a lower triangle, tilde_sigma2_err = -2"""
    L = np.eye(M) + np.tril(0.3 * np.sin(1.0 + np.arange(M * M).reshape(M, M)))
    Lv = L[np.tril_indices(M)] * (1.0 + 0.02 * j)
    if model == "sta":
        return np.concatenate([[-1.5 + 0.02 * j, 0.1 - 0.01 * j], Lv, [-2.0 + 0.01 * j]])
    return np.concatenate([-1.5 + 0.2 * np.sin(5.0 * x + 0.3 * j), 0.1 * np.cos(4.0 * x + 0.2 * j), Lv, [-2.0 + 0.01 * j]])


subs = [subject(n) for n in nobs]
zrng = np.random.default_rng(a.seed + 1)
forms = {"full": ([np.linspace(0.0, 1.0, a.grid) for _ in subs], None),
         "indexed": ([np.sort(zrng.uniform(0.0, 1.0, n // 4)) for n in nobs], [(np.arange(n // 4) % M).astype(np.int32) for n in nobs])}
buckets = hadamard.cohort_buckets(nobs, 0.5)
one = _lib.Context(0)                                  # (i), and the loop (c) on the same context: the set does not mind
per_bucket = [_lib.Context(0) for _ in buckets]        # (ii)
one.had_set_subjects([d[0] for d in subs], [d[1] for d in subs], [d[2] for d in subs], M=M)
for c, idx in zip(per_bucket, buckets):
    c.had_set_subjects([subs[s][0] for s in idx], [subs[s][1] for s in idx], [subs[s][2] for s in idx], M=M)
need = float(sum(n ** 3 for n in nobs))
ratio_one = S * max(nobs) ** 3 / need
ratio_buckets = sum(len(idx) * max(nobs[s] for s in idx) ** 3 for idx in buckets) / need


def cohort(model, c, draws, xs, lab, z):
    if model == "sep":
        return hadamard_sep.cohort_predict(c, draws, xs, hv, indx_star=lab, z=z)
    return hadamard_sta.cohort_predict(c, draws, xs, indx_star=lab)


def sweep_set(model, draws, xs, lab, z):
    return cohort(model, one, draws, xs, lab, z)


def sweep_buckets(model, draws, xs, lab, z):
    out = [None] * S
    pick = lambda v, idx: None if v is None else [v[s] for s in idx]
    for c, idx in zip(per_bucket, buckets):
        for s, r in zip(idx, cohort(model, c, pick(draws, idx), pick(xs, idx), pick(lab, idx), pick(z, idx))):
            out[int(s)] = r
    return out


def sweep_loop(model, draws, xs, lab, z):
    out = []
    for s, d in enumerate(subs):
        one.had_set_data(*d)
        ix = None if lab is None else lab[s]
        if model == "sep":
            out.append(one.predsample_hads(draws[s], hv, xs[s], indx_star=ix, z=None if z is None else z[s]))
        else:
            out.append(one.predict_hadst(draws[s], xs[s], indx_star=ix))
    return out


ARRANGEMENTS = (("set", sweep_set), ("buckets", sweep_buckets), ("loop", sweep_loop))
shapes = [(model, H, form) for model in a.models for H in a.H for form in ("full", "indexed")]
inputs = {}
for model, H, form in shapes:
    xs, lab = forms[form]
    z = None if H == 1 or model == "sta" else [zrng.standard_normal((H, v.shape[0], 2)) for v in xs]
    inputs[(model, H, form)] = (model, [np.stack([draw(model, d[0], j) for j in range(H)]) for d in subs], xs, lab, z)


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


for key in shapes:                                     # warm-up of every shape: prior factors, workspaces, first launches
    res = {name: fn(*inputs[key]) for name, fn in ARRANGEMENTS}
    for name, rs in res.items():
        assert all(np.all(r[-1] == 0) for r in rs), (name, key)
    for name in ("buckets", "loop"):                   # the arrangements compute the same cohort (the test suite holds the bars)
        for r0, r1 in zip(res["set"], res[name]):
            assert np.allclose(r0[1], r1[1], rtol=1e-4, atol=0.0) and np.allclose(r0[0], r1[0], rtol=1e-4, atol=1e-8), (name, key)
for model, H, form in shapes:
    times = {name: [] for name, _ in ARRANGEMENTS}
    for rep in range(a.reps):
        for name, fn in ARRANGEMENTS:
            t0 = time.perf_counter()
            for _ in range(a.sweeps):
                fn(*inputs[(model, H, form)])
            times[name].append((time.perf_counter() - t0) / a.sweeps)
    med = {name: float(np.median(t)) for name, t in times.items()}
    emit({"model": model, "M": M, "subjects": S, "nobs": nobs, "seed": a.seed, "draws_per_subject": H, "form": form,
          "noise": H > 1 and model == "sep", "new_inputs_per_subject": [int(v.shape[0]) for v in forms[form][0]], "reps": a.reps,
          "sweeps_per_rep": a.sweeps, "buckets": [[int(s) for s in idx] for idx in buckets], "flop_ratio_one_set": round(ratio_one, 4),
          "flop_ratio_buckets": round(ratio_buckets, 4), "ms_per_sweep": {n_: round(1e3 * t, 3) for n_, t in med.items()},
          "ms_per_sweep_range": {n_: [round(1e3 * min(ts), 3), round(1e3 * max(ts), 3)] for n_, ts in times.items()},
          "ms_per_sweep_all_reps": {n_: [round(1e3 * t, 3) for t in ts] for n_, ts in times.items()},
          "set_vs_loop": round(med["loop"] / med["set"], 3), "buckets_vs_loop": round(med["loop"] / med["buckets"], 3),
          "buckets_vs_set": round(med["set"] / med["buckets"], 3), "build_id": _lib.build_id()})

# one stage read-out per model of the set call at the largest H, full form (HIP-event timers: the call itself runs slower under them)
Hp = max(a.H)
for model in a.models:
    one.profile_enable(1)
    one.profile_reset()
    t0 = time.perf_counter()
    sweep_set(*inputs[(model, Hp, "full")])
    wall = time.perf_counter() - t0
    stages = one.profile_read()
    one.profile_enable(0)
    emit({"stage_readout": "set", "model": model, "draws_per_subject": Hp, "form": "full", "wall_ms_under_profiling": round(1e3 * wall, 3),
          "stages_ms_launches": {k: [round(v[0], 3), v[1]] for k, v in stages.items() if v[1]}, "build_id": _lib.build_id()})
