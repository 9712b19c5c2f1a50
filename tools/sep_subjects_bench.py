"""Separable model, a cohort of subjects on one GPU: the subject set (nmgp_sep_batch_set_subjects_chains: S subjects x k chains in ONE
nmgp_sep_batch_eval) against the two ways there were before it,
    (a) one context, a loop of set_data + sep_batch_eval(k chains) over the subjects (the cached prior factors go with every set_data),
    (b) S contexts, each keeping its subject resident, evaluated one after the other.
    python tools/sep_subjects_bench.py [--N 1024] [--M 5] [--S 8] [--chains 1 2 8] [--reps 3] [--sweeps 3] [--out FILE]
One sweep evaluates all S * k chains once.  The arrangements alternate within a repetition (set, a, b, set, a, b, ...) in one session;
a repetition times `sweeps` sweeps after one untimed sweep, the figures are medians over the repetitions.  One JSON line per
(k, value | value_grad): ms per sweep and evaluations / s of each arrangement, and the set's ratios to (a) and (b)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nonstationary_multivariate_gaussian_process_amd import _lib, sim  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--N", type=int, default=1024)
ap.add_argument("--M", type=int, default=5)
ap.add_argument("--S", type=int, default=8)
ap.add_argument("--chains", type=int, nargs="+", default=[1, 2, 8])
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--sweeps", type=int, default=3)
ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
a = ap.parse_args()
N, M, S = a.N, a.M, a.S
hv = [sim.HYPER_SEP[k] for k in ("mu_tilde_l", "alpha_tilde_l", "beta_tilde_l", "mu_tilde_sigma", "alpha_tilde_sigma",
                                  "beta_tilde_sigma", "a", "b", "c")]
subs = [sim.simulate_separable(N, M, 30 + s) for s in range(S)]
xs, Ys = np.stack([d["x"] for d in subs]), np.ascontiguousarray(np.stack([d["Y"] for d in subs]))
one = _lib.Context(0)
many = [_lib.Context(0) for _ in range(S)]
for c, d in zip(many, subs):
    c.set_data(d["x"], d["Y"])


def sweep_set(pars, k, grad):
    # (the set is put in place once per repetition: it persists across evaluations, as the resident subjects of (b) do)
    out, _, st = one.sep_batch_eval(pars, hv, True, grad)
    return out[:, 0], st


def sweep_a(pars, k, grad):
    outs, sts = [], []
    for s, d in enumerate(subs):
        one.set_data(d["x"], d["Y"])
        out, _, st = one.sep_batch_eval(pars[s * k:(s + 1) * k], hv, True, grad)
        outs.append(out[:, 0]), sts.append(st)
    return np.concatenate(outs), np.concatenate(sts)


def sweep_b(pars, k, grad):
    outs, sts = [], []
    for s, c in enumerate(many):
        out, _, st = c.sep_batch_eval(pars[s * k:(s + 1) * k], hv, True, grad)
        outs.append(out[:, 0]), sts.append(st)
    return np.concatenate(outs), np.concatenate(sts)


for k in a.chains:
    pars = np.stack([sim.perturb(d["pars_true"], 0.05, 0.4 + 0.1 * j) for d in subs for j in range(k)])
    for grad, key in ((False, "value"), (True, "value_grad")):
        times = {"set": [], "a": [], "b": []}
        vals = {}
        for rep in range(a.reps):
            for name, fn in (("set", sweep_set), ("a", sweep_a), ("b", sweep_b)):
                if name == "set":
                    one.set_data(subs[0]["x"], subs[0]["Y"])
                    one.sep_batch_set_subjects(xs, Ys, k)
                v, st = fn(pars, k, grad)                        # untimed: prior factors of the set / of (b), allocations
                assert np.all(st == 0), (name, st)
                vals[name] = v
                t0 = time.perf_counter()
                for _ in range(a.sweeps):
                    fn(pars, k, grad)
                times[name].append((time.perf_counter() - t0) / a.sweeps)
                if name == "set":
                    one.sep_batch_clear_subjects()
        for name in ("a", "b"):                                  # the three arrangements compute the same cohort
            assert np.allclose(vals["set"], vals[name], rtol=1e-9, atol=0.0), (name, vals["set"], vals[name])
        med = {name: float(np.median(t)) for name, t in times.items()}
        rec = {"N": N, "M": M, "subjects": S, "chains_per_subject": k, "mode": key, "reps": a.reps, "sweeps_per_rep": a.sweeps,
               "ms_per_sweep": {n_: round(1e3 * t, 3) for n_, t in med.items()},
               "ms_per_sweep_all_reps": {n_: [round(1e3 * t, 3) for t in ts] for n_, ts in times.items()},
               "evals_per_s": {n_: round(S * k / t, 1) for n_, t in med.items()},
               "set_vs_a_set_data_loop": round(med["a"] / med["set"], 3), "set_vs_b_context_per_subject": round(med["b"] / med["set"], 3)}
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
