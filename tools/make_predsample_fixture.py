"""Fixture of tests/test_gpu_predsample_parent_bits.py: the bits of the six posterior-draw prediction entries on the smallest shapes
that reach every branch of their host schedule (ps_predict, csrc/nmgp_predsample_common.h).

    python tools/make_predsample_fixture.py [out.npz, default tests/golden/predsample_parent_bits.npz]

runs every case on cuda:0 with the library of the tree it is started from and writes `mean`, `var`, `star` (float64, where the entry
has starred values) and `status` (int32) of each.  Every case has H = 3 draws under NMGP_PREDSAMPLE_CHUNK=2 (chunks of 2 and 1)
and S just above the entry's slice width (two slices, the second short).  The committed fixture was written by the library of the
commit BEFORE the six drivers became one; the test requires the same bytes of every later library.  `--print` runs the cases and
prints them as one JSON line instead (the test's child process under NMGP_POISON=1)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(ROOT, "tests", "golden", "predsample_parent_bits.npz")
HAD_SUBJECT = os.path.join(ROOT, "tests", "golden", "had_N77_M3.npz")      # tests/predsample_had_cases.py's first fixture subject
H = 3
SVC_KEYS = ["mu_tilde_l", "alpha_tilde_l", "beta_tilde_l", "mu_L", "alpha_L", "beta_L", "a", "b"]
SEP_KEYS = ["mu_tilde_l", "alpha_tilde_l", "beta_tilde_l", "mu_tilde_sigma", "alpha_tilde_sigma", "beta_tilde_sigma", "a", "b", "c"]
# separable Hadamard model on the N = 77 subject: two distinct prior pairs (the sim.HYPER_SEP pairs coincide)
HADS_DISTINCT = [-2.4, 1.0, 0.05, 0.0, 1.5, 0.03, 1.0, 1.0, 10.0]

# (name, entry, variant): variant is what the case covers beyond H = 3 draws in chunks of 2 + 1 and two slices
#   z: normals given; star: star_in instead of the regression; nan: the middle draw has a NaN parameter; ix: indexed form;
#   same / distinct: the two prior pairs coincide or not (svc, hads; had's hyper is distinct, sep's coincides)
CASES = (
    ("svc_same_z", "svc", dict(z=True)),                       # N = 40, M = 3, S = 45: 40 + 5
    ("svc_distinct_z_unconstrained", "svc", dict(z=True, distinct=True, flag=False)),
    ("svc_star", "svc", dict(star=True)),
    ("svc_nan", "svc", dict(z=True, nan=True)),
    ("sep_z_jitter", "sep", dict(z=True)),                     # N = 33, M = 3, S = 35: 31 + 4
    ("sep_z_nojitter", "sep", dict(z=True, flag=False)),
    ("sep_star", "sep", dict(star=True)),
    ("sep_nan", "sep", dict(z=True, nan=True)),
    ("sta", "sta", dict()),                                    # N = 33, M = 2, S = 35: 31 + 4
    ("sta_nan", "sta", dict(nan=True)),
    ("had_full_z", "had", dict(z=True)),                       # had_N77_M3, S = 30: 25 + 5
    ("had_ix_z", "had", dict(z=True, ix=True)),                # ... S = 80: 77 + 3
    ("had_full_star", "had", dict(star=True)),
    ("had_full_nan", "had", dict(z=True, nan=True)),
    ("hads_full_distinct_z", "hads", dict(z=True, distinct=True)),
    ("hads_ix_same_z", "hads", dict(z=True, ix=True)),
    ("hads_full_star", "hads", dict(star=True)),
    ("hads_full_nan", "hads", dict(z=True, nan=True)),
    ("hadst_full", "hadst", dict()),
    ("hadst_ix", "hadst", dict(ix=True)),
    ("hadst_full_nan", "hadst", dict(nan=True)),
)
NAMES = tuple(c[0] for c in CASES)


def draws(pars, nan):
    """H smooth perturbations of one parameter vector; nan: entry 0 (a log length-scale in every model) of the middle draw."""
    from nonstationary_multivariate_gaussian_process_amd import sim
    d = np.stack([sim.perturb(pars, 0.05, 0.2 + 0.11 * k) for k in range(H)])
    if nan:
        d[1, 0] = np.nan
    return d


def had_subject():
    with np.load(HAD_SUBJECT) as g:
        return {k: g[k] for k in ("x", "indx", "y", "pars", "hyper")}


def had_pars(entry, g):
    """One parameter vector of `entry`'s model on the Hadamard subject: the fixture's own for the nonseparable model; smooth curves
    and the cross-output factor of sim.simulate_separable for the other two."""
    from nonstationary_multivariate_gaussian_process_amd import sim
    if entry == "had":
        return g["pars"]
    x, M = g["x"], 3
    expo = np.abs(np.arange(M)[:, None] - np.arange(M)[None, :])
    L = np.linalg.cholesky((0.5 ** expo) * np.outer(1.0 + 0.25 * np.arange(M), 1.0 + 0.25 * np.arange(M)))
    uL = L[np.tril_indices(M)].copy()
    if entry == "hadst":                                   # [tilde_l, tilde_sigma, L_vec as it is, tilde_sigma2_err]
        return np.concatenate([[-1.0, 0.0], uL, [np.log(1e-2)]])
    d = sim.tril_diag_slots(M)
    uL[d] = np.log(uL[d])
    return np.concatenate([-2.4 + 0.2 * np.sin(3.0 * x), 0.3 * np.sin(3.0 * x), uL, [np.log(1e-2)]])


def run_case(ctx, i, entry, v):
    """dict(mean, var, status[, star]) of case number i."""
    from nonstationary_multivariate_gaussian_process_amd import sim
    rng = np.random.default_rng(4100 + i)
    nan, flag = v.get("nan", False), v.get("flag", True)
    if entry in ("svc", "sep", "sta"):
        N, M, S = {"svc": (40, 3, 45), "sep": (33, 3, 35), "sta": (33, 2, 35)}[entry]
        gen = {"svc": sim.simulate_nonseparable, "sep": sim.simulate_separable, "sta": sim.simulate_stationary}[entry]
        d = gen(N, M, seed=4000 + ("svc", "sep", "sta").index(entry))
        ctx.set_data(d["x"], d["Y"])
        pars = draws(d["pars_true"], nan)
        width = {"svc": 1 + M * (M + 1) // 2, "sep": 2, "sta": 0}[entry]
        hyper = [(sim.HYPER_SVC_DIST if v.get("distinct") else sim.HYPER_SVC)[k] for k in SVC_KEYS] if entry == "svc" else \
            [sim.HYPER_SEP[k] for k in SEP_KEYS]
    else:
        g = had_subject()
        ctx.had_set_data(g["x"], g["indx"], g["y"], M=3)
        pars = draws(had_pars(entry, g), nan)
        S = 80 if v.get("ix") else 30
        width = {"had": 7, "hads": 2, "hadst": 0}[entry]
        hyper = g["hyper"] if entry == "had" else HADS_DISTINCT if v.get("distinct") else [sim.HYPER_SEP[k] for k in SEP_KEYS]
    xs = np.linspace(-0.02, 1.02, S)
    lab = (5 * np.arange(S)) % 3 if v.get("ix") else None
    z = rng.standard_normal((H, S, width)) if v.get("z") else None
    star = -2.0 + 0.3 * rng.standard_normal((H, S, width)) if v.get("star") else None
    if entry == "svc":
        mean, var, st, status = ctx.predsample_svc(pars, hyper, xs, z=z, star=star, constrained=flag)
    elif entry == "sep":
        mean, var, st, status = ctx.predsample_sep(pars, hyper, xs, z=z, star=star, kss_jitter=flag)
    elif entry == "sta":
        (mean, var, status), st = ctx.predsample_sta(pars, xs), None
    elif entry == "had":
        mean, var, st, status = ctx.predsample_had(pars, hyper, xs, indx_star=lab, z=z, star=star)
    elif entry == "hads":
        mean, var, st, status = ctx.predsample_hads(pars, hyper, xs, indx_star=lab, z=z, star=star)
    else:
        (mean, var, status), st = ctx.predict_hadst(pars, xs, indx_star=lab), None
    ok = np.array([0, 2]) if nan else np.arange(H)         # the draws that must succeed
    assert np.all(status[ok] == 0) and np.all(np.isfinite(mean[ok])) and np.all(np.isfinite(var[ok])), (entry, v, status)
    assert not nan or (status[1] != 0 and np.all(np.isnan(mean[1])) and np.all(np.isnan(var[1]))), (entry, v, status)
    out = dict(mean=mean, var=var, status=status.astype(np.int32))
    if st is not None:
        out["star"] = st
    return {k: np.ascontiguousarray(a) for k, a in out.items()}


def evaluate_all():
    """{"<case>/<mean | var | star | status>": array} of every case, in one context, under NMGP_PREDSAMPLE_CHUNK=2."""
    from nonstationary_multivariate_gaussian_process_amd import _lib
    old = os.environ.get("NMGP_PREDSAMPLE_CHUNK")
    os.environ["NMGP_PREDSAMPLE_CHUNK"] = "2"
    ctx = _lib.Context(0)
    try:
        res = {}
        for i, (name, entry, v) in enumerate(CASES):
            for k, a in run_case(ctx, i, entry, v).items():
                res[name + "/" + k] = a
    finally:
        ctx.close()
        if old is None:
            del os.environ["NMGP_PREDSAMPLE_CHUNK"]
        else:
            os.environ["NMGP_PREDSAMPLE_CHUNK"] = old
    return res


def main():
    res = evaluate_all()
    if "--print" in sys.argv:
        print(json.dumps({k: [str(a.dtype), list(a.shape), a.tobytes().hex()] for k, a in res.items()}))
        return
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = args[0] if args else FIXTURE
    np.savez_compressed(path, **res)
    for k in sorted(res):
        print(k, res[k].shape, res[k].dtype, res[k].reshape(-1)[:2])
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
