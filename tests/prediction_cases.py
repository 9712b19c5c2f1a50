"""Synthetic subjects for the sweep of the complete-data prediction entries (tests/test_prediction_sweep_cpu.py,
tests/test_gpu_prediction_sweep.py): every M from 1 to 8, the 128-column chunks and 64-lane row groups of the row reductions, the
256-wide blocks of the cross-covariance rows, the stride-256 loops of the regression, the three slice lines, and an unsorted,
unevenly spaced subject.  A plain module, not a conftest: both halves import it, so the CPU half checks the very subjects the GPU
half runs.  No random generator sits in the kernels' path: sim.rngfree_inputs / rngfree_pars_* and numpy.random.default_rng(seed) for
the normals."""
import functools

import numpy as np

from conftest import SEP_KEYS, SVC_KEYS
from nonstationary_multivariate_gaussian_process_amd import sim

H = 3                                                                    # parameter vectors per subject
# sigma2_err of every subject's base vectors.  At sim's 1e-2 the two CPU references disagree by 1.2e-10 on the stationary mean at
# N40_M8 (cond 6.8e5), which puts TIGHT at 1.2e-8, above the 1e-8 it has to stay under: raised until it does, the bar is not loosened.
SIGMA2_ERR = 4e-2

# (N, M, layout).  n = M N: 126 / 128 / 129 / 127 around the 128-column chunks; (257, 2): the stride-256 loops over N; (127, 6): the
# largest matrix, of order 762
SUBJECTS = [(1, 1, "even"), (2, 2, "even"), (8, 8, "even"), (9, 7, "even"), (63, 2, "even"), (64, 2, "even"), (43, 3, "even"),
            (127, 1, "even"), (65, 5, "even"), (127, 6, "even"), (129, 4, "even"), (40, 8, "even"), (257, 2, "even"),
            (21, 3, "unsorted")]
LINE = (9, 7, "even")                                                    # the subject of the slice lines
ROWS_256 = (129, 4, "even")                                              # E = 256 / 260 riding rows in one slice
ROWS_64 = (127, 1, "even")                                               # E = 63 / 64 / 65 riding rows in one slice
EIG = [(127, 1, "even"), (64, 2, "even"), (40, 8, "even")]               # the subjects of the eigen formulation
MIRROR = [(63, 2, "even"), (65, 5, "even")]                              # the subjects of the Python mirror
MINOR = (65, 3, "even")                                                  # the subject of the leading-minor status
S_SHORT = 7

HYPER_SEP_DIFF = dict(sim.HYPER_SEP, alpha_tilde_sigma=1.0)              # the separable analogue of sim.HYPER_SVC_MPISIM
HYPERS = {"svc": {"same": np.array([sim.HYPER_SVC[k] for k in SVC_KEYS]), "diff": np.array([sim.HYPER_SVC_MPISIM[k] for k in SVC_KEYS])},
          "sep": {"same": np.array([sim.HYPER_SEP[k] for k in SEP_KEYS]), "diff": np.array([HYPER_SEP_DIFF[k] for k in SEP_KEYS])}}
HYPER_SETS = ("same", "diff")


def case_id(case):
    return "N%d_M%d_%s" % case


def case_seed(case):
    return 10 * case[0] + case[1]


def slice_line(entry, N, M):
    """Grid points per factorisation of the entry: the slice line."""
    return {"predict_svc": max(1, (M * N - 2) // M), "predsample_svc": N, "kron": max(1, N - 2)}[entry]


def edge_grids():
    """(subject, entry, S): every entry's slice line at S = smax, smax + 1, 2 smax + 1, and the riding-row edges in one slice.  'kron'
    stands for the four separable / stationary entries, which share one line."""
    g = []
    for entry in ("predict_svc", "predsample_svc", "kron"):
        k = slice_line(entry, LINE[0], LINE[1])
        g += [(LINE, entry, S) for S in (k, k + 1, 2 * k + 1)]
    g += [(ROWS_256, entry, S) for entry in ("predict_svc", "predsample_svc") for S in (64, 65)]
    g += [(ROWS_64, entry, S) for entry in ("predict_svc", "predsample_svc", "kron") for S in (63, 64, 65)]
    return g


EDGE_GRIDS = edge_grids()
EDGE_MODELS = {"predict_svc": ("svc",), "predsample_svc": ("svc",), "kron": ("sep", "sta")}


# ---- subjects ---------------------------------------------------------------------------------------------------------------------
def unsorted_inputs(N, M, seed):
    """Unevenly spaced inputs in (0.05, 0.95) in a random order, the outputs of sim.rngfree_inputs at them."""
    rng = np.random.default_rng(seed)
    x = 0.05 + 0.9 * np.sort(rng.uniform(0.0, 1.0, N)) ** 1.5
    x = x[rng.permutation(N)]
    Y = np.stack([np.sin(2.0 * np.pi * x * (m + 1)) + 0.1 * m for m in range(M)], 1)
    return x, np.ascontiguousarray(Y)


def base_pars(x, M):
    """sim.rngfree_pars_svc / _sep / _sta as functions of the inputs (equal to them at sim.rngfree_inputs: asserted in the CPU half)"""
    T = M * (M + 1) // 2
    tl = 3.0 * (x - 1.0) ** 3 - 3.0
    uLs = np.stack([0.1 * (t + 1) * np.cos(np.pi * x) - 0.2 for t in range(T)], 1)
    uL = 0.1 * (np.arange(T) + 1.0) - 0.2
    return {"svc": np.concatenate([tl, uLs.reshape(-1), [np.log(1e-2)]]),
            "sep": np.concatenate([tl, 0.3 * np.sin(3.0 * x), uL, [np.log(1e-2)]]),
            "sta": np.concatenate([[-2.0, 0.0], uL, [np.log(1e-2)]])}


def draws(p0, x, M):
    """H smooth perturbations of the three base vectors, as smooth_draws in test_gpu_predsample.py and the fixtures' generators"""
    N, T = x.shape[0], M * (M + 1) // 2
    out = {"svc": [], "sep": [], "sta": []}
    for k in range(H):
        p = p0["svc"].copy()
        p[:N] += 0.05 * np.sin(3.0 * x + 0.4 + k)
        p[N:N + N * T] += (0.05 * np.sin(3.0 * x[:, None] + 0.4 + k + np.arange(T)[None, :])).reshape(-1)
        p[-1] += 0.01 * k
        out["svc"].append(p)
        p = p0["sep"].copy()
        p[:N] += 0.05 * np.sin(3.0 * x + 0.4 + k)
        p[N:2 * N] += 0.05 * np.sin(3.0 * x + 1.4 + k)
        p[2 * N:2 * N + T] += 0.02 * np.cos(np.arange(T) + k)
        p[-1] += 0.01 * k
        out["sep"].append(p)
        p = p0["sta"].copy()
        p[0] += 0.05 * np.sin(0.4 + k)
        p[1] += 0.05 * np.sin(1.4 + k)
        p[2:2 + T] += 0.02 * np.cos(np.arange(T) + k)
        p[-1] += 0.01 * k
        out["sta"].append(p)
    return {m: np.stack(v) for m, v in out.items()}


@functools.lru_cache(maxsize=None)
def build(case):
    """The subject and the H draws of the three models, built once.  The arrays are shared: do not write into them."""
    N, M, layout = case
    if layout == "even":
        x, Y = sim.rngfree_inputs(N, M)
        p0 = {"svc": sim.rngfree_pars_svc(N, M), "sep": sim.rngfree_pars_sep(N, M), "sta": sim.rngfree_pars_sta(M)}
    else:
        x, Y = unsorted_inputs(N, M, case_seed(case))
        p0 = base_pars(x, M)
    for m in p0:
        assert p0[m][-1] == np.log(1e-2)
        p0[m][-1] = np.log(SIGMA2_ERR)
    return dict(N=N, M=M, T=M * (M + 1) // 2, x=x, Y=Y, base=p0, pars=draws(p0, x, M))


# ---- grids, normals, starred values ---------------------------------------------------------------------------------------------------
def grid(x, S):
    """S >= 3 new inputs from 0.1 below the smallest to 0.1 above the largest training input, slot 1 a training input itself"""
    xs = np.linspace(x.min() - 0.1, x.max() + 0.1, S)
    xs[1] = x[len(x) // 2]
    return xs


def normals(case, S, width):
    """The fixed standard normals z [H, S, width] of the latent regressions (width 1 + T: nonseparable, 2: separable)"""
    return np.random.default_rng(case_seed(case) + 1).standard_normal((H, S, width))


def star_svc(xs, M):
    """Caller's starred values [H, S, 1 + T] that are NOT the regressed ones: a smooth tilde_l*, smooth off-diagonal slots of L* and
    diagonal slots in [0.8, 1.2] (the slots enter L* as they are)"""
    T, S = M * (M + 1) // 2, xs.shape[0]
    dg = np.cumsum(np.arange(1, M + 1)) - 1
    st = np.empty((H, S, 1 + T))
    for h in range(H):
        st[h, :, 0] = -2.5 + 0.3 * np.sin(4.0 * xs + h)
        st[h, :, 1:] = 0.3 * np.cos(3.0 * xs[:, None] + np.arange(T)[None, :] + h)
        st[h][:, 1 + dg] = 1.0 + 0.2 * np.sin(2.0 * xs[:, None] + np.arange(M)[None, :] + h)
    return st


def star_sep(xs):
    """Caller's (tilde_l*, tilde_sigma*) [H, S, 2]"""
    return np.stack([np.stack([-2.5 + 0.3 * np.sin(4.0 * xs + h), 0.2 * np.cos(3.0 * xs + h)], axis=1) for h in range(H)])


def sd(a):
    """[S, H, ...] (the restatements' point-major order) <-> [H, S, ...] (the entries' draw-major order)"""
    return np.ascontiguousarray(np.swapaxes(a, 0, 1))


# ---- the references (imported late: they live in test modules) ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle(case, hy, S=S_SHORT):
    """The dense oracle (one Cholesky of the full M N x M N covariance) on draw 0 at grid(x, S):
    {'svc': (mean, var, Lstar), 'sep': (mean, var), 'sta': (mean, var)}"""
    from oracle import nmgp_oracle as O
    c = build(case)
    N, M, x, Y = c["N"], c["M"], c["x"], c["Y"]
    xs = grid(x, S)
    p = c["pars"]["svc"][0]
    _, Ls, mean, var = O.predmap_inhomogeneous(*O.vec2pars_SVC(p, N, M), Y, x, xs, *HYPERS["svc"][hy][:6])
    out = {"xs": xs, "svc": (mean, var, Ls)}
    _, mean, var = O.predmap_separable(*O.vec2pars(c["pars"]["sep"][0], N, M), Y, x, xs, *HYPERS["sep"][hy][:6])
    out["sep"] = (mean, var)
    out["sta"] = O.predmap_stationary(*O.vec2pars_S(c["pars"]["sta"][0], M), Y, x, xs)
    return out


@functools.lru_cache(maxsize=None)
def drawn(case, hy, S=S_SHORT):
    """The restatements of the posterior-draw entries with the regression, under normals(case, S, .), draw-major:
    {('svc', constrained): (mean, var, star), ('sep', kss_jitter): (mean, var, star), 'sta': (mean, var)}"""
    from test_predsample_cpu import restate
    from test_predsample_sep_cpu import restate_sep, restate_sta
    c = build(case)
    x, Y, T = c["x"], c["Y"], c["T"]
    xs = grid(x, S)
    out = {"xs": xs, "z_svc": normals(case, S, 1 + T), "z_sep": normals(case, S, 2)}
    for flag in (True, False):
        out[("svc", flag)] = tuple(sd(a) for a in restate(x, Y, c["pars"]["svc"], HYPERS["svc"][hy], xs, sd(out["z_svc"]), flag))
        out[("sep", flag)] = tuple(sd(a) for a in restate_sep(x, Y, c["pars"]["sep"], HYPERS["sep"][hy], xs, sd(out["z_sep"]), flag))
    out["sta"] = restate_sta(x, Y, c["pars"]["sta"], xs)
    return out


@functools.lru_cache(maxsize=None)
def starred(case, S=S_SHORT):
    """The restatements on the caller's starred values (no regression: the hyper-parameters play no part), draw-major:
    {'svc': (mean, var), ('sep', kss_jitter): (mean, var), 'sta': (mean, var)} and the starred values themselves"""
    from test_predsample_cpu import restate
    from test_predsample_sep_cpu import restate_sep, restate_sta
    c = build(case)
    x, Y, M = c["x"], c["Y"], c["M"]
    xs = grid(x, S)
    out = {"xs": xs, "star_svc": star_svc(xs, M), "star_sep": star_sep(xs)}
    out["svc"] = tuple(sd(a) for a in restate(x, Y, c["pars"]["svc"], HYPERS["svc"]["same"], xs, star=sd(out["star_svc"]))[:2])
    for flag in (True, False):
        out[("sep", flag)] = tuple(sd(a) for a in restate_sep(x, Y, c["pars"]["sep"], HYPERS["sep"]["same"], xs, kss_jitter=flag,
                                                              star=sd(out["star_sep"]))[:2])
    out["sta"] = restate_sta(x, Y, c["pars"]["sta"], xs)
    return out


@functools.lru_cache(maxsize=None)
def dense_starred(case, S=S_SHORT):
    """The third reference: plain dense conditioning on the caller's starred values (test_prediction_sweep_cpu.py), and the dense
    oracle of the stationary model, per draw; the variances are the raw ones, before any clip.  Keys as `starred`."""
    from oracle import nmgp_oracle as O
    from test_prediction_sweep_cpu import dense_star_sep, dense_star_svc
    c = build(case)
    x, Y, M, P = c["x"], c["Y"], c["M"], c["pars"]
    st = starred(case, S)
    xs = st["xs"]
    out = {"svc": tuple(np.stack(a) for a in zip(*[dense_star_svc(x, Y, P["svc"][h], xs, st["star_svc"][h]) for h in range(H)]))}
    for flag in (True, False):
        out[("sep", flag)] = tuple(np.stack(a) for a in zip(*[dense_star_sep(x, Y, P["sep"][h], xs, st["star_sep"][h], flag) for h in range(H)]))
    out["sta"] = tuple(np.stack(a) for a in zip(*[O.predmap_stationary(*O.vec2pars_S(P["sta"][h], M), Y, x, xs) for h in range(H)]))
    return out


# ---- the measures and the tight bar --------------------------------------------------------------------------------------------------
def mean_err(a, b):
    return float(np.max(np.abs(a - b) / (np.abs(b) + 1e-2)))


def var_err(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b)))


def allclose_err(a, b, rtol, atol):
    """The measure numpy's allclose bounds by rtol: max |a - b| / (atol / rtol + |b|)."""
    return float(np.max(np.abs(a - b) / (atol / rtol + np.abs(b))))


def disagreement(case):
    """{quantity: error} between the block-wise restatements and the dense references on the regression-free quantities of one subject"""
    blk, dns = starred(case), dense_starred(case)
    keys = ["svc", ("sep", True), ("sep", False), "sta"]
    return {"mean": max(mean_err(blk[k][0], dns[k][0]) for k in keys), "var": max(var_err(blk[k][1], dns[k][1]) for k in keys)}


@functools.lru_cache(maxsize=None)
def tight():
    """(the largest disagreement between the two CPU references over all subjects, TIGHT = 100 x it).  Both references use LAPACK;
    the device factors in 64-wide blocks with FMA and another summation order; all are backward stable at the same cond(Sigma), so
    their errors are of one order with a constant of tens."""
    worst = max(max(disagreement(case).values()) for case in SUBJECTS)
    return worst, 100.0 * worst
