"""Synthetic subjects for the Hadamard sweep (tests/test_hadamard_sweep_cpu.py, tests/test_gpu_hadamard_sweep.py): every M from 1 to 8,
the edges of the 64 x 64 tiles, four label layouts next to the fixtures' interleaved one, and one slice wider than 256 riding rows.
A plain module, not a conftest: both halves import it, so the CPU half checks the very subjects the GPU half runs."""
import functools

import numpy as np

from conftest import golden

LAYOUTS = ("interleaved", "blocks", "rare_last", "rare_first", "unsorted")

# (N, M, layout): N = M (each label once, full-form slices of one input); 63 / 64 / 65 / 128 / 129 / 193 around the 64-wide tiles
CASES = [(1, 1, "interleaved"), (2, 2, "interleaved"), (8, 8, "interleaved"), (5, 5, "unsorted"), (63, 2, "blocks"),
         (64, 5, "rare_last"), (65, 6, "rare_first"), (128, 2, "interleaved"), (129, 7, "unsorted"), (193, 8, "blocks")]
WIDE = (321, 3, "interleaved")              # (N / M) M = 321 > 256 riding rows in one slice
MINOR = (65, 3, "interleaved")              # the subject of the leading-minor status


def case_id(case):
    return "N%d_M%d_%s" % case


def case_seed(case):
    return 10 * case[0] + case[1]


def subject(N, M, layout, seed):
    """(x, indx int32, y, L_vec): sorted uniform inputs with one repeated time stamp (N >= 4), labels in the given layout (every label
    in [0, M) occurs), y = sin(6 x + label) + noise, and the packed lower triangle of I + tril(0.3 normal): asymmetric in the outputs,
    so that a row / column or label mix-up cannot cancel."""
    assert layout in LAYOUTS and N >= M >= 1
    rng = np.random.default_rng(seed)
    x = np.sort(rng.uniform(0.0, 1.0, N))
    if N >= 4:
        x[N // 2] = x[N // 2 - 1]
    i = np.arange(N)
    if layout in ("interleaved", "unsorted"):
        indx = i % M
    elif layout == "blocks":
        indx = np.sort(i % M)
    elif layout == "rare_last":                       # label M - 1 at the last observation only
        indx = i % max(M - 1, 1)
        indx[-1] = M - 1
    else:                                             # rare_first: label 0 at observation 0 only
        indx = (1 + i % (M - 1)) if M > 1 else np.zeros(N, dtype=np.int64)
        indx[0] = 0
    if layout == "unsorted":
        x = x[rng.permutation(N)]
    indx = indx.astype(np.int32)
    L = np.eye(M) + np.tril(0.3 * rng.standard_normal((M, M)))
    L_vec = L[np.tril_indices(M)]
    y = np.sin(6.0 * x + indx) + 0.1 * rng.standard_normal(N)
    return x, indx, y, L_vec


def parameters(x, M, L_vec):
    """{'sta' [2, T+3], 'sep' [2, 2N+T+1], 'had' [2, N(1+T)+1]}: chain 0 as the issue states it, chain 1 a smooth perturbation of it
    (amplitude 0.05 on the curves and on the L slots, 0.01 on the last slot)."""
    N, T = x.shape[0], M * (M + 1) // 2
    tl, ts = -1.5 + 0.2 * np.sin(5.0 * x), 0.1 * np.cos(4.0 * x)
    Lvs = L_vec[None, :] * (1.0 + 0.1 * np.sin(3.0 * x))[:, None]
    dl, ds = 0.05 * np.sin(3.0 * x + 1.4), 0.05 * np.cos(2.0 * x + 0.3)
    dL = 0.05 * np.sin(1.7 + np.arange(T))
    dLs = 0.05 * np.sin(3.0 * x[:, None] + 1.4 + np.arange(T)[None, :])
    sta0 = np.concatenate([[-1.5, 0.1], L_vec, [-2.0]])
    sta1 = sta0 + np.concatenate([[0.05 * np.sin(1.4), 0.05 * np.cos(0.3)], dL, [0.01]])
    sep0 = np.concatenate([tl, ts, L_vec, [-2.0]])
    sep1 = sep0 + np.concatenate([dl, ds, dL, [0.01]])
    had0 = np.concatenate([tl, Lvs.reshape(-1), [-2.0]])
    had1 = had0 + np.concatenate([dl, dLs.reshape(-1), [0.01]])
    return {"sta": np.stack([sta0, sta1]), "sep": np.stack([sep0, sep1]), "had": np.stack([had0, had1])}


def hypers():
    return {"sta": golden("hsta_N77_M3")["hyper"], "sep": golden("hsep_N77_M3")["hyper"], "had": golden("had_N77_M3")["hyper"]}


def grid(N, M, x, S=None):
    """New inputs: linspace(-0.1, 1.1, S) with a training input in slot 1.  S = 2 (N // M) + 1 below N = 64 (three full-form slices,
    the last ragged; three slices of one input when N = M), 11 otherwise."""
    if S is None:
        S = 2 * (N // M) + 1 if N < 64 else 11
    xs = np.linspace(-0.1, 1.1, S)
    xs[1] = x[0]
    return xs


def grid_labels(S, M, step=3):
    return ((step * np.arange(S)) % M).astype(np.int32)


@functools.lru_cache(maxsize=None)
def build(case):
    """Everything both halves need of one case, built once: the subject, the B = 2 chains of the three models, the hyper-parameters,
    the new inputs and their labels for the indexed forms.  The arrays are shared: do not write into them."""
    N, M, layout = case
    x, indx, y, L_vec = subject(N, M, layout, case_seed(case))
    xs = grid(N, M, x)
    return dict(N=N, M=M, T=M * (M + 1) // 2, x=x, indx=indx, y=y, L_vec=L_vec, pars=parameters(x, M, L_vec), hyper=hypers(), xs=xs,
                lab=grid_labels(xs.shape[0], M))


# ---- the references: the NumPy restatements the fixtures pin (imported late: they live in test modules) --------------------------------
MODELS = ("sta", "sep", "had")


def ref_logpos(model, pars, c, prior, grad=False):
    """(verbose tuple[, d NegLog / d pars]) of the model's restatement on the subject c = build(case)."""
    from test_hadamard_cpu import had_logpos
    from test_hadamard_sep_cpu import hsep_logpos
    from test_hadamard_sta_cpu import hsta_logpos
    fn = {"sta": hsta_logpos, "sep": hsep_logpos, "had": had_logpos}[model]
    return fn(pars, c["x"], c["indx"], c["y"], c["hyper"][model], prior=prior, grad=grad)


def ref_covariance(model, pars, c):
    from test_hadamard_cpu import had_covariance
    from test_hadamard_sep_cpu import hsep_covariance
    from test_hadamard_sta_cpu import hsta_covariance
    N, M, T = c["N"], c["M"], c["T"]
    if model == "sta":
        return hsta_covariance(pars, c["x"], c["indx"], M)
    if model == "sep":
        return hsep_covariance(pars, c["x"], c["indx"], M)
    return had_covariance(pars[:N], pars[N:N + N * T], pars[-1], c["x"], c["indx"], M)


def normals(case, S):
    """The fixed standard normals z [2, S, 2] of the two posterior draws' latent regressions."""
    return np.random.default_rng(case_seed(case) + 1).standard_normal((2, S, 2))


@functools.lru_cache(maxsize=None)
def predictions(case, S=None, step=3, indexed_only=False):
    """The restatements' moments at grid(N, M, x, S), labels (step s) % M in the indexed forms; every variance is the one BEFORE the clip
    (restate_hps returns the clipped scale: its square exceeds sigma2_err exactly when the raw variance does).
      sta_full / sta_ix: per chain (mean, raw);  sep / had: chain 0's (mean [S, M], raw [S, M])
      hps_full / hps_ix: (loc, scale) [S, 2, 2 + K] of the two chains as posterior draws under normals(case, S)"""
    from test_hadamard_cpu import had_predict
    from test_hadamard_sep_cpu import hsep_predict
    from test_hadamard_sta_cpu import hsta_moments
    from test_predsample_hadamard_cpu import restate_hps
    c = build(case)
    N, M, x, indx, y, P, hy = c["N"], c["M"], c["x"], c["indx"], c["y"], c["pars"], c["hyper"]
    xs = grid(N, M, x, S)
    S = xs.shape[0]
    lab = grid_labels(S, M, step)
    z = np.swapaxes(normals(case, S), 0, 1)                                     # the restatement's order [S, H, 2]
    out = dict(xs=xs, lab=lab, z=normals(case, S))
    out["sta_ix"] = [hsta_moments(P["sta"][k], x, indx, y, xs, lab) for k in (0, 1)]
    out["hps_ix"] = restate_hps(x, indx, y, P["sep"], hy["sep"], xs, np.concatenate([z, np.zeros((S, 2, 1))], axis=2), lab)[:2]
    if not indexed_only:
        out["sta_full"] = [hsta_moments(P["sta"][k], x, indx, y, xs) for k in (0, 1)]
        pct, raw = hsep_predict(P["sep"][0], x, indx, y, hy["sep"], xs)
        out["sep"] = (pct[:, 1], raw)
        pct, raw = had_predict(P["had"][0], x, indx, y, hy["had"], xs)
        out["had"] = (pct[:, 1], raw)
        out["hps_full"] = restate_hps(x, indx, y, P["sep"], hy["sep"], xs, np.concatenate([z, np.zeros((S, 2, M))], axis=2))[:2]
    return out


def raw_variance_floor(pred, c):
    """min over every comparison of (variance / sigma2_err of its chain): > 1 means the clip to 1e-6 plays no part anywhere."""
    s2 = {m: np.exp(c["pars"][m][:, -1]) for m in MODELS}
    r = [np.min(pred["sta_ix"][k][1]) / s2["sta"][k] for k in (0, 1)]
    r += [np.min(pred["hps_ix"][1][:, k, 2:] ** 2) / s2["sep"][k] for k in (0, 1)]
    if "sta_full" in pred:
        r += [np.min(pred["sta_full"][k][1]) / s2["sta"][k] for k in (0, 1)]
        r += [np.min(pred["sep"][1]) / s2["sep"][0], np.min(pred["had"][1]) / s2["had"][0]]
        r += [np.min(pred["hps_full"][1][:, k, 2:] ** 2) / s2["sep"][k] for k in (0, 1)]
    return float(min(r))


# section (c): one slice of 107 inputs = 321 riding rows, then 3;  indexed: 321 rows, then 9
WIDE_FULL = dict(S=110, step=3)
WIDE_INDEXED = dict(S=330, step=2, indexed_only=True)


def minor_chains(model):
    """[good, bad, good] on the MINOR subject: the bad chain has sigma2_err = exp(-800) = 0 exactly and a zero row 2 of L (for the
    nonseparable model: of observation 2's own L), so row and column 2 of S are exactly 0 and the third pivot is exactly 0."""
    c = build(MINOR)
    N, T = c["N"], c["T"]
    assert c["indx"][2] == 2
    P = c["pars"][model]
    bad = P[1].copy()
    bad[-1] = -800.0
    if model == "sta":
        bad[2 + 3:2 + 6] = 0.0
    elif model == "sep":
        bad[2 * N + 3:2 * N + 6] = 0.0
    else:
        bad[N + 2 * T + 3:N + 2 * T + 6] = 0.0
    return np.stack([P[0], bad, P[1]])
