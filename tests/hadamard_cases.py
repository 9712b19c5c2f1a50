"""Synthetic subjects for the Hadamard sweep (tests/test_hadamard_sweep_cpu.py, tests/test_gpu_hadamard_sweep.py): every M from 1 to 8,
the edges of the 64 x 64 tiles, four label layouts next to the fixtures' interleaved one, and one slice wider than 256 riding rows.
A plain module, not a conftest: both halves import it, so the CPU half checks the very subjects the GPU half runs.  The cohort sets of
tests/hadamard_cohort_cases.py are built from the same subjects; the measure the gradients are held to block by block, for the
resident entries and the cohort alike, is at the end of this file (block_bar)."""
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


# ---- the gradients block by block ------------------------------------------------------------------------------------------------------
# One whole-vector norm hides a block: at (129, 4, unsorted) the smallest slot column of the nonseparable likelihood gradient is 0.027
# of ||g|| and the last observation's tilde_l entry 0.003 of it, so a slot column wrong by 1e-7 relative moves ||dg|| / ||g|| by
# 2.7e-9, below the whole-vector 1e-8.  The gradients are therefore also taken block by block with the measure of
# tests/objective_cases.py (block_table: ||d_b|| / max(||g_b||, 1e-3 ||g||)); "had" has the nonseparable complete-data layout ("svc":
# tilde_l, every slot column of uL, sigma2), "sep" the separable one, "sta" the four scalars' one.
#
# Without the priors, and for "sta" with them too, every block of a subject is held to
#     block_bar = min(GRAD_TIGHT, max(100 d_cpu, N_s cond(S) eps))
# d_cpu: the worst block, over the subject's two chains, between two CPU references -- the per-subject restatement (ref_logpos) and the
# padded formulation of the CPU halves (tests/test_hadamard_cohort_cpu.py, tests/test_hadamard_cohort_models_cpu.py) at the set's Nmax
# (the resident sweep: Nmax = N_s); the factor 100 is the rule of prediction_cases.tight().  N_s cond(S) eps (eps = 2^-52, the larger
# cond of the two chains) is what a backward-stable solve may lose at that conditioning.  No device figure enters a bar.  Measured on
# the CPU (tests/test_hadamard_cohort_cpu.py::test_block_bars_rest_on_two_cpu_references prints both terms per subject):
# d_cpu <= 2.7e-14 per block on sets F - H and <= 8.8e-14 on set I, over the three models; the bar comes to about 4e-11 at (257, 7) and
# 8.6e-10 at (1030, 2), and at the smallest subjects to the 100 d_cpu term or to N_s eps itself (2.2e-16 at N_s = M = 1).  Achieved on
# the MI355X (profiles/parity_hadamard_cohort_sweep.json): every block at or below 0.16 of its bar, 7 % at sets F - H (1.3e-13 against
# 1.9e-12 at (6, 6)), about 2e-13 against 7.6e-10 on set I; the prior part at most 1.3e-8 against 1e-5.
#
# With the GP priors ("had", "sep": factors of condition number up to 1e11) the prior part g(prior) - g(no prior) is compared block by
# block with the same difference of the restatement at the standing 1e-5; the CPU halves hold the two LAPACK blockings of that
# reference (the subject alone, and padded to Nmax) to PRIOR_PART_REFERENCE = 1e-7 per block (measured: <= 7.9e-10 on sets A - H, <= 3.5e-9 on set I).
GRAD_TIGHT = 1e-8
MACHINE_EPS = 2.0 ** -52
PRIOR_PART_REFERENCE = 1e-7
LAYOUT = {"had": "svc", "sep": "sep", "sta": "sta"}
# (layout name, N, M, block name) -> bar of a likelihood-gradient block that needs one of its own: ten times a discrepancy measured
# between two CPU references, with the figure beside it (the rule of tests/objective_cases.py).  The subject (1, 1): one observation of
# one output.  The two references of d_cpu run the same scalar operations there (d_cpu = 0 for "had" and "sep"), so the rule gives
# N_s cond(S) eps = 1 eps = 2.2e-16, while the restatement itself is further than that from a closed form in np.longdouble
# (tests/test_hadamard_cohort_cpu.py::test_the_single_observation_subject_has_bars_from_a_longdouble_reference; worst of the two chains):
BLOCK_BARS = {
    ("sep", 1, 1, "tilde_sigma"): 3.5e-15,       # measured 3.43e-16
    ("sep", 1, 1, "uL_vec"): 2.9e-15,            # measured 2.85e-16
    ("sep", 1, 1, "sigma2"): 3.4e-15,            # measured 3.37e-16
    ("svc", 1, 1, "uL[0,0]"): 1.9e-15,           # measured 1.87e-16 ("had")
    ("svc", 1, 1, "sigma2"): 5.9e-16,            # measured 5.80e-17 ("had")
}


def layout(model, N, M):
    """the block layout of objective_cases.blocks for a model's gradient"""
    return (LAYOUT[model], N, M)


@functools.lru_cache(maxsize=None)
def reference(model, case, chain, prior):
    """(verbose tuple, d NegLog / d pars) of the restatement on the subject alone; computed once, shared, left unchanged"""
    c = build(case)
    return ref_logpos(model, c["pars"][model][chain], c, prior, grad=True)


@functools.lru_cache(maxsize=None)
def padded_reference(model, case, chain, prior, Nmax):
    """the same of the padded formulation the device runs, restated in the CPU halves, under LAPACK at order Nmax"""
    from test_hadamard_cohort_cpu import padded_logpos
    from test_hadamard_cohort_models_cpu import PADDED
    c = build(case)
    fn = padded_logpos if model == "had" else PADDED[model]
    return fn(c["pars"][model][chain], c, Nmax, prior)


@functools.lru_cache(maxsize=None)
def cond_S(model, case, chain):
    c = build(case)
    return float(np.linalg.cond(ref_covariance(model, c["pars"][model][chain], c)))


def block_table(g, gref, model, N, M):
    from objective_cases import block_table as table
    return table(g, gref, layout(model, N, M))


@functools.lru_cache(maxsize=None)
def block_bar_terms(model, case, Nmax=None):
    """(d_cpu, N_s cond(S) eps) of a subject in a set padded to Nmax (None: the subject alone)"""
    N, M = case[0], case[1]
    Nmax = N if Nmax is None else Nmax
    d = 0.0
    for k in (0, 1):
        for prior in ((False, True) if model == "sta" else (False,)):
            tab = block_table(padded_reference(model, case, k, prior, Nmax)[1], reference(model, case, k, prior)[1], model, N, M)
            d = max(d, max(tab.values()))
    return d, N * max(cond_S(model, case, k) for k in (0, 1)) * MACHINE_EPS


def block_bar(model, case, Nmax=None):
    d, stable = block_bar_terms(model, case, Nmax)
    return min(GRAD_TIGHT, max(100.0 * d, stable))


def prior_part(model, case, chain, Nmax=None):
    """g(prior) - g(no prior) of the restatement (Nmax: of the padded formulation at that order)"""
    if Nmax is None:
        return reference(model, case, chain, True)[1] - reference(model, case, chain, False)[1]
    return padded_reference(model, case, chain, True, Nmax)[1] - padded_reference(model, case, chain, False, Nmax)[1]


def block_entries(prefix, g, gref, model, N, M, bar, bars=None):
    """{"prefix[block]": (achieved, bar)} for check(); `bars`: a table like BLOCK_BARS with the blocks that have a bar of their own"""
    lay = layout(model, N, M)
    return {"%s[%s]" % (prefix, name): (e, (bars or {}).get(lay + (name,), bar)) for name, e in block_table(g, gref, model, N, M).items()}
