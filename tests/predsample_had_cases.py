"""The NumPy restatement of the posterior-draw / held-out prediction of the nonseparable Hadamard model (nmgp_predsample_had) and the
inputs both halves of its tests share (tests/test_predsample_had_cpu.py, tests/test_gpu_predsample_had.py).  A plain module, not a
conftest.  Subjects, draws and grids are tests/hadamard_cases.py's: build(case)["pars"]["had"] as two draws, grid, grid_labels.

The restatement is built from pieces that fixtures already pin: oracle._gp_regress (the conditional means of the starred values),
the conditional-variance expression of tests/test_predsample_cpu.py's restatement, and test_hadamard_cpu.had_covariance / had_rows.
The reference has no posterior-draw form for this model; its MAP predictor is had_predict (z = 0, one draw)."""
import functools
import math

import numpy as np
from scipy.linalg import cho_solve, cholesky, solve_triangular

import hadamard_cases as hc
from conftest import golden
from oracle import nmgp_oracle as oracle

JITTER, PRECISION = 1e-6, 1e-6
FIXTURES = ("had_N77_M3", "had_N200_M4")                 # M = 3 / 4 of the parity sweep


def clip_cv(raw):
    """A conditional variance < 0 is replaced by settings.precision (nmgp_predsample_svc's rule)."""
    return np.where(raw < 0, PRECISION, raw)


def cond_var(x, xs, alpha, beta):
    """The clipped conditional variances [S] of one GP prior (test_predsample_cpu.regression's expression; a value < 0 -> 1e-6)."""
    X1 = x.reshape(-1, 1)
    k = oracle.RBF_cov(X1, xs.reshape(-1, 1), alpha=alpha, beta=beta)
    proj = np.linalg.solve(oracle.RBF_cov(X1, alpha=alpha, beta=beta), k)
    return clip_cv((alpha ** 2 + JITTER) - np.sum(proj * k, axis=0))


def restate_hpn(x, indx, y, draws, hyper, xs, z, indx_star=None):
    """draws [H, N(1+T)+1], xs [S], z [H, S, 1+T] or None (the conditional means) -> (mean, raw variance BEFORE the clip, star
    [H, S, 1+T]); mean and variance are [H, S, M], or [H, S] with indx_star [S] (output indx_star[s] only at xs[s])."""
    from test_hadamard_cpu import had_covariance, had_rows
    x, y, xs = (np.asarray(v, dtype=np.float64) for v in (x, y, xs))
    draws = np.atleast_2d(np.asarray(draws, dtype=np.float64))
    indx = np.asarray(indx).astype(np.int64)
    N, M = x.shape[0], int(np.unique(indx).shape[0])
    T = M * (M + 1) // 2
    mu_l, al_l, be_l, mu_L, al_L, be_L = [float(v) for v in hyper[:6]]
    H, S = draws.shape[0], xs.shape[0]
    z = np.zeros((H, S, 1 + T)) if z is None else np.asarray(z, dtype=np.float64)
    sd_l, sd_L = np.sqrt(cond_var(x, xs, al_l, be_l)), np.sqrt(cond_var(x, xs, al_L, be_L))
    r, c = oracle.tril_slots(M)
    shape = (H, S, M) if indx_star is None else (H, S)
    mean, raw, star = np.zeros(shape), np.zeros(shape), np.zeros((H, S, 1 + T))
    for h in range(H):
        p = draws[h]
        tl, Lv, tse = p[:N], p[N:N + N * T].reshape(N, T), float(p[-1])
        sigma2 = math.exp(tse)
        star[h, :, 0] = oracle._gp_regress(x, xs, tl, mu_l, al_l, be_l) + sd_l * z[h, :, 0]
        for t in range(T):                                                           # the slots as they are: no exp
            star[h, :, 1 + t] = oracle._gp_regress(x, xs, Lv[:, t], mu_L, al_L, be_L) + sd_L * z[h, :, 1 + t]
        C = cholesky(had_covariance(tl, Lv, tse, x, indx, M), lower=True)
        alpha = cho_solve((C, True), y)
        R = had_rows(Lv, indx, M)
        ell = np.exp(tl)
        for s in range(S):
            kx = oracle.Nonstationary_RBF_cov(x.reshape(-1, 1), sigma1=np.ones(N), ell1=ell, X2=xs[s].reshape(1, 1),
                                              sigma2=np.ones(1), ell2=np.array([math.exp(star[h, s, 0])]))[:, 0]     # no jitter
            Ls = np.zeros((M, M))
            Ls[r, c] = star[h, s, 1:]
            ms = np.arange(M) if indx_star is None else np.array([int(indx_star[s])])
            kf = kx[:, None] * (R @ Ls[ms].T)                                         # [N, K]
            V = solve_triangular(C, kf, lower=True)
            m = kf.T @ alpha
            v = (1.0 + JITTER) * np.diag(Ls @ Ls.T)[ms] - (V * V).sum(0) + sigma2
            mean[h, s], raw[h, s] = (m, v) if indx_star is None else (m[0], v[0])
    return mean, raw, star


# ---- the cases of the GPU parity sweep -----------------------------------------------------------------------------------------------
# every M from 1 to 8 but 3 and 4 (the fixtures'): N = M (slices of one input) and the edges of the 64-wide tiles
SWEEP = [(1, 1, "interleaved"), (2, 2, "interleaved"), (8, 8, "interleaved"), (5, 5, "unsorted"), (63, 2, "blocks"),
         (64, 5, "rare_last"), (65, 6, "rare_first"), (129, 7, "unsorted"), (193, 8, "blocks")]
assert all(c in hc.CASES for c in SWEEP)
PARITY = SWEEP + list(FIXTURES)


def parity_id(case):
    return case if isinstance(case, str) else hc.case_id(case)


@functools.lru_cache(maxsize=None)
def subject(case):
    """dict(N, M, T, x, indx, y, draws [2, P], hyper [8], seed): a hadamard_cases subject with its two chains as draws, or a fixture
    with (pars, pars2) as draws.  The arrays are shared: do not write into them."""
    if isinstance(case, str):
        g = golden(case)
        M = int(g["M"])
        draws = np.stack([g["pars"], g["pars2"] if "pars2" in g else g["pars"] + 0.01])
        return dict(N=g["x"].shape[0], M=M, T=M * (M + 1) // 2, x=g["x"], indx=g["indx"], y=g["y"], draws=draws, hyper=g["hyper"],
                    seed=10 * g["x"].shape[0] + M)
    c = hc.build(case)
    return dict(N=c["N"], M=c["M"], T=c["T"], x=c["x"], indx=c["indx"], y=c["y"], draws=c["pars"]["had"], hyper=c["hyper"]["had"],
                seed=hc.case_seed(case))


def new_inputs(case, S=None, step=None):
    """(xs [S], labels [S]): hadamard_cases.grid / grid_labels for a sweep case (S = 2 (N // M) + 1 below N = 64: three full-form
    slices, the last ragged; 11 otherwise); the fixture's own 9-point grid for a fixture, unless S is given (then linspace(-0.02, 1.02,
    S) with a training input in slot 1).  The labels are (step s) % M with step = 3, or 5 where 3 divides M (every label occurs
    once S >= M)."""
    c = subject(case)
    if step is None:
        step = 5 if c["M"] % 3 == 0 else 3
    if isinstance(case, str) and S is None:
        xs = golden(case)["grids"]
    elif isinstance(case, str):
        xs = np.linspace(-0.02, 1.02, S)
        xs[1] = c["x"][0]
    else:
        xs = hc.grid(c["N"], c["M"], c["x"], S)
    return xs, hc.grid_labels(xs.shape[0], c["M"], step)


def normals(case, S):
    """The fixed standard normals z [2, S, 1+T] of the two draws' latent regressions."""
    c = subject(case)
    return np.random.default_rng(c["seed"] + 1).standard_normal((2, S, 1 + c["T"]))


@functools.lru_cache(maxsize=None)
def expected(case, S=None, step=None, indexed_only=False):
    """The restatement's (mean, raw, star) in the full ('full') and indexed ('ix') forms under normals(case, S), with the inputs:
    computed once and shared; do not write into the arrays."""
    c = subject(case)
    xs, lab = new_inputs(case, S, step)
    z = normals(case, xs.shape[0])
    out = dict(xs=xs, lab=lab, z=z)
    out["ix"] = restate_hpn(c["x"], c["indx"], c["y"], c["draws"], c["hyper"], xs, z, lab)
    if not indexed_only:
        out["full"] = restate_hpn(c["x"], c["indx"], c["y"], c["draws"], c["hyper"], xs, z)
    return out


def raw_variance_floor(exp, case):
    """min over every compared raw variance of (variance / sigma2_err of its draw): > 1 means the clip to 1e-6 plays no part
    (hadamard_cases.raw_variance_floor's idea for this entry)."""
    s2 = np.exp(subject(case)["draws"][:, -1])
    r = [np.min(exp[k][1][h]) / s2[h] for k in ("ix", "full") if k in exp for h in (0, 1)]
    return float(min(r))


# one slice wider than 256 riding rows (hadamard_cases.WIDE, N = 321, M = 3): full form 107 inputs = 321 rows, then 3; indexed form
# 321 rows, then 9
WIDE = hc.WIDE
WIDE_FULL = dict(S=110, step=2)
WIDE_INDEXED = dict(S=330, step=2, indexed_only=True)
