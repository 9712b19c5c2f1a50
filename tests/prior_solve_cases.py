"""Subjects, chains, references, measure, case tables, mutations and the branch inventory of the GP-prior solve sweep
(tests/test_prior_solve_cpu.py, tests/test_gpu_prior_solve.py).  A plain module, not a conftest: both halves import it, so the CPU half
checks the very subjects, chains and references the GPU half runs against.

The family is that of tests/metric_cases.py, whose helpers are used here and not copied: pair A = (alpha 1e-3, beta 0.3) for tilde_l,
pair B = (alpha 3e-3, beta 0.2) for the uL columns (separable models: tilde_sigma), mu = 0; the "same" variant uses A for both.  For ANY
inputs, duplicates included, K = jitter I + alpha^2 G with 0 <= G_ij <= 1, so kappa(K) <= 1 + N alpha^2 / jitter (386 for A, 3466 for B
at N = 385): the factors are well conditioned and, on inputs spread over [0, 1], populated far from the diagonal.  Both are asserted per
subject in the CPU half.  A and B differ, so a swap of factors, leading dimensions or strides cannot cancel.

The reference is np.longdouble: the covariance from (x_i - x_j)^2, a column Cholesky (metric_cases.cov_ld / chol_ld), plain
substitutions.  Per chain it gives q_c = ||L^-1 (v_c - mu)||^2 per column, the half log-determinants, the two verbose prior components
and Sigma^-1 (v_c - mu) per column.  The float64 restatement (oracle.RBF_cov -> np.linalg.cholesky -> scipy solves) is what the CPU half
measures against it; 50 x the worst figure per table is the GPU bar (RESTATEMENT_WORST, BAR), never above 1e-10: a margin over the
reference's own error, not over the code under test.

What the GPU half measures: the PRIOR PART of the gradient, g(prior = 1) - g(prior = 0) of two calls on the same chains, block by block
(tilde_l and every stride-T slot column of uL; tilde_l and tilde_sigma in the separable models; the sigma2 entry and the separable uL_vec
belong to other priors), ||d_b|| / ||ref_b||; and the two verbose prior components relative to themselves."""
import functools
import math

import numpy as np

import metric_cases as MC

LD = MC.LD
JITTER = MC.JITTER
PAIR = {"A": MC.HYPER_A, "B": MC.HYPER_B}
VARIANTS = ("same", "diff")                     # same: pl == pL in the library; diff: two cached factors
LOG_2PI = math.log(2.0 * math.pi)
SEP_C = 10.0
BLOCK = 64                                      # k_prior_trsv's block width
GEMV_ROWS = 256                                 # rows per pass of its forward GEMV (16 waves x 16 rows)


def pairs(variant):
    """((alpha, beta) of column 0, (alpha, beta) of the other columns)"""
    return (PAIR["A"], PAIR["A"]) if variant == "same" else (PAIR["A"], PAIR["B"])


def hyper_vec(layout, variant):
    (a0, b0), (a1, b1) = pairs(variant)
    hv = [0.0, a0, b0, 0.0, a1, b1, 1.0, 1.0]
    return np.array(hv + [SEP_C] if layout == "sep" else hv)


def kappa_bound(N, alpha):
    return 1.0 + N * alpha * alpha / JITTER


n_slots = MC.n_slots


def _ro(a):
    a.setflags(write=False)
    return a


# ---------------------------------------------------------------------------------------------------
# the tables
# ---------------------------------------------------------------------------------------------------
# Table A: logpos_svc and svc_batch_eval on the resident subject, x = linspace(0, 1, N).  N: one location; 63 / 64 / 65 around the
# 64-wide block (65: a ragged last block of one row and, N odd, the row pair that reads a column's padding); 129, 193 (the 128-column
# stride of the transposed GEMV: columns 128 .. 191 are a wave's second trip), 257, 385 (rows 320 .. 384 below block 0: a second
# 256-row pass of the forward GEMV).  M = 1, 2, 3, 4, 8: T = 1, 3, 6, 10, 36.
TABLE_A = [(1, 1), (63, 2), (64, 8), (65, 3), (129, 4), (193, 1), (257, 2), (385, 3)]
BATCHES_A = (1, 5)
# Table B: svc_batch_set_subjects, N = 65 (ld = 80: the factor stride ld N is not N^2), subject s on linspace(0, 1 + 0.1 s, N).
# (M, chains per subject): B (1 + T) = 24 and 12 (library forms), 33 and 66 (substitution by default) -- both sides of 32.
TABLE_B = [(2, 2), (2, 1), (4, 1), (4, 2)]
N_B, SUBJECTS = 65, 3
SUBST_MIN_COLUMNS = 32                          # nmgp_svc_batch_eval: multi-subject batches of B (1 + T) >= 32 columns substitute
# Table C: logpos_sep and sep_batch_eval, resident (the 2 B-column call / the per-chain pair) and 3 subjects x 2 chains
TABLE_C = [(64, 3), (65, 1), (129, 8), (385, 2)]
BATCH_C = 3
SUBJECT_CASES_C = [(65, 1), (129, 8)]
CPS_C = 2
# Table D: had_batch_eval and hads_batch_eval on the subjects of tests/hadamard_cases.py (sorted inputs with a repeated time stamp;
# "unsorted": permuted).  M = 1, 2, 5, 8.
TABLE_D = [(63, 1, "unsorted"), (65, 2, "blocks"), (129, 5, "unsorted"), (193, 8, "rare_last"), (385, 2, "unsorted")]
BATCHES_D = (1, 3)
# Table E: had_subjects_eval on a ragged cohort: per-subject factor offsets s0 ld Nmax and masked factors; the reference is each
# subject alone at its own N.
COHORT_NOBS = (65, 2, 64)
COHORT_M = 2
COHORT_CPS = (1, 2)
# once more with 5000 chains per subject (the two chains tiled) under NMGP_HAD_BATCH_SLAB_GB = 1, the smallest cap: a chain with
# gradient takes 0.12 MB of workspace at Nmax = 65, so the call runs as three whole-subject chunks that start at subjects 0, 1, 2
# (cohort_chunks; asserted in the CPU half) -- the chunk's factor and log-determinant offsets at s0 > 0
COHORT_SPLIT_CPS, COHORT_SPLIT_CAP_GB = 5000, 1.0
# Table P: the projections of the predictors, S = 7 new inputs of which slot 1 is a training input
TABLE_P = [(65, 2), (321, 2)]
S_NEW = 7

# Worst error of the float64 restatement against np.longdouble, per table, over every case, variant, chain and block (gradient blocks
# and the two components alike): tests/test_prior_solve_cpu.py measures it, prints the figures and asserts that none exceeds its
# entry here.  Measured (x86-64, 80-bit long double, OpenBLAS): A 9.2e-14 (N = 385, M = 3, different pairs, slot column uL[2,2]),
# B 5.7e-14, C 6.9e-14 (N = 385, tilde_sigma), D 1.05e-13 (N = 385, unsorted inputs, uL[0,0]), E 3.9e-14, P 7.9e-14 (N = 321,
# sqrt(cv) as the GPU half sees it); q_c and the half log-determinants are measured too and sit below the gradient blocks.  The
# entries are these with half as much again for another BLAS's rounding.
RESTATEMENT_WORST = {"A": 1.4e-13, "B": 9e-14, "C": 1.1e-13, "D": 1.6e-13, "E": 6e-14, "P": 1.2e-13}
MARGIN = 50.0
BAR_CAP = 1e-10
BAR = {k: min(MARGIN * v, BAR_CAP) for k, v in RESTATEMENT_WORST.items()}
REJECT = 100.0                                  # a mutation is rejected by an error >= REJECT x the bar


# ---------------------------------------------------------------------------------------------------
# factors of arbitrary inputs
# ---------------------------------------------------------------------------------------------------
_FACTORS = {}


def factor(x, hyper, prec="ld"):
    """Lower Cholesky factor of RBF(x; alpha, beta) + 1e-6 I: longdouble ("ld") or the float64 restatement ("f64"); read-only, cached
    on the inputs' bytes."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    key = (x.tobytes(), float(hyper[0]), float(hyper[1]), prec)
    if key not in _FACTORS:
        if prec == "ld":
            L = MC.chol_ld(MC.cov_ld(x, *hyper))
        else:
            L = np.linalg.cholesky(MC.cov_f64(x, *hyper))
        _FACTORS[key] = _ro(L)
    return _FACTORS[key]


def solve_lower(L, r):
    """L z = r by plain forward substitution (columns of r at once), in the precision of L"""
    z = np.array(r, dtype=L.dtype, copy=True)
    for i in range(L.shape[0]):
        z[i] = (z[i] - L[i, :i] @ z[:i]) / L[i, i]
    return z


def solve_upper(L, z):
    """L^T w = z by plain back substitution"""
    w = np.array(z, dtype=L.dtype, copy=True)
    for i in range(L.shape[0] - 1, -1, -1):
        w[i] = (w[i] - L[i + 1:, i] @ w[i + 1:]) / L[i, i]
    return w


def _fwd(L, r):
    if L.dtype == np.float64:
        from scipy.linalg import solve_triangular
        return solve_triangular(L, r, lower=True)
    return solve_lower(L, r)


def _bwd(L, z):
    if L.dtype == np.float64:
        from scipy.linalg import solve_triangular
        return solve_triangular(L, z, lower=True, trans="T")
    return solve_upper(L, z)


def half_logdet(L):
    return np.sum(np.log(np.diag(L)))


# ---------------------------------------------------------------------------------------------------
# mutations of the solves: each returns the WRONG result
# ---------------------------------------------------------------------------------------------------
MUTATIONS = ("col0_against_B", "last_column_against_A", "forward_solve_only", "subject1_with_subject0_factors",
             "second_gemv_pass_dropped", "ragged_block_unguarded")


def ld_of(N):
    return (N + 15) // 16 * 16                  # leading dimension of a cached prior factor


def _fwd_second_pass_dropped(L, r):
    """(v) the forward sweep without its second 256-row pass: L_ik = 0 for rows 320 or more below the top of k's diagonal block"""
    i, k = np.indices(L.shape)
    Lm = np.where(i >= (k // BLOCK) * BLOCK + BLOCK + GEMV_ROWS, 0, L).astype(L.dtype)
    Lm[np.diag_indices_from(Lm)] = np.diag(L)
    return _fwd(Lm, r)


def _bwd_ragged_unguarded(L, z):
    """(vi) the transposed sweep with both guards of the ragged last block gone: its rows k >= nbk are loaded all the same -- from the
    factor's column-major storage they are the column's padding and then the top of the NEXT column -- and meet the block's solution
    wrapped round (lane k holds x[k mod nbk]) instead of zeros."""
    N = L.shape[0]
    kb = (N - 1) // BLOCK * BLOCK
    nbk = N - kb
    if nbk == BLOCK or kb == 0:
        return _bwd(L, z)
    ld = ld_of(N)
    flat = np.zeros(ld * (N + 1), dtype=L.dtype)
    flat[:ld * N].reshape(N, ld)[:, :N] = L.T                     # column-major with leading dimension ld
    w = np.array(z, dtype=L.dtype, copy=True)
    x_last = _bwd(L[kb:, kb:], w[kb:])
    rest = w[:kb] - L[kb:, :kb].T @ x_last
    k = np.arange(nbk, BLOCK)
    extra = flat[(np.arange(kb) * ld + kb)[:, None] + k[None, :]]  # [kb, 64 - nbk]
    rest = rest - extra @ x_last[k % nbk]
    w[kb:] = x_last
    w[:kb] = _bwd(L[:kb, :kb], rest)
    return w


def mutation_acts(name, N, variant):
    return {"col0_against_B": variant == "diff", "last_column_against_A": variant == "diff", "forward_solve_only": True,
            "subject1_with_subject0_factors": True, "second_gemv_pass_dropped": N > BLOCK + GEMV_ROWS,
            "ragged_block_unguarded": N > BLOCK and N % BLOCK != 0}[name]


# ---------------------------------------------------------------------------------------------------
# the reference and its restatement
# ---------------------------------------------------------------------------------------------------
def gp_blocks(layout, N, M):
    """[(name, index, factor 0 | 1)] of the blocks under a GP prior"""
    bl = MC.blocks(layout, N, M)
    if layout == "svc":
        return [(bl[0][0], bl[0][1], 0)] + [(n, sl, 1) for n, sl in bl[1:-1]]
    return [(bl[0][0], bl[0][1], 0), (bl[1][0], bl[1][1], 1)]


def prior_terms(x, layout, M, V, variant=None, prec="ld", mutation=None, hypers=None):
    """The prior quantities of the chains V [B, P] on the inputs x, in longdouble (prec "ld") or as the float64 restatement ("f64"):
    dict(q [B, ncol], hld [2], comps [B, 2] = the two verbose prior components, grad [B, P] = Sigma^-1 (v - mu) on the GP blocks (zero
    elsewhere)).  hypers: the two (alpha, beta) instead of the variant's.  mutation: one of MUTATIONS (the subject mix-up is made by
    the caller, who hands in the other subject's x)."""
    x = np.asarray(x, dtype=np.float64)
    N = x.shape[0]
    dt = LD if prec == "ld" else np.float64
    V = np.atleast_2d(np.asarray(V, dtype=dt))
    hy = hypers if hypers is not None else pairs(variant)
    Ls = [factor(x, hy[0], prec), factor(x, hy[1], prec)]
    bl = gp_blocks(layout, N, M)
    q = np.zeros((V.shape[0], len(bl)), dtype=dt)
    grad = np.zeros(V.shape, dtype=dt)
    comps = np.zeros((V.shape[0], 2), dtype=dt)
    hld = [half_logdet(L) for L in Ls]
    for c, (name, sl, f) in enumerate(bl):
        if mutation == "col0_against_B" and c == 0:
            f = 1
        if mutation == "last_column_against_A" and c == len(bl) - 1:
            f = 0
        L = Ls[f]
        r = V[:, sl].T                                              # [N, B], mu = 0
        z = _fwd_second_pass_dropped(L, r) if mutation == "second_gemv_pass_dropped" else _fwd(L, r)
        if mutation == "forward_solve_only":
            w = z
        elif mutation == "ragged_block_unguarded":
            w = _bwd_ragged_unguarded(L, z)
        else:
            w = _bwd(L, z)
        q[:, c] = np.sum(z * z, axis=0)
        grad[:, sl] = w.T
        comps[:, 0 if c == 0 else 1] += -dt(0.5) * q[:, c] - hld[f] - dt(0.5 * N * LOG_2PI)
    return dict(q=q, hld=np.array(hld, dtype=dt), comps=comps, grad=grad)


def errors(got_comps, got_grad, ref, layout, N, M):
    """{name: error} of one or more chains against prior_terms' result: the gradient blocks ||d_b|| / ||ref_b|| (got_grad None: left
    out), the components |d| / |ref|; differences in longdouble; the worst chain per name.  A non-finite value is an infinite error."""
    out = {}
    gc = np.atleast_2d(np.asarray(got_comps, dtype=LD))
    rc = np.asarray(ref["comps"], dtype=LD)
    assert gc.shape == rc.shape, (gc.shape, rc.shape)
    for j, name in enumerate(("component0", "component1")):
        e = np.abs(gc[:, j] - rc[:, j]) / np.abs(rc[:, j])
        out[name] = float(np.max(e)) if np.all(np.isfinite(e)) else np.inf
    if got_grad is not None:
        gg = np.atleast_2d(np.asarray(got_grad, dtype=LD))
        rg = np.asarray(ref["grad"], dtype=LD)
        assert gg.shape == rg.shape, (gg.shape, rg.shape)
        for name, sl, _ in gp_blocks(layout, N, M):
            d = np.sqrt(np.sum((gg[:, sl] - rg[:, sl]) ** 2, axis=1)) / np.sqrt(np.sum(rg[:, sl] ** 2, axis=1))
            out[name] = float(np.max(d)) if np.all(np.isfinite(d)) else np.inf
    return out


def worst(errs):
    k = max(errs, key=lambda n: errs[n])
    return errs[k], k


def far_population(L):
    """max |L_ij| over i - j >= 64, relative to the largest off-diagonal entry"""
    i, j = np.indices(L.shape)
    A = np.abs(np.asarray(L, dtype=np.float64))
    return float(np.max(A[i - j >= BLOCK]) / np.max(A[i > j]))


# ---------------------------------------------------------------------------------------------------
# subjects and chains
# ---------------------------------------------------------------------------------------------------
def complete_subject(N, M, s=0):
    """(x, Y) of the complete-data tables: metric_cases.data"""
    return MC.data(N, M, s)


@functools.lru_cache(maxsize=None)
def complete_chains(layout, N, M, B, s=0):
    """[B, P] chains of a complete-data subject: smooth curves plus standard normals of amplitude 0.05, so that every column has a
    rough part (Sigma^-1 v ~ 0.05 / jitter: the prior part dominates the gradient it is read from) -- one seed per chain, the first
    rows the same for every B; B = 5: the last chain is a copy of chain 0."""
    x = MC.grid(N, s)
    T = n_slots(M)
    rows = []
    for k in range(min(B, 4)):
        rng = np.random.default_rng(900000 + 1000 * N + 100 * M + 10 * s + k + (0 if layout == "svc" else 7))
        tl = -1.2 + 0.2 * np.sin(5.0 * x + k) + 0.05 * rng.standard_normal(N)
        if layout == "svc":
            base = np.tile(0.2 * np.sin(1.0 + np.arange(T)), (N, 1)) * (1.0 + 0.3 * np.cos(3.0 * x + k))[:, None]
            uL = base + 0.05 * rng.standard_normal((N, T))
            rows.append(np.concatenate([tl, uL.reshape(-1), [-2.0 + 0.01 * k]]))
        else:
            ts = 0.1 * np.cos(4.0 * x + k) + 0.05 * rng.standard_normal(N)
            uL = 0.2 * np.sin(1.0 + np.arange(T) + k)
            rows.append(np.concatenate([tl, ts, uL, [-2.0 + 0.01 * k]]))
    v = np.stack(rows)
    v = np.concatenate([v, v[:1]])[:B] if B == 5 else v[:B]
    return _ro(np.ascontiguousarray(v))


@functools.lru_cache(maxsize=None)
def hadamard_subject(N, M, layout, seed=None):
    """dict(x, indx, y, chains {"svc": [3, N (1 + T) + 1], "sep": [3, 2 N + T + 1]}) of a Hadamard subject of tests/hadamard_cases.py:
    its two chains and a third (chain 0's curves, chain 1's last slots), each with standard normals of amplitude 0.05 on the curves."""
    import hadamard_cases as hc
    x, indx, y, L_vec = hc.subject(N, M, layout, 10 * N + M if seed is None else seed)
    P = hc.parameters(x, M, L_vec)
    T = n_slots(M)
    out = dict(x=_ro(x), indx=_ro(indx), y=_ro(y), chains={})
    for lay, model, ncurve in (("svc", "had", N * (1 + T)), ("sep", "sep", 2 * N)):
        rows = []
        for k in range(3):
            rng = np.random.default_rng(800000 + 1000 * N + 100 * M + k + (0 if lay == "svc" else 7))
            p = P[model][k % 2].copy()
            p[:ncurve] += 0.05 * rng.standard_normal(ncurve)
            rows.append(p)
        out["chains"][lay] = _ro(np.stack(rows))
    return out


def cohort():
    """The ragged cohort of table E: subjects of COHORT_NOBS observations ("unsorted" layout), two chains each"""
    return [hadamard_subject(n, COHORT_M, "unsorted", 77 + n) for n in COHORT_NOBS]


def new_inputs(x):
    """S_NEW new inputs over [-0.05, 1.05]; slot 1 is a training input"""
    xs = np.linspace(-0.05, 1.05, S_NEW)
    xs[1] = x[len(x) // 3]
    return xs


def projection_terms(x, xs, layout, M, V, variant, prec="ld", curve=None):
    """The starred values of the chains V [B, P] at the new inputs xs: dict(star [B, S, ncol] = mu + k*^T Sigma^-1 (v - mu) per GP
    block, sd [2, S] = sqrt(cv) per factor, cv = alpha^2 + jitter - k*^T Sigma^-1 k*).  curve: a map applied to V first (the
    constrained L_vecs of predsample_svc).  In float64 the restatement's sd is what the GPU half measures: (star + sd) - star."""
    x, xs = np.asarray(x, dtype=np.float64), np.asarray(xs, dtype=np.float64)
    N, S = x.shape[0], xs.shape[0]
    dt = LD if prec == "ld" else np.float64
    V = np.atleast_2d(np.asarray(V, dtype=dt))
    if curve is not None:
        V = curve(V)
    hy = pairs(variant)
    bl = gp_blocks(layout, N, M)
    W, cv = [], np.zeros((2, S), dtype=dt)
    for f in (0, 1):
        alpha, beta = hy[f]
        L = factor(x, hy[f], prec)
        d = (np.asarray(x, dtype=dt)[:, None] / dt(beta) - np.asarray(xs, dtype=dt)[None, :] / dt(beta)) ** 2
        ks = dt(alpha) ** 2 * np.exp(-d / dt(2))                    # [N, S]
        w = _bwd(L, _fwd(L, ks))
        W.append(w)
        cv[f] = (dt(alpha) ** 2 + dt(JITTER)) - np.sum(w * ks, axis=0)
    star = np.stack([V[:, sl] @ W[f] for _, sl, f in bl], axis=2)   # [B, S, ncol]
    sd = np.sqrt(cv)
    if prec != "ld":
        per_col = np.stack([sd[f] for _, _, f in bl], axis=1)[None]
        sd_seen = (star + per_col) - star
    else:
        sd_seen = np.broadcast_to(np.stack([sd[f] for _, _, f in bl], axis=1)[None], star.shape)
    return dict(star=star, cv=cv, sd=sd_seen)


def constrained_curve(N, M):
    """V -> V with exp on the diagonal slots of every location's uL (the curves predsample_svc regresses with constrained=True)"""
    T = n_slots(M)
    dslots = np.cumsum(np.arange(1, M + 1)) - 1

    def f(V):
        V = np.array(V, copy=True)
        U = V[:, N:N + N * T].reshape(V.shape[0], N, T)
        U[:, :, dslots] = np.exp(U[:, :, dslots])
        return V
    return f


def star_errors(got, ref):
    """max over chains and columns of ||got - ref|| / ||ref|| over the new inputs, for [B, S, ncol] starred values (differences in
    longdouble): a curve's regression passes through zero between new inputs, so the measure is per column, not per entry"""
    got, ref = np.asarray(got, dtype=LD), np.asarray(ref, dtype=LD)
    assert got.shape == ref.shape and got.ndim == 3, (got.shape, ref.shape)
    e = np.sqrt(np.sum((got - ref) ** 2, axis=1)) / np.sqrt(np.sum(ref ** 2, axis=1))
    return float(np.max(e)) if np.all(np.isfinite(e)) else np.inf


def rel_rows(got, ref):
    """max over the entries of |got - ref| / |ref| (differences in longdouble); a non-finite value is an infinite error"""
    got, ref = np.asarray(got, dtype=LD), np.asarray(ref, dtype=LD)
    e = np.abs(got - ref) / np.abs(ref)
    return float(np.max(e)) if np.all(np.isfinite(e)) else np.inf


# ---------------------------------------------------------------------------------------------------
# the branch inventory: every solve site and form in the sources, and the cases of the GPU half that reach each
# ---------------------------------------------------------------------------------------------------
# site/form -> what it is.  Both passes (forward, transposed) run wherever the gradient is asked for with the priors on, which every
# case of the GPU half does; the value-only calls run the forward pass alone.
INVENTORY = {
    "svc_enqueue/trsm_same": "nmgp_logpos_svc, pl == pL: one dtrsm over 1 + T columns",
    "svc_enqueue/trsm_pair": "nmgp_logpos_svc, pl != pL: dtrsm of column 0, dtrsm of the T others",
    "svc_enqueue/trsv": "nmgp_logpos_svc under NMGP_PRIOR_SOLVE=trsv: k_prior_trsv",
    "batch_core/resident_same": "nmgp_svc_batch_eval, resident subject, pl == pL: one dtrsm over B (1 + T) columns",
    "batch_core/resident_pair": "resident subject, pl != pL: two strided-batched dtrsm with factor stride 0",
    "batch_core/subjects_strided_same": "subject set, cps = 1, B (1 + T) < 32, pl == pL: one strided-batched dtrsm",
    "batch_core/subjects_strided_pair": "subject set, cps = 1, pl != pL: two strided-batched dtrsm with per-subject factor strides",
    "batch_core/subjects_loop_same": "subject set, cps > 1, pl == pL: one dtrsm over cps (1 + T) columns per subject",
    "batch_core/subjects_loop_pair": "subject set, cps > 1, pl != pL: two strided-batched dtrsm per subject",
    "batch_core/trsv": "k_prior_trsv: NMGP_PRIOR_SOLVE=trsv, or a subject set of B (1 + T) >= 32 columns",
    "prior_solve/trsm": "nmgp_eig.hip prior_solve: dtrsm (separable entries, resident subject)",
    "prior_solve/trsv": "prior_solve under NMGP_PRIOR_SOLVE=trsv",
    "sep_subjects/trsv": "sep_subjects_prior_solve: k_prior_trsv with per-subject factor strides (default)",
    "sep_subjects/trsm_same": "sep_subjects_prior_solve under rocblas, pl == ps: one dtrsm per subject",
    "sep_subjects/trsm_pair": "sep_subjects_prior_solve under rocblas, pl != ps: a strided pair per subject",
    "had_prior_solve/trsv": "had_prior_solve, N <= 3500: k_prior_trsv",
    "had_prior_solve/trsm_same": "had_prior_solve beyond N = 3500 or under rocblas, pl == pL: one dtrsm over B (1 + T) columns",
    "had_prior_solve/trsm_pair": "the same, pl != pL: two strided-batched dtrsm with R + N and stride (1 + T) N",
    "cohort/trsv": "hadc_gp_prior_terms: k_prior_trsv with per-subject factor offsets",
    "cohort/trsv_chunked": "the same in chunks that start at a later subject: factors and log-determinants offset by s0 > 0",
    "gp_project/trsv": "gp_project (nmgp_predict_svc / _sep): k_prior_trsv, forward and transposed",
    "gp_project/trsm": "gp_project under rocblas: the dtrsm pair",
    "project_rows/trsv": "project_rows (the posterior-draw predictors, nmgp_predict_had / _hads): k_prior_trsv, forward and transposed",
    "project_rows/trsm": "project_rows under rocblas: the dtrsm pair",
}
CONTEXTS = ("default", "rocblas", "trsv")


def batch_core_form(context, variant, multi, cps, B, T):
    """The form nmgp_svc_batch_eval's prior block takes (csrc/nmgp_api.hip)"""
    if context != "rocblas" and (context == "trsv" or (multi and B * (1 + T) >= SUBST_MIN_COLUMNS)):
        return "batch_core/trsv"
    if not multi:
        return "batch_core/resident_" + ("same" if variant == "same" else "pair")
    return "batch_core/subjects_%s_%s" % ("loop" if cps > 1 else "strided", "same" if variant == "same" else "pair")


def branch_map():
    """{(table, case tag, context, variant, entry): branch}: every entry the GPU half runs and the solve form it takes, as data.  The
    GPU half looks the label of each parity row up here (branch_of) and runs nothing that has no key; the CPU half asserts that the
    values cover INVENTORY."""
    out = {}
    for variant in VARIANTS:
        sp = "same" if variant == "same" else "pair"
        for N, M in TABLE_A:
            for context in ("default", "trsv"):
                tag = "N%d_M%d" % (N, M)
                out["A", tag, context, variant, "single"] = "svc_enqueue/trsv" if context == "trsv" else "svc_enqueue/trsm_" + sp
                for B in BATCHES_A:
                    out["A", tag, context, variant, "batch%d" % B] = batch_core_form(context, variant, False, 1, B, n_slots(M))
        for M, cps in TABLE_B:
            for context in CONTEXTS:
                out["B", "M%d_cps%d" % (M, cps), context, variant, "set"] = batch_core_form(context, variant, True, cps, SUBJECTS * cps,
                                                                                           n_slots(M))
        for N, M in TABLE_C:
            for context in ("default", "trsv"):
                for entry in ("single", "batch%d" % BATCH_C):
                    out["C", "N%d_M%d" % (N, M), context, variant, entry] = "prior_solve/" + ("trsv" if context == "trsv" else "trsm")
        for N, M in SUBJECT_CASES_C:
            for context in ("default", "rocblas"):
                out["C", "subjects_N%d_M%d" % (N, M), context, variant, "set"] = \
                    "sep_subjects/" + ("trsv" if context == "default" else "trsm_" + sp)
        for N, M, layout in TABLE_D:
            for context in ("default", "rocblas"):
                for entry in ("had_batch_eval", "hads_batch_eval"):
                    out["D", "N%d_M%d_%s" % (N, M, layout), context, variant, entry] = \
                        "had_prior_solve/" + ("trsv" if context == "default" else "trsm_" + sp)
        for cps in COHORT_CPS:
            out["E", "cps%d" % cps, "default", variant, "cohort"] = "cohort/trsv"
        out["E", "cps%d" % COHORT_SPLIT_CPS, "default", variant, "cohort"] = "cohort/trsv_chunked"
        for N, M in TABLE_P:
            for context in ("default", "rocblas"):
                kind = "trsv" if context == "default" else "trsm"
                out["P", "N%d_M%d" % (N, M), context, variant, "predict_svc"] = "gp_project/" + kind
                for entry in ("predsample_svc", "predsample_sep", "predsample_had", "predsample_hads", "predict_had", "predict_hads"):
                    out["P", "N%d_M%d" % (N, M), context, variant, entry] = "project_rows/" + kind
    return out


_BRANCH_MAP = branch_map()


def branch_of(table, tag, context, variant, entry):
    """The label of a parity row: the map's, never the caller's (KeyError: the GPU half runs an entry the map does not hold)"""
    return _BRANCH_MAP[table, tag, context, variant, entry]


def cohort_chunks(nsub, cps, Nmax, M, cap_gb, want_grad=True):
    """[(first subject, chains)] of the chunks nmgp_had_subjects_eval makes of nsub x cps chains under an NMGP_HAD_BATCH_SLAB_GB of
    cap_gb (floored at 1): had_layout<CohNon> of one chain, every piece rounded up to an even count of doubles, then the chunk rule
    (had_for_chunks, csrc/nmgp_hadamard_common.h)."""
    T, N = n_slots(M), Nmax
    P = N * (1 + T) + 1
    ld = ((2 * N + 2 if want_grad else N + 1) + 15) // 16 * 16
    pieces = [P, N, 16, 1, N, N * M, N * (1 + T), 1 + T] + ([N * (1 + T)] if want_grad else []) + [ld * N]
    if want_grad:
        pieces += [N, N * N, max(((N + 63) // 64) * N * (M + 1), N * ((N + 255) // 256)), P, 2]
    per_chain = 8 * sum((n + 1) // 2 * 2 for n in pieces)
    B = nsub * cps
    Bc = min(B, int(max(1.0, cap_gb) * 1e9 // per_chain), 65535)
    assert Bc >= 1
    split = cps > Bc
    if not split:
        Bc = Bc // cps * cps
    out, b0 = [], 0
    while b0 < B:
        s0 = b0 // cps
        nb = min(Bc, B - b0)
        if split:
            nb = min(nb, (s0 + 1) * cps - b0)
        out.append((s0, nb))
        b0 += nb
    return out
