"""Cases, chains, references and restatements of the eigen-formulation objective sweep (tests/test_eig_objective_cpu.py,
tests/test_gpu_eig_objective.py).  A plain module, not a conftest: both halves import it, so the CPU half checks the very subjects,
chains and reference values the GPU half runs against.  Subjects, chains and the block measure are those of objective_cases
(separable) and sta_batch_cases (stationary); no GPU result enters a reference or a bar.

NMGP_SEP=eig evaluates the separable and stationary likelihoods in the joint eigenbasis of B and K_x (nmgp_eig.hip: kron_loglik,
kron_adjoint): rocsolver_dsyevd, k_kron_mv on the N x N eigenvector matrix, k_eig_reduce, k_colscale_d, two dgemm, k_sep_adjoint,
k_sep_grad_sum, k_sep_coreB and the host rotation of coreB.  The shapes put every ragged edge of those kernels under the objective.

References.  A case that objective_cases / sta_batch_cases already holds: its float64 CPU oracle.  A new shape or a degenerate
chain: the dense restatement sep_restated of tests/test_objective_sweep_cpu.py (B kron K_x + sigma2 I, Cholesky column by column), in
np.longdouble while N M <= 1000 and in float64 above; for the stationary layout the same restatement on the parameter vector
expanded to constant curves, the two N-blocks summed.  With the priors on, the prior part of such a reference is the oracle's own
difference g(prior) - g(no prior)."""
import numpy as np

import objective_cases as OC
import sta_batch_cases as SC
from nonstationary_multivariate_gaussian_process_amd import sim

LIK_TIGHT, GRAD_TIGHT = OC.LIK_TIGHT, OC.GRAD_TIGHT
RESTATED_LIK, RESTATED_BLOCK = LIK_TIGHT / 10, GRAD_TIGHT / 10     # what the CPU half holds eig_restated to
RETRY_TOL = 1e-6                        # the standing bar of the singular-covariance retry (tests/test_gpu_parity.py)
RETRY_RESTATED = 1e-7                   # ... and what the CPU half holds the restatement's attempt 1 to
JITTER = 1e-6                           # on K_x's diagonal, always (oracle.JITTER)
PRECISION = 1e-6                        # attempt * PRECISION on both diagonals in the retry loop (nmgp_eig.hip)
LONGDOUBLE_MAX_NM = 1000

# Separable (N, M), chains 0 .. 2 of objective_cases.chain("sep", ...).  objective_cases.SEP_CASES, and
#   (2, 2)                     the smallest matrix with both N and M above 1
#   (63, 4) (64, 6) (66, 7)    one 64-tile of k_sep_adjoint less a row, exactly, plus two rows; completes M = 1 .. 8
#   (257, 8) (in SEP_CASES)    the first ragged 256-block of k_colscale_d / k_sep_grad_sum, the stride loop of k_sep_coreB, M N = 2056:
#                              two passes of k_eig_reduce's 1024 threads, N = 4 * 64 + 1: one live wave in the last k_kron_mv workgroup
#   (390, 2)                   the first even N at which only lanes 0 .. 2 take k_kron_mv<true>'s four-segment loop (c + 192 < N / 2) and
#                              the others only the tail; N mod 4 = 2
#   (514, 1)                   lane 0 takes one unrolled pass and then the tail; M = 1 beyond 256
SEP_NEW = [(2, 2), (63, 4), (64, 6), (66, 7), (390, 2), (514, 1)]
SEP_SHAPES = list(OC.SEP_CASES) + SEP_NEW
SEP_CHAINS = 3
# Stationary: sta_batch_cases.SHAPES as they are (M = 1 .. 8; 63 / 64 / 65, 127 / 128 / 129, 257), four chains each
STA_SHAPES = list(SC.SHAPES)
STA_CHAINS = SC.B_CHAINS
# Degenerate B on chain 0 of these shapes, in both layouts:
#   identity   uL_vec = 0: B = I, every eigenvalue equal, the host Jacobi stops on its first sweep
#   graded     diagonal slots linspace(-6, 1, M), off-diagonal slots 0.3: eigenvalues from 1.7e-12 to 8 at M = 7
DEGENERATE_SHAPES = [(65, 3), (66, 7)]
DEGENERATE_KINDS = ("identity", "graded")
SINGULAR_SEP, SINGULAR_STA = (96, 3), (65, 3)
BATCH = 3
MUTATION_MIN_N, MUTATION_MIN_M = 63, 2

HYPER_SEP_VEC, HYPER_STA_VEC = OC.HYPER_SEP_VEC, SC.HYPER_VEC

# (model, N, M, block name) -> bar, for a block on which the CPU half measures eig_restated itself above RESTATED_BLOCK against the
# dense restatement: ten times that measured discrepancy (the rule of objective_cases.BLOCK_BARS).  Measured values: see the
# docstring of tests/test_eig_objective_cpu.py.
#   stationary (128, 4), sigma2: on chain 1 (sigma2 = 0.0104, the entry -0.059 of a gradient of norm 8.6: 1/2 (sum At^2 - sum w) is a
#   small difference of large sums) eig_restated is 1.38e-8 from np.longdouble under numpy's eigh and scipy's evd, 1.37e-8 under ev,
#   5.3e-9 under evr, and the CPU oracle -- this case's reference -- is 5.3e-9 from it.  Ten times 1.38e-8, rounded up.
#   stationary (128, 4), tilde_l: on the same chain the N per-location entries cancel 3.4e4-fold in the scalar; the oracle is 1.37e-9
#   from np.longdouble (eig_restated 5.1e-10 to 8.6e-10 under the four drivers).  Ten times 1.37e-9, rounded up.
#   stationary (257, 7), sigma2: against the float64 dense restatement (N M = 1799, itself no better: the CPU oracle is 2.0e-9 from it)
#   eig_restated is 7.4e-10, 1.24e-9, 1.39e-9 and 7.4e-10 on chain 0 with 8, 1, 4 and 16 BLAS threads.  Ten times 1.39e-9, rounded up.
BLOCK_BARS = {("sta", 128, 4, "sigma2"): 2e-7, ("sta", 128, 4, "tilde_l"): 2e-8, ("sta", 257, 7, "sigma2"): 2e-8}

case_id = OC.case_id
n_slots = OC.n_slots


def shapes(model):
    return SEP_SHAPES if model == "sep" else STA_SHAPES


def n_chains(model):
    return SEP_CHAINS if model == "sep" else STA_CHAINS


def hyper_vec(model):
    return HYPER_SEP_VEC if model == "sep" else HYPER_STA_VEC


def all_cases():
    """[(model, N, M)] of the sweep, the separable shapes first."""
    return [("sep", N, M) for N, M in SEP_SHAPES] + [("sta", N, M) for N, M in STA_SHAPES]


def subject(model, N, M):
    """(x [N], Y [N, M]), read-only."""
    return (OC.subject("sep", N, M) if model == "sep" else SC.subject(N, M))[:2]


def degenerate_uL(kind, M):
    r, c = np.tril_indices(M)
    if kind == "identity":
        return np.zeros(r.shape[0])
    assert kind == "graded", kind
    return np.where(r == c, np.linspace(-6.0, 1.0, M)[r], 0.3)


def chain(model, N, M, k):
    """Chain k (an index, or one of DEGENERATE_KINDS: chain 0 with the degenerate uL_vec) in the model's own layout; read-only."""
    T = n_slots(M)
    base = OC.chain("sep", N, M, 0 if isinstance(k, str) else k) if model == "sep" else SC.chains(N, M)[0 if isinstance(k, str) else k]
    if not isinstance(k, str):
        return base
    p = np.array(base, dtype=np.float64, copy=True)
    off = 2 * N if model == "sep" else 2
    p[off:off + T] = degenerate_uL(k, M)
    p.setflags(write=False)
    return p


def chains(model, N, M, B=None):
    return np.stack([chain(model, N, M, k) for k in range(n_chains(model) if B is None else B)])


def sta_to_sep(p, N):
    """The stationary vector [tilde_l, tilde_sigma, uL_vec T, sigma2] expanded to the separable layout with constant curves."""
    p = np.asarray(p)
    return np.concatenate([np.full(N, p[0]), np.full(N, p[1]), p[2:]])


def sep_grad_to_sta(g, N):
    """The scalar curves move every location together: the two N-blocks summed."""
    g = np.asarray(g)
    return np.concatenate([[g[:N].sum()], [g[N:2 * N].sum()], g[2 * N:]])


def blocks_over_bar(g, gref, layout):
    return OC.blocks_over_bar(g, gref, layout, GRAD_TIGHT, BLOCK_BARS)


# ---------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------
def dense_dtype(N, M):
    return np.longdouble if N * M <= LONGDOUBLE_MAX_NM else np.float64


_DENSE = {}


def dense(model, N, M, k):
    """(loglik, d(-loglik)/d pars) of the dense restatement for chain k in the model's layout, float64 arrays; computed once."""
    key = "%s,%d,%d,%s" % (model, N, M, k)
    if key not in _DENSE:
        from test_objective_sweep_cpu import sep_restated
        x, Y = subject(model, N, M)
        p = chain(model, N, M, k)
        ll, g = sep_restated(p if model == "sep" else sta_to_sep(p, N), Y, x, dense_dtype(N, M))
        g = np.asarray(g if model == "sep" else sep_grad_to_sta(g, N), dtype=np.float64)
        g.setflags(write=False)
        _DENSE[key] = (float(ll), g)
    return _DENSE[key]


def _oracle_call(model, N, M, k, prior):
    from oracle import nmgp_oracle as O
    x, Y = subject(model, N, M)
    if model == "sep":
        r, g = O.nlogpos_obj(chain(model, N, M, k), Y, x, **sim.HYPER_SEP, verbose=True, Prior=bool(prior), grad=True)
        return np.asarray(r, dtype=np.float64), np.asarray(g, dtype=np.float64)
    # (the reference raises for verbose=True with Prior=False: the likelihood-only call returns NegLog alone)
    r, g = O.nlogpos_obj_S(chain(model, N, M, k), Y, x, **SC.HYPER, verbose=bool(prior), Prior=bool(prior), grad=True)
    r = np.asarray(r, dtype=np.float64).reshape(-1)
    return (r if prior else np.array([r[0], -r[0]])), np.asarray(g, dtype=np.float64)


_REF = {}


def has_oracle_case(model, N, M, k):
    return not isinstance(k, str) and (N, M) in (OC.SEP_CASES if model == "sep" else SC.SHAPES)


def ref(model, N, M, k, prior):
    """(out, grad) the device is held to for chain k, read-only: out[0] NegLog, out[1] loglik, out[2:] the verbose components (with
    the priors on only).  See the module docstring for which reference a case has."""
    key = "%s,%d,%d,%s,%d" % (model, N, M, k, bool(prior))
    if key not in _REF:
        if has_oracle_case(model, N, M, k):
            if model == "sep":
                r, g = OC.oracle("sep", N, M, k, prior)
            else:
                o, gs = SC.oracle(N, M, bool(prior))
                r, g = (o[k] if prior else np.array([o[k][0], -o[k][0]])), gs[k]
        else:
            ll, g0 = dense(model, N, M, k)
            if prior:
                (r, g1), (_, go0) = _oracle_call(model, N, M, k, True), _oracle_call(model, N, M, k, False)
                g = g0 + (g1 - go0)
            else:
                r, g = np.array([-ll, ll]), g0
        r, g = np.array(r, dtype=np.float64), np.array(g, dtype=np.float64)
        r.setflags(write=False)
        g.setflags(write=False)
        _REF[key] = (r, g)
    return _REF[key]


def refs(model, N, M, ks):
    """[{prior: (out, grad)}] for the chains ks: the `refs` of hold_to_oracle."""
    return [{p: ref(model, N, M, k, p) for p in (False, True)} for k in ks]


def save_refs(path):
    """The references computed so far, for a child process that runs the same cases (load_refs)."""
    arrays = {}
    for key, (r, g) in _REF.items():
        arrays["out:" + key], arrays["grad:" + key] = r, g
    np.savez(path, **arrays)


def load_refs(path):
    d = np.load(path)
    for name in d.files:
        if name.startswith("out:"):
            r, g = d[name], d["grad:" + name[4:]]
            r.setflags(write=False)
            g.setflags(write=False)
            _REF.setdefault(name[4:], (r, g))


# ---------------------------------------------------------------------------------------------------
# the singular chains of the retry
# ---------------------------------------------------------------------------------------------------
def singular(model):
    """(x, Y, good chains [BATCH, P], singular chain [P]).  Separable: the subject and chain of
    test_separable_and_stationary_objectives_recover_from_a_singular_covariance (row and column 1 of B exactly zero, sigma2 =
    exp(-800) = 0).  Stationary: sta_batch_cases.singular_chain on chain 1 of (65, 3)."""
    if model == "sep":
        N, M = SINGULAR_SEP
        d = sim.simulate_separable(N, M, 3)
        good = np.stack([sim.perturb(d["pars_true"], 0.05, 0.3 + 0.4 * k) for k in range(BATCH)])
        p = d["pars_true"].copy()
        p[2 * N + 1], p[2 * N + 2], p[2 * N + 4] = 0.0, -800.0, 0.0
        p[-1] = -800.0
        return np.ascontiguousarray(d["x"]), np.ascontiguousarray(d["Y"]), good, p
    N, M = SINGULAR_STA
    x, Y, _ = SC.subject(N, M)
    good = np.array(SC.chains(N, M)[:BATCH])
    return x, Y, good, SC.singular_chain(good[1])


_SINGULAR_REF = {}


def singular_ref(model, attempt=1):
    """The np.longdouble dense likelihood of the covariance that attempt `attempt` of the retry loop evaluates:
    (B + attempt 1e-6 I) kron (K_x + attempt 1e-6 I) + sigma2 I."""
    if (model, attempt) not in _SINGULAR_REF:
        from test_objective_sweep_cpu import _dense_parts, _gibbs_parts, _tril_stack
        x, Y, _, p = singular(model)
        N, M = Y.shape
        p = (p if model == "sep" else sta_to_sep(p, N)).astype(np.longdouble)
        ld = np.longdouble
        sig = np.exp(p[N:2 * N])
        K0, _ = _gibbs_parts(np.asarray(x).astype(ld), p[:N])
        Kx = sig[:, None] * sig[None, :] * K0 + (ld(JITTER) + attempt * ld(PRECISION)) * np.eye(N, dtype=ld)
        L, _, _ = _tril_stack(p[2 * N:2 * N + n_slots(M)], M)
        Bm = L @ L.T + attempt * ld(PRECISION) * np.eye(M, dtype=ld)
        S = np.empty((M * N, M * N), dtype=ld)
        for m in range(M):
            for k in range(M):
                S[m * N:(m + 1) * N, k * N:(k + 1) * N] = Bm[m, k] * Kx
        S[np.diag_indices(M * N)] += np.exp(p[-1])
        _SINGULAR_REF[(model, attempt)] = float(_dense_parts(S, np.asarray(Y).astype(ld).T.reshape(-1))[0])
    return _SINGULAR_REF[(model, attempt)]


# ---------------------------------------------------------------------------------------------------
# the device's eigen arithmetic, restated in float64 NumPy
# ---------------------------------------------------------------------------------------------------
MUTATIONS = {                                   # name -> the block(s) the measure must name
    "dsigma2_without_sum_w": ("sigma2",),           # the trace term of d sigma2 dropped (k_eig_reduce's out[3])
    "coreB_without_diagonal": ("uL_vec",),          # k_sep_coreB's p == p' correction dropped
    "d_over_first_M-1": ("tilde_sigma", "tilde_l"),  # k_colscale_d's sum stops one eigenvalue of B early (the p < M class)
    "last_location_tilde_sigma_zero": ("tilde_sigma",),      # a ragged tile of k_sep_adjoint
    "tilde_l_x1.02": ("tilde_l",),
}


def eig_restated(pars, Y, x, attempt=0, mutation=None, eigh=np.linalg.eigh):
    """(loglik, d(-loglik)/d pars) of the separable model as kron_loglik / kron_adjoint form them, in float64: the eigenpairs of B and
    of K_x + 1e-6 I from `eigh`, everything else from them.  attempt: the retry loop's jitter, attempt * 1e-6 on both diagonals.
    mutation: one of MUTATIONS, the arithmetic changed the way a wrong kernel would change it."""
    from test_objective_sweep_cpu import _gibbs_parts, _tril_stack
    assert mutation is None or mutation in MUTATIONS, mutation
    N, M = Y.shape
    T = n_slots(M)
    pars, x = np.asarray(pars, dtype=np.float64), np.asarray(x, dtype=np.float64)
    s2 = np.exp(pars[-1])
    sig = np.exp(pars[N:2 * N])
    K0, dlogK = _gibbs_parts(x, pars[:N])
    Ks = sig[:, None] * sig[None, :] * K0
    Kx = Ks + JITTER * np.eye(N)
    L, r, c = _tril_stack(pars[2 * N:2 * N + T], M)
    Bm = L @ L.T
    if attempt:
        Kx[np.diag_indices(N)] += attempt * PRECISION
        Bm[np.diag_indices(M)] += attempt * PRECISION
    wB, VB = eigh(Bm)
    wK, VK = eigh(Kx)
    a = VB.T @ np.asarray(Y, dtype=np.float64).T @ VK       # [M, N]: (V_B^T kron V_K^T) y
    t = wB[:, None] * wK[None, :]
    w = 1.0 / (s2 + t)
    loglik = -0.5 * np.log(t + s2).sum() - 0.5 * (a * a * w).sum()
    At = a * w
    Md = M - 1 if (mutation == "d_over_first_M-1" and M > 1) else M
    d = (wB[:Md, None] * w[:Md]).sum(0)
    Cm = (VK * d[None, :]) @ VK.T
    U = VK @ At.T                                           # [N, M]
    dK = 0.5 * ((U * wB[None, :]) @ U.T - Cm)
    coreB = (At * wK[None, :]) @ At.T
    if mutation != "coreB_without_diagonal":
        coreB[np.diag_indices(M)] -= (wK[None, :] * w).sum(1)
    dB = 0.5 * (VB @ coreB @ VB.T)
    ds = 0.5 * ((At * At).sum() - (0.0 if mutation == "dsigma2_without_sum_w" else w.sum()))
    W = 2 * dK * Ks * dlogK
    np.fill_diagonal(W, 0)
    g_uL = (2 * dB @ L)[r, c]
    dg = r == c
    g_uL[dg] *= L[r[dg], c[dg]]
    g = -np.concatenate([W.sum(1), 2 * (dK * Ks).sum(1), g_uL, [s2 * ds]])
    if mutation == "last_location_tilde_sigma_zero":
        g[2 * N - 1] = 0.0
    if mutation == "tilde_l_x1.02":
        g[:N] *= 1.02
    return float(loglik), g


def eig_restated_case(model, N, M, k, **kw):
    """eig_restated on chain k of a case, in the model's layout (stationary: constant curves, the two N-blocks summed)."""
    x, Y = subject(model, N, M)
    p = chain(model, N, M, k)
    ll, g = eig_restated(p if model == "sep" else sta_to_sep(p, N), Y, x, **kw)
    return ll, (g if model == "sep" else sep_grad_to_sta(g, N))
