"""Subjects, chains, oracle values and the error measure of the complete-data objective sweep (tests/test_objective_sweep_cpu.py,
tests/test_gpu_objective_sweep.py).  A plain module, not a conftest: both halves import it, so the CPU half checks the very subjects,
chains and reference values the GPU half runs against.

Why a measure of its own: with the GP priors on, the gradient of either objective is almost entirely Sigma_prior^-1 (v - mu) (norm ~1e6
against ~1e2 for the likelihood part), so ||dg|| / ||g|| < 1e-5 over the whole vector lets a likelihood gradient pass whose sigma2 entry
or whose tilde_l block is wrong.  block_errors() takes the gradient block by block -- tilde_l, every stride-T slot column of uL, the
sigma2 entry -- and is applied to the gradient WITHOUT the priors; the prior part g(prior) - g(no prior) is compared on its own."""
import functools

import numpy as np

from conftest import SEP_KEYS, SVC_KEYS
from nonstationary_multivariate_gaussian_process_amd import sim

# (N, M) of the nonseparable sweep, around the 64-wide location tiles of k_svc_cov / k_svc_adjoint, the 256-wide blocks of
# k_tri_gemv_part and k_xtri_seed in n = N M and the 512-column panel; every M from 1 to 8:
#   (1, 1) (2, 2)        one location, one output; the smallest matrix with both
#   (63, 3) (64, 1) (64, 4)   one tile less one row, one tile exactly, n = 256 exactly
#   (66, 6) (65, 8)      a second tile of 2 / 1 rows, n = 396 and n = 520 > 512
#   (128, 2) (129, 2)    n = 256 from two tiles, n = 258: the 256-wide blocks' first ragged one
#   (129, 7) (193, 5)    n = 903 and 965: a ragged second panel, three and four location tiles
SVC_CASES = [(1, 1), (2, 2), (63, 3), (64, 1), (64, 4), (66, 6), (65, 8), (128, 2), (129, 2), (129, 7), (193, 5)]
# the separable sweep: the 128 x 32 tile edge of k_sep_blocks_b4 and the odd-N kernel
SEP_CASES = [(1, 1), (3, 2), (65, 3), (130, 5), (257, 8)]
SVC_BATCHES = (2, 5)                    # 5: the gradient path halves a panel wider than 256 (fused_base, nmgp_chol.hip)
SEP_BATCH = 3
SUBJECT_SET_CASES = [(65, 8), (129, 2)]  # S = 3 subjects x 2 chains; odd N: the row-pair tail of k_prior_trsv
SUBJECTS, CHAINS_PER_SUBJECT = 3, 2
SCHEDULE_CASE, SCHEDULE_B, SCHEDULE_CHAINS = (193, 3), 128, (0, 64, 127)    # 128 * 579 = 74,112 > 73,728: the throughput schedule
MUTATION_MIN_N = 63                     # the mutations must be rejected at every case with N >= 63

HYPER_SVC_VEC = np.array([sim.HYPER_SVC[k] for k in SVC_KEYS])
HYPER_SEP_VEC = np.array([sim.HYPER_SEP[k] for k in SEP_KEYS])

# Bars of the GPU half without the priors (LIK_TIGHT / GRAD_TIGHT of tests/test_gpu_hadamard_sweep.py, here per block); the CPU half
# holds the float64 oracle to a tenth of them against np.longdouble.
LIK_TIGHT = 1e-10
GRAD_TIGHT = 1e-8
ORACLE_LIK = LIK_TIGHT / 10
ORACLE_BLOCK = GRAD_TIGHT / 10
# (model, N, M, block name) -> bar, for a block on which the CPU half measures the float64 oracle itself above ORACLE_BLOCK against
# np.longdouble: ten times that measured discrepancy.  None was measured (worst oracle block: see test_objective_sweep_cpu.py).
BLOCK_BARS = {}


def case_id(case):
    return "N%d_M%d" % tuple(case)


def n_slots(M):
    return M * (M + 1) // 2


@functools.lru_cache(maxsize=None)
def subject(model, N, M, s=0):
    """(x [N], Y [N, M], generating parameters), read-only.  s > 0: the further subjects of a subject set."""
    gen = sim.simulate_nonseparable if model == "svc" else sim.simulate_separable
    d = gen(N, M, 10 * N + M + 1000 * s)
    x, Y, p = np.ascontiguousarray(d["x"]), np.ascontiguousarray(d["Y"]), d["pars_true"].copy()
    for a in (x, Y, p):
        a.setflags(write=False)
    return x, Y, p


@functools.lru_cache(maxsize=None)
def chain(model, N, M, k, s=0):
    """Chain k of the subject: a smooth perturbation of the generating parameters, one phase per chain; read-only."""
    p = sim.perturb(subject(model, N, M, s)[2], 0.05, 0.3 + 0.4 * k)
    p.setflags(write=False)
    return p


def chains(model, N, M, B, s=0):
    return np.stack([chain(model, N, M, k, s) for k in range(B)])


_ORACLE = {}


def oracle(model, N, M, k, prior, s=0):
    """(out [5] or [6], grad [P]) of the float64 CPU oracle for chain k, computed once and read-only.  out[0] is NegLog (= -loglik
    without the priors), out[1:] the verbose components, which the library reports whatever the prior flag."""
    key = "%s,%d,%d,%d,%d,%d" % (model, N, M, k, bool(prior), s)
    if key not in _ORACLE:
        from oracle import nmgp_oracle as O
        x, Y, _ = subject(model, N, M, s)
        if model == "svc":
            r, g = O.nlogpos_obj_SVC(chain(model, N, M, k, s), Y, x, **sim.HYPER_SVC, verbose=True, Prior=bool(prior), grad=True)
        else:
            r, g = O.nlogpos_obj(chain(model, N, M, k, s), Y, x, **sim.HYPER_SEP, verbose=True, Prior=bool(prior), grad=True)
        r, g = np.asarray(r, dtype=np.float64), np.asarray(g, dtype=np.float64)
        r.setflags(write=False)
        g.setflags(write=False)
        _ORACLE[key] = (r, g)
    return _ORACLE[key]


def save_oracle(path):
    """The oracle values computed so far, for a child process that runs the same cases (load_oracle)."""
    arrays = {}
    for key, (r, g) in _ORACLE.items():
        arrays["out:" + key], arrays["grad:" + key] = r, g
    np.savez(path, **arrays)


def load_oracle(path):
    d = np.load(path)
    for name in d.files:
        if name.startswith("out:"):
            r, g = d[name], d["grad:" + name[4:]]
            r.setflags(write=False)
            g.setflags(write=False)
            _ORACLE.setdefault(name[4:], (r, g))


# ---------------------------------------------------------------------------------------------------
# the block measure
# ---------------------------------------------------------------------------------------------------
def blocks(model, N, M):
    """[(name, index)] of the gradient's blocks.  Nonseparable [tilde_l N | uL N x T location-major | sigma2]: tilde_l, each of the T
    slot columns g[N + t : N + N T : T] (named by the slot's row and column in L), the sigma2 entry.  Separable
    [tilde_l N | tilde_sigma N | uL_vec T | sigma2]: the four of them.  Stationary ("sta") [tilde_l | tilde_sigma | uL_vec T | sigma2]:
    the same four, the two curves scalars (the eigen-formulation sweep, tests/eig_objective_cases.py)."""
    T = n_slots(M)
    if model == "sta":
        return [("tilde_l", slice(0, 1)), ("tilde_sigma", slice(1, 2)), ("uL_vec", slice(2, 2 + T)), ("sigma2", slice(2 + T, 3 + T))]
    if model == "svc":
        r, c = np.tril_indices(M)
        out = [("tilde_l", slice(0, N))]
        out += [("uL[%d,%d]" % (r[t], c[t]), slice(N + t, N + N * T, T)) for t in range(T)]
        return out + [("sigma2", slice(N + N * T, N + N * T + 1))]
    return [("tilde_l", slice(0, N)), ("tilde_sigma", slice(N, 2 * N)), ("uL_vec", slice(2 * N, 2 * N + T)),
            ("sigma2", slice(2 * N + T, 2 * N + T + 1))]


def block_table(g, gref, layout):
    """{block name: ||d_b|| / max(||gref_b||, 1e-3 ||gref||)}.  The floor is there because some blocks are structurally zero: at N = 1
    tilde_l has no likelihood gradient, and at N = 2, M = 2 one slot column has norm 1e-16."""
    model, N, M = layout
    g, gref = np.asarray(g, dtype=np.float64), np.asarray(gref, dtype=np.float64)
    assert g.shape == gref.shape == (blocks(model, N, M)[-1][1].stop,), (g.shape, gref.shape, layout)
    floor = 1e-3 * float(np.linalg.norm(gref))
    return {name: float(np.linalg.norm(g[sl] - gref[sl]) / max(float(np.linalg.norm(gref[sl])), floor, 1e-300))
            for name, sl in blocks(model, N, M)}


def block_errors(g, gref, layout):
    """(error of the worst block, its name): a failure names the slot."""
    tab = block_table(g, gref, layout)
    name = max(tab, key=lambda k: (np.inf if np.isnan(tab[k]) else tab[k]))
    return tab[name], name


def blocks_over_bar(g, gref, layout, bar=GRAD_TIGHT, bars=None):
    """[(block, error, bar)] of the blocks that miss their bar: `bar`, or the block's entry in BLOCK_BARS (`bars`: the table of
    another sweep)."""
    tab = block_table(g, gref, layout)
    bad = []
    for name, e in tab.items():
        b = (BLOCK_BARS if bars is None else bars).get(layout + (name,), bar)
        if not e < b:
            bad.append((name, e, b))
    return bad


# ---------------------------------------------------------------------------------------------------
# the four mutations of a nonseparable likelihood gradient that ||dg|| / ||g|| under the priors lets through
# ---------------------------------------------------------------------------------------------------
def _mut_sigma2(g, N, M):
    g[-1] = 0.0                                     # the whole trace term gone (k_trace_terms)


def _mut_tilde_l(g, N, M):
    g[:N] *= 1.02


def _mut_last_location(g, N, M):
    T = n_slots(M)
    g[N + (N - 1) * T:N + N * T] = 0.0              # a tile edge of k_svc_adjoint


def _mut_last_slot(g, N, M):
    T = n_slots(M)
    g[N + T - 1:N + N * T:T] = 0.0                  # a slot mix-up in k_svc_grad_final


MUTATIONS = {"sigma2_zero": _mut_sigma2, "tilde_l_x1.02": _mut_tilde_l, "last_location_zero": _mut_last_location,
             "last_slot_zero": _mut_last_slot}


def mutate(name, g, N, M):
    out = np.array(g, dtype=np.float64, copy=True)
    MUTATIONS[name](out, N, M)
    return out
