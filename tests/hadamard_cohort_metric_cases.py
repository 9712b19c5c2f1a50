"""Sets, references, measure and recorded figures of the prior-factor metric of the Hadamard cohort (tests/test_hadamard_cohort_metric_cpu.py,
tests/test_gpu_hadamard_cohort_metric.py: nmgp_had_subjects_prior_apply, nmgp_had_subjects_traj_* under mass kind 2, the cohort HMC
drivers with mass="prior").  A plain module, not a conftest; the method is tests/metric_cases.py's (imported as mc):

* the well-conditioned family HYPER_A / HYPER_B there, subject s on linspace(0, 1 + 0.1 s, N_s): kappa <= KAPPA_MAX and factor tiles
  that are populated far from the diagonal (asserted in the CPU half), so that a tiling or masking error cannot hide;
* np.longdouble references: the covariance from (x_i - x_j)^2 directly, a column Cholesky, plain products;
* errors per block, relative to the block (mc.block_table on a subject's rows in the reference layout); trajectories on the
  displacement q1 - q0;
* the GPU bar is 50 x the worst error of the float64 NumPy restatement (the drivers' host loop) against those references, never
  above 1e-10.

The ragged sets sit at the kernel's edges (64-row tiles, TRMM_CG = 8 column groups); every subject holds every label.  The arrays are
shared: do not write into them."""
import functools

import numpy as np

import hadamard_cases as hc
import hadamard_cohort_hmc_cases as hh
import metric_cases as mc

LD = mc.LD
MODELS = ("non", "sep")
LAYOUT = {"non": "svc", "sep": "sep"}
# name -> (M, sizes).  P: one partial tile with N_s = M, both sides of 64 and 128.  Q: T = 36, five column groups, the last of 4.
# R: T = 1, four tiles.  E: no padding.
SETS = {"P": (2, (2, 63, 64, 65, 129)), "Q": (8, (8, 40, 130)), "R": (1, (1, 64, 193)), "E": (3, (65, 65))}
WIDE = 37                                       # one run of P with Nmax + 37
HYPER = {"non": mc.HV_SVC, "sep": np.array([0.0, mc.HYPER_A[0], mc.HYPER_A[1], 0.0, mc.HYPER_B[0], mc.HYPER_B[1], 1.0, 1.0, mc.SEP_C[1]])}
# the cohort cases' own golden hyper-parameters (alpha ~ 1, beta = 0.03 .. 0.05: kappa up to ~1e8 on these grids)
HYPER_ILL = {"non": hc.hypers()["had"], "sep": hc.hypers()["sep"]}
EPS0 = 0.05                                     # whitened step of subject s: EPS0 / (1 + s)
MEANING_EPS0 = 0.5                              # ... of the meaning test: |H1 - H0| of O(1), so that its relative error means something
P_SEED = 4300

# Worst block error of the float64 restatement (drivers._HadamardCohortHMC._prior_factor / _metric_apply / _host_traj) against
# np.longdouble, measured by tests/test_hadamard_cohort_metric_cpu.py, which prints the figures and asserts that none exceeds its entry
# (x86-64, 80-bit long double).  Measured: both products 5.5e-14 (set P, N_s = 129, slot column uL[1,0], not transposed); one and two
# steps 5.5e-14 (the same block: the displacement is dominated by eps L_blk z with the same z); meaning (the whitened host loop against
# the dense-mass leapfrog in longdouble, set P, two steps at MEANING_EPS0) 5.5e-14 on q1 - q0 and 1.6e-13 on H1 - H0 (|H1 - H0| between
# 0.15 and 25).  The entries are these with half as much again for another BLAS's rounding.  ONE_ULP_SENSITIVITY: what moving every
# real entry of the two-step middle point by one unit in the last place does to the restatement in the same measure (measured:
# 9.7e-16 nonseparable, 9.1e-15 separable) -- the two-step bar is the one-step entry plus this.
RESTATEMENT_WORST = {"apply": 8.5e-14, "traj": 8.5e-14, "meaning_q": 8.5e-14, "meaning_H": 2.5e-13}
ONE_ULP_SENSITIVITY = 1.5e-14
RESTATEMENT_WORST["traj2"] = RESTATEMENT_WORST["traj"] + ONE_ULP_SENSITIVITY
BAR = {k: min(50.0 * v, mc.BAR_CAP) for k, v in RESTATEMENT_WORST.items()}

# Test 7 (the metric does its job): set P under HYPER_ILL, chains started at a draw from the prior (prior_draw_chains), 10 leapfrog
# steps of ONE numeric step size for every subject.  Found on the CPU half with the host loop on the restatement (scanned: 0.002 ..
# 0.2): at 0.01 every chain has |dH| < 0.1 under mass="prior" (both models), and under the identity mass at the same step size every
# chain of the subjects with N_s >= 63 FAILS (at 0.002 their |dH| is 1.6e3 .. 2.2e4).  JOB_DIAGONAL: the subject with N_s = M = 2 sits
# on x = {0, 1}, 20 length scales apart: its prior covariances are alpha^2 I to 1e-87, L_blk is diagonal, the metric is the identity
# mass up to one scale per block, and NO step size separates the two masses there (identity |dH| 5e-6 at 0.01, 4e-2 at 0.2, as under
# the metric).  The second statement therefore cannot hold for its chains; they are held to |dH| < 1 under BOTH masses instead.
JOB_DIAGONAL = 0
JOB_EPS, JOB_STEPS = 0.01, 10
JOB_DH_PRIOR, JOB_DH_IDENTITY = 1.0, 10.0
# Test 6 (drivers): every accept test of this seed's host-loop runs on the restatement is further than 1e-6 from its threshold
DRIVER_SEED = 6100
DRIVER_EPS = 0.15
DECISION_MARGIN = 1e-6


def _ro(a):
    a.setflags(write=False)
    return a


def sizes(name):
    return list(SETS[name][1])


def n_labels(name):
    return SETS[name][0]


@functools.lru_cache(maxsize=None)
def subject(name, s, ill=False):
    """Subject s of a set as tests/hadamard_cases.py builds one: x = linspace(0, 1 + 0.1 s, N_s), labels i mod M, y = sin(6 x + label)
    + noise, two chains per model at the scale of the well-conditioned priors (q ~ 1e-3: the potential stays O(1e3), so H1 - H0 is
    resolved), and the hyper-parameters by model name."""
    M, sz = SETS[name]
    N, T = sz[s], M * (M + 1) // 2
    x = mc.grid(N, s)
    rng = np.random.default_rng(8800 + 1000 * M + 10 * N + s)
    indx = (np.arange(N) % M).astype(np.int32)
    Lm = np.eye(M) + np.tril(0.3 * rng.standard_normal((M, M)))
    L_vec = Lm[np.tril_indices(M)]
    y = np.sin(6.0 * x + indx) + 0.1 * rng.standard_normal(N)
    had, sep = [], []
    for b in range(2):
        tl = 1e-3 * (b + 1) * np.sin(5.0 * x + 0.4 * b)
        ts = 1e-3 * (b + 1) * np.cos(4.0 * x + 0.3 * b)
        Lvs = 2e-3 * L_vec[None, :] * (1.0 + 0.1 * np.sin(3.0 * x + 0.7 * b))[:, None]
        had.append(np.concatenate([tl, Lvs.reshape(-1), [-2.0 + 0.01 * b]]))
        sep.append(np.concatenate([tl, ts, L_vec * (1.0 + 0.05 * b), [-2.0 + 0.01 * b]]))
    hyp = HYPER_ILL if ill else HYPER
    return dict(N=N, M=M, T=T, x=_ro(x), indx=_ro(indx), y=_ro(y), pars={"had": _ro(np.stack(had)), "sep": _ro(np.stack(sep))},
                hyper={"had": hyp["non"], "sep": hyp["sep"]})


def subjects(name, ill=False):
    return [subject(name, s, ill) for s in range(len(SETS[name][1]))]


def set_subjects(ctx, name, Nmax=None, only=None):
    subs = subjects(name)
    if only is not None:
        subs = [subs[only]]
    ctx.had_set_subjects([c["x"] for c in subs], [c["indx"] for c in subs], [c["y"] for c in subs], M=n_labels(name), Nmax=Nmax)


def chains(model, name, k):
    return [c["pars"][hh.PARS[model]][:k] for c in subjects(name)]


def eps_of(name, eps0=EPS0):
    return eps0 / (1.0 + np.arange(len(SETS[name][1])))


@functools.lru_cache(maxsize=None)
def _normals(model, name, s, j, seed):
    P = mc.n_pars(LAYOUT[model], SETS[name][1][s], SETS[name][0])
    return _ro(np.random.default_rng(seed + 131 * s + 17 * j + (0 if model == "non" else 50000)).standard_normal(P))


def vectors(model, name, k, seed=P_SEED):
    """per subject [k, P_s] standard normals, a stream per (subject, chain): row 0 of k = 2 is the row of k = 1"""
    return [np.stack([_normals(model, name, s, j, seed) for j in range(k)]) for s in range(len(SETS[name][1]))]


def pack(model, name, rows, Nmax=None, fill=0.0, only=None):
    sz = sizes(name) if only is None else [sizes(name)[only]]
    return hh.pack(model, rows, sz, n_labels(name), Nmax=Nmax, fill=fill)


def unpack(model, name, P, k, only=None):
    sz = sizes(name) if only is None else [sizes(name)[only]]
    return hh.unpack(model, P, sz, n_labels(name), k)


def pads(model, name, k, Nmax=None):
    sz = sizes(name)
    return hh.padded_slots(model, sz, n_labels(name), max(sz) if Nmax is None else Nmax, k)


# ---- factors and products ------------------------------------------------------------------------------------------------------------
def factors(model, name, s, prec="ld", ill=False):
    """(L0, L1) of subject s: the factors of hyper[1..2] and hyper[4..5] on the subject's grid (mc.factor: longdouble or float64)"""
    h = (HYPER_ILL if ill else HYPER)[model]
    N = SETS[name][1][s]
    return (mc.factor("A", N, s, prec, hyper=(float(h[1]), float(h[2]))), mc.factor("B", N, s, prec, hyper=(float(h[4]), float(h[5]))))


def apply_rows(model, name, s, v, trans, prec="ld", ill=False):
    """L_blk,s v (or its transpose) for the rows v [k, P_s] of subject s in the reference layout, in the precision of the factors"""
    L0, L1 = factors(model, name, s, prec, ill)
    if model == "non":
        return mc.apply_svc(L0, L1, v, trans)
    return mc.apply_sep(L0, L1, float((HYPER_ILL if ill else HYPER)["sep"][8]), v, trans)


def layout_of(model, name, s):
    return (LAYOUT[model], SETS[name][1][s], SETS[name][0])


def worst_block(model, name, got, ref):
    """(worst block error, "subject s row b: block") of per-subject lists of rows in the reference layout"""
    worst, where = 0.0, ""
    for s, (g, r) in enumerate(zip(got, ref)):
        e, w = mc.block_errors(g, r, layout_of(model, name, s))
        if e >= worst:
            worst, where = e, "subject %d (N_s = %d) %s" % (s, SETS[name][1][s], w)
    return worst, where


# ---- the leapfrog step under the metric, in longdouble ---------------------------------------------------------------------------------
def leapfrog_ld(model, name, s, q0, z, eps, nsteps, g0, grad_at, ill=False):
    """The whitened trajectory of subject s's rows [k, P_s] in longdouble: u = z; u -= c eps L^T g; q += eps L u; gradients are INPUTS
    (g0 at q0, grad_at(step, q) at the step-th evaluated point).  Returns (points [q0, q_1, ..], u1)."""
    q, u, g, eps = np.asarray(q0, dtype=LD), np.asarray(z, dtype=LD), np.asarray(g0, dtype=LD), LD(eps)
    points = [q]
    for step in range(1, nsteps + 1):
        u = u - (eps / 2 if step == 1 else eps) * apply_rows(model, name, s, g, True, "ld", ill)
        q = q + eps * apply_rows(model, name, s, u, False, "ld", ill)
        points.append(q)
        g = np.asarray(grad_at(step, q), dtype=LD)
    u = u - (eps / 2) * apply_rows(model, name, s, g, True, "ld", ill)
    return points, u


def leapfrog_dense_ld(model, name, s, q0, z, eps, nsteps, g0, grad_at):
    """The same trajectory written as a DENSE-mass leapfrog in longdouble: M^-1 = L_blk L_blk^T, p0 = L_blk^-T z, kick p -= c eps g,
    drift q += eps M^-1 p, K = 1/2 p^T M^-1 p.  Returns (points, K0, K1)."""
    P = np.asarray(q0).shape[1]
    Lb = apply_rows(model, name, s, np.eye(P, dtype=LD), False).T            # columns of L_blk: L_blk itself
    Minv = Lb @ Lb.T
    p = np.stack([solve_upper(Lb.T, np.asarray(r, dtype=LD)) for r in z])     # L_blk^T p = z
    q, g, eps = np.asarray(q0, dtype=LD), np.asarray(g0, dtype=LD), LD(eps)
    K0 = np.sum(p * (p @ Minv.T), axis=1) / 2
    points = [q]
    for step in range(1, nsteps + 1):
        p = p - (eps / 2 if step == 1 else eps) * g
        q = q + eps * (p @ Minv.T)
        points.append(q)
        g = np.asarray(grad_at(step, q), dtype=LD)
    p = p - (eps / 2) * g
    return points, K0, np.sum(p * (p @ Minv.T), axis=1) / 2


def solve_upper(U, b):
    """back substitution in the precision of U"""
    n = U.shape[0]
    x = np.zeros_like(b)
    for i in range(n - 1, -1, -1):
        x[i] = (b[i] - U[i, i + 1:] @ x[i + 1:]) / U[i, i]
    return x


# ---- the restatement as an evaluator (what ``evaluators=`` of the cohort drivers takes) ---------------------------------------------------
def reference_evaluator(model, name, k, ill=False, idx=None):
    """padded rows -> (out, grad, status) from the NumPy restatement of the model on each subject alone; idx: the subjects of the
    rows, in their order (a bucket of the drivers; default: the whole set in the caller's order)"""
    idx = list(range(len(SETS[name][1]))) if idx is None else list(idx)
    subs, sz, M = [subject(name, s, ill) for s in idx], [SETS[name][1][s] for s in idx], n_labels(name)

    def evaluate(P):
        outs, grads, status = [], [], []
        for c, rows in zip(subs, hh.unpack(model, P, sz, M, k)):
            gs = []
            for r in rows:
                try:                                # a chain that left the domain: a status, as the device entries report it
                    with np.errstate(all="ignore"):
                        o, g = hc.ref_logpos(hh.PARS[model], np.array(r), c, True, grad=True)
                    o, g = np.asarray(o, dtype=np.float64), np.asarray(g, dtype=np.float64)
                    ok = bool(np.isfinite(o[0]) and np.all(np.isfinite(g)))
                except (ValueError, OverflowError, np.linalg.LinAlgError, FloatingPointError):
                    ok = False
                if not ok:
                    o, g = np.full(hh.WIDTH[model], np.nan), np.zeros(r.shape[0])
                outs.append(o)
                gs.append(g)
                status.append(0 if ok else -1)
            grads.append(np.stack(gs))
        return np.stack(outs), hh.pack(model, grads, sz, M, Nmax=hh.nmax_of(model, P.shape[1], M)), np.array(status, dtype=np.int32)

    return evaluate


def subject_grad(model, name, s, ill=False):
    """rows [k, P_s] -> (U [k], grad [k, P_s]) of the restatement on subject s"""
    c = subject(name, s, ill)

    def grad(q):
        res = [hc.ref_logpos(hh.PARS[model], np.array(r, dtype=np.float64), c, True, grad=True) for r in np.asarray(q, dtype=np.float64)]
        return np.array([float(r[0][0]) for r in res]), np.stack([np.asarray(r[1], dtype=np.float64) for r in res])

    return grad


def hyper_dict(model, ill=False):
    from nonstationary_multivariate_gaussian_process_amd import drivers
    keys = {"non": drivers.SVC_HYPER_KEYS, "sep": drivers.SEP_HYPER_KEYS}[model]
    return dict(zip(keys, (HYPER_ILL if ill else HYPER)[model]))


def triples(name):
    return [(c["x"], c["indx"], c["y"]) for c in subjects(name)]


@functools.lru_cache(maxsize=None)
def prior_draw_chains(model, name, k):
    """per subject [k, P_s]: a draw from the GP priors of HYPER_ILL (mu + L_blk,s z with the float64 factors), the last slot at -2"""
    out = []
    h = HYPER_ILL[model]
    for s in range(len(SETS[name][1])):
        z = vectors(model, name, k, seed=7700)[s]
        q = np.asarray(apply_rows(model, name, s, z, False, "f64", ill=True), dtype=np.float64)
        N = SETS[name][1][s]
        q[:, :N] += h[0]
        q[:, N:(2 * N if model == "sep" else -1)] += h[3]
        q[:, -1] = -2.0
        out.append(_ro(q))
    return out
