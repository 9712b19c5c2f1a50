"""Factors, references, measure, case tables and mutations of the prior-factor metric and leapfrog sweep (tests/test_metric_sweep_cpu.py,
tests/test_gpu_metric_sweep.py).  A plain module, not a conftest: both halves import it, so the CPU half checks the very factors, vectors
and restatements the GPU half runs against.

The family.  The metric's factors are the Cholesky factors of RBF(x; alpha, beta) + 1e-6 I.  With the scripts' hyper-parameters they have
kappa ~ 1e9 .. 1e11 and are themselves only defined to kappa eps; with beta about one grid spacing they are numerically banded and a tiling
error far from the diagonal is invisible.  A SMALL ALPHA ON A SMOOTH KERNEL, x = linspace(0, 1, N), gives K = 1e-6 (G + I) with G smooth:
kappa <= 200 (A) / 2000 (B) and factor tiles that are populated far from the diagonal (asserted in the CPU half).  A is the factor of
tilde_l, B that of the uL columns: a swap of L0 and L1, of their leading dimensions or strides cannot cancel.

The references are np.longdouble: the covariance from (x_i - x_j)^2 directly, a column Cholesky, plain products.  The float64 restatements
(oracle.RBF_cov -> np.linalg.cholesky -> products) are what the CPU half measures against them; 50 x the worst block error it finds is
the bar of the GPU half (RESTATEMENT_WORST, BAR), a margin over the reference's own error and never above 1e-10.

The measure of a trajectory is taken on the DISPLACEMENT q1 - q0 (formed exactly, in longdouble), block by block, and on the kinetic
energy: q0 is ~1e-4 and a step moves it by ~1e-7, so q1 itself would hide the drift under the start point."""
import functools
from fractions import Fraction

import numpy as np

LD = np.longdouble
JITTER = 1e-6
TRMM_CG = 8                                     # column group of k_prior_trmm (csrc/nmgp_metric.hip)
TILE = 64

HYPER_A = (1e-3, 0.3)                           # (alpha, beta) of factor A: tilde_l (separable: tilde_l)
HYPER_B = (3e-3, 0.2)                           # factor B: every uL column (separable: tilde_sigma)
HV_SVC = np.array([0.0, HYPER_A[0], HYPER_A[1], 0.0, HYPER_B[0], HYPER_B[1], 1.0, 1.0])
KAPPA_MAX = {"A": 200.0, "B": 2000.0}
# the hyper-parameters of today's tests (tests/test_hmc_metric.py): kappa ~ 1e9 .. 1e11, bar 1e-5 on the whole vector
HV_ILL = np.array([0.0, 10.0, 1.0, 0.0, 10.0, 1.0, 1.0, 1.0])
ILL_BAR = 1e-5

# Table A: svc_batch_prior_apply, both orientations.  Every M = 1 .. 8 (T = 1 .. 36: one to five column groups, last group of
# 1, 3, 6, 2, 7, 5, 4, 4), one to five 64-row tiles, both sides of 64 and 128.
TABLE_A = [(1, 1), (2, 2), (63, 1), (64, 8), (65, 3), (127, 5), (128, 4), (129, 6), (193, 7), (257, 2), (257, 8)]
BATCHES_A = (1, 5)                              # in the batch of 5 the last vector is a copy of vector 0
# Table B: 3 subjects x 2 chains, N = 65 (ld = 80: the subject stride ld N is not N^2), subject s on linspace(0, 1 + 0.1 s, N)
TABLE_B = [(65, 2), (65, 4)]
SUBJECTS, CHAINS_PER_SUBJECT = 3, 2
# Table C: sep_prior_apply (N, M, B); T = 1, 6, 36 exercise the tid < 64 + T lanes
TABLE_C = [(1, 1, 1), (63, 8, 4), (64, 3, 1), (65, 1, 4), (129, 8, 1), (193, 3, 4)]
SEP_C = (10.0, 2.3025851)                       # float32 rounds the second
# Table D: trajectories under the prior metric (N, M, r, B).  (65, 3, 257, 2): P = 456 and r = 257 > 256 (the strided loops of
# k_lowrank_apply / k_metric_kinetic); (40, 8, 24, 2): five column groups under the kick.
TABLE_D = [(65, 2, 0, 3), (65, 2, 1, 3), (65, 3, 257, 2), (129, 4, 5, 3), (64, 1, 7, 5), (40, 8, 24, 2)]
TABLE_D2 = [(65, 2, 1, 3), (129, 4, 5, 3)]      # nsteps = 2
FLAG_CASE = (65, 2, 1, 3)
# Table E: one step under the identity / a diagonal / a dense mass, (N, M, B): P = 257 and 513, a multiple of 256 plus one
TABLE_E = [(128, 1, 3), (128, 2, 3)]
MASS_KINDS = ("identity", "diagonal", "dense")
EPS = 1e-4
PRIOR = True                                    # the evaluations of tables D and E run with the priors on

# Worst block error of the float64 restatement against np.longdouble, per table: tests/test_metric_sweep_cpu.py measures it, prints
# the figures and asserts that none exceeds its entry here.  Measured (x86-64, 80-bit long double): A 3.6e-14 (N = 193, M = 7),
# B 2.3e-14, C 2.0e-14, D 3.4e-13 (the one-entry last block of (64, 1, 7, 5), chain 2: the rounding of q1 ~ 3e-4 against a
# displacement of ~1e-7), two steps 7.7e-14, E 8.9e-16; the entries are these with half as much again for another BLAS's rounding.
# ONE_ULP_SENSITIVITY: what moving every entry of the two-step cases' middle point by one unit in the last place does to the float64
# restatement, in the same measure (measured: nothing, not one bit) -- the two-step bar is table D's plus this.
RESTATEMENT_WORST = {"A": 5e-14, "B": 4e-14, "C": 3e-14, "D": 5e-13, "E": 1.5e-15}
ONE_ULP_SENSITIVITY = 1e-15
RESTATEMENT_WORST["D2"] = RESTATEMENT_WORST["D"] + ONE_ULP_SENSITIVITY
BAR = {k: 50.0 * v for k, v in RESTATEMENT_WORST.items()}
BAR_CAP = 1e-10
REJECT = 100.0                                  # a mutation is rejected by a block error >= REJECT x the bar


def n_slots(M):
    return M * (M + 1) // 2


def n_pars(layout, N, M):
    return N * (1 + n_slots(M)) + 1 if layout == "svc" else 2 * N + n_slots(M) + 1


def case_id(case):
    return "_".join("%s%s" % (k, v) for k, v in zip("NMrB" if len(case) == 4 else "NMB", case))


def _ro(a):
    a.setflags(write=False)
    return a


# ---------------------------------------------------------------------------------------------------
# inputs, covariances, factors
# ---------------------------------------------------------------------------------------------------
def grid(N, s=0):
    return _ro(np.linspace(0.0, 1.0 + 0.1 * s, N))


@functools.lru_cache(maxsize=None)
def data(N, M, s=0):
    """(x [N], Y [N, M]) of subject s: the prior factors depend on x alone; Y is what the trajectories' gradients see."""
    x = grid(N, s)
    rng = np.random.default_rng(7000 + 100 * N + 10 * M + s)
    Y = np.stack([np.sin(2.0 * np.pi * x * (m + 1)) + 0.1 * m for m in range(M)], 1) + 0.1 * rng.standard_normal((N, M))
    return x, _ro(np.ascontiguousarray(Y))


def cov_ld(x, alpha, beta):
    """RBF(x; alpha, beta) + 1e-6 I in longdouble, from (x_i - x_j)^2 directly."""
    xs = np.asarray(x, dtype=LD) / LD(beta)
    d = (xs[:, None] - xs[None, :]) ** 2
    return LD(alpha) ** 2 * np.exp(-d / LD(2)) + LD(JITTER) * np.eye(xs.shape[0], dtype=LD)


def cov_f64(x, alpha, beta):
    from oracle import nmgp_oracle as O
    return O.RBF_cov(np.asarray(x, dtype=np.float64)[:, None], None, alpha, beta)


def chol_ld(K):
    """Column Cholesky in the precision of K."""
    n = K.shape[0]
    L = np.zeros_like(K)
    for j in range(n):
        v = K[j:, j] - L[j:, :j] @ L[j, :j]
        L[j:, j] = v / np.sqrt(v[0])
    return L


_FACTORS = {}


def factor(which, N, s=0, prec="ld", hyper=None):
    """Lower Cholesky factor A or B of subject s's grid, longdouble ("ld") or the float64 restatement ("f64"); read-only, cached."""
    alpha, beta = hyper if hyper is not None else (HYPER_A if which == "A" else HYPER_B)
    key = "%s,%d,%d,%s,%r,%r" % (which, N, s, prec, alpha, beta)
    if key not in _FACTORS:
        x = grid(N, s)
        L = chol_ld(cov_ld(x, alpha, beta)) if prec == "ld" else np.linalg.cholesky(cov_f64(x, alpha, beta))
        _FACTORS[key] = _ro(L)
    return _FACTORS[key]


def factors(N, s=0, prec="ld"):
    return factor("A", N, s, prec), factor("B", N, s, prec)


def save_factors(path):
    """The longdouble factors computed so far, for a child process that runs the same cases (load_factors)."""
    np.savez(path, **{k: v for k, v in _FACTORS.items() if ",ld," in k})


def load_factors(path):
    d = np.load(path)
    for k in d.files:
        _FACTORS.setdefault(k, _ro(np.asarray(d[k], dtype=LD)))


# ---------------------------------------------------------------------------------------------------
# the block products, in the precision of the factors handed in
# ---------------------------------------------------------------------------------------------------
def apply_svc(L0, L1, v, trans=False):
    """blockdiag(L0, L1 per stride-T slot column, 1) v (or its transpose) for parameter-shaped rows v [B, P]:
    slot(0, i) = i, slot(j, i) = N + i T + j - 1, last slot identity."""
    N = L0.shape[0]
    v = np.asarray(v, dtype=L0.dtype)
    T = (v.shape[1] - 1 - N) // N
    A0, A1 = (L0.T, L1.T) if trans else (L0, L1)
    out = np.empty_like(v)
    out[:, :N] = v[:, :N] @ A0.T
    out[:, N:N + N * T] = np.matmul(A1, v[:, N:N + N * T].reshape(-1, N, T)).reshape(v.shape[0], -1)
    out[:, -1] = v[:, -1]
    return out


def apply_sep(L0, L1, c, v, trans=False, scale_uL=True):
    """blockdiag(L0, L1, c32 I_T, 1) v on [tilde_l | tilde_sigma | uL_vec | s2], c rounded to float32 as the entry does."""
    N = L0.shape[0]
    v = np.asarray(v, dtype=L0.dtype)
    A0, A1 = (L0.T, L1.T) if trans else (L0, L1)
    c32 = L0.dtype.type(float(np.float32(c))) if scale_uL else L0.dtype.type(1)
    out = np.empty_like(v)
    out[:, :N] = v[:, :N] @ A0.T
    out[:, N:2 * N] = v[:, N:2 * N] @ A1.T
    out[:, 2 * N:-1] = c32 * v[:, 2 * N:-1]
    out[:, -1] = v[:, -1]
    return out


@functools.lru_cache(maxsize=None)
def vectors(layout, N, M, B):
    """Test vectors [B, P]: standard normals; B = 5: the last one is a copy of vector 0.  The first min(B, 4) rows are the same for
    every B (a vector's result must not depend on the batch it sits in)."""
    P = n_pars(layout, N, M)
    v = np.random.default_rng(100 * N + M + (0 if layout == "svc" else 50000)).standard_normal((4, P))
    v = np.concatenate([v, v[:1]])[:B] if B == 5 else v[:B].copy()
    return _ro(np.ascontiguousarray(v))


def subject_vectors(N, M):
    """Table B's [S k, P]: chains 0, 1 of subject 0, chains of subject 1, and for subject 2 the vectors of subject 0 in the other order
    -- the same input under different factors."""
    v = vectors("svc", N, M, 4)
    return _ro(np.ascontiguousarray(np.concatenate([v, v[1::-1]])))


def unit_block_inputs(layout, N, M):
    """[B, P] inputs supported on ONE block each (its entries of vector 0), and the block's index per row: tilde_l, the first, a middle
    and the last slot column and the last entry (separable: the four segments)."""
    bl = blocks(layout, N, M)
    pick = sorted({0, 1, (len(bl) - 1) // 2, len(bl) - 2, len(bl) - 1}) if layout == "svc" else [0, 1, 2, 3]
    v = vectors(layout, N, M, 1)[0]
    e = np.zeros((len(pick), v.shape[0]))
    for row, k in enumerate(pick):
        e[row, bl[k][1]] = v[bl[k][1]]
    return e, pick


# ---------------------------------------------------------------------------------------------------
# the block measure
# ---------------------------------------------------------------------------------------------------
def blocks(layout, N, M):
    """[(name, index)]: nonseparable: tilde_l, each of the T slot columns (named by the slot's row and column in L), the last slot;
    separable: the four segments."""
    T = n_slots(M)
    if layout == "svc":
        r, c = np.tril_indices(M)
        out = [("tilde_l", slice(0, N))]
        out += [("uL[%d,%d]" % (r[t], c[t]), slice(N + t, N + N * T, T)) for t in range(T)]
        return out + [("sigma2", slice(N + N * T, N + N * T + 1))]
    return [("tilde_l", slice(0, N)), ("tilde_sigma", slice(N, 2 * N)), ("uL_vec", slice(2 * N, 2 * N + T)),
            ("sigma2", slice(2 * N + T, 2 * N + T + 1))]


def block_table(got, ref, layout):
    """{(row, block name): ||got_b - ref_b||_2 / ||ref_b||_2} for rows [B, P]; differences in longdouble.  Where a block of the
    reference is exactly zero the result must be exactly zero (error 0, else inf).  A NaN of the reference (an undefined start point)
    must be a NaN of the result and is left out of the norms; any other NaN is an infinite error."""
    lay, N, M = layout
    got, ref = np.atleast_2d(np.asarray(got, dtype=LD)), np.atleast_2d(np.asarray(ref, dtype=LD))
    assert got.shape == ref.shape and got.shape[1] == n_pars(lay, N, M), (got.shape, ref.shape, layout)
    tab = {}
    for b in range(ref.shape[0]):
        for name, sl in blocks(lay, N, M):
            g, r = got[b, sl], ref[b, sl]
            nan = np.isnan(r)
            if not np.array_equal(np.isnan(g), nan):
                e = np.inf
            else:
                g, r = g[~nan], r[~nan]
                nr = np.sqrt(np.sum(r * r))
                if nr == 0:
                    e = 0.0 if not np.any(g) else np.inf
                else:
                    e = float(np.sqrt(np.sum((g - r) ** 2)) / nr)
            tab[(b, name)] = e if np.isfinite(e) else np.inf
    return tab


def block_errors(got, ref, layout):
    """(error of the worst block, "row b: name"): a failure names the chain and the slot."""
    tab = block_table(got, ref, layout)
    key = max(tab, key=lambda k: tab[k])
    return tab[key], "row %d: %s" % key


def scalar_error(got, ref):
    """max_b |got_b - ref_b| / |ref_b| (kinetic energies); NaN anywhere: inf."""
    got, ref = np.asarray(got, dtype=LD), np.asarray(ref, dtype=LD)
    e = np.abs(got - ref) / np.abs(ref)
    return float(np.max(e)) if np.all(np.isfinite(e)) else np.inf


# ---------------------------------------------------------------------------------------------------
# the leapfrog step under the prior metric, in the precision of the factors handed in
# ---------------------------------------------------------------------------------------------------
def draw_table(lam):
    return np.sqrt(1 + lam) - 1


def kinetic_table(lam):
    return lam / (1 + lam)


def prior_draw(z, U, lam, table=draw_table):
    """u0 = z + U^T ((sqrt(1 + lam) - 1) o U z)"""
    if U.shape[0] == 0:
        return z.copy()
    return z + (table(lam) * (z @ U.T)) @ U


def prior_kick(u, g, c, bad, L0, L1, kick_bad=False):
    """u -= c L_blk^T g, skipped where bad (the gradient of an undefined point is undefined: NaN)"""
    new = u - c * apply_svc(L0, L1, g, trans=True)
    return new if kick_bad else np.where(np.asarray(bad, dtype=bool)[:, None], u, new)


def prior_drift(q, u, eps, U, lam, L0, L1, sign=-1):
    """q += eps L_blk (u - U^T (lam / (1 + lam) o U u))"""
    v = u if U.shape[0] == 0 else u + sign * ((kinetic_table(lam) * (u @ U.T)) @ U)
    return q + eps * apply_svc(L0, L1, v)


def prior_kinetic(u, U, lam, kmax=None):
    """1/2 (|u|^2 - sum_k lam_k / (1 + lam_k) (U u)_k^2)"""
    uu = np.sum(u * u, axis=1)
    if U.shape[0] == 0:
        return uu / 2
    corr = kinetic_table(lam) * (u @ U.T) ** 2
    return (uu - np.sum(corr[:, :kmax], axis=1)) / 2


def leapfrog_prior(q0, z, eps, nsteps, U, lam, L0, L1, g0, bad0, grad_at, mutation=None):
    """The trajectory of nmgp_svc_batch_traj_z under the prior-factor metric.  g0 [B, P], bad0 [B]: gradient and flag at q0;
    grad_at(k, q) -> (g, bad) at the k-th evaluated point q (k = 1 .. nsteps; the gradients are INPUTS: the gradient kernels have
    their own sweep).  Returns (points [q0, q_1, .., q_nsteps], kin1 [B]).  mutation: one of TRAJ_MUTATIONS."""
    dt = L0.dtype
    q, z, g = (np.asarray(a, dtype=dt) for a in (q0, z, g0))
    U, lam = np.asarray(U, dtype=dt).reshape(-1, q.shape[1]), np.asarray(lam, dtype=dt).reshape(-1)
    eps = dt.type(eps)
    bad = np.asarray(bad0, dtype=bool)
    u = prior_draw(z, U, lam, kinetic_table if mutation == "draw_with_kinetic_table" else draw_table)
    points = [q]
    for k in range(1, nsteps + 1):
        u = prior_kick(u, g, eps / 2 if k == 1 else eps, bad, L0, L1, mutation == "kick_a_bad_chain")
        new = prior_drift(q, u, eps, U, lam, L0, L1, +1 if mutation == "drift_plus" else -1)
        q = np.where(bad[:, None], q, new) if mutation == "no_drift_of_a_bad_chain" else new
        points.append(q)
        g, bad = grad_at(k, q)
        g, bad = np.asarray(g, dtype=dt), np.asarray(bad, dtype=bool)
    u = prior_kick(u, g, eps / 2, bad, L0, L1, mutation == "kick_a_bad_chain")
    return points, prior_kinetic(u, U, lam, 256 if mutation == "kinetic_first_256" else None)


TRAJ_MUTATIONS = ("drift_plus", "draw_with_kinetic_table", "kinetic_first_256", "kick_a_bad_chain", "no_drift_of_a_bad_chain")


def leapfrog_mass(kind, q0, z, eps, nsteps, minv, mchol, g0, bad0, grad_at, dtype=np.float64):
    """nmgp_svc_batch_traj_z under the identity, a diagonal (minv, mchol [P]) or a dense (minv, mchol [P, P], mchol mchol^T = M) mass:
    p0 = chol(M) z, kick p -= c g unless bad, drift q += eps M^-1 p, kin = 1/2 p^T M^-1 p.  In float64 the identity and diagonal
    steps are the kernels' operation for operation (t = c g; p - t; v = minv p; t = eps v; q + t): the same bits.
    Returns (points, kin1 [B], p1, v1)."""
    dt = np.dtype(dtype)
    q, z, g = (np.asarray(a, dtype=dt) for a in (q0, z, g0))
    eps = dt.type(eps)
    bad = np.asarray(bad0, dtype=bool)
    if kind != "identity":
        minv, mchol = np.asarray(minv, dtype=dt), np.asarray(mchol, dtype=dt)

    def vel(p):
        return p if kind == "identity" else (minv * p if kind == "diagonal" else p @ minv.T)
    p = z.copy() if kind == "identity" else (mchol * z if kind == "diagonal" else z @ mchol.T)
    points = [q]
    for k in range(1, nsteps + 1):
        t = (eps / 2 if k == 1 else eps) * g
        p = np.where(bad[:, None], p, p - t)
        t = eps * vel(p)
        q = q + t
        points.append(q)
        g, bad = grad_at(k, q)
        g, bad = np.asarray(g, dtype=dt), np.asarray(bad, dtype=bool)
    t = (eps / 2) * g
    p = np.where(bad[:, None], p, p - t)
    v = vel(p)
    return points, np.sum(p * v, axis=1) / 2, p, v


def kinetic_bits(p, minv_diag=None):
    """k_hmc_kinetic's float64 result to the bit for one chain p [P] (identity or diagonal mass): 256 strided partial sums of
    correctly rounded fused multiply-adds, a pairwise tree, times 1/2."""
    p = np.asarray(p, dtype=np.float64)
    v = p if minv_diag is None else np.asarray(minv_diag, dtype=np.float64) * p
    red = [0.0] * 256
    for i in range(p.shape[0]):
        red[i % 256] = float(Fraction(float(p[i])) * Fraction(float(v[i])) + Fraction(red[i % 256]))
    red = np.array(red)
    h = 128
    while h > 0:
        red[:h] = red[:h] + red[h:2 * h]
        h >>= 1
    return 0.5 * red[0]


# ---------------------------------------------------------------------------------------------------
# inputs of the trajectory tables
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def traj_inputs(N, M, r, B):
    """(q0 [B, P], z [B, P], U [r, P], lam [r]) of a table-D case, read-only.  q0: small smooth perturbations of zero curves, one
    amplitude and phase per chain; U: orthonormal rows; lam log-uniform in [0.5, 1e4], entry r // 2 exactly 0 where r >= 2
    (PriorMetric.stack pads ranks with zeros)."""
    P = n_pars("svc", N, M)
    rng = np.random.default_rng(31 * N + 7 * M + r)
    k = np.arange(P, dtype=np.float64)
    q0 = np.stack([1e-4 * (b + 1) * np.sin(0.01 * k + 0.4 * b) for b in range(B)])
    z = rng.standard_normal((B, P))
    if r > 0:
        Q, _ = np.linalg.qr(rng.standard_normal((P, r)))
        U = np.ascontiguousarray(Q.T)
        lam = np.exp(rng.uniform(np.log(0.5), np.log(1e4), r))
        if r >= 2:
            lam[r // 2] = 0.0
    else:
        U, lam = np.zeros((0, P)), np.zeros(0)
    return tuple(_ro(a) for a in (q0, z, U, lam))


@functools.lru_cache(maxsize=None)
def mass_inputs(N, M, B):
    """(q0, z, diag M^-1 [P], sqrt(diag M) [P], dense M^-1 [P, P], R [P, P] with R R^T = M) of a table-E case, read-only."""
    P = n_pars("svc", N, M)
    q0, z = traj_inputs(N, M, 0, B)[:2]
    rng = np.random.default_rng(9 * N + M)
    dinv = np.exp(rng.uniform(np.log(0.2), np.log(5.0), P))
    dchol = np.sqrt(1.0 / dinv)
    R = np.eye(P) + 0.3 * np.tril(rng.standard_normal((P, P))) / np.sqrt(P)
    Minv = np.linalg.inv(R @ R.T)
    Minv = 0.5 * (Minv + Minv.T)
    return tuple(_ro(np.ascontiguousarray(a)) for a in (q0, z, dinv, dchol, Minv, R))


def mass_pair(kind, N, M, B):
    _, _, dinv, dchol, Minv, R = mass_inputs(N, M, B)
    return {"identity": (None, None), "diagonal": (dinv, dchol), "dense": (Minv, R)}[kind]


def displacement(points, k=-1):
    """q_k - q_0 in longdouble (exact for float64 points)."""
    return np.asarray(points[k], dtype=LD) - np.asarray(points[0], dtype=LD)


def ulp_shift(q, seed=0):
    """q with every entry moved by one unit in the last place, up or down."""
    q = np.asarray(q, dtype=np.float64)
    up = np.random.default_rng(seed).random(q.shape) < 0.5
    return np.where(up, np.nextafter(q, np.inf), np.nextafter(q, -np.inf))


# ---------------------------------------------------------------------------------------------------
# mutations of the products: each returns the WRONG result
# ---------------------------------------------------------------------------------------------------
def _without_tiles(L, drop):
    L = L.copy()
    nt = (L.shape[0] + TILE - 1) // TILE
    for it in range(nt):
        for kt in range(it + 1):
            if drop(it, kt, nt):
                L[it * TILE:(it + 1) * TILE, kt * TILE:(kt + 1) * TILE] = 0
    return L


def mut_skip_factor_tile(L0, L1, v, trans):
    """1: the non-transposed product without the factor tiles (i-tile >= 2, k-tile 0).  Acts at N >= 129, trans = False."""
    f = lambda L: _without_tiles(L, lambda it, kt, nt: it >= 2 and kt == 0)
    return apply_svc(f(L0), f(L1), v, trans)


def mut_stop_one_tile_early(L0, L1, v, trans):
    """2: the transposed product stopping one tile early: k-tiles ib .. nblk - 2.  Acts at trans = True (every N)."""
    f = lambda L: _without_tiles(L, lambda it, kt, nt: it == nt - 1)
    return apply_svc(f(L0), f(L1), v, trans)


def mut_last_group_full(L0, L1, v, trans):
    """3: the last column group's nc computed as for a full group: its lanes j >= nc read slot j0 + j - 1 >= T, which is TRMM_CG added
    once too often on the flat array -- a low slot of the NEXT location -- and store their sum over that place.  Acts where T is no
    multiple of TRMM_CG."""
    N = L0.shape[0]
    v = np.asarray(v, dtype=L0.dtype)
    out = apply_svc(L0, L1, v, trans)
    T = (v.shape[1] - 1 - N) // N
    extra = (-T) % TRMM_CG
    A1 = L1.T if trans else L1
    flat = v[:, N:]                             # [B, N T + 1]: the slots and, behind them, the last entry
    for s in range(T, T + extra):
        idx = np.arange(N) * T + s
        ok = idx < N * T + 1                    # (reads and writes past the chain's vector: left out)
        vin = np.where(ok[None, :], flat[:, np.minimum(idx, N * T)], 0)
        val = vin @ A1.T
        out[:, N + idx[ok]] = val[:, ok]
    return out


def mut_swap_factors(L0, L1, v, trans):
    """4: L0 and L1 swapped."""
    return apply_svc(L1, L0, v, trans)


def mut_sep_swap_factors(L0, L1, c, v, trans):
    return apply_sep(L1, L0, c, v, trans)


def mut_sep_unscaled(L0, L1, c, v, trans):
    """5: the separable uL_vec block unscaled."""
    return apply_sep(L0, L1, c, v, trans, scale_uL=False)


SVC_MUTATIONS = {"skip_factor_tile": mut_skip_factor_tile, "stop_one_tile_early": mut_stop_one_tile_early,
                 "last_group_full": mut_last_group_full, "swap_factors": mut_swap_factors}


def svc_mutation_acts(name, N, M, trans):
    T = n_slots(M)
    return {"skip_factor_tile": N >= 2 * TILE + 1 and not trans, "stop_one_tile_early": trans,
            "last_group_full": T % TRMM_CG != 0, "swap_factors": True}[name]


# ---------------------------------------------------------------------------------------------------
# the flag scenarios of FLAG_CASE
# ---------------------------------------------------------------------------------------------------
OVERFLOW_SCALE = 1e13       # chain 1's z times this: eps L_blk u ~ 1e6, exp(tilde_l) overflows at the first evaluated point


def overflow_z(z):
    z = np.array(z, copy=True)
    z[1] *= OVERFLOW_SCALE
    return z


def nan_start(q0):
    q0 = np.array(q0, copy=True)
    q0[1, 0] = np.nan
    return q0
