"""Cases, inputs, high-precision references and derived error bars for the sweep of the ten primitive entries
(tests/test_primitive_sweep_cpu.py, tests/test_gpu_primitive_sweep.py): the 64-lane / 4-row workgroups of k_rect, the 256-column blocks
and the 4096-row grid of k_kron, every loop split of k_kron_mv<VEC2> (n2/2 around 192 and 256, a second chunk of m2, a second pass
over m1), M up to 64 and n = M N around 256 and 1024 behind the density / inverse entries.  A plain module, not a conftest: both
halves import it, so the CPU half checks the very cases the GPU half runs.  Inputs come from numpy.random.default_rng(seed of the
case); every reference is NumPy in numpy.longdouble on the host; no GPU result enters a bar.

Bars (eps = 2^-52), derived, not chosen:
 1. pairwise_distances, elementwise: |got - ref| <= (2d + 8) eps (|a|^2 + |b|^2): the first-order forward error of three length-d
    sums and two additions of the expanded form |a|^2 + |b|^2 - 2 a.b (for rbf_cov a, b are the inputs divided by beta).
 2. rbf_cov / nonstat_rbf_cov, elementwise and relative: c bar1 + eps (8 + |arg|), arg the exponent (dist / 2; dist / (li^2 + lj^2)),
    c = d arg / d dist: the error of the expanded distance enters through the exponent.
 3. kron_mv, elementwise: (n2 + m2 + 2) eps ((|B| kron |K|) |y|).
 4. mvn_logpdf (inverse supplied by the caller): (n + 4) eps (|logdet| / 2 + |r|^T |S^-1| |r| / 2).
 5. mvn_logpdf_kron, mvn_logpdf_dense, log-determinant and inverse of kron_inv_logdet, relative: max(64 eps, n eps cond_2(S),
    100 d_cpu), d_cpu the disagreement of the oracle's float64 formulations with the longdouble reference on that case; n eps cond is
    the forward error of a backward-stable method, 100 x the margin the prediction sweep gave itself over its two CPU references.
    The inverse in the max-norm, the log-determinant absolutely against bar max(1, |logdet|)."""
import functools

import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52
JITTER = 1e-6
ALPHA, BETA = 1.7, 0.4
SHIFT = 100.0
# sigma2 of the density / inverse cases.  At 0.05 the case (1, 257) has n eps cond(S) = 2.3e-10, above the 1e-10 every bar of item 5
# has to stay under (the bar of the fixture test): raised until it does (7.6e-11 there, cond 1.3e3), the bar is not loosened.
SIGMA2 = 0.15

# ---- cases ------------------------------------------------------------------------------------------------------------------------------
# (n1, n2, d, shift): 64 lanes along n2, 4 rows per workgroup; shift 100 on every coordinate is the cancellation case
RECT = [(1, 1, 1, 0.0), (3, 65, 1, 0.0), (4, 64, 2, 0.0), (5, 63, 3, 0.0), (65, 129, 3, 0.0), (5, 257, 7, 0.0), (130, 63, 1, 0.0),
        (130, 63, 1, SHIFT), (67, 66, 3, SHIFT)]
GIBBS_SYM = [(True, True), (True, False), (False, True), (False, False)]          # (s given, l given) of the symmetric form
# ((ar, ac), (br, bc)): widths 255 / 256 / 257 around the 256-column block, heights 4099 and 8193 past the 4096-row grid
KRON = [((1, 1), (1, 1)), ((2, 3), (4, 5)), ((1, 3), (2, 85)), ((1, 4), (3, 64)), ((2, 1), (1, 257)), ((4099, 1), (1, 3)),
        ((3, 2), (2731, 1))]
# (m1, m2, n1, n2): n2/2 = 192 no main pass, 193 lane 0 alone, 256 one pass and no tail, 257 / 513 a tail for lane 0 only; m2 > 8 a
# second chunk; m1 = 65 a second pass of the mixing loop; the last two rows are the scalar instantiation with two chunks
KMV = [(1, 1, 1, 1), (3, 3, 6, 6), (2, 9, 5, 2), (3, 8, 4, 384), (9, 8, 67, 386), (3, 12, 130, 512), (3, 12, 130, 514),
       (8, 17, 5, 1026), (65, 64, 4, 128), (5, 7, 3, 513), (2, 16, 7, 65)]
# (M, N): n = 255 / 256 / 257 at (3, 85) / (4, 64) / (1, 257); M > 8 at (9, 15), (16, 8), (64, 3); both parities of N
DENS = [(1, 1), (1, 5), (2, 2), (3, 6), (8, 33), (9, 15), (5, 64), (4, 65), (3, 85), (4, 64), (1, 257), (16, 8), (64, 3)]
TRIANGLE = [(5, 64), (4, 65)]
# n -> (p, q) with n = p q: S = A kron C with A of order p and C of order q, so that S^-1 = A^-1 kron C^-1 and
# log det S = q log det A + p log det C come from two small longdouble factorisations (a dense longdouble product of order 1025 takes
# 20 s); every element of the inverse is one longdouble product of two entries, rounded to float64
MVN = {1: (1, 1), 64: (1, 64), 65: (1, 65), 1023: (33, 31), 1024: (32, 32), 1025: (25, 41)}
MIRROR_RECT, MIRROR_KMV, MIRROR_DENS = (65, 129, 3, 0.0), (9, 8, 67, 386), (4, 65)
HISTORY = [("dens", c) for c in DENS] + [("kmv", c) for c in KMV]


def case_id(case):
    return "_".join(("%g" % v) if np.isscalar(v) else "x".join(str(u) for u in v) for v in case)


def _seed(tag, case):
    return [tag] + [int(v) for v in np.ravel(case)]


def ld(a):
    return np.asarray(a, dtype=np.float64).astype(LD)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rect_inputs(case):
    """x1 [n1, d], x2 [n2, d] uniform in [0, 1)^d (+ shift), Gibbs l = exp(-2 + 0.3 z), s = exp(0.3 z).  Shared: do not write."""
    n1, n2, d, shift = case
    rng = np.random.default_rng(_seed(1, case))
    return dict(x1=rng.uniform(0.0, 1.0, (n1, d)) + shift, x2=rng.uniform(0.0, 1.0, (n2, d)) + shift,
                s1=np.exp(0.3 * rng.standard_normal(n1)), l1=np.exp(-2.0 + 0.3 * rng.standard_normal(n1)),
                s2=np.exp(0.3 * rng.standard_normal(n2)), l2=np.exp(-2.0 + 0.3 * rng.standard_normal(n2)))


@functools.lru_cache(maxsize=None)
def kron_inputs(case):
    rng = np.random.default_rng(_seed(2, case))
    return rng.standard_normal(case[0]), rng.standard_normal(case[1])


@functools.lru_cache(maxsize=None)
def kmv_inputs(case):
    m1, m2, n1, n2 = case
    rng = np.random.default_rng(_seed(3, case))
    return rng.standard_normal((m1, m2)), rng.standard_normal((n1, n2)), rng.standard_normal(m2 * n2)


def sym_upper(A):
    """the symmetric matrix with the upper triangle of A, bit for bit"""
    return np.triu(A) + np.triu(A, 1).T


def spd_B(M, rng):
    """B = L L^T from a random lower triangle with exp on its diagonal"""
    L = np.tril(0.3 * rng.standard_normal((M, M)), -1) + np.diag(np.exp(0.2 * rng.standard_normal(M)))
    return sym_upper(L @ L.T)


def gibbs_K(N, rng):
    """the oracle's Gibbs covariance (jitter included) of N sorted inputs in (0, 1)"""
    from oracle import nmgp_oracle as O
    x = np.sort(rng.uniform(0.0, 1.0, N))
    s, l = np.exp(0.3 * rng.standard_normal(N)), np.exp(-2.0 + 0.3 * rng.standard_normal(N))
    return sym_upper(O.Nonstationary_RBF_cov(x[:, None], s, l))


@functools.lru_cache(maxsize=None)
def dens_inputs(case):
    M, N = case
    rng = np.random.default_rng(_seed(4, case))
    B, K = spd_B(M, rng), gibbs_K(N, rng)
    return dict(B=B, K=K, y=rng.standard_normal(M * N), mu=0.5 * rng.standard_normal(M * N), sigma2=SIGMA2)


def nan_lower(A):
    """A with its strictly lower triangle (row-major) overwritten by NaN"""
    A = A.copy()
    A[np.tril_indices(A.shape[0], -1)] = np.nan
    return A


# ---- longdouble linear algebra -------------------------------------------------------------------------------------------------------
def chol_ld(S):
    """column-by-column Cholesky of the longdouble matrix S: lower L with S = L L^T"""
    n = S.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        v = S[j:, j] - L[j:, :j] @ L[j, :j]
        assert v[0] > 0
        L[j, j] = np.sqrt(v[0])
        L[j + 1:, j] = v[1:] / L[j, j]
    return L


def forward_ld(L, R):
    """X with L X = R by forward substitution (R a vector or a matrix)"""
    X = np.zeros(R.shape, dtype=LD)
    for i in range(L.shape[0]):
        X[i] = (R[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


def spd_ld(S):
    """(log det S, S^-1 = L^-T L^-1, L) of the longdouble matrix S"""
    L = chol_ld(S)
    X = forward_ld(L, np.eye(S.shape[0], dtype=LD))
    return 2.0 * np.sum(np.log(np.diag(L))), X.T @ X, L


# ---- rectangular kernels: references and bars --------------------------------------------------------------------------------------------
def sqdist_ld(a, b):
    """the direct form sum_k (a_k - b_k)^2, which has no cancellation, and bar 1"""
    d = a.shape[1]
    ref = ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
    bar = (2 * d + 8) * LD(EPS) * ((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :])
    return ref, bar


def ref_dist(x1, x2=None):
    """(reference, absolute bar) of pairwise_distances"""
    a = ld(x1)
    return sqdist_ld(a, a if x2 is None else ld(x2))


def ref_rbf(x1, x2=None, alpha=ALPHA, beta=BETA):
    """(reference, absolute bar, largest exponent) of rbf_cov: the jitter sits on the diagonal only when x2 is None"""
    a = ld(x1) / LD(beta)
    dist, bar1 = sqdist_ld(a, a if x2 is None else ld(x2) / LD(beta))
    arg = dist / 2
    ref = LD(alpha) ** 2 * np.exp(-arg)
    if x2 is None:
        ref = ref + LD(JITTER) * np.eye(a.shape[0], dtype=LD)
    return ref, (bar1 / 2 + LD(EPS) * (8 + arg)) * ref, float(arg.max())


def ref_gibbs(x1, s1=None, l1=None, x2=None, s2=None, l2=None):
    """(reference, absolute bar, largest exponent) of nonstat_rbf_cov; with x2 None the second operand is the first"""
    a = ld(x1)
    s1 = np.ones(a.shape[0], dtype=LD) if s1 is None else ld(s1)
    l1 = np.ones(a.shape[0], dtype=LD) if l1 is None else ld(l1)
    if x2 is None:
        b, s2, l2 = a, s1, l1
    else:
        b, s2, l2 = ld(x2), ld(s2), ld(l2)
    dist, bar1 = sqdist_ld(a, b)
    A = (l1 * l1)[:, None] + (l2 * l2)[None, :]
    arg = dist / A
    ref = (s1[:, None] * s2[None, :]) * np.sqrt(2 * (l1[:, None] * l2[None, :]) / A) * np.exp(-arg)
    if x2 is None:
        ref = ref + LD(JITTER) * np.eye(a.shape[0], dtype=LD)
    return ref, (bar1 / A + LD(EPS) * (8 + arg)) * ref, float(arg.max())


def frac(got, ref, bar):
    """the largest |got - ref| / bar over all elements: inside the bar when <= 1.  No element is left out."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape == bar.shape and np.all(bar > 0), (got.shape, ref.shape)
    return float(np.max(np.abs(got.astype(LD) - ref) / bar))


def gibbs_args(case, form):
    """positional arguments of nonstat_rbf_cov: form (s given, l given) of the symmetric call, or 'sep' for a separate x2"""
    c = rect_inputs(case)
    if form == "sep":
        return (c["x1"], c["s1"], c["l1"], c["x2"], c["s2"], c["l2"])
    return (c["x1"], c["s1"] if form[0] else None, c["l1"] if form[1] else None)


@functools.lru_cache(maxsize=None)
def rect_refs(case):
    """{(entry, form): (reference, absolute bar[, largest exponent])}: form 'sym' / 'sep', for Gibbs (s given, l given) / 'sep'"""
    c = rect_inputs(case)
    out = {("dist", "sym"): ref_dist(c["x1"]), ("dist", "sep"): ref_dist(c["x1"], c["x2"]),
           ("rbf", "sym"): ref_rbf(c["x1"]), ("rbf", "sep"): ref_rbf(c["x1"], c["x2"])}
    for form in GIBBS_SYM + ["sep"]:
        out[("gibbs", form)] = ref_gibbs(*gibbs_args(case, form))
    return out


# ---- kron_product, kron_mv -----------------------------------------------------------------------------------------------------------------
def ref_kron_mv(B, K, y):
    """(vec(K Y B^T), bar 3) in longdouble"""
    m2, n2 = B.shape[1], K.shape[1]
    Bl, Kl, Yl = ld(B), ld(K), ld(y).reshape(m2, n2).T
    ref = (Kl @ Yl @ Bl.T).T.reshape(-1)
    mag = (np.abs(Kl) @ np.abs(Yl) @ np.abs(Bl).T).T.reshape(-1)
    return ref, (n2 + m2 + 2) * LD(EPS) * mag


@functools.lru_cache(maxsize=None)
def kmv_ref(case):
    return ref_kron_mv(*kmv_inputs(case))


# ---- densities, log-determinant, inverse -----------------------------------------------------------------------------------------------------
def relerr(got, ref):
    return float(abs(LD(got) - ref) / abs(ref))


def inv_err(got, ref):
    """max-norm of the difference over the max-norm of the reference"""
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64).astype(LD) - ref)) / np.max(np.abs(ref)))


def logdet_err(got, ref):
    """absolute, against max(1, |logdet|)"""
    return float(abs(LD(got) - ref) / max(LD(1), abs(ref)))


def dense_ref(B, K, y, mu, sigma2):
    """The longdouble reference of one density / inverse problem: S = B kron K + sigma2 I factored by chol_ld; the bars of item 5 from
    cond_2(S) and the oracle's float64 formulations; the float64 roundings of the inverse and the log-determinant for mvn_logpdf."""
    from oracle import nmgp_oracle as O
    n = B.shape[0] * K.shape[0]
    S = np.kron(ld(B), ld(K)) + LD(sigma2) * np.eye(n, dtype=LD)
    logdet, inv, L = spd_ld(S)
    r = ld(y) - (0 if mu is None else ld(mu))
    z = forward_ld(L, r)
    logpdf = -0.5 * logdet - 0.5 * (z @ z)
    w = np.linalg.eigvalsh(S.astype(np.float64))
    cond = float(w[-1] / w[0])
    mu0 = np.zeros(n) if mu is None else mu
    d_cpu = dict(logpdf=max(relerr(O.multivariate_normal_logpdf0(y, mu0, B, K, sigma2), logpdf),
                            relerr(O.multivariate_normal_logpdf2(y, mu0, B, K, sigma2), logpdf)),
                 inv=inv_err(O.kron_inv(sigma2, B, K), inv), logdet=logdet_err(O.kron_logdet(sigma2, B, K), logdet))
    bars = {k: max(64 * EPS, n * EPS * cond, 100.0 * v) for k, v in d_cpu.items()}
    return dict(n=n, logdet=logdet, inv=inv, logpdf=logpdf, cond=cond, d_cpu=d_cpu, bars=bars,
                inv64=np.ascontiguousarray(inv.astype(np.float64)), logdet64=float(logdet))


@functools.lru_cache(maxsize=None)
def dens_ref(case):
    c = dens_inputs(case)
    return dense_ref(c["B"], c["K"], c["y"], c["mu"], c["sigma2"])


def ref_mvn(y, mu, logdet64, inv64):
    """(reference, bar 4) of mvn_logpdf at the float64 log-determinant and inverse the caller supplies"""
    n = y.shape[0]
    r = ld(y) - (0 if mu is None else ld(mu))
    P = ld(inv64)
    ref = -0.5 * LD(logdet64) - 0.5 * (r @ (P @ r))
    return ref, float((n + 4) * EPS * (0.5 * abs(LD(logdet64)) + 0.5 * (np.abs(r) @ (np.abs(P) @ np.abs(r)))))


@functools.lru_cache(maxsize=None)
def mvn_inputs(n):
    """y, mu, and the longdouble inverse and log-determinant of S = A kron C (MVN[n]) rounded to float64"""
    p, q = MVN[n]
    rng = np.random.default_rng(_seed(5, (n,)))
    A, C = spd_B(p, rng), gibbs_K(q, rng) + SIGMA2 * np.eye(q)
    ldA, invA, _ = spd_ld(ld(A))
    ldC, invC, _ = spd_ld(ld(C))
    return dict(y=rng.standard_normal(n), mu=0.5 * rng.standard_normal(n), logdet=float(q * ldA + p * ldC),
                inv=np.ascontiguousarray(np.kron(invA, invC).astype(np.float64)))


# ---- one item of the call history: what is called, and the achieved errors next to their bars ---------------------------------------------
def run_dens(ctx, case, B=None, K=None):
    """every density / inverse entry on one case through a _lib.Context:
    (mvn_logpdf_kron, mvn_logpdf_dense, logdet without the inverse, logdet, inverse, mvn_logpdf at the reference's inverse)"""
    c, r = dens_inputs(case), dens_ref(case)
    B, K = c["B"] if B is None else B, c["K"] if K is None else K
    lk = ctx.mvn_logpdf_kron(c["y"], c["mu"], B, K, c["sigma2"])
    lde = ctx.mvn_logpdf_kron(c["y"], c["mu"], c["B"], c["K"], c["sigma2"], dense=True)
    none, ld0 = ctx.kron_inv_logdet(c["sigma2"], B, K, want_inv=False)
    assert none is None
    inv, ld1 = ctx.kron_inv_logdet(c["sigma2"], B, K, want_inv=True)
    lp = ctx.mvn_logpdf(c["y"], c["mu"], r["logdet64"], r["inv64"])
    return (np.float64(lk), np.float64(lde), np.float64(ld0), np.float64(ld1), inv, np.float64(lp))


def dens_errs(case, res):
    """{name: (achieved, bar)} of the results of run_dens (or of the same six quantities from a CPU formulation)"""
    r = dens_ref(case)
    c = dens_inputs(case)
    lk, lde, ld0, ld1, inv, lp = res
    assert inv.shape == r["inv"].shape
    mref, mbar = ref_mvn(c["y"], c["mu"], r["logdet64"], r["inv64"])
    return dict(logpdf_kron=(relerr(lk, r["logpdf"]), r["bars"]["logpdf"]), logpdf_dense=(relerr(lde, r["logpdf"]), r["bars"]["logpdf"]),
                logdet_alone=(logdet_err(ld0, r["logdet"]), r["bars"]["logdet"]), logdet=(logdet_err(ld1, r["logdet"]), r["bars"]["logdet"]),
                inv=(inv_err(inv, r["inv"]), r["bars"]["inv"]), mvn_logpdf=(float(abs(LD(lp) - mref)), mbar))


def run_kmv(ctx, case):
    return (ctx.kron_mv(*kmv_inputs(case)),)


def kmv_errs(case, res):
    ref, bar = kmv_ref(case)
    return dict(kron_mv=(frac(res[0], ref, bar), 1.0))


def run_item(ctx, item):
    return (run_dens if item[0] == "dens" else run_kmv)(ctx, item[1])


def item_errs(item, res):
    return (dens_errs if item[0] == "dens" else kmv_errs)(item[1], res)


def item_id(item):
    return item[0] + "_" + case_id(item[1])
