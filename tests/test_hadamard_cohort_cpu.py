"""CPU half of the Hadamard cohort tests (tests/hadamard_cohort_cases.py).

1. The subjects the cohort sets add to the sweep's table meet what tests/test_hadamard_sweep_cpu.py asserts for its own: every label
   occurs, cond(S) < 1e4 for both chains, the restated gradient within 1e-5 of central differences with and without the priors; for
   the subjects of sets F - I no predictive variance meets the clip.  The two terms of the GPU half's per-block gradient bar
   (tests/hadamard_cases.py: d_cpu between the restatement and the padded formulation at the set's Nmax, N_s cond(S) eps) are
   computed, printed and d_cpu held below 1e-9; the prior part g(prior) - g(no prior) of the two LAPACK blockings agrees per block
   below 1e-7.  Measured: d_cpu <= 8.8e-14 over sets A - I and the three models (2.7e-14 on sets F - H), prior part <= 3.5e-9 (set
   I; 7.9e-10 on set H); the bars come to 2.2e-16 (N_s = M = 1) ... 4e-11 at (257, 7) ... 8.6e-10 at (1030, 2).
2. The padded formulation nmgp_had_subjects_eval runs on the device, restated in NumPy: S, y and both GP-prior covariances padded to Nmax
   with identity / zero, the trace over the real observations.  It equals the per-subject restatement on set A: value and likelihood
   1e-12 relative, gradient 1e-10 in ||dg|| / ||g||, the GP-prior entries included (the chain of comparisons is in the test's
   docstring).  With the trace taken over Nmax the sigma2 slot misses that bar, which is asserted too: the test can bite.
3. cohort_pack / cohort_unpack round-trip; cohort_buckets returns the partition its rule implies."""
import math

import numpy as np
import pytest
from scipy.linalg import cholesky, solve_triangular

import hadamard_cases as hc
import hadamard_cohort_cases as cc
from conftest import relerr, vec_relerr
from oracle import nmgp_oracle as oracle
from test_hadamard_cpu import had_covariance, had_rows
from test_hadamard_sweep_cpu import COND_MAX, EPS, FD_TOL, direction

VAL_TOL, GRAD_TOL = 1e-12, 1e-10


# ---- 1. preconditions of the new subjects ---------------------------------------------------------------------------------------------
def test_the_sets_are_the_sweeps_subjects_plus_the_new_ones():
    known = set(hc.CASES + [hc.WIDE, hc.MINOR])
    used = {case for cases in cc.ALL_SETS.values() for case in cases}
    assert used - known == set(cc.NEW_SUBJECTS) and len(cc.NEW_SUBJECTS) == len(set(cc.NEW_SUBJECTS)) == 9 + 17
    assert cc.NEW_SUBJECTS[9:] == cc.SWEEP_SUBJECTS and len(cc.SWEEP_SUBJECTS) == 17
    assert cc.nobs(cc.SET_A) == [128, 63, 2, 64, 65, 127] and cc.nobs(cc.SET_B) == [193, 8, 130] and cc.nobs(cc.SET_D) == [1, 2, 70]
    assert cc.nobs(cc.SET_C) == [321, 65, 256, 3] and cc.nobs(cc.SET_E) == [64, 64]
    assert cc.nobs(cc.SET_F) == [4, 64, 65, 129, 100] and cc.nobs(cc.SET_G) == [65, 6, 128, 127, 192]
    assert cc.nobs(cc.SET_H) == [129, 7, 63, 257, 130] and cc.nobs(cc.SET_I) == [1030, 1025, 513, 640]
    for cases, M in zip((cc.SET_A, cc.SET_B, cc.SET_C, cc.SET_D, cc.SET_E, cc.SET_F, cc.SET_G, cc.SET_H, cc.SET_I), (2, 8, 3, 1, 5, 4, 6, 7, 2)):
        assert {case[1] for case in cases} == {M}
    # sets G and H keep a subject of the resident sweep each; set I stays out of the parametrisations over SETS
    assert cc.SET_G[0] in hc.CASES and cc.SET_H[0] in hc.CASES and sorted(cc.SETS) == list("ABCDEFGH") and sorted(cc.LARGE_SETS) == ["I"]
    # set I: the trace kernel's second pass (N_s > 1024) for two subjects and not for two, every subject beyond one 512-column panel
    assert sum(n > 1024 for n in cc.nobs(cc.SET_I)) == 2 and min(cc.nobs(cc.SET_I)) > 512


@pytest.mark.parametrize("case", cc.NEW_SUBJECTS, ids=hc.case_id)
def test_new_subject_meets_the_preconditions(case):
    N, M, layout = case
    c = hc.build(case)
    assert c["indx"].dtype == np.int32 and sorted(np.unique(c["indx"]).tolist()) == list(range(M))
    P = c["pars"]["had"]
    assert P.shape == (2, N * (1 + c["T"]) + 1) and not np.array_equal(P[0], P[1])
    for k in (0, 1):
        cond = np.linalg.cond(hc.ref_covariance("had", P[k], c))
        print(hc.case_id(case), "chain", k, "cond", cond)
        assert cond < COND_MAX, (k, cond)
    p = P[1]
    for prior in (False, True):
        v = direction("had", c, smooth=prior)
        g = hc.ref_logpos("had", p, c, prior, grad=True)[1]
        fd = (hc.ref_logpos("had", p + EPS * v, c, prior)[0] - hc.ref_logpos("had", p - EPS * v, c, prior)[0]) / (2.0 * EPS)
        err = abs(fd - g @ v) / abs(fd)
        print(hc.case_id(case), "prior", prior, "directional derivative", fd, "relative error", err)
        assert err < FD_TOL, (prior, err)


@pytest.mark.parametrize("case", cc.SWEEP_SUBJECTS, ids=hc.case_id)
def test_no_predictive_variance_of_a_sweep_subject_meets_the_clip(case):
    """sets F - I: every variance before the clip exceeds its chain's sigma2_err, for the restatements of the separable and stationary
    predictors (hc.predictions) and of the nonseparable one (predsample_had_cases.expected)."""
    import predsample_had_cases as pc
    floors = hc.raw_variance_floor(hc.predictions(case), hc.build(case)), pc.raw_variance_floor(pc.expected(case), case)
    print(hc.case_id(case), "min variance / sigma2_err", floors)
    assert min(floors) > 1.0, floors


def set_nmax(name):
    return max(cc.nobs(cc.ALL_SETS[name]))


@pytest.mark.parametrize("name", sorted(cc.ALL_SETS))
def test_block_bars_rest_on_two_cpu_references(name):
    """The per-block bar of the GPU half, min(GRAD_TIGHT, max(100 d_cpu, N_s cond(S) eps)) (tests/hadamard_cases.py): both terms come
    from the CPU alone.  d_cpu, the worst block between the per-subject restatement and the padded formulation at the set's Nmax, stays
    below GRAD_TIGHT / 10, so the two references determine every block an order below the loosest bar."""
    for case in cc.ALL_SETS[name]:
        d, stable = hc.block_bar_terms("had", case, set_nmax(name))
        print("set", name, hc.case_id(case), "had d_cpu", d, "N cond(S) eps", stable, "bar", hc.block_bar("had", case, set_nmax(name)))
        assert d < hc.GRAD_TIGHT / 10, (case, d)
        assert 0.0 < hc.block_bar("had", case, set_nmax(name)) <= hc.GRAD_TIGHT


def single_observation_gradient_longdouble(model, chain):
    """d NegLog / d pars without the priors at the subject (1, 1, interleaved) in closed form, in np.longdouble:
    S = (K0 + jitter) L^2 + sigma2 with K0 = exp(tilde_sigma)^2 ("sep") or 1 ("had"), G = 1/2 (y^2 / S^2 - 1 / S); the lengthscale
    has no likelihood gradient at one observation."""
    LD = np.longdouble
    c = hc.build((1, 1, "interleaved"))
    p, y = [LD(v) for v in c["pars"][model][chain]], LD(c["y"][0])
    tl, ts, L, tse = p if model == "sep" else (p[0], LD(0), p[1], p[2])
    k0, s2, jitter = np.exp(ts) ** 2, np.exp(tse), LD(1e-6)
    S = (k0 + jitter) * L * L + s2
    G = LD(0.5) * ((y / S) ** 2 - 1 / S)
    g = [LD(0)] + ([2 * G * k0 * L * L] if model == "sep" else []) + [2 * G * (k0 + jitter) * L, s2 * G]
    return -np.array(g, dtype=LD)


@pytest.mark.parametrize("model", ["had", "sep"])
def test_the_single_observation_subject_has_bars_from_a_longdouble_reference(model):
    """At N_s = M = 1 the restatement and the padded formulation run the same scalar operations: d_cpu = 0 and the rule's bar is one
    eps, below the restatement's own distance from the closed form in np.longdouble.  hadamard_cases.BLOCK_BARS holds ten times that
    distance for the blocks where it is not 0; every other block of the subject keeps the rule's bar."""
    case = (1, 1, "interleaved")
    assert hc.block_bar_terms(model, case, 70) == (0.0, hc.MACHINE_EPS) == hc.block_bar_terms(model, case)
    tabs = []
    for k in (0, 1):
        ld = single_observation_gradient_longdouble(model, k)
        ref = hc.reference(model, case, k, False)[1]
        assert np.allclose(ref, ld.astype(np.float64), rtol=1e-14, atol=0.0)              # the closed form IS the restatement's objective
        floor = 1e-3 * np.sqrt(np.sum(ld * ld))
        tabs.append({name: float(np.sqrt(np.sum((ref[sl] - ld[sl]) ** 2)) / max(np.sqrt(np.sum(ld[sl] ** 2)), floor))
                     for name, sl in __import__("objective_cases").blocks(*hc.layout(model, 1, 1))})
    for name in tabs[0]:
        measured = max(t[name] for t in tabs)
        entry = hc.BLOCK_BARS.get(hc.layout(model, 1, 1) + (name,))
        print(model, name, "restatement against np.longdouble", measured, "bar", entry)
        if entry is None:
            assert 10.0 * measured <= hc.MACHINE_EPS, (name, measured)
        else:
            assert 10.0 * measured <= entry <= 5e-15, (name, measured, entry)
    assert [k for k in hc.BLOCK_BARS if k[1:3] != (1, 1)] == []


@pytest.mark.parametrize("name", sorted(cc.ALL_SETS))
def test_prior_part_is_determined_block_by_block(name):
    """g(prior) - g(no prior), what the GPU half compares block by block at 1e-5 with the priors on: the two LAPACK blockings of the
    reference (the subject alone, and padded to the set's Nmax) agree per block below PRIOR_PART_REFERENCE = 1e-7."""
    worst = 0.0
    for case in cc.ALL_SETS[name]:
        for k in (0, 1):
            tab = hc.block_table(hc.prior_part("had", case, k, set_nmax(name)), hc.prior_part("had", case, k), "had", case[0], case[1])
            worst = max(worst, max(tab.values()))
            assert max(tab.values()) < hc.PRIOR_PART_REFERENCE, (case, k, tab)
    print("set", name, "had prior part, alone against padded: worst block", worst)


# ---- 2. the padded formulation ---------------------------------------------------------------------------------------------------------
def pad_identity(A, Nmax):
    out = np.eye(Nmax)
    out[:A.shape[0], :A.shape[0]] = A
    return out


# Two sets of linear-algebra routines for the restatement below.  LAPACK: what the reference restatement calls.  ELEMENTWISE: an
# unblocked right-looking Cholesky and column-oriented substitutions written with elementwise NumPy operations only, so that every
# entry goes through the same sequence of roundings whatever the order of the matrix: padding with identity / zero is then a TRUE
# reordering (the real block of every factor and solution has the same bits) also for the GP-prior covariances, whose condition number
# of up to 1e11 would let a change of LAPACK's blocking move the Mahalanobis terms by far more than 1e-12.
def chol_elementwise(A):
    A = np.array(A, dtype=np.float64)
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        L[j:, j] = A[j:, j] / math.sqrt(A[j, j])
        A[j + 1:, j + 1:] -= L[j + 1:, j, None] * L[None, j + 1:, j]
    return L


def forward_elementwise(L, B):
    X = np.array(B, dtype=np.float64)
    for j in range(L.shape[0]):
        X[j] = X[j] / L[j, j]
        X[j + 1:] -= (L[j + 1:, j, None] * X[None, j]) if X.ndim == 2 else L[j + 1:, j] * X[j]
    return X


def backward_elementwise(L, B):
    X = np.array(B, dtype=np.float64)
    for j in range(L.shape[0] - 1, -1, -1):
        X[j] = X[j] / L[j, j]
        X[:j] -= (L[j, :j, None] * X[None, j]) if X.ndim == 2 else L[j, :j] * X[j]
    return X


LAPACK = (lambda A: cholesky(A, lower=True), lambda L, B: solve_triangular(L, B, lower=True),
          lambda L, B: solve_triangular(L, B, lower=True, trans="T"))
ELEMENTWISE = (chol_elementwise, forward_elementwise, backward_elementwise)


def padded_logpos(pars, c, Nmax, prior, trace_over_nmax=False, ops=LAPACK):
    """The verbose tuple and d NegLog / d pars (the subject's own layout) computed the way the device does it: every matrix of order
    Nmax, padded observations masked to the identity / zero.  Nmax = N is the per-subject restatement under the same routines."""
    chol, forward, backward = ops
    x, indx, y, hyper = c["x"], c["indx"].astype(np.int64), c["y"], c["hyper"]["had"]
    N, M, T = c["N"], c["M"], c["T"]
    pars = np.asarray(pars, dtype=np.float64)
    tl, tse = pars[:N], float(pars[-1])
    sigma2 = math.exp(tse)
    mu_l, al_l, be_l, mu_L, al_L, be_L, a, b = [float(v) for v in hyper[:8]]
    S = pad_identity(had_covariance(tl, pars[N:N + N * T], tse, x, indx, M), Nmax)
    yp = np.concatenate([y, np.zeros(Nmax - N)])
    C = chol(S)
    assert np.array_equal(C[N:, N:], np.eye(Nmax - N)) and not np.any(C[N:, :N])      # the padded part of the factor: exactly I | 0
    z = forward(C, yp)
    loglik = -np.log(np.diag(C)).sum() - 0.5 * (z @ z)
    X1 = x.reshape(-1, 1)
    lps, gps = [], []
    U = pars[N:N + N * T].reshape(N, T)
    for cols, mu, al, be in ((tl[:, None], mu_l, al_l, be_l), (U, mu_L, al_L, be_L)):
        Cp = chol(pad_identity(oracle.RBF_cov(X1, alpha=al, beta=be), Nmax))
        assert np.array_equal(Cp[N:, N:], np.eye(Nmax - N)) and not np.any(Cp[N:, :N])
        R = np.zeros((Nmax, cols.shape[1]))
        R[:N] = cols - mu                                                           # centred real slots, zeros in the padded ones
        Z = forward(Cp, R)
        assert not np.any(Z[N:])
        lp = sum(-0.5 * (N * oracle.LOG_2PI + Z[:, t] @ Z[:, t]) - np.log(np.diag(Cp)).sum() for t in range(cols.shape[1]))
        lps.append(lp)
        gps.append(backward(Cp, Z)[:N])
    lp_s2 = oracle.inverse_gamma_logpdf_u(sigma2, alpha=a, beta=b)
    res = loglik + ((lps[0] + lps[1] + lp_s2 + tse) if prior else 0.0)
    out = np.array([-res, loglik, lps[0], lps[1], lp_s2])
    alpha = backward(C, z)
    Sinv = backward(C, forward(C, np.eye(Nmax)))
    assert np.array_equal(alpha[N:], np.zeros(Nmax - N)) and np.array_equal(Sinv[N:, N:], np.eye(Nmax - N)) and not np.any(Sinv[N:, :N])
    G = 0.5 * (np.outer(alpha, alpha) - Sinv)[:N, :N]
    trace = np.trace(Sinv) if trace_over_nmax else np.trace(Sinv[:N, :N])
    R = had_rows(pars[N:N + N * T], indx, M)
    ell = np.exp(tl)
    D = oracle.pairwise_distances(X1)
    A = (ell ** 2)[:, None] + (ell ** 2)[None, :]
    K0 = np.sqrt(2.0 * np.outer(ell, ell) / A) * np.exp(-D / A)
    dR = 2.0 * (G * (K0 + 1e-6 * np.eye(N))) @ R
    e2 = (ell ** 2)[:, None]
    W = 2.0 * G * K0 * (R @ R.T) * (0.5 - e2 / A + 2.0 * e2 * D / (A * A))
    np.fill_diagonal(W, 0.0)
    g_L = np.zeros((N, T))
    for i, ci in enumerate(indx):
        g_L[i, ci * (ci + 1) // 2: ci * (ci + 1) // 2 + ci + 1] = dR[i, :ci + 1]
    g = np.concatenate([W.sum(1), g_L.reshape(-1), [sigma2 * 0.5 * (alpha @ alpha - trace)]])
    if prior:
        g[:N] -= gps[0][:, 0]
        g[N:N + N * T] -= gps[1].reshape(-1)
        g[-1] += (-a - 1.0) + b / sigma2 + 1.0
    return out, -g


def errors(out, grad, ref_out, ref_grad):
    return dict(value=relerr(out[0], ref_out[0]), loglik=relerr(out[1], ref_out[1]), priors=relerr(out[2:], ref_out[2:]),
                grad=vec_relerr(grad, ref_grad))


def within_the_issues_bars(e):
    return e["value"] < VAL_TOL and e["loglik"] < VAL_TOL and e["priors"] < VAL_TOL and e["grad"] < GRAD_TOL


@pytest.mark.parametrize("case", cc.SET_A, ids=hc.case_id)
def test_padded_formulation_equals_the_per_subject_restatement(case):
    """Three links, every quantity (value, likelihood, prior entries, gradient) with and without the priors:
    a. this file's formulation at Nmax = N_s under LAPACK IS the per-subject restatement hadamard_cases.ref_logpos: the issue's bars;
    b. padded to Nmax = 128 against Nmax = N_s, both under the elementwise routines, where padding is a true reordering also for the
       prior factors: the issue's bars, priors included;
    c. padded to 128 under LAPACK against ref_logpos: the issue's bars for the likelihood and the prior-free objective (cond(S) < 1e4).
       With the priors this link compares two BLOCKINGS of LAPACK's factorisation of matrices of condition 1e11, not two formulations:
       its figures are printed (measured: value <= 6e-12, prior entries <= 1.1e-11, gradient <= 3.2e-10) and (a) + (b) carry the check.
    With the trace over Nmax the sigma2 slot misses the gradient bar in (b) and (c): the test can bite."""
    c = hc.build(case)
    N, Nmax = c["N"], max(cc.nobs(cc.SET_A))
    for k in (0, 1):
        p = c["pars"]["had"][k]
        for prior in (True, False):
            tag = "%s chain %d prior %d" % (hc.case_id(case), k, prior)
            ref_out, ref_grad = cc.reference(case, k, prior)
            ea = errors(*padded_logpos(p, c, N, prior), ref_out, ref_grad)
            print(tag, "(a) own formulation, unpadded, against the restatement", ea)
            assert within_the_issues_bars(ea), ea
            alone = padded_logpos(p, c, N, prior, ops=ELEMENTWISE)
            out_b, grad_b = padded_logpos(p, c, Nmax, prior, ops=ELEMENTWISE)
            eb = errors(out_b, grad_b, *alone)
            print(tag, "(b) padded against unpadded, elementwise routines", eb)
            assert within_the_issues_bars(eb), eb
            out, grad = padded_logpos(p, c, Nmax, prior)
            ec = errors(out, grad, ref_out, ref_grad)
            print(tag, "(c) padded under LAPACK against the restatement", ec)
            assert ec["loglik"] < VAL_TOL and ref_out[4] == out[4]
            if not prior:
                assert ec["value"] < VAL_TOL and ec["grad"] < GRAD_TOL
            for ops, good, ref in ((ELEMENTWISE, grad_b, alone[1]), (LAPACK, grad, ref_grad)):
                bad = padded_logpos(p, c, Nmax, prior, trace_over_nmax=True, ops=ops)[1]
                assert np.array_equal(bad[:-1], good[:-1])
                if N < Nmax:           # tr S^-1 over Nmax counts one per padded observation: the sigma2 slot misses the bar
                    print(tag, "sigma2 slot with the trace over Nmax", bad[-1], "against", ref[-1])
                    assert abs(bad[-1] - ref[-1]) / abs(ref[-1]) > 1e3 * GRAD_TOL and vec_relerr(bad, ref) > GRAD_TOL
                else:
                    assert bad[-1] == good[-1]


# ---- 3. the host helpers ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2])
def test_cohort_pack_and_unpack_round_trip(k):
    from nonstationary_multivariate_gaussian_process_amd import hadamard
    sizes, M, T = cc.nobs(cc.SET_A), 2, 3
    vectors = cc.chains(cc.SET_A, k)
    for Nmax in (None, 130):
        P = hadamard.cohort_pack(vectors, sizes, M, Nmax=Nmax, fill=np.nan)
        N = 128 if Nmax is None else Nmax
        assert P.shape == (len(sizes) * k, N * (1 + T) + 1)
        pads = cc.padded_slots(sizes, M, N, k)
        assert np.all(np.isnan(P[pads])) and np.all(np.isfinite(P[~pads])) and pads.sum() == sum((N - n) * (1 + T) * k for n in sizes)
        back = hadamard.cohort_unpack(P, sizes, M, chains_per_subject=k)
        assert len(back) == len(sizes) and all(np.array_equal(u, v) for u, v in zip(back, vectors))
        for s, n in enumerate(sizes):          # the layout itself: blocks of Nmax and Nmax T, the last slot
            assert np.array_equal(P[s * k, :n], vectors[s][0, :n]) and np.array_equal(P[s * k, N:N + n * T], vectors[s][0, n:n + n * T])
            assert P[s * k + k - 1, -1] == vectors[s][k - 1, -1]
    if k == 1:                                 # one vector per subject may be given as [P_s]
        flat = hadamard.cohort_pack([v[0] for v in vectors], sizes, M)
        assert np.array_equal(flat, hadamard.cohort_pack(vectors, sizes, M)) and not np.any(flat[cc.padded_slots(sizes, M, 128)])
    with pytest.raises(ValueError):
        hadamard.cohort_pack(vectors, sizes, M, Nmax=127)


def check_buckets(sizes, w, buckets):
    assert sorted(int(s) for b in buckets for s in b) == list(range(len(sizes)))          # a partition
    for b in buckets:
        n = [sizes[int(s)] for s in b]
        assert n == sorted(n, reverse=True) and len(n) * max(n) ** 3 <= (1.0 + w) * sum(v ** 3 for v in n)


def test_cohort_buckets():
    from nonstationary_multivariate_gaussian_process_amd.hadamard import cohort_buckets
    sizes = cc.nobs(cc.SET_A)
    # sorted: 128 (0), 127 (5), 65 (4), 64 (3), 63 (1), 2 (2).  3 * 128^3 = 6291456 <= 1.5 * (128^3 + 127^3 + 65^3) = 6630240, but
    # 4 * 128^3 = 8388608 > 1.5 * 4682304 = 7023456; 2 * 64^3 = 524288 <= 1.5 * 512191 = 768286.5, but 3 * 64^3 = 786432 > 768298.5
    got = cohort_buckets(sizes, 0.5)
    assert [b.tolist() for b in got] == [[0, 5, 4], [3, 1], [2]]
    assert [b.tolist() for b in cohort_buckets(sizes)] == [b.tolist() for b in got]           # the default
    check_buckets(sizes, 0.5, got)
    rng = np.random.default_rng(7)
    big = rng.integers(1, 1025, size=40).tolist() + [512, 512, 512]
    for w in (0.0, 0.1, 0.5, 3.0, 1e9):
        b = cohort_buckets(big, w)
        check_buckets(big, w, b)
        assert [v.tolist() for v in cohort_buckets(big, w)] == [v.tolist() for v in b]        # deterministic
        if w == 0.0:
            assert all(len({big[int(s)] for s in v}) == 1 for v in b) and len(b) == len(set(big))
        if w == 1e9:
            assert len(b) == 1
    # the same buckets, as lists of sizes, whatever the input order of equal sizes; within a bucket ties are ordered by index
    sizes = [64, 100, 100, 64, 64]
    a = cohort_buckets(sizes, 0.2)
    assert [v.tolist() for v in a] == [[1, 2], [0, 3, 4]]
    perm = [3, 0, 4, 2, 1]                             # a real permutation: [64, 64, 64, 100, 100]
    shuffled = [sizes[i] for i in perm]
    assert shuffled != sizes
    p = cohort_buckets(shuffled, 0.2)
    assert [v.tolist() for v in p] == [[3, 4], [0, 1, 2]]
    assert [[shuffled[i] for i in v] for v in p] == [[sizes[i] for i in v] for v in a]
    assert [sorted(perm[i] for i in v) for v in p] == [v.tolist() for v in a]          # mapped back: the same subjects
    with pytest.raises(ValueError):
        cohort_buckets([3, 0], 0.5)
