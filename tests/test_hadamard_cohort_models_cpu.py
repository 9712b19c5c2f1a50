"""CPU half of the cohort tests of the separable ("sep") and stationary ("sta") Hadamard models (tests/hadamard_cohort_cases.py,
tests/hadamard_cohort_model_cases.py).

1. The subjects the cohort sets add to the sweep's table meet, for both models, what tests/test_hadamard_cohort_cpu.py asserts for the
   nonseparable one: cond(S) below COND_MAX for both chains, the restated gradient within FD_TOL of central differences with and
   without the priors; the two terms of the GPU half's per-block gradient bar and the prior part of the separable gradient, as there.
2. The padded formulations nmgp_hads_subjects_eval / nmgp_hadst_subjects_eval run on the device, restated in NumPy: S, y and (sep) both
   GP-prior covariances padded to Nmax with identity / zero, the trace over the real observations, the label reduction and the adjoint
   sums over the real observations, N_s log 2 pi.  They equal the per-subject restatements on set A: value and likelihood 1e-12
   relative, gradient 1e-10 in ||dg|| / ||g|| (the bars and the chain of comparisons of tests/test_hadamard_cohort_cpu.py).  Each mask
   can bite: with the trace over Nmax the sigma2 slot misses the bar; for sta with the adjoint sums over Nmax the tilde_sigma slot
   does; for sep with an unmasked label reduction on zero-padded labels (and no mask in the adjoint sums) a label-0 slot of L_vec does.
3. hadamard_sep.cohort_pack / cohort_unpack round-trip."""
import math

import numpy as np
import pytest

import hadamard_cases as hc
import hadamard_cohort_cases as cc
import hadamard_cohort_model_cases as mc
from conftest import relerr, vec_relerr
from oracle import nmgp_oracle as oracle
from test_hadamard_cohort_cpu import ELEMENTWISE, GRAD_TOL, LAPACK, VAL_TOL, pad_identity
from test_hadamard_sep_cpu import hsep_covariance, hsep_rows, hsep_split
from test_hadamard_sta_cpu import hsta_covariance, hsta_rows, hsta_split
from test_hadamard_sweep_cpu import COND_MAX, EPS, FD_TOL, direction


# ---- 1. preconditions of the new subjects ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", mc.MODELS)
@pytest.mark.parametrize("case", cc.NEW_SUBJECTS, ids=hc.case_id)
def test_new_subject_meets_the_preconditions(case, model):
    N, M, layout = case
    c = hc.build(case)
    P = c["pars"][model]
    assert P.shape == (2, mc.plen(model, N, M)) and not np.array_equal(P[0], P[1])
    for k in (0, 1):
        cond = np.linalg.cond(hc.ref_covariance(model, P[k], c))
        print(model, hc.case_id(case), "chain", k, "cond", cond)
        assert cond < COND_MAX, (k, cond)
    p = P[1]
    for prior in (False, True):
        v = direction(model, c, smooth=prior)
        g = hc.ref_logpos(model, p, c, prior, grad=True)[1]
        fd = (hc.ref_logpos(model, p + EPS * v, c, prior)[0] - hc.ref_logpos(model, p - EPS * v, c, prior)[0]) / (2.0 * EPS)
        err = abs(fd - g @ v) / abs(fd)
        print(model, hc.case_id(case), "prior", prior, "directional derivative", fd, "relative error", err)
        assert err < FD_TOL, (prior, err)


@pytest.mark.parametrize("model", mc.MODELS)
@pytest.mark.parametrize("name", sorted(cc.ALL_SETS))
def test_block_bars_rest_on_two_cpu_references(name, model):
    """tests/test_hadamard_cohort_cpu.py's test of the same name for the two models: d_cpu (sta: with the priors too) below
    GRAD_TIGHT / 10, both terms of the GPU half's per-block bar printed."""
    Nmax = max(cc.nobs(cc.ALL_SETS[name]))
    for case in cc.ALL_SETS[name]:
        d, stable = hc.block_bar_terms(model, case, Nmax)
        print("set", name, hc.case_id(case), model, "d_cpu", d, "N cond(S) eps", stable, "bar", hc.block_bar(model, case, Nmax))
        assert d < hc.GRAD_TIGHT / 10, (case, d)
        assert 0.0 < hc.block_bar(model, case, Nmax) <= hc.GRAD_TIGHT


@pytest.mark.parametrize("name", sorted(cc.ALL_SETS))
def test_prior_part_is_determined_block_by_block(name):
    """sep: g(prior) - g(no prior) of the restatement alone against the padded formulation at the set's Nmax, two LAPACK blockings of
    the prior factors: per block below PRIOR_PART_REFERENCE = 1e-7 (sta has no GP prior: its gradient with the priors is held to the
    tight bar whole)."""
    Nmax, worst = max(cc.nobs(cc.ALL_SETS[name])), 0.0
    for case in cc.ALL_SETS[name]:
        for k in (0, 1):
            tab = hc.block_table(hc.prior_part("sep", case, k, Nmax), hc.prior_part("sep", case, k), "sep", case[0], case[1])
            worst = max(worst, max(tab.values()))
            assert max(tab.values()) < hc.PRIOR_PART_REFERENCE, (case, k, tab)
    print("set", name, "sep prior part, alone against padded: worst block", worst)


# ---- 2. the padded formulations --------------------------------------------------------------------------------------------------------
def padded_data(c, Nmax):
    """x, labels and y as the set holds them: zeros in the padded slots"""
    N = c["N"]
    x, y, indx = np.zeros(Nmax), np.zeros(Nmax), np.zeros(Nmax, dtype=np.int64)
    x[:N], y[:N], indx[:N] = c["x"], c["y"], c["indx"]
    return x, y, indx


def factor_and_inverse(S, yp, N, ops):
    chol, forward, backward = ops
    Nmax = S.shape[0]
    C = chol(S)
    assert np.array_equal(C[N:, N:], np.eye(Nmax - N)) and not np.any(C[N:, :N])      # the padded part of the factor: exactly I | 0
    z = forward(C, yp)
    loglik = -np.log(np.diag(C)).sum() - 0.5 * (z @ z)
    alpha = backward(C, z)
    Sinv = backward(C, forward(C, np.eye(Nmax)))
    assert np.array_equal(alpha[N:], np.zeros(Nmax - N)) and np.array_equal(Sinv[N:, N:], np.eye(Nmax - N)) and not np.any(Sinv[N:, :N])
    return loglik, alpha, Sinv


def padded_sep(pars, c, Nmax, prior, ops=LAPACK, trace_over_nmax=False, unmasked_sums=False):
    """The separable verbose tuple and d NegLog / d pars (the subject's own layout) computed the way the device does it: every matrix
    of order Nmax, padded observations masked.  unmasked_sums: the adjoint sums and the label reduction run over all Nmax rows with
    what a padded row holds on the device (x = 0, label 0, ell = sig = 1) -- the variant the masks exist to prevent."""
    chol, forward, backward = ops
    x, indx, hyper = c["x"], c["indx"].astype(np.int64), c["hyper"]["sep"]
    N, M, T = c["N"], c["M"], c["T"]
    pars = np.asarray(pars, dtype=np.float64)
    tl, ts, Lv, tse = hsep_split(pars, N, M)
    sigma2 = math.exp(tse)
    mu_l, al_l, be_l, mu_s, al_s, be_s, a, b, cc_ = [float(v) for v in hyper[:9]]
    xp, yp, ip = padded_data(c, Nmax)
    loglik, alpha, Sinv = factor_and_inverse(pad_identity(hsep_covariance(pars, x, indx, M), Nmax), yp, N, ops)
    X1 = x.reshape(-1, 1)
    lps, gps = [], []
    for col, mu, al, be in ((tl, mu_l, al_l, be_l), (ts, mu_s, al_s, be_s)):
        Cp = chol(pad_identity(oracle.RBF_cov(X1, alpha=al, beta=be), Nmax))
        assert np.array_equal(Cp[N:, N:], np.eye(Nmax - N)) and not np.any(Cp[N:, :N])
        R = np.zeros(Nmax)
        R[:N] = col - mu                                                            # centred real slots, zeros in the padded ones
        Z = forward(Cp, R)
        assert not np.any(Z[N:])
        lps.append(-0.5 * (N * oracle.LOG_2PI + Z @ Z) - np.log(np.diag(Cp)).sum())   # N_s log 2 pi, not Nmax
        gps.append(backward(Cp, Z)[:N])
    lp_L = float(np.sum(oracle.normal_log_prob(Lv, 0.0, cc_)))
    var = float(np.float32(cc_) * np.float32(cc_))
    lp_s2 = oracle.inverse_gamma_logpdf_u(sigma2, alpha=a, beta=b)
    res = loglik + ((lps[0] + lps[1] + lp_L + lp_s2 + tse) if prior else 0.0)
    out = np.array([-res, loglik, lps[0], lps[1], lp_L, lp_s2])
    n = Nmax if unmasked_sums else N
    ell, sig = np.ones(n), np.ones(n)
    ell[:N], sig[:N] = np.exp(tl), np.exp(ts)
    G = 0.5 * (np.outer(alpha, alpha) - Sinv)[:n, :n]
    lab = ip[:n]
    R = hsep_rows(Lv, lab, M)
    D = oracle.pairwise_distances(xp[:n].reshape(-1, 1))
    A = (ell ** 2)[:, None] + (ell ** 2)[None, :]
    K0 = np.outer(sig, sig) * np.sqrt(2.0 * np.outer(ell, ell) / A) * np.exp(-D / A)
    V = 2.0 * G * K0 * (R @ R.T)
    e2 = (ell ** 2)[:, None]
    W = V * (0.5 - e2 / A + 2.0 * e2 * D / (A * A))
    np.fill_diagonal(W, 0.0)
    dR = 2.0 * (G * (K0 + 1e-6 * np.eye(n))) @ R
    g_L = np.zeros(T)
    for m in range(M):
        g_L[m * (m + 1) // 2: m * (m + 1) // 2 + m + 1] = dR[lab == m, :m + 1].sum(0)
    trace = np.trace(Sinv) if trace_over_nmax else np.trace(Sinv[:N, :N])
    g = np.concatenate([W.sum(1)[:N], V.sum(1)[:N], g_L, [sigma2 * 0.5 * (alpha @ alpha - trace)]])
    if prior:
        g[:N] -= gps[0]
        g[N:2 * N] -= gps[1]
        g[2 * N:2 * N + T] -= Lv / var
        g[-1] += (-a - 1.0) + b / sigma2 + 1.0
    return out, -g


def padded_sta(pars, c, Nmax, prior, ops=LAPACK, trace_over_nmax=False, unmasked_sums=False):
    """The stationary verbose tuple and d NegLog / d pars computed the way the device does it; unmasked_sums as in padded_sep (a
    padded row: x = 0, label 0, G_ii = -1/2)."""
    x, indx, hyper = c["x"], c["indx"].astype(np.int64), c["hyper"]["sta"]
    N, M, T = c["N"], c["M"], c["T"]
    pars = np.asarray(pars, dtype=np.float64)
    tl, ts, Lv, tse = hsta_split(pars, M)
    mu_l, sd_l, a, b, cc_ = [float(v) for v in hyper]
    sigma2 = math.exp(tse)
    xp, yp, ip = padded_data(c, Nmax)
    loglik, alpha, Sinv = factor_and_inverse(pad_identity(hsta_covariance(pars, x, indx, M), Nmax), yp, N, ops)
    lp_l = float(oracle.normal_log_prob(tl, mu_l, sd_l))
    lp_L = float(np.sum(oracle.normal_log_prob(Lv, 0.0, cc_)))
    lp_s2 = oracle.inverse_gamma_logpdf_u(sigma2, alpha=a, beta=b)
    res = loglik + ((lp_l + lp_L + lp_s2 + tse) if prior else 0.0)
    out = np.array([-res, loglik, lp_l, lp_L, lp_s2])
    n = Nmax if unmasked_sums else N
    G = 0.5 * (np.outer(alpha, alpha) - Sinv)[:n, :n]
    lab = ip[:n]
    R = hsta_rows(Lv, lab, M)
    D = oracle.pairwise_distances(xp[:n].reshape(-1, 1) / math.exp(tl))
    E = math.exp(ts) ** 2 * np.exp(-0.5 * D)
    V = G * (R @ R.T) * E
    W = (G * (E + 1e-6 * np.eye(n))) @ R
    g_L = np.zeros(T)
    for m in range(M):
        g_L[m * (m + 1) // 2: m * (m + 1) // 2 + m + 1] = 2.0 * W[lab == m, :m + 1].sum(0)
    trace = np.trace(Sinv) if trace_over_nmax else np.trace(Sinv[:N, :N])
    g = np.concatenate([[(V * D).sum(), 2.0 * V.sum()], g_L, [sigma2 * 0.5 * (alpha @ alpha - trace)]])
    if prior:
        g[0] -= (tl - float(np.float32(mu_l))) / float(np.float32(sd_l) * np.float32(sd_l))
        g[2:2 + T] -= Lv / float(np.float32(cc_) * np.float32(cc_))
        g[-1] += (-a - 1.0) + b / sigma2 + 1.0
    return out, -g


PADDED = {"sep": padded_sep, "sta": padded_sta}


def errors(out, grad, ref_out, ref_grad):
    return dict(value=relerr(out[0], ref_out[0]), loglik=relerr(out[1], ref_out[1]), priors=relerr(out[2:], ref_out[2:]),
                grad=vec_relerr(grad, ref_grad))


def within_the_bars(e):
    return e["value"] < VAL_TOL and e["loglik"] < VAL_TOL and e["priors"] < VAL_TOL and e["grad"] < GRAD_TOL


def slot_misses(bad, ref, slot):
    """the slot is off by far more than the gradient bar, and the whole gradient misses it (the existing test's criterion)"""
    return abs(bad[slot] - ref[slot]) / abs(ref[slot]) > 1e3 * GRAD_TOL and vec_relerr(bad, ref) > GRAD_TOL


@pytest.mark.parametrize("model", mc.MODELS)
@pytest.mark.parametrize("case", cc.SET_A, ids=hc.case_id)
def test_padded_formulation_equals_the_per_subject_restatement(case, model):
    """The three links of tests/test_hadamard_cohort_cpu.py, every quantity with and without the priors:
    a. this file's formulation at Nmax = N_s under LAPACK IS the per-subject restatement hadamard_cases.ref_logpos;
    b. padded to Nmax = 128 against Nmax = N_s, both under the elementwise routines, where padding is a true reordering also for the
       prior factors: the bars, priors included;
    c. padded to 128 under LAPACK against ref_logpos: the bars for the likelihood and the prior-free objective, and for the stationary
       model (no GP prior, cond(S) < 1e4) with the priors too.  For sep with the priors this link compares two blockings of LAPACK's
       factorisation of matrices of condition 1e11: its figures are printed and (a) + (b) carry the check.
    Then the masks, in (b) and (c): each variant without its mask misses the gradient bar in the slot the mask protects."""
    c = hc.build(case)
    padded = PADDED[model]
    N, M, Nmax = c["N"], c["M"], max(cc.nobs(cc.SET_A))
    sigma_slot = {"sep": N + 0, "sta": 1}[model]                  # tilde_sigma of observation 0 / the tilde_sigma slot
    label0_slot = {"sep": 2 * N, "sta": 2}[model]                 # L[0, 0]
    for k in (0, 1):
        p = c["pars"][model][k]
        for prior in (True, False):
            tag = "%s %s chain %d prior %d" % (model, hc.case_id(case), k, prior)
            ref_out, ref_grad = mc.reference(model, case, k, prior)
            ea = errors(*padded(p, c, N, prior), ref_out, ref_grad)
            print(tag, "(a) own formulation, unpadded, against the restatement", ea)
            assert within_the_bars(ea), ea
            alone = padded(p, c, N, prior, ops=ELEMENTWISE)
            out_b, grad_b = padded(p, c, Nmax, prior, ops=ELEMENTWISE)
            eb = errors(out_b, grad_b, *alone)
            print(tag, "(b) padded against unpadded, elementwise routines", eb)
            assert within_the_bars(eb), eb
            out, grad = padded(p, c, Nmax, prior)
            ec = errors(out, grad, ref_out, ref_grad)
            print(tag, "(c) padded under LAPACK against the restatement", ec)
            assert ec["loglik"] < VAL_TOL and ref_out[-1] == out[-1]
            if not prior or model == "sta":
                assert ec["value"] < VAL_TOL and ec["grad"] < GRAD_TOL
            for ops, good, ref in ((ELEMENTWISE, grad_b, alone[1]), (LAPACK, grad, ref_grad)):
                bad = padded(p, c, Nmax, prior, trace_over_nmax=True, ops=ops)[1]
                assert np.array_equal(bad[:-1], good[:-1])
                wide = padded(p, c, Nmax, prior, unmasked_sums=True, ops=ops)[1]
                assert wide[-1] == good[-1]
                if N < Nmax:
                    print(tag, "sigma2 slot with the trace over Nmax", bad[-1], "against", ref[-1])
                    assert slot_misses(bad, ref, -1)
                    print(tag, "unmasked sums: tilde_sigma slot", wide[sigma_slot], "against", ref[sigma_slot], "L[0, 0] slot",
                          wide[label0_slot], "against", ref[label0_slot])
                    assert slot_misses(wide, ref, label0_slot)           # a padded row carries label 0
                    if model == "sta":
                        assert slot_misses(wide, ref, sigma_slot)        # G_ii = -1/2 of every padded i reaches a_s
                    else:                                                # the real per-observation slots only gain exact zeros
                        assert vec_relerr(wide[:2 * N], good[:2 * N]) < GRAD_TOL
                else:
                    assert bad[-1] == good[-1] and np.array_equal(wide, good)      # (Nmax = N_s: the same arrays, the same sums)


# ---- 3. the host helpers ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2])
def test_separable_cohort_pack_and_unpack_round_trip(k):
    from nonstationary_multivariate_gaussian_process_amd import hadamard_sep
    sizes, M, T = cc.nobs(cc.SET_A), 2, 3
    vectors = mc.chains("sep", cc.SET_A, k)
    for Nmax in (None, 130):
        P = hadamard_sep.cohort_pack(vectors, sizes, M, Nmax=Nmax, fill=np.nan)
        N = 128 if Nmax is None else Nmax
        assert P.shape == (len(sizes) * k, 2 * N + T + 1)
        pads = mc.padded_slots("sep", sizes, M, N, k)
        assert np.all(np.isnan(P[pads])) and np.all(np.isfinite(P[~pads])) and pads.sum() == sum((N - n) * 2 * k for n in sizes)
        back = hadamard_sep.cohort_unpack(P, sizes, M, chains_per_subject=k)
        assert len(back) == len(sizes) and all(np.array_equal(u, v) for u, v in zip(back, vectors))
        for s, n in enumerate(sizes):          # the layout itself: two blocks of Nmax, the T shared slots, the last slot
            assert np.array_equal(P[s * k, :n], vectors[s][0, :n]) and np.array_equal(P[s * k, N:N + n], vectors[s][0, n:2 * n])
            assert np.array_equal(P[s * k + k - 1, 2 * N:], vectors[s][k - 1, 2 * n:]) and P[s * k + k - 1, -1] == vectors[s][k - 1, -1]
    if k == 1:                                 # one vector per subject may be given as [P_s]
        flat = hadamard_sep.cohort_pack([v[0] for v in vectors], sizes, M)
        assert np.array_equal(flat, hadamard_sep.cohort_pack(vectors, sizes, M)) and not np.any(flat[mc.padded_slots("sep", sizes, M, 128)])
    with pytest.raises(ValueError):
        hadamard_sep.cohort_pack(vectors, sizes, M, Nmax=127)
    with pytest.raises(ValueError):
        hadamard_sep.cohort_unpack(np.zeros((len(sizes) * k, 2 * 127 + T + 1)), sizes, M, chains_per_subject=k)
