"""CPU half of the Hadamard sweep (tests/hadamard_cases.py): the NumPy restatements of the three Hadamard models are pinned to the
reference's recorded runs at the fixtures' shapes only, so before tests/test_gpu_hadamard_sweep.py holds the kernels to them at
M = 1..8, at the tile edges and under four more label layouts, this file checks them there against central differences of their own
values, and asserts the conditions the GPU half's bars rely on.

Bars.  Directional derivative against central differences (eps = 1e-5): 1e-5 relative, the bar of test_headline_size_properties for the
same kind of check (achieved: <= 1.2e-6, nonseparable model at N = 193, M = 8 with the priors; <= 1.8e-8 without them; the
difference quotient limits it).  cond(S) < 1e4: with it cond(S) N eps stays
below the likelihood's 1e-10 bar of the GPU half.  Every predictive variance before the clip exceeds sigma2_err: the clip to 1e-6 plays
no part in any comparison."""
import numpy as np
import pytest
from scipy.linalg import LinAlgError, cholesky

import hadamard_cases as hc

EPS, FD_TOL, COND_MAX = 1e-5, 1e-5, 1e4
ALL_SUBJECTS = hc.CASES + [hc.WIDE, hc.MINOR]


def test_case_table():
    # M = 3 and 4 are the fixtures' (had_N77_M3, had_N200_M4 and their twins); the table adds the six instantiations they leave out
    assert len(hc.CASES) == 10 and sorted({M for _, M, _ in hc.CASES}) == [1, 2, 5, 6, 7, 8] and hc.WIDE[1] == hc.MINOR[1] == 3
    assert {lay for _, _, lay in hc.CASES} == set(hc.LAYOUTS)
    assert {N for N, _, _ in hc.CASES} >= {63, 64, 65, 128, 129} and sum(N == M for N, M, _ in hc.CASES) == 4
    N, M, _ = hc.WIDE
    assert (N // M) * M > 256


@pytest.mark.parametrize("case", ALL_SUBJECTS, ids=hc.case_id)
def test_subject_meets_the_preconditions(case):
    N, M, layout = case
    c = hc.build(case)
    x, indx = c["x"], c["indx"]
    assert indx.dtype == np.int32 and sorted(np.unique(indx).tolist()) == list(range(M))          # nmgp_had_set_data requires it
    assert N < 4 or np.any(np.diff(np.sort(x)) == 0.0)                                            # the repeated time stamp
    assert (layout == "unsorted") == bool(N > 1 and np.any(np.diff(x) < 0))
    if layout == "blocks":
        assert np.all(np.diff(indx) >= 0)
    if layout == "rare_last":
        assert indx[-1] == M - 1 and (indx == M - 1).sum() == 1
    if layout == "rare_first":
        assert indx[0] == 0 and (indx == 0).sum() == 1
    L = np.zeros((M, M))
    L[np.tril_indices(M)] = c["L_vec"]
    assert M == 1 or not np.allclose(L @ L.T, (L @ L.T)[::-1, ::-1])                               # asymmetric in the outputs
    for model in hc.MODELS:
        P = c["pars"][model]
        assert P.shape[0] == 2 and not np.array_equal(P[0], P[1])
        for k in (0, 1):
            cond = np.linalg.cond(hc.ref_covariance(model, P[k], c))
            assert cond < COND_MAX, (model, k, cond)


def direction(model, c, smooth):
    """A unit direction: random on the scalar slots (smooth=False), smooth in x on every curve block either way -- a rough direction
    on a curve under its GP prior has a derivative of size 1e6, of which the difference quotient keeps no digit."""
    N, T, x = c["N"], c["T"], c["x"]
    P = c["pars"][model].shape[1]
    rng = np.random.default_rng(P)
    v = np.sin(0.7 + np.arange(P)) if smooth else rng.standard_normal(P)
    v /= np.linalg.norm(v)
    if model != "sta":
        v[:N] = 0.05 * np.sin(3.0 * x + 0.3)
        if model == "sep":
            v[N:2 * N] = 0.05 * np.cos(2.0 * x)
        else:
            v[N:N + N * T] = (0.05 * np.cos(2.0 * x[:, None] + 0.1 * np.arange(T)[None, :])).reshape(-1)
    return v


@pytest.mark.parametrize("model", hc.MODELS)
@pytest.mark.parametrize("case", hc.CASES + [hc.WIDE], ids=hc.case_id)
def test_restated_gradient_meets_central_differences(case, model):
    c = hc.build(case)
    p = c["pars"][model][1]
    for prior in (False, True):
        v = direction(model, c, smooth=prior)
        g = hc.ref_logpos(model, p, c, prior, grad=True)[1]
        fd = (hc.ref_logpos(model, p + EPS * v, c, prior)[0] - hc.ref_logpos(model, p - EPS * v, c, prior)[0]) / (2.0 * EPS)
        err = abs(fd - g @ v) / abs(fd)
        print(hc.case_id(case), model, "prior", prior, "directional derivative", fd, "relative error", err)
        assert err < FD_TOL, (model, prior, err)


@pytest.mark.parametrize("case", hc.CASES, ids=hc.case_id)
def test_no_predictive_variance_comes_near_the_clip(case):
    c = hc.build(case)
    N, M = c["N"], c["M"]
    pred = hc.predictions(case)
    S = pred["xs"].shape[0]
    assert S == (2 * (N // M) + 1 if N < 64 else 11) and pred["xs"][1] == c["x"][0]
    assert N >= 64 or (S > 2 * max(1, N // M) and S <= 3 * max(1, N // M))                       # three full-form slices, the last ragged
    floor = hc.raw_variance_floor(pred, c)
    print(hc.case_id(case), "min variance / sigma2_err", floor)
    assert floor > 1.0


def test_no_predictive_variance_comes_near_the_clip_in_the_wide_slices():
    c = hc.build(hc.WIDE)
    N, M = c["N"], c["M"]
    full, ix = hc.predictions(hc.WIDE, **hc.WIDE_FULL), hc.predictions(hc.WIDE, **hc.WIDE_INDEXED)
    assert N // M == 107 and full["xs"].shape[0] == 110 and ix["xs"].shape[0] == 330                # 321 riding rows, then 3 / 9
    assert sorted(set(ix["lab"].tolist())) == [0, 1, 2]
    floor = min(hc.raw_variance_floor(full, c), hc.raw_variance_floor(ix, c))
    print("wide slices: min variance / sigma2_err", floor)
    assert floor > 1.0


@pytest.mark.parametrize("model", hc.MODELS)
def test_the_bad_chain_fails_at_the_third_leading_minor(model):
    """sigma2_err = exp(-800) is 0 exactly and row / column 2 of S are exactly 0: the third pivot is exactly 0, LAPACK's rule is
    pivot <= 0, and SciPy names the minor."""
    c = hc.build(hc.MINOR)
    P = hc.minor_chains(model)
    assert np.all(np.isfinite(P)) and np.exp(P[1, -1]) == 0.0
    S = hc.ref_covariance(model, P[1], c)
    assert np.all(S[2] == 0.0) and np.all(S[:, 2] == 0.0) and S[0, 0] > 0.0 and S[0, 0] * S[1, 1] - S[1, 0] ** 2 > 0.0
    with pytest.raises(LinAlgError, match="3-th leading minor"):
        cholesky(S, lower=True)
    for k in (0, 2):
        cholesky(hc.ref_covariance(model, P[k], c), lower=True)
