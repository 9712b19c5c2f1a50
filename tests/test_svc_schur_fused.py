"""The structured value path's Sigma' is written by the inverse SYRK's epilogue (k_syrk_schur) and A, v, the pad rows and the seeded
band of L_A^-T by one assembly launch (k_svc_schur_a).  These cases add to tests/test_svc_schur.py what it does not reach: the large
output counts, whose epilogue runs rolled loops (M = 6, 7, 8), on both tile paths of the SYRK (N a multiple of 128 with K a multiple
of 32: the mask-free path; otherwise the masked one), and a multi-subject batch whose N is not a multiple of 128.  Each is compared
with the dense factorisation of the same build (NMGP_SVC_SCHUR=0)."""
import numpy as np
import pytest

from conftest import relerr
from test_svc_schur import _batch, _chains, _hv


@pytest.mark.gpu
@pytest.mark.parametrize("N,M,B", [(256, 6, 3), (200, 6, 3), (128, 7, 2), (256, 8, 2), (150, 8, 2)])
def test_structured_large_M_matches_dense(N, M, B):
    d, pars = _chains(N, M, B, seed=1300 + N + M)
    hv = _hv()
    o1, s1 = _batch(1, d["x"], d["Y"], pars, hv)
    o0, s0 = _batch(0, d["x"], d["Y"], pars, hv)
    assert np.all(s0 == 0) and np.all(s1 == 0) and np.all(np.isfinite(o1))
    assert relerr(o1[:, 1], o0[:, 1]) < 1e-11, (o1[:, 1], o0[:, 1])
    assert relerr(o1, o0) < 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("N,M", [(330, 3), (203, 4)])
def test_structured_multi_subject_ragged_N(N, M):
    from nonstationary_multivariate_gaussian_process_amd import sim
    S, K = 3, 2
    subs = [sim.simulate_nonseparable(N, M, seed=1700 + 10 * s + M) for s in range(S)]
    pars = np.stack([sim.perturb(d["pars_true"], 0.05, 0.3 + 0.2 * k) for d in subs for k in range(K)])
    xs = np.stack([d["x"] for d in subs])
    Ys = np.stack([d["Y"] for d in subs])
    hv = _hv()
    o1, s1 = _batch(1, subs[0]["x"], subs[0]["Y"], pars, hv, subjects=(xs, Ys), cps=K)
    o0, s0 = _batch(0, subs[0]["x"], subs[0]["Y"], pars, hv, subjects=(xs, Ys), cps=K)
    assert np.all(s0 == 0) and np.all(s1 == 0) and np.all(np.isfinite(o1))
    assert relerr(o1[:, 1], o0[:, 1]) < 1e-11 and relerr(o1, o0) < 1e-9
    # chains of different subjects really see different data (far beyond the rounding the comparison above allows)
    assert abs(o1[0, 1] - o1[K, 1]) > 1e-6 * abs(o1[0, 1])
