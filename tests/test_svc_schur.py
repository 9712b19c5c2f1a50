"""The structured value path of the batched nonseparable evaluation (NMGP_SVC_SCHUR): output 0 of Sigma eliminated in closed
form.  CPU part: the algorithm restated in NumPy against the oracle's dense Cholesky log likelihood.  GPU part: the structured
batch against the dense one (NMGP_SVC_SCHUR=0) of the same build, which the parity tests tie to the reference."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import SVC_KEYS, golden, golden_names, hyper_dict, relerr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JITTER = 1e-6


def _unpack(pars, N, M):
    T = M * (M + 1) // 2
    ell = np.exp(pars[:N])
    Lv = pars[N:N + N * T].reshape(N, T).copy()
    r, c = np.tril_indices(M)
    L = np.zeros((N, M, M))
    L[:, r, c] = Lv
    idx = np.arange(M)
    L[:, idx, idx] = np.exp(L[:, idx, idx])
    return ell, L, float(np.exp(pars[-1]))


def _gibbs(x, ell):
    li2 = ell[:, None] ** 2 + ell[None, :] ** 2
    dist = (x[:, None] ** 2 + x[None, :] ** 2) - 2.0 * (x[:, None] * x[None, :])
    K = np.sqrt(2.0 * (ell[:, None] * ell[None, :]) / li2) * np.exp(-dist / li2)
    return K + JITTER * np.eye(x.shape[0])


def schur_loglik(pars, Y, x):
    """-1/2 log det Sigma - 1/2 y^T Sigma^-1 y by the structured algorithm (nmgp_kernels.hip, k_svc_schur_cov)."""
    Y = np.asarray(Y, dtype=np.float64)
    N, M = Y.shape
    ell, L, s2 = _unpack(np.asarray(pars, dtype=np.float64), N, M)
    Kx = _gibbs(np.asarray(x, dtype=np.float64), ell)
    l00 = L[:, 0, 0]
    E = s2 / l00 ** 2
    v = Y[:, 0] / l00
    LA = np.linalg.cholesky(Kx + np.diag(E))
    w = np.linalg.solve(LA, v)
    X = np.linalg.inv(LA)                      # L_A^-1: A^-1 = X^T X
    Ainv = X.T @ X
    u = Ainv @ v
    g = s2 * L[:, 1:, 0] / l00[:, None] ** 2   # [N, M-1]
    n1 = (M - 1) * N
    S = np.empty((n1, n1))
    for a in range(1, M):
        for b in range(1, M):
            B = (L[:, a, 1:min(a, b) + 1] @ L[:, b, 1:min(a, b) + 1].T)
            blk = Kx * B - np.outer(g[:, a - 1], g[:, b - 1]) * Ainv
            blk[np.diag_indices(N)] += s2 * ((1.0 if a == b else 0.0) + L[:, a, 0] * L[:, b, 0] / l00 ** 2)
            S[(a - 1) * N:a * N, (b - 1) * N:b * N] = blk
    yp = (Y[:, 1:] - L[:, 1:, 0] * (v - E * u)[:, None]).T.reshape(-1)
    LS = np.linalg.cholesky(S)
    wp = np.linalg.solve(LS, yp)
    logdet = 2.0 * np.sum(np.log(l00)) + 2.0 * np.sum(np.log(np.diag(LA))) + 2.0 * np.sum(np.log(np.diag(LS)))
    quad = w @ w + wp @ wp
    return -0.5 * logdet - 0.5 * quad          # (the oracle's loglik term: no 2 pi constant)


def _oracle_loglik(pars, Y, x, hyper):
    from oracle import nmgp_oracle as O
    return O.nlogpos_obj_SVC(pars, Y, x, **hyper, verbose=True)[1]


def _m2_goldens():
    out = []
    for name in golden_names("svc_"):
        g = golden(name)
        if np.asarray(g["Y"]).shape[1] >= 2:
            out.append(name)
    return out


@pytest.mark.parametrize("name", _m2_goldens())
def test_schur_restatement_matches_oracle_on_goldens(name):
    g = golden(name)
    hyper = hyper_dict(g["hyper"], SVC_KEYS)
    ref = _oracle_loglik(g["pars"], g["Y"], g["x"], hyper)
    assert relerr(schur_loglik(g["pars"], g["Y"], g["x"]), ref) < 1e-12


@pytest.mark.parametrize("M", [2, 3, 4, 5])
@pytest.mark.parametrize("diag", [-5.0, 5.0])
def test_schur_restatement_matches_oracle_on_extreme_parameters(M, diag):
    rng = np.random.default_rng(40 + M + int(diag))
    N = 48
    T = M * (M + 1) // 2
    x = np.sort(rng.uniform(0.0, 10.0, N))
    Y = rng.normal(size=(N, M))
    uL = rng.normal(scale=5.0, size=(N, T))
    r, c = np.tril_indices(M)
    uL[:, r == c] = diag + rng.normal(scale=0.3, size=(N, M))
    pars = np.concatenate([rng.normal(scale=0.5, size=N), uL.reshape(-1), [-9.0]])
    hyper = dict(zip(SVC_KEYS, [0.0, 5.0, 1.0, 0.0, 5.0, 1.0, 1.0, 1.0]))
    ref = _oracle_loglik(pars, Y, x, hyper)
    assert relerr(schur_loglik(pars, Y, x), ref) < 1e-9


# ---- GPU: structured batch against the dense batch ----------------------------------------------------------------------


def _batch(mode, x, Y, pars, hv, subjects=None, cps=1, prior=True):
    """One batched value evaluation in a fresh context created under NMGP_SVC_SCHUR=mode (read at context creation)."""
    from nonstationary_multivariate_gaussian_process_amd import _lib
    old = os.environ.get("NMGP_SVC_SCHUR")
    os.environ["NMGP_SVC_SCHUR"] = str(mode)
    try:
        ctx = _lib.Context(0)
    finally:
        if old is None:
            del os.environ["NMGP_SVC_SCHUR"]
        else:
            os.environ["NMGP_SVC_SCHUR"] = old
    try:
        ctx.set_data(x, Y)
        ctx.svc_batch_alloc(pars.shape[0])
        if subjects is not None:
            ctx.svc_batch_set_subjects(subjects[0], subjects[1], cps)
        ctx.svc_batch_set_pars(pars)
        ctx.svc_batch_eval(hv, prior)
        return ctx.svc_batch_fetch()
    finally:
        ctx.close()


def _hv():
    from nonstationary_multivariate_gaussian_process_amd import sim
    return [sim.HYPER_SVC[k] for k in SVC_KEYS]


def _chains(N, M, B, seed):
    from nonstationary_multivariate_gaussian_process_amd import sim
    d = sim.simulate_nonseparable(N, M, seed=seed)
    pars = np.stack([sim.perturb(d["pars_true"], 0.05, 0.2 + 0.11 * k) for k in range(B)])
    return d, pars


@pytest.mark.gpu
@pytest.mark.parametrize("N,M,B", [(256, 2, 6), (256, 3, 6), (128, 4, 4), (192, 5, 3), (213, 4, 5), (1566, 4, 2)])
def test_structured_batch_matches_dense(N, M, B):
    d, pars = _chains(N, M, B, seed=300 + N + M)
    hv = _hv()
    o1, s1 = _batch(1, d["x"], d["Y"], pars, hv)
    o0, s0 = _batch(0, d["x"], d["Y"], pars, hv)
    assert np.all(s0 == 0) and np.all(s1 == 0) and np.all(np.isfinite(o1))
    assert relerr(o1[:, 1], o0[:, 1]) < 1e-11, (o1[:, 1], o0[:, 1])
    assert relerr(o1, o0) < 1e-9


@pytest.mark.gpu
def test_structured_multi_subject_batch_with_several_chains_per_subject():
    from nonstationary_multivariate_gaussian_process_amd import sim
    N, M, S, K = 320, 3, 3, 2
    subs = [sim.simulate_nonseparable(N, M, seed=700 + s) for s in range(S)]
    pars = np.stack([sim.perturb(d["pars_true"], 0.05, 0.3 + 0.2 * k) for d in subs for k in range(K)])
    xs = np.stack([d["x"] for d in subs])
    Ys = np.stack([d["Y"] for d in subs])
    hv = _hv()
    o1, s1 = _batch(1, subs[0]["x"], subs[0]["Y"], pars, hv, subjects=(xs, Ys), cps=K)
    o0, s0 = _batch(0, subs[0]["x"], subs[0]["Y"], pars, hv, subjects=(xs, Ys), cps=K)
    assert np.all(s0 == 0) and np.all(s1 == 0)
    assert relerr(o1[:, 1], o0[:, 1]) < 1e-11 and relerr(o1, o0) < 1e-9
    # chains of different subjects really see different data
    assert abs(o1[0, 1] - o1[K, 1]) > 1e-3 * abs(o1[0, 1])


@pytest.mark.gpu
def test_structured_status_matches_dense_on_failed_chains():
    """A chain whose Sigma cannot be factored gets the dense path's status: the first failing leading minor of Sigma, from A's
    factorisation (output 0) or N + that of the Schur complement (outputs 1..M-1)."""
    N, M, B = 256, 3, 4
    T = M * (M + 1) // 2
    d, pars = _chains(N, M, B, seed=911)
    pars[1, -1] = np.nan                      # sigma2: every entry of Sigma undefined
    pars[2, N + 5 * T + 2] = np.nan           # L_5[1, 1]: only the output-1 rows of location 5 (and below)
    hv = _hv()
    o1, s1 = _batch(1, d["x"], d["Y"], pars, hv)
    o0, s0 = _batch(0, d["x"], d["Y"], pars, hv)
    assert s0[0] == 0 and s0[3] == 0 and s0[1] != 0 and s0[2] != 0
    assert np.array_equal(s1, s0), (s1, s0)
    assert s0[2] > N
    assert relerr(o1[[0, 3]], o0[[0, 3]]) < 1e-9


@pytest.mark.gpu
def test_structured_headline_batch_against_golden():
    """The configuration bench.py times, on the structured path: chain 0 at the golden parameters against the reference's
    value, every chain against the dense batch."""
    from nonstationary_multivariate_gaussian_process_amd import sim
    g = golden("svc_sim_N2048_M3_base")
    B = 128
    pars = np.stack([sim.perturb(g["pars"], 0.002 * k, 0.37 * k) for k in range(B)])
    pars[0] = g["pars"]
    o1, s1 = _batch(1, g["x"], g["Y"], pars, g["hyper"])
    assert np.all(s1 == 0) and np.all(np.isfinite(o1))
    assert relerr(o1[0], g["out"]) < 1e-6 and relerr(o1[0][1], g["out"][1]) < 1e-9
    o0, s0 = _batch(0, g["x"], g["Y"], pars, g["hyper"])
    assert np.all(s0 == 0)
    # the headline parity test's chains at its tolerance; every chain at the value tolerance (the strongly perturbed chains have
    # log likelihoods near zero, so that both paths' rounding of log det ~ -3e4 shows as ~1e-10 relative there)
    assert relerr(o1[[1, 63, 127], 1], o0[[1, 63, 127], 1]) < 1e-11
    assert relerr(o1[:, 1], o0[:, 1]) < 1e-9 and relerr(o1, o0) < 1e-9


POISON_SNIPPET = r"""
import sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import numpy as np
import test_svc_schur as t
for N, M, B in ((213, 3, 3), (256, 2, 4)):
    d, pars = t._chains(N, M, B, seed=50 + N)
    o1, s1 = t._batch(1, d["x"], d["Y"], pars, t._hv())
    o0, s0 = t._batch(0, d["x"], d["Y"], pars, t._hv())
    assert np.all(s1 == 0) and np.all(s0 == 0) and np.all(np.isfinite(o1)), (s1, s0, o1)
    assert t.relerr(o1[:, 1], o0[:, 1]) < 1e-11 and t.relerr(o1, o0) < 1e-9, (o1, o0)
print("POISON_OK")
"""


@pytest.mark.gpu
def test_structured_batch_under_poison():
    """NMGP_POISON=1 (read once per process: a child) fills fresh buffers with NaNs: the structured path reads nothing unwritten."""
    env = dict(os.environ)
    env["NMGP_POISON"] = "1"
    out = subprocess.run([sys.executable, "-c", POISON_SNIPPET % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}],
                         capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0 and "POISON_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
