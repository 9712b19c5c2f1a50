"""CPU half of the batched stationary (LMC) objective (no GPU needed): the oracle that the GPU half is held to is checked against
central differences on the shared subjects; the lock-step drivers BatchedMAPStationary / BatchedHMCStationary run against a NumPy
stand-in for the context (Adam's rows, the frozen tilde_sigma, the shape errors, per-chain random streams); and the new entry is
declared in include/nmgp.h, exported by the built library and bound by the ctypes table."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import sta_batch_cases as C
from conftest import ROOT, vec_relerr

HEADER = os.path.join(ROOT, "include", "nmgp.h")
DECL = (r"int\s+nmgp_sta_batch_eval\s*\(\s*nmgp_ctx\s*\*\s*\w+,\s*const\s+double\s*\*\s*pars,\s*int\s+B,\s*const\s+double\s+hyper\[5\],"
        r"\s*int\s+prior,\s*double\s*\*\s*out5,\s*double\s*\*\s*grad,\s*int\s*\*\s*status\s*\)\s*;")


# ---- the reference of the GPU half --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", C.FD_SHAPES, ids=C.case_id)
@pytest.mark.parametrize("prior", [True, False], ids=["prior", "likelihood"])
def test_oracle_gradient_against_central_differences(shape, prior):
    """Central differences with h = 1e-5 on every one of the T + 3 parameters of chain 0.  Their own error: truncation h^2 f''' / 6
    ~ 1e-10 |g| and rounding eps |f| / h ~ 1e-16 * 1e3 / 1e-5 = 1e-8 per component against |g| >= 1: 1e-6 in ||d|| / ||g|| is a
    hundred times that."""
    from oracle import nmgp_oracle as O
    N, M = shape
    x, Y, _ = C.subject(N, M)
    p = C.chains(N, M)[0]
    g = C.oracle(N, M, prior)[1][0]

    def f(q):
        return float(O.nlogpos_obj_S(q, Y, x, **C.HYPER, verbose=False, Prior=prior))

    h = 1e-5
    fd = np.zeros_like(p)
    for k in range(p.shape[0]):
        e = np.zeros_like(p)
        e[k] = h
        fd[k] = (f(p + e) - f(p - e)) / (2 * h)
    err = vec_relerr(fd, g)
    print("%s prior=%s: central differences vs oracle gradient %.3g" % (C.case_id(shape), prior, err))
    assert err < 1e-6, (err, fd, g)


def test_shared_cases_cover_what_they_claim():
    Ns, Ms = [s[0] for s in C.SHAPES], [s[1] for s in C.SHAPES]
    assert sorted(set(Ms)) == list(range(1, 9))                              # every M instantiation
    assert any(n % 2 for n in Ns) and any(n % 2 == 0 for n in Ns)            # both block-build kernels
    assert {63, 64, 65, 127, 128, 129} <= set(Ns) and max(Ns) > 256
    x, Y, _ = C.subject(*C.UNSORTED, unsorted=True)
    assert np.any(np.diff(x) < 0) and np.std(np.diff(np.sort(x))) > 0
    out, grad = C.oracle(8, 8, True)
    assert out.shape == (C.B_CHAINS, 5) and grad.shape == (C.B_CHAINS, 8 * 9 // 2 + 3) and not out.flags.writeable
    assert C.oracle(8, 8, False)[0].shape == (C.B_CHAINS, 1)


# ---- drivers against a NumPy stand-in -----------------------------------------------------------------------------------------------
def test_batched_map_stationary_rows_are_adam_with_tilde_sigma_frozen():
    """Every row follows torch.optim.Adam over (tilde_l, uL_vec, tilde_sigma2_err) on the oracle's gradient -- map_stationary's loop --
    to 1e-12 (LockStepMAP's promise), tilde_sigma keeps its bits, and a row of a 3-restart run equals the 1-restart run bit for bit."""
    import torch
    from nonstationary_multivariate_gaussian_process_amd.drivers import BatchedMAPStationary, LockStepMAP
    from oracle import nmgp_oracle as O
    N, M, steps = 8, 2, 12
    x, Y, _ = C.subject(N, M)
    P0 = np.array(C.chains(N, M, 3))
    m = BatchedMAPStationary(x, Y, C.HYPER, P0, ctx=C.NumpyStaContext())
    assert isinstance(m, LockStepMAP) and m.lr == 1e-1
    pars, hist, alive = m.run(steps)
    assert np.all(alive) and hist.shape == (steps, 3)
    assert np.array_equal(pars[:, 1], P0[:, 1])                              # tilde_sigma: untouched, bit for bit
    assert not np.any(pars[:, [0, 2, -1]] == P0[:, [0, 2, -1]])
    for b in range(3):
        one = BatchedMAPStationary(x, Y, C.HYPER, P0[b:b + 1], ctx=C.NumpyStaContext()).run(steps)
        assert np.array_equal(one[0][0], pars[b]) and np.array_equal(one[1][:, 0], hist[:, b])
    free = [0] + list(range(2, P0.shape[1]))
    q = torch.from_numpy(P0[1][free].copy()).requires_grad_(True)
    opt = torch.optim.Adam([q], lr=1e-1)
    for i in range(steps):
        full = P0[1].copy()
        full[free] = q.detach().numpy()
        r, g = O.nlogpos_obj_S(full, Y, x, **C.HYPER, verbose=True, grad=True)
        assert abs(-r[0] - hist[i, 1]) <= 1e-12 * abs(r[0])
        opt.zero_grad()
        q.grad = torch.from_numpy(g[free].copy())
        opt.step()
    assert np.allclose(q.detach().numpy(), pars[1][free], rtol=1e-12, atol=1e-12)
    # fix_tilde_sigma=False lets the column move
    free_run = BatchedMAPStationary(x, Y, C.HYPER, P0, ctx=C.NumpyStaContext(), fix_tilde_sigma=False).run(2)
    assert not np.any(free_run[0][:, 1] == P0[:, 1])


def test_batched_map_stationary_subject_form_and_shape_errors():
    from nonstationary_multivariate_gaussian_process_amd.drivers import BatchedMAPStationary
    N, M = 8, 2
    x0, Y0, _ = C.subject(N, M)
    x1, Y1, _ = C.subject(N, M, unsorted=True)
    xs, Ys = np.stack([x0, x1]), np.stack([Y0, Y1])
    P0 = np.array(C.chains(N, M, 4))
    ctx = C.NumpyStaContext()
    m = BatchedMAPStationary(xs, Ys, C.HYPER, P0, ctx=ctx, chains_per_subject=2)
    assert ctx.set is not None and ctx.set[2] == 2
    pars, hist, alive = m.run(3)
    # rows 2, 3 are restarts of subject 1: the same rows on that subject alone
    alone = BatchedMAPStationary(x1, Y1, C.HYPER, P0[2:], ctx=C.NumpyStaContext()).run(3)
    assert np.array_equal(alone[0], pars[2:]) and np.array_equal(alone[1], hist[:, 2:])
    with pytest.raises(ValueError):
        BatchedMAPStationary(xs, Ys, C.HYPER, P0[:3], ctx=C.NumpyStaContext(), chains_per_subject=2)      # B != S * k
    with pytest.raises(ValueError):
        BatchedMAPStationary(xs, Ys[:, :, :1], C.HYPER, P0, ctx=C.NumpyStaContext(), chains_per_subject=2)  # T + 3 does not fit M
    with pytest.raises(ValueError):
        BatchedMAPStationary(x0, Ys, C.HYPER, P0, ctx=C.NumpyStaContext())                                 # xs [N] needs Ys [N, M]
    with pytest.raises(ValueError):
        BatchedMAPStationary(x0, Y0, C.HYPER, P0[0], ctx=C.NumpyStaContext())                              # init_pars must be [B, P]


def test_batched_hmc_stationary_chain_b_is_the_one_chain_run_with_seed_plus_b():
    """Dense mass: chain b of 3 reproduces the one-chain run with seed + b bit for bit (per-chain matrix-vector products), and the
    prior-factor metrics are refused."""
    from nonstationary_multivariate_gaussian_process_amd import drivers as D
    N, M, iters = 8, 2, 3
    x, Y, _ = C.subject(N, M)
    q0 = np.array(C.chains(N, M, 3))
    P = q0.shape[1]
    A = np.random.default_rng(5).standard_normal((P, P))
    mass = A @ A.T / P + np.eye(P)
    kw = dict(step_size=5e-3, num_steps_in_leap=4)
    s3, i3 = D.BatchedHMCStationary(x, Y, C.HYPER, q0, seed=11, ctx=C.NumpyStaContext(), M=mass, **kw).run(iters)
    assert s3.shape == (iters, 3, P) and np.all(np.isfinite(s3))
    for b in range(3):
        s1, i1 = D.BatchedHMCStationary(x, Y, C.HYPER, q0[b:b + 1], seed=11 + b, ctx=C.NumpyStaContext(), M=mass, **kw).run(iters)
        assert np.array_equal(s1[:, 0], s3[:, b]) and i1["accept_rate"][0] == i3["accept_rate"][b]
    assert issubclass(D.BatchedHMCStationary, D.LockStepHMC)
    metric = D.SeparablePriorMetric.__new__(D.SeparablePriorMetric)
    metric.P = P
    with pytest.raises(NotImplementedError):
        D.BatchedHMCStationary(x, Y, C.HYPER, q0, seed=1, ctx=C.NumpyStaContext(), M=metric)
    with pytest.raises(ValueError):
        D.BatchedHMCStationary(np.stack([x, x]), np.stack([Y, Y]), C.HYPER, q0, seed=1, ctx=C.NumpyStaContext())   # 3 chains, 2 subjects
    with pytest.raises(ValueError):
        D.BatchedHMCStationary(x, Y[:, :1], C.HYPER, q0, seed=1, ctx=C.NumpyStaContext())                            # T + 3 does not fit M
    ctx = C.NumpyStaContext()
    D.BatchedHMCStationary(np.stack([x, x]), np.stack([Y, Y]), C.HYPER, np.concatenate([q0, q0[:1]]), seed=1, ctx=ctx)
    assert ctx.set is not None and ctx.set[2] == 2


def test_python_layers_expose_the_stationary_batch():
    from nonstationary_multivariate_gaussian_process_amd import _lib, drivers
    sig = inspect.signature(_lib.Context.sta_batch_eval)
    assert list(sig.parameters) == ["self", "pars", "hyper", "prior", "want_grad"]
    assert sig.parameters["prior"].default is True and sig.parameters["want_grad"].default is False
    assert list(inspect.signature(_lib.Context.sta_batch_set_subjects).parameters) == ["self", "xs", "Ys", "chains_per_subject"]
    assert list(inspect.signature(_lib.Context.sta_batch_clear_subjects).parameters) == ["self"]
    sig = inspect.signature(drivers.BatchedMAPStationary.__init__)
    assert list(sig.parameters) == ["self", "xs", "Ys", "hyper_pars", "init_pars", "lr", "ctx", "chains_per_subject", "fix_tilde_sigma"]
    assert sig.parameters["lr"].default == 1e-1 and sig.parameters["fix_tilde_sigma"].default is True
    sig = inspect.signature(drivers.BatchedHMCStationary.__init__)
    assert list(sig.parameters) == ["self", "x", "Y", "hyper_pars", "init_positions", "step_size", "num_steps_in_leap", "seed", "ctx", "M",
                                    "Minv"]
    sig = inspect.signature(drivers.posterior_predict_stationary)
    assert list(sig.parameters) == ["x", "Y", "hyper_pars", "samples", "xs", "draws", "seed", "ctx"]


# ---- the C surface ------------------------------------------------------------------------------------------------------------------
def test_entry_is_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(DECL, src), "nmgp_sta_batch_eval is not declared in nmgp.h with the documented signature"
    from nonstationary_multivariate_gaussian_process_amd import build as b, _lib
    lib_path = b.build(verbose=False)
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib_path]).decode()
    assert "nmgp_sta_batch_eval" in set(re.findall(r" T (nmgp_[a-z0-9_]+)", out))
    I, V, P = ctypes.c_int, ctypes.c_void_p, _lib.c_double_p
    assert _lib.SIGNATURES["nmgp_sta_batch_eval"] == (I, [V, P, I, P, I, P, P, ctypes.POINTER(ctypes.c_int)])
    lib = _lib.load(require_gpu=False)
    # no context: the entry refuses a NULL handle instead of touching it
    assert lib.nmgp_sta_batch_eval(None, None, 1, None, 1, None, None, None) == -1
