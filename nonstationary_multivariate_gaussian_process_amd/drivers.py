"""The loops the log-posterior path is called from: MAP by Adam and HMC.

* :func:`map_nonseparable` mirrors ``train()`` of ``Nonseparable_Model/Nonseparable_model.py:147-210``: Adam over the
  three leaves ``[tilde_l | uL_vecs | tilde_sigma2_err]`` (lr 0.2 each), ``NegLog.backward()`` per iteration,
  ``target_value_hist[i] = -NegLog``, and the flat parameter vector pickled as ``MAP.dat`` every 100 iterations.
* :class:`HMCSampler` replaces the reference's EXTERNAL, un-vendored ``HMC_Sampler.HMC_sampler.sampler`` (a sibling
  checkout that is not in the reference tree; call sites ``Nonseparable_model.py:228-231``): same constructor keywords
  as those call sites (``sample_size, potential_func, init_position, step_size, num_steps_in_leap, adaptive_step_size,
  M, duplicate_samples, TensorType, **potential kwargs``) and ``main_hmc_loop() -> (samples [S, P], info)``.  Its
  trajectories cannot be pinned against the reference (the package is absent): it is validated by energy conservation
  and by posterior moments on a Gaussian target (tests/test_drivers.py).

Host-side orchestration only; every evaluation of the potential goes to the GPU through ``Utility.logpos``.
"""
from __future__ import annotations

import pickle
import time

import numpy as np
import torch

from .Utility import logpos, settings

# the hyper-parameter dictionaries' keys, in the order of the C ABI's ``hyper`` vectors: nonseparable, separable, stationary model
SVC_HYPER_KEYS = ("mu_tilde_l", "alpha_tilde_l", "beta_tilde_l", "mu_L", "alpha_L", "beta_L", "a", "b")
SEP_HYPER_KEYS = ("mu_tilde_l", "alpha_tilde_l", "beta_tilde_l", "mu_tilde_sigma", "alpha_tilde_sigma", "beta_tilde_sigma", "a", "b", "c")
STA_HYPER_KEYS = ("mu_tilde_l", "sigma_tilde_l", "a", "b", "c")


def map_nonseparable(x, Y, pars0, hyper_pars, N_opt=1000, lr=2e-1, checkpoint_path=None, checkpoint_every=100,
                     verbose=False, callback=None):
    """MAP estimate of the nonseparable model by Adam; returns (pars [P] ndarray, target_value_hist [N_opt])."""
    x = torch.as_tensor(x, dtype=torch.float64)
    Y = torch.as_tensor(Y, dtype=torch.float64)
    N, M = Y.shape
    T = M * (M + 1) // 2
    p0 = torch.as_tensor(np.asarray(pars0, dtype=np.float64))
    tilde_l = p0[:N].clone().requires_grad_(True)
    uL_vecs = p0[N:N + N * T].clone().requires_grad_(True)
    tilde_sigma2_err = p0[-1:].clone().requires_grad_(True)
    optimizer = torch.optim.Adam([{"params": tilde_l, "lr": lr}, {"params": [uL_vecs, tilde_sigma2_err], "lr": lr}])
    hist = np.zeros(N_opt)

    def flat():
        return torch.cat([tilde_l, uL_vecs, tilde_sigma2_err.view(1)])

    for i in range(N_opt):
        optimizer.zero_grad()
        out = logpos.nlogpos_obj_SVC(flat(), Y, x, **hyper_pars, verbose=True)
        NegLog = out[0]
        NegLog.backward()
        optimizer.step()
        hist[i] = -float(NegLog.detach())
        if verbose:
            print("iter %d: loglik %.6g lp_l %.6g lp_uL %.6g lp_s2 %.6g  -> %.8g" % (
                i, float(out[1]), float(out[2]), float(out[3]), float(out[4]), hist[i]))
        if callback is not None:
            callback(i, hist[i])
        if checkpoint_path and i % checkpoint_every == checkpoint_every - 1:
            with open(checkpoint_path, "wb") as f:          # same on-disk format as the reference's MAP.dat
                pickle.dump(flat().detach().numpy(), f)
    pars = flat().detach().numpy().copy()
    if checkpoint_path:
        with open(checkpoint_path, "wb") as f:
            pickle.dump(pars, f)
    return pars, hist


def map_separable(x, Y, pars0, hyper_pars, N_opt=2000, lr=2e-1, verbose=False):
    """MAP estimate of the separable model by Adam (``Separable_Model/Separable_model.py:147-166``): leaves
    ``[tilde_l | tilde_sigma | uL_vec | tilde_sigma2_err]``, two parameter groups with lr 0.2 each, ``NegLog.backward()`` per
    iteration.  Returns (pars [2N+T+1], target_value_hist [N_opt])."""
    x = torch.as_tensor(x, dtype=torch.float64)
    Y = torch.as_tensor(Y, dtype=torch.float64)
    N, M = Y.shape
    T = M * (M + 1) // 2
    p0 = torch.as_tensor(np.asarray(pars0, dtype=np.float64))
    tilde_l = p0[:N].clone().requires_grad_(True)
    tilde_sigma = p0[N:2 * N].clone().requires_grad_(True)
    uL_vec = p0[2 * N:2 * N + T].clone().requires_grad_(True)
    tilde_sigma2_err = p0[-1:].clone().requires_grad_(True)
    optimizer = torch.optim.Adam([{"params": [tilde_sigma, uL_vec, tilde_sigma2_err], "lr": lr}, {"params": tilde_l, "lr": lr}])
    hist = np.zeros(N_opt)
    for i in range(N_opt):
        optimizer.zero_grad()
        Pars = torch.cat([tilde_l, tilde_sigma, uL_vec, tilde_sigma2_err.view(1)])
        out = logpos.nlogpos_obj(Pars, Y, x, **hyper_pars, verbose=True)
        out[0].backward()
        optimizer.step()
        hist[i] = -float(out[0].detach())
        if verbose and i % 100 == 99:
            print("%d/%d target %.8g" % (i + 1, N_opt, hist[i]))
    return torch.cat([tilde_l, tilde_sigma, uL_vec, tilde_sigma2_err.view(1)]).detach().numpy().copy(), hist


def map_stationary(x, Y, pars0, hyper_pars, N_opt=1000, lr=1e-1, verbose=False):
    """MAP estimate of the stationary (LMC) model by Adam (``Stationary_Model/Stationary_model.py:112-131``): Adam(lr 0.1) over
    ``tilde_l, uL_vec, tilde_sigma2_err``; ``tilde_sigma`` stays at its initial value ("fixed for correlation", :89).  Returns
    (pars [T+3], target_value_hist [N_opt])."""
    x = torch.as_tensor(x, dtype=torch.float64)
    Y = torch.as_tensor(Y, dtype=torch.float64)
    M = Y.shape[1]
    T = M * (M + 1) // 2
    p0 = torch.as_tensor(np.asarray(pars0, dtype=np.float64))
    tilde_l = p0[:1].clone().requires_grad_(True)
    tilde_sigma = p0[1:2].clone()
    uL_vec = p0[2:2 + T].clone().requires_grad_(True)
    tilde_sigma2_err = p0[-1:].clone().requires_grad_(True)
    optimizer = torch.optim.Adam([tilde_l, uL_vec, tilde_sigma2_err], lr=lr)
    hist = np.zeros(N_opt)
    for i in range(N_opt):
        optimizer.zero_grad()
        Pars = torch.cat([tilde_l, tilde_sigma, uL_vec, tilde_sigma2_err.view(1)])
        out = logpos.nlogpos_obj_S(Pars, Y, x, **hyper_pars, verbose=True)
        out[0].backward()
        optimizer.step()
        hist[i] = -float(out[0].detach())
        if verbose:
            print("%dth iteration with target value %.8g" % (i + 1, hist[i]))
    return torch.cat([tilde_l, tilde_sigma, uL_vec, tilde_sigma2_err.view(1)]).detach().numpy().copy(), hist


def valid_rows(out, status):
    """ONE validity predicate for every lock-step driver, host- or device-resident: an evaluation counts when the factorisation
    succeeded (status 0) and both the log posterior and the likelihood are finite -- what k_alive_update / k_hmc_status test on the
    device (nmgp_kernels.hip) and nmgp_svc_batch_fetch folds into the status it returns."""
    out = np.asarray(out)
    return (np.asarray(status) == 0) & np.isfinite(out[:, 0]) & np.isfinite(out[:, 1])


class LockStepMAP:
    """MAP by Adam for B independent subjects (or B restarts of one subject) advanced in lock-step: every iteration asks
    ``value_and_grad(P [B, P])`` for the verbose tuples [B, 5], the gradients d NegLog / d pars [B, P] and a status [B] of ALL
    of them at once, then applies torch.optim.Adam's update rule (default betas / eps, no weight decay) row by row -- the same
    arithmetic, in the same order, as one ``torch.optim.Adam`` per subject, so a row reproduces :func:`map_nonseparable`.
    A subject whose evaluation fails (status != 0) is frozen at its last parameters and reported with NegLog = inf from then
    on (the reference wraps ``train()`` in try/except -> NegLog = inf, ``Nonseparable_model_mpisim.py:330-334``) while the
    others go on.  Subclasses provide ``value_and_grad``."""

    def __init__(self, init_pars, lr=2e-1, betas=(0.9, 0.999), eps=1e-8):
        self.P = np.array(init_pars, dtype=np.float64, copy=True)
        if self.P.ndim != 2:
            raise ValueError("init_pars must be [B, P]")
        self.lr, self.b1, self.b2, self.eps = float(lr), float(betas[0]), float(betas[1]), float(eps)
        self.m = np.zeros_like(self.P)
        self.v = np.zeros_like(self.P)
        self.t = 0
        self.alive = np.ones(self.P.shape[0], dtype=bool)

    def value_and_grad(self, P):
        raise NotImplementedError

    def step(self):
        out, grad, status = self.value_and_grad(self.P)
        ok = self.alive & valid_rows(out, status)
        self.alive = ok
        self.t += 1
        bc1 = 1.0 - self.b1 ** self.t
        bc2_sqrt = np.sqrt(1.0 - self.b2 ** self.t)
        g = grad[ok]
        m = self.m[ok] * self.b1 + (1.0 - self.b1) * g            # exp_avg.lerp_(grad, 1 - beta1)
        v = self.v[ok] * self.b2 + (1.0 - self.b2) * g * g        # exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
        denom = np.sqrt(v) / bc2_sqrt + self.eps
        self.P[ok] = self.P[ok] - (self.lr / bc1) * (m / denom)
        self.m[ok], self.v[ok] = m, v
        neglog = np.where(ok, out[:, 0], np.inf)
        return neglog, out

    def run(self, N_opt, callback=None):
        """Returns (pars [B, P], target_value_hist [N_opt, B] = -NegLog per iteration, alive [B])."""
        hist = np.zeros((N_opt, self.P.shape[0]))
        for i in range(N_opt):
            neglog, out = self.step()
            hist[i] = -neglog
            if callback is not None:
                callback(i, hist[i], out)
        return self.P.copy(), hist, self.alive.copy()


class BatchedMAP(LockStepMAP):
    """The MAP loop of ``Nonseparable_model_mpisim.py:330-348`` for ALL subjects of a rank at once: B subjects of the same size
    (own x, Y, own GP-prior factors) form one multi-subject batch on the GPU (``nmgp_svc_batch_set_subjects``) and every Adam
    iteration is ONE batched value+gradient launch sequence -- BASELINE config 4's per-GPU work (8 subjects x N = 1024) in the
    caller's own loop.  ``xs`` [B, N], ``Ys`` [B, N, M], ``init_pars`` [B, N(1+T)+1]."""

    def __init__(self, xs, Ys, hyper_pars, init_pars, lr=2e-1, ctx=None, device_resident=True):
        from . import _lib
        super().__init__(init_pars, lr=lr)
        self.device_resident = bool(device_resident)
        xs = np.ascontiguousarray(xs, dtype=np.float64)
        Ys = np.ascontiguousarray(Ys, dtype=np.float64)
        self.ctx = ctx if ctx is not None else _lib.default_context()
        self.hyper = np.array([float(hyper_pars[k]) for k in SVC_HYPER_KEYS])
        self.ctx.set_data(xs[0], Ys[0])
        self.ctx.svc_batch_alloc(xs.shape[0])
        self.ctx.svc_batch_set_subjects(xs, Ys)

    def value_and_grad(self, P):
        self.ctx.svc_batch_set_pars(P)
        self.ctx.svc_batch_eval(self.hyper, True, want_grad=True)
        out, status = self.ctx.svc_batch_fetch()
        return out, self.ctx.svc_batch_fetch_grad(), status

    def step(self):
        """``device_resident=True`` (default): parameters, gradients and Adam's moments stay in HBM
        (``nmgp_svc_batch_adam_step``: the update is an elementwise kernel behind the batched evaluation); per iteration only
        the B verbose tuples come back, ``self.P`` is refreshed at the end of :meth:`run` (or by :meth:`sync_pars`).  Same
        arithmetic as the host-side update (``device_resident=False``), bit for bit."""
        if not self.device_resident:
            return super().step()
        if self.t == 0:
            self.ctx.svc_batch_set_pars(self.P)
            self.ctx.svc_batch_adam_begin()
        out, alive = self.ctx.svc_batch_adam_step(self.hyper, True, self.lr, self.b1, self.b2, self.eps)
        self.t += 1
        self.alive = alive
        return np.where(alive, out[:, 0], np.inf), out

    def sync_pars(self):
        if self.device_resident and self.t > 0:
            self.P = self.ctx.svc_batch_get_pars()
        return self.P

    def run(self, N_opt, callback=None):
        _, hist, alive = super().run(N_opt, callback)
        return self.sync_pars().copy(), hist, alive


class BatchedMAPSeparable(LockStepMAP):
    """The MAP loop of ``Separable_model_mpiKAISER.py`` for ALL subjects of a rank at once: S subjects of the same size (own x, Y, own
    GP-prior factors) form one subject set on the GPU (``nmgp_sep_batch_set_subjects_chains``) and every Adam iteration is ONE
    ``nmgp_sep_batch_eval`` -- the subjects' S * k * M blocks as one batch of the blocked Cholesky.  Host-side Adam, row by row the
    arithmetic of :func:`map_separable`.  ``xs`` [S, N], ``Ys`` [S, N, M], ``init_pars`` [S * chains_per_subject, 2N+T+1]: row
    s * chains_per_subject + k is restart k of subject s."""

    def __init__(self, xs, Ys, hyper_pars, init_pars, lr=2e-1, ctx=None, chains_per_subject=1):
        from . import _lib
        super().__init__(init_pars, lr=lr)
        xs = np.ascontiguousarray(xs, dtype=np.float64)
        Ys = np.ascontiguousarray(Ys, dtype=np.float64)
        k = int(chains_per_subject)
        if xs.ndim != 2 or Ys.ndim != 3 or k < 1 or self.P.shape[0] != xs.shape[0] * k:
            raise ValueError("xs [S, N], Ys [S, N, M] and init_pars [S * chains_per_subject, P] do not fit: %s, %s, %s, k = %d"
                             % (xs.shape, Ys.shape, self.P.shape, k))
        self.ctx = ctx if ctx is not None else _lib.default_context()
        self.hyper = np.array([float(hyper_pars[key]) for key in SEP_HYPER_KEYS])
        self.prior = True
        self.ctx.set_data(xs[0], Ys[0])
        self.ctx.sep_batch_set_subjects(xs, Ys, k)

    def value_and_grad(self, P):
        """out [B, 6], grad [B, P] and a status that is 0 for every valid evaluation: jitter retries (status > 0) count as valid, a
        numerical failure (status < 0) marks the row dead for :func:`valid_rows`."""
        out, grad, status = self.ctx.sep_batch_eval(P, self.hyper, self.prior, True)
        return out, grad, np.where(status < 0, status, 0)


class HMCSampler:
    """Hamiltonian Monte Carlo with a (optionally dense) constant mass matrix.

    potential_func(position_tensor, **kwargs) -> scalar tensor (the NEGATIVE log posterior, e.g.
    ``logpos.nlogpos_obj_SVC``); gradients come from ``torch.autograd.grad`` (one fused GPU evaluation each).
    """

    def __init__(self, sample_size, potential_func, init_position, step_size=1e-4, num_steps_in_leap=20,
                 adaptive_step_size=False, M=None, duplicate_samples=True, TensorType=settings.torchType, seed=None,
                 target_accept=0.8, **kwargs):
        self.sample_size = int(sample_size)
        self.potential_func = potential_func
        self.q0 = np.asarray(init_position, dtype=np.float64).reshape(-1).copy()
        self.step_size = float(step_size)
        self.L = int(num_steps_in_leap)
        self.adaptive = bool(adaptive_step_size)
        self.duplicate_samples = bool(duplicate_samples)
        self.kwargs = kwargs
        self.rng = np.random.default_rng(seed)
        self.target_accept = target_accept
        P = self.q0.shape[0]
        if M is None:
            self.Mchol = None
            self.Minv = None
        else:
            M = np.asarray(M, dtype=np.float64)
            if M.shape != (P, P):
                raise ValueError("mass matrix must be [P, P]")
            self.Mchol = np.linalg.cholesky(M)
            self.Minv = np.linalg.inv(M)

    # -- pieces ------------------------------------------------------------------------------------
    def potential_and_grad(self, q):
        qt = torch.from_numpy(np.ascontiguousarray(q)).clone().requires_grad_(True)
        U = self.potential_func(qt, **self.kwargs)
        (g,) = torch.autograd.grad(U, qt)
        return float(U.detach()), g.numpy().copy()

    def kinetic(self, p):
        return 0.5 * float(p @ (p if self.Minv is None else self.Minv @ p))

    def draw_momentum(self, P):
        z = self.rng.standard_normal(P)
        return z if self.Mchol is None else self.Mchol @ z

    def velocity(self, p):
        return p if self.Minv is None else self.Minv @ p

    def leapfrog(self, q, p, g, eps):
        """L leapfrog steps from (q, p) with the gradient g at q; returns (q, p, U, g) at the end point."""
        p = p - 0.5 * eps * g
        U = None
        for step in range(self.L):
            q = q + eps * self.velocity(p)
            U, g = self.potential_and_grad(q)
            if not np.isfinite(U):
                return q, p, np.inf, g
            p = p - (eps if step < self.L - 1 else 0.5 * eps) * g
        return q, p, U, g

    # -- the loop -----------------------------------------------------------------------------------
    def main_hmc_loop(self):
        P = self.q0.shape[0]
        q = self.q0.copy()
        U, g = self.potential_and_grad(q)
        samples = np.zeros((self.sample_size, P))
        accepted = 0
        energy_err = np.zeros(self.sample_size)
        eps = self.step_size
        kept = 0
        it = 0
        while kept < self.sample_size:
            p0 = self.draw_momentum(P)
            H0 = U + self.kinetic(p0)
            try:
                q1, p1, U1, g1 = self.leapfrog(q, p0, g, eps)
                H1 = U1 + self.kinetic(p1)
            except RuntimeError:                  # covariance left the positive definite cone: reject
                U1, H1 = np.inf, np.inf
            with np.errstate(invalid="ignore"):       # inf - inf: start and end potential both undefined
                dH = H1 - H0
            u = np.log(self.rng.random())         # drawn every iteration: the stream does not depend on the outcome
            acc = bool(np.isfinite(dH) and (u < -dH))
            if acc:
                q, U, g = q1, U1, g1
                accepted += 1
            if acc or self.duplicate_samples:
                samples[kept] = q
                energy_err[kept] = dH if np.isfinite(dH) else np.nan
                kept += 1
            it += 1
            if self.adaptive and it <= max(50, self.sample_size // 2):
                # simple Robbins-Monro adaptation towards the target acceptance probability
                a = min(1.0, float(np.exp(-dH))) if np.isfinite(dH) else 0.0
                eps *= float(np.exp((a - self.target_accept) / np.sqrt(it)))
        info = {"accept_rate": accepted / max(it, 1), "step_size": eps, "energy_error": energy_err, "iterations": it}
        return samples, info


def sampler(**kw):
    """Alias with the reference's constructor spelling: ``HMC_Sampler.HMC_sampler.sampler(...)``."""
    return HMCSampler(**kw)


def _randomized_eigs(hvp, P, k, rank, power_iters, lam_min, seed):
    """Leading eigenpairs (by |eigenvalue|) of the symmetric operator behind ``hvp(V [k, P]) -> [k, P]`` (row v -> A v) by randomised
    subspace iteration with k probes and ``power_iters`` extra passes.  Returns (U [r, P] orthonormal rows or None, lam [r] = |eig|,
    info).  A NEGATIVE eigenvalue below -lam_min means the reference point is not a mode along that direction (an unconverged MAP
    estimate, a saddle): it enters as |lam| (the SoftAbs rule), which keeps a leapfrog step stable while the chain leaves the region."""
    def orth(Yv):
        Q, _ = np.linalg.qr(Yv.T)
        return np.ascontiguousarray(Q.T)

    rng = np.random.default_rng(seed)
    Yv = hvp(rng.standard_normal((k, P)))
    for _ in range(int(power_iters)):
        Yv = hvp(orth(Yv))
    Q = orth(Yv)
    AQ = hvp(Q)
    Tm = AQ @ Q.T
    asym = float(np.abs(Tm - Tm.T).max() / max(np.abs(Tm).max(), 1e-300))
    ev, W = np.linalg.eigh(0.5 * (Tm + Tm.T))
    order = np.argsort(-np.abs(ev))
    ev, W = ev[order], W[:, order]
    keep = np.flatnonzero(np.abs(ev[:rank]) > lam_min)
    U = np.ascontiguousarray(W[:, keep].T @ Q) if keep.size else None
    lam = np.ascontiguousarray(np.abs(ev[keep])) if keep.size else None
    info = {"probes": int(k), "power_iters": int(power_iters), "kept": int(keep.size),
            "lam_max": float(lam[0]) if keep.size else 0.0, "lam_min_kept": float(lam[-1]) if keep.size else 0.0,
            "first_dropped": float(ev[keep.size]) if keep.size < ev.size else None,
            "negative_kept": [float(v) for v in ev[keep] if v < 0], "most_negative": float(ev.min()),
            "asymmetry_of_projected_hessian": asym, "eigenvalues": [float(v) for v in ev[:min(ev.size, rank + 8)]]}
    return U, lam, info


def _preconditioned_lbfgs(f, to_pars_factory, make_metric, q, maxiter, rounds, history, gtol, verbose, nev):
    """The iteration behind :func:`polish_map` / :func:`polish_map_separable`: L-BFGS in whitened coordinates w (pars = q0 + L w, the
    model's ``apply``), the initial matrix of the two-loop recursion H0 = (I + U diag(lam) U^T)^-1 from ``make_metric(q)`` (rebuilt
    every maxiter / rounds iterations), Armijo backtracking.  ``f(w, to_pars) -> (NegLog, whitened gradient)`` (+inf, None outside the
    domain); ``to_pars_factory(q0) -> to_pars(w)``; ``nev``: one-element evaluation counter shared with the caller."""
    q_cur = q
    P = q.shape[0]
    per_round = max(1, int(np.ceil(maxiter / max(rounds, 1))))
    fk = gn = None
    for rnd in range(max(rounds, 1)):
        met = make_metric(q_cur, rnd)
        U, sc = (met.U, met.lam / (1.0 + met.lam)) if met.rank else (None, None)
        to_pars = to_pars_factory(q_cur)

        def precond(d):
            return d - U.T @ (sc * (U @ d)) if U is not None else d

        xk = np.zeros(P)
        fk, gk = f(xk, to_pars)
        if not np.isfinite(fk):
            raise RuntimeError("polish: the objective is undefined at the start point")
        S, Yv, rho = [], [], []
        stalled = False
        for _ in range(per_round):
            gn = float(np.sqrt(_dot(gk, gk)))
            if gn <= gtol * max(1.0, abs(fk)):
                break
            d = -gk.copy()
            al = []
            for s_, y_, r_ in zip(reversed(S), reversed(Yv), reversed(rho)):
                a_ = r_ * _dot(s_, d)
                al.append(a_)
                d -= a_ * y_
            d = precond(d)                               # H0 = (I + U lam U^T)^-1
            for (s_, y_, r_), a_ in zip(zip(S, Yv, rho), reversed(al)):
                d += (a_ - r_ * _dot(y_, d)) * s_
            slope = _dot(gk, d)
            if slope >= 0:                               # stale pairs: restart from the preconditioned gradient
                S, Yv, rho = [], [], []
                d = precond(-gk.copy())
                slope = _dot(gk, d)
            t = 1.0
            while True:
                xn = xk + t * d
                fn, gnew = f(xn, to_pars)
                if fn <= fk + 1e-4 * t * slope:
                    break
                t *= 0.5
                if t < 1e-10:
                    stalled = True
                    break
            if stalled:
                break
            s_, y_ = xn - xk, gnew - gk
            sy = _dot(s_, y_)
            if sy > 1e-10 * np.sqrt(_dot(s_, s_) * _dot(y_, y_)):
                S.append(s_)
                Yv.append(y_)
                rho.append(1.0 / sy)
                if len(S) > history:
                    S.pop(0), Yv.pop(0), rho.pop(0)
            xk, fk, gk = xn, fn, gnew
        q_cur = to_pars(xk)
        gn = float(np.sqrt(_dot(gk, gk)))
        if verbose is not None:
            verbose("polish round %d: NegLog %.4f, whitened |grad| %.3g, %d evaluations so far, metric rank %d (most negative %.3g)" % (
                rnd, fk, gn, nev[0], met.rank, met.info["most_negative"]))
        if gn <= gtol * max(1.0, abs(fk)):
            break
    return q_cur, fk, gn, nev[0]


def _dot(a, b):
    # (not BLAS: on a 64-core host a threaded ddot of 14,337 elements costs more than the GPU evaluation it sits next to)
    return float(np.sum(a * b))


def polish_map(x, Y, hyper_pars, q, maxiter=300, ctx=None, history=30, gtol=1e-6, rounds=4, rank=64, probes=96, verbose=None):
    """From an Adam MAP estimate to the mode of the nonseparable objective (the reference stops Adam after a fixed number of
    iterations, Nonseparable_model.py:161-175; a sampler metric built from the Hessian wants a point that IS a mode -- at N = 2048
    the committed Adam estimate is 4,000 log-posterior units below it).

    L-BFGS in the coordinates w of the prior-factor metric, pars = q + L_blk w, PRECONDITIONED by the metric's low-rank part: the
    initial matrix of the two-loop recursion is H0 = (I + U diag(lam) U^T)^-1 from :func:`prior_lowrank_metric` at the current point
    (rebuilt every ``maxiter / rounds`` iterations: the likelihood's curvature moves while the point does), so the quasi-Newton
    pairs only have to learn how the Hessian differs from the metric.  In the parameters themselves the GP priors' condition number
    of 1e11 makes a quasi-Newton method crawl (2,000 iterations of SciPy's L-BFGS-B ended with |grad| = 108), and in plain
    whitened coordinates the 26 likelihood directions (eigenvalues up to 4e5 next to ~14,300 ones) do the same.  The change of
    coordinates is the device's (``nmgp_svc_batch_prior_apply``); two-loop recursion and Armijo backtracking in NumPy on the host,
    one single-chain value+gradient evaluation on the GPU per trial point (a point outside the positive definite cone counts as
    +inf).  Returns (pars, NegLog, whitened gradient norm, evaluations incl. the metric's)."""
    from . import _lib
    ctx = ctx if ctx is not None else _lib.default_context()
    hyper = np.array([float(hyper_pars[k]) for k in SVC_HYPER_KEYS])
    x, Y = np.asarray(x, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    ctx.set_data(x, Y)
    nev = [0]
    q_cur = np.array(q, dtype=np.float64, copy=True).reshape(-1)
    P = q_cur.shape[0]
    B = int(min(probes, P))
    buf = np.zeros((B, P))

    def apply(v, trans):
        buf[0] = v
        return ctx.svc_batch_prior_apply(hyper, buf, trans=trans)[0].copy()

    def make_metric(q_at, rnd):
        met = prior_lowrank_metric(x, Y, hyper_pars, q_at, rank=rank, oversample=max(B - rank, 0), power_iters=1, seed=11 + rnd, ctx=ctx,
                                   batch=B)          # (leaves a batch of B chains allocated: `apply` uses it)
        nev[0] += met.info["grad_evals"]
        return met

    def to_pars_factory(q0):
        return lambda w: q0 + apply(w, False)

    def f(w, to_pars):
        nev[0] += 1
        try:
            out, g = ctx.logpos_svc(to_pars(w), hyper, True, True)
        except _lib.NmgpNumericalError:
            return np.inf, None
        v = float(out[0])
        if not (np.isfinite(v) and np.all(np.isfinite(g))):
            return np.inf, None
        return v, apply(g, True)

    return _preconditioned_lbfgs(f, to_pars_factory, make_metric, q_cur, maxiter, rounds, history, gtol, verbose, nev)


class PriorMetric:
    """The prior-factor metric of the device-resident trajectories (``nmgp_svc_batch_traj_set_mass_prior``, csrc/nmgp_metric.hip):

        M^-1 = L_blk (I + U diag(lam) U^T)^-1 L_blk^T,   L_blk = blockdiag(chol Sigma_l, chol Sigma_L per uL column, 1)

    with the Cholesky factors of the GP priors of ``logpos.py:357-365`` (cached on the device per subject) and an optional rank-r
    correction ``U`` [r, P] (or [S, r, P] for S subjects; orthonormal rows), ``lam`` [r] / [S, r] >= 0 for the curvature the
    likelihood adds in the whitened coordinates ``pars = mu + L_blk w`` -- see :func:`prior_lowrank_metric`.  It takes the place of
    the ``M = inv(sample covariance)`` the reference's production runs pass (Nonseparable_model_mpiKAISER.py:398-411), which at
    P = 14,337 would need more draws than a run has."""

    def __init__(self, hyper_pars, U=None, lam=None, info=None):
        self.hyper = np.array([float(hyper_pars[k]) for k in SVC_HYPER_KEYS])
        self.U = None if U is None else np.ascontiguousarray(U, dtype=np.float64)
        self.lam = None if lam is None else np.ascontiguousarray(lam, dtype=np.float64)
        self.info = info or {}

    @property
    def rank(self):
        return 0 if self.U is None else int(self.U.shape[-2])

    @staticmethod
    def stack(metrics):
        """One metric for a multi-subject batch from the subjects' own metrics (same hyper-parameters): U [S, r, P], lam [S, r] with
        r = the largest rank; a subject with fewer directions is padded with lam = 0 rows, which leave its metric unchanged."""
        hyper = metrics[0].hyper
        if any(not np.array_equal(m.hyper, hyper) for m in metrics):
            raise ValueError("the subjects' metrics must share the GP-prior hyper-parameters")
        r = max(m.rank for m in metrics)
        out = PriorMetric.__new__(PriorMetric)
        out.hyper, out.info = hyper.copy(), {"subjects": [m.info for m in metrics]}
        if r == 0:
            out.U = out.lam = None
            return out
        P = next(m.U.shape[-1] for m in metrics if m.U is not None)
        out.U, out.lam = np.zeros((len(metrics), r, P)), np.zeros((len(metrics), r))
        for s_, m in enumerate(metrics):
            if m.rank:
                out.U[s_, :m.rank], out.lam[s_, :m.rank] = m.U, m.lam
        return out


def prior_lowrank_metric(x, Y, hyper_pars, q_ref, rank=96, oversample=32, power_iters=1, h=1e-3, lam_min=0.5, seed=0, ctx=None,
                         batch=None):
    """Build the :class:`PriorMetric` of ONE subject at ``q_ref`` (its MAP estimate): the top eigenpairs of

        A = L_blk^T  Hess(-loglik)(q_ref)  L_blk        (the prior's own Hessian is the identity in these coordinates)

    by randomised subspace iteration (``rank + oversample`` probe vectors, ``power_iters`` extra passes).  Every Hessian-vector
    product is a central difference of the LIKELIHOOD gradient (``Prior=False``: no ill-conditioned prior solve enters), ``batch``
    of them per batched launch sequence (``nmgp_svc_batch_eval``), the change of coordinates runs on the device
    (``nmgp_svc_batch_prior_apply``).  ``h``: largest parameter displacement of a probe.  Eigenvalues with |lam| below ``lam_min``
    are dropped (they change a direction's scale by < 25 %); a negative one beyond that enters as |lam|.  Cost: (2 + power_iters) x 2 x (rank + oversample) gradient evaluations."""
    from . import _lib
    ctx = ctx if ctx is not None else _lib.default_context()
    x, Y = np.asarray(x, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    hyper = np.array([float(hyper_pars[k]) for k in SVC_HYPER_KEYS])
    q_ref = np.asarray(q_ref, dtype=np.float64).reshape(-1)
    P = q_ref.shape[0]
    k = int(min(rank + oversample, P))
    B = int(batch) if batch else min(k, 128)
    ctx.set_data(x, Y)
    ctx.svc_batch_alloc(B)
    n_grad = [0]

    def in_chunks(V, fn):
        out = np.empty_like(V)
        buf = np.zeros((B, P))
        for a in range(0, V.shape[0], B):
            m = min(B, V.shape[0] - a)
            buf[:m] = V[a:a + m]
            buf[m:] = buf[0]                  # pad with a valid row
            out[a:a + m] = fn(buf)[:m]
        return out

    def lik_grad(Q):
        ctx.svc_batch_set_pars(Q)
        ctx.svc_batch_eval(hyper, False, want_grad=True)
        out, status = ctx.svc_batch_fetch()
        if not valid_rows(out, status).all():
            raise RuntimeError("prior_lowrank_metric: the likelihood is undefined at a probe point (status %s): reduce h" % status)
        n_grad[0] += Q.shape[0]
        return ctx.svc_batch_fetch_grad()

    def hvp(V):
        """A V^T for the rows of V [k, P]."""
        D = in_chunks(V, lambda v: ctx.svc_batch_prior_apply(hyper, v, trans=False))
        t = h / np.maximum(np.abs(D).max(1), 1e-300)
        Gp = in_chunks(q_ref[None] + t[:, None] * D, lik_grad)
        Gm = in_chunks(q_ref[None] - t[:, None] * D, lik_grad)
        Hq = (Gp - Gm) / (2.0 * t[:, None])
        return in_chunks(Hq, lambda g: ctx.svc_batch_prior_apply(hyper, g, trans=True))

    U, lam, info = _randomized_eigs(hvp, P, k, rank, power_iters, lam_min, seed)
    info.update(h=float(h), grad_evals=int(n_grad[0]))
    return PriorMetric(hyper_pars, U, lam, info)


class SeparablePriorMetric:
    """The prior-factor metric of the SEPARABLE model (logpos.py:216-296; sampler call Separable_model.py:209-210), host side: its
    parameter vector [tilde_l (N) | tilde_sigma (N) | uL_vec (T) | tilde_sigma2_err] carries GP priors RBF(alpha, beta) + 1e-6 I on
    tilde_l and tilde_sigma (logpos.py:271-281) and Normal(0, c) on uL_vec (:283), so
        L_blk = blockdiag(chol Sigma_l, chol Sigma_sigma, c I_T, 1),     M^-1 = L_blk (I + U diag(lam) U^T)^-1 L_blk^T
    exactly as :class:`PriorMetric` for the nonseparable model.  P = 2N + T + 1 is small enough (8,208 at config 5's size) for the
    leapfrog update itself to stay on the host; its two triangular products per step run on the device with the context's cached
    prior factors (``nmgp_sep_prior_apply``: the nonseparable sampler's ``k_prior_trmm`` with the separable parameter layout)."""

    def __init__(self, L_l, L_s, c, T, U=None, lam=None, info=None, ctx=None, hyper=None, N=None):
        """Either the two factors as host matrices (``L_l``, ``L_s``; tests, or a caller with its own factors) or ``ctx`` + ``hyper``
        [9] + ``N``: the products then run on the device with the context's cached prior factors (``nmgp_sep_prior_apply``)."""
        self.ctx, self.hyper = ctx, (None if hyper is None else np.asarray(hyper, dtype=np.float64))
        self.c, self.T = float(c), int(T)
        if ctx is None:
            self.L_l, self.L_s = np.ascontiguousarray(L_l), np.ascontiguousarray(L_s)
            # both orientations contiguous: the two products of a leapfrog step then are plain row-major GEMMs [B, N] x [N, N]
            self.Lt_l = np.ascontiguousarray(self.L_l.T)
            self.Lt_s = self.Lt_l if L_s is L_l else np.ascontiguousarray(self.L_s.T)
            self.N = self.L_l.shape[0]
        else:
            self.L_l = self.L_s = self.Lt_l = self.Lt_s = None
            self.N = int(N)
        self.P = 2 * self.N + self.T + 1
        self.U = None if U is None else np.ascontiguousarray(U, dtype=np.float64)
        self.lam = None if lam is None else np.ascontiguousarray(lam, dtype=np.float64)
        self.info = info or {}

    @property
    def rank(self):
        return 0 if self.U is None else int(self.U.shape[0])

    def apply(self, v, trans):
        """L_blk v (trans False) or L_blk^T v (trans True) for the rows of v [B, P]."""
        if self.ctx is not None:
            return self.ctx.sep_prior_apply(self.hyper, np.ascontiguousarray(v), trans)
        N, T = self.N, self.T
        out = np.empty_like(v)
        out[:, :N] = np.ascontiguousarray(v[:, :N]) @ (self.L_l if trans else self.Lt_l)
        out[:, N:2 * N] = np.ascontiguousarray(v[:, N:2 * N]) @ (self.L_s if trans else self.Lt_s)
        out[:, 2 * N:2 * N + T] = self.c * v[:, 2 * N:2 * N + T]
        out[:, -1] = v[:, -1]
        return out

    def _lowrank(self, u, w):
        return u if self.U is None else u + ((u @ self.U.T) * w) @ self.U

    def root(self, z):          # u = (I + U lam U^T)^1/2 z
        return self._lowrank(z, None if self.U is None else np.sqrt(1.0 + self.lam) - 1.0)

    def W(self, u):             # (I + U lam U^T)^-1 u
        return self._lowrank(u, None if self.U is None else -self.lam / (1.0 + self.lam))

    def kinetic(self, u):
        k = (u * u).sum(1)
        if self.U is not None:
            c = u @ self.U.T
            k = k - (c * c * (self.lam / (1.0 + self.lam))).sum(1)
        return 0.5 * k


def separable_prior_metric(x, Y, hyper_pars, q_ref, rank=64, oversample=32, power_iters=1, h=1e-3, lam_min=0.5, seed=0, ctx=None,
                           batch=16, factors=None):
    """:class:`SeparablePriorMetric` of one subject at ``q_ref``: the context's cached GP-prior factors (``factors`` is accepted for
    compatibility and ignored) and the leading eigenpairs of L_blk^T Hess(-loglik) L_blk by randomised subspace iteration on central
    differences of the likelihood gradient, ``batch`` chains per ``nmgp_sep_batch_eval``."""
    from . import _lib
    ctx = ctx if ctx is not None else _lib.default_context()
    x, Y = np.asarray(x, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    hyper = np.array([float(hyper_pars[k]) for k in SEP_HYPER_KEYS])
    q_ref = np.asarray(q_ref, dtype=np.float64).reshape(-1)
    N, M = Y.shape
    T = M * (M + 1) // 2
    P = 2 * N + T + 1
    if q_ref.shape[0] != P:
        raise ValueError("q_ref must have 2N + T + 1 = %d entries" % P)
    ctx.set_data(x, Y)
    # Normal(0, c) sees a float32-rounded c in the reference (logpos.py:283 passes a Python number to torch.distributions.Normal)
    met = SeparablePriorMetric(None, None, float(np.float32(hyper[8])), T, ctx=ctx, hyper=hyper, N=N)
    k = int(min(rank + oversample, P))
    n_grad = [0]

    def lik_grad(Q):
        G = np.empty_like(Q)
        for a in range(0, Q.shape[0], batch):
            out, g, st = ctx.sep_batch_eval(Q[a:a + batch], hyper, False, True)
            if (st != 0).any() or not np.all(np.isfinite(out[:, 1])):
                raise RuntimeError("separable_prior_metric: the likelihood is undefined (or needed jitter) at a probe point: reduce h")
            G[a:a + batch] = g
        n_grad[0] += Q.shape[0]
        return G

    def hvp(V):
        D = met.apply(V, False)
        t = h / np.maximum(np.abs(D).max(1), 1e-300)
        Hq = (lik_grad(q_ref[None] + t[:, None] * D) - lik_grad(q_ref[None] - t[:, None] * D)) / (2.0 * t[:, None])
        return met.apply(Hq, True)

    met.U, met.lam, info = _randomized_eigs(hvp, P, k, rank, power_iters, lam_min, seed)
    info.update(h=float(h), grad_evals=int(n_grad[0]))
    met.info = info
    return met


def polish_map_separable(x, Y, hyper_pars, q, maxiter=300, ctx=None, history=30, gtol=1e-6, rounds=4, rank=64, probes=96, batch=16,
                         verbose=None):
    """:func:`polish_map` for the separable objective (``logpos.nlogpos_obj``): metric-preconditioned L-BFGS in the whitened
    coordinates of :class:`SeparablePriorMetric`.  Returns (pars, NegLog, whitened gradient norm, evaluations incl. the metric's)."""
    from . import _lib
    ctx = ctx if ctx is not None else _lib.default_context()
    hyper = np.array([float(hyper_pars[k]) for k in SEP_HYPER_KEYS])
    x, Y = np.asarray(x, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    ctx.set_data(x, Y)
    nev = [0]
    q_cur = np.array(q, dtype=np.float64, copy=True).reshape(-1)
    state = {"met": None}

    def make_metric(q_at, rnd):
        met = separable_prior_metric(x, Y, hyper_pars, q_at, rank=rank, oversample=max(probes - rank, 0), power_iters=1, seed=11 + rnd,
                                     ctx=ctx, batch=batch, factors=state["met"])
        nev[0] += met.info["grad_evals"]
        state["met"] = met
        return met

    def to_pars_factory(q0):
        return lambda w: q0 + state["met"].apply(w[None], False)[0]

    def f(w, to_pars):
        nev[0] += 1
        try:
            out, g = ctx.logpos_sep(to_pars(w), hyper, True, True)
        except _lib.NmgpNumericalError:
            return np.inf, None
        v = float(out[0])
        if not (np.isfinite(v) and np.all(np.isfinite(g))):
            return np.inf, None
        return v, state["met"].apply(g[None], True)[0]

    return _preconditioned_lbfgs(f, to_pars_factory, make_metric, q_cur, maxiter, rounds, history, gtol, verbose, nev)


# ---- what every lock-step sampler shares: the potential of a batched evaluation, the host leapfrog, the Metropolis loop ------------
def _potential_and_grad(out, g, bad):
    """U [B] = ``out[:, 0]`` and dU/dq = ``g`` of a batched evaluation: a chain that is ``bad`` gets U = inf and a zero gradient
    (``g`` may be None: a value-only evaluation).  Each driver states its own ``bad``: they differ on purpose (jitter retries)."""
    U = np.array(out[:, 0])
    U[bad] = np.inf
    if g is not None:
        g[bad] = 0.0
    return U, g


def _leapfrog(q, p, U, g, eps, L, evaluate, kick, drift, mask=None):
    """THE host leapfrog: ``L`` steps from ``(q, p)`` [B, P] with the potential ``U`` [B] and its gradient ``g`` at q,

        p -= eps/2 kick(g);   L x { q += eps drift(p);   U, g = evaluate(q);   p -= eps kick(g) }   (eps/2 in the last step)

    ``eps`` a scalar or a column [B, 1] (a step per row), ``kick`` / ``drift`` the maps the metric puts on the gradient and on the
    momentum.  ``mask`` [B, P] marks the real slots of padded rows: a padded p is +0.0 from the first kick on, a padded q never
    changes, and whatever the padded slots hold (NaN, inf) raises no warning; without a mask every slot is real.  Returns
    ``(q1, p1, U1, g1, failed)``.  A chain whose potential is undefined at ANY point of the trajectory has left the leapfrog map
    (its kick was skipped there): it is ``failed``, and its ``U1`` is inf even if the trajectory came back to a valid point,
    exactly as ``HMCSampler.leapfrog`` returns inf at the first non-finite potential.  The START counts as a point: a chain that
    starts at U = inf has H0 = inf, so dH is -inf or NaN whatever U1 is -- it is rejected and records NaN either way."""
    keep = (lambda new, old: new) if mask is None else (lambda new, old: np.where(mask, new, old))
    with np.errstate(**({} if mask is None else {"invalid": "ignore", "over": "ignore"})):
        p = keep(p - (0.5 * eps) * kick(g), 0.0)
        failed = ~np.isfinite(U)
        for step in range(L):
            q = keep(q + eps * drift(p), q)
            U, g = evaluate(q)
            failed |= ~np.isfinite(U)
            p = keep(p - (eps if step < L - 1 else 0.5 * eps) * kick(g), p)
    return q, p, np.where(failed, np.inf, U), g, failed


def _jitter_rng(seed):
    """the generator of the step jitter: its own stream, so the chains' streams do not depend on ``step_jitter``"""
    return np.random.default_rng(None if seed is None else 7919 * (seed + 1))


def _metropolis(groups, n, B, t_start, step_jitter=0.0, jitter_rng=None):
    """THE Metropolis loop of every lock-step sampler: ``n`` iterations over one or more ``groups`` of chains, ``B`` chains in all.
    A complete-data or per-subject sampler is one group, a cohort bucket is a group.  A group is a dictionary with its state

        ``q`` [b, P] positions (updated in place), ``U`` [b] their potentials, ``rngs`` its chains' generators, ``rows`` the columns
        of the caller's [.., B] order that its chains fill, ``samples`` a list of arrays [n, ...] and ``split(q)`` the list of what
        iteration ``it`` writes into ``samples[j][it]``,

    and with what differs between the samplers:

        ``draw() -> (p0, K0)``: the momenta (or whatever ``trajectory`` takes for them) and the start's kinetic energy; every chain
        draws its P (real) standard normals from its own generator here, the accept uniform follows below (:class:`HMCSampler`'s order);
        ``trajectory(jit, p0) -> (q1, m1, U1, failed, g1)`` at ``jit`` times the group's step size: the end point, its momentum (or
        its kinetic energy, where the device forms it), its potential, the chains that left the domain, and its gradient (or None);
        ``kinetic_end(m1) -> K1``;  ``commit(acc, g1)``: keep the end point's gradient where ``acc`` -- on the host, or on the device.

    ``step_jitter`` j > 0: iteration i runs at ``jit = 1 + j u_i``, u_i ~ U(-1, 1) from ``jitter_rng``, one draw per iteration for
    all groups; otherwise ``jit = 1`` and no generator is touched.  Returns ``(accepted [B], energy_error [n, B], timing)``:
    ``timing`` splits the wall time since ``t_start`` into the setup before the loop, the loop, and inside it the ``trajectory``
    calls (on the device: the upload, the leapfrog launches, the end point's download) against everything the host does around
    them (normal draws, energies, accept test, bookkeeping)."""
    accepted, energy_err = np.zeros(B), np.zeros((n, B))
    t_loop = time.perf_counter()
    t_traj = 0.0
    for it in range(n):
        jit = 1.0 if step_jitter <= 0 else 1.0 + step_jitter * jitter_rng.uniform(-1.0, 1.0)
        for gr in groups:
            p0, K0 = gr["draw"]()
            H0 = gr["U"] + K0
            t0 = time.perf_counter()
            q1, m1, U1, failed, g1 = gr["trajectory"](jit, p0)
            t_traj += time.perf_counter() - t0
            U1 = np.where(failed, np.inf, U1)
            H1 = U1 + gr["kinetic_end"](m1)
            with np.errstate(invalid="ignore"):       # inf - inf: start and end potential both undefined
                dH = H1 - H0
            u = np.array([np.log(r.random()) for r in gr["rngs"]])      # drawn every iteration: the stream does not depend on the outcome
            acc = np.isfinite(dH) & (u < -dH)
            gr["commit"](acc, g1)
            gr["q"][acc] = q1[acc]
            gr["U"] = np.where(acc, U1, gr["U"])
            accepted[gr["rows"]] += acc
            energy_err[it, gr["rows"]] = np.where(np.isfinite(dH), dH, np.nan)
            for rec, v in zip(gr["samples"], gr["split"](gr["q"])):
                rec[it] = v
    t_end = time.perf_counter()
    return accepted, energy_err, {"setup_seconds": t_loop - t_start, "loop_seconds": t_end - t_loop, "trajectory_call_seconds": t_traj,
                                  "device_share": t_traj / max(t_end - t_loop, 1e-12)}


class LockStepHMC:
    """B independent HMC chains advanced in lock-step: every leapfrog step asks ``potential_and_grad(q [B, P])`` for the
    potentials U [B] and gradients [B, P] of ALL chains at once (U = inf marks a chain whose potential is undefined at
    that point, e.g. a covariance outside the positive definite cone).  Constant mass matrix (identity by default, see
    :meth:`set_mass`).  Chain b draws from its own
    generator in the order of :class:`HMCSampler` (momentum, then the uniform of the accept test), so a chain reproduces
    the single-chain sampler started from the same state.  Subclasses provide ``potential_and_grad``."""

    def __init__(self, init_positions, step_size=1e-4, num_steps_in_leap=20, seed=None, M=None, Minv=None):
        self.q = np.array(init_positions, dtype=np.float64, copy=True)
        if self.q.ndim != 2:
            raise ValueError("init_positions must be [B, P]")
        self.B, self.P = self.q.shape
        self.eps = float(step_size)
        self.L = int(num_steps_in_leap)
        self.rngs = [np.random.default_rng(None if seed is None else seed + b) for b in range(self.B)]
        self.set_mass(M, Minv)

    def set_mass(self, M=None, Minv=None):
        """Constant mass matrix shared by the chains (``M`` of the reference's sampler call, Nonseparable_model_mpiKAISER.py:267-270:
        M = inv(sample covariance)): None = identity, a vector [P] = diagonal, a matrix [P, P] = dense.  ``Minv`` may be given
        alongside (the reference's caller HAS it: it is the sample covariance) to spare the inversion; momenta are drawn as
        chol(M) z, the kinetic energy is 1/2 p^T M^-1 p and the drift q += eps M^-1 p."""
        P = self.P
        self.mass_kind = 0
        self.Mchol = self.Minv = self.metric = None
        if M is None and Minv is None:
            return
        if isinstance(M, PriorMetric):
            # the prior-factor metric lives on the device only (whitened momenta, cached prior factors): BatchedHMC's resident loop
            self.mass_kind = 3
            self.metric = M
            return
        if isinstance(M, SeparablePriorMetric):
            if M.P != P:
                raise ValueError("the metric belongs to a parameter vector of length %d, not %d" % (M.P, P))
            self.mass_kind = 4           # host-side whitened-momentum loop of BatchedHMCSeparable
            self.metric = M
            return
        if M is None:
            Minv = np.asarray(Minv, dtype=np.float64)
            M = 1.0 / Minv if Minv.ndim == 1 else np.linalg.inv(Minv)
        M = np.asarray(M, dtype=np.float64)
        if M.shape == (P,):
            if np.any(M <= 0):
                raise ValueError("diagonal mass matrix must be positive")
            self.mass_kind = 1
            self.Mchol = np.sqrt(M)
            self.Minv = 1.0 / M if Minv is None else np.asarray(Minv, dtype=np.float64).reshape(P)
        elif M.shape == (P, P):
            self.mass_kind = 2
            self.Mchol = np.linalg.cholesky(M)
            self.Minv = np.linalg.inv(M) if Minv is None else np.asarray(Minv, dtype=np.float64).reshape(P, P)
        else:
            raise ValueError("mass matrix must be [P] or [P, P] with P = %d" % P)

    def draw_momenta(self):
        """[B, P]: chain b draws P standard normals from its own generator (the stream of :class:`HMCSampler`), then p = chol(M) z."""
        z = self._normals()
        if self.mass_kind == 0:
            return z
        if self.mass_kind >= 3:
            raise NotImplementedError("a PriorMetric / SeparablePriorMetric runs in its sampler's own whitened-momentum loop")
        return z * self.Mchol if self.mass_kind == 1 else z @ self.Mchol.T

    def velocity(self, p):
        if self.mass_kind == 0:
            return p
        if self.mass_kind >= 3:
            raise NotImplementedError("a PriorMetric / SeparablePriorMetric runs in its sampler's own whitened-momentum loop")
        return p * self.Minv if self.mass_kind == 1 else p @ self.Minv          # (M^-1 is symmetric)

    def kinetic(self, p):
        return 0.5 * (p * self.velocity(p)).sum(1)

    def potential_and_grad(self, q):
        raise NotImplementedError

    def _normals(self):
        """z [B, P]: chain b's next P standard normals, from its own generator"""
        return np.stack([r.standard_normal(self.P) for r in self.rngs])

    def _host_group(self, draw, kick, drift, kinetic):
        """The B chains as one group of :func:`_metropolis` whose trajectory runs on the host: :func:`_leapfrog` with the metric's
        ``kick`` and ``drift`` around ``potential_and_grad``, the gradient at the chains' positions kept on the host."""
        U, g = self.potential_and_grad(self.q)
        gr = {"q": self.q, "U": U, "g": g, "draw": draw, "kinetic_end": kinetic}

        def trajectory(jit, p0):
            q1, p1, U1, g1, failed = _leapfrog(gr["q"], p0, gr["U"], gr["g"], self.eps * jit, self.L, self.potential_and_grad, kick, drift)
            return q1, p1, U1, failed, g1

        def commit(acc, g1):
            gr["g"] = np.where(acc[:, None], g1, gr["g"])
        gr.update(trajectory=trajectory, commit=commit)
        return gr

    def _sample(self, group, n, t_start, jittered=False):
        """:func:`_metropolis` over the B chains as ONE group; ``jittered``: with the driver's ``step_jitter``.  Returns
        ``(samples [n, B, P], info)``: ``accept_rate`` [B], ``energy_error`` [n, B] (NaN where it is undefined) and ``timing``."""
        samples = np.zeros((n, self.B, self.P))
        group.update(rngs=self.rngs, rows=slice(None), samples=[samples], split=lambda q: [q])
        accepted, energy_err, timing = _metropolis([group], n, self.B, t_start, *((self.step_jitter, self.jitter_rng) if jittered else ()))
        return samples, {"accept_rate": accepted / n, "energy_error": energy_err, "timing": timing}

    def _draw(self):
        p0 = self.draw_momenta()
        return p0, self.kinetic(p0)

    def run(self, sample_size):
        """``sample_size`` iterations of :func:`_metropolis` with the trajectories on the host (:func:`_leapfrog`) under the constant
        mass of :meth:`set_mass`: p0 = ``draw_momenta()``, K = ``kinetic(p)``, kick p -= c g, drift q += eps ``velocity(p)``."""
        t_start = time.perf_counter()
        return self._sample(self._host_group(self._draw, lambda g: g, self.velocity, self.kinetic), sample_size, t_start)


class BatchedHMC(LockStepHMC):
    """B independent HMC chains of one subject advanced in lock-step on the GPU.

    Every leapfrog step evaluates the potential and its gradient for ALL chains with one batched launch sequence
    (``nmgp_svc_batch_eval(want_grad=1)``): the chains are the reference's embarrassingly-parallel unit
    (one process each there, ``Nonseparable_model_mpisim.py:305-306``); here they share the GPU's launch latency.
    Nonseparable model only (the batched entry point of the C ABI).  ``M`` / ``Minv``: constant mass matrix shared by the
    chains (None: identity; [P]: diagonal; [P, P]: dense, as the reference's production sampler passes it,
    Nonseparable_model_mpiKAISER.py:267-270,398-411) -- resident on the device, the drift of every leapfrog step is one GEMM.
    ``x`` [N], ``Y`` [N, M]: B chains of one subject; ``x`` [S, N], ``Y`` [S, N, M]: S subjects with ``chains_per_subject``
    chains each (default 1: config 4's unit, one chain per subject), ``init_positions`` [S * chains_per_subject, P] subject-major
    (row s * chains_per_subject + k = chain k of subject s).  The chains of a subject share its data and prior factors on the
    device; 8 subjects x 8 chains is config 4's per-GPU subject count at a batch size where the factorisation is
    throughput-bound, and what a between-chain diagnostic (R-hat) needs.
    """

    def __init__(self, x, Y, hyper_pars, init_positions, step_size=1e-4, num_steps_in_leap=20, seed=None, ctx=None,
                 device_resident=True, M=None, Minv=None, chains_per_subject=1, device_momenta=None, step_jitter=0.0):
        from . import _lib
        super().__init__(init_positions, step_size, num_steps_in_leap, seed, M, Minv)
        self.device_resident = bool(device_resident)
        # step_jitter j > 0: iteration i uses eps (1 + j u_i), u_i ~ U(-1, 1) from a generator of its own (the chains' streams are
        # untouched), the same step for all chains of the iteration -- the usual guard against a trajectory length that resonates
        # with the posterior's periods (under a PriorMetric they are all ~2 pi).  Device-resident loop only: device_resident=False
        # IGNORES step_jitter.
        self.step_jitter = float(step_jitter)
        self.jitter_rng = _jitter_rng(seed)
        # device_momenta: the host only draws the standard normals z; p0 = chol(M) z and the end point's kinetic energy
        # 1/2 p1^T M^-1 p1 are formed on the device (nmgp_svc_batch_traj_z).  Default: on whenever a mass matrix is set -- the
        # host's share of a dense-mass sample was two [B, P] x [P, P] NumPy products -- off for the identity (where it would only
        # change the summation order of 1/2 |p|^2 against the host-side loop the tests compare with bit for bit).
        self.device_momenta = (self.mass_kind != 0) if device_momenta is None else bool(device_momenta)
        if self.mass_kind == 3:
            if not self.device_resident or not self.device_momenta:
                raise ValueError("a PriorMetric needs device_resident=True and device_momenta=True")
        self.ctx = ctx if ctx is not None else _lib.default_context()
        self.hyper = np.array([float(hyper_pars[k]) for k in SVC_HYPER_KEYS])
        x, Y = np.asarray(x, dtype=np.float64), np.asarray(Y, dtype=np.float64)
        if x.ndim == 2:
            # one chain per SUBJECT (BASELINE config 4's unit: x [B, N], Y [B, N, M], every subject with its own prior factors)
            k = int(chains_per_subject)
            if k < 1 or x.shape[0] * k != self.B or Y.shape[0] * k != self.B:
                raise ValueError("x [S, N] and Y [S, N, M] must hold B / chains_per_subject = %d / %d subjects" % (self.B, k))
            self.ctx.set_data(x[0], Y[0])
            self.ctx.svc_batch_alloc(self.B)
            self.ctx.svc_batch_set_subjects(x, Y, k)
        else:
            self.ctx.set_data(x, Y)
            self.ctx.svc_batch_alloc(self.B)

    def potential_and_grad(self, q):
        """U [B] and dU/dq [B, P]; a chain whose covariance is not positive definite gets U = inf."""
        self.ctx.svc_batch_set_pars(q)
        self.ctx.svc_batch_eval(self.hyper, True, want_grad=True)
        out, status = self.ctx.svc_batch_fetch()
        return _potential_and_grad(out, self.ctx.svc_batch_fetch_grad(), ~valid_rows(out, status))

    def run(self, sample_size):
        """``device_resident=True`` (default): positions, momenta and gradients stay in HBM for the whole trajectory
        (``nmgp_svc_batch_traj``: the leapfrog updates are elementwise kernels between the batched evaluations); per sample
        the host uploads the momenta it drew, reads the end point back and decides acceptance (:func:`_metropolis`) -- the same
        arithmetic and the same random streams as the host-side trajectories of :meth:`LockStepHMC.run`
        (``device_resident=False``, which ignores ``step_jitter``), bit for bit."""
        if not self.device_resident:
            return super().run(sample_size)
        t_start = time.perf_counter()
        U, _ = self.potential_and_grad(self.q)           # leaves q and dU/dq resident
        if self.mass_kind == 3:
            self.ctx.svc_batch_traj_set_mass_prior(self.metric.hyper, self.metric.U, self.metric.lam)
        else:
            self.ctx.svc_batch_traj_set_mass(None if self.mass_kind == 0 else self.Minv)
            if self.device_momenta and self.mass_kind != 0:
                self.ctx.svc_batch_traj_set_mass_chol(self.Mchol)
        self.ctx.svc_batch_traj_begin()
        gr = {"q": self.q, "U": U, "commit": lambda acc, g1: self.ctx.svc_batch_traj_commit(acc)}
        if self.device_momenta:
            def draw():
                z = self._normals()
                return z, 0.5 * (z * z).sum(1)           # p0 = chol(M) z  =>  1/2 p0^T M^-1 p0 = 1/2 |z|^2

            def trajectory(jit, z):
                q1, K1, U1, failed = self.ctx.svc_batch_traj_z(self.hyper, True, self.eps * jit, self.L, z)
                return q1, K1, U1, failed, None
            gr.update(draw=draw, trajectory=trajectory, kinetic_end=lambda K1: K1)
        else:
            def trajectory(jit, p0):
                q1, p1, U1, failed = self.ctx.svc_batch_traj(self.hyper, True, self.eps * jit, self.L, p0)
                return q1, p1, U1, failed, None
            gr.update(draw=self._draw, trajectory=trajectory, kinetic_end=self.kinetic)
        return self._sample(gr, sample_size, t_start, jittered=True)


class BatchedHMCSeparable(LockStepHMC):
    """B independent HMC chains of the SEPARABLE model of one subject in lock-step: every leapfrog step evaluates
    ``logpos.nlogpos_obj`` and its gradient for all chains with one launch sequence (``nmgp_sep_batch_eval``: the chains' B*M
    blocks ``wB[p] K_x + sigma2 I`` form one batch of the blocked Cholesky).  The sampler call of ``Separable_model.py:209`` /
    ``Separable_model_mpiKAISER.py:281`` for B chains at once; chain b reproduces ``HMCSampler(potential_func=logpos.nlogpos_obj,
    ...)`` started from the same state with the same random stream.  The leapfrog update runs on the host (P = 2N + T + 1).
    ``M=`` a :class:`SeparablePriorMetric` (from :func:`separable_prior_metric`) selects the whitened-momentum loop -- the metric
    under which this model's chains mix; ``step_jitter`` as in :class:`BatchedHMC`, in that loop only: without a prior metric it is
    IGNORED.
    SEVERAL SUBJECTS: ``x`` [S, N] with ``Y`` [S, N, M] puts B / S consecutive chains on each subject (``nmgp_sep_batch_set_subjects_
    chains``: chain b belongs to subject b // (B / S)); identity, diagonal or dense mass only -- a prior metric belongs to one subject."""

    KEYS = SEP_HYPER_KEYS

    def __init__(self, x, Y, hyper_pars, init_positions, step_size=2e-4, num_steps_in_leap=20, seed=None, ctx=None, M=None, Minv=None,
                 step_jitter=0.0):
        from . import _lib
        super().__init__(init_positions, step_size, num_steps_in_leap, seed, M, Minv)
        self.step_jitter = float(step_jitter)
        self.jitter_rng = _jitter_rng(seed)
        self.ctx = ctx if ctx is not None else _lib.default_context()
        self.hyper = np.array([float(hyper_pars[k]) for k in self.KEYS])
        x, Y = np.asarray(x, dtype=np.float64), np.asarray(Y, dtype=np.float64)
        if x.ndim == 2:
            S = x.shape[0]
            if Y.ndim != 3 or Y.shape[0] != S:
                raise ValueError("x [S, N] needs Y [S, N, M]; got %s, %s" % (x.shape, Y.shape))
            if self.B % S:
                raise ValueError("the number of chains %d is not a multiple of the number of subjects %d" % (self.B, S))
            if self.mass_kind == 4:
                raise ValueError("a SeparablePriorMetric belongs to ONE subject's prior factors: with several subjects use the identity, "
                                 "a diagonal or a dense mass matrix (no per-subject prior metric yet)")
            self.ctx.set_data(x[0], Y[0])
            self.ctx.sep_batch_set_subjects(x, Y, self.B // S)
        else:
            self.ctx.set_data(x, Y)

    def potential_and_grad(self, q):
        """U [B] and dU/dq [B, P]; a chain whose covariance stays numerically singular after the jitter retries gets U = inf."""
        out, g, status = self.ctx.sep_batch_eval(q, self.hyper, True, True)
        return _potential_and_grad(out, g, (status < 0) | ~np.isfinite(out[:, 0]))

    def run(self, sample_size):
        """With ``M=`` a :class:`SeparablePriorMetric` the chains carry the whitened momentum u = L_blk^T p (as the device-resident
        nonseparable sampler does): draw u = (I + U lam U^T)^1/2 z with K0 = 1/2 |z|^2, kick u -= c L_blk^T g, drift
        q += eps L_blk (I + U lam U^T)^-1 u, kinetic energy 1/2 u^T (I + U lam U^T)^-1 u -- triangular PRODUCTS with the prior
        factors only, on the host (:func:`_leapfrog`), around one batched evaluation on the GPU per leapfrog step, with
        ``step_jitter``.  Any other mass matrix: :meth:`LockStepHMC.run`, which IGNORES ``step_jitter``."""
        if self.mass_kind != 4:
            return super().run(sample_size)
        t_start = time.perf_counter()
        met = self.metric

        def draw():
            z = self._normals()
            return met.root(z), 0.5 * (z * z).sum(1)
        group = self._host_group(draw, lambda g: met.apply(g, True), lambda u: met.apply(met.W(u), False), met.kinetic)
        return self._sample(group, sample_size, t_start, jittered=True)


# ---- Hadamard form of the nonseparable model (irregularly observed outputs) -------------------------------------------------------
class _HadamardSubject:
    """One Hadamard subject (x [N], indx [N], y [N]) on a context: the batched objective of ``hadamard.nlogpos_obj_hadamard_SVC``."""

    HYPER_KEYS = SVC_HYPER_KEYS

    def _bind(self, x, indx, y, hyper_pars, ctx):
        from . import _lib
        self.ctx = ctx if ctx is not None else _lib.default_context()
        self.hyper = np.array([float(hyper_pars[k]) for k in self.HYPER_KEYS])
        self.x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
        self.indx = np.ascontiguousarray(np.asarray(indx).reshape(-1), dtype=np.int32)
        self.y = np.ascontiguousarray(y, dtype=np.float64).reshape(-1)

    def _eval(self, P):
        self.ctx.had_set_data(self.x, self.indx, self.y)       # (a no-op while this subject is the resident one)
        return self.ctx.had_batch_eval(P, self.hyper, True, True)


class HadamardMAP(_HadamardSubject, LockStepMAP):
    """B restarts of the MAP loop on ``logpos.nlogpos_obj_hadamard_SVC`` in lock-step: host-side Adam (the arithmetic of
    ``torch.optim.Adam``, row by row), every iteration ONE ``nmgp_had_batch_eval`` for all restarts.  ``init_pars`` [B, N(1+T)+1]."""

    def __init__(self, x, indx, y, hyper_pars, init_pars, lr=2e-1, ctx=None):
        LockStepMAP.__init__(self, init_pars, lr=lr)
        self._bind(x, indx, y, hyper_pars, ctx)

    def value_and_grad(self, P):
        return self._eval(P)


class _HadamardNonCohort:
    """What a cohort driver (:class:`_HadamardCohort`) asks of its MODEL, here the nonseparable one: the hyper-parameter keys, the
    ``Context`` entry of a set's evaluation, the model's name in the resident families (``nmgp_had_subjects_adam_*``,
    ``nmgp_had_subjects_traj_*``), how per-subject vectors are packed into / unpacked from the entry's padded layout, and the cohort
    predictor.  The MAP driver and the HMC driver of a model both take them from here."""

    HYPER_KEYS = SVC_HYPER_KEYS
    EVAL = "had_subjects_eval"
    MODEL = "non"

    @staticmethod
    def _pack(vectors, nobs, M):
        from . import hadamard
        return hadamard.cohort_pack(vectors, nobs, M)

    @staticmethod
    def _unpack(P, nobs, M, k):
        from . import hadamard
        return hadamard.cohort_unpack(P, nobs, M, k)

    @staticmethod
    def _predict(ctx, hyper, draws, xs, indx_star):
        from . import hadamard
        return hadamard.cohort_predict(ctx, draws, xs, hyper, indx_star=indx_star)


class _HadamardCohort:
    """A cohort of ragged Hadamard subjects on the device, under the model a mixin names (:class:`_HadamardNonCohort`): buckets of
    similar size (``hadamard.cohort_buckets``), one subject set (``nmgp_had_set_subjects``) per bucket on a ``Context`` of its own,
    held until :meth:`close`.  What the cohort MAP loop and the cohort sampler share."""

    def _bind(self, subjects, hyper_pars, k, max_flop_waste, ctxs, evaluators):
        """Sets ``nobs``, ``M``, ``k``, ``hyper``, ``buckets`` and ``ctxs`` and puts every bucket's subjects on its context (with
        ``evaluators`` no context is created).  Returns the subjects as arrays and, per bucket, the evaluation of the entry's
        padded rows -> ``(out, grad, status)``: the model's ``*_subjects_eval`` on the set, or the caller's evaluator."""
        from . import hadamard
        subjects = [(np.ascontiguousarray(x, dtype=np.float64).reshape(-1), np.asarray(indx).reshape(-1).astype(np.int32),
                     np.ascontiguousarray(y, dtype=np.float64).reshape(-1)) for x, indx, y in subjects]
        self.nobs = [s[0].shape[0] for s in subjects]
        Ms = sorted({int(np.unique(s[1]).shape[0]) for s in subjects})
        if len(Ms) != 1:
            raise ValueError("the subjects have different numbers of distinct labels: %s" % Ms)
        self.M, self.k = Ms[0], k
        self.hyper = np.array([float(hyper_pars[key]) for key in self.HYPER_KEYS])
        self.buckets = hadamard.cohort_buckets(self.nobs, max_flop_waste)
        for name, given in (("contexts", ctxs), ("evaluators", evaluators)):
            if given is not None and len(given) != len(self.buckets):
                raise ValueError("%d %s for %d buckets" % (len(given), name, len(self.buckets)))
        self._own_ctxs = ctxs is None and evaluators is None
        self.ctxs = []
        if evaluators is not None:
            return subjects, list(evaluators)
        from . import _lib
        self.ctxs = list(ctxs) if ctxs is not None else [_lib.Context() for _ in self.buckets]
        for ctx, idx in zip(self.ctxs, self.buckets):
            ctx.had_set_subjects([subjects[s][0] for s in idx], [subjects[s][1] for s in idx], [subjects[s][2] for s in idx], M=self.M)
        return subjects, [(lambda P, ctx=ctx: getattr(ctx, self.EVAL)(P, self.hyper, True, True, k)) for ctx in self.ctxs]

    def close(self):
        """Drops the sets; closes the contexts this object created itself."""
        for ctx in self.ctxs:
            if self._own_ctxs:
                ctx.close()
            elif ctx.h:
                ctx.had_clear_subjects()
        self.ctxs = []

    def predict(self, pars, xs, indx_star=None):
        """MAP prediction (one draw, no noise) for every subject at its own new inputs, on the contexts and sets this object holds:
        ONE cohort prediction call of the model (``nmgp_predsample_had_subjects`` / ``nmgp_predsample_hads_subjects`` /
        ``nmgp_predict_hadst_subjects``) per bucket.  ``pars[s]`` ``[P_s]`` (or ``[k, P_s]`` as :meth:`run` returns them: row 0 is
        used), ``xs[s]`` ``[S_s]``, ``indx_star[s]`` ``[S_s]`` labels or None (all M outputs).  Returns a list, in the caller's subject
        order, of ``(mean [S_s(, M)], var, star [S_s, width], status)``; the stationary model has no ``star``."""
        if not (len(pars) == len(xs) == len(self.nobs)) or (indx_star is not None and len(indx_star) != len(self.nobs)):
            raise ValueError("pars, xs (and indx_star) must hold one entry per subject")
        out = [None] * len(self.nobs)
        for ctx, idx in zip(self.ctxs, self.buckets):
            res = self._predict(ctx, self.hyper, [np.atleast_2d(np.asarray(pars[s], dtype=np.float64))[:1] for s in idx],
                                [xs[s] for s in idx], None if indx_star is None else [indx_star[s] for s in idx])
            for s, r in zip(idx, res):
                out[int(s)] = tuple(a[0] for a in r[:-1]) + (int(r[-1][0]),)
        return out

    def _rows(self, idx):
        """columns of the caller's [.., S k] order that a bucket's rows fill"""
        return (np.asarray(idx)[:, None] * self.k + np.arange(self.k)[None, :]).reshape(-1)


class _HadamardCohortLoop(_HadamardCohort):
    """The cohort MAP loop shared by the three Hadamard models: the buckets and sets of :class:`_HadamardCohort`, ONE
    ``*_subjects_eval`` per bucket and Adam iteration, :class:`LockStepMAP`'s update on the rows of the entry's layout -- or, with
    ``device_resident=True`` (the default: faster at every measured point, README), the same iterations with parameters and moments
    on the device, ``iters_per_call`` of them per call (``nmgp_had_subjects_adam``), bit for bit the host loop's results."""

    def __init__(self, subjects, hyper_pars, init_pars, lr=2e-1, chains_per_subject=1, max_flop_waste=0.5, ctxs=None,
                 device_resident=True, iters_per_call=50, evaluators=None):
        """``device_resident=True``: parameters, gradients and Adam's moments stay in HBM (``nmgp_had_subjects_adam``), every bucket
        advances ``iters_per_call`` iterations per call with ONE synchronisation, and only the verbose tuples come back -- the same
        bits as ``device_resident=False``, the host loop over ``*_subjects_eval`` that DEFINES the arithmetic (see :meth:`run`).
        ``evaluators``: one callable per bucket, padded rows -> ``(out, grad, status)``, instead of contexts (host loop only; no
        context is created).  ``iters_per_call`` may be changed between two calls of :meth:`run`; ``device_resident`` must NOT be
        changed after the first one -- Adam's moments and iteration count live either on the host or on the device and are not
        carried over (:meth:`run` raises ``RuntimeError``)."""
        k = int(chains_per_subject)
        self.device_resident = bool(device_resident) and evaluators is None
        self._first_run_resident = None          # the loop the first run() took
        self.iters_per_call = int(iters_per_call)
        if self.iters_per_call < 1:
            raise ValueError("iters_per_call must be positive")
        subjects = list(subjects)
        if k < 1 or len(subjects) < 1 or len(init_pars) != len(subjects):
            raise ValueError("subjects and init_pars must be lists of one positive length, chains_per_subject >= 1")
        _, evals = self._bind(subjects, hyper_pars, k, max_flop_waste, ctxs, evaluators)
        self.maps = []
        for idx, ev in zip(self.buckets, evals):
            m = LockStepMAP(self._pack([init_pars[s] for s in idx], [self.nobs[s] for s in idx], self.M), lr=lr)
            if m.P.shape[0] != len(idx) * k:
                raise ValueError("init_pars must hold chains_per_subject = %d vectors per subject" % k)
            m.value_and_grad = ev
            m.begun = False            # the resident loop: nmgp_had_subjects_adam_begin has been called for this bucket
            self.maps.append(m)

    def run(self, N_opt, callback=None):
        """Returns (list of per-subject pars [k, P_s], target_value_hist [N_opt, S k] = -NegLog per iteration, alive [S k]), rows and
        columns in the caller's subject order.  ``callback(i, hist[i])`` is called once per iteration, in order; under the resident
        loop (``device_resident=True``) the callbacks ARRIVE LATE: those of a block of ``iters_per_call`` iterations are made after
        the block, when the device is already that far."""
        B = len(self.nobs) * self.k
        hist = np.zeros((N_opt, B))
        if self._first_run_resident is None:
            self._first_run_resident = bool(self.device_resident)
        elif self._first_run_resident != bool(self.device_resident):
            raise RuntimeError("device_resident was changed after the first run(): Adam's moments and iteration count are not carried "
                               "between the host loop and the device")
        if self.device_resident:
            return self._run_resident(N_opt, callback, hist)
        for i in range(N_opt):
            for m, idx in zip(self.maps, self.buckets):
                neglog, _ = m.step()
                hist[i, self._rows(idx)] = -neglog
            if callback is not None:
                callback(i, hist[i])
        pars, alive = [None] * len(self.nobs), np.zeros(B, dtype=bool)
        for m, idx in zip(self.maps, self.buckets):
            alive[self._rows(idx)] = m.alive
            for s, p in zip(idx, self._unpack(m.P, [self.nobs[s] for s in idx], self.M, self.k)):
                pars[int(s)] = p
        return pars, hist, alive

    def _run_resident(self, N_opt, callback, hist):
        """:meth:`run` with parameters and moments on the device: blocks of at most ``iters_per_call`` iterations per bucket and call
        (``nmgp_had_subjects_adam``), ``hist`` from the returned tuples -- ``-out[:, 0]``, ``-inf`` where the row is NaN, what the
        host loop records -- the callbacks of a block after the block, and ONE fetch of the parameters at the end.  A second
        :meth:`run` goes on from the resident state, as the host loop goes on from its own."""
        for m, ctx in zip(self.maps, self.ctxs):
            if not m.begun:
                ctx.had_subjects_adam_begin(self.MODEL, m.P, self.hyper, True, self.k)
                m.begun = True
        from . import _lib
        width = _lib.Context._COHORT_TRAJ_MODELS[self.MODEL][2]           # values per chain and iteration in the history
        step = min([self.iters_per_call] + [max(1, _lib.HAD_ADAM_HIST_MAX // (m.P.shape[0] * width)) for m in self.maps])
        for i0 in range(0, N_opt, step):
            n = min(step, N_opt - i0)
            for m, ctx, idx in zip(self.maps, self.ctxs, self.buckets):
                out, m.alive = ctx.had_subjects_adam(n, m.lr, m.b1, m.b2, m.eps)
                m.t += n
                v = out[:, :, 0]
                hist[i0:i0 + n, self._rows(idx)] = np.where(np.isnan(v), -np.inf, -v)
            if callback is not None:
                for i in range(i0, i0 + n):
                    callback(i, hist[i])
        pars, alive = [None] * len(self.nobs), np.zeros(hist.shape[1], dtype=bool)
        for m, ctx, idx in zip(self.maps, self.ctxs, self.buckets):
            m.P = ctx.had_subjects_adam_get_pars()
            alive[self._rows(idx)] = m.alive
            for s, p in zip(idx, self._unpack(m.P, [self.nobs[s] for s in idx], self.M, self.k)):
                pars[int(s)] = p
        return pars, hist, alive


class HadamardCohortMAP(_HadamardNonCohort, _HadamardCohortLoop):
    """The MAP loop of :class:`HadamardMAP` for a cohort of subjects of RAGGED size: ``subjects`` is a list of ``(x, indx, y)``,
    ``init_pars`` a list of ``[k, P_s]`` (k = ``chains_per_subject`` restarts of subject s, ``P_s = N_s (1 + T) + 1``).  The subjects
    are split into buckets of similar size (``hadamard.cohort_buckets(nobs, max_flop_waste)``); every bucket is one subject set
    (``nmgp_had_set_subjects``, padded to the bucket's largest subject) on a ``Context`` of its own, held for the whole run, and
    every Adam iteration makes ONE ``nmgp_had_subjects_eval`` per bucket, followed by :class:`LockStepMAP`'s update on the padded
    rows -- padded slots have zero gradient and therefore never move.  ``ctxs``: one context per bucket (default: new ones)."""


class BatchedHMCHadamard(_HadamardSubject, LockStepHMC):
    """B independent HMC chains of the Hadamard nonseparable model of one subject in lock-step: every leapfrog step evaluates
    ``logpos.nlogpos_obj_hadamard_SVC`` and its gradient for all chains with one ``nmgp_had_batch_eval``.  The leapfrog update
    runs on the host; identity, diagonal or dense mass matrix through the base class.  Chain b reproduces a one-chain run
    started from the same state with seed ``seed + b``."""

    def __init__(self, x, indx, y, hyper_pars, init_positions, step_size=1e-4, num_steps_in_leap=20, seed=None, ctx=None, M=None,
                 Minv=None):
        LockStepHMC.__init__(self, init_positions, step_size, num_steps_in_leap, seed, M, Minv)
        if self.mass_kind >= 3:
            raise NotImplementedError("the prior-factor metrics belong to the complete-data models")
        self._bind(x, indx, y, hyper_pars, ctx)

    def potential_and_grad(self, q):
        """U [B] and dU/dq [B, P]; a chain whose covariance is not positive definite (or not finite) gets U = inf."""
        out, g, status = self._eval(q)
        return _potential_and_grad(out, g, (status != 0) | ~np.isfinite(out[:, 0]))


# ---- Hadamard form of the separable model (one cross-output matrix shared by all observations) -------------------------------------
class _HadamardSepSubject(_HadamardSubject):
    """One Hadamard subject on a context under the separable model: the batched objective of ``hadamard_sep.nlogpos_obj_hadamard``."""

    HYPER_KEYS = SEP_HYPER_KEYS

    def _eval(self, P):
        self.ctx.had_set_data(self.x, self.indx, self.y)       # (a no-op while this subject is the resident one)
        return self.ctx.hads_batch_eval(P, self.hyper, True, True)


class HadamardSepMAP(_HadamardSepSubject, LockStepMAP):
    """B restarts of the MAP loop on ``logpos.nlogpos_obj_hadamard`` in lock-step: host-side Adam (the arithmetic of
    ``torch.optim.Adam``, row by row), every iteration ONE ``nmgp_hads_batch_eval`` for all restarts.  ``init_pars`` [B, 2N+T+1]."""

    def __init__(self, x, indx, y, hyper_pars, init_pars, lr=2e-1, ctx=None):
        LockStepMAP.__init__(self, init_pars, lr=lr)
        self._bind(x, indx, y, hyper_pars, ctx)

    def value_and_grad(self, P):
        return self._eval(P)


class _HadamardSepCohort:
    """:class:`_HadamardNonCohort`'s hooks for the separable model: the hyper-parameter keys of the per-subject driver,
    ``nmgp_hads_subjects_eval``, the padded layout of ``hadamard_sep.cohort_pack`` and ``hadamard_sep.cohort_predict``."""

    HYPER_KEYS = SEP_HYPER_KEYS
    EVAL = "hads_subjects_eval"
    MODEL = "sep"

    @staticmethod
    def _pack(vectors, nobs, M):
        from . import hadamard_sep
        return hadamard_sep.cohort_pack(vectors, nobs, M)

    @staticmethod
    def _unpack(P, nobs, M, k):
        from . import hadamard_sep
        return hadamard_sep.cohort_unpack(P, nobs, M, k)

    @staticmethod
    def _predict(ctx, hyper, draws, xs, indx_star):
        from . import hadamard_sep
        return hadamard_sep.cohort_predict(ctx, draws, xs, hyper, indx_star=indx_star)


class HadamardSepCohortMAP(_HadamardSepCohort, _HadamardCohortLoop):
    """:class:`HadamardCohortMAP`'s loop under the separable model, against :class:`HadamardSepMAP` subject by subject:
    ``init_pars[s]`` ``[k, 2 N_s + T + 1]``, ONE ``nmgp_hads_subjects_eval`` per bucket and Adam iteration on the padded layout
    (padded slots have zero gradient and never move).  :meth:`predict` is ``hadamard_sep.cohort_predict`` per bucket."""


class BatchedHMCHadamardSep(_HadamardSepSubject, LockStepHMC):
    """B independent HMC chains of the separable Hadamard model of one subject in lock-step: every leapfrog step evaluates
    ``logpos.nlogpos_obj_hadamard`` and its gradient for all chains with one ``nmgp_hads_batch_eval``.  The leapfrog update runs on
    the host; identity, diagonal or dense mass matrix through the base class.  Chain b reproduces a one-chain run started from the
    same state with seed ``seed + b``."""

    def __init__(self, x, indx, y, hyper_pars, init_positions, step_size=1e-4, num_steps_in_leap=20, seed=None, ctx=None, M=None,
                 Minv=None):
        LockStepHMC.__init__(self, init_positions, step_size, num_steps_in_leap, seed, M, Minv)
        if self.mass_kind >= 3:
            raise NotImplementedError("the prior-factor metrics belong to the complete-data models")
        self._bind(x, indx, y, hyper_pars, ctx)

    potential_and_grad = BatchedHMCHadamard.potential_and_grad


# ---- Hadamard form of the stationary model (the LMC baseline: T + 3 parameters, no GP prior) --------------------------------------
class _HadamardStaSubject(_HadamardSubject):
    """One Hadamard subject on a context under the stationary model: the batched objective of ``hadamard_sta.nlogpos_obj_hadamard_S``."""

    HYPER_KEYS = STA_HYPER_KEYS

    def _eval(self, P):
        self.ctx.had_set_data(self.x, self.indx, self.y)       # (a no-op while this subject is the resident one)
        return self.ctx.hadst_batch_eval(P, self.hyper, True, True)


class HadamardStaMAP(_HadamardStaSubject, LockStepMAP):
    """B restarts of the MAP loop on ``logpos.nlogpos_obj_hadamard_S`` in lock-step: host-side Adam (the arithmetic of
    ``torch.optim.Adam``, row by row), every iteration ONE ``nmgp_hadst_batch_eval`` for all restarts.  ``init_pars`` [B, T+3]."""

    def __init__(self, x, indx, y, hyper_pars, init_pars, lr=2e-1, ctx=None):
        LockStepMAP.__init__(self, init_pars, lr=lr)
        self._bind(x, indx, y, hyper_pars, ctx)

    def value_and_grad(self, P):
        return self._eval(P)


class _HadamardStaCohort:
    """:class:`_HadamardNonCohort`'s hooks for the stationary model: the hyper-parameter keys of the per-subject driver,
    ``nmgp_hadst_subjects_eval``, rows stacked as they are (the ``T + 3`` vector has no per-observation part: every slot is real)
    and ``hadamard_sta.cohort_predict`` (no starred values: ``(mean, var, status)`` per subject)."""

    HYPER_KEYS = STA_HYPER_KEYS
    EVAL = "hadst_subjects_eval"
    MODEL = "sta"

    @staticmethod
    def _pack(vectors, nobs, M):
        return np.concatenate([np.atleast_2d(np.asarray(v, dtype=np.float64)) for v in vectors], axis=0)

    @staticmethod
    def _unpack(P, nobs, M, k):
        return [np.array(P[s * k:(s + 1) * k]) for s in range(len(nobs))]

    @staticmethod
    def _predict(ctx, hyper, draws, xs, indx_star):
        from . import hadamard_sta
        return hadamard_sta.cohort_predict(ctx, draws, xs, indx_star=indx_star)


class HadamardStaCohortMAP(_HadamardStaCohort, _HadamardCohortLoop):
    """:class:`HadamardCohortMAP`'s loop under the stationary model, against :class:`HadamardStaMAP` subject by subject:
    ``init_pars[s]`` ``[k, T + 3]``, the update of the per-subject driver (every entry moves, ``tilde_sigma`` included, as there),
    ONE ``nmgp_hadst_subjects_eval`` per bucket and Adam iteration.  :meth:`predict` is ``hadamard_sta.cohort_predict`` per bucket."""


class BatchedHMCHadamardSta(_HadamardStaSubject, LockStepHMC):
    """B independent HMC chains of the stationary Hadamard model of one subject in lock-step: every leapfrog step evaluates
    ``logpos.nlogpos_obj_hadamard_S`` and its gradient for all chains with one ``nmgp_hadst_batch_eval``.  The leapfrog update runs
    on the host; identity, diagonal or dense mass matrix through the base class (with T + 3 parameters and no GP prior a dense mass
    is all the metric the model needs).  Chain b reproduces a one-chain run started from the same state with seed ``seed + b``."""

    def __init__(self, x, indx, y, hyper_pars, init_positions, step_size=1e-2, num_steps_in_leap=20, seed=None, ctx=None, M=None,
                 Minv=None):
        LockStepHMC.__init__(self, init_positions, step_size, num_steps_in_leap, seed, M, Minv)
        if self.mass_kind >= 3:
            raise NotImplementedError("the prior-factor metrics belong to the complete-data models")
        self._bind(x, indx, y, hyper_pars, ctx)

    potential_and_grad = BatchedHMCHadamard.potential_and_grad

    # Under a dense mass the base class takes all chains' momenta through ONE matrix-matrix product, whose summation order depends
    # on the number of rows B.  P = T + 3 is small: here every chain goes through its own matrix-vector product, so chain b keeps
    # its bits whatever B is, under a dense mass too.
    def draw_momenta(self):
        if self.mass_kind != 2:
            return LockStepHMC.draw_momenta(self)
        return np.stack([self.Mchol @ r.standard_normal(self.P) for r in self.rngs])

    def velocity(self, p):
        if self.mass_kind != 2:
            return LockStepHMC.velocity(self, p)
        return np.stack([self.Minv @ row for row in p])


# ---- HMC for a cohort of ragged Hadamard subjects: the sampler between the cohort's MAP and its predictive bands ---------------------
class _HadamardCohortHMC(_HadamardCohort):
    """Lock-step HMC for a cohort of ragged Hadamard subjects, shared by the three models: the buckets, sets and contexts of
    :class:`_HadamardCohort`, the model's pack / unpack hooks, every bucket a group of :func:`_metropolis`, :class:`LockStepHMC`'s
    arithmetic on the rows of the entry's padded layout with a step size per subject.  ``init_positions[s]`` ``[k, P_s]`` (the same k for every subject); ``step_size`` a scalar or ``[S]``;
    ``mass`` None, a list of ``diag(M)`` ``[P_s]`` per subject, or ``"prior"`` (below); ``step_jitter`` as :class:`BatchedHMC` (one
    factor per iteration for all subjects, from a generator of its own).  Chain k of subject s draws from ``default_rng(seed + s k_total + k)`` in
    :class:`HMCSampler`'s order -- ``P_s`` standard normals of the REAL length, then the uniform of the accept test -- so a subject's
    draws do not depend on who else is in the cohort and equal those of the per-subject sampler with ``seed + s k_total``.

    ``device_resident=True``: positions, momenta and gradients stay in HBM for a whole trajectory (``nmgp_had_subjects_traj``: one
    chunked evaluation per leapfrog step, masked elementwise kernels between them, one synchronisation per trajectory and bucket).
    ``device_resident=False``: the host loop over ``*_subjects_eval`` that DEFINES the arithmetic -- padded momentum is 0, the
    kinetic energy is ``0.5 * (p * v).sum()`` over the real slots of a row; the resident loop with ``device_kinetic=False``
    reproduces it bit for bit.  ``device_kinetic=True`` takes the end point's kinetic energy from the device and 1/2 |z|^2 for the
    start.  ``evaluators``: one callable per bucket, padded rows -> ``(out, grad, status)``, instead of contexts (host loop only).

    ``mass="prior"`` (nonseparable and separable model; the stationary one has no GP prior: ``ValueError``): the PRIOR-FACTOR METRIC
    ``M^-1 = L_blk,s L_blk,s^T`` of :class:`PriorMetric` at rank 0, per subject, ``L_blk,s`` the block diagonal of the Cholesky factors
    of the subject's GP priors (``nmgp_had_subjects_traj_set_mass`` kind 2).  The chains' streams and their order are unchanged, so the
    ``P_s`` normals z ARE the whitened momentum: ``K0 = 1/2 |z|^2``, a step is ``u -= c eps_s L_blk,s^T g``, ``q += eps_s L_blk,s u``,
    and ``K1 = 1/2 |u1|^2`` over the real slots.  ``step_size`` is then a step in WHITENED coordinates, where the prior is N(0, I):
    O(0.1), not the O(1e-4) the identity mass needs.  The host loop (``device_resident=False``, also with ``evaluators=``) DEFINES
    this arithmetic with ``L_blk,s`` built in NumPy (:meth:`_prior_factor`); the resident loop agrees with it to a tolerance, NOT bit
    for bit -- the summation order of a triangular product differs between NumPy's GEMM and the kernel's tiles."""

    @staticmethod
    def _prior_factor(x, alpha, beta):
        """chol(RBF(x; alpha, beta) + 1e-6 I) in NumPy, expression by expression the oracle's ``RBF_cov`` (kernels.py:24-43)"""
        xs = (np.asarray(x, dtype=np.float64) / beta).reshape(-1, 1)
        xn = (xs ** 2).sum(1).reshape(-1, 1)
        d = xn + xn.reshape(1, -1) - 2.0 * (xs @ xs.T)
        return np.linalg.cholesky(np.eye(xs.shape[0]) * 1e-6 + np.exp(-0.5 * d) * alpha ** 2)

    def _metric_apply(self, st, v, trans):
        """``L_blk,s v`` (``trans``: ``L_blk,s^T v``) on the real slots of the bucket's padded rows; +0.0 in the padded ones"""
        res = []
        with np.errstate(invalid="ignore"):
            rows = self._unpack(np.where(st["mask"], v, 0.0), st["nobs"], self.M, self.k)
        for (L0, L1), r in zip(st["factors"], rows):
            N, o = L0.shape[0], np.empty_like(r)
            A0, A1 = (L0.T, L1.T) if trans else (L0, L1)
            o[:, :N] = r[:, :N] @ A0.T
            if self.MODEL == "sep":
                o[:, N:2 * N] = r[:, N:2 * N] @ A1.T
                o[:, 2 * N:-1] = float(np.float32(self.hyper[8])) * r[:, 2 * N:-1]
            else:
                o[:, N:-1] = np.matmul(A1, r[:, N:-1].reshape(r.shape[0], N, -1)).reshape(r.shape[0], -1)
            o[:, -1] = r[:, -1]
            res.append(o)
        return self._pack(res, st["nobs"], self.M)

    def __init__(self, subjects, hyper_pars, init_positions, step_size=1e-4, num_steps_in_leap=20, seed=None, mass=None,
                 step_jitter=0.0, device_resident=True, device_kinetic=False, max_flop_waste=0.5, ctxs=None, evaluators=None):
        subjects = list(subjects)
        S = len(subjects)
        if S < 1 or len(init_positions) != S:
            raise ValueError("subjects and init_positions must be lists of one positive length")
        starts = [np.atleast_2d(np.array(v, dtype=np.float64)) for v in init_positions]
        k = starts[0].shape[0]
        if any(v.shape[0] != k for v in starts):
            raise ValueError("every subject must have the same number of chains")
        self.L = int(num_steps_in_leap)
        eps = np.asarray(step_size, dtype=np.float64)
        self.eps = np.full(S, float(eps)) if eps.ndim == 0 else eps.reshape(-1).copy()
        if self.eps.shape[0] != S or not np.all(np.isfinite(self.eps) & (self.eps > 0)):
            raise ValueError("step_size must be a positive scalar or one positive value per subject")
        self.prior_metric = isinstance(mass, str)
        if self.prior_metric:
            if mass != "prior" or self.MODEL == "sta":
                raise ValueError('mass="prior" is the only named mass, and the stationary model has no GP prior to take it from')
            mass = None
        if mass is not None and (len(mass) != S or any(np.shape(m) != (v.shape[1],) or np.any(np.asarray(m) <= 0) for m, v in zip(mass, starts))):
            raise ValueError("mass must hold one positive diag(M) [P_s] per subject")
        self.step_jitter = float(step_jitter)
        self.jitter_rng = _jitter_rng(seed)
        self.rngs = [np.random.default_rng(None if seed is None else seed + b) for b in range(S * k)]
        self.device_resident = bool(device_resident) and evaluators is None
        self.device_kinetic = bool(device_kinetic) and self.device_resident
        subjects, evals = self._bind(subjects, hyper_pars, k, max_flop_waste, ctxs, evaluators)
        # per bucket: the padded rows q, the mask of their real slots, and (with a mass) sqrt(diag M) and diag(M^-1) in that layout
        self.state = []
        for b, idx in enumerate(self.buckets):
            nb = [self.nobs[s] for s in idx]
            st = {"idx": [int(s) for s in idx], "nobs": nb, "q": self._pack([starts[s] for s in idx], nb, self.M), "eval": evals[b]}
            st["mask"] = self._pack([np.ones_like(starts[s]) for s in idx], nb, self.M) == 1.0
            st["mchol"] = st["minv"] = None
            if mass is not None:
                rows = lambda f: self._pack([np.tile(f(np.asarray(mass[s], dtype=np.float64)), (k, 1)) for s in idx], nb, self.M)
                st["mchol"] = rows(np.sqrt)
                st["minv"] = np.where(st["mask"], rows(lambda m: 1.0 / m), 1.0)
            if self.prior_metric and not self.device_resident:
                st["factors"] = [(self._prior_factor(subjects[s][0], self.hyper[1], self.hyper[2]),
                                  self._prior_factor(subjects[s][0], self.hyper[4], self.hyper[5])) for s in idx]
            if self.ctxs:
                st["ctx"] = self.ctxs[b]
            self.state.append(st)

    def close(self):
        """Ends the trajectories and drops the sets; closes the contexts this object created itself."""
        for ctx in self.ctxs:
            if ctx.h:
                ctx.had_subjects_traj_end()
        _HadamardCohort.close(self)

    @staticmethod
    def _potential(res):
        """U [B] and dU/dq [B, Pmax] of an evaluation; a chain whose potential is undefined gets U = inf and a zero gradient"""
        out, g, status = res
        return _potential_and_grad(out, g, (np.asarray(status) != 0) | ~np.isfinite(out[:, 0]))

    def _kinetic(self, st, p, minv=True):
        """0.5 * (p * v).sum() over the real slots of each row, v = diag(M^-1) p (``minv=False``: v = p)"""
        v = p if st["minv"] is None or not minv else p * st["minv"]
        return np.array([0.5 * (p[z][m] * v[z][m]).sum() for z, m in enumerate(st["mask"])])

    def _host_traj(self, st, eps, p0):
        """:func:`_leapfrog` on the bucket's padded rows from ``st["q"]``, ``st["U"]``, ``st["g"]`` with a step size per row; padded
        slots stay as they are.  Under the prior metric p is the whitened momentum u: the gradient goes through L_blk^T, the
        velocity through L_blk."""
        if self.prior_metric:
            kick, drift = (lambda g: self._metric_apply(st, g, True)), (lambda u: self._metric_apply(st, u, False))
        else:
            kick, drift = (lambda g: g), (lambda p: p if st["minv"] is None else st["minv"] * p)
        return _leapfrog(st["q"], p0, st["U"], st["g"], eps[:, None], self.L, lambda q: self._potential(st["eval"](q)), kick, drift,
                         st["mask"])

    def _group(self, st, n):
        """Makes the bucket's state ``st`` a group of :func:`_metropolis`: begins its trajectories (resident) or evaluates its start
        (host), and names how it draws, runs a trajectory and commits."""
        k, mask, resident, dk = self.k, st["mask"], self.device_resident, self.device_kinetic
        if resident:
            out, status = st["ctx"].had_subjects_traj_begin(self.MODEL, st["q"], self.hyper, True, k)
            st["U"], _ = self._potential((out, None, status))
            st["ctx"].had_subjects_traj_set_mass(st["minv"], prior=self.prior_metric)
        else:
            st["U"], st["g"] = self._potential(st["eval"](st["q"]))
        real = [int(m.sum()) for m in mask]

        def draw():
            z = np.zeros(mask.shape)
            for r, (rng, m) in enumerate(zip(st["rngs"], mask)):
                z[r, m] = rng.standard_normal(real[r])
            p0 = z if st["mchol"] is None else np.where(mask, z * st["mchol"], 0.0)
            return p0, self._kinetic(st, z, minv=False) if dk else self._kinetic(st, p0)

        def trajectory(jit, p0):
            eps = self.eps[st["idx"]] * jit            # per subject
            if resident:
                q1, p1, K1, U1, failed = st["ctx"].had_subjects_traj(eps, self.L, p0, want_p1=not dk, want_kin=dk)
                return q1, (K1 if dk else p1), U1, failed, None
            q1, p1, U1, g1, failed = self._host_traj(st, np.repeat(eps, k), p0)
            return q1, p1, U1, failed, g1

        def commit(acc, g1):
            if resident:
                st["ctx"].had_subjects_traj_commit(acc)
            else:
                st["g"] = np.where(acc[:, None], g1, st["g"])
        st.update(rows=self._rows(st["idx"]), draw=draw, trajectory=trajectory, commit=commit,
                  kinetic_end=(lambda K1: K1) if dk else (lambda p1: self._kinetic(st, p1)),
                  samples=[np.zeros((n, k, real[j * k])) for j in range(len(st["idx"]))],
                  split=lambda q: self._unpack(q, st["nobs"], self.M, k))
        st["rngs"] = [self.rngs[b] for b in st["rows"]]
        return st

    def run(self, sample_size):
        """Returns ``(samples, info)``: ``samples[s]`` ``[n, k, P_s]`` in the caller's subject order (what the three
        ``posterior_predict_hadamard*_cohort`` functions take), ``info`` with ``accept_rate`` ``[S k]``, ``energy_error`` ``[n, S k]``
        and ``timing`` as :class:`BatchedHMC`."""
        n, S = int(sample_size), len(self.nobs)
        t_start = time.perf_counter()
        groups = [self._group(st, n) for st in self.state]
        accepted, energy_err, timing = _metropolis(groups, n, S * self.k, t_start, self.step_jitter, self.jitter_rng)
        samples = [None] * S
        for st in self.state:
            for s, rec in zip(st["idx"], st["samples"]):
                samples[s] = rec
        return samples, {"accept_rate": accepted / max(n, 1), "energy_error": energy_err, "timing": timing}


class HadamardCohortHMC(_HadamardNonCohort, _HadamardCohortHMC):
    """:class:`_HadamardCohortHMC` under the nonseparable model: ``init_positions[s]`` ``[k, N_s (1 + T) + 1]``, against
    :class:`BatchedHMCHadamard` subject by subject; ``samples`` go to :func:`posterior_predict_hadamard_cohort`."""


class HadamardSepCohortHMC(_HadamardSepCohort, _HadamardCohortHMC):
    """:class:`_HadamardCohortHMC` under the separable model (keys, entry and layout of :class:`_HadamardSepCohort`):
    ``init_positions[s]`` ``[k, 2 N_s + T + 1]``, against :class:`BatchedHMCHadamardSep`; ``samples`` go to
    :func:`posterior_predict_hadamard_sep_cohort`."""


class HadamardStaCohortHMC(_HadamardStaCohort, _HadamardCohortHMC):
    """:class:`_HadamardCohortHMC` under the stationary model (keys, entry and layout of :class:`_HadamardStaCohort`; every slot of
    the ``T + 3`` vector is real): against :class:`BatchedHMCHadamardSta`; ``samples`` go to
    :func:`posterior_predict_hadamard_sta_cohort`."""


# ---- stationary (LMC) model, complete data: the baseline ----------------------------------------------------------------------------
class BatchedMAPStationary(LockStepMAP):
    """The MAP loop of ``Stationary_model_mpiKAISER.py`` (:func:`map_stationary` per subject) for ALL subjects of a rank, or B restarts
    of one subject, at once: every Adam iteration is ONE ``nmgp_sta_batch_eval`` -- the rows' B * M blocks as one batch of the blocked
    Cholesky.  Host-side Adam, row by row the arithmetic of :func:`map_stationary`.  ``xs`` [N] with ``Ys`` [N, M]: ``init_pars``
    [B, T+3] are B restarts of that subject.  ``xs`` [S, N] with ``Ys`` [S, N, M]: ``init_pars`` [S * chains_per_subject, T+3], row
    s * chains_per_subject + k being restart k of subject s (the subject set of ``nmgp_sep_batch_set_subjects_chains``).
    ``fix_tilde_sigma`` (default) zeroes column 1 of the gradient before Adam's update: the reference keeps ``tilde_sigma`` out of
    its optimiser ("fixed for correlation"), so ``pars[:, 1]`` stays at its initial value, bit for bit."""

    def __init__(self, xs, Ys, hyper_pars, init_pars, lr=1e-1, ctx=None, chains_per_subject=1, fix_tilde_sigma=True):
        from . import _lib
        super().__init__(init_pars, lr=lr)
        xs = np.ascontiguousarray(xs, dtype=np.float64)
        Ys = np.ascontiguousarray(Ys, dtype=np.float64)
        k = int(chains_per_subject)
        if xs.ndim == 1:
            if Ys.ndim != 2 or Ys.shape[0] != xs.shape[0] or k != 1:
                raise ValueError("xs [N] needs Ys [N, M] and chains_per_subject = 1 (the rows of init_pars are the restarts): %s, %s, k = %d"
                                 % (xs.shape, Ys.shape, k))
            M = Ys.shape[1]
        else:
            if xs.ndim != 2 or Ys.ndim != 3 or Ys.shape[:2] != xs.shape or k < 1 or self.P.shape[0] != xs.shape[0] * k:
                raise ValueError("xs [S, N], Ys [S, N, M] and init_pars [S * chains_per_subject, P] do not fit: %s, %s, %s, k = %d"
                                 % (xs.shape, Ys.shape, self.P.shape, k))
            M = Ys.shape[2]
        if self.P.shape[1] != M * (M + 1) // 2 + 3:
            raise ValueError("init_pars must be [B, T+3 = %d] for M = %d outputs, got %s" % (M * (M + 1) // 2 + 3, M, self.P.shape))
        self.ctx = ctx if ctx is not None else _lib.default_context()
        self.hyper = np.array([float(hyper_pars[key]) for key in STA_HYPER_KEYS])
        self.prior = True
        self.fix_tilde_sigma = bool(fix_tilde_sigma)
        if xs.ndim == 1:
            self.ctx.set_data(xs, Ys)
        else:
            self.ctx.set_data(xs[0], Ys[0])
            self.ctx.sta_batch_set_subjects(xs, Ys, k)

    def value_and_grad(self, P):
        """out [B, 5], grad [B, T+3] and a status that is 0 for every valid evaluation: jitter retries (status > 0) count as valid, a
        numerical failure (status < 0) marks the row dead for :func:`valid_rows`."""
        out, grad, status = self.ctx.sta_batch_eval(P, self.hyper, self.prior, True)
        if self.fix_tilde_sigma:
            grad[:, 1] = 0.0
        return out, grad, np.where(status < 0, status, 0)


class BatchedHMCStationary(LockStepHMC):
    """B independent HMC chains of the stationary (LMC) model in lock-step: every leapfrog step evaluates ``logpos.nlogpos_obj_S``
    and its gradient for all chains with one ``nmgp_sta_batch_eval``.  The sampler call of ``Stationary_model.py`` for B chains at
    once; the leapfrog update runs on the host (P = T + 3).  Identity, diagonal or dense mass matrix; the prior-factor metrics belong
    to the models with GP priors and are refused.  Chain b reproduces a one-chain run started from the same state with seed
    ``seed + b``, bit for bit, under a dense mass too (per-chain matrix-vector products, as :class:`BatchedHMCHadamardSta`).
    SEVERAL SUBJECTS: ``x`` [S, N] with ``Y`` [S, N, M] puts B / S consecutive chains on each subject (chain b belongs to subject
    b // (B / S)), as :class:`BatchedHMCSeparable`."""

    def __init__(self, x, Y, hyper_pars, init_positions, step_size=1e-2, num_steps_in_leap=20, seed=None, ctx=None, M=None, Minv=None):
        from . import _lib
        super().__init__(init_positions, step_size, num_steps_in_leap, seed, M, Minv)
        if self.mass_kind >= 3:
            raise NotImplementedError("the prior-factor metrics belong to the models with GP priors: the stationary model takes the "
                                      "identity, a diagonal or a dense mass matrix")
        self.ctx = ctx if ctx is not None else _lib.default_context()
        self.hyper = np.array([float(hyper_pars[k]) for k in STA_HYPER_KEYS])
        x, Y = np.asarray(x, dtype=np.float64), np.asarray(Y, dtype=np.float64)
        Mo = Y.shape[-1]
        if self.P != Mo * (Mo + 1) // 2 + 3:
            raise ValueError("init_positions must be [B, T+3 = %d] for M = %d outputs, got %s" % (Mo * (Mo + 1) // 2 + 3, Mo, self.q.shape))
        if x.ndim == 2:
            S = x.shape[0]
            if Y.ndim != 3 or Y.shape[0] != S:
                raise ValueError("x [S, N] needs Y [S, N, M]; got %s, %s" % (x.shape, Y.shape))
            if self.B % S:
                raise ValueError("the number of chains %d is not a multiple of the number of subjects %d" % (self.B, S))
            self.ctx.set_data(x[0], Y[0])
            self.ctx.sta_batch_set_subjects(x, Y, self.B // S)
        else:
            self.ctx.set_data(x, Y)

    def potential_and_grad(self, q):
        """U [B] and dU/dq [B, P]; a chain whose covariance stays numerically singular after the jitter retries gets U = inf."""
        out, g, status = self.ctx.sta_batch_eval(q, self.hyper, True, True)
        return _potential_and_grad(out, g, (status < 0) | ~np.isfinite(out[:, 0]))

    draw_momenta = BatchedHMCHadamardSta.draw_momenta
    velocity = BatchedHMCHadamardSta.velocity


# ---- the whole recipe behind one call ---------------------------------------------------------------------------------------------
def _sample_recipe(polish, build_metric, make_sampler, pars0, chains, iters, warm, warm_step, windows, window_iters, step_size,
                   step_candidates, target_accept, progress, segment):
    """Mode -> metric -> thermalising iterations -> (metric rebuilt at the chains' mean) x windows -> step search -> main run.
    polish(pars0) -> (mode, NegLog, |grad|, evaluations); build_metric(point, k) -> metric; make_sampler(positions, metric, eps, seed)
    -> an object with run(n) -> (samples [n, B, P], info).  Returns (samples [iters, B, P], info)."""
    say = progress if progress is not None else (lambda msg: None)
    info = {}
    t0 = time.time()
    mode, nl, gn, nev = polish(np.asarray(pars0, dtype=np.float64).reshape(-1))
    info["mode"] = {"pars": mode, "log_posterior": -nl, "whitened_gradient_norm": gn, "gradient_evaluations": nev, "seconds": time.time() - t0}
    say("mode: log posterior %.4f, whitened |grad| %.3g, %d evaluations, %.1f s" % (-nl, gn, nev, time.time() - t0))
    t0 = time.time()
    metric = build_metric(mode, 0)
    info["metric_at_the_mode"] = dict({k: v for k, v in metric.info.items() if k != "eigenvalues"}, rank=metric.rank, seconds=time.time() - t0)
    say("metric at the mode: rank %d, lam max %.3g, most negative %.3g, %.1f s" % (
        metric.rank, metric.info["lam_max"], metric.info["most_negative"], time.time() - t0))
    cur = np.repeat(mode[None], chains, 0)
    stages = []

    def stage(eps, n, seed, tag):
        hm = make_sampler(cur, metric, eps, seed)
        t1 = time.time()
        chunks, ees, acc, done = [], [], np.zeros(chains), 0
        while done < n:
            k = min(segment, n - done)
            s_, inf = hm.run(k)
            chunks.append(s_)
            ees.append(inf["energy_error"])
            acc += inf["accept_rate"] * k
            done += k
            if n > segment:
                say("  %s: %d / %d iterations, %.1f s, accept so far %.3f" % (tag, done, n, time.time() - t1, acc.sum() / (done * chains)))
        dt = time.time() - t1
        ee = np.concatenate(ees)
        st = {"stage": tag, "step_size": eps, "iterations": n, "seconds": dt, "accept_rate_mean": float(acc.sum() / (n * chains)),
              "accept_rate_by_chain": (acc / n).tolist(), "median_abs_dH": float(np.nanmedian(np.abs(ee))),
              "samples_per_s": n * chains / dt}
        stages.append(st)
        say("%s: %d iterations at eps %.3g in %.1f s, accept %.3f, median |dH| %.3g" % (tag, n, eps, dt, st["accept_rate_mean"], st["median_abs_dH"]))
        return np.concatenate(chunks), ee

    s = None
    if warm > 0:
        # all chains start AT the mode, where the first trajectories convert P / 2 units of kinetic into potential energy: the leapfrog
        # error of that transfer rejects every step worth having, so a few iterations at a small step come first
        s, _ = stage(warm_step, warm, 300, "warm-up")
        cur = s[-1]
    for wdw in range(int(windows)):
        center = (s[-max(10, s.shape[0] // 2):].mean((0, 1)) if s is not None else mode)
        t0 = time.time()
        metric = build_metric(center, 1 + wdw)
        say("window %d: metric at the chains' mean: rank %d, lam max %.3g, most negative %.3g, %.1f s" % (
            wdw, metric.rank, metric.info["lam_max"], metric.info["most_negative"], time.time() - t0))
        s, _ = stage(min(step_candidates), window_iters, 400 + wdw, "adaptation window %d" % wdw)
        cur = s[-1]
    if step_size == "auto":
        tried, best = [], None
        for eps in step_candidates:
            _, inf = make_sampler(cur, metric, eps, 200).run(6)
            a_ = float(inf["accept_rate"].mean())
            tried.append({"step_size": eps, "accept_rate_mean": a_, "median_abs_dH": float(np.nanmedian(np.abs(inf["energy_error"])))})
            say("step search: eps %.3g accept %.2f median |dH| %.3g" % (eps, a_, tried[-1]["median_abs_dH"]))
            if a_ >= target_accept:
                best = eps
            elif best is not None:
                break
        eps = best if best is not None else min(step_candidates)
        info["step_search"] = tried
    else:
        eps = float(step_size)
    S, ee = stage(eps, iters, 1, "main")
    info.update(step_size=eps, stages=stages, metric=metric, energy_error=ee, accept_rate=np.array(stages[-1]["accept_rate_by_chain"]))
    return S, info


def sample_nonseparable(x, Y, hyper_pars, pars0, chains=8, iters=1000, num_steps_in_leap=20, rank=64, polish=300, warm=40,
                        warm_step=0.03, windows=0, window_iters=50, step_size="auto", step_candidates=(0.05, 0.065, 0.08, 0.1, 0.12),
                        target_accept=0.7, step_jitter=0.2, seed=1, ctx=None, progress=None, segment=50):
    """The sampler call of ``Nonseparable_model.py:228-231`` for ``chains`` chains in lock-step, as the recipe under which it
    converges at N = 2048 (``tools/hmc_1000.py`` is the same recipe with its diagnostics): mode by metric-preconditioned
    L-BFGS from ``pars0`` (:func:`polish_map`), :class:`PriorMetric` there (:func:`prior_lowrank_metric`), ``warm`` thermalising
    iterations at ``warm_step``, optionally ``windows`` re-adaptations of the metric at the chains' mean, a step search for
    ``target_accept``, then ``iters`` iterations of :class:`BatchedHMC` with ``step_jitter``.  ``progress``: a callable for one-line
    messages.  Returns (samples [iters, chains, P], info: mode, metrics, stages, step_size, energy_error, accept_rate)."""
    from . import _lib
    ctx = ctx if ctx is not None else _lib.default_context()
    x, Y = np.asarray(x, dtype=np.float64), np.asarray(Y, dtype=np.float64)

    def make_sampler(pos, metric, eps, sd):
        return BatchedHMC(x, Y, hyper_pars, pos, step_size=eps, num_steps_in_leap=num_steps_in_leap, seed=sd + 1000 * seed, ctx=ctx, M=metric,
                          step_jitter=step_jitter)
    return _sample_recipe(lambda p: polish_map(x, Y, hyper_pars, p, maxiter=polish, rounds=8, rank=rank, probes=rank + 32, ctx=ctx,
                                               verbose=progress),
                          lambda q, k: prior_lowrank_metric(x, Y, hyper_pars, q, rank=rank, oversample=32, seed=7 + k, ctx=ctx,
                                                            batch=min(rank + 32, 128)),
                          make_sampler, pars0, chains, iters, warm, warm_step, windows, window_iters, step_size, step_candidates,
                          target_accept, progress, segment)


def sample_separable(x, Y, hyper_pars, pars0, chains=8, iters=1000, num_steps_in_leap=20, rank=64, polish=400, warm=50, warm_step=0.04,
                     windows=2, window_iters=50, step_size="auto", step_candidates=(0.08, 0.11, 0.15), target_accept=0.8,
                     step_jitter=0.2, seed=1, ctx=None, progress=None, segment=25, batch=16):
    """The same for the separable model (``Separable_model.py:209-210``; :class:`SeparablePriorMetric`, :class:`BatchedHMCSeparable`).
    ``windows`` defaults to 2: this posterior's mass sits far from its mode (the sigma(x) <-> B scale ridge), so the metric is
    rebuilt at the chains' mean after the warm-up (``tools/hmc_sep.py``)."""
    from . import _lib
    ctx = ctx if ctx is not None else _lib.default_context()
    x, Y = np.asarray(x, dtype=np.float64), np.asarray(Y, dtype=np.float64)

    def make_sampler(pos, metric, eps, sd):
        return BatchedHMCSeparable(x, Y, hyper_pars, pos, step_size=eps, num_steps_in_leap=num_steps_in_leap, seed=sd + 1000 * seed, ctx=ctx,
                                   M=metric, step_jitter=step_jitter)
    return _sample_recipe(lambda p: polish_map_separable(x, Y, hyper_pars, p, maxiter=polish, rounds=8, rank=rank, probes=rank + 32,
                                                         batch=batch, ctx=ctx, verbose=progress),
                          lambda q, k: separable_prior_metric(x, Y, hyper_pars, q, rank=rank, oversample=32, seed=3 + k, ctx=ctx,
                                                              batch=batch),
                          make_sampler, pars0, chains, iters, warm, warm_step, windows, window_iters, step_size, step_candidates,
                          target_accept, progress, segment)


def summarize_posterior_predictive(mean, var, y_samples, tilde_l_star, status, quantiles=(2.5, 50.0, 97.5)):
    """Posterior-predictive summary over H draws (pure NumPy).  mean, var, y_samples: [H, S, M] per-draw predictive moments and
    one sampled y* per draw; tilde_l_star: [H, S]; status: [H] (0 = the draw's covariance factored).  Draws with non-zero status
    are left out and counted.  Returns a dict: ``mean`` [S, M] (mean of the per-draw means), ``var`` [S, M] by the law of total
    variance (mean of the per-draw variances + variance of the per-draw means), ``quantiles`` [len(quantiles), S, M] of the
    sampled y*, ``tilde_l_star`` [H_used, S], ``status`` [H], ``n_used``, ``n_failed``.  The moments may also be [H, S] (one
    output per new input, the indexed form of the Hadamard model): every summary then loses its last axis."""
    mean, var, y_samples = np.asarray(mean, dtype=np.float64), np.asarray(var, dtype=np.float64), np.asarray(y_samples, dtype=np.float64)
    status = np.asarray(status)
    ok = status == 0
    if not ok.any():
        raise RuntimeError("no posterior draw could be used: every covariance failed to factor (status %s)" % status.tolist())
    m = mean[ok]
    return {"mean": m.mean(axis=0), "var": var[ok].mean(axis=0) + m.var(axis=0),
            "quantiles": np.percentile(y_samples[ok], list(quantiles), axis=0),
            "tilde_l_star": np.asarray(tilde_l_star, dtype=np.float64)[ok], "status": status, "n_used": int(ok.sum()),
            "n_failed": int((~ok).sum())}


def posterior_predict(x, Y, hyper_pars, samples, xs, draws=None, seed=0, ctx=None):
    """Posterior-predictive band of the nonseparable model from the sampler's draws (what ``Nonseparable_model_mpiKAISER.py:516-534``
    does with ``pointwise_predsample_inhomogeneous``): ``samples`` [iters, chains, P] or [H, P] as :func:`sample_nonseparable`
    returns them, ``xs`` [S] the new inputs; ``draws`` thins the history evenly to that many.  Per draw and new input the latent
    curves are regressed and sampled and y* is sampled (``seed``: NumPy generator of all the normals); all draws and inputs go
    through one batched device call (``Context.predsample_svc``).  Returns :func:`summarize_posterior_predictive`'s dict."""
    from . import _lib
    ctx = ctx if ctx is not None else _lib.default_context()
    x, Y = np.asarray(x, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    xs = np.asarray(xs, dtype=np.float64).reshape(-1)
    S_ = np.asarray(samples, dtype=np.float64)
    S_ = S_.reshape(-1, S_.shape[-1])
    if draws is not None and int(draws) < S_.shape[0]:
        S_ = S_[np.unique(np.round(np.linspace(0, S_.shape[0] - 1, int(draws))).astype(int))]
    hyper = np.array([float(hyper_pars[k]) for k in SVC_HYPER_KEYS])
    M = Y.shape[1]
    T = M * (M + 1) // 2
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((S_.shape[0], xs.shape[0], 1 + T))
    zy = rng.standard_normal((S_.shape[0], xs.shape[0], M))
    ctx.set_data(x, Y)
    mean, var, star, status = ctx.predsample_svc(S_, hyper, xs, z=z, constrained=True)
    return summarize_posterior_predictive(mean, var, mean + np.sqrt(var) * zy, star[:, :, 0], status)


def posterior_predict_separable(x, Y, hyper_pars, samples, xs, draws=None, seed=0, ctx=None):
    """Posterior-predictive band of the SEPARABLE model from the sampler's draws (what ``Separable_model.py:307-316`` does with
    ``pointwise_predsample``): ``samples`` [iters, chains, 2N+T+1] or [H, 2N+T+1] as :func:`sample_separable` returns them, ``xs``
    [S] the new inputs; ``draws`` thins the history evenly to that many.  Per draw and new input tilde_l* and tilde_sigma* are
    regressed and sampled and y* is sampled (``seed``: NumPy generator of all the normals); all draws and inputs go through one
    batched device call (``Context.predsample_sep``).  Returns :func:`summarize_posterior_predictive`'s dict plus
    ``tilde_sigma_star`` [H_used, S]."""
    from . import _lib
    ctx = ctx if ctx is not None else _lib.default_context()
    x, Y = np.asarray(x, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    xs = np.asarray(xs, dtype=np.float64).reshape(-1)
    S_ = np.asarray(samples, dtype=np.float64)
    S_ = S_.reshape(-1, S_.shape[-1])
    if draws is not None and int(draws) < S_.shape[0]:
        S_ = S_[np.unique(np.round(np.linspace(0, S_.shape[0] - 1, int(draws))).astype(int))]
    hyper = np.array([float(hyper_pars[k]) for k in SEP_HYPER_KEYS])
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((S_.shape[0], xs.shape[0], 2))
    zy = rng.standard_normal((S_.shape[0], xs.shape[0], Y.shape[1]))
    ctx.set_data(x, Y)
    mean, var, star, status = ctx.predsample_sep(S_, hyper, xs, z=z, kss_jitter=True)
    out = summarize_posterior_predictive(mean, var, mean + np.sqrt(var) * zy, star[:, :, 0], status)
    out["tilde_sigma_star"] = star[:, :, 1][status == 0]
    return out


def posterior_predict_stationary(x, Y, hyper_pars, samples, xs, draws=None, seed=0, ctx=None):
    """Posterior-predictive band of the STATIONARY (LMC) model from :class:`BatchedHMCStationary`'s draws: ``samples``
    [iters, chains, T+3] or [H, T+3], ``xs`` [S] the new inputs; ``draws`` thins the history evenly to that many.  The model has no
    latent curve to regress: a draw is a parameter vector, and only y* is sampled (``seed``: NumPy generator of its normals).  All
    draws and inputs go through one batched device call (``Context.predsample_sta``); ``hyper_pars`` is accepted for symmetry with
    the siblings and not used.  Returns :func:`summarize_posterior_predictive`'s dict -- the shape of
    :func:`posterior_predict_separable`'s without ``tilde_sigma_star`` --, ``tilde_l_star`` being each used draw's constant tilde_l
    [H_used, S]."""
    from . import _lib
    ctx = ctx if ctx is not None else _lib.default_context()
    x, Y = np.asarray(x, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    xs = np.asarray(xs, dtype=np.float64).reshape(-1)
    S_ = np.asarray(samples, dtype=np.float64)
    S_ = S_.reshape(-1, S_.shape[-1])
    if draws is not None and int(draws) < S_.shape[0]:
        S_ = S_[np.unique(np.round(np.linspace(0, S_.shape[0] - 1, int(draws))).astype(int))]
    rng = np.random.default_rng(seed)
    zy = rng.standard_normal((S_.shape[0], xs.shape[0], Y.shape[1]))
    ctx.set_data(x, Y)
    mean, var, status = ctx.predsample_sta(S_, xs)
    tl = np.repeat(S_[:, :1], xs.shape[0], axis=1)
    return summarize_posterior_predictive(mean, var, mean + np.sqrt(var) * zy, tl, status)


def posterior_predict_hadamard_sep(x, indx, y, hyper_pars, samples, xs, indx_star=None, draws=None, seed=0, ctx=None):
    """Posterior-predictive band of the separable HADAMARD model (irregularly observed outputs) from :class:`BatchedHMCHadamardSep`'s
    draws -- what the reference's scripts do, commented out, with ``pointwise_predsample_hadamard`` / ``test_predsample_hadamard``:
    ``samples`` [iters, chains, 2N+T+1] or [H, 2N+T+1], ``xs`` [S] the new inputs; ``draws`` thins the history evenly to that many.
    ``indx_star=None`` predicts all M outputs at every new input (moments [S, M]); ``indx_star`` [S] predicts output
    ``indx_star[s]`` only at ``xs[s]`` (held-out pairs; moments [S]).  Per draw and new input tilde_l* and tilde_sigma* are
    regressed and sampled and y* is sampled (``seed``: NumPy generator of all the normals); all draws and inputs go through one
    batched device call (``Context.predsample_hads``).  Returns :func:`summarize_posterior_predictive`'s dict plus
    ``tilde_sigma_star`` [H_used, S]."""
    from . import _lib
    ctx = ctx if ctx is not None else _lib.default_context()
    x, y = np.asarray(x, dtype=np.float64).reshape(-1), np.asarray(y, dtype=np.float64).reshape(-1)
    indx = np.ascontiguousarray(np.asarray(indx).reshape(-1), dtype=np.int32)
    xs = np.asarray(xs, dtype=np.float64).reshape(-1)
    S_ = np.asarray(samples, dtype=np.float64)
    S_ = S_.reshape(-1, S_.shape[-1])
    if draws is not None and int(draws) < S_.shape[0]:
        S_ = S_[np.unique(np.round(np.linspace(0, S_.shape[0] - 1, int(draws))).astype(int))]
    hyper = np.array([float(hyper_pars[k]) for k in SEP_HYPER_KEYS])
    ctx.had_set_data(x, indx, y)
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((S_.shape[0], xs.shape[0], 2))
    zy = rng.standard_normal((S_.shape[0], xs.shape[0]) + (() if indx_star is not None else (ctx.M,)))
    mean, var, star, status = ctx.predsample_hads(S_, hyper, xs, indx_star=indx_star, z=z)
    out = summarize_posterior_predictive(mean, var, mean + np.sqrt(var) * zy, star[:, :, 0], status)
    out["tilde_sigma_star"] = star[:, :, 1][status == 0]
    return out


def posterior_predict_hadamard(x, indx, y, hyper_pars, samples, xs, indx_star=None, draws=None, seed=0, ctx=None):
    """Posterior-predictive band of the nonseparable HADAMARD model (irregularly observed outputs) from :class:`BatchedHMCHadamard`'s
    draws: ``samples`` [iters, chains, N(1+T)+1] or [H, N(1+T)+1], ``xs`` [S] the new inputs; ``draws`` thins the history evenly to
    that many.  ``indx_star=None`` predicts all M outputs at every new input (moments [S, M]); ``indx_star`` [S] predicts output
    ``indx_star[s]`` only at ``xs[s]`` (held-out pairs; moments [S]).  Per draw and new input tilde_l* and the T slots of L* are
    regressed and sampled and y* is sampled (``seed``: NumPy generator of all the normals); all draws and inputs go through one
    batched device call (``Context.predsample_had``).  Returns :func:`summarize_posterior_predictive`'s dict plus ``L_star``
    [H_used, S, T] and ``corr_quantiles`` [3, S, M, M]: the 2.5 / 50 / 97.5 % quantiles over the used draws of cov2cor(L* L*^T), the
    time-varying cross-output correlation at the new inputs (what the reference's ``Post_Process`` scripts report)."""
    from . import _lib
    ctx = ctx if ctx is not None else _lib.default_context()
    x, y = np.asarray(x, dtype=np.float64).reshape(-1), np.asarray(y, dtype=np.float64).reshape(-1)
    indx = np.ascontiguousarray(np.asarray(indx).reshape(-1), dtype=np.int32)
    xs = np.asarray(xs, dtype=np.float64).reshape(-1)
    S_ = np.asarray(samples, dtype=np.float64)
    S_ = S_.reshape(-1, S_.shape[-1])
    if draws is not None and int(draws) < S_.shape[0]:
        S_ = S_[np.unique(np.round(np.linspace(0, S_.shape[0] - 1, int(draws))).astype(int))]
    hyper = np.array([float(hyper_pars[k]) for k in SVC_HYPER_KEYS])
    ctx.had_set_data(x, indx, y)
    M = ctx.M
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((S_.shape[0], xs.shape[0], 1 + M * (M + 1) // 2))
    zy = rng.standard_normal((S_.shape[0], xs.shape[0]) + (() if indx_star is not None else (M,)))
    mean, var, star, status = ctx.predsample_had(S_, hyper, xs, indx_star=indx_star, z=z)
    out = summarize_posterior_predictive(mean, var, mean + np.sqrt(var) * zy, star[:, :, 0], status)
    out["L_star"] = star[:, :, 1:][status == 0]
    out["corr_quantiles"] = correlation_quantiles(out["L_star"], M)
    return out


def _posterior_predict_cohort(subjects, samples, xs, indx_star, draws, seed, max_flop_waste, ctxs, width, predict, summarize):
    """What the three cohort posterior predictors share: the subjects as arrays, every history thinned to one number of draws, the
    normals of subject s from ``default_rng(seed + s)`` in the single-subject driver's order (``width(T)`` starred-value normals
    per draw and input first -- none for width 0 --, then the y* normals), the buckets of ``hadamard.cohort_buckets``, one subject set
    and ONE ``predict(ctx, draws, xs, indx_star, z)`` per bucket on ``ctxs`` (default: new contexts, closed on return), and
    ``summarize(M, result, zy, draws)`` per subject, returned in the caller's subject order."""
    from . import _lib, hadamard
    subjects = [(np.ascontiguousarray(x, dtype=np.float64).reshape(-1), np.asarray(indx).reshape(-1).astype(np.int32),
                 np.ascontiguousarray(y, dtype=np.float64).reshape(-1)) for x, indx, y in subjects]
    n = len(subjects)
    if n < 1 or len(samples) != n or len(xs) != n or (indx_star is not None and len(indx_star) != n):
        raise ValueError("subjects, samples, xs (and indx_star) must be lists of one positive length")
    Ms = sorted({int(np.unique(s[1]).shape[0]) for s in subjects})
    if len(Ms) != 1:
        raise ValueError("the subjects have different numbers of distinct labels: %s" % Ms)
    M = Ms[0]
    W = width(M * (M + 1) // 2)
    hist = []
    for S_ in samples:
        S_ = np.asarray(S_, dtype=np.float64)
        S_ = S_.reshape(-1, S_.shape[-1])
        if draws is not None and int(draws) < S_.shape[0]:
            S_ = S_[np.unique(np.round(np.linspace(0, S_.shape[0] - 1, int(draws))).astype(int))]
        hist.append(S_)
    H = hist[0].shape[0]
    if any(h.shape[0] != H for h in hist):
        raise ValueError("every subject must bring the same number of draws after thinning; got %s" % [h.shape[0] for h in hist])
    xs = [np.asarray(v, dtype=np.float64).reshape(-1) for v in xs]
    zs, zys = [], []
    for s in range(n):
        rng = np.random.default_rng(seed + s)
        zs.append(rng.standard_normal((H, xs[s].shape[0], W)) if W else None)
        zys.append(rng.standard_normal((H, xs[s].shape[0]) + (() if indx_star is not None else (M,))))
    nobs = [s[0].shape[0] for s in subjects]
    buckets = hadamard.cohort_buckets(nobs, max_flop_waste)
    if ctxs is not None and len(ctxs) != len(buckets):
        raise ValueError("%d contexts for %d buckets" % (len(ctxs), len(buckets)))
    out = [None] * n
    for b, idx in enumerate(buckets):
        ctx = ctxs[b] if ctxs is not None else _lib.Context()
        try:
            ctx.had_set_subjects([subjects[s][0] for s in idx], [subjects[s][1] for s in idx], [subjects[s][2] for s in idx], M=M)
            res = predict(ctx, [hist[s] for s in idx], [xs[s] for s in idx],
                          None if indx_star is None else [indx_star[s] for s in idx], [zs[s] for s in idx] if W else None)
        finally:
            if ctxs is None:
                ctx.close()
            elif ctx.h:
                ctx.had_clear_subjects()
        for s, r in zip(idx, res):
            out[int(s)] = summarize(M, r, zys[int(s)], hist[int(s)])
    return out


def posterior_predict_hadamard_cohort(subjects, hyper_pars, samples, xs, indx_star=None, draws=None, seed=0, max_flop_waste=0.5,
                                      ctxs=None):
    """:func:`posterior_predict_hadamard` for a cohort of subjects of RAGGED size: ``subjects`` a list of ``(x, indx, y)``,
    ``samples[s]`` [iters, chains, P_s] or [H, P_s] (thinned evenly to ``draws``; the same number of draws for every subject),
    ``xs[s]`` [S_s] the subject's own new inputs, ``indx_star[s]`` [S_s] labels or None.  One subject set per bucket of
    ``hadamard.cohort_buckets(nobs, max_flop_waste)`` and ONE ``nmgp_predsample_had_subjects`` per bucket (``ctxs``: one context per
    bucket, default new ones, closed on return).  The normals of subject s come from ``default_rng(seed + s)`` -- z first, then the
    y* normals, as the single-subject driver draws them from ``default_rng(seed)`` -- so a subject's band does not depend on who
    else is in the cohort.  Returns a list, in the caller's subject order, of that function's dicts (``L_star`` and
    ``corr_quantiles`` included)."""
    from . import hadamard
    hyper = np.array([float(hyper_pars[k]) for k in SVC_HYPER_KEYS])

    def summarize(M, r, zy, _):
        mean, var, star, status = r
        d = summarize_posterior_predictive(mean, var, mean + np.sqrt(var) * zy, star[:, :, 0], status)
        d["L_star"] = star[:, :, 1:][status == 0]
        d["corr_quantiles"] = correlation_quantiles(d["L_star"], M)
        return d

    return _posterior_predict_cohort(subjects, samples, xs, indx_star, draws, seed, max_flop_waste, ctxs, lambda T: 1 + T,
                                     lambda ctx, h, x_, ix, z: hadamard.cohort_predict(ctx, h, x_, hyper, indx_star=ix, z=z), summarize)


def posterior_predict_hadamard_sep_cohort(subjects, hyper_pars, samples, xs, indx_star=None, draws=None, seed=0, max_flop_waste=0.5,
                                          ctxs=None):
    """:func:`posterior_predict_hadamard_sep` for a cohort of subjects of RAGGED size, with the arguments, buckets, thinning and
    per-subject generators ``default_rng(seed + s)`` of :func:`posterior_predict_hadamard_cohort`: ``samples[s]``
    [iters, chains, 2 N_s + T + 1] or [H, 2 N_s + T + 1], ONE ``nmgp_predsample_hads_subjects`` per bucket.  Returns a list, in the
    caller's subject order, of that function's dicts (``tilde_sigma_star`` included)."""
    from . import hadamard_sep
    hyper = np.array([float(hyper_pars[k]) for k in SEP_HYPER_KEYS])

    def summarize(M, r, zy, _):
        mean, var, star, status = r
        d = summarize_posterior_predictive(mean, var, mean + np.sqrt(var) * zy, star[:, :, 0], status)
        d["tilde_sigma_star"] = star[:, :, 1][status == 0]
        return d

    return _posterior_predict_cohort(subjects, samples, xs, indx_star, draws, seed, max_flop_waste, ctxs, lambda T: 2,
                                     lambda ctx, h, x_, ix, z: hadamard_sep.cohort_predict(ctx, h, x_, hyper, indx_star=ix, z=z),
                                     summarize)


def posterior_predict_hadamard_sta_cohort(subjects, hyper_pars, samples, xs, indx_star=None, draws=None, seed=0, max_flop_waste=0.5,
                                          ctxs=None):
    """:func:`posterior_predict_hadamard_sta` for a cohort of subjects of RAGGED size, with the arguments, buckets, thinning and
    per-subject generators ``default_rng(seed + s)`` of :func:`posterior_predict_hadamard_cohort`: ``samples[s]`` [iters, chains, T + 3]
    or [H, T + 3], ONE ``nmgp_predict_hadst_subjects`` per bucket; only y* is sampled, and ``hyper_pars`` is accepted for symmetry and
    not used.  Returns a list, in the caller's subject order, of that function's dicts."""
    from . import hadamard_sta

    def summarize(M, r, zy, h):
        mean, var, status = r
        tl = np.repeat(h[:, :1], mean.shape[1], axis=1)
        return summarize_posterior_predictive(mean, var, mean + np.sqrt(var) * zy, tl, status)

    return _posterior_predict_cohort(subjects, samples, xs, indx_star, draws, seed, max_flop_waste, ctxs, lambda T: 0,
                                     lambda ctx, h, x_, ix, z: hadamard_sta.cohort_predict(ctx, h, x_, indx_star=ix), summarize)


def correlation_quantiles(L_star, M, quantiles=(2.5, 50.0, 97.5)):
    """[len(quantiles), S, M, M]: quantiles over the draws of cov2cor(L* L*^T), L* the lower triangle packed row by row in
    ``L_star`` [H, S, T] (the slots as they are).  Pure NumPy."""
    L_star = np.asarray(L_star, dtype=np.float64)
    H, S = L_star.shape[:2]
    L = np.zeros((H, S, M, M))
    r, c = np.tril_indices(M)
    L[:, :, r, c] = L_star
    B = L @ np.swapaxes(L, -1, -2)
    d = np.sqrt(np.einsum("hsmm->hsm", B))
    return np.percentile(B / (d[..., :, None] * d[..., None, :]), list(quantiles), axis=0)


def posterior_predict_hadamard_sta(x, indx, y, hyper_pars, samples, xs, indx_star=None, draws=None, seed=0, ctx=None):
    """Posterior-predictive band of the stationary HADAMARD model (irregularly observed outputs) from
    :class:`BatchedHMCHadamardSta`'s draws: ``samples`` [iters, chains, T+3] or [H, T+3], ``xs`` [S] the new inputs; ``draws`` thins
    the history evenly to that many.  ``indx_star=None`` predicts all M outputs at every new input (moments [S, M]); ``indx_star``
    [S] predicts output ``indx_star[s]`` only at ``xs[s]`` (held-out pairs; moments [S]).  The model has no latent curve to regress:
    a draw is a parameter vector, and only y* is sampled (``seed``: NumPy generator of its normals).  All draws and inputs go
    through one batched device call (``Context.predict_hadst``); ``hyper_pars`` is accepted for symmetry with the siblings and not
    used.  Returns :func:`summarize_posterior_predictive`'s dict, ``tilde_l_star`` being each used draw's constant tilde_l [H_used, S]."""
    from . import _lib
    ctx = ctx if ctx is not None else _lib.default_context()
    x, y = np.asarray(x, dtype=np.float64).reshape(-1), np.asarray(y, dtype=np.float64).reshape(-1)
    indx = np.ascontiguousarray(np.asarray(indx).reshape(-1), dtype=np.int32)
    xs = np.asarray(xs, dtype=np.float64).reshape(-1)
    S_ = np.asarray(samples, dtype=np.float64)
    S_ = S_.reshape(-1, S_.shape[-1])
    if draws is not None and int(draws) < S_.shape[0]:
        S_ = S_[np.unique(np.round(np.linspace(0, S_.shape[0] - 1, int(draws))).astype(int))]
    ctx.had_set_data(x, indx, y)
    rng = np.random.default_rng(seed)
    zy = rng.standard_normal((S_.shape[0], xs.shape[0]) + (() if indx_star is not None else (ctx.M,)))
    mean, var, status = ctx.predict_hadst(S_, xs, indx_star=indx_star)
    tl = np.repeat(S_[:, :1], xs.shape[0], axis=1)
    return summarize_posterior_predictive(mean, var, mean + np.sqrt(var) * zy, tl, status)
