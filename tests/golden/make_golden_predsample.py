"""Generate the posterior-draw prediction fixtures (tests/golden/predsample_*.npz) by RUNNING THE REFERENCE on the CPU.

Like make_golden.py (whose set-up -- the reference on sys.path, the ``symeig`` / ``solve`` aliases -- is imported from it), this
only works where a checkout of the reference exists.  ``torch.distributions.Normal.sample`` is patched in this process to
``loc + scale * z`` with z taken from a recorded NumPy stream, and every call's ``loc`` / ``scale`` is recorded: the fixtures hold
inputs, hyper-parameters, the draws, xs, the z stream, the reference's returned samples and the recorded moments split into
(tilde_l*, L*, y).  The stream is consumed per grid point and per draw as 1, T, M numbers.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_predsample.py [--only PREFIX]
"""
import argparse
import contextlib
import io
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (puts the reference on the path, installs the aliases)

from torch.distributions.normal import Normal  # noqa: E402

sim, prediction, logpos, t = G.sim, G.prediction, G.logpos, G.t
PRECISION = 1e-6


class Stream:
    """The patched Normal.sample: consumes z in order, records (loc, scale) of every call."""

    def __init__(self, z):
        self.z = np.asarray(z, dtype=np.float64).reshape(-1)
        self.pos = 0
        self.calls = []

    def sample(self, dist, sample_shape=torch.Size()):
        loc, scale = dist.loc.detach().double(), dist.scale.detach().double()
        k = loc.numel()
        z = torch.from_numpy(self.z[self.pos:self.pos + k].copy()).view(loc.shape)
        assert z.numel() == k, "the recorded stream ran out"
        self.pos += k
        self.calls.append((loc.numpy().reshape(-1).copy(), scale.numpy().reshape(-1).copy()))
        return loc + scale * z


@contextlib.contextmanager
def recorded(z):
    st = Stream(z)
    orig = Normal.sample
    Normal.sample = lambda self, sample_shape=torch.Size(): st.sample(self, sample_shape)
    try:
        with contextlib.redirect_stdout(io.StringIO()):          # the reference prints every grid point
            yield st
    finally:
        Normal.sample = orig
    assert st.pos == st.z.size, "the reference consumed %d of %d numbers" % (st.pos, st.z.size)


def split_calls(calls, S, H, T, M):
    """calls in consumption order (grid point, draw, [tilde_l*, L*, y]) -> loc / scale arrays [S, H, 1 + T + M]."""
    assert len(calls) == 3 * S * H and [c[0].size for c in calls[:3]] == [1, T, M]
    loc = np.concatenate([c[0] for c in calls]).reshape(S, H, 1 + T + M)
    scale = np.concatenate([c[1] for c in calls]).reshape(S, H, 1 + T + M)
    return loc, scale


def smooth_draws(p0, x, N, T, H):
    """The true parameters + 0.05 sin(3x + 0.4 + k [+ t]): smooth in x as in make_golden.gen_pred_grid; p[-1] += 0.01 k."""
    out = []
    for k in range(H):
        p = p0.copy()
        p[:N] += 0.05 * np.sin(3.0 * x + 0.4 + k)
        p[N:N + N * T] += (0.05 * np.sin(3.0 * x[:, None] + 0.4 + k + np.arange(T)[None, :])).reshape(-1)
        p[-1] += 0.01 * k
        out.append(p)
    return np.stack(out)


def condvar(x, xs, alpha, beta):
    """(alpha^2 + 1e-6) - k^T Sigma^-1 k, recomputed independently: the generator asserts that no clip branch was taken."""
    d = (x[:, None] - x[None, :]) / beta
    Sig = alpha ** 2 * np.exp(-0.5 * d ** 2) + 1e-6 * np.eye(len(x))
    k = alpha ** 2 * np.exp(-0.5 * ((x[:, None] - xs[None, :]) / beta) ** 2)
    return (alpha ** 2 + 1e-6) - np.sum(k * np.linalg.solve(Sig, k), axis=0)


def assert_no_clip(loc, scale, x, xs, h, T):
    cl = condvar(x, xs, h["alpha_tilde_l"], h["beta_tilde_l"])
    cL = condvar(x, xs, h["alpha_L"], h["beta_L"])
    assert cl.min() > 0 and cL.min() > 0, (cl.min(), cL.min())
    # the recorded scales are the square roots of those (not of settings.precision put in their place) ...
    assert np.allclose(scale[:, :, 0] ** 2, cl[:, None], rtol=1e-3, atol=0), (scale[:, :, 0] ** 2, cl)
    assert np.allclose(scale[:, :, 1:1 + T] ** 2, cL[:, None, None], rtol=1e-3, atol=0)
    # ... and the predictive variances are far from the clip value
    vy = scale[:, :, 1 + T:] ** 2
    assert vy.min() > 10 * PRECISION, vy.min()
    return float(min(cl.min(), cL.min())), float(max(cl.max(), cL.max())), float(vy.min())


def hist(draws, N, T):
    return t(draws[:, :N]), t(draws[:, N:N + N * T]), t(draws[:, -1])


def gen_family_predsample(x, Y, draws, xs, h, seed):
    N, M = Y.shape
    T = M * (M + 1) // 2
    S, H = len(xs), len(draws)
    z = np.random.default_rng(seed).standard_normal((S, H, 1 + T + M))
    tl, uL, ts = hist(draws, N, T)
    t0 = time.time()
    with recorded(z) as st:
        ys = prediction.pointwise_predsample_inhomogeneous(tl, uL, ts, t(Y), t(x), t(xs), h["mu_tilde_l"], h["alpha_tilde_l"],
                                                           h["beta_tilde_l"], h["mu_L"], h["alpha_L"], h["beta_L"], N_sample=H)
    assert isinstance(ys, np.ndarray) and ys.shape == (S, H, M)
    loc, scale = split_calls(st.calls, S, H, T, M)
    lo, hi, vmin = assert_no_clip(loc, scale, x, xs, h, T)
    print("  predsample %d draws x %d points: %.1f s; conditional variances %.3g..%.3g, smallest predictive variance %.4g"
          % (H, S, time.time() - t0, lo, hi, vmin), flush=True)
    return dict(ps_z=z, ps_y=ys, ps_loc=loc, ps_scale=scale)


def gen_family_sampling(x, Y, p, xs, h, n_sample, seed):
    N, M = Y.shape
    T = M * (M + 1) // 2
    S = len(xs)
    rng = np.random.default_rng(seed)
    tl, uL, ts = logpos.vec2pars_SVC(t(p), N, M)
    hv = (h["mu_tilde_l"], h["alpha_tilde_l"], h["beta_tilde_l"], h["mu_L"], h["alpha_L"], h["beta_L"])
    out = dict(sm_pars=p, sm_n_sample=n_sample)
    z = rng.standard_normal((S, n_sample, 1 + T + M))
    with recorded(z) as st:
        q, mean, std = prediction.pointwise_predmap_inhomogeneous_sampling(n_sample, tl, uL, ts, t(Y), t(x), t(xs), *hv)
    loc, scale = split_calls(st.calls, S, n_sample, T, M)
    assert_no_clip(loc, scale, x, xs, h, T)
    assert q.shape == (S, 2, M) and mean.shape == (S, M) and std.shape == (S, M)
    out.update(sm_z=z, sm_q=q, sm_mean=mean, sm_std=std, sm_loc=loc, sm_scale=scale)
    z = rng.standard_normal((S, n_sample, 1))
    with recorded(z):
        tls = prediction.pointwise_predmap_inhomogeneous_sampling(n_sample, tl, uL, ts, t(Y), t(x), t(xs), *hv, pred_smoothness=True)
    assert tls.shape == (S, n_sample)
    out.update(sm_z_smooth=z, sm_tl=tls)
    z = rng.standard_normal((S, n_sample, T))
    with recorded(z):
        Lf = prediction.pointwise_predmap_inhomogeneous_sampling(n_sample, tl, uL, ts, t(Y), t(x), t(xs), *hv, pred_cov=True)
    assert Lf.shape == (S, n_sample, M, M)
    out.update(sm_z_cov=z, sm_Lf=Lf)
    return out


def gen_n64(only):
    name = "predsample_N64_M3"
    if only and not name.startswith(only):
        return
    N, M = 64, 3
    T = M * (M + 1) // 2
    x, Y = sim.rngfree_inputs(N, M)
    xs = np.array([0.02, 0.2, 0.37, 0.5, 0.613, 0.88, 0.99])           # the grid of pred_N64_M3
    h = sim.HYPER_SVC
    draws = smooth_draws(sim.rngfree_pars_svc(N, M), x, N, T, 6)
    out = dict(x=x, Y=Y, xs=xs, hyper=G.hyper_vec(h, G.SVC_KEYS), draws=draws)
    out.update(gen_family_predsample(x, Y, draws, xs, h, seed=101))
    out.update(gen_family_sampling(x, Y, draws[0], xs, h, n_sample=5, seed=102))
    G.save(name, **out)


def gen_n512(only):
    name = "predsample_N512_M3"
    if only and not name.startswith(only):
        return
    N, M = 512, 3
    T = M * (M + 1) // 2
    d = sim.simulate_nonseparable(N, M, seed=7)
    x, Y = d["x"], d["Y"]
    xs = np.linspace(0.0, 1.0, 201)[[3, 47, 100, 151, 198]]
    h = sim.HYPER_SVC
    draws = smooth_draws(d["pars_true"], x, N, T, 8)
    out = dict(x=x, Y=Y, xs=xs, hyper=G.hyper_vec(h, G.SVC_KEYS), draws=draws)
    out.update(gen_family_predsample(x, Y, draws, xs, h, seed=201))
    G.save(name, **out)
    assert os.path.getsize(os.path.join(HERE, name + ".npz")) < 1 << 20


SMALL = ((8, 1), (12, 2), (10, 8))             # (N, M) away from M = 3: one output, an even M, the largest instantiation
SMALL_XS = np.array([0.02, 0.37, 0.613, 0.99])


def gen_small(only):
    """predsample_N8_M1, predsample_N12_M2, predsample_N10_M8: both families at H = n_sample = 3, S = 4 (a few kB each)."""
    for N, M in SMALL:
        name = "predsample_N%d_M%d" % (N, M)
        if only and not name.startswith(only):
            continue
        T = M * (M + 1) // 2
        x, Y = sim.rngfree_inputs(N, M)
        h = sim.HYPER_SVC
        draws = smooth_draws(sim.rngfree_pars_svc(N, M), x, N, T, 3)
        out = dict(x=x, Y=Y, xs=SMALL_XS, hyper=G.hyper_vec(h, G.SVC_KEYS), draws=draws)
        out.update(gen_family_predsample(x, Y, draws, SMALL_XS, h, seed=500 + M))
        out.update(gen_family_sampling(x, Y, draws[0], SMALL_XS, h, n_sample=3, seed=600 + M))
        G.save(name, **out)
        assert os.path.getsize(os.path.join(HERE, name + ".npz")) < 50000


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    gen_n64(a.only)
    gen_n512(a.only)
    gen_small(a.only)
