"""Generate the separable / stationary posterior-draw prediction fixtures (tests/golden/predsample_sep_*.npz) by RUNNING THE
REFERENCE on the CPU.

The set-up is make_golden_predsample.py's (imported: the reference on sys.path, the ``symeig`` / ``solve`` aliases, the patched
``Normal.sample`` that consumes a recorded NumPy stream and records every call's ``loc`` / ``scale``).  The separable functions
consume the stream per grid point and per draw as 1, 1, M numbers (tilde_l*, tilde_sigma*, y).  The stationary functions draw
ONE ``np.random.randn()`` per (draw, grid point); that function is patched the same way for the duration of the call only.  They
return samples, not moments, so they are run three times: with the recorded z (the samples), with z = 0 (the means) and with
z = 1 (mean + standard deviation); a fourth, unpatched run under ``np.random.seed`` records the reference's own stream.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_predsample_sep.py [--only PREFIX]
"""
import argparse
import contextlib
import io
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402
from make_golden_predsample import PRECISION, SMALL, SMALL_XS, condvar, recorded  # noqa: E402

sim, prediction, logpos, t = G.sim, G.prediction, G.logpos, G.t
HYPER_NAMES = ("mu_tilde_l", "alpha_tilde_l", "beta_tilde_l", "mu_tilde_sigma", "alpha_tilde_sigma", "beta_tilde_sigma")


def split_calls(calls, S, H, M):
    """calls in consumption order (grid point, draw, [tilde_l*, tilde_sigma*, y]) -> loc / scale arrays [S, H, 2 + M]."""
    assert len(calls) == 3 * S * H and [c[0].size for c in calls[:3]] == [1, 1, M]
    loc = np.concatenate([c[0] for c in calls]).reshape(S, H, 2 + M)
    scale = np.concatenate([c[1] for c in calls]).reshape(S, H, 2 + M)
    return loc, scale


def sep_draws(p0, x, N, T, H):
    out = []
    for k in range(H):
        p = p0.copy()
        p[:N] += 0.05 * np.sin(3.0 * x + 0.4 + k)
        p[N:2 * N] += 0.05 * np.sin(3.0 * x + 1.4 + k)
        p[2 * N:2 * N + T] += 0.02 * np.cos(np.arange(T) + k)
        p[-1] += 0.01 * k
        out.append(p)
    return np.stack(out)


def sta_draws(p0, T, H):
    out = []
    for k in range(H):
        p = p0.copy()
        p[0] += 0.05 * np.sin(0.4 + k)
        p[1] += 0.05 * np.sin(1.4 + k)
        p[2:2 + T] += 0.02 * np.cos(np.arange(T) + k)
        p[-1] += 0.01 * k
        out.append(p)
    return np.stack(out)


def assert_no_clip(loc, scale, x, xs, h):
    """A condition, not a measurement: every recorded latent scale^2 is the independently recomputed conditional variance (not
    settings.precision put in its place) and exceeds it; every predictive variance is far from the clip value."""
    cl = condvar(x, xs, h["alpha_tilde_l"], h["beta_tilde_l"])
    cs = condvar(x, xs, h["alpha_tilde_sigma"], h["beta_tilde_sigma"])
    for k, cv in ((0, cl), (1, cs)):
        s2 = scale[:, :, k] ** 2
        assert np.allclose(s2, cv[:, None], rtol=1e-3, atol=0), (s2, cv)
        assert s2.min() > 1.0000001 * PRECISION, s2.min()
    vy = scale[:, :, 2:] ** 2
    assert vy.min() > 10 * PRECISION, vy.min()
    return float(min(cl.min(), cs.min())), float(max(cl.max(), cs.max())), float(vy.min())


def hist(draws, N, T):
    return t(draws[:, :N]), t(draws[:, N:2 * N]), t(draws[:, 2 * N:2 * N + T]), t(draws[:, -1])


def gen_family_predsample(x, Y, draws, xs, h, seed):
    N, M = Y.shape
    T = M * (M + 1) // 2
    S, H = len(xs), len(draws)
    z = np.random.default_rng(seed).standard_normal((S, H, 2 + M))
    t0 = time.time()
    with recorded(z) as st:
        ys = prediction.pointwise_predsample(*hist(draws, N, T), t(Y), t(x), t(xs), *[h[k] for k in HYPER_NAMES], N_sample=H)
    assert isinstance(ys, np.ndarray) and ys.shape == (S, H, M)
    loc, scale = split_calls(st.calls, S, H, M)
    lo, hi, vmin = assert_no_clip(loc, scale, x, xs, h)
    print("  predsample %d draws x %d points: %.1f s; conditional variances %.3g..%.3g, smallest predictive variance %.4g"
          % (H, S, time.time() - t0, lo, hi, vmin), flush=True)
    return dict(ps_z=z, ps_y=ys, ps_loc=loc, ps_scale=scale)


def gen_family_sampling(x, Y, p, xs, h, n_sample, seed):
    N, M = Y.shape
    T = M * (M + 1) // 2
    S = len(xs)
    z = np.random.default_rng(seed).standard_normal((S, n_sample, 2 + M))
    one = (t(p[:N]), t(p[N:2 * N]), t(p[2 * N:2 * N + T]), t(p[-1:])[0])
    with recorded(z) as st:
        q, mean, std = prediction.pointwise_predmap_sampling(n_sample, *one, t(Y), t(x), t(xs), *[h[k] for k in HYPER_NAMES])
    loc, scale = split_calls(st.calls, S, n_sample, M)
    assert_no_clip(loc, scale, x, xs, h)
    assert q.shape == (S, 2, M) and mean.shape == (S, M) and std.shape == (S, M)
    return dict(sm_pars=p, sm_n_sample=n_sample, sm_z=z, sm_q=q, sm_mean=mean, sm_std=std, sm_loc=loc, sm_scale=scale)


@contextlib.contextmanager
def randn_stream(z):
    """np.random.randn() -> the next number of z, for the duration of the block only."""
    z = np.asarray(z, dtype=np.float64).reshape(-1)
    pos = [0]
    orig = np.random.randn

    def randn(*shape):
        assert not shape, "the stationary functions draw scalars"
        pos[0] += 1
        return float(z[pos[0] - 1])

    np.random.randn = randn
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            yield
    finally:
        np.random.randn = orig
    assert pos[0] == z.size, "the reference consumed %d of %d numbers" % (pos[0], z.size)


def gen_family_stationary(x, Y, draws, xs, seed):
    N, M = Y.shape
    T = M * (M + 1) // 2
    H, S = len(draws), len(xs)
    args = (t(draws[:, 0]), t(draws[:, 1]), t(draws[:, 2:2 + T]), t(draws[:, -1]), t(Y), t(x), t(xs))
    z = np.random.default_rng(seed).standard_normal((H, S))
    with randn_stream(z):
        ys = prediction.pointwise_predsample_S(*args)
    with randn_stream(np.zeros((H, S))):
        mean = prediction.pointwise_predsample_S(*args)
    with randn_stream(np.ones((H, S))):
        sd = prediction.pointwise_predsample_S(*args) - mean
    assert isinstance(ys, np.ndarray) and ys.shape == (H, S, M)
    assert np.all(np.isfinite(ys)) and (sd ** 2).min() > 10 * PRECISION, (sd ** 2).min()
    np.random.seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        seeded = prediction.test_predsample_S(*args)
    print("  stationary %d draws x %d points: smallest predictive variance %.4g" % (H, S, (sd ** 2).min()), flush=True)
    return dict(sta_draws=draws, sta_z=z, sta_y=ys, sta_mean=mean, sta_sd=sd, sta_seed=seed, sta_y_seeded=seeded)


def finish(name, out):
    G.save(name, **out)
    assert os.path.getsize(os.path.join(HERE, name + ".npz")) < 1 << 20


def gen_n64(only):
    name = "predsample_sep_N64_M3"
    if only and not name.startswith(only):
        return
    N, M = 64, 3
    T = M * (M + 1) // 2
    x, Y = sim.rngfree_inputs(N, M)
    xs = np.array([0.02, 0.2, 0.37, 0.5, 0.613, 0.88, 0.99])           # the grid of pred_N64_M3
    h = sim.HYPER_SEP
    draws = sep_draws(sim.rngfree_pars_sep(N, M), x, N, T, 6)
    out = dict(x=x, Y=Y, xs=xs, hyper=G.hyper_vec(h, G.SEP_KEYS), draws=draws)
    out.update(gen_family_predsample(x, Y, draws, xs, h, seed=301))
    out.update(gen_family_sampling(x, Y, draws[0], xs, h, n_sample=5, seed=302))
    out.update(gen_family_stationary(x, Y, sta_draws(sim.rngfree_pars_sta(M), T, 5), xs, seed=303))
    finish(name, out)


def gen_n512(only):
    name = "predsample_sep_N512_M5"
    if only and not name.startswith(only):
        return
    N, M = 512, 5
    T = M * (M + 1) // 2
    d = sim.simulate_separable(N, M, seed=7)
    x, Y = d["x"], d["Y"]
    xs = np.linspace(0.0, 1.0, 201)[[3, 47, 100, 151, 198]]
    h = sim.HYPER_SEP
    draws = sep_draws(d["pars_true"], x, N, T, 8)
    out = dict(x=x, Y=Y, xs=xs, hyper=G.hyper_vec(h, G.SEP_KEYS), draws=draws)
    out.update(gen_family_predsample(x, Y, draws, xs, h, seed=401))
    finish(name, out)


def gen_small(only):
    """predsample_sep_N8_M1, predsample_sep_N12_M2, predsample_sep_N10_M8: the three families at H = n_sample = 3, S = 4."""
    for N, M in SMALL:
        name = "predsample_sep_N%d_M%d" % (N, M)
        if only and not name.startswith(only):
            continue
        T = M * (M + 1) // 2
        x, Y = sim.rngfree_inputs(N, M)
        h = sim.HYPER_SEP
        draws = sep_draws(sim.rngfree_pars_sep(N, M), x, N, T, 3)
        out = dict(x=x, Y=Y, xs=SMALL_XS, hyper=G.hyper_vec(h, G.SEP_KEYS), draws=draws)
        out.update(gen_family_predsample(x, Y, draws, SMALL_XS, h, seed=700 + M))
        out.update(gen_family_sampling(x, Y, draws[0], SMALL_XS, h, n_sample=3, seed=800 + M))
        out.update(gen_family_stationary(x, Y, sta_draws(sim.rngfree_pars_sta(M), T, 3), SMALL_XS, seed=900 + M))
        G.save(name, **out)
        assert os.path.getsize(os.path.join(HERE, name + ".npz")) < 50000


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    gen_n64(a.only)
    gen_n512(a.only)
    gen_small(a.only)
