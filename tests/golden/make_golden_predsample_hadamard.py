"""Generate the posterior-draw prediction fixtures of the separable Hadamard model (tests/golden/hps_*.npz) by RUNNING THE
REFERENCE on the CPU (prediction.pointwise_predsample_hadamard, test_predsample_hadamard, test_predmap_harmard).

The set-up is make_golden_predsample.py's (imported: the reference on sys.path, the ``symeig`` / ``solve`` aliases, the patched
``Normal.sample`` that consumes a recorded NumPy stream and records every call's ``loc`` / ``scale``); the subjects are
make_golden_hadamard's ``inputs()`` and the draws make_golden_hadamard_sep's ``pars_smooth(x, M, shift=0.1 k)`` under its HYPER.
The grid family consumes the stream per grid point and per draw as 1, 1, M numbers (tilde_l*, tilde_sigma*, y), the indexed family
as 1, 1, 1.  The fixtures hold inputs, hyper-parameters, the draws, the new inputs, the z streams, the reference's returned samples,
the recorded moments split into [S, H, 2 + M] / [S, H, 3], and the MAP indexed quantiles of ``draws[0]``.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_predsample_hadamard.py [--only PREFIX]
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
import make_golden as G  # noqa: E402
from make_golden_predsample import PRECISION, condvar, recorded  # noqa: E402
from make_golden_hadamard import inputs  # noqa: E402
from make_golden_hadamard_sep import HYPER, pars_smooth  # noqa: E402

prediction, t = G.prediction, G.t
HYPER_NAMES = ("mu_tilde_l", "alpha_tilde_l", "beta_tilde_l", "mu_tilde_sigma", "alpha_tilde_sigma", "beta_tilde_sigma")


def split_calls(calls, S, H, K):
    """calls in consumption order (point, draw, [tilde_l*, tilde_sigma*, y]) -> loc / scale arrays [S, H, 2 + K]."""
    assert len(calls) == 3 * S * H and [c[0].size for c in calls[:3]] == [1, 1, K]
    loc = np.concatenate([c[0] for c in calls]).reshape(S, H, 2 + K)
    scale = np.concatenate([c[1] for c in calls]).reshape(S, H, 2 + K)
    return loc, scale


def assert_no_clip(loc, scale, x, xs):
    """A condition, not a measurement: every recorded latent scale^2 is the independently recomputed conditional variance (not
    settings.precision put in its place) and exceeds it; every predictive variance is far from the clip value."""
    cl = condvar(x, xs, HYPER["alpha_tilde_l"], HYPER["beta_tilde_l"])
    cs = condvar(x, xs, HYPER["alpha_tilde_sigma"], HYPER["beta_tilde_sigma"])
    for k, cv in ((0, cl), (1, cs)):
        s2 = scale[:, :, k] ** 2
        assert np.allclose(s2, cv[:, None], rtol=1e-3, atol=0), (s2, cv)
        assert s2.min() > 1.0000001 * PRECISION, s2.min()
    vy = scale[:, :, 2:] ** 2
    assert vy.min() > 10 * PRECISION, vy.min()
    return float(min(cl.min(), cs.min())), float(max(cl.max(), cs.max())), float(vy.min())


def case(name, N, M, seed, H, x_test, indx_test, zseed):
    T = M * (M + 1) // 2
    x, indx, y = inputs(N, M, seed)
    draws = np.stack([pars_smooth(x, M, shift=0.1 * k) for k in range(H)])
    grids = np.array([-0.05, 0.1, float(x[N // 3]), 0.37, 0.5, 0.62, 0.8, 0.93, 1.02])    # the grid of the hsep_* fixtures
    x_test, indx_test = np.asarray(x_test, dtype=np.float64), np.asarray(indx_test, dtype=np.int64)
    assert sorted(set(indx_test.tolist())) == list(range(M)), "the test labels must cover every output"
    hist = (t(draws[:, :N]), t(draws[:, N:2 * N]), t(draws[:, 2 * N:2 * N + T]), t(draws[:, -1]))
    data = (t(x), torch.from_numpy(indx), t(y))
    h = [HYPER[k] for k in HYPER_NAMES]
    S, St = len(grids), len(x_test)
    rng = np.random.default_rng(zseed)
    z = rng.standard_normal((S, H, 2 + M))
    zi = rng.standard_normal((St, H, 3))
    t0 = time.time()
    with recorded(z) as st:
        ys = prediction.pointwise_predsample_hadamard(*hist, *data, t(grids), *h)
    assert tuple(ys.shape) == (S, H, M)
    loc, scale = split_calls(st.calls, S, H, M)
    lo, hi, vmin = assert_no_clip(loc, scale, x, grids)
    with recorded(zi) as st:
        yi = prediction.test_predsample_hadamard(*hist, *data, t(x_test), torch.from_numpy(indx_test), *h)
    assert tuple(yi.shape) == (St, H)
    iloc, iscale = split_calls(st.calls, St, H, 1)
    lo2, hi2, vmin2 = assert_no_clip(iloc, iscale, x, x_test)
    p = t(draws[0])
    with contextlib.redirect_stdout(io.StringIO()):
        pct = prediction.test_predmap_harmard(p[:N], p[N:2 * N], p[2 * N:2 * N + T], p[-1], *data, t(x_test),
                                              torch.from_numpy(indx_test), *h)
    assert tuple(pct.shape) == (St, 3)
    print("%-14s %d draws, %d + %d points: %.1f s; conditional variances %.3g..%.3g, smallest predictive variance %.4g"
          % (name, H, S, St, time.time() - t0, min(lo, lo2), max(hi, hi2), min(vmin, vmin2)), flush=True)
    G.save(name, x=x, indx=indx.astype(np.int32), y=y, M=M, hyper=G.hyper_vec(HYPER, G.SEP_KEYS), draws=draws, grids=grids,
           ps_z=z, ps_y=ys.numpy(), ps_loc=loc, ps_scale=scale, x_test=x_test, indx_test=indx_test.astype(np.int32), ix_z=zi,
           ix_y=yi.numpy(), ix_loc=iloc, ix_scale=iscale, map_pct=pct.numpy())
    assert os.path.getsize(os.path.join(HERE, name + ".npz")) < 1 << 20


CASES = [
    # two tiles, ragged; label 2 is the rare one (2 observations of 77)
    ("hps_N77_M3", dict(N=77, M=3, seed=77, H=6, x_test=[0.07, 0.3, None, 0.55, 0.81, 1.01], indx_test=[0, 1, 2, 2, 1, 0], zseed=771)),
    # four tiles
    ("hps_N200_M4", dict(N=200, M=4, seed=200, H=4, x_test=[-0.02, 0.21, None, 0.48, 0.77, 0.97], indx_test=[0, 1, 2, 3, 1, 2],
                         zseed=2001)),
]

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    for name, kw in CASES:
        if name.startswith(a.only):
            x = inputs(kw["N"], kw["M"], kw["seed"])[0]
            kw["x_test"] = [float(x[kw["N"] // 2]) if v is None else v for v in kw["x_test"]]      # one observed x among them
            case(name, **kw)
