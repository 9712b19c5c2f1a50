"""Generate the stationary-Hadamard fixtures tests/golden/hsta_*.npz by RUNNING THE REFERENCE (logpos.nlogpos_obj_hadamard_S,
prediction.pointwise_predmap_S_hadamard, prediction.test_predmap_S_hadamard).  Set-up (paths, the torch aliases the reference
needs, helpers) is make_golden's, the subjects are make_golden_hadamard's ``inputs()``: the same (x, indx, y) as the had_* / hsep_*
fixtures.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_hadamard_sta.py [--only PREFIX]

The parameter vector is [tilde_l, tilde_sigma, L_vec (T raw slots), tilde_sigma2_err], P = T + 3; the lower triangle is
make_golden_hadamard_sep.pars_smooth's.  sigma_tilde_l = 0.7 is not a float32 number: torch rounds the Python-number arguments of
Normal(mu, sigma) to float32, and the fixtures record that.  The fixtures are plain data: inputs, hyper-parameters, the reference's
outputs (the five-entry verbose tuple, autograd gradients, the covariance, the percentiles, the indexed predictor's mean and std).

The generator asserts that the reference stays clear of every clip: K positive definite, cond(S) < 1e6, every predictive variance
above 1e-4.

hsta_map_N77_M3 is 30 steps of torch.optim.Adam at lr 0.05 from the fixture point of hsta_N77_M3 under the same HYPER; 20 of them
are compared.
"""
import argparse

import numpy as np
import torch

import make_golden as mg
from make_golden import kernels, logpos, prediction, utils, t
from make_golden_hadamard import inputs
import make_golden_hadamard_sep as hsep

HYPER = dict(mu_tilde_l=-2.0, sigma_tilde_l=0.7, a=2.0, b=0.5, c=3.0)
KEYS = mg.STA_KEYS


def pars_sta(M, shift=0.0):
    T = M * (M + 1) // 2
    Lv = hsep.pars_smooth(np.zeros(1), M, shift)[2:2 + T]
    return np.concatenate([[-2.3 + 0.2 * shift, 0.1 - 0.3 * shift], Lv, [np.log(1e-2) + 0.3 * shift]])


def run(pars, x, indx, y, prior=True):
    p = t(pars).clone().requires_grad_(True)
    out = logpos.nlogpos_obj_hadamard_S(p, t(x), torch.from_numpy(indx), t(y), **HYPER, verbose=True, Prior=prior)
    assert len(out) == 5
    vals = np.array([float(o.detach()) for o in out])
    out[0].backward()
    return vals, p.grad.detach().numpy().copy()


def covariance(pars, x, indx):
    """(K, S = K + sigma2_err I) with the reference's own functions (logpos.py:679-690)."""
    M = int(np.unique(indx).shape[0])
    T = M * (M + 1) // 2
    p = t(pars)
    L = utils.vec2lowtriangle(p[2:2 + T], M)
    B_f = torch.mm(L, L.t())
    K_x = kernels.RBF_cov(t(x).view([-1, 1]), alpha=torch.exp(p[1]), beta=torch.exp(p[0]))
    K = (K_x * logpos.generate_K_index(B_f, torch.from_numpy(indx))).numpy()
    return K, K + float(torch.exp(p[-1])) * np.eye(x.shape[0])


def check(pars, x, indx):
    K, S = covariance(pars, x, indx)
    emin = float(np.linalg.eigvalsh(K)[0])
    cond = float(np.linalg.cond(S))
    assert emin > 0.0, "K is not positive definite (min eig %g)" % emin
    assert cond < 1e6, "cond(S) = %g" % cond
    return S, emin, cond


def grid_of(x):
    N = x.shape[0]
    return np.array([-0.05, 0.1, float(x[N // 3]), 0.37, 0.5, 0.62, 0.8, 0.93, 1.02])    # hsep.predict's grid


def predict(pars, x, indx, y):
    M = int(np.unique(indx).shape[0])
    T = M * (M + 1) // 2
    grids = grid_of(x)
    p = t(pars)
    pct = prediction.pointwise_predmap_S_hadamard(p[0], p[1], p[2:2 + T], p[-1], t(x), torch.from_numpy(indx), t(y), t(grids)).numpy()
    var = ((pct[:, 2] - pct[:, 0]) / (2 * 1.96)) ** 2
    assert var.min() > 1e-4, "a predictive variance took the clip branch (min %g)" % var.min()
    return grids, pct, float(var.min())


def predict_indexed(pars, x, indx, y):
    """The reference's indexed predictor on the 9 grid points with labels arange(9) % M.  Its variance takes B_f[0, 0] for every
    label ((A - B)[0, 0]); recorded as it is."""
    M = int(np.unique(indx).shape[0])
    T = M * (M + 1) // 2
    grids = grid_of(x)
    lab = np.arange(grids.shape[0]) % M
    p = t(pars)
    mean, sd = prediction.test_predmap_S_hadamard(p[0], p[1], p[2:2 + T], p[-1], t(x), torch.from_numpy(indx), t(y), t(grids),
                                                  torch.from_numpy(lab))
    return lab.astype(np.int32), mean.numpy(), sd.numpy()


def case(name, N, M, seed, sigma=False, pred=False, second=False, indexed=False):
    x, indx, y = inputs(N, M, seed)
    pars = pars_sta(M)
    S, emin, cond = check(pars, x, indx)
    vals, g = run(pars, x, indx, y)
    kw = dict(kind="hsta", x=x, indx=indx.astype(np.int32), y=y, M=M, pars=pars, hyper=mg.hyper_vec(HYPER, KEYS), prior=1, out=vals,
              grad=g, min_eig_K=emin, cond_S=cond)
    if sigma:
        kw["Sigma"] = S
    if second:
        p2 = pars_sta(M, shift=0.4)
        check(p2, x, indx)
        v2, g2 = run(p2, x, indx, y, prior=False)
        kw.update(pars2=p2, prior2=0, out2=v2, grad2=g2)
    msg = "min eig K %.3g  cond(S) %.4g" % (emin, cond)
    if pred:
        grids, pct, vmin = predict(pars, x, indx, y)
        kw.update(grids=grids, pred=pct)
        msg += "  min predictive variance %.3g" % vmin
    if indexed:
        lab, mean, sd = predict_indexed(pars, x, indx, y)
        kw.update(indx_star=lab, test_mean=mean, test_std=sd)
    print("%-16s %s" % (name, msg), flush=True)
    mg.save(name, **kw)


def gen_map():
    N, M = 77, 3
    x, indx, y = inputs(N, M, 77)
    p0 = pars_sta(M)
    p = t(p0).clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=5e-2)
    steps = 30
    hist = np.zeros(steps)
    for i in range(steps):
        opt.zero_grad()
        out = logpos.nlogpos_obj_hadamard_S(p, t(x), torch.from_numpy(indx), t(y), **HYPER)
        out.backward()
        opt.step()
        hist[i] = -float(out.detach())
    mg.save("hsta_map_N77_M3", x=x, indx=indx.astype(np.int32), y=y, M=M, pars0=p0, hyper=mg.hyper_vec(HYPER, KEYS),
            target_value_hist=hist, pars_end=p.detach().numpy(), lr=0.05, steps=steps)


CASES = [
    ("hsta_N16_M1", dict(N=16, M=1, seed=16)),                                                        # one partial tile, one label
    ("hsta_N77_M3", dict(N=77, M=3, seed=77, sigma=True, pred=True, second=True, indexed=True)),      # two tiles, ragged
    ("hsta_N200_M4", dict(N=200, M=4, seed=200, sigma=True, pred=True)),                              # four tiles
    ("hsta_N130_M8", dict(N=130, M=8, seed=130)),                                                     # the template's upper end
    ("hsta_N1100_M3", dict(N=1100, M=3, seed=1100)),                                                  # several outer panels, 18 tiles
]

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    for name, kw in CASES:
        if name.startswith(a.only):
            case(name, **kw)
    if "hsta_map_N77_M3".startswith(a.only):
        gen_map()
