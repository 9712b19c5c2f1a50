"""Generate the separable-Hadamard fixtures tests/golden/hsep_*.npz by RUNNING THE REFERENCE (logpos.nlogpos_obj_hadamard,
prediction.pointwise_predmap_hadmard).  Set-up (paths, the torch aliases the reference needs, helpers) is make_golden's, the
subjects are make_golden_hadamard's ``inputs()``: the same (x, indx, y) as the had_* fixtures of the nonseparable model.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_hadamard_sep.py [--only PREFIX]

The parameters are smooth functions of x plus ONE lower triangle shared by all observations.  The fixtures are plain data: inputs,
hyper-parameters, the reference's outputs (the six-entry verbose tuple, autograd gradients, the covariance, the percentiles).

hsep_map_N77_M3 is 30 steps of torch.optim.Adam at lr 0.05 under sim.HYPER_SEP.  Measured when the fixture was made: the NumPy
restatement of tests/test_hadamard_sep_cpu.py follows the first 20 recorded values within the figure its test prints (required: at
least ten times inside the 1e-6 bar the GPU driver is held to), so the run is kept at 30 recorded steps of which 20 are compared.
"""
import argparse
import contextlib
import io

import numpy as np
import torch

import make_golden as mg
from make_golden import kernels, logpos, prediction, utils, sim, t
from make_golden_hadamard import inputs

HYPER = dict(mu_tilde_l=-2.4, alpha_tilde_l=1.0, beta_tilde_l=0.05, mu_tilde_sigma=0.1, alpha_tilde_sigma=1.5, beta_tilde_sigma=0.03,
             a=2.0, b=0.5, c=3.0)
KEYS = mg.SEP_KEYS


def pars_smooth(x, M, shift=0.0):
    tl = -2.5 + 0.5 * np.sin(3.0 * x + shift)
    ts = 0.1 + 0.3 * np.cos(2.0 * np.pi * x + shift)
    Lv = []
    for r in range(M):
        for c in range(r + 1):
            k = len(Lv)
            Lv.append(0.9 + 0.05 * r + 0.1 * shift if c == r else 0.1 * (k % 5 + 1) - 0.25)
    return np.concatenate([tl, ts, Lv, [np.log(1e-2) + 0.3 * shift]])


def run(pars, x, indx, y, prior=True):
    p = t(pars).clone().requires_grad_(True)
    out = logpos.nlogpos_obj_hadamard(p, t(x), torch.from_numpy(indx), t(y), **HYPER, verbose=True, Prior=prior)
    assert len(out) == 6
    vals = np.array([float(o.detach()) for o in out])
    out[0].backward()
    return vals, p.grad.detach().numpy().copy()


def covariance(pars, x, indx):
    """(K, S = K + sigma2 I) with the reference's own functions (logpos.py:517-528)."""
    N, M = x.shape[0], int(np.unique(indx).shape[0])
    T = M * (M + 1) // 2
    p = t(pars)
    L = utils.vec2lowtriangle(p[2 * N:2 * N + T], M)
    B_f = torch.mm(L, L.t())
    K_x = kernels.Nonstationary_RBF_cov(t(x).view([-1, 1]), sigma1=torch.exp(p[N:2 * N]), ell1=torch.exp(p[:N]))
    K = (K_x * logpos.generate_K_index(B_f, torch.from_numpy(indx))).numpy()
    return K, K + float(torch.exp(p[-1])) * np.eye(N)


def check(pars, x, indx):
    K, S = covariance(pars, x, indx)
    emin = float(np.linalg.eigvalsh(K)[0])
    cond = float(np.linalg.cond(S))
    assert emin > 0.0, "K is not positive definite (min eig %g)" % emin
    assert cond < 1e6, "cond(S) = %g" % cond
    return S, emin, cond


def predict(pars, x, indx, y):
    N, M = x.shape[0], int(np.unique(indx).shape[0])
    T = M * (M + 1) // 2
    grids = np.array([-0.05, 0.1, float(x[N // 3]), 0.37, 0.5, 0.62, 0.8, 0.93, 1.02])    # one observed x, two outside its range
    p = t(pars)
    h = [HYPER[k] for k in KEYS[:6]]
    with contextlib.redirect_stdout(io.StringIO()):          # the reference prints every grid point
        pct = prediction.pointwise_predmap_hadmard(p[:N], p[N:2 * N], p[2 * N:2 * N + T], p[-1], t(x), torch.from_numpy(indx), t(y),
                                                   t(grids), *h).numpy()
    var = ((pct[:, 2] - pct[:, 0]) / (2 * 1.96)) ** 2
    assert var.min() > 1e-4, "a predictive variance took the clip branch (min %g)" % var.min()
    return grids, pct, float(var.min())


def case(name, N, M, seed, sigma=False, pred=False, second=False):
    x, indx, y = inputs(N, M, seed)
    pars = pars_smooth(x, M)
    S, emin, cond = check(pars, x, indx)
    vals, g = run(pars, x, indx, y)
    kw = dict(kind="hsep", x=x, indx=indx.astype(np.int32), y=y, M=M, pars=pars, hyper=mg.hyper_vec(HYPER, KEYS), prior=1, out=vals,
              grad=g, min_eig_K=emin, cond_S=cond)
    if sigma:
        kw["Sigma"] = S
    if second:
        p2 = pars_smooth(x, M, shift=0.4)
        check(p2, x, indx)
        v2, g2 = run(p2, x, indx, y, prior=False)
        kw.update(pars2=p2, prior2=0, out2=v2, grad2=g2)
    msg = "min eig K %.3g  cond(S) %.4g" % (emin, cond)
    if pred:
        grids, pct, vmin = predict(pars, x, indx, y)
        kw.update(grids=grids, pred=pct)
        msg += "  min predictive variance %.3g" % vmin
    print("%-16s %s" % (name, msg), flush=True)
    mg.save(name, **kw)


def gen_map():
    N, M = 77, 3
    hyper = sim.HYPER_SEP
    x, indx, y = inputs(N, M, 77)
    p0 = pars_smooth(x, M)
    p = t(p0).clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=5e-2)
    steps = 30
    hist = np.zeros(steps)
    for i in range(steps):
        opt.zero_grad()
        out = logpos.nlogpos_obj_hadamard(p, t(x), torch.from_numpy(indx), t(y), **hyper)
        out.backward()
        opt.step()
        hist[i] = -float(out.detach())
    mg.save("hsep_map_N77_M3", x=x, indx=indx.astype(np.int32), y=y, M=M, pars0=p0, hyper=mg.hyper_vec(hyper, KEYS),
            target_value_hist=hist, pars_end=p.detach().numpy(), lr=0.05, steps=steps)


CASES = [
    ("hsep_N16_M1", dict(N=16, M=1, seed=16)),                                          # one partial tile, every label 0
    ("hsep_N77_M3", dict(N=77, M=3, seed=77, sigma=True, pred=True, second=True)),      # two tiles, ragged, rare last label
    ("hsep_N200_M4", dict(N=200, M=4, seed=200, sigma=True, pred=True)),                # four tiles
    ("hsep_N130_M8", dict(N=130, M=8, seed=130)),                                       # the template's upper end
    ("hsep_N1100_M3", dict(N=1100, M=3, seed=1100)),                                    # several outer panels
]

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    for name, kw in CASES:
        if name.startswith(a.only):
            case(name, **kw)
    if "hsep_map_N77_M3".startswith(a.only):
        gen_map()
