"""Generate the Hadamard fixtures tests/golden/had_*.npz by RUNNING THE REFERENCE (logpos.nlogpos_obj_hadamard_SVC,
prediction.pointwise_predmap_SVC_hadamard).  Set-up (paths, the torch aliases the reference needs, helpers) is make_golden's; one
more alias is added in this process because modern torch removed ``torch.cholesky``.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_hadamard.py [--only PREFIX]

Every x holds repeated time stamps (two outputs measured together); indx is random with every label present and the last label
rare; the parameters are smooth functions of x.  The fixtures are plain data: inputs, hyper-parameters, the reference's outputs.
"""
import argparse
import contextlib
import io

import numpy as np
import torch

import make_golden as mg
from make_golden import kernels, logpos, prediction, utils, sim, t

torch.cholesky = torch.linalg.cholesky

# GP priors with SHORT length scales and two different (alpha, beta) pairs.  The reference's own prior terms carry an error of
# cond(Sigma_prior) x 1e-16 (Cholesky of RBF + 1e-6 I, whose smallest eigenvalue is the jitter: every repeated time stamp puts one
# there): sim.HYPER_SVC (alpha 10, beta 1) gives cond ~ 1e11 and gradients good to 1e-6 only, these give cond ~ 1e8, which is what
# a comparison at 1e-8 needs.  Non-zero means and a != b so that no term drops out.
HYPER = dict(mu_tilde_l=-2.4, alpha_tilde_l=1.0, beta_tilde_l=0.05, mu_L=0.3, alpha_L=1.5, beta_L=0.03, a=2.0, b=0.5)
KEYS = mg.SVC_KEYS


def inputs(N, M, seed):
    """x [N] sorted with about N / 5 repeated time stamps, indx [N], y [N]."""
    rng = np.random.default_rng(seed)
    nu = N - max(2, N // 5)
    base = np.linspace(0.05, 0.95, nu)
    x = np.sort(np.concatenate([base, rng.choice(base, N - nu, replace=False)]))
    if M == 1:
        indx = np.zeros(N, dtype=np.int64)
    else:
        indx = rng.integers(0, M - 1, N)
        rare = rng.choice(N, 2 if N < 100 else 3, replace=False)
        indx[rare] = M - 1
        for i in range(1, N):                      # a repeated time stamp carries two DIFFERENT outputs
            if x[i] == x[i - 1] and indx[i] == indx[i - 1]:
                indx[i] = (indx[i - 1] + 1) % (M - 1) if M > 2 else 1 - indx[i - 1]
        assert np.unique(indx).shape[0] == M and (indx == M - 1).sum() >= 2
    assert np.any(np.diff(x) == 0)
    y = np.sin(2.0 * np.pi * x * (indx + 1)) + 0.1 * indx
    return x, indx, y


def pars_smooth(x, M, shift=0.0):
    T = M * (M + 1) // 2
    tl = -2.5 + 0.5 * np.sin(3.0 * x + shift)
    cols = []
    for r in range(M):
        for c in range(r + 1):
            k = len(cols)
            if c == r:
                cols.append(0.8 + 0.2 * np.sin(2.0 * np.pi * x + k + shift))
            else:
                cols.append(0.1 * (k % 5 + 1) * np.cos(np.pi * x + shift) - 0.2)
    L = np.stack(cols, 1)
    assert L.shape == (x.shape[0], T)
    return np.concatenate([tl, L.reshape(-1), [np.log(1e-2) + 0.3 * shift]])


def run(pars, x, indx, y, prior=True):
    p = t(pars).clone().requires_grad_(True)
    out = logpos.nlogpos_obj_hadamard_SVC(p, t(x), torch.from_numpy(indx), t(y), **HYPER, verbose=True, Prior=prior)
    vals = np.array([float(o.detach()) for o in out])
    out[0].backward()
    return vals, p.grad.detach().numpy().copy()


def covariance(pars, x, indx):
    """(K, S = K + sigma2 I) with the reference's own functions (logpos.py:603-623)."""
    N, M = x.shape[0], int(np.unique(indx).shape[0])
    T = M * (M + 1) // 2
    p = t(pars)
    L_f_list = [utils.vec2lowtriangle(p[N + n * T: N + (n + 1) * T], M) for n in range(N)]
    K_x = kernels.Nonstationary_RBF_cov(t(x).view([-1, 1]), ell1=torch.exp(p[:N]))
    K = (K_x * logpos.generate_K_index_SVC_hadamard0(L_f_list, torch.from_numpy(indx))).numpy()
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
        pct = prediction.pointwise_predmap_SVC_hadamard(p[:N], p[N:N + N * T], p[-1], t(x), torch.from_numpy(indx), t(y), t(grids),
                                                        *h).numpy()
    var = ((pct[:, 2] - pct[:, 0]) / (2 * 1.96)) ** 2
    assert var.min() > 1e-4, "a predictive variance took the clip branch (min %g)" % var.min()
    return grids, pct, float(var.min())


def case(name, N, M, seed, sigma=False, pred=False, second=False):
    x, indx, y = inputs(N, M, seed)
    pars = pars_smooth(x, M)
    S, emin, cond = check(pars, x, indx)
    vals, g = run(pars, x, indx, y)
    kw = dict(kind="had", x=x, indx=indx.astype(np.int32), y=y, M=M, pars=pars, hyper=mg.hyper_vec(HYPER, KEYS), prior=1, out=vals,
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
    """30 steps of torch.optim.Adam (lr 0.2) on the reference objective, from the smooth point of had_N77_M3, under the LONG
    prior length scales of map_svc_N64_M3 (sim.HYPER_SVC).  Steps of 0.2 roughen the curves and the target falls from 1e3 to -6e6
    at once under either set of priors, but under HYPER's short length scales the iteration also multiplies a rounding difference
    by ~10 per step (two implementations 1e-12 apart at step 1 are 2e-2 apart at step 20); under these they stay within 3e-7."""
    N, M = 77, 3
    hyper = sim.HYPER_SVC
    x, indx, y = inputs(N, M, 77)
    p0 = pars_smooth(x, M)
    p = t(p0).clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=2e-1)
    steps = 30
    hist = np.zeros(steps)
    for i in range(steps):
        opt.zero_grad()
        out = logpos.nlogpos_obj_hadamard_SVC(p, t(x), torch.from_numpy(indx), t(y), **hyper)
        out.backward()
        opt.step()
        hist[i] = -float(out.detach())
    mg.save("had_map_N77_M3", x=x, indx=indx.astype(np.int32), y=y, M=M, pars0=p0, hyper=mg.hyper_vec(hyper, KEYS),
            target_value_hist=hist, pars_end=p.detach().numpy(), lr=0.2, steps=steps)


CASES = [
    ("had_N77_M3", dict(N=77, M=3, seed=77, sigma=True, pred=True, second=True)),      # two 64-tiles, ragged
    ("had_N200_M4", dict(N=200, M=4, seed=200, sigma=True, pred=True)),                # four tiles, ragged
    ("had_N16_M1", dict(N=16, M=1, seed=16)),                                          # degenerate: every indx = 0
    ("had_N130_M8", dict(N=130, M=8, seed=130)),                                       # the template's upper end, two rows in tile 3
    ("had_N1100_M3", dict(N=1100, M=3, seed=1100)),                                    # several 512-wide outer panels
]

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    for name, kw in CASES:
        if name.startswith(a.only):
            case(name, **kw)
    if "had_map_N77_M3".startswith(a.only):
        gen_map()
