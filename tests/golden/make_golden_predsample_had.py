"""Generate the fixture tests/golden/hpn_N77_M3.npz by RUNNING THE REFERENCE's held-out MAP predictor of the nonseparable Hadamard
model (prediction.test_predmap_SVC_hadamard, prediction.py:1480-1561) on had_N77_M3's subject and parameters.  Set-up (paths, the
torch aliases the reference needs, helpers) is make_golden's, the subject and parameters make_golden_hadamard's.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_predsample_had.py

12 held-out pairs: labels cycling 0, 1, 2, one x equal to a training input, one outside the range.  The reference returns, per pair,
the mean of output indx_test[s] and -- whatever the label -- the variance (A - B)[0, 0] + sigma2_err with A = (1 + 1e-6) L* L*^T: it
is the predictive variance at the label-0 pairs only.  Both are recorded as they come; the tests compare the
variance where the label is 0.  The fixture is plain data: inputs, labels, the reference's outputs.
"""
import contextlib
import io

import numpy as np
import torch

import make_golden as mg
import make_golden_hadamard as mh
from make_golden import prediction, t

N, M, SEED = 77, 3, 77

if __name__ == "__main__":
    x, indx, y = mh.inputs(N, M, SEED)
    pars = mh.pars_smooth(x, M)
    T = M * (M + 1) // 2
    x_test = np.array([-0.04, 0.08, 0.21, float(x[N // 2]), 0.33, 0.41, 0.5, 0.58, 0.66, 0.77, 0.86, 0.94])
    indx_test = (np.arange(12) % M).astype(np.int32)
    assert x_test[3] in x and (x_test < x.min()).sum() == 1 and x_test.max() < x.max()
    p = t(pars)
    h = [mh.HYPER[k] for k in mh.KEYS[:6]]
    with contextlib.redirect_stdout(io.StringIO()):          # the reference prints every pair
        mean, var = prediction.test_predmap_SVC_hadamard(p[:N], p[N:N + N * T], p[-1], t(x), torch.from_numpy(indx), t(y), t(x_test),
                                                         torch.from_numpy(indx_test.astype(np.int64)), *h)
    mean, var = mean.numpy(), var.numpy()
    assert mean.shape == var.shape == (12,) and var[indx_test == 0].min() > 1e-4, var
    print("mean", mean, "\nvar", var, flush=True)
    mg.save("hpn_N77_M3", kind="hpn", x=x, indx=indx.astype(np.int32), y=y, M=M, pars=pars, hyper=mg.hyper_vec(mh.HYPER, mh.KEYS),
            x_test=x_test, indx_test=indx_test, mean=mean, var=var)
