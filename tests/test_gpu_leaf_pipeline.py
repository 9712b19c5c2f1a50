"""The leaf launches of a 256-column node (k_leaf_step) keep the next previous block's row loads in flight under the MFMAs of the
current one: the loads of block p + 1's 16-column group go into the registers group sg of block p has just finished with, as
buffer loads whose masked lanes lie outside the descriptor's range.  What such a pipelined load can get wrong, and
test_gpu_chol_leftlooking.py does not cover:

  * unwritten memory: a prefetch that reaches it shows as NaN or as changed bits under NMGP_POISON=1 (fresh buffers are NaN-filled)
    -- value N = 320 and 576, gradient N = 256 (rows of L^-T entering at every step), the separable batch of n = 512;
  * M = 2 and M = 4 outputs at N = 256 and 320: Sigma' of order N and 3 N, other numbers of row blocks per workgroup column and
    other 192 + 128 splits than M = 3;
  * an odd batch (9 chains): T * batch of the role-major workgroup ids is no multiple of 8;
  * fewer than 64 rows below the last block of a node: M = 2, N = 256 makes Sigma' ONE node of order 256 with the single
    right-hand-side row below it, so the last launch is workgroup 0 alone with one valid lane and 255 masked ones (and in the A
    phase the rows of L^-T end inside a wave).  It runs under poison as well.

Every case must give the BITS of the default schedule (the fused-step one at these batch sizes), status 0 and the oracle's values at
the bars of test_gpu_chol_leftlooking.py.  Each configuration runs once in a child process, as there: the schedule switches are read
once per process, NMGP_CHOL_FUSED_MAX_BATCH=0 sends small batches through the leaf kernels."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_chol_leftlooking as base
from conftest import ROOT, relerr, vec_relerr

pytestmark = pytest.mark.gpu

VAL_TOL, LIK_TOL, GRAD_TOL = base.VAL_TOL, base.LIK_TOL, base.GRAD_TOL
SEP_LIK_TOL = 1e-8                       # the separable model's likelihood bar (test_gpu_parity.py); the base file sets none for it

# (N, M, chains) of the nonseparable value step
SHAPE_CASES = ((256, 2, 4), (320, 2, 4), (256, 4, 4), (320, 4, 4), (256, 3, 9))
FEW_ROWS_CASE = (256, 2, 4)
POISON_BASE_CASES = ("value:320", "value:576", "grad:256", "sep:512")

SNIPPET = r"""
import json, sys
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import test_gpu_leaf_pipeline as t
from nonstationary_multivariate_gaussian_process_amd import _lib
res = {}
ctx = _lib.Context(0)
for case in sys.argv[1:]:
    N, M, B = (int(v) for v in case.split(":"))
    d, pars = t.shape_case(N, M, B)
    ctx.set_data(d["x"], d["Y"])
    ctx.svc_batch_alloc(B)
    ctx.svc_batch_set_pars(pars)
    ctx.svc_batch_eval(t.base.svc_hyper(), True, want_grad=False)
    out, status = ctx.svc_batch_fetch()
    for name, a in ((case + ":out", out), (case + ":status", status)):
        a = np.ascontiguousarray(a)
        res[name] = [str(a.dtype), list(a.shape), a.tobytes().hex()]
ctx.close()
print(json.dumps(res))
"""


def shape_case(N, M, B):
    return base._svc_chains(N, M, B, 1500 + N + 10 * M + B)


def key(case):
    return "%d:%d:%d" % case


@functools.lru_cache(maxsize=None)
def run_child(throughput, poison, cases):
    """One child process: the (N, M, chains) `cases` under the throughput schedule (or the default one), name -> array."""
    env = dict(os.environ)
    env.pop("NMGP_CHOL_FUSED_MAX_BATCH", None)
    env.pop("NMGP_POISON", None)
    if throughput:
        env["NMGP_CHOL_FUSED_MAX_BATCH"] = "0"
    if poison:
        env["NMGP_POISON"] = "1"
    out = subprocess.run([sys.executable, "-c", SNIPPET % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}]
                         + [key(c) for c in cases], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    raw = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    return {k: np.frombuffer(bytes.fromhex(h), dtype=dt).reshape(shape) for k, (dt, shape, h) in raw.items()}


@functools.lru_cache(maxsize=None)
def svc_oracle(N, M, B):
    from oracle import nmgp_oracle as O
    from nonstationary_multivariate_gaussian_process_amd import sim
    d, pars = shape_case(N, M, B)
    return np.array([O.nlogpos_obj_SVC(pars[k], d["Y"], d["x"], **sim.HYPER_SVC, verbose=True) for k in range(B)], dtype=np.float64)


def check_svc_values(out, want, what):
    for k in range(want.shape[0]):
        assert relerr(out[k][1], want[k][1]) < LIK_TOL, (what, k, out[k], want[k])
        assert relerr(out[k], want[k]) < VAL_TOL, (what, k, out[k], want[k])


def default_bits():
    return run_child(False, False, SHAPE_CASES)


@pytest.mark.parametrize("case", SHAPE_CASES, ids=key)
def test_other_output_counts_and_an_odd_batch_give_the_default_schedules_bits(case):
    new, ref = run_child(True, False, SHAPE_CASES), default_bits()
    out, status = new[key(case) + ":out"], new[key(case) + ":status"]
    assert np.all(status == 0) and np.all(np.isfinite(out))
    assert base.same_bits(status, ref[key(case) + ":status"])
    assert base.same_bits(out, ref[key(case) + ":out"]), (out, ref[key(case) + ":out"])
    check_svc_values(out, svc_oracle(*case), case)


def test_one_row_below_the_last_block_of_a_node_under_poison():
    """M = 2, N = 256: Sigma' is one node with one row below it -- the last launch is workgroup 0 alone, 255 of its 256 row lanes
    masked.  Under poison a masked lane that fetched anything, or a valid one that fetched ahead of what is written, shows."""
    k = key(FEW_ROWS_CASE)
    new, ref = run_child(True, True, (FEW_ROWS_CASE,)), default_bits()
    assert np.all(new[k + ":status"] == 0) and np.all(np.isfinite(new[k + ":out"]))
    assert base.same_bits(new[k + ":status"], ref[k + ":status"])
    assert base.same_bits(new[k + ":out"], ref[k + ":out"]), (new[k + ":out"], ref[k + ":out"])
    check_svc_values(new[k + ":out"], svc_oracle(*FEW_ROWS_CASE), FEW_ROWS_CASE)


def poisoned():
    return base.run_child(True, True, POISON_BASE_CASES), base.run_child(False, False, base.ALL_CASES)


@pytest.mark.parametrize("N", (320, 576))
def test_value_step_reads_nothing_unwritten_under_poison(N):
    from oracle import nmgp_oracle as O
    from nonstationary_multivariate_gaussian_process_amd import sim
    new, ref = poisoned()
    out, status = new["value:%d:out" % N], new["value:%d:status" % N]
    assert np.all(status == 0) and np.all(np.isfinite(out))
    assert base.same_bits(status, ref["value:%d:status" % N])
    assert base.same_bits(out, ref["value:%d:out" % N]), (out, ref["value:%d:out" % N])
    d, pars = base.value_case(N)
    want = np.array([O.nlogpos_obj_SVC(pars[k], d["Y"], d["x"], **sim.HYPER_SVC, verbose=True) for k in range(pars.shape[0])],
                    dtype=np.float64)
    check_svc_values(out, want, N)


def test_gradient_step_reads_nothing_unwritten_under_poison():
    """N = 256 with the rows of L^-T entering at every step of every node: their blocks right of the seeded band are unwritten
    (NaN under poison) until the launch that owns them."""
    from oracle import nmgp_oracle as O
    from nonstationary_multivariate_gaussian_process_amd import sim
    new, ref = poisoned()
    assert np.all(new["grad:256:status"] == 0)
    assert np.all(np.isfinite(new["grad:256:out"])) and np.all(np.isfinite(new["grad:256:grad"]))
    for k in ("grad:256:out", "grad:256:status", "grad:256:grad"):
        assert base.same_bits(new[k], ref[k]), k
    d, pars = base.grad_case()
    for k in range(pars.shape[0]):
        want, gwant = O.nlogpos_obj_SVC(pars[k], d["Y"], d["x"], **sim.HYPER_SVC, verbose=True, grad=True)
        assert relerr(new["grad:256:out"][k][1], want[1]) < LIK_TOL
        assert relerr(new["grad:256:out"][k], np.array(want, dtype=np.float64)) < VAL_TOL
        assert vec_relerr(new["grad:256:grad"][k], gwant) < GRAD_TOL


def test_separable_batch_reads_nothing_unwritten_under_poison():
    """4 chains x 5 blocks of n = 512: two nodes per matrix, the right-hand-side row alone below the second."""
    from oracle import nmgp_oracle as O
    from nonstationary_multivariate_gaussian_process_amd import sim
    new, ref = poisoned()
    out = new["sep:512:out"]
    assert np.all(new["sep:512:status"] == 0) and np.all(np.isfinite(out))
    assert base.same_bits(new["sep:512:status"], ref["sep:512:status"])
    assert base.same_bits(out, ref["sep:512:out"]), (out, ref["sep:512:out"])
    d, pars = base.sep_case()
    for k in range(pars.shape[0]):
        want = np.array(O.nlogpos_obj(pars[k], d["Y"], d["x"], **sim.HYPER_SEP, verbose=True), dtype=np.float64)
        assert relerr(out[k][1], want[1]) < SEP_LIK_TOL, (k, out[k], want)
        assert relerr(out[k], want) < VAL_TOL, (k, out[k], want)
