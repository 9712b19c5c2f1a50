"""The left-looking 256-column nodes of the throughput schedule (k_leaf_step: the K = 128 update between two 128-column leaves
folded into the right leaf's catch-up) must give the BITS of the default schedule, which for these small batches is the
fused-step one: every C entry receives the same products in the same order through the same MFMA k-groups.  Each
configuration runs once in a child process (the schedule switches are read once per process); NMGP_CHOL_FUSED_MAX_BATCH=0 sends
the small batches through the throughput schedule, as in test_gpu_variants.py.

Sizes of the structured value path (order N = A with its N riding rows of L^-T, order 2N = Sigma'; 512-wide outer panels at these
batch sizes): N = 256 one 256-column node alone in A and two under a K = 256 update in Sigma'; 320 splits A into 192 + 128 (a
192-wide node and a lone leaf, which keep the update launch and the two-launch leaf) and Sigma' into a panel of two nodes and a
128-column one; 512 two nodes under a K = 256 update in A and a panel boundary at 512 in Sigma'; 576 the boundary followed by a
64-column panel in A; 768 a node alone in A's second panel and three panels in Sigma'."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, SEP_KEYS, SVC_KEYS, relerr, vec_relerr

pytestmark = pytest.mark.gpu

VALUE_SIZES = (256, 320, 512, 576, 768)
# the bars of test_gpu_parity.py / test_svc_schur.py against the reference: log posterior and priors, likelihood term, gradient
VAL_TOL, LIK_TOL, GRAD_TOL = 1e-6, 1e-9, 1e-5

SNIPPET = r"""
import json, sys
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import test_gpu_chol_leftlooking as t
from nonstationary_multivariate_gaussian_process_amd import _lib
res = {}
def put(name, a):
    a = np.ascontiguousarray(a)
    res[name] = [str(a.dtype), list(a.shape), a.tobytes().hex()]
ctx = _lib.Context(0)
for case in sys.argv[1:]:
    kind, N = case.split(":")
    N = int(N)
    if kind == "value":
        d, pars = t.value_case(N)
        ctx.set_data(d["x"], d["Y"])
        ctx.svc_batch_alloc(pars.shape[0])
        ctx.svc_batch_set_pars(pars)
        ctx.svc_batch_eval(t.svc_hyper(), True, want_grad=False)
        out, status = ctx.svc_batch_fetch()
    elif kind == "grad":
        d, pars = t.grad_case()
        ctx.set_data(d["x"], d["Y"])
        ctx.svc_batch_alloc(pars.shape[0])
        ctx.svc_batch_set_pars(pars)
        ctx.svc_batch_eval(t.svc_hyper(), True, want_grad=True)
        out, status = ctx.svc_batch_fetch()
        put(case + ":grad", ctx.svc_batch_fetch_grad())
    elif kind == "failed":
        d, pars = t.failed_case()
        ctx.set_data(d["x"], d["Y"])
        ctx.svc_batch_alloc(pars.shape[0])
        ctx.svc_batch_set_pars(pars)
        ctx.svc_batch_eval(t.svc_hyper(), True, want_grad=False)
        out, status = ctx.svc_batch_fetch()
    else:
        d, pars = t.sep_case()
        ctx.set_data(d["x"], d["Y"])
        out, _, status = ctx.sep_batch_eval(pars, t.sep_hyper(), True, False)
    put(case + ":out", out)
    put(case + ":status", status)
ctx.close()
print(json.dumps(res))
"""


def svc_hyper():
    from nonstationary_multivariate_gaussian_process_amd import sim
    return [sim.HYPER_SVC[k] for k in SVC_KEYS]


def sep_hyper():
    from nonstationary_multivariate_gaussian_process_amd import sim
    return [sim.HYPER_SEP[k] for k in SEP_KEYS]


@functools.lru_cache(maxsize=None)
def _svc_chains(N, M, B, seed):
    from nonstationary_multivariate_gaussian_process_amd import sim
    d = sim.simulate_nonseparable(N, M, seed=seed)
    return d, np.stack([sim.perturb(d["pars_true"], 0.05, 0.2 + 0.11 * k) for k in range(B)])


def value_case(N):
    return _svc_chains(N, 3, 4, 1200 + N)


def grad_case():
    return _svc_chains(256, 3, 5, 1301)


def failed_case():
    """The parameters of test_svc_schur.py::test_structured_status_matches_dense_on_failed_chains."""
    N, M, B = 256, 3, 4
    T = M * (M + 1) // 2
    d, pars = _svc_chains(N, M, B, 911)
    pars = pars.copy()
    pars[1, -1] = np.nan                      # sigma2: every entry of Sigma undefined
    pars[2, N + 5 * T + 2] = np.nan           # L_5[1, 1]: only the output-1 rows of location 5 (and below)
    return d, pars


@functools.lru_cache(maxsize=None)
def sep_case():
    from nonstationary_multivariate_gaussian_process_amd import sim
    d = sim.simulate_separable(512, 5, seed=1405)
    return d, np.stack([sim.perturb(d["pars_true"], 0.03, 0.3 + 0.2 * k) for k in range(4)])


ALL_CASES = tuple("value:%d" % N for N in VALUE_SIZES) + ("grad:256", "failed:256", "sep:512")


@functools.lru_cache(maxsize=None)
def run_child(throughput, poison, cases):
    """One child process: `cases` under the throughput schedule (or the default one), name -> array with the child's bits."""
    env = dict(os.environ)
    env.pop("NMGP_CHOL_FUSED_MAX_BATCH", None)
    env.pop("NMGP_POISON", None)
    if throughput:
        env["NMGP_CHOL_FUSED_MAX_BATCH"] = "0"
    if poison:
        env["NMGP_POISON"] = "1"
    out = subprocess.run([sys.executable, "-c", SNIPPET % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}] + list(cases),
                         capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    raw = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    return {k: np.frombuffer(bytes.fromhex(h), dtype=dt).reshape(shape) for k, (dt, shape, h) in raw.items()}


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("N", VALUE_SIZES)
def test_structured_value_path_gives_the_default_schedules_bits_and_the_oracles_values(N):
    from oracle import nmgp_oracle as O
    from nonstationary_multivariate_gaussian_process_amd import sim
    new, ref = run_child(True, False, ALL_CASES), run_child(False, False, ALL_CASES)
    out, status = new["value:%d:out" % N], new["value:%d:status" % N]
    assert np.all(status == 0) and np.all(np.isfinite(out))
    assert same_bits(status, ref["value:%d:status" % N])
    assert same_bits(out, ref["value:%d:out" % N]), (out, ref["value:%d:out" % N])
    d, pars = value_case(N)
    for k in range(pars.shape[0]):
        want = np.array(O.nlogpos_obj_SVC(pars[k], d["Y"], d["x"], **sim.HYPER_SVC, verbose=True), dtype=np.float64)
        assert relerr(out[k][1], want[1]) < LIK_TOL, (N, k, out[k], want)
        assert relerr(out[k], want) < VAL_TOL, (N, k, out[k], want)


def test_value_and_gradient_with_fresh_rows_at_every_subtree():
    """n = 768 with xtri = n: rows of L^-T enter at every step of every node and of the 192-wide remainder."""
    from oracle import nmgp_oracle as O
    from nonstationary_multivariate_gaussian_process_amd import sim
    new, ref = run_child(True, False, ALL_CASES), run_child(False, False, ALL_CASES)
    assert np.all(new["grad:256:status"] == 0)
    for key in ("grad:256:out", "grad:256:status", "grad:256:grad"):
        assert same_bits(new[key], ref[key]), key
    d, pars = grad_case()
    for k in range(pars.shape[0]):
        want, gwant = O.nlogpos_obj_SVC(pars[k], d["Y"], d["x"], **sim.HYPER_SVC, verbose=True, grad=True)
        assert relerr(new["grad:256:out"][k][1], want[1]) < LIK_TOL
        assert relerr(new["grad:256:out"][k], np.array(want, dtype=np.float64)) < VAL_TOL
        assert vec_relerr(new["grad:256:grad"][k], gwant) < GRAD_TOL


def test_a_failing_chain_reports_the_default_schedules_status():
    """The diagonal blocks (2, 2) and (3, 3) of a node are factored inside the leaf launches: their status words carry the
    right column offset."""
    new, ref = run_child(True, False, ALL_CASES), run_child(False, False, ALL_CASES)
    s = new["failed:256:status"]
    assert s[0] == 0 and s[3] == 0 and s[1] != 0 and s[2] > 256
    assert same_bits(s, ref["failed:256:status"]), (s, ref["failed:256:status"])
    assert same_bits(new["failed:256:out"][[0, 3]], ref["failed:256:out"][[0, 3]])


def test_nothing_unwritten_is_read_under_poison():
    """NMGP_POISON=1 fills fresh buffers with NaNs: the catch-up of the rows of L^-T stays inside what was seeded or written."""
    case = ("value:%d" % VALUE_SIZES[0],)
    new, ref = run_child(True, True, case), run_child(False, False, ALL_CASES)
    assert np.all(new[case[0] + ":status"] == 0) and np.all(np.isfinite(new[case[0] + ":out"]))
    assert same_bits(new[case[0] + ":out"], ref[case[0] + ":out"])


def test_separable_batch_without_riding_rows():
    """4 chains x 5 blocks of n = 512: 20 matrices, one 512-wide panel of two 256-column nodes each, nothing below the matrix."""
    new, ref = run_child(True, False, ALL_CASES), run_child(False, False, ALL_CASES)
    assert np.all(new["sep:512:status"] == 0) and np.all(np.isfinite(new["sep:512:out"]))
    assert same_bits(new["sep:512:status"], ref["sep:512:status"])
    assert same_bits(new["sep:512:out"], ref["sep:512:out"])
