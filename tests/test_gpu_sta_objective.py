"""The stationary (LMC) objective in the default (Cholesky) formulation on the GPU (run with -m gpu on an MI355X), M = 1 .. 8 around
every ragged edge of its kernels: nmgp_logpos_sta, nmgp_sta_batch_eval and the subject set, that is k_sta_prep_b, k_sta_blocks_b4 /
k_sta_blocks_b, the batched factorisation's substitution-based panels, k_tri_gemv_part, the inverse SYRK, k_sta_reduce_b (at
N = 961 and N = 1026 with two tiles per column group) and the host epilogue of sta_batch_core.  Cases, chains, references and bars
come from tests/sta_objective_cases.py, which tests/test_sta_objective_cpu.py checks.

What is measured, per chain (hold_sta_to_oracle of tests/test_gpu_eig_objective.py, assertions unchanged):
  priors off   likelihood 1e-10 relative; the gradient block by block (tilde_l, tilde_sigma, uL_vec, sigma2) at 1e-8 each or at the
               block's reference-derived entry of sta_objective_cases.BLOCK_BARS; NegLog == -loglik
  priors on    the standing bars: NegLog 1e-6, likelihood 1e-9 and bit-equal to the priors-off call, the components 1e-6, the prior
               part of the gradient 1e-5 in ||.||
  bits         the value-only and the value + gradient batch; a batch row and its single-chain call; a case after a larger and
               after a smaller one
Every achieved error is recorded (sta_objective/<case>/<entry>/prior<0|1>)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import objective_cases as OC
import sta_objective_cases as S
from conftest import ROOT, record_parity, relerr
from test_gpu_eig_objective import hold_sta_to_oracle, make_context

pytestmark = pytest.mark.gpu

SWEEP = "sta_objective"
CASES = S.all_cases()


@pytest.fixture(scope="module")
def ctx():
    from nonstationary_multivariate_gaussian_process_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def eig_ctx():
    c = make_context("eig")
    yield c
    c.close()


# ---------------------------------------------------------------------------------------------------
# the entries and the measures (also run by the NMGP_POISON child, which imports this module)
# ---------------------------------------------------------------------------------------------------
def hold(case, entry, got, refs, name=None):
    N, M, _ = case
    name = S.case_id(case) if name is None else name
    return hold_sta_to_oracle(name, entry, ("sta", N, M), got, refs, tag="%s/%s/%s" % (SWEEP, name, entry), bars=S.BLOCK_BARS)


def resident(ctx, case):
    x, Y, _ = S.subject(*case)
    ctx.set_data(x, Y)


def run_single(ctx, case, ks=None):
    """nmgp_logpos_sta on the chains ks: {prior: (out [len(ks), 5], grad [len(ks), T + 3])}."""
    resident(ctx, case)
    pars = S.chains(*case)
    ks = range(pars.shape[0]) if ks is None else ks
    got = {}
    for prior in (False, True):
        rows = [ctx.logpos_sta(pars[k], S.HYPER_VEC, prior=prior, want_grad=True) for k in ks]
        got[prior] = (np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]))
        assert ctx.last_sep_attempts() == 0
    return got


def run_batch(ctx, pars):
    """nmgp_sta_batch_eval on the rows of pars, with and without the gradient: {prior: (out, grad)}; status all 0 and the value-only
    call's bits those of the value + gradient call."""
    got = {}
    for prior in (False, True):
        out, grad, st = ctx.sta_batch_eval(pars, S.HYPER_VEC, prior, True)
        outv, gv, stv = ctx.sta_batch_eval(pars, S.HYPER_VEC, prior, False)
        assert gv is None and st.tolist() == [0] * len(pars) and stv.tolist() == [0] * len(pars), (st, stv)
        assert np.array_equal(outv, out), (prior, outv, out)
        got[prior] = (out, grad)
    return got


def check_single(ctx, case):
    got = run_single(ctx, case)
    hold(case, "single", got, S.refs(case))
    return got


def check_batch(ctx, case, single=None):
    """The batch against the references, and every row bit for bit against its single-chain call: under the default formulation
    nmgp_logpos_sta is the batch of one, so that the two entries cannot drift apart unnoticed."""
    B = S.batch(*case[:2])
    resident(ctx, case)
    got = run_batch(ctx, S.chains(*case)[:B])
    hold(case, "batch%d_grad" % B, got, S.refs(case, range(B)))
    single = run_single(ctx, case, range(B)) if single is None else single
    for prior in (False, True):
        assert np.array_equal(got[prior][0], single[prior][0][:B]), (case, prior, got[prior][0], single[prior][0][:B])
        assert np.array_equal(got[prior][1], single[prior][1][:B]), (case, prior)


def check_set(ctx, shape):
    """SUBJECTS x CHAINS_PER_SUBJECT rows, each against the reference of its own subject."""
    N, M = shape
    cases = [c for c in S.set_cases() if c[:2] == shape]
    xs, Ys = np.stack([S.subject(*c)[0] for c in cases]), np.stack([S.subject(*c)[1] for c in cases])
    pars = np.concatenate([S.chains(*c)[:S.CHAINS_PER_SUBJECT] for c in cases])
    refs = [r for c in cases for r in S.refs(c, range(S.CHAINS_PER_SUBJECT))]
    ctx.set_data(xs[0], Ys[0])
    ctx.sta_batch_set_subjects(xs, Ys, S.CHAINS_PER_SUBJECT)
    try:
        got = run_batch(ctx, pars)
    finally:
        ctx.sta_batch_clear_subjects()
    hold((N, M, ""), "subjects%dx%d" % (S.SUBJECTS, S.CHAINS_PER_SUBJECT), got, refs, name="set_" + OC.case_id(shape))


def compute_refs():
    for case in CASES + S.set_cases():
        S.refs(case)


# ---------------------------------------------------------------------------------------------------
# 1. nmgp_logpos_sta, every chain of every case
# ---------------------------------------------------------------------------------------------------
_SINGLE = {}


def single_results(ctx, case):
    if case not in _SINGLE:
        _SINGLE[case] = run_single(ctx, case)
    return _SINGLE[case]


@pytest.mark.parametrize("case", CASES, ids=S.case_id)
def test_single_chain_entry_block_by_block(ctx, case):
    hold(case, "single", single_results(ctx, case), S.refs(case))


# ---------------------------------------------------------------------------------------------------
# 2. nmgp_sta_batch_eval
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=S.case_id)
def test_batch_entry_block_by_block(ctx, case):
    check_batch(ctx, case, single_results(ctx, case))


# ---------------------------------------------------------------------------------------------------
# 3. the subject sets
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", S.SET_SHAPES, ids=OC.case_id)
def test_every_row_of_a_subject_set_against_its_own_subjects_reference(ctx, shape):
    check_set(ctx, shape)


# ---------------------------------------------------------------------------------------------------
# 4. call history
# ---------------------------------------------------------------------------------------------------
def test_a_case_has_the_same_bits_after_a_larger_and_after_a_smaller_one(ctx):
    """From the largest case to the smallest and back: on the way down the slab SL_BIG is larger than the case needs and holds the
    previous case's data."""
    order = sorted(CASES, key=lambda c: (-c[0], -c[1], c[2]))
    passes = []
    for cases in (order, order[::-1]):
        res = {}
        for case in cases:
            B = S.batch(*case[:2])
            resident(ctx, case)
            pars = S.chains(*case)
            res[case] = (ctx.logpos_sta(pars[0], S.HYPER_VEC, prior=True, want_grad=True),
                         ctx.sta_batch_eval(pars[:B], S.HYPER_VEC, True, True)[:2])
        passes.append(res)
    for other in passes[1:]:
        for case in order:
            for a, b in zip(passes[0][case], other[case]):
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), case


# ---------------------------------------------------------------------------------------------------
# 5. once more with every fresh buffer and scratch hand-out full of NaNs
# ---------------------------------------------------------------------------------------------------
POISON_SNIPPET = r'''
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import sta_objective_cases as S
import test_gpu_sta_objective as t
from nonstationary_multivariate_gaussian_process_amd import _lib
S.load_refs(%(refs)r)
ctx = _lib.Context(0)
n = 0
for case in t.CASES + t.CASES[::-1]:
    t.check_batch(ctx, case, t.check_single(ctx, case))
    n += 1
for shape in S.SET_SHAPES + S.SET_SHAPES[::-1]:
    t.check_set(ctx, shape)
    n += 1
ctx.close()
print("POISON_OK", n)
'''


def test_sweep_under_poison(tmp_path):
    """NMGP_POISON=1 (read once per process: a child) fills fresh buffers and every scratch hand-out with NaNs: an element the
    entries read without having written it -- the element above a straddling row pair, a partial of a column group without tiles, a
    pad slot of the reduction's LDS columns -- shows up.  1. to 3. forwards then backwards at the same bars; the references go to the
    child in a file, so that they are computed once."""
    compute_refs()
    path = str(tmp_path / "refs.npz")
    S.save_refs(path)
    env = dict(os.environ)
    env["NMGP_POISON"] = "1"
    env.pop("NMGP_STA_BATCH_MAX", None)
    out = subprocess.run([sys.executable, "-c", POISON_SNIPPET % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "refs": path}],
                         capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0 and "POISON_OK %d" % (2 * len(CASES) + 2 * len(S.SET_SHAPES)) in out.stdout, \
        out.stdout[-4000:] + out.stderr[-4000:]


# ---------------------------------------------------------------------------------------------------
# 6. recorded, not barred: the distance to the eigen formulation
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=S.case_id)
def test_distance_to_the_eigen_formulation_is_recorded(ctx, eig_ctx, case):
    """No bar of its own: both formulations are held to the reference (here and in tests/test_gpu_eig_objective.py).  Per block, so
    that the tilde_l figure stands where DESIGN.md quotes it."""
    N, M, _ = case
    chol = single_results(ctx, case)
    resident(eig_ctx, case)
    rows = [eig_ctx.logpos_sta(p, S.HYPER_VEC, prior=False, want_grad=True) for p in S.chains(*case)]
    el = max(relerr(r[0][1], o[1]) for r, o in zip(rows, chol[False][0]))
    tab = {}
    for r, g in zip(rows, chol[False][1]):
        for name, e in OC.block_table(g, r[1], ("sta", N, M)).items():
            tab[name] = max(tab.get(name, 0.0), e)
    print("%s/%s default vs eig: loglik %.3g blocks %s" % (SWEEP, S.case_id(case), el, " ".join("%s=%.3g" % kv for kv in tab.items())))
    record_parity("%s/%s/single_vs_eig/prior0" % (SWEEP, S.case_id(case)), loglik=el, **tab)
    assert np.isfinite(el) and all(np.isfinite(v) for v in tab.values())
