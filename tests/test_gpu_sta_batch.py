"""Batched stationary (LMC) objective nmgp_sta_batch_eval on the GPU (run with -m gpu on an MI355X): parity against the reference's
recorded runs, the CPU oracle, the single-chain entry nmgp_logpos_sta and the separable batch with constant curves; the bits of a chain
whatever the batch, the chunking and the workspace hold; failure handling; the subject set; the lock-step drivers.  Subjects, chains
and oracle values come from tests/sta_batch_cases.py, which the CPU half checks."""
import os
import subprocess
import sys

import numpy as np
import pytest

import sta_batch_cases as C
from conftest import ROOT, SEP_KEYS, STA_KEYS, golden, hyper_dict, record_parity, relerr, vec_relerr

pytestmark = pytest.mark.gpu

SWEEP = [(s, False) for s in C.SHAPES] + [(C.UNSORTED, True)]


def sweep_id(case):
    return C.case_id(case[0]) + ("_unsorted" if case[1] else "")


@pytest.fixture(scope="module")
def ctx():
    from nonstationary_multivariate_gaussian_process_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def resident(ctx, shape, unsorted=False):
    x, Y, _ = C.subject(shape[0], shape[1], unsorted)
    ctx.set_data(x, Y)                                  # (also drops a subject set)
    return x, Y


# ---------------------------------------------------------------------------------------------------
# 1. parity
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sta_rngfree_N8_M3", "sta_rngfree_N64_M3", "sta_sim_N128_M2"])
def test_chain_0_of_a_batch_of_4_against_the_reference_golden(ctx, name):
    """The reference's recorded runs at test_sta_against_reference_golden's bars: out 1e-8 relative, gradient 1e-8 in ||d|| / ||g||."""
    from nonstationary_multivariate_gaussian_process_amd import sim
    g = golden(name)
    ctx.set_data(g["x"], g["Y"])
    pars = np.stack([g["pars"]] + [sim.perturb(g["pars"], 0.05, 0.4 * k) for k in (1, 2, 3)])
    out, grad, st = ctx.sta_batch_eval(pars, g["hyper"], prior=True, want_grad=True)
    assert st.tolist() == [0, 0, 0, 0]
    eo, eg = relerr(out[0], g["out"]), vec_relerr(grad[0], g["grad"])
    print("%s chain 0 of 4 vs reference: out %.3g grad %.3g" % (name, eo, eg))
    record_parity("stab_" + name, components=(eo, 1e-8), grad=(eg, 1e-8))
    assert eo < 1e-8, (out[0], g["out"])
    assert eg < 1e-8, (grad[0], g["grad"])


@pytest.mark.parametrize("prior", [True, False], ids=["prior", "likelihood"])
@pytest.mark.parametrize("case", SWEEP, ids=sweep_id)
def test_sweep_against_the_oracle(ctx, case, prior):
    """Every shared shape, priors on and off: likelihood 1e-8 relative, gradient 1e-7 in ||d|| / ||g||."""
    (N, M), uns = case
    resident(ctx, (N, M), uns)
    pars = C.chains(N, M, unsorted=uns)
    ref, gref = C.oracle(N, M, prior, uns)
    out, grad, st = ctx.sta_batch_eval(pars, C.HYPER_VEC, prior=prior, want_grad=True)
    assert st.tolist() == [0] * C.B_CHAINS and np.all(np.isfinite(out)) and np.all(np.isfinite(grad))
    ll_ref = ref[:, 1] if prior else -ref[:, 0]
    el = max(relerr(out[b][1], ll_ref[b]) for b in range(C.B_CHAINS))
    en = max(relerr(out[b][0], ref[b][0]) for b in range(C.B_CHAINS))
    eg = max(vec_relerr(grad[b], gref[b]) for b in range(C.B_CHAINS))
    print("%s prior=%s vs oracle: loglik %.3g neglog %.3g grad %.3g" % (sweep_id(case), prior, el, en, eg))
    record_parity("stab_%s_%s_vs_oracle" % (sweep_id(case), "prior" if prior else "lik"), loglik=(el, 1e-8), neglog=en, grad=(eg, 1e-7))
    assert el < 1e-8 and eg < 1e-7, (el, eg)
    if not prior:
        assert np.array_equal(out[:, 0], -out[:, 1])    # nmgp_logpos_sta's behaviour with prior = 0: NegLog = -loglik


@pytest.mark.parametrize("case", SWEEP, ids=sweep_id)
def test_sweep_against_the_single_chain_entry(ctx, case):
    """Per chain against nmgp_logpos_sta at the bars nmgp_sep_batch_eval is held to against its single-chain entry: likelihood 1e-10,
    out 1e-9, gradient 1e-8.  (Under the default formulation nmgp_logpos_sta has since become this batch with B = 1, so the two sides
    are the same bits and the comparison measures nothing independent any more; tests/test_gpu_sta_objective.py holds both entries
    block by block to CPU references.  Before that: gradient 9.6e-9 at N200_M6 and 3.8e-9 at N129_M8, most of it the single-chain
    entry's.)"""
    (N, M), uns = case
    resident(ctx, (N, M), uns)
    pars = C.chains(N, M, unsorted=uns)
    out, grad, st = ctx.sta_batch_eval(pars, C.HYPER_VEC, prior=True, want_grad=True)
    assert st.tolist() == [0] * C.B_CHAINS
    el = eo = eg = 0.0
    for b in range(C.B_CHAINS):
        so, sg = ctx.logpos_sta(pars[b], C.HYPER_VEC, prior=True, want_grad=True)
        el, eo, eg = max(el, relerr(out[b][1], so[1])), max(eo, relerr(out[b], so)), max(eg, vec_relerr(grad[b], sg))
    print("%s vs nmgp_logpos_sta: loglik %.3g out %.3g grad %.3g" % (sweep_id(case), el, eo, eg))
    record_parity("stab_%s_vs_single" % sweep_id(case), loglik=(el, 1e-10), out5=(eo, 1e-9), grad=(eg, 1e-8))
    assert el < 1e-10 and eo < 1e-9 and eg < 1e-8, (el, eo, eg)


@pytest.mark.parametrize("shape", [(2, 2), (8, 8), (65, 3), (128, 4), (257, 7)], ids=C.case_id)
def test_against_the_separable_batch_with_constant_curves(ctx, shape):
    """nmgp_sep_batch_eval with tilde_l and tilde_sigma constant over the locations and prior = 0 is the same likelihood: it and the
    T + 1 gradient entries the two layouts share (uL_vec, tilde_sigma2_err) within the single-chain bars (1e-10, 1e-8); the two scalar
    entries are the sums of the separable gradient's per-location halves."""
    from nonstationary_multivariate_gaussian_process_amd import sim
    N, M = shape
    resident(ctx, shape)
    pars = C.chains(N, M)
    sep = np.stack([np.concatenate([np.full(N, p[0]), np.full(N, p[1]), p[2:]]) for p in pars])
    out, grad, st = ctx.sta_batch_eval(pars, C.HYPER_VEC, prior=False, want_grad=True)
    so, sg, ss = ctx.sep_batch_eval(sep, np.array([sim.HYPER_SEP[k] for k in SEP_KEYS]), False, True)
    assert st.tolist() == [0] * C.B_CHAINS and ss.tolist() == [0] * C.B_CHAINS
    el = max(relerr(out[b][1], so[b][1]) for b in range(C.B_CHAINS))
    eg = max(vec_relerr(grad[b][2:], sg[b][2 * N:]) for b in range(C.B_CHAINS))
    es = max(vec_relerr(grad[b][:2], [sg[b][:N].sum(), sg[b][N:2 * N].sum()]) for b in range(C.B_CHAINS))
    print("%s vs sep batch, constant curves: loglik %.3g shared grad %.3g scalar curves %.3g" % (C.case_id(shape), el, eg, es))
    record_parity("stab_%s_vs_sep_constant" % C.case_id(shape), loglik=(el, 1e-10), grad_shared=(eg, 1e-8), grad_scalar_sums=es)
    assert el < 1e-10 and eg < 1e-8, (el, eg)


# ---------------------------------------------------------------------------------------------------
# 2. bit for bit
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SWEEP, ids=sweep_id)
def test_a_chain_has_the_bits_of_its_single_chain_call_and_of_the_value_only_call(ctx, case):
    (N, M), uns = case
    resident(ctx, (N, M), uns)
    pars = C.chains(N, M, unsorted=uns)
    out, grad, st = ctx.sta_batch_eval(pars, C.HYPER_VEC, prior=True, want_grad=True)
    outv, gv, stv = ctx.sta_batch_eval(pars, C.HYPER_VEC, prior=True, want_grad=False)
    assert gv is None and st.tolist() == [0] * C.B_CHAINS and stv.tolist() == [0] * C.B_CHAINS
    assert np.array_equal(out, outv)
    for b in range(C.B_CHAINS):
        o1, g1, s1 = ctx.sta_batch_eval(pars[b], C.HYPER_VEC, prior=True, want_grad=True)      # one vector: B = 1, the same kernels
        assert s1.tolist() == [0] and o1.shape == (1, 5)
        assert np.array_equal(o1[0], out[b]) and np.array_equal(g1[0], grad[b]), (sweep_id(case), b)


def test_a_chunk_cap_of_3_leaves_the_bits_of_8_chains(ctx, monkeypatch):
    N, M = 65, 3
    resident(ctx, (N, M))
    pars = C.chains(N, M, 8)
    monkeypatch.delenv("NMGP_STA_BATCH_MAX", raising=False)
    full = ctx.sta_batch_eval(pars, C.HYPER_VEC, prior=True, want_grad=True)
    monkeypatch.setenv("NMGP_STA_BATCH_MAX", "3")                     # read at call time: chunks of 3, 3, 2 chains
    capped = ctx.sta_batch_eval(pars, C.HYPER_VEC, prior=True, want_grad=True)
    capped_v = ctx.sta_batch_eval(pars, C.HYPER_VEC, prior=True, want_grad=False)
    assert full[2].tolist() == [0] * 8 and capped[2].tolist() == [0] * 8
    assert np.array_equal(full[0], capped[0]) and np.array_equal(full[1], capped[1]) and np.array_equal(full[0], capped_v[0])


def test_300_chains_past_the_latency_regime_against_the_first_four_alone(ctx):
    """B M N = 76,800 crosses the 73,728 at which the factorisation changes its schedule for the fast panel kernels: the substitution-
    based ones must not notice."""
    N, M, B = 128, 2, 300
    resident(ctx, (N, M))
    pars = C.chains(N, M, B)
    assert B * M * N > 73728
    out, grad, st = ctx.sta_batch_eval(pars, C.HYPER_VEC, prior=True, want_grad=True)
    o4, g4, s4 = ctx.sta_batch_eval(pars[:4], C.HYPER_VEC, prior=True, want_grad=True)
    assert st.tolist() == [0] * B and s4.tolist() == [0] * 4
    assert np.array_equal(out[:4], o4) and np.array_equal(grad[:4], g4)
    b = B - 1
    so, sg = ctx.logpos_sta(pars[b], C.HYPER_VEC, prior=True, want_grad=True)
    assert relerr(out[b][1], so[1]) < 1e-10 and relerr(out[b], so) < 1e-9 and vec_relerr(grad[b], sg) < 1e-8


POISON_SNIPPET = r'''
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np
import sta_batch_cases as C
from conftest import relerr, vec_relerr
from nonstationary_multivariate_gaussian_process_amd import _lib
ctx = _lib.Context(0)
n = 0
for (N, M) in C.SHAPES + C.SHAPES[::-1]:
    x, Y, _ = C.subject(N, M)
    ctx.set_data(x, Y)
    pars = C.chains(N, M)
    for prior in (True, False):
        ref, gref = C.oracle(N, M, prior)
        out, grad, st = ctx.sta_batch_eval(pars, C.HYPER_VEC, prior=prior, want_grad=True)
        outv = ctx.sta_batch_eval(pars, C.HYPER_VEC, prior=prior, want_grad=False)[0]
        assert st.tolist() == [0] * C.B_CHAINS and np.all(np.isfinite(out)) and np.all(np.isfinite(grad)), (N, M, st, out, grad)
        assert np.array_equal(out, outv), (N, M)
        ll = ref[:, 1] if prior else -ref[:, 0]
        for b in range(C.B_CHAINS):
            assert relerr(out[b][1], ll[b]) < 1e-8 and vec_relerr(grad[b], gref[b]) < 1e-7, (N, M, prior, b)
        n += 1
ctx.close()
print("POISON_OK", n)
'''


def test_sweep_under_poison():
    """NMGP_POISON=1 (read once per process: a child) fills fresh buffers and every scratch hand-out with NaNs: an element the entry
    reads without having written it -- the seeded band of L^-T, the scratch element above a straddling row pair -- shows up.  The
    sweep forwards and backwards, so that the slab shrinks as well as grows; every result is held to the oracle's bars."""
    env = dict(os.environ)
    env["NMGP_POISON"] = "1"
    env.pop("NMGP_STA_BATCH_MAX", None)
    out = subprocess.run([sys.executable, "-c", POISON_SNIPPET % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}],
                         capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert out.returncode == 0 and "POISON_OK %d" % (4 * len(C.SHAPES)) in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


# ---------------------------------------------------------------------------------------------------
# 3. failure handling
# ---------------------------------------------------------------------------------------------------
def test_a_singular_chain_is_retried_and_its_neighbours_keep_their_bits(ctx):
    N, M = 65, 3
    resident(ctx, (N, M))
    good = np.array(C.chains(N, M))
    bad = good.copy()
    bad[1] = C.singular_chain(good[1])
    out_g, grad_g, st_g = ctx.sta_batch_eval(good, C.HYPER_VEC, prior=True, want_grad=True)
    out, grad, st = ctx.sta_batch_eval(bad, C.HYPER_VEC, prior=True, want_grad=True)
    assert st_g.tolist() == [0, 0, 0, 0]
    assert st[1] < 0 or 1 <= st[1] <= 3, st                             # a retry status or a negative one
    assert [st[0], st[2], st[3]] == [0, 0, 0]
    keep = [0, 2, 3]
    assert np.array_equal(out[keep], out_g[keep]) and np.array_equal(grad[keep], grad_g[keep])
    if st[1] < 0:
        assert np.all(np.isnan(out[1])) and np.all(grad[1] == 0.0)
    else:
        so, sg = ctx.logpos_sta(bad[1], C.HYPER_VEC, prior=True, want_grad=True)     # the retried evaluation itself
        # (sigma2 = 0 leaves NaNs in the inverse-gamma column and in NegLog, in both)
        assert np.array_equal(out[1], so, equal_nan=True) and np.array_equal(grad[1], sg, equal_nan=True)
    # a vector that is not finite: a negative status, a NaN row, a zero gradient row
    nan = good.copy()
    nan[2, 0] = np.nan
    out, grad, st = ctx.sta_batch_eval(nan, C.HYPER_VEC, prior=True, want_grad=True)
    assert st[2] < 0 and np.all(np.isnan(out[2])) and np.all(grad[2] == 0.0)
    assert np.array_equal(out[[0, 1, 3]], out_g[[0, 1, 3]]) and np.array_equal(grad[[0, 1, 3]], grad_g[[0, 1, 3]])


def test_misuse_is_refused_and_the_context_stays_usable(ctx):
    import ctypes
    from nonstationary_multivariate_gaussian_process_amd import _lib
    N, M = 8, 8
    x, Y = resident(ctx, (N, M))
    pars = np.array(C.chains(N, M))
    base = ctx.sta_batch_eval(pars, C.HYPER_VEC, prior=True, want_grad=True)
    with pytest.raises(_lib.NmgpError, match="error -2"):               # NMGP_E_SHAPE: B = 0
        ctx.sta_batch_eval(pars[:0], C.HYPER_VEC)
    out = np.empty((4, 5))
    rc = ctx.lib.nmgp_sta_batch_eval(ctx.h, _lib.ptr(pars), 4, _lib.ptr(C.HYPER_VEC), 1, _lib.ptr(out), None, None)
    assert rc == -1                                                     # NMGP_E_NULL: no status
    with pytest.raises(_lib.NmgpError):                                 # the wrapper's own shape check
        ctx.sta_batch_eval(pars[:, :-1], C.HYPER_VEC)
    ctx.had_set_data(x, np.arange(N) % M, Y[:, 0])
    with pytest.raises(_lib.NmgpError, match="error -3"):               # NMGP_E_STATE: a Hadamard subject is resident
        ctx.sta_batch_eval(pars, C.HYPER_VEC)
    ctx.set_data(x, Y)
    again = ctx.sta_batch_eval(pars, C.HYPER_VEC, prior=True, want_grad=True)
    assert np.array_equal(again[0], base[0]) and np.array_equal(again[1], base[1]) and again[2].tolist() == [0] * 4


# ---------------------------------------------------------------------------------------------------
# 4. the subject set
# ---------------------------------------------------------------------------------------------------
def test_three_subjects_by_two_chains_have_the_resident_paths_bits(ctx, monkeypatch):
    from nonstationary_multivariate_gaussian_process_amd import _lib, sim
    N, M, S, k = 65, 3, 3, 2
    subs = [C.subject(N, M), C.subject(N, M, unsorted=True)]
    d = sim.simulate_stationary(N, M, 4242)
    subs.append((d["x"], d["Y"], d["pars_true"]))
    xs, Ys = np.stack([s[0] for s in subs]), np.stack([s[1] for s in subs])
    pars = np.stack([sim.perturb(subs[s][2], 0.05, 0.3 + 0.2 * j + 0.07 * s) for s in range(S) for j in range(k)])
    ctx.set_data(xs[0], Ys[0])
    ctx.sta_batch_set_subjects(xs, Ys, k)
    out, grad, st = ctx.sta_batch_eval(pars, C.HYPER_VEC, prior=True, want_grad=True)
    assert st.tolist() == [0] * (S * k)
    monkeypatch.setenv("NMGP_STA_BATCH_MAX", "1")                       # a chunk is part of one subject
    split = ctx.sta_batch_eval(pars, C.HYPER_VEC, prior=True, want_grad=True)
    monkeypatch.setenv("NMGP_STA_BATCH_MAX", "5")                       # chunks of whole subjects: 4 + 2 chains
    whole = ctx.sta_batch_eval(pars, C.HYPER_VEC, prior=True, want_grad=True)
    monkeypatch.delenv("NMGP_STA_BATCH_MAX")
    for r in (split, whole):
        assert np.array_equal(r[0], out) and np.array_equal(r[1], grad)
    with pytest.raises(_lib.NmgpError, match="error -2"):               # NMGP_E_SHAPE: B != S * k
        ctx.sta_batch_eval(pars[:5], C.HYPER_VEC)
    # the separable entry sees the same set (one set, two entries)
    with pytest.raises(_lib.NmgpError, match="error -2"):
        ctx.sep_batch_eval(np.zeros((5, 2 * N + M * (M + 1) // 2 + 1)), np.ones(9))
    for s in range(S):
        ctx.set_data(xs[s], Ys[s])                                      # (drops the set: the resident path)
        ro, rg, rs = ctx.sta_batch_eval(pars[s * k:(s + 1) * k], C.HYPER_VEC, prior=True, want_grad=True)
        assert rs.tolist() == [0] * k
        assert np.array_equal(ro, out[s * k:(s + 1) * k]) and np.array_equal(rg, grad[s * k:(s + 1) * k]), s
    # without a set the resident subject is used, whatever B
    assert ctx.sta_batch_eval(pars[:5], C.HYPER_VEC)[2].shape == (5,)


# ---------------------------------------------------------------------------------------------------
# 5. drivers
# ---------------------------------------------------------------------------------------------------
def test_batched_map_stationary_follows_the_reference_trajectory(ctx):
    """map_stationary's bars on the reference's own target_value_hist (tests/golden/map_sep_sta_N64_M3.npz): 1e-7 relative along the
    60 steps, the end point within 1e-3, tilde_sigma untouched; row k of a 3-restart run is the 1-restart run bit for bit."""
    from nonstationary_multivariate_gaussian_process_amd import sim
    from nonstationary_multivariate_gaussian_process_amd.drivers import BatchedMAPStationary
    g = golden("map_sep_sta_N64_M3")
    steps = int(g["steps"])
    h = hyper_dict(g["sta_hyper"], STA_KEYS)
    P0 = np.stack([g["sta_pars0"], sim.perturb(g["sta_pars0"], 0.1, 0.5), sim.perturb(g["sta_pars0"], 0.1, 1.7)])
    pars, hist, alive = BatchedMAPStationary(g["x"], g["Y"], h, P0, ctx=ctx).run(steps)
    assert np.all(alive)
    rel = np.abs(hist[:, 0] - g["sta_hist"]) / np.abs(g["sta_hist"])
    end = np.linalg.norm(pars[0] - g["sta_end"]) / np.linalg.norm(g["sta_end"])
    print("BatchedMAPStationary vs reference trajectory: hist %.3g end %.3g" % (rel.max(), end))
    record_parity("stab_map_N64_M3_vs_reference", hist=(rel.max(), 1e-7), end=(end, 1e-3))
    assert rel.max() < 1e-7, rel.max()
    assert end < 1e-3
    assert np.array_equal(pars[:, 1], P0[:, 1])                         # tilde_sigma is not optimised
    for k in (0, 2):
        p1, h1, a1 = BatchedMAPStationary(g["x"], g["Y"], h, P0[k:k + 1], ctx=ctx).run(steps)
        assert np.array_equal(p1[0], pars[k]) and np.array_equal(h1[:, 0], hist[:, k]), k
    # two subjects x 3 restarts through the subject set: subject 1's rows are the rows above
    xs, Ys = np.stack([g["x"][::-1], g["x"]]), np.stack([g["Y"][::-1] * 1.1, g["Y"]])
    p2, h2, a2 = BatchedMAPStationary(xs, Ys, h, np.concatenate([P0, P0]), ctx=ctx, chains_per_subject=3).run(5)
    assert np.array_equal(h2[:, 3:], hist[:5]) and not np.array_equal(h2[:, :3], hist[:5])
    ctx.sta_batch_clear_subjects()


def test_batched_hmc_stationary_chain_b_is_the_one_chain_run_with_seed_plus_b(ctx):
    from nonstationary_multivariate_gaussian_process_amd.drivers import BatchedHMCStationary
    N, M, iters = 64, 3, 5
    x, Y, _ = C.subject(N, M)
    q0 = np.array(C.chains(N, M, 3))
    P = q0.shape[1]
    A = np.random.default_rng(5).standard_normal((P, P))
    mass = 50.0 * (A @ A.T / P + np.eye(P))
    kw = dict(step_size=5e-3, num_steps_in_leap=5, ctx=ctx, M=mass)
    s3, i3 = BatchedHMCStationary(x, Y, C.HYPER, q0, seed=31, **kw).run(iters)
    assert np.all(np.isfinite(s3)) and not np.array_equal(s3[-1], q0)            # the chains moved
    for b in range(3):
        s1, i1 = BatchedHMCStationary(x, Y, C.HYPER, q0[b:b + 1], seed=31 + b, **kw).run(iters)
        assert np.array_equal(s1[:, 0], s3[:, b]), b
        assert i1["accept_rate"][0] == i3["accept_rate"][b] and np.array_equal(i1["energy_error"][:, 0], i3["energy_error"][:, b])
    print("BatchedHMCStationary accept rates", i3["accept_rate"], "energy errors", np.nanmax(np.abs(i3["energy_error"]), axis=0))


def test_posterior_predict_stationary_summarises_predsample_sta(ctx):
    from nonstationary_multivariate_gaussian_process_amd.drivers import posterior_predict_stationary
    N, M = 64, 3
    x, Y, _ = C.subject(N, M)
    samples = np.array(C.chains(N, M, 6)).reshape(3, 2, -1)            # [iters, chains, T+3]
    xs = np.linspace(0.02, 0.98, 17)
    r = posterior_predict_stationary(x, Y, C.HYPER, samples, xs, seed=3, ctx=ctx)
    assert set(r) == {"mean", "var", "quantiles", "tilde_l_star", "status", "n_used", "n_failed"}      # the separable dict minus the star
    assert r["mean"].shape == (17, M) and r["var"].shape == (17, M) and r["quantiles"].shape == (3, 17, M)
    assert r["n_used"] == 6 and r["n_failed"] == 0 and r["tilde_l_star"].shape == (6, 17)
    assert all(np.all(np.isfinite(r[k])) for k in ("mean", "var", "quantiles")) and np.all(r["var"] > 0)
    assert np.all(r["quantiles"][0] <= r["quantiles"][1]) and np.all(r["quantiles"][1] <= r["quantiles"][2])
    ctx.set_data(x, Y)
    mean, var, st = ctx.predsample_sta(samples.reshape(6, -1), xs)
    assert st.tolist() == [0] * 6 and np.array_equal(r["mean"], mean.mean(axis=0))
    thin = posterior_predict_stationary(x, Y, C.HYPER, samples, xs, draws=3, seed=3, ctx=ctx)
    assert thin["n_used"] == 3
