"""The prior-factor metric and the leapfrog kernels on the GPU (run with -m gpu on an MI355X): k_prior_trmm<TRANS, LAYOUT>,
k_lowrank_proj / _apply, k_metric_kinetic (csrc/nmgp_metric.hip), k_hmc_kick_drift / _drift / _scale / _kinetic / _restore
(csrc/nmgp_kernels.hip) and the host sequences traj_kick_drift, traj_run, nmgp_svc_batch_traj_z (csrc/nmgp_api.hip) against the
np.longdouble references of tests/metric_cases.py, which tests/test_metric_sweep_cpu.py holds the float64 restatements to.

1. Tables A, B, C: both orientations of svc_batch_prior_apply / sep_prior_apply, per block (tilde_l, every slot column of uL, the last
   slot; the four segments), on well-conditioned factors A (tilde_l) and B (uL); exact structure: an input supported on one block gives
   exact zeros in every other, the last slot is copied bit for bit, c32 v for the separable uL_vec, the copy in a batch of 5 and a
   vector's result in a batch of 1 are byte-equal to vector 0's in the batch of 5; every subject's chains against its own factors.
2. Table D, one leapfrog step under the prior metric: the displacement q1 - q0 per block and kin1 against the restatement fed with
   the device's own gradients g0 (at q0) and g1 (at the returned q1).  Two steps once: the restatement's middle point is rounded to
   float64 and its gradient taken from the device (the device itself evaluated a point one rounding away: BAR["D2"]).
3. Flags under the prior metric: a chain whose first evaluated point is undefined (the mode-2 early return of k_prior_trmm), a chain
   whose start is undefined; neighbours to the byte, commit, a second trajectory.
4. Table E: one step under the identity, a diagonal and a dense mass at P = 257 and 513; identity and diagonal also to the byte
   against the float64 host restatement.
5. Items 1 to 3 once more in a child process under NMGP_POISON=1.
The bars are 50 x the float64 restatement's own worst block error per table (metric_cases.BAR), none above 1e-10.  Every achieved
error is recorded (metric_sweep/<table>/<case>/...)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import metric_cases as C
from conftest import ROOT, record_parity

pytestmark = pytest.mark.gpu

HV = C.HV_SVC


@pytest.fixture(scope="module")
def ctx():
    from nonstationary_multivariate_gaussian_process_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------------------
# the measures (also run by the NMGP_POISON child, which imports this module)
# ---------------------------------------------------------------------------------------------------
def hold_blocks(table, tag, got, ref, layout, bad):
    """Every block of every row under BAR[table]; the worst is recorded and named."""
    assert np.all(np.isfinite(got) | np.isnan(np.asarray(ref, dtype=np.float64))), "%s: a non-finite output" % tag
    tab = C.block_table(got, ref, layout)
    worst = max(tab, key=lambda k: tab[k])
    print("metric_sweep/%s/%s: worst block %.3g (row %d: %s), bar %.3g" % ((table, tag, tab[worst]) + worst + (C.BAR[table],)))
    record_parity("metric_sweep/%s/%s" % (table, tag), worst_block=(tab[worst], C.BAR[table]))
    for key, e in tab.items():
        if not e < C.BAR[table]:
            bad.append("%s row %d block %s: %.3g >= %.3g" % ((tag,) + key + (e, C.BAR[table])))


def hold_structure(tag, apply, layout, bad):
    """An input supported on one block: exact zeros in every other block, both orientations."""
    lay, N, M = layout
    e, pick = C.unit_block_inputs(lay, N, M)
    bl = C.blocks(lay, N, M)
    for trans in (False, True):
        out = apply(e, trans)
        for row, k in enumerate(pick):
            other = np.ones(out.shape[1], dtype=bool)
            other[bl[k][1]] = False
            if np.any(out[row, other] != 0) or not np.any(out[row, bl[k][1]] != 0):
                bad.append("%s trans=%d: an input on block %s leaks into another block (or gives nothing)" % (tag, trans, bl[k][0]))


def run_table_a(ctx, case):
    N, M = case
    x, Y = C.data(N, M)
    L0, L1 = C.factors(N)
    bad, res = [], {}
    ctx.set_data(x, Y)
    for B in C.BATCHES_A:
        ctx.svc_batch_alloc(B)
        v = C.vectors("svc", N, M, B)
        for trans in (False, True):
            got = ctx.svc_batch_prior_apply(HV, v, trans=trans)
            hold_blocks("A", "%s/batch%d/trans%d" % (C.case_id(case), B, trans), got, C.apply_svc(L0, L1, v, trans), ("svc", N, M), bad)
            if not same_bytes(got[:, -1], v[:, -1]):
                bad.append("batch %d trans=%d: the last slot is not copied bit for bit" % (B, trans))
            res[B, trans] = got
    for trans in (False, True):
        if not same_bytes(res[5, trans][4], res[5, trans][0]):
            bad.append("trans=%d: the copy of vector 0 in the batch of 5 differs from vector 0's result" % trans)
        if not same_bytes(res[1, trans][0], res[5, trans][0]):
            bad.append("trans=%d: vector 0 alone differs from vector 0 in the batch of 5" % trans)
    e, _ = C.unit_block_inputs("svc", N, M)

    def apply(e, trans):
        buf = np.zeros((5, e.shape[1]))
        buf[:e.shape[0]] = e
        return ctx.svc_batch_prior_apply(HV, buf, trans=trans)[:e.shape[0]]
    hold_structure(C.case_id(case), apply, ("svc", N, M), bad)
    assert not bad, "table A %s:\n  " % C.case_id(case) + "\n  ".join(bad)


def run_table_b(ctx, case):
    N, M = case
    S, k = C.SUBJECTS, C.CHAINS_PER_SUBJECT
    xs = np.stack([C.data(N, M, s)[0] for s in range(S)])
    Ys = np.stack([C.data(N, M, s)[1] for s in range(S)])
    ctx.set_data(xs[1], Ys[1])                          # the resident subject, which the set overrides, is not subject 0
    ctx.svc_batch_alloc(S * k)
    ctx.svc_batch_set_subjects(xs, Ys, k)
    v = C.subject_vectors(N, M)
    bad = []
    for trans in (False, True):
        got = ctx.svc_batch_prior_apply(HV, v, trans=trans)
        for s in range(S):
            rows = slice(s * k, (s + 1) * k)
            hold_blocks("B", "%s/subject%d/trans%d" % (C.case_id(case), s, trans), got[rows],
                        C.apply_svc(*C.factors(N, s), v[rows], trans), ("svc", N, M), bad)
        # subject 2 has subject 0's vectors in the other order: different factors, different results
        if same_bytes(got[4], got[1]) or same_bytes(got[5], got[0]):
            bad.append("trans=%d: subject 2 answers with subject 0's factors" % trans)
    assert not bad, "table B %s:\n  " % C.case_id(case) + "\n  ".join(bad)


def run_table_c(ctx, case):
    N, M, B = case
    T = C.n_slots(M)
    x, Y = C.data(N, M)
    L0, L1 = C.factors(N)
    ctx.set_data(x, Y)
    v = C.vectors("sep", N, M, B)
    bad = []
    for c in C.SEP_C:
        hv = np.concatenate([HV, [c]])
        c32 = float(np.float32(c))
        for trans in (False, True):
            got = ctx.sep_prior_apply(hv, v, trans=trans)
            hold_blocks("C", "%s/c%g/trans%d" % (C.case_id(case), c, trans), got, C.apply_sep(L0, L1, c, v, trans), ("sep", N, M), bad)
            if not same_bytes(got[:, 2 * N:2 * N + T], c32 * v[:, 2 * N:2 * N + T]):
                bad.append("c=%r trans=%d: the uL_vec block is not c32 v" % (c, trans))
            if not same_bytes(got[:, -1], v[:, -1]):
                bad.append("c=%r trans=%d: the last slot is not copied bit for bit" % (c, trans))
            if not same_bytes(ctx.sep_prior_apply(hv, v[:1], trans=trans)[0], got[0]):
                bad.append("c=%r trans=%d: vector 0 alone differs from vector 0 in the batch of %d" % (c, trans, B))
    hv = np.concatenate([HV, [C.SEP_C[1]]])
    hold_structure(C.case_id(case), lambda e, trans: ctx.sep_prior_apply(hv, e, trans=trans), ("sep", N, M), bad)
    assert not bad, "table C %s:\n  " % C.case_id(case) + "\n  ".join(bad)


# ---------------------------------------------------------------------------------------------------
# trajectories
# ---------------------------------------------------------------------------------------------------
def evaluate(ctx, q, defined=None):
    """(U [B], gradient [B, P]) of the batch at q; `defined`: the chains whose evaluation must be defined (all)."""
    ctx.svc_batch_set_pars(q)
    ctx.svc_batch_eval(HV, C.PRIOR, want_grad=True)
    out, st = ctx.svc_batch_fetch()
    g = ctx.svc_batch_fetch_grad()
    ok = np.ones(q.shape[0], dtype=bool) if defined is None else np.asarray(defined, dtype=bool)
    assert np.all(st[ok] == 0) and np.all(np.isfinite(out[ok])) and np.all(np.isfinite(g[ok])), (st, out)
    return out[:, 0].copy(), g


def prior_start(ctx, case, q0, defined=None):
    """Evaluate at q0, set the metric, begin: the state a trajectory starts from.  Returns (U0, g0)."""
    N, M, r, B = case
    _, _, U, lam = C.traj_inputs(N, M, r, B)
    U0, g0 = evaluate(ctx, q0, defined)
    if r > 0:
        ctx.svc_batch_traj_set_mass_prior(HV, U, lam)
    else:
        ctx.svc_batch_traj_set_mass_prior(HV)
    ctx.svc_batch_traj_begin()
    return U0, g0


def setup_case(ctx, case):
    N, M, r, B = case
    x, Y = C.data(N, M)
    ctx.set_data(x, Y)
    ctx.svc_batch_alloc(B)
    return C.traj_inputs(N, M, r, B)


def hold_traj(table, tag, q0, q1, kin1, ref_points, ref_kin, layout, bad, rows=None):
    rows = list(range(q0.shape[0])) if rows is None else rows
    got = (np.asarray(q1, dtype=C.LD) - np.asarray(q0, dtype=C.LD))[rows]
    hold_blocks(table, tag + "/displacement", got, C.displacement(ref_points)[rows], layout, bad)
    ek = C.scalar_error(np.asarray(kin1)[rows], np.asarray(ref_kin)[rows])
    print("metric_sweep/%s/%s: kinetic energy %.3g, bar %.3g" % (table, tag, ek, C.BAR[table]))
    record_parity("metric_sweep/%s/%s" % (table, tag), kinetic=(ek, C.BAR[table]))
    if not ek < C.BAR[table]:
        bad.append("%s: kinetic energy %.3g >= %.3g (%r, restatement %r)" % (tag, ek, C.BAR[table], kin1, np.asarray(ref_kin, dtype=np.float64)))


def run_table_d(ctx, case, nsteps=1):
    N, M, r, B = case
    q0, z, U, lam = setup_case(ctx, case)
    ok = np.zeros(B, dtype=bool)
    U0, g0 = prior_start(ctx, case, q0)
    q1, kin1, U1, failed = ctx.svc_batch_traj_z(HV, C.PRIOR, C.EPS, nsteps, z)
    assert not failed.any() and np.all(np.isfinite(U1)) and np.all(np.isfinite(q1)) and np.all(np.isfinite(kin1))
    _, g_end = evaluate(ctx, q1)                         # the gradient of the closing half kick

    def grad_at(k, q):
        if k == nsteps:
            return g_end, ok
        return evaluate(ctx, np.asarray(q, dtype=np.float64))[1], ok     # the restatement's middle point, rounded
    points, kin = C.leapfrog_prior(q0, z, C.EPS, nsteps, U, lam, *C.factors(N), g0, ok, grad_at)
    bad = []
    table = "D" if nsteps == 1 else "D2"
    hold_traj(table, "%s/steps%d" % (C.case_id(case), nsteps), q0, q1, kin1, points, kin, ("svc", N, M), bad)
    if not np.abs(q1 - q0).max() > 1e-8:
        bad.append("the chains did not move")
    assert not bad, "table %s %s:\n  " % (table, C.case_id(case)) + "\n  ".join(bad)


def run_flags_mid_trajectory(ctx):
    """Chain 1's z scaled so that exp(tilde_l) overflows at its first evaluated point (a status flag: every buffer stays inside its
    allocation), two steps: both kicks after the start are skipped for it, both drifts are not."""
    case = C.FLAG_CASE
    N, M, r, B = case
    q0, z, U, lam = setup_case(ctx, case)
    zbig = C.overflow_z(z)
    flag = np.array([False, True, False])
    # the ordinary run
    prior_start(ctx, case, q0)
    qa, ka, Ua, fa = ctx.svc_batch_traj_z(HV, C.PRIOR, C.EPS, 2, z)
    assert not fa.any()
    # chain 1 out of the domain
    U0, g0 = prior_start(ctx, case, q0)
    qb, kb, Ub, fb = ctx.svc_batch_traj_z(HV, C.PRIOR, C.EPS, 2, zbig)
    bad = []
    if fb.tolist() != [False, True, False] or Ub[1] != np.inf or not np.all(np.isfinite(Ub[[0, 2]])):
        bad.append("failed %r, U1 %r: chain 1 alone must be flagged, with U1 = inf" % (fb, Ub))
    nan = np.full_like(q0, np.nan)
    points, kin = C.leapfrog_prior(q0, zbig, C.EPS, 2, U, lam, *C.factors(N), g0, np.zeros(B, dtype=bool),
                                   lambda k, q: (nan, np.ones(B, dtype=bool)))
    # (the restatement is asked for chain 1 alone: its kicks after the start are skipped, whatever the gradient)
    hold_traj("D", "flags/overflow", q0, qb, kb, points, kin, ("svc", N, M), bad, rows=[1])
    for b in (0, 2):
        if not (same_bytes(qb[b], qa[b]) and kb[b] == ka[b] and Ub[b] == Ua[b]):
            bad.append("chain %d changes with its neighbour's z" % b)
    ctx.svc_batch_traj_commit(np.array([1, 0, 1]))
    now = ctx.svc_batch_get_pars()
    if not (same_bytes(now[1], q0[1]) and same_bytes(now[0], qb[0]) and same_bytes(now[2], qb[2])):
        bad.append("commit([1, 0, 1]) does not put chain 1's q0 back to the byte (or moves an accepted chain)")
    # a second trajectory from there: chain 1 got its gradient and its flag back too
    qc, kc, Uc, fc = ctx.svc_batch_traj_z(HV, C.PRIOR, C.EPS, 1, z)
    prior_start(ctx, case, q0)
    qd, kd, Ud, fd = ctx.svc_batch_traj_z(HV, C.PRIOR, C.EPS, 1, z)
    if fc[1] or fd.any() or not (same_bytes(qc[1], qd[1]) and kc[1] == kd[1] and Uc[1] == Ud[1]):
        bad.append("chain 1's second trajectory differs from one from a fresh start: %r %r, %r %r" % (kc[1], kd[1], Uc[1], Ud[1]))
    assert not bad, "flags, mid-trajectory:\n  " + "\n  ".join(bad)


def run_flags_undefined_start(ctx):
    """Chain 1 starts at a NaN: its kick is skipped, its drift is not (the NaN stays where it is), it is flagged, and a commit of the
    chains that did not fail leaves it where it started; its neighbours never notice."""
    case = C.FLAG_CASE
    N, M, r, B = case
    q0, z, U, lam = setup_case(ctx, case)
    qn = C.nan_start(q0)
    flag = np.array([False, True, False])
    prior_start(ctx, case, q0)
    qa, ka, Ua, fa = ctx.svc_batch_traj_z(HV, C.PRIOR, C.EPS, 1, z)
    U0, g0 = prior_start(ctx, case, qn, defined=~flag)
    qb, kb, Ub, fb = ctx.svc_batch_traj_z(HV, C.PRIOR, C.EPS, 1, z)
    bad = []
    if fa.any() or fb.tolist() != [False, True, False] or Ub[1] != np.inf:
        bad.append("failed %r / %r, U1 %r" % (fa, fb, Ub))
    nan = np.full_like(q0, np.nan)
    points, kin = C.leapfrog_prior(qn, z, C.EPS, 1, U, lam, *C.factors(N), np.where(flag[:, None], np.nan, g0), flag,
                                   lambda k, q: (nan, np.ones(B, dtype=bool)))
    hold_traj("D", "flags/nan_start", qn, qb, kb, points, kin, ("svc", N, M), bad, rows=[1])
    for b in (0, 2):
        if not (same_bytes(qb[b], qa[b]) and kb[b] == ka[b] and Ub[b] == Ua[b]):
            bad.append("chain %d changes with its neighbour's start" % b)
    ctx.svc_batch_traj_commit(~fb)
    now = ctx.svc_batch_get_pars()
    if not (same_bytes(now[1], qn[1]) and same_bytes(now[0], qb[0]) and same_bytes(now[2], qb[2])):
        bad.append("the chain with the undefined start moved")
    qc, kc, Uc, fc = ctx.svc_batch_traj_z(HV, C.PRIOR, C.EPS, 1, z)
    ctx.svc_batch_traj_commit(~fc)
    if fc.tolist() != [False, True, False] or not same_bytes(ctx.svc_batch_get_pars()[1], qn[1]):
        bad.append("the chain with the undefined start moved in its second trajectory (failed %r)" % fc)
    assert not bad, "flags, undefined start:\n  " + "\n  ".join(bad)


def run_table_e(ctx, case, kind):
    N, M, B = case
    x, Y = C.data(N, M)
    ctx.set_data(x, Y)
    ctx.svc_batch_alloc(B)
    q0, z = C.mass_inputs(N, M, B)[:2]
    minv, mchol = C.mass_pair(kind, N, M, B)
    ok = np.zeros(B, dtype=bool)
    U0, g0 = evaluate(ctx, q0)
    ctx.svc_batch_traj_set_mass(minv)
    if kind != "identity":
        ctx.svc_batch_traj_set_mass_chol(mchol)
    ctx.svc_batch_traj_begin()
    q1, kin1, U1, failed = ctx.svc_batch_traj_z(HV, C.PRIOR, C.EPS, 1, z)
    assert not failed.any() and np.all(np.isfinite(U1))
    _, g1 = evaluate(ctx, q1)
    ctx.svc_batch_traj_set_mass(None)
    bad = []
    points, kin, _, _ = C.leapfrog_mass(kind, q0, z, C.EPS, 1, minv, mchol, g0, ok, lambda k, q: (g1, ok), C.LD)
    hold_traj("E", "%s/%s" % (C.case_id(case), kind), q0, q1, kin1, points, kin, ("svc", N, M), bad)
    if kind != "dense":
        # operation for operation the host's float64 arithmetic: the same bits
        pf, kf, p1, v1 = C.leapfrog_mass(kind, q0, z, C.EPS, 1, minv, mchol, g0, ok, lambda k, q: (g1, ok), np.float64)
        if not same_bytes(q1, pf[1]):
            bad.append("q1 is not the float64 host restatement's to the byte (%d entries differ)" % np.count_nonzero(q1 != pf[1]))
        kbits = np.array([C.kinetic_bits(p1[b], minv) for b in range(B)])
        if not same_bytes(kin1, kbits):
            bad.append("kin1 %r is not the float64 host restatement's %r to the byte" % (kin1, kbits))
    assert not bad, "table E %s %s:\n  " % (C.case_id(case), kind) + "\n  ".join(bad)


# ---------------------------------------------------------------------------------------------------
# the tests
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.TABLE_A, ids=C.case_id)
def test_table_a_prior_apply(ctx, case):
    run_table_a(ctx, case)


@pytest.mark.parametrize("case", C.TABLE_B, ids=C.case_id)
def test_table_b_prior_apply_of_a_subject_set(ctx, case):
    run_table_b(ctx, case)


@pytest.mark.parametrize("case", C.TABLE_C, ids=C.case_id)
def test_table_c_separable_prior_apply(ctx, case):
    run_table_c(ctx, case)


@pytest.mark.parametrize("case", C.TABLE_D, ids=C.case_id)
def test_table_d_one_step_under_the_prior_metric(ctx, case):
    run_table_d(ctx, case, 1)


@pytest.mark.parametrize("case", C.TABLE_D2, ids=C.case_id)
def test_table_d_two_steps_under_the_prior_metric(ctx, case):
    run_table_d(ctx, case, 2)


def test_flags_chain_undefined_in_mid_trajectory_under_the_prior_metric(ctx):
    run_flags_mid_trajectory(ctx)


def test_flags_chain_with_an_undefined_start_under_the_prior_metric(ctx):
    run_flags_undefined_start(ctx)


@pytest.mark.parametrize("kind", C.MASS_KINDS)
@pytest.mark.parametrize("case", C.TABLE_E, ids=C.case_id)
def test_table_e_one_step_under_identity_diagonal_and_dense_mass(ctx, case, kind):
    run_table_e(ctx, case, kind)


# ---------------------------------------------------------------------------------------------------
# once more with every fresh buffer and scratch hand-out full of NaNs
# ---------------------------------------------------------------------------------------------------
def poison_order():
    """Items 1 to 3, ordered so that P and the batch first grow and then shrink."""
    size = lambda c: C.n_pars("svc", c[0], c[1])
    a = sorted(C.TABLE_A, key=size)
    return ([("a", c) for c in a] + [("d", c) for c in sorted(C.TABLE_D, key=size, reverse=True)] + [("d2", c) for c in C.TABLE_D2]
            + [("b", c) for c in C.TABLE_B] + [("c", c) for c in sorted(C.TABLE_C, key=lambda c: c[0], reverse=True)]
            + [("flags", None)])


def run_poison_sequence(ctx):
    n = 0
    for what, case in poison_order():
        if what == "flags":
            run_flags_mid_trajectory(ctx)
            run_flags_undefined_start(ctx)
        else:
            {"a": run_table_a, "b": run_table_b, "c": run_table_c, "d": run_table_d,
             "d2": lambda ctx, case: run_table_d(ctx, case, 2)}[what](ctx, case)
        n += 1
    return n


POISON_SNIPPET = r'''
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import metric_cases as C
import test_gpu_metric_sweep as t
from nonstationary_multivariate_gaussian_process_amd import _lib
C.load_factors(%(factors)r)
ctx = _lib.Context(0)
n = t.run_poison_sequence(ctx)
ctx.close()
print("POISON_OK", n)
'''


def test_metric_sweep_under_poison(tmp_path):
    """NMGP_POISON=1 (read once per process: a child) fills fresh buffers and every scratch hand-out with NaNs: the strict upper
    triangle of a cached factor and its padding rows up to ld are then NaN, and no NaN may reach an output.  Items 1 to 3 at the same
    bars; the longdouble factors go to the child in a file, so that they are computed once."""
    for N in sorted({c[0] for c in C.TABLE_A + C.TABLE_C + C.TABLE_D}):
        C.factors(N)
    for N, M in C.TABLE_B:
        for s in range(C.SUBJECTS):
            C.factors(N, s)
    path = str(tmp_path / "factors.npz")
    C.save_factors(path)
    env = dict(os.environ)
    env["NMGP_POISON"] = "1"
    out = subprocess.run([sys.executable, "-c", POISON_SNIPPET % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "factors": path}],
                         capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0 and "POISON_OK %d" % len(poison_order()) in out.stdout, out.stdout[-4000:] + out.stderr[-4000:]
