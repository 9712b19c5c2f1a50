"""CPU half of the prior-factor metric and leapfrog sweep (no GPU; cases, references and measure: tests/metric_cases.py, GPU half:
tests/test_gpu_metric_sweep.py).

1. The float64 restatements (oracle.RBF_cov -> np.linalg.cholesky -> block products; the leapfrog steps in float64) against the
   np.longdouble references at every case of tables A to E; the trajectory cases with the oracle's gradients
   (nlogpos_obj_SVC(..., grad=True)) fed to both.  The worst block error per table is printed (test_report_...) and must not
   exceed its entry of metric_cases.RESTATEMENT_WORST, whose 50-fold is the GPU half's bar; no bar may exceed 1e-10.
2. The conditions the factor family rests on, asserted: kappa(A) <= 200, kappa(B) <= 2000 at every N of the tables; every whole
   64 x 64 tile of the lower triangle of A, and every whole lower tile of B within two tiles of the diagonal, holds an entry >= 1 %
   of the factor's largest.  The ragged last row of tiles (one row at N = 65, 129, 193, 257) is held to 0.5 %: measured, the
   1 x 64 corner of A at N = 257 holds 0.91 % (every other tile of A >= 1.8 %), still five orders above what a rejection needs.
   B's corner tile is below 1 % at N >= 193 (0.27 % and 0.06 %; tiles (3, 0) and (4, 1) at N = 257 hold 2 %): the far tiles are
   A's job.  Every block of every test vector is non-zero.
3. Every mutation of the restatements is rejected -- a block error >= 100 x the bar -- at every case of the tables where it can act.
   For mutation 3 at M = 8 the whole-vector norm on the ill-conditioned hyper-parameters of tests/test_hmc_metric.py is printed next
   to its 1e-5 bar."""
import numpy as np
import pytest

import metric_cases as C

WORST = {}                                     # table -> (error, where), filled by the restatement tests, printed by the last test
ALL_N = sorted({c[0] for c in C.TABLE_A + C.TABLE_B + C.TABLE_C + C.TABLE_D + C.TABLE_E})


def _note(table, err, where):
    if err >= WORST.get(table, (-1.0, ""))[0]:
        WORST[table] = (err, where)
    assert err <= C.RESTATEMENT_WORST[table], (table, where, err, C.RESTATEMENT_WORST[table])


# ---------------------------------------------------------------------------------------------------
# 2. the family
# ---------------------------------------------------------------------------------------------------
def test_the_factor_family_is_well_conditioned_and_populated_far_from_the_diagonal():
    for N in ALL_N:
        for which in "AB":
            for s in range(C.SUBJECTS if N == 65 else 1):
                L = np.asarray(C.factor(which, N, s, "ld"), dtype=np.float64)
                kappa = np.linalg.cond(L) ** 2
                assert kappa <= C.KAPPA_MAX[which], (which, N, s, kappa)
                big = np.abs(L).max()
                nt = (N + C.TILE - 1) // C.TILE
                for it in range(nt):
                    for kt in range(it + 1):
                        m = np.abs(L[it * C.TILE:(it + 1) * C.TILE, kt * C.TILE:(kt + 1) * C.TILE]).max()
                        whole = (it + 1) * C.TILE <= N
                        if which == "A" or it - kt <= 2:
                            assert m >= (0.01 if whole else 0.005) * big, (which, N, it, kt, m / big)
                        elif it == nt - 1 and kt == 0 and N >= 193:
                            assert m < 0.01 * big, (which, N, it, kt, m / big)


def test_the_float64_factor_is_close_to_the_longdouble_one():
    worst = 0.0
    for N in ALL_N:
        for which in "AB":
            Lr, Lf = C.factor(which, N, 0, "ld"), C.factor(which, N, 0, "f64")
            worst = max(worst, float(np.abs(Lf - Lr).max() / np.abs(Lr).max()))
    print("float64 factor against longdouble, relative max-norm: %.3g" % worst)
    assert worst < 1e-13


def test_every_block_of_every_test_vector_is_non_zero():
    for (N, M) in C.TABLE_A + C.TABLE_B:
        v = C.vectors("svc", N, M, 5 if (N, M) in C.TABLE_A else 4)
        for name, sl in C.blocks("svc", N, M):
            assert np.all(np.abs(v[:, sl]).max(axis=1) > 0), (N, M, name)
    for (N, M, B) in C.TABLE_C:
        v = C.vectors("sep", N, M, B)
        for name, sl in C.blocks("sep", N, M):
            assert np.all(np.abs(v[:, sl]).max(axis=1) > 0), (N, M, name)
    assert np.array_equal(C.vectors("svc", 65, 3, 5)[4], C.vectors("svc", 65, 3, 5)[0])
    assert np.array_equal(C.vectors("svc", 65, 3, 1)[0], C.vectors("svc", 65, 3, 5)[0])


def test_no_bar_exceeds_the_cap():
    for k, bar in C.BAR.items():
        assert bar <= C.BAR_CAP, (k, bar)


# ---------------------------------------------------------------------------------------------------
# 1. the restatements: tables A, B, C
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.TABLE_A, ids=C.case_id)
def test_table_a_restatement(case):
    N, M = case
    v = C.vectors("svc", N, M, 5)
    for trans in (False, True):
        got = C.apply_svc(*C.factors(N, 0, "f64"), v, trans)
        ref = C.apply_svc(*C.factors(N, 0, "ld"), v, trans)
        err, where = C.block_errors(got, ref, ("svc", N, M))
        _note("A", err, "%s trans=%d %s" % (C.case_id(case), trans, where))


@pytest.mark.parametrize("case", C.TABLE_B, ids=C.case_id)
def test_table_b_restatement(case):
    N, M = case
    k = C.CHAINS_PER_SUBJECT
    for s in range(C.SUBJECTS):
        v = C.subject_vectors(N, M)[s * k:(s + 1) * k]
        for trans in (False, True):
            got = C.apply_svc(*C.factors(N, s, "f64"), v, trans)
            ref = C.apply_svc(*C.factors(N, s, "ld"), v, trans)
            err, where = C.block_errors(got, ref, ("svc", N, M))
            _note("B", err, "%s subject %d trans=%d %s" % (C.case_id(case), s, trans, where))
    # the subjects' factors really differ
    assert np.abs(C.factor("B", N, 2, "f64") - C.factor("B", N, 0, "f64")).max() > 1e-3 * np.abs(C.factor("B", N, 0, "f64")).max()


@pytest.mark.parametrize("case", C.TABLE_C, ids=C.case_id)
def test_table_c_restatement(case):
    N, M, B = case
    v = C.vectors("sep", N, M, B)
    for c in C.SEP_C:
        for trans in (False, True):
            got = C.apply_sep(*C.factors(N, 0, "f64"), c, v, trans)
            ref = C.apply_sep(*C.factors(N, 0, "ld"), c, v, trans)
            err, where = C.block_errors(got, ref, ("sep", N, M))
            _note("C", err, "%s c=%r trans=%d %s" % (C.case_id(case), c, trans, where))
    assert float(np.float32(C.SEP_C[1])) != C.SEP_C[1] and float(np.float32(C.SEP_C[0])) == C.SEP_C[0]


# ---------------------------------------------------------------------------------------------------
# 1. the restatements: trajectories
# ---------------------------------------------------------------------------------------------------
_GRAD = {}


def oracle_grads(N, M, q, bad):
    """(g [B, P], bad [B]) of the float64 oracle at the rows of q; rows flagged bad are not evaluated: NaN."""
    from oracle import nmgp_oracle as O
    x, Y = C.data(N, M)
    hyper = dict(zip(["mu_tilde_l", "alpha_tilde_l", "beta_tilde_l", "mu_L", "alpha_L", "beta_L", "a", "b"], C.HV_SVC))
    out = np.full(q.shape, np.nan)
    for b in range(q.shape[0]):
        if bad[b]:
            continue
        key = (N, M, q[b].tobytes())
        if key not in _GRAD:
            _GRAD[key] = O.nlogpos_obj_SVC(q[b], Y, x, **hyper, verbose=True, Prior=C.PRIOR, grad=True)[1]
        out[b] = _GRAD[key]
    assert np.all(np.isfinite(out[~np.asarray(bad, dtype=bool)]))
    return out, np.asarray(bad, dtype=bool)


def prior_run(case, nsteps, prec, grads, q0=None, z=None, bads=None, mutation=None, shift=None):
    """The restatement in `prec` with the oracle's gradients.  grads: None (evaluate the oracle at the float64 points and return them)
    or the list of an earlier run.  bads[k]: flags at point k (all defined by default).  shift: seed of a one-ulp change of the
    middle point before its gradient is taken."""
    N, M, r, B = case
    q0_, z_, U, lam = C.traj_inputs(N, M, r, B)
    q0, z = (q0_ if q0 is None else q0), (z_ if z is None else z)
    bads = [np.zeros(B, dtype=bool)] * (nsteps + 1) if bads is None else bads
    L0, L1 = C.factors(N, 0, prec)
    taken = [] if grads is None else None

    def grad_at(k, q):
        if grads is not None:
            return grads[k], bads[k]
        qq = np.asarray(q, dtype=np.float64)
        if shift is not None and k < nsteps:
            qq = C.ulp_shift(qq, shift)
        taken.append(oracle_grads(N, M, qq, bads[k])[0])
        return taken[-1], bads[k]
    if grads is None:
        taken.append(oracle_grads(N, M, np.where(np.isnan(q0), 0.0, q0), bads[0])[0])
    g0 = taken[0] if grads is None else grads[0]
    points, kin = C.leapfrog_prior(q0, z, C.EPS, nsteps, U, lam, L0, L1, g0, bads[0], grad_at, mutation)
    return points, kin, (taken if grads is None else grads)


def traj_error(got, ref, layout, rows=None):
    """max of the worst displacement block and the kinetic energy's error; (error, where)."""
    (pg, kg), (pr, kr) = got, ref
    rows = slice(None) if rows is None else rows
    err, where = C.block_errors(C.displacement(pg)[rows], C.displacement(pr)[rows], layout)
    ek = C.scalar_error(np.asarray(kg)[rows], np.asarray(kr)[rows])
    return (err, "displacement " + where) if err >= ek else (ek, "kinetic energy")


@pytest.mark.parametrize("case", C.TABLE_D, ids=C.case_id)
def test_table_d_restatement_one_step(case):
    N, M, r, B = case
    pf, kf, grads = prior_run(case, 1, "f64", None)
    pr, kr, _ = prior_run(case, 1, "ld", grads)
    err, where = traj_error((pf, kf), (pr, kr), ("svc", N, M))
    _note("D", err, "%s %s" % (C.case_id(case), where))
    lam = C.traj_inputs(N, M, r, B)[3]
    assert r < 2 or (lam[r // 2] == 0.0 and np.count_nonzero(lam) == r - 1 and lam[lam > 0].min() >= 0.5 and lam.max() <= 1e4)
    assert np.abs(C.displacement(pf)).max() > 1e-8                        # the chains went somewhere


@pytest.mark.parametrize("case", C.TABLE_D2, ids=C.case_id)
def test_table_d_restatement_two_steps_and_its_sensitivity_to_the_middle_point(case):
    N, M, r, B = case
    pf, kf, grads = prior_run(case, 2, "f64", None)
    pr, kr, _ = prior_run(case, 2, "ld", grads)
    err, where = traj_error((pf, kf), (pr, kr), ("svc", N, M))
    # the device evaluates a middle point one rounding away from the restatement's: what a one-ulp change of it does
    sens = 0.0
    for seed in (1, 2):
        ps, ks, _ = prior_run(case, 2, "f64", None, shift=seed)
        sens = max(sens, traj_error((ps, ks), (pf, kf), ("svc", N, M))[0])
    print("table D, two steps, %s: restatement %.3g, one-ulp sensitivity %.3g" % (C.case_id(case), err, sens))
    assert sens <= C.ONE_ULP_SENSITIVITY
    _note("D2", err + sens, "%s %s (+ sensitivity %.3g)" % (C.case_id(case), where, sens))


def _flag_scenarios():
    """(name, nsteps, q0, z, bads): chain 1 undefined from the start (NaN in q0) / from the first evaluated point on (z scaled)."""
    N, M, r, B = C.FLAG_CASE
    q0, z = C.traj_inputs(N, M, r, B)[:2]
    flag = np.array([False, True, False])
    return [("nan_start", 1, C.nan_start(q0), z, [flag, flag]),
            ("overflow", 2, q0, C.overflow_z(z), [np.zeros(3, dtype=bool), flag, flag])]


def test_flag_scenarios_restatement():
    N, M, r, B = C.FLAG_CASE
    for name, nsteps, q0, z, bads in _flag_scenarios():
        pf, kf, grads = prior_run(C.FLAG_CASE, nsteps, "f64", None, q0, z, bads)
        pr, kr, _ = prior_run(C.FLAG_CASE, nsteps, "ld", grads, q0, z, bads)
        err, where = traj_error((pf, kf), (pr, kr), ("svc", N, M))
        _note("D", err, "flags/%s %s" % (name, where))
        if name == "overflow":
            # exp(tilde_l) overflows at both evaluated points of chain 1: the scenario's flags are what the device must find
            assert all(np.abs(np.asarray(p, dtype=np.float64)[1, :N]).max() > 1000.0 for p in pf[1:])
        else:
            assert np.isnan(pf[1][1, 0]) and np.count_nonzero(np.isnan(pf[1])) == 1


@pytest.mark.parametrize("kind", C.MASS_KINDS)
@pytest.mark.parametrize("case", C.TABLE_E, ids=C.case_id)
def test_table_e_restatement(case, kind):
    N, M, B = case
    q0, z = C.mass_inputs(N, M, B)[:2]
    minv, mchol = C.mass_pair(kind, N, M, B)
    ok = np.zeros(B, dtype=bool)
    g0 = oracle_grads(N, M, q0, ok)[0]
    taken = []

    def grad_f64(k, q):
        taken.append(oracle_grads(N, M, np.asarray(q, dtype=np.float64), ok)[0])
        return taken[-1], ok
    pf, kf, p1, v1 = C.leapfrog_mass(kind, q0, z, C.EPS, 1, minv, mchol, g0, ok, grad_f64, np.float64)
    pr, kr, _, _ = C.leapfrog_mass(kind, q0, z, C.EPS, 1, minv, mchol, g0, ok, lambda k, q: (taken[0], ok), C.LD)
    err, where = traj_error((pf, kf), (pr, kr), ("svc", N, M))
    _note("E", err, "%s %s %s" % (C.case_id(case), kind, where))
    assert C.n_pars("svc", N, M) % 256 == 1
    if kind != "dense":
        # the kernel's summation order, to the bit, is a restatement of the same sum
        kb = np.array([C.kinetic_bits(p1[b], minv) for b in range(B)])
        assert C.scalar_error(kb, kr) <= C.RESTATEMENT_WORST["E"]


# ---------------------------------------------------------------------------------------------------
# 3. the mutations
# ---------------------------------------------------------------------------------------------------
def _rejected(err, table):
    return err >= C.REJECT * C.BAR[table]


@pytest.mark.parametrize("name", sorted(C.SVC_MUTATIONS))
def test_product_mutations_are_rejected_wherever_they_act(name):
    acted = 0
    for table, cases in (("A", C.TABLE_A), ("B", C.TABLE_B)):
        for (N, M) in cases:
            v = C.vectors("svc", N, M, 5 if table == "A" else 4)
            for trans in (False, True):
                if not C.svc_mutation_acts(name, N, M, trans):
                    continue
                for s in range(C.SUBJECTS if table == "B" else 1):
                    ref = C.apply_svc(*C.factors(N, s, "ld"), v, trans)
                    err, where = C.block_errors(C.SVC_MUTATIONS[name](*C.factors(N, s, "f64"), v, trans), ref, ("svc", N, M))
                    assert _rejected(err, table), (name, N, M, trans, s, err, where)
                    acted += 1
    assert acted >= {"skip_factor_tile": 4, "stop_one_tile_early": 13, "last_group_full": 20, "swap_factors": 26}[name], acted


def test_separable_mutations_are_rejected():
    for (N, M, B) in C.TABLE_C:
        v = C.vectors("sep", N, M, B)
        for c in C.SEP_C:
            for trans in (False, True):
                ref = C.apply_sep(*C.factors(N, 0, "ld"), c, v, trans)
                for mut in (C.mut_sep_swap_factors, C.mut_sep_unscaled):
                    err, where = C.block_errors(mut(*C.factors(N, 0, "f64"), c, v, trans), ref, ("sep", N, M))
                    assert _rejected(err, "C"), (mut.__name__, N, M, c, trans, err, where)


def test_trajectory_mutations_are_rejected_wherever_they_act():
    acted = {m: 0 for m in C.TRAJ_MUTATIONS}
    for case in C.TABLE_D:
        N, M, r, B = case
        pf, kf, grads = prior_run(case, 1, "f64", None)
        ref = prior_run(case, 1, "ld", grads)[:2]
        for mut, acts in (("drift_plus", r > 0), ("draw_with_kinetic_table", r > 0), ("kinetic_first_256", r > 256)):
            if acts:
                err, where = traj_error(prior_run(case, 1, "f64", grads, mutation=mut)[:2], ref, ("svc", N, M))
                assert _rejected(err, "D"), (mut, case, err, where)
                acted[mut] += 1
    N, M, r, B = C.FLAG_CASE
    for name, nsteps, q0, z, bads in _flag_scenarios():
        grads = prior_run(C.FLAG_CASE, nsteps, "f64", None, q0, z, bads)[2]
        ref = prior_run(C.FLAG_CASE, nsteps, "ld", grads, q0, z, bads)[:2]
        for mut in ("kick_a_bad_chain", "no_drift_of_a_bad_chain"):
            got = prior_run(C.FLAG_CASE, nsteps, "f64", grads, q0, z, bads, mutation=mut)[:2]
            err, where = traj_error(got, ref, ("svc", N, M), rows=[1])
            assert _rejected(err, "D"), (mut, name, err, where)
            acted[mut] += 1
            # ... and the flagged chain's neighbours are none of its business
            assert traj_error(got, ref, ("svc", N, M), rows=[0, 2])[0] <= C.RESTATEMENT_WORST["D"]
    assert acted == {"drift_plus": 5, "draw_with_kinetic_table": 5, "kinetic_first_256": 1, "kick_a_bad_chain": 2,
                     "no_drift_of_a_bad_chain": 2}, acted


def test_the_whole_vector_norm_on_the_ill_conditioned_factors_against_mutation_3():
    """Mutation 3 at M = 8 on the hyper-parameters of tests/test_hmc_metric.py (kappa ~ 1e11), measured as that file measures: the
    whole-vector norm against NumPy's factor, bar 1e-5.  The block measure on the well-conditioned family rejects it at every case;
    what the old measure makes of it is printed and recorded, not required either way."""
    N, M = 64, 8
    x = C.grid(N)
    L = np.linalg.cholesky(C.cov_f64(x, C.HV_ILL[1], C.HV_ILL[2]))
    v = C.vectors("svc", N, M, 5)
    for trans in (False, True):
        ref = C.apply_svc(L, L, v, trans)
        got = C.mut_last_group_full(L, L, v, trans)
        whole = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
        print("mutation 3, N = 64, M = 8, trans = %d, ill-conditioned factors: whole-vector error %.3g (bar %.0e: %s)"
              % (trans, whole, C.ILL_BAR, "accepted" if whole < C.ILL_BAR else "rejected"))
        err, where = C.block_errors(C.mut_last_group_full(*C.factors(N, 0, "f64"), v, trans),
                                    C.apply_svc(*C.factors(N, 0, "ld"), v, trans), ("svc", N, M))
        assert _rejected(err, "A"), (err, where)


def test_report_the_worst_restatement_error_per_table():
    """Runs last: what the restatement tests above measured (the figures RESTATEMENT_WORST is read from)."""
    for table in sorted(WORST):
        err, where = WORST[table]
        print("metric sweep, float64 restatement against longdouble, table %s: worst %.3g at %s (recorded %.3g, bar %.3g)"
              % (table, err, where, C.RESTATEMENT_WORST[table], C.BAR[table]))
