"""CPU half of the prior-factor metric of the Hadamard cohort (no GPU; sets, references, measure and recorded figures:
tests/hadamard_cohort_metric_cases.py; GPU half: tests/test_gpu_hadamard_cohort_metric.py).

1. The family: kappa <= metric_cases.KAPPA_MAX for every subject's two factors, and every 64 x 64 tile of the lower triangle holds an
   entry >= 0.5 % (factor A) / 0.01 % (factor B: its ragged corner tiles at N_s = 129 and 193 hold 0.17 % and 0.03 %) of the factor's
   largest -- four orders and more above what a masking or tiling error needs to pass the bar of ~1e-12.
2. The float64 restatement -- the DEFINING host loop of drivers._HadamardCohortHMC with mass="prior": _prior_factor, _metric_apply,
   _host_traj -- against the np.longdouble references: both products, one and two leapfrog steps (gradients from the models'
   restatements, fed to both), the one-ulp sensitivity of the two-step middle point.  The worst figures are printed and must not
   exceed their entries of C.RESTATEMENT_WORST, whose 50-fold (never above 1e-10) is the GPU half's bar.
3. Meaning: the whitened host trajectory against a dense-mass leapfrog with M^-1 = L_blk L_blk^T and p0 = L_blk^-T z in longdouble
   (set P), in q1 - q0 and in H1 - H0.
4. The drivers' host loop on the restatement, 3 iterations x 3 steps on sets P and Q with max_flop_waste 0 and 0.5: every accept
   decision of C.DRIVER_SEED is further than 1e-6 from its threshold (the GPU half compares decisions); the stationary model refuses.
5. The metric does its job: C.JOB_EPS and C.JOB_STEPS on set P under the golden ill-conditioned hyper-parameters -- |dH| < 1 for
   every chain under mass="prior"; under the identity mass every chain fails or has |dH| > 10, except those of the subject with
   N_s = 2, whose L_blk is diagonal (C.JOB_DIAGONAL: no step size can separate the two masses there)."""
import numpy as np
import pytest

import hadamard_cohort_hmc_cases as hh
import hadamard_cohort_metric_cases as C
import metric_cases as mc

WORST = {}


def _note(table, err, where):
    if err >= WORST.get(table, (-1.0, ""))[0]:
        WORST[table] = (err, where)
    print("%s: %.3g at %s (entry %.3g)" % (table, err, where, C.RESTATEMENT_WORST.get(table, C.ONE_ULP_SENSITIVITY)))
    assert err <= C.RESTATEMENT_WORST[table], (table, where, err, C.RESTATEMENT_WORST[table])


def host_driver(model, name, k, nsteps, starts=None, eps=None, mass="prior", ill=False, waste=1e9, seed=C.DRIVER_SEED, evaluators=True):
    """the cohort driver's host loop on the restatement (one evaluator per bucket)"""
    from nonstationary_multivariate_gaussian_process_amd import drivers, hadamard
    ev = None
    if evaluators:
        ev = [C.reference_evaluator(model, name, k, ill, [int(s) for s in idx]) for idx in hadamard.cohort_buckets(C.sizes(name), waste)]
    return getattr(drivers, hh.DRIVER[model])(C.triples(name), C.hyper_dict(model, ill), C.chains(model, name, k) if starts is None else starts,
                                               step_size=C.eps_of(name) if eps is None else eps, num_steps_in_leap=nsteps, seed=seed,
                                               mass=mass, device_resident=False, evaluators=ev, max_flop_waste=waste)


def bucket_rows(drv, st, rows):
    """per-subject rows (caller's order) -> the bucket's padded rows"""
    return drv._pack([rows[s] for s in st["idx"]], st["nobs"], drv.M)


def caller_rows(drv, st, P, n):
    out = [None] * n
    for s, r in zip(st["idx"], drv._unpack(P, st["nobs"], drv.M, drv.k)):
        out[s] = r
    return out


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------------
def test_the_factors_are_well_conditioned_and_populated_far_from_the_diagonal():
    for name in C.SETS:
        for s, N in enumerate(C.sizes(name)):
            for which in "AB":
                L = np.asarray(mc.factor(which, N, s, "ld"), dtype=np.float64)
                kappa = np.linalg.cond(L) ** 2
                assert kappa <= mc.KAPPA_MAX[which], (name, s, which, kappa)
                big, nt = np.abs(L).max(), (N + mc.TILE - 1) // mc.TILE
                for it in range(nt):
                    for kt in range(it + 1):
                        m = np.abs(L[it * mc.TILE:(it + 1) * mc.TILE, kt * mc.TILE:(kt + 1) * mc.TILE]).max()
                        assert m >= (5e-3 if which == "A" else 1e-4) * big, (name, s, which, it, kt, m / big)


def test_the_drivers_factor_is_the_oracles():
    from nonstationary_multivariate_gaussian_process_amd import drivers
    for s, N in enumerate(C.sizes("P")):
        for which, h in (("A", mc.HYPER_A), ("B", mc.HYPER_B)):
            got = drivers._HadamardCohortHMC._prior_factor(mc.grid(N, s), *h)
            assert np.array_equal(got, mc.factor(which, N, s, "f64"))


def test_every_block_of_every_test_vector_is_non_zero_and_no_bar_exceeds_the_cap():
    for model in C.MODELS:
        for name in C.SETS:
            for s, v in enumerate(C.vectors(model, name, 2)):
                for bname, sl in mc.blocks(*C.layout_of(model, name, s)):
                    assert np.all(np.abs(v[:, sl]).max(axis=1) > 0), (model, name, s, bname)
            assert np.array_equal(C.vectors(model, name, 1)[0][0], C.vectors(model, name, 2)[0][0])
    for k, bar in C.BAR.items():
        assert bar <= mc.BAR_CAP, (k, bar)
    assert C.RESTATEMENT_WORST["traj2"] == C.RESTATEMENT_WORST["traj"] + C.ONE_ULP_SENSITIVITY


# ---- 2 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.SETS))
@pytest.mark.parametrize("model", C.MODELS)
def test_restatement_of_the_products(model, name):
    k, S = 2, len(C.sizes(name))
    drv = host_driver(model, name, k, 1)
    st = drv.state[0]
    v = C.vectors(model, name, k)
    for trans in (False, True):
        got = caller_rows(drv, st, drv._metric_apply(st, bucket_rows(drv, st, v), trans), S)
        ref = [C.apply_rows(model, name, s, v[s], trans) for s in range(S)]
        err, where = C.worst_block(model, name, got, ref)
        _note("apply", err, "%s set %s trans=%d %s" % (model, name, trans, where))
    # padded slots of the host product are +0.0, and NaN in the padded slots of the input changes nothing
    Pv = bucket_rows(drv, st, v)
    out = drv._metric_apply(st, np.where(st["mask"], Pv, np.nan), False)
    assert np.array_equal(hh.bits(out), hh.bits(drv._metric_apply(st, Pv, False)))
    assert np.all(out[~st["mask"]] == 0.0) and not np.any(np.signbit(out[~st["mask"]]))


def host_trajectory(model, name, k, nsteps, shift=None):
    """the host loop's trajectory of every subject from C.chains with the whitened momenta C.vectors: per subject (q0, z, g0, q1, u1),
    and the evaluated middle points' gradients are the restatement's; shift: a seed for a one-ulp move of the evaluated middle point"""
    S = len(C.sizes(name))
    drv = host_driver(model, name, k, nsteps)
    st = drv.state[0]
    if shift is not None:
        inner, calls = st["eval"], [0]

        def shifted(P):
            calls[0] += 1
            return inner(np.where(st["mask"], mc.ulp_shift(P, shift), P) if calls[0] == 2 else P)    # call 1: the start, 2: the middle
        st["eval"] = shifted
    st["U"], st["g"] = drv._potential(st["eval"](st["q"]))
    z = C.vectors(model, name, k)
    eps = np.repeat(C.eps_of(name)[st["idx"]], k)
    q1, u1, U1, g1, failed = drv._host_traj(st, eps, bucket_rows(drv, st, z))
    assert not failed.any()
    return (caller_rows(drv, st, st["q"], S), z, caller_rows(drv, st, st["g"], S), caller_rows(drv, st, q1, S), caller_rows(drv, st, u1, S))


def reference_trajectory(model, name, nsteps, q0, z, g0):
    """per subject (displacement q_n - q_0, u1) in longdouble, the gradient of an evaluated point taken from the restatement at the
    point rounded to float64"""
    disp, u1 = [], []
    for s in range(len(C.sizes(name))):
        grad = C.subject_grad(model, name, s)
        pts, u = C.leapfrog_ld(model, name, s, q0[s], z[s], C.eps_of(name)[s], nsteps, g0[s], lambda step, q: grad(q)[1])
        disp.append(mc.displacement(pts))
        u1.append(u)
    return disp, u1


@pytest.mark.parametrize("name", sorted(C.SETS))
@pytest.mark.parametrize("model", C.MODELS)
def test_restatement_of_one_step(model, name):
    q0, z, g0, q1, u1 = host_trajectory(model, name, 2, 1)
    disp, uref = reference_trajectory(model, name, 1, q0, z, g0)
    got = [np.asarray(a, dtype=mc.LD) - np.asarray(b, dtype=mc.LD) for a, b in zip(q1, q0)]
    err, where = C.worst_block(model, name, got, disp)
    _note("traj", err, "%s set %s one step %s" % (model, name, where))
    assert max(float(np.abs(d).max()) for d in got) > 1e-8                    # the chains went somewhere


@pytest.mark.parametrize("model", C.MODELS)
def test_restatement_of_two_steps_and_its_sensitivity_to_the_middle_point(model):
    name = "P"
    q0, z, g0, q1, u1 = host_trajectory(model, name, 2, 2)
    disp, uref = reference_trajectory(model, name, 2, q0, z, g0)
    got = [np.asarray(a, dtype=mc.LD) - np.asarray(b, dtype=mc.LD) for a, b in zip(q1, q0)]
    err, where = C.worst_block(model, name, got, disp)
    sens = 0.0
    for seed in (1, 2):
        qs = host_trajectory(model, name, 2, 2, shift=seed)[3]
        shifted = [np.asarray(a, dtype=mc.LD) - np.asarray(b, dtype=mc.LD) for a, b in zip(qs, q0)]
        sens = max(sens, C.worst_block(model, name, shifted, got)[0])
    print("two steps, %s: restatement %.3g, one-ulp sensitivity %.3g" % (model, err, sens))
    assert sens <= C.ONE_ULP_SENSITIVITY
    _note("traj2", err, "%s set %s two steps %s" % (model, name, where))


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", C.MODELS)
def test_the_whitened_trajectory_is_the_dense_mass_leapfrog(model):
    name, k, nsteps = "P", 2, 2
    S = len(C.sizes(name))
    eps = C.eps_of(name, C.MEANING_EPS0)
    drv = host_driver(model, name, k, nsteps)
    st = drv.state[0]
    st["U"], st["g"] = drv._potential(st["eval"](st["q"]))
    z = C.vectors(model, name, k)
    zp = bucket_rows(drv, st, z)
    q1, u1, U1, g1, failed = drv._host_traj(st, np.repeat(eps[st["idx"]], k), zp)
    assert not failed.any()
    dH = (np.asarray(U1, dtype=mc.LD) + drv._kinetic(st, u1)) - (np.asarray(st["U"], dtype=mc.LD) + drv._kinetic(st, zp))
    q0r, q1r, g0r = caller_rows(drv, st, st["q"], S), caller_rows(drv, st, q1, S), caller_rows(drv, st, st["g"], S)
    worst_q, worst_H = (0.0, ""), (0.0, "")
    for j, s in enumerate(st["idx"]):
        grad = C.subject_grad(model, name, s)
        pts, K0, K1 = C.leapfrog_dense_ld(model, name, s, q0r[s], z[s], eps[s], nsteps, g0r[s], lambda step, q: grad(q)[1])
        e, w = mc.block_errors(np.asarray(q1r[s], dtype=mc.LD) - np.asarray(q0r[s], dtype=mc.LD), mc.displacement(pts), C.layout_of(model, name, s))
        worst_q = max(worst_q, (e, "subject %d %s" % (s, w)))
        ref = (np.asarray(grad(pts[-1])[0], dtype=mc.LD) + K1) - (np.asarray(grad(pts[0])[0], dtype=mc.LD) + K0)
        eH = mc.scalar_error(dH[j * k:(j + 1) * k], ref)
        print("subject", s, "dH", dH[j * k:(j + 1) * k], "dense", ref, "err", eH)
        worst_H = max(worst_H, (eH, "subject %d" % s))
    _note("meaning_q", worst_q[0], "%s %s" % (model, worst_q[1]))
    _note("meaning_H", worst_H[0], "%s %s" % (model, worst_H[1]))


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------------
def replay_uniforms(model, name, k, n, seed):
    """log u of every accept test: chain b draws from default_rng(seed + b): P_s normals, then the uniform, per iteration"""
    out = np.zeros((n, len(C.sizes(name)) * k))
    for s, v in enumerate(C.chains(model, name, k)):
        for j in range(k):
            rng = np.random.default_rng(seed + s * k + j)
            for it in range(n):
                rng.standard_normal(v.shape[1])
                out[it, s * k + j] = np.log(rng.random())
    return out


@pytest.mark.parametrize("waste", (0.0, 0.5))
@pytest.mark.parametrize("name", ("P", "Q"))
@pytest.mark.parametrize("model", C.MODELS)
def test_no_accept_decision_of_the_driver_seed_is_near_its_threshold(model, name, waste):
    k, n = 2, 3
    drv = host_driver(model, name, k, 3, eps=C.DRIVER_EPS, waste=waste)
    samples, info = drv.run(n)
    logu, dH = replay_uniforms(model, name, k, n, C.DRIVER_SEED), info["energy_error"]
    assert np.all(np.isfinite(dH))
    margin = np.abs(logu + dH)
    print(model, name, waste, "accept rate", info["accept_rate"], "smallest margin", margin.min())
    assert margin.min() > C.DECISION_MARGIN
    for s, smp in enumerate(samples):
        assert smp.shape == (n, k, C.chains(model, name, k)[s].shape[1])
    assert 0 < info["accept_rate"].sum() < len(info["accept_rate"])            # both decisions occur


def test_the_stationary_model_refuses_the_prior_metric():
    from nonstationary_multivariate_gaussian_process_amd import drivers
    import hadamard_cohort_cases as cc
    cases = cc.SET_D
    with pytest.raises(ValueError):
        drivers.HadamardStaCohortHMC(hh.subject_triples(cases), hh.hyper_dict("sta", cases), hh.chains("sta", cases, 1), mass="prior",
                                     device_resident=False, evaluators=[None])
    with pytest.raises(ValueError):
        host_driver("non", "E", 1, 1, mass="posterior")


# ---- 5 ----------------------------------------------------------------------------------------------------------------------------------
def job_run(model, mass):
    name, k = "P", 2
    drv = host_driver(model, name, k, C.JOB_STEPS, starts=C.prior_draw_chains(model, name, k), eps=C.JOB_EPS, mass=mass, ill=True)
    samples, info = drv.run(1)
    return info["energy_error"][0]


@pytest.mark.parametrize("model", C.MODELS)
def test_the_metric_does_its_job_on_the_restatement(model):
    dp, di = job_run(model, "prior"), job_run(model, None)
    print(model, "dH under the prior metric", dp, "under the identity", di)
    k = 2
    diag = np.arange(dp.shape[0]) // k == C.JOB_DIAGONAL                        # (see C.JOB_DIAGONAL: a diagonal L_blk)
    assert np.all(np.abs(dp) < C.JOB_DH_PRIOR)
    assert np.all(np.isnan(di[~diag]) | (np.abs(di[~diag]) > C.JOB_DH_IDENTITY))    # (NaN: the chain failed)
    assert np.all(np.abs(di[diag]) < C.JOB_DH_PRIOR)


def test_report_the_restatement_figures():
    for table, (err, where) in sorted(WORST.items()):
        print("%-10s worst %.3g (entry %.3g, GPU bar %.3g) at %s" % (table, err, C.RESTATEMENT_WORST[table], C.BAR[table], where))
