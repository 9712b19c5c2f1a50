"""The one Metropolis loop (drivers._metropolis) and the one host leapfrog (drivers._leapfrog) behind every lock-step sampler, on toy
potentials: the step jitter, the whitened loop of BatchedHMCSeparable against its formulas written out, the leapfrog's mask and step
forms, and a chain that starts where its potential is undefined.  No GPU, no library."""
import warnings

import numpy as np
import pytest

import hadamard_cohort_cases as cc
import hadamard_cohort_hmc_cases as hh
from nonstationary_multivariate_gaussian_process_amd import drivers, hadamard

bits = hh.bits          # (NaN-aware: a NaN equals a NaN of the same bits)


# ---- 1: the jitter ----------------------------------------------------------------------------------------------------------------
def fake_group(rows, P, eps, seed, steps):
    """a group of free particles (U = 0) that records the step size of every trajectory it is asked for"""
    b = len(rows)
    gr = {"q": np.zeros((b, P)), "U": np.zeros(b), "rows": np.asarray(rows), "rngs": [np.random.default_rng(seed + r) for r in rows],
          "kinetic_end": lambda p1: 0.5 * (p1 * p1).sum(1), "commit": lambda acc, g1: None, "split": lambda q: [q]}

    def draw():
        p0 = np.stack([r.standard_normal(P) for r in gr["rngs"]])
        return p0, 0.5 * (p0 * p0).sum(1)

    def trajectory(jit, p0):
        steps.append(eps * jit)
        return gr["q"] + (eps * jit) * p0, p0, gr["U"], np.zeros(b, dtype=bool), None
    gr.update(draw=draw, trajectory=trajectory)
    return gr


@pytest.mark.parametrize("seed", [0, 12])
def test_the_jitter_is_one_factor_per_iteration_for_all_groups(seed):
    n, P, j, eps = 7, 3, 0.3, (0.125, 0.7)
    steps = ([], [])
    groups = [fake_group([0, 2], P, eps[0], seed, steps[0]), fake_group([1, 3, 4], P, eps[1], seed, steps[1])]
    for gr in groups:
        gr["samples"] = [np.zeros((n,) + gr["q"].shape)]
    accepted, ee, timing = drivers._metropolis(groups, n, 5, 0.0, j, drivers._jitter_rng(seed))
    u = np.random.default_rng(7919 * (seed + 1)).uniform(-1.0, 1.0, n)
    assert len(set(u)) == n and np.all(np.abs(u) > 1e-3)                                   # (the factors differ from 1 and from each other)
    for e, got in zip(eps, steps):
        assert got == [e * (1.0 + j * ui) for ui in u]
    assert np.all(accepted == n) and np.all(ee == 0.0)                                   # a free particle conserves its energy exactly
    assert set(timing) == {"setup_seconds", "loop_seconds", "trajectory_call_seconds", "device_share"}
    for gr in groups:
        assert np.array_equal(gr["samples"][0][-1], gr["q"]) and np.any(gr["q"] != 0.0)


def test_without_jitter_the_step_is_the_step_and_no_generator_is_touched():
    n, P = 4, 2
    for j in (0.0, -1.0):
        steps, rng = [], drivers._jitter_rng(3)
        before = rng.bit_generator.state
        gr = fake_group([0, 1], P, 0.3, 5, steps)
        gr["samples"] = [np.zeros((n, 2, P))]
        drivers._metropolis([gr], n, 2, 0.0, j, rng)
        assert steps == [0.3] * n and rng.bit_generator.state == before
        steps.clear()
        gr = fake_group([0, 1], P, 0.3, 5, steps)
        gr["samples"] = [np.zeros((n, 2, P))]
        drivers._metropolis([gr], n, 2, 0.0)                                               # (the default: no jitter, no generator at all)
        assert steps == [0.3] * n


def test_the_cohort_host_loop_runs_every_bucket_at_the_iterations_jittered_step():
    """HadamardStaCohortHMC on the NumPy restatement, several buckets: every trajectory of iteration i gets eps_s (1 + j u_i)."""
    model, cases, k, seed, j, n = "sta", cc.SET_A, 2, 31, 0.25, 3
    buckets = hadamard.cohort_buckets(cc.nobs(cases), 0.0)
    assert len(buckets) > 1
    eps = hh.eps_of(len(cases))
    d = drivers.HadamardStaCohortHMC(hh.subject_triples(cases), hh.hyper_dict(model, cases), hh.chains(model, cases, k), step_size=eps,
                                     num_steps_in_leap=2, seed=seed, step_jitter=j, max_flop_waste=0.0,
                                     evaluators=[hh.reference_evaluator(model, [cases[int(s)] for s in idx], k) for idx in buckets])
    seen, inner = [], d._host_traj

    def recording(st, e, p0):
        seen.append((st["idx"], e.copy()))
        return inner(st, e, p0)
    d._host_traj = recording
    _, info = d.run(n)
    d.close()
    u = np.random.default_rng(7919 * (seed + 1)).uniform(-1.0, 1.0, n)
    assert len(seen) == n * len(buckets) and np.all(np.isfinite(info["energy_error"]))
    for c, (idx, e) in enumerate(seen):
        assert np.array_equal(e, np.repeat(eps[idx] * (1.0 + j * u[c // len(buckets)]), k))


# ---- 2: the whitened loop of BatchedHMCSeparable ----------------------------------------------------------------------------------
N, M, B, L, ITERS = 5, 2, 3, 3, 6
T = M * (M + 1) // 2
P = 2 * N + T + 1
WALL = 0.6                                      # the potential is undefined where q[0] > WALL


def toy_potential(q):
    """an anisotropic quadratic, undefined (inf, zero gradient: what the drivers report) on the half-space q[0] > WALL"""
    a = 0.5 + np.arange(P) / P
    U, g = 0.5 * (a * q * q).sum(1), a * q
    bad = q[:, 0] > WALL
    U[bad] = np.inf
    g[bad] = 0.0
    return U, g


class ToySeparable(drivers.BatchedHMCSeparable):
    """the driver without its constructor's GPU part: no context, no data"""

    def __init__(self, init, eps, seed, metric, step_jitter):
        drivers.LockStepHMC.__init__(self, init, eps, L, seed, metric)
        self.step_jitter, self.jitter_rng = float(step_jitter), drivers._jitter_rng(seed)

    def potential_and_grad(self, q):
        return toy_potential(q)


def toy_metric(rank):
    rng = np.random.default_rng(77)
    x = np.linspace(0.0, 1.0, N)
    K = np.exp(-0.5 * ((x[:, None] - x[None, :]) / 0.4) ** 2)
    L_l, L_s = np.linalg.cholesky(0.8 * K + 1e-3 * np.eye(N)), np.linalg.cholesky(1.3 * K + 1e-2 * np.eye(N))
    U = lam = None
    if rank:
        U = np.ascontiguousarray(np.linalg.qr(rng.standard_normal((P, rank)))[0].T)
        lam = np.array([3.0, 0.7])[:rank]
    return drivers.SeparablePriorMetric(L_l, L_s, 0.9, T, U, lam)


def whitened_loop_written_out(init, eps0, seed, met, j, n):
    """BatchedHMCSeparable.run's docstring, line by line, with the metric's own products: u = (I + U lam U^T)^1/2 z, K0 = 1/2 |z|^2,
    kick u -= c L_blk^T g, drift q += eps L_blk (I + U lam U^T)^-1 u, K1 = 1/2 u^T (I + U lam U^T)^-1 u; a chain whose potential is
    undefined anywhere on the way is rejected; chain b draws P normals, then the accept uniform, from default_rng(seed + b); one
    jitter factor per iteration from default_rng(7919 (seed + 1))."""
    q = init.copy()
    rngs = [np.random.default_rng(seed + b) for b in range(B)]
    jit = np.random.default_rng(7919 * (seed + 1))
    U, g = toy_potential(q)
    samples, ee, accepted, failures = np.zeros((n, B, P)), np.zeros((n, B)), np.zeros(B), 0
    for it in range(n):
        eps = eps0 * (1.0 + j * jit.uniform(-1.0, 1.0))
        z = np.stack([r.standard_normal(P) for r in rngs])
        H0 = U + 0.5 * (z * z).sum(1)
        u1 = met.root(z) - (0.5 * eps) * met.apply(g, True)
        q1, failed = q, np.zeros(B, dtype=bool)
        for step in range(L):
            q1 = q1 + eps * met.apply(met.W(u1), False)
            U1, g1 = toy_potential(q1)
            failed |= ~np.isfinite(U1)
            u1 = u1 - (eps if step < L - 1 else 0.5 * eps) * met.apply(g1, True)
        failures += int((failed & np.isfinite(U1)).sum())                  # left the domain on the way and came back
        with np.errstate(invalid="ignore"):
            dH = np.where(failed, np.inf, U1) + met.kinetic(u1) - H0
        lu = np.array([np.log(r.random()) for r in rngs])
        acc = np.isfinite(dH) & (lu < -dH)
        q = np.where(acc[:, None], q1, q)
        U, g = np.where(acc, U1, U), np.where(acc[:, None], g1, g)
        accepted += acc
        ee[it], samples[it] = np.where(np.isfinite(dH), dH, np.nan), q
    return samples, accepted / n, ee, failures


@pytest.mark.parametrize("rank", [0, 2])
def test_whitened_separable_loop_equals_its_formulas_written_out(rank):
    seed, eps, j = 9, 0.35, 0.2
    met = toy_metric(rank)
    init = 0.3 * np.random.default_rng(1).standard_normal((B, P))
    init[:, 0] = [0.5, -0.4, 0.1]                                          # chain 0 starts next to the wall
    ref_samples, ref_rate, ref_ee, came_back = whitened_loop_written_out(init, eps, seed, met, j, ITERS)
    samples, info = ToySeparable(init, eps, seed, met, j).run(ITERS)
    assert np.array_equal(bits(samples), bits(ref_samples)) and np.array_equal(bits(info["energy_error"]), bits(ref_ee))
    assert np.array_equal(info["accept_rate"], ref_rate)
    # the run shows what it is meant to: a rejection by `failed`, both decisions, and the jitter at work
    assert np.isnan(ref_ee).any() and 0 < ref_rate.sum() < B and not np.any(samples[:, :, 0] > WALL)
    assert not np.array_equal(samples, ToySeparable(init, eps, seed, met, 0.0).run(ITERS)[0])
    print("rank", rank, "accept", ref_rate, "failed trajectories that ended inside the domain:", came_back)


def test_without_a_prior_metric_the_separable_driver_ignores_step_jitter():
    init = 0.3 * np.random.default_rng(2).standard_normal((B, P))
    a = ToySeparable(init, 0.2, 4, None, 0.5).run(ITERS)
    b = ToySeparable(init, 0.2, 4, None, 0.0).run(ITERS)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]["energy_error"]), bits(b[1]["energy_error"]))


# ---- 3: the leapfrog's forms ------------------------------------------------------------------------------------------------------
def leapfrog_case(seed=3):
    rng = np.random.default_rng(seed)
    q, p = 0.4 * rng.standard_normal((B, P)), rng.standard_normal((B, P))
    w, s = 0.5 + rng.random(P), 0.5 + rng.random(P)
    U, g = toy_potential(q)
    return q, p, U, g, (lambda g_: w * g_), (lambda p_: s * p_)


def test_leapfrog_all_true_mask_and_column_step_change_no_bit():
    q, p, U, g, kick, drift = leapfrog_case()
    eps = 0.3
    plain = drivers._leapfrog(q, p, U, g, eps, L, toy_potential, kick, drift)
    assert plain[4].any() and not plain[4].all()                           # a chain fails, a chain does not
    assert np.all(np.isinf(plain[2][plain[4]])) and np.all(np.isfinite(plain[2][~plain[4]]))
    for kw in ({"mask": np.ones((B, P), dtype=bool)}, {}):
        for e in (eps, np.full((B, 1), eps)):
            got = drivers._leapfrog(q, p, U, g, e, L, toy_potential, kick, drift, **kw)
            for a, b in zip(plain, got):
                assert np.array_equal(bits(a), bits(b)) if a.dtype != bool else np.array_equal(a, b)
    rows = drivers._leapfrog(q, p, U, g, np.array([[0.3], [0.2], [0.1]]), L, toy_potential, kick, drift)      # a step per row
    for b_, e in enumerate((0.3, 0.2, 0.1)):
        one = drivers._leapfrog(q, p, U, g, e, L, toy_potential, kick, drift)
        assert all(np.array_equal(bits(a[b_]), bits(c[b_])) for a, c in zip(rows[:4], one[:4]))


def test_leapfrog_padded_slots_are_inert():
    """padded p is +0.0 from the first kick on, padded q never changes, whatever the padded slots hold -- and without a warning"""
    q, p, U, g, kick, drift = leapfrog_case()
    mask = np.ones((B, P), dtype=bool)
    mask[1, 4:7] = mask[2, -2:] = False

    def evaluate(q_):                                                     # the padded slots do not enter the potential
        return toy_potential(np.where(mask, q_, 0.0))
    clean = drivers._leapfrog(np.where(mask, q, 0.0), p, U, g, 0.3, L, evaluate, kick, drift, mask)
    dirty_q, dirty_p, dirty_g = np.where(mask, q, np.nan), np.where(mask, p, np.inf), np.where(mask, g, -np.inf)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        dirty = drivers._leapfrog(dirty_q, dirty_p, U, dirty_g, 0.3, L, evaluate, kick, drift, mask)
    assert np.all(np.isnan(dirty[0][~mask])) and np.all(dirty[1][~mask] == 0.0) and not np.any(np.signbit(dirty[1][~mask]))
    for a, b in zip(clean[:2], dirty[:2]):
        assert np.array_equal(bits(a)[mask], bits(b)[mask])
    assert np.array_equal(bits(clean[2]), bits(dirty[2])) and np.array_equal(clean[4], dirty[4])


# ---- 4: a start where the potential is undefined -----------------------------------------------------------------------------------
class Toy(drivers.LockStepHMC):
    def potential_and_grad(self, q):
        return toy_potential(q)


def test_a_chain_that_starts_at_an_undefined_potential_is_never_accepted():
    """U = inf at the start gives H0 = inf, so dH is -inf or NaN whatever the trajectory does: rejected, NaN on record -- whether or
    not the leapfrog counts the start among the points where a chain fails (it does).  The other chains do not notice."""
    init = 0.3 * np.random.default_rng(6).standard_normal((B, P))
    init[:, 0] = [WALL + 0.05, 0.0, -0.2]                                  # chain 0: just outside, its trajectories reach the domain
    lock = Toy(init, step_size=0.3, num_steps_in_leap=L, seed=2)
    samples, info = lock.run(ITERS)
    assert info["accept_rate"][0] == 0.0 and np.all(np.isnan(info["energy_error"][:, 0]))
    assert np.array_equal(samples[:, 0], np.repeat(init[:1], ITERS, axis=0)) and np.array_equal(lock.q[0], init[0])
    assert info["accept_rate"][1:].min() > 0
    # the claim is not empty: with the momenta of this run, some trajectory of chain 0 ends at a point where the potential is defined
    rng, ended_inside = np.random.default_rng(2), 0
    for _ in range(ITERS):
        p0 = rng.standard_normal(P)[None]
        rng.random()
        U0, g0 = toy_potential(init[:1])
        q1, _, U1, _, failed = drivers._leapfrog(init[:1], p0, U0, g0, 0.3, L, toy_potential, lambda g: g, lambda p: p)
        assert failed[0] and np.isinf(U1[0])
        ended_inside += int(np.isfinite(toy_potential(q1)[0][0]))
    assert ended_inside > 0
    moved = init.copy()
    moved[0, 0] = 0.0                                                      # the same run with chain 0 inside the domain
    other, oinfo = Toy(moved, step_size=0.3, num_steps_in_leap=L, seed=2).run(ITERS)
    assert np.array_equal(bits(samples[:, 1:]), bits(other[:, 1:]))
    assert np.array_equal(bits(info["energy_error"][:, 1:]), bits(oinfo["energy_error"][:, 1:])) and oinfo["accept_rate"][0] > 0
