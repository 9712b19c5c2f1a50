"""The cohort HMC drivers' host loop (drivers.HadamardCohortHMC / HadamardSepCohortHMC / HadamardStaCohortHMC with ``evaluators=``
built from the NumPy restatements: no GPU): against one LockStepHMC per subject, the padding, the per-subject step sizes, and the
layout masks the device kernels restate."""
import numpy as np
import pytest

import hadamard_cohort_cases as cc
import hadamard_cohort_hmc_cases as hh
from nonstationary_multivariate_gaussian_process_amd import drivers, hadamard

SEED = 4100
ITERS, STEPS = 3, 3


def cohort(model, cases, k, starts=None, eps=None, mass=None, seed=SEED, iters=ITERS):
    """one bucket (max_flop_waste huge), the restatement as its evaluator"""
    starts = hh.chains(model, cases, k) if starts is None else starts
    eps = hh.eps_of(len(cases)) if eps is None else eps
    d = make(model, cases, k, starts, eps, mass, seed)
    samples, info = d.run(iters)
    d.close()
    return d, samples, info


def make(model, cases, k, starts, eps, mass=None, seed=SEED):
    """the driver with ONE bucket; its rows are in the bucket's order (by size, descending), and so is the evaluator's subject list"""
    buckets = hadamard.cohort_buckets(cc.nobs(cases), 1e30)
    assert len(buckets) == 1 and sorted(int(s) for s in buckets[0]) == list(range(len(cases)))
    ordered = [cases[int(s)] for s in buckets[0]]
    d = getattr(drivers, hh.DRIVER[model])(hh.subject_triples(cases), hh.hyper_dict(model, cases), starts, step_size=eps,
                                           num_steps_in_leap=STEPS, seed=seed, mass=mass, max_flop_waste=1e30,
                                           evaluators=[hh.reference_evaluator(model, ordered, k)])
    assert [int(s) for s in d.buckets[0]] == [int(s) for s in buckets[0]]
    return d


@pytest.mark.parametrize("masses", [False, True], ids=["identity", "diagonal"])
@pytest.mark.parametrize("name,k", [("A", 2), ("D", 1)])
@pytest.mark.parametrize("model", hh.MODELS)
def test_cohort_host_loop_is_the_per_subject_sampler(model, name, k, masses):
    """Samples, accept decisions and energy errors of the cohort host loop equal, bit for bit, those of one LockStepHMC per subject on
    the same restatement with seed + s k (set D: sizes 1, 2, 70 with M = 1)."""
    cases = cc.SETS[name]
    mass = hh.diag_mass(model, cases) if masses else None
    eps = hh.eps_of(len(cases))
    _, samples, info = cohort(model, cases, k, mass=mass)
    for s, case in enumerate(cases):
        ref = drivers.LockStepHMC(hh.chains(model, cases, k)[s], step_size=eps[s], num_steps_in_leap=STEPS, seed=SEED + s * k,
                                  M=None if mass is None else mass[s])
        ref.potential_and_grad = hh.subject_evaluator(model, case)
        ref_samples, ref_info = ref.run(ITERS)
        rows = slice(s * k, (s + 1) * k)
        assert samples[s].shape == ref_samples.shape and np.array_equal(hh.bits(samples[s]), hh.bits(ref_samples)), (model, case)
        assert np.array_equal(hh.bits(info["energy_error"][:, rows]), hh.bits(ref_info["energy_error"])), (model, case)
        assert np.array_equal(info["accept_rate"][rows], ref_info["accept_rate"]), (model, case)
    assert np.all(np.isfinite(info["energy_error"])) and info["accept_rate"].shape == (len(cases) * k,)
    assert set(info["timing"]) == {"setup_seconds", "loop_seconds", "trajectory_call_seconds", "device_share"}


@pytest.mark.parametrize("model", ("non", "sep"))
def test_padding_is_inert(model):
    """NaN in every padded slot of the start positions changes no bit of a real slot, and comes back unchanged."""
    cases, k = cc.SET_A, 2
    sizes, M = cc.nobs(cases), cases[0][1]
    d0, clean, info0 = cohort(model, cases, k)
    d = make(model, cases, k, hh.chains(model, cases, k), hh.eps_of(len(cases)))
    order = [int(s) for s in d.buckets[0]]
    pads = hh.padded_slots(model, [sizes[s] for s in order], M, max(sizes), k)
    assert pads.any() and np.array_equal(~pads, d.state[0]["mask"])
    d.state[0]["q"][pads] = np.nan
    poisoned, info = d.run(ITERS)
    assert np.all(np.isnan(d.state[0]["q"][pads])) and np.all(np.isfinite(d.state[0]["q"][~pads]))
    for a, b in zip(clean, poisoned):
        assert np.array_equal(hh.bits(a), hh.bits(b))
    assert np.array_equal(hh.bits(info0["energy_error"]), hh.bits(info["energy_error"]))


@pytest.mark.parametrize("model", hh.MODELS)
def test_step_sizes_are_per_subject(model):
    cases, k, who = cc.SET_A, 1, 3
    eps = hh.eps_of(len(cases))
    other = eps.copy()
    other[who] *= 1.5
    _, a, _ = cohort(model, cases, k, eps=eps)
    _, b, _ = cohort(model, cases, k, eps=other)
    for s in range(len(cases)):
        assert np.array_equal(hh.bits(a[s]), hh.bits(b[s])) == (s != who), (model, s)


@pytest.mark.parametrize("M", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("model", hh.MODELS)
def test_mask_and_layout_agree(model, M):
    """real_slot restated equals the complement of the case modules' padded_slots (and of what the package's pack writes), for
    N_s = 1 (where M allows it: a subject holds every label, so N_s >= M), Nmax - 1 and Nmax."""
    T, Nmax = M * (M + 1) // 2, 2 * M + 3
    sizes = sorted({max(1, M), Nmax - 1, Nmax})
    pads = hh.padded_slots(model, sizes, M, Nmax)
    assert pads.shape == (len(sizes), hh.plen(model, Nmax, M))
    for s, n in enumerate(sizes):
        mask = np.array([hh.real_slot(model, i, Nmax, n, T) for i in range(pads.shape[1])], dtype=bool)
        assert np.array_equal(mask, ~pads[s]), (model, M, n)
        if model != "sta":
            ones = hh.pack(model, [np.ones((1, int(mask.sum())))], [n], M, Nmax=Nmax, fill=0.0)
            assert np.array_equal(ones[0] == 1.0, mask)
    if model == "non":          # the package's unpack inverts the mask's order
        v = [np.arange(1.0, n * (1 + T) + 2)[None] for n in sizes]
        P = hadamard.cohort_pack(v, sizes, M, Nmax=Nmax, fill=-1.0)
        for s, n in enumerate(sizes):
            assert np.array_equal(P[s][~pads[s]], v[s][0])
