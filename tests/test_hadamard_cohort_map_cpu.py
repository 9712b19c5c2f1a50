"""The cohort MAP drivers' host loop (drivers.HadamardCohortMAP / HadamardSepCohortMAP / HadamardStaCohortMAP with ``evaluators=``
built from the NumPy restatements: no GPU): against one LockStepMAP per subject, a chain that fails, and the signatures and symbols
of the resident optimiser (nmgp_had_subjects_adam_*)."""
import inspect
import os
import re

import numpy as np
import pytest

import hadamard_cohort_cases as cc
import hadamard_cohort_hmc_cases as hh
import hadamard_cohort_map_cases as hm
from conftest import ROOT
from nonstationary_multivariate_gaussian_process_amd import _lib, drivers, hadamard

ITERS = 4


def make(model, cases, k, evaluator=None):
    """the driver with ONE bucket; its rows are in the bucket's order (by size, descending), and so is the evaluator's subject list"""
    buckets = hadamard.cohort_buckets(cc.nobs(cases), 1e30)
    assert len(buckets) == 1 and sorted(int(s) for s in buckets[0]) == list(range(len(cases)))
    ordered = [cases[int(s)] for s in buckets[0]]
    ev = hh.reference_evaluator(model, ordered, k)
    d = getattr(drivers, hm.DRIVER[model])(hh.subject_triples(cases), hh.hyper_dict(model, cases), hh.chains(model, cases, k), lr=hm.LR,
                                           chains_per_subject=k, max_flop_waste=1e30,
                                           evaluators=[ev if evaluator is None else evaluator(ev)])
    assert d.ctxs == [] and not d.device_resident and [int(s) for s in d.buckets[0]] == [int(s) for s in buckets[0]]
    return d, ordered


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("name", ["A", "D", "E"])
@pytest.mark.parametrize("model", hh.MODELS)
def test_cohort_host_loop_is_the_per_subject_loop(model, name, k):
    """Parameters, history and alive of the cohort loop equal, bit for bit, those of one LockStepMAP per subject on the same
    restatement; the padded slots of the cohort's rows keep their start bits."""
    cases = cc.SETS[name]
    sizes, M = cc.nobs(cases), cases[0][1]
    d, ordered = make(model, cases, k)
    start = d.maps[0].P.copy()
    calls = []
    pars, hist, alive = d.run(ITERS, lambda i, h: calls.append((i, h.copy())))
    d.close()
    assert hist.shape == (ITERS, len(cases) * k) and alive.tolist() == [True] * (len(cases) * k) and np.all(np.isfinite(hist))
    assert [i for i, _ in calls] == list(range(ITERS)) and all(np.array_equal(hh.bits(h), hh.bits(hist[i])) for i, h in calls)
    for s, case in enumerate(cases):
        ref = drivers.LockStepMAP(hh.chains(model, cases, k)[s], lr=hm.LR)
        ref.value_and_grad = hm.subject_evaluator(model, case)
        rp, rh, ra = ref.run(ITERS)
        rows = slice(s * k, (s + 1) * k)
        assert pars[s].shape == rp.shape and np.array_equal(hh.bits(pars[s]), hh.bits(rp)), (model, case)
        assert np.array_equal(hh.bits(hist[:, rows]), hh.bits(rh)) and np.array_equal(alive[rows], ra), (model, case)
        assert not np.array_equal(hh.bits(rp), hh.bits(hh.chains(model, cases, k)[s]))             # (the chains moved)
    if model != "sta":
        pads = hh.padded_slots(model, [sizes[int(s)] for s in d.buckets[0]], M, max(sizes), k)
        assert pads.any() == (name != "E") and np.array_equal(hh.bits(d.maps[0].P)[pads], hh.bits(start)[pads])
        assert not np.array_equal(hh.bits(d.maps[0].P)[~pads], hh.bits(start)[~pads])


@pytest.mark.parametrize("how", ["status", "value"])
@pytest.mark.parametrize("model", hh.MODELS)
def test_a_failed_chain_goes_dead_and_stays_dead(model, how):
    """From iteration 2 on the evaluator reports one chain as failed (status != 0, or a non-finite out[0]): the chain is frozen at its
    parameters, its history is -inf from there, and every other chain keeps the bits of the undisturbed run."""
    cases, k, row, first = cc.SET_A, 2, 3, 2

    def failing(ev):
        n = [0]

        def evaluate(P):
            out, grad, status = ev(P)
            if n[0] >= first:
                if how == "status":
                    status = status.copy()
                    status[row] = 7
                else:
                    out = out.copy()
                    out[row, 0] = np.inf
            n[0] += 1
            return out, grad, status

        return evaluate

    d0, _ = make(model, cases, k)
    clean = d0.run(ITERS)
    d1, _ = make(model, cases, k, failing)
    two = d1.run(first)                      # (the host loop goes on from where a run left it)
    rest = d1.run(ITERS - first)
    col = int(d1._rows(d1.buckets[0])[row])  # the caller's column of the bucket's row: chain j of subject s
    s, j = col // k, col % k
    others = np.arange(len(cases) * k) != col
    assert two[2].all() and not rest[2][col] and rest[2][others].all()
    assert np.all(np.isfinite(two[1])) and np.all(np.isneginf(rest[1][:, col]))
    hist = np.concatenate([two[1], rest[1]])
    assert np.array_equal(hh.bits(hist[:, others]), hh.bits(clean[1][:, others]))
    assert np.array_equal(hh.bits(hist[:first, col]), hh.bits(clean[1][:first, col]))
    for t in range(len(cases)):
        for c in range(k):
            same = np.array_equal(hh.bits(rest[0][t][c]), hh.bits(clean[0][t][c]))
            assert same == ((t, c) != (s, j)), (model, how, t, c)
    # the failed chain stands where iteration `first` found it
    assert np.array_equal(hh.bits(rest[0][s][j]), hh.bits(two[0][s][j]))


def test_signatures_and_symbols():
    new = ("device_resident", "iters_per_call", "evaluators")
    for model in hh.MODELS:
        cls = getattr(drivers, hm.DRIVER[model])
        init = inspect.signature(cls.__init__).parameters
        assert list(init)[:8] == ["self", "subjects", "hyper_pars", "init_pars", "lr", "chains_per_subject", "max_flop_waste", "ctxs"]
        assert all(n in init for n in new) and init["iters_per_call"].default == 50 and init["evaluators"].default is None
        assert isinstance(init["device_resident"].default, bool)
        assert list(inspect.signature(cls.run).parameters) == ["self", "N_opt", "callback"]
        assert list(inspect.signature(cls.predict).parameters) == ["self", "pars", "xs", "indx_star"]
        hmc = getattr(drivers, hh.DRIVER[model])
        assert list(inspect.signature(hmc.__init__).parameters) == [
            "self", "subjects", "hyper_pars", "init_positions", "step_size", "num_steps_in_leap", "seed", "mass", "step_jitter",
            "device_resident", "device_kinetic", "max_flop_waste", "ctxs", "evaluators"]
        assert inspect.signature(hmc.__init__).parameters["device_resident"].default is True
        assert list(inspect.signature(hmc.run).parameters) == ["self", "sample_size"] and hmc.MODEL == model and cls.MODEL == model
    with open(os.path.join(ROOT, "include", "nmgp.h")) as f:
        header = f.read()
    for name in ("nmgp_had_subjects_adam_begin", "nmgp_had_subjects_adam", "nmgp_had_subjects_adam_get_pars", "nmgp_had_subjects_adam_end"):
        assert name in _lib.SIGNATURES and re.search(r"\bint %s\(nmgp_ctx\* ctx" % name, header), name
    for name in ("had_subjects_adam_begin", "had_subjects_adam", "had_subjects_adam_get_pars", "had_subjects_adam_end"):
        assert callable(getattr(_lib.Context, name))
    cap = re.search(r"#define NMGP_HAD_ADAM_HIST_MAX \(1LL << (\d+)\)", header)             # the binding's copy of the header's cap
    assert cap and _lib.HAD_ADAM_HIST_MAX == 1 << int(cap.group(1))
    assert {m: v[2] for m, v in _lib.Context._COHORT_TRAJ_MODELS.items()} == hh.WIDTH


def test_device_resident_must_not_change_after_the_first_run():
    """Adam's moments and iteration count are not carried between the host loop and the device: a flipped switch is an error, not
    a silent restart."""
    d, _ = make("sta", cc.SET_D, 1)
    d.run(1)
    d.iters_per_call = 3                                    # (this one may change)
    d.run(1)
    d.device_resident = True
    with pytest.raises(RuntimeError, match="device_resident was changed"):
        d.run(1)
    d.device_resident = False
    assert d.run(1)[2].all()
