"""Helpers of the cohort MAP tests (tests/test_hadamard_cohort_map_cpu.py, tests/test_gpu_hadamard_cohort_map.py): the host loop --
drivers.LockStepMAP over an evaluation of padded rows -- with the history the resident optimiser returns, on the models, sets and
pack / unpack helpers of tests/hadamard_cohort_hmc_cases.py.  A plain module, not a conftest.  The arrays are shared: do not write
into them."""
import numpy as np

import hadamard_cases as hc
import hadamard_cohort_hmc_cases as hh

DRIVER = {"non": "HadamardCohortMAP", "sep": "HadamardSepCohortMAP", "sta": "HadamardStaCohortMAP"}
PER_SUBJECT = {"non": "HadamardMAP", "sep": "HadamardSepMAP", "sta": "HadamardStaMAP"}
LR = 2e-2            # a test input: small enough that every good chain of sets A - I stays valid for the few iterations of a test


def subject_evaluator(model, case):
    """[B, P_s] -> (out [B, W], grad [B, P_s], status [B]) of the restatement on one subject: ``LockStepMAP.value_and_grad``"""
    c = hc.build(case)

    def value_and_grad(P):
        res = [hc.ref_logpos(hh.PARS[model], np.array(r), c, True, grad=True) for r in P]
        return (np.stack([np.asarray(r[0], dtype=np.float64) for r in res]), np.stack([np.asarray(r[1], dtype=np.float64) for r in res]),
                np.zeros(len(res), dtype=np.int32))

    return value_and_grad


def host_loop(evaluate, P0, niters, lr=LR):
    """``niters`` iterations of drivers.LockStepMAP from the padded rows P0 over ``evaluate(P) -> (out, grad, status)``.  Returns what
    ``had_subjects_adam`` returns for the same iterations -- out_hist [niters, B, W] with NaN rows for the chains that are not alive
    after the iteration's evaluation, alive [B] -- and the parameters [B, Pmax], the per-iteration alive [niters, B] and the
    driver's history [niters, B] = -NegLog (-inf for a dead chain)."""
    from nonstationary_multivariate_gaussian_process_amd import drivers
    m = drivers.LockStepMAP(P0, lr=lr)
    m.value_and_grad = evaluate
    rows, alive = [], []

    def keep(i, h, out):
        rows.append(np.where(m.alive[:, None], out, np.nan))
        alive.append(m.alive.copy())

    with np.errstate(invalid="ignore", over="ignore"):          # (padded slots may hold anything; a chain may be driven out on purpose)
        P, hist, last = m.run(niters, keep)
    return np.stack(rows), last, P, np.stack(alive), hist


def same_hist(a, b):
    """two histories of verbose tuples: NaN in the same places, the same bits elsewhere"""
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(hh.bits(a)[~na], hh.bits(b)[~nb])
