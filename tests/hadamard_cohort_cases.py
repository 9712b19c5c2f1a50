"""The subject sets of the Hadamard cohort tests (tests/test_hadamard_cohort_cpu.py, tests/test_gpu_hadamard_cohort.py): ragged subjects
of tests/hadamard_cases.py grouped by M.  A plain module, not a conftest: both halves import it, so the CPU half checks the very subjects
the GPU half runs.  The arrays are shared: do not write into them."""
import functools

import numpy as np

import hadamard_cases as hc

# nobs = [128, 63, 2, 64, 65, 127]: N_s = Nmax, a mask inside a tile, N_s = M, masks starting on and one past a tile edge, the last row
# alone padded
SET_A = [(128, 2, "interleaved"), (63, 2, "blocks"), (2, 2, "interleaved"), (64, 2, "rare_last"), (65, 2, "unsorted"),
         (127, 2, "rare_first")]
SET_B = [(193, 8, "blocks"), (8, 8, "interleaved"), (130, 8, "unsorted")]
SET_C = [hc.WIDE, hc.MINOR, (256, 3, "blocks"), (3, 3, "interleaved")]
SET_D = [(1, 1, "interleaved"), (2, 1, "interleaved"), (70, 1, "unsorted")]
SET_E = [(64, 5, "rare_last"), (64, 5, "blocks")]                      # no padding
SETS = {"A": SET_A, "B": SET_B, "C": SET_C, "D": SET_D, "E": SET_E}

# the subjects the sweep's table does not hold: the CPU half checks their preconditions
NEW_SUBJECTS = [(64, 2, "rare_last"), (65, 2, "unsorted"), (127, 2, "rare_first"), (130, 8, "unsorted"), (256, 3, "blocks"),
                (3, 3, "interleaved"), (2, 1, "interleaved"), (70, 1, "unsorted"), (64, 5, "blocks")]


def subjects(cases):
    return [hc.build(case) for case in cases]


def nobs(cases):
    return [case[0] for case in cases]


def pack(vectors, sizes, M, Nmax=None, fill=0.0):
    from nonstationary_multivariate_gaussian_process_amd import hadamard
    return hadamard.cohort_pack(vectors, sizes, M, Nmax=Nmax, fill=fill)


def chains(cases, k):
    """per subject [k, P_s]: chain 0 (and chain 1) of c["pars"]["had"]"""
    return [c["pars"]["had"][:k] for c in subjects(cases)]


@functools.lru_cache(maxsize=None)
def reference(case, chain, prior):
    """(verbose tuple, d NegLog / d pars) of the restatement on the subject alone; computed once, shared, left unchanged"""
    c = hc.build(case)
    return hc.ref_logpos("had", c["pars"]["had"][chain], c, prior, grad=True)


def padded_slots(sizes, M, Nmax, k=1):
    """boolean [S k, Pmax]: True in the padded slots of the padded layout"""
    T = M * (M + 1) // 2
    mask = np.ones((len(sizes) * k, Nmax * (1 + T) + 1), dtype=bool)
    for s, n in enumerate(sizes):
        rows = mask[s * k:(s + 1) * k]
        rows[:, :n] = False
        rows[:, Nmax:Nmax + n * T] = False
        rows[:, -1] = False
    return mask
