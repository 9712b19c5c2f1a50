"""The subject sets of the Hadamard cohort tests (tests/test_hadamard_cohort_cpu.py, tests/test_gpu_hadamard_cohort.py): ragged subjects
of tests/hadamard_cases.py grouped by M.  A plain module, not a conftest: both halves import it, so the CPU half checks the very subjects
the GPU half runs.  The arrays are shared: do not write into them.

Sets A - E carry M = 2, 8, 3, 1, 5.  Sets F - H add M = 4, 6, 7, whose M-templated cohort kernels (k_hadc_cov / k_hadc_adjoint with AMP
on and off, k_hadcst_cov / k_hadcst_adjoint, the three k_*_cross_rows) no other set launches: their staging loops
`for (k = tid; k < 64 M; k += 256)` take one exact pass at M = 4 and a ragged second pass at M = 6 and 7, with the mask g < N_s M
cutting through.  F: Nmax = 129 is odd and the last tile holds a single row; G: Nmax = 192 is a multiple of 64; H: Nmax = 257 > 256 with
a ragged fifth tile.  (65, 6, rare_first) and (129, 7, unsorted) are subjects of the resident sweep too.  Sets F - H join every
parametrisation over SETS.

Set I (M = 2, Nmax = 1030) is the cohort's own workload size: k_hadc_trace's stride-1024 loop takes a second pass from N_s = 1025, the
batched factorisation leaves its single 512-column panel, the identity-padded tail of a short subject runs through a second panel, the
gradient path carries 2 Nmax + 2 > 2048 riding rows, and every subject ends inside a different tile.  Its CPU references take seconds,
so it is kept out of SETS and runs with one chain per subject in a few tests only: parity of the three objective entries and of the
three predictors, "padding is inert", and one two-step trajectory against the host loop.

The gradients are held block by block: the rule and its CPU figures are in tests/hadamard_cases.py (block_bar)."""
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
SET_F = [(4, 4, "interleaved"), (64, 4, "rare_first"), (65, 4, "blocks"), (129, 4, "unsorted"), (100, 4, "rare_last")]
SET_G = [(65, 6, "rare_first"), (6, 6, "unsorted"), (128, 6, "blocks"), (127, 6, "interleaved"), (192, 6, "rare_last")]
SET_H = [(129, 7, "unsorted"), (7, 7, "interleaved"), (63, 7, "rare_last"), (257, 7, "blocks"), (130, 7, "rare_first")]
SET_I = [(1030, 2, "unsorted"), (1025, 2, "blocks"), (513, 2, "rare_last"), (640, 2, "interleaved")]
SETS = {"A": SET_A, "B": SET_B, "C": SET_C, "D": SET_D, "E": SET_E, "F": SET_F, "G": SET_G, "H": SET_H}
LARGE_SETS = {"I": SET_I}                                              # one chain per subject, in the tests the docstring names
ALL_SETS = dict(SETS, **LARGE_SETS)

# the subjects the sweep's table does not hold: the CPU half checks their preconditions
SWEEP_SUBJECTS = [(4, 4, "interleaved"), (64, 4, "rare_first"), (65, 4, "blocks"), (129, 4, "unsorted"), (100, 4, "rare_last"),
                  (6, 6, "unsorted"), (128, 6, "blocks"), (127, 6, "interleaved"), (192, 6, "rare_last"),
                  (7, 7, "interleaved"), (63, 7, "rare_last"), (257, 7, "blocks"), (130, 7, "rare_first")] + SET_I
NEW_SUBJECTS = [(64, 2, "rare_last"), (65, 2, "unsorted"), (127, 2, "rare_first"), (130, 8, "unsorted"), (256, 3, "blocks"),
                (3, 3, "interleaved"), (2, 1, "interleaved"), (70, 1, "unsorted"), (64, 5, "blocks")] + SWEEP_SUBJECTS


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


def reference(case, chain, prior):
    """(verbose tuple, d NegLog / d pars) of the restatement on the subject alone; computed once, shared, left unchanged"""
    return hc.reference("had", case, chain, prior)


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
