"""Helpers of the cohort tests of the separable ("sep") and stationary ("sta") Hadamard models (tests/test_hadamard_cohort_models_cpu.py,
tests/test_gpu_hadamard_cohort_models.py) on the subject sets of tests/hadamard_cohort_cases.py: the two models' layouts, chains and
references.  A plain module, not a conftest.  The arrays are shared: do not write into them."""
import numpy as np

import hadamard_cases as hc
import hadamard_cohort_cases as cc

MODELS = ("sep", "sta")
ENTRY = {"sep": "hads_subjects_eval", "sta": "hadst_subjects_eval"}
RESIDENT = {"sep": "hads_batch_eval", "sta": "hadst_batch_eval"}
WIDTH = {"sep": 6, "sta": 5}


def plen(model, Nmax, M):
    T = M * (M + 1) // 2
    return 2 * Nmax + T + 1 if model == "sep" else T + 3


def chains(model, cases, k):
    """per subject [k, P_s]: chain 0 (and chain 1) of c["pars"][model]"""
    return [c["pars"][model][:k] for c in cc.subjects(cases)]


def pack(model, vectors, sizes, M, Nmax=None, fill=0.0):
    """the rows the model's cohort entry takes: the separable padded layout, or the stationary vectors stacked as they are"""
    if model == "sta":
        return np.concatenate([np.atleast_2d(v) for v in vectors], axis=0)
    from nonstationary_multivariate_gaussian_process_amd import hadamard_sep
    return hadamard_sep.cohort_pack(vectors, sizes, M, Nmax=Nmax, fill=fill)


def unpack(model, P, sizes, M, k):
    if model == "sta":
        return [P[s * k:(s + 1) * k] for s in range(len(sizes))]
    from nonstationary_multivariate_gaussian_process_amd import hadamard_sep
    return hadamard_sep.cohort_unpack(P, sizes, M, chains_per_subject=k)


def padded_slots(model, sizes, M, Nmax, k=1):
    """boolean [S k, P]: True in the padded slots (none for the stationary model)"""
    mask = np.zeros((len(sizes) * k, plen(model, Nmax, M)), dtype=bool)
    if model == "sep":
        for s, n in enumerate(sizes):
            rows = mask[s * k:(s + 1) * k]
            rows[:, n:Nmax] = True
            rows[:, Nmax + n:2 * Nmax] = True
    return mask


def hyper_of(model, cases):
    return hc.build(cases[0])["hyper"][model]


def reference(model, case, chain, prior):
    """(verbose tuple, d NegLog / d pars) of the restatement on the subject alone; computed once, shared, left unchanged"""
    return hc.reference(model, case, chain, prior)


def workspace_per_chain(model, Nmax, M, want_grad=True):
    """Bytes of device workspace per chain of a cohort call as INTEGRATION.md ("Hadamard models, many subjects") states them: the
    factorisation buffer of ld columns-of-Nmax with ld = the rows (Nmax + 1, or 2 Nmax + 2 with gradients) rounded up to 16, with
    gradients Nmax^2 for -S^-1 and ceil(Nmax / 64) Nmax (M + 2) adjoint partial rows, and the vectors: P, z, 16 scalars, the status
    word, (sep) ell, sig, Rv, the two prior columns and their two norms, with gradients (sep) the prior gradients and the summed row
    components, alpha, the gradient and the two trace terms.  Every piece is rounded up to an even number of doubles."""
    T = M * (M + 1) // 2
    ev = lambda n: (n + 1) // 2 * 2
    N, P = Nmax, plen(model, Nmax, M)
    ld = ((2 * N + 2 if want_grad else N + 1) + 15) // 16 * 16
    n = ev(P) + ev(N) + 16 + ev(1) + ld * N
    if model == "sep":
        n += 2 * ev(N) + ev(N * M) + ev(2 * N) + 2
        if want_grad:
            n += ev(2 * N) + ev(N * M)
    if want_grad:
        n += ev(N) + ev(N * N) + ev(max(-(-N // 64) * N * (M + 2), N * -(-N // 256))) + ev(P) + 2
    return 8 * n


def chunks_under_cap(model, Nmax, M, S, cps, cap_gb):
    """the number of chunks the entry's rule gives: floor(cap / per chain) chains, at most B and 65535; whole subjects when a
    subject's chains fit, parts of ONE subject's chains otherwise"""
    B = S * cps
    Bc = min(B, int(cap_gb * 1e9 // workspace_per_chain(model, Nmax, M)), 65535)
    assert Bc >= 1
    if cps > Bc:
        return S * -(-cps // Bc)
    return -(-B // (Bc // cps * cps))
