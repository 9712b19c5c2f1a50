"""Helpers of the cohort HMC tests (tests/test_hadamard_cohort_hmc_cpu.py, tests/test_gpu_hadamard_cohort_hmc.py): the three Hadamard
models ("non", "sep", "sta") on the subject sets A-E of tests/hadamard_cohort_cases.py, with the pack / unpack / reference helpers of
that module and of tests/hadamard_cohort_model_cases.py.  A plain module, not a conftest.  The arrays are shared: do not write into
them."""
import numpy as np

import hadamard_cases as hc
import hadamard_cohort_cases as cc
import hadamard_cohort_model_cases as mc

MODELS = ("non", "sep", "sta")
PARS = {"non": "had", "sep": "sep", "sta": "sta"}          # the model's name in tests/hadamard_cases.py
ENTRY = {"non": "had_subjects_eval", "sep": "hads_subjects_eval", "sta": "hadst_subjects_eval"}
WIDTH = {"non": 5, "sep": 6, "sta": 5}
DRIVER = {"non": "HadamardCohortHMC", "sep": "HadamardSepCohortHMC", "sta": "HadamardStaCohortHMC"}
PER_SUBJECT = {"non": "BatchedHMCHadamard", "sep": "BatchedHMCHadamardSep", "sta": "BatchedHMCHadamardSta"}
PREDICT = {"non": "posterior_predict_hadamard_cohort", "sep": "posterior_predict_hadamard_sep_cohort",
           "sta": "posterior_predict_hadamard_sta_cohort"}


def plen(model, Nmax, M):
    T = M * (M + 1) // 2
    return Nmax * (1 + T) + 1 if model == "non" else mc.plen(model, Nmax, M)


def nmax_of(model, Pmax, M):
    """the Nmax a padded row of width Pmax belongs to (None for the stationary model, whose rows have no padding)"""
    T = M * (M + 1) // 2
    return None if model == "sta" else (Pmax - 1) // (1 + T) if model == "non" else (Pmax - T - 1) // 2


def chains(model, cases, k):
    """per subject [k, P_s]: the first k chains of c["pars"]"""
    return [c["pars"][PARS[model]][:k] for c in cc.subjects(cases)]


def pack(model, vectors, sizes, M, Nmax=None, fill=0.0):
    return cc.pack(vectors, sizes, M, Nmax=Nmax, fill=fill) if model == "non" else mc.pack(model, vectors, sizes, M, Nmax=Nmax, fill=fill)


def unpack(model, P, sizes, M, k):
    if model == "non":
        from nonstationary_multivariate_gaussian_process_amd import hadamard
        return hadamard.cohort_unpack(P, sizes, M, k)
    return mc.unpack(model, P, sizes, M, k)


def padded_slots(model, sizes, M, Nmax, k=1):
    return cc.padded_slots(sizes, M, Nmax, k) if model == "non" else mc.padded_slots(model, sizes, M, Nmax, k)


def hyper_of(model, cases):
    return hc.build(cases[0])["hyper"][PARS[model]]


def hyper_dict(model, cases):
    """the hyper-parameters as the drivers take them (a dict by the model's keys)"""
    from nonstationary_multivariate_gaussian_process_amd import drivers
    keys = {"non": drivers.SVC_HYPER_KEYS, "sep": drivers.SEP_HYPER_KEYS, "sta": drivers.STA_HYPER_KEYS}[model]
    return dict(zip(keys, hyper_of(model, cases)))


def real_slot(model, i, Nmax, Ns, T):
    """The layouts' masks as the device states them (real_slot of CohNon / CohSep / CohSta), restated: whether slot i of a padded row
    of a subject with Ns observations is real."""
    if model == "sta":
        return True
    if model == "sep":
        return i < Ns if i < Nmax else (i - Nmax < Ns if i < 2 * Nmax else True)
    return i < Ns if i < Nmax else (i - Nmax < Ns * T if i < Nmax * (1 + T) else True)


def subject_triples(cases):
    return [(c["x"], c["indx"], c["y"]) for c in cc.subjects(cases)]


def eps_of(S):
    """distinct per subject and small enough that every chain stays valid: a test input, not a tuned figure"""
    return 1e-3 / (1.0 + np.arange(S))


def diag_mass(model, cases):
    """per subject diag(M) [P_s]: smooth, positive, away from 1; a function of the subject alone (not of its place in the list)"""
    return [0.5 + 1.5 * (0.5 + 0.5 * np.sin(0.37 * np.arange(v.shape[1]) + 0.01 * v.shape[1])) for v in chains(model, cases, 1)]


def momenta(model, cases, k, seed, Nmax=None, fill=0.0):
    """[S k, Pmax]: standard normals of the real length in the real slots (a stream per row), `fill` in the padded ones"""
    rows = [np.stack([np.random.default_rng(seed + s * k + j).standard_normal(v.shape[1]) for j in range(k)])
            for s, v in enumerate(chains(model, cases, k))]
    return pack(model, rows, cc.nobs(cases), cases[0][1], Nmax=Nmax, fill=fill)


def reference_evaluator(model, cases, k):
    """padded rows -> (out, grad, status) from the NumPy restatement on each subject alone, scattered into the padded layout with +0.0
    gradients in the padded slots (what ``evaluators=`` of the cohort drivers takes)"""
    sizes, M, subs = cc.nobs(cases), cases[0][1], cc.subjects(cases)

    def evaluate(P):
        outs, grads = [], []
        for c, rows in zip(subs, unpack(model, P, sizes, M, k)):
            res = [hc.ref_logpos(PARS[model], np.array(r), c, True, grad=True) for r in rows]
            outs += [np.asarray(r[0], dtype=np.float64) for r in res]
            grads.append(np.stack([np.asarray(r[1], dtype=np.float64) for r in res]))
        return np.stack(outs), pack(model, grads, sizes, M, Nmax=nmax_of(model, P.shape[1], M)), np.zeros(len(outs), dtype=np.int32)

    return evaluate


def subject_evaluator(model, case):
    """[B, P_s] -> (U [B], grad [B, P_s]) of the restatement on one subject: ``LockStepHMC.potential_and_grad``"""
    c = hc.build(case)

    def potential_and_grad(q):
        res = [hc.ref_logpos(PARS[model], np.array(r), c, True, grad=True) for r in q]
        return np.array([float(r[0][0]) for r in res]), np.stack([np.asarray(r[1], dtype=np.float64) for r in res])

    return potential_and_grad


def workspace_per_chain(model, Nmax, M):
    """bytes of device workspace per chain of a cohort evaluation with gradients ("Hadamard models, many subjects")"""
    if model != "non":
        return mc.workspace_per_chain(model, Nmax, M)
    T = M * (M + 1) // 2
    ev = lambda n: (n + 1) // 2 * 2
    N, P = Nmax, plen(model, Nmax, M)
    ld = (2 * N + 2 + 15) // 16 * 16
    n = ev(P) + ev(N) + 16 + ev(1) + ld * N + ev(N) + ev(N * M) + 2 * ev(N * (1 + T)) + ev(1 + T)
    n += ev(N) + ev(N * N) + ev(max(-(-N // 64) * N * (M + 1), N * -(-N // 256))) + ev(P) + 2
    return 8 * n


def chunks_under_cap(model, Nmax, M, S, cps, cap_gb):
    if model != "non":
        return mc.chunks_under_cap(model, Nmax, M, S, cps, cap_gb)
    B = S * cps
    Bc = min(B, int(cap_gb * 1e9 // workspace_per_chain(model, Nmax, M)), 65535)
    assert Bc >= 1
    if cps > Bc:
        return S * -(-cps // Bc)
    return -(-B // (Bc // cps * cps))


def host_trajectory(evaluate, mask, q0, U0, g0, eps_rows, nsteps, p0, minv=None):
    """The host loop's arithmetic, written out over an evaluation of padded rows (``evaluate(P) -> (out, grad, status)``): a kick
    ``t = (kick eps) g; p = p - t`` on the real slots of chains whose gradient is defined, a drift ``v = minv p; q = q + eps v`` on
    the real slots of all chains, padded momentum +0.0, padded positions as they are.  Returns q1, p1, U1 (inf where failed), failed."""
    def potential(P):
        out, g, status = evaluate(P)
        U = np.array(out[:, 0])
        bad = (status != 0) | ~np.isfinite(U)
        U[bad] = np.inf
        g[bad] = 0.0
        return U, g

    e = np.asarray(eps_rows)[:, None]
    q1, g, U1 = q0.copy(), g0, U0
    failed = ~np.isfinite(U0)
    with np.errstate(invalid="ignore", over="ignore"):
        p1 = np.where(mask, p0 - (0.5 * e) * g, 0.0)
        for step in range(nsteps):
            v = p1 if minv is None else minv * p1
            q1 = np.where(mask, q1 + e * v, q1)
            U1, g = potential(q1)
            failed |= ~np.isfinite(U1)
            p1 = np.where(mask, p1 - (e if step < nsteps - 1 else 0.5 * e) * g, p1)
    return q1, p1, np.where(failed, np.inf, U1), failed


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_real_bits(a, b, mask):
    """bit identity of two padded arrays on the real slots"""
    return a.shape == b.shape and np.array_equal(bits(a)[mask], bits(b)[mask])
