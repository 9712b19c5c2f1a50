"""Synthetic subjects and chains for the batched stationary (LMC) objective nmgp_sta_batch_eval (tests/test_sta_batch_cpu.py,
tests/test_gpu_sta_batch.py).  A plain module, not a conftest: both halves import it, so the CPU half checks the very subjects the GPU
half runs.  Subjects come from sim.simulate_stationary (one seed per shape), chains from sim.perturb (one phase per chain); the
references are the CPU oracle's nlogpos_obj_S, computed once per (shape, prior) and left read-only."""
import functools

import numpy as np

from conftest import STA_KEYS
from nonstationary_multivariate_gaussian_process_amd import sim

# (N, M): even and odd N (the two block-build kernels: 128 x 32 tiles with 16-byte stores / 64 x 64 tiles), the 64- and 128-wide tile
# edges (63 / 64 / 65, 127 / 128 / 129), more than one tile per workgroup column of the block build (per = ceil(ntl / 8)) and the
# stride-256 loop of the reduction's |alpha|^2 (257: 15 tiles, two per build column; the reduction's 128 column groups still hold one
# tile each up to N = 960 -- two tiles per group: tests/sta_objective_cases.py), every M instantiation 1 .. 8
SHAPES = [(1, 1), (2, 2), (8, 8), (63, 2), (64, 3), (65, 3), (127, 5), (128, 4), (129, 8), (200, 6), (257, 7)]
UNSORTED = (65, 3)                       # the shape of the subject with unsorted, unevenly spaced inputs
FD_SHAPES = [(8, 8), (65, 3), (127, 5)]  # the oracle's gradient against central differences
B_CHAINS = 4

HYPER = dict(sim.HYPER_STA)
HYPER_VEC = np.array([HYPER[k] for k in STA_KEYS])


def case_id(shape):
    return "N%d_M%d" % shape


@functools.lru_cache(maxsize=None)
def subject(N, M, unsorted=False):
    """(x [N], Y [N, M], generating parameters [T+3]), read-only.  unsorted: the inputs warped (uneven spacing) and shuffled, so that
    no kernel can rely on sorted or evenly spaced x."""
    d = sim.simulate_stationary(N, M, 100 * N + M)
    x, Y, p = d["x"], d["Y"], d["pars_true"].copy()
    if unsorted:
        perm = np.random.default_rng(7 * N + M).permutation(N)
        x, Y = (0.8 * x + 0.2 * x * x)[perm], Y[perm]
    x, Y = np.ascontiguousarray(x), np.ascontiguousarray(Y)
    for a in (x, Y, p):
        a.setflags(write=False)
    return x, Y, p


@functools.lru_cache(maxsize=None)
def chains(N, M, B=B_CHAINS, unsorted=False):
    """[B, T+3]: smooth perturbations of the subject's generating parameters, one phase per chain; read-only."""
    p = subject(N, M, unsorted)[2]
    P = np.stack([sim.perturb(p, 0.05, 0.3 + 0.45 * b) for b in range(B)])
    P.setflags(write=False)
    return P


@functools.lru_cache(maxsize=None)
def oracle(N, M, prior, unsorted=False, B=B_CHAINS):
    """(out [B, 5] or, without priors, [B, 1] = NegLog, grad [B, T+3]) of the CPU oracle for chains(N, M, B); read-only.  The reference
    raises for verbose=True with Prior=False, so the likelihood-only rows carry NegLog = -loglik alone."""
    from oracle import nmgp_oracle as O
    x, Y, _ = subject(N, M, unsorted)
    outs, grads = [], []
    for p in chains(N, M, B, unsorted):
        r, g = O.nlogpos_obj_S(p, Y, x, **HYPER, verbose=bool(prior), Prior=bool(prior), grad=True)
        outs.append(np.asarray(r, dtype=np.float64).reshape(-1))
        grads.append(np.asarray(g, dtype=np.float64))
    out, grad = np.stack(outs), np.stack(grads)
    out.setflags(write=False)
    grad.setflags(write=False)
    return out, grad


def singular_chain(good):
    """The singular parameters of the separable subject-set test (M = 3) in this model's layout, from a good chain [T+3]: row 1 of L
    zeroed (slots (1,0) = 0, (1,1) = exp(-800) = 0, (2,1) = 0: a zero row and column of B) and tilde_sigma2_err = -800 (sigma2 = 0):
    one block of the chain is the zero matrix."""
    p = np.array(good, dtype=np.float64, copy=True)
    assert p.shape[0] == 9, "written for M = 3"
    p[2 + 1], p[2 + 2], p[2 + 4] = 0.0, -800.0, 0.0
    p[-1] = -800.0
    return p


class NumpyStaContext:
    """A NumPy stand-in for the context under the stationary drivers: the batched entry answered by the CPU oracle, the subject set
    kept on the host.  What the drivers need and no more."""

    def __init__(self):
        self.x = self.Y = self.set = None
        self.calls = 0

    def set_data(self, x, Y):
        self.x, self.Y, self.set = np.asarray(x), np.asarray(Y), None
        self.N, self.M = self.Y.shape
        self.T = self.M * (self.M + 1) // 2

    def sta_batch_set_subjects(self, xs, Ys, chains_per_subject=1):
        self.set = (np.asarray(xs), np.asarray(Ys), int(chains_per_subject))

    def sta_batch_clear_subjects(self):
        self.set = None

    def sta_batch_eval(self, pars, hyper, prior=True, want_grad=False):
        from oracle import nmgp_oracle as O
        pars = np.atleast_2d(np.asarray(pars, dtype=np.float64))
        h = dict(zip(STA_KEYS, (float(v) for v in hyper)))
        if self.set is not None and pars.shape[0] != self.set[0].shape[0] * self.set[2]:
            raise ValueError("B does not fit the subject set")
        self.calls += 1
        out, grad = np.empty((pars.shape[0], 5)), np.empty_like(pars)
        for b, p in enumerate(pars):
            x, Y = (self.x, self.Y) if self.set is None else (self.set[0][b // self.set[2]], self.set[1][b // self.set[2]])
            r, g = O.nlogpos_obj_S(p, Y, x, **h, verbose=True, Prior=bool(prior), grad=True)
            out[b], grad[b] = np.asarray(r, dtype=np.float64), g
        return out, (grad if want_grad else None), np.zeros(pars.shape[0], dtype=np.int32)
