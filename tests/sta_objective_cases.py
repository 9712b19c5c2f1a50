"""Cases, references, bars and the restated arithmetic of the stationary (LMC) objective sweep in the default (Cholesky) formulation
(tests/test_sta_objective_cpu.py, tests/test_gpu_sta_objective.py).  A plain module, not a conftest: both halves import it, so the CPU
half checks the very subjects, chains and reference values the GPU half runs against.  No GPU result enters a reference or a bar.

The entries: nmgp_logpos_sta and nmgp_sta_batch_eval under NMGP_SEP=chol (the default), that is sta_batch_core (nmgp_eig.hip):
k_sta_prep_b, k_sta_blocks_b4 (even N) / k_sta_blocks_b (odd N), the batched factorisation with the substitution-based panels,
k_tri_gemv_part, the inverse SYRK, k_sta_reduce_b and the host epilogue.

Shapes.  sta_batch_cases.SHAPES unchanged (four chains each, reference: their CPU oracle), and
  (34, 1)     k_sta_blocks_b4: a second 32-column tile of two columns; the M = 1 template
  (126, 7)    one 128-row tile less a row pair; N M = 882
  (130, 5)    a second row tile of one pair; column J = 4 begins at row tile I = 1
  (258, 2)    a third row tile of one pair; k_tri_gemv_part's first ragged 256 block on even N
  (961, 1)    k_sta_reduce_b with NI = 16, ntl = 136, per = 2: 68 live column groups, each of two tiles.  Tile columns begin at
              t = 0, 16, 31, 45, 58, 70, 81, 91, 100, 108, 115, 121, 126, 130, 133, 135; a group (2 cg, 2 cg + 1) changes column
              mid-walk where a column begins at an odd t: groups 15, 22, 40, 45, 57, 60, 66 and 67 (into columns 2, 3, 6, 7, 10, 11, 14, 15);
              the other 60 walk down within a column.  The odd-N block build with per = ceil(136 / 8) = 17
  (1026, 2)   NI = 17, ntl = 153, per = 2: 77 live groups, the last (cg = 76) holds the single tile 152 (the t1 clamp).  Columns begin at
              0, 17, 33, 48, 62, 75, 87, 98, 108, 117, 125, 132, 138, 143, 147, 150, 152: groups 8, 16, 37, 43, 58, 62, 71 and 73 change
              column (into columns 1, 2, 5, 6, 9, 10, 13, 14).  The even-N build with NI = 9 row tiles, NJ = 33 column tiles
(tile_walk below mirrors the kernel's index arithmetic; the CPU half asserts these lists.)  The two large shapes run chains 0 and 1.
Variants of a shape: "unsorted" (sta_batch_cases' warped and shuffled subject at (65, 3)) and "s1", "s2" (the further subjects of
a subject set, sim.simulate_stationary with other seeds).

References (eig_objective_cases.ref for the plain cases): the CPU oracle where sta_batch_cases holds the case; else the dense
restatement sep_restated on the vector expanded to constant curves, np.longdouble while N M <= 1000 and float64 above, the prior
part the oracle's own g(prior) - g(no prior)."""
import functools

import numpy as np

import eig_objective_cases as E
import objective_cases as OC
import sta_batch_cases as SC
from nonstationary_multivariate_gaussian_process_amd import sim

LIK_TIGHT, GRAD_TIGHT = OC.LIK_TIGHT, OC.GRAD_TIGHT
RESTATED_LIK, RESTATED_BLOCK = LIK_TIGHT / 10, GRAD_TIGHT / 10      # what the CPU half holds sta_restated to
REFERENCE_FLOOR = 1e-9                   # two CPU references further apart than this on a block: an entry of BLOCK_BARS
JITTER = 1e-6                            # NMGP_JITTER, on K_x's diagonal
G = 128                                  # NMGP_SEP_TR_G: the column groups of k_sta_reduce_b
TILE = 64

NEW_SHAPES = [(34, 1), (126, 7), (130, 5), (258, 2), (961, 1), (1026, 2)]
LARGE_SHAPES = [(961, 1), (1026, 2)]
SHAPES = list(SC.SHAPES) + NEW_SHAPES
UNSORTED = SC.UNSORTED                   # (65, 3)
SET_SHAPES = [(65, 3), (130, 5)]         # subject sets: SUBJECTS x CHAINS_PER_SUBJECT
SUBJECTS, CHAINS_PER_SUBJECT = 3, 2
HYPER_VEC = SC.HYPER_VEC

# (model, N, M, block name) -> bar.  The rule: an entry exists only where the CPU half itself measures two CPU references (the CPU
# oracle and the dense restatement) more than REFERENCE_FLOOR apart on a block (tests/test_sta_objective_cpu.py asserts that for
# every entry below, at the 16 BLAS threads the figures are documented for).  The first three are eig_objective_cases.BLOCK_BARS'
# entries for these chains (measured values: there).  In np.longdouble (N M <= 1000) no further block is 1e-9 apart.  With both
# references in float64 the figures move with the BLAS thread count, as that module found; as there, an entry is ten times the
# worst of 1, 4, 8 and 16 threads, rounded up -- but a block that is over the floor at some other thread count only gets none.
BLOCK_BARS = dict(E.BLOCK_BARS)
BLOCK_BARS.update({
    # (257, 7), N M = 1799: the oracle against the float64 dense restatement, as for this shape's sigma2 entry above
    ("sta", 257, 7, "tilde_l"): 3e-8,           # 16 threads: 1.27e-9 (chain 2); 2.16e-9 (chain 3), 4.4e-10, 1.27e-9 with 1, 4, 8
    ("sta", 257, 7, "tilde_sigma"): 3e-8,       # 16 threads: 2.25e-9 (chain 1); 1.28e-9, 1.66e-9, 2.25e-9 with 1, 4, 8
    # (1026, 2), N M = 2052: the oracle against the float64 dense restatement, this case's reference
    ("sta", 1026, 2, "tilde_sigma"): 7e-8,      # 16 threads: 4.67e-9 (chain 0); 6.56e-9, 3.42e-9, 4.67e-9 with 1, 4, 8
    # ((1026, 2) uL_vec: 4.9e-10 at 8 and 16 threads, 8.5e-10 at 1, 1.14e-9 at 4 only: no entry)
})

n_slots = OC.n_slots


def case_id(case):
    """case: (N, M) or (N, M, variant)."""
    return "N%d_M%d" % tuple(case[:2]) + ("_" + case[2] if len(case) > 2 and case[2] else "")


def n_chains(N, M, variant=""):
    if variant:
        return CHAINS_PER_SUBJECT if variant.startswith("s") else SC.B_CHAINS
    return 2 if (N, M) in LARGE_SHAPES else SC.B_CHAINS


def batch(N, M):
    return 2 if (N, M) in LARGE_SHAPES else 3


def all_cases():
    """[(N, M, variant)]: every shape, then the unsorted subject."""
    return [(N, M, "") for N, M in SHAPES] + [UNSORTED + ("unsorted",)]


def set_cases():
    """[(N, M, variant)] of the subjects of the subject sets, subject 0 included."""
    return [(N, M, "" if s == 0 else "s%d" % s) for N, M in SET_SHAPES for s in range(SUBJECTS)]


@functools.lru_cache(maxsize=None)
def _further_subject(N, M, s):
    d = sim.simulate_stationary(N, M, 100 * N + M + 1000 * s)
    x, Y, p = np.ascontiguousarray(d["x"]), np.ascontiguousarray(d["Y"]), d["pars_true"].copy()
    for a in (x, Y, p):
        a.setflags(write=False)
    return x, Y, p


def subject(N, M, variant=""):
    """(x [N], Y [N, M], generating parameters [T + 3]), read-only."""
    if variant == "unsorted":
        return SC.subject(N, M, True)
    if variant:
        return _further_subject(N, M, int(variant[1:]))
    return SC.subject(N, M)


@functools.lru_cache(maxsize=None)
def chains(N, M, variant=""):
    """[n_chains, T + 3], read-only: sta_batch_cases' perturbations of the subject's generating parameters."""
    if variant == "unsorted":
        return SC.chains(N, M, SC.B_CHAINS, True)
    if not variant:
        return SC.chains(N, M)[:n_chains(N, M)]
    P = np.stack([sim.perturb(subject(N, M, variant)[2], 0.05, 0.3 + 0.45 * b) for b in range(CHAINS_PER_SUBJECT)])
    P.setflags(write=False)
    return P


# ---------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------
def dense_dtype(N, M):
    return E.dense_dtype(N, M)


_DENSE, _ORACLE, _REF = {}, {}, {}


def dense(N, M, k, variant=""):
    """(loglik, d(-loglik)/d pars [T + 3]) of the dense restatement on constant curves; computed once."""
    if not variant:
        return E.dense("sta", N, M, k)
    key = (N, M, k, variant)
    if key not in _DENSE:
        from test_objective_sweep_cpu import sep_restated
        x, Y, _ = subject(N, M, variant)
        ll, g = sep_restated(E.sta_to_sep(chains(N, M, variant)[k], N), Y, x, dense_dtype(N, M))
        g = np.asarray(E.sep_grad_to_sta(g, N), dtype=np.float64)
        g.setflags(write=False)
        _DENSE[key] = (float(ll), g)
    return _DENSE[key]


def oracle(N, M, k, prior, variant=""):
    """(out, grad) of the CPU oracle: out = [NegLog, loglik] without the priors, the five verbose values with them; computed once."""
    key = (N, M, k, bool(prior), variant)
    if key not in _ORACLE:
        if variant == "unsorted" or (not variant and (N, M) in SC.SHAPES):
            o, gs = SC.oracle(N, M, bool(prior), variant == "unsorted")
            r, g = (o[k] if prior else np.array([o[k][0], -o[k][0]])), gs[k]
        else:
            from oracle import nmgp_oracle as O
            x, Y, _ = subject(N, M, variant)
            r, g = O.nlogpos_obj_S(chains(N, M, variant)[k], Y, x, **SC.HYPER, verbose=bool(prior), Prior=bool(prior), grad=True)
            r = np.asarray(r, dtype=np.float64).reshape(-1)
            r = r if prior else np.array([r[0], -r[0]])
        r, g = np.array(r, dtype=np.float64), np.array(g, dtype=np.float64)
        r.setflags(write=False)
        g.setflags(write=False)
        _ORACLE[key] = (r, g)
    return _ORACLE[key]


def has_oracle_case(N, M, variant=""):
    return variant == "unsorted" or (not variant and (N, M) in SC.SHAPES)


def ref(N, M, k, prior, variant=""):
    """(out, grad) the device is held to, read-only: out[0] NegLog, out[1] loglik, out[2:] the verbose components (priors on only)."""
    if not variant:
        return E.ref("sta", N, M, k, prior)
    key = "%d,%d,%s,%d,%s" % (N, M, k, bool(prior), variant)
    if key not in _REF:
        if has_oracle_case(N, M, variant):
            r, g = oracle(N, M, k, prior, variant)
        else:
            ll, g0 = dense(N, M, k, variant)
            if prior:
                (r, g1), (_, go0) = oracle(N, M, k, True, variant), oracle(N, M, k, False, variant)
                g = g0 + (g1 - go0)
            else:
                r, g = np.array([-ll, ll]), g0
        r, g = np.array(r, dtype=np.float64), np.array(g, dtype=np.float64)
        r.setflags(write=False)
        g.setflags(write=False)
        _REF[key] = (r, g)
    return _REF[key]


def refs(case, ks=None):
    """[{prior: (out, grad)}] for the chains ks of the case: the `refs` of hold_sta_to_oracle."""
    N, M, variant = case
    ks = range(n_chains(N, M, variant)) if ks is None else ks
    return [{p: ref(N, M, k, p, variant) for p in (False, True)} for k in ks]


def save_refs(path):
    """The references computed so far, for a child process that runs the same cases (load_refs)."""
    arrays = {}
    for tag, table in (("E", E._REF), ("S", _REF)):
        for key, (r, g) in table.items():
            arrays["out:%s:%s" % (tag, key)], arrays["grad:%s:%s" % (tag, key)] = r, g
    np.savez(path, **arrays)


def load_refs(path):
    d = np.load(path)
    for name in d.files:
        if name.startswith("out:"):
            r, g = d[name], d["grad:" + name[4:]]
            r.setflags(write=False)
            g.setflags(write=False)
            (E._REF if name[4] == "E" else _REF).setdefault(name[6:], (r, g))


def blocks_over_bar(g, gref, layout):
    return OC.blocks_over_bar(g, gref, layout, GRAD_TIGHT, BLOCK_BARS)


# ---------------------------------------------------------------------------------------------------
# the tile walk of k_sta_reduce_b
# ---------------------------------------------------------------------------------------------------
def tile_walk(N, groups=G):
    """[[(I, J)]] per column group cg: the 64 x 64 tiles of the lower triangle that k_sta_reduce_b gives it, by the kernel's own index
    arithmetic: per = ceil(ntl / G), t0 = cg per, t1 = min(t0 + per, ntl), (I, J) located from t0 by walking the columns, then
    ++I >= NI -> ++J, I = J."""
    NI = (N + TILE - 1) // TILE
    ntl = NI * (NI + 1) // 2
    per = (ntl + groups - 1) // groups
    walk = []
    for cg in range(groups):
        t0 = cg * per
        t1 = t0 + per if t0 + per < ntl else ntl
        J = I = 0
        if t0 < t1:
            rem = t0
            while rem >= NI - J:
                rem -= NI - J
                J += 1
            I = J + rem
        tiles = []
        for _ in range(t0, t1):
            tiles.append((I, J))
            I += 1
            if I >= NI:
                J += 1
                I = J
        walk.append(tiles)
    return walk


def groups_changing_column(N):
    return [cg for cg, tiles in enumerate(tile_walk(N)) if len({J for _, J in tiles}) > 1]


def blocks4_tiles(N):
    """(NI, NJ, [(I, J)]) of k_sta_blocks_b4's 128 x 32 tile list: column J holds the row tiles J // 4 .. NI - 1."""
    NI, NJ = (N + 127) // 128, (N + 31) // 32
    return NI, NJ, [(I, J) for J in range(NJ) for I in range(J // 4, NI)]


# ---------------------------------------------------------------------------------------------------
# the batch's arithmetic, restated in float64 NumPy
# ---------------------------------------------------------------------------------------------------
MUTATIONS = {                                   # name -> (the blocks the measure may name, the least N and M at which it can act)
    "gts_without_jitter_aa": (("tilde_sigma",), 2, 1),              # the host epilogue's - 1e-6 aa_p dropped (N = 1: see below)
    "tkd_offdiagonal_x1": (("tilde_l",), 2, 1),                      # k_sta_reduce_b: tkd += c kd instead of 2 c kd
    "diagonal_as_offdiagonal": (("tilde_sigma", "uL_vec", "sigma2"), 1, 1),    # the i == j branch never taken
    "akd_from_previous_block": (("tilde_l",), 2, 2),                 # akd_p from alpha_(p - 1) (p = 0: from alpha_(M - 1))
    "last_tile_of_a_group_dropped": (("tilde_l", "tilde_sigma", "uL_vec", "sigma2"), 961, 1),      # t1 one short where per > 1
    "columns_not_reloaded": (("tilde_l", "tilde_sigma", "uL_vec"), 961, 1),    # sx / sa keep the first column of the group
}
# gts_without_jitter_aa at N = 1: the dropped term 1e-6 aa_p stands against alpha_p^T K alpha_p = (s^2 + 1e-6) aa_p with nothing to
# cancel, 1e-6 / s^2 = 1.4e-7 of the entry at s^2 = e^2 -- by the arithmetic alone under REJECT x 1e-8.  There the CPU half asserts
# what it measures, that the block is named over its bar (7.3 x), and counts the case in no least ratio.
OVER_THE_BAR_ONLY = {("gts_without_jitter_aa", 1)}
# where these cannot act the mutated arithmetic is the unmutated one bit for bit (asserted, not assumed): one tile per column group
# below N = 961; no off-diagonal element at N = 1; one block at M = 1
EXACT_WHERE_IDLE = ("last_tile_of_a_group_dropped", "columns_not_reloaded", "tkd_offdiagonal_x1", "akd_from_previous_block")


def can_act(mutation, N, M):
    return N >= MUTATIONS[mutation][1] and M >= MUTATIONS[mutation][2]


def sta_restated(pars, Y, x, mutation=None):
    """(loglik, d(-loglik)/d pars [T + 3]) as sta_batch_core forms them, in float64.  Per block p, from the lower triangle of
    -S_p^-1 only and in k_sta_reduce_b's tiles and column groups: tr, tk, tkd, aa, akd and alpha_p^T K alpha_q (the diagonal element
    carries + 1e-6); then the host epilogue: gtl, gts with both NMGP_JITTER corrections, Xs -> dB -> g_uL, ds.
    mutation: one of MUTATIONS, the arithmetic changed the way a wrong kernel or epilogue would change it."""
    from test_objective_sweep_cpu import _tril_stack
    assert mutation is None or mutation in MUTATIONS, mutation
    Y, x, pars = np.asarray(Y, dtype=np.float64), np.asarray(x, dtype=np.float64), np.asarray(pars, dtype=np.float64)
    N, M = Y.shape
    T = n_slots(M)
    l, sg, s2 = np.exp(pars[0]), np.exp(pars[1]), np.exp(pars[-1])
    L, r, c = _tril_stack(pars[2:2 + T], M)
    wB, VB = np.linalg.eigh(L @ L.T)
    yt = (Y @ VB).T                                          # [M, N]: yt_p = (V_B^T kron I) y
    A = l * l + l * l
    x2 = x * x
    dist = (x2[:, None] + x2[None, :]) - 2.0 * (x[:, None] * x[None, :])
    K = (sg * sg) * np.exp(-dist / A)                       # without the jitter
    Kj = K + JITTER * np.eye(N)
    # S_p^-1 and alpha_p from the eigenpairs of K_x + 1e-6 I: what the device gets from its factorisation, to float64's own accuracy
    # (a float64 Cholesky inverse of S_p, condition 1e6 .. 1e7, is itself 1e-8 off on the blocks that are small differences of large
    # sums: measured 1.2e-8 on tilde_sigma at (1026, 2), chain 1 -- it is the reduction and the epilogue that are restated here)
    lam, V = np.linalg.eigh(Kj)
    loglik = 0.0
    alpha, Cn = np.empty((M, N)), np.empty((M, N, N))
    for p in range(M):
        d = wB[p] * lam + s2
        Cn[p] = (V / d[None, :]) @ V.T                      # S_p^-1; the lower triangle is read
        alpha[p] = V @ ((V.T @ yt[p]) / d)
        loglik += -0.5 * np.log(d).sum() - 0.5 * (yt[p] @ alpha[p])
    tr, tk, tkd, akd = (np.zeros((G, M)) for _ in range(4))
    aKa = np.zeros((G, M, M))
    for cg, tiles in enumerate(tile_walk(N)):
        if mutation == "last_tile_of_a_group_dropped" and len(tiles) > 1:
            tiles = tiles[:-1]
        Jl = -1
        for I, J in tiles:
            if Jl < 0 or (J != Jl and mutation != "columns_not_reloaded"):
                Jl = J
            i0, j0 = I * TILE, J * TILE
            ii = np.arange(i0, min(i0 + TILE, N))
            jj = np.arange(j0, min(j0 + TILE, N))
            jl = jj - j0 + Jl * TILE                        # where the column values come from (LDS): the tile's own column, or a stale one
            xj, aj = x[jl], alpha[:, jl]
            xi, ai = x[ii], alpha[:, ii]
            d = (x2[ii][:, None] + (xj * xj)[None, :]) - 2.0 * (xi[:, None] * xj[None, :])
            kv = (sg * sg) * np.exp(-d / A)
            low = ii[:, None] > jj[None, :]
            dia = ii[:, None] == jj[None, :]
            if mutation == "diagonal_as_offdiagonal":
                low, dia = low | dia, np.zeros_like(dia)
            kd = kv * d
            for p in range(M):
                cm = Cn[p][np.ix_(ii, jj)]
                tr[cg, p] += (cm * dia).sum()
                tk[cg, p] += (cm * (kv + JITTER) * dia).sum() + 2.0 * (cm * kv * low).sum()
                tkd[cg, p] += (1.0 if mutation == "tkd_offdiagonal_x1" else 2.0) * (cm * kd * low).sum()
                pa = (p - 1) % M if mutation == "akd_from_previous_block" else p
                akd[cg, p] += 2.0 * (kd * low * np.outer(ai[pa], aj[pa])).sum()
                for q in range(p, M):
                    v = (kv * low * (np.outer(ai[p], aj[q]) + np.outer(ai[q], aj[p]))).sum()
                    if I == J and dia.any():
                        v += ((np.diag(kv) + JITTER) * ai[p] * ai[q]).sum()
                    aKa[cg, p, q] += v
                    if q != p:
                        aKa[cg, q, p] += v
    tr, tk, tkd, akd, aKa = tr.sum(0), tk.sum(0), tkd.sum(0), akd.sum(0), aKa.sum(0)
    aa = (alpha * alpha).sum(1)
    # the host epilogue of sta_batch_core
    gtl = 0.5 * (wB * (akd - tkd)).sum() / (l * l)
    if mutation == "gts_without_jitter_aa":
        gts = (wB * (np.diag(aKa) - (tk - JITTER * tr))).sum()
    else:
        gts = (wB * ((np.diag(aKa) - JITTER * aa) - (tk - JITTER * tr))).sum()
    Xs = 0.5 * (aKa - np.diag(tk))
    dB = VB @ Xs @ VB.T
    ds = 0.5 * (aa - tr).sum()
    g_uL = ((dB + dB.T) @ L)[r, c]
    dg = r == c
    g_uL[dg] *= L[r[dg], c[dg]]
    return float(loglik), -np.concatenate([[gtl], [gts], g_uL, [s2 * ds]])


_RESTATED = {}


def sta_restated_case(case, k, mutation=None):
    """sta_restated on chain k of a case; computed once."""
    key = (tuple(case), k, mutation)
    if key not in _RESTATED:
        N, M, variant = case
        x, Y, _ = subject(N, M, variant)
        ll, g = sta_restated(chains(N, M, variant)[k], Y, x, mutation)
        g.setflags(write=False)
        _RESTATED[key] = (ll, g)
    return _RESTATED[key]
