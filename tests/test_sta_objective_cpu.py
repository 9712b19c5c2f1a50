"""CPU half of the stationary objective sweep in the default formulation (no GPU): the references of
tests/test_gpu_sta_objective.py agree among themselves, the batch's formulation supports the bars in float64, the block measure names
the mistakes k_sta_reduce_b and the host epilogue can make, and the tile walk of the two large shapes is what the shapes were chosen
for.  Measured values: at the end of this docstring.

1. References among themselves.  On every new shape and variant the CPU oracle (float64, joint eigenbasis) is measured against the
   dense restatement (np.longdouble while N M <= 1000, float64 above): likelihood 1e-11; a block further than 1e-9 apart is an entry
   of sta_objective_cases.BLOCK_BARS at ten times the discrepancy, rounded up.  The three entries of eig_objective_cases.BLOCK_BARS
   are carried over.
2. sta_restated, the float64 NumPy restatement of sta_batch_core's arithmetic in k_sta_reduce_b's own tiles and column groups, is
   held to a tenth of the bars against the references (where both CPU references are float64: against the nearer of the two).
3. Six mutations of it (sta_objective_cases.MUTATIONS) are each named by their block at >= 100 x the bar (metric_cases.REJECT) on
   every chain of every case where they can act; where one cannot (the two tile mutations below N = 961, no off-diagonal element
   at N = 1, one block at M = 1) the mutated arithmetic has the unmutated one's bits.  How many of those cases the standing 1e-7 bar over the whole vector (tests/test_gpu_sta_batch.py) would have caught is
   printed.
4. The tile walk at N = 961 and N = 1026, and the edges of k_sta_blocks_b4 the even shapes reach.
5. The committed parity rows carry the case ids.

Measured (x86-64, 80-bit long double, 16 BLAS threads unless said otherwise):
  oracle vs np.longdouble dense, N M <= 1000     likelihood <= 2.2e-12 ((8, 8), chain 2); blocks <= 5.5e-10 (tilde_sigma, (127, 5), chain
                                                 1) but for (128, 4), chain 1: sigma2 5.3e-9, tilde_l 1.4e-9 (the two entries carried over)
  oracle vs float64 dense, N M > 1000            likelihood <= 1.0e-12; worst of 1, 4, 8, 16 threads: (257, 7) tilde_l 2.16e-9, tilde_sigma
                                                 2.25e-9, sigma2 6.0e-10; (1026, 2) tilde_sigma 6.56e-9, uL_vec 1.14e-9; (129, 8) and
                                                 (200, 6) <= 5.7e-10.  Over the floor at 16 threads: the first, second and fourth, the three new
                                                 entries of BLOCK_BARS (uL_vec: 4.9e-10 at 16 threads, no entry)
  sta_restated vs the references, N M <= 1000    likelihood <= 2.1e-12; blocks tilde_l 1.2e-10 ((961, 1)), tilde_sigma 3.6e-10 ((127, 5)),
                                                 uL_vec 5.1e-11, sigma2 5.6e-10 ((65, 3), subject 1); (128, 4), chain 1: sigma2 8.6e-9 of
                                                 the 2e-8 its entry allows
  sta_restated, N M > 1000, nearer reference     (257, 7) sigma2 1.2e-9 of 2e-9 (2.2e-9 at 4 threads, where the assertion fails), tilde_l
                                                 1.5e-9, tilde_sigma 1.4e-9 of 3e-9; (1026, 2) tilde_sigma 2.9e-9 of 7e-9.  With S_p^-1 from a float64 Cholesky instead of the
                                                 eigenpairs of K_x the same block is 1.2e-8 off: the inverse, not the reduction
  mutations, least ratio to the bar              gts_without_jitter_aa 2.6e3 ((2, 2); at N = 1 5.5 .. 7.3, named but below REJECT); tkd_offdiagonal_x1 5.1e7; diagonal_as_offdiagonal
                                                 1.0e8; akd_from_previous_block 1.6e7; last_tile_of_a_group_dropped 4.1e12;
                                                 columns_not_reloaded 2.3e11 (both at (961, 1)).  The standing 1e-7 over the whole vector
                                                 sees every mutated case (68, 64, 64, 58, 4, 4 of as many): what it lacked was a shape at
                                                 which the last two can act, and the resolution of a block"""
import json
import os

import numpy as np
import pytest

import metric_cases
import objective_cases as OC
import sta_objective_cases as S
from conftest import ROOT, relerr, vec_relerr

FLOOR_CASES = sorted(set(S.all_cases() + S.set_cases()), key=lambda c: (c[0], c[1], c[2]))
STANDING_GRAD_BAR = 1e-7                # tests/test_gpu_sta_batch.py: ||dg|| / ||g|| over the whole T + 3 vector


def _layout(case):
    return ("sta", case[0], case[1])


def _chains(case):
    return range(S.n_chains(*case))


# ---------------------------------------------------------------------------------------------------
# 1. the references among themselves
# ---------------------------------------------------------------------------------------------------
_FLOORS = {}


def _floor(case, k):
    """{block: the CPU oracle's distance from the dense restatement}, and the likelihood's."""
    if (case, k) not in _FLOORS:
        N, M, variant = case
        ll, g = S.dense(N, M, k, variant)
        r, go = S.oracle(N, M, k, False, variant)
        assert r[0] == -r[1]
        _FLOORS[(case, k)] = (relerr(r[1], ll), OC.block_table(go, g, _layout(case)))
    return _FLOORS[(case, k)]


@pytest.mark.parametrize("case", FLOOR_CASES, ids=S.case_id)
def test_the_oracle_against_the_dense_restatement_on_the_new_shapes(case):
    N, M, variant = case
    for k in _chains(case):
        el, tab = _floor(case, k)
        print("%s chain %d oracle vs %s dense: loglik %.3g blocks %s" % (S.case_id(case), k, S.dense_dtype(N, M).__name__, el,
                                                                        " ".join("%s=%.3g" % kv for kv in tab.items())))
        assert el <= S.LIK_TIGHT / 10, (case, k, el)
        for name, e in tab.items():                     # (without an entry: GRAD_TIGHT / 10 = REFERENCE_FLOOR)
            assert e <= S.BLOCK_BARS.get(_layout(case) + (name,), S.GRAD_TIGHT) / 10, (case, k, name, e)


def test_the_table_of_bars_holds_only_measured_discrepancies():
    """Every entry beyond the three carried over belongs to a block of a case whose two references are both float64 (N M > 1000), on
    which the oracle and the dense restatement are measured more than REFERENCE_FLOOR apart HERE, and is no lower than ten times that
    and no higher than ten times the worst of 1, 4, 8 and 16 BLAS threads, rounded up, that stands next to it in
    sta_objective_cases.py (an upper limit of 1e-7 on any of them).  The figures are documented for 16 BLAS threads."""
    import eig_objective_cases as E
    own = {k: v for k, v in S.BLOCK_BARS.items() if k not in E.BLOCK_BARS}
    assert all(S.BLOCK_BARS[k] == v for k, v in E.BLOCK_BARS.items())
    for (model, N, M, name), bar in own.items():
        worst = max(_floor(c, k)[1][name] for c in FLOOR_CASES if c[:2] == (N, M) for k in _chains(c))
        print("bar %s (%d, %d) %s: %.0e, measured discrepancy %.3g" % (model, N, M, name, bar, worst))
        assert model == "sta" and S.dense_dtype(N, M) is np.float64, (N, M, name)
        assert worst > S.REFERENCE_FLOOR, (N, M, name, worst)           # no entry without two references apart
        assert 10 * worst <= bar <= 1e-7, (N, M, name, worst, bar)


# ---------------------------------------------------------------------------------------------------
# 2. the restated arithmetic of the batch
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.all_cases() + [c for c in S.set_cases() if c[2]], ids=S.case_id)
def test_the_restated_batch_arithmetic_against_the_references(case):
    """At a tenth of the bars.  Where both CPU references are float64 (N M > 1000) neither is better than the other, and a block
    is held to the nearer of the two."""
    N, M, variant = case
    for k in _chains(case):
        r, gref = S.ref(N, M, k, False, variant)
        ll, g = S.sta_restated_case(case, k)
        el = relerr(ll, r[1])
        tab = OC.block_table(g, gref, _layout(case))
        if S.dense_dtype(N, M) is np.float64:
            for other in (S.dense(N, M, k, variant)[1], S.oracle(N, M, k, False, variant)[1]):
                for name, e in OC.block_table(g, other, _layout(case)).items():
                    tab[name] = min(tab[name], e)
        print("%s chain %d sta_restated vs reference: loglik %.3g blocks %s" % (S.case_id(case), k, el,
                                                                               " ".join("%s=%.3g" % kv for kv in tab.items())))
        assert el <= S.RESTATED_LIK, (case, k, el)
        for name, e in tab.items():
            assert e <= S.BLOCK_BARS.get(_layout(case) + (name,), S.GRAD_TIGHT) / 10, (case, k, name, e)


# ---------------------------------------------------------------------------------------------------
# 3. the measure bites
# ---------------------------------------------------------------------------------------------------
_LEAST = {}


@pytest.mark.parametrize("case", S.all_cases(), ids=S.case_id)
def test_the_block_measure_names_the_six_mutations(case):
    N, M, variant = case
    layout = _layout(case)
    for k in _chains(case):
        gref = S.ref(N, M, k, False, variant)[1]
        g = S.sta_restated_case(case, k)[1]
        assert not S.blocks_over_bar(g, gref, layout)
        for name, (expect, _, _) in S.MUTATIONS.items():
            gm = S.sta_restated_case(case, k, name)[1]
            if (name, N) in S.OVER_THE_BAR_ONLY:
                tab = OC.block_table(gm, gref, layout)
                print("%s chain %d %s: tilde_sigma at %.3g x its bar (N = 1: named, below REJECT)" % (S.case_id(case), k, name, tab["tilde_sigma"] / S.GRAD_TIGHT))
                assert [b[0] for b in S.blocks_over_bar(gm, gref, layout)] == ["tilde_sigma"], (case, k, name, tab)
                continue
            if not S.can_act(name, N, M):
                assert name in S.EXACT_WHERE_IDLE and np.array_equal(gm, g), (case, k, name)      # idle: the same bits
                continue
            tab = OC.block_table(gm, gref, layout)
            ratios = {b: tab[b] / S.BLOCK_BARS.get(layout + (b,), S.GRAD_TIGHT) for b in tab}
            block = max(ratios, key=ratios.get)
            standing = vec_relerr(gm, gref)
            seen = standing >= STANDING_GRAD_BAR
            print("%s chain %d %s: %s at %.3g x its bar; the standing measure %.3g, %s"
                  % (S.case_id(case), k, name, block, ratios[block], standing, "seen" if seen else "NOT seen"))
            least = _LEAST.setdefault(name, [np.inf, None, 0, 0])
            if ratios[block] < least[0]:
                least[0], least[1] = ratios[block], (S.case_id(case), k)
            least[2] += 1
            least[3] += bool(seen)
            assert block in expect and ratios[block] >= metric_cases.REJECT, (case, k, name, tab)
            assert block in [b[0] for b in S.blocks_over_bar(gm, gref, layout)]
            for b in tab:                               # ... and it names no block it cannot touch
                assert b in expect or ratios[b] < 1, (case, k, name, b, tab)


def test_the_least_ratio_of_every_mutation_is_printed():
    """(after the cases above; alone, it computes the two large shapes and the smallest case with M >= 2)"""
    if not _LEAST:
        for case in [(2, 2, "")] + [c + ("",) for c in S.LARGE_SHAPES]:
            test_the_block_measure_names_the_six_mutations(case)
    for name, (ratio, where, n, seen) in _LEAST.items():
        print("mutation %s: least ratio to the bar %.3g at %s; the standing 1e-7 over the whole vector sees %d of %d cases"
              % (name, ratio, where, seen, n))
        assert ratio >= metric_cases.REJECT
    assert set(_LEAST) == set(S.MUTATIONS)


# ---------------------------------------------------------------------------------------------------
# 4. index arithmetic
# ---------------------------------------------------------------------------------------------------
def test_the_tile_walk_of_the_reduction_at_the_large_shapes():
    for N, _ in S.SHAPES:
        walk = S.tile_walk(N)
        NI = (N + 63) // 64
        flat = [t for tiles in walk for t in tiles]
        assert flat == [(I, J) for J in range(NI) for I in range(J, NI)]       # every tile once, column by column
        if N < 961:
            assert max(len(t) for t in walk) == 1 and not S.groups_changing_column(N)
    w961, w1026 = S.tile_walk(961), S.tile_walk(1026)
    assert [len(t) for t in w961] == [2] * 68 + [0] * 60                        # ntl = 136, per = 2
    assert S.groups_changing_column(961) == [15, 22, 40, 45, 57, 60, 66, 67]
    assert w961[15] == [(15, 1), (2, 2)] and w961[67] == [(15, 14), (15, 15)] and w961[0] == [(0, 0), (1, 0)]
    assert [len(t) for t in w1026] == [2] * 76 + [1] + [0] * 51                 # ntl = 153: the last live group holds one tile
    assert w1026[76] == [(16, 16)]
    assert S.groups_changing_column(1026) == [8, 16, 37, 43, 58, 62, 71, 73]
    assert w1026[8] == [(16, 0), (1, 1)]
    print("N = 961: 68 groups of 2 tiles, column changes in groups %s" % S.groups_changing_column(961))
    print("N = 1026: 76 groups of 2 tiles and group 76 of 1, column changes in groups %s" % S.groups_changing_column(1026))
    # the workgroup -> column group map is a permutation of the G groups
    assert sorted((g & 7) * (S.G >> 3) + (g >> 3) for g in range(S.G)) == list(range(S.G))


def test_the_even_shapes_reach_the_edges_of_the_block_build():
    even = sorted({N for N, _ in S.SHAPES if N % 2 == 0})
    assert {34, 126, 130, 258, 1026} <= set(even)
    NI, NJ, tiles = S.blocks4_tiles(34)
    assert (NI, NJ) == (1, 2) and 34 - 32 == 2                                  # a second column tile of two columns
    assert S.blocks4_tiles(126)[:2] == (1, 4) and 126 == 128 - 2                # one row tile less a pair
    NI, NJ, tiles = S.blocks4_tiles(130)
    assert (NI, NJ) == (2, 5) and (0, 4) not in tiles and (1, 4) in tiles and 130 - 128 == 2      # column 4 begins at row tile 1
    assert S.blocks4_tiles(258)[:2] == (3, 9) and 258 - 256 == 2                # a third row tile of one pair; a ragged 256 block
    NI, NJ, tiles = S.blocks4_tiles(1026)
    assert (NI, NJ) == (9, 33) and len(tiles) == sum(NI - J // 4 for J in range(NJ))
    assert (961 + 63) // 64 == 16 and (16 * 17 // 2 + 7) // 8 == 17              # the odd-N build at 961: per = 17
    assert {M for _, M in S.SHAPES} == set(range(1, 9))
    assert S.dense_dtype(961, 1) is np.longdouble and S.dense_dtype(1026, 2) is np.float64


# ---------------------------------------------------------------------------------------------------
# 5. the committed record
# ---------------------------------------------------------------------------------------------------
def test_committed_parity_rows_carry_the_case_ids():
    rows = json.load(open(os.path.join(ROOT, "profiles", "sta_objective_parity.json")))["rows"]
    names = [r["case"] for r in rows if r["case"].startswith("sta_objective/")]
    assert names
    have = {n.split("/")[1] for n in names}
    want = {S.case_id(c) for c in S.all_cases()} | {"set_" + OC.case_id(s) for s in S.SET_SHAPES}
    assert want <= have, want - have
    for c in S.all_cases():
        for entry in ("single", "batch%d_grad" % S.batch(*c[:2])):
            for prior in (0, 1):
                assert "sta_objective/%s/%s/prior%d" % (S.case_id(c), entry, prior) in names, (c, entry, prior)
