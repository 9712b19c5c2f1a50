"""CPU half of the batched-Cholesky sweep (tests/chol_batch_cases.py, GPU half: tests/test_gpu_chol_batch.py): the float64 reference
the device outputs are held to (np.linalg.cholesky + scipy.linalg.solve_triangular) is itself held to a numpy.longdouble restatement
-- a column Cholesky and a forward substitution -- and must stay within 1 % of every bar; LAPACK's dpotrf reports bad + 1 for every
matrix of the status table; the case tables are the ones the sweep was specified with."""
import numpy as np
import pytest
import scipy.linalg.lapack

import chol_batch_cases as cb

LD = np.longdouble
wide = pytest.mark.skipif(not np.finfo(LD).eps < 1e-18, reason="numpy.longdouble is no wider than float64 here")


def chol_ld(A):
    """Column Cholesky in longdouble."""
    n = A.shape[0]
    A = A.astype(LD)
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        v = A[j:, j] - L[j:, :j] @ L[j, :j]
        L[j:, j] = v / np.sqrt(v[0])
    return L


def forward_ld(L, B):
    """L^-1 B by forward substitution in longdouble."""
    n = L.shape[0]
    Y = np.zeros(B.shape, dtype=LD)
    B = B.astype(LD)
    for i in range(n):
        Y[i] = (B[i] - L[i, :i] @ Y[:i]) / L[i, i]
    return Y


@wide
@pytest.mark.parametrize("n", [333, 768])
def test_float64_reference_is_within_one_percent_of_every_bar(n):
    A = cb.matrix(n, 0)
    R = cb.rows(n, 0, 3)
    assert np.array_equal(A, A.T)
    cond = np.linalg.cond(A)
    print("cond", cond)
    assert cond < 40
    L, X, res = cb.refs(n, 0)
    Lq = chol_ld(A)
    Yq = forward_ld(Lq, np.hstack([np.eye(n), R.T]))          # L^-1 [I | R^T]
    Xq, Zq = Yq[:, :n].T, Yq[:, n:].T                         # L^-T, R L^-T
    invq = -(Xq @ Xq.T)
    assert float(np.abs(Lq @ Lq.T - A.astype(LD)).max()) < 1e-17 * float(np.abs(A).max()) * n
    fr = {"L": cb.frac_L(L, Lq.astype(np.float64)),
          "X": cb.frac_X(X, Xq.astype(np.float64)),
          "rows": cb.frac_rows(cb.rows_ref(L, R), Zq.astype(np.float64))}
    fr["inv"], fr["inv_maxnorm"] = cb.frac_inv(cb.inv_ref(n, 0), invq.astype(np.float64), False)
    print(n, fr, "lapack residual", res)
    for k, v in fr.items():
        assert v <= 0.01, (n, k, v)
    # X is upper triangular in the reference: nothing left of the diagonal takes part in a comparison
    assert not np.tril(X, -1).any()
    # LAPACK's own backward error is at rounding level, so the 20 x bar is a rounding-level bar
    assert res < 8 * cb.EPS


def test_lapack_reports_bad_plus_one_for_every_status_matrix():
    for bad, pos in cb.TABLE_E:
        A, _ = cb.status_inputs(bad, pos)
        for b in range(cb.E_BATCH):
            _, info = scipy.linalg.lapack.dpotrf(A[b], lower=1)
            assert info == (bad + 1 if b == pos else 0), (bad, pos, b, info)
    A, _ = cb.status_inputs()
    assert all(np.linalg.eigvalsh(A[b]).min() >= 1.0 - 1e-12 for b in range(cb.E_BATCH))


def test_case_tables_are_the_specified_ones():
    C = cb.Case
    sizes = [64, 128, 192, 256, 320, 384, 448, 512, 576, 640, 768, 1088, 200, 333, 600]
    assert cb.TABLE_A == [C("A", n, 4, 1, x, 0, 0) for n in sizes for x in (0, 1)] and len(cb.TABLE_A) == 30
    extras, extras_x = [0, 1, 2, 3, 15, 16, 17, 63, 64, 65, 129, 130], [1, 2, 17, 65]
    assert sorted(cb.TABLE_B) == sorted([C("B", n, 4, e, 0, 0, 0) for n in (256, 320) for e in extras] +
                                        [C("B", n, 4, e, 1, 0, 0) for n in (256, 320) for e in extras_x]) and len(cb.TABLE_B) == 32
    assert cb.TABLE_C == [C("C", n, b, 1, 1, 0, 0) for n in (256, 448) for b in (1, 2, 3, 4, 5, 8, 9, 16, 17)]
    assert cb.TABLE_D == [C("D", n, b, e, 0, 0, 1) for n in (64, 200, 256, 333, 576) for b in (1, 5) for e in (0, 1, 70)]
    assert cb.TABLE_F == [C("F", n, b, 1, 1, i, 0) for n in (64, 128, 192, 256, 320, 600) for i in (1, 2) for b in (1, 5)]
    assert cb.E_N == 640 and cb.E_BATCH == 5
    assert [bad for bad, _ in cb.TABLE_E] == [10, 70, 130, 200, 261, 330, 400, 460, 515, 600]
    assert [pos for _, pos in cb.TABLE_E] == [0, 2, 4, 0, 2, 4, 0, 2, 4, 0]
    every = cb.REFERENCE_TABLES
    assert len(every) == 30 + 32 + 18 + 30 + 24 and len(set(every)) == len(every) and max(c.n for c in every) == 1088
    assert max(c.extra for c in every) <= cb.MAX_EXTRA
    ids = [c.table + "/" + cb.case_id(c) for c in every]
    assert len(set(ids)) == len(ids)


def test_inputs_differ_per_matrix_and_the_copy_sits_last():
    c = cb.Case("C", 256, 5, 1, 1, 0, 0)
    A, R = cb.case_inputs(c)
    assert A.shape == (5, 256, 256) and R.shape == (5, 1, 256)
    assert np.array_equal(A[4], A[0]) and np.array_equal(R[4], R[0])
    assert len({A[b].tobytes() for b in range(4)}) == 4 and len({R[b].tobytes() for b in range(4)}) == 4
    d = cb.Case("D", 256, 5, 70, 0, 0, 1)
    A, R = cb.case_inputs(d)
    assert len({A[b].tobytes() for b in range(5)}) == 5 and R.shape == (5, 70, 256)
    assert np.array_equal(R[1][:1], cb.rows(256, 1, 1))
    assert cb.case_inputs(cb.Case("B", 256, 4, 0, 0, 0, 0))[1] is None


def test_measures_reject_what_is_not_finite_or_misplaced():
    L, X, _ = cb.refs(64, 0)
    assert cb.frac_L(L, L) == 0.0 and cb.frac_X(X, X) == 0.0
    bad = L.copy()
    bad[5, 3] = np.nan
    assert cb.frac_L(bad, L) == float("inf")
    # X: NaN left of the diagonal is ignored, on or right of it is not
    Xn = X.copy()
    Xn[np.tril_indices(64, -1)] = np.nan
    assert cb.frac_X(Xn, X) == 0.0
    Xn[3, 5] = np.nan
    assert cb.frac_X(Xn, X) == float("inf")
    # a transposed factor, one swapped pair of rows: far outside
    assert cb.frac_L(L.T, L) > 1e6
    sw = L.copy()
    sw[[10, 11]] = sw[[11, 10]]
    assert cb.frac_L(sw, L) > 1e6
    e, m = cb.frac_inv(np.tril(cb.inv_ref(64, 0)), cb.inv_ref(64, 0), True)
    assert e == 0.0 and m == 0.0
    assert cb.frac_inv(np.tril(cb.inv_ref(64, 0)), cb.inv_ref(64, 0), False)[0] > 1.0
