"""Cases, inputs, float64 references and bars of the batched-Cholesky sweep (tests/test_chol_batch_cpu.py, tests/test_gpu_chol_batch.py):
every output MATRIX of nmgp_cholesky_batch -- the factor, the dense rows that ride below it, X = L^-T and the inverse the gradient
paths build from X -- against LAPACK, per matrix of the batch, at the smallest shapes that reach each launch form of the batched
schedules.  A plain module, not a conftest: both halves import it, so the CPU half checks the very cases and the very reference the
GPU half uses.  No GPU result enters a reference or a bar.

Matrices: those of test_custom_cholesky_against_lapack, G G^T / n + 0.5 I scaled asymmetrically by 1 + i / n (a row/column mix-up
cannot cancel), one seed per (n, position in the batch); condition number ~17.  Table E: I + G G^T with one diagonal entry set to -1,
as in test_custom_cholesky_reports_indefinite_matrix.

Bars (the project's, from test_gpu_parity.py):
  factor                       |got - ref| <= 1e-12 + 1e-11 |ref|, elementwise
  dense rows, X (upper), A^-1  |got - ref| <= 1e-11 + 1e-10 |ref|, elementwise; the inverse also max|got - ref| <= 1e-10 max|A^-1|
  backward error               max|L L^T - A| / max|A| < 20 max(LAPACK's, eps)
The float64 reference itself sits below 1 % of each (test_chol_batch_cpu.py, against numpy.longdouble)."""
import collections
import functools

import numpy as np
import scipy.linalg

EPS = float(np.finfo(np.float64).eps)
L_RTOL, L_ATOL = 1e-11, 1e-12
Z_RTOL, Z_ATOL = 1e-10, 1e-11
BACKWARD_FACTOR = 20.0
MAX_EXTRA = 130

Case = collections.namedtuple("Case", "table n batch extra xtri inv precise")

# ---- case tables ------------------------------------------------------------------------------------------------------------------------
# A: every lone-panel width of panel_halving (128 leaf, 192 = 128 | 64, the 256 node, 320 .. 512), 512 + a 64 / 128 / 256 panel, two
#    full panels + a block (trailing update with two panels, two-stream look-ahead), ragged sizes on the block solve
A_SIZES = [64, 128, 192, 256, 320, 384, 448, 512, 576, 640, 768, 1088, 200, 333, 600]
TABLE_A = [Case("A", n, 4, 1, x, 0, 0) for n in A_SIZES for x in (0, 1)]
# B: row counts below the matrix across a wave (16), workgroup 0 (64) and the first 128-row workgroup; 0 skips a node's last launch
B_EXTRA, B_EXTRA_X = [0, 1, 2, 3, 15, 16, 17, 63, 64, 65, 129, 130], [1, 2, 17, 65]
TABLE_B = [Case("B", n, 4, e, 0, 0, 0) for n in (256, 320) for e in B_EXTRA] + \
          [Case("B", n, 4, e, 1, 0, 0) for n in (256, 320) for e in B_EXTRA_X]
# C: batches below 4 (panel_rl under the throughput switch), odd batches (T * batch no multiple of 8)
C_BATCH = [1, 2, 3, 4, 5, 8, 9, 16, 17]
TABLE_C = [Case("C", n, b, 1, 1, 0, 0) for n in (256, 448) for b in C_BATCH]
# D: the accuracy-first diagonal blocks and solves with a batch
TABLE_D = [Case("D", n, b, e, 0, 0, 1) for n in (64, 200, 256, 333, 576) for b in (1, 5) for e in (0, 1, 70)]
# F: the inverse SYRK -X X^T, lower triangle / both triangles
TABLE_F = [Case("F", n, b, 1, 1, inv, 0) for n in (64, 128, 192, 256, 320, 600) for inv in (1, 2) for b in (1, 5)]
# E: the status word.  n = 640, batch = 5; `bad` in each block of the first 256-column node (blocks 2 and 3 are factored inside the leaf
# launches), the first block of the right node (inside the K = 256 update) and later ones, the first block of the second panel (inside
# the trailing update), the last block; the bad matrix at position 0, 2 or 4, rotated
E_N, E_BATCH = 640, 5
E_BAD = [10, 70, 130, 200, 261, 330, 400, 460, 515, 600]
TABLE_E = [(bad, (0, 2, 4)[k % 3]) for k, bad in enumerate(E_BAD)]
REFERENCE_TABLES = TABLE_A + TABLE_B + TABLE_C + TABLE_D + TABLE_F
COPY_TABLES = ("A", "C")       # the last matrix of the batch is a copy of matrix 0 (batch-position invariance)


def case_id(c):
    return "n%d_b%d_e%d_x%d_i%d_p%d" % (c.n, c.batch, c.extra, c.xtri, c.inv, c.precise)


def source_index(case, b):
    """Which generated matrix sits at position b of the case's batch."""
    return 0 if (case.table in COPY_TABLES and case.batch >= 2 and b == case.batch - 1) else b


# ---- inputs (shared: do not write) --------------------------------------------------------------------------------------------------------
def _sym_from_upper(A):
    """Exactly symmetric, from the triangle the device reads."""
    U = np.triu(A)
    return U + np.triu(A, 1).T


@functools.lru_cache(maxsize=None)
def matrix(n, b):
    rng = np.random.default_rng([n, b])
    G = rng.standard_normal((n, n + 3))
    A = G @ G.T / n + 0.5 * np.eye(n)
    dscale = 1.0 + np.arange(n) / n
    A = _sym_from_upper(A * np.outer(dscale, dscale))
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def _rows_all(n, b):
    R = np.random.default_rng([n, b, 1]).standard_normal((MAX_EXTRA, n))
    R.setflags(write=False)
    return R


def rows(n, b, extra):
    return _rows_all(n, b)[:extra]


@functools.lru_cache(maxsize=None)
def status_matrix(b):
    """Table E's positive definite matrices."""
    G = np.random.default_rng([E_N, b, 2]).standard_normal((E_N, 8)) / np.sqrt(E_N)
    A = _sym_from_upper(np.eye(E_N) + G @ G.T)
    A.setflags(write=False)
    return A


def case_inputs(case):
    A = np.stack([matrix(case.n, source_index(case, b)) for b in range(case.batch)])
    R = np.stack([rows(case.n, source_index(case, b), case.extra) for b in range(case.batch)]) if case.extra else None
    return A, R


def status_inputs(bad=None, pos=None):
    A = np.stack([status_matrix(b) for b in range(E_BATCH)])
    if bad is not None:
        A[pos, bad, bad] = -1.0
    R = np.stack([np.random.default_rng([E_N, b, 3]).standard_normal((1, E_N)) for b in range(E_BATCH)])
    return A, R


# ---- float64 reference --------------------------------------------------------------------------------------------------------------------
def residual(L, A):
    return float(np.abs(L @ L.T - A).max() / np.abs(A).max())


def factor_refs(A):
    """L (np.linalg.cholesky), X = L^-T (scipy.linalg.solve_triangular) and LAPACK's own backward error."""
    L = np.linalg.cholesky(A)
    X = scipy.linalg.solve_triangular(L, np.eye(A.shape[0]), lower=True).T
    return L, X, residual(L, A)


@functools.lru_cache(maxsize=None)
def refs(n, b):
    return factor_refs(matrix(n, b))


@functools.lru_cache(maxsize=None)
def status_refs(b):
    return factor_refs(status_matrix(b))


def rows_ref(L, R):
    return scipy.linalg.solve_triangular(L, R.T, lower=True).T          # R L^-T


def inverse_ref(X):
    return -(X @ X.T)


@functools.lru_cache(maxsize=None)
def inv_ref(n, b):
    return inverse_ref(refs(n, b)[1])


# ---- measures: achieved error as a fraction of the bar (<= 1 passes; anything not finite is inf) -------------------------------------------
def frac(got, ref, rtol, atol):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if got.shape != ref.shape or not np.all(np.isfinite(got)):
        return float("inf")
    if got.size == 0:
        return 0.0
    return float(np.max(np.abs(got - ref) / (atol + rtol * np.abs(ref))))


def frac_L(got, ref):
    return frac(got, ref, L_RTOL, L_ATOL)


def frac_rows(got, ref):
    return frac(got, ref, Z_RTOL, Z_ATOL)


def frac_X(got, ref):
    """The upper triangle only: what lies left of the diagonal is not promised (NaN under NMGP_POISON=1)."""
    iu = np.triu_indices(ref.shape[0])
    return frac(np.asarray(got)[iu], ref[iu], Z_RTOL, Z_ATOL)


def frac_inv(got, ref, lower_only):
    """(elementwise fraction, max-norm fraction: max|got - ref| / (1e-10 max|A^-1|))."""
    if lower_only:
        il = np.tril_indices(ref.shape[0])
        got, ref = np.asarray(got)[il], ref[il]
    e = frac(got, ref, Z_RTOL, Z_ATOL)
    m = float(np.max(np.abs(np.asarray(got) - ref)) / (Z_RTOL * np.max(np.abs(ref)))) if np.isfinite(e) else float("inf")
    return e, m


def frac_backward(L, A, lapack_residual):
    if not np.all(np.isfinite(L)):
        return float("inf")
    return residual(L, A) / (BACKWARD_FACTOR * max(lapack_residual, EPS))
