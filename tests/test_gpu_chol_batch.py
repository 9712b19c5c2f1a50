"""GPU half of the batched-Cholesky sweep (cases, reference and bars: tests/chol_batch_cases.py; CPU half: tests/test_chol_batch_cpu.py).
nmgp_cholesky_batch lays a batch out and launches it as the batched objectives do; here every output MATRIX of it -- the factor, the
dense rows below it, X = L^-T, the inverse -X X^T -- is compared with LAPACK per matrix of the batch, under each schedule switch.  The
switches are read once per process, so one configuration = one child process = one test; the child runs all tables on one Context,
does the comparisons itself and prints one JSON line per case (achieved error as a fraction of its bar, status words, SHA-256 of each
output), which the parent asserts on and records in the parity table.

Asserted per case and matrix: status 0; factor, rows, X (upper triangle only: left of the diagonal nothing is promised, and under
NMGP_POISON=1 it is NaN outside the seeded band, which the poisoned configurations also check), inverse inside their bars; backward
error < 20 x LAPACK's; everything compared finite; in tables A and C the copy of matrix 0 at the last position has the bytes of matrix 0
in every output.  want_inv = 2: syrk_tile_fast / syrk_tile_body store the SAME accumulator value at (i, j) and (j, i) (the `mirror`
stores), so exact symmetry is promised and asserted.  Table E: the bad matrix reports exactly bad + 1 (LAPACK's index), every other
matrix 0 and the bytes it has when the bad matrix is replaced by a good one.

Whether the default and the throughput configuration give the same hashes is RECORDED (parity row chol_batch/identity_1_vs_2/summary
and one row per case that differs), not asserted: the project claims bit identity only at the sizes of test_gpu_chol_leftlooking.py
and test_gpu_leaf_pipeline.py."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import chol_batch_cases as cb
from conftest import ROOT, record_parity

pytestmark = pytest.mark.gpu

CONFIGS = [
    ("default", {}),
    ("throughput", {"NMGP_CHOL_FUSED_MAX_BATCH": "0"}),
    ("throughput_poison", {"NMGP_CHOL_FUSED_MAX_BATCH": "0", "NMGP_POISON": "1"}),
    ("panel_rec", {"NMGP_CHOL_PANEL": "rec"}),
    ("panel_rl", {"NMGP_CHOL_PANEL": "rl"}),
    ("fused_base128", {"NMGP_CHOL_FUSED_BASE": "128"}),
    ("throughput_nb256", {"NMGP_CHOL_FUSED_MAX_BATCH": "0", "NMGP_CHOL_NB1": "256"}),     # every panel one node, look-ahead from n = 768
    ("throughput_syrk_small", {"NMGP_CHOL_FUSED_MAX_BATCH": "0", "NMGP_SYRK_SMALL_MAX": "100000"}),
    ("default_poison", {"NMGP_POISON": "1"}),
]
SWITCHES = sorted({k for _, env in CONFIGS for k in env})
N_LINES = len(cb.REFERENCE_TABLES) + 2 * (1 + len(cb.TABLE_E))
_results = {}          # configuration name -> {row id: JSON line}: the hashes of configurations 1 and 2 are compared when both have run


# ---- the child ------------------------------------------------------------------------------------------------------------------------------
def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def run_case(ctx, case, poison):
    A, R = cb.case_inputs(case)
    Ain = np.where(np.tri(case.n, k=-1, dtype=bool), np.nan, A)      # NaN in the triangle nobody may rely on
    L, Z, X, Sinv, status = ctx.cholesky_batch(Ain, R, want_xtri=case.xtri, want_inv=case.inv, precise=case.precise)
    fr = {"L": 0.0, "backward": 0.0}
    fail = []
    if not np.all(status == 0):
        fail.append("status %s" % status.tolist())
    for b in range(case.batch):
        src = cb.source_index(case, b)
        Lr, Xr, res = cb.refs(case.n, src)
        fr["L"] = max(fr["L"], cb.frac_L(L[b], Lr))
        fr["backward"] = max(fr["backward"], cb.frac_backward(L[b], A[b], res))
        if case.extra:
            fr["rows"] = max(fr.get("rows", 0.0), cb.frac_rows(Z[b], cb.rows_ref(Lr, R[b])))
        if case.xtri:
            fr["X"] = max(fr.get("X", 0.0), cb.frac_X(X[b], Xr))
            if poison and case.n >= 320 and not np.isnan(X[b][case.n - 1, 0]):
                fail.append("X[%d][n - 1, 0] is not NaN under poison: the entry or a kernel wrote left of the seeded band" % b)
        if case.inv:
            e, m = cb.frac_inv(Sinv[b], cb.inv_ref(case.n, src), case.inv == 1)
            fr["inv"], fr["inv_maxnorm"] = max(fr.get("inv", 0.0), e), max(fr.get("inv_maxnorm", 0.0), m)
            if case.inv == 2 and not np.array_equal(Sinv[b], Sinv[b].T):
                fail.append("inverse of matrix %d is not exactly symmetric" % b)
            if case.inv == 1 and np.triu(Sinv[b], 1).any():
                fail.append("want_inv = 1 returned something above the diagonal")
        if np.triu(L[b], 1).any():
            fail.append("L[%d] has entries above the diagonal" % b)
    Xu = None if X is None else np.triu(X)
    outs = {"L": L, "rows": Z, "X": Xu, "inv": Sinv}
    if case.table in cb.COPY_TABLES and case.batch >= 2:
        for k, v in outs.items():
            if v is not None and v[0].tobytes() != v[-1].tobytes():
                fail.append("%s of the copy at position %d differs from matrix 0" % (k, case.batch - 1))
    for k, v in fr.items():
        if not (v < 1.0 if k == "backward" else v <= 1.0):
            fail.append("%s at %.3g of its bar" % (k, v))
    return {"row": "%s/%s" % (case.table, cb.case_id(case)), "frac": fr, "status": status.tolist(), "fail": fail,
            "sha": {k: sha(v) for k, v in outs.items() if v is not None}}


def run_status_table(ctx, xtri):
    """Table E with / without the rows of L^-T: the all-good batch against LAPACK, then one line per (bad, position)."""
    A, R = cb.status_inputs()
    good = ctx.cholesky_batch(A, R, want_xtri=xtri)
    fr = {"L": 0.0, "backward": 0.0, "rows": 0.0}
    fail = [] if np.all(good[4] == 0) else ["status %s" % good[4].tolist()]
    for b in range(cb.E_BATCH):
        Lr, Xr, res = cb.status_refs(b)
        fr["L"] = max(fr["L"], cb.frac_L(good[0][b], Lr))
        fr["backward"] = max(fr["backward"], cb.frac_backward(good[0][b], A[b], res))
        fr["rows"] = max(fr["rows"], cb.frac_rows(good[1][b], cb.rows_ref(Lr, R[b])))
        if xtri:
            fr["X"] = max(fr.get("X", 0.0), cb.frac_X(good[2][b], Xr))
    fail += ["%s at %.3g of its bar" % (k, v) for k, v in fr.items() if not (v < 1.0 if k == "backward" else v <= 1.0)]
    outs = [good[0], good[1]] + ([np.triu(good[2])] if xtri else [])
    yield {"row": "E/good_x%d" % xtri, "frac": fr, "status": good[4].tolist(), "fail": fail, "sha": {"all": sha(*outs)}}
    for bad, pos in cb.TABLE_E:
        Ab, _ = cb.status_inputs(bad, pos)
        got = ctx.cholesky_batch(Ab, R, want_xtri=xtri)
        want = [bad + 1 if b == pos else 0 for b in range(cb.E_BATCH)]
        fail = [] if got[4].tolist() == want else ["status %s, LAPACK's is %s" % (got[4].tolist(), want)]
        gouts = [got[0], got[1]] + ([np.triu(got[2])] if xtri else [])
        others = [b for b in range(cb.E_BATCH) if b != pos]
        for name, g, o in zip(("L", "rows", "X"), gouts, outs):
            for b in others:
                if g[b].tobytes() != o[b].tobytes():
                    fail.append("%s of matrix %d changed with matrix %d indefinite" % (name, b, pos))
        yield {"row": "E/bad%d_pos%d_x%d" % (bad, pos, xtri), "frac": {}, "status": got[4].tolist(), "fail": fail,
               "sha": {"others": sha(*[g[others] for g in gouts])}}


def child():
    sys.path.insert(0, ROOT)
    from nonstationary_multivariate_gaussian_process_amd import _lib
    poison = os.environ.get("NMGP_POISON", "0") not in ("", "0")
    ctx = _lib.Context(0)
    # want_inv without the rows of L^-T is refused, and refusing leaves the context usable
    try:
        ctx.cholesky_batch(cb.matrix(64, 0)[None], None, want_xtri=False, want_inv=1)
        print(json.dumps({"row": "entry/want_inv_without_xtri", "frac": {}, "status": [], "fail": ["not refused"], "sha": {}}))
    except _lib.NmgpError:
        pass
    for case in cb.REFERENCE_TABLES:
        print(json.dumps(run_case(ctx, case, poison)), flush=True)
    for xtri in (0, 1):
        for line in run_status_table(ctx, xtri):
            print(json.dumps(line), flush=True)
    ctx.close()


# ---- the parent -----------------------------------------------------------------------------------------------------------------------------
def run_child(env_extra):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(env_extra)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, timeout=300, env=env,
                         cwd=ROOT)
    assert out.returncode == 0, (env_extra, out.stdout[-1500:], out.stderr[-3000:])
    return [json.loads(ln) for ln in out.stdout.splitlines() if ln.startswith("{")]


@pytest.mark.parametrize("name,env_extra", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_batched_factorisation_outputs_against_lapack(name, env_extra):
    lines = run_child(env_extra)
    # The parity table holds the default configuration's rows in full.  Of any other configuration it holds the rows whose figures
    # differ from the default's row of the same case, and one summary row that counts the rest (the schedules mostly give the same
    # bits, and nine copies of one figure tell nothing more); run without the default configuration, its rows are all recorded.
    base = _results.get(CONFIGS[0][0]) if name != CONFIGS[0][0] else None
    failures, same = [], 0
    for ln in lines:
        print(name, ln["row"], ln["frac"], ln["status"])
        failures += ["%s: %s" % (ln["row"], f) for f in ln["fail"]]
        if base is not None and ln["row"] in base and base[ln["row"]]["frac"] == ln["frac"]:
            same += 1
            continue
        record_parity("chol_batch/%s/%s" % (name, ln["row"]), **{k: (v, 1.0) for k, v in ln["frac"].items()})
    if base is not None:
        record_parity("chol_batch/%s/summary" % name, rows=len(lines), rows_with_the_default_figures=same)
    rows = {ln["row"]: ln for ln in lines}
    assert len(lines) == N_LINES and len(rows) == N_LINES, (len(lines), N_LINES)
    _results[name] = rows
    if name == "throughput" and "default" in _results:
        equal = [row for row, ln in rows.items() if ln["sha"] == _results["default"][row]["sha"]]
        record_parity("chol_batch/identity_1_vs_2/summary", cases=len(rows), same_hashes=len(equal))
        for row in rows:
            if row not in equal:
                record_parity("chol_batch/identity_1_vs_2/%s" % row, same_hashes=0.0)
    assert not failures, (name, len(failures), failures[:40])


if __name__ == "__main__" and sys.argv[1:] == ["--child"]:
    child()
