"""The Sigma' epilogue of k_syrk_schur (the structured value path's inverse SYRK) on the smallest shapes that reach each of its
paths: a full diagonal tile, a full off-diagonal tile with its mirrored pass, a row past a tile edge, partial tiles on the masked
path, M = 2 (no mirrored pass), M = 4 (rolled loops, table), M = 5 (no table) and two subjects with two chains each (the
per-subject x / Y stride).  The cases, their inputs and the evaluation are those of tools/make_schurepi_fixture.py, which wrote
tests/golden/schurepi_parent_bits.npz with the library of the commit before the epilogue's store shape changed: reshaping stores
and index arithmetic must not change one bit of `out` or `status`."""
import functools
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, relerr

pytestmark = pytest.mark.gpu

TOOL = os.path.join(ROOT, "tools", "make_schurepi_fixture.py")
# test_svc_schur.py's bars against the dense path (NMGP_SVC_SCHUR=0) of the same build: log posterior and priors, likelihood term
VAL_TOL, LIK_TOL = 1e-6, 1e-9


@functools.lru_cache(maxsize=None)
def tool():
    spec = importlib.util.spec_from_file_location("make_schurepi_fixture", TOOL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


CASE_NAMES = ("N128_M3_B2", "N256_M3_B2", "N257_M3_B3", "N200_M3_B2", "N384_M2_B2", "N256_M4_B2", "N160_M5_B2", "N256_M3_S2x2")


@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(os.path.join(GOLDEN, "schurepi_parent_bits.npz")) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def structured(name):
    return tool().evaluate(name)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b) and a.tobytes() == b.tobytes()


def test_the_cases_are_the_tools():
    assert tuple(c[0] for c in tool().CASES) == CASE_NAMES
    assert sorted(fixture()) == sorted(n + s for n in CASE_NAMES for s in ("/out", "/status"))


@pytest.mark.parametrize("name", CASE_NAMES)
def test_value_path_gives_the_parent_commits_bits(name):
    out, status = structured(name)
    want_out, want_status = fixture()[name + "/out"], fixture()[name + "/status"]
    assert out.dtype == np.float64 and status.dtype == np.int32
    assert np.all(status == 0) and np.all(np.isfinite(out))
    assert same_bits(status, want_status), (status, want_status)
    assert same_bits(out, want_out), (out, want_out)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_value_path_matches_the_dense_path_of_the_same_build(name):
    o1, s1 = structured(name)
    o0, s0 = tool().evaluate(name, schur=0)
    assert np.all(s0 == 0) and np.all(s1 == 0)
    assert relerr(o1[:, 1], o0[:, 1]) < LIK_TOL, (o1[:, 1], o0[:, 1])
    assert relerr(o1, o0) < VAL_TOL, (o1, o0)


def test_all_cases_once_more_under_poison():
    """NMGP_POISON=1 (read once per process: one child for all cases) fills fresh buffers with NaNs: the epilogue's patches and
    tables hold nothing that was not written, and the bits stay the parent's."""
    env = dict(os.environ)
    env["NMGP_POISON"] = "1"
    env.pop("NMGP_SVC_SCHUR", None)
    out = subprocess.run([sys.executable, TOOL, "--print"], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    raw = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    got = {k: np.frombuffer(bytes.fromhex(h), dtype=dt).reshape(shape) for k, (dt, shape, h) in raw.items()}
    assert sorted(got) == sorted(fixture())
    for k, want in fixture().items():
        assert same_bits(got[k], want), (k, got[k], want)
