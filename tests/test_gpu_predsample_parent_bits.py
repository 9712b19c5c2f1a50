"""The six posterior-draw prediction entries (nmgp_predsample_svc / _sep / _sta / _hads / _had, nmgp_predict_hadst) on the smallest
shapes that reach every branch of their shared host schedule (ps_predict, csrc/nmgp_predsample_common.h): H = 3 draws in chunks of
2 + 1, two slices of new inputs with the second short, z given or star_in instead, both values of the entry's flag, full and
indexed form, coinciding and distinct prior factors, and per entry one call whose middle draw has a NaN parameter (its status pins
the model's status rule, its neighbours' bytes that a bad draw touches nothing else).  The cases, their inputs and the calls are
those of tools/make_predsample_fixture.py, which wrote tests/golden/predsample_parent_bits.npz with the library of the commit
before the six drivers became one: host code that only schedules the same kernels must not change one bit of `mean`, `var`, `star`
or `status`."""
import functools
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

TOOL = os.path.join(ROOT, "tools", "make_predsample_fixture.py")
CASE_NAMES = ("svc_same_z", "svc_distinct_z_unconstrained", "svc_star", "svc_nan", "sep_z_jitter", "sep_z_nojitter", "sep_star",
              "sep_nan", "sta", "sta_nan", "had_full_z", "had_ix_z", "had_full_star", "had_full_nan", "hads_full_distinct_z",
              "hads_ix_same_z", "hads_full_star", "hads_full_nan", "hadst_full", "hadst_ix", "hadst_full_nan")
NO_STAR = ("sta", "sta_nan", "hadst_full", "hadst_ix", "hadst_full_nan")


@functools.lru_cache(maxsize=None)
def tool():
    spec = importlib.util.spec_from_file_location("make_predsample_fixture", TOOL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(os.path.join(GOLDEN, "predsample_parent_bits.npz")) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def computed():
    """every case once, in one context (shared by the tests: do not write into the arrays)"""
    return tool().evaluate_all()


def keys_of(name):
    return [name + "/" + k for k in ("mean", "var", "status") + (() if name in NO_STAR else ("star",))]


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_the_cases_are_the_tools():
    assert tool().NAMES == CASE_NAMES
    assert sorted(fixture()) == sorted(k for n in CASE_NAMES for k in keys_of(n))
    assert sorted(computed()) == sorted(fixture())


@pytest.mark.parametrize("name", CASE_NAMES)
def test_entry_gives_the_parent_commits_bits(name):
    got, want = computed(), fixture()
    status = got[name + "/status"]
    assert status.dtype == np.int32 and status.shape == (3,)
    if name.endswith("_nan"):
        assert status[0] == 0 and status[1] != 0 and status[2] == 0, status
        assert np.all(np.isnan(got[name + "/mean"][1])) and np.all(np.isnan(got[name + "/var"][1]))
    else:
        assert np.all(status == 0), status
        assert all(np.all(np.isfinite(got[k])) for k in keys_of(name))
    for k in keys_of(name):
        assert got[k].dtype == (np.int32 if k.endswith("/status") else np.float64)
        assert same_bits(got[k], want[k]), (k, got[k], want[k])


def test_all_cases_once_more_under_poison():
    """NMGP_POISON=1 (read once per process: one child for all cases) fills fresh buffers with NaNs and the reused prediction
    workspace with 0xFF: the schedule reads nothing it did not write, and the bits stay the parent's."""
    env = dict(os.environ)
    env["NMGP_POISON"] = "1"
    out = subprocess.run([sys.executable, TOOL, "--print"], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    raw = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    got = {k: np.frombuffer(bytes.fromhex(h), dtype=dt).reshape(shape) for k, (dt, shape, h) in raw.items()}
    assert sorted(got) == sorted(fixture())
    for k, want in fixture().items():
        assert same_bits(got[k], want), (k, got[k], want)
