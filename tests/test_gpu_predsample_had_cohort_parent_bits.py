"""The nonseparable cohort predictor (nmgp_predsample_had_subjects) on sets A, D, E and set A padded to Nmax = 192 of
tests/hadamard_cohort_cases.py, in both forms with two draws per subject: under fixed normals, with z = NULL, with star_in, under
NMGP_PREDSAMPLE_CHUNK=1 and with a NaN in a real slot of one draw.  The cases, their inputs and the calls are those of
tools/make_predsample_had_cohort_fixture.py, which wrote tests/golden/predsample_had_cohort_parent_bits.npz (SHA-256 digests of `mean`,
`var`, `star` and `status` of every call) with the library of the commit before the entry's host function became the schedule
hadc_predict<Model> shared with the separable and the stationary cohort predictors: host code that only schedules the same launches
of the same kernels must not change one bit."""
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

TOOL = os.path.join(ROOT, "tools", "make_predsample_had_cohort_fixture.py")
FIXTURE = os.path.join(GOLDEN, "predsample_had_cohort_parent_bits.npz")


@functools.lru_cache(maxsize=None)
def tool():
    spec = importlib.util.spec_from_file_location("make_predsample_had_cohort_fixture", TOOL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def computed():
    """every case once, in one context (shared by the tests: do not write into the arrays)"""
    return tool().evaluate_all()


def test_the_cases_are_the_tools():
    keys = tool().case_keys()
    assert len(keys) == 4 * 2 * 5 * 4 and sorted(fixture()) == sorted(keys) == sorted(computed())
    assert all(v.dtype == np.uint8 and v.shape == (32,) for v in fixture().values())
    assert os.path.getsize(FIXTURE) < 1 << 20


@pytest.mark.parametrize("form", tool().FORMS)
@pytest.mark.parametrize("case", tool().CASES)
def test_entry_gives_the_parent_commits_bits(case, form):
    got, want = computed(), fixture()
    keys = [k for k in tool().case_keys() if k.startswith("%s/%s/" % (case, form))]
    assert len(keys) == 20
    for k in keys:
        assert got[k].tobytes() == want[k].tobytes(), k
    # within the fixture: the chunking and the fed-back starred values change nothing, the NaN draw changes its own row only
    for what in tool().WHAT:
        z = want["%s/%s/z/%s" % (case, form, what)].tobytes()
        assert want["%s/%s/chunk1/%s" % (case, form, what)].tobytes() == z
        assert want["%s/%s/star/%s" % (case, form, what)].tobytes() == z
        assert want["%s/%s/nan/%s" % (case, form, what)].tobytes() != z
        assert (want["%s/%s/mean/%s" % (case, form, what)].tobytes() == z) == (what == "status")


def test_all_cases_once_more_under_poison():
    """NMGP_POISON=1 (read once per process: one child for all cases) fills fresh buffers and the kept workspace with NaNs: the
    schedule reads nothing it did not write, and the bits stay the parent's."""
    env = dict(os.environ)
    env["NMGP_POISON"] = "1"
    out = subprocess.run([sys.executable, TOOL, "--print"], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    raw = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert sorted(raw) == sorted(fixture())
    for k, want in fixture().items():
        assert bytes.fromhex(raw[k]) == want.tobytes(), k
