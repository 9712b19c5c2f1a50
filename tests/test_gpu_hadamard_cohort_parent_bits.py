"""The three cohort evaluation entries (nmgp_had_subjects_eval, nmgp_hads_subjects_eval, nmgp_hadst_subjects_eval) on the subject sets
of tests/hadamard_cohort_cases.py, the smallest that reach every mask position of the masked kernels: sets A, B, D and E with two
chains per subject (priors + gradient, no priors + gradient, value only), set A padded to Nmax = 192 (a whole padded tile), set A with
a NaN in a real slot of the middle chain of one subject (the status rule; the neighbours untouched), set A with NaN in the padded slots
only (inert; nonseparable and separable models), and one call in four chunks, each a part of one subject's chains.  The cases, their
inputs and the calls are those of tools/make_hadamard_cohort_fixture.py, which wrote tests/golden/hadamard_cohort_parent_bits.npz with
the library of the commit before the three entries came to share one chunk skeleton and one masked Gibbs kernel pair: host code that
only schedules the same launches, and kernels that compile to the same code, must not change one bit of `out`, `grad` or `status`.
Stored as SHA-256 digests instead of arrays: every array of the chunked call, and `grad` of set B and of the padded-NaN call."""
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

TOOL = os.path.join(ROOT, "tools", "make_hadamard_cohort_fixture.py")
MODELS = ("had", "sep", "sta")
CASES = ("A2", "B2", "D2", "E2", "A2_nmax192", "A3_nan_real", "A2_nan_pad", "chunk")
CALLS = tuple((case, model) for model in MODELS for case in CASES if not (case == "A2_nan_pad" and model == "sta"))


@functools.lru_cache(maxsize=None)
def tool():
    spec = importlib.util.spec_from_file_location("make_hadamard_cohort_fixture", TOOL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(os.path.join(GOLDEN, "hadamard_cohort_parent_bits.npz")) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def computed():
    """every case once, in one context (shared by the tests: do not write into the arrays)"""
    return tool().evaluate_all()


def keys_of(case, model):
    return [k for k in tool().case_keys() if k.startswith("%s/%s/" % (case, model))]


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_the_cases_are_the_tools():
    assert sorted(k for case, model in CALLS for k in keys_of(case, model)) == sorted(tool().case_keys())
    assert sorted(fixture()) == sorted(tool().case_keys())
    assert sorted(computed()) == sorted(fixture())
    assert os.path.getsize(os.path.join(GOLDEN, "hadamard_cohort_parent_bits.npz")) < 1 << 20


@pytest.mark.parametrize("case,model", CALLS)
def test_entry_gives_the_parent_commits_bits(case, model):
    got, want = computed(), fixture()
    keys = keys_of(case, model)
    assert len(keys) == (8 if case in tool().SET_CASES else 3)
    for k in keys:
        digested = case == "chunk" or (case in ("B2", "A2_nan_pad") and k.endswith("/grad"))
        assert got[k].dtype == (np.uint8 if digested else np.int32 if k.endswith("/status") else np.float64)
        assert same_bits(got[k], want[k]), (k, got[k], want[k])
    if case == "A3_nan_real":                     # chain 1 of subject 1: row 4 of 18
        from nonstationary_multivariate_gaussian_process_amd import _lib
        pre = "%s/%s/pg/" % (case, model)
        assert got[pre + "status"].tolist() == [0] * 4 + [_lib.NUM_NAN] + [0] * 13
        assert np.all(np.isnan(got[pre + "out"][4])) and not np.any(got[pre + "grad"][4])
        keep = np.arange(18) != 4
        assert np.all(np.isfinite(got[pre + "out"][keep])) and np.all(np.isfinite(got[pre + "grad"][keep]))
    elif case != "chunk":
        for k in keys:
            if k.endswith("/status"):
                assert not np.any(got[k]), (k, got[k])
            elif got[k].dtype == np.float64:
                assert np.all(np.isfinite(got[k])), k
    if case == "A2_nan_pad":                      # inert: the bytes of the call without the NaNs
        for what in ("out", "status"):
            assert same_bits(got["A2_nan_pad/%s/pg/%s" % (model, what)], got["A2/%s/pg/%s" % (model, what)])
        assert same_bits(got["A2_nan_pad/%s/pg/grad" % model], tool().digest(got["A2/%s/pg/grad" % model]))


def test_all_cases_once_more_under_poison():
    """NMGP_POISON=1 (read once per process: one child for all cases) fills fresh buffers and the kept workspace with NaNs: the
    schedule reads nothing it did not write, and the bits stay the parent's."""
    env = dict(os.environ)
    env["NMGP_POISON"] = "1"
    out = subprocess.run([sys.executable, TOOL, "--print"], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    raw = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    got = {k: np.frombuffer(bytes.fromhex(h), dtype=dt).reshape(shape) for k, (dt, shape, h) in raw.items()}
    assert sorted(got) == sorted(fixture())
    for k, want in fixture().items():
        assert same_bits(got[k], want), (k, got[k], want)
