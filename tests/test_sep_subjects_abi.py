"""CPU-only: the separable subject-set entries are declared in include/nmgp.h, exported by the built library and bound by the
ctypes table (as tests/test_abi.py checks the whole surface), and the Python layers above them exist."""
import ctypes
import inspect
import os
import re
import subprocess

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "nmgp.h")
ENTRIES = {
    "nmgp_sep_batch_set_subjects_chains": r"int\s+nmgp_sep_batch_set_subjects_chains\s*\(\s*nmgp_ctx\s*\*\s*\w+,\s*const\s+double\s*\*\s*x,"
                                          r"\s*const\s+double\s*\*\s*Y,\s*int\s+S,\s*int\s+chains_per_subject\s*\)\s*;",
    "nmgp_sep_batch_clear_subjects": r"int\s+nmgp_sep_batch_clear_subjects\s*\(\s*nmgp_ctx\s*\*\s*\w+\s*\)\s*;",
}


def test_header_declares_the_subject_set_entries():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, decl in ENTRIES.items():
        assert re.search(decl, src), "%s is not declared in nmgp.h with the documented signature" % name


def test_library_exports_and_binding_carries_the_subject_set_entries():
    from nonstationary_multivariate_gaussian_process_amd import build as b, _lib
    lib_path = b.build(verbose=False)
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib_path]).decode()
    exported = set(re.findall(r" T (nmgp_[a-z0-9_]+)", out))
    for name in ENTRIES:
        assert name in exported, "%s is not exported by %s" % (name, lib_path)
    I, V, P = ctypes.c_int, ctypes.c_void_p, _lib.c_double_p
    assert _lib.SIGNATURES["nmgp_sep_batch_set_subjects_chains"] == (I, [V, P, P, I, I])
    assert _lib.SIGNATURES["nmgp_sep_batch_clear_subjects"] == (I, [V])
    lib = _lib.load(require_gpu=False)
    assert lib.nmgp_sep_batch_set_subjects_chains.argtypes == [V, P, P, I, I]
    # no context: both entries refuse a NULL handle instead of touching it
    assert lib.nmgp_sep_batch_set_subjects_chains(None, None, None, 1, 1) == -1
    assert lib.nmgp_sep_batch_clear_subjects(None) == -1


def test_python_layers_expose_the_subject_set():
    from nonstationary_multivariate_gaussian_process_amd import _lib, drivers
    sig = inspect.signature(_lib.Context.sep_batch_set_subjects)
    assert list(sig.parameters) == ["self", "xs", "Ys", "chains_per_subject"] and sig.parameters["chains_per_subject"].default == 1
    assert list(inspect.signature(_lib.Context.sep_batch_clear_subjects).parameters) == ["self"]
    sig = inspect.signature(drivers.BatchedMAPSeparable.__init__)
    assert list(sig.parameters) == ["self", "xs", "Ys", "hyper_pars", "init_pars", "lr", "ctx", "chains_per_subject"]
    assert sig.parameters["lr"].default == 2e-1 and sig.parameters["chains_per_subject"].default == 1
    assert issubclass(drivers.BatchedMAPSeparable, drivers.LockStepMAP)
