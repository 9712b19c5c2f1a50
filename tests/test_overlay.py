"""The drop-in recipe of INTEGRATION.md section 1 against the layout of the scripts it cites: a model script's import block
(``sys.path.append(".."); import HMC_Sampler; from Utility import ...``) must run unchanged with the mirror installed, the
hot-path names must be the MI355X ones and everything else must come from the user's own checkout of the reference.

The checkout is a stand-in written by the tests themselves (``ref_checkout`` below): the reference's directory layout, model
scripts whose only content is their import lines, and a ``Utility`` folder whose modules define the helpers the scripts call
with trivial bodies -- nothing of the reference lives in this repository or is read at test time.  Its copies of the modules
the mirror provides refuse to be imported, so every test also shows that the mirror wins.  Scripts run in a child process
whose working directory is the script's folder (so that ``sys.path.append("..")`` means what it means for the script).
CPU only: importing never touches the GPU."""
import os
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# modules the mirror does not provide, as the user's checkout has them (helper names only; `from . import utils` shows that a
# passed-through module binds its package-relative imports to the mirror)
PASS_THROUGH = {
    "visualization": "def Plot_posterior(*args, **kwargs):\n    return None\n",
    "posterior_analysis": "from . import utils\n\n\ndef cov2cor(C):\n    return C\n",
    "model_validation": "def get_AIC(*args):\n    return 0.0\n",
    "preprocess_realdata": "def orig2adj(*args):\n    return args\n",
    "empirical_estimation": "from . import utils\n\n\ndef local_estimation(*args):\n    return args\n",
}
# partly mirrored modules: the names the mirror lacks are taken from the user's module of the same name
PARTLY_MIRRORED = {
    "logpos": "from . import kernels, distributions\n\n\ndef nlogpos_obj_hadamard_SVC(*args):\n    return 0.0\n",
    "utils": "".join("def %s(*args):\n    return args\n\n\n" % f for f in ("data_split", "MSE", "RMSE", "LPD")),
    "prediction": "".join("def %s(*args):\n    return args\n\n\n" % f for f in (
        "vec2pars", "vec2list", "pointwise_predsample_inhomogeneous", "test_predmap_inhomogeneous_sampling")),
}
# modules the mirror provides in full: the user's copies must never be imported
MIRRORED = ("kernels", "kronecker_operation", "distributions", "settings")
# model scripts of the three families and the post-processing folder: their import lines only
MAIN_SCRIPT = os.path.join("Nonseparable_Model", "Nonseparable_model.py")
SCRIPTS = {
    MAIN_SCRIPT: ("import sys\n"
                  "sys.path.append(\"..\")\n"
                  "import HMC_Sampler\n"
                  "from Utility import logpos, settings, utils, prediction\n"
                  "from Utility import model_validation, visualization, posterior_analysis, preprocess_realdata, empirical_estimation\n"),
    os.path.join("Nonseparable_Model", "Nonseparable_model_mpisim.py"): (
        "import sys\nsys.path.append('..')\nfrom Utility import logpos\nfrom Utility import utils\nfrom Utility import settings\n"),
    os.path.join("Separable_Model", "Separable_model.py"): (
        "import sys\nsys.path.append('..')\nfrom Utility import kernels, kronecker_operation, distributions\n"
        "from Utility import logpos, prediction, visualization\n"),
    os.path.join("Stationary_Model", "Stationary_model.py"): (
        "import sys\nsys.path.append('..')\nfrom Utility import logpos, utils\n"
        "from Utility import empirical_estimation, model_validation\n"),
    os.path.join("Post_Process", "posterior_summary.py"): (
        "import sys\nsys.path.append('..')\nfrom Utility import posterior_analysis, visualization, utils\n"),
}


@pytest.fixture(scope="module")
def ref_checkout(tmp_path_factory):
    """A stand-in checkout of the reference: returns (root, Utility dir, main script)."""
    root = tmp_path_factory.mktemp("reference_checkout")
    util = root / "Utility"
    util.mkdir()
    (util / "__init__.py").write_text("")
    for name, body in list(PASS_THROUGH.items()) + list(PARTLY_MIRRORED.items()):
        (util / (name + ".py")).write_text(body)
    for name in MIRRORED:
        (util / (name + ".py")).write_text("raise ImportError('the user\\'s %s.py was imported: the mirror must win')\n" % name)
    for rel, body in SCRIPTS.items():
        p = root / rel
        p.parent.mkdir(exist_ok=True)
        p.write_text(body)
    return str(root), str(util), str(root / MAIN_SCRIPT)


CHILD = textwrap.dedent('''
    import os, sys, types
    sys.dont_write_bytecode = True
    # (the script's external HMC package is served by the mirror's own HMC_Sampler package: no stub)
    MODE = sys.argv[1]
    if MODE == "alias":
        sys.path.insert(0, {root!r})
        import nonstationary_multivariate_gaussian_process_amd as nmgp_amd
        nmgp_amd.install_utility_alias()
    elif MODE == "alias_explicit":
        sys.path.insert(0, {root!r})
        import nonstationary_multivariate_gaussian_process_amd as nmgp_amd
        nmgp_amd.install_utility_alias(reference_utility_dir={refutil!r})
    else:                       # PYTHONPATH variant: the mirror's parent first on the path, script untouched
        assert any(p.endswith("nonstationary_multivariate_gaussian_process_amd") for p in sys.path), sys.path
    block = open({script!r}).read()          # the script's import block, run as it stands
    assert "from Utility import logpos" in block and "empirical_estimation" in block
    exec(compile(block, {script!r}, "exec"))
    mirror = os.path.join({root!r}, "nonstationary_multivariate_gaussian_process_amd", "Utility")
    # the script's `import HMC_Sampler` got the mirror's sampler package, with the entry point the model scripts call
    import inspect as _insp
    assert os.path.dirname(os.path.abspath(_insp.getsourcefile(HMC_Sampler.HMC_sampler.sampler))) == os.path.join(
        {root!r}, "nonstationary_multivariate_gaussian_process_amd", "HMC_Sampler"), HMC_Sampler
    _sig = _insp.signature(HMC_Sampler.HMC_sampler.sampler.__init__).parameters
    for _k in ("sample_size", "potential_func", "init_position", "step_size", "num_steps_in_leap", "duplicate_samples", "TensorType",
               "M", "adaptive_step_size"):
        assert _k in _sig, _k
    assert callable(HMC_Sampler.HMC_sampler.sampler.main_hmc_loop)
    def where(obj):
        import inspect
        return os.path.dirname(os.path.abspath(inspect.getsourcefile(obj)))
    # hot path: the mirror's
    assert where(logpos.nlogpos_obj_SVC) == mirror, where(logpos.nlogpos_obj_SVC)
    assert where(logpos.nlogpos_obj) == mirror and where(logpos.nlogpos_obj_S) == mirror
    assert where(prediction.pointwise_predmap_inhomogeneous) == mirror
    assert where(utils.uLvecs2Lvecs) == mirror
    import Utility
    assert where(Utility.kernels.Nonstationary_RBF_cov) == mirror
    assert where(Utility.distributions.multivariate_normal_logpdf0) == mirror
    # everything else: the user's reference checkout
    for obj in (utils.data_split, utils.MSE, utils.RMSE, utils.LPD, prediction.vec2pars, prediction.vec2list,
                prediction.pointwise_predsample_inhomogeneous,
                prediction.test_predmap_inhomogeneous_sampling, logpos.nlogpos_obj_hadamard_SVC,
                visualization.Plot_posterior, posterior_analysis.cov2cor, model_validation.get_AIC,
                preprocess_realdata.orig2adj, empirical_estimation.local_estimation):
        assert where(obj) == {refutil!r}, (obj, where(obj))
    # a passed-through module is a member of the package `Utility`: its own `from . import utils` binds to the mirror
    assert empirical_estimation.utils is utils and posterior_analysis.utils is utils
    assert settings.jitter == 1e-6 and settings.precision == 1e-6
    # host-side helpers work without a GPU, e.g. the data split the script performs at line 88
    import numpy as np, torch
    x = torch.linspace(0, 1, 20).double(); Y = torch.randn(20, 2).double()
    assert utils.uLvec2Lvec(torch.zeros(6).double(), 3).tolist() == [1, 0, 1, 0, 0, 1]
    try:
        Utility.no_such_module
    except AttributeError as e:
        assert "outside the mirrored" in str(e)
    else:
        raise AssertionError("missing submodule must raise AttributeError")
    print("OVERLAY-OK", MODE)
''')


@pytest.mark.parametrize("mode", ["alias", "alias_explicit", "pythonpath"])
def test_reference_script_import_block_runs_on_the_overlay(mode, ref_checkout):
    _, refutil, script = ref_checkout
    code = CHILD.format(root=ROOT, script=script, refutil=refutil)
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1", MPLBACKEND="Agg")
    env.pop("NMGP_REFERENCE_UTILITY", None)
    if mode == "pythonpath":
        env["PYTHONPATH"] = os.path.join(ROOT, "nonstationary_multivariate_gaussian_process_amd") + os.pathsep + \
            env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-c", code, mode], cwd=os.path.dirname(script), env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "OVERLAY-OK" in r.stdout, r.stdout + r.stderr


def test_mirror_alone_names_what_is_missing():
    """Without any reference checkout the mirror still imports, and a name outside the path fails loudly."""
    code = textwrap.dedent('''
        import sys
        sys.path.insert(0, %r)
        import nonstationary_multivariate_gaussian_process_amd as nmgp_amd
        U = nmgp_amd.install_utility_alias()
        from Utility import logpos, utils
        try:
            utils.data_split
        except AttributeError as e:
            assert "no reference checkout" in str(e), e
        else:
            raise AssertionError
        try:
            from Utility import visualization
        except ImportError as e:
            pass
        else:
            raise AssertionError
        print("ALONE-OK")
    ''' % ROOT)
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    env.pop("NMGP_REFERENCE_UTILITY", None)
    env.pop("PYTHONPATH", None)
    r = subprocess.run([sys.executable, "-c", code], cwd="/tmp", env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALONE-OK" in r.stdout, r.stdout + r.stderr


def test_utility_imports_of_every_reference_script_resolve_on_the_overlay(ref_checkout):
    """Every script of the checkout that imports from ``Utility`` (the three model families, an MPI variant, the post-processing
    folder): its ``from Utility import ...`` lines run on the overlay from the script's own directory, and every imported module
    is either a mirror module or the user's own file."""
    import glob
    ref, refutil, _ = ref_checkout
    scripts = sorted(p for p in glob.glob(os.path.join(ref, "*", "*.py"))
                     if os.path.dirname(p) != refutil and "from Utility import" in open(p).read())
    assert len(scripts) == len(SCRIPTS)
    code = textwrap.dedent('''
        import os, sys, types, re
        sys.dont_write_bytecode = True
        for name in ("seaborn", "mpi4py", "pyGPs", "statsmodels", "gpytorch"):
            sys.modules.setdefault(name, types.ModuleType(name))
        sys.path.append("..")              # what every one of these scripts does before its imports
        sys.path.insert(0, %r)
        import nonstationary_multivariate_gaussian_process_amd as nmgp_amd
        nmgp_amd.install_utility_alias()
        mirror = os.path.join(%r, "nonstationary_multivariate_gaussian_process_amd", "Utility")
        refutil = %r
        seen = set()
        for script in sys.argv[1:]:
            os.chdir(os.path.dirname(script))
            lines = [ln.strip() for ln in open(script).read().split("\\n") if re.match(r"\\s*from Utility import ", ln)]
            assert lines, script
            ns = {}
            for ln in lines:
                exec(ln, ns)
            for k, v in ns.items():
                if isinstance(v, types.ModuleType) and k != "__builtins__":
                    d = os.path.dirname(os.path.abspath(v.__file__))
                    assert d in (mirror, refutil), (script, k, d)
                    seen.add((k, d == mirror))
        mirrored = {k for k, m in seen if m}
        assert {"logpos", "kernels", "kronecker_operation", "distributions", "utils", "settings", "prediction"} <= mirrored, mirrored
        assert {"posterior_analysis", "visualization", "empirical_estimation"} <= {k for k, m in seen if not m}
        print("IMPORTS-OK", len(sys.argv) - 1)
    ''') % (ROOT, ROOT, refutil)
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1", MPLBACKEND="Agg")
    env.pop("NMGP_REFERENCE_UTILITY", None)
    r = subprocess.run([sys.executable, "-c", code] + scripts, cwd=os.path.join(ref, "Nonseparable_Model"), env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "IMPORTS-OK" in r.stdout, r.stdout + r.stderr


def test_the_users_own_hmc_sampler_package_wins(tmp_path):
    """The mirror's HMC_Sampler is a stand-in for a package the user normally HAS (the authors' sibling checkout, line 24 of the
    script appends its directory to sys.path): when one is importable, install_utility_alias() leaves it in charge, and reached
    through PYTHONPATH the mirror's package hands over to it."""
    own = tmp_path / "Hamiltonian_Monte_Carlo" / "HMC_Sampler"
    own.mkdir(parents=True)
    (own / "__init__.py").write_text("MINE = True\nfrom . import HMC_sampler\n")
    (own / "HMC_sampler.py").write_text("class sampler:\n    pass\n")
    code = textwrap.dedent('''
        import sys
        sys.path.append(%r)                  # what line 24 of the script does
        MODE = sys.argv[1]
        if MODE == "alias":
            sys.path.insert(0, %r)
            import nonstationary_multivariate_gaussian_process_amd as nmgp_amd
            nmgp_amd.install_utility_alias()
        import HMC_Sampler
        assert getattr(HMC_Sampler, "MINE", False) is True, HMC_Sampler
        assert HMC_Sampler.HMC_sampler.sampler.__module__ == "HMC_Sampler.HMC_sampler"
        print("OWN-OK", MODE)
    ''') % (str(tmp_path / "Hamiltonian_Monte_Carlo"), ROOT)
    for mode in ("alias", "pythonpath"):
        env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
        env.pop("PYTHONPATH", None)
        if mode == "pythonpath":
            env["PYTHONPATH"] = os.path.join(ROOT, "nonstationary_multivariate_gaussian_process_amd")
        r = subprocess.run([sys.executable, "-c", code, mode], cwd="/tmp", env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "OWN-OK" in r.stdout, r.stdout + r.stderr
