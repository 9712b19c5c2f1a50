"""GPU half of the prediction sweep: the six complete-data prediction entries (nmgp_predict_svc / _sep / _sta, nmgp_predsample_svc /
_sep / _sta) at the subjects of tests/prediction_cases.py: every M from 1 to 8, n = M N around the 128-column chunks of the row
reductions, 63 / 64 / 65 and 256 / 260 riding rows in one slice, N = 257 for the stride-256 loops, an unsorted subject, both branches
of the shared prior factor, and every entry's slice line at S = smax, smax + 1 and 2 smax + 1.
tests/test_prediction_sweep_cpu.py holds the references to each other at these very subjects and measures TIGHT.

Bars.  Where the regression of the latent curves is involved (prior factors of condition number 1e11): the standing mean rtol 1e-5 /
atol 1e-7, variance rtol 1e-5 / atol 1e-9, starred values rtol 1e-6 / atol 1e-6.  Where it drops out (the caller's starred values,
the stationary model): TIGHT = 100 x the disagreement of the two CPU references, below 1e-8 (mean: max |a - b| / (|b| + 1e-2),
variance: relative).  One grid in one call against two halves, one noise-free draw against the deterministic predictor, the eigen
against the Cholesky formulation: rtol 1e-9 / atol 1e-11.  H draws against H calls, a batch in chunks of two, and a grid point that
lands in another slice of a posterior-draw entry: bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import prediction_cases as pc
from conftest import record_parity
from test_predsample_cpu import MEAN_TOL, STAR_TOL, VAR_TOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLOSE = dict(rtol=1e-9, atol=1e-11)
ids = dict(ids=pc.case_id)


@pytest.fixture(scope="module")
def ctx():
    from nonstationary_multivariate_gaussian_process_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def default_chunks(monkeypatch):
    monkeypatch.delenv("NMGP_PREDSAMPLE_CHUNK", raising=False)


def same_bits(a, b):
    return all(np.array_equal(u, v, equal_nan=True) for u, v in zip(a, b))


def check(case_name, **errs):
    """print, record, then assert every (achieved, bar)"""
    print(case_name, {k: v[0] for k, v in errs.items()})
    record_parity(case_name, **errs)
    for k, (e, tol) in errs.items():
        assert e < tol, (case_name, k, e, tol)


def name(entry, case, *rest):
    return "/".join(("psweep", entry, pc.case_id(case)) + tuple(str(r) for r in rest))


def standing(mean, var, ref, star=None):
    """{quantity: (achieved, bar)} at the standing bars: (mean, var[, star]) against ref"""
    errs = dict(mean=(pc.allclose_err(mean, ref[0], **MEAN_TOL), MEAN_TOL["rtol"]), var=(pc.allclose_err(var, ref[1], **VAR_TOL), VAR_TOL["rtol"]))
    if star is not None:
        errs["star"] = (pc.allclose_err(star, ref[2], **STAR_TOL), STAR_TOL["rtol"])
    return errs


def tight(mean, var, ref):
    bar = pc.tight()[1]
    assert 0.0 < bar <= 1e-8
    return dict(tight_mean=(pc.mean_err(mean, ref[0]), bar), tight_var=(pc.var_err(var, ref[1]), bar))


def whole(out, shape):
    """every output has its shape, is finite and was written"""
    for a, sh in zip(out, shape):
        assert a.shape == sh and np.all(np.isfinite(a)), (a.shape, sh)


# ---- the entries against the references -----------------------------------------------------------------------------------------------
def run_deterministic(ctx, case, hy, S, models=("svc", "sep", "sta"), tag="short"):
    """The deterministic predictors on draw 0 at pc.grid(x, S) against the dense oracle, and in two halves against themselves."""
    c = pc.build(case)
    M, T, P = c["M"], c["T"], c["pars"]
    ref = pc.oracle(case, hy, S)
    xs, k = ref["xs"], S // 2
    out = {}
    if "svc" in models:
        hv = pc.HYPERS["svc"][hy]
        mean, var, Ls = out["svc"] = ctx.predict_svc(P["svc"][0], hv, xs)
        whole(out["svc"], [(S, M), (S, M), (S, T)])
        check(name("predict_svc", case, hy, tag, S), **standing(mean, var, ref["svc"], Ls))
        a, b = ctx.predict_svc(P["svc"][0], hv, xs[:k]), ctx.predict_svc(P["svc"][0], hv, xs[k:])
        for u, v, w in zip(out["svc"], a, b):
            np.testing.assert_allclose(np.concatenate([v, w]), u, **CLOSE)
    if "sep" in models:
        hv = pc.HYPERS["sep"][hy]
        mean, var = out["sep"] = ctx.predict_sep(P["sep"][0], hv, xs)
        whole(out["sep"], [(S, M), (S, M)])
        check(name("predict_sep", case, hy, tag, S), **standing(mean, var, ref["sep"]))
        a, b = ctx.predict_sep(P["sep"][0], hv, xs[:k]), ctx.predict_sep(P["sep"][0], hv, xs[k:])
        for u, v, w in zip(out["sep"], a, b):
            np.testing.assert_allclose(np.concatenate([v, w]), u, **CLOSE)
    if "sta" in models:
        mean, var = out["sta"] = ctx.predict_sta(P["sta"][0], xs)
        whole(out["sta"], [(S, M), (S, M)])
        check(name("predict_sta", case, tag, S), **tight(mean, var, ref["sta"]))
        a, b = ctx.predict_sta(P["sta"][0], xs[:k]), ctx.predict_sta(P["sta"][0], xs[k:])
        for u, v, w in zip(out["sta"], a, b):
            np.testing.assert_allclose(np.concatenate([v, w]), u, **CLOSE)
    return out


def run_drawn(ctx, case, hy, S, models=("svc", "sep", "sta"), tag="short"):
    """The posterior-draw entries with the regression, under fixed normals, against the restatements; the grid without its first
    two points keeps every remaining point's bits.  Points move to ANOTHER SLICE by that cut only where the grid spans several slices:
    the slice-line grids of pc.EDGE_GRIDS (N = 9, M = 7; S = smax + 1 and 2 smax + 1) and the 7-point grid of the subjects with N <= 8.
    Everywhere else all points sit in one slice, and the check is that a shorter grid (fewer riding rows, another leading dimension)
    keeps the bits."""
    c = pc.build(case)
    M, T, P = c["M"], c["T"], c["pars"]
    ref = pc.drawn(case, hy, S)
    xs = ref["xs"]
    if "svc" in models:
        hv, z = pc.HYPERS["svc"][hy], ref["z_svc"]
        for flag in (True, False):
            mean, var, star, status = ctx.predsample_svc(P["svc"], hv, xs, z=z, constrained=flag)
            whole((mean, var, star), [(pc.H, S, M), (pc.H, S, M), (pc.H, S, 1 + T)])
            assert status.tolist() == [0] * pc.H
            check(name("predsample_svc", case, hy, tag, S, "constrained%d" % flag), **standing(mean, var, ref[("svc", flag)], star))
            cut = ctx.predsample_svc(P["svc"], hv, xs[2:], z=z[:, 2:], constrained=flag)
            assert same_bits([mean[:, 2:], var[:, 2:], star[:, 2:]], cut[:3])
    if "sep" in models:
        hv, z = pc.HYPERS["sep"][hy], ref["z_sep"]
        for flag in (True, False):
            mean, var, star, status = ctx.predsample_sep(P["sep"], hv, xs, z=z, kss_jitter=flag)
            whole((mean, var, star), [(pc.H, S, M), (pc.H, S, M), (pc.H, S, 2)])
            assert status.tolist() == [0] * pc.H
            check(name("predsample_sep", case, hy, tag, S, "kss_jitter%d" % flag), **standing(mean, var, ref[("sep", flag)], star))
            cut = ctx.predsample_sep(P["sep"], hv, xs[2:], z=z[:, 2:], kss_jitter=flag)
            assert same_bits([mean[:, 2:], var[:, 2:], star[:, 2:]], cut[:3])
    if "sta" in models:
        mean, var, status = ctx.predsample_sta(P["sta"], xs)
        whole((mean, var), [(pc.H, S, M), (pc.H, S, M)])
        assert status.tolist() == [0] * pc.H
        check(name("predsample_sta", case, tag, S), **tight(mean, var, ref["sta"]))
        cut = ctx.predsample_sta(P["sta"], xs[2:])
        assert same_bits([mean[:, 2:], var[:, 2:]], cut[:2])


# ---- a. the deterministic predictors ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hy", pc.HYPER_SETS)
@pytest.mark.parametrize("case", pc.SUBJECTS, **ids)
def test_deterministic_predictors_meet_the_dense_oracle(ctx, case, hy):
    c = pc.build(case)
    ctx.set_data(c["x"], c["Y"])
    run_deterministic(ctx, case, hy, pc.S_SHORT, ("svc", "sep", "sta") if hy == "same" else ("svc", "sep"))


@pytest.mark.parametrize("case", pc.EIG, **ids)
def test_eigen_formulation_meets_the_oracle_and_the_cholesky_formulation(ctx, case):
    from nonstationary_multivariate_gaussian_process_amd import _lib
    c = pc.build(case)
    os.environ["NMGP_SEP"] = "eig"
    try:
        eig = _lib.Context(0)
    finally:
        os.environ.pop("NMGP_SEP", None)
    try:
        for k in (ctx, eig):
            k.set_data(c["x"], c["Y"])
        for hy in pc.HYPER_SETS:
            out = run_deterministic(eig, case, hy, pc.S_SHORT, ("sep", "sta") if hy == "same" else ("sep",), tag="eig")
            chol = ctx.predict_sep(c["pars"]["sep"][0], pc.HYPERS["sep"][hy], pc.grid(c["x"], pc.S_SHORT))
            for u, v in zip(out["sep"], chol):
                np.testing.assert_allclose(u, v, **CLOSE)
            if "sta" in out:
                chol = ctx.predict_sta(c["pars"]["sta"][0], pc.grid(c["x"], pc.S_SHORT))
                for u, v in zip(out["sta"], chol):
                    np.testing.assert_allclose(u, v, **CLOSE)
    finally:
        eig.close()


# ---- b. the posterior-draw entries with the regression ---------------------------------------------------------------------------------
@pytest.mark.parametrize("hy", pc.HYPER_SETS)
@pytest.mark.parametrize("case", pc.SUBJECTS, **ids)
def test_posterior_draw_entries_meet_the_restatements(ctx, case, hy):
    c = pc.build(case)
    ctx.set_data(c["x"], c["Y"])
    run_drawn(ctx, case, hy, pc.S_SHORT, ("svc", "sep", "sta") if hy == "same" else ("svc", "sep"))


# ---- c. the caller's starred values: no regression, the tight bar ---------------------------------------------------------------------
@pytest.mark.parametrize("case", pc.SUBJECTS, **ids)
def test_posterior_draw_entries_on_the_callers_starred_values_meet_the_tight_bar(ctx, case):
    c = pc.build(case)
    M, P = c["M"], c["pars"]
    ctx.set_data(c["x"], c["Y"])
    ref = pc.starred(case)
    xs, S = ref["xs"], pc.S_SHORT
    for flag in (True, False):
        mean, var, star, status = ctx.predsample_svc(P["svc"], pc.HYPERS["svc"]["diff"], xs, star=ref["star_svc"], constrained=flag)
        whole((mean, var), [(pc.H, S, M), (pc.H, S, M)])
        assert status.tolist() == [0] * pc.H and np.array_equal(star, ref["star_svc"])
        check(name("predsample_svc", case, "star_in", "constrained%d" % flag), **tight(mean, var, ref["svc"]))
        mean, var, star, status = ctx.predsample_sep(P["sep"], pc.HYPERS["sep"]["diff"], xs, star=ref["star_sep"], kss_jitter=flag)
        whole((mean, var), [(pc.H, S, M), (pc.H, S, M)])
        assert status.tolist() == [0] * pc.H and np.array_equal(star, ref["star_sep"])
        check(name("predsample_sep", case, "star_in", "kss_jitter%d" % flag), **tight(mean, var, ref[("sep", flag)]))


# ---- d. exactness ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pc.SUBJECTS, **ids)
def test_batches_chunks_and_noise_free_draws(ctx, case, monkeypatch):
    c = pc.build(case)
    T, P = c["T"], c["pars"]
    ctx.set_data(c["x"], c["Y"])
    S = pc.S_SHORT
    xs = pc.grid(c["x"], S)
    zv, zs = pc.normals(case, S, 1 + T), pc.normals(case, S, 2)
    hy = pc.HYPER_SETS[pc.SUBJECTS.index(case) % 2]                      # the subjects alternate between the two sets
    hv, hs = pc.HYPERS["svc"][hy], pc.HYPERS["sep"][hy]
    calls = {"svc1": lambda h: ctx.predsample_svc(P["svc"][h], hv, xs, z=zv[h], constrained=True),
             "svc0": lambda h: ctx.predsample_svc(P["svc"][h], hv, xs, z=zv[h], constrained=False),
             "sep1": lambda h: ctx.predsample_sep(P["sep"][h], hs, xs, z=zs[h], kss_jitter=True),
             "sep0": lambda h: ctx.predsample_sep(P["sep"][h], hs, xs, z=zs[h], kss_jitter=False),
             "sta": lambda h: ctx.predsample_sta(P["sta"][h], xs)}
    every = slice(0, pc.H)
    for key, call in calls.items():
        big = call(every)
        assert big[-1].tolist() == [0] * pc.H and not np.array_equal(big[0][0], big[0][1]), key
        for h in range(pc.H):
            assert same_bits([a[h:h + 1] for a in big], call(slice(h, h + 1))), (key, h)
        monkeypatch.setenv("NMGP_PREDSAMPLE_CHUNK", "2")
        chunked = call(every)
        monkeypatch.delenv("NMGP_PREDSAMPLE_CHUNK")
        assert same_bits(big, chunked), key
    # one draw without noise is the deterministic predictor
    m0, v0, L0 = ctx.predict_svc(P["svc"][0], hv, xs)
    mean, var, star, status = ctx.predsample_svc(P["svc"][0], hv, xs, constrained=False)
    assert status.tolist() == [0]
    check(name("predsample_svc", case, hy, "vs_predict_svc"), mean_rtol_1e9_atol_1e11=(pc.allclose_err(mean[0], m0, **CLOSE), 1e-9),
          var_rtol_1e9_atol_1e11=(pc.allclose_err(var[0], v0, **CLOSE), 1e-9), Lstar_rtol_1e9_atol_1e11=(pc.allclose_err(star[0][:, 1:], L0, **CLOSE), 1e-9))
    m0, v0 = ctx.predict_sep(P["sep"][0], hs, xs)
    mean, var, star, status = ctx.predsample_sep(P["sep"][0], hs, xs, kss_jitter=True)         # (predict_sep's k** carries the jitter)
    assert status.tolist() == [0]
    check(name("predsample_sep", case, hy, "vs_predict_sep"), mean_rtol_1e9_atol_1e11=(pc.allclose_err(mean[0], m0, **CLOSE), 1e-9),
          var_rtol_1e9_atol_1e11=(pc.allclose_err(var[0], v0, **CLOSE), 1e-9))
    m0, v0 = ctx.predict_sta(P["sta"][0], xs)
    mean, var, status = ctx.predsample_sta(P["sta"][0], xs)
    assert status.tolist() == [0]
    check(name("predsample_sta", case, "vs_predict_sta"), mean_rtol_1e9_atol_1e11=(pc.allclose_err(mean[0], m0, **CLOSE), 1e-9),
          var_rtol_1e9_atol_1e11=(pc.allclose_err(var[0], v0, **CLOSE), 1e-9))


# ---- e. slice lines and riding-row edges -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,entry,S", pc.EDGE_GRIDS, ids=["%s_%s_S%d" % (pc.case_id(g[0]), g[1], g[2]) for g in pc.EDGE_GRIDS])
def test_slice_lines_and_riding_row_edges(ctx, case, entry, S):
    c = pc.build(case)
    ctx.set_data(c["x"], c["Y"])
    models = pc.EDGE_MODELS[entry]
    for hy in pc.HYPER_SETS:
        if entry != "predsample_svc":
            run_deterministic(ctx, case, hy, S, [m for m in models if m != "sta" or hy == "same"], tag=entry)
        if entry != "predict_svc":
            run_drawn(ctx, case, hy, S, [m for m in models if m != "sta" or hy == "same"], tag=entry)


POISON_SNIPPET = r'''
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np
import prediction_cases as pc
from nonstationary_multivariate_gaussian_process_amd import _lib
ctx = _lib.Context(0)
for case, entry, S in pc.EDGE_GRIDS:
    c = pc.build(case)
    M, T, P = c["M"], c["T"], c["pars"]
    ctx.set_data(c["x"], c["Y"])
    xs = pc.grid(c["x"], S)
    for hy in pc.HYPER_SETS:                      # 'same': the two priors share one factor (W1 aliases W0), 'diff': two factors
        hv, hs = pc.HYPERS["svc"][hy], pc.HYPERS["sep"][hy]
        out, status = [], []
        if entry == "predict_svc":
            out += ctx.predict_svc(P["svc"][0], hv, xs)
        elif entry == "predsample_svc":
            for flag in (True, False):
                *a, st = ctx.predsample_svc(P["svc"], hv, xs, z=pc.normals(case, S, 1 + T), constrained=flag)
                out, status = out + a, status + [st]
        else:
            out += list(ctx.predict_sep(P["sep"][0], hs, xs)) + list(ctx.predict_sta(P["sta"][0], xs))
            for flag in (True, False):
                *a, st = ctx.predsample_sep(P["sep"], hs, xs, z=pc.normals(case, S, 2), kss_jitter=flag)
                out, status = out + a, status + [st]
            *b, st = ctx.predsample_sta(P["sta"], xs)
            out, status = out + b, status + [st]
        assert all(np.all(np.isfinite(a)) for a in out) and not any(st.any() for st in status), (case, entry, S, hy, status)
ctx.close()
print("POISON_OK", len(pc.EDGE_GRIDS))
'''


def test_slice_lines_and_riding_row_edges_under_poison():
    """NMGP_POISON=1 (read once per process: a child) fills fresh buffers with NaNs: an output element that no slice wrote shows up."""
    env = dict(os.environ)
    env["NMGP_POISON"] = "1"
    env.pop("NMGP_PREDSAMPLE_CHUNK", None)
    out = subprocess.run([sys.executable, "-c", POISON_SNIPPET % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}],
                         capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0 and "POISON_OK %d" % len(pc.EDGE_GRIDS) in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


# ---- f. status -------------------------------------------------------------------------------------------------------------------------
def test_a_zero_third_pivot_is_reported_for_its_draw_only(ctx):
    """sigma2_err = exp(-800) = 0 and L_2[0, 0] = exp(-800) = 0 make row 2 of output 0 of Sigma exactly 0 (finite inputs throughout):
    the third pivot is exactly 0 and LAPACK's rule `pivot <= 0` names minor 3."""
    from scipy.linalg import lapack
    from nonstationary_multivariate_gaussian_process_amd import _lib
    from oracle import nmgp_oracle as O
    case = pc.MINOR
    c = pc.build(case)
    N, M, T, P = c["N"], c["M"], c["T"], c["pars"]["svc"]
    bad = P[1].copy()
    bad[-1] = -800.0
    bad[N + 2 * T] = -800.0
    Sigma = O.svc_covariance(*O.vec2pars_SVC(bad, N, M), c["x"], M)
    assert np.all(np.isfinite(Sigma)) and not Sigma[2].any() and lapack.dpotrf(Sigma, lower=1)[1] == 3
    ctx.set_data(c["x"], c["Y"])
    xs = pc.grid(c["x"], pc.S_SHORT)
    z = pc.normals(case, pc.S_SHORT, 1 + T)
    hv = pc.HYPERS["svc"]["diff"]
    clean = ctx.predsample_svc(P[[0, 2]], hv, xs, z=z[[0, 2]])
    assert clean[3].tolist() == [0, 0] and np.all(np.isfinite(clean[0]))
    mean, var, star, status = ctx.predsample_svc(np.stack([P[0], bad, P[2]]), hv, xs, z=z)
    print("predsample_svc status", status.tolist())
    assert status.tolist() == [0, 3, 0]
    assert np.all(np.isnan(mean[1])) and np.all(np.isnan(var[1]))
    assert same_bits([a[[0, 2]] for a in (mean, var, star)], clean[:3])
    with pytest.raises(_lib.NmgpNumericalError) as err:
        ctx.predict_svc(bad, hv, xs)
    assert err.value.code == 3


@pytest.mark.parametrize("case", [(64, 2, "even"), (40, 8, "even")], **ids)
def test_a_nan_draw_of_the_separable_and_stationary_entries_leaves_its_neighbours_alone(ctx, case):
    c = pc.build(case)
    N, P = c["N"], c["pars"]
    ctx.set_data(c["x"], c["Y"])
    xs = pc.grid(c["x"], pc.S_SHORT)
    z = pc.normals(case, pc.S_SHORT, 2)
    hs = pc.HYPERS["sep"]["diff"]
    bad = P["sep"].copy()
    bad[1, N // 2] = np.nan
    clean = ctx.predsample_sep(P["sep"], hs, xs, z=z)
    mean, var, star, status = ctx.predsample_sep(bad, hs, xs, z=z)
    assert clean[3].tolist() == [0, 0, 0] and status[1] != 0 and status[[0, 2]].tolist() == [0, 0]
    assert np.all(np.isnan(mean[1])) and np.all(np.isnan(var[1]))
    assert same_bits([a[[0, 2]] for a in (mean, var, star)], [a[[0, 2]] for a in clean[:3]])
    bad = P["sta"].copy()
    bad[1, 0] = np.nan
    clean = ctx.predsample_sta(P["sta"], xs)
    mean, var, status = ctx.predsample_sta(bad, xs)
    assert clean[2].tolist() == [0, 0, 0] and status[1] != 0 and status[[0, 2]].tolist() == [0, 0]
    assert np.all(np.isnan(mean[1])) and np.all(np.isnan(var[1]))
    assert same_bits([a[[0, 2]] for a in (mean, var)], [a[[0, 2]] for a in clean[:2]])


# ---- g. the Python mirror away from three outputs --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pc.MIRROR, **ids)
def test_python_mirror_slices_the_parameter_vector_for_other_numbers_of_outputs(ctx, case):
    from nonstationary_multivariate_gaussian_process_amd import predsample as ps
    from nonstationary_multivariate_gaussian_process_amd.Utility import prediction as up
    c = pc.build(case)
    N, M, T, P = c["N"], c["M"], c["T"], c["pars"]
    S = pc.S_SHORT
    xs = pc.grid(c["x"], S)
    t = torch.from_numpy
    Y, x, g = t(c["Y"]), t(c["x"]), t(xs)

    def pct_of(mean, var):
        return np.stack([mean - 1.96 * np.sqrt(var), mean, mean + 1.96 * np.sqrt(var)], axis=1)

    hv = pc.HYPERS["svc"]["diff"]
    ctx.set_data(c["x"], c["Y"])
    mean, var, Ls = ctx.predict_svc(P["svc"][0], hv, xs)
    p = P["svc"][0]
    pct, Lm = up.pointwise_predmap_inhomogeneous(t(p[:N].copy()), t(p[N:N + N * T].copy()), t(p[-1:].copy())[0], Y, x, g, *hv[:6])
    assert tuple(pct.shape) == (S, 3, M) and tuple(Lm.shape) == (S, T)
    assert np.array_equal(pct.numpy()[:, 1], mean) and np.array_equal(Lm.numpy(), Ls)
    np.testing.assert_allclose(pct.numpy(), pct_of(mean, var), rtol=1e-14)
    hs = pc.HYPERS["sep"]["diff"]
    mean, var = ctx.predict_sep(P["sep"][0], hs, xs)
    p = P["sep"][0]
    pct = up.pointwise_predmap(t(p[:N].copy()), t(p[N:2 * N].copy()), t(p[2 * N:2 * N + T].copy()), t(p[-1:].copy())[0], Y, x, g, *hs[:6])
    assert tuple(pct.shape) == (S, 3, M) and np.array_equal(pct.numpy()[:, 1], mean)
    np.testing.assert_allclose(pct.numpy(), pct_of(mean, var), rtol=1e-14)
    mean, var = ctx.predict_sta(P["sta"][0], xs)
    p = P["sta"][0]
    pct = up.pointwise_predmap_S(t(p[:1].copy())[0], t(p[1:2].copy())[0], t(p[2:2 + T].copy()), t(p[-1:].copy())[0], Y, x, g)
    assert tuple(pct.shape) == (S, 3, M) and np.array_equal(pct.numpy()[:, 1], mean)
    np.testing.assert_allclose(pct.numpy(), pct_of(mean, var), rtol=1e-14)
    # the posterior-draw family: [N_grid, N_hist, M] samples from the entry's moments and the caller's normals
    z = np.random.default_rng(pc.case_seed(case) + 2).standard_normal((S, pc.H, 1 + T + M))
    d = P["svc"]
    ys = ps.pointwise_predsample_inhomogeneous(t(d[:, :N].copy()), t(d[:, N:N + N * T].copy()), t(d[:, -1].copy()), Y, x, g, *hv[:6],
                                               N_sample=pc.H, z=z)
    mean, var, _, status = ctx.predsample_svc(d, hv, xs, z=pc.sd(z[:, :, :1 + T]))
    assert isinstance(ys, np.ndarray) and ys.shape == (S, pc.H, M) and status.tolist() == [0] * pc.H
    np.testing.assert_allclose(ys, pc.sd(mean) + np.sqrt(pc.sd(var)) * z[:, :, 1 + T:], rtol=1e-13, atol=1e-15)
