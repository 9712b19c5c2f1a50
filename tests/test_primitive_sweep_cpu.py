"""CPU half of the primitive sweep (tests/primitive_cases.py, GPU half: tests/test_gpu_primitive_sweep.py): the float64 oracle, the
mirror's _host_* restatements and the reference fixture prims.npz are held to the longdouble references within the very bars the
device entries are held to, on the very cases they run.  A flaw in a bar's derivation shows up here, not as a GPU failure.  The
conditions on the inputs are asserted too: no covariance value so small that a relative comparison would lose it, no exponent beyond
600, every bar of the density / inverse entries at or below the 1e-10 of the fixture test."""
import numpy as np
import pytest
import torch

import primitive_cases as pc
from conftest import golden
from oracle import nmgp_oracle as O

pytestmark = pytest.mark.skipif(not np.finfo(np.longdouble).eps < 1e-18,
                                reason="numpy.longdouble is no wider than float64 here: the references need its 64-bit mantissa")

ids = dict(ids=pc.case_id)


def t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def inside(name, achieved, bar):
    print(name, achieved, bar)
    assert achieved <= bar, (name, achieved, bar)


def test_longdouble_is_wider_than_float64():
    assert np.finfo(np.longdouble).eps < 1e-18


def test_longdouble_cholesky_and_substitution_reproduce_their_input():
    rng = np.random.default_rng(0)
    S = pc.ld(pc.spd_B(40, rng)) + pc.LD(0.1) * np.eye(40, dtype=pc.LD)
    logdet, inv, L = pc.spd_ld(S)
    assert float(np.max(np.abs(L @ L.T - S))) < 1e-17 * float(np.max(np.abs(S)))
    assert float(np.max(np.abs(inv @ S - np.eye(40)))) < 1e-15
    assert abs(float(logdet) - np.linalg.slogdet(S.astype(np.float64))[1]) < 1e-11
    assert np.array_equal(pc.sym_upper(pc.nan_lower(S.astype(np.float64))), S.astype(np.float64))


@pytest.mark.parametrize("case", pc.RECT, **ids)
def test_rect_oracle_and_host_restatements_inside_the_bars(case):
    from nonstationary_multivariate_gaussian_process_amd.Utility import kernels as k
    c, refs = pc.rect_inputs(case), pc.rect_refs(case)
    n1, n2, d, shift = case
    assert c["x1"].shape == (n1, d) and c["x2"].shape == (n2, d)
    assert np.all(c["x1"] >= shift) and np.all(c["x1"] < shift + 1) and np.all(c["x2"] >= shift) and np.all(c["x2"] < shift + 1)
    # conditions: no element is left out of a relative comparison, no exponent beyond 600
    for key, ref in refs.items():
        if key[0] != "dist":
            assert float(ref[0].min()) > 1e-290 and ref[2] <= 600.0, (key, float(ref[0].min()), ref[2])
    for form, x2 in (("sym", None), ("sep", c["x2"])):
        inside("oracle dist " + form, pc.frac(O.pairwise_distances(c["x1"], x2), *refs[("dist", form)]), 1.0)
        inside("host dist " + form, pc.frac(k._host_sqdist(t(c["x1"]), t(x2)).numpy(), *refs[("dist", form)]), 1.0)
        inside("oracle rbf " + form, pc.frac(O.RBF_cov(c["x1"], x2, pc.ALPHA, pc.BETA), *refs[("rbf", form)][:2]), 1.0)
        inside("host rbf " + form, pc.frac(k._host_rbf(t(c["x1"]), t(x2), pc.ALPHA, pc.BETA).numpy(), *refs[("rbf", form)][:2]), 1.0)
    for form in pc.GIBBS_SYM + ["sep"]:
        args = pc.gibbs_args(case, form)
        inside("oracle gibbs %s" % (form,), pc.frac(O.Nonstationary_RBF_cov(*args), *refs[("gibbs", form)][:2]), 1.0)
        targs = [t(a) for a in args] + [None] * (6 - len(args))
        inside("host gibbs %s" % (form,), pc.frac(k._host_gibbs(*targs).numpy(), *refs[("gibbs", form)][:2]), 1.0)
    # the properties the device entries are held to bit for bit: the reference has them by construction
    for key in [("dist", "sym"), ("rbf", "sym")] + [("gibbs", f) for f in pc.GIBBS_SYM]:
        assert np.array_equal(refs[key][0], refs[key][0].T)
    assert not np.diag(refs[("dist", "sym")][0]).any()
    assert np.array_equal(np.diag(refs[("rbf", "sym")][0]), np.full(n1, pc.LD(pc.JITTER) + pc.LD(pc.ALPHA) ** 2))


@pytest.mark.parametrize("case", pc.KRON, **ids)
def test_kron_product_oracle_is_numpy_kron_bit_for_bit(case):
    a, b = pc.kron_inputs(case)
    assert a.shape == case[0] and b.shape == case[1]
    assert np.array_equal(O.kronecker_product(a, b), np.kron(a, b))
    assert np.array_equal(torch.kron(t(a), t(b)).numpy(), np.kron(a, b))      # the mirror's host restatement


@pytest.mark.parametrize("case", pc.KMV, **ids)
def test_kron_mv_oracle_and_host_restatement_inside_the_bar(case):
    from nonstationary_multivariate_gaussian_process_amd.Utility import kronecker_operation as ko
    B, K, y = pc.kmv_inputs(case)
    ref, bar = pc.kmv_ref(case)
    assert ref.shape == (case[0] * case[2],)
    inside("oracle kron_mv", pc.frac(O.kron_mv(B, K, y), ref, bar), 1.0)
    inside("dense kron_mv", pc.frac(np.kron(B, K) @ y, ref, bar), 1.0)
    inside("host kron_mv", pc.frac(ko._host_kron_mv(t(B), t(K), t(y)).numpy(), ref, bar), 1.0)


@pytest.mark.parametrize("case", pc.DENS, **ids)
def test_density_and_inverse_oracle_and_host_restatements_inside_the_bars(case):
    from nonstationary_multivariate_gaussian_process_amd.Utility import distributions as dist
    from nonstationary_multivariate_gaussian_process_amd.Utility import kronecker_operation as ko
    c, r = pc.dens_inputs(case), pc.dens_ref(case)
    B, K, y, mu, s2 = c["B"], c["K"], c["y"], c["mu"], c["sigma2"]
    assert np.array_equal(B, B.T) and np.array_equal(K, K.T) and mu.any()
    print("cond", r["cond"], "d_cpu", r["d_cpu"], "bars", r["bars"])
    # condition: every bar of item 5 at or below the bar of the fixture test
    assert all(0.0 < b <= 1e-10 for b in r["bars"].values()), r["bars"]
    lp = O.multivariate_normal_logpdf(y, mu, r["logdet64"], r["inv64"])
    oracle = (O.multivariate_normal_logpdf0(y, mu, B, K, s2), O.multivariate_normal_logpdf2(y, mu, B, K, s2),
              O.kron_logdet(s2, B, K), O.kron_logdet(s2, B, K), O.kron_inv(s2, B, K), lp)
    for name, (e, bar) in pc.dens_errs(case, oracle).items():
        inside("oracle " + name, e, bar)
    ts2 = torch.tensor(s2, dtype=torch.float64)
    hk = float(dist._host_mvn_kron(t(y), t(mu), t(B), t(K), ts2))
    hld = float(ko._host_kron_logdet(ts2, t(B), t(K)))
    hlp = float(dist._host_mvn(t(y), t(mu), torch.tensor(r["logdet64"], dtype=torch.float64), t(r["inv64"])))
    host = (hk, hk, hld, hld, ko._host_kron_inv(ts2, t(B), t(K)).numpy(), hlp)
    for name, (e, bar) in pc.dens_errs(case, host).items():
        inside("host " + name, e, bar)


@pytest.mark.parametrize("n", sorted(pc.MVN))
def test_mvn_logpdf_oracle_and_host_restatement_inside_the_bar(n):
    from nonstationary_multivariate_gaussian_process_amd.Utility import distributions as dist
    c = pc.mvn_inputs(n)
    assert c["inv"].shape == (n, n) and np.all(np.isfinite(c["inv"])) and np.isfinite(c["logdet"])
    for mu in (None, c["mu"]):
        ref, bar = pc.ref_mvn(c["y"], mu, c["logdet"], c["inv"])
        m0 = np.zeros(n) if mu is None else mu
        inside("oracle mvn_logpdf", abs(float(pc.LD(O.multivariate_normal_logpdf(c["y"], m0, c["logdet"], c["inv"])) - ref)), bar)
        host = float(dist._host_mvn(t(c["y"]), t(m0), torch.tensor(c["logdet"], dtype=torch.float64), t(c["inv"])))
        inside("host mvn_logpdf", abs(float(pc.LD(host) - ref)), bar)


def test_kronecker_inverse_of_the_large_mvn_cases_is_the_dense_longdouble_inverse():
    """S = A kron C: A^-1 kron C^-1 and q log det A + p log det C against the dense longdouble factorisation of S itself, at an order
    where that is cheap, with the generator of pc.mvn_inputs."""
    rng = np.random.default_rng(9)
    A, C = pc.spd_B(5, rng), pc.gibbs_K(7, rng) + pc.SIGMA2 * np.eye(7)
    ldA, invA, _ = pc.spd_ld(pc.ld(A))
    ldC, invC, _ = pc.spd_ld(pc.ld(C))
    logdet, inv, _ = pc.spd_ld(np.kron(pc.ld(A), pc.ld(C)))
    assert float(np.max(np.abs(np.kron(invA, invC) - inv)) / np.max(np.abs(inv))) < 1e-17
    assert abs(float(7 * ldA + 5 * ldC - logdet)) < 1e-17 * max(1.0, abs(float(logdet)))


def test_reference_fixture_inside_the_bars():
    """tests/golden/prims.npz (the reference project's own outputs) against the longdouble references, within bars 1, 2, 3 and 5"""
    g = golden("prims")
    inside("pd_12", pc.frac(g["pd_12"], *pc.ref_dist(g["X1"], g["X2"])), 1.0)
    inside("pd_11", pc.frac(g["pd_11"], *pc.ref_dist(g["X1"])), 1.0)
    inside("rbf_11", pc.frac(g["rbf_11"], *pc.ref_rbf(g["x1"], None, 1.7, 0.4)[:2]), 1.0)
    inside("rbf_12", pc.frac(g["rbf_12"], *pc.ref_rbf(g["x1"], g["x2"], 1.7, 0.4)[:2]), 1.0)
    inside("rbf2d_12", pc.frac(g["rbf2d_12"], *pc.ref_rbf(g["X1"], g["X2"], 0.9, 1.3)[:2]), 1.0)
    inside("ns_11", pc.frac(g["ns_11"], *pc.ref_gibbs(g["x1"], g["s1"], g["l1"])[:2]), 1.0)
    inside("ns_11_default", pc.frac(g["ns_11_default"], *pc.ref_gibbs(g["x1"])[:2]), 1.0)
    inside("ns_12", pc.frac(g["ns_12"], *pc.ref_gibbs(g["x1"], g["s1"], g["l1"], g["x2"], g["s2"], g["l2"])[:2]), 1.0)
    assert np.array_equal(g["kron_BK"], np.kron(g["B"], g["K"])) and np.array_equal(g["kron_rect"], np.kron(g["Br"], g["Kr"]))
    inside("kron_mv_sq", pc.frac(g["kron_mv_sq"], *pc.ref_kron_mv(g["B"], g["K"], g["yk"])), 1.0)
    inside("kron_mv_rect", pc.frac(g["kron_mv_rect"], *pc.ref_kron_mv(g["Br"], g["Kr"], g["yr"])), 1.0)
    r = pc.dense_ref(pc.sym_upper(g["B"]), pc.sym_upper(g["K"]), g["yk"], None, float(g["sig2"]))
    assert all(b <= 1e-10 for b in r["bars"].values())
    inside("logpdf0", pc.relerr(float(g["logpdf0"]), r["logpdf"]), r["bars"]["logpdf"])
    inside("logpdf2", pc.relerr(float(g["logpdf2"]), r["logpdf"]), r["bars"]["logpdf"])
    inside("logpdf", pc.relerr(float(g["logpdf"]), r["logpdf"]), r["bars"]["logpdf"])
    inside("kron_inv", pc.inv_err(g["kron_inv"], r["inv"]), r["bars"]["inv"])
    inside("kron_logdet", pc.logdet_err(float(g["kron_logdet"]), r["logdet"]), r["bars"]["logdet"])
