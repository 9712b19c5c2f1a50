"""Device-resident HMC trajectories of the Hadamard cohort (nmgp_had_subjects_traj_*) and the cohort HMC drivers: the three models on
the subject sets A-H of tests/hadamard_cohort_cases.py (set I, Nmax = 1030: one two-step trajectory per model).  Everything is compared bit for bit with the host loop's arithmetic over the
models' *_subjects_eval entries (hh.host_trajectory), except the device's kinetic energy (a summation bound) and the comparison with
the per-subject samplers on the resident entries (VAL_TOL, the standing bar between two evaluation paths)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import hadamard_cases as hc
import hadamard_cohort_cases as cc
import hadamard_cohort_hmc_cases as hh
from conftest import ROOT, record_parity, relerr
from test_gpu_hadamard_sweep import VAL_TOL

pytestmark = pytest.mark.gpu

MODELS = hh.MODELS
NAMES = ("A", "B", "C", "D", "E", "F", "G", "H")
P_SEED = 9100                       # momenta of the ABI-level tests
DRIVER_SEED = 5200                  # test 10: every accept test of the reference runs is further than 1e-6 from its threshold


@pytest.fixture(scope="module")
def ctx():
    from nonstationary_multivariate_gaussian_process_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def set_subjects(ctx, cases, Nmax=None):
    subs = cc.subjects(cases)
    ctx.had_set_subjects([c["x"] for c in subs], [c["indx"] for c in subs], [c["y"] for c in subs], M=cases[0][1], Nmax=Nmax)


def packed(model, cases, k, Nmax=None, fill=0.0):
    return hh.pack(model, hh.chains(model, cases, k), cc.nobs(cases), cases[0][1], Nmax=Nmax, fill=fill)


def packed_minv(model, cases, k, Nmax=None, fill=1.0):
    rows = [np.tile(1.0 / m, (k, 1)) for m in hh.diag_mass(model, cases)]
    return hh.pack(model, rows, cc.nobs(cases), cases[0][1], Nmax=Nmax, fill=fill)


def real_mask(model, cases, k, Nmax=None):
    sizes = cc.nobs(cases)
    return ~hh.padded_slots(model, sizes, cases[0][1], max(sizes) if Nmax is None else Nmax, k)


def evaluator(ctx, model, hyper, k):
    return lambda Q: getattr(ctx, hh.ENTRY[model])(Q, hyper, True, True, k)


def host_reference(ctx, model, P, hyper, k, mask, eps, nsteps, p0, minv):
    """the host loop over the model's *_subjects_eval from the positions P"""
    ev = evaluator(ctx, model, hyper, k)
    out, g, status = ev(P)
    U = np.array(out[:, 0])
    bad = (status != 0) | ~np.isfinite(U)
    U[bad] = np.inf
    g[bad] = 0.0
    return hh.host_trajectory(ev, mask, P, U, g, np.repeat(eps, k), nsteps, p0, minv)


def device_traj(ctx, model, P, hyper, k, eps, nsteps, p0, minv=None, want_kin=True):
    """begin at P, the mass, one trajectory: (out, status), (q1, p1, kin1, U1, failed)"""
    start = ctx.had_subjects_traj_begin(model, P, hyper, True, k)
    ctx.had_subjects_traj_set_mass(minv)
    return start, ctx.had_subjects_traj(eps, nsteps, p0, want_p1=True, want_kin=want_kin)


def agree(dev, ref, mask):
    """q1, p1, U1, failed of the device against the host loop: real slots bit for bit, padded momentum +0.0"""
    q1, p1, _, U1, failed = dev
    rq, rp, rU, rf = ref
    assert hh.same_real_bits(q1, rq, mask) and hh.same_real_bits(p1, rp, mask)
    assert np.array_equal(hh.bits(U1), hh.bits(rU)) and np.array_equal(failed, rf)
    assert np.all(p1[~mask] == 0.0) and not np.any(np.signbit(p1[~mask]))


def abi_cases(ctx, model, cases, ks=(1, 2), steps=(1, 3)):
    """test 2's sweep on the set that is on the context: k, nsteps, identity and diagonal mass"""
    hyper, S = hh.hyper_of(model, cases), len(cases)
    eps = hh.eps_of(S)
    for k in ks:
        P, mask = packed(model, cases, k), real_mask(model, cases, k)
        p0 = hh.momenta(model, cases, k, P_SEED)
        for nsteps in steps:
            for minv in (None, packed_minv(model, cases, k)):
                _, dev = device_traj(ctx, model, P, hyper, k, eps, nsteps, p0, minv)
                ref = host_reference(ctx, model, P, hyper, k, mask, eps, nsteps, p0, minv)
                assert not dev[4].any() and np.all(np.isfinite(dev[3]))
                agree(dev, ref, mask)
                yield k, nsteps, minv is not None, dev
    ctx.had_subjects_traj_end()


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("model", MODELS)
def test_begin_is_the_evaluation(ctx, model, name):
    """out and status of begin are the entry's, bit for bit; one step from momenta +0.0 gives q0 - 1/2 eps^2 minv g0 in the stated
    order, which shows that the resident gradient has the entry's bits."""
    cases, k = cc.SETS[name], 2
    set_subjects(ctx, cases)
    hyper, eps = hh.hyper_of(model, cases), hh.eps_of(len(cases))
    P, mask = packed(model, cases, k), real_mask(model, cases, k)
    out, g, status = getattr(ctx, hh.ENTRY[model])(P, hyper, True, True, k)
    assert status.tolist() == [0] * len(status)
    for minv in (None, packed_minv(model, cases, k)):
        (bout, bstatus), (q1, p1, _, U1, failed) = device_traj(ctx, model, P, hyper, k, eps, 1, np.zeros_like(P), minv)
        assert np.array_equal(hh.bits(bout), hh.bits(out)) and np.array_equal(bstatus, status) and not failed.any()
        e = np.repeat(eps, k)[:, None]
        p = 0.0 - (0.5 * e) * g                                     # t = c g; p = p - t
        v = p if minv is None else minv * p
        assert hh.same_real_bits(q1, P + e * v, mask)
        assert np.array_equal(hh.bits(q1)[~mask], hh.bits(P)[~mask])        # padded slots come back as uploaded
    ctx.had_subjects_traj_end()


# ---- 2 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("model", MODELS)
def test_resident_loop_is_the_host_loop(ctx, model, name):
    cases = cc.SETS[name]
    set_subjects(ctx, cases)
    assert len(list(abi_cases(ctx, model, cases))) == 8


@pytest.mark.parametrize("model", MODELS)
def test_resident_loop_is_the_host_loop_in_set_I(ctx, model):
    """Nmax = 1030 (tests/hadamard_cohort_cases.py), one chain per subject: one trajectory of two steps with a diagonal mass."""
    cases, k, nsteps = cc.SET_I, 1, 2
    set_subjects(ctx, cases)
    hyper, eps = hh.hyper_of(model, cases), hh.eps_of(len(cases))
    P, mask, p0, minv = packed(model, cases, k), real_mask(model, cases, k), hh.momenta(model, cases, k, P_SEED), packed_minv(model, cases, k)
    _, dev = device_traj(ctx, model, P, hyper, k, eps, nsteps, p0, minv)
    ref = host_reference(ctx, model, P, hyper, k, mask, eps, nsteps, p0, minv)
    ctx.had_subjects_traj_end()
    assert not dev[4].any() and np.all(np.isfinite(dev[3]))
    agree(dev, ref, mask)


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("model", MODELS)
def test_device_kinetic_energy(ctx, model, name):
    """kin1 against math.fsum over the real slots of the downloaded p1, within the summation bound (P_s + 4) 2^-53 1/2 sum |p v|;
    the bits of a chain alone in a set of one equal those in the full set."""
    cases, k, nsteps = cc.SETS[name], 2, 3
    hyper, M = hh.hyper_of(model, cases), cases[0][1]
    worst, full = 0.0, {}
    for masses in (False, True):
        set_subjects(ctx, cases)
        P, mask, p0 = packed(model, cases, k), real_mask(model, cases, k), hh.momenta(model, cases, k, P_SEED)
        minv = packed_minv(model, cases, k) if masses else None
        _, (q1, p1, kin1, U1, failed) = device_traj(ctx, model, P, hyper, k, hh.eps_of(len(cases)), nsteps, p0, minv)
        for z in range(P.shape[0]):
            pr = p1[z][mask[z]]
            terms = pr * (pr if minv is None else minv[z][mask[z]] * pr)
            bound = (pr.shape[0] + 4) * 2.0 ** -53 * 0.5 * math.fsum(np.abs(terms))
            err = abs(kin1[z] - 0.5 * math.fsum(terms))
            print(model, name, "mass", masses, "row", z, "kin1", kin1[z], "err", err, "bound", bound)
            worst = max(worst, err / bound)
            assert err <= bound
        full[masses] = kin1
    record_parity("hcohort_hmc/%s/%s/kinetic" % (model, name), kin=(worst, 1.0))
    # the first subject alone in a set of one
    set_subjects(ctx, cases[:1])
    for masses in (False, True):
        minv = packed_minv(model, cases[:1], k) if masses else None
        _, dev = device_traj(ctx, model, packed(model, cases[:1], k), hyper, k, hh.eps_of(len(cases))[:1], nsteps,
                             hh.momenta(model, cases[:1], k, P_SEED), minv)
        assert np.array_equal(hh.bits(dev[2]), hh.bits(full[masses][:k]))
    ctx.had_subjects_traj_end()


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------------
def run_unpacked(ctx, model, cases, k, eps, p_rows, Nmax=None, masses=True, nsteps=3, fill=0.0):
    """a trajectory on `cases` -> per subject (q1, p1) [k, P_s] in the reference layout, kin1, U1 [S, k]"""
    sizes, M = cc.nobs(cases), cases[0][1]
    set_subjects(ctx, cases, Nmax=Nmax)
    hyper = hh.hyper_of(model, cases)
    P = packed(model, cases, k, Nmax=Nmax, fill=fill)
    p0 = hh.pack(model, p_rows, sizes, M, Nmax=Nmax, fill=fill)
    minv = packed_minv(model, cases, k, Nmax=Nmax, fill=1.0 if fill == 0.0 else fill) if masses else None
    _, (q1, p1, kin1, U1, failed) = device_traj(ctx, model, P, hyper, k, eps, nsteps, p0, minv)
    assert not failed.any()
    return hh.unpack(model, q1, sizes, M, k), hh.unpack(model, p1, sizes, M, k), kin1.reshape(len(cases), k), U1.reshape(len(cases), k)


def momentum_rows(model, cases, k):
    return [np.stack([np.random.default_rng(P_SEED + 31 * s + j).standard_normal(v.shape[1]) for j in range(k)])
            for s, v in enumerate(hh.chains(model, cases, k))]


def same_subject(a, b, sa, sb, rows=slice(None), what=""):
    """q1, p1, kin1, U1 of subject sa of run a against subject sb of run b, bit for bit; the distances are printed first"""
    dist = [float(np.max(np.abs(x[sa][rows] - y[sb][rows]))) for x, y in zip(a, b)]
    print(what, "subject", sa, "max |difference| of q1, p1, kin1, U1:", dist)
    return all(np.array_equal(hh.bits(x[sa][rows]), hh.bits(y[sb][rows])) for x, y in zip(a, b))


@pytest.mark.parametrize("model", MODELS)
def test_a_chain_depends_on_nothing_else(ctx, model):
    """q1, p1, kin1 and U1 of set A: the subject of N_s = 63 alone (a set of one at the same Nmax = 128, as the evaluation's own
    independence test) against its rows in the full set; k = 1 against row 0 of k = 2; an unpadded Nmax against Nmax + 37; a second
    identical begin + traj after end."""
    cases, who = cc.SET_A, 1
    Nmax = max(cc.nobs(cases))
    assert cases[who][0] == 63 and Nmax == 128
    eps, rows2 = hh.eps_of(len(cases)), momentum_rows(model, cases, 2)
    full = run_unpacked(ctx, model, cases, 2, eps, rows2)
    alone = run_unpacked(ctx, model, cases[who:who + 1], 2, eps[who:who + 1], rows2[who:who + 1], Nmax=Nmax)
    one = run_unpacked(ctx, model, cases, 1, eps, [r[:1] for r in rows2])
    wide = run_unpacked(ctx, model, cases, 2, eps, rows2, Nmax=Nmax + 37)
    ctx.had_subjects_traj_end()
    again = run_unpacked(ctx, model, cases, 2, eps, rows2)
    ctx.had_subjects_traj_end()
    ok = [same_subject(full, alone, who, 0, what="alone")]
    ok += [same_subject(full, one, s, s, slice(0, 1), what="k=1") for s in range(len(cases))]
    ok += [same_subject(full, again, s, s, what="again") for s in range(len(cases))]
    ok += [same_subject(full, wide, s, s, what="Nmax+37") for s in range(len(cases))]
    assert all(ok), ok


# ---- 5 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("model", MODELS)
def test_poisoned_pads_are_never_read(ctx, model, name):
    """NaN, 1e300 and the labels -1 / 99 in every padded slot of pars, p0, minv and of the set's x / indx / y: the real slots keep
    their bits and no chain fails."""
    cases, k = cc.SETS[name], 2
    sizes, M = cc.nobs(cases), cases[0][1]
    Nmax = max(sizes) + 5
    eps, rows = hh.eps_of(len(cases)), momentum_rows(model, cases, k)
    clean = run_unpacked(ctx, model, cases, k, eps, rows, Nmax=Nmax)
    subs = cc.subjects(cases)
    for fill, label in ((np.nan, -1), (1e300, 99)):
        x2, y2 = np.full((len(cases), Nmax), fill), np.full((len(cases), Nmax), fill)
        i2 = np.full((len(cases), Nmax), label, dtype=np.int32)
        for s, c in enumerate(subs):
            x2[s, :sizes[s]], y2[s, :sizes[s]], i2[s, :sizes[s]] = c["x"], c["y"], c["indx"]
        ctx.had_set_subjects_padded(x2, i2, y2, sizes, M)
        hyper = hh.hyper_of(model, cases)
        P = packed(model, cases, k, Nmax=Nmax, fill=fill)
        p0 = hh.pack(model, rows, sizes, M, Nmax=Nmax, fill=fill)
        minv = packed_minv(model, cases, k, Nmax=Nmax, fill=fill)
        if model != "sta":
            pads = hh.padded_slots(model, sizes, M, Nmax, k)
            assert pads.any() and not np.any(np.isfinite(P[pads]) & (np.abs(P[pads]) < 1e299))
        _, (q1, p1, kin1, U1, failed) = device_traj(ctx, model, P, hyper, k, eps, 3, p0, minv)
        assert failed.tolist() == [False] * len(failed)
        got = (hh.unpack(model, q1, sizes, M, k), hh.unpack(model, p1, sizes, M, k), kin1.reshape(len(cases), k), U1.reshape(len(cases), k))
        for s in range(len(cases)):
            assert same_subject(clean, got, s, s), (fill, s)
        if model != "sta":
            assert np.array_equal(hh.bits(q1)[pads], hh.bits(P)[pads]) and np.all(p1[pads] == 0.0) and not np.any(np.signbit(p1[pads]))
    ctx.had_subjects_traj_end()


# ---- 6 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("model", MODELS)
def test_commit_restores_the_rejected_chains(ctx, model, name):
    """accept = 1, 0, 1, ...: a second trajectory with fresh momenta equals a fresh begin at the accepted / restored positions followed
    by the same trajectory."""
    cases, k, nsteps = cc.SETS[name], 2, 2
    set_subjects(ctx, cases)
    hyper, eps = hh.hyper_of(model, cases), hh.eps_of(len(cases))
    P, mask = packed(model, cases, k), real_mask(model, cases, k)
    pa, pb = hh.momenta(model, cases, k, P_SEED), hh.momenta(model, cases, k, P_SEED + 1000)
    minv = packed_minv(model, cases, k)
    _, first = device_traj(ctx, model, P, hyper, k, eps, nsteps, pa, minv)
    accept = (np.arange(P.shape[0]) % 2 == 0)
    ctx.had_subjects_traj_commit(accept)
    second = ctx.had_subjects_traj(eps, nsteps, pb, want_p1=True, want_kin=True)
    at = np.where(accept[:, None], first[0], P)
    _, fresh = device_traj(ctx, model, at, hyper, k, eps, nsteps, pb, minv)
    for a, b in zip(second[:2], fresh[:2]):
        assert hh.same_real_bits(a, b, mask)
    for a, b in zip(second[2:4], fresh[2:4]):
        assert np.array_equal(hh.bits(a), hh.bits(b))
    assert not second[4].any() and not fresh[4].any()
    assert not hh.same_real_bits(first[0], P, mask)                 # (the first trajectory moved the chains)
    ctx.had_subjects_traj_end()


# ---- 7 ----------------------------------------------------------------------------------------------------------------------------------
def three_chains(model, cases, bad):
    """[good, bad or good, good] per subject: hc.minor_chains on the MINOR subject, chain 0, chain 1 and their midpoint elsewhere"""
    out = []
    for case, c in zip(cases, cc.subjects(cases)):
        P = c["pars"][hh.PARS[model]]
        if case == hc.MINOR:
            m = hc.minor_chains(hh.PARS[model])
            out.append(m if bad else np.stack([m[0], P[1], m[2]]))
        else:
            out.append(np.stack([P[0], P[1], 0.5 * (P[0] + P[1])]))
    return out


@pytest.mark.parametrize("model", MODELS)
def test_a_failure_stays_in_its_chain(ctx, model):
    cases, k = cc.SET_C, 3
    sizes, M, S = cc.nobs(cases), cases[0][1], len(cases)
    who = cases.index(hc.MINOR)
    bad_row = who * k + 1
    set_subjects(ctx, cases)
    hyper, eps = hh.hyper_of(model, cases), hh.eps_of(S)
    mask = real_mask(model, cases, k)
    rows = momentum_rows(model, cases, k)
    p0 = hh.pack(model, rows, sizes, M)
    others = np.arange(S * k) != bad_row

    def neighbours_agree(a, b):
        for x, y in zip(a[:2], b[:2]):
            assert hh.same_real_bits(x[others], y[others], mask[others])
        for x, y in zip(a[2:4], b[2:4]):
            assert np.array_equal(hh.bits(x[others]), hh.bits(y[others]))
        assert np.array_equal(a[4][others], b[4][others])

    # (a) a chain that is bad at the start
    good = hh.pack(model, three_chains(model, cases, False), sizes, M)
    bad = hh.pack(model, three_chains(model, cases, True), sizes, M)
    (_, st_good), base = device_traj(ctx, model, good, hyper, k, eps, 2, p0)
    (out, st_bad), dev = device_traj(ctx, model, bad, hyper, k, eps, 2, p0)
    assert st_good.tolist() == [0] * (S * k) and not base[4].any()
    assert st_bad[bad_row] != 0 and st_bad[others].tolist() == [0] * (S * k - 1) and np.all(np.isnan(out[bad_row]))
    assert dev[4][bad_row] and np.isposinf(dev[3][bad_row]) and not dev[4][others].any()
    neighbours_agree(dev, base)
    # (b) a chain pushed out in the middle of a trajectory: p0 = 1e300 in its last real slot, eps[s] = 1e10
    far = eps.copy()
    far[who] = 1e10
    pushed = p0.copy()
    pushed[bad_row, np.flatnonzero(mask[bad_row])[-1]] = 1e300
    _, base = device_traj(ctx, model, good, hyper, k, far, 2, p0)
    _, dev = device_traj(ctx, model, good, hyper, k, far, 2, pushed)
    assert dev[4][bad_row] and np.isposinf(dev[3][bad_row]) and not np.all(np.isfinite(dev[0][bad_row][mask[bad_row]]))
    other_subjects = np.repeat(np.arange(S) != who, k)
    assert not dev[4][other_subjects].any() and np.all(np.isfinite(dev[3][other_subjects]))
    neighbours_agree(dev, base)
    # ... and the host loop says the same of every row
    ref = host_reference(ctx, model, good, hyper, k, mask, far, 2, pushed, None)
    assert np.array_equal(dev[4], ref[3]) and np.array_equal(hh.bits(dev[3]), hh.bits(ref[2]))
    ctx.had_subjects_traj_end()


# ---- 8 ----------------------------------------------------------------------------------------------------------------------------------
CHUNK_NOBS = [1024, 513, 1023, 64]


@pytest.mark.parametrize("model", MODELS)
def test_trajectories_do_not_depend_on_the_chunking(ctx, model, monkeypatch):
    """The shape of test_results_do_not_depend_on_the_chunking (M = 2, Nmax = 1024): (S, cps) = (4, 16) runs as chunks of whole
    subjects under a cap of 1 GB, (2, 48) as parts of one subject's chains; one chunk each under the default cap."""
    M, Nmax, nsteps = 2, max(CHUNK_NOBS), 2
    subs, vecs = [], []
    for s, n in enumerate(CHUNK_NOBS):
        x, indx, y, L_vec = hc.subject(n, M, "interleaved", 3400 + s)
        subs.append((x, indx, y))
        vecs.append(hc.parameters(x, M, L_vec)[hh.PARS[model]])
    hyper = hc.hypers()[hh.PARS[model]]
    for S, cps in ((4, 16), (2, 48)):
        under, whole_n = hh.chunks_under_cap(model, Nmax, M, S, cps, 1.0), hh.chunks_under_cap(model, Nmax, M, S, cps, 96.0)
        print(model, "S", S, "cps", cps, "bytes per chain", hh.workspace_per_chain(model, Nmax, M), "chunks", under, whole_n)
        assert under >= 2 and whole_n == 1
        ctx.had_set_subjects([s[0] for s in subs[:S]], [s[1] for s in subs[:S]], [s[2] for s in subs[:S]], M=M, Nmax=Nmax)
        rows = [v[0][None] + (np.arange(cps) / cps)[:, None] * (v[1] - v[0])[None] for v in vecs[:S]]
        P = hh.pack(model, rows, CHUNK_NOBS[:S], M, Nmax=Nmax)
        p0 = hh.pack(model, [np.random.default_rng(P_SEED + s).standard_normal(r.shape) for s, r in enumerate(rows)], CHUNK_NOBS[:S], M,
                     Nmax=Nmax)
        eps = hh.eps_of(S)
        monkeypatch.setenv("NMGP_HAD_BATCH_SLAB_GB", "1")
        start_c, chunked = device_traj(ctx, model, P, hyper, cps, eps, nsteps, p0)
        monkeypatch.delenv("NMGP_HAD_BATCH_SLAB_GB")
        start_w, whole = device_traj(ctx, model, P, hyper, cps, eps, nsteps, p0)
        assert not whole[4].any() and np.all(np.isfinite(whole[3])) and len(set(whole[3].tolist())) == S * cps
        for a, b in zip(start_c + chunked, start_w + whole):
            assert np.array_equal(hh.bits(a) if a.dtype == np.float64 else a, hh.bits(b) if b.dtype == np.float64 else b)
    ctx.had_clear_subjects()                             # (gives the prior factors back)


# ---- 9 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_refusals_leave_the_context_usable(ctx, model):
    import ctypes
    from nonstationary_multivariate_gaussian_process_amd import _lib
    cases, k = cc.SET_E, 1
    set_subjects(ctx, cases)
    hyper, eps, S = hh.hyper_of(model, cases), hh.eps_of(len(cases)), len(cases)
    P, mask, p0 = packed(model, cases, k), real_mask(model, cases, k), hh.momenta(model, cases, k, P_SEED)
    minv = packed_minv(model, cases, k)

    def still_good():
        _, dev = device_traj(ctx, model, P, hyper, k, eps, 3, p0, minv)
        agree(dev, host_reference(ctx, model, P, hyper, k, mask, eps, 3, p0, minv), mask)

    ctx.had_subjects_traj_end()
    with pytest.raises(_lib.NmgpError, match="error -3"):                       # traj before begin
        ctx.had_subjects_traj(eps, 3, p0)
    with pytest.raises(_lib.NmgpError, match="error -3"):
        ctx.had_subjects_traj_commit(np.ones(S * k))
    with pytest.raises(_lib.NmgpError, match="error -3"):
        ctx.had_subjects_traj_set_mass(minv)
    still_good()
    out, status = np.empty((S * k, hh.WIDTH[model])), np.zeros(S * k, dtype=np.int32)
    ip = ctypes.POINTER(ctypes.c_int)
    for bad_model in (-1, 3):                                                   # a bad model (the binding only knows the three names)
        rc = ctx.lib.nmgp_had_subjects_traj_begin(ctx.h, bad_model, _lib.ptr(P), S * k, k, _lib.ptr(np.asarray(hyper, dtype=np.float64)), 1,
                                                  _lib.ptr(out), status.ctypes.data_as(ip))
        assert rc == -2
    with pytest.raises(_lib.NmgpError):
        ctx.had_subjects_traj_begin("whitened", P, hyper, True, k)
    still_good()
    with pytest.raises(_lib.NmgpError, match="error -2"):                       # B != S cps
        ctx.had_subjects_traj_begin(model, P, hyper, True, 2)
    with pytest.raises(_lib.NmgpError, match="error -2"):
        ctx.had_subjects_traj_begin(model, P, hyper, True, 0)
    with pytest.raises(_lib.NmgpError, match="error -2"):
        ctx.had_subjects_traj_begin(model, P[:1], hyper, True, 1)
    still_good()
    with pytest.raises(_lib.NmgpError, match="error -2"):                       # nsteps = 0
        ctx.had_subjects_traj(eps, 0, p0)
    for bad_eps in (0.0, np.nan, -1e-3, np.inf):
        e = eps.copy()
        e[-1] = bad_eps
        with pytest.raises(_lib.NmgpError, match="error -2"):
            ctx.had_subjects_traj(e, 3, p0)
    m0 = minv.copy()
    m0[-1, np.flatnonzero(mask[-1])[0]] = 0.0
    with pytest.raises(_lib.NmgpError, match="error -2"):                       # a 0 in a real slot of minv
        ctx.had_subjects_traj_set_mass(m0)
    still_good()
    ctx.had_clear_subjects()                                                    # the set ends the trajectory
    with pytest.raises(_lib.NmgpError, match="error -3"):
        ctx.had_subjects_traj(eps, 3, p0)
    set_subjects(ctx, cases)
    with pytest.raises(_lib.NmgpError, match="error -3"):                       # ... and so does a new set
        ctx.had_subjects_traj(eps, 3, p0)
    still_good()
    set_subjects(ctx, cases)
    with pytest.raises(_lib.NmgpError, match="error -3"):
        ctx.had_subjects_traj(eps, 3, p0)
    still_good()
    ctx.had_subjects_traj_end()


# ---- 10 ---------------------------------------------------------------------------------------------------------------------------------
def driver(model, cases, k, steps=3, **kw):
    from nonstationary_multivariate_gaussian_process_amd import drivers
    return getattr(drivers, hh.DRIVER[model])(hh.subject_triples(cases), hh.hyper_dict(model, cases), hh.chains(model, cases, k),
                                              step_size=hh.eps_of(len(cases)), num_steps_in_leap=steps, seed=DRIVER_SEED, **kw)


@pytest.mark.parametrize("masses", [False, True], ids=["identity", "diagonal"])
@pytest.mark.parametrize("model", MODELS)
def test_driver_resident_loop_is_the_host_loop(model, masses):
    cases, k = cc.SET_A, 2
    mass = hh.diag_mass(model, cases) if masses else None
    runs = []
    for resident in (True, False):
        d = driver(model, cases, k, mass=mass, device_resident=resident, device_kinetic=False)
        try:
            runs.append(d.run(4))
        finally:
            d.close()
    (a, ia), (b, ib) = runs
    for s in range(len(cases)):
        assert a[s].shape == (4, k, hh.chains(model, cases, k)[s].shape[1]) and np.array_equal(hh.bits(a[s]), hh.bits(b[s]))
    assert np.array_equal(hh.bits(ia["energy_error"]), hh.bits(ib["energy_error"])) and np.array_equal(ia["accept_rate"], ib["accept_rate"])
    assert np.all(np.isfinite(ia["energy_error"]))


@pytest.mark.parametrize("model", MODELS)
def test_driver_device_kinetic(model):
    """device_kinetic=True: the same accept decisions, energy errors within the two kinetic energies' summation bounds"""
    cases, k = cc.SET_A, 2
    runs = []
    for dk in (False, True):
        d = driver(model, cases, k, device_kinetic=dk)
        try:
            runs.append(d.run(3))
        finally:
            d.close()
    (a, ia), (b, ib) = runs
    assert np.array_equal(ia["accept_rate"], ib["accept_rate"])
    for s in range(len(cases)):
        assert np.array_equal(hh.bits(a[s]), hh.bits(b[s]))
    assert np.max(np.abs(ia["energy_error"] - ib["energy_error"])) < 1e-9


@pytest.mark.parametrize("model", MODELS)
def test_driver_against_the_per_subject_samplers(ctx, model):
    """The cohort driver against BatchedHMCHadamard / Sep / Sta subject by subject on the resident entries: the same starts and seeds,
    3 iterations x 3 steps, max_flop_waste 0 and 0.5.  DRIVER_SEED: every accept test of the reference runs has |log u + dH| > 1e-6."""
    from nonstationary_multivariate_gaussian_process_amd import drivers
    cases, k, iters = cc.SET_A, 2, 3
    eps, starts, hyper = hh.eps_of(len(cases)), hh.chains(model, cases, k), hh.hyper_dict(model, cases)
    refs = []
    for s, (x, indx, y) in enumerate(hh.subject_triples(cases)):
        ref = getattr(drivers, hh.PER_SUBJECT[model])(x, indx, y, hyper, starts[s], step_size=eps[s], num_steps_in_leap=3,
                                                      seed=DRIVER_SEED + s * k, ctx=ctx)
        samples, info = ref.run(iters)
        # the uniforms of the accept tests, from the chains' own streams: P_s normals, then the uniform, per iteration
        for j in range(k):
            rng = np.random.default_rng(DRIVER_SEED + s * k + j)
            for it in range(iters):
                rng.standard_normal(starts[s].shape[1])
                margin = abs(np.log(rng.random()) + info["energy_error"][it, j])
                assert margin > 1e-6, (model, s, j, it, margin)
        refs.append((samples, info))
    for waste in (0.0, 0.5):
        d = driver(model, cases, k, max_flop_waste=waste)
        try:
            samples, info = d.run(iters)
        finally:
            d.close()
        worst, identical = 0.0, True
        for s in range(len(cases)):
            assert np.array_equal(info["accept_rate"][s * k:(s + 1) * k], refs[s][1]["accept_rate"]), (model, waste, s)
            worst = max(worst, relerr(samples[s], refs[s][0]))
            identical = identical and np.array_equal(hh.bits(samples[s]), hh.bits(refs[s][0]))
        print(model, "max_flop_waste", waste, "buckets", len(d.buckets), "distance", worst, "bit identical", identical)
        record_parity("hcohort_hmc/%s/driver/max_flop_waste_%g" % (model, waste), samples=(worst, VAL_TOL), bit_identical=float(identical))
        assert worst < VAL_TOL


@pytest.mark.parametrize("model", MODELS)
def test_samples_go_straight_into_the_cohort_predictor(model):
    from nonstationary_multivariate_gaussian_process_amd import drivers
    cases, k = cc.SET_A, 2
    d = driver(model, cases, k)
    try:
        samples, _ = d.run(2)
    finally:
        d.close()
    xs = [c["xs"] for c in cc.subjects(cases)]
    bands = getattr(drivers, hh.PREDICT[model])(hh.subject_triples(cases), hh.hyper_dict(model, cases), samples, xs, seed=3)
    assert len(bands) == len(cases)
    for c, band in zip(cc.subjects(cases), bands):
        assert band["status"].tolist() == [0] * (2 * k) and band["mean"].shape[0] == c["xs"].shape[0] and np.all(np.isfinite(band["mean"]))


# ---- 11 ---------------------------------------------------------------------------------------------------------------------------------
POISON_SNIPPET = r"""
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import hadamard_cohort_cases as cc
import test_gpu_hadamard_cohort_hmc as t
from nonstationary_multivariate_gaussian_process_amd import _lib
ctx = _lib.Context(0)
for model in t.MODELS:
    t.set_subjects(ctx, cc.SET_B)
    assert len(list(t.abi_cases(ctx, model, cc.SET_B))) == 8
    for cases in (cc.SET_F, cc.SET_G, cc.SET_H):                 # M = 4, 6, 7: two chains, three steps, both masses
        t.set_subjects(ctx, cases)
        assert len(list(t.abi_cases(ctx, model, cases, ks=(2,), steps=(3,)))) == 2
ctx.close()
print("POISON_OK")
"""


def test_poisoned_workspace():
    """NMGP_POISON=1 (read once per process: a fresh child, nothing preloaded) fills fresh buffers and the kept workspace with NaN
    before every call: a resident buffer or a slab piece that nobody wrote would show up in test 2's comparison on set B and, with
    two chains and three steps, on sets F, G and H."""
    env = dict(os.environ)
    env["NMGP_POISON"] = "1"
    env.pop("NMGP_HAD_BATCH_SLAB_GB", None)
    out = subprocess.run([sys.executable, "-c", POISON_SNIPPET % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}],
                         capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0 and "POISON_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
