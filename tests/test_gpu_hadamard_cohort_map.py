"""The device-resident Adam of the Hadamard cohort (nmgp_had_subjects_adam_*) and the cohort MAP drivers on it: the three models on the
subject sets A-E of tests/hadamard_cohort_cases.py (set I, Nmax = 1030: one run of two iterations per model).  Everything is compared
bit for bit with the host loop: drivers.LockStepMAP over the model's *_subjects_eval on the same set (hm.host_loop)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import hadamard_cases as hc
import hadamard_cohort_cases as cc
import hadamard_cohort_hmc_cases as hh
import hadamard_cohort_map_cases as hm
from conftest import ROOT, record_parity

pytestmark = pytest.mark.gpu

MODELS = hh.MODELS
NAMES = ("A", "B", "C", "D", "E")
LR = hm.LR


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


def real_mask(model, cases, k, Nmax=None):
    sizes = cc.nobs(cases)
    return ~hh.padded_slots(model, sizes, cases[0][1], max(sizes) if Nmax is None else Nmax, k)


def evaluator(ctx, model, hyper, k):
    return lambda Q: getattr(ctx, hh.ENTRY[model])(Q, hyper, True, True, k)


def resident(ctx, model, P, hyper, k, calls, lr=LR):
    """begin at P, one call per entry of `calls`: (out_hist of all calls, alive after the last, the parameters)"""
    ctx.had_subjects_adam_begin(model, P, hyper, True, k)
    hists = []
    for n in calls:
        hist, alive = ctx.had_subjects_adam(n, lr)
        assert hist.shape == (n, P.shape[0], hh.WIDTH[model]) and alive.shape == (P.shape[0],)
        hists.append(hist)
    return np.concatenate(hists), alive, ctx.had_subjects_adam_get_pars()


def agree(dev, ref, mask, P):
    """history (the full tuples), alive and the parameters' real slots against the host loop, bit for bit; the padded slots of the
    parameters come back as uploaded"""
    hist, alive, pars = dev
    assert hm.same_hist(hist, ref[0]), float(np.nanmax(np.abs(hist - ref[0])))
    assert np.array_equal(alive, ref[1])
    assert hh.same_real_bits(pars, ref[2], mask)
    assert np.array_equal(hh.bits(pars)[~mask], hh.bits(P)[~mask])


def entry_cases(ctx, model, cases, ks=(1, 2), iters=(1, 5), name="-"):
    """test 1's sweep on the set that is on the context"""
    hyper = hh.hyper_of(model, cases)
    for k in ks:
        P, mask = packed(model, cases, k), real_mask(model, cases, k)
        for n in iters:
            dev = resident(ctx, model, P, hyper, k, [n])
            ref = hm.host_loop(evaluator(ctx, model, hyper, k), P, n)
            assert dev[1].all() and np.all(np.isfinite(dev[0]))
            with np.errstate(invalid="ignore"):
                dist = float(np.max(np.abs(dev[0] - ref[0]))), float(np.max(np.abs(dev[2] - ref[2])[mask]))
            print(model, name, "k", k, "iterations", n, "max |difference| of out_hist, pars against the host loop:", dist)
            record_parity("hcohort_map/%s/%s/k%d/iters%d" % (model, name, k, n), out_hist=(dist[0], 0.0), pars=(dist[1], 0.0))
            agree(dev, ref, mask, P)
            assert not hh.same_real_bits(dev[2], P, mask)                   # (the chains moved)
            yield k, n, dev
    ctx.had_subjects_adam_end()


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("model", MODELS)
def test_entry_is_the_host_loop(ctx, model, name):
    cases = cc.SETS[name]
    set_subjects(ctx, cases)
    assert len(list(entry_cases(ctx, model, cases, name=name))) == 4


@pytest.mark.parametrize("model", MODELS)
def test_entry_is_the_host_loop_in_set_I(ctx, model):
    """Nmax = 1030 (tests/hadamard_cohort_cases.py), one chain per subject, two iterations in one call."""
    cases = cc.SET_I
    set_subjects(ctx, cases)
    assert len(list(entry_cases(ctx, model, cases, ks=(1,), iters=(2,), name="I"))) == 1


# ---- 2 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("A", "C"))
@pytest.mark.parametrize("model", MODELS)
def test_splitting_calls_changes_nothing(ctx, model, name):
    """5 iterations as one call, as 2 + 3 and as 1 x 5: t, m and v persist between calls."""
    cases, k = cc.SETS[name], 2
    set_subjects(ctx, cases)
    hyper, P = hh.hyper_of(model, cases), packed(model, cases, k)
    whole = resident(ctx, model, P, hyper, k, [5])
    for calls in ([2, 3], [1, 1, 1, 1, 1]):
        split = resident(ctx, model, P, hyper, k, calls)
        assert np.array_equal(hh.bits(split[0]), hh.bits(whole[0])) and np.array_equal(split[1], whole[1])
        assert np.array_equal(hh.bits(split[2]), hh.bits(whole[2]))
    assert whole[1].all() and len({tuple(r) for r in whole[0][:, 0, :].tolist()}) == 5         # (five different tuples of chain 0)
    ctx.had_subjects_adam_end()


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------------
def run_unpacked(ctx, model, cases, k, Nmax=None, iters=3, fill=0.0, starts=None):
    """a resident run on `cases` -> per subject (pars [k, P_s] in the reference layout, hist [iters, k, W])"""
    sizes, M = cc.nobs(cases), cases[0][1]
    set_subjects(ctx, cases, Nmax=Nmax)
    P = hh.pack(model, hh.chains(model, cases, k) if starts is None else starts, sizes, M, Nmax=Nmax, fill=fill)
    hist, alive, pars = resident(ctx, model, P, hh.hyper_of(model, cases), k, [iters])
    assert alive.all()
    return hh.unpack(model, pars, sizes, M, k), [hist[:, s * k:(s + 1) * k] for s in range(len(cases))]


def same_subject(a, b, sa, sb, rows=slice(None), what=""):
    """parameters and history of subject sa of run a against subject sb of run b, bit for bit; the distances are printed first"""
    pa, pb, ha, hb = a[0][sa][rows], b[0][sb][rows], a[1][sa][:, rows], b[1][sb][:, rows]
    print(what, "subject", sa, "max |difference| of pars, hist:", float(np.max(np.abs(pa - pb))), float(np.max(np.abs(ha - hb))))
    return np.array_equal(hh.bits(pa), hh.bits(pb)) and np.array_equal(hh.bits(ha), hh.bits(hb))


@pytest.mark.parametrize("model", MODELS)
def test_a_chain_depends_on_nothing_else(ctx, model):
    """Parameters and histories of set A: the subject of N_s = 63 alone (a set of one at the same Nmax = 128) against its rows in the
    full set; k = 1 against row 0 of k = 2; an unpadded Nmax against Nmax + 37; a second identical run after end."""
    cases, who = cc.SET_A, 1
    Nmax = max(cc.nobs(cases))
    assert cases[who][0] == 63 and Nmax == 128
    full = run_unpacked(ctx, model, cases, 2)
    alone = run_unpacked(ctx, model, cases[who:who + 1], 2, Nmax=Nmax)
    one = run_unpacked(ctx, model, cases, 1)
    wide = run_unpacked(ctx, model, cases, 2, Nmax=Nmax + 37)
    ctx.had_subjects_adam_end()
    again = run_unpacked(ctx, model, cases, 2)
    ctx.had_subjects_adam_end()
    ok = [same_subject(full, alone, who, 0, what="alone")]
    ok += [same_subject(full, one, s, s, slice(0, 1), what="k=1") for s in range(len(cases))]
    ok += [same_subject(full, again, s, s, what="again") for s in range(len(cases))]
    ok += [same_subject(full, wide, s, s, what="Nmax+37") for s in range(len(cases))]
    assert all(ok), ok


CHUNK_NOBS = [1024, 513, 1023, 64]


@pytest.mark.parametrize("model", MODELS)
def test_results_do_not_depend_on_the_chunking(ctx, model, monkeypatch):
    """The shape of the evaluation's and the trajectories' chunking tests (M = 2, Nmax = 1024): (S, cps) = (4, 16) runs as chunks of
    whole subjects under a cap of 1 GB, (2, 48) as parts of one subject's chains; one chunk each under the default cap."""
    M, Nmax, iters = 2, max(CHUNK_NOBS), 2
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
        monkeypatch.setenv("NMGP_HAD_BATCH_SLAB_GB", "1")
        chunked = resident(ctx, model, P, hyper, cps, [iters])
        monkeypatch.delenv("NMGP_HAD_BATCH_SLAB_GB")
        whole = resident(ctx, model, P, hyper, cps, [iters])
        assert whole[1].all() and np.all(np.isfinite(whole[0])) and len(set(whole[0][-1, :, 0].tolist())) == S * cps
        assert np.array_equal(hh.bits(chunked[0]), hh.bits(whole[0])) and np.array_equal(chunked[1], whole[1])
        assert np.array_equal(hh.bits(chunked[2]), hh.bits(whole[2]))
    ctx.had_clear_subjects()                             # (gives the prior factors back)


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------------
def poisoned_pads(ctx, model, cases, k=2, iters=3):
    """NaN, 1e300 and the labels -1 / 99 in every padded slot of pars and of the set's x / indx / y: histories and real slots keep
    their bits, no chain dies, and the padded slots of the returned parameters keep their input bits."""
    sizes, M = cc.nobs(cases), cases[0][1]
    Nmax = max(sizes) + 5
    clean = run_unpacked(ctx, model, cases, k, Nmax=Nmax, iters=iters)
    subs = cc.subjects(cases)
    for fill, label in ((np.nan, -1), (1e300, 99)):
        x2, y2 = np.full((len(cases), Nmax), fill), np.full((len(cases), Nmax), fill)
        i2 = np.full((len(cases), Nmax), label, dtype=np.int32)
        for s, c in enumerate(subs):
            x2[s, :sizes[s]], y2[s, :sizes[s]], i2[s, :sizes[s]] = c["x"], c["y"], c["indx"]
        ctx.had_set_subjects_padded(x2, i2, y2, sizes, M)
        P = packed(model, cases, k, Nmax=Nmax, fill=fill)
        if model != "sta":
            pads = hh.padded_slots(model, sizes, M, Nmax, k)
            assert pads.any() and not np.any(np.isfinite(P[pads]) & (np.abs(P[pads]) < 1e299))
        hist, alive, pars = resident(ctx, model, P, hh.hyper_of(model, cases), k, [iters])
        assert alive.tolist() == [True] * len(alive)
        got = (hh.unpack(model, pars, sizes, M, k), [hist[:, s * k:(s + 1) * k] for s in range(len(cases))])
        for s in range(len(cases)):
            assert same_subject(clean, got, s, s), (fill, s)
        if model != "sta":
            assert np.array_equal(hh.bits(pars)[pads], hh.bits(P)[pads])
    ctx.had_subjects_adam_end()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("model", MODELS)
def test_poisoned_pads_are_never_read_or_written(ctx, model, name):
    poisoned_pads(ctx, model, cc.SETS[name])


POISON_SNIPPET = r"""
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import hadamard_cohort_cases as cc
import test_gpu_hadamard_cohort_map as t
from nonstationary_multivariate_gaussian_process_amd import _lib
ctx = _lib.Context(0)
for model in t.MODELS:
    for name in ("A", "C"):
        t.poisoned_pads(ctx, model, cc.SETS[name])
    t.set_subjects(ctx, cc.SET_B)
    assert len(list(t.entry_cases(ctx, model, cc.SET_B, ks=(2,), iters=(3,)))) == 1
ctx.close()
print("POISON_OK")
"""


def test_poisoned_pads_and_workspace():
    """Test 4 on sets A and C and test 1 on set B under NMGP_POISON=1 (read once per process: a fresh child, nothing preloaded), which
    fills fresh buffers and the kept workspace with NaN before every call: a resident buffer or a slab piece that nobody wrote, or a
    padded slot of the moments that somebody read, would show up in the comparisons."""
    env = dict(os.environ)
    env["NMGP_POISON"] = "1"
    env.pop("NMGP_HAD_BATCH_SLAB_GB", None)
    out = subprocess.run([sys.executable, "-c", POISON_SNIPPET % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}],
                         capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0 and "POISON_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


# ---- 5 ----------------------------------------------------------------------------------------------------------------------------------
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


def same_bits_or_nan(a, b):
    """bit identity where the values are numbers, NaN against NaN (an invalid operation's NaN has no agreed sign)"""
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(hh.bits(a)[~na], hh.bits(b)[~nb])


@pytest.mark.parametrize("model", MODELS)
def test_a_failure_stays_in_its_chain(ctx, model):
    cases, k, iters = cc.SET_C, 3, 3
    sizes, M, S = cc.nobs(cases), cases[0][1], len(cases)
    who = cases.index(hc.MINOR)
    bad_row = who * k + 1
    set_subjects(ctx, cases)
    hyper, mask = hh.hyper_of(model, cases), real_mask(model, cases, k)
    others = np.arange(S * k) != bad_row
    good = hh.pack(model, three_chains(model, cases, False), sizes, M)
    base = resident(ctx, model, good, hyper, k, [iters])
    assert base[1].all()

    def dead_from_the_start(start):
        dev = resident(ctx, model, start, hyper, k, [1, iters - 1])
        assert not dev[1][bad_row] and dev[1][others].all() and np.all(np.isnan(dev[0][:, bad_row]))
        assert same_bits_or_nan(dev[2][bad_row][mask[bad_row]], start[bad_row][mask[bad_row]])          # frozen where it started
        assert np.array_equal(hh.bits(dev[0][:, others]), hh.bits(base[0][:, others]))
        assert hh.same_real_bits(dev[2][others], base[2][others], mask[others])
        ref = hm.host_loop(evaluator(ctx, model, hyper, k), start, iters)
        assert hm.same_hist(dev[0], ref[0]) and np.array_equal(dev[1], ref[1]) and same_bits_or_nan(dev[2][mask], ref[2][mask])

    # (a) a chain whose start makes the factorisation fail
    bad = hh.pack(model, three_chains(model, cases, True), sizes, M)
    st = getattr(ctx, hh.ENTRY[model])(bad, hyper, True, False, k)[2]
    assert st[bad_row] not in (0, 1 << 20) and st[others].tolist() == [0] * (S * k - 1)
    dead_from_the_start(bad)
    # (b) a chain with a NaN in a real slot
    nan = good.copy()
    nan[bad_row, np.flatnonzero(mask[bad_row])[-1]] = np.nan
    dead_from_the_start(nan)
    # (c) one subject alone, driven out in the middle of a run by a huge learning rate: the first update makes every real slot
    # non-finite, so iteration 0 is recorded and alive, iteration 1 finds the chain dead, and the parameters stay where the first
    # update put them -- as the host loop has it
    set_subjects(ctx, cases[:1])
    P1, mask1 = packed(model, cases[:1], 1), real_mask(model, cases[:1], 1)
    dev = resident(ctx, model, P1, hyper, 1, [1, 2], lr=1e308)
    ref = hm.host_loop(evaluator(ctx, model, hyper, 1), P1, 3, lr=1e308)
    assert np.all(np.isfinite(dev[0][0])) and np.all(np.isnan(dev[0][1:])) and not dev[1].any()
    assert hm.same_hist(dev[0], ref[0]) and np.array_equal(dev[1], ref[1])
    assert not np.any(np.isfinite(dev[2][mask1])) and same_bits_or_nan(dev[2][mask1], ref[2][mask1])
    ctx.had_subjects_adam_end()


# ---- 6 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_refusals_leave_the_context_usable(ctx, model):
    from nonstationary_multivariate_gaussian_process_amd import _lib
    cases, k = cc.SET_E, 1
    set_subjects(ctx, cases)
    hyper, S = hh.hyper_of(model, cases), len(cases)
    P, mask = packed(model, cases, k), real_mask(model, cases, k)
    W = hh.WIDTH[model]
    code = {"non": 0, "sep": 1, "sta": 2}[model]
    hbuf, abuf = np.empty((2, S * k, W)), np.zeros(S * k, dtype=np.int32)
    ip = ctypes.POINTER(ctypes.c_int)
    hp = _lib.ptr(np.asarray(hyper, dtype=np.float64))

    def raw_adam(niters, hist=hbuf, alive=abuf):
        return ctx.lib.nmgp_had_subjects_adam(ctx.h, niters, LR, 0.9, 0.999, 1e-8, None if hist is None else _lib.ptr(hist),
                                              None if alive is None else alive.ctypes.data_as(ip))

    def message():
        return ctx.lib.nmgp_last_error(ctx.h).decode()

    def still_good():
        agree(resident(ctx, model, P, hyper, k, [5]), hm.host_loop(evaluator(ctx, model, hyper, k), P, 5), mask, P)

    ctx.had_subjects_adam_end()
    with pytest.raises(_lib.NmgpError, match="error -3.*adam_begin must be called first"):              # no begin
        ctx.had_subjects_adam(2, LR)
    with pytest.raises(_lib.NmgpError, match="error -3.*adam_begin must be called first"):
        ctx.had_subjects_adam_get_pars()
    ctx.had_subjects_adam_end()                                                                         # (ending nothing is no error)
    still_good()
    for bad_model in (-1, 3):                                                                           # a bad model
        assert ctx.lib.nmgp_had_subjects_adam_begin(ctx.h, bad_model, _lib.ptr(P), S * k, k, hp, 1) == -2 and "model" in message()
    with pytest.raises(_lib.NmgpError):
        ctx.had_subjects_adam_begin("whitened", P, hyper, True, k)
    for B_, k_ in ((S * k, 2), (S * k, 0), (1, 1)):                                                     # B != S cps
        assert ctx.lib.nmgp_had_subjects_adam_begin(ctx.h, code, _lib.ptr(P), B_, k_, hp, 1) == -2 and "chains_per_subject" in message()
    assert ctx.lib.nmgp_had_subjects_adam_begin(ctx.h, code, None, S * k, k, hp, 1) == -1 and "NULL" in message()        # NULL arguments
    assert ctx.lib.nmgp_had_subjects_adam_begin(ctx.h, code, _lib.ptr(P), S * k, k, None, 1) == -1 and "NULL" in message()
    # the same refusals through the binding, caught by a caller who then goes on with the earlier run
    for P_, k_ in ((P, k + 1), (P, 0), (P[:1], 1)):
        with pytest.raises(_lib.NmgpError, match="error -2.*chains_per_subject"):
            ctx.had_subjects_adam_begin(model, P_, hyper, True, k_)
    # ... all of which left the begun run of still_good() alone, on the device and in the binding's record of its shape: two more
    # iterations are iterations 6 and 7 of the host loop, and the parameters are the host loop's after 7
    more, alive = ctx.had_subjects_adam(2, LR)
    ref = hm.host_loop(evaluator(ctx, model, hyper, k), P, 7)
    assert more.shape == (2, S * k, W) and hm.same_hist(more, ref[0][5:]) and np.array_equal(alive, ref[1])
    got = ctx.had_subjects_adam_get_pars()
    assert got.shape == P.shape and hh.same_real_bits(got, ref[2], mask)
    assert raw_adam(2, hist=None) == -1 and "NULL" in message()
    assert raw_adam(2, alive=None) == -1 and "NULL" in message()
    assert ctx.lib.nmgp_had_subjects_adam_get_pars(ctx.h, None) == -1 and "NULL" in message()
    for n in (0, -3):                                                                                   # niters < 1
        assert raw_adam(n) == -2 and "niters" in message()
    over = (1 << 24) // (S * k * W) + 1                                                                 # a history above the cap
    assert raw_adam(over) == -2 and "NMGP_HAD_ADAM_HIST_MAX" in message()
    assert hh.same_real_bits(ctx.had_subjects_adam_get_pars(), ref[2], mask)                            # the run is where it was
    still_good()
    ctx.had_clear_subjects()                                                                            # the set ends the optimiser
    assert raw_adam(2) == -3 and "nmgp_had_set_subjects must be called first" in message()
    assert ctx.lib.nmgp_had_subjects_adam_begin(ctx.h, code, _lib.ptr(P), S * k, k, hp, 1) == -3
    set_subjects(ctx, cases)
    assert raw_adam(2) == -3 and "adam_begin must be called first" in message()
    still_good()
    set_subjects(ctx, cases)                                                                            # ... and so does a new set
    with pytest.raises(_lib.NmgpError, match="error -3"):
        ctx.had_subjects_adam(2, LR)
    with pytest.raises(_lib.NmgpError, match="error -3"):
        ctx.had_subjects_adam_get_pars()
    still_good()
    # a run that the binding has no record of (begun through the library directly): the binding hands over no buffers, the entries
    # refuse the NULL pointers and write nothing; the run itself is intact
    ctx.had_subjects_adam_end()
    assert ctx.lib.nmgp_had_subjects_adam_begin(ctx.h, code, _lib.ptr(P), S * k, k, hp, 1) == 0
    with pytest.raises(_lib.NmgpError, match="error -1"):
        ctx.had_subjects_adam(2, LR)
    with pytest.raises(_lib.NmgpError, match="error -1"):
        ctx.had_subjects_adam_get_pars()
    assert raw_adam(2) == 0 and hm.same_hist(hbuf, hm.host_loop(evaluator(ctx, model, hyper, k), P, 2)[0])
    still_good()
    ctx.had_subjects_adam_end()


# ---- 7 ----------------------------------------------------------------------------------------------------------------------------------
_POOL = []


def contexts(n):
    """n contexts of a pool shared by the driver tests (a driver sets its own subjects on them; closed with the process)"""
    from nonstationary_multivariate_gaussian_process_amd import _lib
    while len(_POOL) < n:
        _POOL.append(_lib.Context(0))
    return _POOL[:n]


def teardown_module(module):
    while _POOL:
        _POOL.pop().close()


@pytest.mark.parametrize("waste", [0.0, 0.5])
@pytest.mark.parametrize("name", ("A", "C"))
@pytest.mark.parametrize("model", MODELS)
def test_driver_resident_loop_is_the_host_loop(model, name, waste):
    """device_resident=True against False at iters_per_call 1, 2 and 50: parameters, hist, alive and the callbacks' sequence, bit
    for bit; a trajectory begun on a bucket's context before the MAP run returns its bits afterwards; predict works on the contexts
    after a resident run and gives the host run's bits."""
    from nonstationary_multivariate_gaussian_process_amd import drivers, hadamard
    cases, k, iters = cc.SETS[name], 2, 5
    S = len(cases)
    ctxs = contexts(len(hadamard.cohort_buckets(cc.nobs(cases), waste)))
    xs = [c["xs"] for c in cc.subjects(cases)]

    def run(**kw):
        d = getattr(drivers, hm.DRIVER[model])(hh.subject_triples(cases), hh.hyper_dict(model, cases), hh.chains(model, cases, k), lr=LR,
                                               chains_per_subject=k, max_flop_waste=waste, ctxs=ctxs, **kw)
        calls, traj = [], None
        if kw.get("device_resident"):
            # a trajectory on the first bucket's set, put back by a commit that rejects every chain
            c0, idx = d.ctxs[0], [int(s) for s in d.buckets[0]]
            q, eps = d.maps[0].P.copy(), hh.eps_of(len(idx))
            p0 = np.random.default_rng(77).standard_normal(q.shape)              # (padded slots are never read)
            c0.had_subjects_traj_begin(model, q, d.hyper, True, k)
            first = c0.had_subjects_traj(eps, 2, p0, want_p1=True, want_kin=True)
            c0.had_subjects_traj_commit(np.zeros(q.shape[0], dtype=bool))
            traj = (c0, eps, p0, first)
        res = d.run(iters, lambda i, h: calls.append((i, h.copy())))
        if traj is not None:
            c0, eps, p0, first = traj
            second = c0.had_subjects_traj(eps, 2, p0, want_p1=True, want_kin=True)
            for a, b in zip(first, second):
                assert np.array_equal(hh.bits(a) if a.dtype == np.float64 else a, hh.bits(b) if b.dtype == np.float64 else b)
            c0.had_subjects_traj_end()
        pred = d.predict(res[0], xs)
        d.close()
        return res, calls, pred

    (hp, hhist, halive), hcalls, hpred = run(device_resident=False)
    assert halive.all() and np.all(np.isfinite(hhist)) and [i for i, _ in hcalls] == list(range(iters))
    for per_call in (1, 2, 50):
        (rp, rhist, ralive), rcalls, rpred = run(device_resident=True, iters_per_call=per_call)
        assert np.array_equal(hh.bits(rhist), hh.bits(hhist)) and np.array_equal(ralive, halive), (model, name, waste, per_call)
        for s in range(S):
            assert rp[s].shape == hp[s].shape and np.array_equal(hh.bits(rp[s]), hh.bits(hp[s])), (model, name, waste, per_call, s)
        assert [i for i, _ in rcalls] == [i for i, _ in hcalls]
        assert all(np.array_equal(hh.bits(a), hh.bits(b)) for (_, a), (_, b) in zip(rcalls, hcalls))
        for a, b in zip(rpred, hpred):
            assert a[-1] == 0 and b[-1] == 0 and np.all(np.isfinite(a[0]))
            assert all(np.array_equal(hh.bits(u), hh.bits(v)) for u, v in zip(a[:-1], b[:-1]))
