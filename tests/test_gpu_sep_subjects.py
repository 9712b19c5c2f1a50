"""Separable model, many subjects per launch sequence (nmgp_sep_batch_set_subjects_chains; run with -m gpu on an MI355X): every batch
element of nmgp_sep_batch_eval reads ITS subject's x, Y and GP-prior factors.  Checked against the resident path (the subject made
resident, its chains passed to sep_batch_eval), against the CPU oracle on the chain's own subject, and -- where the arithmetic is the
same -- to the bit.  Subjects come from sim.simulate_separable with one seed each; subject 1 of every set has its inputs warped and
shuffled, so that no kernel can rely on sorted or evenly spaced x."""
import numpy as np
import pytest

from conftest import SEP_KEYS, record_parity, relerr, vec_relerr

pytestmark = pytest.mark.gpu

VAL_TOL = 1e-6          # the project's parity bars against the reference / oracle (tests/test_gpu_parity.py)
GRAD_TOL = 1e-5


@pytest.fixture(scope="module")
def ctx():
    from nonstationary_multivariate_gaussian_process_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def hyper_sep(same=True):
    """sim.HYPER_SEP; same=False gives tilde_sigma its own (alpha, beta): two prior factors per subject instead of one shared."""
    from nonstationary_multivariate_gaussian_process_amd import sim
    h = dict(sim.HYPER_SEP)
    if not same:
        h["alpha_tilde_sigma"], h["beta_tilde_sigma"] = 8.0, 0.7
    return h, [h[k] for k in SEP_KEYS]


_SUBJECTS = {}


def subjects(N, M, S, seed0):
    """xs [S, N], Ys [S, N, M], generating parameters [S, P]; distinct subjects, subject 1 warped and shuffled.  Computed once."""
    from nonstationary_multivariate_gaussian_process_amd import sim
    key = (N, M, S, seed0)
    if key not in _SUBJECTS:
        xs, Ys, ps = [], [], []
        for s in range(S):
            d = sim.simulate_separable(N, M, seed0 + s)
            x, Y, p = d["x"], d["Y"], d["pars_true"].copy()
            if s == 1:
                perm = np.random.default_rng(1000 + seed0).permutation(N)
                x, Y = (0.8 * x + 0.2 * x * x)[perm], Y[perm]
                p[:N], p[N:2 * N] = p[:N][perm], p[N:2 * N][perm]
            xs.append(x), Ys.append(Y), ps.append(p)
        _SUBJECTS[key] = (np.ascontiguousarray(np.stack(xs)), np.ascontiguousarray(np.stack(Ys)), np.stack(ps))
        for a in _SUBJECTS[key]:
            a.setflags(write=False)
    return _SUBJECTS[key]


def chains(ps, k, scale=0.03):
    """[S * k, P]: row s * k + j is chain j of subject s, a smooth perturbation of the subject's generating parameters."""
    from nonstationary_multivariate_gaussian_process_amd import sim
    return np.stack([sim.perturb(ps[s], scale, 0.3 + 0.2 * j + 0.07 * s) for s in range(ps.shape[0]) for j in range(k)])


def oracle_row(pars, Y, x, h):
    from oracle import nmgp_oracle as O
    ref, gref = O.nlogpos_obj(pars, Y, x, **h, verbose=True, grad=True)
    return np.asarray(ref, dtype=np.float64), gref


# ---------------------------------------------------------------------------------------------------
# 1. own subject
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("same", [True, False], ids=["one_prior_pair", "two_prior_pairs"])
@pytest.mark.parametrize("N,M,S,k", [(64, 3, 3, 2), (130, 2, 2, 3), (201, 5, 2, 2), (1024, 5, 4, 4)])
def test_every_chain_is_evaluated_on_its_own_subject(ctx, N, M, S, k, same):
    """(64, 3): fused-step schedule; (130, 2): the 128 x 32 tile edge of k_sep_blocks_b4; (201, 5): the 64 x 64 kernel of odd N;
    (1024, 5) x 16 chains: the throughput schedule.  Bars against the resident path: those of the batch-vs-single test
    (likelihood 1e-10, out6 1e-9, gradient 1e-8); against the oracle at N <= 201: VAL_TOL / GRAD_TOL."""
    h, hv = hyper_sep(same)
    xs, Ys, ps = subjects(N, M, S, 40)
    pars = chains(ps, k)
    ctx.set_data(xs[0], Ys[0])
    ctx.sep_batch_set_subjects(xs, Ys, k)
    out, grad, st = ctx.sep_batch_eval(pars, hv, True, True)
    outv, gv, stv = ctx.sep_batch_eval(pars, hv, True, False)
    assert gv is None and list(st) == [0] * (S * k) and list(stv) == [0] * (S * k)
    assert np.all(np.isfinite(out)) and np.all(np.isfinite(grad))
    worst = dict(loglik=0.0, out6=0.0, out6_value_only=0.0, grad=0.0)
    for s in range(S):
        ctx.set_data(xs[s], Ys[s])                       # (drops the set: the resident path)
        ro, rg, rs = ctx.sep_batch_eval(pars[s * k:(s + 1) * k], hv, True, True)
        assert np.all(rs == 0)
        for j in range(k):
            b = s * k + j
            e = dict(loglik=relerr(out[b][1], ro[j][1]), out6=relerr(out[b], ro[j]), out6_value_only=relerr(outv[b], ro[j]),
                     grad=vec_relerr(grad[b], rg[j]))
            print("N=%d M=%d S=%d k=%d same=%s chain %d vs resident: %s" % (N, M, S, k, same, b, e))
            worst = {key: max(worst[key], e[key]) for key in worst}
    record_parity("sepsubj_N%d_M%d_S%d_k%d_%s_vs_resident" % (N, M, S, k, "same" if same else "diff"), loglik=(worst["loglik"], 1e-10),
                  out6=(worst["out6"], 1e-9), out6_value_only=(worst["out6_value_only"], 1e-9), grad=(worst["grad"], 1e-8))
    assert worst["loglik"] < 1e-10 and worst["out6"] < 1e-9 and worst["out6_value_only"] < 1e-9 and worst["grad"] < 1e-8, worst
    if N <= 201:
        wv = wg = 0.0
        for b in range(S * k):
            ref, gref = oracle_row(pars[b], Ys[b // k], xs[b // k], h)
            wv, wg = max(wv, relerr(out[b][0], ref[0])), max(wg, vec_relerr(grad[b], gref))
        print("N=%d M=%d S=%d k=%d same=%s vs oracle: neglog %.3g grad %.3g" % (N, M, S, k, same, wv, wg))
        record_parity("sepsubj_N%d_M%d_S%d_k%d_%s_vs_oracle" % (N, M, S, k, "same" if same else "diff"), neglog=(wv, VAL_TOL),
                      grad=(wg, GRAD_TOL))
        assert wv < VAL_TOL and wg < GRAD_TOL, (wv, wg)


# ---------------------------------------------------------------------------------------------------
# 2. same bits as the resident path
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,M,S,k", [(64, 3, 4, 2), (1024, 5, 2, 4)])
def test_copies_of_one_subject_give_the_resident_paths_bits(ctx, N, M, S, k):
    """S copies of one subject x k chains: the set's kernels do the resident path's arithmetic in its order, so the likelihood and the
    likelihood-only gradient are the same bits; the prior terms are solved by substitution here and by the library there (1e-9)."""
    _, hv = hyper_sep()
    xs, Ys, ps = subjects(N, M, 2, 60)
    x, Y = xs[1], Ys[1]
    pars = chains(np.stack([ps[1]] * S), k)
    ctx.set_data(x, Y)
    r0 = ctx.sep_batch_eval(pars, hv, False, True)
    r1 = ctx.sep_batch_eval(pars, hv, True, True)
    ctx.sep_batch_set_subjects(np.stack([x] * S), np.stack([Y] * S), k)
    s0 = ctx.sep_batch_eval(pars, hv, False, True)
    s1 = ctx.sep_batch_eval(pars, hv, True, True)
    assert np.all(r0[2] == 0) and np.all(s0[2] == 0) and np.all(r1[2] == 0) and np.all(s1[2] == 0)
    assert np.array_equal(s0[0][:, 1], r0[0][:, 1]) and np.array_equal(s0[1], r0[1])
    assert np.array_equal(s1[0][:, 1], r1[0][:, 1])
    e = max(relerr(s1[0][b], r1[0][b]) for b in range(S * k))
    print("N=%d S=%d k=%d prior columns vs resident: %.3g" % (N, S, k, e))
    assert e < 1e-9, e
    ctx.sep_batch_clear_subjects()


# ---------------------------------------------------------------------------------------------------
# 3. permutation of the subjects
# ---------------------------------------------------------------------------------------------------
def test_reversing_the_subjects_reverses_the_rows(ctx):
    N, M, S, k = 130, 2, 3, 2
    _, hv = hyper_sep(False)
    xs, Ys, ps = subjects(N, M, S, 70)
    pars = chains(ps, k)
    ctx.set_data(xs[0], Ys[0])
    ctx.sep_batch_set_subjects(xs, Ys, k)
    out, grad, st = ctx.sep_batch_eval(pars, hv, True, True)
    # subjects reversed, each subject's chains kept in their order
    rows = np.arange(S * k).reshape(S, k)[::-1].reshape(-1)
    ctx.sep_batch_set_subjects(xs[::-1], Ys[::-1], k)
    out_r, grad_r, st_r = ctx.sep_batch_eval(pars[rows], hv, True, True)
    assert np.all(st == 0) and np.all(st_r == 0)
    assert np.array_equal(out_r, out[rows]) and np.array_equal(grad_r, grad[rows])
    ctx.sep_batch_clear_subjects()


# ---------------------------------------------------------------------------------------------------
# 4. chunks
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,k,lines", [(625, 4, (2424, 2427)), (2, 2500, (2427, 2500, 4927))])
def test_chunks_are_aligned_to_subjects(ctx, monkeypatch, S, k, lines):
    """N = 64, M = 3, gradients on, NMGP_SEP_BATCH_SLAB_GB=1 (the floor of that setting): sep_batch_layout takes 51,498 doubles per
    chain, so a chunk holds floor(1e9 / (8 * 51,498)) = 2,427 chains.  (625, 4): the chunk is rounded down to 606 subjects, the first
    chunk ends at chain 2,424 (2,427 is where an unaligned chunk would end).  (2, 2500): a subject does not fit in a chunk and is
    split at 2,427; the next chunk begins with the next subject at 2,500 and is split at 4,927.  Every 97th chain and the chains on both
    sides of each line against the oracle on the chain's OWN subject (all subjects are distinct).
    Measures: the likelihood within 1e-8 and the gradient within GRAD_TOL, as every separable-vs-oracle comparison of test_gpu_parity.py;
    NegLog within VAL_TOL of the SIZE OF ITS TERMS, sum_k |out6[k]|, k = 1..5.  At N = 64 NegLog is of order 1 as the difference of
    terms of order 100, and the two GP-prior terms carry the error of their ill-conditioned covariance factor (RBF + 1e-6 I: about
    1e-8 of the term, here as in the oracle's LAPACK factor), so an error relative to NegLog itself measures the cancellation, not
    the evaluation.  A wrong subject moves the likelihood in its leading digits."""
    N, M = 64, 3
    h, hv = hyper_sep()
    xs, Ys, ps = subjects(N, M, S, 200)
    pars = chains(ps, k, scale=0.02)
    B = S * k
    monkeypatch.setenv("NMGP_SEP_BATCH_SLAB_GB", "1")
    ctx.set_data(xs[0], Ys[0])
    ctx.sep_batch_set_subjects(xs, Ys, k)
    out, grad, st = ctx.sep_batch_eval(pars, hv, True, True)
    ctx.sep_batch_clear_subjects()
    assert np.all(st == 0) and np.all(np.isfinite(out)) and np.all(np.isfinite(grad))
    check = sorted(set(range(0, B, 97)) | {b for ln in lines for b in (ln - 1, ln)} | {B - 1})
    wv = wl = wg = 0.0
    for b in check:
        ref, gref = oracle_row(pars[b], Ys[b // k], xs[b // k], h)
        ev, eg = abs(out[b][0] - ref[0]) / np.sum(np.abs(ref[1:])), vec_relerr(grad[b], gref)
        el = relerr(out[b][1], ref[1])
        assert ev < VAL_TOL and el < 1e-8 and eg < GRAD_TOL, (b, b // k, ev, el, eg, out[b], ref)
        wv, wl, wg = max(wv, ev), max(wl, el), max(wg, eg)
    print("chunks S=%d k=%d: %d chains checked, neglog (on the scale of its terms) %.3g loglik %.3g grad %.3g" % (S, k, len(check), wv, wl, wg))
    record_parity("sepsubj_chunks_S%d_k%d_vs_oracle" % (S, k), neglog_on_the_scale_of_its_terms=(wv, VAL_TOL), loglik=(wl, 1e-8),
                  grad=(wg, GRAD_TOL))


# ---------------------------------------------------------------------------------------------------
# 5. a singular chain
# ---------------------------------------------------------------------------------------------------
def test_a_singular_chain_is_retried_on_its_own_subject(ctx):
    """The numerically singular chain of test_gpu_parity.py (a zero row of B, sigma2 = 0) as chain 1 of subject 1 in a 2 x 2 set:
    it goes through the single-chain entry's jitter retries ON SUBJECT 1, the other chains do not notice, and the resident subject
    (with its cached prior factors) is back afterwards."""
    N, M, S, k = 96, 3, 2, 2
    _, hv = hyper_sep()
    xs, Ys, ps = subjects(N, M, 3, 90)
    resident = (xs[2], Ys[2], ps[2])                    # neither of the set's subjects
    xs, Ys, ps = xs[:2], Ys[:2], ps[:2]
    good = chains(ps, k, scale=0.0)
    T = M * (M + 1) // 2
    sing = good[3].copy()
    uL = sing[2 * N:2 * N + T].copy()
    uL[1], uL[2], uL[4] = 0.0, -800.0, 0.0
    sing[2 * N:2 * N + T] = uL
    sing[-1] = -800.0
    bad = good.copy()
    bad[3] = sing
    ctx.set_data(resident[0], resident[1])
    before = ctx.logpos_sep(resident[2], hv, True, True)
    ctx.sep_batch_set_subjects(xs, Ys, k)
    out_g, grad_g, st_g = ctx.sep_batch_eval(good, hv, False, True)
    out, grad, st = ctx.sep_batch_eval(bad, hv, False, True)
    assert list(st_g) == [0, 0, 0, 0] and list(st) == [0, 0, 0, 1], (st_g, st)
    assert np.array_equal(out[:3], out_g[:3]) and np.array_equal(grad[:3], grad_g[:3])
    after = ctx.logpos_sep(resident[2], hv, True, True)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    # the set is still active and still evaluates every chain on its subject
    again = ctx.sep_batch_eval(good, hv, False, True)
    assert np.array_equal(again[0], out_g) and np.array_equal(again[1], grad_g)
    ctx.set_data(xs[1], Ys[1])
    s_bad, g_bad = ctx.logpos_sep(sing, hv, False, True)
    assert relerr(out[3][:2], s_bad[:2]) < 1e-12 and np.all(np.isfinite(grad[3])) and vec_relerr(grad[3], g_bad) < 1e-10


def test_one_chain_sets_and_the_eigen_formulation_use_the_chains_subject(monkeypatch):
    """B == 1 and NMGP_SEP=eig have no batched path: the chains go through nmgp_logpos_sep, each on its own subject."""
    from nonstationary_multivariate_gaussian_process_amd import _lib
    N, M = 64, 3
    _, hv = hyper_sep()
    xs, Ys, ps = subjects(N, M, 3, 40)
    pars = chains(ps, 1)
    for algo in ("chol", "eig"):
        monkeypatch.setenv("NMGP_SEP", algo)
        c = _lib.Context(0)
        try:
            c.set_data(xs[0], Ys[0])
            c.sep_batch_set_subjects(xs[1:2], Ys[1:2], 1)
            o1, g1, s1 = c.sep_batch_eval(pars[1:2], hv, True, True)
            c.sep_batch_set_subjects(xs, Ys, 1)
            o3, g3, s3 = c.sep_batch_eval(pars, hv, True, True)
            keep = c.logpos_sep(pars[0], hv, True, True)          # the resident subject is subject 0 again
            assert s1[0] == 0 and np.all(s3 == 0)
            for s in range(3):
                c.set_data(xs[s], Ys[s])
                so, sg = c.logpos_sep(pars[s], hv, True, True)
                if s == 0:
                    assert np.array_equal(keep[0], so) and np.array_equal(keep[1], sg)
                if s == 1:
                    assert np.array_equal(o1[0], so) and np.array_equal(g1[0], sg)
                if algo == "eig":
                    assert np.array_equal(o3[s], so) and np.array_equal(g3[s], sg)
                else:
                    assert relerr(o3[s][1], so[1]) < 1e-10 and relerr(o3[s], so) < 1e-9 and vec_relerr(g3[s], sg) < 1e-8
        finally:
            c.close()


# ---------------------------------------------------------------------------------------------------
# 6. state
# ---------------------------------------------------------------------------------------------------
def test_state_and_lifetime_of_the_set(ctx):
    from nonstationary_multivariate_gaussian_process_amd import _lib, sim
    N, M = 64, 3
    _, hv = hyper_sep()
    xs, Ys, ps = subjects(N, M, 3, 40)
    pars = chains(ps, 2)
    fresh = _lib.Context(0)
    try:
        with pytest.raises(_lib.NmgpError, match="error -3"):                  # NMGP_E_STATE: no resident subject yet
            fresh.sep_batch_set_subjects(xs, Ys, 2)
    finally:
        fresh.close()
    ctx.set_data(xs[0], Ys[0])
    base = ctx.sep_batch_eval(pars[:5], hv, True, True)                        # resident path: 5 chains of subject 0
    for bad_args in ((xs, Ys, 0), (xs[:0], Ys[:0], 1)):
        with pytest.raises(_lib.NmgpError, match="error -2"):
            ctx.sep_batch_set_subjects(*bad_args)
    ctx.sep_batch_set_subjects(xs, Ys, 2)
    with pytest.raises(_lib.NmgpError, match=r"error -2.*B = 5.*3 subjects x 2 chains = 6"):
        ctx.sep_batch_eval(pars[:5], hv, True, True)
    full = ctx.sep_batch_eval(pars, hv, True, True)
    assert np.all(full[2] == 0)

    def resident_again():
        r = ctx.sep_batch_eval(pars[:5], hv, True, True)
        return all(np.array_equal(a, b) for a, b in zip(r, base))

    ctx.sep_batch_clear_subjects()
    assert resident_again()
    ctx.sep_batch_clear_subjects()                                             # (nothing to clear: not an error)
    ctx.sep_batch_set_subjects(xs, Ys, 2)
    ctx.set_data(xs[0].copy(), Ys[0].copy())                                   # identical data: the upload is skipped, the set must go
    assert resident_again()
    ctx.sep_batch_set_subjects(xs, Ys, 2)
    d = sim.simulate_separable(N, M, 5)
    ctx.set_data(d["x"], d["Y"])                                               # another subject
    ctx.sep_batch_eval(pars[:5], hv, True, False)                              # (B = 5 is accepted: no set)
    ctx.set_data(xs[0], Ys[0])
    assert resident_again()
    ctx.sep_batch_set_subjects(xs, Ys, 2)
    ctx.had_set_data(np.tile(xs[0], M), np.repeat(np.arange(M), N), Ys[0].T.reshape(-1))
    with pytest.raises(_lib.NmgpError, match="error -3"):                      # a Hadamard subject: no complete-data entry runs
        ctx.sep_batch_eval(np.zeros((5, 2 * ctx.N + ctx.T + 1)), hv, True, True)
    ctx.set_data(xs[0], Ys[0])
    assert resident_again()
    # a second set with another S replaces the first
    ctx.sep_batch_set_subjects(xs, Ys, 2)
    ctx.sep_batch_set_subjects(xs[1:], Ys[1:], 1)
    with pytest.raises(_lib.NmgpError, match="error -2"):
        ctx.sep_batch_eval(pars, hv, True, True)
    two = ctx.sep_batch_eval(pars[[2, 4]], hv, True, True)
    assert np.all(two[2] == 0)
    for r, b in enumerate((2, 4)):
        assert relerr(two[0][r][1], full[0][b][1]) < 1e-10 and relerr(two[0][r], full[0][b]) < 1e-9
        assert vec_relerr(two[1][r], full[1][b]) < 1e-8
    ctx.sep_batch_clear_subjects()


# ---------------------------------------------------------------------------------------------------
# 7. drivers
# ---------------------------------------------------------------------------------------------------
def test_batched_map_separable(ctx):
    from nonstationary_multivariate_gaussian_process_amd import drivers as D, sim
    N, M, S, k = 64, 3, 3, 2
    h, hv = hyper_sep()
    xs, Ys, ps = subjects(N, M, S, 40)
    # S copies of one subject, likelihood-only objective: the parameter history of a LockStepMAP on the resident path, to the bit
    x, Y = xs[1], Ys[1]
    init = chains(np.stack([ps[1]] * S), k, scale=0.3)
    m = D.BatchedMAPSeparable(np.stack([x] * S), np.stack([Y] * S), h, init, ctx=ctx, chains_per_subject=k)
    m.prior = False
    hist = []
    for _ in range(5):
        m.step()
        hist.append(m.P.copy())

    class Resident(D.LockStepMAP):
        def value_and_grad(self, P):
            out, grad, status = ctx.sep_batch_eval(P, hv, False, True)
            return out, grad, np.where(status < 0, status, 0)

    ctx.set_data(x, Y)
    r = Resident(init)
    for i in range(5):
        r.step()
        assert np.array_equal(r.P, hist[i]), i
    assert np.all(m.alive) and not np.array_equal(hist[0], init)
    # distinct subjects, the full objective: the first iteration reports sep_batch_eval's rows; 20 Adam steps lower every NegLog.
    # (lr = 2e-3: Adam moves every coordinate by about lr per step, and the GP priors weigh rough directions of tilde_l / tilde_sigma
    # with 1 / jitter = 1e6 -- at the reference's lr = 0.2 the first iterations RAISE NegLog by orders of magnitude, on the CPU oracle
    # as here, before the moments settle.  At 2e-3 the oracle's NegLog falls monotonically from this start, by > 100 in every row.)
    init = chains(ps, k, scale=0.3)
    m = D.BatchedMAPSeparable(xs, Ys, h, init, lr=2e-3, ctx=ctx, chains_per_subject=k)
    direct = ctx.sep_batch_eval(init, hv, True, True)
    neglog0, out0 = m.step()
    assert np.array_equal(out0, direct[0]) and np.array_equal(neglog0, direct[0][:, 0])
    for _ in range(19):
        neglog, _ = m.step()
    final = ctx.sep_batch_eval(m.P, hv, True, False)[0][:, 0]
    print("BatchedMAPSeparable NegLog start %s after 20 %s" % (neglog0, final))
    assert np.all(m.alive) and np.all(final < neglog0) and np.all(neglog < neglog0)
    with pytest.raises(ValueError):
        D.BatchedMAPSeparable(xs, Ys, h, init[:-1], ctx=ctx, chains_per_subject=k)
    ctx.sep_batch_clear_subjects()


def test_batched_hmc_separable_with_several_subjects(ctx):
    from nonstationary_multivariate_gaussian_process_amd import drivers as D
    N, M, S, k = 64, 3, 2, 2
    h, hv = hyper_sep()
    xs, Ys, ps = subjects(N, M, 3, 40)
    xs, Ys, ps = xs[:S], Ys[:S], ps[:S]
    q0 = chains(ps, k)                                  # the chains of test 1's (64, 3) case, subjects 0 and 1
    kw = dict(step_size=2e-4, num_steps_in_leap=3, seed=11, ctx=ctx)
    hmc = D.BatchedHMCSeparable(xs, Ys, h, q0, **kw)
    U, g = hmc.potential_and_grad(q0)
    out, grad, st = ctx.sep_batch_eval(q0, hv, True, True)
    assert np.all(st == 0) and np.array_equal(U, out[:, 0]) and np.array_equal(g, grad)
    for b in range(S * k):                               # ... which are the chain's own subject's (the oracle, as in test 1)
        ref, gref = oracle_row(q0[b], Ys[b // k], xs[b // k], h)
        assert relerr(U[b], ref[0]) < VAL_TOL and vec_relerr(g[b], gref) < GRAD_TOL
    samples, info = hmc.run(3)
    samples2, _ = D.BatchedHMCSeparable(xs, Ys, h, q0, **kw).run(3)
    assert np.array_equal(samples, samples2) and samples.shape == (3, S * k, q0.shape[1])
    # every subject's chains alone (one-dimensional x: the resident path), same random streams (chain b draws from seed + b)
    for s in range(S):
        one = D.BatchedHMCSeparable(xs[s], Ys[s], h, q0[s * k:(s + 1) * k], **dict(kw, seed=11 + s * k))
        alone, info1 = one.run(3)
        assert np.array_equal(info1["accept_rate"], info["accept_rate"][s * k:(s + 1) * k])
        assert np.allclose(alone, samples[:, s * k:(s + 1) * k], rtol=0.0, atol=1e-9)
    with pytest.raises(ValueError, match="multiple"):
        D.BatchedHMCSeparable(xs, Ys, h, q0[:3], **kw)
    P = q0.shape[1]
    T = M * (M + 1) // 2
    metric = D.SeparablePriorMetric(np.eye(N), np.eye(N), 1.0, T)
    assert metric.P == P
    with pytest.raises(ValueError, match="subject"):
        D.BatchedHMCSeparable(xs, Ys, h, q0, M=metric, **kw)
    # one-dimensional x behaves as before: no set is left behind
    one = D.BatchedHMCSeparable(xs[0], Ys[0], h, q0[:3], **kw)
    U1, _ = one.potential_and_grad(q0[:3])
    assert np.all(np.isfinite(U1))
