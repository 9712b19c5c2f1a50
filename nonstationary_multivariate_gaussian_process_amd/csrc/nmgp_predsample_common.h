// The six posterior-draw prediction entries (nmgp_predsample_svc / _sep / _sta / _hads / _had, nmgp_predict_hadst) share ONE host
// schedule: H parameter vectors of the resident subject -> predictive means and variances at S new inputs.  This header holds it.
//
// ps_predict<Model>: argument checks -> slice and chunk sizes -> one workspace carved out of ctx->ps_buf -> the two priors projected
// once per call -> per chunk of draws: upload, unpack, starred values, per slice of new inputs {covariance, y and the
// cross-covariance rows riding below it, batched nmgp_potrf, ps_rows_reduce}, variance, four downloads, ONE synchronisation, status.
// A Model is a struct of static members, nothing virtual, in the translation unit that has its kernels:
//   P(N, T)                   length of a parameter vector
//   star_width(T)             starred values per draw and input (0: no latent regression, no hyper, star_out not written)
//   order(N, M), mats(M)      order of a matrix and matrices per draw (kron: M of order N; svc: one of order N M; else one of order N)
//   rows(M, indexed)          riding cross-covariance rows per new input
//   smax(N, M, indexed)       new inputs per factorisation
//   PRECISE                   nmgp_potrf's `precise`
//   NAN_PARS, RESETS_KIND     the two status / state rules of the Hadamard entries (see PsHadamard)
//   require(c)                state and algorithm requirements, with their messages
//   size_guard(k)             what the model's kernels can index
//   chunk_doubles(k)          the per-draw size nmgp_ps_chunk is asked about
//   y_rows(k, stride)         the data row(s) riding below the matrices
//   extras(k, take, B)        the model's own pieces of the workspace (the o_* fields below the common ones)
//   host_prep(k)              host work on the chunk's parameter vectors before they are uploaded (kron: its host Jacobi)
//   prep / star / build_cov / cross_rows / finish (k)   hooks: unpacking, starred values of a chunk, covariance and riding rows of a
//                             slice, mean / variance of a chunk
// Every hook receives the call (PsCall) and returns 0 or an error code.
#pragma once

#include "nmgp_internal.h"

#include <algorithm>
#include <vector>

// what a model hook sees of a call; the chunk (Bc) and slice (s0, Sc, E) fields follow the loops
struct PsCall {
    nmgp_ctx* c;
    const double *hyper, *hpars;     // hpars: the chunk's parameter vectors on the host
    int flags;                       // svc: constrained; sep: kss_jitter
    int N, M, T, S;
    long long P;
    bool indexed;                    // indx_star given: one output per new input
    int n, mats, per, Emax, ld;      // matrix order, matrices per draw, riding rows per input and per slice at most, leading dimension
    long long bs;                    // stride between matrices
    int Bc, s0, Sc, E;
    double* w;                       // workspace base; pieces absent from a call are nullptr
    double *xs, *W0, *W1, *cv0, *cv1, *pars, *star, *z, *mean, *dots, *sqs, *var, *Sb;
    const int* is;
    size_t o_ell, o_sig, o_Lv, o_Rv, o_small, o_yt;      // Model::extras
    std::vector<double> host;        // a model's host staging, alive until the chunk's synchronisation (kron: the eigenpairs)
    double* at(size_t o) const { return w + o; }
};

// what the three Hadamard models share: one matrix of order N per draw, indexed form, the resident subject's own y
struct PsHadamard {
    static void host_prep(PsCall&) {}
    static int order(int N, int) { return N; }
    static int mats(int) { return 1; }
    static int rows(int M, bool indexed) { return indexed ? 1 : M; }
    // at most N riding rows (the slices of the MAP predictors in the full form)
    static int smax(int N, int M, bool indexed) { return indexed ? N : std::max(1, N / M); }
    // the substitution-based panel kernels: their bits do not depend on the schedule the batch size selects, so H draws in one call
    // give the bits of H single calls
    static constexpr int PRECISE = 1;
    // a parameter vector that is not finite has no leading minor to blame: NMGP_NUM_NAN whatever pivot met the NaN first, as
    // had_eval_chunk reports it
    static constexpr bool NAN_PARS = true;
    // as had_batch_eval: the call leaves no evaluation behind that a fetch could refer to
    static constexpr bool RESETS_KIND = true;
    static int require(nmgp_ctx* c) {
        NMGP_TRY(require_had(c));
        if (c->M > 8) return nmgp_fail(c, NMGP_E_UNSUPPORTED, "unsupported number of outputs M=%d", c->M);
        return 0;
    }
    static int size_guard(const PsCall& k) {
        if (k.bs >= 0x7fffffffLL)
            return nmgp_fail(k.c, NMGP_E_SHAPE, "a matrix of order N = %d with %d riding rows exceeds the 2^31 elements the row kernels "
                             "index", k.N, k.ld - k.N);
        return 0;
    }
    // (counts the rows, riding ones included, against the leading dimension: the figure these entries have always chunked by)
    static size_t chunk_doubles(const PsCall& k) { return (size_t)(k.N + 1 + k.Emax) * k.ld; }
    static const double* y_rows(const PsCall& k, long long& stride) {
        stride = 0;                  // shared by the draws
        return k.c->had_y;
    }
};

template <class Model>
int ps_predict(nmgp_ctx* c, const double* pars, int H, const double* hyper, const double* xs, const int* indx_star, int S, int flags,
               const double* z, const double* star_in, double* mean, double* var, double* star_out, int* status) {
    if (!c) return NMGP_E_NULL;
    const int N = c->N, M = c->M, T = c->T, SW = Model::star_width(T);
    if (!pars || !xs || !mean || !var || (SW && !hyper)) return nmgp_fail(c, NMGP_E_NULL, "null argument");
    if (H <= 0 || S <= 0) return nmgp_fail(c, NMGP_E_SHAPE, "H and S must be positive (H=%d, S=%d)", H, S);
    if (z && star_in) return nmgp_fail(c, NMGP_E_STATE, "with star_in given the regression is skipped: z must be NULL");
    NMGP_TRY(Model::require(c));
    HIP_TRY(c, hipSetDevice(c->device));
    const bool indexed = indx_star != nullptr;
    if (indexed)
        for (int i = 0; i < S; ++i)
            if (indx_star[i] < 0 || indx_star[i] >= M)
                return nmgp_fail(c, NMGP_E_SHAPE, "indx_star[%d] = %d is not an output label in [0, %d)", i, indx_star[i], M);
    hipStream_t s = c->stream;
    PsCall k{};
    k.c = c, k.hyper = hyper, k.flags = flags, k.N = N, k.M = M, k.T = T, k.S = S, k.indexed = indexed;
    k.P = (long long)Model::P(N, T);
    k.n = Model::order(N, M), k.mats = Model::mats(M), k.per = Model::rows(M, indexed);
    const long long P = k.P;
    const int n = k.n, mats = k.mats, per = k.per;
    // new inputs per factorisation, and the riding rows that makes
    const int smax = Model::smax(N, M, indexed);
    k.Emax = std::min(S, smax) * per;
    const int ld = k.ld = (int)nmgp_ld((size_t)n + 1 + k.Emax);
    const long long bs = k.bs = (long long)ld * n;
    NMGP_TRY(Model::size_guard(k));
    const int chunks = (n + 127) / 128;
    const int B = nmgp_ps_chunk(H, Model::chunk_doubles(k));
    const size_t SC = (size_t)S * SW, O = (size_t)S * (indexed ? 1 : M), Bs = B;

    const bool regress = SW && !star_in;
    PriorFactor *p0 = nullptr, *p1 = nullptr;
    if (regress) NMGP_TRY(had_priors(c, hyper, &p0, &p1));
    const bool same = p0 == p1;
    // one workspace, carved; its size depends on (N, M, S, B), not on H
    size_t off = 0;
    auto take = [&off](size_t nelem) {
        const size_t o = off;
        off += (nelem + 15) / 16 * 16;
        return o;
    };
    const size_t o_xs = take(S), o_is = take(indexed ? ((size_t)S + 1) / 2 : 0), o_W0 = take(regress ? (size_t)N * S : 0),
                 o_W1 = take(regress && !same ? (size_t)N * S : 0), o_cv = take(regress ? 2 * (size_t)S : 0), o_pars = take(Bs * P);
    Model::extras(k, take, Bs);
    // with several matrices per draw the rows reduce into dots / sqs [B, mats, S], which Model::finish combines into the mean;
    // with one they reduce into mean / sqs [B, O] themselves
    const size_t o_star = take(Bs * SC), o_z = take(z ? Bs * SC : 0), o_mean = take(Bs * O), o_dots = mats > 1 ? take(Bs * O) : o_mean,
                 o_sqs = take(Bs * O), o_var = take(Bs * O), o_part = take(Bs * mats * 2 * k.Emax * chunks),
                 o_info = take((Bs * mats + 1) / 2), o_S = take(Bs * mats * bs);
    if (c->ps_cap < off) {
        c->ps_cap = 0;
        NMGP_TRY(nmgp_dev_alloc(c, &c->ps_buf, off));
        c->ps_cap = off;
    } else if (nmgp_poison()) {
        HIP_TRY(c, hipMemsetAsync(c->ps_buf, 0xFF, off * sizeof(double), s));
    }
    double* w = k.w = c->ps_buf;
    k.xs = w + o_xs, k.W0 = w + o_W0, k.W1 = same ? k.W0 : w + o_W1, k.cv0 = w + o_cv, k.cv1 = same ? k.cv0 : k.cv0 + S;
    k.pars = w + o_pars, k.star = SW ? w + o_star : nullptr, k.z = z ? w + o_z : nullptr, k.mean = w + o_mean, k.dots = w + o_dots;
    k.sqs = w + o_sqs, k.var = w + o_var, k.Sb = w + o_S;
    double* part = w + o_part;
    int* d_is = indexed ? reinterpret_cast<int*>(w + o_is) : nullptr;
    int* d_info = reinterpret_cast<int*>(w + o_info);
    k.is = d_is;

    HIP_TRY(c, hipMemcpyAsync(k.xs, xs, (size_t)S * sizeof(double), hipMemcpyHostToDevice, s));
    if (indexed) HIP_TRY(c, hipMemcpyAsync(d_is, indx_star, (size_t)S * sizeof(int), hipMemcpyHostToDevice, s));
    if (regress) {   // once per call per distinct prior factor, not per draw
        NmgpStage sp(c, NMGP_STAGE_PRIOR);
        NMGP_TRY(nmgp_ps_project(c, p0, k.xs, S, k.W0, k.cv0));
        if (!same) NMGP_TRY(nmgp_ps_project(c, p1, k.xs, S, k.W1, k.cv1));
    }
    long long ystride = 0;
    const double* y = Model::y_rows(k, ystride);
    std::vector<int> hinfo(Bs * mats);
    for (int h0 = 0; h0 < H; h0 += B) {
        const int Bc = k.Bc = std::min(B, H - h0), BM = Bc * mats;
        k.hpars = pars + (size_t)h0 * P;
        Model::host_prep(k);         // before the upload: the first chunk's then runs while the device still projects the priors
        HIP_TRY(c, hipMemcpyAsync(k.pars, k.hpars, (size_t)Bc * P * sizeof(double), hipMemcpyHostToDevice, s));
        NMGP_TRY(Model::prep(k));
        if (regress) {
            if (z) HIP_TRY(c, hipMemcpyAsync(k.z, z + (size_t)h0 * SC, Bc * SC * sizeof(double), hipMemcpyHostToDevice, s));
            NmgpStage sp(c, NMGP_STAGE_PRIOR);
            NMGP_TRY(Model::star(k));
        } else if (SW) {
            HIP_TRY(c, hipMemcpyAsync(k.star, star_in + (size_t)h0 * SC, Bc * SC * sizeof(double), hipMemcpyHostToDevice, s));
        }
        HIP_TRY(c, hipMemsetAsync(d_info, 0, (size_t)BM * sizeof(int), s));
        for (int s0 = 0; s0 < S; s0 += smax) {
            k.s0 = s0, k.Sc = std::min(smax, S - s0), k.E = k.Sc * per;
            {
                NmgpStage sp(c, NMGP_STAGE_COV);
                int r = Model::build_cov(k);
                if (r) return nmgp_fail(c, r, "unsupported number of outputs M=%d", M);
                nmgpk::set_row(s, k.Sb, ld, n, y, n, BM, bs, ystride);      // y rides along as row n
                NMGP_TRY(Model::cross_rows(k));                             // ... and the slice's E cross-covariance rows below it
            }
            {
                NmgpStage sp(c, NMGP_STAGE_CHOL);
                nmgp_potrf(c, k.Sb, ld, n, 1 + k.E, 0, d_info, BM, bs, 1, Model::PRECISE);
            }
            NmgpStage sp(c, NMGP_STAGE_REDUCE);
            nmgpk::ps_rows_reduce(s, k.Sb, ld, bs, n, n + 1, n, k.E, part, BM, k.dots, k.sqs, (long long)(O / mats), (long long)s0 * per);
        }
        NMGP_TRY(Model::finish(k));
        double* hm = mean + (size_t)h0 * O;
        double* hv = var + (size_t)h0 * O;
        HIP_TRY(c, hipMemcpyAsync(hm, k.mean, Bc * O * sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(hv, k.var, Bc * O * sizeof(double), hipMemcpyDeviceToHost, s));
        if (star_out && SW)
            HIP_TRY(c, hipMemcpyAsync(star_out + (size_t)h0 * SC, k.star, Bc * SC * sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(hinfo.data(), d_info, (size_t)BM * sizeof(int), hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));          // the one synchronisation of the chunk
        NMGP_TRY(nmgp_take_launch_error(c));
        // per-draw status as the batched evaluations report it: the first non-zero of the draw's status words; a failing draw yields
        // NaN rows, not a failed call
        for (int b = 0; b < Bc; ++b) {
            int st = 0;
            for (int p = 0; p < mats && st == 0; ++p) st = hinfo[(size_t)b * mats + p];
            const double* pb = k.hpars + (size_t)b * P;
            if (Model::NAN_PARS && !std::all_of(pb, pb + P, [](double v) { return std::isfinite(v); })) st = NMGP_NUM_NAN;
            double *m0 = hm + b * O, *v0 = hv + b * O;
            for (size_t i = 0; i < O && st == 0; ++i)
                if (!std::isfinite(m0[i]) || !std::isfinite(v0[i])) st = NMGP_NUM_NAN;
            if (st != 0)
                for (size_t i = 0; i < O; ++i) m0[i] = v0[i] = std::nan("");
            if (status) status[h0 + b] = st;
        }
    }
    if (Model::RESETS_KIND) c->last_kind = 0;
    return 0;
}
