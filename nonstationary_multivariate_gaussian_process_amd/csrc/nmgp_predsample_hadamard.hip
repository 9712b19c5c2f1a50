// Posterior-draw prediction of the separable Hadamard model (prediction.py:461-707: point_ / pointwise_ / indexedpoint_ /
// test_predsample_hadamard): H parameter vectors of the resident Hadamard subject, S new inputs.  Entry declared in include/nmgp.h.
//
// The covariance S_h = K_x o (R R^T) + sigma2 I depends on the draw only (the reference rebuilds and eigendecomposes it per draw AND
// per grid point), so a chunk of B draws is ONE batched blocked Cholesky of B matrices of order N with y and the slice's E
// cross-covariance rows riding below each: nmgp_predict_hads with the draw as a grid dimension.  A riding row is built from the
// draw's OWN sampled (tilde_l*, tilde_sigma*):
//   k_f[i, e] = s_i s*_s g(i, s) B_f[m, c_i],   B_f[m, c_i] = <row m of L_h, r_{h,i}>,
//   mean = (L^-1 k_f)^T (L^-1 y),   var = B_f[m, m] (s*_s^2 + 1e-6) - |L^-1 k_f|^2 + sigma2_err.
// Full form: e = (s - s0) M + m over all outputs m; indexed form (indx_star): e = s - s0, m = indx_star[s].
// The starred values are k_pss_star's (the regressions of the unconstrained curves under the two priors + sqrt(cv) z), the
// covariance build nmgp_hadamard_sep.hip's.  Every kernel is per-draw independent with a fixed summation order: a batch of B draws
// gives the bits of B single calls.
#include <algorithm>

#include "nmgp_internal.h"

using namespace nmgpk;

namespace {

inline unsigned cdiv(long long a, long long b) { return (unsigned)((a + b - 1) / b); }

// Riding row R0 + e below the matrix of draw h = blockIdx.z, observation i = blockIdx.x; lanes along the riding-row index
// (contiguous in a column).  k_hads_crosscov_rows' expressions in their order, with the draw's own starred values.
//   istar == nullptr: e = (s - s0) M + m;  else e = s - s0, m = istar[s]
template <int M>
__global__ __launch_bounds__(256) void k_psh_cross_rows(const double* __restrict__ x, const double* __restrict__ ell,
                                                         const double* __restrict__ sig, const double* __restrict__ Rv,
                                                         const double* __restrict__ pars, long long P, int N,
                                                         const double* __restrict__ xs, const double* __restrict__ star,
                                                         const int* __restrict__ istar, int S, int s0, int E,
                                                         double* __restrict__ A, int ld, long long bstride, int R0) {
    const int e = blockIdx.y * 256 + threadIdx.x;
    const int i = blockIdx.x, h = blockIdx.z;
    if (e >= E) return;
    const int s = istar ? s0 + e : s0 + e / M;
    const int mp = istar ? istar[s] : e % M;
    const double* st = star + ((size_t)h * S + s) * 2;
    const double* Lvec = pars + (size_t)h * P + (size_t)2 * N;
    const double* ri = Rv + ((size_t)h * N + i) * M;
    const double xi = x[i], li = ell[(size_t)h * N + i];
    const double xj = xs[s], lj = exp(st[0]), sj = exp(st[1]);
    const double dist = (xi * xi + xj * xj) - 2.0 * (xi * xj);
    const double Aij = li * li + lj * lj;
    const double kv = (sig[(size_t)h * N + i] * sj) * sqrt(2.0 * (li * lj) / Aij) * exp(-dist / Aij);
    double b = 0.0;
    for (int r = 0; r <= mp; ++r) b += ri[r] * Lvec[mp * (mp + 1) / 2 + r];
    A[(size_t)h * bstride + (size_t)i * ld + R0 + e] = kv * b;
}

// k_hads_predvar with the draw as blockIdx.y: O = S M outputs per draw (k = s M + m), or O = S in the indexed form (k = s,
// m = istar[s]).  A value <= 0 is replaced by settings.precision (prediction.py:535-545, :659-669).
__global__ void k_psh_predvar(const double* __restrict__ star, const double* __restrict__ pars, long long P, int N,
                              const double* __restrict__ colsq, const int* __restrict__ istar, int S, int M,
                              double* __restrict__ var) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x, h = blockIdx.y;
    const int O = istar ? S : S * M;
    if (k >= O) return;
    const int s = istar ? k : k / M;
    const int mp = istar ? istar[s] : k % M;
    const double* Lvec = pars + (size_t)h * P + (size_t)2 * N;
    double b = 0.0;
    for (int r = 0; r <= mp; ++r) {
        const double v = Lvec[mp * (mp + 1) / 2 + r];
        b += v * v;
    }
    const double ss = exp(star[((size_t)h * S + s) * 2 + 1]);
    const double kss = NMGP_JITTER + ss * ss;
    double v = (b * kss - colsq[(size_t)h * O + k]) + exp(pars[(size_t)h * P + (P - 1)]);
    if (v <= 0.0) v = NMGP_PRECISION;
    var[(size_t)h * O + k] = v;
}

int psh_cross_rows(hipStream_t s, const double* x, const double* ell, const double* sig, const double* Rv, const double* pars,
                   long long P, int N, int M, const double* xs, const double* star, const int* istar, int S, int s0, int E,
                   double* A, int ld, long long bstride, int R0, int B) {
    const dim3 grid(N, cdiv(E, 256), B);
    NMGP_HADS_SWITCH(M, NMGP_LAUNCH((k_psh_cross_rows<MM>), grid, dim3(256), 0, s, x, ell, sig, Rv, pars, P, N, xs, star, istar, S,
                                    s0, E, A, ld, bstride, R0));
    return 0;
}

}  // namespace

extern "C" int nmgp_predsample_hads(nmgp_ctx* c, const double* pars, int H, const double hyper[9], const double* xs,
                                    const int* indx_star, int S, const double* z, const double* star_in, double* mean, double* var,
                                    double* star_out, int* status) {
    if (!c) return NMGP_E_NULL;
    if (!pars || !hyper || !xs || !mean || !var) return nmgp_fail(c, NMGP_E_NULL, "null argument");
    if (H <= 0 || S <= 0) return nmgp_fail(c, NMGP_E_SHAPE, "H and S must be positive (H=%d, S=%d)", H, S);
    if (z && star_in) return nmgp_fail(c, NMGP_E_STATE, "with star_in given the regression is skipped: z must be NULL");
    NMGP_TRY(require_had(c));
    HIP_TRY(c, hipSetDevice(c->device));
    const int N = c->N, M = c->M, T = c->T;
    if (M > 8) return nmgp_fail(c, NMGP_E_UNSUPPORTED, "unsupported number of outputs M=%d", M);
    const bool indexed = indx_star != nullptr;
    if (indexed)
        for (int k = 0; k < S; ++k)
            if (indx_star[k] < 0 || indx_star[k] >= M)
                return nmgp_fail(c, NMGP_E_SHAPE, "indx_star[%d] = %d is not an output label in [0, %d)", k, indx_star[k], M);
    const long long P = 2LL * N + T + 1;
    hipStream_t s = c->stream;
    // grid points per factorisation: at most N riding cross-covariance rows (nmgp_predict_hads' slices in the full form)
    const int smax = indexed ? N : std::max(1, N / M), Sm = std::min(S, smax);
    const int per = indexed ? 1 : M, Emax = Sm * per;
    const int ld = (int)nmgp_ld((size_t)N + 1 + Emax);
    const long long bs = (long long)ld * N;
    if (bs >= 0x7fffffffLL)
        return nmgp_fail(c, NMGP_E_SHAPE, "a matrix of order N = %d with %d riding rows exceeds the 2^31 elements the row kernels index",
                         N, ld - N);
    const int chunks = (N + 127) / 128;
    const int B = nmgp_ps_chunk(H, (size_t)(N + 1 + Emax) * ld);
    const size_t S2 = (size_t)S * 2, O = (size_t)S * per;

    const bool regress = star_in == nullptr;
    PriorFactor *pl = nullptr, *pg = nullptr;
    if (regress) NMGP_TRY(had_priors(c, hyper, &pl, &pg));
    const bool same = pl == pg;
    // one workspace, carved; its size depends on (N, M, S, B), not on H
    size_t off = 0;
    auto take = [&off](size_t nelem) {
        const size_t o = off;
        off += (nelem + 15) / 16 * 16;
        return o;
    };
    const size_t o_xs = take(S), o_is = take(indexed ? ((size_t)S + 1) / 2 : 0), o_W0 = take(regress ? (size_t)N * S : 0),
                 o_W1 = take(regress && !same ? (size_t)N * S : 0), o_cv = take(regress ? S2 : 0), o_pars = take((size_t)B * P),
                 o_ell = take((size_t)B * N), o_sig = take((size_t)B * N), o_Rv = take((size_t)B * N * M), o_star = take(B * S2),
                 o_z = take(z ? B * S2 : 0), o_mean = take(B * O), o_colsq = take(B * O), o_var = take(B * O),
                 o_part = take((size_t)B * 2 * Emax * chunks), o_info = take(((size_t)B + 1) / 2), o_S = take((size_t)B * bs);
    if (c->ps_cap < off) {
        c->ps_cap = 0;
        NMGP_TRY(nmgp_dev_alloc(c, &c->ps_buf, off));
        c->ps_cap = off;
    } else if (nmgp_poison()) {
        HIP_TRY(c, hipMemsetAsync(c->ps_buf, 0xFF, off * sizeof(double), s));
    }
    double* w = c->ps_buf;
    double *d_xs = w + o_xs, *W0 = w + o_W0, *W1 = same ? W0 : w + o_W1, *cv0 = w + o_cv, *cv1 = same ? cv0 : cv0 + S,
           *d_pars = w + o_pars, *d_ell = w + o_ell, *d_sig = w + o_sig, *d_Rv = w + o_Rv, *d_star = w + o_star,
           *d_z = z ? w + o_z : nullptr, *d_mean = w + o_mean, *d_colsq = w + o_colsq, *d_var = w + o_var, *part = w + o_part,
           *Sb = w + o_S;
    int* d_is = indexed ? reinterpret_cast<int*>(w + o_is) : nullptr;
    int* d_info = reinterpret_cast<int*>(w + o_info);

    HIP_TRY(c, hipMemcpyAsync(d_xs, xs, (size_t)S * sizeof(double), hipMemcpyHostToDevice, s));
    if (indexed) HIP_TRY(c, hipMemcpyAsync(d_is, indx_star, (size_t)S * sizeof(int), hipMemcpyHostToDevice, s));
    if (regress) {
        NMGP_TRY(nmgp_ps_project(c, pl, d_xs, S, W0, cv0));
        if (!same) NMGP_TRY(nmgp_ps_project(c, pg, d_xs, S, W1, cv1));
    }
    std::vector<int> hinfo(B);
    for (int h0 = 0; h0 < H; h0 += B) {
        const int Bc = std::min(B, H - h0);
        HIP_TRY(c, hipMemcpyAsync(d_pars, pars + (size_t)h0 * P, (size_t)Bc * P * sizeof(double), hipMemcpyHostToDevice, s));
        nmgp_hads_prep(s, d_pars, c->had_indx, N, M, d_ell, d_sig, d_Rv, Bc);
        if (regress) {
            if (z) HIP_TRY(c, hipMemcpyAsync(d_z, z + (size_t)h0 * S2, Bc * S2 * sizeof(double), hipMemcpyHostToDevice, s));
            pss_star(s, W0, W1, cv0, cv1, d_pars, P, d_z, N, S, hyper[0], hyper[3], d_star, Bc);
        } else {
            HIP_TRY(c, hipMemcpyAsync(d_star, star_in + (size_t)h0 * S2, Bc * S2 * sizeof(double), hipMemcpyHostToDevice, s));
        }
        HIP_TRY(c, hipMemsetAsync(d_info, 0, (size_t)Bc * sizeof(int), s));
        for (int s0 = 0; s0 < S; s0 += smax) {
            const int Sc = std::min(smax, S - s0), E = Sc * per;
            int r = nmgp_hads_cov_build(s, c->d_x, d_ell, d_sig, d_Rv, d_pars, P, Sb, ld, N, M, Bc, bs);
            if (r) return nmgp_fail(c, r, "unsupported number of outputs M=%d", M);
            set_row(s, Sb, ld, N, c->had_y, N, Bc, bs, 0);                // y rides along as row N (shared by the draws)
            NMGP_TRY(psh_cross_rows(s, c->d_x, d_ell, d_sig, d_Rv, d_pars, P, N, M, d_xs, d_star, d_is, S, s0, E, Sb, ld, bs, N + 1,
                                    Bc));
            nmgp_potrf(c, Sb, ld, N, 1 + E, 0, d_info, Bc, bs, 1, 1);
            ps_rows_reduce(s, Sb, ld, bs, N, N + 1, N, E, part, Bc, d_mean, d_colsq, (long long)O, (long long)s0 * per);
        }
        NMGP_LAUNCH(k_psh_predvar, dim3(cdiv((long long)O, 256), Bc), dim3(256), 0, s, d_star, d_pars, P, N, d_colsq, d_is, S, M,
                    d_var);
        double* hm = mean + (size_t)h0 * O;
        double* hv = var + (size_t)h0 * O;
        HIP_TRY(c, hipMemcpyAsync(hm, d_mean, Bc * O * sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(hv, d_var, Bc * O * sizeof(double), hipMemcpyDeviceToHost, s));
        if (star_out) HIP_TRY(c, hipMemcpyAsync(star_out + (size_t)h0 * S2, d_star, Bc * S2 * sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(hinfo.data(), d_info, (size_t)Bc * sizeof(int), hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        NMGP_TRY(nmgp_take_launch_error(c));
        // per-draw status as nmgp_hads_batch_eval reports it: a failing draw yields NaN rows, not a failed call; a parameter
        // vector that is not finite has no leading minor to blame
        for (int b = 0; b < Bc; ++b) {
            int st = hinfo[b];
            const double* pb = pars + (size_t)(h0 + b) * P;
            bool finite_in = true;
            for (long long k = 0; k < P && finite_in; ++k) finite_in = std::isfinite(pb[k]);
            if (!finite_in) st = NMGP_NUM_NAN;
            if (st == 0)
                for (size_t k = 0; k < O; ++k)
                    if (!std::isfinite(hm[b * O + k]) || !std::isfinite(hv[b * O + k])) {
                        st = NMGP_NUM_NAN;
                        break;
                    }
            if (st != 0)
                for (size_t k = 0; k < O; ++k) hm[b * O + k] = hv[b * O + k] = std::nan("");
            if (status) status[h0 + b] = st;
        }
    }
    c->last_kind = 0;
    return 0;
}
