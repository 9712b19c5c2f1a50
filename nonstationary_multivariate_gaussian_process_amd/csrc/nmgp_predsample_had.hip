// Posterior-draw and held-out prediction of the nonseparable Hadamard model: H parameter vectors of the resident Hadamard subject, S
// new inputs.  Entry declared in include/nmgp.h.  The reference has no posterior-draw form for this model and its indexed MAP
// predictor (prediction.py:1480-1561) reports the variance of output 0 whatever the label; this entry is nmgp_predsample_hads'
// schedule (nmgp_predsample_hadamard.hip) with this model's covariance, starred values and cross-covariance.
//
// The covariance S_h = K_x o (R_h R_h^T) + sigma2 I depends on the draw only, so a chunk of B draws is ONE batched blocked Cholesky
// of B matrices of order N with y and the slice's E cross-covariance rows riding below each: nmgp_predict_had with the draw as a
// grid dimension.  A riding row is built from the draw's OWN sampled starred values (tilde_l*, the T raw slots of L*):
//   k_f[i, e] = g(i, s) <r_{h,i}, row m of L*_{h,s}>,   r_{h,i} = row indx[i] of the draw's L_i,
//   mean = (L^-1 k_f)^T (L^-1 y),   var = (1 + 1e-6) (L* L*^T)_mm - |L^-1 k_f|^2 + sigma2_err.
// Full form: e = (s - s0) M + m over all outputs m; indexed form (indx_star): e = s - s0, m = indx_star[s].
// The covariance build is nmgp_hadamard_common.h's, the per-draw unpacking nmgp_hadamard.hip's (had_prep).  Every kernel is per-draw
// independent with a fixed summation order: a batch of B draws gives the bits of B single calls.
#include <algorithm>

#include "nmgp_hadamard_common.h"

using namespace nmgpk;

namespace {

inline unsigned cdiv(long long a, long long b) { return (unsigned)((a + b - 1) / b); }

// Starred values of draw h = blockIdx.z at new input s = blockIdx.x, slot cidx = blockIdx.y (0: tilde_l*, 1 + t: slot t of L*, taken
// as it is: no exp):  star = mu + proj_s . (curve - mu) + sqrt(cv_s) z  -- k_had_star's sum in its order, k_pss_star's noise.  One
// conditional variance per prior: cv1 serves all T slots.  z == nullptr: the conditional mean.  star, z: [B, S, 1 + T]; W0 / W1:
// [S, N]; cv0 / cv1: [S].
__global__ __launch_bounds__(256) void k_psn_star(const double* __restrict__ W0, const double* __restrict__ W1,
                                                   const double* __restrict__ cv0, const double* __restrict__ cv1,
                                                   const double* __restrict__ pars, long long P, const double* __restrict__ z, int N,
                                                   int T, int S, double mu_l, double mu_L, double* __restrict__ star) {
    __shared__ double sh[256];
    const int s = blockIdx.x, cidx = blockIdx.y, h = blockIdx.z;
    const double* p = pars + (size_t)h * P;
    const double* W = (cidx == 0 ? W0 : W1) + (size_t)s * N;
    const double mu = cidx == 0 ? mu_l : mu_L;
    const double* cur = cidx == 0 ? p : p + N + (cidx - 1);
    const size_t stride = cidx == 0 ? 1 : (size_t)T;
    double acc = 0.0;
    for (int i = threadIdx.x; i < N; i += 256) acc += W[i] * (cur[(size_t)i * stride] - mu);
    acc = block_sum_256(acc, sh);
    if (threadIdx.x != 0) return;
    const size_t o = ((size_t)h * S + s) * (1 + T) + cidx;
    double v = mu + acc;
    if (z) v = v + sqrt((cidx == 0 ? cv0 : cv1)[s]) * z[o];
    star[o] = v;
}

// Riding row R0 + e below the matrix of draw h = blockIdx.z, observation i = blockIdx.x; lanes along the riding-row index
// (contiguous in a column).  k_had_crosscov_rows' expressions in their order, with the draw's own starred values.
//   istar == nullptr: e = (s - s0) M + m;  else e = s - s0, m = istar[s]
template <int M>
__global__ __launch_bounds__(256) void k_psn_cross_rows(const double* __restrict__ x, const double* __restrict__ ell,
                                                         const double* __restrict__ Rv, int N, const double* __restrict__ xs,
                                                         const double* __restrict__ star, const int* __restrict__ istar, int S,
                                                         int s0, int E, double* __restrict__ A, int ld, long long bstride, int R0) {
    constexpr int T = M * (M + 1) / 2;
    const int e = blockIdx.y * 256 + threadIdx.x;
    const int i = blockIdx.x, h = blockIdx.z;
    if (e >= E) return;
    const int s = istar ? s0 + e : s0 + e / M;
    const int mp = istar ? istar[s] : e % M;
    const double* st = star + ((size_t)h * S + s) * (1 + T);
    const double* ri = Rv + ((size_t)h * N + i) * M;
    const double xi = x[i], li = ell[(size_t)h * N + i];
    const double xj = xs[s], lj = exp(st[0]);
    const double dist = (xi * xi + xj * xj) - 2.0 * (xi * xj);
    const double Aij = li * li + lj * lj;
    const double kv = sqrt(2.0 * (li * lj) / Aij) * exp(-dist / Aij);
    double b = 0.0;
    for (int r = 0; r <= mp; ++r) b += ri[r] * st[1 + mp * (mp + 1) / 2 + r];
    A[(size_t)h * bstride + (size_t)i * ld + R0 + e] = kv * b;
}

// k_had_predvar with the draw as blockIdx.y: O = S M outputs per draw (k = s M + m), or O = S in the indexed form (k = s,
// m = istar[s]).  A value <= 0 is replaced by settings.precision (prediction.py:1455-1461).
__global__ __launch_bounds__(256) void k_psn_predvar(const double* __restrict__ star, const double* __restrict__ pars, long long P,
                                                      const double* __restrict__ colsq, const int* __restrict__ istar, int S, int M,
                                                      int T, double* __restrict__ var) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x, h = blockIdx.y;
    const int O = istar ? S : S * M;
    if (k >= O) return;
    const int s = istar ? k : k / M;
    const int mp = istar ? istar[s] : k % M;
    const double* st = star + ((size_t)h * S + s) * (1 + T) + 1;
    double b = 0.0;
    for (int r = 0; r <= mp; ++r) {
        const double v = st[mp * (mp + 1) / 2 + r];
        b += v * v;
    }
    const double kss = NMGP_JITTER + 1.0;
    double v = (kss * b - colsq[(size_t)h * O + k]) + exp(pars[(size_t)h * P + (P - 1)]);
    if (v <= 0.0) v = NMGP_PRECISION;
    var[(size_t)h * O + k] = v;
}

int psn_cross_rows(hipStream_t s, const double* x, const double* ell, const double* Rv, int N, int M, const double* xs,
                   const double* star, const int* istar, int S, int s0, int E, double* A, int ld, long long bstride, int R0, int B) {
    const dim3 grid(N, cdiv(E, 256), B);
    NMGP_HADS_SWITCH(M, NMGP_LAUNCH((k_psn_cross_rows<MM>), grid, dim3(256), 0, s, x, ell, Rv, N, xs, star, istar, S, s0, E, A, ld,
                                    bstride, R0));
    return 0;
}

}  // namespace

extern "C" int nmgp_predsample_had(nmgp_ctx* c, const double* pars, int H, const double hyper[8], const double* xs,
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
    const long long P = (long long)N * (1 + T) + 1;
    hipStream_t s = c->stream;
    // grid points per factorisation: at most N riding cross-covariance rows (nmgp_predict_had's slices in the full form)
    const int smax = indexed ? N : std::max(1, N / M), Sm = std::min(S, smax);
    const int per = indexed ? 1 : M, Emax = Sm * per;
    const int ld = (int)nmgp_ld((size_t)N + 1 + Emax);
    const long long bs = (long long)ld * N;
    if (bs >= 0x7fffffffLL)
        return nmgp_fail(c, NMGP_E_SHAPE, "a matrix of order N = %d with %d riding rows exceeds the 2^31 elements the row kernels index",
                         N, ld - N);
    const int chunks = (N + 127) / 128;
    const int B = nmgp_ps_chunk(H, (size_t)(N + 1 + Emax) * ld);
    const size_t SW = (size_t)S * (1 + T), O = (size_t)S * per;

    const bool regress = star_in == nullptr;
    PriorFactor *pl = nullptr, *pL = nullptr;
    if (regress) NMGP_TRY(had_priors(c, hyper, &pl, &pL));
    const bool same = pl == pL;
    // one workspace, carved; its size depends on (N, M, S, B), not on H
    size_t off = 0;
    auto take = [&off](size_t nelem) {
        const size_t o = off;
        off += (nelem + 15) / 16 * 16;
        return o;
    };
    const size_t o_xs = take(S), o_is = take(indexed ? ((size_t)S + 1) / 2 : 0), o_W0 = take(regress ? (size_t)N * S : 0),
                 o_W1 = take(regress && !same ? (size_t)N * S : 0), o_cv = take(regress ? (size_t)2 * S : 0),
                 o_pars = take((size_t)B * P), o_ell = take((size_t)B * N), o_Rv = take((size_t)B * N * M), o_star = take(B * SW),
                 o_z = take(z ? B * SW : 0), o_mean = take(B * O), o_colsq = take(B * O), o_var = take(B * O),
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
           *d_pars = w + o_pars, *d_ell = w + o_ell, *d_Rv = w + o_Rv, *d_star = w + o_star, *d_z = z ? w + o_z : nullptr,
           *d_mean = w + o_mean, *d_colsq = w + o_colsq, *d_var = w + o_var, *part = w + o_part, *Sb = w + o_S;
    int* d_is = indexed ? reinterpret_cast<int*>(w + o_is) : nullptr;
    int* d_info = reinterpret_cast<int*>(w + o_info);

    HIP_TRY(c, hipMemcpyAsync(d_xs, xs, (size_t)S * sizeof(double), hipMemcpyHostToDevice, s));
    if (indexed) HIP_TRY(c, hipMemcpyAsync(d_is, indx_star, (size_t)S * sizeof(int), hipMemcpyHostToDevice, s));
    if (regress) {   // once per call per distinct prior factor, not per draw
        NmgpStage sp(c, NMGP_STAGE_PRIOR);
        NMGP_TRY(nmgp_ps_project(c, pl, d_xs, S, W0, cv0));
        if (!same) NMGP_TRY(nmgp_ps_project(c, pL, d_xs, S, W1, cv1));
    }
    std::vector<int> hinfo(B);
    for (int h0 = 0; h0 < H; h0 += B) {
        const int Bc = std::min(B, H - h0);
        HIP_TRY(c, hipMemcpyAsync(d_pars, pars + (size_t)h0 * P, (size_t)Bc * P * sizeof(double), hipMemcpyHostToDevice, s));
        had_prep(s, d_pars, c->had_indx, N, M, d_ell, d_Rv, Bc);
        if (regress) {
            if (z) HIP_TRY(c, hipMemcpyAsync(d_z, z + (size_t)h0 * SW, Bc * SW * sizeof(double), hipMemcpyHostToDevice, s));
            NmgpStage sp(c, NMGP_STAGE_PRIOR);
            NMGP_LAUNCH(k_psn_star, dim3(S, 1 + T, Bc), dim3(256), 0, s, W0, W1, cv0, cv1, d_pars, P, d_z, N, T, S, hyper[0], hyper[3],
                        d_star);
        } else {
            HIP_TRY(c, hipMemcpyAsync(d_star, star_in + (size_t)h0 * SW, Bc * SW * sizeof(double), hipMemcpyHostToDevice, s));
        }
        HIP_TRY(c, hipMemsetAsync(d_info, 0, (size_t)Bc * sizeof(int), s));
        for (int s0 = 0; s0 < S; s0 += smax) {
            const int Sc = std::min(smax, S - s0), E = Sc * per;
            {
                NmgpStage sp(c, NMGP_STAGE_COV);
                int r = gibbs_cov_build<false>(s, c->d_x, d_ell, nullptr, d_Rv, d_pars, P, Sb, ld, N, M, Bc, bs);
                if (r) return nmgp_fail(c, r, "unsupported number of outputs M=%d", M);
                set_row(s, Sb, ld, N, c->had_y, N, Bc, bs, 0);            // y rides along as row N (shared by the draws)
                NMGP_TRY(psn_cross_rows(s, c->d_x, d_ell, d_Rv, N, M, d_xs, d_star, d_is, S, s0, E, Sb, ld, bs, N + 1, Bc));
            }
            {
                NmgpStage sp(c, NMGP_STAGE_CHOL);
                nmgp_potrf(c, Sb, ld, N, 1 + E, 0, d_info, Bc, bs, 1, 1);
            }
            NmgpStage sp(c, NMGP_STAGE_REDUCE);
            ps_rows_reduce(s, Sb, ld, bs, N, N + 1, N, E, part, Bc, d_mean, d_colsq, (long long)O, (long long)s0 * per);
        }
        NMGP_LAUNCH(k_psn_predvar, dim3(cdiv((long long)O, 256), Bc), dim3(256), 0, s, d_star, d_pars, P, d_colsq, d_is, S, M, T,
                    d_var);
        double* hm = mean + (size_t)h0 * O;
        double* hv = var + (size_t)h0 * O;
        HIP_TRY(c, hipMemcpyAsync(hm, d_mean, Bc * O * sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(hv, d_var, Bc * O * sizeof(double), hipMemcpyDeviceToHost, s));
        if (star_out) HIP_TRY(c, hipMemcpyAsync(star_out + (size_t)h0 * SW, d_star, Bc * SW * sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(hinfo.data(), d_info, (size_t)Bc * sizeof(int), hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));          // the one synchronisation of the chunk
        NMGP_TRY(nmgp_take_launch_error(c));
        // per-draw status as nmgp_predsample_hads reports it: a failing draw yields NaN rows, not a failed call; a parameter vector
        // that is not finite has no leading minor to blame
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
