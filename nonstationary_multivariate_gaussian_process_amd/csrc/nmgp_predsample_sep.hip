// Posterior-draw prediction of the separable and the stationary model (prediction.py:34-334 and :1640-1692): H parameter vectors
// of the resident subject, S new inputs, in batched launch sequences.  Entry points declared in include/nmgp.h.
//
// Per draw h: B = L L^T = V_B diag(wB) V_B^T (M x M, host Jacobi), Sigma = B kron K_x + sigma2 I =
// (V_B kron I) blockdiag_p(wB[p] K_x + sigma2 I) (V_B^T kron I).  A chunk of Bc draws is ONE batched block build and ONE batched
// blocked Cholesky over Bc M matrices of order N, with the rotated data row yt_p and the Sc cross-covariance rows k_s of the
// draw's own starred values riding below block p (rows become r L_p^-T), as chol_predict (nmgp_eig.hip) does for one vector:
//   dots[p, s] = (L_p^-1 k_s) . (L_p^-1 yt_p),  sqs[p, s] = |L_p^-1 k_s|^2,
//   mean[s, m] = sum_p wB[p] VB[m, p] dots[p, s],   var[s, m] = B[m, m] kss_s - sum_p (wB[p] VB[m, p])^2 sqs[p, s] + sigma2.
// Separable: the unconstrained tilde_l, tilde_sigma are regressed onto xs under their RBF priors (proj-first, once per call) and
// N(0, conditional variance) noise is added (k_pss_star); K_x is the Gibbs kernel + 1e-6 I (sep_prep_b / sep_blocks_b).
// Stationary: K_x = RBF_cov(x; alpha = sigma, beta = l) + 1e-6 I with the draw's scalars, no latent regression.
// Every kernel below is per-draw independent with a fixed summation order: a batch of B draws gives the bits of B single calls.
#include <algorithm>

#include "nmgp_predsample_common.h"

using namespace nmgpk;

namespace nmgpk {

// per-draw small block (device and host): wB [M] | VB row-major [M, M] | sigma2 | pad | diag(B) [M] | l0 | sig0
// (the first M + M M + 1 entries are the layout sep_prep_b / sep_blocks_b read; l0, sig0: the stationary draw's exp'd scalars)
__host__ __device__ inline int pss_small_per(int M) { return M + M * M + 2 + M + 2; }
__host__ __device__ inline int pss_o_s2(int M) { return M + M * M; }
__host__ __device__ inline int pss_o_bd(int M) { return M + M * M + 2; }
__host__ __device__ inline int pss_o_l0(int M) { return M + M * M + 2 + M; }

// Starred values of draw h = blockIdx.z at new input s = blockIdx.x, slot c = blockIdx.y (0: tilde_l*, 1: tilde_sigma*):
//   star = mu + proj_s . (curve - mu) + sqrt(cv_s) z          (prediction.py:56-61, :66-71; the curves are the UNCONSTRAINED ones)
// z == nullptr: no noise (the conditional mean).  star, z: [B, S, 2]; W0 / W1: [S, N]; cv0 / cv1: [S].
__global__ __launch_bounds__(256) void k_pss_star(const double* __restrict__ W0, const double* __restrict__ W1,
                                                   const double* __restrict__ cv0, const double* __restrict__ cv1,
                                                   const double* __restrict__ pars, long long P, const double* __restrict__ z, int N,
                                                   int S, double mu_l, double mu_s, double* __restrict__ star) {
    __shared__ double sh[256];
    const int s = blockIdx.x, cidx = blockIdx.y, h = blockIdx.z;
    const double* p = pars + (size_t)h * P + (size_t)cidx * N;
    const double* W = (cidx == 0 ? W0 : W1) + (size_t)s * N;
    const double mu = cidx == 0 ? mu_l : mu_s;
    double acc = 0.0;
    for (int i = threadIdx.x; i < N; i += 256) acc += W[i] * (p[i] - mu);
    acc = block_sum_256(acc, sh);
    if (threadIdx.x != 0) return;
    const size_t o = ((size_t)h * S + s) * 2 + cidx;
    double v = mu + acc;
    if (z) v = v + sqrt((cidx == 0 ? cv0 : cv1)[s]) * z[o];
    star[o] = v;
}

// Riding row R0 + e below EVERY one of the M blocks of draw h = blockIdx.z: the cross-covariance vector of grid point s0 + e, built
// once and written M times.  Lanes along the riding-row index (contiguous in the factor's column-major storage), i = blockIdx.x.
//   MODE 0 (separable, prediction.py:88 / :241): Gibbs with (sig_i, ell_i) of the draw against (exp(tilde_sigma*), exp(tilde_l*))
//   MODE 1 (stationary, :1656): RBF_cov(x, xs; alpha = sig0, beta = l0) with the draw's scalars
template <int MODE>
__global__ __launch_bounds__(256) void k_pss_cross_rows(const double* __restrict__ x, const double* __restrict__ ell,
                                                         const double* __restrict__ sig, const double* __restrict__ small, int N,
                                                         int M, const double* __restrict__ xs, const double* __restrict__ star,
                                                         int S, int s0, int Sc, double* __restrict__ A, int ld, long long bstride,
                                                         int R0) {
    const int e = blockIdx.y * 256 + threadIdx.x;
    const int i = blockIdx.x, h = blockIdx.z;
    if (e >= Sc) return;
    const int s = s0 + e;
    double v;
    if (MODE == 0) {
        const double* st = star + ((size_t)h * S + s) * 2;
        const double xi = x[i], li = ell[(size_t)h * N + i], xj = xs[s];
        const double lj = exp(st[0]), sj = exp(st[1]);
        const double dist = (xi * xi + xj * xj) - 2.0 * (xi * xj);
        const double Aij = li * li + lj * lj;
        v = (sig[(size_t)h * N + i] * sj) * sqrt(2.0 * (li * lj) / Aij) * exp(-dist / Aij);
    } else {
        const double* sm = small + (size_t)h * pss_small_per(M) + pss_o_l0(M);
        const double l0 = sm[0], sig0 = sm[1];
        const double xi = x[i] / l0, xj = xs[s] / l0;
        const double dist = (xi * xi + xj * xj) - 2.0 * (xi * xj);
        v = exp(-0.5 * dist) * (sig0 * sig0);
    }
    double* Ah = A + (size_t)h * M * bstride + (size_t)i * ld + R0 + e;
    for (int p = 0; p < M; ++p) Ah[(size_t)p * bstride] = v;
}

// Stationary draw h = blockIdx.z: lower triangles of its M blocks wB[p] (RBF_cov(x; sig0, l0) + 1e-6 I) + sigma2 I, column
// j = blockIdx.y, lanes along i (rbf_cov_sym's expressions, then sep_blocks')
__global__ __launch_bounds__(256) void k_pss_sta_blocks(const double* __restrict__ x, const double* __restrict__ small, int N, int M,
                                                         double* __restrict__ S, int ld, long long bstride) {
    const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y, h = blockIdx.z;
    if (i >= N || i < j) return;
    const double* sm = small + (size_t)h * pss_small_per(M);
    const double l0 = sm[pss_o_l0(M)], sig0 = sm[pss_o_l0(M) + 1], sigma2 = sm[pss_o_s2(M)];
    const double xi = x[i] / l0, xj = x[j] / l0;
    const double dist = (xi * xi + xj * xj) - 2.0 * (xi * xj);
    double v = exp(-0.5 * dist) * (sig0 * sig0);
    if (i == j) v = NMGP_JITTER + v;
    double* o = S + (size_t)h * M * bstride + (size_t)j * ld + i;
    for (int p = 0; p < M; ++p) {
        double b = sm[p] * v;
        if (i == j) b += sigma2;
        o[(size_t)p * bstride] = b;
    }
}

// yt[(h M + p) N + i] = sum_m Y[i, m] VB_h[m, p] (k_sep_prep_b's rotation for a model without per-location parameters)
__global__ __launch_bounds__(256) void k_pss_rotate_y(const double* __restrict__ Y, const double* __restrict__ small, int N, int M,
                                                       double* __restrict__ yt) {
    const int i = blockIdx.x * 256 + threadIdx.x, h = blockIdx.y;
    if (i >= N) return;
    const double* VB = small + (size_t)h * pss_small_per(M) + M;
    for (int p = 0; p < M; ++p) {
        double s = 0.0;
        for (int m = 0; m < M; ++m) s += Y[(size_t)i * M + m] * VB[m * M + p];
        yt[((size_t)h * M + p) * N + i] = s;
    }
}

// k_sep_predict_chol with the draw as blockIdx.y: dots / sqs [B, M, S] -> mean / var [B, S, M].
//   kss (separable): exp(tilde_sigma*)^2, + 1e-6 with kss_jitter (prediction.py:98 against :251); (stationary) sig0^2 (:1659)
//   a variance <= 0 (strict: < 0, the stationary functions) is replaced by settings.precision
__global__ void k_pss_combine(const double* __restrict__ dots, const double* __restrict__ sqs, const double* __restrict__ small,
                              const double* __restrict__ star, int S, int M, int stationary, int kss_jitter,
                              double* __restrict__ mean, double* __restrict__ var) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x, h = blockIdx.y;
    if (k >= S * M) return;
    const int s = k / M, m = k - s * M;
    const double* sm = small + (size_t)h * pss_small_per(M);
    const double* wB = sm;
    const double* VB = sm + M;
    double mu = 0.0, vv = 0.0;
    for (int p = 0; p < M; ++p) {
        const double am = wB[p] * VB[m * M + p];
        mu += am * dots[((size_t)h * M + p) * S + s];
        vv += (am * am) * sqs[((size_t)h * M + p) * S + s];
    }
    double kss;
    if (stationary) {
        const double sig0 = sm[pss_o_l0(M) + 1];
        kss = sig0 * sig0;
    } else {
        const double sg = exp(star[((size_t)h * S + s) * 2 + 1]);
        kss = kss_jitter ? NMGP_JITTER + (sg * sg) : sg * sg;
    }
    double v = (sm[pss_o_bd(M) + m] * kss - vv) + sm[pss_o_s2(M)];
    if (stationary ? (v < 0.0) : (v <= 0.0)) v = NMGP_PRECISION;
    mean[(size_t)h * S * M + k] = mu;
    var[(size_t)h * S * M + k] = v;
}

void pss_star(hipStream_t s, const double* W0, const double* W1, const double* cv0, const double* cv1, const double* pars, long long P,
              const double* z, int N, int S, double mu_l, double mu_s, double* star, int B) {
    NMGP_LAUNCH(k_pss_star, dim3(S, 2, B), dim3(256), 0, s, W0, W1, cv0, cv1, pars, P, z, N, S, mu_l, mu_s, star);
}

}  // namespace nmgpk

namespace {

inline unsigned cdiv(long long a, long long b) { return (unsigned)((a + b - 1) / b); }

// hooks of the two Kronecker models into the shared schedule (nmgp_predsample_common.h): M matrices of order N per draw, one riding
// row per new input below every one of them.  stationary = the model without per-location parameters and without a latent
// regression; flags = kss_jitter (separable only)
template <bool stationary>
struct PsKron {
    static size_t P(int N, int T) { return stationary ? (size_t)T + 3 : 2 * (size_t)N + T + 1; }
    static int star_width(int) { return stationary ? 0 : 2; }
    static int order(int N, int) { return N; }
    static int mats(int M) { return M; }
    static int rows(int, bool) { return 1; }
    // up to N - 2 riding cross-covariance rows besides the data row (as chol_predict)
    static int smax(int N, int, bool) { return std::max(1, N - 2); }
    static constexpr int PRECISE = 1;                    // as chol_predict (nmgp_eig.hip) and why
    static constexpr bool NAN_PARS = false;              // a NaN parameter is reported as whatever the factorisations met
    // the call leaves batched evaluations and a begun trajectory alone
    static constexpr bool RESETS_KIND = false;
    static int require(nmgp_ctx* c) {
        if (!nmgp_complete_subject(c)) return nmgp_fail(c, NMGP_E_STATE, "nmgp_set_data must be called first");
        if (c->chol_algo != 1 || c->sep_algo != 1)
            return nmgp_fail(c, NMGP_E_UNSUPPORTED, "posterior-draw prediction runs on the custom factorisation of the M blocks only "
                                                    "(riding rows): not under NMGP_CHOL=rocsolver or NMGP_SEP=eig");
        return 0;
    }
    static int size_guard(const PsCall& k) {             // (sep_blocks_b addresses a block with 32-bit byte offsets)
        if (8LL * k.ld * k.N >= 0x7fffffffLL)
            return nmgp_fail(k.c, NMGP_E_SHAPE, "a block of order N = %d with %d riding rows exceeds the 2 GiB the block build addresses",
                             k.N, k.ld - k.N);
        return 0;
    }
    static size_t chunk_doubles(const PsCall& k) { return (size_t)k.M * k.bs; }
    static const double* y_rows(const PsCall& k, long long& stride) {
        stride = k.N;                // every block has its own rotated data row
        return k.at(k.o_yt);
    }
    template <class Take>
    static void extras(PsCall& k, Take take, size_t B) {
        k.o_small = take(B * pss_small_per(k.M));
        k.o_ell = take(stationary ? 0 : B * k.N);
        k.o_sig = take(stationary ? 0 : B * k.N);
        k.o_yt = take(B * k.M * k.N);
        k.host.resize(B * pss_small_per(k.M));
    }
    // host: B = L L^T and its eigenpairs per draw (M x M: known before the first launch)
    static void host_prep(PsCall& k) {
        const int N = k.N, M = k.M, sp = pss_small_per(M);
        for (int b = 0; b < k.Bc; ++b) {
            const double* pb = k.hpars + (size_t)b * k.P;
            double* hs = k.host.data() + (size_t)b * sp;
            nmgp_small_eig(pb + (stationary ? 2 : 2 * (size_t)N), M, hs, hs + M, hs + pss_o_bd(M));
            hs[pss_o_s2(M)] = std::exp(pb[k.P - 1]);
            hs[pss_o_s2(M) + 1] = 0.0;
            hs[pss_o_l0(M)] = stationary ? std::exp(pb[0]) : 1.0;
            hs[pss_o_l0(M) + 1] = stationary ? std::exp(pb[1]) : 1.0;
        }
    }
    static int prep(const PsCall& k) {
        nmgp_ctx* c = k.c;
        const int N = k.N, M = k.M, sp = pss_small_per(M);
        double* small = k.at(k.o_small);
        HIP_TRY(c, hipMemcpyAsync(small, k.host.data(), (size_t)k.Bc * sp * sizeof(double), hipMemcpyHostToDevice, c->stream));
        if (stationary)
            NMGP_LAUNCH(k_pss_rotate_y, dim3(cdiv(N, 256), k.Bc), dim3(256), 0, c->stream, c->d_Y, small, N, M, k.at(k.o_yt));
        else
            sep_prep_b(c->stream, k.pars, k.P, c->d_Y, small, sp, N, M, k.at(k.o_ell), k.at(k.o_sig), k.at(k.o_yt), k.Bc);
        return 0;
    }
    static int star(const PsCall& k) {
        pss_star(k.c->stream, k.W0, k.W1, k.cv0, k.cv1, k.pars, k.P, k.z, k.N, k.S, k.hyper[0], k.hyper[3], k.star, k.Bc);
        return 0;
    }
    static int build_cov(const PsCall& k) {
        nmgp_ctx* c = k.c;
        if (stationary)
            NMGP_LAUNCH(k_pss_sta_blocks, dim3(cdiv(k.N, 256), k.N, k.Bc), dim3(256), 0, c->stream, c->d_x, k.at(k.o_small), k.N, k.M,
                        k.Sb, k.ld, k.bs);
        else
            sep_blocks_b(c->stream, c->d_x, k.at(k.o_ell), k.at(k.o_sig), k.at(k.o_small), pss_small_per(k.M), k.N, k.M, k.Sb, k.ld,
                         k.bs, nullptr, k.Bc);
        return 0;
    }
    static int cross_rows(const PsCall& k) {
        nmgp_ctx* c = k.c;
        const dim3 gx(k.N, cdiv(k.Sc, 256), k.Bc);
        if (stationary)
            NMGP_LAUNCH((k_pss_cross_rows<1>), gx, dim3(256), 0, c->stream, c->d_x, nullptr, nullptr, k.at(k.o_small), k.N, k.M, k.xs,
                        nullptr, k.S, k.s0, k.Sc, k.Sb, k.ld, k.bs, k.N + 1);
        else
            NMGP_LAUNCH((k_pss_cross_rows<0>), gx, dim3(256), 0, c->stream, c->d_x, k.at(k.o_ell), k.at(k.o_sig), k.at(k.o_small), k.N,
                        k.M, k.xs, k.star, k.S, k.s0, k.Sc, k.Sb, k.ld, k.bs, k.N + 1);
        return 0;
    }
    static int finish(const PsCall& k) {                 // dots / sqs [B, M, S] -> mean / var [B, S, M]
        NMGP_LAUNCH(k_pss_combine, dim3(cdiv((long long)k.S * k.M, 256), k.Bc), dim3(256), 0, k.c->stream, k.dots, k.sqs,
                    k.at(k.o_small), k.star, k.S, k.M, stationary ? 1 : 0, k.flags ? 1 : 0, k.mean, k.var);
        return 0;
    }
};

}  // namespace

extern "C" int nmgp_predsample_sep(nmgp_ctx* c, const double* pars, int H, const double hyper[9], const double* xs, int S,
                                   int kss_jitter, const double* z, const double* star_in, double* mean, double* var,
                                   double* star_out, int* status) {
    return ps_predict<PsKron<false>>(c, pars, H, hyper, xs, nullptr, S, kss_jitter, z, star_in, mean, var, star_out, status);
}

extern "C" int nmgp_predsample_sta(nmgp_ctx* c, const double* pars, int H, const double* xs, int S, double* mean, double* var,
                                   int* status) {
    return ps_predict<PsKron<true>>(c, pars, H, nullptr, xs, nullptr, S, 0, nullptr, nullptr, mean, var, nullptr, status);
}
