// Posterior-draw prediction of the nonseparable model (prediction.py:1265-1398 and :1038-1262): H parameter vectors of the
// resident subject, S new inputs, in batched launch sequences.  Entry point declared in include/nmgp.h.
//
// Per draw h and new input s the reference regresses the latent curves onto xs_s (GP regression under the RBF priors), adds
// N(0, conditional variance) noise, and predicts y with the draw's covariance.  Here
//   * proj = Sigma_prior^-1 k*(xs) and the conditional variances depend on (x, xs, alpha, beta) only: once per call;
//   * the H (1 + T) regressions are dot products with proj: one kernel with the draw as a grid dimension, which also adds the
//     noise and applies the flavour's exp (k_ps_star);
//   * a chunk of B draws is ONE batched covariance build and ONE batched blocked Cholesky with y and the S M cross-covariance
//     rows of each draw's own starred values riding below each matrix (as nmgp_predict_svc does for one parameter vector).
// Every kernel below is per-draw independent with a fixed summation order: a batch of B draws gives the bits of B single calls.
#include <algorithm>

#include "nmgp_predsample_common.h"

using namespace nmgpk;

namespace nmgpk {

// Conditional variance of the GP regression at xs_s (prediction.py:1289, 1305): (alpha^2 + jitter) - proj_s . k_s, the
// `+ jitter` being RBF_cov(x*) called with X2 = None; a value < 0 is replaced by settings.precision.  W: [S, N] row-major
// (row s = Sigma^-1 k_s); k_s is rebuilt with RBF_cov's expressions.  One workgroup per new input.
__global__ __launch_bounds__(256) void k_ps_condvar(const double* __restrict__ W, const double* __restrict__ x, int N,
                                                     const double* __restrict__ xs, double alpha, double beta,
                                                     double* __restrict__ cv) {
    __shared__ double sh[256];
    const int s = blockIdx.x;
    const double b = xs[s] / beta;
    double acc = 0.0;
    for (int i = threadIdx.x; i < N; i += 256) {
        const double a = x[i] / beta;
        const double dist = (a * a + b * b) - 2.0 * (a * b);
        acc += W[(size_t)s * N + i] * (exp(-0.5 * dist) * (alpha * alpha));
    }
    acc = block_sum_256(acc, sh);
    if (threadIdx.x == 0) {
        double v = (NMGP_JITTER + alpha * alpha) - acc;
        if (v < 0.0) v = NMGP_PRECISION;
        cv[s] = v;
    }
}

// Starred values of draw h = blockIdx.z at new input s = blockIdx.x, slot c = blockIdx.y (0: tilde_l*, 1 + t: slot t of L*):
//   star = mu + proj_s . (curve - mu) + sqrt(cv_s) z
// constrained = 1 (prediction.py:1300-1308): the curve of slot t is the CONSTRAINED L_vecs (exp already applied on the diagonal
// slots, Lv) and the sampled value enters vec2lowtriangle as it is; constrained = 0 (:1128-1137): the curve is the unconstrained
// uL_vecs and exp is applied on the diagonal slots AFTER the noise.  z == nullptr: no noise (the conditional mean).
// star: [B, S, 1 + T]; W0 / W1: [S, N] projections under the tilde_l / L prior; cv: [2, S].
__global__ __launch_bounds__(256) void k_ps_star(const double* __restrict__ W0, const double* __restrict__ W1,
                                                  const double* __restrict__ cv, const double* __restrict__ pars,
                                                  const double* __restrict__ Lv, const double* __restrict__ z, int N, int M, int T,
                                                  int S, double mu_l, double mu_L, int constrained, double* __restrict__ star) {
    __shared__ double sh[256];
    const int s = blockIdx.x, cidx = blockIdx.y, h = blockIdx.z;
    const size_t P = (size_t)N * (1 + T) + 1;
    const double* p = pars + (size_t)h * P;
    const double* W = (cidx == 0 ? W0 : W1) + (size_t)s * N;
    const double mu = cidx == 0 ? mu_l : mu_L;
    double acc = 0.0;
    if (cidx == 0) {
        for (int i = threadIdx.x; i < N; i += 256) acc += W[i] * (p[i] - mu);
    } else {
        const int t = cidx - 1;
        const double* cur = constrained ? Lv + (size_t)h * N * T + t : p + N + t;
        for (int i = threadIdx.x; i < N; i += 256) acc += W[i] * (cur[(size_t)i * T] - mu);
    }
    acc = block_sum_256(acc, sh);
    if (threadIdx.x != 0) return;
    const size_t o = ((size_t)h * S + s) * (1 + T) + cidx;
    double v = mu + acc;
    if (z) v = v + sqrt(cv[(cidx == 0 ? 0 : S) + s]) * z[o];
    if (!constrained && cidx > 0) {
        // diagonal slots of the packed lower triangle: t = r (r + 1) / 2 + r
        const int t = cidx - 1;
        int r = 0;
        while ((r + 1) * (r + 2) / 2 <= t) ++r;
        if (t == r * (r + 1) / 2 + r) v = exp(v);
    }
    star[o] = v;
}

// k_svc_crosscov_rows with the draw as blockIdx.z: extra row R0 + e of draw h's factorisation buffer, e = (s - s0) M + m' for the
// grid points s0 .. s0 + Sc - 1 of a slice, from the draw's own ell, Lv and starred values.  Lanes along the extra-row index.
__global__ __launch_bounds__(256) void k_ps_crosscov_rows(const double* __restrict__ x, const double* __restrict__ ell,
                                                           const double* __restrict__ Lv, int N, int M, int T,
                                                           const double* __restrict__ xs, const double* __restrict__ star, int S,
                                                           int s0, int Sc, double* __restrict__ A, int ld, long long bstride,
                                                           int R0) {
    const int e = blockIdx.y * 256 + threadIdx.x;
    const int i = blockIdx.x, h = blockIdx.z;
    if (e >= Sc * M) return;
    ell += (size_t)h * N;
    Lv += (size_t)h * N * T;
    A += (size_t)h * bstride;
    const int s = s0 + e / M, mp = e % M;
    const double* st = star + ((size_t)h * S + s) * (1 + T);
    const double xi = x[i], li = ell[i];
    const double xj = xs[s], lj = exp(st[0]);
    const double dist = (xi * xi + xj * xj) - 2.0 * (xi * xj);
    const double Aij = li * li + lj * lj;
    const double kv = sqrt(2.0 * (li * lj) / Aij) * exp(-dist / Aij);
    for (int m = 0; m < M; ++m) {
        const int rmax = m < mp ? m : mp;
        double b = 0.0;
        for (int r = 0; r <= rmax; ++r) b += Lv[(size_t)i * T + m * (m + 1) / 2 + r] * st[1 + mp * (mp + 1) / 2 + r];
        A[(size_t)(m * N + i) * ld + R0 + e] = kv * b;
    }
}

// k_pred_rows_part / _sum with the draw as blockIdx.z: after the factorisation row R0 + e of draw h holds v_e = (L^-1 k_e)^T and
// row zrow z = L^-1 y; mean = v_e . z, colsq = |v_e|^2.  Columns in chunks of 128 per workgroup, partial sums in a fixed order:
// part[h][chunk][e][2]; outputs at draw stride ostride, offset o0 (the slice's first output).
__global__ __launch_bounds__(256) void k_ps_rows_part(const double* __restrict__ A, int ld, long long bstride, int n, int R0,
                                                       int zrow, int E, double* __restrict__ part) {
    __shared__ double red[2][4][64];
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int e = blockIdx.x * 64 + lane;
    const int c0 = blockIdx.y * 128 + g * 32;
    A += (size_t)blockIdx.z * bstride;
    part += (size_t)blockIdx.z * gridDim.y * E * 2;
    double am = 0.0, aq = 0.0;
    if (e < E) {
        for (int k = 0; k < 32; ++k) {
            const int c = c0 + k;
            if (c < n) {
                const double v = A[(size_t)c * ld + R0 + e];
                am = fma(v, A[(size_t)c * ld + zrow], am);
                aq = fma(v, v, aq);
            }
        }
    }
    red[0][g][lane] = am;
    red[1][g][lane] = aq;
    __syncthreads();
    if (g == 0 && e < E) {
        double* o = part + ((size_t)blockIdx.y * E + e) * 2;
        o[0] = (red[0][0][lane] + red[0][1][lane]) + (red[0][2][lane] + red[0][3][lane]);
        o[1] = (red[1][0][lane] + red[1][1][lane]) + (red[1][2][lane] + red[1][3][lane]);
    }
}
__global__ __launch_bounds__(256) void k_ps_rows_sum(const double* __restrict__ part, int chunks, int E, double* __restrict__ mean,
                                                      double* __restrict__ colsq, long long ostride, long long o0) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    part += (size_t)blockIdx.y * chunks * E * 2;
    double am = 0.0, aq = 0.0;
    for (int ch = 0; ch < chunks; ++ch) {
        am += part[((size_t)ch * E + e) * 2];
        aq += part[((size_t)ch * E + e) * 2 + 1];
    }
    mean[(size_t)blockIdx.y * ostride + o0 + e] = am;
    colsq[(size_t)blockIdx.y * ostride + o0 + e] = aq;
}

// k_svc_predvar with the draw as blockIdx.y: var = (1 + jitter) diag(L* L*^T) - colsq + sigma2 of the draw, a value <= 0 replaced
// by settings.precision (prediction.py:1339-1345)
__global__ void k_ps_predvar(const double* __restrict__ star, const double* __restrict__ colsq, int S, int M, int T,
                             const double* __restrict__ pars, long long P, double* __restrict__ var) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const int h = blockIdx.y;
    if (k >= S * M) return;
    const int s = k / M, mp = k % M;
    const double* st = star + ((size_t)h * S + s) * (1 + T) + 1;
    double b = 0.0;
    for (int r = 0; r <= mp; ++r) {
        const double v = st[mp * (mp + 1) / 2 + r];
        b += v * v;
    }
    const double kss = NMGP_JITTER + 1.0;
    double v = (kss * b - colsq[(size_t)h * S * M + k]) + exp(pars[(size_t)h * P + (P - 1)]);
    if (v <= 0.0) v = NMGP_PRECISION;
    var[(size_t)h * S * M + k] = v;
}

// the two kernels above for `batch` matrices in one launch each (the separable / stationary entries pass draw x block)
void ps_rows_reduce(hipStream_t s, const double* A, int ld, long long bstride, int n, int R0, int zrow, int E, double* part,
                    int batch, double* dots, double* sqs, long long ostride, long long o0) {
    const int chunks = (n + 127) / 128;
    NMGP_LAUNCH(k_ps_rows_part, dim3((E + 63) / 64, chunks, batch), dim3(256), 0, s, A, ld, bstride, n, R0, zrow, E, part);
    NMGP_LAUNCH(k_ps_rows_sum, dim3((E + 255) / 256, batch), dim3(256), 0, s, part, chunks, E, dots, sqs, ostride, o0);
}

}  // namespace nmgpk

namespace {

inline unsigned cdiv(long long a, long long b) { return (unsigned)((a + b - 1) / b); }

// W = Sigma_prior^-1 K*: rows of W ([S, N] row-major == column-major [N, S]) are the solutions; the reference's order (solve for
// k* first, then the dot products with the curves) and the substitution solve of the deterministic predictor (see gp_project in
// nmgp_eig.hip for why both matter on a factor of condition number ~1e5.5)
int project_rows(nmgp_ctx* c, PriorFactor* pf, const double* d_xs, int S, double* W) {
    const int N = c->N;
    hipStream_t s = c->stream;
    const double one = 1.0;
    rbf_cov_rect(s, d_xs, S, c->d_x, N, 1, pf->alpha, pf->beta, false, W);
    if (N <= 15000 && !c->prior_rocblas) {
        prior_trsv(s, false, pf->L, pf->ld, 0, pf->L, pf->ld, 0, W, N, S, 1);
        prior_trsv(s, true, pf->L, pf->ld, 0, pf->L, pf->ld, 0, W, N, S, 1);
    } else {
        BLAS_TRY(c, rocblas_dtrsm(c->blas, rocblas_side_left, rocblas_fill_lower, rocblas_operation_none,
                                  rocblas_diagonal_non_unit, N, S, &one, pf->L, pf->ld, W, N));
        BLAS_TRY(c, rocblas_dtrsm(c->blas, rocblas_side_left, rocblas_fill_lower, rocblas_operation_transpose,
                                  rocblas_diagonal_non_unit, N, S, &one, pf->L, pf->ld, W, N));
    }
    return 0;
}

int env_int(const char* name, int dflt) {
    const char* e = std::getenv(name);
    return (e && *e) ? std::atoi(e) : dflt;
}

}  // namespace

// W = Sigma_prior^-1 K*(xs) ([S, N] row-major) and the clipped conditional variances cv [S] of one GP prior
int nmgp_ps_project(nmgp_ctx* c, PriorFactor* pf, const double* d_xs, int S, double* W, double* cv) {
    NMGP_TRY(project_rows(c, pf, d_xs, S, W));
    NMGP_LAUNCH(k_ps_condvar, dim3(S), dim3(256), 0, c->stream, W, c->d_x, c->N, d_xs, pf->alpha, pf->beta, cv);
    return 0;
}

// Draws per chunk: as many as keep the factorisation buffers (8 ld n bytes per draw, ld = n + 1 + riding rows) below
// NMGP_PREDSAMPLE_SLAB_GB (default 16) and at most 64; NMGP_PREDSAMPLE_CHUNK overrides.  At N = 2048, D = 3 with the 201-point
// grid a draw takes 0.33 GB: 51 draws per chunk, well inside the throughput schedule of the blocked Cholesky (from 13 on).
int nmgp_ps_chunk(int H, size_t per_draw_doubles) {
    int B = env_int("NMGP_PREDSAMPLE_CHUNK", 0);
    if (B <= 0) {
        const double slab = std::max(1, env_int("NMGP_PREDSAMPLE_SLAB_GB", 16)) * 1073741824.0;
        B = (int)std::min(64.0, slab / (8.0 * (double)per_draw_doubles));
    }
    return std::max(1, std::min(B, std::min(H, 65535)));
}

namespace {

// hooks of the nonseparable model into the shared schedule (nmgp_predsample_common.h); one matrix of order n = N M per draw, M riding
// rows per new input; flags = constrained
struct PsSvc {
    static size_t P(int N, int T) { return (size_t)N * (1 + T) + 1; }
    static int star_width(int T) { return 1 + T; }
    static int order(int N, int M) { return N * M; }
    static int mats(int) { return 1; }
    static int rows(int M, bool) { return M; }
    static int smax(int N, int, bool) { return N; }      // up to n riding cross-covariance rows (x_test = x is one slice)
    // the panel kernels of the evaluations: what this entry has run since it exists and what its golden files were checked against
    static constexpr int PRECISE = 0;
    static constexpr bool NAN_PARS = false;              // a NaN parameter is reported as the pivot that met it
    // the call leaves batched evaluations and a begun trajectory alone
    static constexpr bool RESETS_KIND = false;
    static int require(nmgp_ctx* c) {
        if (!nmgp_complete_subject(c)) return nmgp_fail(c, NMGP_E_STATE, "nmgp_set_data must be called first");
        if (c->chol_algo != 1)
            return nmgp_fail(c, NMGP_E_UNSUPPORTED, "posterior-draw prediction runs on the custom factorisation only (riding rows)");
        return 0;
    }
    static int size_guard(const PsCall&) { return 0; }   // none: this entry has never had one
    static size_t chunk_doubles(const PsCall& k) { return (size_t)k.bs; }
    static const double* y_rows(const PsCall& k, long long& stride) {
        stride = 0;                  // shared by the draws
        return k.c->d_y;
    }
    template <class Take>
    static void extras(PsCall& k, Take take, size_t B) {
        k.o_ell = take(B * k.N);
        k.o_Lv = take(B * k.N * k.T);
    }
    static void host_prep(PsCall&) {}
    static int prep(const PsCall& k) {
        svc_prep(k.c->stream, k.pars, k.N, k.M, k.at(k.o_ell), k.at(k.o_Lv), k.Bc);
        return 0;
    }
    static int star(const PsCall& k) {
        hipStream_t s = k.c->stream;
        // k_ps_star takes ONE cv [2, S]; where the two prior factors coincide the schedule fills its first half only
        if (k.cv1 == k.cv0)
            NMGP_LAUNCH(k_ps_condvar, dim3(k.S), dim3(256), 0, s, k.W1, k.c->d_x, k.N, k.xs, k.hyper[4], k.hyper[5], k.cv0 + k.S);
        NMGP_LAUNCH(k_ps_star, dim3(k.S, 1 + k.T, k.Bc), dim3(256), 0, s, k.W0, k.W1, k.cv0, k.pars, k.at(k.o_Lv), k.z, k.N, k.M, k.T,
                    k.S, k.hyper[0], k.hyper[3], k.flags ? 1 : 0, k.star);
        return 0;
    }
    static int build_cov(const PsCall& k) {
        return svc_cov_build(k.c->stream, k.c->d_x, k.at(k.o_ell), k.at(k.o_Lv), k.pars + (k.P - 1), k.Sb, k.ld, k.N, k.M, false, k.Bc,
                             k.bs, 0, 1);
    }
    static int cross_rows(const PsCall& k) {
        NMGP_LAUNCH(k_ps_crosscov_rows, dim3(k.N, cdiv(k.E, 256), k.Bc), dim3(256), 0, k.c->stream, k.c->d_x, k.at(k.o_ell),
                    k.at(k.o_Lv), k.N, k.M, k.T, k.xs, k.star, k.S, k.s0, k.Sc, k.Sb, k.ld, k.bs, k.n + 1);
        return 0;
    }
    static int finish(const PsCall& k) {
        NMGP_LAUNCH(k_ps_predvar, dim3(cdiv((long long)k.S * k.M, 256), k.Bc), dim3(256), 0, k.c->stream, k.star, k.sqs, k.S, k.M, k.T,
                    k.pars, k.P, k.var);
        return 0;
    }
};

}  // namespace

extern "C" int nmgp_predsample_svc(nmgp_ctx* c, const double* pars, int H, const double hyper[8], const double* xs, int S,
                                   int constrained, const double* z, const double* star_in, double* mean, double* var,
                                   double* star_out, int* status) {
    return ps_predict<PsSvc>(c, pars, H, hyper, xs, nullptr, S, constrained, z, star_in, mean, var, star_out, status);
}
