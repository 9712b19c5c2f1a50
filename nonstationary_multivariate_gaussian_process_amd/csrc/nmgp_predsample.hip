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

#include "nmgp_internal.h"

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

extern "C" int nmgp_predsample_svc(nmgp_ctx* c, const double* pars, int H, const double hyper[8], const double* xs, int S,
                                   int constrained, const double* z, const double* star_in, double* mean, double* var,
                                   double* star_out, int* status) {
    if (!c) return NMGP_E_NULL;
    if (!pars || !hyper || !xs || !mean || !var) return nmgp_fail(c, NMGP_E_NULL, "null argument");
    if (H <= 0 || S <= 0) return nmgp_fail(c, NMGP_E_SHAPE, "H and S must be positive (H=%d, S=%d)", H, S);
    if (z && star_in) return nmgp_fail(c, NMGP_E_STATE, "with star_in given the regression is skipped: z must be NULL");
    if (!nmgp_complete_subject(c)) return nmgp_fail(c, NMGP_E_STATE, "nmgp_set_data must be called first");
    if (c->chol_algo != 1)
        return nmgp_fail(c, NMGP_E_UNSUPPORTED, "posterior-draw prediction runs on the custom factorisation only (riding rows)");
    HIP_TRY(c, hipSetDevice(c->device));
    const int N = c->N, M = c->M, T = c->T, n = c->n;
    const long long P = c->P_svc;
    hipStream_t s = c->stream;
    const double mu_l = hyper[0], al_l = hyper[1], be_l = hyper[2], mu_L = hyper[3], al_L = hyper[4], be_L = hyper[5];
    // grid points per factorisation: up to n riding cross-covariance rows (x_test = x is one slice)
    const int smax = std::max(1, n / M), Sm = std::min(S, smax), Emax = Sm * M;
    const int ld = (int)nmgp_ld((size_t)n + 1 + Emax);
    const long long bs = (long long)ld * n;
    const int chunks = (n + 127) / 128;
    const int B = nmgp_ps_chunk(H, (size_t)bs);
    const size_t SC = (size_t)S * (1 + T), SMo = (size_t)S * M;

    // one workspace, carved; its size depends on (N, M, S, B), not on H
    const bool regress = star_in == nullptr;
    PriorFactor *pl = nullptr, *pL = nullptr;
    if (regress) {
        // (the factor cache is a vector: the second look-up may grow it and move its elements, so the first pointer is re-resolved)
        NMGP_TRY(nmgp_get_prior(c, al_l, be_l, &pl));
        NMGP_TRY(nmgp_get_prior(c, al_L, be_L, &pL));
        NMGP_TRY(nmgp_get_prior(c, al_l, be_l, &pl));
    }
    const bool same = pl == pL;
    size_t off = 0;
    auto take = [&off](size_t nelem) {
        const size_t o = off;
        off += (nelem + 15) / 16 * 16;
        return o;
    };
    const size_t o_xs = take(S), o_W0 = take(regress ? (size_t)N * S : 0), o_W1 = take(regress && !same ? (size_t)N * S : 0),
                 o_cv = take(2 * (size_t)S), o_pars = take((size_t)B * P), o_ell = take((size_t)B * N),
                 o_Lv = take((size_t)B * N * T), o_star = take(B * SC), o_z = take(z ? B * SC : 0), o_mean = take(B * SMo),
                 o_colsq = take(B * SMo), o_var = take(B * SMo), o_part = take((size_t)B * 2 * Emax * chunks),
                 o_info = take(((size_t)B + 1) / 2), o_S = take((size_t)B * bs);
    if (c->ps_cap < off) {
        c->ps_cap = 0;
        NMGP_TRY(nmgp_dev_alloc(c, &c->ps_buf, off));
        c->ps_cap = off;
    } else if (nmgp_poison()) {
        HIP_TRY(c, hipMemsetAsync(c->ps_buf, 0xFF, off * sizeof(double), s));
    }
    double* w = c->ps_buf;
    double *d_xs = w + o_xs, *W0 = w + o_W0, *W1 = same ? W0 : w + o_W1, *cv = w + o_cv, *d_pars = w + o_pars, *d_ell = w + o_ell,
           *d_Lv = w + o_Lv, *d_star = w + o_star, *d_z = z ? w + o_z : nullptr, *d_mean = w + o_mean, *d_colsq = w + o_colsq,
           *d_var = w + o_var, *part = w + o_part, *Sb = w + o_S;
    int* d_info = reinterpret_cast<int*>(w + o_info);

    HIP_TRY(c, hipMemcpyAsync(d_xs, xs, (size_t)S * sizeof(double), hipMemcpyHostToDevice, s));
    if (regress) {
        NMGP_TRY(project_rows(c, pl, d_xs, S, W0));
        NMGP_LAUNCH(k_ps_condvar, dim3(S), dim3(256), 0, s, W0, c->d_x, N, d_xs, al_l, be_l, cv);
        if (!same) NMGP_TRY(project_rows(c, pL, d_xs, S, W1));
        NMGP_LAUNCH(k_ps_condvar, dim3(S), dim3(256), 0, s, W1, c->d_x, N, d_xs, al_L, be_L, cv + S);
    }
    std::vector<int> hinfo(B);
    for (int h0 = 0; h0 < H; h0 += B) {
        const int Bc = std::min(B, H - h0);
        HIP_TRY(c, hipMemcpyAsync(d_pars, pars + (size_t)h0 * P, (size_t)Bc * P * sizeof(double), hipMemcpyHostToDevice, s));
        svc_prep(s, d_pars, N, M, d_ell, d_Lv, Bc);
        if (regress) {
            if (z) HIP_TRY(c, hipMemcpyAsync(d_z, z + (size_t)h0 * SC, Bc * SC * sizeof(double), hipMemcpyHostToDevice, s));
            NMGP_LAUNCH(k_ps_star, dim3(S, 1 + T, Bc), dim3(256), 0, s, W0, W1, cv, d_pars, d_Lv, d_z, N, M, T, S, mu_l, mu_L,
                        constrained ? 1 : 0, d_star);
        } else {
            HIP_TRY(c, hipMemcpyAsync(d_star, star_in + (size_t)h0 * SC, Bc * SC * sizeof(double), hipMemcpyHostToDevice, s));
        }
        HIP_TRY(c, hipMemsetAsync(d_info, 0, (size_t)Bc * sizeof(int), s));
        for (int s0 = 0; s0 < S; s0 += smax) {
            const int Sc = std::min(smax, S - s0), E = Sc * M;
            int r = svc_cov_build(s, c->d_x, d_ell, d_Lv, d_pars + (P - 1), Sb, ld, N, M, false, Bc, bs, 0, 1);
            if (r) return nmgp_fail(c, r, "unsupported number of outputs M=%d", M);
            set_row(s, Sb, ld, n, c->d_y, n, Bc, bs, 0, 1);
            NMGP_LAUNCH(k_ps_crosscov_rows, dim3(N, cdiv(E, 256), Bc), dim3(256), 0, s, c->d_x, d_ell, d_Lv, N, M, T, d_xs, d_star,
                        S, s0, Sc, Sb, ld, bs, n + 1);
            nmgp_potrf(c, Sb, ld, n, 1 + E, 0, d_info, Bc, bs, 1);
            NMGP_LAUNCH(k_ps_rows_part, dim3(cdiv(E, 64), chunks, Bc), dim3(256), 0, s, Sb, ld, bs, n, n + 1, n, E, part);
            NMGP_LAUNCH(k_ps_rows_sum, dim3(cdiv(E, 256), Bc), dim3(256), 0, s, part, chunks, E, d_mean, d_colsq, (long long)SMo,
                        (long long)s0 * M);
        }
        NMGP_LAUNCH(k_ps_predvar, dim3(cdiv((long long)SMo, 256), Bc), dim3(256), 0, s, d_star, d_colsq, S, M, T, d_pars, P, d_var);
        double* hm = mean + (size_t)h0 * SMo;
        double* hv = var + (size_t)h0 * SMo;
        HIP_TRY(c, hipMemcpyAsync(hm, d_mean, Bc * SMo * sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(hv, d_var, Bc * SMo * sizeof(double), hipMemcpyDeviceToHost, s));
        if (star_out)
            HIP_TRY(c, hipMemcpyAsync(star_out + (size_t)h0 * SC, d_star, Bc * SC * sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(hinfo.data(), d_info, (size_t)Bc * sizeof(int), hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        NMGP_TRY(nmgp_take_launch_error(c));
        // per-draw status as nmgp_svc_batch_fetch reports it: a failing draw yields NaN rows, not a failed call
        for (int b = 0; b < Bc; ++b) {
            int st = hinfo[b];
            if (st == 0)
                for (size_t k = 0; k < SMo; ++k)
                    if (!std::isfinite(hm[b * SMo + k]) || !std::isfinite(hv[b * SMo + k])) {
                        st = NMGP_NUM_NAN;
                        break;
                    }
            if (st != 0)
                for (size_t k = 0; k < SMo; ++k) hm[b * SMo + k] = hv[b * SMo + k] = std::nan("");
            if (status) status[h0 + b] = st;
        }
    }
    return 0;
}
