// Hadamard form of the nonseparable model: irregularly observed outputs (logpos.py:566-659, prediction.py:1401-1478).
//
// The data are N single observations (x_i, c_i, y_i), c_i = indx[i] naming the output that was measured at x_i.  The parameter
// vector has the nonseparable layout [tilde_l (N) | L_vecs (N T, row-major per observation) | tilde_sigma2_err], with two
// differences: L_vecs enters vec2lowtriangle as it is (no exp on the diagonal slots), and only ROW c_i of L_i reaches the
// likelihood.  With r_i = that row (slots c_i (c_i + 1) / 2 .. + c_i of observation i, zero-padded to M)
//   S = K_x o (R R^T) + sigma2 I,    K_x the Gibbs kernel of kernels.py:46-73 (+ 1e-6 on its diagonal),
// ONE dense N x N SPD matrix per evaluation: the SVC covariance restricted to the observed (output, input) pairs.  Everything
// between the covariance build and the adjoint is the library's own: the blocked Cholesky with its riding rows (y, the rows of
// L^-T, the cross-covariance rows of prediction), the triangular matrix-vector product, the inverse SYRK, the cached prior
// factors.  The schedule of a batched evaluation and the Gibbs covariance / adjoint kernels (k_gibbs_cov, k_gibbs_adjoint with AMP =
// false: unit amplitude) are nmgp_hadamard_common.h's, shared with the other two Hadamard models.  This file adds the model's own
// kernels (k_had_prep, k_had_grad_final, k_had_star, k_had_crosscov_rows, k_had_predvar), its hooks into that schedule
// (HadNonsep), the MAP predictor and the three host helpers every Hadamard file calls (require_had, had_priors, had_prior_solve).
// There is no structured (Schur) value path: no per-location block to eliminate.
#include "nmgp_hadamard_common.h"

#include <algorithm>

using namespace nmgpk;

namespace {

inline unsigned cdiv(long long a, long long b) { return (unsigned)((a + b - 1) / b); }

// ell = exp(tilde_l);  Rv[i, 0..M) = row c_i of L_i, zero-padded (the slots are taken as they are: no exp)
__global__ void k_had_prep(const double* __restrict__ pars, const int* __restrict__ indx, int N, int M, int T,
                           double* __restrict__ ell, double* __restrict__ Rv) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    pars += (size_t)blockIdx.y * ((size_t)N * (1 + T) + 1);       // blockIdx.y = chain
    ell += (size_t)blockIdx.y * N;
    Rv += (size_t)blockIdx.y * N * M;
    ell[i] = exp(pars[i]);
    const int c = indx[i];
    const double* u = pars + N + (size_t)i * T + c * (c + 1) / 2;
    for (int m = 0; m < M; ++m) Rv[(size_t)i * M + m] = (m <= c) ? u[m] : 0.0;
}

// d NegLog / d pars: the J partials summed in order, the c_i + 1 components of d / d r_i scattered into row c_i's slots, the prior
// gradients Sigma_prior^-1 (v - mu) of tilde_l and of ALL T columns (R2: [N, 1 + T] column-major per chain), the sigma2 terms
// (tr = {sum alpha^2, trace S^-1}; distributions.py:126-134), negated.  The slots are raw: no exp chain rule.
__global__ __launch_bounds__(256) void k_had_grad_final(const double* __restrict__ part, int NJ, int N, int M, int T,
                                                         const int* __restrict__ indx, const double* __restrict__ R2, int ldR,
                                                         const double* __restrict__ pars, const double* __restrict__ tr, double a,
                                                         double b, int prior, double* __restrict__ grad) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const size_t P = (size_t)N * (1 + T) + 1;
    {   // blockIdx.y = chain
        const size_t z = blockIdx.y;
        part += z * (size_t)NJ * N * (M + 1);
        R2 += z * (size_t)(1 + T) * ldR;
        pars += z * P;
        tr += z * 2;
        grad += z * P;
    }
    if (i == 0) {
        const double sigma2 = exp(pars[P - 1]);
        double g = sigma2 * (0.5 * (tr[0] - tr[1]));
        if (prior) g += (-a - 1.0) + b / sigma2 + 1.0;
        grad[P - 1] = -g;
    }
    if (i >= N) return;
    const int c = indx[i], t0 = c * (c + 1) / 2;
    {
        double sacc = 0.0;
        for (int J = 0; J < NJ; ++J) sacc += part[((size_t)J * N + i) * (M + 1)];
        if (prior) sacc -= R2[i];
        grad[i] = -sacc;
    }
    for (int t = 0; t < T; ++t) {
        double g = 0.0;
        if (t >= t0 && t <= t0 + c) {
            double sacc = 0.0;
            for (int J = 0; J < NJ; ++J) sacc += part[((size_t)J * N + i) * (M + 1) + 1 + (t - t0)];
            if (prior) sacc -= R2[(size_t)(1 + t) * ldR + i];
            g = -sacc;
        } else if (prior) {
            g = R2[(size_t)(1 + t) * ldR + i];
        }
        grad[N + (size_t)i * T + t] = g;
    }
}

// Starred values at the new input s = blockIdx.x, slot cidx = blockIdx.y (0: tilde_l*, 1 + t: slot t of L*): mu + proj_s . (curve - mu)
// with W0 / W1 = Sigma_prior^-1 K* ([S, N] row-major) under the tilde_l / L prior; the L* slots are taken as they are (no exp).
__global__ __launch_bounds__(256) void k_had_star(const double* __restrict__ W0, const double* __restrict__ W1,
                                                   const double* __restrict__ pars, int N, int T, double mu_l, double mu_L,
                                                   double* __restrict__ star) {
    __shared__ double sh[256];
    const int s = blockIdx.x, cidx = blockIdx.y;
    const double* W = (cidx == 0 ? W0 : W1) + (size_t)s * N;
    const double mu = cidx == 0 ? mu_l : mu_L;
    const double* cur = cidx == 0 ? pars : pars + N + (cidx - 1);
    const size_t stride = cidx == 0 ? 1 : (size_t)T;
    double acc = 0.0;
    for (int i = threadIdx.x; i < N; i += 256) acc += W[i] * (cur[(size_t)i * stride] - mu);
    acc = block_sum_256(acc, sh);
    if (threadIdx.x == 0) star[(size_t)s * (1 + T) + cidx] = mu + acc;
}

// Cross-covariances k_f[i, (s, m)] = k_x(i, s) <r_i, L*_s[m, :]> (prediction.py:1446-1451; Gibbs cross term without jitter, l* =
// exp(tilde_l*)) of the grid points s0 .. s0 + Sc - 1, written as riding rows R0 + e (e = (s - s0) M + m) below the covariance:
// the factorisation turns each into (L^-1 k_f[:, e])^T.  Lanes along the riding-row index (contiguous in a column).
template <int M>
__global__ __launch_bounds__(256) void k_had_crosscov_rows(const double* __restrict__ x, const double* __restrict__ ell,
                                                            const double* __restrict__ Rv, int N, const double* __restrict__ xs,
                                                            const double* __restrict__ star, int s0, int Sc,
                                                            double* __restrict__ A, int ld, int R0) {
    constexpr int T = M * (M + 1) / 2;
    const int e = blockIdx.y * 256 + threadIdx.x;
    const int i = blockIdx.x;
    if (e >= Sc * M) return;
    const int s = s0 + e / M, mp = e % M;
    const double* st = star + (size_t)s * (1 + T);
    const double xi = x[i], li = ell[i];
    const double xj = xs[s], lj = exp(st[0]);
    const double dist = (xi * xi + xj * xj) - 2.0 * (xi * xj);
    const double Aij = li * li + lj * lj;
    const double kv = sqrt(2.0 * (li * lj) / Aij) * exp(-dist / Aij);
    double b = 0.0;
    for (int r = 0; r <= mp; ++r) b += Rv[(size_t)i * M + r] * st[1 + mp * (mp + 1) / 2 + r];
    A[(size_t)i * ld + R0 + e] = kv * b;
}

// var[s, m] = (1 + jitter) (L* L*^T)_mm - |L^-1 k_f[:, (s, m)]|^2 + sigma2, a value <= 0 replaced by settings.precision
// (prediction.py:1455-1461)
__global__ void k_had_predvar(const double* __restrict__ star, const double* __restrict__ colsq, int S, int M, int T,
                              const double* __restrict__ tse, double* __restrict__ var) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= S * M) return;
    const int s = k / M, mp = k % M;
    const double* st = star + (size_t)s * (1 + T) + 1;
    double b = 0.0;
    for (int r = 0; r <= mp; ++r) {
        const double v = st[mp * (mp + 1) / 2 + r];
        b += v * v;
    }
    const double kss = NMGP_JITTER + 1.0;
    double v = (kss * b - colsq[k]) + exp(tse[0]);
    if (v <= 0.0) v = NMGP_PRECISION;
    var[k] = v;
}

void had_grad_final(hipStream_t s, const double* part, int NJ, int N, int M, const int* indx, const double* R2, int ldR,
                    const double* pars, const double* tr, double a, double b, int prior, double* grad, int batch) {
    NMGP_LAUNCH(k_had_grad_final, dim3(cdiv(N, 256), batch), dim3(256), 0, s, part, NJ, N, M, M * (M + 1) / 2, indx, R2, ldR, pars, tr,
                a, b, prior, grad);
}

int had_crosscov_rows(hipStream_t s, const double* x, const double* ell, const double* Rv, int N, int M, const double* xs,
                      const double* star, int s0, int Sc, double* A, int ld, int R0) {
    const dim3 grid(N, cdiv((long long)Sc * M, 256));
    NMGP_HADS_SWITCH(M, NMGP_LAUNCH((k_had_crosscov_rows<MM>), grid, dim3(256), 0, s, x, ell, Rv, N, xs, star, s0, Sc, A, ld, R0));
    return 0;
}

}  // namespace

// The next four are declared in nmgp_internal.h: require_had guards every entry of the three Hadamard models and of the two
// posterior-draw files; had_priors / had_prior_solve serve the two models with GP priors (this one and the separable one); had_prep
// unpacks this model's parameter vectors, here and in nmgp_predsample_had.hip.
int require_had(nmgp_ctx* c) {
    if (!c->had || !c->d_x) return nmgp_fail(c, NMGP_E_STATE, "nmgp_had_set_data must be called first (the resident subject is not a Hadamard one)");
    if (c->chol_algo != 1)
        return nmgp_fail(c, NMGP_E_UNSUPPORTED, "the Hadamard entries run on the custom factorisation only (riding rows)");
    return 0;
}

void had_prep(hipStream_t s, const double* pars, const int* indx, int N, int M, double* ell, double* Rv, int batch) {
    NMGP_LAUNCH(k_had_prep, dim3(cdiv(N, 256), batch), dim3(256), 0, s, pars, indx, N, M, M * (M + 1) / 2, ell, Rv);
}

// the two cached prior factors (the cache is a vector: the second look-up may move its elements, so the first is re-resolved)
int had_priors(nmgp_ctx* c, const double* hyper, PriorFactor** pl, PriorFactor** pL) {
    NMGP_TRY(nmgp_get_prior(c, hyper[1], hyper[2], pl));
    NMGP_TRY(nmgp_get_prior(c, hyper[4], hyper[5], pL));
    NMGP_TRY(nmgp_get_prior(c, hyper[1], hyper[2], pl));
    return 0;
}

// op(L) X = R for the 1 + T prior columns of every chain (column 0 against pl, the others against pL).  By substitution, one
// workgroup per column, wherever the right-hand side fits the kernel's LDS: a column's bits then do not depend on how many chains
// share the launch.  Beyond that the library's trsm.
int had_prior_solve(nmgp_ctx* c, hipStream_t sp, rocblas_handle hb, bool trans, PriorFactor* pl, PriorFactor* pL, double* R, int N,
                    int T, int B) {
    if (N <= 3500 && !c->prior_rocblas) {
        prior_trsv(sp, trans, pl->L, pl->ld, 0, pL->L, pL->ld, 0, R, N, 1 + T, B);
        return 0;
    }
    const double one = 1.0;
    const rocblas_operation op = trans ? rocblas_operation_transpose : rocblas_operation_none;
    if (pl == pL) {
        BLAS_TRY(c, rocblas_dtrsm(hb, rocblas_side_left, rocblas_fill_lower, op, rocblas_diagonal_non_unit, N, B * (1 + T), &one, pl->L,
                                  pl->ld, R, N));
    } else {
        const rocblas_stride sB = (rocblas_stride)(1 + T) * N;
        BLAS_TRY(c, rocblas_dtrsm_strided_batched(hb, rocblas_side_left, rocblas_fill_lower, op, rocblas_diagonal_non_unit, N, 1, &one,
                                                  pl->L, pl->ld, 0, R, N, sB, B));
        BLAS_TRY(c, rocblas_dtrsm_strided_batched(hb, rocblas_side_left, rocblas_fill_lower, op, rocblas_diagonal_non_unit, N, T, &one,
                                                  pL->L, pL->ld, 0, R + N, N, sB, B));
    }
    return 0;
}

namespace {

// hooks of the nonseparable model into the shared schedule (nmgp_hadamard_common.h)
struct HadNonsep {
    static constexpr int WIDTH = 5;
    static constexpr bool GP_PRIORS = true;
    static constexpr const char* NOUN = "Hadamard";
    static size_t P(int N, int T) { return (size_t)N * (1 + T) + 1; }
    static size_t part_width(int M) { return M + 1; }
    template <class Take>
    static void extras(HadLayout& L, Take take, size_t Bs, size_t N, int M, int T, bool want_grad) {
        L.o_ell = take(Bs * N); L.o_Rv = take(Bs * N * M); L.o_R = take(Bs * N * (1 + T)); L.o_q = take(Bs * (1 + T));
        if (want_grad) L.o_R2 = take(Bs * N * (1 + T));
    }
    static int build_cov(const HadChunk& k) {
        nmgp_ctx* c = k.c;
        const int N = c->N, M = c->M;
        double *dP = k.at(k.L.o_P), *ell = k.at(k.L.o_ell), *Rv = k.at(k.L.o_Rv);
        had_prep(c->stream, dP, c->had_indx, N, M, ell, Rv, k.B);
        return gibbs_cov_build<false>(c->stream, c->d_x, ell, nullptr, Rv, dP, (long long)P(N, c->T), k.at(k.L.o_S), k.L.ld, N, M, k.B,
                                      k.L.bs);
    }
    static int value_epilogue(const HadChunk& k) {
        nmgp_ctx* c = k.c;
        const int N = c->N, T = c->T, B = k.B;
        const double mu_l = k.hyper[0], mu_L = k.hyper[3], a = k.hyper[6], b = k.hyper[7];
        double *dP = k.at(k.L.o_P), *scal = k.at(k.L.o_scal);
        NMGP_TRY(had_gp_prior_terms(k, 1 + T, [&](hipStream_t sp, double* R) { svc_prior_rhs(sp, dP, N, T, mu_l, mu_L, R, N, B); }));
        NmgpStage sp(c, NMGP_STAGE_REDUCE);
        // (ig_const = 0: the Hadamard objective uses the UNNORMALISED inverse-gamma density, logpos.py:650 / distributions.py:116-124,
        // where logpos_SVC uses the normalised one)
        svc_finalize(c->stream, scal, scal + 1, k.at(k.L.o_q), k.p0->logdet, k.p1->logdet, dP, (long long)P(N, T), N, T, a, b, 0.0,
                     k.prior, scal + 8, B, 16, 0, 1);
        return 0;
    }
    static int adjoint_grad(const HadChunk& k) {
        nmgp_ctx* c = k.c;
        const int N = c->N, M = c->M;
        double* part = k.at(k.L.o_part);
        // (the adjoint's partial rows are (N + 63) / 64 * N * (M + 1) per chain, contiguous: the stride of part inside the kernel)
        NMGP_TRY(gibbs_adjoint<false>(c->stream, c->d_x, k.at(k.L.o_ell), nullptr, k.at(k.L.o_Rv), k.at(k.L.o_alpha), k.at(k.L.o_Sneg), N,
                                      N, M, part, k.B));
        had_grad_final(c->stream, part, (N + 63) / 64, N, M, c->had_indx, k.at(k.L.o_R2), N, k.at(k.L.o_P), k.at(k.L.o_tr), k.hyper[6],
                       k.hyper[7], k.prior, k.at(k.L.o_grad), k.B);
        return 0;
    }
};

}  // namespace

// B chains of the resident Hadamard subject: pars [B, P] -> out5 [B, 5] (the verbose tuples), grad [B, P] = d NegLog / d pars or
// NULL, status [B]; see had_batch_eval
extern "C" int nmgp_had_batch_eval(nmgp_ctx* c, const double* pars, int B, const double hyper[8], int prior, double* out5,
                                   double* grad, int* status) {
    return had_batch_eval<HadNonsep>(c, pars, B, hyper, prior, out5, grad, status);
}

// out: [N, N] row-major, the full symmetric S = K_x o (R R^T) + sigma2 I
extern "C" int nmgp_had_covariance(nmgp_ctx* c, const double* pars, double* out) { return had_covariance<HadNonsep>(c, pars, out); }

// MAP prediction of all M outputs at the new inputs xs [S]: the starred values by GP regression under the two priors, then ONE
// factorisation per slice of grid points with y and the slice's S_c M cross-covariance vectors riding below the matrix.
// mean, var: [S, M]; star: [S, 1 + T] (tilde_l*, the T slots of L*) or NULL.
extern "C" int nmgp_predict_had(nmgp_ctx* c, const double* pars, const double hyper[8], const double* xs, int S, double* mean,
                                double* var, double* star) {
    if (!c) return NMGP_E_NULL;
    if (!pars || !hyper || !xs || !mean || !var) return nmgp_fail(c, NMGP_E_NULL, "null argument");
    if (S <= 0) return nmgp_fail(c, NMGP_E_SHAPE, "S must be positive");
    NMGP_TRY(require_had(c));
    HIP_TRY(c, hipSetDevice(c->device));
    const int N = c->N, M = c->M, T = c->T;
    const size_t P = (size_t)N * (1 + T) + 1;
    hipStream_t s = c->stream;
    PriorFactor *pl = nullptr, *pL = nullptr;
    NMGP_TRY(had_priors(c, hyper, &pl, &pL));
    const int smax = std::max(1, N / M), Sm = std::min(S, smax), Emax = Sm * M;      // grid points per factorisation
    const int ld = (int)nmgp_ld((size_t)N + 1 + Emax);
    const int chunks = (N + 127) / 128;
    const size_t SN = (size_t)S * N, SMo = (size_t)S * M;
    auto ev = [](size_t n) { return (n + 1) & ~(size_t)1; };
    double *sm, *buf;
    NMGP_TRY(nmgp_scratch_get(c, HSL_SMALL, ev(P) + ev(N) + ev((size_t)N * M) + ev(S) + 2 * ev(SN) + 2 * ev(S) + ev((size_t)S * (1 + T)) +
                                            3 * ev(SMo) + ev((size_t)2 * Emax * chunks) + 2, &sm));
    NMGP_TRY(nmgp_scratch_get(c, HSL_PRED, (size_t)ld * N, &buf));
    double* dP = sm;
    double* ell = dP + ev(P);
    double* Rv = ell + ev(N);
    double* d_xs = Rv + ev((size_t)N * M);
    double* W0 = d_xs + ev(S);
    double* W1 = W0 + ev(SN);
    double* cv = W1 + ev(SN);                     // [2, S] conditional variances of the regressions (not used by the MAP predictor)
    double* d_star = cv + 2 * ev(S);
    double* d_mean = d_star + ev((size_t)S * (1 + T));
    double* d_colsq = d_mean + ev(SMo);
    double* d_var = d_colsq + ev(SMo);
    double* part = d_var + ev(SMo);
    int* info = reinterpret_cast<int*>(part + ev((size_t)2 * Emax * chunks));
    HIP_TRY(c, hipMemcpyAsync(dP, pars, P * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(d_xs, xs, (size_t)S * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemsetAsync(info, 0, sizeof(int), s));
    NMGP_TRY(nmgp_ps_project(c, pl, d_xs, S, W0, cv));
    if (pl != pL) NMGP_TRY(nmgp_ps_project(c, pL, d_xs, S, W1, cv + ev(S)));
    NMGP_LAUNCH(k_had_star, dim3(S, 1 + T), dim3(256), 0, s, W0, pl != pL ? W1 : W0, dP, N, T, hyper[0], hyper[3], d_star);
    had_prep(s, dP, c->had_indx, N, M, ell, Rv, 1);
    for (int s0 = 0; s0 < S; s0 += smax) {
        const int Sc = std::min(smax, S - s0), E = Sc * M;
        int r = gibbs_cov_build<false>(s, c->d_x, ell, nullptr, Rv, dP, (long long)P, buf, ld, N, M, 1, 0);
        if (r) return nmgp_fail(c, r, "unsupported number of outputs M=%d", M);
        set_row(s, buf, ld, N, c->had_y, N, 1, 0, 0);
        NMGP_TRY(had_crosscov_rows(s, c->d_x, ell, Rv, N, M, d_xs, d_star, s0, Sc, buf, ld, N + 1));
        nmgp_potrf(c, buf, ld, N, 1 + E, 0, info);
        ps_rows_reduce(s, buf, ld, 0, N, N + 1, N, E, part, 1, d_mean, d_colsq, 0, (long long)s0 * M);
    }
    NMGP_LAUNCH(k_had_predvar, dim3(cdiv((long long)S * M, 256)), dim3(256), 0, s, d_star, d_colsq, S, M, T, dP + (P - 1), d_var);
    int h_info = 0;
    HIP_TRY(c, hipMemcpyAsync(mean, d_mean, SMo * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(var, d_var, SMo * sizeof(double), hipMemcpyDeviceToHost, s));
    if (star) HIP_TRY(c, hipMemcpyAsync(star, d_star, (size_t)S * (1 + T) * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(&h_info, info, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    NMGP_TRY(nmgp_take_launch_error(c));
    if (h_info != 0) return nmgp_fail(c, h_info, "covariance not positive definite (leading minor %d)", h_info);
    c->last_kind = 0;
    return 0;
}
