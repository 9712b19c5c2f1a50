// Hadamard form of the separable model: irregularly observed outputs, ONE cross-output matrix (logpos.py:465-563,
// prediction.py:710-808).
//
// The subject is the Hadamard one (nmgp_had_set_data: N single observations (x_i, c_i, y_i)).  The parameter vector is
// [tilde_l (N) | tilde_sigma (N) | L_vec (T) | tilde_sigma2_err], P = 2 N + T + 1.  L = vec2lowtriangle(L_vec) is taken as it is (no
// exp on the diagonal slots) and is shared by all observations: r_i = row c_i of L, zero-padded to M.  With l = exp(tilde_l),
// s = exp(tilde_sigma)
//   S = K_x o (R R^T) + sigma2 I,    K_x[i, j] = s_i s_j sqrt(2 l_i l_j / A) exp(-d_ij / A) + 1e-6 d_ij    (kernels.py:46-73)
// one dense N x N SPD matrix per evaluation.  Priors: a GP on tilde_l, a GP on tilde_sigma, Normal(0, c) on every raw L_vec slot,
// the unnormalised inverse gamma on sigma2.  The factorisation with its riding rows, the triangular matrix-vector product, the
// inverse SYRK, the trace terms and the cached prior factors are the library's.  The schedule of a batched evaluation and the Gibbs
// covariance / adjoint kernels (k_gibbs_cov, k_gibbs_adjoint with AMP = true: the amplitude s_i s_j) are nmgp_hadamard_common.h's,
// shared with the other two Hadamard models; this file adds the model's own kernels, its hooks into that schedule (HadSep) and the
// MAP predictor.
#include "nmgp_hadamard_common.h"

#include <algorithm>

using namespace nmgpk;

namespace {

inline unsigned cdiv(long long a, long long b) { return (unsigned)((a + b - 1) / b); }

// ell = exp(tilde_l), sig = exp(tilde_sigma);  Rv[i, 0..M) = row c_i of the chain's L, zero-padded (the slots as they are)
__global__ void k_hads_prep(const double* __restrict__ pars, const int* __restrict__ indx, int N, int M, int T,
                            double* __restrict__ ell, double* __restrict__ sig, double* __restrict__ Rv) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    pars += (size_t)blockIdx.y * ((size_t)2 * N + T + 1);         // blockIdx.y = chain
    ell += (size_t)blockIdx.y * N;
    sig += (size_t)blockIdx.y * N;
    Rv += (size_t)blockIdx.y * N * M;
    ell[i] = exp(pars[i]);
    sig[i] = exp(pars[N + i]);
    const int c = indx[i];
    const double* u = pars + (size_t)2 * N + c * (c + 1) / 2;
    for (int m = 0; m < M; ++m) Rv[(size_t)i * M + m] = (m <= c) ? u[m] : 0.0;
}

// Final gradient, part one: per observation the J partials summed in order; d NegLog / d tilde_l and / d tilde_sigma with the prior
// gradients Sigma_prior^-1 (v - mu) (R2: [N, 2] column-major per chain); the summed row components go to rsum[i, 0..M) for part
// two; the sigma2 terms (tr = {sum alpha^2, trace S^-1}; distributions.py:116-124 + the Jacobian).
__global__ __launch_bounds__(256) void k_hads_grad_obs(const double* __restrict__ part, int NJ, int N, int M, int T,
                                                        const double* __restrict__ R2, const double* __restrict__ pars,
                                                        const double* __restrict__ tr, double a, double b, int prior,
                                                        double* __restrict__ rsum, double* __restrict__ grad) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const size_t P = (size_t)2 * N + T + 1;
    {   // blockIdx.y = chain
        const size_t z = blockIdx.y;
        part += z * (size_t)NJ * N * (M + 2);
        R2 += z * (size_t)2 * N;
        pars += z * P;
        tr += z * 2;
        rsum += z * (size_t)N * M;
        grad += z * P;
    }
    if (i == 0) {
        const double sigma2 = exp(pars[P - 1]);
        double g = sigma2 * (0.5 * (tr[0] - tr[1]));
        if (prior) g += (-a - 1.0) + b / sigma2 + 1.0;
        grad[P - 1] = -g;
    }
    if (i >= N) return;
    for (int t = 0; t < M + 2; ++t) {
        double sacc = 0.0;
        for (int J = 0; J < NJ; ++J) sacc += part[((size_t)J * N + i) * (M + 2) + t];
        if (t < 2) {
            if (prior) sacc -= R2[(size_t)t * N + i];
            grad[(size_t)t * N + i] = -sacc;
        } else {
            rsum[(size_t)i * M + (t - 2)] = sacc;
        }
    }
}

// Final gradient, part two: the label-segmented reduction.  One workgroup per (slot t = (c, m), chain): thread k walks the
// observations k, k + 256, ... in index order adding the component m of those with label c, then the fixed tree over the 256
// threads.  Neither order depends on the batch.  The prior is Normal(0, c): d lp / d v = -v / var.
__global__ __launch_bounds__(256) void k_hads_grad_lvec(const double* __restrict__ rsum, const int* __restrict__ indx, int N, int M,
                                                         int T, const double* __restrict__ pars, double var, int prior,
                                                         double* __restrict__ grad) {
    __shared__ double sh[256];
    const int t = blockIdx.x;
    const size_t P = (size_t)2 * N + T + 1;
    rsum += (size_t)blockIdx.y * N * M;
    pars += (size_t)blockIdx.y * P;
    grad += (size_t)blockIdx.y * P;
    int c = 0;
    while ((c + 1) * (c + 2) / 2 <= t) ++c;
    const int m = t - c * (c + 1) / 2;
    double acc = 0.0;
    for (int i = threadIdx.x; i < N; i += 256)
        if (indx[i] == c) acc += rsum[(size_t)i * M + m];
    acc = block_sum_256(acc, sh);
    if (threadIdx.x == 0) {
        if (prior) acc -= pars[(size_t)2 * N + t] / var;
        grad[(size_t)2 * N + t] = -acc;
    }
}

// Scalar epilogue (logpos.py:527-563): q[0], q[1] the Mahalanobis terms of tilde_l and tilde_sigma, hl_l / hl_s the half
// log-determinants of the two prior covariances; Normal(0, c).log_prob with the float32-rounded variance and log c that torch
// uses for Python-number arguments (var, log_sd: computed by the host as normal_logprob_f32 of nmgp_eig.hip does).
__global__ void k_hads_finalize(const double* __restrict__ scal, const double* __restrict__ q, const double* __restrict__ hl_l,
                                const double* __restrict__ hl_s, const double* __restrict__ pars, int N, int T, double a, double b,
                                double var, double log_sd, int prior, double* __restrict__ out6) {
    if (threadIdx.x != 0) return;
    const size_t P = (size_t)2 * N + T + 1;
    scal += (size_t)blockIdx.x * 16;             // blockIdx.x = chain: [0] log det, [1] quadratic form, [8..13] the verbose tuple
    out6 += (size_t)blockIdx.x * 16;
    q += (size_t)blockIdx.x * 2;
    pars += (size_t)blockIdx.x * P;
    const double LOG2PI = 1.8378770664093453;
    const double tse = pars[P - 1];
    const double sigma2 = exp(tse);
    const double loglik = -0.5 * scal[0] - 0.5 * scal[1];
    const double lp_l = -0.5 * (N * LOG2PI + q[0]) - hl_l[0];
    const double lp_s = -0.5 * (N * LOG2PI + q[1]) - hl_s[0];
    double lp_L = 0.0;
    for (int t = 0; t < T; ++t) {
        const double v = pars[(size_t)2 * N + t];
        lp_L += -(v * v) / (2.0 * var) - log_sd - log(sqrt(2.0 * M_PI));
    }
    const double lp_s2 = (-a - 1.0) * log(sigma2) - b / sigma2;
    double res = 0.0;
    res += loglik;
    if (prior) {
        res += lp_l;
        res += lp_s;
        res += lp_L;
        res += lp_s2;
        res += tse;
    }
    out6[0] = -res;
    out6[1] = loglik;
    out6[2] = lp_l;
    out6[3] = lp_s;
    out6[4] = lp_L;
    out6[5] = lp_s2;
}

// Starred values at the new input s = blockIdx.x: tilde_l* (blockIdx.y = 0) and tilde_sigma* (1) = mu + proj_s . (curve - mu) with
// W0 / W1 = Sigma_prior^-1 K* ([S, N] row-major) under the two priors
__global__ __launch_bounds__(256) void k_hads_star(const double* __restrict__ W0, const double* __restrict__ W1,
                                                    const double* __restrict__ pars, int N, double mu_l, double mu_s,
                                                    double* __restrict__ star) {
    __shared__ double sh[256];
    const int s = blockIdx.x, which = blockIdx.y;
    const double* W = (which == 0 ? W0 : W1) + (size_t)s * N;
    const double mu = which == 0 ? mu_l : mu_s;
    const double* cur = pars + (size_t)which * N;
    double acc = 0.0;
    for (int i = threadIdx.x; i < N; i += 256) acc += W[i] * (cur[i] - mu);
    acc = block_sum_256(acc, sh);
    if (threadIdx.x == 0) star[(size_t)s * 2 + which] = mu + acc;
}

// Cross-covariances k_f[i, (s, m)] = s_i s*_s g(i, s) B_f[m, c_i] (prediction.py:765-770; Gibbs cross term without jitter), B_f[m,
// c_i] = <row m of L, r_i>, of the grid points s0 .. s0 + Sc - 1, written as riding rows R0 + e (e = (s - s0) M + m) below the
// covariance: the factorisation turns each into (L_S^-1 k_f[:, e])^T.  Lanes along the riding-row index (contiguous in a column).
template <int M>
__global__ __launch_bounds__(256) void k_hads_crosscov_rows(const double* __restrict__ x, const double* __restrict__ ell,
                                                             const double* __restrict__ sig, const double* __restrict__ Rv,
                                                             const double* __restrict__ Lvec, int N,
                                                             const double* __restrict__ xs, const double* __restrict__ star, int s0,
                                                             int Sc, double* __restrict__ A, int ld, int R0) {
    const int e = blockIdx.y * 256 + threadIdx.x;
    const int i = blockIdx.x;
    if (e >= Sc * M) return;
    const int s = s0 + e / M, mp = e % M;
    const double xi = x[i], li = ell[i];
    const double xj = xs[s], lj = exp(star[(size_t)s * 2]), sj = exp(star[(size_t)s * 2 + 1]);
    const double dist = (xi * xi + xj * xj) - 2.0 * (xi * xj);
    const double Aij = li * li + lj * lj;
    const double kv = (sig[i] * sj) * sqrt(2.0 * (li * lj) / Aij) * exp(-dist / Aij);
    double b = 0.0;
    for (int r = 0; r <= mp; ++r) b += Rv[(size_t)i * M + r] * Lvec[mp * (mp + 1) / 2 + r];
    A[(size_t)i * ld + R0 + e] = kv * b;
}

// var[s, m] = B_f[m, m] (s*_s^2 + jitter) - |L_S^-1 k_f[:, (s, m)]|^2 + sigma2, a value <= 0 replaced by settings.precision
// (prediction.py:774-782: the prior term is B_f kron Nonstationary_RBF_cov(x*), which carries the jitter)
__global__ void k_hads_predvar(const double* __restrict__ star, const double* __restrict__ Lvec, const double* __restrict__ colsq,
                               int S, int M, const double* __restrict__ tse, double* __restrict__ var) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= S * M) return;
    const int s = k / M, mp = k % M;
    double b = 0.0;
    for (int r = 0; r <= mp; ++r) {
        const double v = Lvec[mp * (mp + 1) / 2 + r];
        b += v * v;
    }
    const double ss = exp(star[(size_t)s * 2 + 1]);
    const double kss = NMGP_JITTER + ss * ss;
    double v = (b * kss - colsq[k]) + exp(tse[0]);
    if (v <= 0.0) v = NMGP_PRECISION;
    var[k] = v;
}

int hads_crosscov_rows(hipStream_t s, const double* x, const double* ell, const double* sig, const double* Rv, const double* Lvec,
                       int N, int M, const double* xs, const double* star, int s0, int Sc, double* A, int ld, int R0) {
    const dim3 grid(N, cdiv((long long)Sc * M, 256));
    NMGP_HADS_SWITCH(M, NMGP_LAUNCH((k_hads_crosscov_rows<MM>), grid, dim3(256), 0, s, x, ell, sig, Rv, Lvec, N, xs, star, s0, Sc,
                                    A, ld, R0));
    return 0;
}

// hooks of the separable model into the shared schedule (nmgp_hadamard_common.h)
struct HadSep {
    static constexpr int WIDTH = 6;
    static constexpr bool GP_PRIORS = true;
    static constexpr const char* NOUN = "separable Hadamard";
    static size_t P(int N, int T) { return (size_t)2 * N + T + 1; }
    static size_t part_width(int M) { return M + 2; }
    template <class Take>
    static void extras(HadLayout& L, Take take, size_t Bs, size_t N, int M, int, bool want_grad) {
        L.o_ell = take(Bs * N); L.o_sig = take(Bs * N); L.o_Rv = take(Bs * N * M); L.o_R = take(Bs * N * 2); L.o_q = take(Bs * 2);
        if (want_grad) { L.o_R2 = take(Bs * N * 2); L.o_rsum = take(Bs * N * M); }
    }
    // Normal(0, c) with a Python-number c: float32 (see k_hads_finalize)
    static double var_c(const double* hyper) { const float c32 = (float)hyper[8]; return (double)(c32 * c32); }
    static double log_sd_c(const double* hyper) { return (double)std::log((float)hyper[8]); }
    static int build_cov(const HadChunk& k) {
        nmgp_ctx* c = k.c;
        const int N = c->N, M = c->M;
        double *dP = k.at(k.L.o_P), *ell = k.at(k.L.o_ell), *sig = k.at(k.L.o_sig), *Rv = k.at(k.L.o_Rv);
        nmgp_hads_prep(c->stream, dP, c->had_indx, N, M, ell, sig, Rv, k.B);
        return nmgp_hads_cov_build(c->stream, c->d_x, ell, sig, Rv, dP, (long long)P(N, c->T), k.at(k.L.o_S), k.L.ld, N, M, k.B, k.L.bs);
    }
    static int value_epilogue(const HadChunk& k) {
        nmgp_ctx* c = k.c;
        const int N = c->N, T = c->T, B = k.B;
        const double mu_l = k.hyper[0], mu_s = k.hyper[3], a = k.hyper[6], b = k.hyper[7];
        double *dP = k.at(k.L.o_P), *scal = k.at(k.L.o_scal);
        NMGP_TRY(had_gp_prior_terms(k, 2, [&](hipStream_t sp, double* R) {        // two columns per chain
            two_col_rhs_b(sp, dP, (long long)P(N, T), mu_l, mu_s, N, R, B);
        }));
        NmgpStage sp(c, NMGP_STAGE_REDUCE);
        NMGP_LAUNCH(k_hads_finalize, dim3(B), dim3(64), 0, c->stream, scal, k.at(k.L.o_q), k.p0->logdet, k.p1->logdet, dP, N, T, a, b,
                    var_c(k.hyper), log_sd_c(k.hyper), k.prior, scal + 8);
        return 0;
    }
    static int adjoint_grad(const HadChunk& k) {
        nmgp_ctx* c = k.c;
        const int N = c->N, M = c->M, T = c->T, B = k.B, NJ = (N + 63) / 64;
        hipStream_t s = c->stream;
        double *dP = k.at(k.L.o_P), *part = k.at(k.L.o_part), *rsum = k.at(k.L.o_rsum), *dg = k.at(k.L.o_grad);
        // (the adjoint's partial rows are NJ * N * (M + 2) per chain, contiguous: the stride of part inside the kernels)
        NMGP_TRY(gibbs_adjoint<true>(s, c->d_x, k.at(k.L.o_ell), k.at(k.L.o_sig), k.at(k.L.o_Rv), k.at(k.L.o_alpha), k.at(k.L.o_Sneg), N, N,
                                     M, part, B));
        NMGP_LAUNCH(k_hads_grad_obs, dim3(cdiv(N, 256), B), dim3(256), 0, s, part, NJ, N, M, T, k.at(k.L.o_R2), dP, k.at(k.L.o_tr),
                    k.hyper[6], k.hyper[7], k.prior, rsum, dg);
        NMGP_LAUNCH(k_hads_grad_lvec, dim3(T, B), dim3(256), 0, s, rsum, c->had_indx, N, M, T, dP, var_c(k.hyper), k.prior, dg);
        return 0;
    }
};

}  // namespace

// the batched pieces the posterior-draw entry (nmgp_predsample_hadamard.hip) shares with the objective
void nmgp_hads_prep(hipStream_t s, const double* pars, const int* indx, int N, int M, double* ell, double* sig, double* Rv, int batch) {
    NMGP_LAUNCH(k_hads_prep, dim3(cdiv(N, 256), batch), dim3(256), 0, s, pars, indx, N, M, M * (M + 1) / 2, ell, sig, Rv);
}
int nmgp_hads_cov_build(hipStream_t s, const double* x, const double* ell, const double* sig, const double* Rv, const double* pars,
                        long long P, double* S, int ld, int N, int M, int batch, long long sstride) {
    return gibbs_cov_build<true>(s, x, ell, sig, Rv, pars, P, S, ld, N, M, batch, sstride);
}

// B chains of the resident Hadamard subject under the separable model: pars [B, P] -> out6 [B, 6] (the verbose tuples), grad [B, P]
// = d NegLog / d pars or NULL, status [B]; see had_batch_eval
extern "C" int nmgp_hads_batch_eval(nmgp_ctx* c, const double* pars, int B, const double hyper[9], int prior, double* out6,
                                    double* grad, int* status) {
    return had_batch_eval<HadSep>(c, pars, B, hyper, prior, out6, grad, status);
}

// out: [N, N] row-major, the full symmetric S = K_x o (R R^T) + sigma2 I
extern "C" int nmgp_hads_covariance(nmgp_ctx* c, const double* pars, double* out) { return had_covariance<HadSep>(c, pars, out); }

// MAP prediction of all M outputs at the new inputs xs [S]: the starred values by GP regression under the two priors, then ONE
// factorisation per slice of grid points with y and the slice's S_c M cross-covariance vectors riding below the matrix (the
// reference inverts through symeig).  mean, var: [S, M]; star: [S, 2] (tilde_l*, tilde_sigma*) or NULL.
extern "C" int nmgp_predict_hads(nmgp_ctx* c, const double* pars, const double hyper[9], const double* xs, int S, double* mean,
                                 double* var, double* star) {
    if (!c) return NMGP_E_NULL;
    if (!pars || !hyper || !xs || !mean || !var) return nmgp_fail(c, NMGP_E_NULL, "null argument");
    if (S <= 0) return nmgp_fail(c, NMGP_E_SHAPE, "S must be positive");
    NMGP_TRY(require_had(c));
    HIP_TRY(c, hipSetDevice(c->device));
    const int N = c->N, M = c->M, T = c->T;
    const size_t P = (size_t)2 * N + T + 1;
    hipStream_t s = c->stream;
    PriorFactor *pl = nullptr, *pg = nullptr;
    NMGP_TRY(had_priors(c, hyper, &pl, &pg));
    const int smax = std::max(1, N / M), Sm = std::min(S, smax), Emax = Sm * M;      // grid points per factorisation
    const int ld = (int)nmgp_ld((size_t)N + 1 + Emax);
    const int chunks = (N + 127) / 128;
    const size_t SN = (size_t)S * N, SMo = (size_t)S * M;
    auto ev = [](size_t n) { return (n + 1) & ~(size_t)1; };
    double *sm, *buf;
    NMGP_TRY(nmgp_scratch_get(c, HSL_SMALL, ev(P) + 2 * ev(N) + ev((size_t)N * M) + ev(S) + 2 * ev(SN) + 2 * ev(S) + ev((size_t)S * 2) +
                                            3 * ev(SMo) + ev((size_t)2 * Emax * chunks) + 2, &sm));
    NMGP_TRY(nmgp_scratch_get(c, HSL_PRED, (size_t)ld * N, &buf));
    double* dP = sm;
    double* ell = dP + ev(P);
    double* sig = ell + ev(N);
    double* Rv = sig + ev(N);
    double* d_xs = Rv + ev((size_t)N * M);
    double* W0 = d_xs + ev(S);
    double* W1 = W0 + ev(SN);
    double* cv = W1 + ev(SN);                     // [2, S] conditional variances of the regressions (not used by the MAP predictor)
    double* d_star = cv + 2 * ev(S);
    double* d_mean = d_star + ev((size_t)S * 2);
    double* d_colsq = d_mean + ev(SMo);
    double* d_var = d_colsq + ev(SMo);
    double* part = d_var + ev(SMo);
    int* info = reinterpret_cast<int*>(part + ev((size_t)2 * Emax * chunks));
    const double* Lvec = dP + (size_t)2 * N;
    HIP_TRY(c, hipMemcpyAsync(dP, pars, P * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(d_xs, xs, (size_t)S * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemsetAsync(info, 0, sizeof(int), s));
    NMGP_TRY(nmgp_ps_project(c, pl, d_xs, S, W0, cv));
    if (pl != pg) NMGP_TRY(nmgp_ps_project(c, pg, d_xs, S, W1, cv + ev(S)));
    NMGP_LAUNCH(k_hads_star, dim3(S, 2), dim3(256), 0, s, W0, pl != pg ? W1 : W0, dP, N, hyper[0], hyper[3], d_star);
    nmgp_hads_prep(s, dP, c->had_indx, N, M, ell, sig, Rv, 1);
    for (int s0 = 0; s0 < S; s0 += smax) {
        const int Sc = std::min(smax, S - s0), E = Sc * M;
        int r = nmgp_hads_cov_build(s, c->d_x, ell, sig, Rv, dP, (long long)P, buf, ld, N, M, 1, 0);
        if (r) return nmgp_fail(c, r, "unsupported number of outputs M=%d", M);
        set_row(s, buf, ld, N, c->had_y, N, 1, 0, 0);
        NMGP_TRY(hads_crosscov_rows(s, c->d_x, ell, sig, Rv, Lvec, N, M, d_xs, d_star, s0, Sc, buf, ld, N + 1));
        // the substitution-based panel kernels, as every batched entry: their bits do not depend on the schedule the batch size
        // selects, so this predictor is nmgp_predsample_hads with one draw and no noise, bit for bit
        nmgp_potrf(c, buf, ld, N, 1 + E, 0, info, 1, 0, 0, 1);
        ps_rows_reduce(s, buf, ld, 0, N, N + 1, N, E, part, 1, d_mean, d_colsq, 0, (long long)s0 * M);
    }
    NMGP_LAUNCH(k_hads_predvar, dim3(cdiv((long long)S * M, 256)), dim3(256), 0, s, d_star, Lvec, d_colsq, S, M, dP + (P - 1), d_var);
    int h_info = 0;
    HIP_TRY(c, hipMemcpyAsync(mean, d_mean, SMo * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(var, d_var, SMo * sizeof(double), hipMemcpyDeviceToHost, s));
    if (star) HIP_TRY(c, hipMemcpyAsync(star, d_star, (size_t)S * 2 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(&h_info, info, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    NMGP_TRY(nmgp_take_launch_error(c));
    if (h_info != 0) return nmgp_fail(c, h_info, "covariance not positive definite (leading minor %d)", h_info);
    c->last_kind = 0;
    return 0;
}
