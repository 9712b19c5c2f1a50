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
// inverse SYRK, the trace terms and the cached prior factors are the library's; this file adds the kernels around them and the
// entries.  Layout conventions of nmgp_hadamard.hip: a 64 x 64 tile of observations per 256-thread workgroup, lanes along i, the j
// side in LDS, blockIdx.z = chain; fixed summation order and no atomics, so B chains in one launch give the bits of B launches.
#include "nmgp_internal.h"

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

// S[i, j] = (K0(i, j) + jitter d_ij) <r_i, r_j> + sigma2 d_ij, lower triangle, column-major with leading dimension ld
template <int M>
__global__ __launch_bounds__(256) void k_hads_cov(const double* __restrict__ x, const double* __restrict__ ell,
                                                   const double* __restrict__ sig, const double* __restrict__ Rv,
                                                   const double* __restrict__ pars, long long P, double* __restrict__ S, int ld,
                                                   int N, long long sstride) {
    constexpr int TJ = 64;
    __shared__ double sx[TJ], sl[TJ], ss[TJ], sR[TJ * M];
    const int I = blockIdx.x, J = blockIdx.y;
    if (I < J) return;
    ell += (size_t)blockIdx.z * N;
    sig += (size_t)blockIdx.z * N;
    Rv += (size_t)blockIdx.z * N * M;
    pars += (size_t)blockIdx.z * P;
    S += (size_t)blockIdx.z * sstride;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int j0 = J * TJ;
    if (tid < TJ) {
        const int j = j0 + tid;
        sx[tid] = (j < N) ? x[j] : 0.0;
        sl[tid] = (j < N) ? ell[j] : 1.0;
        ss[tid] = (j < N) ? sig[j] : 1.0;
    }
    for (int k = tid; k < TJ * M; k += 256) {
        const size_t g = (size_t)j0 * M + k;
        sR[k] = (g < (size_t)N * M) ? Rv[g] : 0.0;
    }
    __syncthreads();
    const int i = I * 64 + lane;
    if (i >= N) return;
    const double sigma2 = exp(pars[P - 1]);
    const double xi = x[i], li = ell[i], si = sig[i];
    const double xi2 = xi * xi, li2 = li * li;
    double ri[M];
#pragma unroll
    for (int m = 0; m < M; ++m) ri[m] = Rv[(size_t)i * M + m];
#pragma unroll 2
    for (int jj = 0; jj < TJ / 4; ++jj) {
        const int k = w * (TJ / 4) + jj;
        const int j = j0 + k;
        if (j >= N) break;
        if (i < j) continue;
        const double xj = sx[k], lj = sl[k];
        const double dist = (xi2 + xj * xj) - 2.0 * (xi * xj);                     // kernels.py:20
        const double A = li2 + lj * lj;                                            // kernels.py:69
        double kv = (si * ss[k]) * sqrt(2.0 * (li * lj) / A) * exp(-dist / A);     // kernels.py:70-72
        if (i == j) kv = NMGP_JITTER + kv;                                         // kernels.py:64
        double b = 0.0;
#pragma unroll
        for (int m = 0; m < M; ++m) b += ri[m] * sR[k * M + m];
        double v = kv * b;
        if (i == j) v += sigma2;
        S[(size_t)j * ld + i] = v;
    }
}

// Adjoint of the likelihood, one pass over the FULL symmetric -S^-1 (what the inverse SYRK leaves):
//   G = 1/2 (alpha alpha^T - S^-1),  K0[i, j] = s_i s_j g_ij (no jitter),  K_x = K0 + jitter I
//   d loglik / d tilde_l_i     = sum_{j != i} 2 G_ij K0[i, j] <r_i, r_j> (1/2 - l_i^2 / A + 2 l_i^2 d_ij / A^2),  A = l_i^2 + l_j^2
//   d loglik / d tilde_sigma_i = sum_j 2 G_ij K0[i, j] <r_i, r_j>                                   (j = i included)
//   row component m of i       = sum_j 2 G_ij K_x[i, j] r_j[m]          (summed over {i : c_i = c} it is d loglik / d L[c, m])
// Each wave takes 16 j; the four waves' sums meet in LDS and leave part[J][i][0 .. M + 1] (slot 0 = tilde_l, 1 = tilde_sigma,
// 2 + m = row component m).
template <int M>
__global__ __launch_bounds__(256) void k_hads_adjoint(const double* __restrict__ x, const double* __restrict__ ell,
                                                       const double* __restrict__ sig, const double* __restrict__ Rv,
                                                       const double* __restrict__ alpha, const double* __restrict__ Sneg, int ld,
                                                       int N, double* __restrict__ part) {
    constexpr int TJ = 64;
    __shared__ double sx[TJ], sl[TJ], ss[TJ], sR[TJ * M], sa[TJ];
    __shared__ double red[2][4][64];
    const int I = blockIdx.x, J = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int j0 = J * TJ;
    const size_t Ns = (size_t)N;
    {   // blockIdx.z = chain
        const size_t z = blockIdx.z;
        ell += z * Ns;
        sig += z * Ns;
        Rv += z * Ns * M;
        alpha += z * Ns;
        Sneg += z * (size_t)ld * Ns;
        part += z * (size_t)gridDim.y * Ns * (M + 2);
    }
    if (tid < TJ) {
        const int j = j0 + tid;
        sx[tid] = (j < N) ? x[j] : 0.0;
        sl[tid] = (j < N) ? ell[j] : 1.0;
        ss[tid] = (j < N) ? sig[j] : 1.0;
        sa[tid] = (j < N) ? alpha[j] : 0.0;
    }
    for (int k = tid; k < TJ * M; k += 256) {
        const size_t g = (size_t)j0 * M + k;
        sR[k] = (g < Ns * M) ? Rv[g] : 0.0;
    }
    __syncthreads();
    const int i = I * 64 + lane;
    const bool iv = i < N;
    const int ic = iv ? i : N - 1;
    const double xi = x[ic], li = ell[ic], si = sig[ic], ai = alpha[ic];
    const double xi2 = xi * xi, li2 = li * li;
    double ri[M], acc[M + 2];
#pragma unroll
    for (int m = 0; m < M; ++m) ri[m] = Rv[(size_t)ic * M + m];
#pragma unroll
    for (int t = 0; t < M + 2; ++t) acc[t] = 0.0;
    if (iv) {
        for (int jj = 0; jj < TJ / 4; ++jj) {
            const int k = w * (TJ / 4) + jj;
            const int j = j0 + k;
            if (j >= N) break;
            const double xj = sx[k], lj = sl[k];
            const double dist = (xi2 + xj * xj) - 2.0 * (xi * xj);
            const double A = li2 + lj * lj;
            const double k0 = (si * ss[k]) * sqrt(2.0 * (li * lj) / A) * exp(-dist / A);
            const double kx = (i == j) ? (NMGP_JITTER + k0) : k0;
            const double G = 0.5 * (ai * sa[k] + Sneg[(size_t)j * ld + i]);
            const double gk = 2.0 * kx * G;
            double dot = 0.0;
#pragma unroll
            for (int m = 0; m < M; ++m) {
                const double rj = sR[k * M + m];
                acc[2 + m] = fma(gk, rj, acc[2 + m]);
                dot = fma(ri[m], rj, dot);
            }
            const double gd = 2.0 * (G * dot) * k0;
            acc[1] += gd;
            if (i != j) {
                const double dlogk = 0.5 - li2 / A + 2.0 * li2 * dist / (A * A);
                acc[0] = fma(gd, dlogk, acc[0]);
            }
        }
    }
    double* o = part + ((size_t)J * Ns + ic) * (M + 2);
#pragma unroll
    for (int t = 0; t < M + 2; ++t) {
        red[t & 1][w][lane] = acc[t];
        __syncthreads();
        if (w == 0 && iv) o[t] = (red[t & 1][0][lane] + red[t & 1][1][lane]) + (red[t & 1][2][lane] + red[t & 1][3][lane]);
    }
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

void hads_prep(hipStream_t s, const double* pars, const int* indx, int N, int M, double* ell, double* sig, double* Rv, int batch) {
    NMGP_LAUNCH(k_hads_prep, dim3(cdiv(N, 256), batch), dim3(256), 0, s, pars, indx, N, M, M * (M + 1) / 2, ell, sig, Rv);
}

int hads_cov_build(hipStream_t s, const double* x, const double* ell, const double* sig, const double* Rv, const double* pars,
                   long long P, double* S, int ld, int N, int M, int batch, long long sstride) {
    const dim3 grid(cdiv(N, 64), cdiv(N, 64), batch);
    NMGP_HADS_SWITCH(M, NMGP_LAUNCH((k_hads_cov<MM>), grid, dim3(256), 0, s, x, ell, sig, Rv, pars, P, S, ld, N, sstride));
    return 0;
}

int hads_adjoint(hipStream_t s, const double* x, const double* ell, const double* sig, const double* Rv, const double* alpha,
                 const double* Sneg, int ld, int N, int M, double* part, int batch) {
    const dim3 grid(cdiv(N, 64), cdiv(N, 64), batch);      // -S^-1 of chain z: ld x N doubles further on
    NMGP_HADS_SWITCH(M, NMGP_LAUNCH((k_hads_adjoint<MM>), grid, dim3(256), 0, s, x, ell, sig, Rv, alpha, Sneg, ld, N, part));
    return 0;
}

int hads_crosscov_rows(hipStream_t s, const double* x, const double* ell, const double* sig, const double* Rv, const double* Lvec,
                       int N, int M, const double* xs, const double* star, int s0, int Sc, double* A, int ld, int R0) {
    const dim3 grid(N, cdiv((long long)Sc * M, 256));
    NMGP_HADS_SWITCH(M, NMGP_LAUNCH((k_hads_crosscov_rows<MM>), grid, dim3(256), 0, s, x, ell, sig, Rv, Lvec, N, xs, star, s0, Sc,
                                    A, ld, R0));
    return 0;
}

// device workspace of a chunk of B chains, in doubles (every piece at an even offset)
struct HadsLayout {
    size_t o_P, o_ell, o_sig, o_Rv, o_z, o_R, o_q, o_scal, o_info, o_S;
    size_t o_alpha = 0, o_R2 = 0, o_Sneg = 0, o_part = 0, o_rsum = 0, o_grad = 0, o_tr = 0;
    size_t total = 0, tri_part = 0, part_per = 0;
    int ld = 0, xpad = 0, xoff = 0;
    long long bs = 0;
};

HadsLayout hads_layout(int B, int N, int M, int T, bool want_grad) {
    HadsLayout L;
    const size_t P = (size_t)2 * N + T + 1, Bs = B, NJ = (N + 63) / 64;
    // rows: N (matrix) + 1 (y); with gradients + pad + N identity rows (-> L^-T)
    L.xpad = (N + 1) & 1;
    L.xoff = N + 1 + L.xpad;
    L.ld = (int)nmgp_ld(want_grad ? (size_t)2 * N + 2 : (size_t)N + 1);
    L.bs = (long long)L.ld * N;
    L.tri_part = (size_t)N * ((N + 255) / 256);
    // adjoint partial rows; before that pass the same buffer holds the block sums of alpha = L^-T z (tri_gemv_upper)
    L.part_per = std::max(NJ * (size_t)N * (M + 2), L.tri_part);
    size_t off = 0;
    auto take = [&](size_t n) { size_t o = off; off += (n + 1) & ~(size_t)1; return o; };
    L.o_P = take(Bs * P); L.o_ell = take(Bs * N); L.o_sig = take(Bs * N); L.o_Rv = take(Bs * N * M); L.o_z = take(Bs * N);
    L.o_R = take(Bs * N * 2); L.o_q = take(Bs * 2); L.o_scal = take(Bs * 16); L.o_info = take(Bs);
    L.o_S = take(Bs * (size_t)L.bs);
    if (want_grad) {
        L.o_alpha = take(Bs * N); L.o_R2 = take(Bs * N * 2); L.o_Sneg = take(Bs * (size_t)N * N);
        L.o_part = take(Bs * L.part_per); L.o_rsum = take(Bs * N * M);
        L.o_grad = take(Bs * P); L.o_tr = take(Bs * 2);
    }
    L.total = off;
    return L;
}

// chains [0, B) of `pars` (already offset by the caller): value and gradient halves enqueued back to back, ONE synchronisation
int hads_batch_core(nmgp_ctx* c, const double* pars, int B, const double hyper[9], int prior, double* out6, double* grad,
                    int* status) {
    const int N = c->N, M = c->M, T = c->T;
    const size_t P = (size_t)2 * N + T + 1;
    const bool want_grad = grad != nullptr;
    const double mu_l = hyper[0], mu_s = hyper[3], a = hyper[6], b = hyper[7];
    const float c32 = (float)hyper[8];                  // Normal(0, c) with a Python-number c: float32 (see k_hads_finalize)
    const double var = (double)(c32 * c32), log_sd = (double)std::log(c32);
    hipStream_t s = c->stream;
    PriorFactor *pl = nullptr, *pg = nullptr;
    NMGP_TRY(had_priors(c, hyper, &pl, &pg));
    const HadsLayout L = hads_layout(B, N, M, T, want_grad);
    double* slab;
    NMGP_TRY(nmgp_scratch_get(c, HSL_SLAB, L.total, &slab));
    double *dP = slab + L.o_P, *ell = slab + L.o_ell, *sig = slab + L.o_sig, *Rv = slab + L.o_Rv, *z = slab + L.o_z;
    double *R = slab + L.o_R, *q = slab + L.o_q, *scal = slab + L.o_scal, *S = slab + L.o_S;
    int* info = reinterpret_cast<int*>(slab + L.o_info);
    const int ld = L.ld;
    const long long bs = L.bs;
    HIP_TRY(c, hipMemcpyAsync(dP, pars, (size_t)B * P * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemsetAsync(info, 0, (size_t)B * sizeof(int), s));
    PriorStreamScope ps(c);          // fork now, enqueue the prior solves after the factorisation's launches
    {
        NmgpStage sp(c, NMGP_STAGE_COV);
        hads_prep(s, dP, c->had_indx, N, M, ell, sig, Rv, B);
        int r = hads_cov_build(s, c->d_x, ell, sig, Rv, dP, (long long)P, S, ld, N, M, B, bs);
        if (r) return nmgp_fail(c, r, "unsupported number of outputs M=%d", M);
    }
    {
        NmgpStage sp(c, NMGP_STAGE_CHOL);
        set_row(s, S, ld, N, c->had_y, N, B, bs, 0);                // y rides along as row N (shared by the chains)
        if (want_grad) identity_rows(s, S, ld, N + 1, N, L.xpad, B, bs);
        nmgp_potrf(c, S, ld, N, want_grad ? 1 + L.xpad : 1, want_grad ? N : 0, info, B, bs, 1);
        get_row(s, S, ld, N, z, N, B, bs, N);                       // z = L^-1 y
    }
    {
        NmgpStage sp(c, NMGP_STAGE_REDUCE);
        chol_logdet_quad(s, S, ld, N, z, scal, scal + 1, B, bs, 16);
    }
    {
        NmgpStage sp(c, NMGP_STAGE_PRIOR, ps.sp, 0.0, 0.0);
        two_col_rhs_b(ps.sp, dP, (long long)P, mu_l, mu_s, N, R, B);
        NMGP_TRY(had_prior_solve(c, ps.sp, ps.hb, false, pl, pg, R, N, 1, B));     // two columns per chain
        col_sumsq(ps.sp, R, N, N, B * 2, q);
        if (want_grad && prior) {
            double* R2 = slab + L.o_R2;
            HIP_TRY(c, hipMemcpyAsync(R2, R, (size_t)B * N * 2 * sizeof(double), hipMemcpyDeviceToDevice, ps.sp));
            NMGP_TRY(had_prior_solve(c, ps.sp, ps.hb, true, pl, pg, R2, N, 1, B));
        }
    }
    ps.done();
    ps.join();
    {
        NmgpStage sp(c, NMGP_STAGE_REDUCE);
        NMGP_LAUNCH(k_hads_finalize, dim3(B), dim3(64), 0, s, scal, q, pl->logdet, pg->logdet, dP, N, T, a, b, var, log_sd, prior,
                    scal + 8);
    }
    std::vector<double> hs((size_t)B * 16);
    std::vector<int> hi(B);
    HIP_TRY(c, hipMemcpyAsync(hs.data(), scal, hs.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(hi.data(), info, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, s));
    if (want_grad) {
        // enqueued behind the value half without waiting for it (a chain that failed produces garbage here, which the epilogue discards)
        double *alpha = slab + L.o_alpha, *R2 = slab + L.o_R2, *Sneg = slab + L.o_Sneg, *part = slab + L.o_part;
        double *rsum = slab + L.o_rsum, *dg = slab + L.o_grad, *tr = slab + L.o_tr;
        const int NJ = (N + 63) / 64;
        {
            NmgpStage sp(c, NMGP_STAGE_SOLVE);
            tri_gemv_upper(s, S + L.xoff, ld, N, z, alpha, part, B, bs, (long long)L.part_per);   // alpha = L^-T z = X z
        }
        {
            NmgpStage sp(c, NMGP_STAGE_INVERSE);
            syrk_lower(s, S + L.xoff, ld, Sneg, N, N, N, N, B, bs, (long long)N * N, 2);         // -S^-1 = -X X^T, both triangles
        }
        {
            NmgpStage sp(c, NMGP_STAGE_ADJOINT);
            trace_terms(s, alpha, Sneg, N, N, tr, -1.0, B);
            // (the adjoint's partial rows are NJ * N * (M + 2) per chain, contiguous: the stride of part inside the kernels)
            int r = hads_adjoint(s, c->d_x, ell, sig, Rv, alpha, Sneg, N, N, M, part, B);
            if (r) return nmgp_fail(c, r, "unsupported number of outputs M=%d", M);
            NMGP_LAUNCH(k_hads_grad_obs, dim3(cdiv(N, 256), B), dim3(256), 0, s, part, NJ, N, M, T, R2, dP, tr, a, b, prior, rsum, dg);
            NMGP_LAUNCH(k_hads_grad_lvec, dim3(T, B), dim3(256), 0, s, rsum, c->had_indx, N, M, T, dP, var, prior, dg);
        }
        HIP_TRY(c, hipMemcpyAsync(grad, dg, (size_t)B * P * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(c, hipStreamSynchronize(s));          // the one synchronisation of the evaluation
    NMGP_TRY(nmgp_take_launch_error(c));
    for (int z_ = 0; z_ < B; ++z_) {
        int st = hi[z_];
        double* o = out6 + (size_t)z_ * 6;
        for (int k = 0; k < 6; ++k) o[k] = hs[(size_t)z_ * 16 + 8 + k];
        // a parameter vector that is not finite has no leading minor to blame: NMGP_NUM_NAN whatever pivot met the NaN first
        bool finite_in = true;
        for (size_t k = 0; k < P && finite_in; ++k) finite_in = std::isfinite(pars[(size_t)z_ * P + k]);
        if (!finite_in || (st == 0 && (!std::isfinite(o[0]) || !std::isfinite(o[1])))) st = NMGP_NUM_NAN;
        if (st != 0) {
            for (int k = 0; k < 6; ++k) o[k] = std::nan("");
            if (want_grad) std::fill(grad + (size_t)z_ * P, grad + (size_t)(z_ + 1) * P, 0.0);
        }
        status[z_] = st;
    }
    return 0;
}

}  // namespace

// the batched pieces the posterior-draw entry (nmgp_predsample_hadamard.hip) shares with the objective
void nmgp_hads_prep(hipStream_t s, const double* pars, const int* indx, int N, int M, double* ell, double* sig, double* Rv, int batch) {
    hads_prep(s, pars, indx, N, M, ell, sig, Rv, batch);
}
int nmgp_hads_cov_build(hipStream_t s, const double* x, const double* ell, const double* sig, const double* Rv, const double* pars,
                        long long P, double* S, int ld, int N, int M, int batch, long long sstride) {
    return hads_cov_build(s, x, ell, sig, Rv, pars, P, S, ld, N, M, batch, sstride);
}

// B chains of the resident Hadamard subject under the separable model: pars [B, P] -> out6 [B, 6] (the verbose tuples), grad [B, P]
// = d NegLog / d pars or NULL, status [B] (0, a leading-minor index, NMGP_NUM_NAN; a failing chain has a NaN row, a zero gradient
// row, and does not fail the call).  The workspace is the entry's own, evaluated in chunks of chains below NMGP_HAD_BATCH_SLAB_GB
// (default 96).
extern "C" int nmgp_hads_batch_eval(nmgp_ctx* c, const double* pars, int B, const double hyper[9], int prior, double* out6,
                                    double* grad, int* status) {
    if (!c) return NMGP_E_NULL;
    if (!pars || !hyper || !out6 || !status) return nmgp_fail(c, NMGP_E_NULL, "pars/hyper/out6/status must not be NULL");
    if (B <= 0) return nmgp_fail(c, NMGP_E_SHAPE, "B must be positive");
    NMGP_TRY(require_had(c));
    HIP_TRY(c, hipSetDevice(c->device));
    const int N = c->N, M = c->M, T = c->T;
    const size_t P = (size_t)2 * N + T + 1;
    const bool want_grad = grad != nullptr;
    double cap_gb = 96.0;
    if (const char* e = std::getenv("NMGP_HAD_BATCH_SLAB_GB")) cap_gb = std::max(1.0, std::atof(e));
    const size_t per_chain = hads_layout(1, N, M, T, want_grad).total * sizeof(double);
    int Bc = (int)std::min<double>((double)B, std::floor(cap_gb * 1e9 / (double)per_chain));
    Bc = std::min(Bc, 65535);                      // the chain is a grid dimension
    if (Bc < 1)
        return nmgp_fail(c, NMGP_E_SHAPE, "one chain of the separable Hadamard model at N = %d needs %.1f GB of device workspace, "
                         "above the NMGP_HAD_BATCH_SLAB_GB cap of %.0f GB", N, per_chain / 1e9, cap_gb);
    for (int b0 = 0; b0 < B; b0 += Bc) {
        const int nb = std::min(Bc, B - b0);
        NMGP_TRY(hads_batch_core(c, pars + (size_t)b0 * P, nb, hyper, prior, out6 + (size_t)b0 * 6,
                                 want_grad ? grad + (size_t)b0 * P : nullptr, status + b0));
    }
    c->last_kind = 0;
    return 0;
}

// out: [N, N] row-major, the full symmetric S = K_x o (R R^T) + sigma2 I
extern "C" int nmgp_hads_covariance(nmgp_ctx* c, const double* pars, double* out) {
    if (!c) return NMGP_E_NULL;
    if (!pars || !out) return nmgp_fail(c, NMGP_E_NULL, "pars/out must not be NULL");
    NMGP_TRY(require_had(c));
    HIP_TRY(c, hipSetDevice(c->device));
    const int N = c->N, M = c->M, T = c->T;
    const size_t P = (size_t)2 * N + T + 1;
    hipStream_t s = c->stream;
    const int ld = (int)nmgp_ld((size_t)N);
    auto ev = [](size_t n) { return (n + 1) & ~(size_t)1; };
    double* w;
    NMGP_TRY(nmgp_scratch_get(c, HSL_SLAB, ev(P) + 2 * ev(N) + ev((size_t)N * M) + (size_t)ld * N, &w));
    double *dP = w, *ell = dP + ev(P), *sig = ell + ev(N), *Rv = sig + ev(N), *S = Rv + ev((size_t)N * M);
    HIP_TRY(c, hipMemcpyAsync(dP, pars, P * sizeof(double), hipMemcpyHostToDevice, s));
    hads_prep(s, dP, c->had_indx, N, M, ell, sig, Rv, 1);
    int r = hads_cov_build(s, c->d_x, ell, sig, Rv, dP, (long long)P, S, ld, N, M, 1, 0);
    if (r) return nmgp_fail(c, r, "unsupported number of outputs M=%d", M);
    fill_lower_to_full(s, S, ld, N);
    HIP_TRY(c, hipMemcpy2DAsync(out, (size_t)N * sizeof(double), S, (size_t)ld * sizeof(double), (size_t)N * sizeof(double), (size_t)N,
                                hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    return nmgp_take_launch_error(c);
}

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
    hads_prep(s, dP, c->had_indx, N, M, ell, sig, Rv, 1);
    for (int s0 = 0; s0 < S; s0 += smax) {
        const int Sc = std::min(smax, S - s0), E = Sc * M;
        int r = hads_cov_build(s, c->d_x, ell, sig, Rv, dP, (long long)P, buf, ld, N, M, 1, 0);
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
