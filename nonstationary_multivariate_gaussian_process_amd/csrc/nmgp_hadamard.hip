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
// factors.  This file adds the kernels around them (k_had_prep, k_had_cov, k_had_adjoint, k_had_grad_final,
// k_had_crosscov_rows) and the entries.  There is no structured (Schur) value path: no per-location block to eliminate.
//
// Layout conventions of k_svc_cov / k_svc_adjoint: a 64 x 64 tile of observations per 256-thread workgroup, lanes along i (a wave
// stores / loads 512 contiguous bytes of one column), the j side staged in LDS, blockIdx.z = chain; fixed summation order and no
// atomics, so B chains in one launch give the bits of B launches.
#include "nmgp_internal.h"

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

// S[i, j] = (K0(i, j) + jitter d_ij) <r_i, r_j> + sigma2 d_ij, lower triangle, column-major with leading dimension ld
template <int M>
__global__ __launch_bounds__(256) void k_had_cov(const double* __restrict__ x, const double* __restrict__ ell,
                                                  const double* __restrict__ Rv, const double* __restrict__ pars, long long P,
                                                  double* __restrict__ S, int ld, int N, long long sstride) {
    constexpr int TJ = 64;
    __shared__ double sx[TJ], sl[TJ], sR[TJ * M];
    const int I = blockIdx.x, J = blockIdx.y;
    if (I < J) return;
    ell += (size_t)blockIdx.z * N;
    Rv += (size_t)blockIdx.z * N * M;
    pars += (size_t)blockIdx.z * P;
    S += (size_t)blockIdx.z * sstride;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int j0 = J * TJ;
    if (tid < TJ) {
        const int j = j0 + tid;
        sx[tid] = (j < N) ? x[j] : 0.0;
        sl[tid] = (j < N) ? ell[j] : 1.0;
    }
    for (int k = tid; k < TJ * M; k += 256) {
        const size_t g = (size_t)j0 * M + k;
        sR[k] = (g < (size_t)N * M) ? Rv[g] : 0.0;
    }
    __syncthreads();
    const int i = I * 64 + lane;
    if (i >= N) return;
    const double sigma2 = exp(pars[P - 1]);
    const double xi = x[i], li = ell[i];
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
        const double dist = (xi2 + xj * xj) - 2.0 * (xi * xj);   // kernels.py:20
        const double A = li2 + lj * lj;                          // kernels.py:69
        double kv = sqrt(2.0 * (li * lj) / A) * exp(-dist / A);  // kernels.py:70,72 (sigma == 1)
        if (i == j) kv = NMGP_JITTER + kv;                       // kernels.py:64
        double b = 0.0;
#pragma unroll
        for (int m = 0; m < M; ++m) b += ri[m] * sR[k * M + m];
        double v = kv * b;
        if (i == j) v += sigma2;
        S[(size_t)j * ld + i] = v;
    }
}

// Adjoint of the likelihood, one pass over the FULL symmetric -S^-1 (what the inverse SYRK leaves):
//   G = 1/2 (alpha alpha^T - S^-1)
//   d loglik / d r_i       = 2 sum_j G_ij K_x[i, j] r_j                       (j = i included)
//   d loglik / d tilde_l_i = sum_{j != i} 2 G_ij K0[i, j] <r_i, r_j> (1/2 - l_i^2 / A + 2 l_i^2 d_ij / A^2),  A = l_i^2 + l_j^2
// Each wave takes 16 j; the four waves' sums meet in LDS and leave part[J][i][0..M] (slot 0 = tilde_l, 1 + m = component m of r_i).
template <int M>
__global__ __launch_bounds__(256) void k_had_adjoint(const double* __restrict__ x, const double* __restrict__ ell,
                                                      const double* __restrict__ Rv, const double* __restrict__ alpha,
                                                      const double* __restrict__ Sneg, int ld, int N, double* __restrict__ part) {
    constexpr int TJ = 64;
    __shared__ double sx[TJ], sl[TJ], sR[TJ * M], sa[TJ];
    __shared__ double red[2][4][64];
    const int I = blockIdx.x, J = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int j0 = J * TJ;
    const size_t Ns = (size_t)N;
    {   // blockIdx.z = chain
        const size_t z = blockIdx.z;
        ell += z * Ns;
        Rv += z * Ns * M;
        alpha += z * Ns;
        Sneg += z * (size_t)ld * Ns;
        part += z * (size_t)gridDim.y * Ns * (M + 1);
    }
    if (tid < TJ) {
        const int j = j0 + tid;
        sx[tid] = (j < N) ? x[j] : 0.0;
        sl[tid] = (j < N) ? ell[j] : 1.0;
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
    const double xi = x[ic], li = ell[ic], ai = alpha[ic];
    const double xi2 = xi * xi, li2 = li * li;
    double ri[M], acc[M + 1];
#pragma unroll
    for (int m = 0; m < M; ++m) ri[m] = Rv[(size_t)ic * M + m];
#pragma unroll
    for (int t = 0; t <= M; ++t) acc[t] = 0.0;
    if (iv) {
        for (int jj = 0; jj < TJ / 4; ++jj) {
            const int k = w * (TJ / 4) + jj;
            const int j = j0 + k;
            if (j >= N) break;
            const double xj = sx[k], lj = sl[k];
            const double dist = (xi2 + xj * xj) - 2.0 * (xi * xj);
            const double A = li2 + lj * lj;
            const double k0 = sqrt(2.0 * (li * lj) / A) * exp(-dist / A);
            const double kx = (i == j) ? (NMGP_JITTER + k0) : k0;
            const double G = 0.5 * (ai * sa[k] + Sneg[(size_t)j * ld + i]);
            const double gk = 2.0 * kx * G;
            double dot = 0.0;
#pragma unroll
            for (int m = 0; m < M; ++m) {
                const double rj = sR[k * M + m];
                acc[1 + m] = fma(gk, rj, acc[1 + m]);
                dot = fma(ri[m], rj, dot);
            }
            if (i != j) {
                const double dlogk = 0.5 - li2 / A + 2.0 * li2 * dist / (A * A);
                acc[0] = fma(2.0 * (G * dot) * k0, dlogk, acc[0]);
            }
        }
    }
    double* o = part + ((size_t)J * Ns + ic) * (M + 1);
#pragma unroll
    for (int t = 0; t <= M; ++t) {
        red[t & 1][w][lane] = acc[t];
        __syncthreads();
        if (w == 0 && iv) o[t] = (red[t & 1][0][lane] + red[t & 1][1][lane]) + (red[t & 1][2][lane] + red[t & 1][3][lane]);
    }
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

#define NMGP_HAD_SWITCH(M, CALL)                \
    switch (M) {                                \
        case 1: { constexpr int MM = 1; CALL; } break; \
        case 2: { constexpr int MM = 2; CALL; } break; \
        case 3: { constexpr int MM = 3; CALL; } break; \
        case 4: { constexpr int MM = 4; CALL; } break; \
        case 5: { constexpr int MM = 5; CALL; } break; \
        case 6: { constexpr int MM = 6; CALL; } break; \
        case 7: { constexpr int MM = 7; CALL; } break; \
        case 8: { constexpr int MM = 8; CALL; } break; \
        default: return NMGP_E_UNSUPPORTED;     \
    }

void had_prep(hipStream_t s, const double* pars, const int* indx, int N, int M, double* ell, double* Rv, int batch) {
    NMGP_LAUNCH(k_had_prep, dim3(cdiv(N, 256), batch), dim3(256), 0, s, pars, indx, N, M, M * (M + 1) / 2, ell, Rv);
}

int had_cov_build(hipStream_t s, const double* x, const double* ell, const double* Rv, const double* pars, long long P, double* S,
                  int ld, int N, int M, int batch, long long sstride) {
    const dim3 grid(cdiv(N, 64), cdiv(N, 64), batch);
    NMGP_HAD_SWITCH(M, NMGP_LAUNCH((k_had_cov<MM>), grid, dim3(256), 0, s, x, ell, Rv, pars, P, S, ld, N, sstride));
    return 0;
}

int had_adjoint(hipStream_t s, const double* x, const double* ell, const double* Rv, const double* alpha, const double* Sneg,
                int ld, int N, int M, double* part, int batch) {
    const dim3 grid(cdiv(N, 64), cdiv(N, 64), batch);      // -S^-1 of chain z: ld x N doubles further on
    NMGP_HAD_SWITCH(M, NMGP_LAUNCH((k_had_adjoint<MM>), grid, dim3(256), 0, s, x, ell, Rv, alpha, Sneg, ld, N, part));
    return 0;
}

void had_grad_final(hipStream_t s, const double* part, int NJ, int N, int M, const int* indx, const double* R2, int ldR,
                    const double* pars, const double* tr, double a, double b, int prior, double* grad, int batch) {
    NMGP_LAUNCH(k_had_grad_final, dim3(cdiv(N, 256), batch), dim3(256), 0, s, part, NJ, N, M, M * (M + 1) / 2, indx, R2, ldR, pars, tr,
                a, b, prior, grad);
}

int had_crosscov_rows(hipStream_t s, const double* x, const double* ell, const double* Rv, int N, int M, const double* xs,
                      const double* star, int s0, int Sc, double* A, int ld, int R0) {
    const dim3 grid(N, cdiv((long long)Sc * M, 256));
    NMGP_HAD_SWITCH(M, NMGP_LAUNCH((k_had_crosscov_rows<MM>), grid, dim3(256), 0, s, x, ell, Rv, N, xs, star, s0, Sc, A, ld, R0));
    return 0;
}

}  // namespace

// (the next three are shared with nmgp_hadamard_sep.hip: declared in nmgp_internal.h)
int require_had(nmgp_ctx* c) {
    if (!c->had || !c->d_x) return nmgp_fail(c, NMGP_E_STATE, "nmgp_had_set_data must be called first (the resident subject is not a Hadamard one)");
    if (c->chol_algo != 1)
        return nmgp_fail(c, NMGP_E_UNSUPPORTED, "the Hadamard entries run on the custom factorisation only (riding rows)");
    return 0;
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

// device workspace of a chunk of B chains, in doubles (every piece at an even offset)
struct HadLayout {
    size_t o_P, o_ell, o_Rv, o_z, o_R, o_q, o_scal, o_info, o_S;
    size_t o_alpha = 0, o_R2 = 0, o_Sneg = 0, o_part = 0, o_grad = 0, o_tr = 0;
    size_t total = 0, tri_part = 0;
    int ld = 0, xpad = 0, xoff = 0;
    long long bs = 0;
};

HadLayout had_layout(int B, int N, int M, int T, bool want_grad) {
    HadLayout L;
    const size_t P = (size_t)N * (1 + T) + 1, Bs = B, NJ = (N + 63) / 64;
    // rows: N (matrix) + 1 (y); with gradients + pad + N identity rows (-> L^-T)
    L.xpad = (N + 1) & 1;
    L.xoff = N + 1 + L.xpad;
    L.ld = (int)nmgp_ld(want_grad ? (size_t)2 * N + 2 : (size_t)N + 1);
    L.bs = (long long)L.ld * N;
    L.tri_part = (size_t)N * ((N + 255) / 256);
    size_t off = 0;
    auto take = [&](size_t n) { size_t o = off; off += (n + 1) & ~(size_t)1; return o; };
    L.o_P = take(Bs * P); L.o_ell = take(Bs * N); L.o_Rv = take(Bs * N * M); L.o_z = take(Bs * N);
    L.o_R = take(Bs * N * (1 + T)); L.o_q = take(Bs * (1 + T)); L.o_scal = take(Bs * 16); L.o_info = take(Bs);
    L.o_S = take(Bs * (size_t)L.bs);
    if (want_grad) {
        L.o_alpha = take(Bs * N); L.o_R2 = take(Bs * N * (1 + T)); L.o_Sneg = take(Bs * (size_t)N * N);
        // adjoint partial rows; before that pass the same buffer holds the block sums of alpha = L^-T z (tri_gemv_upper)
        L.o_part = take(Bs * std::max(NJ * (size_t)N * (M + 1), L.tri_part));
        L.o_grad = take(Bs * P); L.o_tr = take(Bs * 2);
    }
    L.total = off;
    return L;
}

// chains [0, B) of `pars` (already offset by the caller): value and gradient halves enqueued back to back, ONE synchronisation
int had_batch_core(nmgp_ctx* c, const double* pars, int B, const double hyper[8], int prior, double* out5, double* grad, int* status) {
    const int N = c->N, M = c->M, T = c->T;
    const size_t P = (size_t)N * (1 + T) + 1;
    const bool want_grad = grad != nullptr;
    const double mu_l = hyper[0], mu_L = hyper[3], a = hyper[6], b = hyper[7];
    hipStream_t s = c->stream;
    PriorFactor *pl = nullptr, *pL = nullptr;
    NMGP_TRY(had_priors(c, hyper, &pl, &pL));
    const HadLayout L = had_layout(B, N, M, T, want_grad);
    double* slab;
    NMGP_TRY(nmgp_scratch_get(c, HSL_SLAB, L.total, &slab));
    double *dP = slab + L.o_P, *ell = slab + L.o_ell, *Rv = slab + L.o_Rv, *z = slab + L.o_z, *R = slab + L.o_R, *q = slab + L.o_q;
    double *scal = slab + L.o_scal, *S = slab + L.o_S;
    int* info = reinterpret_cast<int*>(slab + L.o_info);
    const int ld = L.ld;
    const long long bs = L.bs;
    HIP_TRY(c, hipMemcpyAsync(dP, pars, (size_t)B * P * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemsetAsync(info, 0, (size_t)B * sizeof(int), s));
    PriorStreamScope ps(c);          // fork now, enqueue the prior solves after the factorisation's launches (see svc_enqueue)
    {
        NmgpStage sp(c, NMGP_STAGE_COV);
        had_prep(s, dP, c->had_indx, N, M, ell, Rv, B);
        int r = had_cov_build(s, c->d_x, ell, Rv, dP, (long long)P, S, ld, N, M, B, bs);
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
        svc_prior_rhs(ps.sp, dP, N, T, mu_l, mu_L, R, N, B);
        NMGP_TRY(had_prior_solve(c, ps.sp, ps.hb, false, pl, pL, R, N, T, B));
        col_sumsq(ps.sp, R, N, N, B * (1 + T), q);
        if (want_grad && prior) {
            double* R2 = slab + L.o_R2;
            HIP_TRY(c, hipMemcpyAsync(R2, R, (size_t)B * N * (1 + T) * sizeof(double), hipMemcpyDeviceToDevice, ps.sp));
            NMGP_TRY(had_prior_solve(c, ps.sp, ps.hb, true, pl, pL, R2, N, T, B));
        }
    }
    ps.done();
    ps.join();
    {
        NmgpStage sp(c, NMGP_STAGE_REDUCE);
        // (ig_const = 0: the Hadamard objective uses the UNNORMALISED inverse-gamma density, logpos.py:650 / distributions.py:116-124,
        // where logpos_SVC uses the normalised one)
        svc_finalize(s, scal, scal + 1, q, pl->logdet, pL->logdet, dP, (long long)P, N, T, a, b, 0.0, prior, scal + 8, B, 16, 0, 1);
    }
    std::vector<double> hs((size_t)B * 16);
    std::vector<int> hi(B);
    HIP_TRY(c, hipMemcpyAsync(hs.data(), scal, hs.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(hi.data(), info, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, s));
    if (want_grad) {
        // enqueued behind the value half without waiting for it (a chain that failed produces garbage here, which the epilogue discards)
        double *alpha = slab + L.o_alpha, *R2 = slab + L.o_R2, *Sneg = slab + L.o_Sneg, *part = slab + L.o_part;
        double *dg = slab + L.o_grad, *tr = slab + L.o_tr;
        const long long pstride = (long long)std::max((size_t)((N + 63) / 64) * N * (M + 1), L.tri_part);
        {
            NmgpStage sp(c, NMGP_STAGE_SOLVE);
            tri_gemv_upper(s, S + L.xoff, ld, N, z, alpha, part, B, bs, pstride);                 // alpha = L^-T z = X z
        }
        {
            NmgpStage sp(c, NMGP_STAGE_INVERSE);
            syrk_lower(s, S + L.xoff, ld, Sneg, N, N, N, N, B, bs, (long long)N * N, 2);         // -S^-1 = -X X^T, both triangles
        }
        {
            NmgpStage sp(c, NMGP_STAGE_ADJOINT);
            trace_terms(s, alpha, Sneg, N, N, tr, -1.0, B);
            // (the adjoint's partial rows are (N + 63) / 64 * N * (M + 1) per chain, contiguous: the stride of part inside the kernel)
            int r = had_adjoint(s, c->d_x, ell, Rv, alpha, Sneg, N, N, M, part, B);
            if (r) return nmgp_fail(c, r, "unsupported number of outputs M=%d", M);
            had_grad_final(s, part, (N + 63) / 64, N, M, c->had_indx, R2, N, dP, tr, a, b, prior, dg, B);
        }
        HIP_TRY(c, hipMemcpyAsync(grad, dg, (size_t)B * P * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(c, hipStreamSynchronize(s));          // the one synchronisation of the evaluation
    NMGP_TRY(nmgp_take_launch_error(c));
    for (int z_ = 0; z_ < B; ++z_) {
        int st = hi[z_];
        double* o = out5 + (size_t)z_ * 5;
        for (int k = 0; k < 5; ++k) o[k] = hs[(size_t)z_ * 16 + 8 + k];
        // a parameter vector that is not finite has no leading minor to blame: NMGP_NUM_NAN whatever pivot met the NaN first
        bool finite_in = true;
        for (size_t k = 0; k < P && finite_in; ++k) finite_in = std::isfinite(pars[(size_t)z_ * P + k]);
        if (!finite_in || (st == 0 && (!std::isfinite(o[0]) || !std::isfinite(o[1])))) st = NMGP_NUM_NAN;
        if (st != 0) {
            for (int k = 0; k < 5; ++k) o[k] = std::nan("");
            if (want_grad) std::fill(grad + (size_t)z_ * P, grad + (size_t)(z_ + 1) * P, 0.0);
        }
        status[z_] = st;
    }
    return 0;
}

}  // namespace

// B chains of the resident Hadamard subject: pars [B, P] -> out5 [B, 5] (the verbose tuples), grad [B, P] = d NegLog / d pars or
// NULL, status [B] (0, a leading-minor index, NMGP_NUM_NAN; a failing chain has a NaN row, a zero gradient row, and does not fail
// the call).  The workspace is the entry's own, evaluated in chunks of chains below NMGP_HAD_BATCH_SLAB_GB (default 96).
extern "C" int nmgp_had_batch_eval(nmgp_ctx* c, const double* pars, int B, const double hyper[8], int prior, double* out5,
                                   double* grad, int* status) {
    if (!c) return NMGP_E_NULL;
    if (!pars || !hyper || !out5 || !status) return nmgp_fail(c, NMGP_E_NULL, "pars/hyper/out5/status must not be NULL");
    if (B <= 0) return nmgp_fail(c, NMGP_E_SHAPE, "B must be positive");
    NMGP_TRY(require_had(c));
    HIP_TRY(c, hipSetDevice(c->device));
    const int N = c->N, M = c->M, T = c->T;
    const size_t P = (size_t)N * (1 + T) + 1;
    const bool want_grad = grad != nullptr;
    double cap_gb = 96.0;
    if (const char* e = std::getenv("NMGP_HAD_BATCH_SLAB_GB")) cap_gb = std::max(1.0, std::atof(e));
    const size_t per_chain = had_layout(1, N, M, T, want_grad).total * sizeof(double);
    int Bc = (int)std::min<double>((double)B, std::floor(cap_gb * 1e9 / (double)per_chain));
    Bc = std::min(Bc, 65535);                      // the chain is a grid dimension
    if (Bc < 1)
        return nmgp_fail(c, NMGP_E_SHAPE, "one chain of the Hadamard model at N = %d needs %.1f GB of device workspace, above the "
                         "NMGP_HAD_BATCH_SLAB_GB cap of %.0f GB", N, per_chain / 1e9, cap_gb);
    for (int b0 = 0; b0 < B; b0 += Bc) {
        const int nb = std::min(Bc, B - b0);
        NMGP_TRY(had_batch_core(c, pars + (size_t)b0 * P, nb, hyper, prior, out5 + (size_t)b0 * 5,
                                want_grad ? grad + (size_t)b0 * P : nullptr, status + b0));
    }
    c->last_kind = 0;
    return 0;
}

// out: [N, N] row-major, the full symmetric S = K_x o (R R^T) + sigma2 I
extern "C" int nmgp_had_covariance(nmgp_ctx* c, const double* pars, double* out) {
    if (!c) return NMGP_E_NULL;
    if (!pars || !out) return nmgp_fail(c, NMGP_E_NULL, "pars/out must not be NULL");
    NMGP_TRY(require_had(c));
    HIP_TRY(c, hipSetDevice(c->device));
    const int N = c->N, M = c->M, T = c->T;
    const size_t P = (size_t)N * (1 + T) + 1;
    hipStream_t s = c->stream;
    const int ld = (int)nmgp_ld((size_t)N);
    double* w;
    NMGP_TRY(nmgp_scratch_get(c, HSL_SLAB, P + 1 + (size_t)N * (1 + M) + 2 + (size_t)ld * N, &w));
    double *dP = w, *ell = dP + ((P + 1) & ~(size_t)1), *Rv = ell + N, *S = Rv + (((size_t)N * M + 1) & ~(size_t)1);
    HIP_TRY(c, hipMemcpyAsync(dP, pars, P * sizeof(double), hipMemcpyHostToDevice, s));
    had_prep(s, dP, c->had_indx, N, M, ell, Rv, 1);
    int r = had_cov_build(s, c->d_x, ell, Rv, dP, (long long)P, S, ld, N, M, 1, 0);
    if (r) return nmgp_fail(c, r, "unsupported number of outputs M=%d", M);
    fill_lower_to_full(s, S, ld, N);
    HIP_TRY(c, hipMemcpy2DAsync(out, (size_t)N * sizeof(double), S, (size_t)ld * sizeof(double), (size_t)N * sizeof(double), (size_t)N,
                                hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    return nmgp_take_launch_error(c);
}

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
    if (pl != pL) NMGP_TRY(nmgp_ps_project(c, pL, d_xs, S, W1, cv + S));
    NMGP_LAUNCH(k_had_star, dim3(S, 1 + T), dim3(256), 0, s, W0, pl != pL ? W1 : W0, dP, N, T, hyper[0], hyper[3], d_star);
    had_prep(s, dP, c->had_indx, N, M, ell, Rv, 1);
    for (int s0 = 0; s0 < S; s0 += smax) {
        const int Sc = std::min(smax, S - s0), E = Sc * M;
        int r = had_cov_build(s, c->d_x, ell, Rv, dP, (long long)P, buf, ld, N, M, 1, 0);
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
