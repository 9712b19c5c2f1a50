// The three Hadamard models (nmgp_hadamard.hip nonseparable, nmgp_hadamard_sep.hip separable, nmgp_hadamard_sta.hip stationary)
// share ONE host schedule of a batched evaluation and ONE pair of Gibbs kernels.  This header holds both.
//
// Host skeleton: had_batch_eval<Model> (argument checks, workspace cap, chunk loop) -> had_eval_chunk<Model> (upload, factorise,
// reduce, read back, solve, inverse, trace, ONE synchronisation, status) and had_covariance<Model>.  A Model is a struct of static
// members, nothing virtual:
//   WIDTH                 entries of the verbose tuple (the out5 / out6 of the C ABI)
//   NOUN                  the model's name in the workspace-cap message
//   GP_PRIORS             true: the two cached GP-prior factors are resolved and the prior stream is forked for the chunk
//   P(N, T)               length of a parameter vector
//   part_width(M)         components of an adjoint partial row
//   extras(L, take, ...)  the model's own pieces of the workspace (the o_* fields of HadLayout below the common ones)
//   build_cov(k)          hook: parameter unpacking + the covariance launch (lower triangle of every chain's S)
//   value_epilogue(k)     hook: whatever stands between log det / quadratic form and the verbose tuple in scal[8 ..]
//   adjoint_grad(k)       hook: adjoint kernel + final gradient into the o_grad piece
// Every hook receives the chunk (HadChunk) and returns 0 or an error code.
//
// Kernels: k_gibbs_cov<M, AMP> / k_gibbs_adjoint<M, AMP> with their launchers; AMP = false is the nonseparable model (unit
// amplitude), AMP = true the separable one (K_x carries s_i s_j).  A 64 x 64 tile of observations per 256-thread workgroup, lanes
// along i (a wave stores / loads 512 contiguous bytes of one column), the j side staged in LDS, blockIdx.z = chain; fixed summation
// order and no atomics, so B chains in one launch give the bits of B launches.  Below them: the masked pair of the cohort of ragged
// subjects, k_hadc_cov<M, AMP> / k_hadc_adjoint<M, AMP> (the same kernels with the subject's size from a device table; its host
// skeleton is in nmgp_hadamard_cohort_models.hip), and hadst_bf / hadst_stage, the staging of the stationary model's kernels.
#pragma once

#include "nmgp_internal.h"

#include <algorithm>
#include <optional>

// ---- the Gibbs kernels ---------------------------------------------------------------------------------------------------------

// S[i, j] = (K0(i, j) + jitter d_ij) <r_i, r_j> + sigma2 d_ij, lower triangle, column-major with leading dimension ld;
// K0 = [s_i s_j] sqrt(2 l_i l_j / A) exp(-d_ij / A), A = l_i^2 + l_j^2 (kernels.py:46-73; the bracket with AMP only)
template <int M, bool AMP>
__global__ __launch_bounds__(256) void k_gibbs_cov(const double* __restrict__ x, const double* __restrict__ ell,
                                                    const double* __restrict__ sig, const double* __restrict__ Rv,
                                                    const double* __restrict__ pars, long long P, double* __restrict__ S, int ld,
                                                    int N, long long sstride) {
    constexpr int TJ = 64;
    __shared__ double sx[TJ], sl[TJ], ss[AMP ? TJ : 1], sR[TJ * M];
    const int I = blockIdx.x, J = blockIdx.y;
    if (I < J) return;
    ell += (size_t)blockIdx.z * N;
    if constexpr (AMP) sig += (size_t)blockIdx.z * N;
    Rv += (size_t)blockIdx.z * N * M;
    pars += (size_t)blockIdx.z * P;
    S += (size_t)blockIdx.z * sstride;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int j0 = J * TJ;
    if (tid < TJ) {
        const int j = j0 + tid;
        sx[tid] = (j < N) ? x[j] : 0.0;
        sl[tid] = (j < N) ? ell[j] : 1.0;
        if constexpr (AMP) ss[tid] = (j < N) ? sig[j] : 1.0;
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
    [[maybe_unused]] double si = 0.0;
    if constexpr (AMP) si = sig[i];
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
        double kv;                                               // kernels.py:70-72
        if constexpr (AMP) kv = (si * ss[k]) * sqrt(2.0 * (li * lj) / A) * exp(-dist / A);
        else kv = sqrt(2.0 * (li * lj) / A) * exp(-dist / A);
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
//   G = 1/2 (alpha alpha^T - S^-1),  K0 as above (no jitter),  K_x = K0 + jitter I
//   d loglik / d tilde_l_i     = sum_{j != i} 2 G_ij K0[i, j] <r_i, r_j> (1/2 - l_i^2 / A + 2 l_i^2 d_ij / A^2)
//   d loglik / d tilde_sigma_i = sum_j 2 G_ij K0[i, j] <r_i, r_j>                                   (j = i included; AMP only)
//   row component m of i       = sum_j 2 G_ij K_x[i, j] r_j[m]                                      (j = i included)
// Each wave takes 16 j; the four waves' sums meet in LDS and leave part[J][i][0 .. W), W = M + 1 or M + 2: slot 0 = tilde_l,
// (AMP: slot 1 = tilde_sigma,) then the M row components.  The per-chain stride of part is gridDim.y * N * W.
template <int M, bool AMP>
__global__ __launch_bounds__(256) void k_gibbs_adjoint(const double* __restrict__ x, const double* __restrict__ ell,
                                                        const double* __restrict__ sig, const double* __restrict__ Rv,
                                                        const double* __restrict__ alpha, const double* __restrict__ Sneg, int ld,
                                                        int N, double* __restrict__ part) {
    constexpr int TJ = 64, R0 = AMP ? 2 : 1, W = M + R0;
    __shared__ double sx[TJ], sl[TJ], ss[AMP ? TJ : 1], sR[TJ * M], sa[TJ];
    __shared__ double red[2][4][64];
    const int I = blockIdx.x, J = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int j0 = J * TJ;
    const size_t Ns = (size_t)N;
    {   // blockIdx.z = chain
        const size_t z = blockIdx.z;
        ell += z * Ns;
        if constexpr (AMP) sig += z * Ns;
        Rv += z * Ns * M;
        alpha += z * Ns;
        Sneg += z * (size_t)ld * Ns;
        part += z * (size_t)gridDim.y * Ns * W;
    }
    if (tid < TJ) {
        const int j = j0 + tid;
        sx[tid] = (j < N) ? x[j] : 0.0;
        sl[tid] = (j < N) ? ell[j] : 1.0;
        if constexpr (AMP) ss[tid] = (j < N) ? sig[j] : 1.0;
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
    const double xi = x[ic], li = ell[ic];
    [[maybe_unused]] double si = 0.0;
    if constexpr (AMP) si = sig[ic];
    const double ai = alpha[ic];
    const double xi2 = xi * xi, li2 = li * li;
    double ri[M], acc[W];
#pragma unroll
    for (int m = 0; m < M; ++m) ri[m] = Rv[(size_t)ic * M + m];
#pragma unroll
    for (int t = 0; t < W; ++t) acc[t] = 0.0;
    if (iv) {
        for (int jj = 0; jj < TJ / 4; ++jj) {
            const int k = w * (TJ / 4) + jj;
            const int j = j0 + k;
            if (j >= N) break;
            const double xj = sx[k], lj = sl[k];
            const double dist = (xi2 + xj * xj) - 2.0 * (xi * xj);
            const double A = li2 + lj * lj;
            double k0;
            if constexpr (AMP) k0 = (si * ss[k]) * sqrt(2.0 * (li * lj) / A) * exp(-dist / A);
            else k0 = sqrt(2.0 * (li * lj) / A) * exp(-dist / A);
            const double kx = (i == j) ? (NMGP_JITTER + k0) : k0;
            const double G = 0.5 * (ai * sa[k] + Sneg[(size_t)j * ld + i]);
            const double gk = 2.0 * kx * G;
            double dot = 0.0;
#pragma unroll
            for (int m = 0; m < M; ++m) {
                const double rj = sR[k * M + m];
                acc[R0 + m] = fma(gk, rj, acc[R0 + m]);
                dot = fma(ri[m], rj, dot);
            }
            const double gd = 2.0 * (G * dot) * k0;
            if constexpr (AMP) acc[1] += gd;
            if (i != j) {
                const double dlogk = 0.5 - li2 / A + 2.0 * li2 * dist / (A * A);
                acc[0] = fma(gd, dlogk, acc[0]);
            }
        }
    }
    double* o = part + ((size_t)J * Ns + ic) * W;
#pragma unroll
    for (int t = 0; t < W; ++t) {
        red[t & 1][w][lane] = acc[t];
        __syncthreads();
        if (w == 0 && iv) o[t] = (red[t & 1][0][lane] + red[t & 1][1][lane]) + (red[t & 1][2][lane] + red[t & 1][3][lane]);
    }
}

// launchers of the pair; `sig` is not read without AMP (pass nullptr).  NMGP_E_UNSUPPORTED for M outside 1 .. 8.
template <bool AMP>
int gibbs_cov_build(hipStream_t s, const double* x, const double* ell, const double* sig, const double* Rv, const double* pars,
                    long long P, double* S, int ld, int N, int M, int batch, long long sstride) {
    const dim3 grid((unsigned)((N + 63) / 64), (unsigned)((N + 63) / 64), batch);
    NMGP_HADS_SWITCH(M, NMGP_LAUNCH((k_gibbs_cov<MM, AMP>), grid, dim3(256), 0, s, x, ell, sig, Rv, pars, P, S, ld, N, sstride));
    return 0;
}

template <bool AMP>
int gibbs_adjoint(hipStream_t s, const double* x, const double* ell, const double* sig, const double* Rv, const double* alpha,
                  const double* Sneg, int ld, int N, int M, double* part, int batch) {
    const dim3 grid((unsigned)((N + 63) / 64), (unsigned)((N + 63) / 64), batch);      // -S^-1 of chain z: ld x N doubles further on
    NMGP_HADS_SWITCH(M, NMGP_LAUNCH((k_gibbs_adjoint<MM, AMP>), grid, dim3(256), 0, s, x, ell, sig, Rv, alpha, Sneg, ld, N, part));
    return 0;
}

// ---- the masked Gibbs kernels of the cohort (ragged subjects padded to Nmax, nmgp_hadamard_cohort.hip) ---------------------------
// The resident pair above is shared by entries whose bits and register budgets are pinned, so no mask is threaded through it; this
// pair keeps its tile shape, lane mapping, LDS staging, expression order and its handling of AMP, so that a subject with N_s = Nmax
// gets the resident path's bits.  blockIdx.z = chain, subject = chain / cps of the chunk, N_s = nobs[subject]: every mask comes from
// the device table of the subjects' sizes, never from the contents of a padded slot.

// k_gibbs_cov on the real observations, delta_ij on the padded ones: the whole Nmax x Nmax lower triangle.  There i >= j, so a real
// row has real columns only and the mask is the row's.  A tile whose rows are all padded stores and does nothing else.
template <int M, bool AMP>
__global__ __launch_bounds__(256) void k_hadc_cov(const double* __restrict__ x, const double* __restrict__ ell,
                                                   const double* __restrict__ sig, const double* __restrict__ Rv,
                                                   const double* __restrict__ pars, long long P, const int* __restrict__ nobs, int cps,
                                                   double* __restrict__ S, int ld, int N, long long sstride) {
    constexpr int TJ = 64;
    __shared__ double sx[TJ], sl[TJ], ss[AMP ? TJ : 1], sR[TJ * M];
    const int I = blockIdx.x, J = blockIdx.y;
    if (I < J) return;
    const int sub = blockIdx.z / cps;
    const int Ns = nobs[sub];
    x += (size_t)sub * N;
    ell += (size_t)blockIdx.z * N;
    if constexpr (AMP) sig += (size_t)blockIdx.z * N;
    Rv += (size_t)blockIdx.z * N * M;
    pars += (size_t)blockIdx.z * P;
    S += (size_t)blockIdx.z * sstride;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int j0 = J * TJ;
    const int i = I * 64 + lane;
    if (I * 64 >= Ns) {                                      // every row of the tile is padded: store only
        if (i >= N) return;
        for (int jj = 0; jj < TJ / 4; ++jj) {
            const int j = j0 + w * (TJ / 4) + jj;
            if (j >= N) break;
            if (i < j) continue;
            S[(size_t)j * ld + i] = (i == j) ? 1.0 : 0.0;
        }
        return;
    }
    if (tid < TJ) {
        const int j = j0 + tid;
        sx[tid] = (j < Ns) ? x[j] : 0.0;
        sl[tid] = (j < Ns) ? ell[j] : 1.0;
        if constexpr (AMP) ss[tid] = (j < Ns) ? sig[j] : 1.0;
    }
    for (int k = tid; k < TJ * M; k += 256) {
        const size_t g = (size_t)j0 * M + k;
        sR[k] = (g < (size_t)Ns * M) ? Rv[g] : 0.0;
    }
    __syncthreads();
    if (i >= N) return;
    const bool real = i < Ns;
    const int ic = real ? i : 0;
    const double sigma2 = exp(pars[P - 1]);
    const double xi = x[ic], li = ell[ic];
    [[maybe_unused]] double si = 0.0;
    if constexpr (AMP) si = sig[ic];
    const double xi2 = xi * xi, li2 = li * li;
    double ri[M];
#pragma unroll
    for (int m = 0; m < M; ++m) ri[m] = Rv[(size_t)ic * M + m];
#pragma unroll 2
    for (int jj = 0; jj < TJ / 4; ++jj) {
        const int k = w * (TJ / 4) + jj;
        const int j = j0 + k;
        if (j >= N) break;
        if (i < j) continue;
        if (!real) {
            S[(size_t)j * ld + i] = (i == j) ? 1.0 : 0.0;
            continue;
        }
        const double xj = sx[k], lj = sl[k];
        const double dist = (xi2 + xj * xj) - 2.0 * (xi * xj);   // kernels.py:20
        const double A = li2 + lj * lj;                          // kernels.py:69
        double kv;                                               // kernels.py:70-72
        if constexpr (AMP) kv = (si * ss[k]) * sqrt(2.0 * (li * lj) / A) * exp(-dist / A);
        else kv = sqrt(2.0 * (li * lj) / A) * exp(-dist / A);
        if (i == j) kv = NMGP_JITTER + kv;                       // kernels.py:64
        double b = 0.0;
#pragma unroll
        for (int m = 0; m < M; ++m) b += ri[m] * sR[k * M + m];
        double v = kv * b;
        if (i == j) v += sigma2;
        S[(size_t)j * ld + i] = v;
    }
}

// k_gibbs_adjoint with j < N_s and i < N_s masks: part[J][i][0 .. W) of the real i, ZERO partial rows of the padded i (every J) and
// of tiles with nothing real, so that the sums over J and over the observations need no mask of their own.
template <int M, bool AMP>
__global__ __launch_bounds__(256) void k_hadc_adjoint(const double* __restrict__ x, const double* __restrict__ ell,
                                                       const double* __restrict__ sig, const double* __restrict__ Rv,
                                                       const double* __restrict__ alpha, const double* __restrict__ Sneg, int ld,
                                                       int N, const int* __restrict__ nobs, int cps, double* __restrict__ part,
                                                       long long pstride) {
    constexpr int TJ = 64, R0 = AMP ? 2 : 1, W = M + R0;
    __shared__ double sx[TJ], sl[TJ], ss[AMP ? TJ : 1], sR[TJ * M], sa[TJ];
    __shared__ double red[2][4][64];
    const int I = blockIdx.x, J = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int j0 = J * TJ;
    const size_t Nl = (size_t)N;
    const int sub = blockIdx.z / cps;
    const int Ns = nobs[sub];
    {   // blockIdx.z = chain
        const size_t z = blockIdx.z;
        x += (size_t)sub * Nl;
        ell += z * Nl;
        if constexpr (AMP) sig += z * Nl;
        Rv += z * Nl * M;
        alpha += z * Nl;
        Sneg += z * (size_t)ld * Nl;
        part += z * (size_t)pstride;
    }
    const int i = I * 64 + lane;
    const bool inN = i < N;
    if (I * 64 >= Ns || j0 >= Ns) {                          // nothing real in the tile: zero partial rows
        if (w == 0 && inN) {
            double* o = part + ((size_t)J * Nl + i) * W;
#pragma unroll
            for (int t = 0; t < W; ++t) o[t] = 0.0;
        }
        return;
    }
    if (tid < TJ) {
        const int j = j0 + tid;
        sx[tid] = (j < Ns) ? x[j] : 0.0;
        sl[tid] = (j < Ns) ? ell[j] : 1.0;
        if constexpr (AMP) ss[tid] = (j < Ns) ? sig[j] : 1.0;
        sa[tid] = (j < Ns) ? alpha[j] : 0.0;
    }
    for (int k = tid; k < TJ * M; k += 256) {
        const size_t g = (size_t)j0 * M + k;
        sR[k] = (g < (size_t)Ns * M) ? Rv[g] : 0.0;
    }
    __syncthreads();
    const bool iv = i < Ns;
    const int ic = iv ? i : Ns - 1;
    const double xi = x[ic], li = ell[ic];
    [[maybe_unused]] double si = 0.0;
    if constexpr (AMP) si = sig[ic];
    const double ai = alpha[ic];
    const double xi2 = xi * xi, li2 = li * li;
    double ri[M], acc[W];
#pragma unroll
    for (int m = 0; m < M; ++m) ri[m] = Rv[(size_t)ic * M + m];
#pragma unroll
    for (int t = 0; t < W; ++t) acc[t] = 0.0;
    if (iv) {
        for (int jj = 0; jj < TJ / 4; ++jj) {
            const int k = w * (TJ / 4) + jj;
            const int j = j0 + k;
            if (j >= Ns) break;
            const double xj = sx[k], lj = sl[k];
            const double dist = (xi2 + xj * xj) - 2.0 * (xi * xj);
            const double A = li2 + lj * lj;
            double k0;
            if constexpr (AMP) k0 = (si * ss[k]) * sqrt(2.0 * (li * lj) / A) * exp(-dist / A);
            else k0 = sqrt(2.0 * (li * lj) / A) * exp(-dist / A);
            const double kx = (i == j) ? (NMGP_JITTER + k0) : k0;
            const double G = 0.5 * (ai * sa[k] + Sneg[(size_t)j * ld + i]);
            const double gk = 2.0 * kx * G;
            double dot = 0.0;
#pragma unroll
            for (int m = 0; m < M; ++m) {
                const double rj = sR[k * M + m];
                acc[R0 + m] = fma(gk, rj, acc[R0 + m]);
                dot = fma(ri[m], rj, dot);
            }
            const double gd = 2.0 * (G * dot) * k0;
            if constexpr (AMP) acc[1] += gd;
            if (i != j) {
                const double dlogk = 0.5 - li2 / A + 2.0 * li2 * dist / (A * A);
                acc[0] = fma(gd, dlogk, acc[0]);
            }
        }
    }
    double* o = part + ((size_t)J * Nl + (inN ? i : 0)) * W;
#pragma unroll
    for (int t = 0; t < W; ++t) {
        red[t & 1][w][lane] = acc[t];
        __syncthreads();
        // (a padded i < Nmax has four zero accumulators: its row is written as +0.0)
        if (w == 0 && inN) o[t] = (red[t & 1][0][lane] + red[t & 1][1][lane]) + (red[t & 1][2][lane] + red[t & 1][3][lane]);
    }
}

// launchers of the masked pair (x: the chunk's first subject's row of the [S, Nmax] table; `sig` as above)
template <bool AMP>
int hadc_cov_build(hipStream_t s, const double* x, const double* ell, const double* sig, const double* Rv, const double* pars,
                   long long P, const int* nobs, int cps, double* S, int ld, int N, int M, int batch, long long sstride) {
    const dim3 grid((unsigned)((N + 63) / 64), (unsigned)((N + 63) / 64), batch);
    NMGP_HADS_SWITCH(M, NMGP_LAUNCH((k_hadc_cov<MM, AMP>), grid, dim3(256), 0, s, x, ell, sig, Rv, pars, P, nobs, cps, S, ld, N, sstride));
    return 0;
}

template <bool AMP>
int hadc_adjoint(hipStream_t s, const double* x, const double* ell, const double* sig, const double* Rv, const double* alpha,
                 const double* Sneg, int ld, int N, int M, const int* nobs, int cps, double* part, long long pstride, int batch) {
    const dim3 grid((unsigned)((N + 63) / 64), (unsigned)((N + 63) / 64), batch);
    NMGP_HADS_SWITCH(M, NMGP_LAUNCH((k_hadc_adjoint<MM, AMP>), grid, dim3(256), 0, s, x, ell, sig, Rv, alpha, Sneg, ld, N, nobs, cps, part,
                                    pstride));
    return 0;
}

// Whether the REAL slots of a cohort parameter vector are finite (N = the set's Nmax, Ns = the subject's size): the range of the
// NMGP_NUM_NAN test of the cohort's evaluation and prediction entries, per model.
inline bool hadc_finite_non(const double* p, size_t N, size_t Ns, int T) {       // [tilde_l (N) | L_vecs (N T) | tilde_sigma2_err]
    if (!std::isfinite(p[N * (1 + T)])) return false;
    for (size_t t = 0; t < Ns; ++t)
        if (!std::isfinite(p[t])) return false;
    for (size_t t = 0; t < Ns * T; ++t)
        if (!std::isfinite(p[N + t])) return false;
    return true;
}
inline bool hadc_finite_sep(const double* p, size_t N, size_t Ns, int T) {       // [tilde_l (N) | tilde_sigma (N) | L_vec (T) | s2e]
    for (size_t t = 0; t < Ns; ++t)
        if (!std::isfinite(p[t]) || !std::isfinite(p[N + t])) return false;
    for (size_t t = 2 * N; t < 2 * N + T + 1; ++t)
        if (!std::isfinite(p[t])) return false;
    return true;
}
inline bool hadc_finite_sta(const double* p, size_t, size_t, int T) {            // all T + 3 slots: no per-observation part
    for (int t = 0; t < T + 3; ++t)
        if (!std::isfinite(p[t])) return false;
    return true;
}

// ---- device helpers of the stationary model's kernels (k_hadst_* of nmgp_hadamard_sta.hip, k_hadcst_* of the cohort) -----------------

// B_f[a, b] = <row a of L, row b of L> of the packed lower triangle Lvec
template <int M>
__device__ inline double hadst_bf(const double* __restrict__ Lvec, int a, int b) {
    const int lo = a < b ? a : b;
    double acc = 0.0;
#pragma unroll
    for (int m = 0; m < M; ++m)
        if (m <= lo) acc += Lvec[a * (a + 1) / 2 + m] * Lvec[b * (b + 1) / 2 + m];
    return acc;
}

// The chain's scalars, once per workgroup: sp = {l, s2, sigma2_err}, sB = B_f [M, M]; and the j side of the tile: su = x_j / l and
// sc = c_j for j < nreal (the resident kernels pass N, the cohort's the subject's N_s), 0 beyond.  The caller synchronises.
template <int M>
__device__ inline void hadst_stage(const double* __restrict__ pars, long long P, const double* __restrict__ x,
                                   const int* __restrict__ indx, int nreal, int j0, double* sp, double* sB, double* su, int* sc) {
    const int tid = threadIdx.x;
    if (tid < 64) {
        const int j = j0 + tid;
        const double l = exp(pars[0]);
        su[tid] = (j < nreal) ? x[j] / l : 0.0;
        sc[tid] = (j < nreal) ? indx[j] : 0;
        if (tid == 0) {
            const double sg = exp(pars[1]);
            sp[0] = l;
            sp[1] = sg * sg;
            sp[2] = exp(pars[P - 1]);
        }
    } else if (tid - 64 < M * M) {
        const int k = tid - 64;
        sB[k] = hadst_bf<M>(pars + 2, k / M, k % M);
    }
}

// Normal(mean, sd) with Python-number arguments: torch rounds both to float32, squares and takes the logarithm there
struct NormalF32 {
    double mean, var, log_sd;
    NormalF32(double m, double sd) {
        const float m32 = (float)m, s32 = (float)sd;
        mean = (double)m32;
        var = (double)(s32 * s32);
        log_sd = (double)std::log(s32);
    }
};

// ---- the host skeleton ---------------------------------------------------------------------------------------------------------

// device workspace of a chunk of B chains, in doubles (every piece at an even offset)
struct HadLayout {
    size_t o_P = 0, o_z = 0, o_scal = 0, o_info = 0, o_S = 0;
    size_t o_alpha = 0, o_Sneg = 0, o_part = 0, o_grad = 0, o_tr = 0;                      // with gradients only
    size_t o_ell = 0, o_sig = 0, o_Rv = 0, o_R = 0, o_q = 0, o_R2 = 0, o_rsum = 0;         // Model::extras (0: the model has none)
    size_t total = 0;
    size_t part_per = 0;       // per-chain stride of o_part
    int ld = 0, xpad = 0, xoff = 0;
    long long bs = 0;          // per-chain stride of o_S
};

template <class Model>
HadLayout had_layout(int B, int N, int M, int T, bool want_grad) {
    HadLayout L;
    const size_t P = Model::P(N, T), Bs = B, NJ = (N + 63) / 64;
    // rows: N (matrix) + 1 (y); with gradients + pad + N identity rows (-> L^-T)
    L.xpad = (N + 1) & 1;
    L.xoff = N + 1 + L.xpad;
    L.ld = (int)nmgp_ld(want_grad ? (size_t)2 * N + 2 : (size_t)N + 1);
    L.bs = (long long)L.ld * N;
    // adjoint partial rows; before that pass the same buffer holds the block sums of alpha = L^-T z (tri_gemv_upper)
    L.part_per = std::max(NJ * (size_t)N * Model::part_width(M), (size_t)N * ((N + 255) / 256));
    size_t off = 0;
    auto take = [&off](size_t n) { size_t o = off; off += (n + 1) & ~(size_t)1; return o; };
    L.o_P = take(Bs * P); L.o_z = take(Bs * N); L.o_scal = take(Bs * 16); L.o_info = take(Bs);
    Model::extras(L, take, Bs, (size_t)N, M, T, want_grad);
    L.o_S = take(Bs * (size_t)L.bs);
    if (want_grad) {
        L.o_alpha = take(Bs * N); L.o_Sneg = take(Bs * (size_t)N * N); L.o_part = take(Bs * L.part_per);
        L.o_grad = take(Bs * P); L.o_tr = take(Bs * 2);
    }
    L.total = off;
    return L;
}

// what a model hook sees of a chunk
struct HadChunk {
    nmgp_ctx* c;
    const HadLayout& L;
    double* slab;
    int B;
    const double* hyper;
    int prior;
    bool want_grad;
    PriorFactor *p0, *p1;      // GP_PRIORS: the cached factors of hyper[1..2] and hyper[4..5]
    PriorStreamScope* ps;      // GP_PRIORS: the forked prior stream
    double* at(size_t o) const { return slab + o; }
};

// The GP-prior half of a value epilogue, on the forked prior stream: rhs(stream, R) fills R with the nc centred prior columns of
// every chain; then L X = R -> q = column sums of squares (the Mahalanobis terms) -> with gradients and priors R2 = Sigma_prior^-1
// (v - mu).  Enqueued after the factorisation's launches (see svc_enqueue); ends with the join, so the finaliser may follow.
template <class Rhs>
int had_gp_prior_terms(const HadChunk& k, int nc, Rhs rhs) {
    nmgp_ctx* c = k.c;
    PriorStreamScope& ps = *k.ps;
    const int N = c->N, B = k.B;
    double* R = k.at(k.L.o_R);
    {
        NmgpStage sp(c, NMGP_STAGE_PRIOR, ps.sp, 0.0, 0.0);
        rhs(ps.sp, R);
        NMGP_TRY(had_prior_solve(c, ps.sp, ps.hb, false, k.p0, k.p1, R, N, nc - 1, B));
        nmgpk::col_sumsq(ps.sp, R, N, N, B * nc, k.at(k.L.o_q));
        if (k.want_grad && k.prior) {
            double* R2 = k.at(k.L.o_R2);
            HIP_TRY(c, hipMemcpyAsync(R2, R, (size_t)B * N * nc * sizeof(double), hipMemcpyDeviceToDevice, ps.sp));
            NMGP_TRY(had_prior_solve(c, ps.sp, ps.hb, true, k.p0, k.p1, R2, N, nc - 1, B));
        }
    }
    ps.done();
    ps.join();
    return 0;
}

// chains [0, B) of `pars` (already offset by the caller): value and gradient halves enqueued back to back, ONE synchronisation
template <class Model>
int had_eval_chunk(nmgp_ctx* c, const double* pars, int B, const double* hyper, int prior, double* out, double* grad, int* status) {
    constexpr int W = Model::WIDTH;
    const int N = c->N, M = c->M, T = c->T;
    const size_t P = Model::P(N, T);
    const bool want_grad = grad != nullptr;
    hipStream_t s = c->stream;
    PriorFactor *p0 = nullptr, *p1 = nullptr;
    if constexpr (Model::GP_PRIORS) NMGP_TRY(had_priors(c, hyper, &p0, &p1));
    const HadLayout L = had_layout<Model>(B, N, M, T, want_grad);
    double* slab;
    NMGP_TRY(nmgp_scratch_get(c, HSL_SLAB, L.total, &slab));
    double *dP = slab + L.o_P, *z = slab + L.o_z, *scal = slab + L.o_scal, *S = slab + L.o_S;
    int* info = reinterpret_cast<int*>(slab + L.o_info);
    const int ld = L.ld;
    const long long bs = L.bs;
    HIP_TRY(c, hipMemcpyAsync(dP, pars, (size_t)B * P * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemsetAsync(info, 0, (size_t)B * sizeof(int), s));
    std::optional<PriorStreamScope> ps;          // fork now, enqueue the prior solves after the factorisation's launches
    if constexpr (Model::GP_PRIORS) ps.emplace(c);
    const HadChunk k{c, L, slab, B, hyper, prior, want_grad, p0, p1, ps ? &*ps : nullptr};
    {
        NmgpStage sp(c, NMGP_STAGE_COV);
        int r = Model::build_cov(k);
        if (r) return nmgp_fail(c, r, "unsupported number of outputs M=%d", M);
    }
    {
        NmgpStage sp(c, NMGP_STAGE_CHOL);
        nmgpk::set_row(s, S, ld, N, c->had_y, N, B, bs, 0);                // y rides along as row N (shared by the chains)
        if (want_grad) nmgpk::identity_rows(s, S, ld, N + 1, N, L.xpad, B, bs);
        nmgp_potrf(c, S, ld, N, want_grad ? 1 + L.xpad : 1, want_grad ? N : 0, info, B, bs, 1);
        nmgpk::get_row(s, S, ld, N, z, N, B, bs, N);                       // z = L^-1 y
    }
    {
        NmgpStage sp(c, NMGP_STAGE_REDUCE);
        nmgpk::chol_logdet_quad(s, S, ld, N, z, scal, scal + 1, B, bs, 16);
        if constexpr (!Model::GP_PRIORS) NMGP_TRY(Model::value_epilogue(k));     // the finaliser alone: in this stage
    }
    if constexpr (Model::GP_PRIORS) NMGP_TRY(Model::value_epilogue(k));          // prior stream, join, finaliser (a stage of its own)
    std::vector<double> hs((size_t)B * 16);
    std::vector<int> hi(B);
    HIP_TRY(c, hipMemcpyAsync(hs.data(), scal, hs.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(hi.data(), info, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, s));
    if (want_grad) {
        // enqueued behind the value half without waiting for it (a chain that failed produces garbage here, which the epilogue discards)
        double *alpha = slab + L.o_alpha, *Sneg = slab + L.o_Sneg, *part = slab + L.o_part;
        {
            NmgpStage sp(c, NMGP_STAGE_SOLVE);
            nmgpk::tri_gemv_upper(s, S + L.xoff, ld, N, z, alpha, part, B, bs, (long long)L.part_per);   // alpha = L^-T z = X z
        }
        {
            NmgpStage sp(c, NMGP_STAGE_INVERSE);
            nmgpk::syrk_lower(s, S + L.xoff, ld, Sneg, N, N, N, N, B, bs, (long long)N * N, 2);         // -S^-1 = -X X^T, both triangles
        }
        {
            NmgpStage sp(c, NMGP_STAGE_ADJOINT);
            nmgpk::trace_terms(s, alpha, Sneg, N, N, slab + L.o_tr, -1.0, B);
            int r = Model::adjoint_grad(k);
            if (r) return nmgp_fail(c, r, "unsupported number of outputs M=%d", M);
        }
        HIP_TRY(c, hipMemcpyAsync(grad, slab + L.o_grad, (size_t)B * P * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(c, hipStreamSynchronize(s));          // the one synchronisation of the evaluation
    NMGP_TRY(nmgp_take_launch_error(c));
    for (int z_ = 0; z_ < B; ++z_) {
        int st = hi[z_];
        double* o = out + (size_t)z_ * W;
        for (int t = 0; t < W; ++t) o[t] = hs[(size_t)z_ * 16 + 8 + t];
        // a parameter vector that is not finite has no leading minor to blame: NMGP_NUM_NAN whatever pivot met the NaN first
        bool finite_in = true;
        for (size_t t = 0; t < P && finite_in; ++t) finite_in = std::isfinite(pars[(size_t)z_ * P + t]);
        if (!finite_in || (st == 0 && (!std::isfinite(o[0]) || !std::isfinite(o[1])))) st = NMGP_NUM_NAN;
        if (st != 0) {
            for (int t = 0; t < W; ++t) o[t] = std::nan("");
            if (want_grad) std::fill(grad + (size_t)z_ * P, grad + (size_t)(z_ + 1) * P, 0.0);
        }
        status[z_] = st;
    }
    return 0;
}

// The chunk loop of the resident and the cohort entries: B = S * cps chains in chunks below NMGP_HAD_BATCH_SLAB_GB (default 96, at
// least 1) for `per_chain` bytes of workspace per chain.  A chunk is a whole number of subjects, or a part of ONE subject's chains
// (then every chain of the chunk is that subject's), so that no kernel takes a chain offset; the resident entries are one subject of
// B chains.  eval(b0, nb, s0, cps of the chunk) evaluates chains [b0, b0 + nb), the first of which belongs to subject s0.  `noun`,
// `at` and `n` name the model and its order in the refusal.
template <class Eval>
int had_for_chunks(nmgp_ctx* c, int B, int cps, size_t per_chain, const char* noun, const char* at, int n, Eval eval) {
    double cap_gb = 96.0;
    if (const char* e = std::getenv("NMGP_HAD_BATCH_SLAB_GB")) cap_gb = std::max(1.0, std::atof(e));
    int Bc = (int)std::min<double>((double)B, std::floor(cap_gb * 1e9 / (double)per_chain));
    Bc = std::min(Bc, 65535);                      // the chain is a grid dimension
    if (Bc < 1)
        return nmgp_fail(c, NMGP_E_SHAPE, "one chain of the %s %s = %d needs %.1f GB of device workspace, above the "
                         "NMGP_HAD_BATCH_SLAB_GB cap of %.0f GB", noun, at, n, per_chain / 1e9, cap_gb);
    const bool split = cps > Bc;
    if (!split) Bc = (Bc / cps) * cps;
    for (int b0 = 0; b0 < B;) {
        const int s0 = b0 / cps;
        int nb = std::min(Bc, B - b0);
        if (split) nb = std::min(nb, (s0 + 1) * cps - b0);
        NMGP_TRY(eval(b0, nb, s0, split ? nb : cps));
        b0 += nb;
    }
    return 0;
}

// B chains of the resident Hadamard subject: pars [B, P] -> out [B, WIDTH] (the verbose tuples), grad [B, P] = d NegLog / d pars or
// NULL, status [B] (0, a leading-minor index, NMGP_NUM_NAN; a failing chain has a NaN row, a zero gradient row, and does not fail
// the call).  The workspace is the entry's own, evaluated in chunks of chains below NMGP_HAD_BATCH_SLAB_GB (default 96, at least 1).
template <class Model>
int had_batch_eval(nmgp_ctx* c, const double* pars, int B, const double* hyper, int prior, double* out, double* grad, int* status) {
    if (!c) return NMGP_E_NULL;
    if (!pars || !hyper || !out || !status)
        return nmgp_fail(c, NMGP_E_NULL, "pars/hyper/out%d/status must not be NULL", Model::WIDTH);
    if (B <= 0) return nmgp_fail(c, NMGP_E_SHAPE, "B must be positive");
    NMGP_TRY(require_had(c));
    HIP_TRY(c, hipSetDevice(c->device));
    const int N = c->N, M = c->M, T = c->T;
    const size_t P = Model::P(N, T);
    const bool want_grad = grad != nullptr;
    const size_t per_chain = had_layout<Model>(1, N, M, T, want_grad).total * sizeof(double);
    // one "subject" of B chains: one chunk when B fits under the cap, chunks of the cap's chains otherwise
    NMGP_TRY(had_for_chunks(c, B, B, per_chain, Model::NOUN, "model at N", N, [&](int b0, int nb, int, int) {
        return had_eval_chunk<Model>(c, pars + (size_t)b0 * P, nb, hyper, prior, out + (size_t)b0 * Model::WIDTH,
                                     want_grad ? grad + (size_t)b0 * P : nullptr, status + b0);
    }));
    c->last_kind = 0;
    return 0;
}

// out: [N, N] row-major, the full symmetric covariance of one parameter vector.  The workspace is the value half's of one chain (its
// z, scal, info and prior pieces stay unused: a few vectors next to the matrix), so that build_cov finds its pieces where it does in
// an evaluation.
template <class Model>
int had_covariance(nmgp_ctx* c, const double* pars, double* out) {
    if (!c) return NMGP_E_NULL;
    if (!pars || !out) return nmgp_fail(c, NMGP_E_NULL, "pars/out must not be NULL");
    NMGP_TRY(require_had(c));
    HIP_TRY(c, hipSetDevice(c->device));
    const int N = c->N, M = c->M, T = c->T;
    const size_t P = Model::P(N, T);
    hipStream_t s = c->stream;
    HadLayout L = had_layout<Model>(1, N, M, T, false);
    L.ld = (int)nmgp_ld((size_t)N);          // no riding row here: the stride the covariance entries have always used
    double* slab;
    NMGP_TRY(nmgp_scratch_get(c, HSL_SLAB, L.total, &slab));
    double* S = slab + L.o_S;
    HIP_TRY(c, hipMemcpyAsync(slab + L.o_P, pars, P * sizeof(double), hipMemcpyHostToDevice, s));
    int r = Model::build_cov(HadChunk{c, L, slab, 1, nullptr, 0, false, nullptr, nullptr, nullptr});
    if (r) return nmgp_fail(c, r, "unsupported number of outputs M=%d", M);
    nmgpk::fill_lower_to_full(s, S, L.ld, N);
    HIP_TRY(c, hipMemcpy2DAsync(out, (size_t)N * sizeof(double), S, (size_t)L.ld * sizeof(double), (size_t)N * sizeof(double),
                                (size_t)N, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    return nmgp_take_launch_error(c);
}

