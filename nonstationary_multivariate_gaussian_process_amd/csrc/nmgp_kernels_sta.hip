// Batched pieces of the STATIONARY (LMC) objective for B chains per launch sequence (nmgp_sta_batch_eval; logpos.py:383-462; callers:
// Stationary_model.py, Stationary_model_mpisim.py, Stationary_model_mpiKAISER.py).  Sigma = B kron K_rbf + sigma2 I with the two curves
// of the separable model constant: l = exp(tilde_l), s = exp(tilde_sigma).  The factorisation of the chains' B*M blocks is the
// separable entry's batch; what the constant curves change is everything around it:
//   k_sta_prep_b      yt_p = (V_B^T kron I) y of every chain (no per-location curves to unpack)
//   k_sta_blocks_b4   S_bp = wB_b[p] K_b + sigma2_b I written STRAIGHT from (x, l_b, s_b): the element expression of the Gibbs build
//   (k_sta_blocks_b)  (k_sep_blocks_b) with l_i = l_j, where its sqrt factor is exactly 1; K itself is never stored, not even for the
//                     gradient
//   k_sta_reduce_b    the whole adjoint: ONE pass over the lower triangles of the M blocks -S_bp^-1, K_ij and d_ij recomputed from x
//                     and the chain's two scalars.  With constant curves d loglik / d tilde_l and d loglik / d tilde_sigma are
//                     weighted sums of the per-block numbers <S_p^-1, K o D>, alpha_p^T (K o D) alpha_p, <S_p^-1, K>,
//                     alpha_p^T K alpha_p, so no N x N weighted sum C, no per-location adjoint kernel and no stored K_x are needed
// Every sum is made in a fixed order (per thread in tile order, the workgroup's tree, the host over the column groups in index order):
// no atomics, and nothing depends on what else is in the batch.
#include "nmgp_internal.h"

namespace nmgpk {

static inline int cdiv_t(long long a, long long b) { return (int)((a + b - 1) / b); }

__device__ inline double wave_sum_t(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;
}
// sum over the workgroup's 256 threads in a fixed order; thread 0 holds the total
__device__ inline double block_sum_t(double v, double* sh /*[4]*/) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    v = wave_sum_t(v);
    __syncthreads();
    if (lane == 0) sh[w] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// small[b]: wB [M] | VB row-major [M, M] | sigma2 | l | s | pad  (NMGP_STA_SMALL(M) doubles)
// yt[(b M + p) N + i] = sum_m Y[i, m] VB_b[m, p]
__global__ __launch_bounds__(256) void k_sta_prep_b(const double* __restrict__ Y, const double* __restrict__ small, int small_per, int N,
                                                     int M, double* __restrict__ yt, long long ystride, int cps) {
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (i >= N) return;
    Y += (size_t)(b / cps) * ystride;                  // the chain's subject (stride 0: the resident one)
    const double* VB = small + (size_t)b * small_per + M;
    for (int p = 0; p < M; ++p) {
        double s = 0.0;
        for (int m = 0; m < M; ++m) s += Y[(size_t)i * M + m] * VB[m * M + p];
        yt[((size_t)b * M + p) * N + i] = s;
    }
}

void sta_prep_b(hipStream_t s, const double* Y, const double* small, int small_per, int N, int M, double* yt, int B, long long ystride,
                int cps) {
    NMGP_LAUNCH(k_sta_prep_b, dim3(cdiv_t(N, 256), B), dim3(256), 0, s, Y, small, small_per, N, M, yt, ystride, cps < 1 ? 1 : cps);
}

// Lower triangles of the M blocks of chain b = blockIdx.z: k_sep_blocks_b (64 x 64 location tile per workgroup, lanes along i, the
// XCD-aware tile order, buffer stores with one 32-bit byte offset per element) with scalar curves.  s^2 exp(-d_ij / (l^2 + l^2)) are
// the bits the Gibbs expression (s_i s_j) sqrt(2 l_i l_j / (l_i^2 + l_j^2)) exp(-d_ij / (l_i^2 + l_j^2)) gives for constant curves:
// 2 (l l) and l^2 + l^2 are the same double, so the square root is exactly 1.  Taken for odd N.
template <int M>
__global__ __launch_bounds__(256) void k_sta_blocks_b(const double* __restrict__ x, const double* __restrict__ small, int small_per, int N,
                                                       double* __restrict__ S, int ldo, long long bstride, long long xstride, int cps) {
    constexpr int TJ = 64;
    __shared__ double sx[TJ];
    const int b = blockIdx.z;
    x += (size_t)(b / cps) * xstride;                  // the chain's subject (stride 0: the resident one)
    const int NI = (N + 63) / 64, ntl = NI * (NI + 1) / 2, per = (ntl + 7) / 8;
    const int g = blockIdx.x, t = (g & 7) * per + (g >> 3);
    if ((g >> 3) >= per || t >= ntl) return;
    int rem = t, J = 0;
    while (rem >= NI - J) {
        rem -= NI - J;
        ++J;
    }
    const int I = J + rem;
    const double* sm = small + (size_t)b * small_per;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int j0 = J * TJ;
    if (tid < TJ) {
        const int j = j0 + tid;
        sx[tid] = (j < N) ? x[j] : 0.0;
    }
    __syncthreads();
    const int i = I * 64 + lane;
    if (i >= N) return;
    double wB[M];
#pragma unroll
    for (int p = 0; p < M; ++p) wB[p] = sm[p];
    const double sigma2 = sm[M + M * M], l = sm[M + M * M + 1], sg = sm[M + M * M + 2];
    const double A = l * l + l * l, s2 = sg * sg;
    const double xi = x[i], xi2 = xi * xi;
    typedef int v2i_t __attribute__((ext_vector_type(2)));
    union D2 {
        double d;
        v2i_t v;
    };
    double* Sb = S + (size_t)b * M * bstride;
    __amdgpu_buffer_rsrc_t rs[M];
#pragma unroll
    for (int p = 0; p < M; ++p) rs[p] = __builtin_amdgcn_make_buffer_rsrc((void*)(Sb + (size_t)p * bstride), 0, 0x7fffffff, 0x00020000);
    for (int jj = 0; jj < TJ / 4; ++jj) {
        const int k = w * (TJ / 4) + jj;
        const int j = j0 + k;
        if (j >= N) break;
        if (i < j) continue;
        const double xj = sx[k];
        const double dist = (xi2 + xj * xj) - 2.0 * (xi * xj);
        double v = s2 * exp(-dist / A);
        if (i == j) v = NMGP_JITTER + v;
        const int off = (j * ldo + i) * 8;                                       // bytes within a block: < 2^31 up to n = 11,584
        const double dg = (i == j) ? sigma2 : 0.0;
        D2 u;
#pragma unroll
        for (int p = 0; p < M; ++p) {
            u.d = wB[p] * v + dg;
            __builtin_amdgcn_raw_buffer_store_b64(u.v, rs[p], off, 0, 0);
        }
    }
}

// The same blocks from 128 x 32 location tiles (k_sep_blocks_b4 with scalar curves): a lane owns the row pair (i, i + 1), every store
// instruction of a wave writes one kilobyte of a column.  Even N only; row pairs that straddle the diagonal are written whole (the
// element above the diagonal is scratch to every consumer).
template <int M>
__global__ __launch_bounds__(256) void k_sta_blocks_b4(const double* __restrict__ x, const double* __restrict__ small, int small_per, int N,
                                                        double* __restrict__ S, int ldo, long long bstride, long long xstride, int cps) {
    constexpr int TJ = 32, TI = 128;
    __shared__ double sx[TJ];
    const int b = blockIdx.z;
    x += (size_t)(b / cps) * xstride;
    const int NI = (N + TI - 1) / TI, NJ = (N + TJ - 1) / TJ;
    // lower-triangular tile list, column by column: column J holds the row tiles I = J / 4 .. NI - 1
    int ntl = 0;
    for (int J = 0; J < NJ; ++J) ntl += NI - J / 4;
    const int per = (ntl + 7) / 8;
    const int g = blockIdx.x, t = (g & 7) * per + (g >> 3);
    if ((g >> 3) >= per || t >= ntl) return;
    int rem = t, J = 0;
    while (rem >= NI - J / 4) {
        rem -= NI - J / 4;
        ++J;
    }
    const int I = J / 4 + rem;
    const double* sm = small + (size_t)b * small_per;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int j0 = J * TJ;
    if (tid < TJ) {
        const int j = j0 + tid;
        sx[tid] = (j < N) ? x[j] : 0.0;
    }
    __syncthreads();
    const int i = I * TI + 2 * lane;                   // rows i, i + 1 (N even: both valid or both out)
    if (i >= N) return;
    double wB[M];
#pragma unroll
    for (int p = 0; p < M; ++p) wB[p] = sm[p];
    const double sigma2 = sm[M + M * M], l = sm[M + M * M + 1], sg = sm[M + M * M + 2];
    const double A = l * l + l * l, s2 = sg * sg;
    const double xa = x[i], xb = x[i + 1];
    const double xa2 = xa * xa, xb2 = xb * xb;
    typedef int v4i_t __attribute__((ext_vector_type(4)));
    union D4 {
        double d[2];
        v4i_t v;
    };
    double* Sb = S + (size_t)b * M * bstride;
    __amdgpu_buffer_rsrc_t rs[M];
#pragma unroll
    for (int p = 0; p < M; ++p) rs[p] = __builtin_amdgcn_make_buffer_rsrc((void*)(Sb + (size_t)p * bstride), 0, 0x7fffffff, 0x00020000);
    for (int jj = 0; jj < TJ / 4; ++jj) {
        const int k = w * (TJ / 4) + jj;
        const int j = j0 + k;
        if (j >= N) break;
        if (i + 1 < j) continue;                       // the whole pair lies above the diagonal
        const double xj = sx[k], xj2 = xj * xj;
        const double da = (xa2 + xj2) - 2.0 * (xa * xj);
        const double db = (xb2 + xj2) - 2.0 * (xb * xj);
        double va = s2 * exp(-da / A);
        double vb = s2 * exp(-db / A);
        if (i == j) va = NMGP_JITTER + va;
        if (i + 1 == j) vb = NMGP_JITTER + vb;
        const int off = (j * ldo + i) * 8;
        const double ga = (i == j) ? sigma2 : 0.0, gb = (i + 1 == j) ? sigma2 : 0.0;
        D4 u;
#pragma unroll
        for (int p = 0; p < M; ++p) {
            u.d[0] = wB[p] * va + ga;
            u.d[1] = wB[p] * vb + gb;
            __builtin_amdgcn_raw_buffer_store_b128(u.v, rs[p], off, 0, 0);
        }
    }
}

template <int M>
static void launch_sta_blocks_b(hipStream_t s, const double* x, const double* small, int small_per, int N, double* S, int ldo,
                                long long bstride, int B, long long xstride, int cps) {
    if ((N & 1) == 0) {
        const int NI = cdiv_t(N, 128), NJ = cdiv_t(N, 32);
        int ntl = 0;
        for (int J = 0; J < NJ; ++J) ntl += NI - J / 4;
        NMGP_LAUNCH((k_sta_blocks_b4<M>), dim3(8 * ((ntl + 7) / 8), 1, B), dim3(256), 0, s, x, small, small_per, N, S, ldo, bstride, xstride,
                    cps);
    } else {
        const int NI = cdiv_t(N, 64), ntl = NI * (NI + 1) / 2, per = (ntl + 7) / 8;
        NMGP_LAUNCH((k_sta_blocks_b<M>), dim3(8 * per, 1, B), dim3(256), 0, s, x, small, small_per, N, S, ldo, bstride, xstride, cps);
    }
}

int sta_blocks_b(hipStream_t s, const double* x, const double* small, int small_per, int N, int M, double* S, int ldo, long long bstride,
                 int B, long long xstride, int cps) {
    if (cps < 1) cps = 1;
    NMGP_HADS_SWITCH(M, launch_sta_blocks_b<MM>(s, x, small, small_per, N, S, ldo, bstride, B, xstride, cps));
    return 0;
}

// The adjoint of chain b = blockIdx.y: ONE pass over the lower triangles of its M blocks Cneg_bp = -S_bp^-1 (ld = N).  The lower
// triangle is cut into 64 x 64 tiles, listed column by column (J, then I = J ..); column group cg takes the `per` consecutive tiles
// from cg * per on, so its tiles are vertical neighbours, and workgroup g of the launch is column group (g mod 8) * (G / 8) + g / 8:
// the workgroups that share an XCD (dealt round-robin) walk down adjacent runs of the same columns of tiles, whose x and alpha values
// their L2 keeps.  Within a tile a lane owns a row i (every load of a wave reads 512 contiguous bytes of a column of Cneg), a wave 16
// of the 64 columns; the x and alpha_p values of the tile's columns are in LDS, those of the lane's row in registers, K_ij and d_ij
// are recomputed with the build kernel's expression.  Per (b, p, cg), out[((b M + p) G + cg) 5 + ..]:
//   0 tr S_p^-1   1 <S_p^-1, K>   2 <S_p^-1, K o D>   3 |alpha_p|^2 (cg = 0 only)   4 alpha_p^T (K o D) alpha_p
// (full symmetric inner products from the lower triangle), and xi[(b G + cg) M(M+1)/2 + idx(p, q)] = alpha_p^T K alpha_q, p <= q.
// The host adds the G partials in index order.
template <int M>
__global__ __launch_bounds__(256) void k_sta_reduce_b(const double* __restrict__ Cneg, const double* __restrict__ x,
                                                       const double* __restrict__ alpha, const double* __restrict__ small, int small_per,
                                                       int N, int G, double* __restrict__ out, double* __restrict__ xi, long long xstride,
                                                       int cps) {
    constexpr int NX = M * (M + 1) / 2, TJ = 64;
    __shared__ double sx[TJ], sa[M][TJ], sh[4];
    const int g = blockIdx.x, b = blockIdx.y;
    const int cg = (g & 7) * (G >> 3) + (g >> 3);
    x += (size_t)(b / cps) * xstride;                  // the chain's subject (stride 0: the resident one)
    const size_t NN = (size_t)N * N;
    const double* Cb = Cneg + (size_t)b * M * NN;
    const double* Ab = alpha + (size_t)b * M * N;
    const double* sm = small + (size_t)b * small_per;
    const double l = sm[M + M * M + 1], sg = sm[M + M * M + 2];
    const double A = l * l + l * l, s2 = sg * sg;
    const int NI = (N + 63) / 64, ntl = NI * (NI + 1) / 2, per = (ntl + G - 1) / G;
    const int t0 = cg * per, t1 = (t0 + per < ntl) ? t0 + per : ntl;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    double tr[M], tk[M], tkd[M], akd[M], X[NX];
#pragma unroll
    for (int p = 0; p < M; ++p) tr[p] = tk[p] = tkd[p] = akd[p] = 0.0;
#pragma unroll
    for (int e = 0; e < NX; ++e) X[e] = 0.0;
    int J = 0, I = 0;
    if (t0 < t1) {
        int rem = t0;
        while (rem >= NI - J) {
            rem -= NI - J;
            ++J;
        }
        I = J + rem;
    }
    int Jl = -1;                                       // the column of tiles whose x / alpha values are in LDS
    for (int t = t0; t < t1; ++t) {                    // (t0, t1, I, J are uniform over the workgroup: so are the barriers)
        const int j0 = J * TJ;
        if (J != Jl) {
            __syncthreads();
            if (tid < TJ) {
                const int j = j0 + tid;
                sx[tid] = (j < N) ? x[j] : 0.0;
#pragma unroll
                for (int p = 0; p < M; ++p) sa[p][tid] = (j < N) ? Ab[(size_t)p * N + j] : 0.0;
            }
            __syncthreads();
            Jl = J;
        }
        const int i = I * 64 + lane;
        if (i < N) {
            const double xi_ = x[i], xi2 = xi_ * xi_;
            double ai[M];
#pragma unroll
            for (int p = 0; p < M; ++p) ai[p] = Ab[(size_t)p * N + i];
            for (int jj = 0; jj < TJ / 4; ++jj) {
                const int k = w * (TJ / 4) + jj;
                const int j = j0 + k;
                if (j >= N) break;
                if (i < j) continue;
                const double xj = sx[k];
                const double dist = (xi2 + xj * xj) - 2.0 * (xi_ * xj);
                double kv = s2 * exp(-dist / A);
                const size_t o = (size_t)j * N + i;
                if (i == j) {
                    kv = NMGP_JITTER + kv;
#pragma unroll
                    for (int p = 0; p < M; ++p) {
                        const double c = -Cb[(size_t)p * NN + o];
                        tr[p] += c;
                        tk[p] += c * kv;
                    }
                    int e = 0;
#pragma unroll
                    for (int p = 0; p < M; ++p) {
#pragma unroll
                        for (int q = p; q < M; ++q) {
                            X[e] = fma(kv, ai[p] * ai[q], X[e]);
                            ++e;
                        }
                    }
                } else {
                    const double kd = kv * dist;
#pragma unroll
                    for (int p = 0; p < M; ++p) {
                        const double c = -Cb[(size_t)p * NN + o];
                        tk[p] += 2.0 * c * kv;
                        tkd[p] += 2.0 * c * kd;
                        akd[p] = fma(kd, 2.0 * (ai[p] * sa[p][k]), akd[p]);
                    }
                    int e = 0;
#pragma unroll
                    for (int p = 0; p < M; ++p) {
#pragma unroll
                        for (int q = p; q < M; ++q) {
                            X[e] = fma(kv, ai[p] * sa[q][k] + sa[p][k] * ai[q], X[e]);
                            ++e;
                        }
                    }
                }
            }
        }
        if (++I >= NI) {
            ++J;
            I = J;
        }
    }
#pragma unroll
    for (int p = 0; p < M; ++p) {
        double aa = 0.0;
        if (cg == 0) {
            const double* ap = Ab + (size_t)p * N;
            for (int i = tid; i < N; i += 256) aa += ap[i] * ap[i];
        }
        const double v0 = block_sum_t(tr[p], sh), v1 = block_sum_t(tk[p], sh), v2 = block_sum_t(tkd[p], sh);
        const double v3 = block_sum_t(aa, sh), v4 = block_sum_t(akd[p], sh);
        if (tid == 0) {
            double* o = out + (((size_t)b * M + p) * G + cg) * 5;
            o[0] = v0;
            o[1] = v1;
            o[2] = v2;
            o[3] = v3;
            o[4] = v4;
        }
    }
#pragma unroll
    for (int e = 0; e < NX; ++e) {
        const double v = block_sum_t(X[e], sh);
        if (tid == 0) xi[((size_t)b * G + cg) * NX + e] = v;
    }
}

// out: B * M * G * 5 doubles, xi: B * G * M (M + 1) / 2 doubles; G a multiple of 8
int sta_reduce_b(hipStream_t s, const double* Cneg, const double* x, const double* alpha, const double* small, int small_per, int N, int M,
                 int G, double* out, double* xi, int B, long long xstride, int cps) {
    if (cps < 1) cps = 1;
    NMGP_HADS_SWITCH(M, NMGP_LAUNCH((k_sta_reduce_b<MM>), dim3(G, B), dim3(256), 0, s, Cneg, x, alpha, small, small_per, N, G, out, xi,
                                    xstride, cps));
    return 0;
}

}  // namespace nmgpk
