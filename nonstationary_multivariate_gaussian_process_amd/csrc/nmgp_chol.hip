// Custom blocked FP64 Cholesky for gfx950 (replaces rocSOLVER dpotrf on the log-posterior path, which spends
// 20 ms in ~700 tiny launches on a 6144^2 matrix).
//
//   * right-looking, two-level blocking: 64-wide diagonal steps inside NB1-wide outer panels, so that the big
//     trailing update runs with K = NB1 (compute bound) while the panel-internal updates stay narrow;
//   * the right-hand side y rides along as an EXTRA ROW below the matrix (row n of the augmented array):
//     the panel solves and trailing updates turn it into z = L^-1 y, so no separate triangular solve is needed
//     (the reference needs Sigma^-1 y and log det Sigma only: logpos.py:352-354);
//   * k_syrk_lower: C -= A A^T on the lower trapezoid with v_mfma_f64_16x16x4_f64, 128x128 tile per workgroup,
//     4 waves x (4x4) MFMA tiles, k-panels of 16 staged through LDS (double buffered, register prefetch).  The MFMA
//     takes the j-side fragment as its A operand and the i-side fragment as B, so that lanes 0..15 of the result
//     hold 16 consecutive ROWS of C: every store segment is 128 contiguous bytes of a column-major column;
//   * k_potf2_64: one workgroup factors a 64x64 diagonal block held in registers (one barrier per column, the next
//     column is published before the rest of the current column's updates);
//   * look-ahead: the far trailing update runs on a second stream under the next panel's latency-bound steps;
//   * k_trsm_64: X L^T = A for 64 rows per workgroup, four lanes per row with the partial dot products combined by
//     DPP quad permutes (no LDS round trip), rows of A kept in registers.
//
// All matrices column-major, lower triangle; leading dimensions must be even (16-byte vector loads).
#include "nmgp_internal.h"
#include <cstring>

namespace nmgpk {

static inline int cdiv_c(long long a, long long b) { return (int)((a + b - 1) / b); }

typedef double v4d __attribute__((ext_vector_type(4)));

#define SY_BM 128
#define SY_BK 16
#define SY_LD (SY_BM + 16)
#define SY_SB 8          // super-block edge in tiles (XCD-aware order)

// The k-panel prefetch must stay asynchronous: gload() only ISSUES 16-byte loads from clamped (always valid)
// addresses; the zeroing of out-of-range rows / k-columns is applied by sstore(), right before the LDS write, i.e.
// after the MFMAs of the current panel.  Touching the loaded value earlier (a select, or a vector/scalar load pair
// under exec masks) makes hipcc place `s_waitcnt vmcnt(0)` directly behind each load: 8 exposed L2 round trips per
// k-step, which capped this kernel at 60 % MFMA utilisation.
__device__ __forceinline__ int clamp_row_pair(int r, int rows) {
    int rc = r < rows - 1 ? r : rows - 2;
    return rc < 0 ? 0 : rc;
}

// ---------------------------------------------------------------------------------------------
// 64x64 diagonal block: unblocked right-looking Cholesky in LDS, one barrier per column.
// info receives (goff + c + 1) for the first non-positive pivot c (LAPACK convention), left untouched otherwise.
// ---------------------------------------------------------------------------------------------
// reciprocal of a positive double: v_rcp_f64 seed + two Newton steps (about 1 ulp; an IEEE division costs ~3x the
// latency and sits on the critical path of every pivot)
__device__ __forceinline__ double fast_recip(double p) {
    double x = __builtin_amdgcn_rcp(p);
    double e = fma(-p, x, 1.0);
    x = fma(x, e, x);
    e = fma(-p, x, 1.0);
    x = fma(x, e, x);
    return x;
}

// One pivot column of the 64x64 block.  The block is kept UNSCALED: column c holds S[r][c] as it stands when the
// column is finalised and the update is S[r][cc] -= S[r][c] S[cc][c] / S[c][c]; the division by sqrt(pivot) is applied
// once at the end.  Critical path per column = barrier, LDS read, reciprocal, one multiply-add for the NEXT column,
// LDS write: the next column is published before the remaining (register-only) updates of this column are done.
template <int KC, int GC>
__device__ __forceinline__ void potf2_step(double (&a)[16], double (*colbuf)[64], double* pivs, int nb,
                                           int* __restrict__ info, int goff, int r, int g, int tid) {
    constexpr int c = 4 * KC + GC;
    constexpr int NKC = (GC == 3) ? KC + 1 : KC;          // register slot / owner class of column c + 1
    constexpr int NGC = (GC == 3) ? 0 : GC + 1;
    if (c >= nb) return;                                     // uniform
    const double* cb = colbuf[c & 1];
    const double piv = cb[c];
    const double mine = cb[r];
    double t[16];
#pragma unroll
    for (int kk = KC; kk < 16; ++kk) t[kk] = cb[4 * kk + g];
    if (tid == 0) {
        pivs[c] = piv;
        if (!(piv > 0.0)) atomicCAS(info, 0, goff + c + 1);
    }
    const double pinv = fast_recip(piv);
    const double f = mine * pinv;
    if (c + 1 < 64) {
        // next column first: update it, publish it, then the barrier that opens step c + 1
        if (NKC < 16) {
            const int cc = 4 * NKC + g;
            const double upd = fma(-f, t[NKC < 16 ? NKC : 15], a[NKC < 16 ? NKC : 15]);
            const bool on = (g == NGC) && (cc <= r);
            if (NKC < 16) a[NKC < 16 ? NKC : 15] = on ? upd : a[NKC < 16 ? NKC : 15];
            if (g == NGC) colbuf[(c + 1) & 1][r] = a[NKC < 16 ? NKC : 15];
        }
        __syncthreads();
    }
#pragma unroll
    for (int kk = KC; kk < 16; ++kk) {
        const int cc = 4 * kk + g;
        const double upd = fma(-f, t[kk], a[kk]);
        bool on = (kk > KC || g > GC) && (cc <= r);
        if (kk == NKC) on = on && (g != NGC);               // already done above
        a[kk] = on ? upd : a[kk];
    }
}

template <int KC>
__device__ __forceinline__ void potf2_steps4(double (&a)[16], double (*colbuf)[64], double* pivs, int nb,
                                             int* __restrict__ info, int goff, int r, int g, int tid) {
    potf2_step<KC, 0>(a, colbuf, pivs, nb, info, goff, r, g, tid);
    potf2_step<KC, 1>(a, colbuf, pivs, nb, info, goff, r, g, tid);
    potf2_step<KC, 2>(a, colbuf, pivs, nb, info, goff, r, g, tid);
    potf2_step<KC, 3>(a, colbuf, pivs, nb, info, goff, r, g, tid);
}

// The whole factorisation of one 64x64 block by the threads of a workgroup (256 or 512 of them: thread tid acts as
// (r, g) = (tid & 63, (tid >> 6) & 3), so the upper half of a 512-thread workgroup repeats the lower half's work and
// writes identical values).  colbuf / pivs: 3 x 64 doubles of LDS.
__device__ __forceinline__ void potf2_body(double* __restrict__ A, int lda, int nb, int* __restrict__ info, int goff, int tid,
                                           double (*colbuf)[64], double* pivs) {
    // thread (r, g): row r, column class g (wave-uniform); it keeps S[r][4 kk + g], kk = 0..15, in registers.  Columns
    // travel between the waves through a double-buffered LDS column.
    const int r = tid & 63, g = (tid >> 6) & 3;
    double a[16];
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
        const int c = 4 * kk + g;
        double v = (r == c) ? 1.0 : 0.0;
        if (r < nb && c <= r) v = A[(size_t)c * lda + r];
        a[kk] = v;
    }
    if (tid < 64) pivs[tid] = 1.0;
    if (g == 0) colbuf[0][r] = a[0];
    __syncthreads();
#define PF(K) potf2_steps4<K>(a, colbuf, pivs, nb, info, goff, r, g, tid)
    PF(0); PF(1); PF(2); PF(3); PF(4); PF(5); PF(6); PF(7); PF(8); PF(9); PF(10); PF(11); PF(12); PF(13); PF(14); PF(15);
#undef PF
    __syncthreads();
    // scale column c by 1/sqrt(pivot_c): L[r][c] = S[r][c] / sqrt(S[c][c])  (diagonal: sqrt(pivot))
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
        const int c = 4 * kk + g;
        if (r < nb && c <= r) A[(size_t)c * lda + r] = a[kk] * rsqrt(pivs[c]);
    }
}

// ---- fast path of k_syrk_lower: a FULL 128x128 tile, K a multiple of 32, 8 waves of 64 x 32 ------------------------
// On gfx950 the FP64 MFMA competes with every other vector instruction of the SIMD (32 extra v_add_u32 per k-step cost
// 4.3 % in tools/lab/syrk_lab.hip), so the k-loop carries no VALU work at all:
//   * panel loads are buffer loads: uniform descriptor + constant per-lane offset + a scalar offset that advances with k;
//   * the loop is unrolled by two so that the LDS buffer offsets are instruction immediates;
//   * row-PAIRED fragment layout: MFMA tile (2p + s) of the i side covers rows 32p + 2*(lane & 15) + s, so one
//     ds_read_b128 feeds two MFMA operands and every lane owns two consecutive rows of C (16-byte loads / stores of C);
//     the j side is paired the same way;
//   * the accumulators start as -C and the epilogue stores -acc, instead of negating a fragment per k-substep;
//   * no edge masks (the masked generic path below handles partial tiles).
// 68.4 TFLOP/s on the K = 512 trailing update of 32 chains (generic path: 55.1; rocblas_dgemm_strided_batched: 67.1).
typedef double v2d __attribute__((ext_vector_type(2)));
typedef int v4i __attribute__((ext_vector_type(4)));

// Defined next to the diagonal-block kernels below.  Tile (0, 0) of an update holds the NEXT diagonal block of the factorisation
// (the leading 64 x 64 of the updated trapezoid) in the accumulators of two of its waves: instead of storing it, the workgroup
// moves it to LDS (the operand buffers, free after the k-loop: `lds` = 2 x 4608 contiguous doubles) and factors it on the spot
// (potf2b_core_mfma) while the launch's other tiles are still being updated -- the block's own launch (one workgroup per matrix,
// ~20 us with the rest of the chip idle: 48 of them = 6.5 % of a 64-subject evaluation) disappears.
__device__ __forceinline__ void syrk_fused_first_block(double* lds, const v4d (&acc)[2][2][2], bool owner, int wj,
                                                       double* __restrict__ C, int ldc, int* __restrict__ info, int goff);

// ---- epilogue of k_syrk_schur (the structured value path's inverse SYRK; the algebra is above k_svc_schur_a in nmgp_kernels.hip) ----
// The expressions, in their order, of the separate kernel this replaced: bit-identical results under -ffp-contract=off.  After the
// k-loop's last barrier the operand buffers hold one patch per wave and a table of the tile's locations.  Two forms:
//   * full tiles at M <= 3 (svc_schur_subtile, every tile of the headline): a 64 x 17 patch (-A^-1 on 16 columns of the wave's
//     sub-tile), one lane per row, one column of Sigma' over 64 rows per store (512-byte runs at a uniform pointer + lane), and a
//     table of the 128 COLUMN locations that also holds L_c (svc_schur_ctable), read as LDS broadcasts;
//   * partial tiles and M >= 4 (svc_schur_patch): a 32 x 33 patch (a 32-row half of the sub-tile), 32 lanes x 2 columns per store
//     (256-byte runs) and, for M <= 4, a table of the 128 column and 128 row locations: g_c[b] = sigma2 L_c[b,0] / L_c00^2
//     (b = 1..M-1), 1 / L_c00^2, x_c and ell_c (larger M compute / load them where they are used).
// Per element the FP64 exp, sqrt and two divisions of K_x plus the entries' products are ~125 vector instructions that share the
// SIMD's FP64 pipe with the MFMAs, in a launch that already moves 35 GB at 4.3 TB/s: the epilogue is cheapest when it runs beside
// the OTHER workgroup's k-loop (see the tile order of k_syrk_schur in syrk_tile_body; DESIGN Appendix B has the measurements).
// k_syrk_schur's LDS: SY_SCHUR_SMEM doubles (two workgroups per CU).
#define SY_SMEM (4 * SY_BK * SY_LD)
#define SCHUR_PATCH (64 * 17)
#define SY_SCHUR_SMEM (8 * SCHUR_PATCH + 6 * 256)
static_assert(SY_SCHUR_SMEM >= SY_SMEM && SY_SCHUR_SMEM * 8 * 2 <= 160 * 1024, "Schur epilogue LDS");

// Sigma'[(a,r),(b,c)] from kv = K_x[r, c] and nai = -A^-1[r, c]: row location r (L row Lr, il2 = 1 / L_r00^2), column location c
// (L row Lc, gcb = g_c[b])
template <int M>
__device__ __forceinline__ double svc_schur_value(double sigma2, int a, int b, bool rc, const double* __restrict__ Lr, double il2,
                                                  const double* __restrict__ Lc, double kv, double nai, double gcb) {
    constexpr int UR = M <= 3 ? 8 : 1;
    const double gra = sigma2 * Lr[a * (a + 1) / 2] * il2;
    double s = 0.0;
#pragma unroll UR
    for (int q = 1; q <= b; ++q) s += Lr[a * (a + 1) / 2 + q] * Lc[b * (b + 1) / 2 + q];
    double v = kv * s;
    if (rc) v += sigma2 * ((a == b ? 1.0 : 0.0) + Lr[a * (a + 1) / 2] * Lr[b * (b + 1) / 2] * il2);
    v += gra * nai * gcb;
    return v;
}

// the entries (a,r),(b,c) for 1 <= b <= a <= M-1 (b < a only when !ALLB); gc: g_c[1..M-1] in LDS (M <= 4).  Sigma' column-major with
// leading dimension e.ld.  Unrolled for M <= 3; from M = 4 on, rolled loops keep the kernel within 128 VGPRs without scratch.
template <int M, bool ALLB>
__device__ __forceinline__ void svc_schur_entries(const SchurEpi& e, double sigma2, int r, const double* __restrict__ Lr, double il2,
                                                  int c, double kv, double nai, const double* gc) {
    constexpr int T = M * (M + 1) / 2;
    constexpr int UR = M <= 3 ? 8 : 1;
    const size_t Ns = (size_t)e.N;
    const double* __restrict__ Lc = e.Lv + (size_t)c * T;
    const double lcc = M <= 4 ? 0.0 : Lc[0];
#pragma unroll UR
    for (int a = 1; a < M; ++a) {
#pragma unroll UR
        for (int b = 1; b <= (ALLB ? a : a - 1); ++b) {
            const double gcb = M <= 4 ? gc[b - 1] : sigma2 * Lc[b * (b + 1) / 2] / (lcc * lcc);
            e.S[((size_t)(b - 1) * Ns + c) * e.ld + ((size_t)(a - 1) * Ns + r)] =
                svc_schur_value<M>(sigma2, a, b, r == c, Lr, il2, Lc, kv, nai, gcb);
        }
    }
}

constexpr int svc_gstride(int M) { return M + 2; }     // g_c[1..M-1], 1 / L_c00^2, x_c, ell_c

// the table (M <= 4): entry k < 128 = column location col0 + k, k >= 128 = row location row0 + k - 128.  Workgroup-uniform call
// after the k-loop's last barrier; ends on a barrier.
template <int M>
__device__ __forceinline__ void svc_schur_gtable(const SchurEpi& e, double* lds, int row0, int col0, int tid) {
    constexpr int T = M * (M + 1) / 2, GS = svc_gstride(M);
    if constexpr (M <= 4) {
        double* gt = lds + 8 * SCHUR_PATCH;
        if (tid < 256) {
            const int loc = tid < 128 ? col0 + tid : row0 + tid - 128;
            if (loc < e.N) {
                const double sigma2 = exp(e.tse[0]);
                const double* Lc = e.Lv + (size_t)loc * T;
                const double l00 = Lc[0];
#pragma unroll
                for (int b = 1; b < M; ++b) gt[tid * GS + b - 1] = sigma2 * Lc[b * (b + 1) / 2] / (l00 * l00);
                gt[tid * GS + M - 1] = 1.0 / (l00 * l00);
                gt[tid * GS + M] = e.x[loc];
                gt[tid * GS + M + 1] = e.ell[loc];
            }
        }
        __syncthreads();
    }
}

// One wave's 32 x 32 patch P[il * 33 + jl] = -A^-1[i0 + il, j0 + jl] (written by this wave).  Pass 1, lanes along i: every
// lower-triangle element (i >= j) gives K_x[i, j] and the entries (a,i),(b,j), b <= a; at M = 3 it also computes the element's one
// mirrored entry (2,j),(1,i) (i > j; K_x is bitwise symmetric) and leaves it in P.  Pass 2, lanes along j: the mirrored entries
// (a,j),(b,i), b < a, of every element with i > j -- copied from P at M = 3, computed (K_x again) otherwise.  Every store runs along
// the Sigma' row index: 256 contiguous bytes per column.
template <int M>
__device__ __forceinline__ void svc_schur_patch(const SchurEpi& e, double* P, const double* lds, int i0, int j0, int row0, int col0,
                                                int lane) {
    constexpr int T_ = M * (M + 1) / 2, GS = svc_gstride(M);
    constexpr int QU = M <= 3 ? 2 : 1;
    const int N = e.N;
    const size_t Ns = (size_t)N;
    const double sigma2 = exp(e.tse[0]);
    const double* gt = lds + 8 * SCHUR_PATCH;
    const int lo = lane & 31, hi = lane >> 5;
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 1 && M == 2) break;
        const int r = (pass == 0 ? i0 : j0) + lo;          // the lane's own location: row location of its entries
        if (r < N) {
            const double* __restrict__ Lr = e.Lv + (size_t)r * T_;
            const double xr = e.x[r], lr = e.ell[r];
            const double xr2 = xr * xr, lr2 = lr * lr;
            const double l00 = Lr[0];
            const double il2 = 1.0 / (l00 * l00);
#pragma unroll QU
            for (int q = 0; q < 16; ++q) {
                const int o = 2 * q + hi;
                const int il = pass == 0 ? lo : o, jl = pass == 0 ? o : lo;
                const int c = (pass == 0 ? j0 : i0) + o;
                if (pass == 0 ? (c > r || c >= N) : (c <= r || c >= N)) continue;
                const double* gc = gt + (pass == 0 ? c - col0 : 128 + c - row0) * GS;
                if (pass == 1 && M == 3) {
                    e.S[(size_t)c * e.ld + (Ns + r)] = P[il * 33 + jl];
                    continue;
                }
                const double xc = M <= 4 ? gc[M] : e.x[c], lc = M <= 4 ? gc[M + 1] : e.ell[c];
                const double dist = (xr2 + xc * xc) - 2.0 * (xr * xc);
                const double Aa = lr2 + lc * lc;
                double kv = sqrt(2.0 * (lr * lc) / Aa) * exp(-dist / Aa);
                if (r == c) kv = NMGP_JITTER + kv;
                const double nai = P[il * 33 + jl];
                if (pass == 0) {
                    svc_schur_entries<M, true>(e, sigma2, r, Lr, il2, c, kv, nai, gc);
                    if (M == 3 && c < r) {
                        // the mirrored entry: row location c (its 1 / L_c00^2 from the table), column location r (g_r[1])
                        const double* Lc = e.Lv + (size_t)c * T_;
                        P[il * 33 + jl] = svc_schur_value<M>(sigma2, 2, 1, false, Lc, gc[M - 1], Lr, kv, nai, gt[(128 + r - row0) * GS]);
                    }
                } else {
                    svc_schur_entries<M, false>(e, sigma2, r, Lr, il2, c, kv, nai, gc);
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// y'[(a,i)] = Y[i,a] - L_i[a,0] (v_i - E_i u_i) (row n' of Sigma'): one lane per location, the diagonal tiles own their rows
template <int M>
__device__ __forceinline__ void svc_schur_yrow(const SchurEpi& e, int i) {
    constexpr int T = M * (M + 1) / 2;
    if (i >= e.N) return;
    const size_t Ns = (size_t)e.N;
    const int n1 = (M - 1) * e.N;
    const double sigma2 = exp(e.tse[0]);
    const double* Li = e.Lv + (size_t)i * T;
    const double l00 = Li[0];
    const double il2 = 1.0 / (l00 * l00);
    const double vi = e.y[i] / l00;
    const double r = vi - (sigma2 * il2) * e.u[i];
#pragma unroll
    for (int a = 1; a < M; ++a) e.S[((size_t)(a - 1) * Ns + i) * e.ld + n1] = e.y[(size_t)a * Ns + i] - Li[a * (a + 1) / 2] * r;
}

// ---- the epilogue of a FULL tile at M <= 3 (syrk_tile_fast): the same entries from the same expressions as svc_schur_patch, in a
// store shape of one column of Sigma' per instruction ----
// The tile's 128 column locations: g_c[1..M-1], 1 / L_c00^2, x_c, ell_c as in svc_schur_gtable, then L_c's T entries.  (The row
// locations are the lanes' own: registers.)  Workgroup-uniform call after the k-loop's last barrier; ends on a barrier.
constexpr int svc_cstride(int M) { return svc_gstride(M) + M * (M + 1) / 2; }
static_assert(128 * svc_cstride(3) <= 6 * 256, "column table of the full-tile Schur epilogue");

template <int M>
__device__ __forceinline__ void svc_schur_ctable(const SchurEpi& e, double* lds, int col0, int tid, double sigma2) {
    constexpr int T = M * (M + 1) / 2, GS = svc_gstride(M), CS = svc_cstride(M);
    double* ct = lds + 8 * SCHUR_PATCH;
    if (tid < 128) {
        const int loc = col0 + tid;
        const double* Lc = e.Lv + (size_t)loc * T;
        const double l00 = Lc[0];
#pragma unroll
        for (int b = 1; b < M; ++b) ct[tid * CS + b - 1] = sigma2 * Lc[b * (b + 1) / 2] / (l00 * l00);
        ct[tid * CS + M - 1] = 1.0 / (l00 * l00);
        ct[tid * CS + M] = e.x[loc];
        ct[tid * CS + M + 1] = e.ell[loc];
#pragma unroll
        for (int t = 0; t < T; ++t) ct[tid * CS + GS + t] = Lc[t];
    }
    __syncthreads();
}

// One wave's 64 x 32 sub-tile of -A^-1 (acc, the layout of syrk_tile_fast; rows i0.., columns j0.., all inside the matrix), 16
// columns at a time through its 64 x 17 patch P.  Pass 1, one lane per ROW: column c of the chunk is wave-uniform -- its table
// entry comes as LDS broadcasts, the lane's own location stays in registers for the whole sub-tile -- and every store instruction
// writes one column of a Sigma' block over 64 rows, 512 contiguous bytes at a uniform pointer + lane.  At M = 3 the element's
// mirrored entry (2,j),(1,i) replaces it in P, and pass 2 (16 lanes along j, four columns i per instruction) copies those out.
template <int M>
__device__ __forceinline__ void svc_schur_subtile(const SchurEpi& e, double* P, const double* ct, const v4d (&acc)[2][2][2], int i0,
                                                  int j0, int col0, int lane, double sigma2) {
    static_assert(M == 2 || M == 3, "larger M: svc_schur_patch");
    constexpr int T = M * (M + 1) / 2, GS = svc_gstride(M), CS = svc_cstride(M);
    const int l15 = lane & 15, l4 = lane >> 4;
    const size_t Ns = (size_t)e.N, ld = (size_t)e.ld;
    const int r = i0 + lane;
    double Lr[T];
#pragma unroll
    for (int t = 0; t < T; ++t) Lr[t] = e.Lv[(size_t)r * T + t];
    const double xr = e.x[r], lr = e.ell[r];
    const double xr2 = xr * xr, lr2 = lr * lr;
    const double l00 = Lr[0];
    const double il2 = 1.0 / (l00 * l00);
    const double gr1 = sigma2 * Lr[1] / (l00 * l00);            // g_r[1], the table's expression
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int jh = j0 + 16 * h;
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int sx = 0; sx < 2; ++sx)
#pragma unroll
                for (int tj = 0; tj < 2; ++tj)
#pragma unroll
                    for (int r2 = 0; r2 < 2; ++r2)
                        P[(32 * p + 2 * l15 + sx) * 17 + 2 * (l4 + 4 * r2) + tj] = -acc[p][sx][tj][2 * h + r2];
        __builtin_amdgcn_wave_barrier();
#pragma unroll 2
        for (int jl = 0; jl < 16; ++jl) {
            const int c = jh + jl;
            if (c > r) continue;
            const double* cc = ct + (c - col0) * CS;
            const double* Lc = cc + GS;
            const double xc = cc[M], lc = cc[M + 1];
            const double dist = (xr2 + xc * xc) - 2.0 * (xr * xc);
            const double Aa = lr2 + lc * lc;
            double kv = sqrt(2.0 * (lr * lc) / Aa) * exp(-dist / Aa);
            if (r == c) kv = NMGP_JITTER + kv;
            const double nai = P[lane * 17 + jl];
            double* colp = e.S + ((size_t)c * ld + (size_t)i0);          // (uniform) column c of block (1, 1), the sub-tile's first row
#pragma unroll
            for (int a = 1; a < M; ++a)
#pragma unroll
                for (int b = 1; b <= a; ++b)
                    (colp + ((size_t)(b - 1) * Ns * ld + (size_t)(a - 1) * Ns))[lane] =
                        svc_schur_value<M>(sigma2, a, b, r == c, Lr, il2, Lc, kv, nai, cc[b - 1]);
            // the mirrored entry: row location c (its 1 / L_c00^2 from the table), column location r (g_r[1])
            if (M == 3 && c < r) P[lane * 17 + jl] = svc_schur_value<M>(sigma2, 2, 1, false, Lc, cc[M - 1], Lr, kv, nai, gr1);
        }
        if (M == 3) {
            __builtin_amdgcn_wave_barrier();
            const int jl = lane & 15, ii = lane >> 4;
            double* mp = e.S + ((size_t)i0 * ld + Ns + (size_t)jh);      // (uniform) row (2, jh) of column (1, i0)
#pragma unroll 4
            for (int q = 0; q < 16; ++q) {
                const int il = 4 * q + ii;
                if (i0 + il > jh + jl) (mp + (size_t)(4 * q) * ld)[ii * e.ld + jl] = P[il * 17 + jl];
            }
        }
    }
}

// SM > 0: k_syrk_schur (M = SM outputs, se = the chain's epilogue arguments): the tile goes into Sigma' instead of C
template <int SM = 0>
__device__ __forceinline__ void syrk_tile_fast(const double* __restrict__ A, int lda, double* __restrict__ C, int ldc, int K,
                                               int row0, int col0, bool diag, int kt0, bool beta0, int ncw, int yrow,
                                               int nyr, double* sA0, double* sB0, bool skip00 = false,
                                               int* __restrict__ finfo = nullptr, int fgoff = 0, bool mirror = false,
                                               int fresh0 = 0x7fffffff, const SchurEpi* se = nullptr) {
    // fresh0: rows i >= fresh0 (relative to C) are rows of L^-T that take part in an update for the first time (gradient
    // evaluation; see potrf_lower): their C entries have never been written -- the accumulators start from zero instead of a
    // load -- and their A entries left of the diagonal (k < i - fresh0) are structural zeros that nobody wrote either.
    constexpr int BK = 16;
    constexpr int SBUF = BK * SY_LD;             // doubles per LDS buffer
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wi = w & 1, wj = w >> 1;
    const int l15 = lane & 15, l4 = lane >> 4;
    // global -> LDS staging: thread (rp, cg) moves rows 2rp, 2rp + 1 of k-columns cg and cg + 8 of the panel
    const int rp = tid & 63, cg = tid >> 6;
    const int offA = (cg * lda + row0 + 2 * rp) * 8, offB = (cg * lda + col0 + 2 * rp) * 8;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)A, 0, 0x7fffffff, 0x00020000);
    const int gstep = BK * lda * 8, ghalf = 8 * lda * 8;
    int soff = kt0 * gstep;
    // THE ROWS BELOW THE LAST FULL TILE (has_y): nyr <= 16 extra rows starting at `yrow` -- the right-hand-side row of a
    // value evaluation, the last two rows of a gradient evaluation -- would cost a whole masked tile per tile column.
    // Instead the two waves of a DIAGONAL tile whose sub-tile lies above the diagonal (wi = 0, wj = 2, 3) update them:
    // C[yrow.., col0 .. col0+127] -= A[yrow.., :] A[col0 .. col0+127, :]^T, 64 columns per wave, with the tile's own j-side
    // panel (already in LDS) as the MFMA A operand and a 16-row chunk holding the extra rows as B operand: 16 MFMAs per
    // k-step in waves that would otherwise idle through the 32 of their siblings.
    const bool has_y = diag && yrow >= 0;
    const bool ywave = has_y && wi == 0 && wj >= 2;
    const int offY = ((tid & 15) * lda + yrow + (tid >> 4)) * 8;      // thread (k = tid & 15, extra row tid >> 4)
    double* sY = sB0;                              // a diagonal tile stages no B panel: its LDS holds the y k-panels
    v4i ra0, ra1, rb0, rb1;
    double ry = 0.0;
    auto gload = [&]() {
        ra0 = __builtin_amdgcn_raw_buffer_load_b128(rsrc, offA, soff, 0);
        ra1 = __builtin_amdgcn_raw_buffer_load_b128(rsrc, offA, soff + ghalf, 0);
        if (!diag) {
            rb0 = __builtin_amdgcn_raw_buffer_load_b128(rsrc, offB, soff, 0);
            rb1 = __builtin_amdgcn_raw_buffer_load_b128(rsrc, offB, soff + ghalf, 0);
        }
        if (has_y && tid < 16 * nyr) {
            typedef int v2i __attribute__((ext_vector_type(2)));
            const v2i t2 = __builtin_amdgcn_raw_buffer_load_b64(rsrc, offY, soff, 0);
            ry = __builtin_bit_cast(double, t2);
        }
        soff += gstep;
    };
    double* wA = sA0 + cg * SY_LD + 2 * rp;
    double* wB = sB0 + cg * SY_LD + 2 * rp;
    auto sstore = [&](int buf) {
        *reinterpret_cast<v4i*>(wA + buf * SBUF) = ra0;
        *reinterpret_cast<v4i*>(wA + buf * SBUF + 8 * SY_LD) = ra1;
        if (!diag) {
            *reinterpret_cast<v4i*>(wB + buf * SBUF) = rb0;
            *reinterpret_cast<v4i*>(wB + buf * SBUF + 8 * SY_LD) = rb1;
        }
        if (has_y && tid < 16 * nyr) sY[buf * 256 + tid] = ry;         // sY[buf][row][k]
    };
    // sub-tile strictly above the diagonal, or right of a half-width tile (ncw = 64: the j-side rows 64..127 of the staged
    // panel are real rows of A, just not columns of this update): nothing to do
    // skip00: the 64x64 block at the tile's origin (sub-tiles wi = 0, wj = 0, 1) is updated by another workgroup
    const bool active = !(diag && (wi * 64 + 63 < wj * 32)) && (wj * 32 < ncw) && !(skip00 && wi == 0 && wj < 2);
    const int nk = K / BK;
    gload();
    // acc[p][s][tj][r]: i = row0 + wi*64 + 32p + 2*l15 + s ; j = col0 + wj*32 + 2*(l4 + 4r) + tj
    v4d acc[2][2][2];
    if (active) {
        // a wave whose 64 rows are all fresh loads nothing (uniform); in the one wave per tile column that straddles the boundary
        // the fresh lanes sit the loads out (fresh0 is even: a row pair never straddles)
        const int rw0 = __builtin_amdgcn_readfirstlane(row0 + wi * 64);
        const bool wload = !beta0 && rw0 < fresh0;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int i = row0 + wi * 64 + 32 * p + 2 * l15;
            const bool old = i < fresh0;
#pragma unroll
            for (int tj = 0; tj < 2; ++tj)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int j = col0 + wj * 32 + 2 * (l4 + 4 * r) + tj;
                    double2 c = make_double2(0.0, 0.0);
                    if (wload && old) c = *reinterpret_cast<const double2*>(&C[(size_t)j * ldc + i]);
                    acc[p][0][tj][r] = -c.x;
                    acc[p][1][tj][r] = -c.y;
                }
        }
    }
    // accumulators of a y-wave live in acc[u][0][t]: columns j = col0 + 64 (wj - 2) + 32 u + 2 (l4 + 4 r) + t, extra row l15
    if (ywave) {
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int j = col0 + 64 * (wj - 2) + 32 * u + 2 * (l4 + 4 * r) + t;
                    acc[u][0][t][r] = (l15 < nyr && yrow + l15 < fresh0) ? -C[(size_t)j * ldc + yrow + l15] : 0.0;
                }
    }
    sstore(0);
    __syncthreads();
    const double* rA = sA0 + wi * 64 + 2 * l15 + l4 * SY_LD;
    const double* rB = (diag ? sA0 : sB0) + wj * 32 + 2 * l15 + l4 * SY_LD;
    auto compute = [&](int buf) {
        const double* tA = rA + buf * SBUF;
        const double* tB = rB + buf * SBUF;
        v2d fa[2], fb, na[2], nb;
        fa[0] = *reinterpret_cast<const v2d*>(tA);
        fa[1] = *reinterpret_cast<const v2d*>(tA + 32);
        fb = *reinterpret_cast<const v2d*>(tB);
#pragma unroll
        for (int kk = 0; kk < BK / 4; ++kk) {
            if (kk + 1 < BK / 4) {
                na[0] = *reinterpret_cast<const v2d*>(tA + (kk + 1) * 4 * SY_LD);
                na[1] = *reinterpret_cast<const v2d*>(tA + (kk + 1) * 4 * SY_LD + 32);
                nb = *reinterpret_cast<const v2d*>(tB + (kk + 1) * 4 * SY_LD);
            }
#pragma unroll
            for (int tj = 0; tj < 2; ++tj)
#pragma unroll
                for (int p = 0; p < 2; ++p)
#pragma unroll
                    for (int sx = 0; sx < 2; ++sx)
                        acc[p][sx][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(fb[tj], fa[p][sx], acc[p][sx][tj], 0, 0, 0);
            if (kk + 1 < BK / 4) {
                fa[0] = na[0];
                fa[1] = na[1];
                fb = nb;
            }
        }
    };
    const double* rY = sA0 + 64 * (wj - 2) + 2 * l15 + l4 * SY_LD;      // j-side rows of a y-wave (only used by y-waves)
    // extra row l15 of a gradient evaluation is a fresh row of L^-T: structurally zero -- and never written -- for k < yrow + l15 - fresh0
    const int yz = (l15 < nyr) ? yrow + l15 - fresh0 - l4 : 0x7fffffff;
    auto compute_y = [&](int buf, int kb) {
        const double* tB = rY + buf * SBUF;
        const double* ty = sY + buf * 256 + l15 * 16 + l4;
#pragma unroll
        for (int kk = 0; kk < BK / 4; ++kk) {
            const v2d f0 = *reinterpret_cast<const v2d*>(tB + kk * 4 * SY_LD);
            const v2d f1 = *reinterpret_cast<const v2d*>(tB + kk * 4 * SY_LD + 32);
            const double yv = ty[4 * kk];
            const double fy = (kb + 4 * kk >= yz) ? yv : 0.0;
            acc[0][0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(f0[0], fy, acc[0][0][0], 0, 0, 0);
            acc[0][0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(f0[1], fy, acc[0][0][1], 0, 0, 0);
            acc[1][0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(f1[0], fy, acc[1][0][0], 0, 0, 0);
            acc[1][0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(f1[1], fy, acc[1][0][1], 0, 0, 0);
        }
    };
    for (int kt = kt0; kt < nk; kt += 2) {         // nk - kt0 is even
        gload();
        if (active) compute(0);
        else if (ywave) compute_y(0, kt * BK);
        sstore(1);
        __syncthreads();
        if (kt + 2 < nk) gload();
        if (active) compute(1);
        else if (ywave) compute_y(1, kt * BK + BK);
        if (kt + 2 < nk) sstore(0);
        __syncthreads();
    }
    if constexpr (SM > 0) {
        // the k-loop ended on a barrier: each wave moves its sub-tile through its patch into Sigma'
        if constexpr (SM <= 3) {
            const double sigma2 = exp(se->tse[0]);
            svc_schur_ctable<SM>(*se, sA0, col0, tid, sigma2);
            if (active)
                svc_schur_subtile<SM>(*se, sA0 + w * SCHUR_PATCH, sA0 + 8 * SCHUR_PATCH, acc,
                                      __builtin_amdgcn_readfirstlane(row0 + wi * 64), __builtin_amdgcn_readfirstlane(col0 + wj * 32),
                                      col0, lane, sigma2);
            if (diag && wj == 0) svc_schur_yrow<SM>(*se, row0 + wi * 64 + lane);
            return;
        }
        // (M >= 4: 32 rows at a time)
        svc_schur_gtable<SM>(*se, sA0, row0, col0, tid);
        if (active) {
            double* P = sA0 + w * SCHUR_PATCH;
#pragma unroll
            for (int p = 0; p < 2; ++p) {
#pragma unroll
                for (int sx = 0; sx < 2; ++sx)
#pragma unroll
                    for (int tj = 0; tj < 2; ++tj)
#pragma unroll
                        for (int r = 0; r < 4; ++r) P[(2 * l15 + sx) * 33 + 2 * (l4 + 4 * r) + tj] = -acc[p][sx][tj][r];
                svc_schur_patch<SM>(*se, P, sA0, row0 + wi * 64 + 32 * p, col0 + wj * 32, row0, col0, lane);
            }
        }
        if (diag && wj == 0) svc_schur_yrow<SM>(*se, row0 + wi * 64 + lane);
        return;
    }
    if (ywave && l15 < nyr) {
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int j = col0 + 64 * (wj - 2) + 32 * u + 2 * (l4 + 4 * r) + t;
                    C[(size_t)j * ldc + yrow + l15] = -acc[u][0][t][r];
                }
    }
    const bool fowner = finfo != nullptr && wi == 0 && wj < 2;      // these two waves hold the 64x64 block to be factored
    if (active && !fowner) {
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = row0 + wi * 64 + 32 * p + 2 * l15;
                const int j = col0 + wj * 32 + 2 * (l4 + 4 * r) + tj;
                if (diag && j > i + 1) continue;
                double2 c;
                c.x = -acc[p][0][tj][r];
                c.y = -acc[p][1][tj][r];
                if (diag && j == i + 1) C[(size_t)j * ldc + i + 1] = c.y;     // the row pair straddles the diagonal
                else *reinterpret_cast<double2*>(&C[(size_t)j * ldc + i]) = c;
            }
    }
    if (mirror && active) {
        // The result is wanted as a FULL symmetric matrix (the inverse covariance of the gradient path): the sub-tile also goes
        // to its mirror position C[j, i].  Through a wave-private LDS patch (32 x 32, padded), so that the lanes of a store run
        // along j -- 256 contiguous bytes per column of C -- instead of 8-byte accesses a leading dimension apart.  (The k-loop
        // ended on a barrier: the operand buffers are free; a wave's LDS operations execute in order.)
        double* T = sA0 + w * (32 * 33);
        const int jl = lane & 31, ih = lane >> 5;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
#pragma unroll
            for (int sx = 0; sx < 2; ++sx)
#pragma unroll
                for (int tj = 0; tj < 2; ++tj)
#pragma unroll
                    for (int r = 0; r < 4; ++r) T[(2 * l15 + sx) * 33 + 2 * (l4 + 4 * r) + tj] = -acc[p][sx][tj][r];
            const int rowm = col0 + wj * 32 + jl;                       // row index of the mirrored element (= j)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int il = 2 * q + ih;
                const int colm = row0 + wi * 64 + 32 * p + il;          // its column index (= i)
                const double v = T[il * 33 + jl];
                if (colm > rowm) C[(size_t)colm * ldc + rowm] = v;       // (diagonal tiles: strictly upper only)
            }
        }
    }
    if (finfo != nullptr) syrk_fused_first_block(sA0, acc, fowner, wj, C, ldc, finfo, fgoff);     // workgroup-uniform
}

// C[i, j] -= sum_k A[i, k] A[j, k]   for 0 <= j < ncols, j <= i < mrows    (A: mrows x K, C: mrows x ncols)
// NWJ = column groups of waves per 128x128 tile: 2 -> 4 waves of 64x64 (16 MFMA tiles each), 4 -> 8 waves of 64x32
// (8 MFMA tiles each, ~110 VGPRs, so four waves per SIMD hide each other's barrier / LDS / prologue stalls).
// SM > 0: k_syrk_schur's tiles (C unused; se: the launch's epilogue arguments, see syrk_tile_fast)
template <int NWJ, int BK, int SM = 0>
__device__ __forceinline__ void syrk_tile_body(const double* __restrict__ A, int lda, double* __restrict__ C, int ldc, int mrows,
                                               int ncols, int K, long long bstride, long long cstride, int ktri, int swz,
                                               int nbatch, int bx, int by, int bz0, double* sAb, double* sBb,
                                               int tri_row0 = 0x7fffffff, int tri_k0 = 0, int* __restrict__ finfo = nullptr,
                                               int fistride = 0, int fgoff = 0, const SchurEpi* sep = nullptr) {
    // tri_row0 / tri_k0: rows i >= tri_row0 of A are rows of an upper-triangular matrix riding below the factorisation (L^-T of
    // the gradient evaluation): A[i, k] == 0 for k < (i - tri_row0) - tri_k0, so a tile made of such rows starts its k-loop
    // there instead of multiplying zeros (with 1024-wide panels that was 12 % of the update flop, with 2048-wide ones 25 %)
    // (bx, by, bz0) = the launch's blockIdx, or the tile a fused kernel assigns to this workgroup; sAb / sBb: 2 * BK * SY_LD
    // doubles of LDS each
    const int nyr = (ktri >> 2) & 31;         // rows mrows .. mrows + nyr - 1 (just below the full tiles): see syrk_tile_fast
    const bool skipq = (ktri & 128) != 0;     // the leading 64x64 block of tile (0, 0) belongs to somebody else (k_panel_step)
    const bool mirror = (ktri & 512) != 0;    // also write the strictly upper triangle (C symmetric): beta = 0 launches only
    const bool rowmajor = (ktri & 1024) != 0; // tile order of the triangular-operand launches: see below
    const int yrow = nyr ? mrows : -1;
    (void)rowmajor;
    ktri &= 1;
    // rows of L^-T that enter the factorisation with this launch (potrf_lower): the caller describes them by (tri_row0, tri_k0)
    const int fresh0 = tri_row0 == 0x7fffffff ? 0x7fffffff : tri_row0 + tri_k0;
    constexpr int NT = 128 * NWJ;          // threads
    constexpr int CW = 128 / NWJ;          // columns per wave
    constexpr int TJ = CW / 16;            // MFMA tiles per wave along j
    constexpr int NQ = (64 * BK) / NT;     // 16-byte loads per thread per operand and k-step
    constexpr int CGS = NT / 64;           // k-columns covered per load round
    double (*sA)[BK * SY_LD] = reinterpret_cast<double (*)[BK * SY_LD]>(sAb);
    double (*sB)[BK * SY_LD] = reinterpret_cast<double (*)[BK * SY_LD]>(sBb);
    int bi = bx, bj = by;
    int bz = bz0;
    if (swz) {
        // XCD-aware tile order.  Workgroups are dealt round-robin and IN ORDER over the 8 XCDs (t and t + 8 share an
        // L2), so every XCD must receive the same work per round or the others idle behind it: the VALID tiles of all
        // matrices of the batch are enumerated compactly (strips of 8 tile columns; per strip the diagonal triangle,
        // then 8-row blocks) and cut into chunks of 64 tiles = the 32 CUs x 2 resident workgroups of one XCD.  XCD
        // t % 8 walks chunks (t % 8), (t % 8) + 8, ...: a chunk touches <= 16 row panels + 8 column panels of A, which
        // its L2 then fetches once per chunk instead of once per tile.  swz = valid tiles per matrix.
        // Short launches (swz < 0, -swz = valid tiles per matrix) keep the compact enumeration but deal consecutive
        // tiles to consecutive XCDs: no early-exit workgroups, and no correlation between XCD and tile row (with a plain
        // grid of 8 k tile rows XCD x owned tile row x: 1 tile for XCD 0, 8 for XCD 7).
        const int t = bx, q = t >> 3;
        const int tiles_pm = swz > 0 ? swz : -swz;
        const long long g = swz > 0 ? ((long long)(q >> 6) * 8 + (t & 7)) * 64 + (q & 63) : (long long)t;   // compact tile index
        int idx;
        if (finfo != nullptr) {
            // tile (0, 0) of EVERY matrix first: those workgroups go on to factor a diagonal block and must not start late
            if (g >= (long long)tiles_pm * nbatch) return;                   // padding workgroup
            if (g < nbatch) {
                bz = (int)g;
                idx = 0;
            } else {
                const long long g2 = g - nbatch;
                bz = (int)(g2 / (tiles_pm - 1));
                idx = 1 + (int)(g2 - (long long)bz * (tiles_pm - 1));
            }
        } else {
            bz = (int)(g / tiles_pm);
            if (bz >= nbatch) return;                                        // padding workgroup
            idx = (int)(g - (long long)bz * tiles_pm);
            // k_syrk_schur: odd chains walk their tile list backwards (shortest tiles first).  Workgroups t and t + 256 share a CU
            // and would otherwise hold tiles of the same length two chains apart: they leave the k-loop together, and their vector
            // epilogues run with no k-loop beside them and no epilogue beside the k-loops.  With tiles of different length on a CU
            // one workgroup's epilogue falls into the other's k-loop: 8.45 -> 8.12 ms at 128 chains of N = 2048 (DESIGN Appendix
            // B).  The last chains keep longest-first for the launch's tail.  The tiles are independent: same bits in any order.
            if (SM > 0 && (bz & 1) && bz + 8 < nbatch) idx = tiles_pm - 1 - idx;
        }
        const int gx = (mrows + SY_BM - 1) / SY_BM, gy = (ncols + SY_BM - 1) / SY_BM;
        if (rowmajor) {
            // Triangular operand (A = L^-T: the k-loop of tile row bi starts at its first row, K_eff = n - 128 bi): tiles differ in
            // length by up to 48x.  Workgroups are dispatched in id order and id t lands on XCD t % 8, so an XCD that holds longer
            // tiles than the others makes them wait; the strip order above gives XCD x a whole 8 x 8 block of similar tiles and its
            // neighbour a block 8 tile rows further down (shorter).  Here the square lower triangle is enumerated row by row
            // (consecutive ids = consecutive tiles of one tile row = equal length, spread over all XCDs; longest rows first).
            // (a trapezoid with more tile rows than tile columns: the rows below the triangle have gy tiles each)
            const int tri = gy * (gy + 1) / 2;
            if (idx < tri) {
                int b = (int)((sqrt(8.0 * (double)idx + 1.0) - 1.0) * 0.5);
                while ((b + 1) * (b + 2) / 2 <= idx) ++b;
                while (b * (b + 1) / 2 > idx) --b;
                bi = b;
                bj = idx - b * (b + 1) / 2;
            } else {
                bi = gy + (idx - tri) / gy;
                bj = (idx - tri) % gy;
            }
        } else {
        int c0 = 0, W = 0, cnt = 0;
        for (;; c0 += SY_SB) {                       // strip of W tile columns starting at tile column c0
            W = gy - c0 < SY_SB ? gy - c0 : SY_SB;
            cnt = W * (W + 1) / 2 + (gx - c0 - W) * W;
            if (idx < cnt) break;
            idx -= cnt;
        }
        const int tri = W * (W + 1) / 2;
        if (idx < tri) {
            int b = 0;
            while (idx >= W - b) {
                idx -= W - b;
                ++b;
            }
            bj = c0 + b;
            bi = bj + idx;
        } else {
            idx -= tri;
            const int blk = idx / (SY_SB * W), in = idx - blk * (SY_SB * W);
            const int base = c0 + W + blk * SY_SB;
            const int rb = gx - base < SY_SB ? gx - base : SY_SB;
            bj = c0 + in / rb;
            bi = base + in % rb;
        }
        }
    }
    if (bi < bj) return;
    // workgroup-uniform by construction; the 64-bit divisions of the decode run on the VALU, so tell the compiler
    // (keeps the tile origin, the C pointer and the buffer descriptor in SGPRs)
    bi = __builtin_amdgcn_readfirstlane(bi);
    bj = __builtin_amdgcn_readfirstlane(bj);
    bz = __builtin_amdgcn_readfirstlane(bz);
    A += (size_t)bz * bstride;       // batch of independent matrices (one per chain), same shape
    C += (size_t)bz * cstride;
    SchurEpi se{};
    if constexpr (SM > 0) {
        static_assert(NWJ == 4 && BK == 16, "the Schur epilogue assumes 8 waves of 64 x 32");
        constexpr int T = SM * (SM + 1) / 2;
        se = *sep;
        se.x += (size_t)(bz / se.cps) * se.xstride;
        se.y += (size_t)(bz / se.cps) * se.ystride;
        se.ell += (size_t)bz * se.N;
        se.Lv += (size_t)bz * se.N * T;
        se.tse += (size_t)bz * ((size_t)se.N * (1 + T) + 1);
        se.u += (size_t)bz * se.N;
        se.S += (size_t)bz * se.bstride;
    }
    const bool diag = (bi == bj);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wi = w & 1, wj = w >> 1;
    const int row0 = bi * SY_BM, col0 = bj * SY_BM;
    if constexpr (NWJ == 4 && BK == 16) {
        // interior tile (uniform per workgroup): the mask-free, VALU-free path
        // (32-bit byte offsets into the panel: (K + 16) * lda * 8 must stay below 2^31)
        // (a tile that is full in rows and 64 columns wide -- the K = 64 updates inside a panel -- also qualifies)
        const int ncw = ncols - col0 >= SY_BM ? SY_BM : ncols - col0;
        if (row0 + SY_BM <= mrows && (ncw == SY_BM || ncw == 64) && col0 + SY_BM <= mrows && (K & 31) == 0 &&
            (long long)(K + 16) * lda * 8 < 0x7fff0000LL) {
            int kt0f = ktri ? row0 / BK : 0;
            if (row0 >= tri_row0) {
                const int z = (row0 - tri_row0 - tri_k0) / BK;        // leading all-zero k-panels of this tile's rows
                kt0f = z > 0 ? (z & ~1) : 0;                          // (the unrolled loop wants an even number of panels)
            }
            // finfo: tile (0, 0) goes on to factor its leading 64x64 block (the host sets it only when that tile takes this path)
            syrk_tile_fast<SM>(A, lda, C, ldc, K, row0, col0, diag, kt0f, ktri != 0, ncw, yrow, nyr, &sA[0][0], &sB[0][0],
                               skipq && bi == 0 && bj == 0, (finfo != nullptr && bi == 0 && bj == 0) ? finfo + (size_t)bz * fistride : nullptr,
                               fgoff, mirror, fresh0, &se);
            return;
        }
    }
    const int rp = tid & 63, cg = tid >> 6;
    double2 ra[NQ], rb[NQ];

    const int ri = row0 + 2 * rp, rj = col0 + 2 * rp;
    const int ric = clamp_row_pair(ri, mrows), rjc = clamp_row_pair(rj, mrows);
    const bool ix = ri < mrows, iy = ri + 1 < mrows, jx = rj < mrows, jy = rj + 1 < mrows;
    // the last row of an odd-height panel sits at an even index with no partner: its clamped pair starts one row
    // earlier, so the wanted value arrives in .y
    const bool ish = ix && (ric != ri), jsh = jx && (rjc != rj);
    auto gload = [&](int k0) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int kc = k0 + cg + CGS * q;
            const double* colp = A + (size_t)(kc < K ? kc : K - 1) * lda;
            ra[q] = *reinterpret_cast<const double2*>(colp + ric);
            if (!diag) rb[q] = *reinterpret_cast<const double2*>(colp + rjc);
        }
    };
    auto sstore = [&](int buf, int k0) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int kl = cg + CGS * q;
            const bool kin = (k0 + kl) < K;
            double2 va, vb;
            va.x = (kin && ix) ? (ish ? ra[q].y : ra[q].x) : 0.0;
            va.y = (kin && iy) ? ra[q].y : 0.0;
            *reinterpret_cast<double2*>(&sA[buf][kl * SY_LD + 2 * rp]) = va;
            if (!diag) {
                vb.x = (kin && jx) ? (jsh ? rb[q].y : rb[q].x) : 0.0;
                vb.y = (kin && jy) ? rb[q].y : 0.0;
                *reinterpret_cast<double2*>(&sB[buf][kl * SY_LD + 2 * rp]) = vb;
            }
        }
    };

    // a wave whose sub-tile lies strictly above the diagonal has nothing to compute
    const bool active = !(diag && (wi * 64 + 63 < wj * CW));
    const bool skip00g = skipq && bi == 0 && bj == 0;
    const int nk = (K + BK - 1) / BK;
    // ktri: A is upper triangular as a matrix (A[i, k] = 0 for k < i, e.g. L^-T), so the k-panels left of this tile's
    // first row contribute nothing; ktri also means beta = 0: C is OVERWRITTEN with -A A^T (no zero-fill, no read of C)
    int kt0 = ktri ? (row0 / BK) : 0;
    if (row0 >= tri_row0 && row0 - tri_row0 - tri_k0 > 0) kt0 = (row0 - tri_row0 - tri_k0) / BK;
    gload(kt0 * BK);
    // The accumulators START as the C tile (the loads overlap the first panel fetch) and the j-side fragment enters
    // the MFMA negated, so the k-loop leaves C - A A^T in registers and the epilogue is stores only.
    // D[row = (lane>>4) + 4 reg <-> j][col = lane&15 <-> i]
    v4d acc[TJ][4];
#pragma unroll
    for (int tj = 0; tj < TJ; ++tj)
#pragma unroll
        for (int ti = 0; ti < 4; ++ti)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = row0 + wi * 64 + ti * 16 + (lane & 15);
                const int j = col0 + wj * CW + tj * 16 + (lane >> 4) + 4 * r;
                acc[tj][ti][r] = (!ktri && active && i < mrows && j < ncols && i >= j) ? C[(size_t)j * ldc + i] : 0.0;
            }
    if (row0 + SY_BM > fresh0) {          // (uniform) fresh rows start from zero whatever their memory holds: see syrk_tile_fast
#pragma unroll
        for (int tj = 0; tj < TJ; ++tj)
#pragma unroll
            for (int ti = 0; ti < 4; ++ti)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    acc[tj][ti][r] = (row0 + wi * 64 + ti * 16 + (lane & 15) >= fresh0) ? 0.0 : acc[tj][ti][r];
    }
    sstore(0, kt0 * BK);
    __syncthreads();
    for (int kt = kt0; kt < nk; ++kt) {
        const int cur = (kt - kt0) & 1;
        if (kt + 1 < nk) gload((kt + 1) * BK);
        if (active) {
            const double* tA = sA[cur] + wi * 64 + (lane & 15) + (lane >> 4) * SY_LD;
            const double* tB = (diag ? sA[cur] : sB[cur]) + wj * CW + (lane & 15) + (lane >> 4) * SY_LD;
            // fragments of k-substep kk+1 are fetched from LDS while the MFMAs of kk issue (software pipeline:
            // without it every substep exposes one LDS round trip before its first MFMA)
            double fa[4], fb[TJ], na[4], nb[TJ];
#pragma unroll
            for (int t = 0; t < 4; ++t) fa[t] = tA[t * 16];
#pragma unroll
            for (int t = 0; t < TJ; ++t) fb[t] = -tB[t * 16];
#pragma unroll
            for (int kk = 0; kk < BK / 4; ++kk) {
                if (kk + 1 < BK / 4) {
#pragma unroll
                    for (int t = 0; t < 4; ++t) na[t] = tA[(kk + 1) * 4 * SY_LD + t * 16];
#pragma unroll
                    for (int t = 0; t < TJ; ++t) nb[t] = -tB[(kk + 1) * 4 * SY_LD + t * 16];
                }
#pragma unroll
                for (int tj = 0; tj < TJ; ++tj)
#pragma unroll
                    for (int ti = 0; ti < 4; ++ti)
                        acc[tj][ti] = __builtin_amdgcn_mfma_f64_16x16x4f64(fb[tj], fa[ti], acc[tj][ti], 0, 0, 0);
                if (kk + 1 < BK / 4) {
#pragma unroll
                    for (int t = 0; t < 4; ++t) fa[t] = na[t];
#pragma unroll
                    for (int t = 0; t < TJ; ++t) fb[t] = nb[t];
                }
            }
        }
        if (kt + 1 < nk) sstore(cur ^ 1, (kt + 1) * BK);
        __syncthreads();
    }
    if constexpr (SM > 0) {
        // as in syrk_tile_fast: acc holds -A^-1 here; half h of the wave's rows = MFMA tiles ti = 2h, 2h + 1
        svc_schur_gtable<SM>(se, sAb, row0, col0, tid);
        if (active) {
            double* P = sAb + w * SCHUR_PATCH;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
#pragma unroll
                for (int tj = 0; tj < TJ; ++tj)
#pragma unroll
                    for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            P[(t2 * 16 + (lane & 15)) * 33 + tj * 16 + (lane >> 4) + 4 * r] = acc[tj][2 * h + t2][r];
                svc_schur_patch<SM>(se, P, sAb, row0 + wi * 64 + 32 * h, col0 + wj * CW, row0, col0, lane);
            }
        }
        if (diag && wj == 0) svc_schur_yrow<SM>(se, row0 + wi * 64 + lane);
        return;
    }
    if (active) {
#pragma unroll
        for (int tj = 0; tj < TJ; ++tj)
#pragma unroll
            for (int ti = 0; ti < 4; ++ti)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = row0 + wi * 64 + ti * 16 + (lane & 15);
                    const int j = col0 + wj * CW + tj * 16 + (lane >> 4) + 4 * r;
                    if (i < mrows && j < ncols && i >= j && !(skip00g && i < 64 && j < 64)) C[(size_t)j * ldc + i] = acc[tj][ti][r];
                    if (mirror && i < mrows && j < ncols && i > j) C[(size_t)i * ldc + j] = acc[tj][ti][r];   // (edge tiles only)
                }
    }
}

// C[i, j] -= sum_k A[i, k] A[j, k] on the lower trapezoid (see syrk_tile_body): 128x128 tiles, 8 waves of 64x32.
__global__ __launch_bounds__(512, 4) void k_syrk_lower(const double* __restrict__ A, int lda, double* __restrict__ C, int ldc,
                                                        int mrows, int ncols, int K, long long bstride, long long cstride,
                                                        int ktri, int swz, int nbatch, int tri_row0, int tri_k0,
                                                        int* __restrict__ finfo, int fistride, int fgoff) {
    __shared__ __attribute__((aligned(16))) double smem[4 * SY_BK * SY_LD];      // A panels | B panels (contiguous: see finfo)
    syrk_tile_body<4, SY_BK>(A, lda, C, ldc, mrows, ncols, K, bstride, cstride, ktri, swz, nbatch, blockIdx.x, blockIdx.y,
                             blockIdx.z, smem, smem + 2 * SY_BK * SY_LD, tri_row0, tri_k0, finfo, fistride, fgoff);
}

// The structured value path's inverse SYRK (syrk_schur): the triangular-operand launch of k_syrk_lower (ktri = 2) whose tiles write
// Sigma' and y' instead of -A^-1 (syrk_tile_fast / syrk_tile_body with SM = M)
template <int M>
__global__ __launch_bounds__(512, 4) void k_syrk_schur(const double* __restrict__ A, int lda, int N, long long bstride, int kflags,
                                                        int swz, int nbatch, SchurEpi se) {
    __shared__ __attribute__((aligned(16))) double smem[SY_SCHUR_SMEM];
    syrk_tile_body<4, SY_BK, M>(A, lda, nullptr, 0, N, N, N, bstride, 0, kflags, swz, nbatch, blockIdx.x, blockIdx.y, blockIdx.z,
                                smem, smem + 2 * SY_BK * SY_LD, 0x7fffffff, 0, nullptr, 0, 0, &se);
}

// The host schedule's switches, read once per process on first use.
struct Switches {
    enum Panel { kAuto, kFused, kRec, kRl };
    Panel panel = kAuto;            // NMGP_CHOL_PANEL = fused | rec | rl | auto (default): the panel schedule, see Factorisation::panel
    int fused_max_batch = -1;       // NMGP_CHOL_FUSED_MAX_BATCH: largest batch that takes the fused steps under auto (< 0: by size)
    int fused_base = 0;             // NMGP_CHOL_FUSED_BASE=<128|256|512|...>: width of the pieces that run as fused steps (0: auto)
    int la_max_batch = 16;          // NMGP_CHOL_LA_MAX_BATCH: largest batch that takes the two-stream look-ahead
    int syrk_small_max = 256;       // NMGP_SYRK_SMALL_MAX: most 128x128 tiles of an update that runs on 64x64 tiles instead
    const char* step_stamps = nullptr;   // NMGP_STEP_STAMPS=<file>: see StepStamps
};
static const Switches& switches() {
    static const Switches sw = [] {
        Switches w;
        if (const char* e = std::getenv("NMGP_CHOL_PANEL"))
            w.panel = std::strcmp(e, "fused") == 0 ? Switches::kFused
                      : std::strcmp(e, "rec") == 0 ? Switches::kRec : std::strcmp(e, "rl") == 0 ? Switches::kRl : Switches::kAuto;
        if (const char* e = std::getenv("NMGP_CHOL_FUSED_MAX_BATCH")) w.fused_max_batch = std::atoi(e);
        if (const char* e = std::getenv("NMGP_CHOL_FUSED_BASE")) w.fused_base = (std::atoi(e) / 64) * 64;
        if (const char* e = std::getenv("NMGP_CHOL_LA_MAX_BATCH")) w.la_max_batch = std::atoi(e);
        if (const char* e = std::getenv("NMGP_SYRK_SMALL_MAX")) w.syrk_small_max = std::atoi(e);
        w.step_stamps = std::getenv("NMGP_STEP_STAMPS");
        return w;
    }();
    return sw;
}

// NMGP_STEP_STAMPS=<file>: per-step phase stamps of the critical workgroup (developer aid, tools/step_stamps.py).  The device
// buffer (16 slots per 64-column step) is cleared before a factorisation and dumped after it (synchronises).
struct StepStamps {
    long long* dev = nullptr;
    int cap = 0;
    long long* begin(hipStream_t s, int nsteps) {
        if (!switches().step_stamps) return nullptr;
        if (cap < nsteps) {
            if (dev) hipFree(dev);
            if (hipMalloc((void**)&dev, (size_t)nsteps * 16 * sizeof(long long)) != hipSuccess) dev = nullptr;
            cap = dev ? nsteps : 0;
        }
        if (dev) hipMemsetAsync(dev, 0, (size_t)cap * 16 * sizeof(long long), s);
        return dev;
    }
    void dump(hipStream_t s, int nsteps) const {
        if (!switches().step_stamps || !dev) return;
        std::vector<long long> h((size_t)nsteps * 16);
        hipStreamSynchronize(s);
        hipMemcpy(h.data(), dev, h.size() * sizeof(long long), hipMemcpyDeviceToHost);
        if (FILE* f = std::fopen(switches().step_stamps, "w")) {
            for (int k = 0; k < nsteps; ++k) {
                for (int j = 0; j < 9; ++j) std::fprintf(f, "%lld ", h[(size_t)k * 16 + j]);
                std::fprintf(f, "\n");
            }
            std::fclose(f);
        }
    }
};
static StepStamps g_step_stamps;

// tri_row0 / un_fresh / u_tri of a launch without rows of L^-T (what the kernels' defaults say)
static constexpr int kNoTriRows = 0x7fffffff;

// launch geometry of one trapezoid update: grid, tile-order mode and kernel flags (shared with the fused panel step)
struct SyrkPlan {
    dim3 grid;
    int swz = 0;
    int kflags = 0;
    int mrows = 0;       // rows covered by full/partial tiles (the rows below, if any, ride in the diagonal tiles)
    int tiles = 0;       // valid lower-trapezoid tiles per matrix
};

static SyrkPlan syrk_plan(int lda, int ldc, int mrows, int ncols, int K, int batch, int ktri, bool compact_only,
                          bool tri_rows = false) {
    SyrkPlan pl;
    // evaluations carry a few extra rows below a whole number of tiles (value: the right-hand side; gradient: two more rows
    // of L^-T): the diagonal tiles take them along (syrk_tile_fast) and the masked tile row disappears.  Needs every tile
    // of the launch on the fast path.
    int yflag = 0;
    const int nyr = mrows % SY_BM;                      // rows below the last full tile
    if (!ktri && mrows > SY_BM && nyr >= 1 && nyr <= 16 && ncols % SY_BM == 0 && (K & 31) == 0 &&
        (long long)(K + 16) * lda * 8 < 0x7fff0000LL && (lda & 1) == 0 && (ldc & 1) == 0) {
        yflag = nyr << 2;
        mrows -= nyr;
    }
    pl.mrows = mrows;
    pl.grid = dim3(cdiv_c(mrows, SY_BM), cdiv_c(ncols, SY_BM), batch);
    const int gx = pl.grid.x, gy = pl.grid.y;
    for (int c0 = 0; c0 < gy; c0 += SY_SB) {            // valid (lower-trapezoid) tiles per matrix
        const int W = gy - c0 < SY_SB ? gy - c0 : SY_SB;
        pl.tiles += W * (W + 1) / 2 + (gx - c0 - W) * W;
    }
    if (compact_only || gy >= 2) {
        const long long total = (long long)pl.tiles * batch;
        const long long rounds = (total + 511) / 512;   // 8 XCDs x 64 tiles per round
        if (rounds >= 16 && !compact_only) {            // chunks of 64 tiles per XCD (L2 reuse)
            pl.grid = dim3((unsigned)(rounds * 512), 1, 1);
            pl.swz = pl.tiles;
        } else {                                        // fewer rounds: the chunking's tail would cost more than it gains
            pl.grid = dim3((unsigned)total, 1, 1);
            pl.swz = -pl.tiles;
        }
    }
    pl.kflags = (ktri ? 1 : 0) | (ktri == 2 ? 512 : 0) | yflag;          // ktri = 2: triangular A, C overwritten, both triangles
    // (measured, 128 chains value+gradient, same box: strips 257.6-258.2 evals/s, row-major for the inverse SYRK only 258.7-259.0,
    // also for the factorisation's updates with K >= 1024: 262.7-263.1; from K >= 512 / 256 / 64 on: 1.3 / 2.6 / 1.7 evals/s less --
    // there the tiles of L^-T rows are a small share and the L2 reuse of the strip order is worth more)
    // (the inverse SYRK of SMALL batches -- compact enumeration, a few rounds of tiles -- gains most: longest tile rows first is also
    // the better schedule for the launch's tail; one chain value+gradient 163 -> 168 evals/s, its inverse SYRK 1.47 -> 1.22 ms)
    if ((ktri || (tri_rows && K >= 1024)) && gx >= gy && (pl.swz > 0 || (ktri && pl.swz < 0))) {
        // triangular-operand launch (the inverse SYRK; the big updates of a gradient factorisation, whose L^-T rows skip their
        // leading zero k-panels): tiles of very different length -- row-major order, dealt to the XCDs tile by tile (see
        // syrk_tile_body)
        pl.grid = dim3((unsigned)((long long)pl.tiles * batch), 1, 1);
        pl.swz = -pl.tiles;
        pl.kflags |= 1024;
    }
    return pl;
}

__global__ __launch_bounds__(256) void k_potf2_64(double* __restrict__ A, int lda, int nb, int* __restrict__ info,
                                                   int goff, long long bstride, int istride) {
    __shared__ double colbuf[2][64];
    __shared__ double pivs[64];
    potf2_body(A + (size_t)blockIdx.x * bstride, lda, nb, info + (size_t)blockIdx.x * istride, goff, threadIdx.x, colbuf, pivs);
}

// ---------------------------------------------------------------------------------------------
// 64x64 diagonal block, blocked: four 16-column blocks.  The 64 sequential pivots of k_potf2_64 cost ~960 cycles each
// (a workgroup barrier, ~10 LDS reads and ~16 masked FMAs per thread and pivot); here the 16x16 DIAGONAL blocks are factored
// by ONE wave in registers (potf2m_group below) and everything below / right of them goes through the matrix cores:
//   (A) the diagonal block S_qq and, along with it, inv(L_qq);
//   (B) X_i = S_iq inv(L_qq)^T for the row blocks below (4 MFMAs each);
//   (C) S_ij -= X_i X_j^T for q < j <= i.
// The block lives in LDS column-major (S[col][row]); potf2b_core_mfma has the schedule.
// ---------------------------------------------------------------------------------------------
#define PB_LD 66
__device__ __forceinline__ double readlane_f64(double v, int srclane) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_readlane(lo, srclane);
    hi = __builtin_amdgcn_readlane(hi, srclane);
    return __hiloint2double(hi, lo);
}

// ---- 16x16 diagonal block in 4-column groups on the matrix cores (the default of phase (A) below) -------------------
// Pivot by pivot (round 1) a 16x16 block cost ~460 cycles per pivot, most of it waiting for cross-lane traffic (five exposed
// ds_bpermute / v_readlane round trips).  Here the block lives in ONE wave's registers in the MFMA accumulator
// layout -- S[i][j] in register i >> 2 of lane j + 16 (i & 3), kept SYMMETRIC, so that the four rows 4 g .. 4 g + 3 are
// register g and are, as they stand, the B operand (and by symmetry the A operand) of a K = 4 MFMA -- and is factored four
// columns at a time:
//   * the 4x4 diagonal block is read into SGPRs (v_readlane, compile-time lanes) and factored by EVERY lane redundantly
//     (uniform values, no cross-lane traffic), together with its inverse W;
//   * X^T = W S[4g.., :]  (the column block of L and everything below it) is ONE v_mfma_f64_16x16x4_f64 whose result
//     register 0 is, again without moving anything, both operands of the rank-4 update S -= X X^T (one more MFMA);
//   * the same two operands carry the inverse along: Y = W E[4g.., :], E -= X Y, rows 4g.. of inv(L) = Y.
// Critical path per four pivots: 20 v_readlane, the scalar 4x4 factorisation, two dependent MFMAs.
__device__ __forceinline__ double rsqrt_nr(double d) {
    double y = __builtin_amdgcn_rsq(d);
    double t = d * y;
    double e = fma(-t, y, 1.0);
    y = fma(0.5 * y, e, y);
    t = d * y;
    e = fma(-t, y, 1.0);
    y = fma(0.5 * y, e, y);
    return y;
}

template <int G>
__device__ __forceinline__ void potf2m_group(v4d& S, v4d& E, double& yfin, double* __restrict__ Sblk, int& first_bad, int lane,
                                             int l15, int l4) {
    constexpr int b0 = 4 * G;
    // the 4x4 diagonal block (lower part): S[b0 + a][b0 + b] sits in register G of lane (b0 + b) + 16 a
    const double sg = S[G];
    const double d00 = readlane_f64(sg, b0 + 0), d10 = readlane_f64(sg, b0 + 16), d11 = readlane_f64(sg, b0 + 17);
    const double d20 = readlane_f64(sg, b0 + 32), d21 = readlane_f64(sg, b0 + 33), d22 = readlane_f64(sg, b0 + 34);
    const double d30 = readlane_f64(sg, b0 + 48), d31 = readlane_f64(sg, b0 + 49), d32 = readlane_f64(sg, b0 + 50);
    const double d33 = readlane_f64(sg, b0 + 51);
    // Cholesky of the 4x4 block, every lane the same arithmetic; r_c = 1 / l_cc
    const double r0 = rsqrt_nr(d00);
    const double l10 = d10 * r0, l20 = d20 * r0, l30 = d30 * r0;
    const double p1 = fma(-l10, l10, d11);
    const double r1 = rsqrt_nr(p1);
    const double l21 = fma(-l20, l10, d21) * r1, l31 = fma(-l30, l10, d31) * r1;
    const double p2 = fma(-l21, l21, fma(-l20, l20, d22));
    const double r2 = rsqrt_nr(p2);
    const double l32 = fma(-l31, l21, fma(-l30, l20, d32)) * r2;
    const double p3 = fma(-l32, l32, fma(-l31, l31, fma(-l30, l30, d33)));
    const double r3 = rsqrt_nr(p3);
    // first non-positive pivot so far, LAPACK numbering within the 16x16 block (the NaN of a failed earlier pivot also lands
    // here); selects only -- a branch here would sit in the middle of the dependent chain
    {
        int bad = 0;
        bad = !(p3 > 0.0) ? b0 + 4 : bad;
        bad = !(p2 > 0.0) ? b0 + 3 : bad;
        bad = !(p1 > 0.0) ? b0 + 2 : bad;
        bad = !(d00 > 0.0) ? b0 + 1 : bad;
        first_bad = first_bad ? first_bad : bad;
    }
    // W = inv(L_gg), lower triangular
    const double w10 = -(l10 * r0) * r1;
    const double w21 = -(l21 * r1) * r2;
    const double w32 = -(l32 * r2) * r3;
    const double w20 = -fma(l21, w10, l20 * r0) * r2;
    const double w31 = -fma(l32, w21, l31 * r1) * r3;
    const double w30 = -fma(l32, w20, fma(l31, w10, l30 * r0)) * r3;
    // A operand of the two "solve" MFMAs: lane n + 16 k carries W[n][k]
    double a1 = 0.0;
    a1 = (l15 == 0 && l4 == 0) ? r0 : a1;
    a1 = (l15 == 1 && l4 == 0) ? w10 : a1;
    a1 = (l15 == 1 && l4 == 1) ? r1 : a1;
    a1 = (l15 == 2 && l4 == 0) ? w20 : a1;
    a1 = (l15 == 2 && l4 == 1) ? w21 : a1;
    a1 = (l15 == 2 && l4 == 2) ? r2 : a1;
    a1 = (l15 == 3 && l4 == 0) ? w30 : a1;
    a1 = (l15 == 3 && l4 == 1) ? w31 : a1;
    a1 = (l15 == 3 && l4 == 2) ? w32 : a1;
    a1 = (l15 == 3 && l4 == 3) ? r3 : a1;
    const v4d zero = {0.0, 0.0, 0.0, 0.0};
    // X^T = W S[b0.., :]: register 0 of the result holds X[i][n] in lane i + 16 n
    const v4d xt = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, sg, zero, 0, 0, 0);
    const double x = xt[0];
    S = __builtin_amdgcn_mfma_f64_16x16x4f64(-x, x, S, 0, 0, 0);                   // S -= X X^T  (all four registers)
    const v4d yt = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, E[G], zero, 0, 0, 0);   // Y = W E[b0.., :]
    yfin = yt[0];
    E = __builtin_amdgcn_mfma_f64_16x16x4f64(-x, yfin, E, 0, 0, 0);                // E -= X Y
    // column block g of L (rows on and below its diagonal) goes back to the block in LDS
    if (l15 >= b0 + l4) Sblk[(b0 + l4) * PB_LD + l15] = x;
}

// LDS working set of the blocked 64x64 diagonal factorisation (k_potf2_64b and the fused panel step)
struct Potf2Lds {
    double S[64 * PB_LD];            // S[col * PB_LD + row]
    double Einv[4][16][17];          // inv(L_qq)[row][col] of the four diagonal blocks
};

// Factor the 64x64 block held in P.S (lower triangle valid, strict upper zero).  Called by EVERY thread of the workgroup
// (the barriers are workgroup barriers); threads 0..255 do the work, any further waves only take part in the barriers.
// On return (after the trailing barrier) P.S holds L and P.Einv the inverted diagonal 16x16 blocks.
// The whole 64x64 factorisation on the matrix cores.  Wave 0 runs the critical chain WITHOUT waiting for
// the others: after the 16x16 diagonal block q (potf2m_group x 4) and ONE barrier that publishes L_qq and inv(L_qq), it solves
// block row q + 1 itself (4 MFMAs), updates the next diagonal tile (4 MFMAs) -- which never leaves its registers -- and goes
// straight on to the next block.  Waves 1 and 2 bring the rows below up to date meanwhile (row q + 1 + w: X_i, the X_j it needs
// recomputed rather than waited for, its tiles updated in LDS); the X blocks (final columns of L) are written back one
// barrier later, when nobody reads the S they replace any more.  5 barriers instead of 10, none of them with the chain
// waiting for non-critical work.
__device__ __forceinline__ void potf2b_core_mfma(Potf2Lds& P, int* __restrict__ info, int goff) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    v4d Sr = {0.0, 0.0, 0.0, 0.0};          // wave 0: the current diagonal tile, symmetric, accumulator layout
    v4d Xown = {0.0, 0.0, 0.0, 0.0};        // X[row block of this wave][column block q] of the previous iteration
    if (w == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = l4 + 4 * r, j = l15;
            Sr[r] = (i >= j) ? P.S[j * PB_LD + i] : P.S[i * PB_LD + j];
        }
    }
    // X_i = S_iq inv(L_qq)^T for row block i (accumulator layout = operand layout: register kk is k-slice kk)
    auto solve_rows = [&](int q, int i) {
        v4d x = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const double av = P.Einv[q][l15][4 * kk + l4];
            const double bv = P.S[(16 * q + 4 * kk + l4) * PB_LD + 16 * i + l15];
            x = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, x, 0, 0, 0);
        }
        return x;
    };
#pragma unroll 1
    for (int q = 0; q < 4; ++q) {
        if (w == 0) {
            double* Sqq = &P.S[(16 * q) * PB_LD + 16 * q];
            v4d Er;
#pragma unroll
            for (int r = 0; r < 4; ++r) Er[r] = (l4 + 4 * r == l15) ? 1.0 : 0.0;
            double y0, y1, y2, y3;
            int first_bad = 0;
            potf2m_group<0>(Sr, Er, y0, Sqq, first_bad, lane, l15, l4);
            potf2m_group<1>(Sr, Er, y1, Sqq, first_bad, lane, l15, l4);
            potf2m_group<2>(Sr, Er, y2, Sqq, first_bad, lane, l15, l4);
            potf2m_group<3>(Sr, Er, y3, Sqq, first_bad, lane, l15, l4);
            if (first_bad && lane == 0) atomicCAS(info, 0, goff + 16 * q + first_bad);
            P.Einv[q][l4][l15] = (l15 <= l4) ? y0 : 0.0;
            P.Einv[q][4 + l4][l15] = (l15 <= 4 + l4) ? y1 : 0.0;
            P.Einv[q][8 + l4][l15] = (l15 <= 8 + l4) ? y2 : 0.0;
            P.Einv[q][12 + l4][l15] = (l15 <= 12 + l4) ? y3 : 0.0;
        }
        __syncthreads();
        // the X blocks of the previous iteration become column block q - 1 of L (their inputs are dead now)
        if (q > 0 && w < 3 && q + w < 4) {
            const int i = q + w;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) P.S[(16 * (q - 1) + l4 + 4 * reg) * PB_LD + 16 * i + l15] = Xown[reg];
        }
        if (q == 3) break;
        const int i = q + 1 + w;            // row block of this wave in this iteration
        if (w == 0) {
            Xown = solve_rows(q, i);
            // next diagonal tile, symmetric: S_ii - X_i X_i^T
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int a = l4 + 4 * r, b = l15;
                Sr[r] = (a >= b) ? P.S[(16 * i + b) * PB_LD + 16 * i + a] : P.S[(16 * i + a) * PB_LD + 16 * i + b];
            }
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) Sr = __builtin_amdgcn_mfma_f64_16x16x4f64(-Xown[kk], Xown[kk], Sr, 0, 0, 0);
        } else if (w < 3 && i < 4) {
            Xown = solve_rows(q, i);
            for (int j = q + 1; j <= i; ++j) {
                const v4d xj = (j == i) ? Xown : solve_rows(q, j);
                v4d acc;
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) acc[reg] = P.S[(16 * j + l4 + 4 * reg) * PB_LD + 16 * i + l15];
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-xj[kk], Xown[kk], acc, 0, 0, 0);
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) P.S[(16 * j + l4 + 4 * reg) * PB_LD + 16 * i + l15] = acc[reg];
            }
        }
    }
    __syncthreads();
}

__device__ __forceinline__ void potf2b_store(double* __restrict__ A, int lda, int nb, const Potf2Lds& P, int tid, int nthreads) {
    for (int idx = tid; idx < 4096; idx += nthreads) {
        const int r = idx & 63, c = idx >> 6;
        if (r < nb && c < nb) {
            if (c <= r) A[(size_t)c * lda + r] = P.S[c * PB_LD + r];
            else if ((c >> 4) == (r >> 4)) A[(size_t)c * lda + r] = P.Einv[c >> 4][c & 15][r & 15];
        }
    }
}

__device__ __forceinline__ void syrk_fused_first_block(double* lds, const v4d (&acc)[2][2][2], bool owner, int wj,
                                                       double* __restrict__ C, int ldc, int* __restrict__ info, int goff) {
    static_assert(sizeof(Potf2Lds) <= 4 * SY_BK * SY_LD * sizeof(double), "the block's LDS must fit the operand buffers");
    Potf2Lds& P = *reinterpret_cast<Potf2Lds*>(lds);
    const int tid = threadIdx.x, lane = tid & 63;
    const int l15 = lane & 15, l4 = lane >> 4;
    // (the k-loop ended on a barrier; zero fill and block entries go to disjoint addresses)
    for (int idx = tid; idx < 4096; idx += (int)blockDim.x) {
        const int r = idx & 63, c = idx >> 6;
        if (c > r) P.S[c * PB_LD + r] = 0.0;
    }
    if (owner) {
        // accumulators hold MINUS the updated block: i = 32 p + 2 l15 + s, j = 32 wj + 2 (l4 + 4 r) + tj
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int sx = 0; sx < 2; ++sx)
#pragma unroll
                for (int tj = 0; tj < 2; ++tj)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int i = 32 * p + 2 * l15 + sx;
                        const int j = 32 * wj + 2 * (l4 + 4 * r) + tj;
                        if (i >= j) P.S[j * PB_LD + i] = -acc[p][sx][tj][r];
                    }
    }
    __syncthreads();
    potf2b_core_mfma(P, info, goff);
    potf2b_store(C, ldc, 64, P, tid, (int)blockDim.x);
}

__global__ __launch_bounds__(256) void k_potf2_64b(double* __restrict__ A, int lda, int nb, int* __restrict__ info,
                                                    int goff, long long bstride, int istride) {
    A += (size_t)blockIdx.x * bstride;
    info += (size_t)blockIdx.x * istride;
    __shared__ Potf2Lds P;
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int idx = tid + 256 * k;
        const int r = idx & 63, c = idx >> 6;
        double v = (r == c) ? 1.0 : 0.0;
        if (r < nb && c <= r) v = A[(size_t)c * lda + r];
        P.S[c * PB_LD + r] = v;
    }
    __syncthreads();
    potf2b_core_mfma(P, info, goff);
    potf2b_store(A, lda, nb, P, tid, 256);
}

// precise (potrf_lower(precise = 1)): substitution-based panel kernels (no inverted 16x16 blocks) for the ill-conditioned,
// cached prior covariances (RBF + 1e-6 I, condition number up to 1e11), where the inverse-based solves cost parity digits.
// Otherwise the diagonal blocks come from k_potf2_64b and carry inv(L_qq)^T in their strict upper part, which the
// matrix-core solves and the fused schedules read.
static void potf2_64(hipStream_t s, double* A, int lda, int nb, int* info, int goff, int batch, long long bstride,
                     int istride, bool precise) {
    if (precise)
        NMGP_LAUNCH(k_potf2_64, dim3(batch), dim3(256), 0, s, A, lda, nb, info, goff, bstride, istride);
    else
        NMGP_LAUNCH(k_potf2_64b, dim3(batch), dim3(256), 0, s, A, lda, nb, info, goff, bstride, istride);
}

// ---------------------------------------------------------------------------------------------
// The same update on 64x64 tiles, for launches with FEW tiles on the critical path of a latency-bound factorisation (the
// "near" update of the look-ahead schedule: the next panel's 512 columns).  One 128x128x512 tile keeps one CU's matrix pipes
// busy for ~57 us (8 waves, two per SIMD) however small the launch, and the near update of a single 6144^2 matrix has at most
// 176 such tiles for 256 CUs -- 70 us eleven times per factorisation, against a full-chip bound of 45 us for the first and
// 3 us for the last.  With 64x64 tiles (4 waves of 32x32, 16 MFMAs per k-step and wave) there are four times as many
// workgroups, each a quarter of the work.  Plain masked kernel: no extra-row tricks, any shape.
// info != nullptr: the workgroup of tile (0, 0) -- the next panel's first diagonal block, the first to be dispatched -- goes on
// to factor that block (potf2b_core, as k_potf2_64b would in a launch of its own: 17 us + a launch gap per panel boundary)
// while the other tiles are still being updated.
// ---------------------------------------------------------------------------------------------
#define SS_LD 80
__global__ __launch_bounds__(256) void k_syrk_small(const double* __restrict__ A, int lda, double* __restrict__ C, int ldc,
                                                     int mrows, int ncols, int K, long long bstride, int tiles_pm, int nbatch,
                                                     int tri_row0, int tri_k0, int* __restrict__ info, int istride, int goff) {
    constexpr size_t kOps = 4 * 16 * SS_LD * sizeof(double);
    __shared__ __attribute__((aligned(16))) char smem[sizeof(Potf2Lds) > kOps ? sizeof(Potf2Lds) : kOps];
    double (*sA)[16 * SS_LD] = reinterpret_cast<double (*)[16 * SS_LD]>(smem);
    double (*sB)[16 * SS_LD] = reinterpret_cast<double (*)[16 * SS_LD]>(smem + 2 * 16 * SS_LD * sizeof(double));
    // compact enumeration of the lower-trapezoid 64x64 tiles, column by column (bj = 0: gx tiles, bj = 1: gx - 1, ...)
    const int gx = (mrows + 63) >> 6;
    int bz = (int)blockIdx.x / tiles_pm;
    int idx = (int)blockIdx.x - bz * tiles_pm;
    if (bz >= nbatch) return;
    int bj = 0;
    while (idx >= gx - bj) {
        idx -= gx - bj;
        ++bj;
    }
    const int bi = bj + idx;
    A += (size_t)bz * bstride;
    C += (size_t)bz * bstride;
    const bool diag = bi == bj;
    const int row0 = bi * 64, col0 = bj * 64;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wi = w & 1, wj = w >> 1;
    const int l15 = lane & 15, l4 = lane >> 4;
    // staging: thread (rp, cg): row pair rp (0..31), k-columns cg and cg + 8
    const int rp = tid & 31, cg = tid >> 5;
    const int ri = row0 + 2 * rp, rj = col0 + 2 * rp;
    const int ric = clamp_row_pair(ri, mrows), rjc = clamp_row_pair(rj, mrows);
    const bool ix = ri < mrows, iy = ri + 1 < mrows, jx = rj < mrows, jy = rj + 1 < mrows;
    const bool ish = ix && (ric != ri), jsh = jx && (rjc != rj);
    // two register sets: the k-panel stored to LDS at the end of step kt was requested two steps earlier (one step of 16 MFMAs
    // per wave is shorter than an L2 round trip when a CU holds a single workgroup)
    double2 ra[2][2], rb[2][2];
    auto gload = [&](double2 (&xa)[2], double2 (&xb)[2], int k0) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int kc = k0 + cg + 8 * q;
            const double* colp = A + (size_t)(kc < K ? kc : K - 1) * lda;
            xa[q] = *reinterpret_cast<const double2*>(colp + ric);
            if (!diag) xb[q] = *reinterpret_cast<const double2*>(colp + rjc);
        }
    };
    auto sstore = [&](const double2 (&xa)[2], const double2 (&xb)[2], int buf, int k0) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int kl = cg + 8 * q;
            const bool kin = (k0 + kl) < K;
            double2 va, vb;
            va.x = (kin && ix) ? (ish ? xa[q].y : xa[q].x) : 0.0;
            va.y = (kin && iy) ? xa[q].y : 0.0;
            *reinterpret_cast<double2*>(&sA[buf][kl * SS_LD + 2 * rp]) = va;
            if (!diag) {
                vb.x = (kin && jx) ? (jsh ? xb[q].y : xb[q].x) : 0.0;
                vb.y = (kin && jy) ? xb[q].y : 0.0;
                *reinterpret_cast<double2*>(&sB[buf][kl * SS_LD + 2 * rp]) = vb;
            }
        }
    };
    const bool active = !(diag && (wi * 32 + 31 < wj * 32));
    const int nk = (K + 15) / 16;
    int kt0 = 0;                                  // leading all-zero k-panels of triangular rows (see syrk_tile_body)
    if (row0 >= tri_row0 && row0 - tri_row0 - tri_k0 > 0) kt0 = (row0 - tri_row0 - tri_k0) / 16;
    if (kt0 > nk - 1) kt0 = nk - 1;
    const int fresh0 = tri_row0 == 0x7fffffff ? 0x7fffffff : tri_row0 + tri_k0;     // rows whose C nobody has written yet
    gload(ra[0], rb[0], kt0 * 16);
    gload(ra[1], rb[1], (kt0 + 1) * 16);
    // acc[tj][ti][r]: C element (i, j), i = row0 + 32 wi + 16 ti + l15, j = col0 + 32 wj + 16 tj + l4 + 4 r
    v4d acc[2][2];
#pragma unroll
    for (int tj = 0; tj < 2; ++tj)
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = row0 + wi * 32 + ti * 16 + l15;
                const int j = col0 + wj * 32 + tj * 16 + l4 + 4 * r;
                acc[tj][ti][r] = (active && i < mrows && j < ncols && i >= j && i < fresh0) ? C[(size_t)j * ldc + i] : 0.0;
            }
    sstore(ra[0], rb[0], 0, kt0 * 16);
    gload(ra[0], rb[0], (kt0 + 2) * 16);
    __syncthreads();
    auto compute = [&](int cur) {
        if (!active) return;
        const double* tA = sA[cur] + wi * 32 + l15 + l4 * SS_LD;
        const double* tB = (diag ? sA[cur] : sB[cur]) + wj * 32 + l15 + l4 * SS_LD;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const double fa0 = tA[kk * 4 * SS_LD], fa1 = tA[kk * 4 * SS_LD + 16];
            const double fb0 = -tB[kk * 4 * SS_LD], fb1 = -tB[kk * 4 * SS_LD + 16];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(fb0, fa0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(fb0, fa1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(fb1, fa0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(fb1, fa1, acc[1][1], 0, 0, 0);
        }
    };
    // step kt (buffer parity = (kt - kt0) & 1): multiply from the current buffer, store panel kt + 1 (register set of the
    // opposite parity) into the other one, re-use that register set for panel kt + 3
    for (int kt = kt0; kt < nk; kt += 2) {
        compute(0);
        if (kt + 1 < nk) {
            sstore(ra[1], rb[1], 1, (kt + 1) * 16);
            if (kt + 3 < nk) gload(ra[1], rb[1], (kt + 3) * 16);
        }
        __syncthreads();
        if (kt + 1 >= nk) break;
        compute(1);
        if (kt + 2 < nk) {
            sstore(ra[0], rb[0], 0, (kt + 2) * 16);
            if (kt + 4 < nk) gload(ra[0], rb[0], (kt + 4) * 16);
        }
        __syncthreads();
    }
    if (info != nullptr && bi == 0 && bj == 0) {
        // the k-loop ended on a barrier: the operand buffers are free, the block moves from the accumulators into P.S
        Potf2Lds& P = *reinterpret_cast<Potf2Lds*>(smem);
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int idx = tid + 256 * k;
            const int r = idx & 63, c = idx >> 6;
            if (c > r) P.S[c * PB_LD + r] = 0.0;
        }
        if (active) {
#pragma unroll
            for (int tj = 0; tj < 2; ++tj)
#pragma unroll
                for (int ti = 0; ti < 2; ++ti)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int i = wi * 32 + ti * 16 + l15;
                        const int j = wj * 32 + tj * 16 + l4 + 4 * r;
                        if (i >= j) P.S[j * PB_LD + i] = acc[tj][ti][r];
                    }
        }
        __syncthreads();
        potf2b_core_mfma(P, info + (size_t)bz * istride, goff);
        potf2b_store(C, ldc, 64, P, tid, 256);
        return;
    }
    if (active) {
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
#pragma unroll
            for (int ti = 0; ti < 2; ++ti)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = row0 + wi * 32 + ti * 16 + l15;
                    const int j = col0 + wj * 32 + tj * 16 + l4 + 4 * r;
                    if (i < mrows && j < ncols && i >= j) C[(size_t)j * ldc + i] = acc[tj][ti][r];
                }
    }
}

// finfo != nullptr asks the launch to go on and factor the diagonal block in its tile (0, 0) -- the first block of the panel
// part that starts at column `goff`, status words finfo + b * fistride (k_syrk_small / k_syrk_lower: potf2b_core, as k_potf2_64b
// would in a launch of its own).  Returns whether the launch does so (its shape must allow it).
bool syrk_lower(hipStream_t s, const double* A, int lda, double* C, int ldc, int mrows, int ncols, int K, int batch,
                long long bstride, long long cstride, int ktri, int tri_row0, int tri_k0, int* finfo, int fistride, int goff,
                const SyrkHook* hook) {
    if (mrows <= 0 || ncols <= 0 || K <= 0) return false;
    const SyrkPlan pl = syrk_plan(lda, ldc, mrows, ncols, K, batch, ktri, false, tri_row0 != kNoTriRows);
    const long long cs = cstride < 0 ? bstride : cstride;
    void* tok = nullptr;
    if (hook && hook->begin) {
        // algorithmic flop of this launch: 2 K per element (i >= j) of the mrows x ncols lower trapezoid
        const double elems = (double)ncols * mrows - 0.5 * (double)ncols * (ncols - 1);
        tok = hook->begin(hook->user, s, 2.0 * K * elems * batch, 8.0 * batch * (2.0 * elems + (double)mrows * K));
    }
    bool fused;
    // few 128x128 tiles (at most one per CU) and a k-loop long enough to matter: 64x64 tiles (k_syrk_small)
    // (latency regime only: the throughput batches keep one update kernel, whose launches the profiling tools replay)
    // (round 3 tried the 64x64-tile kernel -- three workgroups per CU -- for the K = 64 / 128 updates of the big batches as well: 128
    // chains +0.3 % at K <= 64, -0.5 % at K <= 128; not kept)
    if (!ktri && K >= 128 && batch <= 16 && (long long)pl.tiles * batch <= switches().syrk_small_max && cs == bstride &&
        (lda & 1) == 0 && mrows >= 2) {
        const int gx = (mrows + 63) / 64, gy = (ncols + 63) / 64;
        int tiles = 0;
        for (int bj = 0; bj < gy; ++bj) tiles += gx - bj > 0 ? gx - bj : 0;
        fused = finfo != nullptr && mrows >= 64 && ncols >= 64;
        NMGP_LAUNCH(k_syrk_small, dim3((unsigned)(tiles * batch)), dim3(256), 0, s, A, lda, C, ldc, mrows, ncols, K, bstride, tiles,
                    batch, tri_row0, tri_k0, fused ? finfo : (int*)nullptr, fistride, goff);
    } else {
        // the NEXT diagonal block inside tile (0, 0): only where that tile takes the mask-free path (the conditions of
        // syrk_tile_body); the launch then uses the compact 1-D enumeration, whose fused form deals tile (0, 0) of every matrix first
        fused = finfo != nullptr && !ktri && cs == bstride && pl.mrows >= SY_BM && (ncols >= SY_BM || ncols == 64) &&
                (K & 31) == 0 && (long long)(K + 16) * lda * 8 < 0x7fff0000LL;
        SyrkPlan pf = pl;
        if (fused && pf.swz == 0) {
            pf.grid = dim3((unsigned)((long long)pf.tiles * batch), 1, 1);
            pf.swz = -pf.tiles;
        }
        NMGP_LAUNCH(k_syrk_lower, pf.grid, dim3(512), 0, s, A, lda, C, ldc, pf.mrows, ncols, K, bstride, cs, pf.kflags,
                    pf.swz, batch, tri_row0, tri_k0, fused ? finfo : (int*)nullptr, fistride, goff);
    }
    if (tok && hook->end) hook->end(hook->user, tok);
    return fused;
}

int syrk_schur(hipStream_t s, const double* X, int lda, int N, int M, int batch, const SchurEpi& e) {
    if (N <= 0) return 0;
    if (M < 2 || M > 8) return NMGP_E_UNSUPPORTED;
    // the tile plan of syrk_lower(X, lda, C, ., N, N, N, batch, bs, bs, 2)
    const SyrkPlan pl = syrk_plan(lda, lda, N, N, N, batch, 2, false);
    switch (M) {
#define SCHUR_CASE(m) \
        case m: NMGP_LAUNCH(k_syrk_schur<m>, pl.grid, dim3(512), 0, s, X, lda, pl.mrows, e.bstride, pl.kflags, pl.swz, batch, e); break;
        SCHUR_CASE(2) SCHUR_CASE(3) SCHUR_CASE(4) SCHUR_CASE(5) SCHUR_CASE(6) SCHUR_CASE(7) SCHUR_CASE(8)
#undef SCHUR_CASE
    }
    return 0;
}


// ---------------------------------------------------------------------------------------------
// panel solve  X L^T = A  (L: nb x nb lower, nb <= 64; A: rows x nb, overwritten by X)
// four lanes per row: lane g of a row owns columns k = 4 kk + g in registers; the dot product of step c is split
// over the four lanes and combined with two DPP quad permutes.
// ---------------------------------------------------------------------------------------------
template <int SRC>
__device__ inline double quad_bcast(double v) {
    // value of lane (4 q + SRC) for every lane of quad q: DPP quad_perm [SRC, SRC, SRC, SRC]
    constexpr int ctrl = SRC | (SRC << 2) | (SRC << 4) | (SRC << 6);
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_mov_dpp(lo, ctrl, 0xF, 0xF, true);
    hi = __builtin_amdgcn_mov_dpp(hi, ctrl, 0xF, 0xF, true);
    return __hiloint2double(hi, lo);
}

template <int KC, int GC>
__device__ __forceinline__ void trsm_step(double (&x)[16], const double (*Lm)[65], const double* rinv, int g) {
    constexpr int c = 4 * KC + GC;
    // owner lane (g == GC) finalises column c, the quad receives it, everyone retires column c from its own columns
    double xc = x[KC] * rinv[c];
    xc = quad_bcast<GC>(xc);
    if (g == GC) x[KC] = xc;
    double t[16];
#pragma unroll
    for (int kk = KC; kk < 16; ++kk) t[kk] = Lm[4 * kk + g][c];      // unconditional reads (see k_potf2_64)
    {
        const double upd = x[KC] - xc * t[KC];
        x[KC] = (g > GC) ? upd : x[KC];
    }
#pragma unroll
    for (int kk = KC + 1; kk < 16; ++kk) x[kk] -= xc * t[kk];
}

template <int KC>
__device__ __forceinline__ void trsm_steps4(double (&x)[16], const double (*Lm)[65], const double* rinv, int g) {
    trsm_step<KC, 0>(x, Lm, rinv, g);
    trsm_step<KC, 1>(x, Lm, rinv, g);
    trsm_step<KC, 2>(x, Lm, rinv, g);
    trsm_step<KC, 3>(x, Lm, rinv, g);
}

__global__ __launch_bounds__(256) void k_trsm_64(const double* __restrict__ L, int ldl, int nb, double* __restrict__ A,
                                                  int lda, int rows, long long bstride) {
    L += (size_t)blockIdx.y * bstride;
    A += (size_t)blockIdx.y * bstride;
    __shared__ double Lm[64][65];
    __shared__ double rinv[64];
    const int tid = threadIdx.x;
    const int lr = tid >> 2, g = tid & 3;
    const int row = blockIdx.x * 64 + lr;
    const bool valid = row < rows;
    // both global fetches (this thread's row of A and its share of the factor) are issued before the first wait
    double x[16], lv[16];
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
        const int k = 4 * kk + g;
        x[kk] = (valid && k < nb) ? A[(size_t)k * lda + row] : 0.0;
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int idx = tid + 256 * q;
        const int r = idx & 63, c = idx >> 6;
        double v = (r == c) ? 1.0 : 0.0;
        if (r < nb && c <= r) v = L[(size_t)c * ldl + r];
        lv[q] = v;
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int idx = tid + 256 * q;
        Lm[idx & 63][idx >> 6] = lv[q];
    }
    __syncthreads();
    if (tid < 64) rinv[tid] = 1.0 / Lm[tid][tid];
    __syncthreads();
    trsm_steps4<0>(x, Lm, rinv, g);   trsm_steps4<1>(x, Lm, rinv, g);   trsm_steps4<2>(x, Lm, rinv, g);
    trsm_steps4<3>(x, Lm, rinv, g);   trsm_steps4<4>(x, Lm, rinv, g);   trsm_steps4<5>(x, Lm, rinv, g);
    trsm_steps4<6>(x, Lm, rinv, g);   trsm_steps4<7>(x, Lm, rinv, g);   trsm_steps4<8>(x, Lm, rinv, g);
    trsm_steps4<9>(x, Lm, rinv, g);   trsm_steps4<10>(x, Lm, rinv, g);  trsm_steps4<11>(x, Lm, rinv, g);
    trsm_steps4<12>(x, Lm, rinv, g);  trsm_steps4<13>(x, Lm, rinv, g);  trsm_steps4<14>(x, Lm, rinv, g);
    trsm_steps4<15>(x, Lm, rinv, g);
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
        const int k = 4 * kk + g;
        if (valid && k < nb) A[(size_t)k * lda + row] = x[kk];
    }
}

// ---------------------------------------------------------------------------------------------
// panel solve on the matrix cores.  The VALU substitution above spends ~550 FP64 FMAs + LDS reads per lane and, on
// gfx950, FP64 VALU work and FP64 MFMAs share the SIMD: k_trsm_64 ran at 2.4 TB/s.  Here the 64 columns are split
// into four 16-column blocks:  X_q = (A_q - sum_{p<q} X_p L_qp^T) inv(L_qq)^T  with every product a chain of
// v_mfma_f64_16x16x4_f64.  The workgroup stages L in LDS -- the inverted 16x16 diagonal blocks come with it: k_potf2_64b
// leaves inv(L_qq)^T in their strict upper part -- and lays -L_qp and inv(L_qq) out in LDS in MFMA A-operand order.  The
// accumulator layout of one product (lane: matrix row l & 15, columns (l >> 4) + 4 reg) IS the B-operand layout of
// the next one (k-slice reg), so the rows stay in registers from load to store.
// A workgroup (4 waves) handles 128 rows, a wave two interleaved 16-row chunks (rows 2(l & 15) + s: 16-byte accesses).
// trsm_64 launches it for the partial blocks (nb < 64); full blocks take k_trsm_64h below.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_trsm_64m(const double* __restrict__ L, int ldl, int nb, double* __restrict__ A,
                                                   int lda, int rows, long long bstride, int reps) {
    L += (size_t)blockIdx.y * bstride;
    A += (size_t)blockIdx.y * bstride;
    __shared__ double Lm[64][65];
    __shared__ double Linv[4][16][17];
    __shared__ v4d ops[10][64];                   // ops[blk][lane] = the four k-slices of the lane's A operand
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    // the workgroup handles `reps` groups of 128 rows (the factor preparation is paid once); wave w of group it owns rows
    // rbase, rbase + 1 with rbase = (blockIdx.x * reps + it) * 128 + 32 w + 2 (lane & 15)
    int rbase = blockIdx.x * reps * 128 + w * 32 + 2 * l15;
    v4d T[2][4];
    auto load_rows = [&]() {
        const bool v0 = rbase < rows, v1 = rbase + 1 < rows;
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int col = 16 * q + 4 * r + l4;
                double2 v = make_double2(0.0, 0.0);
                if (v0 && col < nb) v = *reinterpret_cast<const double2*>(&A[(size_t)col * lda + rbase]);
                T[0][q][r] = v.x;
                T[1][q][r] = v1 ? v.y : 0.0;
            }
    };
    // the first group's rows are issued first, so that their latency hides under the factor preparation
    load_rows();
    {
        double lv[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int idx = tid + 256 * q;
            const int r = idx & 63, c = idx >> 6;
            double v = (r == c) ? 1.0 : 0.0;
            // the strict upper part of the diagonal 16x16 blocks holds inv(L_qq)^T (written by k_potf2_64b)
            if (r < nb && c < nb && (c <= r || (c >> 4) == (r >> 4))) v = L[(size_t)c * ldl + r];
            lv[q] = v;
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int idx = tid + 256 * q;
            Lm[idx & 63][idx >> 6] = lv[q];
        }
    }
    __syncthreads();
    {
        // inv(L_qq)[i][j] (i > j) sits at Lm[16 q + j][16 q + i]; the diagonal is 1 / L_ii
        const int qq = tid >> 6, i = (tid >> 2) & 15, j0 = (tid & 3) * 4;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const int j = j0 + jj;
            double v = 0.0;
            if (j < i) v = Lm[16 * qq + j][16 * qq + i];
            else if (j == i) v = 1.0 / Lm[16 * qq + i][16 * qq + i];
            Linv[qq][i][j] = v;
        }
    }
    __syncthreads();
    // A-operand order: ops[blk][kk][l] = M[row = l & 15][k = 4 kk + (l >> 4)]; blk 0..5 = -L_qp (q = 1: p0; q = 2: p0, p1;
    // q = 3: p0, p1, p2), blk 6 + q = inv(L_qq)
#pragma unroll
    for (int e = 0; e < 10; ++e) {
        const int idx = tid + 256 * e;               // 0 .. 2559
        const int blk = idx >> 8, kk = (idx >> 6) & 3, l = idx & 63;
        const int rr = l & 15, kc = 4 * kk + (l >> 4);
        double v;
        if (blk < 6) {
            const int q = blk == 0 ? 1 : (blk < 3 ? 2 : 3);
            const int pp = blk == 0 ? 0 : (blk < 3 ? blk - 1 : blk - 3);
            v = -Lm[16 * q + rr][16 * pp + kc];
        } else {
            v = (kc <= rr) ? Linv[blk - 6][rr][kc] : 0.0;
        }
        reinterpret_cast<double*>(&ops[blk][l])[kk] = v;
    }
    __syncthreads();
    for (int it = 0; it < reps; ++it) {
        // wave-uniform exit only: the MFMAs below need every lane of the wave active (A-operand rows live in all 64 lanes)
        if ((blockIdx.x * reps + it) * 128 + w * 32 >= rows) return;
        if (it > 0) load_rows();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
#pragma unroll
            for (int pp = 0; pp < q; ++pp) {
                const int blk = (q == 1 ? 0 : (q == 2 ? 1 : 3)) + pp;
                const v4d av = ops[blk][lane];
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    T[0][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[kk], T[0][pp][kk], T[0][q], 0, 0, 0);
                    T[1][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[kk], T[1][pp][kk], T[1][q], 0, 0, 0);
                }
            }
            v4d x0 = {0.0, 0.0, 0.0, 0.0}, x1 = {0.0, 0.0, 0.0, 0.0};
            const v4d ai = ops[6 + q][lane];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                x0 = __builtin_amdgcn_mfma_f64_16x16x4f64(ai[kk], T[0][q][kk], x0, 0, 0, 0);
                x1 = __builtin_amdgcn_mfma_f64_16x16x4f64(ai[kk], T[1][q][kk], x1, 0, 0, 0);
            }
            T[0][q] = x0;
            T[1][q] = x1;
        }
        const bool v0 = rbase < rows, v1 = rbase + 1 < rows;
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int col = 16 * q + 4 * r + l4;
                if (col < nb) {
                    if (v1) *reinterpret_cast<double2*>(&A[(size_t)col * lda + rbase]) = make_double2(T[0][q][r], T[1][q][r]);
                    else if (v0) A[(size_t)col * lda + rbase] = T[0][q][r];
                }
            }
        rbase += 128;
    }
}

// The common case -- a full 64-column block -- with the operands built straight from global memory / L2: no staging of L, no
// inversion, 20 KB of LDS.  The solve is a chain of dependent MFMAs; only more waves per SIMD put more independent chains on the
// matrix pipe.  ONE 16-row chunk per wave (64 rows per workgroup, 84 VGPRs, no spills): six workgroups per CU.  The solve is bound
// by HBM at 81 % of what in-place panel accesses reach on this chip; what limits it is how many workgroups of a CU are in
// their load phase at a time, not the matrix pipe (40 MFMAs per wave against 64 KB moved per workgroup).
// Measured against two interleaved 16-row chunks per wave at four workgroups per CU (same box, alternating): 128 chains
// 775.4-776.7 -> 779.3-780.3 evals/s, value+gradient 256.4 -> 258.9, 16 chains 667 -> 676, one chain unchanged; with
// __launch_bounds__(256, 6) the compiler spills 4 registers and half the gain is lost.
template <int OCC>
__global__ __launch_bounds__(256, OCC) void k_trsm_64h(const double* __restrict__ L, int ldl, double* __restrict__ A, int lda,
                                                        int rows, long long bstride) {
    L += (size_t)blockIdx.y * bstride;
    A += (size_t)blockIdx.y * bstride;
    __shared__ v4d ops[10][64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int row = blockIdx.x * 64 + w * 16 + l15;
    const bool v0 = row < rows;
    const int rowc = v0 ? row : rows - 1;
    v4d T[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r) T[q][r] = A[(size_t)(16 * q + 4 * r + l4) * lda + rowc];
#pragma unroll
    for (int e = 0; e < 10; ++e) {
        const int idx = tid + 256 * e;
        const int blk = idx >> 8, kk = (idx >> 6) & 3, l = idx & 63;
        const int rr = l & 15, kc = 4 * kk + (l >> 4);
        double v;
        if (blk < 6) {
            const int q = blk == 0 ? 1 : (blk < 3 ? 2 : 3);
            const int pp = blk == 0 ? 0 : (blk < 3 ? blk - 1 : blk - 3);
            v = -L[(size_t)(16 * pp + kc) * ldl + 16 * q + rr];
        } else {
            const int q = blk - 6;
            if (kc < rr) v = L[(size_t)(16 * q + rr) * ldl + 16 * q + kc];
            else if (kc == rr) v = 1.0 / L[(size_t)(16 * q + rr) * ldl + 16 * q + rr];
            else v = 0.0;
        }
        reinterpret_cast<double*>(&ops[blk][l])[kk] = v;
    }
    __syncthreads();
    if (blockIdx.x * 64 + w * 16 >= rows) return;               // wave-uniform (the MFMAs need every lane)
    // right-looking order: once X_p is solved, its updates of the blocks q > p are independent of each other (up to three
    // accumulator chains in flight instead of one)
#pragma unroll
    for (int pp = 0; pp < 4; ++pp) {
        const v4d ai = ops[6 + pp][lane];
        v4d x0 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) x0 = __builtin_amdgcn_mfma_f64_16x16x4f64(ai[kk], T[pp][kk], x0, 0, 0, 0);
        T[pp] = x0;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
            for (int q = pp + 1; q < 4; ++q) {
                const double a = reinterpret_cast<const double*>(&ops[(q == 1 ? 0 : (q == 2 ? 1 : 3)) + pp][lane])[kk];
                T[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, T[pp][kk], T[q], 0, 0, 0);
            }
    }
    if (v0) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) A[(size_t)(16 * q + 4 * r + l4) * lda + row] = T[q][r];
    }
}

static void trsm_64(hipStream_t s, const double* L, int ldl, int nb, double* A, int lda, int rows, int batch,
                    long long bstride, bool precise) {
    if (rows <= 0) return;
    if (precise) {
        NMGP_LAUNCH(k_trsm_64, dim3(cdiv_c(rows, 64), batch), dim3(256), 0, s, L, ldl, nb, A, lda, rows, bstride);
    } else if (nb == 64) {
        NMGP_LAUNCH(k_trsm_64h<5>, dim3(cdiv_c(rows, 64), batch), dim3(256), 0, s, L, ldl, A, lda, rows, bstride);
    } else {
        // groups of 128 rows per workgroup: more of them amortise the factor preparation once the launch would fill the
        // chip (512 resident workgroups) several times over anyway
        const long long wgs = (long long)cdiv_c(rows, 128) * batch;
        const int reps = wgs >= 4096 ? 4 : (wgs >= 2048 ? 2 : 1);
        NMGP_LAUNCH(k_trsm_64m, dim3(cdiv_c(rows, 128 * reps), batch), dim3(256), 0, s, L, ldl, nb, A, lda, rows, bstride, reps);
    }
}

// ---------------------------------------------------------------------------------------------
// Fused panel step: ONE launch per 64-column step of a panel instead of three dependent ones (diagonal block, panel solve,
// K = 64 update).  A single matrix (or a handful of subjects) is latency-bound: 96 steps x (17 + 12 + 20 us) is the whole
// evaluation time at n = 6144.  The dependency that forces three launches is that the update of step k must reach the next
// diagonal block before it can be factored.  Here the update is DELAYED by one step and the next diagonal block is factored
// by look-ahead inside the same launch:
//
//   state before step k (columns ck .. ck+63, ck = c0 + 64 k, panel = columns [c0, pend)):
//     * columns < ck are final; the diagonal block (ck, ck) is factored, inverted 16x16 blocks in its upper part;
//     * rows >= ck + 64 of the panel columns >= ck have received every column block < k - 1, but NOT block k - 1.
//   step k, workgroups 0 .. T-1 ("solve" role, rows >= ck + 64; workgroup 0: the 64 rows of block row k + 1, the others
//   8 waves x 16 rows each):
//     1. catch-up: C[rows, block k] and C[rows, block k+1] -= X[rows, block k-1] L[.., block k-1]^T   (K = 64, MFMA; the
//        operands are final since the previous launch, so no workgroup waits for another);
//     2. solve: X[rows, block k] = C[rows, block k] inv(L_kk)^T  (the 16x16-blocked scheme of k_trsm_64h);
//     3. workgroup 0 only -- it owns block row k+1: D = C[k+1, k+1] - X[k+1, k] X[k+1, k]^T, factor D (potf2b_core) and
//        store it: the diagonal block of step k + 1 is ready when this launch ends;
//   workgroups T .. ("update" role): the catch-up of the remaining panel columns >= ck + 128, rows >= ck + 128, with the
//     same column block k - 1 -- ordinary k_syrk_lower tiles (syrk_tile_body) that fill the other CUs meanwhile.
//   After the last step of the panel nothing is pending inside it: the trailing update applies all panel columns at once.
// Critical path per step: one launch, two K = 64 MFMA passes over 64 rows, the 64x64 factorisation.
// ---------------------------------------------------------------------------------------------
#define PS_XLD 66
#define PS_XPS_OFF 6656                                  // after opsC (4096 doubles) and opsT (2560)
#define PS_XS_OFF (PS_XPS_OFF + 64 * PS_XLD)
#define PS_SMEM_DOUBLES (PS_XS_OFF + 64 * PS_XLD)        // 15104 doubles = 118 KB (the factorisation's LDS aliases the operands)

// MODE 0: the general step.  MODE 1 / 2: the two steps of a 128-column LEAF of the throughput schedule (big batches: recursive
// halving down to 128 columns, then these two launches instead of diagonal block + solve + K = 64 update + diagonal block + solve:
// the K = 64 update is folded into the second step's solve, 5 passes over the rows' column blocks instead of 7):
//   MODE 1 = first step  (no previous block, a next one; no update role, no P waves): solve + the critical workgroup's D and its
//            factorisation; 54 KB of LDS;
//   MODE 2 = second step (a previous block, no next one): catch-up + solve; 52 KB of LDS.
// With the flags known at compile time at most two 64-column row blocks are live per thread: 96 / 110 VGPRs (OCC = 4), two workgroups
// per CU, so that one's loads travel under the other's MFMAs and stores (the general step holds three blocks in 191 VGPRs, one per
// CU).  The second step runs at OCC = 6: three workgroups per CU (80 VGPRs, 3 x 53 KB of LDS), which it reaches without spilling by
// issuing its row loads only after its operands have gone to LDS (against OCC = 4: 128 chains +0.35 %, 64 subjects +0.8 %); the
// first step does not (its critical workgroup's factorisation wants ~100 registers: 168 spilled, -1 % at 16 chains), it stays at 4.
template <int MODE, int OCC = 2>
__global__ __launch_bounds__(512, OCC) void k_panel_step(double* __restrict__ Ab, int lda, int ck, int has_prev_a,
                                                        int has_next_a,
                                                        int m_act, int pend, long long bstride, int* __restrict__ info,
                                                        int istride, int T, int u_mrows, int u_ncols, int u_kflags,
                                                        int u_tiles, int nbatch, int pre_a, int un_fresh, int u_tri,
                                                        long long* __restrict__ stamps) {
    const int has_prev = MODE == 0 ? has_prev_a : (MODE == 2 ? 1 : 0);
    const int has_next = MODE == 0 ? has_next_a : (MODE == 1 ? 1 : 0);
    const int pre = MODE == 0 ? pre_a : 0;
    constexpr int kOpsT = MODE == 1 ? 0 : 4096;                         // doubles; MODE 1 stages no catch-up operands (opsC)
    constexpr int kXps = PS_XPS_OFF;                                    // (MODE 0 only)
    constexpr int kXs = MODE == 1 ? 2560 : PS_XS_OFF;
    constexpr int kSmem = MODE == 1 ? 2560 + 64 * PS_XLD
                                    : (MODE == 2 ? 6656 : (PS_SMEM_DOUBLES > 4 * SY_BK * SY_LD ? PS_SMEM_DOUBLES : 4 * SY_BK * SY_LD));
    static_assert(MODE != 1 || sizeof(Potf2Lds) <= kSmem * sizeof(double), "the factorisation's LDS aliases the step's");
    // un_fresh / u_tri (gradient evaluations; 0x7fffffff otherwise): rows >= un_fresh (absolute) are rows of L^-T whose
    // entries in column block k + 1 nobody has written yet (they start from zero); u_tri = the same boundary for the update
    // role, relative to its C origin (see potrf_lower on "fresh" rows)
    // developer aid (NMGP_STEP_STAMPS=<file>): thread 0 of workgroup 0 of matrix 0 records the 100 MHz wall clock at the
    // phase boundaries of the critical workgroup
#define PS_STAMP(i)                                                              \
    do {                                                                         \
        if (stamps && blockIdx.x == 0 && threadIdx.x == 0) stamps[i] = (long long)wall_clock64(); \
    } while (0)
    PS_STAMP(0);
    __shared__ __attribute__((aligned(32))) double smem[kSmem];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    // 1-D grid, role-major: workgroup id = role index * nbatch + matrix.  The dispatcher hands out workgroups in id order,
    // so the critical workgroup 0 of EVERY matrix starts in the first round (with matrix-major order the last subjects'
    // critical workgroups of an 8-subject batch queued behind ~270 others and started one round late), and consecutive ids
    // -- the same role of different matrices -- land on different XCDs.
    const int bx = (int)blockIdx.x / nbatch, by = (int)blockIdx.x - bx * nbatch;
    if (bx >= T) {
        // ---- update role: one 128x128 tile of the delayed K = 64 update of the remaining panel columns ----
        if constexpr (MODE == 0) {
            const int t = bx - T + by * u_tiles;       // compact tile index over the batch
            const double* Ap = Ab + (size_t)(ck - 64) * lda + (ck + 128);
            double* Cp = Ab + (size_t)(ck + 128) * lda + (ck + 128);
            syrk_tile_body<4, SY_BK>(Ap, lda, Cp, lda, u_mrows, u_ncols, 64, bstride, bstride, u_kflags, -u_tiles, nbatch, t, 0,
                                     0, smem, smem + 2 * SY_BK * SY_LD, u_tri, 0);
        }
        return;
    }
    // ---- solve role ----
    double* A = Ab + (size_t)by * bstride;
    v4d* opsC = reinterpret_cast<v4d*>(smem);                    // [4 q][4 sg][64 lanes]: -L[cb + 16 q + i][4 (4 sg + kk) + l4]
    v4d* opsT = reinterpret_cast<v4d*>(smem + kOpsT);            // [10][64 lanes], as in k_trsm_64h
    double* Xps = smem + (MODE == 0 ? kXps : 0);                 // [64][PS_XLD]: X[k+2, k-1] (the P waves; MODE 0 only)
    double* Xs = smem + (MODE == 2 ? 0 : kXs);                   // [64][PS_XLD]: X[k+1, k]   (workgroup 0; not in MODE 2)
    // Workgroup 0 owns the critical block row k + 1 ("C", waves 0..3: its diagonal block is factored at the end of this
    // launch) and nothing else: its waves 4..7 only take part in the barriers.  The FP64 matrix pipe of a SIMD is shared by
    // the waves on it, and the ~230 MFMAs per wave that lead up to the factorisation ARE the critical path; a second block
    // row on the same CU doubled them (measured: 12.4 us against 7).
    const bool wg0 = bx == 0;
    const bool isC = wg0 && w < 4;
    // Workgroup 1, waves 0..3 ("P"): block row k + 2, the critical rows of the NEXT launch.  They bring their own diagonal
    // block (k+2, k+2) fully up to date -- column block k - 1 (its pending update, taken over from the update role, which
    // skips that 64x64 block: flag 128) AND column block k (both operands are their own rows: X[k+2, k-1], X[k+2, k]) -- so
    // that next launch's C finds only ONE pass left between its solve and the factorisation.  `pre` = block k + 2 is inside
    // the panel.
    const bool wg1 = pre && bx == 1;
    const bool isP = wg1 && w < 4;
    const int row = wg0 ? ck + 64 + 16 * w + l15 : ck + 128 + 128 * (bx - 1) + 16 * w + l15;
    const bool rv = row < m_act && !(wg0 && w >= 4);
    const int rowc = row < m_act ? row : (m_act - 1);            // clamped: loads stay in bounds, results are masked
    // column block k + 1 of this thread's row: the critical workgroup needs it for D, the others for its catch-up with column
    // block k - 1 -- in the first step of a panel (no k - 1) they neither read nor write it
    const bool un_used = has_next && (has_prev || wg0);
    // (1) issue every global load this thread needs up front
    double oc[8], ot[5];
    v4d Xp[4], Tk[4], Un[4];
    const double* Lp = A + (size_t)(ck - 64) * lda;               // column block k - 1
    if (has_prev) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int e = tid + 512 * j, q = e >> 10, sx = (e >> 6) & 15, l = e & 63;
            oc[j] = -Lp[(size_t)(4 * sx + (l >> 4)) * lda + ck + 16 * q + (l & 15)];
        }
    }
    {
        const double* L = A + (size_t)ck * lda + ck;              // diagonal block k (factor + inverted 16x16 blocks)
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const int idx = tid + 512 * j;                        // 0 .. 2559
            const int blk = idx >> 8, kk = (idx >> 6) & 3, l = idx & 63;
            const int rr = l & 15, kc = 4 * kk + (l >> 4);
            double v;
            if (blk < 6) {
                const int q = blk == 0 ? 1 : (blk < 3 ? 2 : 3);
                const int pp = blk == 0 ? 0 : (blk < 3 ? blk - 1 : blk - 3);
                v = -L[(size_t)(16 * pp + kc) * lda + 16 * q + rr];
            } else {
                const int q = blk - 6;                   // inv(L_qq)[rr][kc] (kc < rr) sits at row 16 q + kc, column 16 q + rr
                if (kc < rr) v = L[(size_t)(16 * q + rr) * lda + 16 * q + kc];
                else if (kc == rr) v = 1.0 / L[(size_t)(16 * q + rr) * lda + 16 * q + rr];
                else v = 0.0;
            }
            ot[j] = v;
        }
    }
    auto load_rows = [&]() {
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = 16 * q + 4 * r + l4;
                Tk[q][r] = rv ? A[(size_t)(ck + c) * lda + rowc] : 0.0;
                Xp[q][r] = (rv && has_prev) ? Lp[(size_t)c * lda + rowc] : 0.0;
                Un[q][r] = (rv && un_used && row < un_fresh) ? A[(size_t)(ck + 64 + c) * lda + rowc] : 0.0;
            }
    };
    if constexpr (MODE != 2) load_rows();
    // (2) operands to LDS
    if (has_prev) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int e = tid + 512 * j, q = e >> 10, sx = (e >> 6) & 15, l = e & 63;
            smem[((q * 4 + (sx >> 2)) * 64 + l) * 4 + (sx & 3)] = oc[j];
        }
        if (isP) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int r = 0; r < 4; ++r) Xps[(16 * w + l15) * PS_XLD + 16 * q + 4 * r + l4] = Xp[q][r];
        }
    }
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const int idx = tid + 512 * j;
        const int blk = idx >> 8, kk = (idx >> 6) & 3, l = idx & 63;
        smem[kOpsT + (blk * 64 + l) * 4 + kk] = ot[j];
    }
    if constexpr (MODE == 2) load_rows();      // (the operand registers are free again: 80 VGPRs, three workgroups per CU)
    __syncthreads();
    PS_STAMP(1);
    // operands of the second catch-up (column block k + 1) travel while the first one computes (workgroup 0 takes them
    // from Xps instead: they ARE block row k + 1 of column block k - 1)
    if (has_prev && has_next && !wg0) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int e = tid + 512 * j, q = e >> 10, sx = (e >> 6) & 15, l = e & 63;
            oc[j] = -Lp[(size_t)(4 * sx + (l >> 4)) * lda + ck + 64 + 16 * q + (l & 15)];
        }
    }
    // (3) catch-up of column block k:  T_q -= X_prev L_prev[block k, q]^T
    if (has_prev && (!wg0 || isC)) {
#pragma unroll
        for (int sg = 0; sg < 4; ++sg)
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const double a = reinterpret_cast<const double*>(&opsC[(q * 4 + sg) * 64 + lane])[kk];
                    Tk[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Xp[sg][kk], Tk[q], 0, 0, 0);
                }
    }
    PS_STAMP(2);
    // (4) solve against the diagonal block (right-looking over the four 16-column blocks, see k_trsm_64h)
#pragma unroll
    for (int pp = 0; pp < 4; ++pp) {
        const v4d ai = opsT[(6 + pp) * 64 + lane];
        v4d x0 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) x0 = __builtin_amdgcn_mfma_f64_16x16x4f64(ai[kk], Tk[pp][kk], x0, 0, 0, 0);
        Tk[pp] = x0;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
            for (int q = pp + 1; q < 4; ++q) {
                const double a = reinterpret_cast<const double*>(&opsT[((q == 1 ? 0 : (q == 2 ? 1 : 3)) + pp) * 64 + lane])[kk];
                Tk[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Tk[pp][kk], Tk[q], 0, 0, 0);
            }
    }
    if (rv) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) A[(size_t)(ck + 16 * q + 4 * r + l4) * lda + row] = Tk[q][r];
    }
    PS_STAMP(3);
    if (!has_next) return;                                        // uniform: last step of the panel
    if (!wg0) {
        if (isP) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int r = 0; r < 4; ++r) Xs[(16 * w + l15) * PS_XLD + 16 * q + 4 * r + l4] = Tk[q][r];
        }
        if (wg1 && !has_prev) __syncthreads();                    // (with has_prev the barriers of (5) publish Xs)
        // (5) catch-up of column block k + 1
        if (has_prev) {
            __syncthreads();                                      // every wave is done with the operands of block k
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int e = tid + 512 * j, q = e >> 10, sx = (e >> 6) & 15, l = e & 63;
                smem[((q * 4 + (sx >> 2)) * 64 + l) * 4 + (sx & 3)] = oc[j];
            }
            __syncthreads();
#pragma unroll
            for (int sg = 0; sg < 4; ++sg)
#pragma unroll
                for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const double a = reinterpret_cast<const double*>(&opsC[(q * 4 + sg) * 64 + lane])[kk];
                        Un[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Xp[sg][kk], Un[q], 0, 0, 0);
                    }
        }
        // (first step of a panel: only the rows of L^-T that enter with it -- their zeros are what the next step's solve loads)
        if (rv && (has_prev || row >= un_fresh)) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int r = 0; r < 4; ++r) A[(size_t)(ck + 64 + 16 * q + 4 * r + l4) * lda + row] = Un[q][r];
        }
        if (isP) {
            // only now (U is stored, its registers are free): the diagonal block (k+2, k+2), its pending column block k - 1
            // and, eagerly, this step's column block: V -= X[k+2, k-1] X[k+2, k-1]^T + X[k+2, k] X[k+2, k]^T
            // (two 16-column blocks at a time: the kernel sits at the VGPR limit)
#pragma unroll 1
            for (int q0 = 0; q0 < 4; q0 += 2) {
                v4d Vn[2];
#pragma unroll
                for (int qq = 0; qq < 2; ++qq)
#pragma unroll
                    for (int r = 0; r < 4; ++r) Vn[qq][r] = A[(size_t)(ck + 128 + 16 * (q0 + qq) + 4 * r + l4) * lda + rowc];
                if (has_prev) {
#pragma unroll
                    for (int sg = 0; sg < 4; ++sg)
#pragma unroll
                        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                            for (int qq = 0; qq < 2; ++qq) {
                                const double a = -Xps[(16 * (q0 + qq) + l15) * PS_XLD + 16 * sg + 4 * kk + l4];
                                const double b = Xps[(16 * w + l15) * PS_XLD + 16 * sg + 4 * kk + l4];     // own row, from LDS
                                Vn[qq] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, Vn[qq], 0, 0, 0);
                            }
                }
#pragma unroll
                for (int sg = 0; sg < 4; ++sg)
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                        for (int qq = 0; qq < 2; ++qq) {
                            const double a = -Xs[(16 * (q0 + qq) + l15) * PS_XLD + 16 * sg + 4 * kk + l4];
                            const double b = Xs[(16 * w + l15) * PS_XLD + 16 * sg + 4 * kk + l4];          // (registers are scarce)
                            Vn[qq] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, Vn[qq], 0, 0, 0);
                        }
#pragma unroll
                for (int qq = 0; qq < 2; ++qq)
#pragma unroll
                    for (int r = 0; r < 4; ++r) A[(size_t)(ck + 128 + 16 * (q0 + qq) + 4 * r + l4) * lda + row] = Vn[qq][r];
            }
        }
        return;
    }
    // (6) workgroup 0: U = (k+1, k+1) arrives with every column block < k applied (the update role up to k - 2, block k - 1 by
    // the P waves of the previous launch, which also applied... nothing of this step: that is the one pass left):
    // D = U - X[k+1, k] X[k+1, k]^T, block row k + 1 as both operands, exchanged through Xs.
    if (isC) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) Xs[(16 * w + l15) * PS_XLD + 16 * q + 4 * r + l4] = Tk[q][r];
    }
    PS_STAMP(4);
    __syncthreads();                                              // X[k+1, k] is in Xs
    PS_STAMP(5);
    if (isC) {
#pragma unroll
        for (int sg = 0; sg < 4; ++sg)
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const double a = -Xs[(16 * q + l15) * PS_XLD + 16 * sg + 4 * kk + l4];
                    Un[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Tk[sg][kk], Un[q], 0, 0, 0);
                }
    }
    Potf2Lds& P = *reinterpret_cast<Potf2Lds*>(smem);            // aliases the operand area: dead after the next barrier
    __syncthreads();
    if (isC) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int rr = 16 * w + l15, cc = 16 * q + 4 * r + l4;
                P.S[cc * PB_LD + rr] = (cc <= rr) ? Un[q][r] : 0.0;
            }
    }
    __syncthreads();
    PS_STAMP(6);
    potf2b_core_mfma(P, info + (size_t)by * istride, ck + 64);
    PS_STAMP(7);
    potf2b_store(A + (size_t)(ck + 64) * lda + (ck + 64), lda, 64, P, tid, 512);
    PS_STAMP(8);
#undef PS_STAMP
}

// ---------------------------------------------------------------------------------------------
// LEFT-LOOKING steps of a 256-column node of the throughput schedule (two 128-column leaves, column blocks 0 .. 3 at c0 + 64 i).
// The K = 128 update between the two leaves (6 passes over the rows' column blocks: read blocks 0 and 1, read and write blocks
// 2 and 3) is folded into the catch-up of the right leaf's two launches, the way MODE 0 / 2 of k_panel_step fold a K = 64 one:
//   launch            catch-up (solve role)        critical workgroup (block row k + 1)          passes
//   k_panel_step<1>   -                            D11, as before                                2
//   <1, true>         block 1 with block 0         D22 = C22 - X20 X20^T - X21 X21^T, factored   3
//   <2, true>         block 2 with blocks 0, 1     D33 = C33 - X30 X30^T - X31 X31^T - X32 X32^T 4
//   <3, false>        block 3 with blocks 0, 1, 2  -                                             5
// 14 passes and 4 launches per node instead of 16 and 5.  Every C entry receives the products it received before, in ascending k
// through the same MFMA k-groups (the update kernels start from -C and store -acc, or negate the j side: exact either way), so
// the factor is bit-identical; only the store and reload between the K = 128 update and the K = 64 catch-up are gone.
// NP = previous column blocks [ck - 64 NP, ck) applied to block k = [ck, ck + 64) before its solve, one after the other: one
// 64-column block of operands in LDS and one of the rows' X in registers at a time, so that with the rows' own block at most
// TWO 64-column row blocks are live per thread.  FACT: workgroup 0 (block row k + 1, waves 0..3) also brings its diagonal block
// up to date with the NP blocks and with block k and factors it (potf2b_core_mfma); its X blocks reach the MFMA's other side
// through LDS (Xs, aliasing the operands), and its diagonal block is loaded only when the first X block has gone there.
// No workgroup waits for another: every operand is final since the previous launch.
// Every launch runs at 4 waves/SIMD (two workgroups per CU) and STREAMS: the prologue issues every load it needs before it waits
// for the first of them ((1) below), and while a workgroup's matrix pipes work on previous block p, the rows' X of block p + 1 is
// already on its way into the registers block p has finished with ((2) below), so a workgroup no longer depends on its
// co-resident one being out of phase.  Measured on one MI355X (one headline step, 128 chains, profiles/leafpipe_*): <1, true>
// 2.76 -> 2.44 ms, <2, true> 3.93 -> 3.23 ms, <3, false> 4.32 -> 3.90 ms (at 6 waves/SIMD the rotation does not fit 80
// registers: 80 spilled); k_panel_step<1, 4> is as it was.
// Rows of L^-T (gradient evaluations, the A phase of the structured value path): rows t_fresh0 <= row < t_fresh1 (absolute) have
// entered since the node began; nobody has written their block k, which starts from zero and is not loaded.  What the
// catch-up reads of such rows left of their own block is either written by an earlier launch of the node or inside the seeded band
// (k_xtri_seed: three blocks left of the row's own; <3, false> reaches exactly that far).
// ---------------------------------------------------------------------------------------------
template <int NP, bool FACT>
__global__ __launch_bounds__(512, 4) void k_leaf_step(double* __restrict__ Ab, int lda, int ck, int m_act, long long bstride,
                                                       int* __restrict__ info, int istride, int T, int nbatch, int t_fresh0,
                                                       int t_fresh1) {
    constexpr int kOpsC = 2560;                                         // doubles; after opsT
    constexpr int kSmem = kOpsC + (FACT ? 64 * PS_XLD : 4096);
    static_assert(64 * PS_XLD >= 4096, "Xs aliases (and covers) the catch-up operands");
    static_assert(!FACT || sizeof(Potf2Lds) <= kSmem * sizeof(double), "the factorisation's LDS aliases the step's");
    static_assert(64 * NP <= 64 * NMGP_XTRI_SEED_BLOCKS, "the catch-up of a row of L^-T would read left of the seeded band");
    __shared__ __attribute__((aligned(32))) double smem[kSmem];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    // role-major workgroup ids, as in k_panel_step: workgroup 0 of every matrix first
    const int bx = (int)blockIdx.x / nbatch, by = (int)blockIdx.x - bx * nbatch;
    double* A = Ab + (size_t)by * bstride;
    v4d* opsT = reinterpret_cast<v4d*>(smem);                    // [10][64 lanes], as in k_trsm_64h
    v4d* opsC = reinterpret_cast<v4d*>(smem + kOpsC);            // [4 q][4 sg][64 lanes]: -L[ck + 16 q + i][4 (4 sg + kk) + l4]
    double* Xs = smem + kOpsC;                                   // [64][PS_XLD]: workgroup 0's X[k+1, .] (FACT)
    const bool wg0 = bx == 0;                                    // block row k + 1, waves 0..3; waves 4..7 only keep the barriers
    const bool isC = wg0 && w < 4;
    const int row = wg0 ? ck + 64 + 16 * w + l15 : ck + 128 + 128 * (bx - 1) + 16 * w + l15;
    const bool rv = row < m_act && !(wg0 && w >= 4);
    const int rowc = row < m_act ? row : (m_act - 1);            // clamped: loads stay in bounds, results are masked
    const bool tload = rv && !(row >= t_fresh0 && row < t_fresh1);
    // addresses = a uniform column pointer + ONE lane offset per access pattern (32 bits): no 64-bit address registers per load
    const int wu = __builtin_amdgcn_readfirstlane(w);
    const unsigned vrow = (unsigned)(l4 * lda + rowc), vops = (unsigned)(l4 * lda + l15);
    auto colp = [&](int col) { return A + (size_t)col * lda; };
    double oc[8], ot[5];
    v4d Xp[4], Tk[4];
    auto load_ops = [&](int p) {                                 // L[block k, previous block p] (store_ops negates)
        const int cb = ck - 64 * (NP - p);
#pragma unroll
        for (int j = 0; j < 8; ++j) oc[j] = (colp(cb + 4 * (wu + 8 * (j & 1))) + ck + 16 * (j >> 1))[vops];
    };
    auto store_ops = [&]() {                                     // element j: q = j >> 1, sx = w + 8 (j & 1), lane
        __builtin_amdgcn_sched_barrier(0);                       // (the negation, hoisted to the loads, would wait for them there)
#pragma unroll
        for (int j = 0; j < 8; ++j) smem[kOpsC + (((j >> 1) * 4 + (j & 1) * 2 + (wu >> 2)) * 64 + lane) * 4 + (wu & 3)] = -oc[j];
    };
    // the rows' 16-column group `g` of the 64-column block at column cb, as BUFFER loads (one descriptor per block, the column as
    // scalar offset): a masked lane gives an offset beyond the descriptor's range, for which the hardware fetches nothing and
    // returns zero, so the loads need no branch around them.  Only without one does hipcc count the loads in flight exactly
    // (s_waitcnt vmcnt(N)): the two sides of a lane-masked branch merge to the smaller count, and the wait of an earlier load then
    // drains the row loads as well.
    auto row_block = [&](int cb) { return __builtin_amdgcn_make_buffer_rsrc(colp(cb), (short)0, 0x7fffffff, 0x00020000); };
    auto load_group = [&](v4d& dst, __amdgpu_buffer_rsrc_t blk, int g, unsigned voff) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            dst[r] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(blk, (int)voff, (16 * g + 4 * r) * lda * 8, 0));
    };
    const unsigned kMasked = 0x80000000u;                        // (in range: offset + 8 <= 0x7fffffff)
    const unsigned vxoff = rv ? vrow * 8u : kMasked, vtoff = tload ? vrow * 8u : kMasked;
    // (1) every load of the prologue is issued before the first of them is waited for: the operands of the first catch-up and of
    // the solve (L2 hits) first, then the rows' own block and their X in the first previous block (HBM).  The operands' way to LDS
    // waits for the operands only, and the rows travel across the barrier.  (Which entry of the diagonal block a lane fetches
    // is a select on the address, and what it makes of it a select on the value: a branch per entry costs a drained queue each.)
    load_ops(0);
    {
        const double* L = A + (size_t)ck * lda + ck;              // diagonal block k (factor + inverted 16x16 blocks)
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const int idx = tid + 512 * j;                        // 0 .. 2559
            const int blk = idx >> 8, kk = (idx >> 6) & 3, l = idx & 63;
            const int rr = l & 15, kc = 4 * kk + (l >> 4);
            if (j < 3) {                                          // blk < 6
                const int q = blk == 0 ? 1 : (blk < 3 ? 2 : 3);
                const int pp = blk == 0 ? 0 : (blk < 3 ? blk - 1 : blk - 3);
                ot[j] = L[(size_t)(16 * pp + kc) * lda + 16 * q + rr];
            } else {
                const int q = blk - 6;                   // inv(L_qq)[rr][kc] (kc < rr) sits at row 16 q + kc, column 16 q + rr
                ot[j] = L[(size_t)(16 * q + rr) * lda + 16 * q + (kc < rr ? kc : rr)];
            }
        }
    }
    {
        const __amdgpu_buffer_rsrc_t own = row_block(ck), x0 = row_block(ck - 64 * NP);
#pragma unroll
        for (int q = 0; q < 4; ++q) load_group(Tk[q], own, q, vtoff);
#pragma unroll
        for (int q = 0; q < 4; ++q) load_group(Xp[q], x0, q, vxoff);
    }
    store_ops();
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const int idx = tid + 512 * j;
        const int blk = idx >> 8, kk = (idx >> 6) & 3, l = idx & 63;
        const int rr = l & 15, kc = 4 * kk + (l >> 4);
        const double v = j < 3 ? -ot[j] : (kc < rr ? ot[j] : (kc == rr ? 1.0 / ot[j] : 0.0));
        smem[(blk * 64 + l) * 4 + kk] = v;
    }
    __syncthreads();
    // (2) catch-up, previous block by previous block in ascending k:  T_q -= X[rows, p] L[block k, p]^T
    // The X registers rotate by 16-column group.  After the 16 MFMAs of group sg of block p, Xp[sg] is dead, and the four loads
    // of block p + 1's group sg go into those same registers right there: they travel under the remaining MFMAs of block p and
    // across the barrier pair, and no third row block is ever live.  The operands of block p + 1 (L2 hits) are loaded AHEAD of
    // the row loads (oc[] is free since store_ops), so that their way to LDS waits for nothing that comes from HBM.
    // Workgroup 0's idle waves issue the (masked) loads too: a branch around them would make the counts inexact again.  hipcc
    // waits vmcnt(23) .. (16) in front of the operands' LDS stores and vmcnt(15) .. in front of the next block's MFMAs; with
    // lane-masked branches both were vmcnt(0) (measured: half the gain).
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const bool more = p + 1 < NP;
        if (more) load_ops(p + 1);
        const __amdgpu_buffer_rsrc_t xnext = row_block(ck - 64 * (NP - p - 1));
#pragma unroll
        for (int sg = 0; sg < 4; ++sg) {
            if (!wg0 || isC) {
#pragma unroll
                for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const double a = reinterpret_cast<const double*>(&opsC[(q * 4 + sg) * 64 + lane])[kk];
                        Tk[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Xp[sg][kk], Tk[q], 0, 0, 0);
                    }
            }
            if (more) load_group(Xp[sg], xnext, sg, vxoff);
        }
        if (more) {
            __syncthreads();                                      // every wave is done with the operands of block p
            store_ops();
            __syncthreads();
        }
    }
    // (3) solve against the diagonal block (right-looking over the four 16-column blocks, see k_trsm_64h)
#pragma unroll
    for (int pp = 0; pp < 4; ++pp) {
        const v4d ai = opsT[(6 + pp) * 64 + lane];
        v4d x0 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) x0 = __builtin_amdgcn_mfma_f64_16x16x4f64(ai[kk], Tk[pp][kk], x0, 0, 0, 0);
        Tk[pp] = x0;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
            for (int q = pp + 1; q < 4; ++q) {
                const double a = reinterpret_cast<const double*>(&opsT[((q == 1 ? 0 : (q == 2 ? 1 : 3)) + pp) * 64 + lane])[kk];
                Tk[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Tk[pp][kk], Tk[q], 0, 0, 0);
            }
    }
    if (rv) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) colp(ck + 16 * q + 4 * r)[vrow] = Tk[q][r];
    }
    if constexpr (FACT) {
        if (!wg0) return;
        // (4) workgroup 0: U = C[k+1, k+1] - sum_p X[k+1, p] X[k+1, p]^T (the previous blocks of its own rows come back from
        // memory into Xs, 64 x 64 at a time: both MFMA operands from LDS) - X[k+1, k] X[k+1, k]^T (the solve's result); factor it
        v4d Un[4];
        if (isC) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int r = 0; r < 4; ++r) Un[q][r] = colp(ck + 64 + 16 * q + 4 * r)[vrow];
        }
#pragma unroll 1
        for (int p = 0; p < NP; ++p) {
            const int cb = ck - 64 * (NP - p);
#pragma unroll
            for (int j = 0; j < 8; ++j) oc[j] = colp(cb + wu + 8 * j)[ck + 64 + lane];
            __syncthreads();                                      // every wave is done with what the area held
#pragma unroll
            for (int j = 0; j < 8; ++j) Xs[lane * PS_XLD + wu + 8 * j] = oc[j];
            __syncthreads();
            if (isC) {
#pragma unroll
                for (int sg = 0; sg < 4; ++sg)
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk) {
                        const double b = Xs[(16 * w + l15) * PS_XLD + 16 * sg + 4 * kk + l4];              // own row
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const double a = -Xs[(16 * q + l15) * PS_XLD + 16 * sg + 4 * kk + l4];
                            Un[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, Un[q], 0, 0, 0);
                        }
                    }
            }
        }
        __syncthreads();                                          // every wave is done with the previous block in Xs
        if (isC) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int r = 0; r < 4; ++r) Xs[(16 * w + l15) * PS_XLD + 16 * q + 4 * r + l4] = Tk[q][r];
        }
        __syncthreads();
        if (isC) {
#pragma unroll
            for (int sg = 0; sg < 4; ++sg)
#pragma unroll
                for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const double a = -Xs[(16 * q + l15) * PS_XLD + 16 * sg + 4 * kk + l4];
                        Un[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Tk[sg][kk], Un[q], 0, 0, 0);
                    }
        }
        Potf2Lds& P = *reinterpret_cast<Potf2Lds*>(smem);        // aliases the operand area: dead after the next barrier
        __syncthreads();
        if (isC) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int rr = 16 * w + l15, cc = 16 * q + 4 * r + l4;
                    P.S[cc * PB_LD + rr] = (cc <= rr) ? Un[q][r] : 0.0;
                }
        }
        __syncthreads();
        potf2b_core_mfma(P, info + (size_t)by * istride, ck + 64);
        potf2b_store(A + (size_t)(ck + 64) * lda + (ck + 64), lda, 64, P, tid, 512);
    }
}

// A[row, j] = v[j]  (the extra row carrying the right-hand side)
// vstride = 0 broadcasts one vector to every matrix of the batch (all chains of a subject share y)
// (cps: consecutive groups of cps matrices share one vector -- the chains of a subject in a multi-subject batch)
__global__ void k_set_row(double* __restrict__ A, int lda, int row, const double* __restrict__ v, int n,
                          long long bstride, long long vstride, int cps) {
    int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) A[(size_t)blockIdx.y * bstride + (size_t)j * lda + row] = v[(size_t)(blockIdx.y / cps) * vstride + j];
}
void set_row(hipStream_t s, double* A, int lda, int row, const double* v, int n, int batch, long long bstride,
             long long vstride, int cps) {
    NMGP_LAUNCH(k_set_row, dim3(cdiv_c(n, 256), batch), dim3(256), 0, s, A, lda, row, v, n, bstride, vstride, cps < 1 ? 1 : cps);
}
__global__ void k_get_row(const double* __restrict__ A, int lda, int row, double* __restrict__ v, int n,
                          long long bstride, long long vstride) {
    int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) v[(size_t)blockIdx.y * vstride + j] = A[(size_t)blockIdx.y * bstride + (size_t)j * lda + row];
}
void get_row(hipStream_t s, const double* A, int lda, int row, double* v, int n, int batch, long long bstride,
             long long vstride) {
    NMGP_LAUNCH(k_get_row, dim3(cdiv_c(n, 256), batch), dim3(256), 0, s, A, lda, row, v, n, bstride, vstride);
}

// Blocked Cholesky of the n x n lower triangle of A.  Below the matrix the same array may hold
//   * `extra` dense rows R (rows n .. n+extra-1): on exit R L^-T (a right-hand side y becomes z = L^-1 y), and
//   * `xtri` identity rows (rows n+extra .. n+extra+xtri-1, seeded by identity_rows()): on exit L^-T, from which
//     Sigma^-1 = (L^-T)(L^-T)^T follows with one more SYRK.  Row r of L^-T is zero left of column r, so only the
//     first `cend` of these rows take part while the factorisation is at column cend (n^3/3 extra flop, not n^3).
//     The caller seeds only a band of each row (k_xtri_seed).  Row r ENTERS with the panel [c0, c1) its index lies in: the
//     launch that applies that panel to the columns right of it is the first to touch X[r, c >= c1], so the update kernels
//     start the launch's last c1 - c0 rows ("fresh" rows: tri_row0 + tri_k0 onwards) from zero instead of loading them,
//     and every later launch finds them written.  Every update call of a gradient factorisation therefore passes
//     (tri_row0, tri_k0).
// batch > 1 factors `batch` matrices of identical shape at once (matrix b at A + b * bstride, status word at
// info + b * istride): every launch covers all of them, so the latency of the 64-wide steps is paid once per batch.
//
// One potrf_lower call: what is constant for it, and the one piece of state its launches hand to each other.
struct Factorisation {
    hipStream_t s, s2;           // panels and near updates on s; far updates of the look-ahead schedule on s2
    double* A;
    int lda, n, extra, xtri;
    int* info;
    int batch;
    long long bs;
    int is;
    bool precise;
    const SyrkHook* hook;
    long long* stamps;           // StepStamps' device buffer, or nullptr
    // the preceding update has already factored the next diagonal block (set by update(), taken by whichever panel routine
    // runs next: every update that may set it is followed by the panel part that starts with that block)
    bool block_done = false;

    double* at(int row, int col) const { return A + (size_t)col * lda + row; }
    // rows that take part when the factorisation has reached column `cend`: the n matrix rows, the `extra` dense rows
    // (right-hand sides) and the first `cend` of the `xtri` identity rows (row r of L^-T is zero left of column r)
    int active_rows(int cend) const { return n + extra + (cend < xtri ? cend : xtri); }
    bool take_block_done() {
        const bool done = block_done;
        block_done = false;
        return done;
    }

    // Trailing update: the factored columns [c0, c0 + k) applied to the columns [c1, c1 + ncols), all rows active at c0 + k.
    // fuse_width: columns left in the panel part that starts at c1 when that part is factored NEXT on the same stream (a full
    // 64-column block is what the fused form factors: the launch's tile (0, 0) holds that diagonal block); 0: nobody asks.
    void update(hipStream_t st, int c0, int k, int c1, int ncols, int fuse_width) {
        const bool fuse = fuse_width >= 64 && !precise;
        const bool done = syrk_lower(st, at(c1, c0), lda, at(c1, c1), lda, active_rows(c0 + k) - c1, ncols, k, batch, bs, -1, 0,
                                     xtri > 0 ? n + extra - c1 : kNoTriRows, c0, fuse ? info : nullptr, is, c1, hook);
        if (fuse) block_done = done;
    }

    // diagonal block (at most 64 columns) + solve of the rows below it
    void block_solve(int c0, int w) {
        if (!take_block_done()) potf2_64(s, at(c0, c0), lda, w, info, c0, batch, bs, is, precise);
        trsm_64(s, at(c0, c0), lda, w, at(c0 + w, c0), lda, active_rows(c0 + w) - (c0 + w), batch, bs, precise);
    }

    // columns [c0, c0 + w), w a multiple of 64, as fused steps: one k_panel_step launch per 64 columns
    void fused_steps(int c0, int w, bool leaf) {
        if (!take_block_done()) potf2_64(s, at(c0, c0), lda, 64, info, c0, batch, bs, is, precise);   // the first diagonal block
        const int nk = w / 64;
        for (int k = 0; k < nk; ++k) {
            const int ck = c0 + 64 * k;
            const int m_act = active_rows(ck + 64);
            const int rows = m_act - (ck + 64);
            if (rows <= 0) continue;                     // last block of the matrix and nothing below it
            const int has_prev = k > 0, has_next = k + 1 < nk;
            const int T = 1 + (rows > 64 ? cdiv_c(rows - 64, 128) : 0);     // workgroup 0: block row k + 1 alone
            SyrkPlan pl;
            const int u_m = m_act - (ck + 128), u_n = c0 + w - (ck + 128);
            if (has_prev && u_m > 0 && u_n > 0) pl = syrk_plan(lda, lda, u_m, u_n, 64, 1, 0, true);
            const int pre = (ck + 192 <= c0 + w) ? 1 : 0;            // block (k+2, k+2) lies inside the panel: see the P waves
            if (pre) pl.kflags |= 128;                                // ... which own it: the update role skips that block
            long long* st = stamps ? stamps + (size_t)(ck / 64) * 16 : nullptr;
            // rows of L^-T that nobody has written yet in the columns this step touches first (see above): row r of L^-T
            // (absolute row n + extra + r) enters with step r / 64 of its panel; its column block k + 1 is first touched by the
            // solve role of that step and of the next one, everything further right by the update role one step later
            const int un_fresh = xtri > 0 ? n + extra + (has_prev ? ck - 64 : ck) : kNoTriRows;
            const int u_tri = xtri > 0 ? n + extra - 64 * NMGP_XTRI_SEED_BLOCKS : kNoTriRows;
            if (leaf && pl.tiles == 0 && !pre && nk == 2) {
                if (k == 0)
                    NMGP_LAUNCH((k_panel_step<1, 4>), dim3((unsigned)(T * batch)), dim3(512), 0, s, A, lda, ck, 0, 1, m_act, c0 + w, bs, info,
                                is, T, 0, 0, 0, 0, batch, 0, un_fresh, u_tri, st);
                else
                    NMGP_LAUNCH((k_panel_step<2, 6>), dim3((unsigned)(T * batch)), dim3(512), 0, s, A, lda, ck, 1, 0, m_act, c0 + w, bs, info,
                                is, T, 0, 0, 0, 0, batch, 0, un_fresh, u_tri, st);
            } else {
                NMGP_LAUNCH((k_panel_step<0, 2>), dim3((unsigned)((T + pl.tiles) * batch)), dim3(512), 0, s, A, lda, ck, has_prev, has_next, m_act,
                            c0 + w, bs, info, is, T, pl.mrows, u_n, pl.kflags, pl.tiles, batch, pre, un_fresh, u_tri, st);
            }
        }
    }

    // columns [c0, c0 + 256) of the throughput schedule: two 128-column leaves with the K = 128 update between them folded into
    // the right leaf's catch-up (k_leaf_step has the table)
    void leaf256(int c0) {
        if (!take_block_done()) potf2_64(s, at(c0, c0), lda, 64, info, c0, batch, bs, is, precise);   // the first diagonal block
        // rows of L^-T that have entered since the node began: their column blocks 2 and 3 start from zero (the removed update's
        // "fresh" rows and, for block 3, those that enter with block 2)
        const int f0 = xtri > 0 ? n + extra + c0 : kNoTriRows;
        for (int k = 0; k < 4; ++k) {
            const int ck = c0 + 64 * k;
            const int m_act = active_rows(ck + 64);
            const int rows = m_act - (ck + 64);
            if (rows <= 0) continue;                     // last block of the matrix and nothing below it
            const int T = 1 + (rows > 64 ? cdiv_c(rows - 64, 128) : 0);     // workgroup 0: block row k + 1 alone
            const dim3 grid((unsigned)(T * batch));
            if (k == 0)
                NMGP_LAUNCH((k_panel_step<1, 4>), grid, dim3(512), 0, s, A, lda, ck, 0, 1, m_act, c0 + 128, bs, info, is, T, 0, 0, 0, 0, batch,
                            0, f0, xtri > 0 ? n + extra - 64 * NMGP_XTRI_SEED_BLOCKS : kNoTriRows,
                            stamps ? stamps + (size_t)(ck / 64) * 16 : nullptr);
            else if (k == 1)
                NMGP_LAUNCH((k_leaf_step<1, true>), grid, dim3(512), 0, s, A, lda, ck, m_act, bs, info, is, T, batch, kNoTriRows,
                            kNoTriRows);
            else if (k == 2)
                NMGP_LAUNCH((k_leaf_step<2, true>), grid, dim3(512), 0, s, A, lda, ck, m_act, bs, info, is, T, batch, f0,
                            xtri > 0 ? f0 + 128 : kNoTriRows);
            else
                NMGP_LAUNCH((k_leaf_step<3, false>), grid, dim3(512), 0, s, A, lda, ck, m_act, bs, info, is, T, batch, f0,
                            xtri > 0 ? f0 + 192 : kNoTriRows);
        }
    }

    // right-looking 64-wide steps (each step updates the rest of the panel with K = 64)
    void panel_rl(int c0, int w) {
        for (int j0 = c0; j0 < c0 + w; j0 += 64) {
            const int jb = (c0 + w - j0 < 64) ? (c0 + w - j0) : 64;
            block_solve(j0, jb);
            update(s, j0, jb, j0 + jb, c0 + w - (j0 + jb), c0 + w - (j0 + jb));
        }
    }

    // Recursive halving (left part, ONE update of the right part with K = left width, right part) down to pieces of at most
    // `base` columns.  The leaf rule:
    enum Leaf {
        kBlockSolve,     // base = 64: diagonal block + solve
        kFusedSteps,     // pieces of `base` columns run as fused steps
        kLeaf128         // the throughput schedule, base = 128: a 256-column node runs left-looking (leaf256: four launches, no
    };                   // update between its leaves), any other 128-column piece takes the two leaf launches (k_panel_step<1>,
                         // <2>), a 64-column remainder the plain diagonal block + solve
    void panel_halving(int c0, int w, int base, Leaf leaf) {
        if (w <= base) {
            if (leaf == kBlockSolve || (leaf == kLeaf128 && w != 128)) block_solve(c0, w);
            else fused_steps(c0, w, leaf == kLeaf128);
            return;
        }
        if (leaf == kLeaf128 && w == 256) {                      // left 128, right 128: no update launch between them
            leaf256(c0);
            return;
        }
        int h = ((w / 2 + 63) / 64) * 64;                       // left width: a multiple of 64, at least half
        if (h >= w) h = ((w - 1) / 64) * 64;
        panel_halving(c0, h, base, leaf);
        update(s, c0, h, c0 + h, w - h, w - h);                 // tile (0, 0) holds the diagonal block the right part starts with
        panel_halving(c0 + h, w - h, base, leaf);
    }

    // Factor the panel of columns [c0, c0 + w) (already up to date) together with all active rows below it.  The schedules:
    //  * right-looking 64-wide steps: shortest critical path of the three-launch forms, for a single matrix, where every
    //    launch is latency-bound anyway;
    //  * recursive halving: touches the panel's C entries log2(w/64) times instead of w/128 times and runs only a quarter of
    //    the update flop at K = 64 (HBM-bound at 8 flop/byte), the rest at K = 128 / 256: for batches, where the launches are
    //    throughput-bound;
    //  * fused steps (k_panel_step: ONE launch per 64 columns) under a recursive split.  A fused step re-reads and re-writes ALL
    //    remaining columns of its panel (the delayed K = 64 update): 1792 column-block passes per 512-wide panel against 768
    //    for recursive halving.  For one matrix that is free -- a step's ~190 workgroups fit the 256 CUs in one round and the
    //    step is latency-bound (~25 us) -- but with 8 subjects a step of the first panel is 720 workgroups at one per CU (118 KB
    //    of LDS) = three rounds, 72 us, bound by that traffic.  So the panel is halved recursively (one K = w/2 update per level,
    //    ordinary update kernel with the next diagonal block fused) until the pieces are `base` wide, and only those run as
    //    fused steps: base = 128 keeps recursive halving's 768 passes with 11 launches per 512 columns instead of 23.
    //  * the throughput schedule (kLeaf128) halves down to 256-column nodes.  A node as leaf, K = 128 update, leaf cost 2 + 3 + 6 +
    //    2 + 3 = 16 passes (one pass = one read or write of a 64-column block of all active rows) in 5 launches; leaf256 runs it
    //    left-looking in 2 + 3 + 4 + 5 = 14 passes and 4 launches (k_leaf_step): the K = 128 launch, HBM-bound at one tile column,
    //    is gone.  Nodes of width 192 (left 128, right 64) keep the K = 128 update and the plain block solve.
    void panel(int c0, int w) {
        const Switches& sw = switches();
        // the matrix-core panel kernels: whole 64-column blocks, 16-byte loads, diagonal blocks with inverted 16x16 blocks
        const bool mfma_ok = w > 0 && (w % 64 == 0) && (lda % 2 == 0) && !precise;
        // latency regime, auto: batch * n <= 73728 (measured: n = 6144: 8 chains 523 vs 503 evals/s, 16 chains 418 vs 616;
        // n = 3072: 16 subjects 3211 vs 2729, 24 subjects 3563, 32 subjects 2877 vs 3714)
        const bool small = sw.fused_max_batch >= 0 ? batch <= sw.fused_max_batch : (long long)batch * n <= 73728;
        const int rec_min_batch = 4;                 // smallest batch that takes the recursive panels
        if (mfma_ok && (sw.panel == Switches::kFused || (sw.panel == Switches::kAuto && small)))
            panel_halving(c0, w, fused_base(w), kFusedSteps);
        else if (mfma_ok && sw.panel == Switches::kAuto && batch >= rec_min_batch && w >= 128)
            panel_halving(c0, w, 128, kLeaf128);
        else if (sw.panel == Switches::kRl || (sw.panel != Switches::kRec && batch < rec_min_batch))
            panel_rl(c0, w);
        else
            panel_halving(c0, w, 64, kBlockSolve);
    }
    int fused_base(int w) const {
        if (switches().fused_base >= 64) return switches().fused_base;
        // measured (MI355X, profiles/r03_fused_base.txt; evals/s at base 512 / 256 / 128): one chain 301 / 286 / 271; 4 chains 537 / 526 /
        // 504; 8 chains 609 / 606 / 587; 8 subjects x N=1024 2935 / 2925 / 2779, value+gradient 1275 / 1338 / 1301; 16 subjects 3603 /
        // 3828 / 3745; separable N=4096 D=5 3.92 / 4.01 / 4.12 ms, value+gradient 9.32 / 9.23 / 9.54 ms.  The K = 256 update a split
        // inserts costs what the steps save until a step is well over two rounds of workgroups: 256 from 16 matrices on, and for
        // gradient evaluations (twice the rows) from 5 matrices on.
        if (w > 256 && (batch >= 16 || (xtri > 0 && batch >= 5))) return 256;
        return w;
    }

    // All panels of nb1 columns.  Look-ahead over two streams: after panel k is factored on `s`, only the NEXT panel's columns
    // are updated on `s` (so that panel k+1 can start at once) while the rest of the trailing matrix is updated on `s2`,
    // concurrently with the latency-bound 64-wide steps of panel k+1.  ev[] must hold at least 2 * ceil(n / nb1) + 1 events;
    // s2 == nullptr (or ev == nullptr) selects the plain single-stream order.
    void run(int nb1, hipEvent_t* ev) {
        // look-ahead pays where the panel steps are latency-bound: one matrix or a handful of subjects (the batched throughput
        // path keeps every kernel exclusive); NMGP_CHOL_LA_MAX_BATCH moves the limit
        const bool la = (s2 != nullptr && ev != nullptr && n > 2 * nb1 && batch <= switches().la_max_batch && !precise);
        if (!la) {
            for (int c0 = 0; c0 < n; c0 += nb1) {
                const int w1 = (n - c0 < nb1) ? (n - c0) : nb1;
                const int c1 = c0 + w1;
                panel(c0, w1);
                update(s, c0, w1, c1, n - c1, n - c1 < nb1 ? n - c1 : nb1);
            }
            return;
        }
        // everything queued on s so far (covariance build, right-hand side row) must be visible to s2
        hipEventRecord(ev[0], s);
        hipStreamWaitEvent(s2, ev[0], 0);
        int k = 0;
        bool prevB = false;
        for (int c0 = 0; c0 < n; c0 += nb1, ++k) {
            const int w1 = (n - c0 < nb1) ? (n - c0) : nb1;
            const int c1 = c0 + w1;
            const int w1n = (c1 < n) ? ((n - c1 < nb1) ? (n - c1) : nb1) : 0;
            const int c2 = c1 + w1n;
            hipEvent_t evPanel = ev[1 + 2 * k], evB = ev[2 + 2 * k];
            panel(c0, w1);
            if (c1 >= n) break;
            // the previous far update also wrote the next panel's columns
            if (prevB) hipStreamWaitEvent(s, ev[2 + 2 * (k - 1)], 0);
            update(s, c0, w1, c1, w1n, w1n);                    // near: the next panel's columns, its first block fused
            // the far update starts only when the NEAR one is through: started together they share the chip and the near
            // update -- which the next panel waits for -- takes 2-4x as long (96-227 us instead of ~45 in the kernel trace)
            hipEventRecord(evPanel, s);
            prevB = false;
            if (c2 < n) {
                hipStreamWaitEvent(s2, evPanel, 0);
                update(s2, c0, w1, c2, n - c2, 0);              // far: everything right of the next panel
                hipEventRecord(evB, s2);
                prevB = true;
            }
        }
        // the caller continues on s: it must see the last far update
        if (prevB) hipStreamWaitEvent(s, ev[2 + 2 * (k - 1)], 0);
    }
};

void potrf_lower(hipStream_t s, hipStream_t s2, hipEvent_t* ev, double* A, int lda, int n, int extra, int xtri,
                 int nb1, int* info, int batch, long long bstride, int istride, const SyrkHook* hook, int precise) {
    // auto panel width (512 / 1024 / 2048; 64 chains of n = 6144: 673 / 716 / 728 evals/s): a wider panel halves the passes over the trailing matrix (each tile's C load / store and launch tail) and
    // pays with one more K = 512 level inside the panel; +1.5 % for 32 chains of n = 6144, +2 % for 64 subjects of
    // n = 3072, slower for one chain or 8 subjects; with the L^-T rows (gradient) 2048 wins since their zero k-panels are skipped
    // (234.6 against 233.6 evals/s at 64 chains)
    if (nb1 <= 0)
        nb1 = (batch >= 16 && n >= 4096) ? 2048         // (n = 4096: 80 blocks of the batched separable model 418.9 -> 430.6 evals/s)
              : (((batch >= 4 && n >= 4096) || (batch >= 32 && n >= 2048)) && (long long)batch * n > 73728) ? 1024 : 512;
    // (batches small enough for the fused panel steps keep 512: separable N = 4096, D = 5: 4.39 ms against 4.55 with 1024)
    const int nsteps = (n + 63) / 64;
    Factorisation f{s, s2, A, lda, n, extra, xtri, info, batch, bstride, istride, precise != 0, hook, g_step_stamps.begin(s, nsteps)};
    f.run(nb1, ev);
    g_step_stamps.dump(s, nsteps);
}

// Seed of the rows that turn into X = L^-T during a gradient evaluation (rows row0 + pad .. row0 + pad + n - 1 of the
// factorisation buffer, n columns) -- what used to be a full "identity rows" write of n^2 doubles per matrix (38.7 GB per
// 128-chain step, 12 ms).  Only what somebody READS BEFORE WRITING is initialised:
//   * the `pad` rows (dense rows that take part from the first column on): zero;
//   * row r of X, columns [64 (r/64 - 3), 64 (r/64 + 1)): the identity.  Its diagonal 64 x 64 block is what the panel solve
//     turns into L^-T; the three blocks left of it are structural zeros that the update kernels read as operands because their
//     k-loops skip leading zero k-panels per TILE, not per row (reach <= 158 columns left of the diagonal), the inverse SYRK
//     (k-loop from the tile's first row: reach 127) and the triangular matrix-vector product (256-wide blocks: reach 255).
// Everything right of the diagonal block is written by the factorisation before it is read: a row enters the factorisation
// with the panel its index lies in, and the update kernels start such "fresh" rows from zero instead of loading them
// (syrk_tile_fast & co.: fresh0; k_panel_step: un_fresh, u_tri).  Everything further left is never touched.
// reach of the readers left of a row's own 64-column block: update tiles skip leading zero k-panels per 128-row TILE in pairs of
// 16-column panels (SY_BM + 2 SY_BK - 2 columns left of the diagonal at most), the inverse SYRK starts at the tile's first row
// (SY_BM - 1), k_panel_step's u_tri = n + extra - 192 assumes exactly three seeded blocks, k_leaf_step<3>'s catch-up of a row that
// enters with a node's last block reads the node's first block: three blocks left of the row's own (asserted in the kernel)
static_assert(SY_BM + 2 * SY_BK - 2 <= 64 * NMGP_XTRI_SEED_BLOCKS, "update tiles of L^-T rows would read left of the seeded band");
static_assert(NMGP_XTRI_SEED_BLOCKS == 3, "k_panel_step (u_tri) and k_xtri_seed's grid (4 column blocks per row block) assume three seeded blocks");
__global__ __launch_bounds__(256) void k_xtri_seed(double* __restrict__ A, int lda, int row0, int n, int pad,
                                                    long long bstride) {
    A += (size_t)blockIdx.z * bstride;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (blockIdx.x == gridDim.x - 1) {                      // the pad rows
        for (int c = blockIdx.y * 256 + threadIdx.x; c < n; c += 256 * gridDim.y)
            for (int q = 0; q < pad; ++q) A[(size_t)c * lda + row0 + q] = 0.0;
        return;
    }
    const int b = blockIdx.x;                                // 64-row block of X; blockIdx.y = which of the four 64-column blocks
    const int r = 64 * b + lane;
    const int cb = b - NMGP_XTRI_SEED_BLOCKS + (int)blockIdx.y;
    if (cb < 0 || r >= n) return;
#pragma unroll 4
    for (int k = 0; k < 16; ++k) {
        const int c = 64 * cb + w + 4 * k;
        if (c < n) A[(size_t)c * lda + row0 + pad + r] = (r == c) ? 1.0 : 0.0;
    }
}
void identity_rows(hipStream_t s, double* A, int lda, int row0, int n, int pad, int batch, long long bstride) {
    NMGP_LAUNCH(k_xtri_seed, dim3(cdiv_c(n, 64) + 1, NMGP_XTRI_SEED_BLOCKS + 1, batch), dim3(256), 0, s, A, lda, row0, n, pad, bstride);
}

}  // namespace nmgpk
