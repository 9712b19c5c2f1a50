// The cohort of ragged Hadamard subjects (nmgp_had_set_subjects, nmgp_hadamard_cohort.hip) under the three models: the entries
// nmgp_had_subjects_eval (nonseparable), nmgp_hads_subjects_eval (separable) and nmgp_hadst_subjects_eval (stationary), ONE argument
// check and chunk loop (cohm_subjects_eval<Model>, had_for_chunks), ONE launch sequence of a chunk (cohm_eval_chunk<Model>) and one
// struct of hooks per model (CohNon, CohSep, CohSta), as the resident entries have in nmgp_hadamard_common.h.  The two skeletons stay
// two functions: they differ in where N comes from, the stride of the riding y row, the trace, the finiteness range and the lifetime
// of the prior factors.
//
// The set and its padding argument are nmgp_hadamard_cohort.hip's: every subject is padded to Nmax with decoupled unit observations,
// the padded part of every factor is the identity, and log det, z, alpha, the Mahalanobis terms and the prior log-determinants gain
// exact zeros.  What does NOT take care of itself, per model:
//   nonseparable tr S^-1 (one per padded observation), the N log 2 pi of the 1 + T GP-prior terms and their centred right-hand sides
//                (k_hadc_* of nmgp_hadamard_cohort.hip, which the predictor there shares)
//   separable    tr S^-1 (one per padded observation), the N log 2 pi of the TWO GP-prior terms, the two centred prior right-hand
//                sides, and the label-segmented reduction of d / d L_vec: the set's labels are zero-padded, so an unmasked walk would
//                add the padded rows to the slots of label 0 (their partial rows are written as zeros here as well)
//   stationary   tr S^-1, and the adjoint sums: a padded i has G_ii = -1/2 (the -1 on the padded diagonal of -S^-1), which would reach
//                a_s (d / d tilde_sigma) and, through the zero-padded labels, the label-0 slots of L; there is no prior stream
// k_gibbs_*, k_hads_* and k_hadst_* are shared by entries whose bits are pinned, so no mask is threaded through them.  The masked
// Gibbs pair of the first two models is k_hadc_cov<M, AMP> / k_hadc_adjoint<M, AMP> (nmgp_hadamard_common.h); the kernels below are
// the separable and stationary models' own, siblings with the originals' 64 x 64 tile, lane mapping, LDS staging (hadst_stage),
// expression order and fixed summation order, blockIdx.z = chain, subject = chain / cps of the chunk; a subject with N_s = Nmax gets
// the resident path's bits.  Every mask comes from the device table of the subjects' sizes (nobs), never from a padded slot.
//
// Separable padded layout: [tilde_l (Nmax) | tilde_sigma (Nmax) | L_vec (T) | tilde_sigma2_err], Pmax = 2 Nmax + T + 1; subject s fills
// the first nobs[s] slots of the two curve blocks.  The stationary vector has no per-observation part: [B, T + 3] as it is.
#include "nmgp_hadamard_common.h"

#include <algorithm>

using namespace nmgpk;

namespace {

inline unsigned cdiv(long long a, long long b) { return (unsigned)((a + b - 1) / b); }

// ---- separable ------------------------------------------------------------------------------------------------------------------------

// Real i: ell = exp(tilde_l), sig = exp(tilde_sigma), Rv[i, 0..M) = row c_i of the chain's L, zero-padded (k_hads_prep).  Padded i:
// ell = sig = 1, Rv = 0 -- written, so that no later kernel reads what nobody wrote, and without reading the padded parameter slots.
__global__ void k_hadcs_prep(const double* __restrict__ pars, const int* __restrict__ indx, const int* __restrict__ nobs, int cps,
                             int N, int M, int T, double* __restrict__ ell, double* __restrict__ sig, double* __restrict__ Rv) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int sub = blockIdx.y / cps;                             // blockIdx.y = chain
    const int Ns = nobs[sub];
    pars += (size_t)blockIdx.y * ((size_t)2 * N + T + 1);
    indx += (size_t)sub * N;
    ell += (size_t)blockIdx.y * N;
    sig += (size_t)blockIdx.y * N;
    Rv += (size_t)blockIdx.y * N * M;
    if (i >= Ns) {
        ell[i] = 1.0;
        sig[i] = 1.0;
        for (int m = 0; m < M; ++m) Rv[(size_t)i * M + m] = 0.0;
        return;
    }
    ell[i] = exp(pars[i]);
    sig[i] = exp(pars[N + i]);
    const int c = indx[i];
    const double* u = pars + (size_t)2 * N + c * (c + 1) / 2;
    for (int m = 0; m < M; ++m) Rv[(size_t)i * M + m] = (m <= c) ? u[m] : 0.0;
}

// two-column prior right-hand side (k_two_col_rhs_b): tilde_l - mu_l and tilde_sigma - mu_s on the real slots, zeros on the padded
// ones, whose parameter slots are not read
__global__ void k_hadcs_prior_rhs(const double* __restrict__ pars, const int* __restrict__ nobs, int cps, int N, int T, double mu_l,
                                  double mu_s, double* __restrict__ R) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (i >= N) return;
    const int Ns = nobs[b / cps];
    pars += (size_t)b * ((size_t)2 * N + T + 1);
    const bool real = i < Ns;
    R[((size_t)2 * b) * N + i] = real ? pars[i] - mu_l : 0.0;
    R[((size_t)2 * b + 1) * N + i] = real ? pars[N + i] - mu_s : 0.0;
}

// k_hads_finalize with the subject's own N_s in the N log 2 pi of both GP-prior terms and the per-subject half log-determinants
// (Nmax is the stride of the padded parameter layout only)
__global__ void k_hadcs_finalize(const double* __restrict__ scal, const double* __restrict__ q, const double* __restrict__ hl_l,
                                 const double* __restrict__ hl_s, const double* __restrict__ pars, const int* __restrict__ nobs,
                                 int cps, int Nmax, int T, double a, double b, double var, double log_sd, int prior,
                                 double* __restrict__ out6) {
    if (threadIdx.x != 0) return;
    const size_t P = (size_t)2 * Nmax + T + 1;
    const int sub = blockIdx.x / cps;
    const int N = nobs[sub];
    hl_l += sub;
    hl_s += sub;
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
        const double v = pars[(size_t)2 * Nmax + t];
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

// k_hads_grad_obs on the padded layout: per REAL observation the J partials summed in order, d NegLog / d tilde_l and / d tilde_sigma
// with the prior gradients (R2: [Nmax, 2] column-major per chain), the summed row components into rsum for the label reduction; +0.0
// in the padded curve slots (R2 is not applied there) and zero rsum rows; the sigma2 slot from the trace over the real observations.
__global__ __launch_bounds__(256) void k_hadcs_grad_obs(const double* __restrict__ part, long long pstride, int NJ, int N, int M,
                                                         int T, const int* __restrict__ nobs, int cps, const double* __restrict__ R2,
                                                         const double* __restrict__ pars, const double* __restrict__ tr, double a,
                                                         double b, int prior, double* __restrict__ rsum, double* __restrict__ grad) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const size_t P = (size_t)2 * N + T + 1;
    const int Ns = nobs[blockIdx.y / cps];
    {   // blockIdx.y = chain
        const size_t z = blockIdx.y;
        part += z * (size_t)pstride;
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
    if (i >= Ns) {
        grad[i] = 0.0;
        grad[(size_t)N + i] = 0.0;
        for (int m = 0; m < M; ++m) rsum[(size_t)i * M + m] = 0.0;
        return;
    }
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

// k_hads_grad_lvec over i < N_s only: the set's labels are zero-padded, so an unmasked walk would add the padded rows to label 0
__global__ __launch_bounds__(256) void k_hadcs_grad_lvec(const double* __restrict__ rsum, const int* __restrict__ indx,
                                                          const int* __restrict__ nobs, int cps, int N, int M, int T,
                                                          const double* __restrict__ pars, double var, int prior,
                                                          double* __restrict__ grad) {
    __shared__ double sh[256];
    const int t = blockIdx.x;
    const size_t P = (size_t)2 * N + T + 1;
    const int sub = blockIdx.y / cps;
    const int Ns = nobs[sub];
    indx += (size_t)sub * N;
    rsum += (size_t)blockIdx.y * N * M;
    pars += (size_t)blockIdx.y * P;
    grad += (size_t)blockIdx.y * P;
    int c = 0;
    while ((c + 1) * (c + 2) / 2 <= t) ++c;
    const int m = t - c * (c + 1) / 2;
    double acc = 0.0;
    for (int i = threadIdx.x; i < Ns; i += 256)
        if (indx[i] == c) acc += rsum[(size_t)i * M + m];
    acc = block_sum_256(acc, sh);
    if (threadIdx.x == 0) {
        if (prior) acc -= pars[(size_t)2 * N + t] / var;
        grad[(size_t)2 * N + t] = -acc;
    }
}

// ---- stationary -----------------------------------------------------------------------------------------------------------------------

// k_hadst_cov on the real observations, delta_ij on the padded ones; a tile whose rows are all padded only stores
template <int M>
__global__ __launch_bounds__(256) void k_hadcst_cov(const double* __restrict__ x, const int* __restrict__ indx,
                                                     const double* __restrict__ pars, long long P, const int* __restrict__ nobs,
                                                     int cps, double* __restrict__ S, int ld, int N, long long sstride) {
    constexpr int TJ = 64;
    __shared__ double su[TJ], sB[M * M], sp[3];
    __shared__ int sc[TJ];
    const int I = blockIdx.x, J = blockIdx.y;
    if (I < J) return;
    const int sub = blockIdx.z / cps;
    const int Ns = nobs[sub];
    x += (size_t)sub * N;
    indx += (size_t)sub * N;
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
    hadst_stage<M>(pars, P, x, indx, Ns, j0, sp, sB, su, sc);
    __syncthreads();
    if (i >= N) return;
    const bool real = i < Ns;
    const int ic = real ? i : 0;
    const double s2 = sp[1], s2e = sp[2];
    const double ui = x[ic] / sp[0];
    const double ui2 = ui * ui;
    const double* bi = sB + indx[ic] * M;
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
        const double uj = su[k];
        const double dist = (ui2 + uj * uj) - 2.0 * (ui * uj);          // kernels.py:20
        double kv = exp(-0.5 * dist) * s2;                              // kernels.py:42
        if (i == j) kv = NMGP_JITTER + kv;                              // kernels.py:35
        double v = kv * bi[sc[k]];
        if (i == j) v += s2e;
        S[(size_t)j * ld + i] = v;
    }
}

// k_hadst_adjoint with i, j < N_s: part[t][J][i] (component-major) of the real i, ZERO for the padded i (every J) and for tiles with
// nothing real, so that k_hadcst_grad_final reads nothing that nobody wrote.  A padded i has G_ii = -1/2; it reaches no sum.
template <int M>
__global__ __launch_bounds__(256) void k_hadcst_adjoint(const double* __restrict__ x, const int* __restrict__ indx,
                                                         const double* __restrict__ pars, long long P,
                                                         const double* __restrict__ alpha, const double* __restrict__ Sneg, int ld,
                                                         int N, const int* __restrict__ nobs, int cps, double* __restrict__ part,
                                                         long long pstride) {
    constexpr int TJ = 64;
    __shared__ double su[TJ], sB[M * M], sp[3], sR[TJ * M], sa[TJ];
    __shared__ int sc[TJ];
    __shared__ double red[2][4][64];
    const int I = blockIdx.x, J = blockIdx.y, NJ = gridDim.y;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int j0 = J * TJ;
    const size_t Nl = (size_t)N;
    const int sub = blockIdx.z / cps;
    const int Ns = nobs[sub];
    {   // blockIdx.z = chain
        const size_t z = blockIdx.z;
        x += (size_t)sub * Nl;
        indx += (size_t)sub * Nl;
        pars += z * (size_t)P;
        alpha += z * Nl;
        Sneg += z * (size_t)ld * Nl;
        part += z * (size_t)pstride;
    }
    const int i = I * 64 + lane;
    const bool inN = i < N;
    if (I * 64 >= Ns || j0 >= Ns) {                          // nothing real in the tile: zeros
        if (w == 0 && inN) {
#pragma unroll
            for (int t = 0; t < M + 2; ++t) part[((size_t)t * NJ + J) * Nl + i] = 0.0;
        }
        return;
    }
    hadst_stage<M>(pars, P, x, indx, Ns, j0, sp, sB, su, sc);
    if (tid < TJ) sa[tid] = (j0 + tid < Ns) ? alpha[j0 + tid] : 0.0;
    for (int k = tid; k < TJ * M; k += 256) {           // r_j = row c_j of L, zero-padded to M
        const int j = j0 + k / M, m = k % M;
        const int cj = (j < Ns) ? indx[j] : 0;
        sR[k] = (j < Ns && m <= cj) ? pars[2 + cj * (cj + 1) / 2 + m] : 0.0;
    }
    __syncthreads();
    const bool iv = i < Ns;
    const int ic = iv ? i : Ns - 1;
    const double s2 = sp[1], ai = alpha[ic];
    const double ui = x[ic] / sp[0];
    const double ui2 = ui * ui;
    const double* bi = sB + indx[ic] * M;
    double acc[M + 2];
#pragma unroll
    for (int t = 0; t < M + 2; ++t) acc[t] = 0.0;
    if (iv) {
        for (int jj = 0; jj < TJ / 4; ++jj) {
            const int k = w * (TJ / 4) + jj;
            const int j = j0 + k;
            if (j >= Ns) break;
            const double uj = su[k];
            const double dist = (ui2 + uj * uj) - 2.0 * (ui * uj);
            const double e = exp(-0.5 * dist) * s2;
            const double G = 0.5 * (ai * sa[k] + Sneg[(size_t)j * ld + i]);
            const double ge = G * e;
            const double gk = (i == j) ? G * (NMGP_JITTER + e) : ge;
            const double gb = ge * bi[sc[k]];
            acc[0] = fma(gb, dist, acc[0]);
            acc[1] += gb;
#pragma unroll
            for (int m = 0; m < M; ++m) acc[2 + m] = fma(gk, sR[k * M + m], acc[2 + m]);
        }
    }
#pragma unroll
    for (int t = 0; t < M + 2; ++t) {
        red[t & 1][w][lane] = acc[t];
        __syncthreads();
        // (a padded i < Nmax has four zero accumulators: +0.0)
        if (w == 0 && inN)
            part[((size_t)t * NJ + J) * Nl + i] =
                (red[t & 1][0][lane] + red[t & 1][1][lane]) + (red[t & 1][2][lane] + red[t & 1][3][lane]);
    }
}

// k_hadst_grad_final walking i < N_s only, with the subject's labels
__global__ __launch_bounds__(256) void k_hadcst_grad_final(const double* __restrict__ part, long long pstride, int NJ, int N, int M,
                                                            int T, const int* __restrict__ indx, const int* __restrict__ nobs, int cps,
                                                            const double* __restrict__ pars, const double* __restrict__ tr, double mu_l,
                                                            double var_l, double var_c, double a, double b, int prior,
                                                            double* __restrict__ grad) {
    __shared__ double sh[256];
    const int t = blockIdx.x, P = T + 3;
    const int sub = blockIdx.y / cps;
    const int Ns = nobs[sub];
    indx += (size_t)sub * N;
    part += (size_t)blockIdx.y * (size_t)pstride;
    pars += (size_t)blockIdx.y * P;
    tr += (size_t)blockIdx.y * 2;
    grad += (size_t)blockIdx.y * P;
    if (t == P - 1) {                      // (uniform over the workgroup)
        if (threadIdx.x == 0) {
            const double sigma2 = exp(pars[P - 1]);
            double g = sigma2 * (0.5 * (tr[0] - tr[1]));
            if (prior) g += (-a - 1.0) + b / sigma2 + 1.0;
            grad[P - 1] = -g;
        }
        return;
    }
    int comp = t, c = -1;                  // component of the partial rows; label of an L slot
    if (t >= 2) {
        const int tl = t - 2;
        c = 0;
        while ((c + 1) * (c + 2) / 2 <= tl) ++c;
        comp = 2 + (tl - c * (c + 1) / 2);
    }
    const double* pc = part + (size_t)comp * NJ * N;
    double acc = 0.0;
    for (int i = threadIdx.x; i < Ns; i += 256) {
        if (c >= 0 && indx[i] != c) continue;
        double sacc = 0.0;
        for (int J = 0; J < NJ; ++J) sacc += pc[(size_t)J * N + i];
        acc += sacc;
    }
    acc = block_sum_256(acc, sh);
    if (threadIdx.x == 0) {
        double g = (t == 0) ? acc : 2.0 * acc;
        if (prior && t == 0) g -= (pars[0] - mu_l) / var_l;
        if (prior && t >= 2) g -= pars[t] / var_c;
        grad[t] = -g;
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------

// what a model hook sees of a cohort chunk: the chunk's slice of the set's tables (chain z belongs to subject z / cps of the slice)
struct CohChunk {
    nmgp_ctx* c;
    const HadLayout& L;
    double* slab;
    int B, s0, cps, N, M, T;
    const double *x, *hyper;
    const int *indx, *nobs;
    int prior;
    bool want_grad;
    PriorFactor *p0, *p1;      // GP_PRIORS: the set's per-subject factors of hyper[1..2] and hyper[4..5]
    PriorStreamScope* ps;      // GP_PRIORS: the forked prior stream
    double* at(size_t o) const { return slab + o; }
};

// The GP-prior half of a cohort value epilogue (had_gp_prior_terms against the factors of subject s0 + z / cps): rhs(stream, R) fills
// R with the nc centred prior columns of every chain, zeros on the padded observations; then L X = R -> q = column sums of squares ->
// with gradients and priors R2 = Sigma_prior^-1 (v - mu).  Ends with the join, so the finaliser may follow.
template <class Rhs>
int hadc_gp_prior_terms(const CohChunk& k, int nc, Rhs rhs) {
    nmgp_ctx* c = k.c;
    PriorStreamScope& ps = *k.ps;
    const int N = k.N, B = k.B;
    double* R = k.at(k.L.o_R);
    const long long f0 = (long long)k.p0->ld * N, f1 = (long long)k.p1->ld * N;
    const double *L0 = k.p0->L + (size_t)k.s0 * f0, *L1 = k.p1->L + (size_t)k.s0 * f1;
    {
        NmgpStage sp(c, NMGP_STAGE_PRIOR, ps.sp, 0.0, 0.0);
        rhs(ps.sp, R);
        prior_trsv(ps.sp, false, L0, k.p0->ld, f0, L1, k.p1->ld, f1, R, N, nc, B, k.cps);
        col_sumsq(ps.sp, R, N, N, B * nc, k.at(k.L.o_q));
        if (k.want_grad && k.prior) {
            double* R2 = k.at(k.L.o_R2);
            HIP_TRY(c, hipMemcpyAsync(R2, R, (size_t)B * N * nc * sizeof(double), hipMemcpyDeviceToDevice, ps.sp));
            prior_trsv(ps.sp, true, L0, k.p0->ld, f0, L1, k.p1->ld, f1, R2, N, nc, B, k.cps);
        }
    }
    ps.done();
    ps.join();
    return 0;
}

// The three models as the cohort schedule sees them (the Model of nmgp_hadamard_common.h with the subject as a table look-up, and
// finite_in(p, Nmax, N_s, T): whether the REAL slots of a padded vector are finite); P, part_width and extras are the resident
// models', at N = Nmax.
struct CohNon {
    static constexpr int WIDTH = 5;
    static constexpr bool GP_PRIORS = true;
    static constexpr const char* NOUN = "Hadamard cohort";
    static constexpr int METRIC_LAYOUT = 0;       // the layout of prior_trmm_cohort (nmgp_metric.hip)
    static size_t P(int N, int T) { return (size_t)N * (1 + T) + 1; }
    static size_t part_width(int M) { return M + 1; }
    template <class Take>
    static void extras(HadLayout& L, Take take, size_t Bs, size_t N, int M, int T, bool want_grad) {
        L.o_ell = take(Bs * N); L.o_Rv = take(Bs * N * M); L.o_R = take(Bs * N * (1 + T)); L.o_q = take(Bs * (1 + T));
        if (want_grad) L.o_R2 = take(Bs * N * (1 + T));
    }
    static bool finite_in(const double* p, size_t N, size_t Ns, int T) { return hadc_finite_non(p, N, Ns, T); }
    // the padded layout [tilde_l (N) | L_vecs (N T) | tilde_sigma2_err] as the device sees it (hadc_finite_non walks the same slots):
    // whether slot i is real, the number of real slots, and the slot of the j-th real one
    __host__ __device__ static bool real_slot(long long i, int N, int Ns, int T) {
        return i < N ? i < Ns : (i < (long long)N * (1 + T) ? i - N < (long long)Ns * T : true);
    }
    __host__ __device__ static long long n_real(int Ns, int T) { return (long long)Ns * (1 + T) + 1; }
    __host__ __device__ static long long slot_of(long long j, int N, int Ns, int T) {
        return j < Ns ? j : (j < (long long)Ns * (1 + T) ? N + (j - Ns) : (long long)N * (1 + T));
    }
    static int build_cov(const CohChunk& k) {
        hipStream_t s = k.c->stream;
        double *dP = k.at(k.L.o_P), *ell = k.at(k.L.o_ell), *Rv = k.at(k.L.o_Rv);
        nmgp_hadc_prep(s, dP, k.indx, k.nobs, k.cps, k.N, k.M, k.T, ell, Rv, k.B);
        return hadc_cov_build<false>(s, k.x, ell, nullptr, Rv, dP, (long long)P(k.N, k.T), k.nobs, k.cps, k.at(k.L.o_S), k.L.ld, k.N, k.M,
                                     k.B, k.L.bs);
    }
    static int value_epilogue(const CohChunk& k) {
        const int N = k.N, T = k.T, B = k.B;
        double *dP = k.at(k.L.o_P), *scal = k.at(k.L.o_scal);
        NMGP_TRY(hadc_gp_prior_terms(k, 1 + T, [&](hipStream_t sp, double* R) {
            nmgp_hadc_prior_rhs(sp, dP, k.nobs, k.cps, N, T, k.hyper[0], k.hyper[3], R, N, B);
        }));
        NmgpStage sp(k.c, NMGP_STAGE_REDUCE);
        nmgp_hadc_finalize(k.c->stream, scal, k.at(k.L.o_q), k.p0->logdet + k.s0, k.p1->logdet + k.s0, dP, (long long)P(N, T), k.nobs, k.cps,
                           T, k.hyper[6], k.hyper[7], k.prior, B);
        return 0;
    }
    static int adjoint_grad(const CohChunk& k) {
        hipStream_t s = k.c->stream;
        const long long pstride = (long long)k.L.part_per;
        double* part = k.at(k.L.o_part);
        NMGP_TRY(hadc_adjoint<false>(s, k.x, k.at(k.L.o_ell), nullptr, k.at(k.L.o_Rv), k.at(k.L.o_alpha), k.at(k.L.o_Sneg), k.N, k.N, k.M,
                                     k.nobs, k.cps, part, pstride, k.B));
        nmgp_hadc_grad_final(s, part, pstride, k.N, k.M, k.T, k.indx, k.nobs, k.cps, k.at(k.L.o_R2), k.at(k.L.o_P), k.at(k.L.o_tr),
                             k.hyper[6], k.hyper[7], k.prior, k.at(k.L.o_grad), k.B);
        return 0;
    }
};

struct CohSep {
    static constexpr int WIDTH = 6;
    static constexpr bool GP_PRIORS = true;
    static constexpr const char* NOUN = "separable Hadamard cohort";
    static constexpr int METRIC_LAYOUT = 1;
    static size_t P(int N, int T) { return (size_t)2 * N + T + 1; }
    static size_t part_width(int M) { return M + 2; }
    template <class Take>
    static void extras(HadLayout& L, Take take, size_t Bs, size_t N, int M, int, bool want_grad) {
        L.o_ell = take(Bs * N); L.o_sig = take(Bs * N); L.o_Rv = take(Bs * N * M); L.o_R = take(Bs * N * 2); L.o_q = take(Bs * 2);
        if (want_grad) { L.o_R2 = take(Bs * N * 2); L.o_rsum = take(Bs * N * M); }
    }
    static bool finite_in(const double* p, size_t N, size_t Ns, int T) { return hadc_finite_sep(p, N, Ns, T); }
    // [tilde_l (N) | tilde_sigma (N) | L_vec (T) | tilde_sigma2_err] (hadc_finite_sep walks the same slots)
    __host__ __device__ static bool real_slot(long long i, int N, int Ns, int) { return i < N ? i < Ns : (i < 2LL * N ? i - N < Ns : true); }
    __host__ __device__ static long long n_real(int Ns, int T) { return 2LL * Ns + T + 1; }
    __host__ __device__ static long long slot_of(long long j, int N, int Ns, int) {
        return j < Ns ? j : (j < 2LL * Ns ? N + (j - Ns) : 2LL * N + (j - 2LL * Ns));
    }
    static int build_cov(const CohChunk& k) {
        hipStream_t s = k.c->stream;
        const int N = k.N, M = k.M, B = k.B;
        double *dP = k.at(k.L.o_P), *ell = k.at(k.L.o_ell), *sig = k.at(k.L.o_sig), *Rv = k.at(k.L.o_Rv);
        nmgp_hadcs_prep(s, dP, k.indx, k.nobs, k.cps, N, M, k.T, ell, sig, Rv, B);
        return hadc_cov_build<true>(s, k.x, ell, sig, Rv, dP, (long long)P(N, k.T), k.nobs, k.cps, k.at(k.L.o_S), k.L.ld, N, M, B, k.L.bs);
    }
    static int value_epilogue(const CohChunk& k) {
        const int N = k.N, T = k.T, B = k.B;
        const NormalF32 nc(0.0, k.hyper[8]);
        double *dP = k.at(k.L.o_P), *scal = k.at(k.L.o_scal);
        NMGP_TRY(hadc_gp_prior_terms(k, 2, [&](hipStream_t sp, double* R) {
            NMGP_LAUNCH(k_hadcs_prior_rhs, dim3(cdiv(N, 256), B), dim3(256), 0, sp, dP, k.nobs, k.cps, N, T, k.hyper[0], k.hyper[3], R);
        }));
        NmgpStage sp(k.c, NMGP_STAGE_REDUCE);
        NMGP_LAUNCH(k_hadcs_finalize, dim3(B), dim3(64), 0, k.c->stream, scal, k.at(k.L.o_q), k.p0->logdet + k.s0, k.p1->logdet + k.s0, dP,
                    k.nobs, k.cps, N, T, k.hyper[6], k.hyper[7], nc.var, nc.log_sd, k.prior, scal + 8);
        return 0;
    }
    static int adjoint_grad(const CohChunk& k) {
        hipStream_t s = k.c->stream;
        const int N = k.N, M = k.M, T = k.T, B = k.B, NJ = (N + 63) / 64;
        const long long pstride = (long long)k.L.part_per;
        const NormalF32 nc(0.0, k.hyper[8]);
        double *dP = k.at(k.L.o_P), *part = k.at(k.L.o_part), *rsum = k.at(k.L.o_rsum), *dg = k.at(k.L.o_grad);
        NMGP_TRY(hadc_adjoint<true>(s, k.x, k.at(k.L.o_ell), k.at(k.L.o_sig), k.at(k.L.o_Rv), k.at(k.L.o_alpha), k.at(k.L.o_Sneg), N, N, M,
                                    k.nobs, k.cps, part, pstride, B));
        NMGP_LAUNCH(k_hadcs_grad_obs, dim3(cdiv(N, 256), B), dim3(256), 0, s, part, pstride, NJ, N, M, T, k.nobs, k.cps, k.at(k.L.o_R2), dP,
                    k.at(k.L.o_tr), k.hyper[6], k.hyper[7], k.prior, rsum, dg);
        NMGP_LAUNCH(k_hadcs_grad_lvec, dim3(T, B), dim3(256), 0, s, rsum, k.indx, k.nobs, k.cps, N, M, T, dP, nc.var, k.prior, dg);
        return 0;
    }
};

struct CohSta {
    static constexpr int WIDTH = 5;
    static constexpr bool GP_PRIORS = false;
    static constexpr const char* NOUN = "stationary Hadamard cohort";
    static constexpr int METRIC_LAYOUT = -1;      // no GP prior: no prior-factor metric
    static size_t P(int, int T) { return (size_t)T + 3; }
    static size_t part_width(int M) { return M + 2; }
    template <class Take>
    static void extras(HadLayout&, Take, size_t, size_t, int, int, bool) {}
    static bool finite_in(const double* p, size_t N, size_t Ns, int T) { return hadc_finite_sta(p, N, Ns, T); }
    // all T + 3 slots are real (hadc_finite_sta)
    __host__ __device__ static bool real_slot(long long, int, int, int) { return true; }
    __host__ __device__ static long long n_real(int, int T) { return (long long)T + 3; }
    __host__ __device__ static long long slot_of(long long j, int, int, int) { return j; }
    static int build_cov(const CohChunk& k) {
        return nmgp_hadcst_cov_build(k.c->stream, k.x, k.indx, k.at(k.L.o_P), (long long)P(k.N, k.T), k.nobs, k.cps, k.at(k.L.o_S), k.L.ld,
                                     k.N, k.M, k.B, k.L.bs);
    }
    static int value_epilogue(const CohChunk& k) {           // no term of the tuple depends on N: the resident finaliser as it is
        nmgp_hadst_finalize(k.c->stream, k.at(k.L.o_scal), k.at(k.L.o_P), k.T, k.hyper, k.prior, k.B);
        return 0;
    }
    static int adjoint_grad(const CohChunk& k) {
        hipStream_t s = k.c->stream;
        const int N = k.N, M = k.M, T = k.T;
        const long long P_ = (long long)P(N, T), pstride = (long long)k.L.part_per;
        const NormalF32 nl(k.hyper[0], k.hyper[1]), nc(0.0, k.hyper[4]);
        double *dP = k.at(k.L.o_P), *part = k.at(k.L.o_part);
        const dim3 grid(cdiv(N, 64), cdiv(N, 64), k.B);
        NMGP_HADS_SWITCH(M, NMGP_LAUNCH((k_hadcst_adjoint<MM>), grid, dim3(256), 0, s, k.x, k.indx, dP, P_, k.at(k.L.o_alpha),
                                        k.at(k.L.o_Sneg), N, N, k.nobs, k.cps, part, pstride));
        NMGP_LAUNCH(k_hadcst_grad_final, dim3((unsigned)P_, k.B), dim3(256), 0, s, part, pstride, (N + 63) / 64, N, M, T, k.indx, k.nobs,
                    k.cps, dP, k.at(k.L.o_tr), nl.mean, nl.var, nc.var, k.hyper[2], k.hyper[3], k.prior, k.at(k.L.o_grad));
        return 0;
    }
};

// The ENQUEUE half of a chunk's evaluation: chains [0, B), chain z belonging to subject s0 + z / cps, positions already on the device
// at slab + L.o_P; had_eval_chunk's sequence at n = Nmax with the model's hooks, value and gradient halves back to back.  Leaves
// info / scal (and with want_grad the gradient rows at slab + L.o_grad) in the slab.  Nothing here touches the host or synchronises:
// the evaluation entries follow it with cohm_chunk_epilogue, the trajectories with device copies.
template <class Model>
int cohm_enqueue_chunk(nmgp_ctx* c, const HadLayout& L, double* slab, int B, int s0, int cps, const double* hyper, int prior,
                       PriorFactor* p0, PriorFactor* p1, bool want_grad) {
    const int N = c->hc_Nmax, M = c->hc_M, T = c->hc_T;
    hipStream_t s = c->stream;
    double *z = slab + L.o_z, *scal = slab + L.o_scal, *S = slab + L.o_S;
    int* info = reinterpret_cast<int*>(slab + L.o_info);
    const int ld = L.ld;
    const long long bs = L.bs;
    // the tables of the chunk's first subject
    const double* y = c->hc_y + (size_t)s0 * N;
    const int* nobs = c->hc_nobs + s0;
    HIP_TRY(c, hipMemsetAsync(info, 0, (size_t)B * sizeof(int), s));
    std::optional<PriorStreamScope> ps;          // fork now, enqueue the prior solves after the factorisation's launches
    if constexpr (Model::GP_PRIORS) ps.emplace(c);
    const CohChunk k{c, L, slab, B, s0, cps, N, M, T, c->hc_x + (size_t)s0 * N, hyper, c->hc_indx + (size_t)s0 * N, nobs, prior,
                     want_grad, p0, p1, ps ? &*ps : nullptr};
    {
        NmgpStage sp(c, NMGP_STAGE_COV);
        int r = Model::build_cov(k);
        if (r) return nmgp_fail(c, r, "unsupported number of outputs M=%d", M);
    }
    {
        NmgpStage sp(c, NMGP_STAGE_CHOL);
        set_row(s, S, ld, N, y, N, B, bs, N, cps);                        // y (zero-padded at set time) rides along as row Nmax
        if (want_grad) identity_rows(s, S, ld, N + 1, N, L.xpad, B, bs);
        nmgp_potrf(c, S, ld, N, want_grad ? 1 + L.xpad : 1, want_grad ? N : 0, info, B, bs, 1);
        get_row(s, S, ld, N, z, N, B, bs, N);                             // z = L^-1 y
    }
    {
        NmgpStage sp(c, NMGP_STAGE_REDUCE);
        chol_logdet_quad(s, S, ld, N, z, scal, scal + 1, B, bs, 16);
        if constexpr (!Model::GP_PRIORS) NMGP_TRY(Model::value_epilogue(k));     // the finaliser alone: in this stage
    }
    if constexpr (Model::GP_PRIORS) NMGP_TRY(Model::value_epilogue(k));          // prior stream, join, finaliser (a stage of its own)
    if (want_grad) {
        double *alpha = slab + L.o_alpha, *Sneg = slab + L.o_Sneg, *part = slab + L.o_part;
        {
            NmgpStage sp(c, NMGP_STAGE_SOLVE);
            tri_gemv_upper(s, S + L.xoff, ld, N, z, alpha, part, B, bs, (long long)L.part_per);    // alpha = L^-T z = X z
        }
        {
            NmgpStage sp(c, NMGP_STAGE_INVERSE);
            syrk_lower(s, S + L.xoff, ld, Sneg, N, N, N, N, B, bs, (long long)N * N, 2);          // -S^-1 = -X X^T, both triangles
        }
        {
            NmgpStage sp(c, NMGP_STAGE_ADJOINT);
            nmgp_hadc_trace(s, alpha, Sneg, N, N, nobs, cps, slab + L.o_tr, -1.0, B);             // over the real observations
            int r = Model::adjoint_grad(k);
            if (r) return nmgp_fail(c, r, "unsupported number of outputs M=%d", M);
        }
    }
    return 0;
}

// The HOST epilogue of a chunk's evaluation: the copies out of the slab, the ONE synchronisation of the chunk, and the status loop
// (`pars` are the caller's rows: the NMGP_NUM_NAN test reads their real slots).
template <class Model>
int cohm_chunk_epilogue(nmgp_ctx* c, const HadLayout& L, double* slab, const double* pars, int B, int s0, int cps, double* out,
                        double* grad, int* status) {
    constexpr int W = Model::WIDTH;
    const int N = c->hc_Nmax, T = c->hc_T;
    const size_t P = Model::P(N, T);
    const bool want_grad = grad != nullptr;
    hipStream_t s = c->stream;
    std::vector<double> hs((size_t)B * 16);
    std::vector<int> hi(B);
    HIP_TRY(c, hipMemcpyAsync(hs.data(), slab + L.o_scal, hs.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(hi.data(), slab + L.o_info, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, s));
    if (want_grad) HIP_TRY(c, hipMemcpyAsync(grad, slab + L.o_grad, (size_t)B * P * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));          // the one synchronisation of the chunk
    NMGP_TRY(nmgp_take_launch_error(c));
    for (int z_ = 0; z_ < B; ++z_) {
        int st = hi[z_];
        double* o = out + (size_t)z_ * W;
        for (int t = 0; t < W; ++t) o[t] = hs[(size_t)z_ * 16 + 8 + t];
        const bool finite_in = Model::finite_in(pars + (size_t)z_ * P, (size_t)N, (size_t)c->hc_nobs_h[s0 + z_ / cps], T);
        if (!finite_in || (st == 0 && (!std::isfinite(o[0]) || !std::isfinite(o[1])))) st = NMGP_NUM_NAN;
        if (st != 0) {
            for (int t = 0; t < W; ++t) o[t] = std::nan("");
            if (want_grad) std::fill(grad + (size_t)z_ * P, grad + (size_t)(z_ + 1) * P, 0.0);
        }
        status[z_] = st;
    }
    return 0;
}

// chains [0, B) of `pars` (already offset by the caller): the upload, the two halves back to back, ONE synchronisation.
template <class Model>
int cohm_eval_chunk(nmgp_ctx* c, const double* pars, int B, int s0, int cps, const double* hyper, int prior, PriorFactor* p0,
                    PriorFactor* p1, double* out, double* grad, int* status) {
    const int N = c->hc_Nmax, M = c->hc_M, T = c->hc_T;
    const size_t P = Model::P(N, T);
    const bool want_grad = grad != nullptr;
    const HadLayout L = had_layout<Model>(B, N, M, T, want_grad);
    double* slab;
    NMGP_TRY(nmgp_scratch_get(c, HSL_SLAB, L.total, &slab));
    HIP_TRY(c, hipMemcpyAsync(slab + L.o_P, pars, (size_t)B * P * sizeof(double), hipMemcpyHostToDevice, c->stream));
    NMGP_TRY(cohm_enqueue_chunk<Model>(c, L, slab, B, s0, cps, hyper, prior, p0, p1, want_grad));
    return cohm_chunk_epilogue<Model>(c, L, slab, pars, B, s0, cps, out, grad, status);
}

template <class Model>
int cohm_subjects_eval(nmgp_ctx* c, const double* pars, int B, int cps, const double* hyper, int prior, double* out, double* grad,
                       int* status) {
    if (!c) return NMGP_E_NULL;
    if (!pars || !hyper || !out || !status)
        return nmgp_fail(c, NMGP_E_NULL, "pars/hyper/out%d/status must not be NULL", Model::WIDTH);
    if (c->hc_S <= 0) return nmgp_fail(c, NMGP_E_STATE, "nmgp_had_set_subjects must be called first");
    if (c->chol_algo != 1)
        return nmgp_fail(c, NMGP_E_UNSUPPORTED, "the Hadamard entries run on the custom factorisation only (riding rows)");
    if (cps < 1 || (long long)B != (long long)c->hc_S * cps)
        return nmgp_fail(c, NMGP_E_SHAPE, "B = %d must be %d subjects x chains_per_subject = %d", B, c->hc_S, cps);
    HIP_TRY(c, hipSetDevice(c->device));
    const int N = c->hc_Nmax, M = c->hc_M, T = c->hc_T;
    const size_t P = Model::P(N, T);
    const bool want_grad = grad != nullptr;
    // one pair of factors per subject (the cache is a vector: the second look-up may move its elements, so the first is re-resolved)
    PriorFactor *p0 = nullptr, *p1 = nullptr;
    if constexpr (Model::GP_PRIORS) NMGP_TRY(nmgp_hadc_priors(c, hyper, &p0, &p1));
    const size_t per_chain = had_layout<Model>(1, N, M, T, want_grad).total * sizeof(double);
    return had_for_chunks(c, B, cps, per_chain, Model::NOUN, "at Nmax", N, [&](int b0, int nb, int s0, int ccps) {
        return cohm_eval_chunk<Model>(c, pars + (size_t)b0 * P, nb, s0, ccps, hyper, prior, p0, p1, out + (size_t)b0 * Model::WIDTH,
                                      want_grad ? grad + (size_t)b0 * P : nullptr, status + b0);
    });
}


// ---- device-resident leapfrog trajectories of the cohort (drivers._HadamardCohortHMC) ------------------------------------------------
// nmgp_svc_batch_traj's loop on the padded rows of a subject set: q, p, g stay in HBM between the chunked evaluations of a
// trajectory.  Every mask comes from the nobs table and the model's layout (Model::real_slot), never from a slot's contents; the step
// size is the subject's.  The arithmetic is the host loop's of drivers._HadamardCohortHMC, operation for operation, so both give the
// same bits.

// after a chunk's evaluation: bad[z] = the potential is undefined for chain z (factorisation status, a non-finite value, or a real
// slot of the position that went non-finite: the three tests of cohm_chunk_epilogue); failed |= bad; U[z] = NegLog (the slab is the
// next chunk's)
__global__ void k_hadc_hmc_status(const int* __restrict__ info, const double* __restrict__ scal, const int* __restrict__ qbad,
                                  int* __restrict__ bad, int* __restrict__ failed, double* __restrict__ U, int B) {
    const int z = blockIdx.x * blockDim.x + threadIdx.x;
    if (z >= B) return;
    const double v0 = scal[(size_t)z * 16 + 8], v1 = scal[(size_t)z * 16 + 9];
    const int b = (qbad[z] != 0 || info[z] != 0 || !isfinite(v0) || !isfinite(v1)) ? 1 : 0;
    bad[z] = b;
    if (b) failed[z] = 1;
    U[z] = v0;
}

// Rows z0 + blockIdx.y of the set, subject z / cps.  Real slots: p -= (kick eps[s]) g for the chains whose gradient is defined, then
// -- if drift -- q += eps[s] (minv p).  Padded slots are neither read nor written, except that the FIRST kick of a trajectory
// writes +0.0 to the padded slots of p.  Statement by statement as k_hmc_kick_drift (the build has no contraction).
template <class Model>
__global__ __launch_bounds__(256) void k_hadc_hmc_kick_drift(double* __restrict__ p, const double* __restrict__ g, double* __restrict__ q,
                                                              const double* __restrict__ minv, const int* __restrict__ bad,
                                                              int* __restrict__ qbad, const int* __restrict__ nobs,
                                                              const double* __restrict__ eps, int cps, int z0, double kick, int drift,
                                                              int first, int N, int T, long long P) {
    const int z = z0 + blockIdx.y;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const int s = z / cps;
    const size_t o = (size_t)z * P + i;
    if (!Model::real_slot(i, N, nobs[s], T)) {
        if (first) p[o] = 0.0;
        return;
    }
    const double e = eps[s];
    const double c = kick * e;
    double pv = p[o];
    if (!bad[z]) {
        const double t = c * g[o];
        pv = pv - t;
        p[o] = pv;
    }
    if (drift) {
        const double v = minv ? minv[o] * pv : pv;
        const double t2 = e * v;
        const double qn = q[o] + t2;
        q[o] = qn;
        if (!isfinite(qn)) qbad[z] = 1;          // (every writer stores the same word)
    }
}

// kin[z] = 1/2 sum over the REAL slots of p v, v = minv p or p.  One workgroup per chain, k_hmc_kinetic's order on the chain's real
// slots counted without the padding (slot_of): a strided fma partial per thread, then the shared-memory tree -- so the bits depend
// on the chain alone, not on Nmax, B, the chunking or the other subjects.
template <class Model>
__global__ __launch_bounds__(256) void k_hadc_hmc_kinetic(const double* __restrict__ p, const double* __restrict__ minv,
                                                           const int* __restrict__ nobs, int cps, int N, int T, long long P,
                                                           double* __restrict__ kin) {
    __shared__ double red[256];
    const int z = blockIdx.x, t = threadIdx.x;
    const int Ns = nobs[z / cps];
    const long long nr = Model::n_real(Ns, T);
    const double* pz = p + (size_t)z * P;
    const double* mz = minv ? minv + (size_t)z * P : nullptr;
    double acc = 0.0;
    for (long long j = t; j < nr; j += 256) {
        const long long i = Model::slot_of(j, N, Ns, T);
        const double pv = pz[i];
        const double v = mz ? mz[i] * pv : pv;
        acc = fma(pv, v, acc);
    }
    red[t] = acc;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h) red[t] += red[t + h];
        __syncthreads();
    }
    if (t == 0) kin[z] = 0.5 * red[0];
}

// rejected chains (accept[z] == 0) get the real slots of their position and gradient, and their validity flag, back (k_hmc_restore;
// padded slots of q never change)
template <class Model>
__global__ __launch_bounds__(256) void k_hadc_hmc_restore(double* __restrict__ q, double* __restrict__ g, const double* __restrict__ q0,
                                                           const double* __restrict__ g0, int* __restrict__ bad,
                                                           const int* __restrict__ bad0, const int* __restrict__ accept,
                                                           const int* __restrict__ nobs, int cps, int z0, int N, int T, long long P) {
    const int z = z0 + blockIdx.y;
    if (accept[z]) return;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) bad[z] = bad0[z];
    if (i >= P || !Model::real_slot(i, N, nobs[z / cps], T)) return;
    const size_t o = (size_t)z * P + i;
    q[o] = q0[o];
    g[o] = g0[o];
}

// flag rows of ht_flags
inline int* ht_bad(nmgp_ctx* c) { return c->ht_flags; }
inline int* ht_bad0(nmgp_ctx* c) { return c->ht_flags + c->ht_B; }
inline int* ht_failed(nmgp_ctx* c) { return c->ht_flags + 2 * (size_t)c->ht_B; }
inline int* ht_accept(nmgp_ctx* c) { return c->ht_flags + 3 * (size_t)c->ht_B; }
inline int* ht_qbad(nmgp_ctx* c) { return c->ht_flags + 4 * (size_t)c->ht_B; }

// the elementwise launches over all B rows: the row is a grid dimension, so more than 65535 rows take several launches
template <class Model>
void cohm_kick_drift(nmgp_ctx* c, double kick, int drift, int first) {
    const long long P = (long long)c->ht_P;
    for (int z0 = 0; z0 < c->ht_B; z0 += 65535) {
        const int nz = std::min(65535, c->ht_B - z0);
        NMGP_LAUNCH((k_hadc_hmc_kick_drift<Model>), dim3((unsigned)((P + 255) / 256), nz), dim3(256), 0, c->stream, c->ht_p, c->ht_g,
                    c->ht_q, c->ht_mass == 1 ? c->ht_minv : nullptr, ht_bad(c), ht_qbad(c), c->hc_nobs, c->ht_eps, c->ht_cps, z0, kick,
                    drift, first, c->hc_Nmax, c->hc_T, P);
    }
}

// The two products of a leapfrog step under the PRIOR-FACTOR METRIC (mass kind 2; k_prior_trmm_coh, nmgp_metric.hip), over all B rows,
// with the set's cached per-subject factors of the trajectory's hyper-parameters -- the trajectory holds no copy of a factor:
//   kick   u -= (kick eps_s) L_blk,s^T g   skipped for bad chains; the first one writes +0.0 to the padded slots of u
//   drift  q += eps_s L_blk,s u            sets qbad where a real slot of q becomes non-finite
// ht_p carries the whitened momentum u; the kinetic energy is k_hadc_hmc_kinetic's without minv.
template <class Model>
void cohm_metric_product(nmgp_ctx* c, const PriorFactor* p0, const PriorFactor* p1, bool kick_not_drift, double kick, int first) {
    if constexpr (Model::GP_PRIORS) {
        const int N = c->hc_Nmax;
        const double cscale = Model::METRIC_LAYOUT == 1 ? (double)(float)c->ht_hyper[8] : 1.0;
        if (kick_not_drift)
            prior_trmm_cohort(c->stream, Model::METRIC_LAYOUT, true, p0->L, p0->ld, (long long)p0->ld * N, p1->L, p1->ld,
                              (long long)p1->ld * N, c->ht_g, c->ht_p, c->hc_nobs, c->ht_eps, c->ht_cps, N, c->hc_T, (long long)c->ht_P,
                              c->ht_B, kick, 2, ht_bad(c), nullptr, first, cscale);
        else
            prior_trmm_cohort(c->stream, Model::METRIC_LAYOUT, false, p0->L, p0->ld, (long long)p0->ld * N, p1->L, p1->ld,
                              (long long)p1->ld * N, c->ht_p, c->ht_q, c->hc_nobs, c->ht_eps, c->ht_cps, N, c->hc_T, (long long)c->ht_P,
                              c->ht_B, 1.0, 1, nullptr, ht_qbad(c), 0, cscale);
    }
}

// a kick (and, if drift, the drift after it) under the trajectory's mass
template <class Model>
void cohm_step(nmgp_ctx* c, const PriorFactor* p0, const PriorFactor* p1, double kick, int drift, int first) {
    if (c->ht_mass != 2) {
        cohm_kick_drift<Model>(c, kick, drift, first);
        return;
    }
    cohm_metric_product<Model>(c, p0, p1, true, kick, first);
    if (drift) cohm_metric_product<Model>(c, p0, p1, false, 1.0, 0);
}

// One value+gradient evaluation of RESIDENT rows q [B, P], chunk by chunk (the chunks of cohm_subjects_eval): positions into the slab,
// the enqueue half, then after(b0, nb, s0, cps of the chunk, L, slab) takes what it needs out of the slab (info, scal, the gradient
// rows at slab + L.o_grad) with work on the stream.  No host synchronisation: the slab's reuse by the next chunk is ordered by the
// stream.  The trajectories and the optimiser share it.
template <class Model, class After>
int cohm_resident_eval(nmgp_ctx* c, const double* q, int B, int cps, const double* hyper, int prior, After after) {
    const int N = c->hc_Nmax, M = c->hc_M, T = c->hc_T;
    const size_t P = Model::P(N, T);
    hipStream_t s = c->stream;
    PriorFactor *p0 = nullptr, *p1 = nullptr;
    if constexpr (Model::GP_PRIORS) NMGP_TRY(nmgp_hadc_priors(c, hyper, &p0, &p1));
    const size_t per_chain = had_layout<Model>(1, N, M, T, true).total * sizeof(double);
    return had_for_chunks(c, B, cps, per_chain, Model::NOUN, "at Nmax", N, [&](int b0, int nb, int s0, int ccps) {
        const HadLayout L = had_layout<Model>(nb, N, M, T, true);
        double* slab;
        NMGP_TRY(nmgp_scratch_get(c, HSL_SLAB, L.total, &slab));
        HIP_TRY(c, hipMemcpyAsync(slab + L.o_P, q + (size_t)b0 * P, (size_t)nb * P * sizeof(double), hipMemcpyDeviceToDevice, s));
        NMGP_TRY(cohm_enqueue_chunk<Model>(c, L, slab, nb, s0, ccps, hyper, prior, p0, p1, true));
        return after(b0, nb, s0, ccps, L, slab);
    });
}

// the trajectories' evaluation: gradient rows out, status and potential out
template <class Model>
int cohm_traj_eval(nmgp_ctx* c) {
    const size_t P = c->ht_P;
    hipStream_t s = c->stream;
    return cohm_resident_eval<Model>(c, c->ht_q, c->ht_B, c->ht_cps, c->ht_hyper, c->ht_prior,
                                     [&](int b0, int nb, int, int, const HadLayout& L, double* slab) {
        HIP_TRY(c, hipMemcpyAsync(c->ht_g + (size_t)b0 * P, slab + L.o_grad, (size_t)nb * P * sizeof(double), hipMemcpyDeviceToDevice, s));
        NMGP_LAUNCH(k_hadc_hmc_status, dim3(cdiv(nb, 64)), dim3(64), 0, s, reinterpret_cast<const int*>(slab + L.o_info),
                    slab + L.o_scal, ht_qbad(c) + b0, ht_bad(c) + b0, ht_failed(c) + b0, c->ht_U + b0, nb);
        return 0;
    });
}

// An API-level failure inside a trajectory call puts the start state back and demands a fresh begin (traj_abort of the complete-data
// family); the first failure's message is kept.
int cohm_traj_abort(nmgp_ctx* c, int rc) {
    const size_t bytes = (size_t)c->ht_B * c->ht_P * sizeof(double);
    const std::string msg = c->err;
    hipMemcpyAsync(c->ht_q, c->ht_q0, bytes, hipMemcpyDeviceToDevice, c->stream);
    hipMemcpyAsync(c->ht_g, c->ht_g0, bytes, hipMemcpyDeviceToDevice, c->stream);
    hipMemcpyAsync(ht_bad(c), ht_bad0(c), (size_t)c->ht_B * sizeof(int), hipMemcpyDeviceToDevice, c->stream);
    hipStreamSynchronize(c->stream);
    (void)hipGetLastError();
    c->ht_model = -1;          // (the buffers go with the next begin, end or set)
    c->err = msg;
    return rc;
}

template <class Model>
int cohm_subjects_traj_begin(nmgp_ctx* c, int model, const double* pars, int B, int cps, const double* hyper, int prior, double* out,
                             int* status) {
    const size_t P = Model::P(c->hc_Nmax, c->hc_T), n = (size_t)B * P;
    // the start point is the evaluation entry's, bits and failing rows included; its gradient rows go back up next to the positions
    std::vector<double> grad(n);
    NMGP_TRY(cohm_subjects_eval<Model>(c, pars, B, cps, hyper, prior, out, grad.data(), status));
    nmgp_had_traj_free(c);
    auto fail = [c](int r) {
        const std::string msg = c->err;
        nmgp_had_traj_free(c);
        c->err = msg;
        return r;
    };
    double** bufs[] = {&c->ht_q, &c->ht_p, &c->ht_g, &c->ht_q0, &c->ht_g0};
    for (double** b : bufs)
        if (int r = nmgp_dev_alloc(c, b, n)) return fail(r);
    if (nmgp_dev_alloc(c, &c->ht_U, (size_t)B) != 0 || nmgp_dev_alloc(c, &c->ht_kin, (size_t)B) != 0 ||
        nmgp_dev_alloc(c, &c->ht_eps, (size_t)c->hc_S) != 0)
        return fail(NMGP_E_NOMEM);
    if (hipMalloc((void**)&c->ht_flags, 5 * (size_t)B * sizeof(int)) != hipSuccess)
        return fail(nmgp_fail(c, NMGP_E_NOMEM, "hipMalloc of the trajectory flags failed"));
    std::vector<int> bad(B);
    for (int z = 0; z < B; ++z) bad[z] = status[z] != 0;
    hipStream_t s = c->stream;
    bool ok = hipMemcpyAsync(c->ht_q, pars, n * sizeof(double), hipMemcpyHostToDevice, s) == hipSuccess &&
              hipMemcpyAsync(c->ht_g, grad.data(), n * sizeof(double), hipMemcpyHostToDevice, s) == hipSuccess &&
              hipMemsetAsync(c->ht_flags, 0, 5 * (size_t)B * sizeof(int), s) == hipSuccess &&
              hipMemcpyAsync(c->ht_flags, bad.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice, s) == hipSuccess &&
              hipStreamSynchronize(s) == hipSuccess;          // the sources are the caller's and this frame's
    if (!ok) return fail(nmgp_fail(c, NMGP_E_HIP, "upload of the trajectory's start state failed (%s)", hipGetErrorString(hipGetLastError())));
    c->ht_model = model;
    c->ht_B = B;
    c->ht_cps = cps;
    c->ht_prior = prior;
    c->ht_P = P;
    c->ht_mass = 0;
    std::copy(hyper, hyper + (model == 0 ? 8 : model == 1 ? 9 : 5), c->ht_hyper);
    return 0;
}

template <class Model>
int cohm_subjects_traj_set_mass(nmgp_ctx* c, int kind, const double* minv) {
    const int N = c->hc_Nmax, T = c->hc_T, B = c->ht_B;
    const size_t P = c->ht_P;
    if (kind == 2) {
        if constexpr (!Model::GP_PRIORS)
            return nmgp_fail(c, NMGP_E_UNSUPPORTED, "the stationary model has no GP prior: no prior-factor metric (kind 2)");
        else {
            PriorFactor *p0 = nullptr, *p1 = nullptr;      // (cached by begin; a failure here leaves the mass as it was)
            NMGP_TRY(nmgp_hadc_priors(c, c->ht_hyper, &p0, &p1));
        }
    }
    if (kind == 1)
        for (int z = 0; z < B; ++z) {
            const int Ns = c->hc_nobs_h[z / c->ht_cps];
            for (size_t i = 0; i < P; ++i) {
                const double m = minv[(size_t)z * P + i];
                if (Model::real_slot((long long)i, N, Ns, T) && !(m > 0.0 && std::isfinite(m)))
                    return nmgp_fail(c, NMGP_E_SHAPE, "minv[%d, %zu] = %g: diag(M^-1) must be finite and > 0 in every real slot", z, i, m);
            }
        }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (kind == 1) {
        if (!c->ht_minv) NMGP_TRY(nmgp_dev_alloc(c, &c->ht_minv, (size_t)B * P));
        HIP_TRY(c, hipMemcpyAsync(c->ht_minv, minv, (size_t)B * P * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    c->ht_mass = kind;
    return 0;
}

// nsteps leapfrog steps from the resident state with momenta p0: one chunked evaluation per step, the elementwise kernels over all B
// rows between them, ONE synchronisation at the end however many chunks the set needs.
template <class Model>
int cohm_subjects_traj(nmgp_ctx* c, const double* eps, int nsteps, const double* p0, double* q1, double* p1, double* kin1, double* U1,
                       int* failed) {
    const int B = c->ht_B;
    const size_t P = c->ht_P, bytes = (size_t)B * P * sizeof(double);
    hipStream_t s = c->stream;
    PriorFactor *f0 = nullptr, *f1 = nullptr;                 // kind 2: the set's factors, resolved before anything of the state is touched
    if constexpr (Model::GP_PRIORS)                           // (no look-up inside the trajectory grows the cache)
        if (c->ht_mass == 2) NMGP_TRY(nmgp_hadc_priors(c, c->ht_hyper, &f0, &f1));
    HIP_TRY(c, hipMemcpyAsync(c->ht_eps, eps, (size_t)c->hc_S * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(c->ht_p, p0, bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(c->ht_q0, c->ht_q, bytes, hipMemcpyDeviceToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(c->ht_g0, c->ht_g, bytes, hipMemcpyDeviceToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(ht_bad0(c), ht_bad(c), (size_t)B * sizeof(int), hipMemcpyDeviceToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(ht_failed(c), ht_bad(c), (size_t)B * sizeof(int), hipMemcpyDeviceToDevice, s));   // bad at the start: failed
    HIP_TRY(c, hipMemsetAsync(ht_qbad(c), 0, (size_t)B * sizeof(int), s));
    cohm_step<Model>(c, f0, f1, 0.5, 1, 1);
    for (int step = 0; step < nsteps; ++step) {
        if (int rc = cohm_traj_eval<Model>(c)) return cohm_traj_abort(c, rc);
        const bool last = step == nsteps - 1;
        cohm_step<Model>(c, f0, f1, last ? 0.5 : 1.0, last ? 0 : 1, 0);
    }
    if (kin1)
        NMGP_LAUNCH((k_hadc_hmc_kinetic<Model>), dim3(B), dim3(256), 0, s, c->ht_p, c->ht_mass == 1 ? c->ht_minv : nullptr, c->hc_nobs,
                    c->ht_cps, c->hc_Nmax, c->hc_T, (long long)P, c->ht_kin);
    hipError_t e = hipMemcpyAsync(q1, c->ht_q, bytes, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && p1) e = hipMemcpyAsync(p1, c->ht_p, bytes, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && kin1) e = hipMemcpyAsync(kin1, c->ht_kin, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(U1, c->ht_U, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(failed, ht_failed(c), (size_t)B * sizeof(int), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);          // the one synchronisation of the trajectory
    if (e != hipSuccess)
        return cohm_traj_abort(c, nmgp_fail(c, NMGP_E_HIP, "the end of the trajectory failed: %s", hipGetErrorString(e)));
    if (int rc = nmgp_take_launch_error(c)) return cohm_traj_abort(c, rc);
    for (int z = 0; z < B; ++z)
        if (failed[z]) U1[z] = INFINITY;
    return 0;
}

template <class Model>
int cohm_subjects_traj_commit(nmgp_ctx* c, const int* accept) {
    const long long P = (long long)c->ht_P;
    HIP_TRY(c, hipMemcpyAsync(ht_accept(c), accept, (size_t)c->ht_B * sizeof(int), hipMemcpyHostToDevice, c->stream));
    for (int z0 = 0; z0 < c->ht_B; z0 += 65535) {
        const int nz = std::min(65535, c->ht_B - z0);
        NMGP_LAUNCH((k_hadc_hmc_restore<Model>), dim3((unsigned)((P + 255) / 256), nz), dim3(256), 0, c->stream, c->ht_q, c->ht_g, c->ht_q0,
                    c->ht_g0, ht_bad(c), ht_bad0(c), ht_accept(c), c->hc_nobs, c->ht_cps, z0, c->hc_Nmax, c->hc_T, P);
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));        // `accept` is the caller's buffer
    return nmgp_take_launch_error(c);
}

// the begun trajectory, or the refusal
int cohm_traj_require(nmgp_ctx* c) {
    if (c->hc_S <= 0) return nmgp_fail(c, NMGP_E_STATE, "nmgp_had_set_subjects must be called first");
    if (c->ht_model < 0) return nmgp_fail(c, NMGP_E_STATE, "nmgp_had_subjects_traj_begin must be called first (on the current set)");
    return 0;
}

// ---- device-resident Adam of the cohort (drivers._HadamardCohortLoop with device_resident=True) --------------------------------------
// nmgp_svc_batch_adam_step's loop on the padded rows of a subject set, many iterations per call: parameters and moments stay in HBM,
// an iteration is the chunked evaluation and, per chunk, a status kernel and the masked update on the chunk's own gradient rows in
// the slab (no gradient leaves it).  The arithmetic is drivers.LockStepMAP.step's, operation for operation, so both give the same bits.

// After a chunk's evaluation, for chunk row z (the pointers are the chunk's): alive[z] &= the evaluation is defined -- the
// factorisation's status, a real slot of the parameters that went non-finite, a non-finite value: the three tests of
// cohm_chunk_epilogue / drivers.valid_rows -- then the chain's WIDTH values, or NaN (the host's std::nan("") bits) if it is not alive,
// into its row of the history.
__global__ void k_hadc_adam_status(const int* __restrict__ info, const double* __restrict__ scal, const int* __restrict__ qbad,
                                   int* __restrict__ alive, double* __restrict__ hist, int W, int B) {
    const int z = blockIdx.x * blockDim.x + threadIdx.x;
    if (z >= B) return;
    const double v0 = scal[(size_t)z * 16 + 8], v1 = scal[(size_t)z * 16 + 9];
    const int a = (alive[z] != 0 && info[z] == 0 && qbad[z] == 0 && isfinite(v0) && isfinite(v1)) ? 1 : 0;
    alive[z] = a;
    const double nan_ = __longlong_as_double(0x7ff8000000000000LL);
    for (int t = 0; t < W; ++t) hist[(size_t)z * W + t] = a ? scal[(size_t)z * 16 + 8 + t] : nan_;
}

// Chunk rows z0 + blockIdx.y, subject z / cps of the chunk's nobs table: k_adam_step's update, statement for statement (the build has
// no contraction), on the real slots of the alive chains.  Padded slots of par, m and v are neither read nor written.  An updated real
// slot that is not finite raises the chain's qbad flag (the NMGP_NUM_NAN test of the next evaluation, as the drift kernel does it).
template <class Model>
__global__ __launch_bounds__(256) void k_hadc_adam_step(double* __restrict__ par, const double* __restrict__ g, double* __restrict__ m,
                                                         double* __restrict__ v, const int* __restrict__ alive, int* __restrict__ qbad,
                                                         const int* __restrict__ nobs, int cps, int z0, double b1, double omb1,
                                                         double b2, double omb2, double bc2s, double eps, double step, int N, int T,
                                                         long long P) {
    const int z = z0 + blockIdx.y;
    if (!alive[z]) return;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= P || !Model::real_slot(i, N, nobs[z / cps], T)) return;
    const size_t o = (size_t)z * P + i;
    const double gv = g[o];
    const double t1 = m[o] * b1, t2 = omb1 * gv;
    const double mn = t1 + t2;
    const double t3 = v[o] * b2, t4 = omb2 * gv;
    const double t5 = t4 * gv;
    const double vn = t3 + t5;
    const double t6 = sqrt(vn) / bc2s;
    const double denom = t6 + eps;
    const double t7 = mn / denom;
    const double t8 = step * t7;
    const double pn = par[o] - t8;
    par[o] = pn;
    m[o] = mn;
    v[o] = vn;
    if (!isfinite(pn)) qbad[z] = 1;          // (every writer stores the same word)
}

inline int* ha_alive(nmgp_ctx* c) { return c->ha_flags; }
inline int* ha_qbad(nmgp_ctx* c) { return c->ha_flags + c->ha_B; }

// An API-level failure inside an optimiser call ends the run: the parameters go back to where the call found them (the last completed
// call's), get_pars still answers, and the next adam demands a fresh begin.  The first failure's message is kept.
int cohm_adam_abort(nmgp_ctx* c, int rc) {
    const std::string msg = c->err;
    hipMemcpyAsync(c->ha_q, c->ha_q0, (size_t)c->ha_B * c->ha_P * sizeof(double), hipMemcpyDeviceToDevice, c->stream);
    hipStreamSynchronize(c->stream);
    (void)hipGetLastError();
    c->ha_ended = true;
    c->err = msg;
    return rc;
}

template <class Model>
int cohm_subjects_adam_begin(nmgp_ctx* c, int model, const double* pars, int B, int cps, const double* hyper, int prior) {
    const int N = c->hc_Nmax, T = c->hc_T;
    const size_t P = Model::P(N, T), n = (size_t)B * P;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    nmgp_had_adam_free(c);
    auto fail = [c](int r) {
        const std::string msg = c->err;
        nmgp_had_adam_free(c);
        c->err = msg;
        return r;
    };
    double** bufs[] = {&c->ha_q, &c->ha_q0, &c->ha_m, &c->ha_v};
    for (double** b : bufs)
        if (int r = nmgp_dev_alloc(c, b, n)) return fail(r);
    if (hipMalloc((void**)&c->ha_flags, 2 * (size_t)B * sizeof(int)) != hipSuccess)
        return fail(nmgp_fail(c, NMGP_E_NOMEM, "hipMalloc of the optimiser's flags failed"));
    // [alive = 1 | qbad = a real slot of the start point is not finite]
    std::vector<int> flags(2 * (size_t)B, 1);
    for (int z = 0; z < B; ++z)
        flags[(size_t)B + z] = Model::finite_in(pars + (size_t)z * P, (size_t)N, (size_t)c->hc_nobs_h[z / cps], T) ? 0 : 1;
    hipStream_t s = c->stream;
    bool ok = hipMemcpyAsync(c->ha_q, pars, n * sizeof(double), hipMemcpyHostToDevice, s) == hipSuccess &&
              hipMemsetAsync(c->ha_m, 0, n * sizeof(double), s) == hipSuccess &&
              hipMemsetAsync(c->ha_v, 0, n * sizeof(double), s) == hipSuccess &&
              hipMemcpyAsync(c->ha_flags, flags.data(), flags.size() * sizeof(int), hipMemcpyHostToDevice, s) == hipSuccess &&
              hipStreamSynchronize(s) == hipSuccess;          // the sources are the caller's and this frame's
    if (!ok) return fail(nmgp_fail(c, NMGP_E_HIP, "upload of the optimiser's start state failed (%s)", hipGetErrorString(hipGetLastError())));
    c->ha_model = model;
    c->ha_B = B;
    c->ha_cps = cps;
    c->ha_prior = prior;
    c->ha_P = P;
    c->ha_t = 0;
    c->ha_ended = false;
    std::copy(hyper, hyper + (model == 0 ? 8 : model == 1 ? 9 : 5), c->ha_hyper);
    return 0;
}

// niters iterations from the resident state: per iteration one chunked evaluation with the status kernel and the masked update behind
// every chunk, ONE synchronisation at the end however many chunks the set needs.  The bias corrections are the host's, from the
// running t, exactly as nmgp_svc_batch_adam_step computes them.
template <class Model>
int cohm_subjects_adam(nmgp_ctx* c, int niters, double lr, double beta1, double beta2, double eps, double* out_hist, int* alive) {
    constexpr int W = Model::WIDTH;
    const int B = c->ha_B, N = c->hc_Nmax, T = c->hc_T;
    const long long P = (long long)c->ha_P;
    const size_t nh = (size_t)niters * B * W;
    hipStream_t s = c->stream;
    if (c->ha_hist_cap < nh) {               // before anything of the state is touched: a refusal here leaves the run as it is
        HIP_TRY(c, hipStreamSynchronize(s));
        if (c->ha_hist) hipFree(c->ha_hist);
        c->ha_hist = nullptr;
        c->ha_hist_cap = 0;
        NMGP_TRY(nmgp_dev_alloc(c, &c->ha_hist, nh));
        c->ha_hist_cap = nh;
    }
    HIP_TRY(c, hipMemcpyAsync(c->ha_q0, c->ha_q, (size_t)B * P * sizeof(double), hipMemcpyDeviceToDevice, s));
    for (int it = 0; it < niters; ++it) {
        const long long t = ++c->ha_t;
        const double bc1 = 1.0 - std::pow(beta1, (double)t);
        const double bc2s = std::sqrt(1.0 - std::pow(beta2, (double)t));
        const double step = lr / bc1;
        double* hist = c->ha_hist + (size_t)it * B * W;
        const int rc = cohm_resident_eval<Model>(c, c->ha_q, B, c->ha_cps, c->ha_hyper, c->ha_prior,
                                                 [&](int b0, int nb, int s0, int ccps, const HadLayout& L, double* slab) {
            NMGP_LAUNCH(k_hadc_adam_status, dim3(cdiv(nb, 64)), dim3(64), 0, s, reinterpret_cast<const int*>(slab + L.o_info),
                        slab + L.o_scal, ha_qbad(c) + b0, ha_alive(c) + b0, hist + (size_t)b0 * W, W, nb);
            for (int z0 = 0; z0 < nb; z0 += 65535) {          // the row is a grid dimension
                const int nz = std::min(65535, nb - z0);
                NMGP_LAUNCH((k_hadc_adam_step<Model>), dim3((unsigned)((P + 255) / 256), nz), dim3(256), 0, s, c->ha_q + (size_t)b0 * P,
                            slab + L.o_grad, c->ha_m + (size_t)b0 * P, c->ha_v + (size_t)b0 * P, ha_alive(c) + b0, ha_qbad(c) + b0,
                            c->hc_nobs + s0, ccps, z0, beta1, 1.0 - beta1, beta2, 1.0 - beta2, bc2s, eps, step, N, T, P);
            }
            return 0;
        });
        if (rc) return cohm_adam_abort(c, rc);
    }
    hipError_t e = hipMemcpyAsync(out_hist, c->ha_hist, nh * sizeof(double), hipMemcpyDeviceToHost, s);       // the history, in one copy
    if (e == hipSuccess) e = hipMemcpyAsync(alive, ha_alive(c), (size_t)B * sizeof(int), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);          // the one synchronisation of the call
    if (e != hipSuccess)
        return cohm_adam_abort(c, nmgp_fail(c, NMGP_E_HIP, "the end of the optimiser call failed: %s", hipGetErrorString(e)));
    if (int rc = nmgp_take_launch_error(c)) return cohm_adam_abort(c, rc);
    return 0;
}

// the begun optimiser, or the refusal
int cohm_adam_require(nmgp_ctx* c) {
    if (c->hc_S <= 0) return nmgp_fail(c, NMGP_E_STATE, "nmgp_had_set_subjects must be called first");
    if (c->ha_model < 0) return nmgp_fail(c, NMGP_E_STATE, "nmgp_had_subjects_adam_begin must be called first (on the current set)");
    return 0;
}

#define COHM_MODEL_SWITCH(model, CALL)                \
    do {                                              \
        switch (model) {                              \
            case 0: { using MODEL = CohNon; return CALL; } \
            case 1: { using MODEL = CohSep; return CALL; } \
            default: { using MODEL = CohSta; return CALL; } \
        }                                             \
    } while (0)

// the width of a model's verbose tuple
int cohm_width(int model) { COHM_MODEL_SWITCH(model, MODEL::WIDTH); }

}  // namespace

// what the prediction entries (nmgp_predsample_had_cohort.hip) share with the evaluations: the separable model's masked unpacking and
// the stationary model's masked covariance
void nmgp_hadcs_prep(hipStream_t s, const double* pars, const int* indx, const int* nobs, int cps, int N, int M, int T, double* ell,
                     double* sig, double* Rv, int batch) {
    NMGP_LAUNCH(k_hadcs_prep, dim3(cdiv(N, 256), batch), dim3(256), 0, s, pars, indx, nobs, cps, N, M, T, ell, sig, Rv);
}
int nmgp_hadcst_cov_build(hipStream_t s, const double* x, const int* indx, const double* pars, long long P, const int* nobs, int cps,
                          double* S, int ld, int N, int M, int batch, long long sstride) {
    const dim3 grid(cdiv(N, 64), cdiv(N, 64), batch);
    NMGP_HADS_SWITCH(M, NMGP_LAUNCH((k_hadcst_cov<MM>), grid, dim3(256), 0, s, x, indx, pars, P, nobs, cps, S, ld, N, sstride));
    return 0;
}

extern "C" int nmgp_had_subjects_eval(nmgp_ctx* c, const double* pars, int B, int chains_per_subject, const double hyper[8], int prior,
                                      double* out5, double* grad, int* status) {
    return cohm_subjects_eval<CohNon>(c, pars, B, chains_per_subject, hyper, prior, out5, grad, status);
}

extern "C" int nmgp_hads_subjects_eval(nmgp_ctx* c, const double* pars, int B, int chains_per_subject, const double hyper[9], int prior,
                                       double* out6, double* grad, int* status) {
    return cohm_subjects_eval<CohSep>(c, pars, B, chains_per_subject, hyper, prior, out6, grad, status);
}

extern "C" int nmgp_hadst_subjects_eval(nmgp_ctx* c, const double* pars, int B, int chains_per_subject, const double hyper[5], int prior,
                                        double* out5, double* grad, int* status) {
    return cohm_subjects_eval<CohSta>(c, pars, B, chains_per_subject, hyper, prior, out5, grad, status);
}

// ---- the trajectory family (see include/nmgp.h) ---------------------------------------------------------------------------------------
void nmgp_had_traj_free(nmgp_ctx* c) {
    double** bufs[] = {&c->ht_q, &c->ht_p, &c->ht_g, &c->ht_q0, &c->ht_g0, &c->ht_minv, &c->ht_U, &c->ht_kin, &c->ht_eps};
    for (double** b : bufs) {
        if (*b) hipFree(*b);
        *b = nullptr;
    }
    if (c->ht_flags) hipFree(c->ht_flags);
    c->ht_flags = nullptr;
    c->ht_model = -1;
    c->ht_B = c->ht_cps = c->ht_prior = c->ht_mass = 0;
    c->ht_P = 0;
}

extern "C" int nmgp_had_subjects_traj_begin(nmgp_ctx* c, int model, const double* pars, int B, int chains_per_subject,
                                            const double* hyper, int prior, double* out, int* status) {
    if (!c) return NMGP_E_NULL;
    if (model < 0 || model > 2) return nmgp_fail(c, NMGP_E_SHAPE, "model = %d must be 0 (nonseparable), 1 (separable) or 2 (stationary)", model);
    // (NULL arguments, the set, the factorisation and B = S * chains_per_subject: the evaluation entry's own refusals)
    COHM_MODEL_SWITCH(model, cohm_subjects_traj_begin<MODEL>(c, model, pars, B, chains_per_subject, hyper, prior, out, status));
}

extern "C" int nmgp_had_subjects_traj_set_mass(nmgp_ctx* c, int kind, const double* minv) {
    if (!c) return NMGP_E_NULL;
    NMGP_TRY(cohm_traj_require(c));
    if (kind < 0 || kind > 2)
        return nmgp_fail(c, NMGP_E_SHAPE, "mass matrix kind must be 0 (identity), 1 (diagonal per chain row) or 2 (prior-factor metric)");
    if (kind == 1 && !minv) return nmgp_fail(c, NMGP_E_NULL, "minv must not be NULL");
    HIP_TRY(c, hipSetDevice(c->device));
    COHM_MODEL_SWITCH(c->ht_model, cohm_subjects_traj_set_mass<MODEL>(c, kind, minv));
}

// out = op(L_blk,s) in for the B padded rows of the set (mode 0 of k_prior_trmm_coh): see include/nmgp.h
extern "C" int nmgp_had_subjects_prior_apply(nmgp_ctx* c, int model, const double* hyper, int trans, const double* in, int B,
                                             int chains_per_subject, double* out) {
    if (!c) return NMGP_E_NULL;
    if (!hyper || !in || !out) return nmgp_fail(c, NMGP_E_NULL, "hyper/in/out must not be NULL");
    if (c->hc_S <= 0) return nmgp_fail(c, NMGP_E_STATE, "nmgp_had_set_subjects must be called first");
    if (model < 0 || model > 2) return nmgp_fail(c, NMGP_E_SHAPE, "model = %d must be 0 (nonseparable), 1 (separable) or 2 (stationary)", model);
    if (model == NMGP_HAD_MODEL_STA) return nmgp_fail(c, NMGP_E_UNSUPPORTED, "the stationary model has no GP prior: no prior factors to apply");
    if (c->chol_algo != 1)
        return nmgp_fail(c, NMGP_E_UNSUPPORTED, "the Hadamard entries run on the custom factorisation only (riding rows)");
    if (chains_per_subject < 1 || (long long)B != (long long)c->hc_S * chains_per_subject)
        return nmgp_fail(c, NMGP_E_SHAPE, "B = %d must be %d subjects x chains_per_subject = %d", B, c->hc_S, chains_per_subject);
    HIP_TRY(c, hipSetDevice(c->device));
    const int N = c->hc_Nmax, T = c->hc_T;
    const size_t P = model == 0 ? CohNon::P(N, T) : CohSep::P(N, T), n = (size_t)B * P;
    PriorFactor *p0 = nullptr, *p1 = nullptr;
    NMGP_TRY(nmgp_hadc_priors(c, hyper, &p0, &p1));
    double *din = nullptr, *dout = nullptr;
    NMGP_TRY(nmgp_scratch_get(c, 3, n, &din));
    NMGP_TRY(nmgp_scratch_get(c, 4, n, &dout));
    HIP_TRY(c, hipMemcpyAsync(din, in, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    prior_trmm_cohort(c->stream, model, trans != 0, p0->L, p0->ld, (long long)p0->ld * N, p1->L, p1->ld, (long long)p1->ld * N, din, dout,
                      c->hc_nobs, nullptr, chains_per_subject, N, T, (long long)P, B, 1.0, 0, nullptr, nullptr, 1,
                      model == 1 ? (double)(float)hyper[8] : 1.0);
    HIP_TRY(c, hipMemcpyAsync(out, dout, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return nmgp_take_launch_error(c);
}

extern "C" int nmgp_had_subjects_traj(nmgp_ctx* c, const double* eps, int nsteps, const double* p0, double* q1, double* p1,
                                      double* kin1, double* U1, int* failed) {
    if (!c) return NMGP_E_NULL;
    if (!eps || !p0 || !q1 || !U1 || !failed) return nmgp_fail(c, NMGP_E_NULL, "eps/p0/q1/U1/failed must not be NULL");
    NMGP_TRY(cohm_traj_require(c));
    if (nsteps < 1) return nmgp_fail(c, NMGP_E_SHAPE, "nsteps = %d must be positive", nsteps);
    for (int s = 0; s < c->hc_S; ++s)
        if (!(eps[s] > 0.0) || !std::isfinite(eps[s]))
            return nmgp_fail(c, NMGP_E_SHAPE, "eps[%d] = %g: every subject's step size must be finite and positive", s, eps[s]);
    HIP_TRY(c, hipSetDevice(c->device));
    COHM_MODEL_SWITCH(c->ht_model, cohm_subjects_traj<MODEL>(c, eps, nsteps, p0, q1, p1, kin1, U1, failed));
}

extern "C" int nmgp_had_subjects_traj_commit(nmgp_ctx* c, const int* accept) {
    if (!c) return NMGP_E_NULL;
    if (!accept) return nmgp_fail(c, NMGP_E_NULL, "accept must not be NULL");
    NMGP_TRY(cohm_traj_require(c));
    HIP_TRY(c, hipSetDevice(c->device));
    COHM_MODEL_SWITCH(c->ht_model, cohm_subjects_traj_commit<MODEL>(c, accept));
}

extern "C" int nmgp_had_subjects_traj_end(nmgp_ctx* c) {
    if (!c) return NMGP_E_NULL;
    if (c->ht_model < 0) return 0;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    nmgp_had_traj_free(c);
    return 0;
}

// ---- the optimiser family (see include/nmgp.h) ----------------------------------------------------------------------------------------
void nmgp_had_adam_free(nmgp_ctx* c) {
    double** bufs[] = {&c->ha_q, &c->ha_q0, &c->ha_m, &c->ha_v, &c->ha_hist};
    for (double** b : bufs) {
        if (*b) hipFree(*b);
        *b = nullptr;
    }
    if (c->ha_flags) hipFree(c->ha_flags);
    c->ha_flags = nullptr;
    c->ha_model = -1;
    c->ha_B = c->ha_cps = c->ha_prior = 0;
    c->ha_P = c->ha_hist_cap = 0;
    c->ha_t = 0;
    c->ha_ended = false;
}

extern "C" int nmgp_had_subjects_adam_begin(nmgp_ctx* c, int model, const double* pars, int B, int chains_per_subject,
                                            const double* hyper, int prior) {
    if (!c) return NMGP_E_NULL;
    if (!pars || !hyper) return nmgp_fail(c, NMGP_E_NULL, "pars/hyper must not be NULL");
    if (model < 0 || model > 2) return nmgp_fail(c, NMGP_E_SHAPE, "model = %d must be 0 (nonseparable), 1 (separable) or 2 (stationary)", model);
    if (c->hc_S <= 0) return nmgp_fail(c, NMGP_E_STATE, "nmgp_had_set_subjects must be called first");
    if (c->chol_algo != 1)
        return nmgp_fail(c, NMGP_E_UNSUPPORTED, "the Hadamard entries run on the custom factorisation only (riding rows)");
    if (chains_per_subject < 1 || (long long)B != (long long)c->hc_S * chains_per_subject)
        return nmgp_fail(c, NMGP_E_SHAPE, "B = %d must be %d subjects x chains_per_subject = %d", B, c->hc_S, chains_per_subject);
    HIP_TRY(c, hipSetDevice(c->device));
    COHM_MODEL_SWITCH(model, cohm_subjects_adam_begin<MODEL>(c, model, pars, B, chains_per_subject, hyper, prior));
}

extern "C" int nmgp_had_subjects_adam(nmgp_ctx* c, int niters, double lr, double beta1, double beta2, double eps, double* out_hist,
                                      int* alive) {
    if (!c) return NMGP_E_NULL;
    NMGP_TRY(cohm_adam_require(c));          // the state first: a caller that knows of no run hands over no buffers
    if (!out_hist || !alive) return nmgp_fail(c, NMGP_E_NULL, "out_hist/alive must not be NULL");
    if (c->ha_ended)
        return nmgp_fail(c, NMGP_E_STATE, "an earlier nmgp_had_subjects_adam failed and ended the run: nmgp_had_subjects_adam_begin must be called again");
    if (niters < 1) return nmgp_fail(c, NMGP_E_SHAPE, "niters = %d must be positive", niters);
    const int W = cohm_width(c->ha_model);
    if ((long long)niters * c->ha_B * W > (long long)NMGP_HAD_ADAM_HIST_MAX)
        return nmgp_fail(c, NMGP_E_SHAPE, "a history of niters = %d x B = %d x %d values is above NMGP_HAD_ADAM_HIST_MAX = %lld: ask for fewer "
                         "iterations per call", niters, c->ha_B, W, (long long)NMGP_HAD_ADAM_HIST_MAX);
    HIP_TRY(c, hipSetDevice(c->device));
    COHM_MODEL_SWITCH(c->ha_model, cohm_subjects_adam<MODEL>(c, niters, lr, beta1, beta2, eps, out_hist, alive));
}

extern "C" int nmgp_had_subjects_adam_get_pars(nmgp_ctx* c, double* pars) {
    if (!c) return NMGP_E_NULL;
    NMGP_TRY(cohm_adam_require(c));          // (the state first, as in nmgp_had_subjects_adam)
    if (!pars) return nmgp_fail(c, NMGP_E_NULL, "pars must not be NULL");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(pars, c->ha_q, (size_t)c->ha_B * c->ha_P * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int nmgp_had_subjects_adam_end(nmgp_ctx* c) {
    if (!c) return NMGP_E_NULL;
    if (c->ha_model < 0) return 0;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    nmgp_had_adam_free(c);
    return 0;
}
