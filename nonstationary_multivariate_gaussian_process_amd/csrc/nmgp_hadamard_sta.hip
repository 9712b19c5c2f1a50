// Hadamard form of the stationary model (the LMC baseline): irregularly observed outputs, ONE cross-output matrix and a stationary
// RBF kernel (logpos.py:662-716, prediction.py:1695-1740).
//
// The subject is the Hadamard one (nmgp_had_set_data: N single observations (x_i, c_i, y_i)).  The parameter vector is
// [tilde_l, tilde_sigma, L_vec (T), tilde_sigma2_err], P = T + 3 (vec2pars_S).  L = vec2lowtriangle(L_vec) is taken as it is (no exp on
// the diagonal slots), B_f = L L^T, r_i = row c_i of L.  With l = exp(tilde_l), s2 = exp(tilde_sigma)^2, u = x / l
//   S[i, j] = B_f[c_i, c_j] (s2 exp(-d_ij / 2) + 1e-6 d_ij) + sigma2_err d_ij,   d_ij = u_i^2 + u_j^2 - 2 u_i u_j   (kernels.py:20-43)
// one dense N x N SPD matrix per evaluation: the jitter is multiplied by B_f[c_i, c_i].  Priors: Normal(mu, sd) on tilde_l, Normal(0, c)
// on every raw L_vec slot, the unnormalised inverse gamma on sigma2_err; none on tilde_sigma.  There is no GP prior: neither the cached
// prior factors nor the prior stream are touched.  The factorisation with its riding rows, the triangular matrix-vector product, the
// inverse SYRK and the trace terms are the library's, and the schedule of a batched evaluation is nmgp_hadamard_common.h's, shared
// with the other two Hadamard models; this file adds the model's kernels and its hooks into that schedule (HadSta) and into the
// prediction schedule of nmgp_predsample_common.h (PsHadSt).
// A draw of the posterior is just another parameter vector (no latent curve to regress), so ONE predictor serves the MAP and a
// chain of draws.  Layout conventions of the Gibbs kernels: a 64 x 64 tile of observations per 256-thread workgroup, lanes along i,
// the j side in LDS, blockIdx.z = chain; fixed summation order and no atomics, so B chains in one launch give the bits of B launches.
#include "nmgp_hadamard_common.h"
#include "nmgp_predsample_common.h"

#include <algorithm>

using namespace nmgpk;

namespace {

inline unsigned cdiv(long long a, long long b) { return (unsigned)((a + b - 1) / b); }

// (hadst_bf<M> and hadst_stage<M>, the chain's scalars and the j side of a tile, are in nmgp_hadamard_common.h: the cohort's
// kernels stage the same way)

// S[i, j] = B_f[c_i, c_j] (s2 exp(-d_ij / 2) + jitter d_ij) + sigma2_err d_ij, lower triangle, column-major with leading dimension ld
template <int M>
__global__ __launch_bounds__(256) void k_hadst_cov(const double* __restrict__ x, const int* __restrict__ indx,
                                                    const double* __restrict__ pars, long long P, double* __restrict__ S, int ld,
                                                    int N, long long sstride) {
    constexpr int TJ = 64;
    __shared__ double su[TJ], sB[M * M], sp[3];
    __shared__ int sc[TJ];
    const int I = blockIdx.x, J = blockIdx.y;
    if (I < J) return;
    pars += (size_t)blockIdx.z * P;
    S += (size_t)blockIdx.z * sstride;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int j0 = J * TJ;
    hadst_stage<M>(pars, P, x, indx, N, j0, sp, sB, su, sc);
    __syncthreads();
    const int i = I * 64 + lane;
    if (i >= N) return;
    const double s2 = sp[1], s2e = sp[2];
    const double ui = x[i] / sp[0];
    const double ui2 = ui * ui;
    const double* bi = sB + indx[i] * M;
#pragma unroll 2
    for (int jj = 0; jj < TJ / 4; ++jj) {
        const int k = w * (TJ / 4) + jj;
        const int j = j0 + k;
        if (j >= N) break;
        if (i < j) continue;
        const double uj = su[k];
        const double dist = (ui2 + uj * uj) - 2.0 * (ui * uj);          // kernels.py:20
        double kv = exp(-0.5 * dist) * s2;                              // kernels.py:42
        if (i == j) kv = NMGP_JITTER + kv;                              // kernels.py:35
        double v = kv * bi[sc[k]];
        if (i == j) v += s2e;
        S[(size_t)j * ld + i] = v;
    }
}

// Adjoint of the likelihood, one pass over the FULL symmetric -S^-1 (what the inverse SYRK leaves):
//   G = 1/2 (alpha alpha^T - S^-1),  e_ij = s2 exp(-d_ij / 2)
//   a_l[i]  = sum_j G_ij B_f[c_i, c_j] e_ij d_ij          (summed over i: d loglik / d tilde_l)
//   a_s[i]  = sum_j G_ij B_f[c_i, c_j] e_ij               (twice its sum: d loglik / d tilde_sigma)
//   w_i[m]  = sum_j G_ij (e_ij + jitter d_ij) r_j[m]      (twice its sum over {i : c_i = c}: d loglik / d L[c, m])
// Each wave takes 16 j; the four waves' sums meet in LDS in a fixed order and leave part[t][J][i] (component t: 0 = a_l, 1 = a_s,
// 2 + m = w[m]; component-major, so that the stores here and the loads of k_hadst_grad_final run along i).
template <int M>
__global__ __launch_bounds__(256) void k_hadst_adjoint(const double* __restrict__ x, const int* __restrict__ indx,
                                                        const double* __restrict__ pars, long long P,
                                                        const double* __restrict__ alpha, const double* __restrict__ Sneg, int ld,
                                                        int N, double* __restrict__ part, long long pstride) {
    constexpr int TJ = 64;
    __shared__ double su[TJ], sB[M * M], sp[3], sR[TJ * M], sa[TJ];
    __shared__ int sc[TJ];
    __shared__ double red[2][4][64];
    const int I = blockIdx.x, J = blockIdx.y, NJ = gridDim.y;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int j0 = J * TJ;
    const size_t Ns = (size_t)N;
    {   // blockIdx.z = chain
        const size_t z = blockIdx.z;
        pars += z * (size_t)P;
        alpha += z * Ns;
        Sneg += z * (size_t)ld * Ns;
        part += z * (size_t)pstride;
    }
    hadst_stage<M>(pars, P, x, indx, N, j0, sp, sB, su, sc);
    if (tid < TJ) sa[tid] = (j0 + tid < N) ? alpha[j0 + tid] : 0.0;
    for (int k = tid; k < TJ * M; k += 256) {           // r_j = row c_j of L, zero-padded to M
        const int j = j0 + k / M, m = k % M;
        const int cj = (j < N) ? indx[j] : 0;
        sR[k] = (j < N && m <= cj) ? pars[2 + cj * (cj + 1) / 2 + m] : 0.0;
    }
    __syncthreads();
    const int i = I * 64 + lane;
    const bool iv = i < N;
    const int ic = iv ? i : N - 1;
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
            if (j >= N) break;
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
        if (w == 0 && iv)
            part[((size_t)t * NJ + J) * Ns + i] =
                (red[t & 1][0][lane] + red[t & 1][1][lane]) + (red[t & 1][2][lane] + red[t & 1][3][lane]);
    }
}

// Final gradient: one workgroup per (output slot t = blockIdx.x, chain = blockIdx.y).  Thread k walks the observations k, k + 256, ...
// in index order, adds each one's NJ partials in order (for an L slot (c, m): of the observations with label c only), then the fixed
// tree over the 256 threads.  No order depends on the batch.  Slot T + 2 is sigma2_err d loglik / d sigma2_err = sigma2_err tr G with
// tr = {sum alpha^2, trace S^-1} (k_trace_terms).  Priors: Normal(mu, sd) on tilde_l, Normal(0, c) on the L slots (d lp / d v =
// -(v - mean) / var), the inverse gamma + Jacobian on tilde_sigma2_err (distributions.py:116-124); none on tilde_sigma.
__global__ __launch_bounds__(256) void k_hadst_grad_final(const double* __restrict__ part, long long pstride, int NJ, int N, int M,
                                                           int T, const int* __restrict__ indx, const double* __restrict__ pars,
                                                           const double* __restrict__ tr, double mu_l, double var_l, double var_c,
                                                           double a, double b, int prior, double* __restrict__ grad) {
    __shared__ double sh[256];
    const int t = blockIdx.x, P = T + 3;
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
    for (int i = threadIdx.x; i < N; i += 256) {
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

// Scalar epilogue (logpos.py:692-716): Normal(mu, sd).log_prob with the float32-rounded mean, variance and log sd that torch uses for
// Python-number arguments (computed by the host as normal_logprob_f32 of nmgp_eig.hip does); loglik drops the 2 pi term
// (distributions.multivariate_normal_logpdf); the three prior entries are reported whether or not `prior` adds them.
__global__ void k_hadst_finalize(const double* __restrict__ scal, const double* __restrict__ pars, int T, double mu_l, double var_l,
                                 double log_sd_l, double var_c, double log_sd_c, double a, double b, int prior,
                                 double* __restrict__ out5) {
    if (threadIdx.x != 0) return;
    const int P = T + 3;
    scal += (size_t)blockIdx.x * 16;             // blockIdx.x = chain: [0] log det, [1] quadratic form, [8..12] the verbose tuple
    out5 += (size_t)blockIdx.x * 16;
    pars += (size_t)blockIdx.x * P;
    const double LOGSQRT2PI = log(sqrt(2.0 * M_PI));
    const double tse = pars[P - 1];
    const double sigma2 = exp(tse);
    const double loglik = -0.5 * scal[0] - 0.5 * scal[1];
    const double r = pars[0] - mu_l;
    const double lp_l = -(r * r) / (2.0 * var_l) - log_sd_l - LOGSQRT2PI;
    double lp_L = 0.0;
    for (int t = 0; t < T; ++t) {
        const double v = pars[2 + t];
        lp_L += -(v * v) / (2.0 * var_c) - log_sd_c - LOGSQRT2PI;
    }
    const double lp_s2 = (-a - 1.0) * log(sigma2) - b / sigma2;
    double res = 0.0;
    res += loglik;
    if (prior) {
        res += lp_l;
        res += lp_L;
        res += lp_s2;
        res += tse;
    }
    out5[0] = -res;
    out5[1] = loglik;
    out5[2] = lp_l;
    out5[3] = lp_L;
    out5[4] = lp_s2;
}

// Cross-covariances k_f[i, e] = B_f[m, c_i] s2 exp(-d(x_i, x*_s) / 2) (prediction.py:1711-1715; no jitter) of the new inputs s0 .. of
// draw h = blockIdx.z, written as riding rows R0 + e below the covariance: the factorisation turns each into (L_S^-1 k_f[:, e])^T.
// Observation i = blockIdx.x; lanes along the riding-row index (contiguous in a column).
//   istar == nullptr: e = (s - s0) M + m;  else e = s - s0, m = istar[s]
template <int M>
__global__ __launch_bounds__(256) void k_hadst_cross_rows(const double* __restrict__ x, const int* __restrict__ indx,
                                                           const double* __restrict__ pars, long long P, int N,
                                                           const double* __restrict__ xs, const int* __restrict__ istar, int s0,
                                                           int E, double* __restrict__ A, int ld, long long bstride, int R0) {
    __shared__ double sBc[M], sp[3];
    const int i = blockIdx.x, h = blockIdx.z;
    pars += (size_t)h * P;
    if (threadIdx.x == 0) {
        const double sg = exp(pars[1]);
        sp[0] = exp(pars[0]);
        sp[1] = sg * sg;
    } else if (threadIdx.x - 64 < (unsigned)M) {
        sBc[threadIdx.x - 64] = hadst_bf<M>(pars + 2, threadIdx.x - 64, indx[i]);     // B_f[m, c_i]
    }
    __syncthreads();
    const int e = blockIdx.y * 256 + threadIdx.x;
    if (e >= E) return;
    const int s = istar ? s0 + e : s0 + e / M;
    const int mp = istar ? istar[s] : e % M;
    const double ui = x[i] / sp[0], uj = xs[s] / sp[0];
    const double dist = (ui * ui + uj * uj) - 2.0 * (ui * uj);
    A[(size_t)h * bstride + (size_t)i * ld + R0 + e] = sBc[mp] * (exp(-0.5 * dist) * sp[1]);
}

// var = B_f[m, m] (jitter + s2) - |L_S^-1 k_f|^2 + sigma2_err, a value <= 0 replaced by settings.precision (prediction.py:1719-1726:
// the prior term is B_f kron RBF_cov(x*), which carries the jitter).  Draw h = blockIdx.y; O = S M outputs per draw (k = s M + m), or
// O = S in the indexed form (k = s, m = istar[s]).
__global__ void k_hadst_predvar(const double* __restrict__ pars, long long P, const double* __restrict__ colsq,
                                const int* __restrict__ istar, int S, int M, double* __restrict__ var) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x, h = blockIdx.y;
    const int O = istar ? S : S * M;
    if (k >= O) return;
    const int mp = istar ? istar[k] : k % M;
    pars += (size_t)h * P;
    double b = 0.0;
    for (int r = 0; r <= mp; ++r) {
        const double v = pars[2 + mp * (mp + 1) / 2 + r];
        b += v * v;
    }
    const double sg = exp(pars[1]);
    const double kss = NMGP_JITTER + sg * sg;
    double v = (b * kss - colsq[(size_t)h * O + k]) + exp(pars[P - 1]);
    if (v <= 0.0) v = NMGP_PRECISION;
    var[(size_t)h * O + k] = v;
}

int hadst_cov_build(hipStream_t s, const double* x, const int* indx, const double* pars, long long P, double* S, int ld, int N, int M,
                    int batch, long long sstride) {
    const dim3 grid(cdiv(N, 64), cdiv(N, 64), batch);
    NMGP_HADS_SWITCH(M, NMGP_LAUNCH((k_hadst_cov<MM>), grid, dim3(256), 0, s, x, indx, pars, P, S, ld, N, sstride));
    return 0;
}

int hadst_adjoint(hipStream_t s, const double* x, const int* indx, const double* pars, long long P, const double* alpha,
                  const double* Sneg, int ld, int N, int M, double* part, long long pstride, int batch) {
    const dim3 grid(cdiv(N, 64), cdiv(N, 64), batch);      // -S^-1 of chain z: ld x N doubles further on
    NMGP_HADS_SWITCH(M, NMGP_LAUNCH((k_hadst_adjoint<MM>), grid, dim3(256), 0, s, x, indx, pars, P, alpha, Sneg, ld, N, part, pstride));
    return 0;
}

// hooks of the stationary model into the shared schedule (nmgp_hadamard_common.h); hyper = {mu_tilde_l, sigma_tilde_l, a, b, c}
struct HadSta {
    static constexpr int WIDTH = 5;
    static constexpr bool GP_PRIORS = false;
    static constexpr const char* NOUN = "stationary Hadamard";
    static size_t P(int, int T) { return (size_t)T + 3; }
    static size_t part_width(int M) { return M + 2; }
    template <class Take>
    static void extras(HadLayout&, Take, size_t, size_t, int, int, bool) {}
    static int build_cov(const HadChunk& k) {
        nmgp_ctx* c = k.c;
        return hadst_cov_build(c->stream, c->d_x, c->had_indx, k.at(k.L.o_P), (long long)P(c->N, c->T), k.at(k.L.o_S), k.L.ld, c->N, c->M,
                               k.B, k.L.bs);
    }
    static int value_epilogue(const HadChunk& k) {
        nmgp_ctx* c = k.c;
        nmgp_hadst_finalize(c->stream, k.at(k.L.o_scal), k.at(k.L.o_P), c->T, k.hyper, k.prior, k.B);
        return 0;
    }
    static int adjoint_grad(const HadChunk& k) {
        nmgp_ctx* c = k.c;
        const int N = c->N, M = c->M, T = c->T;
        const long long P_ = (long long)P(N, T), pstride = (long long)k.L.part_per;
        const NormalF32 nl(k.hyper[0], k.hyper[1]), nc(0.0, k.hyper[4]);
        double *dP = k.at(k.L.o_P), *part = k.at(k.L.o_part);
        NMGP_TRY(hadst_adjoint(c->stream, c->d_x, c->had_indx, dP, P_, k.at(k.L.o_alpha), k.at(k.L.o_Sneg), N, N, M, part, pstride, k.B));
        NMGP_LAUNCH(k_hadst_grad_final, dim3((unsigned)P_, k.B), dim3(256), 0, c->stream, part, pstride, (N + 63) / 64, N, M, T,
                    c->had_indx, dP, k.at(k.L.o_tr), nl.mean, nl.var, nc.var, k.hyper[2], k.hyper[3], k.prior, k.at(k.L.o_grad));
        return 0;
    }
};

// hooks of the stationary model into the shared prediction schedule (nmgp_predsample_common.h): no per-location parameters, so
// nothing to unpack, no latent regression and no workspace of its own
struct PsHadSt : PsHadamard {
    static size_t P(int, int T) { return (size_t)T + 3; }
    static int star_width(int) { return 0; }
    template <class Take>
    static void extras(PsCall&, Take, size_t) {}
    static int prep(const PsCall&) { return 0; }
    static int star(const PsCall&) { return 0; }
    static int build_cov(const PsCall& k) {
        return hadst_cov_build(k.c->stream, k.c->d_x, k.c->had_indx, k.pars, k.P, k.Sb, k.ld, k.N, k.M, k.Bc, k.bs);
    }
    static int cross_rows(const PsCall& k) {
        const dim3 grid(k.N, cdiv(k.E, 256), k.Bc);
        NMGP_HADS_SWITCH(k.M, NMGP_LAUNCH((k_hadst_cross_rows<MM>), grid, dim3(256), 0, k.c->stream, k.c->d_x, k.c->had_indx, k.pars, k.P,
                                          k.N, k.xs, k.is, k.s0, k.E, k.Sb, k.ld, k.bs, k.N + 1));
        return 0;
    }
    static int finish(const PsCall& k) {
        const long long O = (long long)k.S * k.per;
        NMGP_LAUNCH(k_hadst_predvar, dim3(cdiv(O, 256), k.Bc), dim3(256), 0, k.c->stream, k.pars, k.P, k.sqs, k.is, k.S, k.M, k.var);
        return 0;
    }
};

}  // namespace

// the scalar epilogue of `batch` chains (scal: 16 doubles per chain, the tuple into scal[8 ..]); no term depends on N, so the cohort
// entry (nmgp_hadamard_cohort_models.hip) shares it
void nmgp_hadst_finalize(hipStream_t s, double* scal, const double* pars, int T, const double* hyper, int prior, int batch) {
    const NormalF32 nl(hyper[0], hyper[1]), nc(0.0, hyper[4]);
    NMGP_LAUNCH(k_hadst_finalize, dim3(batch), dim3(64), 0, s, scal, pars, T, nl.mean, nl.var, nl.log_sd, nc.var, nc.log_sd, hyper[2],
                hyper[3], prior, scal + 8);
}

// B chains of the resident Hadamard subject under the stationary model: pars [B, T + 3] -> out5 [B, 5] (the verbose tuples), grad
// [B, T + 3] = d NegLog / d pars or NULL, status [B]; see had_batch_eval.  hyper = {mu_tilde_l, sigma_tilde_l, a, b, c}.
extern "C" int nmgp_hadst_batch_eval(nmgp_ctx* c, const double* pars, int B, const double hyper[5], int prior, double* out5,
                                     double* grad, int* status) {
    return had_batch_eval<HadSta>(c, pars, B, hyper, prior, out5, grad, status);
}

// out: [N, N] row-major, the full symmetric S = K_x o B_f[c, c] + sigma2_err I
extern "C" int nmgp_hadst_covariance(nmgp_ctx* c, const double* pars, double* out) { return had_covariance<HadSta>(c, pars, out); }

// Prediction at the new inputs xs [S] under H parameter vectors (H = 1: the MAP predictor; H > 1: posterior draws).  A chunk of B
// draws is ONE batched factorisation of B matrices of order N with y and the slice's cross-covariance rows riding below each.
//   indx_star == NULL: mean, var [H, S, M] (all outputs at every input), slices of max(1, N / M) inputs
//   indx_star given:   mean, var [H, S] (output indx_star[s] at input s), slices of N inputs
// status [H] or NULL as nmgp_hadst_batch_eval reports it; a failing draw has NaN rows and does not fail the call.
extern "C" int nmgp_predict_hadst(nmgp_ctx* c, const double* pars, int H, const double* xs, const int* indx_star, int S, double* mean,
                                  double* var, int* status) {
    return ps_predict<PsHadSt>(c, pars, H, nullptr, xs, indx_star, S, 0, nullptr, nullptr, mean, var, nullptr, status);
}

