// A cohort of Hadamard subjects of RAGGED size per launch sequence: the set (nmgp_had_set_subjects, nmgp_had_clear_subjects), its
// per-subject GP-prior factors, the masked trace, the nonseparable model's own small kernels, and the set's predictor
// nmgp_predsample_had_subjects (second half of the file).  The three evaluation entries, their model hooks and their one chunk
// skeleton are in nmgp_hadamard_cohort_models.hip.
//
// The blocked Cholesky batch wants one matrix order, so every subject of a set is padded to the set's Nmax with decoupled unit
// observations: for a padded i >= N_s, S[i, i] = 1, S[i, j] = S[j, i] = 0, y[i] = 0, and the same in both GP-prior covariances
// (identity block, zero right-hand side).  In IEEE arithmetic, whatever the blocking: the padded part of every factor is the identity
// with exact zeros left of it; log det, z = L^-1 y, alpha, the Mahalanobis terms and the prior log-determinants gain exact zeros; the
// rows of X = L^-T that ride along are identity rows; -S^-1 = -X X^T has -1 on the padded diagonal and 0 elsewhere in the padded rows.
// Three terms do NOT take care of themselves and are masked here: tr S^-1 (it would count one per padded observation), the N log 2 pi
// of the 1 + T prior terms (N_s, not Nmax), and the centred prior right-hand sides (zero in the padded slots).
//
// Everything between the covariance build and the adjoint is the library's own with n = Nmax (set_row, identity_rows, nmgp_potrf with
// precise panels, get_row, chol_logdet_quad, tri_gemv_upper, syrk_lower, col_sumsq, prior_trsv with per-subject factor strides).
// k_gibbs_cov / k_gibbs_adjoint (nmgp_hadamard_common.h) are shared by three models whose bits and register budgets are pinned, so no
// mask is threaded through them; the masked pair k_hadc_cov<M, AMP> / k_hadc_adjoint<M, AMP> stands below them in that header.  Every
// mask comes from the device table of the subjects' sizes (nobs), never from the contents of a padded slot.
//
// Chunks of chains under NMGP_HAD_BATCH_SLAB_GB (had_for_chunks) are aligned to subjects: a chunk is (first subject, chains per
// subject) or a part of ONE subject's chains, so that no kernel takes a chain offset -- the chain z of a chunk belongs to subject
// z / cps of the chunk's slice of the tables.
#include "nmgp_hadamard_common.h"
#include "nmgp_predsample_common.h"

#include <algorithm>

using namespace nmgpk;

namespace {

inline unsigned cdiv(long long a, long long b) { return (unsigned)((a + b - 1) / b); }

__device__ inline double hadc_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// block of up to 1024 threads; result valid in thread 0 (the order of nmgp_kernels.hip's block_sum)
__device__ inline double hadc_block_sum(double v, double* sh /*[16]*/) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    v = hadc_wave_sum(v);
    __syncthreads();
    if (lane == 0) sh[w] = v;
    __syncthreads();
    const int nw = (blockDim.x + 63) >> 6;
    v = ((int)threadIdx.x < nw) ? sh[threadIdx.x] : 0.0;
    if (w == 0) v = hadc_wave_sum(v);
    return v;
}

// Real i: ell = exp(tilde_l), Rv[i, 0..M) = row c_i of L_i, zero-padded (k_had_prep).  Padded i: ell = 1, Rv = 0 -- written, so that
// no later kernel reads what nobody wrote, and without reading the padded parameter slots.  blockIdx.y = chain, subject = chain / cps.
__global__ void k_hadc_prep(const double* __restrict__ pars, const int* __restrict__ indx, const int* __restrict__ nobs, int cps,
                            int N, int M, int T, double* __restrict__ ell, double* __restrict__ Rv) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int sub = blockIdx.y / cps;
    const int Ns = nobs[sub];
    pars += (size_t)blockIdx.y * ((size_t)N * (1 + T) + 1);
    indx += (size_t)sub * N;
    ell += (size_t)blockIdx.y * N;
    Rv += (size_t)blockIdx.y * N * M;
    if (i >= Ns) {
        ell[i] = 1.0;
        for (int m = 0; m < M; ++m) Rv[(size_t)i * M + m] = 0.0;
        return;
    }
    ell[i] = exp(pars[i]);
    const int c = indx[i];
    const double* u = pars + N + (size_t)i * T + c * (c + 1) / 2;
    for (int m = 0; m < M; ++m) Rv[(size_t)i * M + m] = (m <= c) ? u[m] : 0.0;
}

// The masked GP-prior covariance of every subject: RBF(x; alpha, beta) + jitter I on the real observations (the expressions of
// k_cov_sym's RBF branch), delta_ij on the padded ones; lower triangle, blockIdx.z = subject.
__global__ __launch_bounds__(256) void k_hadc_rbf(const double* __restrict__ x, const int* __restrict__ nobs, int N, double alpha,
                                                   double beta, double* __restrict__ out, int ld) {
    constexpr int TJ = 64;
    __shared__ double sx[TJ];
    const int I = blockIdx.x, J = blockIdx.y;
    if (I < J) return;
    const int Ns = nobs[blockIdx.z];
    x += (size_t)blockIdx.z * N;
    out += (size_t)blockIdx.z * ld * N;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int j0 = J * TJ;
    if (tid < TJ) {
        const int j = j0 + tid;
        const double xv = (j < Ns) ? x[j] : 0.0;
        sx[tid] = xv / beta;                                   // kernels.py:38-39 (inputs scaled by 1/beta)
    }
    __syncthreads();
    const int i = I * 64 + lane;
    if (i >= N) return;
    const bool real = i < Ns;
    const double xi = x[real ? i : 0] / beta;
    const double xi2 = xi * xi;
    const double a2 = alpha * alpha;
    for (int jj = 0; jj < TJ / 4; ++jj) {
        const int k = w * (TJ / 4) + jj;
        const int j = j0 + k;
        if (j >= N) break;
        if (i < j) continue;
        double v;
        if (real) {
            const double xj = sx[k];
            const double dist = (xi2 + xj * xj) - 2.0 * (xi * xj);
            v = exp(-0.5 * dist) * a2;                         // kernels.py:42
            if (i == j) v = NMGP_JITTER + v;
        } else {
            v = (i == j) ? 1.0 : 0.0;
        }
        out[(size_t)j * ld + i] = v;
    }
}

// prior right-hand sides (k_svc_prior_rhs): column 0 = tilde_l - mu_l, column 1 + t = L_vecs[:, t] - mu_L on the real observations,
// zeros on the padded ones (their parameter slots are not read)
__global__ void k_hadc_prior_rhs(const double* __restrict__ pars, const int* __restrict__ nobs, int cps, int N, int T, double mu_l,
                                 double mu_L, double* __restrict__ R, int ld) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int Ns = nobs[blockIdx.y / cps];
    pars += (size_t)blockIdx.y * ((size_t)N * (1 + T) + 1);
    R += (size_t)blockIdx.y * (1 + T) * ld;
    if (i >= Ns) {
        for (int t = 0; t <= T; ++t) R[(size_t)t * ld + i] = 0.0;
        return;
    }
    R[i] = pars[i] - mu_l;
    for (int t = 0; t < T; ++t) R[(size_t)(1 + t) * ld + i] = pars[N + (size_t)i * T + t] - mu_L;
}

// k_svc_finalize with the subject's own N_s in the N log 2 pi of the 1 + T prior terms (the kernel it restates multiplies by the
// launch's one N); ig_const = 0: the unnormalised inverse gamma of the Hadamard objective.  hl_l / hl_L: per-subject half log-dets.
__global__ void k_hadc_finalize(const double* __restrict__ logdet, const double* __restrict__ quad, const double* __restrict__ q,
                                const double* __restrict__ hl_l, const double* __restrict__ hl_L, const double* __restrict__ pars,
                                long long P, const int* __restrict__ nobs, int cps, int T, double a, double b, double ig_const,
                                int prior, double* __restrict__ out5, int sstride) {
    if (threadIdx.x != 0) return;
    const int sub = blockIdx.x / cps;
    const int N = nobs[sub];
    hl_l += sub;
    hl_L += sub;
    logdet += (size_t)blockIdx.x * sstride;
    quad += (size_t)blockIdx.x * sstride;
    out5 += (size_t)blockIdx.x * sstride;
    q += (size_t)blockIdx.x * (1 + T);
    pars += (size_t)blockIdx.x * P;
    const double LOG2PI = 1.8378770664093453;
    const double tse = pars[P - 1];
    const double sigma2 = exp(tse);
    const double loglik = -0.5 * logdet[0] - 0.5 * quad[0];
    const double lp_l = -0.5 * (N * LOG2PI + q[0]) - hl_l[0];
    double lp_uL = 0.0;
    for (int t = 0; t < T; ++t) lp_uL += -0.5 * (N * LOG2PI + q[1 + t]) - hl_L[0];
    const double lp_s2 = (-a - 1.0) * log(sigma2) - b / sigma2 + ig_const;
    double res = 0.0;
    res += loglik;
    if (prior) {
        res += lp_l;
        res += lp_uL;
        res += lp_s2;
        res += tse;
    }
    out5[0] = -res;
    out5[1] = loglik;
    out5[2] = lp_l;
    out5[3] = lp_uL;
    out5[4] = lp_s2;
}

// k_trace_terms over the REAL observations: out[0] = sum_{r < N_s} alpha_r^2, out[1] = ssign sum_{r < N_s} Sinv[r, r] (over Nmax the
// trace would count one per padded observation and shift d / d tilde_sigma2_err)
__global__ __launch_bounds__(1024) void k_hadc_trace(const double* __restrict__ alpha, const double* __restrict__ Sinv, int ld, int N,
                                                      const int* __restrict__ nobs, int cps, double* __restrict__ out, double ssign) {
    __shared__ double sh[16];
    const int n = nobs[blockIdx.x / cps];
    alpha += (size_t)blockIdx.x * N;
    Sinv += (size_t)blockIdx.x * ld * N;
    out += (size_t)blockIdx.x * 2;
    double a = 0.0, d = 0.0;
    for (int r = threadIdx.x; r < n; r += blockDim.x) {
        a += alpha[r] * alpha[r];
        d += Sinv[(size_t)r * ld + r];
    }
    a = hadc_block_sum(a, sh);
    d = hadc_block_sum(d, sh);
    if (threadIdx.x == 0) {
        out[0] = a;
        out[1] = ssign * d;
    }
}

// k_had_grad_final on the padded layout: the J partials summed in order, the c_i + 1 components of d / d r_i scattered into row c_i's
// slots, the prior gradients of all T columns, for the real i; +0.0 in every padded slot; the sigma2 slot from the trace over the real
// observations (tr, k_hadc_trace).
__global__ __launch_bounds__(256) void k_hadc_grad_final(const double* __restrict__ part, long long pstride, int NJ, int N, int M,
                                                          int T, const int* __restrict__ indx, const int* __restrict__ nobs, int cps,
                                                          const double* __restrict__ R2, int ldR, const double* __restrict__ pars,
                                                          const double* __restrict__ tr, double a, double b, int prior,
                                                          double* __restrict__ grad) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const size_t P = (size_t)N * (1 + T) + 1;
    const int sub = blockIdx.y / cps;
    const int Ns = nobs[sub];
    {   // blockIdx.y = chain
        const size_t z = blockIdx.y;
        part += z * (size_t)pstride;
        R2 += z * (size_t)(1 + T) * ldR;
        pars += z * P;
        tr += z * 2;
        grad += z * P;
        indx += (size_t)sub * N;
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
        for (int t = 0; t < T; ++t) grad[N + (size_t)i * T + t] = 0.0;
        return;
    }
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

void free_factors(std::vector<PriorFactor>& v) {
    for (auto& pf : v) {
        if (pf.L) hipFree(pf.L);
        if (pf.logdet) hipFree(pf.logdet);
    }
    v.clear();
}

// per-subject factors of the masked RBF(x_s; alpha, beta) + jitter I by ONE batched factorisation (precise panels, as
// nmgp_get_batch_prior), cached with the set
int hadc_get_prior(nmgp_ctx* c, double alpha, double beta, PriorFactor** out) {
    for (auto& p : c->hc_priors)
        if (p.alpha == alpha && p.beta == beta) {
            *out = &p;
            return 0;
        }
    PriorFactor pf;
    pf.alpha = alpha;
    pf.beta = beta;
    const size_t N = c->hc_Nmax, S = c->hc_S;
    pf.ld = (int)nmgp_ld(N);
    NMGP_TRY(nmgp_dev_alloc(c, &pf.L, S * (size_t)pf.ld * N));
    if (nmgp_dev_alloc(c, &pf.logdet, S) != 0) {
        hipFree(pf.L);
        return NMGP_E_NOMEM;
    }
    int* info = nullptr;
    if (hipMalloc((void**)&info, S * sizeof(int)) != hipSuccess) {
        hipFree(pf.L);
        hipFree(pf.logdet);
        return nmgp_fail(c, NMGP_E_NOMEM, "hipMalloc of the prior status words failed");
    }
    hipMemsetAsync(info, 0, S * sizeof(int), c->stream);
    NMGP_LAUNCH(k_hadc_rbf, dim3(cdiv(N, 64), cdiv(N, 64), (unsigned)S), dim3(256), 0, c->stream, c->hc_x, c->hc_nobs, (int)N, alpha, beta,
                pf.L, pf.ld);
    nmgp_potrf(c, pf.L, pf.ld, (int)N, 0, 0, info, (int)S, (long long)pf.ld * N, 1, 1);
    half_logdet(c->stream, pf.L, pf.ld, (int)N, pf.logdet, (int)S);
    std::vector<int> hi(S);
    hipMemcpyAsync(hi.data(), info, S * sizeof(int), hipMemcpyDeviceToHost, c->stream);
    const hipError_t e = hipStreamSynchronize(c->stream);
    hipFree(info);
    int bad = 0, who = -1;
    for (size_t b = 0; b < S; ++b)
        if (hi[b] != 0 && bad == 0) {
            bad = hi[b];
            who = (int)b;
        }
    if (e != hipSuccess || bad != 0) {
        hipFree(pf.L);
        hipFree(pf.logdet);
        if (e != hipSuccess) return nmgp_fail(c, NMGP_E_HIP, "batched prior factorisation failed (%s)", hipGetErrorString(e));
        return nmgp_fail(c, bad, "GP prior covariance RBF(alpha=%g, beta=%g)+jitter of subject %d is not positive definite "
                         "(leading minor %d)", alpha, beta, who, bad);
    }
    c->hc_priors.push_back(pf);
    *out = &c->hc_priors.back();
    return 0;
}

}  // namespace

// what the evaluation entries (nmgp_hadamard_cohort_models.hip) take from this file: the set's two per-subject prior factors of
// hyper[1..2] and hyper[4..5], the masked trace, and the launches of the nonseparable model's own kernels (CohNon's hooks)
void nmgp_hadc_prep(hipStream_t s, const double* pars, const int* indx, const int* nobs, int cps, int N, int M, int T, double* ell,
                    double* Rv, int batch) {
    NMGP_LAUNCH(k_hadc_prep, dim3(cdiv(N, 256), batch), dim3(256), 0, s, pars, indx, nobs, cps, N, M, T, ell, Rv);
}
void nmgp_hadc_prior_rhs(hipStream_t s, const double* pars, const int* nobs, int cps, int N, int T, double mu_l, double mu_L, double* R,
                         int ld, int batch) {
    NMGP_LAUNCH(k_hadc_prior_rhs, dim3(cdiv(N, 256), batch), dim3(256), 0, s, pars, nobs, cps, N, T, mu_l, mu_L, R, ld);
}
void nmgp_hadc_finalize(hipStream_t s, double* scal, const double* q, const double* hl_l, const double* hl_L, const double* pars,
                        long long P, const int* nobs, int cps, int T, double a, double b, int prior, int batch) {
    NMGP_LAUNCH(k_hadc_finalize, dim3(batch), dim3(64), 0, s, scal, scal + 1, q, hl_l, hl_L, pars, P, nobs, cps, T, a, b, 0.0, prior,
                scal + 8, 16);
}
void nmgp_hadc_grad_final(hipStream_t s, const double* part, long long pstride, int N, int M, int T, const int* indx, const int* nobs,
                          int cps, const double* R2, const double* pars, const double* tr, double a, double b, int prior, double* grad,
                          int batch) {
    NMGP_LAUNCH(k_hadc_grad_final, dim3(cdiv(N, 256), batch), dim3(256), 0, s, part, pstride, (N + 63) / 64, N, M, T, indx, nobs, cps, R2,
                N, pars, tr, a, b, prior, grad);
}
int nmgp_hadc_priors(nmgp_ctx* c, const double* hyper, PriorFactor** p0, PriorFactor** p1) {
    NMGP_TRY(hadc_get_prior(c, hyper[1], hyper[2], p0));
    NMGP_TRY(hadc_get_prior(c, hyper[4], hyper[5], p1));
    return hadc_get_prior(c, hyper[1], hyper[2], p0);
}
void nmgp_hadc_trace(hipStream_t s, const double* alpha, const double* Sinv, int ld, int N, const int* nobs, int cps, double* out,
                     double ssign, int batch) {
    NMGP_LAUNCH(k_hadc_trace, dim3(batch), dim3(1024), 0, s, alpha, Sinv, ld, N, nobs, cps, out, ssign);
}

void nmgp_had_subjects_free(nmgp_ctx* c) {
    if (c->hc_x) hipFree(c->hc_x);
    if (c->hc_y) hipFree(c->hc_y);
    if (c->hc_indx) hipFree(c->hc_indx);
    if (c->hc_nobs) hipFree(c->hc_nobs);
    c->hc_x = c->hc_y = nullptr;
    c->hc_indx = c->hc_nobs = nullptr;
    c->hc_nobs_h.clear();
    free_factors(c->hc_priors);
    c->hc_S = c->hc_Nmax = c->hc_M = c->hc_T = 0;
}

extern "C" int nmgp_had_set_subjects(nmgp_ctx* c, const double* x, const int* indx, const double* y, const int* nobs, int S, int Nmax,
                                     int M) {
    if (!c) return NMGP_E_NULL;
    if (!x || !indx || !y || !nobs) return nmgp_fail(c, NMGP_E_NULL, "nmgp_had_set_subjects: x, indx, y and nobs must not be NULL");
    if (S < 1 || M < 1 || M > 8 || Nmax < 1 || Nmax > 3500)
        return nmgp_fail(c, NMGP_E_SHAPE, "nmgp_had_set_subjects: S=%d must be positive, M=%d in [1, 8] and Nmax=%d in [1, 3500]", S, M,
                         Nmax);
    for (int s = 0; s < S; ++s) {
        if (nobs[s] < M || nobs[s] > Nmax)
            return nmgp_fail(c, NMGP_E_SHAPE, "nmgp_had_set_subjects: nobs[%d] = %d is outside [M = %d, Nmax = %d]", s, nobs[s], M, Nmax);
        const int* ix = indx + (size_t)s * Nmax;
        char seen[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int i = 0; i < nobs[s]; ++i) {
            if (ix[i] < 0 || ix[i] >= M)
                return nmgp_fail(c, NMGP_E_SHAPE, "nmgp_had_set_subjects: indx[%d, %d] = %d is outside [0, %d)", s, i, ix[i], M);
            seen[ix[i]] = 1;
        }
        for (int m = 0; m < M; ++m)
            if (!seen[m])
                return nmgp_fail(c, NMGP_E_SHAPE, "nmgp_had_set_subjects: output label %d of %d never occurs in subject %d", m, M, s);
    }
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    nmgp_had_subjects_free(c);
    const size_t SN = (size_t)S * Nmax;
    hipStream_t st = c->stream;
    auto fail = [c](int r) {
        nmgp_had_subjects_free(c);
        return r;
    };
    if (nmgp_dev_alloc(c, &c->hc_x, SN) != 0 || nmgp_dev_alloc(c, &c->hc_y, SN) != 0) return fail(NMGP_E_NOMEM);
    if (hipMalloc((void**)&c->hc_indx, SN * sizeof(int)) != hipSuccess || hipMalloc((void**)&c->hc_nobs, (size_t)S * sizeof(int)) != hipSuccess)
        return fail(nmgp_fail(c, NMGP_E_NOMEM, "nmgp_had_set_subjects: hipMalloc of the label tables failed"));
    // zero padding on the device; only the first nobs[s] entries of a row are read from the caller's arrays
    bool ok = hipMemsetAsync(c->hc_x, 0, SN * sizeof(double), st) == hipSuccess &&
              hipMemsetAsync(c->hc_y, 0, SN * sizeof(double), st) == hipSuccess &&
              hipMemsetAsync(c->hc_indx, 0, SN * sizeof(int), st) == hipSuccess;
    for (int s = 0; s < S && ok; ++s) {
        const size_t o = (size_t)s * Nmax, n = (size_t)nobs[s];
        ok = hipMemcpyAsync(c->hc_x + o, x + o, n * sizeof(double), hipMemcpyHostToDevice, st) == hipSuccess &&
             hipMemcpyAsync(c->hc_y + o, y + o, n * sizeof(double), hipMemcpyHostToDevice, st) == hipSuccess &&
             hipMemcpyAsync(c->hc_indx + o, indx + o, n * sizeof(int), hipMemcpyHostToDevice, st) == hipSuccess;
    }
    ok = ok && hipMemcpyAsync(c->hc_nobs, nobs, (size_t)S * sizeof(int), hipMemcpyHostToDevice, st) == hipSuccess;
    ok = ok && hipStreamSynchronize(st) == hipSuccess;
    if (!ok) return fail(nmgp_fail(c, NMGP_E_HIP, "nmgp_had_set_subjects: upload failed (%s)", hipGetErrorString(hipGetLastError())));
    c->hc_nobs_h.assign(nobs, nobs + S);
    c->hc_S = S;
    c->hc_Nmax = Nmax;
    c->hc_M = M;
    c->hc_T = M * (M + 1) / 2;
    return 0;
}

extern "C" int nmgp_had_clear_subjects(nmgp_ctx* c) {
    if (!c) return NMGP_E_NULL;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    nmgp_had_subjects_free(c);
    return 0;
}

// ---- MAP and posterior-draw prediction for the set: nmgp_predsample_had_subjects -------------------------------------------------------
// ps_predict<PsHad>'s schedule (nmgp_predsample_common.h, nmgp_predsample_had.hip) with the subject as a table look-up, written as a
// sibling: ps_predict and k_psn_* serve six entries whose bits are pinned, so no table is threaded through them.  Subject s brings its
// own new inputs xs[s, 0 .. nstar[s]) of a padded [S, Smax] array.  Once per call and distinct (alpha, beta): k* of all subjects with
// exact zeros at padded observations and in padded input columns (k_hadc_kstar), the two prior_trsv passes with batch = S against the
// set's per-subject factors, the clipped conditional variances (k_hadc_condvar).  Per chunk of draws (whole subjects, or a part of ONE
// subject's draws: no kernel takes a draw offset): k_hadc_prep, the starred values, per slice of new inputs {k_hadc_cov, y and the
// riding cross-covariance rows, batched nmgp_potrf with precise panels, ps_rows_reduce}, the variance, the downloads, ONE
// synchronisation.  The kernels keep k_psn_star / k_psn_cross_rows / k_psn_predvar's lane mapping and expression order (a subject
// with N_s = Nmax and nstar = Smax gets their bits) and take subject = draw / draws-per-subject of the chunk; every mask comes from
// the nobs and nstar tables, never from the contents of a padded slot, and every sum has a fixed order.
namespace {

// W[s, j, i] = RBF(xs[s, j], x[s, i]; alpha, beta) (k_rect<1>'s expressions in their order, its lane mapping: lanes along i), exact
// zero for a padded observation i >= nobs[s] or a padded new input j >= nstar[s].  blockIdx.z = subject.
__global__ __launch_bounds__(256) void k_hadc_kstar(const double* __restrict__ x, const int* __restrict__ nobs,
                                                     const double* __restrict__ xs, const int* __restrict__ nstar, int N, int Smax,
                                                     double alpha, double beta, double* __restrict__ W) {
    const int i = blockIdx.x * 64 + (threadIdx.x & 63);
    const int j = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int sub = blockIdx.z;
    if (i >= N || j >= Smax) return;
    double v = 0.0;
    if (i < nobs[sub] && j < nstar[sub]) {
        const double a = xs[(size_t)sub * Smax + j] / beta, b = x[(size_t)sub * N + i] / beta;
        const double xn = a * a, yn = b * b, dot = a * b;
        const double dist = (xn + yn) - 2.0 * dot;
        v = exp(-0.5 * dist) * (alpha * alpha);
    }
    W[((size_t)sub * Smax + j) * N + i] = v;
}

// k_ps_condvar over the subject's real observations: cv[s, j] = (alpha^2 + jitter) - W[s, j] . k_j summed over i < nobs[s] in its
// order, a value < 0 replaced by settings.precision; +0.0 for a padded new input.  blockIdx = (new input, subject).
__global__ __launch_bounds__(256) void k_hadc_condvar(const double* __restrict__ W, const double* __restrict__ x,
                                                       const int* __restrict__ nobs, const double* __restrict__ xs,
                                                       const int* __restrict__ nstar, int N, int Smax, double alpha, double beta,
                                                       double* __restrict__ cv) {
    __shared__ double sh[256];
    const int s = blockIdx.x, sub = blockIdx.y;
    const size_t o = (size_t)sub * Smax + s;
    if (s >= nstar[sub]) {
        if (threadIdx.x == 0) cv[o] = 0.0;
        return;
    }
    const int Ns = nobs[sub];
    x += (size_t)sub * N;
    const double b = xs[o] / beta;
    double acc = 0.0;
    for (int i = threadIdx.x; i < Ns; i += 256) {
        const double a = x[i] / beta;
        const double dist = (a * a + b * b) - 2.0 * (a * b);
        acc += W[o * N + i] * (exp(-0.5 * dist) * (alpha * alpha));
    }
    acc = block_sum_256(acc, sh);
    if (threadIdx.x == 0) {
        double v = (NMGP_JITTER + alpha * alpha) - acc;
        if (v < 0.0) v = NMGP_PRECISION;
        cv[o] = v;
    }
}

// k_psn_star with subject = draw / cps: the sum runs over the subject's real observations (the padded parameter slots are not read),
// +0.0 for a padded new input (z is not read there).  W0 / W1: [S, Smax, N]; cv0 / cv1: [S, Smax]; star, z: [B, Smax, 1 + T].
__global__ __launch_bounds__(256) void k_hadc_star(const double* __restrict__ W0, const double* __restrict__ W1,
                                                    const double* __restrict__ cv0, const double* __restrict__ cv1,
                                                    const double* __restrict__ pars, long long P, const double* __restrict__ z,
                                                    const int* __restrict__ nobs, const int* __restrict__ nstar, int cps, int N, int T,
                                                    int S, double mu_l, double mu_L, double* __restrict__ star) {
    __shared__ double sh[256];
    const int s = blockIdx.x, cidx = blockIdx.y, h = blockIdx.z;
    const int sub = h / cps;
    const size_t o = ((size_t)h * S + s) * (1 + T) + cidx;
    if (s >= nstar[sub]) {
        if (threadIdx.x == 0) star[o] = 0.0;
        return;
    }
    const int Ns = nobs[sub];
    const size_t ws = (size_t)sub * S + s;
    const double* p = pars + (size_t)h * P;
    const double* W = (cidx == 0 ? W0 : W1) + ws * N;
    const double mu = cidx == 0 ? mu_l : mu_L;
    const double* cur = cidx == 0 ? p : p + N + (cidx - 1);
    const size_t stride = cidx == 0 ? 1 : (size_t)T;
    double acc = 0.0;
    for (int i = threadIdx.x; i < Ns; i += 256) acc += W[i] * (cur[(size_t)i * stride] - mu);
    acc = block_sum_256(acc, sh);
    if (threadIdx.x != 0) return;
    double v = mu + acc;
    if (z) v = v + sqrt((cidx == 0 ? cv0 : cv1)[ws]) * z[o];
    star[o] = v;
}

// the caller's starred values (star_in) as uploaded: +0.0 into the padded new-input slots, which are not read
__global__ void k_hadc_star_mask(const int* __restrict__ nstar, int cps, int S, int W, double* __restrict__ star) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x, h = blockIdx.y;
    if (k >= S * W) return;
    if (k / W >= nstar[h / cps]) star[(size_t)h * S * W + k] = 0.0;
}

// k_psn_cross_rows<M> with subject = draw / cps: riding row R0 + e below the matrix of draw h = blockIdx.z, observation
// i = blockIdx.x; lanes along the riding-row index (contiguous in a column).  Exact zero for a padded observation or a padded new
// input (whose x, label and starred values are not read).  istar: [S_set, S] labels, nullptr in the full form.
template <int M>
__global__ __launch_bounds__(256) void k_hadc_cross_rows(const double* __restrict__ x, const double* __restrict__ ell,
                                                          const double* __restrict__ Rv, const int* __restrict__ nobs,
                                                          const int* __restrict__ nstar, int cps, int N,
                                                          const double* __restrict__ xs, const double* __restrict__ star,
                                                          const int* __restrict__ istar, int S, int s0, int E, double* __restrict__ A,
                                                          int ld, long long bstride, int R0) {
    constexpr int T = M * (M + 1) / 2;
    const int e = blockIdx.y * 256 + threadIdx.x;
    const int i = blockIdx.x, h = blockIdx.z;
    if (e >= E) return;
    const int sub = h / cps;
    const int s = istar ? s0 + e : s0 + e / M;
    double* out = A + (size_t)h * bstride + (size_t)i * ld + R0 + e;
    if (i >= nobs[sub] || s >= nstar[sub]) {
        *out = 0.0;
        return;
    }
    const int mp = istar ? istar[(size_t)sub * S + s] : e % M;
    const double* st = star + ((size_t)h * S + s) * (1 + T);
    const double* ri = Rv + ((size_t)h * N + i) * M;
    const double xi = x[(size_t)sub * N + i], li = ell[(size_t)h * N + i];
    const double xj = xs[(size_t)sub * S + s], lj = exp(st[0]);
    const double dist = (xi * xi + xj * xj) - 2.0 * (xi * xj);
    const double Aij = li * li + lj * lj;
    const double kv = sqrt(2.0 * (li * lj) / Aij) * exp(-dist / Aij);
    double b = 0.0;
    for (int r = 0; r <= mp; ++r) b += ri[r] * st[1 + mp * (mp + 1) / 2 + r];
    *out = kv * b;
}

// k_psn_predvar with subject = draw / cps; a padded new input gets +0.0 in var AND in mean (the slices past the chunk's largest
// nstar are not factorised, so nothing else writes those slots).
__global__ __launch_bounds__(256) void k_hadc_predvar(const double* __restrict__ star, const double* __restrict__ pars, long long P,
                                                       const double* __restrict__ colsq, const int* __restrict__ istar,
                                                       const int* __restrict__ nstar, int cps, int S, int M, int T,
                                                       double* __restrict__ mean, double* __restrict__ var) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x, h = blockIdx.y;
    const int O = istar ? S : S * M;
    if (k >= O) return;
    const int sub = h / cps;
    const int s = istar ? k : k / M;
    if (s >= nstar[sub]) {
        mean[(size_t)h * O + k] = 0.0;
        var[(size_t)h * O + k] = 0.0;
        return;
    }
    const int mp = istar ? istar[(size_t)sub * S + s] : k % M;
    const double* st = star + ((size_t)h * S + s) * (1 + T) + 1;
    double b = 0.0;
    for (int r = 0; r <= mp; ++r) {
        const double v = st[mp * (mp + 1) / 2 + r];
        b += v * v;
    }
    const double kss = NMGP_JITTER + 1.0;
    double v = (kss * b - colsq[(size_t)h * O + k]) + exp(pars[(size_t)h * P + (P - 1)]);
    if (v <= 0.0) v = NMGP_PRECISION;
    var[(size_t)h * O + k] = v;
}

// W = Sigma_prior^-1 K* of all S subjects ([S, Smax, N]) against the set's per-subject factors, by substitution (nmgp_ps_project's
// order: k* first, forward, backward), and the conditional variances cv [S, Smax].  The factor's padded part is the identity and the
// right-hand side there is 0: padded observations contribute exact zeros to W.
int hadc_project(nmgp_ctx* c, const PriorFactor* pf, const double* d_xs, const int* d_nstar, int Smax, double* W, double* cv) {
    const int N = c->hc_Nmax, S = c->hc_S;
    hipStream_t s = c->stream;
    const long long f = (long long)pf->ld * N;
    NMGP_LAUNCH(k_hadc_kstar, dim3(cdiv(N, 64), cdiv(Smax, 4), S), dim3(256), 0, s, c->hc_x, c->hc_nobs, d_xs, d_nstar, N, Smax,
                pf->alpha, pf->beta, W);
    prior_trsv(s, false, pf->L, pf->ld, f, pf->L, pf->ld, f, W, N, Smax, S, 1);
    prior_trsv(s, true, pf->L, pf->ld, f, pf->L, pf->ld, f, W, N, Smax, S, 1);
    NMGP_LAUNCH(k_hadc_condvar, dim3(Smax, S), dim3(256), 0, s, W, c->hc_x, c->hc_nobs, d_xs, d_nstar, N, Smax, pf->alpha, pf->beta,
                cv);
    return 0;
}

}  // namespace

extern "C" int nmgp_predsample_had_subjects(nmgp_ctx* c, const double* pars, int B, int draws_per_subject, const double hyper[8],
                                            const double* xs, const int* indx_star, const int* nstar, int Smax, const double* z,
                                            const double* star_in, double* mean, double* var, double* star_out, int* status) {
    if (!c) return NMGP_E_NULL;
    if (!pars || !hyper || !xs || !mean || !var) return nmgp_fail(c, NMGP_E_NULL, "pars/hyper/xs/mean/var must not be NULL");
    if (c->hc_S <= 0) return nmgp_fail(c, NMGP_E_STATE, "nmgp_had_set_subjects must be called first");
    if (z && star_in) return nmgp_fail(c, NMGP_E_STATE, "with star_in given the regression is skipped: z must be NULL");
    if (c->chol_algo != 1)
        return nmgp_fail(c, NMGP_E_UNSUPPORTED, "the Hadamard entries run on the custom factorisation only (riding rows)");
    const int S = c->hc_S, N = c->hc_Nmax, M = c->hc_M, T = c->hc_T, H = draws_per_subject, SW = 1 + T;
    if (H < 1 || Smax < 1 || (long long)B != (long long)S * H)
        return nmgp_fail(c, NMGP_E_SHAPE, "B = %d must be %d subjects x draws_per_subject = %d (>= 1), and Smax = %d positive", B, S, H,
                         Smax);
    const bool indexed = indx_star != nullptr;
    // the tables of the new inputs, with zeros in the padded slots: nothing of the caller's padded slots is read
    std::vector<int> hns(S), his(indexed ? (size_t)S * Smax : 0, 0);
    std::vector<double> hxs((size_t)S * Smax, 0.0);
    for (int s = 0; s < S; ++s) {
        const int ns = nstar ? nstar[s] : Smax;
        if (ns < 0 || ns > Smax)
            return nmgp_fail(c, NMGP_E_SHAPE, "nmgp_predsample_had_subjects: nstar[%d] = %d is outside [0, Smax = %d]", s, ns, Smax);
        hns[s] = ns;
        const size_t o = (size_t)s * Smax;
        std::copy(xs + o, xs + o + ns, hxs.begin() + o);
        for (int j = 0; j < ns && indexed; ++j) {
            const int m = indx_star[o + j];
            if (m < 0 || m >= M)
                return nmgp_fail(c, NMGP_E_SHAPE, "indx_star[%d, %d] = %d is not an output label in [0, %d)", s, j, m, M);
            his[o + j] = m;
        }
    }
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const size_t P = (size_t)N * (1 + T) + 1;
    const int per = PsHadamard::rows(M, indexed);
    // riding rows per factorisation: the resident entry's rule at Nmax
    const int smax = PsHadamard::smax(N, M, indexed);
    const int Emax = std::min(Smax, smax) * per;
    const int ld = (int)nmgp_ld((size_t)N + 1 + Emax);
    const long long bs = (long long)ld * N;
    if (bs >= 0x7fffffffLL)
        return nmgp_fail(c, NMGP_E_SHAPE, "a matrix of order Nmax = %d with %d riding rows exceeds the 2^31 elements the row kernels index",
                         N, ld - N);
    const int chunks = (N + 127) / 128;
    // a chunk is a whole number of subjects, or a part of ONE subject's draws (then every draw of the chunk is that subject's)
    int Bc = nmgp_ps_chunk(B, (size_t)(N + 1 + Emax) * ld);
    const bool split = H > Bc;
    if (!split) Bc = (Bc / H) * H;
    const size_t SC = (size_t)Smax * SW, O = (size_t)Smax * per, Bs = Bc, SS = (size_t)S * Smax;

    const bool regress = !star_in;
    PriorFactor *p0 = nullptr, *p1 = nullptr;
    if (regress) {   // (the cache is a vector: the second look-up may move its elements, so the first is re-resolved)
        NMGP_TRY(hadc_get_prior(c, hyper[1], hyper[2], &p0));
        NMGP_TRY(hadc_get_prior(c, hyper[4], hyper[5], &p1));
        NMGP_TRY(hadc_get_prior(c, hyper[1], hyper[2], &p0));
    }
    const bool same = p0 == p1;
    size_t off = 0;
    auto take = [&off](size_t nelem) {
        const size_t o = off;
        off += (nelem + 15) / 16 * 16;
        return o;
    };
    const size_t o_xs = take(SS), o_is = take(indexed ? (SS + 1) / 2 : 0), o_ns = take(((size_t)S + 1) / 2),
                 o_W0 = take(regress ? SS * N : 0), o_W1 = take(regress && !same ? SS * N : 0), o_cv = take(regress ? 2 * SS : 0),
                 o_pars = take(Bs * P), o_ell = take(Bs * N), o_Rv = take(Bs * N * M), o_star = take(Bs * SC),
                 o_z = take(z ? Bs * SC : 0), o_mean = take(Bs * O), o_sqs = take(Bs * O), o_var = take(Bs * O),
                 o_part = take(Bs * 2 * Emax * chunks), o_info = take((Bs + 1) / 2), o_S = take(Bs * bs);
    if (c->ps_cap < off) {
        c->ps_cap = 0;
        NMGP_TRY(nmgp_dev_alloc(c, &c->ps_buf, off));
        c->ps_cap = off;
    } else if (nmgp_poison()) {
        HIP_TRY(c, hipMemsetAsync(c->ps_buf, 0xFF, off * sizeof(double), st));
    }
    double* w = c->ps_buf;
    double *d_xs = w + o_xs, *W0 = w + o_W0, *W1 = same ? W0 : w + o_W1, *cv0 = w + o_cv, *cv1 = same ? cv0 : cv0 + SS;
    double *dP = w + o_pars, *ell = w + o_ell, *Rv = w + o_Rv, *d_star = w + o_star, *d_z = z ? w + o_z : nullptr;
    double *d_mean = w + o_mean, *d_sqs = w + o_sqs, *d_var = w + o_var, *part = w + o_part, *Sb = w + o_S;
    int* d_is = indexed ? reinterpret_cast<int*>(w + o_is) : nullptr;
    int* d_ns = reinterpret_cast<int*>(w + o_ns);
    int* d_info = reinterpret_cast<int*>(w + o_info);

    HIP_TRY(c, hipMemcpyAsync(d_xs, hxs.data(), SS * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(d_ns, hns.data(), (size_t)S * sizeof(int), hipMemcpyHostToDevice, st));
    if (indexed) HIP_TRY(c, hipMemcpyAsync(d_is, his.data(), SS * sizeof(int), hipMemcpyHostToDevice, st));
    if (regress) {   // once per call per distinct prior factor, for all subjects at once
        NmgpStage sp(c, NMGP_STAGE_PRIOR);
        NMGP_TRY(hadc_project(c, p0, d_xs, d_ns, Smax, W0, cv0));
        if (!same) NMGP_TRY(hadc_project(c, p1, d_xs, d_ns, Smax, W1, cv1));
    }
    std::vector<int> hinfo(Bs);
    for (int b0 = 0; b0 < B;) {
        const int s0 = b0 / H;
        int nb = std::min(Bc, B - b0);
        if (split) nb = std::min(nb, (s0 + 1) * H - b0);
        const int cps = split ? nb : H, nsub = split ? 1 : nb / H;
        // the tables of the chunk's first subject
        const double* x = c->hc_x + (size_t)s0 * N;
        const double* y = c->hc_y + (size_t)s0 * N;
        const int* indx = c->hc_indx + (size_t)s0 * N;
        const int* nobs = c->hc_nobs + s0;
        const int* ns = d_ns + s0;
        const double* cxs = d_xs + (size_t)s0 * Smax;
        const int* cis = indexed ? d_is + (size_t)s0 * Smax : nullptr;
        const double* hp = pars + (size_t)b0 * P;
        const int Sreal = *std::max_element(hns.begin() + s0, hns.begin() + s0 + nsub);   // slices past it hold padded inputs only
        HIP_TRY(c, hipMemcpyAsync(dP, hp, (size_t)nb * P * sizeof(double), hipMemcpyHostToDevice, st));
        NMGP_LAUNCH(k_hadc_prep, dim3(cdiv(N, 256), nb), dim3(256), 0, st, dP, indx, nobs, cps, N, M, T, ell, Rv);
        if (regress) {
            if (z) HIP_TRY(c, hipMemcpyAsync(d_z, z + (size_t)b0 * SC, nb * SC * sizeof(double), hipMemcpyHostToDevice, st));
            NmgpStage sp(c, NMGP_STAGE_PRIOR);
            const size_t wo = (size_t)s0 * Smax;
            NMGP_LAUNCH(k_hadc_star, dim3(Smax, SW, nb), dim3(256), 0, st, W0 + wo * N, W1 + wo * N, cv0 + wo, cv1 + wo, dP, (long long)P,
                        d_z, nobs, ns, cps, N, T, Smax, hyper[0], hyper[3], d_star);
        } else {
            HIP_TRY(c, hipMemcpyAsync(d_star, star_in + (size_t)b0 * SC, nb * SC * sizeof(double), hipMemcpyHostToDevice, st));
            NMGP_LAUNCH(k_hadc_star_mask, dim3(cdiv((long long)SC, 256), nb), dim3(256), 0, st, ns, cps, Smax, SW, d_star);
        }
        HIP_TRY(c, hipMemsetAsync(d_info, 0, (size_t)nb * sizeof(int), st));
        for (int j0 = 0; j0 < Sreal; j0 += smax) {
            const int Sc = std::min(smax, Smax - j0), E = Sc * per;
            {
                NmgpStage sp(c, NMGP_STAGE_COV);
                int r = hadc_cov_build<false>(st, x, ell, nullptr, Rv, dP, (long long)P, nobs, cps, Sb, ld, N, M, nb, bs);
                if (r) return nmgp_fail(c, r, "unsupported number of outputs M=%d", M);
                set_row(st, Sb, ld, N, y, N, nb, bs, N, cps);               // the subject's y (zero-padded at set time) rides as row Nmax
                const dim3 grid(N, cdiv(E, 256), nb);
                NMGP_HADS_SWITCH(M, NMGP_LAUNCH((k_hadc_cross_rows<MM>), grid, dim3(256), 0, st, x, ell, Rv, nobs, ns, cps, N, cxs, d_star,
                                                cis, Smax, j0, E, Sb, ld, bs, N + 1));
            }
            {
                NmgpStage sp(c, NMGP_STAGE_CHOL);
                nmgp_potrf(c, Sb, ld, N, 1 + E, 0, d_info, nb, bs, 1, 1);
            }
            NmgpStage sp(c, NMGP_STAGE_REDUCE);
            ps_rows_reduce(st, Sb, ld, bs, N, N + 1, N, E, part, nb, d_mean, d_sqs, (long long)O, (long long)j0 * per);
        }
        NMGP_LAUNCH(k_hadc_predvar, dim3(cdiv((long long)O, 256), nb), dim3(256), 0, st, d_star, dP, (long long)P, d_sqs, cis, ns, cps, Smax,
                    M, T, d_mean, d_var);
        double* hm = mean + (size_t)b0 * O;
        double* hv = var + (size_t)b0 * O;
        HIP_TRY(c, hipMemcpyAsync(hm, d_mean, nb * O * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipMemcpyAsync(hv, d_var, nb * O * sizeof(double), hipMemcpyDeviceToHost, st));
        if (star_out) HIP_TRY(c, hipMemcpyAsync(star_out + (size_t)b0 * SC, d_star, nb * SC * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipMemcpyAsync(hinfo.data(), d_info, (size_t)nb * sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));          // the one synchronisation of the chunk
        NMGP_TRY(nmgp_take_launch_error(c));
        for (int b = 0; b < nb; ++b) {
            int stt = hinfo[b];
            const int sub = s0 + b / cps;
            // the finiteness tests cover the row's REAL parameter slots and REAL outputs only
            const size_t Ns = (size_t)c->hc_nobs_h[sub], Or = (size_t)hns[sub] * per;
            const double* p = hp + (size_t)b * P;
            bool finite_in = std::isfinite(p[P - 1]);
            for (size_t t = 0; t < Ns && finite_in; ++t) finite_in = std::isfinite(p[t]);
            for (size_t t = 0; t < Ns * T && finite_in; ++t) finite_in = std::isfinite(p[(size_t)N + t]);
            if (!finite_in) stt = NMGP_NUM_NAN;
            double *m0 = hm + b * O, *v0 = hv + b * O;
            for (size_t i = 0; i < Or && stt == 0; ++i)
                if (!std::isfinite(m0[i]) || !std::isfinite(v0[i])) stt = NMGP_NUM_NAN;
            if (stt != 0)
                for (size_t i = 0; i < Or; ++i) m0[i] = v0[i] = std::nan("");
            if (status) status[b0 + b] = stt;
        }
        b0 += nb;
    }
    return 0;
}
