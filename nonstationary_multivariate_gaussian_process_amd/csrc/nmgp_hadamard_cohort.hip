// A cohort of Hadamard subjects of RAGGED size per launch sequence: the set (nmgp_had_set_subjects, nmgp_had_clear_subjects), its
// per-subject GP-prior factors, the masked trace and the nonseparable model's own small kernels.  The three evaluation entries, their
// model hooks and their one chunk skeleton are in nmgp_hadamard_cohort_models.hip; the three prediction entries and their one
// schedule in nmgp_predsample_had_cohort.hip.
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

// what the evaluation and the prediction entries (nmgp_hadamard_cohort_models.hip, nmgp_predsample_had_cohort.hip) take from this
// file: the set's two per-subject prior factors of hyper[1..2] and hyper[4..5], the masked trace, and the launches of the nonseparable
// model's own kernels (CohNon's hooks, HcNon's unpacking)
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
    nmgp_had_traj_free(c);     // a begun trajectory belongs to the set
    nmgp_had_adam_free(c);     // ... and so does a begun optimiser
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
