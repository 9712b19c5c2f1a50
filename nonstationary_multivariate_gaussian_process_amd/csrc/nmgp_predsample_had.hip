// Posterior-draw and held-out prediction of the nonseparable Hadamard model: H parameter vectors of the resident Hadamard subject, S
// new inputs.  Entry declared in include/nmgp.h.  The reference has no posterior-draw form for this model and its indexed MAP
// predictor (prediction.py:1480-1561) reports the variance of output 0 whatever the label; this entry is nmgp_predsample_hads'
// schedule (nmgp_predsample_hadamard.hip) with this model's covariance, starred values and cross-covariance.
//
// The covariance S_h = K_x o (R_h R_h^T) + sigma2 I depends on the draw only, so a chunk of B draws is ONE batched blocked Cholesky
// of B matrices of order N with y and the slice's E cross-covariance rows riding below each: nmgp_predict_had with the draw as a
// grid dimension.  A riding row is built from the draw's OWN sampled starred values (tilde_l*, the T raw slots of L*):
//   k_f[i, e] = g(i, s) <r_{h,i}, row m of L*_{h,s}>,   r_{h,i} = row indx[i] of the draw's L_i,
//   mean = (L^-1 k_f)^T (L^-1 y),   var = (1 + 1e-6) (L* L*^T)_mm - |L^-1 k_f|^2 + sigma2_err.
// Full form: e = (s - s0) M + m over all outputs m; indexed form (indx_star): e = s - s0, m = indx_star[s].
// The covariance build is nmgp_hadamard_common.h's, the per-draw unpacking nmgp_hadamard.hip's (had_prep).  Every kernel is per-draw
// independent with a fixed summation order: a batch of B draws gives the bits of B single calls.
#include <algorithm>

#include "nmgp_hadamard_common.h"
#include "nmgp_predsample_common.h"

using namespace nmgpk;

namespace {

inline unsigned cdiv(long long a, long long b) { return (unsigned)((a + b - 1) / b); }

// Starred values of draw h = blockIdx.z at new input s = blockIdx.x, slot cidx = blockIdx.y (0: tilde_l*, 1 + t: slot t of L*, taken
// as it is: no exp):  star = mu + proj_s . (curve - mu) + sqrt(cv_s) z  -- k_had_star's sum in its order, k_pss_star's noise.  One
// conditional variance per prior: cv1 serves all T slots.  z == nullptr: the conditional mean.  star, z: [B, S, 1 + T]; W0 / W1:
// [S, N]; cv0 / cv1: [S].
__global__ __launch_bounds__(256) void k_psn_star(const double* __restrict__ W0, const double* __restrict__ W1,
                                                   const double* __restrict__ cv0, const double* __restrict__ cv1,
                                                   const double* __restrict__ pars, long long P, const double* __restrict__ z, int N,
                                                   int T, int S, double mu_l, double mu_L, double* __restrict__ star) {
    __shared__ double sh[256];
    const int s = blockIdx.x, cidx = blockIdx.y, h = blockIdx.z;
    const double* p = pars + (size_t)h * P;
    const double* W = (cidx == 0 ? W0 : W1) + (size_t)s * N;
    const double mu = cidx == 0 ? mu_l : mu_L;
    const double* cur = cidx == 0 ? p : p + N + (cidx - 1);
    const size_t stride = cidx == 0 ? 1 : (size_t)T;
    double acc = 0.0;
    for (int i = threadIdx.x; i < N; i += 256) acc += W[i] * (cur[(size_t)i * stride] - mu);
    acc = block_sum_256(acc, sh);
    if (threadIdx.x != 0) return;
    const size_t o = ((size_t)h * S + s) * (1 + T) + cidx;
    double v = mu + acc;
    if (z) v = v + sqrt((cidx == 0 ? cv0 : cv1)[s]) * z[o];
    star[o] = v;
}

// Riding row R0 + e below the matrix of draw h = blockIdx.z, observation i = blockIdx.x; lanes along the riding-row index
// (contiguous in a column).  k_had_crosscov_rows' expressions in their order, with the draw's own starred values.
//   istar == nullptr: e = (s - s0) M + m;  else e = s - s0, m = istar[s]
template <int M>
__global__ __launch_bounds__(256) void k_psn_cross_rows(const double* __restrict__ x, const double* __restrict__ ell,
                                                         const double* __restrict__ Rv, int N, const double* __restrict__ xs,
                                                         const double* __restrict__ star, const int* __restrict__ istar, int S,
                                                         int s0, int E, double* __restrict__ A, int ld, long long bstride, int R0) {
    constexpr int T = M * (M + 1) / 2;
    const int e = blockIdx.y * 256 + threadIdx.x;
    const int i = blockIdx.x, h = blockIdx.z;
    if (e >= E) return;
    const int s = istar ? s0 + e : s0 + e / M;
    const int mp = istar ? istar[s] : e % M;
    const double* st = star + ((size_t)h * S + s) * (1 + T);
    const double* ri = Rv + ((size_t)h * N + i) * M;
    const double xi = x[i], li = ell[(size_t)h * N + i];
    const double xj = xs[s], lj = exp(st[0]);
    const double dist = (xi * xi + xj * xj) - 2.0 * (xi * xj);
    const double Aij = li * li + lj * lj;
    const double kv = sqrt(2.0 * (li * lj) / Aij) * exp(-dist / Aij);
    double b = 0.0;
    for (int r = 0; r <= mp; ++r) b += ri[r] * st[1 + mp * (mp + 1) / 2 + r];
    A[(size_t)h * bstride + (size_t)i * ld + R0 + e] = kv * b;
}

// k_had_predvar with the draw as blockIdx.y: O = S M outputs per draw (k = s M + m), or O = S in the indexed form (k = s,
// m = istar[s]).  A value <= 0 is replaced by settings.precision (prediction.py:1455-1461).
__global__ __launch_bounds__(256) void k_psn_predvar(const double* __restrict__ star, const double* __restrict__ pars, long long P,
                                                      const double* __restrict__ colsq, const int* __restrict__ istar, int S, int M,
                                                      int T, double* __restrict__ var) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x, h = blockIdx.y;
    const int O = istar ? S : S * M;
    if (k >= O) return;
    const int s = istar ? k : k / M;
    const int mp = istar ? istar[s] : k % M;
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

// hooks of the nonseparable Hadamard model into the shared schedule (nmgp_predsample_common.h)
struct PsHad : PsHadamard {
    static size_t P(int N, int T) { return (size_t)N * (1 + T) + 1; }
    static int star_width(int T) { return 1 + T; }
    template <class Take>
    static void extras(PsCall& k, Take take, size_t B) {
        k.o_ell = take(B * k.N);
        k.o_Rv = take(B * k.N * k.M);
    }
    static int prep(const PsCall& k) {
        had_prep(k.c->stream, k.pars, k.c->had_indx, k.N, k.M, k.at(k.o_ell), k.at(k.o_Rv), k.Bc);
        return 0;
    }
    static int star(const PsCall& k) {
        NMGP_LAUNCH(k_psn_star, dim3(k.S, 1 + k.T, k.Bc), dim3(256), 0, k.c->stream, k.W0, k.W1, k.cv0, k.cv1, k.pars, k.P, k.z, k.N, k.T,
                    k.S, k.hyper[0], k.hyper[3], k.star);
        return 0;
    }
    static int build_cov(const PsCall& k) {
        return gibbs_cov_build<false>(k.c->stream, k.c->d_x, k.at(k.o_ell), nullptr, k.at(k.o_Rv), k.pars, k.P, k.Sb, k.ld, k.N, k.M, k.Bc,
                                      k.bs);
    }
    static int cross_rows(const PsCall& k) {
        const dim3 grid(k.N, cdiv(k.E, 256), k.Bc);
        NMGP_HADS_SWITCH(k.M, NMGP_LAUNCH((k_psn_cross_rows<MM>), grid, dim3(256), 0, k.c->stream, k.c->d_x, k.at(k.o_ell), k.at(k.o_Rv),
                                          k.N, k.xs, k.star, k.is, k.S, k.s0, k.E, k.Sb, k.ld, k.bs, k.N + 1));
        return 0;
    }
    static int finish(const PsCall& k) {
        const long long O = (long long)k.S * k.per;
        NMGP_LAUNCH(k_psn_predvar, dim3(cdiv(O, 256), k.Bc), dim3(256), 0, k.c->stream, k.star, k.pars, k.P, k.sqs, k.is, k.S, k.M, k.T,
                    k.var);
        return 0;
    }
};

}  // namespace

extern "C" int nmgp_predsample_had(nmgp_ctx* c, const double* pars, int H, const double hyper[8], const double* xs,
                                   const int* indx_star, int S, const double* z, const double* star_in, double* mean, double* var,
                                   double* star_out, int* status) {
    return ps_predict<PsHad>(c, pars, H, hyper, xs, indx_star, S, 0, z, star_in, mean, var, star_out, status);
}

