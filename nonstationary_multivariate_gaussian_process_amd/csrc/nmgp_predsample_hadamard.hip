// Posterior-draw prediction of the separable Hadamard model (prediction.py:461-707: point_ / pointwise_ / indexedpoint_ /
// test_predsample_hadamard): H parameter vectors of the resident Hadamard subject, S new inputs.  Entry declared in include/nmgp.h.
//
// The covariance S_h = K_x o (R R^T) + sigma2 I depends on the draw only (the reference rebuilds and eigendecomposes it per draw AND
// per grid point), so a chunk of B draws is ONE batched blocked Cholesky of B matrices of order N with y and the slice's E
// cross-covariance rows riding below each: nmgp_predict_hads with the draw as a grid dimension.  A riding row is built from the
// draw's OWN sampled (tilde_l*, tilde_sigma*):
//   k_f[i, e] = s_i s*_s g(i, s) B_f[m, c_i],   B_f[m, c_i] = <row m of L_h, r_{h,i}>,
//   mean = (L^-1 k_f)^T (L^-1 y),   var = B_f[m, m] (s*_s^2 + 1e-6) - |L^-1 k_f|^2 + sigma2_err.
// Full form: e = (s - s0) M + m over all outputs m; indexed form (indx_star): e = s - s0, m = indx_star[s].
// The starred values are k_pss_star's (the regressions of the unconstrained curves under the two priors + sqrt(cv) z), the
// covariance build nmgp_hadamard_sep.hip's.  Every kernel is per-draw independent with a fixed summation order: a batch of B draws
// gives the bits of B single calls.
#include <algorithm>

#include "nmgp_predsample_common.h"

using namespace nmgpk;

namespace {

inline unsigned cdiv(long long a, long long b) { return (unsigned)((a + b - 1) / b); }

// Riding row R0 + e below the matrix of draw h = blockIdx.z, observation i = blockIdx.x; lanes along the riding-row index
// (contiguous in a column).  k_hads_crosscov_rows' expressions in their order, with the draw's own starred values.
//   istar == nullptr: e = (s - s0) M + m;  else e = s - s0, m = istar[s]
template <int M>
__global__ __launch_bounds__(256) void k_psh_cross_rows(const double* __restrict__ x, const double* __restrict__ ell,
                                                         const double* __restrict__ sig, const double* __restrict__ Rv,
                                                         const double* __restrict__ pars, long long P, int N,
                                                         const double* __restrict__ xs, const double* __restrict__ star,
                                                         const int* __restrict__ istar, int S, int s0, int E,
                                                         double* __restrict__ A, int ld, long long bstride, int R0) {
    const int e = blockIdx.y * 256 + threadIdx.x;
    const int i = blockIdx.x, h = blockIdx.z;
    if (e >= E) return;
    const int s = istar ? s0 + e : s0 + e / M;
    const int mp = istar ? istar[s] : e % M;
    const double* st = star + ((size_t)h * S + s) * 2;
    const double* Lvec = pars + (size_t)h * P + (size_t)2 * N;
    const double* ri = Rv + ((size_t)h * N + i) * M;
    const double xi = x[i], li = ell[(size_t)h * N + i];
    const double xj = xs[s], lj = exp(st[0]), sj = exp(st[1]);
    const double dist = (xi * xi + xj * xj) - 2.0 * (xi * xj);
    const double Aij = li * li + lj * lj;
    const double kv = (sig[(size_t)h * N + i] * sj) * sqrt(2.0 * (li * lj) / Aij) * exp(-dist / Aij);
    double b = 0.0;
    for (int r = 0; r <= mp; ++r) b += ri[r] * Lvec[mp * (mp + 1) / 2 + r];
    A[(size_t)h * bstride + (size_t)i * ld + R0 + e] = kv * b;
}

// k_hads_predvar with the draw as blockIdx.y: O = S M outputs per draw (k = s M + m), or O = S in the indexed form (k = s,
// m = istar[s]).  A value <= 0 is replaced by settings.precision (prediction.py:535-545, :659-669).
__global__ void k_psh_predvar(const double* __restrict__ star, const double* __restrict__ pars, long long P, int N,
                              const double* __restrict__ colsq, const int* __restrict__ istar, int S, int M,
                              double* __restrict__ var) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x, h = blockIdx.y;
    const int O = istar ? S : S * M;
    if (k >= O) return;
    const int s = istar ? k : k / M;
    const int mp = istar ? istar[s] : k % M;
    const double* Lvec = pars + (size_t)h * P + (size_t)2 * N;
    double b = 0.0;
    for (int r = 0; r <= mp; ++r) {
        const double v = Lvec[mp * (mp + 1) / 2 + r];
        b += v * v;
    }
    const double ss = exp(star[((size_t)h * S + s) * 2 + 1]);
    const double kss = NMGP_JITTER + ss * ss;
    double v = (b * kss - colsq[(size_t)h * O + k]) + exp(pars[(size_t)h * P + (P - 1)]);
    if (v <= 0.0) v = NMGP_PRECISION;
    var[(size_t)h * O + k] = v;
}

// hooks of the separable Hadamard model into the shared schedule (nmgp_predsample_common.h)
struct PsHads : PsHadamard {
    static size_t P(int N, int T) { return 2 * (size_t)N + T + 1; }
    static int star_width(int) { return 2; }
    template <class Take>
    static void extras(PsCall& k, Take take, size_t B) {
        k.o_ell = take(B * k.N);
        k.o_sig = take(B * k.N);
        k.o_Rv = take(B * k.N * k.M);
    }
    static int prep(const PsCall& k) {
        nmgp_hads_prep(k.c->stream, k.pars, k.c->had_indx, k.N, k.M, k.at(k.o_ell), k.at(k.o_sig), k.at(k.o_Rv), k.Bc);
        return 0;
    }
    static int star(const PsCall& k) {
        pss_star(k.c->stream, k.W0, k.W1, k.cv0, k.cv1, k.pars, k.P, k.z, k.N, k.S, k.hyper[0], k.hyper[3], k.star, k.Bc);
        return 0;
    }
    static int build_cov(const PsCall& k) {
        return nmgp_hads_cov_build(k.c->stream, k.c->d_x, k.at(k.o_ell), k.at(k.o_sig), k.at(k.o_Rv), k.pars, k.P, k.Sb, k.ld, k.N, k.M,
                                   k.Bc, k.bs);
    }
    static int cross_rows(const PsCall& k) {
        const dim3 grid(k.N, cdiv(k.E, 256), k.Bc);
        NMGP_HADS_SWITCH(k.M, NMGP_LAUNCH((k_psh_cross_rows<MM>), grid, dim3(256), 0, k.c->stream, k.c->d_x, k.at(k.o_ell),
                                          k.at(k.o_sig), k.at(k.o_Rv), k.pars, k.P, k.N, k.xs, k.star, k.is, k.S, k.s0, k.E, k.Sb, k.ld,
                                          k.bs, k.N + 1));
        return 0;
    }
    static int finish(const PsCall& k) {
        const long long O = (long long)k.S * k.per;
        NMGP_LAUNCH(k_psh_predvar, dim3(cdiv(O, 256), k.Bc), dim3(256), 0, k.c->stream, k.star, k.pars, k.P, k.N, k.sqs, k.is, k.S, k.M,
                    k.var);
        return 0;
    }
};

}  // namespace

extern "C" int nmgp_predsample_hads(nmgp_ctx* c, const double* pars, int H, const double hyper[9], const double* xs,
                                    const int* indx_star, int S, const double* z, const double* star_in, double* mean, double* var,
                                    double* star_out, int* status) {
    return ps_predict<PsHads>(c, pars, H, hyper, xs, indx_star, S, 0, z, star_in, mean, var, star_out, status);
}

