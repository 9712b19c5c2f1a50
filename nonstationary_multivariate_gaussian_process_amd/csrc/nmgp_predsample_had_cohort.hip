// MAP and posterior-draw prediction for the cohort of ragged Hadamard subjects (nmgp_had_set_subjects, nmgp_hadamard_cohort.hip) under
// the three models: the entries nmgp_predsample_had_subjects (nonseparable), nmgp_predsample_hads_subjects (separable) and
// nmgp_predict_hadst_subjects (stationary), ONE host schedule hadc_predict<Model> and one struct of hooks per model (HcNon, HcSep,
// HcSta), as ps_predict<Model> (nmgp_predsample_common.h) has for the resident subject and cohm_subjects_eval<Model>
// (nmgp_hadamard_cohort_models.hip) for the cohort's evaluations.
//
// hadc_predict is ps_predict's schedule with the subject as a table look-up, written as a sibling: ps_predict and the resident kernels
// (k_psn_*, k_psh_*, k_hadst_*, k_pss_star) serve entries whose bits are pinned, so no table is threaded through them.  Subject s
// brings its own new inputs xs[s, 0 .. nstar[s]) of a padded [S, Smax] array.  Once per call and distinct (alpha, beta), for the
// models with a latent regression: k* of all subjects with exact zeros at padded observations and in padded input columns
// (k_hadc_kstar), the two prior_trsv passes with batch = S against the set's per-subject factors, the clipped conditional variances
// (k_hadc_condvar).  Per chunk of draws (whole subjects, or a part of ONE subject's draws: no kernel takes a draw offset): the model's
// unpacking, the starred values, per slice of new inputs {masked covariance, y and the riding cross-covariance rows, batched
// nmgp_potrf with precise panels, ps_rows_reduce}, the variance, the downloads, ONE synchronisation.  The kernels keep their resident
// originals' lane mapping and expression order (a subject with N_s = Nmax and nstar = Smax gets their bits) and take subject =
// draw / draws-per-subject of the chunk; every mask comes from the nobs and nstar tables, never from the contents of a padded slot,
// and every sum has a fixed order.  What is masked, per model:
//   nonseparable  the regression sums of the 1 + T curves (k_hadc_star), the riding rows (k_hadc_cross_rows), mean / var of a padded
//                 input (k_hadc_predvar); the covariance is hadc_cov_build<false> behind k_hadc_prep
//   separable     the regression sums of the two curves at pars + c Nmax (k_hadcs_star), the riding rows with L_vec at pars + 2 Nmax
//                 (k_hadcs_cross_rows), mean / var of a padded input (k_hadcs_predvar); hadc_cov_build<true> behind k_hadcs_prep
//   stationary    the riding rows (k_hadcst_cross_rows: the set's labels are zero-padded, so an unmasked row would take B_f[m, 0] at a
//                 padded observation), mean / var of a padded input (k_hadcst_predvar); k_hadcst_cov; no regression, no prior factor
#include "nmgp_hadamard_common.h"
#include "nmgp_predsample_common.h"

#include <algorithm>

using namespace nmgpk;

namespace {

inline unsigned cdiv(long long a, long long b) { return (unsigned)((a + b - 1) / b); }

// ---- nonseparable (and the projections every model with a latent regression shares) ------------------------------------------------------
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

// ---- separable ------------------------------------------------------------------------------------------------------------------------

// k_pss_star with subject = draw / cps: slot c = blockIdx.y (0: tilde_l*, 1: tilde_sigma*), the curve at pars + c Nmax, the sum over
// the subject's real observations (the padded parameter slots are not read), +0.0 for a padded new input (z is not read there).
// W0 / W1: [S, Smax, N]; cv0 / cv1: [S, Smax]; star, z: [B, Smax, 2].
__global__ __launch_bounds__(256) void k_hadcs_star(const double* __restrict__ W0, const double* __restrict__ W1,
                                                     const double* __restrict__ cv0, const double* __restrict__ cv1,
                                                     const double* __restrict__ pars, long long P, const double* __restrict__ z,
                                                     const int* __restrict__ nobs, const int* __restrict__ nstar, int cps, int N, int S,
                                                     double mu_l, double mu_s, double* __restrict__ star) {
    __shared__ double sh[256];
    const int s = blockIdx.x, cidx = blockIdx.y, h = blockIdx.z;
    const int sub = h / cps;
    const size_t o = ((size_t)h * S + s) * 2 + cidx;
    if (s >= nstar[sub]) {
        if (threadIdx.x == 0) star[o] = 0.0;
        return;
    }
    const int Ns = nobs[sub];
    const size_t ws = (size_t)sub * S + s;
    const double* p = pars + (size_t)h * P + (size_t)cidx * N;
    const double* W = (cidx == 0 ? W0 : W1) + ws * N;
    const double mu = cidx == 0 ? mu_l : mu_s;
    double acc = 0.0;
    for (int i = threadIdx.x; i < Ns; i += 256) acc += W[i] * (p[i] - mu);
    acc = block_sum_256(acc, sh);
    if (threadIdx.x != 0) return;
    double v = mu + acc;
    if (z) v = v + sqrt((cidx == 0 ? cv0 : cv1)[ws]) * z[o];
    star[o] = v;
}

// k_psh_cross_rows<M> with subject = draw / cps: riding row R0 + e below the matrix of draw h = blockIdx.z, observation
// i = blockIdx.x; lanes along the riding-row index.  Exact zero for a padded observation or a padded new input (whose x, label and
// starred values are not read).  istar: [S_set, S] labels, nullptr in the full form.
template <int M>
__global__ __launch_bounds__(256) void k_hadcs_cross_rows(const double* __restrict__ x, const double* __restrict__ ell,
                                                           const double* __restrict__ sig, const double* __restrict__ Rv,
                                                           const double* __restrict__ pars, long long P,
                                                           const int* __restrict__ nobs, const int* __restrict__ nstar, int cps, int N,
                                                           const double* __restrict__ xs, const double* __restrict__ star,
                                                           const int* __restrict__ istar, int S, int s0, int E,
                                                           double* __restrict__ A, int ld, long long bstride, int R0) {
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
    const double* st = star + ((size_t)h * S + s) * 2;
    const double* Lvec = pars + (size_t)h * P + (size_t)2 * N;
    const double* ri = Rv + ((size_t)h * N + i) * M;
    const double xi = x[(size_t)sub * N + i], li = ell[(size_t)h * N + i];
    const double xj = xs[(size_t)sub * S + s], lj = exp(st[0]), sj = exp(st[1]);
    const double dist = (xi * xi + xj * xj) - 2.0 * (xi * xj);
    const double Aij = li * li + lj * lj;
    const double kv = (sig[(size_t)h * N + i] * sj) * sqrt(2.0 * (li * lj) / Aij) * exp(-dist / Aij);
    double b = 0.0;
    for (int r = 0; r <= mp; ++r) b += ri[r] * Lvec[mp * (mp + 1) / 2 + r];
    *out = kv * b;
}

// k_psh_predvar with subject = draw / cps; a padded new input gets +0.0 in var AND in mean (the slices past the chunk's largest
// nstar are not factorised, so nothing else writes those slots).
__global__ void k_hadcs_predvar(const double* __restrict__ star, const double* __restrict__ pars, long long P, int N,
                                const double* __restrict__ colsq, const int* __restrict__ istar, const int* __restrict__ nstar, int cps,
                                int S, int M, double* __restrict__ mean, double* __restrict__ var) {
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

// ---- stationary -----------------------------------------------------------------------------------------------------------------------

// k_hadst_cross_rows<M> with subject = draw / cps: x and the label of observation i = blockIdx.x at sub Nmax + i, u = x / l in that
// order, B_f[m, c_i] staged per block as there.  Exact zero for a padded observation (uniform over the block: nothing of it is read,
// its zero-padded label included) or a padded new input.
template <int M>
__global__ __launch_bounds__(256) void k_hadcst_cross_rows(const double* __restrict__ x, const int* __restrict__ indx,
                                                            const double* __restrict__ pars, long long P,
                                                            const int* __restrict__ nobs, const int* __restrict__ nstar, int cps, int N,
                                                            const double* __restrict__ xs, const int* __restrict__ istar, int S, int s0,
                                                            int E, double* __restrict__ A, int ld, long long bstride, int R0) {
    __shared__ double sBc[M], sp[2];             // sp = {l, s2}
    const int i = blockIdx.x, h = blockIdx.z;
    const int sub = h / cps;
    const bool real = i < nobs[sub];
    pars += (size_t)h * P;
    if (real) {
        if (threadIdx.x == 0) {
            const double sg = exp(pars[1]);
            sp[0] = exp(pars[0]);
            sp[1] = sg * sg;
        } else if (threadIdx.x - 64 < (unsigned)M) {
            sBc[threadIdx.x - 64] = hadst_bf<M>(pars + 2, threadIdx.x - 64, indx[(size_t)sub * N + i]);     // B_f[m, c_i]
        }
    }
    __syncthreads();
    const int e = blockIdx.y * 256 + threadIdx.x;
    if (e >= E) return;
    const int s = istar ? s0 + e : s0 + e / M;
    double* out = A + (size_t)h * bstride + (size_t)i * ld + R0 + e;
    if (!real || s >= nstar[sub]) {
        *out = 0.0;
        return;
    }
    const int mp = istar ? istar[(size_t)sub * S + s] : e % M;
    const double ui = x[(size_t)sub * N + i] / sp[0], uj = xs[(size_t)sub * S + s] / sp[0];
    const double dist = (ui * ui + uj * uj) - 2.0 * (ui * uj);
    *out = sBc[mp] * (exp(-0.5 * dist) * sp[1]);
}

// k_hadst_predvar with subject = draw / cps; +0.0 in var AND in mean for a padded new input
__global__ void k_hadcst_predvar(const double* __restrict__ pars, long long P, const double* __restrict__ colsq,
                                 const int* __restrict__ istar, const int* __restrict__ nstar, int cps, int S, int M,
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

// ---- host -----------------------------------------------------------------------------------------------------------------------------

// what a model hook sees of a call; the chunk (nb, cps and the table slices of its first subject) and slice (j0, E) fields follow the
// loops.  Draw z of a chunk belongs to subject z / cps of the slices.
struct HcCall {
    nmgp_ctx* c;
    const double* hyper;
    int N, M, T, Smax;               // N = the set's Nmax
    long long P;
    int ld;
    long long bs;                    // stride between matrices
    int nb, cps, j0, E;
    const double *x, *xs;            // [nsub, Nmax], [nsub, Smax]
    const int *indx, *nobs, *ns, *is;        // is: the labels of the new inputs, nullptr in the full form
    double* w;                       // workspace base; pieces absent from a call are nullptr
    double *W0, *W1, *cv0, *cv1;     // the chunk's first subject's rows of the projections
    double *pars, *star, *z, *mean, *sqs, *var, *Sb;
    size_t o_ell, o_sig, o_Rv;       // Model::extras
    double* at(size_t o) const { return w + o; }
};

// The three models as the schedule sees them, structs of static members, nothing virtual:
//   NAME                      the entry, for the refusals
//   P(N, T)                   length of a (padded) parameter vector
//   star_width(T)             starred values per draw and input (0: no latent regression, no hyper, star_out not written)
//   extras(k, take, B)        the model's own pieces of the workspace
//   finite_in(p, N, N_s, T)   whether the REAL slots of a padded vector are finite (nmgp_hadamard_common.h)
//   prep / star / build_cov / cross_rows / finish (k)   hooks: unpacking and starred values of a chunk, covariance and riding rows of
//                             a slice, variance (and the +0.0 of padded inputs) of a chunk
struct HcNon {
    static constexpr const char* NAME = "nmgp_predsample_had_subjects";
    static size_t P(int N, int T) { return (size_t)N * (1 + T) + 1; }
    static int star_width(int T) { return 1 + T; }
    template <class Take>
    static void extras(HcCall& k, Take take, size_t B) {
        k.o_ell = take(B * k.N);
        k.o_Rv = take(B * k.N * k.M);
    }
    static bool finite_in(const double* p, size_t N, size_t Ns, int T) { return hadc_finite_non(p, N, Ns, T); }
    static void prep(const HcCall& k) {
        nmgp_hadc_prep(k.c->stream, k.pars, k.indx, k.nobs, k.cps, k.N, k.M, k.T, k.at(k.o_ell), k.at(k.o_Rv), k.nb);
    }
    static void star(const HcCall& k) {
        NMGP_LAUNCH(k_hadc_star, dim3(k.Smax, 1 + k.T, k.nb), dim3(256), 0, k.c->stream, k.W0, k.W1, k.cv0, k.cv1, k.pars, k.P, k.z,
                    k.nobs, k.ns, k.cps, k.N, k.T, k.Smax, k.hyper[0], k.hyper[3], k.star);
    }
    static int build_cov(const HcCall& k) {
        return hadc_cov_build<false>(k.c->stream, k.x, k.at(k.o_ell), nullptr, k.at(k.o_Rv), k.pars, k.P, k.nobs, k.cps, k.Sb, k.ld, k.N,
                                     k.M, k.nb, k.bs);
    }
    static int cross_rows(const HcCall& k) {
        const dim3 grid(k.N, cdiv(k.E, 256), k.nb);
        NMGP_HADS_SWITCH(k.M, NMGP_LAUNCH((k_hadc_cross_rows<MM>), grid, dim3(256), 0, k.c->stream, k.x, k.at(k.o_ell), k.at(k.o_Rv),
                                          k.nobs, k.ns, k.cps, k.N, k.xs, k.star, k.is, k.Smax, k.j0, k.E, k.Sb, k.ld, k.bs, k.N + 1));
        return 0;
    }
    static void finish(const HcCall& k, long long O) {
        NMGP_LAUNCH(k_hadc_predvar, dim3(cdiv(O, 256), k.nb), dim3(256), 0, k.c->stream, k.star, k.pars, k.P, k.sqs, k.is, k.ns, k.cps,
                    k.Smax, k.M, k.T, k.mean, k.var);
    }
};

struct HcSep {
    static constexpr const char* NAME = "nmgp_predsample_hads_subjects";
    static size_t P(int N, int T) { return 2 * (size_t)N + T + 1; }
    static int star_width(int) { return 2; }
    template <class Take>
    static void extras(HcCall& k, Take take, size_t B) {
        k.o_ell = take(B * k.N);
        k.o_sig = take(B * k.N);
        k.o_Rv = take(B * k.N * k.M);
    }
    static bool finite_in(const double* p, size_t N, size_t Ns, int T) { return hadc_finite_sep(p, N, Ns, T); }
    static void prep(const HcCall& k) {
        nmgp_hadcs_prep(k.c->stream, k.pars, k.indx, k.nobs, k.cps, k.N, k.M, k.T, k.at(k.o_ell), k.at(k.o_sig), k.at(k.o_Rv), k.nb);
    }
    static void star(const HcCall& k) {
        NMGP_LAUNCH(k_hadcs_star, dim3(k.Smax, 2, k.nb), dim3(256), 0, k.c->stream, k.W0, k.W1, k.cv0, k.cv1, k.pars, k.P, k.z, k.nobs,
                    k.ns, k.cps, k.N, k.Smax, k.hyper[0], k.hyper[3], k.star);
    }
    static int build_cov(const HcCall& k) {
        return hadc_cov_build<true>(k.c->stream, k.x, k.at(k.o_ell), k.at(k.o_sig), k.at(k.o_Rv), k.pars, k.P, k.nobs, k.cps, k.Sb, k.ld,
                                    k.N, k.M, k.nb, k.bs);
    }
    static int cross_rows(const HcCall& k) {
        const dim3 grid(k.N, cdiv(k.E, 256), k.nb);
        NMGP_HADS_SWITCH(k.M, NMGP_LAUNCH((k_hadcs_cross_rows<MM>), grid, dim3(256), 0, k.c->stream, k.x, k.at(k.o_ell), k.at(k.o_sig),
                                          k.at(k.o_Rv), k.pars, k.P, k.nobs, k.ns, k.cps, k.N, k.xs, k.star, k.is, k.Smax, k.j0, k.E,
                                          k.Sb, k.ld, k.bs, k.N + 1));
        return 0;
    }
    static void finish(const HcCall& k, long long O) {
        NMGP_LAUNCH(k_hadcs_predvar, dim3(cdiv(O, 256), k.nb), dim3(256), 0, k.c->stream, k.star, k.pars, k.P, k.N, k.sqs, k.is, k.ns,
                    k.cps, k.Smax, k.M, k.mean, k.var);
    }
};

struct HcSta {
    static constexpr const char* NAME = "nmgp_predict_hadst_subjects";
    static size_t P(int, int T) { return (size_t)T + 3; }
    static int star_width(int) { return 0; }
    template <class Take>
    static void extras(HcCall&, Take, size_t) {}
    static bool finite_in(const double* p, size_t N, size_t Ns, int T) { return hadc_finite_sta(p, N, Ns, T); }
    static void prep(const HcCall&) {}
    static void star(const HcCall&) {}
    static int build_cov(const HcCall& k) {
        return nmgp_hadcst_cov_build(k.c->stream, k.x, k.indx, k.pars, k.P, k.nobs, k.cps, k.Sb, k.ld, k.N, k.M, k.nb, k.bs);
    }
    static int cross_rows(const HcCall& k) {
        const dim3 grid(k.N, cdiv(k.E, 256), k.nb);
        NMGP_HADS_SWITCH(k.M, NMGP_LAUNCH((k_hadcst_cross_rows<MM>), grid, dim3(256), 0, k.c->stream, k.x, k.indx, k.pars, k.P, k.nobs,
                                          k.ns, k.cps, k.N, k.xs, k.is, k.Smax, k.j0, k.E, k.Sb, k.ld, k.bs, k.N + 1));
        return 0;
    }
    static void finish(const HcCall& k, long long O) {
        NMGP_LAUNCH(k_hadcst_predvar, dim3(cdiv(O, 256), k.nb), dim3(256), 0, k.c->stream, k.pars, k.P, k.sqs, k.is, k.ns, k.cps, k.Smax,
                    k.M, k.mean, k.var);
    }
};

// B = S * draws_per_subject parameter vectors of the set -> predictive means and variances at each subject's own new inputs: argument
// checks -> host tables of the new inputs -> slice and chunk sizes -> one workspace carved out of ctx->ps_buf -> the two priors
// projected once per call -> per chunk {upload, unpack, starred values, per slice {covariance, y and the riding rows, batched
// nmgp_potrf, ps_rows_reduce}, variance, downloads, ONE synchronisation, status}.
template <class Model>
int hadc_predict(nmgp_ctx* c, const double* pars, int B, int draws_per_subject, const double* hyper, const double* xs,
                 const int* indx_star, const int* nstar, int Smax, const double* z, const double* star_in, double* mean, double* var,
                 double* star_out, int* status) {
    if (!c) return NMGP_E_NULL;
    const int SW = Model::star_width(c->hc_T);
    if (!pars || (SW && !hyper) || !xs || !mean || !var) return nmgp_fail(c, NMGP_E_NULL, "pars/hyper/xs/mean/var must not be NULL");
    if (c->hc_S <= 0) return nmgp_fail(c, NMGP_E_STATE, "nmgp_had_set_subjects must be called first");
    if (z && star_in) return nmgp_fail(c, NMGP_E_STATE, "with star_in given the regression is skipped: z must be NULL");
    if (c->chol_algo != 1)
        return nmgp_fail(c, NMGP_E_UNSUPPORTED, "the Hadamard entries run on the custom factorisation only (riding rows)");
    const int S = c->hc_S, N = c->hc_Nmax, M = c->hc_M, T = c->hc_T, H = draws_per_subject;
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
            return nmgp_fail(c, NMGP_E_SHAPE, "%s: nstar[%d] = %d is outside [0, Smax = %d]", Model::NAME, s, ns, Smax);
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
    HcCall k{};
    k.c = c, k.hyper = hyper, k.N = N, k.M = M, k.T = T, k.Smax = Smax;
    const size_t P = Model::P(N, T);
    k.P = (long long)P;
    const int per = PsHadamard::rows(M, indexed);
    // riding rows per factorisation: the resident entries' rule at Nmax
    const int smax = PsHadamard::smax(N, M, indexed);
    const int Emax = std::min(Smax, smax) * per;
    const int ld = k.ld = (int)nmgp_ld((size_t)N + 1 + Emax);
    const long long bs = k.bs = (long long)ld * N;
    if (bs >= 0x7fffffffLL)
        return nmgp_fail(c, NMGP_E_SHAPE, "a matrix of order Nmax = %d with %d riding rows exceeds the 2^31 elements the row kernels index",
                         N, ld - N);
    const int chunks = (N + 127) / 128;
    // a chunk is a whole number of subjects, or a part of ONE subject's draws (then every draw of the chunk is that subject's)
    int Bc = nmgp_ps_chunk(B, (size_t)(N + 1 + Emax) * ld);
    const bool split = H > Bc;
    if (!split) Bc = (Bc / H) * H;
    const size_t SC = (size_t)Smax * SW, O = (size_t)Smax * per, Bs = Bc, SS = (size_t)S * Smax;

    const bool regress = SW && !star_in;
    PriorFactor *p0 = nullptr, *p1 = nullptr;
    if (regress) NMGP_TRY(nmgp_hadc_priors(c, hyper, &p0, &p1));
    const bool same = p0 == p1;
    size_t off = 0;
    auto take = [&off](size_t nelem) {
        const size_t o = off;
        off += (nelem + 15) / 16 * 16;
        return o;
    };
    const size_t o_xs = take(SS), o_is = take(indexed ? (SS + 1) / 2 : 0), o_ns = take(((size_t)S + 1) / 2),
                 o_W0 = take(regress ? SS * N : 0), o_W1 = take(regress && !same ? SS * N : 0), o_cv = take(regress ? 2 * SS : 0),
                 o_pars = take(Bs * P);
    Model::extras(k, take, Bs);
    const size_t o_star = take(Bs * SC), o_z = take(z ? Bs * SC : 0), o_mean = take(Bs * O), o_sqs = take(Bs * O), o_var = take(Bs * O),
                 o_part = take(Bs * 2 * Emax * chunks), o_info = take((Bs + 1) / 2), o_S = take(Bs * bs);
    if (c->ps_cap < off) {
        c->ps_cap = 0;
        NMGP_TRY(nmgp_dev_alloc(c, &c->ps_buf, off));
        c->ps_cap = off;
    } else if (nmgp_poison()) {
        HIP_TRY(c, hipMemsetAsync(c->ps_buf, 0xFF, off * sizeof(double), st));
    }
    double* w = k.w = c->ps_buf;
    double *d_xs = w + o_xs, *W0 = w + o_W0, *W1 = same ? W0 : w + o_W1, *cv0 = w + o_cv, *cv1 = same ? cv0 : cv0 + SS;
    k.pars = w + o_pars, k.star = SW ? w + o_star : nullptr, k.z = z ? w + o_z : nullptr;
    k.mean = w + o_mean, k.sqs = w + o_sqs, k.var = w + o_var, k.Sb = w + o_S;
    double* part = w + o_part;
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
        k.nb = nb, k.cps = cps;
        // the tables of the chunk's first subject
        k.x = c->hc_x + (size_t)s0 * N;
        k.indx = c->hc_indx + (size_t)s0 * N;
        k.nobs = c->hc_nobs + s0;
        k.ns = d_ns + s0;
        k.xs = d_xs + (size_t)s0 * Smax;
        k.is = indexed ? d_is + (size_t)s0 * Smax : nullptr;
        if (regress) {
            const size_t wo = (size_t)s0 * Smax;
            k.W0 = W0 + wo * N, k.W1 = W1 + wo * N, k.cv0 = cv0 + wo, k.cv1 = cv1 + wo;
        }
        const double* y = c->hc_y + (size_t)s0 * N;
        const double* hp = pars + (size_t)b0 * P;
        const int Sreal = *std::max_element(hns.begin() + s0, hns.begin() + s0 + nsub);   // slices past it hold padded inputs only
        HIP_TRY(c, hipMemcpyAsync(k.pars, hp, (size_t)nb * P * sizeof(double), hipMemcpyHostToDevice, st));
        Model::prep(k);
        if (regress) {
            if (z) HIP_TRY(c, hipMemcpyAsync(k.z, z + (size_t)b0 * SC, nb * SC * sizeof(double), hipMemcpyHostToDevice, st));
            NmgpStage sp(c, NMGP_STAGE_PRIOR);
            Model::star(k);
        } else if (SW) {
            HIP_TRY(c, hipMemcpyAsync(k.star, star_in + (size_t)b0 * SC, nb * SC * sizeof(double), hipMemcpyHostToDevice, st));
            NMGP_LAUNCH(k_hadc_star_mask, dim3(cdiv((long long)SC, 256), nb), dim3(256), 0, st, k.ns, cps, Smax, SW, k.star);
        }
        HIP_TRY(c, hipMemsetAsync(d_info, 0, (size_t)nb * sizeof(int), st));
        for (int j0 = 0; j0 < Sreal; j0 += smax) {
            const int Sc = std::min(smax, Smax - j0), E = Sc * per;
            k.j0 = j0, k.E = E;
            {
                NmgpStage sp(c, NMGP_STAGE_COV);
                int r = Model::build_cov(k);
                if (r) return nmgp_fail(c, r, "unsupported number of outputs M=%d", M);
                set_row(st, k.Sb, ld, N, y, N, nb, bs, N, cps);             // the subject's y (zero-padded at set time) rides as row Nmax
                NMGP_TRY(Model::cross_rows(k));                             // ... and the slice's E cross-covariance rows below it
            }
            {
                NmgpStage sp(c, NMGP_STAGE_CHOL);
                nmgp_potrf(c, k.Sb, ld, N, 1 + E, 0, d_info, nb, bs, 1, 1);
            }
            NmgpStage sp(c, NMGP_STAGE_REDUCE);
            ps_rows_reduce(st, k.Sb, ld, bs, N, N + 1, N, E, part, nb, k.mean, k.sqs, (long long)O, (long long)j0 * per);
        }
        Model::finish(k, (long long)O);
        double* hm = mean + (size_t)b0 * O;
        double* hv = var + (size_t)b0 * O;
        HIP_TRY(c, hipMemcpyAsync(hm, k.mean, nb * O * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipMemcpyAsync(hv, k.var, nb * O * sizeof(double), hipMemcpyDeviceToHost, st));
        if (star_out && SW)
            HIP_TRY(c, hipMemcpyAsync(star_out + (size_t)b0 * SC, k.star, nb * SC * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipMemcpyAsync(hinfo.data(), d_info, (size_t)nb * sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));          // the one synchronisation of the chunk
        NMGP_TRY(nmgp_take_launch_error(c));
        for (int b = 0; b < nb; ++b) {
            int stt = hinfo[b];
            const int sub = s0 + b / cps;
            // the finiteness tests cover the row's REAL parameter slots and REAL outputs only
            const size_t Or = (size_t)hns[sub] * per;
            if (!Model::finite_in(hp + (size_t)b * P, (size_t)N, (size_t)c->hc_nobs_h[sub], T)) stt = NMGP_NUM_NAN;
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

}  // namespace

extern "C" int nmgp_predsample_had_subjects(nmgp_ctx* c, const double* pars, int B, int draws_per_subject, const double hyper[8],
                                            const double* xs, const int* indx_star, const int* nstar, int Smax, const double* z,
                                            const double* star_in, double* mean, double* var, double* star_out, int* status) {
    return hadc_predict<HcNon>(c, pars, B, draws_per_subject, hyper, xs, indx_star, nstar, Smax, z, star_in, mean, var, star_out, status);
}

extern "C" int nmgp_predsample_hads_subjects(nmgp_ctx* c, const double* pars, int B, int draws_per_subject, const double hyper[9],
                                             const double* xs, const int* indx_star, const int* nstar, int Smax, const double* z,
                                             const double* star_in, double* mean, double* var, double* star_out, int* status) {
    return hadc_predict<HcSep>(c, pars, B, draws_per_subject, hyper, xs, indx_star, nstar, Smax, z, star_in, mean, var, star_out, status);
}

extern "C" int nmgp_predict_hadst_subjects(nmgp_ctx* c, const double* pars, int B, int draws_per_subject, const double* xs,
                                           const int* indx_star, const int* nstar, int Smax, double* mean, double* var, int* status) {
    return hadc_predict<HcSta>(c, pars, B, draws_per_subject, nullptr, xs, indx_star, nstar, Smax, nullptr, nullptr, mean, var, nullptr,
                               status);
}
