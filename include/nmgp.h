/*
 * nmgp.h -- C ABI of libnmgp_hip.so: the MI355X (gfx950) implementation of the multi-output
 * Gaussian-process log-posterior path of Corleno/Nonstationary_Multivariate_Gaussian_Process.
 *
 * The reference has no FFI layer: its boundary is a set of Python module functions
 * (Utility/{kernels,kronecker_operation,distributions,logpos}.py).  Every entry point below names the
 * reference function (file:line under the reference tree) whose arithmetic it replaces; the Python
 * package `nonstationary_multivariate_gaussian_process_amd.Utility` binds these symbols with ctypes
 * behind the reference's own signatures (INTEGRATION.md shows the binding).
 *
 * Conventions
 *   - plain C, no torch / HIP types in any signature; all scalars are double / int / long long.
 *   - unless a name ends in `_dev`, array arguments are caller-owned HOST buffers, float64,
 *     C-contiguous (row-major); the library copies in/out and owns all device memory.
 *   - return value: 0 success; <0 API misuse (NMGP_E_*); >0 numerical failure:
 *       k in [1, 1<<20)  : Cholesky failed, leading minor k not positive definite (rocSOLVER info)
 *       NMGP_NUM_NAN     : a NaN/Inf reached the result
 *       NMGP_NUM_EIG     : eigensolver did not converge
 *     nmgp_last_error(ctx) returns a human readable message for the last non-zero return.
 *   - a context is bound to one GPU and one HIP stream and is NOT thread-safe; use one per host thread.
 *   - layouts follow the reference: Y is [N,M] row-major, the stacked observation vector is
 *     output-major y[m*N+i] = Y[i,m] (logpos.py:338); the nonseparable parameter vector is
 *     [tilde_l (N) | uL_vecs (N*T, location-major, tril row-major slots) | tilde_sigma2_err]
 *     (logpos.py:32-43), the separable one [tilde_l (N) | tilde_sigma (N) | uL_vec (T) | tilde_sigma2_err]
 *     (logpos.py:17-29), the stationary one [tilde_l, tilde_sigma, uL_vec (T), tilde_sigma2_err]
 *     (logpos.py:46-57); T = M(M+1)/2.
 */
#ifndef NMGP_H
#define NMGP_H

#ifdef __cplusplus
extern "C" {
#endif

#define NMGP_VERSION 100

/* API-misuse codes */
#define NMGP_E_NULL        (-1)   /* required pointer is NULL */
#define NMGP_E_SHAPE       (-2)   /* non-positive or inconsistent dimension */
#define NMGP_E_STATE       (-3)   /* call order violated (e.g. eval before nmgp_set_data) */
#define NMGP_E_UNSUPPORTED (-4)   /* M larger than NMGP_MAX_OUTPUTS, etc. */
#define NMGP_E_HIP         (-5)   /* HIP / rocBLAS / rocSOLVER runtime error (see nmgp_last_error) */
#define NMGP_E_NOMEM       (-6)
/* numerical-failure codes (positive) */
#define NMGP_NUM_NAN       (1 << 20)
#define NMGP_NUM_EIG       ((1 << 20) + 1)

#define NMGP_MAX_OUTPUTS 8

typedef struct nmgp_ctx nmgp_ctx;

/* ---- context ------------------------------------------------------------------------------- */
/* device = HIP device ordinal. */
int nmgp_ctx_create(int device, nmgp_ctx** out);
int nmgp_ctx_destroy(nmgp_ctx* ctx);
const char* nmgp_last_error(const nmgp_ctx* ctx);
int nmgp_version(void);
/* SHA-256 (hex) of the sources, headers and code-generation flags the library was built from (build.py: tree_id()).
 * The Python binding refuses a shared object whose id differs from the source tree beside it. */
const char* nmgp_build_id(void);
/* Blocks until all work queued on the context's stream is complete. */
int nmgp_sync(nmgp_ctx* ctx);
/* Number of visible HIP devices (does not create a context). */
int nmgp_device_count(void);

/* ---- data residency ------------------------------------------------------------------------ */
/* Upload one subject's inputs (x: [N], Y: [N,M] row-major) and size all workspaces.  Replaces the
 * per-call tensor plumbing of logpos.py:337-338.  May be called again with another subject. */
int nmgp_set_data(nmgp_ctx* ctx, const double* x, const double* Y, int N, int M);

/* ---- Hadamard form of the nonseparable model: irregularly observed outputs --------------------
 * logpos.nlogpos_obj_hadamard_SVC / logpos_hadamard_SVC (logpos.py:566-659), prediction.point_predmap_SVC_hadamard /
 * pointwise_predmap_SVC_hadamard (prediction.py:1401-1478).  The data are N single observations (x[i], indx[i], y[i]), indx[i] in
 * [0, M) naming the output measured at x[i].  pars = [tilde_l (N) | L_vecs (N*T, row-major per observation) | tilde_sigma2_err],
 * P = N(1+T)+1; the L_vecs slots are taken as they are (no exp) and only row indx[i] of L_i reaches the likelihood.
 *
 * nmgp_had_set_data makes the Hadamard subject the resident one: NMGP_E_SHAPE unless every label is in [0, M) and every label
 * occurs.  The complete-data entries then return NMGP_E_STATE until nmgp_set_data is called again, and the entries below return
 * NMGP_E_STATE while a complete-data subject (or none) is resident. */
int nmgp_had_set_data(nmgp_ctx* ctx, const double* x, const int* indx, const double* y, int N, int M);
/* B parameter vectors pars [B, P] in one launch sequence (one synchronisation per chunk of chains; chunks keep the entry's own
 * device workspace below NMGP_HAD_BATCH_SLAB_GB, default 96).  hyper[8] as for nmgp_logpos_svc.  out5 [B, 5] = the verbose tuples
 * (NegLog, loglik, log_prior_tilde_l, log_prior_L_vecs, log_prior_sigma2_err); grad [B, P] = d NegLog / d pars, or NULL;
 * status [B]: 0, k > 0 (leading minor k of the chain's covariance is not positive definite) or NMGP_NUM_NAN (a non-finite
 * parameter or result).  A failing chain has a NaN row in out5 and a zero row in grad; the call still returns 0. */
int nmgp_had_batch_eval(nmgp_ctx* ctx, const double* pars, int B, const double hyper[8], int prior, double* out5, double* grad,
                        int* status);
/* out [N, N]: the full symmetric covariance K_x o (R R^T) + sigma2 I of one parameter vector. */
int nmgp_had_covariance(nmgp_ctx* ctx, const double* pars, double* out);
/* MAP prediction of all M outputs at the new inputs xs [S]: mean, var [S, M] (a variance <= 0 is replaced by 1e-6);
 * star [S, 1+T] = the regressed tilde_l* and the T slots of L* (no exp), or NULL. */
int nmgp_predict_had(nmgp_ctx* ctx, const double* pars, const double hyper[8], const double* xs, int S, double* mean, double* var,
                     double* star);

/* A cohort of S Hadamard subjects of RAGGED size per launch sequence.  Every subject is padded to the set's Nmax with decoupled
 * unit observations (row / column of the identity in the covariance and in both GP-prior covariances, y = 0): the padded part of
 * every factor is the identity, and log det, the quadratic form, the prior terms and their log-determinants gain exact zeros.
 *   x, indx, y [S, Nmax] row-major: only the first nobs[s] entries of row s are read (the rest may hold anything).
 * NMGP_E_SHAPE unless S >= 1, 1 <= M <= 8, 1 <= Nmax <= 3500 (every GP-prior solve of the set is by substitution),
 * M <= nobs[s] <= Nmax, every real label in [0, M) and every label occurring in every subject.  The set is independent of the
 * resident subject: it needs none, survives nmgp_set_data / nmgp_had_set_data, carries its own Nmax and M, and no other entry
 * sees it.  It ends with nmgp_had_clear_subjects, a second nmgp_had_set_subjects, or the context; its per-subject GP-prior factors
 * (one batched factorisation per (alpha, beta)) are cached with it. */
int nmgp_had_set_subjects(nmgp_ctx* ctx, const double* x, const int* indx, const double* y, const int* nobs, int S, int Nmax, int M);
int nmgp_had_clear_subjects(nmgp_ctx* ctx);
/* B = S * chains_per_subject rows (NMGP_E_SHAPE otherwise); row s * chains_per_subject + k is chain k of subject s.
 * pars [B, Pmax], Pmax = Nmax (1 + T) + 1, the PADDED layout [tilde_l (Nmax) | L_vecs (Nmax * T) | tilde_sigma2_err]: subject s's
 * vector of length nobs[s] (1 + T) + 1 occupies the first nobs[s] entries (nobs[s] * T for L_vecs) of each block and the last slot.
 * Padded slots are never read (a NaN there changes nothing, and the NMGP_NUM_NAN test covers the real slots only); their gradient is
 * +0.0.  out5 [B, 5], grad [B, Pmax] or NULL and status [B] as for nmgp_had_batch_eval; a status k > 0 is a leading minor inside
 * the subject's own nobs[s].  Chunks under NMGP_HAD_BATCH_SLAB_GB are whole subjects or parts of one subject's chains; one
 * synchronisation per chunk; a chain's bits depend neither on the chunking nor on the other subjects of the set.
 * NMGP_E_STATE without a set, NMGP_E_UNSUPPORTED under NMGP_CHOL=rocsolver. */
int nmgp_had_subjects_eval(nmgp_ctx* ctx, const double* pars, int B, int chains_per_subject, const double hyper[8], int prior,
                           double* out5, double* grad, int* status);
/* MAP and posterior-draw prediction for the set: B = S * draws_per_subject rows (row s * draws_per_subject + h is draw h of
 * subject s; pars [B, Pmax] in the padded layout above) at each subject's OWN new inputs, nmgp_predsample_had's schedule with the
 * subject as a table look-up and its conventions for z / star_in / star_out (slot 0 = tilde_l* before exp, slots 1 + t = the raw
 * slots of L*, ONE conditional variance per prior; z == NULL: the conditional means; star_in skips the regression, z must then be
 * NULL) and for the variance ((1 + 1e-6)(L* L*^T)_mm - |L^-1 k_f|^2 + exp(tilde_sigma2_err); a value <= 0 is replaced by 1e-6).
 *   xs [S, Smax]: only the first nstar[s] entries of row s are read; nstar == NULL: all Smax; 0 <= nstar[s] <= Smax.
 *   indx_star == NULL: all M outputs per input, mean / var [B, Smax, M]; indx_star [S, Smax]: output indx_star[s, j] only,
 *   mean / var [B, Smax] (only the labels of real slots are read and range-checked).  z, star_in, star_out: [B, Smax, 1 + T].
 * A padded new-input slot (j >= nstar[s]) gets +0.0 in mean, var and star_out, and nothing is read from xs, indx_star, z or
 * star_in there: every mask comes from the nstar and nobs tables.  status [B]: 0, a leading minor inside the subject's nobs[s], or
 * NMGP_NUM_NAN (the finiteness tests cover the row's real parameter slots and real outputs); a failing draw has NaN in every real
 * output slot of its row, its neighbours keep their bits, the call returns 0.  Chunks of draws (NMGP_PREDSAMPLE_CHUNK,
 * NMGP_PREDSAMPLE_SLAB_GB, read at every call) are whole subjects or parts of ONE subject's draws, one synchronisation each; a
 * row's bits depend neither on the chunking, nor on draws_per_subject, nor on the other subjects of the set, nor on the slice of
 * riding rows a new input falls into.  The set with its cached prior factors, the resident subject and a pending batched result
 * stay as they were.  NMGP_E_STATE without a set or with z and star_in both given; NMGP_E_SHAPE for B != S * draws_per_subject,
 * draws_per_subject < 1, Smax < 1, an nstar[s] outside [0, Smax] or a real label outside [0, M); NMGP_E_UNSUPPORTED under
 * NMGP_CHOL=rocsolver. */
int nmgp_predsample_had_subjects(nmgp_ctx* ctx, const double* pars, int B, int draws_per_subject, const double hyper[8],
                                 const double* xs, const int* indx_star, const int* nstar, int Smax, const double* z,
                                 const double* star_in, double* mean, double* var, double* star_out, int* status);

/* ---- Hadamard form of the separable model: one cross-output matrix shared by all observations ----
 * logpos.nlogpos_obj_hadamard / logpos_hadamard (logpos.py:465-563), prediction.point_predmap_hadamard / pointwise_predmap_hadmard
 * (prediction.py:710-808).  The subject is the one nmgp_had_set_data made resident (NMGP_E_STATE otherwise).
 * pars = [tilde_l (N) | tilde_sigma (N) | L_vec (T) | tilde_sigma2_err], P = 2N+T+1; the L_vec slots are taken as they are (no exp).
 * hyper[9] = {mu_tilde_l, alpha_tilde_l, beta_tilde_l, mu_tilde_sigma, alpha_tilde_sigma, beta_tilde_sigma, a, b, c}. */
/* B parameter vectors pars [B, P] in one launch sequence, chunked as nmgp_had_batch_eval.  out6 [B, 6] = the verbose tuples
 * (NegLog, loglik, log_prior_tilde_l, log_prior_tilde_sigma, log_prior_L_vec, log_prior_sigma2_err; the last is the UNNORMALISED
 * inverse gamma); grad [B, P] = d NegLog / d pars, or NULL; status [B] and the failure semantics as for nmgp_had_batch_eval: a
 * failing chain has a NaN row in out6 and a zero row in grad, and the call still returns 0. */
int nmgp_hads_batch_eval(nmgp_ctx* ctx, const double* pars, int B, const double hyper[9], int prior, double* out6, double* grad,
                         int* status);
/* out [N, N]: the full symmetric covariance K_x o (R R^T) + sigma2 I of one parameter vector. */
int nmgp_hads_covariance(nmgp_ctx* ctx, const double* pars, double* out);
/* MAP prediction of all M outputs at the new inputs xs [S]: mean, var [S, M] (a variance <= 0 is replaced by 1e-6);
 * star [S, 2] = the regressed tilde_l* and tilde_sigma*, or NULL. */
int nmgp_predict_hads(nmgp_ctx* ctx, const double* pars, const double hyper[9], const double* xs, int S, double* mean, double* var,
                      double* star);

/* ---- Hadamard form of the stationary model (logpos.nlogpos_obj_hadamard_S / logpos_hadamard_S, logpos.py:662-716;
 * prediction.point_ / pointwise_predmap_S_hadamard, prediction.py:1695-1740): the LMC baseline on the subject nmgp_had_set_data
 * made resident (NMGP_E_STATE otherwise).  pars = [tilde_l, tilde_sigma, L_vec (T raw slots: no exp), tilde_sigma2_err], P = T + 3;
 * hyper[5] = {mu_tilde_l, sigma_tilde_l, a, b, c} as for nmgp_logpos_sta.  With l = exp(tilde_l), s = exp(tilde_sigma), B_f = L L^T,
 * u = x / l:  S[i, j] = B_f[c_i, c_j] (s^2 exp(-(u_i - u_j)^2 / 2) + 1e-6 d_ij) + sigma2_err d_ij.  No GP prior: neither the prior
 * factors nor the prior stream are used.  The three entries may be interleaved with the nmgp_had_* / nmgp_hads_* ones. */
/* B chains: out5 [B, 5] = (NegLog, loglik without the 2 pi term, log_prior_tilde_l, log_prior_L_vec, log_prior_sigma2_err: the
 * UNNORMALISED inverse gamma; tilde_sigma has no prior; the prior entries are reported whatever `prior` is); grad [B, T + 3] =
 * d NegLog / d pars, or NULL; status [B] and the failure semantics as for nmgp_hads_batch_eval.  Chunks of chains below
 * NMGP_HAD_BATCH_SLAB_GB; no summation order depends on B. */
int nmgp_hadst_batch_eval(nmgp_ctx* ctx, const double* pars /*[B,T+3]*/, int B, const double hyper[5], int prior,
                          double* out5 /*[B,5]*/, double* grad /*[B,T+3] or NULL*/, int* status /*[B]*/);
/* out [N, N]: the full symmetric covariance S of one parameter vector. */
int nmgp_hadst_covariance(nmgp_ctx* ctx, const double* pars, double* out /*[N,N]*/);
/* Prediction at the new inputs xs [S] under H parameter vectors: H = 1 is the MAP predictor, H > 1 a chain of posterior draws (the
 * model has no latent curve to regress: a draw is just another parameter vector).  A chunk of draws (nmgp_ps_chunk with
 * (N + 1 + E) ld doubles per draw) is ONE batched factorisation with y and the slice's E cross-covariance rows riding.
 *   indx_star == NULL: all M outputs at every new input; mean, var: [H,S,M]; slices of max(1, N / M) inputs.
 *   indx_star [S]    : output indx_star[s] only at xs[s]; mean, var: [H,S]; slices of N inputs.  A label outside [0, M): NMGP_E_SHAPE.
 * var = B_f[m, m] (s^2 + 1e-6) - |L_S^-1 k_f|^2 + sigma2_err, a value <= 0 replaced by 1e-6.  status [H] or NULL as for
 * nmgp_predsample_hads; the workspace is the posterior-draw entries' (a pending batch result stays valid).  H draws in one call give
 * the bits of H single calls.  NMGP_E_SHAPE if one draw's factorisation buffer reaches 2^31 elements. */
int nmgp_predict_hadst(nmgp_ctx* ctx, const double* pars /*[H,T+3]*/, int H, const double* xs /*[S]*/,
                       const int* indx_star /*[S] or NULL*/, int S, double* mean, double* var, int* status /*[H] or NULL*/);

/* ---- the cohort of ragged Hadamard subjects under the separable and the stationary model ---------
 * Both entries read the set of nmgp_had_set_subjects (S subjects padded to Nmax <= 3500; see there for the padding) and follow
 * nmgp_had_subjects_eval: B = S * chains_per_subject rows, row s * chains_per_subject + k is chain k of subject s; NMGP_E_STATE
 * without a set, NMGP_E_SHAPE for B != S * chains_per_subject or chains_per_subject < 1, NMGP_E_UNSUPPORTED under
 * NMGP_CHOL=rocsolver; chunks under NMGP_HAD_BATCH_SLAB_GB are whole subjects or parts of one subject's chains, one synchronisation
 * per chunk; a chain's bits depend neither on the chunking nor on the other subjects of the set, and a subject with
 * nobs[s] == Nmax gets the bits of the resident entry's likelihood.  hyper, the tuple, `prior`, status and the failing-row semantics
 * are nmgp_hads_batch_eval's / nmgp_hadst_batch_eval's; a status k > 0 is a leading minor inside the subject's own nobs[s].  The three
 * cohort entries may be interleaved on one set; the separable one shares the set's cached per-subject GP-prior factors.
 *
 * Separable: pars, grad [B, Pmax], Pmax = 2 Nmax + T + 1, the PADDED layout [tilde_l (Nmax) | tilde_sigma (Nmax) | L_vec (T) |
 * tilde_sigma2_err]: subject s fills the first nobs[s] slots of the two curve blocks, the T shared slots and the last slot.  Padded
 * slots are never read (a NaN or 1e300 there changes no bit, and the NMGP_NUM_NAN test covers the real slots only); their gradient
 * is +0.0. */
int nmgp_hads_subjects_eval(nmgp_ctx* ctx, const double* pars /*[B,Pmax]*/, int B, int chains_per_subject, const double hyper[9],
                            int prior, double* out6 /*[B,6]*/, double* grad /*[B,Pmax] or NULL*/, int* status /*[B]*/);
/* Stationary: the parameter vector has no per-observation part, so pars and grad are plain [B, T + 3].  No GP prior: neither the
 * set's prior factors nor the prior stream are touched. */
int nmgp_hadst_subjects_eval(nmgp_ctx* ctx, const double* pars /*[B,T+3]*/, int B, int chains_per_subject, const double hyper[5],
                             int prior, double* out5 /*[B,5]*/, double* grad /*[B,T+3] or NULL*/, int* status /*[B]*/);
/* ---- device-resident HMC trajectories of the cohort (drivers.HadamardCohortHMC / SepCohortHMC / StaCohortHMC) ----
 * ONE family for the three models on the set of nmgp_had_set_subjects: model = NMGP_HAD_MODEL_NONSEP (hyper[8]), _SEP (hyper[9]) or
 * _STA (hyper[5]); rows as in the *_subjects_eval entries (B = S * chains_per_subject, row s * chains_per_subject + k is chain k of
 * subject s), Pmax the model's padded width (T + 3 for the stationary model, where every slot is real).
 *   begin    uploads the start positions and evaluates value + gradient there: out [B, W] and status [B] are the model's
 *            *_subjects_eval's, bit for bit, failing rows included.  Positions, gradients and a per-chain `bad` flag stay on the
 *            device; model, hyper, prior and chains_per_subject are fixed until end.  A second begin replaces the first.
 *   set_mass kind 0: identity (the default after begin); kind 1: minv [B, Pmax] = diag(M^-1) per chain row in the padded layout, of
 *            which only the real slots are read; NMGP_E_SHAPE unless they are finite and > 0; kind 2 (minv NULL): the PRIOR-FACTOR
 *            METRIC M^-1 = L_blk,s L_blk,s^T of the begun model and hyper-parameters, with the set's cached per-subject factors
 *            (below); NMGP_E_UNSUPPORTED for the stationary model, which has no GP prior; any other kind: NMGP_E_SHAPE.  After a
 *            refusal the mass stays what it was.
 *   traj     nsteps leapfrog steps with step size eps[s] for every chain of subject s, momenta p0 [B, Pmax], one value + gradient
 *            evaluation per step (the chunks of the evaluation entries under NMGP_HAD_BATCH_SLAB_GB) and ONE synchronisation at the
 *            end.  Returns the end point q1, p1 (or NULL), the kinetic energy there kin1 [B] = 1/2 sum over the real slots of
 *            p1 minv p1 (or NULL), U1 [B] = NegLog (+inf where failed) and failed [B] = 1 if the potential was undefined at any point
 *            (a chain that is bad at the start counts).  The device then holds the END state.
 *   commit   accept [B]: 0 puts a chain's position, gradient and flag back to what they were before the trajectory.
 *   end      frees the state (also done by nmgp_had_set_subjects, nmgp_had_clear_subjects and the context).
 * Padded slots of pars, p0 and minv are never read (NaN there changes no bit); padded slots of q1 come back as uploaded, those of p1
 * are +0.0.  A chain's bits depend neither on the chunking nor on the other subjects nor on Nmax.  The state is in allocations of its
 * own: every other entry of the context may be called between begin and traj.  NMGP_E_STATE without a set or without begin (a
 * replaced or cleared set included); NMGP_E_SHAPE for a bad model, B != S * chains_per_subject, chains_per_subject < 1, nsteps < 1 or
 * an eps[s] that is not finite and positive; NMGP_E_UNSUPPORTED under NMGP_CHOL=rocsolver.  An API-level failure inside traj puts the
 * start state back and demands a new begin.
 *
 * Under kind 2 the trajectory runs in the whitened coordinates of drivers.PriorMetric at rank 0 (csrc/nmgp_metric.hip):
 *   L_blk,s = blockdiag(chol Sigma_l,s, chol Sigma_L,s per stride-T column of L_vecs, 1)    nonseparable
 *           = blockdiag(chol Sigma_l,s, chol Sigma_sigma,s, c I_T, 1)                        separable (c: float32-rounded hyper[8])
 * on the real slots of subject s (factors of RBF(x_s; hyper[1], hyper[2]) + 1e-6 I and of hyper[4], hyper[5]).  p0 is the WHITENED
 * start momentum (standard normals in the real slots; padded slots are not read), a step is
 *   kick   u -= (kick eps_s) L_blk,s^T g   (skipped for bad chains)        drift   q += eps_s L_blk,s u
 * -- two masked triangular mat-vecs, no solve, no [P, P] matrix, nothing stored per chain -- p1 is the whitened end momentum (+0.0 in
 * padded slots) and kin1 = 1/2 sum over the real slots of p1^2.  commit, end, the chunking, the single synchronisation, the failure
 * semantics and the independence of a chain's bits are unchanged.
 *
 * nmgp_had_subjects_prior_apply: out [B, Pmax] = L_blk,s in (trans 0: whitened -> parameter coordinates, without the prior mean) or
 * L_blk,s^T in (trans 1: a gradient -> whitened coordinates) for the B = S * chains_per_subject padded host rows of the set, model
 * NMGP_HAD_MODEL_NONSEP (hyper[8]) or _SEP (hyper[9]) -- the cohort counterpart of nmgp_svc_batch_prior_apply / nmgp_sep_prior_apply.
 * It needs a set but no begun trajectory.  Padded slots of `in` are never read; padded slots of `out` are +0.0.  NMGP_E_STATE without
 * a set; NMGP_E_SHAPE for B != S * chains_per_subject, chains_per_subject < 1 or a bad model; NMGP_E_UNSUPPORTED for the stationary
 * model and under NMGP_CHOL=rocsolver. */
#define NMGP_HAD_MODEL_NONSEP 0
#define NMGP_HAD_MODEL_SEP    1
#define NMGP_HAD_MODEL_STA    2
int nmgp_had_subjects_traj_begin(nmgp_ctx* ctx, int model, const double* pars /*[B,Pmax]*/, int B, int chains_per_subject,
                                 const double* hyper, int prior, double* out /*[B,W]*/, int* status /*[B]*/);
int nmgp_had_subjects_traj_set_mass(nmgp_ctx* ctx, int kind, const double* minv /*[B,Pmax] or NULL*/);
int nmgp_had_subjects_traj(nmgp_ctx* ctx, const double* eps /*[S]*/, int nsteps, const double* p0 /*[B,Pmax]*/,
                           double* q1 /*[B,Pmax]*/, double* p1 /*[B,Pmax] or NULL*/, double* kin1 /*[B] or NULL*/,
                           double* U1 /*[B]*/, int* failed /*[B]*/);
int nmgp_had_subjects_traj_commit(nmgp_ctx* ctx, const int* accept /*[B]*/);
int nmgp_had_subjects_traj_end(nmgp_ctx* ctx);
int nmgp_had_subjects_prior_apply(nmgp_ctx* ctx, int model, const double* hyper, int trans, const double* in /*[B,Pmax]*/, int B,
                                  int chains_per_subject, double* out /*[B,Pmax]*/);

/* ---- device-resident Adam of the cohort (drivers.HadamardCohortMAP / SepCohortMAP / StaCohortMAP with device_resident=True) ----
 * ONE family for the three models on the set of nmgp_had_set_subjects, next to the trajectories and with allocations of its own: a
 * begun trajectory and a begun optimiser may coexist on one context, and every other entry may be called between two calls.  model,
 * rows, Pmax and hyper as in nmgp_had_subjects_traj_begin.
 *   begin     uploads the start points pars [B, Pmax], zeroes both moments, marks every chain alive, sets t = 0 and stores model,
 *             hyper, prior and chains_per_subject for the run.  It evaluates nothing.  A second begin replaces the first.
 *   adam      niters iterations of torch.optim.Adam's update (no weight decay, no amsgrad) back to back, ONE synchronisation at the
 *             end however many chunks the set needs (the chunks of the evaluation entries under NMGP_HAD_BATCH_SLAB_GB).  Iteration i
 *             is drivers.LockStepMAP.step: value + gradient at the resident parameters, alive[z] &= (status 0, every real slot of the
 *             parameters finite, out[0] and out[1] finite), then for the alive chains, on the real slots,
 *               m = m b1 + (1 - b1) g;  v = v b2 + ((1 - b2) g) g;  pars -= (lr / bc1) (m / (sqrt(v) / sqrt(bc2) + eps))
 *             with bc1 = 1 - b1^t, bc2 = 1 - b2^t from the running t, which persists across calls: 5 iterations in one call equal
 *             2 + 3, bit for bit, and equal the host loop over the model's *_subjects_eval.  out_hist [niters, B, W]: row i holds the
 *             verbose tuples AT the parameters iteration i started from (what the reference logs as target_value_hist), NaN for a
 *             chain that is no longer alive; alive [B] as it stands after the call.  A chain that fails is frozen at its parameters
 *             and stays dead; no other chain notices.
 *   get_pars  pars [B, Pmax] as they stand on the device.
 *   end       frees the state (also done by nmgp_had_set_subjects, nmgp_had_clear_subjects and the context).
 * Padded slots of pars, of the moments and of the set are never read or written (NaN there changes no bit; get_pars returns them as
 * uploaded).  A chain's bits depend neither on the chunking nor on the other subjects nor on Nmax.  NMGP_E_STATE without a set or
 * without begin (a replaced or cleared set included); NMGP_E_NULL for a NULL argument; NMGP_E_SHAPE for a bad model,
 * B != S * chains_per_subject, chains_per_subject < 1, niters < 1, or a history of niters * B * W values above
 * NMGP_HAD_ADAM_HIST_MAX (2^24 doubles = 128 MiB on the device and in out_hist: at 128 chains that is more than 26000 iterations per
 * call); NMGP_E_UNSUPPORTED under NMGP_CHOL=rocsolver.  The state is checked before the pointers: adam and get_pars without a begun run
 * are NMGP_E_STATE whatever else they are given, so a caller that knows of no run may pass NULL buffers.  A refusal leaves the run as
 * it was, and so does NMGP_E_NOMEM from growing the device history at the start of adam, before anything of the state is touched: the
 * same call with fewer iterations may follow.  An API-level failure INSIDE adam's iterations (the evaluation's scratch allocation, a
 * launch or copy error) ends the run: the parameters go back to where the last completed call left them, get_pars still returns
 * them, every further adam is NMGP_E_STATE until a fresh begin, and the first message is kept. */
#define NMGP_HAD_ADAM_HIST_MAX (1LL << 24)
int nmgp_had_subjects_adam_begin(nmgp_ctx* ctx, int model, const double* pars /*[B,Pmax]*/, int B, int chains_per_subject,
                                 const double* hyper, int prior);
int nmgp_had_subjects_adam(nmgp_ctx* ctx, int niters, double lr, double beta1, double beta2, double eps,
                           double* out_hist /*[niters,B,W]*/, int* alive /*[B]*/);
int nmgp_had_subjects_adam_get_pars(nmgp_ctx* ctx, double* pars /*[B,Pmax]*/);
int nmgp_had_subjects_adam_end(nmgp_ctx* ctx);

/* MAP and posterior-draw prediction for the set under the two models.  Both entries follow nmgp_predsample_had_subjects in every
 * convention not named here: B = S * draws_per_subject rows, row s * draws_per_subject + h is draw h of subject s; xs [S, Smax] with
 * the table nstar (NULL: all Smax; 0 <= nstar[s] <= Smax); indx_star == NULL: mean / var [B, Smax, M], indx_star [S, Smax]: mean / var
 * [B, Smax]; a padded new input gets +0.0 in mean, var and star_out, and nothing is read from a padded slot of pars, xs, indx_star, z
 * or star_in, nor from the padded part of the set's x / indx / y: every mask comes from the nobs and nstar tables; status [B] (the
 * finiteness tests cover the row's real parameter slots and real outputs), a failing draw has NaN in its real output slots and leaves
 * its neighbours' bits alone; chunks under NMGP_PREDSAMPLE_CHUNK / NMGP_PREDSAMPLE_SLAB_GB (read at every call) are whole subjects
 * or parts of ONE subject's draws, one synchronisation each; a row's bits depend neither on the chunking, nor on
 * draws_per_subject, nor on the other subjects of the set, nor on the slice a new input falls into; a subject with nobs[s] == Nmax and
 * nstar[s] == Smax gets the bits of the resident entry under the same starred values; the same error codes for the same mistakes,
 * NMGP_E_UNSUPPORTED under NMGP_CHOL=rocsolver; the set, its prior factors, the resident subject and a pending batched result stay
 * as they were.
 *
 * Separable: pars [B, 2 Nmax + T + 1] in the padded layout of nmgp_hads_subjects_eval (real slots: [0, N_s), [Nmax, Nmax + N_s), the
 * T + 1 shared ones); z / star_in / star_out [B, Smax, 2] (tilde_l*, tilde_sigma* before exp) under nmgp_predsample_hads's rules
 * (z == NULL: the conditional means; star_in skips the regression and z must then be NULL: NMGP_E_STATE; a conditional variance < 0
 * is replaced by 1e-6).  var = B_f[m, m] (sigma*^2 + 1e-6) - |L^-1 k_f|^2 + sigma2_err, a value <= 0 replaced by 1e-6.  The priors
 * hyper[1..2] and hyper[4..5] are looked up in the set's cache, shared with the nonseparable entries and nmgp_hads_subjects_eval. */
int nmgp_predsample_hads_subjects(nmgp_ctx* ctx, const double* pars /*[B,2Nmax+T+1]*/, int B, int draws_per_subject,
                                  const double hyper[9], const double* xs, const int* indx_star, const int* nstar, int Smax,
                                  const double* z, const double* star_in, double* mean, double* var, double* star_out, int* status);
/* Stationary: pars [B, T + 3], every slot real; no latent curve, no hyper, no z, no starred values.  draws_per_subject = 1 is the MAP
 * predictor, > 1 the posterior-draw predictor, as nmgp_predict_hadst is.  var = B_f[m, m] (s^2 + 1e-6) - |L^-1 k_f|^2 + sigma2_err
 * with the same replacement.  Neither the set's prior factors nor the prior stream are touched. */
int nmgp_predict_hadst_subjects(nmgp_ctx* ctx, const double* pars /*[B,T+3]*/, int B, int draws_per_subject, const double* xs,
                                const int* indx_star, const int* nstar, int Smax, double* mean, double* var, int* status);

/* ---- nonseparable ("SVC") objective:  logpos.nlogpos_obj_SVC / logpos_SVC, logpos.py:299-380 -- */
/* hyper[8] = {mu_tilde_l, alpha_tilde_l, beta_tilde_l, mu_L, alpha_L, beta_L, a, b}.
 * out5 = {NegLog, loglik, log_prior_tilde_l, log_prior_uL_vecs, log_prior_sigma2_err} (the verbose tuple).
 * prior = the reference's `Prior` flag.  grad (length N(1+T)+1) receives d NegLog / d pars, or pass NULL.
 * Synchronous. */
int nmgp_logpos_svc(nmgp_ctx* ctx, const double* pars, const double hyper[8], int prior,
                    double out5[5], double* grad);

/* Resident form used by MCMC/MAP loops and the benchmark: the parameter vector lives in HBM
 * (nmgp_svc_pars_dev returns its device address, length N(1+T)+1; nmgp_svc_set_pars copies a host
 * vector into it).  nmgp_svc_eval_resident only enqueues work on the context's stream; results stay on
 * the device until nmgp_svc_fetch (which synchronises, checks the factorisation status and copies
 * out5 / grad). */
int nmgp_svc_set_pars(nmgp_ctx* ctx, const double* pars);
double* nmgp_svc_pars_dev(nmgp_ctx* ctx);
double* nmgp_svc_grad_dev(nmgp_ctx* ctx);
int nmgp_svc_eval_resident(nmgp_ctx* ctx, const double hyper[8], int prior, int want_grad);
int nmgp_svc_fetch(nmgp_ctx* ctx, double out5[5], double* grad);

/* Batched form: B chains of the resident subject (same x, Y; B parameter vectors stacked [B, P]) are evaluated by ONE
 * launch sequence -- every kernel takes the chain as a grid dimension, so the latency-bound panel steps of the
 * factorisation are paid once per batch.  This is the throughput path of MCMC with
 * many chains (the reference runs its chains as separate processes, Nonseparable_model_mpisim.py:305-306).
 * nmgp_svc_batch_alloc sizes B covariance buffers (B * 8 * MN * (MN+1) bytes; called again with the SAME B it keeps every buffer --
 * the gradient workspace of 128 chains at the headline size is 116 GB, seconds of allocation -- and only resets the batch's state:
 * chains of the resident subject, identity metric, no trajectory / optimiser, zero parameters); nmgp_svc_batch_eval only enqueues;
 * nmgp_svc_batch_fetch synchronises and returns out[B,5] and per-chain status[B] (0 ok; k>0 leading minor k not
 * positive definite; NMGP_NUM_NAN) -- a failing chain yields NaNs in its row, not a failed call. */
int nmgp_svc_batch_alloc(nmgp_ctx* ctx, int B);
int nmgp_svc_batch_set_pars(nmgp_ctx* ctx, const double* pars);
/* Optional: make every batch element its own SUBJECT (x: [B,N], Y: [B,N,M] row-major; N, M as in nmgp_set_data) with
 * its own GP-prior factors -- BASELINE config 4, the reference's one-process-per-subject pattern in one launch
 * sequence.  Without this call all batch elements are chains of the subject given to nmgp_set_data. */
int nmgp_svc_batch_set_subjects(nmgp_ctx* ctx, const double* x, const double* Y);
/* Several chains per subject: x [S, N], Y [S, N, M] with S = batch / chains_per_subject; batch element b = s * chains_per_subject + k
 * is chain k of subject s (its parameter vector: row b of nmgp_svc_batch_set_pars).  The chains of a subject share its inputs and its
 * GP-prior factors.  (The reference runs one process per subject and chain: Nonseparable_model_mpisim.py:305-348.) */
int nmgp_svc_batch_set_subjects_chains(nmgp_ctx* ctx, const double* x, const double* Y, int chains_per_subject);
double* nmgp_svc_batch_pars_dev(nmgp_ctx* ctx);
int nmgp_svc_batch_eval(nmgp_ctx* ctx, const double hyper[8], int prior, int want_grad);
int nmgp_svc_batch_fetch(nmgp_ctx* ctx, double* out, int* status);
/* gradients d NegLog / d pars of the last batched evaluation (want_grad = 1): [B, P] on the host / in HBM */
int nmgp_svc_batch_fetch_grad(nmgp_ctx* ctx, double* grad);
double* nmgp_svc_batch_grad_dev(nmgp_ctx* ctx);

/* Device-resident leapfrog trajectories of the B chains -- the inner loop of the HMC sampler the reference's scripts hand their
 * potential to (Nonseparable_model.py:228-231: step_size 1e-4, num_steps_in_leap 20; the sampler itself is an external package).
 * Positions (the batch's parameter vectors), momenta and gradients stay in HBM between the `nsteps` batched value+gradient
 * evaluations of a trajectory; the caller draws the momenta and the accept uniforms and keeps the potentials.
 *   nmgp_svc_batch_traj_begin : after a batched value+gradient evaluation of the start positions (set_pars + batch_eval(.., 1))
 *   nmgp_svc_batch_traj       : p0 [B,P] in; end point q1, p1 [B,P], potential U1 [B] (NegLog; +inf where failed) and
 *                               failed [B] (1: the potential was undefined somewhere on the trajectory -> reject) out
 *   nmgp_svc_batch_traj_commit: accept [B]; rejected chains get their pre-trajectory position and gradient back
 *   nmgp_svc_batch_traj_set_mass: constant mass matrix M of the sampler (Nonseparable_model_mpiKAISER.py:267-270,398-411 passes
 *                               M = inv(sample covariance), step size 1e-1, 5 leapfrog steps): kind 0 identity (default),
 *                               1 diagonal (minv = diag(M^-1) [P]), 2 dense (minv = M^-1 [P,P], row-major == column-major: it is
 *                               symmetric).  The drift becomes q += eps M^-1 p (dense: one GEMM per leapfrog step for all chains);
 *                               with nmgp_svc_batch_traj the momenta p ~ N(0, M) and the kinetic energy 1/2 p^T M^-1 p remain
 *                               the caller's.  Changing the metric (or the batch's subjects) invalidates a begun trajectory.
 *   nmgp_svc_batch_traj_set_mass_chol: a square root of M for the same kind -- sqrt(diag M) [P], or R [P,P] COLUMN-major with
 *                               R R^T = M (the lower Cholesky factor, zeros stored above the diagonal, or any other) -- so that
 *                               the device can draw the momenta itself
 *   nmgp_svc_batch_traj_z     : like nmgp_svc_batch_traj, but z [B,P] in are STANDARD NORMALS: p0 = chol(M) z is formed on the
 *                               device (start kinetic energy = 1/2 |z|^2 for any metric) and kin1 [B] = 1/2 p1^T M^-1 p1 comes
 *                               back instead of p1 -- no [B,P] x [P,P] product is left on the host.
 *   nmgp_svc_batch_traj_set_mass_prior: the PRIOR-FACTOR metric (kind 3), the one that makes the sampler mix at N = 2048.  The posterior
 *                               is dominated by the GP priors RBF(alpha, beta) + 1e-6 I on tilde_l and on each stride-T column of uL_vecs
 *                               (logpos.py:357-365; condition number ~1e11), whose Cholesky factors the context caches; in the
 *                               coordinates pars = mu + L_blk w, L_blk = blockdiag(chol Sigma_l, chol Sigma_L x T, 1), the Hessian of
 *                               the potential is I + (a few dozen likelihood-informed directions).  M^-1 = L_blk (I + U diag(lam) U^T)^-1
 *                               L_blk^T with U [S, r, P] (per subject: r orthonormal rows of length P), lam [S, r] >= 0 the rank-r
 *                               correction (rank 0 / NULL: the pure prior metric); hyper as for the objective.  The device carries the
 *                               whitened momentum L_blk^T p: every leapfrog step costs two triangular mat-vecs with the cached
 *                               factors and two [P, r] products per chain, no solve and no [P, P] matrix.  Only nmgp_svc_batch_traj_z
 *                               runs under this metric.  nmgp_svc_batch_set_subjects* resets it to the identity (it belongs to the
 *                               subjects it was built for).
 *   nmgp_svc_batch_prior_apply: out [B,P] = L_blk in (trans 0) or L_blk^T in (trans 1) for B parameter-shaped host vectors -- the
 *                               change of coordinates of that metric, exported so that the caller can build U, lam (Hessian-vector
 *                               products of the likelihood in whitened coordinates: drivers.prior_lowrank_metric).
 * An API-level failure anywhere in a trajectory call (either entry; inside the leapfrog loop or in the end point's reductions and
 * copies) restores the start state and requires a fresh value+gradient evaluation + nmgp_svc_batch_traj_begin. */
int nmgp_svc_batch_traj_begin(nmgp_ctx* ctx);
int nmgp_svc_batch_traj_set_mass(nmgp_ctx* ctx, int kind, const double* minv);
int nmgp_svc_batch_traj_set_mass_chol(nmgp_ctx* ctx, int kind, const double* mchol);
int nmgp_svc_batch_traj_set_mass_prior(nmgp_ctx* ctx, const double hyper[8], int rank, const double* U, const double* lam);
int nmgp_svc_batch_prior_apply(nmgp_ctx* ctx, const double hyper[8], int trans, const double* in, double* out);
/* The same change of coordinates for the SEPARABLE model's parameter vector [tilde_l | tilde_sigma | uL_vec | tilde_sigma2_err]:
 * L_blk = blockdiag(chol Sigma_l, chol Sigma_sigma, c I_T, 1) -- the GP priors of logpos.py:271-281 and the Normal(0, c) prior of
 * :283 (c float32-rounded, as the reference passes it); hyper as for nmgp_logpos_sep.  in / out: B host vectors of length 2N+T+1.
 * The metric of the separable sampler (drivers.SeparablePriorMetric) is built on it. */
int nmgp_sep_prior_apply(nmgp_ctx* ctx, const double hyper[9], int trans, int B, const double* in, double* out);
int nmgp_svc_batch_traj(nmgp_ctx* ctx, const double hyper[8], int prior, double eps, int nsteps, const double* p0,
                        double* q1, double* p1, double* U1, int* failed);
int nmgp_svc_batch_traj_z(nmgp_ctx* ctx, const double hyper[8], int prior, double eps, int nsteps, const double* z,
                          double* q1, double* kin1, double* U1, int* failed);
int nmgp_svc_batch_traj_commit(nmgp_ctx* ctx, const int* accept);

/* Device-resident Adam over the batch -- the MAP loop of Nonseparable_model.py:147-210 (torch.optim.Adam, default betas / eps)
 * for B chains or, with nmgp_svc_batch_set_subjects, for all subjects of a rank at once (Nonseparable_model_mpisim.py:330-348):
 * parameters, gradients and moments stay in HBM; per iteration only the B verbose tuples come back.
 *   nmgp_svc_batch_adam_begin : start points = the batch's parameter vectors (nmgp_svc_batch_set_pars); moments := 0
 *   nmgp_svc_batch_adam_step  : one value+gradient evaluation + update; out [B,5] are the tuples at the parameters the iteration
 *                               started from (NaN row for a subject that is no longer alive); alive [B] turns 0 at a subject's
 *                               first failed evaluation (its parameters stay frozen; the others go on)
 *   nmgp_svc_batch_get_pars   : the parameter vectors [B,P] as they stand */
int nmgp_svc_batch_adam_begin(nmgp_ctx* ctx);
int nmgp_svc_batch_adam_step(nmgp_ctx* ctx, const double hyper[8], int prior, double lr, double beta1, double beta2, double eps,
                             double* out, int* alive);
int nmgp_svc_batch_get_pars(nmgp_ctx* ctx, double* pars);

/* Dense covariance of the nonseparable model as the reference assembles it (logpos.py:339-353:
 * K_x, generate_K_index_SVC, the n-major->m-major permutation, kron(ones, K_x) * K_i, + sigma2 I).
 * out: [MN, MN] full symmetric, output-major.  For tests and for callers that want Sigma itself. */
int nmgp_svc_covariance(nmgp_ctx* ctx, const double* pars, double* out);

/* ---- separable objective:  logpos.nlogpos_obj / logpos, logpos.py:216-296 ------------------- */
/* hyper[9] = {mu_tilde_l, alpha_tilde_l, beta_tilde_l, mu_tilde_sigma, alpha_tilde_sigma,
 *             beta_tilde_sigma, a, b, c};
 * out6 = {NegLog, loglik, lp_tilde_l, lp_tilde_sigma, lp_uL_vec, lp_sigma2_err}; grad length 2N+T+1. */
int nmgp_logpos_sep(nmgp_ctx* ctx, const double* pars, const double hyper[9], int prior,
                    double out6[6], double* grad);

/* ---- stationary objective:  logpos.nlogpos_obj_S / logpos_S, logpos.py:383-462 -------------- */
/* hyper[5] = {mu_tilde_l, sigma_tilde_l, a, b, c}; out5 = {NegLog, loglik, lp_tilde_l, lp_uL_vec,
 * lp_sigma2_err}; grad length T+3. */
int nmgp_logpos_sta(nmgp_ctx* ctx, const double* pars, const double hyper[5], int prior,
                    double out5[5], double* grad);

/* B chains of the SEPARABLE model of the resident subject per launch sequence -- the unit the reference runs as separate processes
 * (Separable_model_mpisim.py:299-300) and the potential evaluations of its sampler (Separable_model.py:209): chain b's M blocks
 * wB_b[p] K_x,b + sigma2_b I join ONE batch of the blocked Cholesky (B M matrices of order N), as do the triangular products and the
 * inverse SYRK of the gradient; objective of logpos.py:216-296 per chain.
 * pars [B, 2N+T+1]; out6 [B, 6] (as nmgp_logpos_sep); grad [B, 2N+T+1] or NULL; status [B]: 0 = exact covariance, k in 1..3 = the
 * chain needed k jitter retries (re-evaluated through nmgp_logpos_sep: the reference's `while loglik != loglik` loop), negative =
 * -(numerical failure code) if it failed even so (its out6 row is NaN, its gradient row zero).  Returns 0 unless an API / runtime
 * error occurred.
 * Every piece of the evaluation takes the chain as a grid dimension and the value and gradient halves are enqueued back to back: one
 * host synchronisation per call.  Device workspace: B M (2N + 2) N doubles for the factorisation with gradients (N + 1 without) +
 * B M N^2 (-S^-1) + 2 B N^2 (K_x, the weighted sum) -- 2.5 GB per chain at N = 4096, D = 5; the batch is evaluated in chunks of
 * chains whose workspace stays below NMGP_SEP_BATCH_SLAB_GB (environment, default 96) and of at most 65,535 / M chains (grid limit);
 * NMGP_E_SHAPE if a single chain does not fit.  Largest batch exercised on hardware: 32 chains x 5 blocks of N = 4096 (B M = 160). */
int nmgp_sep_batch_eval(nmgp_ctx* ctx, const double* pars, int B, const double hyper[9], int prior, double* out6, double* grad,
                        int* status);

/* The separable model for MANY SUBJECTS per launch sequence (the cohort loop of Separable_model_mpiKAISER.py, one process per subject
 * and chain there): x [S, N], Y [S, N, M] row-major, N and M those of nmgp_set_data.  While the set is active nmgp_sep_batch_eval
 * requires B == S * chains_per_subject (NMGP_E_SHAPE otherwise) and batch element b = s * chains_per_subject + k is chain k of
 * subject s: it reads x[s], Y[s] and that subject's GP-prior factors (one pair per subject, one batched factorisation on first use,
 * cached per (alpha, beta) with the set; a subject whose prior covariance is not positive definite fails the evaluation with its
 * index in the message).  Outputs, gradient layout and status are those of nmgp_sep_batch_eval.  The prior terms are solved by
 * substitution against the subject's factors (NMGP_PRIOR_SOLVE=rocblas, and N > 3500: one library trsm per subject), so they agree
 * with the resident path to rounding; the likelihood and its gradient agree to the bit.  Chunks (NMGP_SEP_BATCH_SLAB_GB) are whole
 * subjects, or parts of one subject when chains_per_subject exceeds a chunk.  A chain that fails numerically -- and every chain when
 * B == 1, under NMGP_SEP=eig or beyond the block kernel's N -- is evaluated through nmgp_logpos_sep ON ITS OWN SUBJECT; the
 * resident subject and its cached prior factors are back in place when the call returns.
 * NMGP_E_STATE without a complete-data resident subject, NMGP_E_NULL for a NULL x or Y, NMGP_E_SHAPE for S < 1 or
 * chains_per_subject < 1.  A second call replaces the set.  The set lives until nmgp_sep_batch_clear_subjects, nmgp_set_data or
 * nmgp_had_set_data, each of which frees it with its prior factors; without a set nmgp_sep_batch_eval evaluates the resident
 * subject exactly as before.  nmgp_sta_batch_eval (below) reads the set's x and Y in the same way; no other entry looks at the set:
 * nmgp_logpos_sep, nmgp_logpos_sta, nmgp_sep_prior_apply and the predictors keep using the resident subject. */
int nmgp_sep_batch_set_subjects_chains(nmgp_ctx* ctx, const double* x, const double* Y, int S, int chains_per_subject);
int nmgp_sep_batch_clear_subjects(nmgp_ctx* ctx);

/* B chains of the STATIONARY (LMC) model per launch sequence: Sigma = B kron K_rbf + sigma2 I, the baseline of
 * Stationary_model.py, Stationary_model_mpisim.py (one process per chain there) and Stationary_model_mpiKAISER.py (one per subject);
 * objective of logpos.py:383-462 per chain.  pars [B, T+3] = [tilde_l, tilde_sigma, uL_vec (T), tilde_sigma2_err]; hyper, out5 [B, 5]
 * and the prior terms (reported whatever `prior` is) as nmgp_logpos_sta; grad [B, T+3] or NULL; status [B] as nmgp_sep_batch_eval:
 * 0 = exact covariance, k in 1..3 = the chain needed k jitter retries (re-evaluated through nmgp_logpos_sta), negative = -(numerical
 * failure code) if it failed even so (its out5 row is NaN, its gradient row zero); the other chains keep their bits.
 * Chain b's M blocks wB_b[p] K_b + sigma2_b I (in B_b's eigenbasis) are written straight from (x, exp(tilde_l), exp(tilde_sigma))
 * with the Gibbs build's element expression -- K itself is never stored -- and join ONE batch of the blocked Cholesky on its
 * substitution-based (`precise`) panel kernels, so that a chain's bits depend neither on B nor on its neighbours; B = 1 runs the same
 * kernels.  The gradient is ONE pass over the M blocks -S_p^-1 (K_ij and d_ij recomputed) that leaves partial sums per column
 * group, added by the host in index order.  One host synchronisation per chunk.  Device workspace per chain: M (2N + 2) N doubles
 * for the factorisation with gradients (N + 1 without) + M N^2 (-S^-1): 2.02 GB at N = 4096, D = 5 (the separable entry: 2.29 GB),
 * 0.67 GB without gradients.  Chunks: below NMGP_SEP_BATCH_SLAB_GB, at most 65,535 / M chains and at most NMGP_STA_BATCH_MAX chains
 * (environment, read at call time, unset = no limit); NMGP_E_SHAPE if a single chain does not fit.
 * While a set of nmgp_sep_batch_set_subjects_chains is active, chain b reads x and Y of subject b / chains_per_subject and
 * B == S * chains_per_subject is required (NMGP_E_SHAPE); chunks are whole subjects or parts of one.  Nothing per subject is cached:
 * the model has no GP priors.  Without a set every chain reads the resident subject.  NMGP_E_STATE without a complete-data resident
 * subject (a Hadamard subject included: the context stays usable), NMGP_E_NULL for a NULL pars / hyper / out5 / status,
 * NMGP_E_SHAPE for B < 1.  NMGP_SEP=eig and N > 11,584 evaluate chain by chain through nmgp_logpos_sta. */
int nmgp_sta_batch_eval(nmgp_ctx* ctx, const double* pars, int B, const double hyper[5], int prior, double* out5, double* grad,
                        int* status);

/* ---- primitives (host buffers in / out) ----------------------------------------------------- */
/* kernels.pairwise_distances, kernels.py:5-21.  x1: [n1,d], x2: [n2,d] or NULL (=x1). out: [n1,n2]. */
int nmgp_pairwise_distances(nmgp_ctx* ctx, const double* x1, int n1, const double* x2, int n2, int d,
                            double* out);
/* kernels.RBF_cov, kernels.py:24-43.  x2 == NULL selects the symmetric form with jitter*I. */
int nmgp_rbf_cov(nmgp_ctx* ctx, const double* x1, int n1, const double* x2, int n2, int d,
                 double alpha, double beta, double* out);
/* kernels.Nonstationary_RBF_cov, kernels.py:46-73.  s1/l1 (s2/l2) may be NULL (= ones). */
int nmgp_nonstat_rbf_cov(nmgp_ctx* ctx, const double* x1, const double* s1, const double* l1, int n1,
                         const double* x2, const double* s2, const double* l2, int n2, int d,
                         double* out);
/* kronecker_operation.kronecker_product, kronecker_operation.py:5-22.  a: [ar,ac], b: [br,bc]. */
int nmgp_kron_product(nmgp_ctx* ctx, const double* a, int ar, int ac, const double* b, int br, int bc,
                      double* out);
/* kronecker_operation.kron_mv, kronecker_operation.py:72-85.  B: [m1,m2], K: [n1,n2], y: [m2*n2]
 * (output-major), out: [m1*n1]. */
int nmgp_kron_mv(nmgp_ctx* ctx, const double* B, int m1, int m2, const double* K, int n1, int n2,
                 const double* y, double* out);
/* distributions.multivariate_normal_logpdf, distributions.py:10-23: -0.5 logdet - 0.5 (y-mu)' invSigma (y-mu)
 * for a caller-supplied inverse [n,n] and log-determinant (mu may be NULL = zeros). */
int nmgp_mvn_logpdf(nmgp_ctx* ctx, const double* y, const double* mu, double logdetSigma,
                    const double* invSigma, int n, double* out);
/* distributions.multivariate_normal_logpdf0, distributions.py:26-52: log density (without 2 pi) of
 * N(mu, B kron K + sigma2 I) in the joint eigenbasis.  B: [M,M], K: [N,N], y/mu: [MN] (mu may be NULL). */
int nmgp_mvn_logpdf_kron(nmgp_ctx* ctx, const double* y, const double* mu, const double* B, int M,
                         const double* K, int N, double sigma2, double* out);
/* distributions.multivariate_normal_logpdf2, distributions.py:99-113 (dense Cholesky evaluation). */
int nmgp_mvn_logpdf_dense(nmgp_ctx* ctx, const double* y, const double* mu, const double* B, int M,
                          const double* K, int N, double sigma2, double* out);
/* kronecker_operation.kron_inv / kron_logdet, kronecker_operation.py:36-69. out_inv: [MN,MN]. */
int nmgp_kron_inv_logdet(nmgp_ctx* ctx, double sigma2, const double* B, int M, const double* K, int N,
                         double* out_inv, double* out_logdet);

/* Cholesky factorisation A = L L^T of a symmetric positive definite [n,n] matrix (torch.cholesky as used at
 * prediction.py:974; also the entry through which the custom blocked factorisation of the log-posterior path is
 * tested on its own).  out_L: [n,n] row-major with the factor in the UPPER triangle == column-major lower (i.e.
 * out_L^T is the usual lower factor; the other triangle is scratch: the input's values, except that the diagonal 16x16
 * blocks carry the inverted diagonal blocks the panel solve reuses).  rhs (optional, [n]) is carried
 * through the factorisation as an extra row: out_z = L^-1 rhs.  algo: 1 = custom gfx950 factorisation, 0 = rocSOLVER. */
int nmgp_cholesky(nmgp_ctx* ctx, const double* A, int n, const double* rhs, double* out_L, double* out_z,
                  int algo);
/* Developer entry of the BATCHED custom factorisation, laid out as the batched objectives lay it out: `batch` symmetric
 * [n,n] matrices A [batch,n,n] (only the triangle nmgp_cholesky reads -- the row-major upper one -- is uploaded), below each of
 * them `extra` dense rows (rows: [batch,extra,n], NULL iff extra = 0) and, with want_xtri = 1, a zero pad row if n + extra is
 * odd and the n seeded rows that turn into X = L^-T.  precise = 1: the accuracy-first diagonal blocks and solves.
 *   out_L    [batch,n,n]      as nmgp_cholesky's (out_L^T is the lower factor); the other triangle is returned as zeros
 *   out_rows [batch,extra,n]  the dense rows on exit, R L^-T (NULL iff extra = 0)
 *   out_X    [batch,n,n]      want_xtri: out_X^T is X; only X's upper triangle is promised, what lies left of its diagonal is
 *                             whatever the buffer held (NaN under NMGP_POISON=1) apart from the seeded band
 *   out_inv  [batch,n,n]      want_inv = 1 | 2 (needs want_xtri, NMGP_E_STATE otherwise): -X X^T = -A^-1 as the gradient paths
 *                             build it, out_inv^T's lower triangle (1) or both triangles (2)
 *   status   [batch]          0, or k > 0: leading minor k of that matrix is not positive definite.  Such a matrix does not
 *                             fail the call (return value 0); its outputs are unspecified, the other matrices' are not touched.
 * No device buffer is cleared first: under NMGP_POISON=1 everything the production callers leave unwritten stays NaN. */
int nmgp_cholesky_batch(nmgp_ctx* ctx, const double* A, int n, int batch, const double* rows, int extra, int want_xtri,
                        int want_inv, int precise, double* out_L, double* out_rows, double* out_X, double* out_inv,
                        int* status);

/* ---- deterministic prediction (prediction.py:912-988, 337-408, 1566-1638) -------------------- */
/* Nonseparable: predictive mean / variance of y at S new inputs xs given MAP parameters.
 * mean, var: [S,M]; Lstar: [S,T] (predicted L_vec at xs, exp already applied on the diagonal slots). */
int nmgp_predict_svc(nmgp_ctx* ctx, const double* pars, const double hyper[8], const double* xs, int S,
                     double* mean, double* var, double* Lstar);
int nmgp_predict_sep(nmgp_ctx* ctx, const double* pars, const double hyper[9], const double* xs, int S,
                     double* mean, double* var);
int nmgp_predict_sta(nmgp_ctx* ctx, const double* pars, const double* xs, int S, double* mean,
                     double* var);

/* ---- posterior-draw prediction (prediction.py:1265-1398 and :1038-1262) ---------------------- */
/* The nonseparable predictor for H parameter vectors (posterior draws) of the resident subject at S new inputs, in batched
 * launch sequences.  Per draw h and new input s: the latent curves are regressed onto xs_s under their RBF priors, noise of the
 * conditional variance is added (z: [H,S,1+T] standard normals, slot 0 for tilde_l*, 1..T for L*; NULL = zeros, the conditional
 * mean), and mean / var [H,S,M] of y follow from the draw's covariance as in nmgp_predict_svc.  y* = mean + sqrt(var) z_y is the
 * caller's.
 *   constrained = 1 : the `predsample` family (:1300-1308): the regression runs on the CONSTRAINED L_vecs (exp applied on the
 *                     diagonal slots) and the sampled vector enters vec2lowtriangle with no exp afterwards;
 *   constrained = 0 : the `predmap_*_sampling` family (:1128-1137): the regression runs on the unconstrained uL_vecs, exp is
 *                     applied on the diagonal slots after the noise; with z = NULL this is nmgp_predict_svc's predictor.
 *   star_in         : [H,S,1+T] starred values (tilde_l*, the T slots of L* as they enter vec2lowtriangle) to use instead of
 *                     regressing; z must then be NULL (NMGP_E_STATE otherwise).  star_out (optional): the values used.
 * One conditional variance per prior, (alpha^2 + 1e-6) - proj . k, serves all T slots; a value < 0 is replaced by 1e-6
 * (settings.precision), as is a predictive variance <= 0.
 * status [H] (optional) follows nmgp_svc_batch_fetch: 0 ok, k > 0 the draw's covariance is not positive definite (leading minor
 * k), NMGP_NUM_NAN; such a draw's rows of mean / var are NaN and the call still returns 0.
 * The draws go through in chunks of B: one batched covariance build and one batched blocked Cholesky per chunk and grid slice,
 * with y and the (grid points x M) cross-covariance rows of each draw's own starred values riding below each matrix; more than
 * MN riding rows go through in slices of MN / M grid points.  A batch of draws gives the bits of the same draws one call each.
 * Device workspace: B (MN + 1 + min(S M, MN)) MN doubles for the factorisations + 2 N S for the projections + O(B (P + S (T + M))),
 * independent of H.  B = what keeps the factorisation buffers below NMGP_PREDSAMPLE_SLAB_GB (environment, default 16), at most
 * 64; NMGP_PREDSAMPLE_CHUNK overrides.  The workspace is the entry's own (kept until nmgp_set_data / nmgp_ctx_destroy): the
 * call invalidates nothing -- the resident parameters, a pending batched evaluation, its gradients and a begun trajectory stay
 * valid.  It synchronises the context's stream.  Runs on the custom factorisation only (NMGP_E_UNSUPPORTED under
 * NMGP_CHOL=rocsolver). */
int nmgp_predsample_svc(nmgp_ctx* ctx, const double* pars /*[H,P]*/, int H, const double hyper[8], const double* xs /*[S]*/,
                        int S, int constrained, const double* z, const double* star_in, double* mean, double* var,
                        double* star_out, int* status);

/* The same for the SEPARABLE model (prediction.py:34-334; pars [H, 2N+T+1], hyper as for nmgp_logpos_sep) and the STATIONARY one
 * (:1640-1692; pars [H, T+3], no hyper-parameters: nothing is regressed).  Per draw h: B = L L^T is eigendecomposed on the host
 * and the M blocks wB[p] K_x + sigma2 I of all draws of a chunk are ONE batch of the blocked Cholesky (B M matrices of order N),
 * with the rotated data row and the cross-covariance row of every grid point riding below each block, as nmgp_predict_sep does
 * for one parameter vector.
 *   separable : the UNCONSTRAINED tilde_l and tilde_sigma are regressed onto xs_s, each under its own RBF prior; z, star_in,
 *               star_out: [H,S,2] (slot 0 tilde_l*, slot 1 tilde_sigma*, both before exp); K_x is the Gibbs kernel + 1e-6 I;
 *               kss_jitter = 1: a2 = B_mm (sigma*^2 + 1e-6), the `predsample` family (:98); kss_jitter = 0: a2 = B_mm sigma*^2,
 *               the `predmap_sampling` family (:251).  One draw, z = NULL, kss_jitter = 1 is nmgp_predict_sep's predictor.
 *               A conditional variance < 0 and a predictive variance <= 0 are replaced by 1e-6.
 *   stationary: K_x = RBF_cov(x; alpha = exp(tilde_sigma), beta = exp(tilde_l)) + 1e-6 I, a2 = B_mm sigma^2; a predictive
 *               variance < 0 (strict) is replaced by 1e-6.  One draw is nmgp_predict_sta's predictor.
 * mean, var: [H,S,M]; status, chunking (NMGP_PREDSAMPLE_SLAB_GB / NMGP_PREDSAMPLE_CHUNK: a draw takes 8 M (N + 1 + min(S, N - 2)) N
 * bytes of factorisation buffer), the entry's own workspace, the synchronisation and batch = single bits as for
 * nmgp_predsample_svc; more than N - 2 grid points go through in slices.  NMGP_E_UNSUPPORTED under NMGP_CHOL=rocsolver or
 * NMGP_SEP=eig; NMGP_E_SHAPE if a block with its riding rows exceeds 2 GiB (the block build's 32-bit byte offsets). */
int nmgp_predsample_sep(nmgp_ctx* ctx, const double* pars /*[H,2N+T+1]*/, int H, const double hyper[9], const double* xs /*[S]*/,
                        int S, int kss_jitter, const double* z, const double* star_in, double* mean, double* var,
                        double* star_out, int* status);
int nmgp_predsample_sta(nmgp_ctx* ctx, const double* pars /*[H,T+3]*/, int H, const double* xs /*[S]*/, int S, double* mean,
                        double* var, int* status);
/* The same for the separable Hadamard model (prediction.point_ / pointwise_ / indexedpoint_ / test_predsample_hadamard,
 * prediction.py:461-707): H parameter vectors of the subject nmgp_had_set_data made resident (NMGP_E_STATE otherwise; pars and
 * hyper as for nmgp_hads_batch_eval), S new inputs.  The covariance depends on the draw only, so a chunk of B draws is ONE
 * batched factorisation of B matrices of order N with y and the cross-covariance rows of the draw's own starred values riding.
 *   indx_star == NULL: all M outputs at every new input; mean, var: [H,S,M]; slices of max(1, N / M) grid points.
 *   indx_star [S]    : output indx_star[s] only at xs[s] (the indexed family); mean, var: [H,S]; slices of N points.  A label
 *                      outside [0, M) is NMGP_E_SHAPE.
 * z, star_in, star_out: [H,S,2] (tilde_l*, tilde_sigma*, before exp) as for nmgp_predsample_sep; z == NULL gives the conditional
 * means; with star_in the regression is skipped and z must be NULL.  var = B_f[m,m] (sigma*^2 + 1e-6) - |L_S^-1 k_f|^2 +
 * sigma2_err; a conditional variance < 0 and a predictive variance <= 0 are replaced by 1e-6.  status [H] (or NULL): 0, a
 * leading-minor index, NMGP_NUM_NAN (also for a parameter vector that is not finite); a failing draw has NaN rows and the call
 * still returns 0.  Chunking by NMGP_PREDSAMPLE_SLAB_GB / NMGP_PREDSAMPLE_CHUNK with 8 (N + 1 + E) ld bytes per draw, E the riding
 * rows of a slice; the workspace is the entry's own (a pending nmgp_hads_batch_eval result stays valid).  H draws in one call give
 * the bits of H single-draw calls; one draw with z == NULL and indx_star == NULL is nmgp_predict_hads's predictor.
 * NMGP_E_SHAPE if one draw's factorisation buffer reaches 2^31 elements (the row reduction and the row kernels shared with the
 * other entries take in-matrix positions as 32-bit integers). */
int nmgp_predsample_hads(nmgp_ctx* ctx, const double* pars /*[H,2N+T+1]*/, int H, const double hyper[9], const double* xs /*[S]*/,
                         const int* indx_star /*[S] or NULL*/, int S, const double* z, const double* star_in, double* mean,
                         double* var, double* star_out, int* status);
/* The same for the NONSEPARABLE Hadamard model: posterior-draw and held-out prediction.  The reference has no posterior-draw form
 * for this model, and its indexed MAP predictor (prediction.indexedpoint_ / test_predmap_SVC_hadamard, prediction.py:1480-1561)
 * reports the variance of output 0 whatever the label; this entry is the corrected predictor for one draw and the posterior-draw
 * form for H.  H parameter vectors of the subject nmgp_had_set_data made resident (NMGP_E_STATE otherwise; pars and hyper as for
 * nmgp_had_batch_eval), S new inputs.  A chunk of B draws is ONE batched factorisation of B matrices of order N with y and the
 * cross-covariance rows of the draw's own starred values riding.
 *   indx_star == NULL: all M outputs at every new input; mean, var: [H,S,M]; slices of max(1, N / M) grid points.
 *   indx_star [S]    : output indx_star[s] only at xs[s] (held-out pairs); mean, var: [H,S]; slices of N points.  A label outside
 *                      [0, M) is NMGP_E_SHAPE.
 * z, star_in, star_out: [H,S,1+T]: slot 0 tilde_l* (before exp), slot 1 + t slot t of L* (taken as it is: no exp, as everywhere in
 * this model).  Each is the GP regression of the draw's own curve under its prior (tilde_l: hyper[0..2]; the T columns of L_vecs:
 * hyper[3..5]) + sqrt(cv) z with ONE conditional variance per prior, cv = (alpha^2 + 1e-6) - proj . k, serving all T slots (the
 * rules of nmgp_predsample_svc); z == NULL gives the conditional means; with star_in the regression is skipped and z must be NULL
 * (NMGP_E_STATE).  Riding row: k_f[i] = g(i, s) <row indx[i] of the draw's L_i, row m of L*_s>, g the Gibbs cross term without
 * jitter with l* = exp(tilde_l*).  mean = (L_S^-1 k_f)^T (L_S^-1 y); var = (1 + 1e-6) (L* L*^T)_mm - |L_S^-1 k_f|^2 + sigma2_err; a
 * conditional variance < 0 and a predictive variance <= 0 are replaced by 1e-6.  status [H] (or NULL), the failure semantics, the
 * chunking (8 (N + 1 + E) ld bytes per draw) and the workspace as for nmgp_predsample_hads (a pending nmgp_had_batch_eval result
 * stays valid).  H draws in one call give the bits of H single-draw calls, whatever the chunking and whichever slice a grid point
 * falls in.  One draw with z == NULL and indx_star == NULL is nmgp_predict_had's predictor: the same starred values bit for bit, mean
 * and variance to rounding (this entry factors with the substitution-based panel kernels, that one with the default ones).
 * NMGP_E_UNSUPPORTED for M > 8; NMGP_E_SHAPE if one draw's factorisation buffer reaches 2^31 elements. */
int nmgp_predsample_had(nmgp_ctx* ctx, const double* pars /*[H,N(1+T)+1]*/, int H, const double hyper[8], const double* xs /*[S]*/,
                        const int* indx_star /*[S] or NULL*/, int S, const double* z /*[H,S,1+T] or NULL*/,
                        const double* star_in /*[H,S,1+T] or NULL*/, double* mean, double* var,
                        double* star_out /*[H,S,1+T] or NULL*/, int* status /*[H] or NULL*/);

/* ---- measurement ---------------------------------------------------------------------------- */
/* Per-stage HIP-event timing on the context's stream (bench.py roofline figures).  Stages: */
enum {
    NMGP_STAGE_COV = 0,     /* fused covariance build (kernel #1)            */
    NMGP_STAGE_CHOL = 1,    /* Cholesky factorisation of Sigma               */
    NMGP_STAGE_SOLVE = 2,   /* triangular solve(s) with y                    */
    NMGP_STAGE_REDUCE = 3,  /* log-det / quadratic-form reductions + combine */
    NMGP_STAGE_PRIOR = 4,   /* GP priors (cached factors, trsm)              */
    NMGP_STAGE_INVERSE = 5, /* Sigma^-1 for the gradient                     */
    NMGP_STAGE_ADJOINT = 6, /* fused adjoint contraction (kernel #5)         */
    NMGP_STAGE_EIG = 7,     /* eigendecomposition (separable / stationary)   */
    NMGP_STAGE_KRONMV = 8,  /* Kron-vec contraction (kernel #3)              */
    NMGP_STAGE_SYRK = 9,    /* every k_syrk_lower launch of the blocked Cholesky (FP64 MFMA), timed on its own stream */
    NMGP_STAGE_COUNT = 10
};
int nmgp_profile_enable(nmgp_ctx* ctx, int on);   /* 0 off; 1 one HIP-event pair per stage; 2 additionally one pair per k_syrk_lower launch */
/* Accumulated milliseconds and launch counts per stage since the last reset; synchronises. */
int nmgp_profile_read(nmgp_ctx* ctx, double ms[NMGP_STAGE_COUNT], long long count[NMGP_STAGE_COUNT]);
int nmgp_profile_reset(nmgp_ctx* ctx);
/* As nmgp_profile_read, plus the algorithmic work accumulated per stage; tracked for NMGP_STAGE_SYRK only (0 elsewhere):
 * flop = 2 K per updated lower-trapezoid element of every launch, bytes = 8 * (read + write of those elements + the
 * mrows x K panel read once). */
int nmgp_profile_read_work(nmgp_ctx* ctx, double ms[NMGP_STAGE_COUNT], long long count[NMGP_STAGE_COUNT],
                           double flop[NMGP_STAGE_COUNT], double bytes[NMGP_STAGE_COUNT]);
/* Jitter retries the last nmgp_logpos_sep / nmgp_logpos_sta evaluation needed: 0 = value and gradient are those of the exact
 * covariance, k > 0 = of the covariance with k x 1e-6 added to the diagonals of B and K_x (the reference retries a NaN
 * likelihood with RANDOM jitter of that size, logpos.py:267-268 / distributions.py:55-96; here any numerical failure of the
 * first attempt -- NaN or a non-positive pivot -- triggers the deterministic retry).  -1 for a NULL context. */
int nmgp_last_sep_attempts(const nmgp_ctx* ctx);
/* Micro-benchmarks used to state measured peaks next to the spec ones: HBM stream (GB/s) and a
 * rocBLAS dgemm of size n (TFLOP/s). */
int nmgp_measure_hbm_gbs(nmgp_ctx* ctx, long long bytes, int reps, double* gbs);
/* gbs3 = {copy (read + write bytes counted), read only, write only}: the chip's streaming ceilings as measured in the run, the
 * figures the HBM-bound kernels are judged against (flat 16-byte-per-lane kernels, tools/lab/hbm_lab.hip). */
int nmgp_measure_hbm_rates(nmgp_ctx* ctx, long long bytes, int reps, double gbs3[3]);
int nmgp_measure_dgemm_tflops(nmgp_ctx* ctx, int n, int reps, double* tflops);

#ifdef __cplusplus
}
#endif
#endif /* NMGP_H */
