/*
 * mfgp.h — C ABI of the MI355X-native multi-fidelity GP engine (libmfgp.so).
 *
 * This is the drop-in boundary below the Python mirror of the reference's
 * GPflow-facing API.  The reference (qezlou/multi_fidelity_gpflow) is pure
 * Python and has no FFI of its own; each entry point below names the reference
 * interface whose arithmetic it replaces.  The Python side binds it with ctypes
 * (multi_fidelity_gpflow_amd/_lib.py).
 *
 * Conventions
 *   - Every array argument is a caller-owned DEVICE pointer (fp64, row-major,
 *     leading dimensions in elements).  The library never allocates or frees in
 *     a compute call; scratch comes from a caller-provided workspace whose size
 *     is queried with the matching *_workspace_size function.
 *   - theta (device, fp64, constrained values) has the layout
 *         [vL, lL[0..d-1], vD, lD[0..d-1], rho0, noise]      (2d + 4 entries)
 *     i.e. kernel_L (variance, lengthscales), kernel_delta (variance,
 *     lengthscales), rho[0,0] and the Gaussian likelihood variance.
 *   - X rows hold d input columns followed by the fidelity flag (0.0 / 1.0);
 *     rows whose flag is neither exactly 0 nor 1 produce zero kernel rows
 *     (mfgpflow/linear.py:67-70).
 *   - Calls are asynchronous and ordered on the handle's stream (default: the
 *     null stream); none synchronises, so they can be captured in a hipGraph.
 *   - Return value: 0 = ok, < 0 = bad argument / launch error (see
 *     mfgp_error_string).  A Cholesky that meets a non-positive pivot writes a
 *     LAPACK-style info > 0 (1-based row) into the caller's device int; the
 *     Python layer raises the analogue of TF's InvalidArgumentError.
 *   - Threading: a handle must not be used by two host threads at once.
 */
#ifndef MFGP_H_
#define MFGP_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mfgp_handle_s* mfgp_handle_t;

#define MFGP_OK 0
#define MFGP_ERR_ARG (-1)
#define MFGP_ERR_WORKSPACE (-2)
#define MFGP_ERR_LAUNCH (-3)
#define MFGP_ERR_DIM (-4)
/* mfgp_flow_fence / a flow-bearing call found the device's flow fence held by another host thread
 * for longer than the library's bound (10 s): an MFGP_FENCE_WAIT that was never paired with its
 * MFGP_FENCE_RECORD.  Nothing of the failed call was enqueued. */
#define MFGP_ERR_FENCE (-5)
#define MFGP_MAX_D 32
/* info value written when the persistent Cholesky launch gave up waiting (bounded spin) */
#define MFGP_FLOW_TIMEOUT (-100)

int mfgp_version(void);
/* Hash of the sources this library was built from (every file of csrc/ and include/mfgp.h:
 * multi_fidelity_gpflow_amd/build.py source_hash()); "unknown" for a build made without it. */
const char* mfgp_build_id(void);
const char* mfgp_error_string(int code);

/* Handle: device + stream + tile size (32 or 64).  No reference analogue
 * (TensorFlow's implicit device context). */
int mfgp_create(int device, mfgp_handle_t* out);
int mfgp_destroy(mfgp_handle_t h);
int mfgp_set_stream(mfgp_handle_t h, void* hip_stream);
int mfgp_set_tile(mfgp_handle_t h, int nb);
int mfgp_get_tile(mfgp_handle_t h);
/* Cholesky schedule of the LML path (tile 32): 1 = one persistent dataflow launch
 * (k_chol_flow, default when the device reports its CU count) for factorizations of 8 or more
 * 32-tiles (smaller ones are faster as step launches), 3 = the flow at every size, 0 = one launch
 * per tile step.  mfgp_get_flow returns the mode (0, 1 or 3).
 * Results agree to rounding; a workspace must be sized under the setting it is used with. */
int mfgp_set_flow(mfgp_handle_t h, int enable);   /* 2: flow + diagnostic timeline; 3: flow at every size */
/* Small problems (n <= 64, p <= 64, D <= 16, the AR1 kernel, 32-tiles): the LML value + gradient
 * (+ the Adam step of mfgp_gpr_adam_step), and mfgp_gpr_predict for n* <= 64, as ONE launch each
 * instead of the step sequence (default 1: 36 vs 43.5 us at HBS; 0, or MFGP_TINY=0 in the
 * environment: the step sequence).  Same results to rounding. */
int mfgp_set_tiny(mfgp_handle_t h, int enable);
int mfgp_get_tiny(mfgp_handle_t h);
/* Resident workspace (default 0).  On the fp64 flow path (the AR1 kernel, 32-tiles, the persistent
 * Cholesky) the Gram is formed inside the flow launch; the launch in front of it only sets up the
 * workspace (the publication area's sentinel fill, schedule tables, reduction slots), and every
 * value+grad call (mfgp_gpr_lml with want_grad, mfgp_gpr_adam_step) leaves exactly that set-up
 * behind.  With resident = 1 a value+grad call whose workspace the previous fp64 LML call ON THIS
 * HANDLE left set up for the same (n, p, d) skips the set-up launch and starts with the flow.  The
 * caller guarantees that nothing else wrote the workspace in between (a training session's private
 * workspace); graphs captured in this mode replay that way.  Results are identical either way. */
int mfgp_set_resident(mfgp_handle_t h, int enable);
/* mfgp_gpr_adam_steps: defer each step's reduction into the next flow launch (default 1; 0, or
 * MFGP_STEP_FUSION=0 in the environment at mfgp_create: a plain loop of single steps).  Same bits. */
int mfgp_set_step_fusion(mfgp_handle_t h, int enable);
int mfgp_get_step_fusion(mfgp_handle_t h);
/* k_grad m-tiles per task (fixed at mfgp_create; env MFGP_GRAD_CHUNK).  Workspace sizes depend on it. */
int mfgp_get_grad_chunk(mfgp_handle_t h);
/* fp32 path (dtype MFGP_F32): iterative refinement with an fp64 residual for the value-only LML
 * (want_grad = 0; one step whenever steps >= 1) and the predictive mean (`steps` steps, 0..2;
 * default 2; 0: plain fp32 solve).  The gradient / Adam calls are never refined.  Workspace sizes follow the setting (size after
 * setting it).  Replaces nothing in the reference (it computes in fp64: linear.py:63-64). */
int mfgp_set_f32_refine(mfgp_handle_t h, int steps);
int mfgp_get_flow(mfgp_handle_t h);
/* Bound of every k_chol_flow hand-off wait, in microseconds from the start of that wait
 * (default 50000).  On expiry the launch drains and info = MFGP_FLOW_TIMEOUT: a scheduling
 * failure (not every workgroup resident, e.g. another kernel holding CUs), not a numerical one.
 * 0 makes any wait that polls 8 times give up (diagnostic: exercises the abort path). */
int mfgp_set_flow_timeout_us(mfgp_handle_t h, long long us);
/* Device-wide ordering of the persistent flow (k_chol_flow needs every CU; two flows launched
 * on two streams at once would each stall waiting for workgroups the other keeps off the CUs).
 * The library fences every flow it launches outside a stream capture: the launch waits for the
 * previous flow on the device (any handle, stream or host thread of the process) and becomes the
 * last one.  A captured graph's flows are not fenced at capture: before replaying such a graph
 * call mfgp_flow_fence(h, MFGP_FENCE_WAIT) on the replay stream, and after enqueueing the replay
 * mfgp_flow_fence(h, MFGP_FENCE_RECORD).  Between the two the calling host thread holds the
 * fence: a flow launch or fence call from another host thread blocks on the host until the
 * RECORD (so it cannot land beside the replay's unfenced flows); the holder's own calls pass.
 * Every WAIT MUST be paired with a RECORD from the same host thread (also on error paths).  Holds
 * nest: a thread's nested WAIT / RECORD brackets release the fence only at the outermost RECORD.
 * A thread that finds the fence held by another waits at most 10 s, then the call returns
 * MFGP_ERR_FENCE.  Device ordering is stream-ordered only (no device synchronisation). */
#define MFGP_FENCE_WAIT 0
#define MFGP_FENCE_RECORD 1
int mfgp_flow_fence(mfgp_handle_t h, int op);
/* Where the flow timeline sits inside an mfgp_gpr_* workspace (diagnostic): `count` int64
 * ticks of the 100 MHz device clock from byte `offset`: per step k the diag workgroup's step
 * start [k], A' ready [T+k], factor start [2T+k], D_k published [3T+k], owner hand-offs of
 * A(k,k-2) [4T+k], A(k,k-1) [5T+k], A(k,k) [6T+k] seen, L(k,k-2) formed [7T+k]; then per
 * worker wave w: first item [8T+3w], done [8T+3w+1], ticks spent waiting [8T+3w+2]. */
int mfgp_gpr_flow_trace(mfgp_handle_t h, int n, int p, int d, size_t* offset, int* count);

/* gpflow.kernels.SquaredExponential.K(X1, X2) (GPflow 2.9 stationaries.py via
 * utilities/ops.py:square_distance).  params = [variance, lengthscales[d]]. */
int mfgp_rbf_gram(mfgp_handle_t h, int n1, int n2, int d, const double* X1, int ldx1, const double* X2, int ldx2,
                  const double* params, double* K, int ldk);

/* LinearMultiFidelityKernel.K(X, X2) — mfgpflow/linear.py:55-104.
 * diag_add is added to K[i][i] (use only for X2 == X). */
int mfgp_mf_gram(mfgp_handle_t h, int n1, int n2, int d, const double* X1, int ldx1, const double* X2, int ldx2,
                 const double* theta, double diag_add, double* K, int ldk);

/* LinearMultiFidelityKernel.K_diag(X) — mfgpflow/linear.py:106-136. */
int mfgp_mf_kdiag(mfgp_handle_t h, int n, int d, const double* X, int ldx, const double* theta, double* out);

/* GPR.log_marginal_likelihood() of MultiFidelityGPModel (mfgpflow/linear.py:138-156;
 * GPflow models/gpr.py) and, with want_grad, its gradient w.r.t. theta (the
 * GradientTape of linear.py:205-207).  out[0] = LML, out[1 + q] = dLML/dtheta[q].
 * Y is [n, p]: all p columns share the one Gram / Cholesky (linear.py:90). */
int mfgp_gpr_workspace_size(mfgp_handle_t h, int n, int p, int d, size_t* bytes);
int mfgp_gpr_lml(mfgp_handle_t h, int n, int p, int d, const double* X, int ldx, const double* Y, int ldy,
                 const double* theta, int want_grad, void* ws, size_t ws_bytes, double* out, int* info);

/* One iteration of MultiFidelityGPModel.optimize(use_adam=True) (linear.py:200-214):
 * value+grad at theta, loss_hist[*step] = -LML, Keras-Adam update of the
 * unconstrained vector u for entries with trainable[q] != 0 (entries with equal
 * tie[q] share one variable and its summed gradient; tie may be NULL), theta refreshed
 * (Softplus; Shift(1e-6)+Softplus for the noise entry), ++*step.  lr / beta1 /
 * beta2 are passed already rounded as the caller wants them (TF 2.10 keeps them
 * as float32 hyper variables). */
int mfgp_gpr_adam_step(mfgp_handle_t h, int n, int p, int d, const double* X, int ldx, const double* Y, int ldy,
                       double* theta, double* u, double* m, double* v, const unsigned char* trainable,
                       const int* tie, int* step, double lr, double beta1, double beta2, double eps,
                       double* loss_hist, void* ws, size_t ws_bytes, double* out, int* info);

/* nsteps Adam steps in one call: when it returns to the stream, theta, u, m, v, *step, loss_hist,
 * out and info are bit for bit what nsteps calls of mfgp_gpr_adam_step leave (a failed evaluation
 * in the middle included: no step, NaN loss, and the next evaluation runs on the unchanged theta).
 * Where the persistent flow forms its own Gram (fp64, 32-tiles, the flow on and taken at this
 * size, not the one-launch small path, D <= 29) the reduction + Adam of every step but the last
 * runs in the head of the next step's flow launch instead of a launch of its own
 * (mfgp_set_step_fusion); everywhere else, and for nsteps == 1, the call is a loop of single steps. */
int mfgp_gpr_adam_steps(mfgp_handle_t h, int n, int p, int d, const double* X, int ldx, const double* Y, int ldy,
                        double* theta, double* u, double* m, double* v, const unsigned char* trainable,
                        const int* tie, int* step, double lr, double beta1, double beta2, double eps,
                        double* loss_hist, void* ws, size_t ws_bytes, double* out, int* info, int nsteps);

/* Diagnostic: the mfgp_gpr_lml(want_grad=1) sequence with hipEvents recorded on
 * the handle's stream between its phases; synchronises and writes the elapsed
 * milliseconds of [pre (empty), gram+R init+first factor, tile Cholesky steps (with
 * alpha = L^{-T} Z fused in), gradient, reductions+finalize] into the HOST array ms[5]. */
int mfgp_gpr_lml_phase_times(mfgp_handle_t h, int n, int p, int d, const double* X, int ldx, const double* Y,
                             int ldy, const double* theta, void* ws, size_t ws_bytes, double* out, int* info,
                             float* ms);

/* theta[q] = softplus(u[q]) (+1e-6 for q == noise_index); GPflow positive(). */
int mfgp_theta_from_u(mfgp_handle_t h, const double* u, double* theta, int g, int noise_index);

/* GPR.predict_f(Xnew, full_cov=False) (GPflow models/gpr.py -> base_conditional;
 * mirror at mfgpflow/linear.py:237-286).  mean [nstar, p]; var [nstar] (the
 * reference tiles it over the p outputs). */
int mfgp_gpr_predict_workspace_size(mfgp_handle_t h, int n, int p, int d, int nstar, size_t* bytes);
int mfgp_gpr_predict(mfgp_handle_t h, int n, int p, int d, int nstar, const double* X, int ldx, const double* Y,
                     int ldy, const double* Xs, int ldxs, const double* theta, void* ws, size_t ws_bytes,
                     double* mean, int ldm, double* var, int* info);

/* GPR.predict_f(Xnew, full_cov=True) (GPflow base_conditional full_cov branch: fvar =
 * Knn - A^T A, A = L^{-1} Kmn, the same [nstar, nstar] block for every output; the Python
 * layer tiles it to [p, nstar, nstar]).  nlf = 0: LinearMultiFidelityKernel (theta as
 * mfgp_gpr_*); nlf = m >= 1: GraphMultiFidelityKernel (theta as mfgp_gmf_*, K(X*, X*)
 * carries the kernel's 1e-6 jitter like graph.py:96).  mean / var as mfgp_gpr_predict;
 * cov [nstar][ldc]. */
int mfgp_gpr_predict_cov_workspace_size(mfgp_handle_t h, int nlf, int n, int p, int d, int nstar, size_t* bytes);
int mfgp_gpr_predict_cov(mfgp_handle_t h, int nlf, int n, int p, int d, int nstar, const double* X, int ldx,
                         const double* Y, int ldy, const double* Xs, int ldxs, const double* theta, void* ws,
                         size_t ws_bytes, double* mean, int ldm, double* var, double* cov, int ldc, int* info);

/* GraphMultiFidelityKernel / GraphMultiFidelityGPModel (mfgpflow/graph.py:7-188) with
 * nlf = m LF sources (fidelity flags 0..m-1 LF, m HF; 1 <= m <= 4).  theta layout
 * (graph_theta_size = (m+1)(d+1) + m + m^2 + 1 entries):
 *   [v_0, l_0(d), .., v_{m-1}, l_{m-1}(d), v_delta, l_delta(d), rho_0..rho_{m-1},
 *    rhoLF[m][m] (row-major; diagonal unused, 1.0), noise]
 * K's LF-LF block (i, j) is rhoLF[i][j] k_i (the ROW source's kernel, graph.py:61-63), so K
 * is not symmetric for rhoLF[i][j] != rhoLF[j][i]; like TF, the factorization reads the
 * lower triangle.  The LML adds the kernel's 1e-6 jitter (graph.py:96) and the noise;
 * mfgp_gmf_gram adds diag_add (pass 1e-6 to mirror K(X)).  The gradient (want_grad) is
 * d LML / d theta over every entry of K, as TF differentiates it. */
int mfgp_gmf_gram(mfgp_handle_t h, int nlf, int n1, int n2, int d, const double* X1, int ldx1, const double* X2,
                  int ldx2, const double* theta, double diag_add, double* K, int ldk);
int mfgp_gmf_kdiag(mfgp_handle_t h, int nlf, int n, int d, const double* X, int ldx, const double* theta,
                   double* out);
int mfgp_gmf_gpr_workspace_size(mfgp_handle_t h, int nlf, int n, int p, int d, size_t* bytes);
int mfgp_gmf_gpr_lml(mfgp_handle_t h, int nlf, int n, int p, int d, const double* X, int ldx, const double* Y,
                     int ldy, const double* theta, int want_grad, void* ws, size_t ws_bytes, double* out, int* info);
int mfgp_gmf_gpr_predict_workspace_size(mfgp_handle_t h, int nlf, int n, int p, int d, int nstar, size_t* bytes);
int mfgp_gmf_gpr_predict(mfgp_handle_t h, int nlf, int n, int p, int d, int nstar, const double* X, int ldx,
                         const double* Y, int ldy, const double* Xs, int ldxs, const double* theta, void* ws,
                         size_t ws_bytes, double* mean, int ldm, double* var, int* info);

/* Batched Cholesky factor inverse of SPD matrices (tf.linalg.cholesky +
 * triangular_solve(L, I) as used by GPflow's conditionals): Linv = chol(A)^{-1},
 * ldiag = diag(chol(A)).  A, Linv: [batch][n][n] with strides sA / sL elements. */
int mfgp_potrf_inv_workspace_size(mfgp_handle_t h, int n, int batch, size_t* bytes);
int mfgp_potrf_inv(mfgp_handle_t h, int n, int batch, const double* A, int lda, long sA, void* ws, size_t ws_bytes,
                   double* Linv, int ldl, long sL, double* ldiag, int* info);

/* Joint Gaussian draws from a batch of dense covariances: with L_b = chol(cov_b + jitter I) (lower),
 *   out(b, s, i, c) = mean(b, i, c) + sum_{j <= i} L_b[i][j] eps(b, s, j, c),
 * b < batch, s < nsamp, i < n, c < ncol.
 *   cov    cov_b is [n][ldc] at b * sC (ldc >= n).  Only its lower triangle is read (as TF's cholesky
 *          reads it) and it is never written; jitter is added to the diagonal as the tiles are loaded.
 *   eps    the standard-normal input, and out: element (b, s, i, c) at b * bs + s * ss + i * rs + c.
 *          eps must not alias out.
 *   mean   element (b, i, c) at b * mean_bs + i * mean_rs + c.
 *   info   [batch]: 0, or the 1-based row of the first non-positive or non-finite pivot of entry b; that
 *          entry's output is then unspecified, the other entries are unaffected.
 * One factor serves all ncol columns of its batch entry.  GPR (one [N*, N*] block for the P outputs):
 * batch = 1, ncol = P, rs = P, ss = N* P.  SVGP ([P, N*, N*]): batch = P, ncol = 1, bs = 1, rs = P,
 * ss = N* P, mean_bs = 1, mean_rs = P -- [N*, P] is read and [S, N*, P] written with no transposed copy.
 * 32 x 32 tiles whatever the handle's tile size: a left-looking tile Cholesky that keeps L (one launch
 * per tile column, launch boundaries the only ordering between workgroups), then one launch for the
 * triangular product L eps with the mean added in its epilogue (upper tiles are never touched).
 * ceil(n / 32) + 1 launches.  Fixed-order sums and no floating-point atomics (the same inputs give the
 * same bits); nothing is allocated, no synchronisation, no host read of a device word.  n = 0 or
 * nsamp = 0: a no-op (MFGP_OK; decided before the pointers are looked at, nothing is written).  A negative
 * count, batch < 1 (or > 65535), ncol < 1, ldc < n or a null pointer: MFGP_ERR_ARG; a workspace smaller than
 * mfgp_mvn_sample_workspace_size reports: MFGP_ERR_WORKSPACE; both before any device work.
 * Replaces: gpflow GPModel.predict_f_samples (models/model.py) and conditionals/util.py sample_mvn
 * (tf.linalg.cholesky(cov + default_jitter() I) @ eps + mean), inherited by every model of the reference. */
int mfgp_mvn_sample_workspace_size(mfgp_handle_t h, int n, int batch, size_t* bytes);
int mfgp_mvn_sample(mfgp_handle_t h, int n, int batch, int nsamp, int ncol, const double* cov, int ldc, long sC,
                    double jitter, const double* mean, long mean_rs, long mean_bs, const double* eps, double* out,
                    long rs, long ss, long bs, void* ws, size_t ws_bytes, int* info /* [batch] */);

/* Batched Gaussian log-density with its gradients w.r.t. the mean and the variances: per row s < ns, with
 *   Sigma_s = obs_cov + diag(f_var(s, .) + obs_var(s, .))  and  r = Y(s, .) - mean(s, .),
 *   logp[s]     = -1/2 r^T Sigma_s^{-1} r - 1/2 log det Sigma_s - (p / 2) log 2 pi,
 *   gmean[s][c] = a_c = (Sigma_s^{-1} r)_c                 (d logp / d mean = -d logp / d Y),
 *   gvar[s][c]  = 1/2 (a_c^2 - (Sigma_s^{-1})_cc)          (d logp / d f_var(s, c)).
 *   mean     [ns][ldm], ldm >= p.
 *   Y        row s at s * y_rs; y_rs = 0: one shared vector (otherwise y_rs >= p).
 *   var      f_var(s, c) at s * var_rs + c * var_cs, var_cs 0 or 1; var_cs = 0: one variance per row (GPR).
 *   obs_var  [p] diagonal variances, row s at s * ov_rs (0: shared, otherwise >= p), or NULL.
 *   obs_cov  [p][ldc] SPD, ldc >= p, only the lower triangle is read, or NULL.
 *   gmean    [ns][ldgm] or NULL; gvar [ns][ldgv] or NULL (ldgm, ldgv >= p).  With var_cs = 0, ldgv = 1 is
 *            accepted too: gvar[s] is then the derivative w.r.t. the row's one variance, the fixed-order sum
 *            of the p columns (what mfgp_gpr_posterior_predict_vjp takes as gvar).
 *   info     [ns]: 0, or the 1-based index of the first output with a non-positive / non-finite pivot (dense
 *            form) or total variance (diagonal form) or a non-finite residual; that row's outputs are then
 *            unspecified, the other rows are unaffected.
 * Dense form (obs_cov given): p <= 128, beyond that MFGP_ERR_ARG -- the form is not built for larger p.  One
 * workgroup per row: Sigma_s is formed in LDS, factored there in 8-column blocks with r carried along as one
 * more row (the forward solve and the quadratic form come out of the factorization itself), and, with a
 * gradient asked for, the factor is inverted in place.  The LDS size is chosen at launch from p (34 KB at
 * p = 64: four workgroups per CU; 134 KB at p = 128).  Diagonal form (obs_cov NULL): any p, one wave per row,
 * no factorization; an output whose target Y(s, c) is NaN is left out (no term, both gradients 0: a row with
 * no target at all has logp = 0).  One launch either way.  Fixed-order sums and no floating-point atomics:
 * a row's bits do not depend on ns or on the other rows.  Nothing is allocated, no synchronisation, no host
 * read of a device word; the workspace is reserved (mfgp_mvn_logpdf_workspace_size; the kernels keep
 * everything on chip).  ns = 0: a no-op (MFGP_OK, decided before the pointers are looked at).  A negative
 * count, p < 1, a short leading dimension or stride, or a null required pointer: MFGP_ERR_ARG; a workspace
 * smaller than the size call reports: MFGP_ERR_WORKSPACE; both before any device work.
 * Replaces: gpflow GPModel.predict_log_density / Gaussian._predict_log_density (the diagonal form) and the
 * torch.linalg.cholesky + cholesky_solve + autograd formulation of an emulator likelihood (the dense form). */
int mfgp_mvn_logpdf_workspace_size(mfgp_handle_t h, int ns, int p, size_t* bytes);
int mfgp_mvn_logpdf(mfgp_handle_t h, int ns, int p, const double* mean, int ldm, const double* Y, long y_rs,
                    const double* var, long var_rs, long var_cs, const double* obs_var, long ov_rs,
                    const double* obs_cov, int ldc, void* ws, size_t ws_bytes, double* logp, double* gmean, int ldgm,
                    double* gvar, int ldgv, int* info /* [ns] */);

/* Batched Fisher (Gauss-Newton) matrix of an emulated data vector: per row s < ns, with Sigma_s as in
 * mfgp_mvn_logpdf and J_s [p x d] the Jacobian of the mean w.r.t. the d inputs,
 *   F[s] = J_s^T Sigma_s^{-1} J_s                          [d x d], exactly symmetric.
 *   J        [ns][d][ldj], ldj >= p: J[s][k][c] = d mean(s, c) / d x(s, k), outputs fastest -- the layout the
 *            mfgp_*_jacobian entries write.
 *   var / obs_var / obs_cov  addressed as mfgp_mvn_logpdf addresses them (var_cs = 0: one variance per row).
 *   F        [ns][d][d], dense.
 *   info     [ns]: 0, or the 1-based index of the first output with a non-positive / non-finite pivot (dense
 *            form) or total variance (diagonal form); that row's F is then unspecified, the others unaffected.
 * Dense form (obs_cov given): one workgroup per row.  Sigma_s is formed in LDS as mfgp_mvn_logpdf forms it,
 * the d rows of J_s^T are put under it and the 8-column block Cholesky carries them along: they become
 * J^T L^{-T} and their own trailing updates leave -F[s] in the d x d corner, so F costs no pass of its own;
 * the corner's lower triangle is negated and mirrored.  The LDS image is (P8 + d) x ((P8 + d) | 1) doubles,
 * P8 = p rounded up to 8, chosen at launch (44.4 KB at p = 64, d = 10).  Limit: p <= 128 AND the image within
 * the 160 KiB of a compute unit, i.e. P8 + d <= 143 (p = 128: d <= 15; p <= 104: any d <= 32); beyond it
 * MFGP_ERR_ARG -- use the diagonal form.  Diagonal form (obs_cov NULL): any p,
 * F[a][b] = sum_c J[c][a] J[c][b] / (var_c + obs_var_c) in output order.  One launch either way; fixed-order
 * sums, no floating-point atomics: a row's bits do not depend on ns or on the other rows.  Nothing is
 * allocated, no synchronisation, no host read of a device word; the workspace is reserved
 * (mfgp_mvn_fisher_workspace_size).  ns = 0: a no-op (MFGP_OK, decided before the pointers are looked at).
 * d outside 1..MFGP_MAX_D: MFGP_ERR_DIM; a negative count, p < 1, a short leading dimension or stride, or a
 * null required pointer: MFGP_ERR_ARG; a short workspace: MFGP_ERR_WORKSPACE; all before any device work.
 * This is the mean term of the Gaussian Fisher information; the 1/2 tr(Sigma^-1 dSigma Sigma^-1 dSigma) term
 * of a variance that depends on x is not formed.
 * Replaces: d one-hot VJPs + torch.linalg.cholesky / cholesky_solve on an [ns, p, p] batch. */
int mfgp_mvn_fisher_workspace_size(mfgp_handle_t h, int ns, int p, int d, size_t* bytes);
int mfgp_mvn_fisher(mfgp_handle_t h, int ns, int p, int d, const double* J, int ldj, const double* var, long var_rs,
                    long var_cs, const double* obs_var, long ov_rs, const double* obs_cov, int ldc, void* ws,
                    size_t ws_bytes, double* F, int* info /* [ns] */);

/* SVGP ELBO value (GPflow SVGP.elbo, whiten=True, Gaussian likelihood) for the
 * latent LinearCoregionalization model (mfgpflow/linear_svgp.py:64-203) and the
 * SingleBinSVGP (SeparateIndependent, mfgpflow/singlebin_svgp.py:13-97, W = I):
 *   thetas [L][2d+4] per-latent constrained kernel parameters (noise entry unused),
 *   Z [M, d+1], q_mu [M, L], q_sqrt [L, M, M] (lower used), W [P, L] or NULL
 *   (identity mixing; requires L == P).  out = [elbo, KL, VE]; g_mu / g_var
 *   [L][N] receive the latent predictive moments.
 * Leading dimensions, for this and every mfgp_svgp_elbo* entry below (value and gradient alike):
 * X [n][ldx] and Z [m][ldz] with ldx, ldz >= d + 1, Y [n][ldy] with ldy >= p; anything shorter is
 * MFGP_ERR_ARG before any device work. */
int mfgp_svgp_workspace_size(mfgp_handle_t h, int n, int m, int l, int p, int d, size_t* bytes);
int mfgp_svgp_elbo(mfgp_handle_t h, int n, int m, int l, int p, int d, const double* X, int ldx, const double* Y,
                   int ldy, const double* Z, int ldz, const double* thetas, const double* q_mu,
                   const double* q_sqrt, const double* W, double noise, double scale, double jitter, void* ws,
                   size_t ws_bytes, double* out, double* g_mu, double* g_var, int* info);

/* Gradient of the same objective (the GradientTape of LatentMFCoregionalizationSVGP.optimize,
 * mfgpflow/linear_svgp.py:181-191, and SingleBinSVGP.optimize, singlebin_svgp.py:81-86)
 * E = VE * scale - kl_mult * KL (kl_mult = 1: the ELBO) with respect to the CONSTRAINED
 * parameters: gZ [M][d+1] (fidelity column 0), gtheta [L][2d+4] (noise slot 0),
 * gq_mu [M][L], gq_sqrt [L][M][M] (lower part), gW [P][L] (unused if W == NULL), gnoise [1].
 * noise is a DEVICE pointer (so a training step can be graph-captured).  out / g_mu / g_var
 * as mfgp_svgp_elbo (out[0] is the plain ELBO).  Workspace: mfgp_svgp_grad_workspace_size. */
int mfgp_svgp_grad_workspace_size(mfgp_handle_t h, int n, int m, int l, int p, int d, size_t* bytes);
int mfgp_svgp_elbo_grad(mfgp_handle_t h, int n, int m, int l, int p, int d, const double* X, int ldx,
                        const double* Y, int ldy, const double* Z, int ldz, const double* thetas,
                        const double* q_mu, const double* q_sqrt, const double* W, const double* noise,
                        double scale, double kl_mult, double jitter, void* ws, size_t ws_bytes, double* out, double* g_mu,
                        double* g_var, double* gZ, double* gtheta, double* gq_mu, double* gq_sqrt, double* gW,
                        double* gnoise, int* info);
/* Layout of mfgp_svgp_elbo_grad's q_sqrt (input) and gq_sqrt (output) on this handle: 0 (default)
 * [L][M][M] (lower part used / written, upper zero), 1 packed lower triangles [L][M(M+1)/2], entry
 * (i, j <= i) at i(i+1)/2 + j -- the size of GPflow's unconstrained q_sqrt variable (the
 * FillTriangular bijector's vector; q_sqrt of singlebin_svgp.py:57-62 and GPflow SVGP), so a training
 * state's parameter, gradient and Adam moments hold no upper halves.  Other entry points always
 * take [L][M][M]. */
int mfgp_set_svgp_qs_packed(mfgp_handle_t h, int packed);

/* The same ELBO and gradient with the HeteroscedasticGaussian likelihood: every observation has
 * its own noise variance v[n][c] = noise + Yunc[n][c]^2 (the baseline plus the SQUARED uncertainty,
 * as the reference's code computes it; its docstring says "+ Y_unc"),
 *   VE = sum_{n,c} -1/2 log 2 pi - 1/2 log v - 1/2 ((y - f_mu)^2 + f_var) / v.
 * Yunc [n][ldu] is read for columns 0..p-1 (ldu >= p); a caller holding the reference's combined
 * targets [Y_obs | Y_unc] of shape [N, 2P] passes Y + P with ldu = ldy.  Yunc == NULL is the
 * homoscedastic call (mfgp_svgp_elbo / mfgp_svgp_elbo_grad, bit for bit).  gnoise is the gradient
 * with respect to the baseline.  qs_packed (0 / 1) is the q_sqrt / gq_sqrt layout of THIS call as
 * mfgp_set_svgp_qs_packed describes it; the handle's setting is not read.  The reverse pass of the
 * variational expectations is one row-tiled kernel whose LDS holds a row of r and 1/v:
 * MFGP_ERR_DIM if 2 (p|1) + 4 l > 4000.  Workspaces: mfgp_svgp_workspace_size /
 * mfgp_svgp_grad_workspace_size.
 * Replaces: mfgpflow/linear_svgp.py:223-267 (HeteroscedasticGaussian._variational_expectations
 * under SVGP.elbo and the GradientTape of optimize, linear_svgp.py:181-191). */
int mfgp_svgp_elbo_het(mfgp_handle_t h, int n, int m, int l, int p, int d, const double* X, int ldx, const double* Y,
                       int ldy, const double* Yunc, int ldu, const double* Z, int ldz, const double* thetas,
                       const double* q_mu, const double* q_sqrt, const double* W, double noise, double scale,
                       double jitter, void* ws, size_t ws_bytes, double* out, double* g_mu, double* g_var, int* info);
int mfgp_svgp_elbo_grad_het(mfgp_handle_t h, int n, int m, int l, int p, int d, const double* X, int ldx,
                            const double* Y, int ldy, const double* Yunc, int ldu, const double* Z, int ldz,
                            const double* thetas, const double* q_mu, const double* q_sqrt, int qs_packed,
                            const double* W, const double* noise, double scale, double kl_mult, double jitter,
                            void* ws, size_t ws_bytes, double* out, double* g_mu, double* g_var, double* gZ,
                            double* gtheta, double* gq_mu, double* gq_sqrt, double* gW, double* gnoise, int* info);

/* The same ELBO and gradient with the MaskedGaussian likelihood: a NaN in Y is a missing observation,
 * and every output has its own noise variance.  With obs[n][c] = !isnan(Y[n][c]) and
 * s2[c] = noise[pn == 1 ? 0 : c],
 *   VE = sum_{obs} -1/2 log 2 pi - 1/2 log s2[c] - 1/2 ((y - f_mu)^2 + f_var) / s2[c];
 * a missing entry adds exactly 0 to the value and to every gradient, and ELBO = VE scale - kl_mult KL
 * with the caller's scale (num_data / n: n counts rows, not observed entries).  noise is a DEVICE
 * vector of pn entries, pn = 1 (one shared variance) or pn = p (one per output); any other pn is
 * MFGP_ERR_ARG.  gnoise [pn] is the gradient with respect to noise; an output with no observed entry
 * gets exactly 0.  Y [n][ldy], ldy >= p.  qs_packed (0 / 1) is the q_sqrt / gq_sqrt layout of THIS
 * call as mfgp_set_svgp_qs_packed describes it; the handle's setting is not read.  The reverse pass of
 * the variational expectations is one row-tiled kernel whose LDS holds a row of r, obs / s2 and the
 * noise-gradient terms: MFGP_ERR_DIM if 3 (p|1) + 4 l > 4000.  No atomics: gradients are bitwise
 * reproducible and do not depend on the workspace contents.  Workspaces: mfgp_svgp_workspace_size /
 * mfgp_svgp_grad_workspace_size.
 * Replaces: notebooks/demo: missing output.ipynb, cell 2 (MaskedGaussian._variational_expectations
 * under SVGP.elbo, and the GradientTape of that cell's optimize). */
int mfgp_svgp_elbo_masked(mfgp_handle_t h, int n, int m, int l, int p, int d, const double* X, int ldx,
                          const double* Y, int ldy, const double* Z, int ldz, const double* thetas, const double* q_mu,
                          const double* q_sqrt, const double* W, const double* noise, int pn, double scale,
                          double jitter, void* ws, size_t ws_bytes, double* out, double* g_mu, double* g_var,
                          int* info);
int mfgp_svgp_elbo_grad_masked(mfgp_handle_t h, int n, int m, int l, int p, int d, const double* X, int ldx,
                               const double* Y, int ldy, const double* Z, int ldz, const double* thetas,
                               const double* q_mu, const double* q_sqrt, int qs_packed, const double* W,
                               const double* noise, int pn, double scale, double kl_mult, double jitter, void* ws,
                               size_t ws_bytes, double* out, double* g_mu, double* g_var, double* gZ, double* gtheta,
                               double* gq_mu, double* gq_sqrt, double* gW, double* gnoise, int* info);

/* One Keras-2.10 (legacy) Adam step on a packed parameter vector (the apply_gradients of
 * the SVGP optimize loops, linear_svgp.py:190 / singlebin_svgp.py:86): u unconstrained,
 * c constrained with transform[q] = 0 identity, 1 Softplus, 2 Shift(1e-6) o Softplus, 3 Sigmoid;
 * g = d(+objective)/dc (e.g. the mfgp_svgp_elbo_grad outputs laid out in c's packing);
 * entries with trainable[q] == 0 are left alone; span (may be NULL) ties contiguous entries
 * to one variable (isotropic lengthscales): span[q] = k > 0 for a variable of k entries
 * starting at q (gradient summed, value written to all k), 0 for its followers; learning
 * rate lr_sched[*step] (device array, e.g. the float32 CosineDecay schedule).  Then loss_hist[*step] =
 * -out[0] + (kl_mult - 1) out[1], kl_hist[*step] = out[1] (either may be NULL) and ++*step. */
int mfgp_adam_packed(mfgp_handle_t h, int n, double* u, double* c, const double* g, double* m, double* v,
                     const unsigned char* trainable, const unsigned char* transform, const unsigned char* span,
                     int* step,
                     const double* lr_sched, double beta1, double beta2, double eps, const double* out,
                     double kl_mult, double* loss_hist, double* kl_hist);
/* mfgp_adam_packed gated on the evaluation's info words (info[0..ninfo), e.g. the per-latent
 * Cholesky info of mfgp_svgp_elbo_grad or the info of mfgp_gpr_lml): if any is nonzero the step
 * leaves u / c / m / v and the step counter unchanged (loss_hist[step] still records the loss),
 * like the fused step of mfgp_gpr_adam_step: a session can tell lost steps by the counter. */
int mfgp_adam_packed_ex(mfgp_handle_t h, int n, double* u, double* c, const double* g, double* m, double* v,
                        const unsigned char* trainable, const unsigned char* transform, const unsigned char* span,
                        int* step, const double* lr_sched, double beta1, double beta2, double eps,
                        const double* out, double kl_mult, double* loss_hist, double* kl_hist, const int* info,
                        int ninfo);

/* SVGP.predict_f(Xnew, full_cov, full_output_cov) covariance forms (GPflow base_conditional_with_lm
 * full_cov branch per latent, G_l = Knn_l - A^T A + (Lq^T A)^T Lq^T A, then mix_latent_gp):
 *   mode 1 (full_cov)            f_cov [P][nstar][nstar]     = sum_l W_pl^2 G_l
 *   mode 2 (full_output_cov)     f_cov [nstar][P][P]         = sum_l W_pl W_ql g_var_l
 *   mode 3 (both)                f_cov [nstar][P][nstar][P]  = sum_l W_pl W_ql G_l
 * W == NULL: independent outputs (SeparateIndependent, P == l).  Also writes the diagonal outputs
 * of mfgp_svgp_predict (g_mu, g_var, f_mu, f_var).
 * Workspace: mfgp_svgp_predict_cov_workspace_size(h, nstar, m, l, p, d).
 * Replaces: gpflow SVGP.predict_f(full_cov / full_output_cov) inherited by
 * mfgpflow/linear_svgp.py:64 and singlebin_svgp.py:13. */
int mfgp_svgp_predict_cov_workspace_size(mfgp_handle_t h, int nstar, int m, int l, int p, int d, size_t* bytes);
int mfgp_svgp_predict_cov(mfgp_handle_t h, int mode, int nstar, int m, int l, int p, int d, const double* Xs,
                          int ldxs, const double* Z, int ldz, const double* thetas, const double* q_mu,
                          const double* q_sqrt, const double* W, double jitter, void* ws, size_t ws_bytes,
                          double* g_mu, double* g_var, double* f_mu, double* f_var, double* f_cov, int* info);

/* SVGP.predict_f(Xnew, full_cov=False) of the same models (GPflow posteriors with
 * mix_latent_gp): latent moments g_mu / g_var [L][nstar] and mixed f_mu / f_var
 * [nstar][P].  Workspace: mfgp_svgp_workspace_size(h, nstar, m, l, p, d). */
int mfgp_svgp_predict(mfgp_handle_t h, int nstar, int m, int l, int p, int d, const double* Xs, int ldxs,
                      const double* Z, int ldz, const double* thetas, const double* q_mu, const double* q_sqrt,
                      const double* W, double jitter, void* ws, size_t ws_bytes, double* g_mu, double* g_var,
                      double* f_mu, double* f_var, int* info);

/* ---- Cached posterior (GPflow model.posterior()): the X*-independent work of predict_f done once.
 * A cache is a self-contained device block (training inputs / inducing points, kernel parameters,
 * inverse factor, projected targets): the predict calls read nothing else of the model, run no
 * Gram of X, no factorization, write no info and allocate nothing.  The block is laid out for the
 * handle's tile size (mfgp_set_tile) at build time; predict with the same tile size.  Two predict
 * calls with the same inputs return the same bits (fixed-order sums, no floating-point atomics).
 *
 * GPR (nlf = 0: LinearMultiFidelityKernel, fp64; nlf = m: graph kernel with m LF sources):
 *   build    runs the Gram + factor of mfgp_gpr_predict once and stores X, theta, L^{-1} (lower
 *            tiles) and Z = L^{-1} Y.  ws: at least mfgp_gpr_predict_cov_workspace_size(h, nlf, n, p,
 *            d, 1) bytes.  info as mfgp_gpr_predict (nonzero: the cache is not usable).
 *   predict  A = L^{-1} K(X, X*) with K generated inside the product kernel, mean [nstar x p] (ldm)
 *            = A^T Z, var [nstar] = K_diag(X*) - colsum(A^2); cov (may be NULL) [nstar x nstar] (ldc)
 *            = K(X*, X*) - A^T A.  Two launches when cov is NULL.
 * A cache or workspace smaller than the *_size calls report: MFGP_ERR_WORKSPACE, before any device work. */
int mfgp_gpr_posterior_size(mfgp_handle_t h, int nlf, int n, int p, int d, size_t* bytes);
int mfgp_gpr_posterior_build(mfgp_handle_t h, int nlf, int n, int p, int d, const double* X, int ldx, const double* Y,
                             int ldy, const double* theta, void* ws, size_t ws_bytes, void* cache, size_t cache_bytes,
                             int* info);
int mfgp_gpr_posterior_predict_workspace_size(mfgp_handle_t h, int nlf, int n, int p, int d, int nstar,
                                              size_t* bytes);
int mfgp_gpr_posterior_predict(mfgp_handle_t h, int nlf, int n, int p, int d, int nstar, const void* cache,
                               size_t cache_bytes, const double* Xs, int ldxs, void* ws, size_t ws_bytes, double* mean,
                               int ldm, double* var, double* cov, int ldc);
/* SVGP (arguments as mfgp_svgp_predict): build factors every K_uu and stores Z, thetas, W, q_mu,
 * Lm^{-1} and C = tril(q_sqrt)^T Lm^{-1} per latent (ws: at least mfgp_svgp_workspace_size(h, 1, m, l,
 * p, d) bytes; info [l]).  predict writes the marginal f_mu / f_var [nstar][p] of mfgp_svgp_predict;
 * mixed: 1 when the cache was built with a W (LinearCoregionalization), 0 for independent outputs. */
int mfgp_svgp_posterior_size(mfgp_handle_t h, int m, int l, int p, int d, size_t* bytes);
int mfgp_svgp_posterior_build(mfgp_handle_t h, int m, int l, int p, int d, const double* Z, int ldz,
                              const double* thetas, const double* q_mu, const double* q_sqrt, const double* W,
                              double jitter, void* ws, size_t ws_bytes, void* cache, size_t cache_bytes, int* info);
int mfgp_svgp_posterior_predict_workspace_size(mfgp_handle_t h, int nstar, int m, int l, int p, int d, size_t* bytes);
int mfgp_svgp_posterior_predict(mfgp_handle_t h, int nstar, int m, int l, int p, int d, int mixed, const void* cache,
                                size_t cache_bytes, const double* Xs, int ldxs, void* ws, size_t ws_bytes,
                                double* f_mu, double* f_var);

/* Input gradients of the cached predict calls: the vector-Jacobian product w.r.t. Xs.
 * Arguments as the predict calls (GPR: no cov), plus the upstream gradients gmean [nstar x p]
 * (ldgm) and gvar (GPR: [nstar], the derivative w.r.t. var; SVGP: [nstar x p] dense) -- either may be
 * NULL, meaning zero -- and the output gX [nstar x (d + 1)] (ldgx):
 *   gX[s][k] = sum_c gmean[s][c] dmean[s][c] / dXs[s][k] + (sum_c) gvar[s][(c)] dvar[s][(c)] / dXs[s][k].
 * The fidelity column of Xs enters only through exact == 0 / == 1 tests: gX[s][d] = 0.  mean / var
 * (f_mu / f_var) are written by the predict calls' own forward code (the same bits).  One more
 * launch behind the predict call's two; no floating-point atomics, so two calls with the same
 * inputs return the same bits.  Workspace: the *_vjp_workspace_size calls (MFGP_ERR_WORKSPACE
 * before any device work when smaller); nothing is allocated, no device word is read by the host;
 * nstar = 0 is a no-op.  The graph kernel (nlf > 0) is not supported: MFGP_ERR_ARG. */
int mfgp_gpr_posterior_predict_vjp_workspace_size(mfgp_handle_t h, int nlf, int n, int p, int d, int nstar,
                                                  size_t* bytes);
int mfgp_gpr_posterior_predict_vjp(mfgp_handle_t h, int nlf, int n, int p, int d, int nstar, const void* cache,
                                   size_t cache_bytes, const double* Xs, int ldxs, void* ws, size_t ws_bytes,
                                   double* mean, int ldm, double* var, const double* gmean, int ldgm,
                                   const double* gvar, double* gX, int ldgx);
int mfgp_svgp_posterior_predict_vjp_workspace_size(mfgp_handle_t h, int nstar, int m, int l, int p, int d,
                                                   size_t* bytes);
int mfgp_svgp_posterior_predict_vjp(mfgp_handle_t h, int nstar, int m, int l, int p, int d, int mixed,
                                    const void* cache, size_t cache_bytes, const double* Xs, int ldxs, void* ws,
                                    size_t ws_bytes, double* f_mu, double* f_var, const double* gmean, int ldgm,
                                    const double* gvar, double* gX, int ldgx);

/* Emulator log-likelihood from the cached posterior: logp[s] = log N(Y(s, .) | mean(Xs_s), diag(var(Xs_s) +
 * obs_var(s, .)) + obs_cov), and optionally its gradient w.r.t. Xs, from one call.  Arguments as the predict
 * calls, then Y / obs_var / obs_cov / logp / info as mfgp_mvn_logpdf takes them.  Enqueues, in order: the
 * predict calls' own forward (mean / var, f_mu / f_var carry the predict calls' bits), the density launch
 * on them, and -- with gX [nstar x (d + 1)] (ldgx) given -- k_post_grad fed the density's gmean / gvar,
 * which live in the workspace (GPR: gvar is the [nstar] sum over the outputs that share the one variance).
 * gX is bitwise what *_predict_vjp returns for those upstream gradients; the forward runs once.  gX = NULL:
 * the call ends behind the density launch.  The emulator's own likelihood noise is NOT added: pass it in
 * obs_var.  The graph kernel (nlf > 0) has the value only: a gX there is MFGP_ERR_ARG.  nstar = 0 is a
 * no-op; argument and workspace errors as the VJP calls and mfgp_mvn_logpdf, before any device work. */
int mfgp_gpr_posterior_logdens_workspace_size(mfgp_handle_t h, int nlf, int n, int p, int d, int nstar,
                                              size_t* bytes);
int mfgp_gpr_posterior_logdens(mfgp_handle_t h, int nlf, int n, int p, int d, int nstar, const void* cache,
                               size_t cache_bytes, const double* Xs, int ldxs, void* ws, size_t ws_bytes, double* mean,
                               int ldm, double* var, const double* Y, long y_rs, const double* obs_var, long ov_rs,
                               const double* obs_cov, int ldc, double* logp, double* gX, int ldgx, int* info);
int mfgp_svgp_posterior_logdens_workspace_size(mfgp_handle_t h, int nstar, int m, int l, int p, int d, size_t* bytes);
int mfgp_svgp_posterior_logdens(mfgp_handle_t h, int nstar, int m, int l, int p, int d, int mixed, const void* cache,
                                size_t cache_bytes, const double* Xs, int ldxs, void* ws, size_t ws_bytes,
                                double* f_mu, double* f_var, const double* Y, long y_rs, const double* obs_var,
                                long ov_rs, const double* obs_cov, int ldc, double* logp, double* gX, int ldgx,
                                int* info);

/* Emulator Jacobian from the cached posterior: J[s][k][c] = d mean(Xs_s)[c] / d Xs[s][k] over the d input
 * columns (the fidelity column enters only through exact == 0 / == 1 tests and has no slot), linear
 * multi-fidelity kernel.  With wL = cL vL kL and wD = cD vD kD the two terms of the kernel entry
 * (cL = 1 | rho | rho^2, cD = 1 for HF x HF):
 *   GPR   alpha = L^{-T} Z [n x p];   J[s][k][c] = sum_i alpha[i][c] (wL(i, s) / lL_k^2 + wD(i, s) / lD_k^2)
 *                                                  (x[i][k] - Xs[s][k])
 *   SVGP  alpha_l = Lm_l^{-T} q_mu[:, l];  dg_l[s][k] the same sum with alpha_l and latent l's parameters;
 *         J[s][k][c] = sum_l W[c][l] dg_l[s][k] in latent order (mixed = 0: J[s][k][l] = dg_l[s][k]).
 * A row of either side whose fidelity is neither 0 nor 1 contributes exactly 0.
 *   *_jacobian_weights  computes alpha from the cache block into `weights` (one launch: a transposed-
 *            triangular tile product on the matrix core).  It depends on the cache block alone: compute it
 *            once per block and pass it to every Jacobian call; recompute it whenever the block is rebuilt.
 *            *_jacobian_weights_workspace_size reports the bytes of `weights` (GPR: Npad x Ppad doubles;
 *            SVGP: l x Mpad); the call needs no other workspace.  The cache block is not written.
 *   *_jacobian  arguments as the predict calls (GPR: no cov) plus the weights and J [nstar][d][ldj], ldj >= p,
 *            outputs fastest (the layout mfgp_mvn_fisher reads).  Enqueues the predict calls' own forward
 *            (mean / var, f_mu / f_var carry the predict calls' bits), then GPR: one memset of the task
 *            counters and one launch -- per (column tile of Xs, output tile, chunk of row tiles, group of
 *            input dimensions) the wL / wD tiles are generated in LDS, G_k = (wL / lL_k^2 + wD / lD_k^2)
 *            (x_ik - Xs_sk) is formed as the matrix core's operand and acc_k += G_k^T alpha_tile; chunk partials
 *            are summed in chunk order by the last workgroup to arrive (no spin-wait); SVGP: one launch for the
 *            latents' dg_l partials, one that sums the chunks (more than one chunk only), one that mixes.
 *            The chunk count depends on the shapes alone, every sum has a fixed order and there are no
 *            floating-point atomics: two calls with the same inputs return the same bits.
 * Workspace: the *_jacobian_workspace_size calls.  A cache, weights buffer or workspace smaller than the size
 * calls report: MFGP_ERR_WORKSPACE; argument errors MFGP_ERR_ARG / MFGP_ERR_DIM; both before any device work.
 * Nothing is allocated, the host reads no device word; nstar = 0 is a no-op.  The graph kernel (nlf > 0) is
 * not supported: MFGP_ERR_ARG.  Use the cache and the weights at the tile size they were built for. */
int mfgp_gpr_jacobian_weights_workspace_size(mfgp_handle_t h, int nlf, int n, int p, int d, size_t* bytes);
int mfgp_gpr_jacobian_weights(mfgp_handle_t h, int nlf, int n, int p, int d, const void* cache, size_t cache_bytes,
                              void* weights, size_t weights_bytes);
int mfgp_gpr_jacobian_workspace_size(mfgp_handle_t h, int nlf, int n, int p, int d, int nstar, size_t* bytes);
int mfgp_gpr_jacobian(mfgp_handle_t h, int nlf, int n, int p, int d, int nstar, const void* cache, size_t cache_bytes,
                      const void* weights, size_t weights_bytes, const double* Xs, int ldxs, void* ws, size_t ws_bytes,
                      double* mean, int ldm, double* var, double* J, int ldj);
int mfgp_svgp_jacobian_weights_workspace_size(mfgp_handle_t h, int m, int l, int p, int d, size_t* bytes);
int mfgp_svgp_jacobian_weights(mfgp_handle_t h, int m, int l, int p, int d, int mixed, const void* cache,
                               size_t cache_bytes, void* weights, size_t weights_bytes);
int mfgp_svgp_jacobian_workspace_size(mfgp_handle_t h, int nstar, int m, int l, int p, int d, size_t* bytes);
int mfgp_svgp_jacobian(mfgp_handle_t h, int nstar, int m, int l, int p, int d, int mixed, const void* cache,
                       size_t cache_bytes, const void* weights, size_t weights_bytes, const double* Xs, int ldxs,
                       void* ws, size_t ws_bytes, double* f_mu, double* f_var, double* J, int ldj);

/* Leave-group-out cross-validation from a GPR cache, at the cache's hyper-parameters: for each group
 * S of training rows, what a model built without those rows predicts for them, in closed form from
 * the cached L^{-1} and Z alone (C = L^{-1}[:, S], G = C^T C, H = C^T Z): no Gram, no factorization
 * of K, no kernel evaluation, for nlf = 0 and nlf > 0 alike.
 *   offsets [ngroups + 1], rows [nrows]: device ints; group g is rows[offsets[g] .. offsets[g + 1]),
 *            1 .. gmax (<= 32) distinct training-row indices, offsets[0] = 0, offsets[ngroups] = nrows.
 *            A row may appear in several groups.
 *   resid    [nrows x p] (ldr): E = y_S - mean_{S|-S} = G^{-1} H; the held-out mean is Y[rows] - resid.
 *   cov      [nrows x gmax] (ldc; may be NULL): row r holds its row of its group's latent covariance
 *            Sigma_f = G^{-1} - s2 I (s2: the cached likelihood variance; what predict_f(full_cov) of
 *            the model without S returns), zero beyond the group's size.
 *   logdens  [ngroups x p]: the joint log predictive density of the group's observations per output,
 *            -1/2 H_c^T G^{-1} H_c + 1/2 log det G - |S| / 2 log 2 pi.
 *   info     [ngroups]: 0, or the first non-positive pivot of the group's G (1-based within the
 *            group); -1 on every group when the table is malformed (a size outside 1..gmax, a row
 *            outside 0..n-1): nothing else is written then.
 * Two launches; fixed-order sums and no floating-point atomics (the same inputs give the same bits);
 * nothing is allocated, the cache is only read, the host reads no device word.  gmax > 32 or a
 * non-positive count: MFGP_ERR_ARG; a cache or workspace smaller than the *_size calls report:
 * MFGP_ERR_WORKSPACE before any device work; ngroups = 0 is a no-op.  Use the cache at the tile size
 * it was built for. */
int mfgp_gpr_posterior_leave_out_workspace_size(mfgp_handle_t h, int nlf, int n, int p, int d, int ngroups, int nrows,
                                                size_t* bytes);
int mfgp_gpr_posterior_leave_out(mfgp_handle_t h, int nlf, int n, int p, int d, const void* cache, size_t cache_bytes,
                                 int ngroups, const int* offsets, const int* rows, int nrows, int gmax, void* ws,
                                 size_t ws_bytes, double* resid, int ldr, double* cov, int ldc, double* logdens,
                                 int* info);

/* Simulation design from a GPR cache, at the cache's hyper-parameters: how much one more observation at
 * each candidate input lowers the posterior variance of f over a weighted reference set, in closed
 * form from the cached factors (no refit), for nlf = 0 and nlf > 0 alike.
 *   Xall    [(nref + ncand) x (d + 1)] (ldx): the reference rows, then the candidate rows.  The fidelity
 *           column of a candidate says which simulation is run, that of a reference whose error is
 *           bought down.
 *   w       [nref] weights >= 0 (NULL: ones).
 *   score   [ncand]: score[c] = sum_r w[r] C(r, c)^2 / (v(c) + s2), where C is the [ref, cand] block of
 *           the cov that mfgp_gpr_posterior_predict returns for Xall (K(Xref, Xcand) - A_ref^T A_cand, the
 *           kernel's entry function in that argument order, no jitter), v the marginal var of the
 *           candidate and s2 the cached likelihood variance.  A row whose fidelity is no source of the
 *           kernel has a zero kernel row: such a candidate scores exactly 0, such a reference adds
 *           exactly 0.  The nref x ncand block is formed tile by tile on chip, never in memory.
 *   E       [k x (nref + ncand)] (ldE; may be NULL when k = 0): the conditioning rows of the k candidates
 *           already picked in this batch, as design_append wrote them; C and v are then those after
 *           observing the picks: C - E_ref^T E_cand, v - colsum(E_cand^2).  k <= 32.
 *   refresh 1: run the predict call's forward on Xall and keep A = L^{-1} K(X, Xall) and v in ws;
 *           0: reuse them.  Between a refresh = 1 call and the refresh = 0 / design_append calls that
 *           rely on it, ws must not be touched by anything else, and the geometry, the cache and Xall
 *           must be the same.
 *   design_append  writes row k (< 32) of E for the candidate pick[0] (a device int: the host reads no
 *           device word inside a batch): e(x) = C'(x, c*) / sqrt(v'(c*) + s2) over the nref + ncand
 *           stacked columns, primes meaning "after rows 0..k-1".  A candidate may be picked again (a
 *           replicate).  An index outside 0..ncand-1 writes a zero row.  Needs a refresh = 1 score call first.
 * One launch behind the forward's two (score), one launch (append), each after one memset of the arrival
 * counters; fixed-order sums and no floating-point atomics (the same inputs give the same bits); nothing
 * is allocated, the cache is only read.  A negative count, k > 32 (append: k > 31) or nlf outside
 * 0..MFGP_MAX_LF: MFGP_ERR_ARG; a cache or workspace smaller than the *_size calls report:
 * MFGP_ERR_WORKSPACE before any device work; ncand = 0 is a no-op, nref = 0 writes zeros.  qmax (<= 32):
 * the largest k the workspace will be used with.  Use the cache at the tile size it was built for. */
int mfgp_gpr_posterior_design_workspace_size(mfgp_handle_t h, int nlf, int n, int p, int d, int nref, int ncand,
                                             int qmax, size_t* bytes);
int mfgp_gpr_posterior_design_score(mfgp_handle_t h, int nlf, int n, int p, int d, const void* cache,
                                    size_t cache_bytes, const double* Xall, int ldx, int nref, int ncand,
                                    const double* w, const double* E, int ldE, int k, void* ws, size_t ws_bytes,
                                    double* score, int refresh);
int mfgp_gpr_posterior_design_append(mfgp_handle_t h, int nlf, int n, int p, int d, const void* cache,
                                     size_t cache_bytes, const double* Xall, int ldx, int nref, int ncand, void* ws,
                                     size_t ws_bytes, const int* pick, double* E, int ldE, int k);

/* Block append to a GPR cache: the cache of the n + k rows [X ; Xadd], [Y ; Yadd] at the cached
 * hyper-parameters, from the cached factors in O(n^2 k) (no Gram of X, no factorization of K), for
 * nlf = 0 and nlf > 0 alike.  1 <= k <= 32.
 *   Xadd      [k x (d + 1)] (ldxa), fidelity in the last column.
 *   Yadd      [k x p] (ldya), or NULL: the rows are observed at the cache's own mean at Xadd (a
 *             fantasy): their rows of Z are exactly zero, the mean of the new cache is the old one
 *             and its variance is that of a refit.
 *   out_cache the new block, laid out as mfgp_gpr_posterior_build lays out n + k rows
 *             (mfgp_gpr_posterior_size(n + k) bytes); every byte of it is written.  It must not be
 *             `cache`, which is only read.
 *   mean_add  [k x p] (ldm; may be NULL): the old cache's mean at Xadd.
 *   info      one int: 0; -(r + 1) when row r of Xadd has a fidelity that is no source of the kernel;
 *             the 1-based first non-positive or non-finite pivot of S = K(Xadd, Xadd) + s2 I - A^T A
 *             otherwise.  The new block is not usable unless info is 0.
 * With B the cross block as a factorization of the stacked rows reads it (graph kernel: the new row
 * is the row argument of the entry function; the 1e-6 jitter on the diagonal of K(Xadd, Xadd)):
 * A = L^{-1} B^T, S = L22 L22^T, R = L22^{-1}, new L^{-1} = [L^{-1} 0 ; -R A^T L^{-1}  R], new
 * Z = [Z ; R (Yadd - A^T Z)].  Four launches: the predict call's two on Xadd, one workgroup for S, R and
 * W = -R A^T, and one pass over the cached tiles that copies each to the new row stride and multiplies
 * it into the bottom rows.  Fixed-order sums and no floating-point atomics (the same inputs give the
 * same bits); nothing is allocated, no synchronisation, no host read of a device word.  k outside
 * 1..32, a bad geometry or out_cache == cache: MFGP_ERR_ARG; cache, out_cache or ws smaller than the
 * *_size calls report: MFGP_ERR_WORKSPACE; both before any device work.  Use the cache at the tile
 * size it was built for. */
int mfgp_gpr_posterior_append_workspace_size(mfgp_handle_t h, int nlf, int n, int p, int d, int k, size_t* bytes);
int mfgp_gpr_posterior_append(mfgp_handle_t h, int nlf, int n, int p, int d, int k, const void* cache,
                              size_t cache_bytes, const double* Xadd, int ldxa, const double* Yadd, int ldya, void* ws,
                              size_t ws_bytes, void* out_cache, size_t out_bytes, double* mean_add, int ldm,
                              int* info);

/* Diagnostic: one v_mfma_f64_16x16x4_f64 with A[i][k] = 4i+k+1, B[k][j] = 100k+j;
 * writes C (16x16 row-major, device). */
int mfgp_selftest_mfma(mfgp_handle_t h, double* out);

/* ---- dtype-generic forms (mfgp_mf_gram(h, dtype, ...)).
 * dtype MFGP_F64: X / Y / K / mean / var are double and the call is exactly the fp64 entry point
 * of the same name without "_ex".  dtype MFGP_F32: those arrays are float (device, row-major);
 * theta, out and the Adam state stay double.  The fp32 path is the BASELINE "Synth" config's
 * (N_L = 16384, N_H = 2048, D = 10, P = 512): the reference forces fp64 (linear.py:63-64), so
 * its semantics are the fp64 ones computed in fp32 -- r^2 in direct-difference form (not
 * GPflow's expanded form, which cancels in fp32), every GEMM on v_mfma_f32_32x32x2_f32, the
 * LML / gradient reductions in fp64.  Tolerances against the fp64 oracle: DESIGN.md §8. */
#define MFGP_F64 0
#define MFGP_F32 1
/* fp32 path: 128-wide tile columns per outer Cholesky panel (default 6; env MFGP_F32_PANEL). */
int mfgp_set_f32_panel(mfgp_handle_t h, int tiles);
/* fp32 path: 1 (default; env MFGP_F32_LOOKAHEAD) factors the next panel on a high-priority side
 * stream beside the trailing update (fork / join events, graph-capturable); 0: one stream. */
int mfgp_set_f32_lookahead(mfgp_handle_t h, int enable);
/* fp32 lookahead: CUs the trailing update leaves free for the side stream (default 32; env
 * MFGP_F32_RESERVE; 0: uncapped grid).  Speed only: results do not depend on it. */
int mfgp_set_f32_reserve(mfgp_handle_t h, int cus);
/* LinearMultiFidelityKernel.K (linear.py:55-104), as mfgp_mf_gram. */
int mfgp_mf_gram_ex(mfgp_handle_t h, int dtype, int n1, int n2, int d, const void* X1, int ldx1, const void* X2,
                    int ldx2, const double* theta, double diag_add, void* K, int ldk);
/* GPR.log_marginal_likelihood (+ gradient), as mfgp_gpr_workspace_size / mfgp_gpr_lml. */
int mfgp_gpr_workspace_size_ex(mfgp_handle_t h, int dtype, int n, int p, int d, size_t* bytes);
int mfgp_gpr_lml_ex(mfgp_handle_t h, int dtype, int n, int p, int d, const void* X, int ldx, const void* Y, int ldy,
                    const double* theta, int want_grad, void* ws, size_t ws_bytes, double* out, int* info);
/* One optimize(use_adam=True) iteration (linear.py:200-214), as mfgp_gpr_adam_step. */
int mfgp_gpr_adam_step_ex(mfgp_handle_t h, int dtype, int n, int p, int d, const void* X, int ldx, const void* Y,
                          int ldy, double* theta, double* u, double* m, double* v, const unsigned char* trainable,
                          const int* tie, int* step, double lr, double beta1, double beta2, double eps,
                          double* loss_hist, void* ws, size_t ws_bytes, double* out, int* info);
/* GPR.predict_f(full_cov=False) (linear.py:237-286), as mfgp_gpr_predict; mean / var in dtype. */
int mfgp_gpr_predict_workspace_size_ex(mfgp_handle_t h, int dtype, int n, int p, int d, int nstar, size_t* bytes);
int mfgp_gpr_predict_ex(mfgp_handle_t h, int dtype, int n, int p, int d, int nstar, const void* X, int ldx,
                        const void* Y, int ldy, const void* Xs, int ldxs, const double* theta, void* ws,
                        size_t ws_bytes, void* mean, int ldm, void* var, int* info);
/* predict_f(full_cov=True) in either dtype: mfgp_gpr_predict_cov for MFGP_F64 (any nlf);
 * MFGP_F32 (nlf = 0): cov [nstar x nstar] (ldc) = K(X*, X*) - A^T A computed in fp32 from the
 * same factor sweep as mfgp_gpr_predict_ex.  Workspace: mfgp_gpr_predict_cov_workspace_size_ex. */
int mfgp_gpr_predict_cov_workspace_size_ex(mfgp_handle_t h, int dtype, int nlf, int n, int p, int d, int nstar,
                                           size_t* bytes);
int mfgp_gpr_predict_cov_ex(mfgp_handle_t h, int dtype, int nlf, int n, int p, int d, int nstar, const void* X,
                            int ldx, const void* Y, int ldy, const void* Xs, int ldxs, const double* theta, void* ws,
                            size_t ws_bytes, void* mean, int ldm, void* var, void* cov, int ldc, int* info);
/* Diagnostic: one LML value+grad evaluation with hipEvents around its launches; synchronises.
 * Per phase (HOST arrays of nphase entries): ms, flops performed (fp32 only) and launch count.
 * fp32 phases: [gram, diag factors, panels, in-panel updates, trailing updates, alpha, gradient,
 * reductions]; fp64: mfgp_gpr_lml_phase_times' five phases. */
int mfgp_gpr_phase_times_ex(mfgp_handle_t h, int dtype, int n, int p, int d, const void* X, int ldx, const void* Y,
                            int ldy, const double* theta, void* ws, size_t ws_bytes, double* out, int* info,
                            float* ms, double* flops, int* launches, int nphase);

#ifdef __cplusplus
}
#endif
#endif /* MFGP_H_ */
