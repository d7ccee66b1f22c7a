/* mi_gp.h -- C-ABI of libmi_gp.so, the MI355X (gfx950) GP log-marginal-likelihood backend.
 *
 * The reference (andrew-angus/andvaranaut) has no FFI for this path: the seam is the PyMC model
 * built in GPMCMC.__fit (gpmcmc.py:189-323) and consumed by pm.find_MAP / pm.sample / gp.predict
 * (gpmcmc.py:345,351,593).  In PyMC terms that seam is one value-and-gradient callable
 * theta -> (logp, dlogp) and one conditional (theta, X*) -> (mu*, var*); the entry points below
 * are exactly those two, plus the block-level operations they are built from.  Each entry point
 * names the reference call site it replaces.
 *
 * Conventions
 *  - all arrays are float64, row-major; pointers named *_dev are device (HBM) addresses, e.g.
 *    torch.Tensor.data_ptr(); the library borrows them and never frees them;
 *  - theta is a HOST array in natural (untransformed) scale:
 *        [ ls(nkern*d) | kv(nkern) | alpha(nkern, RatQuad only) | gv | jitter ]
 *    host Python applies priors, log/interval transforms and their Jacobians (gpmcmc.py:193-208);
 *  - every function returns int: 0 ok; >0 LAPACK-style info = 1-based index of the first
 *    non-positive pivot (the LML is then -inf, as PyMC's "posdef" check gives);
 *    <0 bad argument (-1) or HIP/RCCL failure (-2); text via mi_gp_last_error().  Never aborts.
 *  - a handle is bound to one device and one HIP stream and is NOT thread-safe; calls return after
 *    the stream has been synchronised (scalar outputs are valid on return).
 */
#ifndef MI_GP_H
#define MI_GP_H
#ifdef __cplusplus
extern "C" {
#endif

enum { MI_GP_RBF = 0, MI_GP_MATERN52 = 1, MI_GP_MATERN32 = 2, MI_GP_EXPONENTIAL = 3, MI_GP_RATQUAD = 4 };
enum { MI_GP_OP_ADD = 0, MI_GP_OP_MUL = 1 };
#define MI_GP_MAX_KERN 8

/* libmi_gp.so is built with -fvisibility=hidden: these entry points are the only symbols it exports */
#define MI_GP_API __attribute__((visibility("default")))

typedef struct mi_gp_handle mi_gp_handle;

/* kernel string of GPMCMC.change_model (gpmcmc.py:497-515) already split into ids and ops */
typedef struct mi_gp_config {
  int n;                          /* training points */
  int d;                          /* input dimensions (nx) */
  int nkern;                      /* kernel components, <= MI_GP_MAX_KERN */
  int kernel_ids[MI_GP_MAX_KERN]; /* MI_GP_RBF ... */
  int ops[MI_GP_MAX_KERN];        /* ops[i] joins component i and i+1, applied left to right */
  int device;                     /* HIP device ordinal */
  int panel_tiles;                /* Cholesky super-panel width in 128-column tiles; 0 = default */
} mi_gp_config;

/* device buffers, allocated by the caller (PyTorch tensors in the Python host) */
typedef struct mi_gp_buffers {
  const double* X_dev; /* n x d   converted inputs  (xin of gpmcmc.py:235-237) */
  const double* y_dev; /* n       converted outputs (yin of gpmcmc.py:279)     */
  double* K_dev;       /* (np+128) x lda, np = mi_gp_padded_n(): covariance, overwritten by its
                          lower Cholesky factor; the extra 128 rows carry y^T -> beta^T = (L^-1 y)^T */
  long lda;            /* leading dimension of K/Z/W in elements: even, >= np */
  double* Z_dev;       /* np x lda  U = L^-T, upper triangular (mi_gp_lml_grad / mi_gp_predict_grad only; else may be NULL).
                          Rows and columns >= n hold the identity, and U is zero below its diagonal inside the diagonal 128 x 128
                          tiles too (nothing but zeros is ever written to the tiles below them). */
  double* W_dev;       /* np x lda  K^-1 (lower triangle) and GEMM scratch (same entry points; else may be NULL).  Rows and
                          columns >= n of the lower triangle hold the identity; the strict upper triangle is scratch. */
} mi_gp_buffers;

MI_GP_API const char* mi_gp_last_global_error(void);
MI_GP_API const char* mi_gp_last_error(mi_gp_handle* h);

MI_GP_API int mi_gp_create(const mi_gp_config* cfg, mi_gp_handle** out);
MI_GP_API int mi_gp_destroy(mi_gp_handle* h);
MI_GP_API long mi_gp_padded_n(const mi_gp_handle* h);   /* n rounded up to a multiple of 128 */
MI_GP_API int mi_gp_num_theta(const mi_gp_handle* h);   /* nkern*d + 2*nkern + 2 */
MI_GP_API void* mi_gp_stream(const mi_gp_handle* h);    /* the handle's hipStream_t */
/* Binds the buffers.  Every call ends the handle's resident state -- the factor of mi_gp_factor, U = L^-T and the K^-1 of
 * mi_gp_lml_grad live in the buffers they were computed in -- whether or not the pointers changed: mi_gp_predict*, mi_gp_predict_cov
 * and mi_gp_append return -1 until the next mi_gp_factor, mi_gp_alpha and mi_gp_grad_x until the next mi_gp_lml_grad. */
MI_GP_API int mi_gp_set_data(mi_gp_handle* h, const mi_gp_buffers* buffers);

/* LML(theta) = -1/2 |L^-1 y|^2 - sum log L_ii - n/2 log 2pi with L = chol(K(theta) + gv I + jitter I).
 * Replaces the logp evaluation of gp.marginal_likelihood (gpmcmc.py:321-323; explicit form :311-318). */
/* mi_gp_lml, mi_gp_lml_grad and mi_gp_factor (the single evaluations) all factorise in K_dev: each of them, whether it succeeds,
 * returns info > 0 or is refused for its theta, ends what an earlier one left resident -- the factor of mi_gp_factor, U and K^-1.
 * Before the first mi_gp_set_data they return -1. */
MI_GP_API int mi_gp_lml(mi_gp_handle* h, const double* theta_host, double* lml_out);
/* sum log L_ii and |L^-1 y|^2 of the last single evaluation (mi_gp_lml / mi_gp_lml_grad: marginal form, mi_gp_factor: conditional
 * form), grown by every accepted mi_gp_append.  Host-side numbers: mi_gp_set_data, mi_gp_set_diag and the batch calls leave them.
 * Returns -1, and writes neither output, before the first single evaluation and while the last one returned info > 0 or -1. */
MI_GP_API int mi_gp_lml_parts(mi_gp_handle* h, double* logdet_out, double* quad_out);

/* LML and its gradient w.r.t. the natural parameters, grad_out[mi_gp_num_theta()] in theta order
 * (d/d jitter equals d/d gv):  dLML/dtheta_k = 1/2 tr((alpha alpha^T - K^-1) dK/dtheta_k), K^-1 = L^-T L^-1
 * formed on the fp64 MFMA GEMM.  Replaces the dlogp half of model.logp_dlogp_function that
 * pm.find_MAP (gpmcmc.py:332,345,357) and pm.sample / NUTS (gpmcmc.py:351) call per step. */
MI_GP_API int mi_gp_lml_grad(mi_gp_handle* h, const double* theta_host, double* lml_out, double* grad_out);

/* Batched evaluation: `count` covariances of the SAME inputs, one theta each, factorised in lockstep (every kernel launch
 * of the evaluation carries blockIdx.z = problem).  One evaluation below N ~ 10^4 is bound by its serial panel chain and
 * leaves most of the chip idle; the reference evaluates the same data at several theta at once in its MAP restarts
 * (gpmcmc.py:328-343) and in the chains of pm.sample (gpmcmc.py:351).  Buffers (PyTorch tensors, borrowed): problem p uses
 * K_dev + p * stride_k ((np + 128) x lda each, the lda of mi_gp_set_data) and, for the gradient, Z_dev / W_dev +
 * p * stride_zw (np x lda each); strides in elements, even.  Results are those of mi_gp_lml / mi_gp_lml_grad at the same
 * theta (same arithmetic per element).  info_out[p] (optional): 0, or the 1-based index of problem p's first non-positive
 * pivot (lml_out[p] = -inf, its gradient 0).  The handle's single-evaluation state (factor, K^-1) is invalidated. */
typedef struct mi_gp_batch_buffers {
  double* K_dev;
  double* Z_dev; /* may be NULL: mi_gp_lml_batch only */
  double* W_dev; /* may be NULL: mi_gp_lml_batch only */
  long stride_k;
  long stride_zw;
  int count;
} mi_gp_batch_buffers;
/* mi_gp_set_batch (after mi_gp_set_data: -1 before) binds the buffers and ends the batch's conditional factors; the single-evaluation
 * state stays.  A batch call that is refused (-1: no buffers bound, k > count, no Z_dev / W_dev for the gradient) changes nothing.
 * The single K_dev of mi_gp_set_data MAY overlap the batch's K_dev range (member 0 on the single buffer saves one matrix): a batch
 * call then overwrites the single factor -- which it ends anyway -- and every single evaluation (mi_gp_lml, mi_gp_lml_grad,
 * mi_gp_factor) overwrites a member's factor, so with overlapping buffers it also ends the batch's conditional factors
 * (mi_gp_predict_batch returns -1 until the next mi_gp_factor_batch).  Without overlap single evaluations leave them. */
MI_GP_API int mi_gp_set_batch(mi_gp_handle* h, const mi_gp_batch_buffers* buffers);
MI_GP_API int mi_gp_lml_batch(mi_gp_handle* h, int k, const double* thetas_host, double* lml_out, int* info_out);
MI_GP_API int mi_gp_lml_grad_batch(mi_gp_handle* h, int k, const double* thetas_host, double* lml_out, double* grads_out, int* info_out);

/* Data-side gradients at the theta of the last successful mi_gp_lml_grad (K^-1 and alpha still resident):
 *   mi_gp_alpha  : alpha = K^-1 y (n doubles to the host); dLML/dy = -alpha
 *   mi_gp_grad_x : dLML/dX (n x d row-major, device), dLML/dx_im = sum_j (alpha_i alpha_j - Kinv_ij) dK_ij/dx_im
 * They carry the chain rule through the output / input warps whose parameters the reference samples together
 * with the hyper-parameters (cwgp / iwgp, gpmcmc.py:211-279, Jacobian term :319) and through the free
 * observation rows of inverse_opt (gpmcmc.py:1096-1101,1156-1165); PyMC obtains both by autodiff.  Any d (beyond 128 input
 * dimensions mi_gp_grad_x runs one pass per window of 128 output dimensions). */
MI_GP_API int mi_gp_alpha(mi_gp_handle* h, double* alpha_host);
MI_GP_API int mi_gp_grad_x(mi_gp_handle* h, double* gx_dev);
/* Optional per-point diagonal (n doubles, device, borrowed; NULL removes it) added to K on top of theta's
 * (gv, jitter): the noise vector `ynoise` of inverse_opt (gpmcmc.py:1134-1158, K += diag(ynoise)).  Every call, a repeated pointer
 * included, ends the resident state like mi_gp_set_data: the factor, U, K^-1 and the batch's conditional factors were built with the
 * diagonal before it.  May be called before mi_gp_set_data. */
MI_GP_API int mi_gp_set_diag(mi_gp_handle* h, const double* diag_dev);

/* Factorise K(theta) + jitter I + gv I (the conditional's form, [3P] Marginal._build_conditional) and
 * keep L and beta = L^-1 y on the device for mi_gp_predict.  Replaces the first half of
 * gp.predict(x, point=hyps, diag=True, pred_noise=True) at gpmcmc.py:593-594. */
MI_GP_API int mi_gp_factor(mi_gp_handle* h, const double* theta_host);
/* Posterior mean and diagonal variance at m new points (Xnew_dev m x d, converted inputs):
 * A = L^-1 K(X, X*), mu = A^T beta, var = kdiag - colsum(A o A) (+ gv if pred_noise); the same algebra
 * is written out in-tree at gpmcmc.py:766-778.  work_dev is caller scratch of
 * ceil(m/128)*128 rows x ldw (ldw even, >= mi_gp_padded_n()); mean_dev / var_dev receive m doubles.
 * Xnew_dev, mean_dev and var_dev (and dmean_dev / dvar_dev below) may be any DEVICE-VISIBLE address: device memory, or pinned
 * host memory (hipHostMalloc) -- for a few points the Python host passes the latter and skips every copy around the call
 * (up to 256 points: 110 -> 48 us per call at N = 512); the call returns with the stream synchronised either way.
 * mi_gp_predict changes no handle state; mi_gp_predict_u and mi_gp_predict_grad leave U = L^-T (and alpha) resident beside the
 * factor and change nothing else.  The same query in the same resident state returns the same bits every time. */
MI_GP_API int mi_gp_predict(mi_gp_handle* h, const double* Xnew_dev, int m, double* work_dev, long ldw, double* mean_dev,
                  double* var_dev, int pred_noise);
/* The same conditional through U = L^-T (formed once per mi_gp_factor, N^3/3 flops): A = K(X*, X) U is one GEMM with
 * a triangular k-range instead of the blocked triangular solve -- the path for sweeps of many points at fixed
 * hyper-parameters (BO's 10 000-point proposals at gpmcmc.py:691-697).  Needs Z_dev / W_dev; work_dev must hold
 * 2 * ceil(m/128)*128 rows x ldw. */
MI_GP_API int mi_gp_predict_u(mi_gp_handle* h, const double* Xnew_dev, int m, double* work_dev, long ldw, double* mean_dev,
                    double* var_dev, int pred_noise);
/* The same plus d mu / d x* and d var / d x* (m x d each, device): d mu = sum_i alpha_i dk(x_i,x*)/dx*,
 * d var = -2 sum_i w_i dk(x_i,x*)/dx* with w = K^-1 k(X,x*).  Replaces the PyTensor graph of the single-point
 * predictive that BO's refinement differentiates (gpmcmc.py:766-801).  Needs Z_dev / W_dev; work_dev must hold
 * 2 * ceil(m/128)*128 rows x ldw (the upper half receives the w rows); (nkern + 1) * d doubles must fit 60 KB of LDS
 * (d <= 1536 with four components, 3840 with one). */
MI_GP_API int mi_gp_predict_grad(mi_gp_handle* h, const double* Xnew_dev, int m, double* work_dev, long ldw, double* mean_dev,
                       double* var_dev, int pred_noise, double* dmean_dev, double* dvar_dev);

/* Joint conditional and posterior function draws at m new points (PyMC's gp.predict(Xnew, point, diag=False, pred_noise=...),
 * [3P] Marginal._build_conditional; the reference passes diag=True at gpmcmc.py:593-594).
 *   mi_gp_predict_cov  after mi_gp_factor (or mi_gp_append): mean_dev (m doubles) = mi_gp_predict's mean bit for bit (same
 *                      cross-covariance, blocked solve and reduction; work_dev laid out as there: ceil(m/128)*128 rows x ldw,
 *                      ldw even and >= mi_gp_padded_n()).  cov_dev is mp x ldc row-major, mp = ceil(m/128)*128, ldc even and
 *                      >= mp; its lower triangle, diagonal included, receives
 *                          Sigma = K(X*, X*) - A^T A,  A = L^-1 K(X, X*),  + sqrt(gv)^2 I if pred_noise, else + jitter I,
 *                      with the full-matrix kernel form on the diagonal (k(sqrt(1e-12)) for Matern / Exponential, not the 1 of
 *                      diag=True).  Padding rows and columns hold the identity; the strict upper triangle is unspecified.
 *                      Built as the assembly of K(X*, X*) + the diagonal term and one lower-trapezoid GEMM C -= A A^T (k = np):
 *                      m^2 N + N^2 m flops.  The handle's state is not changed.
 *   mi_gp_sample_cov   s joint draws from N(mean, Sigma) for any symmetric positive-definite Sigma in the lower triangle of
 *                      cov_dev (mp x ldc as above; the padding need not be set):  cov_dev's lower triangle is overwritten by
 *                      L_Sigma = chol(Sigma + extra_jitter I) (zeros above the diagonal inside the diagonal 128 x 128 tiles,
 *                      identity in the padding) and
 *                          draws_dev[r * ldd + i] = mean_i + (L_Sigma z_r)_i,   r < s, i < m (ldd >= m),
 *                      z the normals j = r m + i of a counter-based stream: normal j comes from Philox block b = offset + j/4,
 *                      Philox4x64-10 of the 256-bit counter b + 1 under the key (seed, 0) -- the four words
 *                      numpy.random.Philox(key=seed, counter=b).random_raw(4) returns; words (w0, w1) give normals 4b, 4b+1 and
 *                      (w2, w3) give 4b+2, 4b+3 by Box-Muller: u = ((w >> 11) + 0.5) 2^-53, rho = sqrt(-2 log u0), normals
 *                      rho cos(2 pi u1), rho sin(2 pi u1).  A call uses ceil(s m / 4) blocks: consecutive calls with
 *                      offset += ceil(s m / 4) never reuse a number; the same (seed, offset) gives the same bits.  work_dev:
 *                      mi_gp_sample_cov_work(m, s) doubles (-1 for m or s < 1), work_len its length.  m^3/3 + m^2 s flops.
 *                      Returns info > 0 (1-based pivot) if Sigma + extra_jitter I is not positive definite: draws_dev is then
 *                      not written and cov_dev holds a partial factor (rebuild it before another attempt).  Runs on the handle's
 *                      stream and changes NO handle state: the resident factor, U, K^-1, the batch state and the append capacity
 *                      stay valid.
 * Both return -1 on bad arguments, checked before any HIP call (text in mi_gp_last_error(h), and in mi_gp_last_global_error()
 * for a null handle), -2 on a HIP failure. */
MI_GP_API int mi_gp_predict_cov(mi_gp_handle* h, const double* Xnew_dev, int m, double* work_dev, long ldw, double* mean_dev,
                                double* cov_dev, long ldc, int pred_noise);
MI_GP_API long mi_gp_sample_cov_work(int m, int s);
MI_GP_API int mi_gp_sample_cov(mi_gp_handle* h, double* cov_dev, long ldc, int m, const double* mean_dev, double extra_jitter, int s,
                               unsigned long long seed, unsigned long long offset, double* draws_dev, long ldd, double* work_dev,
                               long work_len);

/* Posterior predictive over k hyper-parameter draws (the MCMC draws of GPMCMC.fit(method='mcmc_*'); PyMC's gp.conditional +
 * sample_posterior_predictive), on the buffers of mi_gp_set_batch (k <= count):
 *   mi_gp_factor_batch   factorises k covariances in the conditional form, one theta each (what mi_gp_factor does, k problems in
 *                        lockstep) and keeps every problem's L_p, beta_p = L_p^-1 y and leaf inverses in the batch buffers.
 *                        info_out[p] (optional): 0, or the 1-based index of problem p's first non-positive pivot.  Like the other
 *                        batch calls it invalidates the handle's single-evaluation state.
 *   mi_gp_predict_batch  per problem p: A_p = L_p^-1 K_p(X, X*), mean_dev[p*m + i] = A_p,i . beta_p, var_dev[p*m + i] =
 *                        kdiag_p - |A_p,i|^2 (+ gv_p if pred_noise) -- bit for bit what mi_gp_factor(theta_p) + mi_gp_predict
 *                        return.  Rows of a problem whose info was non-zero are NaN.  mix_mean_dev / mix_var_dev (optional, both
 *                        or neither; m doubles each): the equal-weight mixture over the K' problems with info 0,
 *                        mix_mean = sum mean_p / K', mix_var = sum var_p / K' + sum (mean_p - mix_mean)^2 / K' (two passes,
 *                        problems in index order, sums relative to the first member's moments: K' equal draws return that
 *                        draw's moments exactly; NaN if K' = 0).  work_dev holds k blocks of ceil(m/128)*128 rows x ldw,
 *                        stride_work elements apart (even, >= ceil(m/128)*128 * ldw).  Returns -1 unless mi_gp_factor_batch with
 *                        the same k was the last batch call (mi_gp_set_batch, mi_gp_set_data and mi_gp_set_diag also end it).
 * Xnew_dev, mean_dev, var_dev and the mixture outputs are device-visible addresses as for mi_gp_predict. */
MI_GP_API int mi_gp_factor_batch(mi_gp_handle* h, int k, const double* thetas_host, int* info_out);
MI_GP_API int mi_gp_predict_batch(mi_gp_handle* h, int k, const double* Xnew_dev, int m, double* work_dev, long ldw, long stride_work,
                                  double* mean_dev, double* var_dev, int pred_noise, double* mix_mean_dev, double* mix_var_dev);

/* Appending observations at fixed hyper-parameters (BO / sequential designs that keep theta for several iterations; the
 * reference refits after every evaluated point, gpmcmc.py:883-888 -- SURVEY 8 f-4's "update the Cholesky factor when data are
 * appended").  Costs O(n^2 k) against the O(n^3) of a refactorisation.
 *   mi_gp_reserve  the handle may grow to `capacity` points: every handle-owned scratch that depends on n is sized for it
 *                  (resident contents kept).  The caller promises that the buffers of mi_gp_set_data hold that many points:
 *                  X_dev / y_dev (and the diagonal of mi_gp_set_diag) capacity rows, K_dev padded(capacity) + 128 rows, Z_dev /
 *                  W_dev padded(capacity) rows, lda >= padded(capacity) (checked when data are bound).  Without it a handle
 *                  cannot grow (mi_gp_append returns -1) and behaves as before.  -1 if capacity < n.
 *   mi_gp_append   extends the conditional-form factorisation of the last successful mi_gp_factor by k points (1 <= k <= 128,
 *                  Xnew_dev k x d, ynew_dev k, diag_new_dev k entries of the per-point diagonal -- required exactly when one is
 *                  set) at the same theta: L21 = K21 L11^-T, L22 = chol(K22 + noise - L21 L21^T), beta2 = L22^-1 (y2 - L21 beta1).
 *                  The points are copied into rows n .. n + k - 1 of X_dev / y_dev (/ the diagonal); n grows by k and the padded
 *                  size by a tile when a 128-row boundary is crossed (the beta row moves along).  The first n rows of the
 *                  factor are not touched.  With U = L^-T resident (mi_gp_predict_u / mi_gp_predict_grad) it is extended in
 *                  place and alpha recomputed; mi_gp_predict, _predict_u and _predict_grad continue without a refactorisation,
 *                  mi_gp_lml_parts returns the grown logdet and quad.  K^-1 is invalidated (mi_gp_alpha / mi_gp_grad_x need a
 *                  new mi_gp_lml_grad), and so is the batch state: every batch call returns -1 until mi_gp_set_batch is
 *                  called again (buffers sized for the new n).  work_dev: 4 * 128 * ldw + 65600 doubles, ldw even and
 *                  >= padded(n + k).  Returns -1 without a prior mi_gp_factor, for n + k > capacity, k out of range, a
 *                  diagonal mismatch or ldw too small; info > 0 (1-based global index of the bad pivot) if the appended block
 *                  is not positive definite -- the handle is then exactly as it was. */
MI_GP_API int mi_gp_reserve(mi_gp_handle* h, int capacity);
MI_GP_API int mi_gp_append(mi_gp_handle* h, const double* Xnew_dev, const double* ynew_dev, const double* diag_new_dev, int k,
                           double* work_dev, long ldw);

/* Joint log predictive density of k trial points given the resident factorisation, and its gradients w.r.t. the trial inputs
 * and outputs: the differentiable companion of mi_gp_predict_cov, and mi_gp_append's conditional without the commit.  It is the
 * held-out log predictive density of a fit, and the one term of inverse_opt's potential (gpmcmc.py:1156-1165: the LML of the
 * training set extended by the observation rows) that moves with the trial x:
 *     log p(y2 | y1, X1, X2, theta) = LML(n + k) - LML(n).
 *   mi_gp_logpdf  after a successful mi_gp_factor (or mi_gp_append), 1 <= k <= 128, Xnew_dev k x d, ynew_dev k, diag_new_dev the
 *                 k entries of the per-point diagonal -- required exactly when one is set, as for mi_gp_append; K22 gets
 *                 jitter + gv + diag_new.  L21 = K21 L11^-T, S = K22 - L21 L21^T = L22 L22^T, beta2 = L22^-1 (y2 - L21 beta1),
 *                     *logp_out (host) = -1/2 |beta2|^2 - sum log L22_ii - k/2 log 2 pi.
 *                 Gradients are computed when dx_dev (k x d) or dy_dev (k) is given (device-visible, either may be NULL); they
 *                 need Z_dev / W_dev and make U = L^-T resident exactly as mi_gp_predict_grad does, and (nkern + 1) * d doubles
 *                 must fit 60 KB of LDS as there.  With gamma = L22^-T beta2, P = L21 U11^T, Q = S^-1 P:
 *                     dy = -gamma,
 *                     dx[i][m] = sum_{j<n} C[i][j] dk(x*_i, x_j)/dx*_im + sum_{j<k} D[i][j] dk(x*_i, x*_j)/dx*_im,
 *                     C[i][j] = gamma_i (alpha1[j] - sum_l gamma_l P[l][j]) + Q[i][j],   D[i][j] = gamma_i gamma_j - S^-1[i][j]
 *                 (the trial rows of alpha_J alpha_J^T - K_J^-1 of the joint system); coincident points (r2 = 0) contribute 0.
 *                 NO handle state changes, apart from U / alpha becoming resident on a gradient call: the factor, the beta
 *                 row, the leaf inverses, mi_gp_lml_parts, K^-1's validity, the batch state, n and the capacity all stay (the
 *                 handle's bad-pivot word and mi_gp_append's scalar scratch are used as scratch).  If S is not positive
 *                 definite the call returns info > 0 (1-based global index n + pivot), *logp_out = -inf, and dx_dev / dy_dev
 *                 are not written.  Bad arguments (no factorisation, k out of range, a diagonal mismatch, ldw odd or
 *                 < mi_gp_padded_n(), gradients without Z_dev / W_dev or beyond the LDS rule, a null buffer) return -1 before
 *                 any HIP call, with text in mi_gp_last_error(h) (mi_gp_last_global_error() for a null handle); -2 on a HIP
 *                 failure.  work_dev holds mi_gp_logpdf_work(ldw) doubles; every element a launch reads is written earlier in
 *                 the same call (a work block full of NaN gives the bits of a zeroed one).  The same query in the same resident
 *                 state returns the same bits; with and without U resident the value agrees to rounding (the blocked solve
 *                 against one GEMM with U, as for mi_gp_append).  With profiling level >= 1, mi_gp_timers' out[14..16] receive
 *                 the call's conditional-block, weights (L22^-1, S^-1, P, Q, C) and gradient-kernel times.
 *   mi_gp_logpdf_work  doubles of work_dev for a leading dimension ldw: mi_gp_append's 4 * 128 * ldw + 65600, plus S^-1 (16384)
 *                 and gamma (128); -1 for ldw odd or < 128.  No capacity is needed: nothing grows. */
MI_GP_API long mi_gp_logpdf_work(long ldw);
MI_GP_API int mi_gp_logpdf(mi_gp_handle* h, const double* Xnew_dev, const double* ynew_dev, const double* diag_new_dev, int k,
                           double* work_dev, long ldw, double* logp_out, double* dx_dev, double* dy_dev);

/* Exact k-fold cross-validation at fixed hyper-parameters, from the K^-1 and alpha = K^-1 y that the last successful mi_gp_lml_grad
 * left resident: "how well does the model predict points it has not seen", the question GPMCMC.test_stats answers with one random
 * split and a refit (the numeric half of test_plots, gpmcmc.py:933-976), for every fold of a partition at the cost of one
 * gradient evaluation plus one 128 x 128 factorisation per fold.  For an index set I the hold-out predictive of the noisy
 * observations y_I given all other points is exact in the blocks of K^-1 (marginal form, a per-point diagonal of mi_gp_set_diag
 * included -- the density mi_gp_logpdf defines for its trial block):
 *     Sigma_I = (K^-1_II)^-1,   y_I - mu_I = Sigma_I alpha_I,
 *     log p(y_I | y_-I) = -1/2 alpha_I^T Sigma_I alpha_I + 1/2 log det K^-1_II - |I|/2 log 2 pi.
 *   mi_gp_kfold  nfolds >= 1 folds in CSR form on the HOST: fold f is the points fold_idx_host[fold_ptr_host[f] ..
 *                fold_ptr_host[f + 1]), fold_ptr_host[0] = 0; 1 to 128 points per fold, indices in [0, n), distinct inside a
 *                fold, in any order; folds may overlap one another and need not cover the data.  Outputs (device-visible
 *                addresses as for mi_gp_predict): logp_dev[nfolds]; mean_dev[t] = mu and var_dev[t] = diag Sigma_I for position
 *                t of fold_idx_host (both or neither).  info_out[nfolds] (host, optional): 0, or the 1-based position inside
 *                the fold of the first non-positive pivot of K^-1_II -- that fold's logp is -inf and its moments NaN, the other
 *                folds are not affected, and the call still returns 0.
 *                Per pass of up to P folds: a gather of K^-1_II into a 128 x 128 block per fold (element (a, b) from
 *                W[max(i_a, i_b)][min(i_a, i_b)]: the strict upper triangle of W_dev, scratch, is never read; identity in the
 *                padding) with alpha_I and y_I; the factorisation's leaf kernel, one workgroup per fold, for C = chol(K^-1_II)
 *                and M = C^-1; and one workgroup per fold for t = M alpha_I, mean = y_I - M^T t, var_j = sum_r M[r][j]^2,
 *                logp = -1/2 |t|^2 + sum log C_ii - |I|/2 log 2 pi, every sum in a fixed order.  P = the folds work_dev holds
 *                (work_len doubles, 16-byte aligned): a fold's result does not depend on P, the same query in the same state
 *                returns the same bits, and every element a launch reads is written earlier in the same call (a work block
 *                full of NaN changes nothing).  The library stages the index lists into the work block itself.
 *                A call in which every fold has ONE point (leave-one-out) runs the closed form in one launch and needs no work
 *                block (work_dev may be NULL): var = 1 / Kinv_ii, mean = y_i - alpha_i / Kinv_ii,
 *                logp = 1/2 log Kinv_ii - 1/2 alpha_i^2 / Kinv_ii - 1/2 log 2 pi; Kinv_ii <= 0 gives info 1.
 *                NO handle state changes: nothing is written to K_dev, Z_dev or W_dev, and the handle's bad-pivot word and
 *                mi_gp_append's scalar scratch are not used.  Returns 0; -1 for bad arguments -- K^-1 not resident (before
 *                mi_gp_lml_grad; after mi_gp_set_data, mi_gp_set_diag, mi_gp_lml, mi_gp_factor, mi_gp_append or a batch call),
 *                nfolds < 1, a fold outside 1..128 points, an index outside [0, n) or repeated inside a fold, a null buffer,
 *                one of mean_dev / var_dev alone, a work block too small for one fold -- checked on the host before any HIP
 *                call, with text in mi_gp_last_error(h) (mi_gp_last_global_error() for a null handle); -2 on a HIP failure.
 *                Returns with the stream synchronised.
 *   mi_gp_kfold_work  doubles of work_dev for P = folds_per_pass and total_idx = fold_ptr_host[nfolds]: per fold two 128 x 128
 *                blocks and the gathered alpha_I / y_I (2 * 16384 + 256), plus 2 * total_idx + 2 for the staged index lists
 *                and the folds' bad-pivot words; -1 for folds_per_pass < 1 or total_idx < 1.
 * Out of scope: gradients w.r.t. theta (the sum over leave-one-out or contiguous folds has one: options 48 and 49 of mi_gp_set_option); folds of more than 128 points (they need a blocked factorisation of K^-1_II); the full
 * Sigma_I; a batched (one theta per member) form; phase timers. */
MI_GP_API long mi_gp_kfold_work(int folds_per_pass, long total_idx);
MI_GP_API int mi_gp_kfold(mi_gp_handle* h, int nfolds, const int* fold_ptr_host, const int* fold_idx_host, double* work_dev,
                          long work_len, double* logp_dev, double* mean_dev, double* var_dev, int* info_out);

/* tuning knobs (benchmarks / A-B tests), ALL per handle -- nothing here is process-wide:
 *   0  look-ahead: factor the next super-panel on a second stream while the trailing update runs; 0 never, 1 by size
 *      (default: from 20 tile columns = N > 2432 on, where the overlap beats the cross-stream hand-offs -- and from 4 tile
 *      columns = N > 384 on for problems that run in column mode from the start, options 37 and 45), 2 always
 *   2  super-panel width in 128-column tiles (default 0 = by trailing size, options 4-6)
 *   4-6  trailing sizes (tile columns) above which the super-panel is 16 / 8 / 4 tiles wide (below the last: 2);
 *        defaults: never 16, else 8; with look-ahead active, problems of up to 60 tile columns use at most 4
 *   7  GEMM launches with fewer 128x128 tiles than this run on 64x64 tiles (default 1024)
 *   8  trailing size at or below which look-ahead bulk updates run one workgroup per CU (default: always)
 *   9  128x128-tile GEMM launches with uniform k hand the tiles beyond their last full round of 512 to the 64x64-tile
 *      kernel (default 1: a last round with few tiles costs a whole round; sharded N=65536 on one rank 1.52 -> 1.47 s)
 *   14 band height (tile rows) of the band-column-major tile order of uniform-k trapezoid launches (default 8, 0 = row-major)
 *   16 panel-stream GEMM launches raise their waves' issue priority (s_setprio 3) against the bulk update's (default 1)
 *   18 tiles of a bulk update that run one workgroup per CU beside the panel chain, the rest two per CU (default 1536, 0: no split)
 *   19 ... only when at least this many tiles remain for the second part (default 1024)
 *   20 trailing tile columns from which the next super-panel's update rides at the head of the trailing update's tile
 *      enumeration instead of in launches of its own (default 72, 0: never)
 *   21 trailing tile columns at or below which a two-stream factorisation continues on the main stream alone (default 8)
 *   26 cross-stream edges of the factorisation: 0 hipEventRecord + hipStreamWaitEvent; 1 stream memory operations --
 *      hipStreamWriteValue32 behind the producer's work, hipStreamWaitValue32 in front of the consumer's (4-5 us per edge
 *      instead of 11-12 on MI355X; N = 6144 3.40 -> 3.26 ms); 2 (default) the same protocol with the PANEL stream's halves
 *      folded into launches of the library: its write + wait at a super-panel boundary is one one-lane launch, its wait
 *      for the next-panel update is a poll at the end of the leaf in front of the first reader (N = 4096 1.995 -> 1.965 ms).
 *      Modes 1 and 2 need hipDeviceAttributeCanUseStreamWaitValue: mi_gp_create queries it and falls back to 0 (the
 *      option then stays 0 whatever is set).  The panel stream's polls are enqueued AHEAD of the main-stream writes they
 *      wait for, which needs the two streams' kernels to be dispatched concurrently.  Where they are not -- rocprofv3
 *      --pmc, AMD_SERIALIZE_KERNEL / HIP_LAUNCH_BLOCKING, more handles evaluating at once than the device has hardware
 *      queues for (six per device are tested) -- such a poll ends only through its limit.  The library deals with that
 *      itself (the reference's evaluations never fail for reasons of scheduling, gpmcmc.py:331-339): mi_gp_create probes
 *      the dispatch once (a one-lane poll with a limit of a few ms) and starts with mode 0 where it is serialised; and an
 *      evaluation whose poll gives up (every later poll of it then returns at once) makes the handle switch to mode 0 for
 *      good and is evaluated AGAIN before the call returns -- the caller sees the result, mi_gp_last_error names the
 *      demotion once, mi_gp_get_option(40) reads 1.  Setting option 26 to 1 or 2 again re-arms the polls.  Only a second
 *      time-out in the same call returns -2 ("a cross-stream signal ... was not seen within its poll limit"); the handle
 *      stays usable.  Same bits in every mode.
 *   27 log2 of the number of sleeps after which such a poll gives up (default 22 = seconds; 4 .. 30)
 *   28 test hook: the next two-stream evaluation leaves one main-stream signal unwritten (its poll must give up); needs
 *      option 26 = 2 (refused otherwise: a runtime wait has no limit) and is cleared by the next evaluation whatever its schedule
 *   30 gradient evaluations of 64 tile columns and more: the leaf blocks and the block-doubling levels of U = L^-T with nodes of
 *      up to this many tiles start on the main stream inside the factorisation's chain-bound last steps instead of behind it
 *      (default 16, 0: never; same launches per tile, bit-identical gradients; N = 16384 LML + gradient 69.8 -> 69.4 ms)
 *   31 ... in the steps with at most this many trailing tile columns, half as many new columns per step (default 48)
 *   32 in-panel updates (between two leaves of a super-panel) with k = 128 over at most two tile columns and at most this many
 *      16-row x 128-column slices run on the thin kernel (default 2048; 0: never).  Regroups sums (agreement to rounding); the
 *      choice depends on the update's shape alone, so every schedule and a batch return the same bits.
 *   35 extended super-panels: a super-panel with at most this many tile rows below it (default 32; 0: never) also applies its
 *      in-panel updates to the NEXT super-panel's first tile column, level by level, instead of one update of that column
 *      behind the panel (problems of 20 tile columns or more, not the last 8 columns).  Regroups that column's sums; a rule of
 *      the shape alone as well.
 *   37 column mode: the last this-many tile columns (default 24; 0: never) are factored column by column -- leaf, strip and one
 *      k = 256 thin update of the next column on the panel stream; older columns reach a column through k = 128 updates on the
 *      main stream, a column behind the chain.  Problems of up to that many tile columns run in it from the start, on two
 *      streams from 4 tile columns on (round 6; it was 8 before option 45).  Regroups sums (agreement to rounding); a rule of the shape alone: one stream, two
 *      streams and a batch return the same bits.  N = 2048 0.665 -> 0.619 ms, 3072 0.981 -> 0.920, 4096 1.471 -> 1.443.
 *   46 problems of up to this many tile columns run in column mode from the START even where option 37 would put panels in
 *      front of it (default 31 = N <= 3968; ignored when 37 is 0).  Regroups sums like 37, a rule of the shape alone.
 *      N = 3200 0.994 -> 0.946 ms, 3968 1.292 -> 1.267; at 32 tile columns it turns (N = 4096 1.416 -> 1.454).
 *   38 column mode of a BATCH: the main stream applies its k = 128 updates to the columns behind the chain's next one in
 *      k-segmented launches of this many columns (default 8; 1: one launch per column as for a single evaluation).  The tile
 *      takes every 128-column partial sum as a launch of its own would round it: same bits, scheduling only.
 *   45 two-stream evaluations queue their first two kernels (theta / y rows, assembly) on the PANEL stream, so that the first
 *      leaf follows them in stream order instead of behind a cross-stream edge (default 1; N = 1024 -7 %, 2048 -4 %, from 32 tile
 *      columns on 0.1-0.4 %); scheduling only
 *   47 the HOST's wait at the end of an evaluation: its last kernel publishes the evaluation's sequence number in the pinned result
 *      buffer, behind the values it stands for, and the call spins on that word for up to this many microseconds (default 2000;
 *      0: never) before it falls back to hipStreamSynchronize -- a stream synchronisation costs 6-8 us behind the kernel's end
 *      (N = 128 LML + gradient 0.101 -> 0.090 ms, 1024 0.310 -> 0.291, 4096 1.424 -> 1.387).  An evaluation that outlasts the budget
 *      makes the handle's next 15 calls skip the spin (a long evaluation costs a core 2 ms in 16 calls); every 256th call
 *      synchronises the stream all the same.  The word is the LAST thing the evaluation's last kernel does: when a call returns
 *      through the spin every device-side read and write of the evaluation is complete (that kernel writes nothing but the
 *      pinned result buffer) and only its retirement may be outstanding -- the handle's buffers may be read or overwritten
 *      from any stream, as after a synchronisation.  Same bits.
 *   48 (not a tuning knob) the OBJECTIVE of mi_gp_lml_grad: 0 (default) the log marginal likelihood, 1 the leave-one-out log
 *      predictive density of Rasmussen & Williams section 5.4.2, the criterion to fit hyper-parameters to when the kernel family is
 *      misspecified.  With P = K^-1, p_i = P_ii and alpha = P y (marginal form, a per-point diagonal of mi_gp_set_diag included)
 *          L_LOO = sum_i [ 1/2 log p_i - 1/2 alpha_i^2 / p_i - 1/2 log 2 pi ]     (the sum of mi_gp_kfold's singleton logp)
 *          e_i = alpha_i / p_i,  s_i = sqrt((1 + alpha_i^2 / p_i) / p_i),  w = P e,  M = (P diag s)(P diag s)^T
 *          dL_LOO/dtheta_k = 1/2 sum_ij [ (alpha_i w_j + w_i alpha_j) - M_ij ] dK_ij/dtheta_k.
 *      Under 1, mi_gp_lml_grad runs the ordinary evaluation first (same launches, same schedule: K^-1 and alpha become resident
 *      as always) and then, on the handle's stream, a tail of one lower-trapezoid GEMM with k = padded n (M, about the flops of
 *      the evaluation in front of it, whatever ntheta is -- the forward form, R & W eq. 5.13, costs one N^3 product per
 *      hyper-parameter) between four memory-bound kernels and the LML gradient's contraction kernel, which takes
 *      M - (alpha w^T + w alpha^T) in the place of K^-1 and a zero vector in the place of alpha.  *lml_out = L_LOO, grad_out its
 *      gradient in theta order (d/d jitter = d/d gv); the call returns with the stream synchronised; the same call in the same
 *      state returns the same bits, and every element a launch of the tail reads is written earlier in the same call.  A bad
 *      pivot of the factorisation is reported as under 0 (info > 0, -inf, zero gradient; no tail); a K^-1_ii that is not a
 *      positive finite number -- rounding alone can produce one behind a successful factorisation -- returns i + 1, -inf and
 *      a zero gradient.  K^-1 and alpha stay resident with their meaning: mi_gp_alpha, mi_gp_grad_x (the LML's data-side
 *      gradients) and mi_gp_kfold work behind the call, mi_gp_lml_parts keeps the factorisation's logdet and quad.  K_dev and
 *      Z_dev are the tail's scratch: their contents are unspecified afterwards, except that Z_dev holds zeros wherever the next
 *      evaluation expects them (all of it is cleared).  No buffer is asked of the caller; the handle owns six vectors of padded
 *      capacity (allocated by the first such call, re-sized by mi_gp_reserve).  mi_gp_lml_grad_batch returns -1 under 1 (no
 *      batched form); mi_gp_lml, mi_gp_lml_batch, mi_gp_factor* and every other entry are not affected.  Setting the option
 *      changes no resident state; values other than 0 / 1 return -1, and so does 1 in a build without the tail (the host-only
 *      schedule-trace program).  Out of scope: data-side gradients of L_LOO, a batched or sharded form (k-fold gradients: option 49).
 *   49 (not a tuning knob) the FOLD SIZE b of the cross-validation objective that mi_gp_lml_grad returns under option 48 = 1:
 *      1 (default) is leave-one-out as described there, with the bits it has without this option; 2..128 give the
 *      leave-block-out log predictive density over the contiguous folds I_f = [f b, min((f + 1) b, n)) -- the last fold may be
 *      smaller, down to one point; b >= n is one fold, and L_CV the log marginal likelihood.  With P = K^-1 and alpha = P y as
 *      under option 48, and per fold C = chol(P_II), M = C^-1, t = M alpha_I, tau = |t|^2 (mi_gp_kfold's quantities)
 *          L_CV = sum_f [ -1/2 tau_f + sum_i log C_ii - |I_f|/2 log 2 pi ]        (the sum of mi_gp_kfold's logp over these folds:
 *                                                                                  a fold's logp has mi_gp_kfold's bits)
 *          e_I = M^T t  (= Sigma_I alpha_I, Sigma_I = P_II^-1 = M^T M),   dL_CV/dP_II = 1/2 (e e^T + Sigma_I) = 1/2 R R^T,
 *          R = M^T + c e t^T,  c = 1 / (1 + sqrt(1 + tau)),   q_I = t / sqrt(1 + tau)  (R q = e)
 *          B[:, I_f] = P[:, I_f] R_f,  w = B q = P e,   dL_CV/dtheta_k = -1/2 sum_ij G'_ij dK_ij/dtheta_k,
 *          G' = B B^T - (alpha w^T + w alpha^T):
 *      option 48's tail with diag(s) replaced by the block-diagonal matrix of the folds' R_f.  In front of the tail's GEMM run,
 *      per pass of up to 128 folds, mi_gp_kfold's gather and batched 128 x 128 leaf and one kernel that forms t, e, q, R and the
 *      fold's logp, then a fixed-order reduction over the folds and one multiply B = P blockdiag(R_f) on the fp64 matrix cores
 *      (2 * 128 * padded n * n flops, from the lower triangle of W_dev alone) in the place of the scaling by s; the number of
 *      folds per pass changes no result.  *lml_out = L_CV, grad_out its gradient in theta order (d/d jitter = d/d gv).
 *      Every contract of option 48 carries over: the ordinary evaluation runs first with the same launches; K^-1 and alpha stay
 *      resident with their meaning (mi_gp_alpha, mi_gp_grad_x, mi_gp_kfold, mi_gp_lml_parts); K_dev and Z_dev are scratch and
 *      Z_dev is all zeros afterwards; the call returns with the stream synchronised; the same call in the same state returns the
 *      same bits; every element a launch reads is written earlier in the same call; mi_gp_lml_grad_batch stays refused under
 *      48 = 1.  A bad pivot of the factorisation is reported as under 48 = 0; a fold whose P_II is not positive definite returns
 *      -inf, a zero gradient and the 1-based index of the point at the bad pivot (the smallest over the folds).  The handle owns
 *      the scratch of a pass (allocated by the first such call, re-sized by mi_gp_reserve, freed by mi_gp_destroy).  Setting the
 *      option changes no resident state and has no effect at all under 48 = 0; values outside 1..128 return -1, and so does a
 *      value other than 1 in a build without the tail.  Out of scope: arbitrary index sets (permute the data: the contiguous
 *      folds of a random permutation are random folds), folds of more than 128 points, a batched or sharded form.
 *   50 (not a tuning knob) the TREND: a prior mean h(x)^T beta whose coefficients carry a vague prior and are integrated out in
 *      closed form (universal kriging; Rasmussen & Williams section 2.7, eqs. 2.41-2.45), so theta and mi_gp_num_theta() stay as
 *      they are.  0 (default) no trend; 1 constant, h = [1], p = 1; 2 linear, h = [1, x_1 .. x_d], p = 1 + d (needs d <= 127).
 *      H is n x p with rows h(x_i)^T from the bound X_dev (converted inputs); K_y is the noisy covariance of the entry point's own
 *      form (marginal in mi_gp_lml_grad, conditional in mi_gp_factor; the diagonal of mi_gp_set_diag included), alpha = K_y^-1 y.
 *      mi_gp_lml_grad (option 48 = 0) runs the ordinary evaluation first (same launches, same schedule), then a tail on the
 *      handle's stream:
 *          V = K_y^-1 H,  A = H^T V,  C_A = chol(A),  Q = V C_A^-T,  c = Q^T y
 *          L_T = LML + 1/2 |c|^2 - sum_j log (C_A)_jj + p/2 log 2 pi                                      (R & W eq. 2.45)
 *          P~ = K_y^-1 - Q Q^T,   alpha~ = alpha - Q c  (= P~ y)
 *          dL_T/dtheta_k = 1/2 sum_ij (alpha~_i alpha~_j - P~_ij) dK_ij/dtheta_k              (d/d jitter = d/d gv)
 *      -- V by a symmetric thin multiply on the fp64 matrix cores that reads the lower triangle of W_dev alone (it streams the
 *      matrix once, about 8 N^2 bytes, in slices of k whose partial products are added in index order; measured at about a
 *      quarter of the HBM peak: bound by the latency of its loads, not yet by the bandwidth), A in k segments that are added in index order, the rank-128 update
 *      W -= Q Q^T over the lower trapezoid on the GEMM, and the LML gradient's contraction kernel with P~ and alpha~.
 *      *lml_out = L_T, grad_out its gradient in theta order; the call returns with the stream synchronised.  Afterwards the lower
 *      triangle of W_dev holds P~, not K^-1: the handle marks K^-1 not resident, as after mi_gp_lml (mi_gp_kfold and the data-side
 *      gradients need option 50 = 0 and a new mi_gp_lml_grad); mi_gp_lml_parts keeps the factorisation's logdet and quad.
 *      With option 48 = 1 the call returns -1 (no cross-validation objective under a trend).
 *      mi_gp_factor additionally forms G^T = (L^-1 H)^T (the blocked solve of mi_gp_predict on 128 rows), A = G^T G = C_A C_A^T,
 *      its inverse, beta^ = A^-1 G^T b and b~ = b - G beta^ (b = L^-1 y, the beta row) in scratch the handle owns, and
 *      mi_gp_predict returns the trend's conditional: per point, with a* = L^-1 k(X, x*) (the row the call forms in work_dev)
 *          r = h(x*) - G^T a*,   mean = a* . b~ + h(x*)^T beta^,   var = kdiag - |a*|^2 + |C_A^-1 r|^2 (+ gv if pred_noise)
 *                                                                                                       (R & W eqs. 2.41-2.42)
 *      in one reduction over the rows of work_dev, whose contract (size, layout) does not change; mean_dev / var_dev are written
 *      once and may be pinned host addresses.  n <= p returns -1.  If A is not positive definite the call returns n + j, j the
 *      1-based pivot in the basis (L_T = -inf and a zero gradient; after mi_gp_factor the handle is then not factored).
 *      Refused (-1, before any device call, with a text that names option 50) while the option is not 0: mi_gp_lml,
 *      mi_gp_lml_batch, mi_gp_lml_grad_batch, mi_gp_factor_batch, mi_gp_predict_batch, mi_gp_predict_u, mi_gp_predict_grad,
 *      mi_gp_predict_cov, mi_gp_append, mi_gp_logpdf, mi_gp_kfold, mi_gp_alpha and mi_gp_grad_x.  mi_gp_sample_cov,
 *      mi_gp_set_data, mi_gp_set_diag, mi_gp_reserve and the block-level entries are not affected.  The handle owns the scratch
 *      (H^T / G^T as 128 rows, V and Q as padded capacity x 128, the partial products and three 128 x 128 blocks of A, a few
 *      vectors): allocated by the first use, freed by mi_gp_destroy; mi_gp_reserve re-sizes it and keeps what mi_gp_predict needs
 *      (G^T, C_A^-1, beta^, b~), so the handle stays factored.  No refusal changes the handle's state.  The same call in the same state returns the same bits; every element a launch
 *      reads is written earlier in the same call (NaN in the strict upper triangle of W_dev, in work_dev or in the scratch
 *      changes nothing); the scheduling options change no bit; no sum uses atomics, every one runs in a fixed order.  Values
 *      outside 0..2 return -1, and so do 2 with d > 127 and 1 or 2 in a build without the tail (the host-only schedule-trace
 *      program).  Setting a value other than the current one ends the resident state exactly as mi_gp_set_data does; setting the
 *      current value changes nothing; with 0 the library enqueues exactly what it enqueues without the option.  Out of scope:
 *      the batched and sharded forms; cross-validation objectives, mi_gp_kfold, mi_gp_append and mi_gp_logpdf under a trend;
 *      data-side gradients (and with them warped fits under a trend); reading beta^ out; quadratic or user-supplied bases; a
 *      rank-deficiency test beyond n <= p.
 *   51 (not a tuning knob) the OUTPUTS: the number q of outputs modelled under ONE shared kernel and one noise, independent
 *      given theta, their log marginal likelihoods summed (the form scikit-learn's GaussianProcessRegressor gives a 2-D y);
 *      theta and mi_gp_num_theta() stay as they are.  1 (default) the single y, today's behaviour bit for bit; 2..128 q outputs.
 *      Y is n x q with columns y_o.  Under q >= 2 y_dev of mi_gp_buffers holds q vectors: output o occupies
 *      y_dev[o * lda .. o * lda + n), lda the leading dimension bound by mi_gp_set_data (known when data are bound, >= the padded
 *      capacity, so the layout survives mi_gp_reserve).  Output 0 is the y the factorisation reads as always.  The pointer is
 *      borrowed and read at evaluation time.  K_y is the noisy covariance of the entry point's own form (marginal in
 *      mi_gp_lml_grad, conditional in mi_gp_factor; the diagonal of mi_gp_set_diag included).
 *      mi_gp_lml_grad (option 48 = 0, option 50 = 0) runs the ordinary evaluation first (same launches, same schedule), then a
 *      tail on the handle's stream:
 *          V = K_y^-1 Y,   quad_o = y_o . V[:, o]
 *          L_MO = sum_o LML(y_o) = -q sum_i log L_ii - q n/2 log 2 pi - 1/2 sum_o quad_o
 *          dL_MO/dtheta_k = 1/2 sum_ij (V V^T - q K_y^-1)_ij dK_ij/dtheta_k                      (d/d jitter = d/d gv)
 *      -- Y^T staged as 128 rows (rows >= q and columns >= n zero), V by option 50's symmetric thin multiply on the fp64 matrix
 *      cores (the lower triangle of W_dev alone), the q quads in one kernel, the update W <- q W - V V^T over the lower trapezoid
 *      on the GEMM (alpha = -1, beta = q, k = 128), and the LML gradient's contraction kernel with that W and a zero vector in the
 *      place of alpha.  *lml_out = L_MO, grad_out its gradient in theta order; the call returns with the stream synchronised.
 *      Afterwards the lower triangle of W_dev holds q K^-1 - V V^T, not K^-1: the handle marks K^-1 not resident, as under a
 *      trend; mi_gp_lml_parts keeps the factorisation's logdet and output 0's quad.  A bad pivot is reported as under q = 1:
 *      info > 0, -inf, a zero gradient, no tail.
 *      mi_gp_factor additionally forms B^T = Y^T L^-T (the blocked solve of mi_gp_predict on 128 rows; b_o = L^-1 y_o) in scratch
 *      the handle owns, and mi_gp_predict returns, per point, with a* = L^-1 k(X, x*) (the row the call forms in work_dev)
 *          mean_dev[o * m + i] = a*_i . b_o   (q * m doubles, output-major),   var_dev[i] = kdiag - |a*_i|^2 (+ gv if pred_noise)
 *      (m doubles: the variance does not depend on y and is that of one output) from ONE pass over the rows of work_dev, whose
 *      contract (size, layout) does not change: a workgroup reads the rows of 16 points once, chunk by chunk, and forms their
 *      16 x q products with the rows of B^T on the fp64 matrix cores and |a*|^2 beside them.  mean_dev / var_dev are written once
 *      and may be pinned host addresses.
 *      Refused (-1, before any device call, with a text that names option 51) while q >= 2: mi_gp_lml, mi_gp_lml_batch,
 *      mi_gp_lml_grad_batch, mi_gp_factor_batch, mi_gp_predict_batch, mi_gp_predict_u, mi_gp_predict_grad, mi_gp_predict_cov,
 *      mi_gp_append, mi_gp_logpdf, mi_gp_kfold, mi_gp_alpha and mi_gp_grad_x; mi_gp_lml_grad under option 48 = 1 or option
 *      50 != 0; mi_gp_factor under option 50 != 0.  No refusal changes the handle's state.  The handle owns the scratch (Y^T / B^T
 *      as 128 rows, V and the multiply's partial products as padded capacity x 128, a zero vector, the q quads): allocated by the
 *      first use, freed by mi_gp_destroy; mi_gp_reserve re-sizes it and moves B^T, so the handle stays factored.  The same call in
 *      the same state returns the same bits; every element a launch reads is written earlier in the same call (NaN in the strict
 *      upper triangle of W_dev, in work_dev or in the scratch changes nothing); the scheduling options change no bit; no sum uses
 *      atomics, every one runs in a fixed order.  Values outside 1..128 return -1, and so does a value other than 1 in a build
 *      without the tail (the host-only schedule-trace program).  Setting a value other than the current one ends the resident
 *      state exactly as mi_gp_set_data does; setting the current value changes nothing; with 1 the library enqueues exactly what
 *      it enqueues without the option.  Out of scope: a kernel variance or a noise per output; correlated outputs
 *      (coregionalisation); the batched and sharded forms; data-side gradients and warps; cross-validation objectives and the
 *      trend under several outputs; mi_gp_append, mi_gp_logpdf and the joint covariance under several outputs; q > 128.
 * 8, 14, 16, 18, 19, 21, 26, 27, 30, 31, 38, 45 and 47 only change scheduling (bit-identical results); 20 moves tiles between the
 * two GEMM kernels (same k order); 2, 4-7, 9, 32, 35, 37 and 46 regroup sums (agreement to rounding), and so does 0 where it changes
 * the super-panel width (20 to 60 tile columns).
 * Unknown ids return -1.  (Round 1's options 1, 3, 10-13 -- GEMM variants, hipGraph replay, persistent bulk kernels,
 * exclusive leaf, fused leaf + strip -- and round 5's 29, 33, 34, 36, 39 -- forms that lost their A/B: the next-panel update's
 * occupancy as a knob, strided thin updates, that update in pieces, 64x128 tiles -- and round 3's 24, the assembly in two parts,
 * which stopped paying in round 6, are gone with the code they selected.)
 * Option 52 (not a tuning knob) the OUTPUT COVARIANCE of the q outputs of option 51: 0 (default) none -- the outputs independent
 *      under one kernel variance, today's behaviour bit for bit and launch for launch; 1 the outputs share a q x q covariance
 *      Sigma, vec(Y) ~ N(0, Sigma (x) K_y), under the Jeffreys prior p(Sigma) ~ |Sigma|^-(q+1)/2, and Sigma is integrated out in
 *      closed form (the separable multi-output emulator; Conti & O'Hagan 2010).  theta and mi_gp_num_theta() stay as they are; Y
 *      is bound as under option 51.  The option is read only while option 51 = q >= 2; with one output it is inert.  The result
 *      does not change under an invertible re-mixing or re-scaling of the outputs (Y -> Y M moves L_S by -n log|det M| and leaves
 *      the gradient), and it gives every output its own predictive variance.  It needs n >= q + 2: otherwise mi_gp_lml_grad and
 *      mi_gp_factor return -1 before any device call, with a text that names option 52.
 *      mi_gp_lml_grad runs the ordinary evaluation first (same launches, same schedule), then option 51's tail with S in the
 *      place of the quads:
 *          V = K_y^-1 Y,   S = Y^T V = C_S C_S^T                                                               (q x q)
 *          L_S = -q sum_i log L_ii - n sum_j log (C_S)_jj + log Gamma_q(n/2) - n q/2 log pi
 *          log Gamma_q(a) = q (q - 1) / 4 log pi + sum_{j = 1 .. q} lgamma(a + (1 - j) / 2)                     (on the host)
 *          dL_S/dtheta_k = 1/2 sum_ij (n V S^-1 V^T - q K_y^-1)_ij dK_ij/dtheta_k               (d/d jitter = d/d gv)
 *      -- S as option 50's block A: the k-segmented 128 x 128 Gram product Y^T V, its segments added in index order, the
 *      identity in the padding; the 128 x 128 leaf factorises it in place and its row-major inverse follows; one small kernel
 *      adds log (C_S)_jj in index order and forwards the bad-pivot word; Q = sqrt(n) V C_S^-T on the GEMM; the update
 *      W <- q W - Q Q^T over the lower trapezoid (alpha = -1, beta = q, k = 128); and the LML gradient's contraction kernel with
 *      that W and a zero vector in the place of alpha.  *lml_out = L_S.  Afterwards the lower triangle of W_dev holds
 *      q K^-1 - n V S^-1 V^T, and the handle marks K^-1 not resident, as under option 51; mi_gp_lml_parts keeps the factorisation's
 *      logdet and output 0's quad.  If S is not positive definite (a zero column of Y; collinear columns, as far as rounding
 *      leaves the pivot non-positive) the call returns n + j, j the 1-based pivot among the outputs, with L_S = -inf and a
 *      zero gradient, as option 50 does for its block; the handle stays usable.  A bad pivot of K_y is reported as always.
 *      L_S does not change under K_y -> c K_y (S scales by 1/c, log|K_y| by n log c): kv, gv and the jitter are identified up to
 *      a common factor only, which their priors must fix (for one kernel component without a diagonal of mi_gp_set_diag,
 *      kv dL_S/dkv + gv dL_S/dgv + jitter dL_S/djitter = 0).
 *      mi_gp_factor additionally keeps s_o = |b_o|^2 / (n - q - 1) for o < q (b_o = L^-1 y_o, the rows of option 51's B^T: the
 *      diagonal of S in the conditional form) in the handle's scratch, and mi_gp_predict writes
 *          mean_dev[o * m + i] exactly as under option 51, with the same bits,
 *          var_dev[o * m + i] = (kdiag - |a*_i|^2 (+ gv if pred_noise)) * s_o          (q * m doubles, output-major)
 *      -- the variance of the predictive multivariate t with n - q + 1 degrees of freedom -- from the same ONE pass over the
 *      rows of work_dev, whose contract (size, layout) does not change; var_dev must hold q * m doubles.  mi_gp_reserve carries
 *      s_o along with B^T, so the handle stays factored.
 *      Everything option 51 refuses stays refused, with option 51's text.  The same call in the same state returns the same
 *      bits; every element a launch reads is written earlier in the same call; the scheduling options change no bit; no sum
 *      uses atomics.  Values outside 0..1 return -1, and so does 1 in a build without option 51's tail (the host-only
 *      schedule-trace program).  Setting a value other than the current one ends the resident state exactly as mi_gp_set_data
 *      does (and frees the outputs' scratch, whose layout the value is part of); setting the current value changes nothing.
 *      Out of scope: the off-diagonal predictive covariance between outputs; reading Sigma out; q = 1 (the scale of one output
 *      integrated out); the batched and sharded forms; everything option 51 already lists. */
MI_GP_API int mi_gp_set_option(mi_gp_handle* h, int what, int value);
/* current value of a knob, the library's own defaults included; 40 (read-only): 1 once the handle has switched its cross-stream
 * edges to events by itself (option 26) */
MI_GP_API int mi_gp_get_option(mi_gp_handle* h, int what, int* value);
/* Option 53 (not a tuning knob) the MEAN SWEEP of mi_gp_predict_grad: 0 (default) today's call, bit for bit and launch for
 *      launch; 1 the call becomes the matrix-free sweep of the posterior mean and its input gradient,
 *          mu(x*) = sum_j k(x*, x_j) alpha_j,      d mu / d x*_m = sum_j alpha_j sum_c coef_c kv_c k_c'(r2_c) 2 (x*_m - x_jm) / l_cm^2
 *      with alpha = K^-1 y: O(n d) per point, no work rows and no m x n matrix, where every other prediction route pays O(n^2) per
 *      point for a variance -- the route of Saltelli designs, of E[grad mu grad mu^T] over the input priors and of mean-only
 *      samples of 1e5 .. 1e7 points.  Under 1: Xnew_dev is m x d with m >= 1 and no other limit on m; mean_dev receives m doubles or
 *      is NULL, dmean_dev receives m x d doubles or is NULL, at least one of them is given; work_dev, ldw, var_dev, dvar_dev and
 *      pred_noise are ignored -- NULL is allowed for them, nothing is written there.  Xnew_dev and the outputs are device-visible
 *      addresses as for mi_gp_predict (pinned host memory allowed).  Preconditions, those of today's call: a successful
 *      mi_gp_factor or mi_gp_append, Z_dev / W_dev bound, option 50 = 0 and option 51 = 1 (their texts); further d <= 128 (the
 *      (nkern + 1) * d LDS rule of the scalar kernel does not apply).  Every refusal returns -1 before any HIP call, with a text that
 *      names option 53, and changes no state.  The call makes U = L^-T and alpha resident (make_u_resident, exactly as today's call)
 *      and changes nothing else; the handle owns a scratch -- (capacity + 16) rows of the padded d doubles, the training points
 *      staged for the kernel by every call, and the partial sums of one pass of 16384 query points (4096 for d > 32: 16 parts of
 *      1 + d doubles per point, and for d > 32 the pass's points themselves) -- allocated by the first sweep, dropped by
 *      mi_gp_reserve, freed by mi_gp_destroy; nothing in it is kept between calls and no buffer grows with m.  It
 *      returns with the stream synchronised.
 *      Arithmetic: per component r2_c = sum_m ((x*_m - x_jm) (1 / l_cm))^2, the direct form of the gradient kernels and not the
 *      assembly's expansion -2 x.x' + |x|^2 + |x'|^2, whose residue of a few eps |x / l|^2 Exponential's dk/dr2 ~ 1 / r amplifies
 *      near r = 0; value and derivative per component and the + / * fold as in mi_gp_predict_grad's kernel; the differences
 *      (x*_m - x_jm) are accumulated, never x* sum C - sum C x_j, which cancels for short length scales; a coincident training
 *      point contributes 0 to the gradient.  One thread owns one query point and walks training points in index order.
 *      The training range is split over workgroups by a rule of n alone: 16 parts [y q, min((y + 1) q, n)), q = ceil(n / 16); a
 *      workgroup sums one part for 64 points, and a kernel of the library adds a point's 16 partial sums in part order.  Every
 *      sum runs in a fixed order, the same call in the same state returns the same bits, and a point's results do not depend
 *      on m, on its position in Xnew_dev or on the other points.
 *      Values outside 0..1 return -1, and so does 1 in a build without the sweep (the host-only schedule-trace program; the
 *      text says "not part of this build").  Setting it changes no resident state; mi_gp_get_option(53) reads it back.
 *      Out of scope: the sweep under a trend or several outputs; a batched (one theta per member) and a sharded form; variances;
 *      d > 128; second derivatives. */
/* Option 54 (not a tuning knob) the PATH SWEEP of mi_gp_predict_grad, S posterior sample paths by pathwise conditioning (Wilson
 *      et al. 2020, "Efficiently sampling functions from Gaussian process posteriors"): 0 (default) the call is what option 53
 *      says, bit for bit and launch for launch; S = 1..128 the call evaluates -- and on request first conditions -- S function
 *      draws
 *          f_s(x*) = sum_i W[i,s] cos(om_i . x* + b_i) + sum_j k(x*, x_j) V[j,s],     V[:,s] = K_y^-1 (y - Phi(X) W[:,s] - E[:,s])
 *      -- a prior draw from F random Fourier features of the kernel's spectral measure (the only approximation: it vanishes at
 *      the data) plus a kernel-weighted update, one weight per training point.  A draw is a consistent function: any number of
 *      points, in any number of calls, with its input gradient, at O((n + F) d) per point and path, without an M x M matrix.
 *      Option 55 is F, the number of features: a multiple of 16 in 16..65536, default 1024, read only while option 54 >= 1.
 *      Under option 54 = S: work_dev is the caller's PATH BLOCK in device memory and ldw its row stride, even and >= S.  With
 *      d the input dimension and n the current number of points, the block holds, in doubles from its start,
 *          Omega at 0                      F x d, row-major: the frequencies om_i
 *          b     at F * d                  F: the phases b_i
 *          W     at F * d + F              F rows, ldw apart: the feature weights
 *          V     at F * d + F + F * ldw    n rows, ldw apart: the update weights (on entry to a conditioning call: the noise draw E)
 *      -- F * d + F + (F + n) * ldw doubles.  Columns s < S of W and V belong to path s; the padding columns are never read or
 *      written.  pred_noise is read as `condition`; var_dev and dvar_dev are ignored (NULL allowed, nothing is written there).
 *      condition = 1: the V rows hold E ~ N(0, K_y - K_f) on entry and the call replaces them by V = K_y^-1 (y - Phi(X) W - E) on
 *      the handle's stream: Phi(X) W from the feature half of the sweep kernel at the training points, the residual as a 128-row
 *      block R^T (rows from S on and columns from n on zero), R^T U and (R^T U) U^T on the GEMM against the resident U = L^-T
 *      (mi_gp_predict_u's and mi_gp_append's launches), and the rows written back as columns.  m = 0 is allowed in this form --
 *      conditioning only, Xnew_dev and the outputs NULL; m >= 1 goes on to the evaluation.  condition = 0: the block is used as
 *      it is (any V and W), and m >= 1.  The evaluation writes, for mean_dev, dmean_dev or both (at least one given when m >= 1),
 *          mean_dev[s * m + p]            = f_s(x*_p)                                    (S * m doubles, path-major as option 51's)
 *          dmean_dev[(s * m + p) * d + k] = d f_s / d x*_pk                              (S * m * d doubles)
 *      with no upper limit on m.  Preconditions, option 53's: a successful mi_gp_factor or mi_gp_append, Z_dev / W_dev bound,
 *      option 50 = 0 and option 51 = 1 (their texts); further d <= 32 in this version (the text names option 54 and the limit).
 *      ldw odd or < S, a NULL block, both outputs NULL with m >= 1, m = 0 with condition = 0 and m < 0 are refused, and so is the
 *      call while options 53 = 1 and 54 >= 1 are both set.  Every refusal returns -1 before any HIP call and changes nothing,
 *      the block included.  Apart from making U and alpha resident (make_u_resident, as today's call) no handle state changes:
 *      mi_gp_alpha, the mean sweep and mi_gp_predict_grad return the bits they returned before.  The handle owns a scratch -- the
 *      points, frequencies and weights staged per call in padded rows, the partial sums of one pass (32 parts of 4096 points and
 *      128 columns) and the conditioning's two 128-row blocks -- allocated by the first call, re-sized when F grows, dropped by
 *      mi_gp_reserve, freed by mi_gp_destroy; it holds nothing between calls and does not grow with m.  The call returns with the
 *      stream synchronised.  THE LIBRARY CANNOT KNOW that a block was conditioned on another factorisation (other theta, data or
 *      n): the caller keeps a block with the factorisation that made it.
 *      Arithmetic: option 53's for the kernel sum -- r2 in the direct form, value and derivative per component and the + / * fold
 *      as in the gradient kernels, the differences (x*_m - x_jm) accumulated, a coincident training point contributing 0 to the
 *      gradient; per feature the phase b_i + sum_u om_iu x*_u in index order, one cos and with the gradient one sin, both with
 *      an exact reduction of arguments of any size (Matern and Exponential frequencies are heavy-tailed).  One thread owns one
 *      query point and T paths; the pair's kernel value is formed once and used T times.  The training range is cut into 16
 *      parts [y q, min((y + 1) q, n)), q = ceil(n / 16), the feature range into 16 parts of F / 16: rules of n alone and of F
 *      alone; a kernel of the library adds the 32 partial sums in part order, training parts first.  Every sum runs in a fixed
 *      order of fused multiply-adds: the bits of path s at point p depend on the point, column s of V and W, Omega, b and the
 *      resident state and on nothing else -- not on m, the position of p, S, the other columns, whether the gradient was asked
 *      for, or a repetition.
 *      Values outside 0..128 (option 54) and outside the multiples of 16 in 16..65536 (option 55) return -1 with a text that
 *      names the option, and so does option 54 >= 1 in a build without the path sweep (the host-only schedule-trace program; the
 *      text says "not part of this build").  Setting either changes no resident state; mi_gp_get_option reads them back.
 *      Out of scope: d > 32; a trend or several outputs; batched and sharded forms; draws of noisy observations (add the noise
 *      on the host); variances. */
/* Option 56 (not a tuning knob) the DESIGN CALL of mi_gp_predict_cov, a greedy variance-reduction design (integrated variance
 *      reduction, ALC / IMSE: Cohn 1996, Gramacy & Lee 2009): 0 (default) the call is the joint conditional, bit for bit and launch
 *      for launch; b = 1..128 the call selects up to b of the candidate points it is given, each the one whose observation lowers
 *      the latent posterior variance averaged over a reference sample R the most, given the ones chosen before it:
 *          gain(c) = (1 / Mr) sum_r cov(c, r)^2 / v(c),      v(c) = var_latent(c) + jitter (+ sqrt(gv)^2 with pred_noise = 1)
 *      with cov and var_latent the posterior's at the factored theta.  gain(c) is exactly the drop of mean_r var_latent(r) when
 *      one observation at c is appended (mi_gp_append, pred_noise = 1), whatever its value: a batch is chosen before the target
 *      runs once.  Option 57 is Mr, the number of reference points, >= 0, read only while option 56 >= 1; Mr = 0 is the plain
 *      maximum-variance criterion, gain(c) = var_latent(c), with no reference set.
 *      Under option 56 = b: Xnew_dev is (Mc + Mr) x d, the Mc >= 1 candidates and then the Mr reference points, m = Mc + Mr.
 *      work_dev receives the rows A = L^-1 K(X, .) of the candidates and, from row ceil(Mc/128)*128 on, those of the reference
 *      points: ceil(Mc/128)*128 + ceil(Mr/128)*128 rows, ldw as for mi_gp_predict.  cov_dev receives G, the running cov(C, R):
 *      ceil(Mc/128)*128 rows ldc apart, ldc even and >= ceil(Mr/128)*128; with Mr = 0 it is not touched and may be NULL.
 *      mean_dev receives Mc + 2 b + 1 doubles:
 *          [0, Mc)              the round-0 gains of all candidates (NaN where v is not a finite positive number)
 *          [Mc, Mc + b)         the chosen candidates' indices as doubles, in order, -1 beyond the count
 *          [Mc + b, Mc + 2 b)   their gains at the moment of choice, 0 beyond the count
 *          [Mc + 2 b]           the count: fewer than b when no candidate is left or the best score is not > 0
 *      Setup, from the launchers of mi_gp_predict and mi_gp_predict_cov: the cross-assembly of both point sets and one blocked
 *      solve over their rows, the assembly of K(C, R) into cov_dev, ONE GEMM G -= A_C A_R^T (k = padded n), v from mi_gp_predict's
 *      row reduction and the rows' sums of squares of G.  Then b steps on the handle's stream without a host synchronisation, the
 *      pivot index in device memory: (1) score(c) = sum_r G[c][r]^2 / (Mr v[c]) and its arg-max over the alive candidates with a
 *      finite v > 0, ties to the lowest index; (2) the candidate column g = cov_t(C, c*) = k(C, c*) - A_C a_c* less the earlier
 *      pivots' contributions g_s g_s[c*] / v*_s, one pass over the candidates' rows of A; (3) one fused pass over the alive rows,
 *      G[c][:] -= (g[c] / v*) G[c*][:] with the row's new sum of squares, and v[c] -= g[c]^2 / v*.  The chosen candidate is dead
 *      from step (1) on and the pass skips dead rows, so the pivot row every workgroup reads is written by none.
 *      No atomics; every row sum is lane-strided partial sums (a lane takes pairs of elements) and mi_gp_predict's wave tree, so a
 *      row's bits do not depend on the grid; the same call in the same state returns the same bits; every element a launch reads is written earlier in the call
 *      (NaN in work_dev, cov_dev or the handle's scratch changes nothing).  The handle owns a scratch of (4 + b) ceil(Mc/128)*128
 *      + 130 doubles -- v, the row sums, the candidate columns of the steps so far, v* per step, the alive mask and the pivot --
 *      allocated by the first call, grown by a call that needs more, freed by mi_gp_destroy; it holds nothing between calls.
 *      The call changes no handle state, returns with the stream synchronised and works after mi_gp_append.
 *      Every refusal returns -1 before any HIP call with a text that names option 56: no factorisation, a per-point diagonal
 *      (mi_gp_set_diag), option 50 != 0 or option 51 >= 2, m < Mr + 1, ldw odd or < padded n, ldc odd or too small, a NULL buffer.
 *      Values outside 0..128 (option 56) and below 0 (option 57) return -1 with a text that names the option, and so does option
 *      56 >= 1 in a build without the design call (the text says "not part of this build").  Setting either changes no resident
 *      state; mi_gp_get_option reads them back.
 *      Out of scope: continuous refinement of a chosen point; a trend, several outputs, a per-point diagonal or a sparse fit;
 *      batched and sharded handles; criteria that read y. */

/* profiling: level 0 none, 1 per-phase HIP events, 2 additionally per-GEMM-launch HIP events */
MI_GP_API int mi_gp_set_profiling(mi_gp_handle* h, int level);
/* out[0..13] = assemble_ms, cholesky_ms, reduce_ms, total_ms, gemm_ms (sum over launches),
 *             gemm_flops (algorithmic), number of gemm launches, trtri_ms, lauum_ms, contract_ms,
 *             then the same three GEMM figures for the 128x128-tile kernel (gemm_f64_kernel_b) alone
 *             -- of the last evaluation (profiling level >= 1);
 *   out[13] = host time spent enqueueing the last single evaluation's launches, ms (measured at every profiling level)
 *   out[14..16] = conditional-block, weights and gradient-kernel ms of the last mi_gp_logpdf (profiling level >= 1) */
MI_GP_API int mi_gp_timers(mi_gp_handle* h, double* out, int n);

/* ---- block-level operations (also used by the multi-GPU driver and the parity tests) ---- */

/* C = beta*C + alpha*op(A)*op(B) in fp64 on v_mfma_f64_16x16x4_f64; row-major, m,n multiples of
 * 128, k a positive multiple of 32.  transa=0: A is m x k; 1: A is k x m.  transb=0: B is k x n; 1: B is n x k.
 * tri=1 computes only tiles on/below the block diagonal (the element-wise lower triangle is
 * guaranteed, the strict upper part of diagonal blocks is unspecified); kmode restricts k per tile for triangular
 * operands (0 full, 1 k>=col-tile start, 2 k<row-tile end, 3 k>=row-tile start, 4 k<col-tile end), i.e. it presumes
 * op(B) lower (1), op(A) lower (2), op(A) upper (3) or op(B) upper (4) triangular in its leading square; the skipped
 * k range must hold zeros.  kmode 1 and 4 need k >= n, 2 and 3 k >= m (the tile's k range then stays inside [0, k)).
 * beta = 0 never reads C (NaN there does not propagate).  Anything else returns -1 before touching the device.
 * Replaces the OpenBLAS dgemm/dsyrk calls inside LAPACK dpotrf/dtrtri/dlauum that PyTensor's
 * Cholesky Op reaches (gpmcmc.py:313; scipy.linalg.cholesky). */
MI_GP_API int mi_gp_gemm_f64(int transa, int transb, int m, int n, int k, double alpha, const double* A_dev, long lda,
                   const double* B_dev, long ldb, double beta, double* C_dev, long ldc, int tri, int kmode,
                   int batch, long strideA, long strideB, long strideC, void* hip_stream);

/* The same product (batch 1) with the launcher's knobs per call: launches with fewer than small_below 128x128 tiles run on
 * 64x64 tiles (handle option 7), tail_small (option 9), band height of the trapezoid tile order (option 14), one workgroup
 * per CU (option 8's effect).  For A/B measurements of single launches and the GEMM tests. */
MI_GP_API int mi_gp_gemm_f64_tuned(int transa, int transb, int m, int n, int k, double alpha, const double* A_dev, long lda,
                         const double* B_dev, long ldb, double beta, double* C_dev, long ldc, int tri, int kmode,
                         int small_below, int tail_small, int band, int one_per_cu, void* hip_stream);

/* C = beta*C + alpha*A*B^T (tri as above) with both operands stored as k-segments: segment g (kseg columns, a multiple of
 * 128) of A at A_dev + g * kseg_stride with rows lda apart, the same for B.  This is how the GEMM kernels read the sharded
 * driver's piece-major panel buffers (one contiguous piece per tile column, sent as soon as it is final).  small_below < 0:
 * the launcher's default. */
MI_GP_API int mi_gp_gemm_nt_kseg(int m, int n, int k, double alpha, const double* A_dev, long lda, const double* B_dev, long ldb,
                       int kseg, long kseg_stride, double beta, double* C_dev, long ldc, int tri, int small_below,
                       void* hip_stream);

/* K(Xrows, Xcols) for one rectangular block of a (distributed) covariance: rows row0.. and columns
 * col0.. of the global matrix; noise + jitter go on the global diagonal, identity in the padding
 * (rows >= nrows / columns >= ncols of the padded block).  Same kernel as the single-GPU assembly
 * (gpmcmc.py:282-312).  kernel_ids[0 .. nkern) must be MI_GP_* ids and ops[0 .. nkern-1) MI_GP_OP_* (ops may be null
 * for one component), here, in mi_gp_grad_contract_block and in mi_gp_create / mi_gp_shard_create: else -1. */
MI_GP_API int mi_gp_assemble_block(int d, int nkern, const int* kernel_ids, const int* ops, const double* theta_dev,
                         const double* Xrows_dev, int nrows, const double* Xcols_dev, int ncols, int row0, int col0,
                         double* K_dev, long ldk, int rows_pad, int cols_pad, int noise_form, void* hip_stream);

/* Factor the w_tiles leading 128-column tiles of a (row_tiles x w_tiles)-tile lower trapezoid in place:
 * diagonal leaves, strip solves of all rows below, in-panel updates.  dinv_dev: w_tiles * 16384 doubles that receive
 * the explicit 128x128 inverses of the panel's diagonal blocks (lower triangular, in an internal tile order; the strip solves are
 * products with them, and mi_gp_trsm_block reuses them); *info_dev receives atomicMin(col_base + bad pivot index + 1).
 * LAPACK dpotrf panel step. */
MI_GP_API int mi_gp_chol_panel(double* A_dev, long lda, int row_tiles, int w_tiles, double* dinv_dev, int* info_dev,
                     int col_base, void* hip_stream);

/* out_dev[1] = sum_i log L[i][i], out_dev[2] = sum_i beta[i]^2 over n >= 1 entries (one workgroup), and
 * out_dev[0] = -n/2 log(2 pi) - out_dev[2]/2 - out_dev[1]: all three are overwritten, out_dev[3..] is not touched. */
MI_GP_API int mi_gp_lml_partial(const double* L_dev, long ld, const double* beta_dev, int n, double* out_dev, void* hip_stream);

/* ---- sharded gradient ("gradient at C4 scale needs distributed K^-1"): the reference gets dLML/dtheta from
 * pytensor.grad through Cholesky.L_op behind pm.find_MAP / pm.sample (gpmcmc.py:345,351); the sharded driver
 * (andvaranaut_amd/distributed.py) builds it from these blocks. */

/* X L^T = B in place (X = B L^-T) for the 128-column tiles [c0_tiles, c0_tiles + w_tiles) of a complete lower factor
 * L_dev (element (0,0) first, leading dimension ldl); dinv_dev: the 16384-double leaf inverses mi_gp_chol_panel wrote,
 * indexed by global tile; B_dev points at the first of those columns of the m-row right-hand side (m multiple of 128).
 * With B = rows J of the identity this yields rows J of U = L^-T.  LAPACK dtrsm('R','L','T','N'). */
MI_GP_API int mi_gp_trsm_block(const double* L_dev, long ldl, const double* dinv_dev, int c0_tiles, int w_tiles, double* B_dev,
                     long ldb, int m, void* hip_stream);

/* out = U x for an upper-triangular n x n U (alpha = L^-T beta, gpmcmc.py:315). */
MI_GP_API int mi_gp_trmv_upper(const double* U_dev, long ld, const double* x_dev, int n, double* out_dev, void* hip_stream);

/* grad_dev[ntheta] = 1/2 sum (alpha_i alpha_j - Kinv_ij) dK_ij/dtheta over the column slab [col0, col0 + cols) of the
 * lower triangle (rows >= col0; diagonal counted once).  W_dev points at element (row0, col0) of K^-1 (row0 <= col0,
 * all multiples of 64); part_dev: mi_gp_grad_contract_block_scratch() doubles.  Slab sums add up to mi_gp_lml_grad's. */
MI_GP_API long mi_gp_grad_contract_block_scratch(int n, int col0, int cols, int ntheta);
MI_GP_API int mi_gp_grad_contract_block(int d, int nkern, const int* kernel_ids, const int* ops, const double* theta_dev,
                              const double* X_dev, int n, const double* W_dev, long ldw, int row0, int col0, int cols,
                              const double* alpha_dev, double* part_dev, long part_len, double* grad_dev,
                              void* hip_stream);

/* ---- sharded factorisation, one call per panel step (SURVEY 8e second row; BASELINE config 4).  The covariance is
 * distributed over `world` ranks in 1-D block-cyclic column panels of panel_tiles * 128 columns (panel j belongs to rank
 * j % world); a rank stores its panels side by side (local column li * pw for its li-th panel) with GLOBAL rows.  The
 * exchange itself (one broadcast per tile column of the panel, out of P_dev[j % 2]) stays with the caller (torch.distributed /
 * RCCL); these entries enqueue everything else of a step behind one call:
 *   begin : assemble the owned panels (+ their y^T rows); the owner of panel 0 factors it and stages it into P_dev[0]
 *   step j: panel j is complete in P_dev[j % 2] and visible to main_stream AND side_stream.  The owner of panel j+1 updates it with
 *           panel j, factors it and stages it into P_dev[(j+1) % 2] on side_stream (the caller broadcasts it under that
 *           stream); then ONE GEMM launch on main_stream updates every owned panel > j+1 (panel-list mode of the kernel)
 *   finish: main_stream waits for side_stream; out_dev[1] = sum log L_ii, out_dev[2] = sum beta_i^2 over the owned panels
 * A panel buffer is PIECE-major: piece c (tile column c of the panel) starts at P_dev[b] + c * ldp and holds rows
 * r0 = j * pw .. np + 127 of that column at a row stride of 128 doubles (np = padded n; rows np.. = the y^T block whose
 * first row becomes beta^T), then the column's 128 x 128 leaf inverse (the sharded gradient needs it everywhere):
 * (np + 128 - r0 + 128) * 128 contiguous doubles = ONE broadcast; ldp >= (np + 256) * 128.  On several ranks the owner
 * stages piece c right behind column c's strip (option 5) and the caller sends it -- mi_gp_shard_wait_piece(s, c, stream)
 * orders `stream` behind that staging -- while columns c + 1 .. are still being factored: only the last piece's
 * transfer is exposed.
 * world / rank need not be a process group's: a single process can play rank r of W (tools/emulate_rank.py).
 * Replaces the per-panel LAPACK dpotrf steps behind pt.slinalg.cholesky (gpmcmc.py:313) at a size one GPU need not hold. */
typedef struct mi_gp_shard mi_gp_shard;
typedef struct {
  int n, d, nkern;
  int kernel_ids[MI_GP_MAX_KERN];
  int ops[MI_GP_MAX_KERN];
  int panel_tiles;         /* panel width in 128-column tiles */
  int world, rank;
  int device;
  const double* X_dev;     /* n x d, replicated */
  const double* y_dev;     /* n */
  double* K_dev;           /* (np + 128) x ldk, ldk >= owned panels * pw, even */
  long ldk;
  double* P_dev[2];        /* panel buffers, panel_tiles pieces of ldp doubles each */
  long ldp;                /* piece stride, >= (np + 256) * 128 */
  const double* theta_dev; /* C-ABI theta on the device (the caller uploads it before begin) */
  int* info_dev;           /* [1] bad-pivot word: reset by begin, atomicMin(global column + 1) */
  double* out_dev;         /* [4] scalars of finish */
} mi_gp_shard_config;
MI_GP_API int mi_gp_shard_create(const mi_gp_shard_config* cfg, mi_gp_shard** out);
MI_GP_API int mi_gp_shard_destroy(mi_gp_shard* s);
MI_GP_API int mi_gp_shard_begin(mi_gp_shard* s, int noise_form, void* main_stream, void* side_stream);
MI_GP_API int mi_gp_shard_step(mi_gp_shard* s, int j, void* main_stream, void* side_stream);
MI_GP_API int mi_gp_shard_finish(mi_gp_shard* s, void* main_stream, void* side_stream);
/* `stream` waits until tile column c of the panel this rank factored last (begin: panel 0; step j: panel j + 1) is staged */
MI_GP_API int mi_gp_shard_wait_piece(mi_gp_shard* s, int c, void* hip_stream);
/* options: 0 bulk updates at one workgroup per CU while this rank's side stream factors the next panel (default 1);
 *          1 record per-step HIP events (update / factor / stage on the side stream, bulk on the main stream);
 *          2 update the panel this rank factors in the NEXT step first and alone, so that its chain does not wait for the
 *            whole bulk update (default 1; that panel's update may run on the other tile size: agreement to rounding);
 *          3 the owner's chain (update + factor + stage of the next panel) runs on main_stream AHEAD of its bulk update
 *            instead of beside it on side_stream (default: 1 when world > 1 -- every other rank waits for that chain, and
 *            alone on the chip it is 2-3x shorter than next to a bulk update; 0 on one rank).  Either way side_stream is
 *            ordered behind the staging when the call returns: the caller broadcasts the panel under side_stream.
 * what = 4: tiles of a bulk update that run one workgroup per CU beside this rank's own chain, the rest two per CU (2048;
 *            0: the whole update one per CU).
 * what = 5: a chain on main_stream stages every tile column behind its strip (1), and the previous panel's update takes the
 *            first tile column alone and first so that it is final, staged and sent early (2, the default); 0: the panel is
 *            staged behind its last column.  0 and 1 give the same bits; 2 regroups launches (agreement to rounding).
 * Reproducibility: the sharded factorisation is bit-reproducible for a FIXED world size, panel width and option set.
 * Options 2 and 3 and the world size change which launches update a panel (the early next-panel update goes through the
 * ordinary launcher and may run on 64x64 tiles where the panel-list launch uses 128x128), i.e. they regroup sums: results
 * then agree to rounding (1e-11 relative on the LML in the tests), not bit for bit. */
MI_GP_API int mi_gp_shard_set_option(mi_gp_shard* s, int what, int value);
/* per-step phase times of the last evaluation (option 1; call after synchronising): out[4 * j + 0..3] =
 * update_ms, factor_ms, stage_ms, bulk_ms of step j (0 where the step had no such phase; factor of panel 0 is in
 * out[4 * npanels + 1], its staging in out[4 * npanels + 2]); returns the number of steps written, < 0 on error */
MI_GP_API int mi_gp_shard_times(mi_gp_shard* s, double* out, int max_steps);
/* out[j * panel_tiles + c] = ms from the start of step j's chain to the end of the staging of tile column c of the panel it
 * produces (row npanels: panel 0, from the start of its factorisation); option 1; returns the number of steps written */
MI_GP_API int mi_gp_shard_piece_times(mi_gp_shard* s, double* out, int max_steps);
/* 0: the chain runs on side_stream (it must then wait for panel j as well), 1: on main_stream (option 3) */
MI_GP_API int mi_gp_shard_chain_stream(const mi_gp_shard* s);
MI_GP_API const char* mi_gp_shard_last_error(mi_gp_shard* s);

#ifdef __cplusplus
}
#endif
#endif
