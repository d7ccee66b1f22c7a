// Internal kernel-launch interface of libmi_gp.so (not part of the C-ABI; see include/mi_gp.h).
#pragma once
#include <hip/hip_runtime.h>

namespace migp {

// Batched evaluation (mi_gp_lml_batch / mi_gp_lml_grad_batch): nb covariances of the SAME inputs, one theta each, factorised
// in lockstep -- every launch carries blockIdx.z = problem, so the latency-bound panel chain of one problem runs beside the
// chains of the others.  Strides are in elements; nb = 1 with zero strides is the ordinary single evaluation.
struct Batch {
  int nb = 1;
  long sK = 0, sZ = 0, sW = 0;  // between consecutive problems' K / Z (U = L^-T) / W (K^-1) matrices
  long sdinv = 0;               // ... leaf inverses (ntc * MINV_ELEMS doubles)
  long salpha = 0;              // ... alpha vectors (np doubles)
  long spart = 0;               // ... gradient partial sums
  int stheta = 0;               // ... theta vectors (device copy, pinned host source, pinned gradient)
  int sinfo = 0;                // ... bad-pivot words (ints)
  int sout = 0;                 // ... scalar records in pinned host memory (doubles)
  long swork = 0;               // ... prediction work blocks (mi_gp_predict_batch: K(X*, X) -> L^-1 K(X, X*), one per problem)
};

constexpr double LOG_2PI = 1.8378770664093453;

// The (sum, first bad index) pairs of a workgroup of 256 threads meet in a fixed tree: every thread gets the sum and the
// smallest index (a thread without one passes 0x7fffffff).
__device__ __forceinline__ void tree_sum_first_256(double& acc, int& first) {
  __shared__ double sum[256];
  __shared__ int bad[256];
  const int t = threadIdx.x;
  sum[t] = acc;
  bad[t] = first;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) {
      sum[t] += sum[t + w];
      bad[t] = min(bad[t], bad[t + w]);
    }
    __syncthreads();
  }
  acc = sum[0];
  first = bad[0];
}

// ---------------------------------------------------------------- gemm_f64.hip
// C[mt*128 x nt*128] = beta*C + alpha * op(A) * op(B), all fp64 row-major with leading dimensions.
struct GemmParams {
  const double* A;
  const double* B;
  double* C;
  long lda, ldb, ldc;
  long strideA, strideB, strideC;  // batch strides in elements (blockIdx.z)
  // two-level batch (node-batched launches of the triangular inverse for nb problems): blockIdx.z = z1 + batch1 * z2, level-2
  // strides apply to z2; batch1 = 0: one level
  int batch1 = 0;
  long strideA2 = 0, strideB2 = 0, strideC2 = 0;
  int mt, nt;                      // output tiles (128 x 128) in rows / columns
  int k;                           // contraction length, multiple of 32
  int tri;                         // 1: only tiles with tj <= min(ti, nt-1)  (SYRK / trapezoid)
  int kmode;                       // 0 full k; 1 k >= tj*128; 2 k < (ti+1)*128; 3 k >= ti*128; 4 k < (tj+1)*128
  double alpha, beta;
  // launcher options (per call; a handle keeps its own values, mi_gp_set_option 7 / 14)
  int small_below = 1024;           // launches with fewer 128x128 tiles than this run on the 64x64-tile kernel
  int band = 8;                     // band height (tile rows) of the band-column-major order of uniform-k trapezoid launches, 0 = row-major
  int hiprio = 0;                   // 64x64-tile kernel only: raise the waves' issue priority (launches on the panel chain)
  int one_per_cu = 0;               // request > half a CU's LDS so that one workgroup per CU runs (leaves room for
                                    // the panel chain's leaf / strip kernels next to a bulk update)
  int tail_small = 1;               // uniform-k 128x128-tile launches: the tiles beyond the last full round of 512 go to the
                                    // 64x64-tile kernel in a second launch (mi_gp_set_option 9)
  // 128x128-tile launches only: restrict the launch to tiles [tile0, tile0 + tile_cnt) of the enumeration (tile_cnt 0: all).
  // The Cholesky driver splits a bulk update into a part that runs one workgroup per CU beside the panel chain and a part
  // that runs two per CU after it (mi_gp_set_option 18); which kernel computes which tile does not depend on the split.
  int tile0 = 0, tile_cnt = 0;
  // uniform-k trapezoid launches on the 128x128-tile kernel: enumerate the tiles of the first `fc` tile columns first (row by
  // row, like a narrow trapezoid), then the rest in the banded order.  With a sub-range launch over a prefix this lets the
  // driver finish the NEXT super-panel's columns ahead of the rest of a trailing update inside ONE enumeration.
  int fc = 0;
  // k-segmented operands (NT form, kmode 0 only): A and B are stored as k-segments of `kseg` columns (a multiple of 128),
  // segment g of an operand at base + g * kseg_stride doubles, rows lda / ldb apart inside a segment.  The sharded driver's
  // panel buffer is laid out this way (one contiguous piece per tile column, broadcast as soon as it is final).  0: one segment.
  int kseg = 0;
  long kseg_stride = 0;
  // k-segmented UPDATE (kmode 0, beta = 1): every kflush columns of k (a multiple of 16; the driver uses 128) the tile takes the
  // partial sum, C = beta C + alpha acc rounded there, and the accumulators restart -- the bits of one launch per segment in one
  // launch, with C read and written once.  Such launches run on the 64x64-tile kernel whatever their size.  0: off.
  int kflush = 0;
  // set by the launcher for that second launch: 64x64 tile 4 e + quadrant belongs to 128x128 tile sub_base + e of the
  // parent enumeration (sub_mt x sub_nt tiles of 128); -1: off
  int sub_base = -1, sub_mt = 0, sub_nt = 0;
  // The factorisation's trapezoids end in the y^T tile row: rows np .. np + 127 hold y^T in row np and zeros below, so the LOWER
  // 64-row half of that tile row is all zeros before and after every update.  1: the 64x64-tile kernel's workgroups of that half
  // return at once (2-8 % of the workgroups of an update at N = 2048 .. 8192; the 128x128-tile kernel computes whole tiles)
  int dead_last_half = 0;
  // Panel-list mode (pl != nullptr; sharded driver, api_shard.hip): ONE launch updates the lower trapezoids of pl_n column
  // panels of a block-cyclically distributed matrix, C_e -= P[rows >= g_e] P[rows of panel e]^T for e = pl_first ...
  // pl[e] = {cum, g, ccol, w}: 128x128 tiles of the panels before e, global tile row of panel e's diagonal block, tile
  // column of its first column in C (local storage), width in tile columns; pl[count].cum closes the table.  C's rows are
  // global rows; A = B = the row-panel buffer whose row 0 is global tile row pl_abase; pl_rows = global tile rows (with the
  // y block).  NT form, kmode 0, alpha/beta as given.  mt / nt are ignored.
  const int4* pl = nullptr;
  int pl_first = 0, pl_n = 0, pl_abase = 0, pl_rows = 0;
  int pl_tiles = 0;  // pl[pl_first + pl_n].cum - pl[pl_first].cum (the host knows the table)
};
// opX_kmajor = 0: operand stored [x][k] (A row-major m x k / B stored n x k, i.e. "B^T");
// opX_kmajor = 1: operand stored [k][x].
// part: 0 the whole product; 1 / 2 only the first / second launch of a split one (per-launch event timing); see gemm_tail_tiles
hipError_t launch_gemm_f64(const GemmParams& p, int opA_kmajor, int opB_kmajor, int batch, hipStream_t stream, int part = 0);
int gemm_tail_tiles(const GemmParams& p, int batch);  // 128x128 tiles that the second launch of a split product takes (0: not split)
hipError_t gemm_f64_enable_lds();
bool gemm_uses_small_tiles(const GemmParams& p, int batch);  // true: the 64x64-tile kernel will run

// ---------------------------------------------------------------- leaf_f64.hip
hipError_t leaf_enable_lds();
constexpr int MINV_ELEMS = 128 * 128;  // doubles per leaf inverse
// in-place lower Cholesky of one 128x128 diagonal block; minv receives M = L^-1 (128 x 128 lower triangular, 16x16 tiles in the strip kernel's operand order,
// zeros above the diagonal inside the diagonal 16x16 tiles; the tiles above the block diagonal are not written and
// never read); *info gets atomicMin(col0 + j + 1) on a bad pivot.
// yrow (optional): row 0 of the 128-row block right below Ablk, solved in place against the leaf's inverse (beta = y M^T)
// wait_ptr (optional): the launch ends only once *wait_ptr >= wait_val (a cross-stream signal; see leaf_f64.hip)
hipError_t launch_potrf_leaf128(double* Ablk, long lda, double* minv, int col0, int* info, hipStream_t stream,
                                double* yrow = nullptr, const Batch* bt = nullptr, const unsigned* wait_ptr = nullptr,
                                unsigned wait_val = 0, int poll_log2 = 22, unsigned* start_wr = nullptr);
// (start_wr, optional: raised to wait_val by the first workgroup as it starts)
// one lane: *wr = val (if wr), then wait for *wt >= val (if wt); a poll that gives up (after 2^poll_log2 sleeps) puts
// SIGNAL_TIMEOUT_INFO into the nb bad-pivot words info[p * sinfo]
constexpr int SIGNAL_TIMEOUT_INFO = -99;
hipError_t launch_signal_write_wait(unsigned* wr, const unsigned* wt, unsigned val, int* info, hipStream_t stream, int nb = 1,
                                    int sinfo = 0, int poll_log2 = 22);
// element (row, col) of a 128 x 128 block kept as 16x16 tiles in the strip kernel's MFMA operand order (leaf_f64.hip: the leaf's
// inverse, the strips' operand-order copies of their first rows)
__device__ __forceinline__ int minv_index(int row, int col) {
  const int jb = row >> 4, n = row & 15, kb = col >> 4, c = col & 15;
  return (jb * 8 + kb) * 256 + (c & 2) * 64 + ((c >> 2) * 16 + n) * 2 + (c & 1);
}

// ---------------------------------------------------------------- thin_f64.hip
// C[ti, tj] -= P[ti] P[tj]^T over the lower trapezoid of mt x nt tiles (tj <= ti), k = 128 (nt <= 2) or k = 256 (nt = 1):
// 16-row x 64-column workgroups, for the panel chain's short updates.  wr (optional): workgroup 0 raises *wr to val
// lsw: the rows of P that are the B operand (tile rows 0 .. nt - 1) in operand order, as the strip in front of the update wrote
// them (launch_trsm_strip128's lsw); k = 256: the B operand's first 128 k from lsw, the other 128 from lsw2 (two strips' copies)
hipError_t launch_syrk_thin(const double* P, double* C, long ld, int mt, int nt, int k, hipStream_t stream, const Batch* bt,
                            unsigned* wr, unsigned val, const double* lsw, const double* lsw2 = nullptr);

// ---------------------------------------------------------------- leaf_f64.hip (continued)
// X * L^T = B in place on the m x 128 panel B (m multiple of 16, ldb even) as X = B * M^T with the leaf's inverse M.
// lsw (optional): the first lsw_blocks 16-row groups of X are also written there in MFMA operand order (128 rows per 16384
// doubles; problem z of a batch at lsw + z * bt->sdinv) -- the B operand of launch_syrk_thin
hipError_t launch_trsm_strip128(const double* minv, double* B, long ldb, int m, hipStream_t stream, const Batch* bt = nullptr,
                                long sB2 = 0, double* lsw = nullptr, int lsw_blocks = 0);
// batched form: pair b uses minv + b * MINV_ELEMS and B + b * strideB (m rows each)
// bt (optional): a second batch level over problems (blockIdx.z): minv + z * bt->sdinv, B + z * sB2
hipError_t launch_trsm_strip128_batched(const double* minv, double* B, long ldb, long strideB, int m, int batch,
                                        hipStream_t stream, const Batch* bt = nullptr, long sB2 = 0, double* lsw = nullptr,
                                        int lsw_blocks = 0);

// ---------------------------------------------------------------- assemble.hip
enum { KID_RBF = 0, KID_MATERN52 = 1, KID_MATERN32 = 2, KID_EXPONENTIAL = 3, KID_RATQUAD = 4 };
constexpr int MAX_KERN = 8;  // the gradient kernels are specialised for 1..4 components and take 5..8 through one
                             // instantiation with a run-time component count (arrays in scratch: slower, same arithmetic)
struct KernSpec {
  int nkern;
  int d;
  int kid[MAX_KERN];
  int op[MAX_KERN];  // op[i] joins component i and i+1: 0 '+', 1 '*'
};
// Host-side check of a composition as the C-ABI receives it: nullptr if nkern components with ids kernel_ids[0 .. nkern)
// joined by ops[0 .. nkern - 1) are a covariance the kernels evaluate, else the reason.  ops may be null for one component.
inline const char* kern_spec_error(int nkern, const int* kernel_ids, const int* ops) {
  if (nkern <= 0 || nkern > MAX_KERN) return "1 <= nkern <= 8";
  if (!kernel_ids) return "null kernel_ids";
  for (int i = 0; i < nkern; ++i)
    if (kernel_ids[i] < KID_RBF || kernel_ids[i] > KID_RATQUAD) return "unknown kernel id";
  if (nkern > 1 && !ops) return "null ops";
  for (int i = 0; i + 1 < nkern; ++i)
    if (ops[i] != 0 && ops[i] != 1) return "ops must be 0 ('+') or 1 ('*')";
  return nullptr;
}
// the KernSpec of a composition that passed kern_spec_error (op[nkern - 1 ..] unused, set to 0)
inline KernSpec make_kern_spec(int d, int nkern, const int* kernel_ids, const int* ops) {
  KernSpec s;
  s.nkern = nkern;
  s.d = d;
  for (int i = 0; i < MAX_KERN; ++i) {
    s.kid[i] = i < nkern ? kernel_ids[i] : 0;
    s.op[i] = i + 1 < nkern ? ops[i] : 0;
  }
  return s;
}
// sym=1: lower 64x64 tiles of K(X1,X1) + noise on the diagonal, identity in the padding;
// sym=0: full K(X1,X2), zeros in the padding.  noise_form: 0 marginal, 1 conditional, 2 explicit, 3 sqrt(gv)^2 only,
// 4 jitter only (the joint conditional's pred_noise / stabilize forms, mi_gp_predict_cov).
hipError_t launch_assemble(const KernSpec& spec, const double* theta, const double* X1, int n1, const double* X2,
                           int n2, double* K, long ldk, int rows_pad, int cols_pad, int sym, int noise_form,
                           hipStream_t stream, int diag_shift = -2147483647 - 1, const double* extra_diag = nullptr,
                           const Batch* bt = nullptr);
// diag_shift (sym=0 only): local element (i, j) is on the global diagonal when i + diag_shift == j
// (rectangular blocks of a distributed covariance); the default means "no diagonal" (cross-covariance).
// info (optional): reset to 0x7f7f7f7f ("no bad pivot") by the same launch
hipError_t launch_set_yrows(double* K, long ldk, int row0, int cols_pad, const double* y, int n, hipStream_t stream,
                            int* info = nullptr, const double* theta_src = nullptr, double* theta_dst = nullptr, int ntheta = 0,
                            const Batch* bt = nullptr);
// info (optional): its first word is forwarded as out[3]
// part / sync (optional, zeroed once by the owner): 2 * LML_REDUCE_BLOCKS doubles and one unsigned PER PROBLEM -- with them the
// reduction runs on LML_REDUCE_BLOCKS workgroups (fixed slice order), without them on one
constexpr int LML_REDUCE_BLOCKS = 16;
hipError_t launch_lml_reduce(const double* L, long ld, const double* beta, int n, double* out, hipStream_t stream,
                             const int* info = nullptr, const Batch* bt = nullptr, double* part = nullptr,
                             unsigned* sync = nullptr, double seq = 0.0);

// ---------------------------------------------------------------- grad_predict.hip
hipError_t launch_set_identity_blocks(double* U, long ld, int nblocks, hipStream_t stream, const Batch* bt = nullptr);
// bt: U + z * sZ, beta + z * sK (beta is a row of the factor's matrix), alpha + z * salpha
hipError_t launch_trmv_upper(const double* U, long ld, const double* beta, int n, double* alpha, hipStream_t stream,
                             const Batch* bt = nullptr);
// out = U^T x (= L^-1 x for U = L^-T)
hipError_t launch_trmv_upper_t(const double* U, long ld, const double* x, int n, double* out, hipStream_t stream);
int grad_contract_blocks(int n);
// part: [grad_contract_blocks(n)][ntheta] scratch; grad: [ntheta] (natural parameters, C-ABI order)
hipError_t launch_grad_contract(const KernSpec& spec, const double* theta, const double* X, int n, const double* W,
                                long ldw, const double* alpha, double* part, double* grad, hipStream_t stream,
                                const Batch* bt = nullptr, unsigned* done = nullptr, double* flag = nullptr, double seq = 0.0);
// done / flag / seq (and launch_lml_reduce's seq): the evaluation's LAST kernel publishes its sequence number in pinned host
// memory -- lml_reduce in out[4], the gradient's final reduction in flag[0] (per problem of a batch: + sout) -- see wait_evaluation()
// column slab [col0, col0+cols) of the lower triangle (distributed K^-1): W points at element (row0, col0), row0 <= col0
int grad_contract_slab_blocks(int n, int col0, int cols);
hipError_t launch_grad_contract_slab(const KernSpec& spec, const double* theta, const double* X, int n, const double* W,
                                     long ldw, int row0, int col0, int cols, const double* alpha, double* part,
                                     double* grad, hipStream_t stream);
// gx: [n][d] dLML/dX from Kinv (lower triangle in W) and alpha; d <= 128
int grad_x_splits(int n, int d);  // column splits; scratch of [splits][n][d] doubles is needed when > 1
hipError_t launch_grad_x(const KernSpec& spec, const double* theta, const double* X, int n, const double* W, long ldw,
                         const double* alpha, double* gx, double* scratch, hipStream_t stream);
// dmean/dvar: [m][d] gradients of the conditional at m points; w: row p = K^-1 k(X, x*_p) (leading dimension ldw)
// the kernel keeps x* and every component's 1 / l in dynamic LDS: (nkern + 1) * d doubles, at most PREDICT_GRAD_MAX_LDS bytes
constexpr size_t PREDICT_GRAD_MAX_LDS = 61440;
hipError_t launch_predict_grad(const KernSpec& spec, const double* theta, const double* X, int n, const double* xstar,
                               int m, const double* alpha, const double* w, long ldw, double* dmean, double* dvar,
                               hipStream_t stream);
// mi_gp_logpdf's gradient (api_gp.hip has the algebra).  Linv: L22^-1 row-major 128 x 128 (identity in the padding), beta2: 128.
// Sinv = Linv^T Linv, gamma = Linv^T beta2
hipError_t launch_logpdf_sinv(const double* Linv, const double* beta2, double* Sinv, double* gamma, hipStream_t stream);
// Cw (k rows, ldw apart, Q = S^-1 P on entry) becomes C[i][j] = gamma_i (alpha[j] - sum_l gamma_l P[l][j]) + Q[i][j], j < n;
// dy (optional, k) = -gamma
hipError_t launch_logpdf_weights(double* Cw, const double* P, long ldw, const double* alpha, const double* gamma, int n, int k,
                                 double* dy, hipStream_t stream);
// dx[i][m] (k x d) over the training points (weights: row i of Cw) and the trial points (weights gamma_i gamma_j - Sinv[i][j]);
// the LDS rule of launch_predict_grad
hipError_t launch_logpdf_grad(const KernSpec& spec, const double* theta, const double* X, int n, const double* xstar, int k,
                              const double* Cw, long ldw, const double* gamma, const double* Sinv, double* dx, hipStream_t stream);
hipError_t launch_predict_reduce(const double* A, long lda, const double* beta, int n, int m, double kdiag,
                                 double noise, double* mean, double* var, hipStream_t stream);
// batched form (mi_gp_predict_batch, blockIdx.z = problem z): A + z * bt->swork, beta + z * bt->sK, theta + z * bt->stheta; kdiag
// and the noise come from problem z's own theta (the host fold of mi_gp_predict, same operations); mean / var rows z * m ..;
// a problem whose bad-pivot word info[z * bt->sinfo] is not INFO_OK gets NaN rows
constexpr int INFO_OK = 0x7f7f7f7f;  // the bad-pivot word of a positive-definite factorisation (set_yrows_kernel's reset value)
hipError_t launch_predict_reduce_batched(const KernSpec& spec, const double* theta, const double* A, long lda, const double* beta,
                                         const int* info, int n, int m, int pred_noise, double* mean, double* var,
                                         hipStream_t stream, const Batch& bt);
// equal-weight mixture over the problems whose bad-pivot word is INFO_OK, point by point, problems summed in index order:
// mix_mean = sum mean_p / K', mix_var = sum var_p / K' + sum (mean_p - mix_mean)^2 / K' (NaN where K' = 0); the sums run
// relative to the first member's moments (draws that all agree return its moments exactly)
hipError_t launch_mixture_moments(const double* mean, const double* var, int m, int k, const int* info, int sinfo,
                                  double* mix_mean, double* mix_var, hipStream_t stream);

// ---------------------------------------------------------------- append_f64.hip (mi_gp_append)
// S block: 256 x 128 doubles (ld 128): S = K22 + noise (identity-padded) in rows 0 .. 127, r / beta2 in row 128.
// S -= sum of nparts 128 x 128 partial products (parts, 16384 doubles apart); r = y2 - L21 beta1 (k entries, zeros beyond)
hipError_t launch_append_schur(double* S, const double* parts, int nparts, const double* L21, long ldw, const double* beta1, int np,
                               const double* y2, int k, hipStream_t stream);
// stats[0] = sum log L22_ii, stats[1] = |beta2|^2 (k entries), stats[2] = (double)*info
hipError_t launch_append_stats(const double* S, int k, const int* info, double* stats, hipStream_t stream);
// beta row moved to / extended at row np_new, then rows [n, n + k) of K = [L21, L22, 0] (and identity padding rows of a new tile)
hipError_t launch_append_commit(double* K, long ld, int n, int k, int np_old, int np_new, const double* L21, long ldw, const double* S,
                                hipStream_t stream);
// inverses of ntiles (1 or 2) consecutive lower-triangular 128 x 128 tiles T + t * sT into out + t * sout, rows [i0_first, 128) of
// the first (the rows above it are resident) and every row of a second; plain: row-major instead of minv_index order
hipError_t launch_tile_inverse_rows(const double* T, long ldt, long sT, double* out, long sout, int i0_first, int ntiles, int plain,
                                    hipStream_t stream);
// U = L^-T extended in place by the appended columns: U12 from Qt (k rows, row p = -(L22^-1 L21 U11^T) row p), U22 = Linv22^T
hipError_t launch_append_u(double* Z, long ld, int n, int k, int np_old, int np_new, const double* Qt, long ldw, const double* Linv22,
                           hipStream_t stream);

// ---------------------------------------------------------------- joint_f64.hip (mi_gp_predict_cov / mi_gp_sample_cov)
// Z[r * ldz + i] = normal j = r m + i (r < s, i < m) of the Philox4x64-10 + Box-Muller stream of include/mi_gp.h; the padding
// of Z is not written
hipError_t launch_philox_normals(double* Z, long ldz, int m, int s, unsigned long long seed, unsigned long long offset,
                                 hipStream_t stream);
// C (mp x mp, lower): + shift on the m leading diagonal entries, identity in the lower triangle of rows m .. mp - 1
hipError_t launch_cov_prepare(double* C, long ldc, int m, int mp, double shift, hipStream_t stream);
// zeros in the strict upper triangle of the ntiles diagonal 128 x 128 tiles of L
hipError_t launch_zero_diag_upper(double* L, long ld, int ntiles, hipStream_t stream);
// draws[r * ldd + i] = mean[i] + D[r * ldp + i] for r < s, i < m
hipError_t launch_draw_epilogue(const double* D, long ldp, const double* mean, int m, int s, double* draws, long ldd,
                                hipStream_t stream);

// ---------------------------------------------------------------- kfold_f64.hip (mi_gp_kfold)
// idx / ptr: the folds in CSR form on the device; a pass handles the folds f0 .. f0 + nf - 1.  blocks / minv: nf blocks of
// MINV_ELEMS doubles, vecs: nf x 256 (alpha_I, then y_I), info: one bad-pivot word per fold of the CALL (indexed f0 + f).
// blocks[f] = K^-1_II from the LOWER triangle of W (identity in the padding), vecs and the INFO_OK reset of the words
hipError_t launch_kfold_gather(const double* W, long ld, const double* alpha, const double* y, const int* idx, const int* ptr, int f0,
                               int nf, double* blocks, double* vecs, int* info, hipStream_t stream);
// behind the leaf (blocks = chol(K^-1_II), minv its inverse): logp[f0 + f], mean / var (optional, both or neither) at the fold's
// positions of idx; -inf and NaN for a fold whose word is not INFO_OK
hipError_t launch_kfold_moments(const double* blocks, const double* minv, const double* vecs, const int* ptr, const int* info, int f0,
                                int nf, double* logp, double* mean, double* var, hipStream_t stream);
// every fold one point: the closed form, info[f] = 0 or 1
hipError_t launch_kfold_loo(const double* W, long ld, const double* alpha, const double* y, const int* idx, int nfolds, double* logp,
                            double* mean, double* var, int* info, hipStream_t stream);
// The density of one fold, shared by kfold_moments_kernel and cv_fold_kernel (cvobj_f64.hip) so that both return the same bits:
// a workgroup of 128 threads, thread j = position j of a fold of s points, C = chol(K^-1_II) row-major, M = C^-1 in minv_index
// order, al = alpha_I.  tv / s1 / s2: 128 doubles of LDS each.  Returns logp on every thread; afterwards tv holds t = M alpha_I
// (zeros from s on) and s2[0] = |t|^2.  Every sum runs in a fixed order.
__device__ __forceinline__ double kfold_fold_logp(const double* __restrict__ C, const double* __restrict__ M,
                                                  const double* __restrict__ al, int j, int s, double* tv, double* s1, double* s2) {
  double t = 0.0;
  if (j < s)
    for (int c = 0; c <= j; ++c) t = __builtin_fma(M[minv_index(j, c)], al[c], t);
  tv[j] = t;
  s1[j] = j < s ? log(C[j * 129]) : 0.0;
  s2[j] = t * t;
  __syncthreads();
  for (int w = 64; w > 0; w >>= 1) {
    if (j < w) { s1[j] += s1[j + w]; s2[j] += s2[j + w]; }
    __syncthreads();
  }
  return -0.5 * s2[0] + s1[0] - 0.5 * (double)s * LOG_2PI;
}

// ---------------------------------------------------------------- cvobj_f64.hip (option 49: the k-fold objective, api_loo.hip)
// behind the leaf of a pass (launch_kfold_gather's layout; ptr = the contiguous folds): per fold t = M alpha_I, tau = |t|^2,
// e_I = M^T t, q_I = t / sqrt(1 + tau) and the rows of R = M^T + e t^T / (1 + sqrt(1 + tau)) at the fold's points -- e[i], q[i],
// R[i * 128 + 0 .. 127] (zeros from the fold's size on) -- and flogp[f0 + f], mi_gp_kfold's logp of the fold.  A fold whose word
// is not INFO_OK: -inf and zeros
hipError_t launch_cv_fold(const double* blocks, const double* minv, const double* vecs, const int* ptr, const int* info, int f0,
                          int nf, double* flogp, double* e, double* q, double* R, hipStream_t stream);
// scal[0] = sum_f flogp[f] in a fixed order, scal[1] = the smallest ptr[f] + info[f] over the folds whose word is not INFO_OK
// (the 1-based index of the point at the bad pivot; 0: none)
hipError_t launch_cv_reduce(const double* flogp, const int* ptr, const int* info, int nfolds, double* scal, hipStream_t stream);
// B[:, I_f] = Pfull[:, I_f] R_f for the folds I_f = [f b, min((f + 1) b, n)): Pfull[i][j] = W[max(i, j)][min(i, j)] (the LOWER
// triangle of W alone), R as launch_cv_fold left it; the full np x np matrix, zeros in the rows and columns from n on
hipError_t launch_cv_mirror_multiply(const double* W, long ldw, const double* R, int b, int n, int np, double* B, long ldb,
                                     hipStream_t stream);

// ---------------------------------------------------------------- loo_f64.hip (option 48: the leave-one-out objective, api_loo.hip)
// From P = K^-1 (LOWER triangle of W) and alpha: logp[i] (mi_gp_kfold's singleton density), e[i] = alpha_i / p_i,
// s[i] = sqrt((1 + alpha_i^2 / p_i) / p_i), q[i] = e[i] / s[i] for i < n; scal[0] = sum logp in a fixed order, scal[1] = 1-based index
// of the first p_i that is not a positive finite number (0: none; that point gets logp = -inf and zero weights)
hipError_t launch_loo_weights(const double* W, long ld, const double* alpha, int n, double* e, double* s, double* q, double* logp,
                              double* scal, hipStream_t stream);
// B[i][j] = P[max(i, j)][min(i, j)] * s[j] for i, j < n, zeros up to np: the full np x np matrix (np a multiple of 128)
hipError_t launch_loo_scale_mirror(const double* W, long ldw, const double* s, int n, int np, double* B, long ldb,
                                   hipStream_t stream);
// w[i] = sum_{k < n} B[i][k] q[k], i < n
hipError_t launch_loo_gemv(const double* B, long ld, const double* q, int n, double* w, hipStream_t stream);
// G[i][j] = -(alpha_i w_j + w_i alpha_j) over the 128 x 128 tiles on and below the block diagonal (whole tiles), zeros up to np
hipError_t launch_loo_rank2_init(const double* alpha, const double* w, int n, int np, double* G, long ld, hipStream_t stream);

// ---------------------------------------------------------------- trend_f64.hip (option 50: the GP trend, api_trend.hip)
// The basis h(x) = [1] (p = 1) or [1, x_1 .. x_d] (p = 1 + d <= 128) as H^T: HT[c * ldg + i] = h_c(x_i) for c < p, i < n, zeros up to
// row 127 and column np - 1
hipError_t launch_trend_basis(const double* X, int n, int d, int p, int np, double* HT, long ldg, hipStream_t stream);
// V (np x 128 row-major, all of it written) = Pfull H: Pfull[i][j] = W[max(i, j)][min(i, j)] for i, j < n (the LOWER triangle of W
// alone) and zero beyond, H^T as launch_trend_basis left it
// parts: np x 128 doubles of scratch (the k range runs in slices whose partial products are added in index order)
hipError_t launch_trend_symm(const double* W, long ldw, const double* HT, long ldg, int n, int np, int p, double* V, double* parts,
                             hipStream_t stream);
// A (128 x 128 row-major) = sum of nparts partial products (MINV_ELEMS apart, in index order) over the leading p x p block, the
// identity beyond it
hipError_t launch_trend_gram_sum(const double* parts, int nparts, int p, double* A, hipStream_t stream);
// u[c] = sum_{i < n} M[c * ld + i] x[i], c < 128
hipError_t launch_trend_rowdot(const double* M, long ld, const double* x, int n, double* u, hipStream_t stream);
// behind the leaf on A (C = chol(A) in place, Cinv its row-major inverse): cvec = C^-1 u, beta = C^-T cvec (128 each, zeros from p
// on), scal = {1/2 |cvec|^2, sum_{j < p} log C_jj, (double)*info}
hipError_t launch_trend_solve(const double* C, const double* Cinv, const double* u, const int* info, int p, double* cvec, double* beta,
                              double* scal, hipStream_t stream);
// out[i] = base[i] - sum_{a < p} M[i * si + a * sa] beta[a] for i < n, zeros up to np
hipError_t launch_trend_project(const double* base, const double* M, long si, long sa, const double* beta, int p, int n, int np,
                                double* out, hipStream_t stream);
// mi_gp_predict's reduction under a trend over the m rows a* of A (lda apart; GT = (L^-1 H)^T, bt = b - G beta):
// mean = a* . bt + h(x*)^T beta, var = kdiag - |a*|^2 + |Cinv (h(x*) - G^T a*)|^2 + noise; each output is written once
hipError_t launch_trend_predict_reduce(const double* A, long lda, const double* Xnew, int d, int p, const double* GT, long ldg,
                                       const double* bt, const double* beta, const double* Cinv, int n, int m, double kdiag,
                                       double noise, double* mean, double* var, hipStream_t stream);

// ---------------------------------------------------------------- multi_f64.hip (option 51: several outputs, api_multi.hip)
// Y^T in launch_trend_basis's layout: YT[o * ldg + i] = y[o * ldy + i] for o < q, i < n, zeros up to row 127 and column np - 1
hipError_t launch_multi_stage(const double* y, long ldy, int q, int n, int np, double* YT, long ldg, hipStream_t stream);
// quad[o] = sum_{i < n} YT[o * ldg + i] V[i * 128 + o] for o < q, zeros up to 127; every sum in a fixed order
hipError_t launch_multi_quad(const double* YT, long ldg, const double* V, int q, int n, double* quad, hipStream_t stream);
// mi_gp_predict's reduction under q outputs, ONE pass over the m rows a* of A (lda apart; BT = (L^-1 Y)^T, 128 rows ldg apart):
// mean[o * m + i] = a*_i . b_o for o < q, var[i] = kdiag - |a*_i|^2 + noise; each output is written once.  svar (option 52 = 1,
// else nullptr): q scales s_o, and var[o * m + i] = (kdiag - |a*_i|^2 + noise) * s_o for o < q instead
hipError_t launch_multi_predict(const double* A, long lda, const double* BT, long ldg, int q, int n, int m, double kdiag, double noise,
                                const double* svar, double* mean, double* var, hipStream_t stream);
// option 52 = 1: scal[0] = sum_{j < q} log C[j * 129] of the factored block of S = Y^T K^-1 Y in index order, scal[1] = its bad-pivot
// word
hipError_t launch_multi_cov_scal(const double* C, const int* info, int q, double* scal, hipStream_t stream);
// option 52 = 1: s[o] = sum_{i < n} BT[o * ldg + i]^2 / dof for o < q, zeros up to 127; every sum in a fixed order
hipError_t launch_multi_rowsq(const double* BT, long ldg, int q, int n, double dof, double* s, hipStream_t stream);

// ---------------------------------------------------------------- sweep_f64.hip (option 53: the mean sweep, api_sweep.hip)
constexpr int SWEEP_MAX_D = 128;  // input dimensions the sweep's register windows cover
constexpr int SWEEP_PARTS = 16;   // parts of the training range, [y q, min((y + 1) q, n)) with q = ceil(n / 16): a rule of n alone
int sweep_stride(int d);                    // padded row length of the staged training points
// doubles of scratch for up to cap training points: the staged points, 1 / l and 2 / l^2, the partial sums of one pass of query
// points and (d > 32) the pass's query points
size_t sweep_scratch_len(int cap, int d);
// mean[p] = sum_j k(x*_p, x_j) alpha_j and dmean[p][.] = its gradient w.r.t. x*_p for p < m, each optional (not both null): one
// thread per point and part, j in index order, the parts' sums added in part order; d <= SWEEP_MAX_D.  scratch is staged by the
// same call; the query points are walked in passes of 16384 (d > 32: 4096)
hipError_t launch_mean_sweep(const KernSpec& spec, const double* theta, const double* X, int n, const double* xstar, int m,
                             const double* alpha, double* scratch, double* mean, double* dmean, hipStream_t stream);

// ---------------------------------------------------------------- paths_f64.hip (option 54: the path sweep, api_paths.hip)
constexpr int PATH_MAX_D = 32;      // input dimensions the path sweep's register windows cover (4, 16, 32; no wide form)
constexpr int PATH_MAX_S = 128;     // paths of one block; the row length of the staged weights
constexpr int PATH_PARTS_N = 16;    // parts of the training range, [y q, min((y + 1) q, n)) with q = ceil(n / 16): a rule of n alone
constexpr int PATH_PARTS_F = 16;    // parts of the feature range, [y F / 16, (y + 1) F / 16): a rule of F alone (F is a multiple of 16)
constexpr int PATH_CHUNK = 4096;    // query points of one pass of 128 columns (a pass of fewer columns: up to 8 times as many)
constexpr int PATH_TILE_VALUE = 16; // paths a thread carries without the gradient
int path_window(int d);             // the register window that runs for d dimensions: 4, 16 or 32
int path_tile(int d, bool grad);    // T, the paths a thread carries: PATH_TILE_VALUE, with the gradient 8 / 2 / 1 for the window 4 / 16 / 32
// The handle-owned scratch for up to cap training points and F features (ldr = cap rounded up to 128, the row stride of R1 / R2)
struct PathScratch {
  double *Xp, *il, *il2;  // the training points, 1 / l and 2 / l^2 padded with zeros to the window (sweep_f64.hip's staging)
  double* Om;             // [F][window] the frequencies, zeros from d on
  double *Wp, *Vp;        // [F][128], [cap][128] the weights; columns S .. S rounded up to 16 hold zeros, the rest is never read
  double* part;           // the partial sums of one pass of PATH_CHUNK points and one group of path tiles
  double *R1, *R2;        // [128][ldr] the conditioning's staged blocks R^T and R^T U
  long ldr;
};
size_t path_scratch_len(int cap, int d, int F);
PathScratch path_scratch(double* base, int cap, int d, int F);
// stages X, 1 / l, 2 / l^2, Omega and W (V: launch_path_stage_v, behind the conditioning); W and V rows are ldw apart, S columns used
hipError_t launch_path_stage(const KernSpec& spec, const double* theta, const double* X, int n, const double* Om, const double* W, long ldw,
                             int F, int S, const PathScratch& t, hipStream_t stream);
hipError_t launch_path_stage_v(const double* V, long ldw, int n, int S, const PathScratch& t, hipStream_t stream);
// mean[s * ldo + p] = sum_i W[i,s] cos(om_i . x*_p + b_i) (+ sum_j k(x*_p, x_j) V[j,s] unless features_only) for s < S, p < m, and
// dmean[(s * ldo + p) * d + k] its derivative; each optional (not both null).  One thread per point, part and path tile; a
// point's sums run in index order, the parts' sums are added in part order.  bph: the F phases.
hipError_t launch_path_sweep(const KernSpec& spec, const double* theta, int n, int F, int S, const double* bph, const PathScratch& t,
                             const double* xstar, int m, long ldo, double* mean, double* dmean, bool features_only, hipStream_t stream);
// R1[s * ldr + j] = y[j] - R1[s * ldr + j] - V[j * ldw + s] for s < S, j < n; zeros in the rows from S on and the columns from n on
hipError_t launch_path_residual(const double* y, const double* V, long ldw, int n, int S, const PathScratch& t, hipStream_t stream);
// V[j * ldw + s] = R1[s * ldr + j] for s < S, j < n
hipError_t launch_path_scatter(double* V, long ldw, int n, int S, const PathScratch& t, hipStream_t stream);

// ---------------------------------------------------------------- design_f64.hip (option 56: the design call, api_design.hip)
constexpr int DESIGN_MAX_B = 128;  // points one call selects at most
// The handle-owned scratch for Mc candidates and b steps (mcp = Mc rounded up to 128, the row stride of hist)
struct DesignScratch {
  double *v, *rowsq;      // [mcp] v(c) = var_latent(c) + noise, the rows' sums of squares of G
  double* mean;           // [mcp] the row reduction's means (written, never read)
  double* hist;           // [b][mcp] the candidate columns g_s = cov_s(C, c*_s) of the steps so far, the current one included
  double* vs;             // [128] v* of the steps so far
  int* alive;             // [mcp] 1 until a candidate is chosen
  int* piv;               // the step's pivot, -1 once the selection has stopped
  long mcp;
};
size_t design_scratch_len(int Mc, int b);
DesignScratch design_scratch(double* base, int Mc, int b);
// rowsq[c] = sum_{r < Mr} G[c][r]^2 for c < Mc, each sum in a fixed order
hipError_t launch_design_rowsq(const double* G, long ldc, int Mc, int Mr, double* rowsq, hipStream_t stream);
// Step `step` of the greedy loop, three launches: the pick (score, arg-max with ties to the lowest index, the records in out), the
// candidate column g = cov_t(C, c*) from the rows A (ldw apart, n entries each) and the fused pass over G (Mc x Mr, ldc apart;
// Mr = 0: the plain maximum-variance criterion, G is not touched).  noise = v - var_latent.  out: [Mc] round-0 gains, [b] chosen
// indices as doubles (-1 beyond the count), [b] their gains, the count; step 0 initialises it
hipError_t launch_design_step(const KernSpec& spec, const double* theta, const double* Xc, int Mc, int Mr, int b, int step,
                              const double* A, long ldw, int n, double* G, long ldc, double noise, const DesignScratch& t, double* out,
                              hipStream_t stream);

// ---------------------------------------------------------------- sparse_f64.hip (the sparse inducing-point bound, api_sparse.hip)
int sparse_contract_blocks(int cnt, int m);  // 64 x 64 tiles of the cnt x m cross-covariance
// acc[ntheta] (first: =, else +=) sum_{i < cnt, u < m} (T[i][u] + y[i] tv[u]) dK(x_i, z_u)/dtheta (natural parameters, C-ABI
// order; the gv and jitter slots receive 0).  part: [sparse_contract_blocks(cnt, m)][ntheta] scratch
hipError_t launch_sparse_contract(const KernSpec& spec, const double* theta, const double* X, int cnt, const double* Z, int m,
                                  const double* T, long ldt, const double* y, const double* tv, double* part, double* acc, int first,
                                  hipStream_t stream);
// (sparse_zgrad_f64.hip) Slabs of one chunk's dF/dZ pass: min(64-row blocks of the chunk, cap, ceil(1024 / 64-column blocks of m)), lowered until the
// slab scratch is at most 64 MB -- a function of (cnt, m, d, cap) alone -- and the doubles of scratch they take
int sparse_zgrad_slabs(int cnt, int m, int d, int cap);
long sparse_zgrad_scratch(int cnt, int m, int d, int cap);
// gz[m x d] (first: =, else +=) sum_{i < cnt} (T[i][u] + y[i] tv[u]) dK(x_i, z_u)/dz_u: workgroup (ub, sl) of the grid
// (ceil(m / 64), slabs) walks the data blocks sl, sl + slabs, ..., and the slabs are added in slab order.  scratch:
// sparse_zgrad_scratch(cnt, m, d, cap) doubles
hipError_t launch_sparse_zgrad(const KernSpec& spec, const double* theta, const double* X, int cnt, const double* Z, int m,
                               const double* T, long ldt, const double* y, const double* tv, int cap, double* scratch, double* gz,
                               int first, hipStream_t stream);
// gz[e] (first: =, else +=) sum_{k < nslab} part[k * slab + e] for e < len, in slab order
hipError_t launch_sparse_zgrad_add(const double* part, int nslab, long slab, long len, double* gz, int first, hipStream_t stream);
// (sparse_xgrad_f64.hip) Slabs of one chunk's dF/dX pass: min(64-column blocks of m, cap, ceil(1024 / 64-row blocks of the chunk)), lowered until the
// slab scratch is at most 64 MB -- a function of (cnt, m, d, cap) alone -- and the doubles of scratch they take
int sparse_xgrad_slabs(int cnt, int m, int d, int cap);
long sparse_xgrad_scratch(int cnt, int m, int d, int cap);
// gx[cnt x d] = sum_{u < m} (T[i][u] + y[i] tv[u]) dK(x_i, z_u)/dx_i: workgroup (rb, sl) of the grid (ceil(cnt / 64), slabs) walks
// the blocks of Z sl, sl + slabs, ..., and the slabs' sum is written in slab order.  scratch: sparse_xgrad_scratch(cnt, m, d, cap)
// doubles
hipError_t launch_sparse_xgrad(const KernSpec& spec, const double* theta, const double* X, int cnt, const double* Z, int m,
                               const double* T, long ldt, const double* y, const double* tv, int cap, double* scratch, double* gx,
                               hipStream_t stream);
// gy[i] = -y[i] / s + (sum_{u < m} At[i][u] ahat[u]) / s for i < cnt (rows ld apart), every row's sum in a fixed order
hipError_t launch_sparse_ygrad(const double* At, long ld, int m, const double* ahat, const double* y, int cnt, double sv, double* gy,
                               hipStream_t stream);
// v[u] (first: =, else +=) sum_{i < cnt} At[i][u] y[i] for u < mp (a multiple of 64), yy[0] likewise sum y_i^2
hipError_t launch_sparse_accum_vy(const double* At, long ld, int mp, const double* y, int cnt, double* v, double* yy, int first,
                                  hipStream_t stream);
// B = I + Psi / s over mp x mp (leading dimension mp)
hipError_t launch_sparse_make_b(const double* Psi, double* B, int mp, double s, hipStream_t stream);
// out[i] = in[i] / s, i < n
hipError_t launch_sparse_scale(const double* in, double* out, int n, double s, hipStream_t stream);
// out[0..4] = sum log LB_ii, tr Psi, |c|^2, |a^|^2, tr B^-1 over the leading m entries (ahat / Binv optional: 0 without)
hipError_t launch_sparse_scalars(const double* LB, const double* Psi, long ld, const double* cvec, const double* ahat,
                                 const double* Binv, int m, double* out, hipStream_t stream);
// H = I - B^-1 - a^ a^^T, G0 = Psi / s - H over mp x mp (Psi: lower triangle; ahat: mp entries, zeros from m on)
hipError_t launch_sparse_hg(const double* Psi, const double* Binv, const double* ahat, int mp, double s, double* H, double* G0,
                            hipStream_t stream);
// mean[i] = Bq_i . c, var[i] = kdiag - |A_i|^2 + |Bq_i|^2 + noise for i < mq (rows ld apart, m entries each)
hipError_t launch_sparse_predict_reduce(const double* A, const double* Bq, long ld, const double* cvec, int m, int mq, double kdiag,
                                        double noise, double* mean, double* var, hipStream_t stream);

// ---------------------------------------------------------------- deriv_f64.hip (the joint GP over f and grad f, api_deriv.hip)
constexpr int DERIV_MAX_D = 32;  // input dimensions the two kernels stage in one LDS block
// The covariance of [f ; d_1 f ; .. ; d_d f] at two point sets (include/mi_gp_deriv.h has the blocks): q1 / q2 are the component
// counts of the rows / columns, 1 (values only) or 1 + d; row a = c n1 + i is component c at point i of X1 (n1 x d), N1 = n1 q1 rows
// and N2 = n2 q2 columns.  kid: KID_RBF or KID_MATERN52; theta = [l(d), kv, alpha, gv, jitter]; d <= DERIV_MAX_D.
// launch_assemble's tiling and padding contract: sym = 1 the lower 64x64 tiles of the N1 x N1 matrix with the diagonal -- the
// value rows' noise_form terms, the jitter alone on the derivative rows, extra_diag[N1] (optional) on both -- and the identity in
// the padding; sym = 0 the full rectangle, zeros in the padding, no diagonal.  rows_pad / cols_pad: multiples of 64
hipError_t launch_assemble_deriv(int kid, int d, const double* theta, const double* X1, int n1, int q1, const double* X2, int n2, int q2,
                                 double* K, long ldk, int rows_pad, int cols_pad, int sym, int noise_form, hipStream_t stream,
                                 const double* extra_diag = nullptr);
// launch_grad_contract for that covariance over the N = n (1 + d) observations: grad[d + 4] = 1/2 sum_ab (alpha_a alpha_b - W_ab)
// dK~_ab/dtheta from the LOWER triangle of W; part: [grad_contract_blocks(N)][d + 4] scratch; done / flag / seq as there.  No
// atomics on the sums: per-tile partials, added in tile order
hipError_t launch_grad_contract_deriv(int kid, int d, const double* theta, const double* X, int n, const double* W, long ldw,
                                      const double* alpha, double* part, double* grad, hipStream_t stream, unsigned* done = nullptr,
                                      double* flag = nullptr, double seq = 0.0);

// ---------------------------------------------------------------- api_blocks.hip
// X L^T = B in place for the tile columns [c0, c0 + w) of a lower factor L (the body of mi_gp_trsm_block)
hipError_t trsm_blocks(const double* L, long ldl, const double* dinv, double* B, long ldb, int m, int c0, int w, hipStream_t st);
// text behind mi_gp_last_global_error() (calls that have no handle to carry it: mi_gp_create, the block-level entries)
void set_global_error(const char* text);
// leaf + strip + in-panel updates of the w_tiles leading tile columns of a (row_tiles x w_tiles)-tile lower trapezoid
// (the body of mi_gp_chol_panel)
hipError_t chol_panel_blocks(double* A, long lda, int row_tiles, int w_tiles, double* dinv, int* info, int col_base,
                             hipStream_t st);
int ensure_kernel_attributes();  // per-device dynamic-LDS limits of the GEMM / leaf kernels; 0 or a C-ABI error code

}  // namespace migp
