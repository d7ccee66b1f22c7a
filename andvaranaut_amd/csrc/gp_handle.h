// Private to the handle-level C-ABI: the GP handle, what an evaluation is made of, and what api_gp.hip and the
// factorisation scheduler (gp_sched.hip) share.
#pragma once
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>
#include "migp_kernels.h"
#include "../../include/mi_gp.h"

using namespace migp;

constexpr int SIG_SLOTS = 1024;  // cross-stream edges of one evaluation (a 16384-point factorisation has ~60)

// Per-problem scratch of an evaluation, for k problems (the single evaluation's k = 1, a batch's k = its count); problem p's
// part of an array starts p per-problem sizes in (scratch_strides()).
struct Scratch {
  int k = 0;                    // problems it is sized for (0: none)
  double* theta_dev = nullptr;  // [k][ntheta]
  double* dinv_dev = nullptr;   // [k][ntc + 4][MINV_ELEMS] explicit inverses of the diagonal blocks of L (leaf output, strip operand)
  double* alpha_dev = nullptr;  // [k][np] K^-1 y
  double* part_dev = nullptr;   // [k][grad_contract_blocks(n)][ntheta]
  int* info_dev = nullptr;      // [k][4] bad-pivot words
  double* lr_part_dev = nullptr;    // [k][2 * LML_REDUCE_BLOCKS] slice sums of lml_reduce_kernel
  unsigned* lr_sync_dev = nullptr;  // [2k]: [0, k) lml_reduce's tickets, [k, 2k) grad_final's (zero between evaluations)
  double* grad_host = nullptr;  // pinned [k][ntheta]
  double* out_host = nullptr;   // pinned [k][16] scalar records
  double* theta_host = nullptr; // pinned [k][ntheta]
};

// A device block of a mode's scratch, sized by point capacity and by what the mode's call needs.  Its owner asks for it before
// use (ensure_block); mi_gp_reserve drops it, or moves what must outlive the call (block_keeps_state).
struct CapBlock {
  double* p = nullptr;
  int cap = 0;     // points p is sized for
  size_t len = 0;  // doubles p holds
};
// The handle's mode blocks (mi_gp_handle::blocks).  A new mode adds its id here, asks for its block with ensure_block and
// declares its option in mode_options (api_gp.hip); release_handle and mi_gp_reserve go over all of them.
enum BlockId {
  BLK_LOO,     // [6][padded cap] e, s, q, w, the zero vector and the per-point logp, then [8] scalars (api_loo.hip)
  BLK_CV,      // the fold pass of the objective under option 49 > 1 (cv_fold_pass(), api_loo.hip)
  BLK_TREND,   // TrendScratch (api_trend.hip)
  BLK_MULTI,   // MultiScratch (api_multi.hip); laid out for option 52's value: a change of it drops the block
  BLK_SWEEP,   // the training points staged for the kernel and the partial sums of one pass (sweep_f64.hip: sweep_scratch_len)
  BLK_PATH,    // the points, frequencies and weights staged for the kernel, the partial sums of one pass and the conditioning's
               // two 128-row blocks (paths_f64.hip: path_scratch_len)
  BLK_DESIGN,  // design_f64.hip: design_scratch_len
  BLK_COUNT
};
// true: the block holds the conditional's part of a mode behind mi_gp_factor, and mi_gp_reserve moves it (trend_reserve /
// multi_reserve).  Every other block holds nothing between calls: mi_gp_reserve drops it and its next use allocates it again
constexpr bool block_keeps_state(int id) { return id == BLK_TREND || id == BLK_MULTI; }

struct mi_gp_handle {
  mi_gp_config cfg;
  KernSpec spec;
  int n, np, ntc;       // points, padded points, 128-column tiles
  int ntheta;
  int device;
  hipStream_t stream;    // trailing updates, assembly, reductions
  hipStream_t pstream;   // look-ahead panel factorisation (higher priority)
  std::vector<hipEvent_t> ev_pool;  // one event per cross-stream hand-off of an evaluation (never re-recorded inside one
                                    // evaluation: a captured DAG then holds one node pair per hand-off); Sched::ev_next draws from it
  // Cross-stream edges as stream memory operations (round 4, option 26): `from` writes the evaluation's epoch into a slot of
  // sig_dev behind its work (hipStreamWriteValue32), `to` waits for slot >= epoch (hipStreamWaitValue32).  Measured on
  // MI355X (ping-pong of short kernels over two streams): +4-5 us per edge against +11-12 us with hipEventRecord +
  // hipStreamWaitEvent.  One slot per edge of an evaluation, never re-used inside it; the epoch grows by one per
  // factorisation, so a slot's old value never satisfies a new wait.
  unsigned* sig_dev;                // [SIG_SLOTS]
  unsigned sig_epoch;
  bool smo_supported;               // hipDeviceAttributeCanUseStreamWaitValue
  int poll_limit_log2;              // option 27: an in-kernel poll gives up after 2^this sleeps (default 22: seconds)
  int test_drop_signal;             // option 28 (tests): the next evaluation leaves one main-stream signal unwritten
  bool demoted;                     // a poll ran into its limit (or mi_gp_create's probe found kernel dispatch serialised): the edges
                                    // are events from then on (use_smo = 0) -- mi_gp_get_option(40)
  int u_early_max_s;                // option 30: block-doubling levels of U = L^-T (node sizes up to this many tiles) that start inside the
                                    // factorisation's chain-bound tail on the main stream (gradient evaluations; 0: none)
  int u_early_cols;                 // option 31: ... from this many trailing tile columns on, and at most this many new columns per step
  int thin_max_wg;                  // option 32: in-panel updates of at most this many 16-row x 128-column slices (k = 128, at most
                                    // THIN_MAX_COLS tile columns) run on the thin kernel (thin_f64.hip); 0: never
  int start_on_panel;               // option 45: see enqueue_factor (default 1; scheduling only)
  int spin_us;                      // option 47: wait_evaluation() spins on the evaluation's sequence word for up to this many us (0: never)
  double eval_seq;                  // sequence number of the evaluation in flight (published by its last kernel)
  int spin_backoff;                 // evaluations left that go straight to hipStreamSynchronize (the last spin ran into its budget)
  unsigned spin_hits;               // spin waits that saw the word (every 256th synchronises the stream all the same)
  int rl_group;                     // option 38: column mode of a BATCH applies the main stream's k = 128 updates to the far columns in
                                    // k-segmented launches of this many columns (same bits, the trailing matrices read and written once per group)
  int rl_cols;                      // option 37: the last rl_cols tile columns are factored COLUMN BY COLUMN (cholesky(): column mode); 0: never
  int rl_whole;                     // option 46: problems of up to this many tile columns run in column mode from the start (whole_columns())
  int ext_rows;                     // option 35: a super-panel with at most this many tile rows below it also applies its updates to
                                    // the NEXT super-panel's first tile column, level by level (chol_panel's nx); 0: never
  int use_smo;                      // option 26: 0 events, 1 runtime stream memory operations, 2 (default) the panel stream's
                                    // halves folded into one-lane launches of the library / the end of a leaf
  // tuning options (mi_gp_set_option), all per handle
  int tail_small;   // option 9: 128x128-tile launches finish their last partial round on 64x64 tiles (default 1)
  int chain_prio;   // s_setprio(3) in the GEMM launches of the panel stream (option 16; the leaf and strip kernels always raise it)
  int lookahead;    // 0 never, 1 by size (default: from LOOKAHEAD_MIN_TILES tile columns on), 2 always
  int lowocc_thr;   // trailing sizes (tile columns) at or below which bulk updates run one workgroup per CU
  int w_thr[3];     // trailing sizes (tile columns) above which the super-panel is 16 / 8 / 4 tiles wide
  int small_below;  // GEMM launches with fewer 128x128 tiles than this run on 64x64 tiles
  int band_rows;    // band height of the band-column-major tile order of uniform-k trapezoid launches
  int split_tiles;  // option 18: tiles of a bulk update that run one workgroup per CU beside the chain; the rest two per CU (0: no split)
  int split_min_rest;  // option 19: ... only when at least this many tiles remain for the second part
  int single_below;    // option 21: trailing tile columns at or below which a two-stream factorisation continues on one stream (0: never)
  int merge_min_tiles; // option 20: trailing sizes (tile columns) from which the next super-panel's update rides at the head of the
                       // trailing update's enumeration instead of in launches of its own (0: never)
  mi_gp_buffers buf;
  bool have_data;
  Scratch one;          // the single evaluation's scratch (k = 1, sized for cap points)
  double* gxs_dev;      // [grad_x_splits][n][d] partial dLML/dX (allocated on first mi_gp_grad_x)
  // profiling
  int prof_level;
  hipEvent_t ev[8];
  std::vector<hipEvent_t> gemm_ev;  // pairs
  std::vector<char> gemm_ev_big;    // per pair: 1 if the 128x128-tile kernel ran
  std::vector<double> gemm_ev_flops;
  size_t gemm_ev_used;
  double gemm_flops_acc;
  double t_assemble_ms, t_chol_ms, t_reduce_ms, t_gemm_ms, t_total_ms, gemm_flops, n_gemm;
  double t_trtri_ms, t_lauum_ms, t_contract_ms;
  double t_enqueue_ms;  // host time of enqueueing the last single evaluation (always measured: two clock reads)
  double t_gemm_big_ms, gemm_big_flops, n_gemm_big;  // the 128x128-tile kernel only
  double t_logpdf_ms[3];  // the last mi_gp_logpdf: conditional block, weights (L22^-1, S^-1, P, Q, C), gradient kernel
  // batched evaluation (mi_gp_set_batch / mi_gp_lml_batch / mi_gp_lml_grad_batch): the caller's K / Z / W and the batch's
  // scratch (k = bbuf.count or more, sized for n points); batch_eval() hands both to the enqueue code
  mi_gp_batch_buffers bbuf;
  Scratch batch;
  int b_cond_k;            // problems whose conditional factors (L_p, beta_p, leaf inverses) the last batch call left in the batch
                           // buffers: mi_gp_factor_batch sets it, every other batch call, mi_gp_set_batch / _set_data / _set_diag,
                           // mi_gp_append and a single evaluation into the batch's K (factor_internal) clear it (0)
  bool factored;
  bool have_u;             // Z_dev holds U = L^-T and alpha_dev = K^-1 y of the last mi_gp_factor (mi_gp_predict_grad)
  bool have_kinv;          // W_dev holds K^-1 (lower) and alpha_dev = K^-1 y of the last mi_gp_lml_grad
  bool have_parts;         // one.out_host[1..2] hold logdet / quad of a single evaluation that succeeded (mi_gp_lml_parts; grown by
                           // mi_gp_append): cleared by every single evaluation that fails or is refused
  const double* diag_dev;  // optional per-point diagonal added at assembly (mi_gp_set_diag)
  int cap;                 // points the n-dependent scratch above is sized for (mi_gp_reserve; n until it is called)
  size_t gxs_elems;        // doubles gxs_dev holds
  double* app_stats_dev;   // [4] mi_gp_append's scalar increments and bad-pivot word
  int objective;           // option 48: what mi_gp_lml_grad returns -- 0 the log marginal likelihood, 1 the leave-one-out log
                           // predictive density (loo_objective() behind the ordinary evaluation)
  int cv_block;            // option 49: the fold size b of the objective under option 48 = 1 -- 1 (default) leave-one-out, 2..128 the
                           // leave-block-out density over the contiguous folds [f b, min((f + 1) b, n))
  int trend;               // option 50: the TREND whose coefficients are integrated out -- 0 none, 1 constant h = [1], 2 linear
                           // h = [1, x_1 .. x_d] (mi_gp_lml_grad, mi_gp_factor and mi_gp_predict; api_trend.hip)
  int nout;                // option 51: the number of OUTPUTS q under one shared kernel -- 1 (default) the single y, 2..128 the vectors
                           // y_dev[o * lda ..) (mi_gp_lml_grad, mi_gp_factor and mi_gp_predict; api_multi.hip)
  int outcov;              // option 52: the covariance BETWEEN the outputs of option 51 = q >= 2 -- 0 (default) none, the outputs
                           // independent under one variance; 1 a q x q Sigma under the Jeffreys prior, integrated out (api_multi.hip).
                           // Part of the outputs' block's layout: a change drops the block
  int sweep;               // option 53: what mi_gp_predict_grad is -- 0 (default) the conditional and its gradients, 1 the MEAN SWEEP,
                           // the matrix-free posterior mean and its input gradient (mean_sweep(), api_sweep.hip)
  int npaths;              // option 54: 0 (default) mi_gp_predict_grad is what option 53 says; S = 1..128: it is the PATH SWEEP of S
                           // posterior sample paths over the caller's path block (path_sweep(), api_paths.hip)
  int nfeat;               // option 55: F, the random Fourier features of a path's prior draw (a multiple of 16 in 16..65536; read
                           // only under option 54 >= 1)
  int design_b;            // option 56: 0 (default) mi_gp_predict_cov is the joint conditional; b = 1..128: it is the DESIGN CALL that
                           // selects up to b of the candidates in Xnew_dev (design_select(), api_design.hip)
  int design_nref;         // option 57: Mr, the reference points behind the candidates in Xnew_dev (0: the maximum-variance criterion;
                           // read only under option 56 >= 1)
  CapBlock blocks[BLK_COUNT];  // the modes' scratch, by BlockId (each allocated by its mode's first use)
  int deriv_npts;          // 0 (default), or the points of a GRADIENT BINDING (mi_gp_deriv_bind, api_deriv.hip, the only writer): the
                           // n = deriv_npts (1 + d) observations are [y ; d_1 y ; .. ; d_d y] at the deriv_npts x d points of X_dev
  char err[256];
};

inline int hfail(mi_gp_handle* h, hipError_t e, const char* where) {
  snprintf(h->err, sizeof(h->err), "%s: %s", where, hipGetErrorString(e));
  return -2;
}

#define HCK(call, where)                          \
  do {                                            \
    hipError_t e__ = (call);                      \
    if (e__ != hipSuccess) return hfail(h, e__, where); \
  } while (0)

// Ends the resident state: the factor, U and K^-1 of the single problem and the batch's conditional factors belong to the data,
// diagonal and model they were computed with.  (Each call site says why its change ends them.)
inline void drop_resident(mi_gp_handle* h) {
  h->factored = h->have_kinv = h->have_u = false;
  h->b_cond_k = 0;
}

// frees b; what it held is not kept.  The stream that used it must be idle
inline void drop_block(CapBlock& b) {
  (void)hipFree(b.p);
  b = CapBlock();
}
// The mode block `id` with at least len doubles, sized for the handle's capacity: 0, or the C-ABI error code with the text set
// (`what` names the block).  A block that is missing, was sized for fewer points than h->cap or holds fewer doubles is
// allocated anew behind a synchronisation of the handle's stream (which may still read the old one); what it held is not kept
// (*fresh, where given, says so: the new block's contents are unspecified).
inline int ensure_block(mi_gp_handle* h, BlockId id, size_t len, const char* what, bool* fresh = nullptr) {
  CapBlock& b = h->blocks[id];
  if (fresh) *fresh = false;
  if (b.p && b.cap >= h->cap && b.len >= len) return 0;
  HCK(hipStreamSynchronize(h->stream), "stream sync");
  drop_block(b);
  HCK(hipMalloc(&b.p, sizeof(double) * len), what);
  b.cap = h->cap;
  b.len = len;
  if (fresh) *fresh = true;
  return 0;
}

// What the enqueue code evaluates: the single problem (one_eval) or a batch of problems (batch_eval) -- its K / Z / W, its
// scratch and its per-problem strides.  X, y and lda are the handle's (h->buf) either way.  Built by each call, never stored:
// the handle itself always describes the single problem.
struct Eval {
  double *K, *Z, *W;
  const Scratch& s;
  Batch bt;         // nb = 1 and every stride 0 for the single problem
  bool batched;
  int prof;         // profiling level (a batch: 0)
  const Batch* lb() const { return batched ? &bt : nullptr; }  // what the launchers get (nullptr: one problem)
};

// A cross-stream edge of one evaluation: a slot of sig_dev that is raised to the evaluation's epoch (by a runtime
// hipStreamWriteValue32 or by a kernel), an event of ev_pool, or nothing.  Only the edge functions of gp_sched.hip tell the
// forms apart.
struct Edge {
  int slot = -1;
  hipEvent_t ev = nullptr;
  bool armed() const { return slot >= 0 || ev != nullptr; }
};

// The scheduling state of ONE evaluation: made by run_evaluation() on its stack, passed down by reference, gone with it.
struct Sched {
  // the two-streams decision (plan_streams(), once per evaluation)
  bool la_single = false;  // the size alone asks for two streams (the narrow super-panels go with it)
  bool two = false;        // this evaluation runs on two streams
  bool asm_on_panel = false;  // its set_yrows + assembly were queued on the PANEL stream (two streams, option 45: the first leaf
                              // follows them in stream order, no cross-stream edge in front of the chain)
  int sig_next = 0;        // next free slot of sig_dev / event of ev_pool: the ORDER in which edges take them is part of the
  size_t ev_next = 0;      // schedule (one slot or event per edge, never re-used inside the evaluation)
  // Edges armed for the leaf of one tile column.  Armed by cholesky_enqueue (the step that queues the panel), consumed -- and
  // disarmed -- by chol_panel at that column's leaf (take_armed(), the only reader).
  struct Armed { int col = -1; Edge edge; };
  Armed wait;   // behind the leaf + strip of column wait.col the panel stream waits for the main stream's (a2) update of the
                // columns wait.col + 1 .. (option 26 = 2: the leaf itself polls before it ends)
  Armed wait2;  // the leaf of column wait2.col ends only once this slot is written (everything queued on the main stream before
                // the super-panel's chain: the first in-panel update behind that leaf writes the next super-panel's first column)
  Armed done;   // the update behind the strip of column done.col raises this slot ("super-panel done")
  // U = L^-T inside the factorisation's tail (options 30 / 31)
  bool u_early = false;                      // this evaluation takes part (set by enqueue_all)
  int u_leaf_done = 0, u_node_done[12] = {}; // tile columns whose leaf block of U is done / full nodes done per level
};

// One operand of gemm_call: pointer, leading dimension, stride between the nodes of a node-batched launch, stride between the
// problems of a batched evaluation
template <class T>
struct Operand {
  T* p;
  long ld;
  long node = 0;
  long z = 0;
};
using In = Operand<const double>;
using Out = Operand<double>;

// gp_sched.hip
int run_evaluation(mi_gp_handle* h, const Eval& E, int what);
hipError_t inverse_transpose(mi_gp_handle* h, const Eval& E);  // all of U = L^-T behind a factorisation that started none of it
hipError_t gemm_call(mi_gp_handle* h, const Eval& E, int ak, int bk, In A, In B, Out C, int mt, int nt, int k, int tri, int kmode,
                     double alpha, double beta, int batch, bool single_form = false);

// api_gp.hip
Eval one_eval(const mi_gp_handle* h);  // the single problem
int make_u_resident(mi_gp_handle* h);  // U = L^-T in Z_dev and alpha = U beta, once per mi_gp_factor; 0 or a C-ABI error code
// mi_gp_append's phase 1 (also mi_gp_logpdf's value): L21, the factor of the Schur complement and beta2 in the caller's work block,
// stats = {sum log diag L22, |beta2|^2, bad-pivot word}; 0 or a C-ABI error code
int conditional_block(mi_gp_handle* h, const double* Xnew_dev, const double* ynew_dev, const double* diag_new_dev, int k,
                      double* work_dev, long ldw, double stats[3]);
// What mi_gp_lml_grad and the objectives behind it hand back: a bad code gives -inf, a zero gradient and the code, 0 the value and
// the gradient the contraction left in grad_host
inline int finish_objective(const mi_gp_handle* h, int bad, double value, double* value_out, double* grad_out) {
  *value_out = bad ? -INFINITY : value;
  for (int i = 0; i < h->ntheta; ++i) grad_out[i] = bad ? 0.0 : h->one.grad_host[i];
  return bad;
}

// The k-segmented 128 x 128 Gram product A B^T (bk = 0: B stored like A, [128][k]) or A B (bk = 1: B stored [k][128]) over
// k = 128 ntc (api_gp.hip): a single output tile over all of k would run on four workgroups, so k is cut into segments of
// (ntc + 63) / 64 tile columns -- one node-batched launch over the full segments, one over the tail -- whose 128 x 128 products go
// to parts, MINV_ELEMS apart (at most 65).  *nparts = how many there are, for a kernel that adds them in index order.
hipError_t gram_segments(mi_gp_handle* h, const Eval& E, In A, In B, int bk, double* parts, int* nparts);

// api_kfold.hip: the work block of a fold pass for `pass` folds at a time -- `pass` gathered blocks (the leaf factorises them in
// place), `pass` leaf inverses and `pass` x 256 gathered alpha_I / y_I, then as ints the staged fold_idx [total], fold_ptr
// [nfolds + 1] and one bad-pivot word per fold [nfolds] (nfolds <= total: 2 * total + 2 doubles hold them)
struct FoldWork {
  int pass;
  double *blocks, *minv, *vecs;
  int *idx, *ptr, *info;
};
inline long fold_work_len(long pass, long total) { return pass * (2 * MINV_ELEMS + 256) + 2 * total + 2; }
inline FoldWork fold_layout(double* base, long pass, long total, int nfolds) {
  FoldWork w;
  w.pass = (int)pass;
  w.blocks = base;
  w.minv = w.blocks + pass * MINV_ELEMS;
  w.vecs = w.minv + pass * MINV_ELEMS;
  w.idx = reinterpret_cast<int*>(w.vecs + pass * 256);
  w.ptr = w.idx + total;
  w.info = w.ptr + nfolds + 1;
  return w;
}
// The fold pass over the resident K^-1 and alpha: the host lists go up (they must live until the stream is synchronised), then
// per pass of w.pass folds launch_kfold_gather, the batched 128 x 128 leaf and the caller's step(f0, nf) for the folds
// f0 .. f0 + nf - 1, all on the handle's stream; 0 or a C-ABI error code
int fold_pass(mi_gp_handle* h, const FoldWork& w, int nfolds, const int* ptr_host, const int* idx_host,
              const std::function<hipError_t(int, int)>& step);

// api_loo.hip: the tail of mi_gp_lml_grad under option 48 = 1, behind a successful ordinary evaluation (K^-1 in W_dev, alpha
// resident).  *value = L_LOO and grad[ntheta] its gradient; 0, the 1-based index of the first bad K^-1_ii (-inf, zero gradient) or
// a C-ABI error code.  Under option 49 = b > 1 the k-fold objective over the contiguous folds of b points instead (the same tail
// behind another B; the return value is then the index of the point at the bad pivot of a fold's block).  Weak: api_gp.hip also
// links without it (the host-only schedule-trace program), and option 48 = 1 and option 49 > 1 are refused there.
int loo_objective(mi_gp_handle* h, double* value, double* grad) __attribute__((weak));

// api_trend.hip: the trend of option 50 (include/mi_gp.h has the algebra).  Weak like loo_objective: without the file option
// 50 != 0 is refused.
inline int trend_columns(const mi_gp_handle* h) { return h->trend == 1 ? 1 : h->trend == 2 ? 1 + h->cfg.d : 0; }
// the tail of mi_gp_lml_grad behind a successful ordinary evaluation (K^-1 in W_dev, alpha resident): *value = L_T and grad[ntheta]
// its gradient, W_dev's lower triangle then holds P~; 0, n + j for a bad pivot j of A = H^T K^-1 H (-inf, zero gradient) or a C-ABI
// error code
int trend_objective(mi_gp_handle* h, double* value, double* grad) __attribute__((weak));
// behind a successful mi_gp_factor: G^T = (L^-1 H)^T, C_A = chol(G^T G), its inverse, beta^ and b~ in the handle's scratch; 0,
// n + j or a C-ABI error code
int trend_factor(mi_gp_handle* h) __attribute__((weak));
// mi_gp_predict's reduction under a trend (the rows L^-1 k(X, x*) are in work_dev)
hipError_t trend_predict_reduce(mi_gp_handle* h, const double* Xnew_dev, const double* work_dev, long ldw, int m, double* mean_dev,
                                double* var_dev, int pred_noise) __attribute__((weak));
// mi_gp_reserve's part: the scratch re-sized for `capacity` points, the conditional's state (G^T, C_A^-1, beta^, b~) kept
hipError_t trend_reserve(mi_gp_handle* h, int capacity) __attribute__((weak));
// doubles of the trend's scratch for up to cap points (TrendScratch, api_trend.hip)
constexpr int TREND_PARTS = 65;
inline size_t trend_scratch_len(int cap) {
  const size_t vl = (size_t)(cap + 127) / 128 * 128;
  return 128 * (vl + 16) + 2 * vl * 128 + (size_t)(TREND_PARTS + 3) * MINV_ELEMS + 3 * 128 + 2 * vl + 8 + 2;
}
// the -1 of an entry point that has no form under a trend
inline int refuse_trend(mi_gp_handle* h, const char* entry) {
  snprintf(h->err, sizeof(h->err), "%s has no form under a trend (option 50 = %d): set option 50 to 0 first", entry, h->trend);
  return -1;
}

// api_multi.hip: several outputs under one shared kernel (option 51; include/mi_gp.h has the algebra).  Weak like loo_objective:
// without the file option 51 >= 2 is refused.
// the tail of mi_gp_lml_grad behind a successful ordinary evaluation (K^-1 in W_dev; out_host[1] the factorisation's logdet):
// *value = L_MO and grad[ntheta] its gradient, W_dev's lower triangle then holds q K^-1 - V V^T; 0 or a C-ABI error code.
// Under option 52 = 1: *value = L_S, W_dev's lower triangle then holds q K^-1 - n V S^-1 V^T; 0, n + j for a bad pivot j of
// S = Y^T K^-1 Y (-inf, zero gradient) or a C-ABI error code
int multi_objective(mi_gp_handle* h, double* value, double* grad) __attribute__((weak));
// behind a successful mi_gp_factor: B^T = Y^T L^-T (128 rows, rows from q on zero) in the handle's scratch, and under option
// 52 = 1 the scales s_o = |b_o|^2 / (n - q - 1); 0 or a C-ABI error code
int multi_factor(mi_gp_handle* h) __attribute__((weak));
// mi_gp_predict's reduction under q outputs (the rows L^-1 k(X, x*) are in work_dev): mean[o * m + i], var[i] (option 52 = 1:
// var[o * m + i])
hipError_t multi_predict_reduce(mi_gp_handle* h, const double* work_dev, long ldw, int m, double* mean_dev, double* var_dev,
                                int pred_noise) __attribute__((weak));
// mi_gp_reserve's part: the scratch re-sized for `capacity` points, the conditional's B^T kept
hipError_t multi_reserve(mi_gp_handle* h, int capacity) __attribute__((weak));
// the -1 of an entry point that has no form under several outputs
inline int refuse_multi(mi_gp_handle* h, const char* entry) {
  snprintf(h->err, sizeof(h->err), "%s has no form under several outputs (option 51 = %d): set option 51 to 1 first", entry, h->nout);
  return -1;
}
// api_deriv.hip: the gradient binding (include/mi_gp_deriv.h has the algebra).  Weak like loo_objective: a library without the file
// has no mi_gp_deriv_bind, so deriv_npts stays 0 and none of the three is reached.  Each stands where the plain launch stands --
// the training assembly of enqueue_factor, the contraction of enqueue_gradient, the cross-covariance of mi_gp_predict -- with the
// plain launch's arguments and stream
hipError_t deriv_assemble_train(mi_gp_handle* h, const Eval& E, int noise_form, hipStream_t st) __attribute__((weak));
hipError_t deriv_grad_contract(mi_gp_handle* h, const Eval& E) __attribute__((weak));
hipError_t deriv_assemble_cross(mi_gp_handle* h, const double* Xnew_dev, int m, double* work_dev, long ldw, int mp) __attribute__((weak));
// the -1 of an entry point that has no form under a gradient binding (0 without one)
inline int refuse_deriv(mi_gp_handle* h, const char* entry) {
  if (!h->deriv_npts) return 0;
  snprintf(h->err, sizeof(h->err), "%s has no form under a gradient binding (mi_gp_deriv_bind, %d points): unbind with npts = 0 first",
           entry, h->deriv_npts);
  return -1;
}
// api_gp.hip: is every mode option (48-57) at its default
bool modes_at_default(const mi_gp_handle* h);

// an entry point that has no form under a trend or several outputs: 0, or the -1 of the trend's refusal, else of the outputs'
inline int refuse_trend_or_multi(mi_gp_handle* h, const char* entry) {
  return h->trend != 0 ? refuse_trend(h, entry) : h->nout > 1 ? refuse_multi(h, entry) : 0;
}
// an entry point of the plain model alone (no trend, one output, no gradient binding): 0 or the -1 of the first that refuses
inline int refuse_plain_model(mi_gp_handle* h, const char* entry) {
  if (int r = refuse_trend_or_multi(h, entry)) return r;
  return refuse_deriv(h, entry);
}
// option 52 = 1 under q >= 2 outputs integrates a q x q covariance out: n >= q + 2 (the predictive t has n - q + 1 degrees of
// freedom, its variance needs more than two).  True -- and the text is set -- when the entry point must return -1
inline bool refuse_outcov(mi_gp_handle* h, const char* entry) {
  if (!(h->outcov && h->nout > 1) || h->n >= h->nout + 2) return false;
  snprintf(h->err, sizeof(h->err), "%s: the between-output covariance (option 52 = 1) of q = %d outputs needs n >= q + 2, got n = %d",
           entry, h->nout, h->n);
  return true;
}

// api_sweep.hip: mi_gp_predict_grad under option 53 = 1 (include/mi_gp.h has the contract).  Weak like loo_objective: without the
// file option 53 = 1 is refused.  0 or a C-ABI error code; every refusal comes before any HIP call
int mean_sweep(mi_gp_handle* h, const double* Xnew_dev, int m, double* mean_dev, double* dmean_dev) __attribute__((weak));

// api_paths.hip: mi_gp_predict_grad under option 54 = S >= 1 (include/mi_gp.h has the contract).  Weak like mean_sweep: without
// the file option 54 >= 1 is refused.  0 or a C-ABI error code; every refusal comes before any HIP call
int path_sweep(mi_gp_handle* h, const double* Xnew_dev, int m, double* block_dev, long ldw, double* mean_dev, int condition,
               double* dmean_dev) __attribute__((weak));

// api_design.hip: mi_gp_predict_cov under option 56 = b >= 1 (include/mi_gp.h has the contract).  Weak like mean_sweep: without the
// file option 56 >= 1 is refused.  0 or a C-ABI error code; every refusal comes before any HIP call
int design_select(mi_gp_handle* h, const double* Xnew_dev, int m, double* work_dev, long ldw, double* out_dev, double* G_dev, long ldc,
                  int pred_noise) __attribute__((weak));

// api_gp.hip
hipError_t trsm_rec(mi_gp_handle* h, const Eval& E, double* Bw, long ldw, int mp, int c0, int w);  // X L^T = B in place
// mi_gp_predict's scalars at the factored theta: the composite prior variance (Stationary.diag == 1: the +/* fold of kv) and
// sqrt(gv)^2 with pred_noise
inline void predict_scalars(const mi_gp_handle* h, int pred_noise, double* kdiag, double* noise) {
  const int nk = h->spec.nkern, d = h->spec.d;
  const double* th = h->one.theta_host;
  double kd = th[nk * d];
  for (int c = 1; c < nk; ++c) kd = (h->spec.op[c - 1] == 0) ? kd + th[nk * d + c] : kd * th[nk * d + c];
  const double sg = std::sqrt(th[nk * d + 2 * nk]);
  *kdiag = kd;
  *noise = pred_noise ? sg * sg : 0.0;
}
