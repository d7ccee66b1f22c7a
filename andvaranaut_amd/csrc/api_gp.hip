// Handle-level C-ABI (include/mi_gp.h): covariance assembly -> blocked right-looking Cholesky ->
// log marginal likelihood.  Replaces what pm.find_MAP / pm.sample evaluate per step through
// pm.gp.Marginal.marginal_likelihood (gpmcmc.py:321-323, 345, 351).
#include "gp_handle.h"

extern "C" const char* mi_gp_last_error(mi_gp_handle* h) { return h ? h->err : "null handle"; }

// The per-problem sizes of the Scratch arrays for up to `cap` points, as the strides of a Batch (+ 4 blocks behind the leaf
// inverses: the strips' operand-order copies of their first 256 rows for the thin updates, two buffers of two blocks --
// column mode reads the previous column's copy beside the current one's)
static Batch scratch_strides(const mi_gp_handle* h, int cap) {
  const long np = (cap + 127) / 128 * 128;
  Batch bt;
  bt.sdinv = MINV_ELEMS * (np / 128 + 4); bt.salpha = np; bt.spart = (long)grad_contract_blocks(cap) * h->ntheta;
  bt.stheta = h->ntheta; bt.sinfo = 4; bt.sout = 16;
  return bt;
}

static void free_scratch(Scratch& s) {
  (void)hipFree(s.theta_dev); (void)hipFree(s.dinv_dev); (void)hipFree(s.alpha_dev); (void)hipFree(s.part_dev);
  (void)hipFree(s.info_dev); (void)hipFree(s.lr_part_dev); (void)hipFree(s.lr_sync_dev);
  if (s.grad_host) (void)hipHostFree(s.grad_host);
  if (s.out_host) (void)hipHostFree(s.out_host);
  if (s.theta_host) (void)hipHostFree(s.theta_host);
  s = Scratch();
}

// s (empty) for k problems of up to cap points; on failure s keeps what it got (free_scratch) and k stays 0
static hipError_t alloc_scratch(const mi_gp_handle* h, Scratch& s, int k, int cap) {
  const Batch z = scratch_strides(h, cap);
  const size_t kk = (size_t)k;
  hipError_t e = hipMalloc(&s.theta_dev, sizeof(double) * kk * z.stheta);
  if (e == hipSuccess) e = hipMalloc(&s.dinv_dev, sizeof(double) * kk * z.sdinv);
  if (e == hipSuccess) e = hipMalloc(&s.alpha_dev, sizeof(double) * kk * z.salpha);
  if (e == hipSuccess) e = hipMalloc(&s.part_dev, sizeof(double) * kk * z.spart);
  if (e == hipSuccess) e = hipMalloc(&s.info_dev, sizeof(int) * kk * z.sinfo);
  if (e == hipSuccess) e = hipMalloc(&s.lr_part_dev, sizeof(double) * kk * 2 * LML_REDUCE_BLOCKS);
  if (e == hipSuccess) e = hipMalloc(&s.lr_sync_dev, sizeof(unsigned) * kk * 2);
  if (e == hipSuccess) e = hipMemset(s.lr_sync_dev, 0, sizeof(unsigned) * kk * 2);
  if (e == hipSuccess) e = hipHostMalloc(&s.grad_host, sizeof(double) * kk * z.stheta);
  if (e == hipSuccess) e = hipHostMalloc(&s.out_host, sizeof(double) * kk * z.sout);
  if (e == hipSuccess) memset(s.out_host, 0, sizeof(double) * kk * z.sout);  // (the sequence words: wait_evaluation())
  if (e == hipSuccess) e = hipHostMalloc(&s.theta_host, sizeof(double) * kk * z.stheta);
  if (e == hipSuccess) s.k = k;
  return e;
}

Eval one_eval(const mi_gp_handle* h) {
  return {h->buf.K_dev, h->buf.Z_dev, h->buf.W_dev, h->one, Batch(), false, h->prof_level};
}

// the first k problems of the batch buffers and scratch
static Eval batch_eval(const mi_gp_handle* h, int k) {
  Batch bt = scratch_strides(h, h->n);
  bt.nb = k;
  bt.sK = h->bbuf.stride_k; bt.sZ = bt.sW = h->bbuf.stride_zw;
  return {h->bbuf.K_dev, h->bbuf.Z_dev, h->bbuf.W_dev, h->batch, bt, true, 0};
}

// frees whatever a (possibly half-built) handle owns; every member is null / empty until it is created
static void release_handle(mi_gp_handle* h) {
  (void)hipSetDevice(h->device);
  if (h->pstream) (void)hipStreamSynchronize(h->pstream);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  free_scratch(h->one);
  free_scratch(h->batch);
  (void)hipFree(h->sig_dev); (void)hipFree(h->gxs_dev); (void)hipFree(h->app_stats_dev);
  for (CapBlock& b : h->blocks) (void)hipFree(b.p);
  for (int i = 0; i < 8; ++i) if (h->ev[i]) (void)hipEventDestroy(h->ev[i]);
  for (auto& ev : h->gemm_ev) (void)hipEventDestroy(ev);
  for (auto& ev : h->ev_pool) (void)hipEventDestroy(ev);
  if (h->pstream) (void)hipStreamDestroy(h->pstream);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

// The default edges (option 26 = 2) enqueue a poll on the panel stream AHEAD of the main-stream write it waits for.  That ends
// only through its limit where kernel dispatch is serialised: rocprofv3 --pmc, AMD_SERIALIZE_KERNEL / HIP_LAUNCH_BLOCKING, a
// debugger.  One probe at creation -- a one-lane poll on the panel stream with a short limit (2^14 sleeps: a few ms), the write
// behind it on the main stream -- finds that out before an evaluation can stall for seconds; such a handle uses events
// (gpmcmc.py:331-339: the reference's evaluations never fail for reasons of scheduling).  ~40 us where dispatch is concurrent.
static hipError_t probe_dispatch(mi_gp_handle* h) {
  hipError_t e = hipMemset(h->one.info_dev, 0x7f, sizeof(int) * 4);
  // (both streams have launched before: the probe does not time the first launch's code-object load)
  if (e == hipSuccess) e = launch_signal_write_wait(h->sig_dev + SIG_SLOTS - 1, nullptr, 0u, h->one.info_dev, h->pstream);
  if (e == hipSuccess) e = launch_signal_write_wait(h->sig_dev + SIG_SLOTS - 1, nullptr, 0u, h->one.info_dev, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->pstream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e == hipSuccess) e = launch_signal_write_wait(nullptr, h->sig_dev + SIG_SLOTS - 1, 1u, h->one.info_dev, h->pstream, 1, 0, 14);
  if (e == hipSuccess) e = launch_signal_write_wait(h->sig_dev + SIG_SLOTS - 1, nullptr, 1u, h->one.info_dev, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->pstream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  int info = 0;
  if (e == hipSuccess) e = hipMemcpy(&info, h->one.info_dev, sizeof(int), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemset(h->sig_dev + SIG_SLOTS - 1, 0, sizeof(unsigned));
  if (e == hipSuccess && info == SIGNAL_TIMEOUT_INFO) {
    h->use_smo = 0;
    h->demoted = true;
    snprintf(h->err, sizeof(h->err), "kernel dispatch is serialised on this device: cross-stream edges are events (option 26 = 0)");
  }
  return e;
}

// ---------------------------------------------------------------- tuning options (include/mi_gp.h lists them)
// The plain options: a member, its default and its clamp (flag: normalised to 0 / 1).  mi_gp_create takes the defaults from
// here, mi_gp_set_option and mi_gp_get_option look the id up; the modes follow in mode_options, the few options that do more
// than either in special_option().
constexpr int ANY_LO = -2147483647 - 1, ANY_HI = 2147483647;
struct PlainOption {
  int id;
  int mi_gp_handle::*member;
  int lo, hi;
  bool flag;
  int def;
};
static const PlainOption plain_options[] = {
    {0, &mi_gp_handle::lookahead, 0, 2, false, 1},
    {7, &mi_gp_handle::small_below, ANY_LO, ANY_HI, false, GemmParams().small_below},  // (768 looked 1 % better at N = 6144 .. 12288 while the 64x64-tile kernel carried the k-flush branch; without it: level)
    // round-2 A/B (tools/dev_ab_opts.py, interleaved in one process): bulk updates at one workgroup per CU whenever the
    // panel chain runs beside them (N = 16384: 29.99 -> 28.97 ms) and 8-tile super-panels at every size (N = 2048 1.045 ->
    // 1.017 ms, 4096 2.470 -> 2.388, 8192 6.417 -> 6.348, 16384 28.59 -> 28.39 against the 8 / 4 split of round 1)
    // (the super-panel widths: options 4-6, special_defaults())
    {8, &mi_gp_handle::lowocc_thr, ANY_LO, ANY_HI, false, 1 << 20},
    {9, &mi_gp_handle::tail_small, 0, 1, true, 1},
    {14, &mi_gp_handle::band_rows, ANY_LO, ANY_HI, false, GemmParams().band},
    {16, &mi_gp_handle::chain_prio, ANY_LO, ANY_HI, false, 1},  // N = 8192: 6.06 -> 5.94 ms, N = 16384: 28.11 -> 27.74 ms (interleaved A/B)
    {18, &mi_gp_handle::split_tiles, ANY_LO, ANY_HI, false, 1536},  // (2048 until the chain got shorter -- stream memory operations, strip kernel: N = 16384 26.21 -> 25.96 ms,
                                                                    // 1024: 26.21, 1280: 26.09, 1792: 26.08; N = 12288 flat)
    {19, &mi_gp_handle::split_min_rest, ANY_LO, ANY_HI, false, 1024},
    {20, &mi_gp_handle::merge_min_tiles, ANY_LO, ANY_HI, false, 72},
    {21, &mi_gp_handle::single_below, ANY_LO, ANY_HI, false, 8},  // (16 with event hand-offs; with option 26: N = 4096 1.983 -> 1.958 ms, 8192 5.50 -> 5.49, 16384 26.84 -> 26.73)
    {27, &mi_gp_handle::poll_limit_log2, 4, 30, false, 22},
    {30, &mi_gp_handle::u_early_max_s, 0, ANY_HI, false, 16},
    {31, &mi_gp_handle::u_early_cols, 8, ANY_HI, false, 48},
    {32, &mi_gp_handle::thin_max_wg, 0, ANY_HI, false, 2048},
    {35, &mi_gp_handle::ext_rows, 0, ANY_HI, false, 32},
    {37, &mi_gp_handle::rl_cols, 0, ANY_HI, false, 24},
    {38, &mi_gp_handle::rl_group, 1, 8, false, 8},
    {45, &mi_gp_handle::start_on_panel, 0, 1, true, 1},
    {46, &mi_gp_handle::rl_whole, 0, ANY_HI, false, 31},
};

// The mode options (48-57): what an entry point computes.  Where a knob clamps, a mode refuses: a value outside lo..hi (or no
// multiple of step), a value other than the default whose code is not linked (the weak functions of gp_handle.h: the host-only
// schedule-trace program links api_gp.hip without them), and whatever `refuse` adds.  A new mode is a row here, a BlockId for its
// scratch (gp_handle.h) and its dispatch in the entry point it changes.  The texts are the C-ABI's: callers and tests read them.
enum ModeEffect {
  MODE_KEEPS,          // no resident state changes with the option
  MODE_ENDS_RESIDENT,  // a change ends the resident state as mi_gp_set_data does: the factor belongs to the model it was computed under
  MODE_ENDS_RESIDENT_DROPS_MULTI,  // ... and the outputs' scratch is laid out for the option's value: its next use allocates it again
};
struct ModeOption {
  int id;
  int mi_gp_handle::*member;
  int def;                // the default, and the value that needs nothing linked: the mode is off
  int lo, hi, step;
  const char* legal;      // "mi_gp_set_option: option <id> is <legal>, got <value>"
  bool (*built)();        // are the mode's functions linked (nullptr: it has none)
  const char* not_built;  // the refusal when they are not: snprintf's format with the value as its one argument, so at most one
                          // conversion, a %d
  bool (*refuse)(mi_gp_handle*, int);  // nullptr, or a further check of the value: true with the text set
  ModeEffect effect;
};
static bool linear_trend_too_wide(mi_gp_handle* h, int value) {
  if (value != 2 || h->cfg.d <= 127) return false;
  snprintf(h->err, sizeof(h->err), "mi_gp_set_option: the linear trend (option 50 = 2) needs d <= 127, got %d", h->cfg.d);
  return true;
}
static bool loo_built() { return loo_objective; }
static bool trend_built() { return trend_objective && trend_factor && trend_predict_reduce; }
static bool multi_built() { return multi_objective && multi_factor && multi_predict_reduce; }
static bool sweep_built() { return mean_sweep; }
static bool paths_built() { return path_sweep; }
static bool design_built() { return design_select; }
static_assert(DESIGN_MAX_B == 128, "the text of option 56 names the largest batch");
static const ModeOption mode_options[] = {
    {48, &mi_gp_handle::objective, 0, 0, 1, 1, "0 (log marginal likelihood) or 1 (leave-one-out)", loo_built,
     "mi_gp_set_option: the leave-one-out objective (option 48 = 1) is not part of this build", nullptr, MODE_KEEPS},
    {49, &mi_gp_handle::cv_block, 1, 1, 128, 1, "a fold size of 1 (leave-one-out) to 128 points", loo_built,
     "mi_gp_set_option: the k-fold objective (option 49 > 1) is not part of this build", nullptr, MODE_KEEPS},
    {50, &mi_gp_handle::trend, 0, 0, 2, 1, "0 (no trend), 1 (constant) or 2 (linear)", trend_built,
     "mi_gp_set_option: the trend (option 50 = %d) is not part of this build", linear_trend_too_wide, MODE_ENDS_RESIDENT},
    {51, &mi_gp_handle::nout, 1, 1, 128, 1, "a number of outputs of 1 (the single y) to 128", multi_built,
     "mi_gp_set_option: several outputs (option 51 = %d) are not part of this build", nullptr, MODE_ENDS_RESIDENT},
    {52, &mi_gp_handle::outcov, 0, 0, 1, 1, "0 (independent outputs) or 1 (the between-output covariance integrated out)", multi_built,
     "mi_gp_set_option: the between-output covariance (option 52 = %d) is not part of this build", nullptr, MODE_ENDS_RESIDENT_DROPS_MULTI},
    {53, &mi_gp_handle::sweep, 0, 0, 1, 1, "0 (the conditional and its gradients) or 1 (the mean sweep)", sweep_built,
     "mi_gp_set_option: the mean sweep (option 53 = 1) is not part of this build", nullptr, MODE_KEEPS},
    {54, &mi_gp_handle::npaths, 0, 0, 128, 1, "0 (no paths) or a number of sample paths of 1 to 128", paths_built,
     "mi_gp_set_option: the path sweep (option 54 >= 1) is not part of this build", nullptr, MODE_KEEPS},
    {55, &mi_gp_handle::nfeat, 1024, 16, 65536, 16, "a number of features, a multiple of 16 in 16..65536", nullptr, nullptr, nullptr, MODE_KEEPS},
    {56, &mi_gp_handle::design_b, 0, 0, DESIGN_MAX_B, 1, "0 (the joint conditional) or a batch of 1 to 128 points to select",
     design_built, "mi_gp_set_option: the design call (option 56 >= 1) is not part of this build", nullptr, MODE_KEEPS},
    {57, &mi_gp_handle::design_nref, 0, 0, ANY_HI, 1, "a number of reference points >= 0", nullptr, nullptr, nullptr, MODE_KEEPS},
};

template <class Row, size_t N>
static const Row* find_option(const Row (&rows)[N], int what) {
  for (const Row& o : rows)
    if (o.id == what) return &o;
  return nullptr;
}

// 0, or -1 with the refusal's text
static int set_mode_option(mi_gp_handle* h, const ModeOption& o, int value) {
  if (value < o.lo || value > o.hi || value % o.step != 0) {
    snprintf(h->err, sizeof(h->err), "mi_gp_set_option: option %d is %s, got %d", o.id, o.legal, value);
    return -1;
  }
  if (o.refuse && o.refuse(h, value)) return -1;
  if (value != o.def && h->deriv_npts) {
    snprintf(h->err, sizeof(h->err), "mi_gp_set_option: option %d = %d has no form under a gradient binding (mi_gp_deriv_bind, %d points): "
             "unbind with npts = 0 first", o.id, value, h->deriv_npts);
    return -1;
  }
  if (value != o.def && o.built && !o.built()) {
    snprintf(h->err, sizeof(h->err), o.not_built, value);
    return -1;
  }
  if (value == h->*o.member) return 0;
  h->*o.member = value;
  if (o.effect != MODE_KEEPS) drop_resident(h);
  if (o.effect == MODE_ENDS_RESIDENT_DROPS_MULTI && h->blocks[BLK_MULTI].p) {  // (every entry point returns with the stream synchronised)
    (void)hipSetDevice(h->device);
    drop_block(h->blocks[BLK_MULTI]);
  }
  return 0;
}

bool modes_at_default(const mi_gp_handle* h) {
  for (const ModeOption& o : mode_options)
    if (h->*o.member != o.def) return false;
  return true;
}

// defaults of the options below (2: mi_gp_config's panel_tiles)
static void special_defaults(mi_gp_handle* h) {
  h->w_thr[0] = 1 << 20; h->w_thr[1] = 0; h->w_thr[2] = 0;
  h->use_smo = 2;  // (0 where the driver lacks stream memory operations: mi_gp_create)
  h->spin_us = 2000;
}

// The options with behaviour beyond a clamp; `set` (or nullptr) is the new value, `get` (or nullptr) receives the current one.
// 1: done, 0: not one of them (40 is read-only), -1: refused (h->err says why)
static int special_option(mi_gp_handle* h, int what, const int* set, int* get) {
  switch (what) {
    case 2:
      if (set) h->cfg.panel_tiles = *set;
      else *get = h->cfg.panel_tiles;
      return 1;
    case 4: case 5: case 6:
      if (set) h->w_thr[what - 4] = *set;
      else *get = h->w_thr[what - 4];
      return 1;
    case 26:
      if (set) {
        h->use_smo = !h->smo_supported ? 0 : *set < 0 ? 0 : *set > 2 ? 2 : *set;
        if (h->use_smo != 0) h->demoted = false;  // (the caller asks for polls again: the next time-out demotes again)
      } else {
        *get = h->use_smo;
      }
      return 1;
    case 28:
      if (set) {
        // (with option 26 = 1 the waiter is a runtime hipStreamWaitValue32 without a limit: the hook would hang the process)
        if (*set && h->use_smo < 2) {
          snprintf(h->err, sizeof(h->err), "mi_gp_set_option: option 28 needs option 26 = 2 (a bounded in-kernel poll)");
          return -1;
        }
        h->test_drop_signal = *set ? 1 : 0;
      } else {
        *get = h->test_drop_signal;
      }
      return 1;
    case 40:  // 1 once the handle has demoted its edges to events
      if (set) return 0;
      *get = h->demoted ? 1 : 0;
      return 1;
    case 47:
      if (set) { h->spin_us = *set < 0 ? 0 : *set; h->spin_backoff = 0; }
      else *get = h->spin_us;
      return 1;
  }
  return 0;
}

extern "C" int mi_gp_create(const mi_gp_config* cfg, mi_gp_handle** out) {
  if (!cfg || !out) { set_global_error("mi_gp_create: null argument"); return -1; }
  if (cfg->n <= 0 || cfg->d <= 0 || cfg->nkern <= 0 || cfg->nkern > MAX_KERN) {
    set_global_error("mi_gp_create: n, d must be positive and 1 <= nkern <= 8");
    return -1;
  }
  if (const char* why = kern_spec_error(cfg->nkern, cfg->kernel_ids, cfg->ops)) {
    char msg[128];
    snprintf(msg, sizeof(msg), "mi_gp_create: %s", why);
    set_global_error(msg);
    return -1;
  }
  mi_gp_handle* h = new mi_gp_handle();  // value-initialised: every pointer / stream / event starts null, every flag, counter,
                                         // timer and the signal epoch zero
  memset(h->err, 0, sizeof(h->err));
  h->cfg = *cfg;
  h->spec = make_kern_spec(cfg->d, cfg->nkern, cfg->kernel_ids, cfg->ops);
  h->n = cfg->n;
  h->np = (cfg->n + 127) / 128 * 128;
  h->ntc = h->np / 128;
  h->ntheta = cfg->nkern * cfg->d + 2 * cfg->nkern + 2;
  h->device = cfg->device;
  h->cap = cfg->n;
  hipError_t e = hipSetDevice(h->device);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  if (e == hipSuccess) {
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
    e = hipStreamCreateWithPriority(&h->pstream, hipStreamNonBlocking, hi);
  }
  for (const PlainOption& o : plain_options) h->*o.member = o.def;
  for (const ModeOption& o : mode_options) h->*o.member = o.def;
  special_defaults(h);
  // hipStreamWriteValue32 / hipStreamWaitValue32 need driver support: without it every two-stream evaluation would fail,
  // so the edges fall back to events (option 26 = 0; mi_gp_set_option refuses 1 and 2 then)
  int can = 0;
  if (hipDeviceGetAttribute(&can, hipDeviceAttributeCanUseStreamWaitValue, h->device) != hipSuccess) can = 0;
  (void)hipGetLastError();
  h->smo_supported = can != 0;
  if (!h->smo_supported) h->use_smo = 0;
  if (e == hipSuccess) e = alloc_scratch(h, h->one, 1, h->cap);
  if (e == hipSuccess) e = hipMalloc(&h->sig_dev, sizeof(unsigned) * SIG_SLOTS);
  if (e == hipSuccess) e = hipMemset(h->sig_dev, 0, sizeof(unsigned) * SIG_SLOTS);
  for (int i = 0; i < 8 && e == hipSuccess; ++i) e = hipEventCreate(&h->ev[i]);
  if (e == hipSuccess) e = gemm_f64_enable_lds();
  if (e == hipSuccess) e = leaf_enable_lds();
  if (e == hipSuccess && h->use_smo >= 2) e = probe_dispatch(h);
  if (e != hipSuccess) {
    char msg[200];
    snprintf(msg, sizeof(msg), "mi_gp_create: %s", hipGetErrorString(e));
    set_global_error(msg);
    release_handle(h);
    return -2;
  }
  *out = h;
  return 0;
}

extern "C" int mi_gp_destroy(mi_gp_handle* h) {
  if (!h) return 0;
  release_handle(h);
  return 0;
}

extern "C" long mi_gp_padded_n(const mi_gp_handle* h) { return h ? h->np : -1; }
extern "C" int mi_gp_num_theta(const mi_gp_handle* h) { return h ? h->ntheta : -1; }
extern "C" void* mi_gp_stream(const mi_gp_handle* h) { return h ? (void*)h->stream : nullptr; }

extern "C" int mi_gp_set_data(mi_gp_handle* h, const mi_gp_buffers* b) {
  if (!h || !b || !b->X_dev || !b->y_dev || !b->K_dev) return -1;
  if (b->lda < h->np || (b->lda & 1)) {
    snprintf(h->err, sizeof(h->err), "mi_gp_set_data: lda must be even and >= padded n (%d)", h->np);
    return -1;
  }
  h->buf = *b;
  h->have_data = true;
  // (the resident factor, U and K^-1 belong to the buffers they were computed in: mi_gp_predict* behind a rebind would read an
  // unfactored K, mi_gp_alpha / mi_gp_grad_x another W)
  drop_resident(h);
  return 0;
}

extern "C" int mi_gp_set_option(mi_gp_handle* h, int what, int value) {
  if (!h) return -1;
  if (const PlainOption* o = find_option(plain_options, what)) {
    h->*o->member = o->flag ? (value ? 1 : 0) : value < o->lo ? o->lo : value > o->hi ? o->hi : value;
    return 0;
  }
  if (const ModeOption* o = find_option(mode_options, what)) return set_mode_option(h, *o, value);
  const int r = special_option(h, what, &value, nullptr);
  if (r == 0) snprintf(h->err, sizeof(h->err), "mi_gp_set_option: unknown option %d", what);
  return r > 0 ? 0 : -1;
}

// current value of a knob (the library's own defaults included)
extern "C" int mi_gp_get_option(mi_gp_handle* h, int what, int* value) {
  if (!h || !value) return -1;
  if (const PlainOption* o = find_option(plain_options, what)) {
    *value = h->*o->member;
    return 0;
  }
  if (const ModeOption* o = find_option(mode_options, what)) {
    *value = h->*o->member;
    return 0;
  }
  if (special_option(h, what, nullptr, value) > 0) return 0;
  snprintf(h->err, sizeof(h->err), "mi_gp_get_option: unknown option %d", what);
  return -1;
}

extern "C" int mi_gp_set_profiling(mi_gp_handle* h, int level) {
  if (!h) return -1;
  h->prof_level = level;
  return 0;
}

// A poll of the last evaluation ran into its limit: the factor is unsynchronised garbage.  The reference's evaluations never
// fail for reasons of scheduling (a failed one is swallowed inside the optimiser loop, gpmcmc.py:331-339), so the handle gives
// up the protocol that needs concurrent dispatch -- polls enqueued ahead of the writes they wait for -- for event edges, says
// so once through mi_gp_last_error, and the caller's loop evaluates the same theta again (attempt 1).  A second time-out (event
// edges have no polls: the test hook, or a caller who re-armed option 26 in between) is the caller's error -2.
static int poll_timeout(mi_gp_handle* h, int attempt) {
  HCK(hipStreamSynchronize(h->pstream), "panel stream sync");  // (its remaining launches ran through: every later poll gave up at once)
  if (attempt == 0 && h->use_smo != 0) {
    h->use_smo = 0;
    h->demoted = true;
    snprintf(h->err, sizeof(h->err), "a cross-stream signal was not seen within its poll limit: this handle's cross-stream edges are "
                                     "events from now on (option 26 = 0), the evaluation was repeated");
    return 0;
  }
  snprintf(h->err, sizeof(h->err), "a cross-stream signal of the factorisation was not seen within its poll limit");
  return -2;
}

// The host's end of an evaluation.  The evaluation's last kernel -- lml_reduce, or the gradient's final reduction -- publishes
// the evaluation's sequence number in the pinned result buffer (out[4] / out[5] of every problem), released at system scope
// behind the scalars it stands for.  hipStreamSynchronize costs a round trip of 6-8 us behind that kernel's end (a completion
// signal and a blocked wait); spinning on the word sees it within the PCIe write latency: N = 128 0.056 -> 0.051 ms, 512 0.161 ->
// 0.153, 1024 0.310 -> 0.291, 4096 1.424 -> 1.387.  The spin has a budget (option 47, default 2 ms); an evaluation that runs
// into it synchronises the stream as before and the handle's next 15 evaluations do not spin at all, so a long evaluation
// costs a core 2 ms in 16 calls, not its run time.  The word is the LAST thing the evaluation's last kernel does, and that
// kernel writes nothing but the pinned result buffer: after a successful spin every device-side read and write of the
// evaluation is complete and only the kernel's RETIREMENT may be outstanding.  Everything this library does next goes through
// the same stream (in order); the paths that need idle streams (time-outs, the epoch wrap, profiling events, destruction)
// synchronise them themselves; every 256th spin synchronises the stream all the same (keeps the runtime's bookkeeping of
// completed launches short).  The panel stream is idle by then: the main stream's last kernels wait for it.
static hipError_t wait_evaluation(mi_gp_handle* h, const Eval& E, int what) {
  bool seen = false;
  const int k = E.bt.nb;
  if (h->spin_us > 0 && E.prof < 1 && h->spin_backoff == 0) {
    long long want;
    memcpy(&want, &h->eval_seq, sizeof(want));
    const double* f = E.s.out_host + (what == 2 ? 5 : 4);
    const auto t0 = std::chrono::steady_clock::now();
    int p = 0;
    for (unsigned it = 1;; ++it) {
      while (p < k && __atomic_load_n(reinterpret_cast<const long long*>(f + (long)E.bt.sout * p), __ATOMIC_ACQUIRE) == want) ++p;
      if (p == k) { seen = true; break; }
      __builtin_ia32_pause();
      if ((it & 63u) == 0 && std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() > h->spin_us) break;
    }
    if (!seen) h->spin_backoff = 15;
    else if ((++h->spin_hits & 255u) == 0) seen = false;
  } else if (h->spin_backoff > 0) {
    --h->spin_backoff;
  }
  return seen ? hipSuccess : hipStreamSynchronize(h->stream);
}

static int factor_internal(mi_gp_handle* h, const double* theta, int what) {
  h->factored = false;
  h->have_kinv = false;
  h->have_u = false;
  h->have_parts = false;
  if (!h->have_data) { snprintf(h->err, sizeof(h->err), "mi_gp_set_data has not been called"); return -1; }
  if (h->b_cond_k > 0) {  // (a caller may let the single K_dev alias one of the batch's: this evaluation then overwrites that factor)
    const char *s0 = (const char*)h->buf.K_dev, *s1 = s0 + sizeof(double) * (size_t)(h->np + 128) * h->buf.lda;
    const char *b0 = (const char*)h->bbuf.K_dev, *b1 = b0 + sizeof(double) * (size_t)h->bbuf.count * h->bbuf.stride_k;
    if (s0 < b1 && b0 < s1) h->b_cond_k = 0;
  }
  HCK(hipSetDevice(h->device), "hipSetDevice");
  for (int i = 0; i < h->ntheta; ++i) {
    if (!std::isfinite(theta[i])) { snprintf(h->err, sizeof(h->err), "theta[%d] is not finite", i); return -1; }
    h->one.theta_host[i] = theta[i];
  }
  const Eval E = one_eval(h);
  for (int attempt = 0;; ++attempt) {
    const auto t_enq0 = std::chrono::steady_clock::now();
    if (int r = run_evaluation(h, E, what)) return r;
    h->t_enqueue_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_enq0).count();
    HCK(wait_evaluation(h, E, what), "stream sync");
    if ((int)h->one.out_host[3] != SIGNAL_TIMEOUT_INFO) break;
    if (int r = poll_timeout(h, attempt)) return r;
  }
  if (E.prof >= 1) {
    float ms;
    (void)hipEventElapsedTime(&ms, h->ev[0], h->ev[1]); h->t_assemble_ms = ms;
    (void)hipEventElapsedTime(&ms, h->ev[1], h->ev[2]); h->t_chol_ms = ms;
    (void)hipEventElapsedTime(&ms, h->ev[2], h->ev[3]); h->t_reduce_ms = ms;
    (void)hipEventElapsedTime(&ms, h->ev[0], h->ev[3]); h->t_total_ms = ms;
    double g = 0.0, gb = 0.0, fb = 0.0, nb = 0.0;
    for (size_t i = 0; i + 1 < h->gemm_ev_used; i += 2) {
      (void)hipEventElapsedTime(&ms, h->gemm_ev[i], h->gemm_ev[i + 1]);
      g += ms;
      if (h->gemm_ev_big[i / 2]) { gb += ms; fb += h->gemm_ev_flops[i / 2]; nb += 1.0; }
    }
    h->t_gemm_ms = g;
    h->t_gemm_big_ms = gb;
    h->gemm_big_flops = fb;
    h->n_gemm_big = nb;
    h->gemm_flops = h->gemm_flops_acc;
    h->n_gemm = (double)(h->gemm_ev_used / 2);
    if (what == 2) {
      (void)hipEventElapsedTime(&ms, h->ev[4], h->ev[5]); h->t_trtri_ms = ms;
      (void)hipEventElapsedTime(&ms, h->ev[5], h->ev[6]); h->t_lauum_ms = ms;
      (void)hipEventElapsedTime(&ms, h->ev[6], h->ev[7]); h->t_contract_ms = ms;
    }
  }
  const int info = (int)h->one.out_host[3];  // forwarded by lml_reduce_kernel (reset by set_yrows_kernel)
  if (info != 0x7f7f7f7f) return info;  // 1-based index of the first bad pivot
  h->have_parts = true;
  return 0;
}

extern "C" int mi_gp_lml(mi_gp_handle* h, const double* theta, double* lml_out) {
  if (!h || !theta || !lml_out) return -1;
  if (int r = refuse_trend_or_multi(h, "mi_gp_lml")) return r;
  const int r = factor_internal(h, theta, 0);
  if (r < 0) return r;
  if (r > 0) { *lml_out = -INFINITY; return r; }
  *lml_out = h->one.out_host[0];
  return 0;
}

extern "C" int mi_gp_lml_parts(mi_gp_handle* h, double* logdet, double* quad) {
  if (!h) return -1;
  // (out_host keeps the numbers of a failed evaluation -- NaN behind the bad pivot -- and of none at all)
  if (!h->have_parts) { snprintf(h->err, sizeof(h->err), "mi_gp_lml_parts: the last single evaluation did not succeed"); return -1; }
  if (logdet) *logdet = h->one.out_host[1];
  if (quad) *quad = h->one.out_host[2];
  return 0;
}

// out: [assemble_ms, chol_ms, reduce_ms, total_ms, gemm_ms, gemm_flops, n_gemm_launches,
//       trtri_ms, lauum_ms, contract_ms, gemm_b_ms, gemm_b_flops, n_gemm_b_launches, enqueue_ms (host, any profiling level),
//       the last mi_gp_logpdf's conditional-block, weights and gradient-kernel ms]
extern "C" int mi_gp_timers(mi_gp_handle* h, double* out, int n) {
  if (!h || !out) return -1;
  const double v[17] = {h->t_assemble_ms, h->t_chol_ms, h->t_reduce_ms, h->t_total_ms, h->t_gemm_ms, h->gemm_flops,
                        h->n_gemm, h->t_trtri_ms, h->t_lauum_ms, h->t_contract_ms, h->t_gemm_big_ms,
                        h->gemm_big_flops, h->n_gemm_big, h->t_enqueue_ms, h->t_logpdf_ms[0], h->t_logpdf_ms[1], h->t_logpdf_ms[2]};
  for (int i = 0; i < n && i < 17; ++i) out[i] = v[i];
  return 0;
}
extern "C" int mi_gp_lml_grad(mi_gp_handle* h, const double* theta, double* lml_out, double* grad_out) {
  if (!h || !theta || !lml_out || !grad_out) return -1;
  if (!h->buf.Z_dev || !h->buf.W_dev) {
    snprintf(h->err, sizeof(h->err), "mi_gp_lml_grad needs Z_dev and W_dev in mi_gp_set_data");
    return -1;
  }
  if (h->nout > 1 && (h->objective == 1 || h->trend != 0)) {
    snprintf(h->err, sizeof(h->err), "mi_gp_lml_grad: several outputs (option 51 = %d) have no form under %s", h->nout,
             h->objective == 1 ? "a cross-validation objective (option 48 = 1)" : "a trend (option 50)");
    return -1;
  }
  if (refuse_outcov(h, "mi_gp_lml_grad")) return -1;
  if (h->trend != 0 && (h->objective == 1 || h->n <= trend_columns(h))) {
    if (h->objective == 1)
      snprintf(h->err, sizeof(h->err), "mi_gp_lml_grad: no cross-validation objective (option 48 = 1) under a trend (option 50 = %d)", h->trend);
    else
      snprintf(h->err, sizeof(h->err), "mi_gp_lml_grad: the trend (option 50 = %d) has %d coefficients, n = %d must exceed that", h->trend,
               trend_columns(h), h->n);
    return -1;
  }
  // the gradient kernels run unconditionally behind the factorisation (one captured DAG); on a
  // non-positive-definite K their output is discarded
  const int r = factor_internal(h, theta, 2);
  if (r < 0) return r;
  if (finish_objective(h, r, h->one.out_host[0], lml_out, grad_out)) return r;
  h->have_kinv = true;
  // option 50 != 0: the same evaluation, then the trend's tail on the resident K^-1 and alpha (api_trend.hip); W_dev then holds P~
  if (h->trend != 0) {
    h->have_kinv = false;
    return trend_objective(h, lml_out, grad_out);
  }
  // option 51 >= 2: the same evaluation, then the outputs' tail on the resident K^-1 (api_multi.hip); W_dev then holds q K^-1 - V V^T
  if (h->nout > 1) {
    h->have_kinv = false;
    return multi_objective(h, lml_out, grad_out);
  }
  // option 48 = 1: the same evaluation, then the leave-one-out tail on the resident K^-1 and alpha (api_loo.hip)
  if (h->objective == 1) return loo_objective(h, lml_out, grad_out);
  return 0;
}

// Data-side gradients of the LML at the theta of the last successful mi_gp_lml_grad (whose K^-1 and alpha are
// still resident): dLML/dy = -alpha and dLML/dX.  They feed the chain rule through the reference's output and
// input warps (cwgp / iwgp, gpmcmc.py:211-279) and through the free observation rows of inverse_opt
// (gpmcmc.py:1096-1101), which PyMC differentiates by autodiff through the same Cholesky.
extern "C" int mi_gp_alpha(mi_gp_handle* h, double* alpha_host) {
  if (!h || !alpha_host) return -1;
  if (int r = refuse_plain_model(h, "mi_gp_alpha")) return r;
  if (!h->have_kinv) { snprintf(h->err, sizeof(h->err), "mi_gp_alpha: call mi_gp_lml_grad first"); return -1; }
  HCK(hipSetDevice(h->device), "hipSetDevice");
  HCK(hipMemcpyAsync(alpha_host, h->one.alpha_dev, sizeof(double) * h->n, hipMemcpyDeviceToHost, h->stream), "alpha download");
  HCK(hipStreamSynchronize(h->stream), "stream sync");
  return 0;
}

extern "C" int mi_gp_grad_x(mi_gp_handle* h, double* gx_dev) {
  if (!h || !gx_dev) return -1;
  if (int r = refuse_plain_model(h, "mi_gp_grad_x")) return r;
  if (!h->have_kinv) { snprintf(h->err, sizeof(h->err), "mi_gp_grad_x: call mi_gp_lml_grad first"); return -1; }
  HCK(hipSetDevice(h->device), "hipSetDevice");
  const int nsplit = grad_x_splits(h->n, h->cfg.d);
  const size_t gxs_need = (size_t)nsplit * h->n * h->cfg.d;
  if (nsplit > 1 && gxs_need > h->gxs_elems) {  // (grown by mi_gp_append: the handle's n is larger than at the first call)
    (void)hipFree(h->gxs_dev);
    h->gxs_dev = nullptr;
    h->gxs_elems = 0;
    HCK(hipMalloc(&h->gxs_dev, sizeof(double) * gxs_need), "grad_x scratch");
    h->gxs_elems = gxs_need;
  }
  HCK(launch_grad_x(h->spec, h->one.theta_dev, h->buf.X_dev, h->n, h->buf.W_dev, h->buf.lda, h->one.alpha_dev, gx_dev,
                    nsplit > 1 ? h->gxs_dev : nullptr, h->stream), "grad_x");
  HCK(hipStreamSynchronize(h->stream), "stream sync");
  return 0;
}

// Optional per-point diagonal (n doubles on the device, borrowed; nullptr removes it) added to K at assembly on
// top of the (gv, jitter) terms of theta: the observation-noise vector of inverse_opt (gpmcmc.py:1134-1158).
extern "C" int mi_gp_set_diag(mi_gp_handle* h, const double* diag_dev) {
  if (!h) return -1;
  h->diag_dev = diag_dev;
  drop_resident(h);  // (as mi_gp_set_data: K, U and K^-1 belong to the diagonal they were built with)
  return 0;
}

// ---------------------------------------------------------------- batched evaluation
// K covariances of the SAME inputs (one theta each) factorised in lockstep: every launch of the evaluation carries
// blockIdx.z = problem.  One evaluation below N ~ 10^4 is bound by its serial panel chain (leaf -> strip -> update per 128
// columns) and leaves most of the chip idle; MAP restarts (gpmcmc.py:328-343) and the NUTS chains that share a GPU
// (gpmcmc.py:351) evaluate the same data at different theta, so their chains can run side by side inside the same launches
// instead of on separate handles and streams (which stops paying at the fourth handle: hardware queues).
extern "C" int mi_gp_set_batch(mi_gp_handle* h, const mi_gp_batch_buffers* b) {
  if (!h) return -1;
  if (int r = refuse_deriv(h, "mi_gp_set_batch")) return r;
  if (!b || !b->K_dev || b->count < 1) {
    snprintf(h->err, sizeof(h->err), "mi_gp_set_batch: buffers with K_dev and count >= 1 are required");
    return -1;
  }
  const long need_k = (long)(h->np + 128) * h->buf.lda, need_z = (long)h->np * h->buf.lda;
  if (!h->have_data) { snprintf(h->err, sizeof(h->err), "mi_gp_set_batch: call mi_gp_set_data first (lda is taken from it)"); return -1; }
  if (b->stride_k < need_k || ((b->Z_dev || b->W_dev) && b->stride_zw < need_z) || (b->stride_k & 1) || (b->stride_zw & 1)) {
    snprintf(h->err, sizeof(h->err), "mi_gp_set_batch: strides must be even and >= (np + 128) * lda = %ld (K), np * lda = %ld (Z, W)", need_k, need_z);
    return -1;
  }
  HCK(hipSetDevice(h->device), "hipSetDevice");
  if (b->count > h->batch.k) {
    (void)hipStreamSynchronize(h->stream);
    free_scratch(h->batch);
    HCK(alloc_scratch(h, h->batch, b->count, h->n), "batch scratch");
  }
  h->bbuf = *b;
  h->b_cond_k = 0;
  return 0;
}

// what: 0 LML, 1 the conditional's factors (mi_gp_factor_batch: they stay in the batch buffers), 2 LML + gradient.
// info_out[p]: 0, or the 1-based index of problem p's first bad pivot (its LML is -inf then).  lml_out may be null.
static int batch_internal(mi_gp_handle* h, int k, const double* thetas, int what, double* lml_out, double* grad_out, int* info_out) {
  if (!h->have_data || h->batch.k < 1) { snprintf(h->err, sizeof(h->err), "call mi_gp_set_data and mi_gp_set_batch first"); return -1; }
  if (k < 1 || k > h->bbuf.count) { snprintf(h->err, sizeof(h->err), "batch of %d problems, buffers for %d", k, h->bbuf.count); return -1; }
  if (what == 2 && (!h->bbuf.Z_dev || !h->bbuf.W_dev)) { snprintf(h->err, sizeof(h->err), "mi_gp_lml_grad_batch needs Z_dev and W_dev in mi_gp_set_batch"); return -1; }
  HCK(hipSetDevice(h->device), "hipSetDevice");
  const Scratch& s = h->batch;
  for (int i = 0; i < k * h->ntheta; ++i) {
    if (!std::isfinite(thetas[i])) { snprintf(h->err, sizeof(h->err), "theta[%d] of problem %d is not finite", i % h->ntheta, i / h->ntheta); return -1; }
    s.theta_host[i] = thetas[i];
  }
  drop_resident(h);  // the single-evaluation state of the handle is not touched, but K_dev may alias
  const Eval E = batch_eval(h, k);
  for (int attempt = 0;; ++attempt) {
    if (int r = run_evaluation(h, E, what)) return r;
    HCK(wait_evaluation(h, E, what), "stream sync");
    // a cross-stream poll that gave up leaves unsynchronised data behind in EVERY problem: the whole batch is evaluated again
    // with event edges (poll_timeout), or fails as a whole
    bool timed_out = false;
    for (int p = 0; p < k; ++p) timed_out = timed_out || (int)s.out_host[E.bt.sout * p + 3] == SIGNAL_TIMEOUT_INFO;
    if (!timed_out) break;
    if (int r = poll_timeout(h, attempt)) return r;
  }
  for (int p = 0; p < k; ++p) {
    const int info = (int)s.out_host[E.bt.sout * p + 3];
    const bool ok = info == 0x7f7f7f7f;
    if (info_out) info_out[p] = ok ? 0 : info;
    if (lml_out) lml_out[p] = ok ? s.out_host[E.bt.sout * p] : -INFINITY;
    if (grad_out)
      for (int i = 0; i < h->ntheta; ++i) grad_out[(size_t)p * h->ntheta + i] = ok ? s.grad_host[(size_t)p * h->ntheta + i] : 0.0;
  }
  if (what == 1) h->b_cond_k = k;
  return 0;
}

extern "C" int mi_gp_lml_batch(mi_gp_handle* h, int k, const double* thetas, double* lml_out, int* info_out) {
  if (!h || !thetas || !lml_out) return -1;
  if (int r = refuse_plain_model(h, "mi_gp_lml_batch")) return r;
  return batch_internal(h, k, thetas, 0, lml_out, nullptr, info_out);
}

extern "C" int mi_gp_lml_grad_batch(mi_gp_handle* h, int k, const double* thetas, double* lml_out, double* grad_out, int* info_out) {
  if (!h || !thetas || !lml_out || !grad_out) return -1;
  if (int r = refuse_plain_model(h, "mi_gp_lml_grad_batch")) return r;
  if (h->objective == 1) {
    snprintf(h->err, sizeof(h->err), "mi_gp_lml_grad_batch: the leave-one-out objective (option 48 = 1) has no batched form");
    return -1;
  }
  return batch_internal(h, k, thetas, 2, lml_out, grad_out, info_out);
}

// ---------------------------------------------------------------- conditional (K8)
extern "C" int mi_gp_factor(mi_gp_handle* h, const double* theta) {
  if (!h || !theta) return -1;
  if (h->nout > 1 && h->trend != 0) {
    snprintf(h->err, sizeof(h->err), "mi_gp_factor: several outputs (option 51 = %d) have no form under a trend (option 50)", h->nout);
    return -1;
  }
  if (refuse_outcov(h, "mi_gp_factor")) return -1;
  if (h->trend != 0 && h->n <= trend_columns(h)) {
    snprintf(h->err, sizeof(h->err), "mi_gp_factor: the trend (option 50 = %d) has %d coefficients, n = %d must exceed that", h->trend,
             trend_columns(h), h->n);
    return -1;
  }
  const int r = factor_internal(h, theta, 1);
  h->factored = (r == 0);
  if (r == 0 && h->nout > 1) {  // B^T = Y^T L^-T (api_multi.hip)
    const int rm = multi_factor(h);
    h->factored = (rm == 0);
    return rm;
  }
  if (r == 0 && h->trend != 0) {  // G = L^-1 H, chol(G^T G), beta^ and b~ (api_trend.hip)
    const int rt = trend_factor(h);
    h->factored = (rt == 0);
    return rt;
  }
  return r;
}

// solve X L^T = B in place for tile columns [c0, c0+w) of the mp x np work matrix (a batch: every problem's, work
// blocks bt.swork apart, L_p and its leaf inverses in the batch buffers; the GEMMs take the single problem's tile form)
hipError_t trsm_rec(mi_gp_handle* h, const Eval& E, double* Bw, long ldw, int mp, int c0, int w) {
  const double* L = E.K;
  const long lda = h->buf.lda;
  const long zW = E.bt.swork, zK = E.bt.sK;
  if (w == 1) {
    return launch_trsm_strip128(E.s.dinv_dev + (size_t)c0 * MINV_ELEMS, Bw + (long)c0 * 128, ldw, mp, h->stream, E.lb(), zW);
  }
  const int w1 = w / 2, w2 = w - w1;
  hipError_t e = trsm_rec(h, E, Bw, ldw, mp, c0, w1);
  if (e != hipSuccess) return e;
  // B[:, c0+w1 : c0+w) -= X[:, c0 : c0+w1) * L[c0+w1 : c0+w, c0 : c0+w1)^T
  e = gemm_call(h, E, 0, 0, {Bw + (long)c0 * 128, ldw, 0, zW}, {L + (long)(c0 + w1) * 128 * lda + (long)c0 * 128, lda, 0, zK},
                {Bw + (long)(c0 + w1) * 128, ldw, 0, zW}, mp / 128, w2, w1 * 128, 0, 0, -1.0, 1.0, 1, true);
  if (e != hipSuccess) return e;
  return trsm_rec(h, E, Bw, ldw, mp, c0 + w1, w2);
}

// mi_gp_predict's reduction over A (one row per point in work_dev) with the single problem's beta.  Stationary.diag == 1: the
// composite diagonal is the +/* fold of kv; pred_noise adds sqrt(gv)^2
static hipError_t predict_reduce(const mi_gp_handle* h, const double* work_dev, long ldw, int m, double* mean_dev, double* var_dev,
                                 int pred_noise) {
  double kd, noise;
  predict_scalars(h, pred_noise, &kd, &noise);
  return launch_predict_reduce(work_dev, ldw, h->buf.K_dev + (long)h->np * h->buf.lda, h->n, m, kd, noise, mean_dev, var_dev,
                               h->stream);
}

extern "C" int mi_gp_predict(mi_gp_handle* h, const double* Xnew_dev, int m, double* work_dev, long ldw,
                             double* mean_dev, double* var_dev, int pred_noise) {
  if (!h || !Xnew_dev || !work_dev || !mean_dev || !var_dev || m <= 0) return -1;
  if (!h->factored) { snprintf(h->err, sizeof(h->err), "mi_gp_predict: call mi_gp_factor first"); return -1; }
  if (ldw < h->np || (ldw & 1)) { snprintf(h->err, sizeof(h->err), "mi_gp_predict: ldw must be even and >= padded n"); return -1; }
  HCK(hipSetDevice(h->device), "hipSetDevice");
  const int mp = (m + 127) / 128 * 128;
  // K(Xnew, X): one prediction point per row, zeros in the padding
  if (h->deriv_npts)  // a gradient binding: cov(f(x*), [f ; grad f](X)) in the launch's place
    HCK(deriv_assemble_cross(h, Xnew_dev, m, work_dev, ldw, mp), "assemble cross (gradient binding)");
  else
    HCK(launch_assemble(h->spec, h->one.theta_dev, Xnew_dev, m, h->buf.X_dev, h->n, work_dev, ldw, mp, h->np, 0, 0, h->stream),
        "assemble cross");
  HCK(trsm_rec(h, one_eval(h), work_dev, ldw, mp, 0, h->ntc), "trsm");
  if (h->nout > 1) HCK(multi_predict_reduce(h, work_dev, ldw, m, mean_dev, var_dev, pred_noise), "outputs predict_reduce");
  else if (h->trend != 0) HCK(trend_predict_reduce(h, Xnew_dev, work_dev, ldw, m, mean_dev, var_dev, pred_noise), "trend predict_reduce");
  else HCK(predict_reduce(h, work_dev, ldw, m, mean_dev, var_dev, pred_noise), "predict_reduce");
  HCK(hipStreamSynchronize(h->stream), "stream sync");
  return 0;
}

// ---------------------------------------------------------------- joint conditional and posterior draws
// Sigma = (K(X*, X*) + gv or jitter on the diagonal) - A A^T with mi_gp_predict's A = L^-1 K(X, X*) rows in work_dev: the
// cross-covariance, blocked solve and reduction of mi_gp_predict (same bits for the mean), then the assembly of K** and ONE
// lower-trapezoid GEMM with k = np.  The reduction's variance is parked in row 0 of cov_dev, which the assembly then overwrites
// (the rest of that row is strict upper triangle: unspecified).
extern "C" int mi_gp_predict_cov(mi_gp_handle* h, const double* Xnew_dev, int m, double* work_dev, long ldw, double* mean_dev,
                                 double* cov_dev, long ldc, int pred_noise) {
  if (h && h->design_b) return design_select(h, Xnew_dev, m, work_dev, ldw, mean_dev, cov_dev, ldc, pred_noise);  // option 56 >= 1
  const long mp = m > 0 ? (m + 127) / 128 * 128 : 0;
  const char* why = (!Xnew_dev || !work_dev || !mean_dev || !cov_dev) ? "null buffer"
                  : m <= 0 ? "m must be >= 1"
                  : (ldc < mp || (ldc & 1)) ? "ldc must be even and >= ceil(m/128)*128"
                  : !h ? "null handle"
                  : h->trend != 0 ? "no form under a trend (option 50): set option 50 to 0 first"
                  : h->nout > 1 ? "no form under several outputs (option 51): set option 51 to 1 first"
                  : h->deriv_npts ? "no form under a gradient binding (mi_gp_deriv_bind): unbind with npts = 0 first"
                  : !h->factored ? "call mi_gp_factor first"
                  : (ldw < h->np || (ldw & 1)) ? "ldw must be even and >= padded n" : nullptr;
  if (why) {
    char text[200];
    snprintf(text, sizeof(text), "mi_gp_predict_cov: %s", why);
    set_global_error(text);
    if (h) snprintf(h->err, sizeof(h->err), "%s", text);
    return -1;
  }
  HCK(hipSetDevice(h->device), "hipSetDevice");
  const Eval E = one_eval(h);
  HCK(launch_assemble(h->spec, h->one.theta_dev, Xnew_dev, m, h->buf.X_dev, h->n, work_dev, ldw, (int)mp, h->np, 0, 0, h->stream),
      "assemble cross");
  HCK(trsm_rec(h, E, work_dev, ldw, (int)mp, 0, h->ntc), "trsm");
  HCK(predict_reduce(h, work_dev, ldw, m, mean_dev, cov_dev, 1), "predict_reduce");
  HCK(launch_assemble(h->spec, h->one.theta_dev, Xnew_dev, m, Xnew_dev, m, cov_dev, ldc, (int)mp, (int)mp, 1, pred_noise ? 3 : 4,
                      h->stream), "assemble K**");
  // C -= A A^T over the lower tiles; A's padding rows are zero, so the padding of Sigma keeps the assembly's identity
  HCK(gemm_call(h, E, 0, 0, {work_dev, ldw}, {work_dev, ldw}, {cov_dev, ldc}, (int)(mp / 128), (int)(mp / 128), h->np, 1, 0,
                -1.0, 1.0, 1), "Sigma update");
  HCK(hipStreamSynchronize(h->stream), "stream sync");
  return 0;
}

// scratch of mi_gp_sample_cov, in doubles: the bad-pivot word (8 doubles), the leaf inverses of L_Sigma (one per tile column),
// Z and the product D (ceil(s/128)*128 x mp each)
static long sample_cov_work(int m, int s) {
  if (m <= 0 || s <= 0) return -1;
  const long mp = (m + 127) / 128 * 128, sp = (s + 127) / 128 * 128;
  return 8 + (mp / 128) * (long)MINV_ELEMS + 2 * sp * mp;
}
extern "C" long mi_gp_sample_cov_work(int m, int s) { return sample_cov_work(m, s); }

constexpr int SIGMA_PANEL_TILES = 4;  // tile columns per panel of the right-looking factorisation of Sigma

extern "C" int mi_gp_sample_cov(mi_gp_handle* h, double* cov_dev, long ldc, int m, const double* mean_dev, double extra_jitter,
                                int s, unsigned long long seed, unsigned long long offset, double* draws_dev, long ldd,
                                double* work_dev, long work_len) {
  const long mp = m > 0 ? (m + 127) / 128 * 128 : 0;
  const char* why = (!cov_dev || !mean_dev || !draws_dev || !work_dev) ? "null buffer"
                  : m <= 0 ? "m must be >= 1"
                  : s <= 0 ? "s must be >= 1"
                  : (ldc < mp || (ldc & 1)) ? "ldc must be even and >= ceil(m/128)*128"
                  : ldd < m ? "ldd must be >= m"
                  : !(extra_jitter >= 0.0 && std::isfinite(extra_jitter)) ? "extra_jitter must be finite and >= 0"
                  : work_len < sample_cov_work(m, s) ? "work_len is shorter than mi_gp_sample_cov_work(m, s)"
                  : !h ? "null handle"
                  : h->deriv_npts ? "no form under a gradient binding (mi_gp_deriv_bind): unbind with npts = 0 first" : nullptr;
  if (why) {
    char text[200];
    snprintf(text, sizeof(text), "mi_gp_sample_cov: %s", why);
    set_global_error(text);
    if (h) snprintf(h->err, sizeof(h->err), "%s", text);
    return -1;
  }
  HCK(hipSetDevice(h->device), "hipSetDevice");
  if (int r = ensure_kernel_attributes()) { snprintf(h->err, sizeof(h->err), "mi_gp_sample_cov: %s", mi_gp_last_global_error()); return r; }
  const int mt = (int)(mp / 128), sp = (s + 127) / 128 * 128;
  int* info_dev = reinterpret_cast<int*>(work_dev);
  double* dinv = work_dev + 8;
  double* Z = dinv + (long)mt * MINV_ELEMS;
  double* D = Z + (long)sp * mp;
  hipStream_t st = h->stream;
  const Eval E = one_eval(h);
  // L_Sigma in place: leaf / strip / in-panel updates per panel, then the trailing lower trapezoid on the GEMM
  HCK(launch_cov_prepare(cov_dev, ldc, m, (int)mp, extra_jitter, st), "cov_prepare");
  HCK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(info_dev), INFO_OK, 1, st), "info reset");
  for (int c0 = 0; c0 < mt; c0 += SIGMA_PANEL_TILES) {
    const int w = mt - c0 < SIGMA_PANEL_TILES ? mt - c0 : SIGMA_PANEL_TILES, rest = mt - c0 - w;
    double* P = cov_dev + (long)c0 * 128 * ldc + (long)c0 * 128;
    HCK(chol_panel_blocks(P, ldc, mt - c0, w, dinv + (size_t)c0 * MINV_ELEMS, info_dev, c0 * 128, st), "Sigma panel");
    if (rest > 0)
      HCK(gemm_call(h, E, 0, 0, {P + (long)w * 128 * ldc, ldc}, {P + (long)w * 128 * ldc, ldc},
                    {P + (long)w * 128 * ldc + (long)w * 128, ldc}, rest, rest, w * 128, 1, 0, -1.0, 1.0, 1), "Sigma update");
  }
  int info = 0;
  HCK(hipMemcpyAsync(&info, info_dev, sizeof(int), hipMemcpyDeviceToHost, st), "info download");
  HCK(hipStreamSynchronize(st), "stream sync");
  if (info != INFO_OK) {
    snprintf(h->err, sizeof(h->err), "mi_gp_sample_cov: Sigma is not positive definite (pivot %d)", info);
    return info;
  }
  // draws: D = Z L_Sigma^T (kmode 4: L_Sigma^T is upper triangular, so the diagonal tiles' strict upper halves must hold zeros)
  HCK(launch_zero_diag_upper(cov_dev, ldc, mt, st), "zero upper");
  HCK(hipMemsetAsync(Z, 0, sizeof(double) * (size_t)sp * mp, st), "Z padding");
  HCK(launch_philox_normals(Z, mp, m, s, seed, offset, st), "normals");
  HCK(gemm_call(h, E, 0, 0, {Z, mp}, {cov_dev, ldc}, {D, mp}, sp / 128, mt, (int)mp, 0, 4, 1.0, 0.0, 1), "Z L^T");
  HCK(launch_draw_epilogue(D, mp, mean_dev, m, s, draws_dev, ldd, st), "draw epilogue");
  HCK(hipStreamSynchronize(st), "stream sync");
  return 0;
}

// ---------------------------------------------------------------- batched conditional
// The posterior predictive over k hyper-parameter draws: k conditional-form factorisations in lockstep (batch_internal, what = 1,
// the kernels of mi_gp_factor with blockIdx.z = problem), then mi_gp_predict's three steps -- cross-covariance, blocked
// triangular solve, reduction -- for all k problems in the same launches.  Problem p's rows are mi_gp_factor(theta_p) +
// mi_gp_predict's bits: same kernels, same per-element arithmetic, and the solve's GEMMs take the single problem's tile form.
extern "C" int mi_gp_factor_batch(mi_gp_handle* h, int k, const double* thetas, int* info_out) {
  if (!h) return -1;
  if (int r = refuse_plain_model(h, "mi_gp_factor_batch")) return r;
  if (k < 1 || !thetas) { snprintf(h->err, sizeof(h->err), "mi_gp_factor_batch: k >= 1 and thetas are required"); return -1; }
  return batch_internal(h, k, thetas, 1, nullptr, nullptr, info_out);
}

extern "C" int mi_gp_predict_batch(mi_gp_handle* h, int k, const double* Xnew_dev, int m, double* work_dev, long ldw,
                                   long stride_work, double* mean_dev, double* var_dev, int pred_noise, double* mix_mean_dev,
                                   double* mix_var_dev) {
  if (!h) return -1;
  if (int r = refuse_plain_model(h, "mi_gp_predict_batch")) return r;
  if (k < 1 || !Xnew_dev || !work_dev || !mean_dev || !var_dev || m <= 0) {
    snprintf(h->err, sizeof(h->err), "mi_gp_predict_batch: k >= 1, m >= 1 and the point / work / output buffers are required");
    return -1;
  }
  if (!mix_mean_dev != !mix_var_dev) {
    snprintf(h->err, sizeof(h->err), "mi_gp_predict_batch: mix_mean_dev and mix_var_dev go together (both or neither)");
    return -1;
  }
  if (h->b_cond_k < 1) {
    snprintf(h->err, sizeof(h->err), "mi_gp_predict_batch: mi_gp_factor_batch must be the last batch call");
    return -1;
  }
  if (k != h->b_cond_k) {
    snprintf(h->err, sizeof(h->err), "mi_gp_predict_batch: %d problems, the last mi_gp_factor_batch factorised %d", k, h->b_cond_k);
    return -1;
  }
  const int mp = (m + 127) / 128 * 128;
  if (ldw < h->np || (ldw & 1)) { snprintf(h->err, sizeof(h->err), "mi_gp_predict_batch: ldw must be even and >= padded n"); return -1; }
  if (stride_work < (long)mp * ldw || (stride_work & 1)) {
    snprintf(h->err, sizeof(h->err), "mi_gp_predict_batch: stride_work must be even and >= ceil(m/128)*128 * ldw = %ld", (long)mp * ldw);
    return -1;
  }
  HCK(hipSetDevice(h->device), "hipSetDevice");
  // mi_gp_predict's steps on the batch's factors, blockIdx.z = problem
  Eval E = batch_eval(h, k);
  E.bt.swork = stride_work;
  Batch bw = E.bt;
  bw.sK = stride_work;  // (the assembly writes the cross-covariance blocks: its output stride is the work blocks')
  HCK(launch_assemble(h->spec, E.s.theta_dev, Xnew_dev, m, h->buf.X_dev, h->n, work_dev, ldw, mp, h->np, 0, 0, h->stream,
                      -2147483647 - 1, nullptr, &bw), "assemble cross");
  HCK(trsm_rec(h, E, work_dev, ldw, mp, 0, h->ntc), "trsm");
  HCK(launch_predict_reduce_batched(h->spec, E.s.theta_dev, work_dev, ldw, E.K + (long)h->np * h->buf.lda, E.s.info_dev, h->n, m,
                                    pred_noise ? 1 : 0, mean_dev, var_dev, h->stream, E.bt), "predict_reduce");
  if (mix_mean_dev)
    HCK(launch_mixture_moments(mean_dev, var_dev, m, k, E.s.info_dev, E.bt.sinfo, mix_mean_dev, mix_var_dev, h->stream), "mixture");
  HCK(hipStreamSynchronize(h->stream), "stream sync");
  return 0;
}

// U = L^-T in Z_dev and alpha = U beta, formed once per mi_gp_factor (mi_gp_predict_u / mi_gp_predict_grad)
int make_u_resident(mi_gp_handle* h) {
  if (h->have_u) return 0;
  HCK(inverse_transpose(h, one_eval(h)), "inverse_transpose");
  HCK(launch_trmv_upper(h->buf.Z_dev, h->buf.lda, h->buf.K_dev + (long)h->np * h->buf.lda, h->n, h->one.alpha_dev, h->stream), "trmv");
  h->have_u = true;
  return 0;
}

// mean / var at m points through U: K(X*, X) rows into the second ceil(m/128)*128 rows of work_dev, A = K(X*, X) U into the
// first -- one triangular-k GEMM, or (per_point) one pass over U per point, A_p = U^T k*_p -- then mi_gp_predict's reduction
static int predict_via_u(mi_gp_handle* h, const double* Xnew_dev, int m, double* work_dev, long ldw, double* mean_dev,
                         double* var_dev, int pred_noise, bool per_point) {
  const long ld = h->buf.lda;
  const int mp = (m + 127) / 128 * 128;
  double* krows = work_dev + (long)mp * ldw;
  HCK(launch_assemble(h->spec, h->one.theta_dev, Xnew_dev, m, h->buf.X_dev, h->n, krows, ldw, mp, h->np, 0, 0, h->stream),
      "assemble cross");
  if (per_point) {
    for (int p = 0; p < m; ++p)
      HCK(launch_trmv_upper_t(h->buf.Z_dev, ld, krows + (long)p * ldw, h->n, work_dev + (long)p * ldw, h->stream), "trmv_t");
  } else {
    HCK(gemm_call(h, one_eval(h), 0, 1, {krows, ldw}, {h->buf.Z_dev, ld}, {work_dev, ldw}, mp / 128, h->ntc, h->np, 0, 4, 1.0, 0.0, 1),
        "K* U");
  }
  HCK(predict_reduce(h, work_dev, ldw, m, mean_dev, var_dev, pred_noise), "predict_reduce");
  return 0;
}

// The same conditional through U = L^-T: A = K(X*, X) U is ONE triangular-k GEMM (k < (tj+1)*128, ~70 TFLOP/s) instead
// of the blocked triangular solve (~250 launches, ~30 TFLOP/s on tall-skinny right-hand sides).  U costs N^3/3 flops
// once per factorisation, so this is the path for sweeps of many points at fixed hyper-parameters (BO's 10 000-point
// proposals, differential-evolution generations).  Needs Z_dev / W_dev; work_dev must hold 2 * ceil(m/128)*128 rows.
extern "C" int mi_gp_predict_u(mi_gp_handle* h, const double* Xnew_dev, int m, double* work_dev, long ldw,
                               double* mean_dev, double* var_dev, int pred_noise) {
  if (!h || !Xnew_dev || !work_dev || !mean_dev || !var_dev || m <= 0) return -1;
  if (int r = refuse_plain_model(h, "mi_gp_predict_u")) return r;
  if (!h->factored) { snprintf(h->err, sizeof(h->err), "mi_gp_predict_u: call mi_gp_factor first"); return -1; }
  if (!h->buf.Z_dev || !h->buf.W_dev) {
    snprintf(h->err, sizeof(h->err), "mi_gp_predict_u needs Z_dev and W_dev in mi_gp_set_data");
    return -1;
  }
  if (ldw < h->np || (ldw & 1)) { snprintf(h->err, sizeof(h->err), "mi_gp_predict_u: ldw must be even and >= padded n"); return -1; }
  HCK(hipSetDevice(h->device), "hipSetDevice");
  if (int r = make_u_resident(h)) return r;
  if (int r = predict_via_u(h, Xnew_dev, m, work_dev, ldw, mean_dev, var_dev, pred_noise, false)) return r;
  HCK(hipStreamSynchronize(h->stream), "stream sync");
  return 0;
}

// Posterior mean / variance at m points AND their gradients w.r.t. the (converted) points: the differentiable
// predictive of BO's refinement (gpmcmc.py:766-801).  Needs Z_dev / W_dev (U = L^-T is formed once per
// mi_gp_factor, N^3/3 flops on the GEMM kernel) and work_dev with 2 * ceil(m/128)*128 rows: the second half
// receives w_p = K^-1 k(X, x*_p) = U (L^-1 k*_p), one row per point.
extern "C" int mi_gp_predict_grad(mi_gp_handle* h, const double* Xnew_dev, int m, double* work_dev, long ldw,
                                  double* mean_dev, double* var_dev, int pred_noise, double* dmean_dev,
                                  double* dvar_dev) {
  if (!h) return -1;
  if (h->npaths) {  // option 54 = S >= 1: the path sweep, work_dev the caller's path block and pred_noise `condition`
    if (h->sweep) {
      snprintf(h->err, sizeof(h->err), "mi_gp_predict_grad: option 53 = 1 (the mean sweep) and option 54 = %d (the path sweep) are both "
               "set: set one of them to 0", h->npaths);
      return -1;
    }
    return path_sweep(h, Xnew_dev, m, work_dev, ldw, mean_dev, pred_noise, dmean_dev);
  }
  if (h->sweep) return mean_sweep(h, Xnew_dev, m, mean_dev, dmean_dev);  // option 53 = 1: another call behind the same entry point
  if (!dmean_dev || !dvar_dev) return -1;
  if (int r = refuse_plain_model(h, "mi_gp_predict_grad")) return r;
  if (!h->buf.Z_dev || !h->buf.W_dev) {
    snprintf(h->err, sizeof(h->err), "mi_gp_predict_grad needs Z_dev and W_dev in mi_gp_set_data");
    return -1;
  }
  if ((size_t)(h->cfg.nkern + 1) * h->cfg.d * sizeof(double) > PREDICT_GRAD_MAX_LDS) {
    snprintf(h->err, sizeof(h->err), "mi_gp_predict_grad: (nkern + 1) * d must fit %d bytes of LDS (d <= %d here)", (int)PREDICT_GRAD_MAX_LDS,
             (int)(PREDICT_GRAD_MAX_LDS / sizeof(double)) / (h->cfg.nkern + 1));
    return -1;
  }
  if (!h->factored) { snprintf(h->err, sizeof(h->err), "mi_gp_predict_grad: call mi_gp_factor first"); return -1; }
  if (!Xnew_dev || !work_dev || !mean_dev || !var_dev || m <= 0) return -1;
  if (ldw < h->np || (ldw & 1)) { snprintf(h->err, sizeof(h->err), "mi_gp_predict_grad: ldw must be even and >= padded n"); return -1; }
  HCK(hipSetDevice(h->device), "hipSetDevice");
  if (int r = make_u_resident(h)) return r;
  // few points (BO refinement): with U resident, A_p = L^-1 k*_p = U^T k*_p is one pass over U per point instead of the
  // ~250-launch blocked triangular solve
  const int r = m <= 16 ? predict_via_u(h, Xnew_dev, m, work_dev, ldw, mean_dev, var_dev, pred_noise, true)
                        : mi_gp_predict(h, Xnew_dev, m, work_dev, ldw, mean_dev, var_dev, pred_noise);
  if (r != 0) return r;
  const long ld = h->buf.lda;
  const int mp = (m + 127) / 128 * 128;
  double* wrows = work_dev + (long)mp * ldw;  // (over predict_via_u's K(X*, X) rows)
  for (int p = 0; p < m; ++p)
    HCK(launch_trmv_upper(h->buf.Z_dev, ld, work_dev + (long)p * ldw, h->n, wrows + (long)p * ldw, h->stream), "trmv w");
  HCK(launch_predict_grad(h->spec, h->one.theta_dev, h->buf.X_dev, h->n, Xnew_dev, m, h->one.alpha_dev, wrows, ldw, dmean_dev,
                          dvar_dev, h->stream), "predict_grad");
  HCK(hipStreamSynchronize(h->stream), "stream sync");
  return 0;
}

// ---------------------------------------------------------------- appending points at fixed theta
// The handle's n-dependent scratch for up to `capacity` points; the resident contents (leaf inverses, alpha) are kept.
extern "C" int mi_gp_reserve(mi_gp_handle* h, int capacity) {
  if (!h) { set_global_error("mi_gp_reserve: null handle"); return -1; }
  if (int r = refuse_deriv(h, "mi_gp_reserve")) return r;
  if (capacity < h->n) { snprintf(h->err, sizeof(h->err), "mi_gp_reserve: capacity %d < n = %d", capacity, h->n); return -1; }
  const int cap_np = (capacity + 127) / 128 * 128;
  if (h->have_data && h->buf.lda < cap_np) {
    snprintf(h->err, sizeof(h->err), "mi_gp_reserve: lda %ld of mi_gp_set_data < padded capacity %d", h->buf.lda, cap_np);
    return -1;
  }
  if (capacity <= h->cap) return 0;
  HCK(hipSetDevice(h->device), "hipSetDevice");
  HCK(hipStreamSynchronize(h->stream), "stream sync");
  // (the single scratch's point-dependent arrays, as alloc_scratch sizes them; the rest does not depend on n)
  const Batch z = scratch_strides(h, capacity);
  Scratch& s = h->one;
  double *dinv = nullptr, *alpha = nullptr, *part = nullptr;
  hipError_t e = hipMalloc(&dinv, sizeof(double) * z.sdinv);
  if (e == hipSuccess) e = hipMalloc(&alpha, sizeof(double) * z.salpha);
  if (e == hipSuccess) e = hipMalloc(&part, sizeof(double) * z.spart);
  if (e == hipSuccess) e = hipMemcpy(dinv, s.dinv_dev, sizeof(double) * MINV_ELEMS * (size_t)h->ntc, hipMemcpyDeviceToDevice);
  if (e == hipSuccess) e = hipMemcpy(alpha, s.alpha_dev, sizeof(double) * h->np, hipMemcpyDeviceToDevice);
  if (e != hipSuccess) {
    (void)hipFree(dinv); (void)hipFree(alpha); (void)hipFree(part);
    return hfail(h, e, "mi_gp_reserve");
  }
  (void)hipFree(s.dinv_dev); (void)hipFree(s.alpha_dev); (void)hipFree(s.part_dev);
  s.dinv_dev = dinv; s.alpha_dev = alpha; s.part_dev = part;
  h->cap = capacity;
  // the modes' blocks: those that hold nothing between calls are dropped (their next use allocates them again), the trend's
  // keeps the conditional's G^T, beta^ and b~, the outputs' its B^T
  for (int id = 0; id < BLK_COUNT; ++id)
    if (!block_keeps_state(id)) drop_block(h->blocks[id]);
  static_assert(block_keeps_state(BLK_TREND) && block_keeps_state(BLK_MULTI) && [] {
    int kept = 0;
    for (int id = 0; id < BLK_COUNT; ++id) kept += block_keeps_state(id);
    return kept;
  }() == 2, "every block that block_keeps_state() names needs its reserve function called here");
  if (h->blocks[BLK_TREND].p && trend_reserve) HCK(trend_reserve(h, capacity), "mi_gp_reserve");
  if (h->blocks[BLK_MULTI].p && multi_reserve) HCK(multi_reserve(h, capacity), "mi_gp_reserve");
  return 0;
}

// The k-segmented 128 x 128 Gram product (gp_handle.h).  Segment g of an operand starts g * seg * 128 columns of k in: that many
// doubles along a row of A (and of B under bk = 0), that many rows of 128 doubles of B under bk = 1.
hipError_t gram_segments(mi_gp_handle* h, const Eval& E, In A, In B, int bk, double* parts, int* nparts) {
  const int ntc = h->ntc, seg = (ntc + 63) / 64, nfull = ntc / seg, rem = ntc - nfull * seg;
  const long ka = seg * 128L, kb = bk ? ka * 128 : ka;
  *nparts = nfull + (rem > 0 ? 1 : 0);
  hipError_t e = gemm_call(h, E, 0, bk, {A.p, A.ld, ka}, {B.p, B.ld, kb}, {parts, 128, MINV_ELEMS}, 1, 1, seg * 128, 0, 0, 1.0, 0.0, nfull);
  if (e == hipSuccess && rem > 0)
    e = gemm_call(h, E, 0, bk, {A.p + nfull * ka, A.ld}, {B.p + nfull * kb, B.ld}, {parts + (long)nfull * MINV_ELEMS, 128}, 1, 1, rem * 128,
                  0, 0, 1.0, 0.0, 1);
  return e;
}

// Phase 1 of mi_gp_append, shared with mi_gp_logpdf (api_logpdf.hip): the conditional of k new points given the resident
// factor, in the caller's work block alone -- L21 = K21 L11^-T (one GEMM against U when it is resident, else the blocked
// solve), S = K22 + noise - L21 L21^T and its factor L22 in the S block, beta2 = L22^-1 (y2 - L21 beta1) in row 128 of that
// block -- then stats = {sum log diag L22, |beta2|^2, the bad-pivot word} on the host.  Of the handle it uses info_dev and the
// stats scratch; the stream is idle when it returns.
// work_dev layout (R = 128 * ldw doubles): [0, R) L21, [R, 2R) K21 (U route), [2R, 4R) the k-segmented partial products of
// L21 L21^T, then the S block (2 * 16384), S's leaf inverse (16384) and room for L22^-1 row-major (16384).
int conditional_block(mi_gp_handle* h, const double* Xnew_dev, const double* ynew_dev, const double* diag_new_dev, int k,
                      double* work_dev, long ldw, double stats[3]) {
  const int n = h->n, np = h->np, ntc = h->ntc;
  const long ld = h->buf.lda;
  if (!h->app_stats_dev) HCK(hipMalloc(&h->app_stats_dev, sizeof(double) * 4), "append scratch");
  const long R = 128L * ldw;
  double *L21 = work_dev, *W1 = work_dev + R, *parts = work_dev + 2 * R, *S = work_dev + 4 * R;
  double* Sinv = S + 2 * MINV_ELEMS;
  const hipStream_t st = h->stream;
  const double* beta1 = h->buf.K_dev + (long)np * ld;
  const Eval E = one_eval(h);
  if (h->have_u) {  // L21 = K21 U11: one GEMM against the resident inverse (mi_gp_predict_u's route)
    HCK(launch_assemble(h->spec, h->one.theta_dev, Xnew_dev, k, h->buf.X_dev, n, W1, ldw, 128, np, 0, 0, st), "assemble K21");
    HCK(gemm_call(h, E, 0, 1, {W1, ldw}, {h->buf.Z_dev, ld}, {L21, ldw}, 1, ntc, np, 0, 4, 1.0, 0.0, 1), "K21 U11");
  } else {
    HCK(launch_assemble(h->spec, h->one.theta_dev, Xnew_dev, k, h->buf.X_dev, n, L21, ldw, 128, np, 0, 0, st), "assemble K21");
    HCK(trsm_rec(h, E, L21, ldw, 128, 0, ntc), "trsm L21");
  }
  int nparts = 0;
  HCK(gram_segments(h, E, {L21, ldw}, {L21, ldw}, 0, parts, &nparts), "L21 L21^T segments");
  HCK(hipMemsetAsync(S, 0, sizeof(double) * 2 * MINV_ELEMS, st), "S clear");
  HCK(launch_assemble(h->spec, h->one.theta_dev, Xnew_dev, k, Xnew_dev, k, S, 128, 128, 128, 1, 1, st, -2147483647 - 1, diag_new_dev),
      "assemble K22");
  HCK(launch_append_schur(S, parts, nparts, L21, ldw, beta1, np, ynew_dev, k, st), "schur");
  HCK(hipMemsetAsync(h->one.info_dev, 0x7f, sizeof(int), st), "info reset");
  HCK(launch_potrf_leaf128(S, 128, Sinv, n, h->one.info_dev, st, S + MINV_ELEMS), "leaf S");
  HCK(launch_append_stats(S, k, h->one.info_dev, h->app_stats_dev, st), "append stats");
  HCK(hipMemcpyAsync(stats, h->app_stats_dev, sizeof(double) * 3, hipMemcpyDeviceToHost, st), "stats download");
  HCK(hipStreamSynchronize(st), "stream sync");
  return 0;
}

// Conditional-form factor of n points -> n + k points at the same theta (Schur complement of the appended block):
//   L21 = K21 L11^-T, S = K22 + noise - L21 L21^T = L22 L22^T, beta2 = L22^-1 (y2 - L21 beta1),
//   logdet += sum log diag L22, quad += |beta2|^2; with U resident U12 = -U11 L21^T U22, U22 = L22^-T, alpha = U beta.
// Everything up to the factor of S runs in the caller's work block (conditional_block()): a non-positive-definite S leaves the
// handle untouched.  The commit reuses that block: [0, R) L21 becomes -L22^-1 L21 U11^T, [R, 2R) becomes L21 U11^T.
extern "C" int mi_gp_append(mi_gp_handle* h, const double* Xnew_dev, const double* ynew_dev, const double* diag_new_dev, int k,
                            double* work_dev, long ldw) {
  if (!h) { set_global_error("mi_gp_append: null handle"); return -1; }
  if (int r = refuse_plain_model(h, "mi_gp_append")) return r;
  if (!Xnew_dev || !ynew_dev || !work_dev) { snprintf(h->err, sizeof(h->err), "mi_gp_append: null point, value or work buffer"); return -1; }
  if (k < 1 || k > 128) { snprintf(h->err, sizeof(h->err), "mi_gp_append: 1 <= k <= 128 (got %d)", k); return -1; }
  if (!h->factored) { snprintf(h->err, sizeof(h->err), "mi_gp_append: call mi_gp_factor first"); return -1; }
  if (h->n + k > h->cap) {
    snprintf(h->err, sizeof(h->err), "mi_gp_append: n + k = %d exceeds the capacity %d (mi_gp_reserve)", h->n + k, h->cap);
    return -1;
  }
  if (!diag_new_dev != !h->diag_dev) {
    snprintf(h->err, sizeof(h->err), "mi_gp_append: diag_new_dev must be given exactly when a diagonal is set (mi_gp_set_diag)");
    return -1;
  }
  const int n = h->n, n2 = n + k;
  const int np = h->np, ntc = h->ntc, np2 = (n2 + 127) / 128 * 128;
  const long ld = h->buf.lda;
  if (ldw < np2 || (ldw & 1)) { snprintf(h->err, sizeof(h->err), "mi_gp_append: ldw must be even and >= padded(n + k) = %d", np2); return -1; }
  if (ld < np2) { snprintf(h->err, sizeof(h->err), "mi_gp_append: lda of mi_gp_set_data < padded(n + k) = %d", np2); return -1; }
  HCK(hipSetDevice(h->device), "hipSetDevice");
  const long R = 128L * ldw;
  double *L21 = work_dev, *W1 = work_dev + R, *S = work_dev + 4 * R;
  double* Linv22 = S + 3 * MINV_ELEMS;
  const hipStream_t st = h->stream;
  const Eval E = one_eval(h);
  // ---- phase 1: scratch only
  double stats[3];
  if (int r = conditional_block(h, Xnew_dev, ynew_dev, diag_new_dev, k, work_dev, ldw, stats)) return r;
  const int info = (int)stats[2];
  if (info != INFO_OK) {
    snprintf(h->err, sizeof(h->err), "mi_gp_append: the appended block is not positive definite (pivot %d); the handle is unchanged", info);
    return info;
  }
  // ---- phase 2: commit
  HCK(hipMemcpyAsync(const_cast<double*>(h->buf.X_dev) + (long)n * h->cfg.d, Xnew_dev, sizeof(double) * k * h->cfg.d,
                     hipMemcpyDeviceToDevice, st), "X rows");
  HCK(hipMemcpyAsync(const_cast<double*>(h->buf.y_dev) + n, ynew_dev, sizeof(double) * k, hipMemcpyDeviceToDevice, st), "y rows");
  if (h->diag_dev)
    HCK(hipMemcpyAsync(const_cast<double*>(h->diag_dev) + n, diag_new_dev, sizeof(double) * k, hipMemcpyDeviceToDevice, st), "diag rows");
  if (h->have_u)  // P = L21 U11^T (U11 upper: k >= column tile), read before U grows
    HCK(gemm_call(h, E, 0, 0, {L21, ldw}, {h->buf.Z_dev, ld}, {W1, ldw}, 1, ntc, np, 0, 1, 1.0, 0.0, 1), "L21 U11^T");
  HCK(launch_append_commit(h->buf.K_dev, ld, n, k, np, np2, L21, ldw, S, st), "commit rows");
  const int t0 = n / 128, t1 = (n2 - 1) / 128;
  HCK(launch_tile_inverse_rows(h->buf.K_dev + (long)t0 * 128 * (ld + 1), ld, 128 * (ld + 1), h->one.dinv_dev + (size_t)t0 * MINV_ELEMS,
                               MINV_ELEMS, n - t0 * 128, t1 - t0 + 1, 0, st), "leaf inverses");
  if (h->have_u) {
    HCK(launch_tile_inverse_rows(S, 128, 0, Linv22, 0, 0, 1, 1, st), "L22 inverse");
    HCK(gemm_call(h, E, 0, 1, {Linv22, 128}, {W1, ldw}, {L21, ldw}, 1, ntc, 128, 0, 0, -1.0, 0.0, 1), "U12^T");
    HCK(launch_append_u(h->buf.Z_dev, ld, n, k, np, np2, L21, ldw, Linv22, st), "U columns");
    HCK(launch_trmv_upper(h->buf.Z_dev, ld, h->buf.K_dev + (long)np2 * ld, n2, h->one.alpha_dev, st), "trmv");
  }
  HCK(hipStreamSynchronize(st), "stream sync");
  h->n = n2;
  h->np = np2;
  h->ntc = np2 / 128;
  h->one.out_host[1] += stats[0];
  h->one.out_host[2] += stats[1];
  h->one.out_host[0] = -0.5 * (double)n2 * LOG_2PI - 0.5 * h->one.out_host[2] - h->one.out_host[1];
  h->have_kinv = false;
  // the caller's batch buffers were sized for the old n: every batch call is refused until mi_gp_set_batch (which re-sizes the
  // batch scratch for the new n)
  h->b_cond_k = 0;
  h->bbuf = mi_gp_batch_buffers();
  free_scratch(h->batch);
  return 0;
}
