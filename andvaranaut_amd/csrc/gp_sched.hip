// The scheduler of the handle-level evaluations (api_gp.hip): which launch goes to which stream behind which cross-stream edge.
#include "gp_handle.h"

// ---------------------------------------------------------------- driver pieces
static hipError_t prof_gemm(mi_gp_handle* h, const Eval& E, const GemmParams& p, int ak, int bk, int batch, double flops,
                            hipStream_t st) {
  if (E.prof >= 2) {
    // one event pair per kernel launch: a split product (gemm_tail_tiles) is two launches, its flops divided by tiles;
    // `flops` are those of the WHOLE product, a sub-range launch (p.tile0 / p.tile_cnt) is credited its share of tiles
    const int tail = gemm_tail_tiles(p, batch);
    const int tiles = p.tri ? p.nt * (p.nt + 1) / 2 + (p.mt - p.nt) * p.nt : p.mt * p.nt;
    const int t0 = p.tile0, t1 = p.tile_cnt > 0 ? (t0 + p.tile_cnt < tiles ? t0 + p.tile_cnt : tiles) : tiles;
    const int big_end = t1 < tiles - tail ? t1 : tiles - tail;
    hipError_t r = hipSuccess;
    for (int part = 1; part <= 2 && r == hipSuccess; ++part) {
      const int mine = part == 1 ? (gemm_uses_small_tiles(p, batch) ? (t0 == 0 ? tiles : 0) : big_end - t0)
                                 : ((tail > 0 && t1 == tiles) ? tail : 0);
      if (mine <= 0) continue;
      if (h->gemm_ev_used + 2 > h->gemm_ev.size()) {
        for (int i = 0; i < 64; ++i) {
          hipEvent_t e;
          r = hipEventCreate(&e);
          if (r != hipSuccess) return r;
          h->gemm_ev.push_back(e);
        }
      }
      (void)hipEventRecord(h->gemm_ev[h->gemm_ev_used], st);
      r = launch_gemm_f64(p, ak, bk, batch, st, part);
      (void)hipEventRecord(h->gemm_ev[h->gemm_ev_used + 1], st);
      const size_t pair = h->gemm_ev_used / 2;
      if (h->gemm_ev_big.size() <= pair) { h->gemm_ev_big.resize(pair + 64); h->gemm_ev_flops.resize(pair + 64); }
      h->gemm_ev_big[pair] = (part == 1 && !gemm_uses_small_tiles(p, batch)) ? 1 : 0;
      h->gemm_ev_flops[pair] = flops * (double)mine / (double)tiles;
      h->gemm_flops_acc += flops * (double)mine / (double)tiles;
      h->gemm_ev_used += 2;
    }
    return r;
  }
  return launch_gemm_f64(p, ak, bk, batch, st);
}

// ---------------------------------------------------------------- cross-stream edges
// The only functions that tell an edge's forms apart (option 26: 0 events, 1 runtime stream memory operations, 2 the panel
// stream's halves folded into kernels, which take edge_ptr()).
static hipError_t next_event(mi_gp_handle* h, Sched& S, hipEvent_t* out) {
  if (S.ev_next == h->ev_pool.size()) {
    hipEvent_t ev;
    hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (e != hipSuccess) return e;
    h->ev_pool.push_back(ev);
  }
  *out = h->ev_pool[S.ev_next++];
  return hipSuccess;
}

// a fresh slot that a KERNEL will write or poll (the caller has checked that one is left: that decides its launches)
static Edge edge_reserve(Sched& S) { return Edge{S.sig_next++}; }

// what a launcher that folds the write or the poll into a kernel takes: the slot's address, nullptr for an event or no edge
static unsigned* edge_ptr(const mi_gp_handle* h, const Edge& g) { return g.slot >= 0 ? h->sig_dev + g.slot : nullptr; }

// `from` raises a reserved slot behind everything queued on it so far
static hipError_t edge_write(mi_gp_handle* h, const Edge& g, hipStream_t from) {
  return hipStreamWriteValue32(from, h->sig_dev + g.slot, h->sig_epoch, 0);
}

// everything queued on `from` so far, as a fresh edge: a slot where the caller's protocol uses them (`slots`) and one is left,
// otherwise an event
static hipError_t edge_signal(mi_gp_handle* h, Sched& S, hipStream_t from, bool slots, Edge* g) {
  *g = Edge();
  if (slots && S.sig_next < SIG_SLOTS) {
    *g = edge_reserve(S);
    return edge_write(h, *g, from);
  }
  hipError_t e = next_event(h, S, &g->ev);
  return e != hipSuccess ? e : hipEventRecord(g->ev, from);
}

// `to` waits for an edge
static hipError_t edge_wait(mi_gp_handle* h, const Edge& g, hipStream_t to) {
  return g.slot >= 0 ? hipStreamWaitValue32(to, h->sig_dev + g.slot, h->sig_epoch, hipStreamWaitValueGte, 0xffffffffu)
                     : hipStreamWaitEvent(to, g.ev, 0);
}

// `to` waits for everything queued on `from` so far
static hipError_t hand_off(mi_gp_handle* h, Sched& S, hipStream_t from, hipStream_t to) {
  Edge g;
  hipError_t e = edge_signal(h, S, from, h->use_smo != 0, &g);
  return e != hipSuccess ? e : edge_wait(h, g, to);
}

// the edge armed for the leaf of tile column c0, if any: taken and disarmed (chol_panel's leaf is the one consume point)
static bool take_armed(Sched::Armed& a, int c0, Edge* g) {
  if (a.col != c0) return false;
  *g = a.edge;
  a = Sched::Armed();
  return true;
}

// trapezoid update  A[r0:, c0:c0+nc] -= P P_c^T  with P = A[r0:, k0:k0+kw] (tile units)
// In-panel updates only (their shapes do not depend on the schedule), by SHAPE alone -- not the batch size, not a scheduling
// option: a batch returns the single evaluation's bits, and so does every schedule.
constexpr int THIN_MAX_COLS = 2;  // (the strip in front of such an update hands it its B operand in operand order: 2 x 128 rows)
static bool thin_shape(const mi_gp_handle* h, int mt, int nc, int kw) {
  return h->thin_max_wg > 0 && nc <= THIN_MAX_COLS && kw == 1 && (long)mt * 8 * nc <= h->thin_max_wg;
}

// How a trapezoid update is launched (its geometry and stream are syrk_trapezoid's own parameters); filled by name
struct TrapLaunch {
  int one_per_cu = 0;           // GemmParams: one workgroup per CU,
  int tile0 = 0, tile_cnt = 0;  // a sub-range of the tile enumeration,
  int fc = 0;                   // the first fc tile columns enumerated first,
  int kflush = 0;               // a k-segmented update
  bool in_panel = false;        // an in-panel update (the only ones that may take the thin kernel and raise an edge)
  bool lsw = false;             // the strip in front of this update has written its first rows in operand order -- chol_panel
                                // decides both by the same rule
  Edge raise;                   // in-panel updates only: raised once everything queued on the stream before this update is done
};

static hipError_t syrk_trapezoid(mi_gp_handle* h, const Eval& E, double* A, long lda, int ntr, int r0, int nc, int k0, int kw,
                                 hipStream_t st, const TrapLaunch& o = TrapLaunch()) {
  unsigned* wr = edge_ptr(h, o.raise);
  if (o.in_panel && o.lsw && thin_shape(h, ntr - r0, nc, kw))
    return launch_syrk_thin(A + (long)r0 * 128 * lda + (long)k0 * 128, A + (long)r0 * 128 * lda + (long)r0 * 128, lda, ntr - r0, nc,
                            kw * 128, st, E.lb(), wr, h->sig_epoch, E.s.dinv_dev + (size_t)h->ntc * MINV_ELEMS);
  if (wr != nullptr) {  // (the 64x64-tile kernel has no such hook: a one-lane launch in front of it)
    hipError_t we = launch_signal_write_wait(wr, nullptr, h->sig_epoch, E.s.info_dev, st);
    if (we != hipSuccess) return we;
  }
  GemmParams p;
  p.one_per_cu = o.one_per_cu;
  p.tile0 = o.tile0;
  p.tile_cnt = o.tile_cnt;
  p.fc = o.fc;
  p.hiprio = (st == h->pstream && h->chain_prio) ? 1 : 0;
  p.small_below = h->small_below;
  p.tail_small = h->tail_small;
  p.band = h->band_rows;
  p.A = A + (long)r0 * 128 * lda + (long)k0 * 128;
  p.B = p.A;
  p.C = A + (long)r0 * 128 * lda + (long)r0 * 128;
  p.lda = p.ldb = p.ldc = lda;
  p.strideA = p.strideB = p.strideC = E.bt.sK;
  p.mt = ntr - r0;
  p.nt = nc;
  p.k = kw * 128;
  p.tri = 1;
  p.kmode = 0;
  p.alpha = -1.0;
  p.beta = 1.0;
  p.kflush = o.kflush;
  p.dead_last_half = 1;  // (every trapezoid of the factorisation ends in the y^T tile row)
  // algorithmic flops (nb*m^2 for the lower-triangle SYRK, 2*nb*rows*cols for the block
  // below it, one y^T row for the folded-in forward solve); the MFMA work issued is slightly larger
  // (full diagonal tiles, a 128-row tile for the y row).
  const double c = nc * 128.0, rows_real = (p.mt - 1) * 128.0;
  const double flops = (double)p.k * (c * (c + 1.0) + 2.0 * (rows_real - c) * c + 2.0 * c);
  return prof_gemm(h, E, p, 0, 0, E.bt.nb, flops, st);
}

// factor tile columns [c0, c0+w) of the (ntr x ntc)-tile trapezoid, recursively halving w; nx (0 / 1): every level's update
// also covers the nx tile columns behind the panel, so that they are up to date when the panel's last strip is.
// follow: number of tile columns of the k = 128 update that the CALLER runs right behind this (one-column) panel's strip
static hipError_t chol_panel(mi_gp_handle* h, const Eval& E, Sched& S, double* A, long lda, int ntr, int c0, int w, hipStream_t st, int nx = 0,
                             int follow = 0) {
  hipError_t e;
  if (w == 1) {
    // the update behind this column's strip is a k = 128 one over `fol` columns: on the thin kernel the strip hands it its
    // B operand (the first fol x 128 rows of the strip) in operand order
    const int fol = nx > 0 ? nx : follow;
    const bool sw = fol > 0 && fol <= 2 && thin_shape(h, ntr - c0 - 1, fol, 1);
    double* lsw = E.s.dinv_dev + (size_t)h->ntc * MINV_ELEMS;
    double* blk = A + (long)c0 * 128 * lda + (long)c0 * 128;
    double* dinv = E.s.dinv_dev + (size_t)c0 * MINV_ELEMS;
    const int m = (ntr - c0 - 1) * 128;
    // (the trapezoid's last tile row is the y^T block: below the last tile column there is nothing else, and the leaf
    // solves that one row itself)
    // the super-panel's other columns are being updated on the main stream ((a2)); their first reader is the in-panel update
    // behind this column's strip.  Option 26 = 2: this leaf polls for that update's signal before it ends (it is done by
    // then as a rule: it started with (a1)); otherwise a runtime wait behind the strip.
    Edge wait, wait2;
    const bool waits = take_armed(S.wait, c0, &wait);
    // the other edge a leaf may carry: everything the main stream had queued before this panel's chain (wait2; see cholesky()).
    // That slot is written behind the (a2) signal, so where both fall on one leaf it stands for both.  (Armed with option
    // 26 = 2 only, and always as a slot: ext_edges.)
    const bool waits2 = take_armed(S.wait2, c0, &wait2);
    const bool folded = waits2 || (waits && wait.slot >= 0 && h->use_smo >= 2);
    e = launch_potrf_leaf128(blk, lda, dinv, c0 * 128, E.s.info_dev, st, m == 128 ? blk + 128 * lda : nullptr, E.lb(),
                             waits2 ? edge_ptr(h, wait2) : folded ? edge_ptr(h, wait) : nullptr, h->sig_epoch, h->poll_limit_log2);
    if (e == hipSuccess && m > 128)
      e = launch_trsm_strip128(dinv, blk + 128 * lda, lda, m, st, E.lb(), E.bt.sK, sw ? lsw : nullptr, 8 * fol);
    if (e == hipSuccess && waits && !folded) e = edge_wait(h, wait, st);
    if (e == hipSuccess && nx > 0) {
      TrapLaunch o;
      o.in_panel = true;
      o.lsw = sw;
      take_armed(S.done, c0, &o.raise);
      e = syrk_trapezoid(h, E, A, lda, ntr, c0 + 1, nx, c0, 1, st, o);
    }
    return e;
  }
  const int w1 = w / 2, w2 = w - w1;
  e = chol_panel(h, E, S, A, lda, ntr, c0, w1, st, 0, w1 == 1 ? w2 + nx : 0);
  if (e != hipSuccess) return e;
  TrapLaunch o;
  o.in_panel = true;
  o.lsw = w1 == 1 && w2 + nx <= 2 && thin_shape(h, ntr - c0 - w1, w2 + nx, 1);
  e = syrk_trapezoid(h, E, A, lda, ntr, c0 + w1, w2 + nx, c0, w1, st, o);
  if (e != hipSuccess) return e;
  return chol_panel(h, E, S, A, lda, ntr, c0 + w1, w2, st, nx);
}

// Right-looking blocked Cholesky of the (ntr x ntc)-tile lower trapezoid with one super-panel of
// look-ahead: while the trailing update of super-panel J runs on the main stream, the next
// super-panel (whose columns were updated first) is factored on the high-priority panel stream.
// super-panel width (128-column tiles) for a trailing matrix of `rem` tile columns: wide panels while
// the trailing update is long enough to hide their factorisation (k = 1024 runs the GEMM at ~64
// TFLOP/s instead of ~57 at k = 512), narrower ones once the panel chain is the critical path
// Super-panel width in tiles for `rem` remaining tile columns.  `cap` (0: none) limits the size-derived width: the
// two-stream driver factors problems of up to 64 tile columns in 4-tile super-panels (8 vs 4, interleaved A/B at the end
// of round 2: N = 4608 2.510 vs 2.475 ms, 5120 2.840 vs 2.725, 6144 3.602 vs 3.504, 7168 4.628 vs 4.538, 8192 5.742 vs
// 5.678; 9216 equal, 10240 9.05 vs 9.14, 16384 27.4 vs 28.8 -- and 4-tile panels only for the last 52 / 64 columns of
// larger problems lose 1-2 %).  An explicit panel_tiles (option 2) overrides everything.
constexpr int NARROW_PANELS_MAX_TILES = 60;  // (64 until the end of round 4: with the cheaper cross-stream edges N = 8192 runs 5.41 vs 5.33 ms
                                           // on 4- vs 8-tile panels; 7168: 4.16 vs 4.18, 6144: 3.16 vs 3.26, 4096: 1.94 vs 2.01)
static int pick_w(const mi_gp_handle* h, int rem, int cap) {
  int W = h->cfg.panel_tiles;
  if (W <= 0) {
    W = (rem > h->w_thr[0]) ? 16 : (rem > h->w_thr[1]) ? 8 : (rem > h->w_thr[2]) ? 4 : 2;
    if (cap > 0 && W > cap) W = cap;
  }
  return rem < W ? rem : W;
}

// Below this many tile columns one stream is faster than two: the cross-stream hand-offs cost more than the overlap
// returns (one stream vs two, end of round 2: N = 2048 0.94 vs 1.01 ms, N = 4096 2.235 vs 2.252, N = 4608 2.513 vs 2.472,
// N = 5120 2.849 vs 2.820, N = 6144 3.81 vs 3.59, N = 8192 6.35 vs 5.67).
constexpr int LOOKAHEAD_MIN_TILES = 20;  // round 4: with the single-stream tail (option 21) two streams won from 28 tile columns on
                                       // (N = 3584 1.735 -> 1.670 ms, 4096 2.099 -> 2.054); with the hand-offs as stream memory
                                       // operations (option 26) from 20 (one stream vs two: N = 2048 0.875 vs 0.908 ms, 2304 1.026 vs
                                       // 1.022, 2560 1.145 vs 1.119, 2816 1.268 vs 1.251, 3072 1.373 vs 1.352, 3328 1.532 vs 1.484,
                                       // 3584 1.736 vs 1.606)

// ... and from COLUMN_MODE_MIN_TILES on when the whole problem runs in column mode (round 5: three launches per column on the
// panel stream, the rest on the main stream: one stream vs two at N = 1024 0.348 vs 0.336 ms, 1536 0.512 vs 0.475, 2048 0.665 vs
// 0.619; in panel mode two streams still lose there: N = 2048 0.665 vs 0.699).  Round 6: with the evaluation STARTING on the
// panel stream (option 45: no hand-off ahead of the first leaf) two streams win from 4 tile columns on (one stream vs two:
// N = 384 0.124 vs 0.124 ms, 512 0.168 vs 0.158, 640 0.211 vs 0.195, 768 0.258 vs 0.236, 896 0.305 vs 0.273); it was 8.
constexpr int COLUMN_MODE_MIN_TILES = 4;
// Column mode for the WHOLE problem: up to rl_cols tile columns by the tail rule itself, and (round 6, option 46) up to rl_whole = 31:
// for 25 .. 31 tile columns a first panel of 1 .. 7 columns with its entry stall costs more than the main stream's lag behind
// the chain in the first columns (24 / 31: N = 3200 0.994 -> 0.946 ms, 3456 1.101 -> 1.059, 3584 1.156 -> 1.141, 3840 1.234 -> 1.209,
// 3968 1.292 -> 1.267; batches of 8 -1.7 .. -3.3 %).  At 32 columns it turns: N = 4096 1.416 -> 1.454 (a batch of 8 would still
// gain 2.7 %, but the rule is one of the shape alone, and the single evaluation decides it).
static bool whole_columns(const mi_gp_handle* h, int ntc) {
  return h->rl_cols > 0 && (ntc <= h->rl_cols || ntc <= h->rl_whole);
}

static hipError_t u_levels(mi_gp_handle* h, const Eval& E, Sched& S, int final_cols, int max_s);

// COLUMN MODE (round 5, option 37): tile columns [cs, ntc) one by one.  The chain-bound end of a factorisation -- and all of
// a small one -- pays a fixed ~5-8 us per launch on the panel stream, so the fewest, shortest launches per column win: leaf,
// strip, and ONE thin update of the next column by the two columns before it (k = 256, both B operands from the strips'
// operand-order copies); everything older reaches a column through the main stream, which applies column p to the columns
// from p + 3 on (k = 128, 64x64 tiles) a column behind the chain:
//   panel stream:  leaf j [start: S_j -- strips <= j-1 are done | end: polls T_(j-2)]  strip j  thin(col j+1 <- cols j-1, j)
//   main stream:   wait S_j   update(cols >= j+2 <- col j-1)   signal T_(j-1)
// The main stream's update starts when leaf j HAS its CU (it would otherwise fill the chip in front of it) and has until the
// end of leaf j+1 -- ~58 us for ~20.  Which kernel updates a tile with which k is a matter of the column alone (not of the
// streams: on one stream the same launches run in program order), so every schedule returns the same bits.
// t_pending: something queued on the main stream writes columns > cs (the previous super-panel's update): leaf cs polls for it.
static hipError_t chol_columns(mi_gp_handle* h, const Eval& E, Sched& S, double* A, long lda, int ntr, int ntc, int cs, hipStream_t T,
                               hipStream_t P, bool t_pending) {
  hipError_t e = hipSuccess;
#define CKC(x) do { e = (x); if (e != hipSuccess) return e; } while (0)
  const bool two = P != T;
  const bool smo = two && h->use_smo >= 2;
  Edge tedge[3];  // tedge[p % 3]: the edge behind the main stream's update by column p (or the entry update)
  auto t_signal = [&](int idx) { return edge_signal(h, S, T, smo, &tedge[idx]); };
  double* lsw0 = E.s.dinv_dev + (size_t)h->ntc * MINV_ELEMS;
  const int group = E.bt.nb > 1 ? h->rl_group : 1;
  int seg0 = cs;  // grouped schedule: first column (k-segment) the columns behind the chain's next one have not had yet
  if (two && t_pending) CKC(t_signal((cs + 1) % 3));  // polled by leaf cs: the index leaf j polls is (j - 2) mod 3 = (j + 1) mod 3
  for (int j = cs; j < ntc; ++j) {
    double* blk = A + (long)j * 128 * lda + (long)j * 128;
    double* dinv = E.s.dinv_dev + (size_t)j * MINV_ELEMS;
    const int m = (ntr - j - 1) * 128;
    // (the thin update of column c reads the strips of columns c - 2 and c - 1: a strip writes its operand-order copy when the
    // NEXT column's update is a thin one as well -- the limit is monotone in the column, so that covers this column's)
    auto thin_at = [&](int c) { return h->thin_max_wg > 0 && (long)(ntr - c - 1) * 8 <= h->thin_max_wg; };
    const bool thin_ok = thin_at(j);
    const bool lsw_out = thin_ok || (j + 2 < ntc && thin_at(j + 1));
    double* lswj = lsw0 + (size_t)(2 * (j & 1)) * MINV_ELEMS;
    // main stream's work of this step: column j - 1 (final since strip j - 1) updates the columns from j + 2 on
    const bool t_work = j - 1 >= cs && j + 2 < ntc;
    const int pidx = (j + 1) % 3;  // = (j - 2) mod 3
    const Edge poll = tedge[pidx];  // (armed on two streams only: the leaf polls a slot, an event is waited for behind the strip)
    tedge[pidx] = Edge();
    Edge start;  // the leaf raises it as it starts: the main stream's go-ahead for this step's update
    if (two && t_work) {
      if (smo && S.sig_next < SIG_SLOTS) start = edge_reserve(S);
      else CKC(hand_off(h, S, P, T));  // (behind the previous step's thin update: strip j - 1 is done)
    }
    CKC(launch_potrf_leaf128(blk, lda, dinv, j * 128, E.s.info_dev, P, m == 128 ? blk + 128 * lda : nullptr, E.lb(),
                             edge_ptr(h, poll), h->sig_epoch, h->poll_limit_log2, edge_ptr(h, start)));
    if (m > 128) CKC(launch_trsm_strip128(dinv, blk + 128 * lda, lda, m, P, E.lb(), E.bt.sK, lsw_out ? lswj : nullptr, 16));
    if (poll.ev) CKC(edge_wait(h, poll, P));
    if (j + 1 < ntc) {
      // the next column <- this one and (from the second column of the mode on) the one before it
      const bool k2 = j - 1 >= cs;
      const int k0 = k2 ? j - 1 : j, kw = k2 ? 2 : 1, mt = ntr - j - 1;
      double* Pp = A + (long)(j + 1) * 128 * lda + (long)k0 * 128;
      double* Cc = A + (long)(j + 1) * 128 * lda + (long)(j + 1) * 128;
      if (thin_ok) {
        const double* la = k2 ? lsw0 + (size_t)(2 * ((j - 1) & 1) + 1) * MINV_ELEMS : lswj;  // column j-1: its strip's SECOND block
        CKC(launch_syrk_thin(Pp, Cc, lda, mt, 1, kw * 128, P, E.lb(), nullptr, h->sig_epoch, la, k2 ? lswj : nullptr));
      } else {
        CKC(syrk_trapezoid(h, E, A, lda, ntr, j + 1, 1, k0, kw, P));
      }
    }
    if (t_work) {
      if (start.armed()) CKC(edge_wait(h, start, T));
      if (group <= 1) {
        CKC(syrk_trapezoid(h, E, A, lda, ntr, j + 2, ntc - j - 2, j - 1, 1, T));
        if (two) CKC(t_signal((j - 1) % 3));
      } else {
        // A batch is bound by the main stream's updates, not by the chain, and a k = 128 update reads and writes the trailing
        // matrices for 128 columns of k.  Same arithmetic, grouped: the column the chain needs next takes the segments it
        // has not had yet (k-segmented launch: the tile takes each 128-column partial sum as a launch of its own would), the
        // columns behind it take `group` segments at a time.  Invariant: every column >= j + 3 has exactly the segments < seg0.
        TrapLaunch seg;
        seg.kflush = j - seg0 > 1 ? 128 : 0;
        CKC(syrk_trapezoid(h, E, A, lda, ntr, j + 2, 1, seg0, j - seg0, T, seg));
        if (two) CKC(t_signal((j - 1) % 3));
        if (j - seg0 >= group && j + 3 < ntc) {
          seg.kflush = 128;
          CKC(syrk_trapezoid(h, E, A, lda, ntr, j + 3, ntc - j - 3, seg0, j - seg0, T, seg));
          seg0 = j;
        }
      }
    }
    if (two && S.u_early && j > cs && (j - cs) % 4 == 0) {
      // gradient evaluations: U = L^-T over the columns that are final (strips <= j - 1), behind the main stream's update
      const int upto = S.u_leaf_done + h->u_early_cols / 2 < j ? S.u_leaf_done + h->u_early_cols / 2 : j;
      if (!t_work && !start.armed()) CKC(hand_off(h, S, P, T));
      CKC(u_levels(h, E, S, upto, h->u_early_max_s));
    }
  }
#undef CKC
  return e;
}

static int lookahead_min_tiles(const mi_gp_handle* h, int ntc) {
  return whole_columns(h, ntc) ? COLUMN_MODE_MIN_TILES : LOOKAHEAD_MIN_TILES;
}

// THE two-streams rule: does an evaluation of nb problems of ntc tile columns run on two streams (S.two), and would the single
// evaluation of that size (S.la_single)?  Once per evaluation; enqueue_factor and cholesky_enqueue read the answer.
static void plan_streams(const mi_gp_handle* h, int ntc, int nb, Sched& S) {
  // A batched evaluation (blockIdx.z = problem) carries nb times the work per launch, so the look-ahead pays from smaller
  // problems on (nb = 8: N = 2560 +5 %, 3072 +10 %, 4096 +7 %; nb = 2 from 3072 on).  The super-panel widths stay those of
  // the single evaluation of the same size, so that a batch returns the single entry points' bits.
  S.la_single = h->lookahead == 2 || (h->lookahead == 1 && ntc >= lookahead_min_tiles(h, ntc));
  S.two = S.la_single || (h->lookahead == 1 && nb >= 2 && ntc >= (nb >= 8 ? 20 : 24));
}

static hipError_t cholesky_enqueue(mi_gp_handle* h, const Eval& E, Sched& S, double* A, long lda, int ntr, int ntc);
static hipError_t cholesky(mi_gp_handle* h, const Eval& E, Sched& S, double* A, long lda, int ntr, int ntc) {
  const hipError_t e = cholesky_enqueue(h, E, S, A, lda, ntr, ntc);
  h->test_drop_signal = 0;  // (option 28 is for ONE evaluation, whether or not its schedule had the edge the hook drops)
  return e;
}

static hipError_t cholesky_enqueue(mi_gp_handle* h, const Eval& E, Sched& S, double* A, long lda, int ntr, int ntc) {
  const int nb = E.bt.nb;
  hipStream_t T = h->stream, P = S.two ? h->pstream : h->stream;
  hipError_t e;
#define CKE(x) do { e = (x); if (e != hipSuccess) return e; } while (0)
  if (++h->sig_epoch == 0xffffffffu) {  // (4e9 factorisations on one handle: start over)
    CKE(hipStreamSynchronize(h->stream));
    CKE(hipStreamSynchronize(h->pstream));
    CKE(hipMemset(h->sig_dev, 0, sizeof(unsigned) * SIG_SLOTS));
    h->sig_epoch = 1;
  }
  // the panel stream starts after what is queued on the main stream (assembly) -- unless the assembly is in front of the
  // chain on that very stream (asm_on_panel: two streams only)
  if (P != T && !S.asm_on_panel) CKE(hand_off(h, S, T, P));
  const int wcap = (S.la_single && ntc <= NARROW_PANELS_MAX_TILES) ? 4 : 0;
  int w = pick_w(h, ntc, wcap);
  // EXTENDED super-panels (round 5, option 35): in the chain-bound part of a factorisation the panel's own in-panel updates
  // also cover the next super-panel's first tile column (chol_panel's nx = 1), level by level.  The separate update of that
  // column behind the panel ((a1): k = the panel's width, 23-33 us on the chain at N = 4096, and a one-lane launch for the
  // two edges in front of it, 8 us) becomes one k = 128 update behind the last strip, whose first workgroup also tells the
  // main stream that the panel is done.  A rule of the SHAPE alone (every schedule applies it, so the bits do not depend on
  // the schedule): at most ext_rows tile rows below the panel, more than EXT_MIN_REST tile columns behind it (the last
  // columns run on one stream, where it would only add a launch), problems of LOOKAHEAD_MIN_TILES tile columns or more.
  // While the trailing update is the critical path it would be wrong: the panel then waits for the main stream's bulk update
  // in its MIDDLE (the first in-panel update that touches the next column), and the main stream idles for the other half.
  constexpr int EXT_MIN_REST = 8;
  auto ext = [&](int c0, int wp) {
    const int m1 = c0 + wp;
    return (h->ext_rows > 0 && ntc >= LOOKAHEAD_MIN_TILES && ntr - m1 <= h->ext_rows && ntc - m1 > EXT_MIN_REST) ? 1 : 0;
  };
  Edge done_cur;  // the slot super-panel J's last in-panel update raises (extended panels on two streams)
  // edges of an extended panel [c0, c0 + wp) that is about to be queued on the panel stream: its first update of the next
  // column (behind the leaf of column c0 + wp / 2 - 1) needs everything queued on the main stream so far
  auto ext_edges = [&](int c0, int wp) -> hipError_t {
    done_cur = Edge();
    S.done = Sched::Armed();
    if (P == T) return hipSuccess;
    if (h->use_smo >= 2 && S.sig_next + 2 <= SIG_SLOTS) {
      S.wait2.col = c0 + (wp >= 2 ? wp / 2 : 1) - 1;
      S.wait2.edge = edge_reserve(S);
      hipError_t we = edge_write(h, S.wait2.edge, T);
      S.done.col = c0 + wp - 1;
      S.done.edge = done_cur = edge_reserve(S);
      return we;
    }
    return hand_off(h, S, T, P);
  };
  // column mode (chol_columns) for the last rl_cols tile columns -- a rule of the shape alone, like the extended panels
  auto rl = [&](int c0) { return h->rl_cols > 0 && c0 < ntc && (ntc - c0 <= h->rl_cols || (c0 == 0 && whole_columns(h, ntc))); };
  if (rl(0)) {
    CKE(chol_columns(h, E, S, A, lda, ntr, ntc, 0, T, P, false));
    if (P != T) CKE(hand_off(h, S, P, T));
    return hipSuccess;
  }
  int nx_cur = ext(0, w);
  if (nx_cur) CKE(ext_edges(0, w));
  CKE(chol_panel(h, E, S, A, lda, ntr, 0, w, P, nx_cur));
  for (int J = 0; J < ntc;) {
    const int n1 = J + w;  // first tile column right of this super-panel
    // The panel stream's edges at a super-panel boundary: it tells the main stream that super-panel J is done (the main
    // stream may read it from here on) and, when it goes on to the next panel on its own stream, it waits for the main
    // stream's previous update of that panel's first column (the T -> P edge further down).  With option 26 = 2 the two are
    // ONE one-lane launch on the panel stream (write, then poll) instead of two runtime kernels; the main stream's halves
    // stay runtime stream memory operations.
    Edge tp;  // a slot: the panel stream already waits for it; the T -> P edge below only has to write it
    auto t_to_p = [&]() { return tp.slot >= 0 ? edge_write(h, tp, T) : hand_off(h, S, T, P); };
    if (P != T && S.u_early && J > 0 && ntc - J <= h->u_early_cols) {
      // Gradient evaluations: in the chain-bound last steps the main stream would now idle until the panel stream has
      // factored super-panel J.  The leaf blocks and the first block-doubling levels of U = L^-T over the columns that are
      // final (everything left of J) run here instead of behind the factorisation (same launches on the same tiles, only
      // grouped differently over the node batches: same bits).
      const int upto = S.u_leaf_done + h->u_early_cols / 2 < J ? S.u_leaf_done + h->u_early_cols / 2 : J;
      CKE(u_levels(h, E, S, upto, h->u_early_max_s));
    }
    if (P != T) {
      const bool stays_two = n1 < ntc && (rl(n1) || !(ntc - n1 <= h->single_below / nb));
      bool tp_edge = false;
      if (stays_two && !nx_cur) {
        const int wn_ = pick_w(h, ntc - n1, wcap);
        const bool merged_ = n1 + wn_ < ntc && h->merge_min_tiles > 0 && ntc - n1 >= h->merge_min_tiles;
        tp_edge = merged_ || J > 0;
      }
      if (nx_cur && done_cur.armed()) {
        // (an extended panel: its last in-panel update raised the slot -- nothing to launch on the panel stream)
        CKE(edge_wait(h, done_cur, T));
      } else if (h->use_smo >= 2 && tp_edge && S.sig_next + 2 <= SIG_SLOTS) {
        const Edge a = edge_reserve(S);
        tp = edge_reserve(S);
        CKE(launch_signal_write_wait(edge_ptr(h, a), edge_ptr(h, tp), h->sig_epoch, E.s.info_dev, P, E.bt.nb, E.bt.sinfo,
                                     h->poll_limit_log2));
        CKE(edge_wait(h, a, T));
      } else {
        CKE(hand_off(h, S, P, T));
      }
    }
    if (n1 >= ntc) break;
    if (rl(n1)) {
      // the rest column by column: column n1 <- super-panel J on the panel stream ((a1); an extended panel has done it),
      // the columns behind it <- super-panel J on the main stream, polled for by the first leaf
      if (P != T) {
        if (!nx_cur) {
          if (J > 0) CKE(t_to_p());
          CKE(syrk_trapezoid(h, E, A, lda, ntr, n1, 1, J, w, P));
        }
        if (ntc - n1 - 1 > 0) CKE(syrk_trapezoid(h, E, A, lda, ntr, n1 + 1, ntc - n1 - 1, J, w, T));
      } else if (ntc - n1 - nx_cur > 0) {
        CKE(syrk_trapezoid(h, E, A, lda, ntr, n1 + nx_cur, ntc - n1 - nx_cur, J, w, T));
      }
      CKE(chol_columns(h, E, S, A, lda, ntr, ntc, n1, T, P, P != T && ntc - n1 - 1 > 0));
      if (P != T) CKE(hand_off(h, S, P, T));
      break;
    }
    // The END of a large factorisation is a small one: below LOOKAHEAD_MIN_TILES trailing columns the cross-stream hand-offs
    // cost more than the overlap returns (that is why small problems run on one stream), so the rest runs on the main
    // stream alone (round 4, option 21; the super-panel widths stay what they were, so the arithmetic does not change).
    if (P != T && ntc - n1 <= h->single_below / nb) P = T;  // (a batch's launches carry nb times the work)
    const int wn = pick_w(h, ntc - n1, wcap);
    const bool bulk = n1 + wn < ntc;
    // tiles of the trailing update of columns [n1 + wn, ntc) / of the whole trailing trapezoid [n1, ntc)
    const int bc = ntc - n1 - wn, br = ntr - n1 - wn;
    const int btiles = bc * (bc + 1) / 2 + (br - bc) * bc;
    const int low = ntc - n1 <= h->lowocc_thr ? 1 : 0;
    const int nxn = ext(n1, wn);  // the panel queued in this step
    if (P != T && bulk && !nx_cur && h->merge_min_tiles > 0 && ntc - n1 >= h->merge_min_tiles) {
      // BULK-BOUND super-panels (round 4): the panel stream idles for most of such a step, so the next super-panel need not
      // be updated by launches of its own ((a1) on the panel stream + (a2) on the main stream, 64x64 tiles, ~55 TFLOP/s, a
      // last partial round each).  The whole trailing trapezoid [n1, ntc) is ONE enumeration on the 128x128-tile kernel with
      // the next super-panel's wn columns first; a prefix of full rounds that covers them runs two workgroups per CU with
      // nothing beside it, the panel stream starts behind it, and the rest follows as below (one per CU beside the chain,
      // then two per CU).  Same tiles and k order per tile as the split form.
      const int ac = ntc - n1, ar = ntr - n1;
      const int atiles = ac * (ac + 1) / 2 + (ar - ac) * ac;
      const int ft = wn * (wn + 1) / 2 + (ar - wn) * wn;
      int x1 = (ft + 511) / 512 * 512;
      if (x1 > atiles) x1 = atiles;
      TrapLaunch part;  // (the next super-panel's wn columns first in every part's enumeration)
      part.fc = wn;
      part.tile_cnt = x1;
      CKE(syrk_trapezoid(h, E, A, lda, ntr, n1, ac, J, w, T, part));
      CKE(t_to_p());
      part.tile0 = x1;
      part.tile_cnt = atiles;
      if (low && h->split_tiles > 0 && atiles - x1 >= h->split_tiles + h->split_min_rest) {
        part.one_per_cu = 1;
        part.tile_cnt = h->split_tiles;
        CKE(syrk_trapezoid(h, E, A, lda, ntr, n1, ac, J, w, T, part));
        part.one_per_cu = 0;
        part.tile0 = x1 + h->split_tiles;
        part.tile_cnt = atiles;
        CKE(syrk_trapezoid(h, E, A, lda, ntr, n1, ac, J, w, T, part));
      } else if (atiles > x1) {
        part.one_per_cu = low;
        CKE(syrk_trapezoid(h, E, A, lda, ntr, n1, ac, J, w, T, part));
      }
      if (nxn) CKE(ext_edges(n1, wn));
      CKE(chol_panel(h, E, S, A, lda, ntr, n1, wn, P, nxn));
      J = n1;
      w = wn;
      nx_cur = nxn;
      continue;
    }
    if (P != T) {
      // (a1) the next super-panel's FIRST tile column on the panel stream itself: the chain goes on to its leaf without
      //      waiting for the other wn - 1 columns (round 1 updated all wn columns on the main stream first: 40-80 us on
      //      the critical path per super-panel).  That column was last touched by the previous step's bulk update (b)
      //      on the main stream: wait for it first.
      // (a2) the other columns on the main stream meanwhile; the panel stream waits for them after that leaf + strip
      if (!nx_cur) {  // (an extended panel has updated column n1 itself, behind the main stream's earlier updates of it)
        if (J > 0) CKE(t_to_p());
        CKE(syrk_trapezoid(h, E, A, lda, ntr, n1, 1, J, w, P));
      }
      if (wn > 1) {
        // One workgroup per CU for problems of up to 48 tile columns: the chain's next leaf needs a CU to itself, and with two
        // 64x64-tile workgroups on every CU none empties before this grid drains (the first leaf of a super-panel waits 70-160 us
        // at N = 8192).  Beyond that the update itself takes so much longer at half occupancy that N >= 8192 loses 1.5-2 % (the
        // chain waits for THIS launch at those steps, not for the leaf); N <= 6144 gains 0.7-1 %.  Scheduling only.
        TrapLaunch a2;
        a2.one_per_cu = ntc <= 48 ? 1 : 0;
        CKE(syrk_trapezoid(h, E, A, lda, ntr, n1 + 1, wn - 1, J, w, T, a2));
        if (h->test_drop_signal && h->use_smo >= 2 && S.sig_next < SIG_SLOTS) {
          // test hook (option 28): this edge's slot is never written -- the panel stream's poll has to give up
          h->test_drop_signal = 0;
          S.wait.edge = edge_reserve(S);
        } else {
          CKE(edge_signal(h, S, T, h->use_smo != 0, &S.wait.edge));
        }
        S.wait.col = n1;
      }
    } else if (wn - nx_cur > 0) {
      CKE(syrk_trapezoid(h, E, A, lda, ntr, n1 + nx_cur, wn - nx_cur, J, w, T));
    }
    // (b) the rest of the trailing matrix, concurrently with that panel factorisation; once the panel chain is the
    // critical path the bulk update runs one workgroup per CU so that a leaf / strip workgroup fits beside it everywhere.
    // Enqueued BEFORE the chain's ~25 launches: when the host runs only just ahead of the device (under rocprofv3 it does:
    // 150-200 us of idle main stream per super-panel at N = 8192) the bulk update is already queued when (a2) ends.
    // (On a single stream the order cannot matter for the schedule; there the bulk update stays behind the chain, where
    // it measures 1.6 % faster -- 1.771 vs 1.800 ms per launch at N = 16384, same box, interleaved: it then starts after
    // ~0.5 ms of a mostly idle chip instead of straight after the next-panel update.)
    bool ext_done = false;
    TrapLaunch bulk_low;
    bulk_low.one_per_cu = low;
    if (bulk && P != T && nxn && h->use_smo >= 2) {
      // an extended panel follows: its chain polls for the bulk update of column n1 + wn in its middle -- that column first,
      // the signal, then the rest (the same tiles on the same kernels as one launch would give them: same bits)
      CKE(syrk_trapezoid(h, E, A, lda, ntr, n1 + wn, 1, J, w, T, bulk_low));
      CKE(ext_edges(n1, wn));
      ext_done = true;
      if (bc > 1) CKE(syrk_trapezoid(h, E, A, lda, ntr, n1 + wn + 1, bc - 1, J, w, T, bulk_low));
    } else if (bulk && P != T) {
      // Early super-panels are bound by the bulk update, not by the chain (the panel stream idles for most of it): only the
      // first split_tiles tiles run one workgroup per CU -- the mode that leaves every CU room for the chain's leaf /
      // strip / in-panel workgroups (and costs the kernel 5 % even alone) -- and the rest runs two per CU once the chain is through
      // (same tiles, same kernels: bit-identical results).  split_tiles ~ what the update gets done while a chain runs.
      if (low && h->split_tiles > 0 && btiles >= h->split_tiles + h->split_min_rest) {
        TrapLaunch part;
        part.one_per_cu = 1;
        part.tile_cnt = h->split_tiles;
        CKE(syrk_trapezoid(h, E, A, lda, ntr, n1 + wn, bc, J, w, T, part));
        part.one_per_cu = 0;
        part.tile0 = h->split_tiles;
        part.tile_cnt = btiles;
        CKE(syrk_trapezoid(h, E, A, lda, ntr, n1 + wn, bc, J, w, T, part));
      } else {
        CKE(syrk_trapezoid(h, E, A, lda, ntr, n1 + wn, bc, J, w, T, bulk_low));
      }
    }
    // (an extended panel writes column n1 + wn: in every schedule BEHIND this step's bulk update of that column)
    if (bulk && P == T && nxn) CKE(syrk_trapezoid(h, E, A, lda, ntr, n1 + wn, ntc - n1 - wn, J, w, T));
    if (nxn && !ext_done) CKE(ext_edges(n1, wn));
    CKE(chol_panel(h, E, S, A, lda, ntr, n1, wn, P, nxn));
    if (bulk && P == T && !nxn) CKE(syrk_trapezoid(h, E, A, lda, ntr, n1 + wn, ntc - n1 - wn, J, w, T));
    J = n1;
    w = wn;
    nx_cur = nxn;
  }
#undef CKE
  return hipSuccess;
}

// Kernels of one evaluation: assembly, factorisation of the augmented trapezoid [[K],[y^T]] (L ends
// up in K_dev, beta = L^-1 y in row np), reduction.
static int enqueue_factor(mi_gp_handle* h, const Eval& E, Sched& S, int noise_form, bool prof) {
  // Two-stream evaluations (round 6): the evaluation's first two kernels go to the PANEL stream, so that the first leaf follows the
  // assembly in stream order instead of behind a cross-stream edge (~10 us: N = 1024 0.335 -> 0.308 ms, 2048 0.651 -> 0.605; from 32
  // tile columns on, where a panel and not a column comes first, it is 0.1-0.4 %: N = 4096 1.411 -> 1.405, LML + gradient 2.515 -> 2.473).
  // The main stream's first launch waits for the panel stream anyway (a leaf's start signal in column mode, the first panel's
  // end otherwise), and every API call ends with both streams drained.  Same launches: scheduling only.
  plan_streams(h, h->ntc, E.bt.nb, S);
  S.asm_on_panel = S.two && h->start_on_panel;
  const hipStream_t s0 = S.asm_on_panel ? h->pstream : h->stream;
  if (prof) (void)hipEventRecord(h->ev[0], s0);
  // first kernel of the evaluation: y rows, the bad-pivot word, and theta from the pinned host buffer to theta_dev
  HCK(launch_set_yrows(E.K, h->buf.lda, h->np, h->np, h->buf.y_dev, h->n, s0, E.s.info_dev, E.s.theta_host,
                       E.s.theta_dev, h->ntheta, E.lb()), "set_yrows");
  // (Until round 6 evaluations of 96 tile columns and more assembled the first super-panel's columns first and the rest one
  // workgroup per CU beside its factorisation, option 24: with the faster assembly it measured level to 0.5 % behind one launch at
  // N = 12288 .. 20480 and 0.8 % behind at N = 8192, profiles/NOTES_r06.md -- removed.)
  if (h->deriv_npts)  // a gradient binding: the joint covariance of the values and the derivatives in the launch's place
    HCK(deriv_assemble_train(h, E, noise_form, s0), "assemble (gradient binding)");
  else
    HCK(launch_assemble(h->spec, E.s.theta_dev, h->buf.X_dev, h->n, h->buf.X_dev, h->n, E.K, h->buf.lda, h->np,
                        h->np, 1, noise_form, s0, 0, h->diag_dev, E.lb()), "assemble");
  if (prof) (void)hipEventRecord(h->ev[1], s0);
  HCK(cholesky(h, E, S, E.K, h->buf.lda, h->ntc + 1, h->ntc), "cholesky");
  if (prof) (void)hipEventRecord(h->ev[2], h->stream);
  // the scalars go straight to the pinned host buffer (device-visible): no download launch behind the reduction
  h->eval_seq += 1.0;  // (exact in a double for 2^53 evaluations)
  HCK(launch_lml_reduce(E.K, h->buf.lda, E.K + (long)h->np * h->buf.lda, h->n, E.s.out_host, h->stream, E.s.info_dev,
                        E.lb(), E.s.lr_part_dev, E.s.lr_sync_dev, h->eval_seq), "lml_reduce");
  if (prof) (void)hipEventRecord(h->ev[3], h->stream);
  return 0;
}

static int enqueue_gradient(mi_gp_handle* h, const Eval& E, Sched& S, bool prof);

static int enqueue_all(mi_gp_handle* h, const Eval& E, int what, bool prof) {
  Sched S;  // this evaluation's scheduling state
  // (from 64 tile columns on: N = 8192 LML + gradient 11.17 -> 10.98 ms, N = 16384 69.81 -> 69.40; at N = 4096 the main stream
  // has no idle time to fill in those steps: 2.74 -> 2.81)
  S.u_early = what == 2 && !E.batched && h->u_early_max_s > 0 && h->ntc >= 64 && E.Z && E.W;
  if (int r = enqueue_factor(h, E, S, what == 1 ? 1 : 0, prof)) return r;
  if (what == 2) return enqueue_gradient(h, E, S, prof);
  return 0;
}

// Run `what` (0 factor marginal form, 1 factor conditional form, 2 factor + gradient) as plain launches on the handle's
// stream(s).  Round 1 replayed a captured hipGraph per evaluation; measured again in round 2 (tools/time_sizes.py) replay
// is 1-4 % faster than plain launches from N = 4096 on and SLOWER below (N = 128: 0.104 vs 0.087 ms), its keep / drop
// heuristic made the timing depend on the instantiation, and the HIP runtime of this stack crashes in
// hip::Graph::UpdateStreams when executable graphs of two-stream captures come and go
// (profiles/r02_hipgraph_updatestreams_segv.txt; tools/stress_handles.py reproduced it in seconds) -- removed.
int run_evaluation(mi_gp_handle* h, const Eval& E, int what) {
  const bool prof = E.prof >= 1;
  h->gemm_ev_used = 0;
  h->gemm_flops_acc = 0.0;
  // theta travels inside the first kernel (set_yrows_kernel); the scalars and the gradient are written to pinned host
  // memory by the kernels that produce them: no copy launches
  return enqueue_all(h, E, what, prof);
}

// ---------------------------------------------------------------- gradient (K7)
// U = L^-T (upper triangular, row-major in Z_dev) by leaf solves + level-batched block doubling:
//   [[L11, 0], [L21, L22]]^-T = [[U11, -U11 L21^T U22], [0, U22]]
// then Kinv = U U^T (lower tiles, W_dev), alpha = U beta, and the contraction kernel.
// single_form: a batched launch takes the tile form (64x64 / 128x128) that the same product of ONE problem takes -- a rule of the
// shape, not of the batch size (gemm_uses_small_tiles counts tiles x batch)
hipError_t gemm_call(mi_gp_handle* h, const Eval& E, int ak, int bk, In A, In B, Out C, int mt, int nt, int k, int tri, int kmode,
                     double alpha, double beta, int batch, bool single_form) {
  GemmParams p;
  p.A = A.p; p.B = B.p; p.C = C.p; p.lda = A.ld; p.ldb = B.ld; p.ldc = C.ld;
  p.strideA = A.node; p.strideB = B.node; p.strideC = C.node;
  p.mt = mt; p.nt = nt; p.k = k; p.tri = tri; p.kmode = kmode; p.alpha = alpha; p.beta = beta;
  p.small_below = h->small_below; p.band = h->band_rows; p.tail_small = h->tail_small;
  if (E.batched && single_form) p.small_below = gemm_uses_small_tiles(p, batch) ? 0x7fffffff : 0;
  if (E.batched) {  // batched evaluation: the problems are the second batch level (the operands' z: the strides of the matrices A, B, C live in)
    p.batch1 = batch;
    p.strideA2 = A.z; p.strideB2 = B.z; p.strideC2 = C.z;
    batch *= E.bt.nb;
  }
  return launch_gemm_f64(p, ak, bk, batch, h->stream);
}

// Leaf blocks and FULL nodes of the block-doubling levels of U over tile columns [0, final_cols) of L, as far as they are
// not done yet (u_leaf_done / u_node_done): level s (nodes of 2 s tiles, li = log2 s) needs its nodes' halves -- full nodes of
// level s / 2 -- done.  Called with growing final_cols inside the factorisation's tail (cholesky()) and once with everything
// from inverse_transpose(); the node batches are split differently, the per-tile arithmetic is the same.
static hipError_t u_levels(mi_gp_handle* h, const Eval& E, Sched& S, int final_cols, int max_s) {
  const double* L = E.K;
  double* U = E.Z;
  double* T = E.W;
  const long ld = h->buf.lda;
  const int ntc = h->ntc;
  const long zK = E.bt.sK, zZ = E.bt.sZ, zW = E.bt.sW;
  hipError_t e;
  if (final_cols > ntc) final_cols = ntc;
  if (final_cols > S.u_leaf_done) {
    if (S.u_leaf_done == 0) {
      e = launch_set_identity_blocks(U, ld, ntc, h->stream, E.lb());
      if (e != hipSuccess) return e;
    }
    // leaves: X L_kk^T = I  ->  X = L_kk^-T
    const int c0 = S.u_leaf_done;
    e = launch_trsm_strip128_batched(E.s.dinv_dev + (size_t)c0 * MINV_ELEMS, U + (long)c0 * (128 * ld + 128), ld, 128 * ld + 128, 128,
                                     final_cols - c0, h->stream, E.lb(), zZ);
    if (e != hipSuccess) return e;
    S.u_leaf_done = final_cols;
  }
  int li = 0;
  for (int s = 1; s < ntc && s <= max_s; s *= 2, ++li) {
    const int child_cols = li == 0 ? S.u_leaf_done : S.u_node_done[li - 1] * s;  // columns covered by finished halves
    const int avail = child_cols / (2 * s);  // (<= ntc / (2 s): only full nodes)
    const int done = S.u_node_done[li];
    if (avail <= done) continue;
    const long node = (long)2 * s * 128 * (ld + 1);
    const long off = (long)done * node;
    const int batch = avail - done;
    const double* U11 = U + off;
    const double* U22 = U + off + (long)s * 128 * (ld + 1);
    const double* L21 = L + off + (long)s * 128 * ld;
    double* P = T + off + (long)s * 128;
    double* U12 = U + off + (long)s * 128;
    // P = U11 L21^T   (U11 upper triangular: k >= row tile)
    e = gemm_call(h, E, 0, 0, {U11, ld, node, zZ}, {L21, ld, node, zK}, {P, ld, node, zW}, s, s, s * 128, 0, 3, 1.0, 0.0, batch);
    if (e != hipSuccess) return e;
    // U12 = -P U22    (U22 upper triangular: k <= column tile)
    e = gemm_call(h, E, 0, 1, {P, ld, node, zW}, {U22, ld, node, zZ}, {U12, ld, node, zZ}, s, s, s * 128, 0, 4, -1.0, 0.0, batch);
    if (e != hipSuccess) return e;
    S.u_node_done[li] = avail;
  }
  return hipSuccess;
}

static hipError_t inverse_transpose(mi_gp_handle* h, const Eval& E, Sched& S) {
  const double* L = E.K;
  double* U = E.Z;
  double* T = E.W;
  const long ld = h->buf.lda;
  const int ntc = h->ntc;
  const long zK = E.bt.sK, zZ = E.bt.sZ, zW = E.bt.sW;
  // every full node of every level (what the factorisation's tail has not done already), then the trailing partial nodes
  // level by level: a partial node's first half is a full node of the level below, its second half is built by the partial
  // nodes of the levels below
  hipError_t e = u_levels(h, E, S, ntc, 1 << 30);
  if (e != hipSuccess) return e;
  for (int s = 1; s < ntc; s *= 2) {
    const int nfull = ntc / (2 * s);             // nodes whose second half is complete
    const int rem = ntc - nfull * 2 * s;         // tiles left for a trailing partial node
    if (rem <= s) continue;
    const long node = (long)2 * s * 128 * (ld + 1);
    const int s2 = rem - s;
    const long off = (long)nfull * node;
    const double* U11 = U + off;
    const double* U22 = U + off + (long)s * 128 * (ld + 1);
    const double* L21 = L + off + (long)s * 128 * ld;
    double* P = T + off + (long)s * 128;
    double* U12 = U + off + (long)s * 128;
    e = gemm_call(h, E, 0, 0, {U11, ld, node, zZ}, {L21, ld, node, zK}, {P, ld, node, zW}, s, s2, s * 128, 0, 3, 1.0, 0.0, 1);
    if (e != hipSuccess) return e;
    e = gemm_call(h, E, 0, 1, {P, ld, node, zW}, {U22, ld, node, zZ}, {U12, ld, node, zZ}, s, s2, s2 * 128, 0, 4, -1.0, 0.0, 1);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t inverse_transpose(mi_gp_handle* h, const Eval& E) {
  Sched S;
  return inverse_transpose(h, E, S);
}

// everything after the factorisation: U = L^-T, Kinv = U U^T, alpha = U beta, contraction, download
static int enqueue_gradient(mi_gp_handle* h, const Eval& E, Sched& S, bool prof) {
  if (prof) (void)hipEventRecord(h->ev[4], h->stream);
  HCK(inverse_transpose(h, E, S), "inverse_transpose");
  if (prof) (void)hipEventRecord(h->ev[5], h->stream);
  const long ld = h->buf.lda;
  // Kinv = U U^T, lower tiles only, k >= row tile
  const long zZ = E.bt.sZ, zW = E.bt.sW;
  HCK(gemm_call(h, E, 0, 0, {E.Z, ld, 0, zZ}, {E.Z, ld, 0, zZ}, {E.W, ld, 0, zW}, h->ntc, h->ntc, h->np, 1, 3, 1.0, 0.0, 1), "lauum");
  if (prof) (void)hipEventRecord(h->ev[6], h->stream);
  HCK(launch_trmv_upper(E.Z, ld, E.K + (long)h->np * ld, h->n, E.s.alpha_dev, h->stream, E.lb()), "trmv");
  // the final reduction writes the gradient straight into the handle's pinned host buffer (device-visible)
  if (h->deriv_npts)  // a gradient binding: the joint covariance's contraction in the launch's place (the same publication)
    HCK(deriv_grad_contract(h, E), "grad_contract (gradient binding)");
  else
    HCK(launch_grad_contract(h->spec, E.s.theta_dev, h->buf.X_dev, h->n, E.W, ld, E.s.alpha_dev, E.s.part_dev,
                             E.s.grad_host, h->stream, E.lb(), E.s.lr_sync_dev + E.bt.nb, E.s.out_host + 5, h->eval_seq),
        "grad_contract");
  if (prof) (void)hipEventRecord(h->ev[7], h->stream);
  return 0;
}
