"""Checker for the launch traces of tests/sched_trace: is the schedule of one evaluation race-free, are its edges sound,
and does it compute the factorisation (and the gradient's U = L^-T) it is meant to?

ORDERING MODEL (profiles/NOTES_sched_trace.md has the long form).  Every launch has a start point and an end point.  On one
stream the end of an operation precedes the start of the next.  A runtime write (hipStreamWriteValue32, hipEventRecord) is
ordered behind everything queued before it on its stream; a runtime wait orders everything behind it on its stream after the
matching write.  A wait for an EVENT that is enqueued ahead of the event's record orders nothing (and is a finding).  A
kernel-side write (the leaf's start_wr, the thin kernel's and the one-lane launch's wr) happens at the kernel's START; a
kernel-side poll (the leaf's wait_ptr, the one-lane launch's wt) orders only the kernel's END behind the write.
A launch's knowledge is a vector with one component per stream: known[s] = the position on stream s up to which every launch
has ended before this one starts.  end(Y) precedes start(X) iff Y.pos <= X.known[Y.stream].

FOOTPRINTS are sets of 128x128 tiles of K / Z / W, whole leaf-inverse blocks, whole strip-copy blocks and a few small arrays,
taken from the launcher contracts in andvaranaut_amd/csrc/migp_kernels.h; where in doubt larger.

REPLAY: tile (i, j) of the augmented trapezoid carries the number of k columns (128 wide) applied to it, which must grow in
order: the bits of a tile depend on the order of its partial sums, and every schedule promises the same bits.
"""
import json

import numpy as np

LEAF, STRIP, THIN, GEMM, ONE_LANE = "potrf_leaf128", "trsm_strip128", "syrk_thin", "gemm_f64", "signal_write_wait"


class Finding:
    def __init__(self, kind, text):
        self.kind, self.text = kind, text

    def __repr__(self):
        return "%s: %s" % (self.kind, self.text)


def split_evaluations(text):
    """[(config, records, end)] of a trace program's output."""
    out, cfg, recs = [], None, None
    for line in text.splitlines():
        if not line:
            continue
        r = json.loads(line)
        k = r["k"]
        if k == "config":
            cfg = r
        elif k == "begin":
            recs = []
        elif k == "end":
            out.append((cfg, recs, r))
            cfg, recs = None, None
        elif k == "error":
            raise RuntimeError("sched_trace: %s: %s" % (r["what"], r["why"]))
        elif recs is not None:
            recs.append(r)
    return out


# ------------------------------------------------------------------------------------------------ operations
class Op:
    __slots__ = ("idx", "s", "kind", "rec", "pos", "known", "start_write", "end_poll", "key", "val", "fp")

    def __init__(self, idx, s, kind, rec):
        self.idx, self.s, self.kind, self.rec = idx, s, kind, rec
        self.pos = -1
        self.known = None
        self.start_write = self.end_poll = self.key = self.val = None
        self.fp = ()


def _slot(p):
    return None if p is None else (p[0], p[1])


def parse_ops(records):
    ops = []
    for idx, r in enumerate(records):
        k = r["k"]
        op = Op(idx, r["s"], k, r)
        if k == "launch":
            fn = r["fn"]
            if fn == LEAF:
                op.start_write, op.end_poll, op.val = _slot(r["start_wr"]), _slot(r["wait_ptr"]), r["wait_val"]
            elif fn == THIN:
                op.start_write, op.val = _slot(r["wr"]), r["val"]
            elif fn == ONE_LANE:
                op.start_write, op.end_poll, op.val = _slot(r["wr"]), _slot(r["wt"]), r["val"]
        elif k in ("write32", "wait32"):
            op.key, op.val = _slot(r["ptr"]), r["val"]
        elif k in ("ev_record", "ev_wait"):
            op.key = ("ev", r["ev"])
        ops.append(op)
    return ops


# ------------------------------------------------------------------------------------------------ footprints
class Geometry:
    """Tile coordinates of the pointers of one evaluation (problem 0 of a batch)."""

    def __init__(self, cfg):
        self.cfg = cfg
        self.lda, self.ntc, self.minv = cfg["lda"], cfg["ntc"], cfg["minv_elems"]
        self.ntr = self.ntc + 1
        self.shape = {"K": (self.ntr, self.ntc), "Z": (self.ntc, self.ntc), "W": (self.ntc, self.ntc)}
        self.elems = {"K": (cfg["np"] + 128) * self.lda, "Z": cfg["np"] * self.lda, "W": cfg["np"] * self.lda}

    def mat(self, p):
        name = p[0]
        return name[1:] if name in ("bK", "bZ", "bW") else name

    def tile(self, p, ld=None):
        """(matrix, tile row, tile column) of a pointer into K / Z / W"""
        ld = ld or self.lda
        if ld != self.lda:
            raise ValueError("leading dimension %d, handle's %d" % (ld, self.lda))
        m, off = self.mat(p), p[1]
        if m not in self.shape:
            raise ValueError("pointer into %s where a matrix was expected" % p[0])
        row, col = divmod(off, ld)
        if row % 128 or col % 128:
            raise ValueError("pointer %s is not on a tile boundary" % (p,))
        return m, row // 128, col // 128

    def block(self, p):
        """index of a leaf-inverse / strip-copy block"""
        if not p[0].endswith(".dinv") or p[1] % self.minv:
            raise ValueError("pointer %s is not a leaf-inverse block" % (p,))
        return p[1] // self.minv


_TRI = {}


def tri_mask(mt, nt, upper=False):
    key = (mt, nt, upper)
    if key not in _TRI:
        i, j = np.arange(mt)[:, None], np.arange(nt)[None, :]
        _TRI[key] = (i <= j) if upper else (i >= j)
    return _TRI[key]


def trapezoid_ranges(r):
    """the tile enumeration range [t0, t1) of a (sub-range) launch, its tile count, and the tiles of the first fc columns"""
    mt, nt = r["mt"], r["nt"]
    tiles = nt * (nt + 1) // 2 + (mt - nt) * nt if r["tri"] else mt * nt
    t0 = r["tile0"]
    t1 = min(t0 + r["tile_cnt"], tiles) if r["tile_cnt"] > 0 else tiles
    fc = r["fc"] if (r["tri"] and r["kmode"] == 0 and 0 < r["fc"] < nt) else 0
    ft = fc * (fc + 1) // 2 + (mt - fc) * fc
    return t0, t1, tiles, fc, ft


def footprint(op, g):
    """[(mode, resource)]: mode 'r' / 'w' / 'a' (atomic); a resource is ('T', matrix, r0, r1, c0, c1, mask) or a hashable key"""
    r, fn, fp = op.rec, op.rec["fn"], []

    def rect(mode, m, r0, nr, c0, nc, mask=None):
        rows, cols = g.shape[m]
        if r0 < 0 or c0 < 0 or r0 + nr > rows or c0 + nc > cols:
            raise ValueError("%s tiles [%d, %d) x [%d, %d) leave the %d x %d matrix" % (m, r0, r0 + nr, c0, c0 + nc, rows, cols))
        if nr > 0 and nc > 0:
            fp.append((mode, ("T", m, r0, r0 + nr, c0, c0 + nc, mask)))

    def whole(mode, m):
        rect(mode, m, 0, g.shape[m][0], 0, g.shape[m][1])

    def small(mode, p):
        if p is not None:
            fp.append((mode, ("S", p[0].split(".")[-1])))

    def blocks(mode, p, n):
        b = g.block(p)
        for i in range(n):
            fp.append((mode, ("B", b + i)))

    if fn == "set_yrows":  # migp_kernels.h launch_set_yrows: y rows, the bad-pivot word, theta
        whole("w", g.mat(r["K"]))
        small("w", r["info"]); small("w", r["theta_dst"])
    elif fn == "assemble":  # launch_assemble
        whole("w", g.mat(r["K"]))
        small("r", r["theta"])
    elif fn == LEAF:  # launch_potrf_leaf128: Ablk in place, minv out, yrow in place, info atomicMin
        m, i, j = g.tile(r["Ablk"], r["lda"])
        rect("w", m, i, 1, j, 1)
        if r["yrow"] is not None:
            m2, i2, j2 = g.tile(r["yrow"], r["lda"])
            rect("w", m2, i2, 1, j2, 1)
        blocks("w", r["minv"], 1)
        small("a", r["info"])
    elif fn == STRIP:  # launch_trsm_strip128: X = B M^T in place on m x 128, lsw copies of the first lsw_blocks 16-row groups
        m, i, j = g.tile(r["B"], r["ldb"])
        rect("w", m, i, r["m"] // 128, j, 1)
        blocks("r", r["minv"], 1)
        if r["lsw"] is not None:
            blocks("w", r["lsw"], (r["lsw_blocks"] + 7) // 8)
    elif fn == THIN:  # launch_syrk_thin: C[ti, tj] -= P[ti] P[tj]^T, tj <= ti; B operand from lsw (/ lsw2)
        kw = r["kk"] // 128
        m, i, j = g.tile(r["P"], r["ld"])
        rect("r", m, i, r["mt"], j, kw)
        m, i, j = g.tile(r["C"], r["ld"])
        rect("w", m, i, r["mt"], j, r["nt"], tri_mask(r["mt"], r["nt"]))
        blocks("r", r["lsw"], r["nt"] if kw == 1 else 1)
        if r["lsw2"] is not None:
            blocks("r", r["lsw2"], 1)
    elif fn == ONE_LANE:
        small("a", r["info"])
    elif fn == GEMM:  # GemmParams / launch_gemm_f64
        mt, nt, kt, kmode, tri = r["mt"], r["nt"], r["kk"] // 128, r["kmode"], r["tri"]
        if r["kk"] % 128:
            raise ValueError("gemm k = %d is not whole tiles" % r["kk"])
        nodes = r["batch1"] if r["batch1"] > 0 else r["batch"]
        t0, t1, tiles, fc, ft = trapezoid_ranges(r)
        for z in range(nodes):
            offs = [z * r["strideA"], z * r["strideB"], z * r["strideC"]]
            ptrs = [[r[x][0], r[x][1] + o] for x, o in zip("ABC", offs)]
            if any(p[1] >= g.elems[g.mat(p)] for p in ptrs):
                continue  # (the other problems of a batch run in lockstep: blockIdx.z)
            ma, ia, ja = g.tile(ptrs[0], r["lda"])
            mb, ib, jb = g.tile(ptrs[1], r["ldb"])
            mc, ic, jc = g.tile(ptrs[2], r["ldc"])
            # A: [x][k] (ak = 0) or [k][x]
            ka = min(kt, nt) if kmode == 4 else kt
            amask = tri_mask(mt, ka, upper=True) if kmode == 3 else None
            if r["ak"] == 0:
                rect("r", ma, ia, mt, ja, ka, amask)
            else:
                rect("r", ma, ia, ka, ja, mt, None if amask is None else amask.T)
            # B tile (tj, kk): kmode 4 takes k < (tj + 1) * 128; the tri form of kmode 3 takes k >= ti * 128 >= tj * 128
            bmask = tri_mask(nt, kt) if kmode == 4 else tri_mask(nt, kt, upper=True) if (kmode == 3 and tri) else None
            if r["bk"] == 0:
                rect("r", mb, ib, nt, jb, kt, bmask)
            else:
                rect("r", mb, ib, kt, jb, nt, None if bmask is None else bmask.T)
            cm = "w"  # (beta != 0 reads C as well: a write conflicts with everything a read does)
            if not tri:
                rect(cm, mc, ic, mt, jc, nt)
            elif fc and t1 <= ft:
                rect(cm, mc, ic, mt, jc, fc, tri_mask(mt, fc))  # a prefix inside the first fc columns' tiles
            elif fc and t0 >= ft:
                mask = tri_mask(mt, nt).copy()
                mask[:, :fc] = False
                rect(cm, mc, ic, mt, jc, nt, mask)
            else:
                rect(cm, mc, ic, mt, jc, nt, tri_mask(mt, nt))
    elif fn == "trsm_strip128_batched":  # pair b: minv + b * MINV_ELEMS, B + b * strideB
        if r["strideB"] != 128 * r["ldb"] + 128 or r["m"] != 128:
            raise ValueError("batched strip is not a run of diagonal blocks")
        m, i, j = g.tile(r["B"], r["ldb"])
        for b in range(r["batch"]):
            rect("w", m, i + b, 1, j + b, 1)
        blocks("r", r["minv"], r["batch"])
    elif fn == "set_identity_blocks":
        whole("w", g.mat(r["U"]))
    elif fn == "lml_reduce":
        whole("r", g.mat(r["L"]))
        small("r", r["info"]); small("w", r["out"]); small("w", r["part"]); small("w", r["sync"])
    elif fn == "trmv_upper":
        whole("r", g.mat(r["U"])); whole("r", g.mat(r["beta"]))
        small("w", r["alpha"])
    elif fn == "grad_contract":
        whole("r", g.mat(r["W"]))
        small("r", r["alpha"]); small("r", r["theta"]); small("w", r["part"]); small("w", r["grad"])
        fp.append(("w", ("S", "flag")))
    else:
        raise ValueError("no footprint for launcher %s" % fn)
    return fp


# ------------------------------------------------------------------------------------------------ description of a launch
def column_mode_start(ops, g):
    """first tile column factored in column mode (the column whose successor takes a k = 256 update of one column), or ntc"""
    cs = g.ntc
    for op in ops:
        if op.kind != "launch":
            continue
        r = op.rec
        if (r["fn"] == THIN and r["kk"] == 256) or (r["fn"] == GEMM and r.get("tri") and r["kk"] == 256 and r["nt"] == 1 and r["kmode"] == 0):
            try:
                _, i, j = g.tile(r["C"], r.get("ld") or r.get("ldc"))
            except ValueError:
                continue
            if g.mat(r["C"]) == "K":
                cs = min(cs, j - 2)
    return cs


def describe(op, g, cs, main):
    """launcher, geometry, stream, and the rule of gp_sched.hip that queues such a launch"""
    r = op.rec
    st = "main" if op.s == main else "panel"
    if op.kind != "launch":
        return "#%d %s on the %s stream" % (op.idx, op.kind, st)
    fn = r["fn"]
    try:
        if fn == LEAF:
            c = r["col0"] // 128
            return "#%d leaf of column %d on the %s stream (%s)" % (op.idx, c, st, "chol_columns" if c >= cs else "chol_panel")
        if fn == STRIP:
            c = g.tile(r["B"], r["ldb"])[2]
            return "#%d strip of column %d on the %s stream (%s)" % (op.idx, c, st, "chol_columns" if c >= cs else "chol_panel")
        if fn in (THIN, GEMM) and g.mat(r["C"]) == "K":
            _, i, j = g.tile(r["C"], r.get("ld") or r.get("ldc"))
            k0 = g.tile(r["P"] if fn == THIN else r["A"], r.get("ld") or r.get("lda"))[2]
            kw = r["kk"] // 128
            if k0 >= cs:
                rule = "chol_columns: the next column's update" if j == k0 + kw else "chol_columns: main-stream update"
            elif j > k0 + kw or r["nt"] > 2 * kw:
                rule = "cholesky: (a2) / bulk / merged update"
            else:
                rule = "chol_panel: in-panel update, or cholesky: (a1)"
            sub = "" if fn == THIN or (r["tile0"] == 0 and r["tile_cnt"] == 0) else " tiles [%d, +%d) fc %d" % (r["tile0"], r["tile_cnt"], r["fc"])
            return "#%d update of columns [%d, %d) by columns [%d, %d)%s on the %s stream (%s)" % (op.idx, j, j + r["nt"], k0, k0 + kw, sub, st, rule)
    except (ValueError, KeyError, TypeError):
        pass
    return "#%d %s on the %s stream" % (op.idx, fn, st)


# ------------------------------------------------------------------------------------------------ the check
class Result:
    def __init__(self):
        self.findings = []
        self.order = []        # launches in a linearisation of their start points
        self.stats = {}

    def add(self, kind, text):
        self.findings.append(Finding(kind, text))

    def kinds(self):
        return sorted({f.kind for f in self.findings})


def check(cfg, records, replay=True, final=True):
    res = Result()
    g = Geometry(cfg)
    ops = parse_ops(records)
    launches = [o for o in ops if o.kind == "launch"]
    if not launches:
        res.add("trace", "no launch in the trace")
        return res
    if any(o.rec["fn"] == GEMM and o.rec["part"] != 0 for o in launches):
        # (profiling level 2 launches a split product's two kernels one by one: such a trace is for gemm_figures() only)
        res.add("trace", "recorded at profiling level 2: not a schedule the library runs unobserved")
        return res
    main = launches[-1].s
    cs = column_mode_start(ops, g)
    streams = sorted({o.s for o in ops if o.s >= 0})
    sidx = {s: i for i, s in enumerate(streams)}
    ns = len(streams)

    # ---- edge discipline that needs no ordering
    writers, waiters = {}, {}
    for o in ops:
        for key, tab in ((o.start_write, writers), (o.key if o.kind in ("write32", "ev_record") else None, writers),
                         (o.end_poll, waiters), (o.key if o.kind in ("wait32", "ev_wait") else None, waiters)):
            if key is not None:
                tab.setdefault(key, []).append(o)
    for key, ws in writers.items():
        if len(ws) > 1:
            res.add("rewrite", "%s is written or recorded %d times in one evaluation (%s)" % (key, len(ws), ", ".join(describe(w, g, cs, main) for w in ws)))
    slots = {k for k in list(writers) + list(waiters) if k[0] == "sig"}
    if len(slots) > cfg["sig_slots"] or any(k[1] >= cfg["sig_slots"] for k in slots):
        res.add("slots", "%d slots used, highest %d, of %d" % (len(slots), max(k[1] for k in slots), cfg["sig_slots"]))
    for key, ws in waiters.items():
        if key not in writers:
            res.add("unwritten", "%s waits for %s, which nothing writes" % (describe(ws[0], g, cs, main), key))
        elif key[0] == "sig":
            for w in ws:
                if w.val != writers[key][0].val:
                    res.add("value", "%s waits for %s >= %s, written %s" % (describe(w, g, cs, main), key, w.val, writers[key][0].val))
    # An event is not a slot: hipStreamWaitEvent on an event that has not been recorded yet (in enqueue order) does not wait for the
    # record that follows -- it returns at once, or waits for the previous evaluation's record of the pooled event.  Such a wait is
    # a finding and orders nothing.  (A poll queued ahead of its write is legal for slots only: the epoch makes old values stale.)
    early_waits = set()
    for key, ws in waiters.items():
        if key[0] == "ev" and key in writers:
            for w in ws:
                if w.idx < writers[key][0].idx:
                    early_waits.add(w.idx)
                    res.add("early-wait", "%s waits for event %d, which is recorded only later (%s): the wait orders nothing" % (
                        describe(w, g, cs, main), key[1], describe(writers[key][0], g, cs, main)))
    res.stats = {"launches": len(launches), "slots": len(slots), "events": len({k for k in waiters if k[0] == "ev"}),
                 "edges": len(waiters), "records": len(ops)}
    if any(f.kind == "unwritten" for f in res.findings):
        return res

    # ---- simulate the points: per stream a list of items ('start' / 'end' of a launch, a runtime write or wait)
    items = [[] for _ in range(ns)]
    npos = [0] * ns
    for o in ops:
        if o.kind == "sync":
            # the host blocks: everything enqueued later, on either stream, comes behind everything queued on o.s so far
            key = ("sync", o.idx)
            items[sidx[o.s]].append(("write", o, key))
            for t in range(ns):
                items[t].append(("wait", o, key))
            continue
        if o.s < 0:
            continue
        t = sidx[o.s]
        if o.kind == "launch":
            o.pos = npos[t]
            npos[t] += 1
            items[t].append(("start", o, o.start_write))
            items[t].append(("end", o, o.end_poll))
        elif o.kind in ("write32", "ev_record"):
            items[t].append(("write", o, o.key))
        elif o.kind in ("wait32", "ev_wait") and o.idx not in early_waits:
            items[t].append(("wait", o, o.key))
    by_pos = [[o for o in launches if sidx[o.s] == t] for t in range(ns)]
    know = [[-1] * ns for _ in range(ns)]
    written = {}
    cur = [0] * ns
    while True:
        # of the streams whose next item can run, the one that was enqueued first: a sound schedule is replayed in enqueue
        # order wherever a poll queued ahead of its write allows it, and a report names launches in that order
        t = -1
        for u in range(ns):
            if cur[u] == len(items[u]):
                continue
            what, o, key = items[u][cur[u]]
            if (what == "wait" or (what == "end" and key is not None)) and key not in written:
                continue
            if t < 0 or o.idx < items[t][cur[t]][1].idx:
                t = u
        if t < 0:
            break
        what, o, key = items[t][cur[t]]
        if what == "start":
            o.known = list(know[t])
            if key is not None:
                written.setdefault(key, list(o.known))
            res.order.append(o)
        elif what == "end":
            if key is not None:
                know[t] = [max(a, b) for a, b in zip(know[t], written[key])]
            know[t][t] = o.pos
        elif what == "write":
            written.setdefault(key, list(know[t]))
        else:
            know[t] = [max(a, b) for a, b in zip(know[t], written[key])]
        cur[t] += 1
    stuck = [t for t in range(ns) if cur[t] < len(items[t])]
    if stuck:
        res.add("cycle", "the streams wait for each other: " + "; ".join(
            "%s waits for %s, queued behind it" % (describe(items[t][cur[t]][1], g, cs, main), items[t][cur[t]][2]) for t in stuck))
        return res

    # ---- races, in the order of the start points (end(Y) <= start(X) implies that Y starts first, so one direction is enough)
    wmax = {m: np.full((ns,) + g.shape[m], -1, dtype=np.int32) for m in g.shape}
    rmax = {m: np.full((ns,) + g.shape[m], -1, dtype=np.int32) for m in g.shape}
    small = {}  # key -> {'w': [pos per stream], 'r': ..., 'a': ...}
    conflicts = {"r": ("w", "a"), "a": ("w", "r"), "w": ("w", "r", "a")}
    seen_pairs = set()

    def race(x, t, pos, what):
        y = by_pos[t][pos]
        if (y.idx, x.idx) in seen_pairs:
            return
        seen_pairs.add((y.idx, x.idx))
        res.add("race", "%s is not ordered behind %s; both touch %s" % (describe(x, g, cs, main), describe(y, g, cs, main), what))

    for x in res.order:
        try:
            x.fp = footprint(x, g)
        except ValueError as e:
            res.add("trace", "%s: %s" % (describe(x, g, cs, main), e))
            continue
        tx = sidx[x.s]
        for mode, rsc in x.fp:
            if rsc[0] == "T":
                _, m, r0, r1, c0, c1, mask = rsc
                for t in range(ns):
                    if t == tx:
                        continue
                    for tab in ((wmax[m],) if mode == "r" else (wmax[m], rmax[m])):
                        v = tab[t, r0:r1, c0:c1]
                        bad = v > x.known[t]
                        if mask is not None:
                            bad = bad & mask
                        if bad.any():
                            i, j = np.argwhere(bad)[0]
                            race(x, t, int(v[i, j]), "tile (%d, %d) of %s" % (r0 + i, c0 + j, m))
                tab = (rmax if mode == "r" else wmax)[m]
                v = tab[tx, r0:r1, c0:c1]
                if mask is None:
                    v[...] = x.pos
                else:
                    v[mask] = x.pos
            else:
                st = small.setdefault(rsc, {k: [-1] * ns for k in "rwa"})
                for t in range(ns):
                    if t == tx:
                        continue
                    for other in conflicts[mode]:
                        if st[other][t] > x.known[t]:
                            race(x, t, st[other][t], "block %d of the leaf inverses / strip copies" % rsc[1] if rsc[0] == "B" else rsc[1])
                st[mode][tx] = x.pos

    # ---- the evaluation's last kernel (main stream: it publishes the sequence word) comes behind every other launch
    if final:
        last = launches[-1]
        for t in range(ns):
            n_before = npos[t] - (1 if t == sidx[last.s] else 0)
            if last.known[t] < n_before - 1:
                res.add("final", "%s is not ordered behind %s" % (describe(last, g, cs, main), describe(by_pos[t][n_before - 1], g, cs, main)))
    if replay:
        replay_algebra(cfg, g, res, cs, main)
    return res


# ------------------------------------------------------------------------------------------------ symbolic replay
def replay_algebra(cfg, g, res, cs, main):
    ntc, ntr = g.ntc, g.ntr
    cnt = np.zeros((ntr, ntc), dtype=np.int32)      # k columns applied to tile (i, j), in order
    solved = np.zeros((ntr, ntc), dtype=bool)       # the tile is final (leaf or strip done)
    lower = tri_mask(ntr, ntc)
    have = {"yrows": False, "assembled": False, "ident": False, "kinv": False, "alpha": False, "contract": False, "reduce": False}
    dinv = {}      # leaf-inverse block -> column
    copies = {}    # strip-copy block -> (column, tile row)
    ub = np.zeros((ntc, ntc), dtype=np.int32)       # times tile (i, j) of U was built
    wp = np.full((ntc, ntc), -1, dtype=np.int64)    # which node's P = U11 L21^T sits in tile (i, j) of W
    pending = {}   # a product launched in sub-ranges: key -> [tiles covered, fc columns applied]

    def bad(o, text):
        res.add("replay", "%s: %s" % (describe(o, g, cs, main), text))

    def apply_update(o, r0, mt, ncols, k0, kw, cols_from=0):
        # C tiles (r0 + ti, r0 + tj), cols_from <= tj < ncols, ti >= tj, take k columns [k0, k0 + kw)
        mask = tri_mask(mt, ncols).copy()
        mask[:, :cols_from] = False
        c = cnt[r0:r0 + mt, r0:r0 + ncols]
        if (solved[r0:r0 + mt, r0:r0 + ncols] & mask).any():
            bad(o, "updates a tile that is final already")
        if (c[mask] != k0).any():
            i, j = np.argwhere(mask & (c != k0))[0]
            bad(o, "tile (%d, %d) has had %d k columns, the update applies [%d, %d)" % (r0 + i, r0 + j, c[i, j], k0, k0 + kw))
        c[mask] = k0 + kw

    def sources_final(o, r0, mt, k0, kw):
        if not solved[r0:r0 + mt, k0:k0 + kw].all():
            i, j = np.argwhere(~solved[r0:r0 + mt, k0:k0 + kw])[0]
            bad(o, "reads tile (%d, %d), which is not final" % (r0 + i, k0 + j))

    for o in res.order:
        r = o.rec
        fn = r["fn"]
        try:
            if fn == "set_yrows":
                have["yrows"] = True
            elif fn == "assemble":
                have["assembled"] = True
            elif fn == LEAF:
                _, i, j = g.tile(r["Ablk"], r["lda"])
                c = r["col0"] // 128
                if (i, j) != (c, c):
                    bad(o, "col0 = %d, block at tile (%d, %d)" % (r["col0"], i, j))
                if not (have["yrows"] and have["assembled"]):
                    bad(o, "runs before the assembly")
                if cnt[c, c] != c or solved[c, c]:
                    bad(o, "tile (%d, %d) has had %d k columns%s" % (c, c, cnt[c, c], ", and is final" if solved[c, c] else ""))
                solved[c, c] = True
                if g.block(r["minv"]) != c:
                    bad(o, "writes leaf inverse %d" % g.block(r["minv"]))
                dinv[g.block(r["minv"])] = c
                if (r["yrow"] is not None) != (c == ntc - 1):
                    bad(o, "yrow given" if r["yrow"] is not None else "the last column's leaf has no yrow")
                if r["yrow"] is not None:
                    _, i2, j2 = g.tile(r["yrow"], r["lda"])
                    if (i2, j2) != (c + 1, c) or cnt[i2, j2] != c or solved[i2, j2]:
                        bad(o, "y row tile (%d, %d) with %d k columns" % (i2, j2, cnt[i2, j2]))
                    solved[i2, j2] = True
            elif fn == STRIP:
                _, i, j = g.tile(r["B"], r["ldb"])
                rows = r["m"] // 128
                if i != j + 1 or i + rows != ntr or r["m"] % 128:
                    bad(o, "rows [%d, %d) of column %d" % (i, i + rows, j))
                if dinv.get(g.block(r["minv"])) != j or not solved[j, j]:
                    bad(o, "column %d's leaf inverse is not there" % j)
                if (cnt[i:i + rows, j] != j).any() or solved[i:i + rows, j].any():
                    bad(o, "tiles below (%d, %d) have had %s k columns" % (j, j, sorted(set(cnt[i:i + rows, j].tolist()))))
                solved[i:i + rows, j] = True
                if r["lsw"] is not None:
                    b = g.block(r["lsw"])
                    if b < ntc or b + (r["lsw_blocks"] + 7) // 8 > ntc + 4:
                        bad(o, "strip copy in block %d" % b)
                    for q in range((r["lsw_blocks"] + 7) // 8):
                        copies[b + q] = (j, i + q)
            elif fn == THIN or (fn == GEMM and g.mat(r["C"]) == "K"):
                thin = fn == THIN
                _, pi, pj = g.tile(r["P"] if thin else r["A"], r["ld"] if thin else r["lda"])
                _, ci, cj = g.tile(r["C"], r["ld"] if thin else r["ldc"])
                mt, nt, kw = r["mt"], r["nt"], r["kk"] // 128
                if not thin and not (r["tri"] == 1 and r["kmode"] == 0 and r["A"] == r["B"] and r["alpha"] == -1.0 and r["beta"] == 1.0
                                     and r["ak"] == 0 and r["bk"] == 0 and r["kflush"] in (0, 128) and r["kk"] % 128 == 0):
                    bad(o, "not a trapezoid update C -= P P^T")
                if ci != cj or pi != ci or ci + mt != ntr or pj + kw > ci:
                    bad(o, "geometry: P at (%d, %d), C at (%d, %d), %d x %d tiles, k %d" % (pi, pj, ci, cj, mt, nt, kw))
                    continue
                sources_final(o, ci, mt, pj, kw)
                if thin:
                    want = [(pj, ci + q) for q in range(nt)] if kw == 1 else [(pj, ci)]
                    b = g.block(r["lsw"])
                    got = [copies.get(b + q) for q in range(len(want))]
                    if kw == 2:
                        want.append((pj + 1, ci))
                        got.append(copies.get(g.block(r["lsw2"])) if r["lsw2"] is not None else None)
                    if got != want:
                        bad(o, "strip copies hold %s, the update's B operand is %s (column, tile row)" % (got, want))
                    apply_update(o, ci, mt, nt, pj, kw)
                    continue
                t0, t1, tiles, fc, ft = trapezoid_ranges(r)
                if t0 == 0 and t1 == tiles:
                    apply_update(o, ci, mt, nt, pj, kw)
                    continue
                key = (ci, mt, nt, pj, kw, r["fc"])
                st = pending.setdefault(key, [0, False])
                if t0 != st[0]:
                    bad(o, "sub-range starts at tile %d, the product is covered up to %d" % (t0, st[0]))
                st[0] = t1
                if fc and not st[1] and st[0] >= ft:
                    apply_update(o, ci, mt, fc, pj, kw)
                    st[1] = True
                if st[0] == tiles:
                    apply_update(o, ci, mt, nt, pj, kw, cols_from=fc if st[1] else 0)
                    del pending[key]
            elif fn == "lml_reduce":
                have["reduce"] = True
                if not solved[lower].all():
                    i, j = np.argwhere(lower & ~solved)[0]
                    bad(o, "tile (%d, %d) is not final" % (i, j))
            elif fn == "set_identity_blocks":
                have["ident"] = True
            elif fn == "trsm_strip128_batched":
                _, i, j = g.tile(r["B"], r["ldb"])
                b0 = g.block(r["minv"])
                for q in range(r["batch"]):
                    c = i + q
                    if not have["ident"] or dinv.get(b0 + q) != c or i != j or b0 != i:
                        bad(o, "leaf block %d of U without its identity or leaf inverse" % c)
                    ub[c, c] += 1
            elif fn == GEMM:
                mt, nt, kt, kmode = r["mt"], r["nt"], r["kk"] // 128, r["kmode"]
                nodes = r["batch1"] if r["batch1"] > 0 else r["batch"]
                ma, mb, mc = g.mat(r["A"]), g.mat(r["B"]), g.mat(r["C"])
                if (ma, mb, mc, kmode, r["tri"]) == ("Z", "Z", "W", 3, 1):  # Kinv = U U^T
                    up = tri_mask(ntc, ntc, upper=True)
                    if (ub[up] != 1).any() or mt != ntc or nt != ntc or kt != ntc:
                        bad(o, "K^-1 = U U^T before all of U is built")
                    have["kinv"] = True
                    continue
                for z in range(nodes):
                    pa, pb, pc = [[r[x][0], r[x][1] + z * r["stride" + x]] for x in "ABC"]
                    _, ia, ja = g.tile(pa, r["lda"])
                    _, ib, jb = g.tile(pb, r["ldb"])
                    _, ic, jc = g.tile(pc, r["ldc"])
                    s, s2 = mt, nt
                    if (ma, mb, mc, kmode) == ("Z", "K", "W", 3):  # P = U11 L21^T
                        if not (ia == ja == ic == jb and ib == ia + s and jc == ia + s and kt == s and r["ak"] == 0 and r["bk"] == 0 and r["beta"] == 0.0):
                            bad(o, "node geometry")
                            continue
                        if (ub[ia:ia + s, ia:ia + s][tri_mask(s, s, upper=True)] != 1).any():
                            bad(o, "first half [%d, %d) of the node is not built" % (ia, ia + s))
                        if not solved[ib:ib + s2, jb:jb + s].all():
                            bad(o, "L21 tiles of the node at %d are not final" % ia)
                        wp[ic:ic + s, jc:jc + s2] = o.idx
                    elif (ma, mb, mc, kmode) == ("W", "Z", "Z", 4):  # U12 = -P U22
                        if not (ia == ic and ja == jc and ib == jb == ja and kt == s2 and r["ak"] == 0 and r["bk"] == 1 and r["beta"] == 0.0 and r["alpha"] == -1.0):
                            bad(o, "node geometry")
                            continue
                        p = wp[ia:ia + s, ja:ja + s2]
                        if (p < 0).any() or (p != p[0, 0]).any():
                            bad(o, "P of the node at (%d, %d) is not there" % (ia, ja))
                        if (ub[ib:ib + s2, ib:ib + s2][tri_mask(s2, s2, upper=True)] != 1).any():
                            bad(o, "second half [%d, %d) of the node is not built" % (ib, ib + s2))
                        ub[ic:ic + s, jc:jc + s2] += 1
                        wp[ia:ia + s, ja:ja + s2] = -1
                    else:
                        bad(o, "a product the replay does not know")
            elif fn == "trmv_upper":
                if (ub[tri_mask(ntc, ntc, upper=True)] != 1).any() or not have["reduce"]:
                    bad(o, "alpha = U beta before U and beta are there")
                have["alpha"] = True
            elif fn == "grad_contract":
                if not (have["kinv"] and have["alpha"]):
                    bad(o, "the contraction runs before K^-1 and alpha")
                have["contract"] = True
        except (ValueError, TypeError) as e:
            bad(o, str(e))
    last = res.order[-1]
    if pending:
        bad(last, "products left incomplete: %s" % sorted(pending))
    if not solved[lower].all():
        i, j = np.argwhere(lower & ~solved)[0]
        bad(last, "at the end tile (%d, %d) is not final (%d k columns)" % (i, j, cnt[i, j]))
    if not have["reduce"]:
        bad(last, "no lml_reduce")
    if cfg["what"] == 2:
        if (ub[tri_mask(ntc, ntc, upper=True)] != 1).any():
            i, j = np.argwhere(tri_mask(ntc, ntc, upper=True) & (ub != 1))[0]
            bad(last, "tile (%d, %d) of U was built %d times" % (i, j, ub[i, j]))
        if not have["contract"]:
            bad(last, "no gradient contraction")


# ------------------------------------------------------------------------------------------------ figures of a profiled trace
def gemm_figures(records):
    """(launches, algorithmic flops) of the factorisation's GEMM launches as mi_gp_timers counts them at profiling level 2:
    one per launch_gemm_f64 with part 1 / 2 (the 128x128-tile part / the 64x64-tile tail of a split product)."""
    launches, flops = 0, 0.0
    for r in records:
        if r["k"] != "launch" or r["fn"] != GEMM or r["part"] == 0:
            continue
        t0, t1, tiles, _, _ = trapezoid_ranges(r)
        small = r["kflush"] > 0 or (tiles * r["batch"] < r["small_below"] and r["kmode"] != 2)
        rem = tiles % 512
        tail = rem if (r["tail_small"] and r["kmode"] == 0 and r["batch"] == 1 and not small and tiles > 512 and 0 < rem <= 384) else 0
        big_end = min(t1, tiles - tail)
        if r["part"] == 1:
            mine = (tiles if t0 == 0 else 0) if small else big_end - t0
        else:
            mine = tail if (tail > 0 and t1 == tiles) else 0
        c, rows_real = r["nt"] * 128.0, (r["mt"] - 1) * 128.0
        whole = float(r["kk"]) * (c * (c + 1.0) + 2.0 * (rows_real - c) * c + 2.0 * c)
        launches += 1
        flops += whole * float(mine) / float(tiles)
    return launches, flops
