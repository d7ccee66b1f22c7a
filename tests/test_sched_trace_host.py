"""Every factorisation schedule, checked for races on its recorded launch trace -- without a device.

tests/sched_trace is a host-only program: the real api_gp.hip and gp_sched.hip linked against recording stand-ins.  It writes
down what an evaluation enqueues; tests/sched_check.py orders the records (two streams, events, stream memory operations,
writes and polls folded into kernels), intersects the launches' footprints, and replays the algebra symbolically.  A missing
cross-stream edge does not change a result on an idle device; here it is a finding.
"""
import collections

import pytest

import sched_check as C
import sched_trace_harness as H

SINGLES = ("lml", "factor", "lml_grad")
BATCHES = ("lml_batch", "factor_batch", "lml_grad_batch")


@pytest.fixture(scope="module")
def prog():
    return H.build_trace_program()


def _sweep_lines():
    """every configuration of the sweeps below (the sanitizer build runs them all as well)"""
    lines = {}
    lines["defaults"] = [H.config_line(c, e) for c in range(1, 141) for e in SINGLES]
    lines["batches"] = [H.config_line(c, e, batch=b) for c in H.SWITCH_COUNTS for b in (2, 3, 8) for e in BATCHES]
    opt = []
    for o in H.OPTION_SETS:
        for c in H.SWITCH_COUNTS:
            opt += [H.config_line(c, "lml", options=o), H.config_line(c, "lml_grad", options=o)]
            if 38 in o or 37 in o:  # (column mode's grouped main-stream updates: a batch's alone)
                opt.append(H.config_line(c, "lml_batch", batch=3, options=o))
    for w in H.PANEL_TILES:
        for c in H.SWITCH_COUNTS:
            opt += [H.config_line(c, "lml", panel_tiles=w), H.config_line(c, "lml_grad", panel_tiles=w)]
    for o in H.BATCH_OPTION_SETS:  # a batch under each 32 / 35 / 37 / 46 tuple with option 38 = 8, 1 and 3
        opt += [H.config_line(c, "lml_batch", batch=3, options=o) for c in H.SWITCH_COUNTS]
    for o in H.PINNED_SETS:  # the scheduling list with the super-panel width pinned (below 20 tile columns nothing is pinned)
        for c in H.SWITCH_COUNTS:
            if H.pinned_width(c) is not None:
                po = {**o, 2: H.pinned_width(c)}
                opt += [H.config_line(c, "lml", options=po), H.config_line(c, "lml_grad", options=po)]
    lines["options"] = opt
    lines["exhaustion"] = [H.config_line(SLOT_EXHAUSTION_COLUMNS, "lml", panel_tiles=1)]
    return lines


# One super-panel per tile column takes two slots per step (the one-lane launch's write and poll): SIG_SLOTS = 1024 run out
# after about 510 steps.  700 tile columns are long enough; the issue's 2048 would only repeat the event fall-back 1300 more times.
SLOT_EXHAUSTION_COLUMNS = 700


def _check_all(prog, lines, tmp_path, replay=True):
    bad = []
    for i, ntc, ret, refused, findings in H.check_traces_parallel(prog, lines, tmp_path, replay):
        assert ret == 0 and refused == [], (lines[i], ret, refused)
        if findings:
            bad.append("%s (%d tile columns): %s" % (lines[i], ntc, findings[:4]))
    assert not bad, "%d of %d schedules:\n%s" % (len(bad), len(lines), "\n".join(bad[:20]))


def test_defaults_every_tile_column_count(prog, tmp_path):
    _check_all(prog, _sweep_lines()["defaults"], tmp_path)


def test_batches_at_the_switching_counts(prog, tmp_path):
    _check_all(prog, _sweep_lines()["batches"], tmp_path)


def test_option_sets_at_the_switching_counts(prog, tmp_path):
    _check_all(prog, _sweep_lines()["options"], tmp_path)


def test_slot_exhaustion_falls_back_to_events_and_stays_race_free(prog, tmp_path):
    _check_all(prog, _sweep_lines()["exhaustion"], tmp_path, replay=False)
    (cfg, recs, end), = C.split_evaluations(H.run_traces(prog, _sweep_lines()["exhaustion"], tmp_path))
    slots = {tuple(r["ptr"]) for r in recs if r["k"] in ("write32", "wait32")}
    for r in recs:
        if r["k"] == "launch":
            slots |= {tuple(r[f]) for f in ("wr", "wt", "wait_ptr", "start_wr") if r.get(f) is not None}
    assert len(slots) == cfg["sig_slots"], len(slots)           # every slot was used ...
    assert any(r["k"] == "ev_wait" for r in recs)               # ... and the edges behind them are events


# ---------------------------------------------------------------------------------------------- the checker must be able to fail
CFG2 = dict(n=219, np=256, ntc=2, lda=256, nb=1, batched=0, what=0, sig_slots=1024, minv_elems=16384)


def _leaf(s, c, **kw):
    r = dict(k="launch", s=s, fn=C.LEAF, Ablk=["K", c * 128 * 256 + c * 128], lda=256, minv=["one.dinv", c * 16384], col0=c * 128,
             info=["one.info", 0], yrow=None, wait_ptr=None, wait_val=1, poll_log2=22, start_wr=None, nb=1, batched=0)
    r.update(kw)
    return r


def _strip(s, c, rows):
    return dict(k="launch", s=s, fn=C.STRIP, minv=["one.dinv", c * 16384], B=["K", (c + 1) * 128 * 256 + c * 128], ldb=256, m=rows * 128,
                sB2=0, lsw=None, lsw_blocks=0, nb=1, batched=0)


def _update(s):  # column 1 <- column 0
    return dict(k="launch", s=s, fn=C.GEMM, A=["K", 128 * 256], B=["K", 128 * 256], C=["K", 128 * 256 + 128], lda=256, ldb=256, ldc=256,
                strideA=0, strideB=0, strideC=0, batch1=0, strideA2=0, strideB2=0, strideC2=0, mt=2, nt=1, kk=128, tri=1, kmode=0,
                alpha=-1.0, beta=1.0, small_below=1024, band=8, hiprio=0, one_per_cu=0, tail_small=1, tile0=0, tile_cnt=0, fc=0, kseg=0,
                kflush=0, dead_last_half=1, ak=0, bk=0, batch=1, part=0)


def _head(s):
    return [dict(k="launch", s=s, fn="set_yrows", K=["K", 0], info=["one.info", 0], theta_dst=["one.theta", 0]),
            dict(k="launch", s=s, fn="assemble", K=["K", 0], theta=["one.theta", 0])]


def _reduce(s):
    return dict(k="launch", s=s, fn="lml_reduce", L=["K", 0], info=["one.info", 0], out=["one.out_host", 0], part=["one.lr_part", 0],
                sync=["one.lr_sync", 0])


def _w(s, slot):
    return dict(k="write32", s=s, ptr=["sig", slot], val=1, flags=0)


def _wt(s, slot):
    return dict(k="wait32", s=s, ptr=["sig", slot], val=1, flags=0, mask=0xffffffff)


def test_hand_written_trace_that_is_sound():
    # stream 1 factors column 0, stream 0 updates column 1 behind it and goes on alone
    t = _head(1) + [_leaf(1, 0), _strip(1, 0, 2), _w(1, 0), _wt(0, 0), _update(0), _leaf(0, 1, yrow=["K", 2 * 128 * 256 + 128]), _reduce(0)]
    assert C.check(CFG2, t).findings == []


def test_hand_written_trace_with_a_race():
    # the same without the edge: the update reads the strip's tiles while the strip may still write them
    t = _head(1) + [_leaf(1, 0), _strip(1, 0, 2), _update(0), _leaf(0, 1, yrow=["K", 2 * 128 * 256 + 128]), _reduce(0)]
    res = C.check(CFG2, t)
    assert "race" in res.kinds()
    texts = [f.text for f in res.findings if f.kind == "race"]
    assert any("update of columns [1, 2) by columns [0, 1)" in t and "strip of column 0" in t and "tile (1, 0) of K" in t for t in texts), texts


def test_a_kernel_side_poll_orders_only_the_end_of_its_kernel():
    # leaf 1 polls for the update of its own tile: the poll holds back the leaf's END, its reads are not ordered -- a race;
    # a runtime wait in front of the leaf is the edge that works
    tail = [_leaf(1, 1, yrow=["K", 2 * 128 * 256 + 128]), _w(1, 2), _wt(0, 2), _reduce(0)]
    polled = _head(1) + [_leaf(1, 0), _strip(1, 0, 2), _w(1, 0), _wt(0, 0), _update(0), _w(0, 1)]
    bad = polled + [dict(tail[0], wait_ptr=["sig", 1])] + tail[1:]
    assert "race" in C.check(CFG2, bad).kinds()
    assert C.check(CFG2, polled + [_wt(1, 1)] + tail).findings == []


def _er(s, ev):
    return dict(k="ev_record", s=s, ev=ev)


def _ew(s, ev):
    return dict(k="ev_wait", s=s, ev=ev)


def test_an_event_wait_queued_ahead_of_its_record_orders_nothing():
    # the sound trace with an event for the slot ...
    t = _head(1) + [_leaf(1, 0), _strip(1, 0, 2), _er(1, 5), _ew(0, 5), _update(0), _leaf(0, 1, yrow=["K", 2 * 128 * 256 + 128]), _reduce(0)]
    assert C.check(CFG2, t).findings == []
    # ... and with the wait moved ahead of the record: hipStreamWaitEvent does not wait for a record that follows (an early
    # poll is legal for slots only), so the edge is gone
    t = _head(1) + [_ew(0, 5), _leaf(1, 0), _strip(1, 0, 2), _er(1, 5), _update(0), _leaf(0, 1, yrow=["K", 2 * 128 * 256 + 128]), _reduce(0)]
    kinds = C.check(CFG2, t).kinds()
    assert "early-wait" in kinds and "race" in kinds, kinds
    # the same early wait on a slot is the protocol of option 26 = 2
    t = _head(1) + [_wt(0, 0), _leaf(1, 0), _strip(1, 0, 2), _w(1, 0), _update(0), _leaf(0, 1, yrow=["K", 2 * 128 * 256 + 128]), _reduce(0)]
    assert C.check(CFG2, t).findings == []


def test_hand_written_trace_with_a_slot_nobody_writes():
    t = _head(1) + [_leaf(1, 0), _strip(1, 0, 2), _wt(0, 0), _update(0), _leaf(0, 1, yrow=["K", 2 * 128 * 256 + 128]), _reduce(0)]
    assert C.check(CFG2, t).kinds() == ["unwritten"]


def test_hand_written_trace_with_a_cycle():
    # each stream's write is queued behind its own wait for the other's
    t = _head(1) + [_leaf(1, 0), _strip(1, 0, 2), _wt(1, 1), _w(1, 0), _wt(0, 0), _w(0, 1), _update(0),
                    _leaf(0, 1, yrow=["K", 2 * 128 * 256 + 128]), _reduce(0)]
    assert C.check(CFG2, t).kinds() == ["cycle"]


def test_hand_written_trace_that_writes_a_slot_twice_or_skips_an_update():
    t = _head(1) + [_leaf(1, 0), _strip(1, 0, 2), _w(1, 0), _w(1, 0), _wt(0, 0), _update(0), _leaf(0, 1, yrow=["K", 2 * 128 * 256 + 128]), _reduce(0)]
    assert C.check(CFG2, t).kinds() == ["rewrite"]
    t = _head(1) + [_leaf(1, 0), _strip(1, 0, 2), _w(1, 0), _wt(0, 0), _leaf(0, 1, yrow=["K", 2 * 128 * 256 + 128]), _reduce(0)]
    assert C.check(CFG2, t).kinds() == ["replay"]


def test_option_28_leaves_a_slot_unwritten_and_the_checker_says_so(prog, tmp_path):
    lines = [H.config_line(c, "lml", options={28: 1}) for c in (40, 70)]
    for cfg, recs, end in C.split_evaluations(H.run_traces(prog, lines, tmp_path)):
        assert cfg["options"]["28"] == 1
        res = C.check(cfg, recs)
        assert res.kinds() == ["unwritten"], res.findings


# ---------------------------------------------------------------------------------------------- deletions
U_LAUNCHERS = ("set_identity_blocks", "trsm_strip128_batched")
EDGE_KINDS = ["start-behind-assembly", "panel-done", "a2", "extended-wait", "extended-done", "column-start", "column-polls",
              "final-hand-off", "u-levels-hand-off"]


def wait_sites(cfg, recs):
    """[(kind of edge, index of the record that waits)]: every runtime wait and every kernel-side poll of a trace"""
    ops = C.parse_ops(recs)
    g = C.Geometry(cfg)
    cs = C.column_mode_start(ops, g)
    launches = [o for o in ops if o.kind == "launch"]
    main = launches[-1].s
    writer = {}
    for o in ops:
        for key in (o.start_write, o.key if o.kind in ("write32", "ev_record") else None):
            if key is not None:
                writer.setdefault(key, o)

    def launch_on(stream, idx, step):
        i = idx + step
        while 0 <= i < len(ops):
            if ops[i].kind == "launch" and ops[i].s == stream:
                return ops[i]
            i += step
        return None

    sites = []
    for o in ops:
        key = o.end_poll if o.kind == "launch" else o.key if o.kind in ("wait32", "ev_wait") else None
        if key is None or key not in writer:
            continue
        w = writer[key]
        wfn = w.rec.get("fn")
        if o.s == main:
            nxt = launch_on(main, o.idx, +1)
            nfn = nxt.rec["fn"] if nxt is not None else None
            if wfn == C.LEAF:
                kind = "column-start"
            elif wfn == C.THIN or (wfn == C.ONE_LANE and w.end_poll is None):
                kind = "extended-done"
            elif wfn == C.ONE_LANE:
                kind = "panel-done"
            elif nfn in U_LAUNCHERS or (nfn == C.GEMM and nxt.rec["C"][0] in ("Z", "W", "bZ", "bW")):
                kind = "u-levels-hand-off"
            elif nfn == "lml_reduce":
                kind = "final-hand-off"
            else:
                kind = "panel-done"
        elif o.kind != "launch":
            kind = "start-behind-assembly" if launch_on(o.s, o.idx, -1) is None else "other-runtime-wait"
        elif o.rec["fn"] == C.ONE_LANE:
            kind = "main-to-panel"  # (the panel stream's wait for the previous bulk update of the next panel's first column)
        else:
            col = o.rec["col0"] // 128
            prev = launch_on(w.s, w.idx, -1)
            a2 = prev is not None and prev.rec["fn"] == C.GEMM and prev.rec["C"][0] == "K" and g.tile(prev.rec["C"], prev.rec["ldc"])[2] == col + 1
            kind = "column-polls" if col >= cs else "a2" if a2 else "extended-wait"
        sites.append((kind, o.idx))
    return sites


def without_wait(recs, i):
    r = recs[i]
    if r["k"] != "launch":
        return recs[:i] + recs[i + 1:]
    return recs[:i] + [dict(r, **{"wait_ptr" if r["fn"] == C.LEAF else "wt": None})] + recs[i + 1:]


def without_update(recs, i):
    """the trace without update i; an edge that the update's kernel raises stays (as the one-lane launch in front of a
    64x64-tile update would raise it)"""
    r = recs[i]
    keep = []
    if r["fn"] == C.THIN and r["wr"] is not None:
        keep = [dict(k="launch", s=r["s"], fn=C.ONE_LANE, wr=r["wr"], wt=None, val=r["val"], info=["one.info", 0], nb=1, sinfo=0, poll_log2=22)]
    return recs[:i] + keep + recs[i + 1:]


def test_deleting_any_update_or_any_kind_of_edge_is_caught(prog, tmp_path):
    """At 26, 40 and 70 tile columns (defaults): every update launch deleted in turn is caught by the replay; every wait deleted
    in turn -- each kind of edge at least once -- is caught as a race.  The evaluation starts on the panel stream by default
    (option 45), so the edge between the assembly and the panel stream's start exists only with 45 = 0: those traces are added."""
    lines = [H.config_line(c, e) for c in (26, 40, 70) for e in ("lml", "lml_grad")]
    lines += [H.config_line(c, "lml", options={45: 0}) for c in (26, 40, 70)]
    raced, unnoticed, other, seen = collections.Counter(), [], [], collections.Counter()
    for line, (cfg, recs, end) in zip(lines, C.split_evaluations(H.run_traces(prog, lines, tmp_path))):
        assert C.check(cfg, recs).findings == []
        for i, r in enumerate(recs):
            if r["k"] == "launch" and (r["fn"] == C.THIN or (r["fn"] == C.GEMM and r["C"][0] == "K")):
                kinds = C.check(cfg, without_update(recs, i)).kinds()
                assert "replay" in kinds, (line, i, r, kinds)
        for kind, i in wait_sites(cfg, recs):
            seen[kind] += 1
            kinds = C.check(cfg, without_wait(recs, i)).kinds()
            if "race" in kinds:
                raced[kind] += 1
            elif not kinds:
                unnoticed.append((line, kind, i))
            else:
                other.append((line, kind, i, kinds))
    print("waits by kind of edge:", dict(seen), "caught as a race:", dict(raced), "unnoticed (implied edges):", unnoticed)
    for kind in EDGE_KINDS:
        assert raced[kind] >= 1, (kind, dict(seen), dict(raced))
    # profiles/NOTES_sched_trace.md lists the implied edges: none at these sizes -- every single deletion is caught as a race
    assert unnoticed == [] and other == [] and raced == seen, (unnoticed, other)


# ---------------------------------------------------------------------------------------------- profiled traces
def _unobserved(recs):
    """a trace without what profiling adds: timing events (recorded, never waited for), the host's synchronisation at the end,
    the one-by-one launches of a split product (part 1 / 2 merged into the one launch of level 0); events renumbered"""
    waited = {r["ev"] for r in recs if r["k"] == "ev_wait"}
    names, out = {}, []
    for r in recs:
        if r["k"] == "sync" or (r["k"] == "ev_record" and r["ev"] not in waited):
            continue
        if r["k"] in ("ev_record", "ev_wait"):
            r = dict(r, ev=names.setdefault(r["ev"], len(names)))
        elif r["k"] == "launch" and r["fn"] == C.GEMM and r["part"] != 0:
            r = dict(r, part=0)
            if out and out[-1] == r:
                continue
        out.append(r)
    return out


def test_a_profiled_trace_holds_the_unprofiled_schedule(prog, tmp_path):
    """tests/test_gpu_sched_trace.py ties the device to traces taken at profiling level 2, the sweeps above check level 0: apart
    from the timing events, the final synchronisation and the split products' parts the two are the same records."""
    sets = [(c, e, o) for c in (5, 26, 40, 70, 130) for e in ("lml", "lml_grad") for o in ({}, {26: 0})]
    sets += [(ntc, e, o) for ntc in ((n + 127) // 128 for n in (600, 3300, 5100, 8900)) for e in ("lml", "lml_grad") for o in ({}, {26: 0})]
    plain = C.split_evaluations(H.run_traces(prog, [H.config_line(c, e, options=o) for c, e, o in sets], tmp_path))
    prof = C.split_evaluations(H.run_traces(prog, [H.config_line(c, e, options=dict(o, prof=2)) for c, e, o in sets], tmp_path))
    for key, (_, a, _), (_, b, _) in zip(sets, plain, prof):
        assert any(r["k"] == "launch" and r["fn"] == C.GEMM and r["part"] for r in b), key
        assert _unobserved(a) == _unobserved(b), key


# ---------------------------------------------------------------------------------------------- the sanitizer build
def test_sanitizer_build_runs_the_whole_sweep_clean(prog, tmp_path):
    """The same program under AddressSanitizer and UndefinedBehaviorSanitizer (a plain host executable: nothing is preloaded)
    runs every configuration of the sweeps and writes the same records."""
    san = H.build_trace_program(sanitize=True)
    lines = [l for group in _sweep_lines().values() for l in group]
    lines += [H.config_line(c, "lml", options={28: 1}) for c in (40, 70)]
    assert H.run_traces(san, lines, tmp_path) == H.run_traces(prog, lines, tmp_path)
