"""The handle's mode options 48-57 on the host, call for call against the record of the commit before the ModeOption table.

tests/sched_trace/modes_main.hip runs SCRIPT below through the real mi_gp_set_option / mi_gp_get_option / mi_gp_factor /
mi_gp_lml_grad / mi_gp_predict_grad / mi_gp_predict_cov / mi_gp_reserve, linked (a) without the mode files -- every weak mode
function null, every "not part of this build" refusal fires -- and (b) with tests/sched_trace/mode_standin.hip, where the modes
are accepted, end the resident state and are dispatched to.  tests/golden/mode_options_parent.json holds what the same test
sources printed when built against the library sources of the parent commit it names (recorded by running this file as a script:
see the end); return codes, texts, option values and state flags must be equal record by record.
"""
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sched_trace_harness as H  # noqa: E402

GOLDEN = os.path.join(H.ROOT, "tests", "golden", "mode_options_parent.json")
INT_MIN, INT_MAX = -2**31, 2**31 - 1
# id -> (lo, hi, an interior value)
RANGES = {48: (0, 1, 1), 49: (1, 128, 5), 50: (0, 2, 1), 51: (1, 128, 3), 52: (0, 1, 1), 53: (0, 1, 1), 54: (0, 128, 2),
          55: (16, 65536, 1024), 56: (0, 128, 4), 57: (0, INT_MAX, 8)}
EXTRA = {55: [15, 17, 24, 32, 65536, 65552]}
# what the dispatch calls run under
MODES = [[], [(48, 1)], [(49, 5), (48, 1)], [(50, 1)], [(50, 2)], [(51, 3)], [(51, 3), (52, 1)], [(53, 1)], [(54, 2)],
         [(53, 1), (54, 2)], [(55, 64), (54, 2)], [(56, 4)], [(57, 8), (56, 4)], [(51, 3), (53, 1)], [(50, 1), (56, 4)]]


def values(oid):
    lo, hi, mid = RANGES[oid]
    out = []
    for v in [lo - 1, lo, lo + 1, mid, hi - 1, hi, hi + 1, INT_MIN, INT_MAX] + EXTRA.get(oid, []):
        if INT_MIN <= v <= INT_MAX and v not in out:
            out.append(v)
    return out


def script():
    s = []
    for oid in sorted(RANGES):
        for v in values(oid):
            # on a fresh handle; then behind a successful factor, where 50 / 51 / 52 end the resident state on a change only:
            # the same value once more behind a second factor must leave it
            s += ["handle 100 2", "set %d %d" % (oid, v), "get %d" % oid]
            s += ["handle 100 2", "factor", "set %d %d" % (oid, v), "get %d" % oid, "factor", "set %d %d" % (oid, v), "get %d" % oid]
    # option 50 = 2 needs d <= 127
    s += ["handle 100 128"] + ["set 50 %d" % v for v in (0, 1, 2, 3, 2, 0)] + ["get 50"]
    # option 52 drops the outputs' block that a factor under option 51 allocates
    s += ["handle 100 2", "set 51 3", "factor", "set 52 1", "factor", "set 52 1", "set 52 0", "factor", "set 51 1", "set 52 1", "get 52"]
    for mode in MODES:
        sets = ["set %d %d" % kv for kv in mode]
        s += ["handle 100 2"] + sets + ["predict_grad", "predict_cov", "factor", "predict_grad", "predict_cov", "lml_grad", "factor",
                                       "reserve 300", "predict_grad", "predict_cov"]
        s += ["get %d" % oid for oid in sorted(RANGES)]
    s += ["handle 100 2", "get 47", "get 58", "set 58 1", "get 99"]
    return s


def run_script(prog, lines, tmp_path):
    path = os.path.join(str(tmp_path), "modes_%s.txt" % os.path.basename(os.path.dirname(prog)))
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    r = subprocess.run([prog, path], capture_output=True, text=True)
    if r.returncode != 0 or r.stderr.strip():
        raise RuntimeError("the mode-option program exited with %d:\n%s" % (r.returncode, r.stderr[-4000:]))
    return [json.loads(l) for l in r.stdout.splitlines() if l]


def build(variant, **kw):
    return H.build_trace_program(main="modes_main.hip", extra=("mode_standin.hip",) if variant == "b" else (), **kw)


FLAGS = ("factored", "have_u", "have_kinv", "b_cond_k", "multi")


def pack(records):
    """the golden's form of a run: every text and every state (options 48-57 and the flags) once; a call's record is [return
    code, value of a get or None, index of the text, index of the state], a stand-in's line its name.  The calls themselves are
    the script's lines other than `handle`, in order."""
    texts, states, out = [], [], []
    for r in records:
        if r["k"] == "mode":
            out.append(r["fn"])
            continue
        state = r["options"] + [r[f] for f in FLAGS]
        for table, item in ((texts, r["err"]), (states, state)):
            if item not in table:
                table.append(item)
        out.append([r["ret"], r.get("value"), texts.index(r["err"]), states.index(state)])
    return {"texts": texts, "states": states, "records": out}


def unpack(packed, lines):
    calls = iter(l for l in lines if not l.startswith("handle"))
    out = []
    for r in packed["records"]:
        if isinstance(r, str):
            out.append({"k": "mode", "fn": r})
            continue
        state = packed["states"][r[3]]
        rec = {"k": "call", "call": next(calls), "ret": r[0], "err": packed["texts"][r[2]], "options": state[:10],
               **dict(zip(FLAGS, state[10:]))}
        if r[1] is not None:
            rec["value"] = r[1]
        out.append(rec)
    return out


def compare(got, packed, variant):
    want = unpack(packed, golden()["script"])
    assert len(got) == len(want), "variant %s: %d records, the parent printed %d" % (variant, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "variant %s, record %d:\n  here:   %s\n  parent: %s" % (variant, i, json.dumps(g), json.dumps(w))


def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def test_script_is_the_recorded_one():
    assert script() == golden()["script"]


def test_script_covers_the_issue():
    calls = set(script())
    for oid, (lo, hi, mid) in RANGES.items():
        for v in (lo - 1, lo, lo + 1, mid, hi - 1, hi, hi + 1, INT_MIN, INT_MAX):
            assert v > INT_MAX or v < INT_MIN or "set %d %d" % (oid, v) in calls
    assert all("set 55 %d" % v in calls for v in EXTRA[55])
    assert {"factor", "lml_grad", "predict_grad", "predict_cov", "reserve 300"} <= calls


def test_without_the_mode_files(tmp_path):
    g = golden()
    got = run_script(build("a"), g["script"], tmp_path)
    assert not [r for r in got if r["k"] == "mode"]
    assert any("is not part of this build" in r["err"] for r in got)
    compare(got, g["a"], "a")


def test_with_mode_standins(tmp_path):
    g = golden()
    got = run_script(build("b"), g["script"], tmp_path)
    fns = {r["fn"] for r in got if r["k"] == "mode"}
    assert fns >= {"loo_objective", "trend_objective", "trend_factor", "multi_objective", "multi_factor", "multi_reserve", "mean_sweep",
                   "path_sweep", "design_select"}
    assert any(r["k"] == "call" and r["multi"] == 1 for r in got)
    compare(got, g["b"], "b")


def test_sanitized(tmp_path):
    """both variants under AddressSanitizer and UBSan (stand-alone host programs): the same records, no report"""
    g = golden()
    for variant in ("a", "b"):
        compare(run_script(build(variant, sanitize=True), g["script"], tmp_path), g[variant], variant)


if __name__ == "__main__":
    # python tests/test_mode_options_host.py PARENT_TREE PARENT_HASH: PARENT_TREE is a checkout of the parent commit with THIS
    # tree's tests/sched_trace copied over its own (the same test sources against the parent's library sources); the parent's
    # handle names its outputs' block multi_blk
    import tempfile

    tree, commit = sys.argv[1:]
    rec = {"parent": commit, "script": script()}
    with tempfile.TemporaryDirectory() as tmp:
        for variant in ("a", "b"):
            prog = build(variant, root=os.path.abspath(tree), defines=("MULTI_BLOCK(h)=(h)->multi_blk",))
            rec[variant] = pack(run_script(prog, rec["script"], tmp))
    with open(GOLDEN, "w") as fh:
        json.dump(rec, fh, separators=(",", ":"))
        fh.write("\n")
