"""Builds tests/sched_trace (the host-only trace program of the factorisation scheduler) and runs it.

The program links the host-only objects of andvaranaut_amd/csrc/api_gp.hip and gp_sched.hip against recording stand-ins;
no HIP runtime, no kernel file, no device.  Built lazily, once per test session and variant, into a fresh temporary directory
of the session's own.
"""
import atexit
import json
import os
import shutil
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "andvaranaut_amd", "csrc")
HERE = os.path.join(ROOT, "tests", "sched_trace")
STANDINS = ("hip_standin.hip", "kernel_standin.hip")
LIBRARY = ("gp_sched.hip", "api_gp.hip")
SANITIZE = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-Xarch_host", "-fno-omit-frame-pointer"]


def _hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return None


_built = {}  # variant -> path of the program or of one of its objects, this session


def build_trace_program(sanitize=False, main="trace_main.hip", extra=(), root=ROOT, defines=()):
    """path of the trace program (built on first use in this session); skips the calling test if there is no hipcc.  main: the
    file of tests/sched_trace with the program's main (modes_main.hip: the mode-option program); extra: further files of that
    directory; root / defines: another tree with the same layout and -D flags (the recording of tests/test_mode_options_host.py)"""
    variant = (sanitize, main, tuple(extra), root, tuple(defines))
    if variant in _built:
        return _built[variant]
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found: the schedule-trace program cannot be built")
    work = tempfile.mkdtemp(prefix="migp_sched_trace_")  # (mode 0700, ours alone)
    atexit.register(shutil.rmtree, work, ignore_errors=True)
    flags = ["--offload-host-only", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-result"] + (SANITIZE if sanitize else [])
    flags += ["-D" + d for d in defines]
    here, csrc = os.path.join(root, os.path.relpath(HERE, ROOT)), os.path.join(root, os.path.relpath(CSRC, ROOT))
    objs = []
    for src in [os.path.join(here, f) for f in STANDINS + (main,) + tuple(extra)] + [os.path.join(csrc, f) for f in LIBRARY]:
        key = (sanitize, src, tuple(defines))  # (the programs of a session share their objects)
        if key not in _built:
            obj = os.path.join(work, os.path.basename(src) + ".o")
            r = subprocess.run([hipcc] + flags + ["-c", src, "-o", obj], capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError("compiling %s failed:\n%s" % (src, r.stderr[-4000:]))
            _built[key] = obj
        objs.append(_built[key])
    # (-no-hip-rt: the stand-ins ARE the runtime; nothing of libamdhip64 is linked)
    prog = os.path.join(work, "sched_trace")
    r = subprocess.run([hipcc, "--offload-host-only", "-no-hip-rt"] + (SANITIZE if sanitize else []) + objs + ["-o", prog],
                       capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("linking the trace program failed:\n%s" % r.stderr[-4000:])
    _built[variant] = prog
    return prog


def ragged_n(ntc):
    """a point count whose last tile column is partly filled"""
    return 128 * ntc - 37


def config_line(ntc, entry, batch=0, panel_tiles=0, options=None, n=None, d=2):
    opts = " ".join("%s=%d" % kv for kv in (options or {}).items())
    return "%d %d %d %s %d %s" % (n if n is not None else ragged_n(ntc), d, batch, entry, panel_tiles, opts)


def run_traces(prog, lines, tmp_path):
    """the program's output for a list of configurations (one process)"""
    listing = os.path.join(str(tmp_path), "configs_%d.txt" % len(os.listdir(str(tmp_path))))
    with open(listing, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    r = subprocess.run([prog, "--file", listing], capture_output=True, text=True)
    if r.returncode not in (0, 1) or r.stderr.strip():
        raise RuntimeError("sched_trace exited with %d:\n%s" % (r.returncode, r.stderr[-4000:]))
    return r.stdout


def check_traces(prog, lines, tmp_path, replay=True):
    """[(index of the configuration, tile columns, return value, refused options, [findings as text])], one per configuration"""
    import sched_check as C

    evs = C.split_evaluations(run_traces(prog, lines, tmp_path))
    if len(evs) != len(lines):
        raise RuntimeError("%d traces for %d configurations" % (len(evs), len(lines)))
    return [(i, cfg["ntc"], end["ret"], cfg["refused"], [repr(f) for f in C.check(cfg, recs, replay=replay).findings])
            for i, (cfg, recs, end) in enumerate(evs)]


def check_traces_parallel(prog, lines, tmp_path, replay=True, workers=None):
    """check_traces() with the configurations dealt out to worker processes (this file run as a script): the traces are
    independent of each other, and the large sweeps are a few thousand of them"""
    if workers is None:
        workers = max(1, min(8, len(os.sched_getaffinity(0)) // 2, len(lines) // 200))
    if workers <= 1:
        return check_traces(prog, lines, tmp_path, replay)
    procs = []
    for w in range(workers):
        part = os.path.join(str(tmp_path), "part_%d_%d" % (len(os.listdir(str(tmp_path))), w))
        os.mkdir(part)
        with open(os.path.join(part, "lines.txt"), "w") as fh:
            fh.write("\n".join(lines[w::workers]) + "\n")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), prog, part, "1" if replay else "0"],
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    out = []
    for w, p in enumerate(procs):
        stdout, stderr = p.communicate()
        if p.returncode != 0:
            raise RuntimeError("checker worker %d failed:\n%s" % (w, stderr[-4000:]))
        out += [(w + workers * i, ntc, ret, refused, findings) for i, ntc, ret, refused, findings in json.loads(stdout)]
    return sorted(out)


def _worker(argv):
    prog, part, replay = argv
    with open(os.path.join(part, "lines.txt")) as fh:
        lines = [l for l in fh.read().splitlines() if l]
    json.dump(check_traces(prog, lines, part, replay == "1"), sys.stdout)


# ---------------------------------------------------------------------------------------------------------------- the sweeps
SWITCH_COUNTS = [1, 3, 4, 7, 8, 19, 20, 23, 24, 25, 31, 32, 33, 47, 48, 49, 60, 61, 64, 71, 72, 73, 96, 97, 130]

# every option set on its own ...
OPTION_SETS = [{26: 0}, {26: 1}, {26: 2}, {0: 0}, {0: 2}, {45: 0}, {37: 0}, {46: 0}, {35: 0}, {32: 0}, {21: 0}, {21: 16}, {20: 0},
               {20: 40}, {18: 0}, {18: 1024, 19: 256}, {8: 0}, {8: 1 << 20}, {30: 0}, {31: 16}, {31: 48}, {38: 1}, {38: 8}]
# ... and in the combinations of the GPU tests: SCHED_SETS of test_gpu_handle_layouts.py (with the 32 / 35 / 37 / 46 sets of
# test_gpu_stream_edges.py), the scheduling lists of test_gpu_stream_edges.py and test_gpu_headline_parity.py
OPTION_SETS += [{37: 0, 2: 2}]
OPTION_SETS += [dict(zip((32, 35, 37, 46), c)) for c in
                [(0, 32, 24, 31), (2048, 0, 24, 31), (2048, 32, 0, 31), (0, 0, 0, 31), (2048, 64, 34, 31), (64, 8, 12, 31),
                 (2048, 32, 24, 34), (2048, 32, 12, 40)]]
OPTION_SETS += [{26: 0, 0: 2}, {45: 0, 26: 0}, {30: 64, 31: 48}, {30: 4, 31: 16}, {18: 0, 20: 0, 21: 0}, {18: 1024, 19: 256, 20: 40},
                {26: 0, 21: 16}]
# test_gpu_stream_edges.py runs a batch under each 32 / 35 / 37 / 46 tuple with option 38 = 8, 1 and 3 ...
R5_TUPLES = [dict(zip((32, 35, 37, 46), c)) for c in
             [(2048, 32, 24, 31), (0, 32, 24, 31), (2048, 0, 24, 31), (2048, 32, 0, 31), (0, 0, 0, 31), (2048, 64, 34, 31), (64, 8, 12, 31),
              (2048, 32, 24, 34), (2048, 32, 12, 40)]]
BATCH_OPTION_SETS = [{**t, 38: g} for t in R5_TUPLES for g in (8, 1, 3)]
# ... and its scheduling list with the super-panel width pinned (option 2) to what the two-stream default picks, from 20 tile
# columns on: 4 up to 60 tile columns, 8 beyond
PINNED_SETS = [{}, {0: 0}, {0: 2}, {26: 0}, {26: 1}, {26: 0, 0: 2}, {21: 16}, {30: 0}, {45: 0}, {45: 0, 26: 0}]


def pinned_width(ntc):
    return None if ntc < 20 else 4 if ntc <= 60 else 8


PANEL_TILES = [1, 2, 3, 4, 8, 16]


if __name__ == "__main__":
    _worker(sys.argv[1:])
