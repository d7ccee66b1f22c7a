"""Register budgets of the path sweep's kernels (csrc/paths_f64.hip), read from the code object's metadata (no GPU needed), in the
manner of test_kernel_registers.py: a thread carries T path accumulators and, with the gradient, T x window gradient
accumulators, so every instantiation must stay without spills and at or below 256 VGPRs, the occupancy cliff."""
import os
import re
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_uninit_check as chk  # noqa: E402

OBJ = os.path.join(ROOT, "andvaranaut_amd", "csrc", "paths_f64.o")


def kernel_registers(obj):
    """{kernel symbol: (vgpr_count, vgpr_spill_count, private_segment_fixed_size)} of a HIP object file."""
    tmp = tempfile.mkdtemp(prefix="pathregs")
    local = os.path.join(tmp, os.path.basename(obj))
    with open(local, "wb") as f:
        f.write(open(obj, "rb").read())
    subprocess.run([f"{chk.LLVM}/llvm-objdump", "--offloading", local], check=True, capture_output=True)
    dev = [f for f in os.listdir(tmp) if "amdgcn" in f and f.startswith(os.path.basename(obj))]
    assert dev, os.listdir(tmp)
    text = subprocess.check_output([f"{chk.LLVM}/llvm-readelf", "--notes", os.path.join(tmp, dev[0])], text=True)
    seen = {}
    for block in text.split("- .agpr_count:")[1:]:
        name = re.search(r"^    \.name:\s+(\S+)", block, re.M)
        vg = re.search(r"\.vgpr_count:\s+(\d+)", block)
        sp = re.search(r"\.vgpr_spill_count:\s+(\d+)", block)
        pv = re.search(r"\.private_segment_fixed_size:\s+(\d+)", block)
        if name and vg:
            seen[name.group(1)] = (int(vg.group(1)), int(sp.group(1)) if sp else 0, int(pv.group(1)) if pv else 0)
    return seen


def test_no_path_kernel_spills_or_passes_256_vgprs():
    if not os.path.exists(OBJ) or not os.path.exists(os.path.join(chk.LLVM, "llvm-readelf")):
        pytest.skip("csrc/paths_f64.o or llvm-readelf missing (run __graft_entry__.build() first)")
    seen = kernel_registers(OBJ)
    sweeps = {k: v for k, v in seen.items() if "path_sweep_kernel" in k}
    # 5 component slots x gradient yes / no x 3 windows, and the stage, stage-V, reduce, residual and scatter kernels
    assert len(sweeps) == 30 and len(seen) == 35, sorted(seen)
    for k, (vg, sp, _) in sorted(seen.items()):
        print(f"{k}: {vg} VGPRs, {sp} spilled")
        assert sp == 0, (k, sp)
        assert vg <= 256, (k, vg)
