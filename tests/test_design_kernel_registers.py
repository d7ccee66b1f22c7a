"""Register budgets of the design call's kernels (csrc/design_f64.hip), read from the code object's metadata (no GPU needed), in the
manner of test_sparse_kernel_registers.py.  The three kernels of a step are bound by memory, not by issue: none may spill a vector
register or use scratch, the streaming passes (row sums, fused update) keep full occupancy (at most 64 VGPRs), and the candidate
column, which also evaluates the kernel function, keeps four waves per SIMD (at most 128)."""
import os

import pytest

from test_path_kernel_registers import ROOT, chk, kernel_registers

OBJ = os.path.join(ROOT, "andvaranaut_amd", "csrc", "design_f64.o")


def test_no_design_kernel_spills_or_uses_scratch():
    if not os.path.exists(OBJ) or not os.path.exists(os.path.join(chk.LLVM, "llvm-readelf")):
        pytest.skip("csrc/design_f64.o or llvm-readelf missing (run __graft_entry__.build() first)")
    seen = kernel_registers(OBJ)
    assert len(seen) == 4, sorted(seen)
    for k, (vg, sp, pv) in sorted(seen.items()):
        print(f"{k}: {vg} VGPRs, {sp} spilled, {pv} bytes of scratch")
        assert sp == 0 and pv == 0, (k, sp, pv)
        assert vg <= (128 if "design_column_kernel" in k else 64), (k, vg)
