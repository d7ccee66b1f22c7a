"""Register budgets of the kernels behind the sparse bound's gradients by the data (csrc/sparse_xgrad_f64.hip), read from the code
object's metadata (no GPU needed), in the manner of test_sparse_zgrad_kernel_registers.py.  sparse_xgrad_kernel is
sparse_zgrad_kernel with the owned and the walked set exchanged: no instantiation may spill a vector register, and one component
-- the hot case -- keeps two waves per SIMD for every window width (at most 256 VGPRs) with nothing in scratch memory.  Composite
kernels may keep r2 and the coefficient tiles in scratch memory behind the rolled coefficient loop, as their twins do."""
import os

import pytest

from test_path_kernel_registers import ROOT, chk, kernel_registers

OBJ = os.path.join(ROOT, "andvaranaut_amd", "csrc", "sparse_xgrad_f64.o")


def test_no_xgrad_kernel_spills_and_one_component_uses_no_scratch():
    if not os.path.exists(OBJ) or not os.path.exists(os.path.join(chk.LLVM, "llvm-readelf")):
        pytest.skip("csrc/sparse_xgrad_f64.o or llvm-readelf missing (run __graft_entry__.build() first)")
    seen = kernel_registers(OBJ)
    xgrad = {k: v for k, v in seen.items() if "sparse_xgrad_kernel" in k}
    # 5 component slots x 3 window widths, and dF/dy's kernel
    assert len(xgrad) == 15 and len(seen) == 16, sorted(seen)
    for k, (vg, sp, pv) in sorted(seen.items()):
        print(f"{k}: {vg} VGPRs, {sp} spilled, {pv} bytes of scratch per lane")
        assert sp == 0, (k, sp)
    one = [v for k, v in xgrad.items() if "ILi1ELi" in k]
    assert len(one) == 3 and all(vg <= 256 and pv == 0 for vg, _, pv in one), one
    assert all(vg <= 64 for k, (vg, _, _) in seen.items() if k not in xgrad)  # the small kernel: full occupancy
