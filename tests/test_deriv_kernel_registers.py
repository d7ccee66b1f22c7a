"""Register budgets of the two kernels of the gradient binding (csrc/deriv_f64.hip), read from the code object's metadata (no GPU
needed), in the manner of test_sparse_xgrad_kernel_registers.py.  Both carry a 4x4 micro-tile per thread -- the assembly its
squared distances, the contraction three coefficient tiles -- and take the dimension of a row's component from LDS, never by
indexing registers: nothing may spill and nothing may live in scratch memory.  Recorded at the commit that added them:
deriv_assemble_kernel 128 (RBF) and 128 (Matern-5/2) VGPRs, deriv_contract_kernel 208 and 212 (two waves per SIMD),
deriv_final_kernel 8."""
import os

import pytest

from test_path_kernel_registers import ROOT, chk, kernel_registers

OBJ = os.path.join(ROOT, "andvaranaut_amd", "csrc", "deriv_f64.o")


def test_deriv_kernels_use_no_scratch():
    if not os.path.exists(OBJ) or not os.path.exists(os.path.join(chk.LLVM, "llvm-readelf")):
        pytest.skip("csrc/deriv_f64.o or llvm-readelf missing (run __graft_entry__.build() first)")
    seen = kernel_registers(OBJ)
    asm = {k: v for k, v in seen.items() if "deriv_assemble_kernel" in k}
    con = {k: v for k, v in seen.items() if "deriv_contract_kernel" in k}
    # two kernel families each, and the final reduction
    assert len(asm) == 2 and len(con) == 2 and len(seen) == 5, sorted(seen)
    for k, (vg, sp, pv) in sorted(seen.items()):
        print(f"{k}: {vg} VGPRs, {sp} spilled, {pv} bytes of scratch per lane")
        assert sp == 0 and pv == 0, (k, sp, pv)
    assert all(vg <= 128 for vg, _, _ in asm.values())  # four waves per SIMD: 256 threads per workgroup, two workgroups per CU
    assert all(vg <= 256 for vg, _, _ in con.values())
