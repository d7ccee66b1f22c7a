"""Register budgets of the sparse bound's kernels (csrc/sparse_f64.hip), read from the code object's metadata (no GPU needed), in
the manner of test_path_kernel_registers.py.  The contraction kernel is the rectangular twin of grad_contract_kernel and is bound
like it by LDS and exp latency, not by issue, so it is built for the same occupancies: one component for three waves per SIMD
(at most 168 VGPRs, the allocation granule below 512 / 3), two components without a rational quadratic for two (at most 256);
the others run one wave per SIMD and may use accumulation registers beyond 256, as their twins do (test_kernel_registers.py
bounds the same two).  No kernel may spill a vector register to memory."""
import os

import pytest

from test_path_kernel_registers import ROOT, chk, kernel_registers

OBJ = os.path.join(ROOT, "andvaranaut_amd", "csrc", "sparse_f64.o")


def test_no_sparse_kernel_spills_and_the_contraction_keeps_its_occupancy():
    if not os.path.exists(OBJ) or not os.path.exists(os.path.join(chk.LLVM, "llvm-readelf")):
        pytest.skip("csrc/sparse_f64.o or llvm-readelf missing (run __graft_entry__.build() first)")
    seen = kernel_registers(OBJ)
    contract = {k: v for k, v in seen.items() if "sparse_contract_kernel" in k}
    # 5 component slots x (no rational quadratic, one), and the accumulate, v / yy, B, scale, scalars, H / G0 and reduce kernels
    assert len(contract) == 10 and len(seen) == 17, sorted(seen)
    for k, (vg, sp, _) in sorted(seen.items()):
        print(f"{k}: {vg} VGPRs, {sp} spilled")
        assert sp == 0, (k, sp)
    one = [v for k, v in contract.items() if "ILi1E" in k]
    assert len(one) == 2 and all(vg <= 168 for vg, _, _ in one), one
    two = [v for k, v in contract.items() if "ILi2ELb0E" in k]
    assert len(two) == 1 and two[0][0] <= 256, two
    assert all(vg <= 64 for k, (vg, _, _) in seen.items() if k not in contract)  # the helpers: full occupancy
