"""CPU tier: every instantiation of the RGB head's folded MFMA kernel (csrc/head_mfma.hpp) fits two waves per SIMD (<= 256 VGPRs) and keeps
its main loop free of scratch operations (tools/isa_check.py compiles the unit for gfx950; hipcc cross-compiles without a GPU)."""
import os
import shutil

import pytest

from test_isa import _isa_check


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("c++filt") is None, reason="needs hipcc and c++filt")
def test_folded_head_registers_and_scratch():
    ic = _isa_check()
    asm = ic.compile_asm(unit="conv_g64_launch.cpp")
    res = ic.kernel_resources(asm, "head_mfma_kernel<")
    assert len(res) == 3, res                                    # tile heights 8, 16, 32
    for name, (vgpr, _) in res.items():
        assert vgpr <= 256, (name, vgpr)
    rows = ic.analyse(asm, "head_mfma_kernel<")
    assert len(rows) == 3, rows
    for r in rows:
        assert r["mfma"] >= 60 and r["scratch"] == 0, r         # the loop spanning the most MFMAs is the K loop (20 steps of 3 or 6 MFMAs)
    inner = ic.scratch_in_inner_loops(asm, "head_mfma_kernel<")
    assert len(inner) == 3 and all(v == 0 for v in inner.values()), inner
