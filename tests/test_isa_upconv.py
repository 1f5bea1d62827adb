"""CPU tier: the fused-upsample instantiations of the patch kernel (conv_h2u_kernel, csrc/conv_h2.hpp UP2) keep the occupancy their direct
twins are scheduled for -- the 4 x 64 tile three workgroups per CU (<= 168 VGPRs, <= 53 KB of LDS), the 4 x 128 tile two (<= 256 VGPRs) -- and
hold no scratch, in the slab loop or anywhere else (tools/isa_check.py compiles the unit for gfx950; hipcc cross-compiles without a GPU)."""
import os
import shutil

import pytest

from test_isa import _isa_check


def h2_lds_bytes(cin, up2):
    """csrc/conv_h2.hpp h2_lds_bytes for a four-row tile, one K group"""
    return 2 * 2 * 2 * 7 * 512 + 2048 + (2 * 4 * 18 * 64 if up2 else 0) + 2 * cin * 4


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("c++filt") is None, reason="needs hipcc and c++filt")
def test_fused_upsample_tiles_registers_lds_and_scratch():
    ic = _isa_check()
    asm = ic.compile_asm()
    res = ic.kernel_resources(asm, "conv_h2u_kernel<")
    assert len(res) == 4, res                                    # tiles 4 x 64 and 4 x 128, raw input and IN + ReLU
    for name, (vgpr, scratch) in res.items():
        assert vgpr <= (256 if "<4, 128," in name else 168), (name, vgpr)
        assert scratch == 0, (name, scratch)
    rows = ic.analyse(asm, "conv_h2u_kernel<")
    assert len(rows) == 4, rows
    for r in rows:
        assert r["mfma"] >= 108 and r["scratch"] == 0, r         # the slab pair: 18 steps of 6 or 12 MFMAs
    assert h2_lds_bytes(128, True) <= 53 * 1024                  # the decoder's last up-convolution: three workgroups in a CU's 160 KiB
    assert h2_lds_bytes(512, True) <= 53 * 1024                  # ... and the widest layer three of them fit with
