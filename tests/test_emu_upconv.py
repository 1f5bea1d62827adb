"""CPU tier: the decoder's up-convolution with the x2 upsample formed in the patch staging (tsnet_op_upconv2d, conv_h2.hpp UP2) on the emulation
build -- the cases of upconv_cases.py: the fused route and upsample2x + convolution give the same bits, and both match the fp64 reference."""
import os
import subprocess

import pytest

import upconv_cases as uc

REL = 2e-6     # test_emu_ops.REL: the patch kernel's error relative to max|fp64 reference|


@pytest.mark.parametrize("case", uc.CASES, ids=[c[0] for c in uc.CASES])
def test_fused_upconv_matches_two_launches_and_reference(emu_lib, case):
    uc.check_case(emu_lib, "cpu", case, REL)


def test_upconv_refusals_leave_the_output_untouched(emu_lib):
    uc.check_refusals(emu_lib, "cpu")


def test_planner_takes_the_half_resolution_input_on_the_patch_kernel_alone(tmp_path):
    """conv_plan.hpp on the host: ConvShape::up2 is planned for the reflection-padded fp16 x 2 form of the 3 x 3 / stride-1 patch kernel on its plain
    4 x 64 and 4 x 128 tiles; everything else is refused.  (plan_driver's line protocol carries no such field: a driver of its own.)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = next((c for c in ("/opt/rocm/lib/llvm/bin/clang++", "/usr/bin/clang++", "/usr/bin/g++", "/usr/bin/c++") if os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "up2_plan.cpp"
    src.write_text('''
#include <cstdio>
#include "%s/wacv23_tsnet_amd/csrc/conv_plan.hpp"
using namespace tsnet;
static ConvShape base() {
    ConvShape s; s.ks = 3; s.stride = 1; s.pad = 1; s.reflect = 1; s.cin = 128; s.cout = 64; s.npad = 64; s.kpad = 9 * 128;
    s.N = 4; s.H = 256; s.W = 256; s.transform = true; s.nprod = 3; s.up2 = true; return s;
}
static int plan(const ConvShape& s, const ConvRequest& r) {
    try { const ConvPlan p = plan_conv(s, r, 256); return p.up2 && p.family == ConvFamily::H2 ? p.rows * 1000 + p.width : -2; }
    catch (const std::invalid_argument&) { return -1; }
}
int main() {
    ConvShape s = base(); ConvRequest r;
    std::printf("%%d", plan(s, r));
    r.width = 128; s.cout = 128; s.npad = 128; std::printf(" %%d", plan(s, r));
    r = ConvRequest{}; s = base();
    { ConvShape t = s; t.reflect = 0; std::printf(" %%d", plan(t, r)); }
    { ConvShape t = s; t.stride = 2; std::printf(" %%d", plan(t, r)); }
    { ConvShape t = s; t.ks = 1; t.pad = 0; t.kpad = 128; std::printf(" %%d", plan(t, r)); }
    { ConvShape t = s; t.nprod = 1; std::printf(" %%d", plan(t, r)); }
    { ConvShape t = s; t.nprod = 1; t.f16 = true; std::printf(" %%d", plan(t, r)); }
    { ConvShape t = s; t.nprod = 4; std::printf(" %%d", plan(t, r)); }
    { ConvShape t = s; t.form = 1; t.kpad = 12 * 128; std::printf(" %%d", plan(t, r)); }
    { ConvShape t = s; t.H = 258; std::printf(" %%d", plan(t, r)); }
    { ConvRequest q; q.width = 32; std::printf(" %%d", plan(s, q)); }
    { ConvRequest q; q.rows = 2; q.width = 128; ConvShape t = s; t.cout = 128; t.npad = 128; std::printf(" %%d", plan(t, q)); }
    { ConvRequest q; q.rows = 4; q.width = 64; q.sched = ConvSched::TwoGroups; std::printf(" %%d", plan(s, q)); }
    { ConvRequest q; q.kernel = ConvKernel::General; std::printf(" %%d", plan(s, q)); }
    { ConvShape t = s; t.up2 = false; const ConvPlan p = plan_conv(t, r, 256); std::printf(" %%d", (int)p.up2); }
    std::printf(" %%d %%d\\n", (int)plan_takes_up2(s, 256), (int)plan_takes_up2([&] { ConvShape t = s; t.reflect = 0; return t; }(), 256));
    return 0;
}
''' % root)
    exe = tmp_path / "up2_plan"
    subprocess.check_call([cxx, "-std=c++17", "-O1", str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["4064", "4128"] + ["-1"] * 12 + ["0", "1", "0"], out
