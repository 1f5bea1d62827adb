// conv_g64_launch.cpp -- instantiations and launchers of the general implicit GEMM with 64-deep K steps (conv_g64.hpp) and of the 32-channel
// stem patch kernel (conv_h2s32.hpp): the two kernels that took over conv_h2r's hot layers in round 6; and of the RGB head's MFMA form
// (head_mfma.hpp), which needs this unit's build: no SLP vectoriser beside MFMAs.
#include <stdexcept>

#include "conv_g64.hpp"
#include "conv_h2s32.hpp"
#include "head_mfma.hpp"
#include "kernels.hpp"

namespace tsnet {
namespace {

template <int KS, int BM, int NPROD>
void go(const ConvArgs& a, hipStream_t s) {
    launch_tiles(a.in_alpha ? conv_g64_kernel<KS, BM, NPROD, true> : conv_g64_kernel<KS, BM, NPROD, false>, BM * 4, (size_t)g64_lds_bytes(BM, one_product(NPROD) ? 1 : 2, a.Cin), a, s);
}

template <int NPROD>
void go_np(const ConvArgs& a, const ConvPlan& p, hipStream_t s) {
    if (a.taps == 1 && p.rows == 64) return go<1, 64, NPROD>(a, s);
    if (a.taps == 1 && p.rows == 128) return go<1, 128, NPROD>(a, s);
    if (a.taps == 9 && p.rows == 64) return go<3, 64, NPROD>(a, s);
    if (a.taps == 9 && p.rows == 128) return go<3, 128, NPROD>(a, s);
    plan_not_built(p, NPROD);
}

}  // namespace

void launch_conv_g64(const ConvArgs& a, const ConvPlan& p, int nprod, hipStream_t s) {
    nprod == 3 ? go_np<3>(a, p, s) : (nprod == kNprodF16 ? go_np<kNprodF16>(a, p, s) : go_np<1>(a, p, s));
}

void launch_conv_h2s32(const ConvArgs& a, int nprod, hipStream_t s) {
    if (nprod == 3) launch_tiles(conv_h2s32_kernel<3>, 256, (size_t)h2s32_lds_bytes(2), a, s);
    else if (nprod == kNprodF16) launch_tiles(conv_h2s32_kernel<kNprodF16>, 256, (size_t)h2s32_lds_bytes(1), a, s);
    else launch_tiles(conv_h2s32_kernel<1>, 256, (size_t)h2s32_lds_bytes(1), a, s);
}

template <int TR>
static void go_head(const HeadMfmaArgs& a, hipStream_t s) {
    const size_t lds = head_mfma_lds_bytes(TR, a.C);
    ensure_dynamic_lds(reinterpret_cast<const void*>(head_mfma_kernel<TR>), lds);
    hipLaunchKernelGGL(head_mfma_kernel<TR>, dim3(((a.W + 31) / 32) * ((a.H + TR - 1) / TR), a.N), dim3(hm_threads(TR)), lds, s, a);
}

void launch_head_mfma(const HeadMfmaArgs& a, int rows, hipStream_t s) {
    if (rows == 32) go_head<32>(a, s);
    else if (rows == 16) go_head<16>(a, s);
    else if (rows == 8) go_head<8>(a, s);
    else throw std::logic_error("head_mfma: tile rows must be 8, 16 or 32");
}

void pack_head_mfma(const float* w_oihw_dev, int C, float scale, unsigned short* planes, hipStream_t s) {
    hipLaunchKernelGGL(pack_head_mfma_kernel, dim3(64), dim3(256), 0, s, w_oihw_dev, planes, C, scale);
}

}  // namespace tsnet
