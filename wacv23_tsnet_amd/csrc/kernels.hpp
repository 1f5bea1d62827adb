// kernels.hpp -- launchers of the convolution kernels and the large-map flow kernel.  Each kernel family lives in its own translation unit
// (conv_h2_launch.cpp, conv_h2r_launch.cpp, conv_g64_launch.cpp, conv_w1_launch.cpp, flow_p_launch.cpp) so that the library builds in parallel and the MFMA
// kernels build without the SLP vectorizer; engine.cpp holds the host logic and the small kernels.
#pragma once
#include <hip/hip_runtime.h>

#include "conv_common.hpp"
#include "conv_plan.hpp"
#include "flow_args.hpp"

namespace tsnet {

// The convolution launchers DISPATCH: run_conv fills ConvArgs from the ConvPlan (conv_plan.hpp: plan_conv has validated the layer and plans
// instantiated kernels only); a family with several tiles takes the plan and runs the instantiation it names -- none is a bug, std::logic_error.
// nprod: 1 (bf16 operands), 16 (kNprodF16: one fp16 plane; every family but conv_w1), 3, or 4 (h2 only); affine = a.in_alpha != null; kernel size from a.taps.  abl / opt: tools build only, outside the plan.
// conv_h2.hpp -- patch kernels:
//   h2  (3x3 / stride 1): rows x width in {4x32, 4x64, 4x128, 2x128}, the bf16 4x128 tile's side-by-side wave grid, two K groups (4x32, 4x64)
//   h2s (7x7 stem, 8 input channels): 4 x 64
//   h2d (3x3 / stride 2): 4x64 (four waves), 4x128 (eight waves), 2x128 (four waves) and its deep schedule
void launch_conv_h2(const ConvArgs& a, const ConvPlan& p, int nprod, int abl, int opt, hipStream_t s);
void launch_conv_h2s(const ConvArgs& a, int nprod, hipStream_t s);
void launch_conv_h2d(const ConvArgs& a, const ConvPlan& p, int nprod, hipStream_t s);
// conv_w1.hpp -- 3x3 / stride 1 / pad 1 as Winograd F(2,3) along x: 4 x 32 pixels x 64 channels per tile (eight waves); the layer's
// weights are the TRANSFORMED filters (12 "taps": tap row ky x position p, pack_weights_kernel with kh = 3, kw = 4)
void launch_conv_w1(const ConvArgs& a, int nprod, int abl, hipStream_t s);      // abl: tools build only
// conv_h2r.hpp -- general implicit GEMM: ks in {1, 3, 7}, 128 positions x 64 (any) or 128 (ks = 3, Cin >= 16) channels; Cin = 8 or a multiple of 16
void launch_conv_h2r(const ConvArgs& a, const ConvPlan& p, int nprod, hipStream_t s);
// conv_g64.hpp -- the same GEMM in 64-deep K steps (Cin, and the concat split, multiples of 64; Npad a multiple of 128): ks in {1, 3},
// 64 (four waves) or 128 (eight waves) positions x 128 channels; the same bits as conv_h2r
void launch_conv_g64(const ConvArgs& a, const ConvPlan& p, int nprod, hipStream_t s);
// conv_h2s32.hpp -- 7 x 7 stems at 32 raw input channels (the pose model) as a patch kernel: 4 x 32 pixels x 64 channels; the same bits as conv_h2r
void launch_conv_h2s32(const ConvArgs& a, int nprod, hipStream_t s);

// head_mfma.hpp -- the RGB head on the matrix pipe (2 x 4 output pixels x 3 channels folded into the MFMA's N); built in conv_g64_launch.cpp
struct HeadMfmaArgs {
    const float* x;             // (N,H,W,C) raw output of the last up-convolution, NHWC (bf16 if x_bf16)
    const float* alpha;         // (N*C) InstanceNorm scale / shift of x
    const float* beta;
    const unsigned short* wq;   // folded filter planes [C/8 stages][40 steps][hi, lo][64 lanes][8] of w * 2^sw (pack_head_mfma_kernel)
    const float* w_unscale;     // device scalar 2^-sw
    const float* bias;          // (3)
    float* y;                   // (N,3,H,W) NCHW
    int N, H, W, C;
    int composite, fore_x0, fore_x1;
    float bg[3];
    int x_bf16;
    float in_scale, in_unscale; // 2^sa, 2^-sa from the bound sqrt(H W)
};

constexpr size_t head_mfma_table_halves(int C) { return (size_t)(C / 8) * 40 * 2 * 64 * 8; }     // 16-bit entries of the folded filter planes (80 C x 32 x 2)
void launch_head_mfma(const HeadMfmaArgs& a, int rows, hipStream_t s);                             // rows: 8, 16 or 32 (tile height)
void pack_head_mfma(const float* w_oihw_dev, int C, float scale, unsigned short* planes, hipStream_t s);

// flow_persist.hpp -- flow_kernel_p: a.K, a.G (flowp_plan), a.part, a.cnt set by the caller; variant: tools build only
void launch_flow_p(const FlowArgs& a, int variant, hipStream_t s);
// flow_sweep.hpp -- flow_kernel<NT>: NT = 1 or 2 target blocks per workgroup, `grid` workgroups, `lds` = flow_lds_bytes(NT, h, w, C)
void launch_flow(const FlowArgs& a, int NT, size_t lds, unsigned grid, hipStream_t s);

// dynamic LDS above the default limit needs hipFuncAttributeMaxDynamicSharedMemorySize: set once per (kernel, device), not per launch
void ensure_dynamic_lds(const void* kernel, size_t bytes);
// a convolution kernel on one workgroup per tile of the plan
template <class Kernel>
void launch_tiles(Kernel k, int threads, size_t lds, const ConvArgs& a, hipStream_t s) {
    ensure_dynamic_lds(reinterpret_cast<const void*>(k), lds);
    hipLaunchKernelGGL(k, dim3(a.tiles_m * a.tiles_n), dim3(threads), lds, s, a);
}

}  // namespace tsnet
