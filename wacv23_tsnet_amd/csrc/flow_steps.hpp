// flow_steps.hpp -- the steps flow_kernel<NT> (flow_sweep.hpp) and flow_kernel_p (flow_persist.hpp) both take, spelled once.  DEVICE code,
// compiled in flow_p_launch.cpp (built without the SLP vectorizer: flow_persist.hpp) and seen by engine.cpp.
// A step lives here only while both kernels keep their code, instruction for instruction (tools/isa_diff.py against the parent commit).
// The target-plane copy, the MFMA pair sweep, the online-softmax rescale and the fixed-order merges did not pass that test in any spelling
// tried and stay per kernel: profiles/between_convs_one_spelling.txt, section 2, has every form and its figures.
#pragma once
#include <hip/hip_runtime.h>
#include "flow_args.hpp"

namespace tsnet {

// F.interpolate(nearest) of mask number `image` of a stack m of (H, W) masks, at feature position p of the (h, w) map: src = dst * scale
__device__ __forceinline__ float flow_mask_at(const float* m, int image, const FlowArgs& a, int p) {
    const int py = p / a.w, px = p - py * a.w;
    return m[(size_t)image * a.H * a.W + (size_t)(py * a.sy) * a.W + px * a.sx];
}

}  // namespace tsnet
