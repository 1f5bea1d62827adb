// engine.cpp -- host side of the TS-Net forward engine behind include/tsnet_abi.h.
//
// Compiled with hipcc for gfx950 (the product) and, by tests only, with a host compiler against tests/emu's HIP emulation headers so
// that the launch geometry / indexing logic of every kernel can be checked against the oracle without a GPU.  There is no CPU fallback
// in the product: every entry point launches HIP kernels and reports HIP failures through tsnet_last_error.
//
// ONE schedule (reference: model/TSNet.py:309-407), NHWC fp32 activations throughout, the K sources batched into one launch per layer
// (image index n = s*B + b):
//   pack_input -> img_enc (stem 7x7, 3 stride-2 convs, 9 ResnetBlocks)           [A2, A4]
//   pack_input -> lbl_enc (stem + 3 stride-2 convs)                              [A3]      (side stream)
//   l2norm x2 -> flow_kernel -> warp_mean_kernel                                 [A5, A6]  (side stream)
//   fuse conv1 (per-source half + shared target half) -> conv2 -> residual+mean -> 1x1 conv   [A7, A6]
//   dec map 1x1 (cat on load) -> ResnetBlocks -> 3x (upsample, conv) -> 7x7+tanh [A8, A9]
// Every convolution reads the producer's RAW fp32 output and applies that producer's InstanceNorm + ReLU while it stages its operand
// tile; operands enter the matrix pipe as fp16 x 2 splits (three products) or, with tsnet_cfg.operand_mode = 1 / 3, as one bf16 / fp16 plane.
// Which kernel a layer runs on (the Winograd-along-x kernel of conv_w1.hpp for the ResnetBlock / FuseNet layers and the first two
// up-convolutions, the patch kernels of conv_h2.hpp where the output splits into 4 x 32 rectangles, the general implicit GEMM of
// conv_g64.hpp / conv_h2r.hpp elsewhere) and which tile it takes depend on the layer and the frame size only -- never on the batch, never
// on the environment.  Three launch parameters DO follow the batch -- conv_w1's tiles per workgroup, the stride-2 tile's deep schedule and the
// RGB head's tile rows -- and are bit-neutral by construction (the same chains per output element in every form): a frame's result is the
// same bits alone (B = 1) and in any batch
// (tests/test_gpu_forward.py::test_single_frame_forward).  conv_plan.hpp holds these choices.
// InstanceNorm statistics: fp64 partial sums in the producing conv's epilogue, finalised there by the last-arriving workgroup
// (or by in_finalize2 when an image has many tiles).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/tsnet_abi.h"
#include "entry_common.hpp"
#include "conv_plan.hpp"
#include "kernels.hpp"
#include "flow_warp.hpp"
#include "head_conv.hpp"
#include "norm_elementwise.hpp"
#include "pack_weights.hpp"
#include "postproc.hpp"
#include "train_extras.hpp"

using namespace tsnet;

namespace {

int64_t g_launch_counters[4] = {0, 0, 0, 0};   // conv launches: [0] patch kernels (conv_h2.hpp), [1] general kernel (conv_h2r.hpp), [2] RGB head;
                                               // [3] = tile code (rows * 1000 + width, + 20000 two K groups) of the last ResnetBlock-class convolution launch
std::string g_create_error;

#ifdef TSNET_TOOLS
int g_tools_knob[8] = {3, 0, 0, 0, 0, 0, 0, 0};     // tools build only (tsnet_tools_set): [0] largest conv_w1 chunk the launcher may choose; [1] != 0: the decoder never takes the fused upsample; [2] != 0 (read when an engine is created): its second up-convolution stays on the direct kernel
#endif
inline int round_up(int x, int m) { return (x + m - 1) / m * m; }
static_assert(kPlanTileRows == kPatchRows && kPlanTileCols == kPatchCols, "conv_plan.hpp's patch tile is conv_common.hpp's");
// CUs of the current device (MI355X: 256 in 8 XCDs -- the XCD count is part of the kernels' block -> tile maps, conv_common.hpp; the CU count
// only enters launch heuristics: how many tiles fill the chip in whole rounds).  A device that reports nothing counts as 256.
inline int current_device_cus() {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v < 8) v = 256;
    return v;
}
inline int ilog2(int x) { int l = 0; while ((1 << l) < x) ++l; return l; }
inline int next_pow2(int x) { int p = 4; while (p < x) p <<= 1; return p; }

// ------------------------------------------------------------------------------------------------
// timing of launch classes (bench.py's roofline object)
struct Timing {
    bool on = false;
    struct Rec { int cls; hipEvent_t a, b; };
    std::vector<Rec> recs;
    double ms[TSNET_TIMING_CLASSES] = {0};
    int64_t launches[TSNET_TIMING_CLASSES] = {0};
    void begin(int cls, hipStream_t s) {
        if (!on) return;
        Rec r{cls, nullptr, nullptr};
        HIP_TRY(hipEventCreate(&r.a));
        HIP_TRY(hipEventCreate(&r.b));
        HIP_TRY(hipEventRecord(r.a, s));
        recs.push_back(r);
    }
    void end(hipStream_t s) {
        if (!on) return;
        HIP_TRY(hipEventRecord(recs.back().b, s));
    }
    void collect() {
        for (auto& r : recs) {
            HIP_TRY(hipEventSynchronize(r.b));
            float t = 0.f;
            HIP_TRY(hipEventElapsedTime(&t, r.a, r.b));
            ms[r.cls] += t;
            launches[r.cls] += 1;
            (void)hipEventDestroy(r.a);
            (void)hipEventDestroy(r.b);
        }
        recs.clear();
    }
};

struct Ctx {            // what a launch helper needs
    hipStream_t stream;
    int cus;            // CUs of the device the launches go to (launch heuristics only: conv_plan.hpp)
    Timing* timing = nullptr;
    int lane = 0;       // 0 = the caller's stream; 1 = the engine's side stream (own statistics scratch, see tsnet_forward)
    Ctx(hipStream_t s, int cus_, Timing* t = nullptr, int lane_ = 0) : stream(s), cus(cus_), timing(t), lane(lane_) {}
};

// a pair of timing events, destroyed on every exit path
struct EventPair {
    hipEvent_t a = nullptr, b = nullptr;
    EventPair() {
        HIP_TRY(hipEventCreate(&a));
        try { HIP_TRY(hipEventCreate(&b)); } catch (...) { (void)hipEventDestroy(a); throw; }
    }
    ~EventPair() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); }
    EventPair(const EventPair&) = delete;
    EventPair& operator=(const EventPair&) = delete;
    float ms() {            // between the two records, once b has completed
        HIP_TRY(hipEventSynchronize(b));
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, a, b));
        return t;
    }
};

// Scope guard of a fork onto the engine's side stream: if the scope is left before the explicit join (an exception between fork
// and join), the caller's stream still waits for whatever the side lane has in flight.
struct SideJoin {
    hipStream_t side, main; hipEvent_t ev; bool done = false;
    ~SideJoin() { if (!done && side && hipEventRecord(ev, side) == hipSuccess) (void)hipStreamWaitEvent(main, ev, 0); }
};

struct TimeScope {
    Ctx& c;
    TimeScope(Ctx& c_, int cls) : c(c_) { if (c.timing) c.timing->begin(cls, c.stream); }
    ~TimeScope() { if (c.timing) { try { c.timing->end(c.stream); } catch (...) {} } }
};

void launch_finalize_impl(const double* part, float* alpha, float* beta, int N, int C, int S, int HW, hipStream_t s);
inline void launch_finalize(const double* part, float* alpha, float* beta, int N, int C, int S, int HW, hipStream_t s) { launch_finalize_impl(part, alpha, beta, N, C, S, HW, s); }

// pack_input_kernel: grid.x blocks per image (grid.y = images), sized so the whole grid stays near 8 blocks per CU
inline int pack_grid(int hw) {
    int g = (hw + 255) / 256;
    if (g > 128) g = 128;
    return g < 1 ? 1 : g;
}
// ------------------------------------------------------------------------------------------------
// convolution layer description + launch
struct ConvLayer {
    std::string name;       // state_dict prefix, e.g. "img_enc.model.1"
    std::string wparam, bparam;   // parameter names feeding this layer (bparam empty = no bias)
    int cin_real = 0, cin_pad = 0, cout = 0, ks = 1, stride = 1, pad = 0, reflect = 0;
    int cin_total = 0, cin_off = 0;   // window of the parameter's input channels this layer consumes
    int kpad = 0, npad = 0;
    int form = 0;                     // 0: the filter as it is (ks x ks taps); 1: its Winograd F(2,3)-along-x transform, 3 x 4 "taps" (conv_w1.hpp)
    size_t w_off = 0, b_off = 0;          // offsets into the packed buffer: operand planes (16-bit units from the plane section), bias (floats)
    const unsigned short* wq = nullptr;   // device: operand planes [planes][K/16][Npad][2 octets][8] (conv_common.hpp pack_weights_kernel)
    const float* w_unscale = nullptr;     // device scalar 2^-sw (in the packed buffer: replicas receive it with the broadcast); null in the bf16 modes
    const float* bias = nullptr;          // device (cout)
};

// device allocations of an operator entry point: freed on every exit path (a rejected tile / variant throws out of run_conv routinely)
struct DevBufs {
    std::vector<void*> p;
    template <typename T> T* alloc(size_t bytes) { void* q = nullptr; HIP_TRY(hipMalloc(&q, bytes)); p.push_back(q); return static_cast<T*>(q); }
    ~DevBufs() { for (void* q : p) (void)hipFree(q); }
    DevBufs() = default;
    DevBufs(const DevBufs&) = delete;
    DevBufs& operator=(const DevBufs&) = delete;
};

// doubles a convolution's statistics scratch must hold: (sum, sum of squares) per (tile, channel)
inline size_t stat_part_doubles(size_t N, size_t tpi, size_t Cout) { return N * tpi * Cout * 2; }
constexpr int KPAD_ALIGN = 32;   // packed weights are K-padded to an even number of 16-deep chunks (fragment prefetch runs up to two past the end)

inline int conv_kpad(int ks, int cin_pad) { return round_up(ks * ks * cin_pad, KPAD_ALIGN); }
inline int conv_kpad_w1(int cin_pad) { return round_up(12 * cin_pad, KPAD_ALIGN); }    // Winograd-along-x form: tap row ky x position p
inline int conv_npad(int cout) { return cout >= 128 ? round_up(cout, 128) : round_up(cout, 64); }
inline int conv_cin_pad(int cin) { return cin <= 8 ? 8 : round_up(cin, 16); }     // 8 (two taps per k-group) or a multiple of 16

struct ConvCall {
    const float* x = nullptr; const float* x2 = nullptr;      // x2: channels >= csplit come from a second tensor (torch.cat on load), image n % x2_nmod
    int csplit = 0, x2_nmod = 1;
    const float* alpha = nullptr; const float* beta = nullptr; int relu = 0;   // x*alpha+beta (+ReLU) on load, or the raw tensor
    float bound = 0.f;          // max |operand| after the transform (InstanceNorm output: sqrt(HW); residual stream: (blocks+1) sqrt(HW))
    const unsigned* in_amax = nullptr; float bound_add = 0.f;   // or: bound = max |x| published on the device by x's producer + bound_add
    int N = 0, H = 0, W = 0;
    float* y = nullptr;
    const float* addend = nullptr; int add_nmod = 1;
    double* stat_part = nullptr; mutable int stat_S = 0;        // stat_S out: partials per image; 0 = none; -1 = finalised in the kernel
    float* fin_alpha = nullptr; float* fin_beta = nullptr; int* fin_counter = nullptr;
    unsigned* amax_out = nullptr;   // publish max |y| per image (operand scale of a consumer without an a-priori bound)
    int x_bf16 = 0, y_bf16 = 0; // bf16 storage mode (bf16-operand kernels only): the input / output tensor holds bf16
    int nprod = 3;              // products per k-group: 3 (4 adds lo*lo), 1 = bf16 operands, or TSNET_NPROD_F16 = one product on one fp16 plane
    int tclass = TSNET_T_CONV;
    bool up2 = false;           // x is the half-resolution map (N, H/2, W/2, Cin): the kernel forms its x2 upsample while staging (conv_h2.hpp UP2); alpha / beta / relu apply to x
};

// power-of-two operand scale: |x| <= bound  ->  |x * 2^sa| <= 2^15 < 65504 (fp16 max).  lim: the largest |sa|.  24 keeps the residual plane of
// the fp16 x 2 split meaningful; the one-plane fp16 kind has no residual and takes 64 (2^-(sa + sw) stays a normal fp32), so that its
// results are covariant with a power-of-two scaling of the input far outside fp16's own range.  A scale derived on the device from a
// published maximum (h2_device_scale, conv_common.hpp) keeps 24 in every kind.
inline int h2_scale_log2(float bound, int lim = 24) {
    if (!(bound > 0.f) || !std::isfinite(bound)) throw ArgError("conv: the operand bound must be positive and finite");
    int e = 0;
    (void)std::frexp(bound, &e);          // bound = m * 2^e, m in [0.5, 1)  ->  bound <= 2^e
    int sa = 15 - e;
    if (sa > lim) sa = lim;
    if (sa < -lim) sa = -lim;
    return sa;
}

// the layer and the call as the planner sees them
ConvShape conv_shape(const ConvLayer& L, const ConvCall& c) {
    const bool f16 = c.nprod == TSNET_NPROD_F16;
    ConvShape sh;
    sh.ks = L.ks; sh.stride = L.stride; sh.pad = L.pad; sh.reflect = L.reflect; sh.cin = L.cin_pad; sh.cout = L.cout; sh.npad = L.npad; sh.kpad = L.kpad;
    sh.form = L.form; sh.N = c.N; sh.H = c.H; sh.W = c.W; sh.csplit = c.x2 ? c.csplit : 0; sh.x2_nmod = c.x2_nmod > 0 ? c.x2_nmod : 1;
    sh.transform = c.alpha != nullptr; sh.nprod = f16 ? 1 : c.nprod; sh.f16 = f16; sh.fin_counter = c.stat_part && c.fin_counter;
    sh.up2 = c.up2; sh.x_bf16 = c.x_bf16 != 0;
    return sh;
}

// What depends on pointers is checked here; the layer, the geometry and the request by plan_conv (conv_plan.hpp), before anything is launched.
void run_conv(Ctx& ctx, const ConvLayer& L, const ConvCall& c, ConvRequest req = {}) {
    const bool bf16 = c.nprod == 1, f16 = c.nprod == TSNET_NPROD_F16;      // the two one-product kinds: unscaled bf16, or fp16 with the split path's scales
    if (!L.wq) throw ArgError("conv: layer has no packed weights");
    if (c.alpha && !c.beta) throw ArgError("conv: alpha without beta");
    if ((c.x_bf16 || c.y_bf16) && !bf16) throw ArgError("conv: bf16 storage goes with bf16 operands");
    if (c.x_bf16 && c.x2) throw ArgError("conv: bf16 storage of a concatenated input is not built");
    if (c.x2 && c.csplit == 0) throw ArgError("conv: a second tensor needs a channel split");
#ifdef TSNET_TOOLS
    req.chunk_cap = g_tools_knob[0];          // tools/forward_ab.py: the same forward with and without chunks, one process
#endif
    if (c.up2 && (c.x_bf16 || c.y_bf16 || c.in_amax)) throw ArgError("conv: the fused x2 upsample takes fp32 tensors and an a-priori operand bound");
    const ConvShape sh = conv_shape(L, c);
    ConvPlan p;
    try { p = plan_conv(sh, req, ctx.cus); } catch (const std::invalid_argument& e) { throw ArgError(e.what()); }
    ConvArgs g{};
    g.x = c.x; g.x2 = c.x2; g.in_alpha = c.alpha; g.in_beta = c.alpha ? c.beta : nullptr; g.in_relu = c.relu;
    const int sa = (bf16 || c.in_amax) ? 0 : h2_scale_log2(L.form == 1 ? 2.f * c.bound : c.bound, f16 ? 64 : 24);   // Winograd: |V| <= 2 max |x|
    g.in_scale = std::ldexp(1.0f, sa); g.in_unscale = std::ldexp(1.0f, -sa);
    g.in_amax = bf16 ? nullptr : c.in_amax; g.in_bound_add = c.bound_add; g.amax_out = c.amax_out;
    g.w = L.wq; g.w_unscale = bf16 ? nullptr : L.w_unscale; g.bias = L.bias; g.y = c.y;
    g.stat_part = c.stat_part; g.addend = c.addend; g.add_nmod = c.add_nmod > 0 ? c.add_nmod : 1;
    g.x_bf16 = c.x_bf16; g.y_bf16 = c.y_bf16;
    g.N = c.N; g.H = c.H; g.W = c.W; g.Cin = L.cin_pad; g.cin_log2 = ilog2(L.cin_pad);
    g.Csplit = c.x2 ? c.csplit : L.cin_pad; g.x2_nmod = sh.x2_nmod;
    g.Ho = sh.ho(); g.Wo = sh.wo();
    g.Cout = L.cout; g.Npad = L.npad; g.stride = L.stride; g.pad = L.pad; g.reflect = L.reflect;
    g.taps = L.form == 1 ? 12 : L.ks * L.ks; g.nchunks = (g.taps * g.Cin + 15) / 16; g.M = c.N * g.Ho * g.Wo;
    g.fin_alpha = c.fin_alpha; g.fin_beta = c.fin_beta; g.fin_eps = 1e-5f;
    // the one place a plan's launch geometry enters the kernel arguments
    g.tpi = p.tpi; g.tiles_m = p.tiles_m; g.tiles_n = p.tiles_n; g.fin_S = p.tpi; g.xcd_gn = p.xcd_gn;
    g.w1_chunk = p.w1_chunk; g.w1_tab2 = p.w1_tab2; g.fin_counter = p.fin ? c.fin_counter : nullptr;
    TimeScope ts(ctx, c.tclass);
    try {
        switch (p.family) {
        case ConvFamily::W1: launch_conv_w1(g, c.nprod, req.abl, ctx.stream); break;
        case ConvFamily::H2: launch_conv_h2(g, p, c.nprod, req.abl, req.opt, ctx.stream); break;
        case ConvFamily::H2S: launch_conv_h2s(g, c.nprod, ctx.stream); break;
        case ConvFamily::H2S32: launch_conv_h2s32(g, c.nprod, ctx.stream); break;
        case ConvFamily::H2D: launch_conv_h2d(g, p, c.nprod, ctx.stream); break;
        case ConvFamily::G64: launch_conv_g64(g, p, c.nprod, ctx.stream); break;
        case ConvFamily::H2R: launch_conv_h2r(g, p, c.nprod, ctx.stream); break;
        }
    } catch (const std::invalid_argument& e) { throw ArgError(e.what()); }      // a tools-build variant that is not instantiated
    ++g_launch_counters[p.family == ConvFamily::G64 || p.family == ConvFamily::H2R ? 1 : 0];
    if (c.tclass == TSNET_T_CONV_RES && plan_tile_code(p)) g_launch_counters[3] = plan_tile_code(p);
    check_launch("conv");
    c.stat_S = !c.stat_part ? 0 : (g.fin_counter ? -1 : g.tpi);
}

// InstanceNorm statistics -> (alpha, beta); `part` must hold N*64*C*2 doubles
void run_stats(Ctx& ctx, const float* x, int N, int HW, int C, double* part, float* alpha, float* beta) {
    if (C & 3) throw ArgError("instnorm: C must be a multiple of 4");
    TimeScope ts(ctx, TSNET_T_STATS);
    const int cq = C / 4, cols = cq < 256 ? cq : 256, R = 256 / cols;
    int S = (HW + R * 8 - 1) / (R * 8);
    if (S > 64) S = 64;
    if (S < 1) S = 1;
    const int rps = (HW + S - 1) / S;
    S = (HW + rps - 1) / rps;
    StatsArgs sa{x, part, HW, C, S, rps};
    hipLaunchKernelGGL(in_stats_partial_kernel, dim3(S, N, (cq + 255) / 256), dim3(256), 0, ctx.stream, sa);
    check_launch("in_stats_partial");
    launch_finalize(part, alpha, beta, N, C, S, HW, ctx.stream);
}

// stage 2 of the statistics: with more than a handful of partials per image the 16-group kernel (one serial walk per (image, channel)
// is latency-bound: 39 us for the 64 partials of the FuseNet join)
void launch_finalize_impl(const double* part, float* alpha, float* beta, int N, int C, int S, int HW, hipStream_t s) {
    if (S > 8) {
        hipLaunchKernelGGL(in_finalize2_kernel, dim3((C + kFin2Ch - 1) / kFin2Ch, N), dim3(256), 0, s, part, alpha, beta, C, S, HW, 1e-5f);
    } else {
        const int NC = N * C;
        hipLaunchKernelGGL(in_finalize_kernel, dim3((NC + 255) / 256), dim3(256), 0, s, part, alpha, beta, NC, C, S, HW, 1e-5f);
    }
    check_launch("in_finalize");
}

// y[n] = x[slot[n]] + add[n % add_nmod] with the InstanceNorm statistics of y -> (alpha, beta); `part` must hold N*64*C*2 doubles; slot: device, N ints
void run_add_stats(Ctx& ctx, const float* x, const int* slot, const float* add, int add_nmod, float* y, int N, int HW, int C, double* part, float* alpha, float* beta) {
    if (C & 3) throw ArgError("add_stats: C must be a multiple of 4");
    TimeScope ts(ctx, TSNET_T_STATS);
    const int cq = C / 4, cols = cq < 256 ? cq : 256, R = 256 / cols;
    int S = (HW + R * 8 - 1) / (R * 8);
    if (S > 64) S = 64;
    if (S < 1) S = 1;
    const int rps = (HW + S - 1) / S;
    S = (HW + rps - 1) / rps;
    const int nmod = add_nmod > 0 ? add_nmod : 1;
    AddStatsArgs sa{x, slot, add, y, part, HW, C, S, rps, nmod};
    hipLaunchKernelGGL(add_stats_partial_kernel, dim3(S, N, (cq + 255) / 256), dim3(256), 0, ctx.stream, sa);
    check_launch("add_stats_partial");
    // (its finalize stays a launch: 64 splits x 1024 channels per image are a megabyte of partials -- one last-arriving workgroup per image
    // would read them at a single block's rate, in_finalize2 spreads them over 64 x N)
    launch_finalize(part, alpha, beta, N, C, S, HW, ctx.stream);
}

void run_norm_act(Ctx& ctx, const float* x, const float* alpha, const float* beta, int relu, const float* resid,
                  int N, int HW, int C, float* y) {
    if (C & 3) throw ArgError("norm_act: C must be a multiple of 4");
    TimeScope ts(ctx, TSNET_T_ELEMWISE);
    NormActArgs a{x, alpha, beta, resid, y, HW, C, relu, (size_t)N * HW * C / 4};
    if ((double)HW * C / 4 >= 4294967295.0 || N > 65535) throw ArgError("norm_act: tensor too large");
    size_t per_img4 = (size_t)HW * C / 4, gx = (per_img4 + 255) / 256, cap = std::max<size_t>(1, 4096 / (size_t)N);
    if (gx > cap) gx = cap;
    hipLaunchKernelGGL(norm_act_kernel, dim3((unsigned)gx, N), dim3(256), 0, ctx.stream, a);
    check_launch("norm_act");
}

void run_upsample(Ctx& ctx, const float* x, const float* alpha, const float* beta, int relu, int N, int H, int W, int C, float* y, int x_bf16 = 0, int y_bf16 = 0) {
    if (C & 3) throw ArgError("upsample: C must be a multiple of 4");
    TimeScope ts(ctx, TSNET_T_UPSAMPLE);
    UpsampleArgs a{x, alpha, beta, y, N, H, W, C, relu, x_bf16, y_bf16};
    if (2 * H > 65535 || N > 65535) throw ArgError("upsample: tensor too large");
    const size_t row4 = (size_t)2 * W * C / 4;
    hipLaunchKernelGGL(upsample2x_kernel, dim3((unsigned)std::min<size_t>((row4 + 255) / 256, 64), 2 * H, N), dim3(256), 0, ctx.stream, a);
    check_launch("upsample2x");
}

// RGB head.  Widths that are multiples of 16 under a fused InstanceNorm + ReLU (every forward of a model with n_downsampling > 0: the
// operand then has the a-priori bound sqrt(H W)) run the folded MFMA form (head_mfma.hpp) on the packed planes `wq`; without the transform
// head_conv3_kernel (head_conv.hpp), and the one-pixel-per-thread form for narrower nets.  The choice depends on the width and on the
// presence of the transform alone, never on the batch; head_conv3's tile rows follow conv_plan.hpp head_rows, the folded form runs 8-row tiles,
// unless force_rows (8, 16, 32: operator tests) says otherwise; tile rows are bit-neutral in both.
void launch_head(const HeadArgs& ha, int hh, int ww, int B, hipStream_t s, int cus, int force_rows = 0, const unsigned short* wq = nullptr,
                 const float* wq_unscale = nullptr) {
    if (ha.C % (2 * kHead3Ch) == 0 && ha.alpha) {
        if (!wq || !wq_unscale) throw std::logic_error("head: the folded filter planes are missing");
        if ((double)B * hh * ww * ha.C * 4 >= 2147483648.0 || B > 65535) throw ArgError("head: tensor too large");
        HeadMfmaArgs m{};
        m.x = ha.x; m.alpha = ha.alpha; m.beta = ha.beta; m.wq = wq; m.w_unscale = wq_unscale; m.bias = ha.bias; m.y = ha.y;
        m.N = B; m.H = hh; m.W = ww; m.C = ha.C; m.composite = ha.composite; m.fore_x0 = ha.fore_x0; m.fore_x1 = ha.fore_x1;
        for (int c = 0; c < 3; ++c) m.bg[c] = ha.bg[c];
        m.x_bf16 = ha.x_bf16;
        const int sa = h2_scale_log2(std::sqrt((float)hh * (float)ww));        // |relu(IN(x))| <= sqrt(H W - 1)
        m.in_scale = std::ldexp(1.0f, sa); m.in_unscale = std::ldexp(1.0f, -sa);
        // 8-row tiles in every batch: 40 KB of LDS and 135 VGPRs put four workgroups = two waves on every SIMD, which hides the staging round trips
        // the 16- and 32-row tiles (one wave per SIMD) wait out: 53 against 78 - 80 us at B = 4, 28 against 63 us for one frame (profiles/head_mfma.txt)
        launch_head_mfma(m, force_rows ? force_rows : 8, s);
        check_launch("head_mfma");
        ++g_launch_counters[2];
        return;
    }
    if (ha.C % (2 * kHead3Ch) != 0) {
        if (force_rows) throw ArgError("head: the narrow head (C not a multiple of 16) has no tile rows to force");
        const int tiles = ((ww + kHeadT - 1) / kHeadT) * ((hh + kHeadT - 1) / kHeadT);
        hipLaunchKernelGGL(head_conv_kernel, dim3(tiles, B), dim3(256), 0, s, ha);
    } else {
        const int tiles_x = (ww + kHead3T - 1) / kHead3T;
        auto go = [&](auto tr) {
            constexpr int TR = decltype(tr)::value;
            const size_t lds = (size_t)(2 * (head3_patch_f4(TR) + kHead3WtsF4) + ha.C / 2) * sizeof(float4);
            ensure_dynamic_lds(reinterpret_cast<const void*>(head_conv3_kernel<TR>), lds);
            hipLaunchKernelGGL(head_conv3_kernel<TR>, dim3(tiles_x * ((hh + TR - 1) / TR), B), dim3(TR * 16), lds, s, ha);
        };
        const int rows = force_rows ? force_rows : head_rows(B, tiles_x, hh, cus);
        if (rows == 32) go(std::integral_constant<int, 32>{});
        else if (rows == 16) go(std::integral_constant<int, 16>{});
        else go(std::integral_constant<int, 8>{});
    }
    check_launch("head_conv");
    ++g_launch_counters[2];
}

// F.normalize over channels of N images of P positions -> the flow kernel's fp16 (hi, lo) operand planes (flow_plane_halves(N, P, C) halves)
void run_l2norm_split(Ctx& ctx, const float* x, unsigned short* q, int N, int P, int C) {
    if (C & 7) throw ArgError("l2norm: C must be a multiple of 8");
    TimeScope ts(ctx, TSNET_T_ELEMWISE);
    const int Ppad = flow_ppad(P);
    hipLaunchKernelGGL(l2norm_split_kernel, dim3((unsigned)(((size_t)N * Ppad + 3) / 4)), dim3(256), 0, ctx.stream, x, q, N, P, Ppad, C, flow_ksteps(C));
    check_launch("l2norm_split");
}

// variant (tsnet_op_flow_k; the forward passes 0): 1 = flow_kernel whatever the plan says; 2 = flow_kernel_p without the exp pass (tools build)
// slot (device, NB ints): the slot table, entry s*B + b the image of a.sq / a.src_bbox that (source s, driving frame b) reads
void run_flow(Ctx& ctx, FlowArgs a, int NB, const int* slot, int variant = 0) {
    if (a.C & 7) throw ArgError("flow: C must be a multiple of 8");
    a.slot = slot;
    if (variant < 0 || variant > 2) throw ArgError("flow: variant 0, 1 or 2");
    TimeScope ts(ctx, TSNET_T_FLOW);
    const size_t budget = 160 * 1024;
    // large maps (a.part / a.cnt supplied): persistent target tiles, the K sources of a batch element swept in G slices (flow_persist.hpp)
    const int G = (a.part && a.cnt && NB % a.B == 0 && NB / a.B <= 8 && variant != 1) ? flowp_plan(a.B, a.h, a.w, a.C) : 0;
    if (G) {
        a.K = NB / a.B; a.G = G; a.S = flowp_slices(a.h, a.w);
        try {
            launch_flow_p(a, variant, ctx.stream);
        } catch (const std::invalid_argument& e) { throw ArgError(e.what()); }
        check_launch("flow_p");
        return;
    }
    // 64 target positions per workgroup while their planes fit in LDS beside the mask row (C <= 512 at P <= 4096), else 32
    const int NT = flow_lds_bytes(2, a.h, a.w, a.C) <= budget ? 2 : 1;
    const size_t lds = flow_lds_bytes(NT, a.h, a.w, a.C);
    if (lds > budget) throw ArgError("flow: feature width / position count exceed the LDS budget");
    try {
        launch_flow(a, NT, lds, (unsigned)(flow_ppad(a.P) / (32 * NT) * NB), ctx.stream);
    } catch (const std::invalid_argument& e) { throw ArgError(e.what()); }
    check_launch("flow");
}

// slot (device, K*B ints): the slot table, entry s*B + b the image of src that (source s, driving frame b) reads
void run_warp(Ctx& ctx, const float* src, const int* slot, const float* flow, float* out, int B, int K, int h, int w, int C) {
    TimeScope ts(ctx, TSNET_T_WARP);
    WarpArgs a{src, flow, out, slot, B, K, h, w, C};
    hipLaunchKernelGGL(warp_mean_kernel, dim3(ew_grid((size_t)B * h * w * C / 4)), dim3(256), 0, ctx.stream, a);
    check_launch("warp_mean");
}

// Stem input assembly (pack_input_kernel) of p.S * p.B images.  `amax_clear` maxima from p.amax_out on are zeroed first: the images' own,
// or more where the caller resets neighbouring maxima of the same forward in the one memset.  The caller opens the timing scope.
void run_pack_input(Ctx& ctx, const PackArgs& p, size_t amax_clear) {
    if (p.amax_out) HIP_TRY(hipMemsetAsync(p.amax_out, 0, amax_clear * sizeof(unsigned), ctx.stream));
    hipLaunchKernelGGL(pack_input_kernel, dim3(pack_grid(p.H * p.W), p.S * p.B), dim3(256), 0, ctx.stream, p);
    check_launch(p.nimg ? "pack_input(img)" : "pack_input(lbl)");
}

// One call's inputs in either form.  wide: fp32 tensors as the reference's loaders leave them (img = byte - IMG_MEAN (B,3,H,W), lbl one-hot
// (B,L,H,W), bbox 0/1 floats (B,H,W)); compact (u8): the bytes they were made from (img (B,3,H,W), lbl class indices (B,H,W), bbox (B,H,W)) and
// the image mean, widened on load by pack_input_u8_kernel.
struct SrcIn {
    bool u8 = false;
    const void* const* img = nullptr;     // per source
    const void* const* lbl = nullptr;
    const void* const* bbox = nullptr;
    const float* mean = nullptr;          // u8: 3 HOST floats (B, G, R)
};
struct TarIn { bool u8 = false; const void* lbl = nullptr; const void* bbox = nullptr; };

// Stem input assembly from either form: p holds everything but the planes (p.img / p.lbl are filled here from S entries of img / lbl; img
// null: the label-only form).  Compact inputs also leave their masks widened at bbox_out (+ s * bbox_sstride + b * H*W) when bbox is given;
// wide masks are the caller's to copy.
void run_pack_any(Ctx& ctx, PackArgs p, size_t amax_clear, bool u8, const void* const* img, const void* const* lbl, const void* const* bbox,
                  const float* mean, float* bbox_out, size_t bbox_sstride) {
    if (!u8) {
        for (int s = 0; s < p.S; ++s) { p.img[s] = img ? static_cast<const float*>(img[s]) : nullptr; p.lbl[s] = static_cast<const float*>(lbl[s]); }
        run_pack_input(ctx, p, amax_clear);
        return;
    }
    PackU8Args q{};
    for (int s = 0; s < p.S; ++s) {
        q.img[s] = img ? static_cast<const unsigned char*>(img[s]) : nullptr;
        q.lbl[s] = static_cast<const unsigned char*>(lbl[s]);
        q.bbox[s] = bbox ? static_cast<const unsigned char*>(bbox[s]) : nullptr;
        q.img_div[s] = p.img_div[s];
    }
    q.coords = p.coords; q.out = p.out; q.bbox_out = bbox_out; q.bbox_sstride = bbox_sstride;
    q.S = p.S; q.B = p.B; q.H = p.H; q.W = p.W; q.L = p.L; q.nimg = p.nimg; q.Cp = p.Cp; q.amax_out = p.amax_out;
    for (int c = 0; c < 3; ++c) q.mean[c] = mean ? mean[c] : 0.f;
    if (q.amax_out) HIP_TRY(hipMemsetAsync(q.amax_out, 0, amax_clear * sizeof(unsigned), ctx.stream));
    hipLaunchKernelGGL(pack_input_u8_kernel, dim3(pack_grid((p.H * p.W + kPackU8Px - 1) / kPackU8Px), p.S * p.B), dim3(256), 0, ctx.stream, q);
    check_launch(p.nimg ? "pack_input_u8(img)" : "pack_input_u8(lbl)");
}

// FuseNet tail: zbar = mean over sources of cat(src_fea, tar_fea) + (y2 * alpha + beta)   (FuseTailArgs)
void run_fuse_tail(Ctx& ctx, const FuseTailArgs& t) {
    TimeScope ts(ctx, TSNET_T_ELEMWISE);
    hipLaunchKernelGGL(fuse_resid_mean_kernel, dim3(ew_grid((size_t)t.B * t.P * 2 * t.C1 / 4)), dim3(256), 0, ctx.stream, t);
    check_launch("fuse_resid_mean");
}

// n slot-table entries, host -> device on the stream: by value in the kernel arguments (slot_fill_kernel), so that nothing of the caller's
// is read after this returns and two tables enqueued back to back cannot meet
void run_slot_fill(hipStream_t s, int* dst, const int* host, int n) {
    for (int i0 = 0; i0 < n; i0 += kSlotFill) {
        SlotFillArgs a{};
        a.dst = dst + i0; a.n = std::min(kSlotFill, n - i0);
        for (int i = 0; i < a.n; ++i) a.v[i] = host[i0 + i];
        hipLaunchKernelGGL(slot_fill_kernel, dim3(1), dim3(kSlotFill), 0, s, a);
        check_launch("slot_fill");
    }
}

// weights of one layer -> operand planes + the un-scale factor; `stage` holds the OIHW parameter on the device (form 1: its transform,
// kernel 3 x 4).  planes: 2 = fp16 (hi, lo), 1 = one bf16 plane, -1 = one fp16 plane (hi alone)
void pack_layer(const float* stage, const ConvLayer& L, unsigned short* planes_out, int planes, float scale, hipStream_t s) {
    hipLaunchKernelGGL(pack_weights_kernel, dim3(ew_grid((size_t)L.kpad * L.npad)), dim3(256), 0, s, stage, planes_out, scale, planes,
                       L.cout, L.cin_real, L.cin_pad, L.ks, L.form == 1 ? 4 : L.ks, L.kpad, L.npad, L.cin_total > 0 ? L.cin_total : L.cin_real, L.cin_off);
    check_launch("pack_weights");
}

// Winograd F(2,3) filter transform along x (conv_w1.hpp): (O, I, 3, 3) -> (O, I, 3, 4),  U_p[ky] = sum_kx G[p][kx] g[ky][kx] with
// G = [[1,0,0],[.5,.5,.5],[.5,-.5,.5],[0,0,1]], evaluated in fp64 and rounded once to fp32
std::vector<float> winograd_x_filters(const std::vector<float>& w) {
    if (w.size() % 9) throw ArgError("winograd filter transform: not a 3 x 3 kernel");
    std::vector<float> u(w.size() / 9 * 12);
    for (size_t i = 0; i < w.size() / 3; ++i) {                     // one (o, i, ky) row of three taps -> four positions
        const double g0 = w[3 * i], g1 = w[3 * i + 1], g2 = w[3 * i + 2];
        u[4 * i] = (float)g0;
        u[4 * i + 1] = (float)(0.5 * (g0 + g1 + g2));
        u[4 * i + 2] = (float)(0.5 * (g0 - g1 + g2));
        u[4 * i + 3] = (float)g2;
    }
    return u;
}

// torch.linspace(-1, 1, n) in float32: step = (end-start)/(n-1); first half start+i*step, second half
// end-(n-1-i)*step (ATen's symmetric formula).
void linspace_pm1(int n, float* out) {
    if (n == 1) { out[0] = -1.f; return; }
    const float start = -1.f, end = 1.f;
    const float step = (end - start) / (float)(n - 1);
    const int half = n / 2;
    // ATen evaluates both halves with a fused multiply-add (e.g. linspace(-1,1,7)[3] == -2.98e-8, not 0)
    for (int i = 0; i < n; ++i) out[i] = i < half ? fmaf(step, (float)i, start) : fmaf(-step, (float)(n - i - 1), end);
}

// Encoder.coord_conv channels: xx = 2*(j/(w-1))-1, yy likewise, rr = sqrt(xx*xx+yy*yy); layout (H,W,3).
void coord_table(int H, int W, float* out) {
    for (int i = 0; i < H; ++i) {
        volatile float ys = (float)i / (float)(H - 1);
        volatile float yy = 2.f * ys - 1.f;
        for (int j = 0; j < W; ++j) {
            volatile float xs = (float)j / (float)(W - 1);
            volatile float xx = 2.f * xs - 1.f;
            volatile float x2 = xx * xx;
            volatile float y2 = yy * yy;
            volatile float ss = x2 + y2;
            float* o = out + ((size_t)i * W + j) * 3;
            o[0] = xx; o[1] = yy; o[2] = sqrtf(ss);
        }
    }
}

}  // namespace

// ================================================================================================
struct tsnet_engine {
    tsnet_cfg cfg{};
    std::string err;
    bool finalized = false;
    int cus = 256;                        // CUs of the engine's device, read at tsnet_finalize (launch heuristics only: conv_plan.hpp)
    int C = 0, h = 0, w = 0, P = 0, K = 0, Bmax = 0;
    int cp_img = 0, cp_lbl = 0;
    int np = 3;                           // MFMA products per k-group: 3 (fp16 x 2 operands), or 1 = the bf16- and fp16-operand modes (cfg.operand_mode)
    bool f16 = false;                     // np = 1: one fp16 plane of the scaled operand (cfg.operand_mode = 3) instead of one bf16 plane
    bool st16 = false;                    // cfg.operand_mode = 2: bf16 operands AND bf16 storage of the large conv-to-conv activations (the encoder's
                                          // 256^2 .. 64^2 maps, the decoder's up-convolution outputs and upsampled inputs); statistics from fp32 accumulators

    struct Param { std::string name; std::vector<int64_t> shape; std::vector<float> host; bool loaded = false; };
    std::vector<Param> params;
    std::map<std::string, int> pindex;

    // layers
    std::vector<ConvLayer> img_enc, lbl_enc;            // stem, downs, then 2 per resblock
    ConvLayer fuse_c1_src, fuse_c1_tar;   // FuseNet's first convolution split at the channel concat: per-source half / shared target half
    ConvLayer fuse_c2, fuse_out, dec_map, dec_head;
    std::vector<ConvLayer> dec_res, dec_up;
    std::vector<ConvLayer*> all_layers;   // every layer that runs on the MFMA kernels (all but the RGB head)
    float* head_w = nullptr;              // [49][ngf][4] weights of the RGB head (head_conv.hpp)
    const float* head_bias = nullptr;
    unsigned short* head_wq = nullptr;    // folded fp16 (hi, lo) filter planes of the head's MFMA form (head_mfma.hpp) and their un-scale factor
    const float* head_wq_unscale = nullptr;

    // device memory
    float* wpack = nullptr; size_t wpack_floats = 0;    // ONE buffer: biases, RGB-head table, un-scale factors, operand planes of every layer
    float* arena = nullptr; size_t arena_floats = 0;
    float* d_coords = nullptr; float* d_gx = nullptr; float* d_gy = nullptr;
    unsigned* amax = nullptr;             // device: max |x| PER IMAGE of tensors without an a-priori bound, as float bits; reset before each
                                          // producer.  One slot per image: a sample's scale (hence its result, bit for bit) never depends on the
                                          // rest of the batch.  K*Bmax packed source inputs | Bmax packed label inputs | Bmax sg | Bmax decoder streams
    unsigned* amax_src() const { return amax; }
    unsigned* amax_tar() const { return amax + (size_t)K * Bmax; }
    unsigned* amax_sg() const { return amax + (size_t)(K + 1) * Bmax; }
    unsigned* amax_dec() const { return amax + (size_t)(K + 2) * Bmax; }

    // arena buffers (sized for Bmax)
    float *x_img = nullptr, *x_lbl = nullptr;
    std::vector<float*> raw_img, raw_lbl;
    float *X = nullptr, *Y1 = nullptr, *Y2 = nullptr;
    float *tar_fea = nullptr, *that = nullptr, *shat = nullptr, *flow = nullptr, *pg = nullptr;   // that / shat: fp16 operand planes of the flow kernel
    float *F1 = nullptr, *F2 = nullptr, *zbar = nullptr, *sg = nullptr;
    float* F1s = nullptr;                 // per-source half of FuseNet's first convolution (+ bias): computed by set_sources, cached in clip mode
    float* FT = nullptr;                  // (B,P,2C) target half of it, computed once per driving frame
    float *D = nullptr, *DY1 = nullptr, *DY2 = nullptr;
    std::vector<float*> U, R;
    float* ab[4][2] = {{nullptr}};
    float* ab_side[2][2] = {{nullptr}};   // (alpha, beta) buffers of the side lane (target-label encoder)
    int ab_rr = 0, ab_side_rr = 0;
    double* part = nullptr;
    double* part_side = nullptr;       // statistics partials / arrival counters of the side lane
    int* fin_counter = nullptr;        // arrival counters of the in-kernel statistics finalize (conv_epilogue), all zero between launches
    int* fin_counter_side = nullptr;
    int* flow_cnt = nullptr;           // arrival counters of flow_kernel_p (256 ints behind the two above), all zero between launches
    float* flow_part = nullptr;        // its partial softmax states (large maps only)
    hipStream_t side_stream = nullptr; // target-label chain of a full forward runs here, concurrently with the source encoder
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_fork2 = nullptr, ev_join2 = nullptr;
    hipEvent_t ev_done = nullptr;      // recorded behind the last launch of a forward on the caller's stream
    float* train_ws = nullptr;         // workspace of tsnet_train_extras, allocated on first use

    // The encoded sources: ONE scheme.  The source-side tensors are K * Bmax SLOTS of one source each -- slot j is image j of X / shat / F1s
    // and mask j of bbox_copy, all dense -- and every forward names, in a table, the slot that each (source s, driving frame b) pair reads:
    // entry s*B + b (use_table; the kernels read nothing else to find a source).  Whatever is indexed by the pair itself -- flows, F1, F2 and
    // their InstanceNorm pairs -- stays at n = s*B + b.  The modes differ in who fills the slots and who writes the table:
    //   per-batch cache (tsnet_set_sources at batch B, the one-shot forward)   source s of frame b in slot s*B + b    table: the identity
    //   shared cache (tsnet_set_sources_shared)                               source s in slot s                     table: s for every b
    //   bank (tsnet_bank_put / tsnet_forward_bank)                            the slots the caller puts              table: the caller's
    // They write the same buffers: whichever was written last is the one that can be read.
    int cached_B = 0;               // batch of the cached sources: that of tsnet_set_sources, 1 for tsnet_set_sources_shared; 0 = no cache
    bool cached_shared = false;     // one source set for every driving frame: tsnet_forward_target takes any batch
    bool bank = false;              // the slots hold a bank (cached_B = 0 then)
    std::vector<char> bank_filled;  // per slot: put since the bank was started
    float* bbox_copy = nullptr;     // (K * Bmax, H, W) device copies of the source bboxes, one per slot
    int* slot_tab = nullptr;        // device (arena): K * Bmax ints, the table of the forward being enqueued (written by slot_fill_kernel)
    std::vector<int> slot_tab_host; // what slot_tab holds once everything enqueued so far has run: a forward with the same table skips the fill
    float* tbox = nullptr;          // (Bmax, H, W): the driving frames' masks widened from a compact call (wide calls pass their own tensor on)
    int last_B = 0;
    int last_SB = 0;                // images per source the last forward's sources held: its batch, 1 on a shared source set (what "src_fea" holds per source)
    bool last_shared = false;       // ... and whether it ran on a shared source set (tsnet_train_extras refuses: its src_img is per batch element)
    bool last_bank = false;         // the last forward ran on the bank ("src_fea" holds K * Bmax images; tsnet_train_extras refuses)
    int cur_B = 0;                        // batch of the forward being enqueued
    float src_div[TSNET_MAX_SOURCES];  // per-source image divisor (255; 1 for use_prev sources), tsnet_set_source_divisors

    Timing timing;

    void add_param(const std::string& name, std::vector<int64_t> shape) {
        pindex[name] = (int)params.size();
        Param p; p.name = name; p.shape = std::move(shape);
        params.push_back(std::move(p));
    }
    ConvLayer make_conv(const std::string& name, int cin_real, int cout, int ks, int stride, int pad, int reflect) {
        ConvLayer L; L.name = name; L.cin_real = cin_real; L.cin_pad = conv_cin_pad(cin_real); L.cout = cout; L.ks = ks;
        L.stride = stride; L.pad = pad; L.reflect = reflect;
        L.kpad = conv_kpad(ks, L.cin_pad); L.npad = conv_npad(cout);
        L.wparam = name + ".weight"; L.bparam = name + ".bias"; L.cin_total = cin_real; L.cin_off = 0;
        add_param(L.wparam, {cout, cin_real, ks, ks});
        add_param(L.bparam, {cout});
        return L;
    }
    void build_layers();
    void alloc_all(hipStream_t s);

    std::pair<float*, float*> next_ab(const Ctx& ctx) {
        if (!ctx.lane) { auto r = std::make_pair(ab[ab_rr][0], ab[ab_rr][1]); ab_rr = (ab_rr + 1) & 3; return r; }
        auto r = std::make_pair(ab_side[ab_side_rr][0], ab_side[ab_side_rr][1]); ab_side_rr ^= 1; return r;
    }
    float enc_bound() const { return (float)(cfg.enc_blocks + 1) * std::sqrt((float)P); }  // bound of the source features: |relu(IN)| <= sqrt(P), + one IN output per block
    // every convolution of the forward goes through here: the engine's operand mode, the lane's statistics scratch, the finalize
    void conv(Ctx& ctx, const ConvLayer& L, ConvCall& c) { c.nprod = f16 ? TSNET_NPROD_F16 : np; run_conv(ctx, L, c); }
    void conv_stats(Ctx& ctx, const ConvLayer& L, ConvCall& c, int N, int HW, float* alpha, float* beta) {
        double* pt = ctx.lane ? part_side : part;
        c.stat_part = pt;
        c.fin_alpha = alpha; c.fin_beta = beta; c.fin_counter = ctx.lane ? fin_counter_side : fin_counter;
        conv(ctx, L, c);
        if (c.stat_S < 0) return;              // finalised by the last workgroups of the convolution itself
        TimeScope ts(ctx, TSNET_T_STATS);
        hipLaunchKernelGGL(in_finalize2_kernel, dim3((L.cout + kFin2Ch - 1) / kFin2Ch, N), dim3(256), 0, ctx.stream, pt, alpha, beta, L.cout, c.stat_S, HW, 1e-5f);
        check_launch("in_finalize2");
    }
    void encode(Ctx& ctx, std::vector<ConvLayer>& L, const float* xin, const unsigned* xin_amax, int N, std::vector<float*>& raw, float* out_fea, int nblocks);
    // ResnetBlock.  stream_amax == null: the residual stream Xs has the a-priori bound stream_bound (encoder: (blocks+1) sqrt(HW));
    // else its bound is measured: max |first value| published by the producer + amax_add (decoder: the stream starts at a raw conv output)
    void resblock(Ctx& ctx, const ConvLayer& c1, const ConvLayer& c2, float* Xs, float stream_bound, const unsigned* stream_amax, float amax_add,
                  float* y1, float* y2, int N, int hh, int ww);
    void set_sources(Ctx& ctx, const SrcIn& in, int B, hipStream_t bbox_stream = nullptr);
    void target_chain(Ctx& ctx, const TarIn& tar, int B);
    void bank_put(Ctx& ctx, int first, int count, const SrcIn& in, const float* div);
    void use_table(Ctx& ctx, int B, int Kc, const int* bank_slots);
    void forward_rest(Ctx& ctx, const TarIn& tar, float* out_rgb, float* out_flow, int B, int Kc, const int* bank_slots = nullptr);
    void forward_target(Ctx& ctx, const TarIn& tar, float* out_rgb, float* out_flow, int B) {
        target_chain(ctx, tar, B);
        forward_rest(ctx, tar, out_rgb, out_flow, B, K);
    }
};

void tsnet_engine::build_layers() {
    const tsnet_cfg& c = cfg;
    const int coords = c.addcoords ? 3 : 0;
    auto enc = [&](const std::string& net, int cin, int nblocks, std::vector<ConvLayer>& out) {
        const int cin_real = cin + coords;
        out.push_back(make_conv(net + ".model.1", cin_real, c.ngf, 7, 1, 3, 1));
        int idx = 4, ch = c.ngf;
        for (int i = 0; i < c.n_downsampling; ++i) {
            out.push_back(make_conv(net + ".model." + std::to_string(idx), ch, ch * 2, 3, 2, 1, 0));
            ch *= 2; idx += 3;
        }
        for (int i = 0; i < nblocks; ++i) {
            out.push_back(make_conv(net + ".model." + std::to_string(idx) + ".conv_block.1", ch, ch, 3, 1, 1, 1));
            out.push_back(make_conv(net + ".model." + std::to_string(idx) + ".conv_block.5", ch, ch, 3, 1, 1, 1));
            idx += 1;
        }
        return out[0].cin_pad;
    };
    cp_img = enc("img_enc", 3 + c.label_nc, c.enc_blocks, img_enc);
    cp_lbl = enc("lbl_enc", c.label_nc, 0, lbl_enc);
    const int fc = 2 * C;   // FuseNet width: cat of two feature maps (1024 in the reference, TSNet.py:227)
    // conv(cat(src, tar)) = conv_src(src) + conv_tar(tar): the target half is shared by the K sources (SURVEY.md 7.2, -9.66 GMAC/frame).
    // Both halves read windows of the same OIHW parameter.
    fuse_c1_src = make_conv("fuse_net.model.0.conv_block.1", fc, fc, 3, 1, 1, 1);
    fuse_c1_src.name += "[src]"; fuse_c1_src.cin_real = C; fuse_c1_src.cin_pad = conv_cin_pad(C); fuse_c1_src.cin_off = 0;
    fuse_c1_src.kpad = conv_kpad(3, fuse_c1_src.cin_pad);
    fuse_c1_tar = fuse_c1_src; fuse_c1_tar.name = "fuse_net.model.0.conv_block.1[tar]"; fuse_c1_tar.cin_off = C; fuse_c1_tar.bparam.clear();
    fuse_c2 = make_conv("fuse_net.model.0.conv_block.5", fc, fc, 3, 1, 1, 1);
    fuse_out = make_conv("fuse_net.conv", fc, fc / 2, 1, 1, 0, 0);
    dec_map = make_conv("dec.map_conv", 2 * C, C, 1, 1, 0, 0);
    int n = 0;
    for (int i = 0; i < c.n_blocks; ++i) {
        dec_res.push_back(make_conv("dec.model" + std::to_string(n) + ".0.conv_block.1", C, C, 3, 1, 1, 1));
        dec_res.push_back(make_conv("dec.model" + std::to_string(n) + ".0.conv_block.5", C, C, 3, 1, 1, 1));
        ++n;
    }
    for (int i = 0; i < c.n_downsampling; ++i) {
        const int ci = c.ngf << (c.n_downsampling - i);
        dec_up.push_back(make_conv("dec.model" + std::to_string(n) + ".2", ci, ci / 2, 3, 1, 1, 1));
        ++n;
    }
    dec_head = make_conv("dec.model" + std::to_string(n) + ".1", c.ngf, 3, 7, 1, 3, 1);
    // ---- Winograd-along-x form (conv_w1.hpp) for the 3 x 3 / stride-1 layers it wins on, where the frame splits into whole 4 x 32 tiles: the
    // ResnetBlocks (127 / 133 us against 153 / 150 us at the headline batch, 39 against 50 us for one frame), FuseNet (266 / 87 / 565 us
    // against 293 / 101 / 618), the decoder's first up-convolution (86 against 101 us); profiles/round4_conv_variants.txt.  The later
    // up-convolutions (128^2: equal; 256^2: 120 against 111 us) and the bf16-operand mode keep the direct kernel.  A layer has ONE packed
    // form and therefore one kernel in every batch.
    auto to_w1 = [&](ConvLayer& L, int hh, int ww) {
        if (np == 1 || !w1_eligible(L.ks, L.stride, L.pad, L.cin_pad, hh, ww)) return;
        L.form = 1; L.kpad = conv_kpad_w1(L.cin_pad);
    };
    for (size_t i = 1 + c.n_downsampling; i < img_enc.size(); ++i) to_w1(img_enc[i], h, w);
    to_w1(fuse_c1_src, h, w); to_w1(fuse_c1_tar, h, w); to_w1(fuse_c2, h, w);
    for (auto& L : dec_res) to_w1(L, h, w);
    if (!dec_up.empty()) to_w1(dec_up[0], 2 * h, 2 * w);
    bool up1_w1 = true;
#ifdef TSNET_TOOLS
    up1_w1 = g_tools_knob[2] == 0;           // gpu A/B: the second up-convolution on the direct kernel (which then takes the fused upsample)
#endif
    if (dec_up.size() > 1 && up1_w1) to_w1(dec_up[1], 4 * h, 4 * w);      // equal at B = 4 (102.7 against 103.4 us), 29.7 against 34 us for one frame; the third (256^2 x 128 -> 64) stays direct: 118 against 140 us
    for (auto& L : img_enc) all_layers.push_back(&L);
    for (auto& L : lbl_enc) all_layers.push_back(&L);
    all_layers.push_back(&fuse_c1_src); all_layers.push_back(&fuse_c1_tar);
    all_layers.push_back(&fuse_c2); all_layers.push_back(&fuse_out);
    all_layers.push_back(&dec_map);
    for (auto& L : dec_res) all_layers.push_back(&L);
    for (auto& L : dec_up) all_layers.push_back(&L);
}

void tsnet_engine::alloc_all(hipStream_t s) {
    // ---- packed weights: ONE contiguous buffer (a single RCCL broadcast replicates a model): biases, the RGB-head table, the per-layer
    // un-scale factors 2^-sw, then the operand planes of every layer -- fp16 (hi, lo) of w * 2^sw, or one bf16 plane in the bf16-operand
    // mode.  Nothing else is packed: what a replica receives is exactly what its kernels read.
    const int planes = np == 1 ? 1 : 2;
    size_t off = 0;
    for (ConvLayer* L : all_layers) { L->b_off = off; off += (size_t)round_up(L->cout, 4); }
    dec_head.b_off = off; off += 4;
    off = (off + 63) / 64 * 64;            // 256-byte aligned sections
    const size_t head_off = off;
    off += (size_t)49 * cfg.ngf * 4 + 64;  // + one 16-channel row: the narrow-net head kernel reads whole 16-channel rows of the last tap
    off = (off + 63) / 64 * 64;
    const size_t tab_off = off;
    off += round_up((int)all_layers.size() + 1, 64);       // + the RGB head's folded planes
    off = (off + 63) / 64 * 64;
    const size_t head_planes_off = off;    // fp16 (hi, lo) planes of the head's folded filters (head_mfma.hpp): 80 ngf x 32 x 2 halves
    if (cfg.ngf % 16 == 0) off += head_mfma_table_halves(cfg.ngf) / 2;
    off = (off + 63) / 64 * 64;
    const size_t planes_off = off;
    size_t o16 = 0;
    for (ConvLayer* L : all_layers) { L->w_off = o16; o16 += (size_t)planes * L->kpad * L->npad; o16 = (o16 + 127) / 128 * 128; }
    off += (o16 + 1) / 2;                  // two 16-bit values per float slot
    wpack_floats = off;
    HIP_TRY(hipMalloc((void**)&wpack, wpack_floats * sizeof(float)));
    HIP_TRY(hipMemsetAsync(wpack, 0, wpack_floats * sizeof(float), s));
    size_t max_w = 0;
    for (ConvLayer* L : all_layers) max_w = std::max(max_w, (size_t)L->cout * L->cin_total * L->ks * (L->form == 1 ? 4 : L->ks));
    max_w = std::max(max_w, (size_t)3 * cfg.ngf * 49);
    float* stage = nullptr;
    HIP_TRY(hipMalloc((void**)&stage, max_w * sizeof(float)));
    unsigned short* planes_base = reinterpret_cast<unsigned short*>(wpack + planes_off);
    for (size_t i = 0; i < all_layers.size(); ++i) {
        ConvLayer* L = all_layers[i];
        const Param& pw = params[pindex[L->wparam]];
        // the filter as the kernel consumes it: itself, or its Winograd transform along x (fp64 on the host, rounded once)
        std::vector<float> wino;
        if (L->form == 1) wino = winograd_x_filters(pw.host);
        const std::vector<float>& wsrc = L->form == 1 ? wino : pw.host;
        // per layer a power-of-two scale from the largest |weight|: |w * 2^sw| <= 2^15
        float mx = 0.f;
        for (float v : wsrc) { const float av = std::fabs(v); if (av > mx) mx = av; }
        if (!std::isfinite(mx)) throw WeightError("parameter '" + L->wparam + "' holds a non-finite value");
        const int sw = ((np != 1 || f16) && mx > 0.f) ? h2_scale_log2(mx) : 0;
        const float unscale = std::ldexp(1.0f, -sw);
        HIP_TRY(hipMemcpyAsync(stage, wsrc.data(), wsrc.size() * sizeof(float), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(wpack + tab_off + i, &unscale, sizeof(float), hipMemcpyHostToDevice, s));
        pack_layer(stage, *L, planes_base + L->w_off, f16 ? -1 : planes, std::ldexp(1.0f, sw), s);
        if (!L->bparam.empty()) {
            const Param& pb = params[pindex[L->bparam]];
            HIP_TRY(hipMemcpyAsync(wpack + L->b_off, pb.host.data(), pb.host.size() * sizeof(float), hipMemcpyHostToDevice, s));
        }
        HIP_TRY(hipStreamSynchronize(s));   // host vectors / staging buffer reused next iteration
        L->wq = planes_base + L->w_off;
        L->w_unscale = (np == 1 && !f16) ? nullptr : wpack + tab_off + i;
        L->bias = L->bparam.empty() ? nullptr : wpack + L->b_off;
    }
    {                                      // RGB head: fp32 weights in the vector kernel's order + bias
        const Param& pw = params[pindex[dec_head.wparam]];
        const Param& pb = params[pindex[dec_head.bparam]];
        HIP_TRY(hipMemcpyAsync(stage, pw.host.data(), pw.host.size() * sizeof(float), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(wpack + dec_head.b_off, pb.host.data(), pb.host.size() * sizeof(float), hipMemcpyHostToDevice, s));
        head_w = wpack + head_off;
        head_bias = wpack + dec_head.b_off;
        hipLaunchKernelGGL(pack_head_weights_kernel, dim3(64), dim3(256), 0, s, stage, head_w, cfg.ngf);
        check_launch("pack_head_weights");
        if (cfg.ngf % 16 == 0) {           // the folded form's planes, in every operand mode (the head always runs three products)
            float mx = 0.f;
            for (float v : pw.host) { const float av = std::fabs(v); if (av > mx) mx = av; }
            if (!std::isfinite(mx)) throw WeightError("parameter '" + dec_head.wparam + "' holds a non-finite value");
            const int sw = mx > 0.f ? h2_scale_log2(mx) : 0;
            const float unscale = std::ldexp(1.0f, -sw);
            const size_t slot = tab_off + all_layers.size();
            HIP_TRY(hipMemcpyAsync(wpack + slot, &unscale, sizeof(float), hipMemcpyHostToDevice, s));
            head_wq = reinterpret_cast<unsigned short*>(wpack + head_planes_off);
            head_wq_unscale = wpack + slot;
            pack_head_mfma(stage, cfg.ngf, std::ldexp(1.0f, sw), head_wq, s);
            check_launch("pack_head_mfma");
        }
        HIP_TRY(hipStreamSynchronize(s));
    }
    HIP_TRY(hipFree(stage));
    for (auto& p : params) { std::vector<float>().swap(p.host); }   // host copies no longer needed

    // ---- constant tables
    const int H = cfg.height, W = cfg.width;
    {
        std::vector<float> t((size_t)H * W * 3), gx(w), gy(h);
        coord_table(H, W, t.data());
        linspace_pm1(w, gx.data());
        linspace_pm1(h, gy.data());
        HIP_TRY(hipMalloc((void**)&d_coords, t.size() * sizeof(float)));
        HIP_TRY(hipMalloc((void**)&d_gx, w * sizeof(float)));
        HIP_TRY(hipMalloc((void**)&d_gy, h * sizeof(float)));
        HIP_TRY(hipMemcpy(d_coords, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_gx, gx.data(), w * sizeof(float), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_gy, gy.data(), h * sizeof(float), hipMemcpyHostToDevice));
    }

    // ---- workspace arena: every buffer gets a fixed offset (no allocation after finalize)
    const size_t NB = (size_t)K * Bmax, B = Bmax;
    std::vector<std::pair<float**, size_t>> req;
    auto want = [&](float** p, size_t n) { req.emplace_back(p, (n + 63) & ~(size_t)63); };
    want(&x_img, NB * H * W * cp_img);
    want(&x_lbl, B * H * W * cp_lbl);
    raw_img.assign(cfg.n_downsampling + 1, nullptr);
    raw_lbl.assign(cfg.n_downsampling + 1, nullptr);
    for (int l = 0; l <= cfg.n_downsampling; ++l) {
        const size_t e = (size_t)(H >> l) * (W >> l) * (cfg.ngf << l);
        want(&raw_img[l], NB * e);
        want(&raw_lbl[l], B * e);
    }
    const size_t fe = (size_t)P * C;
    want(&X, NB * fe); want(&Y1, NB * fe); want(&Y2, NB * fe);
    want(&tar_fea, B * fe); want(&that, (flow_plane_halves((int)B, P, C) + 1) / 2); want(&shat, (flow_plane_halves((int)NB, P, C) + 1) / 2); want(&flow, NB * P * 2); want(&pg, B * fe);
    want(&F1, NB * fe * 2); want(&F2, NB * fe * 2); want(&F1s, NB * fe * 2); want(&zbar, B * fe * 2); want(&sg, B * fe); want(&FT, B * fe * 2);
    want(&D, B * fe); want(&DY1, B * fe); want(&DY2, B * fe);
    U.assign(cfg.n_downsampling, nullptr); R.assign(cfg.n_downsampling, nullptr);
    for (int i = 0; i < cfg.n_downsampling; ++i) {
        const size_t sp = (size_t)(h << (i + 1)) * (w << (i + 1));
        want(&U[i], B * sp * (C >> i));
        want(&R[i], B * sp * (C >> (i + 1)));
    }
    for (int i = 0; i < 4; ++i) { want(&ab[i][0], NB * 2 * C); want(&ab[i][1], NB * 2 * C); }
    for (int i = 0; i < 2; ++i) { want(&ab_side[i][0], NB * 2 * C); want(&ab_side[i][1], NB * 2 * C); }
    want(&bbox_copy, NB * H * W);
    float* slot_f = nullptr;
    want(&slot_f, NB);                                                       // the slot table (ints)
    if (P >= 2048 && P % 64 == 0) want(&flow_part, 2 * flowp_part_words((int)NB, P, flowp_slices(h, w)));   // flow_kernel_p: one softmax state per (image, target tile, slice, column), 8-byte words
    // InstanceNorm partials (doubles = 2 floats each): the stand-alone pass N*64*C*2, a conv epilogue N * tiles-per-image * Cout * 2
    // with tiles of at least 64 positions (ceil for ragged images), per lane
    size_t part_doubles = NB * 64 * 2 * C * 2;
    for (int l = 0; l <= cfg.n_downsampling; ++l) {
        const size_t hw = (size_t)(H >> l) * (W >> l), tpi = (hw + 63) / 64;
        part_doubles = std::max(part_doubles, stat_part_doubles(NB, tpi, (size_t)std::max(cfg.ngf << l, 2 * C)));
    }
    float *part_f = nullptr, *part_side_f = nullptr;
    want(&part_f, 2 * part_doubles); want(&part_side_f, 2 * part_doubles);
    want(&tbox, B * H * W);                                                  // (last: every buffer above keeps its offset)
    size_t total = 0;
    for (auto& r : req) total += r.second;
    arena_floats = total;
    HIP_TRY(hipMalloc((void**)&arena, total * sizeof(float)));
    size_t o = 0;
    for (auto& r : req) { *r.first = arena + o; o += r.second; }
    part = reinterpret_cast<double*>(part_f);
    part_side = reinterpret_cast<double*>(part_side_f);
    slot_tab = reinterpret_cast<int*>(slot_f);
    bank_filled.assign(NB, 0);
    HIP_TRY(hipMalloc((void**)&amax, (size_t)(K + 3) * Bmax * sizeof(unsigned)));
    HIP_TRY(hipMemsetAsync(amax, 0, (size_t)(K + 3) * Bmax * sizeof(unsigned), s));
    // arrival counters: one per (image, 32-channel group) of a launch; launches with more (image, group) pairs than kFinCounterInts
    // fall back to the in_finalize2 kernel (plan_conv checks the index range against this size)
    HIP_TRY(hipMalloc((void**)&fin_counter, (2 * kFinCounterInts + 256) * sizeof(int)));
    HIP_TRY(hipMemsetAsync(fin_counter, 0, (2 * kFinCounterInts + 256) * sizeof(int), s));
    fin_counter_side = fin_counter + kFinCounterInts;
    flow_cnt = fin_counter + 2 * kFinCounterInts;
    // side lane (tsnet_forward): own statistics scratch, counters, (alpha, beta) pairs (above), stream and events
    HIP_TRY(hipStreamCreateWithFlags(&side_stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&ev_join, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&ev_fork2, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&ev_join2, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&ev_done, hipEventDisableTiming));
}

void tsnet_engine::resblock(Ctx& ctx, const ConvLayer& c1, const ConvLayer& c2, float* Xs, float stream_bound, const unsigned* stream_amax,
                            float amax_add, float* y1, float* y2, int N, int hh, int ww) {
    const int Cc = c1.cout, HW = hh * ww;
    auto s1 = next_ab(ctx);
    ConvCall a; a.x = Xs; a.bound = stream_bound; a.in_amax = stream_amax; a.bound_add = amax_add;
    a.N = N; a.H = hh; a.W = ww; a.y = y1; a.tclass = TSNET_T_CONV_RES;
    conv_stats(ctx, c1, a, N, HW, s1.first, s1.second);
    ConvCall b; b.x = y1; b.alpha = s1.first; b.beta = s1.second; b.relu = 1; b.bound = std::sqrt((float)HW);   // |IN(.)| <= sqrt(HW - 1)
    b.N = N; b.H = hh; b.W = ww; b.y = y2; b.tclass = TSNET_T_CONV_RES;
    auto s2 = next_ab(ctx);
    conv_stats(ctx, c2, b, N, HW, s2.first, s2.second);
    run_norm_act(ctx, y2, s2.first, s2.second, 0, Xs, N, HW, Cc, Xs);   // X += IN(y2)
}

// Encoder.forward (TSNet.py:52-105) on a packed NHWC input whose maximum its producer published; out_fea = final feature map
void tsnet_engine::encode(Ctx& ctx, std::vector<ConvLayer>& L, const float* xin, const unsigned* xin_amax, int N, std::vector<float*>& raw,
                          float* out_fea, int nblocks) {
    int hh = cfg.height, ww = cfg.width;
    auto st = next_ab(ctx);
    {
        ConvCall a; a.x = xin; a.in_amax = xin_amax; a.bound = 1.f; a.N = N; a.H = hh; a.W = ww; a.y = raw[0];
        a.y_bf16 = st16;                                             // bf16 storage: the stem's and the first down-convolutions' raw outputs
        conv_stats(ctx, L[0], a, N, hh * ww, st.first, st.second);
    }
    for (int l = 1; l <= cfg.n_downsampling; ++l) {
        // the downsampling convolution reads relu(IN(previous)): the transform is applied while its operand tile is staged
        auto prev = st;
        st = next_ab(ctx);
        ConvCall d; d.x = raw[l - 1]; d.alpha = prev.first; d.beta = prev.second; d.relu = 1; d.bound = std::sqrt((float)(hh * ww));
        d.N = N; d.H = hh; d.W = ww; d.y = raw[l];
        d.x_bf16 = st16; d.y_bf16 = st16 && l < cfg.n_downsampling;  // the last one feeds norm_act (32 x 32 features: fp32)
        hh /= 2; ww /= 2;
        conv_stats(ctx, L[l], d, N, hh * ww, st.first, st.second);
    }
    run_norm_act(ctx, raw[cfg.n_downsampling], st.first, st.second, 1, nullptr, N, hh * ww, C, out_fea);
    // |relu(IN(.))| <= sqrt(HW) and every block adds one more InstanceNorm output: the stream stays below (blocks + 1) sqrt(HW)
    const float bound = (float)(nblocks + 1) * std::sqrt((float)(hh * ww));
    for (int i = 0; i < nblocks; ++i)
        resblock(ctx, L[cfg.n_downsampling + 1 + 2 * i], L[cfg.n_downsampling + 2 + 2 * i], out_fea, bound, nullptr, 0.f, Y1, Y2, N, hh, ww);
}

// bbox_stream: where the K bounding-box copies of the clip cache are enqueued.  Their only reader is the flow kernel; the one-shot forward
// passes its side stream (the flow kernel's own lane: the copies are ordered ahead of it there and cost the caller's lane nothing --
// three 4.7 us copy kernels + their boundaries sat in front of the stem until round 5); null = the caller's stream (clip mode).
// Compact sources: the packing kernel widens the masks into bbox_copy itself, on the caller's lane (ordered ahead of the flow kernel by the join).
// Source s of frame b goes to slot s*B + b of every source-side tensor, the masks included.
void tsnet_engine::set_sources(Ctx& ctx, const SrcIn& in, int B, hipStream_t bbox_stream) {
    cur_B = B;
    const int H = cfg.height, W = cfg.width;
    {
        TimeScope ts(ctx, TSNET_T_PACK);
        PackArgs p{};
        for (int s = 0; s < K; ++s) p.img_div[s] = src_div[s];
        p.coords = cfg.addcoords ? d_coords : nullptr;
        p.out = x_img; p.S = K; p.B = B; p.H = H; p.W = W; p.L = cfg.label_nc; p.nimg = 3; p.Cp = cp_img;
        p.amax_out = amax_src();
        run_pack_any(ctx, p, (size_t)K * B, in.u8, in.img, in.lbl, in.bbox, in.mean, bbox_copy, (size_t)B * H * W);
        for (int s = 0; s < K && !in.u8; ++s)
            HIP_TRY(hipMemcpyAsync(bbox_copy + (size_t)s * B * H * W, in.bbox[s], (size_t)B * H * W * sizeof(float), hipMemcpyDeviceToDevice,
                                   bbox_stream ? bbox_stream : ctx.stream));
    }
    encode(ctx, img_enc, x_img, amax_src(), K * B, raw_img, X, cfg.enc_blocks);
    run_l2norm_split(ctx, X, reinterpret_cast<unsigned short*>(shat), K * B, P, C);
    // the per-source half of FuseNet's first convolution (conv(cat(src, tar)) = conv_src(src) + conv_tar(tar), TSNet.py:195-197)
    // depends on the sources only: computed here, so a driving frame of a clip does not pay for it
    ConvCall a; a.x = X; a.bound = enc_bound(); a.N = K * B; a.H = h; a.W = w; a.y = F1s;
    conv(ctx, fuse_c1_src, a);
    cached_B = B; cached_shared = false; bank = false;
}

// `count` sources of batch 1 -> slots first .. first + count - 1 of the bank: set_sources' chain on count images, its outputs at the slot
// offset.  x_img, raw_img, the ResnetBlock scratch and the first `count` source maxima are staging; the other slots are not touched.
void tsnet_engine::bank_put(Ctx& ctx, int first, int count, const SrcIn& in, const float* div) {
    cur_B = 1;
    const int H = cfg.height, W = cfg.width;
    if (!bank) { std::fill(bank_filled.begin(), bank_filled.end(), 0); bank = true; cached_B = 0; cached_shared = false; }
    for (int i = 0; i < count; ++i) bank_filled[first + i] = 0;     // until everything below is enqueued
    {
        TimeScope ts(ctx, TSNET_T_PACK);
        for (int i0 = 0; i0 < count; i0 += TSNET_MAX_SOURCES) {     // the packing kernel takes up to eight plane pointers by value
            const int n = std::min(TSNET_MAX_SOURCES, count - i0);
            PackArgs p{};
            for (int s = 0; s < n; ++s) p.img_div[s] = div ? div[i0 + s] : 255.0f;
            p.coords = cfg.addcoords ? d_coords : nullptr;
            p.out = x_img + (size_t)i0 * H * W * cp_img; p.S = n; p.B = 1; p.H = H; p.W = W; p.L = cfg.label_nc; p.nimg = 3; p.Cp = cp_img;
            p.amax_out = amax_src() + i0;
            run_pack_any(ctx, p, (size_t)n, in.u8, in.img + i0, in.lbl + i0, in.bbox + i0, in.mean, bbox_copy + (size_t)(first + i0) * H * W, (size_t)H * W);
        }
        for (int i = 0; i < count && !in.u8; ++i)
            HIP_TRY(hipMemcpyAsync(bbox_copy + (size_t)(first + i) * H * W, in.bbox[i], (size_t)H * W * sizeof(float), hipMemcpyDeviceToDevice, ctx.stream));
    }
    float* fea = X + (size_t)first * P * C;
    encode(ctx, img_enc, x_img, amax_src(), count, raw_img, fea, cfg.enc_blocks);
    run_l2norm_split(ctx, fea, reinterpret_cast<unsigned short*>(shat) + (size_t)first * flow_plane_halves(1, P, C), count, P, C);
    ConvCall a; a.x = fea; a.bound = enc_bound(); a.N = count; a.H = h; a.W = w; a.y = F1s + (size_t)first * P * C * 2;
    conv(ctx, fuse_c1_src, a);
    for (int i = 0; i < count; ++i) bank_filled[first + i] = 1;
}

// Everything that depends on the driving frame only: label encoder, its L2-normalised features and the target half of
// FuseNet's first convolution.  Independent of the source encoder, so a full forward runs it on the side stream.
void tsnet_engine::target_chain(Ctx& ctx, const TarIn& tar, int B) {
    cur_B = B;
    const int H = cfg.height, W = cfg.width;
    {
        TimeScope ts(ctx, TSNET_T_PACK);
        PackArgs p{};
        p.coords = cfg.addcoords ? d_coords : nullptr;
        p.out = x_lbl; p.S = 1; p.B = B; p.H = H; p.W = W; p.L = cfg.label_nc; p.nimg = 0; p.Cp = cp_lbl;
        // one reset for the three per-image maxima of this forward (target input, sg, decoder stream: contiguous)
        p.amax_out = amax_tar();
        run_pack_any(ctx, p, (size_t)3 * Bmax, tar.u8, nullptr, &tar.lbl, &tar.bbox, nullptr, tbox, 0);    // compact: the masks -> tbox
    }
    encode(ctx, lbl_enc, x_lbl, amax_tar(), B, raw_lbl, tar_fea, 0);
    run_l2norm_split(ctx, tar_fea, reinterpret_cast<unsigned short*>(that), B, P, C);
    ConvCall t; t.x = tar_fea; t.bound = std::sqrt((float)P); t.N = B; t.H = h; t.W = w; t.y = FT;      // shared target half of fuse conv1
    conv(ctx, fuse_c1_tar, t);
}

// The slot table of a forward of B driving frames on Kc sources each -> slot_tab, on the caller's stream.  The one place that says what the
// modes are (struct tsnet_engine): the bank forward passes its caller's table, the caches' tables are written here.  The fill is skipped when
// the device already holds (or, stream-ordered, will hold) the same entries: a clip's forwards at one batch share one table.  That rests on
// what tsnet_abi.h asks of any two calls on one handle -- they share the arena, so the caller orders them, and with them this fill.
void tsnet_engine::use_table(Ctx& ctx, int B, int Kc, const int* bank_slots) {
    std::vector<int> t((size_t)Kc * B);
    for (int s = 0; s < Kc; ++s)
        for (int b = 0; b < B; ++b) t[s * B + b] = bank_slots ? bank_slots[s * B + b] : cached_shared ? s : s * B + b;
    if (t.size() <= slot_tab_host.size() && std::equal(t.begin(), t.end(), slot_tab_host.begin())) return;
    slot_tab_host.clear();                                  // (a launch that throws leaves no claim behind)
    run_slot_fill(ctx.stream, slot_tab, t.data(), (int)t.size());
    slot_tab_host = std::move(t);
}

// Kc sources per driving frame; bank_slots (host, entry s*B + b): the table of a forward on the source bank, null on the caches
void tsnet_engine::forward_rest(Ctx& ctx, const TarIn& tar, float* out_rgb, float* out_flow, int B, int Kc, const int* bank_slots) {
    cur_B = B;
    const float* tar_bbox = tar.u8 ? tbox : static_cast<const float*>(tar.bbox);      // compact: widened by target_chain's packing kernel
    const int K = Kc;                                      // sources per driving frame of THIS forward
    const int H = cfg.height, W = cfg.width, NB = K * B;
    use_table(ctx, B, K, bank_slots);                      // ahead of the fork: the side lane's readers are ordered behind it
    const int* slot = slot_tab;
    // ---- transformation branch.  Its result (pg) is first needed by the decoder, and its kernels are latency-bound (384 workgroups):
    // with the side stream available it runs there, concurrently with the MFMA-bound synthesis branch below, and joins before dec_map.
    const bool fork = side_stream && !ctx.timing && ctx.lane == 0;
    Ctx cside(side_stream, cus, nullptr, 1);
    Ctx& cx = fork ? cside : ctx;
    SideJoin join2{fork ? side_stream : nullptr, ctx.stream, ev_join2};
    if (fork) {
        HIP_TRY(hipEventRecord(ev_fork2, ctx.stream));
        HIP_TRY(hipStreamWaitEvent(side_stream, ev_fork2, 0));
    }
    FlowArgs fa{};
    fa.tq = reinterpret_cast<const unsigned short*>(that); fa.sq = reinterpret_cast<const unsigned short*>(shat); fa.tar_bbox = tar_bbox;
    fa.src_bbox = bbox_copy;
    fa.gx = d_gx; fa.gy = d_gy; fa.flow = flow;
    fa.part = reinterpret_cast<unsigned long long*>(flow_part); fa.cnt = flow_cnt;
    fa.B = B; fa.P = P; fa.C = C; fa.h = h; fa.w = w; fa.H = H; fa.W = W; fa.sy = H / h; fa.sx = W / w;
    run_flow(cx, fa, NB, slot);
    if (out_flow)
        HIP_TRY(hipMemcpyAsync(out_flow, flow, (size_t)NB * P * 2 * sizeof(float), hipMemcpyDeviceToDevice, cx.stream));
    run_warp(cx, X, slot, flow, pg, B, K, h, w, C);
    if (fork) HIP_TRY(hipEventRecord(ev_join2, side_stream));

    // ---- synthesis branch
    const float sqP = std::sqrt((float)P);
    {
        auto s1 = next_ab(ctx);
        auto s2 = next_ab(ctx);
        // F1 = conv_src(src) [from set_sources] + conv_tar(tar) [target chain], and its InstanceNorm statistics
        run_add_stats(ctx, F1s, slot, FT, B, F1, NB, P, 2 * C, part, s1.first, s1.second);
        ConvCall b; b.x = F1; b.alpha = s1.first; b.beta = s1.second; b.relu = 1; b.bound = sqP;
        b.N = NB; b.H = h; b.W = w; b.y = F2;
        conv_stats(ctx, fuse_c2, b, NB, P, s2.first, s2.second);
        run_fuse_tail(ctx, FuseTailArgs{X, tar_fea, F2, s2.first, s2.second, zbar, slot, B, K, P, C});
        // zbar = mean over sources of cat(src_fea, tar_fea) + IN(.): bounded by enc_bound + sqrt(P).  fuse_net.conv has no norm behind it:
        // it publishes max |sg| per image for dec.map_conv's operand scale
        ConvCall c; c.x = zbar; c.bound = enc_bound() + sqP; c.N = B; c.H = h; c.W = w; c.y = sg;
        c.amax_out = amax_sg();
        conv(ctx, fuse_out, c);
    }

    // ---- decoder
    if (fork) HIP_TRY(hipStreamWaitEvent(ctx.stream, ev_join2, 0));
    join2.done = true;
    // dec.map_conv reads cat(pg, sg) (TSNet.py:163) formed on load: |pg| <= enc_bound (a convex combination of source features, zero
    // padded), |sg| <= its published maximum.  The decoder's stream starts at map_conv's raw output: no a-priori bound either, so map_conv
    // publishes max |D| and the convolutions reading the stream derive their operand scale from it on the device:
    // D_i = D_0 + (i InstanceNorm outputs), |D_i| <= max |D_0| + i sqrt(P).  (bf16-operand mode: no scales; the maxima are not read.)
    {
        ConvCall a; a.x = pg; a.x2 = sg; a.csplit = C; a.x2_nmod = B; a.N = B; a.H = h; a.W = w; a.y = D;
        a.in_amax = amax_sg(); a.bound_add = enc_bound();
        a.amax_out = amax_dec();
        conv(ctx, dec_map, a);
    }
    for (int i = 0; i < cfg.n_blocks; ++i)
        resblock(ctx, dec_res[2 * i], dec_res[2 * i + 1], D, 0.f, amax_dec(), (float)i * sqP, DY1, DY2, B, h, w);
    const float* cur = D; const float* cal = nullptr; const float* cbe = nullptr;
    int hh = h, ww = w, cc = C;
    for (int i = 0; i < cfg.n_downsampling; ++i) {
        // input of up-convolution i = bilinear x2 of relu(IN(previous)) -- a convex combination of InstanceNorm outputs, bounded by
        // sqrt(HW) of the low-resolution map; the first one upsamples the decoder stream itself: published max |D_0| + n_blocks sqrt(P)
        const float in_bound = std::sqrt((float)(hh * ww));
        // A direct 3 x 3 layer under IN + ReLU whose plan takes the fused form (conv_plan.hpp: fp16 x 2 operands, 4 x 32 tiles) reads the
        // low-resolution map itself and blends while it stages its patch -- U[i] is never written (the last up-convolution of the headline:
        // 134 MB written and read back).  The bound holds: the blend is a convex combination.  Same bits as the two launches.  The layers in
        // the Winograd form keep them: their producers have neither the registers nor the LDS.
        bool fused = false;
        if (cal && !st16) {
            ConvCall q; q.N = B; q.H = 2 * hh; q.W = 2 * ww; q.alpha = cal; q.nprod = f16 ? TSNET_NPROD_F16 : np;
            fused = plan_takes_up2(conv_shape(dec_up[i], q), ctx.cus);
        }
#ifdef TSNET_TOOLS
        if (g_tools_knob[1]) fused = false;      // tools/forward_ab.py: the same forward on the two-launch route, one process
#endif
        if (!fused) run_upsample(ctx, cur, cal, cbe, cal ? 1 : 0, B, hh, ww, cc, U[i], st16 && i > 0, st16);
        hh *= 2; ww *= 2;
        cc /= 2;
        auto st = next_ab(ctx);
        ConvCall a; a.x = U[i]; a.bound = in_bound; a.N = B; a.H = hh; a.W = ww; a.y = R[i];
        a.x_bf16 = st16; a.y_bf16 = st16;
        if (fused) { a.x = cur; a.alpha = cal; a.beta = cbe; a.relu = 1; a.up2 = true; }
        if (!cal) { a.in_amax = amax_dec(); a.bound_add = (float)cfg.n_blocks * sqP; }
        conv_stats(ctx, dec_up[i], a, B, hh * ww, st.first, st.second);
        cur = R[i]; cal = st.first; cbe = st.second;
    }
    {
        TimeScope ts(ctx, TSNET_T_CONV);     // it is a convolution: keep it in the conv class for the roofline accounting
        HeadArgs ha{};
        ha.x = cur; ha.alpha = cal; ha.beta = cbe; ha.w = head_w; ha.bias = head_bias; ha.y = out_rgb;
        ha.N = B; ha.H = hh; ha.W = ww; ha.C = cc; ha.x_bf16 = st16 && cfg.n_downsampling > 0;
        ha.composite = cfg.pose_composite; ha.fore_x0 = 64; ha.fore_x1 = 192;          // TSNet_pose.py:279
        for (int c = 0; c < 3; ++c) ha.bg[c] = (-cfg.pose_mean[c]) / 255.0f;             // TSNet_pose.py:276
        launch_head(ha, hh, ww, B, ctx.stream, ctx.cus, 0, head_wq, head_wq_unscale);
    }
    last_B = B; last_SB = bank ? 1 : cached_B; last_shared = cached_shared; last_bank = bank;
    HIP_TRY(hipEventRecord(ev_done, ctx.stream));       // what tsnet_stage_ptr orders its widening pass behind
}

// ================================================================================================
// C ABI
#define API_BEGIN(h)                        \
    if (!(h)) return TSNET_ERR_ARG;         \
    try {
#define API_END(h)                                                              \
    } catch (const ArgError& e) { (h)->err = e.what(); return TSNET_ERR_ARG; }   \
      catch (const WeightError& e) { (h)->err = e.what(); return TSNET_ERR_WEIGHT; } \
      catch (const std::bad_alloc&) { (h)->err = "out of host memory"; return TSNET_ERR_NOMEM; } \
      catch (const std::exception& e) { (h)->err = e.what(); return TSNET_ERR_HIP; } \
    return TSNET_OK;

extern "C" {

int tsnet_abi_version(void) { return TSNET_ABI_VERSION; }

int tsnet_create(const tsnet_cfg* cfg, tsnet_handle* out) {
    if (!cfg || !out) { g_create_error = "null argument"; return TSNET_ERR_ARG; }
    *out = nullptr;
    auto bad = [&](const char* m) { g_create_error = m; return TSNET_ERR_ARG; };
    if (cfg->n_source < 1 || cfg->n_source > TSNET_MAX_SOURCES) return bad("n_source must be in 1..8");
    if (cfg->label_nc < 1) return bad("label_nc must be >= 1");
    if (cfg->n_downsampling < 1 || cfg->n_downsampling > 5) return bad("n_downsampling must be in 1..5");
    if (cfg->ngf < 8 || (cfg->ngf & (cfg->ngf - 1))) return bad("ngf must be a power of two >= 8");
    if (cfg->n_blocks < 0 || cfg->enc_blocks < 0) return bad("block counts must be >= 0");
    const int ds = 1 << cfg->n_downsampling;
    if (cfg->height < ds * 2 || cfg->width < ds * 2 || cfg->height % ds || cfg->width % ds)
        return bad("height/width must be multiples of 2^n_downsampling (and at least twice that)");
    if (cfg->max_batch < 1) return bad("max_batch must be >= 1");
    if (cfg->pose_composite && (cfg->height != 256 || cfg->width != 256))
        return bad("pose composite is defined for 256x256 frames only (TSNet_pose.py:277-280)");
    if (cfg->operand_mode < 0 || cfg->operand_mode > 3) return bad("operand_mode must be 0 (fp32-class), 1 (bf16 operands), 2 (bf16 operands + bf16 storage) or 3 (fp16 operands)");
    try {
        tsnet_engine* e = new tsnet_engine();
        e->cfg = *cfg;
        e->K = cfg->n_source; e->Bmax = cfg->max_batch;
        for (int s = 0; s < TSNET_MAX_SOURCES; ++s) e->src_div[s] = 255.0f;
        e->C = cfg->ngf << cfg->n_downsampling;
        e->h = cfg->height / ds; e->w = cfg->width / ds; e->P = e->h * e->w;
        e->np = cfg->operand_mode != 0 ? 1 : 3;
        e->st16 = cfg->operand_mode == 2;
        e->f16 = cfg->operand_mode == 3;
        e->build_layers();
        *out = e;
    } catch (const std::exception& ex) { g_create_error = ex.what(); return TSNET_ERR_NOMEM; }
    return TSNET_OK;
}

const char* tsnet_last_error(tsnet_handle h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int tsnet_num_params(tsnet_handle h) { return h ? (int)h->params.size() : TSNET_ERR_ARG; }

int tsnet_param_info(tsnet_handle h, int index, const char** name, int64_t shape_out[4], int* rank) {
    API_BEGIN(h)
    if (index < 0 || index >= (int)h->params.size()) throw ArgError("param index out of range");
    const auto& p = h->params[index];
    if (name) *name = p.name.c_str();
    if (rank) *rank = (int)p.shape.size();
    if (shape_out) for (size_t i = 0; i < 4; ++i) shape_out[i] = i < p.shape.size() ? p.shape[i] : 1;
    API_END(h)
}

int tsnet_load_weights(tsnet_handle h, const char* name, const float* data, const int64_t* shape, int rank) {
    API_BEGIN(h)
    if (h->finalized) throw ArgError("load_weights after finalize");
    if (!name || !data || !shape) throw ArgError("null argument");
    auto it = h->pindex.find(name);
    if (it == h->pindex.end()) throw WeightError(std::string("unknown parameter '") + name + "'");
    auto& p = h->params[it->second];
    bool ok = rank == (int)p.shape.size();
    for (int i = 0; ok && i < rank; ++i) ok = shape[i] == p.shape[i];
    if (!ok) {
        std::string m = std::string("shape mismatch for '") + name + "': expected (";
        for (auto d : p.shape) m += std::to_string(d) + ",";
        m += ") got (";
        for (int i = 0; i < rank; ++i) m += std::to_string(shape[i]) + ",";
        throw WeightError(m + ")");
    }
    size_t n = 1;
    for (auto d : p.shape) n *= (size_t)d;
    p.host.resize(n);
    HIP_TRY(hipMemcpy(p.host.data(), data, n * sizeof(float), hipMemcpyDefault));
    p.loaded = true;
    API_END(h)
}

int tsnet_finalize(tsnet_handle h, void* stream) {
    API_BEGIN(h)
    if (h->finalized) throw ArgError("finalize called twice");
    for (auto& p : h->params)
        if (!p.loaded) throw WeightError("parameter '" + p.name + "' was never loaded");
    h->alloc_all((hipStream_t)stream);
    h->cus = current_device_cus();                  // the engine's device: its allocations live there
    h->finalized = true;
    API_END(h)
}

void tsnet_destroy(tsnet_handle h) {
    if (!h) return;
    (void)hipFree(h->fin_counter); (void)hipFree(h->train_ws); (void)hipFree(h->amax);
    if (h->side_stream) (void)hipStreamDestroy(h->side_stream);
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    if (h->ev_join) (void)hipEventDestroy(h->ev_join);
    if (h->ev_fork2) (void)hipEventDestroy(h->ev_fork2);
    if (h->ev_join2) (void)hipEventDestroy(h->ev_join2);
    if (h->ev_done) (void)hipEventDestroy(h->ev_done);
    (void)hipFree(h->wpack); (void)hipFree(h->arena); (void)hipFree(h->d_coords); (void)hipFree(h->d_gx); (void)hipFree(h->d_gy);
    delete h;
}

int tsnet_packed_weights(tsnet_handle h, void** dev_ptr, size_t* bytes) {
    API_BEGIN(h)
    if (!h->finalized) throw ArgError("packed_weights before finalize");
    if (dev_ptr) *dev_ptr = h->wpack;
    if (bytes) *bytes = h->wpack_floats * sizeof(float);
    API_END(h)
}

static void check_forward_args(tsnet_handle h, int B) {
    if (!h->finalized) throw ArgError("forward before finalize");
    if (B < 1 || B > h->Bmax) throw ArgError("batch size outside 1..max_batch");
}

int tsnet_set_source_divisors(tsnet_handle h, const float* div, int n) {
    API_BEGIN(h)
    if (n < 0 || n > TSNET_MAX_SOURCES || (n > 0 && !div)) throw ArgError("set_source_divisors: bad argument");
    for (int s = 0; s < TSNET_MAX_SOURCES; ++s) {
        const float d = s < n ? div[s] : 255.0f;
        if (!(d > 0.f) || !std::isfinite(d)) throw ArgError("set_source_divisors: divisors must be positive and finite");
        h->src_div[s] = d;
    }
    h->cached_B = 0; h->cached_shared = false; h->bank = false;     // cached source features were encoded with the previous divisors
    API_END(h)
}

// The forward entry points take their inputs in either form (SrcIn / TarIn): the wide entries and their _u8 siblings differ in the descriptor only.
static const void* const* vlist(const float* const* p) { return reinterpret_cast<const void* const*>(p); }
static const void* const* vlist(const uint8_t* const* p) { return reinterpret_cast<const void* const*>(p); }
static SrcIn src_in(const float* const* img, const float* const* lbl, const float* const* bbox) {
    SrcIn in; in.img = vlist(img); in.lbl = vlist(lbl); in.bbox = vlist(bbox); return in;
}
static SrcIn src_in(const uint8_t* const* img, const uint8_t* const* lbl, const uint8_t* const* bbox, const float* mean) {
    SrcIn in; in.u8 = true; in.img = vlist(img); in.lbl = vlist(lbl); in.bbox = vlist(bbox); in.mean = mean; return in;
}
static TarIn tar_in(const float* lbl, const float* bbox) { TarIn t; t.lbl = lbl; t.bbox = bbox; return t; }
static TarIn tar_in(const uint8_t* lbl, const uint8_t* bbox) { TarIn t; t.u8 = true; t.lbl = lbl; t.bbox = bbox; return t; }
// what a compact call needs beyond its wide sibling's checks (after them: the sibling's messages come first)
static void check_compact(tsnet_handle h, const SrcIn* in) {
    if (h->cfg.label_nc > 255) throw ArgError("compact inputs: class indices are bytes (label_nc <= 255)");
    if (in && in->u8 && !in->mean) throw ArgError("compact inputs: null mean_bgr");
}

static int set_sources_any(tsnet_handle h, const SrcIn& in, int B, bool shared, void* stream) {
    API_BEGIN(h)
    check_forward_args(h, B);
    if (!in.img || !in.lbl || !in.bbox) throw ArgError("null source list");
    for (int s = 0; s < h->K; ++s)
        if (!in.img[s] || !in.lbl[s] || !in.bbox[s]) throw ArgError("null source tensor (need n_source entries)");
    if (in.u8) check_compact(h, &in);
    Ctx ctx((hipStream_t)stream, h->cus, h->timing.on ? &h->timing : nullptr);
    h->set_sources(ctx, in, B);                                 // shared: K images, source-batch extent 1
    h->cached_shared = shared;
    API_END(h)
}

int tsnet_set_sources(tsnet_handle h, const float* const* src_img, const float* const* src_lbl,
                      const float* const* src_bbox, int B, void* stream) {
    return set_sources_any(h, src_in(src_img, src_lbl, src_bbox), B, false, stream);
}

int tsnet_set_sources_shared(tsnet_handle h, const float* const* src_img, const float* const* src_lbl,
                             const float* const* src_bbox, void* stream) {
    return set_sources_any(h, src_in(src_img, src_lbl, src_bbox), 1, true, stream);
}

int tsnet_set_sources_u8(tsnet_handle h, const uint8_t* const* src_img, const uint8_t* const* src_lbl, const uint8_t* const* src_bbox,
                         const float* mean_bgr, int B, int shared, void* stream) {
    if (h && shared && B != 1) { h->err = "set_sources_u8: a shared source set has batch 1"; return TSNET_ERR_ARG; }
    return set_sources_any(h, src_in(src_img, src_lbl, src_bbox, mean_bgr), B, shared != 0, stream);
}

static int forward_target_any(tsnet_handle h, const TarIn& tar, float* out_rgb, float* out_flow, int B, void* stream) {
    API_BEGIN(h)
    check_forward_args(h, B);
    if (!tar.lbl || !tar.bbox || !out_rgb) throw ArgError("null target/output tensor");
    if (!h->cached_shared && h->cached_B != B) throw ArgError("forward_target: batch differs from the cached sources (call tsnet_set_sources first)");
    if (tar.u8) check_compact(h, nullptr);
    Ctx ctx((hipStream_t)stream, h->cus, h->timing.on ? &h->timing : nullptr);
    h->forward_target(ctx, tar, out_rgb, out_flow, B);
    API_END(h)
}

int tsnet_forward_target(tsnet_handle h, const float* tar_lbl, const float* tar_bbox,
                         float* out_rgb, float* out_flow, int B, void* stream) {
    return forward_target_any(h, tar_in(tar_lbl, tar_bbox), out_rgb, out_flow, B, stream);
}

int tsnet_forward_target_u8(tsnet_handle h, const uint8_t* tar_lbl, const uint8_t* tar_bbox,
                            float* out_rgb, float* out_flow, int B, void* stream) {
    return forward_target_any(h, tar_in(tar_lbl, tar_bbox), out_rgb, out_flow, B, stream);
}

int tsnet_bank_capacity(tsnet_handle h) { return h ? h->K * h->Bmax : TSNET_ERR_ARG; }

static int bank_put_any(tsnet_handle h, int first_slot, int count, const SrcIn& in, const float* div, void* stream) {
    API_BEGIN(h)
    if (!h->finalized) throw ArgError("bank_put before finalize");
    const int cap = h->K * h->Bmax;
    if (count < 1 || first_slot < 0 || first_slot > cap - count)
        throw ArgError("bank_put: slots " + std::to_string(first_slot) + " .. " + std::to_string((long long)first_slot + count - 1) + " are outside the bank (capacity " + std::to_string(cap) + ")");
    if (!in.img || !in.lbl || !in.bbox) throw ArgError("bank_put: null source list");
    for (int i = 0; i < count; ++i) {
        if (!in.img[i] || !in.lbl[i] || !in.bbox[i]) throw ArgError("bank_put: null source tensor (need `count` entries)");
        if (div && (!(div[i] > 0.f) || !std::isfinite(div[i]))) throw ArgError("bank_put: divisors must be positive and finite");
    }
    if (in.u8) check_compact(h, &in);
    Ctx ctx((hipStream_t)stream, h->cus, h->timing.on ? &h->timing : nullptr);
    h->bank_put(ctx, first_slot, count, in, div);
    API_END(h)
}

int tsnet_bank_put(tsnet_handle h, int first_slot, int count, const float* const* src_img, const float* const* src_lbl,
                   const float* const* src_bbox, const float* div, void* stream) {
    return bank_put_any(h, first_slot, count, src_in(src_img, src_lbl, src_bbox), div, stream);
}

int tsnet_bank_put_u8(tsnet_handle h, int first_slot, int count, const uint8_t* const* src_img, const uint8_t* const* src_lbl,
                      const uint8_t* const* src_bbox, const float* mean_bgr, const float* div, void* stream) {
    return bank_put_any(h, first_slot, count, src_in(src_img, src_lbl, src_bbox, mean_bgr), div, stream);
}

static int forward_bank_any(tsnet_handle h, const int* slots, int Kc, const TarIn& tar, float* out_rgb, float* out_flow, int B, void* stream) {
    API_BEGIN(h)
    check_forward_args(h, B);
    if (Kc < 1 || Kc > h->K) throw ArgError("forward_bank: sources per frame outside 1..n_source");
    if (!h->bank) throw ArgError("forward_bank: no source bank (call tsnet_bank_put first)");
    if (!slots || !tar.lbl || !tar.bbox || !out_rgb) throw ArgError("forward_bank: null slot table / target / output tensor");
    const int cap = h->K * h->Bmax;
    for (int i = 0; i < Kc * B; ++i) {
        if (slots[i] < 0 || slots[i] >= cap) throw ArgError("forward_bank: slot " + std::to_string(slots[i]) + " is outside the bank (capacity " + std::to_string(cap) + ")");
        if (!h->bank_filled[slots[i]]) throw ArgError("forward_bank: slot " + std::to_string(slots[i]) + " is not filled");
    }
    if (tar.u8) check_compact(h, nullptr);
    Ctx ctx((hipStream_t)stream, h->cus, h->timing.on ? &h->timing : nullptr);
    h->target_chain(ctx, tar, B);
    h->forward_rest(ctx, tar, out_rgb, out_flow, B, Kc, slots);
    API_END(h)
}

int tsnet_forward_bank(tsnet_handle h, const int* slots, int Kc, const float* tar_lbl, const float* tar_bbox,
                       float* out_rgb, float* out_flow, int B, void* stream) {
    return forward_bank_any(h, slots, Kc, tar_in(tar_lbl, tar_bbox), out_rgb, out_flow, B, stream);
}

int tsnet_forward_bank_u8(tsnet_handle h, const int* slots, int Kc, const uint8_t* tar_lbl, const uint8_t* tar_bbox,
                          float* out_rgb, float* out_flow, int B, void* stream) {
    return forward_bank_any(h, slots, Kc, tar_in(tar_lbl, tar_bbox), out_rgb, out_flow, B, stream);
}

static int forward_any(tsnet_handle h, const SrcIn& in, const TarIn& tar, float* out_rgb, float* out_flow, int B, void* stream) {
    if (h && h->finalized && h->side_stream && !h->timing.on && tar.lbl && tar.bbox && out_rgb) {
        // Full forward on two lanes: the driving-frame chain (label encoder, L2 norm, target half of FuseNet conv1 --
        // small launches that leave most CUs idle at B = 4) runs on the engine's side stream while the caller's stream
        // encodes the sources; they join before the flow kernel.  Same kernels, same arithmetic: the result is
        // bit-identical to tsnet_set_sources + tsnet_forward_target (tested).  Per-kernel timing runs them in sequence.
        API_BEGIN(h)
        check_forward_args(h, B);
        hipStream_t main = (hipStream_t)stream;
        HIP_TRY(hipEventRecord(h->ev_fork, main));
        HIP_TRY(hipStreamWaitEvent(h->side_stream, h->ev_fork, 0));
        Ctx cs(h->side_stream, h->cus, nullptr, 1);
        // from here on the side lane has work in flight: whatever happens below (an exception included), the caller's stream waits
        // for it before this call returns -- the side lane must not outlive the call
        SideJoin join{h->side_stream, main, h->ev_join};
        if (!in.img || !in.lbl || !in.bbox) throw ArgError("null source list");
        for (int s = 0; s < h->K; ++s)
            if (!in.img[s] || !in.lbl[s] || !in.bbox[s]) throw ArgError("null source tensor (need n_source entries)");
        if (in.u8 || tar.u8) check_compact(h, &in);
        h->target_chain(cs, tar, B);
        Ctx cm(main, h->cus);
        h->set_sources(cm, in, B, h->side_stream);      // (the bounding-box copies ride the side lane, ahead of the flow kernel)
        HIP_TRY(hipEventRecord(h->ev_join, h->side_stream));
        HIP_TRY(hipStreamWaitEvent(main, h->ev_join, 0));
        join.done = true;
        Ctx ctx(main, h->cus);
        h->forward_rest(ctx, tar, out_rgb, out_flow, B, h->K);
        API_END(h)
    }
    int rc = set_sources_any(h, in, B, false, stream);
    if (rc != TSNET_OK) return rc;
    return forward_target_any(h, tar, out_rgb, out_flow, B, stream);
}

int tsnet_forward(tsnet_handle h, const float* const* src_img, const float* const* src_lbl, const float* const* src_bbox,
                  const float* tar_lbl, const float* tar_bbox, float* out_rgb, float* out_flow, int B, void* stream) {
    return forward_any(h, src_in(src_img, src_lbl, src_bbox), tar_in(tar_lbl, tar_bbox), out_rgb, out_flow, B, stream);
}

int tsnet_forward_u8(tsnet_handle h, const uint8_t* const* src_img, const uint8_t* const* src_lbl, const uint8_t* const* src_bbox,
                     const uint8_t* tar_lbl, const uint8_t* tar_bbox, const float* mean_bgr, float* out_rgb, float* out_flow, int B, void* stream) {
    return forward_any(h, src_in(src_img, src_lbl, src_bbox, mean_bgr), tar_in(tar_lbl, tar_bbox), out_rgb, out_flow, B, stream);
}

// ---- the training extras' launches (train_extras.hpp), stated once: tsnet_train_extras runs them on the engine's flows, features and workspace,
// tsnet_op_patch_warp / tsnet_op_train_tail on the caller's tensors
constexpr int kTrainChunks = 16;    // blocks of renorm_l1_kernel per (frame, channel): l1 partials are (K*B*3*kTrainChunks) doubles
constexpr int kTrainNcos = 256;     // blocks of cosine_partial_kernel = its partials

struct TrainWs {
    float *gen_mean, *gen_std;      // (K*B*3) each
    float *ref_mean, *ref_std;      // (B*3) each
    double *l1_part, *cos_part;     // (K*B*3*kTrainChunks), (kTrainNcos)
};

// model/TSNet.py:373-379: src_img K x (B,3,H,W) raw, div K host floats, flow (K*B, h*w, 2) -> out (K,B,3,H,W)
static void launch_patch_warp(const float* const* src_img, const float* div, const float* flow, float* out, int K, int B, int H, int W, int hh, int ww,
                              hipStream_t st) {
    PatchWarpArgs pa{};
    for (int s = 0; s < K; ++s) { pa.src[s] = src_img[s]; pa.div[s] = div[s]; }
    pa.flow = flow; pa.out = out; pa.K = K; pa.B = B; pa.H = H; pa.W = W; pa.h = hh; pa.w = ww; pa.down = H / hh;
    hipLaunchKernelGGL(patch_warp_kernel, dim3(ew_grid((size_t)K * B * H * W)), dim3(256), 0, st, pa);
    check_launch("patch_warp");
}

// everything after the patch warp: x (K*B,3,H*W) re-normalised in place to the statistics of tar_img (B,3,H,W) raw, the composite when
// fore_x1 > fore_x0, losses[0] = loss_warp; pg / sg (B*P, C) or both null (the pose form: no cosine launch, losses[1] = 0)
static void launch_train_tail(float* x, const float* tar_img, const float* pg, const float* sg, int K, int B, int H, int W, int P, int C,
                              int fore_x0, int fore_x1, const float* bg, const TrainWs& ws, float* losses, hipStream_t st) {
    const int N = K * B, HW = H * W, chunks = kTrainChunks, ncos = kTrainNcos;
    const bool pose = !pg && !sg;
    hipLaunchKernelGGL(frame_stats_kernel, dim3(3, B), dim3(256), 0, st, tar_img, 3, HW, 255.0f, ws.ref_mean, ws.ref_std);      // TSNet.py:329-330
    check_launch("frame_stats(tar)");
    hipLaunchKernelGGL(frame_stats_kernel, dim3(3, N), dim3(256), 0, st, x, 3, HW, 1.0f, ws.gen_mean, ws.gen_std);              // :381-382
    check_launch("frame_stats(warp)");
    hipLaunchKernelGGL(renorm_l1_kernel, dim3(chunks, 3, N), dim3(256), 0, st, x, tar_img, B, HW, ws.gen_mean, ws.gen_std, ws.ref_mean, ws.ref_std, ws.l1_part,
                       W, fore_x0, fore_x1, bg[0], bg[1], bg[2]);
    check_launch("renorm_l1");
    if (!pose) {
        hipLaunchKernelGGL(cosine_partial_kernel, dim3(ncos), dim3(256), 0, st, pg, sg, B * P, C, ws.cos_part);
        check_launch("cosine_partial");
    }
    hipLaunchKernelGGL(train_losses_kernel, dim3(1), dim3(64), 0, st, ws.l1_part, K, B * 3 * chunks, (double)B * 3 * HW, ws.cos_part, pose ? 0 : ncos, (double)B * P, losses);
    check_launch("train_losses");
}

int tsnet_train_extras(tsnet_handle h, const float* const* src_img, const float* tar_img, int B,
                       float* warp_src_img, float* losses, void* stream) {
    API_BEGIN(h)
    check_forward_args(h, B);
    if (h->last_B != B) throw ArgError("train_extras: call tsnet_forward with the same batch first (uses its flows and features)");
    if (h->last_shared) throw ArgError("train_extras: the last forward ran on a shared source set (tsnet_set_sources_shared); src_img is per batch element here");
    if (h->last_bank) throw ArgError("train_extras: the last forward ran on a source bank (tsnet_forward_bank); src_img is per batch element here");
    if (!src_img || !tar_img || !warp_src_img || !losses) throw ArgError("train_extras: null tensor");
    const int K = h->K, H = h->cfg.height, W = h->cfg.width, hh = h->h, ww = h->w, P = h->P, C = h->C;
    for (int s = 0; s < K; ++s) if (!src_img[s]) throw ArgError("train_extras: null source image (need n_source entries)");
    if (H % hh || W % ww || H / hh != W / ww) throw ArgError("train_extras: image size must be a multiple of the feature size");
    hipStream_t st = (hipStream_t)stream;
    const int N = K * B;
    // workspace: gen mean/std (2*N*3) + ref mean/std (2*B*3) floats, then doubles: l1 partials (N*3*chunks) + cos partials
    const size_t nf = (size_t)2 * h->K * h->Bmax * 3 + 2 * h->Bmax * 3, nfp = (nf + 3) / 4 * 4;
    const size_t nd = (size_t)h->K * h->Bmax * 3 * kTrainChunks + kTrainNcos;
    if (!h->train_ws) HIP_TRY(hipMalloc((void**)&h->train_ws, nfp * sizeof(float) + nd * sizeof(double)));
    TrainWs ws;
    ws.gen_mean = h->train_ws; ws.gen_std = ws.gen_mean + N * 3;
    ws.ref_mean = h->train_ws + 2 * h->K * h->Bmax * 3; ws.ref_std = ws.ref_mean + B * 3;
    ws.l1_part = reinterpret_cast<double*>(h->train_ws + nfp); ws.cos_part = ws.l1_part + (size_t)h->K * h->Bmax * 3 * kTrainChunks;

    launch_patch_warp(src_img, h->src_div, h->flow, warp_src_img, K, B, H, W, hh, ww, st);
    const bool pose = h->cfg.pose_composite != 0;       // TSNet_pose.py:399-400 composite before the L1; no alignment loss
    float bg[3];
    for (int c = 0; c < 3; ++c) bg[c] = (-h->cfg.pose_mean[c]) / 255.0f;            // TSNet_pose.py:276
    launch_train_tail(warp_src_img, tar_img, pose ? nullptr : h->pg, pose ? nullptr : h->sg, K, B, H, W, P, C, pose ? 64 : 0, pose ? 192 : 0, bg, ws, losses, st);
    API_END(h)
}

int tsnet_stage_ptr(tsnet_handle h, const char* name, const float** dev_ptr, size_t* count) {
    API_BEGIN(h)
    if (!h->finalized || h->last_B < 1) throw ArgError("stage_ptr before a forward");
    const size_t fe = (size_t)h->P * h->C, B = h->last_B;
    std::string n = name ? name : "";
    const float* p = nullptr; size_t c = 0;
    if (n == "src_fea") { p = h->X; c = (size_t)h->K * (h->last_bank ? h->Bmax : h->last_SB) * fe; }   // K * SB images (K after a forward on a shared source set; every slot after one on a bank)
    else if (n == "tar_fea") { p = h->tar_fea; c = B * fe; }
    else if (n == "pg") { p = h->pg; c = B * fe; }
    else if (n == "sg") { p = h->sg; c = B * fe; }
    else if (n == "dec_map") { p = h->D; c = B * fe; }
    else if (n.rfind("dec_up", 0) == 0 && n.size() == 7 && n[6] >= '0' && n[6] < '0' + h->cfg.n_downsampling) {
        const int i = n[6] - '0';        // raw output of the i-th decoder up-convolution (before its InstanceNorm)
        p = h->R[i]; c = B * ((size_t)(h->h << (i + 1)) * (h->w << (i + 1)) * (h->C >> (i + 1)));
        if (h->st16) {                   // stored as bf16: widened into the (now idle, twice as large) upsampled-input buffer of the same level
            // ordered behind the last forward -- the engine's streams are non-blocking, the NULL stream orders nothing against them
            // ... and not on the caller's stream handle either, which may be gone by now: the forward leaves an event behind its last
            // launch; the engine's own side stream waits for it, widens and is drained before this call returns
            HIP_TRY(hipStreamWaitEvent(h->side_stream, h->ev_done, 0));
            hipLaunchKernelGGL(bf16_widen_kernel, dim3(ew_grid(c)), dim3(256), 0, h->side_stream, reinterpret_cast<const unsigned short*>(h->R[i]), h->U[i], c);
            check_launch("bf16_widen");
            HIP_TRY(hipStreamSynchronize(h->side_stream));
            p = h->U[i];
        }
    }
    else throw ArgError("unknown stage '" + n + "'");
    if (dev_ptr) *dev_ptr = p;
    if (count) *count = c;
    API_END(h)
}

double tsnet_forward_macs(tsnet_handle h, int B) {
    if (!h) return 0.0;
    // SURVEY.md section 8-a closed form, generalised: every conv = M*N*K_real, plus the correlation
    // (one masked GEMM per source) and the soft-argmax.
    const tsnet_cfg& c = h->cfg;
    const double H = c.height, W = c.width, P = h->P, C = h->C, K = h->K;
    auto enc = [&](double cin, int nres) {
        double t = H * W * c.ngf * cin * 49;
        for (int i = 0; i < c.n_downsampling; ++i) {
            const double ho = H / (2 << i), wo = W / (2 << i), ci = c.ngf << i;
            t += ho * wo * (2 * ci) * ci * 9;
        }
        return t + nres * 2.0 * P * C * C * 9;
    };
    const double coords = c.addcoords ? 3 : 0;
    const double fuse = 2.0 * P * (2 * C) * (2 * C) * 9 + P * C * (2 * C);
    double dec = P * C * (2 * C) + c.n_blocks * 2.0 * P * C * C * 9;
    for (int i = 0; i < c.n_downsampling; ++i) {
        const double sp = P * (double)(1 << (2 * (i + 1))), ci = C / (1 << i);
        dec += sp * (ci / 2) * ci * 9;
    }
    dec += H * W * 3 * c.ngf * 49;
    const double corr = K * P * P * C + K * P * P * 2;
    return B * (K * enc(3 + c.label_nc + coords, c.enc_blocks) + enc(c.label_nc + coords, 0) + K * fuse + dec + corr);
}

int tsnet_timing_enable(tsnet_handle h, int on) {
    API_BEGIN(h)
    h->timing.on = on != 0;
    API_END(h)
}

int tsnet_timing_read(tsnet_handle h, double ms_out[TSNET_TIMING_CLASSES], int64_t launches_out[TSNET_TIMING_CLASSES], int reset) {
    API_BEGIN(h)
    h->timing.collect();
    for (int i = 0; i < TSNET_TIMING_CLASSES; ++i) {
        if (ms_out) ms_out[i] = h->timing.ms[i];
        if (launches_out) launches_out[i] = h->timing.launches[i];
        if (reset) { h->timing.ms[i] = 0; h->timing.launches[i] = 0; }
    }
    API_END(h)
}

// ---------------------------------------------------------------------------------------------
// single operators
const char* tsnet_op_last_error(void) { return g_op_error.c_str(); }

namespace {
// one convolution layer with its own packed weights, for the operator entry points
struct OpLayer {
    ConvLayer L;
    DevBufs mem;                  // a member: destroyed even when the constructor throws after the first allocation
    float* wd = nullptr; float* bd = nullptr; float* un = nullptr; unsigned short* wq = nullptr;
    OpLayer(const float* w_oihw, const float* bias, int Cin, int Cout, int ks, int stride, int pad, int reflect, int nprod, hipStream_t s, int form = 0) {
        L.name = "op"; L.cin_real = Cin; L.cin_pad = conv_cin_pad(Cin); L.cin_total = Cin; L.cout = Cout; L.ks = ks; L.stride = stride; L.pad = pad;
        L.reflect = reflect; L.form = form; L.kpad = form == 1 ? conv_kpad_w1(L.cin_pad) : conv_kpad(ks, L.cin_pad); L.npad = conv_npad(Cout);
        if (L.cin_pad != Cin) throw ArgError("conv2d op: Cin must be 8 or a multiple of 16 (pad channels with zeros)");
        if (form == 1 && (ks != 3 || stride != 1 || pad != 1)) throw ArgError("conv2d op: the Winograd form is for 3 x 3 / stride 1 / pad 1");
        size_t wn = (size_t)Cout * Cin * ks * ks;
        std::vector<float> hw(wn);
        HIP_TRY(hipMemcpy(hw.data(), w_oihw, wn * sizeof(float), hipMemcpyDefault));
        if (form == 1) { hw = winograd_x_filters(hw); wn = hw.size(); }
        float mx = 0.f;
        for (float v : hw) mx = std::max(mx, std::fabs(v));
        const bool f16 = nprod == TSNET_NPROD_F16;
        const int planes = (nprod == 1 || f16) ? 1 : 2;
        const int sw = (nprod != 1 && mx > 0.f) ? h2_scale_log2(mx) : 0;
        wd = mem.alloc<float>(wn * sizeof(float));
        wq = mem.alloc<unsigned short>((size_t)L.kpad * L.npad * 2 * planes);
        un = mem.alloc<float>(sizeof(float));
        HIP_TRY(hipMemcpy(wd, hw.data(), wn * sizeof(float), hipMemcpyHostToDevice));
        const float unscale = std::ldexp(1.0f, -sw);
        HIP_TRY(hipMemcpy(un, &unscale, sizeof(float), hipMemcpyHostToDevice));
        pack_layer(wd, L, wq, f16 ? -1 : planes, std::ldexp(1.0f, sw), s);
        if (bias) {
            bd = mem.alloc<float>(Cout * sizeof(float));
            HIP_TRY(hipMemcpy(bd, bias, Cout * sizeof(float), hipMemcpyDefault));
        }
        L.wq = wq; L.w_unscale = nprod == 1 ? nullptr : un; L.bias = bd;
    }
    OpLayer(const OpLayer&) = delete;
    OpLayer& operator=(const OpLayer&) = delete;
};
}  // namespace

int tsnet_op_conv2d(const float* x, int N, int H, int W, int Cin, const float* w_oihw, const float* bias, int Cout,
                    int ksize, int stride, int pad, int pad_mode, const float* in_alpha, const float* in_beta, int in_relu,
                    float bound, int nprod, int kernel, int tile, float* y, void* stream) {
    OP_BEGIN
    if (!x || !w_oihw || !y) throw ArgError("null tensor");
    if (nprod != 1 && nprod != 3 && nprod != 4 && nprod != TSNET_NPROD_F16) throw ArgError("conv2d op: nprod must be 1 (bf16 operands), 16 (fp16 operands: one fp16 plane), 3 or 4 products");
    hipStream_t s = (hipStream_t)stream;
    Ctx ctx(s, current_device_cus());
    ConvRequest req;
    try { req = decode_tile_code(kernel, tile); } catch (const std::invalid_argument& e) { throw ArgError(e.what()); }
    OpLayer op(w_oihw, bias, Cin, Cout, ksize, stride, pad, pad_mode, nprod, s, kernel == 3 ? 1 : 0);     // kernel 3: Winograd-along-x form (conv_w1.hpp)
    ConvCall c; c.x = x; c.alpha = in_alpha; c.beta = in_beta; c.relu = in_relu; c.bound = bound; c.N = N; c.H = H; c.W = W; c.y = y; c.nprod = nprod;
    run_conv(ctx, op.L, c, req);
    HIP_TRY(hipStreamSynchronize(s));
    OP_END
}

// The convolution as the forward calls it: tsnet_op_conv2d plus what conv_epilogue does beside storing y.  Everything the launches index is
// sized from the plan BEFORE the first one; a refusal leaves y, the partials and alpha / beta as they were.
int tsnet_op_conv2d_epi(const float* x, int N, int H, int W, int Cin, const float* w_oihw, const float* bias, int Cout,
                        int ksize, int stride, int pad, int pad_mode, const float* in_alpha, const float* in_beta, int in_relu,
                        float bound, int nprod, int kernel, int tile, float* y, const tsnet_conv_epi* epi, void* stream) {
    OP_BEGIN
    if (!x || !w_oihw || !y || !epi) throw ArgError("null tensor");
    if (nprod != 1 && nprod != 3 && nprod != 4 && nprod != TSNET_NPROD_F16) throw ArgError("conv2d op: nprod must be 1 (bf16 operands), 16 (fp16 operands: one fp16 plane), 3 or 4 products");
    const tsnet_conv_epi& e = *epi;
    if (e.stats < 0 || e.stats > 2) throw ArgError("conv2d_epi op: stats must be 0 (none), 1 (partials + finalize launch) or 2 (arrival counters offered)");
    if (e.repeat < 1) throw ArgError("conv2d_epi op: repeat must be at least 1");
    if (e.stats && (!e.part || !e.alpha || !e.beta)) throw ArgError("conv2d_epi op: statistics need part, alpha and beta");
    if (e.stats == 2 && !e.counters) throw ArgError("conv2d_epi op: stats = 2 needs the arrival counters");
    if (e.addend && (e.add_nmod < 1 || N % e.add_nmod)) throw ArgError("conv2d_epi op: add_nmod must divide N");
    if ((e.x_bf16 || e.y_bf16) && nprod != 1) throw ArgError("conv: bf16 storage goes with bf16 operands");
    hipStream_t s = (hipStream_t)stream;
    Ctx ctx(s, current_device_cus());
    ConvRequest req;
    try { req = decode_tile_code(kernel, tile); } catch (const std::invalid_argument& ex) { throw ArgError(ex.what()); }
    OpLayer op(w_oihw, bias, Cin, Cout, ksize, stride, pad, pad_mode, nprod, s, kernel == 3 ? 1 : 0);
    ConvCall c; c.x = x; c.alpha = in_alpha; c.beta = in_beta; c.relu = in_relu; c.bound = bound; c.N = N; c.H = H; c.W = W; c.y = y; c.nprod = nprod;
    c.addend = e.addend; c.add_nmod = e.addend ? e.add_nmod : 1;
    c.amax_out = e.amax_out; c.in_amax = e.in_amax; c.bound_add = e.bound_add; c.x_bf16 = e.x_bf16; c.y_bf16 = e.y_bf16;
    if (e.stats) {                                      // tsnet_engine::conv_stats' request; stats = 1 withholds the counters
        c.stat_part = e.part; c.fin_alpha = e.alpha; c.fin_beta = e.beta; c.fin_counter = e.stats == 2 ? e.counters : nullptr;
    }
    if (in_alpha && !in_beta) throw ArgError("conv: alpha without beta");
    ConvPlan p;
    try { p = plan_conv(conv_shape(op.L, c), req, ctx.cus); } catch (const std::invalid_argument& ex) { throw ArgError(ex.what()); }
    const size_t part_n = stat_part_doubles((size_t)N, (size_t)p.tpi, (size_t)Cout);
    if (e.stats && (e.part_capacity < 0 || part_n > (size_t)e.part_capacity))
        throw ArgError("conv2d_epi op: part holds " + std::to_string(e.part_capacity) + " doubles, the plan writes N * tpi * Cout * 2 = " + std::to_string(part_n));
    if (e.stats == 2 && (size_t)N * ((op.L.npad + 31) / 32) > kFinCounterInts)
        throw ArgError("conv2d_epi op: more (image, 32-channel group) pairs than arrival counters");
    const int hw = conv_shape(op.L, c).ho() * conv_shape(op.L, c).wo();
    for (int it = 0; it < e.repeat; ++it) {
        // every partial a NaN before each launch: an entry folded before its store is visible, or never written, shows in alpha / beta
        if (e.stats) HIP_TRY(hipMemsetAsync(e.part, 0xFF, part_n * sizeof(double), s));
        if (e.amax_out) HIP_TRY(hipMemsetAsync(e.amax_out, 0, (size_t)N * sizeof(unsigned), s));
        run_conv(ctx, op.L, c, req);
        if (c.stat_S > 0) {                             // not finalised in the kernel: conv_stats' launch
            hipLaunchKernelGGL(in_finalize2_kernel, dim3((Cout + kFin2Ch - 1) / kFin2Ch, N), dim3(256), 0, s, e.part, e.alpha, e.beta, Cout, c.stat_S, hw, 1e-5f);
            check_launch("in_finalize2");
        }
    }
    HIP_TRY(hipStreamSynchronize(s));
    if (e.counters && e.counters_nonzero_out) {
        std::vector<int> hc(kFinCounterInts);
        HIP_TRY(hipMemcpy(hc.data(), e.counters, kFinCounterInts * sizeof(int), hipMemcpyDefault));
        int nz = 0;
        for (int v : hc) nz += v != 0;
        *e.counters_nonzero_out = nz;
    }
    if (e.info_out) {
        int* o = e.info_out;
        o[0] = (int)p.family; o[1] = p.tpi; o[2] = (e.stats && c.stat_S < 0) ? 1 : 0; o[3] = p.w1_chunk; o[4] = p.w1_tab2;
        o[5] = p.rows; o[6] = p.width; o[7] = p.tiles_n;
    }
    OP_END
}

int tsnet_op_upconv2d(const float* x, int N, int H, int W, int Cin, const float* w_oihw, const float* bias, int Cout,
                      int ksize, int stride, int pad, int pad_mode, const float* in_alpha, const float* in_beta, int in_relu,
                      float bound, int nprod, int kernel, int tile, float* y, void* stream) {
    OP_BEGIN
    if (!x || !w_oihw || !y) throw ArgError("null tensor");
    if (ksize != 3 || stride != 1 || pad != 1 || pad_mode != 1) throw ArgError("upconv2d op: a 3 x 3 / stride-1 / pad-1 layer with reflection padding");
    if (nprod != 3) throw ArgError("upconv2d op: fp16 x 2 operands (nprod = 3) and fp32 tensors");
    if (kernel != 0 && kernel != 1) throw ArgError("upconv2d op: kernel 0 (fused) or 1 (upsample2x, then the convolution)");
    if (in_alpha && !in_beta) throw ArgError("upconv2d op: alpha without beta");
    if (N < 1 || H < 1 || W < 1 || (double)N * H * W * 4 * Cin >= 536870912.0) throw ArgError("upconv2d op: empty or too large a tensor");
    hipStream_t s = (hipStream_t)stream;
    Ctx ctx(s, current_device_cus());
    ConvRequest req;
    try { req = decode_tile_code(0, tile); } catch (const std::invalid_argument& e) { throw ArgError(e.what()); }
    OpLayer op(w_oihw, bias, Cin, Cout, ksize, stride, pad, pad_mode, nprod, s);
    // both routes answer to the fused form's plan: what it refuses is refused before anything is launched
    ConvCall c; c.x = x; c.alpha = in_alpha; c.beta = in_beta; c.relu = in_alpha ? in_relu : 0; c.bound = bound; c.N = N; c.H = 2 * H; c.W = 2 * W; c.y = y; c.nprod = nprod;
    c.up2 = true;
    try { (void)plan_conv(conv_shape(op.L, c), req, ctx.cus); } catch (const std::invalid_argument& e) { throw ArgError(e.what()); }
    DevBufs mem;
    if (kernel == 1) {
        float* up = mem.alloc<float>((size_t)N * 2 * H * 2 * W * Cin * sizeof(float));
        run_upsample(ctx, x, in_alpha, in_alpha ? in_beta : nullptr, c.relu, N, H, W, Cin, up);
        c.x = up; c.alpha = nullptr; c.beta = nullptr; c.relu = 0; c.up2 = false;
    }
    run_conv(ctx, op.L, c, req);
    HIP_TRY(hipStreamSynchronize(s));
    OP_END
}

int tsnet_op_conv2d_cat(const float* x, const float* x2, int N, int H, int W, int C1, int C2, int x2_nmod, const float* w_oihw, const float* bias, int Cout,
                        int ksize, int stride, int pad, int pad_mode, float bound, int nprod, float* y, void* stream) {
    OP_BEGIN
    if (!x || !x2 || !w_oihw || !y) throw ArgError("null tensor");
    hipStream_t s = (hipStream_t)stream;
    Ctx ctx(s, current_device_cus());
    OpLayer op(w_oihw, bias, C1 + C2, Cout, ksize, stride, pad, pad_mode, nprod, s);
    ConvCall c; c.x = x; c.x2 = x2; c.csplit = C1; c.x2_nmod = x2_nmod; c.bound = bound; c.N = N; c.H = H; c.W = W; c.y = y; c.nprod = nprod;
    run_conv(ctx, op.L, c);
    HIP_TRY(hipStreamSynchronize(s));
    OP_END
}

int tsnet_op_head(const float* x, int N, int H, int W, int C, const float* in_alpha, const float* in_beta, const float* w_oihw, const float* bias,
                  int composite, const float* bg, float* y, void* stream) {
    OP_BEGIN
    if (!x || !w_oihw || !bias || !y) throw ArgError("null tensor");
    if (C < 4 || (C & 3)) throw ArgError("head op: C must be a multiple of 4");
    if (in_alpha && !in_beta) throw ArgError("head op: alpha without beta");
    HeadRequest hr;
    try { hr = decode_head_code(composite); } catch (const std::invalid_argument& e) { throw ArgError(e.what()); }
    hipStream_t s = (hipStream_t)stream;
    const size_t wn = (size_t)3 * C * 49;
    DevBufs mem;
    float* wd = mem.alloc<float>(wn * sizeof(float));
    float* tab = mem.alloc<float>(((size_t)49 * C * 4 + 64) * sizeof(float));
    float* bd = mem.alloc<float>(4 * sizeof(float));
    HIP_TRY(hipMemsetAsync(tab, 0, ((size_t)49 * C * 4 + 64) * sizeof(float), s));
    HIP_TRY(hipMemcpy(wd, w_oihw, wn * sizeof(float), hipMemcpyDefault));
    HIP_TRY(hipMemcpy(bd, bias, 3 * sizeof(float), hipMemcpyDefault));
    hipLaunchKernelGGL(pack_head_weights_kernel, dim3(64), dim3(256), 0, s, wd, tab, C);
    check_launch("pack_head_weights");
    HeadArgs ha{};
    ha.x = x; ha.alpha = in_alpha; ha.beta = in_alpha ? in_beta : nullptr; ha.w = tab; ha.bias = bd; ha.y = y;
    ha.N = N; ha.H = H; ha.W = W; ha.C = C;
    ha.composite = hr.composite; ha.fore_x0 = 64; ha.fore_x1 = 192;
    for (int c = 0; c < 3; ++c) ha.bg[c] = bg ? bg[c] : 0.f;
    unsigned short* wq = nullptr; float* un = nullptr;
    if (C % 16 == 0 && in_alpha) {         // the folded MFMA form's planes for this call
        std::vector<float> hw(wn);
        HIP_TRY(hipMemcpy(hw.data(), w_oihw, wn * sizeof(float), hipMemcpyDefault));
        float mx = 0.f;
        for (float v : hw) mx = std::max(mx, std::fabs(v));
        const int sw = mx > 0.f ? h2_scale_log2(mx) : 0;
        const float unscale = std::ldexp(1.0f, -sw);
        wq = mem.alloc<unsigned short>(head_mfma_table_halves(C) * sizeof(unsigned short));
        un = mem.alloc<float>(sizeof(float));
        HIP_TRY(hipMemcpy(un, &unscale, sizeof(float), hipMemcpyHostToDevice));
        pack_head_mfma(wd, C, std::ldexp(1.0f, sw), wq, s);
        check_launch("pack_head_mfma");
    }
    launch_head(ha, H, W, N, s, current_device_cus(), hr.rows, wq, un);
    HIP_TRY(hipStreamSynchronize(s));
    OP_END
}

int tsnet_op_instnorm_stats(const float* x, int N, int HW, int C, float* alpha, float* beta, void* stream) {
    OP_BEGIN
    if (!x || !alpha || !beta) throw ArgError("null tensor");
    Ctx ctx((hipStream_t)stream, current_device_cus());
    DevBufs mem;
    double* part = mem.alloc<double>((size_t)N * 64 * C * 2 * sizeof(double));
    run_stats(ctx, x, N, HW, C, part, alpha, beta);
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    OP_END
}

int tsnet_op_norm_act(const float* x, const float* alpha, const float* beta, int relu, const float* resid,
                      int N, int HW, int C, float* y, void* stream) {
    OP_BEGIN
    if (!x || !y) throw ArgError("null tensor");
    Ctx ctx((hipStream_t)stream, current_device_cus());
    run_norm_act(ctx, x, alpha, beta, relu, resid, N, HW, C, y);
    OP_END
}

int tsnet_op_upsample2x(const float* x, const float* alpha, const float* beta, int relu, int N, int H, int W, int C, float* y, void* stream) {
    OP_BEGIN
    if (!x || !y) throw ArgError("null tensor");
    Ctx ctx((hipStream_t)stream, current_device_cus());
    run_upsample(ctx, x, alpha, beta, relu, N, H, W, C, y);
    OP_END
}

// The operator entry points run the forward's kernels, which find a source image through a slot table alone: every spelling of an operator is
// one launch on the table that expresses it.  The table lives in the call's DevBufs, so each of these entries returns after the stream has drained.
static const int* op_table(DevBufs& bufs, const int* t, int n) {      // n host entries -> a device copy
    int* d = bufs.alloc<int>((size_t)n * sizeof(int));
    HIP_TRY(hipMemcpy(d, t, (size_t)n * sizeof(int), hipMemcpyHostToDevice));
    return d;
}
// the legacy spellings' source-batch extent: src holds K * ext images and (source k, frame b) reads image k*ext + b % ext (ext = B: the identity)
static const int* op_table_ext(DevBufs& bufs, int B, int K, int ext) {
    std::vector<int> t((size_t)K * B);
    for (int n = 0; n < K * B; ++n) t[n] = n / B * ext + n % B % ext;
    return op_table(bufs, t.data(), K * B);
}
// a caller's table of n entries in 0 .. n_src - 1
static const int* op_slot_table(DevBufs& bufs, const char* op, const int* slots, int n, int n_src) {
    if (!slots) throw ArgError(std::string(op) + ": null slot table");
    if (n_src < 1) throw ArgError(std::string(op) + ": the number of source images must be >= 1");
    for (int i = 0; i < n; ++i)
        if (slots[i] < 0 || slots[i] >= n_src) throw ArgError(std::string(op) + ": slot " + std::to_string(slots[i]) + " is outside the " + std::to_string(n_src) + " source images");
    return op_table(bufs, slots, n);
}

// tar_fea (B), flow (K*B, image k*B + b).  repeat > 1 re-launches the flow kernel (identical results) for timing.
// slots (host, K*B entries) + n_src: src_fea / src_bbox hold n_src images and (source k, frame b) reads image slots[k*B + b]; null: K*B images, the identity
static void op_flow_impl(const float* tar_fea, const float* src_fea, const float* tar_bbox, const float* src_bbox,
                         int B, int K, int h, int w, int C, int H, int W, float* flow, int variant, int repeat, float* ms_out, hipStream_t stream,
                         const int* slots = nullptr, int n_src = 0) {
    if (!tar_fea || !src_fea || !tar_bbox || !src_bbox || !flow) throw ArgError("null tensor");
    if (B < 1 || K < 1 || K > 8) throw ArgError("flow op: 1 <= K <= 8 sources, B >= 1");
    if (H % h || W % w) throw ArgError("flow op: bbox size must be a multiple of the feature size");
    Ctx ctx(stream, current_device_cus());
    const int P = h * w, NB = K * B;
    DevBufs bufs;
    const int* dslot = slots ? op_slot_table(bufs, "flow op", slots, NB, n_src) : op_table_ext(bufs, B, K, B);
    const int NS = slots ? n_src : NB;                      // source images
    auto* that = bufs.alloc<unsigned short>(flow_plane_halves(B, P, C) * 2);
    auto* shat = bufs.alloc<unsigned short>(flow_plane_halves(NS, P, C) * 2);
    auto* gx = bufs.alloc<float>(w * sizeof(float));
    auto* gy = bufs.alloc<float>(h * sizeof(float));
    std::vector<float> hx(w), hy(h);
    linspace_pm1(w, hx.data()); linspace_pm1(h, hy.data());
    HIP_TRY(hipMemcpy(gx, hx.data(), w * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(gy, hy.data(), h * sizeof(float), hipMemcpyHostToDevice));
    FlowArgs fa{};
    const int G = flowp_plan(B, h, w, C);
    if (G) {
        fa.part = bufs.alloc<unsigned long long>(flowp_part_words(NB, P, flowp_slices(h, w)) * 8);
        fa.cnt = bufs.alloc<int>((size_t)B * (P / 64) * sizeof(int));
        HIP_TRY(hipMemsetAsync(fa.cnt, 0, (size_t)B * (P / 64) * sizeof(int), ctx.stream));
    }
    run_l2norm_split(ctx, tar_fea, that, B, P, C);
    run_l2norm_split(ctx, src_fea, shat, NS, P, C);
    fa.tq = that; fa.sq = shat; fa.tar_bbox = tar_bbox; fa.gx = gx; fa.gy = gy; fa.flow = flow;
    fa.src_bbox = src_bbox;
    fa.B = B; fa.P = P; fa.C = C; fa.h = h; fa.w = w; fa.H = H; fa.W = W; fa.sy = H / h; fa.sx = W / w;
    std::unique_ptr<EventPair> ev(ms_out ? new EventPair : nullptr);
    run_flow(ctx, fa, NB, dslot, variant);
    if (ev) HIP_TRY(hipEventRecord(ev->a, ctx.stream));
    for (int r = 1; r < repeat; ++r) run_flow(ctx, fa, NB, dslot, variant);
    if (ev) HIP_TRY(hipEventRecord(ev->b, ctx.stream));
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    if (ms_out) *ms_out = repeat > 1 ? ev->ms() / (float)(repeat - 1) : 0.f;
}

int tsnet_op_flow(const float* tar_fea, const float* src_fea, const float* tar_bbox, const float* src_bbox,
                  int B, int h, int w, int C, int H, int W, float* flow, void* stream) {
    OP_BEGIN
    op_flow_impl(tar_fea, src_fea, tar_bbox, src_bbox, B, 1, h, w, C, H, W, flow, 0, 1, nullptr, (hipStream_t)stream);
    OP_END
}

int tsnet_op_flow_k(const float* tar_fea, const float* src_fea, const float* tar_bbox, const float* src_bbox,
                    int B, int K, int h, int w, int C, int H, int W, float* flow, int variant, int repeat, float* ms_out, void* stream) {
    OP_BEGIN
    op_flow_impl(tar_fea, src_fea, tar_bbox, src_bbox, B, K, h, w, C, H, W, flow, variant, repeat, ms_out, (hipStream_t)stream);
    OP_END
}

int tsnet_op_flow_k_slots(const float* tar_fea, const float* src_fea, const float* tar_bbox, const float* src_bbox,
                          int B, int K, int h, int w, int C, int H, int W, float* flow, int variant, int repeat, float* ms_out,
                          const int* slots, int n_src, void* stream) {
    OP_BEGIN
    if (!slots) throw ArgError("flow op: null slot table");
    op_flow_impl(tar_fea, src_fea, tar_bbox, src_bbox, B, K, h, w, C, H, W, flow, variant, repeat, ms_out, (hipStream_t)stream, slots, n_src);
    OP_END
}

int tsnet_flow_plan(int B, int h, int w, int C) { return (B < 1 || h < 1 || w < 1 || C < 8 || (C & 7)) ? -1 : flowp_plan(B, h, w, C); }

int tsnet_op_warp(const float* src_fea, const float* flow, int B, int h, int w, int C, float* out, void* stream) {
    OP_BEGIN
    if (!src_fea || !flow || !out) throw ArgError("null tensor");
    if (C & 3) throw ArgError("warp op: C must be a multiple of 4");
    Ctx ctx((hipStream_t)stream, current_device_cus());
    DevBufs mem;
    run_warp(ctx, src_fea, op_table_ext(mem, B, 1, B), flow, out, B, 1, h, w, C);
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    OP_END
}

int tsnet_op_warp_k(const float* src_fea, const float* flow, int B, int K, int h, int w, int C, float* out, int repeat, float* ms_out, void* stream) {
    OP_BEGIN
    if (!src_fea || !flow || !out) throw ArgError("null tensor");
    if (C & 3) throw ArgError("warp op: C must be a multiple of 4");
    if (B < 1 || K < 1 || K > TSNET_MAX_SOURCES || h < 1 || w < 1) throw ArgError("warp op: bad shape");
    Ctx ctx((hipStream_t)stream, current_device_cus());
    if (ms_out) *ms_out = 0.f;
    DevBufs mem;
    const int* d = op_table_ext(mem, B, K, B);        // uploaded once, outside the events
    run_warp(ctx, src_fea, d, flow, out, B, K, h, w, C);
    if (repeat > 1) {                    // launches 2 .. repeat between two events: the kernel ALONE (tools/warp_bench.py)
        EventPair ev;
        HIP_TRY(hipEventRecord(ev.a, ctx.stream));
        for (int i = 1; i < repeat; ++i) run_warp(ctx, src_fea, d, flow, out, B, K, h, w, C);
        HIP_TRY(hipEventRecord(ev.b, ctx.stream));
        const float t = ev.ms();
        if (ms_out) *ms_out = t / (float)(repeat - 1);
    }
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    OP_END
}

// tsnet_op_warp_k_shared (ext = its SB) and tsnet_op_warp_k_slots (ext < 0: the caller's table)
static void op_warp_any(const float* src_fea, const float* flow, int B, int K, int ext, const int* slots, int n_src, int h, int w, int C, float* out, void* stream) {
    if (!src_fea || !flow || !out) throw ArgError("warp op: null tensor");
    if (C < 4 || (C & 3)) throw ArgError("warp op: C must be a multiple of 4");
    if (B < 1 || K < 1 || K > TSNET_MAX_SOURCES || h < 1 || w < 1) throw ArgError("warp op: bad shape (1 <= K <= 8 sources, B, h, w >= 1)");
    if (ext >= 0 && (ext < 1 || B % ext)) throw ArgError("warp op: the source-batch extent must divide the batch");
    Ctx ctx((hipStream_t)stream, current_device_cus());
    DevBufs mem;
    run_warp(ctx, src_fea, ext >= 0 ? op_table_ext(mem, B, K, ext) : op_slot_table(mem, "warp op", slots, K * B, n_src), flow, out, B, K, h, w, C);
    HIP_TRY(hipStreamSynchronize(ctx.stream));
}

int tsnet_op_warp_k_shared(const float* src_fea, const float* flow, int B, int K, int SB, int h, int w, int C, float* out, void* stream) {
    OP_BEGIN
    op_warp_any(src_fea, flow, B, K, SB < 0 ? 0 : SB, nullptr, 0, h, w, C, out, stream);
    OP_END
}

int tsnet_op_warp_k_slots(const float* src_fea, const float* flow, int B, int K, int h, int w, int C, float* out, const int* slots, int n_src, void* stream) {
    OP_BEGIN
    op_warp_any(src_fea, flow, B, K, -1, slots, n_src, h, w, C, out, stream);
    OP_END
}

// tsnet_op_add_stats (ext = its x_sb) and tsnet_op_add_stats_slots (ext < 0: the caller's table)
static void op_add_stats_any(const float* x, const float* add, int add_nmod, int ext, const int* slots, int n_src, int N, int HW, int C,
                             float* y, float* alpha, float* beta, void* stream) {
    if (!x || !add || !y || !alpha || !beta) throw ArgError("add_stats op: null tensor");
    if (C < 4 || (C & 3)) throw ArgError("add_stats op: C must be a multiple of 4");
    if (N < 1 || N > 65535 || HW < 1) throw ArgError("add_stats op: bad shape (1 <= N <= 65535, HW >= 1)");
    if (add_nmod < 1 || N % add_nmod) throw ArgError("add_stats op: add_nmod must divide N");
    if (ext >= 0 && (ext < 1 || add_nmod % ext)) throw ArgError("add_stats op: the source-batch extent must divide add_nmod");
    Ctx ctx((hipStream_t)stream, current_device_cus());
    DevBufs mem;
    const int* d = ext >= 0 ? op_table_ext(mem, add_nmod, N / add_nmod, ext) : op_slot_table(mem, "add_stats op", slots, N, n_src);
    double* part = mem.alloc<double>((size_t)N * 64 * C * 2 * sizeof(double));
    run_add_stats(ctx, x, d, add, add_nmod, y, N, HW, C, part, alpha, beta);
    HIP_TRY(hipStreamSynchronize(ctx.stream));
}

int tsnet_op_add_stats(const float* x, const float* add, int add_nmod, int x_sb, int N, int HW, int C, float* y, float* alpha, float* beta, void* stream) {
    OP_BEGIN
    op_add_stats_any(x, add, add_nmod, x_sb < 0 ? 0 : x_sb, nullptr, 0, N, HW, C, y, alpha, beta, stream);
    OP_END
}

int tsnet_op_add_stats_slots(const float* x, const float* add, int add_nmod, int N, int HW, int C, float* y, float* alpha, float* beta,
                             const int* slots, int n_src, void* stream) {
    OP_BEGIN
    op_add_stats_any(x, add, add_nmod, -1, slots, n_src, N, HW, C, y, alpha, beta, stream);
    OP_END
}

int tsnet_op_finalize_stats(const double* part, int N, int S, int C, int HW, float* alpha, float* beta, void* stream) {
    OP_BEGIN
    if (!part || !alpha || !beta) throw ArgError("finalize op: null tensor");
    if (C < 4 || (C & 3)) throw ArgError("finalize op: C must be a multiple of 4");
    if (N < 1 || N > 65535 || S < 1 || HW < 1) throw ArgError("finalize op: bad shape (1 <= N <= 65535, S >= 1, HW >= 1)");
    launch_finalize(part, alpha, beta, N, C, S, HW, (hipStream_t)stream);
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    OP_END
}

// tsnet_op_fuse_tail (ext = its SB) and tsnet_op_fuse_tail_slots (ext < 0: the caller's table)
static void op_fuse_tail_any(const float* src_fea, const float* tar_fea, const float* y2, const float* alpha, const float* beta,
                             int B, int K, int ext, const int* slots, int n_src, int P, int C1, float* zbar, void* stream) {
    if (!src_fea || !tar_fea || !y2 || !alpha || !beta || !zbar) throw ArgError("fuse_tail op: null tensor");
    if (C1 < 4 || (C1 & 3)) throw ArgError("fuse_tail op: C1 must be a multiple of 4");
    if (B < 1 || K < 1 || K > TSNET_MAX_SOURCES || P < 1) throw ArgError("fuse_tail op: bad shape (1 <= K <= 8 sources, B, P >= 1)");
    if (ext >= 0 && (ext < 1 || B % ext)) throw ArgError("fuse_tail op: the source-batch extent must divide the batch");
    Ctx ctx((hipStream_t)stream, current_device_cus());
    DevBufs mem;
    const int* d = ext >= 0 ? op_table_ext(mem, B, K, ext) : op_slot_table(mem, "fuse_tail op", slots, K * B, n_src);
    run_fuse_tail(ctx, FuseTailArgs{src_fea, tar_fea, y2, alpha, beta, zbar, d, B, K, P, C1});
    HIP_TRY(hipStreamSynchronize(ctx.stream));
}

int tsnet_op_fuse_tail(const float* src_fea, const float* tar_fea, const float* y2, const float* alpha, const float* beta,
                       int B, int K, int SB, int P, int C1, float* zbar, void* stream) {
    OP_BEGIN
    op_fuse_tail_any(src_fea, tar_fea, y2, alpha, beta, B, K, SB < 0 ? 0 : SB, nullptr, 0, P, C1, zbar, stream);
    OP_END
}

int tsnet_op_fuse_tail_slots(const float* src_fea, const float* tar_fea, const float* y2, const float* alpha, const float* beta,
                             int B, int K, int P, int C1, float* zbar, const int* slots, int n_src, void* stream) {
    OP_BEGIN
    op_fuse_tail_any(src_fea, tar_fea, y2, alpha, beta, B, K, -1, slots, n_src, P, C1, zbar, stream);
    OP_END
}

int tsnet_op_patch_warp(const float* const* src_img, const float* div, const float* flow, int K, int B, int H, int W, int h, int w, float* out,
                        void* stream) {
    OP_BEGIN
    if (K < 1 || K > TSNET_MAX_SOURCES) throw ArgError("patch_warp op: 1 <= K <= 8 sources");
    if (!src_img || !div || !flow || !out) throw ArgError("patch_warp op: null tensor");
    for (int s = 0; s < K; ++s) {
        if (!src_img[s]) throw ArgError("patch_warp op: null source image (need K entries)");
        if (!(div[s] > 0.f)) throw ArgError("patch_warp op: the image divisors must be positive");
    }
    if (B < 1 || H < 1 || W < 1 || h < 1 || w < 1 || (double)H * W >= 2147483647.0 || (double)K * B * h * w >= 2147483647.0 / 2)
        throw ArgError("patch_warp op: bad shape (B, H, W, h, w >= 1)");
    if (H % h || W % w || H / h != W / w) throw ArgError("patch_warp op: image size must be a multiple of the feature size, the same along both axes");
    launch_patch_warp(src_img, div, flow, out, K, B, H, W, h, w, (hipStream_t)stream);
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    OP_END
}

int tsnet_op_train_tail(float* x, const float* tar_img, const float* pg, const float* sg, int K, int B, int H, int W, int P, int C,
                        int fore_x0, int fore_x1, const float* bg, float* gen_mean, float* gen_std, float* ref_mean, float* ref_std,
                        float* losses, void* stream) {
    OP_BEGIN
    if (!x || !tar_img || !losses) throw ArgError("train_tail op: null tensor");
    if (K < 1 || K > TSNET_MAX_SOURCES) throw ArgError("train_tail op: 1 <= K <= 8 sources");
    if (B < 1 || (size_t)K * B > 65535 || H < 1 || W < 1 || (double)H * W >= 2147483647.0) throw ArgError("train_tail op: bad shape (B, H, W >= 1, K * B <= 65535)");
    if ((pg == nullptr) != (sg == nullptr)) throw ArgError("train_tail op: pg and sg come together (both null: the pose form)");
    if (pg) {
        if (C < 4 || (C & 3)) throw ArgError("train_tail op: C must be a multiple of 4");
        if (P < 1 || (double)B * P >= 2147483647.0) throw ArgError("train_tail op: bad shape (P >= 1)");
        if (((uintptr_t)pg & 15) || ((uintptr_t)sg & 15)) throw ArgError("train_tail op: pg and sg must be 16-byte aligned");
    }
    const float zero[3] = {0.f, 0.f, 0.f};
    if (fore_x1 > fore_x0 && !bg) throw ArgError("train_tail op: the composite needs its background");
    hipStream_t st = (hipStream_t)stream;
    const size_t N = (size_t)K * B, nl1 = N * 3 * kTrainChunks;
    DevBufs mem;
    float* fs = mem.alloc<float>((2 * N * 3 + 2 * (size_t)B * 3) * sizeof(float));
    double* ds = mem.alloc<double>((nl1 + kTrainNcos) * sizeof(double));
    HIP_TRY(hipMemsetAsync(ds, 0xFF, (nl1 + kTrainNcos) * sizeof(double), st));       // every partial a NaN: a slot read before it is written shows in the losses
    TrainWs ws;
    ws.gen_mean = gen_mean ? gen_mean : fs; ws.gen_std = gen_std ? gen_std : fs + N * 3;
    ws.ref_mean = ref_mean ? ref_mean : fs + 2 * N * 3; ws.ref_std = ref_std ? ref_std : fs + 2 * N * 3 + (size_t)B * 3;
    ws.l1_part = ds; ws.cos_part = ds + nl1;
    launch_train_tail(x, tar_img, pg, sg, K, B, H, W, P, C, fore_x0, fore_x1, bg ? bg : zero, ws, losses, st);
    HIP_TRY(hipStreamSynchronize(st));
    OP_END
}

// both forms of the packing op: the checks, the coordinate table, the launch
static void op_pack_any(bool u8, const void* const* img, const void* const* lbl, const void* const* bbox, int S, int B, int H, int W, int L, int nimg,
                        int Cp, int coords, const float* img_div, const float* mean, float* out, float* bbox_out, unsigned int* amax, void* stream) {
    if (S < 1 || S > TSNET_MAX_SOURCES) throw ArgError("pack op: 1 <= S <= 8 sources");
    if (!lbl || !out || !amax) throw ArgError("pack op: null tensor");
    if (nimg != 0 && nimg != 3) throw ArgError("pack op: nimg is 3 (image + label) or 0 (label only)");
    if (nimg && (!img || !img_div)) throw ArgError("pack op: null tensor");
    for (int s = 0; s < S; ++s) {
        if (!lbl[s] || (nimg && !img[s])) throw ArgError("pack op: null tensor");
        if (nimg && !(img_div[s] > 0.f)) throw ArgError("pack op: the image divisors must be positive");
    }
    if (B < 1 || (size_t)S * B > 65535 || H < 1 || W < 1 || L < 1) throw ArgError("pack op: bad shape (B, H, W, L >= 1, S * B <= 65535)");
    if (coords && (H < 2 || W < 2)) throw ArgError("pack op: the coordinate table needs H, W >= 2");
    const int creal = nimg + L + (coords ? 3 : 0);
    if (Cp < creal) throw ArgError("pack op: Cp is smaller than the real channel count");
    if (Cp != conv_cin_pad(Cp)) throw ArgError("pack op: Cp must be 8 or a multiple of 16");
    if (u8) {
        if (L > 255) throw ArgError("pack op: class indices are bytes (L <= 255)");
        if (nimg && !mean) throw ArgError("pack op: null tensor");
        if (bbox) {
            if (!bbox_out) throw ArgError("pack op: null tensor");
            for (int s = 0; s < S; ++s) if (!bbox[s]) throw ArgError("pack op: null tensor");
        }
    }
    Ctx ctx((hipStream_t)stream, current_device_cus());
    DevBufs mem;
    PackArgs p{};
    for (int s = 0; s < S; ++s) p.img_div[s] = nimg ? img_div[s] : 1.f;
    if (coords) {                                   // as tsnet_finalize builds d_coords
        std::vector<float> t((size_t)H * W * 3);
        coord_table(H, W, t.data());
        float* d = mem.alloc<float>(t.size() * sizeof(float));
        HIP_TRY(hipMemcpy(d, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice));
        p.coords = d;
    }
    p.out = out; p.S = S; p.B = B; p.H = H; p.W = W; p.L = L; p.nimg = nimg; p.Cp = Cp; p.amax_out = amax;
    run_pack_any(ctx, p, (size_t)S * B, u8, nimg ? img : nullptr, lbl, bbox, mean, bbox_out, (size_t)B * H * W);
    HIP_TRY(hipStreamSynchronize(ctx.stream));
}

int tsnet_op_pack_input(const float* const* img, const float* const* lbl, int S, int B, int H, int W, int L, int nimg, int Cp, int coords,
                        const float* img_div, float* out, unsigned int* amax, void* stream) {
    OP_BEGIN
    op_pack_any(false, vlist(img), vlist(lbl), nullptr, S, B, H, W, L, nimg, Cp, coords, img_div, nullptr, out, nullptr, amax, stream);
    OP_END
}

int tsnet_op_pack_input_u8(const uint8_t* const* img, const uint8_t* const* lbl, const uint8_t* const* bbox, int S, int B, int H, int W, int L,
                           int nimg, int Cp, int coords, const float* img_div, const float* mean_bgr, float* out, float* bbox_out,
                           unsigned int* amax, void* stream) {
    OP_BEGIN
    op_pack_any(true, vlist(img), vlist(lbl), vlist(bbox), S, B, H, W, L, nimg, Cp, coords, img_div, mean_bgr, out, bbox_out, amax, stream);
    OP_END
}

int tsnet_op_upsample2x_st(const float* x, const float* alpha, const float* beta, int relu, int N, int H, int W, int C, int x_bf16, int y_bf16,
                           float* y, void* stream) {
    OP_BEGIN
    if (!x || !y) throw ArgError("upsample op: null tensor");
    if (alpha && !beta) throw ArgError("upsample op: alpha without beta");
    if (C < 4 || (C & 3)) throw ArgError("upsample op: C must be a multiple of 4");
    if (N < 1 || H < 1 || W < 1) throw ArgError("upsample op: bad shape (N, H, W >= 1)");
    Ctx ctx((hipStream_t)stream, current_device_cus());
    run_upsample(ctx, x, alpha, beta, relu, N, H, W, C, y, x_bf16 != 0, y_bf16 != 0);
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    OP_END
}

int tsnet_bench_conv(int N, int H, int W, int Cin, int Cout, int ksize, int stride, int pad, int pad_mode, int norm,
                     int variant, int iters, float* ms_out, void* stream) {
    OP_BEGIN
    if (iters < 1 || !ms_out) throw ArgError("bench_conv: bad argument");
    hipStream_t s = (hipStream_t)stream;
    Ctx ctx(s, current_device_cus());
    // variant (-1 = the layer's own kernel and tile): conv_plan.hpp decode_bench_variant
    BenchVariant bv;
    try { bv = decode_bench_variant(variant); } catch (const std::invalid_argument& e) { throw ArgError(e.what()); }
    const int nprod = bv.nprod;
    const int Ho = (H + 2 * pad - ksize) / stride + 1, Wo = (W + 2 * pad - ksize) / stride + 1;
    const size_t xn = (size_t)N * H * W * Cin, yn = (size_t)N * Ho * Wo * Cout, wn = (size_t)Cout * Cin * ksize * ksize;
    DevBufs mem;
    float* x = mem.alloc<float>(xn * 4); float* y = mem.alloc<float>(yn * 4);
    float* al = mem.alloc<float>((size_t)N * Cin * 4); float* be = mem.alloc<float>((size_t)N * Cin * 4);
    // pseudo-random fill (not zeros: MI355X clocks higher on zero operands, cdna_hip_programming.md rule 25)
    std::vector<float> hbuf(std::max(std::max(xn, wn), (size_t)N * Cin));
    unsigned st = 12345u;
    auto fill = [&](float* d, size_t n, float scale, float off) {
        for (size_t i = 0; i < n; ++i) { st = st * 1664525u + 1013904223u; hbuf[i] = off + scale * ((float)(st >> 8) / 16777216.0f - 0.5f); }
        if (d) HIP_TRY(hipMemcpy(d, hbuf.data(), n * 4, hipMemcpyHostToDevice));
    };
    fill(x, xn, 2.f, 0.f); fill(al, (size_t)N * Cin, 1.f, 1.f); fill(be, (size_t)N * Cin, 0.5f, 0.f);
    fill(nullptr, wn, 0.1f, 0.f);
    {
        const int form = bv.form;
        OpLayer op(hbuf.data(), nullptr, Cin, Cout, ksize, stride, pad, pad_mode, nprod, s, form);
        // COLD weights -- every launch reads another copy of the packed planes (24 copies: beyond the 256 MiB Infinity Cache for the
        // big layers), as consecutive layers of a forward do; the default re-launches one layer, whose planes stay cache-resident
        std::vector<std::unique_ptr<OpLayer>> cold;
        if (bv.cold) for (int i = 0; i < 24; ++i) cold.emplace_back(new OpLayer(hbuf.data(), nullptr, Cin, Cout, ksize, stride, pad, pad_mode, nprod, s, form));
        ConvCall c; c.x = x; c.N = N; c.H = H; c.W = W; c.y = y; c.bound = (norm & 1) ? 64.f : 1.f; c.nprod = nprod;
        if (norm & 1) { c.alpha = al; c.beta = be; c.relu = 1; }
        if (norm & 2) {                                              // with the InstanceNorm statistics of the output, as the forward's layers run
            const size_t tpi = ((size_t)Ho * Wo + 63) / 64;
            c.stat_part = mem.alloc<double>(stat_part_doubles(N, tpi, Cout) * sizeof(double));
            c.fin_alpha = mem.alloc<float>((size_t)N * Cout * 4); c.fin_beta = mem.alloc<float>((size_t)N * Cout * 4);
            c.fin_counter = mem.alloc<int>(kFinCounterInts * sizeof(int));
            HIP_TRY(hipMemset(c.fin_counter, 0, kFinCounterInts * sizeof(int)));
        }
        for (int i = 0; i < 2; ++i) run_conv(ctx, op.L, c, bv.req);
        EventPair ev;
        HIP_TRY(hipEventRecord(ev.a, s));
        for (int i = 0; i < iters; ++i) run_conv(ctx, cold.empty() ? op.L : cold[(size_t)i % cold.size()]->L, c, bv.req);
        HIP_TRY(hipEventRecord(ev.b, s));
        *ms_out = ev.ms() / iters;
    }
    OP_END
}

#ifdef TSNET_TOOLS
void tsnet_tools_set(int key, int value) { if (key >= 0 && key < 8) g_tools_knob[key] = value; }      // not in the product library / ABI header
#endif
void tsnet_debug_counters(int64_t out[4], int reset) {
    for (int i = 0; i < 4; ++i) { if (out) out[i] = g_launch_counters[i]; if (reset && i < 3) g_launch_counters[i] = 0; }
}

void tsnet_linspace(int n, float* out) { linspace_pm1(n, out); }
void tsnet_coord_table(int H, int W, float* out) { coord_table(H, W, out); }

}  // extern "C"

#define TSNET_ENGINE_CPP      // clip_entries.hpp refuses every other includer
#include "clip_entries.hpp"
