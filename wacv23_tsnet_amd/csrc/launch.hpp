// launch.hpp -- how the host launches the kernels of the forward, and the small types that go with it: the timing of launch classes (Timing,
// TimeScope, EventPair), what a launch needs (Ctx), the owners of device memory, streams and events (DevBufs, Owned), a convolution layer and
// a call on it (ConvLayer, ConvCall, run_conv: the one place a ConvPlan of conv_plan.hpp becomes kernel arguments), the run_* / launch_* helper
// of every other kernel, weight packing and the constant tables.  Nothing here knows tsnet_engine: the engine (engine.cpp) and the
// single-operator entries (op_entries.hpp) launch through the same helpers.  engine.cpp includes this file once, ahead of its own code: it is
// part of that translation unit and of no other, and everything in it has internal linkage.  HOST code.
#pragma once
#ifndef TSNET_ENGINE_CPP
#error "launch.hpp is the head of engine.cpp: include it from there only"
#endif
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

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
// launch(0 .. n-1) between two events on s: the mean milliseconds of one launch, once the last has completed (n < 1: nothing launched, 0)
template <typename F>
float timed_repeats(hipStream_t s, int n, F&& launch) {
    if (n < 1) return 0.f;
    EventPair ev;
    HIP_TRY(hipEventRecord(ev.a, s));
    for (int i = 0; i < n; ++i) launch(i);
    HIP_TRY(hipEventRecord(ev.b, s));
    return ev.ms() / (float)n;
}

struct Timing {
    bool on = false;
    struct Rec { int cls; EventPair ev; };      // a record owns its events: those never collected go with the Timing
    std::vector<std::unique_ptr<Rec>> recs;
    double ms[TSNET_TIMING_CLASSES] = {0};
    int64_t launches[TSNET_TIMING_CLASSES] = {0};
    void begin(int cls, hipStream_t s) {
        if (!on) return;
        std::unique_ptr<Rec> r(new Rec{cls, {}});
        HIP_TRY(hipEventRecord(r->ev.a, s));
        recs.push_back(std::move(r));
    }
    void end(hipStream_t s) {
        if (!on) return;
        HIP_TRY(hipEventRecord(recs.back()->ev.b, s));
    }
    void collect() {
        for (auto& r : recs) {
            ms[r->cls] += r->ev.ms();
            launches[r->cls] += 1;
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

// a stream or an event of the engine's: the holder destroys what was created into `v` (reset: now).  Reads as the handle it holds.
template <typename T, hipError_t (*Destroy)(T)>
struct Owned {
    T v = nullptr;
    Owned() = default;
    Owned(const Owned&) = delete;
    Owned& operator=(const Owned&) = delete;
    ~Owned() { reset(); }
    void reset() { if (v) (void)Destroy(v); v = nullptr; }
    operator T() const { return v; }
};
using OwnedStream = Owned<hipStream_t, hipStreamDestroy>;
using OwnedEvent = Owned<hipEvent_t, hipEventDestroy>;

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

// device allocations of an operator entry point (freed on every exit path: a rejected tile / variant throws out of run_conv routinely) or of
// an engine (freed with it; release: now, when a finalize is taken back)
struct DevBufs {
    std::vector<void*> p;
    template <typename T> T* alloc(size_t bytes) { p.push_back(nullptr); HIP_TRY(hipMalloc(&p.back(), bytes)); return static_cast<T*>(p.back()); }
    void release() { for (void* q : p) (void)hipFree(q); p.clear(); }
    ~DevBufs() { release(); }
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

// the power-of-two scale of a filter from its largest |w|: |w * 2^sw| <= 2^15 (sw = 0 where `apply` is false or the filter is all zeros).
// who: the parameter's name where a non-finite value is refused (the engine's weights); null: not looked at, as the operators always did
struct WeightScale { int sw; float scale, unscale; };       // 2^sw, 2^-sw
inline WeightScale weight_scale(const std::vector<float>& w, bool apply, const std::string* who = nullptr) {
    float mx = 0.f;                      // the largest |w|; where non-finite values are refused a NaN sticks to it, elsewhere it is passed over
    for (float v : w) { const float av = std::fabs(v); if (av > mx || (who && av != av)) mx = av; }
    if (who && !std::isfinite(mx)) throw WeightError("parameter '" + *who + "' holds a non-finite value");
    const int sw = (apply && mx > 0.f) ? h2_scale_log2(mx) : 0;
    return {sw, std::ldexp(1.0f, sw), std::ldexp(1.0f, -sw)};
}

constexpr float kInEps = 1e-5f;      // InstanceNorm's epsilon (torch.nn.InstanceNorm2d's default, the reference's), in every finalize

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
    const ConvPlan p = arg_checked([&] { return plan_conv(sh, req, ctx.cus); });
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
    g.fin_alpha = c.fin_alpha; g.fin_beta = c.fin_beta; g.fin_eps = kInEps;
    // the one place a plan's launch geometry enters the kernel arguments
    g.tpi = p.tpi; g.tiles_m = p.tiles_m; g.tiles_n = p.tiles_n; g.fin_S = p.tpi; g.xcd_gn = p.xcd_gn;
    g.w1_chunk = p.w1_chunk; g.w1_tab2 = p.w1_tab2; g.fin_counter = p.fin ? c.fin_counter : nullptr;
    TimeScope ts(ctx, c.tclass);
    arg_checked([&] {                                                            // (refused: a tools-build variant that is not instantiated)
        switch (p.family) {
        case ConvFamily::W1: launch_conv_w1(g, c.nprod, req.abl, ctx.stream); break;
        case ConvFamily::H2: launch_conv_h2(g, p, c.nprod, req.abl, req.opt, ctx.stream); break;
        case ConvFamily::H2S: launch_conv_h2s(g, c.nprod, ctx.stream); break;
        case ConvFamily::H2S32: launch_conv_h2s32(g, c.nprod, ctx.stream); break;
        case ConvFamily::H2D: launch_conv_h2d(g, p, c.nprod, ctx.stream); break;
        case ConvFamily::G64: launch_conv_g64(g, p, c.nprod, ctx.stream); break;
        case ConvFamily::H2R: launch_conv_h2r(g, p, c.nprod, ctx.stream); break;
        }
    });
    ++g_launch_counters[p.family == ConvFamily::G64 || p.family == ConvFamily::H2R ? 1 : 0];
    if (c.tclass == TSNET_T_CONV_RES && plan_tile_code(p)) g_launch_counters[3] = plan_tile_code(p);
    check_launch("conv");
    c.stat_S = !c.stat_part ? 0 : (g.fin_counter ? -1 : g.tpi);
}

// the in_finalize2 launch: S partials per (image, channel) -> (alpha, beta).  The caller checks the launch under its own name.
inline void launch_finalize2(const double* part, float* alpha, float* beta, int N, int C, int S, int HW, hipStream_t s) {
    hipLaunchKernelGGL(in_finalize2_kernel, dim3((C + kFin2Ch - 1) / kFin2Ch, N), dim3(256), 0, s, part, alpha, beta, C, S, HW, kInEps);
}

// stage 2 of the stand-alone statistics: with more than a handful of partials per image the 16-group kernel (one serial walk per (image,
// channel) is latency-bound: 39 us for the 64 partials of the FuseNet join).  The two kernels add in different orders.
void launch_finalize(const double* part, float* alpha, float* beta, int N, int C, int S, int HW, hipStream_t s) {
    if (S > 8) {
        launch_finalize2(part, alpha, beta, N, C, S, HW, s);
    } else {
        const int NC = N * C;
        hipLaunchKernelGGL(in_finalize_kernel, dim3((NC + 255) / 256), dim3(256), 0, s, part, alpha, beta, NC, C, S, HW, kInEps);
    }
    check_launch("in_finalize");
}

// how the statistics kernels split an image of HW positions x C channels: S partials of rps rows each, and the grid over N images
struct StatSplit { int S, rps; dim3 grid; };
constexpr int kStatMaxSplits = 64;
inline StatSplit stat_split(int N, int HW, int C) {
    const int cq = C / 4, cols = cq < 256 ? cq : 256, R = 256 / cols;
    int S = (HW + R * 8 - 1) / (R * 8);
    if (S > kStatMaxSplits) S = kStatMaxSplits;
    if (S < 1) S = 1;
    const int rps = (HW + S - 1) / S;
    S = (HW + rps - 1) / rps;
    return {S, rps, dim3(S, N, (cq + 255) / 256)};
}
// doubles the `part` scratch of run_stats / run_add_stats must hold, whatever HW is: every split stat_split may choose
inline size_t stat_scratch_doubles(size_t N, size_t C) { return stat_part_doubles(N, kStatMaxSplits, C); }

// InstanceNorm statistics -> (alpha, beta); `part` must hold stat_scratch_doubles(N, C) doubles
void run_stats(Ctx& ctx, const float* x, int N, int HW, int C, double* part, float* alpha, float* beta) {
    if (C & 3) throw ArgError("instnorm: C must be a multiple of 4");
    TimeScope ts(ctx, TSNET_T_STATS);
    const StatSplit sp = stat_split(N, HW, C);
    StatsArgs sa{x, part, HW, C, sp.S, sp.rps};
    hipLaunchKernelGGL(in_stats_partial_kernel, sp.grid, dim3(256), 0, ctx.stream, sa);
    check_launch("in_stats_partial");
    launch_finalize(part, alpha, beta, N, C, sp.S, HW, ctx.stream);
}

// y[n] = x[slot[n]] + add[n % add_nmod] with the InstanceNorm statistics of y -> (alpha, beta); `part` must hold stat_scratch_doubles(N, C) doubles; slot: device, N ints
void run_add_stats(Ctx& ctx, const float* x, const int* slot, const float* add, int add_nmod, float* y, int N, int HW, int C, double* part, float* alpha, float* beta) {
    if (C & 3) throw ArgError("add_stats: C must be a multiple of 4");
    TimeScope ts(ctx, TSNET_T_STATS);
    const StatSplit sp = stat_split(N, HW, C);
    const int nmod = add_nmod > 0 ? add_nmod : 1;
    AddStatsArgs sa{x, slot, add, y, part, HW, C, sp.S, sp.rps, nmod};
    hipLaunchKernelGGL(add_stats_partial_kernel, sp.grid, dim3(256), 0, ctx.stream, sa);
    check_launch("add_stats_partial");
    // (its finalize stays a launch: 64 splits x 1024 channels per image are a megabyte of partials -- one last-arriving workgroup per image
    // would read them at a single block's rate, in_finalize2 spreads them over 64 x N)
    launch_finalize(part, alpha, beta, N, C, sp.S, HW, ctx.stream);
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
        arg_checked([&] { launch_flow_p(a, variant, ctx.stream); });
        check_launch("flow_p");
        return;
    }
    // 64 target positions per workgroup while their planes fit in LDS beside the mask row (C <= 512 at P <= 4096), else 32
    const int NT = flow_lds_bytes(2, a.h, a.w, a.C) <= budget ? 2 : 1;
    const size_t lds = flow_lds_bytes(NT, a.h, a.w, a.C);
    if (lds > budget) throw ArgError("flow: feature width / position count exceed the LDS budget");
    arg_checked([&] { launch_flow(a, NT, lds, (unsigned)(flow_ppad(a.P) / (32 * NT) * NB), ctx.stream); });
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
inline const void* const* vlist(const float* const* p) { return reinterpret_cast<const void* const*>(p); }
inline const void* const* vlist(const uint8_t* const* p) { return reinterpret_cast<const void* const*>(p); }

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
void launch_patch_warp(const float* const* src_img, const float* div, const float* flow, float* out, int K, int B, int H, int W, int hh, int ww,
                       hipStream_t st) {
    PatchWarpArgs pa{};
    for (int s = 0; s < K; ++s) { pa.src[s] = src_img[s]; pa.div[s] = div[s]; }
    pa.flow = flow; pa.out = out; pa.K = K; pa.B = B; pa.H = H; pa.W = W; pa.h = hh; pa.w = ww; pa.down = H / hh;
    hipLaunchKernelGGL(patch_warp_kernel, dim3(ew_grid((size_t)K * B * H * W)), dim3(256), 0, st, pa);
    check_launch("patch_warp");
}

// everything after the patch warp: x (K*B,3,H*W) re-normalised in place to the statistics of tar_img (B,3,H,W) raw, the composite when
// fore_x1 > fore_x0, losses[0] = loss_warp; pg / sg (B*P, C) or both null (the pose form: no cosine launch, losses[1] = 0)
void launch_train_tail(float* x, const float* tar_img, const float* pg, const float* sg, int K, int B, int H, int W, int P, int C,
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

}  // namespace
