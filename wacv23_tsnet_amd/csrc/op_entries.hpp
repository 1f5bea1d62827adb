// op_entries.hpp -- the C entry points that run ONE operator of the forward on the caller's tensors (include/tsnet_abi.h, tsnet_op_*), the
// convolution benchmark and the process-wide helpers (launch counters, the tools-build knobs, the constant tables): the launch helpers of
// launch.hpp on allocations of their own, none of it touching tsnet_engine.  engine.cpp includes this file once, after its own entries: it is
// part of that translation unit and of no other.  HOST code.
#pragma once
#ifndef TSNET_ENGINE_CPP
#error "op_entries.hpp is a part of engine.cpp: include it from there only"
#endif
#include "launch.hpp"

namespace {
// the operand kinds tsnet_op_conv2d and tsnet_op_conv2d_epi take
void op_check_nprod(int nprod) {
    if (nprod != 1 && nprod != 3 && nprod != 4 && nprod != TSNET_NPROD_F16) throw ArgError("conv2d op: nprod must be 1 (bf16 operands), 16 (fp16 operands: one fp16 plane), 3 or 4 products");
}
// the fields every convolution operator fills from its arguments
ConvCall op_conv_call(const float* x, const float* alpha, const float* beta, int relu, float bound, int N, int H, int W, float* y, int nprod) {
    ConvCall c; c.x = x; c.alpha = alpha; c.beta = beta; c.relu = relu; c.bound = bound; c.N = N; c.H = H; c.W = W; c.y = y; c.nprod = nprod;
    return c;
}
}  // namespace

extern "C" {

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
        const bool f16 = nprod == TSNET_NPROD_F16;
        const int planes = (nprod == 1 || f16) ? 1 : 2;
        const WeightScale ws = weight_scale(hw, nprod != 1);
        wd = mem.alloc<float>(wn * sizeof(float));
        wq = mem.alloc<unsigned short>((size_t)L.kpad * L.npad * 2 * planes);
        un = mem.alloc<float>(sizeof(float));
        HIP_TRY(hipMemcpy(wd, hw.data(), wn * sizeof(float), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(un, &ws.unscale, sizeof(float), hipMemcpyHostToDevice));
        pack_layer(wd, L, wq, f16 ? -1 : planes, ws.scale, s);
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
    op_check_nprod(nprod);
    hipStream_t s = (hipStream_t)stream;
    Ctx ctx(s, current_device_cus());
    const ConvRequest req = arg_checked([&] { return decode_tile_code(kernel, tile); });
    OpLayer op(w_oihw, bias, Cin, Cout, ksize, stride, pad, pad_mode, nprod, s, kernel == 3 ? 1 : 0);     // kernel 3: Winograd-along-x form (conv_w1.hpp)
    run_conv(ctx, op.L, op_conv_call(x, in_alpha, in_beta, in_relu, bound, N, H, W, y, nprod), req);
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
    op_check_nprod(nprod);
    const tsnet_conv_epi& e = *epi;
    if (e.stats < 0 || e.stats > 2) throw ArgError("conv2d_epi op: stats must be 0 (none), 1 (partials + finalize launch) or 2 (arrival counters offered)");
    if (e.repeat < 1) throw ArgError("conv2d_epi op: repeat must be at least 1");
    if (e.stats && (!e.part || !e.alpha || !e.beta)) throw ArgError("conv2d_epi op: statistics need part, alpha and beta");
    if (e.stats == 2 && !e.counters) throw ArgError("conv2d_epi op: stats = 2 needs the arrival counters");
    if (e.addend && (e.add_nmod < 1 || N % e.add_nmod)) throw ArgError("conv2d_epi op: add_nmod must divide N");
    if ((e.x_bf16 || e.y_bf16) && nprod != 1) throw ArgError("conv: bf16 storage goes with bf16 operands");
    hipStream_t s = (hipStream_t)stream;
    Ctx ctx(s, current_device_cus());
    const ConvRequest req = arg_checked([&] { return decode_tile_code(kernel, tile); });
    OpLayer op(w_oihw, bias, Cin, Cout, ksize, stride, pad, pad_mode, nprod, s, kernel == 3 ? 1 : 0);
    ConvCall c = op_conv_call(x, in_alpha, in_beta, in_relu, bound, N, H, W, y, nprod);
    c.addend = e.addend; c.add_nmod = e.addend ? e.add_nmod : 1;
    c.amax_out = e.amax_out; c.in_amax = e.in_amax; c.bound_add = e.bound_add; c.x_bf16 = e.x_bf16; c.y_bf16 = e.y_bf16;
    if (e.stats) {                                      // tsnet_engine::conv_stats' request; stats = 1 withholds the counters
        c.stat_part = e.part; c.fin_alpha = e.alpha; c.fin_beta = e.beta; c.fin_counter = e.stats == 2 ? e.counters : nullptr;
    }
    if (in_alpha && !in_beta) throw ArgError("conv: alpha without beta");
    const ConvShape sh = conv_shape(op.L, c);
    const ConvPlan p = arg_checked([&] { return plan_conv(sh, req, ctx.cus); });
    const size_t part_n = stat_part_doubles((size_t)N, (size_t)p.tpi, (size_t)Cout);
    if (e.stats && (e.part_capacity < 0 || part_n > (size_t)e.part_capacity))
        throw ArgError("conv2d_epi op: part holds " + std::to_string(e.part_capacity) + " doubles, the plan writes N * tpi * Cout * 2 = " + std::to_string(part_n));
    if (e.stats == 2 && (size_t)N * ((op.L.npad + 31) / 32) > kFinCounterInts)
        throw ArgError("conv2d_epi op: more (image, 32-channel group) pairs than arrival counters");
    const int hw = sh.ho() * sh.wo();
    for (int it = 0; it < e.repeat; ++it) {
        // every partial a NaN before each launch: an entry folded before its store is visible, or never written, shows in alpha / beta
        if (e.stats) HIP_TRY(hipMemsetAsync(e.part, 0xFF, part_n * sizeof(double), s));
        if (e.amax_out) HIP_TRY(hipMemsetAsync(e.amax_out, 0, (size_t)N * sizeof(unsigned), s));
        run_conv(ctx, op.L, c, req);
        if (c.stat_S > 0) {                             // not finalised in the kernel: conv_stats' launch
            launch_finalize2(e.part, e.alpha, e.beta, N, Cout, c.stat_S, hw, s);
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
    const ConvRequest req = arg_checked([&] { return decode_tile_code(0, tile); });
    OpLayer op(w_oihw, bias, Cin, Cout, ksize, stride, pad, pad_mode, nprod, s);
    // both routes answer to the fused form's plan: what it refuses is refused before anything is launched
    ConvCall c = op_conv_call(x, in_alpha, in_beta, in_alpha ? in_relu : 0, bound, N, 2 * H, 2 * W, y, nprod);
    c.up2 = true;
    arg_checked([&] { (void)plan_conv(conv_shape(op.L, c), req, ctx.cus); });
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
    ConvCall c = op_conv_call(x, nullptr, nullptr, 0, bound, N, H, W, y, nprod);
    c.x2 = x2; c.csplit = C1; c.x2_nmod = x2_nmod;
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
    const HeadRequest hr = arg_checked([&] { return decode_head_code(composite); });
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
        const WeightScale ws = weight_scale(hw, true);
        wq = mem.alloc<unsigned short>(head_mfma_table_halves(C) * sizeof(unsigned short));
        un = mem.alloc<float>(sizeof(float));
        HIP_TRY(hipMemcpy(un, &ws.unscale, sizeof(float), hipMemcpyHostToDevice));
        pack_head_mfma(wd, C, ws.scale, wq, s);
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
    double* part = mem.alloc<double>(stat_scratch_doubles(N, C) * sizeof(double));
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

// tsnet_op_upsample2x (fp32 tensors; returns with the launch enqueued) and tsnet_op_upsample2x_st (either storage; returns after the stream has drained)
static void op_upsample_any(const float* x, const float* alpha, const float* beta, int relu, int N, int H, int W, int C, int x_bf16, int y_bf16,
                            float* y, void* stream, bool drain) {
    if (!x || !y) throw ArgError("upsample op: null tensor");
    if (alpha && !beta) throw ArgError("upsample op: alpha without beta");
    if (C < 4 || (C & 3)) throw ArgError("upsample op: C must be a multiple of 4");
    if (N < 1 || H < 1 || W < 1) throw ArgError("upsample op: bad shape (N, H, W >= 1)");
    Ctx ctx((hipStream_t)stream, current_device_cus());
    run_upsample(ctx, x, alpha, beta, relu, N, H, W, C, y, x_bf16 != 0, y_bf16 != 0);
    if (drain) HIP_TRY(hipStreamSynchronize(ctx.stream));
}

int tsnet_op_upsample2x(const float* x, const float* alpha, const float* beta, int relu, int N, int H, int W, int C, float* y, void* stream) {
    OP_BEGIN
    op_upsample_any(x, alpha, beta, relu, N, H, W, C, 0, 0, y, stream, false);
    OP_END
}

int tsnet_op_upsample2x_st(const float* x, const float* alpha, const float* beta, int relu, int N, int H, int W, int C, int x_bf16, int y_bf16,
                           float* y, void* stream) {
    OP_BEGIN
    op_upsample_any(x, alpha, beta, relu, N, H, W, C, x_bf16, y_bf16, y, stream, true);
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
    run_flow(ctx, fa, NB, dslot, variant);
    const float ms = timed_repeats(ctx.stream, repeat - 1, [&](int) { run_flow(ctx, fa, NB, dslot, variant); });
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    if (ms_out) *ms_out = ms;
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

// every spelling of the warp: tsnet_op_warp (K = 1) and tsnet_op_warp_k (ext = B: the identity), tsnet_op_warp_k_shared (ext = its SB) and
// tsnet_op_warp_k_slots (ext < 0: the caller's table).  repeat > 1 re-launches the kernel ALONE between two events, the table uploaded once
// and the first launch outside them (tools/warp_bench.py); *ms_out = the mean of those launches, 0 without them.
static void op_warp_any(const float* src_fea, const float* flow, int B, int K, int ext, const int* slots, int n_src, int h, int w, int C, float* out,
                        void* stream, int repeat = 1, float* ms_out = nullptr) {
    if (!src_fea || !flow || !out) throw ArgError("warp op: null tensor");
    if (C < 4 || (C & 3)) throw ArgError("warp op: C must be a multiple of 4");
    if (B < 1 || K < 1 || K > TSNET_MAX_SOURCES || h < 1 || w < 1) throw ArgError("warp op: bad shape (1 <= K <= 8 sources, B, h, w >= 1)");
    if (ext >= 0 && (ext < 1 || B % ext)) throw ArgError("warp op: the source-batch extent must divide the batch");
    Ctx ctx((hipStream_t)stream, current_device_cus());
    if (ms_out) *ms_out = 0.f;
    DevBufs mem;
    const int* d = ext >= 0 ? op_table_ext(mem, B, K, ext) : op_slot_table(mem, "warp op", slots, K * B, n_src);
    run_warp(ctx, src_fea, d, flow, out, B, K, h, w, C);
    const float ms = timed_repeats(ctx.stream, repeat - 1, [&](int) { run_warp(ctx, src_fea, d, flow, out, B, K, h, w, C); });
    if (ms_out) *ms_out = ms;
    HIP_TRY(hipStreamSynchronize(ctx.stream));
}

int tsnet_op_warp(const float* src_fea, const float* flow, int B, int h, int w, int C, float* out, void* stream) {
    OP_BEGIN
    op_warp_any(src_fea, flow, B, 1, B, nullptr, 0, h, w, C, out, stream);
    OP_END
}

int tsnet_op_warp_k(const float* src_fea, const float* flow, int B, int K, int h, int w, int C, float* out, int repeat, float* ms_out, void* stream) {
    OP_BEGIN
    op_warp_any(src_fea, flow, B, K, B, nullptr, 0, h, w, C, out, stream, repeat, ms_out);
    OP_END
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
    double* part = mem.alloc<double>(stat_scratch_doubles(N, C) * sizeof(double));
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

int tsnet_bench_conv(int N, int H, int W, int Cin, int Cout, int ksize, int stride, int pad, int pad_mode, int norm,
                     int variant, int iters, float* ms_out, void* stream) {
    OP_BEGIN
    if (iters < 1 || !ms_out) throw ArgError("bench_conv: bad argument");
    hipStream_t s = (hipStream_t)stream;
    Ctx ctx(s, current_device_cus());
    // variant (-1 = the layer's own kernel and tile): conv_plan.hpp decode_bench_variant
    const BenchVariant bv = arg_checked([&] { return decode_bench_variant(variant); });
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
        ConvCall c = op_conv_call(x, nullptr, nullptr, 0, 1.f, N, H, W, y, nprod);
        if (norm & 1) { c.alpha = al; c.beta = be; c.relu = 1; c.bound = 64.f; }
        if (norm & 2) {                                              // with the InstanceNorm statistics of the output, as the forward's layers run
            const size_t tpi = ((size_t)Ho * Wo + 63) / 64;
            c.stat_part = mem.alloc<double>(stat_part_doubles(N, tpi, Cout) * sizeof(double));
            c.fin_alpha = mem.alloc<float>((size_t)N * Cout * 4); c.fin_beta = mem.alloc<float>((size_t)N * Cout * 4);
            c.fin_counter = mem.alloc<int>(kFinCounterInts * sizeof(int));
            HIP_TRY(hipMemset(c.fin_counter, 0, kFinCounterInts * sizeof(int)));
        }
        for (int i = 0; i < 2; ++i) run_conv(ctx, op.L, c, bv.req);
        *ms_out = timed_repeats(s, iters, [&](int i) { run_conv(ctx, cold.empty() ? op.L : cold[(size_t)i % cold.size()]->L, c, bv.req); });
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
