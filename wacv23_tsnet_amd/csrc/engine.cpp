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
//
// The unit follows its seams: launch.hpp (how kernels are launched, and the types that go with it), this file (tsnet_engine, the forward, the
// entries that take a handle, the training extras), op_entries.hpp (the single-operator entries) and clip_entries.hpp (the clip side).
#define TSNET_ENGINE_CPP      // launch.hpp, op_entries.hpp and clip_entries.hpp refuse every other includer
#include <map>

#include "launch.hpp"

namespace { std::string g_create_error; }

// What the source-side slots hold, or what a forward ran on: nothing, the K sources of a batch of B (source s of frame b in slot s*B + b), ONE
// source set for every driving frame (source s in slot s), or a bank of slots the caller put.  The rules of the modes are read off the kind.
struct SrcState {
    enum Kind { None, PerBatch, Shared, Bank } kind = None;
    int B = 0;                            // PerBatch: the batch the sources were set at
};

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

    // device memory.  `mem` owns every allocation of the handle, the holders below its stream and events: the destructor releases them, and
    // release() a finalize that did not complete.  The pointers are views into what `mem` owns.
    DevBufs mem;
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
    OwnedStream side_stream;           // target-label chain of a full forward runs here, concurrently with the source encoder
    OwnedEvent ev_fork, ev_join, ev_fork2, ev_join2;
    OwnedEvent ev_done;                // recorded behind the last launch of a forward on the caller's stream
    float* train_ws = nullptr;         // workspace of tsnet_train_extras, allocated on first use
    void release() {                   // a finalize that threw: the handle owns nothing of that attempt.  The other views into `mem` (the arena
                                       // members, the layers' wq / bias) dangle until the next finalize sets them: every reader asks `finalized` first
        mem.release(); side_stream.reset(); wpack = arena = nullptr; wpack_floats = arena_floats = 0;
        for (OwnedEvent* e : {&ev_fork, &ev_join, &ev_fork2, &ev_join2, &ev_done}) e->reset();
    }

    // The encoded sources: ONE scheme.  The source-side tensors are K * Bmax SLOTS of one source each -- slot j is image j of X / shat / F1s
    // and mask j of bbox_copy, all dense -- and every forward names, in a table, the slot that each (source s, driving frame b) pair reads:
    // entry s*B + b (use_table; the kernels read nothing else to find a source).  Whatever is indexed by the pair itself -- flows, F1, F2 and
    // their InstanceNorm pairs -- stays at n = s*B + b.  The modes differ in who fills the slots and who writes the table:
    //   per-batch cache (tsnet_set_sources at batch B, the one-shot forward)   source s of frame b in slot s*B + b    table: the identity
    //   shared cache (tsnet_set_sources_shared)                               source s in slot s                     table: s for every b
    //   bank (tsnet_bank_put / tsnet_forward_bank)                            the slots the caller puts              table: the caller's
    // They write the same buffers: whichever was written last is the one that can be read.
    SrcState cached;                // what the slots hold now (None while they are being written)
    SrcState last;                  // what the last forward ran on: "src_fea"'s image count, tsnet_train_extras' refusals
    std::vector<char> bank_filled;  // per slot: put since the bank was started
    float* bbox_copy = nullptr;     // (K * Bmax, H, W) device copies of the source bboxes, one per slot
    int* slot_tab = nullptr;        // device (arena): K * Bmax ints, the table of the forward being enqueued (written by slot_fill_kernel)
    std::vector<int> slot_tab_host; // what slot_tab holds once everything enqueued so far has run: a forward with the same table skips the fill
    float* tbox = nullptr;          // (Bmax, H, W): the driving frames' masks widened from a compact call (wide calls pass their own tensor on)
    int last_B = 0;                 // its batch of driving frames
    // images of X after a forward on `s`: K * B, K on a shared source set, every slot on a bank
    size_t src_images(const SrcState& s) const { return (size_t)K * (s.kind == SrcState::Bank ? Bmax : s.kind == SrcState::Shared ? 1 : s.B); }
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
        launch_finalize2(pt, alpha, beta, N, L.cout, c.stat_S, HW, ctx.stream);
        check_launch("in_finalize2");
    }
    void encode(Ctx& ctx, std::vector<ConvLayer>& L, const float* xin, const unsigned* xin_amax, int N, std::vector<float*>& raw, float* out_fea, int nblocks);
    // ResnetBlock.  stream_amax == null: the residual stream Xs has the a-priori bound stream_bound (encoder: (blocks+1) sqrt(HW));
    // else its bound is measured: max |first value| published by the producer + amax_add (decoder: the stream starts at a raw conv output)
    void resblock(Ctx& ctx, const ConvLayer& c1, const ConvLayer& c2, float* Xs, float stream_bound, const unsigned* stream_amax, float amax_add,
                  float* y1, float* y2, int N, int hh, int ww);
    void source_chain(Ctx& ctx, int first, int n);
    void set_sources(Ctx& ctx, const SrcIn& in, int B, SrcState::Kind kind, hipStream_t bbox_stream = nullptr);
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
    wpack = mem.alloc<float>(wpack_floats * sizeof(float));
    HIP_TRY(hipMemsetAsync(wpack, 0, wpack_floats * sizeof(float), s));
    size_t max_w = 0;
    for (ConvLayer* L : all_layers) max_w = std::max(max_w, (size_t)L->cout * L->cin_total * L->ks * (L->form == 1 ? 4 : L->ks));
    max_w = std::max(max_w, (size_t)3 * cfg.ngf * 49);
    DevBufs staging;                       // the parameter being packed: freed when this function is left, however
    float* stage = staging.alloc<float>(max_w * sizeof(float));
    unsigned short* planes_base = reinterpret_cast<unsigned short*>(wpack + planes_off);
    for (size_t i = 0; i < all_layers.size(); ++i) {
        ConvLayer* L = all_layers[i];
        const Param& pw = params[pindex[L->wparam]];
        // the filter as the kernel consumes it: itself, or its Winograd transform along x (fp64 on the host, rounded once)
        std::vector<float> wino;
        if (L->form == 1) wino = winograd_x_filters(pw.host);
        const std::vector<float>& wsrc = L->form == 1 ? wino : pw.host;
        const WeightScale ws = weight_scale(wsrc, np != 1 || f16, &L->wparam);      // per layer; the bf16 modes take the weights as they are
        HIP_TRY(hipMemcpyAsync(stage, wsrc.data(), wsrc.size() * sizeof(float), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(wpack + tab_off + i, &ws.unscale, sizeof(float), hipMemcpyHostToDevice, s));
        pack_layer(stage, *L, planes_base + L->w_off, f16 ? -1 : planes, ws.scale, s);
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
            const WeightScale ws = weight_scale(pw.host, true, &dec_head.wparam);
            const size_t slot = tab_off + all_layers.size();
            HIP_TRY(hipMemcpyAsync(wpack + slot, &ws.unscale, sizeof(float), hipMemcpyHostToDevice, s));
            head_wq = reinterpret_cast<unsigned short*>(wpack + head_planes_off);
            head_wq_unscale = wpack + slot;
            pack_head_mfma(stage, cfg.ngf, ws.scale, head_wq, s);
            check_launch("pack_head_mfma");
        }
        HIP_TRY(hipStreamSynchronize(s));
    }
    staging.release();

    // ---- constant tables
    const int H = cfg.height, W = cfg.width;
    {
        std::vector<float> t((size_t)H * W * 3), gx(w), gy(h);
        coord_table(H, W, t.data());
        linspace_pm1(w, gx.data());
        linspace_pm1(h, gy.data());
        d_coords = mem.alloc<float>(t.size() * sizeof(float));
        d_gx = mem.alloc<float>(w * sizeof(float));
        d_gy = mem.alloc<float>(h * sizeof(float));
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
    // InstanceNorm partials (doubles = 2 floats each): the stand-alone pass (2 C channels at most), a conv epilogue N * tiles-per-image *
    // Cout * 2 with tiles of at least 64 positions (ceil for ragged images), per lane
    size_t part_doubles = stat_scratch_doubles(NB, 2 * C);
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
    arena = mem.alloc<float>(total * sizeof(float));
    size_t o = 0;
    for (auto& r : req) { *r.first = arena + o; o += r.second; }
    part = reinterpret_cast<double*>(part_f);
    part_side = reinterpret_cast<double*>(part_side_f);
    slot_tab = reinterpret_cast<int*>(slot_f);
    bank_filled.assign(NB, 0);
    amax = mem.alloc<unsigned>((size_t)(K + 3) * Bmax * sizeof(unsigned));
    HIP_TRY(hipMemsetAsync(amax, 0, (size_t)(K + 3) * Bmax * sizeof(unsigned), s));
    // arrival counters: one per (image, 32-channel group) of a launch; launches with more (image, group) pairs than kFinCounterInts
    // fall back to the in_finalize2 kernel (plan_conv checks the index range against this size)
    fin_counter = mem.alloc<int>((2 * kFinCounterInts + 256) * sizeof(int));
    HIP_TRY(hipMemsetAsync(fin_counter, 0, (2 * kFinCounterInts + 256) * sizeof(int), s));
    fin_counter_side = fin_counter + kFinCounterInts;
    flow_cnt = fin_counter + 2 * kFinCounterInts;
    // side lane (tsnet_forward): own statistics scratch, counters, (alpha, beta) pairs (above), stream and events
    HIP_TRY(hipStreamCreateWithFlags(&side_stream.v, hipStreamNonBlocking));
    for (OwnedEvent* e : {&ev_fork, &ev_join, &ev_fork2, &ev_join2, &ev_done}) HIP_TRY(hipEventCreateWithFlags(&e->v, hipEventDisableTiming));
    for (auto& p : params) { std::vector<float>().swap(p.host); }   // host copies no longer needed (kept until nothing above can fail: a retry packs them again)
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

// The source chain: encoder -> the flow kernel's operand planes -> the per-source half of FuseNet's first convolution (conv(cat(src, tar)) =
// conv_src(src) + conv_tar(tar), TSNet.py:195-197: it depends on the sources only, so a driving frame of a clip does not pay for it, SURVEY.md
// 8-f rank 1), on the n packed images of x_img, into slots first .. first + n - 1.  raw_img, the ResnetBlock scratch and the first n source
// maxima are staging; the other slots are not touched.
void tsnet_engine::source_chain(Ctx& ctx, int first, int n) {
    float* fea = X + (size_t)first * P * C;
    encode(ctx, img_enc, x_img, amax_src(), n, raw_img, fea, cfg.enc_blocks);
    run_l2norm_split(ctx, fea, reinterpret_cast<unsigned short*>(shat) + (size_t)first * flow_plane_halves(1, P, C), n, P, C);
    ConvCall a; a.x = fea; a.bound = enc_bound(); a.N = n; a.H = h; a.W = w; a.y = F1s + (size_t)first * P * C * 2;
    conv(ctx, fuse_c1_src, a);
}

// kind: PerBatch or Shared (B = 1), what the slots hold once everything here is enqueued; until then they hold nothing a forward may read.
// bbox_stream: where the K bounding-box copies of the clip cache are enqueued.  Their only reader is the flow kernel; the one-shot forward
// passes its side stream (the flow kernel's own lane: the copies are ordered ahead of it there and cost the caller's lane nothing --
// three 4.7 us copy kernels + their boundaries sat in front of the stem until round 5); null = the caller's stream (clip mode).
// Compact sources: the packing kernel widens the masks into bbox_copy itself, on the caller's lane (ordered ahead of the flow kernel by the join).
// Source s of frame b goes to slot s*B + b of every source-side tensor, the masks included.
void tsnet_engine::set_sources(Ctx& ctx, const SrcIn& in, int B, SrcState::Kind kind, hipStream_t bbox_stream) {
    const int H = cfg.height, W = cfg.width;
    cached = {};
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
    source_chain(ctx, 0, K * B);
    cached = {kind, B};
}

// `count` sources of batch 1 -> slots first .. first + count - 1 of the bank: the source chain on count images, its outputs at the slot offset
void tsnet_engine::bank_put(Ctx& ctx, int first, int count, const SrcIn& in, const float* div) {
    const int H = cfg.height, W = cfg.width;
    if (cached.kind != SrcState::Bank) { std::fill(bank_filled.begin(), bank_filled.end(), 0); cached = {SrcState::Bank, 0}; }
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
    source_chain(ctx, first, count);
    for (int i = 0; i < count; ++i) bank_filled[first + i] = 1;
}

// Everything that depends on the driving frame only: label encoder, its L2-normalised features and the target half of
// FuseNet's first convolution.  Independent of the source encoder, so a full forward runs it on the side stream.
void tsnet_engine::target_chain(Ctx& ctx, const TarIn& tar, int B) {
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
        for (int b = 0; b < B; ++b) t[s * B + b] = bank_slots ? bank_slots[s * B + b] : cached.kind == SrcState::Shared ? s : s * B + b;
    if (t.size() <= slot_tab_host.size() && std::equal(t.begin(), t.end(), slot_tab_host.begin())) return;
    slot_tab_host.clear();                                  // (a launch that throws leaves no claim behind)
    run_slot_fill(ctx.stream, slot_tab, t.data(), (int)t.size());
    slot_tab_host = std::move(t);
}

// Kc sources per driving frame; bank_slots (host, entry s*B + b): the table of a forward on the source bank, null on the caches
void tsnet_engine::forward_rest(Ctx& ctx, const TarIn& tar, float* out_rgb, float* out_flow, int B, int Kc, const int* bank_slots) {
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
    last_B = B; last = cached;
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
    try { h->alloc_all((hipStream_t)stream); } catch (...) { h->release(); throw; }
    h->cus = current_device_cus();                  // the engine's device: its allocations live there
    h->finalized = true;
    API_END(h)
}

void tsnet_destroy(tsnet_handle h) { delete h; }

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
    h->cached = {};                                 // cached source features were encoded with the previous divisors
    API_END(h)
}

// The forward entry points take their inputs in either form (SrcIn / TarIn): the wide entries and their _u8 siblings differ in the descriptor only.
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

static void check_source_list(tsnet_handle h, const SrcIn& in) {
    if (!in.img || !in.lbl || !in.bbox) throw ArgError("null source list");
    for (int s = 0; s < h->K; ++s)
        if (!in.img[s] || !in.lbl[s] || !in.bbox[s]) throw ArgError("null source tensor (need n_source entries)");
}

static int set_sources_any(tsnet_handle h, const SrcIn& in, int B, bool shared, void* stream) {
    API_BEGIN(h)
    check_forward_args(h, B);
    check_source_list(h, in);
    if (in.u8) check_compact(h, &in);
    Ctx ctx((hipStream_t)stream, h->cus, h->timing.on ? &h->timing : nullptr);
    h->set_sources(ctx, in, B, shared ? SrcState::Shared : SrcState::PerBatch);     // shared: K images, source-batch extent 1
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
    if (h->cached.kind != SrcState::Shared && !(h->cached.kind == SrcState::PerBatch && h->cached.B == B)) throw ArgError("forward_target: batch differs from the cached sources (call tsnet_set_sources first)");
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
    if (h->cached.kind != SrcState::Bank) throw ArgError("forward_bank: no source bank (call tsnet_bank_put first)");
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
        check_source_list(h, in);               // (after the fork, as ever: the join below covers a refusal)
        if (in.u8 || tar.u8) check_compact(h, &in);
        h->target_chain(cs, tar, B);
        Ctx cm(main, h->cus);
        h->set_sources(cm, in, B, SrcState::PerBatch, h->side_stream);      // (the bounding-box copies ride the side lane, ahead of the flow kernel)
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


int tsnet_train_extras(tsnet_handle h, const float* const* src_img, const float* tar_img, int B,
                       float* warp_src_img, float* losses, void* stream) {
    API_BEGIN(h)
    check_forward_args(h, B);
    if (h->last_B != B) throw ArgError("train_extras: call tsnet_forward with the same batch first (uses its flows and features)");
    if (h->last.kind == SrcState::Shared) throw ArgError("train_extras: the last forward ran on a shared source set (tsnet_set_sources_shared); src_img is per batch element here");
    if (h->last.kind == SrcState::Bank) throw ArgError("train_extras: the last forward ran on a source bank (tsnet_forward_bank); src_img is per batch element here");
    if (!src_img || !tar_img || !warp_src_img || !losses) throw ArgError("train_extras: null tensor");
    const int K = h->K, H = h->cfg.height, W = h->cfg.width, hh = h->h, ww = h->w, P = h->P, C = h->C;
    for (int s = 0; s < K; ++s) if (!src_img[s]) throw ArgError("train_extras: null source image (need n_source entries)");
    if (H % hh || W % ww || H / hh != W / ww) throw ArgError("train_extras: image size must be a multiple of the feature size");
    hipStream_t st = (hipStream_t)stream;
    const int N = K * B;
    // workspace: gen mean/std (2*N*3) + ref mean/std (2*B*3) floats, then doubles: l1 partials (N*3*chunks) + cos partials
    const size_t nf = (size_t)2 * h->K * h->Bmax * 3 + 2 * h->Bmax * 3, nfp = (nf + 3) / 4 * 4;
    const size_t nd = (size_t)h->K * h->Bmax * 3 * kTrainChunks + kTrainNcos;
    if (!h->train_ws) h->train_ws = h->mem.alloc<float>(nfp * sizeof(float) + nd * sizeof(double));
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
    if (n == "src_fea") { p = h->X; c = h->src_images(h->last) * fe; }
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

}  // extern "C"

#include "op_entries.hpp"
#include "clip_entries.hpp"
