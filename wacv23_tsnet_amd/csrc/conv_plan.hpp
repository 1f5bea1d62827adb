// conv_plan.hpp -- which kernel, tile and schedule a convolution launch runs on.  Plain C++17: no HIP, no device code, so that every launch
// choice can be checked on the CPU (tests/test_conv_plan.py).  The planner VALIDATES AND CHOOSES: plan_conv refuses (std::invalid_argument)
// every layer geometry the kernels cannot index (validate_conv) and every request whose kernel the product build does not instantiate, so
// a ConvPlan always names a kernel that exists.  run_conv (launch.hpp, part of engine.cpp's unit) checks what depends on pointers, asks plan_conv, fills ConvArgs from
// the plan and hands both to the family's launcher (kernels.hpp), which only dispatches: no launcher repeats a rule written here.
//
// The promise these rules keep: the kernel family and the tile rows (and with them the statistics tiling) depend on the layer and the frame
// size only -- never on the batch (the patch kernels sum K slab-major, the general one tap-major; a tile's rows decide how the statistics
// partials group).  What DOES follow the batch runs the same chains per output element in every form, so a frame's result is the same bits
// alone (B = 1) and in any batch: conv_w1's tiles per workgroup, the stride-2 tile's deep schedule, the RGB head's tile rows, and the
// width / wave grid of a one-group tile of conv_h2 or conv_h2r (wide_pays and the bf16 rule count tiles per CU).  The CU count only enters
// these heuristics (how many tiles fill the chip in whole rounds), never a kernel's block -> tile map, so it is bit-neutral as well.
#pragma once
#include <cstddef>
#include <stdexcept>
#include <string>

namespace tsnet {

constexpr int kPlanTileRows = 4, kPlanTileCols = 32;   // the patch tile: conv_common.hpp kPatchRows x kPatchCols output pixels
constexpr size_t kFinCounterInts = 65536;   // size of the arrival-counter arrays of the in-kernel statistics finalize
constexpr int kFinMaxTiles = 32;            // most tiles per image the last-arriving workgroup folds itself (conv_epilogue); above: in_finalize2

enum class ConvFamily { H2R, G64, H2, H2S, H2S32, H2D, W1 };   // conv_h2r.hpp (general), conv_g64.hpp, conv_h2.hpp's three, conv_h2s32.hpp, conv_w1.hpp
enum class ConvKernel { Own = 0, General = 1, Patch = 2 };
enum class ConvSched { Plain = 0, Deep = 1, TwoGroups = 2 };

// the layer and the call, as far as a launch choice may look at them
struct ConvShape {
    int ks = 1, stride = 1, pad = 0, reflect = 0;
    int cin = 0;                 // padded input channels: 8 or a multiple of 16
    int cout = 0, npad = 0, kpad = 0;
    int form = 0;                // 1: packed in the Winograd-along-x form (conv_w1.hpp)
    int N = 0, H = 0, W = 0;
    int csplit = 0;              // > 0: channels >= csplit come from a second tensor (concat on load)
    int x2_nmod = 1;             // images of that second tensor (image n reads its image n % x2_nmod)
    bool transform = false;      // the producer's InstanceNorm (+ ReLU) applied while the operand is staged
    int nprod = 3;               // 1 = one operand plane, 3 or 4 fp16 x 2 products
    bool f16 = false;            // nprod = 1: the plane holds fp16 of the scaled operand (fp16-operand mode) instead of bf16.  Every rule keyed on
                                 // nprod == 1 counts MFMA work per staged byte and holds for both kinds: an fp16 layer runs its bf16 twin's plan
    bool fin_counter = false;    // output statistics with arrival counters supplied: the in-kernel finalize is possible
    bool up2 = false;            // the input tensor is the HALF-resolution map (N, H/2, W/2, cin): the kernel forms its bilinear x2 upsample while it
                                 // stages the patch (conv_h2.hpp UP2); H and W stay the extent the convolution sees
    bool x_bf16 = false;         // bf16 storage: the input tensor holds bf16 (conv_common.hpp load_x_octet).  Built into conv_h2's 3 x 3 kernels
                                 // (stride 1 and 2), conv_h2r and conv_g64; the Winograd form and the 7 x 7 stems load fp32 and nothing else
    int ho() const { return (H + 2 * pad - ks) / stride + 1; }
    int wo() const { return (W + 2 * pad - ks) / stride + 1; }
};

// an explicit choice (operator entry points, tsnet_bench_conv, tools); the forward runs the default
struct ConvRequest {
    ConvKernel kernel = ConvKernel::Own;
    int rows = 0;                // patch tile rows, 2 or 4; 0 = the planner's
    int width = 0;               // tile width 32 / 64 / 128 (conv_g64: its rows, 64 / 128); 0 = the planner's.  Every tile code sets it
    bool alt = false;            // the 3xxx codes: on a 3 x 3 / stride-1 patch layer the bf16 4 x 128 tile with its four waves side by side,
                                 // on the general kernel its 64-deep-step form (conv_g64)
    ConvSched sched = ConvSched::Plain;
    int chunk = 0;               // conv_w1 tiles per workgroup, 1..3; 0 = the planner's
    int chunk_cap = 3;           // largest chunk the planner may choose (the tools build's tsnet_tools_set key 0)
    int abl = 0, opt = 0;        // tools build: ablation / experiment masks (tsnet_bench_conv)
    int xcd_gn = -1;             // -1 = the planner's; 0 = consecutive tiles per XCD; 1, 2, 4, 8 = XCD grid columns over the N tiles
};

struct ConvPlan {
    ConvFamily family = ConvFamily::H2R;
    int rows = 0;                // patch families: output rows of a tile (x 32 columns); conv_g64 / conv_h2r: output positions of a tile
    int width = 0;               // output channels of a tile
    bool side_by_side = false;   // conv_h2 4 x 128: the four waves 1 x 4 instead of 2 x 2
    ConvSched sched = ConvSched::Plain;
    int w1_chunk = 1, w1_tab2 = 0;
    int xcd_gn = 0;
    int tpi = 0, tiles_m = 0, tiles_n = 0;
    bool fin = false;            // the statistics are finalised by the convolution's last-arriving workgroups
    bool up2 = false;            // conv_h2's fused-upsample form (ConvShape::up2)
};

// tsnet_op_conv2d's (kernel, tile) pair (include/tsnet_abi.h).  kernel 3 (the Winograd form) takes tile = tiles per workgroup.
inline ConvRequest decode_tile_code(int kernel, int tile) {
    ConvRequest r;
    if (kernel == 3) {
        if (tile < 0 || tile > 3) throw std::invalid_argument("conv: the Winograd form takes 0 to 3 tiles per workgroup");
        r.chunk = tile;
        return r;
    }
    if (kernel < 0 || kernel > 2) throw std::invalid_argument("conv: kernel must be 0 (the layer's own), 1 (general), 2 (patch) or 3 (Winograd form)");
    r.kernel = static_cast<ConvKernel>(kernel);
    switch (tile) {
        case 0: break;
        case 32: case 64: case 128: r.width = tile; break;
        case 2128: r.rows = 2; r.width = 128; break;
        case 3064: case 3128: r.alt = true; r.width = tile - 3000; break;
        case 12128: r.rows = 2; r.width = 128; r.sched = ConvSched::Deep; break;
        case 20032: case 20064: r.rows = 4; r.width = tile - 20000; r.sched = ConvSched::TwoGroups; break;
        default: throw std::invalid_argument("conv: unknown tile code " + std::to_string(tile));
    }
    return r;
}

// tsnet_bench_conv's variant bits: 0-11 tile code (with bit 15: tiles per workgroup), 12 general kernel, 13 bf16 operands, 14 patch kernel,
// 15 Winograd form, 16-20 ablation mask, 21 cold weights, 22 weights five steps ahead, 23 two K groups, 24-27 experiment mask, 28-30 XCD grid
struct BenchVariant { ConvRequest req; int nprod = 3, form = 0; bool cold = false; };
inline BenchVariant decode_bench_variant(int variant) {
    const int v = variant < 0 ? 0 : variant;
    BenchVariant b;
    b.form = (v & 32768) ? 1 : 0;
    b.req = decode_tile_code(b.form ? 3 : ((v & 4096) ? 1 : ((v & 16384) ? 2 : 0)), v & 4095);
    b.nprod = (v & 8192) ? 1 : 3;
    b.cold = (v & (1 << 21)) != 0;
    b.req.abl = (v >> 16) & 31;
    b.req.opt = ((v >> 24) & 15) | ((v & (1 << 23)) ? 16 : 0) | ((v & (1 << 22)) ? 32 : 0);
    // deep prefetch + two K groups and nothing else is no experiment: the product's two-group tiles (tile codes 20032 / 20064)
    if (!b.req.abl && b.req.opt == (8 | 16)) { b.req.sched = ConvSched::TwoGroups; b.req.opt = 0; }
    const int gx = (v >> 28) & 7;                  // 0 the planner's, 1 linear, 2..5 a grid with 1, 2, 4, 8 columns
    if (gx > 5) throw std::invalid_argument("bench_conv: XCD grid code 0 to 5");
    b.req.xcd_gn = gx == 0 ? -1 : (gx == 1 ? 0 : 1 << (gx - 2));
    return b;
}

// tsnet_op_head's `composite`: bit 0 the pose composite, bits 8.. the tile rows of head_conv3 to force (0 = the planner's)
struct HeadRequest { bool composite = false; int rows = 0; };
inline HeadRequest decode_head_code(int code) {
    if (code < 0 || (code & 0xFE)) throw std::invalid_argument("head: composite is bit 0, the tile rows bits 8 and up");
    HeadRequest r;
    r.composite = code & 1;
    r.rows = code >> 8;
    if (r.rows != 0 && r.rows != 8 && r.rows != 16 && r.rows != 32) throw std::invalid_argument("head: tile rows 8, 16 or 32");
    return r;
}

constexpr size_t w1_lds_bytes_host(int Cin, int tables) {       // conv_w1.hpp w1_lds_bytes for the two-plane stages
    return 3 * (size_t)(2 * (4 * 2 * 2 * (96 * 16 + 64) + 16)) + (size_t)tables * 2 * ((Cin + 31) / 32 * 32) * 4;
}
// a layer packed in the Winograd-along-x form runs conv_w1 and nothing else: 3 x 3 / stride 1 / pad 1 on frames of whole 4 x 32 tiles
inline bool w1_eligible(int ks, int stride, int pad, int cin, int H, int W) {
    // (the three V stages + the transform table of 2 Cin floats must fit the CU's 160 KiB beside the epilogue's 64 B of static LDS: 1216
    // channels at most, inside the two channels per thread that the prologue's table request covers -- conv_w1_launch.cpp asserts it)
    return ks == 3 && stride == 1 && pad == 1 && cin >= 16 && (cin & 15) == 0 && H >= 4 && W >= 32 && H % kPlanTileRows == 0 && W % kPlanTileCols == 0 &&
           w1_lds_bytes_host(cin, 1) + 256 <= 160 * 1024;
}

// What every convolution kernel assumes of a layer and a call: a refusal here comes before anything is launched.
inline void validate_conv(const ConvShape& s) {
    auto refuse = [](const char* why) { throw std::invalid_argument(why); };
    if (s.ks != 1 && s.ks != 3 && s.ks != 7) refuse("conv: kernel size must be 1, 3 or 7");
    if (s.cin != 8 && (s.cin < 16 || (s.cin & 15))) refuse("conv: input channels must be 8 or a multiple of 16 (pad with zeros)");
    if (s.stride < 1 || s.pad < 0) refuse("conv: the stride must be positive, the padding not negative");
    if (s.N < 1 || s.H < 1 || s.W < 1 || s.H + 2 * s.pad < s.ks || s.W + 2 * s.pad < s.ks || s.cout < 1) refuse("conv: empty tensor");
    if (s.reflect && (s.pad >= s.H || s.pad >= s.W)) refuse("conv: reflection pad needs pad < input size");
    if (s.csplit && ((s.csplit & 15) || s.csplit < 0 || s.csplit >= s.cin)) refuse("conv: channel split must be a multiple of 16 inside the channel range");
    const double px = (double)s.H * s.W * 4, c1 = s.csplit ? s.csplit : s.cin;
    if (s.N * px * c1 >= 2147483648.0 || s.x2_nmod * px * (s.cin - c1) >= 2147483648.0 || (double)s.N * s.ho() * s.wo() * s.cout >= 2147483647.0 ||
        (double)s.kpad * s.npad * 2 >= 2147483648.0)
        refuse("conv: tensor too large for 32-bit buffer offsets");
    if ((size_t)2 * s.cin * 4 > 32 * 1024) refuse("conv: too many input channels for the transform table");
}

// Kernel class of a layer at a frame size.  The patch kernels sum K slab-major, the general one tap-major: the class must depend on the
// layer and the geometry alone, never on the batch (a sample's result is the same bits in any batch, B = 1 included).
// eligible_only: what the layer CAN run on (an explicit request, op tests / tools); otherwise what the forward runs it on
inline ConvFamily conv_class(const ConvShape& s, int rows, bool eligible_only) {
    const int Ho = s.ho(), Wo = s.wo();
    const bool onep = s.nprod == 1;                  // one product: a bf16 plane or (s.f16) an fp16 plane
    const bool s1 = s.ks == 3 && s.stride == 1 && s.pad == 1 && s.cin >= 16 && (s.cin & 15) == 0 && s.H >= 2 && s.W >= 2;
    if (s.csplit || Ho <= 0 || Wo <= 0 || Wo % kPlanTileCols) return ConvFamily::H2R;
    const bool s2 = s.ks == 3 && s.stride == 2 && s.pad == 1 && !s.reflect && s.cin >= (eligible_only ? 16 : 128) && (s.cin & 15) == 0 && s.H == 2 * Ho && s.W == 2 * Wo;
    if (rows == 2 && Ho % 2 == 0) {                              // a 2-row tile (requested explicitly, or the stride-2 layers' own choice)
        if (s1) return ConvFamily::H2;
        if (s2) return ConvFamily::H2D;
    }
    if (Ho % kPlanTileRows) return ConvFamily::H2R;
    if (s1) return ConvFamily::H2;
    if (s.ks == 7 && s.stride == 1 && s.pad == 3 && s.reflect && s.cin == 8 && !s.transform && s.H >= 4 && s.W >= 4) return ConvFamily::H2S;
    // the pose model's stems (31 / 28 channels padded to 32): their own patch kernel since round 6 (653 + 231 us on the general kernel at configs[3])
    if (s.ks == 7 && s.stride == 1 && s.pad == 3 && s.reflect && s.cin == 32 && !s.transform && s.H >= 4 && s.W >= 4) return ConvFamily::H2S32;
    // stride 2: the patch kernel from 128 input channels on (117 / 125 us on the 128 -> 256 / 256 -> 512 layers against 132 / 142 us for the
    // general kernel); with 64 channels the K loop is four slabs long and the general kernel's smaller per-tile prologue wins (147 vs 157 us)
    // bf16 operands: a third of the MFMA work per staged byte -- the patch tiles' five-round staging binds (459 / 378 us on 128 -> 256 /
    // 256 -> 512 at 24 images against 180 us for the general kernel's 128-wide tile: profiles/round4_bf16_layers.txt)
    if (s2 && (eligible_only || !onep)) return ConvFamily::H2D;
    return ConvFamily::H2R;
}

// `cus` CUs each run ceil(tiles / cus) tiles (co-resident workgroups share the MFMA pipe): minimise that count x tile area / efficiency
inline bool wide_pays(const ConvShape& s, long tm, double gain, int cus) {
    const double c64 = (double)((tm * ((s.cout + 63) / 64) + cus - 1) / cus) * 64.0;
    const double c128 = (double)((tm * ((s.cout + 127) / 128) + cus - 1) / cus) * 128.0 / gain;
    return s.npad % 128 == 0 && s.cout > 64 && c128 < c64;
}

// XCD grid: weight planes far beyond the 4 MiB of an XCD's L2 (FuseNet: 37.7 MB, its 1024 -> 1024 layer in the Winograd form 50 MB): a
// 2 x 4 XCD grid streams a quarter of them per XCD (conv_w1: 603 -> 565 us on 1024 -> 1024; conv_h2: -2..3 % on the 1024 -> 1024 layer,
// nothing on the 512 -> 512 ones: profiles/round3_conv_variants.txt)
inline int xcd_grid(const ConvShape& s, int requested, int tiles_m, int tiles_n, const char* who) {
    int gn = requested < 0 ? (((double)s.kpad * s.npad * 4 > 16e6) ? 4 : 0) : requested;
    if (gn && ((gn != 1 && gn != 2 && gn != 4 && gn != 8) || tiles_n % gn || tiles_m % (8 / gn))) {
        if (requested >= 0) throw std::invalid_argument(std::string(who) + ": the XCD grid does not divide the tile matrix");
        gn = 0;
    }
    return gn;
}

// Tiles per workgroup (conv_w1.hpp): chunks of 3 or 2 consecutive spatial tiles of one channel tile -- the prologue of every tile but a
// chunk's first disappears under its predecessor's last two periods.  Every XCD owns whole rows of the tile matrix (or its cell of the XCD
// grid) and the chunk size must divide their count.  A chunk that crosses into the next image needs the second transform table in LDS (it
// fits up to 512 input channels; a raw input has no table); without it chunks stay inside an image.  Chosen where the chunks fill the CUs
// in whole rounds -- so the chunk size DOES depend on the batch; what keeps a frame's bits independent of its batch is that every chunk
// size runs the same chains per output element (bit-identical, tested at the forward's shapes and under random ones).  A request of 1, 2
// or 3 forces a size (op tests, tools).
inline void plan_w1_chunk(const ConvShape& s, const ConvRequest& r, int cus, ConvPlan& p) {
    const int n = p.tiles_m * p.tiles_n, npp = ((s.cin >> 4) + 1) / 2;
    const int rows = p.xcd_gn ? p.tiles_m / (8 / p.xcd_gn) : (p.tiles_m % 8 ? 0 : p.tiles_m / 8);
    const bool tab2 = !s.transform || w1_lds_bytes_host(s.cin, 2) + 256 <= 160 * 1024;
    // (four periods at least: the fetch stream reads the next tile's periods 0..2 without the last period's tail mask -- with three
    // periods and an odd slab count, period 2 would stage another pixel's channels past Cin)
    auto fits = [&](int cc) { return cc == 1 || (s.nprod != 1 && npp >= 4 && rows > 0 && rows % cc == 0 && (tab2 || p.tpi % cc == 0)); };
    int cc = 1;
    if (r.chunk) {
        if (!fits(r.chunk)) throw std::invalid_argument("conv(w1): this chunk size does not fit the layer");
        cc = r.chunk;
    } else {
        for (int t : {3, 2}) if (fits(t) && n % (cus * t) == 0) { cc = t; break; }
        if (cc > r.chunk_cap) cc = 1;
    }
    p.w1_chunk = cc; p.w1_tab2 = (s.transform && tab2 && cc > 1) ? 1 : 0;
}

inline ConvPlan plan_conv(const ConvShape& s, const ConvRequest& r, int cus) {
    validate_conv(s);
    const bool onep = s.nprod == 1;                  // one product: a bf16 plane or (s.f16) an fp16 plane
    const int Ho = s.ho(), hw = Ho * s.wo();
    ConvPlan p;
    if (s.form == 1) {
        if (s.csplit || !w1_eligible(s.ks, s.stride, s.pad, s.cin, s.H, s.W))
            throw std::invalid_argument("conv(w1): the layer is packed in the Winograd form, which needs a single source and whole 4 x 32 tiles");
        if (s.f16) throw std::invalid_argument("conv(w1): the Winograd form is not built for fp16 operands (one fp16 plane); its one-product form takes bf16 operands");
        p.family = ConvFamily::W1;
    } else if (r.kernel == ConvKernel::General) {
        p.family = ConvFamily::H2R;
    } else {
        p.family = conv_class(s, r.rows == 2 ? 2 : kPlanTileRows, r.kernel == ConvKernel::Patch);
        if (r.kernel == ConvKernel::Patch && p.family == ConvFamily::H2R) throw std::invalid_argument("conv: this layer / frame size has no patch kernel");
    }
    // the half-resolution input: the 3 x 3 / stride-1 patch kernel's reflection-padded fp16 x 2 form and nothing else (checked further in case H2)
    if (s.up2 && (p.family != ConvFamily::H2 || !s.reflect || s.nprod != 3 || (s.H & 1) || (s.W & 1)))
        throw std::invalid_argument("conv: a half-resolution input (fused x2 upsample) needs the 3x3 / stride-1 patch kernel, reflection padding, fp16 x 2 operands (three products) and an even frame");
    // a bf16-stored input: the families without a bf16 load would read an fp32 descriptor over bf16 bytes (these three never become another
    // family below).  The forward never asks: its stems read the packed fp32 input and the bf16 modes keep the direct kernels.
    if (s.x_bf16 && (p.family == ConvFamily::W1 || p.family == ConvFamily::H2S || p.family == ConvFamily::H2S32))
        throw std::invalid_argument("conv: a bf16-stored input is not built for the Winograd form or the 7x7 stem kernels (they load fp32): the 3x3 patch kernels and the general kernels take it");
    if (s.nprod != 1 && s.nprod != 3 && (s.nprod != 4 || p.family != ConvFamily::H2))
        throw std::invalid_argument("conv: 1 (bf16 operands), 16 (fp16 operands) or 3 products; four on the 3x3 / stride-1 patch kernel's plain 4x64 and 4x128 tiles");
    if (s.f16 && s.nprod != 1) throw std::invalid_argument("conv: fp16 operands (one fp16 plane) run one product");
    auto set_tiles = [&](int rows_per_tile_m, int bn) {     // rows_per_tile_m: output positions of an M tile (patch: PR * 32; general: 128)
        p.tpi = (hw + rows_per_tile_m - 1) / rows_per_tile_m;
        p.tiles_m = s.N * p.tpi; p.tiles_n = (s.cout + bn - 1) / bn;
        // few tiles per image: the last workgroup of each (image, channel tile) finalises the statistics (conv_epilogue).  Many tiles per
        // image (the 64^2 .. 256^2 layers): the in_finalize2 launch spreads the fold over C / 16 x N workgroups.
        p.fin = s.fin_counter && p.tpi <= kFinMaxTiles && (size_t)s.N * ((s.npad + 31) / 32) <= kFinCounterInts;
    };
    switch (p.family) {
    case ConvFamily::W1:
        if (r.opt || r.sched != ConvSched::Plain) throw std::invalid_argument("conv(w1): no experiment variants");
        p.rows = kPlanTileRows; p.width = 64;
        set_tiles(kPlanTileRows * kPlanTileCols, 64);
        p.xcd_gn = xcd_grid(s, r.xcd_gn, p.tiles_m, p.tiles_n, "conv(w1)");
        plan_w1_chunk(s, r, cus, p);
        break;
    case ConvFamily::H2: {
        int pr = r.rows ? r.rows : kPlanTileRows, bn = r.width;
        if (bn == 0) {
            // 128-wide tiles (wave tile 64 x 64) move half the LDS / L1 bytes per MFMA: measured 1.07-1.15x per unit area without the
            // fused transform, 1.03x with it; the 384-tile ResnetBlock layers at batch 4 are the case where 768 64-wide tiles = exactly
            // three per CU win.  Small M (one driving frame: the decoder's ResnetBlocks are 64 tiles of 128 x 64 on 256 CUs): 32-wide
            // tiles double the number of workgroups; each stages the same patch but runs half the MFMA chain.
            const long tm = (long)s.N * (hw / 128);
            bn = wide_pays(s, tm, s.transform ? 1.03 : 1.10, cus) ? 128 : 64;
            // bf16 operands: one product per step -- the 64-wide tile is latency-bound (mfma_util 0.19, 81 % of the wave cycles
            // waiting at configs[4]); the 128-wide one runs three workgroups per CU as well (no second accumulator level) and wins
            // whenever it still fills the chip
            if (onep && s.npad % 128 == 0 && s.cout > 64 && tm * ((s.cout + 127) / 128) >= cus) bn = 128;
            // (Round 3 gave a forward of ONE frame two-K-group tiles here -- eight waves, total = P0 + P1: another association of the same
            // chains, so a frame run alone differed from its copy inside a batch in the last bits.  Since round 5 every layer that form
            // paid on runs conv_w1 in every batch (the decoder's second up-convolution included: 29.7 against 34.0 us for one frame, equal
            // at B = 4), and the forward no longer takes it: a frame's bits do not depend on its batch, B = 1 included.  The tile codes
            // 20032 / 20064 stay available to tsnet_op_conv2d.)
        }
        // bf16 operands, the 4 x 128 tile: the four waves SIDE BY SIDE (1 x 4, wave tile 128 x 32) instead of 2 x 2 (64 x 64) -- every weight
        // fragment is loaded once per workgroup instead of twice (the tile was bound by its weight loads: 72 of 80 vector loads per slab),
        // the A rows double-buffered by tap column: 120.5 -> 107.0 us on the 512 -> 512 layer, 96.1 -> 86.3 us on the decoder's first
        // up-convolution (profiles/round6_h2_1x4.txt).  Same K order and chains: the same bits as the 2 x 2 form (tests).  Tile code 3128
        // forces it, 128 the 2 x 2 form.
        p.side_by_side = r.alt || (!r.width && onep && pr == 4 && bn == 128);
        // what conv_h2_launch.cpp instantiates
        if (p.side_by_side && (!onep || bn != 128 || pr != 4)) throw std::invalid_argument("conv(h2): the 1 x 4 wave grid is the bf16 4 x 128 tile's (and its fp16-operand twin's: one product)");
        if (!(pr == 4 && (bn == 32 || bn == 64 || bn == 128)) && !(pr == 2 && bn == 128)) throw std::invalid_argument("conv(h2): tile must be 4x32, 4x64, 4x128 or 2x128");
        if (Ho % pr) throw std::invalid_argument("conv(h2): the output height must be a multiple of the tile's rows (2 or 4)");
        if (s.nprod == 4 && (pr != 4 || bn == 32 || r.sched != ConvSched::Plain)) throw std::invalid_argument("conv(h2): four products on the plain 4x64 and 4x128 tiles");
        if (r.sched == ConvSched::Deep) throw std::invalid_argument("conv(h2): the deep schedule (1xxxx) is the stride-2 2 x 128 tile's");
        if (r.sched == ConvSched::TwoGroups && (pr != 4 || bn == 128 || r.abl || r.opt))
            throw std::invalid_argument("conv(h2): the two-group tiles are 4x32 and 4x64, without experiment variants");
        if ((r.sched == ConvSched::TwoGroups || (r.opt & 16)) && (s.cin >> 4) % 2)       // (opt bit 4: the tools build's two-group experiments)
            throw std::invalid_argument("conv(h2): two K groups need an even number of 16-channel slabs");
        if (s.npad % bn) throw std::invalid_argument("conv(h2): the tile width must divide the padded output width");
        if (s.up2 && (pr != 4 || bn == 32 || p.side_by_side || r.sched != ConvSched::Plain || r.abl || r.opt))
            throw std::invalid_argument("conv(h2): the fused x2 upsample is built for the plain 4x64 and 4x128 tiles");
        p.up2 = s.up2;
        p.rows = pr; p.width = bn; p.sched = r.sched;
        set_tiles(pr * kPlanTileCols, bn);
        p.xcd_gn = xcd_grid(s, r.xcd_gn, p.tiles_m, p.tiles_n, "conv(h2)");
        break;
    }
    case ConvFamily::H2S:
    case ConvFamily::H2S32:
        p.rows = kPlanTileRows; p.width = 64;
        set_tiles(128, 64);
        break;
    case ConvFamily::H2D: {
        // two rows x 128 columns (four waves, 44 KiB of LDS: three workgroups per CU) wherever the layer is 128 channels wide: 125 -> 99 us
        // on 256 -> 512, 117 -> 109 us on 128 -> 256 at batch 4, equal or better down to one frame (profiles/round3_conv_variants.txt);
        // the four-row shapes hold 80 KiB and run one workgroup per CU
        if (r.sched == ConvSched::TwoGroups) throw std::invalid_argument("conv(h2d): the stride-2 tiles have no two-K-group form (1xxxx: the deep schedule of the 2 x 128 tile)");
        if (r.alt) throw std::invalid_argument("conv(h2d): tiles have two or four output rows");
        int pr = r.rows ? r.rows : kPlanTileRows, bn = r.width;
        if (bn == 0) {
            bn = 64;
            if (s.npad % 128 == 0 && s.cout > 64 && Ho % 2 == 0) { pr = 2; bn = 128; }
        }
        if (!(pr == 4 && (bn == 64 || bn == 128)) && !(pr == 2 && bn == 128))
            throw std::invalid_argument("conv(h2d): tile must be 4x64 (four waves), 4x128 (eight waves) or 2x128 (four waves)");
        if (s.npad % bn) throw std::invalid_argument("conv(h2d): the tile width must divide the padded output width");
        if (Ho % pr) throw std::invalid_argument("conv(h2d): the output height must be a multiple of the tile's rows");
        p.rows = pr; p.width = bn;
        set_tiles(pr * kPlanTileCols, bn);
        // A launch of at most two workgroups per CU (a single frame's: 64 .. 384 tiles) runs the deep schedule -- nothing else hides a lone
        // workgroup's memory round trips (72 -> us on the 64-tile launch).  Same bits: the choice may follow the batch.  Tile code 12128 forces
        // it, 2128 the plain schedule.
        const bool deep = r.width ? r.sched == ConvSched::Deep : (pr == 2 && bn == 128 && s.nprod == 3 && (long)p.tiles_m * p.tiles_n <= 2L * cus);
        if (deep && s.f16) throw std::invalid_argument("conv(h2d): the deep schedule (12128) is not built for fp16 operands (one fp16 plane): fp16 x 2 operands only");
        if (deep && (pr != 2 || bn != 128 || s.nprod != 3)) throw std::invalid_argument("conv(h2d): the deep schedule is the 2 x 128 tile's, fp16 x 2 operands");
        p.sched = deep ? ConvSched::Deep : ConvSched::Plain;
        break;
    }
    case ConvFamily::H2R:
    case ConvFamily::G64: {
        if (r.abl || r.opt) throw std::invalid_argument("conv: experiment variants exist for the 3x3 / stride-1 patch kernel only");
        if (r.rows || r.sched != ConvSched::Plain || (r.width && r.width != 64 && r.width != 128)) throw std::invalid_argument("conv(h2r): the tile width must be 64 or 128");
        // 64-deep K steps (conv_g64.hpp: the same bits, a quarter of the barriers and address computations, whole cache lines per
        // load) wherever the layer allows: 1 x 1 / 3 x 3, input channels (and the concat split) multiples of 64, 128-wide output.  In the
        // forward: the two 1 x 1 convolutions, the 64 -> 128 stride-2 layer and, with bf16 operands, every stride-2 layer.  Tile codes
        // 3064 / 3128 (with kernel = general) request it with 64 / 128 rows; 64 / 128 request conv_h2r with that width.
        const bool g64_ok = (s.ks == 1 || s.ks == 3) && (s.cin & 63) == 0 && (!s.csplit || (s.csplit & 63) == 0) && s.npad % 128 == 0 && s.cout > 64;
        if (r.alt || (!r.width && g64_ok)) {
            if (!g64_ok) throw std::invalid_argument("conv(g64): needs a 1 x 1 / 3 x 3 layer, input channels in multiples of 64 and more than 64 output channels");
            // rows per tile: 64 in every batch (with statistics the tile decides the partial sums' grouping, so it may never depend on the
            // batch: a frame's bits do not)
            // (measured, tools/g64_variants.py: the 128-row tile -- eight waves at 140 VGPRs: one workgroup per CU -- loses everywhere with
            // fp16 x 2 operands, 208 vs 156 us on the 64 -> 128 stride-2 layer, and ties with bf16 operands)
            p.family = ConvFamily::G64;
            p.rows = r.width ? r.width : 64; p.width = 128;
            set_tiles(p.rows, 128);
        } else {
            const long tm = (long)s.N * ((hw + 127) / 128);
            const int bn = r.width ? r.width : ((s.ks == 3 && s.cin >= 16 && wide_pays(s, tm, 1.15, cus)) ? 128 : 64);
            if (bn == 128 && (s.ks != 3 || s.cin == 8)) throw std::invalid_argument("conv(h2r): 128-wide tiles are built for 3x3 layers with at least 16 input channels");
            if (s.ks == 1 && s.cin == 8) throw std::invalid_argument("conv(h2r): 1x1 layers need at least 16 input channels");
            if (s.npad % bn) throw std::invalid_argument("conv(h2r): the tile width must divide the padded output width");
            p.family = ConvFamily::H2R;
            p.rows = 128; p.width = bn;
            set_tiles(128, bn);
        }
        break;
    }
    }
    return p;
}

// Does the layer take the fused-upsample form at this shape?  (The decoder asks before it decides whether the upsampled tensor has to exist.)
inline bool plan_takes_up2(ConvShape s, int cus) {
    s.up2 = true;
    try { return plan_conv(s, ConvRequest{}, cus).up2; } catch (const std::invalid_argument&) { return false; }
}

// g_launch_counters[3] (tsnet_launch_counters: bench.py labels the roofline kernel with it): rows * 1000 + width of a 3 x 3 / stride-1 tile,
// 3xxx its side-by-side wave grid, + 20000 two K groups, + 30000 the Winograd form; 0: the family has no code
inline int plan_tile_code(const ConvPlan& p) {
    if (p.family == ConvFamily::W1) return 30000 + p.rows * 1000 + p.width;
    if (p.family != ConvFamily::H2) return 0;
    return (p.side_by_side ? 3 : p.rows) * 1000 + p.width + (p.sched == ConvSched::TwoGroups ? 20000 : 0);
}

// A launcher handed a plan it has no kernel for: the planner and the launcher disagree -- a bug, not a user error.
[[noreturn]] inline void plan_not_built(const ConvPlan& p, int nprod) {
    throw std::logic_error("conv: no kernel for plan family " + std::to_string((int)p.family) + ", tile " + std::to_string(p.rows) + " x " + std::to_string(p.width) +
                           (p.side_by_side ? " side by side" : "") + ", schedule " + std::to_string((int)p.sched) + ", " + std::to_string(nprod) + " products");
}

// RGB head (head_conv.hpp head_conv3_kernel): tile rows by the number of workgroups -- the tallest tile that still gives every CU one: 32
// rows from B = 4 on at 256^2, 16 at B = 2, 8 for one frame (84 -> 3x us there: eight waves on 64 CUs queue at the LDS pipe).  Same bits
// for every choice.
inline int head_rows(int B, int tiles_x, int hh, int cus) {
    return (long)B * tiles_x * ((hh + 31) / 32) >= cus ? 32 : ((long)B * tiles_x * ((hh + 15) / 16) >= cus ? 16 : 8);
}

}  // namespace tsnet
