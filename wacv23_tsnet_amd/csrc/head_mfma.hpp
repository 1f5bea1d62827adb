// head_mfma.hpp -- the decoder's RGB head (ReflectionPad2d(3) + Conv2d(C -> 3, 7x7) + bias + Tanh on relu(IN(x)), pose composite) on the
// matrix pipe.  One output pixel per GEMM row wastes 91 % of the MFMA (Cout = 3 of 32 columns).  Here a BLOCK of 2 x 4 output pixels x 3
// channels is folded into N: the block at rows 2Y, 2Y+1 / columns 4X .. 4X+3 shares an 8 x 10 input window, so
//   A[(Y, X)][(r, j, c)]       = relu(x * alpha + beta) at pixel (2Y + r - 3, 4X + j - 3) (reflected), channel c        r = 0..7, j = 0..9
//   B[(r, j, c)][(dy, dx, o)]  = w[o][c][r - dy][j - dx] where 0 <= r - dy <= 6 and 0 <= j - dx <= 6, else 0;  n = (dy * 4 + dx) * 3 + o < 24
//   out[o][2Y + dy][4X + dx]   = tanh(total * unscale + bias[o])
// 24 of 32 columns and 49 of 80 window positions are real: 0.46 of the matrix work is useful instead of 0.09.
//
// Operands are the fp16 (hi, lo) split of every convolution here (conv_common.hpp), activations scaled by the power of two of the a-priori
// bound sqrt(H W) of an InstanceNorm output, weights by the power of two of their maximum; three products per k-group in w1_step_products'
// order (lo*hi, hi*lo, hi*hi), in every operand mode.
//
// K ORDER AND CHAINS (fixed: a pixel's bits depend on neither tile height, tile position, batch nor the frame's edges).  The channels go in
// STAGES of 8; inside a stage k = ((r * 5 + jp) * 2 + lh) * 8 + e: window row r, column pair jp, column j = 2 jp + lh, channel 8 stage + e
// -- a 16-deep MFMA step is two adjacent window columns x 8 channels, 40 steps per stage.  A chain is one window row of a stage (5 steps =
// 80 k, 15 MFMAs from a zero accumulator); chains fold into a running fp32 total in the order they run.  The even stages run on one half of
// the workgroup's waves and the odd stages on the other (each half through its own patch: two waves per CU at work on every SIMD pair);
// result = (total of the even stages + total of the odd stages) * unscale.  Blocks hanging over the frame's edge stage clamped (finite)
// pixels; their products meet the zero rows of B in the pixels that are stored.
//
// Staging follows the patch kernels: the (TR + 6) x 38-pixel patch of a stage pair's 16 channels is fetched once by the whole workgroup (four
// lanes per pixel: 64 contiguous bytes), IN + ReLU + scale + split in registers, written as 8-byte half octets into the two halves' patches.  The 32 lanes of an A fragment are the 4 x 8 blocks of an 8-row x 32-column
// row tile: pixels 4 apart in x and 2 apart in y.  Patch columns are de-interleaved modulo 4 ([row][column phase][slot]), so the eight
// blocks of a row read consecutive slots, and the row pitch is 44 slots = 704 B (2 rows = 128 mod 256 B): the two block rows of a 16-lane
// group sit on disjoint banks.  A wave loads its weight fragments itself, three steps ahead, from the folded filter table (80 C x 32 x two
// planes; 640 KiB at C = 64: the same for every workgroup, L2-resident).  With 16- or 32-row tiles a wave owns TWO row tiles (one 1 KiB
// fragment per 6 MFMAs) but the workgroup's 62 - 107 KB of LDS leave one wave per SIMD, and nothing covers its staging round trips: 78 - 80 us
// at B = 4.  The 8-row tile (one row tile per wave, a fragment per 3 MFMAs, 40 KB, 135 VGPRs) runs four workgroups per CU = two waves per
// SIMD: 53 us, and 28 us for one frame -- the launcher's choice in every batch (profiles/head_mfma.txt).  Same bits for every tile height.
#pragma once
#include "kernels.hpp"

namespace tsnet {

constexpr int kHmPitch = 44, kHmPhase = 11;                       // slots (16 B) per patch row and per column phase
constexpr int kHmSteps = 40;                                      // MFMA steps per 8-channel stage
constexpr int hm_plane_bytes(int TR) { return (TR + 6) * kHmPitch * 16; }
constexpr int hm_threads(int TR) { return TR == 32 ? 256 : 128; }
constexpr size_t head_mfma_lds_bytes(int TR, int C) { return (size_t)4 * hm_plane_bytes(TR) + (size_t)2 * C * sizeof(float); }
static_assert(head_mfma_table_halves(8) == (size_t)kHmSteps * 2 * 64 * 8, "one stage of the table");

template <int TR>
__global__ __launch_bounds__(hm_threads(TR), 1) void head_mfma_kernel(HeadMfmaArgs a) {
    static_assert(TR == 32 || TR == 16 || TR == 8, "tile rows");
    constexpr int MT = TR >= 16 ? 2 : 1;                          // row tiles (8 rows x 32 columns = 32 blocks) of a wave
    constexpr int WH = TR / 8 / MT;                               // waves of a half
    constexpr int TH = WH * 64;
    constexpr int PRW = TR + 6, PC = 38, PP = PRW * PC;
    constexpr int PLANE = hm_plane_bytes(TR);
    constexpr int NT = 2 * TH;                                    // threads of the workgroup
    constexpr int NPE = (PP * 4 + NT - 1) / NT;                   // staged (pixel, channel quad) entries per thread and stage pair: 23 (TR = 32), 27, 17
    constexpr int NBATCH = 2, BE = (NPE + NBATCH - 1) / NBATCH;

    HIP_DYNAMIC_SHARED(__attribute__((aligned(16))) unsigned char, smem_raw)
    const int half = TSNET_UNIFORM((int)(threadIdx.x / TH));      // wave-uniform
    const int tid = threadIdx.x - half * TH;
    const int lane = tid & 63, li = lane & 31, lh = lane >> 5;
    const int wv = TSNET_UNIFORM(tid >> 6);                       // wave of the half: row tiles wv * MT ..
    unsigned char* tile = smem_raw + half * 2 * PLANE;            // [plane][patch row][column phase][slot] x 16 B
    float* abt = reinterpret_cast<float*>(smem_raw + 4 * PLANE);  // alpha * 2^sa [C], beta * 2^sa [C]
    const int tiles_x = (a.W + 31) / 32;
    const int n = blockIdx.y;
    const int bx0 = (blockIdx.x % tiles_x) * 32, by0 = (blockIdx.x / tiles_x) * TR;

#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)      // (a vectorised form multiplies in pairs: no packed fp32 multiply in an MFMA unit)
    for (int i = threadIdx.x; i < 2 * a.C; i += 2 * TH)
        abt[i] = (i < a.C ? a.alpha[(size_t)n * a.C + i] : a.beta[(size_t)n * a.C + i - a.C]) * a.in_scale;

    const unsigned xbytes = (unsigned)((size_t)a.N * a.H * a.W * a.C * (a.x_bf16 ? 2 : 4));
    const tsnet_brsrc_t rsx = tsnet_make_brsrc(a.x, xbytes);
    const unsigned wbytes = (unsigned)(head_mfma_table_halves(a.C) * 2);
    const tsnet_brsrc_t rsw = tsnet_make_brsrc(a.wq, wbytes);

    // ---- staging geometry, fixed over the stages.  The whole workgroup stages BOTH halves' patches of a stage pair (16 channels = 64 B of a
    //      pixel): four adjacent lanes read the four channel quads of one pixel -- 64 contiguous bytes, a wave's load covers 16 lines, not 64
    //      -- quads 0, 1 are the octet of half 0's stage, quads 2, 3 that of half 1's.  Source offset in fp32 bytes.
    const int quad = threadIdx.x & 3;
    unsigned src_off[NPE];
#pragma unroll
    for (int e = 0; e < NPE; ++e) {
        const int i = ((int)threadIdx.x + e * NT) >> 2;
        const int p = i < PP ? i : PP - 1;
        const int py = p / PC, px = p - py * PC;
        int iy = by0 + py - 3, ix = bx0 + px - 3;
        iy = iy < 0 ? -iy : iy; iy = iy >= a.H ? 2 * (a.H - 1) - iy : iy;
        ix = ix < 0 ? -ix : ix; ix = ix >= a.W ? 2 * (a.W - 1) - ix : ix;
        iy = iy < 0 ? 0 : (iy >= a.H ? a.H - 1 : iy);             // tiles and blocks hanging over the edge: any valid address
        ix = ix < 0 ? 0 : (ix >= a.W ? a.W - 1 : ix);
        src_off[e] = (unsigned)((((size_t)n * a.H + iy) * a.W + ix) * a.C * 4 + quad * 16);
    }
    auto stage = [&](int sp) __attribute__((always_inline)) {      // stage pair sp: channels 16 sp .. 16 sp + 15
        int tx = (int)threadIdx.x;
        TSNET_OPAQUE_V(tx);
        const F4 al = *reinterpret_cast<const F4*>(abt + sp * 16 + quad * 4), be = *reinterpret_cast<const F4*>(abt + a.C + sp * 16 + quad * 4);
#pragma unroll
        for (int b = 0; b < NBATCH; ++b) {
            F4 sx[BE];
#pragma unroll
            for (int e = 0; e < BE; ++e) {
                if (b * BE + e < NPE) {
                    if (a.x_bf16) {                               // bf16 storage: four bf16 = 8 bytes, widened exactly
                        const F2 q = TSNET_BUF_LOAD8(rsx, src_off[b * BE + e] >> 1, (unsigned)(sp * 32));
                        const unsigned w0 = __builtin_bit_cast(unsigned, q.v[0]), w1 = __builtin_bit_cast(unsigned, q.v[1]);
                        sx[e].v[0] = __builtin_bit_cast(float, w0 << 16); sx[e].v[1] = __builtin_bit_cast(float, w0 & 0xFFFF0000u);
                        sx[e].v[2] = __builtin_bit_cast(float, w1 << 16); sx[e].v[3] = __builtin_bit_cast(float, w1 & 0xFFFF0000u);
                    } else {
                        sx[e] = TSNET_BUF_LOAD16(rsx, src_off[b * BE + e], (unsigned)(sp * 64));
                    }
                }
            }
#pragma unroll
            for (int e = 0; e < BE; ++e) {
                if (b * BE + e < NPE) {
                    float t[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) t[k] = __builtin_fmaxf(__builtin_fmaf(sx[e].v[k], al.v[k], be.v[k]), 0.f);
                    unsigned h0, l0, h1, l1;
                    TSNET_SPLIT_2PAIRS(t[0], t[1], t[2], t[3], h0, l0, h1, l1);
                    const int i = (tx + (b * BE + e) * NT) >> 2;   // the LDS slot is recomputed under the loads' latency, not kept in registers
                    if (i < PP) {
                        const int py = i / PC, px = i - py * PC;
                        unsigned char* dst = smem_raw + (quad >> 1) * 2 * PLANE + (py * kHmPitch + (px & 3) * kHmPhase + (px >> 2)) * 16 + (quad & 1) * 8;
                        uint2 hw2, lw2;
                        hw2.x = h0; hw2.y = h1; lw2.x = l0; lw2.y = l1;
                        *reinterpret_cast<uint2*>(dst) = hw2;
                        *reinterpret_cast<uint2*>(dst + PLANE) = lw2;
                    }
                }
            }
        }
    };

    // ---- fragments: A of step t at window (r, jp) is a shifted view of the patch; B straight from the table, three steps ahead
    const unsigned char* abase = tile + (((wv * MT * 8 + 2 * (li >> 3)) * kHmPitch + lh * kHmPhase + (li & 7)) * 16);
    const unsigned vB = (unsigned)(lane * 16);
    F4 af[2][2][MT], bf[4][2];
    auto load_b = [&](int set, int g) __attribute__((always_inline)) {            // g = stage * 40 + step; past the table the descriptor returns zeros
#pragma unroll
        for (int p = 0; p < 2; ++p) bf[set][p] = TSNET_BUF_LOAD16(rsw, vB, (unsigned)((g * 2 + p) * 1024));
    };
    auto load_a = [&](int set, int t) __attribute__((always_inline)) {            // t: wave-uniform step of the stage
        const int r = t / 5, jp = t - r * 5;
        const unsigned char* b = abase + (r * kHmPitch + ((2 * jp) & 3) * kHmPhase + (jp >> 1)) * 16;
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int p = 0; p < 2; ++p) af[set][p][i] = *reinterpret_cast<const F4*>(b + p * PLANE + i * 8 * kHmPitch * 16);
    };
    f32x16 acc[MT], tot[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc[i][r] = 0.f; tot[i][r] = 0.f; }
    auto product = [&](int sa, int sb, int pa, int pb, bool fresh) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            f32x16 c = acc[i];
            if (fresh) {
#pragma unroll
                for (int r = 0; r < 16; ++r) c[r] = 0.f;
            }
            acc[i] = TSNET_MFMA_F16(af[sa][pa][i], bf[sb][pb], c);
        }
    };

    const int nst = a.C / 8;                                      // an even number of stages (C % 16 == 0: the launcher)
    load_b(0, half * kHmSteps); load_b(1, half * kHmSteps + 1); load_b(2, half * kHmSteps + 2);
    __syncthreads();                                              // the transform table
    for (int stg = half; stg < nst; stg += 2) {
        stage(stg >> 1);
        __syncthreads();
        load_a(0, 0);
#pragma unroll 1
        for (int rq = 0; rq < 2; ++rq) {                          // 2 x 20 steps: four window rows (chains) per iteration
#pragma unroll
            for (int u = 0; u < 20; ++u) {
                const int t = rq * 20 + u;
                const int tb = t + 3;                             // B three steps ahead: the tail of a stage fetches the head of this half's next one
                load_b((u + 3) & 3, stg * kHmSteps + tb + (tb >= kHmSteps ? kHmSteps : 0));
                const int ta = t + 1;                             // A one step ahead (the last step re-reads step 0: unused, but a valid address)
                load_a((u + 1) & 1, ta >= kHmSteps ? 0 : ta);
                product(u & 1, u & 3, 1, 0, u % 5 == 0);          // lo * hi
                product(u & 1, u & 3, 0, 1, false);               // hi * lo
                product(u & 1, u & 3, 0, 0, false);               // hi * hi
                if (u % 5 == 4) {
#pragma unroll
                    for (int i = 0; i < MT; ++i) tot[i] += acc[i];
                }
            }
        }
        __syncthreads();                                          // the patch is free for the next stage
    }

    // ---- half 1 hands its totals over through LDS (the patches are free after the last barrier); half 0 + half 1, un-scale, bias, tanh
    float* xch = reinterpret_cast<float*>(smem_raw);
    if (half == 1) {
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) xch[(i * 16 + r) * TH + tid] = tot[i][r];
    }
    __syncthreads();
    if (half == 1) return;
    const float unscale = a.in_unscale * a.w_unscale[0];
    const int o = li % 3, dx = (li / 3) & 3, dy = li / 12;
    const float bias = li < 24 ? a.bias[o] : 0.f;
    const float bgv = o == 0 ? a.bg[0] : (o == 1 ? a.bg[1] : a.bg[2]);
    const size_t hw = (size_t)a.H * a.W;
#pragma unroll
    for (int i = 0; i < MT; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = (r & 3) + 8 * (r >> 2) + 4 * lh;        // block of the row tile: (m >> 3, m & 7)
            const int oy = by0 + (wv * MT + i) * 8 + 2 * (m >> 3) + dy, ox = bx0 + 4 * (m & 7) + dx;
            float v = tanhf((tot[i][r] + xch[(i * 16 + r) * TH + tid]) * unscale + bias);
            if (a.composite && (ox < a.fore_x0 || ox >= a.fore_x1)) v = bgv;
            if (li < 24 && oy < a.H && ox < a.W) a.y[((size_t)n * 3 + o) * hw + (size_t)oy * a.W + ox] = v;
        }
    }
}

// w (3, C, 7, 7) fp32 -> the folded planes in the kernel's fragment order, scaled by `scale` (a power of two) and split
__global__ void pack_head_mfma_kernel(const float* __restrict__ w, unsigned short* __restrict__ out, int C, float scale) {
    const size_t total = head_mfma_table_halves(C);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int e = (int)(i & 7), lane = (int)((i >> 3) & 63), plane = (int)((i >> 9) & 1);
        const int g = (int)(i >> 10), stg = g / kHmSteps, t = g - stg * kHmSteps;
        const int r = t / 5, j = 2 * (t - r * 5) + (lane >> 5), nn = lane & 31, c = stg * 8 + e;
        unsigned hi = 0, lo = 0;
        if (nn < 24) {
            const int o = nn % 3, dx = (nn / 3) & 3, dy = nn / 12;
            const int ky = r - dy, kx = j - dx;
            if (ky >= 0 && ky <= 6 && kx >= 0 && kx <= 6) split_h2(w[((size_t)o * C + c) * 49 + ky * 7 + kx] * scale, hi, lo);
        }
        out[i] = (unsigned short)(plane ? lo : hi);
    }
}

}  // namespace tsnet
