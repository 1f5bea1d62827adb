// norm_elementwise.hpp -- HBM-bound kernels around the convolutions (NHWC fp32, 16 B per lane).
//
// Replaces on the reference hot path:
//   * nn.InstanceNorm2d statistics (affine=False, eps=1e-5, biased variance; TSNet.py:53 default
//     norm_layer)                                                        -> in_stats_partial + in_finalize
//   * the ResnetBlock tail  x + IN(conv(..))   (TSNet.py:47-49)          -> norm_act_kernel(resid)
//   * Encoder tail  ReLU(IN(.)) materialised once (TSNet.py:70-71)       -> norm_act_kernel(relu)
//   * FuseNet residual + the mean over sources (TSNet.py:195-200, :400)  -> fuse_resid_mean_kernel
//   * nn.Upsample(x2, bilinear, align_corners=False) (TSNet.py:145)      -> upsample2x_kernel
//   * set_test_input's /255 + torch.cat + coord_conv (TSNet.py:286,312,107-125) -> pack_input_kernel
// All reductions use a fixed order (no float atomics): results are run-to-run deterministic.
#pragma once
#include <hip/hip_runtime.h>

#include "conv_common.hpp"

namespace tsnet {

// ---------------------------------------------------------------------------------------------
// InstanceNorm statistics, stage 1: per (image n, split s) partial sum / sum of squares per channel,
// accumulated in fp64.  x: (N, HW, C).  part: (N, S, C, 2) doubles.
// Thread layout: cq = float4 column within the row, rg = row group; block covers all C/4 columns
// (or 256 of them; grid.z walks the rest).
struct StatsArgs {
    const float* x;
    double* part;
    int HW, C, S, rows_per_split;
};

// The same reduction fused with an addition: y[n] = x[slot[n]] + add[n % add_nmod], statistics of y.  FuseNet's first convolution is split at
// the channel concat (TSNet.py:195-197: cat(src_fea, tar_fea) -> conv): the per-source half is computed once per source set
// (tsnet_set_sources, cached in clip mode), the shared target half once per driving frame; this kernel joins them and produces the
// InstanceNorm statistics of the sum.  One-shot forward and clip mode run the SAME kernels in the same order: bit-identical results.
struct AddStatsArgs {
    const float* x;      // (slots, HW, C): image n reads x[slot[n]]
    const int* slot;     // [N] device, the slot table (flow_args.hpp); n is fixed per workgroup: one scalar load
    const float* add;    // (add_nmod, HW, C)
    float* y;            // (N, HW, C)
    double* part;        // (N, S, C, 2)
    int HW, C, S, rows_per_split, add_nmod;
};

// The body of both statistics kernels: the thread layout, the fp64 accumulation of a float4 per row, the fixed-order LDS fold over the row
// groups and the partial store.  ADD selects the load alone: the plain tensor, or the sum with its store of y.
template <bool ADD, typename Args>
__device__ __forceinline__ void stats_partial_body(const Args& a) {
    __shared__ double red[256 * 8];
    const int cq_total = a.C >> 2;
    const int cols = cq_total < 256 ? cq_total : 256;   // float4 columns handled per block
    const int R = 256 / cols;                            // row groups
    const int tid = threadIdx.x;
    const int cq = tid % cols + blockIdx.z * 256;
    const int rg = tid / cols;
    const int n = blockIdx.y, s = blockIdx.x;
    const int r0 = s * a.rows_per_split;
    int r1 = r0 + a.rows_per_split;
    if (r1 > a.HW) r1 = a.HW;
    double sm[4] = {0, 0, 0, 0}, sq[4] = {0, 0, 0, 0};
    if (rg < R && cq < cq_total) {
        const size_t cb = (size_t)cq * 4;
        int nb = 0, nx = n;                                  // the images of add and of x
        if constexpr (ADD) { nb = n % a.add_nmod; nx = a.slot[n]; }
        const float* bx = a.x + ((size_t)nx * a.HW) * a.C + cb;
        const float* ba = nullptr;
        float* by = nullptr;
        if constexpr (ADD) { ba = a.add + ((size_t)nb * a.HW) * a.C + cb; by = a.y + ((size_t)n * a.HW) * a.C + cb; }
        for (int r = r0 + rg; r < r1; r += R) {
            float4 v = *reinterpret_cast<const float4*>(bx + (size_t)r * a.C);
            if constexpr (ADD) {
                v = add4(v, *reinterpret_cast<const float4*>(ba + (size_t)r * a.C));
                *reinterpret_cast<float4*>(by + (size_t)r * a.C) = v;
            }
            sm[0] += v.x; sq[0] += (double)v.x * v.x;
            sm[1] += v.y; sq[1] += (double)v.y * v.y;
            sm[2] += v.z; sq[2] += (double)v.z * v.z;
            sm[3] += v.w; sq[3] += (double)v.w * v.w;
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) { red[tid * 8 + e] = sm[e]; red[tid * 8 + 4 + e] = sq[e]; }
    __syncthreads();
    if (rg == 0 && cq < cq_total) {
        double tsm[4] = {0, 0, 0, 0}, tsq[4] = {0, 0, 0, 0};
        for (int g = 0; g < R; ++g) {
            const int t = g * cols + tid;
#pragma unroll
            for (int e = 0; e < 4; ++e) { tsm[e] += red[t * 8 + e]; tsq[e] += red[t * 8 + 4 + e]; }
        }
        double* o = a.part + (((size_t)n * a.S + s) * a.C + (size_t)cq * 4) * 2;
#pragma unroll
        for (int e = 0; e < 4; ++e) { o[e * 2] = tsm[e]; o[e * 2 + 1] = tsq[e]; }
    }
}
__global__ __launch_bounds__(256) void in_stats_partial_kernel(StatsArgs a) { stats_partial_body<false>(a); }
__global__ __launch_bounds__(256) void add_stats_partial_kernel(AddStatsArgs a) { stats_partial_body<true>(a); }

// stage 2: alpha = 1/sqrt(var+eps), beta = -mean*alpha  (the x*alpha+beta form ATen's CPU
// batch-norm transform uses), one thread per (n, c).
// (The tail -- mean, clamped variance, alpha, beta -- is not shared with in_finalize2_kernel and conv_epilogue: as in_alpha_beta(sm, sq, HW,
// eps, ...) taking the two elements' addresses, the arrays and an index, or the sums by reference and the index as a functor, both kernels
// kept their instruction and register counts but not their text: the zero fills of sm / sq swap, or the index is formed before the division.)
__global__ void in_finalize_kernel(const double* __restrict__ part, float* __restrict__ alpha, float* __restrict__ beta,
                                   int NC, int C, int S, int HW, float eps) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= NC) return;
    const int n = i / C, c = i - n * C;
    double sm = 0, sq = 0;
    for (int s = 0; s < S; ++s) {
        const double* p = part + (((size_t)n * S + s) * C + c) * 2;
        sm += p[0];
        sq += p[1];
    }
    const double mean = sm / HW;
    double var = sq / HW - mean * mean;
    if (var < 0) var = 0;
    const float al = 1.0f / sqrtf((float)var + eps);
    alpha[i] = al;
    beta[i] = -((float)mean) * al;
}

// stage 2 for many partials (conv-epilogue statistics: S = tiles per image, up to 1024):
// block = (image n, 16 channels); 16 thread groups split the S partials (group g takes s = g, g + 16, ...), fixed-order LDS combine.
// (Four groups of 64 channels left 12 workgroups walking 128 dependent additions each on the 7 x 7 stem: 16 us of latency per launch.)
constexpr int kFin2Ch = 16, kFin2Groups = 16;
__global__ __launch_bounds__(256) void in_finalize2_kernel(const double* __restrict__ part, float* __restrict__ alpha,
                                                            float* __restrict__ beta, int C, int S, int HW, float eps) {
    __shared__ double red[256 * 2];
    const int n = blockIdx.y, cl = threadIdx.x & (kFin2Ch - 1), c = blockIdx.x * kFin2Ch + cl, g = threadIdx.x / kFin2Ch;
    double sm = 0, sq = 0;
    if (c < C) {
        // the loads of 8 partials are issued before the first addition (explicitly: an `unroll 8` of the one-pair loop still compiled to a
        // memory round trip per partial -- 77 us for the 512 partials of the stem); the additions stay in order, entries past S contribute +0.0
        for (int s0 = g; s0 < S; s0 += 8 * kFin2Groups) {
            double v[8], w[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int s = s0 + u * kFin2Groups;
                const double* p = part + (((size_t)n * S + (s < S ? s : g)) * C + c) * 2;
                v[u] = p[0]; w[u] = p[1];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const bool in = s0 + u * kFin2Groups < S;
                sm += in ? v[u] : 0.0;
                sq += in ? w[u] : 0.0;
            }
        }
    }
    red[threadIdx.x * 2] = sm; red[threadIdx.x * 2 + 1] = sq;
    __syncthreads();
    if (g == 0 && c < C) {
        for (int k = 1; k < kFin2Groups; ++k) { sm += red[(k * kFin2Ch + cl) * 2]; sq += red[(k * kFin2Ch + cl) * 2 + 1]; }
        const double mean = sm / HW;
        double var = sq / HW - mean * mean;
        if (var < 0) var = 0;
        const float al = 1.0f / sqrtf((float)var + eps);
        alpha[(size_t)n * C + c] = al;
        beta[(size_t)n * C + c] = -((float)mean) * al;
    }
}

// ---------------------------------------------------------------------------------------------
// y = alpha*x + beta (optionally ReLU) (+ resid).  alpha==null -> y = x (+resid).  In-place safe.
struct NormActArgs {
    const float* x;
    const float* alpha;
    const float* beta;
    const float* resid;
    float* y;
    int HW, C, relu;
    size_t total4;   // N*HW*C/4
};

// grid = (chunks, N): the image comes from blockIdx.y and the channel quad is advanced incrementally -- no per-element
// division (a 64-bit i / per_img, i % c4n per float4 made this kernel VALU-bound at 3.2 TB/s).  When the grid stride
// is a multiple of C/4 (always, for the power-of-two widths of the model) a thread stays on one channel quad and the
// scale/shift pair is loaded once.
__global__ __launch_bounds__(256) void norm_act_kernel(NormActArgs a) {
    const unsigned c4n = (unsigned)a.C >> 2;
    const unsigned per_img = (unsigned)a.HW * c4n;
    const unsigned n = blockIdx.y;
    const unsigned stride = gridDim.x * 256u;
    const unsigned sc = stride % c4n;
    unsigned j = blockIdx.x * 256u + threadIdx.x;
    unsigned cq = j % c4n;
    const bool fixed_c = sc == 0 && a.alpha != nullptr;
    float4 al = make_float4(1.f, 1.f, 1.f, 1.f), be = make_float4(0.f, 0.f, 0.f, 0.f);
    if (fixed_c) {
        al = *reinterpret_cast<const float4*>(a.alpha + (size_t)n * a.C + cq * 4);
        be = *reinterpret_cast<const float4*>(a.beta + (size_t)n * a.C + cq * 4);
    }
    for (; j < per_img; j += stride) {
        const size_t i = (size_t)n * per_img + j;
        float4 v = reinterpret_cast<const float4*>(a.x)[i];
        if (a.alpha) {
            if (!fixed_c) {
                al = *reinterpret_cast<const float4*>(a.alpha + (size_t)n * a.C + cq * 4);
                be = *reinterpret_cast<const float4*>(a.beta + (size_t)n * a.C + cq * 4);
                cq += sc; if (cq >= c4n) cq -= c4n;
            }
            v = fma4(v, al, be);
        }
        if (a.relu) v = relu4(v);
        if (a.resid) v = add4(reinterpret_cast<const float4*>(a.resid)[i], v);
        reinterpret_cast<float4*>(a.y)[i] = v;
    }
}

// ---------------------------------------------------------------------------------------------
// FuseNet tail: zbar[b,p,:] = (1/K) * sum_i ( cat(src_fea[slot[i*B+b]], tar_fea[b])[p,:] + IN(y2[i*B+b])[p,:] )
// The 1x1 `fuse_net.conv` that follows is linear, so it is applied once to the mean
// (mean_i conv(z_i)+bias == conv(mean_i z_i)+bias).
struct FuseTailArgs {
    const float* src_fea;   // (slots, P, C1): (source s, driving frame b) reads image slot[s*B + b]
    const float* tar_fea;   // (B, P, C1)
    const float* y2;        // (K*B, P, 2*C1)
    const float* alpha;     // (K*B * 2*C1)
    const float* beta;
    float* zbar;            // (B, P, 2*C1)
    const int* slot;        // [K*B] device, the slot table (flow_args.hpp)
    int B, K, P, C1;
};

__global__ __launch_bounds__(256) void fuse_resid_mean_kernel(FuseTailArgs a) {
    const int C = 2 * a.C1;
    const int c4n = C >> 2;
    const size_t total = (size_t)a.B * a.P * c4n;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int c = (int)(i % c4n) * 4;
        const size_t bp = i / c4n;                  // b*P + p
        const int b = (int)(bp / a.P);
        const int p = (int)(bp - (size_t)b * a.P);
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int s = 0; s < a.K; ++s) {
            const int n = s * a.B + b;
            float4 xr;
            if (c < a.C1) xr = *reinterpret_cast<const float4*>(a.src_fea + ((size_t)a.slot[n] * a.P + p) * a.C1 + c);
            else          xr = *reinterpret_cast<const float4*>(a.tar_fea + ((size_t)b * a.P + p) * a.C1 + (c - a.C1));
            const float4 y = *reinterpret_cast<const float4*>(a.y2 + ((size_t)n * a.P + p) * C + c);
            const float4 al = *reinterpret_cast<const float4*>(a.alpha + (size_t)n * C + c);
            const float4 be = *reinterpret_cast<const float4*>(a.beta + (size_t)n * C + c);
            acc = add4(acc, add4(xr, fma4(y, al, be)));
        }
        *reinterpret_cast<float4*>(a.zbar + ((size_t)b * a.P + p) * C + c) = div4(acc, (float)a.K);
    }
}

// The slot table of a forward: up to kSlotFill entries per launch, passed by value and written with ordinary vector stores.
// Stream-ordered by construction -- no host buffer outlives the call that enqueues it.
constexpr int kSlotFill = 64;
struct SlotFillArgs { int* dst; int n; int v[kSlotFill]; };
__global__ __launch_bounds__(64) void slot_fill_kernel(SlotFillArgs a) {
    const int i = threadIdx.x;
    if (i < a.n) a.dst[i] = a.v[i];
}

// ---------------------------------------------------------------------------------------------
// Bilinear x2 upsample, align_corners=False: src = (dst+0.5)/2-0.5 clamped at 0, neighbour index
// clamped at in-1; horizontal lerp first, then vertical (ATen's separable order).  Optional
// producer InstanceNorm+ReLU applied to the four taps on load.
struct UpsampleArgs {
    const float* x;       // (N,H,W,C)
    const float* alpha;   // (N*C) or null
    const float* beta;
    float* y;             // (N,2H,2W,C)
    int N, H, W, C, relu;
    int x_bf16, y_bf16;   // bf16 storage mode: x / y hold bf16 (ConvArgs)
};

// four consecutive channels of an fp32 tensor, or of the same tensor stored as bf16 (exact widening)
__device__ __forceinline__ float4 ld4_f32_or_bf16(const float* base, size_t elem, bool b16) {
    if (!b16) return *reinterpret_cast<const float4*>(base + elem);
    const uint2 p = *reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned short*>(base) + elem);
    return make_float4(__builtin_bit_cast(float, p.x << 16), __builtin_bit_cast(float, p.x & 0xFFFF0000u),
                       __builtin_bit_cast(float, p.y << 16), __builtin_bit_cast(float, p.y & 0xFFFF0000u));
}

// the four channels of a tap on load (conv_common.hpp up2_tap)
__device__ __forceinline__ float4 na4(float4 v, const float4& al, const float4& be, bool norm, bool relu) {
    v.x = up2_tap(v.x, al.x, be.x, norm, relu); v.y = up2_tap(v.y, al.y, be.y, norm, relu);
    v.z = up2_tap(v.z, al.z, be.z, norm, relu); v.w = up2_tap(v.w, al.w, be.w, norm, relu);
    return v;
}

// grid = (chunks of one output row, 2H, N): row and image come from the block index, one 32-bit division per element
__global__ __launch_bounds__(256) void upsample2x_kernel(UpsampleArgs a) {
    const unsigned c4n = (unsigned)a.C >> 2;
    const int Ho = 2 * a.H, Wo = 2 * a.W;
    const int oy = blockIdx.y, n = blockIdx.z;
    const unsigned row4 = (unsigned)Wo * c4n;
    for (unsigned j = blockIdx.x * 256u + threadIdx.x; j < row4; j += gridDim.x * 256u) {
        const int ox = (int)(j / c4n);
        const int c = (int)(j - (unsigned)ox * c4n) * 4;
        const size_t i = ((size_t)n * Ho + oy) * row4 + j;
        int y0, y1, x0, x1;
        float wy0, wy1, wx0, wx1;
        up2_source(oy, a.H, y0, y1, wy0, wy1);
        up2_source(ox, a.W, x0, x1, wx0, wx1);
        const bool norm = a.alpha != nullptr;
        float4 al = make_float4(1.f, 1.f, 1.f, 1.f), be = make_float4(0.f, 0.f, 0.f, 0.f);
        if (norm) {
            al = *reinterpret_cast<const float4*>(a.alpha + (size_t)n * a.C + c);
            be = *reinterpret_cast<const float4*>(a.beta + (size_t)n * a.C + c);
        }
        const size_t base = ((size_t)n * a.H * a.W) * a.C + c;
        const bool xb = a.x_bf16 != 0;
        const float4 v00 = na4(ld4_f32_or_bf16(a.x, base + ((size_t)y0 * a.W + x0) * a.C, xb), al, be, norm, a.relu);
        const float4 v01 = na4(ld4_f32_or_bf16(a.x, base + ((size_t)y0 * a.W + x1) * a.C, xb), al, be, norm, a.relu);
        const float4 v10 = na4(ld4_f32_or_bf16(a.x, base + ((size_t)y1 * a.W + x0) * a.C, xb), al, be, norm, a.relu);
        const float4 v11 = na4(ld4_f32_or_bf16(a.x, base + ((size_t)y1 * a.W + x1) * a.C, xb), al, be, norm, a.relu);
        float4 o;
        o.x = up2_blend(v00.x, v01.x, v10.x, v11.x, wx0, wx1, wy0, wy1);
        o.y = up2_blend(v00.y, v01.y, v10.y, v11.y, wx0, wx1, wy0, wy1);
        o.z = up2_blend(v00.z, v01.z, v10.z, v11.z, wx0, wx1, wy0, wy1);
        o.w = up2_blend(v00.w, v01.w, v10.w, v11.w, wx0, wx1, wy0, wy1);
        if (a.y_bf16) {
            uint2 q;
            q.x = TSNET_CVT_PK_BF16(o.x, o.y);
            q.y = TSNET_CVT_PK_BF16(o.z, o.w);
            reinterpret_cast<uint2*>(a.y)[i] = q;
        } else {
            reinterpret_cast<float4*>(a.y)[i] = o;
        }
    }
}

// bf16 -> fp32 (debug accessor of the bf16-storage mode)
__global__ void bf16_widen_kernel(const unsigned short* __restrict__ x, float* __restrict__ y, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        y[i] = __builtin_bit_cast(float, (unsigned)x[i] << 16);
}

// ---------------------------------------------------------------------------------------------
// Stem input assembly: NCHW planes -> one NHWC tensor with Cp channels
//   [ img/255 (nimg) | lbl (L) | xx yy rr (if coords) | 0 ... ]   image index n = s*B + b.
struct PackArgs {
    const float* img[8];   // per source: (B,3,H,W) or null (label encoder input)
    const float* lbl[8];   // per source: (B,L,H,W)
    const float* coords;   // (H,W,3) table or null
    float* out;            // (S*B, H, W, Cp)
    int S, B, H, W, L, nimg, Cp;
    float img_div[8];      // per source: 255 (set_test_input's /255, TSNet.py:286) or 1 (use_prev: a frame already in [0,1], TSNet.py:269-276)
    unsigned* amax_out;    // null, or amax_out[image] <- max |packed value| of that image (float bits; operand scale of the fp16 x 2 stem)
};

// grid = (blocks per image, S * B images).  Eight channels at a time: their eight loads are issued TOGETHER -- each from a wave-uniform plane
// pointer picked by selects, a dummy address for a padding channel -- and the /255 follows in a second pass.  (Written as one branch per
// channel kind and element, the round-5 kernel compiled to eight dependent load -> branch -> load links per pixel: 39 us for the 12 source
// images of the headline forward, 1 TB/s.)
__global__ __launch_bounds__(256) void pack_input_kernel(PackArgs a) {
    const size_t HW = (size_t)a.H * a.W;
    const int creal = a.nimg + a.L + (a.coords ? 3 : 0);
    const int n = blockIdx.y;
    const int s = n / a.B, b = n - s * a.B;
    const float* const img_b = a.nimg ? a.img[s] + (size_t)b * a.nimg * HW : a.lbl[s];
    const float* const lbl_b = a.lbl[s] + (size_t)b * a.L * HW;
    const float* const dummy = a.lbl[s];                         // any readable address: the value is discarded
    const float div = a.img_div[s];
    float vmax = 0.f;
    for (size_t pix = (size_t)blockIdx.x * blockDim.x + threadIdx.x; pix < HW; pix += (size_t)gridDim.x * blockDim.x) {
        float* o = a.out + ((size_t)n * HW + pix) * a.Cp;
        for (int c0 = 0; c0 < a.Cp; c0 += 8) {
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {                        // every pointer / stride below is wave-uniform
                const int c = c0 + e;
                const bool is_img = c < a.nimg, is_lbl = !is_img && c < a.nimg + a.L, is_crd = !is_img && !is_lbl && c < creal;
                const float* p = is_img ? img_b + (size_t)c * HW : (is_lbl ? lbl_b + (size_t)(c - a.nimg) * HW : (is_crd ? a.coords + (c - a.nimg - a.L) : dummy));
                const size_t idx = is_crd ? pix * 3 : ((is_img || is_lbl) ? pix : 0);
                const float t = p[idx];
                v[e] = (is_img || is_lbl || is_crd) ? t : 0.f;
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if (c0 + e < a.nimg) v[e] = v[e] / div;          // set_test_input's /255 (TSNet.py:286): IEEE division, as torch divides
                vmax = __builtin_fmaxf(vmax, __builtin_fabsf(v[e]));
            }
            *reinterpret_cast<float4*>(o + c0) = make_float4(v[0], v[1], v[2], v[3]);          // Cp = 8 or a multiple of 16 (conv_cin_pad)
            *reinterpret_cast<float4*>(o + c0 + 4) = make_float4(v[4], v[5], v[6], v[7]);
        }
    }
    if (a.amax_out) tsnet_publish_amax(a.amax_out + n, vmax);      // per image; block-uniform branch: every thread of the workgroup arrives
}

// The same assembly from COMPACT inputs: one byte per value instead of four.  img[s] (B,3,H,W) bytes (planes B, G, R), lbl[s] (B,H,W) class
// indices, optionally bbox[s] (B,H,W) mask bytes.  The widening is the arithmetic the wide form went through on its way here -- (float)byte is
// exact, - mean and / div are the loader's and pack_input_kernel's own two fp32 operations, one-hot is a comparison (an index >= L: all
// zeros, as vl2ch's == ci) -- so `out` and `amax_out` carry the bits pack_input_kernel gives on the widened tensors.
struct PackU8Args {
    const unsigned char* img[8];    // per source: (B,3,H,W) or null (label encoder input)
    const unsigned char* lbl[8];    // per source: (B,H,W)
    const unsigned char* bbox[8];   // per source: (B,H,W), or all null
    const float* coords;            // (H,W,3) table or null
    float* out;                     // (S*B, H, W, Cp)
    float* bbox_out;                // mask of image (s, b) -> bbox_out[s * bbox_sstride + b * H*W ..] as (float)byte
    size_t bbox_sstride;
    int S, B, H, W, L, nimg, Cp;
    float img_div[8];
    float mean[3];                  // B, G, R
    unsigned* amax_out;
};

constexpr int kPackU8Px = 4;        // consecutive pixels of one lane: one 32-bit load per plane

// four consecutive bytes of a plane from pixel `pix` on (a multiple of 4) as one word, pixel i in bits 8i..: ONE 32-bit load where the
// address is 4-byte aligned and the four pixels exist, byte loads elsewhere (plane bases are odd when H*W is: the base of the plane is
// wave-uniform, so only the lane holding an image's tail diverges)
__device__ __forceinline__ unsigned pack_u8_ld4(const unsigned char* plane, size_t pix, int cnt) {
    const unsigned char* p = plane + pix;
    if (cnt == kPackU8Px && (reinterpret_cast<uintptr_t>(p) & 3u) == 0) return *reinterpret_cast<const unsigned*>(p);
    unsigned v = 0;
#pragma unroll
    for (int i = 0; i < kPackU8Px; ++i)
        if (i < cnt) v |= (unsigned)p[i] << (8 * i);
    return v;
}

// grid = (blocks per image, S * B images), a lane owns kPackU8Px consecutive pixels: 64 lanes read 256 consecutive bytes of a plane and
// write 4 * Cp consecutive floats each, as the float4 stores of pack_input_kernel.  Channel kinds are picked by selects on compile-time
// register names (no indexed register arrays).
__global__ __launch_bounds__(256) void pack_input_u8_kernel(PackU8Args a) {
    const size_t HW = (size_t)a.H * a.W;
    const int nl = a.nimg + a.L, creal = nl + (a.coords ? 3 : 0);
    const int n = blockIdx.y;
    const int s = n / a.B, b = n - s * a.B;
    const unsigned char* const lbl_b = a.lbl[s] + (size_t)b * HW;
    const unsigned char* const img_b = a.nimg ? a.img[s] + (size_t)b * 3 * HW : lbl_b;      // (nimg = 0: never read)
    const unsigned char* const box_b = a.bbox[s] ? a.bbox[s] + (size_t)b * HW : nullptr;
    float* const box_o = a.bbox_out + (size_t)s * a.bbox_sstride + (size_t)b * HW;
    const float div = a.img_div[s];
    const size_t quads = (HW + kPackU8Px - 1) / kPackU8Px;
    float vmax = 0.f;
    for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (size_t)gridDim.x * blockDim.x) {
        const size_t pix = q * kPackU8Px;
        const int cnt = HW - pix < (size_t)kPackU8Px ? (int)(HW - pix) : kPackU8Px;
        unsigned wi0 = 0, wi1 = 0, wi2 = 0;
        if (a.nimg) { wi0 = pack_u8_ld4(img_b, pix, cnt); wi1 = pack_u8_ld4(img_b + HW, pix, cnt); wi2 = pack_u8_ld4(img_b + 2 * HW, pix, cnt); }
        const unsigned wl = pack_u8_ld4(lbl_b, pix, cnt);
        float4 cr0 = make_float4(0.f, 0.f, 0.f, 0.f), cr1 = cr0, cr2 = cr0;                  // xx yy rr of the four pixels, 12 consecutive floats
        if (a.coords) {
            const float* cp = a.coords + pix * 3;                                             // 48 q bytes: 16-byte aligned
            if (cnt == kPackU8Px) {
                cr0 = *reinterpret_cast<const float4*>(cp); cr1 = *reinterpret_cast<const float4*>(cp + 4); cr2 = *reinterpret_cast<const float4*>(cp + 8);
            } else {
                float t[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                for (int i = 0; i < 9; ++i) if (i < cnt * 3) t[i] = cp[i];
                cr0 = make_float4(t[0], t[1], t[2], t[3]); cr1 = make_float4(t[4], t[5], t[6], t[7]); cr2 = make_float4(t[8], 0.f, 0.f, 0.f);
            }
        }
        if (box_b) {
            const unsigned wb = pack_u8_ld4(box_b, pix, cnt);
            float* bo = box_o + pix;
            if (cnt == kPackU8Px && (reinterpret_cast<uintptr_t>(bo) & 15u) == 0) {
                *reinterpret_cast<float4*>(bo) = make_float4((float)(wb & 255u), (float)((wb >> 8) & 255u), (float)((wb >> 16) & 255u), (float)(wb >> 24));
            } else {
#pragma unroll
                for (int i = 0; i < kPackU8Px; ++i) if (i < cnt) bo[i] = (float)((wb >> (8 * i)) & 255u);
            }
        }
        const float crd[12] = {cr0.x, cr0.y, cr0.z, cr0.w, cr1.x, cr1.y, cr1.z, cr1.w, cr2.x, cr2.y, cr2.z, cr2.w};
#pragma unroll
        for (int p = 0; p < kPackU8Px; ++p) {
            if (p < cnt) {
                // set_test_input's /255 (TSNet.py:286) on the loader's byte - IMG_MEAN: two fp32 operations, IEEE division
                const float i0 = ((float)((wi0 >> (8 * p)) & 255u) - a.mean[0]) / div;
                const float i1 = ((float)((wi1 >> (8 * p)) & 255u) - a.mean[1]) / div;
                const float i2 = ((float)((wi2 >> (8 * p)) & 255u) - a.mean[2]) / div;
                const int cls = (int)((wl >> (8 * p)) & 255u) + a.nimg;                       // the channel that is 1
                const float x0 = crd[3 * p], x1 = crd[3 * p + 1], x2 = crd[3 * p + 2];
                float* o = a.out + ((size_t)n * HW + pix + p) * a.Cp;
                for (int c0 = 0; c0 < a.Cp; c0 += 4) {                                        // Cp = 8 or a multiple of 16 (conv_cin_pad)
                    float v[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int c = c0 + e, k = c - nl;
                        const float im = c == 0 ? i0 : (c == 1 ? i1 : i2);
                        const float cd = k == 0 ? x0 : (k == 1 ? x1 : x2);
                        v[e] = c < a.nimg ? im : (c < nl ? (c == cls ? 1.f : 0.f) : (c < creal ? cd : 0.f));
                        vmax = __builtin_fmaxf(vmax, __builtin_fabsf(v[e]));
                    }
                    *reinterpret_cast<float4*>(o + c0) = make_float4(v[0], v[1], v[2], v[3]);
                }
            }
        }
    }
    if (a.amax_out) tsnet_publish_amax(a.amax_out + n, vmax);      // per image; block-uniform branch: every thread of the workgroup arrives
}

}  // namespace tsnet
