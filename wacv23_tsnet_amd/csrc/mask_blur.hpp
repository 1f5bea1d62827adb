// mask_blur.hpp -- feathered paste masks on the device: Pillow's Image.filter(ImageFilter.GaussianBlur(r)) on an "L" image, byte for byte.
// Pillow's Gaussian blur (libImaging/BoxBlur.c) is kMbPasses = 3 passes of an extended box blur per axis in 32-bit integers, each pass rounded
// to bytes, the rows first and then the columns.  The contract, restated in tests/feather_cases.py:
//   1. the box radius R of a blur radius r, in FLOAT arithmetic (mb_box_radius; double arithmetic gives other bytes at r = 1 and r = 0.3);
//   2. per axis: radius = (int)R, ww = (uint32)((float)(1 << 24) / (R * 2 + 1)), fw = ((1 << 24) - (2 radius + 1) ww) / 2;
//   3. one pass along a line in[0 .. n), clamp replicating the end pixels (a radius larger than the line is legal):
//        acc = sum_{d = -radius .. radius} in[clamp(x + d)],  far = in[clamp(x - radius - 1)] + in[clamp(x + radius + 1)],
//        out[x] = (uint8)((acc ww + far fw + (1 << 23)) >> 24)            -- nothing overflows 32 bits;
//   4. an axis whose radius is 0 is skipped; both 0 is a copy.
// An integer sum has one value in any order, so the running accumulator below equals Pillow exactly.
//
// One body serves both axes.  A workgroup owns kMbLines = 64 lines of one frame -- 64 rows held whole, or a tile of 64 columns as high as the
// image -- in LDS as bytes, position-major: byte (line l, position p) at p * 64 + (l ^ swizzle(p)).  One lane of the first wavefront walks one
// line with Pillow's running accumulator (two LDS reads and one write per pixel whatever the radius; the first window costs at most n reads),
// all three passes between two LDS buffers with a barrier after each.  At a fixed position the 64 lanes touch the 64 bytes of 16 consecutive
// dwords: no bank conflict.  The swizzle moves a line by whole dwords ((p / 4) % 16 of them), which keeps that property and spreads the
// TRANSPOSING accesses of the row form -- lanes over 64 consecutive positions of one row, 64 bytes apart without it (banks 0, 16, 32, 48 only) --
// over all 64 banks.  Global loads and stores run with the lanes along x in both forms: a wavefront touches 64 consecutive bytes.
// Two buffers of kMbMaxSide * 64 bytes are the 64 KiB a workgroup may declare; kMbMaxSide = 512 is the longest line, and the launcher refuses a
// longer side by that name before anything is launched.
// The source is a byte image, optionally binarised (every non-zero byte counts as 255: the engine's 0 / 1 bbox masks), or no image at all: the
// indicator of a rectangle, 255 inside and 0 outside, formed while the tile is filled.  Plain vector loads and stores, no atomics.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace tsnet {

constexpr int kMbLines = 64;             // lines of a tile: the lanes of one wavefront
constexpr int kMbMaxSide = 512;          // the longest line a tile holds: the largest H and W of tsnet_blur_mask
constexpr int kMbPasses = 3;             // Pillow's GaussianBlur: three box passes per axis
constexpr float kMbMaxRadius = 4096.f;   // blur radii beyond this are refused (the window sum of a pass stays far inside 32 bits)

// HOST.  Pillow's _gaussian_blur_radius, operation for operation: floats, with the doubles C's promotion rules put inside sqrt and floor.
inline float mb_box_radius(float radius, int passes) {
    float sigma2 = radius * radius / passes;
    float L = sqrt(12.0 * sigma2 + 1.0);
    float l = floor((L - 1.0) / 2.0);
    float a = (2 * l + 1) * (l * (l + 1) - 3 * sigma2);
    a /= 6 * (sigma2 - (l + 1) * (l + 1));
    return l + a;
}

// HOST.  ImagingLineBoxBlur's constants of a box radius R
inline void mb_line_constants(float R, int& radius, unsigned& ww, unsigned& fw) {
    radius = (int)R;
    ww = (unsigned)((float)(1u << 24) / (R * 2 + 1));
    fw = ((1u << 24) - (unsigned)(radius * 2 + 1) * ww) / 2;
}

struct MaskBlurArgs {
    const unsigned char* in;             // (F, H, W), or null: the indicator of the rectangle
    unsigned char* out;                  // (F, H, W)
    int H, W;
    int x0, y0, x1, y1;                  // the rectangle (in == null)
    int binary;                          // non-zero source bytes count as 255
    int passes;                          // 0: the tile is copied (and binarised / formed from the rectangle)
    int radius;
    unsigned ww, fw;
};

__device__ __forceinline__ int mb_at(int line, int p) { return p * kMbLines + (line ^ (((p >> 1) & 15) << 2)); }

// One pass along line `line` of n bytes, src -> dst (two LDS buffers that do not overlap: the loads of later pixels may pass the stores).
__device__ __forceinline__ void mb_line_pass(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, int line, int n, int radius,
                                             unsigned ww, unsigned fw) {
    const int last = n - 1;
    const unsigned first_px = src[mb_at(line, 0)], last_px = src[mb_at(line, last)];
    const int m = radius < last ? radius : last;
    unsigned acc = (unsigned)(radius + 1) * first_px + (unsigned)(radius - m) * last_px;       // the clamped ends of the window at x = 0
    for (int d = 1; d <= m; ++d) acc += src[mb_at(line, d)];
    unsigned left = first_px;                                                               // in[clamp(x - radius - 1)]
    for (int x = 0; x < n; ++x) {
        const int pl = x + radius + 1, pn = x - radius;
        const unsigned lead = pl > last ? last_px : src[mb_at(line, pl)];
        const unsigned next = pn < 0 ? first_px : (pn > last ? last_px : src[mb_at(line, pn)]);
        dst[mb_at(line, x)] = (unsigned char)((acc * ww + (left + lead) * fw + (1u << 23)) >> 24);
        acc += lead - next;                                                                  // the window of x + 1
        left = next;
    }
}

// grid = (ceil(lines / 64), F), 256 threads; ROWS: the lines are rows (n = W, H of them), else columns (n = H, W of them).
template <bool ROWS>
__device__ __forceinline__ void mask_blur_body(const MaskBlurArgs& a) {
    __shared__ unsigned char buf[2][kMbMaxSide * kMbLines];
    const int tid = threadIdx.x, q = tid & (kMbLines - 1), s = tid >> 6, step = blockDim.x >> 6;
    const int f = blockIdx.y, l0 = blockIdx.x * kMbLines;
    const int n = ROWS ? a.W : a.H, lines = ROWS ? a.H : a.W;
    const int nl = lines - l0 > kMbLines ? kMbLines : lines - l0;
    if (nl <= 0 || n < 1 || n > kMbMaxSide) return;                      // uniform over the workgroup; the launcher rules it out
    const size_t base = (size_t)f * a.H * a.W;
    // the lanes of a wavefront lie along x: positions of one row (ROWS), or the tile's columns at one y
    const int lcount = ROWS ? nl : n, xcount = ROWS ? n : nl;
    for (int j = s; j < lcount; j += step)
        for (int i = q; i < xcount; i += kMbLines) {
            const int line = ROWS ? j : i, p = ROWS ? i : j;
            const int y = ROWS ? l0 + line : p, x = ROWS ? p : l0 + line;
            int v;
            if (a.in) {
                v = a.in[base + (size_t)y * a.W + x];
                if (a.binary && v) v = 255;
            } else {
                v = (x >= a.x0 && x < a.x1 && y >= a.y0 && y < a.y1) ? 255 : 0;
            }
            buf[0][mb_at(line, p)] = (unsigned char)v;
        }
    __syncthreads();
    int cur = 0;
    for (int pass = 0; pass < a.passes; ++pass) {                       // uniform: every thread meets every barrier
        if (tid < nl) mb_line_pass(buf[cur], buf[cur ^ 1], tid, n, a.radius, a.ww, a.fw);
        cur ^= 1;
        __syncthreads();
    }
    for (int j = s; j < lcount; j += step)
        for (int i = q; i < xcount; i += kMbLines) {
            const int line = ROWS ? j : i, p = ROWS ? i : j;
            const int y = ROWS ? l0 + line : p, x = ROWS ? p : l0 + line;
            a.out[base + (size_t)y * a.W + x] = buf[cur][mb_at(line, p)];
        }
}

__global__ __launch_bounds__(256) void mask_blur_rows_kernel(MaskBlurArgs a) { mask_blur_body<true>(a); }
__global__ __launch_bounds__(256) void mask_blur_cols_kernel(MaskBlurArgs a) { mask_blur_body<false>(a); }

}  // namespace tsnet
