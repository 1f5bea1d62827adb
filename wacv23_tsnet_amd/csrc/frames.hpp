// frames.hpp -- the image side of the reference's data loaders on the device: decoded video frames -> the generator's image tensors.
// Replaces, per frame, the host work of
//   * FaceDatasetTest.__getitem__ (dataset/dataset_video_face.py:318-329, 391-401): self.crop + Image.resize((256, 256)) + RGB -> BGR - IMG_MEAN
//   * PoseDatasetTestVideo.__getitem__ (dataset/dataset_video_pose.py:346, 412-417, 450-457): crop + Image.resize((128, 256)) + resize_square's
//     black bars + RGB -> BGR - IMG_MEAN
// Image.resize's default filter is bicubic, and Pillow's 8-bit resampler (libImaging/Resample.c) is integer arithmetic once its coefficient
// tables exist: per axis, weights bicubic((j + first - center + 0.5) / filterscale) normalised in double and rounded to 22 fractional bits;
// a pass is 2^21 + sum(pixel * k) in int32, shifted down by 22 and clamped to a byte.  The horizontal pass runs first and ROUNDS TO BYTES, the
// vertical pass reads those bytes; a pass along an axis that keeps its size is skipped.  The tables are built on the HOST (bicubic_table below,
// in Pillow's operation order; engine.cpp is compiled without fp contraction) and the kernel does the integer work, so the result EQUALS
// frame.crop(box).resize(size) byte for byte (tests/test_frames.py: live Pillow, and the stored loader outputs of the g10 goldens).
// Image.crop semantics: the box may leave the frame, the part outside reads as 0; the resampling window clamps to the CROP, never to the frame.
// paste.hpp, the way back, shares the vertical pass (fr_vpass) and the window of rows a tile keeps (fr_row_window) with the loader: one spelling.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

namespace tsnet {

constexpr int kBicubicBits = 22;         // PRECISION_BITS of Pillow's 8 bits-per-channel resampler

inline double pil_bicubic(double x) {    // bicubic_filter, a = -0.5
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

// ksize of precompute_coeffs: the row stride of the coefficient table
inline int bicubic_taps(int n_in, int n_out) {
    const double scale = (double)n_in / (double)n_out, fs = scale < 1.0 ? 1.0 : scale;
    return (int)std::ceil(2.0 * fs) * 2 + 1;
}

// precompute_coeffs + normalize_coeffs_8bpc for the whole axis (box = the full input): first[n_out], count[n_out], coef[n_out * taps] (unused
// taps zero).  HOST.
inline void bicubic_table(int n_in, int n_out, int* first, int* count, int* coef) {
    const double scale = (double)n_in / (double)n_out, fs = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * fs, ss = 1.0 / fs;
    const int taps = (int)std::ceil(support) * 2 + 1;
    std::vector<double> w((size_t)taps);
    for (int o = 0; o < n_out; ++o) {
        const double center = (o + 0.5) * scale;
        int lo = (int)(center - support + 0.5), hi = (int)(center + support + 0.5);
        if (lo < 0) lo = 0;
        if (hi > n_in) hi = n_in;
        const int n = hi - lo;
        double ww = 0.0;
        for (int j = 0; j < n; ++j) { w[j] = pil_bicubic((j + lo - center + 0.5) * ss); ww += w[j]; }
        int* k = coef + (size_t)o * taps;
        for (int j = 0; j < taps; ++j) {
            if (j >= n) { k[j] = 0; continue; }
            const double v = ww != 0.0 ? w[j] / ww : w[j];
            k[j] = v < 0 ? (int)(-0.5 + v * (double)(1 << kBicubicBits)) : (int)(0.5 + v * (double)(1 << kBicubicBits));
        }
        first[o] = lo; count[o] = n;
    }
}

constexpr int kFrTileW = 64;             // output columns of a workgroup's tile
constexpr int kFrTileH = 32;             // output rows of a tile, at most (the launcher lowers it for steep vertical reductions)
constexpr int kFrRows = 112;             // rows of the horizontal pass a tile keeps in LDS: 780 -> 256 with 32 output rows needs 108
constexpr int kFrRowBytes = 3 * kFrTileW;

// Rows of the horizontal pass that `th` consecutive output rows read, at most: first > center - support - 0.5, last <= center + support + 0.5
inline int frames_row_span(int n_in, int n_out, int th) {
    if (n_in == n_out) return th;
    const double scale = (double)n_in / (double)n_out, fs = scale < 1.0 ? 1.0 : scale;
    return (int)((th - 1) * scale + 4.0 * fs + 1.0) + 1;
}

struct FrameArgs {
    const unsigned char* frames;         // (F, h, w, 3) RGB
    float* out;                          // (F, 3, OH, OW), planes B, G, R -- floats (byte - mean), or the bytes themselves (prepare_frames_body<true>)
    const int *xfirst, *xcount, *xcoef, *yfirst, *ycount, *ycoef;
    int h, w, bx0, by0, cw, ch;          // frame size; the crop box's corner in frame coordinates and its size
    int ow, oh, xtaps, ytaps, pad_top, pad_left, OH, OW, th;
    float mean[3];                       // B, G, R
};

// |k| <= 2^22 and a pixel <= 255: both fit v_mad_i32_i24.  The shift pair is the identity on such k and lets the compiler prove it.
__device__ __forceinline__ int fr_k24(int k) { return (k << 8) >> 8; }
__device__ __forceinline__ int fr_clip8(int acc) { const int v = acc >> kBicubicBits; return v < 0 ? 0 : (v > 255 ? 255 : v); }

// The rows of the horizontal pass a tile keeps in LDS for its resized rows [oyA, oyB), oyA < oyB: source rows [ybase, ybase + rows) of a crop
// ch rows tall, from the vertical tables (not read when skipy), never more than kFrRows.  cap: rows also end at the crop's last row (paste.hpp,
// whose source rows are read without a check against the image).  Shared by prepare_frames_body and paste.hpp's paste_frames_body.
__device__ __forceinline__ void fr_row_window(const int* yfirst, const int* ycount, int ch, int oyA, int oyB, bool skipy, bool cap, int& ybase, int& rows) {
    if (skipy) { ybase = oyA; rows = oyB - oyA; }
    else {
        ybase = yfirst[oyA];
        ybase = ybase < 0 ? 0 : (ybase > ch ? ch : ybase);
        int yend = yfirst[oyB - 1] + ycount[oyB - 1];
        yend = yend > ch ? ch : yend;
        rows = yend - ybase;
    }
    if (cap && ybase + rows > ch) rows = ch - ybase;
    rows = rows < 0 ? 0 : (rows > kFrRows ? kFrRows : rows);
}

// One output byte of the vertical pass: resized row oy (0 <= oy < oh) of an LDS column whose rows lie `stride` bytes apart; the column holds
// `rows` rows of the horizontal pass, the first of them source row ybase (fr_row_window).  Shared by prepare_frames_body and paste.hpp's
// paste_frames_body.  The range test of the skipy branch is the paste's; the loader read col[(oy - ybase) * stride] without one, and for it the
// test is always true (rows = oyB - oyA <= th there and oy lies in [oyA, oyB)): the same bytes, five more instructions per loader kernel.
__device__ __forceinline__ int fr_vpass(const int* yfirst, const int* ycount, const int* ycoef, int ytaps, const unsigned char* col, int stride, int oy,
                                        int ybase, int rows, bool skipy) {
    if (skipy) { const int rr = oy - ybase; return rr >= 0 && rr < rows ? col[rr * stride] : 0; }
    const int first = yfirst[oy] - ybase;
    int cnt = ycount[oy];
    cnt = cnt > ytaps ? ytaps : cnt;
    const int* k = ycoef + (size_t)oy * ytaps;
    int acc = 1 << (kBicubicBits - 1);
    for (int j = 0; j < cnt; ++j) {
        const int rr = first + j;
        if (rr >= 0 && rr < rows) acc += (int)col[rr * stride] * fr_k24(k[j]);
    }
    return fr_clip8(acc);
}

// grid = (ceil(OW / 64), ceil(OH / th), F), 256 threads.  A workgroup owns th x 64 pixels of one frame's PADDED output.  It runs the horizontal
// pass for the crop rows its output rows read, straight from the frame (the taps of neighbouring lanes overlap: the vector L1 serves them) into
// LDS as bytes, plane by plane; then the vertical pass from LDS, and stores fp32 rows of 64 consecutive floats per plane.  The byte image
// between the passes never reaches memory.  Every index that comes from a table is range-checked: a bad table gives wrong pixels, not a fault.
// U8: store the resized byte itself (a.out holds bytes, a.mean is not read) -- the compact image of pack_input_u8_kernel, which subtracts the mean
// on load: (float)byte - mean is then the float store below, bit for bit.
// mean: a.mean where the kernel's arguments hold it (the per-frame-box kernels run the body on a copy of theirs, and a plane-indexed array in a
// copy would live in scratch).
template <bool U8>
__device__ __forceinline__ void prepare_frames_body(const FrameArgs& a, const float* mean) {
    __shared__ unsigned char hbuf[kFrRows * kFrRowBytes];
    const int tid = threadIdx.x;
    const int X0 = blockIdx.x * kFrTileW, Y0 = blockIdx.y * a.th, f = blockIdx.z;
    // the tile's share of the resized image: output rows [oyA, oyB), tile-local columns [lxA, lxB)
    const int oyA = Y0 - a.pad_top < 0 ? 0 : Y0 - a.pad_top;
    const int oyB = Y0 + a.th - a.pad_top > a.oh ? a.oh : Y0 + a.th - a.pad_top;
    const int lxA = a.pad_left - X0 < 0 ? 0 : a.pad_left - X0;
    const int lxB = a.pad_left + a.ow - X0 > kFrTileW ? kFrTileW : a.pad_left + a.ow - X0;
    const bool content = oyA < oyB && lxA < lxB;                  // uniform over the workgroup
    const bool skipx = a.ow == a.cw, skipy = a.oh == a.ch;
    int ybase = 0, rows = 0;
    if (content) {
        fr_row_window(a.yfirst, a.ycount, a.ch, oyA, oyB, skipy, false, ybase, rows);
        const unsigned char* img = a.frames + (size_t)f * a.h * a.w * 3;
        for (int i = tid; i < rows * kFrRowBytes; i += blockDim.x) {
            const int r = i / kFrRowBytes, e = i - r * kFrRowBytes, c = e / kFrTileW, lx = e - c * kFrTileW;
            const int ox = X0 + lx - a.pad_left, fy = a.by0 + ybase + r;
            int v = 0;
            if (lx >= lxA && lx < lxB && fy >= 0 && fy < a.h) {
                const unsigned char* row = img + (size_t)fy * a.w * 3 + c;
                if (skipx) {
                    const int fx = a.bx0 + ox;
                    v = (fx >= 0 && fx < a.w) ? row[fx * 3] : 0;
                } else {
                    const int first = a.xfirst[ox];
                    int cnt = a.xcount[ox];
                    cnt = cnt > a.xtaps ? a.xtaps : cnt;
                    const int* k = a.xcoef + (size_t)ox * a.xtaps;
                    int acc = 1 << (kBicubicBits - 1);
                    for (int j = 0; j < cnt; ++j) {
                        const int cx = first + j, fx = a.bx0 + cx;
                        if (cx >= 0 && cx < a.cw && fx >= 0 && fx < a.w) acc += (int)row[fx * 3] * fr_k24(k[j]);
                    }
                    v = fr_clip8(acc);
                }
            }
            hbuf[i] = (unsigned char)v;
        }
    }
    __syncthreads();
    const int tile_rows = a.OH - Y0 < a.th ? a.OH - Y0 : a.th;
    for (int i = tid; i < tile_rows * kFrRowBytes; i += blockDim.x) {
        const int ly = i / kFrRowBytes, e = i - ly * kFrRowBytes, c = e / kFrTileW, lx = e - c * kFrTileW;
        const int X = X0 + lx, Y = Y0 + ly, oy = Y - a.pad_top;
        if (X >= a.OW) continue;
        int v = 0;                                                // the bars of resize_square: byte 0
        if (content && oy >= oyA && oy < oyB && lx >= lxA && lx < lxB)
            v = fr_vpass(a.yfirst, a.ycount, a.ycoef, a.ytaps, hbuf + c * kFrTileW + lx, kFrRowBytes, oy, ybase, rows, skipy);
        const int p = 2 - c;                                      // RGB -> BGR
        const size_t o = (((size_t)f * 3 + p) * a.OH + Y) * a.OW + X;
        if (U8) reinterpret_cast<unsigned char*>(a.out)[o] = (unsigned char)v;
        else a.out[o] = (float)v - mean[p];
    }
}

__global__ __launch_bounds__(256) void prepare_frames_kernel(FrameArgs a) { prepare_frames_body<false>(a, a.mean); }
__global__ __launch_bounds__(256) void prepare_frames_u8_kernel(FrameArgs a) { prepare_frames_body<true>(a, a.mean); }

// ---------------------------------------------------------------------------------------------------------------- a box per frame
// FaceDatasetTest(fix_crop_pos=False) crops every frame by the box of its own landmarks (dataset/dataset_video_face.py:303-308, 317-320).  The box,
// and with it the coefficient tables, then belongs to the frame: a launch takes (F, 8) ints, one row per frame,
//   {x0, y0, x1, y1, xoff, xtaps, yoff, ytaps}
// and one POOL of tables; xoff / yoff are the offsets, in ints, of that axis' table inside the pool, where it lies as
// first[n_out] | count[n_out] | coef[n_out * taps] (-1: the axis keeps its size, no table).  The table of a size pair is the single-box table of
// that pair and the passes are the body above, so frame f of a launch has the bytes of the single-box kernel on frame f with box f.
constexpr int kFrDesc = 8;               // ints of a frame's descriptor
constexpr int kFrBoxMax = 1 << 24;       // what the kernels accept as a box size or (paste) corner; the launchers stop at 10^6

// The three tables of an axis from its pool offset, or false when they do not lie inside the pool.
__device__ __forceinline__ bool fr_pool_axis(const int* pool, int pool_len, int off, int n_out, int taps, const int*& first, const int*& count, const int*& coef) {
    if (off < 0 || taps < 1 || (long long)off + (long long)n_out * (2 + (long long)taps) > (long long)pool_len) return false;
    first = pool + off; count = first + n_out; coef = count + n_out;
    return true;
}

struct FrameBoxArgs {
    FrameArgs g;                         // what a launch fixes: frames, out, the output geometry, th, mean; its tables and box are not read
    const int* desc;                     // (F, kFrDesc) DEVICE
    const int* pool;
    int pool_len;
};

// The grid and the body of prepare_frames_body; the frame's descriptor is read once, through an address that depends on blockIdx.z alone (scalar
// loads), and everything taken from it is range-checked before the body sees it: a bad descriptor gives a black frame, not an access outside the
// pool or the frames (the body checks every frame read against h, w).
template <bool U8>
__device__ __forceinline__ void prepare_frames_boxes_body(const FrameBoxArgs& b) {
    const int* d = b.desc + (size_t)blockIdx.z * kFrDesc;
    FrameArgs a = b.g;
    const int x0 = d[0], y0 = d[1];
    a.cw = (int)((unsigned)d[2] - (unsigned)x0); a.ch = (int)((unsigned)d[3] - (unsigned)y0);
    // a box that starts below -2^24 (it is at most 2^24 wide) or beyond 2^30 (h * w * 3 < 2^31) lies outside the frame: clamped, it reads the
    // same zeros, and bx0 + cx cannot overflow
    a.bx0 = x0 < -kFrBoxMax ? -kFrBoxMax : (x0 > (1 << 30) ? (1 << 30) : x0);
    a.by0 = y0 < -kFrBoxMax ? -kFrBoxMax : (y0 > (1 << 30) ? (1 << 30) : y0);
    a.xtaps = d[5]; a.ytaps = d[7];
    bool ok = a.cw >= 1 && a.ch >= 1 && a.cw <= kFrBoxMax && a.ch <= kFrBoxMax;
    if (ok && a.ow != a.cw) ok = fr_pool_axis(b.pool, b.pool_len, d[4], a.ow, a.xtaps, a.xfirst, a.xcount, a.xcoef);
    if (ok && a.oh != a.ch) ok = fr_pool_axis(b.pool, b.pool_len, d[6], a.oh, a.ytaps, a.yfirst, a.ycount, a.ycoef);
    if (!ok) { a.ow = 0; a.oh = 0; }                              // no content: the body stores byte 0 everywhere and reads no table
    prepare_frames_body<U8>(a, b.g.mean);
}

__global__ __launch_bounds__(256) void prepare_frames_boxes_kernel(FrameBoxArgs b) { prepare_frames_boxes_body<false>(b); }
__global__ __launch_bounds__(256) void prepare_frames_boxes_u8_kernel(FrameBoxArgs b) { prepare_frames_boxes_body<true>(b); }

}  // namespace tsnet
