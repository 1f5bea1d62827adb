// paste.hpp -- the way back of frames.hpp: generated frames -> the full video frames they were cropped from, on the device.  Per frame f, in
// Pillow's terms (default bicubic filter, 8 bits per channel):
//   g = Image.fromarray(gen[f]).crop((sx0, sy0, sx1, sy1)).resize((x1 - x0, y1 - y0))
//   m = None if mask is None else Image.fromarray(mask[f], "L").crop((sx0, sy0, sx1, sy1)).resize((x1 - x0, y1 - y0))
//   frame_f.paste(g, (x0, y0), m)                  # in place; the box may leave the frame
// Three Pillow behaviours are the contract (tests/paste_cases.py restates them in numpy and checks live Pillow against the restatement):
//   * crop, then resize: the resampling window clamps to the source rectangle, never to the rest of gen;
//   * clipped paste: exactly box ∩ frame is written, destination pixel (X, Y) gets resized pixel (X - x0, Y - y0); a box outside writes nothing;
//   * masked paste (paste_mask_L), per byte with a = frame, b = resized gen, m = resized mask: t = b * m + a * (255 - m) + 128,
//     out = (t + (t >> 8)) >> 8.  The mask is one channel through the same tables and rounding as a colour channel.
// The resampler is frames.hpp's: integer passes on tsnet_bicubic_table's tables, the horizontal one first and ROUNDED TO BYTES, a pass along an
// axis that keeps its size skipped.  The vertical pass and the window of source rows a tile keeps are frames.hpp's own code, fr_vpass and
// fr_row_window, called from both bodies.  The horizontal pass is this file's (paste_hpass): it reads a rectangle the launcher proved inside gen
// at a run-time pixel stride, where the loader checks every read against the frame and returns zeros outside it -- one function for both would
// carry the other's checks into each kernel.
#pragma once
#include <hip/hip_runtime.h>

#include "frames.hpp"

namespace tsnet {

struct PasteArgs {
    const unsigned char* gen;            // (F, GH, GW, 3) RGB
    const unsigned char* mask;           // (F, GH, GW) or null (paste_frames_body<false>)
    unsigned char* frames;               // (F, h, w, 3) RGB, written in place inside box ∩ frame
    const int *xfirst, *xcount, *xcoef, *yfirst, *ycount, *ycoef;
    int GH, GW, sx0, sy0, cw, ch;        // gen's size; the source rectangle's corner and size
    int h, w, x0, y0, ow, oh;            // frame size; the box's corner in frame coordinates and its size (= the resized image's)
    int rx0, ry0, rx1, ry1;              // box ∩ frame, not empty
    int xtaps, ytaps, th;
};

// One output byte of the horizontal pass: resized column ox (0 <= ox < ow) of a source row whose pixels lie `stride` bytes apart.
__device__ __forceinline__ int paste_hpass(const PasteArgs& a, const unsigned char* row, int stride, int ox, bool skipx) {
    if (skipx) return ox < a.cw ? row[ox * stride] : 0;
    const int first = a.xfirst[ox];
    int cnt = a.xcount[ox];
    cnt = cnt > a.xtaps ? a.xtaps : cnt;
    const int* k = a.xcoef + (size_t)ox * a.xtaps;
    int acc = 1 << (kBicubicBits - 1);
    for (int j = 0; j < cnt; ++j) {
        const int cx = first + j;
        if (cx >= 0 && cx < a.cw) acc += (int)row[cx * stride] * fr_k24(k[j]);
    }
    return fr_clip8(acc);
}

// grid = (ceil(region width / 64), ceil(region height / th), F), 256 threads, region = box ∩ frame.  A workgroup owns th x 64 pixels of one
// frame's region.  It runs the horizontal pass for the source rows its output rows read, from gen (and mask) into LDS as bytes, INTERLEAVED
// as the frame is (byte e of a row: pixel e / 3, channel e % 3), the mask's 64 bytes per row behind the colour rows; then the vertical pass
// from LDS with the lanes laid over the 192 consecutive bytes of a tile row, so that a wavefront's stores (and, with a mask, its loads of the
// bytes it overwrites) are consecutive addresses.  No workgroup reads frame bytes another writes: in place is safe.  Every index that comes
// from a table is range-checked -- a bad table gives wrong pixels, not an access outside gen -- and every store is checked against the frame.
template <bool MASK>
__device__ __forceinline__ void paste_frames_body(const PasteArgs& a) {
    __shared__ unsigned char hbuf[kFrRows * (kFrRowBytes + (MASK ? kFrTileW : 0))];
    unsigned char* const mbuf = hbuf + kFrRows * kFrRowBytes;
    const int tid = threadIdx.x;
    const int X0 = a.rx0 + blockIdx.x * kFrTileW, Y0 = a.ry0 + blockIdx.y * a.th, f = blockIdx.z;
    const int nx = a.rx1 - X0 > kFrTileW ? kFrTileW : a.rx1 - X0;          // the tile's columns and rows inside the region
    const int ny = a.ry1 - Y0 > a.th ? a.th : a.ry1 - Y0;
    const int oyA = Y0 - a.y0 < 0 ? 0 : Y0 - a.y0;                          // resized rows [oyA, oyB), resized columns from oxA on
    const int oyB = Y0 + ny - a.y0 > a.oh ? a.oh : Y0 + ny - a.y0;
    const int oxA = X0 - a.x0;
    if (nx <= 0 || oyA >= oyB || oxA < 0 || oxA + nx > a.ow) return;         // uniform over the workgroup; the launcher rules it out
    const bool skipx = a.ow == a.cw, skipy = a.oh == a.ch;
    int ybase, rows;
    fr_row_window(a.yfirst, a.ycount, a.ch, oyA, oyB, skipy, true, ybase, rows);
    // source row ybase + r of the rectangle, 0 <= ybase + r < ch: inside gen, the launcher checked the rectangle
    const size_t src0 = ((size_t)f * a.GH + a.sy0 + ybase) * a.GW + a.sx0;
    for (int i = tid; i < rows * kFrRowBytes; i += blockDim.x) {
        const int r = i / kFrRowBytes, e = i - r * kFrRowBytes, lx = e / 3, c = e - lx * 3;
        int v = 0;
        if (lx < nx) v = paste_hpass(a, a.gen + (src0 + (size_t)r * a.GW) * 3 + c, 3, oxA + lx, skipx);
        hbuf[i] = (unsigned char)v;
    }
    if (MASK) {
        for (int i = tid; i < rows * kFrTileW; i += blockDim.x) {
            const int r = i / kFrTileW, lx = i - r * kFrTileW;
            int v = 0;
            if (lx < nx) v = paste_hpass(a, a.mask + src0 + (size_t)r * a.GW, 1, oxA + lx, skipx);
            mbuf[i] = (unsigned char)v;
        }
    }
    __syncthreads();
    unsigned char* img = a.frames + (size_t)f * a.h * a.w * 3;
    for (int i = tid; i < ny * kFrRowBytes; i += blockDim.x) {
        const int ly = i / kFrRowBytes, e = i - ly * kFrRowBytes, lx = e / 3;
        const int X = X0 + lx, Y = Y0 + ly, oy = Y - a.y0;
        if (lx >= nx || X < 0 || X >= a.w || Y < 0 || Y >= a.h || oy < oyA || oy >= oyB) continue;
        unsigned char* dst = img + ((size_t)Y * a.w + X0) * 3 + e;            // byte e of the tile row: consecutive lanes, consecutive bytes
        int v = fr_vpass(a.yfirst, a.ycount, a.ycoef, a.ytaps, hbuf + e, kFrRowBytes, oy, ybase, rows, skipy);
        if (MASK) {
            const int m = fr_vpass(a.yfirst, a.ycount, a.ycoef, a.ytaps, mbuf + lx, kFrTileW, oy, ybase, rows, skipy);
            const int t = v * m + (int)*dst * (255 - m) + 128;              // paste_mask_L
            v = (t + (t >> 8)) >> 8;
        }
        *dst = (unsigned char)v;
    }
}

__global__ __launch_bounds__(256) void paste_frames_kernel(PasteArgs a) { paste_frames_body<false>(a); }
__global__ __launch_bounds__(256) void paste_frames_mask_kernel(PasteArgs a) { paste_frames_body<true>(a); }

// ---------------------------------------------------------------------------------------------------------------- a box per frame
// The way back of prepare_frames_boxes_kernel: frame f is pasted at ITS box, descriptor row f of frames.hpp's layout {x0, y0, x1, y1, xoff, xtaps,
// yoff, ytaps} with the tables of (source rectangle -> box size) in the pool.  The source rectangle is the launch's.
struct PasteBoxArgs {
    PasteArgs g;                         // what a launch fixes: gen, mask, frames, GH, GW, the source rectangle, h, w, th; tables, box and region not read
    const int* desc;                     // (F, kFrDesc) DEVICE
    const int* pool;
    int pool_len;
};

// grid = (ceil(W / 64), ceil(H / th), F) with W x H the LARGEST box ∩ frame of the launch.  The descriptor is read once, through an address that
// depends on blockIdx.z alone (scalar loads); the frame's region is computed here from the box and h, w.  A workgroup outside its frame's region
// -- a smaller region than the grid's, a box outside the frame, or a descriptor that fails a range check -- leaves through the body's first
// test, which is uniform over the workgroup and comes before the barrier.  A bad descriptor gives wrong (or no) pixels: pool offsets are checked
// against the pool's length here, every store against h, w in the body.
template <bool MASK>
__device__ __forceinline__ void paste_frames_boxes_body(const PasteBoxArgs& b) {
    const int* d = b.desc + (size_t)blockIdx.z * kFrDesc;
    PasteArgs a = b.g;
    a.x0 = d[0]; a.y0 = d[1];
    a.ow = (int)((unsigned)d[2] - (unsigned)a.x0); a.oh = (int)((unsigned)d[3] - (unsigned)a.y0);
    a.xtaps = d[5]; a.ytaps = d[7];
    bool ok = a.ow >= 1 && a.oh >= 1 && a.ow <= kFrBoxMax && a.oh <= kFrBoxMax && a.x0 >= -kFrBoxMax && a.x0 <= kFrBoxMax && a.y0 >= -kFrBoxMax && a.y0 <= kFrBoxMax;
    if (ok && a.ow != a.cw) ok = fr_pool_axis(b.pool, b.pool_len, d[4], a.ow, a.xtaps, a.xfirst, a.xcount, a.xcoef);
    if (ok && a.oh != a.ch) ok = fr_pool_axis(b.pool, b.pool_len, d[6], a.oh, a.ytaps, a.yfirst, a.ycount, a.ycoef);
    if (!ok) { a.x0 = a.y0 = 0; a.ow = a.oh = 0; }                    // an empty region
    a.rx0 = a.x0 < 0 ? 0 : a.x0; a.ry0 = a.y0 < 0 ? 0 : a.y0;
    a.rx1 = a.x0 + a.ow > a.w ? a.w : a.x0 + a.ow;
    a.ry1 = a.y0 + a.oh > a.h ? a.h : a.y0 + a.oh;
    paste_frames_body<MASK>(a);
}

__global__ __launch_bounds__(256) void paste_frames_boxes_kernel(PasteBoxArgs b) { paste_frames_boxes_body<false>(b); }
__global__ __launch_bounds__(256) void paste_frames_boxes_mask_kernel(PasteBoxArgs b) { paste_frames_boxes_body<true>(b); }

}  // namespace tsnet
