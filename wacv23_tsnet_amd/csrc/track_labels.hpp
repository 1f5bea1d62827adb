// track_labels.hpp -- the face labels of a clip with a crop PER FRAME (FaceDatasetTest(fix_crop_pos=False), dataset/dataset_video_face.py:303-320,
// 348-353, 397-398) in one pass over frames of different sizes: tsnet_face_labels_boxes[_u8].
//
// The kernels are the ragged forms of raster.hpp's face_edges_kernel, face_bbox_kernel, gauss1d_u8_kernel, u8_minmax_kernel and
// resize_label_kernel: one launch of each serves every frame of the call, a frame's size and place come from its DEVICE descriptor, the grid
// covers the largest image of the call and a block beyond its own image's extent returns.  Every per-pixel step is SHARED with those kernels,
// not restated: both forms call raster.hpp's draw_face_piece, face_keypoint_box, gauss1d_u8_at and resize_label_at on one image and its own
// h, w.  The kernels here keep what differs -- the descriptor checks, a frame's place in the workspace, the grid -- so frame f of a call has the
// bits of the single-size entries called on frame f alone.  (The min / max of an image has no order to keep -- min and max commute -- and each
// kernel folds it its own way: track_minmax_kernel in the block first, u8_minmax_kernel per thread.)
// The 2F maps of a call are the IMAGES of the ragged batch: image m < F is the edge map of frame m, image F + f the bounding-box mask of frame f.
//
// Descriptor, kTlDesc ints per frame: {h, w, off, lw_rows, woff_rows, lw_cols, woff_cols, 0}
//   h, w        the frame's crop
//   off         byte offset of the frame's region in the workspace
//   lw_*        the Gaussian's half width along that axis: -1 = the axis does not shrink, no pass; 0 = the single weight 1.0, the identity,
//               skipped as well; 1..63 = a pass with the lw + 1 doubles (centre first) at woff_* in the pool of doubles
//
// Workspace, ws_len bytes, 4-byte aligned:
//   [0, 16 F)                          2F {min, max} int pairs, pair m of image m (written by track_fill_kernel, raised by track_minmax_kernel)
//   [off_f, off_f + 4 h_f w_f)         frame f:  edge map A | mask A | edge map B | mask B, h_f w_f bytes each.  A holds what the rasteriser
//                                      drew; the rows pass reads A and writes B, the columns pass reads whichever is current and writes the
//                                      other; a frame without a pass never touches B.
// Regions do not overlap each other nor the pairs (the host checks its copy of the descriptors).  The kernels trust the device copy as far as
// pixels go and no further: everything taken from it is checked against ws_len, pool_len and F here (tl_frame), a row that fails gives an
// all-zero label for that frame, and the outputs are indexed by OH, OW and the grid alone.
//
// Launches of a call: track_fill (mask A, zeroed edge map A, the pairs), track_edges, the rows pass, the columns pass, track_minmax,
// track_resize -- six, four when no frame of the call takes a pass; no memset, no copy.
#pragma once
#include <hip/hip_runtime.h>

#include "raster.hpp"

namespace tsnet {

constexpr int kTlDesc = 8;               // ints of a frame's descriptor
constexpr int kTlMaxSide = 32767;        // h, w: the image's pixel index stays an int
constexpr int kTlMaxLw = 63;

struct TrackLabelArgs {
    const double* kp;                    // (F, 68, 2), relative to each frame's crop
    const double* curves;                // (F, 34, 8), tsnet_fit_face_curves
    const int* desc;                     // (F, kTlDesc) DEVICE
    const double* pool;                  // pool_len doubles
    unsigned char* ws;
    long long ws_len;
    int pool_len, F, bw, OH, OW;
    int map0, nmaps;                     // the maps wanted: [map0, map0 + nmaps) of {0 = edge map / class map, 1 = mask}
    void* out[2];                        // (F, OH, OW) class map, mask: float or bytes
};

struct TlFrame {
    int h, w, lw[2];
    unsigned char* base;                 // the frame's region
    const double* wts[2];
};

// Frame f's descriptor, checked: false = the row cannot be used (the host copy never fails here)
__device__ __forceinline__ bool tl_frame(const TrackLabelArgs& a, int f, TlFrame& t) {
    const int* d = a.desc + (size_t)f * kTlDesc;
    const int h = d[0], w = d[1], off = d[2];
    if (h < 1 || w < 1 || h > kTlMaxSide || w > kTlMaxSide) return false;
    const long long hw = (long long)h * w;
    if ((long long)off < 16ll * a.F || (long long)off + 4 * hw > a.ws_len) return false;
    t.h = h; t.w = w; t.base = a.ws + off;
    for (int ax = 0; ax < 2; ++ax) {
        const int lw = d[3 + 2 * ax], wo = d[4 + 2 * ax];
        if (lw < -1 || lw > kTlMaxLw) return false;
        if (lw > 0 && (wo < 0 || (long long)wo + lw + 1 > (long long)a.pool_len)) return false;
        t.lw[ax] = lw; t.wts[ax] = lw > 0 ? a.pool + wo : nullptr;
    }
    return true;
}

// buffer `which` (0 = A, 1 = B) of the frame's image `map`; tl_final: the buffer its last pass wrote
__device__ __forceinline__ unsigned char* tl_buf(const TlFrame& t, int map, int which) {
    return t.base + (size_t)(2 * which + map) * t.h * t.w;
}
__device__ __forceinline__ int tl_final(const TlFrame& t) { return (t.lw[0] > 0) != (t.lw[1] > 0) ? 1 : 0; }

// grid = (ceil(max h w / 1024), F), 256 threads, four pixels each: the mask (the box of face_keypoint_box, as face_bbox_kernel fills it) into
// mask A, zeros into edge map A, and the frame's two {min, max} pairs set to {255, 0}
__global__ __launch_bounds__(256) void track_fill_kernel(TrackLabelArgs a) {
    const int f = blockIdx.y;
    TlFrame t;
    const bool ok = tl_frame(a, f, t);
    if (blockIdx.x == 0 && threadIdx.x < 4) {                        // pairs f and F + f; a row that fails keeps them defined
        int* mm = reinterpret_cast<int*>(a.ws);
        mm[2 * ((threadIdx.x >> 1) * a.F + f) + (threadIdx.x & 1)] = (threadIdx.x & 1) ? 0 : 255;
    }
    if (!ok) return;
    const int h = t.h, w = t.w, hw = h * w;
    const int first = blockIdx.x * 1024 + threadIdx.x;
    if (blockIdx.x * 1024 >= (unsigned)hw) return;
    const bool edges = a.map0 == 0, mask = a.map0 + a.nmaps == 2;
    int bx0 = 0, bx1 = 0, by0 = 0, by1 = 0;
    if (mask) face_keypoint_box(a.kp + (size_t)f * kFaceKeypoints * 2, h, w, bx0, bx1, by0, by1);
    unsigned char* e = tl_buf(t, 0, 0);
    unsigned char* m = tl_buf(t, 1, 0);
    for (int j = 0; j < 4; ++j) {
        const int i = first + j * 256;
        if (i >= hw) break;
        if (edges) e[i] = 0;
        if (mask) {
            const int y = i / w, x = i - y * w;
            m[i] = (y >= by0 && y < by1 && x >= bx0 && x < bx1) ? 255 : 0;
        }
    }
}

// grid = (kFaceSubEdges, F), 64 threads: draw_face_piece into edge map A, clamped to the frame's own h, w
__global__ __launch_bounds__(64) void track_edges_kernel(TrackLabelArgs a) {
    const int e = blockIdx.x, f = blockIdx.y;
    TlFrame t;
    if (!tl_frame(a, f, t)) return;
    draw_face_piece(a.curves + ((size_t)f * kFaceSubEdges + e) * kCurveRec, tl_buf(t, 0, 0), t.h, t.w, a.bw);
}

// grid = (ceil(max h w / 256), nmaps F), one pixel per thread: gauss1d_u8_at along `axis` (0 = rows, 1 = columns) for the frames that take
// that pass (lw > 0); the others return
__global__ __launch_bounds__(256) void track_gauss_kernel(TrackLabelArgs a, int axis) {
    const int map = a.map0 + blockIdx.y / a.F, f = blockIdx.y % a.F;
    TlFrame t;
    if (!tl_frame(a, f, t)) return;
    const int lw = axis ? t.lw[1] : t.lw[0];                         // selects, not t.lw[axis]: a run-time index would put the frame in memory
    if (lw <= 0) return;
    const int h = t.h, w = t.w;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x * 256 >= (unsigned)(h * w) || i >= h * w) return;
    const int src = (axis == 1 && t.lw[0] > 0) ? 1 : 0;              // the rows pass, when taken, left its result in B
    const unsigned char* img = tl_buf(t, map, src);
    unsigned char* out = tl_buf(t, map, src ^ 1);
    const double* wts = axis ? t.wts[1] : t.wts[0];
    const int y = i / w, x = i - y * w;
    out[i] = gauss1d_u8_at(img, h, w, y, x, axis, wts, lw);
}

// grid = (min(64, ceil(max h w / 256)), nmaps F), 256 threads: u8_minmax_kernel of every image's final buffer into its pair.  The block folds
// its threads' values first (min and max commute: the pair does not depend on the order), then one thread raises the pair with the vector
// atomics u8_minmax_kernel uses.
__global__ __launch_bounds__(256) void track_minmax_kernel(TrackLabelArgs a) {
    __shared__ int slo[256], shi[256];
    const int map = a.map0 + blockIdx.y / a.F, f = blockIdx.y % a.F, tid = threadIdx.x;
    TlFrame t;
    if (!tl_frame(a, f, t)) return;                                  // uniform over the block: no thread reaches the barriers
    const int hw = t.h * t.w;
    const unsigned char* img = tl_buf(t, map, tl_final(t));
    int lo = 255, hi = 0;
    for (int i = blockIdx.x * 256 + tid; i < hw; i += gridDim.x * 256) {
        const int v = img[i];
        lo = v < lo ? v : lo; hi = v > hi ? v : hi;
    }
    slo[tid] = lo; shi[tid] = hi;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (tid < k) { slo[tid] = imin(slo[tid], slo[tid + k]); shi[tid] = imax(shi[tid], shi[tid + k]); }
        __syncthreads();
    }
    if (tid == 0) {
        int* mm = reinterpret_cast<int*>(a.ws) + 2 * (map * a.F + f);
        __hip_atomic_fetch_min(mm, slo[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_max(mm + 1, shi[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// grid = (ceil(OH OW / 256), nmaps F), one output pixel per thread: resize_label_at from the image's final buffer into out[map][f]
template <bool U8>
__global__ __launch_bounds__(256) void track_resize_kernel(TrackLabelArgs a) {
    const int map = a.map0 + blockIdx.y / a.F, f = blockIdx.y % a.F;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.OH * a.OW) return;
    const size_t o = (size_t)f * a.OH * a.OW + i;
    TlFrame t;
    float res = 0.f;
    if (tl_frame(a, f, t)) {
        const int h = t.h, w = t.w, OW = a.OW;
        const double fr = (double)h / (double)a.OH, fc = (double)w / (double)OW;
        const int Y = i / OW, X = i - Y * OW;
        res = resize_label_at(tl_buf(t, map, tl_final(t)), h, w, fr, fc, Y, X, reinterpret_cast<const int*>(a.ws) + 2 * (map * a.F + f));
    }
    if (U8) static_cast<unsigned char*>(a.out[map])[o] = (unsigned char)res;
    else static_cast<float*>(a.out[map])[o] = res;
}

}  // namespace tsnet
