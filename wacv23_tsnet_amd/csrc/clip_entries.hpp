// clip_entries.hpp -- the C entry points of the clip side (include/tsnet_abi.h): what a video clip needs around the forward, none of it touching
// tsnet_engine, Ctx or a convolution -- frame statistics and post-processing (postproc.hpp), the host curve fits and key-point preparation
// (lmfit.hpp, face_adapt.hpp), rasterisation and label resizing (raster.hpp), the frame loader (frames.hpp), the paste (paste.hpp), its feathered masks (mask_blur.hpp),
// the colour conversion to and from YUV 4:2:0 (yuv_frames.hpp) and the labels of a clip with a crop per frame (track_labels.hpp).  engine.cpp includes this file once, last, after its own entries and op_entries.hpp: it is part of that translation
// unit and of no other.  HOST code.
#pragma once
#ifndef TSNET_ENGINE_CPP
#error "clip_entries.hpp is the tail of engine.cpp: include it from there only"
#endif
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "entry_common.hpp"
#include "face_adapt.hpp"
#include "frames.hpp"
#include "lmfit.hpp"
#include "mask_blur.hpp"
#include "paste.hpp"
#include "postproc.hpp"
#include "raster.hpp"
#include "track_labels.hpp"
#include "yuv_frames.hpp"

using namespace tsnet;

extern "C" {

int tsnet_frame_stats(const float* x, int B, int C, int HW, float div, float* mean, float* std_unbiased, void* stream) {
    OP_BEGIN
    if (!x || !mean || !std_unbiased) throw ArgError("frame_stats: null tensor");
    if (B < 1 || C < 1 || HW < 1 || B > 65535 || !(div > 0.f)) throw ArgError("frame_stats: bad shape or divisor");
    hipLaunchKernelGGL(frame_stats_kernel, dim3(C, B), dim3(256), 0, (hipStream_t)stream, x, C, HW, div, mean, std_unbiased);
    check_launch("frame_stats");
    OP_END
}

int tsnet_demo_postprocess(const float* rec, int B, int H, int W, const float* gen_mean, const float* gen_std,
                           const float* ref_mean, const float* ref_std, const float* img_mean_over_255,
                           unsigned char* out_rgb, void* stream) {
    OP_BEGIN
    if (!rec || !gen_mean || !gen_std || !ref_mean || !ref_std || !img_mean_over_255 || !out_rgb) throw ArgError("demo_postprocess: null tensor");
    if (B < 1 || H < 1 || W < 1) throw ArgError("demo_postprocess: bad shape");
    DemoPostArgs a{rec, gen_mean, gen_std, ref_mean, ref_std, {img_mean_over_255[0], img_mean_over_255[1], img_mean_over_255[2]},
                   out_rgb, B, H * W};
    hipLaunchKernelGGL(demo_post_kernel, dim3(ew_grid((size_t)B * H * W)), dim3(256), 0, (hipStream_t)stream, a);
    check_launch("demo_post");
    OP_END
}

int tsnet_fit_face_curves(const double* keypoints, int F, double* curves) {
    OP_BEGIN
    if (!keypoints || !curves || F < 1) throw ArgError("fit_face_curves: bad argument");
    for (int f = 0; f < F; ++f)
        for (int e = 0; e < kFaceSubEdges; ++e) {
            double pts[6];
            const int n = hFaceSubEdgeTable[e][2] < 0 ? 2 : 3;
            for (int i = 0; i < n; ++i) {
                const double* k = keypoints + ((size_t)f * kFaceKeypoints + hFaceSubEdgeTable[e][i]) * 2;
                pts[2 * i] = k[0]; pts[2 * i + 1] = k[1];
            }
            lm::fit_piece(pts, n, curves + ((size_t)f * kFaceSubEdges + e) * kCurveRec);
        }
    OP_END
}

// key-point preparation of a cross-identity face pair (csrc/face_adapt.hpp): host arithmetic, no device work
int tsnet_face_adapt_stats(const double* kp, int F, double* stats) {
    OP_BEGIN
    if (const char* err = face_adapt::stats(kp, F, stats)) throw ArgError(err);
    OP_END
}

int tsnet_face_adapt_apply(const double* stats, double* kp, int F) {
    OP_BEGIN
    if (const char* err = face_adapt::apply(stats, kp, F)) throw ArgError(err);
    OP_END
}

int tsnet_smooth_keypoints(const double* in, int F, int P, double* out) {
    OP_BEGIN
    if (const char* err = face_adapt::smooth(in, F, P, out)) throw ArgError(err);
    OP_END
}

int tsnet_fit_pose_curves(const double* pts, int F, int flags, double* curves) {
    OP_BEGIN
    if (!pts || !curves || F < 1) throw ArgError("fit_pose_curves: bad argument");
    for (int f = 0; f < F; ++f) {
        const double* P = pts + (size_t)f * kPosePts * 2;
        for (int e = 0; e < kPosePrims; ++e) {
            double* rec = curves + ((size_t)f * kPosePrims + e) * kCurveRec;
            for (int i = 0; i < kCurveRec; ++i) rec[i] = 0.0;
            int ia = 0, ib = 0;
            if (!pose_primitive_points(e, flags, ia, ib)) continue;
            const double two[4] = {P[2 * ia], P[2 * ia + 1], P[2 * ib], P[2 * ib + 1]};
            if (two[0] == 0.0 || two[2] == 0.0) continue;               // `0 not in x` (connect_keypoints): a missing point
            lm::fit_piece(two, 2, rec);
        }
    }
    OP_END
}

int tsnet_raster_face(const double* keypoints, const double* curves, int F, int h, int w, int bw, unsigned char* edges, unsigned char* bbox, void* stream) {
    OP_BEGIN
    if ((!edges && !bbox) || (edges && !curves) || (bbox && !keypoints)) throw ArgError("raster_face: null tensor");
    if (F < 1 || F > 65535 || h < 1 || w < 1 || bw < 1 || (double)h * w >= 2147483647.0) throw ArgError("raster_face: bad shape");
    hipStream_t s = (hipStream_t)stream;
    if (edges) {
        HIP_TRY(hipMemsetAsync(edges, 0, (size_t)F * h * w, s));
        hipLaunchKernelGGL(face_edges_kernel, dim3(kFaceSubEdges, F), dim3(64), 0, s, curves, edges, h, w, bw);
        check_launch("face_edges");
    }
    if (bbox) {
        hipLaunchKernelGGL(face_bbox_kernel, dim3(F), dim3(256), 0, s, keypoints, bbox, h, w);
        check_launch("face_bbox");
    }
    OP_END
}

int tsnet_raster_pose(const double* pts, const double* curves, int F, int h, int w, int win_x0, int win_y0, int win_x1, int win_y1, int flags,
                      unsigned char* labels, void* stream) {
    OP_BEGIN
    if (!pts || !curves || !labels) throw ArgError("raster_pose: null tensor");
    if (F < 1 || F > 65535 || h < 1 || w < 1 || (double)h * w >= 2147483647.0) throw ArgError("raster_pose: bad shape");
    if (win_x0 < 0 || win_y0 < 0 || win_x1 > w || win_y1 > h || win_x1 <= win_x0 || win_y1 <= win_y0) throw ArgError("raster_pose: window outside the frame");
    if (((uintptr_t)labels & 3) != 0) throw ArgError("raster_pose: labels must be 4-byte aligned (and padded to a multiple of 4 bytes)");
    hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)F * (win_y1 - win_y0) * (win_x1 - win_x0), n4 = (n + 3) / 4 * 4;
    HIP_TRY(hipMemsetAsync(labels, 0, n4, s));
    hipLaunchKernelGGL(pose_edges_kernel, dim3(kPosePrims, F), dim3(64), 0, s, pts, curves, labels, h, w, win_x0, win_y0, win_x1, win_y1, flags);
    check_launch("pose_edges");
    hipLaunchKernelGGL(pose_order_to_class_kernel, dim3(ew_grid(n)), dim3(256), 0, s, labels, n);
    check_launch("pose_order_to_class");
    OP_END
}

int tsnet_label_bbox(const unsigned char* labels, int F, int h, int w, unsigned char* bbox, void* stream) {
    OP_BEGIN
    if (!labels || !bbox) throw ArgError("label_bbox: null tensor");
    if (F < 1 || F > 65535 || h < 1 || w < 1 || (double)h * w >= 2147483647.0) throw ArgError("label_bbox: bad shape");
    hipLaunchKernelGGL(label_bbox_kernel, dim3(F), dim3(256), 0, (hipStream_t)stream, labels, bbox, h, w);
    check_launch("label_bbox");
    OP_END
}

int tsnet_resize_pad(const unsigned char* in, int F, int h, int w, const int* ytab, const int* xtab, int oh, int ow,
                     int pad_top, int pad_left, int OH, int OW, int binarise, float* out, void* stream) {
    OP_BEGIN
    if (!in || !ytab || !xtab || !out) throw ArgError("resize_pad: null tensor");
    if (F < 1 || h < 1 || w < 1 || oh < 1 || ow < 1 || pad_top < 0 || pad_left < 0 || pad_top + oh > OH || pad_left + ow > OW)
        throw ArgError("resize_pad: bad shape");
    hipLaunchKernelGGL(gather_pad_kernel, dim3(ew_grid((size_t)F * OH * OW)), dim3(256), 0, (hipStream_t)stream, in, F, h, w, ytab, xtab, oh, ow,
                       pad_top, pad_left, OH, OW, out, binarise);
    check_launch("gather_pad");
    OP_END
}

int tsnet_resize_label(const unsigned char* in, int F, int h, int w, int OH, int OW, const double* wts_rows, int lw_rows,
                       const double* wts_cols, int lw_cols, float* out, void* stream) {
    OP_BEGIN
    if (!in || !out) throw ArgError("resize_label: null tensor");
    if (F < 1 || h < 1 || w < 1 || OH < 1 || OW < 1) throw ArgError("resize_label: bad shape");
    if (lw_rows < -1 || lw_cols < -1 || lw_rows > 63 || lw_cols > 63 || (lw_rows >= 0 && !wts_rows) || (lw_cols >= 0 && !wts_cols))
        throw ArgError("resize_label: bad Gaussian kernel");
    hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)F * h * w;
    unsigned char *t0 = nullptr, *t1 = nullptr;
    double* dw = nullptr;
    int* mm = nullptr;
    struct Guard { unsigned char*& a; unsigned char*& b; double*& c; int*& d; ~Guard() { (void)hipFree(a); (void)hipFree(b); (void)hipFree(c); (void)hipFree(d); } } guard{t0, t1, dw, mm};
    const unsigned char* cur = in;
    // anti-aliasing passes: one per axis that shrinks (lw >= 0); the caller supplies the kernel halves (centre first) it computed in fp64
    for (int axis = 0; axis < 2; ++axis) {
        const int lw = axis ? lw_cols : lw_rows;
        const double* wts = axis ? wts_cols : wts_rows;
        if (lw < 0) continue;
        unsigned char*& dst = (cur == t0) ? t1 : t0;
        if (!dst) HIP_TRY(hipMalloc((void**)&dst, n));
        if (!dw) HIP_TRY(hipMalloc((void**)&dw, 2 * 64 * sizeof(double)));
        HIP_TRY(hipMemcpyAsync(dw + axis * 64, wts, (lw + 1) * sizeof(double), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(gauss1d_u8_kernel, dim3(ew_grid(n)), dim3(256), 0, s, cur, dst, F, h, w, axis, dw + axis * 64, lw);
        check_launch("gauss1d_u8");
        cur = dst;
    }
    HIP_TRY(hipMalloc((void**)&mm, (size_t)2 * F * sizeof(int)));
    std::vector<int> init(2 * F);
    for (int f = 0; f < F; ++f) { init[2 * f] = 255; init[2 * f + 1] = 0; }
    HIP_TRY(hipMemcpyAsync(mm, init.data(), init.size() * sizeof(int), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(u8_minmax_kernel, dim3(std::min(64, (h * w + 255) / 256), F), dim3(256), 0, s, cur, F, h * w, mm);
    check_launch("u8_minmax");
    hipLaunchKernelGGL(resize_label_kernel, dim3(ew_grid((size_t)F * OH * OW)), dim3(256), 0, s, cur, F, h, w, OH, OW, mm, out);
    check_launch("resize_label");
    HIP_TRY(hipStreamSynchronize(s));                                  // host temporaries (init, the caller's kernels) and device scratch end here
    OP_END
}

int tsnet_vl2ch(const float* labels, int B, int HW, int num_classes, float* out, void* stream) {
    OP_BEGIN
    if (!labels || !out) throw ArgError("vl2ch: null tensor");
    if (B < 1 || HW < 1 || num_classes < 1) throw ArgError("vl2ch: bad shape");
    hipLaunchKernelGGL(onehot_kernel, dim3(ew_grid((size_t)B * num_classes * HW)), dim3(256), 0, (hipStream_t)stream, labels, out, B, HW, num_classes);
    check_launch("onehot");
    OP_END
}

int tsnet_bicubic_taps(int n_in, int n_out) {
    if (n_in < 1 || n_out < 1) { g_op_error = "bicubic_taps: sizes must be positive"; return TSNET_ERR_ARG; }
    return bicubic_taps(n_in, n_out);
}

int tsnet_bicubic_table(int n_in, int n_out, int* first, int* count, int* coef) {
    OP_BEGIN
    if (n_in < 1 || n_out < 1 || !first || !count || !coef) throw ArgError("bicubic_table: bad argument");
    bicubic_table(n_in, n_out, first, count, coef);
    OP_END
}

// ---- the loader (frames.hpp) and the paste (paste.hpp), each with ONE box for the call (tables: three arrays per axis) and with a box PER FRAME
// (HOST descriptors {x0, y0, x1, y1, xoff, xtaps, yoff, ytaps}, tables in a pool).  The checks of a box are stated once for both forms: the
// single-box entries call them once with pre = "<entry>: ", the per-frame entries per descriptor row with pre = box_frame(who, f), all rows
// before anything is launched.  The two forms word their table refusals differently and order them differently; both are kept as they were.
static std::string box_frame(const char* who, int f) { return std::string(who) + ": frame " + std::to_string(f) + ": "; }

static void check_frames_shape(const char* who, int F, int h, int w) {
    if (F < 1 || F > 65535 || h < 1 || w < 1 || (double)h * w * 3 >= 2147483647.0) throw ArgError(std::string(who) + ": bad frame shape");
}

// box = {x0, y0, x1, y1}; the paste also bounds the corner from above (its kernels add the corner to a pixel index)
static void check_box_limits(const std::string& pre, const int* box, bool paste) {
    const int x0 = box[0], y0 = box[1], x1 = box[2], y1 = box[3];
    bool bad = x1 <= x0 || y1 <= y0 || (double)x1 - x0 > 1e6 || (double)y1 - y0 > 1e6 || x0 < -1000000 || y0 < -1000000;
    if (paste) bad = bad || x0 > 1000000 || y0 > 1000000;
    if (bad) throw ArgError(pre + (paste ? "empty or absurd box" : "empty or absurd crop box"));
}

// One resampling axis of a box, n_in -> n_out with `taps` coefficients per table row.  An axis that keeps its size is skipped: nothing of its
// table is looked at.  A row of fewer coefficients than the size ratio needs (count > taps) cannot be a table of tsnet_bicubic_table.
struct BoxAxis { const char* name; int n_in, n_out, taps; };
static bool axis_skipped(const BoxAxis& a) { return a.n_in == a.n_out; }
static bool axis_taps_wrong(const BoxAxis& a) { return !axis_skipped(a) && a.taps != bicubic_taps(a.n_in, a.n_out); }

// single box: the tables of both axes, then the taps of both; have_*: that axis' three arrays are there; *taps_text: the entry's words for wrong taps
static void check_single_tables(const std::string& pre, const BoxAxis& x, bool have_x, const char* xtaps_text, const BoxAxis& y, bool have_y, const char* ytaps_text) {
    if (!axis_skipped(x) && !have_x) throw ArgError(pre + "the horizontal pass needs its tables");
    if (!axis_skipped(y) && !have_y) throw ArgError(pre + "the vertical pass needs its tables");
    if (axis_taps_wrong(x)) throw ArgError(pre + xtaps_text);
    if (axis_taps_wrong(y)) throw ArgError(pre + ytaps_text);
}

// a box per frame: one axis at a time, its table at `off` in a pool of pool_len ints
static void check_frame_axis(const std::string& pre, const BoxAxis& a, int off, const int* pool, int pool_len) {
    if (axis_skipped(a)) return;
    if (off < 0) throw ArgError(pre + "the " + a.name + " pass needs its table (offset " + std::to_string(off) + ")");
    if (axis_taps_wrong(a)) throw ArgError(pre + a.name + " taps are not tsnet_bicubic_taps(" + std::to_string(a.n_in) + ", " + std::to_string(a.n_out) + ")");
    if (!pool || (long long)off + (long long)a.n_out * (2 + (long long)a.taps) > (long long)pool_len)
        throw ArgError(pre + "the " + a.name + " table at offset " + std::to_string(off) + " ends beyond the pool of " + std::to_string(pool_len) + " ints");
}

// th, the running tile height of a launch, lowered until the rows of the horizontal pass that th output rows read (frames_row_span; the paste
// never keeps more than the ch rows its source rectangle has) fit the kFrRows a tile holds
static void lower_tile_height(const std::string& pre, int ch, int oh, bool paste, int& th) {
    auto span = [&](int t) { const int s = frames_row_span(ch, oh, t); return paste && s > ch ? ch : s; };
    while (th > 1 && span(th) > kFrRows) th >>= 1;
    if (span(th) > kFrRows)
        throw ArgError(pre + (paste ? "vertical reduction too steep (more than 112 source rows under one output row)" : "vertical reduction too steep (more than 112 taps)"));
}

static void check_prepare_output(const char* who, int oh, int ow, int pad_top, int pad_left, int OH, int OW) {
    if (oh < 1 || ow < 1 || pad_top < 0 || pad_left < 0 || pad_top + oh > OH || pad_left + ow > OW || (double)OH * OW >= 2147483647.0 / 4)
        throw ArgError(std::string(who) + ": the resized image and its padding do not fit the output");
}

// mean_bgr null: the byte form (out holds (F,3,OH,OW) bytes)
static void prepare_frames_any(const unsigned char* frames, int F, int h, int w, int x0, int y0, int x1, int y1,
                               const int* xfirst, const int* xcount, const int* xcoef, int xtaps,
                               const int* yfirst, const int* ycount, const int* ycoef, int ytaps,
                               int oh, int ow, int pad_top, int pad_left, int OH, int OW, const float* mean_bgr, void* out, bool u8, void* stream) {
    const char* who = "prepare_frames";
    const std::string pre = "prepare_frames: ";
    const int box[4] = {x0, y0, x1, y1};
    if (!frames || !out || (!u8 && !mean_bgr)) throw ArgError("prepare_frames: null tensor");
    check_frames_shape(who, F, h, w);
    check_box_limits(pre, box, false);                               // this entry looks at its box before its output, the per-frame one after
    check_prepare_output(who, oh, ow, pad_top, pad_left, OH, OW);
    const int cw = x1 - x0, ch = y1 - y0;
    check_single_tables(pre, {"horizontal", cw, ow, xtaps}, xfirst && xcount && xcoef, "xtaps is not tsnet_bicubic_taps(x1 - x0, ow)",
                        {"vertical", ch, oh, ytaps}, yfirst && ycount && ycoef, "ytaps is not tsnet_bicubic_taps(y1 - y0, oh)");
    int th = kFrTileH;
    lower_tile_height(pre, ch, oh, false, th);
    const int gy = (OH + th - 1) / th;
    if (gy > 65535) throw ArgError("prepare_frames: output too tall");
    FrameArgs a{frames, static_cast<float*>(out), xfirst, xcount, xcoef, yfirst, ycount, ycoef, h, w, x0, y0, cw, ch, ow, oh, xtaps, ytaps, pad_top, pad_left, OH, OW, th,
                {u8 ? 0.f : mean_bgr[0], u8 ? 0.f : mean_bgr[1], u8 ? 0.f : mean_bgr[2]}};
    const dim3 grid((OW + kFrTileW - 1) / kFrTileW, gy, F);
    if (u8) hipLaunchKernelGGL(prepare_frames_u8_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(prepare_frames_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
    check_launch("prepare_frames");
}

int tsnet_prepare_frames(const unsigned char* frames, int F, int h, int w, int x0, int y0, int x1, int y1,
                         const int* xfirst, const int* xcount, const int* xcoef, int xtaps,
                         const int* yfirst, const int* ycount, const int* ycoef, int ytaps,
                         int oh, int ow, int pad_top, int pad_left, int OH, int OW, const float* mean_bgr, float* out, void* stream) {
    OP_BEGIN
    prepare_frames_any(frames, F, h, w, x0, y0, x1, y1, xfirst, xcount, xcoef, xtaps, yfirst, ycount, ycoef, ytaps, oh, ow, pad_top, pad_left, OH, OW,
                       mean_bgr, out, false, stream);
    OP_END
}

int tsnet_prepare_frames_u8(const unsigned char* frames, int F, int h, int w, int x0, int y0, int x1, int y1,
                            const int* xfirst, const int* xcount, const int* xcoef, int xtaps,
                            const int* yfirst, const int* ycount, const int* ycoef, int ytaps,
                            int oh, int ow, int pad_top, int pad_left, int OH, int OW, unsigned char* out, void* stream) {
    OP_BEGIN
    prepare_frames_any(frames, F, h, w, x0, y0, x1, y1, xfirst, xcount, xcoef, xtaps, yfirst, ycount, ycoef, ytaps, oh, ow, pad_top, pad_left, OH, OW,
                       nullptr, out, true, stream);
    OP_END
}

static void prepare_frames_boxes_any(const unsigned char* frames, int F, int h, int w, const int* boxes_host, const int* boxes_dev, const int* pool,
                                     int pool_len, int oh, int ow, int pad_top, int pad_left, int OH, int OW, const float* mean_bgr, void* out, bool u8,
                                     void* stream) {
    const char* who = "prepare_frames_boxes";
    if (!frames || !out || (!u8 && !mean_bgr) || !boxes_host || !boxes_dev) throw ArgError("prepare_frames_boxes: null tensor");
    check_frames_shape(who, F, h, w);
    if (pool_len < 0) throw ArgError("prepare_frames_boxes: negative pool length");
    check_prepare_output(who, oh, ow, pad_top, pad_left, OH, OW);
    int th = kFrTileH;                                               // one tile height per launch: the smallest any frame needs
    for (int f = 0; f < F; ++f) {
        const int* d = boxes_host + (size_t)f * kFrDesc;
        const std::string pre = box_frame(who, f);
        check_box_limits(pre, d, false);
        const int cw = d[2] - d[0], ch = d[3] - d[1];
        check_frame_axis(pre, {"horizontal", cw, ow, d[5]}, d[4], pool, pool_len);
        check_frame_axis(pre, {"vertical", ch, oh, d[7]}, d[6], pool, pool_len);
        lower_tile_height(pre, ch, oh, false, th);
    }
    const int gy = (OH + th - 1) / th;
    if (gy > 65535) throw ArgError("prepare_frames_boxes: output too tall");
    FrameBoxArgs b{{frames, static_cast<float*>(out), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, h, w, 0, 0, 0, 0, ow, oh, 0, 0, pad_top, pad_left, OH, OW, th,
                    {u8 ? 0.f : mean_bgr[0], u8 ? 0.f : mean_bgr[1], u8 ? 0.f : mean_bgr[2]}}, boxes_dev, pool, pool_len};
    const dim3 grid((OW + kFrTileW - 1) / kFrTileW, gy, F);
    if (u8) hipLaunchKernelGGL(prepare_frames_boxes_u8_kernel, grid, dim3(256), 0, (hipStream_t)stream, b);
    else hipLaunchKernelGGL(prepare_frames_boxes_kernel, grid, dim3(256), 0, (hipStream_t)stream, b);
    check_launch("prepare_frames_boxes");
}

int tsnet_prepare_frames_boxes(const unsigned char* frames, int F, int h, int w, const int* boxes_host, const int* boxes_dev, const int* pool, int pool_len,
                               int oh, int ow, int pad_top, int pad_left, int OH, int OW, const float* mean_bgr, float* out, void* stream) {
    OP_BEGIN
    prepare_frames_boxes_any(frames, F, h, w, boxes_host, boxes_dev, pool, pool_len, oh, ow, pad_top, pad_left, OH, OW, mean_bgr, out, false, stream);
    OP_END
}

int tsnet_prepare_frames_boxes_u8(const unsigned char* frames, int F, int h, int w, const int* boxes_host, const int* boxes_dev, const int* pool, int pool_len,
                                  int oh, int ow, int pad_top, int pad_left, int OH, int OW, unsigned char* out, void* stream) {
    OP_BEGIN
    prepare_frames_boxes_any(frames, F, h, w, boxes_host, boxes_dev, pool, pool_len, oh, ow, pad_top, pad_left, OH, OW, nullptr, out, true, stream);
    OP_END
}

// the paste's tensors and shapes; `desc`: false when the per-frame form misses a descriptor array
static void check_paste_frames(const char* who, const unsigned char* gen, const unsigned char* frames, bool desc, int F, int GH, int GW, int sx0, int sy0,
                               int sx1, int sy1, int h, int w) {
    if (!gen || !frames || !desc) throw ArgError(std::string(who) + ": null tensor");
    check_frames_shape(who, F, h, w);
    if (GH < 1 || GW < 1 || (double)GH * GW * 3 >= 2147483647.0) throw ArgError(std::string(who) + ": bad shape of the generated frames");
    if (sx0 < 0 || sy0 < 0 || sx1 <= sx0 || sy1 <= sy0 || sx1 > GW || sy1 > GH)
        throw ArgError(std::string(who) + ": the source rectangle is empty or not inside the generated frame");
}

// box ∩ frame -> r = {rx0, ry0, rx1, ry1}; false when it is empty (Image.paste: a box outside the frame writes nothing)
static bool paste_region(const int* box, int h, int w, int* r) {
    r[0] = box[0] < 0 ? 0 : box[0]; r[1] = box[1] < 0 ? 0 : box[1]; r[2] = box[2] > w ? w : box[2]; r[3] = box[3] > h ? h : box[3];
    return r[0] < r[2] && r[1] < r[3];
}

int tsnet_paste_frames(const unsigned char* gen, const unsigned char* mask, int F, int GH, int GW, int sx0, int sy0, int sx1, int sy1,
                       const int* xfirst, const int* xcount, const int* xcoef, int xtaps,
                       const int* yfirst, const int* ycount, const int* ycoef, int ytaps,
                       unsigned char* frames, int h, int w, int x0, int y0, int x1, int y1, void* stream) {
    OP_BEGIN
    const std::string pre = "paste_frames: ";
    check_paste_frames("paste_frames", gen, frames, true, F, GH, GW, sx0, sy0, sx1, sy1, h, w);
    const int box[4] = {x0, y0, x1, y1};
    check_box_limits(pre, box, true);
    const int cw = sx1 - sx0, ch = sy1 - sy0, ow = x1 - x0, oh = y1 - y0;
    check_single_tables(pre, {"horizontal", cw, ow, xtaps}, xfirst && xcount && xcoef, "xtaps is not tsnet_bicubic_taps(sx1 - sx0, x1 - x0)",
                        {"vertical", ch, oh, ytaps}, yfirst && ycount && ycoef, "ytaps is not tsnet_bicubic_taps(sy1 - sy0, y1 - y0)");
    int th = kFrTileH, r[4];
    lower_tile_height(pre, ch, oh, true, th);
    if (!paste_region(box, h, w, r)) return TSNET_OK;
    const int gy = (r[3] - r[1] + th - 1) / th;
    if (gy > 65535) throw ArgError("paste_frames: region too tall");
    PasteArgs a{gen, mask, frames, xfirst, xcount, xcoef, yfirst, ycount, ycoef, GH, GW, sx0, sy0, cw, ch, h, w, x0, y0, ow, oh, r[0], r[1], r[2], r[3], xtaps, ytaps, th};
    const dim3 grid((r[2] - r[0] + kFrTileW - 1) / kFrTileW, gy, F);
    if (mask) hipLaunchKernelGGL(paste_frames_mask_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(paste_frames_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
    check_launch("paste_frames");
    OP_END
}

int tsnet_paste_frames_boxes(const unsigned char* gen, const unsigned char* mask, int F, int GH, int GW, int sx0, int sy0, int sx1, int sy1,
                             const int* boxes_host, const int* boxes_dev, const int* pool, int pool_len, unsigned char* frames, int h, int w, void* stream) {
    OP_BEGIN
    const char* who = "paste_frames_boxes";
    check_paste_frames(who, gen, frames, boxes_host && boxes_dev, F, GH, GW, sx0, sy0, sx1, sy1, h, w);
    if (pool_len < 0) throw ArgError("paste_frames_boxes: negative pool length");
    const int cw = sx1 - sx0, ch = sy1 - sy0;
    int th = kFrTileH, rw = 0, rh = 0;                               // one tile height per launch; the largest box ∩ frame
    for (int f = 0; f < F; ++f) {
        const int* d = boxes_host + (size_t)f * kFrDesc;
        const std::string pre = box_frame(who, f);
        check_box_limits(pre, d, true);
        const int ow = d[2] - d[0], oh = d[3] - d[1];
        check_frame_axis(pre, {"horizontal", cw, ow, d[5]}, d[4], pool, pool_len);
        check_frame_axis(pre, {"vertical", ch, oh, d[7]}, d[6], pool, pool_len);
        lower_tile_height(pre, ch, oh, true, th);
        int r[4];
        if (paste_region(d, h, w, r)) { rw = r[2] - r[0] > rw ? r[2] - r[0] : rw; rh = r[3] - r[1] > rh ? r[3] - r[1] : rh; }
    }
    if (rw == 0) return TSNET_OK;                                    // Image.paste: every box is outside its frame, nothing is written
    const int gy = (rh + th - 1) / th;
    if (gy > 65535) throw ArgError("paste_frames_boxes: region too tall");
    PasteBoxArgs b{{gen, mask, frames, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, GH, GW, sx0, sy0, cw, ch, h, w, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, th},
                   boxes_dev, pool, pool_len};
    const dim3 grid((rw + kFrTileW - 1) / kFrTileW, gy, F);
    if (mask) hipLaunchKernelGGL(paste_frames_boxes_mask_kernel, grid, dim3(256), 0, (hipStream_t)stream, b);
    else hipLaunchKernelGGL(paste_frames_boxes_kernel, grid, dim3(256), 0, (hipStream_t)stream, b);
    check_launch("paste_frames_boxes");
    OP_END
}

// ---- feathered paste masks (mask_blur.hpp): Pillow's GaussianBlur on "L" images
int tsnet_gaussian_box_params(float radius, int passes, int* box_radius, unsigned* ww, unsigned* fw) {
    OP_BEGIN
    if (!box_radius || !ww || !fw) throw ArgError("gaussian_box_params: null output");
    if (!(radius >= 0.f) || std::isinf(radius)) throw ArgError("gaussian_box_params: the radius must be finite and not negative");
    if (passes < 1) throw ArgError("gaussian_box_params: passes must be at least 1");
    const float R = mb_box_radius(radius, passes);
    if (!(R >= 0.f && R <= 1e9f)) throw ArgError("gaussian_box_params: the box radius of this blur radius does not fit an int");
    mb_line_constants(R, *box_radius, *ww, *fw);
    OP_END
}

int tsnet_blur_mask(const unsigned char* in, int F, int H, int W, const int* rect, float radius_x, float radius_y, int flags,
                    unsigned char* out, unsigned char* tmp, void* stream) {
    OP_BEGIN
    if (!out || !tmp) throw ArgError("blur_mask: null output or intermediate");
    if (!in && !rect) throw ArgError("blur_mask: neither an input image nor a rectangle");
    if (F < 1 || F > 65535 || H < 1 || W < 1) throw ArgError("blur_mask: bad shape");
    if (H > kMbMaxSide || W > kMbMaxSide)
        throw ArgError("blur_mask: image of " + std::to_string(H) + " x " + std::to_string(W) + " (H x W): a side is over kMbMaxSide = " + std::to_string(kMbMaxSide));
    for (float r : {radius_x, radius_y})
        if (!(r >= 0.f) || !(r <= kMbMaxRadius)) throw ArgError("blur_mask: a radius must be a number in 0 .. " + std::to_string((int)kMbMaxRadius));
    if ((flags & ~0xFF01) != 0) throw ArgError("blur_mask: unknown flag bits");
    if (((flags >> 8) & 0xFF) > 1) throw ArgError("blur_mask: unknown route " + std::to_string((flags >> 8) & 0xFF) + " (0 = the library's choice, 1 = rows then columns)");
    if (!in && (rect[0] < 0 || rect[1] < 0 || rect[2] > W || rect[3] > H || rect[2] <= rect[0] || rect[3] <= rect[1]))
        throw ArgError("blur_mask: the rectangle is empty or not inside the image");
    if (out == in || out == tmp) throw ArgError("blur_mask: out must not be in or tmp");
    hipStream_t s = (hipStream_t)stream;
    const bool rows = radius_x != 0.f, cols = radius_y != 0.f;
    MaskBlurArgs a{in, out, H, W, 0, 0, 0, 0, flags & 1, 0, 0, 0u, 0u};
    if (!in) { a.x0 = rect[0]; a.y0 = rect[1]; a.x1 = rect[2]; a.y1 = rect[3]; }
    const dim3 grid_rows((H + kMbLines - 1) / kMbLines, F), grid_cols((W + kMbLines - 1) / kMbLines, F);
    if (rows) {                                                      // the rows first; through tmp when the columns follow
        a.out = cols ? tmp : out;
        a.passes = kMbPasses;
        mb_line_constants(mb_box_radius(radius_x, kMbPasses), a.radius, a.ww, a.fw);
        hipLaunchKernelGGL(mask_blur_rows_kernel, grid_rows, dim3(256), 0, s, a);
        check_launch("mask_blur_rows");
        a.in = tmp; a.binary = 0;                                    // what follows reads bytes that are final
    }
    if (cols || !rows) {                                             // neither axis: the column form with no pass is the copy
        a.out = out;
        a.passes = cols ? kMbPasses : 0;
        if (cols) mb_line_constants(mb_box_radius(radius_y, kMbPasses), a.radius, a.ww, a.fw);
        hipLaunchKernelGGL(mask_blur_cols_kernel, grid_cols, dim3(256), 0, s, a);
        check_launch("mask_blur_cols");
    }
    OP_END
}

// ---- video in and out as YUV 4:2:0 (yuv_frames.hpp): integer colour conversion on 16-bit fixed-point tables, I420 or NV12
int tsnet_yuv_coeffs(int standard, int full_range, int* fwd, int* inv) {
    OP_BEGIN
    if (!fwd || !inv) throw ArgError("yuv_coeffs: null table");
    if (!yuv_tables(standard, full_range != 0, fwd, inv)) throw ArgError("yuv_coeffs: unknown standard " + std::to_string(standard) + " (601 = BT.601, 709 = BT.709)");
    OP_END
}

// what the two conversions check alike; the table is checked by the caller.  Returns the launch's arguments but for the table.
static YuvArgs yuv_checked_args(const std::string& who, const void* src, void* dst, const int* table, int F, int h, int w, int layout) {
    if (!src || !dst) throw ArgError(who + ": null tensor");
    if (!table) throw ArgError(who + ": null table");
    if (F < 1 || h < 1 || w < 1) throw ArgError(who + ": bad shape");
    if (F > kYuvMaxFrames) throw ArgError(who + ": " + std::to_string(F) + " frames, over kYuvMaxFrames = " + std::to_string(kYuvMaxFrames) + " (the grid's second dimension)");
    if ((long long)h * w * 3 > 2147483647LL)
        throw ArgError(who + ": a frame of " + std::to_string(h) + " x " + std::to_string(w) + " (h x w) is over 2^31 - 1 RGB bytes, the 32-bit index inside a frame");
    if (layout != 0 && layout != 1) throw ArgError(who + ": unknown layout " + std::to_string(layout) + " (0 = I420, 1 = NV12)");
    if (src == dst) throw ArgError(who + ": yuv and rgb must not be the same buffer");
    YuvArgs a{};
    a.src = (const unsigned char*)src; a.dst = (unsigned char*)dst;
    a.h = h; a.w = w; a.ch = (h + 1) / 2; a.cw = (w + 1) / 2;
    a.nbx = (w + kYuvBlockW - 1) / kYuvBlockW;
    a.nv12 = layout;
    return a;
}

static dim3 yuv_grid(const YuvArgs& a, int F) { return dim3((unsigned)(((long long)a.nbx * a.ch + 255) / 256), (unsigned)F); }

int tsnet_rgb_to_yuv420(const unsigned char* rgb, int F, int h, int w, const int* fwd, int layout, unsigned char* yuv, void* stream) {
    OP_BEGIN
    YuvArgs a = yuv_checked_args("rgb_to_yuv420", rgb, yuv, fwd, F, h, w, layout);
    for (int r = 0; r < 3; ++r) {
        if (!yuv_fwd_row_fits(fwd + 4 * r))
            throw ArgError("rgb_to_yuv420: table row " + std::to_string(r) + " has a sum of |c| over kYuvRowSumMax = " + std::to_string(kYuvRowSumMax) + ": the sums would overflow 32 bits");
        if (fwd[4 * r + 3] < 0 || fwd[4 * r + 3] > 255) throw ArgError("rgb_to_yuv420: table offset " + std::to_string(fwd[4 * r + 3]) + " outside 0 .. 255");
    }
    for (int i = 0; i < 12; ++i) a.c[i] = fwd[i];
    hipLaunchKernelGGL(rgb_to_yuv420_kernel, yuv_grid(a, F), dim3(256), 0, (hipStream_t)stream, a);
    check_launch("rgb_to_yuv420");
    OP_END
}

int tsnet_yuv420_to_rgb(const unsigned char* yuv, int F, int h, int w, const int* inv, int layout, unsigned char* rgb, void* stream) {
    OP_BEGIN
    YuvArgs a = yuv_checked_args("yuv420_to_rgb", yuv, rgb, inv, F, h, w, layout);
    for (int i = 0; i < 5; ++i)
        if (!yuv_inv_coef_fits(inv[i]))
            throw ArgError("yuv420_to_rgb: table entry " + std::to_string(i) + " is over kYuvInvCoefMax = " + std::to_string(kYuvInvCoefMax) + " in size: the sums would overflow 32 bits");
    if (inv[5] < 0 || inv[5] > 255) throw ArgError("yuv420_to_rgb: table offset " + std::to_string(inv[5]) + " outside 0 .. 255");
    for (int i = 0; i < 6; ++i) a.c[i] = inv[i];
    hipLaunchKernelGGL(yuv420_to_rgb_kernel, yuv_grid(a, F), dim3(256), 0, (hipStream_t)stream, a);
    check_launch("yuv420_to_rgb");
    OP_END
}

// ---- face labels with a crop per frame (track_labels.hpp): HOST descriptors {h, w, off, lw_rows, woff_rows, lw_cols, woff_cols, 0}, all of them
// checked here before anything is enqueued
static void check_label_axis(const char* who, int f, const char* axis, int n_in, int n_out, int lw, int woff, const double* pool, int pool_len) {
    if (lw < -1 || lw > kTlMaxLw) throw ArgError(box_frame(who, f) + axis + " lw " + std::to_string(lw) + " is outside -1 .. 63");
    const double sigma = std::max(0.0, ((double)n_in / (double)n_out - 1.0) / 2.0);         // skimage's anti-aliasing sigma (demo._aa_kernel)
    if (sigma <= 1e-15) {
        if (lw >= 0) throw ArgError(box_frame(who, f) + "the " + axis + " do not shrink (" + std::to_string(n_in) + " -> " + std::to_string(n_out) + "): lw must be -1");
        return;
    }
    if (lw != (int)(4.0 * sigma + 0.5))
        throw ArgError(box_frame(who, f) + axis + " lw " + std::to_string(lw) + " is not int(4 sigma + 0.5) of " + std::to_string(n_in) + " -> " + std::to_string(n_out));
    if (woff < 0 || !pool || (long long)woff + lw + 1 > (long long)pool_len)
        throw ArgError(box_frame(who, f) + "the " + axis + " half-kernel at offset " + std::to_string(woff) + " ends beyond the pool of " + std::to_string(pool_len) + " doubles");
}

static void face_labels_boxes_any(const double* keypoints, const double* curves, int F, const int* desc_host, const int* desc_dev, const double* pool,
                                  int pool_len, int bw, void* workspace, long long ws_len, int OH, int OW, void* cls, void* box, bool u8, void* stream) {
    const char* who = "face_labels_boxes";
    if ((!cls && !box) || (cls && !curves) || (box && !keypoints) || !desc_host || !desc_dev || !workspace) throw ArgError("face_labels_boxes: null tensor");
    if (F < 1 || 2 * (long long)F > 65535) throw ArgError("face_labels_boxes: F must be 1 .. 32767 (two images per frame along the grid's y)");
    if (bw < 1) throw ArgError("face_labels_boxes: bw must be at least 1");
    if (OH < 1 || OW < 1 || (double)OH * OW >= 2147483647.0 / 4) throw ArgError("face_labels_boxes: bad output shape");
    if (pool_len < 0 || ws_len < 0) throw ArgError("face_labels_boxes: negative pool or workspace length");
    if (((uintptr_t)workspace & 3) != 0) throw ArgError("face_labels_boxes: the workspace must be 4-byte aligned");
    if (16ll * F > ws_len) throw ArgError("face_labels_boxes: the workspace of " + std::to_string(ws_len) + " bytes cannot hold the " + std::to_string(2 * F) + " min / max pairs");
    std::vector<std::pair<long long, int>> starts((size_t)F);         // (offset, frame)
    int max_hw = 0;
    bool pass[2] = {false, false};
    for (int f = 0; f < F; ++f) {
        const int* d = desc_host + (size_t)f * kTlDesc;
        const int h = d[0], w = d[1];
        if (h < 1 || w < 1 || h > kTlMaxSide || w > kTlMaxSide) throw ArgError(box_frame(who, f) + "crop of " + std::to_string(h) + " x " + std::to_string(w) + " (h x w): sides must be 1 .. 32767");
        check_label_axis(who, f, "rows", h, OH, d[3], d[4], pool, pool_len);
        check_label_axis(who, f, "columns", w, OW, d[5], d[6], pool, pool_len);
        const long long off = d[2], end = off + 4ll * h * w;
        if (off < 16ll * F) throw ArgError(box_frame(who, f) + "its workspace region at offset " + std::to_string(off) + " overlaps the " + std::to_string(2 * F) + " min / max pairs");
        if (end > ws_len) throw ArgError(box_frame(who, f) + "its workspace region ends at " + std::to_string(end) + ", beyond the workspace of " + std::to_string(ws_len) + " bytes");
        starts[(size_t)f] = {off, f};
        max_hw = std::max(max_hw, h * w);
        pass[0] = pass[0] || d[3] > 0; pass[1] = pass[1] || d[5] > 0;
    }
    std::sort(starts.begin(), starts.end());
    for (int i = 1; i < F; ++i) {
        const int p = starts[(size_t)i - 1].second, f = starts[(size_t)i].second;
        const int* dp = desc_host + (size_t)p * kTlDesc;
        if (starts[(size_t)i - 1].first + 4ll * dp[0] * dp[1] > starts[(size_t)i].first)
            throw ArgError(box_frame(who, std::max(p, f)) + "its workspace region overlaps that of frame " + std::to_string(std::min(p, f)));
    }
    hipStream_t s = (hipStream_t)stream;
    TrackLabelArgs a{keypoints, curves, desc_dev, pool, static_cast<unsigned char*>(workspace), ws_len, pool_len, F, bw, OH, OW,
                     cls ? 0 : 1, (cls ? 1 : 0) + (box ? 1 : 0), {cls, box}};
    const unsigned px = (unsigned)((max_hw + 255) / 256), images = (unsigned)(a.nmaps * F);
    hipLaunchKernelGGL(track_fill_kernel, dim3((max_hw + 1023) / 1024, F), dim3(256), 0, s, a);
    check_launch("track_fill");
    if (cls) {
        hipLaunchKernelGGL(track_edges_kernel, dim3(kFaceSubEdges, F), dim3(64), 0, s, a);
        check_launch("track_edges");
    }
    for (int axis = 0; axis < 2; ++axis) {
        if (!pass[axis]) continue;                                   // no frame of the call takes this pass
        hipLaunchKernelGGL(track_gauss_kernel, dim3(px, images), dim3(256), 0, s, a, axis);
        check_launch("track_gauss");
    }
    hipLaunchKernelGGL(track_minmax_kernel, dim3(std::min(64u, px), images), dim3(256), 0, s, a);
    check_launch("track_minmax");
    const dim3 grid((OH * OW + 255) / 256, images);
    if (u8) hipLaunchKernelGGL(track_resize_kernel<true>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(track_resize_kernel<false>, grid, dim3(256), 0, s, a);
    check_launch("track_resize");
}

int tsnet_face_labels_boxes(const double* keypoints, const double* curves, int F, const int* desc_host, const int* desc_dev, const double* pool, int pool_len,
                            int bw, void* workspace, long long workspace_len, int OH, int OW, float* labels, float* masks, void* stream) {
    OP_BEGIN
    face_labels_boxes_any(keypoints, curves, F, desc_host, desc_dev, pool, pool_len, bw, workspace, workspace_len, OH, OW, labels, masks, false, stream);
    OP_END
}

int tsnet_face_labels_boxes_u8(const double* keypoints, const double* curves, int F, const int* desc_host, const int* desc_dev, const double* pool, int pool_len,
                               int bw, void* workspace, long long workspace_len, int OH, int OW, unsigned char* labels, unsigned char* masks, void* stream) {
    OP_BEGIN
    face_labels_boxes_any(keypoints, curves, F, desc_host, desc_dev, pool, pool_len, bw, workspace, workspace_len, OH, OW, labels, masks, true, stream);
    OP_END
}

}  // extern "C"
