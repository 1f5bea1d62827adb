// yuv_frames.hpp -- packed RGB frames <-> planar YUV 4:2:0 on the device: what crosses PCIe at both ends of a clip at 1.5 bytes per pixel instead
// of 3, in the form every encoder and decoder speaks (I420: a Y4M frame's payload; NV12: the hardware codecs').  The contract is INTEGER
// arithmetic on 16-bit fixed-point tables (include/tsnet_abi.h states it, tests/yuv_cases.py restates it in numpy, the tests hold equality):
//   forward  Y = clamp((cR R + cG G + cB B + (off << 16) + 32768) >> 16), per pixel;
//            C = clamp((S (4 / n) + (off << 18) + (1 << 17)) >> 18), S the sum of cR R + cG G + cB B over the n = 4, 2 or 1 pixels of the 2 x 2
//            block that lie inside the frame: ONE rounding of the block's mean chroma, centred (JPEG) siting;
//   inverse  the chroma sample of pixel (y, x) is the one at (y >> 1, x >> 1), replicated; t = (Y - oy) iy, u = Cb - 128, v = Cr - 128,
//            R = clamp((t + rv v + 32768) >> 16), G = clamp((t + gu u + gv v + 32768) >> 16), B = clamp((t + bu u + 32768) >> 16).
// Everything fits 32 bits for the tables the launcher lets through (yuv_fwd_table_ok, yuv_inv_table_ok).
//
// These kernels move bytes and nothing else: no LDS, no cross-lane traffic.  A lane owns a block of 8 pixels by 2 rows -- per row 24 RGB bytes
// and 8 Y bytes, and 4 bytes of each chroma plane (8 interleaved bytes in NV12).  The lanes are numbered over (chroma row, block column) jointly,
// so a wavefront covers 64 consecutive blocks of a row and runs on into the next one: no lane idles at the right edge of a narrow frame.
// Every run of bytes a lane owns is moved by yuv_ld / yuv_st.  A WHOLE run whose address is a multiple of 8 or 4 goes as 8- or 4-byte accesses;
// a ragged run (right and bottom edges) and a run that starts off a multiple of 4 (rows of a width that is no multiple of 4, frames of odd size
// after the first, chroma rows of odd width) go byte by byte with every byte checked against the run's length.  Both fill and drain the same
// registers, a byte outside the frame reads as 0 (it adds 0 to S), and the arithmetic between them is one piece of code: the two paths cannot
// give different bytes.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

namespace tsnet {

constexpr int kYuvBlockW = 8;            // pixels per lane along x (and 2 rows): 24 + 24 RGB bytes, 8 + 8 Y bytes, 4 + 4 chroma bytes
constexpr int kYuvRowSumMax = 1 << 17;   // the largest sum of |c| over a forward row: 4 pixels x 255 x that, plus offset and rounding, < 2^31
constexpr int kYuvInvCoefMax = 1 << 21;  // the largest |c| of an inverse table: 255 iy + 128 (|gu| + |gv|) + rounding < 2^31
constexpr int kYuvMaxFrames = 65535;     // grid.y

// HOST.  The tables of a (standard, range) pair, computed in double: tsnet_yuv_coeffs' body.  false: an unknown standard.
inline bool yuv_tables(int standard, int full_range, int* fwd, int* inv) {
    double kr, kb;
    if (standard == 601) { kr = 0.299; kb = 0.114; }
    else if (standard == 709) { kr = 0.2126; kb = 0.0722; }
    else return false;
    const double kg = 1.0 - kr - kb;
    const double sy = full_range ? 1.0 : 219.0 / 255.0, sc = full_range ? 1.0 : 224.0 / 255.0;
    const int oy = full_range ? 0 : 16;
    auto rnd = [](double v) { return (int)std::floor(v * 65536.0 + 0.5); };
    const double rows[3][3] = {{sy * kr, sy * kg, sy * kb},
                               {sc * -kr / (2.0 * (1.0 - kb)), sc * -kg / (2.0 * (1.0 - kb)), sc * (1.0 - kb) / (2.0 * (1.0 - kb))},
                               {sc * (1.0 - kr) / (2.0 * (1.0 - kr)), sc * -kg / (2.0 * (1.0 - kr)), sc * -kb / (2.0 * (1.0 - kr))}};
    const int sums[3] = {rnd(sy), 0, 0}, offs[3] = {oy, 128, 128};
    for (int r = 0; r < 3; ++r) {
        int* o = fwd + 4 * r;
        o[0] = rnd(rows[r][0]); o[2] = rnd(rows[r][2]);
        o[1] = sums[r] - o[0] - o[2];                                    // the green entry carries the row's rounding: grey has chroma 128 exactly
        o[3] = offs[r];
    }
    inv[0] = rnd(1.0 / sy);
    inv[1] = rnd(2.0 * (1.0 - kr) / sc);
    inv[2] = -rnd(kb * 2.0 * (1.0 - kb) / (kg * sc));
    inv[3] = -rnd(kr * 2.0 * (1.0 - kr) / (kg * sc));
    inv[4] = rnd(2.0 * (1.0 - kb) / sc);
    inv[5] = oy;
    return true;
}

// HOST.  The launcher's overflow bounds.
inline bool yuv_fwd_row_fits(const int* row) {
    long long s = 0;
    for (int i = 0; i < 3; ++i) s += row[i] < 0 ? -(long long)row[i] : (long long)row[i];
    return s <= kYuvRowSumMax;
}
inline bool yuv_inv_coef_fits(int c) { return c >= -kYuvInvCoefMax && c <= kYuvInvCoefMax; }

struct YuvArgs {
    const unsigned char* src;            // forward: (F, h, w, 3) RGB; inverse: F frames of h w + 2 ch cw bytes
    unsigned char* dst;
    int h, w, ch, cw;                    // ch = (h + 1) / 2, cw = (w + 1) / 2
    int nbx;                             // lane blocks per row: ceil(w / 8)
    int nv12;                            // 0: I420 (Y, Cb, Cr planes), 1: NV12 (Y plane, interleaved Cb Cr rows)
    int c[12];                           // forward: three rows {cR, cG, cB, offset}; inverse: {iy, rv, gu, gv, bu, oy}
};

template <class T>
__device__ __forceinline__ T yuv_ld_as(const unsigned char* p) {
    T v;
    __builtin_memcpy(&v, __builtin_assume_aligned(p, sizeof(T)), sizeof(T));
    return v;
}
template <class T>
__device__ __forceinline__ void yuv_st_as(unsigned char* p, T v) {
    __builtin_memcpy(__builtin_assume_aligned(p, sizeof(T)), &v, sizeof(T));
}

// A run of 4 DW bytes at p of which the first n exist (0 <= n <= 4 DW), little-endian in d[0 .. DW); what does not exist reads as 0.
template <int DW>
__device__ __forceinline__ void yuv_ld(const unsigned char* p, int n, unsigned (&d)[DW]) {
    const unsigned al = (unsigned)(uintptr_t)p;
    if (n == 4 * DW && DW % 2 == 0 && (al & 7u) == 0) {
#pragma unroll
        for (int k = 0; k < DW / 2; ++k) {
            const unsigned long long v = yuv_ld_as<unsigned long long>(p + 8 * k);
            d[2 * k] = (unsigned)v; d[2 * k + 1] = (unsigned)(v >> 32);
        }
    } else if (n == 4 * DW && (al & 3u) == 0) {
#pragma unroll
        for (int k = 0; k < DW; ++k) d[k] = yuv_ld_as<unsigned>(p + 4 * k);
    } else {
#pragma unroll
        for (int k = 0; k < DW; ++k) {
            unsigned v = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (4 * k + b < n) v |= (unsigned)p[4 * k + b] << (8 * b);
            d[k] = v;
        }
    }
}

// The first n bytes of d[0 .. DW) to p; nothing beyond them is written.
template <int DW>
__device__ __forceinline__ void yuv_st(unsigned char* p, int n, const unsigned (&d)[DW]) {
    const unsigned al = (unsigned)(uintptr_t)p;
    if (n == 4 * DW && DW % 2 == 0 && (al & 7u) == 0) {
#pragma unroll
        for (int k = 0; k < DW / 2; ++k) yuv_st_as<unsigned long long>(p + 8 * k, (unsigned long long)d[2 * k] | ((unsigned long long)d[2 * k + 1] << 32));
    } else if (n == 4 * DW && (al & 3u) == 0) {
#pragma unroll
        for (int k = 0; k < DW; ++k) yuv_st_as<unsigned>(p + 4 * k, d[k]);
    } else {
#pragma unroll
        for (int k = 0; k < DW; ++k)
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (4 * k + b < n) p[4 * k + b] = (unsigned char)(d[k] >> (8 * b));
    }
}

template <int DW>
__device__ __forceinline__ int yuv_byte(const unsigned (&d)[DW], int i) { return (int)((d[i >> 2] >> (8 * (i & 3))) & 0xFFu); }
template <int DW>
__device__ __forceinline__ void yuv_put(unsigned (&d)[DW], int i, int v) { d[i >> 2] |= (unsigned)v << (8 * (i & 3)); }
__device__ __forceinline__ int yuv_clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// The lane's block: frame f, chroma row j (pixel rows 2j, 2j + 1), block column bx (pixels 8 bx ..).  false: the lane is beyond the frame.
__device__ __forceinline__ bool yuv_lane_block(const YuvArgs& a, int& j, int& bx) {
    const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
    j = (int)(t / (unsigned)a.nbx);
    bx = (int)(t - (unsigned)j * (unsigned)a.nbx);
    return j < a.ch;
}

// grid = (ceil(nbx ch / 256), F), 256 threads.
__global__ __launch_bounds__(256) void rgb_to_yuv420_kernel(YuvArgs a) {
    int j, bx;
    if (!yuv_lane_block(a, j, bx)) return;
    const int x0 = bx * kYuvBlockW, y0 = 2 * j;
    const int nx = a.w - x0 > kYuvBlockW ? kYuvBlockW : a.w - x0;        // 1 .. 8 pixels of the block inside the frame
    const int ny = a.h - y0 > 1 ? 2 : 1;
    const size_t plane = (size_t)a.h * a.w, cplane = (size_t)a.ch * a.cw;
    const unsigned char* rgb = a.src + (size_t)blockIdx.y * plane * 3;
    unsigned char* yuv = a.dst + (size_t)blockIdx.y * (plane + 2 * cplane);
    unsigned px[2][6], yy[2][2] = {{0u, 0u}, {0u, 0u}};
    yuv_ld<6>(rgb + ((size_t)y0 * a.w + x0) * 3, 3 * nx, px[0]);
    yuv_ld<6>(rgb + ((size_t)(y0 + ny - 1) * a.w + x0) * 3, ny == 2 ? 3 * nx : 0, px[1]);
    int su[4] = {0, 0, 0, 0}, sv[4] = {0, 0, 0, 0};
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int i = 0; i < kYuvBlockW; ++i) {
            const int R = yuv_byte<6>(px[r], 3 * i), G = yuv_byte<6>(px[r], 3 * i + 1), B = yuv_byte<6>(px[r], 3 * i + 2);
            yuv_put<2>(yy[r], i, yuv_clip8((a.c[0] * R + a.c[1] * G + a.c[2] * B + (a.c[3] << 16) + 32768) >> 16));
            su[i >> 1] += a.c[4] * R + a.c[5] * G + a.c[6] * B;          // a pixel outside the frame is 0, 0, 0 and adds nothing
            sv[i >> 1] += a.c[8] * R + a.c[9] * G + a.c[10] * B;
        }
    yuv_st<2>(yuv + (size_t)y0 * a.w + x0, nx, yy[0]);
    yuv_st<2>(yuv + (size_t)(y0 + ny - 1) * a.w + x0, ny == 2 ? nx : 0, yy[1]);
    unsigned cb[1] = {0u}, cr[1] = {0u}, uv[2] = {0u, 0u};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = (ny == 2 ? 1 : 2) * (nx - 2 * i >= 2 ? 1 : 2);     // 4 / n
        const int u = yuv_clip8((su[i] * m + (a.c[7] << 18) + (1 << 17)) >> 18), v = yuv_clip8((sv[i] * m + (a.c[11] << 18) + (1 << 17)) >> 18);
        yuv_put<1>(cb, i, u); yuv_put<1>(cr, i, v);
        yuv_put<2>(uv, 2 * i, u); yuv_put<2>(uv, 2 * i + 1, v);
    }
    const int i0 = bx * (kYuvBlockW / 2);
    const int nc = (nx + 1) >> 1;                                        // 1 .. 4 chroma samples of the block inside the plane
    const size_t at = (size_t)j * a.cw + i0;
    if (a.nv12) {
        yuv_st<2>(yuv + plane + 2 * at, 2 * nc, uv);
    } else {
        yuv_st<1>(yuv + plane + at, nc, cb);
        yuv_st<1>(yuv + plane + cplane + at, nc, cr);
    }
}

__global__ __launch_bounds__(256) void yuv420_to_rgb_kernel(YuvArgs a) {
    int j, bx;
    if (!yuv_lane_block(a, j, bx)) return;
    const int x0 = bx * kYuvBlockW, y0 = 2 * j;
    const int nx = a.w - x0 > kYuvBlockW ? kYuvBlockW : a.w - x0;
    const int ny = a.h - y0 > 1 ? 2 : 1;
    const size_t plane = (size_t)a.h * a.w, cplane = (size_t)a.ch * a.cw;
    const unsigned char* yuv = a.src + (size_t)blockIdx.y * (plane + 2 * cplane);
    unsigned char* rgb = a.dst + (size_t)blockIdx.y * plane * 3;
    unsigned yy[2][2], cb[1], cr[1];
    yuv_ld<2>(yuv + (size_t)y0 * a.w + x0, nx, yy[0]);
    yuv_ld<2>(yuv + (size_t)(y0 + ny - 1) * a.w + x0, ny == 2 ? nx : 0, yy[1]);
    const int i0 = bx * (kYuvBlockW / 2);
    const int nc = (nx + 1) >> 1;
    const size_t at = (size_t)j * a.cw + i0;
    if (a.nv12) {
        unsigned uv[2];
        yuv_ld<2>(yuv + plane + 2 * at, 2 * nc, uv);
        cb[0] = cr[0] = 0u;
#pragma unroll
        for (int i = 0; i < 4; ++i) { yuv_put<1>(cb, i, yuv_byte<2>(uv, 2 * i)); yuv_put<1>(cr, i, yuv_byte<2>(uv, 2 * i + 1)); }
    } else {
        yuv_ld<1>(yuv + plane + at, nc, cb);
        yuv_ld<1>(yuv + plane + cplane + at, nc, cr);
    }
    unsigned px[2][6] = {{0u, 0u, 0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u, 0u, 0u}};
#pragma unroll
    for (int i = 0; i < kYuvBlockW; ++i) {
        const int u = yuv_byte<1>(cb, i >> 1) - 128, v = yuv_byte<1>(cr, i >> 1) - 128;
        const int dr = a.c[1] * v + 32768, dg = a.c[2] * u + a.c[3] * v + 32768, db = a.c[4] * u + 32768;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int t = (yuv_byte<2>(yy[r], i) - a.c[5]) * a.c[0];
            yuv_put<6>(px[r], 3 * i, yuv_clip8((t + dr) >> 16));
            yuv_put<6>(px[r], 3 * i + 1, yuv_clip8((t + dg) >> 16));
            yuv_put<6>(px[r], 3 * i + 2, yuv_clip8((t + db) >> 16));
        }
    }
    yuv_st<6>(rgb + ((size_t)y0 * a.w + x0) * 3, 3 * nx, px[0]);
    yuv_st<6>(rgb + ((size_t)(y0 + ny - 1) * a.w + x0) * 3, ny == 2 ? 3 * nx : 0, px[1]);
}

}  // namespace tsnet
