// face_adapt.hpp -- HOST code: the key-point preparation of a cross-identity face pair, as the reference's test loader does it between reading
// a driving clip's 68 landmarks and drawing its edge maps (dataset/dataset_video_face.py FaceDatasetTest.__getitem__):
//   normalize_faces (:335, :355, :411-454)  the subject clip's face proportions ("reference") are measured per mirror-symmetric landmark group,
//                                           and every group of every driving frame is re-scaled to them;
//   the moving average (:357-379)           five frames, through a running sum over the clip.
// A few hundred double operations per frame, once per clip: no kernel.  The arithmetic is the reference's, operation for operation, so that
// the result carries its bits (tests/test_face_crossid.py, == on doubles against tests/golden/g12_face_crossid.npz):
//   * every sum is sequential, frames outer, a group's points inner (Python's sum() over a list built in that order; np.mean / np.cumsum along
//     the outer axis of a short array);
//   * a centroid is sum / n, a distance sqrt(dx*dx + dy*dy) (np.linalg.norm of a 2-vector), nothing contracted (-ffp-contract=off);
//   * ref / mean / img_scale divides twice, in that order; a moved point is ((p - c) * sx + (c - fc) * sy) + fc.
// Every function returns NULL or the message of the argument it refuses; nothing is written in that case.
#pragma once
#include <cmath>
#include <vector>

namespace tsnet {
namespace face_adapt {

constexpr int kPoints = 68, kGroups = 38, kStats = 2 * kGroups + 1;       // stats: ref_dist_x[38] | ref_dist_y[38] | face width of the first frame
constexpr int kCentre = 8;                                                 // central_keypoints (:412): the chin
// part_list of normalize_faces (:418-424), -1 = no further point.  A centroid sums its points in this order ({7, 9, 8}).
static const signed char kGroupTable[kGroups][3] = {
    {0, 16, -1}, {1, 15, -1}, {2, 14, -1}, {3, 13, -1}, {4, 12, -1}, {5, 11, -1}, {6, 10, -1}, {7, 9, 8},                   // face
    {17, 26, -1}, {18, 25, -1}, {19, 24, -1}, {20, 23, -1}, {21, 22, -1},                                                  // eyebrows
    {27, -1, -1}, {28, -1, -1}, {29, -1, -1}, {30, -1, -1}, {31, 35, -1}, {32, 34, -1}, {33, -1, -1},                       // nose
    {36, 45, -1}, {37, 44, -1}, {38, 43, -1}, {39, 42, -1}, {40, 47, -1}, {41, 46, -1},                                    // eyes
    {48, 54, -1}, {49, 53, -1}, {50, 52, -1}, {51, -1, -1}, {55, 59, -1}, {56, 58, -1}, {57, -1, -1},                       // mouth
    {60, 64, -1}, {61, 63, -1}, {62, -1, -1}, {65, 67, -1}, {66, -1, -1}};                                                 // tongue

inline int group_size(int g) { return kGroupTable[g][1] < 0 ? 1 : (kGroupTable[g][2] < 0 ? 2 : 3); }

inline bool all_finite(const double* v, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

// np.mean(keypoints[pts_idx], axis=0) of one frame
inline void centroid(const double* frame, int g, double& cx, double& cy) {
    const int n = group_size(g);
    double sx = frame[2 * kGroupTable[g][0]], sy = frame[2 * kGroupTable[g][0] + 1];
    for (int i = 1; i < n; ++i) { sx = sx + frame[2 * kGroupTable[g][i]]; sy = sy + frame[2 * kGroupTable[g][i] + 1]; }
    cx = sx / (double)n; cy = sy / (double)n;
}

// face_centers (:413): landmark 8 of every frame, taken before any point moves (8 is itself in a group)
inline std::vector<double> face_centres(const double* kp, int F) {
    std::vector<double> fc((size_t)F * 2);
    for (int f = 0; f < F; ++f) { fc[2 * f] = kp[((size_t)f * kPoints + kCentre) * 2]; fc[2 * f + 1] = kp[((size_t)f * kPoints + kCentre) * 2 + 1]; }
    return fc;
}

// mean_dist_x, mean_dist_y of group g over a clip (:428-437): the mean over frames and points of |point - centroid| and of
// |centroid - face centre| (counted once per point), each plus 1e-3
inline void group_means(const double* kp, const double* fc, int F, int g, double& mean_x, double& mean_y) {
    const int n = group_size(g);
    double sum_x = 0.0, sum_y = 0.0;
    for (int f = 0; f < F; ++f) {
        const double* fr = kp + (size_t)f * kPoints * 2;
        double cx, cy;
        centroid(fr, g, cx, cy);
        const double ex = cx - fc[2 * f], ey = cy - fc[2 * f + 1];
        const double off = std::sqrt(ex * ex + ey * ey);
        for (int i = 0; i < n; ++i) {
            const double dx = fr[2 * kGroupTable[g][i]] - cx, dy = fr[2 * kGroupTable[g][i] + 1] - cy;
            sum_x = sum_x + std::sqrt(dx * dx + dy * dy);
            sum_y = sum_y + off;
        }
    }
    const double count = (double)((long long)F * n);
    mean_x = sum_x / count + 1e-3;
    mean_y = sum_y / count + 1e-3;
}

// all_keypoints[0][:, 0].max() - all_keypoints[0][:, 0].min()
inline double first_frame_width(const double* kp) {
    double lo = kp[0], hi = kp[0];
    for (int p = 1; p < kPoints; ++p) { const double x = kp[2 * p]; if (x < lo) lo = x; if (x > hi) hi = x; }
    return hi - lo;
}

// normalize_faces(is_ref=True): the subject clip.  kp (F,68,2) relative to the crop; stats[77].
inline const char* stats(const double* kp, int F, double* out) {
    if (!kp || !out) return "face_adapt_stats: null pointer";
    if (F < 1) return "face_adapt_stats: needs at least one frame";
    if (!all_finite(kp, (size_t)F * kPoints * 2)) return "face_adapt_stats: non-finite key point";
    const std::vector<double> fc = face_centres(kp, F);
    for (int g = 0; g < kGroups; ++g) group_means(kp, fc.data(), F, g, out[g], out[kGroups + g]);
    out[2 * kGroups] = first_frame_width(kp);
    return nullptr;
}

// normalize_faces(is_ref=False): the driving clip, in place.
inline const char* apply(const double* st, double* kp, int F) {
    if (!st || !kp) return "face_adapt_apply: null pointer";
    if (F < 1) return "face_adapt_apply: needs at least one frame";
    if (!all_finite(st, kStats)) return "face_adapt_apply: non-finite statistics";
    if (!all_finite(kp, (size_t)F * kPoints * 2)) return "face_adapt_apply: non-finite key point";
    const double width = first_frame_width(kp);
    if (!(width > 0.0) || !std::isfinite(width)) return "face_adapt_apply: the driving clip's first frame has no width";
    const double img_scale = st[2 * kGroups] / width;                      // :416
    if (!(img_scale > 0.0) || !std::isfinite(img_scale)) return "face_adapt_apply: the subject's face width must be positive";
    const std::vector<double> fc = face_centres(kp, F);
    // the groups are disjoint and a group's statistics read its own points only (the centres come from fc), so group by group in place
    // is the reference's order of reads and writes
    for (int g = 0; g < kGroups; ++g) {
        const int n = group_size(g);
        double mean_x, mean_y;
        group_means(kp, fc.data(), F, g, mean_x, mean_y);
        const double sx = st[g] / mean_x / img_scale, sy = st[kGroups + g] / mean_y / img_scale;      // :444-445
        for (int f = 0; f < F; ++f) {
            double* fr = kp + (size_t)f * kPoints * 2;
            double cx, cy;
            centroid(fr, g, cx, cy);
            const double ox = (cx - fc[2 * f]) * sy, oy = (cy - fc[2 * f + 1]) * sy;
            for (int i = 0; i < n; ++i) {                                   // :451-453
                double* p = fr + 2 * kGroupTable[g][i];
                p[0] = ((p[0] - cx) * sx + ox) + fc[2 * f];
                p[1] = ((p[1] - cy) * sx + oy) + fc[2 * f + 1];
            }
        }
    }
    return nullptr;
}

// The loader's moving average (:357-379) of (F, P, 2) key points over the frames, per point and coordinate, through the running sum c:
// out[0] = in[0], out[1] = c[2] / 3, out[2] = c[4] / 5, out[i] = (c[i+2] - c[i-3]) / 5 for 3 <= i <= F-3, out[F-2] = (c[F-1] - c[F-4]) / 3,
// out[F-1] = in[F-1].  The differences of running sums are part of the bits: not a windowed sum.  out may be in.
inline const char* smooth(const double* in, int F, int P, double* out) {
    if (!in || !out) return "smooth_keypoints: null pointer";
    if (P < 1) return "smooth_keypoints: needs at least one point";
    if (F < 5) return "smooth_keypoints: needs at least five frames (the reference's window)";
    const size_t cols = (size_t)P * 2;
    if (!all_finite(in, (size_t)F * cols)) return "smooth_keypoints: non-finite key point";
    std::vector<double> c(F);
    for (size_t j = 0; j < cols; ++j) {
        c[0] = in[j];
        for (int i = 1; i < F; ++i) c[i] = c[i - 1] + in[(size_t)i * cols + j];       // np.cumsum
        const double last = in[(size_t)(F - 1) * cols + j];
        out[j] = c[0];
        out[cols + j] = c[2] / 3.0;
        out[2 * cols + j] = c[4] / 5.0;
        for (int i = 3; i < F - 2; ++i) out[(size_t)i * cols + j] = (c[i + 2] - c[i - 3]) / 5.0;
        out[(size_t)(F - 2) * cols + j] = (c[F - 1] - c[F - 4]) / 3.0;
        out[(size_t)(F - 1) * cols + j] = last;
    }
    return nullptr;
}

}  // namespace face_adapt
}  // namespace tsnet
