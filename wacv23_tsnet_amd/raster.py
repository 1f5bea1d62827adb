"""Host side of the device rasterisation: key-point files of a clip -> the label tensors
`set_test_input` takes.  The reference does this per frame on the CPU in its data loader
(dataset/dataset_video_face.py:283-330, FaceDatasetTest.__getitem__); here the key points of a whole clip go to the device once
and three kernels (csrc/raster.hpp) produce every frame's edge map, bounding-box mask and one-hot label.  With a crop per frame
(fix_crop_pos=False) the frames have different sizes; their labels at the model's resolution are still one call (csrc/track_labels.hpp).

Only the crop arithmetic (a handful of integer operations per clip, dataset_video_face.py:507-518) stays on the host, and for a
cross-identity pair the loader's key-point preparation of the driving clip (`FaceAdapter`, `smooth_keypoints`, `face_driving_keypoints`:
normalize_faces :411-454 and the five-frame moving average :357-379), a few hundred double operations per frame in the library's host code.

Pose clips (dataset/dataset_video_pose.py:304-461, PoseDatasetTestVideo.__getitem__): `PoseRasteriser` takes the OpenPose points of a clip to the
device once; the colour-coded skeleton (as class indices), its crop, the bounding-box mask, the nearest-neighbour resize to 128 x 256, the
padding to 256 x 256 and the one-hot label are kernels.  The host keeps what is per-person arithmetic on 137 points: the confidence
thresholds, the choice of the person, the crop rectangle, the temporal smoothing of a driving clip, the limb re-scaling of opposite-sex pairs and the
two index tables of the resize.  (The loader-side preprocessing of a driving clip -- five-frame smoothing, shift into the crop, limb re-scaling of
opposite-sex pairs: SURVEY.md section 2 marks it out of scope -- lives in tools/pose_preprocess.py, outside the product package.)"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._call import Wrapper, call


def read_keypoints(path: str) -> np.ndarray:
    """68 x 2 landmark file of the demo clips: one 'x,y' pair per line (FaceDatasetTest.read_data, :457: np.loadtxt(delimiter=','))."""
    return np.loadtxt(path, delimiter=",")


def crop_coords(keypoints: np.ndarray) -> Tuple[int, int, int, int]:
    """FaceDatasetTest.get_crop_coords (:507-518): a square of twice the face width around the landmarks -> (min_y, max_y, min_x, max_x)."""
    min_y, max_y = int(keypoints[:, 1].min()), int(keypoints[:, 1].max())
    min_x, max_x = int(keypoints[:, 0].min()), int(keypoints[:, 0].max())
    x_cen, y_cen = (min_x + max_x) // 2, (min_y + max_y) // 2
    side = max_x - min_x
    x0 = x_cen - side
    y0 = y_cen - side * 1.25
    return int(y0), int(y0 + side * 2), int(x0), int(x0 + side * 2)


def crop_coords_clip(keypoints: Sequence[np.ndarray]) -> np.ndarray:
    """`crop_coords` of every frame -> (F,4) int64 rows (min_y, max_y, min_x, max_x): the crops of FaceDatasetTest(fix_crop_pos=False)
    (:303-305, :348-350).  The reference does not smooth them over time, and neither does this."""
    return np.array([crop_coords(np.asarray(k)) for k in keypoints], dtype=np.int64).reshape(-1, 4)


def _clip_array(kps, what: Optional[str] = None) -> np.ndarray:
    """F arrays (68,2) -> a new contiguous (F,68,2) float64 array"""
    kp = np.ascontiguousarray(np.stack([np.asarray(k, dtype=np.float64) for k in kps]))
    if kp.ndim != 3 or kp.shape[1:] != (68, 2):
        raise ValueError((f"{what}: " if what else "") + f"expected F x 68 x 2 key points, got {kp.shape}")
    return kp


def _face_points(keypoints, crop=None, relative: bool = False, bw: Optional[int] = None, lib=None):
    """The front half of everything that takes a clip's key points: -> (points (F,68,2) float64 relative to their crop, the crop or (F,4)
    int64 crops, bw, the fitted curves (F,34,8) -- None when no lib is given).
    crop: (min_y, max_y, min_x, max_x), default crop_coords of the first frame (fix_crop_pos=True, :294-299), or (F,4), one per frame
    (fix_crop_pos=False); relative=True: the points are relative already and go on untouched.  bw defaults to max(1, h // 256) of the
    crop (:295), the FIRST frame's when there is one per frame: the reference computes the brush once per clip (:302, :347)."""
    kp = _clip_array(keypoints)
    F = kp.shape[0]
    if relative and crop is None:
        raise ValueError("relative=True: key points relative to a crop need that crop")
    if crop is None:
        crop = crop_coords(kp[0])
    if np.ndim(crop) == 2:
        crop = np.asarray(crop).astype(np.int64)
        if crop.shape != (F, 4):
            raise ValueError(f"expected ({F},4) crops for {F} frames, got {crop.shape}")
        top, left, h = crop[:, 0, None], crop[:, 2, None], int(crop[0, 1] - crop[0, 0])
    else:
        top, left, h = crop[0], crop[2], crop[1] - crop[0]
    if not relative:
        kp[:, :, 0] -= left                                        # read_keypoints (:497-507): each frame by its crop
        kp[:, :, 1] -= top
    if bw is None:
        bw = max(1, h // 256)
    curves = None
    if lib is not None:
        # interp_points' Levenberg-Marquardt fits run on the host (34 per frame, microseconds each; csrc/lmfit.hpp reproduces scipy's
        # curve_fit to the last bit); the device samples and draws the fitted curves
        curves = np.empty((F, 34, 8), dtype=np.float64)
        call(lib, "tsnet_fit_face_curves", kp.ctypes.data, F, curves.ctypes.data)
    return kp, crop, bw, curves


class FaceRasteriser(Wrapper):
    """Edge maps / bounding-box masks of a clip at crop resolution, and one-hot labels, on `device`.

    lib: tests pass the CPU emulation build; product code leaves it None (the in-tree HIP library, no fallback)."""

    def __init__(self, device, lib=None):
        super().__init__(device, lib)
        self._wpool_host = np.zeros(0, np.float64)                   # the Gaussian half-kernels of the per-frame-crop labels, one after the other
        self._wpool_at = {}                                          # (n_in, n_out) -> (lw, offset in doubles)
        self._wpool = None                                           # the device copy; replaced (never written) when the pool has grown
        self._ws = None                                              # the workspace of tsnet_face_labels_boxes; replaced when a clip needs more

    def _draw(self, kp: np.ndarray, curves: np.ndarray, h: int, w: int, bw: int):
        """frames of one size: (edges (F,h,w) uint8, bbox (F,h,w) uint8, the two uploads)"""
        F = kp.shape[0]
        kd = torch.from_numpy(kp).to(self.device)
        cd = torch.from_numpy(curves).to(self.device)
        edges = torch.empty((F, h, w), dtype=torch.uint8, device=self.device)
        bbox = torch.empty((F, h, w), dtype=torch.uint8, device=self.device)
        call(self.lib, "tsnet_raster_face", kd.data_ptr(), cd.data_ptr(), F, h, w, bw, edges.data_ptr(), bbox.data_ptr(), device=self.device)
        return edges, bbox, (kd, cd)

    def rasterise(self, keypoints: Sequence[np.ndarray], crop: Optional[Tuple[int, int, int, int]] = None, relative: bool = False,
                  bw: Optional[int] = None):
        """keypoints: F arrays (68,2) in frame coordinates.  crop: (min_y, max_y, min_x, max_x); default = crop_coords of the first
        frame (fix_crop_pos=True, :294-299).  relative=True: the points are already relative to `crop` (which must be given) and go to the
        fit untouched -- the way for fractional points such as face_driving_keypoints', where (a + c) - c is not a.
        bw: the brush width, default max(1, h // 256) of the crop.
        Returns (edges (F,h,w) uint8, bbox (F,h,w) uint8, crop, bw).
        crop may be an (F,4) array, a crop per frame (fix_crop_pos=False, `crop_coords_clip`): every frame is drawn at its own crop's size and the
        result is (edges, bbox, crops, bw) with edges / bbox LISTS of F tensors (h_f, w_f).  bw then defaults to that of the FIRST frame's crop:
        the reference computes the brush once per clip (:302, :347).  Frames of equal size share one call of the kernels."""
        kp, crop, bw, curves = _face_points(keypoints, crop, relative, bw, self.lib)
        if np.ndim(crop) == 2:                                       # the frames of every size together, and back into frame order
            edges, bbox, held = [None] * len(kp), [None] * len(kp), []
            for (h, w), idx in self._size_groups(crop).items():
                e, b, up = self._draw(kp[idx], curves[idx], h, w, bw)
                held.append(up)
                for j, f in enumerate(idx):
                    edges[f], bbox[f] = e[j], b[j]
        else:
            edges, bbox, held = self._draw(kp, curves, crop[1] - crop[0], crop[3] - crop[2], bw)
        self._held["rasterise"] = {"uploads": held}
        return edges, bbox, crop, bw

    @staticmethod
    def _size_groups(crops: np.ndarray):
        """{(h, w): [frame indices]} of (F,4) crops, in order of first appearance"""
        groups = {}
        for f, c in enumerate(crops):
            groups.setdefault((int(c[1] - c[0]), int(c[3] - c[2])), []).append(f)
        return groups

    def vl2ch(self, labels: torch.Tensor, num_classes: int) -> torch.Tensor:
        """utils/misc.py vl2ch (:50-67): (B,H,W) class indices -> (B,num_classes,H,W) one-hot float32."""
        lab = labels.to(self.device, dtype=torch.float32).contiguous()
        B, H, W = lab.shape
        out = torch.empty((B, num_classes, H, W), dtype=torch.float32, device=self.device)
        call(self.lib, "tsnet_vl2ch", lab.data_ptr(), B, H * W, num_classes, out.data_ptr(), device=self.device)
        self._held["vl2ch"] = {"labels": lab}
        return out

    def clip_labels(self, keypoints: Sequence[np.ndarray], size: Tuple[int, int] = (256, 256), crop=None, relative: bool = False,
                    compact: bool = False, bw: Optional[int] = None):
        """The label tensors of a clip as the model takes them: rasterise, then the loader's resize to `size` (demo.resize_label).
        compact=False: one-hot labels (F,2,H,W) float32 (vl2ch) and masks (F,H,W) float32 0/1.  compact=True: the class map (F,H,W) and the
        mask (F,H,W) as uint8 -- what Engine.forward_target / ClipRunner take as a compact call; no vl2ch, the stem's packing kernel makes
        the one-hot planes on load.  Returns (labels, masks, crop).
        crop may be an (F,4) array, a crop per frame (see `rasterise`); bw: the brush width, as `rasterise` takes it.  The tensors are the same
        (F, ...) ones, every frame drawn and resized at its own crop's size, and frame f has the bits of this method called on frame f alone with
        crop f and the clip's bw.  That form is ONE call of the library (`tsnet_face_labels_boxes[_u8]`, csrc/track_labels.hpp) however many
        sizes the clip has -- a clip of a single size, F = 1 included, goes the same way (measured no slower than the single-size entries:
        profiles/track_labels.txt).  Once a clip's sizes have been seen a call is one upload on the current stream (key points, fitted curves
        and descriptors in one buffer, from pageable memory as FrameLoader's descriptors are) and at most six kernels, with no allocation and
        no synchronisation inside the library; the weight pool and the workspace live on the rasteriser and are replaced when a clip needs
        more.  One stream at a time per rasteriser."""
        from .demo import resize_label
        if crop is not None and np.ndim(crop) == 2:
            cls, box, crop, held = self._clip_labels_crops(keypoints, size, crop, relative, compact, bw)
        else:
            edges, bbox, crop, _ = self.rasterise(keypoints, crop, relative, bw)
            cls, box = resize_label(edges, size, lib=self.lib), resize_label(bbox, size, lib=self.lib)
            held = {"rasterise": self._held["rasterise"]}
            if compact:
                cls, box = cls.to(torch.uint8), box.to(torch.uint8)          # exact: the maps hold 0 / 1
        if not compact:
            cls = self.vl2ch(cls, 2)
            held["vl2ch"] = self._held["vl2ch"]
        self._held["clip_labels"] = held
        return cls, box, crop

    def _aa_axis(self, n_in: int, n_out: int) -> Tuple[int, int]:
        """(lw, offset in doubles) of an axis' Gaussian half-kernel (demo._aa_kernel) in the pool, appended on first sight; (-1, 0) for an axis
        that does not shrink"""
        key = (n_in, n_out)
        if key not in self._wpool_at:
            from .demo import _aa_kernel
            lw, w = _aa_kernel(n_in, n_out)
            if lw < 0:
                self._wpool_at[key] = (-1, 0)
            else:
                self._wpool_at[key] = (lw, len(self._wpool_host))
                self._wpool_host = np.concatenate([self._wpool_host, w])
        return self._wpool_at[key]

    def _label_descriptors(self, crops: np.ndarray, size: Tuple[int, int]):
        """(host (F,8) int32 rows {h, w, off, lw_rows, woff_rows, lw_cols, woff_cols, 0}, workspace bytes) as tsnet_face_labels_boxes takes them:
        the 2F min / max pairs, then a region of 4 h w bytes per frame, each on a 64-byte boundary"""
        OH, OW = int(size[0]), int(size[1])
        F = len(crops)
        rows, off = [], (16 * F + 63) // 64 * 64
        for f, c in enumerate(crops.tolist()):                       # plain ints: this loop is per frame and per call
            h, w = c[1] - c[0], c[3] - c[2]
            if h < 1 or w < 1:
                raise ValueError(f"frame {f}: empty crop {tuple(c)}")
            (lr, wr), (lc, wc) = self._aa_axis(h, OH), self._aa_axis(w, OW)
            rows.append((h, w, off, lr, wr, lc, wc, 0))
            off += (4 * h * w + 63) // 64 * 64
            if off >= 2 ** 31:
                raise ValueError(f"frame {f}: the clip's crops need more than 2 GiB of workspace in one call; split the clip")
        return np.array(rows, dtype=np.int32).reshape(-1, 8), off

    def _clip_labels_crops(self, keypoints, size, crops, relative: bool, compact: bool, bw: Optional[int]):
        """clip_labels with a crop per frame, before vl2ch: one call of tsnet_face_labels_boxes[_u8] -> (class map, mask, crops, what it holds)"""
        kp, crops, bw, curves = _face_points(keypoints, crops, relative, bw, self.lib)
        F = kp.shape[0]
        desc, ws_len = self._label_descriptors(crops, size)
        # one upload: key points | curves | descriptors (multiples of 8 bytes, so each part is aligned for its type)
        up = torch.from_numpy(np.concatenate([kp.reshape(-1).view(np.uint8), curves.reshape(-1).view(np.uint8), desc.reshape(-1).view(np.uint8)])).to(self.device)
        kd = up.data_ptr()
        cd, dd = kd + kp.nbytes, kd + kp.nbytes + curves.nbytes
        old_pool = old_ws = None                                     # what this call replaces: an enqueued kernel may still read it
        if self._wpool is None or self._wpool.numel() != len(self._wpool_host):
            old_pool, self._wpool = self._wpool, torch.from_numpy(self._wpool_host.copy()).to(self.device)
        if self._ws is None or self._ws.numel() < ws_len:
            old_ws, self._ws = self._ws, torch.empty(ws_len, dtype=torch.uint8, device=self.device)
        OH, OW = int(size[0]), int(size[1])
        dtype = torch.uint8 if compact else torch.float32
        cls = torch.empty((F, OH, OW), dtype=dtype, device=self.device)
        box = torch.empty((F, OH, OW), dtype=dtype, device=self.device)
        call(self.lib, "tsnet_face_labels_boxes_u8" if compact else "tsnet_face_labels_boxes", kd, cd, F, desc.ctypes.data, dd,
             self._wpool.data_ptr() if self._wpool.numel() else None, self._wpool.numel(), int(bw), self._ws.data_ptr(), self._ws.numel(),
             OH, OW, cls.data_ptr(), box.data_ptr(), device=self.device)
        return cls, box, crops, {"upload": up, "pool": self._wpool, "workspace": self._ws, "old_pool": old_pool, "old_workspace": old_ws}


# ------------------------------------------------------------------------------------------------- cross-identity face pairs
class FaceAdapter:
    """FaceDatasetTest.normalize_faces (dataset_video_face.py:411-454): `fit` measures the subject clip's face proportions (is_ref=True, :335),
    `apply` re-scales every mirror-symmetric landmark group of a driving clip to them (is_ref=False, :355).  Key points are relative to their
    clip's crop, as read_keypoints (:497-505) leaves them.  The arithmetic is host code of the library (csrc/face_adapt.hpp) and returns the
    reference's float64 bits.

    lib: tests pass the CPU emulation build; product code leaves it None (the in-tree HIP library, no fallback)."""

    def __init__(self, lib=None):
        self.lib = lib if lib is not None else _lib.load()
        self._stats = None

    @property
    def stats(self) -> np.ndarray:
        """77 doubles: ref_dist_x[38] | ref_dist_y[38] | the subject's face width in its first frame"""
        if self._stats is None:
            raise RuntimeError("FaceAdapter: fit() a subject clip first")
        return self._stats.copy()

    def fit(self, subject_kps_rel) -> "FaceAdapter":
        kp = _clip_array(subject_kps_rel, "FaceAdapter.fit")
        stats = np.empty(77, dtype=np.float64)
        call(self.lib, "tsnet_face_adapt_stats", kp.ctypes.data, kp.shape[0], stats.ctypes.data)
        self._stats = stats
        return self

    def apply(self, driving_kps_rel) -> np.ndarray:
        """-> (F,68,2) float64, a new array: the driving clip with the subject's proportions"""
        if self._stats is None:
            raise RuntimeError("FaceAdapter: fit() a subject clip first")
        kp = _clip_array(driving_kps_rel, "FaceAdapter.apply")
        call(self.lib, "tsnet_face_adapt_apply", self._stats.ctypes.data, kp.ctypes.data, kp.shape[0])
        return kp


def smooth_keypoints(kps, lib=None) -> np.ndarray:
    """The loader's five-frame moving average of a driving clip's key points over its frames (dataset_video_face.py:357-379): (F,P,2) -> a new
    (F,P,2) float64 array, the reference's bits.  F >= 5."""
    lib = lib if lib is not None else _lib.load()
    kp = np.ascontiguousarray(np.stack([np.asarray(k, dtype=np.float64) for k in kps]))
    if kp.ndim != 3 or kp.shape[2] != 2:
        raise ValueError(f"expected F x P x 2 key points, got {kp.shape}")
    out = np.empty_like(kp)
    call(lib, "tsnet_smooth_keypoints", kp.ctypes.data, kp.shape[0], kp.shape[1], out.ctypes.data)
    return out


def face_driving_keypoints(subject_kps, driving_kps, lib=None, fix_crop_pos: bool = True):
    """The driving key points of a cross-identity pair in the order FaceDatasetTest.__getitem__ prepares them (fix_crop_pos=True, as the demo
    runs): each clip is cropped by the crop of its own first frame (:299-308, :344-353), the driving clip is adapted to the subject's face
    proportions (:335, :355) and then smoothed over its frames (:357-379); the subject clip is neither adapted nor smoothed.
    subject_kps, driving_kps: F arrays (68,2) in frame coordinates, as `read_keypoints` returns them.
    Returns (points (F,68,2) float64 relative to the driving crop, driving crop (min_y, max_y, min_x, max_x), bw): what
    `FaceRasteriser.rasterise(points, crop, relative=True)` takes.
    fix_crop_pos=False: every frame of each clip is made relative to its OWN crop (read_keypoints(path, None), :306-308, :351-353, :499-507);
    adaptation and smoothing then run as above.  Returns (points, crops (F,4) of the driving frames, bw of the FIRST driving frame (:347))."""
    sub, drv = _clip_array(subject_kps, "subject"), _clip_array(driving_kps, "driving")
    sub = _face_points(sub, None if fix_crop_pos else crop_coords_clip(sub))[0]
    drv, crop, bw, _ = _face_points(drv, None if fix_crop_pos else crop_coords_clip(drv))
    return smooth_keypoints(FaceAdapter(lib).fit(sub).apply(drv), lib), crop, bw


# ---------------------------------------------------------------------------------------------------------------- pose clips
_POSE_GROUPS = (("pose_keypoints_2d", 25), ("face_keypoints_2d", 70), ("hand_left_keypoints_2d", 21), ("hand_right_keypoints_2d", 21))
_FACE_RUNS = ((0, 17), (17, 22), (22, 27), (31, 36), (48, 55))           # consecutive runs of face_list (keypoint2img_posenorm.py:439-447)
_FACE_CHAINS = ((28, 31), (35, 28), (36, 37, 38, 39), (39, 40, 41, 36), (42, 43, 44, 45), (45, 46, 47, 42), (54, 55, 56, 57, 58, 59, 48))
_FINGERS = tuple((0,) + tuple(range(4 * i + 1, 4 * i + 5)) for i in range(5))


def _usable(points: np.ndarray) -> np.ndarray:
    """extract_valid_keypoints (keypoint2img_posenorm.py:242-262): a face / hand chain is kept only if ALL its points are confident
    (> 0.1 / > 0.01); body points are kept one by one (> 0.01).  (n,3) -> (n,2), dropped points zero."""
    conf, out = points[:, 2], np.zeros((points.shape[0], 2))
    if points.shape[0] == 25:
        keep = conf > 0.01
        out[keep] = points[keep, :2]
        return out
    chains = [tuple(range(a, b)) for a, b in _FACE_RUNS] + list(_FACE_CHAINS) if points.shape[0] == 70 else _FINGERS
    thr = 0.1 if points.shape[0] == 70 else 0.01
    for chain in chains:
        idx = list(chain)
        if np.all(conf[idx] > thr):
            out[idx] = points[idx, :2]
    return out


def read_openpose(path_or_text: str) -> np.ndarray:
    """One OpenPose frame file (or its text) -> (137,2) float64: body 25 | face 70 | left hand 21 | right hand 21 of the person with the
    largest vertical extent (read_keypoints_posenorm, keypoint2img_posenorm.py:11-41); unusable points are zero."""
    import json
    import os
    text = open(path_or_text, encoding="utf-8").read() if os.path.exists(path_or_text) else path_or_text
    chosen, extent = np.zeros((137, 2)), 0.0
    for person in json.loads(text)["people"]:
        groups = [_usable(np.asarray(person[key], dtype=np.float64).reshape(n, 3)) for key, n in _POSE_GROUPS]
        span = groups[0][:, 1].max() - groups[0][:, 1].min()
        if span > extent:
            extent, chosen = span, np.concatenate(groups)
    return chosen


def pose_crop_coords(points: np.ndarray, size: Tuple[int, int], scale: float = 1.5) -> Tuple[int, int, int, int]:
    """PoseDatasetTestVideo.get_crop_coords (dataset_video_pose.py:554-588, no random offset, aspect_ratio 0.5): a box of `scale` body heights,
    half as wide, clamped into the (w, h) frame -> (xs, ys, xe, ye).  points: (137,2) or (25,2)."""
    w, h = size
    body = np.asarray(points, dtype=np.float64)[:25]
    seen = body[body[:, 0] != 0]
    if seen.shape[0]:
        x_cen = int(seen[:, 0].min() + seen[:, 0].max()) // 2
        top = max(seen[:, 1].min(), min(body[15, 1], body[16, 1]))          # not above the eyes
        bottom = max(body[11, 1], body[14, 1])                               # the ankles, if seen
        if bottom == 0:
            bottom = seen[:, 1].max()
        y_cen, height = int(top + bottom) // 2, bottom - top
    else:
        x_cen, y_cen, height = w // 2, h // 2, h // 2
    half_h = int(min(h, max(h // 4, height * scale))) // 2
    half_w = int(half_h * 0.5)
    x_cen = max(half_w, min(w - half_w, x_cen))
    y_cen = max(half_h, min(h - half_h, y_cen))
    return x_cen - half_w, y_cen - half_h, x_cen + half_w, y_cen + half_h


def nearest_table(n_in: int, n_out: int) -> np.ndarray:
    """Source index of every output index of PIL's Image.resize(.., NEAREST) along one axis: the sampling position starts at scale / 2 and is
    ADVANCED by `scale` per output pixel in double precision (libImaging Geometry.c, ImagingScaleAffine), then truncated -- the running sum,
    not (i + 0.5) * scale, decides ties.  tests/test_raster_pose.py checks the table against PIL itself."""
    scale = float(n_in) / float(n_out)
    pos, tab = scale * 0.5, np.empty(n_out, dtype=np.int32)
    for i in range(n_out):
        tab[i] = min(int(pos), n_in - 1)
        pos += scale
    return tab


class PoseRasteriser(Wrapper):
    """Class-index skeleton labels, bounding-box masks and the model's 256 x 256 label tensors of a pose clip on `device`.

    lib: tests pass the CPU emulation build; product code leaves it None (the in-tree HIP library, no fallback)."""

    def rasterise(self, points: Sequence[np.ndarray], size: Tuple[int, int], window: Optional[Tuple[int, int, int, int]] = None,
                  basic_point_only: bool = False, remove_face_labels: bool = False) -> torch.Tensor:
        """points: F arrays (137,2) in the coordinates of the (w, h) = size frame.  window (xs, ys, xe, ye): the crop that is kept
        (crop_person_region); default the whole frame.  Returns (F, ye-ys, xe-xs) uint8 class indices 0..24 on the device:
        im2vl(connect_keypoints(..)) of the reference."""
        pts = np.stack([np.asarray(p, dtype=np.float64) for p in points])
        if pts.ndim != 3 or pts.shape[1:] != (137, 2):
            raise ValueError(f"expected F x 137 x 2 points, got {pts.shape}")
        w, h = size
        xs, ys, xe, ye = window if window is not None else (0, 0, w, h)
        F = pts.shape[0]
        n = F * (ye - ys) * (xe - xs)
        pts = np.ascontiguousarray(pts)
        flags = (1 if basic_point_only else 0) | (2 if remove_face_labels else 0)
        curves = np.empty((F, 118, 8), dtype=np.float64)              # every stroke's line, fitted on the host as the reference fits it (csrc/lmfit.hpp)
        call(self.lib, "tsnet_fit_pose_curves", pts.ctypes.data, F, flags, curves.ctypes.data)
        pd = torch.from_numpy(pts).to(self.device)
        cd = torch.from_numpy(curves).to(self.device)
        buf = torch.empty((n + 3) // 4 * 4, dtype=torch.uint8, device=self.device)      # whole 32-bit words: the kernel raises bytes with word atomics
        call(self.lib, "tsnet_raster_pose", pd.data_ptr(), cd.data_ptr(), F, h, w, xs, ys, xe, ye, flags, buf.data_ptr(), device=self.device)
        self._held["rasterise"] = {"points": pd, "curves": cd}
        return buf[:n].view(F, ye - ys, xe - xs)

    def bbox(self, labels: torch.Tensor) -> torch.Tensor:
        """get_bbox_image (dataset_video_pose.py:590-607) of (F,h,w) uint8 labels -> (F,h,w) uint8 0/255"""
        lab = labels.to(self.device).contiguous()
        F, h, w = lab.shape
        out = torch.empty_like(lab)
        call(self.lib, "tsnet_label_bbox", lab.data_ptr(), F, h, w, out.data_ptr(), device=self.device)
        self._held["bbox"] = {"labels": lab}
        return out

    def to_square(self, maps: torch.Tensor, img_size: Tuple[int, int] = (128, 256), binarise: bool = False) -> torch.Tensor:
        """Image.resize(img_size, NEAREST) + resize_square (dataset_video_pose.py:425-432, :471-477) of (F,h,w) uint8 maps -> (F,S,S) float32 with
        S = max(img_size); binarise gives the `!= 0` mask of :441."""
        m = maps.to(self.device).contiguous()
        F, h, w = m.shape
        ow, oh = img_size
        S = max(ow, oh)
        yt = torch.from_numpy(nearest_table(h, oh)).to(self.device)
        xt = torch.from_numpy(nearest_table(w, ow)).to(self.device)
        out = torch.empty((F, S, S), dtype=torch.float32, device=self.device)
        call(self.lib, "tsnet_resize_pad", m.data_ptr(), F, h, w, yt.data_ptr(), xt.data_ptr(), oh, ow, (S - oh) // 2, (S - ow) // 2, S, S,
             int(binarise), out.data_ptr(), device=self.device)
        self._held["to_square"] = {"maps": m, "rows": yt, "columns": xt}
        return out

    def clip_labels(self, points: Sequence[np.ndarray], size: Tuple[int, int], window=None, img_size=(128, 256), compact: bool = False):
        """The label tensors of a clip as the data loader hands them to the model: class maps (F,256,256) float (vl2ch makes them one-hot),
        bounding-box masks (F,256,256) float 0/1, and the crop used (from the first frame when not given, :331-334).
        compact=True: the same two maps as uint8 (class indices 0..24, masks 0 / 1) -- a compact call's labels and masks as they are, no
        vl2ch: the stem's packing kernel makes the one-hot planes on load."""
        if window is None:
            window = pose_crop_coords(points[0], size)
        cls = self.rasterise(points, size, window)
        box = self.bbox(cls)
        held = {"rasterise": self._held["rasterise"], "bbox": self._held["bbox"]}
        cls = self.to_square(cls, img_size)
        held["to_square(labels)"] = self._held["to_square"]
        box = self.to_square(box, img_size, binarise=True)
        held["to_square(bbox)"] = self._held["to_square"]
        self._held["clip_labels"] = held
        if compact:
            cls, box = cls.to(torch.uint8), box.to(torch.uint8)             # exact: small integers
        return cls, box, window
