"""Frame loading on the device: decoded video frames -> the image tensors `set_test_input` / `set_sources` take.

The reference does this per frame on the host in its data loaders (dataset/dataset_video_face.py:318-329, 391-401; dataset/dataset_video_pose.py:346,
412-417, 450-457): PIL `crop` to the clip's crop box, `Image.resize` with Pillow's default filter (bicubic) to 256 x 256 (face) or 128 x 256 (pose),
for pose `resize_square` to 256 x 256 with black bars, RGB -> BGR, `- IMG_MEAN`; the fp32 result (12 bytes per pixel) is then uploaded.  Here the
uint8 frames go to the device once (3 bytes per pixel) and one kernel (csrc/frames.hpp, `tsnet_prepare_frames`) does the rest.  Pillow's 8-bit
resampler is integer arithmetic on coefficient tables; the tables are built on the host in Pillow's operation order (`bicubic_table`, a few hundred
doubles per axis), so the tensors EQUAL the reference's, byte for byte before the mean subtraction (tests/test_frames.py).

The way back is here too: `FrameLoader.paste` resizes generated frames (the bytes `DemoPostprocessor` returns) to the crop box they came from and
pastes them into the full frames (csrc/paste.hpp, `tsnet_paste_frames`) -- Pillow's `crop().resize()` + `Image.paste()`, mask included, byte
for byte (tests/test_paste_frames.py).  `FrameLoader.feather_mask` makes the mask of a soft seam (csrc/mask_blur.hpp, `tsnet_blur_mask`): Pillow's
`Image.filter(ImageFilter.GaussianBlur(r))` on "L" images, byte for byte (tests/test_feather_mask.py); `paste(..., feather=r)` uses it.

Both ends can cross PCIe as YUV 4:2:0, 1.5 bytes per pixel instead of 3, in the form encoders and decoders speak: `FrameLoader.to_yuv420` /
`from_yuv420` (csrc/yuv_frames.hpp, `tsnet_rgb_to_yuv420` / `tsnet_yuv420_to_rgb`; I420 or NV12, BT.601 or BT.709, full or limited range) --
integer arithmetic on the tables of `tsnet_yuv_coeffs`, held to equality with a numpy restatement (tests/test_yuv_frames.py).

Decoding PNG / JPEG files stays with PIL on the host; the training loaders' random crop / scale / flip are out of scope."""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from ._call import Wrapper, call, fail, last_error
from .demo import IMG_MEAN

PRECISION_BITS = 22


def bicubic_taps(n_in: int, n_out: int) -> int:
    """Row stride of an axis' coefficient table (ksize of Pillow's precompute_coeffs)."""
    return int(math.ceil(2.0 * max(n_in / n_out, 1.0))) * 2 + 1


def _bicubic(x: float, a: float = -0.5) -> float:
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def bicubic_table(n_in: int, n_out: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Pillow's coefficient table of one axis of `Image.resize((.., ..))` (bicubic, 8 bits per channel): (first[n_out], count[n_out],
    coef[n_out, taps]) int32 -- libImaging/Resample.c precompute_coeffs + normalize_coeffs_8bpc restated in their operation order.  Output pixel o
    is clip8((2^21 + sum_j in[first[o] + j] * coef[o, j]) >> 22).  `tsnet_bicubic_table` is the same table from C; the tests hold them equal."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support, ss = 2.0 * fs, 1.0 / fs
    taps = int(math.ceil(support)) * 2 + 1
    first, count, coef = np.zeros(n_out, np.int32), np.zeros(n_out, np.int32), np.zeros((n_out, taps), np.int32)
    for o in range(n_out):
        center = (o + 0.5) * scale
        lo, hi = max(int(center - support + 0.5), 0), min(int(center + support + 0.5), n_in)
        w = [_bicubic((j + lo - center + 0.5) * ss) for j in range(hi - lo)]
        ww = 0.0
        for v in w:
            ww += v
        for j, v in enumerate(w):
            v = v / ww if ww != 0.0 else v
            coef[o, j] = int(v * (1 << PRECISION_BITS) - 0.5) if v < 0 else int(v * (1 << PRECISION_BITS) + 0.5)
        first[o], count[o] = lo, hi - lo
    return first, count, coef


def bicubic_table_c(lib, n_in: int, n_out: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The same table from the library's host entry `tsnet_bicubic_table`."""
    taps = call(lib, "tsnet_bicubic_taps", n_in, n_out, check=False)
    if taps < 0:
        fail(lib, "tsnet_bicubic_taps", taps)
    first, count, coef = np.zeros(n_out, np.int32), np.zeros(n_out, np.int32), np.zeros((n_out, taps), np.int32)
    call(lib, "tsnet_bicubic_table", n_in, n_out, first.ctypes.data, count.ctypes.data, coef.ctypes.data)
    return first, count, coef


YUV_STANDARDS = {"bt601": 601, "bt709": 709}
YUV_LAYOUTS = {"i420": 0, "nv12": 1}


def _yuv_layout(layout) -> int:
    if str(layout).lower() not in YUV_LAYOUTS:
        raise ValueError(f"layout must be one of {sorted(YUV_LAYOUTS)}, not {layout!r}")
    return YUV_LAYOUTS[str(layout).lower()]


def yuv_frame_bytes(h: int, w: int) -> int:
    """bytes of one 4:2:0 frame of h x w pixels, either layout"""
    return h * w + 2 * ((h + 1) // 2) * ((w + 1) // 2)


def yuv_planes(buf, h: int, w: int, layout: str = "i420"):
    """Views of the planes of (F, yuv_frame_bytes(h, w)) frames, tensor or array: (Y (F,h,w), Cb (F,ch,cw), Cr (F,ch,cw)); in "nv12" the two
    chroma views are the strided halves of the interleaved plane."""
    ch, cw = (h + 1) // 2, (w + 1) // 2
    if buf.ndim != 2 or buf.shape[1] != yuv_frame_bytes(h, w):
        raise ValueError(f"expected frames of shape (F, {yuv_frame_bytes(h, w)}) for size {(h, w)}, got {tuple(buf.shape)}")
    F = buf.shape[0]
    y = buf[:, :h * w].reshape(F, h, w)
    if _yuv_layout(layout) == 0:
        return y, buf[:, h * w:h * w + ch * cw].reshape(F, ch, cw), buf[:, h * w + ch * cw:].reshape(F, ch, cw)
    uv = buf[:, h * w:].reshape(F, ch, cw, 2)
    return y, uv[..., 0], uv[..., 1]


class FrameLoader(Wrapper):
    """Network-input image tensors of a clip's frames on `device`.

    lib: tests pass the CPU emulation build; product code leaves it None (the in-tree HIP library, no fallback).
    The coefficient tables of an (input size, output size) pair are built and uploaded once and kept; after that `prepare` on frames that are
    already on the device only enqueues one kernel on the current stream (no allocation inside the library, no synchronisation)."""

    def __init__(self, device, lib=None):
        super().__init__(device, lib)
        self._tables = {}
        self._pool_host = np.zeros(0, np.int32)                      # the tables of the per-frame-box calls, one after the other
        self._pool_at = {}                                           # (n_in, n_out) -> (offset in ints, taps)
        self._pool = None                                            # the device copy; replaced (never written) when the pool has grown
        self._feather_tmp = None                                     # the intermediate between feather_mask's two kernels; grows, never shrinks
        self._yuv_tables = {}                                        # (standard, full range) -> (fwd, inv) of tsnet_yuv_coeffs

    def _axis(self, n_in: int, n_out: int):
        """(device int32 tensor [first | count | coef], taps) of one axis, cached"""
        key = (n_in, n_out)
        if key not in self._tables:
            first, count, coef = bicubic_table_c(self.lib, n_in, n_out)
            flat = torch.from_numpy(np.concatenate([first, count, coef.ravel()])).to(self.device)
            self._tables[key] = (flat, coef.shape[1])
        return self._tables[key]

    def _axis_args(self, n_in: int, n_out: int):
        """that table as tsnet_prepare_frames / tsnet_paste_frames take it: (first, count, coef, taps)"""
        flat, taps = self._axis(n_in, n_out)
        return flat.data_ptr(), flat.data_ptr() + 4 * n_out, flat.data_ptr() + 8 * n_out, taps

    # ------------------------------------------------------------------------------------------------------------------ a box per frame
    def _pool_axis(self, n_in: int, n_out: int) -> Tuple[int, int]:
        """(offset, taps) of an axis' table in the pool, appended on first sight; (-1, 0) for an axis that keeps its size"""
        if n_in == n_out:
            return -1, 0
        key = (n_in, n_out)
        if key not in self._pool_at:
            first, count, coef = bicubic_table_c(self.lib, n_in, n_out)
            self._pool_at[key] = (len(self._pool_host), coef.shape[1])
            self._pool_host = np.concatenate([self._pool_host, first, count, coef.ravel()])
        return self._pool_at[key]

    def _descriptors(self, boxes: np.ndarray, sizes):
        """boxes (F,4) x0, y0, x1, y1; sizes(box) -> ((x n_in, x n_out), (y n_in, y n_out)).  Returns (host (F,8) int32, its device copy, the
        device pool, the pool it replaced or None): rows {x0, y0, x1, y1, xoff, xtaps, yoff, ytaps} as tsnet_*_frames_boxes take them."""
        rows, at = [], self._pool_at
        for f, b in enumerate(boxes.tolist()):                       # plain ints: this loop is per frame and per call
            if b[2] <= b[0] or b[3] <= b[1]:
                raise ValueError(f"frame {f}: empty box {tuple(b)}")
            (xi, xo), (yi, yo) = sizes(b)
            x = (-1, 0) if xi == xo else (at.get((xi, xo)) or self._pool_axis(xi, xo))
            y = (-1, 0) if yi == yo else (at.get((yi, yo)) or self._pool_axis(yi, yo))
            rows.append((b[0], b[1], b[2], b[3], x[0], x[1], y[0], y[1]))
        desc = np.array(rows, dtype=np.int32).reshape(-1, 8)
        old = None
        if self._pool is None or self._pool.numel() != len(self._pool_host):     # grown: a new device copy; an enqueued kernel may still read the old one
            old, self._pool = self._pool, torch.from_numpy(self._pool_host.copy()).to(self.device)
        return desc, torch.from_numpy(desc).to(self.device), self._pool, old

    @staticmethod
    def _boxes(boxes, F: int, order=(0, 1, 2, 3)) -> np.ndarray:
        b = np.asarray(boxes.cpu() if isinstance(boxes, torch.Tensor) else boxes)
        if b.ndim != 2 or b.shape[1] != 4:
            raise ValueError(f"expected (F,4) boxes, got shape {b.shape}")
        if b.shape[0] != F:
            raise ValueError(f"{b.shape[0]} boxes for {F} frames")
        return b.astype(np.int64)[:, list(order)]

    def _prepare_front(self, frames, size, square, mean, as_bytes):
        """what `prepare` does before it looks at its box: (the frames on the device, (oh, ow, pad_top, pad_left, OH, OW), the mean as the ABI
        takes it, the output tensor)"""
        if isinstance(frames, np.ndarray):
            frames = torch.from_numpy(np.ascontiguousarray(frames))
        if frames.dim() != 4 or frames.shape[3] != 3 or frames.dtype != torch.uint8:
            raise ValueError(f"expected uint8 frames of shape (F,h,w,3), got {tuple(frames.shape)} {frames.dtype}")
        fr = frames.to(self.device).contiguous()
        ow, oh = int(size[0]), int(size[1])
        S = max(ow, oh)
        OH, OW = (S, S) if square else (oh, ow)
        m = np.asarray(mean, dtype=np.float32)
        mean_c = (C.c_float * 3)(float(m[0]), float(m[1]), float(m[2]))
        out = torch.empty((fr.shape[0], 3, OH, OW), dtype=torch.uint8 if as_bytes else torch.float32, device=self.device)
        return fr, (oh, ow, (OH - oh) // 2, (OW - ow) // 2, OH, OW), mean_c, out

    def prepare(self, frames, box: Sequence[int], size: Tuple[int, int], square: bool = False, mean=IMG_MEAN, as_bytes: bool = False) -> torch.Tensor:
        """frames: (F,h,w,3) uint8 RGB, tensor or array (uploaded once when on the host).  box: (x0, y0, x1, y1) in PIL order; it may leave the
        frame (Image.crop: zeros there).  size: (ow, oh) as Image.resize takes it.  square: resize_square's centred padding with byte 0 to
        max(ow, oh).  Returns (F,3,H,W) float32 on the device: BGR planes of frame.crop(box).resize(size) minus `mean` (B, G, R).
        as_bytes=True (`tsnet_prepare_frames_u8`): the resized bytes themselves, (F,3,H,W) uint8, `mean` not applied -- the image of a compact
        call (Engine.forward(..., mean=)), a quarter of the size; bytes.float() - mean is the float32 result, bit for bit.
        box may be an (F,4) array-like, one box per frame (`tsnet_prepare_frames_boxes`, still one kernel): frame f then has the bytes of
        prepare(frames[f:f+1], box[f], ...)."""
        fr, geom, mean_c, out = self._prepare_front(frames, size, square, mean, as_bytes)
        F, h, w, _ = fr.shape
        oh, ow = geom[:2]
        held = {"frames": fr}
        if np.ndim(box) == 2:
            desc, desc_d, pool, old = self._descriptors(self._boxes(box, F), lambda b: ((int(b[2] - b[0]), ow), (int(b[3] - b[1]), oh)))
            entry, where = "tsnet_prepare_frames_boxes", (desc.ctypes.data, desc_d.data_ptr(), pool.data_ptr(), pool.numel())
            held.update(descriptors=desc_d, pool=pool, old_pool=old)
        else:
            x0, y0, x1, y1 = (int(v) for v in box)
            if x1 <= x0 or y1 <= y0:
                raise ValueError(f"empty crop box {tuple(box)}")
            entry, where = "tsnet_prepare_frames", (x0, y0, x1, y1, *self._axis_args(x1 - x0, ow), *self._axis_args(y1 - y0, oh))
        if as_bytes:
            call(self.lib, entry + "_u8", fr.data_ptr(), F, h, w, *where, *geom, out.data_ptr(), device=self.device)
        else:
            call(self.lib, entry, fr.data_ptr(), F, h, w, *where, *geom, mean_c, out.data_ptr(), device=self.device)
        self._held["prepare"] = held
        return out

    def face(self, frames, crop: Sequence[int], size: Tuple[int, int] = (256, 256), mean=IMG_MEAN, as_bytes: bool = False) -> torch.Tensor:
        """The face loader's image: crop = [min_y, max_y, min_x, max_x] as raster.crop_coords returns it (get_crop_coords, not clipped to the frame)."""
        if np.ndim(crop) == 2:                                       # (F,4): a crop per frame, as raster.crop_coords_clip returns them
            box = self._boxes(crop, len(frames), (2, 0, 3, 1))
        else:
            min_y, max_y, min_x, max_x = crop
            box = (min_x, min_y, max_x, max_y)
        out = self.prepare(frames, box, size, square=False, mean=mean, as_bytes=as_bytes)
        self._held["face"] = self._held["prepare"]
        return out

    def pose(self, frames, crop: Sequence[int], img_size: Tuple[int, int] = (128, 256), mean=IMG_MEAN, as_bytes: bool = False) -> torch.Tensor:
        """The pose loader's image: crop = (xs, ys, xe, ye) as raster.pose_crop_coords returns it; 128 x 256, then padded to 256 x 256."""
        out = self.prepare(frames, crop, img_size, square=True, mean=mean, as_bytes=as_bytes)
        self._held["pose"] = self._held["prepare"]
        return out

    # ------------------------------------------------------------------------------------------------------------------ the way back
    def _u8(self, t, what: str, ndim: int) -> torch.Tensor:
        if isinstance(t, np.ndarray):
            t = torch.from_numpy(np.ascontiguousarray(t))
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != ndim or (ndim == 4 and t.shape[3] != 3):
            want = "(F,h,w,3)" if ndim == 4 else "(F,h,w)"
            raise ValueError(f"expected uint8 {what} of shape {want}, got {tuple(getattr(t, 'shape', ()))} {getattr(t, 'dtype', type(t))}")
        return t

    # ------------------------------------------------------------------------------------------------------------------ feathered masks
    def _box_params(self, radius: float) -> Tuple[int, int, int]:
        """(box_radius, ww, fw) of one axis from `tsnet_gaussian_box_params` (three passes, as Pillow's GaussianBlur)"""
        br, ww, fw = C.c_int(), C.c_uint(), C.c_uint()
        if call(self.lib, "tsnet_gaussian_box_params", float(radius), 3, C.byref(br), C.byref(ww), C.byref(fw), check=False) != 0:
            raise ValueError(f"feather radius {radius!r}: {last_error(self.lib)}")
        return br.value, ww.value, fw.value

    @staticmethod
    def _radii(radius) -> Tuple[float, float]:
        rx, ry = (radius, radius) if np.ndim(radius) == 0 else radius
        return float(rx), float(ry)

    def feather_inset(self, radius):
        """3 (box_radius + 1) + 1: by how many pixels a rectangle must be shrunk per side so that the outermost ring of its box is exactly 0
        after `feather_mask` (a pixel farther than 3 (box_radius + 1) from every non-zero pixel stays 0).  A number for a number, (ix, iy) for
        a radius pair (rx, ry)."""
        if np.ndim(radius) == 0:
            return 3 * (self._box_params(radius)[0] + 1) + 1
        rx, ry = self._radii(radius)
        return 3 * (self._box_params(rx)[0] + 1) + 1, 3 * (self._box_params(ry)[0] + 1) + 1

    def feather_mask(self, src, radius, size: Optional[Sequence[int]] = None, rect: Optional[Sequence[int]] = None, binary: bool = False) -> torch.Tensor:
        """A paste mask with a soft edge (`tsnet_blur_mask`, csrc/mask_blur.hpp): per frame f, byte for byte,
            Image.fromarray(src[f], "L").filter(ImageFilter.GaussianBlur(radius))
        src: (F,H,W) uint8, tensor or array (uploaded when on the host); binary=True: every non-zero byte counts as 255 (0 / 1 masks as they are).
        src=None: the source is the indicator of rect = (x0, y0, x1, y1) -- 255 inside, 0 outside -- in size = (F,H,W), the same for every frame;
        nothing is read or uploaded.  radius: a number or (rx, ry), as GaussianBlur takes it; an axis with radius 0 is skipped.  H, W <= 512.
        Returns the (F,H,W) uint8 mask on the device.  The intermediate between the two kernels is the loader's and kept between calls; on
        device tensors the call only enqueues (at most) two kernels on the current stream."""
        rx, ry = self._radii(radius)
        rect_c = None
        if src is None:
            if size is None or rect is None:
                raise ValueError("feather_mask(None, ...) needs size=(F,H,W) and rect=(x0, y0, x1, y1)")
            F, H, W = (int(v) for v in size)
            rect_c = (C.c_int * 4)(*(int(v) for v in rect))
            m = None
        else:
            m = self._u8(src, "mask", 3).to(self.device).contiguous()
            F, H, W = m.shape
        n = max(F * H * W, 1)
        old = None
        if self._feather_tmp is None or self._feather_tmp.numel() < n:
            old, self._feather_tmp = self._feather_tmp, torch.empty(n, dtype=torch.uint8, device=self.device)
        out = torch.empty((max(F, 0), max(H, 0), max(W, 0)), dtype=torch.uint8, device=self.device)
        call(self.lib, "tsnet_blur_mask", None if m is None else m.data_ptr(), F, H, W, rect_c, rx, ry, 1 if binary else 0, out.data_ptr(),
             self._feather_tmp.data_ptr(), device=self.device, refusal=ValueError)
        self._held["feather_mask"] = {"src": m, "old_workspace": old}
        return out

    def _paste_mask(self, mask, feather, size, src_box):
        """the mask of a paste with feather=radius: the given mask blurred (0 / 1 masks as binary), or, in size = (F,GH,GW), the feathered
        indicator of the source rectangle shrunk by `feather_inset` per side"""
        if mask is not None:
            m = self._u8(mask, "mask", 3)
            return self.feather_mask(m, feather, binary=bool(m.numel()) and int(m.max()) <= 1)
        F, GH, GW = size
        sx0, sy0, sx1, sy1 = (0, 0, GW, GH) if src_box is None else (int(v) for v in src_box)
        ix, iy = self.feather_inset(self._radii(feather))
        rect = (sx0 + ix, sy0 + iy, sx1 - ix, sy1 - iy)
        if rect[2] <= rect[0] or rect[3] <= rect[1]:
            raise ValueError(f"feather {feather!r} needs an inset of {ix} x {iy} pixels per side (feather_inset), which leaves nothing of the "
                             f"{sx1 - sx0} x {sy1 - sy0} source rectangle")
        return self.feather_mask(None, feather, size=(F, GH, GW), rect=rect)

    def _paste_front(self, gen, frames, box, src_box, mask, inplace):
        """what `paste` does before it builds its box arguments: (g, m, out) checked and on the device -- out the frames, or their clone --,
        the source rectangle, and the call's single box as ints (box=None, a box per frame: None; those are `_descriptors`' to check)."""
        g = self._u8(gen, "generated frames", 4)
        fr = self._u8(frames, "frames", 4)
        m = None if mask is None else self._u8(mask, "mask", 3)
        F, GH, GW, _ = g.shape
        if fr.shape[0] != F:
            raise ValueError(f"{F} generated frames, {fr.shape[0]} frames to paste into")
        if m is not None and tuple(m.shape) != (F, GH, GW):
            raise ValueError(f"mask of shape {tuple(m.shape)}, generated frames {tuple(g.shape)}")
        if box is not None:
            x0, y0, x1, y1 = (int(v) for v in box)
            if x1 <= x0 or y1 <= y0:
                raise ValueError(f"empty box {tuple(box)}")
            box = (x0, y0, x1, y1)
        sx0, sy0, sx1, sy1 = (0, 0, GW, GH) if src_box is None else (int(v) for v in src_box)
        if not (0 <= sx0 < sx1 <= GW and 0 <= sy0 < sy1 <= GH):
            raise ValueError(f"source rectangle {(sx0, sy0, sx1, sy1)} is empty or not inside the {GW} x {GH} generated frames")
        g = g.to(self.device).contiguous()
        m = None if m is None else m.to(self.device).contiguous()
        out = fr.to(self.device).contiguous()
        if not inplace and out.data_ptr() == fr.data_ptr():
            out = out.clone()
        return g, m, out, (sx0, sy0, sx1, sy1), box

    def paste(self, gen, frames, box: Sequence[int], src_box: Optional[Sequence[int]] = None, mask=None, inplace: bool = False, feather=None) -> torch.Tensor:
        """Generated frames back into the video (`tsnet_paste_frames`, csrc/paste.hpp): per frame f, byte for byte,
            g = Image.fromarray(gen[f]).crop(src_box).resize((x1 - x0, y1 - y0)); frame_f.paste(g, (x0, y0), m)
        with m the mask through the same crop and resize, or None.  gen: (F,GH,GW,3) uint8 RGB as `DemoPostprocessor` returns it; frames:
        (F,h,w,3) uint8 RGB; box: (x0, y0, x1, y1) in frame coordinates, it may leave the frame (Pillow clips the paste; outside, nothing is
        written); src_box: the part of gen that holds picture, None = all of it; mask: (F,GH,GW) uint8, 255 = gen, 0 = frame (Pillow's
        paste_mask_L blend in between).  Tensors or arrays; what is on the host is uploaded.  Returns the frames on the device: a clone, or with
        inplace=True `frames` itself when it already is a contiguous tensor on the device.  gen / mask must not share memory with frames.
        box may be an (F,4) array-like, one box per frame (`tsnet_paste_frames_boxes`, still one kernel); src_box stays one per call.
        feather: a radius (or (rx, ry)) for a soft seam, None = the call as it always was.  With mask=None the mask is `feather_mask` of the
        indicator of src_box shrunk by `feather_inset` per side -- in Pillow's terms the rectangle image through
        filter(ImageFilter.GaussianBlur(feather)) -- so that the blend reaches exactly 0 on the source rectangle's outermost ring; a
        rectangle too small for the inset is a ValueError.  With a mask, the mask is blurred first (one holding only 0 / 1 as 0 / 255)."""
        held = {}
        if feather is not None:
            mask = self._paste_mask(mask, feather, tuple(self._u8(gen, "generated frames", 4).shape[:3]), src_box)
            held["feather_mask"] = self._held["feather_mask"]
        per_frame = np.ndim(box) == 2
        g, m, out, src, one = self._paste_front(gen, frames, None if per_frame else box, src_box, mask, inplace)
        F, GH, GW, _ = g.shape
        h, w = out.shape[1], out.shape[2]
        sw, sh = src[2] - src[0], src[3] - src[1]
        head = (g.data_ptr(), None if m is None else m.data_ptr(), F, GH, GW, *src)
        held["gen"], held["mask"] = g, m
        if per_frame:
            desc, desc_d, pool, old = self._descriptors(self._boxes(box, F), lambda b: ((sw, int(b[2] - b[0])), (sh, int(b[3] - b[1]))))
            call(self.lib, "tsnet_paste_frames_boxes", *head, desc.ctypes.data, desc_d.data_ptr(), pool.data_ptr(), pool.numel(), out.data_ptr(), h, w, device=self.device)
            held.update(descriptors=desc_d, pool=pool, old_pool=old)
        else:
            call(self.lib, "tsnet_paste_frames", *head, *self._axis_args(sw, one[2] - one[0]), *self._axis_args(sh, one[3] - one[1]), out.data_ptr(), h, w, *one, device=self.device)
        self._held["paste"] = held
        return out

    def paste_face(self, gen, frames, crop: Sequence[int], mask=None, inplace: bool = False, feather=None) -> torch.Tensor:
        """The inverse of `face`: crop = [min_y, max_y, min_x, max_x]; the whole generated image goes back into that box."""
        if np.ndim(crop) == 2:
            box = self._boxes(crop, len(frames), (2, 0, 3, 1))
        else:
            min_y, max_y, min_x, max_x = crop
            box = (min_x, min_y, max_x, max_y)
        out = self.paste(gen, frames, box, mask=mask, inplace=inplace, feather=feather)
        self._held["paste_face"] = self._held["paste"]
        return out

    def paste_pose(self, gen, frames, crop: Sequence[int], img_size: Tuple[int, int] = (128, 256), mask=None, inplace: bool = False,
                   feather=None) -> torch.Tensor:
        """The inverse of `pose`: crop = (xs, ys, xe, ye); the img_size picture between resize_square's bars goes back into that box."""
        gh, gw = (gen.shape[1], gen.shape[2]) if hasattr(gen, "shape") and len(gen.shape) == 4 else (0, 0)
        S = max(int(img_size[0]), int(img_size[1]))
        if (gh, gw) != (S, S):
            raise ValueError(f"expected generated frames of {S} x {S} (img_size {tuple(img_size)} padded square), got {gw} x {gh}")
        px, py = (S - int(img_size[0])) // 2, (S - int(img_size[1])) // 2
        out = self.paste(gen, frames, crop, src_box=(px, py, px + int(img_size[0]), py + int(img_size[1])), mask=mask, inplace=inplace, feather=feather)
        self._held["paste_pose"] = self._held["paste"]
        return out

    # ------------------------------------------------------------------------------------------------------------------ YUV 4:2:0 in and out
    def yuv_tables(self, standard: str = "bt601", full_range: bool = True) -> Tuple[np.ndarray, np.ndarray]:
        """(fwd int32[12], inv int32[6]) of `tsnet_yuv_coeffs`, cached per (standard, range)"""
        key = (str(standard).lower(), bool(full_range))
        if key not in self._yuv_tables:
            if key[0] not in YUV_STANDARDS:
                raise ValueError(f"standard must be one of {sorted(YUV_STANDARDS)}, not {standard!r}")
            fwd, inv = np.zeros(12, np.int32), np.zeros(6, np.int32)
            if call(self.lib, "tsnet_yuv_coeffs", YUV_STANDARDS[key[0]], int(key[1]), fwd.ctypes.data, inv.ctypes.data, check=False) != 0:
                raise RuntimeError(f"tsnet_yuv_coeffs failed: {last_error(self.lib)}")
            self._yuv_tables[key] = (fwd, inv)
        return self._yuv_tables[key]

    def _yuv_out(self, out, shape) -> torch.Tensor:
        if out is None:
            return torch.empty(shape, dtype=torch.uint8, device=self.device)
        if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != tuple(shape) or out.device.type != self.device.type \
                or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous uint8 tensor of shape {tuple(shape)} on {self.device}")
        return out

    def to_yuv420(self, frames, layout: str = "i420", standard: str = "bt601", full_range: bool = True, out=None) -> torch.Tensor:
        """(F,h,w,3) uint8 RGB, tensor or array (uploaded when on the host) -> (F, h*w + 2*ch*cw) uint8 on the device, ch = (h+1)//2,
        cw = (w+1)//2 (`tsnet_rgb_to_yuv420`, csrc/yuv_frames.hpp): 8-bit Y'CbCr 4:2:0, half the bytes of the RGB frames.  layout "i420": the Y
        plane, then Cb, then Cr -- a Y4M frame's payload (`video.Y4MWriter`); "nv12": the Y plane, then rows of interleaved (Cb, Cr) pairs.
        standard "bt601" / "bt709", full_range True (JFIF) / False (16 .. 235 / 240): the integer tables of `tsnet_yuv_coeffs`; one chroma sample
        is one rounding of the mean over its 2 x 2 block (centred siting), odd sizes included.  out: the tensor to write, else a new one.
        On device tensors the call enqueues one kernel on the current stream: no allocation in the library, no synchronisation."""
        fr = self._u8(frames, "frames", 4).to(self.device).contiguous()
        F, h, w, _ = fr.shape
        fwd, _ = self.yuv_tables(standard, full_range)
        out = self._yuv_out(out, (F, yuv_frame_bytes(h, w)))
        call(self.lib, "tsnet_rgb_to_yuv420", fr.data_ptr(), F, h, w, fwd.ctypes.data, _yuv_layout(layout), out.data_ptr(), refusal=ValueError, device=self.device)
        self._held["to_yuv420"] = {"frames": fr}
        return out

    def from_yuv420(self, yuv, size: Tuple[int, int], layout: str = "i420", standard: str = "bt601", full_range: bool = True, out=None) -> torch.Tensor:
        """The inverse (`tsnet_yuv420_to_rgb`): (F, h*w + 2*ch*cw) uint8 frames as a decoder or `video.Y4MReader` hands them out, size = (h, w)
        -> (F,h,w,3) uint8 RGB on the device, the chroma samples replicated over their 2 x 2 blocks.  rgb -> yuv -> rgb is not the identity:
        on constant 2 x 2 blocks it comes back within 1 per byte with the full-range tables and within 2 with the limited ones."""
        h, w = (int(v) for v in size)
        if isinstance(yuv, np.ndarray):
            yuv = torch.from_numpy(np.ascontiguousarray(yuv))
        if not isinstance(yuv, torch.Tensor) or yuv.dtype != torch.uint8 or yuv.dim() != 2 or h < 1 or w < 1 or yuv.shape[1] != yuv_frame_bytes(h, w):
            raise ValueError(f"expected uint8 frames of shape (F, {yuv_frame_bytes(max(h, 1), max(w, 1))}) for size {(h, w)}, got "
                             f"{tuple(getattr(yuv, 'shape', ()))} {getattr(yuv, 'dtype', type(yuv))}")
        src = yuv.to(self.device).contiguous()
        F = src.shape[0]
        _, inv = self.yuv_tables(standard, full_range)
        out = self._yuv_out(out, (F, h, w, 3))
        call(self.lib, "tsnet_yuv420_to_rgb", src.data_ptr(), F, h, w, inv.ctypes.data, _yuv_layout(layout), out.data_ptr(), refusal=ValueError, device=self.device)
        self._held["from_yuv420"] = {"frames": src}
        return out

    @staticmethod
    def yuv_planes(buf, h: int, w: int, layout: str = "i420"):
        """the module's `yuv_planes`, for who holds a loader"""
        return yuv_planes(buf, h, w, layout)
