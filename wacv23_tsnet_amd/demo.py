"""Demo-side post-processing on the device.

Mirrors what demo/demo_face.py:180-231 and demo/demo_pose.py:186-242 do around `model.forward()`:
the generated frame is re-normalised to the first source image's per-channel statistics, `sample_img`
turns it into an RGB byte image, and PIL writes the three-panel strip and the clip.  The arithmetic runs
in two HIP kernels behind the C ABI (`tsnet_frame_stats`, `tsnet_demo_postprocess`); only the packed
uint8 frame crosses PCIe (3 bytes per pixel instead of the reference's 12).  PNG / GIF writing uses PIL
only (the reference's cv2 / imageio are not needed)."""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np
import torch

from . import _lib
from ._call import call

IMG_MEAN = np.array((101.84807705937696, 112.10832843463207, 111.65973036298041), dtype=np.float32)   # demo_face.py:27


class DemoPostprocessor:
    """ref_img: (1,3,H,W) or (3,H,W) float32 -- the first source image as the demo feeds it (mean-subtracted, 0..255
    scale).  Calling the object on generated frames (B,3,H,W) returns (B,H,W,3) uint8 RGB on the same device."""

    def __init__(self, ref_img: torch.Tensor, lib=None):
        self.lib = lib if lib is not None else _lib.load()
        ref = ref_img.reshape(1, 3, -1).contiguous().float()
        self.ref_mean = torch.empty(3, dtype=torch.float32, device=ref.device)
        self.ref_std = torch.empty(3, dtype=torch.float32, device=ref.device)
        call(self.lib, "tsnet_frame_stats", ref.data_ptr(), 1, 3, ref.shape[2], 255.0, self.ref_mean.data_ptr(), self.ref_std.data_ptr(),
             device=ref.device)
        # IMG_MEAN / 255 in float32, as `torch.from_numpy(IMG_MEAN).cuda() / 255` (demo_face.py:98)
        self._img_mean = (C.c_float * 3)(*[float(v) for v in (torch.from_numpy(IMG_MEAN) / 255).tolist()])

    def __call__(self, rec: torch.Tensor) -> torch.Tensor:
        if rec.dim() != 4 or rec.shape[1] != 3 or rec.dtype != torch.float32:
            raise ValueError("expected generated frames of shape (B,3,H,W), float32")
        if rec.device != self.ref_mean.device:
            raise ValueError("frames and reference image must be on the same device")
        rec = rec.contiguous()
        B, _, H, W = rec.shape
        gm = torch.empty(B * 3, dtype=torch.float32, device=rec.device)
        gs = torch.empty(B * 3, dtype=torch.float32, device=rec.device)
        out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=rec.device)
        call(self.lib, "tsnet_frame_stats", rec.data_ptr(), B, 3, H * W, 1.0, gm.data_ptr(), gs.data_ptr(), device=rec.device)
        call(self.lib, "tsnet_demo_postprocess", rec.data_ptr(), B, H, W, gm.data_ptr(), gs.data_ptr(), self.ref_mean.data_ptr(),
             self.ref_std.data_ptr(), self._img_mean, out.data_ptr(), device=rec.device)
        return out


def input_to_rgb(img: torch.Tensor) -> np.ndarray:
    """A mean-subtracted BGR input image (3,H,W) as the uint8 RGB panel of the strip (demo_face.py:201-213)."""
    a = img.detach().cpu().numpy().copy().transpose(1, 2, 0)
    a = a + IMG_MEAN
    return np.ascontiguousarray(a[:, :, ::-1]).astype("uint8")


def save_strip(src_rgb: np.ndarray, tar_rgb: np.ndarray, rec_rgb: np.ndarray, path: str) -> np.ndarray:
    """The source | driving | generated strip of demo_face.py:215-231; returns the strip as an array."""
    from PIL import Image
    h, w = rec_rgb.shape[:2]
    strip = Image.new("RGB", (w * 3, h))
    for i, a in enumerate((src_rgb, tar_rgb, rec_rgb)):
        strip.paste(Image.fromarray(np.ascontiguousarray(a), "RGB"), (w * i, 0))
    strip.save(path)
    return np.asarray(strip)


def save_gif(frames: Sequence[np.ndarray], path: str, duration_ms: int = 100):
    """imageio.mimsave(video_pth, new_im_list) of demo_face.py:234-235, with PIL."""
    from PIL import Image
    ims = [Image.fromarray(np.ascontiguousarray(f), "RGB") for f in frames]
    ims[0].save(path, save_all=True, append_images=ims[1:], duration=duration_ms, loop=0)


# ----------------------------------------------------------------------------------------------------------------------
# Clip harness: what demo/demo_face.py:108-236 does around the model, with the per-frame work on the device.
RESIZE_NOTE = ("label maps resized by a restatement of skimage.transform.resize + img_as_bool (scikit-image 0.18.3, dataset_video_face.py:316-317): "
               "PARITY UNPINNED -- scikit-image is absent from this image, nothing to check the restatement against")


def _aa_kernel(n_in: int, n_out: int):
    """scipy.ndimage.gaussian_filter1d's weights for skimage's anti-aliasing sigma, centre first -> (lw, doubles) or (-1, None)"""
    sigma = max(0.0, (n_in / n_out - 1.0) / 2.0)
    if sigma <= 1e-15:
        return -1, None
    lw = int(4.0 * sigma + 0.5)
    k = np.arange(-lw, lw + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * k ** 2)
    w = phi / phi.sum()
    return lw, np.ascontiguousarray(w[lw:], dtype=np.float64)


def resize_label(x: torch.Tensor, size=(256, 256), lib=None) -> torch.Tensor:
    """(F,h,w) byte maps (0 / 255) -> (F,H,W) {0,1} floats: np.asarray(img_as_bool(resize(x, size))) of the reference's loaders
    (dataset_video_face.py:104-106, 316-317, 397-398) through `tsnet_resize_label` -- restated from the published algorithm of scikit-image
    0.18.3: anti-aliasing Gaussian on the uint8 image (sigma = (in / out - 1) / 2, truncating cast, identity for crops below 320 pixels),
    bilinear sampling at f (o + 0.5) - 0.5 with mirrored borders in float64, threshold 0.5.  PARITY UNPINNED (RESIZE_NOTE): the kernels
    follow oracle/skimage_resize.py, which tests/test_resize.py holds them equal to, but neither can be run against scikit-image here.
    lib: tests pass the CPU emulation build; product code leaves it None (the in-tree HIP library, no fallback)."""
    lib = lib if lib is not None else _lib.load()
    F_, h, w = x.shape
    H, W = size
    src = x.to(torch.uint8).contiguous()
    out = torch.empty((F_, H, W), dtype=torch.float32, device=src.device)
    (lr, wr), (lc, wc) = _aa_kernel(h, H), _aa_kernel(w, W)
    call(lib, "tsnet_resize_label", src.data_ptr(), F_, h, w, H, W, wr.ctypes.data if wr is not None else None, lr,
         wc.ctypes.data if wc is not None else None, lc, out.data_ptr(), device=src.device)
    return out


class ClipRunner:
    """One (source set, driving clip) job in the reference's demo protocol (demo_face.py:166-231):
      * the K source frames are encoded ONCE (`tsnet_set_sources`; the reference re-encodes them for every driving frame, :187-192);
      * every driving frame is one `tsnet_forward_target` at batch 1, re-normalised to the first source image's statistics and turned
        into RGB bytes on the device (`DemoPostprocessor`); only the bytes cross PCIe;
      * with batch > 1 the one source set is cached for the whole batch (`tsnet_set_sources_shared`: K encoded images, not K * batch) and
        `run()` walks the clip in groups of `batch` driving frames with a ragged last group -- the same bytes as batch 1, at the batch rate;
      * `replace_source(i, ...)` swaps one source for another at 1 / K of the encoding work: from the first call on the runner keeps its sources
        in slots 0 .. K-1 of the engine's source bank (`tsnet_bank_put`, `tsnet_forward_bank`) and re-encodes slot i alone;
      * sources and driving frames may be COMPACT (uint8: image bytes before the mean subtraction, class maps, 0 / 1 masks; `img_mean` is what the
        float32 images have subtracted) -- per call, either form, the same bytes out: the engine widens them on load (`tsnet_*_u8`);
      * the three-panel strips and the GIF are written with PIL;
      * `run(..., paste_into=frames, paste_box=...)` resizes every generated frame to the crop box it came from and pastes it into the full
        video frame on the device (`FrameLoader.paste`), and returns / writes the full frames; `paste_boxes=` (F,4) gives every frame its own box.
    model: a wacv23_tsnet_amd.model.TSNet on the GPU.

    The runner OWNS an engine -- a second copy of the packed weights (~350 MB for the 67 M-parameter net) plus an arena for `batch` frames on the device.
    Release it with `close()` or use the runner as a context manager (`with ClipRunner(...) as r:`); `__del__` is only a fallback (at
    interpreter shutdown the library may already be gone)."""

    def __init__(self, model, src_img: Sequence[torch.Tensor], src_lbl: Sequence[torch.Tensor], src_bbox: Sequence[torch.Tensor], batch: int = 1,
                 img_mean=IMG_MEAN):
        if batch < 1:
            raise ValueError("batch must be >= 1")
        self.model = model
        self.batch = batch
        self.img_mean = [float(v) for v in np.asarray(img_mean, dtype=np.float32)]
        # its OWN engine (the model's weights at this moment, default /255 source divisors): the model's shared engine is
        # re-created when a later forward() needs a larger batch or new weights, and carries the divisors of the last set_train_input
        self.eng = model._new_engine(batch)
        K = model.n_source
        dev = model._device()
        u8 = self._is_compact(src_lbl[0])
        mv = lambda t: self._mv(t, dev, u8)
        self.src_img = [mv(x) for x in src_img[:K]]
        self.src_lbl, self.src_bbox = [mv(x) for x in src_lbl[:K]], [mv(x) for x in src_bbox[:K]]
        self.eng.set_sources(self.src_img, self.src_lbl, self.src_bbox, shared=batch > 1, **self._mean_kw(u8))
        self._bank = False                                          # replace_source moves the sources into the engine's source bank
        self._set_ref()

    @staticmethod
    def _is_compact(lbl: torch.Tensor) -> bool:
        return lbl.dtype == torch.uint8

    @staticmethod
    def _mv(t: torch.Tensor, dev, u8: bool) -> torch.Tensor:
        """a call's tensor on the device in the call's form; a compact call keeps whatever is not uint8 as it is (the engine names it)"""
        return (t.to(dev) if u8 else t.to(dev, dtype=torch.float32)).contiguous()

    def _mean_kw(self, u8: bool):
        return {"mean": self.img_mean} if u8 else {}

    def _set_ref(self):
        """the first source image as float32 BGR - mean (widened when it came as bytes): post-processing statistics (ref_img_list[0], :180) and strips"""
        a = self.src_img[0]
        if a.dtype == torch.uint8:
            a = a.float() - torch.tensor(self.img_mean, dtype=torch.float32, device=a.device).view(1, 3, 1, 1)
        self._src0 = a
        self.post = DemoPostprocessor(a, lib=self.eng.lib)

    def replace_source(self, i: int, img: torch.Tensor, lbl: torch.Tensor, bbox: torch.Tensor):
        """Source i <- (img (1,3,H,W), lbl (1,L,H,W), bbox (1,H,W)); the frames produced afterwards are those of a fresh runner built
        with the new set.  Only source i is encoded -- except in the first call, which moves all K sources from the clip cache into
        slots 0 .. K-1 of the source bank (the two lay the bounding boxes out differently)."""
        K = len(self.src_img)
        if not 0 <= i < K:
            raise ValueError(f"source {i} of {K}")
        dev = self.src_img[0].device
        u8 = self._is_compact(lbl)
        mv = lambda t: self._mv(t, dev, u8)
        self.src_img[i], self.src_lbl[i], self.src_bbox[i] = mv(img), mv(lbl), mv(bbox)
        put = lambda j, n: self.eng.bank_put(j, self.src_img[j:j + n], self.src_lbl[j:j + n], self.src_bbox[j:j + n],
                                             **self._mean_kw(self._is_compact(self.src_lbl[j])))
        if self._bank:
            put(i, 1)
        else:
            if len({self._is_compact(t) for t in self.src_lbl}) == 1:
                put(0, K)
            else:                                                   # sources in both forms: a put is one form
                for j in range(K):
                    put(j, 1)
            self._bank = True
        if i == 0:
            self._set_ref()

    def close(self):
        if self.eng is not None:
            self.eng.close()
            self.eng = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def frames(self, tar_lbl: torch.Tensor, tar_bbox: torch.Tensor) -> torch.Tensor:
        """n <= batch driving frames (n,L,H,W), (n,H,W) in one forward_target -> (n,H,W,3) uint8 RGB on the device"""
        if tar_lbl.shape[0] > self.batch:
            raise ValueError(f"{tar_lbl.shape[0]} driving frames, runner built for batch {self.batch}")
        dev = self.src_img[0].device
        u8 = self._is_compact(tar_lbl)
        tl, tb = self._mv(tar_lbl, dev, u8), self._mv(tar_bbox, dev, u8)
        if self._bank:
            rec, _ = self.eng.forward_bank([list(range(len(self.src_img)))] * tl.shape[0], tl, tb)
        else:
            rec, _ = self.eng.forward_target(tl, tb)
        return self.post(rec)

    def frame(self, tar_lbl: torch.Tensor, tar_bbox: torch.Tensor) -> torch.Tensor:
        """one driving frame (1,L,H,W), (1,H,W) -> (H,W,3) uint8 RGB on the device"""
        return self.frames(tar_lbl, tar_bbox)[0]

    def run(self, tar_lbls: torch.Tensor, tar_bboxs: torch.Tensor, out_dir: str = None, tar_imgs: torch.Tensor = None, name: str = "clip",
            paste_into=None, paste_box=None, paste_src_box=None, paste_mask=None, paste_boxes=None, paste_feather=None, paste_feather_from="box",
            y4m=None, y4m_standard="bt601", y4m_full_range=True):
        """tar_lbls (F,L,H,W), tar_bboxs (F,H,W); returns the generated frames (F,H,W,3) uint8 (host).  With out_dir: strips + GIF.
        paste_into: (F,h,w,3) uint8 video frames, tensor or array -- every group's bytes are resized to paste_box = (x0, y0, x1, y1) (the crop box
        the clip was loaded with; it may leave the frame) and pasted into its frames on the device (`FrameLoader.paste`: Pillow's resize + paste,
        byte for byte); paste_src_box: the part of a generated frame that holds picture (pose: (64, 0, 192, 256)), None = all of it; paste_mask:
        (F,H,W) uint8, None = plain paste.  `run` then returns the full frames (F,h,w,3) uint8 (host), a copy -- paste_into is left as it is --
        and out_dir also gets them as "{i:06d}_{name}_full.png"; strips and GIF are written from the generated bytes as without it.
        paste_boxes: (F,4) instead of paste_box, a box per frame (tracking crops, raster.crop_coords_clip in x0, y0, x1, y1 order): every group
        pastes with its slice of boxes, still one launch per group (`tsnet_paste_frames_boxes`).
        paste_feather: a radius (or (rx, ry)) for a soft seam (`FrameLoader.feather_mask`: Pillow's GaussianBlur of the mask, byte for byte), None =
        the hard seam.  paste_feather_from="box": the feathered indicator of paste_src_box shrunk by `feather_inset`, made once per run and reused
        for every group; "bbox": every group's tar_bboxs rows (float32 or compact) become that group's mask -- the feathered face region, another
        for every frame.  With paste_mask the given mask is blurred instead (once, before the first group).
        y4m: a `video.Y4MWriter` (left open) or a path (opened and closed here, size taken from the frames, 25 frames/s) -- every group's
        output frames, the pasted full frames with paste_into and the generated frames without, are converted on the device
        (`FrameLoader.to_yuv420`, y4m_standard, y4m_full_range), downloaded as I420, half the bytes of RGB, and appended to the file.  With y4m
        and no out_dir no RGB byte is downloaded and `run` returns the number of frames written; with both, everything above is as without y4m."""
        import os
        n = tar_lbls.shape[0]
        full = None
        if y4m is not None:
            from .frames import FrameLoader
            from .video import Y4MWriter
            yld = FrameLoader(self.src_img[0].device, lib=self.eng.lib)
            writer, written = (y4m if isinstance(y4m, Y4MWriter) else None), 0
        if paste_feather_from not in ("box", "bbox"):
            raise ValueError(f"paste_feather_from must be 'box' or 'bbox', not {paste_feather_from!r}")
        if paste_feather is not None and paste_into is None:
            raise ValueError("paste_feather needs paste_into")
        if paste_feather is not None and paste_mask is not None and paste_feather_from == "bbox":
            raise ValueError("paste_mask and paste_feather_from='bbox': one source for the mask, not both")
        if paste_box is not None and paste_boxes is not None:
            raise ValueError("paste_box and paste_boxes: one box for the clip or one per frame, not both")
        if paste_into is not None:
            from .frames import FrameLoader
            if paste_box is None and paste_boxes is None:
                raise ValueError("paste_into needs paste_box or paste_boxes")
            if paste_boxes is not None:
                paste_boxes = FrameLoader._boxes(paste_boxes, n)
            dev = self.src_img[0].device
            ld = FrameLoader(dev, lib=self.eng.lib)
            full = ld._u8(paste_into, "frames to paste into", 4)
            if full.shape[0] != n or (paste_mask is not None and paste_mask.shape[0] != n):
                raise ValueError(f"{n} driving frames, {full.shape[0]} frames to paste into")
            host = full
            full = host.to(dev).contiguous()
            if full.data_ptr() == host.data_ptr():                  # already on the device: paste into a copy
                full = full.clone()
            if paste_feather is not None and paste_mask is not None:
                paste_mask = ld._paste_mask(paste_mask, paste_feather, None, None)
        groups, box_mask = [], None
        try:
            for i in range(0, n, self.batch):
                g = self.frames(tar_lbls[i:i + self.batch], tar_bboxs[i:i + self.batch])
                if full is not None:
                    mask = None if paste_mask is None else paste_mask[i:i + self.batch]
                    if paste_feather is not None and paste_mask is None:
                        if paste_feather_from == "bbox":                # 0 / 1 rows in either form: every non-zero byte counts as 255
                            tb = tar_bboxs[i:i + self.batch].to(dev)
                            mask = ld.feather_mask(tb if tb.dtype == torch.uint8 else (tb != 0).to(torch.uint8), paste_feather, binary=True)
                        else:
                            if box_mask is None:                        # one mask for the run: the first group is the largest
                                box_mask = ld._paste_mask(None, paste_feather, tuple(g.shape[:3]), paste_src_box)
                            mask = box_mask[:g.shape[0]]
                    ld.paste(g, full[i:i + self.batch], paste_box if paste_boxes is None else paste_boxes[i:i + self.batch], src_box=paste_src_box,
                             mask=mask, inplace=True)
                if y4m is not None:
                    o = g if full is None else full[i:i + self.batch]
                    if writer is None:
                        writer = Y4MWriter(y4m, o.shape[2], o.shape[1], full_range=y4m_full_range)
                    written += writer.write(yld.to_yuv420(o, "i420", y4m_standard, y4m_full_range).cpu())
                if y4m is None or out_dir:
                    groups.append(g)
        finally:
            if y4m is not None and writer is not None and writer is not y4m:     # opened here from a path
                writer.close()
        if y4m is not None and not out_dir:
            return written
        out = torch.cat(groups).cpu().numpy()
        if out_dir:
            os.makedirs(out_dir, exist_ok=True)
            strips = []
            src_rgb = input_to_rgb(self._src0[0])
            for i in range(out.shape[0]):
                if tar_imgs is not None:
                    tar_rgb = input_to_rgb(tar_imgs[i])
                else:                                               # no ground-truth driving frame: show the label map (every non-background class) instead
                    t = tar_lbls[i].detach().cpu().numpy()
                    m = ((t != 0) if self._is_compact(tar_lbls) else (t[0] == 0)).astype(np.uint8) * 255
                    tar_rgb = np.repeat(m[:, :, None], 3, axis=2)
                strips.append(save_strip(src_rgb, tar_rgb, out[i], os.path.join(out_dir, f"{i:06d}_{name}.png")))
            save_gif(strips, os.path.join(out_dir, f"{name}.gif"))
        if full is None:
            return out
        full = full.cpu().numpy()
        if out_dir:
            from PIL import Image
            for i in range(full.shape[0]):
                Image.fromarray(full[i], "RGB").save(os.path.join(out_dir, f"{i:06d}_{name}_full.png"))
        return full
