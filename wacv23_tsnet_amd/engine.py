"""Python owner of one `tsnet_handle` (include/tsnet_abi.h): device buffers in, device buffers out.

PyTorch is plumbing here -- tensors provide device memory and the current HIP stream; every
FLOP of the forward runs in libtsnet_hip.so.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import torch

from . import _lib
from ._call import call

POSE_MEAN = (101.84807705937696, 112.10832843463207, 111.65973036298041)  # reference model/TSNet_pose.py:215


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


class TSNetEngine:
    """One model replica on one device.

    lib: the bound C library.  Product code never passes it (the in-tree HIP library is used and
    its absence is an error); tests pass the CPU *emulation* build of the same sources to check
    host logic without a GPU.
    """

    def __init__(self, *, label_nc: int, n_blocks: int, n_downsampling: int = 3, n_source: int = 3, ngf: int = 64,
                 enc_blocks: int = 9, addcoords: bool = True, pose_composite: bool = False,
                 pose_mean: Sequence[float] = POSE_MEAN, height: int = 256, width: int = 256, max_batch: int = 4,
                 operands: str = "fp32", lib=None):
        self.lib = lib if lib is not None else _lib.load()
        cfg = _lib.TsnetCfg()
        cfg.label_nc, cfg.n_blocks, cfg.n_downsampling, cfg.n_source = label_nc, n_blocks, n_downsampling, n_source
        cfg.ngf, cfg.enc_blocks, cfg.addcoords, cfg.pose_composite = ngf, enc_blocks, int(addcoords), int(pose_composite)
        for i in range(3):
            cfg.pose_mean[i] = float(pose_mean[i])
        cfg.height, cfg.width, cfg.max_batch = height, width, max_batch
        if operands not in ("fp32", "bf16", "bf16s", "fp16"):
            raise ValueError("operands must be 'fp32' (fp32-class arithmetic), 'bf16' (bf16 conv operands, fp32 accumulate), 'bf16s' (+ bf16 storage "
                             "of the large activations) or 'fp16' (scaled fp16 conv operands, fp32 accumulate and storage)")
        cfg.operand_mode = {"fp32": 0, "bf16": 1, "bf16s": 2, "fp16": 3}[operands]
        self.cfg = cfg
        self.K = n_source
        self.h = height >> n_downsampling
        self.w = width >> n_downsampling
        self.C = ngf << n_downsampling
        self._h = C.c_void_p()
        call(self.lib, "tsnet_create", C.byref(cfg), C.byref(self._h), handle=None)
        self.finalized = False
        self.device: Optional[torch.device] = None     # fixed at finalize(): every allocation, stream and launch of this handle lives there
        self._held = {}                                 # method -> the tensors its last call launched on ("what a wrapper keeps")

    # ------------------------------------------------------------------ helpers
    def _call(self, entry: str, *args, dev=None, stream: bool = False, **kw) -> int:
        """An entry of this handle through `_call.call`: the engine's GPU (or `dev`, before finalize() has fixed it) is current for the
        duration of the call, stream=True appends torch's current stream there, failures read tsnet_last_error(handle)."""
        return call(self.lib, entry, self._h, *args, device=dev if dev is not None else self.device, stream=stream, handle=self._h, **kw)

    def _same_device(self, *tensors):
        for t in tensors:
            if t is not None and self.device is not None and t.device != self.device:
                raise ValueError(f"tensor on {t.device}, engine finalized on {self.device}")

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._call("tsnet_destroy", check=False)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def param_shapes(self) -> Dict[str, tuple]:
        n = self._call("tsnet_num_params", check=False)
        out = {}
        name = C.c_char_p()
        shape = (C.c_int64 * 4)()
        rank = C.c_int()
        for i in range(n):
            self._call("tsnet_param_info", i, C.byref(name), shape, C.byref(rank))
            out[name.value.decode()] = tuple(int(shape[j]) for j in range(rank.value))
        return out

    # ------------------------------------------------------------------ weights
    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True):
        """sd keys: '<net>.<key>' with nets img_enc / lbl_enc / fuse_net / dec (checkpoint schema of
        the reference, train_face.py:350-355).  Extra keys (netD, netDF, ...) are ignored unless strict."""
        expected = self.param_shapes()
        for k, v in sd.items():
            if k not in expected:
                if strict:
                    raise KeyError(f"unexpected parameter {k!r}")
                continue
            t = v.detach().to(torch.float32).contiguous()
            shp = (C.c_int64 * t.dim())(*t.shape)
            if t.is_cuda:      # the cast / copy above is queued on torch's stream; tsnet_load_weights does a blocking hipMemcpy on the null stream
                torch.cuda.current_stream(t.device).synchronize()
            self._call("tsnet_load_weights", k.encode(), t.data_ptr(), shp, t.dim(), dev=t.device if t.is_cuda else None, what=f"load_weights({k})")
        return self

    def finalize(self, device: Optional[torch.device] = None):
        dev = torch.device(device) if device is not None else None
        if dev is not None and dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self._call("tsnet_finalize", dev=dev, stream=True)
        self.device = dev
        self.finalized = True
        return self

    def packed_weights(self, device) -> torch.Tensor:
        """Alias the engine's packed weight buffer as a flat uint8 torch tensor (for the RCCL broadcast)."""
        p = C.c_void_p()
        n = C.c_size_t()
        self._call("tsnet_packed_weights", C.byref(p), C.byref(n))
        return _alias_device_bytes(p.value, n.value, device)

    # ------------------------------------------------------------------ forward
    def _ptr_array(self, ts: Sequence[torch.Tensor]):
        arr = (C.c_void_p * _lib.MAX_SOURCES)()
        for i, t in enumerate(ts):
            arr[i] = t.data_ptr()
        return arr

    @staticmethod
    def _prep(t: torch.Tensor, shape: tuple, name: str) -> torch.Tensor:
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
        if t.dtype != torch.float32:
            raise TypeError(f"{name}: expected float32, got {t.dtype}")
        return t if t.is_contiguous() else t.contiguous()

    # Compact inputs (include/tsnet_abi.h, tsnet_*_u8): a call whose LABEL tensor is torch.uint8 passes the bytes the wide tensors are made
    # from -- img (B,3,H,W) before the mean subtraction, lbl (B,H,W) class indices, bbox (B,H,W) 0 / 1 -- and the image mean as `mean=`
    # wherever images are passed.  Every tensor of such a call must be uint8; the result has the bits of the float32 call on the widened tensors.
    @staticmethod
    def _prep_u8(t: torch.Tensor, shape: tuple, name: str) -> torch.Tensor:
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name}: expected compact shape {tuple(shape)}, got {tuple(t.shape)}")
        if t.dtype != torch.uint8:
            raise TypeError(f"{name}: expected uint8 (a compact call: its label tensor is uint8), got {t.dtype}")
        return t if t.is_contiguous() else t.contiguous()

    def _form(self, lbl: torch.Tensor, B: int):
        """(compact?, prep, image shape, label shape, bbox shape) of a call, decided by its label tensor"""
        H, W, L = self.cfg.height, self.cfg.width, self.cfg.label_nc
        u8 = lbl.dtype == torch.uint8
        form = self._prep_u8 if u8 else self._prep

        def prep(t, shape, name):
            if (t.dtype == torch.uint8) != u8:                       # a call in both forms: named before any shape (the two forms differ in shape too)
                raise TypeError(f"{name}: {t.dtype} in a {'compact (uint8)' if u8 else 'float32'} call -- the label tensor decides the form, and "
                                "every tensor of a call has it")
            return form(t, shape, name)
        return u8, prep, (B, 3, H, W), ((B, H, W) if u8 else (B, L, H, W)), (B, H, W)

    @staticmethod
    def _mean_arg(mean, u8: bool, what: str):
        if not u8:
            if mean is not None:
                raise ValueError(f"{what}: mean= belongs to a compact (uint8) call; float32 images have it subtracted already")
            return None
        if mean is None:
            raise ValueError(f"{what}: a compact (uint8) call needs mean= (B, G, R), what the float32 images have subtracted")
        m = [float(x) for x in mean]
        if len(m) != 3:
            raise ValueError(f"{what}: mean= takes three values (B, G, R)")
        return (C.c_float * 3)(*m)

    def forward(self, src_img: List[torch.Tensor], src_lbl: List[torch.Tensor], src_bbox: List[torch.Tensor],
                tar_lbl: torch.Tensor, tar_bbox: torch.Tensor, return_flow: bool = False, mean=None):
        """tsnet_forward (tsnet_forward_u8 when tar_lbl is uint8).  All tensors on one device.  Returns (rec (B,3,H,W), flows K x (B,h,w,2) | None)."""
        B = tar_lbl.shape[0]
        H, W, K = self.cfg.height, self.cfg.width, self.K
        if len(src_img) < K or len(src_lbl) < K or len(src_bbox) < K:
            raise ValueError(f"need {K} sources")
        u8, prep, ishape, lshape, bshape = self._form(tar_lbl, B)
        si = [prep(src_img[i], ishape, f"src_img[{i}]") for i in range(K)]
        sl = [prep(src_lbl[i], lshape, f"src_lbl[{i}]") for i in range(K)]
        sb = [prep(src_bbox[i], bshape, f"src_bbox[{i}]") for i in range(K)]
        tl = prep(tar_lbl, lshape, "tar_lbl")
        tb = prep(tar_bbox, bshape, "tar_bbox")
        m = self._mean_arg(mean, u8, "forward")
        out = torch.empty((B, 3, H, W), dtype=torch.float32, device=tl.device)
        flow = torch.empty((K, B, self.h, self.w, 2), dtype=torch.float32, device=tl.device) if return_flow else None
        self._same_device(*si, *sl, *sb, tl, tb)
        src = (self._ptr_array(si), self._ptr_array(sl), self._ptr_array(sb), tl.data_ptr(), tb.data_ptr())
        if u8:
            self._call("tsnet_forward_u8", *src, m, out.data_ptr(), _ptr(flow), B, stream=True)
        else:
            self._call("tsnet_forward", *src, out.data_ptr(), _ptr(flow), B, stream=True)
        self._held["forward"] = (si, sl, sb, tl, tb)
        return out, ([flow[i] for i in range(K)] if return_flow else None)

    def set_source_divisors(self, divisors: Optional[Sequence[float]] = None):
        """tsnet_set_source_divisors: per-source divisor of the source images on load -- 255 (default: the reference's `/255.0`,
        TSNet.py:267,286) or 1 for `use_prev` sources that are already in [0,1] (TSNet.py:269-276).  None resets all to 255."""
        d = list(divisors or [])
        arr = (C.c_float * max(len(d), 1))(*([float(x) for x in d] or [255.0]))
        self._call("tsnet_set_source_divisors", arr, len(d))

    def set_sources(self, src_img, src_lbl, src_bbox, shared: bool = False, mean=None):
        """tsnet_set_sources: encode and cache the K sources of a batch; forward_target then takes driving frames of that batch.
        shared=True (tsnet_set_sources_shared): ONE source set, tensors of batch 1, for every driving frame -- forward_target then
        takes any batch up to max_batch, and frame b of its result has the bits of forward() on (these sources, frame b)."""
        B = src_img[0].shape[0]
        if shared and B != 1:
            raise ValueError(f"shared sources must have batch 1, got {B}")
        K = self.K
        u8, prep, ishape, lshape, bshape = self._form(src_lbl[0], B)
        si = [prep(src_img[i], ishape, f"src_img[{i}]") for i in range(K)]
        sl = [prep(src_lbl[i], lshape, f"src_lbl[{i}]") for i in range(K)]
        sb = [prep(src_bbox[i], bshape, f"src_bbox[{i}]") for i in range(K)]
        m = self._mean_arg(mean, u8, "set_sources")
        self._same_device(*si, *sl, *sb)
        src = (self._ptr_array(si), self._ptr_array(sl), self._ptr_array(sb))
        if u8:
            self._call("tsnet_set_sources_u8", *src, m, B, int(shared), stream=True)
        elif shared:
            self._call("tsnet_set_sources_shared", *src, stream=True)
        else:
            self._call("tsnet_set_sources", *src, B, stream=True)
        self._held["set_sources"] = (si, sl, sb)

    def forward_target(self, tar_lbl, tar_bbox, return_flow: bool = False):
        B = tar_lbl.shape[0]
        H, W, K = self.cfg.height, self.cfg.width, self.K
        u8, prep, _, lshape, bshape = self._form(tar_lbl, B)
        tl = prep(tar_lbl, lshape, "tar_lbl")
        tb = prep(tar_bbox, bshape, "tar_bbox")
        out = torch.empty((B, 3, H, W), dtype=torch.float32, device=tl.device)
        flow = torch.empty((K, B, self.h, self.w, 2), dtype=torch.float32, device=tl.device) if return_flow else None
        self._same_device(tl, tb)
        self._call("tsnet_forward_target_u8" if u8 else "tsnet_forward_target", tl.data_ptr(), tb.data_ptr(), out.data_ptr(), _ptr(flow), B, stream=True)
        self._held["forward_target"] = (tl, tb)
        return out, ([flow[i] for i in range(K)] if return_flow else None)

    # ------------------------------------------------------------------ source bank
    @property
    def bank_capacity(self) -> int:
        """tsnet_bank_capacity: slots of the source bank, n_source * max_batch."""
        return int(self._call("tsnet_bank_capacity", check=False))

    def bank_put(self, slots, src_img, src_lbl, src_bbox, divisors: Optional[Sequence[float]] = None, mean=None):
        """tsnet_bank_put: encode sources of batch 1 into slots of the bank, one tsnet_set_sources' worth of work per n_source slots.
        slots: an int (the first slot: source i goes to slot slots + i) or one slot per source, in any order; a list is split into
        contiguous runs, one call each.  divisors: per source, 255 (default) or 1 for a frame already in [0,1]."""
        n = len(src_img)
        sl = list(range(slots, slots + n)) if isinstance(slots, int) else [int(x) for x in slots]
        if n < 1 or len(sl) != n or len(src_lbl) != n or len(src_bbox) != n or (divisors is not None and len(divisors) != n):
            raise ValueError(f"bank_put: {len(sl)} slots, {n} images, {len(src_lbl)} label maps, {len(src_bbox)} bboxes"
                             + ("" if divisors is None else f", {len(divisors)} divisors") + ": need one of each per source")
        if len(set(sl)) != n:
            raise ValueError("bank_put: a slot is named twice")
        u8, prep, ishape, lshape, bshape = self._form(src_lbl[0], 1)
        si = [prep(src_img[i], ishape, f"src_img[{i}]") for i in range(n)]
        sb_ = [prep(src_bbox[i], bshape, f"src_bbox[{i}]") for i in range(n)]
        sl_ = [prep(src_lbl[i], lshape, f"src_lbl[{i}]") for i in range(n)]
        m = self._mean_arg(mean, u8, "bank_put")
        self._same_device(*si, *sl_, *sb_)
        lo = 0
        while lo < n:                                           # contiguous ascending runs
            hi = lo + 1
            while hi < n and sl[hi] == sl[hi - 1] + 1:
                hi += 1
            c = hi - lo
            arr = lambda ts: (C.c_void_p * c)(*[t.data_ptr() for t in ts[lo:hi]])
            div = None if divisors is None else (C.c_float * c)(*[float(x) for x in divisors[lo:hi]])
            if u8:
                self._call("tsnet_bank_put_u8", sl[lo], c, arr(si), arr(sl_), arr(sb_), m, div, stream=True)
            else:
                self._call("tsnet_bank_put", sl[lo], c, arr(si), arr(sl_), arr(sb_), div, stream=True)
            lo = hi
        self._held["bank_put"] = (si, sl_, sb_)

    def forward_bank(self, index, tar_lbl, tar_bbox, return_flow: bool = False):
        """tsnet_forward_bank.  index: (B, Kc) integers on the host (nested lists, numpy, a CPU tensor) -- row b lists the slots of
        driving frame b's sources, in order.  Returns (rec (B,3,H,W), flows Kc x (B,h,w,2) | None); frame b has the bits of forward()
        at B = 1 on (those sources, frame b)."""
        if isinstance(index, torch.Tensor):
            if index.is_cuda:
                raise ValueError("forward_bank: index must be on the host")
            if index.dtype.is_floating_point or index.dtype in (torch.bool, torch.complex64, torch.complex128):
                raise ValueError(f"forward_bank: index must hold integers, got {index.dtype}")
            rows = index.tolist()
        else:
            import numpy as np
            a = np.asarray(index)
            if a.dtype.kind not in "iu":
                raise ValueError(f"forward_bank: index must hold integers, got dtype {a.dtype}")
            rows = a.tolist()
        B = tar_lbl.shape[0]
        if not isinstance(rows, list) or len(rows) != B or not all(isinstance(r, list) and r and len(r) == len(rows[0])
                                                                   and all(isinstance(v, int) for v in r) for r in rows):
            raise ValueError(f"forward_bank: index must have shape (B, Kc) with B = {B} driving frames")
        Kc = len(rows[0])
        H, W = self.cfg.height, self.cfg.width
        u8, prep, _, lshape, bshape = self._form(tar_lbl, B)
        tl = prep(tar_lbl, lshape, "tar_lbl")
        tb = prep(tar_bbox, bshape, "tar_bbox")
        table = (C.c_int * (Kc * B))(*[rows[b][s] for s in range(Kc) for b in range(B)])     # the ABI's layout: entry s*B + b
        out = torch.empty((B, 3, H, W), dtype=torch.float32, device=tl.device)
        flow = torch.empty((Kc, B, self.h, self.w, 2), dtype=torch.float32, device=tl.device) if return_flow else None
        self._same_device(tl, tb)
        self._call("tsnet_forward_bank_u8" if u8 else "tsnet_forward_bank", table, Kc, tl.data_ptr(), tb.data_ptr(), out.data_ptr(), _ptr(flow), B,
                   stream=True)
        self._held["forward_bank"] = (tl, tb)
        return out, ([flow[i] for i in range(Kc)] if return_flow else None)

    def train_extras(self, src_img: List[torch.Tensor], tar_img: torch.Tensor):
        """tsnet_train_extras: the is_train branches of the reference forward (TSNet.py:327-331, 372-390, 402-405) for the
        forward that was just run.  Returns (warp_src_img_list: K x (B,3,H,W), loss_warp, loss_align) -- the losses as 0-d
        device tensors.  With pose_composite (the pose model, TSNet_pose.py:343-346, 386-404) the warped images carry the
        fixed-background composite and loss_align is None (that model has none)."""
        B = tar_img.shape[0]
        H, W, K = self.cfg.height, self.cfg.width, self.K
        si = [self._prep(src_img[i], (B, 3, H, W), f"src_img[{i}]") for i in range(K)]
        ti = self._prep(tar_img, (B, 3, H, W), "tar_img")
        warp = torch.empty((K, B, 3, H, W), dtype=torch.float32, device=ti.device)
        losses = torch.empty(2, dtype=torch.float32, device=ti.device)
        self._same_device(*si, ti)
        self._call("tsnet_train_extras", self._ptr_array(si), ti.data_ptr(), B, warp.data_ptr(), losses.data_ptr(), stream=True)
        self._held["train_extras"] = (si, ti)
        return [warp[i] for i in range(K)], losses[0], (None if self.cfg.pose_composite else losses[1])

    def stage(self, name: str, device, shape=None) -> torch.Tensor:
        """Copy of a stage tensor of the last forward, NHWC (see tsnet_stage_ptr); `shape` = trailing (H, W, C)
        for stages that are not at the feature resolution ("dec_up<i>")."""
        p = C.c_void_p()
        n = C.c_size_t()
        self._call("tsnet_stage_ptr", name.encode(), C.byref(p), C.byref(n))
        flat = _alias_device_bytes(p.value, n.value * 4, device).view(torch.float32).clone()
        return flat.view(-1, *(shape if shape is not None else (self.h, self.w, self.C)))

    def forward_macs(self, B: int) -> float:
        return float(self._call("tsnet_forward_macs", B, check=False))

    def timing_enable(self, on: bool):
        self._call("tsnet_timing_enable", int(on))

    def timing_read(self, reset: bool = True):
        ms = (C.c_double * _lib.TIMING_CLASSES)()
        cnt = (C.c_int64 * _lib.TIMING_CLASSES)()
        self._call("tsnet_timing_read", ms, cnt, int(reset))
        return {n: (ms[i], int(cnt[i])) for i, n in enumerate(_lib.TIMING_NAMES)}


def _alias_device_bytes(ptr: int, nbytes: int, device) -> torch.Tensor:
    """View `nbytes` of memory at `ptr` as a uint8 tensor without copying.

    cuda: through __cuda_array_interface__ (zero-copy, the engine keeps ownership);
    cpu (emulation build in tests): through ctypes."""
    dev = torch.device(device)
    if dev.type == "cuda":
        class _Holder:
            pass
        h = _Holder()
        h.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}
        return torch.as_tensor(h, device=dev)
    buf = (C.c_ubyte * nbytes).from_address(ptr)
    return torch.frombuffer(buf, dtype=torch.uint8)
