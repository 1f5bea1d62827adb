"""The one way from the Python wrappers into the C ABI (include/tsnet_abi.h): device, stream, return code, error text."""
from __future__ import annotations

import contextlib
from typing import Optional

import torch

from . import _lib

_OP = object()          # the message comes from tsnet_op_last_error (no engine handle)


def last_error(lib, handle=_OP) -> str:
    return (lib.tsnet_op_last_error() if handle is _OP else lib.tsnet_last_error(handle)).decode()


def fail(lib, entry: str, rc: int, handle=_OP, refusal=RuntimeError):
    raise (refusal if rc == -1 else RuntimeError)(f"{entry} failed ({rc}): {last_error(lib, handle)}")


def call(lib, entry: str, *args, device=None, stream: Optional[bool] = None, handle=_OP, refusal=RuntimeError, what: Optional[str] = None,
         check: bool = True) -> int:
    """rc = lib.<entry>(*args[, stream]) with `device` current, checked.

    device: the torch.device of the call's tensors.  A GPU is made the current HIP device for the duration of the call -- the library
    allocates, creates its streams and launches on the CURRENT device, which may be another one (model on cuda:1, current device 0).
    None: a host-only entry (tsnet_fit_*_curves, tsnet_face_adapt_*, tsnet_smooth_keypoints, tsnet_bicubic_*, tsnet_yuv_coeffs,
    tsnet_gaussian_box_params), no device, no stream.
    stream: whether the entry's last parameter is a stream; the default is "when a device is given".  It gets torch's current stream
    of `device`, None on the CPU (emulation build).  Engine entries that allocate but take no stream pass stream=False.
    handle: an engine handle (None before tsnet_create has made one) -- the message is then tsnet_last_error(handle), else
    tsnet_op_last_error().  The handle is NOT added to args.

    rc != 0 raises "{entry} failed ({rc}): {last error}", entry as called (`_u8` included; `what` replaces it where a wrapper has always
    named something else).  The type is RuntimeError.  The one exception: the entries behind FrameLoader.feather_mask, to_yuv420 and
    from_yuv420 pass refusal=ValueError, and their rc == -1 (TSNET_ERR_ARG, the library refusing the arguments) is a ValueError; every
    other rc of theirs is a RuntimeError as well.  check=False returns rc unchecked for the three wrappers that word their own error with
    `last_error` / `fail`: FrameLoader._box_params (ValueError for any rc != 0: the radius is the caller's), yuv_tables, and
    bicubic_table_c's tap count (negative = failed)."""
    gpu = device is not None and device.type == "cuda"
    if stream or (stream is None and device is not None):
        args += (torch.cuda.current_stream(device).cuda_stream if gpu else None,)
    with torch.cuda.device(device) if gpu else contextlib.nullcontext():
        rc = getattr(lib, entry)(*args)
    if check and rc != 0:
        fail(lib, what or entry, rc, handle, refusal)
    return rc


class Wrapper:
    """What FrameLoader and the rasterisers share: the library, the device, and what their calls keep referenced.

    lib: tests pass the CPU emulation build; product code leaves it None (the in-tree HIP library, no fallback).
    _held: public method -> what its last call uploaded, made contiguous or replaced (an old pool, an old workspace) for its launches,
    by name; a method that calls other public methods lists theirs too.  Assigned once per call, so it holds each method's last call and
    nothing older ("What a wrapper keeps referenced")."""

    def __init__(self, device, lib=None):
        self.lib = lib if lib is not None else _lib.load()
        self.device = torch.device(device)
        self._held = {}
