"""Y4M (YUV4MPEG2) files: uncompressed planar YUV 4:2:0 video with a text header.  Host side, pure Python, no library.

    YUV4MPEG2 W640 H480 F25:1 Ip A1:1 C420jpeg XCOLORRANGE=FULL\\n        the stream header
    FRAME\\n  + h*w + 2*ch*cw bytes: the Y plane, then Cb, then Cr           per frame (ch = (h+1)//2, cw = (w+1)//2)

A frame's payload is the "i420" layout of `FrameLoader.to_yuv420` / `from_yuv420`.  `ffmpeg -i clip.mp4 -pix_fmt yuv420p clip.y4m` makes such a
file, `ffmpeg -i out.y4m out.mp4` and any player take one.  Encoding and decoding stay with the caller."""
from __future__ import annotations

import os
from typing import Iterator, Optional, Tuple

import numpy as np
import torch

MAGIC = b"YUV4MPEG2"
C420 = ("420jpeg", "420mpeg2", "420paldv", "420")                   # 8-bit 4:2:0; they differ in where the chroma samples sit


def frame_bytes(width: int, height: int) -> int:
    return width * height + 2 * ((width + 1) // 2) * ((height + 1) // 2)


def _as_rows(frames, n: int) -> np.ndarray:
    """host frames, tensor or array, as a contiguous (k, n) uint8 array"""
    if isinstance(frames, torch.Tensor):
        if frames.device.type != "cpu":
            raise ValueError("Y4MWriter.write takes host frames: download them first (yuv.cpu(), or a pinned tensor)")
        frames = frames.numpy()
    a = np.ascontiguousarray(frames)
    if a.dtype != np.uint8 or a.size % n != 0 or (a.ndim > 1 and a.shape[-1] != n):
        raise ValueError(f"expected whole uint8 I420 frames of {n} bytes, got shape {a.shape} {a.dtype}")
    return a.reshape(-1, n)


class Y4MWriter:
    """Writes I420 frames to a Y4M file.  path_or_file: a path (opened here and closed by `close`) or a binary file object (left open).
    The header says C420jpeg -- chroma sited at the centre of its 2 x 2 block, as `to_yuv420` computes it -- and XCOLORRANGE=FULL or LIMITED.

        with Y4MWriter("out.y4m", 640, 480, fps=(30000, 1001)) as wr:
            wr.write(loader.to_yuv420(frames).cpu())"""

    def __init__(self, path_or_file, width: int, height: int, fps: Tuple[int, int] = (25, 1), full_range: bool = True):
        self.width, self.height, self.fps, self.full_range = int(width), int(height), (int(fps[0]), int(fps[1])), bool(full_range)
        if self.width < 1 or self.height < 1 or self.fps[0] < 1 or self.fps[1] < 1:
            raise ValueError(f"bad size {width} x {height} or frame rate {fps}")
        self.frame_bytes = frame_bytes(self.width, self.height)
        self.frames_written = 0
        self._own = isinstance(path_or_file, (str, bytes, os.PathLike))
        self._f = open(path_or_file, "wb") if self._own else path_or_file
        self._f.write(self.header().encode("ascii"))

    def header(self) -> str:
        return (f"YUV4MPEG2 W{self.width} H{self.height} F{self.fps[0]}:{self.fps[1]} Ip A1:1 C420jpeg "
                f"XCOLORRANGE={'FULL' if self.full_range else 'LIMITED'}\n")

    def write(self, frames_i420) -> int:
        """frames_i420: (k, frame_bytes) uint8 (or one frame), host tensor or array; returns k"""
        rows = _as_rows(frames_i420, self.frame_bytes)
        for r in rows:
            self._f.write(b"FRAME\n")
            self._f.write(memoryview(r))
        self.frames_written += len(rows)
        return len(rows)

    def close(self):
        if self._f is not None:
            self._f.flush()
            if self._own:
                self._f.close()
            self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


class Y4MReader:
    """Reads the frames of a Y4M file as I420 bytes.  Header fields: width, height, fps (num, den), interlace ("p"), aspect (num, den),
    colourspace (the C tag's value, "420jpeg" when there is none), full_range (True / False from XCOLORRANGE, None when absent), frame_bytes.
    C420jpeg, C420mpeg2, C420paldv, C420 and a missing C tag are all taken as 8-bit 4:2:0.  They differ in chroma siting (centred, left
    co-sited, co-sited with alternating lines); that difference is IGNORED here -- `from_yuv420` replicates every sample over its 2 x 2 block
    whatever the tag says.  Every other colour space (C422, C444, Cmono, the high-bit-depth forms) and interlaced material (It, Ib, Im) are
    refused with a ValueError.  Parameters of the FRAME lines are skipped.

        with Y4MReader("clip.y4m") as rd:
            for yuv in rd.frames(8, pinned=True):                   # (<= 8, frame_bytes) uint8
                rgb = loader.from_yuv420(yuv, (rd.height, rd.width), full_range=bool(rd.full_range))       # no tag: limited, as most video is"""

    def __init__(self, path_or_file):
        self._own = isinstance(path_or_file, (str, bytes, os.PathLike))
        self._f = open(path_or_file, "rb") if self._own else path_or_file
        try:
            self._parse(self._line(256))
        except Exception:
            self.close()
            raise

    def _line(self, limit: int) -> bytes:
        line = self._f.readline(limit)
        if line and not line.endswith(b"\n"):
            raise ValueError(f"Y4M: a header line longer than {limit} bytes or cut short: {line[:40]!r}")
        return line[:-1]

    def _parse(self, line: bytes):
        tok = line.split(b" ")
        if tok[0] != MAGIC:
            raise ValueError(f"not a Y4M file: it starts with {line[:16]!r}, not {MAGIC!r}")
        self.width = self.height = 0
        self.fps, self.interlace, self.aspect, self.colourspace, self.full_range = (25, 1), "p", (0, 0), "420jpeg", None
        ratio = lambda v: tuple(int(x) for x in v.split(":"))
        for t in (t.decode("ascii", "replace") for t in tok[1:] if t):
            k, v = t[0], t[1:]
            if k == "W":
                self.width = int(v)
            elif k == "H":
                self.height = int(v)
            elif k == "F":
                self.fps = ratio(v)
            elif k == "I":
                self.interlace = v
            elif k == "A":
                self.aspect = ratio(v)
            elif k == "C":
                self.colourspace = v
            elif k == "X" and v.startswith("COLORRANGE="):
                self.full_range = {"FULL": True, "LIMITED": False}.get(v.split("=", 1)[1])
        if self.width < 1 or self.height < 1:
            raise ValueError(f"Y4M: no frame size in the header {line!r}")
        if self.colourspace not in C420:
            raise ValueError(f"Y4M: colour space C{self.colourspace} is not 8-bit 4:2:0 (one of {', '.join('C' + c for c in C420)}); convert it "
                             "first, e.g. ffmpeg -pix_fmt yuv420p")
        if self.interlace not in ("p", "?"):
            raise ValueError(f"Y4M: interlaced material (I{self.interlace}) is not supported; deinterlace it first")
        self.frame_bytes = frame_bytes(self.width, self.height)

    def read(self, n: int = 1, pinned: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """up to n frames -> (k, frame_bytes) uint8 host tensor, k < n at the end of the file (k = 0: nothing left).  pinned: the tensor is
        page-locked, for an asynchronous upload.  out: a (>= n, frame_bytes) uint8 host tensor to read into (its first k rows are returned)."""
        if out is None:
            out = torch.empty((n, self.frame_bytes), dtype=torch.uint8)
            if pinned:
                out = out.pin_memory()
        elif out.dtype != torch.uint8 or out.dim() != 2 or out.shape[0] < n or out.shape[1] != self.frame_bytes or not out.is_contiguous() \
                or out.device.type != "cpu":
            raise ValueError(f"out must be a contiguous host uint8 tensor of shape (>= {n}, {self.frame_bytes})")
        rows = out.numpy()
        k = 0
        while k < n:
            line = self._line(256)
            if not line:                                             # the end of the file
                break
            if line.split(b" ")[0] != b"FRAME":
                raise ValueError(f"Y4M: expected a FRAME line before frame {k}, got {line[:40]!r}")
            got = self._f.readinto(memoryview(rows[k]))
            if got != self.frame_bytes:
                raise ValueError(f"Y4M: the file ends inside a frame ({got} of {self.frame_bytes} bytes)")
            k += 1
        return out[:k]

    def frames(self, n: int = 1, pinned: bool = False) -> Iterator[torch.Tensor]:
        """groups of up to n frames until the file ends; every group is a new tensor"""
        while True:
            g = self.read(n, pinned=pinned)
            if g.shape[0]:
                yield g
            if g.shape[0] < n:
                return

    def __iter__(self):
        return self.frames(1)

    def close(self):
        if self._f is not None and self._own:
            self._f.close()
        self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
