"""Frames in and out as YUV 4:2:0 (tsnet_yuv_coeffs, tsnet_rgb_to_yuv420, tsnet_yuv420_to_rgb, FrameLoader.to_yuv420 / from_yuv420 /
yuv_planes, video.Y4MWriter / Y4MReader, ClipRunner.run(y4m=), csrc/yuv_frames.hpp) -- CPU-emulation tier.
  * the numpy restatement of yuv_cases.py (the contract) against outside authorities: the real-valued formula over all 2^24 colours and the
    four tables (every byte within 0.51: 0.5 from the rounding, 255 * 2.5 / 65536 from the coefficients' rounding and the green correction),
    live Pillow's convert("YCbCr") for 601 full (within 1: Pillow truncates where T.871 rounds), the pinned tables, grey -> chroma 128;
  * every case through the C entries (outputs between sentinels) and FrameLoader, both layouts, forward and inverse: EQUALITY;
  * the two large frames and the round-trip bound; one refusal test per cause, each asserting that nothing was written;
  * Y4M writer -> reader, into the frame loader; ClipRunner.run(y4m=); the tools' flag.
The GPU tier (test_gpu_yuv_frames.py) runs the same cases through the HIP library."""
import io
import os
import sys
import time

import numpy as np
import pytest
import torch
from PIL import Image

import compact_cases as cc
import helpers as Hh
import yuv_cases as yc
from wacv23_tsnet_amd import demo, frames, video

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
TABLE_IDS = [f"{s}-{'full' if f else 'limited'}" for s, f in yc.TABLES]


# --------------------------------------------------------------------------------------------------- the restatement against outside authorities
def _every_colour(chunk):
    """colours [chunk << 20, (chunk + 1) << 20) as (n, 1, 1, 3) frames of one pixel: n = 1 blocks, whose chroma is the pixel's own"""
    v = np.arange(chunk << 20, (chunk + 1) << 20, dtype=np.uint32)
    return np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], -1).astype(np.uint8).reshape(-1, 1, 1, 3)


@pytest.mark.parametrize("table", yc.TABLES, ids=TABLE_IDS)
def test_restatement_against_the_real_formula(table):
    """all 2^24 colours: every byte within 0.51 of the real-valued matrix; nothing clamps but Cb of pure blue and Cr of pure red in full range"""
    fwd, _ = yc.derive(*table)
    rows, offs, _ = yc.matrix(*table)
    worst, clamped = 0.0, set()
    for chunk in range(16):
        rgb = _every_colour(chunk)
        Y, Cb, Cr, raw = yc.rgb_to_yuv_planes(rgb, fwd)
        p = rgb.reshape(-1, 3).astype(np.float64)
        for r, got in enumerate((Y, Cb, Cr)):
            real = p @ np.array(rows[r]) + offs[r]
            worst = max(worst, float(np.abs(got.reshape(-1) - real).max()))
        for r, plane in ((1, raw[0]), (2, raw[1])):
            for i in np.flatnonzero((plane.reshape(-1) < 0) | (plane.reshape(-1) > 255)):
                clamped.add((r,) + tuple(int(c) for c in rgb.reshape(-1, 3)[i]))
    print(f"[yuv] {table}: worst distance from the real formula {worst:.4f}, clamped {sorted(clamped)}")
    assert worst <= 0.51, worst
    assert clamped == ({(1, 0, 0, 255), (2, 255, 0, 0)} if table[1] else set()), clamped


def test_restatement_against_pillow():
    """601 full is JFIF: within 1 of Pillow's convert("YCbCr") over all 2^24 colours (Pillow truncates where T.871 rounds)"""
    fwd, _ = yc.derive("bt601", True)
    worst = 0
    for chunk in range(16):
        rgb = _every_colour(chunk)
        pil = np.asarray(Image.fromarray(rgb.reshape(1024, 1024, 3), "RGB").convert("YCbCr")).reshape(-1, 3).astype(np.int64)
        Y, Cb, Cr, _ = yc.rgb_to_yuv_planes(rgb, fwd)
        ours = np.stack([Y.reshape(-1), Cb.reshape(-1), Cr.reshape(-1)], -1)
        worst = max(worst, int(np.abs(ours - pil).max()))
    assert worst <= 1, (worst, "Pillow %s" % Image.__version__)


@pytest.mark.parametrize("table", yc.TABLES, ids=TABLE_IDS)
def test_tables_are_the_pinned_ones(emu_lib, table):
    fwd, inv = yc.derive(*table)
    oy = 0 if table[1] else 16
    assert tuple(map(tuple, fwd.reshape(3, 4)[:, :3])) == yc.PINNED_FWD[table] and list(fwd.reshape(3, 4)[:, 3]) == [oy, 128, 128]
    assert tuple(inv[:5]) == yc.PINNED_INV[table] and inv[5] == oy
    rc, cf, ci = yc.coeffs_c(emu_lib, *table)
    assert rc == 0 and np.array_equal(cf, fwd) and np.array_equal(ci, inv)
    ld = frames.FrameLoader("cpu", lib=emu_lib)
    a, b = ld.yuv_tables(*table)
    assert np.array_equal(a, fwd) and np.array_equal(b, inv) and ld.yuv_tables(*table)[0] is a              # cached per (standard, range)


def test_coeffs_refusals(emu_lib):
    rc, fwd, inv = yc.coeffs_c(emu_lib, 2020, True)
    assert rc == -1 and (fwd == -7).all() and (inv == -7).all()
    assert emu_lib.tsnet_op_last_error().decode().startswith("yuv_coeffs")
    assert emu_lib.tsnet_yuv_coeffs(601, 1, None, None) == -1
    with pytest.raises(ValueError):
        frames.FrameLoader("cpu", lib=emu_lib).yuv_tables("bt2020")


@pytest.mark.parametrize("table", yc.TABLES, ids=TABLE_IDS)
def test_grey_has_chroma_128(emu_lib, table):
    """every grey level, on a frame with blocks of n = 4, 2 and 1: chroma exactly 128 (the green correction), in the restatement and the kernel"""
    g = np.arange(256, dtype=np.uint8).repeat(3 * 5).reshape(256, 3, 5)                         # frame f: 3 x 5 pixels of grey level f
    rgb = np.stack([g, g, g], -1)
    want = yc.rgb_to_yuv(rgb, yc.derive(*table)[0])
    assert (want[:, 15:] == 128).all()
    if table[1]:
        assert (want[:, :15] == g.reshape(256, 15)).all()                                        # and full-range luma is the grey level itself
    got = frames.FrameLoader("cpu", lib=emu_lib).to_yuv420(rgb, "i420", *table)
    assert np.array_equal(got.numpy(), want)


# ----------------------------------------------------------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("cid", yc.IDS)
def test_cases_emulated(emu_lib, cid):
    yc.check_case(emu_lib, "cpu", frames.FrameLoader("cpu", lib=emu_lib), cid)


def test_cases_reach_what_they_are_for():
    """the case list does what its comments say: every row alignment, every block count, both clamps"""
    e = yc.expected("1x64x130-primaries")
    y, cb, cr = frames.yuv_planes(e["want"]["i420"], 64, 130, "i420")
    assert y.shape == (1, 64, 130) and cb.shape == cr.shape == (1, 32, 65)
    full_tables = [c for c in yc.CASES if c[2] == "primaries" and c[3][1]]
    assert full_tables and any(yc.expected(c[0])["want"]["i420"].max() == 255 for c in full_tables)
    assert {3 * s[2] % 4 for s in yc.SHAPES} == {0, 1, 2, 3} and {(s[1] * s[2]) % 2 for s in yc.SHAPES} == {0, 1}
    inv = yc.expected("2x18x33-random")["want_rgb"]["nv12"]
    assert inv.min() == 0 and inv.max() == 255                                                  # the inverse's clamps are reached
    ck = yc.expected("1x4x16-checker")
    _, cb, _ = frames.yuv_planes(ck["want"]["nv12"], 4, 16, "nv12")
    assert len(np.unique(cb)) == 1                                                              # a pixel-pitch checkerboard has one block mean


def test_yuv_planes_views():
    buf = torch.arange(2 * yc.frame_bytes(3, 5), dtype=torch.uint8).reshape(2, -1)
    for layout in yc.LAYOUTS:
        y, cb, cr = frames.FrameLoader.yuv_planes(buf, 3, 5, layout)
        ny, ncb, ncr = yc._unpack(buf.numpy(), 3, 5, layout)
        assert np.array_equal(y.numpy(), ny) and np.array_equal(cb.numpy(), ncb) and np.array_equal(cr.numpy(), ncr)
        assert y.data_ptr() == buf.data_ptr()                                                   # views, not copies
    with pytest.raises(ValueError):
        frames.yuv_planes(buf, 4, 5)


def test_large_frames(emu_lib):
    """every colour once (luma exhaustive, chroma on mixed blocks) and the lattice of constant blocks with its round trip: at most 1 per byte
    off with the full-range tables, 2 with the limited ones.  The emulator runs the whole 4096 x 4096 frame when a 512 x 512 cut of it says it
    will take under about ten seconds, else the cut alone."""
    ld = frames.FrameLoader("cpu", lib=emu_lib)
    rgb, want = yc.all_colours(512)
    t0 = time.perf_counter()
    got = ld.to_yuv420(np.array(rgb), "i420", "bt709", False).numpy()
    dt = time.perf_counter() - t0
    assert np.array_equal(got, want)
    print(f"[yuv] round trip worst per table: {yc.check_large(ld, None if dt * 64 < 10.0 else 512)}; 512 x 512 on the emulator: {dt * 1e3:.1f} ms")


# -------------------------------------------------------------------------------------------------------------------------------- refusals
SHAPE = yc.ERR_SHAPE


@pytest.mark.parametrize("cause", list(yc.ARG_ERRORS))
def test_argument_errors_write_nothing(emu_lib, cause):
    yc.check_refusal(emu_lib, "cpu", cause)


def test_same_buffer_is_refused(emu_lib):
    fwd, inv = yc.derive("bt601", True)
    buf, view = yc.guarded((1, 2 * 2 * 3), "cpu")                                                # large enough for either direction of a 2 x 2 frame
    assert yc.forward_c(emu_lib, view, (1, 2, 2), fwd, "i420", view) == -1 and emu_lib.tsnet_op_last_error().decode().startswith("rgb_to_yuv420")
    assert yc.inverse_c(emu_lib, view, (1, 2, 2), inv, "nv12", view) == -1 and "same buffer" in emu_lib.tsnet_op_last_error().decode()
    assert yc.untouched(buf)


def test_loader_value_errors(emu_lib):
    ld = frames.FrameLoader("cpu", lib=emu_lib)
    rgb = yc.make_rgb("loader", SHAPE, "random")
    yuv = yc.rgb_to_yuv(rgb, yc.derive("bt601", True)[0])
    for bad in (lambda: ld.to_yuv420(rgb, layout="yv12"), lambda: ld.to_yuv420(rgb, standard="bt2020"), lambda: ld.to_yuv420(rgb[0]),
                lambda: ld.to_yuv420(rgb.astype(np.float32)), lambda: ld.to_yuv420(rgb, out=torch.empty((2, 5), dtype=torch.uint8)),
                lambda: ld.from_yuv420(yuv, (6, 11)), lambda: ld.from_yuv420(yuv[:, :-1], (6, 10)), lambda: ld.from_yuv420(yuv, (0, 10)),
                lambda: ld.from_yuv420(yuv, (6, 10), out=torch.empty((2, 6, 10, 3), dtype=torch.float32))):
        with pytest.raises(ValueError):
            bad()
    out = torch.empty((2, yc.frame_bytes(6, 10)), dtype=torch.uint8)
    assert ld.to_yuv420(rgb, out=out).data_ptr() == out.data_ptr() and np.array_equal(out.numpy(), yuv)
    back = torch.empty((2, 6, 10, 3), dtype=torch.uint8)
    assert ld.from_yuv420(yuv, (6, 10), out=back) is back and np.array_equal(back.numpy(), yc.yuv_to_rgb(yuv, 6, 10, yc.derive("bt601", True)[1]))


# ------------------------------------------------------------------------------------------------------------------------------------- Y4M
def test_y4m_round_trip(tmp_path):
    h, w, n = 5, 7, 5
    yuv = np.random.default_rng(3).integers(0, 256, (n, yc.frame_bytes(h, w)), dtype=np.uint8)
    path = str(tmp_path / "a.y4m")
    with video.Y4MWriter(path, w, h, fps=(30000, 1001), full_range=False) as wr:
        assert wr.write(yuv[:2]) == 2 and wr.write(torch.from_numpy(yuv[2:4])) == 2 and wr.write(yuv[4]) == 1       # arrays, tensors, one frame
        with pytest.raises(ValueError):
            wr.write(yuv[:, :-1])
    raw = open(path, "rb").read()
    assert raw.startswith(b"YUV4MPEG2 W7 H5 F30000:1001 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\nFRAME\n")
    assert len(raw) == raw.index(b"\n") + 1 + n * (6 + yc.frame_bytes(h, w))
    with video.Y4MReader(path) as rd:
        assert (rd.width, rd.height, rd.fps, rd.interlace, rd.aspect, rd.colourspace, rd.full_range) == (7, 5, (30000, 1001), "p", (1, 1), "420jpeg", False)
        assert rd.frame_bytes == yc.frame_bytes(h, w)
        first = rd.read(2)
        assert first.dtype == torch.uint8 and np.array_equal(first.numpy(), yuv[:2])
        rest = list(rd.frames(2))
        assert [g.shape[0] for g in rest] == [2, 1] and np.array_equal(torch.cat(rest).numpy(), yuv[2:]) and rd.read(1).shape[0] == 0
    with video.Y4MReader(io.BytesIO(raw)) as rd:                                                 # a file object; read into the caller's tensor
        out = torch.zeros((8, rd.frame_bytes), dtype=torch.uint8)
        got = rd.read(8, out=out)
        assert got.shape[0] == n and got.data_ptr() == out.data_ptr() and np.array_equal(got.numpy(), yuv)
    assert np.array_equal(np.concatenate([g.numpy() for g in video.Y4MReader(path)]), yuv)     # iteration: a frame at a time


def _y4m(header, payload=b""):
    return io.BytesIO(header + b"\n" + payload)


def test_y4m_headers():
    one = b"FRAME\n" + bytes(range(6))
    for tag in (b" C420jpeg", b" C420mpeg2", b" C420paldv", b" C420", b""):                      # all taken as 4:2:0; siting is ignored
        rd = video.Y4MReader(_y4m(b"YUV4MPEG2 W2 H2 F25:1" + tag, one))
        assert rd.full_range is None and rd.read(1).numpy().tolist() == [list(range(6))]
    rd = video.Y4MReader(_y4m(b"YUV4MPEG2 W2 H2 F25:1 Ip A4:3 C420jpeg XYSCSS=420JPEG XCOLORRANGE=FULL", b"FRAME Ip\n" + bytes(6)))
    assert rd.full_range is True and rd.aspect == (4, 3) and rd.read(3).shape == (1, 6)
    for header, word in ((b"YUV4MPEG2 W2 H2 F25:1 C444", "C444"), (b"YUV4MPEG2 W2 H2 F25:1 C422", "C422"), (b"YUV4MPEG2 W2 H2 F25:1 C420p10", "C420p10"),
                         (b"YUV4MPEG2 W2 H2 F25:1 Cmono", "Cmono"), (b"YUV4MPEG2 W2 H2 F25:1 It C420jpeg", "interlaced"),
                         (b"YUV4MPEG2 W2 H2 F25:1 Ib", "interlaced"), (b"YUV4MPEG2 F25:1 C420", "size"), (b"RIFF W2 H2", "not a Y4M")):
        with pytest.raises(ValueError, match=word):
            video.Y4MReader(_y4m(header, one))
    with pytest.raises(ValueError, match="ends inside"):
        video.Y4MReader(_y4m(b"YUV4MPEG2 W2 H2 F25:1", b"FRAME\n" + bytes(5))).read(1)
    with pytest.raises(ValueError, match="FRAME"):
        video.Y4MReader(_y4m(b"YUV4MPEG2 W2 H2 F25:1", b"PLANE\n" + bytes(6))).read(1)
    with pytest.raises(ValueError):
        video.Y4MWriter(io.BytesIO(), 0, 2)


def test_y4m_into_the_frame_loader(emu_lib, tmp_path):
    """a written file, read, through from_yuv420 and FrameLoader.face: equal to FrameLoader.face on the restatement's RGB"""
    ld = frames.FrameLoader("cpu", lib=emu_lib)
    h, w = 45, 62
    rgb = yc.make_rgb("y4m-face", (3, h, w), "random")
    fwd, inv = yc.derive("bt601", True)
    yuv = ld.to_yuv420(rgb)
    yc.write_y4m(str(tmp_path / "in.y4m"), yuv, w, h)
    with video.Y4MReader(str(tmp_path / "in.y4m")) as rd:
        got = rd.read(3, pinned=False)
        back = ld.from_yuv420(got, (rd.height, rd.width), full_range=rd.full_range)
    want_rgb = yc.yuv_to_rgb(yc.rgb_to_yuv(rgb, fwd), h, w, inv)
    assert np.array_equal(back.numpy(), want_rgb)
    crop = [3, 40, -4, 50]
    assert torch.equal(ld.face(back, crop, size=(32, 32)), ld.face(want_rgb, crop, size=(32, 32)))


# ------------------------------------------------------------------------------------------------------------------------- the clip harness
K, H, W = 2, 32, 32


class _EmuModel:
    """what demo.ClipRunner asks of a model, on the emulator (test_compact_inputs.py's narrow net)"""

    def __init__(self, lib):
        self.lib, self.n_source = lib, K
        self.cfg, self.sd = cc.narrow_net(L=2, n_source=K)

    def _device(self):
        return torch.device("cpu")

    def _new_engine(self, batch):
        return Hh.make_engine(self.cfg, self.sd, H, W, batch, "cpu", lib=self.lib)


def test_clip_runner_writes_y4m(emu_lib, tmp_path):
    """3 driving frames at batch 2 (a ragged last group), generated frames and pasted full frames (an odd-sized video)"""
    src, drv = cc.Inputs(2, K, 1, H, W, seed=40), cc.Inputs(2, 1, 3, H, W, seed=41)
    vid = np.random.default_rng(9).integers(0, 256, (3, 51, 61, 3), dtype=np.uint8)
    with demo.ClipRunner(_EmuModel(emu_lib), *src.src("f", range(K)), batch=2) as runner:
        small, full = yc.check_clip_runner(runner, frames.FrameLoader("cpu", lib=emu_lib), drv.tar("f"), vid, (-5, 8, 41, 48), tmp_path)
    assert small.shape == (3, H, W, 3) and full.shape == vid.shape


@pytest.mark.parametrize("tool", ["demo_clip", "demo_pose_clip"])
def test_tools_take_a_y4m_path(tool, monkeypatch, capsys):
    """the flag exists and wants a path (checked as the feather flags are: through the tool's own parser, before any device work)"""
    mod = __import__(tool)
    monkeypatch.setattr(sys, "argv", [tool + ".py", "--y4m"])
    with pytest.raises(SystemExit) as e:
        mod.main()
    assert e.value.code == 2 and "--y4m" in capsys.readouterr().err
    monkeypatch.setattr(sys, "argv", [tool + ".py", "--help"])
    with pytest.raises(SystemExit) as e:
        mod.main()
    assert e.value.code == 0 and "--y4m OUT.y4m" in capsys.readouterr().out
