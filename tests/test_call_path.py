"""The Python wrappers' one way into the library (wacv23_tsnet_amd/_call.py) and what they keep referenced after a call (`_held`), on the CPU:
a stub library for the helper's own rules, the emulation build for the wrappers."""
import ctypes as C

import numpy as np
import pytest
import torch

from wacv23_tsnet_amd import _lib, frames, raster
from wacv23_tsnet_amd._call import call


class StubLib:
    """tsnet_stub returns `rc` and records its arguments; the two last-error entries answer differently"""

    def __init__(self, rc=0):
        self.rc, self.args, self.handles = rc, None, []

    def tsnet_stub(self, *args):
        self.args = args
        return self.rc

    def tsnet_stub_u8(self, *args):
        return self.rc

    def tsnet_op_last_error(self):
        return b"stub: the op's text"

    def tsnet_last_error(self, handle):
        self.handles.append(handle)
        return b"stub: the handle's text"


def tensors(held):
    """every tensor in a `_held` value, however nested"""
    if isinstance(held, torch.Tensor):
        return [held]
    if isinstance(held, dict):
        held = list(held.values())
    return [t for v in held for t in tensors(v)] if isinstance(held, (list, tuple)) else []


@pytest.mark.parametrize("rc", [-1, -4])
def test_failure_message_and_type(rc):
    lib = StubLib(rc)
    with pytest.raises(Exception) as e:                                    # the default: RuntimeError whatever the code
        call(lib, "tsnet_stub", 1, 2)
    assert type(e.value) is RuntimeError and str(e.value) == f"tsnet_stub failed ({rc}): stub: the op's text"
    with pytest.raises(Exception) as e:                                    # feather_mask, to_yuv420, from_yuv420: a refusal (-1) alone is a ValueError
        call(lib, "tsnet_stub_u8", refusal=ValueError)
    assert type(e.value) is (ValueError if rc == -1 else RuntimeError) and str(e.value) == f"tsnet_stub_u8 failed ({rc}): stub: the op's text"
    assert lib.handles == []
    handle = C.c_void_p(7)
    with pytest.raises(Exception) as e:                                    # an engine handle's entry: tsnet_last_error(handle)
        call(lib, "tsnet_stub", handle, 1, handle=handle)
    assert type(e.value) is RuntimeError and str(e.value) == f"tsnet_stub failed ({rc}): stub: the handle's text"
    assert lib.handles == [handle] and lib.args == (handle, 1)
    with pytest.raises(RuntimeError, match=r"^tsnet_stub failed"):        # before tsnet_create has made one
        call(lib, "tsnet_stub", handle=None)
    assert lib.handles == [handle, None]
    assert call(lib, "tsnet_stub", check=False) == rc


def test_stream_goes_last_and_is_none_on_the_cpu():
    lib = StubLib()
    assert call(lib, "tsnet_stub", 5, 6, device=torch.device("cpu")) == 0 and lib.args == (5, 6, None)
    call(lib, "tsnet_stub", 5, 6)                                          # a host-only entry: no device, no stream parameter
    assert lib.args == (5, 6)
    call(lib, "tsnet_stub", 5, device=torch.device("cpu"), stream=False)   # device work without a stream parameter (tsnet_load_weights)
    assert lib.args == (5,)
    call(lib, "tsnet_stub", 5, stream=True)                                # an engine on the emulation build: finalized without a device
    assert lib.args == (5, None)


def test_a_refusal_of_the_library_itself(emu_lib):
    with pytest.raises(RuntimeError, match=r"^tsnet_gaussian_box_params failed \(-1\): gaussian_box_params"):
        call(emu_lib, "tsnet_gaussian_box_params", 1.0, 3, None, None, None)
    ld = frames.FrameLoader("cpu", lib=emu_lib)
    with pytest.raises(ValueError, match=r"^feather radius -2: gaussian_box_params"):     # _box_params: its own words, ValueError
        ld.feather_inset(-2)


def test_pose_bbox_and_to_square_hold_one_call(emu_lib):
    r = raster.PoseRasteriser("cpu", lib=emu_lib)
    maps = torch.zeros((2, 8, 6), dtype=torch.uint8)
    maps[:, 2:5, 1:4] = 3
    for method, name in ((lambda: r.bbox(maps.clone()), "bbox"), (lambda: r.to_square(maps.clone(), (4, 8)), "to_square")):
        method()
        first = tensors(r._held)
        assert len(tensors(r._held[name])) == (1 if name == "bbox" else 3)
        method()
        method()
        assert len(tensors(r._held)) == len(first) and not any(a is b for a in tensors(r._held[name]) for b in first)


def test_pose_clip_labels_holds_what_its_calls_uploaded(emu_lib, monkeypatch):
    launched = []

    def recording(lib, entry, *args, **kw):
        launched.append((entry, args))
        return call(lib, entry, *args, **kw)

    monkeypatch.setattr(raster, "call", recording)
    r = raster.PoseRasteriser("cpu", lib=emu_lib)
    rng = np.random.default_rng(11)
    pts = [rng.uniform(4, 44, (137, 2)) for _ in range(2)]
    r.clip_labels(pts, (48, 48), window=(2, 4, 42, 46), img_size=(8, 16))
    assert [e for e, _ in launched] == ["tsnet_fit_pose_curves", "tsnet_raster_pose", "tsnet_label_bbox", "tsnet_resize_pad", "tsnet_resize_pad"]
    inputs = {"tsnet_fit_pose_curves": (), "tsnet_raster_pose": (0, 1), "tsnet_label_bbox": (0,), "tsnet_resize_pad": (0, 4, 5)}   # what each reads of the uploads
    held = {t.data_ptr() for t in tensors(r._held["clip_labels"])}
    for entry, args in launched:
        assert all(args[i] in held for i in inputs[entry]), entry
    tables = [a[4] for e, a in launched if e == "tsnet_resize_pad"]
    assert tables[0] != tables[1]                                          # both to_square calls' tables: the second did not take the first's place
    n = len(tensors(r._held))
    r.clip_labels(pts, (48, 48), window=(2, 4, 42, 46), img_size=(8, 16))
    assert len(tensors(r._held)) == n


def test_paste_with_feather_holds_both_calls_inputs(emu_lib):
    ld = frames.FrameLoader("cpu", lib=emu_lib)
    g = torch.Generator().manual_seed(3)
    gen, fr = (torch.randint(0, 256, (2, 40, 40, 3), generator=g, dtype=torch.uint8) for _ in range(2))
    mask = torch.randint(0, 256, (2, 40, 40), generator=g, dtype=torch.uint8)
    for box in ((5, 6, 33, 35), [(5, 6, 33, 35), (1, 2, 30, 39)]):
        ld.paste(gen, fr, box, mask=mask, feather=2)
        held = ld._held["paste"]
        assert held["gen"] is gen and held["feather_mask"]["src"] is mask and ld._held["feather_mask"]["src"] is mask    # on the CPU `.to` is the identity
        assert held["mask"] is not mask and tuple(held["mask"].shape) == (2, 40, 40)                                   # the blurred mask the paste read
    assert held["pool"] is ld._pool and held["old_pool"] is None and held["descriptors"].shape == (2, 8)
    ld.feather_mask(mask[:1], 1)                                           # the two slots are separate: paste's stays
    assert ld._held["paste"] is held and ld._held["feather_mask"]["src"] is not mask


def test_one_table_binds_every_symbol(emu_lib):
    assert set(_lib.ABI_SYMBOLS) == set(_lib.ABI) and len(_lib.ABI_SYMBOLS) == len(_lib.ABI)
    for name, sig in _lib.ABI.items():
        argtypes, restype = sig if isinstance(sig, tuple) else (sig, C.c_int)
        fn = getattr(emu_lib, name)                                        # a current build exports every one
        assert fn.restype is restype, name
        assert (fn.argtypes is None) if argtypes is None else (list(fn.argtypes) == list(argtypes)), name
