"""ctypes binding of the C ABI in include/tsnet_abi.h.

`load()` opens the in-tree HIP library (wacv23_tsnet_amd/lib/libtsnet_hip.so, built by
`__graft_entry__.build()` / `python -m wacv23_tsnet_amd.build`).  There is no fallback: if the
library is missing or fails to load, importing code gets a RuntimeError telling it to build.

torch must be imported before the library is opened: the library depends on libamdhip64.so.7,
and the dynamic loader then re-uses the HIP runtime torch already mapped (same SONAME), so
torch's allocations and our kernel launches share one runtime and one stream namespace.
"""
from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  (must precede CDLL, see module docstring)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libtsnet_hip.so")
MAX_SOURCES = 8
TIMING_CLASSES = 9
TIMING_NAMES = ("conv", "stats", "elementwise", "flow", "warp", "pack", "upsample", "other", "conv_res")

class TsnetCfg(C.Structure):
    """struct tsnet_cfg (include/tsnet_abi.h)."""
    _fields_ = [
        ("label_nc", C.c_int), ("n_blocks", C.c_int), ("n_downsampling", C.c_int), ("n_source", C.c_int),
        ("ngf", C.c_int), ("enc_blocks", C.c_int), ("addcoords", C.c_int), ("pose_composite", C.c_int),
        ("pose_mean", C.c_float * 3), ("height", C.c_int), ("width", C.c_int), ("max_batch", C.c_int), ("operand_mode", C.c_int),
    ]


_fp = C.POINTER(C.c_float)
_vp = C.c_void_p
CONV_EPI_INFO = 8


class TsnetConvEpi(C.Structure):
    """struct tsnet_conv_epi (include/tsnet_abi.h): the optional parts of tsnet_op_conv2d_epi; device pointers as integers."""
    _fields_ = [
        ("stats", C.c_int), ("repeat", C.c_int), ("part", _vp), ("part_capacity", C.c_longlong), ("alpha", _vp), ("beta", _vp),
        ("counters", _vp), ("counters_nonzero_out", C.POINTER(C.c_int)), ("addend", _vp), ("add_nmod", C.c_int), ("amax_out", _vp),
        ("in_amax", _vp), ("bound_add", C.c_float), ("x_bf16", C.c_int), ("y_bf16", C.c_int), ("info_out", C.POINTER(C.c_int)),
    ]


_i, _pp, _ip = C.c_int, C.POINTER(_vp), C.POINTER(C.c_int)
_conv2d = [_vp, _i, _i, _i, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _i, C.c_float, _i, _i, _i, _vp, _vp]
_prepare = [_vp] + [_i] * 7 + [_vp, _vp, _vp, _i, _vp, _vp, _vp, _i] + [_i] * 6        # frames, one box, two axis tables, output geometry
_prepare_boxes = [_vp] + [_i] * 3 + [_vp, _vp, _vp, _i] + [_i] * 6                      # frames, descriptors + pool, output geometry
_face_labels = [_vp, _vp, _i, _vp, _vp, _vp, _i, _i, _vp, C.c_longlong, _i, _i, _vp, _vp, _vp]
_yuv = [_vp, _i, _i, _i, _vp, _i, _vp, _vp]

# Every symbol include/tsnet_abi.h declares (tests/test_abi.py checks header <-> library <-> this table): name -> argtypes, or
# (argtypes, restype) where the entry does not return an int (restype None: void); argtypes None: the entry takes nothing.
ABI = {
    "tsnet_abi_version": None,
    "tsnet_create": [C.POINTER(TsnetCfg), _pp],
    "tsnet_load_weights": [_vp, C.c_char_p, _vp, C.POINTER(C.c_int64), _i],
    "tsnet_finalize": [_vp, _vp],
    "tsnet_destroy": ([_vp], None),
    "tsnet_last_error": ([_vp], C.c_char_p),
    "tsnet_num_params": [_vp],
    "tsnet_param_info": [_vp, _i, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), _ip],
    "tsnet_packed_weights": [_vp, _pp, C.POINTER(C.c_size_t)],
    "tsnet_forward": [_vp, _pp, _pp, _pp, _vp, _vp, _vp, _vp, _i, _vp],
    "tsnet_set_source_divisors": [_vp, _fp, _i],
    "tsnet_set_sources": [_vp, _pp, _pp, _pp, _i, _vp],
    "tsnet_set_sources_shared": [_vp, _pp, _pp, _pp, _vp],
    "tsnet_forward_target": [_vp, _vp, _vp, _vp, _vp, _i, _vp],
    "tsnet_train_extras": [_vp, _pp, _vp, _i, _vp, _vp, _vp],
    "tsnet_stage_ptr": [_vp, C.c_char_p, _pp, C.POINTER(C.c_size_t)],
    "tsnet_forward_macs": ([_vp, _i], C.c_double),
    "tsnet_timing_enable": [_vp, _i],
    "tsnet_timing_read": [_vp, C.POINTER(C.c_double), C.POINTER(C.c_int64), _i],
    "tsnet_op_conv2d": _conv2d,
    "tsnet_op_conv2d_cat": [_vp, _vp] + [_i] * 6 + [_vp, _vp] + [_i] * 5 + [C.c_float, _i, _vp, _vp],
    "tsnet_op_head": [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _fp, _vp, _vp],
    "tsnet_op_instnorm_stats": [_vp, _i, _i, _i, _vp, _vp, _vp],
    "tsnet_op_norm_act": [_vp, _vp, _vp, _i, _vp, _i, _i, _i, _vp, _vp],
    "tsnet_op_upsample2x": [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp],
    "tsnet_op_flow": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp],
    "tsnet_op_flow_k": [_vp, _vp, _vp, _vp] + [_i] * 7 + [_vp, _i, _i, _fp, _vp],
    "tsnet_flow_plan": [_i] * 4,
    "tsnet_op_warp": [_vp, _vp, _i, _i, _i, _i, _vp, _vp],
    "tsnet_op_warp_k": [_vp, _vp] + [_i] * 5 + [_vp, _i, _fp, _vp],
    "tsnet_op_warp_k_shared": [_vp, _vp] + [_i] * 6 + [_vp, _vp],
    "tsnet_op_add_stats": [_vp, _vp] + [_i] * 5 + [_vp, _vp, _vp, _vp],
    "tsnet_op_finalize_stats": [_vp] + [_i] * 4 + [_vp, _vp, _vp],
    "tsnet_op_fuse_tail": [_vp] * 5 + [_i] * 5 + [_vp, _vp],
    "tsnet_op_pack_input": [_pp, _pp] + [_i] * 8 + [_fp, _vp, _vp, _vp],
    "tsnet_op_upsample2x_st": [_vp, _vp, _vp] + [_i] * 7 + [_vp, _vp],
    "tsnet_op_last_error": (None, C.c_char_p),
    "tsnet_frame_stats": [_vp, _i, _i, _i, C.c_float, _vp, _vp, _vp],
    "tsnet_demo_postprocess": [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _fp, _vp, _vp],
    "tsnet_fit_face_curves": [_vp, _i, _vp],
    "tsnet_raster_face": [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp],
    "tsnet_vl2ch": [_vp, _i, _i, _i, _vp, _vp],
    "tsnet_fit_pose_curves": [_vp, _i, _i, _vp],
    "tsnet_raster_pose": [_vp, _vp] + [_i] * 8 + [_vp, _vp],
    "tsnet_label_bbox": [_vp, _i, _i, _i, _vp, _vp],
    "tsnet_resize_pad": [_vp, _i, _i, _i, _vp, _vp] + [_i] * 7 + [_vp, _vp],
    "tsnet_resize_label": [_vp, _i, _i, _i, _i, _i, _vp, _i, _vp, _i, _vp, _vp],
    "tsnet_bench_conv": [_i] * 12 + [_fp, _vp],
    "tsnet_debug_counters": ([C.POINTER(C.c_int64), _i], None),
    "tsnet_linspace": ([_i, _fp], None),
    "tsnet_coord_table": ([_i, _i, _fp], None),
    "tsnet_bicubic_taps": [_i, _i],
    "tsnet_bicubic_table": [_i, _i, _vp, _vp, _vp],
    "tsnet_prepare_frames": _prepare + [_fp, _vp, _vp],
    "tsnet_face_adapt_stats": [_vp, _i, _vp],
    "tsnet_face_adapt_apply": [_vp, _vp, _i],
    "tsnet_smooth_keypoints": [_vp, _i, _i, _vp],
    "tsnet_bank_capacity": [_vp],
    "tsnet_bank_put": [_vp, _i, _i, _pp, _pp, _pp, _fp, _vp],
    "tsnet_forward_bank": [_vp, _ip, _i, _vp, _vp, _vp, _vp, _i, _vp],
    "tsnet_op_flow_k_slots": [_vp, _vp, _vp, _vp] + [_i] * 7 + [_vp, _i, _i, _fp, _ip, _i, _vp],
    "tsnet_op_warp_k_slots": [_vp, _vp] + [_i] * 5 + [_vp, _ip, _i, _vp],
    "tsnet_op_add_stats_slots": [_vp, _vp] + [_i] * 4 + [_vp, _vp, _vp, _ip, _i, _vp],
    "tsnet_op_fuse_tail_slots": [_vp] * 5 + [_i] * 4 + [_vp, _ip, _i, _vp],
    "tsnet_forward_u8": [_vp, _pp, _pp, _pp, _vp, _vp, _fp, _vp, _vp, _i, _vp],
    "tsnet_set_sources_u8": [_vp, _pp, _pp, _pp, _fp, _i, _i, _vp],
    "tsnet_forward_target_u8": [_vp, _vp, _vp, _vp, _vp, _i, _vp],
    "tsnet_bank_put_u8": [_vp, _i, _i, _pp, _pp, _pp, _fp, _fp, _vp],
    "tsnet_forward_bank_u8": [_vp, _ip, _i, _vp, _vp, _vp, _vp, _i, _vp],
    "tsnet_op_pack_input_u8": [_pp, _pp, _pp] + [_i] * 8 + [_fp, _fp, _vp, _vp, _vp, _vp],
    "tsnet_prepare_frames_u8": _prepare + [_vp, _vp],
    "tsnet_paste_frames": [_vp, _vp] + [_i] * 7 + [_vp, _vp, _vp, _i, _vp, _vp, _vp, _i] + [_vp] + [_i] * 6 + [_vp],
    "tsnet_prepare_frames_boxes": _prepare_boxes + [_fp, _vp, _vp],
    "tsnet_prepare_frames_boxes_u8": _prepare_boxes + [_vp, _vp],
    "tsnet_paste_frames_boxes": [_vp, _vp] + [_i] * 7 + [_vp, _vp, _vp, _i] + [_vp, _i, _i, _vp],
    "tsnet_face_labels_boxes": _face_labels,
    "tsnet_face_labels_boxes_u8": _face_labels,
    "tsnet_op_upconv2d": _conv2d,
    "tsnet_op_conv2d_epi": _conv2d[:-1] + [C.POINTER(TsnetConvEpi), _vp],
    "tsnet_op_patch_warp": [_pp, _fp, _vp] + [_i] * 6 + [_vp, _vp],
    "tsnet_op_train_tail": [_vp] * 4 + [_i] * 8 + [_fp] + [_vp] * 6,
    "tsnet_gaussian_box_params": [C.c_float, _i, _ip, C.POINTER(C.c_uint), C.POINTER(C.c_uint)],
    "tsnet_blur_mask": [_vp, _i, _i, _i, _vp, C.c_float, C.c_float, _i, _vp, _vp, _vp],
    "tsnet_yuv_coeffs": [_i, _i, _vp, _vp],
    "tsnet_rgb_to_yuv420": _yuv,
    "tsnet_yuv420_to_rgb": _yuv,
}
ABI_SYMBOLS = tuple(ABI)


def bind(lib: C.CDLL) -> C.CDLL:
    """Attach argtypes/restypes for every ABI entry point the library has."""
    for name, sig in ABI.items():
        if hasattr(lib, name):                     # newer entries are absent from an older build opened beside this one (tools/*.py --lib2)
            fn = getattr(lib, name)
            argtypes, fn.restype = sig if isinstance(sig, tuple) else (sig, C.c_int)
            if argtypes is not None:
                fn.argtypes = argtypes
    return lib


_cached = None


def load_tools() -> C.CDLL:
    """The tools flavour of the library (build.py --tools): product kernels + superseded generations + ablation variants.
    For tools/*.py on the GPU box only; the package itself never opens it."""
    from . import build as _b
    if not os.path.exists(_b.OUT_TOOLS):
        raise RuntimeError(f"{_b.OUT_TOOLS} is missing: run `python -m wacv23_tsnet_amd.build --tools`")
    return bind(C.CDLL(_b.OUT_TOOLS))


def load() -> C.CDLL:
    """Open the HIP library; raises (never falls back) if it is not built."""
    global _cached
    if _cached is not None:
        return _cached
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the HIP extension is not built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc). "
            "There is no CPU fallback for the TS-Net forward path.")
    try:
        _cached = bind(C.CDLL(LIB_PATH))
    except OSError as e:  # pragma: no cover - depends on the machine
        raise RuntimeError(f"failed to load {LIB_PATH}: {e}") from e
    if _cached.tsnet_abi_version() != 5:
        raise RuntimeError("libtsnet_hip.so ABI version mismatch; rebuild")
    return _cached
