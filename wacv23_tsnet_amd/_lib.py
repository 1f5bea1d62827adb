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

# every symbol include/tsnet_abi.h declares (tests/test_abi.py checks header <-> library <-> this list)
ABI_SYMBOLS = (
    "tsnet_abi_version", "tsnet_create", "tsnet_load_weights", "tsnet_finalize", "tsnet_destroy",
    "tsnet_last_error", "tsnet_num_params", "tsnet_param_info", "tsnet_packed_weights",
    "tsnet_forward", "tsnet_set_source_divisors", "tsnet_set_sources", "tsnet_set_sources_shared", "tsnet_forward_target", "tsnet_train_extras", "tsnet_stage_ptr",
    "tsnet_forward_macs", "tsnet_timing_enable", "tsnet_timing_read",
    "tsnet_op_conv2d", "tsnet_op_conv2d_cat", "tsnet_op_head", "tsnet_op_instnorm_stats", "tsnet_op_norm_act", "tsnet_op_upsample2x",
    "tsnet_op_flow", "tsnet_op_flow_k", "tsnet_flow_plan", "tsnet_op_warp", "tsnet_op_warp_k", "tsnet_op_warp_k_shared", "tsnet_op_add_stats", "tsnet_op_finalize_stats", "tsnet_op_fuse_tail", "tsnet_op_pack_input", "tsnet_op_upsample2x_st", "tsnet_op_last_error", "tsnet_frame_stats", "tsnet_demo_postprocess", "tsnet_fit_face_curves", "tsnet_raster_face", "tsnet_vl2ch", "tsnet_fit_pose_curves", "tsnet_raster_pose", "tsnet_label_bbox", "tsnet_resize_pad", "tsnet_resize_label", "tsnet_bench_conv", "tsnet_debug_counters", "tsnet_linspace", "tsnet_coord_table",
    "tsnet_bicubic_taps", "tsnet_bicubic_table", "tsnet_prepare_frames",
    "tsnet_face_adapt_stats", "tsnet_face_adapt_apply", "tsnet_smooth_keypoints",
    "tsnet_bank_capacity", "tsnet_bank_put", "tsnet_forward_bank",
    "tsnet_op_flow_k_slots", "tsnet_op_warp_k_slots", "tsnet_op_add_stats_slots", "tsnet_op_fuse_tail_slots",
    "tsnet_forward_u8", "tsnet_set_sources_u8", "tsnet_forward_target_u8", "tsnet_bank_put_u8", "tsnet_forward_bank_u8",
    "tsnet_op_pack_input_u8", "tsnet_prepare_frames_u8",
    "tsnet_paste_frames",
    "tsnet_prepare_frames_boxes", "tsnet_prepare_frames_boxes_u8", "tsnet_paste_frames_boxes",
    "tsnet_face_labels_boxes", "tsnet_face_labels_boxes_u8",
    "tsnet_op_upconv2d", "tsnet_op_conv2d_epi",
    "tsnet_op_patch_warp", "tsnet_op_train_tail",
    "tsnet_gaussian_box_params", "tsnet_blur_mask",
    "tsnet_yuv_coeffs", "tsnet_rgb_to_yuv420", "tsnet_yuv420_to_rgb",
)


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


def bind(lib: C.CDLL) -> C.CDLL:
    """Attach argtypes/restypes for every ABI entry point."""
    lib.tsnet_abi_version.restype = C.c_int
    lib.tsnet_create.argtypes = [C.POINTER(TsnetCfg), C.POINTER(_vp)]
    lib.tsnet_load_weights.argtypes = [_vp, C.c_char_p, _vp, C.POINTER(C.c_int64), C.c_int]
    lib.tsnet_finalize.argtypes = [_vp, _vp]
    lib.tsnet_destroy.argtypes = [_vp]
    lib.tsnet_destroy.restype = None
    lib.tsnet_last_error.argtypes = [_vp]
    lib.tsnet_last_error.restype = C.c_char_p
    lib.tsnet_num_params.argtypes = [_vp]
    lib.tsnet_param_info.argtypes = [_vp, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.POINTER(C.c_int)]
    lib.tsnet_packed_weights.argtypes = [_vp, C.POINTER(_vp), C.POINTER(C.c_size_t)]
    pp = C.POINTER(_vp)
    lib.tsnet_forward.argtypes = [_vp, pp, pp, pp, _vp, _vp, _vp, _vp, C.c_int, _vp]
    lib.tsnet_set_source_divisors.argtypes = [_vp, _fp, C.c_int]
    lib.tsnet_set_sources.argtypes = [_vp, pp, pp, pp, C.c_int, _vp]
    if hasattr(lib, "tsnet_set_sources_shared"):   # absent from an older build opened beside this one (tools/forward_ab.py --lib2)
        lib.tsnet_set_sources_shared.argtypes = [_vp, pp, pp, pp, _vp]
    lib.tsnet_forward_target.argtypes = [_vp, _vp, _vp, _vp, _vp, C.c_int, _vp]
    lib.tsnet_train_extras.argtypes = [_vp, pp, _vp, C.c_int, _vp, _vp, _vp]
    lib.tsnet_stage_ptr.argtypes = [_vp, C.c_char_p, C.POINTER(_vp), C.POINTER(C.c_size_t)]
    lib.tsnet_forward_macs.argtypes = [_vp, C.c_int]
    lib.tsnet_forward_macs.restype = C.c_double
    lib.tsnet_timing_enable.argtypes = [_vp, C.c_int]
    lib.tsnet_timing_read.argtypes = [_vp, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_int]
    lib.tsnet_op_conv2d.argtypes = [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int,
                                    C.c_int, C.c_int, _vp, _vp, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, _vp, _vp]
    lib.tsnet_op_conv2d_cat.argtypes = [_vp, _vp] + [C.c_int] * 6 + [_vp, _vp] + [C.c_int] * 5 + [C.c_float, C.c_int, _vp, _vp]
    lib.tsnet_op_head.argtypes = [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, C.c_int, _fp, _vp, _vp]
    lib.tsnet_op_instnorm_stats.argtypes = [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp]
    lib.tsnet_op_norm_act.argtypes = [_vp, _vp, _vp, C.c_int, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp]
    lib.tsnet_op_upsample2x.argtypes = [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp]
    lib.tsnet_resize_label.argtypes = [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_int, _vp, C.c_int, _vp, _vp]
    lib.tsnet_op_flow.argtypes = [_vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp]
    lib.tsnet_op_flow_k.argtypes = [_vp, _vp, _vp, _vp] + [C.c_int] * 7 + [_vp, C.c_int, C.c_int, _fp, _vp]
    lib.tsnet_flow_plan.argtypes = [C.c_int] * 4
    lib.tsnet_op_warp.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp]
    if hasattr(lib, "tsnet_op_warp_k"):          # absent from an older build opened beside this one (tools/forward_ab.py --lib2)
        lib.tsnet_op_warp_k.argtypes = [_vp, _vp] + [C.c_int] * 5 + [_vp, C.c_int, _fp, _vp]
    if hasattr(lib, "tsnet_op_fuse_tail"):       # absent from an older build opened beside this one (tools/forward_ab.py --lib2)
        lib.tsnet_op_warp_k_shared.argtypes = [_vp, _vp] + [C.c_int] * 6 + [_vp, _vp]
        lib.tsnet_op_add_stats.argtypes = [_vp, _vp] + [C.c_int] * 5 + [_vp, _vp, _vp, _vp]
        lib.tsnet_op_finalize_stats.argtypes = [_vp] + [C.c_int] * 4 + [_vp, _vp, _vp]
        lib.tsnet_op_fuse_tail.argtypes = [_vp] * 5 + [C.c_int] * 5 + [_vp, _vp]
        lib.tsnet_op_pack_input.argtypes = [pp, pp] + [C.c_int] * 8 + [_fp, _vp, _vp, _vp]
        lib.tsnet_op_upsample2x_st.argtypes = [_vp, _vp, _vp] + [C.c_int] * 7 + [_vp, _vp]
    lib.tsnet_op_last_error.restype = C.c_char_p
    lib.tsnet_frame_stats.argtypes = [_vp, C.c_int, C.c_int, C.c_int, C.c_float, _vp, _vp, _vp]
    lib.tsnet_demo_postprocess.argtypes = [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _fp, _vp, _vp]
    lib.tsnet_fit_face_curves.argtypes = [_vp, C.c_int, _vp]
    lib.tsnet_fit_pose_curves.argtypes = [_vp, C.c_int, C.c_int, _vp]
    lib.tsnet_raster_face.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp]
    lib.tsnet_vl2ch.argtypes = [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp]
    lib.tsnet_raster_pose.argtypes = [_vp, _vp] + [C.c_int] * 8 + [_vp, _vp]
    lib.tsnet_label_bbox.argtypes = [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp]
    lib.tsnet_resize_pad.argtypes = [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp] + [C.c_int] * 7 + [_vp, _vp]
    lib.tsnet_bench_conv.argtypes = [C.c_int] * 12 + [_fp, _vp]
    lib.tsnet_debug_counters.argtypes = [C.POINTER(C.c_int64), C.c_int]
    lib.tsnet_debug_counters.restype = None
    lib.tsnet_linspace.argtypes = [C.c_int, _fp]
    lib.tsnet_linspace.restype = None
    lib.tsnet_coord_table.argtypes = [C.c_int, C.c_int, _fp]
    lib.tsnet_coord_table.restype = None
    if hasattr(lib, "tsnet_prepare_frames"):     # absent from an older build opened beside this one (tools/forward_ab.py --lib2)
        lib.tsnet_bicubic_taps.argtypes = [C.c_int, C.c_int]
        lib.tsnet_bicubic_table.argtypes = [C.c_int, C.c_int, _vp, _vp, _vp]
        lib.tsnet_prepare_frames.argtypes = [_vp] + [C.c_int] * 7 + [_vp, _vp, _vp, C.c_int, _vp, _vp, _vp, C.c_int] + [C.c_int] * 6 + [_fp, _vp, _vp]
    if hasattr(lib, "tsnet_face_adapt_stats"):   # absent from an older build opened beside this one (tools/forward_ab.py --lib2)
        lib.tsnet_face_adapt_stats.argtypes = [_vp, C.c_int, _vp]
        lib.tsnet_face_adapt_apply.argtypes = [_vp, _vp, C.c_int]
        lib.tsnet_smooth_keypoints.argtypes = [_vp, C.c_int, C.c_int, _vp]
    if hasattr(lib, "tsnet_forward_bank"):       # absent from an older build opened beside this one (tools/forward_ab.py --lib2)
        _ip = C.POINTER(C.c_int)
        lib.tsnet_bank_capacity.argtypes = [_vp]
        lib.tsnet_bank_put.argtypes = [_vp, C.c_int, C.c_int, pp, pp, pp, _fp, _vp]
        lib.tsnet_forward_bank.argtypes = [_vp, _ip, C.c_int, _vp, _vp, _vp, _vp, C.c_int, _vp]
        lib.tsnet_op_flow_k_slots.argtypes = [_vp, _vp, _vp, _vp] + [C.c_int] * 7 + [_vp, C.c_int, C.c_int, _fp, _ip, C.c_int, _vp]
        lib.tsnet_op_warp_k_slots.argtypes = [_vp, _vp] + [C.c_int] * 5 + [_vp, _ip, C.c_int, _vp]
        lib.tsnet_op_add_stats_slots.argtypes = [_vp, _vp] + [C.c_int] * 4 + [_vp, _vp, _vp, _ip, C.c_int, _vp]
        lib.tsnet_op_fuse_tail_slots.argtypes = [_vp] * 5 + [C.c_int] * 4 + [_vp, _ip, C.c_int, _vp]
    if hasattr(lib, "tsnet_forward_u8"):         # absent from an older build opened beside this one (tools/clip_bench.py --lib2)
        _ip = C.POINTER(C.c_int)
        lib.tsnet_forward_u8.argtypes = [_vp, pp, pp, pp, _vp, _vp, _fp, _vp, _vp, C.c_int, _vp]
        lib.tsnet_set_sources_u8.argtypes = [_vp, pp, pp, pp, _fp, C.c_int, C.c_int, _vp]
        lib.tsnet_forward_target_u8.argtypes = [_vp, _vp, _vp, _vp, _vp, C.c_int, _vp]
        lib.tsnet_bank_put_u8.argtypes = [_vp, C.c_int, C.c_int, pp, pp, pp, _fp, _fp, _vp]
        lib.tsnet_forward_bank_u8.argtypes = [_vp, _ip, C.c_int, _vp, _vp, _vp, _vp, C.c_int, _vp]
        lib.tsnet_op_pack_input_u8.argtypes = [pp, pp, pp] + [C.c_int] * 8 + [_fp, _fp, _vp, _vp, _vp, _vp]
        lib.tsnet_prepare_frames_u8.argtypes = [_vp] + [C.c_int] * 7 + [_vp, _vp, _vp, C.c_int, _vp, _vp, _vp, C.c_int] + [C.c_int] * 6 + [_vp, _vp]
    if hasattr(lib, "tsnet_paste_frames"):       # absent from an older build opened beside this one (tools/forward_ab.py --lib2)
        lib.tsnet_paste_frames.argtypes = [_vp, _vp] + [C.c_int] * 7 + [_vp, _vp, _vp, C.c_int, _vp, _vp, _vp, C.c_int] + [_vp] + [C.c_int] * 6 + [_vp]
    if hasattr(lib, "tsnet_paste_frames_boxes"): # absent from an older build opened beside this one (tools/forward_ab.py --lib2)
        lib.tsnet_prepare_frames_boxes.argtypes = [_vp] + [C.c_int] * 3 + [_vp, _vp, _vp, C.c_int] + [C.c_int] * 6 + [_fp, _vp, _vp]
        lib.tsnet_prepare_frames_boxes_u8.argtypes = [_vp] + [C.c_int] * 3 + [_vp, _vp, _vp, C.c_int] + [C.c_int] * 6 + [_vp, _vp]
        lib.tsnet_paste_frames_boxes.argtypes = [_vp, _vp] + [C.c_int] * 7 + [_vp, _vp, _vp, C.c_int] + [_vp, C.c_int, C.c_int, _vp]
    if hasattr(lib, "tsnet_face_labels_boxes"):  # absent from an older build opened beside this one (tools/track_labels_bench.py --lib2)
        for fn in (lib.tsnet_face_labels_boxes, lib.tsnet_face_labels_boxes_u8):
            fn.argtypes = [_vp, _vp, C.c_int, _vp, _vp, _vp, C.c_int, C.c_int, _vp, C.c_longlong, C.c_int, C.c_int, _vp, _vp, _vp]
    if hasattr(lib, "tsnet_op_upconv2d"):        # absent from an older build opened beside this one (tools/forward_ab.py --lib2)
        lib.tsnet_op_upconv2d.argtypes = lib.tsnet_op_conv2d.argtypes
    if hasattr(lib, "tsnet_op_conv2d_epi"):      # absent from an older build opened beside this one (tools/forward_ab.py --lib2)
        lib.tsnet_op_conv2d_epi.argtypes = lib.tsnet_op_conv2d.argtypes[:-1] + [C.POINTER(TsnetConvEpi), _vp]
    if hasattr(lib, "tsnet_op_train_tail"):      # absent from an older build opened beside this one (tools/forward_ab.py --lib2)
        lib.tsnet_op_patch_warp.argtypes = [pp, _fp, _vp] + [C.c_int] * 6 + [_vp, _vp]
        lib.tsnet_op_train_tail.argtypes = [_vp] * 4 + [C.c_int] * 8 + [_fp] + [_vp] * 6
    if hasattr(lib, "tsnet_blur_mask"):          # absent from an older build opened beside this one (tools/forward_ab.py --lib2)
        lib.tsnet_gaussian_box_params.argtypes = [C.c_float, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_uint), C.POINTER(C.c_uint)]
        lib.tsnet_blur_mask.argtypes = [_vp, C.c_int, C.c_int, C.c_int, _vp, C.c_float, C.c_float, C.c_int, _vp, _vp, _vp]
    if hasattr(lib, "tsnet_rgb_to_yuv420"):      # absent from an older build opened beside this one (tools/forward_ab.py --lib2)
        lib.tsnet_yuv_coeffs.argtypes = [C.c_int, C.c_int, _vp, _vp]
        lib.tsnet_rgb_to_yuv420.argtypes = lib.tsnet_yuv420_to_rgb.argtypes = [_vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int, _vp, _vp]
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
