"""dbde_video_cpp_amd -- Python doorway to the MI355X DBDE codec (libdbde_hip.so).

This is plumbing, not the product: every function is a ctypes call into the C-ABI declared
in include/dbde_hip.h.  PyTorch is used only for what it is good at here -- device memory
(`tensor.data_ptr()`), streams and `torch.distributed`.  Method names follow the reference's
dbde_util.h (pack_frame, unpack_frame, pack_8x8, ...), so tests read like the reference's.

There is no CPU fallback.  If the in-tree library is missing, importing raises; if no
gfx950 device is usable, `Codec()` raises.

The directory is called `dbde-video-cpp_amd`; import it as `dbde_video_cpp_amd` (the
repository root carries a one-file loader of that name).
"""
import ctypes as C
import os
import subprocess
import weakref

import numpy as np

try:  # torch first: its bundled libamdhip64.so.7 must be the one HIP runtime in the process
    import torch
except Exception:  # pragma: no cover - host-only use of the header helpers
    torch = None

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG_DIR)
LIB_PATH = os.path.join(PKG_DIR, "libdbde_hip.so")
SHIM_PATH = os.path.join(PKG_DIR, "libdbde_util_hip.so")

OK, ERR_ARG, ERR_HIP, ERR_CAPACITY, ERR_DEVICE = 0, -1, -2, -3, -4

MODES = {"noise8": 0, "mixed": 1, "flat": 2, "smooth": 3}

# every symbol include/dbde_hip.h declares (tests/test_capi_symbols.py checks the export list)
C_ABI_SYMBOLS = [
    "dbde_hip_create", "dbde_hip_destroy", "dbde_hip_sync", "dbde_hip_last_error", "dbde_hip_device_arch",
    "dbde_hip_max_frame_bytes", "dbde_hip_image_bytes",
    "dbde_hip_encode_frames", "dbde_hip_decode_frames", "dbde_hip_index_stream", "dbde_hip_index_stream_async",
    "dbde_hip_scan_ahead", "dbde_hip_scan_join", "dbde_hip_synth_frames",
    "dbde_hip_pack_8x8", "dbde_hip_pack_8x8_partial", "dbde_hip_pack_image", "dbde_hip_pack_frame",
    "dbde_hip_unpack_8x8", "dbde_hip_unpack_8x8_partial", "dbde_hip_unpack_image", "dbde_hip_unpack_frame",
    "dbde_hip_pack_frame_header", "dbde_hip_pack_video_header",
    "dbde_hip_unpack_frame_header", "dbde_hip_unpack_video_header",
    "dbde_hip_timing_enable", "dbde_hip_timing_read", "dbde_hip_encode_plan", "dbde_hip_decode_plan",
    "dbde_hip_stream_handle", "dbde_hip_device_index",
    "dbde16_hip_max_frame_bytes", "dbde16_hip_encode_frames", "dbde16_hip_decode_frames",
    "dbde_hip_writer_open", "dbde_hip_writer_put", "dbde_hip_writer_error", "dbde_hip_writer_close",
    "dbde_hip_reader_open", "dbde_hip_reader_next", "dbde_hip_reader_close",
    "dbde_hip_gather_unique_id", "dbde_hip_gather_create", "dbde_hip_gather_attach", "dbde_hip_gather_destroy",
    "dbde_hip_gather_error", "dbde_hip_gather_set_max_message", "dbde_hip_gather_begin", "dbde_hip_gather_post",
    "dbde_hip_gather_join", "dbde_hip_gather_sync", "dbde_hip_gather_rccl_version", "dbde_hip_gather_plan",
    "dbde_hip_gather_set_window", "dbde_hip_gather_check",
    "dbde_hip_scatter_create", "dbde_hip_scatter_attach", "dbde_hip_scatter_destroy", "dbde_hip_scatter_error",
    "dbde_hip_scatter_set_max_message", "dbde_hip_scatter_set_capacity", "dbde_hip_scatter_begin", "dbde_hip_scatter_post",
    "dbde_hip_scatter_join", "dbde_hip_scatter_sync", "dbde_hip_scatter_blocks", "dbde_hip_scatter_check",
    "dbde_hip_scatter_plan", "dbde_hip_create_on_own_stream", "dbde_hip_set_host_staging",
    "dbde_hip_decode_roi", "dbde_hip_unpack_image_roi", "dbde_hip_roi_plan",
    "dbde16_hip_decode_roi", "dbde16_hip_roi_plan",
    "dbde_hip_project", "dbde_hip_project_plan", "dbde16_hip_project", "dbde16_hip_project_plan",
    "dbde_hip_trace_map_summary", "dbde_hip_trace_map_create", "dbde_hip_trace_map_destroy", "dbde_hip_trace_map_info",
    "dbde_hip_trace_map_pixels", "dbde_hip_traces", "dbde16_hip_traces", "dbde_hip_trace_plan", "dbde16_hip_trace_plan",
    "dbde_hip_histogram", "dbde16_hip_histogram", "dbde_hip_histogram_plan", "dbde16_hip_histogram_plan",
    "dbde_hip_decode_binned", "dbde16_hip_decode_binned", "dbde_hip_binned_plan", "dbde16_hip_binned_plan",
    "dbde_hip_decode_scaled", "dbde16_hip_decode_scaled", "dbde_hip_scaled_plan", "dbde16_hip_scaled_plan",
    "dbde_hip_decode_mask", "dbde16_hip_decode_mask", "dbde_hip_mask_plan", "dbde16_hip_mask_plan",
    "dbde_hip_decode_patches", "dbde16_hip_decode_patches", "dbde_hip_patches_plan", "dbde16_hip_patches_plan",
    "dbde_hip_patch_moments", "dbde16_hip_patch_moments", "dbde_hip_patch_moments_plan", "dbde16_hip_patch_moments_plan",
    "dbde_hip_match_patches", "dbde16_hip_match_patches", "dbde_hip_match_plan", "dbde16_hip_match_plan",
    "dbde_hip_crop_frames", "dbde16_hip_crop_frames", "dbde_hip_crop_plan", "dbde16_hip_crop_plan",
    "dbde_hip_encode_window", "dbde16_hip_encode_window", "dbde_hip_window_encode_plan", "dbde16_hip_window_encode_plan",
    "dbde_hip_writer_put_window",
    "dbde_hip_project_groups", "dbde16_hip_project_groups", "dbde_hip_project_groups_plan",
    "dbde16_hip_project_groups_plan",
    "dbde_hip_project_weighted", "dbde16_hip_project_weighted", "dbde_hip_project_weighted_plan",
    "dbde16_hip_project_weighted_plan",
    "dbde_hip_project_counts", "dbde16_hip_project_counts", "dbde_hip_project_counts_plan",
    "dbde16_hip_project_counts_plan",
    "dbde_hip_project_pairs", "dbde16_hip_project_pairs", "dbde_hip_project_pairs_plan", "dbde16_hip_project_pairs_plan",
    "dbde_hip_project_lag", "dbde16_hip_project_lag", "dbde_hip_project_lag_plan", "dbde16_hip_project_lag_plan",
    "dbde_hip_project_registered", "dbde16_hip_project_registered", "dbde_hip_project_registered_plan",
    "dbde16_hip_project_registered_plan",
]


def build(verbose=False):
    """Compile the HIP library and the dbde_util.h shim in-tree (hipcc --offload-arch=gfx950)."""
    r = subprocess.run(["make", "-C", os.path.join(PKG_DIR, "csrc")], capture_output=True, text=True)
    if verbose or r.returncode:
        print(r.stdout[-4000:], r.stderr[-4000:])
    if r.returncode:
        raise RuntimeError("building libdbde_hip.so failed")


class FrameHeader(C.Structure):
    _fields_ = [("u64s", C.c_uint32), ("index", C.c_uint64), ("elapsed_ns", C.c_uint64)]


class VideoHeader(C.Structure):
    _fields_ = [("u64s", C.c_uint32), ("height", C.c_uint64), ("width", C.c_uint64), ("frame_hz", C.c_double)]


class FrameResult(C.Structure):
    _fields_ = [("header", FrameHeader), ("consumed", C.c_uint64)]


class ScatterBlock(C.Structure):
    _fields_ = [("first_frame", C.c_uint64), ("n_frames", C.c_uint64), ("byte_start", C.c_uint64), ("byte_count", C.c_uint64)]


class ScatterOp(C.Structure):
    _fields_ = [("peer", C.c_int32), ("kind", C.c_int32), ("source_offset", C.c_uint64), ("dest_offset", C.c_uint64),
                ("bytes", C.c_uint64)]


SCATTER_SEND_BYTES, SCATTER_RECV_BYTES, SCATTER_SEND_OFFSETS, SCATTER_RECV_OFFSETS, SCATTER_OWN = 1, 2, 3, 4, 5
SCATTER_LOOPBACK = 1


class GatherOp(C.Structure):
    _fields_ = [("peer", C.c_int32), ("kind", C.c_int32), ("segment_offset", C.c_uint64),
                ("window_offset", C.c_uint64), ("bytes", C.c_uint64)]


GATHER_SEND, GATHER_RECV, GATHER_OWN = 1, 2, 3
GATHER_LOOPBACK = 1
GATHER_ID_BYTES = 128


u8p = C.POINTER(C.c_uint8)
_lib = None


def lib():
    """The loaded C-ABI library; raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(there is no CPU fallback)")
    L = C.CDLL(LIB_PATH)
    vp, i, u64, sz = C.c_void_p, C.c_int, C.c_uint64, C.c_size_t
    L.dbde_hip_create.restype = i
    L.dbde_hip_create.argtypes = [i, vp, C.POINTER(vp)]
    L.dbde_hip_destroy.restype = None
    L.dbde_hip_destroy.argtypes = [vp]
    L.dbde_hip_sync.restype = i
    L.dbde_hip_sync.argtypes = [vp]
    L.dbde_hip_last_error.restype = C.c_char_p
    L.dbde_hip_last_error.argtypes = [vp]
    L.dbde_hip_device_arch.restype = C.c_char_p
    L.dbde_hip_device_arch.argtypes = [vp]
    L.dbde_hip_max_frame_bytes.restype = sz
    L.dbde_hip_max_frame_bytes.argtypes = [i, i]
    L.dbde_hip_image_bytes.restype = sz
    L.dbde_hip_image_bytes.argtypes = [i, i, u64]
    L.dbde_hip_encode_frames.restype = i
    L.dbde_hip_encode_frames.argtypes = [vp, vp, i, i, i, u64, vp, vp, vp, sz, u64, vp, vp]
    L.dbde_hip_decode_frames.restype = i
    L.dbde_hip_decode_frames.argtypes = [vp, vp, sz, vp, i, i, i, vp, vp]
    L.dbde_hip_index_stream.restype = i
    L.dbde_hip_index_stream.argtypes = [vp, vp, sz, i, i, i, vp, C.POINTER(i)]
    L.dbde_hip_index_stream_async.restype = i
    L.dbde_hip_index_stream_async.argtypes = [vp, vp, sz, i, i, i, vp, vp]
    L.dbde_hip_scan_ahead.restype = i
    L.dbde_hip_scan_ahead.argtypes = [vp, vp, sz, i, i, i, vp, vp, vp]
    L.dbde_hip_scan_join.restype = i
    L.dbde_hip_scan_join.argtypes = [vp]
    L.dbde_hip_synth_frames.restype = i
    L.dbde_hip_synth_frames.argtypes = [vp, i, u64, u64, i, i, i, vp]
    L.dbde_hip_pack_8x8.restype = C.c_uint32
    L.dbde_hip_pack_8x8.argtypes = [vp, vp, i, vp]
    L.dbde_hip_pack_8x8_partial.restype = C.c_uint32
    L.dbde_hip_pack_8x8_partial.argtypes = [vp, vp, i, i, i, vp]
    L.dbde_hip_pack_image.restype = sz
    L.dbde_hip_pack_image.argtypes = [vp, vp, i, i, vp]
    L.dbde_hip_pack_frame.restype = sz
    L.dbde_hip_pack_frame.argtypes = [vp, u64, vp, i, i, vp]
    L.dbde_hip_unpack_8x8.restype = None
    L.dbde_hip_unpack_8x8.argtypes = [vp, C.c_uint8, C.c_uint8, vp, sz, vp]
    L.dbde_hip_unpack_8x8_partial.restype = None
    L.dbde_hip_unpack_8x8_partial.argtypes = [vp, C.c_uint8, C.c_uint8, vp, sz, i, i, vp]
    L.dbde_hip_unpack_image.restype = sz
    L.dbde_hip_unpack_image.argtypes = [vp, vp, i, i, vp]
    L.dbde_hip_unpack_frame.restype = FrameHeader
    L.dbde_hip_unpack_image_roi.argtypes = [vp, vp, i, i, i, i, i, i, vp]
    L.dbde_hip_unpack_image_roi.restype = sz
    L.dbde_hip_decode_roi.argtypes = [vp, vp, sz, vp, i, i, i, i, i, i, i, vp, vp, vp]
    L.dbde_hip_decode_roi.restype = i
    L.dbde_hip_roi_plan.argtypes = [i, i, i, i, i, i, i, C.POINTER(RoiPlan)]
    L.dbde_hip_roi_plan.restype = i
    L.dbde16_hip_decode_roi.argtypes = [vp, vp, sz, vp, i, i, i, i, i, i, i, vp, vp, vp]
    L.dbde16_hip_decode_roi.restype = i
    L.dbde16_hip_roi_plan.argtypes = [i, i, i, i, i, i, i, C.POINTER(RoiPlan)]
    L.dbde16_hip_roi_plan.restype = i
    L.dbde_hip_project.argtypes = [vp, vp, sz, vp, i, i, i, i, i, i, i, i, vp, vp, vp, vp, vp, vp]
    L.dbde_hip_project.restype = i
    L.dbde_hip_project_plan.argtypes = [i, i, i, i, i, i, i, C.c_uint, i, C.POINTER(ProjectPlan)]
    L.dbde_hip_project_plan.restype = i
    L.dbde16_hip_project.argtypes = [vp, vp, sz, vp, i, i, i, i, i, i, i, i, vp, vp, vp, vp, vp, vp]
    L.dbde16_hip_project.restype = i
    L.dbde16_hip_project_plan.argtypes = [i, i, i, i, i, i, i, C.c_uint, i, C.POINTER(ProjectPlan)]
    L.dbde16_hip_project_plan.restype = i
    for fn in ("dbde_hip_project_groups", "dbde16_hip_project_groups"):
        getattr(L, fn).argtypes = [vp, vp, sz, vp, i, i, i, i, i, i, i, i, vp, i, i, i, vp, vp, vp, vp, vp, vp]
        getattr(L, fn).restype = i
    for fn in ("dbde_hip_project_groups_plan", "dbde16_hip_project_groups_plan"):
        getattr(L, fn).argtypes = [i, i, i, i, i, i, i, i, i, i, i, i, u64, u64, u64, u64, u64, i,
                                   C.POINTER(GroupProjectPlan)]
        getattr(L, fn).restype = i
    for fn in ("dbde_hip_project_weighted", "dbde16_hip_project_weighted"):
        getattr(L, fn).argtypes = [vp, vp, sz, vp, i, i, i, i, i, i, i, vp, i, sz, i, i, vp, vp, vp]
        getattr(L, fn).restype = i
    for fn in ("dbde_hip_project_weighted_plan", "dbde16_hip_project_weighted_plan"):
        getattr(L, fn).argtypes = [i, i, i, i, i, i, i, i, u64, i, u64, u64, u64, i, C.POINTER(WeightedProjectPlan)]
        getattr(L, fn).restype = i
    for fn in ("dbde_hip_project_counts", "dbde16_hip_project_counts"):
        getattr(L, fn).argtypes = [vp, vp, sz, vp, i, i, i, i, i, i, i, vp, i, sz, i, i, vp, vp, vp]
        getattr(L, fn).restype = i
    for fn in ("dbde_hip_project_counts_plan", "dbde16_hip_project_counts_plan"):
        getattr(L, fn).argtypes = [i, i, i, i, i, i, i, i, u64, i, u64, u64, u64, i, C.POINTER(CountProjectPlan)]
        getattr(L, fn).restype = i
    for fn in ("dbde_hip_project_pairs", "dbde16_hip_project_pairs"):
        getattr(L, fn).argtypes = [vp, vp, sz, vp, i, i, i, i, i, i, i, i, i, vp, vp, vp]
        getattr(L, fn).restype = i
    for fn in ("dbde_hip_project_pairs_plan", "dbde16_hip_project_pairs_plan"):
        getattr(L, fn).argtypes = [i, i, i, i, i, i, i, i, u64, u64, i, C.POINTER(PairProjectPlan)]
        getattr(L, fn).restype = i
    for fn in ("dbde_hip_project_lag", "dbde16_hip_project_lag"):
        getattr(L, fn).argtypes = [vp, vp, sz, vp, i, i, i, i, i, i, i, i, i, i, vp, vp, vp, vp, vp, vp, vp, vp]
        getattr(L, fn).restype = i
    for fn in ("dbde_hip_project_lag_plan", "dbde16_hip_project_lag_plan"):
        getattr(L, fn).argtypes = [i, i, i, i, i, i, i, i, i, C.c_uint, u64, u64, u64, u64, i, C.POINTER(LagProjectPlan)]
        getattr(L, fn).restype = i
    for fn in ("dbde_hip_project_registered", "dbde16_hip_project_registered"):
        getattr(L, fn).argtypes = [vp, vp, sz, vp, i, i, i, i, i, vp, i, vp, vp, vp, vp, vp, vp, vp]
        getattr(L, fn).restype = i
    for fn in ("dbde_hip_project_registered_plan", "dbde16_hip_project_registered_plan"):
        getattr(L, fn).argtypes = [i, i, i, i, i, C.c_uint, i, C.POINTER(RegisteredProjectPlan)]
        getattr(L, fn).restype = i
    L.dbde_hip_trace_map_summary.argtypes =[vp, i, i, i, C.POINTER(TraceMapInfo), vp]
    L.dbde_hip_trace_map_summary.restype = i
    L.dbde_hip_trace_map_create.argtypes = [vp, vp, i, i, i, C.POINTER(vp)]
    L.dbde_hip_trace_map_create.restype = i
    L.dbde_hip_trace_map_destroy.argtypes = [vp]
    L.dbde_hip_trace_map_destroy.restype = None
    L.dbde_hip_trace_map_info.argtypes = [vp, C.POINTER(TraceMapInfo)]
    L.dbde_hip_trace_map_info.restype = i
    L.dbde_hip_trace_map_pixels.argtypes = [vp]
    L.dbde_hip_trace_map_pixels.restype = vp
    for fn in ("dbde_hip_traces", "dbde16_hip_traces"):
        getattr(L, fn).argtypes = [vp, vp, sz, vp, i, i, i, vp, vp, vp, vp, vp, vp]
        getattr(L, fn).restype = i
    for fn in ("dbde_hip_trace_plan", "dbde16_hip_trace_plan"):
        getattr(L, fn).argtypes = [i, i, i, C.POINTER(TraceMapInfo), C.c_uint, i, C.POINTER(TracePlan)]
        getattr(L, fn).restype = i
    for fn in ("dbde_hip_histogram", "dbde16_hip_histogram"):
        getattr(L, fn).argtypes = [vp, vp, sz, vp, i, i, i, i, i, i, i, i, i, i, vp, vp, vp, vp]
        getattr(L, fn).restype = i
    for fn in ("dbde_hip_histogram_plan", "dbde16_hip_histogram_plan"):
        getattr(L, fn).argtypes = [i, i, i, i, i, i, i, i, i, C.c_uint, i, C.POINTER(HistogramPlan)]
        getattr(L, fn).restype = i
    for fn in ("dbde_hip_decode_binned", "dbde16_hip_decode_binned"):
        getattr(L, fn).argtypes = [vp, vp, sz, vp, i, i, i, i, i, i, i, i, vp, vp, vp, vp]
        getattr(L, fn).restype = i
    for fn in ("dbde_hip_binned_plan", "dbde16_hip_binned_plan"):
        getattr(L, fn).argtypes = [i, i, i, i, i, i, i, i, C.c_uint, C.POINTER(BinnedPlan)]
        getattr(L, fn).restype = i
    for fn in ("dbde_hip_decode_scaled", "dbde16_hip_decode_scaled"):
        getattr(L, fn).argtypes = [vp, vp, sz, vp, i, i, i, i, i, i, i, vp, i, vp, C.c_float, vp, C.c_float, vp, vp]
        getattr(L, fn).restype = i
    for fn in ("dbde_hip_scaled_plan", "dbde16_hip_scaled_plan"):
        getattr(L, fn).argtypes = [i, i, i, i, i, i, i, i, C.POINTER(ScaledPlan)]
        getattr(L, fn).restype = i
    for fn in ("dbde_hip_decode_mask", "dbde16_hip_decode_mask"):
        getattr(L, fn).argtypes = [vp, vp, sz, vp, i, i, i, i, i, i, i, vp, i, vp, C.c_uint32, vp, C.c_uint32, vp, vp, vp, vp]
        getattr(L, fn).restype = i
    for fn in ("dbde_hip_mask_plan", "dbde16_hip_mask_plan"):
        getattr(L, fn).argtypes = [i, i, i, i, i, i, i, C.POINTER(MaskPlan)]
        getattr(L, fn).restype = i
    for fn in ("dbde_hip_decode_patches", "dbde16_hip_decode_patches"):
        getattr(L, fn).argtypes = [vp, vp, sz, vp, i, i, i, i, i, i, vp, vp, i, C.c_uint32, vp, vp, vp]
        getattr(L, fn).restype = i
    for fn in ("dbde_hip_patches_plan", "dbde16_hip_patches_plan"):
        getattr(L, fn).argtypes = [i, i, i, i, i, i, i, C.POINTER(PatchPlan)]
        getattr(L, fn).restype = i
    for fn in ("dbde_hip_patch_moments", "dbde16_hip_patch_moments"):
        getattr(L, fn).argtypes = [vp, vp, sz, vp, i, i, i, i, i, i, vp, vp, i, C.c_uint32, C.c_uint32, i, vp, vp, vp, vp]
        getattr(L, fn).restype = i
    for fn in ("dbde_hip_patch_moments_plan", "dbde16_hip_patch_moments_plan"):
        getattr(L, fn).argtypes = [i, i, i, i, i, i, i, C.POINTER(PatchMomentsPlan)]
        getattr(L, fn).restype = i
    for fn in ("dbde_hip_match_patches", "dbde16_hip_match_patches"):
        getattr(L, fn).argtypes = [vp, vp, sz, vp, i, i, i, i, i, i, i, vp, vp, i, C.c_uint32, vp, i, C.c_uint, vp, vp, vp,
                                   vp, vp]
        getattr(L, fn).restype = i
    for fn in ("dbde_hip_match_plan", "dbde16_hip_match_plan"):
        getattr(L, fn).argtypes = [i, i, i, i, i, i, i, i, i, C.c_uint32, C.c_uint, C.POINTER(MatchPlan)]
        getattr(L, fn).restype = i
    for fn in ("dbde_hip_crop_frames", "dbde16_hip_crop_frames"):
        getattr(L, fn).argtypes = [vp, vp, sz, vp, i, i, i, i, i, i, i, vp, vp, sz, u64, vp, vp, vp, vp]
        getattr(L, fn).restype = i
    for fn in ("dbde_hip_crop_plan", "dbde16_hip_crop_plan"):
        getattr(L, fn).argtypes = [i, i, i, i, i, i, i, u64, C.POINTER(CropPlan)]
        getattr(L, fn).restype = i
    L.dbde_hip_encode_window.argtypes = [vp, vp, sz, i, i, u64, u64, i, i, i, i, i, vp, u64, vp, vp, vp, sz, u64, vp, vp]
    L.dbde_hip_encode_window.restype = i
    L.dbde16_hip_encode_window.argtypes = [vp, vp, sz, i, i, u64, u64, i, i, i, i, i, vp, u64, vp, sz, u64, vp, vp]
    L.dbde16_hip_encode_window.restype = i
    for fn in ("dbde_hip_window_encode_plan", "dbde16_hip_window_encode_plan"):
        getattr(L, fn).argtypes = [u64, sz, i, i, u64, u64, i, i, i, i, i, i, sz, u64, i, C.POINTER(WindowEncodePlan)]
        getattr(L, fn).restype = i
    L.dbde_hip_writer_put_window.argtypes = [vp, vp, sz, i, i, u64, u64, i, i, i, vp, u64, vp, vp]
    L.dbde_hip_writer_put_window.restype = i
    L.dbde_hip_unpack_frame.argtypes = [vp, C.POINTER(vp), i, i, vp]
    L.dbde_hip_pack_frame_header.restype = sz
    L.dbde_hip_pack_frame_header.argtypes = [C.POINTER(FrameHeader), vp]
    L.dbde_hip_pack_video_header.restype = sz
    L.dbde_hip_pack_video_header.argtypes = [C.POINTER(VideoHeader), vp]
    L.dbde_hip_unpack_frame_header.restype = FrameHeader
    L.dbde_hip_unpack_frame_header.argtypes = [C.POINTER(vp)]
    L.dbde_hip_unpack_video_header.restype = VideoHeader
    L.dbde_hip_unpack_video_header.argtypes = [C.POINTER(vp)]
    L.dbde_hip_timing_enable.restype = i
    L.dbde_hip_timing_enable.argtypes = [vp, i]
    L.dbde_hip_timing_read.restype = i
    L.dbde_hip_timing_read.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(u64), i]
    L.dbde_hip_stream_handle.restype = vp
    L.dbde_hip_stream_handle.argtypes = [vp]
    L.dbde_hip_device_index.restype = i
    L.dbde_hip_device_index.argtypes = [vp]
    L.dbde16_hip_max_frame_bytes.restype = sz
    L.dbde16_hip_max_frame_bytes.argtypes = [i, i]
    L.dbde16_hip_encode_frames.restype = i
    L.dbde16_hip_encode_frames.argtypes = [vp, vp, i, i, i, u64, vp, sz, u64, vp, vp]
    L.dbde16_hip_decode_frames.restype = i
    L.dbde16_hip_decode_frames.argtypes = [vp, vp, sz, vp, i, i, i, vp, vp]
    L.dbde_hip_writer_open.restype = i
    L.dbde_hip_writer_open.argtypes = [vp, C.c_char_p, i, i, C.c_double, i, C.POINTER(vp)]
    L.dbde_hip_writer_put.restype = i
    L.dbde_hip_writer_put.argtypes = [vp, vp, i, u64, vp, vp]
    L.dbde_hip_writer_error.restype = C.c_char_p
    L.dbde_hip_writer_error.argtypes = [vp]
    L.dbde_hip_writer_close.restype = i
    L.dbde_hip_writer_close.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
    L.dbde_hip_reader_open.restype = i
    L.dbde_hip_reader_open.argtypes = [vp, C.c_char_p, i, C.POINTER(VideoHeader), C.POINTER(vp)]
    L.dbde_hip_reader_next.restype = i
    L.dbde_hip_reader_next.argtypes = [vp, vp, i, C.POINTER(FrameHeader), C.POINTER(i)]
    L.dbde_hip_reader_close.restype = None
    L.dbde_hip_reader_close.argtypes = [vp]
    L.dbde_hip_gather_unique_id.restype = i
    L.dbde_hip_gather_unique_id.argtypes = [vp]
    L.dbde_hip_gather_create.restype = i
    L.dbde_hip_gather_create.argtypes = [vp, vp, i, i, i, C.POINTER(vp)]
    L.dbde_hip_gather_attach.restype = i
    L.dbde_hip_gather_attach.argtypes = [vp, vp, i, i, i, C.POINTER(vp)]
    L.dbde_hip_gather_destroy.restype = None
    L.dbde_hip_gather_destroy.argtypes = [vp]
    L.dbde_hip_gather_error.restype = C.c_char_p
    L.dbde_hip_gather_error.argtypes = [vp]
    L.dbde_hip_gather_set_max_message.restype = i
    L.dbde_hip_gather_set_max_message.argtypes = [vp, u64]
    L.dbde_hip_gather_begin.restype = i
    L.dbde_hip_gather_begin.argtypes = [vp, i, vp, vp]
    L.dbde_hip_gather_post.restype = i
    L.dbde_hip_gather_post.argtypes = [vp, i, vp, vp, sz, C.POINTER(u64), C.c_uint32]
    L.dbde_hip_gather_join.restype = i
    L.dbde_hip_gather_join.argtypes = [vp, i]
    L.dbde_hip_gather_sync.restype = i
    L.dbde_hip_gather_sync.argtypes = [vp, i]
    L.dbde_hip_gather_rccl_version.restype = i
    L.dbde_hip_gather_rccl_version.argtypes = []
    L.dbde_hip_gather_plan.restype = i
    L.dbde_hip_gather_plan.argtypes = [i, i, i, C.POINTER(u64), u64, C.POINTER(GatherOp), i, C.POINTER(u64)]
    L.dbde_hip_gather_set_window.restype = i
    L.dbde_hip_gather_set_window.argtypes = [vp, u64]
    L.dbde_hip_gather_check.restype = i
    L.dbde_hip_gather_check.argtypes = [i, i, C.POINTER(u64), C.POINTER(u64)]
    L.dbde_hip_scatter_create.restype = i
    L.dbde_hip_scatter_create.argtypes = [vp, vp, i, i, i, C.POINTER(vp)]
    L.dbde_hip_scatter_attach.restype = i
    L.dbde_hip_scatter_attach.argtypes = [vp, vp, i, i, i, C.POINTER(vp)]
    L.dbde_hip_scatter_destroy.restype = None
    L.dbde_hip_scatter_destroy.argtypes = [vp]
    L.dbde_hip_scatter_error.restype = C.c_char_p
    L.dbde_hip_scatter_error.argtypes = [vp]
    L.dbde_hip_scatter_set_max_message.restype = i
    L.dbde_hip_scatter_set_max_message.argtypes = [vp, u64]
    L.dbde_hip_scatter_set_capacity.restype = i
    L.dbde_hip_scatter_set_capacity.argtypes = [vp, u64, u64]
    L.dbde_hip_scatter_begin.restype = i
    L.dbde_hip_scatter_begin.argtypes = [vp, i, vp, u64, vp, vp]
    L.dbde_hip_scatter_post.restype = i
    L.dbde_hip_scatter_post.argtypes = [vp, i, vp, vp, C.POINTER(ScatterBlock), C.POINTER(ScatterBlock), C.c_uint32]
    L.dbde_hip_scatter_join.restype = i
    L.dbde_hip_scatter_join.argtypes = [vp, i]
    L.dbde_hip_scatter_sync.restype = i
    L.dbde_hip_scatter_sync.argtypes = [vp, i]
    L.dbde_hip_scatter_blocks.restype = i
    L.dbde_hip_scatter_blocks.argtypes = [i, u64, C.POINTER(u64), u64, C.POINTER(ScatterBlock)]
    L.dbde_hip_scatter_check.restype = i
    L.dbde_hip_scatter_check.argtypes = [i, C.POINTER(ScatterBlock), C.POINTER(u64)]
    L.dbde_hip_scatter_plan.restype = i
    L.dbde_hip_scatter_plan.argtypes = [i, i, i, C.POINTER(ScatterBlock), u64, C.POINTER(ScatterOp), i]
    _lib = L
    return L


def max_frame_bytes(W, H):
    return int(lib().dbde_hip_max_frame_bytes(W, H))


def tiles(W, H):
    return ((W + 7) // 8) * ((H + 7) // 8)


def gather_plan(nranks, rank, root, sizes, max_piece=0):
    """dbde_hip_gather_plan: the ordered transfers of `rank` given every rank's byte count (host arithmetic only).
    -> (list of (peer, kind, segment_offset, window_offset, bytes), total bytes)."""
    arr = (C.c_uint64 * nranks)(*[int(x) for x in sizes])
    total = C.c_uint64(0)
    n = lib().dbde_hip_gather_plan(nranks, rank, root, arr, max_piece, None, 0, C.byref(total))
    if n < 0:
        raise ValueError(f"dbde_hip_gather_plan({nranks}, {rank}, {root}) -> {n}")
    ops = (GatherOp * max(n, 1))()
    lib().dbde_hip_gather_plan(nranks, rank, root, arr, max_piece, ops, n, None)
    return [(o.peer, o.kind, o.segment_offset, o.window_offset, o.bytes) for o in ops[:n]], total.value


class LaunchPlan(C.Structure):
    """dbde_hip_launch_plan (include/dbde_hip.h)."""
    _fields_ = [("kernel", C.c_int32), ("input_mode", C.c_int32), ("image_mode", C.c_int32), ("index_mode", C.c_int32),
                ("threads", C.c_int32), ("aligned_out", C.c_int32), ("chunks_per_frame", C.c_uint32),
                ("chunk_tiles", C.c_uint32), ("n_chunks", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


def encode_plan(W, H, n_frames, image_address=0, out_address=0, slot_stride=0, resident_workgroups=513):
    """dbde_hip_encode_plan: which kernel form an encode call with these arguments runs (host arithmetic only)."""
    pl = LaunchPlan()
    L = lib()
    L.dbde_hip_encode_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.POINTER(LaunchPlan)]
    rc = L.dbde_hip_encode_plan(W, H, n_frames, image_address, out_address, slot_stride, resident_workgroups, C.byref(pl))
    if rc != OK:
        raise ValueError(f"dbde_hip_encode_plan({W}, {H}, {n_frames}) -> {rc}")
    return pl.as_dict()


def decode_plan(W, H, n_frames, image_address=0, n_cu=256):
    """dbde_hip_decode_plan: which kernel form a decode call with these arguments runs (host arithmetic only)."""
    pl = LaunchPlan()
    L = lib()
    L.dbde_hip_decode_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_int, C.POINTER(LaunchPlan)]
    rc = L.dbde_hip_decode_plan(W, H, n_frames, image_address, n_cu, C.byref(pl))
    if rc != OK:
        raise ValueError(f"dbde_hip_decode_plan({W}, {H}, {n_frames}) -> {rc}")
    return pl.as_dict()


class RoiPlan(C.Structure):
    """dbde_hip_roi_plan_t (include/dbde_hip.h)."""
    _fields_ = [("tile_x", C.c_int32), ("tile_y", C.c_int32), ("tiles_x", C.c_int32), ("tiles_y", C.c_int32),
                ("max_tiles_x", C.c_int32), ("max_tiles_y", C.c_int32), ("chunks_per_frame", C.c_uint32),
                ("chunk_tiles", C.c_uint32), ("chunk_pieces", C.c_uint32), ("index_split", C.c_uint32),
                ("threads", C.c_uint32), ("pieces_x", C.c_uint32), ("grid", C.c_uint64), ("grid_origins", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


def _roi_plan(fn, W, H, n_frames, x, y, rw, rh):
    """roi_plan / roi16_plan through the C function named fn."""
    pl = RoiPlan()
    rc = getattr(lib(), fn)(W, H, n_frames, x, y, rw, rh, C.byref(pl))
    if rc != OK:
        raise ValueError(f"{fn}({W}, {H}, {n_frames}, {x}, {y}, {rw}, {rh}) -> {rc}")
    return pl.as_dict()


def roi_plan(W, H, n_frames, x, y, rw, rh):
    """dbde_hip_roi_plan: the tile window, index geometry and launch of a window decode (host arithmetic only).
    Raises ValueError where dbde_hip_decode_roi would return DBDE_HIP_ERR_ARG."""
    return _roi_plan("dbde_hip_roi_plan", W, H, n_frames, x, y, rw, rh)


def roi16_plan(W, H, n_frames, x, y, rw, rh):
    """dbde16_hip_roi_plan: roi_plan for DBDE16 windows (dbde16_hip_decode_roi).
    Raises ValueError where dbde16_hip_decode_roi would return DBDE_HIP_ERR_ARG."""
    return _roi_plan("dbde16_hip_roi_plan", W, H, n_frames, x, y, rw, rh)


def gather_check(nranks, root, sizes, caps):
    """dbde_hip_gather_check: (verdict, total) every rank reaches from the exchanged {count, capacity} pairs."""
    pairs = (C.c_uint64 * (2 * nranks))(*[int(x) for r in range(nranks) for x in (sizes[r], caps[r])])
    total = C.c_uint64(0)
    rc = lib().dbde_hip_gather_check(nranks, root, pairs, C.byref(total))
    return rc, int(total.value)


def scatter_blocks(nranks, frame_offsets, stream_bytes):
    """dbde_hip_scatter_blocks: [(first_frame, n_frames, byte_start, byte_count)] per rank from a host-side frame index."""
    n = len(frame_offsets)
    arr = (C.c_uint64 * max(n, 1))(*[int(x) for x in frame_offsets])
    table = (ScatterBlock * nranks)()
    rc = lib().dbde_hip_scatter_blocks(nranks, n, arr, int(stream_bytes), table)
    if rc != OK:
        raise ValueError(f"dbde_hip_scatter_blocks -> {rc}")
    return [(int(b.first_frame), int(b.n_frames), int(b.byte_start), int(b.byte_count)) for b in table]


def _scatter_table(blocks):
    table = (ScatterBlock * len(blocks))()
    for k, b in enumerate(blocks):
        table[k].first_frame, table[k].n_frames, table[k].byte_start, table[k].byte_count = [int(x) for x in b]
    return table


def scatter_check(blocks, caps):
    """dbde_hip_scatter_check: OK or ERR_CAPACITY; caps = [(segment_bytes, max_frames)] per rank."""
    flat = (C.c_uint64 * (2 * len(caps)))(*[int(x) for c in caps for x in c])
    return lib().dbde_hip_scatter_check(len(blocks), _scatter_table(blocks), flat)


def scatter_plan(nranks, rank, root, blocks, max_piece=0):
    """dbde_hip_scatter_plan: the ordered transfers of `rank` -> [(peer, kind, source_offset, dest_offset, bytes)]."""
    table = _scatter_table(blocks)
    n = lib().dbde_hip_scatter_plan(nranks, rank, root, table, max_piece, None, 0)
    if n < 0:
        raise ValueError(f"dbde_hip_scatter_plan({nranks}, {rank}, {root}) -> {n}")
    ops = (ScatterOp * max(n, 1))()
    lib().dbde_hip_scatter_plan(nranks, rank, root, table, max_piece, ops, n)
    return [(o.peer, o.kind, int(o.source_offset), int(o.dest_offset), int(o.bytes)) for o in ops[:n]]


def gather_unique_id():
    """Rendezvous token of the native gather (ncclGetUniqueId), as a 128-byte uint8 numpy array."""
    out = np.zeros(GATHER_ID_BYTES, np.uint8)
    rc = lib().dbde_hip_gather_unique_id(out.ctypes.data)
    if rc != OK:
        raise RuntimeError(f"dbde_hip_gather_unique_id failed ({rc}): librccl could not be opened")
    return out


# ---- header wire format (host only) ------------------------------------------------------

def pack_frame_header(u64s, index, elapsed_ns):
    out = np.zeros(20, np.uint8)
    fh = FrameHeader(u64s, index, elapsed_ns)
    assert lib().dbde_hip_pack_frame_header(C.byref(fh), out.ctypes.data) == 20
    return out


def pack_video_header(u64s, height, width, frame_hz):
    out = np.zeros(28, np.uint8)
    vh = VideoHeader(u64s, height, width, frame_hz)
    assert lib().dbde_hip_pack_video_header(C.byref(vh), out.ctypes.data) == 28
    return out


def unpack_frame_header(packed):
    buf = np.ascontiguousarray(np.asarray(packed, np.uint8)[:20])
    cur = C.c_void_p(buf.ctypes.data)
    fh = lib().dbde_hip_unpack_frame_header(C.byref(cur))
    return cur.value - buf.ctypes.data, (fh.u64s, fh.index, fh.elapsed_ns)


def unpack_video_header(packed):
    buf = np.ascontiguousarray(np.asarray(packed, np.uint8)[:28])
    cur = C.c_void_p(buf.ctypes.data)
    vh = lib().dbde_hip_unpack_video_header(C.byref(cur))
    return cur.value - buf.ctypes.data, (vh.u64s, vh.height, vh.width, vh.frame_hz)


STATS = {"max": 1, "min": 2, "sum": 4, "sumsq": 8}


def stats_mask(stats):
    """("max", "min", "sum", "sumsq") names (or an int bitmask) -> dbde_hip_project_plan's bitmask."""
    if isinstance(stats, int):
        return stats
    if isinstance(stats, str):
        stats = (stats,)
    mask = 0
    for name in stats:
        if name not in STATS:
            raise ValueError(f"unknown statistic {name!r} (one of {sorted(STATS)})")
        mask |= STATS[name]
    return mask


class ProjectPlan(C.Structure):
    """dbde_hip_project_plan_t (include/dbde_hip.h)."""
    _fields_ = [("tile_x", C.c_int32), ("tile_y", C.c_int32), ("tiles_x", C.c_int32), ("tiles_y", C.c_int32),
                ("chunks_per_frame", C.c_uint32), ("chunk_tiles", C.c_uint32), ("chunk_pieces", C.c_uint32),
                ("index_split", C.c_uint32), ("threads", C.c_uint32), ("pieces_x", C.c_uint32),
                ("segments", C.c_uint32), ("frames_per_segment", C.c_uint32), ("max_frames_per_segment", C.c_uint32),
                ("reserved_", C.c_uint32), ("grid", C.c_uint64), ("combine_grid", C.c_uint64),
                ("workspace_bytes", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "reserved_"}


def _project_plan(fn, W, H, n_frames, x, y, rw, rh, stats, n_cu):
    """project_plan / project16_plan through the C function named fn."""
    rw = W - x if rw is None else rw
    rh = H - y if rh is None else rh
    pl = ProjectPlan()
    rc = getattr(lib(), fn)(W, H, n_frames, x, y, rw, rh, stats_mask(stats), n_cu, C.byref(pl))
    if rc != OK:
        raise ValueError(f"{fn}({W}, {H}, {n_frames}, {x}, {y}, {rw}, {rh}, {stats}) -> {rc}")
    return pl.as_dict()


def project_plan(W, H, n_frames, x=0, y=0, rw=None, rh=None, stats=("max", "min", "sum", "sumsq"), n_cu=256):
    """dbde_hip_project_plan: the tile window, index geometry, launch and workspace of a projection (host arithmetic
    only).  rw / rh default to the rest of the frame.  Raises ValueError where dbde_hip_project would return
    DBDE_HIP_ERR_ARG."""
    return _project_plan("dbde_hip_project_plan", W, H, n_frames, x, y, rw, rh, stats, n_cu)


def project16_plan(W, H, n_frames, x=0, y=0, rw=None, rh=None, stats=("max", "min", "sum", "sumsq"), n_cu=256):
    """dbde16_hip_project_plan: project_plan for DBDE16 projections (Codec.project16)."""
    return _project_plan("dbde16_hip_project_plan", W, H, n_frames, x, y, rw, rh, stats, n_cu)


class Projection:
    """Device tensors of a temporal projection (Codec.project): max / min uint8 (rh, rw), sum / sumsq int64 (rh, rw)
    (the values stay below 2^63), count int64 (1,).  A statistic that was not asked for is None.  Codec.project16's
    max / min are int16 tensors holding the U16 bits (as decode_frames16 returns its images)."""

    def __init__(self, max=None, min=None, sum=None, sumsq=None, count=None):
        self.max, self.min, self.sum, self.sumsq, self.count = max, min, sum, sumsq, count

    @classmethod
    def empty(cls, rh, rw, stats, device, pix=1):
        """Uninitialised outputs for `stats`; pix: bytes per pixel of max / min (1: uint8, 2: int16 for DBDE16)."""
        mask = stats_mask(stats)
        if pix not in (1, 2):
            raise ValueError(f"pix must be 1 or 2, not {pix!r}")
        mm_dtype = torch.uint8 if pix == 1 else torch.int16
        mm = lambda: torch.empty((rh, rw), dtype=mm_dtype, device=device)      # noqa: E731
        i64 = lambda: torch.empty((rh, rw), dtype=torch.int64, device=device)   # noqa: E731
        return cls(mm() if mask & 1 else None, mm() if mask & 2 else None, i64() if mask & 4 else None,
                   i64() if mask & 8 else None, torch.zeros(1, dtype=torch.int64, device=device))

    def mean(self):
        """Per-pixel mean (float64, on the device); NaN where no frame contributed."""
        return self.sum.to(torch.float64) / self.count.to(torch.float64)

    def std(self):
        """Per-pixel population standard deviation (float64, on the device); NaN where no frame contributed."""
        n = self.count.to(torch.float64)
        m = self.sum.to(torch.float64) / n
        return (self.sumsq.to(torch.float64) / n - m * m).clamp_(min=0.0).sqrt_()


SUM_U32, SUM_U16 = 0, 1


def _sum_type(sum_dtype):
    """torch.int32 (U32 bits) / torch.int16 (U16 bits), or SUM_U32 / SUM_U16 -> dbde_hip_project_groups' sum_type."""
    if isinstance(sum_dtype, int) and sum_dtype in (SUM_U32, SUM_U16):
        return sum_dtype
    if torch is not None and sum_dtype == torch.int32:
        return SUM_U32
    if torch is not None and sum_dtype == torch.int16:
        return SUM_U16
    raise ValueError(f"sum_dtype must be torch.int32 or torch.int16, not {sum_dtype!r}")


class GroupProjectPlan(C.Structure):
    """dbde_hip_project_groups_plan_t (include/dbde_hip.h)."""
    _fields_ = [("tile_x", C.c_int32), ("tile_y", C.c_int32), ("tiles_x", C.c_int32), ("tiles_y", C.c_int32),
                ("chunks_per_frame", C.c_uint32), ("chunk_tiles", C.c_uint32), ("chunk_pieces", C.c_uint32),
                ("index_split", C.c_uint32), ("threads", C.c_uint32), ("pieces_x", C.c_uint32),
                ("runs", C.c_uint32), ("groups_per_run", C.c_uint32), ("max_group_frames", C.c_uint32),
                ("stats", C.c_uint32), ("grid", C.c_uint64), ("sum_bytes", C.c_uint64), ("max_bytes", C.c_uint64),
                ("min_bytes", C.c_uint64), ("sumsq_bytes", C.c_uint64), ("counts_bytes", C.c_uint64),
                ("workspace_bytes", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


def _project_groups_plan(fn, W, H, n_frames, x, y, rw, rh, group_frames, has_group_starts, n_groups, stats, sum_dtype,
                         accumulate, n_cu, addresses):
    """project_groups_plan / project_groups16_plan through the C function named fn."""
    rw = W - x if rw is None else rw
    rh = H - y if rh is None else rh
    g = 0 if group_frames is None else int(group_frames)
    if n_groups is None:
        if has_group_starts or g < 1:
            raise ValueError("n_groups is needed (only the uniform form implies it)")
        n_groups = -(-n_frames // g)
    mask = stats_mask(stats)
    addr = {name: (4096 if mask & bit else 0) for name, bit in STATS.items()}
    addr["counts"] = 4096
    addr.update(addresses or {})
    pl = GroupProjectPlan()
    rc = getattr(lib(), fn)(W, H, n_frames, x, y, rw, rh, g, 1 if has_group_starts else 0, n_groups,
                            _sum_type(sum_dtype), int(accumulate), addr["max"], addr["min"], addr["sum"], addr["sumsq"],
                            addr["counts"], n_cu, C.byref(pl))
    if rc != OK:
        raise ValueError(f"{fn}({W}, {H}, {n_frames}, {x}, {y}, {rw}, {rh}, g={g}, starts={has_group_starts}, "
                         f"groups={n_groups}, {stats}) -> {rc}")
    return pl.as_dict()


def project_groups_plan(W, H, n_frames, x=0, y=0, rw=None, rh=None, group_frames=None, has_group_starts=False,
                        n_groups=None, stats=("max", "min", "sum", "sumsq"), sum_dtype=SUM_U32, accumulate=False,
                        n_cu=256, addresses=None):
    """dbde_hip_project_groups_plan: the tile window, index geometry, launch and plane sizes of a grouped projection
    (host arithmetic only).  n_groups defaults to ceil(n_frames / group_frames) in the uniform form.  addresses: optional
    {"max" | "min" | "sum" | "sumsq" | "counts": address} standing for the call's output pointers (0 = NULL; the default
    is an aligned address for every statistic in `stats`).  Raises ValueError where dbde_hip_project_groups would return
    DBDE_HIP_ERR_ARG."""
    return _project_groups_plan("dbde_hip_project_groups_plan", W, H, n_frames, x, y, rw, rh, group_frames,
                                has_group_starts, n_groups, stats, sum_dtype, accumulate, n_cu, addresses)


def project_groups16_plan(W, H, n_frames, x=0, y=0, rw=None, rh=None, group_frames=None, has_group_starts=False,
                          n_groups=None, stats=("max", "min", "sum", "sumsq"), sum_dtype=SUM_U32, accumulate=False,
                          n_cu=256, addresses=None):
    """dbde16_hip_project_groups_plan: project_groups_plan for DBDE16 streams (Codec.project_groups16)."""
    return _project_groups_plan("dbde16_hip_project_groups_plan", W, H, n_frames, x, y, rw, rh, group_frames,
                                has_group_starts, n_groups, stats, sum_dtype, accumulate, n_cu, addresses)


class GroupProjection:
    """Device tensors of a grouped projection (Codec.project_groups): max / min uint8 (n_groups, rh, rw), sum int32
    holding the U32 bits (int16 holding U16 bits with sum_dtype=torch.int16), sumsq int64, counts int32 (n_groups,).
    A statistic that was not asked for is None.  Codec.project_groups16's max / min are int16 tensors holding the U16
    bits."""

    def __init__(self, max=None, min=None, sum=None, sumsq=None, counts=None):
        self.max, self.min, self.sum, self.sumsq, self.counts = max, min, sum, sumsq, counts

    @classmethod
    def empty(cls, n_groups, rh, rw, stats, device, pix=1, sum_dtype=None):
        """Uninitialised planes for `stats`; pix: bytes per pixel of max / min (1: uint8, 2: int16 for DBDE16)."""
        mask = stats_mask(stats)
        if pix not in (1, 2):
            raise ValueError(f"pix must be 1 or 2, not {pix!r}")
        sum_dtype = torch.int32 if sum_dtype is None else sum_dtype
        _sum_type(sum_dtype)
        mm_dtype = torch.uint8 if pix == 1 else torch.int16
        new = lambda dt: torch.empty((n_groups, rh, rw), dtype=dt, device=device)   # noqa: E731
        return cls(new(mm_dtype) if mask & 1 else None, new(mm_dtype) if mask & 2 else None,
                   new(sum_dtype) if mask & 4 else None, new(torch.int64) if mask & 8 else None,
                   torch.zeros(n_groups, dtype=torch.int32, device=device))

    def sums(self):
        """The sums as int64 values (the U32 / U16 bits unsigned)."""
        bits = 0xFFFF if self.sum.dtype == torch.int16 else 0xFFFFFFFF
        return self.sum.to(torch.int64) & bits

    def _n(self):
        return (self.counts.to(torch.int64) & 0xFFFFFFFF).to(torch.float64).view(-1, 1, 1)

    def mean(self):
        """Per-group, per-pixel mean (float64, on the device); NaN for a group without an accepted frame."""
        return self.sums().to(torch.float64) / self._n()

    def std(self):
        """Per-group, per-pixel population standard deviation (float64, on the device); NaN for a group with count 0."""
        n = self._n()
        m = self.sums().to(torch.float64) / n
        return (self.sumsq.to(torch.float64) / n - m * m).clamp_(min=0.0).sqrt_()


WPROJ_MAX_REGRESSORS = 8
WPROJ_ONE_SEGMENT = 1
REJECTED_CONSUMED = 20       # `consumed` of a frame that failed validation (results[:, 3]); an accepted frame has more


def accepted_frames(results):
    """bool (n,): the frames of a results tensor (n, 4) that passed validation.  The verdict is read from `consumed`: a
    rejected frame reports 20, an accepted one its whole size; header.u64s is whatever the stream's header holds."""
    return results[:, 3] != REJECTED_CONSUMED


class WeightedProjectPlan(C.Structure):
    """dbde_hip_project_weighted_plan_t (include/dbde_hip.h)."""
    _fields_ = [("tile_x", C.c_int32), ("tile_y", C.c_int32), ("tiles_x", C.c_int32), ("tiles_y", C.c_int32),
                ("chunks_per_frame", C.c_uint32), ("chunk_tiles", C.c_uint32), ("chunk_pieces", C.c_uint32),
                ("index_split", C.c_uint32), ("threads", C.c_uint32), ("pieces_x", C.c_uint32),
                ("segments", C.c_uint32), ("frames_per_segment", C.c_uint32), ("max_frames_per_segment", C.c_uint32),
                ("regressors", C.c_uint32), ("grid", C.c_uint64), ("combine_grid", C.c_uint64),
                ("workspace_bytes", C.c_uint64), ("lds_bytes", C.c_uint32), ("reserved_", C.c_uint32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "reserved_"}


def _wproject_plan(fn, W, H, n_frames, x, y, rw, rh, regressors, n_cu, one_segment, weight_stride, addresses):
    """wproject_plan / wproject16_plan through the C function named fn."""
    rw = W - x if rw is None else rw
    rh = H - y if rh is None else rh
    addr = {"weights": 4096, "out": 4096, "count": 4096}
    addr.update(addresses or {})
    flags = one_segment if isinstance(one_segment, int) and not isinstance(one_segment, bool) else (
        WPROJ_ONE_SEGMENT if one_segment else 0)
    stride = max(n_frames, 0) if weight_stride is None else weight_stride
    pl = WeightedProjectPlan()
    rc = getattr(lib(), fn)(W, H, n_frames, x, y, rw, rh, regressors, stride, flags, addr["weights"], addr["out"],
                            addr["count"], n_cu, C.byref(pl))
    if rc != OK:
        raise ValueError(f"{fn}({W}, {H}, {n_frames}, {x}, {y}, {rw}, {rh}, R={regressors}, stride={stride}, "
                         f"flags={flags}) -> {rc}")
    return pl.as_dict()


def wproject_plan(W, H, n_frames, x=0, y=0, rw=None, rh=None, regressors=1, n_cu=256, one_segment=False,
                  weight_stride=None, addresses=None):
    """dbde_hip_project_weighted_plan: the tile window, index geometry, launch, segments and workspace of a weighted
    projection (host arithmetic only).  rw / rh default to the rest of the frame, weight_stride to n_frames.
    one_segment: True / False (or an int: the raw flags).  addresses: optional {"weights" | "out" | "count": address}
    standing for the call's pointers (0 = NULL; aligned by default).  Raises ValueError where
    dbde_hip_project_weighted would return DBDE_HIP_ERR_ARG."""
    return _wproject_plan("dbde_hip_project_weighted_plan", W, H, n_frames, x, y, rw, rh, regressors, n_cu, one_segment,
                          weight_stride, addresses)


def wproject16_plan(W, H, n_frames, x=0, y=0, rw=None, rh=None, regressors=1, n_cu=256, one_segment=False,
                    weight_stride=None, addresses=None):
    """dbde16_hip_project_weighted_plan: wproject_plan for DBDE16 streams (Codec.project_weighted16)."""
    return _wproject_plan("dbde16_hip_project_weighted_plan", W, H, n_frames, x, y, rw, rh, regressors, n_cu,
                          one_segment, weight_stride, addresses)


class WeightedProjection:
    """Device tensors of a weighted projection (Codec.project_weighted): out float32 (R, rh, rw), plane r holding the
    sum over the accepted frames of weights[r][f] * pixel; count int64 (1,), the frames that contributed."""

    def __init__(self, out=None, count=None):
        self.out, self.count = out, count

    @classmethod
    def empty(cls, R, rh, rw, device):
        """Uninitialised planes and a zero count."""
        return cls(torch.empty((R, rh, rw), dtype=torch.float32, device=device),
                   torch.zeros(1, dtype=torch.int64, device=device))

    @staticmethod
    def weight_sums(weights, results):
        """Sum of the accepted frames' weights per regressor: float64 (R,), on the weights' device.  weights: (R, >= n)
        or (>= n,); results: the (n, 4) int64 tensor the call returned (accepted_frames reads the verdicts).  A torch
        helper, not a kernel: it is what turns plane r into a covariance with `Projection.sum` (regressors.pearson)."""
        w = weights if weights.dim() == 2 else weights.view(1, -1)
        n = results.shape[0]
        ok = accepted_frames(results).to(w.device)
        w64 = w[:, :n].to(torch.float64)
        return torch.where(ok.view(1, -1), w64, torch.zeros_like(w64)).sum(1)


COUNTS_MAX_LEVELS = 8
COUNTS_MAPS = 1


class CountProjectPlan(C.Structure):
    """dbde_hip_project_counts_plan_t (include/dbde_hip.h)."""
    _fields_ = [("tile_x", C.c_int32), ("tile_y", C.c_int32), ("tiles_x", C.c_int32), ("tiles_y", C.c_int32),
                ("chunks_per_frame", C.c_uint32), ("chunk_tiles", C.c_uint32), ("chunk_pieces", C.c_uint32),
                ("index_split", C.c_uint32), ("threads", C.c_uint32), ("pieces_x", C.c_uint32),
                ("segments", C.c_uint32), ("frames_per_segment", C.c_uint32), ("max_frames_per_segment", C.c_uint32),
                ("levels", C.c_uint32), ("grid", C.c_uint64), ("combine_grid", C.c_uint64),
                ("workspace_bytes", C.c_uint64), ("lds_bytes", C.c_uint32), ("reserved_", C.c_uint32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "reserved_"}


def _counts_plan(fn, W, H, n_frames, x, y, rw, rh, levels, n_cu, maps, level_stride, addresses):
    """counts_plan / counts16_plan through the C function named fn."""
    rw = W - x if rw is None else rw
    rh = H - y if rh is None else rh
    addr = {"thresholds": 4096, "out": 4096, "count": 4096}
    addr.update(addresses or {})
    flags = maps if isinstance(maps, int) and not isinstance(maps, bool) else (COUNTS_MAPS if maps else 0)
    stride = max(rw, 0) * max(rh, 0) if level_stride is None else level_stride
    pl = CountProjectPlan()
    rc = getattr(lib(), fn)(W, H, n_frames, x, y, rw, rh, levels, stride, flags, addr["thresholds"], addr["out"],
                            addr["count"], n_cu, C.byref(pl))
    if rc != OK:
        raise ValueError(f"{fn}({W}, {H}, {n_frames}, {x}, {y}, {rw}, {rh}, K={levels}, stride={stride}, "
                         f"flags={flags}) -> {rc}")
    return pl.as_dict()


def counts_plan(W, H, n_frames, x=0, y=0, rw=None, rh=None, levels=1, n_cu=256, maps=False, level_stride=None,
                addresses=None):
    """dbde_hip_project_counts_plan: the tile window, index geometry, launch, segments and workspace of a count
    projection (host arithmetic only).  rw / rh default to the rest of the frame, level_stride to rw * rh.  maps: True /
    False (or an int: the raw flags).  addresses: optional {"thresholds" | "out" | "count": address} standing for the
    call's pointers (0 = NULL; aligned by default).  Raises ValueError where dbde_hip_project_counts would return
    DBDE_HIP_ERR_ARG."""
    return _counts_plan("dbde_hip_project_counts_plan", W, H, n_frames, x, y, rw, rh, levels, n_cu, maps, level_stride,
                        addresses)


def counts16_plan(W, H, n_frames, x=0, y=0, rw=None, rh=None, levels=1, n_cu=256, maps=False, level_stride=None,
                  addresses=None):
    """dbde16_hip_project_counts_plan: counts_plan for DBDE16 streams (Codec.project_counts16)."""
    return _counts_plan("dbde16_hip_project_counts_plan", W, H, n_frames, x, y, rw, rh, levels, n_cu, maps,
                        level_stride, addresses)


class CountProjection:
    """Device tensors of a count projection (Codec.project_counts): out int32 (K, rh, rw), plane k holding the number of
    accepted frames whose pixel is <= threshold k (U32 bits: exact below 2^31 frames); count int64 (1,), the frames that
    contributed."""

    def __init__(self, out=None, count=None):
        self.out, self.count = out, count

    @classmethod
    def empty(cls, K, rh, rw, device):
        """Uninitialised planes and a zero count."""
        return cls(torch.empty((K, rh, rw), dtype=torch.int32, device=device),
                   torch.zeros(1, dtype=torch.int64, device=device))

    def fraction(self):
        """out / count in float64 (K, rh, rw): the fraction of the accepted frames at or below each threshold (NaN where
        no frame was accepted)."""
        return self.out.to(torch.float64) / self.count.to(torch.float64)


PAIR_RIGHT, PAIR_DOWN, PAIR_DOWN_RIGHT, PAIR_DOWN_LEFT = 1, 2, 4, 8
PAIR_OFFSETS = ((1, 0), (0, 1), (1, 1), (-1, 1))   # (dx, dy) of bits 0..3


def pairs_mask(pairs):
    """4 (the 4-neighbourhood: RIGHT | DOWN), 8 (the 8-neighbourhood: all four), any other int in 1..15 (a mask of
    PAIR_* bits), or an iterable of (dx, dy) from PAIR_OFFSETS -> dbde_hip_project_pairs' mask.  The ints 4 and 8 always
    mean the neighbourhoods: DOWN_RIGHT or DOWN_LEFT alone are asked for as [(1, 1)] / [(-1, 1)]."""
    if isinstance(pairs, (int, np.integer)) and not isinstance(pairs, bool):
        mask = {4: 3, 8: 15}.get(int(pairs), int(pairs))
    else:
        mask = 0
        for off in pairs:
            off = tuple(int(v) for v in off)
            if off not in PAIR_OFFSETS:
                raise ValueError(f"offset {off} is not one of {PAIR_OFFSETS}")
            mask |= 1 << PAIR_OFFSETS.index(off)
    if not 1 <= mask <= 15:
        raise ValueError(f"pairs must be 4, 8, a mask in 1..15 or offsets from {PAIR_OFFSETS}, not {pairs!r}")
    return mask


def pair_offsets(mask):
    """The (dx, dy) of each plane of mask, in plane order."""
    return tuple(PAIR_OFFSETS[b] for b in range(4) if (mask >> b) & 1)


class PairProjectPlan(C.Structure):
    """dbde_hip_project_pairs_plan_t (include/dbde_hip.h)."""
    _fields_ = [("tile_x", C.c_int32), ("tile_y", C.c_int32), ("tiles_x", C.c_int32), ("tiles_y", C.c_int32),
                ("chunks_per_frame", C.c_uint32), ("chunk_tiles", C.c_uint32), ("chunk_pieces", C.c_uint32),
                ("index_split", C.c_uint32), ("threads", C.c_uint32), ("pieces_x", C.c_uint32),
                ("segments", C.c_uint32), ("frames_per_segment", C.c_uint32), ("max_frames_per_segment", C.c_uint32),
                ("planes", C.c_uint32), ("grid", C.c_uint64), ("combine_grid", C.c_uint64),
                ("workspace_bytes", C.c_uint64), ("lds_bytes", C.c_uint32), ("instance", C.c_uint32),
                ("piece_tiles", C.c_uint32), ("piece_stride", C.c_uint32), ("halo_left", C.c_uint32),
                ("halo_right", C.c_uint32), ("rows_below", C.c_uint32), ("reserved_", C.c_uint32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "reserved_"}


def _pairs_plan(fn, W, H, n_frames, x, y, rw, rh, pairs, n_cu, addresses):
    """pairs_plan / pairs16_plan through the C function named fn."""
    rw = W - x if rw is None else rw
    rh = H - y if rh is None else rh
    addr = {"out": 4096, "count": 4096}
    addr.update(addresses or {})
    pl = PairProjectPlan()
    rc = getattr(lib(), fn)(W, H, n_frames, x, y, rw, rh, pairs, addr["out"], addr["count"], n_cu, C.byref(pl))
    if rc != OK:
        raise ValueError(f"{fn}({W}, {H}, {n_frames}, {x}, {y}, {rw}, {rh}, pairs={pairs}) -> {rc}")
    return pl.as_dict()


def pairs_plan(W, H, n_frames, x=0, y=0, rw=None, rh=None, pairs=15, n_cu=256, addresses=None):
    """dbde_hip_project_pairs_plan: the tile window, index geometry, launch, halo, segments and workspace of a pair
    projection (host arithmetic only).  rw / rh default to the rest of the frame.  pairs: the raw mask (anything outside
    1..15 is rejected).  addresses: optional {"out" | "count": address} standing for the call's pointers (0 = NULL;
    aligned by default).  Raises ValueError where dbde_hip_project_pairs would return DBDE_HIP_ERR_ARG."""
    return _pairs_plan("dbde_hip_project_pairs_plan", W, H, n_frames, x, y, rw, rh, pairs, n_cu, addresses)


def pairs16_plan(W, H, n_frames, x=0, y=0, rw=None, rh=None, pairs=15, n_cu=256, addresses=None):
    """dbde16_hip_project_pairs_plan: pairs_plan for DBDE16 streams (Codec.project_pairs16)."""
    return _pairs_plan("dbde16_hip_project_pairs_plan", W, H, n_frames, x, y, rw, rh, pairs, n_cu, addresses)


class PairProjection:
    """Device tensors of a pair projection (Codec.project_pairs): out int64 (P, rh, rw) holding the U64 bits (the sums
    stay below 2^63, see include/dbde_hip.h), plane j the sum over the accepted frames of p[y][x] * p[y + dy][x + dx]
    for (dx, dy) = offsets[j], zero where the partner lies outside the window; count int64 (1,), the frames that
    contributed; offsets, the (dx, dy) of each plane."""

    def __init__(self, out=None, count=None, offsets=None):
        self.out, self.count, self.offsets = out, count, tuple(offsets) if offsets is not None else None

    @property
    def mask(self):
        return pairs_mask(self.offsets)

    @classmethod
    def empty(cls, pairs, rh, rw, device):
        """Uninitialised planes and a zero count for `pairs` (what Codec.project_pairs takes)."""
        offsets = pair_offsets(pairs_mask(pairs))
        return cls(torch.empty((len(offsets), rh, rw), dtype=torch.int64, device=device),
                   torch.zeros(1, dtype=torch.int64, device=device), offsets)


LAG_STATS = ("product", "pairsum", "absdiff", "sqdiff", "maxdiff")   # bits 0..4 of dbde_hip_project_lag_plan's stats
LAG_MAX = 8


def lag_mask(stats):
    """An iterable of names from LAG_STATS (or one name, or a mask in 1..31) -> the DBDE_HIP_LAG_* mask."""
    if isinstance(stats, (int, np.integer)) and not isinstance(stats, bool):
        mask = int(stats)
    else:
        mask = 0
        for name in ((stats,) if isinstance(stats, str) else stats):
            if name not in LAG_STATS:
                raise ValueError(f"statistic {name!r} is not one of {LAG_STATS}")
            mask |= 1 << LAG_STATS.index(name)
    if not 1 <= mask <= 31:
        raise ValueError(f"stats must name at least one of {LAG_STATS}, not {stats!r}")
    return mask


def lag_stats(mask):
    """The names of the statistics of mask, in bit order."""
    return tuple(LAG_STATS[b] for b in range(5) if (mask >> b) & 1)


class LagProjectPlan(C.Structure):
    """dbde_hip_project_lag_plan_t (include/dbde_hip.h)."""
    _fields_ = [("tile_x", C.c_int32), ("tile_y", C.c_int32), ("tiles_x", C.c_int32), ("tiles_y", C.c_int32),
                ("chunks_per_frame", C.c_uint32), ("chunk_tiles", C.c_uint32), ("chunk_pieces", C.c_uint32),
                ("index_split", C.c_uint32), ("threads", C.c_uint32), ("pieces_x", C.c_uint32),
                ("segments", C.c_uint32), ("frames_per_segment", C.c_uint32), ("max_frames_per_segment", C.c_uint32),
                ("planes", C.c_uint32), ("grid", C.c_uint64), ("combine_grid", C.c_uint64),
                ("workspace_bytes", C.c_uint64), ("lds_bytes", C.c_uint32), ("instance", C.c_uint32),
                ("first_frame", C.c_uint32), ("history_frames", C.c_uint32), ("first_pair", C.c_uint32),
                ("reserved_", C.c_uint32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "reserved_"}


def _lag_plan(fn, W, H, n_frames, x, y, rw, rh, lag, lead, stats, n_cu, addresses):
    """lag_plan / lag16_plan through the C function named fn."""
    rw = W - x if rw is None else rw
    rh = H - y if rh is None else rh
    addr = {"sums": 4096, "maxdiff": 4096, "pairs": 4096, "count": 4096}
    addr.update(addresses or {})
    pl = LagProjectPlan()
    rc = getattr(lib(), fn)(W, H, n_frames, x, y, rw, rh, lag, lead, stats, addr["sums"], addr["maxdiff"], addr["pairs"],
                            addr["count"], n_cu, C.byref(pl))
    if rc != OK:
        raise ValueError(f"{fn}({W}, {H}, {n_frames}, {x}, {y}, {rw}, {rh}, lag={lag}, lead={lead}, stats={stats}) -> {rc}")
    return pl.as_dict()


def lag_plan(W, H, n_frames, x=0, y=0, rw=None, rh=None, lag=1, lead=0, stats=31, n_cu=256, addresses=None):
    """dbde_hip_project_lag_plan: the tile window, index geometry, launch, segments, history frames, instance and
    workspace of a lag projection (host arithmetic only).  rw / rh default to the rest of the frame.  stats: the raw
    mask of DBDE_HIP_LAG_* bits (anything outside 1..31 is rejected).  addresses: optional {"sums" | "maxdiff" | "pairs"
    | "count": address} standing for the call's pointers (aligned by default; pairs / count 0 = NULL).  Raises
    ValueError where dbde_hip_project_lag would return DBDE_HIP_ERR_ARG."""
    return _lag_plan("dbde_hip_project_lag_plan", W, H, n_frames, x, y, rw, rh, lag, lead, stats, n_cu, addresses)


def lag16_plan(W, H, n_frames, x=0, y=0, rw=None, rh=None, lag=1, lead=0, stats=31, n_cu=256, addresses=None):
    """dbde16_hip_project_lag_plan: lag_plan for DBDE16 streams (Codec.project_lag16)."""
    return _lag_plan("dbde16_hip_project_lag_plan", W, H, n_frames, x, y, rw, rh, lag, lead, stats, n_cu, addresses)


class RegisteredProjectPlan(C.Structure):
    """dbde_hip_project_registered_plan_t (include/dbde_hip.h)."""
    _fields_ = [("chunks_per_frame", C.c_uint32), ("chunk_tiles", C.c_uint32), ("chunk_pieces", C.c_uint32),
                ("index_split", C.c_uint32), ("threads", C.c_uint32), ("piece_cols", C.c_uint32),
                ("pieces_x", C.c_uint32), ("band_rows", C.c_uint32), ("bands", C.c_uint32), ("segments", C.c_uint32),
                ("frames_per_segment", C.c_uint32), ("max_frames_per_segment", C.c_uint32), ("grid", C.c_uint64),
                ("combine_grid", C.c_uint64), ("workspace_bytes", C.c_uint64), ("lds_bytes", C.c_uint32),
                ("instance", C.c_uint32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


def _registered_plan(fn, W, H, n_frames, rw, rh, stats, n_cu):
    """registered_plan / registered16_plan through the C function named fn."""
    pl = RegisteredProjectPlan()
    rc = getattr(lib(), fn)(W, H, n_frames, rw, rh, stats_mask(stats), n_cu, C.byref(pl))
    if rc != OK:
        raise ValueError(f"{fn}({W}, {H}, {n_frames}, {rw}, {rh}, {stats}) -> {rc}")
    return pl.as_dict()


def registered_plan(W, H, n_frames, rw, rh, stats=("max", "min", "sum", "sumsq"), n_cu=256):
    """dbde_hip_project_registered_plan: the index geometry, pieces, bands, segments, instance, LDS and workspace of a
    registered projection (host arithmetic only).  Raises ValueError where dbde_hip_project_registered would return
    DBDE_HIP_ERR_ARG for its sizes or statistics."""
    return _registered_plan("dbde_hip_project_registered_plan", W, H, n_frames, rw, rh, stats, n_cu)


def registered16_plan(W, H, n_frames, rw, rh, stats=("max", "min", "sum", "sumsq"), n_cu=256):
    """dbde16_hip_project_registered_plan: registered_plan for DBDE16 streams (Codec.project_registered16)."""
    return _registered_plan("dbde16_hip_project_registered_plan", W, H, n_frames, rw, rh, stats, n_cu)


class LagProjection:
    """Device tensors of a lag projection (Codec.project_lag): product, pairsum, absdiff, sqdiff int64 (rh, rw) holding
    the U64 bits (the sums stay below 2^63, see include/dbde_hip.h), maxdiff uint8 (rh, rw) (project_lag16: int16
    holding the U16 bits), each None where not requested; pairs int64 (1,), the counted pairs; count int64 (1,), the
    accepted frames past the lead; lag, the distance of the two frames of a pair."""

    def __init__(self, product=None, pairsum=None, absdiff=None, sqdiff=None, maxdiff=None, pairs=None, count=None,
                 lag=None):
        self.product, self.pairsum, self.absdiff, self.sqdiff, self.maxdiff = product, pairsum, absdiff, sqdiff, maxdiff
        self.pairs, self.count, self.lag = pairs, count, lag

    @property
    def stats(self):
        return tuple(k for k in LAG_STATS if getattr(self, k) is not None)

    @classmethod
    def empty(cls, stats, rh, rw, device, lag=1, bits=8):
        """Uninitialised planes and zero scalars for `stats` (what Codec.project_lag takes)."""
        names = lag_stats(lag_mask(stats))
        planes = {k: torch.empty((rh, rw), dtype=(torch.int64 if k != "maxdiff" else
                                                  torch.uint8 if bits == 8 else torch.int16), device=device)
                  for k in names}
        return cls(pairs=torch.zeros(1, dtype=torch.int64, device=device),
                   count=torch.zeros(1, dtype=torch.int64, device=device), lag=lag, **planes)


class TraceMapInfo(C.Structure):
    """dbde_hip_trace_map_info_t (include/dbde_hip.h)."""
    _fields_ = [("W", C.c_int32), ("H", C.c_int32), ("n_labels", C.c_uint32), ("tiles", C.c_uint32),
                ("tiles_active", C.c_uint32), ("tiles_whole", C.c_uint32), ("tiles_mixed", C.c_uint32),
                ("reserved_", C.c_uint32), ("device_bytes", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "reserved_"}

    @classmethod
    def from_dict(cls, d):
        return cls(**{k: int(d[k]) for k, _ in cls._fields_ if k != "reserved_"})


class TracePlan(C.Structure):
    """dbde_hip_trace_plan_t (include/dbde_hip.h)."""
    _fields_ = [("chunks_per_frame", C.c_uint32), ("chunk_tiles", C.c_uint32), ("chunk_pieces", C.c_uint32),
                ("index_split", C.c_uint32), ("threads", C.c_uint32), ("tiles_per_workgroup", C.c_uint32),
                ("spans_x", C.c_uint32), ("spans", C.c_uint32), ("segments", C.c_uint32),
                ("frames_per_segment", C.c_uint32), ("grid", C.c_uint64), ("row_grid", C.c_uint64),
                ("workspace_bytes", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


def _labels_host(labels, n_labels):
    """A label image (numpy, or a torch tensor on any device) -> (contiguous int32 numpy (H, W), n_labels)."""
    if torch is not None and isinstance(labels, torch.Tensor):
        labels = labels.detach().cpu().numpy()
    a = np.asarray(labels)
    if a.ndim != 2:
        raise ValueError(f"labels must be a 2-D (H, W) array, not shape {a.shape}")
    if a.dtype.kind not in "iu":
        raise ValueError(f"labels must be integers, not {a.dtype}")
    lo, hi = (int(a.min()), int(a.max())) if a.size else (0, 0)
    if n_labels is None:
        n_labels = hi
    if lo < 0 or hi > int(n_labels):
        raise ValueError(f"labels must lie in [0, n_labels = {n_labels}], found [{lo}, {hi}]")
    if not 1 <= int(n_labels) <= 65535:
        raise ValueError(f"n_labels must lie in [1, 65535], not {n_labels}")
    return np.ascontiguousarray(a, dtype=np.int32), int(n_labels)


def trace_map_summary(labels, n_labels=None):
    """dbde_hip_trace_map_summary (host only): the trace map's tile classes and per-label pixel counts of a label image
    (H, W) with 0 = no region and 1..n_labels = region ids.  n_labels defaults to labels.max().  Returns the fields of
    dbde_hip_trace_map_info_t plus "pixels", an int64 numpy array (n_labels,).  Raises ValueError for labels outside
    [0, n_labels] or n_labels outside [1, 65535]."""
    a, L = _labels_host(labels, n_labels)
    info = TraceMapInfo()
    pixels = np.zeros(L, np.uint64)
    rc = lib().dbde_hip_trace_map_summary(a.ctypes.data, a.shape[1], a.shape[0], L, C.byref(info), pixels.ctypes.data)
    if rc != OK:
        raise ValueError(f"dbde_hip_trace_map_summary({a.shape[1]}, {a.shape[0]}, {L}) -> {rc}")
    d = info.as_dict()
    d["pixels"] = pixels.astype(np.int64)
    return d


def _trace_plan(fn, W, H, n_frames, info, stats, n_cu):
    if isinstance(info, TraceMap):
        info = info.info
    ti = TraceMapInfo.from_dict(info)
    pl = TracePlan()
    rc = getattr(lib(), fn)(W, H, n_frames, C.byref(ti), stats_mask(stats), n_cu, C.byref(pl))
    if rc != OK:
        raise ValueError(f"{fn}({W}, {H}, {n_frames}, {stats}, n_cu={n_cu}) -> {rc}")
    return pl.as_dict()


def trace_plan(W, H, n_frames, info, stats=("max", "min", "sum", "sumsq"), n_cu=256):
    """dbde_hip_trace_plan: the index geometry, trace launch and workspace of Codec.traces (host arithmetic only).
    info: a TraceMap, or the dict trace_map_summary / TraceMap.info returns.  Raises ValueError where dbde_hip_traces
    would return DBDE_HIP_ERR_ARG for these sizes."""
    return _trace_plan("dbde_hip_trace_plan", W, H, n_frames, info, stats, n_cu)


def trace16_plan(W, H, n_frames, info, stats=("max", "min", "sum", "sumsq"), n_cu=256):
    """dbde16_hip_trace_plan: trace_plan for DBDE16 traces (Codec.traces16)."""
    return _trace_plan("dbde16_hip_trace_plan", W, H, n_frames, info, stats, n_cu)


class TraceMap:
    """A label image classified into the device form dbde_hip_traces reads (Codec.trace_map).  .n_labels, .info (dict),
    .pixels (int64 device tensor (n_labels,): pixels per label), .close().  Holds its codec, and is closed before it."""

    def __init__(self, codec, labels, n_labels=None):
        a, L = _labels_host(labels, n_labels)
        self.codec = codec
        h = C.c_void_p()
        codec._check(codec.L.dbde_hip_trace_map_create(codec.h, a.ctypes.data, a.shape[1], a.shape[0], L, C.byref(h)),
                     "dbde_hip_trace_map_create")
        self.h = h
        self.n_labels = L
        info = TraceMapInfo()
        codec.L.dbde_hip_trace_map_info(h, C.byref(info))
        self.info = info.as_dict()
        self.W, self.H = a.shape[1], a.shape[0]
        # the counts the map holds (dbde_hip_trace_map_pixels), counted here from the same labels
        counts = np.bincount(a.reshape(-1), minlength=L + 1)[1:]
        pixels = torch.from_numpy(counts.astype(np.int64)).to(codec.device)
        self.pixels = pixels

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            self.codec.L.dbde_hip_trace_map_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Traces:
    """Device tensors of region traces (Codec.traces): max / min (n, L) uint8, sum / sumsq (n, L) int64, and pixels
    (L,) int64, the map's pixels per label.  Column j is label j + 1.  A statistic that was not asked for is None.
    Codec.traces16's max / min are int16 tensors holding the U16 bits."""

    def __init__(self, max=None, min=None, sum=None, sumsq=None, pixels=None):
        self.max, self.min, self.sum, self.sumsq, self.pixels = max, min, sum, sumsq, pixels

    @classmethod
    def empty(cls, n, L, stats, device, pix=1, pixels=None):
        """Uninitialised outputs for `stats`; pix: bytes per value of max / min (1: uint8, 2: int16 for DBDE16)."""
        mask = stats_mask(stats)
        if pix not in (1, 2):
            raise ValueError(f"pix must be 1 or 2, not {pix!r}")
        mm_dtype = torch.uint8 if pix == 1 else torch.int16
        mm = lambda: torch.empty((n, L), dtype=mm_dtype, device=device)      # noqa: E731
        i64 = lambda: torch.empty((n, L), dtype=torch.int64, device=device)   # noqa: E731
        return cls(mm() if mask & 1 else None, mm() if mask & 2 else None, i64() if mask & 4 else None,
                   i64() if mask & 8 else None, pixels)

    def mean(self):
        """Per-frame, per-label mean (float64, on the device); NaN for labels without pixels."""
        return self.sum.to(torch.float64) / self.pixels.to(torch.float64)

    def std(self):
        """Per-frame, per-label population standard deviation (float64, on the device); NaN for labels without pixels."""
        n = self.pixels.to(torch.float64)
        m = self.sum.to(torch.float64) / n
        return (self.sumsq.to(torch.float64) / n - m * m).clamp_(min=0.0).sqrt_()


HIST_OUTPUTS = {"rows": 1, "total": 2}


BINNED_STATS = {"sum": 1, "max": 2, "min": 4}


def binned_mask(stats):
    """("sum", "max", "min") names (or an int bitmask) -> dbde_hip_binned_plan's bitmask."""
    if isinstance(stats, int):
        return stats
    if isinstance(stats, str):
        stats = (stats,)
    mask = 0
    for name in stats:
        if name not in BINNED_STATS:
            raise ValueError(f"unknown statistic {name!r} (one of {sorted(BINNED_STATS)})")
        mask |= BINNED_STATS[name]
    return mask


class BinnedPlan(C.Structure):
    """dbde_hip_binned_plan_t (include/dbde_hip.h)."""
    _fields_ = [("tile_x", C.c_int32), ("tile_y", C.c_int32), ("tiles_x", C.c_int32), ("tiles_y", C.c_int32),
                ("chunks_per_frame", C.c_uint32), ("chunk_tiles", C.c_uint32), ("chunk_pieces", C.c_uint32),
                ("index_split", C.c_uint32), ("out_w", C.c_uint32), ("out_h", C.c_uint32), ("threads", C.c_uint32),
                ("pieces_x", C.c_uint32), ("lds_bytes", C.c_uint32), ("reserved_", C.c_uint32), ("grid", C.c_uint64),
                ("sum_bytes", C.c_uint64), ("max_bytes", C.c_uint64), ("min_bytes", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "reserved_"}


def _binned_plan(fn, W, H, n_frames, bin, x, y, rw, rh, stats):
    """binned_plan / binned16_plan through the C function named fn."""
    rw = W - x if rw is None else rw
    rh = H - y if rh is None else rh
    pl = BinnedPlan()
    rc = getattr(lib(), fn)(W, H, n_frames, x, y, rw, rh, bin, binned_mask(stats), C.byref(pl))
    if rc != OK:
        raise ValueError(f"{fn}({W}, {H}, {n_frames}, {x}, {y}, {rw}, {rh}, bin={bin}, stats={stats!r}) -> {rc}")
    return pl.as_dict()


def binned_plan(W, H, n_frames, bin, x=0, y=0, rw=None, rh=None, stats=("sum",)):
    """dbde_hip_binned_plan: the tile window, index geometry, plane shape and bytes, launch and LDS of
    Codec.decode_binned (host arithmetic only).  rw / rh default to the rest of the frame.  Raises ValueError where
    dbde_hip_decode_binned would return DBDE_HIP_ERR_ARG."""
    return _binned_plan("dbde_hip_binned_plan", W, H, n_frames, bin, x, y, rw, rh, stats)


def binned16_plan(W, H, n_frames, bin, x=0, y=0, rw=None, rh=None, stats=("sum",)):
    """dbde16_hip_binned_plan: binned_plan for DBDE16 frames (Codec.decode_binned16)."""
    return _binned_plan("dbde16_hip_binned_plan", W, H, n_frames, bin, x, y, rw, rh, stats)


OUT_F32, OUT_F16, OUT_BF16 = 0, 1, 2   # DBDE_HIP_OUT_* (include/dbde_hip.h)


def _scaled_type(dtype):
    """torch.float32 / float16 / bfloat16 -> (DBDE_HIP_OUT_*, torch dtype)."""
    table = {torch.float32: OUT_F32, torch.float16: OUT_F16, torch.bfloat16: OUT_BF16}
    if dtype in table:
        return table[dtype], dtype
    raise ValueError(f"unknown output type {dtype!r} (torch.float32, torch.float16 or torch.bfloat16)")


class ScaledPlan(C.Structure):
    """dbde_hip_scaled_plan_t (include/dbde_hip.h)."""
    _fields_ = [("tile_x", C.c_int32), ("tile_y", C.c_int32), ("tiles_x", C.c_int32), ("tiles_y", C.c_int32),
                ("max_tiles_x", C.c_int32), ("max_tiles_y", C.c_int32), ("chunks_per_frame", C.c_uint32),
                ("chunk_tiles", C.c_uint32), ("chunk_pieces", C.c_uint32), ("index_split", C.c_uint32),
                ("threads", C.c_uint32), ("pieces_x", C.c_uint32), ("lds_bytes", C.c_uint32), ("elem_bytes", C.c_uint32),
                ("grid", C.c_uint64), ("grid_origins", C.c_uint64), ("out_bytes", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


def _scaled_plan(fn, W, H, n_frames, x, y, rw, rh, dtype):
    """scaled_plan / scaled16_plan through the C function named fn."""
    rw = W - x if rw is None else rw
    rh = H - y if rh is None else rh
    out_type = dtype if isinstance(dtype, int) and not isinstance(dtype, bool) else _scaled_type(dtype)[0]
    pl = ScaledPlan()
    rc = getattr(lib(), fn)(W, H, n_frames, x, y, rw, rh, out_type, C.byref(pl))
    if rc != OK:
        raise ValueError(f"{fn}({W}, {H}, {n_frames}, {x}, {y}, {rw}, {rh}, type={out_type}) -> {rc}")
    return pl.as_dict()


def scaled_plan(W, H, n_frames, x=0, y=0, rw=None, rh=None, dtype=OUT_F32):
    """dbde_hip_scaled_plan: the tile window, index geometry, launch, LDS and output bytes of Codec.decode_scaled (host
    arithmetic only).  rw / rh default to the rest of the frame; dtype: a torch dtype or a DBDE_HIP_OUT_* value.
    Raises ValueError where dbde_hip_decode_scaled would return DBDE_HIP_ERR_ARG."""
    return _scaled_plan("dbde_hip_scaled_plan", W, H, n_frames, x, y, rw, rh, dtype)


def scaled16_plan(W, H, n_frames, x=0, y=0, rw=None, rh=None, dtype=OUT_F32):
    """dbde16_hip_scaled_plan: scaled_plan for DBDE16 frames (Codec.decode_scaled16)."""
    return _scaled_plan("dbde16_hip_scaled_plan", W, H, n_frames, x, y, rw, rh, dtype)


MASK_INSIDE, MASK_OUTSIDE = 0, 1   # DBDE_HIP_MASK_* (include/dbde_hip.h)


class MaskPlan(C.Structure):
    """dbde_hip_mask_plan_t (include/dbde_hip.h)."""
    _fields_ = [("tile_x", C.c_int32), ("tile_y", C.c_int32), ("tiles_x", C.c_int32), ("tiles_y", C.c_int32),
                ("max_tiles_x", C.c_int32), ("max_tiles_y", C.c_int32), ("chunks_per_frame", C.c_uint32),
                ("chunk_tiles", C.c_uint32), ("chunk_pieces", C.c_uint32), ("index_split", C.c_uint32),
                ("threads", C.c_uint32), ("pieces_x", C.c_uint32), ("piece_words", C.c_uint32), ("lds_bytes", C.c_uint32),
                ("words", C.c_uint32), ("pieces_x_fixed", C.c_uint32), ("piece_words_fixed", C.c_uint32),
                ("reserved", C.c_uint32),
                ("grid", C.c_uint64), ("grid_origins", C.c_uint64), ("mask_bytes", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "reserved"}


def _mask_plan(fn, W, H, n_frames, x, y, rw, rh):
    """mask_plan / mask16_plan through the C function named fn."""
    rw = W - x if rw is None else rw
    rh = H - y if rh is None else rh
    pl = MaskPlan()
    rc = getattr(lib(), fn)(W, H, n_frames, x, y, rw, rh, C.byref(pl))
    if rc != OK:
        raise ValueError(f"{fn}({W}, {H}, {n_frames}, {x}, {y}, {rw}, {rh}) -> {rc}")
    return pl.as_dict()


def mask_plan(W, H, n_frames, x=0, y=0, rw=None, rh=None):
    """dbde_hip_mask_plan: the tile window, index geometry, launch, LDS, words per row and mask bytes of
    Codec.decode_mask (host arithmetic only).  rw / rh default to the rest of the frame.  Raises ValueError where
    dbde_hip_decode_mask would return DBDE_HIP_ERR_ARG for its sizes and window."""
    return _mask_plan("dbde_hip_mask_plan", W, H, n_frames, x, y, rw, rh)


def mask16_plan(W, H, n_frames, x=0, y=0, rw=None, rh=None):
    """dbde16_hip_mask_plan: mask_plan for DBDE16 frames (Codec.decode_mask16)."""
    return _mask_plan("dbde16_hip_mask_plan", W, H, n_frames, x, y, rw, rh)


class Mask:
    """Device tensors of a mask decode (Codec.decode_mask): bits (int64, (n, rh, words), words = ceil(rw / 64)) holds
    bit (c & 63) of word (c >> 6) of row r for window pixel (r, c), the bits at and beyond rw being 0; counts (int32,
    (n,)) the set bits per frame; boxes (int32, (n, 4)) x_min, y_min, x_max, y_max of the set bits in window
    coordinates, inclusive, (rw, rh, -1, -1) for a frame with none.  An output that was not asked for is None."""

    def __init__(self, bits=None, counts=None, boxes=None, rw=None):
        self.bits, self.counts, self.boxes, self.rw = bits, counts, boxes, rw

    @classmethod
    def empty(cls, n, rh, rw, device, bits=True, counts=True, boxes=False):
        """Zeroed outputs (a rejected frame's words then read 0)."""
        words = -(-rw // 64)
        return cls(torch.zeros((n, rh, words), dtype=torch.int64, device=device) if bits else None,
                   torch.zeros((n,), dtype=torch.int32, device=device) if counts else None,
                   torch.zeros((n, 4), dtype=torch.int32, device=device) if boxes else None, rw=rw)

    def unpack(self):
        """The mask as a bool tensor (n, rh, rw)."""
        n, rh, words = self.bits.shape
        sh = torch.arange(64, dtype=torch.int64, device=self.bits.device)
        return ((self.bits.unsqueeze(-1) >> sh) & 1).to(torch.bool).reshape(n, rh, words * 64)[:, :, :self.rw]


def band_from_background(bg, below, above=None):
    """(lo, hi) maps in bg's dtype for Codec.decode_mask(..., outside=True): lo = clamp(bg - below), hi = clamp(bg +
    above) (above defaults to below), so that the set bits are the pixels with p < bg - below or p > bg + above.  bg:
    uint8 (DBDE) or int16 holding the U16 bits (DBDE16, as decode_frames16 returns its images)."""
    above = below if above is None else above
    if bg.dtype == torch.uint8:
        v, top = bg.to(torch.int32), 255
    elif bg.dtype == torch.int16:
        v, top = bg.to(torch.int32) & 0xFFFF, 65535
    else:
        raise ValueError(f"bg must be uint8 or int16 (U16 bits), not {bg.dtype}")
    lo, hi = (v - int(below)).clamp(0, top), (v + int(above)).clamp(0, top)
    if bg.dtype == torch.uint8:
        return lo.to(torch.uint8).contiguous(), hi.to(torch.uint8).contiguous()
    as16 = lambda t: torch.where(t > 32767, t - 65536, t).to(torch.int16).contiguous()   # noqa: E731
    return as16(lo), as16(hi)


PATCH_CLAMP, PATCH_FILL = 0, 1   # DBDE_HIP_PATCH_* (include/dbde_hip.h)


def patch_edge_mode(edge):
    """"clamp" / "fill" (or DBDE_HIP_PATCH_CLAMP / _FILL as an int) -> the C-ABI's edge mode."""
    if isinstance(edge, str):
        if edge not in ("clamp", "fill"):
            raise ValueError(f"edge must be 'clamp' or 'fill', not {edge!r}")
        return PATCH_CLAMP if edge == "clamp" else PATCH_FILL
    return int(edge)


class PatchPlan(C.Structure):
    """dbde_hip_patches_plan_t (include/dbde_hip.h)."""
    _fields_ = [("max_tiles_x", C.c_int32), ("max_tiles_y", C.c_int32), ("rows_per_workgroup", C.c_uint32),
                ("groups_per_patch", C.c_uint32), ("threads", C.c_uint32), ("chunks_per_frame", C.c_uint32),
                ("chunk_tiles", C.c_uint32), ("chunk_pieces", C.c_uint32), ("index_split", C.c_uint32),
                ("lds_bytes", C.c_uint32), ("grid", C.c_uint64), ("out_bytes", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


def _patches_plan(fn, W, H, n_frames, pw, ph, n_patches, edge):
    """patches_plan / patches16_plan through the C function named fn."""
    pl = PatchPlan()
    rc = getattr(lib(), fn)(W, H, n_frames, pw, ph, n_patches, patch_edge_mode(edge), C.byref(pl))
    if rc != OK:
        raise ValueError(f"{fn}({W}, {H}, {n_frames}, {pw}, {ph}, {n_patches}, {edge}) -> {rc}")
    return pl.as_dict()


def patches_plan(W, H, n_frames, pw, ph, n_patches, edge="clamp"):
    """dbde_hip_patches_plan: the tiles a patch can span, the tile rows per workgroup, the workgroups per patch, the
    index geometry, the grid and the output bytes of Codec.decode_patches (host arithmetic only).  Raises ValueError
    where dbde_hip_decode_patches would return DBDE_HIP_ERR_ARG for its sizes and edge mode."""
    return _patches_plan("dbde_hip_patches_plan", W, H, n_frames, pw, ph, n_patches, edge)


def patches16_plan(W, H, n_frames, pw, ph, n_patches, edge="clamp"):
    """dbde16_hip_patches_plan: patches_plan for DBDE16 frames (Codec.decode_patches16)."""
    return _patches_plan("dbde16_hip_patches_plan", W, H, n_frames, pw, ph, n_patches, edge)


def origins_from_centres(centres, pw, ph):
    """Patch origins from object centres: (n, K, 2) float or int (x, y) centres -> int32 origins of the same shape,
    origin = floor(c + 0.5) - p // 2 per axis (p = pw for x, ph for y): the centre is rounded half up to a pixel, and
    that pixel is column pw // 2, row ph // 2 of the patch -- the middle pixel of an odd size, the one right of / below
    the middle of an even size.  Results outside int32 are clamped to it (decode_patches treats such origins as far
    outside the frame).  centres: a torch tensor (the origins stay on its device) or anything numpy takes."""
    if torch.is_tensor(centres):
        c = centres
        if c.dim() != 3 or c.shape[2] != 2:
            raise ValueError("centres must have shape (n, K, 2)")
        half = torch.tensor([pw // 2, ph // 2], dtype=torch.int64, device=c.device)
        r = torch.floor(c.to(torch.float64) + 0.5).to(torch.int64) if c.is_floating_point() else c.to(torch.int64)
        return (r - half).clamp(-2 ** 31, 2 ** 31 - 1).to(torch.int32).contiguous()
    c = np.asarray(centres)
    if c.ndim != 3 or c.shape[2] != 2:
        raise ValueError("centres must have shape (n, K, 2)")
    r = np.floor(c.astype(np.float64) + 0.5).astype(np.int64) if c.dtype.kind == "f" else c.astype(np.int64)
    return np.ascontiguousarray(np.clip(r - np.array([pw // 2, ph // 2], np.int64), -2 ** 31, 2 ** 31 - 1).astype(np.int32))


MOMENT_COUNT, MOMENT_VALUE, MOMENT_ABOVE, MOMENT_BELOW = 0, 1, 2, 3   # DBDE_HIP_MOMENT_* (include/dbde_hip.h)
MOMENT_WEIGHTS = {"count": MOMENT_COUNT, "value": MOMENT_VALUE, "above": MOMENT_ABOVE, "below": MOMENT_BELOW}


def moment_weight_mode(weight):
    """"count" / "value" / "above" / "below" (or DBDE_HIP_MOMENT_* as an int) -> the C-ABI's weight mode."""
    if isinstance(weight, str):
        if weight not in MOMENT_WEIGHTS:
            raise ValueError(f"weight must be one of {sorted(MOMENT_WEIGHTS)}, not {weight!r}")
        return MOMENT_WEIGHTS[weight]
    return int(weight)


class PatchMomentsPlan(C.Structure):
    """dbde_hip_patch_moments_plan_t (include/dbde_hip.h)."""
    _fields_ = [("max_tiles_x", C.c_int32), ("max_tiles_y", C.c_int32), ("rows_per_workgroup", C.c_uint32),
                ("steps_per_patch", C.c_uint32), ("threads", C.c_uint32), ("chunks_per_frame", C.c_uint32),
                ("chunk_tiles", C.c_uint32), ("chunk_pieces", C.c_uint32), ("index_split", C.c_uint32),
                ("lds_bytes", C.c_uint32), ("grid", C.c_uint64), ("moments_bytes", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


def _patch_moments_plan(fn, W, H, n_frames, pw, ph, n_patches, edge):
    """patch_moments_plan / patch_moments16_plan through the C function named fn."""
    pl = PatchMomentsPlan()
    rc = getattr(lib(), fn)(W, H, n_frames, pw, ph, n_patches, patch_edge_mode(edge), C.byref(pl))
    if rc != OK:
        raise ValueError(f"{fn}({W}, {H}, {n_frames}, {pw}, {ph}, {n_patches}, {edge}) -> {rc}")
    return pl.as_dict()


def patch_moments_plan(W, H, n_frames, pw, ph, n_patches, edge="clamp"):
    """dbde_hip_patch_moments_plan: the tiles a patch can span, the tile rows per step and the steps one workgroup
    walks per patch, the index geometry, the grid and the bytes of moments of Codec.patch_moments (host arithmetic
    only).  Raises ValueError where dbde_hip_patch_moments would return DBDE_HIP_ERR_ARG for its sizes and edge mode."""
    return _patch_moments_plan("dbde_hip_patch_moments_plan", W, H, n_frames, pw, ph, n_patches, edge)


def patch_moments16_plan(W, H, n_frames, pw, ph, n_patches, edge="clamp"):
    """dbde16_hip_patch_moments_plan: patch_moments_plan for DBDE16 frames (Codec.patch_moments16)."""
    return _patch_moments_plan("dbde16_hip_patch_moments_plan", W, H, n_frames, pw, ph, n_patches, edge)


class PatchMoments:
    """What Codec.patch_moments returns: per frame and patch the eight sums over the selected pixels,
    moments[f, k] = (N, S, Sx, Sy, Sxx, Sxy, Syy, Sww) as int64 (n, K, 8) in PATCH coordinates (column j, row i); bbox
    (optional) int32 (n, K, 4) = (j_min, i_min, j_max, i_max), (pw, ph, -1, -1) where nothing is selected; used int32
    (n, K, 2), the origins the patches were taken at.  Entries of rejected frames and of patches beyond a frame's count
    hold whatever the tensors held before the call.  The derived quantities are float64 torch tensors on the moments'
    device (numpy arrays work the same way through PatchMoments(torch.from_numpy(...), ...))."""

    def __init__(self, moments, bbox, used, pw, ph):
        self.moments, self.bbox, self.used, self.pw, self.ph = moments, bbox, used, int(pw), int(ph)

    def count(self):
        """N: the selected pixels, int64 (n, K)."""
        return self.moments[..., 0]

    def mass(self):
        """S: the sum of the weights, int64 (n, K)."""
        return self.moments[..., 1]

    def _means(self):
        m = self.moments.to(torch.float64)
        S = m[..., 1]
        S = torch.where(S == 0, torch.full_like(S, float("nan")), S)
        return m, S, m[..., 2] / S, m[..., 3] / S

    def centroid(self):
        """(n, K, 2) float64 (x, y) in FRAME coordinates: used + (Sx / S, Sy / S); NaN where S = 0."""
        _, _, mx, my = self._means()
        return torch.stack((mx, my), dim=-1) + self.used.to(torch.float64)

    def covariance(self):
        """(n, K, 2, 2) float64 [[cxx, cxy], [cxy, cyy]]: the central second moments over S, cxx = Sxx / S - (Sx / S)^2,
        cxy = Sxy / S - (Sx / S)(Sy / S), cyy = Syy / S - (Sy / S)^2; NaN where S = 0."""
        m, S, mx, my = self._means()
        cxx, cxy, cyy = m[..., 4] / S - mx * mx, m[..., 5] / S - mx * my, m[..., 6] / S - my * my
        return torch.stack((torch.stack((cxx, cxy), dim=-1), torch.stack((cxy, cyy), dim=-1)), dim=-2)

    def orientation(self):
        """(angle, major, minor), float64 (n, K) each: the angle of the major axis against the x axis in radians, in
        (-pi/2, pi/2], 0.5 atan2(2 cxy, cxx - cyy), and the axis lengths 2 sqrt(eigenvalue) of the covariance (the
        semi-axes of a uniformly filled ellipse); NaN where S = 0."""
        c = self.covariance()
        cxx, cxy, cyy = c[..., 0, 0], c[..., 0, 1], c[..., 1, 1]
        half, diff = (cxx + cyy) / 2, (cxx - cyy) / 2
        root = torch.sqrt(diff * diff + cxy * cxy)
        angle = 0.5 * torch.atan2(2 * cxy, cxx - cyy)
        return angle, 2 * torch.sqrt(half + root), 2 * torch.sqrt(torch.clamp(half - root, min=0))


MATCH_PROD, MATCH_SUM, MATCH_SQ = 1, 2, 4   # DBDE_HIP_MATCH_* (include/dbde_hip.h)
MATCH_STATS = {"prod": MATCH_PROD, "sum": MATCH_SUM, "sq": MATCH_SQ}
MATCH_MAX_TEMPLATE, MATCH_MAX_RADIUS = 128, 16


def match_mask(stats):
    """("prod", "sum", "sq") names (or a DBDE_HIP_MATCH_* mask as an int) -> the C-ABI's mask of surfaces."""
    if isinstance(stats, int):
        return stats
    m = 0
    for s in stats:
        if s not in MATCH_STATS:
            raise ValueError(f"stats must be among {sorted(MATCH_STATS)}, not {s!r}")
        m |= MATCH_STATS[s]
    return m


class MatchPlan(C.Structure):
    """dbde_hip_match_plan_t (include/dbde_hip.h)."""
    _fields_ = [("pw", C.c_int32), ("ph", C.c_int32), ("D", C.c_int32), ("max_tiles_x", C.c_int32),
                ("max_tiles_y", C.c_int32), ("rows_per_wave", C.c_uint32), ("decode_waves", C.c_uint32),
                ("steps_per_patch", C.c_uint32), ("row_slices", C.c_uint32), ("threads", C.c_uint32),
                ("chunks_per_frame", C.c_uint32), ("chunk_tiles", C.c_uint32), ("chunk_pieces", C.c_uint32),
                ("index_split", C.c_uint32), ("lds_bytes", C.c_uint32), ("grid", C.c_uint64), ("surface_bytes", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


def _match_plan(fn, W, H, n_frames, tw, th, S, n_patches, n_templates, edge, fill, stats):
    """match_plan / match16_plan through the C function named fn.  What ctypes would take modulo 2^32 is refused here."""
    mask = match_mask(stats)
    what = f"{fn}({W}, {H}, {n_frames}, {tw}x{th}, S={S}, {n_patches}, {n_templates}, {edge}, fill={fill}, stats={stats})"
    if not (0 <= int(fill) < 2 ** 32 and 0 <= mask < 2 ** 32):
        raise ValueError(f"{what}: fill or stats out of range")
    pl = MatchPlan()
    rc = getattr(lib(), fn)(W, H, n_frames, tw, th, S, n_patches, n_templates if n_templates is not None else n_patches,
                            patch_edge_mode(edge), int(fill), mask, C.byref(pl))
    if rc != OK:
        raise ValueError(f"{what} -> {rc}")
    return pl.as_dict()


def match_plan(W, H, n_frames, tw, th, S, n_patches, n_templates=None, edge="clamp", fill=0, stats=("prod", "sum", "sq")):
    """dbde_hip_match_plan: the search patch and surface sizes, the tiles a search patch can span, the decoding waves and
    steps, the row slices, the index geometry, LDS, grid and the bytes of one surface of Codec.match_patches (host
    arithmetic only).  n_templates: 1 or n_patches (the default).  Raises ValueError where dbde_hip_match_patches would
    return DBDE_HIP_ERR_ARG for these arguments."""
    return _match_plan("dbde_hip_match_plan", W, H, n_frames, tw, th, S, n_patches, n_templates, edge, fill, stats)


def match16_plan(W, H, n_frames, tw, th, S, n_patches, n_templates=None, edge="clamp", fill=0, stats=("prod", "sum", "sq")):
    """dbde16_hip_match_plan: match_plan for DBDE16 frames (Codec.match_patches16)."""
    return _match_plan("dbde16_hip_match_plan", W, H, n_frames, tw, th, S, n_patches, n_templates, edge, fill, stats)


def best_shift(score, S, maximize=True):
    """The best entry of score surfaces (..., D, D), D = 2S + 1, row dy + S, column dx + S: the arg-max (maximize=False:
    the arg-min), NaN never winning; ties go to the smallest |dx| + |dy|, then the smallest dy, then the smallest dx.
    Returns (shifts int64 (..., 2) as (dx, dy), the score there); an all-NaN surface gives (0, 0) and NaN."""
    D = 2 * S + 1
    if score.shape[-2:] != (D, D):
        raise ValueError(f"score surfaces must end in ({D}, {D})")
    flat = score.reshape(*score.shape[:-2], D * D)
    off = torch.arange(D, device=score.device, dtype=torch.int64) - S
    dy, dx = off[:, None].expand(D, D).reshape(-1), off[None, :].expand(D, D).reshape(-1)
    rank = ((dx.abs() + dy.abs()) * D + (dy + S)) * D + (dx + S)
    if flat.is_floating_point():
        valid = ~torch.isnan(flat)
        worst = float("-inf") if maximize else float("inf")
        s = torch.where(valid, flat, torch.full_like(flat, worst))
    else:
        valid = torch.ones_like(flat, dtype=torch.bool)
        s = flat
    top = (s.max(-1, keepdim=True).values if maximize else s.min(-1, keepdim=True).values)
    cand = (s == top) & valid
    pick = torch.where(cand, rank, torch.full_like(rank, 4 * D * D * D)).argmin(-1)
    none = ~cand.any(-1)
    pick = torch.where(none, torch.full_like(pick, S * D + S), pick)
    shifts = torch.stack((dx[pick], dy[pick]), dim=-1)
    value = flat.gather(-1, pick[..., None])[..., 0]
    if flat.is_floating_point():
        value = torch.where(none, torch.full_like(value, float("nan")), value)
    return shifts, value


class PatchMatch:
    """What Codec.match_patches returns: per frame and patch the D x D surfaces over the shifts -S..S (row dy + S, column
    dx + S) as int64 (n, K, D, D): prod = sum T P, sum = sum P, sq = sum P^2 over the template's footprint at that shift
    (None where not requested); used int32 (n, K, 2), the search patches' used origins; t_sum and t_sq int64 (Kt,), the
    templates' own sum T and sum T^2 (Kt = 1 or K).  Entries of rejected frames and of patches beyond a frame's count
    hold whatever the tensors held before the call.  The derived quantities are torch tensors on the surfaces' device."""

    def __init__(self, prod, sum, sq, used, t_sum, t_sq, tw, th, S):
        self.prod, self.sum, self.sq, self.used, self.t_sum, self.t_sq = prod, sum, sq, used, t_sum, t_sq
        self.tw, self.th, self.S = int(tw), int(th), int(S)

    def _need(self, *names):
        for nm in names:
            if getattr(self, nm) is None:
                raise ValueError(f"the surface {nm!r} was not requested")

    def ssd(self):
        """sum (T - P)^2 = sum T^2 - 2 prod + sq, int64 (n, K, D, D), exact."""
        self._need("prod", "sq")
        return self.t_sq.view(1, -1, 1, 1) - 2 * self.prod + self.sq

    def zncc(self):
        """The zero-mean normalised cross-correlation, float64 (n, K, D, D), from the exact integers: with N = tw th,
        (N prod - sum T sum) / sqrt((N sum T^2 - (sum T)^2) (N sq - sum^2)); NaN where the denominator is 0 (a flat
        template or a flat footprint)."""
        self._need("prod", "sum", "sq")
        N = self.tw * self.th
        ts, tq = self.t_sum.view(1, -1, 1, 1), self.t_sq.view(1, -1, 1, 1)
        num = (N * self.prod - ts * self.sum).to(torch.float64)        # below 2^61: exact in int64
        var_t = (N * tq - ts * ts).to(torch.float64)
        var_p = (N * self.sq - self.sum * self.sum).to(torch.float64)
        den = torch.sqrt(var_t * var_p)
        return torch.where(den == 0, torch.full_like(den, float("nan")), num / den)

    def _score(self, score):
        if score == "zncc":
            return self.zncc(), True
        if score == "ssd":
            return self.ssd(), False
        raise ValueError("score must be 'zncc' or 'ssd'")

    def best(self, score="zncc"):
        """(shifts int64 (n, K, 2) as (dx, dy), score (n, K)): the arg-max of zncc (NaN never wins) or the arg-min of
        ssd; ties go to the smallest |dx| + |dy|, then the smallest dy, then the smallest dx; an all-NaN surface gives
        (0, 0) and NaN."""
        s, up = self._score(score)
        return best_shift(s, self.S, maximize=up)

    def refine(self, score="zncc"):
        """best's shifts plus the three-point parabolic sub-pixel offset per axis around the best entry, float64
        (n, K, 2): with l, c, r the scores left of, at and right of the best, 0.5 (l - r) / (l - 2 c + r); 0 on the
        border of the surface, and where a neighbour is NaN or the three lie on a line."""
        s, up = self._score(score)
        shifts, _ = best_shift(s, self.S, maximize=up)
        s = s.to(torch.float64)
        D = 2 * self.S + 1
        col, row = shifts[..., 0] + self.S, shifts[..., 1] + self.S

        def at(r, c):
            idx = (r.clamp(0, D - 1) * D + c.clamp(0, D - 1))[..., None]
            return s.reshape(*s.shape[:-2], D * D).gather(-1, idx)[..., 0]

        out = []
        for lo, hi, pos in ((at(row, col - 1), at(row, col + 1), col), (at(row - 1, col), at(row + 1, col), row)):
            c = at(row, col)
            den = lo - 2 * c + hi
            off = 0.5 * (lo - hi) / den
            ok = (pos > 0) & (pos < D - 1) & torch.isfinite(off)
            out.append(torch.where(ok, off, torch.zeros_like(off)))
        return shifts.to(torch.float64) + torch.stack(out, dim=-1)


class CropPlan(C.Structure):
    """dbde_hip_crop_plan_t (include/dbde_hip.h)."""
    _fields_ = [("tile_x", C.c_int32), ("tile_y", C.c_int32), ("tiles_x", C.c_int32), ("tiles_y", C.c_int32),
                ("out_tiles", C.c_uint32), ("recoded_tiles", C.c_uint32),
                ("chunks_per_frame", C.c_uint32), ("chunk_tiles", C.c_uint32), ("chunk_pieces", C.c_uint32),
                ("index_split", C.c_uint32),
                ("size_threads", C.c_uint32), ("size_lds_bytes", C.c_uint32),
                ("repack_threads", C.c_uint32), ("repack_lds_bytes", C.c_uint32),
                ("rows_threads", C.c_uint32), ("rows_lds_bytes", C.c_uint32),
                ("place_threads", C.c_uint32), ("place_lds_bytes", C.c_uint32),
                ("copy_threads", C.c_uint32), ("copy_lds_bytes", C.c_uint32),
                ("size_grid", C.c_uint64), ("rows_grid", C.c_uint64), ("place_grid", C.c_uint64),
                ("copy_grid", C.c_uint64), ("repack_grid", C.c_uint64), ("max_out_frame_bytes", C.c_uint64), ("out_capacity", C.c_uint64),
                ("workspace_bytes", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


def _crop_plan(fn, W, H, n_frames, x, y, rw, rh, slot_stride):
    """crop_plan / crop16_plan through the C function named fn."""
    rw = W - x if rw is None else rw
    rh = H - y if rh is None else rh
    pl = CropPlan()
    rc = getattr(lib(), fn)(W, H, n_frames, x, y, rw, rh, slot_stride, C.byref(pl))
    if rc != OK:
        raise ValueError(f"{fn}({W}, {H}, {n_frames}, {x}, {y}, {rw}, {rh}, slot_stride={slot_stride}) -> {rc}")
    return pl.as_dict()


def crop_plan(W, H, n_frames, x=0, y=0, rw=None, rh=None, slot_stride=0):
    """dbde_hip_crop_plan: the tile window, output size and capacity, index geometry, launches, LDS and workspace of
    Codec.crop_frames (host arithmetic only).  rw / rh default to the rest of the frame.  Raises ValueError where
    dbde_hip_crop_frames would return DBDE_HIP_ERR_ARG."""
    return _crop_plan("dbde_hip_crop_plan", W, H, n_frames, x, y, rw, rh, slot_stride)


def crop16_plan(W, H, n_frames, x=0, y=0, rw=None, rh=None, slot_stride=0):
    """dbde16_hip_crop_plan: crop_plan for DBDE16 frames (Codec.crop_frames16)."""
    return _crop_plan("dbde16_hip_crop_plan", W, H, n_frames, x, y, rw, rh, slot_stride)


class WindowEncodePlan(C.Structure):
    """dbde_hip_window_encode_plan_t (include/dbde_hip.h)."""
    _fields_ = [("forwards", C.c_uint32), ("tiles_x", C.c_uint32), ("tiles_y", C.c_uint32), ("tiles", C.c_uint32),
                ("lanes_per_row", C.c_uint32), ("chunks_per_frame", C.c_uint32), ("chunk_tiles", C.c_uint32),
                ("record_group", C.c_uint32), ("threads", C.c_uint32), ("lds_bytes", C.c_uint32),
                ("grid", C.c_uint64), ("pitch", C.c_uint64), ("frame_stride", C.c_uint64),
                ("min_image_bytes", C.c_uint64), ("max_out_frame_bytes", C.c_uint64), ("out_capacity", C.c_uint64),
                ("workspace_bytes", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


def _window_encode_plan(fn, pix, W, H, n_frames, x, y, rw, rh, pitch, frame_stride, image_bytes, image_address,
                        has_origins, out_capacity, slot_stride, n_cu):
    """window_encode_plan / window_encode16_plan through the C function named fn."""
    rw = W - x if rw is None else rw
    rh = H - y if rh is None else rh
    if image_bytes is None:   # the least extent of this layout
        pt = pitch or W * pix
        image_bytes = max(n_frames - 1, 0) * (frame_stride or H * pt) + (H - 1) * pt + W * pix if n_frames else 0
    pl = WindowEncodePlan()
    rc = getattr(lib(), fn)(image_address, image_bytes, W, H, pitch, frame_stride, n_frames, x, y, rw, rh,
                            1 if has_origins else 0, out_capacity, slot_stride, n_cu, C.byref(pl))
    if rc != OK:
        raise ValueError(f"{fn}({W}, {H}, pitch={pitch}, frame_stride={frame_stride}, image_bytes={image_bytes}, "
                         f"n={n_frames}, window {rw}x{rh} at {x},{y}, slot_stride={slot_stride}) -> {rc}")
    return pl.as_dict()


def window_encode_plan(W, H, n_frames, x=0, y=0, rw=None, rh=None, pitch=0, frame_stride=0, image_bytes=None,
                       image_address=0, has_origins=False, out_capacity=0, slot_stride=0, n_cu=256):
    """dbde_hip_window_encode_plan: whether Codec.encode_window forwards to encode_frames, else the window's tiles,
    chunks, workgroup, grid, LDS and workspace, and the least image_bytes / out_capacity (host arithmetic only).
    pitch / frame_stride in bytes, 0 = compact; image_bytes None = the least extent; out_capacity 0 = not checked.
    Raises ValueError where dbde_hip_encode_window would return an error."""
    return _window_encode_plan("dbde_hip_window_encode_plan", 1, W, H, n_frames, x, y, rw, rh, pitch, frame_stride,
                               image_bytes, image_address, has_origins, out_capacity, slot_stride, n_cu)


def window_encode16_plan(W, H, n_frames, x=0, y=0, rw=None, rh=None, pitch=0, frame_stride=0, image_bytes=None,
                         image_address=0, has_origins=False, out_capacity=0, slot_stride=0, n_cu=256):
    """dbde16_hip_window_encode_plan: window_encode_plan for U16 sources (Codec.encode_window16)."""
    return _window_encode_plan("dbde16_hip_window_encode_plan", 2, W, H, n_frames, x, y, rw, rh, pitch, frame_stride,
                               image_bytes, image_address, has_origins, out_capacity, slot_stride, n_cu)


def bin_pixels(rh, rw, bin, device=None):
    """int32 (ceil(rh / bin), ceil(rw / bin)): the pixels of each bin of an rw x rh window; bin * bin except in the
    last row and column, whose bins end at the window's edge."""
    ny = torch.arange(0, rh, bin, dtype=torch.int32, device=device).neg_().add_(rh).clamp_(max=bin)
    nx = torch.arange(0, rw, bin, dtype=torch.int32, device=device).neg_().add_(rw).clamp_(max=bin)
    return ny[:, None] * nx[None, :]


class Binned:
    """Device tensors of a binned decode (Codec.decode_binned): per frame, the sum / max / min of every bin x bin block
    of the window, each (n, oh, ow).  DBDE: sum int16 (at most 64 * 255), max / min uint8.  DBDE16: sum int32 (at most
    64 * 65535), max / min int16 tensors holding the U16 bits (as decode_frames16 returns its images).  A statistic that
    was not asked for is None.  bin is the bin's side; pixels (int32, (oh, ow)) each bin's pixel count: bin * bin
    except on the window's right and bottom edge."""

    def __init__(self, sum=None, max=None, min=None, bin=None, pixels=None):
        self.sum, self.max, self.min, self.bin, self.pixels = sum, max, min, bin, pixels

    @classmethod
    def empty(cls, n, rh, rw, bin, stats, device, pix=1):
        """Zeroed outputs for `stats` (a rejected frame's planes then read 0); pix: bytes per pixel (1: DBDE, 2: DBDE16)."""
        mask = binned_mask(stats)
        if pix not in (1, 2):
            raise ValueError(f"pix must be 1 or 2, not {pix!r}")
        if bin not in (2, 4, 8):
            raise ValueError(f"bin must be 2, 4 or 8, not {bin!r}")
        oh, ow = -(-rh // bin), -(-rw // bin)
        sum_dtype, mm_dtype = (torch.int16, torch.uint8) if pix == 1 else (torch.int32, torch.int16)
        plane = lambda dt: torch.zeros((n, oh, ow), dtype=dt, device=device)   # noqa: E731
        return cls(plane(sum_dtype) if mask & 1 else None, plane(mm_dtype) if mask & 2 else None,
                   plane(mm_dtype) if mask & 4 else None, bin=bin, pixels=bin_pixels(rh, rw, bin, device))

    def mean(self):
        """Per-bin mean (float32, (n, oh, ow)): sum / pixels."""
        return self.sum.to(torch.float32) / self.pixels.to(torch.float32)


def max_bins(pix, shift=0):
    """The most bins a histogram may have: 256 >> shift (DBDE, pix 1), min(4096, 65536 >> shift) (DBDE16, pix 2)."""
    return (256 >> shift) if pix == 1 else min(4096, 65536 >> shift)


class HistogramPlan(C.Structure):
    """dbde_hip_histogram_plan_t (include/dbde_hip.h)."""
    _fields_ = [("tile_x", C.c_int32), ("tile_y", C.c_int32), ("tiles_x", C.c_int32), ("tiles_y", C.c_int32),
                ("chunks_per_frame", C.c_uint32), ("chunk_tiles", C.c_uint32), ("chunk_pieces", C.c_uint32),
                ("index_split", C.c_uint32), ("threads", C.c_uint32), ("tiles_per_piece", C.c_uint32),
                ("pieces_x", C.c_uint32), ("pieces", C.c_uint32), ("segments", C.c_uint32),
                ("pieces_per_segment", C.c_uint32), ("lds_bins", C.c_uint32), ("lds_copies", C.c_uint32),
                ("lds_bytes", C.c_uint32), ("reserved_", C.c_uint32), ("grid", C.c_uint64), ("init_grid", C.c_uint64),
                ("global_atomics_per_frame", C.c_uint64), ("workspace_bytes", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "reserved_"}


def _histogram_plan(fn, pix, W, H, n_frames, x, y, rw, rh, shift, bins, per_frame, total, n_cu):
    """histogram_plan / histogram16_plan through the C function named fn."""
    rw = W - x if rw is None else rw
    rh = H - y if rh is None else rh
    if bins is None:   # the most allowed (0, rejected, for a shift outside the rules)
        bins = max_bins(pix, shift) if 0 <= shift < 8 * pix else 0
    outputs = (1 if per_frame else 0) | (2 if total else 0)
    pl = HistogramPlan()
    rc = getattr(lib(), fn)(W, H, n_frames, x, y, rw, rh, shift, bins, outputs, n_cu, C.byref(pl))
    if rc != OK:
        raise ValueError(f"{fn}({W}, {H}, {n_frames}, {x}, {y}, {rw}, {rh}, shift={shift}, bins={bins}, "
                         f"outputs={outputs}) -> {rc}")
    return pl.as_dict()


def histogram_plan(W, H, n_frames, x=0, y=0, rw=None, rh=None, shift=0, bins=None, per_frame=True, total=False,
                   n_cu=256):
    """dbde_hip_histogram_plan: the tile window, index geometry, launch, LDS and workspace of Codec.histogram (host
    arithmetic only).  rw / rh default to the rest of the frame, bins to the most allowed.  Raises ValueError where
    dbde_hip_histogram would return DBDE_HIP_ERR_ARG."""
    return _histogram_plan("dbde_hip_histogram_plan", 1, W, H, n_frames, x, y, rw, rh, shift, bins, per_frame, total,
                           n_cu)


def histogram16_plan(W, H, n_frames, x=0, y=0, rw=None, rh=None, shift=0, bins=None, per_frame=True, total=False,
                     n_cu=256):
    """dbde16_hip_histogram_plan: histogram_plan for DBDE16 histograms (Codec.histogram16)."""
    return _histogram_plan("dbde16_hip_histogram_plan", 2, W, H, n_frames, x, y, rw, rh, shift, bins, per_frame, total,
                           n_cu)


class Histograms:
    """Device tensors of per-frame histograms (Codec.histogram): counts int32 (n, bins) (the U32 counts, at most
    2^30), total int64 (bins,), count int64 (1,).  An output that was not asked for is None.  shift, bins and pixels
    (= rw * rh, the pixels of one frame's window) describe the binning: value v is in bin min(v >> shift, bins - 1)."""

    def __init__(self, counts=None, total=None, count=None, shift=0, bins=None, pixels=None):
        self.counts, self.total, self.count = counts, total, count
        self.shift, self.bins, self.pixels = shift, bins, pixels

    @classmethod
    def empty(cls, n, bins, device, shift=0, pixels=None, per_frame=True, total=False):
        """Zeroed outputs (a rejected frame's row then reads 0)."""
        return cls(torch.zeros((n, bins), dtype=torch.int32, device=device) if per_frame else None,
                   torch.zeros(bins, dtype=torch.int64, device=device) if total else None,
                   torch.zeros(1, dtype=torch.int64, device=device) if total else None,
                   shift=shift, bins=bins, pixels=pixels)

    @staticmethod
    def _quantile(h, q, shift):
        """Per row of h (int64, (..., bins)): the lower edge b << shift of the bin holding the k-th smallest value,
        k = floor(q * (N - 1)) with N the row's sum; -1 for an all-zero row."""
        if not 0.0 <= q <= 1.0:
            raise ValueError(f"q must lie in [0, 1], not {q!r}")
        c = torch.cumsum(h, dim=-1)
        n = c[..., -1:]
        k = torch.floor(q * (n - 1).clamp(min=0).to(torch.float64)).to(torch.int64)
        b = torch.searchsorted(c, k, right=True).squeeze(-1)
        return torch.where(n.squeeze(-1) > 0, b << shift, torch.full_like(b, -1))

    def quantile(self, q):
        """Per frame (int64, (n,)): the value of the k-th smallest pixel, k = floor(q * (pixels - 1)) (0-based), as its
        bin's lower edge b << shift; -1 for an all-zero row (a rejected frame)."""
        return self._quantile(self.counts.to(torch.int64), q, self.shift)

    def total_quantile(self, q):
        """quantile(q) of the total over the accepted frames (an int64 scalar tensor; -1 when it is empty)."""
        return self._quantile(self.total.to(torch.int64), q, self.shift)


class DbdeError(RuntimeError):
    pass


class Codec:
    """One C-ABI context: a HIP device + stream.  Not thread-safe (one per thread)."""

    def __init__(self, device=0, stream=None):
        self.L = lib()
        if torch is None or not torch.cuda.is_available():
            raise DbdeError("no HIP device visible to PyTorch; the DBDE codec has no CPU path")
        self.device = torch.device("cuda", device)
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        self.stream = stream
        h = C.c_void_p()
        rc = self.L.dbde_hip_create(device, C.c_void_p(stream.cuda_stream), C.byref(h))
        if rc != OK or not h.value:
            raise DbdeError(f"dbde_hip_create failed ({rc}): needs a gfx950 device; no CPU path")
        self.h = h

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            for m in list(getattr(self, "_trace_maps", ())):   # a map is destroyed before its context
                m.close()
            self.L.dbde_hip_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != OK:
            raise DbdeError(f"{what} failed ({rc}): {self.L.dbde_hip_last_error(self.h).decode()}")

    @property
    def arch(self):
        return self.L.dbde_hip_device_arch(self.h).decode()

    def sync(self):
        self._check(self.L.dbde_hip_sync(self.h), "dbde_hip_sync")

    # ---- batch API on device tensors ---------------------------------------------------
    def synth_frames(self, mode, seed, first_frame, n, W, H, out=None):
        if out is None:
            out = torch.empty((n, H, W), dtype=torch.uint8, device=self.device)
        m = MODES[mode] if isinstance(mode, str) else mode
        self._check(self.L.dbde_hip_synth_frames(self.h, m, seed, first_frame, n, W, H, out.data_ptr()),
                    "dbde_hip_synth_frames")
        return out

    def alloc_stream(self, W, H, n, slot_stride=0, lead=32):
        """Device buffer for n worst-case frames.  `lead` bytes are kept in front of the first
        frame (28-byte video header at lead-28) so that frames start 8-byte aligned."""
        cap = (n - 1) * slot_stride + max_frame_bytes(W, H) if slot_stride else n * max_frame_bytes(W, H)
        buf = torch.empty(lead + cap + 64, dtype=torch.uint8, device=self.device)
        return buf, lead, cap

    def encode_frames(self, images, W, H, n, out, out_offset, capacity, first_index=0, indices=None,
                      elapsed_ns=None, slot_stride=0, offsets=None, nbytes=None):
        """images: uint8 device tensor of n*H*W bytes.  Frames are written from
        out.data_ptr()+out_offset.  Returns (offsets, nbytes) int64 device tensors (per frame)."""
        if offsets is None:
            offsets = torch.empty(n, dtype=torch.int64, device=self.device)
        if nbytes is None:
            nbytes = torch.empty(n, dtype=torch.int64, device=self.device)
        rc = self.L.dbde_hip_encode_frames(
            self.h, images.data_ptr(), W, H, n, first_index,
            indices.data_ptr() if indices is not None else None,
            elapsed_ns.data_ptr() if elapsed_ns is not None else None,
            out.data_ptr() + out_offset, capacity, slot_stride, offsets.data_ptr(), nbytes.data_ptr())
        self._check(rc, "dbde_hip_encode_frames")
        return offsets, nbytes

    def decode_frames(self, stream, stream_offset, stream_bytes, offsets, W, H, n, images=None, results=None):
        """Decodes n frames; frame f starts at stream.data_ptr()+stream_offset+offsets[f]."""
        if images is None:
            images = torch.empty((n, H, W), dtype=torch.uint8, device=self.device)
        if results is None:
            results = torch.empty((n, 4), dtype=torch.int64, device=self.device)
        rc = self.L.dbde_hip_decode_frames(self.h, stream.data_ptr() + stream_offset, stream_bytes,
                                           offsets.data_ptr(), W, H, n, images.data_ptr(), results.data_ptr())
        self._check(rc, "dbde_hip_decode_frames")
        return images, results

    def _decode_roi(self, fn, dtype, stream, stream_offset, stream_bytes, offsets, W, H, n, x, y, rw, rh, origins, out,
                    results):
        """decode_roi / decode_roi16 through the C function named fn; dtype: the windows' tensor type."""
        if out is None:
            out = torch.empty((n, rh, rw), dtype=dtype, device=self.device)
        if results is None:
            results = torch.empty((n, 4), dtype=torch.int64, device=self.device)
        rc = getattr(self.L, fn)(self.h, stream.data_ptr() + stream_offset, stream_bytes, offsets.data_ptr(),
                                 W, H, n, x, y, rw, rh, origins.data_ptr() if origins is not None else None,
                                 out.data_ptr(), results.data_ptr())
        self._check(rc, fn)
        return out, results

    def _project(self, fn, pix, stream, stream_offset, stream_bytes, offsets, W, H, n, x, y, rw, rh, stats, out,
                 accumulate, results):
        """project / project16 through the C function named fn; pix: bytes per pixel of max / min."""
        rw = W - x if rw is None else rw
        rh = H - y if rh is None else rh
        if out is None:
            if accumulate:
                raise ValueError("accumulate=True needs out= (the projection to continue)")
            out = Projection.empty(rh, rw, stats, self.device, pix=pix)
        if results is None:
            results = torch.empty((max(n, 0), 4), dtype=torch.int64, device=self.device)
        ptr = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
        rc = getattr(self.L, fn)(self.h, stream.data_ptr() + stream_offset, stream_bytes, offsets.data_ptr(),
                                 W, H, n, x, y, rw, rh, 1 if accumulate else 0, ptr(out.max), ptr(out.min),
                                 ptr(out.sum), ptr(out.sumsq), ptr(out.count), ptr(results) if n > 0 else None)
        self._check(rc, fn)
        return out, results

    def decode_roi(self, stream, stream_offset, stream_bytes, offsets, W, H, n, x, y, rw, rh, origins=None, out=None,
                   results=None):
        """Decodes the rw x rh window at (x, y) of n frames (frame f at stream.data_ptr()+stream_offset+offsets[f]).
        origins: optional int32 device tensor (n, 2) of per-frame (x, y), clamped into the frame.
        Returns (windows uint8 (n, rh, rw), results (n, 4) int64) like decode_frames."""
        return self._decode_roi("dbde_hip_decode_roi", torch.uint8, stream, stream_offset, stream_bytes, offsets, W, H,
                                n, x, y, rw, rh, origins, out, results)

    def project(self, stream, stream_offset, stream_bytes, offsets, W, H, n, x=0, y=0, rw=None, rh=None,
                stats=("max", "min", "sum", "sumsq"), out=None, accumulate=False, results=None):
        """Temporal projection of the rw x rh window at (x, y) over n frames (frame f at
        stream.data_ptr()+stream_offset+offsets[f]): per-pixel max, min, sum and sum of squares of the accepted frames.
        rw / rh default to the rest of the frame.  out: a Projection to write into (accumulate=True continues it);
        its statistics are the ones computed.  Returns (Projection, results (n, 4) int64) like decode_frames."""
        return self._project("dbde_hip_project", 1, stream, stream_offset, stream_bytes, offsets, W, H, n, x, y, rw, rh,
                             stats, out, accumulate, results)

    def _project_registered(self, fn, pix, stream, stream_offset, stream_bytes, offsets, W, H, n, rw, rh, origins, stats,
                            out, accumulate, origins_used, results):
        """project_registered / project_registered16 through the C function named fn; pix: bytes per pixel."""
        for name, t in (("origins", origins), ("origins_used", origins_used)):
            if t is None and name == "origins_used":
                continue
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int32:
                raise ValueError(f"{name} must be an int32 tensor")
            if t.device != self.device:
                raise ValueError(f"{name} must be on {self.device}, not {t.device}")
            if t.dim() != 2 or t.shape[1] != 2 or t.shape[0] < n:
                raise ValueError(f"{name} must have shape (>= {n}, 2), not {tuple(t.shape)}")
            if not t.is_contiguous():
                raise ValueError(f"{name} must be contiguous")
        if out is None:
            if accumulate:
                raise ValueError("accumulate=True needs out= (the projection to continue)")
            out = Projection.empty(rh, rw, stats, self.device, pix=pix)
        if results is None:
            results = torch.empty((max(n, 0), 4), dtype=torch.int64, device=self.device)
        ptr = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
        rc = getattr(self.L, fn)(self.h, stream.data_ptr() + stream_offset, stream_bytes, offsets.data_ptr(),
                                 W, H, n, rw, rh, origins.data_ptr(), 1 if accumulate else 0, ptr(out.max),
                                 ptr(out.min), ptr(out.sum), ptr(out.sumsq), ptr(out.count), ptr(origins_used),
                                 ptr(results) if n > 0 else None)
        self._check(rc, fn)
        return out, results

    def project_registered(self, stream, stream_offset, stream_bytes, offsets, W, H, n, rw, rh, origins,
                           stats=("max", "min", "sum", "sumsq"), out=None, accumulate=False, origins_used=None,
                           results=None):
        """Registered temporal projection: project's statistics of an rw x rh window whose origin moves with the
        frames.  origins: int32 device tensor (>= n, 2) of per-frame (x, y), clamped into the frame as decode_roi
        clamps (registration.origins_from_shifts builds it from a registration's shifts).  origins_used: optional
        int32 device tensor (>= n, 2) that receives the clamped origin of every accepted frame.  out / accumulate /
        results as in project.  Returns (Projection, results (n, 4) int64); the Projection is in window coordinates."""
        return self._project_registered("dbde_hip_project_registered", 1, stream, stream_offset, stream_bytes, offsets,
                                        W, H, n, rw, rh, origins, stats, out, accumulate, origins_used, results)

    def project_registered16(self, stream, stream_offset, stream_bytes, offsets, W, H, n, rw, rh, origins,
                             stats=("max", "min", "sum", "sumsq"), out=None, accumulate=False, origins_used=None,
                             results=None):
        """project_registered for DBDE16 streams: max / min as int16 tensors holding the U16 bits, as project16."""
        return self._project_registered("dbde16_hip_project_registered", 2, stream, stream_offset, stream_bytes,
                                        offsets, W, H, n, rw, rh, origins, stats, out, accumulate, origins_used, results)

    def _project_weighted(self, fn, stream, stream_offset, stream_bytes, offsets, W, H, n, weights, x, y, rw, rh, out,
                          accumulate, one_segment, results):
        """project_weighted / project_weighted16 through the C function named fn."""
        rw = W - x if rw is None else rw
        rh = H - y if rh is None else rh
        if weights.dim() == 1:
            weights = weights.view(1, -1)
        if weights.dim() != 2 or weights.dtype != torch.float32 or not weights.is_cuda:
            raise ValueError("weights must be a float32 device tensor (R, >= n) or (>= n,)")
        R = weights.shape[0]
        if R < 1 or weights.shape[1] < n or (weights.shape[1] > 1 and weights.stride(1) != 1):
            raise ValueError("weights need at least one row, n columns and unit stride along the frames")
        if out is None:
            if accumulate:
                raise ValueError("accumulate=True needs out= (the projection to continue)")
            out = WeightedProjection.empty(R, rh, rw, self.device)
        if tuple(out.out.shape) != (R, rh, rw) or out.out.dtype != torch.float32 or not out.out.is_contiguous():
            raise ValueError(f"out.out must be a contiguous float32 tensor ({R}, {rh}, {rw})")
        if results is None:
            results = torch.empty((max(n, 0), 4), dtype=torch.int64, device=self.device)
        flags = WPROJ_ONE_SEGMENT if one_segment else 0
        for r0 in range(0, R, WPROJ_MAX_REGRESSORS):   # more than 8 rows: successive calls (the index pass repeats)
            rows = weights[r0: r0 + WPROJ_MAX_REGRESSORS]
            stride = rows.stride(0) if rows.shape[0] > 1 else max(rows.shape[1], n)
            count = out.count
            if r0 > 0:   # the frames are counted once: the later calls count into a spare that the output keeps alive
                if getattr(out, "_spare_count", None) is None:
                    out._spare_count = torch.zeros_like(out.count)
                count = out._spare_count
            rc = getattr(self.L, fn)(self.h, stream.data_ptr() + stream_offset, stream_bytes, offsets.data_ptr(),
                                     W, H, n, x, y, rw, rh, rows.data_ptr(), rows.shape[0], stride,
                                     1 if accumulate else 0, flags, out.out[r0: r0 + rows.shape[0]].data_ptr(),
                                     count.data_ptr(), results.data_ptr() if n > 0 else None)
            self._check(rc, fn)
        return out, results

    def project_weighted(self, stream, stream_offset, stream_bytes, offsets, W, H, n, weights, x=0, y=0, rw=None,
                         rh=None, out=None, accumulate=False, one_segment=False, results=None):
        """Weighted temporal projection of the rw x rh window at (x, y) over n frames: plane r is the sum over the
        accepted frames f of weights[r][f] * pixel, a chain of F32 fused multiply-adds in frame order (the defined value:
        include/dbde_hip.h).  weights: float32 device tensor (R, >= n) with unit stride along the frames and any row
        stride, so a column slice weights[:, a:b] goes in without a copy; 1-D means R = 1.  Only columns [0, n) are read.
        More than 8 rows are served by successive calls of at most 8 rows into slices of one output; the index pass then
        repeats once per call.  out: a WeightedProjection to write into (accumulate=True adds to it; unlike the integer
        projections, a run split into accumulating calls may differ in the last bits).  one_segment=True gives the pure
        frame-order chain whatever the device.  Returns (WeightedProjection, results (n, 4) int64)."""
        return self._project_weighted("dbde_hip_project_weighted", stream, stream_offset, stream_bytes, offsets, W, H, n,
                                      weights, x, y, rw, rh, out, accumulate, one_segment, results)

    def project_weighted16(self, stream, stream_offset, stream_bytes, offsets, W, H, n, weights, x=0, y=0, rw=None,
                           rh=None, out=None, accumulate=False, one_segment=False, results=None):
        """project_weighted for DBDE16 streams (U16 pixels; every one is exact in float32)."""
        return self._project_weighted("dbde16_hip_project_weighted", stream, stream_offset, stream_bytes, offsets, W, H,
                                      n, weights, x, y, rw, rh, out, accumulate, one_segment, results)

    def _project_counts(self, fn, pix, stream, stream_offset, stream_bytes, offsets, W, H, n, thresholds, x, y, rw, rh,
                        out, accumulate, results):
        """project_counts / project_counts16 through the C function named fn; pix: bytes per pixel and threshold."""
        rw = W - x if rw is None else rw
        rh = H - y if rh is None else rh
        dtype = torch.uint8 if pix == 1 else torch.int16
        if not torch.is_tensor(thresholds):
            t = np.atleast_1d(np.asarray(thresholds, dtype=np.int64))
            if t.ndim != 1 or t.size < 1 or t.min() < 0 or t.max() >= 1 << (8 * pix):
                raise ValueError(f"scalar thresholds must be one or more ints in [0, {(1 << (8 * pix)) - 1}]")
            t = t.astype(np.uint8) if pix == 1 else t.astype(np.uint16).view(np.int16)
            thresholds = torch.as_tensor(t, device=self.device)
        if thresholds.dtype != dtype or not thresholds.is_cuda or thresholds.dim() not in (1, 3):
            raise ValueError(f"thresholds must be ints or a {dtype} device tensor (K,) or (K, rh, rw)")
        maps = thresholds.dim() == 3
        K = thresholds.shape[0]
        if K < 1:
            raise ValueError("thresholds need at least one level")
        if maps:
            if tuple(thresholds.shape[1:]) != (rh, rw) or not thresholds[0].is_contiguous() or (
                    K > 1 and thresholds.stride(0) < rw * rh):
                raise ValueError(f"threshold maps must be (K, {rh}, {rw}) with contiguous levels (a slice along the "
                                 "level axis is fine)")
        elif K > 1 and thresholds.stride(0) != 1:
            raise ValueError("scalar thresholds must have unit stride")
        if out is None:
            if accumulate:
                raise ValueError("accumulate=True needs out= (the projection to continue)")
            out = CountProjection.empty(K, rh, rw, self.device)
        if tuple(out.out.shape) != (K, rh, rw) or out.out.dtype != torch.int32 or not out.out.is_contiguous():
            raise ValueError(f"out.out must be a contiguous int32 tensor ({K}, {rh}, {rw})")
        if results is None:
            results = torch.empty((max(n, 0), 4), dtype=torch.int64, device=self.device)
        for k0 in range(0, K, COUNTS_MAX_LEVELS):   # more than 8 levels: successive calls (the index pass repeats)
            lv = thresholds[k0: k0 + COUNTS_MAX_LEVELS]
            stride = (lv.stride(0) if lv.shape[0] > 1 else rw * rh) if maps else 0
            count = out.count
            if k0 > 0:   # the frames are counted once: the later calls count into a spare that the output keeps alive
                if getattr(out, "_spare_count", None) is None:
                    out._spare_count = torch.zeros_like(out.count)
                count = out._spare_count
            rc = getattr(self.L, fn)(self.h, stream.data_ptr() + stream_offset, stream_bytes, offsets.data_ptr(),
                                     W, H, n, x, y, rw, rh, lv.data_ptr(), lv.shape[0], stride,
                                     1 if accumulate else 0, COUNTS_MAPS if maps else 0,
                                     out.out[k0: k0 + lv.shape[0]].data_ptr(), count.data_ptr(),
                                     results.data_ptr() if n > 0 else None)
            self._check(rc, fn)
        return out, results

    def project_counts(self, stream, stream_offset, stream_bytes, offsets, W, H, n, thresholds, x=0, y=0, rw=None,
                       rh=None, out=None, accumulate=False, results=None):
        """Count projection of the rw x rh window at (x, y) over n frames: plane k is the number of accepted frames whose
        pixel is <= threshold k (unsigned; include/dbde_hip.h).  thresholds: an int or a sequence of ints (uploaded as
        scalars), a uint8 device tensor (K,) (scalars, nothing synchronises) or a uint8 device tensor (K, rh, rw) of
        per-pixel maps in window coordinates; a map tensor may be a slice along the level axis of a wider one.  More than
        8 levels are served by successive calls of at most 8 into slices of one output; the index pass then repeats once
        per call and the frames are counted once.  out: a CountProjection to write into (accumulate=True adds to it: the
        counts are exact integers, so any split of a run of frames gives the same planes).  Returns (CountProjection,
        results (n, 4) int64)."""
        return self._project_counts("dbde_hip_project_counts", 1, stream, stream_offset, stream_bytes, offsets, W, H, n,
                                    thresholds, x, y, rw, rh, out, accumulate, results)

    def project_counts16(self, stream, stream_offset, stream_bytes, offsets, W, H, n, thresholds, x=0, y=0, rw=None,
                         rh=None, out=None, accumulate=False, results=None):
        """project_counts for DBDE16 streams: U16 pixels and thresholds, the tensors int16 holding the U16 bits."""
        return self._project_counts("dbde16_hip_project_counts", 2, stream, stream_offset, stream_bytes, offsets, W, H,
                                    n, thresholds, x, y, rw, rh, out, accumulate, results)

    def _project_pairs(self, fn, stream, stream_offset, stream_bytes, offsets, W, H, n, pairs, x, y, rw, rh, out,
                       accumulate, results):
        """project_pairs / project_pairs16 through the C function named fn."""
        rw = W - x if rw is None else rw
        rh = H - y if rh is None else rh
        mask = pairs_mask(pairs)
        if out is None:
            if accumulate:
                raise ValueError("accumulate=True needs out= (the projection to continue)")
            out = PairProjection.empty(pair_offsets(mask), rh, rw, self.device)
        if out.offsets != pair_offsets(mask):
            raise ValueError(f"out holds the offsets {out.offsets}, the call asks for {pair_offsets(mask)}")
        if (tuple(out.out.shape) != (len(out.offsets), rh, rw) or out.out.dtype != torch.int64
                or not out.out.is_contiguous()):
            raise ValueError(f"out.out must be a contiguous int64 tensor ({len(out.offsets)}, {rh}, {rw})")
        if results is None:
            results = torch.empty((max(n, 0), 4), dtype=torch.int64, device=self.device)
        rc = getattr(self.L, fn)(self.h, stream.data_ptr() + stream_offset, stream_bytes, offsets.data_ptr(), W, H, n,
                                 x, y, rw, rh, mask, 1 if accumulate else 0, out.out.data_ptr(), out.count.data_ptr(),
                                 results.data_ptr() if n > 0 else None)
        self._check(rc, fn)
        return out, results

    def project_pairs(self, stream, stream_offset, stream_bytes, offsets, W, H, n, pairs=8, x=0, y=0, rw=None, rh=None,
                      out=None, accumulate=False, results=None):
        """Neighbour-product projection of the rw x rh window at (x, y) over n frames: per requested forward offset
        (dx, dy) one plane of sums of p[y][x] * p[y + dy][x + dx] over the accepted frames, both pixels inside the
        window (include/dbde_hip.h).  pairs: 4 (RIGHT and DOWN), 8 (all four offsets), a mask, or an iterable of (dx, dy)
        (pairs_mask).  out: a PairProjection to write into (accumulate=True adds to it: the sums are exact integers, so
        any split of a run of frames gives the same planes).  With project's sum, sumsq and count of the same frames
        and window, correlation.local_correlation turns it into the local correlation image.  Returns (PairProjection,
        results (n, 4) int64)."""
        return self._project_pairs("dbde_hip_project_pairs", stream, stream_offset, stream_bytes, offsets, W, H, n, pairs,
                                   x, y, rw, rh, out, accumulate, results)

    def project_pairs16(self, stream, stream_offset, stream_bytes, offsets, W, H, n, pairs=8, x=0, y=0, rw=None,
                        rh=None, out=None, accumulate=False, results=None):
        """project_pairs for DBDE16 streams (U16 pixels; a product stays below 2^32)."""
        return self._project_pairs("dbde16_hip_project_pairs", stream, stream_offset, stream_bytes, offsets, W, H, n,
                                   pairs, x, y, rw, rh, out, accumulate, results)

    def _project_lag(self, fn, bits, stream, stream_offset, stream_bytes, offsets, W, H, n, lag, stats, lead, x, y, rw,
                     rh, out, accumulate, results):
        """project_lag / project_lag16 through the C function named fn; bits: of a pixel (the maxdiff plane's)."""
        rw = W - x if rw is None else rw
        rh = H - y if rh is None else rh
        names = lag_stats(lag_mask(stats))
        if out is None:
            if accumulate:
                raise ValueError("accumulate=True needs out= (the projection to continue)")
            out = LagProjection.empty(names, rh, rw, self.device, lag=lag, bits=bits)
        if out.lag != lag:
            raise ValueError(f"out holds lag {out.lag}, the call asks for {lag}")
        ptr = {}
        for k in LAG_STATS:
            t = getattr(out, k) if k in names else None
            if k in names:
                want = torch.int64 if k != "maxdiff" else torch.uint8 if bits == 8 else torch.int16
                if t is None or tuple(t.shape) != (rh, rw) or t.dtype != want or not t.is_contiguous():
                    raise ValueError(f"out.{k} must be a contiguous {want} tensor ({rh}, {rw})")
            ptr[k] = t.data_ptr() if t is not None else None
        if results is None:
            results = torch.empty((max(n, 0), 4), dtype=torch.int64, device=self.device)
        rc = getattr(self.L, fn)(self.h, stream.data_ptr() + stream_offset, stream_bytes, offsets.data_ptr(), W, H, n,
                                 x, y, rw, rh, lag, lead, 1 if accumulate else 0, ptr["product"], ptr["pairsum"],
                                 ptr["absdiff"], ptr["sqdiff"], ptr["maxdiff"], out.pairs.data_ptr(),
                                 out.count.data_ptr(), results.data_ptr() if n > 0 else None)
        self._check(rc, fn)
        return out, results

    def project_lag(self, stream, stream_offset, stream_bytes, offsets, W, H, n, lag=1, stats=("sqdiff",), lead=0, x=0,
                    y=0, rw=None, rh=None, out=None, accumulate=False, results=None):
        """Lag projection of the rw x rh window at (x, y) over n frames: per pixel, over the pairs
        (a, b) = (p[f - lag], p[f]) with f >= max(lead, lag) and both frames accepted, the requested ones of
        product = sum a b, pairsum = sum (a + b), absdiff = sum |b - a|, sqdiff = sum (b - a)^2 and
        maxdiff = max |b - a| (include/dbde_hip.h).  stats: names from LAG_STATS.  lead: leading frames that are history
        only (the frames carried over from the call before).  out: a LagProjection to write into; planes of out that
        stats does not name are left alone (accumulate=True adds to it: the values are exact integers, so a run of
        frames split by the header's rule gives the same planes).  lagged.py turns the planes into the noise image, the
        mean absolute difference and the autocorrelation.  Returns (LagProjection, results (n, 4) int64)."""
        return self._project_lag("dbde_hip_project_lag", 8, stream, stream_offset, stream_bytes, offsets, W, H, n, lag,
                                 stats, lead, x, y, rw, rh, out, accumulate, results)

    def project_lag16(self, stream, stream_offset, stream_bytes, offsets, W, H, n, lag=1, stats=("sqdiff",), lead=0,
                      x=0, y=0, rw=None, rh=None, out=None, accumulate=False, results=None):
        """project_lag for DBDE16 streams (U16 pixels; maxdiff int16 holding the U16 bits)."""
        return self._project_lag("dbde16_hip_project_lag", 16, stream, stream_offset, stream_bytes, offsets, W, H, n,
                                 lag, stats, lead, x, y, rw, rh, out, accumulate, results)

    def _project_groups(self, fn, pix, stream, stream_offset, stream_bytes, offsets, W, H, n, x, y, rw, rh, group_frames,
                        group_starts, stats, sum_dtype, accumulate, out, results):
        """project_groups / project_groups16 through the C function named fn; pix: bytes per pixel of max / min."""
        rw = W - x if rw is None else rw
        rh = H - y if rh is None else rh
        if (group_frames is None) == (group_starts is None):
            raise ValueError("give exactly one of group_frames= and group_starts=")
        if group_starts is not None:
            if not torch.is_tensor(group_starts):
                group_starts = torch.as_tensor(np.asarray(group_starts, dtype=np.int64).astype(np.uint32).view(np.int32),
                                               device=self.device)
            if group_starts.dtype != torch.int32 or group_starts.dim() != 1 or not group_starts.is_contiguous():
                raise ValueError("group_starts must be a contiguous 1-D int32 tensor (the U32 bits)")
            n_groups, g = group_starts.numel() - 1, 0
        else:
            g = int(group_frames)
            n_groups = -(-n // g) if g > 0 else 0
        if out is None:
            if accumulate:
                raise ValueError("accumulate=True needs out= (the projection to continue)")
            out = GroupProjection.empty(max(n_groups, 0), rh, rw, stats, self.device, pix=pix, sum_dtype=sum_dtype)
        sum_type = _sum_type(out.sum.dtype if out.sum is not None else sum_dtype)
        if results is None:
            results = torch.empty((max(n, 0), 4), dtype=torch.int64, device=self.device)
        if group_starts is None and n == 0 and g > 0:
            return out, results   # no frame, no group: nothing to do (planes of no group have no address to pass)
        ptr = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
        rc = getattr(self.L, fn)(self.h, stream.data_ptr() + stream_offset, stream_bytes, offsets.data_ptr(),
                                 W, H, n, x, y, rw, rh, g, ptr(group_starts), n_groups, sum_type,
                                 1 if accumulate else 0, ptr(out.max), ptr(out.min), ptr(out.sum), ptr(out.sumsq),
                                 ptr(out.counts), ptr(results) if n > 0 else None)
        self._check(rc, fn)
        return out, results

    def project_groups(self, stream, stream_offset, stream_bytes, offsets, W, H, n, x=0, y=0, rw=None, rh=None,
                       group_frames=None, group_starts=None, stats=("max", "min", "sum", "sumsq"),
                       sum_dtype=None, accumulate=False, out=None, results=None):
        """Grouped temporal projection: Codec.project's reduction once per group of frames.  group_frames=g: group k is
        frames [k*g, min((k+1)*g, n)).  group_starts: n_groups + 1 frame numbers (a sequence, or an int32 device tensor
        holding U32 bits), group k is frames [s[k], s[k+1]) clamped into [0, n].  sum_dtype: torch.int32 (the default:
        U32 bits) or torch.int16 (U16 bits; groups of at most 257 frames, no accumulate).  out: a GroupProjection to
        write into (accumulate=True continues it).  Returns (GroupProjection, results (n, 4) int64)."""
        return self._project_groups("dbde_hip_project_groups", 1, stream, stream_offset, stream_bytes, offsets, W, H, n,
                                    x, y, rw, rh, group_frames, group_starts, stats,
                                    torch.int32 if sum_dtype is None else sum_dtype, accumulate, out, results)

    def project_groups16(self, stream, stream_offset, stream_bytes, offsets, W, H, n, x=0, y=0, rw=None, rh=None,
                         group_frames=None, group_starts=None, stats=("max", "min", "sum", "sumsq"),
                         sum_dtype=None, accumulate=False, out=None, results=None):
        """project_groups for DBDE16 streams: max / min int16 tensors holding the U16 bits, U32 sums only."""
        return self._project_groups("dbde16_hip_project_groups", 2, stream, stream_offset, stream_bytes, offsets, W, H,
                                    n, x, y, rw, rh, group_frames, group_starts, stats,
                                    torch.int32 if sum_dtype is None else sum_dtype, accumulate, out, results)

    def _histogram(self, fn, pix, stream, stream_offset, stream_bytes, offsets, W, H, n, x, y, rw, rh, shift, bins,
                   per_frame, total, out, accumulate, results):
        """histogram / histogram16 through the C function named fn."""
        rw = W - x if rw is None else rw
        rh = H - y if rh is None else rh
        if bins is None:
            bins = out.bins if out is not None and out.bins is not None else max_bins(pix, shift)
        if out is None:
            if accumulate:
                raise ValueError("accumulate=True needs out= (the histograms to continue)")
            out = Histograms.empty(max(n, 0), bins, self.device, shift=shift, pixels=rw * rh, per_frame=per_frame,
                                   total=total)
        else:
            out.shift, out.bins, out.pixels = shift, bins, rw * rh
        if results is None:
            results = torch.empty((max(n, 0), 4), dtype=torch.int64, device=self.device)
        ptr = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
        rc = getattr(self.L, fn)(self.h, stream.data_ptr() + stream_offset, stream_bytes, offsets.data_ptr(),
                                 W, H, n, x, y, rw, rh, shift, bins, 1 if accumulate else 0, ptr(out.counts),
                                 ptr(out.total), ptr(out.count), ptr(results) if n > 0 else None)
        self._check(rc, fn)
        return out, results

    def histogram(self, stream, stream_offset, stream_bytes, offsets, W, H, n, x=0, y=0, rw=None, rh=None, shift=0,
                  bins=None, per_frame=True, total=False, out=None, accumulate=False, results=None):
        """Per-frame histograms of the rw x rh window at (x, y) of n frames (frame f at
        stream.data_ptr()+stream_offset+offsets[f]): value v counts in bin min(v >> shift, bins - 1).  rw / rh default
        to the rest of the frame, bins to 256 >> shift.  per_frame: the (n, bins) rows; total: the sum over the accepted
        frames and their number (accumulate=True adds to out's).  out: a Histograms to write into.
        Returns (Histograms, results (n, 4) int64) like decode_frames."""
        return self._histogram("dbde_hip_histogram", 1, stream, stream_offset, stream_bytes, offsets, W, H, n, x, y, rw,
                               rh, shift, bins, per_frame, total, out, accumulate, results)

    def histogram16(self, stream, stream_offset, stream_bytes, offsets, W, H, n, x=0, y=0, rw=None, rh=None, shift=0,
                    bins=None, per_frame=True, total=False, out=None, accumulate=False, results=None):
        """DBDE16 per-frame histograms: histogram's arguments and results over U16 values; bins default to
        min(4096, 65536 >> shift)."""
        return self._histogram("dbde16_hip_histogram", 2, stream, stream_offset, stream_bytes, offsets, W, H, n, x, y,
                               rw, rh, shift, bins, per_frame, total, out, accumulate, results)

    def _decode_binned(self, fn, pix, stream, stream_offset, stream_bytes, offsets, W, H, n, bin, x, y, rw, rh, stats,
                       out, results):
        """decode_binned / decode_binned16 through the C function named fn."""
        rw = W - x if rw is None else rw
        rh = H - y if rh is None else rh
        if out is None:
            out = Binned.empty(max(n, 0), rh, rw, bin, stats, self.device, pix=pix)
        else:
            out.bin, out.pixels = bin, bin_pixels(rh, rw, bin, self.device)
        if results is None:
            results = torch.empty((max(n, 0), 4), dtype=torch.int64, device=self.device)
        if n == 0:   # nothing to do (empty planes have no address to pass): the arguments are still checked
            mask = (1 if out.sum is not None else 0) | (2 if out.max is not None else 0) | (4 if out.min is not None else 0)
            _binned_plan(fn.replace("decode_binned", "binned_plan"), W, H, 0, bin, x, y, rw, rh, mask)
            return out, results
        ptr = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
        rc = getattr(self.L, fn)(self.h, stream.data_ptr() + stream_offset, stream_bytes, offsets.data_ptr(),
                                 W, H, n, x, y, rw, rh, bin, ptr(out.sum), ptr(out.max), ptr(out.min),
                                 ptr(results) if n > 0 else None)
        self._check(rc, fn)
        return out, results

    def decode_binned(self, stream, stream_offset, stream_bytes, offsets, W, H, n, bin, x=0, y=0, rw=None, rh=None,
                      stats=("sum",), out=None, results=None):
        """Binned decode of the rw x rh window at (x, y) of n frames (frame f at
        stream.data_ptr()+stream_offset+offsets[f]): the sum, max and min of every bin x bin block (bin 2, 4 or 8; x and
        y multiples of bin), bins on the right and bottom edge ending at the window's edge.  rw / rh default to the rest
        of the frame.  out: a Binned to write into; its planes are the ones computed (stats is then ignored).
        Returns (Binned, results (n, 4) int64) like decode_frames."""
        return self._decode_binned("dbde_hip_decode_binned", 1, stream, stream_offset, stream_bytes, offsets, W, H, n,
                                   bin, x, y, rw, rh, stats, out, results)

    def decode_binned16(self, stream, stream_offset, stream_bytes, offsets, W, H, n, bin, x=0, y=0, rw=None, rh=None,
                        stats=("sum",), out=None, results=None):
        """DBDE16 binned decode: decode_binned's arguments and results over U16 pixels (sum int32, max / min int16
        tensors holding the U16 bits)."""
        return self._decode_binned("dbde16_hip_decode_binned", 2, stream, stream_offset, stream_bytes, offsets, W, H, n,
                                   bin, x, y, rw, rh, stats, out, results)

    def _decode_scaled(self, fn, stream, stream_offset, stream_bytes, offsets, W, H, n, x, y, rw, rh, dtype, dark, gain,
                       origins, out, results):
        """decode_scaled / decode_scaled16 through the C function named fn."""
        rw = W - x if rw is None else rw
        rh = H - y if rh is None else rh
        try:
            out_type, dtype = _scaled_type(dtype)
        except ValueError as e:
            raise DbdeError(f"{fn}: {e}") from None

        def term(v, name, default):
            """(map pointer or None, scalar) of dark= / gain=."""
            if v is None:
                return None, default
            if isinstance(v, torch.Tensor):
                if v.dtype != torch.float32 or tuple(v.shape) != (H, W) or not v.is_contiguous() or not v.is_cuda:
                    raise DbdeError(f"{fn}: {name} must be a contiguous float32 device tensor of shape ({H}, {W}), "
                                    f"not {v.dtype} {tuple(v.shape)}")
                return v.data_ptr(), default
            return None, float(v)

        d_ptr, d0 = term(dark, "dark", 0.0)
        g_ptr, g0 = term(gain, "gain", 1.0)
        if out is None:
            out = torch.empty((max(n, 0), rh, rw), dtype=dtype, device=self.device)
        elif out.dtype != dtype:
            raise DbdeError(f"{fn}: out is {out.dtype}, dtype= is {dtype}")
        elif not out.is_cuda or not out.is_contiguous() or out.numel() < max(n, 0) * rw * rh:
            raise DbdeError(f"{fn}: out must be a contiguous device tensor of at least {max(n, 0)} x {rh} x {rw} "
                            f"elements, not {tuple(out.shape)}")
        if results is None:
            results = torch.empty((max(n, 0), 4), dtype=torch.int64, device=self.device)
        if n == 0:   # nothing to do (empty tensors have no address to pass): the arguments are still checked
            _scaled_plan(fn.replace("decode_scaled", "scaled_plan"), W, H, 0, x, y, rw, rh, out_type)
            return out, results
        rc = getattr(self.L, fn)(self.h, stream.data_ptr() + stream_offset, stream_bytes, offsets.data_ptr(),
                                 W, H, n, x, y, rw, rh, origins.data_ptr() if origins is not None else None,
                                 out_type, d_ptr, d0, g_ptr, g0, out.data_ptr(), results.data_ptr())
        self._check(rc, fn)
        return out, results

    def decode_scaled(self, stream, stream_offset, stream_bytes, offsets, W, H, n, x=0, y=0, rw=None, rh=None,
                      dtype=torch.float32, dark=None, gain=None, origins=None, out=None, results=None):
        """Scaled float decode of the rw x rh window at (x, y) of n frames (frame f at
        stream.data_ptr()+stream_offset+offsets[f]): ((pixel.float() - dark) * gain).to(dtype) in one pass, dtype
        torch.float32, float16 or bfloat16.  dark / gain: None (0.0 / 1.0), a Python float, or a contiguous float32
        device tensor (H, W) in FRAME coordinates.  rw / rh default to the rest of the frame.  origins: optional int32
        device tensor (n, 2) of per-frame (x, y), clamped into the frame as decode_roi clamps them.
        Returns (windows (n, rh, rw) of dtype, results (n, 4) int64) like decode_frames."""
        return self._decode_scaled("dbde_hip_decode_scaled", stream, stream_offset, stream_bytes, offsets, W, H, n, x, y,
                                   rw, rh, dtype, dark, gain, origins, out, results)

    def decode_scaled16(self, stream, stream_offset, stream_bytes, offsets, W, H, n, x=0, y=0, rw=None, rh=None,
                        dtype=torch.float32, dark=None, gain=None, origins=None, out=None, results=None):
        """DBDE16 scaled float decode: decode_scaled's arguments and results over U16 pixels (16 is the stream format;
        the output type is dtype=)."""
        return self._decode_scaled("dbde16_hip_decode_scaled", stream, stream_offset, stream_bytes, offsets, W, H, n, x,
                                   y, rw, rh, dtype, dark, gain, origins, out, results)

    def _decode_mask(self, fn, pix, stream, stream_offset, stream_bytes, offsets, W, H, n, x, y, rw, rh, lo, hi, outside,
                     origins, mask, counts, boxes, results):
        """decode_mask / decode_mask16 through the C function named fn."""
        rw = W - x if rw is None else rw
        rh = H - y if rh is None else rh
        map_dtype, top = (torch.uint8, 255) if pix == 1 else (torch.int16, 65535)

        def term(v, name, default):
            """(map pointer or None, scalar) of lo= / hi=."""
            if v is None:
                return None, default
            if isinstance(v, torch.Tensor):
                if v.dtype != map_dtype or tuple(v.shape) != (H, W) or not v.is_contiguous() or not v.is_cuda:
                    raise DbdeError(f"{fn}: {name} must be a contiguous {map_dtype} device tensor of shape ({H}, {W}), "
                                    f"not {v.dtype} {tuple(v.shape)}")
                return v.data_ptr(), default
            if int(v) != v or not 0 <= int(v) <= top:
                raise DbdeError(f"{fn}: {name}={v!r} is not an integer in [0, {top}]")
            return None, int(v)

        lo_ptr, lo0 = term(lo, "lo", 0)
        hi_ptr, hi0 = term(hi, "hi", top)
        n0 = max(n, 0)
        if mask is None:
            mask = Mask.empty(n0, rh, rw, self.device, bits=True, counts=bool(counts), boxes=bool(boxes))
        else:
            mask.rw = rw
            words = -(-rw // 64)
            for name, t, dt, want in (("bits", mask.bits, torch.int64, n0 * rh * words), ("counts", mask.counts, torch.int32, n0),
                                      ("boxes", mask.boxes, torch.int32, 4 * n0)):
                if t is not None and (t.dtype != dt or not t.is_cuda or not t.is_contiguous() or t.numel() < want):
                    raise DbdeError(f"{fn}: mask.{name} must be a contiguous {dt} device tensor of at least {want} "
                                    f"elements, not {t.dtype} {tuple(t.shape)}")
            if mask.bits is None and mask.counts is None and mask.boxes is None:
                raise DbdeError(f"{fn}: the Mask has no output")
        if results is None:
            results = torch.empty((n0, 4), dtype=torch.int64, device=self.device)
        if n == 0:   # nothing to do (empty tensors have no address to pass): the arguments are still checked
            try:
                _mask_plan(fn.replace("decode_mask", "mask_plan"), W, H, 0, x, y, rw, rh)
            except ValueError as e:   # the same error as with frames to decode
                raise DbdeError(f"{fn}: {e}") from None
            return mask, results
        ptr = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
        rc = getattr(self.L, fn)(self.h, stream.data_ptr() + stream_offset, stream_bytes, offsets.data_ptr(),
                                 W, H, n, x, y, rw, rh, ptr(origins), MASK_OUTSIDE if outside else MASK_INSIDE,
                                 lo_ptr, lo0, hi_ptr, hi0, ptr(mask.bits), ptr(mask.counts), ptr(mask.boxes),
                                 results.data_ptr())
        self._check(rc, fn)
        return mask, results

    def decode_mask(self, stream, stream_offset, stream_bytes, offsets, W, H, n, x=0, y=0, rw=None, rh=None,
                    lo=None, hi=None, outside=False, origins=None, mask=None, counts=True, boxes=False, results=None):
        """Threshold mask of the rw x rh window at (x, y) of n frames (frame f at
        stream.data_ptr()+stream_offset+offsets[f]): one bit per pixel, set where lo <= pixel <= hi (outside=True: where
        pixel < lo or pixel > hi), straight from the stream.  lo / hi: None (0 / 255), an integer, or a contiguous uint8
        device tensor (H, W) in FRAME coordinates; lo > hi is an empty band.  rw / rh default to the rest of the frame.
        origins: optional int32 device tensor (n, 2) of per-frame (x, y), clamped into the frame as decode_roi clamps
        them.  counts / boxes: also the set bits per frame / their bounding boxes.  mask: a Mask to write into; its
        tensors are the outputs computed (counts / boxes are then ignored; bits may be None).
        Returns (Mask, results (n, 4) int64) like decode_frames."""
        return self._decode_mask("dbde_hip_decode_mask", 1, stream, stream_offset, stream_bytes, offsets, W, H, n, x, y,
                                 rw, rh, lo, hi, outside, origins, mask, counts, boxes, results)

    def decode_mask16(self, stream, stream_offset, stream_bytes, offsets, W, H, n, x=0, y=0, rw=None, rh=None,
                      lo=None, hi=None, outside=False, origins=None, mask=None, counts=True, boxes=False, results=None):
        """DBDE16 threshold mask: decode_mask's arguments and results over U16 pixels; lo / hi default to 0 / 65535,
        maps are int16 tensors holding the U16 bits (as decode_frames16 returns its images)."""
        return self._decode_mask("dbde16_hip_decode_mask", 2, stream, stream_offset, stream_bytes, offsets, W, H, n, x,
                                 y, rw, rh, lo, hi, outside, origins, mask, counts, boxes, results)

    def _decode_patches(self, fn, dtype, stream, stream_offset, stream_bytes, offsets, W, H, n, pw, ph, origins, counts,
                        edge, fill, out, used, results):
        """decode_patches / decode_patches16 through the C function named fn; dtype: the patches' tensor type."""
        if (not torch.is_tensor(origins) or origins.dtype != torch.int32 or origins.dim() != 3 or origins.shape[0] != n
                or origins.shape[2] != 2 or not origins.is_contiguous()):
            raise ValueError("origins must be a contiguous int32 device tensor of shape (n, K, 2)")
        K = int(origins.shape[1])
        if counts is not None and (not torch.is_tensor(counts) or counts.dtype != torch.int32 or counts.dim() != 1
                                   or counts.numel() != n or not counts.is_contiguous()):
            raise ValueError("counts must be a contiguous 1-D int32 tensor of n entries (the U32 bits)")
        if used is not None and (not torch.is_tensor(used) or used.dtype != torch.int32 or not used.is_contiguous()
                                 or used.numel() < 2 * n * K):
            raise ValueError("used must be a contiguous int32 device tensor of at least n * K * 2 entries")
        if out is None:
            out = torch.empty((n, K, ph, pw), dtype=dtype, device=self.device)
        elif out.dtype != dtype or not out.is_contiguous() or out.numel() < n * K * ph * pw:
            raise ValueError(f"out must be a contiguous {dtype} device tensor of at least n * K * ph * pw entries")
        if results is None:
            results = torch.empty((max(n, 0), 4), dtype=torch.int64, device=self.device)
        ptr = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
        rc = getattr(self.L, fn)(self.h, stream.data_ptr() + stream_offset, stream_bytes, offsets.data_ptr(), W, H, n,
                                 pw, ph, K, origins.data_ptr(), ptr(counts), patch_edge_mode(edge), int(fill),
                                 out.data_ptr(), ptr(used), ptr(results) if n > 0 else None)
        self._check(rc, fn)
        return out, results

    def decode_patches(self, stream, stream_offset, stream_bytes, offsets, W, H, n, pw, ph, origins, counts=None,
                       edge="clamp", fill=0, out=None, used=None, results=None):
        """Decodes K patches of pw x ph per frame of n frames (frame f at stream.data_ptr()+stream_offset+offsets[f]) in
        one call.  origins: int32 device tensor (n, K, 2) of (x, y) per frame and patch (origins_from_centres makes them
        from object centres).  edge="clamp": origins are clamped into the frame, patch (f, k) is decode_roi's window at
        origins[f, k]; edge="fill": the patch sits where its origin says and its pixels outside the frame are fill.
        counts: optional int32 (n,), the live patches of each frame; patches k >= counts[f] stay untouched.  used:
        optional int32 (n, K, 2) that receives the origins used (the clamped ones in clamp mode).
        Returns (patches uint8 (n, K, ph, pw), results (n, 4) int64) like decode_frames."""
        return self._decode_patches("dbde_hip_decode_patches", torch.uint8, stream, stream_offset, stream_bytes, offsets,
                                    W, H, n, pw, ph, origins, counts, edge, fill, out, used, results)

    def decode_patches16(self, stream, stream_offset, stream_bytes, offsets, W, H, n, pw, ph, origins, counts=None,
                         edge="clamp", fill=0, out=None, used=None, results=None):
        """DBDE16 patches: decode_patches' arguments and results with int16 patches holding the U16 bits (as
        decode_frames16 returns its images); fill up to 65535."""
        return self._decode_patches("dbde16_hip_decode_patches", torch.int16, stream, stream_offset, stream_bytes,
                                    offsets, W, H, n, pw, ph, origins, counts, edge, fill, out, used, results)

    def _patch_moments(self, fn, stream, stream_offset, stream_bytes, offsets, W, H, n, pw, ph, origins, lo, hi, weight,
                       counts, edge, out, bbox, used, results):
        """patch_moments / patch_moments16 through the C function named fn."""
        if (not torch.is_tensor(origins) or origins.dtype != torch.int32 or origins.dim() != 3 or origins.shape[0] != n
                or origins.shape[2] != 2 or not origins.is_contiguous()):
            raise ValueError("origins must be a contiguous int32 device tensor of shape (n, K, 2)")
        K = int(origins.shape[1])
        if counts is not None and (not torch.is_tensor(counts) or counts.dtype != torch.int32 or counts.dim() != 1
                                   or counts.numel() != n or not counts.is_contiguous()):
            raise ValueError("counts must be a contiguous 1-D int32 tensor of n entries (the U32 bits)")
        # what the C call refuses of the scalars, checked here as well: the call is not made when n == 0, and ctypes would
        # take lo, hi and the mode modulo 2^32 before the C range check sees them
        lo, hi, mode, top = int(lo), int(hi), moment_weight_mode(weight), 0xFFFF if fn.startswith("dbde16") else 0xFF
        if not (0 <= lo <= top and 0 <= hi <= top):
            raise DbdeError(f"{fn}: thresholds lo={lo}, hi={hi} outside [0, {top}]")
        if mode not in MOMENT_WEIGHTS.values():
            raise DbdeError(f"{fn}: unknown weight mode {mode}")
        if used is None:
            used = torch.empty((n, K, 2), dtype=torch.int32, device=self.device)
        elif not torch.is_tensor(used) or used.dtype != torch.int32 or not used.is_contiguous() or used.numel() < 2 * n * K:
            raise ValueError("used must be a contiguous int32 device tensor of at least n * K * 2 entries")
        if bbox is True:
            bbox = torch.empty((n, K, 4), dtype=torch.int32, device=self.device)
        elif bbox is False:
            bbox = None
        elif bbox is not None and (not torch.is_tensor(bbox) or bbox.dtype != torch.int32 or not bbox.is_contiguous()
                                   or bbox.numel() < 4 * n * K):
            raise ValueError("bbox must be a contiguous int32 device tensor of at least n * K * 4 entries")
        if out is None:
            out = torch.empty((n, K, 8), dtype=torch.int64, device=self.device)
        elif not torch.is_tensor(out) or out.dtype != torch.int64 or not out.is_contiguous() or out.numel() < 8 * n * K:
            raise ValueError("out must be a contiguous int64 device tensor of at least n * K * 8 entries")
        if results is None:
            results = torch.empty((max(n, 0), 4), dtype=torch.int64, device=self.device)
        if n == 0:   # nothing to do (empty tensors have no address to pass): the sizes are still checked
            try:
                _patch_moments_plan(fn + "_plan", W, H, 0, pw, ph, max(K, 1), edge)
            except ValueError as e:
                raise DbdeError(f"{fn}: {e}") from None
            return PatchMoments(out, bbox, used, pw, ph), results
        ptr = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
        rc = getattr(self.L, fn)(self.h, stream.data_ptr() + stream_offset, stream_bytes, offsets.data_ptr(), W, H, n,
                                 pw, ph, K, origins.data_ptr(), ptr(counts), patch_edge_mode(edge), lo, hi,
                                 mode, out.data_ptr(), ptr(bbox), used.data_ptr(),
                                 ptr(results) if n > 0 else None)
        self._check(rc, fn)
        return PatchMoments(out, bbox, used, pw, ph), results

    def patch_moments(self, stream, stream_offset, stream_bytes, offsets, W, H, n, pw, ph, origins, lo, hi,
                      weight="above", counts=None, edge="clamp", out=None, bbox=None, used=None, results=None):
        """Thresholded image moments of K patches of pw x ph per frame of n frames (frame f at
        stream.data_ptr()+stream_offset+offsets[f]) in one call, straight from the stream: no pixel is written.
        origins, counts and edge as in decode_patches, except that a patch pixel outside the frame counts for nothing
        (there is no fill).  A pixel p is selected when lo <= p <= hi; its weight is 1 ("count"), p ("value"), p - lo
        ("above") or hi - p ("below").  out: optional int64 (n, K, 8) to write the sums into; bbox: True for the
        selected pixels' boxes, or an int32 (n, K, 4) tensor to write them into; used: optional int32 (n, K, 2).
        Returns (PatchMoments, results (n, 4) int64) like decode_frames."""
        return self._patch_moments("dbde_hip_patch_moments", stream, stream_offset, stream_bytes, offsets, W, H, n, pw,
                                   ph, origins, lo, hi, weight, counts, edge, out, bbox, used, results)

    def patch_moments16(self, stream, stream_offset, stream_bytes, offsets, W, H, n, pw, ph, origins, lo, hi,
                        weight="above", counts=None, edge="clamp", out=None, bbox=None, used=None, results=None):
        """DBDE16 patch moments: patch_moments' arguments and results over U16 pixels (lo, hi up to 65535)."""
        return self._patch_moments("dbde16_hip_patch_moments", stream, stream_offset, stream_bytes, offsets, W, H, n,
                                   pw, ph, origins, lo, hi, weight, counts, edge, out, bbox, used, results)

    def _match_patches(self, fn, dtype, stream, stream_offset, stream_bytes, offsets, W, H, n, templates, S, origins,
                       counts, edge, fill, stats, out, used, results):
        """match_patches / match_patches16 through the C function named fn; dtype: the templates' tensor type."""
        if (not torch.is_tensor(origins) or origins.dtype != torch.int32 or origins.dim() != 3 or origins.shape[0] != n
                or origins.shape[2] != 2 or not origins.is_contiguous()):
            raise ValueError("origins must be a contiguous int32 device tensor of shape (n, K, 2)")
        K = int(origins.shape[1])
        if (not torch.is_tensor(templates) or templates.dtype != dtype or templates.dim() != 3
                or not templates.is_contiguous() or templates.shape[0] not in (1, K)):
            raise ValueError(f"templates must be a contiguous {dtype} device tensor of shape (K, th, tw) or (1, th, tw)")
        Kt, th, tw = (int(v) for v in templates.shape)
        if counts is not None and (not torch.is_tensor(counts) or counts.dtype != torch.int32 or counts.dim() != 1
                                   or counts.numel() != n or not counts.is_contiguous()):
            raise ValueError("counts must be a contiguous 1-D int32 tensor of n entries (the U32 bits)")
        # what the C call refuses of the scalars, checked here as well: the call is not made when n == 0, and ctypes would
        # take them modulo 2^32 before the C range check sees them
        S, fill, mask = int(S), int(fill), match_mask(stats)
        try:
            pl = _match_plan(fn.replace("match_patches", "match_plan"), W, H, max(n, 0), tw, th, S, max(K, 1),
                             Kt if K > 0 else 1, edge, fill, mask)
        except ValueError as e:
            raise DbdeError(f"{fn}: {e}") from None
        D = pl["D"]
        if used is None:
            used = torch.empty((n, K, 2), dtype=torch.int32, device=self.device)
        elif not torch.is_tensor(used) or used.dtype != torch.int32 or not used.is_contiguous() or used.numel() < 2 * n * K:
            raise ValueError("used must be a contiguous int32 device tensor of at least n * K * 2 entries")
        names = ("prod", "sum", "sq")
        if out is None:
            out = {}
        elif not isinstance(out, dict) or any(k not in names for k in out):
            raise ValueError("out must be a dict of int64 tensors under 'prod', 'sum', 'sq'")
        surf = []
        for bit, nm in enumerate(names):
            t = out.get(nm)
            if not mask >> bit & 1:
                t = None
            elif t is None:
                t = torch.empty((n, K, D, D), dtype=torch.int64, device=self.device)
            elif not torch.is_tensor(t) or t.dtype != torch.int64 or not t.is_contiguous() or t.numel() < n * K * D * D:
                raise ValueError(f"out[{nm!r}] must be a contiguous int64 device tensor of at least n * K * D * D entries")
            surf.append(t)
        t64 = templates.to(torch.int64)
        if dtype == torch.int16:
            t64 = t64 & 0xFFFF
        pm = PatchMatch(surf[0], surf[1], surf[2], used, t64.sum((1, 2)), (t64 * t64).sum((1, 2)), tw, th, S)
        if results is None:
            results = torch.empty((max(n, 0), 4), dtype=torch.int64, device=self.device)
        if n == 0 or K == 0:   # nothing to do (empty tensors have no address to pass): the sizes are checked above
            return pm, results
        ptr = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
        rc = getattr(self.L, fn)(self.h, stream.data_ptr() + stream_offset, stream_bytes, offsets.data_ptr(), W, H, n,
                                 tw, th, S, K, origins.data_ptr(), ptr(counts), patch_edge_mode(edge), fill,
                                 templates.data_ptr(), Kt, mask, ptr(surf[0]), ptr(surf[1]), ptr(surf[2]),
                                 used.data_ptr(), ptr(results))
        self._check(rc, fn)
        return pm, results

    def match_patches(self, stream, stream_offset, stream_bytes, offsets, W, H, n, templates, S, origins, counts=None,
                      edge="clamp", fill=0, stats=("prod", "sum", "sq"), out=None, used=None, results=None):
        """Correlation surfaces of K templates over the shifts -S..S in x and y, per frame of n frames (frame f at
        stream.data_ptr()+stream_offset+offsets[f]), straight from the stream: no pixel is written.  templates: uint8
        device tensor (K, th, tw), or (1, th, tw) for one template shared by all patches.  origins: int32 (n, K, 2), the
        (x, y) of the SEARCH patches of (tw + 2S) x (th + 2S) pixels (registration.search_origins makes them from the
        templates' positions); counts, edge and fill as in decode_patches, a fill pixel counting like any other.
        stats: the surfaces wanted among "prod", "sum", "sq"; out: optional dict of int64 tensors to write them into;
        used: optional int32 (n, K, 2).  Returns (PatchMatch, results (n, 4) int64) like decode_frames."""
        return self._match_patches("dbde_hip_match_patches", torch.uint8, stream, stream_offset, stream_bytes, offsets, W,
                                   H, n, templates, S, origins, counts, edge, fill, stats, out, used, results)

    def match_patches16(self, stream, stream_offset, stream_bytes, offsets, W, H, n, templates, S, origins, counts=None,
                        edge="clamp", fill=0, stats=("prod", "sum", "sq"), out=None, used=None, results=None):
        """DBDE16 patch match: match_patches' arguments and results over U16 pixels; templates are int16 tensors holding
        the U16 bits (as decode_frames16 returns its images), fill up to 65535."""
        return self._match_patches("dbde16_hip_match_patches", torch.int16, stream, stream_offset, stream_bytes, offsets,
                                   W, H, n, templates, S, origins, counts, edge, fill, stats, out, used, results)

    def _crop_frames(self, fn, stream, stream_offset, stream_bytes, offsets, W, H, n, x, y, rw, rh, out, out_offset,
                     capacity, origins, slot_stride, out_offsets, out_bytes, origins_used, results):
        """crop_frames / crop_frames16 through the C function named fn."""
        if out_offsets is None:
            out_offsets = torch.empty(n, dtype=torch.int64, device=self.device)
        if out_bytes is None:
            out_bytes = torch.empty(n, dtype=torch.int64, device=self.device)
        if results is None:
            results = torch.empty((n, 4), dtype=torch.int64, device=self.device)
        rc = getattr(self.L, fn)(self.h, stream.data_ptr() + stream_offset, stream_bytes, offsets.data_ptr(),
                                 W, H, n, x, y, rw, rh, origins.data_ptr() if origins is not None else None,
                                 out.data_ptr() + out_offset, capacity, slot_stride, out_offsets.data_ptr(),
                                 out_bytes.data_ptr(),
                                 origins_used.data_ptr() if origins_used is not None else None, results.data_ptr())
        self._check(rc, fn)
        return out_offsets, out_bytes, results

    def crop_frames(self, stream, stream_offset, stream_bytes, offsets, W, H, n, x, y, rw, rh, out, out_offset,
                    capacity, origins=None, slot_stride=0, out_offsets=None, out_bytes=None, origins_used=None,
                    results=None):
        """Crops the rw x rh window at (x, y; multiples of 8) of n frames into n DBDE frames of an rw x rh image,
        written from out.data_ptr()+out_offset like encode_frames (alloc_stream(rw, rh, n, slot_stride) sizes `out`):
        tiles are copied in the compressed domain, only those the window's right / bottom edge cuts are re-packed.
        origins: optional int32 device tensor (n, 2) of per-frame (x, y), clamped into the frame and rounded down to
        a multiple of 8; origins_used (optional, same shape) receives the origin of each cropped frame.
        Returns (out_offsets, out_bytes, results): int64 device tensors; a rejected frame has 0 bytes."""
        return self._crop_frames("dbde_hip_crop_frames", stream, stream_offset, stream_bytes, offsets, W, H, n, x, y,
                                 rw, rh, out, out_offset, capacity, origins, slot_stride, out_offsets, out_bytes,
                                 origins_used, results)

    def crop_frames16(self, stream, stream_offset, stream_bytes, offsets, W, H, n, x, y, rw, rh, out, out_offset,
                      capacity, origins=None, slot_stride=0, out_offsets=None, out_bytes=None, origins_used=None,
                      results=None):
        """crop_frames for DBDE16 frames in and out (worst case per frame: dbde16_hip_max_frame_bytes(rw, rh))."""
        return self._crop_frames("dbde16_hip_crop_frames", stream, stream_offset, stream_bytes, offsets, W, H, n, x,
                                 y, rw, rh, out, out_offset, capacity, origins, slot_stride, out_offsets, out_bytes,
                                 origins_used, results)

    def _window_source(self, images, pix, x, y, rw, rh, origins, capacity, slot_stride):
        """(n, W, H, pitch, frame_stride, image_bytes, rw, rh) of a strided image tensor for the window encoders; raises
        DbdeError naming the rule the C call would reject it by."""
        dtypes = (torch.uint8,) if pix == 1 else (torch.int16, torch.uint16)
        if images.dtype not in dtypes:
            raise DbdeError(f"encode_window: images must be {' or '.join(str(d) for d in dtypes)}, not {images.dtype}")
        if not images.is_cuda or images.dim() not in (2, 3):
            raise DbdeError("encode_window: images must be a CUDA tensor of shape (n, H, W) or (H, W)")
        n = images.shape[0] if images.dim() == 3 else 1
        H, W = int(images.shape[-2]), int(images.shape[-1])
        if H < 1 or W < 1:
            raise DbdeError("encode_window: empty image")
        if W > 1 and images.stride(-1) != 1:
            raise DbdeError(f"encode_window: the innermost stride must be 1 (is {images.stride(-1)}): pixels of a row are adjacent")
        pitch = images.stride(-2) * pix if H > 1 else W * pix
        if pitch < W * pix:
            raise DbdeError(f"encode_window: pitch {pitch} below W * PIX = {W * pix} (rows overlap)")
        extent = (H - 1) * pitch + W * pix
        stride = images.stride(0) * pix if images.dim() == 3 and n > 1 else H * pitch
        if stride < extent:
            raise DbdeError(f"encode_window: frame stride {stride} below (H-1) * pitch + W * PIX = {extent} (frames overlap)")
        image_bytes = images.untyped_storage().nbytes() - images.storage_offset() * images.element_size()
        rw = W - x if rw is None else rw
        rh = H - y if rh is None else rh
        if not (1 <= rw <= W and 1 <= rh <= H):
            raise DbdeError(f"encode_window: window size {rw}x{rh} outside [1, {W}] x [1, {H}]")
        if not (0 <= x <= W - rw and 0 <= y <= H - rh):
            raise DbdeError(f"encode_window: window origin ({x}, {y}) outside [0, {W - rw}] x [0, {H - rh}]")
        if origins is not None and (origins.dtype != torch.int32 or tuple(origins.shape) != (n, 2) or not origins.is_contiguous()):
            raise DbdeError("encode_window: origins must be a contiguous int32 tensor of shape (n, 2)")
        fn = "dbde_hip_window_encode_plan" if pix == 1 else "dbde16_hip_window_encode_plan"
        pl = WindowEncodePlan()
        rc = getattr(self.L, fn)(images.data_ptr(), image_bytes, W, H, pitch, stride, n, x, y, rw, rh,
                                 0 if origins is None else 1, 0, 0, 1, C.byref(pl))
        if rc != OK:
            raise DbdeError(f"encode_window: {fn} rejects the source ({rc}): image_bytes {image_bytes} below "
                            f"{(n - 1) * stride + extent}, or too many tiles / chunks in one call")
        if slot_stride and slot_stride < pl.max_out_frame_bytes:
            raise DbdeError(f"encode_window: slot_stride {slot_stride} below the window's worst case {pl.max_out_frame_bytes}")
        need = (n - 1) * slot_stride + pl.max_out_frame_bytes if slot_stride else n * pl.max_out_frame_bytes
        if capacity < need:
            raise DbdeError(f"encode_window: capacity {capacity} below the worst case {need}")
        return n, W, H, pitch, stride, image_bytes, rw, rh

    def encode_window(self, images, out, out_offset, capacity, x=0, y=0, rw=None, rh=None, origins=None, first_index=0,
                      indices=None, elapsed_ns=None, slot_stride=0, offsets=None, nbytes=None):
        """Encodes the rw x rh window at (x, y) of each image of `images` -- a uint8 CUDA tensor (n, H, W) or (H, W) whose
        innermost stride is 1; any other strides are taken as they are, so a sliced view such as frames[:, 3:34, 5:38]
        goes in without a copy (pitch, frame stride and the readable extent come from the tensor's strides and storage).
        Frames are written from out.data_ptr()+out_offset exactly as encode_frames writes the window's contiguous copy
        (alloc_stream(rw, rh, n, slot_stride) sizes `out`).  origins: optional int32 device tensor (n, 2) of per-frame
        (x, y), clamped into the source.  rw / rh default to the rest of the image.  Anything the C call would reject
        raises DbdeError before it.  Returns (offsets, nbytes) int64 device tensors."""
        n, W, H, pitch, stride, image_bytes, rw, rh = self._window_source(images, 1, x, y, rw, rh, origins, capacity, slot_stride)
        if offsets is None:
            offsets = torch.empty(n, dtype=torch.int64, device=self.device)
        if nbytes is None:
            nbytes = torch.empty(n, dtype=torch.int64, device=self.device)
        rc = self.L.dbde_hip_encode_window(
            self.h, images.data_ptr(), image_bytes, W, H, pitch, stride, n, x, y, rw, rh,
            origins.data_ptr() if origins is not None else None, first_index,
            indices.data_ptr() if indices is not None else None,
            elapsed_ns.data_ptr() if elapsed_ns is not None else None,
            out.data_ptr() + out_offset, capacity, slot_stride, offsets.data_ptr(), nbytes.data_ptr())
        self._check(rc, "dbde_hip_encode_window")
        return offsets, nbytes

    def encode_window16(self, images, out, out_offset, capacity, x=0, y=0, rw=None, rh=None, origins=None, first_index=0,
                        slot_stride=0, offsets=None, nbytes=None):
        """encode_window for int16 / uint16 images, DBDE16 frames out (worst case per frame:
        dbde16_hip_max_frame_bytes(rw, rh)); no indices / elapsed_ns, as encode_frames16 has none."""
        n, W, H, pitch, stride, image_bytes, rw, rh = self._window_source(images, 2, x, y, rw, rh, origins, capacity, slot_stride)
        if offsets is None:
            offsets = torch.empty(n, dtype=torch.int64, device=self.device)
        if nbytes is None:
            nbytes = torch.empty(n, dtype=torch.int64, device=self.device)
        rc = self.L.dbde16_hip_encode_window(
            self.h, images.data_ptr(), image_bytes, W, H, pitch, stride, n, x, y, rw, rh,
            origins.data_ptr() if origins is not None else None, first_index,
            out.data_ptr() + out_offset, capacity, slot_stride, offsets.data_ptr(), nbytes.data_ptr())
        self._check(rc, "dbde16_hip_encode_window")
        return offsets, nbytes

    def trace_map(self, labels, n_labels=None):
        """A TraceMap of this codec from a label image (H, W): numpy, or a torch tensor on any device; 0 = no region,
        1..n_labels = region ids, n_labels defaulting to labels.max()."""
        m = TraceMap(self, labels, n_labels)
        if not hasattr(self, "_trace_maps"):
            self._trace_maps = weakref.WeakSet()
        self._trace_maps.add(m)
        return m

    def _traces(self, fn, pix, stream, stream_offset, stream_bytes, offsets, W, H, n, tmap, stats, out, results):
        """traces / traces16 through the C function named fn; pix: bytes per value of max / min."""
        if out is None:
            out = Traces.empty(n, tmap.n_labels, stats, self.device, pix=pix, pixels=tmap.pixels)
        if results is None:
            results = torch.empty((max(n, 0), 4), dtype=torch.int64, device=self.device)
        ptr = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
        rc = getattr(self.L, fn)(self.h, stream.data_ptr() + stream_offset, stream_bytes, offsets.data_ptr(), W, H, n,
                                 tmap.h, ptr(out.max), ptr(out.min), ptr(out.sum), ptr(out.sumsq),
                                 ptr(results) if n > 0 else None)
        self._check(rc, fn)
        return out, results

    def traces(self, stream, stream_offset, stream_bytes, offsets, W, H, n, tmap, stats=("max", "min", "sum", "sumsq"),
               out=None, results=None):
        """Region traces of n frames (frame f at stream.data_ptr()+stream_offset+offsets[f]) over the TraceMap tmap:
        per frame and label, the max, min, sum and sum of squares of the label's pixels.  out: a Traces to write into
        (its statistics are the ones computed); a rejected frame's rows are left as they were.  Returns
        (Traces (n, n_labels), results (n, 4) int64) like decode_frames."""
        return self._traces("dbde_hip_traces", 1, stream, stream_offset, stream_bytes, offsets, W, H, n, tmap, stats,
                            out, results)

    def index_stream(self, stream, stream_offset, stream_bytes, W, H, max_frames):
        offsets = torch.empty(max(max_frames, 1), dtype=torch.int64, device=self.device)
        n = C.c_int(0)
        rc = self.L.dbde_hip_index_stream(self.h, stream.data_ptr() + stream_offset, stream_bytes, W, H,
                                          max_frames, offsets.data_ptr(), C.byref(n))
        self._check(rc, "dbde_hip_index_stream")
        return offsets[:n.value], n.value

    def index_stream_async(self, stream, stream_offset, stream_bytes, W, H, max_frames, offsets, count=None):
        """Enqueues the frame-to-frame walk; offsets (int64 device tensor, >= max_frames) and the device
        word `count` (int32 tensor, 1 element) are valid once the stream reaches this point."""
        if count is None:
            count = torch.empty(1, dtype=torch.int32, device=self.device)
        rc = self.L.dbde_hip_index_stream_async(self.h, stream.data_ptr() + stream_offset, stream_bytes, W, H,
                                                max_frames, offsets.data_ptr(), count.data_ptr())
        self._check(rc, "dbde_hip_index_stream_async")
        return offsets, count

    def scan_ahead(self, stream, stream_offset, stream_bytes, W, H, max_frames, cursor, offsets, count):
        """Enqueues the walk of the next batch on the context's second stream (see dbde_hip.h): `cursor`
        (int64 device tensor, 1 element, zeroed before the first call) is advanced past the frames found."""
        rc = self.L.dbde_hip_scan_ahead(self.h, stream.data_ptr() + stream_offset, stream_bytes, W, H, max_frames,
                                        cursor.data_ptr(), offsets.data_ptr(), count.data_ptr())
        self._check(rc, "dbde_hip_scan_ahead")

    def scan_join(self):
        self._check(self.L.dbde_hip_scan_join(self.h), "dbde_hip_scan_join")

    @staticmethod
    def parse_results(results):
        """results tensor (n,4) int64 -> list of (u64s, index, elapsed_ns, consumed)."""
        r = results.cpu().numpy().view(np.uint64)
        return [(int(a) & 0xFFFFFFFF, int(b), int(c), int(d)) for a, b, c, d in r]

    # ---- DBDE16 (higher-bit-depth extension, parity unpinned) ---------------------------------
    def encode_frames16(self, images, W, H, n, out, out_offset, capacity, first_index=0, slot_stride=0):
        """images: int16/uint16-sized device tensor of n*H*W pixels.  Returns (offsets, nbytes) int64 device tensors."""
        offsets = torch.empty(n, dtype=torch.int64, device=self.device)
        nbytes = torch.empty(n, dtype=torch.int64, device=self.device)
        rc = self.L.dbde16_hip_encode_frames(self.h, images.data_ptr(), W, H, n, first_index, out.data_ptr() + out_offset,
                                             capacity, slot_stride, offsets.data_ptr(), nbytes.data_ptr())
        self._check(rc, "dbde16_hip_encode_frames")
        return offsets, nbytes

    def decode_frames16(self, stream, stream_offset, stream_bytes, offsets, W, H, n, images=None):
        if images is None:
            images = torch.empty((n, H, W), dtype=torch.int16, device=self.device)
        results = torch.empty((n, 4), dtype=torch.int64, device=self.device)
        rc = self.L.dbde16_hip_decode_frames(self.h, stream.data_ptr() + stream_offset, stream_bytes, offsets.data_ptr(),
                                             W, H, n, images.data_ptr(), results.data_ptr())
        self._check(rc, "dbde16_hip_decode_frames")
        return images, results

    def decode_roi16(self, stream, stream_offset, stream_bytes, offsets, W, H, n, x, y, rw, rh, origins=None, out=None,
                     results=None):
        """DBDE16 window decode: the rw x rh window at (x, y) of n frames (frame f at
        stream.data_ptr()+stream_offset+offsets[f]); origins as in decode_roi.  Returns (windows int16 (n, rh, rw)
        holding the U16 bits, as decode_frames16 does; results (n, 4) int64)."""
        return self._decode_roi("dbde16_hip_decode_roi", torch.int16, stream, stream_offset, stream_bytes, offsets, W,
                                H, n, x, y, rw, rh, origins, out, results)

    def project16(self, stream, stream_offset, stream_bytes, offsets, W, H, n, x=0, y=0, rw=None, rh=None,
                  stats=("max", "min", "sum", "sumsq"), out=None, accumulate=False, results=None):
        """DBDE16 temporal projection: project's arguments and results, with max / min as int16 tensors holding the
        U16 bits (Projection.empty(..., pix=2)).  .to(torch.int32) & 0xFFFF gives their values."""
        return self._project("dbde16_hip_project", 2, stream, stream_offset, stream_bytes, offsets, W, H, n, x, y, rw,
                             rh, stats, out, accumulate, results)

    def traces16(self, stream, stream_offset, stream_bytes, offsets, W, H, n, tmap,
                 stats=("max", "min", "sum", "sumsq"), out=None, results=None):
        """DBDE16 region traces: traces' arguments and results, with max / min as int16 tensors holding the U16 bits
        (Traces.empty(..., pix=2)).  .to(torch.int32) & 0xFFFF gives their values."""
        return self._traces("dbde16_hip_traces", 2, stream, stream_offset, stream_bytes, offsets, W, H, n, tmap, stats,
                            out, results)

    # ---- host-pointer API: the reference's functions -------------------------------------
    def pack_frame(self, index, image, W, H):
        src = np.ascontiguousarray(image, np.uint8).reshape(-1)
        out = np.full(max_frame_bytes(W, H) + 64, 0xEE, np.uint8)
        n = self.L.dbde_hip_pack_frame(self.h, index, src.ctypes.data, W, H, out.ctypes.data)
        assert (out[n:] == 0xEE).all(), "wrote past the returned size"
        return out[:n].copy()

    def pack_image(self, image, W, H):
        src = np.ascontiguousarray(image, np.uint8).reshape(-1)
        out = np.full(max_frame_bytes(W, H) + 64, 0xEE, np.uint8)
        n = self.L.dbde_hip_pack_image(self.h, src.ctypes.data, W, H, out.ctypes.data)
        assert (out[n:] == 0xEE).all(), "wrote past the returned size"
        return out[:n].copy()

    def unpack_image(self, packed, W, H, fill=0xEE):
        img = np.full(W * H, fill, np.uint8)
        buf = np.concatenate([np.asarray(packed, np.uint8), np.zeros(64, np.uint8)])
        n = self.L.dbde_hip_unpack_image(self.h, buf.ctypes.data, W, H, img.ctypes.data)
        return int(n), img.reshape(H, W)

    def unpack_image_roi(self, packed, W, H, x, y, rw, rh, fill=0xEE):
        """dbde_hip_unpack_image_roi: one packed frame_data -> (bytes consumed, the rh x rw window)."""
        win = np.full(max(rw, 0) * max(rh, 0), fill, np.uint8)
        buf = np.concatenate([np.asarray(packed, np.uint8), np.zeros(64, np.uint8)])
        n = self.L.dbde_hip_unpack_image_roi(self.h, buf.ctypes.data, W, H, x, y, rw, rh, win.ctypes.data)
        return int(n), win.reshape(max(rh, 0), max(rw, 0))

    def unpack_frame(self, packed, W, H, fill=0xEE):
        img = np.full(W * H, fill, np.uint8)
        buf = np.concatenate([np.asarray(packed, np.uint8), np.zeros(64, np.uint8)])
        cur = C.c_void_p(buf.ctypes.data)
        fh = self.L.dbde_hip_unpack_frame(self.h, C.byref(cur), W, H, img.ctypes.data)
        return cur.value - buf.ctypes.data, (fh.u64s, fh.index, fh.elapsed_ns), img.reshape(H, W)

    def pack_8x8(self, image, off, stride):
        out = np.full(64 + 16, 0xEE, np.uint8)
        code = self.L.dbde_hip_pack_8x8(self.h, image.ctypes.data + off, stride, out.ctypes.data)
        return int(code), out[:8 * (code >> 8)].copy(), out

    def pack_8x8_partial(self, image, off, stride, rm, dm):
        out = np.full(64 + 16, 0xEE, np.uint8)
        code = self.L.dbde_hip_pack_8x8_partial(self.h, image.ctypes.data + off, stride, rm, dm, out.ctypes.data)
        return int(code), out[:8 * (code >> 8)].copy(), out

    def unpack_8x8(self, depth, minval, packed, stride, canvas, off=0):
        buf = np.zeros(64 + 8, np.uint8)
        buf[:len(packed)] = packed
        self.L.dbde_hip_unpack_8x8(self.h, depth, minval, buf.ctypes.data, stride, canvas.ctypes.data + off)
        return canvas

    def unpack_8x8_partial(self, depth, minval, packed, stride, rm, dm, canvas, off=0):
        buf = np.zeros(64 + 8, np.uint8)
        buf[:len(packed)] = packed
        self.L.dbde_hip_unpack_8x8_partial(self.h, depth, minval, buf.ctypes.data, stride, rm, dm,
                                           canvas.ctypes.data + off)
        return canvas

    # ---- .dbde files: batched writer / reader (include/dbde_hip.h, file I/O) ----------------
    def open_writer(self, path, W, H, frame_hz=30.0, batch_frames=16):
        return FileWriter(self, path, W, H, frame_hz, batch_frames)

    def open_reader(self, path, batch_frames=16):
        return FileReader(self, path, batch_frames)

    # ---- timing hook ------------------------------------------------------------------
    def timing(self, on=True):
        self._check(self.L.dbde_hip_timing_enable(self.h, 1 if on else 0), "dbde_hip_timing_enable")

    def timing_read(self, reset=True):
        ms = (C.c_double * 4)()
        n = (C.c_uint64 * 4)()
        self._check(self.L.dbde_hip_timing_read(self.h, ms, n, 1 if reset else 0), "dbde_hip_timing_read")
        return {"encode": (ms[0], n[0]), "decode_index": (ms[1], n[1]), "decode": (ms[2], n[2]), "scan": (ms[3], n[3])}


class Gather:
    """dbde_hip_gather_*: this rank's end of the variable-length gather of the compressed stream (RCCL).
    `unique_id`: 128 uint8 (gather_unique_id() on one rank, handed to the others), or pass `comm`=an ncclComm_t."""

    def __init__(self, codec, unique_id, nranks, rank, root=0, comm=None, max_message_bytes=None):
        self.codec, self.nranks, self.rank, self.root = codec, nranks, rank, root
        self.h = C.c_void_p()
        if comm is not None:
            rc = codec.L.dbde_hip_gather_attach(codec.h, C.c_void_p(comm), nranks, rank, root, C.byref(self.h))
        else:
            uid = np.ascontiguousarray(np.asarray(unique_id, np.uint8))
            assert uid.size == GATHER_ID_BYTES
            rc = codec.L.dbde_hip_gather_create(codec.h, uid.ctypes.data, nranks, rank, root, C.byref(self.h))
        if rc != OK or not self.h.value:
            raise DbdeError(f"dbde_hip_gather_create failed ({rc})")
        if max_message_bytes:
            self._check(codec.L.dbde_hip_gather_set_max_message(self.h, int(max_message_bytes)), "set_max_message")

    def _check(self, rc, what):
        if rc != OK:
            raise DbdeError(f"dbde_hip_gather_{what} failed ({rc}): {self.codec.L.dbde_hip_gather_error(self.h).decode()}")

    def set_window(self, window_bytes):
        """Root: the bytes its window holds; travels with every size exchange so that an overflow is ONE verdict on all ranks."""
        self._check(self.codec.L.dbde_hip_gather_set_window(self.h, int(window_bytes)), "set_window")

    def begin(self, slot, last_offset, last_bytes):
        """last_offset / last_bytes: 1-element int64 device tensors (views of the encoder's outputs) or None."""
        self._check(self.codec.L.dbde_hip_gather_begin(self.h, slot, last_offset.data_ptr() if last_offset is not None else None,
                                                       last_bytes.data_ptr() if last_bytes is not None else None), "begin")

    def post(self, slot, segment, segment_offset, window, window_offset, window_bytes, loopback=False):
        """-> list of every rank's byte count.  segment / window: uint8 device tensors (either may be None where the
        rank does not need it)."""
        sizes = (C.c_uint64 * self.nranks)()
        seg = segment.data_ptr() + segment_offset if segment is not None else None
        win = window.data_ptr() + window_offset if window is not None else None
        self._check(self.codec.L.dbde_hip_gather_post(self.h, slot, seg, win, window_bytes, sizes,
                                                      GATHER_LOOPBACK if loopback else 0), "post")
        return [int(x) for x in sizes]

    def join(self, slot):
        self._check(self.codec.L.dbde_hip_gather_join(self.h, slot), "join")

    def sync(self, slot):
        self._check(self.codec.L.dbde_hip_gather_sync(self.h, slot), "sync")

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            self.codec.L.dbde_hip_gather_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Scatter:
    """dbde_hip_scatter_*: this rank's end of the scatter of a .dbde body to the ranks' frame blocks (RCCL): the decode-side
    mirror of Gather.  `unique_id` as for Gather, or `comm` = an ncclComm_t."""

    def __init__(self, codec, unique_id, nranks, rank, root=0, comm=None, max_message_bytes=None):
        self.codec, self.nranks, self.rank, self.root = codec, nranks, rank, root
        self.h = C.c_void_p()
        if comm is not None:
            rc = codec.L.dbde_hip_scatter_attach(codec.h, C.c_void_p(comm), nranks, rank, root, C.byref(self.h))
        else:
            uid = np.ascontiguousarray(np.asarray(unique_id, np.uint8))
            assert uid.size == GATHER_ID_BYTES
            rc = codec.L.dbde_hip_scatter_create(codec.h, uid.ctypes.data, nranks, rank, root, C.byref(self.h))
        if rc != OK or not self.h.value:
            raise DbdeError(f"dbde_hip_scatter_create failed ({rc})")
        if max_message_bytes:
            self._check(codec.L.dbde_hip_scatter_set_max_message(self.h, int(max_message_bytes)), "set_max_message")

    def _check(self, rc, what):
        if rc != OK:
            raise DbdeError(f"dbde_hip_scatter_{what} failed ({rc}): {self.codec.L.dbde_hip_scatter_error(self.h).decode()}")

    def set_capacity(self, segment_bytes, max_frames):
        self._check(self.codec.L.dbde_hip_scatter_set_capacity(self.h, int(segment_bytes), int(max_frames)), "set_capacity")

    def begin(self, slot, stream=None, stream_offset=0, stream_bytes=0, offsets=None, count=None):
        """Root: the stream (uint8 device tensor), its extent, the scanner's offsets (int64) and count (int32, 1 element)."""
        self._check(self.codec.L.dbde_hip_scatter_begin(
            self.h, slot, stream.data_ptr() + stream_offset if stream is not None else None, int(stream_bytes),
            offsets.data_ptr() if offsets is not None else None, count.data_ptr() if count is not None else None), "begin")

    def post(self, slot, segment, offsets_out, loopback=False):
        """-> (mine, table): (first_frame, n_frames, byte_start, byte_count) of this rank and of every rank."""
        mine, table = ScatterBlock(), (ScatterBlock * self.nranks)()
        self._check(self.codec.L.dbde_hip_scatter_post(self.h, slot, segment.data_ptr() if segment is not None else None,
                                                       offsets_out.data_ptr(), C.byref(mine), table,
                                                       SCATTER_LOOPBACK if loopback else 0), "post")
        t = lambda b: (int(b.first_frame), int(b.n_frames), int(b.byte_start), int(b.byte_count))
        return t(mine), [t(b) for b in table]

    def join(self, slot):
        self._check(self.codec.L.dbde_hip_scatter_join(self.h, slot), "join")

    def sync(self, slot):
        self._check(self.codec.L.dbde_hip_scatter_sync(self.h, slot), "sync")

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            self.codec.L.dbde_hip_scatter_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FileWriter:
    """dbde_hip_writer_*: appends device-resident frames to a .dbde file, a batch per launch."""

    def __init__(self, codec, path, W, H, frame_hz, batch_frames):
        self.codec, self.W, self.H = codec, W, H
        self.h = C.c_void_p()
        rc = codec.L.dbde_hip_writer_open(codec.h, os.fsencode(path), W, H, frame_hz, batch_frames, C.byref(self.h))
        if rc != OK:
            raise DbdeError(f"dbde_hip_writer_open({path!r}) failed ({rc})")

    def put(self, images, n, first_index=0, indices=None, elapsed_ns=None):
        rc = self.codec.L.dbde_hip_writer_put(self.h, images.data_ptr(), n, first_index,
                                              indices.data_ptr() if indices is not None else None,
                                              elapsed_ns.data_ptr() if elapsed_ns is not None else None)
        if rc != OK:
            raise DbdeError(f"dbde_hip_writer_put failed ({rc}): {self.codec.L.dbde_hip_writer_error(self.h).decode()}")

    def put_window(self, images, x=0, y=0, origins=None, first_index=0, indices=None, elapsed_ns=None):
        """Appends the writer-sized (W x H) window at (x, y) of each image of a strided uint8 CUDA tensor (n, SH, SW) or
        (SH, SW), as Codec.encode_window takes it (dbde_hip_writer_put_window)."""
        cap = 1 << 62   # the writer's own windows are sized for the worst case
        n, SW, SH, pitch, stride, image_bytes, _, _ = self.codec._window_source(images, 1, x, y, self.W, self.H, origins, cap, 0)
        rc = self.codec.L.dbde_hip_writer_put_window(self.h, images.data_ptr(), image_bytes, SW, SH, pitch, stride, n, x, y,
                                                     origins.data_ptr() if origins is not None else None, first_index,
                                                     indices.data_ptr() if indices is not None else None,
                                                     elapsed_ns.data_ptr() if elapsed_ns is not None else None)
        if rc != OK:
            raise DbdeError(f"dbde_hip_writer_put_window failed ({rc}): {self.codec.L.dbde_hip_writer_error(self.h).decode()}")

    def close(self):
        """Returns (frames written, file bytes)."""
        if not self.h.value:
            return None
        fr, by = C.c_uint64(0), C.c_uint64(0)
        rc = self.codec.L.dbde_hip_writer_close(self.h, C.byref(fr), C.byref(by))
        self.h = C.c_void_p()
        if rc != OK:
            raise DbdeError(f"dbde_hip_writer_close failed ({rc})")
        return fr.value, by.value

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class FileReader:
    """dbde_hip_reader_*: walks a .dbde file a batch at a time, images land in HBM."""

    def __init__(self, codec, path, batch_frames):
        self.codec, self.batch = codec, batch_frames
        self.h = C.c_void_p()
        vh = VideoHeader()
        rc = codec.L.dbde_hip_reader_open(codec.h, os.fsencode(path), batch_frames, C.byref(vh), C.byref(self.h))
        if rc != OK:
            raise DbdeError(f"dbde_hip_reader_open({path!r}) failed ({rc})")
        self.video_header = (vh.u64s, vh.height, vh.width, vh.frame_hz)
        self.W, self.H = int(vh.width), int(vh.height)

    def next(self, max_frames=None, images=None):
        """-> (images[:n] device tensor, [(u64s, index, elapsed_ns)] * n); n == 0 ends the walk."""
        m = self.batch if max_frames is None else min(max_frames, self.batch)
        if images is None:
            images = torch.empty((m, self.H, self.W), dtype=torch.uint8, device=self.codec.device)
        hdr = (FrameHeader * max(m, 1))()
        n = C.c_int(0)
        rc = self.codec.L.dbde_hip_reader_next(self.h, images.data_ptr(), m, hdr, C.byref(n))
        if rc != OK:
            raise DbdeError(f"dbde_hip_reader_next failed ({rc}): {self.codec.L.dbde_hip_last_error(self.codec.h).decode()}")
        return images[:n.value], [(hdr[k].u64s, hdr[k].index, hdr[k].elapsed_ns) for k in range(n.value)]

    def __iter__(self):
        while True:
            imgs, hdrs = self.next()
            if not hdrs:
                return
            yield imgs, hdrs

    def close(self):
        if self.h.value:
            self.codec.L.dbde_hip_reader_close(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
