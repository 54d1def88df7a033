"""Host-side mirror of the reference's public surface, bound to libfelics over its C ABI.

Reference items mirrored (paths relative to the reference repository):
  ColorType, PixelDepth, Header, read_header, write_header   src/compression/format.rs:8-84
  DecompressionError                                          src/compression/error.rs:4-19
  CompressDecompress::{compress, decompress}                 src/compression/traits.rs:47-65
  compress_image, decompress_image                            src/compression.rs:412-441

An image is a numpy array: (H, W) for Luma, (H, W, 3) for Rgb; dtype uint8 or uint16 -- the
same four types the trait is implemented for (compression.rs:250, :317).  `to` / `from_` are
binary file objects, standing in for `W: Write` / `R: Read`.

Encode runs on the GPU through the C ABI; this module has no other encode path and raises
FelicsError if the HIP device or libfelics.so is missing.
"""
import collections
import ctypes as C
import enum
import importlib.util
import io
import os

import numpy as np

from . import build as _build


class ColorType(enum.IntEnum):  # format.rs:8-12
    Gray = 0
    Rgb = 1


class PixelDepth(enum.IntEnum):  # format.rs:27-31
    Eight = 0
    Sixteen = 1


class FelicsError(RuntimeError):
    """Any non-zero code of the C ABI."""

    def __init__(self, code, detail=""):
        self.code = code
        msg = lib().felics_strerror(code).decode()
        super().__init__("felics error %d: %s%s" % (code, msg, (" (" + detail + ")") if detail else ""))


class DecompressionError(FelicsError):
    """error.rs:4-19; `.kind` is the variant name."""

    KINDS = {-1: "IoError", -2: "InvalidValue", -3: "ValueOverflow", -4: "InvalidDimensions",
             -5: "InvalidColorType", -6: "InvalidPixelDepth", -7: "InvalidSignature"}

    def __init__(self, code):
        super().__init__(code)
        self.kind = self.KINDS.get(code, "Other")


class _CHeader(C.Structure):
    _fields_ = [("color_type", C.c_uint8), ("pixel_depth", C.c_uint8),
                ("width", C.c_uint32), ("height", C.c_uint32)]


class _CStats(C.Structure):
    _fields_ = [("submissions", C.c_uint64), ("ticket_retries", C.c_uint64), ("slot_overflows", C.c_uint64), ("lookback_fallbacks", C.c_uint64),
                ("two_pass", C.c_int), ("failed", C.c_int), ("scatter_fallbacks", C.c_uint64), ("sorted_event_sorts", C.c_uint64),
                ("tile_overflows", C.c_uint64)]


class _CImage(C.Structure):  # felics_image
    _fields_ = [("pixels", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32), ("color", C.c_int), ("depth", C.c_int)]


class _CView(C.Structure):  # felics_view
    _fields_ = [("data", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32), ("color", C.c_int), ("depth", C.c_int),
                ("row_stride", C.c_int64), ("pixel_stride", C.c_int64), ("channel_stride", C.c_int64)]


class _CViewStats(C.Structure):  # felics_view_stats
    _fields_ = [("views", C.c_uint64), ("dense", C.c_uint64), ("in_place", C.c_uint64), ("gathered", C.c_uint64),
                ("bytes_staged", C.c_uint64)]


class _CSurfaces(C.Structure):  # felics_surfaces
    _fields_ = [("frame0", _CView), ("frame_stride", C.c_int64), ("count", C.c_uint64)]


class _CSurfaceStats(C.Structure):  # felics_surface_stats
    _fields_ = [("submissions", C.c_uint64), ("queued", C.c_uint64), ("immediate", C.c_uint64), ("frames_in_place", C.c_uint64),
                ("frames_gathered", C.c_uint64), ("bytes_staged", C.c_uint64)]


class _CDecodeViewStats(C.Structure):  # felics_decode_view_stats
    _fields_ = [("views", C.c_uint64), ("dense", C.c_uint64), ("in_place", C.c_uint64), ("scattered", C.c_uint64),
                ("bytes_staged", C.c_uint64)]


class _CDecodeStats(C.Structure):  # felics_decode_stats
    _fields_ = [("streams", C.c_uint64), ("wave8", C.c_uint64), ("lanes8", C.c_uint64), ("wave16", C.c_uint64), ("lanes16", C.c_uint64),
                ("host", C.c_uint64), ("undecoded", C.c_uint64), ("lanes16_table_bytes", C.c_uint64)]


class _CIndexStats(C.Structure):  # felics_index_stats
    _fields_ = [("streams", C.c_uint64), ("segments8", C.c_uint64), ("lane_segments8", C.c_uint64), ("lane_passes", C.c_uint64)]


class _CIndexViewStats(C.Structure):  # felics_index_view_stats
    _fields_ = [("streams", C.c_uint64), ("undecoded", C.c_uint64), ("items", C.c_uint64), ("launches", C.c_uint64), ("passes", C.c_uint64),
                ("plane_bytes", C.c_uint64)]


class _CIndex16Stats(C.Structure):  # felics_index16_stats
    _fields_ = [("streams", C.c_uint64), ("segments16", C.c_uint64), ("passes", C.c_uint64), ("rows_loaded", C.c_uint64),
                ("table_bytes", C.c_uint64)]


class _CIndex16ViewStats(C.Structure):  # felics_index16_view_stats
    _fields_ = [("streams", C.c_uint64), ("undecoded", C.c_uint64), ("items", C.c_uint64), ("launches", C.c_uint64), ("passes", C.c_uint64),
                ("rows_loaded", C.c_uint64), ("plane_bytes", C.c_uint64), ("table_bytes", C.c_uint64)]


class _CIndex16EmitStats(C.Structure):  # felics_index16_emit_stats
    _fields_ = [("streams", C.c_uint64), ("rows_written", C.c_uint64), ("index_bytes", C.c_uint64), ("passes", C.c_uint64)]


class _CIndex16ViewEmitStats(C.Structure):  # felics_index16_view_emit_stats
    _fields_ = [("views", C.c_uint64), ("indexes", C.c_uint64), ("rows_written", C.c_uint64), ("index_bytes", C.c_uint64),
                ("sub_batches", C.c_uint64), ("shapes_max", C.c_uint64), ("redone", C.c_uint64)]


class _CIndexEmitStats(C.Structure):  # felics_index_emit_stats
    _fields_ = [("indexes", C.c_uint64), ("checkpoints", C.c_uint64), ("in_mixed", C.c_uint64), ("redone", C.c_uint64)]


class _CRegion(C.Structure):  # felics_region
    _fields_ = [("stream", C.c_uint32), ("x", C.c_uint32), ("y", C.c_uint32), ("w", C.c_uint32), ("h", C.c_uint32)]


class _CRegionStats(C.Structure):  # felics_region_stats
    _fields_ = [("regions", C.c_uint64), ("segments_walked", C.c_uint64), ("segments_skipped", C.c_uint64), ("pixels_walked", C.c_uint64)]


class _CRegion16Stats(C.Structure):  # felics_region16_stats
    _fields_ = [("regions", C.c_uint64), ("segments_walked", C.c_uint64), ("segments_skipped", C.c_uint64), ("pixels_walked", C.c_uint64),
                ("rows_loaded", C.c_uint64), ("passes", C.c_uint64)]


class _CRegionViewStats(C.Structure):  # felics_region_view_stats
    _fields_ = [("regions", C.c_uint64), ("undecoded", C.c_uint64), ("segments_walked", C.c_uint64), ("segments_skipped", C.c_uint64),
                ("pixels_walked", C.c_uint64), ("launches", C.c_uint64), ("passes", C.c_uint64), ("plane_bytes", C.c_uint64)]


class _CRegion16ViewStats(C.Structure):  # felics_region16_view_stats
    _fields_ = _CRegionViewStats._fields_ + [("rows_loaded", C.c_uint64), ("table_bytes", C.c_uint64)]


INDEX_GRANULE = 4096  # FELICS_INDEX_GRANULE
E_INVALID_INDEX = -12


class Header:  # format.rs:44-49
    def __init__(self, color_type, pixel_depth, width, height):
        self.color_type = ColorType(color_type)
        self.pixel_depth = PixelDepth(pixel_depth)
        self.width = int(width)
        self.height = int(height)

    def __eq__(self, other):
        return (self.color_type, self.pixel_depth, self.width, self.height) == (
            other.color_type, other.pixel_depth, other.width, other.height)

    def __repr__(self):
        return "Header(%s, %s, %d, %d)" % (self.color_type.name, self.pixel_depth.name, self.width, self.height)


IndexedStreams16 = collections.namedtuple("IndexedStreams16", "streams offsets lens index idx_offsets idx_lens")

EXPORTS = [
    "felics_ctx_create", "felics_ctx_destroy", "felics_max_compressed_size", "felics_compress",
    "felics_compress_batch", "felics_compress_batch_device", "felics_submit_batch_device", "felics_wait_batch",
    "felics_read_header", "felics_write_header",
    "felics_decompress", "felics_strerror", "felics_last_error", "felics_set_profiling",
    "felics_stage_count", "felics_stage_name", "felics_get_stage_ms", "felics_get_stage_launches",
    "felics_lane_count", "felics_ctx_lane_count", "felics_get_span_ms", "felics_decompress_with_header", "felics_get_stats", "felics_decompress_batch_device",
    "felics_compress_images", "felics_compress_images_device", "felics_read_headers_device",
    "felics_decompress_images_device",
    "felics_compress_views_device", "felics_view_extent", "felics_get_view_stats",
    "felics_get_decode_stats", "felics_decode_lanes_min_streams",
    "felics_decompress_views_device", "felics_view_writable", "felics_get_decode_view_stats",
    "felics_surfaces_extent", "felics_submit_surfaces_device", "felics_compress_surfaces_device", "felics_get_surface_stats",
    "felics_index_size", "felics_index_build", "felics_decompress_indexed", "felics_decompress_batch_device_indexed",
    "felics_get_index_stats", "felics_compress_batch_device_indexed", "felics_index_lanes_min_items",
    "felics_region_segments", "felics_decompress_region_indexed", "felics_decompress_regions_device_indexed", "felics_get_region_stats",
    "felics_decompress_views_device_indexed", "felics_decompress_indexed_view", "felics_get_index_view_stats",
    "felics_index_plan", "felics_compress_views_device_indexed", "felics_get_index_emit_stats",
    "felics_index_wide_size_max", "felics_index_wide_build", "felics_decompress_indexed_wide", "felics_decompress_batch_device_indexed_wide",
    "felics_get_index_wide_stats",
    "felics_compress_batch_device_indexed_wide", "felics_get_index_wide_emit_stats",
    "felics_decompress_region_indexed_wide", "felics_decompress_regions_device_indexed_wide", "felics_get_region_wide_stats",
    "felics_decompress_views_device_indexed_wide", "felics_decompress_indexed_view_wide", "felics_get_index_view_wide_stats",
    "felics_compress_views_device_indexed_wide", "felics_get_index_view_wide_emit_stats",
    "felics_decompress_region_views_device_indexed", "felics_decompress_region_views_device_indexed_wide",
    "felics_decompress_region_indexed_view", "felics_decompress_region_indexed_view_wide",
    "felics_get_region_view_stats", "felics_get_region_view_wide_stats",
]

_lib = None


def _share_hip_runtime():
    """One HIP runtime per process.  A PyTorch wheel bundles its own libamdhip64.so (same soname as
    the system one); if libfelics pulled in the system copy first and torch its own later, the second
    runtime would find no GPU.  Loading torch's copy first (without importing torch) lets both
    resolve to the same file."""
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    path = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(path):
        try:
            C.CDLL(path, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def lib():
    """The loaded libfelics.so with argument types declared."""
    global _lib
    if _lib is not None:
        return _lib
    # libfelics overlaps kernels on four HIP streams; give them hardware queues of their own
    # (ROCm default: 4 per process).  Read by the HIP runtime when it initialises.
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
    _share_hip_runtime()
    L = C.CDLL(_build.ensure_lib())
    vp, sz = C.c_void_p, C.c_size_t
    L.felics_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.felics_ctx_destroy.argtypes = [vp]
    L.felics_ctx_destroy.restype = None
    L.felics_max_compressed_size.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_int]
    L.felics_max_compressed_size.restype = sz
    L.felics_compress.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_int, C.c_int, vp, sz, C.POINTER(sz)]
    L.felics_compress_batch.argtypes = [vp, sz, C.POINTER(vp), C.c_uint32, C.c_uint32, C.c_int, C.c_int,
                                        C.POINTER(vp), C.POINTER(sz), C.POINTER(sz)]
    L.felics_compress_batch_device.argtypes = [vp, sz, vp, C.c_uint32, C.c_uint32, C.c_int, C.c_int, vp, sz,
                                               C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.felics_submit_batch_device.argtypes = [vp, sz, vp, C.c_uint32, C.c_uint32, C.c_int, C.c_int, vp, sz, C.POINTER(C.c_int)]
    L.felics_wait_batch.argtypes = [vp, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.felics_read_header.argtypes = [vp, sz, C.POINTER(_CHeader)]
    L.felics_write_header.argtypes = [C.POINTER(_CHeader), vp, sz]
    L.felics_decompress.argtypes = [vp, sz, vp, sz, C.POINTER(_CHeader)]
    L.felics_decompress_with_header.argtypes = [vp, sz, C.POINTER(_CHeader), vp, sz]
    L.felics_get_stats.argtypes = [vp, C.POINTER(_CStats)]
    L.felics_compress_images.argtypes = [vp, sz, C.POINTER(_CImage), C.POINTER(vp), C.POINTER(sz), C.POINTER(sz)]
    L.felics_compress_images_device.argtypes = [vp, sz, C.POINTER(_CImage), vp, sz, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.felics_decompress_batch_device.argtypes = [vp, sz, vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), vp, sz,
                                                 C.POINTER(_CHeader), C.POINTER(C.c_int)]
    L.felics_read_headers_device.argtypes = [vp, sz, vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(_CHeader),
                                             C.POINTER(C.c_int)]
    L.felics_decompress_images_device.argtypes = [vp, sz, vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), vp, sz, C.POINTER(C.c_uint64),
                                                  C.POINTER(_CHeader), C.POINTER(C.c_int)]
    L.felics_compress_views_device.argtypes = [vp, sz, C.POINTER(_CView), vp, vp, sz, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.felics_view_extent.argtypes = [C.POINTER(_CView), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.felics_get_view_stats.argtypes = [vp, C.POINTER(_CViewStats), sz]
    if hasattr(L, "felics_submit_surfaces_device"):  # (FELICS_LIB_PATH may name an older build: A/B measurements against the parent's library)
        L.felics_surfaces_extent.argtypes = [C.POINTER(_CSurfaces), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.felics_submit_surfaces_device.argtypes = [vp, C.POINTER(_CSurfaces), vp, vp, sz, C.POINTER(C.c_int)]
        L.felics_compress_surfaces_device.argtypes = [vp, C.POINTER(_CSurfaces), vp, vp, sz, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.felics_get_surface_stats.argtypes = [vp, C.POINTER(_CSurfaceStats), sz]
    L.felics_get_decode_stats.argtypes = [vp, C.POINTER(_CDecodeStats), sz]
    L.felics_decompress_views_device.argtypes = [vp, sz, vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(_CView), vp,
                                                 C.POINTER(_CHeader), C.POINTER(C.c_int)]
    L.felics_view_writable.argtypes = [C.POINTER(_CView)]
    L.felics_get_decode_view_stats.argtypes = [vp, C.POINTER(_CDecodeViewStats), sz]
    L.felics_decode_lanes_min_streams.argtypes = [C.c_int, C.c_int]
    L.felics_decode_lanes_min_streams.restype = C.c_uint32
    L.felics_index_size.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_uint32]
    L.felics_index_size.restype = sz
    L.felics_index_build.argtypes = [vp, sz, C.c_uint32, vp, sz, C.POINTER(sz)]
    L.felics_decompress_indexed.argtypes = [vp, sz, vp, sz, vp, sz, C.POINTER(_CHeader)]
    L.felics_decompress_batch_device_indexed.argtypes = [vp, sz, vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), vp, sz, vp, sz,
                                                        C.POINTER(_CHeader), C.POINTER(C.c_int)]
    L.felics_compress_batch_device_indexed.argtypes = [vp, sz, vp, C.c_uint32, C.c_uint32, C.c_int, C.c_int, vp, sz, C.c_uint32, vp, sz,
                                                      C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.felics_get_index_stats.argtypes = [vp, C.POINTER(_CIndexStats), sz]
    if hasattr(L, "felics_index_lanes_min_items"):  # (as above: an older build has one form of the indexed decode call)
        L.felics_index_lanes_min_items.argtypes = [C.c_int]
        L.felics_index_lanes_min_items.restype = C.c_uint32
    if hasattr(L, "felics_region_segments"):  # (as above: an older build has no regions)
        L.felics_region_segments.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(_CRegion), C.POINTER(C.c_uint32), sz, C.POINTER(sz)]
        L.felics_decompress_region_indexed.argtypes = [vp, sz, vp, sz, C.POINTER(_CRegion), vp, sz, C.POINTER(_CHeader)]
        L.felics_decompress_regions_device_indexed.argtypes = [vp, sz, vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), vp, sz, sz,
                                                              C.POINTER(_CRegion), vp, sz, C.POINTER(C.c_uint64), C.POINTER(_CHeader),
                                                              C.POINTER(C.c_int)]
        L.felics_get_region_stats.argtypes = [vp, C.POINTER(_CRegionStats), sz]
    if hasattr(L, "felics_decompress_views_device_indexed"):  # (as above: an older build has no indexed views call)
        L.felics_decompress_views_device_indexed.argtypes = [vp, sz, vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), vp, C.POINTER(C.c_uint64),
                                                             C.POINTER(C.c_uint64), C.POINTER(_CView), vp, C.POINTER(_CHeader), C.POINTER(C.c_int)]
        L.felics_decompress_indexed_view.argtypes = [vp, sz, vp, sz, C.POINTER(_CView), C.POINTER(_CHeader)]
        L.felics_get_index_view_stats.argtypes = [vp, C.POINTER(_CIndexViewStats), sz]
    if hasattr(L, "felics_compress_views_device_indexed"):  # (as above: an older build writes indexes for one shape only)
        u64, u32 = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
        L.felics_index_plan.argtypes = [sz, C.POINTER(_CView), u32, u64, u64, u64]
        L.felics_compress_views_device_indexed.argtypes = [vp, sz, C.POINTER(_CView), u32, vp, vp, sz, vp, sz, u64, u64, u64]
        L.felics_get_index_emit_stats.argtypes = [vp, C.POINTER(_CIndexEmitStats), sz]
    if hasattr(L, "felics_decompress_batch_device_indexed_wide"):  # (as above: an older build has no index for 16-bit streams)
        L.felics_index_wide_size_max.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_uint32]
        L.felics_index_wide_size_max.restype = sz
        L.felics_index_wide_build.argtypes = [vp, sz, C.c_uint32, vp, sz, C.POINTER(sz)]
        L.felics_decompress_indexed_wide.argtypes = [vp, sz, vp, sz, vp, sz, C.POINTER(_CHeader)]
        L.felics_decompress_batch_device_indexed_wide.argtypes = [vp, sz, vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), vp, C.POINTER(C.c_uint64),
                                                               C.POINTER(C.c_uint64), vp, sz, C.POINTER(_CHeader), C.POINTER(C.c_int)]
        L.felics_get_index_wide_stats.argtypes = [vp, C.POINTER(_CIndex16Stats), sz]
    if hasattr(L, "felics_compress_batch_device_indexed_wide"):  # (as above: an older build's encoder writes no index for 16-bit streams)
        u64 = C.POINTER(C.c_uint64)
        L.felics_compress_batch_device_indexed_wide.argtypes = [vp, sz, vp, C.c_uint32, C.c_uint32, C.c_int, vp, sz, C.c_uint32, vp, sz, u64, u64,
                                                               u64, u64, u64]
        L.felics_get_index_wide_emit_stats.argtypes = [vp, C.POINTER(_CIndex16EmitStats), sz]
    if hasattr(L, "felics_decompress_regions_device_indexed_wide"):  # (as above: an older build has no regions of 16-bit streams)
        u64 = C.POINTER(C.c_uint64)
        L.felics_decompress_region_indexed_wide.argtypes = [vp, sz, vp, sz, C.POINTER(_CRegion), vp, sz, C.POINTER(_CHeader)]
        L.felics_decompress_regions_device_indexed_wide.argtypes = [vp, sz, vp, u64, u64, vp, u64, u64, sz, C.POINTER(_CRegion), vp, sz, u64,
                                                                   C.POINTER(_CHeader), C.POINTER(C.c_int)]
        L.felics_get_region_wide_stats.argtypes = [vp, C.POINTER(_CRegion16Stats), sz]
    if hasattr(L, "felics_decompress_views_device_indexed_wide"):
        u64 = C.POINTER(C.c_uint64)
        L.felics_decompress_views_device_indexed_wide.argtypes = [vp, sz, vp, u64, u64, vp, u64, u64, C.POINTER(_CView), vp, C.POINTER(_CHeader),
                                                                  C.POINTER(C.c_int)]
        L.felics_decompress_indexed_view_wide.argtypes = [vp, sz, vp, sz, C.POINTER(_CView), C.POINTER(_CHeader)]
        L.felics_get_index_view_wide_stats.argtypes = [vp, C.POINTER(_CIndex16ViewStats), sz]
    if hasattr(L, "felics_decompress_region_views_device_indexed"):  # (as above: an older build decodes no regions into views)
        u64 = C.POINTER(C.c_uint64)
        for call in (L.felics_decompress_region_views_device_indexed, L.felics_decompress_region_views_device_indexed_wide):
            call.argtypes = [vp, sz, vp, u64, u64, vp, u64, u64, sz, C.POINTER(_CRegion), C.POINTER(_CView), vp, C.POINTER(_CHeader),
                             C.POINTER(C.c_int)]
        for call in (L.felics_decompress_region_indexed_view, L.felics_decompress_region_indexed_view_wide):
            call.argtypes = [vp, sz, vp, sz, C.POINTER(_CRegion), C.POINTER(_CView), C.POINTER(_CHeader)]
        L.felics_get_region_view_stats.argtypes = [vp, C.POINTER(_CRegionViewStats), sz]
        L.felics_get_region_view_wide_stats.argtypes = [vp, C.POINTER(_CRegion16ViewStats), sz]
    if hasattr(L, "felics_compress_views_device_indexed_wide"):  # (as above: an older build writes 16-bit indexes for one shape only)
        u64 = C.POINTER(C.c_uint64)
        L.felics_compress_views_device_indexed_wide.argtypes = [vp, sz, C.POINTER(_CView), C.POINTER(C.c_uint32), vp, vp, sz, vp, sz, u64, u64,
                                                                u64, u64, u64]
        L.felics_get_index_view_wide_emit_stats.argtypes = [vp, C.POINTER(_CIndex16ViewEmitStats), sz]
    L.felics_strerror.argtypes = [C.c_int]
    L.felics_strerror.restype = C.c_char_p
    L.felics_last_error.argtypes = [vp]
    L.felics_last_error.restype = C.c_char_p
    L.felics_set_profiling.argtypes = [vp, C.c_int]
    L.felics_stage_name.argtypes = [C.c_int]
    L.felics_stage_name.restype = C.c_char_p
    L.felics_get_stage_ms.argtypes = [vp, C.POINTER(C.c_float), C.c_int]
    L.felics_get_span_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.felics_get_stage_launches.argtypes = [vp, C.POINTER(C.c_int), C.c_int]
    L.felics_ctx_lane_count.argtypes = [vp]
    _lib = L
    return L


def _describe(image):
    image = np.ascontiguousarray(image)
    if image.dtype == np.uint8:
        depth = PixelDepth.Eight
    elif image.dtype == np.uint16:
        depth = PixelDepth.Sixteen
    else:
        raise TypeError("Unsupported image format: %s" % image.dtype)  # cfelics.rs:69-72
    if image.ndim == 2:
        color = ColorType.Gray
    elif image.ndim == 3 and image.shape[2] == 3:
        color = ColorType.Rgb
    else:
        raise TypeError("Unsupported image format: shape %s" % (image.shape,))
    return image, image.shape[1], image.shape[0], color, depth


def _cview(view):
    """A view tuple (ptr, w, h, color, depth, row_stride, pixel_stride, channel_stride) as a felics_view."""
    p, w, h, c, d, rs, ps, cs = view
    return _CView(int(p) if p else None, int(w), int(h), int(c), int(d), int(rs), int(ps), int(cs))


def view_extent(view):
    """felics_view_extent: the half-open byte range (lo, hi) relative to the view's pointer that an encode of it may read; the
    view is checked exactly as Encoder.compress_views_device checks it (FelicsError otherwise).  Host only, needs no GPU."""
    lo, hi = C.c_int64(0), C.c_int64(0)
    v = _cview(view)
    rc = lib().felics_view_extent(C.byref(v), C.byref(lo), C.byref(hi))
    if rc != 0:
        raise FelicsError(rc)
    return int(lo.value), int(hi.value)


def view_writable(view):
    """felics_view_writable: the code Encoder.decompress_views_device gives a view before anything is launched -- 0, or the error
    of felics_view_extent's checks, or FELICS_E_INVALID_ARGUMENT (-11) for a view whose samples may share bytes (the nested-strides
    rule of felics.h).  Host only, needs no GPU."""
    v = _cview(view)
    return int(lib().felics_view_writable(C.byref(v)))


def view_of_array(array):
    """The view tuple of an object with __cuda_array_interface__ (a torch tensor on ROCm, a cupy array): shape (H, W) is gray,
    (H, W, 3) RGB; typestr |u1 / <u2 gives the depth; strides (bytes, None for dense) are taken as given -- so a slice
    t[y0:y1, x0:x1], rgba[..., :3] and chw.permute(1, 2, 0) are views of the memory they came from, no copy made."""
    cai = array.__cuda_array_interface__
    shape = tuple(int(v) for v in cai["shape"])
    typestr = cai["typestr"]
    if typestr in ("|u1", "<u1", "u1"):
        depth, size = PixelDepth.Eight, 1
    elif typestr == "<u2":
        depth, size = PixelDepth.Sixteen, 2
    else:
        raise TypeError("Unsupported image format: %s" % typestr)
    if len(shape) == 2:
        color = ColorType.Gray
    elif len(shape) == 3 and shape[2] == 3:
        color = ColorType.Rgb
    else:
        raise TypeError("Unsupported image format: shape %s" % (shape,))
    strides = cai.get("strides")
    if strides is None:  # C-contiguous
        strides, step = [], size
        for extent in reversed(shape):
            strides.insert(0, step)
            step *= extent
    strides = [int(v) for v in strides]
    ptr = int(cai["data"][0]) if shape[0] * shape[1] else 0
    return (ptr, shape[1], shape[0], color, depth, strides[0], strides[1], strides[2] if len(shape) == 3 else 0)


def _stream_arrays(offsets, lens, idx_offsets, idx_lens, also=None, what="a length and an index per stream"):
    """The four per-stream arrays of an indexed decode call as contiguous uint64, all of the length of `offsets` (and of `also`, if given):
    -> (n, ctypes pointers to the four; a pointer keeps its array alive)."""
    arrays = [np.ascontiguousarray(a, dtype=np.uint64) for a in (offsets, lens, idx_offsets, idx_lens)]
    n = len(arrays[0])
    if any(len(a) != n for a in arrays) or (also is not None and also != n):
        raise ValueError(what)
    return (n, *(a.ctypes.data_as(C.POINTER(C.c_uint64)) for a in arrays))


def _segments(segment_pixels, n):
    """segment_pixels of n views as a uint32 array: one int for all of them, or a sequence of n"""
    segs = np.full(n, segment_pixels, dtype=np.uint32) if np.isscalar(segment_pixels) else np.ascontiguousarray(segment_pixels, dtype=np.uint32)
    if len(segs) != n:
        raise ValueError("a segment per view")
    return np.resize(segs, max(n, 1))


def index_plan(views, segment_pixels):
    """felics_index_plan: where the restart indexes of views (tuples as for Encoder.compress_views_device) go in one buffer.
    segment_pixels: an int for all views or one per view; 0 = no index for that view.  Returns (idx_offsets, idx_lens, total):
    offsets are multiples of 16 in view order, a view without an index has length 0.  Host only, needs no GPU."""
    n = len(views)
    cv = (_CView * max(n, 1))(*[_cview(v) for v in views])
    segs = _segments(segment_pixels, n)
    offs = np.zeros(max(n, 1), dtype=np.uint64)
    lens = np.zeros(max(n, 1), dtype=np.uint64)
    total = C.c_uint64(0)
    u64 = C.POINTER(C.c_uint64)
    rc = lib().felics_index_plan(n, cv, segs.ctypes.data_as(C.POINTER(C.c_uint32)), offs.ctypes.data_as(u64), lens.ctypes.data_as(u64), C.byref(total))
    if rc != 0:
        raise FelicsError(rc)
    return offs[:n], lens[:n], int(total.value)


def _csurfaces(surfaces):
    """A surfaces tuple (view tuple of frame 0, frame_stride in bytes, count) as ONE felics_surfaces: no per-frame objects."""
    view, frame_stride, count = surfaces
    return _CSurfaces(_cview(view), int(frame_stride), int(count))


def surfaces_extent(surfaces):
    """felics_surfaces_extent: the half-open byte range (lo, hi) relative to frame 0's pointer that an encode of the n frames may
    read; checked exactly as Encoder.submit_surfaces_device checks the descriptor (FelicsError otherwise).  Host only, needs no GPU."""
    lo, hi = C.c_int64(0), C.c_int64(0)
    cs = _csurfaces(surfaces)
    rc = lib().felics_surfaces_extent(C.byref(cs), C.byref(lo), C.byref(hi))
    if rc != 0:
        raise FelicsError(rc)
    return int(lo.value), int(hi.value)


class _Frames:
    """Dimension 0 of an array interface peeled off: what view_of_array sees of frame 0."""

    def __init__(self, cai, shape, strides):
        self.__cuda_array_interface__ = dict(cai, shape=shape, strides=strides)


def surfaces_of_array(array):
    """The surfaces tuple (view of frame 0, frame_stride, count) of an object with __cuda_array_interface__ of shape N x H x W (gray),
    N x H x W x 3 or N x 3 x H x W (RGB; a last dimension of 3 reads as channels), or of a slice / channel selection / permutation
    of one: t[:, 3:20, 5:40], rgba[..., :3], rgb[..., ::-1], nchw.permute(0, 2, 3, 1).  Frame 0 is whatever view_of_array accepts.
    A list or tuple of such frames is accepted if they are one shape and layout and a constant number of bytes apart; anything else
    raises ValueError.  No copy is made."""
    if isinstance(array, (list, tuple)):
        views = [view_of_array(a) for a in array]
        if not views:
            raise ValueError("no frames")
        if any(v[1:] != views[0][1:] for v in views):
            raise ValueError("the frames of a surfaces descriptor have one shape, type and layout")
        step = views[1][0] - views[0][0] if len(views) > 1 else 0
        if any(views[i + 1][0] - views[i][0] != step for i in range(len(views) - 1)):
            raise ValueError("the frames are not a constant stride apart")
        return (views[0], step, len(views))
    cai = array.__cuda_array_interface__
    shape = tuple(int(v) for v in cai["shape"])
    if len(shape) not in (3, 4):
        raise TypeError("Unsupported surfaces: shape %s" % (shape,))
    strides = cai.get("strides")
    if strides is None:  # C-contiguous
        size = 2 if cai["typestr"] == "<u2" else 1
        strides, step = [], size
        for extent in reversed(shape):
            strides.insert(0, step)
            step *= extent
    strides = [int(v) for v in strides]
    fshape, fstrides = list(shape[1:]), list(strides[1:])
    if len(shape) == 4 and shape[3] != 3:
        if shape[1] != 3:
            raise TypeError("Unsupported surfaces: shape %s" % (shape,))
        fshape, fstrides = [shape[2], shape[3], 3], [strides[2], strides[3], strides[1]]  # N x C x H x W
    view = view_of_array(_Frames(cai, tuple(fshape), tuple(fstrides)))
    return (view, strides[0] if shape[0] > 1 else 0, shape[0])


class Encoder:
    """One GPU context (felics_ctx): one device, one HIP stream, a reusable workspace in HBM."""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        rc = lib().felics_ctx_create(device, C.byref(self._h))
        if rc != 0:
            self._h = None
            raise FelicsError(rc, "device %d" % device)
        self.device = device

    def close(self):
        if self._h:
            lib().felics_ctx_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _raise(self, rc):
        raise FelicsError(rc, lib().felics_last_error(self._h).decode())

    def _stats(self, getter_name, struct, bare=False):
        """what every *_stats method returns: the counts the context's getter fills `struct` with, as a dict.  A failure raises with the
        context's last error text, or (bare) the code alone."""
        st = struct()
        rc = getattr(lib(), getter_name)(self._h, C.byref(st), C.sizeof(st))
        if rc != 0:
            if bare:
                raise FelicsError(rc)
            self._raise(rc)
        return {k: int(getattr(st, k)) for k, _ in struct._fields_}

    def _indexed_error(self, rc, **carried):
        """what an indexed decode call raises for rc != 0: DecompressionError if rc is a stream error, FelicsError otherwise (with the
        context's text behind a HIP failure); the error carries what the call had filled in (.status, .headers)."""
        err = DecompressionError(rc) if rc in DecompressionError.KINDS else FelicsError(rc, lib().felics_last_error(self._h).decode() if rc == -9 else "")
        for name, value in carried.items():
            setattr(err, name, value)
        return err

    def compress(self, image):
        """The whole .felics file of one image as bytes."""
        return self.compress_batch([image])[0]

    def compress_batch(self, images):
        """Files of a list of same-shaped images (one submission: felics_compress_batch)."""
        if not images:
            return []
        descr = [_describe(im) for im in images]
        first = descr[0]
        for d in descr:
            if d[1:] != first[1:]:
                raise ValueError("a batch holds images of one shape and type")
        _, w, h, color, depth = first
        n = len(descr)
        caps = [14 + 8 * 3 + d[0].nbytes + d[0].nbytes // 2 + 64 for d in descr]
        while True:
            outs = [np.empty(c, dtype=np.uint8) for c in caps]
            px = (C.c_void_p * n)(*[d[0].ctypes.data if d[0].size else None for d in descr])
            op = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
            cp = (C.c_size_t * n)(*caps)
            lens = (C.c_size_t * n)()
            rc = lib().felics_compress_batch(self._h, n, px, w, h, int(color), int(depth), op, cp, lens)
            if rc == -8:  # grow to the sizes the library reported and submit again
                grown = [max(c, int(l)) for c, l in zip(caps, lens)]
                if grown == caps:  # (nothing to grow by: not a size of ours -- do not spin)
                    self._raise(rc)
                caps = grown
                continue
            if rc != 0:
                self._raise(rc)
            return [outs[i][: lens[i]].tobytes() for i in range(n)]

    def compress_images(self, images):
        """Files of a list of images of any shapes and types, in one call (felics_compress_images)."""
        if not images:
            return []
        descr = [_describe(im) for im in images]
        n = len(descr)
        imgs = (_CImage * n)(*[_CImage(d[0].ctypes.data if d[0].size else None, d[1], d[2], int(d[3]), int(d[4])) for d in descr])
        caps = [14 + 8 * 3 + d[0].nbytes + d[0].nbytes // 2 + 64 for d in descr]
        while True:
            outs = [np.empty(c, dtype=np.uint8) for c in caps]
            op = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
            cp = (C.c_size_t * n)(*caps)
            lens = (C.c_size_t * n)()
            rc = lib().felics_compress_images(self._h, n, imgs, op, cp, lens)
            if rc == -8:  # grow to the sizes the library reported and submit again
                grown = [max(c, int(l)) for c, l in zip(caps, lens)]
                if grown == caps:
                    self._raise(rc)
                caps = grown
                continue
            if rc != 0:
                self._raise(rc)
            return [outs[i][: lens[i]].tobytes() for i in range(n)]

    def compress_images_device(self, descs, d_out, d_out_cap):
        """felics_compress_images_device: descs = [(device pointer, w, h, color, depth), ...], streams into d_out (device).
        Returns (offsets, lens) numpy arrays."""
        n = len(descs)
        imgs = (_CImage * max(n, 1))(*[_CImage(int(p) if p else None, int(w), int(h), int(c), int(d)) for p, w, h, c, d in descs])
        offs = np.zeros(max(n, 1), dtype=np.uint64)
        lens = np.zeros(max(n, 1), dtype=np.uint64)
        rc = lib().felics_compress_images_device(self._h, n, imgs, d_out, d_out_cap, offs.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                 lens.ctypes.data_as(C.POINTER(C.c_uint64)))
        if rc == -8:
            raise FelicsError(rc, "need %d bytes" % int(lens[0]))
        if rc != 0:
            self._raise(rc)
        return offs[:n], lens[:n]

    def compress_views_device(self, views, d_out, d_out_cap, ready_event=None):
        """felics_compress_views_device: views = [(device pointer, w, h, color, depth, row_stride, pixel_stride, channel_stride), ...]
        (strides in bytes, signed), streams into d_out (device).  ready_event: a hipEvent_t handle (torch: Event.cuda_event) recorded
        behind the producer of the views; the library's streams wait for it, the host does not.  Returns (offsets, lens)."""
        n = len(views)
        cv = (_CView * max(n, 1))(*[_cview(v) for v in views])
        offs = np.zeros(max(n, 1), dtype=np.uint64)
        lens = np.zeros(max(n, 1), dtype=np.uint64)
        rc = lib().felics_compress_views_device(self._h, n, cv, int(ready_event) if ready_event else None, d_out, d_out_cap,
                                                offs.ctypes.data_as(C.POINTER(C.c_uint64)), lens.ctypes.data_as(C.POINTER(C.c_uint64)))
        if rc == -8:
            raise FelicsError(rc, "need %d bytes" % int(lens[0]))
        if rc != 0:
            self._raise(rc)
        return offs[:n], lens[:n]

    def compress_arrays_device(self, arrays, d_out, d_out_cap, ready_event=None):
        """compress_views_device on objects with __cuda_array_interface__ (view_of_array): slices, channel selections and permuted
        tensors are encoded from the memory they lie in."""
        return self.compress_views_device([view_of_array(a) for a in arrays], d_out, d_out_cap, ready_event)

    def compress_views_device_indexed(self, views, segment_pixels, d_out, d_out_cap, d_index, d_index_cap, idx_offsets=None, ready_event=None):
        """felics_compress_views_device_indexed: compress_views_device plus, for every view whose segment_pixels (an int for all views,
        or one per view; 0: none) is not 0, the restart index of its stream at d_index + idx_offsets[i] (device; idx_offsets=None:
        where index_plan puts them).  Every index equals index_build(stream i, segment_pixels[i]).  Returns (offsets, lens,
        idx_offsets, idx_lens)."""
        n = len(views)
        planned, idx_lens, _ = index_plan(views, segment_pixels)
        idx_offsets = planned if idx_offsets is None else np.ascontiguousarray(idx_offsets, dtype=np.uint64)
        if len(idx_offsets) != n:
            raise ValueError("an index offset per view")
        cv = (_CView * max(n, 1))(*[_cview(v) for v in views])
        segs = _segments(segment_pixels, n)
        offs = np.zeros(max(n, 1), dtype=np.uint64)
        lens = np.zeros(max(n, 1), dtype=np.uint64)
        u64 = C.POINTER(C.c_uint64)
        rc = lib().felics_compress_views_device_indexed(
            self._h, n, cv, segs.ctypes.data_as(C.POINTER(C.c_uint32)), int(ready_event) if ready_event else None, d_out, d_out_cap, d_index,
            d_index_cap, np.resize(idx_offsets, max(n, 1)).ctypes.data_as(u64) if n else None, offs.ctypes.data_as(u64), lens.ctypes.data_as(u64))
        if rc == -8:
            raise FelicsError(rc, "need %d bytes" % int(lens[0]) if lens[0] else "the index buffer is too small")
        if rc != 0:
            self._raise(rc)
        return offs[:n], lens[:n], idx_offsets, idx_lens

    def compress_arrays_device_indexed(self, arrays, segment_pixels, d_out, d_out_cap, d_index, d_index_cap, idx_offsets=None, ready_event=None):
        """compress_views_device_indexed on objects with __cuda_array_interface__ (view_of_array), as compress_arrays_device."""
        return self.compress_views_device_indexed([view_of_array(a) for a in arrays], segment_pixels, d_out, d_out_cap, d_index, d_index_cap,
                                                  idx_offsets, ready_event)

    def index_emit_stats(self):
        """felics_get_index_emit_stats: indexes written by compress_views_device_indexed and their checkpoints, how many of them by
        the mixed kernels (in_mixed) and how many by the uniform writer inside a remedy (redone); cumulative."""
        return self._stats("felics_get_index_emit_stats", _CIndexEmitStats)

    def view_stats(self):
        """felics_get_view_stats: views seen, and how they were read (dense / in_place / gathered, bytes_staged); cumulative."""
        return self._stats("felics_get_view_stats", _CViewStats)

    def submit_surfaces_device(self, surfaces, d_out, d_out_cap, ready_event=None):
        """felics_submit_surfaces_device: surfaces = (view tuple of frame 0, frame_stride, count) or an object surfaces_of_array
        takes; streams into d_out (device) behind ready_event (a hipEvent_t handle, torch: Event.cuda_event).  Returns a ticket for
        wait_batch; tickets of this call and of submit_batch_device share the lanes and the waiting order."""
        if not isinstance(surfaces, tuple) or len(surfaces) != 3 or not isinstance(surfaces[0], tuple):
            surfaces = surfaces_of_array(surfaces)
        cs = _csurfaces(surfaces)
        ticket = C.c_int(-1)
        rc = lib().felics_submit_surfaces_device(self._h, C.byref(cs), int(ready_event) if ready_event else None, d_out, d_out_cap, C.byref(ticket))
        if rc != 0:
            self._raise(rc)
        return ticket.value, int(cs.count)

    def compress_surfaces_device(self, surfaces, d_out, d_out_cap, ready_event=None):
        """felics_compress_surfaces_device: submit_surfaces_device and wait_batch in one blocking call.  Returns (offsets, lens)."""
        if not isinstance(surfaces, tuple) or len(surfaces) != 3 or not isinstance(surfaces[0], tuple):
            surfaces = surfaces_of_array(surfaces)
        cs = _csurfaces(surfaces)
        n = int(cs.count)
        offs = np.zeros(max(n, 1), dtype=np.uint64)
        lens = np.zeros(max(n, 1), dtype=np.uint64)
        rc = lib().felics_compress_surfaces_device(self._h, C.byref(cs), int(ready_event) if ready_event else None, d_out, d_out_cap,
                                                   offs.ctypes.data_as(C.POINTER(C.c_uint64)), lens.ctypes.data_as(C.POINTER(C.c_uint64)))
        if rc == -8:
            raise FelicsError(rc, "need %d bytes" % int(lens[0]))
        if rc != 0:
            self._raise(rc)
        return offs[:n], lens[:n]

    def surface_stats(self):
        """felics_get_surface_stats: submissions, queued / immediate, frames_in_place / frames_gathered, bytes_staged; cumulative."""
        return self._stats("felics_get_surface_stats", _CSurfaceStats)

    def compress_batch_host(self, pixel_ptrs, n, w, h, color, depth, out_ptrs, caps):
        """felics_compress_batch on raw HOST pointers (lists of n addresses: frames in, buffers of caps[i] bytes out): the
        reference's call shape without Python objects in the way -- the copies run at the link's rate when the memory behind the
        pointers is page-locked (a pinned torch tensor).  Returns the streams' lengths (numpy)."""
        px = (C.c_void_p * n)(*[int(p) for p in pixel_ptrs])
        op = (C.c_void_p * n)(*[int(p) for p in out_ptrs])
        cp = (C.c_size_t * n)(*[int(c) for c in caps])
        lens = (C.c_size_t * n)()
        rc = lib().felics_compress_batch(self._h, n, px, w, h, int(color), int(depth), op, cp, lens)
        if rc == -8:
            raise FelicsError(rc, "a stream needs up to %d bytes" % max(lens))
        if rc != 0:
            self._raise(rc)
        return np.array(lens[:], dtype=np.uint64)

    def compress_batch_device(self, d_pixels, n, w, h, color, depth, d_out, d_out_cap):
        """Frames and streams in device memory (raw pointers). Returns (offsets, lens) numpy arrays."""
        offs = np.zeros(n, dtype=np.uint64)
        lens = np.zeros(n, dtype=np.uint64)
        rc = lib().felics_compress_batch_device(
            self._h, n, d_pixels, w, h, int(color), int(depth), d_out, d_out_cap,
            offs.ctypes.data_as(C.POINTER(C.c_uint64)), lens.ctypes.data_as(C.POINTER(C.c_uint64)))
        if rc == -8:
            raise FelicsError(rc, "need %d bytes" % int(lens[0]))
        if rc != 0:
            self._raise(rc)
        return offs, lens

    def compress_batch_device_indexed(self, d_pixels, n, w, h, color, depth, d_out, d_out_cap, segment_pixels, d_index, d_index_cap):
        """felics_compress_batch_device_indexed: compress_batch_device plus the restart index of stream i at
        d_index + i * index_size(w, h, color, depth, segment_pixels) (raw device pointers).  Returns (offsets, lens)."""
        offs = np.zeros(n, dtype=np.uint64)
        lens = np.zeros(n, dtype=np.uint64)
        rc = lib().felics_compress_batch_device_indexed(
            self._h, n, d_pixels, w, h, int(color), int(depth), d_out, d_out_cap, segment_pixels, d_index, d_index_cap,
            offs.ctypes.data_as(C.POINTER(C.c_uint64)), lens.ctypes.data_as(C.POINTER(C.c_uint64)))
        if rc == -8:
            raise FelicsError(rc, "need %d bytes" % int(lens[0]) if lens[0] else "the index buffer is too small")
        if rc != 0:
            self._raise(rc)
        return offs, lens

    def compress_batch_device_indexed16_raw(self, d_pixels, n, w, h, color, d_out, d_out_cap, segment_pixels, d_index, d_index_cap):
        """felics_compress_batch_device_indexed_wide on raw device pointers, one call: (rc, offsets, lens, idx_offsets, idx_lens,
        idx_total).  rc = -8 with idx_total != 0: the index buffer is short of idx_total bytes (streams, offsets and lens are
        complete); with idx_total == 0 it is the stream buffer, lens[0] = the bytes needed."""
        u64 = C.POINTER(C.c_uint64)
        arr = [np.zeros(n, dtype=np.uint64) for _ in range(4)]
        total = C.c_uint64(0)
        rc = lib().felics_compress_batch_device_indexed_wide(self._h, n, d_pixels, w, h, int(color), d_out, d_out_cap, segment_pixels, d_index,
                                                             d_index_cap, *(a.ctypes.data_as(u64) for a in arr), C.byref(total))
        return (rc, *arr, int(total.value))

    def compress_batch_device_indexed16(self, frames, segment_pixels, alloc=None):
        """felics_compress_batch_device_indexed_wide: `frames`, an object with __cuda_array_interface__ holding N dense uint16 frames of
        one shape (N x H x W gray16, N x H x W x 3 RGB16), encoded as compress_batch_device encodes them, with the version-2 restart
        index of every stream written on the GPU beside it.  The two buffers come from alloc(nbytes) -> an object with
        __cuda_array_interface__ whose memory is 64-byte aligned (default: a torch uint8 tensor on the current device); the index
        buffer is sized by the two-call pattern -- a first call with a guess, a second with idx_total bytes if the guess was short.
        Returns IndexedStreams16(streams, offsets, lens, index, idx_offsets, idx_lens): the two device buffers and four numpy arrays,
        what decompress_batch_device_indexed16 takes.  8-bit frames are refused (FELICS_E_UNSUPPORTED): compress_batch_device_indexed
        is their call."""
        cai = frames.__cuda_array_interface__
        shape = tuple(cai["shape"])
        if cai["typestr"] not in ("<u2", "=u2", "|u2"):
            raise FelicsError(-10, "compress_batch_device_indexed16 takes uint16 frames")
        if len(shape) not in (3, 4) or (len(shape) == 4 and shape[3] != 3):
            raise ValueError("frames: N x H x W or N x H x W x 3")
        if cai.get("strides") is not None:
            dense = tuple(int(np.prod(shape[i + 1:])) * 2 for i in range(len(shape)))
            if tuple(cai["strides"]) != dense:
                raise ValueError("frames must be dense")
        if alloc is None:
            import torch

            def alloc(nbytes):
                return torch.empty(max(int(nbytes), 64), dtype=torch.uint8, device="cuda")
        n, h, w = shape[:3]
        color = 1 if len(shape) == 4 else 0
        ptr = lambda buf: int(buf.__cuda_array_interface__["data"][0])
        frame_bytes = h * w * 2 * (3 if color else 1)
        out_cap = max(n, 1) * (frame_bytes + frame_bytes // 4 + 80)
        idx_cap = 0
        if n and index16_size_max(w, h, color, segment_pixels):  # the guess: header, directory, windows and 64 rows per checkpoint
            planes, k = (3 if color else 1), -(-(h * w) // segment_pixels)
            idx_cap = n * (256 + planes * k * (32 + 4 * w * (4 if color else 2) + 16 + 64 * 64))
        streams, index = alloc(out_cap), alloc(max(idx_cap, 64))
        for _ in range(8):
            rc, offs, lens, ioffs, ilens, total = self.compress_batch_device_indexed16_raw(
                int(cai["data"][0]), n, w, h, color, ptr(streams), out_cap, segment_pixels, ptr(index), idx_cap)
            if rc == -8 and total:  # the streams are done; their indexes need `total` bytes
                idx_cap = total
                index = alloc(idx_cap)
                continue
            if rc == -8 and n and lens[0] > out_cap:
                out_cap = int(lens[0]) + 64
                streams = alloc(out_cap)
                continue
            break
        if rc != 0:
            self._raise(rc)
        return IndexedStreams16(streams, offs, lens, index, ioffs, ilens)

    def index16_emit_stats(self):
        """felics_get_index_wide_emit_stats: streams handed to compress_batch_device_indexed16, the state rows and bytes of the indexes
        written and the passes that wrote them (all cumulative)."""
        return self._stats("felics_get_index_wide_emit_stats", _CIndex16EmitStats, bare=True)

    def compress_views_device_indexed16_raw(self, views, segment_pixels, d_out, d_out_cap, d_index, d_index_cap, ready_event=None):
        """felics_compress_views_device_indexed_wide on raw device pointers, one call: (rc, offsets, lens, idx_offsets, idx_lens,
        idx_total).  views as for compress_views_device; segment_pixels: an int for all views or one per view (0: no index).  rc = -8
        with idx_total != 0: the index buffer is short of idx_total bytes (streams, offsets and lens are complete); with
        idx_total == 0 it is the stream buffer, lens[0] = the bytes needed."""
        n = len(views)
        u64 = C.POINTER(C.c_uint64)
        cv = (_CView * max(n, 1))(*[_cview(v) for v in views])
        segs = _segments(segment_pixels, n)
        arr = [np.zeros(max(n, 1), dtype=np.uint64) for _ in range(4)]
        total = C.c_uint64(0)
        rc = lib().felics_compress_views_device_indexed_wide(
            self._h, n, cv, segs.ctypes.data_as(C.POINTER(C.c_uint32)), int(ready_event) if ready_event else None, d_out, d_out_cap, d_index,
            d_index_cap, *(a.ctypes.data_as(u64) for a in arr), C.byref(total))
        return (rc, *(a[:n] for a in arr), int(total.value))

    def compress_views_device_indexed16(self, views, segment_pixels, alloc=None, ready_event=None):
        """felics_compress_views_device_indexed_wide: compress_views_device plus, for every 16-bit view whose segment_pixels (an int for
        all views, or one per view; 0: none) is not 0, the version-2 restart index of its stream, written on the GPU and PLACED BY THE
        LIBRARY (idx_offsets are multiples of 64, in no specified order; a view without an index has idx_lens[i] = 0).  The two buffers
        come from alloc(nbytes) as in compress_batch_device_indexed16, the index buffer by the two-call pattern: a first call with a
        guess, a second with idx_total bytes if the guess was short.  Returns IndexedStreams16(streams, offsets, lens, index,
        idx_offsets, idx_lens): what decompress_views_device_indexed16 takes (for the views that asked for an index)."""
        if alloc is None:
            import torch

            def alloc(nbytes):
                return torch.empty(max(int(nbytes), 64), dtype=torch.uint8, device="cuda")
        n = len(views)
        segs = _segments(segment_pixels, n)
        ptr = lambda buf: int(buf.__cuda_array_interface__["data"][0])
        out_cap, idx_cap = 64, 0
        for (_, w, h, color, depth, *_s), seg in zip(views, segs[:n]):
            planes, sample = (3 if color else 1), (2 if depth == PixelDepth.Sixteen else 1)
            frame_bytes = h * w * sample * planes
            out_cap += frame_bytes + frame_bytes // 4 + 80
            if seg and w * h:  # the guess: header, directory, windows and 64 rows per checkpoint
                k = -(-(h * w) // int(seg))
                idx_cap += 256 + planes * k * (32 + 4 * w * (4 if color else 2) + 16 + 64 * 64)
            elif seg:
                idx_cap += 64
        streams, index = alloc(out_cap), alloc(max(idx_cap, 64))
        for _ in range(8):
            rc, offs, lens, ioffs, ilens, total = self.compress_views_device_indexed16_raw(views, segs[:n], ptr(streams), out_cap, ptr(index),
                                                                                          idx_cap, ready_event)
            if rc == -8 and total:  # the streams are done; their indexes need `total` bytes
                idx_cap = total
                index = alloc(idx_cap)
                continue
            if rc == -8 and n and lens[0] > out_cap:
                out_cap = int(lens[0]) + 64
                streams = alloc(out_cap)
                continue
            break
        if rc != 0:
            self._raise(rc)
        return IndexedStreams16(streams, offs, lens, index, ioffs, ilens)

    def compress_arrays_device_indexed16(self, arrays, segment_pixels, alloc=None, ready_event=None):
        """compress_views_device_indexed16 on objects with __cuda_array_interface__ (view_of_array), as compress_arrays_device."""
        return self.compress_views_device_indexed16([view_of_array(a) for a in arrays], segment_pixels, alloc, ready_event)

    def index16_view_emit_stats(self):
        """felics_get_index_view_wide_emit_stats: views handed to compress_views_device_indexed16, the indexes its kernels wrote, their state
        rows and bytes, the sub-batches the table-driven writer served, the distinct shapes of the last call's most mixed one
        (shapes_max: not cumulative) and the indexes the uniform writer wrote inside a remedy (redone)."""
        return self._stats("felics_get_index_view_wide_emit_stats", _CIndex16ViewEmitStats, bare=True)

    def submit_batch_device(self, d_pixels, n, w, h, color, depth, d_out, d_out_cap):
        """Queues a batch and returns a ticket; up to two can be in flight (felics_submit_batch_device)."""
        ticket = C.c_int(-1)
        rc = lib().felics_submit_batch_device(self._h, n, d_pixels, w, h, int(color), int(depth), d_out, d_out_cap,
                                              C.byref(ticket))
        if rc != 0:
            self._raise(rc)
        return ticket.value, n

    def wait_batch(self, submission):
        """Blocks until the batch of `submission` (from submit_batch_device or submit_surfaces_device) is complete: (offsets, lens)."""
        ticket, n = submission
        offs = np.zeros(n, dtype=np.uint64)
        lens = np.zeros(n, dtype=np.uint64)
        rc = lib().felics_wait_batch(self._h, ticket, offs.ctypes.data_as(C.POINTER(C.c_uint64)),
                                     lens.ctypes.data_as(C.POINTER(C.c_uint64)))
        if rc == -8:
            raise FelicsError(rc, "need %d bytes" % int(lens[0]))
        if rc != 0:
            self._raise(rc)
        return offs, lens

    def decompress_batch_device(self, d_streams, offsets, lens, d_pixels, d_pixels_cap):
        """GPU decoder (felics_decompress_batch_device): streams and pixels in device memory (raw pointers).
        Returns (Header, status array); raises DecompressionError with the first failing stream's code."""
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint64)
        n = len(offsets)
        status = np.zeros(n, dtype=np.int32)
        ch = _CHeader()
        rc = lib().felics_decompress_batch_device(
            self._h, n, d_streams, offsets.ctypes.data_as(C.POINTER(C.c_uint64)), lens.ctypes.data_as(C.POINTER(C.c_uint64)),
            d_pixels, d_pixels_cap, C.byref(ch), status.ctypes.data_as(C.POINTER(C.c_int)))
        if rc in DecompressionError.KINDS:
            err = DecompressionError(rc)
            err.status = status
            raise err
        if rc != 0:
            self._raise(rc)
        return Header(ch.color_type, ch.pixel_depth, ch.width, ch.height), status

    def decompress_batch_device_indexed(self, d_streams, offsets, lens, d_index, index_stride, d_pixels, d_pixels_cap):
        """felics_decompress_batch_device_indexed: streams of one shape, their restart indexes (index i at d_index + i * index_stride)
        and the pixels in device memory (raw pointers).  A wave per (stream, plane, segment); from index_lanes_min_items(color)
        items on (n // 64 * 64 * C * K, with W >= 8 and n >= 64) the first n // 64 * 64 streams are decoded 64 segments to a wave, a
        lane per stream, and the rest a wave per segment beside them: same pixels, same statuses, decode_stats() says which form ran
        (FELICS_TEST_INDEX_LANES=1 / =0 forces / forbids the lane form).  Returns (Header, status array); raises
        DecompressionError with the first failing stream's code if it is a stream error, FelicsError otherwise (both carry .status)."""
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint64)
        n = len(offsets)
        status = np.zeros(n, dtype=np.int32)
        ch = _CHeader()
        rc = lib().felics_decompress_batch_device_indexed(
            self._h, n, d_streams, offsets.ctypes.data_as(C.POINTER(C.c_uint64)), lens.ctypes.data_as(C.POINTER(C.c_uint64)),
            d_index, index_stride, d_pixels, d_pixels_cap, C.byref(ch), status.ctypes.data_as(C.POINTER(C.c_int)))
        if rc != 0:
            raise self._indexed_error(rc, status=status)
        return Header(ch.color_type, ch.pixel_depth, ch.width, ch.height), status

    def decompress_batch_device_indexed16(self, d_streams, offsets, lens, d_index, idx_offsets, idx_lens, d_pixels, d_pixels_cap):
        """felics_decompress_batch_device_indexed_wide: 16-bit streams of one shape, their version-2 restart indexes (index i at
        d_index + idx_offsets[i], a multiple of 64; idx_lens[i] bytes, index16_build's exact size) and the uint16 pixels in device
        memory (raw pointers).  A wave per (stream, plane, segment).  Returns (Header, status array); raises as
        decompress_batch_device_indexed does (the error carries .status)."""
        n, offsets, lens, idx_offsets, idx_lens = _stream_arrays(offsets, lens, idx_offsets, idx_lens)
        status = np.zeros(n, dtype=np.int32)
        ch = _CHeader()
        rc = lib().felics_decompress_batch_device_indexed_wide(
            self._h, n, d_streams, offsets, lens, d_index, idx_offsets, idx_lens, d_pixels, d_pixels_cap, C.byref(ch),
            status.ctypes.data_as(C.POINTER(C.c_int)))
        if rc != 0:
            raise self._indexed_error(rc, status=status)
        return Header(ch.color_type, ch.pixel_depth, ch.width, ch.height), status

    def index16_stats(self):
        """felics_get_index_wide_stats: streams handed to decompress_batch_device_indexed16, their waves (segments16), the passes they ran
        in, the state rows loaded (all cumulative) and the table memory of one pass of the last call."""
        return self._stats("felics_get_index_wide_stats", _CIndex16Stats, bare=True)

    def decompress_regions_device_indexed(self, d_streams, offsets, lens, d_index, index_stride, regions, d_pixels, d_pixels_cap):
        """felics_decompress_regions_device_indexed: windows of streams of one shape through their restart indexes, everything in
        device memory (raw pointers).  regions: (stream, x, y, w, h) each; crop r is dense at d_pixels + out_offsets[r].  Only the
        segments that hold a pixel of a region are walked.  Returns (Header, status array, out_offsets); raises like
        decompress_batch_device_indexed (the error carries .status, one per region)."""
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint64)
        regs = (_CRegion * max(len(regions), 1))(*[_CRegion(*(int(v) for v in r)) for r in regions])
        status = np.zeros(len(regions), dtype=np.int32)
        out_offsets = np.zeros(len(regions), dtype=np.uint64)
        ch = _CHeader()
        rc = lib().felics_decompress_regions_device_indexed(
            self._h, len(offsets), d_streams, offsets.ctypes.data_as(C.POINTER(C.c_uint64)), lens.ctypes.data_as(C.POINTER(C.c_uint64)),
            d_index, index_stride, len(regions), regs, d_pixels, d_pixels_cap, out_offsets.ctypes.data_as(C.POINTER(C.c_uint64)),
            C.byref(ch), status.ctypes.data_as(C.POINTER(C.c_int)))
        if rc != 0:
            raise self._indexed_error(rc, status=status)
        return Header(ch.color_type, ch.pixel_depth, ch.width, ch.height), status, out_offsets

    def region_stats(self):
        """felics_get_region_stats: regions handed to decompress_regions_device_indexed, the segments walked for them, the segments
        of their frames that were not (C * K per region minus the walked), the pixels those walks cover; cumulative."""
        return self._stats("felics_get_region_stats", _CRegionStats)

    def decompress_regions_device_indexed16(self, d_streams, offsets, lens, d_index, idx_offsets, idx_lens, regions, d_pixels, d_pixels_cap):
        """felics_decompress_regions_device_indexed_wide: windows of 16-bit streams of one shape through their version-2 restart indexes
        (index i at d_index + idx_offsets[i], a multiple of 64; idx_lens[i] bytes), everything in device memory (raw pointers).
        regions: (stream, x, y, w, h) each; crop r is dense uint16 at d_pixels + out_offsets[r] (bytes).  Only the segments that hold a
        pixel of a region are walked, a wave each.  Returns (Header, status array, out_offsets); raises like
        decompress_regions_device_indexed (the error carries .status, one per region)."""
        n, offsets, lens, idx_offsets, idx_lens = _stream_arrays(offsets, lens, idx_offsets, idx_lens)
        regs = (_CRegion * max(len(regions), 1))(*[_CRegion(*(int(v) for v in r)) for r in regions])
        status = np.zeros(len(regions), dtype=np.int32)
        out_offsets = np.zeros(len(regions), dtype=np.uint64)
        ch = _CHeader()
        rc = lib().felics_decompress_regions_device_indexed_wide(
            self._h, n, d_streams, offsets, lens, d_index, idx_offsets, idx_lens, len(regions), regs, d_pixels, d_pixels_cap,
            out_offsets.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(ch), status.ctypes.data_as(C.POINTER(C.c_int)))
        if rc != 0:
            raise self._indexed_error(rc, status=status)
        return Header(ch.color_type, ch.pixel_depth, ch.width, ch.height), status, out_offsets

    def region16_stats(self):
        """felics_get_region_wide_stats: regions handed to decompress_regions_device_indexed16, the segments walked for them, the
        segments of their frames that were not, the pixels those walks cover, the state rows loaded and the passes; cumulative."""
        return self._stats("felics_get_region_wide_stats", _CRegion16Stats)

    def read_headers_device(self, d_streams, offsets, lens):
        """felics_read_headers_device: the headers of streams in device memory (raw pointer), read on the GPU.
        Returns (list of Header, or None where the header is invalid; status array of felics_read_header codes)."""
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint64)
        n = len(offsets)
        status = np.zeros(max(n, 1), dtype=np.int32)
        hdrs = (_CHeader * max(n, 1))()
        rc = lib().felics_read_headers_device(self._h, n, d_streams, offsets.ctypes.data_as(C.POINTER(C.c_uint64)),
                                              lens.ctypes.data_as(C.POINTER(C.c_uint64)), hdrs, status.ctypes.data_as(C.POINTER(C.c_int)))
        if rc != 0 and rc not in DecompressionError.KINDS:
            self._raise(rc)
        out = [Header(h.color_type, h.pixel_depth, h.width, h.height) if s == 0 else None for h, s in zip(hdrs[:n], status[:n])]
        return out, status[:n]

    def decompress_images_device(self, d_streams, offsets, lens, d_pixels, d_pixels_cap):
        """felics_decompress_images_device: streams of any shapes in device memory -> frames in device memory (raw pointers).
        Returns (pix_offsets, list of Header -- zeros where a header is invalid --, status array); a too-small buffer raises FelicsError(-8, "need N bytes"), a
        failing stream DecompressionError with .status (and .pix_offsets, .headers)."""
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint64)
        n = len(offsets)
        status = np.zeros(max(n, 1), dtype=np.int32)
        pix = np.zeros(max(n, 1), dtype=np.uint64)
        hdrs = (_CHeader * max(n, 1))()
        rc = lib().felics_decompress_images_device(
            self._h, n, d_streams, offsets.ctypes.data_as(C.POINTER(C.c_uint64)), lens.ctypes.data_as(C.POINTER(C.c_uint64)), d_pixels,
            d_pixels_cap, pix.ctypes.data_as(C.POINTER(C.c_uint64)), hdrs, status.ctypes.data_as(C.POINTER(C.c_int)))
        if rc == -8:
            err = FelicsError(rc, "need %d bytes" % int(pix[0]))
            err.status = status[:n]
            raise err
        headers = [Header(h.color_type, h.pixel_depth, h.width, h.height) for h in hdrs[:n]]  # (zeros where the header is invalid)
        if rc in DecompressionError.KINDS:
            err = DecompressionError(rc)
            err.status, err.pix_offsets, err.headers = status[:n], pix[:n], headers
            raise err
        if rc != 0:
            self._raise(rc)
        return pix[:n], headers, status[:n]

    def decompress_views_device(self, d_streams, offsets, lens, views, ready_event=None):
        """felics_decompress_views_device: stream i (device memory, raw pointer) decoded straight into views[i] = (device pointer, w,
        h, color, depth, row_stride, pixel_stride, channel_stride); only sample bytes are written.  ready_event: a hipEvent_t handle
        (torch: Event.cuda_event) recorded behind whatever produces the streams and last used the views; the library's streams wait
        for it, the host does not.  Returns (list of Header -- zeros where a header is invalid --, status array); a refused view
        raises FelicsError, a failing stream DecompressionError with .status and .headers."""
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint64)
        n = len(offsets)
        if len(views) != n:
            raise ValueError("a view per stream")
        cv = (_CView * max(n, 1))(*[_cview(v) for v in views])
        status = np.zeros(max(n, 1), dtype=np.int32)
        hdrs = (_CHeader * max(n, 1))()
        rc = lib().felics_decompress_views_device(
            self._h, n, d_streams, offsets.ctypes.data_as(C.POINTER(C.c_uint64)), lens.ctypes.data_as(C.POINTER(C.c_uint64)), cv,
            int(ready_event) if ready_event else None, hdrs, status.ctypes.data_as(C.POINTER(C.c_int)))
        headers = [Header(h.color_type, h.pixel_depth, h.width, h.height) for h in hdrs[:n]]  # (zeros where the header is invalid)
        if rc in DecompressionError.KINDS:
            err = DecompressionError(rc)
            err.status, err.headers = status[:n], headers
            raise err
        if rc != 0:
            try:
                self._raise(rc)
            except FelicsError as err:
                err.status = status[:n]
                raise
        return headers, status[:n]

    def decompress_arrays_device(self, d_streams, offsets, lens, arrays, ready_event=None):
        """decompress_views_device into objects with __cuda_array_interface__ (view_of_array): a batch tensor's t[i],
        chw.permute(1, 2, 0), rgba[..., :3] and mosaic[y0:y1, x0:x1] are decoded into where they lie."""
        return self.decompress_views_device(d_streams, offsets, lens, [view_of_array(a) for a in arrays], ready_event)

    def decompress_views_device_indexed(self, d_streams, offsets, lens, d_index, idx_offsets, idx_lens, views, ready_event=None):
        """felics_decompress_views_device_indexed: 8-bit streams of any shapes, each with its restart index at d_index + idx_offsets[i]
        (a multiple of 16; idx_lens[i] bytes, the index's exact size), decoded a wave per (stream, plane, segment) straight into
        views[i] (tuples as for decompress_views_device); only sample bytes are written, gray through any strides with nothing staged.
        ready_event as for decompress_views_device.  Returns (list of Header -- zeros where a header is invalid --, status array); a
        refused view or index address raises FelicsError, a failing stream DecompressionError or FelicsError (a 16-bit stream, a bad
        index) with .status and .headers."""
        return self._views_indexed(lib().felics_decompress_views_device_indexed, d_streams, offsets, lens, d_index, idx_offsets, idx_lens, views,
                                   ready_event)

    def _views_indexed(self, call, d_streams, offsets, lens, d_index, idx_offsets, idx_lens, views, ready_event):
        """what decompress_views_device_indexed and decompress_views_device_indexed16 share: the arrays, the call, the errors"""
        n, offsets, lens, idx_offsets, idx_lens = _stream_arrays(offsets, lens, idx_offsets, idx_lens, also=len(views),
                                                                 what="a length, an index and a view per stream")
        cv = (_CView * max(n, 1))(*[_cview(v) for v in views])
        status = np.zeros(max(n, 1), dtype=np.int32)
        hdrs = (_CHeader * max(n, 1))()
        rc = call(self._h, n, d_streams, offsets, lens, d_index, idx_offsets, idx_lens, cv, int(ready_event) if ready_event else None, hdrs,
                  status.ctypes.data_as(C.POINTER(C.c_int)))
        headers = [Header(h.color_type, h.pixel_depth, h.width, h.height) for h in hdrs[:n]]  # (zeros where the header is invalid)
        if rc != 0:
            raise self._indexed_error(rc, status=status[:n], headers=headers)
        return headers, status[:n]

    def decompress_arrays_device_indexed(self, d_streams, offsets, lens, d_index, idx_offsets, idx_lens, arrays, ready_event=None):
        """decompress_views_device_indexed into objects with __cuda_array_interface__ (view_of_array), as decompress_arrays_device: the
        images of an N x C x H x W tensor (t[i].permute(1, 2, 0)), rgba[..., :3], the cells of a mosaic."""
        return self.decompress_views_device_indexed(d_streams, offsets, lens, d_index, idx_offsets, idx_lens, [view_of_array(a) for a in arrays],
                                                    ready_event)

    def decompress_views_device_indexed16(self, d_streams, offsets, lens, d_index, idx_offsets, idx_lens, views, ready_event=None):
        """felics_decompress_views_device_indexed16: decompress_views_device_indexed for 16-bit streams, each with its version-2 index at
        d_index + idx_offsets[i] (a multiple of 64; idx_lens[i] bytes), into views of depth 16 (even addresses and strides); gray is one
        2-byte store per sample through any strides, nothing staged.  Returns and raises as decompress_views_device_indexed (an 8-bit
        stream is FelicsError -10)."""
        return self._views_indexed(lib().felics_decompress_views_device_indexed_wide, d_streams, offsets, lens, d_index, idx_offsets, idx_lens,
                                   views, ready_event)

    def decompress_arrays_device_indexed16(self, d_streams, offsets, lens, d_index, idx_offsets, idx_lens, arrays, ready_event=None):
        """decompress_views_device_indexed16 into uint16 objects with __cuda_array_interface__ (view_of_array), as
        decompress_arrays_device_indexed."""
        return self.decompress_views_device_indexed16(d_streams, offsets, lens, d_index, idx_offsets, idx_lens, [view_of_array(a) for a in arrays],
                                                      ready_event)

    def decompress_region_views_device_indexed(self, d_streams, offsets, lens, d_index, idx_offsets, idx_lens, regions, views, ready_event=None):
        """felics_decompress_region_views_device_indexed: windows of 8-bit streams of any shapes, each stream with its restart index at
        d_index + idx_offsets[s] (a multiple of 16; idx_lens[s] bytes), decoded a wave per (region, plane, needed segment) straight
        into views[r] (tuples as for decompress_views_device, w x h of regions[r] = (stream, x, y, w, h)); only sample bytes are
        written.  ready_event as for decompress_views_device.  Returns (list of Header per stream -- zeros where a header is invalid
        --, status array per region); a refused view, region or index address raises FelicsError, a failing region
        DecompressionError or FelicsError, with .status (per region) and .headers."""
        return self._region_views_indexed(lib().felics_decompress_region_views_device_indexed, d_streams, offsets, lens, d_index, idx_offsets,
                                          idx_lens, regions, views, ready_event)

    def _region_views_indexed(self, call, d_streams, offsets, lens, d_index, idx_offsets, idx_lens, regions, views, ready_event):
        """what decompress_region_views_device_indexed and its 16-bit form share: the arrays, the call, the errors"""
        n, offsets, lens, idx_offsets, idx_lens = _stream_arrays(offsets, lens, idx_offsets, idx_lens)
        nr = len(regions)
        if len(views) != nr:
            raise ValueError("a view per region")
        regs = (_CRegion * max(nr, 1))(*[_CRegion(*(int(v) for v in r)) for r in regions])
        cv = (_CView * max(nr, 1))(*[_cview(v) for v in views])
        status = np.zeros(max(nr, 1), dtype=np.int32)
        hdrs = (_CHeader * max(n, 1))()
        rc = call(self._h, n, d_streams, offsets, lens, d_index, idx_offsets, idx_lens, nr, regs, cv, int(ready_event) if ready_event else None,
                  hdrs, status.ctypes.data_as(C.POINTER(C.c_int)))
        headers = [Header(h.color_type, h.pixel_depth, h.width, h.height) for h in hdrs[:n]]  # (zeros where the header is invalid)
        if rc != 0:
            raise self._indexed_error(rc, status=status[:nr], headers=headers)
        return headers, status[:nr]

    def decompress_region_arrays_device_indexed(self, d_streams, offsets, lens, d_index, idx_offsets, idx_lens, regions, arrays, ready_event=None):
        """decompress_region_views_device_indexed into objects with __cuda_array_interface__ (view_of_array), as
        decompress_arrays_device_indexed: window r goes into arrays[r] -- batch[r], a cell of a mosaic, rgba[..., :3]."""
        return self.decompress_region_views_device_indexed(d_streams, offsets, lens, d_index, idx_offsets, idx_lens, regions,
                                                           [view_of_array(a) for a in arrays], ready_event)

    def decompress_region_views_device_indexed16(self, d_streams, offsets, lens, d_index, idx_offsets, idx_lens, regions, views, ready_event=None):
        """felics_decompress_region_views_device_indexed16: decompress_region_views_device_indexed for 16-bit streams and their
        version-2 indexes (index addresses multiples of 64), into views of depth 16."""
        return self._region_views_indexed(lib().felics_decompress_region_views_device_indexed_wide, d_streams, offsets, lens, d_index, idx_offsets,
                                          idx_lens, regions, views, ready_event)

    def decompress_region_arrays_device_indexed16(self, d_streams, offsets, lens, d_index, idx_offsets, idx_lens, regions, arrays, ready_event=None):
        """decompress_region_views_device_indexed16 into uint16 objects with __cuda_array_interface__ (view_of_array)."""
        return self.decompress_region_views_device_indexed16(d_streams, offsets, lens, d_index, idx_offsets, idx_lens, regions,
                                                             [view_of_array(a) for a in arrays], ready_event)

    def region_view_stats(self):
        """felics_get_region_view_stats: regions handed to decompress_region_views_device_indexed, those that got a code before a wave
        was launched for them, the segments walked and skipped, the pixels walked, launches and passes; cumulative -- and plane_bytes,
        the RGB scratch of the last call's largest pass."""
        return self._stats("felics_get_region_view_stats", _CRegionViewStats)

    def region16_view_stats(self):
        """felics_get_region16_view_stats: region_view_stats for decompress_region_views_device_indexed16, with the state rows loaded
        (cumulative) and table_bytes (the last call's estimator tables)."""
        return self._stats("felics_get_region_view_wide_stats", _CRegion16ViewStats)

    def index16_view_stats(self):
        """felics_get_index16_view_stats: streams handed to decompress_views_device_indexed16, those that got a code before a wave was
        launched for them, the waves (items), kernel launches, stream passes and state rows loaded; cumulative -- and plane_bytes (the
        RGB scratch of the last call's largest pass) and table_bytes (the last call's estimator tables)."""
        return self._stats("felics_get_index_view_wide_stats", _CIndex16ViewStats)

    def index_view_stats(self):
        """felics_get_index_view_stats: streams handed to decompress_views_device_indexed, those that got a code before a wave was
        launched for them, the waves (items), launches and passes; cumulative -- and plane_bytes, the RGB scratch of the last call's
        largest pass."""
        return self._stats("felics_get_index_view_stats", _CIndexViewStats)

    def decode_view_stats(self):
        """felics_get_decode_view_stats: views handed to decompress_views_device and how they were written (dense / in_place /
        scattered, bytes_staged); cumulative."""
        return self._stats("felics_get_decode_view_stats", _CDecodeViewStats)

    def decode_stats(self):
        """felics_get_decode_stats: how many streams the two device decode calls were handed and which form they took (wave8 / lanes8 /
        wave16 / lanes16 / host / undecoded; cumulative), and lanes16_table_bytes of the last call."""
        out = self._stats("felics_get_decode_stats", _CDecodeStats)
        # (felics_index_stats: the segments decompress_batch_device_indexed gave a wave each / a lane each -- together n * C * K per
        # call -- and the lane-form passes it launched)
        ist = self._stats("felics_get_index_stats", _CIndexStats)
        out["segments8"] = ist["segments8"]
        out["lane_segments8"] = ist["lane_segments8"]
        out["lane_passes"] = ist["lane_passes"]
        return out

    def lane_count(self):
        """felics_ctx_lane_count: submissions this context can have in flight (fixed when it was created)."""
        return int(lib().felics_ctx_lane_count(self._h))

    def stats(self):
        """felics_get_stats: batches redone (slot overflow, look-back fallback), slow-path / failed flags."""
        st = _CStats()
        lib().felics_get_stats(self._h, C.byref(st))
        return {k: int(getattr(st, k)) for k, _ in _CStats._fields_}

    def set_profiling(self, on):
        lib().felics_set_profiling(self._h, int(bool(on)))

    def stage_ms(self):
        """Per stage: sum of the durations (ms) of its launches in the last submission."""
        n = lib().felics_stage_count()
        buf = (C.c_float * n)()
        lib().felics_get_stage_ms(self._h, buf, n)
        return {lib().felics_stage_name(i).decode(): float(buf[i]) for i in range(n)}

    def span_ms(self):
        """First kernel -> last byte of the last submission collected (profiling on), in ms."""
        v = C.c_float(0)
        lib().felics_get_span_ms(self._h, C.byref(v))
        return float(v.value)

    def stage_launches(self):
        n = lib().felics_stage_count()
        buf = (C.c_int * n)()
        lib().felics_get_stage_launches(self._h, buf, n)
        return {lib().felics_stage_name(i).decode(): int(buf[i]) for i in range(n)}


_default = {}


def decode16_lanes_min_streams(color=0):
    """felics_decode_lanes_min_streams(1, color): streams a device decode call must hold for its 16-bit streams (color: 0 gray, 1 RGB) to be
    decoded 64 to a wave; 0xFFFFFFFF: never (the form is then reached with FELICS_TEST_DECODE16_LANES=1 only)."""
    return int(lib().felics_decode_lanes_min_streams(1, int(color)))


def index_lanes_min_items(color=0):
    """felics_index_lanes_min_items(color): lane-form items (n // 64 * 64 * C * K) from which decompress_batch_device_indexed decodes
    64 segments to a wave by itself (color: 0 gray, 1 RGB); 0xFFFFFFFF: never (the form is then reached with
    FELICS_TEST_INDEX_LANES=1 only)."""
    return int(lib().felics_index_lanes_min_items(int(color)))


def default_encoder(device=0):
    if device not in _default:
        _default[device] = Encoder(device)
    return _default[device]


# ---- the reference's free functions -------------------------------------------------------

def write_header(header, to):
    """format.rs:51-61."""
    ch = _CHeader(int(header.color_type), int(header.pixel_depth), header.width, header.height)
    buf = (C.c_uint8 * 14)()
    rc = lib().felics_write_header(C.byref(ch), buf, 14)
    if rc != 0:
        raise FelicsError(rc)
    to.write(bytes(buf))


def read_header(from_):
    """format.rs:63-84; consumes up to 14 bytes of `from_`."""
    data = from_.read(14)
    ch = _CHeader()
    arr = np.frombuffer(data, dtype=np.uint8)
    rc = lib().felics_read_header(arr.ctypes.data if len(arr) else None, len(arr), C.byref(ch))
    if rc != 0:
        raise DecompressionError(rc)
    return Header(ch.color_type, ch.pixel_depth, ch.width, ch.height)


def compress_image(to, image, encoder=None):
    """compression.rs:412-418: writes the .felics stream of `image` to `to`."""
    enc = encoder or default_encoder()
    to.write(enc.compress(image))


def compress(image, to, encoder=None):
    """CompressDecompress::compress (traits.rs:48-50)."""
    compress_image(to, image, encoder)


def decompress_image(from_):
    """compression.rs:420-441: returns the image as (H,W) / (H,W,3) uint8 / uint16."""
    data = from_.read() if hasattr(from_, "read") else bytes(from_)
    arr = np.frombuffer(data, dtype=np.uint8)
    ch = _CHeader()
    rc = lib().felics_read_header(arr.ctypes.data if len(arr) else None, len(arr), C.byref(ch))
    if rc != 0:
        raise DecompressionError(rc)
    planes = 3 if ch.color_type else 1
    dt = np.uint16 if ch.pixel_depth else np.uint8
    # a corrupt header must not make us allocate before the stream proves it holds that many pixels
    if ch.width * ch.height * planes > max(len(arr), 1) * 8 + 2 * planes:  # a pixel costs at least one bit
        raise DecompressionError(-1)
    shape = (ch.height, ch.width, 3) if planes == 3 else (ch.height, ch.width)
    out = np.zeros(shape, dtype=dt)
    rc = lib().felics_decompress(arr.ctypes.data, len(arr), out.ctypes.data if out.size else None,
                                 out.nbytes, None)
    if rc != 0:
        raise DecompressionError(rc)
    return out


def decompress(from_):
    """CompressDecompress::decompress (traits.rs:57-64)."""
    return decompress_image(from_)


def decompress_with_header(from_, header):
    """CompressDecompress::decompress_with_header (traits.rs:53-56): `from_` is positioned behind the header."""
    data = from_.read() if hasattr(from_, "read") else bytes(from_)
    arr = np.frombuffer(data, dtype=np.uint8)
    planes = 3 if int(header.color_type) else 1
    dt = np.uint16 if int(header.pixel_depth) else np.uint8
    if header.width * header.height * planes > max(len(arr), 1) * 8 + 2 * planes:  # a pixel costs at least one bit
        raise DecompressionError(-1)
    shape = (header.height, header.width, 3) if planes == 3 else (header.height, header.width)
    out = np.zeros(shape, dtype=dt)
    ch = _CHeader(int(header.color_type), int(header.pixel_depth), header.width, header.height)
    rc = lib().felics_decompress_with_header(arr.ctypes.data if len(arr) else None, len(arr), C.byref(ch),
                                             out.ctypes.data if out.size else None, out.nbytes)
    if rc != 0:
        raise DecompressionError(rc)
    return out


def index_size(width, height, color, depth, segment_pixels):
    """felics_index_size: bytes of the restart index of a width x height image; 0 if there is none (16-bit, bad segment_pixels)."""
    return int(lib().felics_index_size(width, height, int(color), int(depth), segment_pixels))


def index_build(data, segment_pixels):
    """felics_index_build: the restart index (bytes) of an 8-bit stream, built by decoding it once on the CPU."""
    arr = np.frombuffer(bytes(data), dtype=np.uint8)
    need = C.c_size_t(0)
    L = lib()
    rc = L.felics_index_build(arr.ctypes.data if len(arr) else None, len(arr), segment_pixels, None, 0, C.byref(need))
    if rc == 0:
        return b""
    if rc != -8:
        raise DecompressionError(rc) if rc in DecompressionError.KINDS else FelicsError(rc)
    out = np.zeros(need.value, dtype=np.uint8)
    rc = L.felics_index_build(arr.ctypes.data, len(arr), segment_pixels, out.ctypes.data, out.nbytes, C.byref(need))
    if rc != 0:
        raise DecompressionError(rc) if rc in DecompressionError.KINDS else FelicsError(rc)
    return out[:need.value].tobytes()


def decompress_indexed(data, index):
    """felics_decompress_indexed: the image of an 8-bit stream, decoded segment by segment through its restart index."""
    arr = np.frombuffer(bytes(data), dtype=np.uint8)
    idx = np.frombuffer(bytes(index), dtype=np.uint8)
    ch = _CHeader()
    rc = lib().felics_read_header(arr.ctypes.data if len(arr) else None, len(arr), C.byref(ch))
    if rc != 0:
        raise DecompressionError(rc)
    planes = 3 if ch.color_type else 1
    if ch.width * ch.height * planes > max(len(arr), 1) * 8 + 2 * planes:  # a pixel costs at least one bit
        raise DecompressionError(-1)
    shape = (ch.height, ch.width, 3) if planes == 3 else (ch.height, ch.width)
    out = np.zeros(shape, dtype=np.uint16 if ch.pixel_depth else np.uint8)
    rc = lib().felics_decompress_indexed(arr.ctypes.data, len(arr), idx.ctypes.data if len(idx) else None, len(idx),
                                         out.ctypes.data if out.size else None, out.nbytes, None)
    if rc != 0:
        raise DecompressionError(rc) if rc in DecompressionError.KINDS else FelicsError(rc)
    return out


def index16_size_max(width, height, color, segment_pixels):
    """felics_index_wide_size_max: an upper bound of the bytes of the version-2 restart index of a width x height 16-bit image; 0 for
    bad arguments."""
    return int(lib().felics_index_wide_size_max(width, height, int(color), segment_pixels))


def index16_build(data, segment_pixels):
    """felics_index_wide_build: the version-2 restart index (bytes) of a 16-bit stream, built by decoding it once on the CPU."""
    arr = np.frombuffer(bytes(data), dtype=np.uint8)
    need = C.c_size_t(0)
    L = lib()
    rc = L.felics_index_wide_build(arr.ctypes.data if len(arr) else None, len(arr), segment_pixels, None, 0, C.byref(need))
    if rc == 0:
        return b""
    if rc != -8:
        raise DecompressionError(rc) if rc in DecompressionError.KINDS else FelicsError(rc)
    out = np.zeros(need.value, dtype=np.uint8)
    rc = L.felics_index_wide_build(arr.ctypes.data, len(arr), segment_pixels, out.ctypes.data, out.nbytes, C.byref(need))
    if rc != 0:
        raise DecompressionError(rc) if rc in DecompressionError.KINDS else FelicsError(rc)
    return out[:need.value].tobytes()


def decompress_indexed16(data, index):
    """felics_decompress_indexed_wide: the image of a 16-bit stream, decoded segment by segment through its version-2 restart index."""
    arr = np.frombuffer(bytes(data), dtype=np.uint8)
    idx = np.frombuffer(bytes(index), dtype=np.uint8)
    ch = _CHeader()
    rc = lib().felics_read_header(arr.ctypes.data if len(arr) else None, len(arr), C.byref(ch))
    if rc != 0:
        raise DecompressionError(rc)
    planes = 3 if ch.color_type else 1
    if ch.width * ch.height * planes > max(len(arr), 1) * 8 + 2 * planes:  # a pixel costs at least one bit
        raise DecompressionError(-1)
    shape = (ch.height, ch.width, 3) if planes == 3 else (ch.height, ch.width)
    out = np.zeros(shape, dtype=np.uint16 if ch.pixel_depth else np.uint8)
    rc = lib().felics_decompress_indexed_wide(arr.ctypes.data, len(arr), idx.ctypes.data if len(idx) else None, len(idx),
                                           out.ctypes.data if out.size else None, out.nbytes, None)
    if rc != 0:
        raise DecompressionError(rc) if rc in DecompressionError.KINDS else FelicsError(rc)
    return out


def decompress_indexed_view(data, index, array):
    """felics_decompress_indexed_view: an 8-bit stream decoded through its restart index INTO `array`, a writable numpy array of shape
    (H, W) or (H, W, 3) and any admissible strides (a slice of a pitched buffer, buf[::-1], rgba[..., :3], chw.transpose(1, 2, 0), a
    mosaic cell): only the array's own samples are written.  The host model of Encoder.decompress_views_device_indexed."""
    return _indexed_view(lib().felics_decompress_indexed_view, data, index, array)


def decompress_indexed16_view(data, index, array):
    """felics_decompress_indexed16_view: decompress_indexed_view for a 16-bit stream and its version-2 index, into a uint16 array.  The
    host model of Encoder.decompress_views_device_indexed16."""
    return _indexed_view(lib().felics_decompress_indexed_view_wide, data, index, array)


def _indexed_view(call, data, index, array):
    if not isinstance(array, np.ndarray) or array.dtype not in (np.uint8, np.uint16) or array.ndim not in (2, 3) or (array.ndim == 3 and array.shape[2] != 3):
        raise TypeError("Unsupported image format")
    if not array.flags.writeable:
        raise ValueError("the array is read-only")
    arr = np.frombuffer(bytes(data), dtype=np.uint8)
    idx = np.frombuffer(bytes(index), dtype=np.uint8)
    h, w = array.shape[:2]
    rgb = array.ndim == 3
    view = _CView(array.ctypes.data if array.size else None, w, h, int(rgb), int(array.dtype == np.uint16), array.strides[0], array.strides[1],
                  array.strides[2] if rgb else 0)
    rc = call(arr.ctypes.data if len(arr) else None, len(arr), idx.ctypes.data if len(idx) else None, len(idx), C.byref(view), None)
    if rc != 0:
        raise DecompressionError(rc) if rc in DecompressionError.KINDS else FelicsError(rc)
    return array


def decompress_region_indexed_view(data, index, x, y, w, h, array):
    """felics_decompress_region_indexed_view: the w x h window at (x, y) of an 8-bit stream decoded through its restart index INTO
    `array`, a writable numpy array as for decompress_indexed_view: only the array's own samples are written.  The host model of
    Encoder.decompress_region_views_device_indexed."""
    return _indexed_view(lambda d, dl, i, il, view, hdr: lib().felics_decompress_region_indexed_view(
        d, dl, i, il, C.byref(_CRegion(0, x, y, w, h)), view, hdr), data, index, array)


def decompress_region_indexed16_view(data, index, x, y, w, h, array):
    """felics_decompress_region_indexed16_view: decompress_region_indexed_view for a 16-bit stream and its version-2 index, into a
    uint16 array.  The host model of Encoder.decompress_region_views_device_indexed16."""
    return _indexed_view(lambda d, dl, i, il, view, hdr: lib().felics_decompress_region_indexed_view_wide(
        d, dl, i, il, C.byref(_CRegion(0, x, y, w, h)), view, hdr), data, index, array)


def region_segments(width, height, segment_pixels, x, y, w, h):
    """felics_region_segments: the segments (ascending list) of a plane of a width x height image cut every segment_pixels pixels that
    hold a pixel of the w x h window at (x, y)."""
    reg = _CRegion(0, x, y, w, h)
    need = C.c_size_t(0)
    L = lib()
    rc = L.felics_region_segments(width, height, segment_pixels, C.byref(reg), None, 0, C.byref(need))
    if rc == 0:
        return []
    if rc != -8:
        raise FelicsError(rc)
    segs = (C.c_uint32 * need.value)()
    rc = L.felics_region_segments(width, height, segment_pixels, C.byref(reg), segs, need.value, C.byref(need))
    if rc != 0:
        raise FelicsError(rc)
    return list(segs)


def decompress_region_indexed(data, index, x, y, w, h):
    """felics_decompress_region_indexed: the w x h window at (x, y) of an 8-bit stream's image (ndarray, h x w or h x w x 3), decoded
    from the checkpoints of the segments that hold its pixels and from nothing else."""
    arr = np.frombuffer(bytes(data), dtype=np.uint8)
    idx = np.frombuffer(bytes(index), dtype=np.uint8)
    ch = _CHeader()
    rc = lib().felics_read_header(arr.ctypes.data if len(arr) else None, len(arr), C.byref(ch))
    if rc != 0:
        raise DecompressionError(rc)
    reg = _CRegion(0, x, y, w, h)
    out = np.zeros((h, w, 3) if ch.color_type else (h, w), dtype=np.uint8)
    rc = lib().felics_decompress_region_indexed(arr.ctypes.data, len(arr), idx.ctypes.data if len(idx) else None, len(idx), C.byref(reg),
                                                out.ctypes.data if out.size else None, out.nbytes, None)
    if rc != 0:
        raise DecompressionError(rc) if rc in DecompressionError.KINDS else FelicsError(rc)
    return out


def decompress_region_indexed16(data, index, x, y, w, h):
    """felics_decompress_region_indexed_wide: the w x h window at (x, y) of a 16-bit stream's image (uint16 ndarray, h x w or
    h x w x 3), decoded from the checkpoints of the segments that hold its pixels and from nothing else."""
    arr = np.frombuffer(bytes(data), dtype=np.uint8)
    idx = np.frombuffer(bytes(index), dtype=np.uint8)
    ch = _CHeader()
    rc = lib().felics_read_header(arr.ctypes.data if len(arr) else None, len(arr), C.byref(ch))
    if rc != 0:
        raise DecompressionError(rc)
    reg = _CRegion(0, x, y, w, h)
    out = np.zeros((h, w, 3) if ch.color_type else (h, w), dtype=np.uint16)
    rc = lib().felics_decompress_region_indexed_wide(arr.ctypes.data, len(arr), idx.ctypes.data if len(idx) else None, len(idx), C.byref(reg),
                                                     out.ctypes.data if out.size else None, out.nbytes, None)
    if rc != 0:
        raise DecompressionError(rc) if rc in DecompressionError.KINDS else FelicsError(rc)
    return out


def decompress_bytes(data):
    return decompress_image(io.BytesIO(data))
