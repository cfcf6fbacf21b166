"""Device-resident batch API over the C ABI in ``include/rir_amd_device.h``.

Inputs and outputs are ``torch`` CUDA(HIP) tensors; torch is plumbing only (device memory and
streams) - every operation is one call into ``librir_amd.so`` on torch's current HIP stream.
"""
import ctypes as ct
from collections import namedtuple

import numpy as np
import torch

from .low_level.misc import _lib, last_error
from .signal_processing.rir_signal_processing import (DIST2_NONE, DISTANCE_MAX_SIDE, LocalStats, PixelStats, RegionGeometry,  # noqa: F401 (API)
                                                      RegionHistogram, RegionQuantiles, RegionStats, _distance_transform_args, _pixel_quantiles_args,
                                                      _pixel_stats_args, _polygon_map_args, _region_geometry_args, _region_histogram_args,
                                                      _region_quantiles_args, _region_quantiles_percents, _region_stats_args,
                                                      _local_stats_args, _morphology_args, _rank_filter_args, _temporal_median_args,
                                                      _window_size, percentile_rank,
                                                      RECONSTRUCT_BORDER, RECONSTRUCT_MARKER, RECONSTRUCT_SHIFT, _NO_SHIFT, _reconstruct_args)

DEFAULT_GOP = 50  # reference key-frame cadence, src/cpp/video_io/h264.cpp:1662-1665

_DTYPE_CHARS = {
    torch.bool: "?",
    torch.int8: "b",
    torch.uint8: "B",
    torch.int16: "h",
    torch.uint16: "H",
    torch.int32: "i",
    torch.uint32: "I",
    torch.int64: "l",
    torch.uint64: "L",
    torch.float32: "f",
    torch.float64: "d",
}
_NP_OF = {
    torch.bool: np.bool_,
    torch.int8: np.int8,
    torch.uint8: np.uint8,
    torch.int16: np.int16,
    torch.uint16: np.uint16,
    torch.int32: np.int32,
    torch.uint32: np.uint32,
    torch.int64: np.int64,
    torch.uint64: np.uint64,
    torch.float32: np.float32,
    torch.float64: np.float64,
}
_DTYPE_NAMES = {t: np.dtype(a).name for t, a in _NP_OF.items()}  # as the _..._args checkers of the host module name them


class CodecLayout(ct.Structure):
    _fields_ = [
        ("width", ct.c_int),
        ("height", ct.c_int),
        ("nframes", ct.c_int),
        ("gop", ct.c_int),
        ("ntiles", ct.c_int),
        ("nchunks", ct.c_int),
        ("hdr_bytes", ct.c_int64),
        ("tile_off_bytes", ct.c_int64),
        ("chunk_off_bytes", ct.c_int64),
        ("stream_max_bytes", ct.c_int64),
        ("workspace_bytes", ct.c_int64),
    ]


class CodecSlots(ct.Structure):
    _fields_ = [("slots_offset_bytes", ct.c_int64), ("slot_words", ct.c_int64), ("seg_words_offset_bytes", ct.c_int64), ("nslots", ct.c_int64)]


class CodecPackedLayout(ct.Structure):
    _fields_ = [("ntiles", ct.c_int), ("nchunks", ct.c_int), ("hdr_bytes", ct.c_int64), ("seg_pos_bytes", ct.c_int64), ("seg_words_bytes", ct.c_int64),
                ("stream_budget_bytes", ct.c_int64), ("stream_max_bytes", ct.c_int64), ("workspace_min_bytes", ct.c_int64),
                ("workspace_max_bytes", ct.c_int64)]


_vp = ct.c_void_p
_lib.rir_codec_slots_query.argtypes = [ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.POINTER(CodecSlots)]
_lib.rir_device_available.restype = ct.c_int
_lib.rir_stream_synchronize.argtypes = [_vp]
_lib.rir_codec_layout_query.argtypes = [ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.POINTER(CodecLayout)]
_lib.rir_codec_encode_device.argtypes = [_vp, ct.c_int, ct.c_int, ct.c_int, ct.c_int, _vp, _vp, _vp, _vp, _vp, ct.c_longlong, _vp]
_lib.rir_codec_encode_single_pass_device.argtypes = [_vp, ct.c_int, ct.c_int, ct.c_int, ct.c_int, _vp, _vp, _vp, _vp, _vp, ct.c_longlong, _vp]
_lib.rir_codec_encode_status.argtypes = [_vp, _vp]
_lib.rir_codec_encode_tiles_device.argtypes = [_vp, ct.c_int, ct.c_int, ct.c_int, ct.c_int, _vp, _vp, ct.c_longlong, _vp]
_lib.rir_codec_encode_compact_device.argtypes = [ct.c_int, ct.c_int, ct.c_int, ct.c_int, _vp, _vp, _vp, _vp, ct.c_longlong, _vp]
_lib.rir_codec_workspace_create_device.argtypes = [_vp, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_longlong, ct.POINTER(ct.c_void_p),
                                                   ct.POINTER(ct.c_float), ct.POINTER(ct.c_int), _vp]
_lib.rir_buffer_create_beside_device.argtypes = [_vp, ct.c_longlong, ct.c_longlong, ct.c_int, ct.c_longlong, ct.POINTER(ct.c_void_p), ct.POINTER(ct.c_float),
                                                 ct.POINTER(ct.c_int), _vp]
_lib.rir_buffer_destroy_device.argtypes = [_vp]
_lib.rir_buffer_destroy_device.restype = None
_lib.rir_codec_workspace_destroy_device.argtypes = [_vp]
_lib.rir_codec_workspace_destroy_device.restype = None
_lib.rir_codec_decode_slots_device.argtypes = [_vp, _vp, ct.c_longlong, ct.c_int, ct.c_int, ct.c_int, ct.c_int, _vp, _vp, _vp]
_lib.rir_codec_packed_query.argtypes = [ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.POINTER(CodecPackedLayout)]
_lib.rir_codec_encode_packed_device.argtypes = [_vp, ct.c_int, ct.c_int, ct.c_int, ct.c_int, _vp, _vp, _vp, _vp, ct.c_longlong, _vp, ct.c_longlong, _vp]
_lib.rir_codec_encode_packed_launch_device.argtypes = [_vp, ct.c_int, ct.c_int, ct.c_int, ct.c_int, _vp, _vp, _vp, _vp, ct.c_longlong, _vp, ct.c_longlong, _vp]
_lib.rir_codec_packed_reset_device.argtypes = [_vp, ct.c_longlong, _vp]
_lib.rir_codec_encode_packed_status.argtypes = [_vp, ct.POINTER(ct.c_ulonglong), _vp]
_lib.rir_codec_decode_packed_device.argtypes = [_vp, _vp, _vp, _vp, ct.c_longlong, ct.c_int, ct.c_int, ct.c_int, ct.c_int, _vp, _vp, _vp]
_lib.rir_codec_decode_device.argtypes = [_vp, _vp, _vp, _vp, ct.c_longlong, ct.c_int, ct.c_int, ct.c_int, ct.c_int, _vp, _vp, _vp]
_lib.rir_codec_decode_chunks_device.argtypes = [_vp, _vp, _vp, _vp, ct.c_longlong, ct.c_int, ct.c_int, ct.c_int, ct.c_int, _vp, ct.c_longlong, _vp,
                                                _vp, _vp]
_lib.rir_translate_device.argtypes = [ct.c_int, _vp, _vp, ct.c_int, ct.c_int, ct.c_int, _vp, ct.c_int, _vp, ct.c_char_p, _vp]
_lib.rir_gaussian_filter_device.argtypes = [_vp, _vp, ct.c_int, ct.c_int, ct.c_int, ct.c_float, _vp]
_lib.rir_gaussian_filter_u16_device.argtypes = [_vp, _vp, ct.c_int, ct.c_int, ct.c_int, ct.c_float, _vp]
_lib.rir_translate_f32_u16_device.argtypes = [_vp, _vp, ct.c_int, ct.c_int, ct.c_int, _vp, ct.c_int, _vp, ct.c_char_p, _vp]
_lib.rir_filter_chain_device.argtypes = [ct.c_int, _vp, _vp, ct.c_int, ct.c_int, ct.c_int, ct.c_float, _vp, ct.c_int, _vp, ct.c_char_p, _vp]
_lib.rir_find_median_pixel_device.argtypes = [_vp, _vp, ct.c_int, ct.c_int, ct.c_float, _vp, _vp, _vp]
_lib.rir_bad_pixels_create_device.argtypes = [_vp, ct.c_int, ct.c_int, _vp]
_lib.rir_bad_pixels_create_rows_device.argtypes = [_vp, ct.c_int, ct.c_int, ct.c_int, _vp]
_lib.rir_bad_pixels_correct_device.argtypes = [ct.c_int, _vp, _vp, ct.c_int, _vp]
_lib.rir_bad_pixels_info.argtypes = [ct.c_int, _vp, _vp, ct.c_int]
_lib.rir_remove_bad_pixels_device.argtypes = [ct.c_int, _vp, ct.c_int, ct.c_int, _vp]
_lib.rir_remove_motion_device.argtypes = [_vp, _vp, ct.c_int, ct.c_int, ct.c_int, ct.c_int, _vp, _vp]
_lib.rir_median_filter_device.argtypes = [_vp, _vp, ct.c_int, ct.c_int, ct.c_int, _vp]
_lib.rir_temporal_median_device.argtypes = [_vp, _vp, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_int, _vp]
_lib.rir_morphology_device.argtypes = [ct.c_int, _vp, _vp] + [ct.c_int] * 7 + [_vp]
_lib.rir_rank_filter_device.argtypes = [ct.c_int, _vp, _vp] + [ct.c_int] * 7 + [_vp]
_lib.rir_local_stats_device.argtypes = [ct.c_int, _vp] + [ct.c_int] * 6 + [_vp] * 4
_lib.rir_local_threshold_device.argtypes = [ct.c_int, _vp, _vp] + [ct.c_int] * 10 + [_vp]
_lib.rir_distance_transform_device.argtypes = [ct.c_int, _vp] + [ct.c_int] * 6 + [_vp, _vp, _vp, ct.c_size_t, _vp]
_lib.rir_distance_transform_workspace_bytes.argtypes = [ct.c_int] * 4
_lib.rir_distance_transform_workspace_bytes.restype = ct.c_size_t
_lib.rir_reconstruct_device.argtypes = [ct.c_int, _vp, _vp, _vp] + [ct.c_int] * 9 + [_vp, ct.c_size_t, ct.POINTER(ct.c_int), _vp]
_lib.rir_reconstruct_workspace_bytes.argtypes = [ct.c_int] * 4
_lib.rir_reconstruct_workspace_bytes.restype = ct.c_size_t
_lib.rir_region_stats_device.argtypes =[_vp, _vp] + [ct.c_int] * 5 + [_vp] * 8 + [ct.c_size_t, _vp]
_lib.rir_region_stats_workspace_bytes.argtypes = [ct.c_int] * 5
_lib.rir_region_stats_workspace_bytes.restype = ct.c_size_t
_lib.rir_region_geometry_device.argtypes = [_vp, _vp] + [ct.c_int] * 5 + [_vp] * 5 + [ct.c_size_t, _vp]
_lib.rir_region_geometry_workspace_bytes.argtypes = [ct.c_int] * 6
_lib.rir_region_geometry_workspace_bytes.restype = ct.c_size_t
_lib.rir_region_quantiles_device.argtypes = [_vp, _vp] + [ct.c_int] * 5 + [_vp, ct.c_int, _vp, _vp, _vp, ct.c_size_t, _vp]
_lib.rir_region_quantiles_workspace_bytes.argtypes = [ct.c_int] * 6
_lib.rir_region_quantiles_workspace_bytes.restype = ct.c_size_t
_lib.rir_region_histogram_device.argtypes = [_vp, _vp] + [ct.c_int] * 9 + [_vp] * 4 + [ct.c_size_t, _vp]
_lib.rir_region_histogram_workspace_bytes.argtypes = [ct.c_int] * 7
_lib.rir_region_histogram_workspace_bytes.restype = ct.c_size_t
_lib.rir_pixel_stats_device.argtypes = [_vp] + [ct.c_int] * 5 + [_vp] * 7 + [ct.c_size_t, _vp]
_lib.rir_pixel_stats_workspace_bytes.argtypes = [ct.c_int] * 3
_lib.rir_pixel_stats_workspace_bytes.restype = ct.c_size_t
_lib.rir_pixel_quantiles_passes.argtypes = []
_lib.rir_pixel_quantiles_state_bytes.argtypes = [ct.c_int] * 3
_lib.rir_pixel_quantiles_state_bytes.restype = ct.c_size_t
_lib.rir_pixel_quantiles_workspace_bytes.argtypes = [ct.c_int] * 4
_lib.rir_pixel_quantiles_workspace_bytes.restype = ct.c_size_t
_lib.rir_pixel_quantiles_device.argtypes = [_vp] + [ct.c_int] * 3 + [_vp, ct.c_int, _vp, _vp, ct.c_size_t, _vp]
_lib.rir_pixel_quantiles_push_device.argtypes = [_vp] + [ct.c_int] * 5 + [_vp, ct.c_size_t, _vp]
_lib.rir_pixel_quantiles_resolve_device.argtypes = [ct.c_int, ct.c_int, _vp, ct.c_int, ct.c_int, ct.c_longlong, _vp, ct.c_size_t, _vp, _vp]
_lib.rir_track_components_device.argtypes = [_vp, _vp] + [ct.c_int] * 4 + [_vp] * 6 + [ct.c_int, _vp, _vp, ct.c_size_t, _vp]
_lib.rir_track_components_workspace_bytes.argtypes = [ct.c_int] * 4
_lib.rir_track_components_workspace_bytes.restype = ct.c_size_t
_lib.rir_polygon_map_device.argtypes = [_vp] * 3 + [ct.c_int] * 4 + [_vp] + [ct.c_int] * 3 + [_vp, _vp, ct.c_size_t, _vp]
_lib.rir_polygon_map_workspace_bytes.argtypes = [ct.c_int] * 5
_lib.rir_polygon_map_workspace_bytes.restype = ct.c_size_t
_lib.bad_pixels_destroy.argtypes = [ct.c_int]
_lib.rir_label_workspace_bytes.argtypes = [ct.c_int, ct.c_int]
_lib.rir_label_workspace_bytes.restype = ct.c_size_t
_lib.rir_label_workspace_bytes_batch.argtypes = [ct.c_int, ct.c_int, ct.c_int]
_lib.rir_label_workspace_bytes_batch.restype = ct.c_size_t
_lib.rir_label_hot_spots_workspace_bytes.argtypes = [ct.c_int, ct.c_int, ct.c_int]
_lib.rir_label_hot_spots_workspace_bytes.restype = ct.c_size_t
_lib.rir_label_hot_spots_device.argtypes = ([_vp] + [ct.c_int] * 5 + [_vp, ct.c_int, ct.c_int, _vp] + [ct.c_int] * 3 + [_vp] * 3
                                            + [ct.c_int, _vp, _vp, ct.c_size_t, _vp])
_lib.rir_label_images_device.argtypes =[ct.c_int, _vp, _vp, ct.c_int, ct.c_int, ct.c_int, _vp, _vp, _vp, ct.c_int, _vp, _vp, ct.c_size_t, _vp]
_lib.rir_keep_largest_areas_device.argtypes = [ct.c_int, _vp, _vp, ct.c_int, ct.c_int, ct.c_int, _vp, ct.c_int, _vp, ct.c_size_t, _vp]
_lib.rir_label_image_device.argtypes = [ct.c_int, _vp, _vp, ct.c_int, ct.c_int, _vp, _vp, _vp, _vp, _vp, ct.c_size_t, _vp]
_lib.rir_keep_largest_area_device.argtypes = [ct.c_int, _vp, _vp, ct.c_int, ct.c_int, _vp, ct.c_int, _vp, ct.c_size_t, _vp]
_lib.rir_lossy_create.argtypes = [ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_double, ct.c_int, ct.c_int, ct.c_int]
_lib.rir_lossy_step_device.argtypes = [ct.c_int, _vp, _vp, ct.c_int, ct.c_int, _vp, _vp, _vp]
_lib.rir_lossy_step_multi_device.argtypes = [_vp, ct.c_int, _vp, _vp, ct.c_int, ct.c_int, _vp, _vp, _vp]
_lib.rir_lossy_destroy.argtypes = [ct.c_int]
_lib.rir_lossy_status.argtypes = [ct.c_int, _vp]
_lib.rir_lossy_path_stats.argtypes = [ct.c_int, ct.POINTER(ct.c_int), _vp]
_lib.rir_lossy_spec_stats.argtypes = [ct.c_int, ct.POINTER(ct.c_int), _vp]
_lib.rir_lossy_set_errors.argtypes = [ct.c_int, ct.c_int, ct.c_int, ct.c_double]
_lib.rir_downsampler_create.argtypes = [ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_double, ct.c_int]
_lib.rir_downsampler_push_device.argtypes = [ct.c_int, _vp, ct.c_int, _vp, _vp, _vp, _vp, _vp]
_lib.rir_downsampler_count.argtypes = [ct.c_int]
_lib.rir_downsampler_destroy.argtypes = [ct.c_int]
_lib.rir_downsampler_destroy.restype = None
_lib.rir_downsample_decide.argtypes = [ct.c_int, ct.c_double, ct.c_int, ct.c_longlong, _vp, ct.c_int, _vp, _vp, _vp]
_lib.rir_downsample_state_bytes.restype = ct.c_size_t
_lib.rir_split_planes_device.argtypes = [_vp, _vp, ct.c_int, ct.c_int, ct.c_int, ct.c_int, _vp, _vp, _vp, _vp]
_lib.rir_merge_planes_device.argtypes = [_vp, _vp, _vp, ct.c_int, ct.c_int, ct.c_int, ct.c_int, _vp, _vp, _vp]
_lib.bad_pixels_destroy.restype = None


def device_available():
    return bool(_lib.rir_device_available())


def _stream():
    return ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def _check(r, what):
    if r != 0:
        raise RuntimeError("%s failed: %s" % (what, last_error()))


def _frames3(t, dtype=None):
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if t.dim() != 3 or not t.is_cuda:
        raise RuntimeError("expected a CUDA tensor of shape (n, h, w)")
    if dtype is not None and t.dtype != dtype:
        raise RuntimeError("expected dtype %s" % dtype)
    return t.contiguous()


# What the forms of the frame filters share ("The Python forms of the frame filters").
def _stack_of(t):
    """-> (the shape of `t`, that shape as a stack [n][h][w] - one image being a stack of one -, the numpy name of its dtype), the last two as the
    ``_..._args`` checkers take them"""
    shape = tuple(t.shape)
    return shape, (1,) + shape if len(shape) == 2 else shape, _DTYPE_NAMES.get(t.dtype) or str(t.dtype)


def _is_out(t, dtypes, shape, contiguous=True):
    """whether `t` can take an output: a CUDA tensor of one of `dtypes` and of `shape`, contiguous unless that is not asked for"""
    return isinstance(t, torch.Tensor) and t.is_cuda and t.dtype in dtypes and tuple(t.shape) == shape and (not contiguous or t.is_contiguous())


def _out_or_new(out, dtype, shape, device, message, *args):
    """`out` checked - a contiguous CUDA tensor of `dtype` and `shape`, else ``RuntimeError(message % args)``, the form's own words - or, for
    None, a new tensor on `device`"""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if not _is_out(out, (dtype,), shape):
        raise RuntimeError(message % args)
    return out


def _workspace(need, device):
    """an 8-byte aligned workspace of at least `need` bytes on `device`: work.data_ptr(), work.numel() * 8"""
    return torch.empty(need // 8 + 1, dtype=torch.int64, device=device)


def _queue(entry, n, *args):
    """queue `entry`, a ``rir_<name>_device`` of the C ABI, over `args` on the current stream, which is its last argument; nothing for n = 0 frames"""
    if n:
        _check(entry(*args, _stream()), entry.__name__)


def _queue_with_workspace(entry, workspace_bytes, query, device, n, *args, form=None, after=()):
    """``_queue`` for an entry that takes a workspace and its size behind `args` (and `after` behind those): the workspace is what its
    ``workspace_bytes(*query)`` asks for, on `device`; `form`: the name of a form to which 0 bytes mean that the geometry is refused"""
    if n:
        need = workspace_bytes(*query)
        if form is not None and need == 0:
            raise RuntimeError("%s: geometry refused" % form)
        work = _workspace(need, device)
        _queue(entry, n, *args, work.data_ptr(), work.numel() * 8, *after)


def codec_layout(width, height, nframes, gop=DEFAULT_GOP):
    L = CodecLayout()
    _check(_lib.rir_codec_layout_query(width, height, nframes, gop, ct.byref(L)), "rir_codec_layout_query")
    return L


class EncodedBatch:
    """Device-resident compressed batch (tables + compact stream), format RIRB1."""

    def __init__(self, layout, hdr, tile_off, chunk_off, stream):
        self.layout = layout
        self.hdr = hdr  # int64(bit pattern uint64) [nchunks, ntiles, gop]
        self.tile_off = tile_off  # int32(bit pattern uint32) [nchunks, ntiles+1]
        self.chunk_off = chunk_off  # int64 [nchunks+1]
        self.stream = stream  # int64 words (capacity = worst case)

    def total_words(self):
        return int(self.chunk_off[-1].item())

    def compressed_bytes(self):
        """stream + tables: what a container has to store"""
        L = self.layout
        return self.total_words() * 8 + L.hdr_bytes + L.tile_off_bytes + L.chunk_off_bytes


class _LibraryBuffer:
    """Device memory allocated by the library (rir_codec_workspace_create_device), seen from torch as a uint8 tensor that keeps
    this object - and so the allocation - alive."""

    def __init__(self, ptr, nbytes, destroy=None):
        self.ptr, self.nbytes = int(ptr), int(nbytes)
        self._destroy = destroy if destroy is not None else _lib.rir_codec_workspace_destroy_device
        self.__cuda_array_interface__ = {"shape": (self.nbytes,), "typestr": "|u1", "data": (self.ptr, False), "version": 2}

    def tensor(self, device):
        return torch.as_tensor(self, device=device)

    def __del__(self):
        try:
            if self.ptr:
                self._destroy(ct.c_void_p(self.ptr))
                self.ptr = 0
        except Exception:
            pass


def empty_beside(other, shape, dtype, tries=6, spacing_bytes=6 << 30):
    """A device tensor of ``shape`` / ``dtype`` in another placement class than the tensor ``other`` (rir_buffer_create_beside_device): the
    output buffer for a kernel that reads ``other`` and writes an output of similar size at the same pace - translate, gaussian_filter,
    filter_chain, median_filter are 5-10 % faster then (placement classes).  One-off set-up: candidates are
    allocated by the library, a streaming copy is timed on each, the rest is freed.  Returns (tensor, measured times in us, kept first)."""
    nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    nbytes = (nbytes + 15) // 16 * 16
    ptr = ct.c_void_p()
    times = (ct.c_float * (int(tries) + 1))()
    nt = ct.c_int(0)
    o = other.contiguous()
    _check(_lib.rir_buffer_create_beside_device(o.data_ptr(), o.numel() * o.element_size(), nbytes, int(tries), int(spacing_bytes), ct.byref(ptr), times,
                                                ct.byref(nt), _stream()), "rir_buffer_create_beside_device")
    owner = _LibraryBuffer(ptr.value, nbytes, _lib.rir_buffer_destroy_device)
    t = owner.tensor(other.device)[:int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()].view(dtype).view(*shape)
    t._rir_owner = owner  # (belt and braces: the allocation lives as long as the tensor object the caller holds)
    return t, [float(times[i]) for i in range(nt.value)]


class CodecContext:
    """Pre-allocated buffers for repeated encode/decode of one batch geometry (no allocation in
    the timed path)."""

    def __init__(self, width, height, nframes, gop=DEFAULT_GOP, device="cuda"):
        self.layout = L = codec_layout(width, height, nframes, gop)
        dev = torch.device(device)
        self.hdr = torch.zeros((L.nchunks, L.ntiles, L.gop), dtype=torch.int64, device=dev)
        self.tile_off = torch.zeros((L.nchunks, L.ntiles + 1), dtype=torch.int32, device=dev)
        self.chunk_off = torch.zeros((L.nchunks + 1,), dtype=torch.int64, device=dev)
        self.stream = torch.empty((L.stream_max_bytes // 8,), dtype=torch.int64, device=dev)
        self.workspace = torch.empty((L.workspace_bytes,), dtype=torch.uint8, device=dev)
        self.error = torch.zeros((1,), dtype=torch.int32, device=dev)

    def encode(self, frames, single_pass=False):
        """single_pass: the one-kernel encoder (dense stream written directly, decoupled look-back) - same outputs"""
        L = self.layout
        fr = _frames3(frames, torch.uint16)
        if tuple(fr.shape) != (L.nframes, L.height, L.width):
            raise RuntimeError("encode: frames do not match the context geometry")
        _check(
            (_lib.rir_codec_encode_single_pass_device if single_pass else _lib.rir_codec_encode_device)(
                fr.data_ptr(), L.width, L.height, L.nframes, L.gop, self.hdr.data_ptr(), self.tile_off.data_ptr(),
                self.chunk_off.data_ptr(), self.stream.data_ptr(), self.workspace.data_ptr(), L.workspace_bytes, _stream(),
            ),
            "rir_codec_encode_device",
        )
        return EncodedBatch(L, self.hdr, self.tile_off, self.chunk_off, self.stream)

    def place_workspace(self, frames, tries=6, spacing_bytes=6 << 30):
        """Replaces the encode workspace by one the LIBRARY allocates where the packing kernel runs fast for THIS frames buffer
        (rir_codec_workspace_create_device; DESIGN.md §7: device allocations fall into a few placement classes, and the kernel -
        frames in, slots out at the same pace - is 10 % slower when both are of one class).  One-off set-up of a few
        milliseconds; the candidates that lose and the spacers between them are freed by the library before it returns, torch's
        allocator is not touched.  There are three classes and they come in runs of 8-24 GiB of the address space
        (profiles/r03_placement/): candidates ``spacing_bytes`` apart, at most ``tries`` of them.  Returns the measured packing
        times in microseconds, the kept candidate's first."""
        L = self.layout
        fr = _frames3(frames, torch.uint16)
        if tuple(fr.shape) != (L.nframes, L.height, L.width):
            raise RuntimeError("place_workspace: frames do not match the context geometry")
        ptr = ct.c_void_p()
        times = (ct.c_float * (int(tries) + 1))()
        nt = ct.c_int(0)
        _check(_lib.rir_codec_workspace_create_device(fr.data_ptr(), L.width, L.height, L.nframes, L.gop, int(tries), int(spacing_bytes), ct.byref(ptr),
                                                      times, ct.byref(nt), _stream()), "rir_codec_workspace_create_device")
        owner = _LibraryBuffer(ptr.value, L.workspace_bytes)
        self.workspace = owner.tensor(self.hdr.device)
        self._workspace_owner = owner  # (the allocation lives as long as this context uses it, whatever torch keeps alive)
        return [float(times[i]) for i in range(nt.value)]

    def encode_status(self):
        """0 when the last single-pass encode completed, 1 when one of its look-backs gave up (waits for the stream)"""
        return int(_lib.rir_codec_encode_status(self.workspace.data_ptr(), _stream()))

    def encode_tiles(self, frames):
        """stage 1 only (single pass over the raw frames); finish with encode_compact()"""
        L = self.layout
        fr = _frames3(frames, torch.uint16)
        if tuple(fr.shape) != (L.nframes, L.height, L.width):
            raise RuntimeError("encode: frames do not match the context geometry")
        _check(_lib.rir_codec_encode_tiles_device(fr.data_ptr(), L.width, L.height, L.nframes, L.gop, self.hdr.data_ptr(),
                                                  self.workspace.data_ptr(), L.workspace_bytes, _stream()), "rir_codec_encode_tiles_device")

    def slots(self):
        """Views of the slotted form inside the workspace (valid after encode_tiles): (seg_words int32[nchunks, ntiles] - bit
        pattern uint32 -, slots int64[nchunks, ntiles, slot_words] - bit pattern uint64)."""
        L = self.layout
        S = CodecSlots()
        _check(_lib.rir_codec_slots_query(L.width, L.height, L.nframes, L.gop, ct.byref(S)), "rir_codec_slots_query")
        n = L.nchunks * L.ntiles
        seg = self.workspace[S.seg_words_offset_bytes:S.seg_words_offset_bytes + n * 4].view(torch.int32).view(L.nchunks, L.ntiles)
        sl = self.workspace[S.slots_offset_bytes:S.slots_offset_bytes + n * S.slot_words * 8].view(torch.int64).view(L.nchunks, L.ntiles, S.slot_words)
        return seg, sl

    def slots_payload_bytes(self):
        """payload bytes of the slotted batch in the workspace (sum of the segment lengths)"""
        return int(self.slots()[0].to(torch.int64).sum().item()) * 8

    def decode_slots(self, out=None, check=True):
        """decode of the slotted form left by encode_tiles (rir_codec_decode_slots_device): no second encoder pass"""
        L = self.layout
        if out is None:
            out = torch.empty((L.nframes, L.height, L.width), dtype=torch.uint16, device=self.hdr.device)
        if check:
            self.error.zero_()
        _check(_lib.rir_codec_decode_slots_device(self.hdr.data_ptr(), self.workspace.data_ptr(), L.workspace_bytes, L.width, L.height, L.nframes,
                                                  L.gop, out.data_ptr(), self.error.data_ptr(), _stream()), "rir_codec_decode_slots_device")
        if check and int(self.error.item()) != 0:
            raise RuntimeError("rir_codec_decode_slots_device: malformed stream")
        return out

    def encode_compact(self):
        L = self.layout
        _check(_lib.rir_codec_encode_compact_device(L.width, L.height, L.nframes, L.gop, self.tile_off.data_ptr(), self.chunk_off.data_ptr(),
                                                    self.stream.data_ptr(), self.workspace.data_ptr(), L.workspace_bytes, _stream()),
               "rir_codec_encode_compact_device")
        return EncodedBatch(L, self.hdr, self.tile_off, self.chunk_off, self.stream)

    def decode(self, enc, out=None, check=True):
        L = self.layout
        if out is None:
            out = torch.empty((L.nframes, L.height, L.width), dtype=torch.uint16, device=self.hdr.device)
        if check:
            self.error.zero_()
        _check(
            _lib.rir_codec_decode_device(
                enc.hdr.data_ptr(), enc.tile_off.data_ptr(), enc.chunk_off.data_ptr(), enc.stream.data_ptr(), enc.stream.numel(), L.width, L.height,
                L.nframes, L.gop, out.data_ptr(), self.error.data_ptr(), _stream(),
            ),
            "rir_codec_decode_device",
        )
        if check and int(self.error.item()) != 0:
            raise RuntimeError("rir_codec_decode_device: malformed stream")
        return out


class PackedBatch:
    """An encoded batch in the packed form: record headers, one (position, length) pair per (chunk, tile) segment and a stream
    buffer whose two ends hold the payload without holes - ``[0, low)`` and ``[capacity - high, capacity)`` words.  ``nbytes()``
    is what it occupies and what has to be kept, sent or written."""

    def __init__(self, codec, hdr, seg_pos, seg_words, stream, low, high):
        self.codec, self.hdr, self.seg_pos, self.seg_words, self.stream, self.low, self.high = codec, hdr, seg_pos, seg_words, stream, int(low), int(high)
        self.words = self.low + self.high

    def extents(self):
        """the two pieces of the payload as views of the stream buffer"""
        return self.stream[:self.low], self.stream[self.stream.numel() - self.high:]

    def payload_bytes(self):
        return self.words * 8

    def nbytes(self):
        return self.words * 8 + self.hdr.numel() * 8 + self.seg_pos.numel() * 8 + self.seg_words.numel() * 4


class PackedCodec:
    """Encode / decode of one batch geometry through the PACKED form (rir_codec_encode_packed_device): one pass over the
    frames, the encoded batch = exactly its payload + tables.  ``stream_bytes``: capacity of the stream buffer - default the
    8 bit-per-pixel budget (half the raw size; the reference documents a factor of about 5, docs/video_io.md:13), "max" = room
    for any data.  ``workspace_bytes``: default the minimum (control block + a small arena), "max" = room for any data.  A batch
    that does not fit raises in ``finish()`` / ``encode(..., check=True)`` with the sizes it needs; ``grow()`` provides them."""

    def __init__(self, width, height, nframes, gop=DEFAULT_GOP, device="cuda", stream_bytes=None, workspace_bytes=None):
        self.width, self.height, self.nframes, self.gop = int(width), int(height), int(nframes), int(gop)
        self.P = P = CodecPackedLayout()
        _check(_lib.rir_codec_packed_query(width, height, nframes, gop, ct.byref(P)), "rir_codec_packed_query")
        self.device = dev = torch.device(device)
        self.hdr = torch.zeros((P.nchunks, P.ntiles, self.gop), dtype=torch.int64, device=dev)
        self.seg_pos = torch.zeros((P.nchunks, P.ntiles), dtype=torch.int64, device=dev)
        self.seg_words = torch.zeros((P.nchunks, P.ntiles), dtype=torch.int32, device=dev)
        sb = P.stream_budget_bytes if stream_bytes is None else (P.stream_max_bytes if stream_bytes == "max" else int(stream_bytes))
        wb = P.workspace_min_bytes if workspace_bytes is None else (P.workspace_max_bytes if workspace_bytes == "max" else int(workspace_bytes))
        self.stream = torch.empty((max(sb // 8, 1),), dtype=torch.int64, device=dev)
        self.workspace = torch.empty((max(wb, 4096),), dtype=torch.uint8, device=dev)
        self.error = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.raw_bytes = self.width * self.height * self.nframes * 2
        # the packing kernel leaves the workspace's control block zero when it runs to its end: only a block not known to be so (a new
        # workspace, after grow(), after an encode whose status was not 0) is zeroed before the next encode - a fill launch of its own.
        # (the address of the workspace whose block is known to be zero: a workspace put in its place is not)
        self._clean_ws = None

    def reset(self):
        """the first half of encode(): zero the workspace's control block (a fill launch of its own)"""
        _check(_lib.rir_codec_packed_reset_device(self.workspace.data_ptr(), self.workspace.numel(), _stream()), "rir_codec_packed_reset_device")
        self._clean_ws = self.workspace.data_ptr()

    def encode(self, frames, check=False, reset=True):
        """Asynchronous; ``check=True`` (or a later ``finish()``) waits and returns the PackedBatch.  One launch when the control block is
        known to be clean (the previous encode on this stream left it so), else a fill launch before it.  ``reset=False``: the caller has
        just called reset() on the same stream (the packing kernel alone, for timings)."""
        fr = _frames3(frames, torch.uint16)
        if tuple(fr.shape) != (self.nframes, self.height, self.width):
            raise RuntimeError("encode: frames do not match the codec geometry")
        fill = reset and self._clean_ws != self.workspace.data_ptr()
        _check((_lib.rir_codec_encode_packed_device if fill else _lib.rir_codec_encode_packed_launch_device)(fr.data_ptr(), self.width, self.height, self.nframes, self.gop, self.hdr.data_ptr(), self.seg_pos.data_ptr(),
                                                   self.seg_words.data_ptr(), self.stream.data_ptr(), self.stream.numel(), self.workspace.data_ptr(),
                                                   self.workspace.numel(), _stream()), "rir_codec_encode_packed_device")
        self._clean_ws = self.workspace.data_ptr()
        return self.finish() if check else None

    def status(self):
        """(code, low words, high words, arena words asked for) of the last encode: code 0 complete, bit 0 stream capacity, bit 1 arena
        exceeded; waits."""
        out = (ct.c_ulonglong * 3)()
        r = int(_lib.rir_codec_encode_packed_status(self.workspace.data_ptr(), out, _stream()))
        if r != 0:
            self._clean_ws = None  # (the kernel leaves the block zero all the same; it is not relied upon after a failure)
        if r < 0:
            raise RuntimeError("rir_codec_encode_packed_status failed: %s" % last_error())
        return r, int(out[0]), int(out[1]), int(out[2])

    def finish(self):
        r, low, high, arena = self.status()
        if r != 0:
            raise RuntimeError("packed encode: the batch does not fit (code %d): it needs %d stream bytes (capacity %d) and asked for %d arena bytes "
                               "(capacity %d)" % (r, (low + high) * 8, self.stream.numel() * 8, arena * 8, self.workspace.numel() - 4096))
        return PackedBatch(self, self.hdr, self.seg_pos, self.seg_words, self.stream, low, high)

    def grow(self):
        """room for any data (after a batch did not fit)"""
        self.stream = torch.empty((self.P.stream_max_bytes // 8,), dtype=torch.int64, device=self.device)
        self.workspace = torch.empty((self.P.workspace_max_bytes,), dtype=torch.uint8, device=self.device)
        self._clean_ws = None

    def decode(self, batch=None, out=None, check=True):
        hdr, pos, seg, st = (batch.hdr, batch.seg_pos, batch.seg_words, batch.stream) if batch is not None else (self.hdr, self.seg_pos, self.seg_words, self.stream)
        if out is None:
            out = torch.empty((self.nframes, self.height, self.width), dtype=torch.uint16, device=self.device)
        if check:
            self.error.zero_()
        _check(_lib.rir_codec_decode_packed_device(hdr.data_ptr(), pos.data_ptr(), seg.data_ptr(), st.data_ptr(), st.numel(), self.width, self.height,
                                                   self.nframes, self.gop, out.data_ptr(), self.error.data_ptr(), _stream()), "rir_codec_decode_packed_device")
        if check and int(self.error.item()) != 0:
            raise RuntimeError("rir_codec_decode_packed_device: malformed batch")
        return out


def decode_chunks(hdr, tile_off, chunk_off, stream, chunk_frames, out, gop, error):
    """Chunks that do not form one contiguous batch (gathered from several shards): table entry k = one chunk,
    ``chunk_frames[k] = (first frame, frame count)`` inside ``out`` (N, H, W) uint16.  ``error``: int32[1] device tensor,
    raised to 1 on malformed tables; asynchronous on the current stream (rir_codec_decode_chunks_device)."""
    n, h, w = out.shape
    nchunks = chunk_frames.shape[0]
    if hdr.shape[0] < nchunks or tile_off.shape[0] < nchunks or chunk_off.numel() < nchunks + 1 or chunk_frames.dtype != torch.int64:
        raise RuntimeError("decode_chunks: tables do not cover the chunks")
    _check(
        _lib.rir_codec_decode_chunks_device(hdr.data_ptr(), tile_off.data_ptr(), chunk_off.data_ptr(), stream.data_ptr(), stream.numel(), w, h,
                                            nchunks, gop, chunk_frames.data_ptr(), n, out.data_ptr(), error.data_ptr(), _stream()),
        "rir_codec_decode_chunks_device",
    )
    return out


def translate(frames, offsets, strategy="", background=0):
    """frames (n,h,w) any supported dtype; offsets: (dx,dy) or tensor (n,2) of float32 per-frame shifts."""
    fr = _frames3(frames)
    n, h, w = fr.shape
    ch = _DTYPE_CHARS.get(fr.dtype)
    if ch is None:
        raise RuntimeError("translate: unsupported dtype")
    off = torch.as_tensor(offsets, dtype=torch.float32, device=fr.device).contiguous()
    per_frame = 1 if off.dim() == 2 else 0
    if per_frame and off.shape[0] != n:
        raise RuntimeError("translate: one (dx,dy) pair per frame expected")
    # "noborder" leaves the pixels without a source as they are and the wrapper pre-fills with the input
    # (reference rir_signal_processing.py:54-55): "noborder_source" is that, without the copy
    dst = torch.empty_like(fr)
    if strategy in ("", "noborder"):
        strategy = "noborder_source"
    back = np.zeros(1, dtype=_NP_OF[fr.dtype])
    back[0] = background
    if strategy == "constant":
        strategy = "background"
    _check(
        _lib.rir_translate_device(ord(ch), fr.data_ptr(), dst.data_ptr(), w, h, n, off.data_ptr(), per_frame, back.ctypes.data,
                                  strategy.encode(), _stream()),
        "rir_translate_device",
    )
    return dst


def gaussian_filter(frames, sigma):
    """float32 frames, or uint16 frames (converted on the fly: same result as frames.float(), sigma < 2.5)."""
    if frames.dtype == torch.uint16:
        fr = _frames3(frames, torch.uint16)
        n, h, w = fr.shape
        dst = torch.empty((n, h, w), dtype=torch.float32, device=fr.device)
        _check(_lib.rir_gaussian_filter_u16_device(fr.data_ptr(), dst.data_ptr(), w, h, n, float(sigma), _stream()), "rir_gaussian_filter_u16_device")
        return dst
    fr = _frames3(frames, torch.float32)
    n, h, w = fr.shape
    dst = torch.empty_like(fr)
    _check(_lib.rir_gaussian_filter_device(fr.data_ptr(), dst.data_ptr(), w, h, n, float(sigma), _stream()), "rir_gaussian_filter_device")
    return dst


def translate_to_u16(frames, offsets, strategy="nearest", background=0):
    """translate(float32 frames).to(uint16) in one pass (strategies that write every pixel)."""
    fr = _frames3(frames, torch.float32)
    n, h, w = fr.shape
    if strategy in ("", "noborder"):
        raise RuntimeError("translate_to_u16: 'noborder' needs a pre-filled destination, use translate()")
    off = torch.as_tensor(offsets, dtype=torch.float32, device=fr.device).contiguous()
    per_frame = 1 if off.dim() == 2 else 0
    if per_frame and off.shape[0] != n:
        raise RuntimeError("translate: one (dx,dy) pair per frame expected")
    dst = torch.empty((n, h, w), dtype=torch.uint16, device=fr.device)
    back = np.array([background], dtype=np.uint16)
    if strategy == "constant":
        strategy = "background"
    _check(_lib.rir_translate_f32_u16_device(fr.data_ptr(), dst.data_ptr(), w, h, n, off.data_ptr(), per_frame, back.ctypes.data,
                                             strategy.encode(), _stream()), "rir_translate_f32_u16_device")
    return dst


def filter_chain(frames, bad_pixels, sigma, offsets, strategy="nearest", background=0, out=None):
    """``bad_pixels.correct`` -> ``gaussian_filter(sigma)`` -> ``translate(offsets, strategy)`` -> uint16, in ONE pass over the
    uint16 frames (4 bytes of HBM traffic per pixel instead of 14); bit-identical to the three calls.  ``bad_pixels``: a
    ``BadPixels`` object or None.  Strategies "nearest" and "background"; for the others run the three calls."""
    fr = _frames3(frames, torch.uint16)
    n, h, w = fr.shape
    if strategy == "constant":
        strategy = "background"
    if strategy not in ("nearest", "background"):
        raise RuntimeError("filter_chain: strategy must be 'nearest' or 'background'")
    off = torch.as_tensor(offsets, dtype=torch.float32, device=fr.device).contiguous()
    per_frame = 1 if off.dim() == 2 else 0
    if per_frame and off.shape[0] != n:
        raise RuntimeError("filter_chain: one (dx,dy) pair per frame expected")
    if out is not None and (tuple(out.shape) != (n, h, w) or out.dtype != torch.uint16 or not out.is_contiguous() or out.data_ptr() == fr.data_ptr()):
        raise RuntimeError("filter_chain: out must be a contiguous uint16 tensor of the frames' shape, not the input")
    dst = out if out is not None else torch.empty((n, h, w), dtype=torch.uint16, device=fr.device)  # (out: e.g. from empty_beside(frames, ...))
    back = np.array([background], dtype=np.uint16)
    handle = bad_pixels.handle if bad_pixels is not None else 0
    _check(_lib.rir_filter_chain_device(handle, fr.data_ptr(), dst.data_ptr(), w, h, n, float(sigma), off.data_ptr(), per_frame, back.ctypes.data,
                                        strategy.encode(), _stream()), "rir_filter_chain_device")
    return dst


def find_median_pixel(frames, percent=0.5, mask=None):
    fr = _frames3(frames, torch.uint16)
    n, h, w = fr.shape
    res = torch.zeros((n,), dtype=torch.int32, device=fr.device)
    hist = torch.empty((n, 65536), dtype=torch.int32, device=fr.device)
    mptr = None
    if mask is not None:
        mask = _frames3(mask, torch.uint8)
        mptr = mask.data_ptr()
    _check(_lib.rir_find_median_pixel_device(fr.data_ptr(), mptr, h * w, n, float(percent), res.data_ptr(), hist.data_ptr(), _stream()),
           "rir_find_median_pixel_device")
    return res


class BadPixels:
    """Device-side counterpart of librir's BadPixels (reference src/python/librir/signal_processing/BadPixels.py)."""

    def __init__(self, first_image, rows=None):
        img = _frames3(first_image, torch.uint16)
        _, h, w = img.shape
        if rows is None:
            self.handle = _lib.rir_bad_pixels_create_device(img.data_ptr(), w, h, _stream())
        else:
            self.handle = _lib.rir_bad_pixels_create_rows_device(img.data_ptr(), w, h, int(rows), _stream())
        if self.handle <= 0:
            raise RuntimeError("bad_pixels_create failed: %s" % last_error())
        self.shape = (h, w)
        info = (ct.c_int * 3)()
        _lib.rir_bad_pixels_info(self.handle, info, None, 0)
        self.count, self.floor_correct, self.floor_detect = info[0], info[1], info[2]

    def positions(self):
        xy = np.zeros((max(self.count, 1), 2), dtype=np.int32)
        info = (ct.c_int * 3)()
        _lib.rir_bad_pixels_info(self.handle, info, xy.ctypes.data, self.count)
        return xy[: self.count]

    def correct(self, frames):
        fr = _frames3(frames, torch.uint16)
        out = torch.empty_like(fr)
        _check(_lib.rir_bad_pixels_correct_device(self.handle, fr.data_ptr(), out.data_ptr(), fr.shape[0], _stream()), "rir_bad_pixels_correct_device")
        return out

    def remove_inplace(self, frames, rows):
        fr = _frames3(frames, torch.uint16)
        _check(_lib.rir_remove_bad_pixels_device(self.handle, fr.data_ptr(), int(rows), fr.shape[0], _stream()), "rir_remove_bad_pixels_device")
        return fr

    def close(self):
        if getattr(self, "handle", 0) > 0:
            _lib.bad_pixels_destroy(self.handle)
            self.handle = 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def remove_motion(frames, shifts, rows=None):
    fr = _frames3(frames, torch.uint16)
    n, h, w = fr.shape
    sh = torch.as_tensor(shifts, dtype=torch.float32, device=fr.device).contiguous()
    out = torch.empty_like(fr)
    _check(_lib.rir_remove_motion_device(fr.data_ptr(), out.data_ptr(), w, h, h if rows is None else int(rows), n, sh.data_ptr(), _stream()),
           "rir_remove_motion_device")
    return out


def median_filter(frames):
    fr = _frames3(frames, torch.uint16)
    n, h, w = fr.shape
    out = torch.empty_like(fr)
    _check(_lib.rir_median_filter_device(fr.data_ptr(), out.data_ptr(), w, h, n, _stream()), "rir_median_filter_device")
    return out


def temporal_median(frames, window, threshold=0, rows=None, first=0, count=None, step=1, out=None):
    """Temporal median of a uint16 stack ``frames[n][h][w]`` (C ABI ``rir_temporal_median_device``), on the current stream: output k is
    frame t = first + k * step, the upper median ``sorted(S)[len(S) // 2]`` of the frames t - r .. t + r (r = window // 2; the window is
    truncated at the ends of ``frames``) where it differs from ``frames[t]`` by more than ``threshold``, ``frames[t]`` elsewhere; rows
    ``>= rows`` are copied.  ``count=None``: every position from ``first`` to the end at ``step``.  Returns ``[count][h][w]`` uint16
    (``out`` when given: a contiguous uint16 CUDA tensor of that shape that does not overlap ``frames``)."""
    if frames.dim() == 2:
        frames = frames.unsqueeze(0)
    rows, count = _temporal_median_args(tuple(frames.shape), window, threshold, rows, first, count, step)
    fr = _frames3(frames, torch.uint16)
    n, h, w = fr.shape
    out = _out_or_new(out, torch.uint16, (count, h, w), fr.device, "temporal_median: out must be a contiguous uint16 CUDA tensor of shape %s", (count, h, w))
    _queue(_lib.rir_temporal_median_device, count, fr.data_ptr(), out.data_ptr(), w, h, n, int(first), count, int(step), int(window), int(threshold), rows)
    return out


def _window_filter(name, check, entry, frames, own, size, rows, out):
    """``morphology`` and ``rank_filter``: the device entry of the C ABI over ``frames`` with the parameters that ``check`` passes, ``own``
    being the op or the rank"""
    shape, stack, dtype_name = _stack_of(frames)
    type_char, own, size_y, size_x, rows = check(stack, dtype_name, own, size, rows)
    out = _out_or_new(out, frames.dtype, shape, frames.device, "%s: out must be a contiguous %s CUDA tensor of shape %s", name, frames.dtype, shape)
    fr = _frames3(frames)
    n, h, w = fr.shape
    _queue(entry, n, type_char, fr.data_ptr(), out.data_ptr(), w, h, n, own, size_x, size_y, rows)
    return out


def morphology(frames, op, size, rows=None, out=None):
    """Flat morphology of a uint16, uint8 or bool stack ``frames[n][h][w]`` (or one image ``[h][w]``) with a centred rectangle ``size`` (an
    odd int, or ``(size_y, size_x)``, each 1..15) (C ABI ``rir_morphology_device``), one launch on the current stream.  ``op``: "erode" /
    "dilate" - min / max over the window clipped to the image, never padded -, "open" (dilate of erode), "close" (erode of dilate),
    "tophat" (frames - open), "blackhat" (close - frames), "gradient" (dilate - erode).  The image is the first ``rows`` rows of a frame
    (default: all); the others are copied.  Returns a tensor of the input's dtype and shape (``out`` when given: a contiguous CUDA tensor
    of that dtype and shape that does not overlap ``frames``)."""
    return _window_filter("morphology", _morphology_args, _lib.rir_morphology_device, frames, op, size, rows, out)


def erode(frames, size, rows=None, out=None):
    """``morphology(frames, "erode", ...)``: the minimum over the clipped window"""
    return morphology(frames, "erode", size, rows, out)


def dilate(frames, size, rows=None, out=None):
    """``morphology(frames, "dilate", ...)``: the maximum over the clipped window"""
    return morphology(frames, "dilate", size, rows, out)


def morph_open(frames, size, rows=None, out=None):
    """``morphology(frames, "open", ...)``: dilate(erode(frames)) - removes bright details smaller than the window"""
    return morphology(frames, "open", size, rows, out)


def morph_close(frames, size, rows=None, out=None):
    """``morphology(frames, "close", ...)``: erode(dilate(frames)) - fills dark details smaller than the window"""
    return morphology(frames, "close", size, rows, out)


def top_hat(frames, size, rows=None, out=None):
    """``morphology(frames, "tophat", ...)``: frames - open(frames), the bright details on a flattened background"""
    return morphology(frames, "tophat", size, rows, out)


def black_hat(frames, size, rows=None, out=None):
    """``morphology(frames, "blackhat", ...)``: close(frames) - frames, the dark details"""
    return morphology(frames, "blackhat", size, rows, out)


def morph_gradient(frames, size, rows=None, out=None):
    """``morphology(frames, "gradient", ...)``: dilate(frames) - erode(frames)"""
    return morphology(frames, "gradient", size, rows, out)


def rank_filter(frames, rank, size, rows=None, out=None):
    """Spatial rank filter of a uint16, uint8 or bool stack ``frames[n][h][w]`` (or one image ``[h][w]``) with a centred rectangle ``size``
    (an odd int, or ``(size_y, size_x)``, each 1..15) (C ABI ``rir_rank_filter_device``), one launch on the current stream: every pixel
    becomes the element of 0-based rank ``rank`` (negative: from the end, as in scipy) among the ``size_y * size_x`` values of its window.
    The window is always full - a position outside the image takes the nearest pixel, ``scipy.ndimage.rank_filter(..., mode="nearest")``
    - which is not the border rule of ``median_filter`` (a smaller window along the border).  The image is the first ``rows`` rows of a
    frame (default: all); the others are copied.  Returns a tensor of the input's dtype and shape (``out`` when given: a contiguous CUDA
    tensor of that dtype and shape that does not overlap ``frames``)."""
    return _window_filter("rank_filter", _rank_filter_args, _lib.rir_rank_filter_device, frames, rank, size, rows, out)


def _window_sizes(size):
    """(size_y, size_x) of a window parameter that ``_rank_filter_args`` is still to check (an unusable one: (1, 1))"""
    try:
        return _window_size("", size)
    except ValueError:
        return 1, 1


def window_median(frames, size, rows=None, out=None):
    """``rank_filter`` at rank ``size_y * size_x // 2``: the median of the full window, ``scipy.ndimage.median_filter(..., mode="nearest")``;
    3 x 3 and 5 x 5 on frames of even width stay in registers"""
    size_y, size_x = _window_sizes(size)
    return rank_filter(frames, size_y * size_x // 2, size, rows, out)


def percentile_filter(frames, percent, size, rows=None, out=None):
    """``rank_filter`` at ``percentile_rank(percent, size_y, size_x)``: ``scipy.ndimage.percentile_filter(..., mode="nearest")``; a negative
    percent counts from 100"""
    size_y, size_x = _window_sizes(size)
    return rank_filter(frames, percentile_rank(percent, size_y, size_x), size, rows, out)


_LOCAL_OUT = "%s: %s must be a contiguous %s CUDA tensor of shape %s"  # what local_stats and local_threshold say to an 'out' that does not fit


def local_stats(frames, size, rows=None, sum=True, sumsq=False, mean=False, out=None):
    """Local window statistics of a uint16, uint8 or bool stack ``frames[n][h][w]`` (or one image ``[h][w]``, which keeps its shape) over a
    centred rectangle ``size`` (an odd int, or ``(size_y, size_x)``, each 1..15) (C ABI ``rir_local_stats_device``), one launch on the
    current stream: a ``LocalStats`` of tensors of the input's shape - ``sum`` (int32) the window's sum S, ``sumsq`` (int64) its sum of
    squares Q, ``mean`` (the input's dtype) ``(S + n // 2) // n``, the mean rounded half up - with None for what was not asked for, and
    ``n`` = size_y * size_x.  The
    window is always full, coordinates replicated at the border (``mode="nearest"``, as ``rank_filter``).  The image is the first ``rows``
    rows of a frame (default: all); below them the sums are 0 and the mean is the input.  ``out``: a ``LocalStats`` (or a tuple ``(sum,
    sumsq, mean)``) with a contiguous CUDA tensor of the right dtype and shape for every output asked for, none of which overlaps
    ``frames`` or another; they are fully overwritten.  Non-contiguous input is copied first.  All integer, bit for bit
    (``local_variance_terms`` gives the exact variance); ``ValueError`` on bad parameters, before any device work."""
    shape, stack, dtype_name = _stack_of(frames)
    type_char, size_y, size_x, rows = _local_stats_args("local_stats", stack, dtype_name, size, rows, outputs=(sum, sumsq, mean))
    if out is not None and (not isinstance(out, (tuple, list)) or len(out) not in (3, 4)):
        raise RuntimeError("local_stats: out must be a LocalStats or a tuple (sum, sumsq, mean)")
    asked = zip((sum, sumsq, mean), LocalStats._fields, (torch.int32, torch.int64, frames.dtype))
    outs = [_out_or_new(None if out is None else out[k], dtype, shape, frames.device, _LOCAL_OUT, "local_stats", "out." + field, dtype, shape)
            if wanted else None for k, (wanted, field, dtype) in enumerate(asked)]
    fr = _frames3(frames)
    n, h, w = fr.shape
    _queue(_lib.rir_local_stats_device, n, type_char, fr.data_ptr(), w, h, n, size_x, size_y, rows, *(None if t is None else t.data_ptr() for t in outs))
    return LocalStats(*outs, size_y * size_x)


def box_sum(frames, size, rows=None, out=None):
    """``local_stats(...).sum``: the int32 sum of every pixel's ``size`` window (``out``: the int32 tensor it goes to)"""
    return local_stats(frames, size, rows, True, False, False, None if out is None else (out, None, None)).sum


def box_mean(frames, size, rows=None, out=None):
    """``local_stats(...).mean``: the mean of every pixel's ``size`` window, rounded half up, in the input's dtype (``out``: the tensor it
    goes to)"""
    return local_stats(frames, size, rows, False, False, True, None if out is None else (None, None, out)).mean


def local_threshold(frames, size, k, delta=0, polarity="above", rows=None, out=None):
    """The z-score mask of a uint16, uint8 or bool stack ``frames[n][h][w]`` (or one image ``[h][w]``) (C ABI ``rir_local_threshold_device``),
    one launch on the current stream that reads the stack once and writes a byte a pixel: a ``torch.bool`` tensor of the input's shape,
    True where the pixel lies more than ``delta`` (an int in -65535..65535) above the mean of its ``size`` window (an odd int, or ``(size_y,
    size_x)``, each 1..15) AND more than ``k`` population standard deviations of that window (centre pixel included) off it - ``k`` an int
    or ``(num, den)``, 0 <= num <= 255, 1 <= den <= 64.  Both tests are strict and exact: with S, Q the window's sum and sum of squares,
    ``d = n v - S`` and ``V = n Q - S^2``, "above" is ``d > delta n and d^2 den^2 > num^2 V``; ``polarity`` "below" takes ``-d`` in the first
    test, "both" either.  A constant window gives False; ``k = 0`` is "off the local mean by more than delta".  Window border and ``rows``
    as ``local_stats``; rows below the image are False.  ``out``: a contiguous bool or uint8 CUDA tensor of the input's shape that does not
    overlap ``frames`` (it receives 0 / 1 and is returned).  The mask - as uint8 through ``.view(torch.uint8)`` - is what ``label_images``
    and ``morphology`` take: ``label_images(morph_open(local_threshold(frames, 9, 4, delta=20).view(torch.uint8), 3))``.  ``ValueError`` on
    bad parameters, before any device work."""
    shape, stack, dtype_name = _stack_of(frames)
    type_char, size_y, size_x, rows, k_num, k_den, delta, polarity = _local_stats_args("local_threshold", stack, dtype_name, size, rows, k=k, delta=delta,
                                                                                       polarity=polarity)
    dtype = torch.uint8 if isinstance(out, torch.Tensor) and out.dtype == torch.uint8 else torch.bool  # (either is taken)
    out = _out_or_new(out, dtype, shape, frames.device, _LOCAL_OUT, "local_threshold", "out", dtype, shape)
    fr = _frames3(frames)
    n, h, w = fr.shape
    _queue(_lib.rir_local_threshold_device, n, type_char, fr.data_ptr(), out.data_ptr(), w, h, n, size_x, size_y, rows, k_num, k_den, delta, polarity)
    return out


def local_variance_terms(stats):
    """``(n Q - S^2, n^2)`` of a ``LocalStats`` that has ``sum`` and ``sumsq`` (tensors or numpy arrays): an int64 array that is n^2 times
    every window's population variance, exactly (at most 5.44e13), and the int n^2, n = ``stats.n`` being the window's cell count -
    ``terms.double() / n2`` is the variance in float64 from exact integers, 0 exactly where a window is constant"""
    if stats.sum is None or stats.sumsq is None:
        raise ValueError("local_variance_terms: the sum and the sum of squares are needed (local_stats(..., sum=True, sumsq=True))")
    wide = stats.sum.long() if isinstance(stats.sum, torch.Tensor) else stats.sum.astype(np.int64)
    return stats.n * stats.sumsq - wide * wide, stats.n * stats.n


_DISTANCE_WORK_BYTES = 256 << 20  # the workspace of one distance_transform call at most (or one frame's need): longer stacks go in groups


def _distance_transform_inputs(masks, background, border, rows, out, return_indices):
    """distance_transform's checks, the parameters first, which need no device; -> (masks [n][h][w], type char, background, border, rows,
    dist2, index or None), the outputs of the shape of `masks`"""
    shape, stack, dtype_name = _stack_of(masks)
    type_char, background, border, rows = _distance_transform_args(stack, dtype_name, background, border, rows)
    outs = (out if return_indices else (out,)) if out is not None else ()
    if out is not None and (not isinstance(outs, (tuple, list)) or len(outs) != 1 + bool(return_indices)
                            or not all(_is_out(t, (torch.int32,), shape) for t in outs)):
        raise RuntimeError("distance_transform: out must be %s of shape %s" % (
            "a pair (dist2, index) of contiguous int32 CUDA tensors" if return_indices else "a contiguous int32 CUDA tensor", shape))
    fr = _frames3(masks)
    dist2 = outs[0] if outs else torch.empty(shape, dtype=torch.int32, device=fr.device)
    index = None if not return_indices else outs[1] if outs else torch.empty(shape, dtype=torch.int32, device=fr.device)
    return fr, type_char, background, border, rows, dist2, index


def _distance_transform_into(fr, type_char, background, border, rows, dist2, index):
    """queue the transform of fr [n][h][w] into dist2 and index (None: not wanted), contiguous int32 of n * h * w cells; the workspace is
    that of the whole stack or _DISTANCE_WORK_BYTES worth of whole frames, and the entry walks the stack in groups that fit it"""
    n, h, w = fr.shape
    want = int(index is not None)
    one, need = _lib.rir_distance_transform_workspace_bytes(w, h, 1, want), _lib.rir_distance_transform_workspace_bytes(w, h, n, want)
    if one == 0:
        raise RuntimeError("distance_transform: geometry refused")
    work = _workspace(max(one, min(need, _DISTANCE_WORK_BYTES // one * one)), fr.device)  # (its size is not the query's answer: no _queue_with_workspace)
    _queue(_lib.rir_distance_transform_device, n, type_char, fr.data_ptr(), w, h, n, background, border, rows, dist2.data_ptr(),
           None if index is None else index.data_ptr(), work.data_ptr(), work.numel() * 8)


def distance_transform(masks, background=0, border=False, rows=None, return_indices=False, out=None):
    """Exact Euclidean distance transform of a bool, uint8, uint16 or int32 stack ``masks[n][h][w]`` (or one image ``[h][w]``) - masks or
    label maps - on the current stream (C ABI ``rir_distance_transform_device``, where the rule is defined): an int32 tensor of the input's
    shape with the SQUARED distance of every pixel to the nearest pixel of its image that equals ``background``, 0 on background,
    ``DIST2_NONE`` in an image without one.  ``border=True``: everything outside the image is background too.  The image is the first
    ``rows`` rows of a frame (default: all); the others get 0.  ``return_indices=True``: ``(dist2, index)``, index int32, the lowest flat
    index ``y * w + x`` among the nearest background pixels - the feature transform -, -1 where there is none or the outside is strictly
    nearer, a pixel's own index in the rows outside the image.  ``out``: a contiguous int32 CUDA tensor of the input's shape (a pair of them
    with ``return_indices``) that overlaps neither ``masks`` nor each other.  All integer, bit for bit; a stack whose workspace (2 bytes a
    pixel) exceeds 256 MiB goes through in groups of frames.  ``dist2 > r * r`` under a mask is its erosion by the disc of radius r
    (``disc_erode``); the per-region maximum of ``dist2`` under a label map is the squared inscribed radius of each region.  ``ValueError``
    on bad parameters, before any device work."""
    fr, type_char, background, border, rows, dist2, index = _distance_transform_inputs(masks, background, border, rows, out, return_indices)
    if fr.shape[0]:
        _distance_transform_into(fr, type_char, background, border, rows, dist2, index)
    return (dist2, index) if return_indices else dist2


def _disc_args(name, mask, radius):
    """the checks of the disc_* forms, which need no device; -> r2 = floor(radius^2)"""
    if mask.dtype not in (torch.bool, torch.uint8):
        raise ValueError("%s: a bool or uint8 mask expected, not %s" % (name, mask.dtype))
    if mask.dim() not in (2, 3) or min(mask.shape[-2:]) < 1 or max(mask.shape[-2:]) > DISTANCE_MAX_SIDE:
        raise ValueError("%s: a mask [h][w] or a stack [n][h][w] of 1..%d rows and columns expected" % (name, DISTANCE_MAX_SIDE))
    if isinstance(radius, (bool, np.bool_)) or not isinstance(radius, (int, float, np.integer, np.floating)) or not 0 <= radius < float("inf"):
        raise ValueError("%s: radius must be a non-negative number (got %r)" % (name, radius))
    r = float(radius)
    return int(min(np.floor(r * r), float(DIST2_NONE - 1)))  # (no distance inside a frame reaches 2^31 - 2)


def disc_erode(mask, radius, border=False):
    """Erosion of a bool or uint8 mask ``[n][h][w]`` (or ``[h][w]``; non-zero is set) by the Euclidean disc of ``radius`` (any non-negative
    number): a pixel stays set when no unset pixel lies within ``radius`` of it, ``mask & (distance_transform(mask) > floor(radius^2))`` -
    ``scipy.ndimage.binary_erosion`` with the disc ``dy^2 + dx^2 <= radius^2`` and ``border_value=1``; ``border=True`` counts the outside
    of the image as unset (``border_value=0``).  One distance transform, whatever the radius; radius 0 copies.  Returns a mask of the input's
    dtype (set is 1 / True)."""
    r2 = _disc_args("disc_erode", mask, radius)
    if not isinstance(border, (bool, np.bool_)) and border not in (0, 1):
        raise ValueError("disc_erode: border must be a bool")
    if radius == 0:
        return mask.clone()
    return ((mask != 0) & (distance_transform(mask, border=border) > r2)).to(mask.dtype)


def disc_dilate(mask, radius):
    """Dilation of a bool or uint8 mask by the Euclidean disc of ``radius``: a pixel is set when a set pixel lies within ``radius`` of it,
    ``distance_transform(mask == 0) <= floor(radius^2)`` - ``scipy.ndimage.binary_dilation`` with the disc ``dy^2 + dx^2 <= radius^2``.  The
    transform of the inverted mask (one torch op), whatever the radius: "grow every hot spot by 12 px" is ``disc_dilate(mask, 12)``.  Radius
    0 copies.  Returns a mask of the input's dtype."""
    r2 = _disc_args("disc_dilate", mask, radius)
    if radius == 0:
        return mask.clone()
    return (distance_transform(mask == 0) <= r2).to(mask.dtype)


def disc_open(mask, radius):
    """``disc_dilate(disc_erode(mask, radius), radius)``: removes what the disc does not fit into (``scipy.ndimage.binary_opening`` with the
    disc; the erosion takes the outside of the image as set, as ``disc_erode`` does by default)"""
    _disc_args("disc_open", mask, radius)
    return disc_dilate(disc_erode(mask, radius), radius)


def disc_close(mask, radius):
    """``disc_erode(disc_dilate(mask, radius), radius)``: fills what the disc does not fit into (``scipy.ndimage.binary_closing`` with the
    disc, the outside of the image taken as set by the erosion)"""
    _disc_args("disc_close", mask, radius)
    return disc_erode(disc_dilate(mask, radius), radius)


def _reconstruct(name, mask, marker, method, connectivity, rows, out, mode, h, output, return_rounds=False):
    """the reconstruction forms: ``rir_reconstruct_device`` over ``mask`` with the parameters checked first, which needs no device"""
    shape, stack, dtype_name = _stack_of(mask)
    type_char, method, connectivity, rows, param = _reconstruct_args(name, stack, dtype_name, method, connectivity, rows, h)
    if marker is not None and (not isinstance(marker, torch.Tensor) or marker.dtype != mask.dtype or tuple(marker.shape) != shape):
        raise ValueError("%s: the marker must be a tensor of the mask's dtype and shape" % name)
    out = _out_or_new(out, mask.dtype, shape, mask.device, "%s: out must be a contiguous %s CUDA tensor of shape %s", name, mask.dtype, shape)
    fr = _frames3(mask)
    seed = None if marker is None else _frames3(marker)
    n, height, w = fr.shape
    rounds = ct.c_int(0)
    _queue_with_workspace(_lib.rir_reconstruct_device, _lib.rir_reconstruct_workspace_bytes, (type_char, w, height, n), fr.device, n, type_char,
                          fr.data_ptr(), None if seed is None else seed.data_ptr(), out.data_ptr(), w, height, n, method, connectivity, mode, param,
                          output, rows, form=name, after=(ct.byref(rounds),))
    return (out, rounds.value) if return_rounds else out


def reconstruct(marker, mask, method="dilation", connectivity=8, rows=None, out=None, return_rounds=False):
    """Grey-level morphological reconstruction of ``marker`` under ``mask``, uint16, uint8 or bool CUDA stacks ``[n][h][w]`` (or one image
    ``[h][w]``) of the same dtype and shape (C ABI ``rir_reconstruct_device``, where the rule is defined).  ``method="dilation"``: the
    marker, clamped to ``min(marker, mask)``, spreads under the mask until nothing changes - the fixed point of ``min(mask, dilate(f, 3))``
    (``connectivity=8``) or of the same with the cross (4), the window clipped to the image; per pixel the best, over all paths that reach
    it, of the lowest mask value on the path and the marker at its start.  ``method="erosion"``: the dual, from ``max(marker, mask)`` down.
    This is ``skimage.morphology.reconstruction`` and, on bool, ``scipy.ndimage.binary_propagation(marker, structure, mask=mask)``: "keep
    what is connected to a marker".  The image is the first ``rows`` rows of a frame (default: all); the others are a copy of the mask.
    Bit for bit, whatever the reach: tiles converge in LDS and the call repeats rounds until one writes nothing, so it waits for the
    current stream between rounds - it is synchronous with the host and cannot be captured into a graph.  Returns a tensor of the input's
    dtype and shape (``out`` when given: a contiguous CUDA tensor of that dtype and shape that overlaps neither input);
    ``return_rounds=True``: ``(result, rounds)``.  ``ValueError`` on bad parameters, before any device work."""
    return _reconstruct("reconstruct", mask, marker, method, connectivity, rows, out, RECONSTRUCT_MARKER, _NO_SHIFT, 0, return_rounds)


def h_maxima(frames, h, connectivity=8, rows=None, out=None):
    """The h-maxima transform ``reconstruct(frames - h, frames)`` (the subtraction saturating at 0; no marker stack is stored): every
    maximum cut down by ``h``, or to the level at which it joins a higher one.  ``h``: an int in 0..the dtype's maximum."""
    return _reconstruct("h_maxima", frames, None, "dilation", connectivity, rows, out, RECONSTRUCT_SHIFT, h, 0)


def h_dome(frames, h, connectivity=8, rows=None, out=None):
    """The h-domes ``frames - h_maxima(frames, h)``: what stands above its surround, at most ``h`` of it, whatever the extent of the
    structure - a top-hat without a window, for hot spots larger than any window on an uneven background.  ``h_dome(f, 0)`` is 0."""
    return _reconstruct("h_dome", frames, None, "dilation", connectivity, rows, out, RECONSTRUCT_SHIFT, h, 1)


def h_minima(frames, h, connectivity=8, rows=None, out=None):
    """The dual of ``h_maxima``: ``reconstruct(frames + h, frames, "erosion")`` (the sum saturating at the dtype's maximum): every minimum
    raised by ``h``, or to the level at which it joins a lower one"""
    return _reconstruct("h_minima", frames, None, "erosion", connectivity, rows, out, RECONSTRUCT_SHIFT, h, 0)


def h_basin(frames, h, connectivity=8, rows=None, out=None):
    """The dual of ``h_dome``: ``h_minima(frames, h) - frames``, the depth, at most ``h``, of what lies below its surround"""
    return _reconstruct("h_basin", frames, None, "erosion", connectivity, rows, out, RECONSTRUCT_SHIFT, h, 1)


def _regional(name, method, frames, connectivity, rows, out):
    """``regional_maxima`` and ``regional_minima``: where the difference output of a shift by 1 is not 0"""
    shape, stack, dtype_name = _stack_of(frames)
    if out is not None and not _is_out(out, (torch.bool,), shape, contiguous=False):  # (torch.ne writes through any strides)
        _reconstruct_args(name, stack, dtype_name, method, connectivity, rows)  # (bad parameters come first)
        raise RuntimeError("%s: out must be a bool CUDA tensor of shape %s" % (name, shape))
    depth = _reconstruct(name, frames, None, method, connectivity, rows, None, RECONSTRUCT_SHIFT, 1, 1)
    found = torch.ne(depth.view(torch.int16) if depth.dtype == torch.uint16 else depth, 0, out=out)
    if rows is not None:
        found[..., int(rows):, :] = False  # (outside the image)
    return found


def regional_maxima(frames, connectivity=8, rows=None, out=None):
    """The regional maxima as a bool mask, ``h_dome(frames, 1) != 0``: the plateaus with no higher neighbour.  One consequence of the
    saturating marker: a plateau of value 0 is no maximum (a constant frame of zeros has none).  Rows outside the image are False."""
    return _regional("regional_maxima", "dilation", frames, connectivity, rows, out)


def regional_minima(frames, connectivity=8, rows=None, out=None):
    """The regional minima as a bool mask, ``h_basin(frames, 1) != 0``: the plateaus with no lower neighbour.  A plateau of the dtype's
    maximum is no minimum.  Rows outside the image are False."""
    return _regional("regional_minima", "erosion", frames, connectivity, rows, out)


def fill_holes(frames, connectivity=4, rows=None, out=None):
    """Reconstruction by erosion from the image's border (the marker is the frame on its border and the dtype's maximum inside; no marker
    stack is stored): every basin that does not reach the border is filled up to its rim.  On a bool mask at the default
    ``connectivity=4`` - the connectivity of the BACKGROUND - this is ``scipy.ndimage.binary_fill_holes``; it mends a hot spot with a
    saturated or repaired centre before ``region_geometry``, ``distance_transform`` or ``track_components``.  The border is that of the
    first ``rows`` rows."""
    return _reconstruct("fill_holes", frames, None, "erosion", connectivity, rows, out, RECONSTRUCT_BORDER, _NO_SHIFT, 0)


def clear_border(frames, connectivity=8, rows=None, out=None):
    """``frames - reconstruct(border marker, frames)``, the marker being the frame on the image's border and 0 inside: removes everything
    connected to the edge of the image, grey or binary (``skimage.segmentation.clear_border`` on a bool mask)"""
    return _reconstruct("clear_border", frames, None, "dilation", connectivity, rows, out, RECONSTRUCT_BORDER, _NO_SHIFT, 1)


class TemporalMedian:
    """``temporal_median`` over a sequence that arrives in batches.  ``push(frames)`` returns the outputs complete so far (they trail the
    input by window // 2 frames, so a push may return none), ``finish()`` the last ones, over windows truncated at the sequence's end;
    together they equal one ``temporal_median`` call over the concatenated input, bit for bit.  The object keeps at most window - 1 frames
    of history (copied once per push) and is ready for a new sequence after ``finish()`` or ``reset()``."""

    def __init__(self, window, threshold=0, rows=None):
        _temporal_median_args((1, 1 if rows is None else int(rows), 1), window, threshold, rows)
        self.window, self.threshold, self.rows = int(window), int(threshold), rows
        self.reset()

    def reset(self):
        self._shape = None  # (h, w) of the sequence
        self._hist = None  # input frames [base, seen) still needed
        self._base = 0
        self._seen = 0  # input frames pushed
        self._done = 0  # outputs returned

    def _range(self, batch, lo, hi):
        """input frames [lo, hi) from the history and the batch that starts at self._seen"""
        if lo >= self._seen:
            return batch[lo - self._seen:hi - self._seen]
        if hi <= self._seen:
            return self._hist[lo - self._base:hi - self._base]
        return torch.cat((self._hist[lo - self._base:], batch[:hi - self._seen]))

    def _outputs(self, stack, lo, t0, t1, out):
        """outputs [t0, t1) from `stack` = input frames lo .. into out"""
        temporal_median(stack, self.window, self.threshold, self.rows, first=t0 - lo, count=t1 - t0, out=out)

    def push(self, frames):
        fr = _frames3(frames, torch.uint16)
        if self._shape is None:
            self._shape = tuple(fr.shape[1:])
        elif tuple(fr.shape[1:]) != self._shape:
            raise ValueError("TemporalMedian.push: frames of shape %s, the sequence's are %s" % (tuple(fr.shape[1:]), self._shape))
        r = self.window // 2
        n0, n = self._seen, self._seen + fr.shape[0]
        t0, t1 = self._done, max(self._done, n - r)  # outputs whose window is complete
        out = torch.empty((t1 - t0,) + self._shape, dtype=torch.uint16, device=fr.device)
        split = min(max(t0, n0 + r if n0 else 0), t1)  # outputs from `split` on read the batch alone
        if split > t0:
            self._outputs(self._range(fr, max(0, t0 - r), split - 1 + r + 1), max(0, t0 - r), t0, split, out[:split - t0])
        if t1 > split:
            lo = max(0, split - r)
            self._outputs(fr[lo - n0:t1 - 1 + r + 1 - n0], lo, split, t1, out[split - t0:])
        keep = max(0, t1 - r)
        self._hist = self._range(fr, keep, n).clone()
        self._base, self._seen, self._done = keep, n, t1
        return out

    def finish(self):
        h, w = self._shape if self._shape is not None else (0, 0)
        t0, n = self._done, self._seen
        device = self._hist.device if self._hist is not None else torch.device("cuda", torch.cuda.current_device())
        out = torch.empty((n - t0, h, w), dtype=torch.uint16, device=device)
        if n > t0:
            self._outputs(self._hist, self._base, t0, n, out)
        self.reset()
        return out


def _region_inputs(frames, labels, nregions, what="region_stats", args=_region_stats_args):
    """region_stats' checks (region_quantiles' with its `what` and `args`), in the order that needs no device for the shapes, dtypes and
    nregions; -> (frames, labels, n, h, w, per_frame)"""
    if frames.dtype != torch.uint16:
        raise RuntimeError("%s: uint16 frames expected, not %s" % (what, frames.dtype))
    if labels.dtype != torch.int32:
        raise RuntimeError("%s: int32 labels expected, not %s" % (what, labels.dtype))
    n, h, w, per_frame = args(tuple(frames.shape), tuple(labels.shape), nregions)
    if not frames.is_cuda or not labels.is_cuda or frames.device != labels.device:
        raise RuntimeError("%s: frames and labels on one CUDA device expected" % what)
    return _frames3(frames), labels.contiguous(), n, h, w, per_frame


def _nregions(nregions, lab, check):
    """nregions as an int; for None, lab.max() + 1 (at least 1, synchronises), which check(nregions) sees again"""
    if nregions is None:
        nregions = max(1, int(lab.max()) + 1)
        check(nregions)
    return int(nregions)


def _region_stats_into(fr, lab, per_frame, nregions, out):
    """queue the statistics of fr [n][h][w] over lab into out (a RegionStats of contiguous [n][nregions] tensors)"""
    n, h, w = fr.shape
    _queue_with_workspace(_lib.rir_region_stats_device, _lib.rir_region_stats_workspace_bytes, (w, h, n, per_frame, nregions), fr.device, n,
                          fr.data_ptr(), lab.data_ptr(), w, h, n, per_frame, nregions, *(t.data_ptr() for t in out))


def _region_stats_empty(n, nregions, device):
    return RegionStats(*(torch.empty((n, nregions), dtype=dt, device=device)
                         for dt in (torch.int32, torch.int64, torch.int64, torch.int32, torch.int32, torch.int32, torch.int32)))


def region_stats(frames, labels, nregions=None):
    """Statistics of a uint16 stack ``frames (n, h, w)`` (or one ``(h, w)`` image: a stack of one) over the regions of the int32 label map
    ``labels`` (``(h, w)`` shared by every frame, or ``(n, h, w)``), on the current stream (C ABI ``rir_region_stats_device``): a
    ``RegionStats`` of CUDA tensors ``[n][nregions]`` - count, exact sum and sum of squares, min, max and the lowest flat index y * w + x of
    each.  Labels outside [0, nregions) are ignored; ``nregions=None`` takes ``labels.max() + 1`` (at least 1), which synchronises."""
    fr, lab, n, h, w, per_frame = _region_inputs(frames, labels, nregions)
    nregions = _nregions(nregions, lab, lambda k: _region_stats_args(tuple(frames.shape), tuple(labels.shape), k))
    out = _region_stats_empty(n, nregions, fr.device)
    if n:
        _region_stats_into(fr, lab, per_frame, nregions, out)
    return out


def _region_geometry_inputs(labels, frames, nregions):
    """region_geometry's checks, in the order that needs no device for the shapes, dtypes and nregions; -> (labels [h][w] or [n][h][w],
    frames [n][h][w] or None, n, h, w, per_frame)"""
    if frames is not None and frames.dtype != torch.uint16:
        raise RuntimeError("region_geometry: uint16 frames expected, not %s" % frames.dtype)
    if labels.dtype != torch.int32:
        raise RuntimeError("region_geometry: int32 labels expected, not %s" % labels.dtype)
    n, h, w, per_frame = _region_geometry_args(tuple(labels.shape), None if frames is None else tuple(frames.shape), nregions)
    if not labels.is_cuda or (frames is not None and (not frames.is_cuda or frames.device != labels.device)):
        raise RuntimeError("region_geometry: labels%s on one CUDA device expected" % ("" if frames is None else " and frames"))
    return labels.contiguous(), None if frames is None else _frames3(frames), n, h, w, per_frame


def _region_geometry_into(lab, fr, n, per_frame, nregions, out):
    """queue the geometry of lab ([h][w], or [n][h][w] with per_frame) weighted by fr ([n][h][w], or None) into out (a RegionGeometry of
    contiguous tensors, [n][nregions] leading)"""
    h, w = lab.shape[-2:]
    _queue_with_workspace(_lib.rir_region_geometry_device, _lib.rir_region_geometry_workspace_bytes,
                          (w, h, n, per_frame, nregions, int(fr is not None)), lab.device, n, lab.data_ptr(), None if fr is None else fr.data_ptr(), w, h, n, per_frame, nregions, out.count.data_ptr(), out.bbox.data_ptr(),
                          out.moments.data_ptr(), None if fr is None else out.weighted.data_ptr())


def _region_geometry_empty(n, nregions, weighted, device):
    return RegionGeometry(torch.empty((n, nregions), dtype=torch.int32, device=device), torch.empty((n, nregions, 4), dtype=torch.int32, device=device),
                          torch.empty((n, nregions, 5), dtype=torch.int64, device=device),
                          torch.empty((n, nregions, 3), dtype=torch.int64, device=device) if weighted else None)


def region_geometry(labels, nregions=None, frames=None):
    """Where the regions of the int32 label map ``labels`` (``(h, w)``, or ``(n, h, w)``) are and how they are spread, on the current stream
    (C ABI ``rir_region_geometry_device``): a ``RegionGeometry`` of CUDA tensors, ``[n][nregions]`` leading - count, the bounding box
    ``[..][4]`` = xmin, ymin, xmax, ymax (-1 for an empty region), the exact sums ``[..][5]`` of x, y, x^2, x*y, y^2 over the region and,
    with ``frames`` (uint16 ``(n, h, w)`` or one ``(h, w)`` image; a shared ``(h, w)`` map then serves every frame, each with its own
    row), the sums ``[..][3]`` of v, v*x, v*y; ``weighted`` is None without frames.  ``centroid()``, ``weighted_centroid()``,
    ``covariance()`` and ``ellipse()`` of the result give the derived float64 quantities.  Labels outside [0, nregions) are ignored;
    ``nregions=None`` takes ``labels.max() + 1`` (at least 1), which synchronises.  At most 32 768 rows and columns."""
    lab, fr, n, h, w, per_frame = _region_geometry_inputs(labels, frames, nregions)
    nregions = _nregions(nregions, lab, lambda k: _region_geometry_args(tuple(labels.shape), None if frames is None else tuple(frames.shape), k))
    out = _region_geometry_empty(n, nregions, fr is not None, lab.device)
    if n:
        _region_geometry_into(lab, fr, n, per_frame, nregions, out)
    return out


def _region_quantiles_into(fr, lab, per_frame, nregions, percents, out):
    """queue the quantiles of fr [n][h][w] over lab at percents (float32 numpy) into out (a RegionQuantiles of contiguous tensors)"""
    n, h, w = fr.shape
    _queue_with_workspace(_lib.rir_region_quantiles_device, _lib.rir_region_quantiles_workspace_bytes, (w, h, n, per_frame, nregions, percents.size),
                          fr.device, n, fr.data_ptr(), lab.data_ptr(), w, h, n, per_frame, nregions, percents.ctypes.data, percents.size, out.count.data_ptr(), out.values.data_ptr())


def _region_quantiles_empty(n, nregions, npercents, device):
    return RegionQuantiles(torch.empty((n, nregions), dtype=torch.int32, device=device),
                           torch.empty((n, nregions, npercents), dtype=torch.int32, device=device))


def region_quantiles(frames, labels, percents, nregions=None):
    """Quantiles of a uint16 stack ``frames (n, h, w)`` (or one ``(h, w)`` image: a stack of one) over the regions of the int32 label map
    ``labels`` (``(h, w)`` shared by every frame, or ``(n, h, w)``) at ``percents`` (a float or 1..8 floats in [0, 1]), on the current
    stream (C ABI ``rir_region_quantiles_device``, where the rule is defined): a ``RegionQuantiles`` of CUDA int32 tensors, count
    ``[n][nregions]`` and values ``[n][nregions][len(percents)]`` - for a non-empty region what
    ``find_median_pixel(frame, p, labels == r)`` gives, -1 for an empty one.  Labels outside [0, nregions) are ignored; at most 65 536
    regions; ``nregions=None`` takes ``labels.max() + 1`` (at least 1), which synchronises."""
    pc = _region_quantiles_percents(percents)
    fr, lab, n, h, w, per_frame = _region_inputs(frames, labels, nregions, "region_quantiles", _region_quantiles_args)
    nregions = _nregions(nregions, lab, lambda k: _region_quantiles_args(tuple(frames.shape), tuple(labels.shape), k))
    out = _region_quantiles_empty(n, nregions, pc.size, fr.device)
    if n:
        _region_quantiles_into(fr, lab, per_frame, nregions, pc, out)
    return out


def _region_histogram_inputs(frames, labels, nbins, lo, width, nregions, rows, what="region_histogram"):
    """region_histogram's checks (labels None: no map), in the order that needs no device for the shapes, dtypes, bins, rows and nregions;
    -> (frames, labels or None, n, h, w, per_frame, nbins, lo, width, rows)"""
    if frames.dtype != torch.uint16:
        raise RuntimeError("%s: uint16 frames expected, not %s" % (what, frames.dtype))
    if labels is not None and labels.dtype != torch.int32:
        raise RuntimeError("%s: int32 labels expected, not %s" % (what, labels.dtype))
    n, h, w, per_frame, nbins, lo, width, rows = _region_histogram_args(tuple(frames.shape), None if labels is None else tuple(labels.shape), nbins, lo,
                                                                        width, nregions, rows, what)
    if not frames.is_cuda or (labels is not None and (not labels.is_cuda or frames.device != labels.device)):
        raise RuntimeError("%s: frames%s on one CUDA device expected" % (what, "" if labels is None else " and labels"))
    return _frames3(frames), None if labels is None else labels.contiguous(), n, h, w, per_frame, nbins, lo, width, rows


def _region_histogram_into(fr, lab, per_frame, nregions, rows, out):
    """queue the histograms of the first `rows` rows of fr [n][h][w] over lab (None: one region) into out (a RegionHistogram of contiguous
    tensors, whose hist, lo and width give the bins)"""
    n, h, w = fr.shape
    nbins = out.hist.shape[-1]
    _queue_with_workspace(_lib.rir_region_histogram_device, _lib.rir_region_histogram_workspace_bytes, (w, h, rows, n, per_frame, nregions, nbins),
                          fr.device, n, fr.data_ptr(), None if lab is None else lab.data_ptr(), w, h, rows, n, per_frame, nregions, out.lo, out.width, nbins, out.count.data_ptr(),
                          out.hist.data_ptr(), out.outside.data_ptr())


def _region_histogram_empty(n, nregions, nbins, lo, width, device):
    return RegionHistogram(torch.empty((n, nregions), dtype=torch.int32, device=device),
                           torch.empty((n, nregions, nbins), dtype=torch.int32, device=device),
                           torch.empty((n, nregions, 2), dtype=torch.int32, device=device), lo, width)


def region_histogram(frames, labels, nbins, lo=0, width=1, nregions=None, rows=None):
    """Histograms of a uint16 stack ``frames (n, h, w)`` (or one ``(h, w)`` image: a stack of one) over the regions of the int32 label map
    ``labels`` (``(h, w)`` shared by every frame, or ``(n, h, w)``), on the current stream (C ABI ``rir_region_histogram_device``, where
    the bins are defined): a ``RegionHistogram`` of CUDA int32 tensors - count ``[n][nregions]``, hist ``[n][nregions][nbins]`` with
    ``nbins`` bins of ``width`` levels from ``lo``, outside ``[n][nregions][2]`` - whose ``edges()``, ``mode()``, ``cumulative()`` and
    ``otsu()`` give the derived quantities.  Only the first ``rows`` rows of every frame and map are counted (None: all).  Labels outside
    [0, nregions) are ignored; at most 65 536 regions and bins, nregions * nbins at most 2^24; ``nregions=None`` takes
    ``labels.max() + 1`` (at least 1), which synchronises.  ``labels=None`` is ``histogram``."""
    if labels is None:
        _region_histogram_args(tuple(frames.shape), None, nbins, lo, width, nregions, rows)
        return histogram(frames, nbins, lo, width, rows)
    fr, lab, n, h, w, per_frame, nbins, lo, width, rows = _region_histogram_inputs(frames, labels, nbins, lo, width, nregions, rows)
    nregions = _nregions(nregions, lab, lambda k: _region_histogram_args(tuple(frames.shape), tuple(labels.shape), nbins, lo, width, k, rows))
    out = _region_histogram_empty(n, nregions, nbins, lo, width, fr.device)
    if n:
        _region_histogram_into(fr, lab, per_frame, nregions, rows, out)
    return out


def histogram(frames, nbins, lo=0, width=1, rows=None):
    """``region_histogram`` without a map: the whole image (its first ``rows`` rows) is region 0, and only the frames are read - a
    ``RegionHistogram`` with count ``[n][1]``, hist ``[n][1][nbins]`` and outside ``[n][1][2]``."""
    fr, _, n, h, w, _, nbins, lo, width, rows = _region_histogram_inputs(frames, None, nbins, lo, width, 1, rows, "histogram")
    out = _region_histogram_empty(n, 1, nbins, lo, width, fr.device)
    if n:
        _region_histogram_into(fr, None, 0, 1, rows, out)
    return out


def _polygon_inputs(a, device):
    """the packed polygons, values and shifts of a PolygonMapArgs as contiguous tensors on `device` (None where there is none)"""
    def up(t, dtype):
        if t is None:
            return None
        if not isinstance(t, torch.Tensor):
            t = torch.from_numpy(np.ascontiguousarray(t))
        return t.to(device=device, dtype=dtype).contiguous()

    return up(a.xy, torch.float64), up(a.npts, torch.int32), up(a.values, torch.int32), up(a.shifts, torch.float64)


def _polygon_map_into(xy, npts, values, shifts, per_map, background, out):
    """queue the maps out [n][h][w] (contiguous int32) of the packed polygons xy [(n)][npoly][max_pts][2], npts [(n)][npoly]"""
    n, h, w = out.shape
    npoly, max_pts = xy.shape[-3], xy.shape[-2]
    _queue_with_workspace(_lib.rir_polygon_map_device, _lib.rir_polygon_map_workspace_bytes, (w, h, n, npoly, max_pts), out.device, n,
                          xy.data_ptr() if npoly else None, npts.data_ptr() if npoly else None,
                          values.data_ptr() if values is not None and npoly else None, npoly, max_pts, n, per_map,
                          shifts.data_ptr() if shifts is not None else None, w, h, int(background), out.data_ptr())


def polygon_map(polygons, shape, values=None, background=-1, shifts=None, out=None):
    """Polygon regions of interest rasterised into int32 label maps of ``shape`` (h, w) on the current stream (C ABI
    ``rir_polygon_map_device``), as ``region_stats`` takes them: the map is filled with ``background`` (-1: what region_stats ignores) and
    the polygons are painted in order with ``values`` (default 0, 1, ...), later ones over earlier ones, exactly as the reference's
    ``draw_polygon`` paints each.  ``polygons``: a list of (k, 2) array-likes of (x, y), packed on the host - one point draws a pixel, two a
    line - or a list of such lists, one per map, or a packed pair ``(xy, npts)`` of CUDA tensors (float64 (npoly, max_pts, 2) with int32
    (npoly,), or with a leading n for one set per map), used where they are.  ``shifts`` (n, 2), array or tensor: map m is drawn with every
    vertex moved by (dx, dy) = shifts[m].  -> an int32 CUDA tensor (h, w) for one set without shifts, else (n, h, w); ``out``: such a
    tensor to write into.  A polygon with a coordinate that is not finite or beyond 2^24 draws nothing.  ``ValueError`` on bad shapes."""
    a = _polygon_map_args(polygons, shape, values, background, None if isinstance(shifts, torch.Tensor) else shifts)
    if isinstance(shifts, torch.Tensor):  # stays on the device: only its shape is checked
        if shifts.dim() != 2 or shifts.shape[1] != 2 or (a.per_map and shifts.shape[0] != a.nmaps):
            raise ValueError("polygon_map: shifts (n, 2) expected%s, not %s" % (" with n = %d sets" % a.nmaps if a.per_map else "", tuple(shifts.shape)))
        a = a._replace(shifts=shifts, nmaps=shifts.shape[0], out_shape=(shifts.shape[0], a.h, a.w))
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.int32 or tuple(out.shape) != a.out_shape or not out.is_contiguous():
            raise RuntimeError("polygon_map: out must be a contiguous int32 tensor of shape %s" % (a.out_shape,))
        if not out.is_cuda:
            raise RuntimeError("polygon_map: out on a CUDA device expected")
    device = out.device if out is not None else a.xy.device if isinstance(a.xy, torch.Tensor) else torch.device("cuda", torch.cuda.current_device())
    if device.type != "cuda":
        raise RuntimeError("polygon_map: packed polygons on a CUDA device expected")
    if out is None:
        out = torch.empty(a.out_shape, dtype=torch.int32, device=device)
    if a.nmaps:
        _polygon_map_into(*_polygon_inputs(a, device), a.per_map, background, out.view(a.nmaps, a.h, a.w))
    return out


def _pixel_inputs(frames, sums, extremes, t0):
    """pixel_stats' checks, those that need no device first; -> (frames, n, h, w)"""
    if frames.dtype != torch.uint16:
        raise RuntimeError("pixel_stats: uint16 frames expected, not %s" % frames.dtype)
    n, h, w = _pixel_stats_args(tuple(frames.shape), sums, extremes, t0)
    if not frames.is_cuda:
        raise RuntimeError("pixel_stats: frames on a CUDA device expected")
    return _frames3(frames), n, h, w


def _pixel_stats_state(h, w, device, sums, extremes, empty):
    """the six outputs [h][w] (None for a group that is off); empty: in the empty state (sums 0, -1 elsewhere), else uninitialised"""
    def make(dtype, fill):
        return torch.full((h, w), fill, dtype=dtype, device=device) if empty else torch.empty((h, w), dtype=dtype, device=device)

    return [make(torch.int64, 0) if sums else None for _ in range(2)] + [make(torch.int32, -1) if extremes else None for _ in range(4)]


def _pixel_stats_into(fr, t0, accumulate, out):
    """queue the statistics of fr [n][h][w], n >= 1, into out (six contiguous [h][w] tensors or None), written or merged"""
    n, h, w = fr.shape
    _queue_with_workspace(_lib.rir_pixel_stats_device, _lib.rir_pixel_stats_workspace_bytes, (w, h, n), fr.device, n, fr.data_ptr(), w, h, n, int(t0),
                          int(accumulate),
                          *(None if t is None else t.data_ptr() for t in out))


def pixel_stats(frames, sums=True, extremes=True, t0=0):
    """Statistics over time of a uint16 stack ``frames (n, h, w)`` (or one ``(h, w)`` image: a stack of one), on the current stream (C ABI
    ``rir_pixel_stats_device``): a ``PixelStats`` of CUDA tensors ``[h][w]`` - per pixel the exact sum and sum of squares (``sums``), the
    min, the max and ``t0`` + the lowest frame index that holds each (``extremes``).  A group that is off is ``None`` and costs nothing."""
    fr, n, h, w = _pixel_inputs(frames, sums, extremes, t0)
    out = _pixel_stats_state(h, w, fr.device, sums, extremes, empty=n == 0)
    if n:
        _pixel_stats_into(fr, t0, 0, out)
    return PixelStats(*out, count=n)


class PixelStatsAccumulator:
    """``pixel_stats`` over a sequence that arrives in batches, in any order.  ``push(frames, t0)`` merges a batch whose first frame has time
    index ``t0`` into the state in place (``t0=None``: right after the highest index pushed so far); ``result()`` is the ``PixelStats`` so
    far, bit for bit that of one call over the frames pushed; ``merge(stats)`` takes in a result computed elsewhere (another device's shard,
    say) over other time indices.  The frame size is that of the first batch, or ``shape=(h, w)`` when given; before any frame arrives
    ``result()`` is the empty state - sums 0, -1 elsewhere, ``count`` 0 - of that size, or of size ``(0, 0)`` when none is known."""

    def __init__(self, sums=True, extremes=True, shape=None, device=None):
        _pixel_stats_args((0, 1, 1) if shape is None else (0,) + tuple(shape), sums, extremes)
        self.sums, self.extremes = bool(sums), bool(extremes)
        self._shape0 = None if shape is None else (int(shape[0]), int(shape[1]))
        self._device0 = device
        self.reset()

    def reset(self):
        self.count = 0  # frames behind the state
        self._next = 0  # one past the highest time index pushed
        self._out = None
        if self._shape0 is not None:
            dev = torch.device("cuda", torch.cuda.current_device()) if self._device0 is None else torch.device(self._device0)
            self._out = _pixel_stats_state(*self._shape0, dev, self.sums, self.extremes, empty=True)

    def _state(self, h, w, device):
        if self._out is None:
            self._out = _pixel_stats_state(h, w, device, self.sums, self.extremes, empty=True)
        ref = next(t for t in self._out if t is not None)
        if tuple(ref.shape) != (h, w) or ref.device != device:
            raise RuntimeError("PixelStatsAccumulator: frames of %s on %s expected, not %s on %s" % (tuple(ref.shape), ref.device, (h, w), device))
        return self._out

    def push(self, frames, t0=None):
        t = self._next if t0 is None else t0
        fr, n, h, w = _pixel_inputs(frames, self.sums, self.extremes, t)
        out = self._state(h, w, fr.device)
        if n:
            _pixel_stats_into(fr, t, 1, out)
            self.count += n
            self._next = max(self._next, int(t) + n)

    def merge(self, other):
        """take in ``other``, a ``PixelStats`` over time indices that were not pushed here: sums add; the smaller minimum wins and, of equal
        minima, the lower time index; likewise for the maximum.  ``other`` must hold the groups this accumulator keeps."""
        ref = next((t for t in other if t is not None), None)
        if ref is None or (self.sums and other.sum is None) or (self.extremes and other.min is None):
            raise ValueError("PixelStatsAccumulator.merge: the other result lacks a group that this one keeps")
        if not other.count:
            return
        h, w = ref.shape
        cur = self._out[0 if self.sums else 2].device if self._out is not None else None
        dev = cur if cur is not None else (ref.device if hasattr(ref, "is_cuda") and ref.is_cuda else torch.device("cuda", torch.cuda.current_device()))
        out = self._state(int(h), int(w), dev)
        o = [None if t is None else torch.as_tensor(t).to(dev) for t in other]
        if self.sums:
            out[0] += o[0]
            out[1] += o[1]
        if self.extremes:
            for val, arg, better in ((2, 4, torch.lt), (3, 5, torch.gt)):
                mine, theirs = out[val], o[val]
                take = (theirs >= 0) & ((mine < 0) | better(theirs, mine) | ((theirs == mine) & (o[arg] < out[arg])))
                out[arg].copy_(torch.where(take, o[arg], out[arg]))
                out[val].copy_(torch.where(take, theirs, mine))
        self.count += other.count

    def result(self):
        if self._out is None:
            dev = torch.device("cuda", torch.cuda.current_device()) if self._device0 is None else torch.device(self._device0)
            return PixelStats(*_pixel_stats_state(0, 0, dev, self.sums, self.extremes, empty=True), count=0)
        return PixelStats(*(None if t is None else t.clone() for t in self._out), count=self.count)


def _pixel_quantile_inputs(frames, what="pixel_quantiles"):
    """pixel_quantiles' checks on the frames, those that need no device first; -> (frames, n, h, w)"""
    if frames.dtype != torch.uint16:
        raise RuntimeError("%s: uint16 frames expected, not %s" % (what, frames.dtype))
    n, h, w = _pixel_quantiles_args(tuple(frames.shape), what)
    if not frames.is_cuda:
        raise RuntimeError("%s: frames on a CUDA device expected" % what)
    return _frames3(frames), n, h, w


def pixel_quantiles(frames, percents):
    """Quantiles over time of a uint16 stack ``frames (n, h, w)`` (or one ``(h, w)`` image: a stack of one) at ``percents`` (a float or 1..8
    floats in [0, 1]), on the current stream (C ABI ``rir_pixel_quantiles_device``, where the rule is defined): an int32 CUDA tensor
    ``(len(percents), h, w)``, one image per percent - ``pixel_quantiles(frames, 0.5)[0]`` is the median image.  Per pixel it is what
    ``find_median_pixel(series of the pixel, p, mask of ones)`` gives, the rule of ``region_quantiles``; -1 everywhere for no frames."""
    pc = _region_quantiles_percents(percents)
    fr, n, h, w = _pixel_quantile_inputs(frames)
    out = torch.empty((pc.size, h, w), dtype=torch.int32, device=fr.device)
    work = _workspace(_lib.rir_pixel_quantiles_workspace_bytes(w, h, n, pc.size), fr.device)  # (queued for no frames too: they give -1 everywhere)
    _check(_lib.rir_pixel_quantiles_device(fr.data_ptr() if n else None, w, h, n, pc.ctypes.data, pc.size, out.data_ptr(), work.data_ptr(),
                                           work.numel() * 8, _stream()), "rir_pixel_quantiles_device")
    return out


class PixelQuantileSelector:
    """``pixel_quantiles`` over a sequence that is not resident: the sequence is streamed ``passes`` times.  In every pass ``push(frames)``
    takes the batches of the sequence, in any order, and ``next_pass()`` closes the pass; after the last one ``result()`` is the int32
    ``(len(percents), h, w)`` tensor, bit for bit that of one ``pixel_quantiles`` call over the whole sequence.  Every pass must see the
    same frames: closing a later pass with another frame count than pass 0 raises ``RuntimeError``.  ``reset()`` starts over.  The frame
    size is that of the first batch, or ``shape=(h, w)`` when given; with no frames pushed ``result()`` is all -1 of that size, or of shape
    ``(len(percents), 0, 0)`` when none is known.  The state is 72 bytes per pixel and percent, whatever the length of the sequence.
    Digit counts add: shards of a sequence on several devices could be merged by adding their states before each pass is closed (not
    built)."""

    def __init__(self, percents, shape=None, device=None):
        self._pc = _region_quantiles_percents(percents)
        if shape is not None:
            _pixel_quantiles_args((0,) + tuple(shape), "PixelQuantileSelector")
        self.passes = int(_lib.rir_pixel_quantiles_passes())
        self._shape0 = None if shape is None else (int(shape[0]), int(shape[1]))
        self._device0 = device
        self.reset()

    def reset(self):
        self.pass_index = 0  # the open pass; == passes: all closed
        self.count = 0  # frames pushed in the open pass
        self._total = None  # frames of pass 0
        self._state = self._values = None

    def _device(self):
        if self._device0 is None:
            return torch.device("cuda", torch.cuda.current_device())
        d = torch.device(self._device0)
        return torch.device("cuda", torch.cuda.current_device()) if d.type == "cuda" and d.index is None else d

    def _make(self, h, w, device):
        need = _lib.rir_pixel_quantiles_state_bytes(w, h, self._pc.size)
        self._state = torch.zeros(need // 8 + 1, dtype=torch.int64, device=device)  # all zero: the empty state
        self._values = torch.empty((self._pc.size, h, w), dtype=torch.int32, device=device)

    def push(self, frames):
        fr, n, h, w = _pixel_quantile_inputs(frames, "PixelQuantileSelector")
        if self.pass_index >= self.passes:
            raise RuntimeError("PixelQuantileSelector: every pass is closed; reset() starts a new sequence")
        if self._shape0 is not None and (h, w) != self._shape0:
            raise RuntimeError("PixelQuantileSelector: frames of %s expected, not %s" % (self._shape0, (h, w)))
        if self._device0 is not None and fr.device != self._device():
            raise RuntimeError("PixelQuantileSelector: frames on %s expected, not on %s" % (self._device(), fr.device))
        if self._state is None:
            self._make(h, w, fr.device)
        if tuple(self._values.shape[1:]) != (h, w) or self._values.device != fr.device:
            raise RuntimeError("PixelQuantileSelector: frames of %s on %s expected, not %s on %s"
                               % (tuple(self._values.shape[1:]), self._values.device, (h, w), fr.device))
        if n:
            _check(_lib.rir_pixel_quantiles_push_device(fr.data_ptr(), w, h, n, self._pc.size, self.pass_index, self._state.data_ptr(),
                                                        self._state.numel() * 8, _stream()), "rir_pixel_quantiles_push_device")
            self.count += n

    def next_pass(self):
        if self.pass_index >= self.passes:
            raise RuntimeError("PixelQuantileSelector: every pass is closed")
        if self.pass_index == 0:
            self._total = self.count
        elif self.count != self._total:
            raise RuntimeError("PixelQuantileSelector: pass %d saw %d frames, pass 0 saw %d" % (self.pass_index, self.count, self._total))
        if self._state is None and self._shape0 is not None:
            self._make(*self._shape0, self._device())
        if self._state is not None:
            _, h, w = self._values.shape
            _check(_lib.rir_pixel_quantiles_resolve_device(w, h, self._pc.ctypes.data, self._pc.size, self.pass_index, self._total,
                                                           self._state.data_ptr(), self._state.numel() * 8, self._values.data_ptr(), _stream()),
                   "rir_pixel_quantiles_resolve_device")
        self.pass_index += 1
        self.count = 0

    def result(self):
        if self.pass_index < self.passes:
            raise RuntimeError("PixelQuantileSelector: result() after pass %d of %d; push the sequence and call next_pass() for each"
                               % (self.pass_index, self.passes))
        if self._values is None:
            return torch.full((self._pc.size, 0, 0), -1, dtype=torch.int32, device=self._device())
        return self._values.clone()


def _label_args(image, background):
    if image.dim() != 2 or not image.is_cuda:
        raise RuntimeError("label_image: one (h, w) image on the device expected")
    img = image.contiguous()
    ch = _DTYPE_CHARS.get(img.dtype)
    if ch is None:
        raise RuntimeError("label_image: unsupported dtype")
    h, w = img.shape
    need = _lib.rir_label_workspace_bytes(w, h)
    if need == 0:
        raise RuntimeError("label_image: geometry refused")
    work = _workspace(need, img.device)
    back = np.zeros(1, dtype=_NP_OF[img.dtype])
    back[0] = background
    return img, ch, h, w, work, back


def label_image(image, background=0):
    """Connected components of one image in device memory (reference Filters.h:365-509): (labels int32 (h, w), areas, first-pixel table),
    everything on the device; entry 0 of the tables is the background's."""
    img, ch, h, w, work, back = _label_args(image, background)
    dst = torch.empty((h, w), dtype=torch.int32, device=img.device)
    xy = torch.empty((h * w + 1, 2), dtype=torch.float64, device=img.device)
    area = torch.empty(h * w + 1, dtype=torch.int32, device=img.device)
    count = torch.zeros(1, dtype=torch.int32, device=img.device)
    _check(_lib.rir_label_image_device(ord(ch), img.data_ptr(), dst.data_ptr(), w, h, back.ctypes.data, xy.data_ptr(), area.data_ptr(),
                                       count.data_ptr(), work.data_ptr(), work.numel() * 8, _stream()), "rir_label_image_device")
    r = int(count.item())
    return dst, area[:r], xy[:r]


def keep_largest_area(image, background=0, foreground=1):
    """`foreground` on the largest component, int(background) elsewhere (reference Filters.h:511-540), int32 (h, w) on the device."""
    img, ch, h, w, work, back = _label_args(image, background)
    dst = torch.empty((h, w), dtype=torch.int32, device=img.device)
    _check(_lib.rir_keep_largest_area_device(ord(ch), img.data_ptr(), dst.data_ptr(), w, h, back.ctypes.data, int(foreground), work.data_ptr(),
                                             work.numel() * 8, _stream()), "rir_keep_largest_area_device")
    return dst


def _label_batch_args(frames, background):
    fr = _frames3(frames)
    if not fr.is_cuda:
        raise RuntimeError("label_images: frames on the device expected")
    ch = _DTYPE_CHARS.get(fr.dtype)
    if ch is None:
        raise RuntimeError("label_images: unsupported dtype")
    n, h, w = fr.shape
    need = _lib.rir_label_workspace_bytes_batch(w, h, n)
    if need == 0:
        raise RuntimeError("label_images: geometry refused")
    work = _workspace(need, fr.device)
    back = np.zeros(1, dtype=_NP_OF[fr.dtype])
    back[0] = background
    return fr, ch, n, h, w, work, back


def _label_images_into(frames, background, dst, xy, area, count):
    """queue the labelling of a batch into dst int32 (n, h, w), xy float64 (n, cap, 2), area int32 (n, cap) and count int32 (n,), all contiguous"""
    fr, ch, n, h, w, work, back = _label_batch_args(frames, background)
    _check(_lib.rir_label_images_device(ord(ch), fr.data_ptr(), dst.data_ptr(), w, h, n, back.ctypes.data, xy.data_ptr(), area.data_ptr(),
                                        area.shape[1], count.data_ptr(), work.data_ptr(), work.numel() * 8, _stream()), "rir_label_images_device")


def label_images(frames, background=0, table_entries=None):
    """Connected components of every image of a batch (n, h, w) in device memory, five launches for the whole batch: (labels int32 (n, h, w),
    areas (n, table_entries), first-pixel table (n, table_entries, 2), counts (n,)), on the device.  counts[i] = components of image i + 1;
    a table with fewer entries than that holds the first ``table_entries`` of them (default: 1 024 entries, or h*w + 1 if that is less)."""
    fr = _frames3(frames)
    n, h, w = fr.shape
    cap = min(1024, h * w + 1) if table_entries is None else int(table_entries)
    dst = torch.empty((n, h, w), dtype=torch.int32, device=fr.device)
    xy = torch.zeros((n, cap, 2), dtype=torch.float64, device=fr.device)
    area = torch.zeros((n, cap), dtype=torch.int32, device=fr.device)
    count = torch.zeros(n, dtype=torch.int32, device=fr.device)
    _label_images_into(fr, background, dst, xy, area, count)
    return dst, area, xy, count


class HotSpotFilter(namedtuple("HotSpotFilter", "low low_map use_high high high_map min_area max_area clear_border rows table_entries")):
    """The checked parameters of a ``label_hot_spots`` call: thresholds as int32 in [-1, 65535] - a number, and None or an (h, w) int32 map
    (numpy, or a tensor where a tensor was given) that takes its place -, the area window, and the rows that count."""

    __slots__ = ()


def _hot_spot_threshold(t, h, w, name):
    """a threshold as label_hot_spots takes it -> (int, None) or (0, int32 (h, w) map); a float t stands for floor(t): v > t == v > floor(t) for
    an integer v"""
    if isinstance(t, (bool, np.bool_)):
        raise ValueError("label_hot_spots: %s must be a number or an (h, w) map, not a bool" % name)
    if isinstance(t, (int, np.integer)):
        return min(max(int(t), -1), 65535), None
    if isinstance(t, (float, np.floating)):
        if t != t:
            raise ValueError("label_hot_spots: %s is NaN" % name)
        return int(np.floor(min(max(float(t), -1.0), 65535.0))), None
    if isinstance(t, torch.Tensor):
        if tuple(t.shape) != (h, w):
            raise ValueError("label_hot_spots: %s must be a number or an (h, w) = %s map, not shape %s" % (name, (h, w), tuple(t.shape)))
        f = t.to(torch.float64)
        if bool(torch.isnan(f).any()):
            raise ValueError("label_hot_spots: %s holds a NaN" % name)
        return 0, f.clamp(-1.0, 65535.0).floor().to(torch.int32).contiguous()
    a = np.asarray(t)
    if a.dtype.kind not in "biuf":
        raise ValueError("label_hot_spots: %s must be a number or an (h, w) map of numbers" % name)
    if a.shape != (h, w):
        raise ValueError("label_hot_spots: %s must be a number or an (h, w) = %s map, not shape %s" % (name, (h, w), a.shape))
    f = a.astype(np.float64)
    if np.isnan(f).any():
        raise ValueError("label_hot_spots: %s holds a NaN" % name)
    return 0, np.ascontiguousarray(np.floor(np.clip(f, -1.0, 65535.0)).astype(np.int32))


def _label_hot_spots_args(shape, low, high=None, min_area=1, max_area=None, clear_border=False, rows=None, table_entries=None):
    """the parameters of a label_hot_spots call over frames of `shape`, (h, w) or (n, h, w), checked without a device; -> (n, h, w, HotSpotFilter)"""
    if len(shape) not in (2, 3):
        raise ValueError("label_hot_spots: frames (n, h, w) or one image (h, w) expected")
    n, h, w = (1,) + tuple(shape) if len(shape) == 2 else tuple(shape)
    if h < 1 or w < 1 or h * w > TRACK_MAX_INDEX:
        raise ValueError("label_hot_spots: frames of at least 1x1 and at most 0x7FFF0000 pixels expected")
    lo, lo_map = _hot_spot_threshold(low, h, w, "low")
    hi, hi_map = (0, None) if high is None else _hot_spot_threshold(high, h, w, "high")
    if isinstance(min_area, bool) or not isinstance(min_area, (int, np.integer)) or min_area < 1:
        raise ValueError("label_hot_spots: min_area must be an int >= 1 (got %r)" % (min_area,))
    if max_area is not None and (isinstance(max_area, bool) or not isinstance(max_area, (int, np.integer)) or max_area < min_area):
        raise ValueError("label_hot_spots: max_area must be an int >= min_area (got %r)" % (max_area,))
    if rows is not None and (isinstance(rows, bool) or not isinstance(rows, (int, np.integer)) or not 1 <= rows <= h):
        raise ValueError("label_hot_spots: rows must be in 1..h (got %r)" % (rows,))
    if table_entries is not None and (int(table_entries) != table_entries or not 1 <= table_entries <= 0x7FFFFFFF):
        raise ValueError("label_hot_spots: table_entries must be in 1..2^31 - 1 (got %r)" % (table_entries,))
    cap = min(1024, h * w + 1) if table_entries is None else int(table_entries)
    return n, h, w, HotSpotFilter(lo, lo_map, high is not None, hi, hi_map, min(int(min_area), 0x7FFFFFFF),
                                  0x7FFFFFFF if max_area is None else min(int(max_area), 0x7FFFFFFF), bool(clear_border),
                                  h if rows is None else int(rows), cap)


def _hot_spot_maps_on(spec, device):
    """the filter with its threshold maps as int32 tensors on `device`"""
    def place(m):
        return None if m is None else (m if isinstance(m, torch.Tensor) else torch.from_numpy(m)).to(device)

    return spec._replace(low_map=place(spec.low_map), high_map=place(spec.high_map))


def _label_hot_spots_into(frames, spec, dst, first, area, count):
    """queue the labelling of the hot spots of uint16 frames (n, h, w) on the device under ``spec`` (a HotSpotFilter for frames of this size) into
    dst int32 (n, h, w), first and area int32 (n, cap) and count int32 (n,), all contiguous"""
    fr = _frames3(frames, torch.uint16)
    n, h, w = fr.shape
    need = _lib.rir_label_hot_spots_workspace_bytes(w, h, n)
    if need == 0:
        raise RuntimeError("label_hot_spots: geometry refused")
    spec = _hot_spot_maps_on(spec, fr.device)
    work = _workspace(need, fr.device)
    _check(_lib.rir_label_hot_spots_device(fr.data_ptr(), w, h, n, spec.rows, spec.low, None if spec.low_map is None else spec.low_map.data_ptr(),
                                           int(spec.use_high), spec.high, None if spec.high_map is None else spec.high_map.data_ptr(),
                                           spec.min_area, spec.max_area, int(spec.clear_border), dst.data_ptr(), first.data_ptr(), area.data_ptr(),
                                           area.shape[1], count.data_ptr(), work.data_ptr(), work.numel() * 8, _stream()), "rir_label_hot_spots_device")


def label_hot_spots(frames, low, high=None, min_area=1, max_area=None, clear_border=False, rows=None, table_entries=None):
    """The hot spots of uint16 frames (n, h, w) (or one image) in device memory, detected, filtered and numbered without a mask in memory
    (C ABI ``rir_label_hot_spots_device``): (labels int32 (n, h, w), area (n, table_entries), first (n, table_entries), counts (n,)), on the
    device.  Pixel (y, x) is foreground when ``y < rows`` (default: every row) and its value is ``> low``; components are the 4-connected
    sets of foreground pixels, as ``label_images(frames > low)`` finds them.  A component is KEPT when it holds a pixel ``> high`` (when
    ``high`` is given; one below ``low`` filters nothing), ``min_area <= area <= max_area`` (no upper limit by default), and - with
    ``clear_border`` - none of its pixels lies in row 0, row ``rows - 1``, column 0 or column ``w - 1``.  Kept components are numbered
    1, 2, ... per frame in the raster order of their first pixel; everything else is 0, so ``labels`` is ``label_images(kept mask)[0]``.
    ``area`` and ``first`` - the raster index ``y * w + x`` of the first pixel - hold one entry per component, entry 0 the background's
    (0, -1); ``counts[i]`` = kept components of frame i + 1, and a table with fewer entries than that holds the first ``table_entries``
    (default: 1 024, or h*w + 1 if that is less).  ``low`` and ``high`` are an int, a float or an (h, w) array or tensor; a float t stands
    for floor(t), and thresholds are held as int32 in [-1, 65535].  ``ValueError`` on bad parameters, before any device work."""
    shape = tuple(frames.shape)
    n, h, w, spec = _label_hot_spots_args(shape, low, high, min_area, max_area, clear_border, rows, table_entries)
    fr = _frames3(frames, torch.uint16)
    cap = spec.table_entries
    dst = torch.empty((n, h, w), dtype=torch.int32, device=fr.device)
    first = torch.zeros((n, cap), dtype=torch.int32, device=fr.device)
    area = torch.zeros((n, cap), dtype=torch.int32, device=fr.device)
    count = torch.zeros(n, dtype=torch.int32, device=fr.device)
    _label_hot_spots_into(fr, spec, dst, first, area, count)
    return dst, area, first, count


TRACK_MAX_INDEX = 0x7FFF0000  # pixels of a frame, and frames x nlabels, of one track_components call


class ComponentTracks(namedtuple("ComponentTracks", "tracks track_of ntracks truncated first_frame last_frame first_label components")):
    """The result of ``track_components``, CUDA tensors: ``tracks`` int32 (n, h, w), the track of every pixel (0: background), or None;
    ``track_of`` int32 (n, nlabels), the track of each component (0 where it does not exist); ``ntracks`` (0-d) = tracks + 1 and
    ``truncated`` (0-d) = frames whose components >= nlabels were dropped; per track, ``table_entries`` entries each: ``first_frame``,
    ``last_frame``, ``first_label`` (the label of the track's lowest node, in frame first_frame) and ``components`` (its nodes).  Entry 0
    is the background's (-1, -1, 0, 0); entries from ntracks on are 0."""

    __slots__ = ()


def _track_args(labels_shape, counts_shape, nlabels, table_entries):
    """the shapes and ranges of a track_components call, checked without a device; -> (n, h, w).  nlabels / table_entries None: left to the caller"""
    if len(labels_shape) != 3:
        raise ValueError("track_components: labels (n, h, w) expected")
    n, h, w = labels_shape
    if h < 1 or w < 1 or h * w > TRACK_MAX_INDEX:
        raise ValueError("track_components: frames of at least 1x1 and at most 0x7FFF0000 pixels expected")
    if counts_shape is not None and tuple(counts_shape) != (n,):
        raise ValueError("track_components: counts of shape %s expected, not %s" % ((n,), tuple(counts_shape)))
    if nlabels is not None and (int(nlabels) != nlabels or nlabels < 1 or n * nlabels > TRACK_MAX_INDEX):
        raise ValueError("track_components: nlabels must be at least 1 with n * nlabels <= 0x7FFF0000 (got %r)" % (nlabels,))
    if table_entries is not None and (int(table_entries) != table_entries or not 1 <= table_entries <= 0x7FFFFFFF):
        raise ValueError("track_components: table_entries must be in 1..2^31 - 1 (got %r)" % (table_entries,))
    return n, h, w


def _track_inputs(labels, counts, nlabels, table_entries, relabel, out):
    """track_components' checks, those that need no device first; -> (n, h, w)"""
    if labels.dtype != torch.int32:
        raise RuntimeError("track_components: int32 labels expected, not %s" % labels.dtype)
    if counts is not None and counts.dtype != torch.int32:
        raise RuntimeError("track_components: int32 counts expected, not %s" % counts.dtype)
    n, h, w = _track_args(tuple(labels.shape), None if counts is None else tuple(counts.shape), nlabels, table_entries)
    if out is not None:
        if not relabel:
            raise ValueError("track_components: 'out' given with relabel=False")
        if out.dtype != torch.int32 or tuple(out.shape) != (n, h, w) or not out.is_contiguous():
            raise RuntimeError("track_components: 'out' must be a C-contiguous int32 tensor of shape %s" % ((n, h, w),))
    if not labels.is_cuda or (counts is not None and counts.device != labels.device) or (out is not None and out.device != labels.device):
        raise RuntimeError("track_components: labels, counts and out on one CUDA device expected")
    return n, h, w


def track_components(labels, counts=None, nlabels=None, table_entries=None, relabel=True, out=None):
    """Tracks of the components of a stack of per-frame label maps ``labels`` int32 (n, h, w), as ``label_images`` writes them, on the
    current stream (C ABI ``rir_track_components_device``): a ``ComponentTracks``.  Component k of frame t exists when
    1 <= k < min(nlabels, counts[t]) (``counts``: int32 (n,) as ``label_images`` returns it; without it 1 <= k < nlabels); components of
    adjacent frames that share a pixel are linked, a track is a connected set of components, and tracks are numbered 1, 2, ... in the
    order of their lowest (frame, label).  ``relabel``: also the track map ``tracks``, written into ``out`` when given - ``out=labels``
    relabels in place.  ``nlabels=None`` takes ``int(counts.max())`` (``labels.max() + 1`` without counts, at least 1), which synchronises;
    ``table_entries`` defaults to min(n * (nlabels - 1) + 1, 65 536).  ``region_stats(frames, tracks, int(ntracks))`` is then the time
    trace of every track: its ``count`` is the track's area in each frame."""
    n, h, w = _track_inputs(labels, counts, nlabels, table_entries, relabel, out)
    in_place = out is not None and out.data_ptr() == labels.data_ptr() and labels.is_contiguous()
    lab = labels.contiguous()
    cnt = None if counts is None else counts.contiguous()
    if nlabels is None:
        nlabels = max(1, (int(cnt.max()) if cnt is not None else int(lab.max()) + 1) if n else 1)
        _track_args(tuple(labels.shape), None, nlabels, None)
    K = int(nlabels)
    T = min(n * (K - 1) + 1, 65536) if table_entries is None else int(table_entries)
    dev = lab.device
    track_of = torch.empty((n, K), dtype=torch.int32, device=dev)
    info = torch.empty(2, dtype=torch.int32, device=dev)
    tables = [torch.empty(T, dtype=torch.int32, device=dev) for _ in range(4)]
    dst = None
    if relabel:
        dst = lab if in_place else out if out is not None else torch.empty((n, h, w), dtype=torch.int32, device=dev)
    need = _lib.rir_track_components_workspace_bytes(w, h, n, K)
    if need == 0:
        raise RuntimeError("track_components: geometry refused")
    work = _workspace(need, dev)
    _check(_lib.rir_track_components_device(lab.data_ptr(), None if cnt is None else cnt.data_ptr(), w, h, n, K, track_of.data_ptr(), info.data_ptr(),
                                            *(t.data_ptr() for t in tables), T, None if dst is None else dst.data_ptr(), work.data_ptr(),
                                            work.numel() * 8, _stream()), "rir_track_components_device")
    return ComponentTracks(out if in_place else dst, track_of, info[0], info[1], *tables)


def keep_largest_areas(frames, background=0, foreground=1):
    """``foreground`` on the largest component of every image of a batch (n, h, w), int(background) elsewhere; int32 (n, h, w) on the device."""
    fr, ch, n, h, w, work, back = _label_batch_args(frames, background)
    dst = torch.empty((n, h, w), dtype=torch.int32, device=fr.device)
    _check(_lib.rir_keep_largest_areas_device(ord(ch), fr.data_ptr(), dst.data_ptr(), w, h, n, back.ctypes.data, int(foreground), work.data_ptr(),
                                              work.numel() * 8, _stream()), "rir_keep_largest_areas_device")
    return dst


def split_planes(frames, linesize=None, it=None):
    """uint16 frames -> (Y, U, V) byte planes [n][h][linesize] (reference h264.cpp:1066-1082)."""
    fr = _frames3(frames, torch.uint16)
    n, h, w = fr.shape
    ls = w if linesize is None else int(linesize)
    Y, U, V = (torch.zeros((n, h, ls), dtype=torch.uint8, device=fr.device) for _ in range(3))
    itp = None
    if it is not None:
        it = _frames3(it, torch.uint8)
        itp = it.data_ptr()
    _check(_lib.rir_split_planes_device(fr.data_ptr(), itp, w, h, n, ls, Y.data_ptr(), U.data_ptr(), V.data_ptr(), _stream()), "rir_split_planes_device")
    return Y, U, V


def merge_planes(Y, U, V, width, with_it=False):
    """(Y, U, V) byte planes -> uint16 frames (and the 8-bit image carried by Y) (reference h264.cpp:3016-3051)."""
    U = _frames3(U, torch.uint8)
    V = _frames3(V, torch.uint8)
    n, h, ls = U.shape
    img = torch.empty((n, h, width), dtype=torch.uint16, device=U.device)
    it = torch.empty((n, h, width), dtype=torch.uint8, device=U.device) if with_it else None
    Yp = _frames3(Y, torch.uint8).data_ptr() if Y is not None else None
    _check(_lib.rir_merge_planes_device(Yp, U.data_ptr(), V.data_ptr(), ls, width, h, n, img.data_ptr(), it.data_ptr() if with_it else None,
                                        _stream()), "rir_merge_planes_device")
    return (img, it) if with_it else img


class LossyStream:
    """Bounded-loss step on device-resident frames (reference H264_Saver::addImageLossyNoCamera / addLoss)."""

    def __init__(self, width, height, lossy_height=None, low_value_error=6, high_value_error=2, std_factor=5.0, running_average=32,
                 subtract_min=False, remove_bad_pixels=False):
        self.shape = (height, width)
        self.handle = _lib.rir_lossy_create(width, height, height if lossy_height is None else int(lossy_height), int(low_value_error),
                                            int(high_value_error), float(std_factor), int(running_average), int(bool(subtract_min)),
                                            int(bool(remove_bad_pixels)))
        if self.handle <= 0:
            raise RuntimeError("rir_lossy_create failed: %s" % last_error())

    def step(self, frames, add_loss=False, errors=True):
        """frames (n,h,w) uint16 on the device -> (processed frames, low_errors, high_errors).  With ``errors=False`` the
        frames are only queued on the current stream (nothing waits) and the two error arrays are None."""
        fr = _frames3(frames, torch.uint16)
        n = fr.shape[0]
        if tuple(fr.shape[1:]) != self.shape:
            raise RuntimeError("LossyStream.step: wrong frame size")
        out = torch.empty_like(fr)
        lo = np.zeros(n, np.int32) if errors else None
        hi = np.zeros(n, np.int32) if errors else None
        _check(_lib.rir_lossy_step_device(self.handle, fr.data_ptr(), out.data_ptr(), n, int(bool(add_loss)),
                                          lo.ctypes.data if errors else None, hi.ctypes.data if errors else None, _stream()),
               "rir_lossy_step_device")
        return out, lo, hi

    @staticmethod
    def step_many(streams, frames, add_loss=False, errors=True):
        """The step for several independent streams in shared launches (rir_lossy_step_multi_device): ``streams`` are
        LossyStream objects of one geometry that have seen the same number of frames, ``frames`` one (n,h,w) uint16 device
        tensor per stream.  -> (list of processed tensors, low_errors[stream][frame], high_errors[stream][frame])."""
        S = len(streams)
        frs = [_frames3(f, torch.uint16) for f in frames]
        if S == 0 or len(frs) != S or any(tuple(f.shape) != tuple(frs[0].shape) for f in frs) or tuple(frs[0].shape[1:]) != streams[0].shape:
            raise RuntimeError("LossyStream.step_many: one tensor of the streams' frame size per stream expected")
        n = frs[0].shape[0]
        outs = [torch.empty_like(f) for f in frs]
        handles = (ct.c_int * S)(*[s.handle for s in streams])
        pin = (ct.c_void_p * S)(*[f.data_ptr() for f in frs])
        pout = (ct.c_void_p * S)(*[o.data_ptr() for o in outs])
        lo = np.zeros((S, n), np.int32) if errors else None
        hi = np.zeros((S, n), np.int32) if errors else None
        _check(_lib.rir_lossy_step_multi_device(ct.cast(handles, _vp), S, ct.cast(pin, _vp), ct.cast(pout, _vp), n, int(bool(add_loss)),
                                                lo.ctypes.data if errors else None, hi.ctypes.data if errors else None, _stream()),
               "rir_lossy_step_multi_device")
        return outs, lo, hi

    def set_errors(self, low_value_error, high_value_error, std_factor):
        """lowValueError / highValueError / stdFactor from the next frame on (the budget's history stays)"""
        _check(_lib.rir_lossy_set_errors(self.handle, int(low_value_error), int(high_value_error), float(std_factor)), "rir_lossy_set_errors")

    def path_stats(self):
        """(groups of frames of the last batch this stream led that were offered to the constant-budget form, groups it took); waits"""
        out = (ct.c_int * 2)()
        _check(_lib.rir_lossy_path_stats(self.handle, out, _stream()), "rir_lossy_path_stats")
        return int(out[0]), int(out[1])

    def spec_stats(self):
        """the speculative form's books for the last batch this stream led: (groups through its launches, groups offered, groups committed,
        passes over all groups); waits"""
        out = (ct.c_int * 4)()
        _check(_lib.rir_lossy_spec_stats(self.handle, out, _stream()), "rir_lossy_spec_stats")
        return int(out[0]), int(out[1]), int(out[2]), int(out[3])

    def status(self):
        """raises when a queue-only ``step`` / ``step_many`` led by this stream went wrong on the device (waits for the stream)"""
        _check(_lib.rir_lossy_status(self.handle, _stream()), "rir_lossy_status")

    def close(self):
        if getattr(self, "handle", 0) > 0:
            _lib.rir_lossy_destroy(self.handle)
            self.handle = 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


Downsampled = namedtuple("Downsampled", "frames timestamps positions stats")


def _downsample_args(width, height, factor, factor_std, lossy_height, method):
    """the checks of ``Downsampler`` that need no device; -> (width, height, lossy_height, factor, factor_std, method)"""
    width, height, factor, method = int(width), int(height), int(factor), int(method)
    lossy_height = height if lossy_height is None else int(lossy_height)
    factor_std = float(factor_std)
    if width < 1 or height < 1 or width * height > 2147483647:
        raise ValueError("Downsampler: width, height >= 1 with width * height < 2^31 expected")
    if not 1 <= lossy_height <= height:
        raise ValueError("Downsampler: lossy_height in 1..height expected, not %d" % lossy_height)
    if width * lossy_height < 2:
        raise ValueError("Downsampler: width * lossy_height >= 2 expected")
    if factor < 1:
        raise ValueError("Downsampler: factor >= 1 expected, not %d" % factor)
    if not 0.0 <= factor_std <= 1.0:
        raise ValueError("Downsampler: factor_std in [0, 1] expected, not %r" % factor_std)
    if method not in (1, 2):
        raise ValueError("Downsampler: method 1 or 2 expected, not %d" % method)
    return width, height, lossy_height, factor, factor_std, method


def _downsample_stamps(timestamps, n, last):
    """the time stamps of a push as int64 [n], strictly increasing from ``last`` (or None) on"""
    ts = np.ascontiguousarray(np.asarray(timestamps).reshape(-1), dtype=np.int64)
    if ts.size != n:
        raise ValueError("Downsampler.push: %d time stamps for %d frames" % (ts.size, n))
    if (n > 1 and not (ts[1:] > ts[:-1]).all()) or (n and last is not None and ts[0] <= last):
        raise ValueError("Downsampler.push: the time stamps must increase strictly, from the last one pushed on")
    return ts


class Downsampler:
    """Adaptive temporal downsampling with max-hold of device-resident frames (reference ``VideoDownsampler``, C ABI
    ``rir_downsampler_*``): about one image in ``factor`` is kept, more while the scene changes (``factor_std`` in [0, 1]: the quantile of
    the recent frame-to-frame statistics an image must exceed; ``method`` 1 = ``addImage``, 2 = ``addImage2``), and every kept image is
    the per-pixel maximum of the images since the last kept one over the first ``lossy_height`` rows."""

    def __init__(self, width, height, factor, factor_std, lossy_height=None, method=1):
        self.handle = 0
        width, height, lossy_height, factor, factor_std, method = _downsample_args(width, height, factor, factor_std, lossy_height, method)
        self.shape = (height, width)
        self.lossy_height, self.factor, self.factor_std, self.method = lossy_height, factor, factor_std, method
        self._last = None
        self.handle = _lib.rir_downsampler_create(width, height, lossy_height, factor, factor_std, method)
        if self.handle <= 0:
            raise RuntimeError("rir_downsampler_create failed: %s" % last_error())

    def push(self, frames, timestamps, out=None):
        """The next images of the stream: ``frames`` (n, h, w) uint16 on the device, ``timestamps`` n strictly increasing integers ->
        ``Downsampled(frames, timestamps, positions, stats)``: the kept images (a CUDA tensor [kept][h][w], a view of ``out`` - capacity n
        images, not overlapping ``frames`` - when given), their time stamps, the index within this push of the image that triggered
        each, and the statistic of every pushed image (numpy).  Waits once for the current stream; the kept images are queued on it."""
        if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint16:
            raise RuntimeError("Downsampler.push: a uint16 tensor expected")
        if frames.dim() != 3 or tuple(frames.shape[1:]) != self.shape:
            raise RuntimeError("Downsampler.push: frames of shape (n, %d, %d) expected" % self.shape)
        n = frames.shape[0]
        ts = _downsample_stamps(timestamps, n, self._last)
        fr = _frames3(frames, torch.uint16)
        if out is None:
            out = torch.empty_like(fr)
        elif not out.is_cuda or out.dtype != torch.uint16 or tuple(out.shape) != tuple(fr.shape) or not out.is_contiguous():
            raise RuntimeError("Downsampler.push: 'out' must be a C-contiguous CUDA uint16 tensor of the frames' shape")
        positions = np.zeros(n, np.int32)
        stats = np.zeros(n, np.float64)
        kept = _lib.rir_downsampler_push_device(self.handle, fr.data_ptr(), n, ts.ctypes.data, out.data_ptr(), positions.ctypes.data,
                                                stats.ctypes.data, _stream()) if n else 0
        if kept < 0:
            raise RuntimeError("rir_downsampler_push_device failed: %s" % last_error())
        if n:
            self._last = int(ts[-1])
        positions = positions[:kept].copy()
        return Downsampled(out[:kept], ts[positions], positions, stats)

    @property
    def count(self):
        """images kept so far"""
        return int(_lib.rir_downsampler_count(self.handle)) if self.handle > 0 else 0

    def close(self):
        """-> the images kept over the stream's life, as the reference's ``close()``"""
        kept = self.count
        if getattr(self, "handle", 0) > 0:
            _lib.rir_downsampler_destroy(self.handle)
            self.handle = 0
        return kept

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def downsample(frames, timestamps, factor, factor_std, lossy_height=None, method=1, out=None):
    """One stack through a fresh ``Downsampler`` of its size -> ``Downsampled``."""
    if not isinstance(frames, torch.Tensor) or frames.dim() != 3:
        raise RuntimeError("downsample: a tensor of shape (n, h, w) expected")
    d = Downsampler(frames.shape[2], frames.shape[1], factor, factor_std, lossy_height, method)
    try:
        return d.push(frames, timestamps, out)
    finally:
        d.close()
