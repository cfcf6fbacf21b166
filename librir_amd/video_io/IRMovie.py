"""Reading side of the Python interface: ``IRMovie`` gives array-like access to the images of a recording.

Public interface (class methods ``from_filename`` / ``from_bytes`` / ``from_numpy_array``, indexing and slicing,
``data``, ``timestamps``, ``attributes``, ``frame_attributes``, ``bad_pixels_correction``, ``registration*``,
``to_h264`` ...) as the reference class ``librir.video_io.IRMovie`` (reference
src/python/librir/video_io/IRMovie.py:72-676) for the part the hot path needs; the implementation is this build's:
frames are decoded on the MI355X a chunk at a time, the read-back filters run there as well, and one image crosses
PCIe per ``load_pos``.  Only digital levels are offered (no calibration plugin is shipped).
"""
import math
import os
import tempfile
from pathlib import Path

import numpy as np

from ..low_level.misc import touch_ahead as _touch_ahead
from ..tools.FileAttributes import FileAttributes
from . import rir_video_io as _abi
from .rir_video_io import FileFormat
from .IRSaver import IRSaver

_TI_MASK, _TI_SHIFT = 0xE000, 13  # the three top bits of a digital level carry the integration-time index


class InvalidMovie(Exception):
    pass


class CalibrationNotFound(Exception):
    """a calibration asked for by name or number that the movie does not offer (reference IRMovie.py:52-53, :172-197)"""


def create_pcr_header(rows, columns, frequency=50, bits=16):
    """The 1024-byte header of a raw PCR file as 256 little-endian uint32 (layout: reference IRFileLoader.h:43-61;
    words 2/3 = X/Y, 5 = Bits, 7 = Frequency, 9 = bytes per image, 10/11 = grab size)."""
    words = np.zeros(256, dtype=np.uint32)
    for index, value in ((2, columns), (3, rows), (5, bits), (7, frequency), (9, rows * columns * 2), (10, columns), (11, rows)):
        words[index] = value
    return words


def _remove_quietly(path):
    try:
        if path and os.path.exists(str(path)):
            os.unlink(str(path))
    except OSError:
        pass


class IRMovie(object):
    _file_attributes = None  # second, independent object on the same file: global attributes can be rewritten through it

    # ---- construction ------------------------------------------------------------------------------------------------
    def __init__(self, handle):
        if _abi.get_image_count(handle) < 0:
            raise InvalidMovie("Invalid ir_movie descriptor")
        self.handle = handle
        self.times = None  # seconds, filled on the first load_secs
        self._calibration_index = 0
        self._seconds = None
        self._bp_on = False
        self._reg_file = None
        self._per_frame = {}  # position -> attributes of that image, as read
        self._current = -1
        self._shape = None  # (height, width), fetched once
        self._owned_file = None  # temporary file this object must delete on close

    @classmethod
    def _attach_attributes(cls, movie, opener, source, optional):
        try:
            fa = opener(source)
            fa.attributes = _abi.get_global_attributes(movie.handle)
            movie._file_attributes = fa
        except RuntimeError:
            if not optional:
                movie.close()
                raise
            movie._file_attributes = None  # a movie in memory may carry no trailer: read-only attributes then
        return movie

    @classmethod
    def from_filename(cls, filename):
        return cls._attach_attributes(cls(_abi.open_camera_file(str(filename))), FileAttributes.from_filename, filename, False)

    @classmethod
    def from_bytes(cls, data):
        return cls._attach_attributes(cls(_abi.open_camera_memory(data)), FileAttributes.from_buffer, data, True)

    @classmethod
    def from_numpy_array(cls, arr, attrs=None, times=None, cthreads=8):
        """The array goes through the codec and the encoded (temporary) file is what the returned movie reads, like the reference
        (IRMovie.py:108-144).  The reference gets there through a raw PCR file that it writes and re-encodes with ``to_h264``; here the
        images are recorded straight from the array - the same file (50 images a second when ``times`` is not given, as a PCR header
        says; no attributes; ``to_h264``'s saver parameters) without writing, reading and copying the movie twice more (1 000 images
        640x512: 310-470 ms that way, of which 30 are the recording)."""
        frames = np.asarray(arr)
        if frames.ndim not in (2, 3):
            raise ValueError("mismatch array shape. Must be 2D or 3D")
        rows, columns = frames.shape[-2:]
        stack = np.ascontiguousarray(frames, dtype=np.uint16).reshape(-1, rows, columns)
        if stack.shape[0] == 0:
            raise RuntimeError("No images in selected range to save")
        handle, name = tempfile.mkstemp(suffix=".h264")
        os.close(handle)
        encoded = Path(name)
        try:
            if times is None:  # what a raw file's time stamps come to on their way through ``to_h264`` (seconds, then nanoseconds again)
                times = [t * 1e9 for t in (np.arange(stack.shape[0], dtype=np.int64) * (1000000000 // 50)) * 1e-9]
            with IRSaver(str(encoded), columns, rows, rows, 8) as saver:
                saver.set_global_attributes({})
                saver.set_parameter("threads", cthreads)
                saver.set_parameter("codec", "h264")
                for pos in range(stack.shape[0]):
                    saver.add_image(stack[pos], times[pos], attributes={})
            movie = cls.from_filename(encoded)
        except BaseException:
            encoded.unlink(missing_ok=True)
            raise
        movie._owned_file = encoded
        if attrs is not None:
            movie.attributes = attrs
            movie._file_attributes.flush()
        return movie

    # ---- life cycle ----------------------------------------------------------------------------------------------------
    def close(self):
        fa, self._file_attributes = self._file_attributes, None
        if fa is not None:
            try:
                fa.close()
            except Exception:
                pass
        handle, self.handle = getattr(self, "handle", 0), 0
        if handle > 0:
            _abi.close_camera(handle)
        owned, self._owned_file = getattr(self, "_owned_file", None), None
        _remove_quietly(owned)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __repr__(self):
        return "IRMovie({})".format(self.filename)

    # ---- calibration: digital levels only --------------------------------------------------------------------------------
    @property
    def calibrations(self):
        return _abi.supported_calibrations(self.handle)

    def _calibration_number(self, which):
        if which == 0:  # digital levels: always there, always first (the per-image path asks for nothing else)
            return 0
        names = self.calibrations
        if isinstance(which, str):
            if which in ("DL", "Digital Level"):
                return 0
            if which not in names:
                raise CalibrationNotFound("%s not in available calibrations : %s" % (which, names + ["DL"]))
            return names.index(which)
        number = int(which)
        if not 0 <= number < len(names):
            raise CalibrationNotFound("Available calibrations : %s. Calibration index out of range : %s" % (names, number))
        return number

    # short names of the calibrations, in the library's order (reference IRMovie.py:77, :169-170: "DL" for "Digital Level")
    _calibration_nickname_mapper = {"DL": "Digital Level"}

    @property
    def calibration(self):
        """the current calibration by its SHORT name where it has one ("DL"), as upstream answers"""
        short = list(self._calibration_nickname_mapper)
        return short[self._calibration_index] if self._calibration_index < len(short) else self.calibrations[self._calibration_index]

    @calibration.setter
    def calibration(self, value):
        self._calibration_index = self._calibration_number(value)

    def flip_calibration(self, flip_rl, flip_ud):
        _abi.flip_camera_calibration(self.handle, flip_rl, flip_ud)

    @property
    def support_emissivity(self):
        return _abi.support_emissivity(self.handle)

    # (reference IRMovie.py:401-423: a movie whose calibration takes no emissivity reads as 1 everywhere and refuses to be set)
    @property
    def global_emissivity(self):
        return _abi.get_global_emissivity(self.handle) if self.support_emissivity else 1.0

    @global_emissivity.setter
    def global_emissivity(self, value):
        if not self.support_emissivity:
            raise RuntimeError("Cannot set custom emissivity value for this handle")
        _abi.set_global_emissivity(self.handle, value)

    @property
    def emissivity(self):
        return _abi.get_emissivity(self.handle) if self.support_emissivity else np.ones(self.image_size, dtype=np.float32)

    @emissivity.setter
    def emissivity(self, emissivity_array):
        if not self.support_emissivity:
            raise RuntimeError("Cannot set custom emissivity value for this handle")
        _abi.set_emissivity(self.handle, emissivity_array)

    def calibrate(self, image, calib):
        """``calib`` applied to a digital-level image, as a new array (IRMovie.py:510-514); only calibration 0 exists here."""
        return _abi.calibrate_image(self.handle, image, calib)

    @property
    def calibration_files(self):
        try:
            return _abi.calibration_files(self.handle)
        except RuntimeError:
            return []

    # ---- geometry ----------------------------------------------------------------------------------------------------------
    @property
    def images(self):
        return _abi.get_image_count(self.handle)

    def __len__(self):
        return self.images

    @property
    def image_size(self):
        return _abi.get_image_size(self.handle)

    height = property(lambda self: self.image_size[0])
    width = property(lambda self: self.image_size[1])

    @property
    def filename(self):
        """a ``Path`` (None for a movie without a file), like upstream (IRMovie.py:341-344)"""
        name = _abi.get_filename(self.handle)
        return Path(name) if name else None

    @property
    def video_file_format(self):
        return _abi.video_file_format(self.filename)

    @property
    def is_file_uncompressed(self):
        return self.video_file_format in (FileFormat.PCR, FileFormat.WEST, FileFormat.PCR_ENCAPSULATED)

    # ---- images --------------------------------------------------------------------------------------------------------------
    def load_pos(self, pos, calibration=None, out=None):
        """Image number ``pos`` (bad-pixel repair and motion correction applied when enabled).  ``out``: a C-contiguous uint16 array of
        the image's shape to read into (not part of the reference's signature; slices use it to fill their stack in place)."""
        pos = int(pos)
        if self._shape is None:
            self._shape = _abi.get_image_size(self.handle)
        image = _abi.load_image(self.handle, pos, self._calibration_number(0 if calibration is None else calibration), self._shape, out)
        self._per_frame[pos] = _abi.get_attributes(self.handle)
        self._current = pos
        return image

    def _window(self, window, what):
        """``window`` as four Python ints ``(y0, x0, h, w)``, checked against the image size"""
        if not isinstance(window, (tuple, list)) or len(window) != 4 or not all(type(v) is int for v in window):
            raise ValueError("%s: window=(y0, x0, h, w), four ints, expected, not %r" % (what, window))
        y0, x0, h, w = window
        H, W = self.image_size
        if h < 1 or w < 1 or y0 < 0 or x0 < 0 or y0 + h > H or x0 + w > W:
            raise ValueError("%s: window %r is empty or not inside the %d x %d image" % (what, tuple(window), H, W))
        return y0, x0, h, w

    def _load_device(self, first, count, step, out, window):
        if window is None:
            _abi.load_images_device(self.handle, first, count, step, out)
        else:
            _abi.load_window_device(self.handle, first, count, step, window, out)

    def to_tensor(self, selection=slice(None), dtype=None, out=None, temporal_median=None, median_threshold=0, window=None):
        """Images of ``selection`` (an int, or a slice with a positive step; negative bounds as ``movie[...]`` takes them) as a CUDA
        tensor ``[n][h][w]`` of ``dtype`` (``torch.uint16``, the default, or ``torch.float32``) on the current CUDA device - the images
        ``movie[selection]`` gives, bit for bit, decoded on the device: only the compressed chunks of a recording of this library cross
        the link.  ``out``: a preallocated C-contiguous CUDA tensor of that shape and dtype.  The current image (``load_pos``) and its
        attributes stay what they were.

        ``window=(y0, x0, h, w)`` (Python ints, inside the image): the result is ``[n][h][w]``, bit for bit
        ``to_tensor(...)[:, y0:y0+h, x0:x0+w]``.  With no read-back filter on, only the 512-pixel tiles of a recording of this library
        that the window's rows lie in are read, sent and decoded; with one, the images are made whole on the device and cut there.

        ``temporal_median=W`` (odd, 1..63): each selected image p becomes the temporal median of the images p - W//2 .. p + W//2 of the
        recording as ``movie[...]`` gives them (read-back filters applied first; the window is truncated only at the recording's first and
        last image), taken where it differs from image p by more than ``median_threshold`` - ``librir_amd.device.temporal_median``.  The
        recording is read in pieces with W//2 images of halo on either side: the temporary device memory holds at most
        max(64 MiB, W images) of uint16 input, plus as many uint16 output images for a float32 result, whatever the selection's length
        (with a window the pieces are read through it and counted in window bytes)."""
        if window is not None:  # (before anything touches the device)
            window = self._window(window, "to_tensor")
        import torch

        dtype = torch.uint16 if dtype is None else dtype
        if temporal_median is not None:
            from ..device import _temporal_median_args

            h, w = self.image_size
            _temporal_median_args((1, h, w), temporal_median, median_threshold, None)
        if dtype not in (torch.uint16, torch.float32):
            raise ValueError("to_tensor: dtype torch.uint16 or torch.float32 expected, not %s" % (dtype,))
        if self._calibration_index != 0:
            raise ValueError("to_tensor: only digital levels (DL) are read to the device")
        positions = self._stats_positions(selection, "to_tensor")
        h, w = self.image_size if window is None else window[2:]
        shape = (len(positions), h, w)
        out = self._result(out, shape, dtype, "to_tensor: 'out' must be a C-contiguous CUDA tensor of shape %s and dtype %s", shape, dtype)
        if len(positions):
            total = self.images
            if positions.start < 0 or positions[-1] >= total:
                raise IndexError("to_tensor: images %s out of range (%d images)" % (positions, total))
            if temporal_median is None:
                self._load_device(positions.start, len(positions), positions.step, out, window)
            else:
                self._median_to_tensor(positions, int(temporal_median), int(median_threshold), out, window)
        return out

    _MEDIAN_PIECE_BYTES = 64 << 20  # uint16 input images read at once by to_tensor(temporal_median=...)

    def _median_to_tensor(self, positions, window, threshold, out, crop=None):
        import torch

        from ..device import temporal_median

        r, total, step = window // 2, self.images, positions.step
        h, w = self.image_size if crop is None else crop[2:]
        budget = max(window, self._MEDIAN_PIECE_BYTES // (2 * h * w))  # input images per piece
        per_piece = max(1, (budget - 2 * r - 1) // step + 1)  # outputs per piece: their images, halo included, fit the budget
        for k0 in range(0, len(positions), per_piece):
            sel = positions[k0:k0 + per_piece]
            lo, hi = max(0, sel[0] - r), min(total, sel[-1] + r + 1)
            stack = torch.empty((hi - lo, h, w), dtype=torch.uint16, device=out.device)
            self._load_device(lo, hi - lo, 1, stack, crop)
            dst = out[k0:k0 + len(sel)]
            if out.dtype == torch.uint16:
                temporal_median(stack, window, threshold, first=sel[0] - lo, count=len(sel), step=step, out=dst)
            else:
                dst.copy_(temporal_median(stack, window, threshold, first=sel[0] - lo, count=len(sel), step=step))

    _STATS_PIECE_BYTES = 64 << 20  # images (and what their caller keeps beside each) that one piece of _pieces holds

    def region_stats(self, labels, selection=slice(None), nregions=None):
        """Statistics of the images of ``selection`` (as ``to_tensor`` takes it) over the regions of one int32 label map ``labels`` (h, w),
        numpy or CUDA, uploaded once - ``librir_amd.device.region_stats`` over the images ``movie[selection]`` gives (read-back filters
        applied): a ``RegionStats`` of CUDA tensors ``[len(selection)][nregions]``.  ``nregions=None`` takes labels.max() + 1.  The
        recording is read in pieces of at most ``_STATS_PIECE_BYTES`` of images, so the device memory used does not grow with the selection."""
        return self.region_stats_window(labels, None, selection, nregions)

    def region_stats_window(self, labels, window, selection=slice(None), nregions=None):
        """``region_stats`` of the window ``(y0, x0, h, w)`` of the images, read through it (``to_tensor(window=...)``): ``labels`` is the
        (h, w) of the window, the result that of ``librir_amd.device.region_stats`` on ``to_tensor(selection)[:, y0:y0+h, x0:x0+w]``, the
        pieces are counted in window bytes.  ``window=None``: the whole image."""
        if window is not None:
            window = self._window(window, "region_stats")
        from ..device import _region_inputs, _region_stats_empty, _region_stats_into

        return self._region_reduce("region_stats", labels, nregions, selection, lambda probe, lab, k: _region_inputs(probe, lab, k)[1:2],
                                   _region_stats_empty, lambda fr, lab, k, out: _region_stats_into(fr, lab, 0, k, out), window, two_d=False)

    def _pieces(self, positions, device, window=None, bytes_per_pixel=2):
        """The walk of every analysis over a recording: the images at ``positions`` (a range) read in pieces of at most
        ``_STATS_PIECE_BYTES`` - read when the walk starts; ``bytes_per_pixel`` is what an image costs its caller, 2 for the image alone -
        through ``window`` if given, whose bytes are then the ones counted.  Yields ``(k0, k1, frames)``: ``frames`` holds the images
        ``positions[k0:k1]``, uint16 ``[k1 - k0][h][w]``, and is a view of ONE buffer on ``device`` that the next piece overwrites."""
        import torch

        h, w = self.image_size if window is None else window[2:]
        per_piece = self._piece_images(len(positions), h, w, bytes_per_pixel)
        if not per_piece:  # (an empty selection: nothing is read)
            return
        piece = torch.empty((per_piece, h, w), dtype=torch.uint16, device=device)
        for k0 in range(0, len(positions), per_piece):
            sel = positions[k0:k0 + per_piece]
            fr = piece[:len(sel)]
            self.to_tensor(slice(sel.start, sel.stop, sel.step), out=fr, window=window)
            yield k0, k0 + len(sel), fr

    def _piece_images(self, n, h, w, bytes_per_pixel=2):
        """the images in a piece of ``_pieces`` over n images (h, w): what ``_STATS_PIECE_BYTES`` holds, one at least, n at most"""
        return min(n, max(1, self._STATS_PIECE_BYTES // (bytes_per_pixel * h * w)))

    @staticmethod
    def _rows(out, k0, k1):
        """rows k0 .. k1 of a namedtuple of tensors; what is no tensor (a histogram's lo and width) stays"""
        return type(out)(*(t if isinstance(t, int) else t[k0:k1] for t in out))

    @staticmethod
    def _result(out, shape, dtype, message, *args):
        """``out`` if it is a C-contiguous CUDA tensor of `shape` and `dtype` - ``RuntimeError(message % args)`` if not - or, for None, a new
        one on the current device"""
        import torch

        if out is None:
            return torch.empty(shape, dtype=dtype, device=torch.device("cuda", torch.cuda.current_device()))
        if not out.is_cuda or out.dtype != dtype or tuple(out.shape) != shape or not out.is_contiguous():
            raise RuntimeError(message % args)
        return out

    def _label_map(self, what, labels, nregions, inputs, h, w, two_d):
        """The label map of a region reducer on the device and ``nregions`` resolved.  ``labels`` is numpy (int32, uploaded to the current
        device), a CUDA tensor, or None where the caller's checks allow it; ``two_d``: one map (h, w), refused here under `what` otherwise.
        ``inputs(probe, labels, nregions)`` runs the caller's checks of ``librir_amd.device`` over `probe`, an empty stack of (h, w) images,
        and returns (the map as the kernels take it, whatever else the caller needs); it runs before ``nregions=None`` is resolved to
        labels.max() + 1 and, with that, again.  -> (what ``inputs`` returned, nregions, device)"""
        import torch

        if isinstance(labels, np.ndarray):
            if labels.dtype != np.int32:
                raise RuntimeError("%s: int32 labels expected, not %s" % (what, labels.dtype))
            labels = torch.from_numpy(np.ascontiguousarray(labels)).to(torch.device("cuda", torch.cuda.current_device()))
        if two_d and labels is not None and labels.dim() != 2:
            raise ValueError("%s: one label map (h, w) expected, not shape %s" % (what, tuple(labels.shape)))
        device = labels.device if labels is not None else torch.device("cuda", torch.cuda.current_device())
        probe = torch.empty((0, h, w), dtype=torch.uint16, device=device)
        checked = inputs(probe, labels, nregions)
        if nregions is None:
            nregions = max(1, int(checked[0].max()) + 1)
            inputs(probe, labels, nregions)
        return checked, int(nregions), device

    def _region_reduce(self, what, labels, nregions, selection, inputs, empty, into, window=None, two_d=True):
        """What the region_* methods share: the label map taken in (``_label_map`` with `what`, ``inputs`` and ``two_d``), the selection
        parsed, the result made - ``empty(len(selection), nregions, *more, device)``, `more` being what ``inputs`` returned after the map -
        and filled piece by piece by ``into(frames, map, nregions, rows of the result, *more)``."""
        h, w = self.image_size if window is None else window[2:]
        (lab, *more), nregions, device = self._label_map(what, labels, nregions, inputs, h, w, two_d)
        positions = self._stats_positions(selection, what)
        out = empty(len(positions), nregions, *more, device)
        for k0, k1, fr in self._pieces(positions, device, window):
            into(fr, lab, nregions, self._rows(out, k0, k1), *more)
        return out

    def region_geometry(self, labels, selection=slice(None), nregions=None):
        """Geometry of the regions of one int32 label map ``labels`` (h, w), numpy or CUDA, weighted by the images of ``selection`` - what
        ``librir_amd.device.region_geometry(labels, nregions, frames=movie[selection])`` gives (read-back filters applied): a
        ``RegionGeometry`` of CUDA tensors ``[len(selection)][nregions]`` leading; count, bbox and moments repeat for every image, the
        weighted sums follow the recording.  Labels, selection, ``nregions`` and the pieces the recording is read in are those of
        ``region_stats``."""
        from ..device import _region_geometry_empty, _region_geometry_inputs, _region_geometry_into

        return self._region_reduce("region_geometry", labels, nregions, selection, lambda probe, lab, k: _region_geometry_inputs(lab, probe, k)[:1],
                                   lambda n, k, device: _region_geometry_empty(n, k, True, device),
                                   lambda fr, lab, k, out: _region_geometry_into(lab, fr, len(fr), 0, k, out))

    def region_quantiles(self, labels, percents, selection=slice(None), nregions=None):
        """Quantiles of the images of ``selection`` over the regions of one int32 label map ``labels`` (h, w), numpy or CUDA, at
        ``percents`` (a float or 1..8 floats in [0, 1]) - what ``librir_amd.device.region_quantiles`` over the images ``movie[selection]``
        gives (read-back filters applied): a ``RegionQuantiles`` of CUDA tensors, count ``[len(selection)][nregions]`` and values
        ``[len(selection)][nregions][len(percents)]``.  Labels, selection, ``nregions`` and the pieces the recording is read in are those
        of ``region_stats``."""
        from ..device import (_region_inputs, _region_quantiles_args, _region_quantiles_empty, _region_quantiles_into,
                              _region_quantiles_percents)

        pc = _region_quantiles_percents(percents)
        return self._region_reduce("region_quantiles", labels, nregions, selection,
                                   lambda probe, lab, k: _region_inputs(probe, lab, k, "region_quantiles", _region_quantiles_args)[1:2],
                                   lambda n, k, device: _region_quantiles_empty(n, k, pc.size, device),
                                   lambda fr, lab, k, out: _region_quantiles_into(fr, lab, 0, k, pc, out), two_d=False)

    def region_histogram(self, labels, nbins, lo=0, width=1, selection=slice(None), nregions=None, rows=None):
        """Histograms of the images of ``selection`` over the regions of one int32 label map ``labels`` (h, w), numpy or CUDA (None: the
        whole image is region 0), ``nbins`` bins of ``width`` levels from ``lo`` over the first ``rows`` rows (None: all) - what
        ``librir_amd.device.region_histogram`` over the images ``movie[selection]`` gives (read-back filters applied): a
        ``RegionHistogram`` of CUDA tensors, count ``[len(selection)][nregions]``, hist ``[..][nbins]`` and outside ``[..][2]``.  Labels,
        selection, ``nregions`` and the pieces the recording is read in are those of ``region_stats``."""
        from ..device import _region_histogram_empty, _region_histogram_inputs, _region_histogram_into

        what = "region_histogram" if labels is not None else "histogram"

        def inputs(probe, lab, k):  # -> (the map, nbins, lo, width, rows), the four as the checks leave them
            checked = _region_histogram_inputs(probe, lab, nbins, lo, width, k, rows, what)
            return checked[1:2] + checked[6:]

        return self._region_reduce(what, labels, 1 if labels is None else nregions, selection, inputs,
                                   lambda n, k, nbins, lo, width, rows, device: _region_histogram_empty(n, k, nbins, lo, width, device),
                                   lambda fr, lab, k, out, nbins, lo, width, rows: _region_histogram_into(fr, lab, 0, k, rows, out))

    def histogram(self, nbins, lo=0, width=1, selection=slice(None), rows=None):
        """``region_histogram`` without a map: the whole image (its first ``rows`` rows) is region 0 - what
        ``librir_amd.device.histogram`` over the images ``movie[selection]`` gives."""
        return self.region_histogram(None, nbins, lo, width, selection, 1, rows)

    def background_levels(self, selection=slice(None), rows=None):
        """The background level of every image of ``selection`` as the bounded-loss recorder defines it (reference ``get_background``,
        h264.cpp:1955-1990): of the 16 384 bins of v >> 2 the first of the fullest, as the level ``(bin << 2) + 1`` - an int32 CUDA tensor
        ``[len(selection)]``; -1 * 4 + 1 = -3 for an image without counted pixels (``rows`` 0)."""
        import torch

        return (self.histogram(16384, 0, 4, selection, rows).mode()[:, 0] * 4 + 1).to(torch.int32)

    def polygon_stats(self, polygons, selection=slice(None), shifts=None, values=None):
        """Statistics of the images of ``selection`` (as ``region_stats`` takes it) over polygon regions of interest
        (``librir_amd.device.polygon_map`` takes ``polygons`` and ``values`` the same way): a ``RegionStats`` of CUDA tensors
        ``[len(selection)][nregions]``, region r being the pixels painted with value r - ``nregions`` is the number of polygons, or
        ``max(values) + 1``.  Without ``shifts`` one map is drawn and ``region_stats`` runs over it.  With ``shifts`` of shape
        ``(len(selection), 2)``, e.g. a registration table, image k is measured with every polygon moved by ``+shifts[k]``: the maps of each
        piece of images are drawn beside it, pieces sized so that images and maps together stay within ``_STATS_PIECE_BYTES``."""
        import torch

        from ..device import _polygon_inputs, _polygon_map_args, _polygon_map_into, _region_stats_empty, _region_stats_into, polygon_map

        h, w = self.image_size
        positions = self._stats_positions(selection, "polygon_stats")
        n = len(positions)
        a = _polygon_map_args(polygons, (h, w), values, -1, shifts.detach().cpu().numpy() if isinstance(shifts, torch.Tensor) else shifts)
        if (a.per_map or a.shifts is not None) and a.nmaps != n:
            raise ValueError("polygon_stats: one shift or set of polygons per image of the selection expected (%d), not %d" % (n, a.nmaps))
        nregions = max(1, a.npoly if a.values is None else int(a.values.max(initial=-1)) + 1)
        if not a.per_map and a.shifts is None:
            return self.region_stats(polygon_map(polygons, (h, w), values), selection, nregions)
        device = a.xy.device if isinstance(a.xy, torch.Tensor) else torch.device("cuda", torch.cuda.current_device())
        xy, npts, vals, moves = _polygon_inputs(a, device)
        out = _region_stats_empty(n, nregions, device)
        maps = torch.empty((self._piece_images(n, h, w, 6), h, w), dtype=torch.int32, device=device)  # (6: an image and its int32 map)
        for k0, k1, fr in self._pieces(positions, device, bytes_per_pixel=6):
            _polygon_map_into(xy[k0:k1] if a.per_map else xy, npts[k0:k1] if a.per_map else npts, vals, None if moves is None else moves[k0:k1],
                              a.per_map, -1, maps[:k1 - k0])
            _region_stats_into(fr, maps[:k1 - k0], 1, nregions, self._rows(out, k0, k1))
        return out

    def pixel_stats(self, selection=slice(None), sums=True, extremes=True):
        """Statistics over time of the images of ``selection`` (as ``region_stats`` takes it) - ``librir_amd.device.pixel_stats`` over the
        images ``movie[selection]`` gives (read-back filters applied): a ``PixelStats`` of CUDA tensors ``[h][w]``, per pixel the exact sum
        and sum of squares (``sums``), the min, the max and where each first occurs (``extremes``).  ``argmin`` / ``argmax`` index into the
        selection: k means image ``movie[selection][k]``.  The recording is read in pieces of at most ``_STATS_PIECE_BYTES`` of images
        into one accumulator, so the device memory used does not grow with the selection."""
        return self.pixel_stats_window(None, selection, sums, extremes)

    def pixel_stats_window(self, window, selection=slice(None), sums=True, extremes=True):
        """``pixel_stats`` of the window ``(y0, x0, h, w)`` of the images, read through it (``to_tensor(window=...)``): tensors ``[h][w]`` of
        the window, the result that of ``librir_amd.device.pixel_stats`` on ``to_tensor(selection)[:, y0:y0+h, x0:x0+w]``, the pieces are
        counted in window bytes.  ``window=None``: the whole image."""
        if window is not None:
            window = self._window(window, "pixel_stats")
        import torch

        from ..device import PixelStatsAccumulator

        h, w = self.image_size if window is None else window[2:]
        positions = self._stats_positions(selection, "pixel_stats")
        device = torch.device("cuda", torch.cuda.current_device())
        acc = PixelStatsAccumulator(sums, extremes, shape=(h, w), device=device)
        for k0, _, fr in self._pieces(positions, device, window):
            acc.push(fr, k0)
        return acc.result()

    def morphology(self, op, size, selection=slice(None), rows=None, out=None):
        """Flat morphology of the images of ``selection`` (as ``region_stats`` takes it) - ``librir_amd.device.morphology(frames, op, size,
        rows)`` over the images ``to_tensor(selection)`` gives (read-back filters applied), filtered on the device: a uint16 CUDA tensor
        ``[len(selection)][h][w]`` (``out`` when given: a contiguous uint16 CUDA tensor of that shape).  ``op`` is "erode", "dilate",
        "open", "close", "tophat", "blackhat" or "gradient", ``size`` an odd int or ``(size_y, size_x)``, each 1..15; ``rows=None``
        filters all rows, otherwise rows ``>= rows`` are copied.  The recording is read in pieces of at most ``_STATS_PIECE_BYTES`` of
        images; images are filtered one by one, so any split gives the same bits.

        The other analysis calls take no morphology parameter; they compose with it::

            mask = mov.morphology("tophat", 9) > t                  # small hot spots on a spatially varying background
            mask = librir_amd.device.morph_open(mask, 3)            # drop single-pixel noise ...
            labels = librir_amd.device.label_images(mask)           # ... before labelling and track_components
        """
        from ..device import _morphology_args, morphology

        return self._window_filter("morphology", _morphology_args, morphology, op, size, selection, rows, out)

    def _window_filter(self, name, check, filter, own, size, selection, rows, out):
        """``morphology`` and ``rank_filter``: ``filter`` of ``librir_amd.device`` over the images of ``selection``, read in pieces, with the
        parameters that ``check`` passes; ``own`` is the op or the rank"""
        import torch

        h, w = self.image_size
        check((1, h, w), "uint16", own, size, rows)
        return self._filter_pieces(name, lambda fr, out: filter(fr, own, size, rows, out=out), torch.uint16, selection, out)

    def rank_filter(self, rank, size, selection=slice(None), rows=None, out=None):
        """Spatial rank filter of the images of ``selection`` (as ``region_stats`` takes it) - ``librir_amd.device.rank_filter(frames, rank,
        size, rows)`` over the images ``to_tensor(selection)`` gives (read-back filters applied), filtered on the device: a uint16 CUDA
        tensor ``[len(selection)][h][w]`` (``out`` when given: a contiguous uint16 CUDA tensor of that shape).  Every pixel becomes the
        element of 0-based rank ``rank`` (negative: from the end) of its full ``size`` window (an odd int or ``(size_y, size_x)``, each
        1..15), coordinates replicated at the border; ``rows=None`` filters all rows, otherwise rows ``>= rows`` are copied.  The recording
        is read in pieces of at most ``_STATS_PIECE_BYTES`` of images; images are filtered one by one, so any split gives the same bits::

            background = mov.rank_filter(librir_amd.device.percentile_rank(25, 9, 9), 9)   # a low percentile under sparse hot spots
        """
        from ..device import _rank_filter_args, rank_filter

        return self._window_filter("rank_filter", _rank_filter_args, rank_filter, rank, size, selection, rows, out)

    def window_median(self, size, selection=slice(None), rows=None, out=None):
        """``rank_filter`` at the median rank ``size_y * size_x // 2``: ``librir_amd.device.window_median`` over the images of
        ``selection`` - a despeckle at 3 or 5, a background estimate to subtract at 9 and more"""
        from ..device import _window_sizes

        size_y, size_x = _window_sizes(size)
        return self.rank_filter(size_y * size_x // 2, size, selection, rows, out)

    def h_dome(self, h, selection=slice(None), connectivity=8, rows=None, out=None):
        """The h-domes of the images of ``selection`` (as ``region_stats`` takes it) - ``librir_amd.device.h_dome(frames, h, connectivity,
        rows)`` over the images ``to_tensor(selection)`` gives (read-back filters applied), on the device: a uint16 CUDA tensor
        ``[len(selection)][h][w]`` (``out`` when given: a contiguous uint16 CUDA tensor of that shape) with what stands above its surround,
        ``h`` of it at most - ``image - R(image - h, image)``, R the reconstruction by dilation.  Unlike ``morphology("tophat", 9)`` it has
        no window: a strike line or a 40-pixel spot keeps its contrast.  ``connectivity`` is 8 or 4; ``rows=None`` takes all rows,
        otherwise rows ``>= rows`` are copied.  The recording is read in pieces of at most ``_STATS_PIECE_BYTES`` of images; images are
        independent, so any split gives the same bits::

            labels = librir_amd.device.label_hot_spots(mov.h_dome(40), low=10, min_area=4)   # hot spots of any size, 10 counts of contrast
        """
        return self._reconstruct_form("h_dome", h, selection, connectivity, rows, out)

    def h_maxima(self, h, selection=slice(None), connectivity=8, rows=None, out=None):
        """The h-maxima transform of the images of ``selection`` - ``librir_amd.device.h_maxima(frames, h, connectivity, rows)`` over the
        images ``to_tensor(selection)`` gives: every maximum cut down by ``h``, ``image - mov.h_dome(h)``; parameters and pieces as
        ``h_dome``"""
        return self._reconstruct_form("h_maxima", h, selection, connectivity, rows, out)

    def _reconstruct_form(self, name, h, selection, connectivity, rows, out):
        """``h_dome`` and ``h_maxima``: the form of that name of ``librir_amd.device`` over the images of ``selection``, read in pieces"""
        import torch

        from .. import device

        height, w = self.image_size
        device._reconstruct_args(name, (1, height, w), "uint16", "dilation", connectivity, rows, h)
        form = getattr(device, name)
        return self._filter_pieces(name, lambda fr, out: form(fr, h, connectivity, rows, out=out), torch.uint16, selection, out)

    def _filter_pieces(self, name, filter, dtype, selection, out):
        """what the window filters and the local statistics share: ``filter(piece, out=...)`` of ``librir_amd.device`` over the images of
        ``selection``, read in pieces, into a `dtype` tensor ``[len(selection)][h][w]``"""
        h, w = self.image_size
        positions = self._stats_positions(selection, name)
        shape = (len(positions), h, w)
        out = self._result(out, shape, dtype, "%s: 'out' must be a C-contiguous %s CUDA tensor of shape %s", name, str(dtype)[6:], shape)
        for k0, k1, fr in self._pieces(positions, out.device):
            filter(fr, out=out[k0:k1])
        return out

    def local_threshold(self, size, k, delta=0, polarity="above", selection=slice(None), rows=None, out=None):
        """The z-score mask of the images of ``selection`` (as ``region_stats`` takes it) - ``librir_amd.device.local_threshold(frames, size,
        k, delta, polarity, rows)`` over the images ``to_tensor(selection)`` gives (read-back filters applied), on the device: a bool CUDA
        tensor ``[len(selection)][h][w]`` (``out`` when given: a contiguous bool CUDA tensor of that shape), True where a pixel lies more
        than ``delta`` above the mean of its ``size`` window and more than ``k`` (an int or ``(num, den)``) local standard deviations off
        it.  The recording is read in pieces of at most ``_STATS_PIECE_BYTES`` of images; images are filtered one by one, so any split
        gives the same bits.  An adaptive threshold where ``morphology("tophat", 9) > t`` has one ``t`` for the whole image::

            labels = librir_amd.device.label_images(mov.local_threshold(9, 4, delta=20))   # hot spots 4 sigma and 20 counts above their surround
        """
        import torch

        from ..device import _local_stats_args, local_threshold

        h, w = self.image_size
        _local_stats_args("local_threshold", (1, h, w), "uint16", size, rows, k=k, delta=delta, polarity=polarity)
        return self._filter_pieces("local_threshold", lambda fr, out: local_threshold(fr, size, k, delta, polarity, rows, out=out), torch.bool, selection,
                                  out)

    def box_mean(self, size, selection=slice(None), rows=None, out=None):
        """The local mean of the images of ``selection`` - ``librir_amd.device.box_mean(frames, size, rows)`` over the images
        ``to_tensor(selection)`` gives: a uint16 CUDA tensor ``[len(selection)][h][w]`` (``out`` when given), every pixel the mean of its
        full ``size`` window rounded half up, coordinates replicated at the border; read in pieces as ``local_threshold``"""
        import torch

        from ..device import _local_stats_args, box_mean

        h, w = self.image_size
        _local_stats_args("box_mean", (1, h, w), "uint16", size, rows, outputs=(False, False, True))
        return self._filter_pieces("box_mean", lambda fr, out: box_mean(fr, size, rows, out=out), torch.uint16, selection, out)

    _QUANTILE_RESIDENT_BYTES = 1 << 30  # uint16 images that pixel_quantiles decodes into one stack

    def pixel_quantiles(self, percents, selection=slice(None)):
        """Quantiles over time of the images of ``selection`` (as ``region_stats`` takes it) at ``percents`` (a float or 1..8 floats in
        [0, 1]) - ``librir_amd.device.pixel_quantiles`` over the images ``movie[selection]`` gives (read-back filters applied): an int32
        CUDA tensor ``(len(percents), h, w)``; ``mov.pixel_quantiles(0.5)[0]`` is the median image, a background that hot spots do not
        pull up, and ``mov.pixel_quantiles(0.5)[0] + margin`` is a per-pixel threshold that ``track_hot_spots`` accepts.  A selection of at
        most ``_QUANTILE_RESIDENT_BYTES`` of images is decoded once into one stack; a longer one is read once per pass in pieces of at most
        ``_STATS_PIECE_BYTES`` into a ``PixelQuantileSelector``, so the device memory used does not grow with the selection.  The bits are
        the same either way."""
        import torch

        from ..device import PixelQuantileSelector, _region_quantiles_percents, pixel_quantiles

        h, w = self.image_size
        pc = _region_quantiles_percents(percents)
        positions = self._stats_positions(selection, "pixel_quantiles")
        n = len(positions)
        device = torch.device("cuda", torch.cuda.current_device())
        if 2 * h * w * n <= self._QUANTILE_RESIDENT_BYTES:
            stack = torch.empty((n, h, w), dtype=torch.uint16, device=device)
            if n:
                self.to_tensor(slice(positions.start, positions.stop, positions.step), out=stack)
            return pixel_quantiles(stack, pc)
        select = PixelQuantileSelector(pc, shape=(h, w), device=device)
        for _ in range(select.passes):
            for _, _, fr in self._pieces(positions, device):
                select.push(fr)
            select.next_pass()
        return select.result()

    def track_hot_spots(self, threshold, selection=slice(None), table_entries=None, stats=True):
        """The hot spots of the images of ``selection`` (as ``region_stats`` takes it) as tracks through time: every image ``movie[selection]``
        gives (read-back filters applied) is thresholded - ``image > threshold``, an int or an ``(h, w)`` array or tensor for a per-pixel
        threshold, e.g. from ``pixel_stats`` - and labelled (``librir_amd.device.label_images``), and the components of adjacent images of
        the selection that share a pixel are joined into tracks (``librir_amd.device.track_components``).  -> ``(ComponentTracks,
        RegionStats or None)``: the tracks, with ``tracks`` the int32 track map ``[len(selection)][h][w]``, and with ``stats`` the
        ``region_stats`` of every image over its track map, ``[len(selection)][ntracks]`` - the time trace of every hot spot (``count`` is
        its area in each image).  The recording is read in pieces of at most ``_STATS_PIECE_BYTES`` of images (twice with ``stats``), but
        the label stack of the whole selection stays on the device: 4 bytes a pixel and image.  ``track_hot_spots_geometry`` adds the
        box, centroid and extent of every hot spot; ``track_kept_hot_spots`` tracks only the components that pass a hysteresis, area or
        border filter."""
        return self._track_hot_spots(threshold, selection, table_entries, stats, False)

    def track_hot_spots_geometry(self, threshold, selection=slice(None), table_entries=None, stats=True):
        """``track_hot_spots`` with a third element: -> ``(ComponentTracks, RegionStats or None, RegionGeometry)``, the geometry of every image
        over its track map (``librir_amd.device.region_geometry``), ``[len(selection)][ntracks]`` leading and weighted by the images - the
        box, centroid and extent of every hot spot over time; its ``count`` is that of the statistics.  It is computed in the same second
        pass over the recording as the statistics (a pass of its own with ``stats=False``)."""
        return self._track_hot_spots(threshold, selection, table_entries, stats, True)

    def track_kept_hot_spots(self, threshold, selection=slice(None), table_entries=None, stats=True, geometry=False, high=None, min_area=1,
                             max_area=None, clear_border=False):
        """``track_hot_spots`` (``track_hot_spots_geometry`` with ``geometry=True``) over the components that are KEPT, as
        ``librir_amd.device.label_hot_spots`` chooses them with ``threshold`` as its ``low``: a component of ``image > threshold`` is kept
        when it holds a pixel ``> high`` (an int, a float or an ``(h, w)`` map; hysteresis - ``None``: not asked for),
        ``min_area <= area <= max_area`` (no upper limit by default), and - with ``clear_border`` - none of its pixels lies on the first
        or last row or column of the image.  Dropped components are background: they join no track and count in no statistic.
        ``threshold`` may also be a float, which stands for its floor.
        The images are labelled straight from their pixels, no mask is stored; with all four filters at their defaults every component
        is kept and the result is ``track_hot_spots``'.  ``ValueError`` on bad parameters, before the recording is read."""
        return self._track_hot_spots(threshold, selection, table_entries, stats, bool(geometry),
                                     dict(high=high, min_area=min_area, max_area=max_area, clear_border=clear_border))

    def _track_hot_spots(self, threshold, selection, table_entries, stats, geometry, filters=None):
        import torch

        from ..device import (_hot_spot_maps_on, _label_hot_spots_args, _label_hot_spots_into, _label_images_into, _region_geometry_empty,
                              _region_geometry_into, _region_stats_empty, _region_stats_into, _track_args, track_components)

        h, w = self.image_size
        positions = self._stats_positions(selection, "track_hot_spots")
        n = len(positions)
        _track_args((n, h, w), None, None, table_entries)
        filtered = filters is not None  # (track_kept_hot_spots: labelled by label_hot_spots, whatever the filters)
        if filtered:
            kept = _label_hot_spots_args((max(n, 1), h, w), threshold, rows=None, table_entries=1, **filters)[3]
        device = torch.device("cuda", torch.cuda.current_device())
        if filtered:
            kept = _hot_spot_maps_on(kept, device)
        else:
            cut = self._hot_cut(threshold, device, "track_hot_spots")
        stack = torch.empty((n, h, w), dtype=torch.int32, device=device)
        counts = torch.zeros(n, dtype=torch.int32, device=device)
        per_piece = self._piece_images(n, h, w)
        xy = torch.zeros((per_piece, 1, 2), dtype=torch.float64, device=device)
        area = torch.zeros((per_piece, 1), dtype=torch.int32, device=device)
        first = torch.zeros_like(area) if filtered else None
        for k0, k1, fr in self._pieces(positions, device):
            if filtered:
                _label_hot_spots_into(fr, kept, stack[k0:k1], first[:k1 - k0], area[:k1 - k0], counts[k0:k1])
                continue
            _label_images_into(self._hot_mask(fr, cut), 0, stack[k0:k1], xy[:k1 - k0], area[:k1 - k0], counts[k0:k1])
        nlabels = max(1, int(counts.max())) if n else 1
        tracks = track_components(stack, counts, nlabels, table_entries, out=stack)
        if not stats and not geometry:
            return tracks, None
        ntracks = int(tracks.ntracks)
        out = _region_stats_empty(n, ntracks, device) if stats else None
        geo = _region_geometry_empty(n, ntracks, True, device) if geometry else None
        for k0, k1, fr in self._pieces(positions, device):
            if stats:
                _region_stats_into(fr, stack[k0:k1], 1, ntracks, self._rows(out, k0, k1))
            if geometry:
                _region_geometry_into(stack[k0:k1], fr, k1 - k0, 1, ntracks, self._rows(geo, k0, k1))
        return (tracks, out, geo) if geometry else (tracks, out)

    @staticmethod
    def _hot_mask(fr, cut):
        """``fr > cut`` of uint16 images ``fr``, widened to int32 for the comparison, with the int or the map of ``_hot_cut``"""
        import torch

        return (fr.view(torch.int16).to(torch.int32) & 0xFFFF) > cut

    def _hot_cut(self, threshold, device, what):
        """the threshold of ``image > threshold`` as the hot-spot calls take it, an int or an (h, w) array or tensor: an int, or a map on `device`"""
        import torch

        if isinstance(threshold, (int, np.integer)):
            return int(threshold)
        h, w = self.image_size
        cut = threshold if isinstance(threshold, torch.Tensor) else np.asarray(threshold)
        if tuple(cut.shape) != (h, w):
            raise ValueError("%s: an int or an (h, w) threshold expected, not shape %s" % (what, tuple(cut.shape)))
        if isinstance(cut, np.ndarray):
            cut = torch.from_numpy(np.ascontiguousarray(cut, np.float64 if cut.dtype.kind == "f" else np.int64))
        cut = cut.to(device)
        if not cut.is_floating_point():
            cut = cut.to(torch.int32) if cut.dtype in (torch.uint16, torch.int16, torch.uint8, torch.int8) else cut
        return cut

    def distance_transform(self, threshold, selection=slice(None), invert=False, border=False, rows=None, return_indices=False):
        """Exact Euclidean distance transform of the hot-spot masks of the images of ``selection`` (as ``region_stats`` takes it) -
        ``librir_amd.device.distance_transform(to_tensor(selection) > threshold, ...)``, read-back filters applied, on the device: an int32
        CUDA tensor ``[len(selection)][h][w]`` with the SQUARED distance of every pixel to the nearest pixel that is not hot (0 outside
        the hot spots, ``librir_amd.device.DIST2_NONE`` in an image without such a pixel), or ``(dist2, index)`` with
        ``return_indices``, index the lowest flat index ``y * w + x`` of such a nearest pixel.  ``threshold`` is an int or an ``(h, w)``
        array or tensor, as in ``track_hot_spots``.  ``invert=True`` gives the distance TO the hot pixels instead: of every pixel to the
        nearest hot one, and which one that is.  ``border=True`` counts the outside of the image as a pixel to measure to; the image is
        its first ``rows`` rows (default: all), the others get 0.  The recording is read in pieces of at most ``_STATS_PIECE_BYTES`` of
        images; images are transformed one by one, so any split gives the same bits.

        Two idioms::

            # thickness per hot spot: the largest inscribed radius, the per-region maximum of dist2 under the label map
            dist2 = mov.distance_transform(t)
            labels = librir_amd.device.label_images(mov.to_tensor() > t)[0]
            regions = librir_amd.device.region_stats(dist2.clamp(max=65535).to(torch.uint16), labels)   # max: squared radius, up to 255 px
            radius = regions.max.double().sqrt()

            # merge the fragments of a spot before labelling: grow every hot spot by 3 px
            mask = librir_amd.device.disc_dilate(mov.to_tensor() > t, 3)
            labels = librir_amd.device.label_images(mask)[0]
        """
        import torch

        from ..device import _distance_transform_args, distance_transform

        h, w = self.image_size
        _distance_transform_args((1, h, w), "bool", 0, border, rows)
        positions = self._stats_positions(selection, "distance_transform")
        n = len(positions)
        device = torch.device("cuda", torch.cuda.current_device())
        cut = self._hot_cut(threshold, device, "distance_transform")
        dist2 = torch.empty((n, h, w), dtype=torch.int32, device=device)
        index = torch.empty((n, h, w), dtype=torch.int32, device=device) if return_indices else None
        for k0, k1, fr in self._pieces(positions, device):
            distance_transform(self._hot_mask(fr, cut), int(bool(invert)), border, rows, return_indices,
                               out=(dist2[k0:k1], index[k0:k1]) if return_indices else dist2[k0:k1])
        return (dist2, index) if return_indices else dist2

    def _stats_positions(self, selection, what):
        """the positions of an int or a slice with a positive step, as a range; `what` is the caller's name in the refusals"""
        total = self.images
        if isinstance(selection, (int, np.integer)):
            pos = int(selection) + (total if selection < 0 else 0)
            if not 0 <= pos < total:
                raise IndexError("image %d out of range (%d images)" % (int(selection), total))
            return range(pos, pos + 1)
        if isinstance(selection, slice):
            if selection.step is not None and selection.step <= 0:
                raise ValueError("%s: a slice with a positive step expected" % what)
            return self._positions(selection)[0]
        raise TypeError("%s: an int or a slice expected" % what)

    def load_secs(self, time, calibration=None):
        """The image whose time stamp is closest to ``time`` (seconds)."""
        if self.times is None:
            self.times = np.array(list(self.timestamps), dtype=np.float64)
        return self.load_pos(int(np.abs(self.times - time).argmin()), calibration)

    def _positions(self, selection):
        total = self.images
        first = selection.start or 0
        last = total if selection.stop is None or selection.stop == 0 else selection.stop
        stride = selection.step or 1
        first = first + total if first < 0 else first
        last = last + total if last < 0 else last
        return range(first, last, stride), math.ceil((last - first) / stride)

    def __getitem__(self, item):
        if isinstance(item, slice):
            positions, count = self._positions(item)
            stack = np.empty((count,) + tuple(self.image_size), dtype=np.uint16)
            if count:
                with _touch_ahead(stack):  # (the stack's pages are made by threads of their own while the images are read)
                    for row, pos in enumerate(positions):
                        self.load_pos(pos, self._calibration_index, out=stack[row])  # (in place: no copy of each image into the stack)
            return stack
        if isinstance(item, (int, np.integer)):
            return self.load_pos(int(item) + (self.images if item < 0 else 0), self._calibration_index)
        if isinstance(item, float):
            return self.load_secs(item, self._calibration_index)
        if isinstance(item, list) or (isinstance(item, np.ndarray) and item.ndim == 1):
            return np.array([self[e] for e in item])
        raise TypeError("unsupported index type")

    def __iter__(self):
        return (self.load_pos(pos, self._calibration_index) for pos in range(self.images))

    @property
    def data(self):
        return self[:]

    @property
    def tis(self):
        stack = self.data  # (a fresh array of this call: masked and shifted in place, no two further copies of the movie)
        stack &= _TI_MASK
        stack >>= _TI_SHIFT
        return stack

    # ---- time --------------------------------------------------------------------------------------------------------------------
    @property
    def timestamps(self):
        """seconds"""
        if self._seconds is None:
            self._seconds = np.fromiter((_abi.get_image_time(self.handle, pos) for pos in range(self.images)), dtype=np.float64) * 1e-9
        return self._seconds

    @timestamps.setter
    def timestamps(self, nanoseconds):
        self._seconds = np.array(nanoseconds) * 1e-9

    @property
    def frame_period(self):
        return np.diff(self.timestamps).mean().round(3)

    @property
    def duration(self):
        return (_abi.get_image_time(self.handle, self.images - 1) - _abi.get_image_time(self.handle, 0)) * 1e-9

    # ---- attributes -----------------------------------------------------------------------------------------------------------------
    @property
    def attributes(self):
        fa = self._file_attributes
        return _abi.get_global_attributes(self.handle) if fa is None else fa.attributes

    @attributes.setter
    def attributes(self, value):
        if self._file_attributes is not None:
            self._file_attributes.attributes = value

    @property
    def frame_attributes(self):
        """attributes of the image read last"""
        return self._per_frame.get(self._current, {})

    @property
    def frames_attributes(self):
        """The attributes of EVERY image as a table, one row per image (IRMovie.py:642-649: images not read yet are read for it).
        A pandas DataFrame like the reference's; values are the attribute bytes as stored."""
        import pandas as pd

        for pos in range(self.images):
            if pos not in self._per_frame:
                self.load_pos(pos, self._calibration_index)
        return pd.DataFrame({pos: self._per_frame[pos] for pos in range(self.images)}).T

    def _frame_attribute_getter(self, key):
        """one attribute of every image as floats (empty when no image carries it)"""
        try:
            values = self.frames_attributes[key]
        except KeyError:
            values = []
        return np.array(values, dtype=float)

    def to_thermavip(self, th_instance="Thermavip-1", player_id=0):
        """The reference hands the file to a running Thermavip viewer through shared memory (IRMovie.py:660-676); that bridge is outside
        this build: like the reference without a Thermavip instance, nothing is opened and None is returned."""
        return None

    # ---- filters applied while reading -----------------------------------------------------------------------------------------------
    @property
    def bad_pixels_correction(self):
        return self._bp_on

    @bad_pixels_correction.setter
    def bad_pixels_correction(self, value):
        self._bp_on = bool(value)
        _abi.enable_bad_pixels(self.handle, self._bp_on)

    @property
    def registration_file(self):
        return self._reg_file

    @registration_file.setter
    def registration_file(self, value):
        _abi.load_motion_correction_file(self.handle, str(value))
        self._reg_file = Path(value)

    @property
    def registration(self):
        return _abi.motion_correction_enabled(self.handle)

    @registration.setter
    def registration(self, value):
        _abi.enable_motion_correction(self.handle, bool(value))

    # ---- writing a (part of a) movie again ---------------------------------------------------------------------------------------------
    def to_h264(self, dst_filename, start_img=0, count=-1, clevel=8, attrs=None, times=None, frame_attributes=None, cthreads=8, cfiles=None,
                downsample=None):
        """Record images ``start_img .. start_img + count`` into a new file, with their attributes and time stamps.

        ``downsample=(factor, factor_std)`` or ``(factor, factor_std, method)``: the images go through a ``librir_amd.device.Downsampler``
        on the device, piece by piece, and only the images it keeps are recorded - each the per-pixel maximum since the last kept one,
        with the time stamp and the frame attributes of the image that triggered it."""
        available = self.images - start_img
        count = available if count < 0 else min(count, available)
        if count == 0:
            raise RuntimeError("No images in selected range to save")
        if frame_attributes is not None and len(frame_attributes) != count:
            raise RuntimeError("Given frame attributes are not equal to the number of saved images")
        global_attrs = dict(self.attributes) if attrs is None else attrs
        for stale in ("MIN_T", "MIN_T_HEIGHT", "STORE_IT"):  # they describe how THIS file stores its pixels
            global_attrs.pop(stale, None)
        stamps = [t * 1e9 for t in self.timestamps] if times is None else times
        rows, columns = self.image_size
        with IRSaver(str(dst_filename), columns, rows, rows, clevel) as saver:
            saver.set_global_attributes(global_attrs)
            saver.set_parameter("threads", cthreads)
            saver.set_parameter("codec", "h264")
            if downsample is not None:
                self._record_downsampled(saver, downsample, start_img, count, stamps, frame_attributes)
                return
            # A recording of this library goes from its loader to the saver without leaving the device (chunks decoded into device memory,
            # their images copied device to device into the chunk the saver assembles, attributes with them): 6 us an image.  Anything
            # else - raw files, read-back filters switched on, attributes given per image - goes image by image through host memory.
            if frame_attributes is None and _abi.transcode_images(self.handle, saver.handle, start_img, count,
                                                                  [int(stamps[pos]) for pos in range(start_img, start_img + count)]):
                return
            # (Measured and not kept for that path: a thread reading ahead of the recording one.  Image by image 33-70 us an image, in
            # stacks of sixteen through bulk library calls 34-37 us - against 30-33 us for one thing after the other as below.  Reading alone
            # is 17 us an image, recording alone 17-19: the two do not overlap, because the kernels' own traffic over the link does not - a
            # chunk's encode reading its frames from host memory (705 us) and a chunk's decode writing its frames there (660 us) take
            # 1 210-1 270 us together on two streams, with or without disjoint compute-unit masks, while the copy engines' transfers up and
            # down do overlap (587 + 585 -> 686 us), and so do a copy call upwards and the decode's writes (581 + 660 -> 812): it is the
            # kernels' reads of host memory that do not share the link.  profiles/r05_link_duplex.txt.)
            for written, pos in enumerate(range(start_img, start_img + count)):
                image = self.load_pos(pos, 0)
                saver.add_image(image, stamps[pos], attributes=self.frame_attributes if frame_attributes is None else frame_attributes[written])

    def _record_downsampled(self, saver, downsample, start_img, count, stamps, frame_attributes):
        """to_h264's images through a Downsampler: read to the device in pieces of at most ``_STATS_PIECE_BYTES``, the kept images recorded
        one by one with the attributes of their source positions"""
        import torch

        from ..device import Downsampler

        if len(downsample) not in (2, 3):
            raise ValueError("to_h264: downsample=(factor, factor_std) or (factor, factor_std, method) expected")
        h, w = self.image_size
        thin = Downsampler(w, h, downsample[0], downsample[1], None, downsample[2] if len(downsample) == 3 else 1)
        try:
            device = torch.device("cuda", torch.cuda.current_device())
            kept_buffer = torch.empty((self._piece_images(count, h, w), h, w), dtype=torch.uint16, device=device)
            for k0, k1, fr in self._pieces(range(start_img, start_img + count), device):
                first = start_img + k0
                kept = thin.push(fr, [int(stamps[pos]) for pos in range(first, start_img + k1)], out=kept_buffer[:k1 - k0])
                images = kept.frames.cpu().numpy()
                for image, at in zip(images, kept.positions):
                    pos = first + int(at)
                    if frame_attributes is None:
                        self.load_pos(pos, 0)  # (for the attributes of the image)
                        attributes = self.frame_attributes
                    else:
                        attributes = frame_attributes[pos - start_img]
                    saver.add_image(image, stamps[pos], attributes=attributes)
        finally:
            thin.close()

    def _build_outfile(self):
        """where pcr2h264 writes by default: beside the movie, suffix ``.h264``; a movie that is encoded already names itself
        (IRMovie.py:533-545)"""
        if self.video_file_format != FileFormat.H264:
            source = str(self._owned_file or self.filename)
            return os.path.abspath(os.path.splitext(source)[0] + ".h264")
        return self.filename

    def pcr2h264(self, outfile=None, overwrite=False, **kwargs):
        """A raw (PCR) movie re-recorded through the codec; ``kwargs`` go to ``to_h264``.  A destination that exists is kept unless
        ``overwrite``.  Returns the destination file name (IRMovie.py:520-531)."""
        outfile = outfile or self._build_outfile()
        if not os.path.exists(outfile) or overwrite:
            self.to_h264(outfile, **kwargs)
        return outfile
