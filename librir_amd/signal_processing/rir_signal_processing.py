"""ctypes shims over the signal_processing C ABI (include/rir_amd_signal_processing.h).

Same function names, argument meaning and error behaviour as the reference wrapper
(reference src/python/librir/signal_processing/rir_signal_processing.py:23-160 and :330-415):
numpy arrays in, numpy arrays out, ``RuntimeError`` on bad dimensions / dtypes / library errors.
"""
import ctypes as ct
from collections import namedtuple

import numpy as np

from ..low_level.misc import _signal_processing as _sp
from ..low_level.misc import last_error, result_buffer, toCharP

# numpy dtype -> type character of the C entry point.  The reference maps int64 to 'L'
# (duplicated dict key, rir_signal_processing.py:15-16); both int64 and uint64 are accepted here
# and int64 keeps its own signed instantiation.
_DTYPES = {
    np.dtype(np.bool_): "?",
    np.dtype(np.int8): "b",
    np.dtype(np.uint8): "B",
    np.dtype(np.int16): "h",
    np.dtype(np.uint16): "H",
    np.dtype(np.int32): "i",
    np.dtype(np.uint32): "I",
    np.dtype(np.int64): "l",
    np.dtype(np.uint64): "L",
    np.dtype(np.float32): "f",
    np.dtype(np.float64): "d",
}

_sp.translate.argtypes = [ct.c_int, ct.c_void_p, ct.c_void_p, ct.c_int, ct.c_int, ct.c_float, ct.c_float, ct.c_void_p, ct.c_char_p]
_sp.gaussian_filter.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_int, ct.c_int, ct.c_float]
_sp.rir_gaussian_filter_u16.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_int, ct.c_int, ct.c_float]
_sp.find_median_pixel.argtypes = [ct.c_void_p, ct.c_int, ct.c_float]
_sp.find_median_pixel_mask.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_int, ct.c_float]
_sp.bad_pixels_create.argtypes = [ct.c_void_p, ct.c_int, ct.c_int]
_sp.bad_pixels_correct.argtypes = [ct.c_int, ct.c_void_p, ct.c_void_p]
_sp.bad_pixels_destroy.argtypes = [ct.c_int]
_sp.bad_pixels_destroy.restype = None


def translate(image, dx, dy, strategy=str(), background=None):
    """Translate ``image`` by the floating point offset (dx, dy).

    strategy: "" / "noborder" (border pixels keep the source value), "constant" or "background"
    (border pixels set to ``background``), "nearest", "wrap".
    """
    image = np.asarray(image)
    if image.ndim != 2:
        raise RuntimeError("translate: wrong input image dimension")
    if strategy == "background" and background is None:
        raise RuntimeError("translate: wrong background value")
    ch = _DTYPES.get(image.dtype)
    if ch is None:
        raise RuntimeError("An error occured while calling 'translate'")
    strat = toCharP(strategy)
    if strat == b"constant":
        strat = b"background"
    src = np.ascontiguousarray(image)  # (the library reads it and leaves it alone: no copy of an array that is contiguous already)
    # "noborder" leaves the values of the pixels it does not reach in place: only then does the result start as a copy of the image
    dst = result_buffer(src.shape, src.dtype)
    if strat in (b"", b"noborder"):
        np.copyto(dst, src)
    back = np.zeros(1, dtype=image.dtype)
    if background is not None:
        back[0] = background
    r = _sp.translate(ord(ch), src.ctypes.data, dst.ctypes.data, src.shape[1], src.shape[0], np.float32(dx), np.float32(dy),
                      back.ctypes.data, strat)
    if r < 0:
        raise RuntimeError("An error occured while calling 'translate': " + last_error())
    return dst


def gaussian_filter(image, sigma=1.0):
    """Gaussian filter; the result is always float32."""
    image = np.asarray(image)
    if image.ndim != 2:
        raise RuntimeError("gaussian_filter: wrong input image dimension")
    dst = result_buffer(image.shape, np.float32)  # (the library writes every pixel or fails)
    r = -1
    if image.dtype == np.uint16 and 0 < float(sigma) < 2.5:
        # every uint16 is a float32: the kernel converts as it reads - the same bits as converting first (what the reference's wrapper does,
        # rir_signal_processing.py:85-113), half the bytes up the link and no float copy of the image on the host
        src = np.ascontiguousarray(image)
        r = _sp.rir_gaussian_filter_u16(src.ctypes.data, dst.ctypes.data, src.shape[1], src.shape[0], np.float32(sigma))
    if r < 0:
        src = np.ascontiguousarray(image, dtype=np.float32)
        r = _sp.gaussian_filter(src.ctypes.data, dst.ctypes.data, src.shape[1], src.shape[0], np.float32(sigma))
    if r < 0:
        raise RuntimeError("An error occured while calling 'gaussian_filter': " + last_error())
    return dst


def find_median_pixel(image, percent=0.5, mask=None):
    """Smallest pixel value below or at which at least percent*size pixels lie."""
    image = np.asarray(image)
    if image.ndim != 2:
        raise RuntimeError("find_median_pixel: wrong input image dimension")
    img = np.ascontiguousarray(image, dtype=np.uint16)
    if mask is not None:
        m = np.ascontiguousarray(mask, dtype=np.uint8)
        res = _sp.find_median_pixel_mask(img.ctypes.data, m.ctypes.data, img.size, float(percent))
    else:
        res = _sp.find_median_pixel(img.ctypes.data, img.size, float(percent))
    if res < 0:
        raise RuntimeError("An error occured while calling 'find_median_pixel': " + last_error())
    return res


def bad_pixels_create(first_image):
    first_image = np.asarray(first_image)
    if first_image.ndim != 2:
        raise RuntimeError("bad_pixels_create: wrong input image dimension")
    img = np.ascontiguousarray(first_image, dtype=np.uint16)
    h = _sp.bad_pixels_create(img.ctypes.data, img.shape[1], img.shape[0])
    if h <= 0:
        raise RuntimeError("An error occured while calling 'bad_pixels_create': " + last_error())
    return h


def bad_pixels_correct(handle, img):
    img = np.asarray(img)
    if img.ndim != 2:
        raise RuntimeError("bad_pixels_correct: wrong input image dimension")
    src = np.ascontiguousarray(img, dtype=np.uint16)
    out = result_buffer(src.shape, np.uint16)  # (the library writes every pixel or fails)
    r = _sp.bad_pixels_correct(handle, src.ctypes.data, out.ctypes.data)
    if r < 0:
        raise RuntimeError("An error occured while calling 'bad_pixels_correct': " + last_error())
    return out


def bad_pixels_destroy(handle):
    _sp.bad_pixels_destroy(handle)


# ---- extension: the three pre-recording filters in one call ----------------------------------------------------------------------
_sp.rir_filter_chain.argtypes = [ct.c_int, ct.c_void_p, ct.c_void_p, ct.c_int, ct.c_int, ct.c_float, ct.c_float, ct.c_float, ct.c_void_p, ct.c_char_p]


def filter_chain(image, bad_pixels, sigma, dx, dy, strategy="nearest", background=0):
    """Extension: ``bad_pixels.correct(image)`` -> ``gaussian_filter(sigma)`` -> ``translate(dx, dy, strategy)`` -> uint16 in ONE library call
    on one uint16 image (the three calls cross the link three times with two float images in between).  ``bad_pixels``: a ``BadPixels``
    object, a handle, or None.  Strategies "nearest" and "background" / "constant"."""
    img = np.ascontiguousarray(image)
    if img.ndim != 2 or img.dtype != np.uint16:
        raise RuntimeError("filter_chain: a 2-D uint16 image expected")
    if strategy == "constant":
        strategy = "background"
    handle = 0 if bad_pixels is None else int(getattr(bad_pixels, "handle", bad_pixels))
    out = result_buffer(img.shape, np.uint16)
    back = np.array([background], dtype=np.uint16)
    if _sp.rir_filter_chain(handle, img.ctypes.data, out.ctypes.data, img.shape[1], img.shape[0], float(sigma), float(dx), float(dy), back.ctypes.data,
                            toCharP(strategy)) < 0:
        raise RuntimeError("An error occured while calling 'filter_chain': " + (last_error() or ""))
    return out


# ---- what the extension forms share ------------------------------------------------------------------------------------------------
def _host_stack(name, images):
    """-> (the contiguous array, its view [n][h][w]) of an image or a stack"""
    img = np.ascontiguousarray(images)
    if img.ndim not in (2, 3):
        raise ValueError("%s: an image [h][w] or a stack [n][h][w] expected" % name)
    return img, img.reshape((-1,) + img.shape[-2:])


def _call(name, n, entry, *args):
    """the entry of the form `name` over `args`, unless there are n = 0 frames to go through; ``RuntimeError`` with the library's words when it fails"""
    if n and entry(*args) < 0:
        raise RuntimeError("An error occured while calling '%s': %s" % (name, last_error() or ""))


# ---- extension: temporal median of a stack ------------------------------------------------------------------------------------
_sp.rir_temporal_median.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_int]


def _temporal_median_args(shape, window, threshold, rows, first=0, count=None, step=1):
    """the parameters of a temporal median over a stack of `shape`, checked without a device; -> (rows, count)"""
    if len(shape) != 3:
        raise ValueError("temporal_median: a stack [n][h][w] expected")
    n, h, _ = shape
    if int(window) != window or not 1 <= window <= 63 or window % 2 == 0:
        raise ValueError("temporal_median: window must be odd, 1 to 63 (got %r)" % (window,))
    if not 0 <= int(threshold) <= 65535:
        raise ValueError("temporal_median: threshold must be in 0..65535")
    rows = h if rows is None else int(rows)
    if not 0 <= rows <= h:
        raise ValueError("temporal_median: rows must be in 0..h")
    step = int(step)
    if step < 1:
        raise ValueError("temporal_median: step must be >= 1")
    first = int(first)
    if not 0 <= first <= n:
        raise ValueError("temporal_median: first must be in 0..%d" % n)
    count = len(range(first, n, step)) if count is None else int(count)
    if count < 0 or (count > 0 and first + (count - 1) * step > n - 1):
        raise ValueError("temporal_median: outputs first + k * step (k < count) must lie in the stack")
    return rows, count


def temporal_median(images, window, threshold=0, rows=None):
    """Extension: temporal median of a uint16 stack ``images[n][h][w]`` (``rir_temporal_median``): image t becomes the upper median of
    images t - r .. t + r (r = window // 2, window odd 1..63, truncated at the ends of the stack) where it differs from image t by more
    than ``threshold``; rows ``>= rows`` (default: all rows filtered) are left as they are.  ``ValueError`` on bad parameters,
    ``RuntimeError`` when the library fails."""
    img = np.ascontiguousarray(images)
    if img.ndim != 3 or img.dtype != np.uint16:
        raise RuntimeError("temporal_median: a 3-D uint16 stack expected")
    rows, _ = _temporal_median_args(img.shape, window, threshold, rows)
    out = np.empty_like(img)
    n, h, w = img.shape
    _call("temporal_median", n, _sp.rir_temporal_median, img.ctypes.data, out.ctypes.data, w, h, n, int(window), int(threshold), rows)
    return out


# ---- extension: flat morphology ------------------------------------------------------------------------------------------------
_sp.rir_morphology.argtypes = [ct.c_int, ct.c_void_p, ct.c_void_p] + [ct.c_int] * 7

MORPHOLOGY_OPS = ("erode", "dilate", "open", "close", "tophat", "blackhat", "gradient")  # the op numbers of the C ABI
_MORPHOLOGY_TYPES = {"uint16": "H", "uint8": "B", "bool": "?"}


# The parameters that the window filters (morphology, the rank filters) share, checked without a device.  Each filter has one parameter of its
# own, tested at its own place among these - the op right after the type, the rank once the sizes are known - so the checks are three pieces
# that _morphology_args and _rank_filter_args call in their order; every piece raises ValueError with the filter's name in front.
def _window_type(name, shape, dtype_name):
    """-> the type char of the C ABI for a stack of `shape`"""
    if len(shape) != 3:
        raise ValueError("%s: a stack [n][h][w] expected" % name)
    if dtype_name not in _MORPHOLOGY_TYPES:
        raise ValueError("%s: uint16, uint8 or bool frames expected, not %s" % (name, dtype_name))
    return ord(_MORPHOLOGY_TYPES[dtype_name])


def _window_size(name, size):
    """-> (size_y, size_x) of a window parameter: an odd int for a square, or a pair of them, each 1..15"""
    sizes = tuple(size) if isinstance(size, (tuple, list)) else (size, size)
    if len(sizes) != 2 or not all(isinstance(s, (int, np.integer)) and not isinstance(s, bool) for s in sizes):
        raise ValueError("%s: size must be an odd int or (size_y, size_x)" % name)
    if not all(1 <= s <= 15 and s % 2 == 1 for s in sizes):
        raise ValueError("%s: sizes must be odd, 1 to 15 (got %r)" % (name, size))
    return int(sizes[0]), int(sizes[1])


def _window_rows(name, shape, rows):
    """-> the rows of the image within frames of `shape`: all of them for None"""
    _, h, w = shape
    if h < 1 or w < 1:
        raise ValueError("%s: empty frames" % name)
    rows = h if rows is None else int(rows)
    if not 0 <= rows <= h:
        raise ValueError("%s: rows must be in 0..h" % name)
    return rows


def _morphology_args(shape, dtype_name, op, size, rows):
    """the parameters of a morphology call over a stack of `shape`, checked without a device; -> (type char, op number, size_y, size_x, rows)"""
    type_char = _window_type("morphology", shape, dtype_name)
    if op not in MORPHOLOGY_OPS:
        raise ValueError("morphology: op must be one of %s (got %r)" % (", ".join(MORPHOLOGY_OPS), op))
    size_y, size_x = _window_size("morphology", size)
    return type_char, MORPHOLOGY_OPS.index(op), size_y, size_x, _window_rows("morphology", shape, rows)


def morphology(images, op, size, rows=None):
    """Extension: flat morphology of a uint16, uint8 or bool stack ``images[n][h][w]`` (or one image ``[h][w]``) with a centred rectangle
    ``size`` (an odd int, or ``(size_y, size_x)``, each 1..15) (``rir_morphology``).  ``op``: "erode" / "dilate" - min / max over the
    window clipped to the image -, "open" (dilate of erode), "close" (erode of dilate), "tophat" (image - open), "blackhat" (close -
    image), "gradient" (dilate - erode).  Per image this is ``scipy.ndimage.minimum_filter`` / ``maximum_filter(size=size,
    mode="nearest")`` composed stage by stage.  The image is its first ``rows`` rows (default: all); the others are copied.  Returns an
    array of the input's dtype and shape.  ``ValueError`` on bad parameters, ``RuntimeError`` when the library fails."""
    img, stack = _host_stack("morphology", images)
    type_char, op_number, size_y, size_x, rows = _morphology_args(stack.shape, img.dtype.name, op, size, rows)
    out = np.empty_like(stack)
    n, h, w = stack.shape
    _call("morphology", n, _sp.rir_morphology, type_char, stack.ctypes.data, out.ctypes.data, w, h, n, op_number, size_x, size_y, rows)
    return out.reshape(img.shape)


# ---- extension: spatial rank filters ---------------------------------------------------------------------------------------------
_sp.rir_rank_filter.argtypes = [ct.c_int, ct.c_void_p, ct.c_void_p] + [ct.c_int] * 7


def _rank_filter_args(shape, dtype_name, rank, size, rows):
    """the parameters of a rank filter over a stack of `shape`, checked without a device; a negative rank counts from the end, as in scipy;
    -> (type char, rank, size_y, size_x, rows)"""
    type_char = _window_type("rank_filter", shape, dtype_name)
    size_y, size_x = _window_size("rank_filter", size)
    cells = size_y * size_x
    if not isinstance(rank, (int, np.integer)) or isinstance(rank, bool):
        raise ValueError("rank_filter: rank must be an int")
    rank = int(rank) + cells if rank < 0 else int(rank)
    if not 0 <= rank < cells:
        raise ValueError("rank_filter: rank must be in %d..%d for a %d x %d window" % (-cells, cells - 1, size_y, size_x))
    return type_char, rank, size_y, size_x, _window_rows("rank_filter", shape, rows)


def percentile_rank(percent, size_y, size_x):
    """The rank ``scipy.ndimage.percentile_filter`` takes in a ``size_y x size_x`` window of n cells: n - 1 at 100, otherwise
    ``int(float(n) * percent / 100.0)``; a negative percent counts from 100.  ``ValueError`` outside [-100, 100]."""
    cells = int(size_y) * int(size_x)
    percent = float(percent)
    if percent < 0.0:
        percent += 100.0
    if not 0.0 <= percent <= 100.0:  # (NaN fails both)
        raise ValueError("percentile_rank: percent must be in -100..100")
    return cells - 1 if percent == 100.0 else int(float(cells) * percent / 100.0)


def rank_filter(images, rank, size, rows=None):
    """Extension: spatial rank filter of a uint16, uint8 or bool stack ``images[n][h][w]`` (or one image ``[h][w]``) with a centred rectangle
    ``size`` (an odd int, or ``(size_y, size_x)``, each 1..15) (``rir_rank_filter``): every pixel becomes the element of 0-based rank
    ``rank`` (negative: from the end) among the values of its window, which is always full - coordinates are replicated at the border.
    Per image this is ``scipy.ndimage.rank_filter(image, rank, size=size, mode="nearest")``; ``rank = size_y * size_x // 2`` is the median,
    ``percentile_rank`` gives the rank of a percentile.  The image is its first ``rows`` rows (default: all); the others are copied.
    Returns an array of the input's dtype and shape.  ``ValueError`` on bad parameters, ``RuntimeError`` when the library fails."""
    img, stack = _host_stack("rank_filter", images)
    type_char, rank, size_y, size_x, rows = _rank_filter_args(stack.shape, img.dtype.name, rank, size, rows)
    out = np.empty_like(stack)
    n, h, w = stack.shape
    _call("rank_filter", n, _sp.rir_rank_filter, type_char, stack.ctypes.data, out.ctypes.data, w, h, n, rank, size_x, size_y, rows)
    return out.reshape(img.shape)


# ---- extension: local window statistics ------------------------------------------------------------------------------------------
_sp.rir_local_stats.argtypes = [ct.c_int, ct.c_void_p] + [ct.c_int] * 6 + [ct.c_void_p] * 3
_sp.rir_local_threshold.argtypes = [ct.c_int, ct.c_void_p, ct.c_void_p] + [ct.c_int] * 10

LocalStats = namedtuple("LocalStats", ["sum", "sumsq", "mean", "n"])  # an array that was not asked for is None; n: the window's cells
LOCAL_POLARITIES = ("above", "below", "both")  # the polarity numbers of the C ABI
LOCAL_K_NUM_MAX, LOCAL_K_DEN_MAX, LOCAL_DELTA_MAX = 255, 64, 65535  # what keeps the z-score test inside int64


def _local_stats_args(name, shape, dtype_name, size, rows, outputs=None, k=None, delta=0, polarity="above"):
    """the parameters of ``local_stats`` (``outputs``: the three flags sum, sumsq, mean) or ``local_threshold`` (``k``, ``delta``,
    ``polarity``) over a stack of `shape`, checked without a device under the caller's `name`; -> (type char, size_y, size_x, rows) and,
    for a threshold, (k_num, k_den, delta, polarity number) after them"""
    type_char = _window_type(name, shape, dtype_name)
    size_y, size_x = _window_size(name, size)
    if outputs is not None:
        if not any(outputs):
            raise ValueError("%s: no output asked for" % name)
        return type_char, size_y, size_x, _window_rows(name, shape, rows)
    ks = tuple(k) if isinstance(k, (tuple, list)) else (k, 1)
    if len(ks) != 2 or not all(isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) for v in ks):
        raise ValueError("%s: k must be an int or (num, den)" % name)
    if not (0 <= ks[0] <= LOCAL_K_NUM_MAX and 1 <= ks[1] <= LOCAL_K_DEN_MAX):
        raise ValueError("%s: k = num / den needs 0 <= num <= %d and 1 <= den <= %d (got %r)" % (name, LOCAL_K_NUM_MAX, LOCAL_K_DEN_MAX, k))
    if not isinstance(delta, (int, np.integer)) or isinstance(delta, (bool, np.bool_)) or not -LOCAL_DELTA_MAX <= delta <= LOCAL_DELTA_MAX:
        raise ValueError("%s: delta must be an int in %d..%d" % (name, -LOCAL_DELTA_MAX, LOCAL_DELTA_MAX))
    if polarity not in LOCAL_POLARITIES:
        raise ValueError("%s: polarity must be one of %s (got %r)" % (name, ", ".join(LOCAL_POLARITIES), polarity))
    return type_char, size_y, size_x, _window_rows(name, shape, rows), int(ks[0]), int(ks[1]), int(delta), LOCAL_POLARITIES.index(polarity)


def local_stats(images, size, rows=None, sum=True, sumsq=False, mean=False):
    """Extension: local window statistics of a uint16, uint8 or bool stack ``images[n][h][w]`` (or one image ``[h][w]``) over a centred
    rectangle ``size`` (an odd int, or ``(size_y, size_x)``, each 1..15) (``rir_local_stats``): a ``LocalStats`` of arrays of the input's
    shape - ``sum`` (int32) the window's sum, ``sumsq`` (int64) its sum of squares, ``mean`` (the input's dtype) ``(sum + n // 2) // n`` -,
    None for what was not asked for, and the window's cell count ``n``.  The window is always full, coordinates replicated at the border: per image ``sum`` is
    ``scipy.ndimage.correlate(image.astype(int64), ones(size), mode="nearest")``.  The image is its first ``rows`` rows (default: all);
    below them the sums are 0 and the mean is the input.  ``ValueError`` on bad parameters, ``RuntimeError`` when the library fails."""
    img, stack = _host_stack("local_stats", images)
    type_char, size_y, size_x, rows = _local_stats_args("local_stats", stack.shape, img.dtype.name, size, rows, outputs=(sum, sumsq, mean))
    outs = [np.zeros(stack.shape, dt) if want else None for want, dt in ((sum, np.int32), (sumsq, np.int64), (mean, img.dtype))]
    n, h, w = stack.shape
    _call("local_stats", n, _sp.rir_local_stats, type_char, stack.ctypes.data, w, h, n, size_x, size_y, rows,
          *(None if o is None else o.ctypes.data for o in outs))
    return LocalStats(*(None if o is None else o.reshape(img.shape) for o in outs), size_y * size_x)


def local_threshold(images, size, k, delta=0, polarity="above", rows=None):
    """Extension: the z-score mask of a uint16, uint8 or bool stack ``images[n][h][w]`` (or one image ``[h][w]``) (``rir_local_threshold``): a
    bool array of the input's shape, True where the pixel lies more than ``delta`` above the mean of its ``size`` window and more than
    ``k`` (an int, or ``(num, den)`` with 0 <= num <= 255, 1 <= den <= 64) population standard deviations of that window off it, both strict
    and exact; ``polarity`` "below" tests below the mean, "both" either.  Window, border and ``rows`` as ``local_stats``; rows below the
    image are False.  ``ValueError`` on bad parameters, ``RuntimeError`` when the library fails."""
    img, stack = _host_stack("local_threshold", images)
    type_char, size_y, size_x, rows, k_num, k_den, delta, polarity = _local_stats_args("local_threshold", stack.shape, img.dtype.name, size, rows, k=k,
                                                                                       delta=delta, polarity=polarity)
    out = np.zeros(stack.shape, np.bool_)
    n, h, w = stack.shape
    _call("local_threshold", n, _sp.rir_local_threshold, type_char, stack.ctypes.data, out.ctypes.data, w, h, n, size_x, size_y, rows, k_num, k_den, delta,
          polarity)
    return out.reshape(img.shape)


# ---- extension: grey-level morphological reconstruction --------------------------------------------------------------------------
_sp.rir_reconstruct.argtypes = [ct.c_int, ct.c_void_p, ct.c_void_p, ct.c_void_p] + [ct.c_int] * 9 + [ct.c_void_p]

RECONSTRUCT_METHODS = ("dilation", "erosion")  # the method numbers of the C ABI
RECONSTRUCT_MARKER, RECONSTRUCT_SHIFT, RECONSTRUCT_BORDER = 0, 1, 2  # its marker modes
_TYPE_TOP = {"uint16": 65535, "uint8": 255, "bool": 1}
_NO_SHIFT = object()  # the h of a form whose marker is no shifted mask


def _reconstruct_args(name, shape, dtype_name, method, connectivity, rows, h=_NO_SHIFT):
    """the parameters of a reconstruction over a stack of `shape`, checked without a device; `h` is the shift of the marker where the call
    has one; -> (type char, method number, connectivity, rows, h or 0)"""
    type_char = _window_type(name, shape, dtype_name)
    if method not in RECONSTRUCT_METHODS:
        raise ValueError("%s: method must be one of %s (got %r)" % (name, ", ".join(RECONSTRUCT_METHODS), method))
    if isinstance(connectivity, (bool, np.bool_)) or connectivity not in (4, 8):
        raise ValueError("%s: connectivity must be 4 or 8 (got %r)" % (name, connectivity))
    if h is not _NO_SHIFT:
        if not isinstance(h, (int, np.integer)) or isinstance(h, (bool, np.bool_)) or not 0 <= int(h) <= _TYPE_TOP[dtype_name]:
            raise ValueError("%s: h must be an int in 0..%d for %s (got %r)" % (name, _TYPE_TOP[dtype_name], dtype_name, h))
    return type_char, RECONSTRUCT_METHODS.index(method), int(connectivity), _window_rows(name, shape, rows), 0 if h is _NO_SHIFT else int(h)


def _reconstruct_host(name, images, marker, method, connectivity, rows, mode, h, output):
    img, stack = _host_stack(name, images)
    type_char, method, connectivity, rows, param = _reconstruct_args(name, stack.shape, img.dtype.name, method, connectivity, rows, h)
    seed = None
    if marker is not None:
        seed = np.ascontiguousarray(marker)
        if seed.dtype != img.dtype or seed.shape != img.shape:
            raise ValueError("%s: the marker must have the mask's dtype and shape" % name)
    out = np.empty_like(stack)
    n, height, w = stack.shape
    _call(name, n, _sp.rir_reconstruct, type_char, stack.ctypes.data, None if seed is None else seed.ctypes.data, out.ctypes.data, w, height, n, method,
          connectivity, mode, param, output, rows, None)
    return out.reshape(img.shape)


def reconstruct(marker, mask, method="dilation", connectivity=8, rows=None):
    """Extension: grey-level morphological reconstruction of ``marker`` under ``mask``, uint16, uint8 or bool stacks ``[n][h][w]`` (or one
    image ``[h][w]``) of the same dtype and shape (``rir_reconstruct``, where the rule is defined).  ``method="dilation"``: the marker,
    clamped to ``min(marker, mask)``, spreads under the mask until nothing changes - the fixed point of ``min(mask, maximum_filter(f))`` over
    the 3x3 window (``connectivity=8``) or the cross (4), clipped to the image: ``skimage.morphology.reconstruction``, and on bool
    ``scipy.ndimage.binary_propagation(marker, structure, mask=mask)``.  ``method="erosion"``: the dual, from ``max(marker, mask)`` down.
    The image is its first ``rows`` rows (default: all); the others are a copy of the mask.  Returns an array of the input's dtype and
    shape.  ``ValueError`` on bad parameters, ``RuntimeError`` when the library fails."""
    return _reconstruct_host("reconstruct", mask, marker, method, connectivity, rows, RECONSTRUCT_MARKER, _NO_SHIFT, 0)


def h_maxima(images, h, connectivity=8, rows=None):
    """Extension: the h-maxima transform ``R(images - h, images)``, reconstruction by dilation of the image lowered by ``h`` (saturating at
    0) under itself: every maximum cut down by ``h``, or to the level at which it joins a higher one (``reconstruct``)"""
    return _reconstruct_host("h_maxima", images, None, "dilation", connectivity, rows, RECONSTRUCT_SHIFT, h, 0)


def h_dome(images, h, connectivity=8, rows=None):
    """Extension: the h-domes ``images - R(images - h, images)``: what stands above its surround, at most ``h`` of it, whatever the extent
    of the structure - a top-hat without a window (``reconstruct``)"""
    return _reconstruct_host("h_dome", images, None, "dilation", connectivity, rows, RECONSTRUCT_SHIFT, h, 1)


def fill_holes(images, connectivity=4, rows=None):
    """Extension: reconstruction by erosion from the border of the image: every basin that does not reach the border is filled up to its
    rim.  On a bool mask at the default ``connectivity=4`` (of the background) this is ``scipy.ndimage.binary_fill_holes`` (``reconstruct``)"""
    return _reconstruct_host("fill_holes", images, None, "erosion", connectivity, rows, RECONSTRUCT_BORDER, _NO_SHIFT, 0)


# ---- extension: exact Euclidean distance transform -------------------------------------------------------------------------------
_sp.rir_distance_transform.argtypes = [ct.c_int, ct.c_void_p] + [ct.c_int] * 6 + [ct.c_void_p, ct.c_void_p]

DIST2_NONE = 0x7FFFFFFF  # dist2 of an image without a background pixel (RIR_DIST2_NONE)
DISTANCE_MAX_SIDE = 16384
_DISTANCE_TYPES = {"bool": ("?", 0, 1), "uint8": ("B", 0, 255), "uint16": ("H", 0, 65535), "int32": ("i", -(1 << 31), (1 << 31) - 1)}


def _distance_transform_args(shape, dtype_name, background=0, border=False, rows=None):
    """the parameters of a distance transform over a stack of `shape`, checked without a device; -> (type char, background, border, rows)"""
    if len(shape) != 3:
        raise ValueError("distance_transform: a stack [n][h][w] expected")
    if dtype_name not in _DISTANCE_TYPES:
        raise ValueError("distance_transform: bool, uint8, uint16 or int32 masks expected, not %s" % dtype_name)
    type_char, lo, hi = _DISTANCE_TYPES[dtype_name]
    if not isinstance(background, (int, np.integer)) or (isinstance(background, (bool, np.bool_)) and dtype_name != "bool"):
        raise ValueError("distance_transform: background must be an int")
    if not lo <= int(background) <= hi:
        raise ValueError("distance_transform: background %d is outside the range of %s" % (int(background), dtype_name))
    if not isinstance(border, (bool, np.bool_)) and border not in (0, 1):
        raise ValueError("distance_transform: border must be a bool")
    _, h, w = shape
    if not (1 <= h <= DISTANCE_MAX_SIDE and 1 <= w <= DISTANCE_MAX_SIDE):
        raise ValueError("distance_transform: frames of 1..%d rows and columns expected" % DISTANCE_MAX_SIDE)
    return ord(type_char), int(background), int(bool(border)), _window_rows("distance_transform", shape, rows)


def distance_transform(images, background=0, border=False, rows=None, return_indices=False):
    """Extension: exact Euclidean distance transform of a bool, uint8, uint16 or int32 stack ``images[n][h][w]`` (or one image ``[h][w]``)
    (``rir_distance_transform``): an int32 array of the input's shape with the SQUARED distance of every pixel to the nearest pixel equal to
    ``background`` in its image - ``round(scipy.ndimage.distance_transform_edt(images != background) ** 2)`` wherever the image has a
    background pixel, ``DIST2_NONE`` where it has none.  ``border=True``: everything outside the image is background too.  The image is
    its first ``rows`` rows (default: all); the others get 0.  ``return_indices=True``: ``(dist2, index)``, index the lowest flat index
    ``y * w + x`` among the nearest background pixels, -1 where there is none or the outside is strictly nearer, a pixel's own index in
    the rows outside the image (scipy's ``return_indices`` breaks ties differently).  At most 16 384 rows and columns.  ``ValueError`` on
    bad parameters, ``RuntimeError`` when the library fails."""
    img, stack = _host_stack("distance_transform", images)
    type_char, background, border, rows = _distance_transform_args(stack.shape, img.dtype.name, background, border, rows)
    n, h, w = stack.shape
    dist2 = np.empty(stack.shape, np.int32)
    index = np.empty(stack.shape, np.int32) if return_indices else None
    _call("distance_transform", n, _sp.rir_distance_transform, type_char, stack.ctypes.data, w, h, n, background, border, rows, dist2.ctypes.data,
          index.ctypes.data if return_indices else None)
    dist2 = dist2.reshape(img.shape)
    return (dist2, index.reshape(img.shape)) if return_indices else dist2


# ---- extension: per-region statistics ------------------------------------------------------------------------------------------
_sp.rir_region_stats.argtypes = [ct.c_void_p, ct.c_void_p] + [ct.c_int] * 5 + [ct.c_void_p] * 7

MAX_REGIONS = 1 << 24


class RegionStats(namedtuple("RegionStats", "count sum sumsq min max argmin argmax")):
    """Statistics per (frame, region), each ``[n][nregions]``: count (int32), sum and sumsq (int64, exact), min and max (int32), argmin and
    argmax (int32: the lowest flat index y * w + x that holds the extreme).  An empty region has count, sum and sumsq 0 and -1 elsewhere.
    numpy arrays (``signal_processing.region_stats``) or CUDA tensors (``device.region_stats``)."""

    __slots__ = ()

    def mean(self):
        """float64 mean from the exact sum; NaN where count == 0"""
        if isinstance(self.sum, np.ndarray):
            with np.errstate(invalid="ignore", divide="ignore"):
                return self.sum.astype(np.float64) / self.count
        return self.sum.double() / self.count

    def std(self):
        """float64 population standard deviation from the exact sums; NaN where count == 0"""
        if isinstance(self.sum, np.ndarray):
            c = self.count.astype(np.float64)
            with np.errstate(invalid="ignore", divide="ignore"):
                m = self.sum / c
                return np.sqrt(np.maximum((self.sumsq - self.sum * m) / c, 0.0))
        c = self.count.double()
        m = self.sum.double() / c
        return ((self.sumsq.double() - self.sum.double() * m) / c).clamp_min(0.0).sqrt()


def _region_stats_args(frames_shape, labels_shape, nregions, what="region_stats", max_regions=MAX_REGIONS):
    """the shapes of a region_stats (or region_quantiles) call, checked without a device; -> (n, h, w, labels_per_frame).  nregions None is
    left to the caller."""
    if len(frames_shape) == 2:
        frames_shape = (1,) + tuple(frames_shape)
    if len(frames_shape) != 3:
        raise ValueError("%s: frames (n, h, w) or (h, w) expected" % what)
    n, h, w = frames_shape
    if h < 1 or w < 1 or h * w >= 1 << 31:
        raise ValueError("%s: frames of at least 1x1 and fewer than 2^31 pixels expected" % what)
    if tuple(labels_shape) == (h, w):
        per_frame = 0
    elif tuple(labels_shape) == (n, h, w):
        per_frame = 1
    else:
        raise ValueError("%s: labels of shape %s or %s expected, not %s" % (what, (h, w), (n, h, w), tuple(labels_shape)))
    if nregions is not None and (int(nregions) != nregions or not 1 <= nregions <= max_regions):
        raise ValueError("%s: nregions must be in 1..2^%d (got %r)" % (what, max_regions.bit_length() - 1, nregions))
    return n, h, w, per_frame


def region_stats(images, labels, nregions=None):
    """Extension: statistics of a uint16 stack ``images[n][h][w]`` (or one ``(h, w)`` image) over the regions of the int32 label map
    ``labels`` (``(h, w)`` shared by every image, or ``(n, h, w)``): a ``RegionStats`` of numpy arrays ``[n][nregions]``
    (``rir_region_stats``).  Labels outside [0, nregions) are ignored; ``nregions=None`` takes labels.max() + 1 (at least 1).
    ``ValueError`` on bad shapes or ``nregions``, ``RuntimeError`` on other dtypes and when the library fails."""
    img = np.ascontiguousarray(images)
    lab = np.ascontiguousarray(labels)
    if img.dtype != np.uint16:
        raise RuntimeError("region_stats: uint16 images expected, not %s" % img.dtype)
    if lab.dtype != np.int32:
        raise RuntimeError("region_stats: int32 labels expected, not %s" % lab.dtype)
    n, h, w, per_frame = _region_stats_args(img.shape, lab.shape, nregions)
    if nregions is None:
        nregions = max(1, int(lab.max()) + 1 if lab.size else 1)
        _region_stats_args(img.shape, lab.shape, nregions)
    k = int(nregions)
    out = RegionStats(*(np.empty((n, k), dt) for dt in (np.int32, np.int64, np.int64, np.int32, np.int32, np.int32, np.int32)))
    _call("region_stats", n, _sp.rir_region_stats, img.ctypes.data, lab.ctypes.data, w, h, n, per_frame, k, *(a.ctypes.data for a in out))
    return out


# ---- extension: per-region geometry ------------------------------------------------------------------------------------------------
_sp.rir_region_geometry.argtypes = [ct.c_void_p, ct.c_void_p] + [ct.c_int] * 5 + [ct.c_void_p] * 4

MAX_GEOMETRY_SIDE = 32768


def _f64(a):
    return a.astype(np.float64) if isinstance(a, np.ndarray) else a.double()


def _stack_last(parts):
    if isinstance(parts[0], np.ndarray):
        return np.stack(parts, -1)
    import torch

    return torch.stack(parts, -1)


class RegionGeometry(namedtuple("RegionGeometry", "count bbox moments weighted")):
    """Geometry per (frame, region), ``[n][nregions]`` leading: count (int32), bbox ``[..][4]`` = xmin, ymin, xmax, ymax inclusive (int32;
    -1 four times for an empty region), moments ``[..][5]`` = the exact sums of x, y, x^2, x*y, y^2 over the region's pixels (int64) and
    weighted ``[..][3]`` = the exact sums of v, v*x, v*y (int64; None when no frames were given).  numpy arrays
    (``signal_processing.region_geometry``) or CUDA tensors (``device.region_geometry``).

    The helpers are float64 arithmetic on these exact integers (the integers are converted first: exact below 2^53): the centroids carry
    one rounding of the division, and the rounding error of ``covariance`` - a difference of two terms of size up to w^2 + h^2 - is
    bounded by about 4 * 2^-53 * (w^2 + h^2): 7.3e-10 at 1024x768, where 2.5e-11 was observed against rational arithmetic."""

    __slots__ = ()

    def _ratios(self, num, den):
        """num[..][k] / den[..] in float64; NaN where den == 0"""
        num, den = _f64(num), _f64(den)[..., None]
        if isinstance(num, np.ndarray):
            with np.errstate(invalid="ignore", divide="ignore"):
                return np.where(den == 0, np.nan, num / den)
        return (num / den).masked_fill(den == 0, float("nan"))

    def centroid(self):
        """float64 ``[..][2]`` = (sum x / count, sum y / count); NaN where count == 0"""
        return self._ratios(self.moments[..., 0:2], self.count)

    def weighted_centroid(self):
        """float64 ``[..][2]`` = (sum v*x / sum v, sum v*y / sum v); NaN where sum v == 0"""
        if self.weighted is None:
            raise ValueError("weighted_centroid: the geometry was computed without frames")
        return self._ratios(self.weighted[..., 1:3], self.weighted[..., 0])

    def covariance(self):
        """float64 ``[..][3]`` = (cxx, cxy, cyy) = (sum x^2 / c - mx^2, sum x*y / c - mx * my, sum y^2 / c - my^2), the population covariance
        of the pixel coordinates; NaN where count == 0"""
        m = self._ratios(self.moments, self.count)
        mx, my = m[..., 0], m[..., 1]
        return _stack_last([m[..., 2] - mx * mx, m[..., 3] - mx * my, m[..., 4] - my * my])

    def ellipse(self):
        """float64 ``[..][3]`` = (major, minor, angle) of the ellipse with the region's covariance: the full axis lengths 4 * sqrt(l+) and
        4 * sqrt(l-), l+- = (cxx + cyy) / 2 +- sqrt(((cxx - cyy) / 2)^2 + cxy^2) clamped at 0, and the angle of the major axis from +x
        towards +y, atan2(2 cxy, cxx - cyy) / 2 in (-pi/2, pi/2] (0 for a single pixel or a disc); NaN where count == 0"""
        c = self.covariance()
        cxx, cxy, cyy = c[..., 0], c[..., 1], c[..., 2]
        half, diff = (cxx + cyy) / 2, (cxx - cyy) / 2
        if isinstance(c, np.ndarray):
            root = np.sqrt(diff * diff + cxy * cxy)
            return np.stack([4 * np.sqrt(np.maximum(half + root, 0.0)), 4 * np.sqrt(np.maximum(half - root, 0.0)),
                             0.5 * np.arctan2(2 * cxy, cxx - cyy)], -1)
        import torch

        root = (diff * diff + cxy * cxy).sqrt()
        return torch.stack([4 * (half + root).clamp_min(0.0).sqrt(), 4 * (half - root).clamp_min(0.0).sqrt(),
                            0.5 * torch.atan2(2 * cxy, cxx - cyy)], -1)


def _region_geometry_args(labels_shape, frames_shape, nregions, what="region_geometry"):
    """the shapes of a region_geometry call, checked without a device; -> (n, h, w, labels_per_frame).  frames_shape None: no weights, and
    the labels alone give n.  nregions None is left to the caller."""
    labels_shape = tuple(labels_shape)
    if frames_shape is None:
        if len(labels_shape) not in (2, 3):
            raise ValueError("%s: labels (h, w) or (n, h, w) expected, not %s" % (what, labels_shape))
        frames_shape = labels_shape
    n, h, w, per_frame = _region_stats_args(tuple(frames_shape), labels_shape, nregions, what)
    if h > MAX_GEOMETRY_SIDE or w > MAX_GEOMETRY_SIDE:
        raise ValueError("%s: at most %d rows and columns expected" % (what, MAX_GEOMETRY_SIDE))
    return n, h, w, per_frame


def region_geometry(labels, nregions=None, frames=None):
    """Extension: where the regions of the int32 label map ``labels`` (``(h, w)``, or ``(n, h, w)``) are and how they are spread - a
    ``RegionGeometry`` of numpy arrays (``rir_region_geometry``): count, bounding box, the exact first and second moments of the pixel
    coordinates and, with ``frames`` (uint16 ``(n, h, w)`` or one ``(h, w)`` image; a shared ``(h, w)`` map then serves every image), the
    sums weighted by the pixel values; ``weighted`` is None without frames.  Labels outside [0, nregions) are ignored; ``nregions=None``
    takes labels.max() + 1 (at least 1).  ``ValueError`` on bad shapes or ``nregions``, ``RuntimeError`` on other dtypes and when the
    library fails."""
    lab = np.ascontiguousarray(labels)
    img = None if frames is None else np.ascontiguousarray(frames)
    if img is not None and img.dtype != np.uint16:
        raise RuntimeError("region_geometry: uint16 frames expected, not %s" % img.dtype)
    if lab.dtype != np.int32:
        raise RuntimeError("region_geometry: int32 labels expected, not %s" % lab.dtype)
    shapes = (lab.shape, None if img is None else img.shape)
    n, h, w, per_frame = _region_geometry_args(*shapes, nregions)
    if nregions is None:
        nregions = max(1, int(lab.max()) + 1 if lab.size else 1)
        _region_geometry_args(*shapes, nregions)
    k = int(nregions)
    out = RegionGeometry(np.empty((n, k), np.int32), np.empty((n, k, 4), np.int32), np.empty((n, k, 5), np.int64),
                         None if img is None else np.empty((n, k, 3), np.int64))
    _call("region_geometry", n, _sp.rir_region_geometry, lab.ctypes.data, None if img is None else img.ctypes.data, w, h, n, per_frame, k,
          out.count.ctypes.data, out.bbox.ctypes.data, out.moments.ctypes.data, None if img is None else out.weighted.ctypes.data)
    return out


# ---- extension: per-region quantiles ---------------------------------------------------------------------------------------------
_sp.rir_region_quantiles.argtypes = [ct.c_void_p, ct.c_void_p] + [ct.c_int] * 5 + [ct.c_void_p, ct.c_int, ct.c_void_p, ct.c_void_p]

MAX_QUANTILE_REGIONS = 1 << 16
MAX_PERCENTS = 8


class RegionQuantiles(namedtuple("RegionQuantiles", "count values")):
    """Quantiles per (frame, region): count ``[n][nregions]`` and values ``[n][nregions][len(percents)]`` (int32).  With c = count and
    t = (int)roundf((float)c * p) - float32, half away from zero, the reference's ``find_median_pixel_mask`` rule - a value is -1 for an
    empty region, 0 when t == 0, else the t-th smallest value of the region, and 0 where that is 65535 (which the reference counts in no
    bin).  numpy arrays (``signal_processing.region_quantiles``) or CUDA tensors (``device.region_quantiles``)."""

    __slots__ = ()


def _region_quantiles_percents(percents):
    """a float or a sequence of 1..8 floats in [0, 1]; -> float32 array"""
    p = np.atleast_1d(np.asarray(percents, dtype=np.float64))
    if p.ndim != 1 or not 1 <= p.size <= MAX_PERCENTS:
        raise ValueError("region_quantiles: 1..%d percents expected" % MAX_PERCENTS)
    if not np.all((p >= 0.0) & (p <= 1.0)):  # NaN fails both
        raise ValueError("region_quantiles: every percent must be in [0, 1] (got %r)" % (p.tolist(),))
    return np.ascontiguousarray(p, dtype=np.float32)


def _region_quantiles_args(frames_shape, labels_shape, nregions):
    return _region_stats_args(frames_shape, labels_shape, nregions, "region_quantiles", MAX_QUANTILE_REGIONS)


def region_quantiles(images, labels, percents, nregions=None):
    """Extension: quantiles of a uint16 stack ``images[n][h][w]`` (or one ``(h, w)`` image) over the regions of the int32 label map
    ``labels`` (``(h, w)`` shared by every image, or ``(n, h, w)``) at ``percents`` (a float or 1..8 floats in [0, 1]): a
    ``RegionQuantiles`` of numpy arrays (``rir_region_quantiles``).  Labels outside [0, nregions) are ignored; ``nregions=None`` takes
    labels.max() + 1 (at least 1); at most 65 536 regions.  ``ValueError`` on bad shapes, ``nregions`` or percents, ``RuntimeError`` on
    other dtypes and when the library fails."""
    img = np.ascontiguousarray(images)
    lab = np.ascontiguousarray(labels)
    if img.dtype != np.uint16:
        raise RuntimeError("region_quantiles: uint16 images expected, not %s" % img.dtype)
    if lab.dtype != np.int32:
        raise RuntimeError("region_quantiles: int32 labels expected, not %s" % lab.dtype)
    pc = _region_quantiles_percents(percents)
    n, h, w, per_frame = _region_quantiles_args(img.shape, lab.shape, nregions)
    if nregions is None:
        nregions = max(1, int(lab.max()) + 1 if lab.size else 1)
        _region_quantiles_args(img.shape, lab.shape, nregions)
    k = int(nregions)
    out = RegionQuantiles(np.empty((n, k), np.int32), np.empty((n, k, pc.size), np.int32))
    _call("region_quantiles", n, _sp.rir_region_quantiles, img.ctypes.data, lab.ctypes.data, w, h, n, per_frame, k, pc.ctypes.data, pc.size,
          out.count.ctypes.data, out.values.ctypes.data)
    return out


# ---- extension: per-region histograms ---------------------------------------------------------------------------------------------
_sp.rir_region_histogram.argtypes = [ct.c_void_p, ct.c_void_p] + [ct.c_int] * 9 + [ct.c_void_p] * 3

MAX_HISTOGRAM_REGIONS = 1 << 16
MAX_HISTOGRAM_BINS = 1 << 16
MAX_HISTOGRAM_CELLS = 1 << 24


class RegionHistogram(namedtuple("RegionHistogram", "count hist outside lo width")):
    """Histograms per (frame, region), int32: count ``[n][nregions]``, hist ``[n][nregions][nbins]`` - bin b counts the values v with
    lo + b * width <= v < lo + (b + 1) * width - and outside ``[n][nregions][2]``, the values below lo and those at or above
    lo + nbins * width, so that count == outside[..., 0] + hist.sum(-1) + outside[..., 1].  ``lo`` and ``width`` are the ints of the call.
    numpy arrays (``signal_processing.region_histogram``) or tensors (``device.region_histogram``, ``device.histogram``); the helpers
    answer in kind."""

    __slots__ = ()

    def _numpy(self):
        return isinstance(self.hist, np.ndarray)

    def _bins(self, dtype):
        """0 .. nbins - 1 beside the histograms"""
        nbins = self.hist.shape[-1]
        if self._numpy():
            return np.arange(nbins, dtype=np.dtype(dtype))
        import torch

        return torch.arange(nbins, dtype=getattr(torch, dtype), device=self.hist.device)

    def edges(self):
        """int64 ``[nbins + 1]``: bin b is [edges[b], edges[b + 1])"""
        nbins = self.hist.shape[-1]
        if self._numpy():
            return self.lo + np.arange(nbins + 1, dtype=np.int64) * self.width
        import torch

        return self.lo + torch.arange(nbins + 1, dtype=torch.int64, device=self.hist.device) * self.width

    def _lowest_of_the_largest(self, score, nothing):
        """per (frame, region) the lowest bin whose score is the largest, as a min over the bins that hold it: ties go to the lowest bin by
        construction; -1 where `nothing`"""
        nbins = self.hist.shape[-1]
        bins = self._bins("int32")
        if self._numpy():
            first = np.where(score == score.max(-1, keepdims=True), bins, nbins).min(-1)
            return np.where(nothing, -1, first).astype(np.int32)
        import torch

        first = torch.where(score == score.amax(-1, keepdim=True), bins, torch.full_like(bins, nbins)).amin(-1)
        return torch.where(nothing, torch.full_like(first, -1), first)

    def mode(self):
        """int32 ``[n][nregions]``: the lowest bin among the fullest; -1 where every bin is empty"""
        return self._lowest_of_the_largest(self.hist, self.hist.max(-1) == 0 if self._numpy() else self.hist.amax(-1) == 0)

    def cumulative(self):
        """int64 ``[n][nregions][nbins]``: the counts of the bins up to and including each"""
        if self._numpy():
            return np.cumsum(self.hist, -1, dtype=np.int64)
        import torch

        return torch.cumsum(self.hist, -1, dtype=torch.int64)

    def otsu(self):
        """float64 ``[n][nregions]``: Otsu's threshold as a bin - the bin t that maximises the between-class variance of the classes
        "bins <= t" and "bins > t", the lowest such t (the values of the upper class start at edges()[t + 1]); -1 where fewer than two
        bins are occupied.  With c = cumulative(), N = c[-1], m[t] = sum of b * hist[b] over b <= t and M = m[-1], the variance is
        (M * c[t] - m[t] * N)^2 / (c[t] * (N - c[t])) up to the factor N^2: the counts are exact, the products and the quotient float64."""
        c = _f64(self.cumulative())
        m = _f64(self.hist) * self._bins("float64")
        m = np.cumsum(m, -1) if self._numpy() else m.cumsum(-1)
        total, moment = c[..., -1:], m[..., -1:]
        split = c * (total - c)
        few = (self.hist > 0).sum(-1) < 2
        if self._numpy():
            with np.errstate(invalid="ignore", divide="ignore"):
                score = np.where(split > 0, (moment * c - m * total) ** 2 / split, -1.0)
        else:
            import torch

            score = torch.where(split > 0, (moment * c - m * total) ** 2 / split, torch.full_like(split, -1.0))
        return _f64(self._lowest_of_the_largest(score, few))


def _region_histogram_bins(nbins, lo, width, nregions=1, what="region_histogram"):
    """the bins of a histogram call, checked without a device; -> (nbins, lo, width) as ints"""
    for name, v, first, last in (("nbins", nbins, 1, MAX_HISTOGRAM_BINS), ("lo", lo, 0, 65535), ("width", width, 1, 65536)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not first <= v <= last:
            raise ValueError("%s: %s must be an int in %d..%d (got %r)" % (what, name, first, last, v))
    if nregions is not None and int(nregions) * int(nbins) > MAX_HISTOGRAM_CELLS:
        raise ValueError("%s: nregions * nbins must be at most 2^24 (got %d * %d)" % (what, nregions, nbins))
    return int(nbins), int(lo), int(width)


def _histogram_rows(rows, h, what="region_histogram"):
    """rows None is h; -> rows as an int in 0..h"""
    if rows is None:
        return h
    if isinstance(rows, bool) or not isinstance(rows, (int, np.integer)) or not 0 <= rows <= h:
        raise ValueError("%s: rows must be an int in 0..%d (got %r)" % (what, h, rows))
    return int(rows)


def _region_histogram_args(frames_shape, labels_shape, nbins, lo=0, width=1, nregions=None, rows=None, what="region_histogram"):
    """the shapes and bins of a region_histogram call, checked without a device; labels_shape None: no map, one region.
    -> (n, h, w, labels_per_frame, nbins, lo, width, rows).  nregions None is left to the caller."""
    if labels_shape is None:
        if nregions not in (None, 1):
            raise ValueError("%s: without labels there is one region (got nregions %r)" % (what, nregions))
        nregions = 1
        n, h, w, per_frame = _region_stats_args(frames_shape, tuple(frames_shape)[-2:], nregions, what)
    else:
        n, h, w, per_frame = _region_stats_args(frames_shape, labels_shape, nregions, what, MAX_HISTOGRAM_REGIONS)
    nbins, lo, width = _region_histogram_bins(nbins, lo, width, nregions, what)
    return n, h, w, per_frame, nbins, lo, width, _histogram_rows(rows, h, what)


def region_histogram(images, labels, nbins, lo=0, width=1, nregions=None, rows=None):
    """Extension: histograms of a uint16 stack ``images[n][h][w]`` (or one ``(h, w)`` image) over the regions of the int32 label map
    ``labels`` (``(h, w)`` shared by every image, or ``(n, h, w)``; None: the whole image is region 0), ``nbins`` bins of ``width``
    levels from ``lo``: a ``RegionHistogram`` of numpy arrays (``rir_region_histogram``).  Only the first ``rows`` rows of every image
    and map are counted (None: all).  Labels outside [0, nregions) are ignored; ``nregions=None`` takes labels.max() + 1 (at least 1); at
    most 65 536 regions and bins, nregions * nbins at most 2^24.  ``ValueError`` on bad shapes, bins, rows or ``nregions``,
    ``RuntimeError`` on other dtypes and when the library fails."""
    img = np.ascontiguousarray(images)
    lab = None if labels is None else np.ascontiguousarray(labels)
    if img.dtype != np.uint16:
        raise RuntimeError("region_histogram: uint16 images expected, not %s" % img.dtype)
    if lab is not None and lab.dtype != np.int32:
        raise RuntimeError("region_histogram: int32 labels expected, not %s" % lab.dtype)
    shapes = (img.shape, None if lab is None else lab.shape)
    n, h, w, per_frame, nbins, lo, width, rows = _region_histogram_args(*shapes, nbins, lo, width, nregions, rows)
    if nregions is None:
        nregions = 1 if lab is None else max(1, int(lab.max()) + 1 if lab.size else 1)
        _region_histogram_args(*shapes, nbins, lo, width, nregions, rows)
    k = int(nregions)
    out = RegionHistogram(np.zeros((n, k), np.int32), np.zeros((n, k, nbins), np.int32), np.zeros((n, k, 2), np.int32), lo, width)
    _call("region_histogram", n, _sp.rir_region_histogram, img.ctypes.data, None if lab is None else lab.ctypes.data, w, h, rows, n, per_frame, k, lo, width,
          nbins, out.count.ctypes.data, out.hist.ctypes.data, out.outside.ctypes.data)
    return out


# ---- extension: per-pixel statistics over time ----------------------------------------------------------------------------------
_sp.rir_pixel_stats.argtypes = [ct.c_void_p] + [ct.c_int] * 3 + [ct.c_void_p] * 6

_PIXEL_DTYPES = ("int64", "int64", "int32", "int32", "int32", "int32")  # of sum sumsq min max argmin argmax


class PixelStats(namedtuple("PixelStats", "sum sumsq min max argmin argmax")):
    """Statistics per pixel over time, each ``[h][w]``: sum and sumsq (int64, exact), min and max (int32), argmin and argmax (int32: the
    lowest time index that holds the extreme).  A group that was not asked for (sum, sumsq / min, max, argmin, argmax) is ``None``.
    ``count`` is the number of frames behind them; with none the sums are 0 and the other four -1.  numpy arrays
    (``signal_processing.pixel_stats``) or CUDA tensors (``device.pixel_stats``)."""

    count = 0

    def __new__(cls, sum, sumsq, min, max, argmin, argmax, count=0):
        self = super().__new__(cls, sum, sumsq, min, max, argmin, argmax)
        self.count = int(count)
        return self

    def mean(self):
        """float64 mean from the exact sum; NaN where count == 0"""
        if isinstance(self.sum, np.ndarray):
            with np.errstate(invalid="ignore", divide="ignore"):
                return self.sum.astype(np.float64) / np.float64(self.count)
        return self.sum.double() / float(self.count) if self.count else self.sum.double() * float("nan")

    def std(self):
        """float64 population standard deviation from the exact sums; NaN where count == 0"""
        if isinstance(self.sum, np.ndarray):
            c = np.float64(self.count)
            with np.errstate(invalid="ignore", divide="ignore"):
                m = self.sum / c
                return np.sqrt(np.maximum((self.sumsq - self.sum * m) / c, 0.0))
        if not self.count:
            return self.sum.double() * float("nan")
        c = float(self.count)
        m = self.sum.double() / c
        return ((self.sumsq.double() - self.sum.double() * m) / c).clamp_min(0.0).sqrt()


def _pixel_stats_args(frames_shape, sums=True, extremes=True, t0=0):
    """the arguments of a pixel_stats call, checked without a device; -> (n, h, w)"""
    if len(frames_shape) == 2:
        frames_shape = (1,) + tuple(frames_shape)
    if len(frames_shape) != 3:
        raise ValueError("pixel_stats: frames (n, h, w) or (h, w) expected")
    n, h, w = frames_shape
    if h < 1 or w < 1 or h * w >= 1 << 31:
        raise ValueError("pixel_stats: frames of at least 1x1 and fewer than 2^31 pixels expected")
    if not sums and not extremes:
        raise ValueError("pixel_stats: at least one of sums and extremes expected")
    if int(t0) != t0 or t0 < 0 or t0 + n > (1 << 31) - 1:
        raise ValueError("pixel_stats: t0 >= 0 with t0 + n <= 2^31 - 1 expected (got t0 = %r, n = %d)" % (t0, n))
    return n, h, w


def pixel_stats(images, sums=True, extremes=True):
    """Extension: statistics over time of a uint16 stack ``images[n][h][w]`` (or one ``(h, w)`` image): a ``PixelStats`` of numpy arrays
    ``[h][w]`` (``rir_pixel_stats``) - per pixel the exact sum and sum of squares (``sums``), the min, the max and the lowest image index of
    each (``extremes``).  ``ValueError`` on bad shapes or when neither group is asked for, ``RuntimeError`` on other dtypes and when the
    library fails."""
    img = np.ascontiguousarray(images)
    if img.dtype != np.uint16:
        raise RuntimeError("pixel_stats: uint16 images expected, not %s" % img.dtype)
    n, h, w = _pixel_stats_args(img.shape, sums, extremes)
    on = (sums, sums, extremes, extremes, extremes, extremes)
    out = [np.full((h, w), 0 if k < 2 else -1, dt) if g else None for k, (g, dt) in enumerate(zip(on, _PIXEL_DTYPES))]
    _call("pixel_stats", n, _sp.rir_pixel_stats, img.ctypes.data, w, h, n, *(a.ctypes.data if a is not None else None for a in out))
    return PixelStats(*out, count=n)


# ---- extension: per-pixel quantiles over time -----------------------------------------------------------------------------------
_sp.rir_pixel_quantiles.argtypes = [ct.c_void_p] + [ct.c_int] * 3 + [ct.c_void_p, ct.c_int, ct.c_void_p]


def _pixel_quantiles_args(frames_shape, what="pixel_quantiles"):
    """the shape of a pixel_quantiles call, checked without a device; -> (n, h, w)"""
    if len(frames_shape) == 2:
        frames_shape = (1,) + tuple(frames_shape)
    if len(frames_shape) != 3:
        raise ValueError("%s: frames (n, h, w) or (h, w) expected" % what)
    n, h, w = frames_shape
    if h < 1 or w < 1 or h * w >= 1 << 31 or n > (1 << 31) - 1:
        raise ValueError("%s: frames of at least 1x1 and fewer than 2^31 pixels, at most 2^31 - 1 of them, expected" % what)
    return n, h, w


def pixel_quantiles(images, percents):
    """Extension: quantiles over time of a uint16 stack ``images[n][h][w]`` (or one ``(h, w)`` image) at ``percents`` (a float or 1..8
    floats in [0, 1]): an int32 numpy array ``(len(percents), h, w)``, one image per percent (``rir_pixel_quantiles``) -
    ``pixel_quantiles(images, 0.5)[0]`` is the median image over time.  Per pixel the rule of ``region_quantiles``; -1 everywhere for no
    images.  ``ValueError`` on bad shapes or percents, ``RuntimeError`` on other dtypes and when the library fails."""
    img = np.ascontiguousarray(images)
    if img.dtype != np.uint16:
        raise RuntimeError("pixel_quantiles: uint16 images expected, not %s" % img.dtype)
    pc = _region_quantiles_percents(percents)
    n, h, w = _pixel_quantiles_args(img.shape)
    out = np.empty((pc.size, h, w), np.int32)
    _call("pixel_quantiles", True, _sp.rir_pixel_quantiles, img.ctypes.data if n else None, w, h, n, pc.ctypes.data, pc.size,
          out.ctypes.data)  # (called for no images too: it is the entry that fills in the -1)
    return out


# ---- extension: polygon label maps ----------------------------------------------------------------------------------------------
_sp.rir_polygon_map.argtypes = [ct.c_void_p] * 3 + [ct.c_int] * 4 + [ct.c_void_p] + [ct.c_int] * 3 + [ct.c_void_p]

MAX_POLYGONS = 1 << 16
MAX_POLYGON_POINTS = 1024
MAX_MAP_PIXELS = 0x7FFF0000

PolygonMapArgs = namedtuple("PolygonMapArgs", "xy npts values shifts nmaps per_map npoly max_pts h w out_shape")


def _is_polygon(e):
    """a (k, 2) array-like of points (an empty sequence: no point), as opposed to a list of polygons"""
    if hasattr(e, "ndim"):
        return e.ndim == 2 or (e.ndim == 1 and e.shape[0] == 0)
    if not isinstance(e, (list, tuple)):
        raise ValueError("polygon_map: polygons as (k, 2) array-likes expected, not %s" % type(e).__name__)
    return len(e) == 0 or np.ndim(e[0]) == 1


def _pack_polygons(sets):
    """lists of (k, 2) array-likes, one list per set -> xy float64 (nsets, npoly, max_pts, 2), npts int32 (nsets, npoly); sets with fewer
    polygons are filled up with polygons of no point"""
    arrays = []
    for s in sets:
        row = []
        for p in s:
            a = np.asarray(p, np.float64)
            if a.size == 0:
                a = a.reshape(0, 2)
            if a.ndim != 2 or a.shape[1] != 2:
                raise ValueError("polygon_map: a polygon is a (k, 2) array of (x, y), not of shape %s" % (a.shape,))
            row.append(a)
        arrays.append(row)
    npoly = max((len(r) for r in arrays), default=0)
    max_pts = max((len(a) for r in arrays for a in r), default=0)
    xy = np.zeros((len(arrays), npoly, max(1, max_pts), 2), np.float64)
    npts = np.zeros((len(arrays), npoly), np.int32)
    for s, r in enumerate(arrays):
        for p, a in enumerate(r):
            xy[s, p, :len(a)] = a
            npts[s, p] = len(a)
    return xy, npts


def _polygon_map_args(polygons, shape, values=None, background=-1, shifts=None):
    """the arguments of a polygon_map call, packed and checked without a device -> PolygonMapArgs.  ``polygons``: a list of (k, 2)
    array-likes (one set for every map), a list of such lists (one set per map), or a packed pair (xy, npts) - xy float64
    (npoly, max_pts, 2) with npts int32 (npoly,), or (n, npoly, max_pts, 2) with (n, npoly) - of numpy arrays or tensors, which is passed
    on as it is.  values and shifts come back as numpy arrays (or None)."""
    if len(shape) != 2 or int(shape[0]) != shape[0] or int(shape[1]) != shape[1] or shape[0] < 1 or shape[1] < 1 or shape[0] * shape[1] > MAX_MAP_PIXELS:
        raise ValueError("polygon_map: shape (h, w) of at least 1x1 and at most 0x7FFF0000 pixels expected, not %r" % (shape,))
    h, w = int(shape[0]), int(shape[1])
    packed = isinstance(polygons, (tuple, list)) and len(polygons) == 2 and all(hasattr(a, "ndim") and hasattr(a, "dtype") for a in polygons) and \
        polygons[0].ndim in (3, 4)
    if packed:
        xy, npts = polygons
        if "float64" not in str(xy.dtype) or "int32" not in str(npts.dtype):
            raise RuntimeError("polygon_map: packed polygons are float64 xy and int32 npts, not %s and %s" % (xy.dtype, npts.dtype))
        if xy.shape[-1] != 2 or tuple(npts.shape) != tuple(xy.shape[:-2]):
            raise ValueError("polygon_map: packed xy (n, npoly, max_pts, 2) with npts (n, npoly), or without n, expected, not %s and %s"
                             % (tuple(xy.shape), tuple(npts.shape)))
        per_map = xy.ndim == 4
    else:
        if not isinstance(polygons, (tuple, list)):
            raise ValueError("polygon_map: a list of polygons, a list of such lists or a packed (xy, npts) pair expected")
        kinds = [_is_polygon(e) for e in polygons]
        if any(kinds) and not all(kinds):
            raise ValueError("polygon_map: either polygons or lists of polygons expected, not both in one list")
        per_map = len(kinds) > 0 and not kinds[0]
        xy, npts = _pack_polygons(polygons if per_map else [polygons])
        if not per_map:
            xy, npts = xy[0], npts[0]
    nsets = xy.shape[0] if per_map else 1
    npoly, max_pts = int(xy.shape[-3]), int(xy.shape[-2])
    if npoly > MAX_POLYGONS or not 1 <= max_pts <= MAX_POLYGON_POINTS:
        raise ValueError("polygon_map: at most %d polygons of at most %d points expected (got %d of up to %d)"
                         % (MAX_POLYGONS, MAX_POLYGON_POINTS, npoly, max_pts))
    if values is not None:
        v = np.asarray(values)
        if v.shape != (npoly,) or v.dtype.kind not in "iu" or (v.size and (v.min() < -(1 << 31) or v.max() >= 1 << 31)):
            raise ValueError("polygon_map: values are %d int32, one per polygon" % npoly)
        values = np.ascontiguousarray(v, np.int32)
    if int(background) != background or not -(1 << 31) <= background < 1 << 31:
        raise ValueError("polygon_map: an int32 background expected, not %r" % (background,))
    nmaps = nsets
    if shifts is not None:
        shifts = np.ascontiguousarray(shifts.detach().cpu().numpy() if hasattr(shifts, "detach") else shifts, np.float64)
        if shifts.ndim != 2 or shifts.shape[1] != 2 or (per_map and shifts.shape[0] != nsets):
            raise ValueError("polygon_map: shifts (n, 2) expected%s, not %s" % (" with n = %d sets" % nsets if per_map else "", shifts.shape))
        nmaps = shifts.shape[0]
    out_shape = (nmaps, h, w) if per_map or shifts is not None else (h, w)
    return PolygonMapArgs(xy, npts, values, shifts, nmaps, int(per_map), npoly, max_pts, h, w, out_shape)


def polygon_map(polygons, shape, values=None, background=-1, shifts=None, out=None):
    """Extension: polygon regions of interest rasterised into int32 label maps of ``shape`` (h, w), as ``region_stats`` takes them
    (``rir_polygon_map``): the map is filled with ``background`` (-1: what region_stats ignores) and the polygons are painted in order
    with ``values`` (default 0, 1, ...), later ones over earlier ones, exactly as the reference's ``draw_polygon`` paints each.
    ``polygons``: a list of (k, 2) arrays of (x, y) - one point draws a pixel, two a line - or a list of such lists, one per map, or a
    packed ``(xy, npts)`` pair; ``shifts`` (n, 2): map m is drawn with every vertex moved by (dx, dy) = shifts[m].  -> a numpy array
    (h, w) for one set without shifts, else (n, h, w).  A polygon with a coordinate that is not finite or beyond 2^24 draws nothing.
    ``ValueError`` on bad shapes, ``RuntimeError`` on other dtypes and when the library fails."""
    a = _polygon_map_args(polygons, shape, values, background, shifts)
    xy, npts = (np.ascontiguousarray(t.cpu().numpy() if hasattr(t, "cpu") else t) for t in (a.xy, a.npts))
    if out is None:
        out = np.empty(a.out_shape, np.int32)
    elif not isinstance(out, np.ndarray) or out.dtype != np.int32 or out.shape != a.out_shape or not out.flags.c_contiguous:
        raise RuntimeError("polygon_map: out must be a contiguous int32 array of shape %s" % (a.out_shape,))
    _call("polygon_map", a.nmaps, _sp.rir_polygon_map, xy.ctypes.data if a.npoly else None, npts.ctypes.data if a.npoly else None,
          a.values.ctypes.data if a.values is not None and a.npoly else None, a.npoly, a.max_pts, a.nmaps, a.per_map,
          a.shifts.ctypes.data if a.shifts is not None else None, a.w, a.h, int(background), out.ctypes.data)
    return out


# ---- time axes (host bookkeeping, csrc/time_series.cpp) -------------------------------------------------------------------------
_sp.extract_times.argtypes = [ct.c_void_p, ct.c_int, ct.c_void_p, ct.c_int, ct.c_void_p, ct.POINTER(ct.c_int)]
_sp.resample_time_serie.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_int, ct.c_void_p, ct.c_int, ct.c_int, ct.c_double, ct.c_void_p, ct.POINTER(ct.c_int)]
_sp.label_image.argtypes = [ct.c_int, ct.c_void_p, ct.c_void_p, ct.c_int, ct.c_int, ct.c_void_p, ct.c_void_p, ct.c_void_p]
_sp.keep_largest_area.argtypes = [ct.c_int, ct.c_void_p, ct.c_void_p, ct.c_int, ct.c_int, ct.c_void_p, ct.c_int]


def extract_times(time_series, strategy="union"):
    """
    One time axis out of several (same call as reference rir_signal_processing.py:150-207): ``time_series`` is a list of time vectors,
    ``strategy`` says which span the result covers - 'union': from the earliest to the latest sample of any series, 'inter': only the span
    all of them share.  The result is increasing and holds every distinct sample time of the inputs inside that span once.

    Where the reference never returns (an empty series, a NaN at either end of one or two NaN in one, a series with no sample inside the
    common range of 'inter') the library refuses and this raises RuntimeError.
    """
    if len(time_series) == 0:
        raise RuntimeError("extract_times: NULL size")
    if strategy != "union" and strategy != "inter":
        raise RuntimeError("extract_times: wrong strategy")
    series = [np.array(t, dtype=np.float64).ravel() for t in time_series]
    times = np.ascontiguousarray(np.concatenate(series + [np.zeros(1)]))  # (one spare element: never an empty buffer)
    sizes = np.array([t.size for t in series], dtype=np.int32)
    outsize = ct.c_int(int(sizes.sum()))
    out = np.zeros(max(outsize.value, 1), dtype=np.float64)
    s = 1 if strategy == "inter" else 0
    tmp = _sp.extract_times(times.ctypes.data, len(series), sizes.ctypes.data, s, out.ctypes.data, ct.byref(outsize))
    if tmp == -2:
        out = np.zeros(outsize.value, dtype=np.float64)
        tmp = _sp.extract_times(times.ctypes.data, len(series), sizes.ctypes.data, s, out.ctypes.data, ct.byref(outsize))
    if tmp != 0:
        raise RuntimeError(last_error() or "extract_times: unknown error")
    return out[0:outsize.value]


def resample_time_serie(x, y, time_vector, padd=None, interp=True):
    """
    The series (``x`` sample times, ``y`` values) read off at the times of ``time_vector`` (same call as reference
    rir_signal_processing.py:210-270).  ``interp`` true: linear interpolation between the two samples around each new time, false: the value of
    the nearer of the two.  New times outside the series get ``padd`` when it is given, the first / last value otherwise.  Returns the values.

    (The reference gives the library room for 2 * len(x) values and raises "unknown error" for a longer time_vector; here the room is
    the time vector's length.)
    """
    if len(x) != len(y) or len(x) == 0:
        raise RuntimeError("resample_time_serie: wrong input serie size")
    if len(time_vector) == 0:
        raise RuntimeError("resample_time_serie: wrong time vector size")
    x = np.ascontiguousarray(np.array(x, dtype=np.float64).ravel())
    y = np.ascontiguousarray(np.array(y, dtype=np.float64).ravel())
    time_vector = np.ascontiguousarray(np.array(time_vector, dtype=np.float64).ravel())
    s = 0
    if padd is not None:
        s |= 2
    if bool(interp):
        s |= 4
    padd = 0.0 if padd is None else float(padd)
    outsize = ct.c_int(max(2 * x.size, time_vector.size))
    out = np.zeros(outsize.value, dtype=np.float64)
    tmp = _sp.resample_time_serie(x.ctypes.data, y.ctypes.data, x.size, time_vector.ctypes.data, time_vector.size, s, padd, out.ctypes.data,
                                  ct.byref(outsize))
    if tmp != 0:
        raise RuntimeError(last_error() or "resample_time_serie: unknown error")
    return out[0:outsize.value]


# ---- connected components (csrc/label_kernels.hip) ------------------------------------------------------------------------------
def _labelling_input(image, background_value, name):
    if not isinstance(image, np.ndarray) or len(image.shape) != 2:
        raise RuntimeError("%s: wrong input image dimension" % name)
    dt = _DTYPES.get(image.dtype, None)
    if dt is None:
        raise RuntimeError("An error occured while calling '%s'" % name)
    img = np.ascontiguousarray(image)
    background = np.zeros(1, dtype=image.dtype)
    background[0] = background_value
    return img, background, dt


def label_image(image: np.ndarray, background_value=0):
    """
    Connected components of ``image`` (same call as reference rir_signal_processing.py:319-370): -> (labels int32 of the image's shape, areas,
    first_points); entry ``k`` of the two tables belongs to label ``k``, entry 0 to the background (nothing useful in it).

    Pixels differing from background_value form the components; vertical neighbours are joined whatever their values, horizontal
    neighbours when their values are equal (as upstream); labels follow the raster order of the components' first pixels.  As upstream,
    both columns of first_points hold the first pixel's x.
    """
    img, background, dt = _labelling_input(image, background_value, "label_image")
    res = np.empty(img.shape, dtype=np.int32)
    areas = np.empty(img.size + 1, dtype=np.int32)  # (the reference allocates img.size entries: one short when every pixel of a row
    xy = np.empty((img.size + 1, 2), dtype=np.float64)  # image is its own component)
    r = _sp.label_image(ord(dt), img.ctypes.data, res.ctypes.data, img.shape[1], img.shape[0], background.ctypes.data, xy.ctypes.data,
                        areas.ctypes.data)
    if r < 0:
        raise RuntimeError("An error occured while calling 'label_image'")
    return (res, areas[0:r], xy[0:r])


def keep_largest_area(image, background_value=0, foreground_value=1):
    """
    int32 image with ``foreground_value`` on the component of ``image`` that has the most pixels and ``background_value`` everywhere else (same
    call as reference rir_signal_processing.py:373-415; among equals the component met first in raster order wins).
    """
    img, background, dt = _labelling_input(image, background_value, "keep_largest_area")
    res = np.empty(img.shape, dtype=np.int32)
    r = _sp.keep_largest_area(ord(dt), img.ctypes.data, res.ctypes.data, img.shape[1], img.shape[0], background.ctypes.data, int(foreground_value))
    if r < 0:
        raise RuntimeError("An error occured while calling 'keep_largest_area'")
    return res
