"""Flat morphology: the plain-numpy reference the tests compare with, the test images and the list of small cases.  No test functions."""
import zlib
from collections import namedtuple

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

OPS = ("erode", "dilate", "open", "close", "tophat", "blackhat", "gradient")
DTYPES = {"uint16": np.uint16, "uint8": np.uint8, "bool": np.bool_}


def type_max(dtype):
    return 1 if np.dtype(dtype) == np.bool_ else int(np.iinfo(dtype).max)


def _stage(img, take_max, size_y, size_x):
    """min / max of an unsigned 2-D image over the size_y x size_x window clipped to the image: the image is padded with the value that is
    neutral for the stage (the type's maximum for a min, 0 for a max), so the padding never wins"""
    ry, rx = size_y // 2, size_x // 2
    padded = np.pad(img, ((ry, ry), (rx, rx)), constant_values=0 if take_max else type_max(img.dtype))
    windows = sliding_window_view(padded, (size_y, size_x))
    return windows.max(axis=(2, 3)) if take_max else windows.min(axis=(2, 3))


def reference_image(img, op, size_y, size_x):
    """one unsigned image, every row part of it, stage by stage"""
    erode = lambda f: _stage(f, False, size_y, size_x)  # noqa: E731
    dilate = lambda f: _stage(f, True, size_y, size_x)  # noqa: E731
    if op == "erode":
        return erode(img)
    if op == "dilate":
        return dilate(img)
    if op == "open":
        return dilate(erode(img))
    if op == "close":
        return erode(dilate(img))
    if op == "tophat":
        return img - dilate(erode(img))
    if op == "blackhat":
        return erode(dilate(img)) - img
    if op == "gradient":
        return dilate(img) - erode(img)
    raise ValueError(op)


def reference(stack, op, size_y, size_x, rows=None):
    """the definition: per frame, the image is the first `rows` rows; the other rows are copied"""
    stack = np.asarray(stack)
    n, h, w = stack.shape
    rows = h if rows is None else rows
    work = stack.view(np.uint8) if stack.dtype == np.bool_ else stack
    out = work.copy()
    if rows > 0:
        for i in range(n):
            out[i, :rows] = reference_image(work[i, :rows], op, size_y, size_x)
    return out.view(stack.dtype)


# ---- test images -----------------------------------------------------------------------------------------------------------------------
def random_image(rng, h, w, dtype):
    return rng.integers(0, type_max(dtype) + 1, (h, w)).astype(dtype)


def constant_image(rng, h, w, dtype):
    return np.full((h, w), rng.integers(0, type_max(dtype) + 1)).astype(dtype)


def border_image(rng, h, w, dtype):
    """random inside; 0 and the type's maximum along the borders and at the four corners - what a second stage that sees first-stage values
    outside the image gets wrong"""
    top = type_max(dtype)
    img = random_image(rng, h, w, dtype)
    img[0, :], img[-1, :] = top, 0
    img[:, 0], img[:, -1] = 0, top
    img[0, 0], img[0, -1], img[-1, 0], img[-1, -1] = 0, top, top, 0
    return img


def spike_images(h, w, dtype):
    """18 images: one extreme pixel - the type's maximum in a flat low image, then 0 in a flat high image - at each of the nine positions
    corner / edge / interior"""
    top = type_max(dtype)
    low, high = (0, top) if top == 1 else (top // 4, top - top // 4)
    ys, xs = sorted({0, h // 2, h - 1}), sorted({0, w // 2, w - 1})
    frames = []
    for flat, spike in ((low, top), (high, 0)):
        for y in ys:
            for x in xs:
                img = np.full((h, w), flat).astype(dtype)
                img[y, x] = spike
                frames.append(img)
    return np.stack(frames)


PATTERNS = (random_image, border_image, constant_image)


def make_stack(case):
    """the frames of a case: random, border, constant, ... in turn, starting with a pattern that depends on the case"""
    seed = zlib.crc32(repr(tuple(case)).encode())
    rng = np.random.default_rng(seed)
    dtype = DTYPES[case.dtype]
    return np.stack([PATTERNS[(seed + i) % (3 if case.n > 1 else 2)](rng, case.h, case.w, dtype) for i in range(case.n)])


# ---- the small cases ---------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "dtype h w n size_y size_x op")


def case_id(c):
    return "%s-%dx%dx%d-%dx%d-%s" % (c.dtype, c.n, c.h, c.w, c.size_y, c.size_x, c.op)


def _cases():
    out = []
    # the squares 3, 5, 7 on even widths (the two-columns-per-lane kernels: one per type, size and op).  130 columns: two wave tiles,
    # whatever the halo (124, 120 or 116 outputs per wave); 64: one tile; 67 rows: two workgroups.  (six shapes against seven ops: every
    # kernel meets another shape than its neighbours)
    shapes = [(67, 130), (17, 64), (3, 130), (1, 64), (67, 64), (17, 130)]
    k = 0
    for dtype in ("uint16", "uint8", "bool"):
        for size in (3, 5, 7):
            for op in OPS:
                h, w = shapes[k % len(shapes)]
                out.append(Case(dtype, h, w, 1 + k % 3, size, size, op))
                k += 1
    # an image narrower than a halo, and three wave tiles
    out += [Case("uint16", 17, 2, 2, 3, 3, "open"), Case("uint16", 3, 2, 1, 7, 7, "erode"), Case("uint8", 17, 2, 3, 5, 5, "close"),
            Case("bool", 1, 2, 1, 3, 3, "gradient"), Case("uint16", 17, 250, 1, 7, 7, "tophat"), Case("uint8", 3, 250, 2, 3, 3, "blackhat")]
    # every other size, and the squares on odd widths (the LDS tile kernel: 64 x 32 outputs per workgroup)
    sizes = [(1, 1), (1, 5), (7, 3), (3, 9), (15, 15), (15, 1), (9, 9), (3, 3), (5, 5), (7, 7), (9, 5)]
    shapes = [(17, 83), (67, 65), (3, 63), (1, 5), (17, 1), (67, 83), (3, 5), (17, 130), (67, 63), (1, 1), (3, 65)]
    dtypes = ("uint16", "uint8", "bool", "uint16")
    k = 0
    for size_y, size_x in sizes:
        for op in OPS:
            h, w = shapes[k % len(shapes)]
            if size_y == size_x and 3 <= size_y <= 7 and w % 2 == 0:
                w += 1
            out.append(Case(dtypes[k % len(dtypes)], h, w, 1 + k % 3, size_y, size_x, op))
            k += 1
    return out


CASES = _cases()
