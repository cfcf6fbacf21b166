"""Spatial rank filters: the plain-numpy reference the tests compare with, the test images and the list of small cases.  No test functions."""
import zlib
from collections import namedtuple

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

from morphology_cases import DTYPES, border_image, constant_image, random_image, type_max


def reference_image(img, rank, size_y, size_x):
    """one unsigned 2-D image, every row part of it: the image padded by replicating its border pixels, every full window sorted, the element
    of 0-based rank `rank` taken"""
    ry, rx = size_y // 2, size_x // 2
    windows = sliding_window_view(np.pad(img, ((ry, ry), (rx, rx)), mode="edge"), (size_y, size_x))
    return np.sort(windows.reshape(img.shape + (size_y * size_x,)), axis=-1)[..., rank]


def reference(stack, rank, size_y, size_x, rows=None):
    """the definition: per frame, the image is the first `rows` rows; the other rows are copied.  A negative rank counts from the end."""
    stack = np.asarray(stack)
    n, h, w = stack.shape
    rows = h if rows is None else rows
    rank = rank + size_y * size_x if rank < 0 else rank
    work = stack.view(np.uint8) if stack.dtype == np.bool_ else stack
    out = work.copy()
    if rows > 0:
        for i in range(n):
            out[i, :rows] = reference_image(work[i, :rows], rank, size_y, size_x)
    return out.view(stack.dtype)


# ---- test images -----------------------------------------------------------------------------------------------------------------------
def full_range_image(rng, h, w, dtype):
    """random over the full range, with 0 and the type's maximum present (where the image has two pixels)"""
    img = random_image(rng, h, w, dtype)
    flat = img.reshape(-1)
    if flat.size >= 2:
        at = rng.choice(flat.size, 2, replace=False)
        flat[at[0]], flat[at[1]] = 0, type_max(dtype)
    return img


def three_level_image(rng, h, w, dtype):
    """values drawn from three levels only (two for bool): every window is full of ties, where a counting select is off by one"""
    top = type_max(dtype)
    levels = np.array([0, 1] if top == 1 else [top // 3, top // 3 + 1, top]).astype(dtype)
    return levels[rng.integers(0, len(levels), (h, w))]


PATTERNS = (full_range_image, three_level_image, border_image, constant_image)


def make_stack(case):
    """the frames of a case: full-range, three-level, border, constant, ... in turn, starting with a pattern that depends on the case (a
    single frame is never the constant one)"""
    seed = zlib.crc32(repr(tuple(case)).encode())
    rng = np.random.default_rng(seed)
    dtype = DTYPES[case.dtype]
    return np.stack([PATTERNS[(seed % 3 + i) % 4](rng, case.h, case.w, dtype) for i in range(case.n)])


# ---- the small cases ---------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "dtype h w n size_y size_x rank")


def case_id(c):
    return "%s-%dx%dx%d-%dx%d-r%d" % (c.dtype, c.n, c.h, c.w, c.size_y, c.size_x, c.rank)


def _register_cases():
    """the medians of 3x3 and 5x5 on even widths (the two-columns-per-lane kernels: one per pixel type and size).  130 columns: two wave
    tiles (124 outputs per wave); 67 rows: two workgroups at 3x3 (64 rows each), three at 5x5 (32 rows each); 17 x 2 and 1 x 2: narrower
    than the halo, every neighbour a replicated pixel; 250: three wave tiles"""
    shapes = [(67, 130), (17, 64), (3, 130), (1, 64), (17, 2), (1, 2), (17, 250)]
    out = []
    k = 0
    for size in (3, 5):
        for h, w in shapes:
            for dtype in ("uint16", "uint8", "bool"):
                out.append(Case(dtype, h, w, 1 + k % 3, size, size, size * size // 2))
                k += 1
    return out


def _tile_cases():
    """every other size and rank, and the squares 3 and 5 at non-median ranks and on odd widths (the LDS tile kernel: 64 x 32 outputs per
    workgroup, 8 rows per thread, the region's columns 64 and up in a dword of their own).  83 and 65 columns: two tiles, the second one ragged; 67 rows: three tiles; 1 x 1: a 15 x 15
    window is one pixel replicated 225 times"""
    sizes = [(1, 1), (1, 5), (7, 3), (3, 9), (9, 9), (15, 15), (15, 1), (3, 3), (5, 5)]
    shapes = [(17, 83), (67, 65), (3, 63), (1, 5), (17, 1), (1, 1)]
    dtypes = ("uint16", "uint8", "bool")
    out = []
    k = 0
    for size_y, size_x in sizes:
        cells = size_y * size_x
        ranks = sorted({r for r in (1, cells // 2 - 1, cells // 2, cells - 2) if 0 <= r < cells}) or [0]
        for rank in ranks:
            for j in range(2):  # two shapes and types per (size, rank); all six shapes and three types per size
                h, w = shapes[k % len(shapes)]
                out.append(Case(dtypes[(k // len(shapes) + k) % len(dtypes)], h, w, 1 + k % 3, size_y, size_x, rank))
                k += 1
    # the medians of 3x3 and 5x5 where the pair kernels do not apply: odd widths
    out += [Case("uint16", 17, 83, 2, 3, 3, 4), Case("uint8", 67, 65, 1, 5, 5, 12), Case("bool", 3, 63, 3, 3, 3, 4), Case("uint16", 17, 1, 1, 5, 5, 12)]
    # the largest window on the smallest images, and on more than one tile each way
    out += [Case("uint16", 1, 1, 2, 15, 15, 112), Case("uint8", 1, 5, 1, 15, 15, 1), Case("uint16", 17, 1, 1, 15, 15, 223),
            Case("uint16", 67, 65, 1, 15, 15, 112), Case("uint8", 17, 83, 2, 9, 9, 40)]
    return out


REGISTER_CASES = _register_cases()
TILE_CASES = _tile_cases()
CASES = REGISTER_CASES + TILE_CASES
