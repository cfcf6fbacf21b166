"""Local window statistics: the plain-numpy reference the tests compare with, the test images and the case lists.  No test functions."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

from morphology_cases import type_max

K_NUM_MAX, K_DEN_MAX, DELTA_MAX = 255, 64, 65535  # the limits of local_threshold's parameters
INT64_MAX = (1 << 63) - 1
POLARITIES = ("above", "below", "both")


def sizes_of(size):
    return (size, size) if isinstance(size, int) else tuple(size)


def reference_sums(stack, size_y, size_x, rows=None, power=1):
    """int64 [n][h][w]: per frame, the image is the first `rows` rows, padded by replicating its border pixels; the sum of v ** power over
    every full window.  0 in the rows below the image."""
    stack = np.asarray(stack)
    n, h, w = stack.shape
    rows = h if rows is None else rows
    out = np.zeros((n, h, w), np.int64)
    if rows > 0 and n > 0:
        ry, rx = size_y // 2, size_x // 2
        image = stack[:, :rows].astype(np.int64) ** power
        padded = np.pad(image, ((0, 0), (ry, ry), (rx, rx)), mode="edge")
        out[:, :rows] = sliding_window_view(padded, (size_y, size_x), axis=(1, 2)).sum(axis=(3, 4), dtype=np.int64)
    return out


def reference_mean(stack, size_y, size_x, rows=None):
    """(S + n // 2) // n in the input's type in the image, the input below it"""
    stack = np.asarray(stack)
    rows = stack.shape[1] if rows is None else rows
    n = size_y * size_x
    out = stack.copy()
    out[:, :rows] = ((reference_sums(stack, size_y, size_x, rows)[:, :rows] + n // 2) // n).astype(stack.dtype)
    return out


def as_rational(k):
    return (int(k[0]), int(k[1])) if isinstance(k, (tuple, list)) else (int(k), 1)


def reference_mask(stack, size_y, size_x, k, delta=0, polarity="above", rows=None, exact=False):
    """bool [n][h][w]: the rule of rir_local_threshold_device, term by term, in int64 - or, with `exact`, in Python integers (object arrays), so
    that the reference itself cannot wrap where the products come near 2^63"""
    stack = np.asarray(stack)
    rows = stack.shape[1] if rows is None else rows
    n = size_y * size_x
    num, den = as_rational(k)
    wide = (lambda a: a.astype(object)) if exact else (lambda a: a)
    S = wide(reference_sums(stack, size_y, size_x, rows))
    Q = wide(reference_sums(stack, size_y, size_x, rows, power=2))
    v = wide(stack.astype(np.int64))
    d = n * v - S
    V = n * Q - S * S
    far = d * d * (den * den) > (num * num) * V
    up, down = d > delta * n, -d > delta * n
    side = up if polarity == "above" else down if polarity == "below" else (up | down)
    out = np.asarray(far & side, dtype=bool)
    out[:, rows:] = False
    return out


def largest_products(stack, size_y, size_x, k_den, k_num):
    """(the largest d^2 k_den^2, the largest k_num^2 V) over a stack, in Python integers: what the kernel's comparison has to hold"""
    n = size_y * size_x
    S = reference_sums(stack, size_y, size_x).astype(object)
    Q = reference_sums(stack, size_y, size_x, power=2).astype(object)
    d = n * np.asarray(stack).astype(np.int64).astype(object) - S
    V = n * Q - S * S
    assert (V >= 0).all()
    return int((d * d).max()) * k_den * k_den, int(V.max()) * k_num * k_num


# ---- test images -----------------------------------------------------------------------------------------------------------------------
def checkerboard(h, w, dtype, phase=0):
    """0 / the type's maximum, alternating both ways: the window with the largest variance"""
    yy, xx = np.mgrid[0:h, 0:w]
    return (((yy + xx + phase) & 1) * type_max(dtype)).astype(dtype)


def ramp(h, w, dtype):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((yy * 37 + xx * 101) % (type_max(dtype) + 1)).astype(dtype)


def noise(rng, h, w, dtype, spread=None):
    """a level with noise around it (the full range for bool), the noise level rising from left to right"""
    top = type_max(dtype)
    if top == 1:
        return rng.integers(0, 2, (h, w)).astype(dtype)
    spread = top // 16 if spread is None else spread
    sigma = np.linspace(1, spread, w)[None, :]
    return np.clip(np.rint(top // 2 + rng.standard_normal((h, w)) * sigma), 0, top).astype(dtype)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
# 64, 130: one and two wave tiles of the pair kernel (112 outputs per wave) at even widths; 65, 11: the general kernel; 67 rows: two
# workgroups (64 rows each); 3 rows and (5, 6) at 15: windows larger than the image; (1, 1): one pixel replicated n times
SHAPES = [(17, 64), (17, 130), (17, 65), (9, 11), (3, 64), (67, 130), (1, 1)]
SIZES = [1, 3, 5, 7, 9, 15, (7, 3), (3, 9), (1, 15), (15, 1)]
DTYPES = ["uint16", "uint8", "bool"]
OUTPUTS = [dict(sum=True, sumsq=False, mean=False), dict(sum=True, sumsq=True, mean=False), dict(sum=False, sumsq=False, mean=True),
           dict(sum=True, sumsq=True, mean=True)]
KS = [0, 1, 3, (5, 2), (255, 64), (255, 1)]
DELTAS = [0, 1, -1, 20, 65535, -65535]
