"""What the reconstruction tests share (no tests here): the numpy reference - the plain iteration to the fixed point with scipy's maximum /
minimum filters -, an independent brute force of the path definition for tiny images, the image makers and the case list.

The kernel converges tiles of 64 x 32 pixels (w x h) in LDS, so the shapes are: 1x1, 1x5, 17x1, 3x2 (narrower than a halo), 17x64 (one tile,
full width), 17x65 (one pixel past a tile edge in x), 33x66 (one past in y, two past in x), 67x130 and 67x83 (3 x 3 and 3 x 2 tiles, the
last ones 3 rows and 2 / 19 columns wide, an odd width)."""
import itertools
from collections import namedtuple

import numpy as np

TOP = {"uint16": 65535, "uint8": 255, "bool": 1}
TYPES = ("uint16", "uint8", "bool")
METHODS = ("dilation", "erosion")
MARKER, SHIFT, BORDER = 0, 1, 2
SHAPES = [(1, 1), (1, 5), (17, 1), (3, 2), (17, 64), (17, 65), (33, 66), (67, 130), (67, 83)]  # (h, w)


def footprint(connectivity):
    return np.ones((3, 3), bool) if connectivity == 8 else np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], bool)


def as_int(a):
    return (a.view(np.uint8) if a.dtype == np.bool_ else a).astype(np.int64)


def reference_image(marker, mask, method="dilation", connectivity=8):
    """(R, iterations) of one image: int64 arrays in, the plain iteration F <- min(G, max of F over N) (or its dual) until nothing changes;
    mode="nearest" replicates the border, which for a maximum / minimum is the window clipped to the image"""
    import scipy.ndimage as ndi

    fp = footprint(connectivity)
    g = mask.astype(np.int64)
    f = np.maximum(marker, g) if method == "erosion" else np.minimum(marker, g)
    k = 0
    while True:
        if method == "erosion":
            nxt = np.maximum(g, ndi.minimum_filter(f, footprint=fp, mode="nearest"))
        else:
            nxt = np.minimum(g, ndi.maximum_filter(f, footprint=fp, mode="nearest"))
        if np.array_equal(nxt, f):
            return f, k
        f, k = nxt, k + 1


def marker_of(mask, method, mode, param, top):
    """the marker of modes SHIFT and BORDER for an int64 image"""
    if mode == SHIFT:
        return np.minimum(mask + param, top) if method == "erosion" else np.maximum(mask - param, 0)
    m = np.full_like(mask, top if method == "erosion" else 0)
    m[0, :], m[-1, :], m[:, 0], m[:, -1] = mask[0, :], mask[-1, :], mask[:, 0], mask[:, -1]
    return m


def reference(mask, marker=None, method="dilation", connectivity=8, mode=MARKER, param=0, output=0, rows=None, iterations=None):
    """the definition of rir_reconstruct_device over a stack [n][h][w] (or an image); `iterations`: a list that receives each frame's count"""
    stack = mask.reshape((-1,) + mask.shape[-2:])
    seeds = None if marker is None else marker.reshape(stack.shape)
    top = TOP[mask.dtype.name]
    rows = stack.shape[1] if rows is None else rows
    out = as_int(stack).copy()
    for i in range(stack.shape[0]):
        if rows == 0:
            continue
        g = as_int(stack[i, :rows])
        f = as_int(seeds[i, :rows]) if mode == MARKER else marker_of(g, method, mode, param, top)
        r, k = reference_image(f, g, method, connectivity)
        if iterations is not None:
            iterations.append(k)
        out[i, :rows] = r if not output else (r - g if method == "erosion" else g - r)
    assert out.min() >= 0 and out.max() <= top
    return out.astype(np.uint8 if mask.dtype == np.bool_ else mask.dtype).view(mask.dtype).reshape(mask.shape)


def brute_force_image(marker, mask, method="dilation", connectivity=8):
    """The path definition on a tiny int64 image: B[q][p] = the best, over the connected paths from q to p, of the lowest mask value on the
    path (both ends included), by a Floyd-Warshall relaxation over all pixels; R(p) = max over q of min(F0(q), B[q][p]).  Erosion is
    dilation of the negated images."""
    if method == "erosion":
        return -brute_force_image(-marker, -mask, "dilation", connectivity)
    h, w = mask.shape
    n = h * w
    g = mask.ravel().astype(np.int64)
    none = g.min() - 1
    B = np.full((n, n), none, np.int64)
    for y in range(h):
        for x in range(w):
            p = y * w + x
            B[p, p] = g[p]
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if (dy or dx) and (connectivity == 8 or not (dy and dx)) and 0 <= y + dy < h and 0 <= x + dx < w:
                        q = (y + dy) * w + x + dx
                        B[p, q] = min(g[p], g[q])
    for k in range(n):
        B = np.maximum(B, np.minimum(B[:, k, None], B[None, k, :]))
    f0 = np.minimum(marker.ravel().astype(np.int64), g)
    return np.minimum(f0[:, None], B).max(axis=0).reshape(h, w)


# ---- image makers ---------------------------------------------------------------------------------------------------------------------------
def levels_image(rng, h, w, dtype_name, nlevels=6):
    """a few grey levels in patches, 0 and the type's maximum among them: plateaus that a value can travel along"""
    top = TOP[dtype_name]
    if dtype_name == "bool":
        img = rng.random((h, w)) < 0.62
    else:
        levels = np.unique(np.concatenate([[0, top], rng.integers(0, top + 1, nlevels)]))
        img = levels[rng.integers(0, len(levels), (h, w))].astype(dtype_name)
    if h * w > 2:  # both ends of the range, wherever the draw left them out
        at = rng.choice(h * w, 2, replace=False)
        img.flat[at[0]], img.flat[at[1]] = 0, top
    return img


def marker_image(rng, mask, density=0.08):
    """a sparse marker: mostly the far end (0; the type's maximum for erosion is made by the caller), some pixels at or ABOVE the mask"""
    top = TOP[mask.dtype.name]
    if mask.dtype == np.bool_:
        return rng.random(mask.shape) < density  # (some of them outside the mask: clamped)
    m = np.zeros(mask.shape, np.int64)
    pick = rng.random(mask.shape) < density
    m[pick] = rng.integers(0, top + 1, int(pick.sum()))
    m.flat[0] = top
    return m.astype(mask.dtype)


def serpentine(h, w, dtype=np.uint16, level=1000, gap=2):
    """rows of mask joined alternately at the right and the left end: one corridor whose length is about h * w / gap"""
    m = np.zeros((h, w), dtype)
    for y in range(0, h, gap):
        m[y, :] = level
        if y + gap < h:
            m[y:y + gap, w - 1 if (y // gap) % 2 == 0 else 0] = level
    return m


def spiral(h, w, dtype=np.uint16, level=1000):
    """a one-pixel corridor that winds inwards from (0, 0), clockwise, one pixel of 0 between its turns"""
    m = np.zeros((h, w), dtype)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = level
    while True:
        for _ in range(2):  # straight on, or one turn to the right
            ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if 0 <= ny < h and 0 <= nx < w and not m[ny, nx] and not (0 <= ay < h and 0 <= ax < w and m[ay, ax]):
                y, x = ny, nx
                m[y, x] = level
                break
            dy, dx = dx, -dy
        else:
            return m


def diagonal(h, w, dtype=np.uint16, level=1000):
    """a one-pixel diagonal corridor from (0, 0): connected at connectivity 8 only"""
    m = np.zeros((h, w), dtype)
    k = np.arange(min(h, w))
    m[k, k] = level
    return m


def blobs_and_noise(h=512, w=640, seed=1):
    """the full-size scene of the issue: smooth blobs on a level of 3 000 plus noise of sigma 20"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w]
    f = 3000 + 1500 * np.exp(-((yy - 0.39 * h) ** 2 + (xx - 0.47 * w) ** 2) / 5000.0) + 800 * np.exp(-((yy - 0.78 * h) ** 2 + (xx - 0.16 * w) ** 2) / 300.0)
    return (f + rng.normal(0, 20, (h, w))).astype(np.uint16)


# ---- the small cases ------------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "dtype h w n method connectivity mode param seed")


def case_id(c):
    return "%s-%dx%d-%s%d-mode%d-p%d" % (c.dtype, c.h, c.w, c.method[:3], c.connectivity, c.mode, c.param)


def _cases():
    out = []
    for i, (dtype, method, conn) in enumerate(itertools.product(TYPES, METHODS, (8, 4))):
        top = TOP[dtype]
        for j in range(3):  # three of the nine shapes for every type x method x connectivity, every shape four times in all
            h, w = SHAPES[(i * 3 + j * 4) % 9]
            mode = (i + j) % 3
            param = (0, 1, top // 5, top)[(i + j) % 4] if mode == SHIFT else 0
            out.append(Case(dtype, h, w, 2, method, conn, mode, min(param, top), 100 * i + j))
    return out


CASES = _cases()


def make_case(c):
    """-> (mask stack, marker stack or None)"""
    rng = np.random.default_rng(c.seed)
    mask = np.stack([levels_image(rng, c.h, c.w, c.dtype) for _ in range(c.n)])
    if c.mode != MARKER:
        return mask, None
    marker = np.stack([marker_image(rng, mask[i]) for i in range(c.n)])
    if c.method == "erosion":  # the far end is the type's maximum
        marker = (~marker) if c.dtype == "bool" else (TOP[c.dtype] - marker).astype(mask.dtype)
    return mask, marker
