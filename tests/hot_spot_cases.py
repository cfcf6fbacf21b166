"""Helper of the hot-spot labelling tests (not a test module): the numpy oracle of rir_label_hot_spots_device - a union-find over the
foreground pixels in which a root is its component's first pixel in raster order, then the predicates of a kept component, then the
numbers as a cumulative count over the kept roots in raster order - and the scenes.  It restates the contract of
include/rir_amd_device.h and needs nothing but numpy."""
import numpy as np

TILE_W, TILE_H = 64, 32  # the tile of the first launch (label_kernels.hip): a component in more than one tile is joined across a tile border

RANDOM_SHAPES = [(2, 70, 130), (3, 33, 65), (2, 5, 9), (1, 1, 1), (2, 32, 64), (2, 64, 128), (1, 3, 1025)]
RANDOM_LOW = 29490
# each predicate on its own, and the four together
RANDOM_FILTERS = [dict(high=64000), dict(min_area=5), dict(max_area=40), dict(clear_border=True),
                  dict(high=64000, min_area=5, max_area=400, clear_border=True)]


def random_frames(shape):
    return np.random.default_rng(5).integers(0, 65536, shape).astype(np.uint16)


def roots_of(mask):
    """int64 (h, w): the raster index of the first pixel of every foreground pixel's 4-connected component, -1 on the background"""
    h, w = mask.shape
    parent = np.arange(h * w)
    idx = np.arange(h * w).reshape(h, w)

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    side = mask[:, 1:] & mask[:, :-1]
    above = mask[1:] & mask[:-1]
    pairs = np.concatenate([np.stack([idx[:, 1:][side], idx[:, :-1][side]], 1), np.stack([idx[1:][above], idx[:-1][above]], 1)])
    for a, b in pairs.tolist():
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)  # the lower root stays: a root is the lowest index of its tree
    out = np.full(h * w, -1, np.int64)
    for i in np.flatnonzero(mask.reshape(-1)).tolist():
        out[i] = find(i)
    return out.reshape(h, w)


def threshold_map(t, h, w):
    """an int, a float or an (h, w) array of either, compared as it is: v > t is the definition, whatever t's type"""
    return np.broadcast_to(np.asarray(t), (h, w))


def oracle(frames, low, high=None, min_area=1, max_area=None, clear_border=False, rows=None, table_entries=None):
    """what label_hot_spots returns, as numpy arrays, and what it rests on: `roots` (n, h, w), `kept` (n, h * w) bool per root index, `mask`
    (the kept pixels).  low / high: a number or an (h, w) array."""
    frames = np.asarray(frames)
    assert frames.dtype == np.uint16
    if frames.ndim == 2:
        frames = frames[None]
    n, h, w = frames.shape
    rows = h if rows is None else rows
    cap = min(1024, h * w + 1) if table_entries is None else table_entries
    v = frames.astype(np.int64)
    y, x = np.mgrid[0:h, 0:w]
    fg = (v > threshold_map(low, h, w)) & (y < rows)
    on_edge = (y == 0) | (y == rows - 1) | (x == 0) | (x == w - 1)
    labels = np.zeros((n, h, w), np.int32)
    area = np.zeros((n, cap), np.int32)
    first = np.zeros((n, cap), np.int32)
    counts = np.zeros(n, np.int32)
    roots = np.zeros((n, h, w), np.int64)
    kept = np.zeros((n, h * w), bool)
    for f in range(n):
        r = roots[f] = roots_of(fg[f])
        px = r[fg[f]]
        size = np.bincount(px, minlength=h * w)
        keep = (size >= min_area) & (size > 0)
        if max_area is not None:
            keep &= size <= max_area
        if high is not None:
            strong = fg[f] & (v[f] > threshold_map(high, h, w))
            keep &= np.bincount(r[strong], minlength=h * w) > 0
        if clear_border:
            keep &= np.bincount(r[fg[f] & on_edge], minlength=h * w) == 0
        kept[f] = keep
        number = np.cumsum(keep)  # a kept root's number: the kept roots up to it in raster order
        labels[f][fg[f]] = np.where(keep[px], number[px], 0)
        counts[f] = number[-1] + 1
        first[f, 0] = -1
        where = np.flatnonzero(keep)[:cap - 1]
        first[f, 1:1 + len(where)] = where
        area[f, 1:1 + len(where)] = size[where]
    return dict(labels=labels, area=area, first=first, counts=counts, roots=roots, kept=kept, mask=labels > 0)


def spanning(o, f):
    """(kept, dropped): the components of frame f of an oracle result that lie in more than one tile"""
    r = o["roots"][f]
    h, w = r.shape
    y, x = np.mgrid[0:h, 0:w]
    tile = (y // TILE_H) * ((w + TILE_W - 1) // TILE_W) + x // TILE_W
    fg = r >= 0
    lo = np.full(h * w, 1 << 30)
    hi = np.full(h * w, -1)
    np.minimum.at(lo, r[fg], tile[fg])
    np.maximum.at(hi, r[fg], tile[fg])
    wide = hi > lo
    return int((wide & o["kept"][f]).sum()), int((wide & ~o["kept"][f]).sum())


def spiral(h, w):
    """one path, a pixel wide, from (0, 0) inwards, a pixel of background between its turns: one component, a forest as deep as it gets"""
    m = np.zeros((h, w), bool)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = True
    while True:
        for _ in range(2):
            ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if 0 <= ny < h and 0 <= nx < w and not m[ny, nx] and not (0 <= ay < h and 0 <= ax < w and m[ay, ax]):
                y, x = ny, nx
                m[y, x] = True
                break
            dy, dx = dx, -dy
        else:
            return m


def comb(h, w):
    """a spine along the first row and a tooth down every fourth column: one component whose every tooth is joined at the top only"""
    m = np.zeros((h, w), bool)
    m[0] = True
    m[:, ::4] = True
    return m


WEAK, STRONG = 1000, 2000  # pixel values of the hand-made scenes; their thresholds:
LOW, HIGH = 500, 1500


def scene(mask, strong_at=()):
    """uint16 frame: WEAK on the mask, STRONG at the pixels `strong_at` [(y, x), ...], 0 elsewhere"""
    f = np.where(mask, WEAK, 0).astype(np.uint16)
    for y, x in strong_at:
        f[y, x] = STRONG
    return f
