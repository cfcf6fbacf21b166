"""The exact Euclidean distance transform's test material (no tests here): the brute-force numpy reference for dist2 and index by the
definition in include/rir_amd_device.h (rir_distance_transform_device), a separable reference that is fast enough for a full frame, and the
images and shapes the CPU and GPU tests share."""
import numpy as np

DIST2_NONE = 0x7FFFFFFF
SHAPES = [(1, 1), (1, 7), (7, 1), (3, 64), (5, 65), (2, 129), (130, 3), (37, 70), (65, 63)]  # (h, w)
TYPES = {"?": np.bool_, "B": np.uint8, "H": np.uint16, "i": np.int32}


def _apply_border(dist2, index, rows, w):
    """the border switch of the definition on the image rows of dist2 / index (in place)"""
    ys, xs = np.mgrid[:rows, :w]
    b = np.minimum(np.minimum(xs + 1, w - xs), np.minimum(ys + 1, rows - ys)).astype(np.int64)
    nearer = b * b < dist2[:rows]
    dist2[:rows][nearer] = (b * b)[nearer]
    index[:rows][nearer] = -1


def _outside_rows(h, w, rows):
    """dist2 and index as int64 [h][w] with the rows outside the image filled in: 0 and the pixel's own index"""
    dist2 = np.zeros((h, w), np.int64)
    index = np.arange(h * w, dtype=np.int64).reshape(h, w)
    return dist2, index


def brute_force(img, background=0, border=False, rows=None):
    """(dist2, index), int32 [h][w], of one image by the definition: every pixel against every background pixel, O(pixels x background)"""
    h, w = img.shape
    rows = h if rows is None else rows
    dist2, index = _outside_rows(h, w, rows)
    qy, qx = np.nonzero(img[:rows] == background)  # (raster order: the first minimum is the lowest flat index)
    xs = np.arange(w, dtype=np.int64)
    for y in range(rows):
        if qy.size == 0:
            dist2[y], index[y] = DIST2_NONE, -1
            continue
        d = (y - qy[None, :]) ** 2 + (xs[:, None] - qx[None, :]) ** 2
        k = d.argmin(axis=1)
        dist2[y], index[y] = d[xs, k], qy[k] * w + qx[k]
    if border and rows:
        _apply_border(dist2, index, rows, w)
    return dist2.astype(np.int32), index.astype(np.int32)


def line_offsets(bg):
    """per row of the bool image bg [rows][w]: the signed offset qx - x to the nearest True cell of the row, the left one on a tie; the
    rows without one get `far` everywhere; -> (offsets int64, has: which rows have a cell)"""
    rows, w = bg.shape
    xs = np.arange(w, dtype=np.int64)
    far = 4 * w + 4
    left = np.maximum.accumulate(np.where(bg, xs, -far), axis=1)  # x of the last cell at or left
    right = np.minimum.accumulate(np.where(bg, xs, far)[:, ::-1], axis=1)[:, ::-1]  # x of the next cell at or right
    dl, dr = xs - left, right - xs
    return np.where(dl <= dr, -dl, dr), bg.any(axis=1)


def separable(img, background=0, border=False, rows=None):
    """(dist2, index), int32 [h][w], of one image in two passes: the nearest background cell of every row, then for every pixel the minimum
    over the rows s of (y - s)^2 + offset(s, x)^2, the first s on a tie - O(h) per pixel, vectorised, for frames the brute force cannot take"""
    h, w = img.shape
    rows = h if rows is None else rows
    dist2, index = _outside_rows(h, w, rows)
    if rows:
        offs, has = line_offsets(img[:rows] == background)
        if not has.any():
            dist2[:rows], index[:rows] = DIST2_NONE, -1
        else:
            s = np.nonzero(has)[0].astype(np.int64)
            f = offs[s] ** 2  # [rows that have a cell][w]
            xs = np.arange(w, dtype=np.int64)
            for y in range(rows):
                cost = f + ((y - s) ** 2)[:, None]
                k = cost.argmin(axis=0)
                dist2[y] = cost[k, xs]
                index[y] = s[k] * w + xs + offs[s[k], xs]
        if border:
            _apply_border(dist2, index, rows, w)
    return dist2.astype(np.int32), index.astype(np.int32)


def reference_stack(stack, background=0, border=False, rows=None, how=brute_force):
    """(dist2, index) [n][h][w] of a stack, frame by frame"""
    pairs = [how(f, background, border, rows) for f in stack]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def _nine(h, w):
    """the corner, edge and interior positions of an h x w image (fewer where they coincide)"""
    return sorted({(y, x) for y in (0, h // 2, h - 1) for x in (0, w // 2, w - 1)})


def foregrounds(h, w):
    """[(name, bool [h][w] foreground)]: the images every test runs, in a fixed order"""
    rng = np.random.default_rng(h * 1000 + w)
    ys, xs = np.mgrid[:h, :w]
    out = [("all_background", np.zeros((h, w), bool)), ("all_foreground", np.ones((h, w), bool))]
    for y, x in _nine(h, w):
        one = np.ones((h, w), bool)
        one[y, x] = False
        out.append(("one_background_%d_%d" % (y, x), one))
        out.append(("one_foreground_%d_%d" % (y, x), ~one))
    for density in (0.5, 0.97, 0.999):
        out.append(("random_%g" % density, rng.random((h, w)) < density))
    out.append(("left_half", xs < w // 2))
    out.append(("bottom_half", ys >= h // 2))
    out.append(("checkerboard", (ys + xs) % 2 == 0))
    out.append(("diagonal_background", ys * max(w - 1, 1) != xs * max(h - 1, 1)))
    out.append(("diagonal_foreground", ys * max(w - 1, 1) == xs * max(h - 1, 1)))
    out.append(("rows_without_background", (ys % 3 == 1) | (xs != (ys * 7) % w)))
    out.append(("columns_without_background", (xs % 2 == 1) | (ys != (xs * 5) % h)))
    disc = (ys - h // 2) ** 2 + (xs - w // 2) ** 2 <= 36
    out.append(("disc_6", disc))
    out.append(("hole_6", ~disc))
    return out


def label_map(h, w):
    """an int32 label map with labels -2 .. 5: blocks of a few pixels, 0 and 3 among them"""
    rng = np.random.default_rng(h * 77 + w)
    coarse = rng.integers(-2, 6, ((h + 2) // 3, (w + 3) // 4)).astype(np.int32)
    return np.kron(coarse, np.ones((3, 4), np.int32))[:h, :w].copy()


def typed_stack(h, w, type_char):
    """the images of foregrounds(h, w) as one stack [n][h][w] of the type: background cells 0, foreground cells 1 for bool and otherwise some
    non-zero value of the type (every value but the background is foreground); the int32 stack ends on a label map"""
    dtype = TYPES[type_char]
    rng = np.random.default_rng(ord(type_char) + h + w)
    frames = []
    for _, fg in foregrounds(h, w):
        if type_char == "?":
            frames.append(fg.copy())
            continue
        lo, hi = (-(1 << 31), (1 << 31) - 1) if type_char == "i" else (1, np.iinfo(dtype).max)
        values = rng.integers(lo, hi, (h, w), endpoint=True).astype(dtype)
        values[values == 0] = 1
        frames.append(np.where(fg, values, dtype(0)).astype(dtype))
    if type_char == "i":
        frames.append(label_map(h, w))
    return np.ascontiguousarray(np.stack(frames))
