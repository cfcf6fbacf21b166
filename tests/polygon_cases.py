"""Polygon label maps: the seeded cases shared by tests/golden/make_polygon_golden.py, test_polygon_map_cpu.py and test_gpu_polygon_map.py, and
the numpy oracle - a row-local restatement of the reference's scanline fill (the definition is with rir_polygon_map_device,
include/rir_amd_device.h): every row follows from the rounded vertices alone, nothing is carried over from the row above.

A case is a dict: shape (h, w), sets (one list of polygons, or one list per map when per_map), values (list or None), background, shifts
((n, 2) or None).  A polygon is a (k, 2) float64 array of (x, y)."""
import numpy as np

LIMIT = float(1 << 24)  # a polygon with a shifted coordinate that is not finite or larger than this draws nothing


def round_half_away(v):
    """std::round on float64: halves away from zero (-0.5 -> -1)"""
    v = np.asarray(v, np.float64)
    t = np.trunc(v)
    return t + np.where(np.abs(v - t) >= 0.5, np.sign(v), 0.0)


def rounded_vertices(poly, shift):
    """-> (X, Y) int64 arrays, or None when the polygon is out of range in this map"""
    p = np.asarray(poly, np.float64).reshape(-1, 2)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + np.asarray(shift, np.float64)
    if not np.all(np.isfinite(s)) or np.any(np.abs(s) > LIMIT):
        return None
    r = round_half_away(s).astype(np.int64)
    return r[:, 0], r[:, 1]


def polygon_row(X, Y, y, first, xmin, xmax):
    """the spans (lo, hi), inclusive, of row y of a polygon of >= 3 vertices; xmin, xmax: the clipped box's columns"""
    n = len(X)
    Xj, Yj = np.roll(X, 1), np.roll(Y, 1)
    if first:
        cross = ((Y <= y) & (Yj >= y)) | ((Yj <= y) & (Y >= y))
    else:
        cross = ((Y < y) & (Yj >= y)) | ((Yj < y) & (Y >= y))
    cross &= Y != Yj
    xi, yi, xj, yj = X[cross], Y[cross], Xj[cross], Yj[cross]
    t = (y - yi).astype(np.float64) / (yj - yi).astype(np.float64)
    prod = t * (xj - xi).astype(np.float64)
    nodes = np.sort(round_half_away(xi.astype(np.float64) + prod).astype(np.int64))
    buf = np.zeros(n + 1, np.int64)
    buf[:len(nodes)] = nodes
    count = len(nodes)
    if first:
        count = 1
        for i in range(1, len(nodes)):
            if buf[i] != buf[i - 1]:
                buf[count] = buf[i]
                count += 1
    spans = []
    for i in range(0, count, 2):
        a, b = int(buf[i]), int(buf[i + 1])
        if a >= xmax:
            break
        if b >= xmin:
            spans.append((max(a, xmin), min(b, xmax - 1)))
    return spans


def line_row(X, Y, y, w):
    """the columns of row y that the two-point form draws"""
    x1, x2, y1, y2 = int(X[0]), int(X[1]), int(Y[0]), int(Y[1])
    dx, dy = x2 - x1, y2 - y1
    out = []
    if dx == 0:
        if min(y1, y2) <= y <= max(y1, y2):
            out.append(x1)
    elif dy == 0:
        if y == y1:
            out.extend(range(min(x1, x2), max(x1, x2) + 1))
    else:
        a = np.float64(dy) / np.float64(dx)
        b = np.float64(y1) - a * np.float64(x1)
        if abs(dx) > abs(dy):
            step = 1 if dx > 0 else -1
            lo, hi = (max(x1, 0), min(x2 - 1, w - 1)) if step > 0 else (max(x2 + 1, 0), min(x1, w - 1))
            if lo <= hi:
                xs = np.arange(lo, hi + 1)
                ys = round_half_away(xs.astype(np.float64) * a + b).astype(np.int64)
                out.extend(int(x) for x in xs[ys == y])
        elif y != y2 and min(y1, y2) <= y <= max(y1, y2):
            out.append(int(round_half_away((np.float64(y) - b) / a)))
        if y == y2:
            out.append(x2)
    return [x for x in out if 0 <= x < w]


def draw(img, X, Y, value):
    """paint one polygon of rounded vertices into img (h, w) as the reference's draw_polygon does"""
    h, w = img.shape
    n = len(X)
    if n == 0:
        return
    if n == 1:
        if 0 <= X[0] < w and 0 <= Y[0] < h:
            img[Y[0], X[0]] = value
        return
    if n == 2:
        for y in range(max(int(Y.min()), 0), min(int(Y.max()), h - 1) + 1):
            for x in line_row(X, Y, y, w):
                img[y, x] = value
        return
    xmin, xmax, ymin, ymax = int(X.min()), int(X.max()) + 1, int(Y.min()), int(Y.max()) + 1
    if xmax <= 0 or xmin >= w or ymax <= 0 or ymin >= h:
        return
    xmin, xmax, ymin, ymax = max(xmin, 0), min(xmax, w), max(ymin, 0), min(ymax, h)
    for y in range(ymin, ymax):
        for lo, hi in polygon_row(X, Y, y, y == ymin, xmin, xmax):
            if lo <= hi:
                img[y, lo:hi + 1] = value


def n_maps(case):
    if case["shifts"] is not None:
        return len(case["shifts"])
    return len(case["sets"]) if case["per_map"] else 1


def oracle(case):
    """-> int32 (n, h, w); the API gives (h, w) for one set without shifts"""
    h, w = case["shape"]
    n = n_maps(case)
    out = np.full((n, h, w), case["background"], np.int32)
    for m in range(n):
        polys = case["sets"][m] if case["per_map"] else case["sets"]
        shift = case["shifts"][m] if case["shifts"] is not None else (0.0, 0.0)
        for p, poly in enumerate(polys):
            v = rounded_vertices(poly, shift)
            if v is not None:
                draw(out[m], v[0], v[1], p if case["values"] is None else case["values"][p])
    return out


def api_args(case):
    """the arguments of device.polygon_map / signal_processing.polygon_map for a case, and the shape of the result"""
    n = n_maps(case)
    kw = dict(values=case["values"], background=case["background"], shifts=case["shifts"])
    squeeze = not case["per_map"] and case["shifts"] is None
    return case["sets"], case["shape"], kw, (case["shape"] if squeeze else (n,) + tuple(case["shape"]))


# ---- polygons -----------------------------------------------------------------------------------------------------------------------
KINDS = ("fractional", "integer", "half", "star", "repeated")


def random_polygon(rng, kind, h, w):
    lo, span = np.array([-0.35 * w - 1, -0.35 * h - 1]), np.array([1.7 * w + 2, 1.7 * h + 2])
    if kind == "star":
        k = int(rng.integers(4, 9))
        c = lo + span * (0.25 + 0.5 * rng.random(2))
        r = np.where(np.arange(2 * k) % 2 == 0, 0.45, 0.18) * max(h, w, 4) * (0.6 + 0.8 * rng.random())
        ang = rng.random() * 6.28 + np.arange(2 * k) * np.pi / k
        return c + np.stack([r * np.cos(ang), r * np.sin(ang)], 1)
    p = lo + span * rng.random((int(rng.integers(3, 10)), 2))
    if kind == "integer":
        p = np.floor(p)
    elif kind == "half":
        p = np.floor(p) + 0.5
    elif kind == "repeated":
        p = np.repeat(p, rng.integers(1, 4, len(p)), axis=0)
    return p


def ring(k, cx, cy, rx, ry, phase=0.1):
    a = phase + np.arange(k) * 2 * np.pi / k
    return np.stack([cx + rx * np.cos(a), cy + ry * np.sin(a)], 1)


def octagons(h, w, count=16):
    """count octagons on a grid that cover about 0.4 of the image (the scene of tests/perf/polygon_map_time.py)"""
    g = int(np.ceil(np.sqrt(count)))
    r = np.sqrt(0.4 * h * w / count / 2.83)  # an octagon of circumradius r has area 2.83 r^2
    return [ring(8, (i % g + 0.5) * w / g, (i // g + 0.5) * h / g, r, r, 0.39) for i in range(count)]


def case(shape, sets, values=None, background=-1, shifts=None, per_map=False):
    def arr(p):
        return np.asarray(p, np.float64).reshape(-1, 2)

    sets = [[arr(p) for p in s] for s in sets] if per_map else [arr(p) for p in sets]
    return dict(shape=tuple(shape), sets=sets, values=None if values is None else [int(v) for v in values], background=int(background),
                shifts=None if shifts is None else np.asarray(shifts, np.float64).reshape(-1, 2), per_map=per_map)


SMALL_SHAPES = [(1, 1), (3, 5), (9, 13), (33, 70), (17, 130), (64, 64)]
BIG_SHAPE = (512, 640)

# vertices on 9x13 -> pixels drawn (counted with the reference)
DEGENERATES = {
    "flat_to_column_0": ([(0, 3), (5, 3), (9, 3)], 1),
    "flat_inside": ([(2, 3), (5, 3), (9, 3)], 0),
    "vertical_run": ([(4, 1), (4, 6), (4, 3)], 6),
    "identical": ([(4, 4)] * 3, 0),
    "rectangle": ([(2, 2), (9, 2), (9, 7), (2, 7)], 48),
    "starts_above": ([(2, -5), (11, -5), (6, 6)], 23),
    "bow_tie": ([(1, 1), (11, 8), (11, 1), (1, 8)], 57),
}
TIE_TRIANGLE = [(-38, 10), (7, 0), (30, 10)]  # on 12x32: row 1 starts at x = 3 (a fused multiply-add gives 2)

LINES = [
    [(3, 1), (3, 7)], [(3, 7), (3, 1)],  # vertical
    [(1, 4), (10, 4)], [(10, 4), (1, 4)],  # horizontal
    [(1, 1), (11, 5)], [(11, 5), (1, 1)], [(0, 8), (12, 3)],  # x-major
    [(2, 0), (5, 8)], [(5, 8), (2, 0)], [(9, 8), (7, 1)],  # y-major
    [(6, 6), (6, 6)],  # equal points
    [(-5, -3), (20, 11)], [(15, 4), (-4, 4)], [(5, -6), (5, 20)], [(-3, 12), (4, -9)], [(30, 30), (40, 35)],  # end points outside
    [(2.5, 1.5), (9.49, 6.5)], [(-0.5, 3.5), (7.5, -0.5)],  # rounded first
]
POINTS = [[(0, 0)], [(12, 8)], [(13, 8)], [(-1, 3)], [(4.5, 2.5)], [(-0.5, -0.5)], [(5, 9)]]


def _kinds(seed, shape, per_kind=2):
    rng = np.random.default_rng(seed)
    return [random_polygon(rng, k, *shape) for k in KINDS for _ in range(per_kind)]


def cases():
    """name -> case; names ending in _big are stored as SHA-256 only"""
    c = {}
    for i, shape in enumerate(SMALL_SHAPES + [BIG_SHAPE]):
        tag = "%dx%d%s" % (shape + ("_big" if shape == BIG_SHAPE else "",))
        c["kinds_" + tag] = case(shape, _kinds(100 + i, shape), values=[3, 1, 4, 1, 5, 9, 2, 6, 5, -1])
        c["default_" + tag] = case(shape, _kinds(200 + i, shape))
    c["tie_triangle"] = case((12, 32), [TIE_TRIANGLE], values=[7], background=0)
    for name, (pts, _) in DEGENERATES.items():
        c["degenerate_" + name] = case((9, 13), [pts], values=[1], background=0)
    c["degenerates_together"] = case((9, 13), [pts for pts, _ in DEGENERATES.values()])
    # the same with a 65-vertex polygon in the set: every polygon then takes the form for long polygons
    c["degenerates_long_form"] = case((9, 13), [pts for pts, _ in DEGENERATES.values()] + [ring(65, 6, 4, 5.5, 3.5)])
    c["kinds_long_form"] = case((33, 70), _kinds(103, (33, 70)) + [ring(70, 30, 16, 12, 9)], values=[3, 1, 4, 1, 5, 9, 2, 6, 5, -1, 7])
    # other geometry
    c["outside"] = case((33, 70), [[(80, 5), (95, 9), (85, 30)], [(5, -20), (30, -3), (9, -2)], [(-9, 5), (-1, 20), (-30, 30)], [(3, 40), (60, 50), (9, 35)]])
    c["covers_all"] = case((33, 70), [[(-5, -5), (100, -5), (100, 50), (-5, 50)]], values=[12])
    c["covers_all_exactly"] = case((17, 130), [[(0, 0), (129, 0), (129, 16), (0, 16)]], values=[2], background=9)
    for shape in ((33, 70), (17, 130)):
        h, w = shape
        many = [ring(3, w / 2, h / 2, w / 3, h / 2.2), ring(64, w / 3, h / 2, w / 3.5, h / 2.5), ring(65, w / 1.6, h / 2.2, w / 4, h / 1.8),
                ring(200, w / 2, h / 1.7, w / 1.9, h / 2.1), np.zeros((0, 2)), [(2, 2), (w - 3, 3), (w // 2, h - 2)]]
        c["vertex_counts_%dx%d" % shape] = case(shape, many, values=[4, 3, 2, 1, 8, 0])
    rng = np.random.default_rng(7)
    wiggly = ring(200, 320, 256, 300, 240) + rng.normal(0, 6, (200, 2))
    c["vertex_counts_big"] = case(BIG_SHAPE, [ring(64, 200, 200, 180, 150), ring(65, 400, 300, 200.5, 190.25), wiggly, ring(3, 500, 100, 90, 80)])
    c["octagons_big"] = case(BIG_SHAPE, octagons(*BIG_SHAPE))
    # more polygons than one look at the boxes takes (64), and rows wider than one segment of the row buffer (1 536 columns)
    rng = np.random.default_rng(17)
    c["many_polygons"] = case((64, 64), [ring(int(rng.integers(3, 7)), *rng.uniform(-4, 68, 2), *rng.uniform(1, 9, 2)) for _ in range(150)])
    c["wide_rows"] = case((6, 3300), [[(-10, -2), (3400, 1), (1500, 9)], [(1530, 0), (1541, 0), (1541, 5), (1530, 5)], [(100, 1), (3299, 4)],
                                      [(3071.5, 2), (3072.5, 2), (3200, 5.5)], [(1536, 3)], [(1535, 3)], [(3299, 5), (0, 5)], [(3000, -3), (3080, 8)]],
                          values=[1, 2, 3, 4, 5, 6, 7, 8], background=0)
    # one-point and two-point polygons
    c["lines"] = case((9, 13), LINES, values=list(range(1, len(LINES) + 1)), background=0)
    for k, ln in enumerate(LINES):
        c["line_%02d" % k] = case((9, 13), [ln], values=[1], background=0)
    c["points"] = case((9, 13), POINTS)
    rng = np.random.default_rng(11)
    c["random_lines"] = case((33, 70), [np.floor(rng.random((2, 2)) * [110, 60] - [20, 13]) / 2 for _ in range(40)])
    c["lines_wide"] = case((17, 130), [[(-4, 2), (140, 15)], [(129, 0), (0, 16)], [(64, -3), (66, 30)], [(3, 8), (127, 8)]], values=[1, 2, 3, 1], background=0)
    # painter's order
    over = [[(2, 2), (40, 2), (40, 25), (2, 25)], [(20, 10), (65, 12), (50, 31)], [(10, 5), (30, 5), (30, 30), (10, 30)], [(25, 0), (35, 0), (35, 32), (25, 32)],
            [(0, 15), (69, 15), (69, 18), (0, 18)], [(33, 16)], [(5, 5), (60, 28)]]
    c["painter"] = case((33, 70), over, values=[5, 2, 5, -1, 0, 7, 2])
    c["painter_default_values"] = case((33, 70), over, background=3)
    # maps
    shifts70 = np.concatenate([[(0, 0), (0.5, -0.5), (-0.5, 0.5), (2.5, 1.5), (-3.5, -2.5), (0.25, 0.75), (-7.3, 4.9)],
                               np.random.default_rng(13).uniform(-9, 9, (63, 2))])
    c["shared_1_map"] = case((9, 13), _kinds(300, (9, 13), 1), shifts=[(1.5, -0.5)])
    c["shared_3_maps"] = case((33, 70), _kinds(301, (33, 70), 1) + [[(3, 3), (30, 20)], [(40, 9)]], shifts=shifts70[1:4] * 3)
    c["shared_70_maps"] = case((9, 13), _kinds(302, (9, 13), 1) + [[(1, 2), (9, 7)]], shifts=shifts70)
    c["per_map_1"] = case((9, 13), [_kinds(303, (9, 13), 1)], per_map=True)
    c["per_map_3"] = case((33, 70), [_kinds(304 + m, (33, 70), 1) for m in range(3)], values=[2, 0, 1, 0, 6], per_map=True)
    c["per_map_70"] = case((3, 5), [_kinds(400 + m, (3, 5), 1) for m in range(70)], per_map=True)
    c["per_map_3_shifted"] = case((17, 130), [_kinds(310 + m, (17, 130), 1) for m in range(3)], shifts=[(0.5, 0.5), (-20.5, 3.25), (64, -8)], per_map=True)
    c["per_map_70_shifted"] = case((9, 13), [_kinds(500 + m, (9, 13), 1)[:3] for m in range(70)], shifts=shifts70[::-1], per_map=True)
    # the out-of-range rule: the polygon with the bad vertex, and only it, draws nothing
    good = [[(1, 1), (11, 2), (6, 8)], [(3, 0), (12, 7), (0, 7)]]
    for name, bad in (("nan", np.nan), ("inf", np.inf), ("minus_inf", -np.inf), ("1e30", 1e30)):
        c["out_of_range_" + name] = case((9, 13), [good[0], [(2, 2), (bad, 4), (9, 8), (2, 7)], good[1], [(4, bad)], [(1, 1), (5, bad)]], background=-1)
    c["out_of_range_by_shift"] = case((9, 13), good, shifts=[(0, 0), (3e7, 0), (1, -3e7), (-1, 1)])
    return c
