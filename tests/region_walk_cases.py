"""The counting reducers where a workgroup walks many items and frames: a model of the launch shape of walk_counters (csrc/region_walk.h) and
the cases test_region_walk_cases_cpu.py pins and test_gpu_counting_walk.py runs.  region_histogram, histogram and both counting passes of
region_quantiles give a workgroup the contiguous items [b * items / grid, (b + 1) * items / grid); with grid = min(items, cus * (2..8)) a
workgroup meets a second frame only where a stack has several times cus * 8 items, so the stack length n of every case is a function of the
CU count.  No test functions here.

Measured for cus = 256, a case with its inputs made and the oracle's answer checked (test_region_walk_cases_cpu.py, one CPU core), and the
same case on an MI355X with its oracle (test_gpu_counting_walk.py); n frames, million pixels:
    A  3x5      n 6151 and 1543     0.1 Mpx    CPU 0.04 - 0.44 s   GPU test 0.02 - 0.21 s
    A  32x64    n 6151 and 1543    12.6 and 3.2 Mpx   CPU 0.35 - 1.73 s   GPU test 0.09 - 0.59 s   (quantiles at three percents the slowest)
    B  129x128  n 769              12.7 Mpx    CPU 0.60 - 2.21 s   GPU test 0.14 - 0.81 s
    B  129x128  n 3073, light LDS  50.7 Mpx    CPU 1.39 s          GPU test 0.28 s
    B  160x256  n 685              28.1 Mpx    CPU 0.86 - 5.16 s   GPU test 0.22 - 1.95 s   (quantiles of 64 regions: a sort of 41 000 pixels a frame)
    C  32x64    n 6151             12.6 Mpx    CPU 1.30 - 2.05 s   GPU test 0.54 - 0.71 s
    D  32x64 n 6151, 160x256 n 685             CPU 0.55 - 1.37 s   GPU test 0.11 - 0.34 s
The statistics and geometry oracles (scatter operations) take the 12.6 Mpx stack of case A in 0.7 s and 1.0 s.  The whole CPU file runs
40 s, the whole GPU file 17 s.  The quantile cases of 64 regions are at the fewest regions and the shortest stack their conditions allow."""
import os
import re
import zlib
from collections import namedtuple

import numpy as np

from test_region_quantiles_cpu import PERCENTS as EIGHT_PERCENTS, frame_bytes, full_range_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "librir_amd", "csrc")


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def constant(text, name):
    """`constexpr <type> NAME = <integers joined by * or <<>;` as an int"""
    m = re.search(r"constexpr (?:int|size_t) %s = ([^;]+);" % name, text)
    assert m, "no constant %s" % name
    expr = m.group(1).replace("(size_t)", "")
    assert re.fullmatch(r"[\d\s*<]+", expr), (name, expr)
    shifts = [int(np.prod([int(x) for x in part.split("*")], dtype=object)) for part in expr.split("<<")]
    value = shifts[0]
    for s in shifts[1:]:
        value <<= s
    return value


WALK_ITEM, WALK_BLOCKS_PER_CU, WALK_LDS_BYTES = (constant(source("region_walk.h"), x) for x in ("WALK_ITEM", "WALK_BLOCKS_PER_CU", "WALK_LDS_BYTES"))
HISTOGRAM_LDS_MAX, HISTOGRAM_COPY_MAX, HISTOGRAM_MAX_COPIES = (constant(source("histogram_kernels.h"), x)
                                                               for x in ("HISTOGRAM_LDS_MAX", "HISTOGRAM_COPY_MAX", "HISTOGRAM_MAX_COPIES"))
QUANTILE_LDS_MAX = constant(source("quantile_kernels.h"), "QUANTILE_LDS_MAX")
QUANTILE_WORK_BYTES = constant(source("signal_processing_abi.cpp"), "QUANTILE_WORK_BYTES")  # what device.region_quantiles asks for at most
CUS = (32, 64, 128, 256)


def launch_shape(npx, n, lds_bytes, cus):
    """walk_launch_shape: -> (per_item_frame, items, grid)"""
    per_item_frame = (npx + WALK_ITEM - 1) // WALK_ITEM
    items = n * per_item_frame
    fit = max(1, WALK_LDS_BYTES // lds_bytes) if lds_bytes else WALK_BLOCKS_PER_CU
    return per_item_frame, items, min(items, cus * min(WALK_BLOCKS_PER_CU, fit))


def histogram_lds_bytes(k, nbins):
    """launch_region_histogram: -> (LDS bytes of a workgroup, copies of a counter)"""
    total = k * (nbins + 3)
    lds_n = min(total, HISTOGRAM_LDS_MAX)
    cshift = 0
    while (2 << cshift) <= HISTOGRAM_MAX_COPIES and (total << (cshift + 1)) <= HISTOGRAM_COPY_MAX:
        cshift += 1
    return (lds_n << cshift) * 4, 1 << cshift


def quantile_lds_bytes(k, nq, low):
    """launch_count<LOW>"""
    return min(k * (nq if low else 1), QUANTILE_LDS_MAX) * 1024


def quantile_groups(n, k, nq, work_bytes=None):
    """launch_region_quantiles: the frames of each group the stack is worked through in; work_bytes None: what
    rir_region_quantiles_workspace_bytes answers, which device.region_quantiles allocates"""
    b = frame_bytes(k, nq)
    if work_bytes is None:
        work_bytes = b * min(max(n, 1), max(1, QUANTILE_WORK_BYTES // b))
    group = min(n, work_bytes // b)
    return [min(group, n - g0) for g0 in range(0, n, group)]


def ranges(items, grid):
    """walk_counters: the [first, last) of every workgroup, as two arrays"""
    b = np.arange(grid, dtype=np.int64)
    return b * items // grid, (b + 1) * items // grid


def frames_in(rng, per_item_frame):
    """the frames a range [first, last) of items touches"""
    first, last = rng
    return range(first // per_item_frame, (last - 1) // per_item_frame + 1)


Walk = namedtuple("Walk", "deep touches begins_inside ends_inside whole_between ragged")


def walk_of(per_item_frame, items, grid):
    """what the ranges of one launch do: deep - more than three items a workgroup; touches - the fewest frames a range touches;
    begins_inside / ends_inside - some range is cut inside a frame at that end; whole_between - some range holds a whole frame between two
    partial ones; ragged - items / grid is neither an integer nor a multiple of per_item_frame"""
    first, last = ranges(items, grid)
    p = per_item_frame
    touches = int(((last - 1) // p - first // p + 1).min())
    inside_a, inside_b = first % p != 0, last % p != 0
    whole = inside_a & inside_b & (-(-first // p) < last // p)
    return Walk(items > 3 * grid, touches, bool(inside_a.any()), bool(inside_b.any()), bool(whole.any()), items % grid != 0 and items % (grid * p) != 0)


# One reducer on one stack.  op "hist": bins = (lo, width, nbins), labelled False takes device.histogram (one region, no map); op "quant":
# percents.  scene "full": the full 16-bit range with planted 0s and 65535s; "static": rows of one level out of 8000 +- 40 with long runs;
# "ramp": frame i holds 256 * (i % 200) + noise in [0, 256).  n: "8" -> 3 * 8 * cus + 7, "2" -> 3 * 2 * cus + 7, "model" -> pick_n().
# maps: the label maps the case runs with.  rows: None, or the rows of a frame that count.  copies: the copies of a counter the histogram
# keeps in LDS.  shallow: the launches that the n the case is set at leaves with one item a workgroup.
Case = namedtuple("Case", "name group h w op k labelled bins percents scene n maps rows copies shallow", defaults=(None, None, ()))
THREE = (0.0, 0.5, 1.0)
BOTH = ("shared", "per-frame")


def _cases():
    out = []
    for h, w in ((3, 5), (32, 64)):
        s = "A %dx%d " % (h, w)
        out += [
            Case(s + "hist 8 copies", "A", h, w, "hist", 1, False, (0, 256, 256), None, "full", "8", ("none",), copies=8),
            Case(s + "hist 8 copies, a map", "A", h, w, "hist", 1, True, (0, 256, 256), None, "full", "8", BOTH, copies=8),
            Case(s + "hist 4 copies", "A", h, w, "hist", 3, True, (0, 256, 256), None, "full", "8", BOTH, copies=4),
            Case(s + "hist static scene", "A", h, w, "hist", 3, True, (7960, 1, 81), None, "static", "8", BOTH, copies=8),
            Case(s + "quant three percents", "A", h, w, "quant", 3, True, None, THREE, "full", "8", BOTH),
            # two workgroups a CU: 20 495 counters of which 16 384 are in LDS; 65 histograms of which 64 are; 72 low-byte histograms
            Case(s + "hist beyond LDS", "A", h, w, "hist", 5, True, (0, 16, 4096), None, "full", "2", BOTH, copies=1),
            Case(s + "quant 65 regions", "A", h, w, "quant", 65, True, None, (0.5,), "full", "2", BOTH),
            # 9 regions keep the high-byte pass at eight workgroups a CU, so at this n it walks one item a workgroup
            Case(s + "quant eight percents", "A", h, w, "quant", 9, True, None, EIGHT_PERCENTS, "full", "2", BOTH, shallow=("high",)),
        ]
    for h, w in ((129, 128), (160, 256)):
        s = "B %dx%d " % (h, w)
        out += [
            Case(s + "hist 16 432 counters", "B", h, w, "hist", 16, True, (0, 64, 1024), None, "full", "model", BOTH, copies=1),
            Case(s + "quant 64 regions", "B", h, w, "quant", 64, True, None, (0.25, 0.5), "full", "model", BOTH),
        ]
    out += [
        Case("B 129x128 hist light LDS", "B", 129, 128, "hist", 1, False, (0, 256, 256), None, "full", "model", ("none",), copies=8),
        Case("C one label", "C", 32, 64, "quant", 1, True, None, (0.25, 0.5, 0.99), "ramp", "8", ("zeros",)),
        Case("C three stripes", "C", 32, 64, "quant", 3, True, None, (0.25, 0.5, 0.99), "ramp", "8", ("stripes",)),
        Case("D 32x64 rows", "D", 32, 64, "hist", 3, True, (0, 256, 256), None, "full", "8", BOTH, 29, 4),
        Case("D 160x256 rows", "D", 160, 256, "hist", 16, True, (0, 64, 1024), None, "full", "model", BOTH, 157, 1),
    ]
    return out


CASES = _cases()


def by_name(name):
    return next(c for c in CASES if c.name == name)


def walked_pixels(case):
    return (case.h if case.rows is None else case.rows) * case.w


def launches(case, n, cus, work_bytes=None):
    """every counting launch of the case on a stack of n frames: [(name, per_item_frame, items, grid)]"""
    npx = walked_pixels(case)
    if case.op == "hist":
        return [("count",) + launch_shape(npx, n, histogram_lds_bytes(case.k, case.bins[2])[0], cus)]
    out = []
    for g in quantile_groups(n, case.k, len(case.percents), work_bytes):
        out += [(name,) + launch_shape(npx, g, quantile_lds_bytes(case.k, len(case.percents), low), cus) for name, low in (("high", False), ("low", True))]
    return out


def pick_n(case, cus):
    """case B: the shortest stack on which every launch is deep, ragged, cut inside a frame at either end of some range, and has a range
    with a whole frame between two partial ones"""
    grid = max(g for _, _, _, g in launches(case, 1 << 20, cus, work_bytes=1 << 50))  # of a stack long enough that the CUs set it
    per = launch_shape(walked_pixels(case), 1, 0, cus)[0]
    assert per >= 2, case.name
    for n in range(3 * grid // per + 1, 8 * grid):
        walks = [walk_of(p, items, g) for _, p, items, g in launches(case, n, cus)]
        if all(w.deep and w.ragged and w.begins_inside and w.ends_inside and w.whole_between for w in walks):
            return n
    raise AssertionError("no stack length for %s at %d CUs" % (case.name, cus))


def frames_of(case, cus):
    """n, a function of the CU count"""
    if case.n == "model":
        return pick_n(case, cus)
    return 3 * int(case.n) * cus + 7


def make_inputs(case, cus, maps):
    """-> (frames [n][h][w] uint16, labels [h][w] or [n][h][w] int32 or None), seeded by the case's name; frames and per-frame maps differ
    from frame to frame, labels run from -1 to k"""
    n, h, w, k = frames_of(case, cus), case.h, case.w, case.k
    seed = zlib.crc32(("%s %s" % (case.name, maps)).encode())
    rng = np.random.default_rng(seed)
    per_frame = maps == "per-frame"
    if case.scene == "full":
        frames, labels = full_range_case(seed, n, h, w, k, per_frame)
        labels[..., 0, 0], labels[..., -1, -1] = -1, k  # both ends, whatever 15 draws gave
    elif case.scene == "static":
        frames = np.repeat(rng.integers(7960, 8041, (n, h, 1)), w, 2).astype(np.uint16)  # one level a row, other rows in every frame
        at = rng.integers(0, h * w, (n, 2))  # two pixels of every frame break its runs
        frames.reshape(n, -1)[np.arange(n)[:, None], at] = rng.integers(0, 65536, (n, 2))
        y = np.arange(h)[None, :, None] + (np.arange(n)[:, None, None] if per_frame else 0)  # bands of rows, from -1 to k, that move
        labels = np.broadcast_to((y % h) * (k + 1) // (h - 1) - 1, (n if per_frame else 1, h, w)).astype(np.int32)
        labels = np.ascontiguousarray(labels if per_frame else labels[0])
    else:
        frames = (256 * (np.arange(n) % 200)[:, None, None] + rng.integers(0, 256, (n, h, w))).astype(np.uint16)
        labels = np.zeros((h, w), np.int32) if maps == "zeros" else np.broadcast_to((np.arange(w) * 3 // w).astype(np.int32), (h, w)).copy()
    if maps == "none":
        labels = None
    elif n > 1:
        assert not np.array_equal(frames[0], frames[1]) and (not per_frame or not np.array_equal(labels[0], labels[1]))
    return frames, labels


def in_chunks(oracle, frames, labels, *args, pixels=1 << 22):
    """oracle(frames, labels, *args) a few million pixels at a time (every frame is on its own): the arrays of the results, joined"""
    step = max(1, pixels // (frames.shape[1] * frames.shape[2]))
    per_frame = labels is not None and labels.ndim == 3
    parts = [oracle(frames[i:i + step], labels[i:i + step] if per_frame else labels, *args) for i in range(0, frames.shape[0], step)]
    if isinstance(parts[0], dict):
        return {key: None if parts[0][key] is None else np.concatenate([p[key] for p in parts]) for key in parts[0]}
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(len(parts[0])))
