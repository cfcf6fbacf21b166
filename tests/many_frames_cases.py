"""Stacks of more frames than one grid dimension holds: the periodic stack and its expectation, the shapes - from the kernels' own constants -
and, per entry, the P distinct frames with their reference.  No test functions.

A stack of N frames is never made on the host: frame i is ``distinct[i % P]``, indexed on the device, and so are the per-frame side arrays and
the expectation, which is the reference of the P distinct frames.  P = 7: the piece sizes the units use (65 535, 65 536, 32 768) leave
residues 1, 2 and 1, so a piece read or written one piece early or late, a dropped piece or a frame index cut to 16 bits lands on a frame
with other content."""
import re

import numpy as np
from cases import full_range_frames

import morphology_cases
import reconstruct_cases
from region_walk_cases import constant, source

N = 65537
P = 7


# ---- the constants of the units ------------------------------------------------------------------------------------------------------------
def grid_limits():
    """{(file, the line's pattern): value} of every literal that bounds a piece of a stack, or the stack, in the units' sources"""
    found = {}
    for name, pattern in (("pair_tile.h", r"constexpr int MAX_GRID_Z = (\d+);"),
                          ("distance_kernels.hip", r"work_bytes / distance_frame_bytes\(w, h\)\), (\d+)\);"),
                          ("temporal_kernels.hip", r"constexpr int TM_GRID_Y = (\d+);"), ("downsample_kernels.hip", r"s0 \+= (\d+)\)"),
                          ("downsample_kernels.hip", r"slabs > (\d+)\)"), ("label_kernels.hip", r"frames > 0 && frames <= (\d+);")):
        m = re.search(pattern, source(name))
        assert m, (name, pattern)
        found[(name, pattern)] = int(m.group(1))
    return found


_filters, _morph, _temporal = (source(x) for x in ("filter_kernels.hip", "morphology_kernels.hip", "temporal_kernels.hip"))
TR_TY, GAUSS_TY, CHAIN_TY, MEDIAN_TY = (constant(_filters, x) for x in ("TR_TY", "GAUSS_TY", "CHAIN_TY", "MEDIAN_TY"))
MORPH_TY = constant(_morph, "MORPH_TY")
TM_GRID_Y, TM_RUN_MIN = constant(_temporal, "TM_GRID_Y"), constant(_temporal, "TM_RUN_MIN")
MAX_GRID_Z = constant(source("pair_tile.h"), "MAX_GRID_Z")


def _pair(text, names):
    m = re.search(r"constexpr int %s = (\d+), %s = (\d+);" % names, text)
    assert m, names
    return int(m.group(1)), int(m.group(2))


G_TW, G_TH = _pair(_morph, ("G_TW", "G_TH"))  # the general morphology kernel's tile
REC_TW, REC_TH = _pair(source("reconstruct_kernels.h"), ("RECONSTRUCT_TILE_W", "RECONSTRUCT_TILE_H"))
DISTANCE_ROWS = constant(source("distance_kernels.hip"), "DISTANCE_ROWS_PER_BLOCK")


def tile_shapes(tile_w, tile_h, small=(2, 2), thin=2):
    """(h, w): the small frame, one pixel wider than a tile and `thin` rows high, one row taller than a workgroup's rows and `thin` pixels wide"""
    return [small, (thin, tile_w + 1), (tile_h + 1, thin)]


TRANSLATE_SHAPES = tile_shapes(63, 4 * TR_TY)
SIGMAS = {1: 0.75, 2: 1.0}  # radius -> a sigma that takes it
# the direct gaussian kernel (256 columns a workgroup, gridDim.y = h): several rows; a second workgroup along x needs 257 columns, 67 MB a tensor
DIRECT_GAUSS_CASES = [(0.75, (2, 2)), (0.75, (5, 3)), (3.3, (2, 2)), (3.3, (5, 3))]  # (sigma, (h, w)): radius 1, and 6 in either order
GAUSS_SHAPES = {r: tile_shapes(64 - 2 * r, 4 * GAUSS_TY) for r in SIGMAS}
MEDIAN_SHAPES = tile_shapes(60, 4 * MEDIAN_TY, small=(3, 3), thin=3)  # (the entry wants 3 x 3 pixels at least)
CHAIN_SHAPES = {r: tile_shapes(64 - 2 * r - 2, 4 * (CHAIN_TY - 2)) for r in SIGMAS}
PLANES_SHAPES = [((2, 2), 8), ((3, 70), 96)]  # ((h, w), linesize)


def morph_pair_shapes(size, stages=1):
    """the shapes of the pair kernel of a square of `size`: its halo is `stages` radii of pixels, hl pairs - lanes - on each side of a wave"""
    hl = (stages * (size // 2) + 1) // 2
    return [(2, 2), (2, 2 * (64 - 2 * hl) + 2), (4 * MORPH_TY + 1, 2)]


MORPH_GENERAL_SHAPES = [(2, 3), (2, G_TW + 1), (G_TH + 1, 3)]  # odd widths: the general kernel whatever the size
RECONSTRUCT_SHAPES = [(2, 2), (1, REC_TW + 1)]
# 64 columns per block; rows = h - 1 leaves one row more than a block's; 3 x 3: the outputs of 2 x 2 masks at rows = 1 are too few to differ
DISTANCE_SHAPES = [(3, 3), (2, 64 + 1), (DISTANCE_ROWS + 2, 2)]


# ---- the periodic stack ----------------------------------------------------------------------------------------------------------------------
_SIGNED = {"uint16": "int16", "uint32": "int32", "uint64": "int64"}


def _torch():
    import torch

    return torch


def to_device(a):
    torch = _torch()
    a = np.ascontiguousarray(a)
    if a.dtype.name in _SIGNED:  # (unsigned types wider than a byte: moved and indexed as their signed twins)
        return torch.from_numpy(a.view(_SIGNED[a.dtype.name])).cuda().view(getattr(torch, a.dtype.name))
    return torch.from_numpy(a).cuda()


def frame_index(n=N):
    torch = _torch()
    return torch.arange(n, device="cuda") % P


def periodic(distinct, n=N):
    """the stack of `n` frames on the device whose frame i is distinct[i % P]; `distinct`: a numpy array or a device tensor of P items"""
    torch = _torch()
    d = distinct if isinstance(distinct, torch.Tensor) else to_device(distinct)
    assert d.shape[0] == P
    name = str(d.dtype).split(".")[1]
    if name in _SIGNED:
        return d.view(getattr(torch, _SIGNED[name]))[frame_index(n)].view(d.dtype)
    return d[frame_index(n)]


def bits(t):
    """the tensor as integers of its item size, for comparisons bit for bit (NaNs and signed zeros included)"""
    torch = _torch()
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def assert_periodic(got, want_distinct, what=""):
    """`got` [n][...] equals, bit for bit, the P items of `want_distinct` repeated; the message names the first frame that differs"""
    torch = _torch()
    n = got.shape[0]
    want = periodic(want_distinct, n)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, tuple(got.shape), tuple(want.shape))
    g, w = bits(got), bits(want)
    if torch.equal(g, w):
        return
    first = int((g != w).reshape(n, -1).any(dim=1).nonzero()[0])
    raise AssertionError("%s: frame %d (residue %d mod %d) is the first of %d frames that differs" % (what, first, first % P, P, n))


def pairwise_different(items):
    """whether no two of the items (arrays, or tuples of arrays) are equal"""
    keys = [b"".join(np.ascontiguousarray(a).tobytes() for a in (it if isinstance(it, (tuple, list)) else (it,))) for it in items]
    return len(set(keys)) == len(keys)


# ---- the frame filters ---------------------------------------------------------------------------------------------------------------------
FILTER_KINDS = ("ti_bits", "saturated_blob", "checkerboard", "uniform", "high_dead", "flat_40000", "wide_normal")
STRATEGIES = ("nearest", "background", "noborder")
BACKGROUND = 65535


def filter_frames(h, w, dtype=np.uint16):
    """P frames over the whole 16-bit range, one of each kind of cases.FULL_RANGE_KINDS that is not flat"""
    fr = np.stack([full_range_frames(k, h, w)[1][i % 3] for i, k in enumerate(FILTER_KINDS)])
    assert len(fr) == P
    return fr.astype(dtype)


def frame_offsets(h, w):
    """(P, 2) float32 (dx, dy): non-integer, in both directions, one whole pixel, and the last past the border on both axes"""
    return np.array([(0.5, 0.25), (-0.25, 0.5), (0.3, -0.7), (-0.999, 0.001), (1.0, -1.0), (-0.5, -0.5), (w + 1.5, -h - 0.25)], np.float32)


def hot_first(h, w):
    """a first image for BadPixels: a cold scene with two saturated pixels - the deviation is NaN and about half of the pixels are flagged"""
    rng = np.random.default_rng(h * 1000 + w)
    img = (120 + rng.integers(0, 40, (h, w))).astype(np.uint16)
    img.flat[rng.choice(h * w, 2, replace=False)] = 65535
    return img


BAD_PIXELS_SHAPES = [(2, 61), (57, 2), (4, 80)]  # (4 x 80: more flagged pixels than one workgroup of the repair kernels takes)


def translate_reference(oracle, frames, offsets, strategy):
    return np.stack([oracle.translate(f, o[0], o[1], "" if strategy == "noborder" else strategy, background=BACKGROUND) for f, o in zip(frames, offsets)])


def planes_frames(h, w):
    rng = np.random.default_rng(h * 100 + w)
    return rng.integers(0, 65536, (P, h, w)).astype(np.uint16), rng.integers(0, 256, (P, h, w)).astype(np.uint8)


# ---- morphology ------------------------------------------------------------------------------------------------------------------------------
def morphology_frames(h, w, dtype):
    """P frames of the type: full-range noise with both ends of the range present, one of them constant"""
    import rank_cases

    rng = np.random.default_rng(h * 1000 + w + np.dtype(dtype).itemsize)
    fr = [rank_cases.full_range_image(rng, h, w, dtype) for _ in range(P - 1)]
    return np.stack(fr + [morphology_cases.constant_image(rng, h, w, dtype)])


# (op, size, (h, w)): the squares 3 and 7 on even widths take the pair kernel - two stages and a wider halo for the top hat -, an odd width
# or a rectangle the general one
def _morphology_cases():
    out = []
    for op in ("erode", "dilate", "tophat"):
        for size in (3, 7):
            out += [(op, size, s) for s in morph_pair_shapes(size, 2 if op == "tophat" else 1)]
        out += [(op, 3, s) for s in MORPH_GENERAL_SHAPES[1:]]  # the odd-width variant
        out += [(op, (3, 5), s) for s in [(2, 2)] + MORPH_GENERAL_SHAPES[1:]]
    return out


MORPHOLOGY_CASES = _morphology_cases()
MORPHOLOGY_DTYPES = (np.uint16, np.uint8)


def sizes_of(size):
    return (size, size) if isinstance(size, int) else size


# ---- rank filter and local statistics: walked by for_frame_chunks as morphology is ---------------------------------------------------------------
_rank, _local = source("rank_kernels.hip"), source("local_kernels.hip")
RT_TW, RT_TH = (int(x) for x in re.search(r"constexpr int RT_TW = (\d+), RT_TH = (\d+),", _rank).groups())
LOCAL_TY, LOCAL_HL = _pair(_local, ("LOCAL_TY", "LOCAL_HL"))
# (rank, size, (h, w)): the medians of 3 x 3 and 5 x 5 on even widths take the register kernels (16 and 8 rows a wave, one halo lane a side),
# another rank or an odd width the tile kernel
RANK_CASES = ([(4, 3, s) for s in [(2, 2), (2, 2 * 62 + 2), (4 * 16 + 1, 2)]] + [(12, 5, s) for s in [(2, 2 * 62 + 2), (4 * 8 + 1, 2)]] +
              [(2, 3, s) for s in [(2, 2), (2, RT_TW + 1), (RT_TH + 1, 3)]])
LOCAL_SHAPES = [(2, 2), (2, 2 * (64 - 2 * LOCAL_HL) + 2), (4 * LOCAL_TY + 1, 2), (2, 2 * (64 - 2 * LOCAL_HL) + 1)]  # the last: an odd width
LOCAL_THRESHOLD = dict(k=(1, 2), delta=5, polarity="both")


# ---- reconstruct ---------------------------------------------------------------------------------------------------------------------------
CORRIDOR_AT = 2  # 65 536 % 7: the last frame of the long stack is the corridor


def reconstruct_frames(h, w):
    """-> (mask, marker) uint16 [P][h][w]: levels_image masks under sparse markers; on frames wider than a tile, frame CORRIDOR_AT is a
    corridor over the full width, seeded at its left end only: the second tile learns of it in the second round"""
    rng = np.random.default_rng(4 + h * 100 + w)
    mask = np.stack([reconstruct_cases.levels_image(rng, h, w, "uint16") for _ in range(P)])
    marker = np.stack([reconstruct_cases.marker_image(rng, m, density=0.3) for m in mask])
    if w > REC_TW:
        mask[CORRIDOR_AT] = 1000
        marker[CORRIDOR_AT] = 0
        marker[CORRIDOR_AT, :, 0] = 700
    return mask, marker


H_DOME = 9000


# ---- distance transform ----------------------------------------------------------------------------------------------------------------------
def distance_frames(h, w):
    """P masks (uint8, foreground any non-zero value) of densities from sparse to nearly full"""
    rng = np.random.default_rng(h * 10 + w)
    dens = (0.15, 0.3, 0.45, 0.6, 0.75, 0.9, 0.5)
    return np.stack([np.where(rng.random((h, w)) < d, rng.integers(1, 256, (h, w)), 0) for d in dens]).astype(np.uint8)


# ---- temporal median -----------------------------------------------------------------------------------------------------------------------
def sliding_median(stack, window, threshold=0, rows=None, step=1):
    """test_temporal_median_cpu.temporal_median_oracle in one sort: the upper median of the window truncated at the ends of the stack"""
    from numpy.lib.stride_tricks import sliding_window_view

    n, h, w = stack.shape
    r = window // 2
    rows = h if rows is None else rows
    med = stack.copy()
    med[r:n - r] = np.sort(sliding_window_view(stack, window, axis=0), axis=-1)[..., r]
    for t in list(range(r)) + list(range(n - r, n)):
        lo, hi = max(0, t - r), min(n - 1, t + r)
        med[t] = np.sort(stack[lo:hi + 1], axis=0)[(hi - lo + 1) // 2]
    out = np.where(np.abs(stack.astype(np.int32) - med.astype(np.int32)) > threshold, med, stack)
    out[:, rows:] = stack[:, rows:]
    return np.ascontiguousarray(out[::step])


def temporal_distinct(h, w):
    """P frames over the whole range; along time the periodic stack gives every pixel a window of different values"""
    return np.random.default_rng(7 + h * 31 + w).integers(0, 65536, (P, h, w)).astype(np.uint16)


TEMPORAL_RUN_FRAMES = TM_GRID_Y * TM_RUN_MIN + 2 * TM_RUN_MIN + 3  # more than TM_GRID_Y runs of the shortest run, window 3


def host_periodic(distinct, n):
    """the periodic stack on the host - for the small frames of the entries whose frames are not independent"""
    return np.ascontiguousarray(distinct[np.arange(n) % P])


# ---- downsample ----------------------------------------------------------------------------------------------------------------------------
DOWNSAMPLE = dict(factor=2, factor_std=0.0, method=1)
DS_SLAB = constant(source("downsample_kernels.h"), "DS_SLAB")


def downsample_stack(n):
    """n frames of 1 x 8: pixel 0 swings about 32768 with an amplitude that grows frame by frame (and starts again every 20 000 frames), the
    others stand still - the statistic of a frame exceeds the lowest of the 96 before it, so with factor_std 0 method 1 keeps it"""
    i = np.arange(n)
    frames = np.empty((n, 1, 8), np.uint16)
    frames[:, 0, 1:] = np.array([7, 65535, 0, 40000, 123, 65534, 9], np.uint16)
    frames[:, 0, 0] = 32768 + np.where(i % 2 == 0, 1, -1) * (1 + i % 20000)
    return frames


def downsample_case():
    """-> (frames, time stamps, the oracle's Result): the shortest such stack that gives N kept images - segments - in one push.  (It is longer
    than N frames: while the history fills, the first 96 frames, only every other frame is kept.)"""
    import downsample_cases as DC

    frames = downsample_stack(N + 400)
    keep = DC.decide(DC.pair_sums(frames, 8), 8, **DOWNSAMPLE)[0]
    n = int(np.flatnonzero(np.cumsum(keep) == N)[0]) + 1
    frames = frames[:n]
    stamps = DC.stamps(n, step=3) + (np.arange(n) % 5 == 0)  # (uneven steps)
    return frames, stamps, DC.oracle(frames, stamps, lossy_height=1, **DOWNSAMPLE)


# ---- the region reducers -------------------------------------------------------------------------------------------------------------------
REGIONS = dict(h=3, w=5, k=4, percents=(0.0, 0.5, 1.0), nbins=8, lo=1000, width=8000, seed=60)


def region_case(per_frame):
    """-> (frames uint16 [P][3][5], labels int32 [3][5] or [P][3][5]) of test_region_quantiles_cpu.full_range_case"""
    from test_region_quantiles_cpu import full_range_case

    return full_range_case(REGIONS["seed"] + per_frame, P, REGIONS["h"], REGIONS["w"], REGIONS["k"], bool(per_frame))


def region_references(frames, labels):
    """{entry: {field: array [P][...]}} by the oracles of the test_region_*_cpu modules"""
    from test_region_geometry_cpu import region_geometry_oracle
    from test_region_histogram_cpu import region_histogram_oracle
    from test_region_quantiles_cpu import region_quantiles_oracle
    from test_region_stats_cpu import region_stats_oracle

    k, r = REGIONS["k"], REGIONS
    hist = region_histogram_oracle(frames, labels, k, r["lo"], r["width"], r["nbins"], rows=r["h"] - 1)
    whole = region_histogram_oracle(frames, None, 1, r["lo"], r["width"], r["nbins"], rows=r["h"] - 1)
    quant = region_quantiles_oracle(frames, labels, k, r["percents"])
    return {"region_stats": region_stats_oracle(frames, labels, k), "region_geometry": region_geometry_oracle(labels, k, frames),
            "region_histogram": dict(zip(("count", "hist", "outside"), hist)), "histogram": dict(zip(("count", "hist", "outside"), whole)),
            "region_quantiles": dict(zip(("count", "values"), quant))}


# ---- labelling -----------------------------------------------------------------------------------------------------------------------------
LABEL_FRAMES = 65535  # the largest count the labelling entries accept
LABEL_SHAPE = (2, 3)


def label_frames():
    """P uint16 frames of 2 x 3 in three levels, 0 the background: from no component to six"""
    fr = np.array([[[0, 0, 0], [0, 0, 0]], [[5, 5, 5], [5, 5, 5]], [[5, 0, 9], [0, 9, 0]], [[5, 9, 5], [9, 5, 9]], [[9, 9, 0], [0, 5, 5]],
                   [[0, 5, 0], [5, 5, 9]], [[9, 0, 0], [9, 9, 5]]], np.uint16)
    assert fr.shape == (P,) + LABEL_SHAPE
    return fr


def label_references(oracle, frames, foreground=6):
    """-> (labels [P][h][w], area [P][cap], xy [P][cap][2], counts [P], largest [P][h][w]) by the oracle, the tables padded with 0 to cap = h * w + 1"""
    cap = frames[0].size + 1
    labels, area, xy, counts, largest = [], np.zeros((P, cap), np.int32), np.zeros((P, cap, 2), np.float64), np.zeros(P, np.int32), []
    for i, f in enumerate(frames):
        lab, a, at = oracle.label_image(f, 0)
        labels.append(lab)
        area[i, :len(a)], xy[i, :len(a)], counts[i] = a, at, len(a)
        largest.append(oracle.keep_largest_area(f, 0, foreground))
    return np.stack(labels), area, xy, counts, np.stack(largest)


HOT_SPOTS = dict(low=30000, high=50000, min_area=2, max_area=5)


def hot_spot_frames():
    """P uint16 frames of 2 x 3 at both sides of the two thresholds: none, one and two kept components of other areas and first pixels, one
    too weak and one too small among them"""
    L, M, H, T = 30000, 30001, 50001, 65535  # background at the low threshold, foreground just above it, strong just above the high one
    fr = np.array([[[L, 0, L], [0, L, 0]], [[H, M, L], [L, L, L]], [[0, T, M], [L, 0, L]], [[H, M, M], [L, L, L]], [[H, L, T], [M, 0, M]],
                   [[M, M, L], [L, H, H]], [[M, M, L], [T, L, H]]], np.uint16)
    assert fr.shape == (P,) + LABEL_SHAPE
    return fr
