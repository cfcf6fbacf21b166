"""GPU: the two walks over labelled pixels of csrc/region_walk.h at their own boundaries - walk_regions, which region_stats and
region_geometry share, and walk_counters, which region_quantiles, region_histogram and histogram share: item and step edges, the
pixel-by-pixel loads, label changes at every offset of a thread's 8 pixels, the wave-wide flush on both sides of geometry's threshold,
labels outside the range at a flush - in both forms of each reducer.  Every reducer runs on the same inputs, bit for bit against its
oracle; the histogram also without a map, on the same frames, and over the map of zeros that is its twin."""
import os
import re

import numpy as np
import pytest

from test_region_geometry_cpu import FIELDS as GEOMETRY_FIELDS, region_geometry_oracle
from test_region_histogram_cpu import region_histogram_oracle
from test_region_quantiles_cpu import region_quantiles_oracle
from test_region_stats_cpu import FIELDS as STATS_FIELDS, region_stats_oracle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "librir_amd", "csrc", "quantile_kernels.h")) as _f:
    QUANTILE_LDS_MAX = int(re.search(r"constexpr int QUANTILE_LDS_MAX = (\d+);", _f.read()).group(1))
# one region more than the LDS form takes: of quantiles (its high-byte pass, and twice that; with three percents the low-byte pass is past
# it from 22 regions), of geometry (geometry_kernels.h GEOMETRY_LDS_MAX) and of statistics (region_kernels.h REGION_LDS_MAX)
GLOBAL_FORMS = (QUANTILE_LDS_MAX + 1, 2 * QUANTILE_LDS_MAX + 1, 1024 + 1, 4096 + 1)
PERCENTS = (0.0, 0.5, 1.0)
BINNINGS = ((0, 256, 256), (1, 7, 255))
HISTOGRAM_FIELDS = ("count", "hist", "outside")
N = 2
INT32_MIN = -(2 ** 31)
STEP = 2048  # pixels per workgroup and step: 256 threads x 8 pixels; an item is 8 steps


def dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda().view(torch.uint16)


def dev32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()


def frames_of(h, w, seed):
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 65536, (N, h, w), dtype=np.uint16)
    f.reshape(N, -1)[:, ::7] = 0
    f.reshape(N, -1)[:, 3::11] = 65535
    return f


def same(fields, got, exp, what):
    for k, t in zip(fields, got):
        e = exp[k]
        if e is None:
            assert t is None, (what, k)
            continue
        g = t.cpu().numpy()
        assert g.dtype == e.dtype and g.shape == e.shape, (what, k, g.dtype, g.shape)
        if not np.array_equal(g, e):
            bad = np.argwhere(g != e)[:5]
            raise AssertionError("%s %s differs at %s: got %s, expected %s" % (what, k, bad.tolist(), g[tuple(bad.T)], e[tuple(bad.T)]))


def all_reducers(frames, labels, ks=(3,), what="", tensors=None):
    """statistics, geometry (weighted and labels only), quantiles and histograms of `frames` over `labels` with k regions, for every k,
    against the oracles, and the histograms of `frames` without a map and over a map of zeros; tensors: the (frames, labels) device tensors
    to pass, where a test made its own"""
    from librir_amd import device as D

    f, lab = tensors if tensors is not None else (dev16(frames), dev32(labels))
    for k in ks:
        same(STATS_FIELDS, D.region_stats(f, lab, k), region_stats_oracle(frames, labels, k), (what, k, "stats"))
        same(GEOMETRY_FIELDS, D.region_geometry(lab, k, f), region_geometry_oracle(labels, k, frames), (what, k, "geometry, weighted"))
        same(GEOMETRY_FIELDS, D.region_geometry(lab, k), region_geometry_oracle(labels, k), (what, k, "geometry, labels only"))
        exp = dict(zip(("count", "values"), region_quantiles_oracle(frames, labels, k, PERCENTS)))
        same(("count", "values"), D.region_quantiles(f, lab, PERCENTS, k), exp, (what, k, "quantiles"))
        for lo, width, nbins in BINNINGS:
            exp = dict(zip(HISTOGRAM_FIELDS, region_histogram_oracle(frames, labels, k, lo, width, nbins)))
            same(HISTOGRAM_FIELDS, D.region_histogram(f, lab, nbins, lo, width, k)[:3], exp, (what, k, "histogram", lo, width, nbins))
    zeros = torch.zeros(tuple(f.shape[-2:]), dtype=torch.int32, device="cuda")
    for lo, width, nbins in BINNINGS:
        exp = dict(zip(HISTOGRAM_FIELDS, region_histogram_oracle(frames, None, 1, lo, width, nbins)))
        same(HISTOGRAM_FIELDS, D.histogram(f, nbins, lo, width)[:3], exp, (what, "histogram, no map", lo, width, nbins))
        same(HISTOGRAM_FIELDS, D.region_histogram(f, zeros, nbins, lo, width, 1)[:3], exp, (what, "histogram, a map of zeros", lo, width, nbins))


@pytest.mark.parametrize("h,w", [(127, 129), (128, 128), (5, 3277), (3, 10923), (1, 2047), (1, 2048), (1, 2049), (8, 257)])
def test_item_and_step_edges(h, w):
    """16 383, 16 384, 16 385 and 32 769 pixels end one short of, at and one past the edge of an item (only 128 x 128 takes the vector
    loads); 2047, 2048, 2049 and 2056 pixels do the same at the edge of a step inside one"""
    f = frames_of(h, w, seed=w)
    runs = (np.arange(h * w) // 1000 % 4 - 1).astype(np.int32).reshape(h, w)  # runs of 1000 pixels that cross every edge, one of them of -1
    all_reducers(f, runs, what=("runs", h, w))
    per = np.random.default_rng(h).integers(-1, 4, (N, h, w)).astype(np.int32)  # a change at most pixels, a map per frame
    all_reducers(f, per, what=("per-frame", h, w))


def test_pixel_by_pixel_loads_of_an_unaligned_stack():
    """a multiple of 8 pixels, so only the data pointers - 2 bytes past a 16-byte boundary for the frames, 4 for the labels - turn the
    vector loads off"""
    h, w = 40, 64
    f = frames_of(h, w, seed=1)
    lab = np.random.default_rng(1).integers(-1, 4, (h, w)).astype(np.int32)
    f_off = dev16(np.concatenate([[9], f.reshape(-1)]).astype(np.uint16))[1:].view(N, h, w)
    lab_off = dev32(np.concatenate([[7], lab.reshape(-1)]))[1:].view(h, w)
    assert f_off.data_ptr() % 16 == 2 and lab_off.data_ptr() % 16 == 4
    all_reducers(f, lab, what="frames off", tensors=(f_off, dev32(lab)))
    all_reducers(f, lab, what="labels off", tensors=(dev16(f), lab_off))


def test_label_changes_at_every_offset_of_a_thread():
    h, w = 16, 264  # 4224 pixels: two full steps and a checked one; 264 = 33 x 8, so the rows shift against the threads' 8 pixels
    f = frames_of(h, w, seed=2)
    x = np.arange(h * w)
    for width in (1, 3, 8, 9):
        all_reducers(f, (x // width % 3).astype(np.int32).reshape(h, w), what=("stripes", width))
    for j in range(8):
        lab = np.zeros(h * w, np.int32)
        lab[8 * 300 + j] = 1  # thread 44 of the second step
        all_reducers(f, lab.reshape(h, w), what=("one pixel", j))


@pytest.mark.parametrize("m", [1, 31, 32, 63, 64])
def test_wave_wide_flush_on_both_sides_of_the_geometry_threshold(m):
    """two steps of one workgroup.  m lanes of the first wave meet a new label in their second 8 pixels, at the same point: statistics adds
    their runs across the wave from one lane up, geometry from 32.  In both forms of every reducer."""
    h, w = 2, STEP
    f = frames_of(h, w, seed=m)
    lab = np.zeros((h, w), np.int32)
    lab[1, :8 * m] = 1
    all_reducers(f, lab, (3,) + GLOBAL_FORMS[-1:], ("one new label", m))
    lab[1, :8 * m:16] = 2  # every other of the m lanes: the runs open at the end of the item do not all have one label
    all_reducers(f, lab, (3,) + GLOBAL_FORMS[-1:], ("two new labels", m))
    lab[0, :8 * 64] = np.repeat(np.arange(64) % 2 + 1, 8)  # the first wave's lanes alternate 1, 2 in the first step
    lab[1, :8 * 64] = 0  # ... and m of them, or all 64, flush runs of two labels at one point
    lab[1, 8 * m:8 * 64] = lab[0, 8 * m:8 * 64]
    all_reducers(f, lab, (3,) + GLOBAL_FORMS[-1:], ("two old labels", m))


@pytest.mark.parametrize("bad", [-1, 3, INT32_MIN])
def test_labels_outside_the_range_at_a_flush(bad):
    """the run that is flushed, the run that starts, or both, belong to no region: whole waves of them (the label is dropped once for the
    wave) and 20 lanes (each lane drops its own); INT32_MIN is also the label of a thread's run before its first pixel"""
    h, w = 2, STEP
    f = frames_of(h, w, seed=5)
    other = {-1: INT32_MIN, 3: -1, INT32_MIN: 3}[bad]
    for before, after in ((bad, 0), (0, bad), (bad, other)):
        lab = np.full((h, w), before, np.int32)
        lab[1] = after
        all_reducers(f, lab, what=("rows", before, after))
        lab = np.zeros((h, w), np.int32)
        lab[0, :8 * 20], lab[1, :8 * 20] = before, after
        all_reducers(f, lab, what=("20 lanes", before, after))
        lab[1, 8 * 20 + 3] = bad  # and one pixel inside a thread's 8
        all_reducers(f, lab, what=("one pixel", before, after))


@pytest.mark.parametrize("k", GLOBAL_FORMS)
def test_global_forms_with_labels_from_the_whole_range(k):
    """one more region than the LDS form of quantiles, geometry and statistics takes: short runs of every label, a few outside"""
    h, w = 40, 97
    f = frames_of(h, w, seed=k)
    rng = np.random.default_rng(k)
    all_reducers(f, rng.integers(-2, k + 2, (h, w)).astype(np.int32), (k,), "shared")
    all_reducers(f, np.repeat(rng.integers(-2, k + 2, (N, h * w // 5)), 5, 1).astype(np.int32).reshape(N, h, w), (k,), "per-frame runs of 5")
