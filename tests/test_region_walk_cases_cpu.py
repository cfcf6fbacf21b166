"""CPU: the cases of region_walk_cases.py do what test_gpu_counting_walk.py needs of them on 32 to 256 CUs - every counting launch gives a
workgroup more than three items, case A three frames or more, case B ranges that are cut inside frames - the model of the launch shape is
the source's, line by line, so that a change to walk_launch_shape or to a launcher's LDS use fails here and does not quietly turn the GPU
tests back into walks of one item; and the oracles take every case at 256 CUs."""
import re

import numpy as np
import pytest

import region_walk_cases as W
from test_region_histogram_cpu import region_histogram_oracle
from test_region_quantiles_cpu import frame_bytes, region_quantiles_oracle

CASE_MAPS = [(c, m) for c in W.CASES for m in c.maps]
IDS = ["%s, %s" % (c.name, m) for c, m in CASE_MAPS]


def test_the_constants_are_the_headers():
    assert (W.WALK_ITEM, W.WALK_BLOCKS_PER_CU, W.WALK_LDS_BYTES) == (16384, 8, 160 * 1024)
    assert (W.HISTOGRAM_LDS_MAX, W.HISTOGRAM_COPY_MAX, W.HISTOGRAM_MAX_COPIES, W.QUANTILE_LDS_MAX) == (16384, 5120, 8, 64)
    assert W.QUANTILE_WORK_BYTES == 256 << 20
    assert W.constant("constexpr int A = 3 * 5;\nconstexpr size_t B = (size_t)3 << 4;", "A") == 15
    assert W.constant("constexpr int A = 3 * 5;\nconstexpr size_t B = (size_t)3 << 4;", "B") == 48


def test_the_model_is_the_source():
    """the lines that define what launch_shape, ranges, histogram_lds_bytes, quantile_lds_bytes and quantile_groups restate"""
    walk, hist, quant, abi = (W.source(x) for x in ("region_walk.h", "histogram_kernels.hip", "quantile_kernels.hip", "signal_processing_abi.cpp"))
    for text, lines in ((walk, [
        "s.per_item_frame = (int)((npx + WALK_ITEM - 1) / WALK_ITEM);",
        "s.items = (int64_t)n * s.per_item_frame;",
        "const size_t fit = lds_bytes_per_block ? std::max<size_t>(1, WALK_LDS_BYTES / lds_bytes_per_block) : WALK_BLOCKS_PER_CU;",
        "s.grid = (unsigned)std::min<int64_t>(s.items, (int64_t)cus * (int64_t)std::min<size_t>(WALK_BLOCKS_PER_CU, fit));",
        "const int64_t first = (int64_t)blockIdx.x * items / gridDim.x, last = ((int64_t)blockIdx.x + 1) * items / gridDim.x;",
        "const int64_t fi = item < last ? item / per_item_frame : -1;",
    ]), (hist, [
        "const int64_t total = (int64_t)nregions * (nbins + 3);",
        "const int lds_n = (int)std::min<int64_t>(total, HISTOGRAM_LDS_MAX);",
        "while ((2 << cshift) <= HISTOGRAM_MAX_COPIES && (total << (cshift + 1)) <= HISTOGRAM_COPY_MAX)",
        "const size_t lds = ((size_t)lds_n << cshift) * 4;",
        "const WalkShape s = walk_launch_shape(npx, n, lds, cus);",
        "walk_counters(pol, npx, items, per_item_frame);",
    ]), (quant, [
        "const size_t lds = (size_t)std::min<int64_t>((int64_t)nregions * (LOW ? nq : 1), QUANTILE_LDS_MAX) * 1024;",
        "const WalkShape s = walk_launch_shape(npx, n, lds, cus);",
        "const int group = (int)std::min<size_t>((size_t)n, work_bytes / frame_bytes);",
        "return (size_t)nregions * (1024 + 16 + (size_t)npercents * (8 + 1024));",
        "launch_count<false>(f, l, npx, g, per_frame, nregions, npercents, cus, nullptr, hist_hi, st);",
        "launch_count<true>(f, l, npx, g, per_frame, nregions, npercents, cus, codes, hist_lo, st);",
        "walk_counters(pol, npx, items, per_item_frame);",
    ]), (abi, [
        "return B * std::min<size_t>((size_t)std::max(nframes, 1), std::max<size_t>(1, QUANTILE_WORK_BYTES / B));",
    ])):
        for line in lines:
            assert line in text, line
    assert frame_bytes(7, 3) == 7 * (1024 + 16 + 3 * (8 + 1024))


def test_the_model_on_shapes_counted_by_hand():
    assert W.launch_shape(640 * 512, 1000, 0, 256) == (20, 20000, 2048)
    assert W.launch_shape(640 * 512, 1000, 64 * 1024, 256) == (20, 20000, 512)
    assert W.launch_shape(640 * 512, 1000, 200 * 1024, 256) == (20, 20000, 256)  # more LDS than half a CU's: still one workgroup a CU
    assert W.launch_shape(16385, 3, 1024, 256) == (2, 6, 6)
    assert W.histogram_lds_bytes(1, 256) == (259 * 8 * 4, 8) and W.histogram_lds_bytes(3, 256) == (777 * 4 * 4, 4)
    assert W.histogram_lds_bytes(9, 256) == (2331 * 2 * 4, 2) and W.histogram_lds_bytes(10, 256) == (2590 * 4, 1)
    assert W.histogram_lds_bytes(5, 4096) == (65536, 1) and W.histogram_lds_bytes(16, 1024) == (65536, 1)
    assert W.quantile_lds_bytes(3, 3, False) == 3072 and W.quantile_lds_bytes(3, 3, True) == 9216
    assert W.quantile_lds_bytes(9, 8, False) == 9216 and W.quantile_lds_bytes(9, 8, True) == 65536 and W.quantile_lds_bytes(65, 1, False) == 65536
    assert W.quantile_groups(10, 3, 3) == [10] and W.quantile_groups(10, 3, 3, 4 * frame_bytes(3, 3) + 8) == [4, 4, 2]
    assert W.quantile_groups(3000, 65, 3) == [998, 998, 998, 6]
    first, last = W.ranges(7, 3)
    assert first.tolist() == [0, 2, 4] and last.tolist() == [2, 4, 7]
    assert list(W.frames_in((2, 4), 3)) == [0, 1] and list(W.frames_in((3, 6), 3)) == [1] and list(W.frames_in((5, 13), 3)) == [1, 2, 3, 4]
    # 14 items of two to a frame over 4 workgroups: [0, 3) [3, 7) [7, 10) [10, 14)
    assert W.walk_of(2, 14, 4) == W.Walk(True, 2, True, True, True, True)
    assert W.walk_of(2, 16, 4) == W.Walk(True, 2, False, False, False, False)
    assert W.walk_of(1, 13, 4) == W.Walk(True, 3, False, False, False, True)


def test_the_case_list_is_the_one_asked_for():
    names = [c.name for c in W.CASES]
    assert len(set(names)) == len(names) == 2 * 8 + 2 * 2 + 1 + 2 + 2
    for c in W.CASES:
        assert (c.op == "hist") == (c.bins is not None) and (c.op == "quant") == (c.percents is not None), c.name
        assert c.labelled or (c.k == 1 and c.maps == ("none",)), c.name
        assert c.group in "CD" or c.maps in (W.BOTH, ("none",)), c.name
    a = [c for c in W.CASES if c.group == "A"]
    assert sorted({(c.h, c.w) for c in a}) == [(3, 5), (32, 64)]
    assert {(c.op, c.k, c.bins, c.percents, c.scene, c.n) for c in a} == {
        ("hist", 1, (0, 256, 256), None, "full", "8"), ("hist", 3, (0, 256, 256), None, "full", "8"), ("hist", 3, (7960, 1, 81), None, "static", "8"),
        ("quant", 3, None, (0.0, 0.5, 1.0), "full", "8"), ("hist", 5, (0, 16, 4096), None, "full", "2"), ("quant", 65, None, (0.5,), "full", "2"),
        ("quant", 9, None, W.EIGHT_PERCENTS, "full", "2")}
    assert 5 * (4096 + 3) == 20495 and len(W.EIGHT_PERCENTS) == 8
    b = [c for c in W.CASES if c.group == "B"]
    assert all(c.n == "model" for c in b) and sorted({(c.h, c.w) for c in b}) == [(129, 128), (160, 256)]
    assert all(c.k * (c.bins[2] + 3) >= W.HISTOGRAM_LDS_MAX for c in b if c.op == "hist" and c.labelled)
    assert all(c.k >= W.QUANTILE_LDS_MAX for c in b if c.op == "quant")
    for c in (x for x in W.CASES if x.group == "D"):
        assert c.rows == c.h - 3 and c.op == "hist"


@pytest.mark.parametrize("cus", W.CUS)
def test_every_launch_walks_more_than_three_items_a_workgroup(cus):
    """and the stack lengths are the issue's: 3 * 8 * cus + 7, 3 * 2 * cus + 7 where a launch holds two workgroups a CU"""
    for c in W.CASES:
        n = W.frames_of(c, cus)
        assert c.n == "model" or n == 3 * int(c.n) * cus + 7
        ls = W.launches(c, n, cus)
        assert len(ls) == (1 if c.op == "hist" else 2), (c.name, ls)  # device.region_quantiles takes the stack in one group
        for name, per, items, grid in ls:
            assert items == n * per and (items > 3 * grid) == (name not in c.shallow), (c.name, name, items, grid)
            if c.n == "2" and name not in c.shallow or (c.group in "BD" and c.n == "model" and c.labelled):
                assert grid == 2 * cus, (c.name, name, grid)
            if c.n == "8":
                assert grid == 8 * cus, (c.name, name, grid)
        if c.op == "hist":
            assert W.histogram_lds_bytes(c.k, c.bins[2])[1] == c.copies, c.name
        assert [x.name for x in W.CASES if x.shallow] == ["A 3x5 quant eight percents", "A 32x64 quant eight percents"]


@pytest.mark.parametrize("cus", W.CUS)
def test_case_a_ranges_touch_three_frames_or_more(cus):
    for c in (x for x in W.CASES if x.group in "AC" or x.name == "D 32x64 rows"):
        for name, per, items, grid in W.launches(c, W.frames_of(c, cus), cus):
            walk = W.walk_of(per, items, grid)
            assert per == 1 and (name in c.shallow or walk.touches >= 3), (c.name, name, walk)
            first, last = W.ranges(items, grid)
            assert name in c.shallow or min(len(W.frames_in((int(a), int(b)), per)) for a, b in zip(first[:50], last[:50])) >= 3


@pytest.mark.parametrize("cus", W.CUS)
def test_case_b_ranges_are_cut_inside_frames(cus):
    for c in (x for x in W.CASES if x.group == "B" or x.name == "D 160x256 rows"):
        n = W.frames_of(c, cus)
        for name, per, items, grid in W.launches(c, n, cus):
            walk = W.walk_of(per, items, grid)
            assert per == {129: 2, 160: 3}[c.h], c.name
            assert walk.deep and walk.begins_inside and walk.ends_inside and walk.whole_between and walk.ragged, (c.name, name, walk)
            assert items % grid != 0 and (items / grid) % per != 0
            first, last = (x.tolist() for x in W.ranges(items, grid))
            assert first[0] == 0 and last[-1] == items and first[1:] == last[:-1]
            # by the definition: a range that begins and ends inside frames and holds every item of some frame between
            assert any(a % per and b % per and any(a <= f * per and (f + 1) * per <= b for f in W.frames_in((a, b), per)) for a, b in zip(first, last))
        assert n * c.h * c.w <= 52e6, (c.name, n)
    assert W.walked_pixels(W.by_name("B 129x128 hist light LDS")) - W.WALK_ITEM == 128  # the second item: one checked step of 128 pixels
    assert W.walked_pixels(W.by_name("B 160x256 quant 64 regions")) - 2 * W.WALK_ITEM == W.WALK_ITEM // 2
    d = W.by_name("D 160x256 rows")
    assert W.walked_pixels(d) < d.h * d.w and W.launch_shape(W.walked_pixels(d), 1, 0, 256)[0] == 3


def test_case_c_frames_choose_other_buckets():
    """consecutive frames keep all their pixels in one high byte, and not the same one: codes cached from the frame before would count none"""
    for name, maps in (("C one label", "zeros"), ("C three stripes", "stripes")):
        frames, labels = W.make_inputs(W.by_name(name), 32, maps)
        hi = frames >> 8
        assert (hi.reshape(len(hi), -1) == hi[:, :1, 0]).all() and (hi[1:, 0, 0] != hi[:-1, 0, 0]).all()
        assert labels.shape == (32, 64) and sorted(np.unique(labels).tolist()) == list(range(W.by_name(name).k))


@pytest.mark.parametrize("case,maps", CASE_MAPS, ids=IDS)
def test_the_oracles_take_every_case_at_256_cus(case, maps):
    """the inputs are what the case list says - labels from -1 to k, frames and per-frame maps that differ - and the oracle's counts are the
    labelled pixels of every frame"""
    frames, labels = W.make_inputs(case, 256, maps)
    n, k, rows = W.frames_of(case, 256), case.k, case.rows
    assert frames.shape == (n, case.h, case.w) and frames.dtype == np.uint16
    if labels is None:
        inside = np.full((n, 1), W.walked_pixels(case))
    else:
        assert labels.dtype == np.int32 and labels.shape == ((n, case.h, case.w) if maps == "per-frame" else (case.h, case.w))
        lab = np.broadcast_to(labels, frames.shape)[:, :rows].reshape(n, -1)
        if case.group != "C":
            assert lab.min() == -1 and lab.max() == k
        inside = np.stack([(lab == r).sum(1) for r in range(min(k, 4))], 1)
    if rows is not None:
        below_l, below_v = np.broadcast_to(labels, frames.shape)[:, rows:], frames[:, rows:]
        lo, width, nbins = case.bins
        assert ((below_l >= 0) & (below_l < k) & (below_v >= lo) & (below_v < lo + width * nbins)).any(axis=(1, 2)).all()
    if case.op == "hist":
        count, hist, outside = W.in_chunks(region_histogram_oracle, frames, labels, k, *case.bins, rows)
        assert hist.shape == (n, k, case.bins[2]) and np.array_equal(count, hist.sum(-1) + outside.sum(-1))
        if case.scene == "static":
            assert (hist.sum((0, 1)) > 0).all() and outside.sum() > 0  # every level is met, and the pixels that break the runs
    else:
        count, values = W.in_chunks(region_quantiles_oracle, frames, labels, k, case.percents)
        assert values.shape == (n, k, len(case.percents)) and (values[count > 0] >= 0).all()
    assert np.array_equal(count[:, :4], inside)
