"""GPU: region_histogram, histogram and region_quantiles where a workgroup of walk_counters (csrc/region_walk.h) walks several items and
passes from frame to frame - the cases of region_walk_cases.py, built for the CU count of the device, bit for bit against the numpy oracles
of test_region_histogram_cpu.py and test_region_quantiles_cpu.py.  What the walk carries across work is what is under test: the open run
that is closed at a frame change, the drain before frame() repoints the counters, the sum of the LDS copies and their reset, the codes the
low-byte pass caches.  The statistics and the geometry of the same stacks, whose grid-stride walk meets more items than workgroups the same
way, against their oracles; the same call twice; the raw entries on outputs and workspaces filled with garbage."""
import ctypes as ct

import numpy as np
import pytest

import region_walk_cases as W
from test_region_geometry_cpu import FIELDS as GEOMETRY_FIELDS, region_geometry_oracle
from test_region_histogram_cpu import DEVICE_ARGS as HISTOGRAM_ARGS, region_histogram_oracle
from test_region_quantiles_cpu import frame_bytes, region_quantiles_oracle
from test_region_stats_cpu import FIELDS as STATS_FIELDS, region_stats_oracle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

QUANTILES_ARGS = [ct.c_void_p, ct.c_void_p] + [ct.c_int] * 5 + [ct.c_void_p, ct.c_int] + [ct.c_void_p] * 3 + [ct.c_size_t, ct.c_void_p]
CASE_MAPS = [(c, m) for c in W.CASES for m in c.maps]
IDS = ["%s, %s" % (c.name, m) for c, m in CASE_MAPS]


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda().view(torch.uint16)


def dev32(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()


def same(names, got, exp, what):
    for name, t, e in zip(names, got, exp):
        g = t.cpu().numpy()
        assert g.dtype == e.dtype and g.shape == e.shape, (what, name, g.dtype, g.shape, e.shape)
        if not np.array_equal(g, e):
            bad = np.argwhere(g != e)
            raise AssertionError("%s %s differs at %d places, the first at %s: got %s, expected %s"
                                 % (what, name, len(bad), bad[:5].tolist(), g[tuple(bad[:5].T)], e[tuple(bad[:5].T)]))


def conditions(case, n, cus, work_bytes=None):
    """the model's answer for this device: the walk the case is there for happens, or the test fails"""
    for name, per, items, grid in W.launches(case, n, cus, work_bytes):
        walk = W.walk_of(per, items, grid)
        if name in case.shallow:
            continue
        assert items > 3 * grid, (case.name, name, items, grid)
        if per == 1:
            assert walk.touches >= 3, (case.name, name, walk)
        else:
            assert walk.begins_inside and walk.ends_inside and walk.whole_between and walk.ragged, (case.name, name, walk)
    if case.op == "hist":
        assert W.histogram_lds_bytes(case.k, case.bins[2])[1] == case.copies


def expected(case, frames, labels):
    if case.op == "hist":
        return W.in_chunks(region_histogram_oracle, frames, labels, case.k, *case.bins, case.rows)
    return W.in_chunks(region_quantiles_oracle, frames, labels, case.k, case.percents)


def run(case, f, lab):
    from librir_amd import device as D

    if case.op == "quant":
        return tuple(D.region_quantiles(f, lab, case.percents, case.k))
    lo, width, nbins = case.bins
    got = D.histogram(f, nbins, lo, width, case.rows) if lab is None else D.region_histogram(f, lab, nbins, lo, width, case.k, case.rows)
    return got.count, got.hist, got.outside


def names(case):
    return ("count", "hist", "outside") if case.op == "hist" else ("count", "values")


@pytest.mark.parametrize("case,maps", CASE_MAPS, ids=IDS)
def test_counts_where_a_workgroup_walks_many_items_and_frames(case, maps, cus):
    frames, labels = W.make_inputs(case, cus, maps)
    conditions(case, frames.shape[0], cus)
    same(names(case), run(case, dev16(frames), dev32(labels)), expected(case, frames, labels), (case.name, maps))


@pytest.mark.parametrize("maps", W.BOTH)
@pytest.mark.parametrize("name", ["A 3x5 hist 4 copies", "A 32x64 hist 4 copies"])
def test_statistics_and_geometry_of_the_same_stacks(name, maps, cus):
    """walk_regions strides over the items by the grid: on these stacks every workgroup takes three items or four, of as many frames"""
    from librir_amd import device as D

    case = W.by_name(name)
    frames, labels = W.make_inputs(case, cus, maps)
    assert frames.shape[0] > 3 * W.WALK_BLOCKS_PER_CU * cus
    f, lab = dev16(frames), dev32(labels)
    exp = W.in_chunks(region_stats_oracle, frames, labels, case.k)
    same(STATS_FIELDS, D.region_stats(f, lab, case.k), [exp[x] for x in STATS_FIELDS], (name, maps, "stats"))
    exp = W.in_chunks(lambda fr, lb, k: region_geometry_oracle(lb, k, fr), frames, labels, case.k)
    same(GEOMETRY_FIELDS, D.region_geometry(lab, case.k, f), [exp[x] for x in GEOMETRY_FIELDS], (name, maps, "geometry, weighted"))


@pytest.mark.parametrize("name,maps", [("A 32x64 hist 4 copies", "per-frame"), ("B 129x128 hist light LDS", "none"),
                                       ("B 129x128 quant 64 regions", "shared")])
def test_the_same_call_twice_gives_the_same_tensors(name, maps, cus):
    case = W.by_name(name)
    frames, labels = W.make_inputs(case, cus, maps)
    conditions(case, frames.shape[0], cus)
    f, lab = dev16(frames), dev32(labels)
    first, second = run(case, f, lab), run(case, f, lab)
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    same(names(case), second, expected(case, frames, labels), (name, maps))


@pytest.mark.parametrize("name,maps", [("A 32x64 hist 4 copies", "shared"), ("B 129x128 hist 16 432 counters", "per-frame")])
def test_the_histogram_entry_clears_outputs_filled_with_garbage(lib, name, maps, cus):
    case = W.by_name(name)
    frames, labels = W.make_inputs(case, cus, maps)
    n, h, w = frames.shape
    conditions(case, n, cus)
    f, lab = dev16(frames), dev32(labels)
    lo, width, nbins = case.bins
    fn = lib.rir_region_histogram_device
    fn.argtypes = HISTOGRAM_ARGS
    out = [torch.full(shape, fill, dtype=torch.int32, device="cuda") for shape, fill in (((n, case.k), -7), ((n, case.k, nbins), 0x01010101), ((n, case.k, 2), -1))]
    work = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    stream = ct.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert fn(f.data_ptr(), lab.data_ptr(), w, h, h, n, int(maps == "per-frame"), case.k, lo, width, nbins, *(t.data_ptr() for t in out), work.data_ptr(), 8,
              stream) == 0
    same(names(case), out, expected(case, frames, labels), (name, maps, "raw entry"))


@pytest.mark.parametrize("name,maps", [("A 32x64 quant three percents", "per-frame"), ("B 129x128 quant 64 regions", "shared")])
def test_the_quantile_entry_on_workspaces_filled_with_garbage(lib, name, maps, cus):
    """a workspace for the whole stack in one group, and one whose groups do not divide the stack"""
    case = W.by_name(name)
    frames, labels = W.make_inputs(case, cus, maps)
    n, h, w = frames.shape
    f, lab = dev16(frames), dev32(labels)
    pc = np.array(case.percents, np.float32)
    b = frame_bytes(case.k, pc.size)
    fn = lib.rir_region_quantiles_device
    fn.argtypes = QUANTILES_ARGS
    exp = expected(case, frames, labels)
    stream = ct.c_void_p(torch.cuda.current_stream().cuda_stream)
    group = 2 * n // 5 + 1
    assert n % group != 0 and W.quantile_groups(n, case.k, pc.size, group * b + 8) == [group, group, n - 2 * group]
    conditions(case, n, cus, n * b)
    for size in (n * b, group * b + 8):
        work = torch.full((size // 8,), -1, dtype=torch.int64, device="cuda")
        count = torch.full((n, case.k), -7, dtype=torch.int32, device="cuda")
        values = torch.full((n, case.k, pc.size), -7, dtype=torch.int32, device="cuda")
        assert fn(f.data_ptr(), lab.data_ptr(), w, h, n, int(maps == "per-frame"), case.k, pc.ctypes.data, pc.size, count.data_ptr(), values.data_ptr(),
                  work.data_ptr(), size, stream) == 0
        same(names(case), (count, values), exp, (name, maps, "workspace of %d frames" % (size // b)))
