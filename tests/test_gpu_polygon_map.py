"""GPU: polygon label maps, bit for bit against the oracle of polygon_cases.py (which test_polygon_map_cpu.py pins to the reference's own
maps) - every case through device.polygon_map, signal_processing.polygon_map and the raw C entry, into memory pre-filled with garbage, twice;
the host entry across slabs, packed tensors, out= at every alignment, a side stream, refused arguments, and IRMovie.polygon_stats with shared
and moving regions."""
import ctypes as ct
import functools

import numpy as np
import pytest

import polygon_cases as PC
from test_gpu_region_stats import check, record
from test_region_stats_cpu import region_stats_oracle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

CASES = PC.cases()
GARBAGE = 0x5A5A5A5A


@functools.lru_cache(maxsize=None)
def expected(name):
    out = PC.oracle(CASES[name])
    out.setflags(write=False)
    return out


def differs(got, exp, what):
    bad = np.argwhere(got != exp)[:5]
    return "%s differs at %s: got %s, expected %s" % (what, bad.tolist(), got[tuple(bad.T)], exp[tuple(bad.T)])


def raw_entry(lib):
    fn = lib.rir_polygon_map_device
    fn.argtypes = [ct.c_void_p] * 3 + [ct.c_int] * 4 + [ct.c_void_p] + [ct.c_int] * 3 + [ct.c_void_p, ct.c_void_p, ct.c_size_t, ct.c_void_p]
    lib.rir_polygon_map_workspace_bytes.argtypes = [ct.c_int] * 5
    lib.rir_polygon_map_workspace_bytes.restype = ct.c_size_t
    return fn


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_route_equals_the_oracle(lib, name):
    from librir_amd import device as D
    from librir_amd import signal_processing as S

    case = CASES[name]
    polygons, shape, kw, out_shape = PC.api_args(case)
    exp = expected(name).reshape(out_shape)
    got = D.polygon_map(polygons, shape, **kw)
    assert got.dtype == torch.int32 and got.is_cuda and tuple(got.shape) == out_shape
    first = got.cpu().numpy()
    assert np.array_equal(first, exp), differs(first, exp, "device.polygon_map")
    # out= reused, holding garbage: every pixel is written, and the second run gives the same bits
    out = torch.full(out_shape, GARBAGE, dtype=torch.int32, device="cuda")
    assert D.polygon_map(polygons, shape, out=out, **kw) is out
    assert np.array_equal(out.cpu().numpy(), first)
    out.fill_(-GARBAGE)
    D.polygon_map(polygons, shape, out=out, **kw)
    assert np.array_equal(out.cpu().numpy(), first)
    host = S.polygon_map(polygons, shape, **kw)
    assert isinstance(host, np.ndarray) and host.dtype == np.int32 and host.shape == out_shape
    assert np.array_equal(host, exp), differs(host, exp, "signal_processing.polygon_map")
    # the raw entry on the packed arrays
    a = D._polygon_map_args(polygons, shape, **kw)
    xy, npts, values, shifts = D._polygon_inputs(a, torch.device("cuda"))
    fn = raw_entry(lib)
    need = lib.rir_polygon_map_workspace_bytes(a.w, a.h, a.nmaps, a.npoly, a.max_pts)
    assert need > 0
    work = torch.full((need // 8 + 1,), -1, dtype=torch.int64, device="cuda")
    dst = torch.full((a.nmaps, a.h, a.w), GARBAGE, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = fn(xy.data_ptr(), npts.data_ptr(), values.data_ptr() if values is not None else None, a.npoly, a.max_pts, a.nmaps, a.per_map,
            shifts.data_ptr() if shifts is not None else None, a.w, a.h, case["background"], dst.data_ptr(), work.data_ptr(), need, None)
    assert rc == 0
    torch.cuda.synchronize()
    raw = dst.cpu().numpy()
    assert np.array_equal(raw, expected(name)), differs(raw, expected(name), "rir_polygon_map_device")


@pytest.mark.parametrize("per_map", [True, False])
def test_host_entry_in_slabs(per_map):
    """five maps of 2048x2048 are 80 MiB: the host entry makes them in slabs of four and one, and the second slab starts at its own polygon
    set and its own shift.  Against device.polygon_map, which the cases above pin to the oracle."""
    from librir_amd import device as D
    from librir_amd import signal_processing as S

    shape, n = (2048, 2048), 5
    shifts = np.array([(0.5, 0.5), (-20.5, 3.25), (64, -8), (300.25, 900), (1500, 1200.5)])
    if per_map:
        polygons = [PC._kinds(310 + m, (17, 130), 1) for m in range(n)]
    else:
        polygons = PC._kinds(301, (33, 70), 1) + [[(3, 3), (30, 20)], [(40, 9)]]
    want = D.polygon_map(polygons, shape, shifts=shifts).cpu().numpy()
    assert want.shape == (n,) + shape and all((want[m] >= 0).any() for m in range(n))
    assert all(not np.array_equal(want[a], want[b]) for a in range(n) for b in range(a))  # a slab at another map's offset shows
    host = S.polygon_map(polygons, shape, shifts=shifts)
    assert host.dtype == np.int32 and np.array_equal(host, want), differs(host, want, "signal_processing.polygon_map in slabs")


def test_no_polygon_and_no_map(lib):
    from librir_amd import device as D
    from librir_amd import signal_processing as S

    assert (D.polygon_map([], (7, 9), background=5).cpu().numpy() == 5).all()
    assert (S.polygon_map([], (7, 9), shifts=np.zeros((3, 2))) == -1).all()
    assert tuple(D.polygon_map([[(1, 1)]], (7, 9), shifts=np.zeros((0, 2))).shape) == (0, 7, 9)
    assert S.polygon_map([[(1, 1)]], (7, 9), shifts=np.zeros((0, 2))).shape == (0, 7, 9)
    empty = D.polygon_map([[], np.zeros((0, 2))], (7, 9), values=[1, 2])
    assert (empty.cpu().numpy() == -1).all()


@pytest.mark.parametrize("name", ["kinds_33x70", "shared_3_maps", "per_map_3_shifted", "lines_wide", "wide_rows"])
def test_out_at_every_alignment_and_packed_tensors(name):
    """rows that start at any word of a 16-byte chunk; the polygons as packed CUDA tensors, the shifts as a CUDA tensor"""
    from librir_amd import device as D

    case = CASES[name]
    polygons, shape, kw, out_shape = PC.api_args(case)
    a = D._polygon_map_args(polygons, shape, **kw)
    xy, npts, _, shifts = D._polygon_inputs(a, torch.device("cuda"))
    kw = dict(kw, shifts=shifts)
    exp = expected(name).reshape(out_shape)
    count = int(np.prod(out_shape))
    room = torch.full((count + 8,), GARBAGE, dtype=torch.int32, device="cuda")
    for off in range(4):
        room.fill_(GARBAGE)
        out = room[off:off + count].view(out_shape)
        D.polygon_map((xy, npts), shape, out=out, **kw)
        got = room.cpu().numpy()
        assert np.array_equal(got[off:off + count].reshape(out_shape), exp), differs(got[off:off + count].reshape(out_shape), exp, (name, off))
        assert (got[:off] == GARBAGE).all() and (got[off + count:] == GARBAGE).all(), (name, off)


def test_queued_on_a_side_stream_behind_the_upload():
    from librir_amd import device as D

    case = CASES["octagons_big"]
    polygons, shape, kw, out_shape = PC.api_args(case)
    a = D._polygon_map_args(polygons, shape, **kw)
    shifts = np.random.default_rng(5).uniform(-30, 30, (40, 2))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        xy = torch.from_numpy(a.xy).pin_memory().to("cuda", non_blocking=True)
        npts = torch.from_numpy(a.npts).pin_memory().to("cuda", non_blocking=True)
        moves = torch.from_numpy(shifts).pin_memory().to("cuda", non_blocking=True)
        maps = D.polygon_map((xy, npts), shape, shifts=moves)
        area = (maps >= 0).sum(dim=(1, 2))
    side.synchronize()
    exp = PC.oracle(dict(case, shifts=shifts[[0, 17, 39]]))
    got = maps.cpu().numpy()
    assert np.array_equal(got[[0, 17, 39]], exp), differs(got[[0, 17, 39]], exp, "side stream")
    assert np.array_equal(area.cpu().numpy(), (got >= 0).sum(axis=(1, 2)))


def test_refused_arguments(lib):
    from librir_amd.low_level.misc import last_error

    fn = raw_entry(lib)
    xy = torch.tensor([[[1, 1], [6, 1], [3, 5.0]]], dtype=torch.float64, device="cuda")
    npts = torch.tensor([3], dtype=torch.int32, device="cuda")
    buf = torch.zeros(4096, dtype=torch.int64, device="cuda")
    dst, work = buf.data_ptr(), buf.data_ptr() + 8192
    need = lib.rir_polygon_map_workspace_bytes(8, 7, 2, 1, 3)
    args = lambda **k: [k.get("xy", xy.data_ptr()), k.get("npts", npts.data_ptr()), None, k.get("npoly", 1), k.get("max_pts", 3), k.get("nmaps", 2),  # noqa: E731
                        k.get("sets", 0), None, k.get("w", 8), 7, -1, k.get("dst", dst), k.get("work", work), k.get("wb", need), None]
    assert fn(*args()) == 0
    torch.cuda.synchronize()
    assert fn(*args(wb=need - 1)) == -1 and "workspace" in last_error()
    assert fn(*args(work=work + 4)) == -1 and "workspace" in last_error()
    assert fn(*args(work=dst + 16)) == -1 and "overlap" in last_error()
    assert fn(*args(dst=xy.data_ptr())) == -1 and "overlap" in last_error()
    assert fn(*args(dst=None)) == -1 and fn(*args(work=None)) == -1 and fn(*args(xy=None)) == -1 and fn(*args(npts=None)) == -1
    assert fn(*args(w=0)) == -1 and fn(*args(sets=2)) == -1 and fn(*args(max_pts=0)) == -1 and fn(*args(max_pts=1025)) == -1
    assert fn(*args(npoly=-1)) == -1 and fn(*args(nmaps=-1)) == -1
    assert fn(*args(nmaps=0, dst=None, work=None)) == 0  # no map: nothing to do
    assert fn(*args(npoly=0, xy=None, npts=None)) == 0  # no polygon: background maps
    torch.cuda.synchronize()
    assert (buf[:2 * 7 * 8 // 2].view(torch.int32) == -1).all()


def test_movie_polygon_stats(tmp_path):
    """shared regions, regions that follow a shift table and one set of regions per image, against region_stats over oracle maps"""
    from librir_amd.synthetic import s1_noisy_background
    from librir_amd.video_io import IRMovie

    n, h, w = 20, 33, 70
    arr = s1_noisy_background(n, h, w, seed=21)
    polygons = [PC.ring(8, 20, 12, 9, 8), PC.ring(5, 50, 20, 14.5, 9), [(3, 3), (66, 30)], [(35, 16)], PC.ring(6, 34, 15, 6, 6)]
    values = [2, 0, 3, 3, 1]
    rng = np.random.default_rng(3)
    shifts = np.concatenate([[(0, 0), (0.5, -0.5), (-40, 3)], rng.uniform(-12, 12, (n - 3, 2))])
    with IRMovie.from_filename(record(tmp_path / "roi.h264", arr)) as mov:
        mov._STATS_PIECE_BYTES = 7 * h * w * 6  # pieces of 7, 7 and 6 images
        for sel in (slice(None), slice(1, 19, 2)):
            frames = np.asarray(mov[sel])
            k = len(frames)
            shared = PC.oracle(PC.case((h, w), polygons, values=values))[0]
            check(mov.polygon_stats(polygons, sel, values=values), region_stats_oracle(frames, shared, 4), ("shared", sel))
            moved = PC.oracle(PC.case((h, w), polygons, shifts=shifts[:k]))
            check(mov.polygon_stats(polygons, sel, shifts=shifts[:k]), region_stats_oracle(frames, moved, 5), ("shifted", sel))
            check(mov.polygon_stats(polygons, sel, shifts=torch.from_numpy(shifts[:k]).cuda(), values=values),
                  region_stats_oracle(frames, PC.oracle(PC.case((h, w), polygons, values=values, shifts=shifts[:k])), 4), ("shifted, values", sel))
            sets = [[np.asarray(p) + (t, -t / 2) for p in polygons[:2 + t % 3]] for t in range(k)]
            per_image = PC.oracle(PC.case((h, w), sets, per_map=True))
            check(mov.polygon_stats(sets, sel), region_stats_oracle(frames, per_image, 4), ("per image", sel))
        with pytest.raises(ValueError, match="polygon_stats"):
            mov.polygon_stats(polygons, slice(None), shifts=shifts[:5])
