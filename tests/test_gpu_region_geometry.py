"""GPU: per-region geometry, bit for bit against the oracle of test_region_geometry_cpu.py - shapes, stack lengths, shared and per-frame maps,
with and without weights, region counts on both sides of the LDS / global threshold, widths whose 8-pixel steps cross row ends, sliced
inputs, the widest and tallest frames, reproducibility, the host entry, recordings read through IRMovie.region_geometry and the hot-spot
tracks of IRMovie.track_hot_spots_geometry."""
import ctypes as ct

import numpy as np
import pytest

from test_region_geometry_cpu import FIELDS, region_geometry_oracle as oracle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LDS_MAX = 1024  # geometry_kernels.h GEOMETRY_LDS_MAX: the form changes above it


def dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda().view(torch.uint16)


def dev32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()


def check(g, exp, what=""):
    for k, t in zip(FIELDS, g):
        if exp[k] is None:
            assert t is None, (what, k)
            continue
        got = t.cpu().numpy() if hasattr(t, "cpu") else t
        assert got.dtype == exp[k].dtype and got.shape == exp[k].shape, (what, k, got.dtype, got.shape)
        if not np.array_equal(got, exp[k]):
            bad = np.argwhere(got != exp[k])[:5]
            raise AssertionError("%s %s differs at %s: got %s, expected %s" % (what, k, bad.tolist(), got[tuple(bad.T)], exp[k][tuple(bad.T)]))


def frames_of(n, h, w, seed):
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 65536, (n, h, w), dtype=np.uint16)
    f.reshape(n, -1)[:, ::7] = 0
    f.reshape(n, -1)[:, 3::11] = 65535
    return f


def rect_map(h, w, ny, nx):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((yy * ny // h) * nx + xx * nx // w).astype(np.int32)


def blob_map(h, w, k, seed):
    """k random blobs: every pixel takes the nearest of k random centres (a Voronoi map), a few pixels masked out with -1"""
    rng = np.random.default_rng(seed)
    cy, cx = rng.integers(0, h, k), rng.integers(0, w, k)
    lab = np.zeros((h, w), np.int32)
    best = np.full((h, w), np.iinfo(np.int64).max)
    yy, xx = np.mgrid[0:h, 0:w]
    for i in range(k):
        d = (yy - cy[i]).astype(np.int64) ** 2 + (xx - cx[i]).astype(np.int64) ** 2
        closer = d < best
        lab[closer], best[closer] = i, d[closer]
    lab.reshape(-1)[::97] = -1
    return lab


def run(labels, k, frames=None):
    from librir_amd import device as D

    return D.region_geometry(dev32(labels), k, None if frames is None else dev16(frames))


def check_both(labels, k, frames, what):
    """with the frames as weights, and the labels alone: the same count, bbox and moments"""
    exp = oracle(labels, k, frames)
    g = run(labels, k, frames)
    check(g, exp, (what, "weighted"))
    plain = run(labels, k)
    check(plain, oracle(labels, k), (what, "labels only"))
    m = plain.count.shape[0]
    for a, b in zip(plain[:3], g[:3]):
        assert torch.equal(a, b[:m]), (what, "frames=None differs from the weighted call")


@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (17, 33), (40, 97)])
@pytest.mark.parametrize("n", [1, 2, 7])
def test_shapes_shared_and_per_frame_maps(h, w, n):
    """17 x 33 takes the pixel-by-pixel loads (561 pixels); 40 x 97 the vector loads with a row end inside most 8-pixel steps"""
    f = frames_of(n, h, w, seed=h * 3 + n)
    rng = np.random.default_rng(n + w)
    for k in (1, 16, 1023):
        shared = rng.integers(-1, k + 1, (h, w)).astype(np.int32)
        check_both(shared, k, f, ("shared", h, w, n, k))
        per = rng.integers(-1, k + 1, (n, h, w)).astype(np.int32)
        check_both(per, k, f, ("per-frame", h, w, n, k))


def test_one_full_size_stack():
    n, h, w = 3, 512, 640
    f = frames_of(n, h, w, seed=1)
    for lab, k in [(rect_map(h, w, 4, 4), 16), (blob_map(h, w, 300, seed=2), 300), (np.zeros((h, w), np.int32), 1)]:
        check_both(lab, k, f, ("512x640", k))
    per = np.stack([blob_map(h, w, 40, seed=s) for s in range(n)])
    check_both(per, 40, f, "512x640 per-frame blobs")


def test_single_image_is_a_stack_of_one():
    from librir_amd import device as D

    f = frames_of(1, 17, 33, seed=1)
    lab = blob_map(17, 33, 5, seed=1)
    g = D.region_geometry(dev32(lab), 5, dev16(f[0]))
    assert tuple(g.count.shape) == (1, 5) and tuple(g.bbox.shape) == (1, 5, 4) and tuple(g.moments.shape) == (1, 5, 5) and tuple(g.weighted.shape) == (1, 5, 3)
    check(g, oracle(lab, 5, f))
    g = D.region_geometry(dev32(lab))  # nregions from the largest label, no weights
    assert g.weighted is None
    check(g, oracle(lab, 5))


@pytest.mark.parametrize("k", [LDS_MAX - 1, LDS_MAX, LDS_MAX + 1, 100000])
def test_region_counts_across_the_forms(k):
    n, h, w = 2, 160, 256  # three work items a frame
    f = frames_of(n, h, w, seed=k % 1000)
    rng = np.random.default_rng(k)
    lab = rng.integers(-3, k + 3, (h, w)).astype(np.int32)
    check_both(lab, k, f, ("random shared", k))
    per = rng.integers(0, k, (n, h, w)).astype(np.int32)
    check_both(per, k, f, ("random per-frame", k))
    blobs = blob_map(h, w, 200, seed=k)
    check_both(blobs, k, f, ("blobs", k))


@pytest.mark.parametrize("h,w", [(40, 33), (40, 97), (24, 1000), (3, 2056), (5, 4099)])
def test_rows_that_end_inside_a_step(h, w):
    """large regions (long runs) over widths that are no multiple of 8, narrower and wider than the 2048 pixels of a workgroup's step"""
    n = 2
    f = frames_of(n, h, w, seed=w)
    for lab, k in [(np.zeros((h, w), np.int32), 1), (rect_map(h, w, 2, 3), 6), (blob_map(h, w, 12, seed=h), LDS_MAX + 5)]:
        check_both(lab, k, f, (h, w, k))


def test_sliced_inputs_at_odd_offsets():
    """frames and labels that start 2 and 4 bytes past an allocation (torch slices): the pixel-by-pixel path"""
    from librir_amd import device as D

    for (n, h, w), k in [((5, 17, 33), 9), ((3, 64, 80), 16), ((4, 64, 64), LDS_MAX + 7)]:
        f = frames_of(n + 1, h, w, seed=w)
        flat = dev16(f.reshape(-1))
        fr = flat[1:1 + n * h * w].view(n, h, w)
        fh = f.reshape(-1)[1:1 + n * h * w].reshape(n, h, w)
        lab = np.random.default_rng(h).integers(-1, k + 1, (n, h, w)).astype(np.int32)
        lab_t = dev32(np.concatenate([[7], lab.reshape(-1)]))[1:].view(n, h, w)
        check(D.region_geometry(lab_t, k, fr), oracle(lab, k, fh), ("per-frame slice", n, h, w))
        check(D.region_geometry(lab_t[1], k, fr), oracle(lab[1], k, fh), ("shared slice", n, h, w))
        check(D.region_geometry(lab_t, k), oracle(lab, k), ("labels only slice", n, h, w))
        check(D.region_geometry(lab_t, k, dev16(f)[:n]), oracle(lab, k, f[:n]), ("aligned frames, sliced labels", n, h, w))
        every = dev16(f)[::2]  # a non-contiguous stack is made contiguous
        check(D.region_geometry(lab_t[0], k, every), oracle(lab[0], k, f[::2]), ("strided", n, h, w))


@pytest.mark.parametrize("h,w", [(2, 32768), (32768, 3)])
def test_widest_and_tallest_frames_one_region_of_65535(h, w):
    """the partial sums at their widest: one row of 32768 pixels has a sum of x^2 of 1.17e13, 32768 rows a sum of y^2 of 3.5e13"""
    f = np.full((1, h, w), 65535, np.uint16)
    lab = np.zeros((h, w), np.int32)
    g = run(lab, 1, f)
    check(g, oracle(lab, 1, f), (h, w))
    sx, sy = h * w * (w - 1) // 2, w * h * (h - 1) // 2
    assert g.moments[0, 0].tolist()[:2] == [sx, sy] and g.weighted[0, 0].tolist() == [65535 * h * w, 65535 * sx, 65535 * sy]
    assert g.bbox[0, 0].tolist() == [0, 0, w - 1, h - 1]
    check(run(lab, LDS_MAX + 1, f), oracle(lab, LDS_MAX + 1, f), (h, w, "global form"))
    check(run(lab, 1), oracle(lab, 1), (h, w, "labels only"))


def test_full_frame_of_65535_one_region():
    h, w = 768, 1024
    f = np.full((2, h, w), 65535, np.uint16)
    f[1, 100, 200] = 3
    lab = np.zeros((h, w), np.int32)
    for k in (1, LDS_MAX + 1):  # one region in both forms
        g = run(lab, k, f)
        check(g, oracle(lab, k, f), k)
    assert int(g.weighted[0, 0, 1]) == 65535 * h * (w * (w - 1) // 2) and int(g.weighted[1, 0, 0]) == 65535 * (h * w - 1) + 3


def test_two_runs_give_identical_bits():
    """every pixel of 64 frames in 3 regions, in both forms: the same bytes from two runs"""
    from librir_amd import device as D

    n, h, w = 64, 256, 320
    fh = frames_of(n, h, w, seed=5)
    f = dev16(fh)
    labh = np.random.default_rng(5).integers(0, 3, (h, w)).astype(np.int32)
    lab = dev32(labh)
    for k in (3, LDS_MAX + 3):
        a = D.region_geometry(lab, k, f)
        b = D.region_geometry(lab, k, f)
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    check(a, oracle(labh, LDS_MAX + 3, fh))


def test_refused_arguments(lib):
    from librir_amd import device as D
    from librir_amd.low_level.misc import last_error

    f = dev16(frames_of(2, 8, 8, seed=0))
    lab = dev32(np.zeros((8, 8), np.int32))
    with pytest.raises(RuntimeError):
        D.region_geometry(lab.to(torch.int64), 1, f)
    with pytest.raises(RuntimeError):
        D.region_geometry(lab, 1, f.view(torch.int16))
    with pytest.raises(RuntimeError):
        D.region_geometry(lab.cpu(), 1, f)
    fn = lib.rir_region_geometry_device
    fn.argtypes = [ct.c_void_p, ct.c_void_p] + [ct.c_int] * 5 + [ct.c_void_p] * 5 + [ct.c_size_t, ct.c_void_p]
    K = 4
    buf = torch.zeros(4096, dtype=torch.int64, device="cuda")
    base = buf.data_ptr()
    outs = [base + 1024 * i for i in range(4)]
    work = base + 1024 * 8
    args = lambda o=outs, wk=work, wb=64, fr=f.data_ptr(): [lab.data_ptr(), fr, 8, 8, 2, 0, K] + o + [wk, wb, None]  # noqa: E731
    assert fn(*args()) == 0
    torch.cuda.synchronize()
    assert fn(*args(wb=0)) == -1 and "workspace" in last_error()
    assert fn(*args(wk=work + 4)) == -1 and "workspace" in last_error()
    assert fn(*args(o=[outs[0], outs[0] + 8] + outs[2:])) == -1 and "overlap" in last_error()
    assert fn(*args(o=[f.data_ptr()] + outs[1:])) == -1 and "overlap" in last_error()
    assert fn(*args(wk=outs[2])) == -1
    assert fn(*args(o=[None] + outs[1:])) == -1
    assert fn(*args(o=outs[:3] + [None])) == -1  # frames without d_weighted
    assert fn(*args(fr=None)) == -1  # d_weighted without frames
    assert fn(*args(fr=None, o=outs[:3] + [None])) == -1  # two frames over a shared map without weights
    for at, value in ((2, 0), (2, 32769), (5, 2), (6, 0)):
        a = args()
        a[at] = value
        assert fn(*a) == -1, (at, value)
    a = args()
    a[4] = 0
    assert fn(*a) == 0  # nframes 0: nothing to do
    a = args(fr=None, o=outs[:3] + [None])
    a[4] = 1
    assert fn(*a) == 0  # one shared map, labels only
    torch.cuda.synchronize()


def test_host_entry_equals_device_entry():
    from librir_amd import signal_processing as S

    for (n, h, w), k, per_frame in [((3, 17, 33), 9, False), ((2, 17, 33), 9, True), ((1, 1, 1), 1, False), ((5, 64, 80), LDS_MAX + 1, True)]:
        f = frames_of(n, h, w, seed=n + k)
        lab = np.random.default_rng(k).integers(-1, k + 1, (n, h, w) if per_frame else (h, w)).astype(np.int32)
        host = S.region_geometry(lab, k, f)
        check(host, oracle(lab, k, f), ("host", n, h, w, k))
        assert isinstance(host.count, np.ndarray)
        check(S.region_geometry(lab, k), oracle(lab, k), ("host, labels only", n, h, w, k))
    g = S.region_geometry(lab)
    assert g.weighted is None and g.count.shape == (5, int(lab.max()) + 1)
    # more than one 64 MiB slab: 110 frames of 512 x 640 are 1.1 slabs of frames alone, 2.2 of maps alone and 3.3 of both.  The stack
    # repeats 8 frames and 8 maps, so the oracle runs over 8 and its rows repeat
    n, h, w = 110, 512, 640
    rep = np.arange(n) % 8
    f8 = frames_of(8, h, w, seed=3)
    per8 = np.broadcast_to(rect_map(h, w, 4, 4), f8.shape).copy()
    per8[::3] = blob_map(h, w, 16, seed=1)
    f, per = f8[rep], per8[rep]
    tiled = lambda o: {k: None if a is None else a[rep] for k, a in o.items()}  # noqa: E731
    check(S.region_geometry(per, 16, f), tiled(oracle(per8, 16, f8)), "slabs per-frame")
    check(S.region_geometry(per, 16), tiled(oracle(per8, 16)), "slabs labels only")
    check(S.region_geometry(per8[1], 16, f), tiled(oracle(per8[1], 16, f8)), "slabs shared")


def record(path, frames):
    from librir_amd.video_io import IRSaver

    n, h, w = frames.shape
    with IRSaver(str(path), w, h, h) as s:
        for i in range(n):
            s.add_image(frames[i], i * 20000000 + 7)
    return str(path)


def test_movie_region_geometry(tmp_path):
    from librir_amd.synthetic import s1_noisy_background
    from librir_amd.video_io import IRMovie

    n, h, w = 43, 67, 83
    arr = s1_noisy_background(n, h, w, seed=12)
    lab = blob_map(h, w, 9, seed=12)
    with IRMovie.from_filename(record(tmp_path / "m.h264", arr)) as mov:
        mov._STATS_PIECE_BYTES = 11 * h * w * 2  # uneven pieces
        for sel in (slice(None), slice(2, 40, 3), 5, -1):
            exp = oracle(lab, 9, np.asarray(mov[sel]).reshape(-1, h, w))
            check(mov.region_geometry(lab, sel), exp, ("numpy labels", sel))
            check(mov.region_geometry(dev32(lab), sel, 9), exp, ("cuda labels", sel))
        with pytest.raises(RuntimeError):
            mov.region_geometry(lab.astype(np.int64))
        with pytest.raises(ValueError):
            mov.region_geometry(np.zeros((2, h, w), np.int32))


def test_track_hot_spots_with_geometry(tmp_path):
    """two blobs that move across a flat background: the geometry of every image over its track map"""
    from librir_amd.video_io import IRMovie

    n, h, w = 12, 48, 64
    rng = np.random.default_rng(4)
    arr = rng.integers(1000, 1100, (n, h, w)).astype(np.uint16)
    for i in range(n):
        arr[i, 5 + i:10 + i, 8 + 2 * i:15 + 2 * i] = 30000 + rng.integers(0, 2000, (5, 7))
        arr[i, 30:36, 50 - 3 * i:55 - 3 * i] = 40000 + rng.integers(0, 2000, (6, 5))
    with IRMovie.from_filename(record(tmp_path / "t.h264", arr)) as mov:
        got = mov.track_hot_spots_geometry(20000)
        assert len(got) == 3
        tracks, stats, geo = got
        k = int(tracks.ntracks)
        images = np.asarray(mov[:]).reshape(-1, h, w)
        tmap = tracks.tracks.cpu().numpy()
        check(geo, oracle(tmap, k, images), "tracks")
        assert torch.equal(geo.count, stats.count) and tuple(geo.count.shape) == (n, k)
        assert torch.equal(geo.weighted[..., 0], stats.sum)
        hot = [r for r in range(k) if int(geo.count[:, r].min()) in (30, 35)]  # the two blobs are present in every image
        assert len(hot) == 2
        cen = geo.centroid().cpu().numpy()
        blob = [r for r in hot if int(geo.count[0, r]) == 35][0]
        assert np.allclose(cen[:, blob, 0], 11 + 2 * np.arange(n)) and np.allclose(cen[:, blob, 1], 7 + np.arange(n))
        assert geo.bbox[3, blob].tolist() == [14, 8, 20, 12]
        alone = mov.track_hot_spots_geometry(20000, stats=False)
        assert len(alone) == 3 and alone[1] is None
        check(alone[2], oracle(tmap, k, images), "geometry alone")
        default = mov.track_hot_spots(20000)
        assert len(default) == 2 and torch.equal(default[1].count, stats.count)
        assert len(mov.track_hot_spots(20000, stats=False)) == 2
