"""GPU: per-region statistics, bit for bit against the oracle of test_region_stats_cpu.py - shapes, stack lengths, shared and per-frame maps,
region counts on both sides of the LDS / global threshold, sliced inputs, stream order, reproducibility, the host entry, hot-spot components
from label_images and recordings read through IRMovie.region_stats."""
import ctypes as ct
import time

import numpy as np
import pytest

from test_region_stats_cpu import FIELDS, region_stats_oracle as oracle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LDS_MAX = 4096  # region_kernels.h REGION_LDS_MAX: the form changes above it


def dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda().view(torch.uint16)


def dev32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()


def check(rs, exp, what=""):
    for k, t in zip(FIELDS, rs):
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


def run(frames, labels, k):
    from librir_amd import device as D

    return D.region_stats(dev16(frames), dev32(labels), k)


SHAPES = [(1, 1), (3, 5), (17, 33), (512, 640), (768, 1024)]


@pytest.mark.parametrize("h,w", SHAPES)
@pytest.mark.parametrize("n", [1, 2, 7])
def test_shapes_shared_and_per_frame_maps(h, w, n):
    f = frames_of(n, h, w, seed=h * 3 + n)
    rng = np.random.default_rng(n + w)
    for k in (1, 16, 1023):
        shared = rng.integers(-1, k + 1, (h, w)).astype(np.int32)
        check(run(f, shared, k), oracle(f, shared, k), ("shared", h, w, n, k))
        per = rng.integers(-1, k + 1, (n, h, w)).astype(np.int32)
        check(run(f, per, k), oracle(f, per, k), ("per-frame", h, w, n, k))


def test_single_image_is_a_stack_of_one():
    from librir_amd import device as D

    f = frames_of(1, 17, 33, seed=1)
    lab = blob_map(17, 33, 5, seed=1)
    rs = D.region_stats(dev16(f[0]), dev32(lab), 5)
    assert all(tuple(t.shape) == (1, 5) for t in rs)
    check(rs, oracle(f, lab, 5))


@pytest.mark.parametrize("k", [1, 16, 1023, 1024, 1025, 2048, LDS_MAX - 1, LDS_MAX, LDS_MAX + 1, 100000])
def test_region_counts_across_the_forms(k):
    n, h, w = 3, 512, 640
    f = frames_of(n, h, w, seed=k % 1000)
    rng = np.random.default_rng(k)
    lab = rng.integers(-3, k + 3, (h, w)).astype(np.int32)
    check(run(f, lab, k), oracle(f, lab, k), ("random shared", k))
    per = rng.integers(0, k, (n, h, w)).astype(np.int32)
    check(run(f, per, k), oracle(f, per, k), ("random per-frame", k))
    if k <= LDS_MAX + 1:
        blobs = blob_map(h, w, min(k, 600), seed=k) if k > 1 else np.zeros((h, w), np.int32)
        check(run(f, blobs, k), oracle(f, blobs, k), ("blobs", k))


@pytest.mark.parametrize("n", [1, 256])
def test_rectangles_and_blobs_long_stacks(n):
    h, w = 512, 640
    f = frames_of(n, h, w, seed=n)
    for lab, k in [(rect_map(h, w, 4, 4), 16), (rect_map(h, w, 2, 3), 6), (blob_map(h, w, 1024, seed=3), 1024), (rect_map(h, w, 64, 40), LDS_MAX + 512)]:
        check(run(f, lab, k), oracle(f, lab, k), (n, k))


def test_full_frame_of_65535_gives_the_largest_sums():
    h, w = 768, 1024
    f = np.full((2, h, w), 65535, np.uint16)
    f[1, 100, 200] = 3
    lab = np.zeros((h, w), np.int32)
    rs = run(f, lab, 1)
    exp = oracle(f, lab, 1)
    check(rs, exp)
    assert int(rs.sumsq[0, 0]) == h * w * 65535 ** 2 and int(rs.argmax[0, 0]) == 0 and int(rs.argmin[1, 0]) == 100 * w + 200
    for k in (1, LDS_MAX + 1):  # one region in both forms
        check(run(f, lab, k), oracle(f, lab, k), k)


def test_sliced_inputs_at_odd_offsets():
    """frames and labels that start 2 and 4 bytes past an allocation (torch slices), odd widths: the pixel-by-pixel path"""
    from librir_amd import device as D

    for (n, h, w), k in [((5, 17, 33), 9), ((3, 512, 640), 16), ((4, 64, 64), LDS_MAX + 7)]:
        f = frames_of(n + 1, h, w, seed=w)
        flat = dev16(f.reshape(-1))
        fr = flat[1:1 + n * h * w].view(n, h, w)
        lab = np.random.default_rng(h).integers(-1, k + 1, (n, h, w)).astype(np.int32)
        lflat = dev32(np.concatenate([[7], lab.reshape(-1)]))
        lab_t = lflat[1:].view(n, h, w)
        exp = oracle(f.reshape(-1)[1:1 + n * h * w].reshape(n, h, w), lab, k)
        check(D.region_stats(fr, lab_t, k), exp, ("per-frame slice", n, h, w))
        check(D.region_stats(fr, lab_t[1], k), oracle(f.reshape(-1)[1:1 + n * h * w].reshape(n, h, w), lab[1], k), ("shared slice", n, h, w))
        # a non-contiguous stack (every other frame) is made contiguous
        every = dev16(f)[::2]
        check(D.region_stats(every, lab_t[0], k), oracle(f[::2], lab[0], k), ("strided", n, h, w))


def test_nregions_none_takes_the_largest_label():
    from librir_amd import device as D

    f = frames_of(2, 17, 33, seed=2)
    lab = blob_map(17, 33, 7, seed=2)
    rs = D.region_stats(dev16(f), dev32(lab))
    assert rs.count.shape == (2, 7)
    check(rs, oracle(f, lab, 7))
    neg = np.full((17, 33), -5, np.int32)
    rs = D.region_stats(dev16(f), dev32(neg))
    assert rs.count.shape == (2, 1) and int(rs.count.sum()) == 0 and int(rs.min[0, 0]) == -1


def test_refused_arguments(lib):
    from librir_amd import device as D
    from librir_amd.low_level.misc import last_error

    f = dev16(frames_of(2, 8, 8, seed=0))
    lab = dev32(np.zeros((8, 8), np.int32))
    with pytest.raises(RuntimeError):
        D.region_stats(f, lab.to(torch.int64), 1)
    with pytest.raises(RuntimeError):
        D.region_stats(f.view(torch.int16), lab, 1)
    with pytest.raises(RuntimeError):
        D.region_stats(f, lab.cpu(), 1)
    fn = lib.rir_region_stats_device
    fn.argtypes = [ct.c_void_p, ct.c_void_p] + [ct.c_int] * 5 + [ct.c_void_p] * 8 + [ct.c_size_t, ct.c_void_p]
    K = 4
    buf = torch.zeros(4096, dtype=torch.int64, device="cuda")
    base = buf.data_ptr()
    outs = [base + 1024 * i for i in range(7)]
    work = base + 1024 * 8
    args = lambda o=outs, wk=work, wb=2 * K * 32: [f.data_ptr(), lab.data_ptr(), 8, 8, 2, 0, K] + o + [wk, wb, None]  # noqa: E731
    assert fn(*args()) == 0
    torch.cuda.synchronize()
    assert fn(*args(wb=2 * K * 32 - 1)) == -1 and "workspace" in last_error()
    assert fn(*args(o=[outs[0], outs[0] + 8] + outs[2:])) == -1 and "overlap" in last_error()
    assert fn(*args(o=[f.data_ptr()] + outs[1:])) == -1 and "overlap" in last_error()
    assert fn(*args(wk=outs[3])) == -1
    assert fn(*args(o=[None] + outs[1:])) == -1
    a = args()
    a[2] = 0
    assert fn(*a) == -1
    a = args()
    a[5] = 2
    assert fn(*a) == -1
    a = args()
    a[6] = 0
    assert fn(*a) == -1
    a = args()
    a[4] = 0
    assert fn(*a) == 0  # nframes 0: nothing to do
    torch.cuda.synchronize()


def test_queued_behind_the_kernel_that_writes_the_frames():
    """the frames are written by kernels on a side stream and reduced on that stream at once"""
    from librir_amd import device as D

    n, h, w = 200, 512, 640
    f = frames_of(n, h, w, seed=9)
    lab = rect_map(h, w, 4, 4)
    host = torch.from_numpy(f.view(np.int16)).pin_memory()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        src = torch.empty((n, h, w), dtype=torch.int16, device="cuda")
        src.copy_(host, non_blocking=True)
        src.add_(0)
        labels = torch.from_numpy(lab).pin_memory().to("cuda", non_blocking=True)
        rs = D.region_stats(src.view(torch.uint16), labels, 16)
    side.synchronize()
    check(rs, oracle(f, lab, 16))


def test_contended_case_is_reproducible():
    """every pixel of 256 frames in 3 regions, in both forms: the same bytes from two runs"""
    from librir_amd import device as D

    n, h, w = 256, 512, 640
    f = dev16(frames_of(n, h, w, seed=5))
    lab = dev32(np.random.default_rng(5).integers(0, 3, (h, w)).astype(np.int32))
    for k in (3, LDS_MAX + 3):
        a = D.region_stats(f, lab, k)
        b = D.region_stats(f, lab, k)
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    check(a, oracle(f.cpu().view(torch.int16).numpy().view(np.uint16), lab.cpu().numpy(), LDS_MAX + 3))


def test_host_entry_equals_device_entry():
    from librir_amd import signal_processing as S

    for (n, h, w), k, per_frame in [((3, 17, 33), 9, False), ((2, 17, 33), 9, True), ((1, 1, 1), 1, False), ((5, 64, 80), LDS_MAX + 1, True)]:
        f = frames_of(n, h, w, seed=n + k)
        rng = np.random.default_rng(k)
        lab = rng.integers(-1, k + 1, (n, h, w) if per_frame else (h, w)).astype(np.int32)
        host = S.region_stats(f, lab, k)
        exp = oracle(f, lab, k)
        check(host, exp, ("host", n, h, w, k))
        check(run(f, lab, k), exp, ("device", n, h, w, k))
    # more than one 64 MiB slab of frames, shared map uploaded once and per-frame maps sent with their slab
    f = frames_of(230, 512, 640, seed=3)
    lab = rect_map(512, 640, 4, 4)
    check(S.region_stats(f, lab, 16), oracle(f, lab, 16), "slabs shared")
    per = np.broadcast_to(lab, f.shape).copy()
    per[::3] = blob_map(512, 640, 16, seed=1)
    check(S.region_stats(f, per, 16), oracle(f, per, 16), "slabs per-frame")


def test_hot_spot_components_from_label_images():
    """labels, areas, xy, counts = label_images(frames > t); region_stats(frames, labels, counts.max()): component c of frame f is region c"""
    from librir_amd import device as D
    from librir_amd.synthetic import s1_noisy_background

    n, h, w = 6, 128, 160
    f = s1_noisy_background(n, h, w, seed=4).copy()
    rng = np.random.default_rng(4)
    for i in range(n):
        for _ in range(12):
            y, x, r = rng.integers(5, h - 5), rng.integers(5, w - 5), rng.integers(1, 4)
            f[i, y - r:y + r + 1, x - r:x + r + 1] = 60000 + rng.integers(0, 5000)
    t = dev16(f)
    threshold = int(np.percentile(f, 99))
    hot = (t.view(torch.int16).to(torch.int32) & 0xFFFF) > threshold  # (frames > t, compared as int32)
    labels, areas, xy, counts = D.label_images(hot)
    kmax = int(counts.max())
    rs = D.region_stats(t, labels, kmax)
    lab = labels.cpu().numpy()
    check(rs, oracle(f, lab, kmax))
    cnt, am = rs.count.cpu().numpy(), rs.argmax.cpu().numpy()
    c = counts.cpu().numpy()
    a = areas.cpu().numpy()
    for i in range(n):
        assert c[i] > 2
        assert np.array_equal(cnt[i, 1:c[i]], a[i, 1:c[i]])
        for comp in range(1, c[i]):
            assert lab[i].reshape(-1)[am[i, comp]] == comp


def record(path, frames):
    from librir_amd.video_io import IRSaver

    n, h, w = frames.shape
    with IRSaver(str(path), w, h, h) as s:
        for i in range(n):
            s.add_image(frames[i], i * 20000000 + 7)
    return str(path)


@pytest.mark.parametrize("bad_pixels", [False, True])
def test_movie_region_stats(tmp_path, bad_pixels):
    from librir_amd.synthetic import inject_bad_pixels, s1_noisy_background
    from librir_amd.video_io import IRMovie

    n, h, w = 43, 67, 83
    arr = inject_bad_pixels(s1_noisy_background(n, h, w, seed=12), 7)
    lab = blob_map(h, w, 9, seed=12)
    with IRMovie.from_filename(record(tmp_path / "m.h264", arr)) as mov:
        mov.bad_pixels_correction = bad_pixels
        for sel in (slice(None), slice(2, 40, 3), 5, -1):
            exp = oracle(np.asarray(mov[sel]).reshape(-1, h, w), lab, 9)
            check(mov.region_stats(lab, sel), exp, ("numpy labels", sel))
            check(mov.region_stats(dev32(lab), sel, 9), exp, ("cuda labels", sel))
        with pytest.raises(RuntimeError):
            mov.region_stats(lab.astype(np.int64))


def test_movie_region_stats_in_uneven_pieces(tmp_path):
    from librir_amd.synthetic import s1_noisy_background
    from librir_amd.video_io import IRMovie

    n, h, w = 50, 40, 48
    arr = s1_noisy_background(n, h, w, seed=2)
    lab = rect_map(h, w, 3, 3)
    with IRMovie.from_filename(record(tmp_path / "p.h264", arr)) as mov:
        mov._STATS_PIECE_BYTES = 11 * h * w * 2
        for sel in (slice(None), slice(1, None, 2), slice(3, 45, 7)):
            check(mov.region_stats(lab, sel, 9), oracle(np.asarray(mov[sel]), lab, 9), sel)


# Rate floors over 1 000 frames of 640x512 (uint16), shared map: about 0.7 of what tests/perf/region_stats_time.py measured when the feature
# was added, on one MI355X.
FLOOR_RECT16 = 1.35e6  # measured 1.93-1.94 M frames/s
FLOOR_BLOB1024 = 0.95e6  # measured 1.37-1.39 M


@pytest.mark.perf
@pytest.mark.parametrize("kind,floor", [("rect16", FLOOR_RECT16), ("blob1024", FLOOR_BLOB1024)])
def test_rate_floor(kind, floor):
    from librir_amd import device as D

    n, h, w = 1000, 512, 640
    src = torch.randint(0, 65536, (n, h, w), dtype=torch.int32, device="cuda").to(torch.int16).view(torch.uint16)
    lab, k = (rect_map(h, w, 4, 4), 16) if kind == "rect16" else (blob_map(h, w, 1024, seed=7), 1024)
    labels = dev32(lab)
    for _ in range(3):
        D.region_stats(src, labels, k)
    torch.cuda.synchronize()
    reps = 20
    t0 = time.perf_counter()
    for _ in range(reps):
        D.region_stats(src, labels, k)
    torch.cuda.synchronize()
    rate = reps * n / (time.perf_counter() - t0)
    assert rate >= floor, "%s: %.3g frames/s, floor %.3g" % (kind, rate, floor)
