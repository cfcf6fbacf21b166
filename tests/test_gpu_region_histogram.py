"""GPU: per-region histograms, bit for bit against the oracle of test_region_histogram_cpu.py - shapes, stack lengths, shared, per-frame and
no maps, every binning case over full-range and static scenes, rows, region counts on both sides of the LDS and copy thresholds, wide
counters, the pixel-by-pixel loads, reproducibility, stream order, what region_stats and region_quantiles give for the same pixels, the
reference's background level, the host entry and recordings read through IRMovie."""
import re

import numpy as np
import pytest

from test_region_histogram_cpu import DEVICE_ARGS, HEADER, region_histogram_oracle as oracle
from test_region_quantiles_cpu import full_range_case, quantile_rank

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LDS_MAX, COPY_MAX, MAX_COPIES = (int(re.search(r"constexpr int %s = (\d+);" % name, HEADER).group(1))
                                 for name in ("HISTOGRAM_LDS_MAX", "HISTOGRAM_COPY_MAX", "HISTOGRAM_MAX_COPIES"))
BINNINGS = [(0, 1, 65536), (0, 4, 16384), (0, 256, 256), (0, 65536, 1), (7960, 1, 81), (8000, 3, 10), (1, 7, 255), (65535, 1, 1), (100, 1000, 70)]


def dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda().view(torch.uint16)


def dev32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()


def check(got, exp, what=""):
    for name, t, e in zip(("count", "hist", "outside"), got, exp):
        g = t.cpu().numpy() if hasattr(t, "cpu") else t
        assert g.dtype == np.int32 and g.shape == e.shape, (what, name, g.dtype, g.shape, e.shape)
        if not np.array_equal(g, e):
            bad = np.argwhere(g != e)[:5]
            raise AssertionError("%s %s differs at %s: got %s, expected %s" % (what, name, bad.tolist(), g[tuple(bad.T)], e[tuple(bad.T)]))


def run(frames, labels, k, lo, width, nbins, rows=None):
    from librir_amd import device as D

    if labels is None:
        return D.histogram(dev16(frames), nbins, lo, width, rows)
    return D.region_histogram(dev16(frames), dev32(labels), nbins, lo, width, k, rows)


def both(frames, labels, k, lo, width, nbins, rows=None, what=""):
    exp = oracle(frames, labels, k, lo, width, nbins, rows)
    assert np.array_equal(exp[0], exp[2][..., 0] + exp[1].sum(-1) + exp[2][..., 1])
    check(run(frames, labels, k, lo, width, nbins, rows), exp, (what, lo, width, nbins, rows))


def static_scene(n, h, w, seed):
    """a 14-bit scene of a few hundred levels: 8 000 +- 40"""
    return np.random.default_rng(seed).integers(7960, 8041, (n, h, w)).astype(np.uint16)


def rect_map(h, w, ny, nx):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((yy * ny // h) * nx + xx * nx // w).astype(np.int32)


@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (17, 33), (64, 80)])
@pytest.mark.parametrize("n", [1, 2, 7])
def test_shapes_shared_per_frame_and_no_maps(h, w, n):
    for k, (lo, width, nbins) in ((1, (0, 256, 256)), (16, (0, 4, 16384)), (5, (1, 7, 255)), (300, (100, 1000, 70))):
        f, shared = full_range_case(h * 3 + n + k, n, h, w, k)  # labels from -1 to k: both ends are ignored
        both(f, shared, k, lo, width, nbins, what=("shared", h, w, n, k))
        _, per = full_range_case(n + w + k, n, h, w, k, per_frame=True)
        both(f, per, k, lo, width, nbins, what=("per-frame", h, w, n, k))
        both(f, None, 1, lo, width, nbins, what=("no map", h, w, n))


@pytest.mark.parametrize("lo,width,nbins", BINNINGS)
def test_binning_cases(lo, width, nbins):
    n, h, w, k = 2, 64, 80, 3
    full, lab = full_range_case(nbins % 1000 + lo, n, h, w, k)
    assert (full == 0).any() and (full == 65535).any()
    scene = static_scene(n, h, w, seed=width)
    for f, name in ((full, "full range"), (scene, "8000 +- 40")):
        both(f, lab, k, lo, width, nbins, what=name)
        both(f, None, 1, lo, width, nbins, what=name + ", no map")
        both(f[:, :17, :33].copy(), lab[:17, :33].copy(), k, lo, width, nbins, what=name + ", 17x33")
    if lo + nbins * width > 65536:  # the bins beyond 65535 stay 0
        got = run(full, None, 1, lo, width, nbins)
        assert int(got.hist[..., (65536 - lo + width - 1) // width:].sum()) == 0 and int(got.outside[..., 1].sum()) == 0


@pytest.mark.parametrize("h,w", [(17, 33), (64, 80)])
def test_rows(h, w):
    """the rows beyond `rows` hold valid labels and values inside the bins, and do not count"""
    n, k = 3, 4
    f, lab = full_range_case(h, n, h, w, k)
    _, per = full_range_case(w, n, h, w, k, per_frame=True)
    for rows in (0, 1, h - 3, h):
        for lo, width, nbins in ((0, 256, 256), (1, 7, 255)):
            both(f, lab, k, lo, width, nbins, rows, "shared")
            both(f, per, k, lo, width, nbins, rows, "per-frame")
            both(f, None, 1, lo, width, nbins, rows, "no map")
    got = run(f, lab, k, 0, 256, 256, 0)
    assert not got.count.any() and not got.hist.any() and not got.outside.any()


def sparse_labels(k, n, h, w, seed):
    rng = np.random.default_rng(seed)
    used = np.unique(np.concatenate([[0, k - 1, -1, k], rng.integers(0, k, 30)])).astype(np.int32)
    return used[rng.integers(0, used.size, (h, w))], used[rng.integers(0, used.size, (n, h, w))]


def threshold_cases():
    """(k, nbins) with k * (nbins + 3) counters just below, at and above what LDS holds, and what is kept in 2, 4 and 8 copies"""
    cases = []
    for nbins in (1, 13, 256):
        s = nbins + 3
        for limit in (LDS_MAX,) + tuple(COPY_MAX // c for c in (2, 4, 8) if c <= MAX_COPIES):
            cases += [(limit // s + d, nbins) for d in (-1, 0, 1) if limit // s + d >= 1]
    return sorted(set(cases))


@pytest.mark.parametrize("k,nbins", threshold_cases())
def test_region_counts_across_the_forms(k, nbins):
    """64x80, three frames, most regions empty: a few dozen labels out of k, the first and the last among them"""
    n, h, w = 3, 64, 80
    f = static_scene(n, h, w, seed=k % 1000)
    shared, per = sparse_labels(k, n, h, w, seed=k + nbins)
    lo, width = 7990, max(1, 64 // nbins)
    both(f, shared, k, lo, width, nbins, what=("shared", k))
    both(f, per, k, lo, width, nbins, what=("per-frame", k))
    cnt = oracle(f, shared, k, lo, width, nbins)[0]
    assert cnt[:, 0].all() and cnt[:, k - 1].all() and (cnt == 0).sum() >= (k - 34) * n


def test_counters_that_cannot_fit_in_lds():
    """K = 1 with 65 536 bins, and 65 536 regions: the counters beyond the LDS limit are counted in global memory"""
    n, h, w = 2, 64, 80
    f, _ = full_range_case(1, n, h, w, 1)
    assert LDS_MAX < 65536 and (f >= LDS_MAX).any() and (f < LDS_MAX).any()
    both(f, np.zeros((h, w), np.int32), 1, 0, 1, 65536, what="one region, 65 536 bins")
    both(f, None, 1, 0, 1, 65536, what="no map, 65 536 bins")
    shared, per = sparse_labels(65536, n, h, w, seed=2)
    both(f, shared, 65536, 0, 256, 256, what="65 536 regions")
    both(f, per, 65536, 100, 1000, 70, what="65 536 regions, per-frame")


def test_wide_counters():
    h, w = 512, 640
    f = np.full((1, h, w), 12345, np.uint16)
    for labels in (None, np.zeros((h, w), np.int32)):
        for lo, width, nbins in ((0, 256, 256), (0, 1, 65536), (12345, 1, 1)):
            got = run(f, labels, 1, lo, width, nbins)
            check(got, oracle(f, labels, 1, lo, width, nbins), "one value")
            assert int(got.hist.max()) == h * w == 327680 and int(got.count[0, 0]) == h * w
    got = run(f, None, 1, 20000, 1, 16)
    assert got.outside.cpu().numpy().tolist() == [[[h * w, 0]]]


def test_large_frames_with_rectangles():
    n, h, w = 2, 768, 1024
    f, _ = full_range_case(768, n, h, w, 1)
    both(f, rect_map(h, w, 4, 4), 16, 0, 256, 256, what="rectangles")
    both(static_scene(n, h, w, seed=3), rect_map(h, w, 4, 4), 16, 7000, 1, 2048, what="rectangles, static scene, fine bins")


def test_sliced_inputs_at_odd_offsets():
    """frames and labels that start 2 and 4 bytes past a 16-byte boundary (torch slices, used where they are), and frames whose pixel count
    is no multiple of 8: the pixel-by-pixel loads"""
    from librir_amd import device as D

    for (n, h, w), k in [((5, 17, 33), 9), ((3, 64, 80), 16)]:
        f, _ = full_range_case(w + k, n + 1, h, w, k)
        fr = dev16(f.reshape(-1))[1:1 + n * h * w].view(n, h, w)
        assert fr.data_ptr() % 16 == 2 and fr.is_contiguous()
        host = f.reshape(-1)[1:1 + n * h * w].reshape(n, h, w)
        _, lab = full_range_case(h, n, h, w, k, per_frame=True)
        lab_t = dev32(np.concatenate([[7], lab.reshape(-1)]))[1:].view(n, h, w)
        assert lab_t.data_ptr() % 16 == 4
        for lo, width, nbins in ((0, 256, 256), (1, 7, 255)):
            check(D.region_histogram(fr, lab_t, nbins, lo, width, k), oracle(host, lab, k, lo, width, nbins), ("per-frame slice", n, h, w))
            check(D.region_histogram(fr, lab_t[1], nbins, lo, width, k, h - 3), oracle(host, lab[1], k, lo, width, nbins, h - 3), ("shared slice", n, h, w))
            check(D.histogram(fr, nbins, lo, width), oracle(host, None, 1, lo, width, nbins), ("no map, slice", n, h, w))
            check(D.region_histogram(dev16(f)[::2], lab_t[0], nbins, lo, width, k), oracle(f[::2], lab[0], k, lo, width, nbins), ("strided", n, h, w))


def test_single_image_nregions_none_and_no_frames():
    from librir_amd import device as D

    f, lab = full_range_case(1, 2, 17, 33, 6)
    lab[lab == 6] = 5  # the largest label is a region of its own
    one = D.region_histogram(dev16(f[0]), dev32(lab), 70, 100, 1000, 6)
    assert tuple(one.count.shape) == (1, 6) and tuple(one.hist.shape) == (1, 6, 70) and tuple(one.outside.shape) == (1, 6, 2)
    assert (one.lo, one.width) == (100, 1000)
    check(one, oracle(f[:1], lab, 6, 100, 1000, 70))
    check(D.region_histogram(dev16(f), dev32(lab), 70, 100, 1000), oracle(f, lab, 6, 100, 1000, 70), "nregions from the map")
    check(D.region_histogram(dev16(f), None, 70, 100, 1000), oracle(f, None, 1, 100, 1000, 70), "labels None")
    empty = D.region_histogram(dev16(f)[:0], dev32(lab), 70, 100, 1000, 6)
    assert tuple(empty.count.shape) == (0, 6) and tuple(empty.hist.shape) == (0, 6, 70) and tuple(D.histogram(dev16(f)[:0], 4).hist.shape) == (0, 1, 4)
    edges = one.edges()
    assert edges.is_cuda and edges.dtype == torch.int64 and edges[0] == 100 and edges[-1] == 70100


def test_the_same_call_twice_and_on_a_side_stream_gives_the_same_bits():
    from librir_amd import device as D

    n, h, w = 7, 64, 80
    f = dev16(static_scene(n, h, w, seed=5))
    lab = dev32(np.random.default_rng(5).integers(0, 3, (h, w)).astype(np.int32))
    side = torch.cuda.Stream()
    for k, (lo, width, nbins) in ((3, (7960, 1, 81)), (3, (0, 4, 16384)), (LDS_MAX // 84 + 3, (7960, 1, 81))):
        a = D.region_histogram(f, lab, nbins, lo, width, k)
        b = D.region_histogram(f, lab, nbins, lo, width, k)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            c = D.region_histogram(f, lab, nbins, lo, width, k)
        side.synchronize()
        for x in (b, c):
            assert torch.equal(a.count, x.count) and torch.equal(a.hist, x.hist) and torch.equal(a.outside, x.outside), k
    a, b = D.histogram(f, 81, 7960), D.histogram(f, 81, 7960)
    assert torch.equal(a.hist, b.hist) and torch.equal(a.count, b.count)


def test_null_outputs_and_refused_arguments(lib):
    from librir_amd.low_level.misc import last_error

    n, h, w, k = 2, 8, 8, 4
    f, lab = full_range_case(0, n, h, w, k)
    exp = oracle(f, lab, k, 0, 4096, 16)
    fr, lt = dev16(f), dev32(lab)
    fn = lib.rir_region_histogram_device
    fn.argtypes = DEVICE_ARGS
    buf = torch.full((8192,), -1, dtype=torch.int32, device="cuda")
    base = buf.data_ptr()
    good = dict(fr=fr.data_ptr(), lab=lt.data_ptr(), w=w, h=h, rows=h, n=n, per=0, k=k, lo=0, width=4096, nbins=16, count=base, hist=base + 1024,
                outside=base + 4096, work=base + 8192, wb=8)

    def call(**kw):
        a = dict(good, **kw)
        return fn(*(a[x] for x in ("fr", "lab", "w", "h", "rows", "n", "per", "k", "lo", "width", "nbins", "count", "hist", "outside", "work", "wb")), None)

    def outputs():
        torch.cuda.synchronize()
        return (buf[:n * k].view(n, k), buf[256:256 + n * k * 16].view(n, k, 16), buf[1024:1024 + n * k * 2].view(n, k, 2))

    assert call() == 0
    check(outputs(), exp, "all outputs")
    buf.fill_(-1)
    assert call(count=None, outside=None) == 0
    got = outputs()
    check((exp[0], got[1], exp[2]), exp, "hist alone")
    assert (got[0] == -1).all() and (got[2] == -1).all()  # what was not asked for is not written
    assert call(rows=0) == 0 and not any(t.any() for t in outputs())  # zeroed
    for kw in (dict(w=0), dict(rows=h + 1), dict(n=-1), dict(per=2), dict(k=0), dict(k=65537), dict(lo=65536), dict(width=0), dict(nbins=65537),
               dict(k=257, nbins=65536), dict(lab=None), dict(fr=None), dict(hist=None), dict(work=None), dict(wb=7), dict(work=base + 8196)):
        assert call(**kw) == -1, kw
    assert call(outside=base + 1024 + 8) == -1 and "overlap" in last_error()
    assert call(hist=fr.data_ptr()) == -1 and "overlap" in last_error()
    assert call(n=0) == 0
    torch.cuda.synchronize()


def test_consistent_with_region_stats_and_region_quantiles():
    from librir_amd import device as D

    n, h, w, k = 3, 64, 80, 16
    f, lab = full_range_case(21, n, h, w, k)
    f[1] >>= 2  # a frame without 65535
    fr, lt = dev16(f), dev32(lab)
    hg = D.region_histogram(fr, lt, 256, 0, 256, k)
    assert torch.equal(hg.count, D.region_stats(fr, lt, k).count)
    percents = (0.25, 0.5, 0.75, 0.99)
    q = D.region_quantiles(fr, lt, percents, k)
    assert torch.equal(q.count, hg.count)
    cum, cnt, val = hg.cumulative().cpu().numpy(), hg.count.cpu().numpy(), q.values.cpu().numpy()
    checked = 0
    for i in range(n):
        for r in range(k):
            for j, p in enumerate(percents):
                if val[i, r, j] in (-1, 0):
                    continue
                t = quantile_rank(cnt[i, r], p)
                assert val[i, r, j] >> 8 == int(np.argmax(cum[i, r] >= t)), (i, r, p)  # the first bin whose cumulative count reaches the rank
                checked += 1
    assert checked > n * k * 3


def record(path, frames):
    from librir_amd.video_io import IRSaver

    n, h, w = frames.shape
    with IRSaver(str(path), w, h, h) as s:
        for i in range(n):
            s.add_image(frames[i], i * 20000000 + 7)
    return str(path)


def test_background_levels(tmp_path):
    """the reference's get_background per image: of the bins of v >> 2 the first of the largest, (index << 2) + 1"""
    from librir_amd.synthetic import hot_spots
    from librir_amd.video_io import IRMovie

    arr = np.ascontiguousarray(hot_spots(4, 64, 80))
    tie = np.full((1, 64, 80), 1000, np.uint16)
    tie.reshape(-1)[:64 * 40] = 9002  # two equally full bins, 250 and 2250: the lower one wins
    arr = np.concatenate([arr, tie])
    def levels(stack, rows=64):
        return [int(np.bincount(fr[:rows].reshape(-1) >> 2, minlength=16384).argmax()) * 4 + 1 for fr in stack]  # (argmax: the first of the largest)

    from librir_amd import device as D

    assert levels(arr)[-1] == 1001
    assert (D.histogram(dev16(arr), 16384, 0, 4).mode()[:, 0] * 4 + 1).cpu().tolist() == levels(arr)
    with IRMovie.from_filename(record(tmp_path / "b.h264", arr)) as mov:
        back = np.asarray(mov[:]).reshape(arr.shape)
        got = mov.background_levels()
        assert got.is_cuda and got.dtype == torch.int32 and tuple(got.shape) == (5,) and got.cpu().tolist() == levels(back)
        assert levels(back)[-1] == 1001
        assert mov.background_levels(slice(1, None, 2)).cpu().tolist() == levels(back)[1::2]
        assert mov.background_levels(rows=32).cpu().tolist() == levels(back, 32)


def test_host_entry_equals_device_entry():
    from librir_amd import signal_processing as S

    for (n, h, w), k, per_frame, (lo, width, nbins), rows in [((3, 17, 33), 9, False, (0, 256, 256), None), ((2, 17, 33), 9, True, (1, 7, 255), 14),
                                                             ((1, 1, 1), 1, False, (0, 65536, 1), None), ((5, 64, 80), 70, True, (100, 1000, 70), 61)]:
        f, lab = full_range_case(n + k, n, h, w, k, per_frame)
        host = S.region_histogram(f, lab, nbins, lo, width, k, rows)
        assert all(isinstance(a, np.ndarray) for a in host[:3]) and (host.lo, host.width) == (lo, width)
        exp = oracle(f, lab, k, lo, width, nbins, rows)
        check(host, exp, ("host", n, h, w, k))
        check(run(f, lab, k, lo, width, nbins, rows), exp, ("device", n, h, w, k))
        check(S.region_histogram(f, None, nbins, lo, width, rows=rows), oracle(f, None, 1, lo, width, nbins, rows), ("host, no map", n, h, w))
    check(S.region_histogram(f[0], lab[0], 16, 0, 4096), oracle(f[:1], lab[0], int(lab[0].max()) + 1, 0, 4096, 16), "one image, nregions from the map")
    # 65 536 regions of 256 bins: one frame's outputs are a whole slab, so the frames go one by one, each with its own map
    f, _ = full_range_case(9, 2, 17, 33, 1)
    lab = np.random.default_rng(9).integers(65500, 65537, (2, 17, 33)).astype(np.int32)
    assert not np.array_equal(lab[0], lab[1])
    check(S.region_histogram(f, lab, 256, 0, 256, 65536), oracle(f, lab, 65536, 0, 256, 256), "frame by frame")
    check(S.region_histogram(f, lab[1], 256, 0, 256, 65536), oracle(f, lab[1], 65536, 0, 256, 256), "frame by frame, shared map")


def test_host_entry_without_count_and_outside(lib):
    """rir_region_histogram with count, outside or both null: hist as ever, and what was not asked for is not written"""
    from test_region_histogram_cpu import HOST_ARGS

    n, h, w, k = 3, 17, 33, 4
    f, lab = full_range_case(31, n, h, w, k)
    exp = oracle(f, lab, k, 100, 1000, 70)
    fn = lib.rir_region_histogram
    fn.argtypes = HOST_ARGS
    for want_count, want_outside in ((False, False), (True, False), (False, True)):
        count, hist, outside = np.full((n, k), -7, np.int32), np.full((n, k, 70), -7, np.int32), np.full((n, k, 2), -7, np.int32)
        assert fn(f.ctypes.data, lab.ctypes.data, w, h, h, n, 0, k, 100, 1000, 70, count.ctypes.data if want_count else None, hist.ctypes.data,
                  outside.ctypes.data if want_outside else None) == 0
        check((count if want_count else exp[0], hist, outside if want_outside else exp[2]), exp, (want_count, want_outside))
        assert want_count or (count == -7).all()
        assert want_outside or (outside == -7).all()
    hist = np.full((n, 1, 70), -7, np.int32)
    assert fn(f.ctypes.data, None, w, h, h - 3, n, 0, 1, 100, 1000, 70, None, hist.ctypes.data, None) == 0
    assert np.array_equal(hist, oracle(f, None, 1, 100, 1000, 70, h - 3)[1])


@pytest.mark.parametrize("bad_pixels", [False, True])
def test_movie_region_histogram(tmp_path, bad_pixels):
    from librir_amd import device as D
    from librir_amd.synthetic import inject_bad_pixels, s1_noisy_background
    from librir_amd.video_io import IRMovie

    n, h, w = 23, 64, 80
    arr = inject_bad_pixels(s1_noisy_background(n, h, w, seed=12), 7)
    lab = rect_map(h, w, 3, 3)
    lab[::5, ::3] = -1
    lo, width, nbins = int(arr.min()) + 3, 5, 300
    with IRMovie.from_filename(record(tmp_path / "m.h264", arr)) as mov:
        mov.bad_pixels_correction = bad_pixels
        for pieces in (None, 5 * h * w * 2):
            if pieces:
                mov._STATS_PIECE_BYTES = pieces  # the selections below cross pieces of five images
            for sel in (slice(None), slice(2, 21, 3), slice(1, None, 2), 5, -1):
                stack = mov.to_tensor(sel)
                want = D.region_histogram(stack, dev32(lab), nbins, lo, width, 9, h - 3)
                for got in (mov.region_histogram(lab, nbins, lo, width, sel, rows=h - 3), mov.region_histogram(dev32(lab), nbins, lo, width, sel, 9, h - 3)):
                    assert torch.equal(got.count, want.count) and torch.equal(got.hist, want.hist) and torch.equal(got.outside, want.outside), (pieces, sel)
                    assert (got.lo, got.width) == (lo, width)
                check(got, oracle(np.asarray(mov[sel]).reshape(-1, h, w), lab, 9, lo, width, nbins, h - 3), ("oracle", pieces, sel))
                want = D.histogram(stack, nbins, lo, width)
                got = mov.histogram(nbins, lo, width, sel)
                assert torch.equal(got.count, want.count) and torch.equal(got.hist, want.hist) and torch.equal(got.outside, want.outside), (pieces, sel)
        with pytest.raises(RuntimeError):
            mov.region_histogram(lab.astype(np.int64), 16)
        with pytest.raises(ValueError):
            mov.region_histogram(lab, 0)
        with pytest.raises(ValueError):
            mov.histogram(16, rows=h + 1)
