"""GPU: per-region quantiles, bit for bit against the oracle of test_region_quantiles_cpu.py - shapes, stack lengths, shared and per-frame
maps, region counts on both sides of the LDS / global threshold of either counting pass, value ranges that stress the two-level select, the
ties of the rank, pixel tails, frame groups of every size, stream order, reproducibility, what region_stats and find_median_pixel give for
the same pixels, maps from label_images and polygon_map, the host entry and recordings read through IRMovie.region_quantiles."""
import ctypes as ct
import os
import re

import numpy as np
import pytest

from test_region_quantiles_cpu import PERCENTS, frame_bytes, quantile_rank, region_quantiles_oracle as oracle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "librir_amd", "csrc", "quantile_kernels.h")) as _f:
    LDS_MAX = int(re.search(r"constexpr int QUANTILE_LDS_MAX = (\d+);", _f.read()).group(1))  # histograms per frame a pass keeps in LDS
FOUR = (0.25, 0.5, 0.75, 0.99)


def dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda().view(torch.uint16)


def dev32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()


def check(got, exp, what=""):
    for name, t, e in zip(("count", "values"), got, exp):
        g = t.cpu().numpy() if hasattr(t, "cpu") else t
        assert g.dtype == np.int32 and g.shape == e.shape, (what, name, g.dtype, g.shape, e.shape)
        if not np.array_equal(g, e):
            bad = np.argwhere(g != e)[:5]
            raise AssertionError("%s %s differs at %s: got %s, expected %s" % (what, name, bad.tolist(), g[tuple(bad.T)], e[tuple(bad.T)]))


def run(frames, labels, k, percents):
    from librir_amd import device as D

    return D.region_quantiles(dev16(frames), dev32(labels), percents, k)


def both(frames, labels, k, percents, what=""):
    check(run(frames, labels, k, percents), oracle(frames, labels, k, percents), what)


def frames_of(n, h, w, seed):
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 65536, (n, h, w), dtype=np.uint16)
    f.reshape(n, -1)[:, ::7] = 0
    f.reshape(n, -1)[:, 3::11] = 65535
    return f


def static_scene(n, h, w, seed):
    """a 14-bit scene of a few hundred levels: 8 000 +- 40"""
    return np.random.default_rng(seed).integers(7960, 8041, (n, h, w)).astype(np.uint16)


def rect_map(h, w, ny, nx):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((yy * ny // h) * nx + xx * nx // w).astype(np.int32)


@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (17, 33), (64, 80)])
@pytest.mark.parametrize("n", [1, 2, 7])
def test_shapes_shared_and_per_frame_maps(h, w, n):
    f = frames_of(n, h, w, seed=h * 3 + n)
    rng = np.random.default_rng(n + w)
    for k, pc in ((1, PERCENTS), (16, (0.5,)), (1023, PERCENTS)):
        shared = rng.integers(-1, k + 1, (h, w)).astype(np.int32)  # -1 and k: ignored
        both(f, shared, k, pc, ("shared", h, w, n, k))
        per = rng.integers(-1, k + 1, (n, h, w)).astype(np.int32)
        both(f, per, k, pc, ("per-frame", h, w, n, k))


@pytest.mark.parametrize("h,w", [(512, 640), (768, 1024)])
def test_large_frames(h, w):
    n = 2
    f = frames_of(n, h, w, seed=h)
    both(f, rect_map(h, w, 4, 4), 16, PERCENTS, "rectangles")
    per = np.random.default_rng(w).integers(-1, 1024, (n, h, w)).astype(np.int32)
    both(f, per, 1023, FOUR, "per-frame random")
    both(static_scene(n, h, w, seed=w), rect_map(h, w, 2, 3), 6, FOUR, "static scene")


@pytest.mark.parametrize("k", [LDS_MAX - 1, LDS_MAX, LDS_MAX + 1, 65536])
def test_region_counts_across_the_forms(k):
    """64x80, three frames, most regions empty: a few dozen labels out of k, the first and the last among them"""
    n, h, w = 3, 64, 80
    f = frames_of(n, h, w, seed=k % 1000)
    rng = np.random.default_rng(k)
    used = np.unique(np.concatenate([[0, k - 1, -1, k], rng.integers(0, k, 30)])).astype(np.int32)
    shared = used[rng.integers(0, used.size, (h, w))]
    per = used[rng.integers(0, used.size, (n, h, w))]
    for pc in ((0.5,), FOUR):
        both(f, shared, k, pc, ("shared", k, pc))
        both(f, per, k, pc, ("per-frame", k, pc))
    cnt, _ = oracle(f, shared, k, (0.5,))
    assert (cnt == 0).sum() >= (k - used.size) * n


@pytest.mark.parametrize("k,q", [(LDS_MAX // 8, 8), (LDS_MAX // 8 + 1, 8), (LDS_MAX // 2, 2), (LDS_MAX // 2 + 1, 2)])
def test_low_byte_pass_on_both_sides_of_its_threshold(k, q):
    """the low-byte pass has k * q histograms a frame: LDS form up to QUANTILE_LDS_MAX of them while the high-byte pass is still in LDS"""
    n, h, w = 3, 64, 80
    pc = PERCENTS[:q] if q == 8 else (0.5, 0.99)
    for f in (frames_of(n, h, w, seed=k), static_scene(n, h, w, seed=k)):
        both(f, np.random.default_rng(q).integers(-1, k + 1, (n, h, w)).astype(np.int32), k, pc, (k, q))
        both(f, rect_map(h, w, 1, k), k, pc, (k, q, "stripes"))


def test_static_scene_and_constant_frames():
    both(static_scene(3, 64, 80, seed=1), rect_map(64, 80, 4, 4), 16, PERCENTS, "8000 +- 40")
    both(static_scene(2, 17, 33, seed=2), np.zeros((17, 33), np.int32), 1, PERCENTS, "8000 +- 40, one region")
    # 327 680 pixels in one counter: more than 16 bits hold
    h, w = 512, 640
    f = np.empty((3, h, w), np.uint16)
    f[0], f[1], f[2] = 12345, 65534, 65535
    got = run(f, np.zeros((h, w), np.int32), 1, PERCENTS)
    check(got, oracle(f, np.zeros((h, w), np.int32), 1, PERCENTS), "constant frames")
    v = got.values.cpu().numpy()
    assert v[0, 0].tolist() == [0] + [12345] * 7 and v[1, 0].tolist() == [0] + [65534] * 7 and (v[2, 0] == 0).all()
    assert got.count.cpu().numpy().tolist() == [[h * w]] * 3


def test_values_on_bucket_edges():
    edges = np.array([0, 255, 256, 0xFEFF, 0xFF00, 65534, 65535], np.uint16)
    rng = np.random.default_rng(3)
    n, h, w = 3, 17, 33
    f = edges[rng.integers(0, edges.size, (n, h, w))]
    both(f, rng.integers(-1, 6, (h, w)).astype(np.int32), 5, PERCENTS, "edges")
    both(f[:, :, :32], np.zeros((n, 17, 32), np.int32), 1, PERCENTS, "edges, one region")
    # a region that is all 65535 gives 0 at every percent; its neighbour one below gives 65534
    lab = rect_map(h, w, 1, 3)
    g = f.copy()
    g[:, lab == 1] = 65535
    g[:, lab == 2] = 65534
    got = run(g, lab, 4, PERCENTS)
    check(got, oracle(g, lab, 4, PERCENTS), "all 65535")
    v = got.values.cpu().numpy()
    assert quantile_rank(17 * 11, 0.001) == 0  # the regions are 187 pixels: t == 0 at the first two percents
    assert (v[:, 1] == 0).all() and (v[:, 2, :2] == 0).all() and (v[:, 2, 2:] == 65534).all() and (v[:, 3] == -1).all()


def test_percent_lists():
    n, h, w = 2, 17, 33
    rng = np.random.default_rng(4)
    lab = rng.integers(0, 3, (h, w)).astype(np.int32)
    f = rng.integers(1000, 1101, (n, h, w)).astype(np.uint16)  # high bytes 3 (1000..1023) and 4
    both(f, lab, 3, (0.5,), "one")
    both(f, lab, 3, (0.5, 0.5, 0.25, 0.5, 0.25), "repeated")
    _, same = oracle(f, lab, 3, (0.5, 0.6))
    assert ((same[..., 0] >> 8) == (same[..., 1] >> 8)).all() and (same[..., 0] != same[..., 1]).any()
    both(f, lab, 3, (0.5, 0.6), "two percents in one high-byte bucket")
    _, apart = oracle(f, lab, 3, (0.1, 0.9))
    assert ((apart[..., 0] >> 8) != (apart[..., 1] >> 8)).all()
    both(f, lab, 3, (0.1, 0.9), "two percents in two buckets")
    both(f, lab, 3, (0.9, 0.1, 0.95, 0.15, 0.5, 1.0, 0.0, 0.12), "eight, unordered, in two buckets")
    got = run(frames_of(n, h, w, seed=4), lab, 3, 0.5)  # a float is a list of one
    assert tuple(got.values.shape) == (n, 3, 1)
    check(got, oracle(frames_of(n, h, w, seed=4), lab, 3, (0.5,)), "a float")


def test_ties_of_the_rank():
    """regions of 1, 2, 3, 5, 6 and 7 pixels at 0.25, 0.5 and 0.75: c * p ends in .5 for eight of them, and roundf goes up"""
    sizes = (1, 2, 3, 5, 6, 7)
    lab = np.full((4, 9), -1, np.int32)
    flat = lab.reshape(-1)
    at = 0
    for r, c in enumerate(sizes):
        flat[at:at + c] = r
        at += c + 1
    f = np.random.default_rng(5).permutation(36).astype(np.uint16).reshape(1, 4, 9) * 1500
    pc = (0.25, 0.5, 0.75)
    got = run(f, lab, len(sizes), pc)
    check(got, oracle(f, lab, len(sizes), pc), "ties")
    v = got.values.cpu().numpy()
    for r, c in enumerate(sizes):
        ordered = np.sort(f.reshape(-1)[flat == r]).astype(np.int64)
        assert v[0, r].tolist() == [int(ordered[quantile_rank(c, p) - 1]) if quantile_rank(c, p) else 0 for p in pc]


def test_sliced_inputs_at_odd_offsets():
    """frames and labels that start 2 and 4 bytes past an allocation (torch slices, used where they are): the pixel-by-pixel loads"""
    from librir_amd import device as D

    for (n, h, w), k in [((5, 17, 33), 9), ((3, 64, 80), 16), ((2, 64, 80), LDS_MAX + 7)]:
        f = frames_of(n + 1, h, w, seed=w + k)
        fr = dev16(f.reshape(-1))[1:1 + n * h * w].view(n, h, w)
        assert fr.data_ptr() % 16 == 2 and fr.is_contiguous()
        host = f.reshape(-1)[1:1 + n * h * w].reshape(n, h, w)
        lab = np.random.default_rng(h).integers(-1, k + 1, (n, h, w)).astype(np.int32)
        lab_t = dev32(np.concatenate([[7], lab.reshape(-1)]))[1:].view(n, h, w)
        check(D.region_quantiles(fr, lab_t, FOUR, k), oracle(host, lab, k, FOUR), ("per-frame slice", n, h, w))
        check(D.region_quantiles(fr, lab_t[1], FOUR, k), oracle(host, lab[1], k, FOUR), ("shared slice", n, h, w))
        check(D.region_quantiles(dev16(f)[::2], lab_t[0], FOUR, k), oracle(f[::2], lab[0], k, FOUR), ("strided", n, h, w))


def test_single_image_and_nregions_none():
    from librir_amd import device as D

    f = frames_of(2, 17, 33, seed=1)
    lab = np.random.default_rng(1).integers(-1, 7, (17, 33)).astype(np.int32)
    one = D.region_quantiles(dev16(f[0]), dev32(lab), FOUR, 7)
    assert tuple(one.count.shape) == (1, 7) and tuple(one.values.shape) == (1, 7, 4)
    check(one, oracle(f[:1], lab, 7, FOUR))
    auto = D.region_quantiles(dev16(f), dev32(lab), FOUR)
    assert tuple(auto.count.shape) == (2, 7)
    check(auto, oracle(f, lab, 7, FOUR))
    none = D.region_quantiles(dev16(f), dev32(np.full((17, 33), -5, np.int32)), 0.5)
    assert tuple(none.values.shape) == (2, 1, 1) and int(none.count.sum()) == 0 and (none.values == -1).all()
    empty = D.region_quantiles(dev16(f)[:0], dev32(lab), FOUR, 7)
    assert tuple(empty.count.shape) == (0, 7) and tuple(empty.values.shape) == (0, 7, 4)


ARGTYPES = [ct.c_void_p, ct.c_void_p] + [ct.c_int] * 5 + [ct.c_void_p, ct.c_int] + [ct.c_void_p] * 3 + [ct.c_size_t, ct.c_void_p]


def test_frame_groups_of_every_size_give_the_same_bits(lib):
    n, h, w, k = 7, 17, 33, 9
    pc = np.array([0.25, 0.5, 0.99], np.float32)
    f = frames_of(n, h, w, seed=7)
    lab = np.random.default_rng(7).integers(-1, k + 1, (n, h, w)).astype(np.int32)
    exp = oracle(f, lab, k, pc)
    fr, lt = dev16(f), dev32(lab)
    fn, query = lib.rir_region_quantiles_device, lib.rir_region_quantiles_workspace_bytes
    fn.argtypes = ARGTYPES
    query.argtypes, query.restype = [ct.c_int] * 6, ct.c_size_t
    b = frame_bytes(k, pc.size)
    assert query(w, h, n, 1, k, pc.size) == n * b
    stream = ct.c_void_p(torch.cuda.current_stream().cuda_stream)
    for size in (b, 2 * b, 3 * b, query(w, h, n, 1, k, pc.size), 2 * b + 8):
        work = torch.full((size // 8,), -1, dtype=torch.int64, device="cuda")  # what a workspace holds before the call does not matter
        count = torch.full((n, k), -7, dtype=torch.int32, device="cuda")
        values = torch.full((n, k, pc.size), -7, dtype=torch.int32, device="cuda")
        assert fn(fr.data_ptr(), lt.data_ptr(), w, h, n, 1, k, pc.ctypes.data, pc.size, count.data_ptr(), values.data_ptr(), work.data_ptr(), size,
                  stream) == 0
        check((count, values), exp, ("workspace", size // b))


def test_refused_arguments(lib):
    from librir_amd import device as D
    from librir_amd.low_level.misc import last_error

    f = dev16(frames_of(2, 8, 8, seed=0))
    lab = dev32(np.zeros((8, 8), np.int32))
    with pytest.raises(RuntimeError):
        D.region_quantiles(f, lab.to(torch.int64), 0.5, 1)
    with pytest.raises(RuntimeError):
        D.region_quantiles(f, lab.cpu(), 0.5, 1)
    with pytest.raises(ValueError):
        D.region_quantiles(f, lab, 1.5, 1)
    fn = lib.rir_region_quantiles_device
    fn.argtypes = ARGTYPES
    k, b = 4, frame_bytes(4, 2)
    buf = torch.zeros(8192, dtype=torch.int64, device="cuda")
    base = buf.data_ptr()
    pc = np.array([0.5, 0.9], np.float32)
    good = dict(fr=f.data_ptr(), lab=lab.data_ptr(), w=8, h=8, n=2, per=0, k=k, pc=pc.ctypes.data, q=2, count=base, values=base + 1024, work=base + 4096,
                wb=2 * b)

    def call(**kw):
        a = dict(good, **kw)
        return fn(*(a[x] for x in ("fr", "lab", "w", "h", "n", "per", "k", "pc", "q", "count", "values", "work", "wb")), None)

    assert call() == 0 and call(wb=b) == 0
    torch.cuda.synchronize()
    assert call(wb=b - 1) == -1 and "workspace" in last_error()
    assert call(work=base + 4100) == -1 and "workspace" in last_error()
    assert call(values=base + 8) == -1 and "overlap" in last_error()
    assert call(count=f.data_ptr()) == -1 and "overlap" in last_error()
    assert call(work=base + 1024) == -1 and "overlap" in last_error()
    for null in ("fr", "lab", "pc", "count", "values", "work"):
        assert call(**{null: None}) == -1, null
    for kw in (dict(w=0), dict(h=0), dict(n=-1), dict(per=2), dict(k=0), dict(k=65537), dict(q=0), dict(q=9)):
        assert call(**kw) == -1, kw
    for bad in (-0.5, 1.5, float("nan")):
        assert call(pc=np.array([0.5, bad], np.float32).ctypes.data) == -1 and "percent" in last_error()
    assert call(n=0) == 0  # nothing to do
    torch.cuda.synchronize()


def test_two_calls_on_one_stream_share_a_workspace(lib):
    """queued back to back with different inputs and percents: the second starts when the first has finished with the workspace"""
    n, h, w, k = 3, 64, 80, 16
    fa, fb = frames_of(n, h, w, seed=11), static_scene(n, h, w, seed=12)
    la, lb = rect_map(h, w, 4, 4), np.random.default_rng(12).integers(-1, k + 1, (h, w)).astype(np.int32)
    pa, pb = np.array([0.25, 0.5], np.float32), np.array([0.99, 0.01], np.float32)
    fn = lib.rir_region_quantiles_device
    fn.argtypes = ARGTYPES
    size = n * frame_bytes(k, 2)
    work = torch.empty(size // 8, dtype=torch.int64, device="cuda")
    outs = [(torch.empty((n, k), dtype=torch.int32, device="cuda"), torch.empty((n, k, 2), dtype=torch.int32, device="cuda")) for _ in range(2)]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ins = [(dev16(fa), dev32(la), pa), (dev16(fb), dev32(lb), pb)]
        for (fr, lt, pc), (count, values) in zip(ins, outs):
            assert fn(fr.data_ptr(), lt.data_ptr(), w, h, n, 0, k, pc.ctypes.data, 2, count.data_ptr(), values.data_ptr(), work.data_ptr(), size,
                      ct.c_void_p(side.cuda_stream)) == 0
    side.synchronize()
    check(outs[0], oracle(fa, la, k, pa), "first")
    check(outs[1], oracle(fb, lb, k, pb), "second")


def test_the_same_call_twice_gives_the_same_tensors():
    from librir_amd import device as D

    n, h, w = 7, 64, 80
    f = dev16(static_scene(n, h, w, seed=5))
    lab = dev32(np.random.default_rng(5).integers(0, 3, (h, w)).astype(np.int32))
    for k in (3, LDS_MAX + 3):
        a = D.region_quantiles(f, lab, PERCENTS, k)
        b = D.region_quantiles(f, lab, PERCENTS, k)
        assert torch.equal(a.count, b.count) and torch.equal(a.values, b.values)


def test_consistent_with_region_stats_and_find_median_pixel():
    from librir_amd import device as D

    n, h, w, k = 3, 64, 80, 16
    f = frames_of(n, h, w, seed=21)
    f[1] >>= 2  # a frame without 65535
    lab = np.random.default_rng(21).integers(-1, k + 1, (h, w)).astype(np.int32)
    fr, lt = dev16(f), dev32(lab)
    q = D.region_quantiles(fr, lt, (1.0, 0.5), k)
    rs = D.region_stats(fr, lt, k)
    assert torch.equal(q.count, rs.count)
    top, vmax = q.values[:, :, 0], rs.max
    assert torch.equal(top[vmax < 65535], vmax[vmax < 65535]) and (top[vmax == 65535] == 0).all() and (vmax[1] < 65535).all()
    ones = torch.ones((n, h, w), dtype=torch.uint8, device="cuda")
    full = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    for p in PERCENTS:
        assert torch.equal(D.region_quantiles(fr, full, p, 1).values[:, 0, 0], D.find_median_pixel(fr, p, ones)), p
    # and under a mask that is one region of a map
    mask = (lt == 3).to(torch.uint8).expand(n, h, w).contiguous()
    for j, p in enumerate((1.0, 0.5)):
        assert torch.equal(q.values[:, 3, j], D.find_median_pixel(fr, p, mask)), p


def test_hot_spot_components_from_label_images():
    from librir_amd import device as D
    from librir_amd.synthetic import s1_noisy_background

    n, h, w = 4, 64, 80
    f = s1_noisy_background(n, h, w, seed=4).copy()
    rng = np.random.default_rng(4)
    for i in range(n):
        for _ in range(8):
            y, x, r = rng.integers(5, h - 5), rng.integers(5, w - 5), rng.integers(1, 4)
            f[i, y - r:y + r + 1, x - r:x + r + 1] = 60000 + rng.integers(0, 5000, (2 * r + 1, 2 * r + 1))
    t = dev16(f)
    hot = (t.view(torch.int16).to(torch.int32) & 0xFFFF) > int(np.percentile(f, 99))
    labels, areas, _, counts = D.label_images(hot)
    kmax = int(counts.max())
    q = D.region_quantiles(t, labels, (0.5, 0.95), kmax)
    check(q, oracle(f, labels.cpu().numpy(), kmax, (0.5, 0.95)))
    cnt, c, a = q.count.cpu().numpy(), counts.cpu().numpy(), areas.cpu().numpy()
    for i in range(n):
        assert c[i] > 2 and np.array_equal(cnt[i, 1:c[i]], a[i, 1:c[i]])


def test_polygon_maps_with_shifts():
    from librir_amd import device as D

    n, h, w = 5, 64, 80
    f = static_scene(n, h, w, seed=8)
    polygons = [[(5, 5), (30, 8), (25, 30), (6, 25)], [(40, 10), (70, 12), (60, 50)], [(10, 40), (35, 45), (20, 60)]]
    shifts = np.array([[0, 0], [1.5, -2], [-3, 4], [10, 10], [-4.25, 0.5]], np.float64)
    maps = D.polygon_map(polygons, (h, w), shifts=shifts)
    assert tuple(maps.shape) == (n, h, w)
    q = D.region_quantiles(dev16(f), maps, FOUR)
    exp = oracle(f, maps.cpu().numpy(), 3, FOUR)
    check(q, exp)
    assert (exp[0] > 0).all()


def test_host_entry_equals_device_entry():
    from librir_amd import signal_processing as S

    for (n, h, w), k, per_frame, pc in [((3, 17, 33), 9, False, FOUR), ((2, 17, 33), 9, True, PERCENTS), ((1, 1, 1), 1, False, (0.5,)),
                                        ((5, 64, 80), LDS_MAX + 1, True, (0.5, 0.99))]:
        f = frames_of(n, h, w, seed=n + k)
        lab = np.random.default_rng(k).integers(-1, k + 1, (n, h, w) if per_frame else (h, w)).astype(np.int32)
        host = S.region_quantiles(f, lab, pc, k)
        assert isinstance(host.count, np.ndarray) and isinstance(host.values, np.ndarray)
        exp = oracle(f, lab, k, pc)
        check(host, exp, ("host", n, h, w, k))
        check(run(f, lab, k, pc), exp, ("device", n, h, w, k))
    host = S.region_quantiles(f[0], lab[0], 0.5)
    check(host, oracle(f[:1], lab[0], int(lab[0].max()) + 1, (0.5,)), "one image, nregions from the map")
    # 65 536 regions at eight percents: one frame's outputs and workspace are beyond a slab, so the frames go one by one
    f = frames_of(2, 17, 33, seed=9)
    lab = np.random.default_rng(9).integers(65500, 65537, (17, 33)).astype(np.int32)
    check(S.region_quantiles(f, lab, PERCENTS, 65536), oracle(f, lab, 65536, PERCENTS), "frame by frame")


def test_host_entry_frame_by_frame_with_per_frame_maps():
    """65 536 regions at eight percents again, now with one map per frame: every frame is its own slab and takes its own map up with it"""
    from librir_amd import signal_processing as S

    f = frames_of(3, 17, 33, seed=10)
    lab = np.random.default_rng(10).integers(65500, 65537, (3, 17, 33)).astype(np.int32)
    assert not np.array_equal(lab[0], lab[1]) and not np.array_equal(lab[1], lab[2])
    check(S.region_quantiles(f, lab, PERCENTS, 65536), oracle(f, lab, 65536, PERCENTS), "frame by frame, per-frame maps")


def record(path, frames):
    from librir_amd.video_io import IRSaver

    n, h, w = frames.shape
    with IRSaver(str(path), w, h, h) as s:
        for i in range(n):
            s.add_image(frames[i], i * 20000000 + 7)
    return str(path)


@pytest.mark.parametrize("bad_pixels", [False, True])
def test_movie_region_quantiles(tmp_path, bad_pixels):
    from librir_amd import device as D
    from librir_amd.synthetic import inject_bad_pixels, s1_noisy_background
    from librir_amd.video_io import IRMovie

    n, h, w = 23, 40, 48
    arr = inject_bad_pixels(s1_noisy_background(n, h, w, seed=12), 7)
    lab = rect_map(h, w, 3, 3)
    lab[::5, ::3] = -1
    with IRMovie.from_filename(record(tmp_path / "m.h264", arr)) as mov:
        mov.bad_pixels_correction = bad_pixels
        for pieces in (None, 5 * h * w * 2):
            if pieces:
                mov._STATS_PIECE_BYTES = pieces  # the selections below cross pieces of five images
            for sel in (slice(None), slice(2, 21, 3), slice(1, None, 2), 5, -1):
                stack = mov.to_tensor(sel)
                want = D.region_quantiles(stack, dev32(lab), FOUR, 9)
                got = mov.region_quantiles(lab, FOUR, sel)
                assert torch.equal(got.count, want.count) and torch.equal(got.values, want.values), (pieces, sel)
                got = mov.region_quantiles(dev32(lab), FOUR, sel, 9)
                assert torch.equal(got.values, want.values), (pieces, sel)
                check(got, oracle(np.asarray(mov[sel]).reshape(-1, h, w), lab, 9, FOUR), ("oracle", pieces, sel))
        with pytest.raises(RuntimeError):
            mov.region_quantiles(lab.astype(np.int64), 0.5)
        with pytest.raises(ValueError):
            mov.region_quantiles(lab, (0.5, 2.0))
