"""GPU: per-pixel statistics over time, bit for bit against the oracle of test_pixel_stats_cpu.py - shapes, stack lengths around the number
of waves that split the time axis and around the sets of frames a wave walks, each group of outputs alone and both, ties, long thin stacks that are cut into slabs, the largest sums,
accumulating in and out of order, sliced inputs, refused arguments, stream order, reproducibility, the host entry and recordings read
through IRMovie.pixel_stats."""
import ctypes as ct
import time

import numpy as np
import pytest

from test_gpu_pixel_quantiles import LENGTHS
from test_gpu_region_stats import dev16, frames_of, record
from test_pixel_stats_cpu import DEV_ARGS, FIELDS, SUMS, empty_state, four_values
from test_pixel_stats_cpu import pixel_stats_oracle as small_oracle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GROUPS = [(True, True), (True, False), (False, True)]


def oracle(frames, t0=0):
    """pixel_stats_oracle without its int64 copy of the whole stack: the sums of squares are taken a few frames at a time"""
    frames = np.asarray(frames)
    if frames.size <= 1 << 22:
        return small_oracle(frames, t0)
    n = frames.shape[0]
    sq = np.zeros(frames.shape[1:], np.int64)
    for a in range(0, n, 8):
        v = frames[a:a + 8].astype(np.int64)
        sq += (v * v).sum(0)
    return {"sum": frames.sum(0, dtype=np.int64), "sumsq": sq, "min": frames.min(0).astype(np.int32), "max": frames.max(0).astype(np.int32),
            "argmin": (frames.argmin(0) + t0).astype(np.int32), "argmax": (frames.argmax(0) + t0).astype(np.int32)}


def check(ps, exp, what="", sums=True, extremes=True):
    for k, t in zip(FIELDS, ps):
        if not (sums if k in SUMS else extremes):
            assert t is None, (what, k)
            continue
        got = t.cpu().numpy() if hasattr(t, "cpu") else t
        assert got.dtype == exp[k].dtype and got.shape == exp[k].shape, (what, k, got.dtype, got.shape)
        if not np.array_equal(got, exp[k]):
            bad = np.argwhere(got != exp[k])[:5]
            raise AssertionError("%s %s differs at %s: got %s, expected %s" % (what, k, bad.tolist(), got[tuple(bad.T)], exp[k][tuple(bad.T)]))


def check_groups(frames_dev, exp, what, t0=0):
    from librir_amd import device as D

    n = frames_dev.shape[0] if frames_dev.dim() == 3 else 1
    for sums, extremes in GROUPS:
        ps = D.pixel_stats(frames_dev, sums, extremes, t0)
        assert ps.count == n
        check(ps, exp, (what, sums, extremes), sums, extremes)


SMALL_SHAPES, LARGE_SHAPES = [(1, 1), (3, 5), (17, 33)], [(512, 640), (768, 1024)]
# four waves split the frames; a wave enters the walk's main loop at 8 frames and ends on 0 .. 7 left over: every count of a wave around its
# multiples of 8 (test_gpu_pixel_quantiles.py's list) on the small shapes, the lengths around the number of waves on the large ones
LENGTHS_AND_SHAPES = [(n, h, w) for n in LENGTHS for h, w in SMALL_SHAPES] + [(n, h, w) for n in [1, 2, 3, 4, 5, 7, 257] for h, w in LARGE_SHAPES]


@pytest.mark.parametrize("n,h,w", LENGTHS_AND_SHAPES)
def test_shapes_and_lengths(n, h, w):
    f = frames_of(n, h, w, seed=h * 3 + n)
    check_groups(dev16(f), oracle(f), (h, w, n))


def test_single_image_is_a_stack_of_one():
    from librir_amd import device as D

    f = frames_of(1, 17, 33, seed=1)
    ps = D.pixel_stats(dev16(f[0]), t0=12)
    assert ps.count == 1 and all(tuple(t.shape) == (17, 33) for t in ps)
    check(ps, oracle(f, 12))
    none = D.pixel_stats(dev16(f[:0]))
    assert none.count == 0
    check(none, empty_state(17, 33))


@pytest.mark.parametrize("h,w", [(17, 33), (512, 640)])
def test_ties_fall_to_the_lowest_index(h, w):
    f = four_values(h, 64, h, w)
    exp = oracle(f, 5)
    assert (exp["argmin"] > 5).any() and (exp["argmax"] > 5).any()
    check_groups(dev16(f), exp, ("ties", h, w), t0=5)
    const = np.full((64, h, w), 21845, np.uint16)
    ps_exp = oracle(const)
    assert not ps_exp["argmin"].any() and not ps_exp["argmax"].any()
    check_groups(dev16(const), ps_exp, ("constant", h, w))


@pytest.mark.parametrize("n,h,w", [(70001, 3, 5), (70001, 1, 1), (5000, 64, 80)])
def test_long_and_thin_stacks_are_split_along_time(lib, n, h, w):
    f = frames_of(n, h, w, seed=n + w)
    f[n - 1, 0, 0] = 65535  # a maximum in the last frame alone
    f[:n - 1, 0, 0] = np.minimum(f[:n - 1, 0, 0], 65534)
    if h * w > 1:
        f[0, h - 1, w - 1] = f[n - 1, h - 1, w - 1] = 0  # a minimum in the first and, tied, in the last
    fn = lib.rir_pixel_stats_workspace_bytes
    fn.argtypes = [ct.c_int] * 3
    fn.restype = ct.c_size_t
    assert fn(w, h, n) >= 2 * 20 * h * w  # more than one slab
    exp = oracle(f, 3)
    assert exp["argmax"][0, 0] == 3 + n - 1 and (h * w == 1 or exp["argmin"][h - 1, w - 1] == 3)
    check_groups(dev16(f), exp, ("thin", n, h, w), t0=3)


def test_largest_sums_and_all_zeros():
    h, w = 768, 1024
    f = np.full((3, h, w), 65535, np.uint16)
    f[1, 100, 200] = 3
    exp = oracle(f)
    assert exp["sumsq"][0, 0] == 3 * 65535 ** 2 and exp["argmin"][100, 200] == 1 and exp["argmax"][100, 200] == 0 and exp["argmin"][0, 0] == 0
    check_groups(dev16(f), exp, "65535")
    z = np.zeros((3, h, w), np.uint16)
    check_groups(dev16(z), oracle(z), "zeros")


@pytest.mark.parametrize("n,h,w,cuts", [(100, 67, 83, [0, 1, 38, 39, 77, 100]), (40, 512, 640, [0, 13, 14, 33, 40])])
def test_accumulating_in_and_out_of_order(n, h, w, cuts):
    from librir_amd import device as D

    f = frames_of(n, h, w, seed=n)
    t = dev16(f)
    batches = list(zip(cuts, cuts[1:]))
    assert any(b - a == 1 for a, b in batches)
    for sums, extremes in GROUPS:
        whole = D.pixel_stats(t, sums, extremes)
        check(whole, oracle(f), ("whole", sums, extremes), sums, extremes)
        acc = D.PixelStatsAccumulator(sums, extremes)
        before = acc.result()
        assert before.count == 0 and all(x is None or x.numel() == 0 for x in before)
        for a, b in batches:
            acc.push(t[a:b])
        shuffled = D.PixelStatsAccumulator(sums, extremes, shape=(h, w))
        check(shuffled.result(), empty_state(h, w), "empty", sums, extremes)
        order = batches[1::2] + batches[0::2][::-1]
        for a, b in order:
            shuffled.push(t[a:b], a)
        for got in (acc.result(), shuffled.result()):
            assert got.count == n
            for x, y in zip(got, whole):
                assert (x is None and y is None) or torch.equal(x, y)
        # reset: the next sequence starts from the empty state and from time 0
        acc.reset()
        assert acc.result().count == 0
        acc.push(t[:7])
        check(acc.result(), oracle(f[:7]), "after reset", sums, extremes)
        # two halves computed separately (with their time origins) and merged, in both orders
        half = cuts[2]
        lo, hi = D.pixel_stats(t[:half], sums, extremes), D.pixel_stats(t[half:], sums, extremes, t0=half)
        for first, second in ((lo, hi), (hi, lo)):
            m = D.PixelStatsAccumulator(sums, extremes)
            m.merge(first)
            m.merge(second)
            got = m.result()
            assert got.count == n
            for x, y in zip(got, whole):
                assert (x is None and y is None) or torch.equal(x, y)


def test_time_origin_up_to_the_int32_limit():
    from librir_amd import device as D

    f = four_values(3, 9, 17, 33)
    t0 = (1 << 31) - 1 - 9
    check_groups(dev16(f), oracle(f, t0), "t0 max", t0=t0)
    acc = D.PixelStatsAccumulator()
    acc.push(dev16(f[4:]), t0 + 4)
    acc.push(dev16(f[:4]), t0)
    check(acc.result(), oracle(f, t0), "t0 max, accumulated")
    with pytest.raises(ValueError):
        acc.push(dev16(f[:1]))  # continues at 2^31 - 1: past the last index


def test_sliced_inputs_at_odd_offsets():
    """a stack that starts 2 bytes past an allocation, an every-other-frame view, odd frame sizes with n > 1: the pixel-by-pixel path"""
    for n, h, w in [(5, 17, 33), (3, 512, 640), (6, 7, 9), (2, 1, 1)]:
        f = frames_of(n + 1, h, w, seed=w)
        flat = dev16(f.reshape(-1))
        fr = flat[1:1 + n * h * w].view(n, h, w)
        assert fr.data_ptr() % 16 == 2
        check_groups(fr, oracle(f.reshape(-1)[1:1 + n * h * w].reshape(n, h, w)), ("offset", n, h, w))
        check_groups(dev16(f)[::2], oracle(f[::2]), ("strided", n, h, w))
    f = frames_of(300, 21, 31, seed=4)  # odd frame size: every other frame starts 2 bytes off a 16-byte boundary
    check_groups(dev16(f), oracle(f), "odd frames")


def test_refused_arguments(lib):
    from librir_amd import device as D
    from librir_amd.low_level.misc import last_error

    f = dev16(frames_of(2, 8, 8, seed=0))
    with pytest.raises(RuntimeError):
        D.pixel_stats(f.view(torch.int16))
    with pytest.raises(RuntimeError):
        D.pixel_stats(f.cpu())
    with pytest.raises(ValueError):
        D.pixel_stats(f, sums=False, extremes=False)
    fn = lib.rir_pixel_stats_device
    fn.argtypes = DEV_ARGS
    need = lib.rir_pixel_stats_workspace_bytes
    need.argtypes = [ct.c_int] * 3
    need.restype = ct.c_size_t
    wb = need(8, 8, 2)
    assert wb > 0
    buf = torch.zeros(4096, dtype=torch.int64, device="cuda")
    base = buf.data_ptr()
    outs = [base + 1024 * i for i in range(6)]
    work = base + 1024 * 8

    def args(o=outs, wk=work, wbytes=wb, w=8, h=8, n=2, t0=0, acc=0, fr=f.data_ptr()):
        return [fr, w, h, n, t0, acc] + list(o) + [wk, wbytes, None]

    assert fn(*args()) == 0
    assert fn(*args(o=[None, None] + outs[2:])) == 0  # extremes alone
    assert fn(*args(o=outs[:2] + [None] * 4)) == 0  # sums alone
    torch.cuda.synchronize()
    assert fn(*args(o=[None] * 6)) == -1 and "group" in last_error()
    assert fn(*args(o=[outs[0], None] + outs[2:])) == -1 and "group" in last_error()  # half a group
    assert fn(*args(o=outs[:5] + [None])) == -1 and "group" in last_error()
    assert fn(*args(o=outs[:2] + [None, outs[3], None, None])) == -1
    assert fn(*args(wbytes=wb - 1)) == -1 and "workspace" in last_error()
    assert fn(*args(wk=None)) == -1
    assert fn(*args(fr=None)) == -1
    assert fn(*args(o=[outs[0], outs[0] + 8] + outs[2:])) == -1 and "overlap" in last_error()
    assert fn(*args(o=[f.data_ptr()] + outs[1:])) == -1 and "overlap" in last_error()
    assert fn(*args(o=outs[:5] + [f.data_ptr() + 64])) == -1 and "overlap" in last_error()
    assert fn(*args(wk=outs[3])) == -1 and "overlap" in last_error()
    assert fn(*args(wk=f.data_ptr())) == -1
    for bad in (dict(w=0), dict(h=-1), dict(n=-1), dict(t0=-1), dict(t0=(1 << 31) - 2), dict(acc=2)):
        assert fn(*args(**bad)) == -1, bad
    before = buf.clone()
    assert fn(*args(n=0)) == 0  # nframes 0: nothing to do
    assert fn(*args(n=0, o=[None] * 6, wk=None)) == 0
    torch.cuda.synchronize()
    assert torch.equal(buf, before)


def test_queued_behind_the_kernel_that_writes_the_frames():
    """the frames are written by kernels on a side stream and reduced on that stream at once"""
    from librir_amd import device as D

    n, h, w = 200, 512, 640
    f = frames_of(n, h, w, seed=9)
    host = torch.from_numpy(f.view(np.int16)).pin_memory()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        src = torch.empty((n, h, w), dtype=torch.int16, device="cuda")
        src.copy_(host, non_blocking=True)
        src.add_(0)
        ps = D.pixel_stats(src.view(torch.uint16))
    side.synchronize()
    check(ps, oracle(f))


def test_two_runs_give_equal_bytes():
    from librir_amd import device as D

    f = dev16(frames_of(256, 512, 640, seed=5))
    a, b = D.pixel_stats(f), D.pixel_stats(f)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    thin = dev16(frames_of(3000, 8, 8, seed=6))  # the form with partials and a fold
    a, b = D.pixel_stats(thin), D.pixel_stats(thin)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_host_entry_equals_device_entry():
    from librir_amd import device as D
    from librir_amd import signal_processing as S

    for n, h, w in [(3, 17, 33), (1, 1, 1), (5, 64, 80), (600, 4, 8)]:
        f = frames_of(n, h, w, seed=n + h)
        exp = oracle(f)
        for sums, extremes in GROUPS:
            host = S.pixel_stats(f, sums, extremes)
            assert host.count == n
            check(host, exp, ("host", n, h, w), sums, extremes)
            check(D.pixel_stats(dev16(f), sums, extremes), exp, ("device", n, h, w), sums, extremes)
    none = S.pixel_stats(np.zeros((0, 4, 5), np.uint16))
    assert none.count == 0
    check(none, empty_state(4, 5))
    # more than one 64 MiB slab of frames, accumulated on the device
    f = frames_of(230, 512, 640, seed=3)
    exp = oracle(f)
    check(S.pixel_stats(f), exp, "slabs")
    check(S.pixel_stats(f, sums=False), exp, "slabs, extremes", sums=False)
    check(D.pixel_stats(dev16(f)), exp, "device")


@pytest.mark.parametrize("bad_pixels", [False, True])
def test_movie_pixel_stats(tmp_path, bad_pixels):
    from librir_amd.synthetic import inject_bad_pixels, s1_noisy_background
    from librir_amd.video_io import IRMovie

    n, h, w = 43, 67, 83
    arr = inject_bad_pixels(s1_noisy_background(n, h, w, seed=12), 7)
    with IRMovie.from_filename(record(tmp_path / "m.h264", arr)) as mov:
        mov.bad_pixels_correction = bad_pixels
        for sel in (slice(None), slice(2, 40, 3), 5, -1):
            images = np.asarray(mov[sel]).reshape(-1, h, w)
            exp = oracle(images)
            ps = mov.pixel_stats(sel)
            assert ps.count == len(images)
            check(ps, exp, ("both", sel))
            check(mov.pixel_stats(sel, sums=False), exp, ("extremes", sel), sums=False)
            check(mov.pixel_stats(sel, extremes=False), exp, ("sums", sel), extremes=False)
        with pytest.raises(ValueError):
            mov.pixel_stats(slice(None, None, -1))
        with pytest.raises(IndexError):
            mov.pixel_stats(n)
        with pytest.raises(TypeError):
            mov.pixel_stats([1, 2])
        with pytest.raises(ValueError):
            mov.pixel_stats(sums=False, extremes=False)


def test_movie_pixel_stats_in_uneven_pieces(tmp_path):
    from librir_amd.synthetic import s1_noisy_background
    from librir_amd.video_io import IRMovie

    n, h, w = 50, 40, 48
    arr = s1_noisy_background(n, h, w, seed=2)
    with IRMovie.from_filename(record(tmp_path / "p.h264", arr)) as mov:
        mov._STATS_PIECE_BYTES = 11 * h * w * 2
        for sel in (slice(None), slice(1, None, 2), slice(3, 45, 7)):
            check(mov.pixel_stats(sel), oracle(np.asarray(mov[sel])), sel)


# Rate floors over 1 000 frames of 640x512 (uint16) in one call: about 0.7 of what tests/perf/pixel_stats_time.py measured when the feature
# was added, on one MI355X.
FLOOR_BOTH = 5.4e6  # measured 7.77 M frames/s (both groups)
FLOOR_EXTREMES = 6.0e6  # measured 8.67-8.75 M (extremes only)


@pytest.mark.perf
@pytest.mark.parametrize("sums,floor", [(True, FLOOR_BOTH), (False, FLOOR_EXTREMES)])
def test_rate_floor(sums, floor):
    from librir_amd import device as D

    n, h, w = 1000, 512, 640
    src = torch.randint(0, 65536, (n, h, w), dtype=torch.int32, device="cuda").to(torch.int16).view(torch.uint16)
    for _ in range(3):
        D.pixel_stats(src, sums=sums)
    torch.cuda.synchronize()
    reps = 20
    t0 = time.perf_counter()
    for _ in range(reps):
        D.pixel_stats(src, sums=sums)
    torch.cuda.synchronize()
    rate = reps * n / (time.perf_counter() - t0)
    assert rate >= floor, "sums %s: %.3g frames/s, floor %.3g" % (sums, rate, floor)
