"""GPU: the temporal median filter, bit for bit against the oracle of test_temporal_median_cpu.py (np.sort over the truncated window, then the
threshold and rows rules) - shapes, stack lengths, every window, partial calls, overlap, streaming, the host entry, stream order, spike
removal, reading recordings through IRMovie.to_tensor and recording the stream's output."""
import ctypes as ct
import time

import numpy as np
import pytest

from test_temporal_median_cpu import temporal_median_oracle as oracle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

WINDOWS = list(range(1, 16, 2)) + [17, 31, 63]


def stack_of(n, h, w, seed):
    """random values across the whole range, with 0 and 65535 runs"""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 65536, (n, h, w), dtype=np.uint16)
    s.reshape(n, -1)[:, ::7] = 0
    s.reshape(n, -1)[:, 3::11] = 65535
    return s


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda().view(torch.uint16)


def host(t):
    return t.cpu().view(torch.int16).numpy().view(np.uint16)


def run(stack, window, **kw):
    from librir_amd import device as D

    return host(D.temporal_median(dev(stack), window, **kw))


@pytest.mark.parametrize("h,w", [(67, 83), (3, 5), (1, 1)])
@pytest.mark.parametrize("n", [1, 2, 5, 64, 300])
def test_every_window_small_shapes(h, w, n):
    s = stack_of(n, h, w, seed=n * 7 + h)
    for window in WINDOWS:
        assert np.array_equal(run(s, window), oracle(s, window)), (h, w, n, window)


@pytest.mark.parametrize("n,windows", [(64, [1, 3, 5, 9, 15, 63]), (300, [9]), (5, [3, 63]), (1, [5])])
def test_full_frames(n, windows):
    s = stack_of(n, 512, 640, seed=n)
    for window in windows:
        assert np.array_equal(run(s, window), oracle(s, window)), (n, window)


@pytest.mark.parametrize("h,w", [(512, 640), (67, 83)])
@pytest.mark.parametrize("threshold", [0, 1, 1000])
def test_threshold_and_rows(h, w, threshold):
    s = stack_of(24, h, w, seed=threshold + h)
    for window in (3, 9, 15):
        for rows in (h, h - 3, 0):
            got = run(s, window, threshold=threshold, rows=rows)
            assert np.array_equal(got, oracle(s, window, threshold, rows)), (window, rows)


@pytest.mark.parametrize("h,w", [(512, 640), (67, 83), (3, 5)])
def test_partial_calls(h, w):
    n = 40
    s = stack_of(n, h, w, seed=11)
    for window in (3, 7, 15, 63):
        for first, count, step in [(0, n, 1), (5, 20, 1), (0, 3, 1), (37, 3, 1), (1, 19, 2), (0, 4, window), (2, 5, window + 1), (39, 1, 1), (12, 0, 1)]:
            if count and first + (count - 1) * step > n - 1:
                continue
            got = run(s, window, first=first, count=count, step=step)
            assert np.array_equal(got, oracle(s, window, first=first, count=count, step=step)), (window, first, count, step)
    assert np.array_equal(run(s, 5, first=3, step=4), oracle(s, 5, first=3, step=4))  # count=None: to the end


def test_unaligned_and_sliced_stacks():
    """frames that start at a 2-byte offset (a slice of a stack of odd w*h, a view one pixel in): the pixel-by-pixel path"""
    from librir_amd import device as D

    s = stack_of(30, 67, 83, seed=4)
    t = dev(s)
    for window in (3, 9, 31):
        got = D.temporal_median(t[1:], window).cpu().view(torch.int16).numpy().view(np.uint16)
        assert np.array_equal(got, oracle(s[1:], window))
    flat = torch.from_numpy(stack_of(1, 1, 1 + 20 * 64 * 64, seed=5).reshape(-1).view(np.int16)).cuda().view(torch.uint16)
    view = flat[1:].view(20, 64, 64)
    exp = oracle(view.cpu().view(torch.int16).numpy().view(np.uint16), 5)
    assert np.array_equal(D.temporal_median(view, 5).cpu().view(torch.int16).numpy().view(np.uint16), exp)


def test_overlap_is_refused(lib):
    from librir_amd import device as D
    from librir_amd.low_level.misc import last_error

    t = torch.zeros((10, 8, 8), dtype=torch.uint16, device="cuda")
    with pytest.raises(RuntimeError):
        D.temporal_median(t, 3, out=t)
    with pytest.raises(RuntimeError):
        D.temporal_median(t[:6], 3, out=t[5:])
    big = torch.zeros((20, 8, 8), dtype=torch.uint16, device="cuda")
    with pytest.raises(RuntimeError):
        D.temporal_median(big[2:12], 3, out=big[:10])
    assert "overlap" in last_error()
    out = D.temporal_median(big[:10], 3, out=big[10:])  # adjacent, not overlapping
    assert out.data_ptr() == big[10:].data_ptr()
    f = lib.rir_temporal_median_device
    f.argtypes = [ct.c_void_p, ct.c_void_p] + [ct.c_int] * 9 + [ct.c_void_p]
    p = big.data_ptr()
    assert f(p, p + 2, 8, 8, 5, 0, 5, 1, 3, 0, 8, None) == -1
    assert f(p, p + 5 * 128, 8, 8, 5, 0, 5, 1, 3, 0, 8, None) == 0
    assert f(p, None, 8, 8, 5, 0, 5, 1, 3, 0, 8, None) == -1
    assert f(p, p + 5 * 128, 8, 8, 5, 0, 0, 1, 3, 0, 8, None) == 0  # count 0: nothing to do
    for bad in [(8, 8, 5, 0, 5, 1, 4, 0, 8), (8, 8, 5, 0, 6, 1, 3, 0, 8), (8, 8, 5, 0, 5, 1, 3, 70000, 8), (8, 8, 5, 0, 5, 1, 3, 0, 9),
                (8, 8, 5, 0, 3, 0, 3, 0, 8), (8, 8, 5, 3, 2, 2, 3, 0, 8)]:
        assert f(p, p + 10 * 128, *bad, None) == -1, bad
    torch.cuda.synchronize()


def split_points(rng, n):
    cuts, k = [0], 0
    while k < n:
        k = min(n, k + int(rng.choice([0, 0, 1, 1, 2, 3, 5, 9, 17, 40])))
        cuts.append(k)
    return cuts


@pytest.mark.parametrize("window", [1, 3, 5, 9, 15, 31, 63])
@pytest.mark.parametrize("threshold,rows", [(0, None), (1000, 29)])
def test_stream_equals_one_call(window, threshold, rows):
    from librir_amd import device as D

    n, h, w = 130, 32, 37
    s = stack_of(n, h, w, seed=window)
    t = dev(s)
    exp = oracle(s, window, threshold, rows)
    tm = D.TemporalMedian(window, threshold, rows)
    for seed in range(4):
        cuts = split_points(np.random.default_rng(seed + 100 * window), n)
        parts = [tm.push(t[a:b].clone()) for a, b in zip(cuts, cuts[1:])]
        parts.append(tm.finish())
        assert all(p.shape[1:] == (h, w) for p in parts)
        got = torch.cat(parts).cpu().view(torch.int16).numpy().view(np.uint16)
        assert np.array_equal(got, exp), (seed, cuts)
    assert tm.push(t[:2]).shape[0] == max(0, 2 - window // 2)
    with pytest.raises(ValueError):
        tm.push(t[:2, :, :5])
    tm.reset()
    assert tm.push(t[:0]).shape[0] == 0 and tm.finish().shape[0] == 0


def test_host_entry_equals_device_entry():
    from librir_amd import signal_processing as S

    for (n, h, w), window, threshold, rows in [((50, 67, 83), 7, 0, 67), ((20, 3, 5), 63, 1, 1), ((9, 1, 1), 3, 0, 1)]:
        s = stack_of(n, h, w, seed=n)
        assert np.array_equal(S.temporal_median(s, window, threshold, rows), run(s, window, threshold=threshold, rows=rows))
        assert np.array_equal(S.temporal_median(s, window, threshold, rows), oracle(s, window, threshold, rows))
    # larger than the slab (64 MiB of frames): three slabs with halo
    s = stack_of(300, 512, 640, seed=3)
    for window in (9, 63):
        assert np.array_equal(S.temporal_median(s, window), run(s, window)), window
    assert np.array_equal(S.temporal_median(s, 9), oracle(s, 9))


def test_stream_order_without_synchronise():
    """the input is written by a kernel on a side stream and filtered on that stream at once"""
    from librir_amd import device as D

    s = stack_of(200, 512, 640, seed=9)
    host = torch.from_numpy(s.view(np.int16)).pin_memory()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        src = torch.empty((200, 512, 640), dtype=torch.int16, device="cuda")
        src.copy_(host, non_blocking=True)
        src.add_(0)  # (a kernel on the side stream writes the frames)
        got = D.temporal_median(src.view(torch.uint16), 5)
    side.synchronize()
    assert np.array_equal(got.cpu().view(torch.int16).numpy().view(np.uint16), oracle(s, 5))


def test_spike_removal():
    """a scene smooth in space that steps up every 10 frames, with +5 000 spikes that last one frame: the median of 3 with threshold 1 000
    gives the clean sequence back exactly"""
    n, h, w = 60, 64, 96
    yy, xx = np.mgrid[0:h, 0:w]
    base = 20000 + 1000 * np.sin(xx / 9.0) * np.cos(yy / 13.0) + yy * 3
    clean = np.stack([(base + 7 * (t // 10)).astype(np.uint16) for t in range(n)])
    rng = np.random.default_rng(1)
    noisy = clean.copy()
    # spikes two frames or more from a step and from each other at one pixel, so every window of 3 holds at most one spike and no step
    t, y, x = rng.integers(2, n - 2, 600), rng.integers(0, h, 600), rng.integers(0, w, 600)
    keep = (t % 10 >= 2) & (t % 10 <= 7)
    seen = set()
    for i in np.flatnonzero(keep):
        if any((t[i] + d, y[i], x[i]) in seen for d in (-2, -1, 0, 1, 2)):
            keep[i] = False
        else:
            seen.add((t[i], y[i], x[i]))
    noisy[t[keep], y[keep], x[keep]] += 5000
    assert keep.sum() > 200 and (noisy != clean).sum() == keep.sum()
    assert np.array_equal(oracle(noisy, 3, 1000), clean)
    assert np.array_equal(run(noisy, 3, threshold=1000), clean)


def record(path, frames):
    from librir_amd.video_io import IRSaver

    n, h, w = frames.shape
    with IRSaver(str(path), w, h, h) as s:
        for i in range(n):
            s.add_image(frames[i], i * 20000000 + 7)
    return str(path)


SELECTIONS = [slice(None), slice(3, 17), slice(2, 40, 3), slice(-9, -2), slice(-20, None, 3), 0, 5, -1, slice(8, 8), slice(0, None, 13)]


@pytest.mark.parametrize("bad_pixels", [False, True])
def test_to_tensor_with_temporal_median(tmp_path, bad_pixels):
    from librir_amd.synthetic import inject_bad_pixels, s1_noisy_background
    from librir_amd.video_io import IRMovie

    n, h, w = 43, 67, 83
    arr = inject_bad_pixels(s1_noisy_background(n, h, w, seed=12), 7)
    with IRMovie.from_filename(record(tmp_path / "m.h264", arr)) as mov:
        mov.bad_pixels_correction = bad_pixels
        data = mov.data
        before = mov.load_pos(4).copy()
        for window, threshold in [(3, 0), (9, 0), (5, 40), (63, 0)]:
            full = oracle(data, window, threshold)
            for sel in SELECTIONS:
                positions = [sel + (n if sel < 0 else 0)] if isinstance(sel, int) else list(range(n))[sel]
                got = mov.to_tensor(sel, temporal_median=window, median_threshold=threshold)
                assert got.dtype == torch.uint16 and tuple(got.shape) == (len(positions), h, w)
                assert np.array_equal(got.cpu().view(torch.int16).numpy().view(np.uint16), full[positions]), (window, sel)
                gf = mov.to_tensor(sel, dtype=torch.float32, temporal_median=window, median_threshold=threshold)
                assert gf.dtype == torch.float32 and torch.equal(gf, got.float()), (window, sel)
        assert mov._current == 4 and np.array_equal(mov.load_pos(4), before)
        assert np.array_equal(mov.to_tensor(slice(None)).cpu().view(torch.int16).numpy().view(np.uint16), data)


def test_to_tensor_median_reads_in_pieces(tmp_path):
    """pieces smaller than the selection: the halo of every piece comes from the recording"""
    from librir_amd.synthetic import s1_noisy_background
    from librir_amd.video_io import IRMovie

    n, h, w = 50, 40, 48
    arr = s1_noisy_background(n, h, w, seed=2)
    with IRMovie.from_filename(record(tmp_path / "p.h264", arr)) as mov:
        mov._MEDIAN_PIECE_BYTES = 11 * h * w * 2
        for sel, window in [(slice(None), 5), (slice(1, None, 2), 9), (slice(3, 45, 20), 7)]:
            got = mov.to_tensor(sel, temporal_median=window).cpu().view(torch.int16).numpy().view(np.uint16)
            assert np.array_equal(got, oracle(arr, window)[sel]), (sel, window)


def test_stream_into_saver(tmp_path):
    from librir_amd import device as D
    from librir_amd.synthetic import s1_noisy_background
    from librir_amd.video_io import IRMovie, IRSaver

    n, h, w = 70, 64, 96
    arr = s1_noisy_background(n, h, w, seed=6)
    t = dev(arr)
    tm = D.TemporalMedian(7, 0, h - 3)
    path = str(tmp_path / "s.h264")
    written = 0
    with IRSaver(path, w, h, h) as s:
        for a, b in [(0, 2), (2, 3), (3, 30), (30, 30), (30, 70)]:
            out = tm.push(t[a:b])
            s.add_images(out, np.arange(written, written + out.shape[0], dtype=np.int64) * 1000)
            written += out.shape[0]
        out = tm.finish()
        s.add_images(out, np.arange(written, written + out.shape[0], dtype=np.int64) * 1000)
    with IRMovie.from_filename(path) as mov:
        got = mov.to_tensor().cpu().view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(got, oracle(arr, 7, rows=h - 3))


# Rate floors over 1 000 frames of 640x512 (uint16): about 0.7 of what tests/perf/temporal_median_time.py measured when the filter was added,
# on one MI355X: window 5 at 3.82 M frames/s, window 15 at 3.22 M.
FLOOR_W5 = 2.6e6
FLOOR_W15 = 2.2e6


@pytest.mark.perf
@pytest.mark.parametrize("window,floor", [(5, FLOOR_W5), (15, FLOOR_W15)])
def test_rate_floor(window, floor):
    from librir_amd import device as D

    n = 1000
    src = torch.randint(0, 65536, (n, 512, 640), dtype=torch.int32, device="cuda").to(torch.int16).view(torch.uint16)
    out = torch.empty_like(src)
    for _ in range(3):
        D.temporal_median(src, window, out=out)
    torch.cuda.synchronize()
    reps = 20
    t0 = time.perf_counter()
    for _ in range(reps):
        D.temporal_median(src, window, out=out)
    torch.cuda.synchronize()
    rate = reps * n / (time.perf_counter() - t0)
    assert rate >= floor, "window %d: %.3g frames/s, floor %.3g" % (window, rate, floor)
