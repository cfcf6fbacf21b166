"""GPU: per-pixel quantiles over time, bit for bit against the oracle of test_pixel_quantiles_cpu.py - pixel tiles and tails, stack lengths
around the kernel's own periods (the waves that split the time axis, the flush of the 4-bit fields every 12 frames of a wave, the 15 frames a
field holds at most, the slabs of long thin stacks), every digit position, 0 and 65535, unaligned and sliced inputs, the cross-check with
region_quantiles, streaming in any split and order, reproducibility, stream order, refused arguments, the host entry and recordings read
through IRMovie.pixel_quantiles."""
import ctypes as ct

import numpy as np
import pytest

from test_gpu_region_stats import dev16, frames_of, record
from test_pixel_quantiles_cpu import DEV_ARGS, PUSH_ARGS, RESOLVE_ARGS, pixel_quantiles_oracle
from test_region_quantiles_cpu import PERCENTS

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

MEDIAN = (0.5,)
THREE = (0.05, 0.5, 0.95)
PERCENT_SETS = [MEDIAN, THREE, PERCENTS]  # one group of 1, one of 3, two of 4 percents per pass
SHAPES = [(1, 1), (3, 5), (17, 33), (64, 80)]
# 4, 8 (two to four percents) waves split the frames; a wave enters its main loop at 8 frames, flushes its 4-bit fields every 12 and ends
# on at most 15 unflushed ones: 8, 12 and 15 frames a wave are 32 / 48 / 60 frames for 4 waves and 64 / 96 / 120 for 8
LENGTHS = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 49, 59, 60, 61, 63, 64, 65, 95, 96, 97, 119, 120, 121, 257]


def check(got, exp, what=""):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    assert got.dtype == np.int32 and got.shape == exp.shape, (what, got.dtype, got.shape, exp.shape)
    if not np.array_equal(got, exp):
        bad = np.argwhere(got != exp)[:5]
        raise AssertionError("%s differs at %s: got %s, expected %s" % (what, bad.tolist(), got[tuple(bad.T)], exp[tuple(bad.T)]))


def check_sets(frames, what, sets=PERCENT_SETS):
    from librir_amd import device as D

    t = dev16(frames)
    for pc in sets:
        check(D.pixel_quantiles(t, pc), pixel_quantiles_oracle(frames, pc), (what, pc))


@pytest.fixture(scope="module")
def full_frame():
    """33 frames of 640x512, the device copy and the oracle's answers: shared, never written"""
    f = frames_of(33, 512, 640, seed=33)
    f[:, 100, 200] = 65535
    return f, dev16(f), {pc: pixel_quantiles_oracle(f, pc) for pc in (MEDIAN, THREE)}


@pytest.mark.parametrize("n", LENGTHS)
def test_lengths_on_small_shapes(n):
    for h, w in SHAPES:
        check_sets(frames_of(n, h, w, seed=n * 7 + w), (n, h, w))


def test_full_frame_tiles(full_frame):
    from librir_amd import device as D

    _, t, exp = full_frame
    for pc in (MEDIAN, THREE):
        check(D.pixel_quantiles(t, pc), exp[pc], ("640x512", pc))


def test_single_image_scalar_percent_and_no_frames():
    from librir_amd import device as D

    f = frames_of(1, 17, 33, seed=1)
    got = D.pixel_quantiles(dev16(f[0]), 0.5)
    assert tuple(got.shape) == (1, 17, 33)  # the leading axis is always there
    check(got, pixel_quantiles_oracle(f, 0.5))
    none = D.pixel_quantiles(dev16(f[:0]), THREE)
    assert tuple(none.shape) == (3, 17, 33) and bool((none == -1).all())


@pytest.mark.parametrize("shift", [0, 4, 8, 12])
def test_values_that_differ_in_one_digit(shift):
    rng = np.random.default_rng(shift)
    base = np.uint16(0x5A5A & ~(15 << shift))
    f = (rng.integers(0, 16, (64, 17, 33)).astype(np.uint16) << np.uint16(shift)) | base
    check_sets(f, ("digit", shift))


def test_constant_and_two_valued_stacks():
    check_sets(np.full((64, 17, 33), 21845, np.uint16), "constant")  # one bucket in every pass
    rng = np.random.default_rng(2)
    f = (rng.integers(0, 2, (65, 17, 33)) * 65535).astype(np.uint16)
    f[:, 3, 3] = 65535  # 65535 throughout: 0
    f[:, 4, 4] = 0
    exp = pixel_quantiles_oracle(f, PERCENTS)
    assert (exp[:, 3, 3] == 0).all() and set(np.unique(exp)) == {0}
    check_sets(f, "0 and 65535")
    g = frames_of(64, 17, 33, seed=8)
    g[:, 5, 5] = 65535
    g[:40, 6, 6] = 65535  # the upper quantiles fall on 65535, the lower ones do not
    exp = pixel_quantiles_oracle(g, PERCENTS)
    assert exp[-1, 6, 6] == 0 and exp[2, 6, 6] > 0  # p = 1 and p = 0.25
    check_sets(g, "full range")


@pytest.mark.parametrize("n", [513, 1025, 70001])
def test_long_thin_stacks_are_split_along_time(n):
    """more than one slab of frames per tile: the counts of the slabs are added with atomics; 70 001 crosses every 16-bit bound"""
    h, w = 3, 5
    check_sets(np.full((n, h, w), 21845, np.uint16), ("thin constant", n), [MEDIAN, PERCENTS])
    f = frames_of(n, h, w, seed=n)
    f[:, 0, 1] = np.arange(n) % 65536  # every value once (and some twice)
    check_sets(f, ("thin", n))


def test_sliced_and_unaligned_inputs():
    from librir_amd import device as D

    for n, h, w in [(5, 17, 33), (20, 16, 24), (2, 1, 1)]:
        f = frames_of(n + 1, h, w, seed=w)
        flat = dev16(f.reshape(-1))
        fr = flat[1:1 + n * h * w].view(n, h, w)  # the base is one pixel off: the pixel-by-pixel path
        assert fr.data_ptr() % 16 == 2
        exp = f.reshape(-1)[1:1 + n * h * w].reshape(n, h, w)
        for pc in PERCENT_SETS:
            check(D.pixel_quantiles(fr, pc), pixel_quantiles_oracle(exp, pc), ("offset", n, h, w, pc))
        t = dev16(f)
        if w > 1:
            check(D.pixel_quantiles(t[:, :, 1:], THREE), pixel_quantiles_oracle(f[:, :, 1:], THREE), ("columns", n, h, w))  # made contiguous
        check(D.pixel_quantiles(t[::2], THREE), pixel_quantiles_oracle(f[::2], THREE), ("strided", n, h, w))
    f = frames_of(300, 21, 31, seed=4)  # odd frame size: every other frame starts 2 bytes off a 16-byte boundary
    check_sets(f, "odd frames")


def test_equals_region_quantiles_over_the_column_view():
    from librir_amd import device as D

    n, h, w = 64, 64, 80
    f = frames_of(n, h, w, seed=64)
    t = dev16(f)
    labels = torch.arange(h * w, dtype=torch.int32, device="cuda").repeat(n, 1)
    rq = D.region_quantiles(t.view(1, n, h * w), labels, PERCENTS, h * w)
    assert bool((rq.count == n).all())
    got = D.pixel_quantiles(t, PERCENTS)
    assert torch.equal(got, rq.values[0].t().reshape(len(PERCENTS), h, w))
    check(got, pixel_quantiles_oracle(f, PERCENTS))


def run_selector(sel, batches):
    for _ in range(sel.passes):
        for b in batches:
            sel.push(b)
        sel.next_pass()
    return sel.result()


@pytest.mark.parametrize("pc", PERCENT_SETS)
def test_streaming_equals_one_call(pc):
    from librir_amd import device as D

    n, h, w = 257, 17, 33
    f = frames_of(n, h, w, seed=257)
    t = dev16(f)
    whole = D.pixel_quantiles(t, pc)
    check(whole, pixel_quantiles_oracle(f, pc), "whole")
    batches = [t[:1], t[1:101], t[101:]]
    sel = D.PixelQuantileSelector(pc)
    assert sel.passes == 4
    assert torch.equal(run_selector(sel, batches), whole)
    assert torch.equal(run_selector(D.PixelQuantileSelector(pc, shape=(h, w)), batches[::-1]), whole)
    # another order in every pass, and an empty batch
    other = D.PixelQuantileSelector(pc)
    for k in range(other.passes):
        for b in (batches[k % 3:] + batches[:k % 3] + [t[:0]]):
            other.push(b)
        other.next_pass()
    assert torch.equal(other.result(), whole)
    # two selectors interleaved on one stream
    g = frames_of(40, h, w, seed=40)
    a, b = D.PixelQuantileSelector(pc), D.PixelQuantileSelector(pc)
    tg = dev16(g)
    for _ in range(a.passes):
        a.push(t[:100])
        b.push(tg[:13])
        a.push(t[100:])
        b.push(tg[13:])
        b.next_pass()
        a.next_pass()
    assert torch.equal(a.result(), whole)
    check(b.result(), pixel_quantiles_oracle(g, pc), "interleaved")
    # reset and reuse, also from the middle of a sequence
    sel.reset()
    check(run_selector(sel, [tg]), pixel_quantiles_oracle(g, pc), "after reset")
    sel.reset()
    sel.push(t)
    sel.next_pass()
    sel.push(t[:5])
    sel.reset()
    assert torch.equal(run_selector(sel, batches), whole)


def test_selector_misuse_and_empty_sequences():
    from librir_amd import device as D

    t = dev16(frames_of(10, 8, 8, seed=0))
    sel = D.PixelQuantileSelector(THREE)
    with pytest.raises(RuntimeError):
        sel.result()
    sel.push(t)
    with pytest.raises(RuntimeError):
        sel.push(dev16(frames_of(2, 8, 9, seed=0)))  # another size
    with pytest.raises(RuntimeError):
        sel.push(t.cpu())
    sel.next_pass()
    with pytest.raises(RuntimeError):
        sel.result()  # three passes to go
    sel.push(t[:9])
    with pytest.raises(RuntimeError, match="pass 0 saw 10"):
        sel.next_pass()
    sel.push(t[9:])
    sel.next_pass()
    for _ in range(2):
        sel.push(t)
        sel.next_pass()
    check(sel.result(), pixel_quantiles_oracle(t.cpu().numpy().view(np.uint16), THREE), "after a refused close")
    with pytest.raises(RuntimeError):
        sel.push(t)  # every pass is closed
    with pytest.raises(RuntimeError):
        sel.next_pass()
    with pytest.raises(RuntimeError):
        D.PixelQuantileSelector(0.5, shape=(8, 9)).push(t)
    with pytest.raises(RuntimeError, match="cuda:1"):
        D.PixelQuantileSelector(0.5, device="cuda:1").push(t)  # the first batch already: not the device asked for
    D.PixelQuantileSelector(0.5, device="cuda").push(t)
    D.PixelQuantileSelector(0.5, device=t.device).push(t)
    known = D.PixelQuantileSelector(THREE, shape=(5, 7))
    for _ in range(known.passes):
        known.next_pass()
    got = known.result()
    assert tuple(got.shape) == (3, 5, 7) and got.dtype == torch.int32 and bool((got == -1).all())
    unknown = D.PixelQuantileSelector(THREE)
    for _ in range(unknown.passes):
        unknown.next_pass()
    assert tuple(unknown.result().shape) == (3, 0, 0)


def test_two_runs_give_equal_bytes(full_frame):
    from librir_amd import device as D

    _, t, exp = full_frame
    a, b = D.pixel_quantiles(t, THREE), D.pixel_quantiles(t, THREE)
    assert torch.equal(a, b)
    check(a, exp[THREE])
    thin = dev16(frames_of(3000, 8, 8, seed=6))  # the form with slabs and atomic adds
    assert torch.equal(D.pixel_quantiles(thin, PERCENTS), D.pixel_quantiles(thin, PERCENTS))


def test_queued_behind_the_kernel_that_writes_the_frames(full_frame):
    """the frames are written by kernels on a side stream and selected from on that stream at once"""
    from librir_amd import device as D

    f, _, exp = full_frame
    host = torch.from_numpy(f.view(np.int16)).pin_memory()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        src = torch.empty(f.shape, dtype=torch.int16, device="cuda")
        src.copy_(host, non_blocking=True)
        src.add_(0)
        got = D.pixel_quantiles(src.view(torch.uint16), MEDIAN)
    side.synchronize()
    check(got, exp[MEDIAN])


def test_refused_arguments(lib):
    from librir_amd import device as D
    from librir_amd.low_level.misc import last_error

    n, h, w, q = 6, 8, 8, 2
    f = dev16(frames_of(n, h, w, seed=0))
    with pytest.raises(RuntimeError):
        D.pixel_quantiles(f.view(torch.int16), 0.5)
    with pytest.raises(RuntimeError):
        D.pixel_quantiles(f.cpu(), 0.5)
    with pytest.raises(ValueError):
        D.pixel_quantiles(f, 1.5)
    one, push, resolve = lib.rir_pixel_quantiles_device, lib.rir_pixel_quantiles_push_device, lib.rir_pixel_quantiles_resolve_device
    one.argtypes, push.argtypes, resolve.argtypes = DEV_ARGS, PUSH_ARGS, RESOLVE_ARGS
    lib.rir_pixel_quantiles_state_bytes.argtypes = [ct.c_int] * 3
    lib.rir_pixel_quantiles_state_bytes.restype = ct.c_size_t
    sb = lib.rir_pixel_quantiles_state_bytes(w, h, q)
    passes = lib.rir_pixel_quantiles_passes()
    assert sb == 72 * q * h * w
    pc = np.array([0.25, 0.5], np.float32)
    nan = np.array([0.25, np.nan], np.float32)
    buf = torch.full((4096,), 7, dtype=torch.int64, device="cuda")
    values, state = buf.data_ptr(), buf.data_ptr() + 8192
    before = buf.clone()
    fp = f.data_ptr()

    assert one(fp, w, h, n, pc.ctypes.data, q, fp + 64, state, sb, None) == -1 and "overlap" in last_error()  # the values in the frames
    assert one(fp, w, h, n, pc.ctypes.data, q, values, fp, sb, None) == -1 and "overlap" in last_error()
    assert one(fp, w, h, n, pc.ctypes.data, q, state + 8, state, sb, None) == -1 and "overlap" in last_error()
    assert one(fp, w, h, n, pc.ctypes.data, q, values, state, sb - 1, None) == -1 and "workspace" in last_error()
    assert one(fp, w, h, n, pc.ctypes.data, q, values, state + 4, sb, None) == -1  # not 8-byte aligned
    for nulls in ((None, pc.ctypes.data, values, state), (fp, None, values, state), (fp, pc.ctypes.data, None, state), (fp, pc.ctypes.data, values, None)):
        assert one(nulls[0], w, h, n, nulls[1], q, nulls[2], nulls[3], sb, None) == -1 and "null" in last_error()
    assert one(fp, w, h, n, nan.ctypes.data, q, values, state, sb, None) == -1 and "percent" in last_error()
    for bad in (dict(w=0), dict(h=-1), dict(n=-1), dict(q=0), dict(q=9)):
        a = dict(dict(w=w, h=h, n=n, q=q), **bad)
        assert one(fp, a["w"], a["h"], a["n"], pc.ctypes.data, a["q"], values, state, sb, None) == -1, bad
    assert push(fp, w, h, n, q, passes, state, sb, None) == -1 and "pass" in last_error()
    assert push(fp, w, h, n, q, -1, state, sb, None) == -1
    assert push(fp, w, h, n, q, 0, state, sb - 1, None) == -1 and "state" in last_error()
    assert push(fp, w, h, n, q, 0, fp, sb, None) == -1 and "overlap" in last_error()
    assert push(None, w, h, n, q, 0, state, sb, None) == -1 and push(fp, w, h, n, q, 0, None, sb, None) == -1
    assert push(fp, w, h, -1, q, 0, state, sb, None) == -1
    assert push(fp, w, h, 0, q, 0, state, sb, None) == 0  # no frames: nothing is done
    assert resolve(w, h, pc.ctypes.data, q, passes, n, state, sb, values, None) == -1 and "pass" in last_error()
    assert resolve(w, h, pc.ctypes.data, q, passes - 1, n, state, sb, None, None) == -1 and "null" in last_error()
    assert resolve(w, h, pc.ctypes.data, q, passes - 1, n, state, sb, state + 16, None) == -1 and "overlap" in last_error()
    assert resolve(w, h, pc.ctypes.data, q, 0, n, state, sb - 1, None, None) == -1 and "state" in last_error()
    assert resolve(w, h, pc.ctypes.data, q, 0, -1, state, sb, None, None) == -1
    assert resolve(w, h, pc.ctypes.data, q, 0, 1 << 31, state, sb, None, None) == -1
    assert resolve(w, h, nan.ctypes.data, q, 0, n, state, sb, None, None) == -1 and "percent" in last_error()
    assert resolve(w, h, None, q, 0, n, state, sb, None, None) == -1 and resolve(w, h, pc.ctypes.data, q, 0, n, None, sb, None, None) == -1
    torch.cuda.synchronize()
    assert torch.equal(buf, before)  # nothing was written by a refused call

    # the same buffers, accepted: the one-call form, the streamed form on a zeroed state, and no frames at all
    exp = pixel_quantiles_oracle(f.cpu().numpy().view(np.uint16), pc)
    assert one(fp, w, h, n, pc.ctypes.data, q, values, state, sb, None) == 0
    torch.cuda.synchronize()
    check(buf[:q * h * w // 2].view(torch.int32).view(q, h, w), exp, "one call")
    buf.fill_(0)
    for k in range(passes):
        assert push(fp, w, h, 4, q, k, state, sb, None) == 0 and push(fp + 4 * h * w * 2, w, h, n - 4, q, k, state, sb, None) == 0
        assert resolve(w, h, pc.ctypes.data, q, k, n, state, sb, None if k < passes - 1 else values, None) == 0
    torch.cuda.synchronize()
    check(buf[:q * h * w // 2].view(torch.int32).view(q, h, w), exp, "streamed")
    buf.fill_(0)
    assert one(None, w, h, 0, pc.ctypes.data, q, values, state, sb, None) == 0
    torch.cuda.synchronize()
    assert bool((buf[:q * h * w // 2].view(torch.int32) == -1).all()) and not bool(buf[q * h * w // 2:].any())
    buf.fill_(0)
    for k in range(passes):
        assert resolve(w, h, pc.ctypes.data, q, k, 0, state, sb, values, None) == 0
    torch.cuda.synchronize()
    assert bool((buf[:q * h * w // 2].view(torch.int32) == -1).all())


def test_host_entry():
    from librir_amd import signal_processing as S

    f = frames_of(257, 17, 33, seed=17)
    for pc in PERCENT_SETS:
        check(S.pixel_quantiles(f, pc), pixel_quantiles_oracle(f, pc), ("host", pc))
    check(S.pixel_quantiles(f[0], 0.5), pixel_quantiles_oracle(f[:1], 0.5), "one image")
    none = S.pixel_quantiles(np.zeros((0, 4, 5), np.uint16), THREE)
    assert none.shape == (3, 4, 5) and none.dtype == np.int32 and (none == -1).all()


def test_host_entry_streams_a_stack_above_the_resident_limit():
    """more than 256 MiB of frames: slabs of 64 MiB, once per pass - the bits of the device entry over the resident stack"""
    from librir_amd import device as D
    from librir_amd import signal_processing as S

    n, h, w = 420, 512, 640
    f = np.random.default_rng(420).integers(0, 65536, (n, h, w), dtype=np.uint16)
    assert f.nbytes > 256 << 20
    got = S.pixel_quantiles(f, THREE)
    assert np.array_equal(got, D.pixel_quantiles(dev16(f), THREE).cpu().numpy())
    assert np.array_equal(got[1, :2], pixel_quantiles_oracle(f[:, :2], 0.5)[0])


@pytest.mark.parametrize("bad_pixels", [False, True])
def test_movie_pixel_quantiles(tmp_path, monkeypatch, bad_pixels):
    from librir_amd.synthetic import inject_bad_pixels, s1_noisy_background
    from librir_amd.video_io import IRMovie

    n, h, w = 40, 64, 80
    arr = inject_bad_pixels(s1_noisy_background(n, h, w, seed=12), 7)
    with IRMovie.from_filename(record(tmp_path / "m.h264", arr)) as mov:
        mov.bad_pixels_correction = bad_pixels
        resident = {}
        for sel in (slice(None), slice(2, 38, 3), 5):
            images = np.asarray(mov[sel]).reshape(-1, h, w)
            resident[str(sel)] = got = mov.pixel_quantiles(THREE, sel)
            check(got, pixel_quantiles_oracle(images, THREE), ("resident", sel))
        median = mov.pixel_quantiles(0.5)
        assert tuple(median.shape) == (1, h, w) and torch.equal(median[0], resident[str(slice(None))][1])
        tracks, _ = mov.track_hot_spots(median[0] + 50, stats=False)  # a per-pixel threshold from the median image
        assert tuple(tracks.tracks.shape) == (n, h, w)
        # the same selections streamed: four passes over pieces of 7 images
        monkeypatch.setattr(IRMovie, "_QUANTILE_RESIDENT_BYTES", 0)
        monkeypatch.setattr(IRMovie, "_STATS_PIECE_BYTES", 7 * h * w * 2)
        for sel in (slice(None), slice(2, 38, 3), 5):
            assert torch.equal(mov.pixel_quantiles(THREE, sel), resident[str(sel)]), sel
        with pytest.raises(ValueError):
            mov.pixel_quantiles(0.5, slice(None, None, -1))
        with pytest.raises(IndexError):
            mov.pixel_quantiles(0.5, n)
        with pytest.raises(ValueError):
            mov.pixel_quantiles(1.5)
