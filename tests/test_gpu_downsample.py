"""GPU: adaptive temporal downsampling (max-hold), bit for bit against the oracle of downsample_cases.py (which test_downsample_cpu.py pins to
a second restatement): images, positions, time stamps and statistics - shapes with ragged sizes and 16-byte loads across the lossy_height
boundary, stack lengths around the time-slab cut, the 16-bit range and ties, any split into pushes, refused calls, stream order, and the
routes through IRSaver.add_images and IRMovie.to_h264."""
import ctypes as ct
import functools

import numpy as np
import pytest

import downsample_cases as DC
from test_gpu_region_stats import dev16

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

CUT = 64  # frames a workgroup of the pair sums walks (DS_SLAB, downsample_kernels.h): longer stacks are cut along time
SHAPES = [(1, 2), (3, 5), (17, 33), (40, 130), (40, 132), (512, 640)]
GEOMETRIES = [(h, w, lossy) for h, w in SHAPES for lossy in ([h, h - 3] if h > 3 else [h])]


@functools.lru_cache(maxsize=None)
def scene(h, w):
    f = DC.scene(130 if h * w > 100000 else DC.FRAMES, h, w, seed=h + w)
    f.setflags(write=False)
    return f


def run(frames, stamps, factor, factor_std, lossy, method, cuts=(), dev=None):
    """the sequence through one Downsampler, pushed in the pieces `cuts` delimit -> (Result, count)"""
    from librir_amd import device as D

    n, h, w = frames.shape
    fr = dev16(frames) if dev is None else dev
    d = D.Downsampler(w, h, factor, factor_std, lossy, method)
    images, positions, times, stats = [], [], [], []
    edges = [0] + list(cuts) + [n]
    for a, b in zip(edges[:-1], edges[1:]):
        got = d.push(fr[a:b], stamps[a:b])
        assert got.frames.dtype == torch.uint16 and tuple(got.frames.shape) == (len(got.positions), h, w)
        assert got.positions.dtype == np.int32 and got.stats.shape == (b - a,) and got.timestamps.dtype == np.int64
        images.append(got.frames.cpu().numpy())
        positions.append(got.positions + a)
        times.append(got.timestamps)
        stats.append(got.stats)
    count = d.count
    assert d.close() == count and d.count == 0
    return DC.Result(np.concatenate(images), np.concatenate(positions).astype(np.int32), np.concatenate(times), np.concatenate(stats), None, None), count


def check(frames, factor, factor_std, lossy, method, cuts=(), what=""):
    stamps = DC.stamps(len(frames))
    exp = DC.oracle(frames, stamps, factor, factor_std, lossy, method)
    got, count = run(frames, stamps, factor, factor_std, lossy, method, cuts)
    DC.same(got, exp, what)
    assert count == len(exp.positions)
    return exp


@pytest.mark.parametrize("method", DC.METHODS)
@pytest.mark.parametrize("h,w,lossy", GEOMETRIES)
def test_scenes_at_every_shape(h, w, lossy, method):
    f = scene(h, w)
    exp = check(f, 10, .9, lossy, method, what=(h, w, lossy, method))
    if h >= 12:
        assert (exp.positions % 10 != 0).any()  # an event was kept off the grid


@pytest.mark.parametrize("method", DC.METHODS)
@pytest.mark.parametrize("factor,factor_std", DC.PARAMS)
def test_parameter_sets(factor, factor_std, method):
    check(scene(40, 132), factor, factor_std, 37, method, what=(factor, factor_std, method))


@pytest.mark.parametrize("h,w,lossy", [(40, 132, 37), (17, 33, 14)])
@pytest.mark.parametrize("n", [1, 2, 7, 8, 9, 15, 16, 17, CUT - 1, CUT, CUT + 1, 2 * CUT - 1, 2 * CUT, 2 * CUT + 1])  # (7 .. 17: the walk's sets of 4 + 4 frames)
def test_lengths_around_the_time_slab_cut(n, h, w, lossy):
    f = scene(h, w)
    check(f[:n], 4, .75, lossy, 2, what=("whole", n))
    check(f[:n + 3], 4, .75, lossy, 1, cuts=[3], what=("after a push of three", n))  # (the carried image ahead of the first slab)


def value_stacks(h, w):
    rng = np.random.default_rng(h * w)
    n = 150
    full = rng.integers(0, 65536, (n, h, w), dtype=np.uint16)
    flip = np.zeros((n, h, w), np.uint16)
    flip[1::2] = 65535  # the largest sums: every d is 65535
    flip[70:, 1, 1] = 77  # (a pixel that stays, so that the statistic is not 0 everywhere)
    four = rng.integers(0, 4, (n, h, w)).astype(np.uint16) * np.uint16(21845)  # ties in the maximum
    return {"full": full, "flip": flip, "four": four}


@pytest.mark.parametrize("kind", ["full", "flip", "four"])
@pytest.mark.parametrize("h,w,lossy", [(40, 132, 37), (17, 33, 17), (40, 130, 40)])
def test_the_16_bit_range_and_ties(h, w, lossy, kind):
    f = value_stacks(h, w)[kind]
    for method in DC.METHODS:
        check(f, 5, .5, lossy, method, what=(kind, method))
        check(f, 5, .5, lossy, method, cuts=[1, 64, 65, 149], what=(kind, method, "cut"))


@pytest.mark.parametrize("method", DC.METHODS)
@pytest.mark.parametrize("h,w,lossy", [(40, 130, 37), (40, 132, 40), (3, 5, 3)])
def test_any_split_into_pushes_gives_one_push(h, w, lossy, method):
    f = scene(h, w)
    n = len(f)
    rng = np.random.default_rng(n + method)
    for k in (1, 4, 17):
        cuts = sorted(rng.choice(np.arange(1, n), k, replace=False).tolist())
        check(f, 10, .9, lossy, method, cuts=cuts, what=("cuts", cuts))
    check(f[:140], 10, .9, lossy, method, cuts=list(range(1, 140)), what="one frame a push")


def test_rows_below_lossy_height_and_the_carried_maximum():
    """a flash in a push that keeps nothing is in the image the next push keeps; the rows that are not held are the keeping frame's"""
    from librir_amd import device as D

    h, w, lossy = 8, 16, 5
    f = np.full((8, h, w), 100, np.uint16)
    f += np.arange(8, dtype=np.uint16)[:, None, None]  # frame i holds 100 + i
    f[5, 1, 2] = 9000  # a flash above the boundary row, in the second push
    f[5, 6, 3] = 8000  # and one below it: not held
    d = D.Downsampler(w, h, 4, .5, lossy, 1)
    a = d.push(dev16(f[:4]), DC.stamps(8)[:4])
    b = d.push(dev16(f[4:7]), DC.stamps(8)[4:7])  # image 4 is kept; 5 and 6 are carried
    c = d.push(dev16(f[7:]), DC.stamps(8)[7:])
    assert a.positions.tolist() == [0] and b.positions.tolist() == [0] and c.positions.tolist() == []
    e = d.push(dev16(f[:1] + 1), [DC.stamps(9)[8]])  # image 8: kept, and the flash of image 5 with it
    assert e.positions.tolist() == [0] and d.count == 3
    img = e.frames.cpu().numpy()[0]
    exp = np.full((h, w), 107, np.uint16)
    exp[1, 2] = 9000
    exp[lossy:] = 101
    assert np.array_equal(img, exp)
    d.close()


def test_refused_calls_leave_the_state_untouched(lib):
    from librir_amd import device as D
    from librir_amd.low_level.misc import last_error

    h, w, lossy = 40, 132, 37
    f = scene(h, w)
    stamps = DC.stamps(len(f))
    exp = DC.oracle(f, stamps, 4, .75, lossy, 2)
    fr = dev16(f)
    d = D.Downsampler(w, h, 4, .75, lossy, 2)
    first = d.push(fr[:100], stamps[:100])
    lib.rir_downsampler_push_device.argtypes = [ct.c_int, ct.c_void_p, ct.c_int, ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_void_p]
    pos = np.zeros(160, np.int32)
    st = ct.c_void_p(torch.cuda.current_stream().cuda_stream)
    piece = fr[100:]
    ts = np.ascontiguousarray(stamps[100:])
    # the output over the frames, and one image into them
    for out in (piece.data_ptr(), piece.data_ptr() + (len(piece) - 1) * h * w * 2, piece.data_ptr() - h * w * 2):
        assert lib.rir_downsampler_push_device(d.handle, piece.data_ptr(), len(piece), ts.ctypes.data, out, pos.ctypes.data, None, st) == -1
        assert "overlaps" in last_error()
    out = torch.empty_like(piece)
    for bad in (ts[::-1].copy(), np.concatenate([ts[:5], ts[4:-1]]), ts - ts[0] + stamps[99], ts - ts[0]):
        assert lib.rir_downsampler_push_device(d.handle, piece.data_ptr(), len(piece), bad.ctypes.data, out.data_ptr(), pos.ctypes.data, None, st) == -1
        assert "time stamps" in last_error()
    with pytest.raises(ValueError):
        d.push(piece, ts[::-1].copy())
    assert lib.rir_downsampler_push_device(d.handle, None, 3, ts.ctypes.data, out.data_ptr(), pos.ctypes.data, None, st) == -1
    assert lib.rir_downsampler_push_device(d.handle, piece.data_ptr(), -1, ts.ctypes.data, out.data_ptr(), pos.ctypes.data, None, st) == -1
    assert lib.rir_downsampler_push_device(d.handle, None, 0, None, None, None, None, st) == 0
    assert d.count == len(first.positions) and not pos.any()
    second = d.push(piece, ts, out=out)
    assert second.frames.data_ptr() == out.data_ptr()
    got = DC.Result(np.concatenate([first.frames.cpu().numpy(), second.frames.cpu().numpy()]), np.concatenate([first.positions, second.positions + 100]),
                    np.concatenate([first.timestamps, second.timestamps]), np.concatenate([first.stats, second.stats]), None, None)
    DC.same(got, exp)
    assert d.close() == len(exp.positions)
    with pytest.raises(RuntimeError):
        D.Downsampler(w, h, 4, .75, lossy, 2).push(fr[:, :-1], stamps)


def test_factor_one_and_the_one_shot_form():
    from librir_amd import device as D

    f = scene(17, 33)[:40]
    stamps = DC.stamps(40)
    got = D.downsample(dev16(f), stamps, 1, .5, 14, 2)
    DC.same(DC.Result(got.frames.cpu().numpy(), got.positions, got.timestamps, got.stats, None, None), DC.oracle(f, stamps, 1, .5, 14, 2))
    got = D.downsample(dev16(f), stamps, 3, .5, method=2)
    DC.same(DC.Result(got.frames.cpu().numpy(), got.positions, got.timestamps, got.stats, None, None), DC.oracle(f, stamps, 3, .5, 17, 2))
    empty = D.downsample(dev16(f[:0]), stamps[:0], 3, .5)
    assert tuple(empty.frames.shape) == (0, 17, 33) and len(empty.positions) == 0 and len(empty.stats) == 0


def test_stream_order_and_reproducibility():
    """a push queued behind the kernel that writes its frames sees them; two runs give the same bytes"""
    from librir_amd import device as D

    h, w = 512, 640
    f = scene(h, w)
    stamps = DC.stamps(len(f))
    exp = DC.oracle(f, stamps, 10, .9, h - 3, 1)
    src = dev16(f).view(torch.int16)
    side = torch.cuda.Stream()
    runs = []
    for _ in range(2):
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fr = torch.zeros_like(src)
            for _ in range(3):
                fr = fr + src - fr  # (kernels that write the frames, queued right before the push)
            got = D.downsample(fr.view(torch.uint16), stamps, 10, .9, h - 3, 1)
            runs.append(DC.Result(got.frames.cpu().numpy(), got.positions, got.timestamps, got.stats, None, None))
        torch.cuda.current_stream().wait_stream(side)
    DC.same(runs[0], exp)
    DC.same(runs[1], runs[0])


def test_saver_records_the_kept_images(tmp_path):
    from librir_amd import device as D
    from librir_amd.video_io import IRMovie, IRSaver

    h, w, lossy = 40, 132, 37
    f = scene(h, w)
    stamps = DC.stamps(len(f))
    exp = DC.oracle(f, stamps, 10, .9, lossy, 2)
    fr = dev16(f)
    paths = [str(tmp_path / name) for name in ("thin.h264", "kept.h264", "all.h264", "all_none.h264")]
    with IRSaver(paths[0], w, h, lossy) as s:
        d = D.Downsampler(w, h, 10, .9, lossy, 2)
        assert s.add_images(fr[:100], stamps[:100], downsampler=d) + s.add_images(fr[100:], stamps[100:], downsampler=d) == len(exp.positions)
        with pytest.raises(RuntimeError):
            s.add_images(fr, stamps, downsampler=D.Downsampler(w, h, 10, .9, h, 2))  # not the saver's lossy_height
        assert d.close() == len(exp.positions)
    with IRSaver(paths[1], w, h, lossy) as s:
        s.add_images(dev16(exp.images), exp.timestamps)
    with IRSaver(paths[2], w, h, lossy) as s:
        assert s.add_images(fr, stamps) is None
    with IRSaver(paths[3], w, h, lossy) as s:
        s.add_images(fr, stamps, downsampler=None)
    assert open(paths[0], "rb").read() == open(paths[1], "rb").read()
    assert open(paths[2], "rb").read() == open(paths[3], "rb").read()
    with IRMovie.from_filename(paths[0]) as mov:
        assert mov.images == len(exp.positions)
        assert np.array_equal(mov.data, exp.images)
        assert np.array_equal(np.round(np.asarray(mov.timestamps) * 1e9).astype(np.int64), exp.timestamps)


@pytest.mark.parametrize("spec", [(4, .75), (4, .75, 2), (1, .5)])
def test_movie_is_recorded_again_downsampled(tmp_path, spec):
    from librir_amd.video_io import IRMovie, IRSaver

    h, w = 33, 70
    f = DC.scene(150, h, w, seed=3)
    stamps = DC.stamps(150)
    src = str(tmp_path / "src.h264")
    with IRSaver(src, w, h, h) as s:
        for i in range(150):
            s.add_image(f[i], int(stamps[i]), attributes={"pos": str(i), "odd": "y" if i & 1 else "n"})
    exp = DC.oracle(f, stamps, spec[0], spec[1], h, spec[2] if len(spec) == 3 else 1)
    with IRMovie.from_filename(src) as mov:
        mov._STATS_PIECE_BYTES = 37 * h * w * 2  # (several pieces)
        times = np.asarray(mov.timestamps)
        mov.to_h264(str(tmp_path / "thin.h264"), downsample=spec)
        mov.to_h264(str(tmp_path / "part.h264"), start_img=20, count=100, downsample=spec)
        mov.to_h264(str(tmp_path / "plain.h264"))
        mov.to_h264(str(tmp_path / "plain_none.h264"), downsample=None)
        with pytest.raises(ValueError):
            mov.to_h264(str(tmp_path / "bad.h264"), downsample=(4,))
    with IRMovie.from_filename(str(tmp_path / "thin.h264")) as thin:
        assert thin.images == len(exp.positions)
        assert np.array_equal(thin.data, exp.images)
        assert np.abs(np.asarray(thin.timestamps) - times[exp.positions]).max() < 2e-9  # (seconds and back: within the last nanosecond)
        for k, at in enumerate(exp.positions):
            thin.load_pos(k)
            assert thin.frame_attributes == {"pos": str(at).encode(), "odd": b"y" if at & 1 else b"n"}
    part = DC.oracle(f[20:120], stamps[20:120], spec[0], spec[1], h, spec[2] if len(spec) == 3 else 1)
    with IRMovie.from_filename(str(tmp_path / "part.h264")) as thin:
        assert np.array_equal(thin.data, part.images) and np.abs(np.asarray(thin.timestamps) - times[20:120][part.positions]).max() < 2e-9
        thin.load_pos(1)
        assert thin.frame_attributes["pos"] == str(20 + part.positions[1]).encode()
    with IRMovie.from_filename(str(tmp_path / "plain.h264")) as a, IRMovie.from_filename(str(tmp_path / "plain_none.h264")) as b:
        assert np.array_equal(a.data, f) and np.array_equal(b.data, f) and np.array_equal(np.asarray(a.timestamps), np.asarray(b.timestamps))
    assert open(str(tmp_path / "plain.h264"), "rb").read() == open(str(tmp_path / "plain_none.h264"), "rb").read()
