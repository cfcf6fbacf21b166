"""GPU: recordings read into device tensors (IRMovie.to_tensor, rir_load_images_device) and recorded from them (IRSaver.add_images,
rir_add_images_device) - parity with the image-by-image host calls, the camera's read state left alone, failures, stream order."""
import hashlib
import os
import time

import numpy as np
import pytest

from librir_amd.synthetic import inject_bad_pixels, s1_noisy_background
from librir_amd.video_io import IRMovie, IRSaver
from librir_amd.video_io import rir_video_io as rv

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def record(path, frames, gop=None, times=None):
    n, h, w = frames.shape
    times = np.arange(n, dtype=np.int64) * 20000000 + 7 if times is None else times
    with IRSaver(path, w, h, h) as s:
        if gop:
            s.set_parameter("GOP", gop)
        for i in range(n):
            s.add_image(frames[i], int(times[i]))
    return path


def host_stack(mov, positions):
    h, w = mov.image_size
    return np.stack([mov.load_pos(p) for p in positions]) if len(positions) else np.empty((0, h, w), np.uint16)


def check_selections(mov, sels):
    """to_tensor(sel) against load_pos image by image, uint16 and float32"""
    n = mov.images
    for sel in sels:
        positions = [sel + (n if sel < 0 else 0)] if isinstance(sel, int) else list(range(n))[sel]
        exp = host_stack(mov, positions)
        got = mov.to_tensor(sel)
        assert got.is_cuda and got.dtype == torch.uint16 and tuple(got.shape) == exp.shape, sel
        assert torch.equal(got.cpu(), torch.from_numpy(exp.astype(np.int32)).to(torch.uint16)), sel
        gf = mov.to_tensor(sel, dtype=torch.float32)
        assert gf.dtype == torch.float32 and torch.equal(gf, got.float()), sel


SELECTIONS = [slice(None), slice(3, 17), slice(6, 7), 5, -1, slice(1, None, 3), slice(2, 40, 7), slice(0, None, 13), slice(-9, -2), slice(-20, None, 3),
              slice(8, 8), slice(30, 10)]


@pytest.mark.parametrize("h,w,gop", [(67, 83, None), (67, 83, 4), (64, 96, 5), (48, 1024, 6)])
def test_read_parity_rirb(tmp_path, h, w, gop):
    """ragged frames (tiles cut by the frame's end), the default GOP and small ones, a short last chunk"""
    n = 43
    arr = s1_noisy_background(n, h, w, seed=3)
    with IRMovie.from_filename(record(tmp_path / "m.h264", arr, gop)) as mov:
        assert torch.equal(mov.to_tensor().cpu(), torch.from_numpy(arr.astype(np.int32)).to(torch.uint16))
        check_selections(mov, SELECTIONS)


def test_read_parity_with_filters_and_state(tmp_path):
    """bad pixels, motion correction and both, as load_pos gives them; the camera's current image is not disturbed"""
    n, h, w = 26, 67, 83
    arr = inject_bad_pixels(s1_noisy_background(n, h, w, seed=5), 9)
    reg = tmp_path / "reg.csv"
    rng = np.random.default_rng(2)
    with open(reg, "w") as f:
        f.write("frame\tx\ty\tconfidence\n")
        for i in range(n):
            f.write("%d\t%g\t%g\t1\n" % (i, float(rng.uniform(-4, 4)), float(rng.uniform(-4, 4))))
    with IRMovie.from_filename(record(tmp_path / "f.h264", arr, 4)) as mov:
        mov.registration_file = reg
        for bp, motion in ((True, False), (False, True), (True, True)):
            mov.bad_pixels_correction = bp
            mov.registration = motion
            check_selections(mov, [slice(None), slice(3, 19, 3), 7, slice(-5, None)])
        # state: after load_pos(k), to_tensor of another range leaves image k current
        k = 9
        img = mov.load_pos(k)
        attrs = dict(mov.frame_attributes)
        x, y = 11, 20
        raw = rv.get_last_image_raw_value(mov.handle, x, y)
        mov.to_tensor(slice(14, 25, 2))
        assert rv.get_last_image_raw_value(mov.handle, x, y) == raw == arr[k, y, x]
        assert rv.get_attributes(mov.handle) == attrs
        assert np.array_equal(mov.load_pos(k), img)


def test_read_parity_subtract_min(tmp_path):
    """a bounded-loss recording with subtractMin: MIN_T is added back on the first MIN_T_HEIGHT rows, as load_pos does"""
    n, h, w, hl = 23, 64, 80, 61
    arr = s1_noisy_background(n, h, w, seed=11)
    dst = tmp_path / "lossy.h264"
    with IRSaver(dst, w, h, hl) as s:
        s.set_parameter("subtractMin", 1)
        s.set_parameter("GOP", 5)
        for i in range(n):
            s.add_image_lossy(arr[i], i * 1000)
    with IRMovie.from_filename(dst) as mov:
        assert int(mov.attributes["MIN_T"]) > 0
        check_selections(mov, [slice(None), slice(2, 21, 4), 6])


@pytest.mark.parametrize("kind", ["pcr", "bin", "zfile"])
def test_read_parity_raw_and_zfile(tmp_path, kind):
    from librir_amd.video_io.IRMovie import create_pcr_header

    n, h, w = 17, 40, 72
    arr = inject_bad_pixels(s1_noisy_background(n, h, w, seed=8), 5)
    p = tmp_path / ("m." + kind)
    if kind == "pcr":
        with open(p, "wb") as f:
            f.write(create_pcr_header(h, w, 50).astype(np.uint32).tobytes())
            f.write(arr.tobytes())
    elif kind == "bin":
        import struct

        zh = bytes([1, 1, 0]) + b"\0" * 125  # version, one trigger, compression 0: raw frames behind the two blocks
        zt = struct.pack("<11Q", 0, 50, n, 0, 0, 1, 0, 0, 0, w, h)  # date, rate, samples, ..., data_size_x, data_size_y
        zt = zt + b"\0" * (128 - len(zt))
        p.write_bytes(zh + zt + arr.tobytes())
    else:
        wr = rv.open_video_write(p, w, h, 50, 1, 3)
        for i in range(n):
            rv.image_write(wr, arr[i], i * 1000)
        rv.close_video(wr)
    with IRMovie.from_filename(p) as mov:
        assert mov.images == n and np.array_equal(mov[3], arr[3])
        check_selections(mov, [slice(None), slice(2, 15, 3), -2, slice(5, 5)])
        mov.bad_pixels_correction = True
        check_selections(mov, [slice(None), slice(1, 16, 5)])


def test_failures_are_refused_and_leave_the_movie_readable(tmp_path):
    import struct

    n, h, w, gop = 12, 32, 64, 4
    arr = s1_noisy_background(n, h, w, seed=4)
    src = record(tmp_path / "ok.h264", arr, gop)
    blob = bytearray(open(src, "rb").read())
    # chunk 1 (behind chunk 0): its first record header gets mode 3, which no record has
    index_offset = struct.unpack_from("<Q", blob, 32 + 32)[0]  # (ftyp box, then the file header: DESIGN.md §4)
    c1 = struct.unpack_from("<Q", blob, index_offset + 24)[0]  # index entry 1: its chunk's offset
    assert blob[c1:c1 + 4] == b"CHNK"
    blob[c1 + 32 + 1] |= 0xC0
    bad = tmp_path / "bad.h264"
    bad.write_bytes(bytes(blob))
    with IRMovie.from_filename(bad) as mov:
        with pytest.raises(RuntimeError):
            mov.load_pos(5)
        with pytest.raises(RuntimeError):
            mov.to_tensor()
        assert torch.equal(mov.to_tensor(slice(0, gop)).cpu(), torch.from_numpy(arr[:gop].astype(np.int32)).to(torch.uint16))
        assert np.array_equal(mov.load_pos(2), arr[2]) and np.array_equal(mov.load_pos(9), arr[9])
    with IRMovie.from_filename(src) as mov:
        guard = torch.full((n + 1, h, w), 0x5A5A, dtype=torch.int16, device="cuda").view(torch.uint16)
        with pytest.raises(RuntimeError):
            mov.to_tensor(out=torch.empty((n, h, w), dtype=torch.uint16))  # a CPU tensor
        with pytest.raises(RuntimeError):
            mov.to_tensor(out=guard[:n].float())  # the wrong dtype
        with pytest.raises(RuntimeError):
            mov.to_tensor(out=guard[: n - 1])  # too small
        with pytest.raises(ValueError):
            mov.to_tensor(slice(0, None, -1))
        with pytest.raises(ValueError):
            mov.to_tensor(dtype=torch.int32)
        cam = mov.handle
        code = ord("H")
        st = torch.cuda.current_stream().cuda_stream
        ptr, nbytes = guard.data_ptr(), guard.numel() * 2
        assert rv._v.rir_load_images_device(cam, 0, 4, 0, code, ptr, nbytes, st) == -1  # step 0
        assert rv._v.rir_load_images_device(cam, 0, 4, -2, code, ptr, nbytes, st) == -1
        assert rv._v.rir_load_images_device(cam, 0, n, 1, code, ptr, n * h * w * 2 - 2, st) == -1  # one byte short
        assert rv._v.rir_load_images_device(cam, 0, n + 1, 1, code, ptr, nbytes, st) == -1  # past the end
        assert rv._v.rir_load_images_device(cam, 0, 2, 1, ord("d"), ptr, nbytes, st) == -1
        torch.cuda.synchronize()
        assert bool((guard.view(torch.int16) == 0x5A5A).all())  # nothing was written
        assert torch.equal(mov.to_tensor(out=guard[:n]).cpu(), torch.from_numpy(arr.astype(np.int32)).to(torch.uint16))


def sha(p):
    return hashlib.sha256(open(p, "rb").read()).hexdigest()


@pytest.mark.parametrize("h,w,gop,n", [(48, 80, 5, 23), (67, 83, None, 61), (512, 640, 50, 120)])
def test_write_parity_byte_identical(tmp_path, h, w, gop, n):
    arr = s1_noisy_background(n, h, w, seed=21)
    ts = np.arange(n, dtype=np.int64) * 1000003 + 11
    ref = record(tmp_path / "ref.h264", arr, gop, ts)
    t = torch.from_numpy(arr.astype(np.int32)).to(torch.uint16).cuda()

    def saver(name):
        s = IRSaver(tmp_path / name, w, h, h)
        if gop:
            s.set_parameter("GOP", gop)
        return s

    with saver("dev.h264") as s:  # device adds only, in uneven pieces
        for a, b in ((0, 7), (7, 8), (8, n)):
            s.add_images(t[a:b], ts[a:b])
    assert sha(tmp_path / "dev.h264") == sha(ref)
    g = gop or 50
    cut = [min(n, g - 2), min(n, g + 3)]
    with saver("mix.h264") as s:  # host, then device across a chunk boundary, then host
        for i in range(cut[0]):
            s.add_image(arr[i], int(ts[i]))
        s.add_images(t[cut[0]:cut[1]], ts[cut[0]:cut[1]])
        for i in range(cut[1], n):
            s.add_image(arr[i], int(ts[i]))
    assert sha(tmp_path / "mix.h264") == sha(ref)
    with IRMovie.from_filename(tmp_path / "dev.h264") as mov:
        assert torch.equal(mov.to_tensor(), t)


def test_write_stream_order_and_buffer_reuse(tmp_path):
    n, h, w = 40, 256, 320
    arr = s1_noisy_background(n, h, w, seed=30)
    ts = np.arange(n, dtype=np.int64) * 1000
    src = torch.from_numpy(arr.astype(np.int32)).cuda()
    dst = tmp_path / "order.h264"
    s = IRSaver(dst, w, h, h)
    s.set_parameter("GOP", 8)
    for k in range(0, n, 10):
        # frames made by torch ops on the current stream just before the call (long enough a kernel for a missing wait to show)
        x = src[k:k + 10].clone()
        for _ in range(30):
            x = (x * 3 + 1) % 65536
        t = x.to(torch.uint16)
        s.add_images(t, ts[k:k + 10])
        t.fill_(0xABCD)  # overwritten at once: the file must not see it
    s.close()
    x = src.clone()
    for _ in range(30):
        x = (x * 3 + 1) % 65536
    exp = x.to(torch.uint16)
    with IRMovie.from_filename(dst) as mov:
        assert torch.equal(mov.to_tensor(), exp)
        assert np.array_equal(mov[17], exp[17].cpu().numpy())


def test_lossy_saver_is_refused(tmp_path):
    n, h, w = 4, 32, 64
    arr = s1_noisy_background(n, h, w)
    with IRSaver(tmp_path / "l.h264", w, h, h - 3) as s:
        s.add_image_lossy(arr[0], 0)
        t = torch.from_numpy(arr.astype(np.int32)).to(torch.uint16).cuda()
        assert rv._v.rir_add_images_device(s.handle, t.data_ptr(), n, np.arange(n, dtype=np.int64).ctypes.data, None) == -2
        with pytest.raises(RuntimeError):
            s.add_images(t, np.arange(n))


@pytest.mark.perf
def test_to_tensor_rate_floor(tmp_path):
    """to_tensor of the 1 000-image S1 movie against torch.from_numpy(mov.data).cuda(), in one process"""
    arr = s1_noisy_background(1000, 512, 640)
    with IRMovie.from_filename(record(tmp_path / "s1.h264", arr)) as mov:
        mov.to_tensor()
        torch.from_numpy(mov.data.astype(np.int32))
        torch.cuda.synchronize()
        best_dev = best_host = 1e9
        for _ in range(3):
            t0 = time.perf_counter()
            mov.to_tensor()
            best_dev = min(best_dev, time.perf_counter() - t0)
            t0 = time.perf_counter()
            torch.from_numpy(mov.data).cuda()
            torch.cuda.synchronize()
            best_host = min(best_host, time.perf_counter() - t0)
    print("to_tensor %.1f ms, from_numpy(mov.data).cuda() %.1f ms: %.2fx" % (best_dev * 1e3, best_host * 1e3, best_host / best_dev))
    assert best_host / best_dev >= RATE_FLOOR


RATE_FLOOR = 6.0  # first GPU run: 12.5x (to_tensor 5.2 ms against 65.1 ms); half of that, for a loaded box
