"""GPU: windowed reads of recordings (IRMovie.to_tensor(window=...), rir_load_window_device, rirb1_decode_window) - bit for bit the crop
of the whole read: over frame shapes whose tiles straddle rows or are cut, windows that take the FAST and the general form and that miss
tiles of their run, every selection, the full 16-bit range, read-back filters, MIN_T, the other file kinds, and the reducers on top."""
import struct

import numpy as np
import pytest

from librir_amd.synthetic import inject_bad_pixels, s1_noisy_background
from librir_amd.video_io import IRMovie, IRSaver
from librir_amd.video_io import rir_video_io as rv

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TILE_PX = 512
SELECTIONS = [slice(None), slice(3, 17), 5, -1, slice(1, None, 3), slice(2, 40, 7), slice(8, 8)]


def record(path, frames, gop=None):
    n, h, w = frames.shape
    with IRSaver(path, w, h, h) as s:
        if gop:
            s.set_parameter("GOP", gop)
        for i in range(n):
            s.add_image(frames[i], i * 20000000 + 7)
    return path


def dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.int32)).to(torch.uint16).cuda()


def same(a, b):
    """equal shapes, dtypes and bits (uint16 compared as int16: the same bytes)"""
    if a.dtype == torch.uint16 and b.dtype == torch.uint16:
        a, b = a.view(torch.int16), b.view(torch.int16)
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


def positions_of(sel, n):
    return [sel + (n if sel < 0 else 0)] if isinstance(sel, int) else list(range(n))[sel]


def check_windows(mov, expected, windows, sels=SELECTIONS):
    """to_tensor(sel, window=...) against the crop of `expected` (a CUDA uint16 tensor of every image) and of to_tensor(sel), both dtypes"""
    n = mov.images
    for sel in sels:
        pos = positions_of(sel, n)
        exp = expected.view(torch.int16)[pos].view(torch.uint16) if len(pos) else expected[:0]
        whole = mov.to_tensor(sel)
        assert same(whole, exp), sel
        for win in windows:
            y0, x0, h, w = win
            got = mov.to_tensor(sel, window=win)
            assert got.is_cuda and got.dtype == torch.uint16 and tuple(got.shape) == (len(pos), h, w) and got.is_contiguous(), (sel, win)
            assert same(got, exp[:, y0:y0 + h, x0:x0 + w]), (sel, win)
            assert same(got, whole[:, y0:y0 + h, x0:x0 + w]), (sel, win)
            gf = mov.to_tensor(sel, dtype=torch.float32, window=win)
            assert gf.dtype == torch.float32 and tuple(gf.shape) == (len(pos), h, w) and torch.equal(gf, got.float()), (sel, win)


def windows_of(h, w):
    """the windows of the issue, each where it fits the shape"""
    wins = [(0, 0, h, w), (0, 0, 1, 1), (h - 1, w - 1, 1, 1), (h // 2, 0, 1, w), (0, w // 3, h, 1), (5, 3, 9, 13), (h - 11, w - 21, 11, 21),
            (h - 1, 0, 1, w), (0, w - 1, h, 1)]
    if w % 8 == 0:
        wins += [(8, 8, 16, 16), (8, 9, 16, 16), (0, w - 24, h, 24)]  # FAST; the general form on the same data; FAST to the last column
    if w == 1024:
        wins += [(10, 0, 5, 512), (10, 512, 5, 512), (10, 500, 5, 24), (2, 100, 1, 40), (2, 104, 1, 40), (0, 512, 48, 8)]
    return wins


def tile_run(h, w, win):
    y0, x0, wh, ww = win
    return (y0 * w + x0) // TILE_PX, ((y0 + wh - 1) * w + x0 + ww - 1) // TILE_PX + 1


def test_cases_reach_what_they_are_for():
    """(arithmetic only) the shapes and windows reach: lanes that straddle rows, a cut last tile, tiles of the run without a window
    pixel, a window inside one tile, FAST windows, and tiles that straddle rows with W % 8 == 0"""
    assert 83 % 8 and (67 * 83) % TILE_PX  # lanes straddle rows; the last tile is cut
    assert tile_run(67, 83, (66, 82, 1, 1)) == (10, 11) and 67 * 83 < 11 * TILE_PX  # the last pixel lies in the cut tile
    assert 520 % 8 == 0 and TILE_PX % 520  # whole lanes, tiles that straddle rows
    assert tile_run(48, 1024, (10, 0, 5, 512)) == (20, 29) and tile_run(48, 1024, (10, 512, 5, 512)) == (21, 30)  # every second tile misses
    a, b = tile_run(48, 1024, (2, 100, 1, 40))
    assert b - a == 1
    a, b = tile_run(48, 1024, (0, 100, 48, 1))
    assert b - a == 95  # a column: every left-half tile, the right-half ones between them miss
    for h, w in ((64, 96), (48, 1024), (40, 520)):
        assert (8, 8, 16, 16) in windows_of(h, w)


@pytest.mark.parametrize("h,w,gop", [(67, 83, None), (67, 83, 4), (64, 96, 5), (48, 1024, 6), (40, 520, 4)])
def test_window_parity_rirb(tmp_path, h, w, gop):
    n = 43
    arr = s1_noisy_background(n, h, w, seed=3)
    with IRMovie.from_filename(record(tmp_path / "m.h264", arr, gop)) as mov:
        full = mov.to_tensor(window=(0, 0, h, w))
        assert same(full, mov.to_tensor()) and same(full, dev16(arr))
        check_windows(mov, dev16(arr), windows_of(h, w))


@pytest.mark.parametrize("h,w,gop,win", [(67, 83, 4, (5, 3, 9, 13)), (40, 520, 4, (8, 8, 16, 16)), (48, 1024, 6, (10, 512, 5, 512))])
def test_stores_stay_inside_out(tmp_path, h, w, gop, win):
    n = 43
    arr = s1_noisy_background(n, h, w, seed=6)
    y0, x0, wh, ww = win
    exp = dev16(arr)[:, y0:y0 + wh, x0:x0 + ww]
    with IRMovie.from_filename(record(tmp_path / "m.h264", arr, gop)) as mov:
        big = torch.full((n + 2, wh, ww), 0xABCD - 65536, dtype=torch.int16, device="cuda").view(torch.uint16)
        guard = big[0].clone()
        got = mov.to_tensor(out=big[1:n + 1], window=win)
        assert got.data_ptr() == big[1].data_ptr() and same(got, exp)
        assert same(big[0], guard) and same(big[n + 1], guard)
        bigf = torch.full((n + 2, wh, ww), -7.0, dtype=torch.float32, device="cuda")
        mov.to_tensor(dtype=torch.float32, out=bigf[1:n + 1], window=win)
        assert torch.equal(bigf[1:n + 1], exp.float()) and bool((bigf[0] == -7.0).all()) and bool((bigf[n + 1] == -7.0).all())
        # a selection that fills part of `out` from a batch with skipped frames: the slots behind stay as they were
        big.view(torch.int16).fill_(0xABCD - 65536)
        k = len(range(n)[2:40:7])
        mov.to_tensor(slice(2, 40, 7), out=big[1:k + 1], window=win)
        assert same(big[1:k + 1], exp[2:40:7]) and same(big[0], guard) and all(same(big[i], guard) for i in range(k + 1, n + 2))


def key_modes(path, ntiles, gop):
    """the mode of every tile's key record in the first chunk of a recording (the container: DESIGN.md section 4)"""
    blob = open(path, "rb").read()
    index_offset = struct.unpack_from("<Q", blob, 32 + 32)[0]
    c0 = struct.unpack_from("<Q", blob, index_offset)[0]
    assert blob[c0:c0 + 4] == b"CHNK"
    hdr = np.frombuffer(blob, np.uint64, ntiles * gop, c0 + 32).reshape(ntiles, gop)
    return (hdr[:, 0] >> np.uint64(14)) & np.uint64(3)


@pytest.mark.parametrize("kind", ["uniform", "ramp"])
def test_full_range_and_key_modes(tmp_path, kind):
    n, h, w, gop = 43, 67, 83, 4
    rng = np.random.default_rng(17)
    if kind == "uniform":  # RAW keys, 16-bit planes; frames that are all 0 and all 65535
        arr = rng.integers(0, 65536, (n, h, w)).astype(np.uint16)
        arr[4], arr[5], arr[9], arr[22] = 0, 65535, 65535, 0
    else:  # the first image of every chunk a ramp and small noise: a LEFT key record.  The ramp runs along the pixels of a tile, 512 in
        # frame order (a ramp along the rows of 83 jumps back in every block of a tile's pixels, and RAW is the shorter record)
        arr = s1_noisy_background(n, h, w, seed=9)
        keys = 30000 + 61 * (np.arange(h * w) % TILE_PX)[None, :] + rng.integers(0, 4, (len(arr[::gop]), h * w))
        arr[::gop] = keys.reshape(-1, h, w).astype(np.uint16)
    p = record(tmp_path / "m.h264", arr, gop)
    modes = key_modes(p, (h * w + TILE_PX - 1) // TILE_PX, gop)
    assert (modes == (0 if kind == "uniform" else 2)).all(), modes  # RIRB1_MODE_RAW / RIRB1_MODE_LEFT
    with IRMovie.from_filename(p) as mov:
        check_windows(mov, dev16(arr), [(5, 3, 9, 13), (0, 0, h, w)])


def host_stack(mov, n):
    return np.stack([mov.load_pos(p) for p in range(n)])


def test_filters(tmp_path):
    """bad pixels, motion correction and both: the crop of what load_pos gives; the second window reaches the rows the filters leave alone"""
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
            exp = host_stack(mov, n)
            assert not np.array_equal(exp, arr)
            check_windows(mov, dev16(exp), [(5, 3, 9, 13), (60, 70, 7, 13)], [slice(None), slice(3, 19, 3), 7])


def test_camera_state_is_left_alone(tmp_path):
    n, h, w = 26, 67, 83
    arr = s1_noisy_background(n, h, w, seed=5)
    with IRMovie.from_filename(record(tmp_path / "s.h264", arr, 4)) as mov:
        k, x, y = 9, 11, 20
        img = mov.load_pos(k)
        attrs = dict(mov.frame_attributes)
        raw = rv.get_last_image_raw_value(mov.handle, x, y)
        got = mov.to_tensor(slice(14, 25, 2), window=(5, 3, 9, 13))
        assert same(got, dev16(arr[14:25:2, 5:14, 3:16]))
        assert rv.get_last_image_raw_value(mov.handle, x, y) == raw == arr[k, y, x]
        assert rv.get_attributes(mov.handle) == attrs
        assert np.array_equal(mov.load_pos(k), img)


def test_subtract_min(tmp_path):
    """a bounded-loss recording with subtractMin: MIN_T comes back on the first 61 rows only, which two of the windows straddle"""
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
        check_windows(mov, dev16(host_stack(mov, n)), [(58, 0, 6, 80), (59, 7, 4, 11), (0, 0, 3, 8)], [slice(None), slice(2, 21, 4), 6])


@pytest.mark.parametrize("kind", ["pcr", "bin", "zfile"])
def test_raw_and_zfile(tmp_path, kind):
    from librir_amd.video_io.IRMovie import create_pcr_header

    n, h, w = 17, 40, 72
    arr = inject_bad_pixels(s1_noisy_background(n, h, w, seed=8), 5)
    p = tmp_path / ("m." + kind)
    if kind == "pcr":
        with open(p, "wb") as f:
            f.write(create_pcr_header(h, w, 50).astype(np.uint32).tobytes())
            f.write(arr.tobytes())
    elif kind == "bin":
        zh = bytes([1, 1, 0]) + b"\0" * 125  # version, one trigger, compression 0: raw frames behind the two blocks
        zt = struct.pack("<11Q", 0, 50, n, 0, 0, 1, 0, 0, 0, w, h)
        p.write_bytes(zh + zt + b"\0" * (128 - len(zt)) + arr.tobytes())
    else:
        wr = rv.open_video_write(p, w, h, 50, 1, 3)
        for i in range(n):
            rv.image_write(wr, arr[i], i * 1000)
        rv.close_video(wr)
    wins = [(5, 3, 9, 13), (0, 0, h, w)]
    with IRMovie.from_filename(p) as mov:
        assert mov.images == n
        check_windows(mov, dev16(arr), wins, [slice(None), slice(2, 15, 3), -2, slice(5, 5)])
        mov.bad_pixels_correction = True
        exp = host_stack(mov, n)
        assert not np.array_equal(exp, arr)
        check_windows(mov, dev16(exp), wins, [slice(None), slice(1, 16, 5)])


def test_temporal_median_through_a_window(tmp_path):
    n, h, w = 43, 67, 83
    win = (5, 3, 9, 13)
    arr = s1_noisy_background(n, h, w, seed=3)
    with IRMovie.from_filename(record(tmp_path / "m.h264", arr, 4)) as mov:
        whole = {i: mov.to_tensor(sel, temporal_median=5, median_threshold=0) for i, sel in enumerate((slice(None), slice(2, 40, 7)))}
        mov._MEDIAN_PIECE_BYTES = 11 * 9 * 13 * 2  # eleven images of the window a piece
        for i, sel in enumerate((slice(None), slice(2, 40, 7))):
            for dtype in (torch.uint16, torch.float32):
                got = mov.to_tensor(sel, dtype=dtype, temporal_median=5, median_threshold=0, window=win)
                exp = whole[i][:, 5:14, 3:16]
                assert same(got, exp if dtype == torch.uint16 else exp.float()), (sel, dtype)
        assert not same(whole[0], dev16(arr))  # (the filter did something)


def test_region_and_pixel_stats_through_a_window(tmp_path):
    from librir_amd import device as D

    n, h, w = 43, 67, 83
    y0, x0, wh, ww = win = (5, 3, 9, 13)
    arr = s1_noisy_background(n, h, w, seed=3)
    labels = ((np.arange(wh)[:, None] // 3) * 2 + (np.arange(ww)[None, :] // 7)).astype(np.int32)
    labels[0, :4] = -1
    with IRMovie.from_filename(record(tmp_path / "m.h264", arr, 4)) as mov:
        mov._STATS_PIECE_BYTES = 15 * wh * ww * 2  # 43 images: three pieces
        for sel in (slice(None), slice(1, None, 3)):
            crop = mov.to_tensor(sel)[:, y0:y0 + wh, x0:x0 + ww].contiguous()
            exp = D.region_stats(crop, torch.from_numpy(labels).cuda(), 6)
            for lab in (labels, torch.from_numpy(labels).cuda()):
                got = mov.region_stats_window(lab, win, sel, 6)
                for name, a, b in zip(exp._fields, got, exp):
                    assert same(a, b), (sel, name)
            exp = D.pixel_stats(crop)
            got = mov.pixel_stats_window(win, sel)
            assert got.count == exp.count == crop.shape[0]
            for name, a, b in zip(exp._fields, got, exp):
                assert tuple(a.shape) == (wh, ww) and same(a, b), (sel, name)
        with pytest.raises((RuntimeError, ValueError)):
            mov.region_stats_window(np.zeros((h, w), np.int32), win)  # labels of the whole image


def test_corrupted_tile_offsets_inside_the_run(tmp_path):
    """a tile offset of the first chunk that decreases, at a tile of the window's run: refused by the host's check of the slice before
    anything is launched - the output untouched, the next read of the intact file fine"""
    n, h, w, gop = 12, 40, 520, 4
    win = (8, 8, 16, 16)
    arr = s1_noisy_background(n, h, w, seed=4)
    src = record(tmp_path / "ok.h264", arr, gop)
    ntiles = (h * w + TILE_PX - 1) // TILE_PX
    t_lo, t_hi = tile_run(h, w, win)
    t = (t_lo + t_hi) // 2
    assert t_lo < t < t_hi - 1
    blob = bytearray(open(src, "rb").read())
    index_offset = struct.unpack_from("<Q", blob, 32 + 32)[0]  # (ftyp box, then the file header)
    c0 = struct.unpack_from("<Q", blob, index_offset)[0]  # index entry 0: its chunk's offset
    assert blob[c0:c0 + 4] == b"CHNK"
    toff = c0 + 32 + ntiles * gop * 8  # chunk header, record headers, then ntiles + 1 tile offsets
    offs = struct.unpack_from("<%dI" % (ntiles + 1), blob, toff)
    assert offs[0] == 0 and all(a < b for a, b in zip(offs, offs[1:])) and offs[ntiles] == struct.unpack_from("<Q", blob, c0 + 16)[0]
    struct.pack_into("<I", blob, toff + 4 * (t + 1), offs[t] - 1)
    bad = tmp_path / "bad.h264"
    bad.write_bytes(bytes(blob))
    out = torch.full((n, 16, 16), 0xABCD - 65536, dtype=torch.int16, device="cuda").view(torch.uint16)
    guard = out.clone()
    with IRMovie.from_filename(bad) as mov:
        with pytest.raises(RuntimeError, match="corrupted tile offsets"):
            mov.to_tensor(out=out, window=win)
        torch.cuda.synchronize()
        assert same(out, guard)
        assert same(mov.to_tensor(slice(gop, None), window=win), dev16(arr[gop:, 8:24, 8:24]))  # the chunks behind it are intact
        with pytest.raises(RuntimeError, match="corrupted tile offsets"):
            mov.to_tensor(1, window=win)
    with IRMovie.from_filename(src) as mov:
        assert same(mov.to_tensor(out=out, window=win), dev16(arr[:, 8:24, 8:24]))
