"""GPU: recordings read into device tensors (IRMovie.to_tensor, rir_load_images_device) and recorded from them (IRSaver.add_images,
rir_add_images_device) over the full 16-bit range, pinned to numpy - the frames that were recorded, or MIN_T as numpy defines it
(device_io_cases.min_t_expected) - and never to another call of the library; the one exception are reads with a read-back filter on,
where load_pos image by image is the reference as elsewhere in the suite (said where it applies).

test_gpu_device_io.py compares this path with the library's other route on S1 data (values below about 1 100).  What that leaves open, and
is closed here (cases and their reach: device_io_cases.py, test_device_io_cases_cpu.py):
  a. values >= 16 384 through the selective decoder: 16-bit-wide records, the float32 conversion of values with bit 15 set (decoder, and
     the raw path's u16 -> f32 kernel), wrap-around of the packed 16-bit add; GOP 1, step == GOP, a lone last frame of a chunk and of the
     short last chunk, a recording that is a multiple of its GOP, a GOP larger than the recording; frames of 1 and 8 pixels;
  b. MIN_T added to 1..7 pixels of a lane, in a whole (FAST) tile and in the cut last tile, MIN_T that wraps past 65 535 or below 0,
     MIN_T_HEIGHT absent / h / beyond h, MIN_T in a second and a third batch;
  c. `out` off the 16-byte grid (every tile through the ragged form) with sentinels before and behind it, while frames are skipped before,
     between and inside chunks;
  d. filtered reads (bad pixels, motion, both; uint16 and float32) of three batches: the per-batch output slot, shift table and output
     offset (k0 > 0), with a start inside the recording; MIN_T and the filters together;
  e. the two other batch cuts - 64 MiB of page-locked payload, 256 MiB of scratch - and the reuse of a page-locked buffer;
  f. the saver fed from the device with full-range data: pieces that end on and off chunk boundaries, an empty piece, source tensors off
     the 16-byte grid, host and device calls interleaved - the file byte for byte the one add_image makes.

On the MI355X:
  - MIN_T / MIN_T_HEIGHT given through IRSaver.set_global_attributes before the frames survive into the file as they are ("-5" too); no
    rewrite through IRMovie.attributes was needed.
  - (e) byte cut: 138 922 215 B of file for 137 625 600 B of frames (1.0094: tables and trailer on top of a payload of the raw size);
    scratch cut: 28 588 071 B of file (0.2077 of the frames), far below 64 MiB.
  - A slice whose stop lies past the recording is refused by to_tensor (not clamped, as movie[...] does not clamp it either): the chunk by
    chunk reference read of (e) ends its last slice at the recording's length.
  - Everything passed as the library stood: no kernel or host code had to change.  By hand, on a scratch copy, each of these turned a test
    of this file red: `2 * k <= nmin` in SelectSink::add_min (test_min_t_partial_lanes_and_wrap; test_gpu_device_io.py's subtractMin test
    sees this one too, in its lanes behind the boundary), a plain 32-bit add in its place of pk_add16 (test_min_t_partial_lanes_and_wrap),
    `(float)(short)(o.d[0] >> 16)` (test_lossless_read_full_range), the shift table without `+ 2 * k0`
    (test_filtered_reads_past_the_first_batch), `out_first` without `- k0` (the same test: the read is refused as malformed) - the last
    four with test_gpu_device_io.py still green.
"""
import os

import numpy as np
import pytest

import device_io_cases as C
from librir_amd.synthetic import inject_bad_pixels
from librir_amd.video_io import IRMovie, IRSaver
from librir_amd.video_io import rir_video_io as rv
from test_gpu_device_io import host_stack, record, sha

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def picked(arr, sel):
    """arr[sel] as to_tensor shapes it: an int selects a stack of one"""
    return arr[sel][None] if isinstance(sel, int) else arr[sel]


def check_numpy(mov, exp_all, sels):
    """to_tensor(sel), uint16 and float32, against numpy's exp_all[sel]"""
    for sel in sels:
        exp = picked(exp_all, sel)
        got = mov.to_tensor(sel)
        assert got.is_cuda and got.dtype == torch.uint16 and tuple(got.shape) == exp.shape, sel
        assert np.array_equal(got.cpu().numpy(), exp), sel
        gf = mov.to_tensor(sel, dtype=torch.float32)
        assert gf.is_cuda and gf.dtype == torch.float32 and tuple(gf.shape) == exp.shape, sel
        assert torch.equal(gf, torch.from_numpy(exp.astype(np.float32)).cuda()), sel


# ---- a. lossless reads over the full range -------------------------------------------------------------------------------------------


@pytest.mark.parametrize("h,w", C.LOSSLESS_SHAPES)
@pytest.mark.parametrize("kind", C.KINDS)
def test_lossless_read_full_range(tmp_path, kind, h, w):
    recordings = C.LOSSLESS_RECORDINGS + (C.LOSSLESS_EXTRA_RECORDINGS if (h, w) in C.LOSSLESS_EXTRA_SHAPES else [])
    for gop, n in recordings:
        arr = C.frames(kind, n, h, w, seed=n + h)
        with IRMovie.from_filename(record(tmp_path / ("m%s_%d.h264" % (gop, n)), arr, gop)) as mov:
            assert mov.images == n
            assert np.array_equal(mov.to_tensor().cpu().numpy(), arr)
            check_numpy(mov, arr, C.selections(n, gop or C.DEFAULT_GOP))


@pytest.mark.parametrize("kind", ["pcr", "zfile"])
def test_raw_and_zfile_read_full_range(tmp_path, kind):
    """raw frames go up as they are; float32 through the u16 -> f32 kernel, values >= 32 768 included"""
    from librir_amd.video_io.IRMovie import create_pcr_header

    (h, w), n = C.RAW_SHAPE, C.RAW_N
    arr = C.frames("uniform", n, h, w, seed=8)
    assert (arr >= 32768).any()
    p = tmp_path / ("m." + kind)
    if kind == "pcr":
        with open(p, "wb") as f:
            f.write(create_pcr_header(h, w, 50).astype(np.uint32).tobytes())
            f.write(arr.tobytes())
    else:
        wr = rv.open_video_write(p, w, h, 50, 1, 3)
        for i in range(n):
            rv.image_write(wr, arr[i], i * 1000)
        rv.close_video(wr)
    with IRMovie.from_filename(p) as mov:
        assert mov.images == n
        check_numpy(mov, arr, C.selections(n, 4))


# ---- b. MIN_T on a lossless recording ------------------------------------------------------------------------------------------------
# MIN_T / MIN_T_HEIGHT are given to the saver as global attributes before the frames (IRSaver.set_global_attributes): the saver writes
# what it was given, the reader finds them as it finds a bounded-loss recording's.


def record_min_t(path, arr, gop, min_t, min_t_height):
    n, h, w = arr.shape
    attrs = {"MIN_T": str(min_t)}
    if min_t_height is not None:
        attrs["MIN_T_HEIGHT"] = str(min_t_height)
    with IRSaver(path, w, h, h) as s:
        s.set_global_attributes(attrs)
        s.set_parameter("GOP", gop)
        for i in range(n):
            s.add_image(arr[i], i * 1000)
    return path


@pytest.mark.parametrize("min_t", C.MIN_T_VALUES)
@pytest.mark.parametrize("h,w,rows", C.MIN_T_GEOMETRIES)
def test_min_t_partial_lanes_and_wrap(tmp_path, h, w, rows, min_t):
    gop, n = C.MIN_T_RECORDING
    arr = C.with_ends(C.frames("uniform", n, h, w, seed=rows))
    for mth in (rows, None, h, h + 8):
        exp = C.min_t_expected(arr, min_t, 0 if mth is None else mth)
        if mth == h + 8:  # clamped to the frame
            assert np.array_equal(exp, C.min_t_expected(arr, min_t, h))
        changed = exp != arr
        assert changed[:, :C.min_t_rows(h, mth or 0)].all() and not changed[:, C.min_t_rows(h, mth or 0):].any()
        assert (exp.astype(np.int64) != arr.astype(np.int64) + min_t)[changed].any()  # some pixel wrapped
        with IRMovie.from_filename(record_min_t(tmp_path / ("m%s.h264" % mth), arr, gop, min_t, mth)) as mov:
            assert int(mov.attributes["MIN_T"]) == min_t
            assert ("MIN_T_HEIGHT" in mov.attributes) == (mth is not None) and (mth is None or int(mov.attributes["MIN_T_HEIGHT"]) == mth)
            check_numpy(mov, exp, C.MIN_T_SELECTIONS)
            assert np.array_equal(host_stack(mov, range(n)), exp)  # the host route, pinned to numpy as well


def test_min_t_past_the_first_batch(tmp_path):
    d = C.MIN_T_LONG
    arr = C.with_ends(C.frames("uniform", d["n"], d["h"], d["w"], seed=37))
    exp = C.min_t_expected(arr, d["min_t"], d["rows"])
    with IRMovie.from_filename(record_min_t(tmp_path / "long.h264", arr, d["gop"], d["min_t"], d["rows"])) as mov:
        assert int(mov.attributes["MIN_T"]) == d["min_t"]
        check_numpy(mov, exp, d["selections"])
        assert np.array_equal(host_stack(mov, range(d["n"])), exp)


# ---- c. `out` off the 16-byte grid, its neighbours untouched -----------------------------------------------------------------------------


def sentinel_room(elements, dtype):
    """(the room as integers, the same memory as `dtype`, the sentinel): 0x5A5A, or a NaN's bits, in every element"""
    if dtype == torch.uint16:
        raw = torch.full((elements,), 0x5A5A, dtype=torch.int16, device="cuda")
        return raw, raw.view(torch.uint16), 0x5A5A
    raw = torch.full((elements,), 0x7FC05A5A, dtype=torch.int32, device="cuda")
    return raw, raw.view(torch.float32), 0x7FC05A5A


@pytest.mark.parametrize("dtype", ["uint16", "float32"])
@pytest.mark.parametrize("h,w", C.OUT_SHAPES)
def test_out_off_the_grid_and_neighbours(tmp_path, h, w, dtype):
    gop, n = C.OUT_RECORDING
    npx = h * w
    dt = getattr(torch, dtype)
    esz = 2 if dtype == "uint16" else 4
    arr = C.frames("uniform", n, h, w, seed=w)
    with IRMovie.from_filename(record(tmp_path / "m.h264", arr, gop)) as mov:
        for sel in [slice(None, None, step) for step in C.OUT_STEPS] + [slice(1, None, 3), slice(2, None, 2)]:
            exp = arr[sel]
            count = len(exp)
            exp_t = torch.from_numpy(exp.astype(np.float32) if dtype == "float32" else exp).cuda()
            for off in C.OUT_OFFSETS[dtype]:
                raw, room, mark = sentinel_room(count * npx + 16, dt)
                out = room[off:off + count * npx].view(count, h, w)
                assert room.data_ptr() % 16 == 0 and out.data_ptr() % 16 == (off * esz) % 16
                got = mov.to_tensor(sel, dtype=dt, out=out)
                assert got.data_ptr() == out.data_ptr() and torch.equal(out, exp_t), (sel, off)
                assert bool((raw[:off] == mark).all()) and bool((raw[off + count * npx:] == mark).all()), (sel, off)
        # an `out` one frame shorter than the selection is refused before anything is launched
        st = torch.cuda.current_stream().cuda_stream
        for off in C.OUT_OFFSETS[dtype][1:]:
            raw, room, mark = sentinel_room(n * npx + 16, dt)
            short = room[off:off + (n - 1) * npx].view(n - 1, h, w)
            with pytest.raises(RuntimeError):
                mov.to_tensor(dtype=dt, out=short)
            code = ord("H") if dtype == "uint16" else ord("f")
            assert rv._v.rir_load_images_device(mov.handle, 0, n, 1, code, short.data_ptr(), (n - 1) * npx * esz, st) == -1
            torch.cuda.synchronize()
            assert bool((raw == mark).all())


# ---- d. filtered reads past the first batch ------------------------------------------------------------------------------------------------
# (a read-back filter is on: load_pos image by image is the reference here)


def write_shifts(path, shifts):
    with open(path, "w") as f:
        f.write("frame\tx\ty\tconfidence\n")
        for i, (x, y) in enumerate(shifts):
            f.write("%d\t%g\t%g\t1\n" % (i, x, y))
    return path


def check_filtered(mov, n, sels):
    """to_tensor(sel) against load_pos image by image, float32 against the uint16 result; returns the load_pos stack"""
    ref = host_stack(mov, range(n))
    for sel in sels:
        exp = picked(ref, sel)
        got = mov.to_tensor(sel)
        assert got.dtype == torch.uint16 and tuple(got.shape) == exp.shape and np.array_equal(got.cpu().numpy(), exp), sel
        gf = mov.to_tensor(sel, dtype=torch.float32)
        assert gf.dtype == torch.float32 and torch.equal(gf, got.float()), sel
        assert torch.equal(gf, torch.from_numpy(exp.astype(np.float32)).cuda()), sel
    return ref


def test_filtered_reads_past_the_first_batch(tmp_path):
    d = C.FILTERED
    n, h, w, gop = d["n"], d["h"], d["w"], d["gop"]
    arr = inject_bad_pixels(C.frames("s1_high", n, h, w, seed=5), 9)
    shifts = np.random.default_rng(2).uniform(-4, 4, (n, 2))
    reg = write_shifts(tmp_path / "reg.csv", shifts)
    path = record(tmp_path / "f.h264", arr, gop)
    with IRMovie.from_filename(path) as mov:
        mov.registration_file = reg
        refs = {}
        for bp, motion in ((True, False), (False, True), (True, True)):
            mov.bad_pixels_correction = bp
            mov.registration = motion
            refs[bp, motion] = check_filtered(mov, n, d["selections"])
        assert not np.array_equal(refs[True, False], arr)  # the repair did something
        moved = refs[False, True]
        for p in (17, 20, 33):  # images of the second and third batch: the shifts were applied at all
            assert not np.array_equal(moved[p], arr[p])
        # frame p read with frame p - 16's shift is another image: a shift table that is off by a batch's first slot cannot pass
        p = 20
        with IRMovie.from_filename(path) as other:
            other.registration_file = write_shifts(tmp_path / "rolled.csv", np.roll(shifts, 16, axis=0))
            other.registration = True
            wrong = other.to_tensor(p).cpu().numpy()[0]
            assert np.array_equal(wrong, other.load_pos(p)) and not np.array_equal(wrong, moved[p])


def test_min_t_with_filters_past_the_first_batch(tmp_path):
    """the order of MIN_T and the filters, as load_pos has it"""
    d = C.FILTERED
    n, h, w, gop = d["n"], d["h"], d["w"], d["gop"]
    arr = inject_bad_pixels(C.frames("s1_high", n, h, w, seed=6), 9)
    reg = write_shifts(tmp_path / "reg.csv", np.random.default_rng(3).uniform(-4, 4, (n, 2)))
    with IRMovie.from_filename(record_min_t(tmp_path / "fm.h264", arr, gop, 5, h - 3)) as mov:
        exp = C.min_t_expected(arr, 5, h - 3)
        check_numpy(mov, exp, d["selections"])  # no filter on yet: numpy is the reference
        mov.registration_file = reg
        for bp, motion in ((True, False), (False, True), (True, True)):
            mov.bad_pixels_correction = bp
            mov.registration = motion
            ref = check_filtered(mov, n, d["selections"])
            assert not np.array_equal(ref, exp)


# ---- e. the byte cut and the scratch cut ------------------------------------------------------------------------------------------------------


def record_from_device(path, t, gop):
    n, h, w = t.shape
    with IRSaver(path, w, h, h) as s:
        s.set_parameter("GOP", gop)
        s.add_images(t, np.arange(n, dtype=np.int64) * 1000)
    return path


def test_byte_cut(tmp_path):
    """incompressible chunks of 50 images: two fit into the 64 MiB of a page-locked buffer, a third does not - batches of 2, 2 and 1
    chunks, both buffers taken a second time"""
    d = C.LARGE
    h, w, gop = d["h"], d["w"], d["gop"]
    arr = C.large_frames("uniform", seed=41)
    t = torch.from_numpy(arr).cuda()
    path = record_from_device(tmp_path / "big.h264", t, gop)
    size = os.path.getsize(path)
    print("byte cut: file %d B, frames %d B (%.4f)" % (size, arr.nbytes, size / arr.nbytes))
    assert size > 0.95 * arr.nbytes  # the premise: nothing was compressed away, a chunk carries about 32.8 MB
    assert size * 2 * gop / d["n"] + C.batch_bytes_bound(h, w, gop, 2, 0) < C.BATCH_BYTES  # ... and two of them fit
    with IRMovie.from_filename(path) as mov:
        got = mov.to_tensor()
        assert torch.equal(got, t)
        del got
        assert torch.equal(mov.to_tensor(slice(0, None, 7)), t[0::7])


def test_scratch_cut(tmp_path):
    """float32 with motion correction needs two scratch images per selected image: 200 images fit into 256 MiB, 210 do not - batches of
    4 chunks and 1.  Reference: the same movie read chunk by chunk (one batch each); load_pos for four images."""
    d = C.LARGE
    h, w, n, gop = d["h"], d["w"], d["n"], d["gop"]
    arr = C.large_frames("s1_high", seed=42)
    path = record_from_device(tmp_path / "s1.h264", torch.from_numpy(arr).cuda(), gop)
    size = os.path.getsize(path)
    print("scratch cut: file %d B, frames %d B (%.4f)" % (size, arr.nbytes, size / arr.nbytes))
    assert size < 64 << 20  # the premise: the byte limit cannot be what cuts this read
    reg = write_shifts(tmp_path / "reg.csv", np.random.default_rng(4).uniform(-4, 4, (n, 2)))
    with IRMovie.from_filename(path) as mov:
        assert np.array_equal(mov.to_tensor(slice(195, 205)).cpu().numpy(), arr[195:205])
        mov.registration_file = reg
        mov.registration = True
        got = mov.to_tensor(dtype=torch.float32)
        for c in range((n + gop - 1) // gop):
            piece = mov.to_tensor(slice(gop * c, min(n, gop * c + gop)), dtype=torch.float32)  # (a stop past the end is not clamped)
            assert torch.equal(got[gop * c:gop * c + gop], piece), c
            del piece
        for p in (0, 199, 200, 209):
            img = mov.load_pos(p)
            assert np.array_equal(got[p].cpu().numpy(), img.astype(np.float32)), p
            assert not np.array_equal(img, arr[p])


# ---- f. the write side ----------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("h,w", C.WRITE_SHAPES)
def test_write_full_range_byte_identical(tmp_path, h, w, kind):
    gop, n = C.WRITE_RECORDING
    npx = h * w
    arr = C.frames(kind, n, h, w, seed=h)
    ts = np.arange(n, dtype=np.int64) * 1000003 + 11
    ref = sha(record(tmp_path / "ref.h264", arr, gop, ts))
    t = torch.from_numpy(arr).cuda()
    keep = t.clone()

    def saver(name):
        s = IRSaver(tmp_path / name, w, h, h)
        s.set_parameter("GOP", gop)
        return s

    names = ["pieces.h264", "mixed.h264"]
    with saver(names[0]) as s:  # the cut at 3 lies on a chunk boundary, the others do not; (3, 3) is empty
        for a, b in C.WRITE_PIECES:
            s.add_images(t[a:b], ts[a:b])
    with saver(names[1]) as s:  # host and device calls interleaved, the device's across chunk boundaries
        for a, b, device in ((0, 2, False), (2, 7, True), (7, 8, False), (8, n, True)):
            if device:
                s.add_images(t[a:b], ts[a:b])
            else:
                for i in range(a, b):
                    s.add_image(arr[i], int(ts[i]))
    for off in C.WRITE_OFFSETS:  # a source that starts 1 and 4 elements past a 16-byte boundary
        flat = torch.zeros(n * npx + 8, dtype=torch.int16, device="cuda")
        flat[off:off + n * npx].copy_(t.view(torch.int16).flatten())
        src = flat.view(torch.uint16)[off:off + n * npx].view(n, h, w)
        assert flat.data_ptr() % 16 == 0 and src.data_ptr() % 16 == 2 * off and src.is_contiguous()
        names.append("off%d.h264" % off)
        with saver(names[-1]) as s:
            s.add_images(src, ts)
        assert torch.equal(src, keep)
    assert torch.equal(t, keep)  # the source is left as it was
    for name in names:
        assert sha(tmp_path / name) == ref, name
        with IRMovie.from_filename(tmp_path / name) as mov:
            assert np.array_equal(mov.data, arr), name
            assert np.array_equal(mov.to_tensor().cpu().numpy(), arr), name
