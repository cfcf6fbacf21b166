"""GPU: flat morphology, bit for bit against the numpy reference of morphology_cases.py (checked against scipy in test_morphology_cpu.py) - the
small cases over every kernel (type, size, op) and tile edge, extreme pixels at the nine corner / edge / interior positions, the rows rule,
sentinel fill, batches, full-size frames, the named forms, the host entry and recordings through IRMovie.morphology."""
import ctypes as ct

import numpy as np
import pytest

from morphology_cases import CASES, OPS, Case, case_id, make_stack, reference, spike_images

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).cuda().view(torch.uint16)
    return torch.from_numpy(a).cuda()


def host(t):
    if t.dtype == torch.uint16:
        return t.cpu().view(torch.int16).numpy().view(np.uint16)
    return t.cpu().numpy()


def run(stack, op, size, **kw):
    from librir_amd import device as D

    return host(D.morphology(dev(stack), op, size, **kw))


def teq(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(host(a), host(b))


def same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_small_cases(case):
    stack = make_stack(case)
    assert same(run(stack, case.op, (case.size_y, case.size_x)), reference(stack, case.op, case.size_y, case.size_x))


@pytest.mark.parametrize("case", [c for c in CASES if c.h >= 17][::4], ids=case_id)
def test_rows(case):
    """the same stack with the last three rows, and with every row, outside the image: copied, and read by no window"""
    stack = make_stack(case)
    for rows in (case.h - 3, 0, 1):
        assert same(run(stack, case.op, (case.size_y, case.size_x), rows=rows), reference(stack, case.op, case.size_y, case.size_x, rows)), rows


@pytest.mark.parametrize("dtype", [np.uint16, np.uint8, np.bool_], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("h,w,size", [(17, 64, 3), (17, 64, 5), (17, 64, 7), (17, 65, 3), (9, 11, (7, 3)), (17, 65, (3, 9)), (3, 64, 3), (5, 6, 15)])
def test_one_extreme_pixel_at_the_nine_positions(dtype, h, w, size):
    stack = spike_images(h, w, dtype)
    sy, sx = (size, size) if isinstance(size, int) else size
    for op in OPS:
        assert same(run(stack, op, size), reference(stack, op, sy, sx)), op


@pytest.mark.parametrize("case", [CASES[0], CASES[17], CASES[40], CASES[70], CASES[99], CASES[140]], ids=case_id)
def test_out_is_fully_overwritten(case):
    from librir_amd import device as D

    stack = make_stack(case)
    for rows in (case.h, max(0, case.h - 3)):
        want = reference(stack, case.op, case.size_y, case.size_x, rows)
        for sentinel in (0, 1):  # (no value is free in a bool image: two fills, one of which every pixel differs from)
            fill = np.full(stack.shape, 165 if sentinel and stack.dtype != np.bool_ else sentinel).astype(stack.dtype)
            out = dev(fill)
            back = D.morphology(dev(stack), case.op, (case.size_y, case.size_x), rows=rows, out=out)
            assert back is out and same(host(out), want), (rows, sentinel)


@pytest.mark.parametrize("size", [3, 7, (9, 5)])
def test_a_batch_equals_its_frames(size):
    case = Case("uint16", 67, 130, 5, 0, 0, "")
    stack = np.concatenate([make_stack(case), spike_images(67, 130, np.uint16)[:4]])
    for op in OPS:
        whole = run(stack, op, size)
        for i in range(stack.shape[0]):
            assert np.array_equal(whole[i], run(stack[i], op, size)), (op, i)
        assert run(stack[0], op, size).shape == (67, 130)


@pytest.fixture(scope="module")
def full_frames():
    rng = np.random.default_rng(5)
    stack = rng.integers(0, 65536, (4, 512, 640)).astype(np.uint16)
    stack[1, ::9, ::7] = 0
    stack[2] = stack[2] // 256 + 20000  # a flat frame with small detail
    stack[3, 0, :], stack[3, -1, :], stack[3, :, 0], stack[3, :, -1] = 65535, 0, 0, 65535
    return stack, dev(stack)


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("size", [(3, 3), (9, 5)], ids=["3x3", "9x5"])
def test_full_size_frames(full_frames, size, op):
    from librir_amd import device as D

    stack, d_stack = full_frames
    assert same(host(D.morphology(d_stack, op, size)), reference(stack, op, size[0], size[1]))


def test_named_forms_equal_the_generic_one():
    from librir_amd import device as D

    stack = make_stack(Case("uint16", 17, 130, 3, 0, 0, ""))
    mask = make_stack(Case("bool", 17, 83, 2, 0, 0, ""))
    names = dict(erode=D.erode, dilate=D.dilate, open=D.morph_open, close=D.morph_close, tophat=D.top_hat, blackhat=D.black_hat,
                 gradient=D.morph_gradient)
    assert sorted(names) == sorted(OPS)
    for frames in (stack, mask):
        d = dev(frames)
        for op, f in names.items():
            for size, rows in ((3, None), ((5, 3), 14)):
                want = D.morphology(d, op, size, rows)
                assert teq(f(d, size, rows), want)
                out = torch.empty_like(d)
                assert f(d, size, rows=rows, out=out) is out and teq(out, want)


def test_non_contiguous_and_sliced_input():
    """a column slice is copied to a contiguous stack first; frames that start at an odd pixel take the tile kernel"""
    from librir_amd import device as D

    stack = make_stack(Case("uint16", 17, 131, 3, 0, 0, ""))
    d = dev(stack)
    assert same(host(D.morphology(d[:, :, 1:], "open", 3)), reference(stack[:, :, 1:], "open", 3, 3))
    flat = dev(np.concatenate([np.zeros(1, np.uint16), stack[:, :, :130].ravel()]))
    odd = flat[1:].view(3, 17, 130)  # contiguous, 2 bytes off dword alignment
    assert same(host(D.morphology(odd, "tophat", 5)), reference(stack[:, :, :130], "tophat", 5, 5))
    bytes_ = make_stack(Case("uint8", 17, 130, 2, 0, 0, ""))
    flat8 = dev(np.concatenate([np.zeros(1, np.uint8), bytes_.ravel()]))
    assert same(host(D.morphology(flat8[1:].view(2, 17, 130), "close", 3)), reference(bytes_, "close", 3, 3))


def test_overlap_is_refused():
    from librir_amd import device as D

    d = dev(make_stack(Case("uint16", 17, 64, 4, 0, 0, "")))
    with pytest.raises(RuntimeError, match="overlap"):
        D.morphology(d[:3], "erode", 3, out=d[1:])
    with pytest.raises(RuntimeError, match="overlap"):
        D.morphology(d, "erode", 3, out=d)


@pytest.mark.parametrize("dtype", ["uint16", "uint8", "bool"])
def test_host_entry_equals_device_entry(lib, dtype):
    from librir_amd import signal_processing as S

    for (n, h, w), op, size, rows in [((5, 67, 83), "tophat", (9, 5), None), ((3, 17, 64), "open", 3, 14), ((2, 1, 1), "gradient", 15, None),
                                      ((1, 3, 5), "erode", 1, 0)]:
        stack = make_stack(Case(dtype, h, w, n, 0, 0, ""))
        want = run(stack, op, size, rows=rows)
        sy, sx = (size, size) if isinstance(size, int) else size
        assert same(want, reference(stack, op, sy, sx, rows))
        assert same(S.morphology(stack, op, size, rows), want)
        assert same(S.morphology(stack[0], op, size, rows), want[0])
        # dst == src through the C entry
        lib.rir_morphology.argtypes = [ct.c_int, ct.c_void_p, ct.c_void_p] + [ct.c_int] * 7
        work = stack.copy()
        assert lib.rir_morphology(ord({"uint16": "H", "uint8": "B", "bool": "?"}[dtype]), work.ctypes.data, work.ctypes.data, w, h, n, OPS.index(op), sx, sy,
                                  h if rows is None else rows) == 0
        assert same(work, want)


def test_host_entry_in_slabs():
    """more than one 64 MiB slab of frames: 110 frames of 640 x 512 uint16"""
    from librir_amd import signal_processing as S

    rng = np.random.default_rng(9)
    stack = np.tile(rng.integers(0, 65536, (5, 512, 640)).astype(np.uint16), (22, 1, 1))
    stack[:, 0, 0] = np.arange(110)
    got = S.morphology(stack, "dilate", 3)
    assert same(got[:5], reference(stack[:5], "dilate", 3, 3)) and same(got[105:], reference(stack[105:], "dilate", 3, 3))
    assert np.array_equal(got[5:, 5:, 5:], np.tile(got[:5, 5:, 5:], (21, 1, 1)))


def record(path, frames):
    from librir_amd.video_io import IRSaver

    n, h, w = frames.shape
    with IRSaver(str(path), w, h, h) as s:
        for i in range(n):
            s.add_image(frames[i], i * 20000000 + 7)
    return str(path)


def test_recordings(tmp_path):
    from librir_amd import device as D
    from librir_amd.synthetic import s1_noisy_background
    from librir_amd.video_io import IRMovie

    n, h, w = 7, 67, 83
    arr = s1_noisy_background(n, h, w, seed=4)
    with IRMovie.from_filename(record(tmp_path / "m.h264", arr)) as mov:
        for sel, op, size, rows in [(slice(None), "tophat", 9, None), (slice(1, None, 2), "open", (3, 5), h - 3), (3, "gradient", 3, None),
                                    (slice(0, 0), "erode", 3, None)]:
            frames = mov.to_tensor(sel)
            want = D.morphology(frames, op, size, rows)
            got = mov.morphology(op, size, sel, rows)
            assert got.dtype == torch.uint16 and got.shape == frames.shape and teq(got, want), (sel, op)
            out = dev(np.full(tuple(want.shape), 12345, np.uint16))
            assert mov.morphology(op, size, selection=sel, rows=rows, out=out) is out and teq(out, want)
            sy, sx = (size, size) if isinstance(size, int) else size
            assert same(host(got), reference(host(frames), op, sy, sx, rows))
        # pieces smaller than the selection give the same bits
        want = mov.morphology("close", 5)
        mov._STATS_PIECE_BYTES = 3 * h * w * 2
        assert teq(mov.morphology("close", 5), want)
        with pytest.raises(ValueError):
            mov.morphology("open", 4)
        with pytest.raises(RuntimeError):
            mov.morphology("open", 3, out=torch.empty((n, h, w + 1), dtype=torch.uint16, device="cuda"))
