"""GPU: spatial rank filters, bit for bit against the numpy reference of rank_cases.py (checked against scipy in test_rank_filter_cpu.py) - the
small cases over both kernels (type, size, rank) and every tile edge, ties, extreme pixels at the nine corner / edge / interior positions,
the rows rule, the two extreme ranks against erode and dilate, the relation to median_filter, long stacks, out=, the host entry and
recordings through IRMovie.window_median."""
import ctypes as ct

import numpy as np
import pytest
from numpy.lib.stride_tricks import sliding_window_view

from morphology_cases import spike_images, type_max
from rank_cases import REGISTER_CASES, TILE_CASES, Case, case_id, full_range_image, make_stack, reference, three_level_image

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


def run(stack, rank, size, **kw):
    from librir_amd import device as D

    return host(D.rank_filter(dev(stack), rank, size, **kw))


def teq(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(host(a), host(b))


def same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("case", REGISTER_CASES, ids=case_id)
def test_register_kernels(case):
    """the medians of 3x3 and 5x5 on even widths, through window_median and through the rank"""
    from librir_amd import device as D

    stack = make_stack(case)
    want = reference(stack, case.rank, case.size_y, case.size_x)
    assert same(host(D.window_median(dev(stack), case.size_y)), want)
    assert same(run(stack, case.rank - case.size_y * case.size_x, (case.size_y, case.size_x)), want)  # counted from the end


@pytest.mark.parametrize("case", TILE_CASES, ids=case_id)
def test_tile_kernel(case):
    stack = make_stack(case)
    assert same(run(stack, case.rank, (case.size_y, case.size_x)), reference(stack, case.rank, case.size_y, case.size_x))


@pytest.mark.parametrize("dtype", [np.uint16, np.uint8, np.bool_], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("h,w,size", [(17, 64, 3), (17, 130, 5), (17, 65, 3), (9, 11, (7, 3)), (17, 65, (3, 9)), (3, 64, 3), (5, 6, 15)])
def test_one_extreme_pixel_at_the_nine_positions(dtype, h, w, size):
    stack = spike_images(h, w, dtype)
    sy, sx = (size, size) if isinstance(size, int) else size
    for rank in sorted({1, sy * sx // 2 - 1, sy * sx // 2, sy * sx - 2}):
        assert same(run(stack, rank, size), reference(stack, rank, sy, sx)), rank


@pytest.mark.parametrize("dtype", [np.uint16, np.uint8, np.bool_], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("h,w,size", [(67, 130, 3), (67, 130, 5), (17, 83, 5), (17, 83, (7, 3)), (67, 65, 9)])
def test_ties_and_constant_images(dtype, h, w, size):
    """three levels only, and one level: every rank of a constant window is that level"""
    rng = np.random.default_rng(h * w)
    stack = np.stack([three_level_image(rng, h, w, dtype), np.full((h, w), type_max(dtype)).astype(dtype), three_level_image(rng, h, w, dtype)])
    sy, sx = (size, size) if isinstance(size, int) else size
    for rank in sorted({1, sy * sx // 2 - 1, sy * sx // 2, sy * sx // 2 + 1, sy * sx - 2}):
        assert same(run(stack, rank, size), reference(stack, rank, sy, sx)), rank


@pytest.mark.parametrize("dtype", [np.uint16, np.uint8, np.bool_], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("h,w,size,rank", [(19, 130, 3, 4), (19, 130, 5, 12), (19, 83, 5, 12), (35, 65, (9, 3), 7), (19, 83, 15, 200)])
def test_rows(dtype, h, w, size, rank):
    """rows below the image are copied and read by no window: a tail of the type's maximum does not leak into the last image rows, so the
    clamp goes to rows - 1 and not to h - 1; rows = 0 is a copy"""
    rng = np.random.default_rng(h + w)
    image = np.stack([full_range_image(rng, h, w, dtype) for _ in range(2)])
    if dtype != np.bool_:
        image //= 2  # (the upper half of the range is the tail's alone)
    sy, sx = (size, size) if isinstance(size, int) else size
    for rows in (h - 3, 1, 0, h):
        stack = image.copy()
        stack[:, rows:] = type_max(dtype)
        got = run(stack, rank, size, rows=rows)
        assert same(got, reference(stack, rank, sy, sx, rows)), rows
        assert same(got[:, rows:], stack[:, rows:])
        if dtype != np.bool_:
            assert (got[:, :rows] < type_max(dtype)).all(), rows


@pytest.mark.parametrize("dtype", ["uint16", "uint8", "bool"])
def test_extreme_ranks_are_erode_and_dilate(dtype):
    from librir_amd import device as D

    for (h, w), size in [((67, 130), 3), ((17, 83), (7, 3)), ((17, 64), 5), ((3, 5), 15), ((5, 6), 1)]:
        stack = make_stack(Case(dtype, h, w, 3, 0, 0, 0))
        d = dev(stack)
        sy, sx = (size, size) if isinstance(size, int) else size
        for rows in (None, max(h - 3, 0)):
            assert teq(D.rank_filter(d, 0, size, rows), D.erode(d, size, rows))
            assert teq(D.rank_filter(d, -1, size, rows), D.dilate(d, size, rows)) and teq(D.rank_filter(d, sy * sx - 1, size, rows), D.dilate(d, size, rows))
            assert teq(D.percentile_filter(d, 0, size, rows), D.erode(d, size, rows)) and teq(D.percentile_filter(d, 100, size, rows), D.dilate(d, size, rows))
        assert same(host(D.rank_filter(d, 0, size)), reference(stack, 0, sy, sx))


def test_percentile_filter_is_the_rank_filter_at_scipys_rank():
    from librir_amd import device as D

    stack = make_stack(Case("uint16", 17, 83, 2, 0, 0, 0))
    d = dev(stack)
    for percent, size, rank in [(25, 9, 20), (-25, 3, 6), (50, 5, 12), (99.9, (3, 5), 14), (10, (7, 3), 2)]:
        sy, sx = (size, size) if isinstance(size, int) else size
        assert same(host(D.percentile_filter(d, percent, size)), reference(stack, rank, sy, sx)), percent


def test_window_median_and_median_filter():
    """the same comparisons inside; on the border the full window with replicated pixels is not the reference's shrunken one"""
    from librir_amd import device as D

    stack = np.random.default_rng(3).integers(0, 65536, (2, 67, 130)).astype(np.uint16)
    for frames in (stack, stack[:, :, :83]):  # the register kernel, and the tile kernel
        d = dev(frames)
        ours, theirs = host(D.window_median(d, 3)), host(D.median_filter(d))
        assert np.array_equal(ours[:, 1:-1, 1:-1], theirs[:, 1:-1, 1:-1])
        border = np.ones(ours.shape, bool)
        border[:, 1:-1, 1:-1] = False
        assert (ours[border] != theirs[border]).any()
        assert same(ours, reference(frames, 4, 3, 3))


def test_a_batch_equals_its_frames_and_one_image_keeps_its_shape():
    stack = make_stack(Case("uint16", 67, 130, 5, 0, 0, 0))
    for size, rank in ((3, 4), (5, 12), (5, 3), ((9, 5), 22)):
        whole = run(stack, rank, size)
        for i in range(stack.shape[0]):
            assert np.array_equal(whole[i], run(stack[i], rank, size)), (size, i)
        assert run(stack[0], rank, size).shape == (67, 130)


def test_full_size_frames():
    rng = np.random.default_rng(5)
    stack = rng.integers(0, 65536, (3, 512, 640)).astype(np.uint16)
    stack[1] = stack[1] // 256 + 20000  # a flat frame with small detail: ties
    stack[2, 0, :], stack[2, -1, :], stack[2, :, 0], stack[2, :, -1] = 65535, 0, 0, 65535
    for size, rank, frames in ((3, 4, stack), (5, 12, stack), (7, 24, stack[2:])):
        assert same(run(frames, rank, size), reference(frames, rank, size, size)), size


def test_more_frames_than_one_grid_holds():
    """65 537 frames of 2 x 2 uint8: the launcher walks gridDim.z in pieces of 65 535"""
    rng = np.random.default_rng(8)
    stack = rng.integers(0, 256, (65537, 2, 2)).astype(np.uint8)
    # (the reference of the whole stack in one sort: frame by frame it would take seconds)
    windows = np.sort(sliding_window_view(np.pad(stack, ((0, 0), (1, 1), (1, 1)), mode="edge"), (3, 3), axis=(1, 2)).reshape(-1, 2, 2, 9), axis=-1)
    for rank in (4, 2):  # the register kernel, and the tile kernel
        assert same(windows[:3, :, :, rank], reference(stack[:3], rank, 3, 3))
        assert same(run(stack, rank, 3), np.ascontiguousarray(windows[..., rank])), rank


def test_non_contiguous_and_unaligned_input():
    """a column slice is copied to a contiguous stack first; frames that start at an odd pixel take the tile kernel"""
    from librir_amd import device as D

    stack = make_stack(Case("uint16", 17, 131, 3, 0, 0, 0))
    d = dev(stack)
    assert same(host(D.window_median(d[:, :, 1:], 3)), reference(stack[:, :, 1:], 4, 3, 3))
    flat = dev(np.concatenate([np.zeros(1, np.uint16), stack[:, :, :130].ravel()]))
    assert same(host(D.window_median(flat[1:].view(3, 17, 130), 5)), reference(stack[:, :, :130], 12, 5, 5))
    bytes_ = make_stack(Case("uint8", 17, 130, 2, 0, 0, 0))
    flat8 = dev(np.concatenate([np.zeros(1, np.uint8), bytes_.ravel()]))
    assert same(host(D.window_median(flat8[1:].view(2, 17, 130), 3)), reference(bytes_, 4, 3, 3))


@pytest.mark.parametrize("size,rank", [(3, 4), (5, 12), ((7, 3), 5)])
def test_out_is_honoured_and_fully_overwritten(size, rank):
    from librir_amd import device as D

    stack = make_stack(Case("uint16", 67, 130, 2, 0, 0, 0))
    sy, sx = (size, size) if isinstance(size, int) else size
    for rows in (67, 64):
        want = reference(stack, rank, sy, sx, rows)
        for sentinel in (0, 165):
            out = dev(np.full(stack.shape, sentinel, np.uint16))
            assert D.rank_filter(dev(stack), rank, size, rows=rows, out=out) is out and same(host(out), want), (rows, sentinel)
    out = torch.empty((2, 67, 130), dtype=torch.uint16, device="cuda")
    assert D.window_median(dev(stack), size, out=out) is out and same(host(out), reference(stack, sy * sx // 2, sy, sx))
    assert D.percentile_filter(dev(stack), 50, size, out=out) is out and same(host(out), reference(stack, sy * sx // 2, sy, sx))


def test_overlap_is_refused():
    from librir_amd import device as D

    d = dev(make_stack(Case("uint16", 17, 64, 4, 0, 0, 0)))
    with pytest.raises(RuntimeError, match="overlap"):
        D.rank_filter(d[:3], 4, 3, out=d[1:])
    with pytest.raises(RuntimeError, match="overlap"):
        D.window_median(d, 3, out=d)


@pytest.mark.parametrize("dtype", ["uint16", "uint8", "bool"])
def test_host_entry_equals_device_entry(lib, dtype):
    from librir_amd import signal_processing as S

    for (n, h, w), rank, size, rows in [((3, 17, 64), 4, 3, 14), ((2, 67, 130), 12, 5, None), ((5, 67, 83), 11, (9, 5), None), ((2, 1, 1), 100, 15, None),
                                        ((1, 3, 5), 0, 1, 0)]:
        stack = make_stack(Case(dtype, h, w, n, 0, 0, 0))
        want = run(stack, rank, size, rows=rows)
        sy, sx = (size, size) if isinstance(size, int) else size
        assert same(want, reference(stack, rank, sy, sx, rows))
        assert same(S.rank_filter(stack, rank, size, rows), want)
        assert same(S.rank_filter(stack[0], rank - sy * sx, size, rows), want[0])
        # dst == src through the C entry
        lib.rir_rank_filter.argtypes = [ct.c_int, ct.c_void_p, ct.c_void_p] + [ct.c_int] * 7
        work = stack.copy()
        assert lib.rir_rank_filter(ord({"uint16": "H", "uint8": "B", "bool": "?"}[dtype]), work.ctypes.data, work.ctypes.data, w, h, n, rank, sx, sy,
                                   h if rows is None else rows) == 0
        assert same(work, want)


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

    n, h, w = 7, 67, 84
    arr = s1_noisy_background(n, h, w, seed=4)
    with IRMovie.from_filename(record(tmp_path / "m.h264", arr)) as mov:
        assert same(host(mov.window_median(3)), reference(np.asarray(mov.data), 4, 3, 3))
        for sel, size, rows in [(slice(None), 5, None), (slice(1, None, 2), (3, 5), h - 3), (3, 9, None), (slice(0, 0), 3, None)]:
            frames = mov.to_tensor(sel)
            sy, sx = (size, size) if isinstance(size, int) else size
            got = mov.window_median(size, sel, rows)
            assert got.dtype == torch.uint16 and got.shape == frames.shape and teq(got, D.window_median(frames, size, rows)), (sel, size)
            assert same(host(got), reference(host(frames), sy * sx // 2, sy, sx, rows))
            out = dev(np.full(tuple(got.shape), 12345, np.uint16))
            assert mov.window_median(size, selection=sel, rows=rows, out=out) is out and teq(out, got)
            assert teq(mov.rank_filter(1, size, sel, rows), D.rank_filter(frames, 1, size, rows))
        # pieces smaller than the selection give the same bits
        want = mov.rank_filter(-2, 5)
        mov._STATS_PIECE_BYTES = 3 * h * w * 2
        assert teq(mov.rank_filter(-2, 5), want)
        with pytest.raises(ValueError):
            mov.window_median(4)
        with pytest.raises(ValueError):
            mov.rank_filter(9, 3)
        with pytest.raises(RuntimeError):
            mov.window_median(3, out=torch.empty((n, h, w + 1), dtype=torch.uint16, device="cuda"))
