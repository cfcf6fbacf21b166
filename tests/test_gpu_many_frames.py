"""GPU: every stack entry on more frames than one grid dimension holds (many_frames_cases.py: 65 537 frames, frame i one of 7 distinct frames),
or at the largest count it accepts and the first it refuses.  The reference of the 7 distinct frames - the oracle, or the numpy reference of
the entry's own tests - never runs the kernel under test at that count; the long stack must repeat it bit for bit, and a mismatch names the
first frame that differs.

The entries treat the 65 535 blocks that the code takes for the most one of the grid's second and third dimensions holds in three ways, and
each test says which one it pins:
  WALK    the launcher walks the stack in pieces (morphology, reconstruct, distance_transform, temporal_median, the max-hold of downsample);
  REFUSE  the entry refuses more than 65 535 frames (the labelling entries, downsample's pair sums);
  DIRECT  the launcher passes the frame count into the grid as it is (the frame filters of filter_kernels.hip).

OBSERVED on the MI355X (gfx950) with the HIP runtime of ROCm 7.2: the runtime takes a DIRECT launch as it is.  Grids of 65 537 blocks in the
second or the third dimension - translate in all its forms, remove_motion, both gaussians in either order, the 3 x 3 median, the fused
chain with its repair launch and its tile list, BadPixels.correct and remove_inplace, split_planes and merge_planes - are launched without
an error and give the bits of the short stack in every frame: the 65 535 that the walking units cut their stacks at is not a limit of
this runtime.  Nothing in filter_kernels.hip had to change; the walks stay, as they cost one launch on any stack below the cut."""
import numpy as np
import pytest

import many_frames_cases as M
from many_frames_cases import N, P, assert_periodic, bits, periodic, to_device
from test_gpu_filters_full_range import gaussian_close, u16_as_kernels

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def ids(shapes):
    return ["%dx%d" % s for s in shapes]


def same_bits(t, a):
    """device tensor `t` holds the bits of numpy array `a`"""
    a = np.ascontiguousarray(a)
    return tuple(t.shape) == a.shape and t.element_size() == a.dtype.itemsize and torch.equal(bits(t), bits(to_device(a)))


@pytest.fixture
def reference_order(lib):
    lib.rir_set_gaussian_reference_order(1)
    yield
    lib.rir_set_gaussian_reference_order(0)


# ---- DIRECT: the frame filters ---------------------------------------------------------------------------------------------------------------


# (8-byte frames: the 2 x 2 frame only - 40 MB a tensor)
TRANSLATE_CASES = [(d, s) for d in (np.uint16, np.float32) for s in M.TRANSLATE_SHAPES] + [(np.float64, (2, 2))]


@pytest.mark.parametrize("dtype,shape", TRANSLATE_CASES, ids=["%s-%dx%d" % (np.dtype(d).name, s[0], s[1]) for d, s in TRANSLATE_CASES])
def test_translate(dev, oracle, dtype, shape):
    """DIRECT (launch_translate_t: gridDim.z = nframes).  Per-frame offsets, each strategy; the oracle bit for bit on the distinct frames."""
    h, w = shape
    frames, offsets = M.filter_frames(h, w, dtype), M.frame_offsets(h, w)
    long_frames, long_offsets = periodic(frames), periodic(offsets)
    for strategy in M.STRATEGIES:
        small = dev.translate(to_device(frames), to_device(offsets), strategy, background=M.BACKGROUND)
        assert same_bits(small, M.translate_reference(oracle, frames, offsets, strategy)), strategy
        assert_periodic(dev.translate(long_frames, long_offsets, strategy, background=M.BACKGROUND), small, "translate %s" % strategy)
    # one offset for all frames: the other reading of d_offsets
    small = dev.translate(to_device(frames), (0.3, -0.7), "nearest")
    assert same_bits(small, M.translate_reference(oracle, frames, [(0.3, -0.7)] * P, "nearest"))
    assert_periodic(dev.translate(long_frames, (0.3, -0.7), "nearest"), small, "translate, one offset")


@pytest.mark.parametrize("shape", M.TRANSLATE_SHAPES, ids=ids(M.TRANSLATE_SHAPES))
def test_translate_to_u16(dev, oracle, shape):
    """DIRECT (launch_translate_t<float, u16_via_f32>).  The oracle's float translate, truncated as the kernels truncate, bit for bit."""
    h, w = shape
    frames, offsets = M.filter_frames(h, w, np.float32), M.frame_offsets(h, w)
    long_frames, long_offsets = periodic(frames), periodic(offsets)
    for strategy in ("nearest", "background"):
        small = dev.translate_to_u16(to_device(frames), to_device(offsets), strategy, background=M.BACKGROUND)
        assert same_bits(small, u16_as_kernels(M.translate_reference(oracle, frames, offsets, strategy))), strategy
        assert_periodic(dev.translate_to_u16(long_frames, long_offsets, strategy, background=M.BACKGROUND), small, "translate_to_u16 %s" % strategy)


@pytest.mark.parametrize("shape", M.TRANSLATE_SHAPES, ids=ids(M.TRANSLATE_SHAPES))
def test_remove_motion(dev, oracle, shape):
    """DIRECT (launch_remove_motion: gridDim.z = nframes), per-frame shifts, rows < h: the last row is copied."""
    h, w = shape
    frames, shifts = M.filter_frames(h, w), M.frame_offsets(h, w)
    for rows in (h - 1, h):
        small = dev.remove_motion(to_device(frames), to_device(shifts), rows=rows)
        assert same_bits(small, np.stack([oracle.remove_motion(f, s[0], s[1], rows=rows) for f, s in zip(frames, shifts)])), rows
        assert_periodic(dev.remove_motion(periodic(frames), periodic(shifts), rows=rows), small, "remove_motion, rows %d" % rows)


GAUSS_CASES = [(r, s) for r in sorted(M.GAUSS_SHAPES) for s in M.GAUSS_SHAPES[r]]


def _gaussian_inputs(frames, sigma):
    """the float32 form, and the uint16 form where the entry takes it"""
    return (frames.astype(np.float32),) + ((frames,) if sigma < 2.5 else ())


@pytest.mark.parametrize("radius,shape", GAUSS_CASES, ids=["r%d-%dx%d" % (r, s[0], s[1]) for r, s in GAUSS_CASES])
def test_gaussian_filter(dev, oracle, radius, shape):
    """DIRECT (the separable wave-tile kernels: gridDim.z = nframes), float32 and uint16 frames; the distinct frames against the oracle by the
    rule of test_gaussian_full_range."""
    h, w = shape
    frames, sigma = M.filter_frames(h, w), M.SIGMAS[radius]
    want = np.stack([oracle.gaussian_filter(f.astype(np.float32), sigma) for f in frames])
    for x in _gaussian_inputs(frames, sigma):
        small = dev.gaussian_filter(to_device(x), sigma)
        assert gaussian_close(small.cpu().numpy(), want), x.dtype
        assert_periodic(dev.gaussian_filter(periodic(x), sigma), small, "gaussian_filter %s" % x.dtype)


@pytest.mark.parametrize("sigma,shape", M.DIRECT_GAUSS_CASES, ids=["s%g-%dx%d" % (g, s[0], s[1]) for g, s in M.DIRECT_GAUSS_CASES])
def test_gaussian_filter_in_reference_order(dev, oracle, reference_order, sigma, shape):
    """DIRECT (gaussian_kernel, the direct form every radius above 4 takes and, in the reference's order, every radius: gridDim.y = h,
    gridDim.z = nframes); bit for bit the oracle."""
    h, w = shape
    frames = M.filter_frames(h, w)
    want = np.stack([oracle.gaussian_filter(f.astype(np.float32), sigma) for f in frames])
    for x in _gaussian_inputs(frames, sigma):
        small = dev.gaussian_filter(to_device(x), sigma)
        assert same_bits(small, want), x.dtype
        assert_periodic(dev.gaussian_filter(periodic(x), sigma), small, "gaussian_filter in reference order, %s" % x.dtype)


@pytest.mark.parametrize("shape", M.MEDIAN_SHAPES, ids=ids(M.MEDIAN_SHAPES))
def test_median_filter(dev, oracle, shape):
    """DIRECT (the 3 x 3 median: gridDim.z = nframes)."""
    h, w = shape
    frames = M.filter_frames(h, w)
    small = dev.median_filter(to_device(frames))
    assert same_bits(small, np.stack([oracle.median_filter(f) for f in frames]))
    assert_periodic(dev.median_filter(periodic(frames)), small, "median_filter")


def _bad_pixels(dev, oracle, shape, rows=None):
    """-> (the BadPixels object of hot_first(shape), its list and its floor by the oracle): one flagged pixel at least"""
    first = M.hot_first(*shape)
    image = first if rows is None else first[:rows]
    xy, (_, fc) = oracle.bad_pixels_detect(image), oracle.bad_pixels_stats(image)
    bp = dev.BadPixels(to_device(first), rows=rows)
    assert len(xy) >= 1 and np.array_equal(bp.positions(), xy) and bp.floor_correct == fc
    return bp, xy, fc


@pytest.mark.parametrize("shape", M.BAD_PIXELS_SHAPES, ids=ids(M.BAD_PIXELS_SHAPES))
def test_bad_pixels_correct(dev, oracle, shape):
    """DIRECT (bad_pixels_correct: the clamp over the stack and bad_pixels_fix_kernel with gridDim.y = nframes)."""
    bp, xy, fc = _bad_pixels(dev, oracle, shape)
    frames = M.filter_frames(*shape)
    small = bp.correct(to_device(frames))
    assert same_bits(small, np.stack([oracle.bad_pixels_correct(f, xy, fc) for f in frames]))
    assert_periodic(bp.correct(periodic(frames)), small, "BadPixels.correct")
    bp.close()


@pytest.mark.parametrize("shape", M.BAD_PIXELS_SHAPES, ids=ids(M.BAD_PIXELS_SHAPES))
def test_bad_pixels_remove_inplace(dev, oracle, shape):
    """DIRECT (remove_bad_pixels_kernel: gridDim.y = nframes), in place, on the first h - 1 rows."""
    rows = shape[0] - 1
    bp, xy, _ = _bad_pixels(dev, oracle, shape, rows=rows)
    frames = M.filter_frames(*shape)
    small = bp.remove_inplace(to_device(frames), rows)
    assert same_bits(small, np.stack([oracle.remove_bad_pixels(f, xy, rows=rows) for f in frames]))
    assert_periodic(bp.remove_inplace(periodic(frames), rows), small, "BadPixels.remove_inplace")
    bp.close()


CHAIN_CASES = [(r, s) for r in sorted(M.CHAIN_SHAPES) for s in M.CHAIN_SHAPES[r]]


@pytest.mark.parametrize("radius,shape", CHAIN_CASES, ids=["r%d-%dx%d" % (r, s[0], s[1]) for r, s in CHAIN_CASES])
def test_filter_chain(dev, oracle, radius, shape):
    """DIRECT (launch_filter_chain: bad_pixels_fix_kernel with gridDim.y = nframes into the [nframes][nbad] scratch, then gridDim.z = nframes -
    radius 1: the regular kernel and the tile list the listed kernel works off; radius 2: filter_chain_kernel).  Per-frame offsets and a list
    of flagged pixels.  The distinct frames by the rule of
    test_filter_chain_equals_the_three_kernels: bit for bit the three entries one after the other, each checked against the oracle above."""
    h, w = shape
    frames, offsets, sigma = M.filter_frames(h, w), M.frame_offsets(h, w), M.SIGMAS[radius]
    bp = _bad_pixels(dev, oracle, shape)[0]
    for strategy in ("nearest", "background"):
        x, off = to_device(frames), to_device(offsets)
        three = dev.translate_to_u16(dev.gaussian_filter(bp.correct(x), sigma), off, strategy, background=M.BACKGROUND)
        small = dev.filter_chain(x, bp, sigma, off, strategy, background=M.BACKGROUND)
        assert torch.equal(bits(small), bits(three)), strategy
        assert_periodic(dev.filter_chain(periodic(frames), bp, sigma, periodic(offsets), strategy, background=M.BACKGROUND), small, "filter_chain %s" % strategy)
    bp.close()


@pytest.mark.parametrize("radius,shape", CHAIN_CASES, ids=["r%d-%dx%d" % (r, s[0], s[1]) for r, s in CHAIN_CASES])
def test_filter_chain_in_reference_order(dev, oracle, reference_order, radius, shape):
    """DIRECT, as test_filter_chain; in the reference's order the distinct frames are the oracle's chain bit for bit."""
    h, w = shape
    frames, offsets, sigma = M.filter_frames(h, w), M.frame_offsets(h, w), M.SIGMAS[radius]
    bp, xy, fc = _bad_pixels(dev, oracle, shape)
    want = np.stack([u16_as_kernels(oracle.translate(oracle.gaussian_filter(oracle.bad_pixels_correct(f, xy, fc).astype(np.float32), sigma), o[0], o[1], "nearest"))
                     for f, o in zip(frames, offsets)])
    small = dev.filter_chain(to_device(frames), bp, sigma, to_device(offsets), "nearest")
    assert same_bits(small, want)
    assert_periodic(dev.filter_chain(periodic(frames), bp, sigma, periodic(offsets), "nearest"), small, "filter_chain in reference order")
    bp.close()


@pytest.mark.parametrize("shape,linesize", M.PLANES_SHAPES, ids=["%dx%d" % s for s, _ in M.PLANES_SHAPES])
def test_split_and_merge_planes(dev, oracle, shape, linesize):
    """DIRECT (split_planes_kernel, merge_planes_kernel: gridDim.y = nframes), with the 8-bit image in Y."""
    h, w = shape
    frames, it = M.planes_frames(h, w)
    want = [np.stack(p) for p in zip(*[oracle.split_planes(f, linesize, i) for f, i in zip(frames, it)])]
    small = dev.split_planes(to_device(frames), linesize, to_device(it))
    long = dev.split_planes(periodic(frames), linesize, periodic(it))
    for name, s, l, o in zip("YUV", small, long, want):
        assert same_bits(s, o), name
        assert_periodic(l, s, "split_planes %s" % name)
    back = [np.stack(p) for p in zip(*[oracle.merge_planes(y, u, v, w, with_it=True) for y, u, v in zip(*want)])]
    assert np.array_equal(back[0], frames) and np.array_equal(back[1], it)
    for name, s, l, o in zip(("frames", "it"), dev.merge_planes(*small, w, with_it=True), dev.merge_planes(*long, w, with_it=True), back):
        assert same_bits(s, o), name
        assert_periodic(l, s, "merge_planes %s" % name)


# ---- WALK ----------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("dtype", M.MORPHOLOGY_DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("op,size,shape", M.MORPHOLOGY_CASES,
                         ids=["%s-%s-%dx%d" % (o, "x".join(map(str, M.sizes_of(z))), s[0], s[1]) for o, z, s in M.MORPHOLOGY_CASES])
def test_morphology(dev, op, size, shape, dtype):
    """WALK (for_frame_chunks: pieces of MAX_GRID_Z frames; in the pair kernels the frame comes out of tile_decode over an XCD-permuted id,
    here with more than one tile a frame).  erode, dilate and top_hat, rows = h - 1, against morphology_cases.reference."""
    import morphology_cases

    h, w = shape
    form = {"erode": dev.erode, "dilate": dev.dilate, "tophat": dev.top_hat}[op]
    frames = M.morphology_frames(h, w, dtype)
    small = form(to_device(frames), size, rows=h - 1)
    assert same_bits(small, morphology_cases.reference(frames, op, *M.sizes_of(size), rows=h - 1))
    assert_periodic(form(periodic(frames), size, rows=h - 1), small, "%s %s" % (op, size))


@pytest.mark.parametrize("rank,size,shape", M.RANK_CASES, ids=["rank%d-%d-%dx%d" % (r, z, s[0], s[1]) for r, z, s in M.RANK_CASES])
def test_rank_filter(dev, rank, size, shape):
    """WALK (for_frame_chunks; the register kernels decode the frame with tile_decode), with more than one tile a frame - what the 2 x 2 frames
    of test_gpu_rank_filter.py never have.  rows = h - 1, against rank_cases.reference."""
    import rank_cases

    h, w = shape
    frames = M.morphology_frames(h, w, np.uint16)
    small = dev.rank_filter(to_device(frames), rank, size, rows=h - 1)
    assert same_bits(small, rank_cases.reference(frames, rank, size, size, rows=h - 1))
    assert_periodic(dev.rank_filter(periodic(frames), rank, size, rows=h - 1), small, "rank_filter %d of %d x %d" % (rank, size, size))


@pytest.mark.parametrize("shape", M.LOCAL_SHAPES, ids=ids(M.LOCAL_SHAPES))
def test_local_stats_and_threshold(dev, shape):
    """WALK (for_frame_chunks, every output advanced by the piece), with more than one tile a frame.  The window mean and the z-score mask of
    uint8 frames, rows = h - 1, on the small frame the sums (of all its rows), against local_cases."""
    import local_cases

    h, w = shape
    frames = M.morphology_frames(h, w, np.uint8)
    long_frames = periodic(frames)
    small = dev.box_mean(to_device(frames), 3, rows=h - 1)
    assert same_bits(small, local_cases.reference_mean(frames, 3, 3, h - 1))
    assert_periodic(dev.box_mean(long_frames, 3, rows=h - 1), small, "box_mean")
    if shape != (2, 2):  # (the masks of 2 pixels are too few to tell 7 frames apart; test_gpu_local_stats.py has that frame)
        small = dev.local_threshold(to_device(frames), 3, rows=h - 1, **M.LOCAL_THRESHOLD)
        assert same_bits(small, local_cases.reference_mask(frames, 3, 3, rows=h - 1, **M.LOCAL_THRESHOLD))
        assert_periodic(dev.local_threshold(long_frames, 3, rows=h - 1, **M.LOCAL_THRESHOLD), small, "local_threshold")
    else:
        small, got = dev.local_stats(to_device(frames), 3, sumsq=True), dev.local_stats(long_frames, 3, sumsq=True)
        assert same_bits(small.sum, local_cases.reference_sums(frames, 3, 3).astype(np.int32))
        assert same_bits(small.sumsq, local_cases.reference_sums(frames, 3, 3, None, 2))
        assert_periodic(got.sum, small.sum, "local_stats sum")
        assert_periodic(got.sumsq, small.sumsq, "local_stats sumsq")


TYPE_CHAR = {"uint16": "H", "uint8": "B"}


def _reconstruct_entry(dev, mask, marker, mode, param, output, work_frames):
    """rir_reconstruct_device with a workspace of `work_frames` frames' share -> (result, rounds)"""
    import ctypes as ct

    n, h, w = mask.shape
    type_char = ord(TYPE_CHAR[str(mask.dtype).split(".")[1]])
    need = dev._lib.rir_reconstruct_workspace_bytes(type_char, w, h, 1) * work_frames
    work = torch.zeros(need // 8 + 1, dtype=torch.int64, device="cuda")
    out, rounds = torch.empty_like(mask), ct.c_int(-1)
    r = dev._lib.rir_reconstruct_device(type_char, mask.data_ptr(), None if marker is None else marker.data_ptr(), out.data_ptr(), w, h, n, 0, 8, mode, param,
                                        output, h, work.data_ptr(), need, ct.byref(rounds), dev._stream())
    assert r == 0, dev.last_error()
    return out, rounds.value


@pytest.mark.parametrize("shape", M.RECONSTRUCT_SHAPES, ids=ids(M.RECONSTRUCT_SHAPES))
def test_reconstruct(dev, shape):
    """WALK (groups of equal size, MAX_GRID_Z frames at most, then `mask + npx * o`; the flags of a group's frames in the workspace).  With a
    marker stack and as h_dome, against reconstruct_cases.reference; on the frames wider than a tile the corridor frame - the last frame of the
    long stack among them - needs a second round.  Then with a workspace of 3 frames' share: groups that are not the grid's limit."""
    import reconstruct_cases as RC

    mask, marker = M.reconstruct_frames(*shape)
    small, _ = dev.reconstruct(to_device(marker), to_device(mask), return_rounds=True)
    assert same_bits(small, RC.reference(mask, marker))
    dome = dev.h_dome(to_device(mask), M.H_DOME)
    assert same_bits(dome, RC.reference(mask, None, "dilation", 8, RC.SHIFT, M.H_DOME, 1))
    long_mask, long_marker = periodic(mask), periodic(marker)
    got, rounds = dev.reconstruct(long_marker, long_mask, return_rounds=True)
    assert_periodic(got, small, "reconstruct")
    if shape[1] > M.REC_TW:
        assert (N - 1) % P == M.CORRIDOR_AT and rounds >= 2
    assert_periodic(dev.h_dome(long_mask, M.H_DOME), dome, "h_dome")
    got, rounds3 = _reconstruct_entry(dev, long_mask, long_marker, RC.MARKER, 0, 0, 3)
    assert_periodic(got, small, "reconstruct in groups of 3")
    assert rounds3 == rounds
    assert_periodic(_reconstruct_entry(dev, long_mask, None, RC.SHIFT, M.H_DOME, 1, 3)[0], dome, "h_dome in groups of 3")


@pytest.mark.parametrize("border", [False, True], ids=["open", "border"])
@pytest.mark.parametrize("shape", M.DISTANCE_SHAPES, ids=ids(M.DISTANCE_SHAPES))
def test_distance_transform(dev, shape, border):
    """WALK (groups of equal size, 65 535 frames at most, dist2 and index advanced by the group).  With indices, rows = h - 1, against
    distance_cases.brute_force; then through the C entry with a workspace of 3 frames' share."""
    import distance_cases as DC

    h, w = shape
    masks = M.distance_frames(h, w)
    small = dev.distance_transform(to_device(masks), border=border, rows=h - 1, return_indices=True)
    for s, o in zip(small, DC.reference_stack(masks, 0, border, h - 1)):
        assert same_bits(s, o.astype(np.int32))
    long_masks = periodic(masks)
    for name, l, s in zip(("dist2", "index"), dev.distance_transform(long_masks, border=border, rows=h - 1, return_indices=True), small):
        assert_periodic(l, s, "distance_transform %s" % name)
    need = dev._lib.rir_distance_transform_workspace_bytes(w, h, 1, 1) * 3
    work = torch.zeros(need // 8 + 1, dtype=torch.int64, device="cuda")
    dist2, index = (torch.full((N, h, w), -7, dtype=torch.int32, device="cuda") for _ in range(2))
    r = dev._lib.rir_distance_transform_device(ord("B"), long_masks.data_ptr(), w, h, N, 0, int(border), h - 1, dist2.data_ptr(), index.data_ptr(), work.data_ptr(),
                                               need, dev._stream())
    assert r == 0, dev.last_error()
    assert_periodic(dist2, small[0], "distance_transform dist2 in groups of 3")
    assert_periodic(index, small[1], "distance_transform index in groups of 3")


def _temporal(dev, stack, what, **kw):
    """temporal_median of a host stack against the sliding median of the whole stack, on the device; the message names the first output"""
    got = dev.temporal_median(to_device(stack), **kw)
    want = to_device(M.sliding_median(stack, kw["window"], kw.get("threshold", 0), kw.get("rows"), kw.get("step", 1)))
    assert got.shape == want.shape
    if not torch.equal(bits(got), bits(want)):
        first = int((bits(got) != bits(want)).reshape(got.shape[0], -1).any(dim=1).nonzero()[0])
        raise AssertionError("%s: output %d of %d (frame %d, residue %d mod %d) is the first that differs" % (
            what, first, got.shape[0], first * kw.get("step", 1), first * kw.get("step", 1) % P, P))


def test_temporal_median_edge_outputs(dev):
    """WALK (temporal_median_edge in pieces of TM_GRID_Y outputs): step 2 sends every output through the edge kernel - 32 769 of them.  The frames
    are not independent: the stack is periodic along time and the reference is the sliding median of the whole 2 x 2 stack."""
    from test_temporal_median_cpu import temporal_median_oracle

    stack = M.host_periodic(M.temporal_distinct(2, 2), N)
    assert np.array_equal(M.sliding_median(stack[:40], 5, 300, 1, 2), temporal_median_oracle(stack[:40], 5, 300, 1, step=2))
    assert (N + 1) // 2 > M.TM_GRID_Y
    _temporal(dev, stack, "edge kernel", window=5, step=2)
    _temporal(dev, stack, "edge kernel, threshold and rows", window=5, step=2, threshold=20000, rows=1)


def test_temporal_median_runs(dev):
    """WALK (temporal_median_run in pieces of TM_GRID_Y runs): step 1, window 3, 1 x 2 frames - so few threads that a run is TM_RUN_MIN outputs -
    and more than TM_GRID_Y runs of them."""
    from test_temporal_median_cpu import temporal_median_oracle

    n = M.TEMPORAL_RUN_FRAMES
    stack = M.host_periodic(M.temporal_distinct(1, 2), n)
    assert np.array_equal(M.sliding_median(stack[:40], 3), temporal_median_oracle(stack[:40], 3))
    assert (n - 2 + M.TM_RUN_MIN - 1) // M.TM_RUN_MIN > M.TM_GRID_Y
    _temporal(dev, stack, "run kernel", window=3)
    _temporal(dev, stack, "run kernel, threshold", window=3, threshold=20000)
    two_rows = M.host_periodic(M.temporal_distinct(2, 1), n)
    _temporal(dev, two_rows, "run kernel, rows", window=3, rows=1)


def test_downsample_more_segments_than_one_launch(dev):
    """WALK (ds_max_hold in pieces of 65 535 segments, the segment list advanced by the piece): one push whose kept images - one segment each -
    are N, against downsample_cases.oracle."""
    import downsample_cases as DC

    frames, stamps, want = M.downsample_case()
    assert len(want.positions) == N
    got = dev.downsample(to_device(frames), stamps, lossy_height=1, **M.DOWNSAMPLE)
    assert np.array_equal(got.positions, want.positions) and np.array_equal(got.timestamps, want.timestamps)
    assert DC.bits(got.stats).tolist() == DC.bits(want.stats).tolist()
    images = to_device(want.images)
    if not torch.equal(bits(got.frames), bits(images)):
        first = int((bits(got.frames) != bits(images)).reshape(N, -1).any(dim=1).nonzero()[0])
        raise AssertionError("kept image %d of %d is the first that differs" % (first, N))


def test_downsample_refuses_more_frames_than_the_pair_sums_take(dev):
    """REFUSE (launch_pair_sums: 65 535 slabs of DS_SLAB frames at most): the first count past it is an error that names the limit, before any
    device work."""
    n = 65535 * M.DS_SLAB + 1
    frames = torch.zeros((n, 1, 2), dtype=torch.uint16, device="cuda")
    d = dev.Downsampler(2, 1, 2, 0.5)
    with pytest.raises(RuntimeError, match=str(65535 * M.DS_SLAB)):
        d.push(frames, np.arange(n, dtype=np.int64))
    assert d.count == 0
    small = d.push(frames[:5], np.arange(5, dtype=np.int64))  # (the refused push left the stream as it was)
    assert small.positions.tolist() == [0, 2, 4]
    d.close()


# ---- the region reducers: one-dimensional grids over work items, outputs [n][K] ----------------------------------------------------------------


def _fields(result):
    return {k: v for k, v in result._asdict().items() if isinstance(v, torch.Tensor)}


@pytest.mark.parametrize("maps", ["shared", "per-frame"])
def test_region_reducers(dev, maps):
    """region_stats, region_geometry, region_histogram, histogram and region_quantiles (grids over work items, not over frames; every output
    is [n][regions]) on N frames of 3 x 5 with 4 regions, against the oracles of the test_region_*_cpu modules."""
    frames, labels = M.region_case(maps == "per-frame")
    want = M.region_references(frames, labels)
    r = M.REGIONS
    calls = {"region_stats": lambda f, l: dev.region_stats(f, l, r["k"]), "region_geometry": lambda f, l: dev.region_geometry(l, r["k"], f),
             "region_histogram": lambda f, l: dev.region_histogram(f, l, r["nbins"], r["lo"], r["width"], r["k"], rows=r["h"] - 1),
             "histogram": lambda f, l: dev.histogram(f, r["nbins"], r["lo"], r["width"], rows=r["h"] - 1),
             "region_quantiles": lambda f, l: dev.region_quantiles(f, l, r["percents"], r["k"])}
    long_frames = periodic(frames)
    long_labels = periodic(labels) if maps == "per-frame" else to_device(labels)
    for name, call in calls.items():
        small, got = _fields(call(to_device(frames), to_device(labels))), _fields(call(long_frames, long_labels))
        assert set(small) == set(want[name]) == set(got), name
        for field in small:
            assert same_bits(small[field], want[name][field]), (name, field)
            assert_periodic(got[field], small[field], "%s.%s, %s map" % (name, field, maps))


# ---- REFUSE: the labelling entries -------------------------------------------------------------------------------------------------------------
SENTINEL = -7


def test_label_images_and_keep_largest_areas_at_the_largest_count(dev, oracle):
    """REFUSE, the accepted side: 65 535 frames (blockIdx.y up to 65 534) of 2 x 3, against oracle.label_image and oracle.keep_largest_area."""
    frames = M.label_frames()
    want = M.label_references(oracle, frames)
    cap = frames[0].size + 1
    long_frames = periodic(frames, M.LABEL_FRAMES)
    small, got = dev.label_images(to_device(frames), 0, table_entries=cap), dev.label_images(long_frames, 0, table_entries=cap)
    for name, s, g, o in zip(("labels", "area", "xy", "counts"), small, got, want):
        assert same_bits(s, o), name
        assert_periodic(g, s, "label_images %s" % name)
    largest = dev.keep_largest_areas(to_device(frames), 0, 6)
    assert same_bits(largest, want[4])
    assert_periodic(dev.keep_largest_areas(long_frames, 0, 6), largest, "keep_largest_areas")


def test_label_hot_spots_at_the_largest_count(dev):
    """REFUSE, the accepted side: 65 535 frames of 2 x 3, against hot_spot_cases.oracle."""
    import hot_spot_cases

    frames = M.hot_spot_frames()
    want = hot_spot_cases.oracle(frames, **M.HOT_SPOTS)
    small, got = dev.label_hot_spots(to_device(frames), **M.HOT_SPOTS), dev.label_hot_spots(periodic(frames, M.LABEL_FRAMES), **M.HOT_SPOTS)
    for name, s, g in zip(("labels", "area", "first", "counts"), small, got):
        assert same_bits(s, want[name]), name
        assert_periodic(g, s, "label_hot_spots %s" % name)


def test_labelling_refuses_the_first_count_past_the_limit(dev):
    """REFUSE, the refused side: 65 536 frames.  The Python forms raise before any output exists; the C entries return an error and leave
    outputs filled with a sentinel as they were."""
    n = M.LABEL_FRAMES + 1
    h, w = M.LABEL_SHAPE
    frames = periodic(M.label_frames(), n)
    for call in (lambda: dev.label_images(frames), lambda: dev.keep_largest_areas(frames), lambda: dev.label_hot_spots(frames, **M.HOT_SPOTS)):
        with pytest.raises(RuntimeError, match="refused"):
            call()
    lib, cap = dev._lib, h * w + 1
    assert lib.rir_label_workspace_bytes_batch(w, h, n) == 0 and lib.rir_label_hot_spots_workspace_bytes(w, h, n) == 0
    need = max(lib.rir_label_workspace_bytes_batch(w, h, n - 1), lib.rir_label_hot_spots_workspace_bytes(w, h, n - 1))
    assert need > 0
    work = torch.zeros(need // 8 + 1, dtype=torch.int64, device="cuda")
    dst, area, count = (torch.full(s, SENTINEL, dtype=torch.int32, device="cuda") for s in ((n, h, w), (n, cap), (n,)))
    first = torch.full((n, cap), SENTINEL, dtype=torch.int32, device="cuda")
    xy = torch.full((n, cap, 2), float(SENTINEL), dtype=torch.float64, device="cuda")
    back = np.zeros(1, np.uint16)
    untouched = lambda: all(bool((t == SENTINEL).all()) for t in (dst, area, count, first, xy))  # noqa: E731
    assert lib.rir_label_images_device(ord("H"), frames.data_ptr(), dst.data_ptr(), w, h, n, back.ctypes.data, xy.data_ptr(), area.data_ptr(), cap, count.data_ptr(),
                                       work.data_ptr(), work.numel() * 8, dev._stream()) != 0
    assert untouched()
    assert lib.rir_keep_largest_areas_device(ord("H"), frames.data_ptr(), dst.data_ptr(), w, h, n, back.ctypes.data, 6, work.data_ptr(), work.numel() * 8,
                                             dev._stream()) != 0
    assert untouched()
    _, _, _, spec = dev._label_hot_spots_args((n, h, w), **M.HOT_SPOTS)
    assert lib.rir_label_hot_spots_device(frames.data_ptr(), w, h, n, spec.rows, spec.low, None, int(spec.use_high), spec.high, None, spec.min_area, spec.max_area,
                                          int(spec.clear_border), dst.data_ptr(), first.data_ptr(), area.data_ptr(), cap, count.data_ptr(), work.data_ptr(),
                                          work.numel() * 8, dev._stream()) != 0
    assert untouched()
