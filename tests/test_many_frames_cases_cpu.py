"""CPU: the cases of many_frames_cases.py do what test_gpu_many_frames.py needs of them - no piece size of the units is a multiple of the period
of the long stack, and the references of the P distinct frames of every entry differ pairwise, so a frame taken from the wrong place of the
stack shows; the shapes put a second tile on each axis; the downsample stack gives exactly N segments."""
import numpy as np
import pytest

import many_frames_cases as M
from many_frames_cases import N, P, pairwise_different


def test_no_piece_size_is_a_multiple_of_the_period():
    limits = M.grid_limits()
    assert sorted(set(limits.values())) == [32768, 65535]
    assert M.MAX_GRID_Z == 65535 and M.TM_GRID_Y == 32768
    for s in sorted(set(limits.values()) | {65536, 3}):  # (65 536: an index cut to 16 bits; 3: the groups of the small workspaces)
        assert s % P != 0, s
    assert N > max(limits.values()) and M.LABEL_FRAMES == 65535
    # the groups of equal size that reconstruct and distance_transform cut N frames into, and the last frame of the long stack
    assert (N + 1) // 2 % P != 0 and (N - 1) % P == M.CORRIDOR_AT


def test_the_shapes_put_a_second_tile_on_each_axis():
    assert (M.TR_TY, M.GAUSS_TY, M.CHAIN_TY, M.MEDIAN_TY, M.MORPH_TY) == (16, 16, 16, 16, 16)
    assert (M.G_TW, M.G_TH, M.REC_TW, M.REC_TH, M.DISTANCE_ROWS) == (64, 32, 64, 32, 4)
    assert M.TRANSLATE_SHAPES == [(2, 2), (2, 64), (65, 2)]
    assert M.GAUSS_SHAPES == {1: [(2, 2), (2, 63), (65, 2)], 2: [(2, 2), (2, 61), (65, 2)]}
    assert M.MEDIAN_SHAPES == [(3, 3), (3, 61), (65, 3)]
    assert M.CHAIN_SHAPES == {1: [(2, 2), (2, 61), (57, 2)], 2: [(2, 2), (2, 59), (57, 2)]}
    assert M.morph_pair_shapes(3) == [(2, 2), (2, 126), (65, 2)] and M.morph_pair_shapes(7, 2) == [(2, 2), (2, 118), (65, 2)]
    assert M.MORPH_GENERAL_SHAPES == [(2, 3), (2, 65), (33, 3)] and M.RECONSTRUCT_SHAPES == [(2, 2), (1, 65)]
    assert M.DISTANCE_SHAPES == [(3, 3), (2, 65), (6, 2)]
    # no tensor above about 40 MB: the widest item of each entry's inputs and outputs
    for item, shapes in ((4, M.TRANSLATE_SHAPES), (2, M.MEDIAN_SHAPES), (2, [s for _, _, s in M.MORPHOLOGY_CASES]), (4, M.DISTANCE_SHAPES), (2, M.BAD_PIXELS_SHAPES),
                         (4, sum(M.GAUSS_SHAPES.values(), [])), (4, sum(M.CHAIN_SHAPES.values(), [])), (4, [s for _, s in M.DIRECT_GAUSS_CASES]), (2, M.RECONSTRUCT_SHAPES)):
        for h, w in shapes:
            assert N * h * w * item <= 42 << 20, (h, w, item)
    assert M.TEMPORAL_RUN_FRAMES == M.TM_GRID_Y * M.TM_RUN_MIN + 2 * M.TM_RUN_MIN + 3 == 262163


def test_the_helpers_of_the_comparison():
    assert pairwise_different([np.zeros(3), np.ones(3)]) and not pairwise_different([np.zeros(3), np.ones(3), np.zeros(3)])
    assert pairwise_different([(np.zeros(2), np.ones(1)), (np.zeros(2), np.zeros(1))])
    assert M.host_periodic(np.arange(P), 16).tolist() == [i % P for i in range(16)]


# ---- the references of the P distinct frames differ pairwise ----------------------------------------------------------------------------------


@pytest.mark.parametrize("shape", M.TRANSLATE_SHAPES)
@pytest.mark.parametrize("dtype", [np.uint16, np.float32, np.float64])
def test_translate_references_differ(oracle, dtype, shape):
    frames, offsets = M.filter_frames(*shape, dtype), M.frame_offsets(*shape)
    assert pairwise_different(frames) and pairwise_different(offsets)
    for strategy in M.STRATEGIES:
        assert pairwise_different(M.translate_reference(oracle, frames, offsets, strategy)), strategy
    assert pairwise_different(M.translate_reference(oracle, frames, [(0.3, -0.7)] * P, "nearest"))
    if dtype == np.uint16:
        for rows in (shape[0] - 1, shape[0]):
            assert pairwise_different([oracle.remove_motion(f, s[0], s[1], rows=rows) for f, s in zip(frames, offsets)]), rows


def test_gaussian_median_and_planes_references_differ(oracle):
    for radius, shapes in M.GAUSS_SHAPES.items():
        for shape in shapes + [s for _, s in M.DIRECT_GAUSS_CASES]:
            for sigma in (M.SIGMAS[radius], 3.3):
                assert pairwise_different([oracle.gaussian_filter(f.astype(np.float32), sigma) for f in M.filter_frames(*shape)]), (shape, sigma)
    for shape in M.MEDIAN_SHAPES:
        assert pairwise_different([oracle.median_filter(f) for f in M.filter_frames(*shape)]), shape
    for shape, linesize in M.PLANES_SHAPES:
        frames, it = M.planes_frames(*shape)
        assert pairwise_different([oracle.split_planes(f, linesize, i) for f, i in zip(frames, it)]), shape


def test_bad_pixel_and_chain_references_differ(oracle):
    from test_gpu_filters_full_range import u16_as_kernels

    for shape in M.BAD_PIXELS_SHAPES:
        frames, first = M.filter_frames(*shape), M.hot_first(*shape)
        xy, (_, fc) = oracle.bad_pixels_detect(first), oracle.bad_pixels_stats(first)
        assert len(xy) >= 1 and pairwise_different([oracle.bad_pixels_correct(f, xy, fc) for f in frames]), shape
        xy = oracle.bad_pixels_detect(first[:shape[0] - 1])
        assert len(xy) >= 1 and pairwise_different([oracle.remove_bad_pixels(f, xy, rows=shape[0] - 1) for f in frames]), shape
    assert len(oracle.bad_pixels_detect(M.hot_first(*M.BAD_PIXELS_SHAPES[-1]))) > 64  # more than one workgroup of the repair
    for radius, shapes in M.CHAIN_SHAPES.items():
        for shape in shapes:
            frames, offsets, first = M.filter_frames(*shape), M.frame_offsets(*shape), M.hot_first(*shape)
            xy, (_, fc) = oracle.bad_pixels_detect(first), oracle.bad_pixels_stats(first)
            assert len(xy) >= 1
            for strategy in ("nearest", "background"):
                chain = [u16_as_kernels(oracle.translate(oracle.gaussian_filter(oracle.bad_pixels_correct(f, xy, fc).astype(np.float32), M.SIGMAS[radius]), o[0], o[1],
                                                         strategy, background=M.BACKGROUND)) for f, o in zip(frames, offsets)]
                assert pairwise_different(chain), (shape, strategy)


@pytest.mark.parametrize("dtype", M.MORPHOLOGY_DTYPES, ids=lambda d: np.dtype(d).name)
def test_morphology_references_differ(dtype):
    import morphology_cases

    for op, size, shape in M.MORPHOLOGY_CASES:
        frames = M.morphology_frames(*shape, dtype)
        assert pairwise_different(morphology_cases.reference(frames, op, *M.sizes_of(size), rows=shape[0] - 1)), (op, size, shape)


def test_rank_and_local_references_differ():
    import local_cases
    import rank_cases

    assert (M.RT_TW, M.RT_TH, M.LOCAL_TY, M.LOCAL_HL) == (64, 32, 16, 4)
    for rank, size, shape in M.RANK_CASES:
        frames = M.morphology_frames(*shape, np.uint16)
        assert pairwise_different(rank_cases.reference(frames, rank, size, size, rows=shape[0] - 1)), (rank, size, shape)
    for shape in M.LOCAL_SHAPES:
        frames = M.morphology_frames(*shape, np.uint8)
        assert pairwise_different(local_cases.reference_mean(frames, 3, 3, shape[0] - 1)), shape
        if shape != (2, 2):
            assert pairwise_different(local_cases.reference_mask(frames, 3, 3, rows=shape[0] - 1, **M.LOCAL_THRESHOLD)), shape
    frames = M.morphology_frames(2, 2, np.uint8)
    assert pairwise_different(local_cases.reference_sums(frames, 3, 3)) and pairwise_different(local_cases.reference_sums(frames, 3, 3, None, 2))


@pytest.mark.parametrize("shape", M.RECONSTRUCT_SHAPES)
def test_reconstruct_references_differ(shape):
    import reconstruct_cases as RC

    mask, marker = M.reconstruct_frames(*shape)
    iterations = []
    assert pairwise_different(RC.reference(mask, marker, iterations=iterations))
    assert pairwise_different(RC.reference(mask, None, "dilation", 8, RC.SHIFT, M.H_DOME, 1))
    if shape[1] > M.REC_TW:  # the corridor: the plain iteration walks its whole width, the kernel meets a tile edge on the way
        assert iterations[M.CORRIDOR_AT] >= M.REC_TW


@pytest.mark.parametrize("shape", M.DISTANCE_SHAPES)
def test_distance_references_differ(shape):
    import distance_cases as DC

    masks = M.distance_frames(*shape)
    for border in (False, True):
        dist2, index = DC.reference_stack(masks, 0, border, shape[0] - 1)
        assert pairwise_different(list(zip(dist2, index))), border


def test_temporal_references_differ_and_the_sliding_median_is_the_oracle():
    from test_temporal_median_cpu import temporal_median_oracle

    for (h, w), kw in (((2, 2), dict(window=5, step=2)), ((2, 2), dict(window=5, step=2, threshold=20000, rows=1)), ((1, 2), dict(window=3)),
                       ((1, 2), dict(window=3, threshold=20000)), ((2, 1), dict(window=3, rows=1))):
        stack = M.host_periodic(M.temporal_distinct(h, w), 61)
        want = temporal_median_oracle(stack, **kw)
        assert np.array_equal(M.sliding_median(stack, kw["window"], kw.get("threshold", 0), kw.get("rows"), kw.get("step", 1)), want)
        # the outputs of the frames of one period, away from the ends
        step = kw.get("step", 1)
        assert pairwise_different(want[14 // step:14 // step + P]), kw
    assert (N + 1) // 2 > M.TM_GRID_Y and (M.TEMPORAL_RUN_FRAMES - 2 + M.TM_RUN_MIN - 1) // M.TM_RUN_MIN > M.TM_GRID_Y


def test_downsample_case_gives_exactly_n_segments():
    frames, stamps, want = M.downsample_case()
    assert frames.shape[1:] == (1, 8) and len(want.positions) == N > 65535
    assert want.keep[-1] and (np.diff(stamps) > 0).all()
    assert int((~want.keep).sum()) == len(frames) - N > 0  # some images are merged into the next kept one
    # kept images one piece of 65 535 apart differ: a segment list read one piece off shows
    assert (want.images[65535:, 0, 0] != want.images[:N - 65535, 0, 0]).all()
    assert M.DS_SLAB == 64


def test_region_references_differ():
    for per_frame in (0, 1):
        frames, labels = M.region_case(per_frame)
        assert labels.shape == ((P, 3, 5) if per_frame else (3, 5))
        for name, fields in M.region_references(frames, labels).items():
            assert pairwise_different(list(zip(*fields.values()))), (name, per_frame)


def test_labelling_references_differ(oracle):
    import hot_spot_cases

    labels, area, xy, counts, largest = M.label_references(oracle, M.label_frames())
    assert pairwise_different(labels) and pairwise_different(list(zip(labels, area, xy))) and sorted(set(counts.tolist())) == [1, 2, 3, 4]
    assert len({a.tobytes() for a in largest}) >= 5  # (the largest area of several frames is the same pixels)
    o = hot_spot_cases.oracle(M.hot_spot_frames(), **M.HOT_SPOTS)
    assert pairwise_different(list(zip(o["labels"], o["area"], o["first"]))) and sorted(set(o["counts"].tolist())) == [1, 2, 3]
