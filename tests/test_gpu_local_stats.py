"""GPU: local window statistics and the z-score mask, bit for bit against the numpy reference of local_cases.py (checked against scipy in
test_local_stats_cpu.py) - types, shapes, sizes and output sets over the pair and the general kernel, the values that overflow 32 bits, the
rounding of the mean, the mask over polarities, k, delta and scenes with exact ties, the rows rule, long stacks, layouts, out=, the host
entries and recordings through IRMovie."""
import ctypes as ct

import numpy as np
import pytest

from local_cases import (DELTAS, DTYPES, KS, OUTPUTS, POLARITIES, SHAPES, SIZES, checkerboard, noise, ramp, reference_mask, reference_mean, reference_sums,
                         sizes_of)
from morphology_cases import spike_images, type_max

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).cuda().view(torch.uint16)
    return torch.from_numpy(a).cuda()


def host(t):
    if t is None:
        return None
    if t.dtype == torch.uint16:
        return t.cpu().view(torch.int16).numpy().view(np.uint16)
    return t.cpu().numpy()


def same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)


def teq(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(host(a), host(b))


def stats(stack, size, **kw):
    """device.local_stats on a numpy stack -> (sum, sumsq, mean) as numpy arrays or None"""
    from librir_amd import device as D

    got = D.local_stats(dev(stack), size, **kw)
    assert got.n == np.prod(sizes_of(size))
    return host(got.sum), host(got.sumsq), host(got.mean)


def mask_of(stack, size, k, delta=0, polarity="above", **kw):
    from librir_amd import device as D

    got = D.local_threshold(dev(stack), size, k, delta, polarity, **kw)
    assert got.dtype == torch.bool
    return host(got)


def wanted(stack, size, rows=None):
    """the three reference arrays of a stack, in the types of the outputs"""
    sy, sx = sizes_of(size)
    return (reference_sums(stack, sy, sx, rows).astype(np.int32), reference_sums(stack, sy, sx, rows, power=2), reference_mean(stack, sy, sx, rows))


def check_stats(stack, size, rows=None, outputs=OUTPUTS):
    want = wanted(stack, size, rows)
    for asked in outputs:
        got = stats(stack, size, rows=rows, **asked)
        for g, w, name in zip(got, want, ("sum", "sumsq", "mean")):
            assert (g is None) == (not asked[name]), (size, asked, name)
            assert g is None or same(g, w), (size, asked, name)


def full_range(rng, h, w, dtype):
    """random over the full range, two frames; the second one with 0 and the type's maximum along its borders"""
    top = type_max(dtype)
    stack = rng.integers(0, top + 1, (2, h, w)).astype(dtype)
    stack[1, 0, :], stack[1, -1, :] = top, 0
    stack[1, :, 0], stack[1, :, -1] = 0, top
    return stack


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("h,w", SHAPES, ids=lambda v: str(v))
def test_types_shapes_sizes_and_outputs(dtype, h, w):
    """every size and every set of outputs; the outputs of one call equal those of separate calls (each is compared with the same reference)"""
    stack = full_range(np.random.default_rng(h * 131 + w), h, w, np.dtype(dtype).type)
    for size in SIZES:
        check_stats(stack, size)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_window_larger_than_the_image(dtype):
    stack = full_range(np.random.default_rng(56), 5, 6, np.dtype(dtype).type)
    check_stats(stack, 15)
    check_stats(stack[:, :, :5], 15)
    check_stats(stack[:, :1, :1], 15)


def test_values_that_overflow_32_bits():
    """an all-65535 frame at 15 x 15: S = 14 745 375 and Q = 966 338 150 625 everywhere; the 0 / 65535 checkerboard; one 0 in 65535 and one
    65535 in 0 at the nine corner / edge / interior positions"""
    full = np.full((1, 33, 66), 65535, np.uint16)
    s, q, m = stats(full, 15, sumsq=True, mean=True)
    assert (s == 14745375).all() and (q == 966338150625).all() and (m == 65535).all() and s.dtype == np.int32 and q.dtype == np.int64
    spikes = spike_images(17, 66, np.uint16)
    spikes[:9][spikes[:9] != 65535] = 0
    spikes[9:][spikes[9:] != 0] = 65535
    board = np.stack([checkerboard(17, 66, np.uint16), checkerboard(17, 66, np.uint16, 1)])
    for stack in (board, spikes, board[:, :, :65], spikes[:, :9, :11]):
        for size in (15, 3, (15, 1), (1, 15), 9):
            check_stats(stack, size, outputs=OUTPUTS[3:])
    for dtype in (np.uint8, np.bool_):
        top = np.full((1, 17, 66), type_max(dtype)).astype(dtype)
        s, q, m = stats(top, 15, sumsq=True, mean=True)
        assert (s == 225 * type_max(dtype)).all() and (q == 225 * type_max(dtype) ** 2).all() and (m == top).all()
        check_stats(np.stack([checkerboard(17, 66, dtype), checkerboard(17, 66, dtype, 1)]), 15, outputs=OUTPUTS[3:])


@pytest.mark.parametrize("dtype", DTYPES)
def test_mean_rounding(dtype):
    """pixels of 1 on 0, and of q + 1 on q: windows whose sum is n // 2 short of a multiple of n (n q + n // 2 + 1: rounds up), n // 2 above
    one (rounds down), equal to one, and everything between; the mean of a constant frame is the constant for every size"""
    from librir_amd import device as D

    np_type = np.dtype(dtype).type
    rng = np.random.default_rng(11)
    base = (rng.random((4, 19, 66)) < np.array([0.5, 0.2, 0.8, 0.0])[:, None, None]).astype(np.int64)
    base[3, 9, 30], base[3, 9, 31], base[3, 10, 30] = 1, 1, 1  # three pixels of 1: most windows sum to a multiple of n exactly
    levels = [0] if dtype == "bool" else [0, 7, type_max(np_type) - 1]
    for size in (3, 5, (3, 5), 15, (1, 3)):
        sy, sx = sizes_of(size)
        n = sy * sx
        for q in levels:
            stack = (base + q).astype(np_type)
            sums = reference_sums(stack, sy, sx)
            rest = set(np.unique((sums - n * q)).tolist())
            assert {0, n // 2, n // 2 + 1} <= rest, (size, sorted(rest))  # a multiple of n, and both sides of the half above it
            want = reference_mean(stack, sy, sx)
            assert set(np.unique(want.astype(np.int64)).tolist()) == {q, q + 1}
            assert same(host(D.box_mean(dev(stack), size)), want), (size, q)
    for size in SIZES:
        for value in sorted({0, 1, type_max(np_type) // 3, type_max(np_type)}):
            flat = np.full((1, 9, 66), value).astype(np_type)
            assert same(host(D.box_mean(dev(flat), size)), flat) and same(host(D.box_mean(dev(flat[:, :, :11]), size)), flat[:, :, :11])


def scenes(dtype, h=21, w=66):
    """noise whose level rises across the frame, the spike frames, a constant frame of 0, the checkerboard, a ramp, and the S1 background with a
    few planted spots"""
    from librir_amd.synthetic import s1_noisy_background

    rng = np.random.default_rng(h * w)
    top = type_max(dtype)
    s1 = s1_noisy_background(2, h, w, seed=9)
    for y, x, lift in ((3, 5, 3000), (10, 40, 800), (h - 1, w - 1, 10000), (0, 33, 2100), (12, 12, 20)):  # (the background spreads over 0..1000)
        s1[:, y, x] += lift
    s1 = np.minimum(s1 // (40 if top == 255 else 1), top).astype(dtype) if top > 1 else (s1 > 500)
    frames = [noise(rng, h, w, dtype)[None], noise(rng, h, w, dtype, spread=3)[None], spike_images(h, w, dtype), np.zeros((1, h, w), dtype),
              checkerboard(h, w, dtype)[None], ramp(h, w, dtype)[None], s1]
    return np.concatenate(frames)


def mask_from(stack, S, Q, n, k, delta, polarity):
    """reference_mask's rule on sums computed once (int64: every product fits, test_local_stats_cpu.py)"""
    num, den = (k if isinstance(k, tuple) else (k, 1))
    d = n * stack.astype(np.int64) - S
    V = n * Q - S * S
    up, down = d > delta * n, -d > delta * n
    return (d * d * (den * den) > (num * num) * V) & (up if polarity == "above" else down if polarity == "below" else up | down)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("size,width", [(3, 66), (9, 66), ((7, 15), 66), (5, 65)], ids=str)
def test_mask_over_polarity_k_delta_and_scenes(dtype, size, width):
    stack = scenes(np.dtype(dtype).type)[:, :, :width]
    sy, sx = sizes_of(size)
    S, Q = reference_sums(stack, sy, sx), reference_sums(stack, sy, sx, power=2)
    d = dev(stack)
    from librir_amd import device as D

    hot = 0
    for polarity in POLARITIES:
        for k in KS:
            for delta in DELTAS:
                want = mask_from(stack, S, Q, sy * sx, k, delta, polarity)
                got = host(D.local_threshold(d, size, k, delta, polarity))
                assert same(got, want), (polarity, k, delta, int((got != want).sum()))
                hot += int(want.sum())
    assert hot > 0
    assert same(mask_from(stack, S, Q, sy * sx, (5, 2), 1, "both"), reference_mask(stack, sy, sx, (5, 2), 1, "both"))
    assert not mask_of(stack, size, 0, 0, "both")[20].any()  # the constant frame: d = 0 and V = 0
    if dtype != "bool" and width == 66:  # k = 0: above the local mean by more than delta, whatever the spread
        want = np.stack([stack[i].astype(np.int64) * sy * sx - S[i] > 20 * sy * sx for i in range(len(stack))])
        assert same(mask_of(stack, size, 0, 20), want)


def test_mask_at_the_limits_of_int64():
    """the scenes with the largest d and V at 15 x 15 with k = 255 / 64 and 255: the reference in Python integers"""
    spikes = spike_images(17, 34, np.uint16)
    spikes[:9][spikes[:9] != 65535] = 0
    spikes[9:][spikes[9:] != 0] = 65535
    stack = np.concatenate([spikes, checkerboard(17, 34, np.uint16)[None], checkerboard(17, 34, np.uint16, 1)[None]])
    for k in ((255, 64), (255, 1), (1, 64), (3, 1)):
        for polarity, delta in (("above", 0), ("below", 0), ("both", -65535), ("both", 65535), ("above", 30000)):
            want = reference_mask(stack, 15, 15, k, delta, polarity, exact=True)
            assert same(mask_of(stack, 15, k, delta, polarity), want), (k, polarity, delta)
            assert same(mask_of(stack[:, :, :33], (15, 3), k, delta, polarity), reference_mask(stack[:, :, :33], 15, 3, k, delta, polarity, exact=True))


@pytest.mark.parametrize("dtype,a", [("uint16", 65535), ("uint16", 3), ("uint8", 255), ("bool", 1)])
def test_ties_are_not_hot(dtype, a):
    """d^2 den^2 == num^2 V exactly, where strict means 0.  A window of n cells with m cells of `a` (the pixel itself among them) on 0 has d =
    (n - m) a and V = m (n - m) a^2 at such a pixel, so equality is (n - m) den^2 == m num^2:
      1 x 5, m = 1: d = 4a, V = 4a^2 - a tie at k = 2 / 1 (and 4 / 2, 128 / 64);
      5 x 5, m = 5 (a plus sign): d = 20a, V = 100a^2 - a tie at k = 2 / 1 too; at a 0 pixel of that window d = -5a, V = 100a^2: k = 1 / 2
      (polarity below).
    One step of k below the tie is hot, the tie and everything above it are not."""
    np_type = np.dtype(dtype).type
    img = np.zeros((1, 21, 66), np_type)
    img[0, 10, 20] = a  # alone in its 1 x 5 windows
    for y, x in ((10, 40), (9, 40), (11, 40), (10, 39), (10, 41)):  # the plus sign
        img[0, y, x] = a
    for size, (y, x) in (((1, 5), (10, 20)), (5, (10, 40))):
        sy, sx = sizes_of(size)
        for k, hot in (((2, 1), False), ((4, 2), False), ((128, 64), False), ((127, 64), True), ((1, 1), True), ((3, 1), False), ((129, 64), False)):
            got = mask_of(img, size, k)
            assert same(got, reference_mask(img, sy, sx, k, exact=True)) and got[0, y, x] == hot, (size, k)
    # (11, 41): a 0 whose 5 x 5 window holds the five pixels of the plus sign
    for k, hot in (((1, 2), False), ((32, 64), False), ((31, 64), True), ((0, 1), True), ((1, 1), False)):
        got = mask_of(img, 5, k, polarity="below")
        assert same(got, reference_mask(img, 5, 5, k, polarity="below", exact=True)) and got[0, 11, 41] == hot, k
        assert not mask_of(img, 5, k, polarity="above")[0, 11, 41]


def test_the_mask_goes_into_labelling_and_morphology():
    from librir_amd import device as D
    from librir_amd.synthetic import s1_noisy_background

    frames = s1_noisy_background(2, 67, 130, seed=5)
    frames[0, 20:23, 30:33] += 5000  # (the background spreads over 0..1000: sigma 289; a 3 x 3 spot is sqrt(72 / 9) = 2.8 sigma of its 9 x 9 window)
    frames[1, 40, 100] += 5000
    d = dev(frames)
    mask = D.local_threshold(d, 9, 2, delta=20)
    want = reference_mask(frames, 9, 9, 2, 20)
    assert same(host(mask), want) and want[0, 21, 31] and want[1, 40, 100]
    as_bytes = D.local_threshold(d, 9, 2, delta=20, out=torch.empty((2, 67, 130), dtype=torch.uint8, device="cuda"))
    assert as_bytes.dtype == torch.uint8 and same(host(as_bytes), want.astype(np.uint8))
    labels, _, _, counts = D.label_images(as_bytes)
    labels_b, _, _, counts_b = D.label_images(mask)
    assert teq(labels, labels_b) and teq(counts, counts_b) and same(host(labels) != 0, want)
    opened = D.morph_open(as_bytes, 3)
    assert same(host(opened), host(D.morph_open(dev(want.astype(np.uint8)), 3)))
    assert host(opened)[0, 21, 31] == 1 and host(opened)[1, 40, 100] == 0  # the 3 x 3 spot stays, the single pixel goes


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("h,w,size", [(19, 130, 3), (19, 83, 5), (35, 66, (9, 3)), (19, 66, 15)], ids=str)
def test_rows(dtype, h, w, size):
    """rows below the image are read by no window: a tail of the type's maximum leaks into no output - the clamp goes to rows - 1 and not to
    h - 1; the mean copies the tail, the sums and the mask are 0 there"""
    np_type = np.dtype(dtype).type
    rng = np.random.default_rng(h + w)
    image = rng.integers(0, type_max(np_type) + 1, (2, h, w)).astype(np_type)
    if dtype != "bool":
        image //= 2  # (the upper half of the range is the tail's alone)
    sy, sx = sizes_of(size)
    for rows in (h - 3, 1, 0, h):
        stack = image.copy()
        stack[:, rows:] = type_max(np_type)
        check_stats(stack, size, rows, outputs=OUTPUTS[3:])
        s, q, m = stats(stack, size, rows=rows, sumsq=True, mean=True)
        assert not s[:, rows:].any() and not q[:, rows:].any() and same(m[:, rows:], stack[:, rows:])
        if dtype != "bool":
            assert (m[:, :rows] < type_max(np_type)).all() and (s[:, :rows] <= sy * sx * (type_max(np_type) // 2)).all(), rows
        for k, delta, polarity in ((1, 0, "above"), ((5, 2), -3, "both")):
            got = mask_of(stack, size, k, delta, polarity, rows=rows)
            assert same(got, reference_mask(stack, sy, sx, k, delta, polarity, rows)) and not got[:, rows:].any(), rows


def test_a_batch_equals_its_frames_and_one_image_keeps_its_shape():
    from librir_amd import device as D

    stack = full_range(np.random.default_rng(2), 67, 130, np.uint16)
    stack = np.concatenate([stack, stack[::-1] // 3, stack[:1] // 300])
    for size in (3, (9, 5), 15):
        whole = stats(stack, size, sumsq=True, mean=True)
        whole_mask = mask_of(stack, size, (5, 2), 3, "both")
        for i in range(stack.shape[0]):
            one = stats(stack[i], size, sumsq=True, mean=True)
            assert all(o.shape == (67, 130) and np.array_equal(o, w[i]) for o, w in zip(one, whole)), (size, i)
            assert np.array_equal(mask_of(stack[i], size, (5, 2), 3, "both"), whole_mask[i])
        assert D.box_sum(dev(stack[0]), size).shape == (67, 130) and D.box_mean(dev(stack[0]), size).dtype == torch.uint16


def test_more_frames_than_one_grid_holds():
    """65 537 frames of 2 x 2 uint8: the launcher walks gridDim.z in pieces of 65 535"""
    stack = np.random.default_rng(8).integers(0, 256, (65537, 2, 2)).astype(np.uint8)
    want = wanted(stack, 3)
    got = stats(stack, 3, sumsq=True, mean=True)
    assert all(same(g, w) for g, w in zip(got, want))
    assert same(mask_of(stack, 3, 1), reference_mask(stack, 3, 3, 1))
    odd = np.ascontiguousarray(stack[:, :, :1])  # 2 x 1 frames: the general kernel
    assert all(same(g, w) for g, w in zip(stats(odd, 3, sumsq=True, mean=True), wanted(odd, 3)))


@pytest.mark.parametrize("dtype", ["uint16", "uint8"])
def test_non_contiguous_and_unaligned_input(dtype):
    """a column slice is copied to a contiguous stack first; frames that start at an odd pixel take the general kernel and give the bits the
    pair kernel gives on the same data"""
    from librir_amd import device as D

    np_type = np.dtype(dtype).type
    stack = full_range(np.random.default_rng(4), 17, 131, np_type)
    d = dev(stack)
    even = stack[:, :, :130]
    flat = dev(np.concatenate([np.zeros(1, np_type), even.ravel()]))
    shifted = flat[1:].view(2, 17, 130)
    assert shifted.data_ptr() % (2 * stack.itemsize) != 0 and shifted.is_contiguous()
    for size in (3, 9, (5, 15)):
        sy, sx = sizes_of(size)
        sliced = D.local_stats(d[:, :, 1:], size, sumsq=True, mean=True)
        assert all(same(host(g), w) for g, w in zip(sliced[:3], wanted(stack[:, :, 1:], size)))
        aligned, general = D.local_stats(dev(even), size, sumsq=True, mean=True), D.local_stats(shifted, size, sumsq=True, mean=True)
        assert all(teq(a, g) for a, g in zip(aligned[:3], general[:3])) and same(host(general.sumsq), wanted(even, size)[1])
        assert teq(D.local_threshold(dev(even), size, 2, 1, "both"), D.local_threshold(shifted, size, 2, 1, "both"))
        assert same(host(D.local_threshold(d[:, :, 1:], size, 2, 1, "both")), reference_mask(stack[:, :, 1:], sy, sx, 2, 1, "both"))
        # an output that is not aligned to a pair of its cells: the general kernel again
        out = torch.zeros(2 * 17 * 130 + 1, dtype=torch.int32, device="cuda")[1:].view(2, 17, 130)
        assert teq(D.box_sum(dev(even), size, out=out), aligned.sum)


@pytest.mark.parametrize("size", [3, (7, 3), 15])
def test_out_is_honoured_and_fully_overwritten(size):
    from librir_amd import device as D

    stack = full_range(np.random.default_rng(6), 67, 130, np.uint16)
    sy, sx = sizes_of(size)
    d = dev(stack)
    for rows in (67, 64):
        want = wanted(stack, size, rows)
        want_mask = reference_mask(stack, sy, sx, 2, 5, "both", rows)
        for sentinel in (0, 165):
            outs = (dev(np.full(stack.shape, sentinel, np.int32)), dev(np.full(stack.shape, sentinel, np.int64)), dev(np.full(stack.shape, sentinel, np.uint16)))
            got = D.local_stats(d, size, rows, True, True, True, out=outs)
            assert all(g is o and same(host(o), w) for g, o, w in zip(got[:3], outs, want)), (rows, sentinel)
            got = D.local_stats(d, size, rows, False, False, True, out=D.LocalStats(None, None, outs[2].fill_(sentinel), None))
            assert got.mean is outs[2] and got.sum is None and same(host(outs[2]), want[2])
            assert D.box_sum(d, size, rows, out=outs[0].fill_(sentinel)) is outs[0] and same(host(outs[0]), want[0])
            assert D.box_mean(d, size, rows, out=outs[2].fill_(sentinel)) is outs[2] and same(host(outs[2]), want[2])
            mask = torch.full(stack.shape, bool(sentinel), dtype=torch.bool, device="cuda")
            assert D.local_threshold(d, size, 2, 5, "both", rows, out=mask) is mask and same(host(mask), want_mask)
            as_bytes = dev(np.full(stack.shape, sentinel, np.uint8))
            assert D.local_threshold(d, size, 2, 5, "both", rows, out=as_bytes) is as_bytes and same(host(as_bytes), want_mask.astype(np.uint8))


def test_overlap_is_refused():
    from librir_amd import device as D

    d = dev(full_range(np.random.default_rng(7), 17, 64, np.uint16).repeat(2, axis=0))
    with pytest.raises(RuntimeError, match="overlap"):
        D.box_mean(d[:3], 3, out=d[1:])
    squares = torch.zeros((2, 17, 64), dtype=torch.int64, device="cuda")
    sums = squares.view(torch.int32).view(-1)[:2 * 17 * 64].view(2, 17, 64)  # the first half of the squares' memory
    with pytest.raises(RuntimeError, match="overlap"):
        D.local_stats(d[:2], 3, sumsq=True, out=(sums, squares, None))
    d8 = dev(np.zeros((4, 17, 64), np.uint8))
    with pytest.raises(RuntimeError, match="overlap"):
        D.local_threshold(d8[:3], 3, 1, out=d8[1:])
    with pytest.raises(RuntimeError, match="overlap"):
        D.local_threshold(d8, 3, 1, out=d8.view(torch.bool))


@pytest.mark.parametrize("dtype", DTYPES)
def test_host_entries_equal_device_entries(lib, dtype):
    from librir_amd import device as D
    from librir_amd import signal_processing as S

    np_type = np.dtype(dtype).type
    for (n, h, w), size, rows in [((3, 17, 64), 3, 14), ((2, 67, 130), 5, None), ((5, 67, 83), (9, 5), None), ((2, 1, 1), 15, None), ((1, 3, 5), 1, 0)]:
        stack = np.concatenate([full_range(np.random.default_rng(n * h), h, w, np_type)] * 3)[:n]
        sy, sx = sizes_of(size)
        want = stats(stack, size, rows=rows, sumsq=True, mean=True)
        assert all(same(g, w_) for g, w_ in zip(want, wanted(stack, size, rows)))
        got = S.local_stats(stack, size, rows, sumsq=True, mean=True)
        assert all(same(g, w_) for g, w_ in zip(got[:3], want)) and got.n == sy * sx
        one = S.local_stats(stack[0], size, rows, sum=False, mean=True)
        assert one.sum is None and one.sumsq is None and same(one.mean, want[2][0])
        want_mask = mask_of(stack, size, (3, 2), 1, "both", rows=rows)
        assert same(want_mask, reference_mask(stack, sy, sx, (3, 2), 1, "both", rows))
        assert same(S.local_threshold(stack, size, (3, 2), 1, "both", rows), want_mask)
        assert same(S.local_threshold(stack[0], size, (3, 2), 1, "both", rows), want_mask[0])
        terms, n2 = D.local_variance_terms(got)
        assert n2 == (sy * sx) ** 2 and same(terms, sy * sx * want[1] - want[0].astype(np.int64) ** 2) and (terms >= 0).all()
        # through the C entries
        lib.rir_local_stats.argtypes = [ct.c_int, ct.c_void_p] + [ct.c_int] * 6 + [ct.c_void_p] * 3
        lib.rir_local_threshold.argtypes = [ct.c_int, ct.c_void_p, ct.c_void_p] + [ct.c_int] * 10
        char = ord({"uint16": "H", "uint8": "B", "bool": "?"}[dtype])
        sums, squares, mask = np.full(stack.shape, -1, np.int32), np.full(stack.shape, -1, np.int64), np.full(stack.shape, 9, np.uint8)
        assert lib.rir_local_stats(char, stack.ctypes.data, w, h, n, sx, sy, h if rows is None else rows, sums.ctypes.data, squares.ctypes.data, None) == 0
        assert same(sums, want[0]) and same(squares, want[1])
        assert lib.rir_local_threshold(char, stack.ctypes.data, mask.ctypes.data, w, h, n, sx, sy, h if rows is None else rows, 3, 2, 1, 2) == 0
        assert same(mask, want_mask.astype(np.uint8))


def test_device_variance_terms():
    from librir_amd import device as D

    stack = full_range(np.random.default_rng(12), 17, 66, np.uint16)
    got = D.local_stats(dev(stack), 7, sumsq=True)
    terms, n2 = D.local_variance_terms(got)
    S, Q = reference_sums(stack, 7, 7), reference_sums(stack, 7, 7, power=2)
    assert n2 == 49 * 49 and terms.dtype == torch.int64 and same(host(terms), 49 * Q - S * S)
    variance = host(terms).astype(np.float64) / n2
    assert np.allclose(variance[0, 8, 30], stack[0, 5:12, 27:34].astype(np.float64).var(), rtol=1e-12)


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
    arr[:, 30, 40] += 5000
    with IRMovie.from_filename(record(tmp_path / "m.h264", arr)) as mov:
        assert same(host(mov.local_threshold(9, 4, delta=20)), reference_mask(np.asarray(mov.data), 9, 9, 4, 20))
        assert same(host(mov.box_mean(9)), reference_mean(np.asarray(mov.data), 9, 9))
        mov._STATS_PIECE_BYTES = 3 * h * w * 2
        for sel, size, rows in [(slice(None), 5, None), (slice(1, None, 2), (3, 5), h - 3), (3, 9, None), (slice(0, 0), 3, None)]:
            frames = mov.to_tensor(sel)
            sy, sx = sizes_of(size)
            got = mov.local_threshold(size, (5, 2), 3, "both", sel, rows)
            assert got.dtype == torch.bool and got.shape == frames.shape and teq(got, D.local_threshold(frames, size, (5, 2), 3, "both", rows)), (sel, size)
            assert same(host(got), reference_mask(host(frames), sy, sx, (5, 2), 3, "both", rows))
            out = torch.ones(tuple(got.shape), dtype=torch.bool, device="cuda")
            assert mov.local_threshold(size, (5, 2), 3, "both", selection=sel, rows=rows, out=out) is out and teq(out, got)
            mean = mov.box_mean(size, sel, rows)
            assert mean.dtype == torch.uint16 and teq(mean, D.box_mean(frames, size, rows)) and same(host(mean), reference_mean(host(frames), sy, sx, rows))
            out = dev(np.full(tuple(mean.shape), 12345, np.uint16))
            assert mov.box_mean(size, selection=sel, rows=rows, out=out) is out and teq(out, mean)
        labels = D.label_images(mov.local_threshold(9, 4, delta=20))[0]
        assert (host(labels)[:, 30, 40] != 0).all()
        with pytest.raises(ValueError):
            mov.local_threshold(4, 3)
        with pytest.raises(ValueError):
            mov.local_threshold(3, (1, 0))
        with pytest.raises(ValueError):
            mov.box_mean(17)
        with pytest.raises(RuntimeError):
            mov.box_mean(3, out=torch.empty((n, h, w + 1), dtype=torch.uint16, device="cuda"))
        with pytest.raises(RuntimeError):
            mov.local_threshold(3, 3, out=torch.empty((n, h, w), dtype=torch.uint8, device="cuda"))
