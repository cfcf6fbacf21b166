"""GPU: the exact Euclidean distance transform, bit for bit against the references of distance_cases.py (checked against scipy and against each
other in test_distance_transform_cpu.py) - every image, shape and type with the border off and on, dist2 and index, the rows rule, batches
and groups, sentinel fill, out=, full-size frames, the disc forms against scipy's binary morphology, the host entry, and recordings through
IRMovie.distance_transform."""
import functools

import numpy as np
import pytest

from distance_cases import DIST2_NONE, SHAPES, TYPES, brute_force, foregrounds, label_map, reference_stack, separable, typed_stack

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).cuda().view(torch.uint16)
    return torch.from_numpy(a).cuda()


def run(stack, **kw):
    """(dist2, index) as numpy arrays"""
    from librir_amd import device as D

    dist2, index = D.distance_transform(dev(stack), return_indices=True, **kw)
    assert dist2.dtype == torch.int32 and index.dtype == torch.int32 and tuple(dist2.shape) == stack.shape == tuple(index.shape)
    return dist2.cpu().numpy(), index.cpu().numpy()


def same(got, want):
    return all(g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))


_references = {}


def small_reference(h, w, border):
    """the brute-force (dist2, index) of foregrounds(h, w), computed once"""
    key = (h, w, border)
    if key not in _references:
        _references[key] = reference_stack(np.stack([fg for _, fg in foregrounds(h, w)]), 0, border)
    return _references[key]


@pytest.mark.parametrize("type_char", list(TYPES))
@pytest.mark.parametrize("h,w", SHAPES)
def test_every_image_shape_and_type(h, w, type_char):
    from librir_amd import device as D

    stack = typed_stack(h, w, type_char)
    names = [name for name, _ in foregrounds(h, w)]
    for border in (False, True):
        want = small_reference(h, w, border)
        if type_char == "i":  # (the label map at the end)
            extra = brute_force(stack[-1], 0, border)
            want = tuple(np.concatenate([a, b[None]]) for a, b in zip(want, extra))
        got = run(stack, border=border)
        for i in range(stack.shape[0]):
            assert same((got[0][i], got[1][i]), (want[0][i], want[1][i])), (names + ["label_map"])[i]
        only = D.distance_transform(dev(stack), border=border)  # (the launch without indices)
        assert only.dtype == torch.int32 and np.array_equal(only.cpu().numpy(), want[0])


@pytest.mark.parametrize("h,w", SHAPES)
def test_background_value(h, w):
    lab = label_map(h, w)[None]
    for background in (0, 3, -2, 7):
        for border in (False, True):
            assert same(run(lab, background=background, border=border), reference_stack(lab, background, border)), (background, border)
    bytes_ = (label_map(h, w) + 2).astype(np.uint8)[None]
    assert same(run(bytes_, background=5), reference_stack(bytes_, 5))
    words = (label_map(h, w).astype(np.int64) * 9000 + 20000).astype(np.uint16)[None]
    assert same(run(words, background=65000), reference_stack(words, 65000)) and same(run(words, background=47000), reference_stack(words, 47000))
    mask = (label_map(h, w) > 0)[None]
    assert same(run(mask, background=1, border=True), reference_stack(mask, 1, True))


@pytest.mark.parametrize("h,w", [s for s in SHAPES if s[0] > 3])
def test_rows(h, w):
    """the last three rows, all but one row, and every row outside the image: read by nothing, dist2 0 and their own index"""
    stack = typed_stack(h, w, "B")[::3]
    for rows in (h - 3, 1, 0):
        for border in (False, True):
            got, want = run(stack, rows=rows, border=border), reference_stack(stack, 0, border, rows, separable)
            assert same(got, want), (rows, border)
            own = np.arange(h * w).reshape(h, w)[rows:]
            assert (got[0][:, rows:] == 0).all() and (got[1][:, rows:] == own).all()


@pytest.fixture(scope="module")
def many_frames():
    """67 different frames of 37 x 70, with their reference"""
    rng = np.random.default_rng(67)
    base = np.stack([fg for _, fg in foregrounds(37, 70)])
    stack = np.concatenate([base, rng.random((67 - len(base), 37, 70)) < rng.random((67 - len(base), 1, 1))]).astype(np.uint8)
    return stack, reference_stack(stack, 0, False, None, separable)


@pytest.mark.parametrize("n", [1, 2, 5, 67])
def test_a_batch_equals_its_frames(many_frames, n):
    stack, want = many_frames
    whole = run(stack[:n])
    assert same(whole, (want[0][:n], want[1][:n]))
    for i in sorted({0, n // 2, n - 1}):
        assert same(run(stack[i]), (whole[0][i], whole[1][i])), i


def test_small_groups_equal_one_group(many_frames, monkeypatch):
    """a workspace of three frames, and of one: the entry walks the stack in groups and gives the same bits"""
    from librir_amd import device as D

    stack, want = many_frames
    whole = run(stack)
    assert same(whole, want)
    one = D._lib.rir_distance_transform_workspace_bytes(70, 37, 1, 1)
    for frames in (3, 1, 0):
        monkeypatch.setattr(D, "_DISTANCE_WORK_BYTES", frames * one + 5)
        assert same(run(stack), whole), frames
        assert np.array_equal(D.distance_transform(dev(stack), border=True).cpu().numpy(), reference_stack(stack, 0, True, None, separable)[0])


def test_outputs_are_fully_overwritten_and_out_is_honoured():
    from librir_amd import device as D

    stack = typed_stack(37, 70, "H")
    for rows in (37, 34):
        want = reference_stack(stack, 0, True, rows, separable)
        for sentinel in (-7, 0x5A5A5A5A):
            dist2, index = dev(np.full(stack.shape, sentinel, np.int32)), dev(np.full(stack.shape, sentinel, np.int32))
            back = D.distance_transform(dev(stack), border=True, rows=rows, return_indices=True, out=(dist2, index))
            assert back[0] is dist2 and back[1] is index and same((dist2.cpu().numpy(), index.cpu().numpy()), want), (rows, sentinel)
            alone = dev(np.full(stack.shape, sentinel, np.int32))
            assert D.distance_transform(dev(stack), border=True, rows=rows, out=alone) is alone and np.array_equal(alone.cpu().numpy(), want[0])
    one = dev(np.full((37, 70), -7, np.int32))
    assert D.distance_transform(dev(stack[3]), out=one) is one and np.array_equal(one.cpu().numpy(), brute_force(stack[3])[0])
    assert D.distance_transform(dev(stack[:0])).shape == (0, 37, 70)
    d = dev(stack.astype(np.int32))
    with pytest.raises(RuntimeError, match="overlap"):
        D.distance_transform(d, out=d)
    with pytest.raises(RuntimeError, match="overlap"):
        D.distance_transform(d[:3], return_indices=True, out=(d[3:6], d[5:8]))


@functools.lru_cache(maxsize=None)
def full_frames():
    """[(name, uint8 [512][640])]: one background pixel in a corner (the largest distances), a background diagonal (a parabola from every row
    in every column), hot-spot masks and their inversions (the distance from everywhere to a few spots), and no background at all"""
    from librir_amd.synthetic import hot_spots

    corner = np.ones((512, 640), np.uint8)
    corner[0, 0] = 0
    hot = (hot_spots(24)[[5, 12, 23]] > 4000).astype(np.uint8)
    ys, xs = np.mgrid[:512, :640]
    return [("corner", corner), ("diagonal", (ys != xs).astype(np.uint8)), ("hot_0", hot[0]), ("hot_1", hot[1]), ("hot_2", hot[2]),
            ("cold_0", 1 - hot[0]), ("cold_1", 1 - hot[1]), ("all_foreground", np.ones((512, 640), np.uint8))]


@pytest.fixture(scope="module")
def full_size():
    frames = full_frames()
    stack = np.stack([f for _, f in frames])
    return [name for name, _ in frames], stack, reference_stack(stack, 0, False, None, separable), run(stack), run(stack, border=True)


def test_full_size_frames(full_size):
    names, stack, want, got, got_border = full_size
    assert got[0][0].max() == got[0][0][511, 639] == 511 ** 2 + 639 ** 2 == 669442 and (got[1][0] == 0).all()
    assert (got[0][-1] == DIST2_NONE).all() and (got[1][-1] == -1).all()
    for i, name in enumerate(names):
        assert same((got[0][i], got[1][i]), (want[0][i], want[1][i])), name
    ys, xs = np.mgrid[:512, :640]
    b2 = (np.minimum(np.minimum(xs + 1, 640 - xs), np.minimum(ys + 1, 512 - ys)) ** 2).astype(np.int32)
    assert np.array_equal(got_border[0], np.minimum(want[0], b2)) and np.array_equal(got_border[1], np.where(b2 < want[0], -1, want[1]))


def test_full_size_frames_against_scipy(full_size):
    ndi = pytest.importorskip("scipy.ndimage")
    names, stack, want, got, _ = full_size
    for i, name in enumerate(names[:-1]):
        assert np.array_equal(got[0][i], np.rint(ndi.distance_transform_edt(stack[i]) ** 2).astype(np.int32)), name


def disc(radius):
    r = int(np.floor(radius))
    ys, xs = np.mgrid[-r:r + 1, -r:r + 1]
    return ys * ys + xs * xs <= radius * radius


@pytest.mark.parametrize("radius", [0, 1, 1.5, 2.3, 5, 20])
def test_disc_forms_against_scipy(radius):
    ndi = pytest.importorskip("scipy.ndimage")
    from librir_amd import device as D

    st = disc(radius)
    erode = lambda m, border_value=1: ndi.binary_erosion(m, st, border_value=border_value)  # noqa: E731
    dilate = lambda m: ndi.binary_dilation(m, st)  # noqa: E731
    for h, w in ((37, 70), (65, 63), (1, 7)):
        masks = np.stack([fg for _, fg in foregrounds(h, w)])[::4 if radius > 5 else 1]  # (scipy's 41 x 41 element is slow on the host)
        for stack in (masks, masks.astype(np.uint8) * 3):
            d = dev(stack)
            as_type = lambda frames: np.stack(frames).astype(stack.dtype)  # noqa: E731
            for got, want in ((D.disc_erode(d, radius), [erode(m) for m in masks]), (D.disc_erode(d, radius, border=True), [erode(m, 0) for m in masks]),
                              (D.disc_dilate(d, radius), [dilate(m) for m in masks]), (D.disc_open(d, radius), [dilate(erode(m)) for m in masks]),
                              (D.disc_close(d, radius), [erode(dilate(m)) for m in masks])):
                assert got.dtype == d.dtype and got.shape == d.shape
                want = as_type(want) if radius else stack  # (radius 0 copies: a uint8 mask keeps its values)
                assert np.array_equal(got.cpu().numpy(), want), (h, w, stack.dtype)
        assert np.array_equal(D.disc_dilate(dev(masks[3]), radius).cpu().numpy(), dilate(masks[3]))


@pytest.mark.parametrize("type_char", list(TYPES))
def test_host_entry_equals_device_entry(type_char):
    from librir_amd import signal_processing as S

    for h, w, background, border, rows in ((37, 70, 0, False, None), (5, 65, 0, True, 3), (1, 1, 0, False, None), (130, 3, 1, True, None)):
        stack = typed_stack(h, w, type_char)
        want = run(stack, background=background, border=border, rows=rows)
        assert same(want, reference_stack(stack, background, border, rows))
        got = S.distance_transform(stack, background, border, rows, return_indices=True)
        assert same(got, want)
        alone = S.distance_transform(stack[2], background, border, rows)
        assert alone.dtype == np.int32 and np.array_equal(alone, want[0][2])


def test_host_entry_in_slabs():
    """more than one 64 MiB slab: 40 frames of 640 x 512 with indices take 8 bytes of outputs a pixel, 25 frames a slab"""
    from librir_amd import signal_processing as S

    frames = np.stack([f for _, f in full_frames()[2:7]])
    stack = np.tile(frames, (8, 1, 1))
    stack[:, 300, 400] = np.arange(40) % 2
    got = S.distance_transform(stack, return_indices=True)
    assert same((got[0][:5], got[1][:5]), reference_stack(stack[:5], 0, False, None, separable))
    assert same((got[0][35:], got[1][35:]), run(stack[35:]))
    assert np.array_equal(got[0][10:20], got[0][:10]) and np.array_equal(got[1][30:40], got[1][:10])


def record(path, frames):
    from librir_amd.video_io import IRSaver

    n, h, w = frames.shape
    with IRSaver(str(path), w, h, h) as s:
        for i in range(n):
            s.add_image(frames[i], i * 20000000 + 7)
    return str(path)


def test_recordings(tmp_path):
    from librir_amd import device as D
    from librir_amd.synthetic import hot_spots
    from librir_amd.video_io import IRMovie

    n, h, w = 7, 67, 83
    arr = hot_spots(n, h, w, seed=4)
    level = int(np.percentile(arr, 90))
    cut_map = np.full((h, w), level, np.int32)
    cut_map[:, w // 2:] += 50
    with IRMovie.from_filename(record(tmp_path / "m.h264", arr)) as mov:
        for sel, t, invert, border, rows in [(slice(None), level, False, False, None), (slice(1, None, 2), level, True, True, h - 3),
                                             (3, cut_map, False, True, None), (slice(None), torch.from_numpy(cut_map).cuda(), True, False, None),
                                             (slice(0, 0), level, False, False, None)]:
            frames = mov.to_tensor(sel)
            cut = t if isinstance(t, int) else torch.as_tensor(t).cuda()
            hot = (frames.view(torch.int16).to(torch.int32) & 0xFFFF) > cut
            want = D.distance_transform(hot, int(invert), border, rows, return_indices=True)
            got = mov.distance_transform(t, sel, invert, border, rows, return_indices=True)
            assert got[0].dtype == torch.int32 and got[0].shape == frames.shape and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
            assert torch.equal(mov.distance_transform(t, sel, invert=invert, border=border, rows=rows), want[0])
            ref = reference_stack(hot.cpu().numpy(), int(invert), border, rows, separable) if frames.shape[0] else None
            assert ref is None or same((got[0].cpu().numpy(), got[1].cpu().numpy()), ref)
        # pieces smaller than the selection give the same bits
        want = mov.distance_transform(level, return_indices=True)
        assert int(want[0].max()) > 0 and int((want[0] == 0).sum()) > 0
        mov._STATS_PIECE_BYTES = 3 * h * w * 2
        got = mov.distance_transform(level, return_indices=True)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        with pytest.raises(ValueError):
            mov.distance_transform(level, rows=h + 1)
        with pytest.raises(ValueError):
            mov.distance_transform(np.zeros((h, w + 1)))
