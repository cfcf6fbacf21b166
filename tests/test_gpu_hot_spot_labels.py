"""GPU: hot spots labelled straight from the frames, every output bit for bit against the oracle of hot_spot_cases.py - random frames
at the shapes that cross, meet and miss the 64 x 32 tile's borders under each predicate and all of them, hand-made scenes (a spiral and a
comb over four tiles whose only strong pixel is far from the root, exact area limits, a corner on the border, full and empty frames, the
ends of the 16-bit range, cut rows, per-pixel thresholds, short tables), the equalities with label_images, reproducibility, stream order
and recordings read through IRMovie.track_kept_hot_spots."""
import numpy as np
import pytest

import hot_spot_cases as HC
import track_cases as TC
from hot_spot_cases import HIGH, LOW, STRONG, WEAK

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

OUTPUTS = ("labels", "area", "first", "counts")


def dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda().view(torch.uint16)


def same(got, exp, what):
    got = got.cpu().numpy()
    assert got.dtype == exp.dtype and got.shape == exp.shape, (what, got.dtype, got.shape, exp.shape)
    if not np.array_equal(got, exp):
        bad = np.argwhere(got != exp)[:5]
        raise AssertionError("%s differs at %s: got %s, expected %s" % (what, bad.tolist(), got[tuple(bad.T)], exp[tuple(bad.T)]))


def run(frames, low, what="", **kw):
    """label_hot_spots on the device against the oracle; -> (the device's result, the oracle's)"""
    from librir_amd import device as D

    frames = np.asarray(frames, np.uint16)
    got = D.label_hot_spots(dev16(frames), low, **kw)
    exp = HC.oracle(frames, low, **kw)
    for k, g in zip(OUTPUTS, got):
        same(g, exp[k], (what, kw, k))
    return got, exp


@pytest.fixture(scope="module")
def random_frames():
    return {shape: HC.random_frames(shape) for shape in HC.RANDOM_SHAPES}


@pytest.mark.parametrize("shape", HC.RANDOM_SHAPES)
@pytest.mark.parametrize("kw", HC.RANDOM_FILTERS, ids="+".join)
def test_random_frames(random_frames, shape, kw):
    _, exp = run(random_frames[shape], HC.RANDOM_LOW, shape, **kw)
    if shape == (2, 70, 130) and len(kw) == 1:  # the predicate keeps and drops components that were joined across a tile border
        for f in range(2):
            kept, dropped = HC.spanning(exp, f)
            assert kept > 0 and dropped > 0, (kw, f, kept, dropped)


@pytest.mark.parametrize("shape", HC.RANDOM_SHAPES)
def test_low_alone_is_label_images_of_the_mask(random_frames, shape):
    """labels, areas and counts of label_images(frames > low), and its launches: no component can be dropped"""
    from librir_amd import device as D

    frames = random_frames[shape]
    cap = shape[1] * shape[2] + 1
    got, exp = run(frames, HC.RANDOM_LOW, shape, table_entries=cap)
    lab, area, xy, counts = D.label_images(torch.from_numpy(frames.astype(np.int32) > HC.RANDOM_LOW).cuda(), table_entries=cap)
    assert torch.equal(got[0], lab) and torch.equal(got[1], area) and torch.equal(got[3], counts)
    k = int(counts[0])
    assert np.array_equal(exp["first"][0, 1:k] % shape[2], xy[0, 1:k, 0].cpu().numpy())  # (its table holds the first pixel's column)


@pytest.mark.parametrize("kw", HC.RANDOM_FILTERS, ids="+".join)
def test_filtered_map_is_label_images_of_the_kept_mask(random_frames, kw):
    from librir_amd import device as D

    got, exp = run(random_frames[(2, 70, 130)], HC.RANDOM_LOW, **kw)
    lab, _, _, counts = D.label_images(torch.from_numpy(exp["mask"]).cuda(), table_entries=1)
    assert torch.equal(got[0], lab) and torch.equal(got[3], counts)


@pytest.mark.parametrize("scene", ["spiral", "comb"])
@pytest.mark.parametrize("strong_at", ["last pixel", "root"])
def test_strong_pixel_far_from_the_root(scene, strong_at):
    """one component over four tiles; its only strong pixel is its last pixel in raster order, in the tile farthest from the root - or
    the root itself; frame 1 has none and stays empty"""
    mask = HC.spiral(64, 128) if scene == "spiral" else HC.comb(64, 128)
    ys, xs = np.nonzero(mask)
    at = (int(ys[-1]), int(xs[-1])) if strong_at == "last pixel" else (0, 0)
    assert at[0] >= 32 and at[1] >= 64 or at == (0, 0)
    frames = np.stack([HC.scene(mask, [at]), HC.scene(mask), HC.scene(mask, [at])])
    if scene == "comb":  # weak specks between the teeth, and one strong one
        frames[:, 40, 66::4] = WEAK
        frames[2, 40, 70] = STRONG
    _, exp = run(frames, LOW, high=HIGH)
    area = int(mask.sum())
    assert exp["counts"].tolist() == [2, 1, 3 if scene == "comb" else 2] and exp["area"][0, 1] == area and exp["first"][0, 1] == 0
    run(frames, LOW, high=HIGH, min_area=area, max_area=area)
    run(frames, LOW, high=HIGH, clear_border=True)


def test_area_limits_are_inclusive():
    a = 37
    mask = np.zeros((48, 72), bool)
    mask[31, 50:71] = True  # an L of exactly `a` pixels over the tile borders in x and in y
    mask[31:48, 70] = True
    mask[3:6, 3:6] = True  # 9 pixels
    mask[40, 10:15] = True  # 5 pixels
    frames = HC.scene(mask)[None]
    assert sorted(HC.oracle(frames, LOW)["area"][0, 1:4].tolist()) == [5, 9, a]
    for key in ("min_area", "max_area"):
        for limit in (a - 1, a, a + 1):
            _, exp = run(frames, LOW, **{key: limit})
            assert (a in exp["area"][0, 1:]) == (limit <= a if key == "min_area" else limit >= a), (key, limit)
    _, exp = run(frames, LOW, min_area=a, max_area=a)
    assert exp["counts"].tolist() == [2] and exp["first"][0, 1] == 31 * 72 + 50


def diamond(mask, cy, cx, r=3):
    y, x = np.mgrid[0:mask.shape[0], 0:mask.shape[1]]
    mask |= abs(y - cy) + abs(x - cx) <= r


def test_border_touched_at_a_corner_pixel_only():
    """a component whose one pixel on the border is the tip of a diamond, on each side of the image, and single pixels in the image's corners"""
    h, w = 40, 131
    for inset in (0, 1):
        mask = np.zeros((h, w), bool)
        for cy, cx in ((3 + inset, 30), (h - 4 - inset, 90), (20, 3 + inset), (20, w - 4 - inset), (20, 64)):
            diamond(mask, cy, cx)
        on_border = mask[0].sum() + mask[-1].sum() + mask[:, 0].sum() + mask[:, -1].sum()
        assert on_border == (0 if inset else 4)
        _, exp = run(HC.scene(mask)[None], LOW, inset, clear_border=True)
        assert exp["counts"].tolist() == [6 if inset else 2]
    mask = np.zeros((h, w), bool)
    mask[[0, 0, -1, -1], [0, -1, 0, -1]] = True
    mask[1, 1] = mask[h - 2, w - 2] = True  # diagonal neighbours are not joined
    _, exp = run(HC.scene(mask)[None], LOW, "corners", clear_border=True)
    assert exp["counts"].tolist() == [3] and exp["first"][0, 1:3].tolist() == [w + 1, (h - 2) * w + w - 2]


def test_full_and_empty_frames():
    """a frame that is one component, and an empty frame between full ones: counts and numbers are each frame's own"""
    h, w = 37, 131
    rng = np.random.default_rng(8)
    busy = np.where(rng.random((h, w)) < 0.05, STRONG, rng.integers(0, 1000, (h, w))).astype(np.uint16)
    frames = np.stack([np.full((h, w), WEAK, np.uint16), busy, np.zeros((h, w), np.uint16), busy, np.full((h, w), STRONG, np.uint16)])
    _, exp = run(frames, LOW, table_entries=h * w + 1)
    assert exp["counts"][[0, 2, 4]].tolist() == [2, 1, 2] and exp["counts"][1] == exp["counts"][3] > 100 and exp["area"][0, 1] == h * w
    _, exp = run(frames, LOW, high=HIGH, min_area=3)
    assert exp["counts"][[0, 2, 4]].tolist() == [1, 1, 2] and exp["counts"][1] == exp["counts"][3] > 10
    _, exp = run(frames, LOW, clear_border=True, max_area=h * w - 1)
    assert exp["counts"][[0, 2, 4]].tolist() == [1, 1, 1]
    _, exp = run(frames, LOW, max_area=h * w)
    assert exp["counts"][[0, 2, 4]].tolist() == [2, 1, 2]


@pytest.mark.parametrize("low", [-1, 0, 65534, 65535, -7, 70000, -0.5, 65534.5])
def test_ends_of_the_range(low):
    h, w = 33, 67
    frames = np.zeros((2, h, w), np.uint16)
    frames[0, ::3, ::2] = 65535
    frames[1] = 65535
    frames[1, 5:9, 60:66] = 0
    _, exp = run(frames, low)
    fg = exp["mask"].reshape(2, -1).sum(1).tolist()
    assert fg == ([h * w, h * w] if low < 0 else [0, 0] if low >= 65535 else [int((frames[0] > 0).sum()), h * w - 24]), fg
    run(frames, low, high=65534)
    run(frames, -1, high=low, min_area=2)
    run(frames, np.full((h, w), int(np.floor(min(max(low, -1), 65535))), np.int32), high=np.full((h, w), 65534.0))


def test_rows_cut_strong_pixels_and_the_border():
    h, w = 40, 70
    mask = np.zeros((h, w), bool)
    mask[30:, 20] = True  # reaches into the cut rows, where its strong pixel is
    mask[34:37, 40:43] = True  # ends on the last row that counts
    mask[10:13, 10:13] = True
    frames = HC.scene(mask, [(h - 2, 20), (11, 11), (35, 41)])[None]
    _, exp = run(frames, LOW, rows=h - 3, high=HIGH)
    assert exp["counts"].tolist() == [3] and not exp["labels"][0, h - 3:].any() and exp["labels"][0, 30:h - 3, 20].tolist() == [0] * 7
    _, exp = run(frames, LOW, rows=h - 3, clear_border=True)
    assert exp["counts"].tolist() == [2]
    _, exp = run(frames, LOW, rows=h - 3, min_area=8)
    assert exp["counts"].tolist() == [3]  # (the cut column holds 7 pixels)
    run(frames, LOW, rows=1)
    run(frames, LOW, rows=h, high=HIGH, clear_border=True)


def test_per_pixel_thresholds():
    """equal values: foreground in one column and not in the next, strong in one column and not in the next"""
    h, w = 34, 130
    frames = np.full((2, h, w), WEAK, np.uint16)
    frames[1, ::2] = 0
    low = np.where(np.arange(w)[None, :] % 3 == 2, WEAK, WEAK - 1) + np.zeros((h, 1), np.int64)
    low[20] = WEAK  # a row of background: two bands of stripes
    high = np.full((h, w), WEAK, np.int64)
    high[5, 64] = high[25, 1] = WEAK - 1
    _, exp = run(frames, low, table_entries=h * w + 1)
    assert exp["counts"][0] == 2 * ((w + 2) // 3) + 1
    for lo, hi in ((low, high), (low.astype(np.int32), torch.from_numpy(high).cuda()), (torch.from_numpy(low.astype(np.float64) + 0.5), high)):
        _, exp = run_maps(frames, lo, hi, low, high)
        assert exp["counts"].tolist() == [3, 3]
    run(frames, low, high=WEAK - 1, min_area=14, clear_border=True)
    run(frames, WEAK - 1, high=high)


def run_maps(frames, lo, hi, lo_np, hi_np):
    from librir_amd import device as D

    got = D.label_hot_spots(dev16(frames), lo, high=hi)
    exp = HC.oracle(frames, lo_np, high=hi_np)
    for k, g in zip(OUTPUTS, got):
        same(g, exp[k], k)
    return got, exp


def test_short_tables_and_high_below_low():
    frames = HC.random_frames((2, 70, 130))
    for cap in (1, 2, 17):
        _, exp = run(frames, HC.RANDOM_LOW, min_area=3, table_entries=cap)
        assert exp["counts"].min() > 17
    got, exp = run(frames, HC.RANDOM_LOW, high=HC.RANDOM_LOW - 5)  # a high below low filters nothing
    plain = HC.oracle(frames, HC.RANDOM_LOW)
    assert all(np.array_equal(exp[k], plain[k]) for k in OUTPUTS)


def test_one_image_and_checks_on_the_device():
    from librir_amd import device as D

    img = HC.random_frames((33, 65))
    got = D.label_hot_spots(dev16(img), HC.RANDOM_LOW, min_area=2)
    exp = HC.oracle(img, HC.RANDOM_LOW, min_area=2)
    for k, g in zip(OUTPUTS, got):
        same(g, exp[k], k)
    with pytest.raises(RuntimeError, match="dtype"):
        D.label_hot_spots(torch.zeros((2, 4, 5), dtype=torch.int32, device="cuda"), 1)
    with pytest.raises(ValueError, match="label_hot_spots: high holds a NaN"):
        D.label_hot_spots(dev16(img), 1, high=torch.full((33, 65), float("nan"), device="cuda"))


def test_twice_in_a_row_and_on_a_side_stream():
    from librir_amd import device as D

    frames = HC.random_frames((3, 70, 130))
    kw = dict(high=64000, min_area=3, max_area=400, clear_border=True)
    exp = HC.oracle(frames, HC.RANDOM_LOW, **kw)
    t = dev16(frames)
    runs = [D.label_hot_spots(t, HC.RANDOM_LOW, **kw) for _ in range(3)]
    host = torch.from_numpy(frames.view(np.int16)).pin_memory()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        runs.append(D.label_hot_spots(host.to("cuda", non_blocking=True).view(torch.uint16), HC.RANDOM_LOW, **kw))
    side.synchronize()
    for r in runs:
        for k, g in zip(OUTPUTS, r):
            same(g, exp[k], k)


def record(path, frames):
    from librir_amd.video_io import IRSaver

    n, h, w = frames.shape
    with IRSaver(str(path), w, h, h) as s:
        for i in range(n):
            s.add_image(frames[i], i * 20000000 + 7)
    return str(path)


def test_movie_track_kept_hot_spots(tmp_path):
    """tracks, and the region_stats counts, equal track_components over the oracle's maps"""
    from librir_amd import device as D
    from librir_amd.synthetic import hot_spots
    from librir_amd.video_io import IRMovie

    n, h, w = 30, 40, 70
    frames = hot_spots(n, h, w, 2024)
    frames[:, 3::7, 5::9] += 3000  # specks above the low threshold (the background stays below 2 100, the discs are 8 000 above it)
    path = record(tmp_path / "hot.h264", frames)
    low = 4000 + np.arange(h * w).reshape(h, w) % 7 * 100
    with IRMovie.from_filename(path) as mov:
        mov._STATS_PIECE_BYTES = 11 * h * w * 2  # several pieces
        for threshold, kw in ((4000, dict(high=9000, min_area=4)), (low, dict(min_area=2, clear_border=True)), (4000.5, dict(max_area=30))):
            frames = np.asarray(mov[:])
            exp = HC.oracle(frames, np.floor(threshold).astype(np.int64), **kw)
            assert exp["counts"].max() > 1 and exp["counts"].sum() < HC.oracle(frames, np.floor(threshold).astype(np.int64))["counts"].sum()
            want = D.track_components(torch.from_numpy(exp["labels"]).cuda(), torch.from_numpy(exp["counts"]).cuda())
            tracks, stats = mov.track_kept_hot_spots(threshold, **kw)
            for a, b in zip(tracks, want):
                assert torch.equal(a, b)
            ntracks = int(want.ntracks)
            assert ntracks >= 2
            rs = D.region_stats(dev16(frames), want.tracks, ntracks)
            assert torch.equal(stats.count, rs.count)
            oracle_tracks = TC.track_oracle(exp["labels"], exp["counts"], int(exp["counts"].max()))
            same(tracks.tracks, oracle_tracks["tracks"], "tracks")
            tracks3, _, geo = mov.track_kept_hot_spots(threshold, stats=False, geometry=True, **kw)
            assert torch.equal(tracks3.tracks, tracks.tracks) and torch.equal(geo.count, rs.count)
        for threshold in (4000, low):  # no filter: what track_hot_spots gives, by the other route
            got, want = mov.track_kept_hot_spots(threshold), mov.track_hot_spots(threshold)
            assert all(torch.equal(a, b) for a, b in zip(got[0], want[0])) and all(torch.equal(a, b) for a, b in zip(got[1], want[1]))
        with pytest.raises(ValueError, match="label_hot_spots.*min_area"):
            mov.track_kept_hot_spots(4000, min_area=0)
