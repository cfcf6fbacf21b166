"""GPU: components tracked through time, every output bit for bit against the oracle of track_cases.py - random boolean stacks through
label_images, hand-made label maps, scenes that stress the forest (late merges, a staircase, combs, checkerboards), more frames than a
grid dimension holds, short tables, the three relabel modes, reproducibility, stream order, composition with region_stats and recordings
read through IRMovie.track_hot_spots."""
import numpy as np
import pytest

import track_cases as TC
from test_region_stats_cpu import FIELDS, region_stats_oracle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

OUTPUTS = ("track_of", "first_frame", "last_frame", "first_label", "components")


def dev32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()


def dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda().view(torch.uint16)


def same(got, exp, what):
    got = got.cpu().numpy()
    assert got.dtype == exp.dtype and got.shape == exp.shape, (what, got.dtype, got.shape, exp.shape)
    if not np.array_equal(got, exp):
        bad = np.argwhere(got != exp)[:5]
        raise AssertionError("%s differs at %s: got %s, expected %s" % (what, bad.tolist(), got[tuple(bad.T)], exp[tuple(bad.T)]))


def check(res, exp, what="", tracks=True):
    for k in OUTPUTS:
        same(getattr(res, k), exp[k], (what, k))
    assert [int(res.ntracks), int(res.truncated)] == exp["info"].tolist(), (what, int(res.ntracks), int(res.truncated), exp["info"])
    assert res.ntracks.dtype == torch.int32 and res.ntracks.dim() == 0 and res.truncated.dim() == 0
    if tracks:
        same(res.tracks, exp["tracks"], (what, "tracks"))
    else:
        assert res.tracks is None


def label(mask):
    """(labels, counts) of a boolean stack, on the device"""
    from librir_amd import device as D

    m = torch.from_numpy(mask).cuda()
    parts = [D.label_images(m[i:i + 32768], table_entries=1) for i in range(0, len(m), 32768)]  # (a labelling call takes 65 535 frames at most)
    return torch.cat([p[0] for p in parts]), torch.cat([p[3] for p in parts])


def run_mask(mask, what, **kw):
    from librir_amd import device as D

    labels, counts = label(mask)
    lab, cnt = labels.cpu().numpy(), counts.cpu().numpy()
    k = int(cnt.max())
    res = D.track_components(labels, counts, **kw)
    exp = TC.track_oracle(lab, cnt, k, kw.get("table_entries"))
    check(res, exp, what)
    assert torch.equal(labels.cpu(), torch.from_numpy(lab))  # a separate destination leaves the labels alone
    return res, exp


# the shapes of the CPU test, the ones that cross a 64-frame run at n = 65 / 66 and 129 / 130, and the ones for wave and workgroup strips,
# tails that are no multiple of 4 and odd row lengths
SHAPES = TC.RANDOM_SHAPES + [(66, 5, 9), (129, 2, 3), (2, 33, 257), (3, 1, 1025), (2, 7, 4 * 64 * 4 + 3)]


@pytest.mark.parametrize("n,h,w", SHAPES)
def test_random_boolean_stacks(n, h, w):
    res, exp = run_mask(TC.random_mask(n * 1000 + w, n, h, w), (n, h, w))
    assert exp["info"][0] > 1 or n * h * w == 1


def test_random_boolean_stack_is_the_3d_labelling():
    ndi = pytest.importorskip("scipy.ndimage")
    mask = TC.random_mask(7, 70, 9, 67)
    res, _ = run_mask(mask, "scipy")
    structure = np.zeros((3, 3, 3), int)
    structure[1] = [[0, 1, 0], [1, 1, 1], [0, 1, 0]]
    structure[:, 1, 1] = 1
    exp, ntracks = ndi.label(mask, structure)
    assert int(res.ntracks) == ntracks + 1 and np.array_equal(res.tracks.cpu().numpy(), exp)


@pytest.mark.parametrize("n,h,w", [(5, 8, 16), (66, 5, 9), (3, 4, 7)])
def test_label_stack_one_element_off_a_16_byte_boundary(n, h, w):
    from librir_amd import device as D

    labels, counts = label(TC.random_mask(n + w, n, h, w))
    flat = torch.zeros(n * h * w + 1, dtype=torch.int32, device="cuda")
    view = flat[1:].view(n, h, w)
    view.copy_(labels)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    exp = TC.track_oracle(labels.cpu().numpy(), counts.cpu().numpy(), int(counts.max()))
    check(D.track_components(view, counts), exp, "offset view")
    res = D.track_components(view, counts, out=view)
    assert res.tracks.data_ptr() == view.data_ptr()
    check(res, exp, "offset view in place")
    assert int(flat[0]) == 0


@pytest.mark.parametrize("seed,n,h,w,nlabels,with_counts", [(1, 4, 6, 37, 9, True), (2, 70, 3, 5, 6, True), (3, 3, 17, 64, 300, True),
                                                            (4, 5, 6, 37, 9, False), (5, 67, 2, 9, 4, False), (6, 3, 5, 1023, 40, True)])
def test_hand_made_label_maps(seed, n, h, w, nlabels, with_counts):
    """negative labels, labels >= counts[t] and >= K, counts on both sides of K (or none): background by contract"""
    from librir_amd import device as D

    labels, counts = TC.random_labels(seed, n, h, w, nlabels, with_counts)
    exp = TC.track_oracle(labels, counts, nlabels)
    res = D.track_components(dev32(labels), None if counts is None else dev32(counts), nlabels)
    check(res, exp, (seed, n, h, w, nlabels))
    if with_counts:
        assert int(res.truncated) == int((counts > nlabels).sum())


def test_nlabels_below_the_counts_drops_components_that_then_link_nothing():
    """two columns through 6 frames; the second one is component 2: with K = 2 it is dropped in every frame, and a full frame in the
    middle (component 1) links only the first column's nodes"""
    from librir_amd import device as D

    mask = np.zeros((6, 3, 7), bool)
    mask[:, :, 1] = mask[:, :, 5] = True
    labels, counts = label(mask)
    lab, cnt = labels.cpu().numpy(), counts.cpu().numpy()
    assert cnt.tolist() == [3] * 6
    full = TC.track_oracle(lab, cnt, 3)
    check(D.track_components(labels, counts), full, "K = counts.max()")
    assert full["info"].tolist() == [3, 0] and full["components"][:3].tolist() == [0, 6, 6]
    cut = TC.track_oracle(lab, cnt, 2)
    res = D.track_components(labels, counts, nlabels=2)
    check(res, cut, "K = 2")
    assert cut["info"].tolist() == [2, 6] and int(res.truncated) == 6 and not (res.tracks[:, :, 5] != 0).any()


def test_counts_none_and_nlabels_none():
    from librir_amd import device as D

    labels, counts = label(TC.random_mask(3, 9, 6, 21))
    lab, cnt = labels.cpu().numpy(), counts.cpu().numpy()
    k = int(cnt.max())
    res = D.track_components(labels)  # K = labels.max() + 1 = counts.max(): every label below K exists in every frame
    assert res.track_of.shape == (9, k)
    check(res, TC.track_oracle(lab, None, k), "no counts")
    check(D.track_components(labels, counts), TC.track_oracle(lab, cnt, k), "counts")
    zero = torch.zeros((3, 4, 5), dtype=torch.int32, device="cuda")
    check(D.track_components(zero), TC.track_oracle(zero.cpu().numpy(), None, 1), "all background")


def test_one_label_value_is_all_background():
    from librir_amd import device as D

    labels, counts = TC.random_labels(9, 5, 4, 9, 3)
    exp = TC.track_oracle(labels, counts, 1)
    res = D.track_components(dev32(labels), dev32(counts), nlabels=1)
    check(res, exp, "K = 1")
    assert int(res.ntracks) == 1 and res.track_of.shape == (5, 1) and not res.tracks.any() and res.first_frame.tolist() == [-1]


def test_no_frames():
    from librir_amd import device as D

    res = D.track_components(torch.zeros((0, 4, 5), dtype=torch.int32, device="cuda"), nlabels=3, table_entries=4)
    assert [int(res.ntracks), int(res.truncated)] == [1, 0] and res.tracks.shape == (0, 4, 5) and res.track_of.shape == (0, 3)
    assert res.first_frame.tolist() == [-1, 0, 0, 0] and res.last_frame.tolist() == [-1, 0, 0, 0]
    assert res.first_label.tolist() == [0] * 4 and res.components.tolist() == [0] * 4


@pytest.mark.parametrize("m,n,joined_first", [(300, 40, False), (300, 40, True), (70, 131, False), (70, 131, True)])
def test_late_merge(m, n, joined_first):
    res, exp = run_mask(TC.late_merge(m, n, joined_first), ("late merge", m, n, joined_first))
    assert exp["info"].tolist() == [2, 0] and exp["components"][1] == m * (n - 1) + 1
    assert exp["first_frame"][1] == 0 and exp["last_frame"][1] == n - 1


def test_staircase():
    n, h, w = 150, 9, 23
    res, exp = run_mask(TC.staircase(n, h, w), "staircase")
    blob = exp["tracks"][0, 2, 0]
    assert exp["first_frame"][blob] == 0 and exp["last_frame"][blob] == n - 1 and exp["components"][blob] == n
    labels_of_blob = {int(np.flatnonzero(exp["track_of"][t] == blob)[0]) for t in range(n)}
    assert len(labels_of_blob) >= 4


@pytest.mark.parametrize("teeth_first", [True, False])
def test_comb(teeth_first):
    h, w = 3, 1030
    res, exp = run_mask(TC.comb(h, w, teeth_first), ("comb", teeth_first))
    assert exp["info"].tolist() == [2, 0] and exp["components"][1] == w // 2 + 1


def test_complementary_checkerboards():
    n, h, w = 5, 7, 33
    mask = TC.checkerboards(n, h, w)
    res, exp = run_mask(mask, "checkerboards", table_entries=n * h * w)
    assert int(res.ntracks) - 1 == int(mask.sum()) and exp["components"][1:int(res.ntracks)].tolist() == [1] * int(mask.sum())


def test_more_frames_than_a_grid_dimension():
    res, exp = run_mask(TC.random_mask(11, 70001, 3, 5), "70 001 frames")
    assert exp["last_frame"].max() > 65535


def test_short_tables():
    from librir_amd import device as D

    labels, counts = label(TC.random_mask(5, 12, 9, 31))
    lab, cnt = labels.cpu().numpy(), counts.cpu().numpy()
    k = int(cnt.max())
    ntracks = TC.track_oracle(lab, cnt, k)["info"][0]
    assert ntracks > 8
    for t in (1, 2, 8, ntracks - 1, ntracks, ntracks + 5):
        res = D.track_components(labels, counts, table_entries=t)
        assert res.first_frame.shape == (t,)
        check(res, TC.track_oracle(lab, cnt, k, t), ("table", t))


def test_relabel_modes():
    from librir_amd import device as D

    labels, counts = label(TC.random_mask(8, 20, 11, 45))
    lab, cnt = labels.cpu().numpy(), counts.cpu().numpy()
    exp = TC.track_oracle(lab, cnt, int(cnt.max()))
    check(D.track_components(labels, counts, relabel=False), exp, "relabel off", tracks=False)
    assert np.array_equal(labels.cpu().numpy(), lab)
    out = torch.full_like(labels, -7)
    res = D.track_components(labels, counts, out=out)
    assert res.tracks is out
    check(res, exp, "separate out")
    assert np.array_equal(labels.cpu().numpy(), lab)
    res = D.track_components(labels, counts, out=labels)
    assert res.tracks is labels
    check(res, exp, "in place")


def test_results_are_bit_identical_from_run_to_run():
    from librir_amd import device as D

    for mask in (TC.late_merge(300, 40, False), TC.late_merge(70, 131, True), TC.comb(3, 1030, True), TC.comb(3, 1030, False)):
        labels, counts = label(mask)
        runs = [D.track_components(labels, counts) for _ in range(5)]
        for r in runs[1:]:
            for a, b in zip(runs[0], r):
                assert torch.equal(a, b)
        check(runs[0], TC.track_oracle(labels.cpu().numpy(), counts.cpu().numpy(), int(counts.max())))


def test_on_a_side_stream():
    from librir_amd import device as D

    mask = TC.random_mask(21, 40, 24, 100)
    host = torch.from_numpy(mask).pin_memory()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        m = host.to("cuda", non_blocking=True)
        labels, _, _, counts = D.label_images(m, table_entries=1)
        res = D.track_components(labels, counts, nlabels=24 * 100 // 2 + 2)
    side.synchronize()
    lab, cnt = labels.cpu().numpy(), counts.cpu().numpy()
    check(res, TC.track_oracle(lab, cnt, 24 * 100 // 2 + 2), "side stream")


HOT_LEVEL = 4000  # between the background (below 2 100 in these scenes) and the discs (8 000 above it)


def hot_mask(t, level):
    return (t.view(torch.int16).to(torch.int32) & 0xFFFF) > level


def test_composition_with_region_stats():
    """region_stats over the track map is the time trace of every track"""
    from librir_amd import device as D
    from librir_amd.synthetic import hot_spots

    n = 40
    f = hot_spots(n, 48, 64, 3)
    t = dev16(f)
    labels, _, _, counts = D.label_images(hot_mask(t, HOT_LEVEL), table_entries=1)
    exp = TC.track_oracle(labels.cpu().numpy(), counts.cpu().numpy(), int(counts.max()))
    res = D.track_components(labels, counts)
    check(res, exp, "hot spots")
    ntracks = int(res.ntracks)
    assert ntracks >= 4
    rs = D.region_stats(t, res.tracks, ntracks)
    count = rs.count.cpu().numpy().astype(np.int64)
    assert np.array_equal(count.sum(0), exp["volume"])
    first, last = exp["first_frame"][:ntracks], exp["last_frame"][:ntracks]
    frame = np.arange(n)[:, None]
    assert np.array_equal(count[:, 1:] > 0, ((first[None, 1:] <= frame) & (frame <= last[None, 1:])))
    ro = region_stats_oracle(f, exp["tracks"], ntracks)
    for k, got in zip(FIELDS, rs):
        assert np.array_equal(got.cpu().numpy(), ro[k]), k


def record(path, frames):
    from librir_amd.video_io import IRSaver

    n, h, w = frames.shape
    with IRSaver(str(path), w, h, h) as s:
        for i in range(n):
            s.add_image(frames[i], i * 20000000 + 7)
    return str(path)


@pytest.fixture(scope="module")
def movie_file(tmp_path_factory):
    from librir_amd.synthetic import hot_spots

    return record(tmp_path_factory.mktemp("tracks") / "hot.h264", hot_spots(50, 40, 48, 2024))


@pytest.mark.parametrize("per_pixel", [False, True])
def test_movie_track_hot_spots(movie_file, per_pixel):
    from librir_amd.video_io import IRMovie

    h, w = 40, 48
    level = HOT_LEVEL + (np.arange(h * w).reshape(h, w) % 7 * 100 if per_pixel else 0)
    with IRMovie.from_filename(movie_file) as mov:
        mov._STATS_PIECE_BYTES = 11 * h * w * 2  # tracks cross piece borders
        for sel in (slice(None), slice(1, None, 2), slice(3, 45, 7)):
            frames = np.asarray(mov[sel])
            mask = frames > level
            threshold = level if per_pixel else int(level)
            tracks, stats = mov.track_hot_spots(torch.from_numpy(level).cuda() if per_pixel and sel.step == 7 else threshold, sel)
            labels, counts = label(mask)
            lab, cnt = labels.cpu().numpy(), counts.cpu().numpy()
            exp = TC.track_oracle(lab, cnt, max(1, int(cnt.max())))
            check(tracks, exp, ("movie", sel, per_pixel))
            ntracks = int(exp["info"][0])
            assert ntracks >= 2
            ro = region_stats_oracle(frames, exp["tracks"], ntracks)
            for k, got in zip(FIELDS, stats):
                got = got.cpu().numpy()
                assert got.dtype == ro[k].dtype and np.array_equal(got, ro[k]), (sel, k)
        tracks, stats = mov.track_hot_spots(HOT_LEVEL, slice(0, 20), table_entries=2, stats=False)
        assert stats is None and tracks.first_frame.shape == (2,) and tracks.tracks.shape == (20, h, w)
