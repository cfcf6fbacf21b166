"""GPU: the refusals of the analysis methods of ``IRMovie`` that need a device before they are reached - an ``out`` that does not fit, label
maps and threshold maps on the device of a wrong shape, ``nregions`` 0, shifts that do not match the selection, and the selections of the
region reducers, which take their map to the device first - against the "gpu" group of tests/golden/movie_analysis_messages.json (see
test_movie_analysis_messages_cpu.py); then the walk that all these methods read a recording with, ``IRMovie._pieces``.

``PYTHONPATH=. python tests/test_gpu_movie_analysis_messages.py`` on a machine with a device writes the "gpu" group anew and keeps the other."""
import json
import os

import numpy as np
import pytest

import test_movie_analysis_messages_cpu as C

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

N, H, W = 50, 40, 48


def record(path):
    from librir_amd.video_io import IRSaver

    frames = (np.arange(N * H * W, dtype=np.uint32) * 37 % 16000).astype(np.uint16).reshape(N, H, W)
    with IRSaver(str(path), W, H, H) as s:
        for i in range(N):
            s.add_image(frames[i], i * 20000000 + 7)
    return str(path)


@pytest.fixture(scope="module")
def movie(tmp_path_factory):
    from librir_amd.video_io import IRMovie

    with IRMovie.from_filename(record(tmp_path_factory.mktemp("messages") / "m.h264")) as mov:
        yield mov


def gpu_answers(m):
    """{"<method> <what is wrong>": [exception type, message]}"""
    bad = [0, 1]
    ten = slice(0, 10)
    calls = {}

    def cuda(shape, dtype):
        return torch.zeros(shape, dtype=dtype, device="cuda")

    # 'out': another dtype, another shape, not contiguous, on the host; with a second mistake
    for name, dtype, call in (("to_tensor", torch.uint16, lambda sel, out: m.to_tensor(sel, out=out)),
                              ("to_tensor, float32", torch.float32, lambda sel, out: m.to_tensor(sel, torch.float32, out)),
                              ("to_tensor, a window", torch.uint16, lambda sel, out: m.to_tensor(sel, out=out, window=(0, 0, H, W))),
                              ("to_tensor, temporal_median", torch.uint16, lambda sel, out: m.to_tensor(sel, out=out, temporal_median=3)),
                              ("morphology", torch.uint16, lambda sel, out: m.morphology("open", 3, sel, out=out)),
                              ("rank_filter", torch.uint16, lambda sel, out: m.rank_filter(4, 3, sel, out=out)),
                              ("window_median", torch.uint16, lambda sel, out: m.window_median(3, sel, out=out)),
                              ("local_threshold", torch.bool, lambda sel, out: m.local_threshold(3, 2, selection=sel, out=out)),
                              ("box_mean", torch.uint16, lambda sel, out: m.box_mean(3, sel, out=out))):
        other = torch.int32 if dtype != torch.int32 else torch.uint16
        for what, out in (("of another dtype", cuda((10, H, W), other)), ("of nine images", cuda((9, H, W), dtype)),
                          ("of another width", cuda((10, H, W + 1), dtype)), ("of one image", cuda((H, W), dtype)),
                          ("not contiguous", cuda((10, H, 2 * W), dtype)[:, :, ::2]), ("on the host", torch.zeros((10, H, W), dtype=dtype))):
            calls["%s out %s" % (name, what)] = lambda call=call, out=out: call(ten, out)
        calls["%s out of nine images, a list" % name] = lambda call=call, dtype=dtype: call(bad, cuda((9, H, W), dtype))
        calls["%s out for an empty selection, of one image" % name] = lambda call=call, dtype=dtype: call(slice(5, 5), cuda((1, H, W), dtype))
    calls["morphology out of nine images, size=4"] = lambda: m.morphology("open", 4, ten, out=cuda((9, H, W), torch.uint16))
    calls["local_threshold out of nine images, k=-1"] = lambda: m.local_threshold(3, -1, selection=ten, out=cuda((9, H, W), torch.bool))
    # label maps on the device
    for name, call in C.BY_LABELS.items():
        for what, lab in (("three maps", cuda((3, H, W), torch.int32)), ("ten maps", cuda((10, H, W), torch.int32)),
                          ("of another width", cuda((H, W + 1), torch.int32)), ("of another height", cuda((H - 1, W), torch.int32)),
                          ("a row", cuda((W,), torch.int32)), ("int64", cuda((H, W), torch.int64)), ("three maps, int64", cuda((3, H, W), torch.int64))):
            for k in (None, 4):
                calls["%s labels %s, nregions=%r" % (name, what, k)] = lambda call=call, lab=lab, k=k: call(m, lab, ten, k)
            calls["%s labels %s, a list" % (name, what)] = lambda call=call, lab=lab: call(m, lab, bad, 4)
            calls["%s labels %s, nregions=0" % (name, what)] = lambda call=call, lab=lab: call(m, lab, ten, 0)
        good = cuda((H, W), torch.int32)
        for k in (0, -1, 1 << 25):
            calls["%s nregions=%r" % (name, k)] = lambda call=call, k=k: call(m, good, ten, k)
            calls["%s nregions=%r, a list" % (name, k)] = lambda call=call, k=k: call(m, good, bad, k)
            calls["%s numpy labels, nregions=%r" % (name, k)] = lambda call=call, k=k: call(m, np.zeros((H, W), np.int32), ten, k)
        for what, lab in (("three maps", np.zeros((3, H, W), np.int32)), ("of another width", np.zeros((H, W + 1), np.int32))):
            calls["%s numpy labels %s" % (name, what)] = lambda call=call, lab=lab: call(m, lab, ten, None)
            calls["%s numpy labels %s, a list" % (name, what)] = lambda call=call, lab=lab: call(m, lab, bad, None)
        for what, sel in C.BAD_SELECTIONS.items():
            sel = N if what == "an int past the end" else -N - 1 if what == "an int before the start" else sel
            calls["%s selection: %s" % (name, what)] = lambda call=call, sel=sel: call(m, good, sel, None)
            calls["%s numpy labels, selection: %s" % (name, what)] = lambda call=call, sel=sel: call(m, np.zeros((H, W), np.int32), sel, 4)
    calls["region_stats_window labels of the image, a window"] = lambda: m.region_stats_window(cuda((H, W), torch.int32), (2, 2, 4, 4), ten)
    calls["region_stats_window three maps, a window"] = lambda: m.region_stats_window(cuda((3, 4, 4), torch.int32), (2, 2, 4, 4), ten)
    for what, sel in C.BAD_SELECTIONS.items():
        sel = N if what == "an int past the end" else -N - 1 if what == "an int before the start" else sel
        calls["histogram selection: %s" % what] = lambda sel=sel: m.histogram(16, 0, 4, sel)
        calls["background_levels selection: %s" % what] = lambda sel=sel: m.background_levels(sel)
        calls["region_histogram labels=None, nregions=3, selection: %s" % what] = lambda sel=sel: m.region_histogram(None, 16, 0, 4, sel, 3)
    for change in ({"nbins": 0}, {"nbins": 2.0}, {"lo": -1}, {"width": 0}, {"rows": H + 1}, {"nbins": 0, "selection": bad}, {"rows": H + 1, "selection": bad}):
        kw = dict({"nbins": 16, "lo": 0, "width": 4, "selection": ten, "rows": None}, **change)
        calls["histogram %s" % C.label(change)] = lambda kw=kw: m.histogram(**kw)
    calls["background_levels rows=%d" % (H + 1)] = lambda: m.background_levels(ten, H + 1)
    # shifts, one per image of the selection
    for what, shifts in (("three shifts", np.zeros((3, 2))), ("three shifts on the device", cuda((3, 2), torch.float64)), ("eleven shifts", np.zeros((11, 2))),
                         ("shifts of three columns", np.zeros((10, 3)))):
        calls["polygon_stats %s for ten images" % what] = lambda shifts=shifts: m.polygon_stats(C.TRIANGLE, ten, shifts)
        calls["polygon_stats %s, a list" % what] = lambda shifts=shifts: m.polygon_stats(C.TRIANGLE, bad, shifts)
    calls["polygon_stats three sets of polygons for ten images"] = lambda: m.polygon_stats([C.TRIANGLE] * 3, ten)
    calls["polygon_stats one shift for an empty selection"] = lambda: m.polygon_stats(C.TRIANGLE, slice(5, 5), np.zeros((1, 2)))
    # threshold maps
    for name in ("track_hot_spots", "track_hot_spots_geometry", "track_kept_hot_spots", "distance_transform"):
        for what, cut in (("of another width", cuda((H, W + 1), torch.int32)), ("three maps", cuda((3, H, W), torch.int32)),
                          ("numpy of another height", np.zeros((H + 1, W))), ("a row", np.zeros(W, np.int32)), ("a list", [1, 2])):
            calls["%s threshold %s" % (name, what)] = lambda name=name, cut=cut: getattr(m, name)(cut, ten)
            calls["%s threshold %s, a list" % (name, what)] = lambda name=name, cut=cut: getattr(m, name)(cut, bad)
            calls["%s threshold %s, an empty selection" % (name, what)] = lambda name=name, cut=cut: getattr(m, name)(cut, slice(5, 5))
    for name in ("track_hot_spots", "track_hot_spots_geometry", "track_kept_hot_spots"):
        calls["%s threshold of another width, table_entries=0" % name] = lambda name=name: getattr(m, name)(cuda((H, W + 1), torch.int32), ten, 0)
    calls["distance_transform threshold of another width, rows=%d" % (H + 1)] = lambda: m.distance_transform(cuda((H, W + 1), torch.int32), ten, rows=H + 1)
    return {key: C.raised(call) for key, call in calls.items()}


def test_refusals_on_the_device_are_worded_and_ordered_as_recorded(movie):
    with open(C.RECORD) as f:
        recorded = json.load(f)["gpu"]
    got = gpu_answers(movie)
    C.compare(got, recorded)
    assert not [k for k, v in got.items() if v[0] == "nothing raised"]


# ---- the walk -------------------------------------------------------------------------------------------------------------------------
def walk(mov, selection, piece_images, **kw):
    """(k0, k1) of every piece, after checks that hold for every walk: one buffer, the images of the selection"""
    device = torch.device("cuda", torch.cuda.current_device())
    window = kw.get("window")
    h, w = (H, W) if window is None else window[2:]
    mov._STATS_PIECE_BYTES = piece_images * h * w * kw.get("bytes_per_pixel", 2)
    want = mov.to_tensor(selection, window=window)
    spans, pointers = [], set()
    try:
        for k0, k1, frames in mov._pieces(mov._stats_positions(selection, "walk"), device, **kw):
            assert frames.dtype == torch.uint16 and frames.is_cuda and frames.is_contiguous() and tuple(frames.shape) == (k1 - k0, h, w)
            assert torch.equal(frames, want[k0:k1])
            spans.append((k0, k1))
            pointers.add(frames.data_ptr())
    finally:
        del mov._STATS_PIECE_BYTES  # (the class's again)
    assert len(pointers) <= 1
    return spans


def test_the_walk_cuts_a_selection_into_pieces_of_one_buffer(movie):
    assert walk(movie, slice(None), 11) == [(0, 11), (11, 22), (22, 33), (33, 44), (44, 50)]
    assert walk(movie, slice(3, 45, 7), 11) == [(0, 6)]
    assert walk(movie, 7, 11) == [(0, 1)] and walk(movie, slice(None, 22), 11) == [(0, 11), (11, 22)]
    assert walk(movie, slice(5, 5), 11) == [] and walk(movie, slice(7, 3), 1) == []
    assert walk(movie, slice(10, 13), 0) == [(0, 1), (1, 2), (2, 3)]  # (a budget below one image: one image a piece)


def test_the_walk_counts_in_window_bytes_and_in_the_bytes_a_pixel_costs(movie):
    window = (3, 5, 17, 29)
    assert walk(movie, slice(None), 11, window=window) == [(0, 11), (11, 22), (22, 33), (33, 44), (44, 50)]
    movie._STATS_PIECE_BYTES = 11 * H * W * 2  # (eleven whole images: 42 240 bytes, 42 windows of 17 x 29 x 2 = 986)
    try:
        device = torch.device("cuda", torch.cuda.current_device())
        assert [(k0, k1) for k0, k1, _ in movie._pieces(range(N), device, window)] == [(0, 42), (42, N)]
    finally:
        del movie._STATS_PIECE_BYTES
    assert walk(movie, slice(0, 20), 7, bytes_per_pixel=6) == [(0, 7), (7, 14), (14, 20)]  # (polygon_stats: an image and its int32 map)
    assert walk(movie, slice(0, 20), 21, bytes_per_pixel=6) == [(0, 20)]


def test_the_walk_reads_its_budget_when_called_and_every_piece_once(movie, monkeypatch):
    from librir_amd.video_io import IRMovie

    reads = []
    to_tensor = IRMovie.to_tensor
    monkeypatch.setattr(IRMovie, "to_tensor", lambda self, selection=slice(None), *a, **kw: reads.append(selection) or to_tensor(self, selection, *a, **kw))
    monkeypatch.setattr(IRMovie, "_STATS_PIECE_BYTES", 20 * H * W * 2)  # (on the class, as test_gpu_pixel_quantiles.py sets it)
    device = torch.device("cuda", torch.cuda.current_device())
    assert [(k0, k1) for k0, k1, _ in movie._pieces(range(1, N, 2), device)] == [(0, 20), (20, 25)]
    assert reads == [slice(1, 41, 2), slice(41, 51, 2)]
    del reads[:]
    assert list(movie._pieces(range(0), device)) == [] and reads == []


if __name__ == "__main__":
    import tempfile

    from librir_amd.video_io import IRMovie

    with tempfile.TemporaryDirectory() as d:
        with IRMovie.from_filename(record(os.path.join(d, "m.h264"))) as mov:
            C.write_group("gpu", gpu_answers(mov))
