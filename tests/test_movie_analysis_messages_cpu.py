"""CPU: what the analysis methods of ``IRMovie`` answer to a call they refuse before any device work - the exception type and the full
message - equals the "cpu" group of the record tests/golden/movie_analysis_messages.json, which was made before the methods' read-in-pieces
loops, label intakes and selection parsers were merged.  The other tests ask only that a bad call is refused; this one pins the words and,
with the calls that are wrong in two ways at once, the order in which the conditions are tested.  The recording is a raw file read on the
host, so no device is needed; the refusals that need one are in test_gpu_movie_analysis_messages.py and the record's "gpu" group.

``PYTHONPATH=. python tests/test_movie_analysis_messages_cpu.py`` writes the "cpu" group anew from the library as it is and keeps the other."""
import json
import os

import numpy as np

RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "movie_analysis_messages.json")
N, H, W = 12, 12, 16

BAD_WINDOWS = {"three ints": (0, 0, 4), "a float": (0, 0, 4, 4.0), "an array": np.array([0, 0, 4, 4]), "no rows": (0, 0, 0, 4),
               "negative corner": (-1, 0, 4, 4), "past the last row": (9, 0, 4, 4), "past the last column": (0, 13, 4, 4)}
BAD_SELECTIONS = {"a list": [0, 1], "an int past the end": N, "an int before the start": -N - 1, "a negative step": slice(None, None, -1),
                  "a zero step": slice(0, 4, 0)}
TRIANGLE = [np.array([[1.0, 1.0], [9.0, 2.0], [4.0, 8.0]])]

# every method whose selection is parsed before the device is touched, in a call that is good but for the selection it is given
BY_SELECTION = {
    "to_tensor": lambda m, s: m.to_tensor(s),
    "to_tensor, temporal_median": lambda m, s: m.to_tensor(s, temporal_median=3),
    "polygon_stats": lambda m, s: m.polygon_stats(TRIANGLE, s),
    "pixel_stats": lambda m, s: m.pixel_stats(s),
    "pixel_stats_window": lambda m, s: m.pixel_stats_window((2, 2, 4, 4), s),
    "morphology": lambda m, s: m.morphology("open", 3, s),
    "rank_filter": lambda m, s: m.rank_filter(4, 3, s),
    "window_median": lambda m, s: m.window_median(3, s),
    "local_threshold": lambda m, s: m.local_threshold(3, 2, selection=s),
    "box_mean": lambda m, s: m.box_mean(3, s),
    "pixel_quantiles": lambda m, s: m.pixel_quantiles(0.5, s),
    "track_hot_spots": lambda m, s: m.track_hot_spots(100, s),
    "track_hot_spots_geometry": lambda m, s: m.track_hot_spots_geometry(100, s),
    "track_kept_hot_spots": lambda m, s: m.track_kept_hot_spots(100, s, min_area=2),
    "distance_transform": lambda m, s: m.distance_transform(100, s),
}
BY_WINDOW = {
    "to_tensor": lambda m, w, s: m.to_tensor(s, window=w),
    "region_stats_window": lambda m, w, s: m.region_stats_window(np.zeros((4, 4), np.int32), w, s),
    "pixel_stats_window": lambda m, w, s: m.pixel_stats_window(w, s),
}
# the four region reducers over one label map: (labels, selection, nregions)
BY_LABELS = {
    "region_stats": lambda m, lab, s, k: m.region_stats(lab, s, k),
    "region_stats_window": lambda m, lab, s, k: m.region_stats_window(lab, None, s, k),
    "region_geometry": lambda m, lab, s, k: m.region_geometry(lab, s, k),
    "region_quantiles": lambda m, lab, s, k: m.region_quantiles(lab, 0.5, s, k),
    "region_histogram": lambda m, lab, s, k: m.region_histogram(lab, 16, 0, 4, s, k),
}


def write_movie(path, n=N, h=H, w=W):
    """a raw recording of n images (h, w), which the host reads"""
    from librir_amd.video_io.IRMovie import create_pcr_header

    frames = (np.arange(n * h * w, dtype=np.uint32) * 37 % 16000).astype(np.uint16)
    with open(path, "wb") as f:
        f.write(create_pcr_header(h, w).astype(np.uint32).tobytes())
        f.write(frames.tobytes())
    return str(path)


def raised(call):
    try:
        call()
    except Exception as e:  # noqa: BLE001  (the type is what is recorded)
        return [type(e).__name__, str(e)]
    return ["nothing raised", ""]


def parameter_calls(m, all_images=slice(None)):
    """{"<method> <what is wrong>": call}: one bad parameter each, then two mistakes at once; none reaches the device"""
    import torch

    bad = [0, 1]  # (a selection that is refused)
    frames_out = torch.zeros((N, H, W), dtype=torch.uint16)  # (a CPU tensor: 'out' is refused for that alone)
    calls = {
        "to_tensor dtype=int32": lambda: m.to_tensor(dtype=torch.int32),
        "to_tensor dtype=int32, a list": lambda: m.to_tensor(bad, dtype=torch.int32),
        "to_tensor out on the host": lambda: m.to_tensor(out=frames_out),
        "to_tensor out on the host, a list": lambda: m.to_tensor(bad, out=frames_out),
        "to_tensor out on the host, a window": lambda: m.to_tensor(out=frames_out, window=(2, 2, 4, 4)),
        "to_tensor out on the host, float32": lambda: m.to_tensor(slice(2, 9, 3), dtype=torch.float32, out=frames_out),
        "polygon_stats values of another length": lambda: m.polygon_stats(TRIANGLE, values=[0, 1]),
        "polygon_stats three shifts for %d images" % N: lambda: m.polygon_stats(TRIANGLE, shifts=np.zeros((3, 2))),
        "polygon_stats three shifts, a list": lambda: m.polygon_stats(TRIANGLE, bad, shifts=np.zeros((3, 2))),
        "to_h264 downsample of one value": lambda: m.to_h264(str(m.filename) + ".h264", downsample=(2,)),
    }
    for tm in (2, 65, 0, "3"):
        calls["to_tensor temporal_median=%r" % (tm,)] = lambda tm=tm: m.to_tensor(temporal_median=tm)
    calls["to_tensor temporal_median=3, median_threshold=-1"] = lambda: m.to_tensor(temporal_median=3, median_threshold=-1)
    calls["to_tensor temporal_median=2, dtype=int32"] = lambda: m.to_tensor(temporal_median=2, dtype=torch.int32)
    calls["to_tensor temporal_median=2, a list"] = lambda: m.to_tensor(bad, temporal_median=2)
    for name, own, good in (("morphology", "op", "open"), ("rank_filter", "rank", 4)):
        for change in ({own: "median"}, {own: 9}, {own: None}, {"size": 4}, {"size": 17}, {"size": (3, 3, 3)}, {"size": 3.0}, {"rows": H + 1}, {"rows": -1},
                       {own: 99, "size": 4}, {"size": 4, "rows": H + 1}, {own: 99, "selection": bad}, {"size": 4, "selection": bad},
                       {"rows": H + 1, "selection": bad}, {"out": frames_out}, {"out": frames_out, "selection": bad}, {"out": frames_out, "size": 4}):
            kw = dict({own: good, "size": 3, "selection": all_images, "rows": None, "out": None}, **change)
            calls["%s %s" % (name, label(change))] = lambda name=name, own=own, kw=kw: getattr(m, name)(kw[own], kw["size"], kw["selection"], kw["rows"],
                                                                                                   kw["out"])
    for change in ({"size": 4}, {"size": 0}, {"size": (3, 3, 3)}, {"rows": H + 1}, {"size": 4, "selection": bad}, {"out": frames_out}):
        kw = dict({"size": 3, "selection": all_images, "rows": None, "out": None}, **change)
        calls["window_median %s" % label(change)] = lambda kw=kw: m.window_median(kw["size"], kw["selection"], kw["rows"], kw["out"])
        calls["box_mean %s" % label(change)] = lambda kw=kw: m.box_mean(kw["size"], kw["selection"], kw["rows"], kw["out"])
    mask_out = torch.zeros((N, H, W), dtype=torch.bool)
    for change in ({"size": 4}, {"size": 17}, {"k": -1}, {"k": 2.5}, {"k": (1, 0)}, {"k": (1, 2, 3)}, {"delta": 0.5}, {"delta": 65536},
                   {"polarity": "up"}, {"polarity": 1}, {"rows": H + 1}, {"size": 4, "k": -1}, {"k": -1, "polarity": "up"}, {"k": -1, "rows": H + 1},
                   {"polarity": "up", "selection": bad}, {"size": 4, "selection": bad}, {"out": mask_out}, {"out": mask_out, "selection": bad},
                   {"out": frames_out}):
        kw = dict({"size": 3, "k": 2, "delta": 0, "polarity": "above", "selection": all_images, "rows": None, "out": None}, **change)
        calls["local_threshold %s" % label(change)] = lambda kw=kw: m.local_threshold(**kw)
    for percents in (1.5, -0.1, [], [0.5] * 9, [[0.5]], "half", float("nan")):
        calls["pixel_quantiles percents=%r" % (percents,)] = lambda p=percents: m.pixel_quantiles(p)
    calls["pixel_quantiles percents=1.5, a list"] = lambda: m.pixel_quantiles(1.5, bad)
    for entries in (0, -1, "many", 1 << 40):
        for name in ("track_hot_spots", "track_hot_spots_geometry", "track_kept_hot_spots"):
            calls["%s table_entries=%r" % (name, entries)] = lambda name=name, e=entries: getattr(m, name)(100, table_entries=e)
    calls["track_hot_spots table_entries=0, a list"] = lambda: m.track_hot_spots(100, bad, table_entries=0)
    for change in ({"threshold": "hot"}, {"threshold": np.zeros((H, W + 1))}, {"threshold": np.zeros((2, H, W))},
                   {"high": np.zeros((H + 1, W))}, {"high": "hot"}, {"min_area": 0}, {"min_area": 2.0}, {"max_area": 0},
                   {"min_area": 5, "max_area": 4}, {"min_area": 0, "table_entries": 0},
                   {"min_area": 0, "selection": bad}, {"min_area": 0, "threshold": "hot"}, {"high": 50, "min_area": 0}):
        kw = dict({"threshold": 100, "selection": all_images}, **change)
        calls["track_kept_hot_spots %s" % label(change)] = lambda kw=kw: m.track_kept_hot_spots(**kw)
    for change in ({"rows": H + 1}, {"rows": -1}, {"border": 2}, {"border": "yes"}, {"border": 2, "rows": H + 1}, {"rows": H + 1, "selection": bad},
                   {"border": 2, "selection": bad}):
        kw = dict({"threshold": 100, "selection": all_images}, **change)
        calls["distance_transform %s" % label(change)] = lambda kw=kw: m.distance_transform(**kw)
    return calls


def label(change):
    def short(v):
        return "%s%s" % (type(v).__name__, tuple(v.shape)) if hasattr(v, "shape") else repr(v)

    return ",".join("%s=%s" % (k, short(v)) for k, v in change.items())


def label_calls(m):
    """{"<method> <what is wrong>": call}: label maps that are refused before they would go to the device - numpy maps that are not int32,
    and tensors on the host, which the checks of ``librir_amd.device`` see before they ask where a tensor lies"""
    import torch

    bad = [0, 1]
    calls = {}
    for name, call in BY_LABELS.items():
        for what, lab in (("int64", np.zeros((H, W), np.int64)), ("uint16", np.zeros((H, W), np.uint16)), ("float32", np.zeros((H, W), np.float32)),
                          ("int64, three maps", np.zeros((3, H, W), np.int64))):
            calls["%s numpy labels %s" % (name, what)] = lambda call=call, lab=lab: call(m, lab, slice(None), None)
            calls["%s numpy labels %s, a list" % (name, what)] = lambda call=call, lab=lab: call(m, lab, bad, None)
            calls["%s numpy labels %s, nregions=0" % (name, what)] = lambda call=call, lab=lab: call(m, lab, slice(None), 0)
        for what, lab in (("int32", torch.zeros((H, W), dtype=torch.int32)), ("int64", torch.zeros((H, W), dtype=torch.int64)),
                          ("three maps", torch.zeros((3, H, W), dtype=torch.int32)), ("of another width", torch.zeros((H, W + 1), dtype=torch.int32)),
                          ("of another height", torch.zeros((H - 1, W), dtype=torch.int32)), ("a row", torch.zeros((W,), dtype=torch.int32))):
            for k in (None, 4, 0, -1, 2.0):
                calls["%s host tensor labels %s, nregions=%r" % (name, what, k)] = lambda call=call, lab=lab, k=k: call(m, lab, slice(None), k)
            calls["%s host tensor labels %s, a list" % (name, what)] = lambda call=call, lab=lab: call(m, lab, bad, 4)
    host = torch.zeros((H, W), dtype=torch.int32)
    calls["region_stats_window host tensor labels of the image, a window"] = lambda: m.region_stats_window(host, (2, 2, 4, 4))
    calls["region_stats_window int64 labels, a bad window"] = lambda: m.region_stats_window(np.zeros((H, W), np.int64), (0, 0, 4))
    for percents in (1.5, [], [0.5] * 9):
        calls["region_quantiles percents=%r" % (percents,)] = lambda p=percents: m.region_quantiles(host, p)
        calls["region_quantiles percents=%r, int64 labels" % (percents,)] = lambda p=percents: m.region_quantiles(np.zeros((H, W), np.int64), p)
    for change in ({"nbins": 0}, {"nbins": 2.0}, {"nbins": 1 << 17}, {"lo": -1}, {"lo": 65536}, {"width": 0}, {"width": 65537}, {"rows": H + 1}, {"rows": -1},
                   {"nbins": 0, "rows": H + 1}, {"nbins": 0, "nregions": 0}, {"nbins": 65536, "nregions": 257}, {"nbins": 0, "selection": bad},
                   {"nbins": 0, "labels": np.zeros((H, W), np.int64)}, {"nbins": 0, "labels": torch.zeros((3, H, W), dtype=torch.int32)}):
        kw = dict({"labels": host, "nbins": 16, "lo": 0, "width": 4, "selection": slice(None), "nregions": 4, "rows": None}, **change)
        calls["region_histogram %s" % label(change)] = lambda kw=kw: m.region_histogram(**kw)
    return calls


def cpu_answers(path):
    from librir_amd.video_io import IRMovie

    out = {}
    with IRMovie.from_filename(path) as m:
        for name, call in BY_SELECTION.items():
            for what, sel in BAD_SELECTIONS.items():
                out["%s selection: %s" % (name, what)] = raised(lambda: call(m, sel))
        for name, call in BY_WINDOW.items():
            for what, window in BAD_WINDOWS.items():
                out["%s window: %s" % (name, what)] = raised(lambda: call(m, window, slice(None)))
            out["%s window: three ints, selection: a list" % name] = raised(lambda: call(m, (0, 0, 4), [0, 1]))
            out["%s window: past the last row, selection: a negative step" % name] = raised(lambda: call(m, (9, 0, 4, 4), slice(None, None, -1)))
        out["to_tensor window: three ints, dtype=int32"] = raised(lambda: m.to_tensor(dtype=np.int32, window=(0, 0, 4)))
        out["to_tensor window: three ints, temporal_median=2"] = raised(lambda: m.to_tensor(temporal_median=2, window=(0, 0, 4)))
        for key, call in list(parameter_calls(m).items()) + list(label_calls(m).items()):
            assert key not in out, key
            out[key] = raised(call)
    return out


def compare(got, recorded):
    assert sorted(got) == sorted(recorded)
    different = {k: (v, recorded[k]) for k, v in got.items() if v != recorded[k]}
    assert not different, different


def write_group(group, answers):
    """the record with `group` replaced by `answers`"""
    record = {}
    if os.path.exists(RECORD):
        with open(RECORD) as f:
            record = json.load(f)
    record[group] = answers
    with open(RECORD, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")


def test_refusals_before_the_device_are_worded_and_ordered_as_recorded(tmp_path):
    with open(RECORD) as f:
        recorded = json.load(f)["cpu"]
    got = cpu_answers(write_movie(tmp_path / "m.pcr"))
    compare(got, recorded)
    assert not [k for k, v in got.items() if v[0] == "nothing raised"]


if __name__ == "__main__":
    import tempfile

    with tempfile.TemporaryDirectory() as d:
        write_group("cpu", cpu_answers(write_movie(os.path.join(d, "m.pcr"))))
