"""Hot spots labelled straight from the frames, over 1 000 frames of 640x512 (GPU box): ms of one device.label_hot_spots call against the
only ways to the same maps that existed before it, timed in the same run and in turns with it (the median of each over the turns):
    (a) no filter     label_hot_spots(f, 4000) against the three torch passes of IRMovie.track_hot_spots' mask,
                      (f.view(int16).to(int32) & 0xFFFF) > 4000, and label_images on it - the same maps, fewer bytes
    (b) four filters  label_hot_spots(f, low, high, min_area, max_area, clear_border) against that mask and label_images, per-label strong
                      and border flags by scatter_reduce, the area test on label_images' table, new numbers by cumsum and a gather - the
                      two results are compared bit for bit first
    (c) noise         synthetic.s1_noisy_background without its ramp (frame i minus i: the scene's level rises by one count a frame),
                      low = one count above every pixel's median over time: specks.  Components a frame and the track_components rate on
                      the maps, without filters and with min_area=4, high=low+3.  Reported only.
    python tests/perf/hot_spot_label_time.py [--frames N] [--turns T] [--parts a,b,c] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from librir_amd import device as D  # noqa: E402
from librir_amd.synthetic import hot_spots, s1_noisy_background  # noqa: E402

H, W = 512, 640
LOW = 4000
FILTERS = dict(high=9000, min_area=4, max_area=5000, clear_border=True)


def on_device(frames):
    return torch.from_numpy(frames.view(np.int16)).cuda().view(torch.uint16)


def as_int32(frames):
    return frames.view(torch.int16).to(torch.int32) & 0xFFFF


def in_turns(calls, turns):
    """the calls timed one after the other, `turns` times over, with device events; -> the median seconds of each"""
    for fn in calls:
        fn()
    torch.cuda.synchronize()
    times = [[] for _ in calls]
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(turns):
        for k, fn in enumerate(calls):
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            times[k].append(start.elapsed_time(stop) * 1e-3)
    return [statistics.median(t) for t in times]


def mask_and_label(f, low, table_entries=1):
    """the route of IRMovie.track_hot_spots: the mask by three torch passes, then label_images"""
    return D.label_images(as_int32(f) > low, table_entries=table_entries)


def torch_filters(f, low, cap, high, min_area, max_area, clear_border):
    """(labels, counts) of the kept components from calls that existed before label_hot_spots; cap: at least the largest count of a frame"""
    n, h, w = f.shape
    v = as_int32(f)
    labels, area, _, counts = D.label_images(v > low, table_entries=cap)
    flat = labels.view(n, -1).long()
    strong = torch.zeros((n, cap), dtype=torch.int32, device=f.device).scatter_reduce_(1, flat, (v > high).view(n, -1).to(torch.int32), "amax")
    edge = torch.zeros((h, w), dtype=torch.int32, device=f.device)
    edge[0] = edge[-1] = edge[:, 0] = edge[:, -1] = 1
    touches = torch.zeros((n, cap), dtype=torch.int32, device=f.device).scatter_reduce_(1, flat, edge.view(1, -1).expand(n, -1), "amax")
    keep = (area >= min_area) & (area <= max_area) & (strong > 0)
    if clear_border:
        keep &= touches == 0
    keep[:, 0] = False
    number = (torch.cumsum(keep, 1) * keep).to(torch.int32)
    return number.gather(1, flat).view(n, h, w), (keep.sum(1) + 1).to(torch.int32)


def no_filters(f, turns):
    """(a) -> (seconds of the mask and label_images, seconds of label_hot_spots)"""
    old, new = mask_and_label(f, LOW), D.label_hot_spots(f, LOW, table_entries=1)
    assert torch.equal(old[0], new[0]) and torch.equal(old[3], new[3]), "label_hot_spots differs from label_images of the mask"
    del old, new
    return in_turns([lambda: mask_and_label(f, LOW), lambda: D.label_hot_spots(f, LOW, table_entries=1)], turns)


def four_filters(f, turns):
    """(b) -> (seconds of the torch route, seconds of label_hot_spots, kept components a frame); the two results are equal bit for bit"""
    cap = int(mask_and_label(f, LOW)[3].max())
    old, new = torch_filters(f, LOW, cap, **FILTERS), D.label_hot_spots(f, LOW, table_entries=1, **FILTERS)
    assert torch.equal(old[0], new[0]) and torch.equal(old[1], new[3]), "label_hot_spots differs from the torch route"
    kept = float((new[3] - 1).float().mean())
    assert kept > 0 and int(new[3].sum()) < int(mask_and_label(f, LOW)[3].sum()), "the filters keep and drop components"
    del old, new
    t = in_turns([lambda: torch_filters(f, LOW, cap, **FILTERS), lambda: D.label_hot_spots(f, LOW, table_entries=1, **FILTERS)], turns)
    return t[0], t[1], kept


def noise(n, turns):
    """(c) -> rows (what, components a frame, seconds of label_hot_spots, seconds of track_components without the track map)"""
    host = s1_noisy_background(n, H, W, seed=1)
    host -= np.arange(n, dtype=np.uint16).reshape(n, 1, 1)
    f = on_device(host)
    low = D.pixel_quantiles(f, 0.5)[0] + 1
    rows = []
    for what, kw in (("no filter", {}), ("min_area=2", dict(min_area=2)), ("min_area=4, high=low+3", dict(min_area=4, high=low + 3))):
        labels, _, _, counts = D.label_hot_spots(f, low, table_entries=1, **kw)
        k = max(1, int(counts.max()))
        t_label, t_track = in_turns([lambda: D.label_hot_spots(f, low, table_entries=1, **kw),
                                     lambda: D.track_components(labels, counts, k, relabel=False)], turns)
        rows.append((what, float((counts - 1).float().mean()), t_label, t_track))
        del labels
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--turns", type=int, default=9)
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--json")
    a = ap.parse_args()
    assert torch.cuda.is_available() and D.device_available(), "needs a GPU"
    n, parts, out = a.frames, a.parts.split(","), {"frames": a.frames, "shape": [H, W]}
    if "a" in parts or "b" in parts:
        f = on_device(hot_spots(n, H, W))
        if "a" in parts:
            old, new = no_filters(f, a.turns)
            out["no_filter"] = {"mask_and_label_images_ms": old * 1e3, "label_hot_spots_ms": new * 1e3, "ratio": old / new}
            print("(a) no filter:    mask + label_images %.3f ms, label_hot_spots %.3f ms (%.4g frames/s), ratio %.3f"
                  % (old * 1e3, new * 1e3, n / new, old / new), flush=True)
        if "b" in parts:
            old, new, kept = four_filters(f, a.turns)
            out["four_filters"] = {"torch_route_ms": old * 1e3, "label_hot_spots_ms": new * 1e3, "ratio": old / new, "kept_per_frame": kept}
            print("(b) four filters: torch route %.3f ms, label_hot_spots %.3f ms (%.4g frames/s), ratio %.3f, %.2f kept components a frame"
                  % (old * 1e3, new * 1e3, n / new, old / new, kept), flush=True)
        del f
    if "c" in parts:
        out["noise"] = []
        for what, per_frame, t_label, t_track in noise(n, a.turns):
            out["noise"].append({"what": what, "components_per_frame": per_frame, "label_hot_spots_ms": t_label * 1e3,
                                 "track_components_frames_per_s": n / t_track})
            print("(c) noise, %-24s %9.1f components a frame, label_hot_spots %.3f ms, track_components %.4g frames/s"
                  % (what + ":", per_frame, t_label * 1e3, n / t_track), flush=True)
    if a.json:
        with open(a.json, "w") as fp:
            json.dump(out, fp, indent=1)


if __name__ == "__main__":
    main()
