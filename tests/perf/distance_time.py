"""Distance transform rate over 256 masks of 640x512 uint8 (GPU box), for three scenes - (a) hot spots above a threshold (sparse foreground),
(b) its inversion (the distance from everywhere to a few spots), (c) a half plane - with and without indices: frames/s of one
device.distance_transform call, ms, the share of the 8 TB/s HBM peak on the 5WH (9WH with indices) bytes a frame has to move (the mask
read once, each output written once; the workspace traffic is not counted), and the ratio to the yardstick, device.morphology(mask, "erode",
15) - the largest structuring element of the window filters - on the same stack in the same process.  Rounds alternate yardstick and
scenes; the figures are medians over the rounds, with the spread of the ratio.  scipy.ndimage.distance_transform_edt on the host, a few
frames, is the comparison row.
    python tests/perf/distance_time.py [--frames N] [--rounds R] [--reps K] [--no-scipy] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from librir_amd import device as D  # noqa: E402
from librir_amd.synthetic import hot_spots  # noqa: E402

PEAK_BYTES_PER_S = 8.0e12
H, W = 512, 640
SCENES = ("hot_spots", "inverted", "half_plane")
_scenes = {}


def scenes_of(n):
    """{scene: uint8 CUDA stack [n][512][640]}, shared by every measurement of the process; 32 different hot-spot frames, repeated"""
    if n not in _scenes:
        hot = np.tile((hot_spots(32) > 4000).astype(np.uint8), ((n + 31) // 32, 1, 1))[:n]
        half = np.zeros((n, H, W), np.uint8)
        half[:, :, W // 2:] = 1
        _scenes[n] = {"hot_spots": torch.from_numpy(hot).cuda(), "inverted": torch.from_numpy(1 - hot).cuda(), "half_plane": torch.from_numpy(half).cuda(),
                      "dist2": torch.empty((n, H, W), dtype=torch.int32, device="cuda"), "index": torch.empty((n, H, W), dtype=torch.int32, device="cuda")}
        _scenes[n]["eroded"] = torch.empty_like(_scenes[n]["hot_spots"])
    return _scenes[n]


def time_call(fn, reps):
    """seconds per call over reps calls between two events, after one warm-up call"""
    fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e-3 / reps


def measure(scene, indices, n, reps):
    """frames/s of device.distance_transform over n frames of `scene`; scene "yardstick:<scene>": of device.morphology(erode, 15) on it"""
    s = scenes_of(n)
    if scene.startswith("yardstick:"):
        return n / time_call(lambda: D.morphology(s[scene[10:]], "erode", 15, out=s["eroded"]), reps)
    out = (s["dist2"], s["index"]) if indices else s["dist2"]
    return n / time_call(lambda: D.distance_transform(s[scene], return_indices=indices, out=out), reps)


def rounds_of(n, rounds, reps, scenes=SCENES, index_forms=(False, True)):
    """[{(scene, indices): frames/s, ("yardstick", scene): frames/s} per round], yardstick and transform alternating"""
    out = []
    for _ in range(rounds):
        r = {}
        for scene in scenes:
            r["yardstick", scene] = measure("yardstick:" + scene, False, n, reps)
            for indices in index_forms:
                r[scene, indices] = measure(scene, indices, n, reps)
        out.append(r)
    return out


def summary(rs, scene, indices):
    """(median frames/s, median ratio to the yardstick, lowest and highest ratio of a round)"""
    ratios = [r[scene, indices] / r["yardstick", scene] for r in rs]
    return statistics.median(r[scene, indices] for r in rs), statistics.median(ratios), min(ratios), max(ratios)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--json")
    a = ap.parse_args()
    assert torch.cuda.is_available() and D.device_available(), "needs a GPU"
    n = a.frames
    rs = rounds_of(n, a.rounds, a.reps)
    rows = []
    print("%11s %8s %12s %8s %8s %12s %16s %22s" % ("scene", "indices", "frames/s", "ms", "of peak", "x erode 15", "(lowest..highest)", "erode 15x15 frames/s"))
    for scene in SCENES:
        yard = statistics.median(r["yardstick", scene] for r in rs)
        for indices in (False, True):
            rate, ratio, lo, hi = summary(rs, scene, indices)
            row = {"scene": scene, "indices": indices, "frames_per_s": rate, "ms": n / rate * 1e3,
                   "fraction_of_peak": rate * (9 if indices else 5) * H * W / PEAK_BYTES_PER_S, "ratio_to_erode_15": ratio, "ratio_lowest": lo,
                   "ratio_highest": hi, "erode_15_frames_per_s": yard}
            rows.append(row)
            print("%11s %8s %12.4g %8.3f %8.4f %12.3f %16s %22.4g" % (scene, indices, rate, row["ms"], row["fraction_of_peak"], ratio,
                                                                    "%.3f..%.3f" % (lo, hi), yard), flush=True)
    host = {}
    if not a.no_scipy:
        try:
            from scipy import ndimage
        except ImportError:
            ndimage = None
            print("scipy is not installed: no host row")
        if ndimage is not None:
            for scene in SCENES:
                frames = scenes_of(n)[scene][:4].cpu().numpy()
                t0 = time.perf_counter()
                for f in frames:
                    ndimage.distance_transform_edt(f)
                host[scene] = len(frames) / (time.perf_counter() - t0)
                print("scipy.ndimage.distance_transform_edt, %s, one core: %.4g frames/s" % (scene, host[scene]))
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"frames": n, "shape": [H, W], "rounds": a.rounds, "reps": a.reps, "peak_bytes_per_s": PEAK_BYTES_PER_S, "rows": rows,
                       "scipy_frames_per_s": host}, f, indent=1)


if __name__ == "__main__":
    main()
