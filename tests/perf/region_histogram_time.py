"""Per-region histogram rate over 1 000 frames of 640x512 uint16 S1 frames (GPU box): frames/s and ms of one device.region_histogram (or
device.histogram) call, the algorithmic bytes (the frames read once, a shared map read once or a per-frame map read with its frame: 2 bytes
a pixel without a map, 2-6 with one) and their share of the 8 TB/s HBM peak, beside them the bytes of the outputs that the call zeroes, for
    no map      device.histogram, K = 1
    K = 1       a shared map of zeros
    rect16      a shared map of 16 rectangles
    hotspots    per-frame maps: the components of each frame above its 99.9th percentile, from label_images (K = the largest count)
each at the bins (lo, width, nbins) = (0, 256, 256), (0, 4, 16384) and (7000, 1, 2048), and for comparison, on the same inputs,
    quantiles   device.region_quantiles at one percent (its first pass counts the bins (0, 256, 256)), where there is a map
    torch       torch.bincount of label * nbins + bin per frame, over --torch-frames frames
    python tests/perf/region_histogram_time.py [--frames N] [--reps R] [--torch-frames T] [--no-torch] [--json out.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from librir_amd import device as D  # noqa: E402
from region_quantiles_time import H, PEAK_BYTES_PER_S, W, hot_spot_maps, rect_map, s1_frames, time_call  # noqa: E402

BINS = {"coarse": (0, 256, 256), "background": (0, 4, 16384), "fine": (7000, 1, 2048)}  # name -> (lo, width, nbins)
KINDS = ("nomap", "one", "rect16", "hotspots")


def algorithmic_bytes(n, npx, labels):
    """the frames once, the map once (shared) or with every frame: 2 bytes a pixel without a map, 2-6 with one.  The outputs are not
    counted: they are reported beside it (output_bytes)"""
    maps = 0 if labels is None else (n if labels.dim() == 3 else 1) * npx * 4
    return n * npx * 2 + maps


def output_bytes(n, k, nbins):
    """count, hist and outside, which the call zeroes before it counts into them"""
    return n * k * (nbins + 3) * 4


def workload(kind, frames):
    """-> (labels or None, K)"""
    if kind == "nomap":
        return None, 1
    if kind == "one":
        return torch.zeros((H, W), dtype=torch.int32, device="cuda"), 1
    if kind == "rect16":
        return torch.from_numpy(rect_map(H, W, 4, 4)).cuda(), 16
    if kind == "hotspots":
        return hot_spot_maps(frames)
    raise ValueError(kind)


def call(frames, labels, k, bins):
    lo, width, nbins = bins
    if labels is None:
        return D.histogram(frames, nbins, lo, width)
    return D.region_histogram(frames, labels, nbins, lo, width, k)


def measure(kind, bins, n=1000, reps=10):
    """frames/s of one call over n S1 frames; kind in KINDS, bins = (lo, width, nbins).  kind "rect16" or "one" with bins "quantiles": the
    frames/s of device.region_quantiles(..., 0.5) on the same stack and map"""
    frames = s1_frames(n)
    labels, k = workload(kind, frames)
    if bins == "quantiles":
        return n / time_call(lambda: D.region_quantiles(frames, labels, (0.5,), k), reps)
    return n / time_call(lambda: call(frames, labels, k, bins), reps)


def measure_pair(kind, n=1000, reps=10):
    """in one run, on one stack and map, alternating: (seconds of region_histogram(..., 256, 0, 256), seconds of region_quantiles(..., 0.5)),
    the best of `reps` each"""
    frames = s1_frames(n)
    labels, k = workload(kind, frames)
    th = tq = 1e9
    for _ in range(2):
        th = min(th, time_call(lambda: call(frames, labels, k, BINS["coarse"]), reps))
        tq = min(tq, time_call(lambda: D.region_quantiles(frames, labels, (0.5,), k), reps))
    return th, tq


def torch_route(frames32, labels, k, bins):
    """one torch.bincount per frame of label * (nbins + 2) + slot (labels outside [0, k) dropped by a mask), into a preallocated
    [n][k][nbins + 2]: a timing companion, not an oracle"""
    lo, width, nbins = bins
    out = torch.empty((frames32.shape[0], k, nbins + 2), dtype=torch.int64, device=frames32.device)
    for i in range(frames32.shape[0]):
        v = frames32[i].reshape(-1)
        slot = torch.where(v < lo, torch.zeros_like(v), torch.clamp((v - lo) // width, max=nbins) + 1)
        if labels is None:
            key = slot
        else:
            lab = (labels[i] if labels.dim() == 3 else labels).reshape(-1).long()
            keep = (lab >= 0) & (lab < k)
            key = (lab * (nbins + 2) + slot)[keep]
        out[i] = torch.bincount(key, minlength=k * (nbins + 2)).view(k, nbins + 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-frames", type=int, default=100)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--json")
    a = ap.parse_args()
    assert torch.cuda.is_available() and D.device_available(), "needs a GPU"
    n, npx = a.frames, H * W
    frames = s1_frames(n)
    tn = min(n, a.torch_frames)
    frames32 = (frames[:tn].view(torch.int16).to(torch.int64) & 0xFFFF) if not a.no_torch else None
    rows = []
    print("%-10s %-11s %6s %6s %12s %9s %8s %8s %8s %14s %8s" % ("workload", "bins", "K", "nbins", "frames/s", "ms", "GB read", "of peak", "GB out",
                                                                "torch frames/s", "speedup"))
    for kind in KINDS:
        labels, k = workload(kind, frames)
        for name, bins in BINS.items():
            if n * k * (bins[2] + 3) * 4 > 4 << 30:  # (hot spots at 16 384 bins: tens of GB of counters that are nearly all zero)
                print("%-10s %-11s %6d %6d   outputs beyond 4 GiB: not timed" % (kind, name, k, bins[2]), flush=True)
                continue
            t = time_call(lambda: call(frames, labels, k, bins), a.reps)
            nbytes, out = algorithmic_bytes(n, npx, labels), output_bytes(n, k, bins[2])
            row = {"workload": kind, "bins": list(bins), "K": k, "frames_per_s": n / t, "ms": t * 1e3, "bytes": nbytes, "output_bytes": out,
                   "fraction_of_peak": nbytes / t / PEAK_BYTES_PER_S}
            tt = None
            if not a.no_torch:
                tl = labels[:tn] if labels is not None and labels.dim() == 3 else labels
                tt = time_call(lambda: torch_route(frames32, tl, k, bins), max(1, a.reps // 5)) / tn
                row["torch_frames_per_s"] = 1 / tt
            rows.append(row)
            print("%-10s %-11s %6d %6d %12.4g %9.3f %8.3f %8.3f %8.3f %14s %8s" % (kind, name, k, bins[2], n / t, t * 1e3, nbytes / 1e9,
                                                                                 row["fraction_of_peak"], out / 1e9, "%.4g" % (1 / tt) if tt else "-",
                                                                                 "%.1fx" % (tt * n / t) if tt else "-"), flush=True)
        if labels is not None:
            tq = time_call(lambda: D.region_quantiles(frames, labels, (0.5,), k), a.reps)
            rows.append({"workload": kind, "bins": "region_quantiles(0.5)", "K": k, "frames_per_s": n / tq, "ms": tq * 1e3})
            print("%-10s %-11s %6d %6s %12.4g %9.3f" % (kind, "quantiles", k, "-", n / tq, tq * 1e3), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"frames": n, "shape": [H, W], "peak_bytes_per_s": PEAK_BYTES_PER_S, "torch_frames": tn, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
