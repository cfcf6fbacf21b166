"""Per-region geometry rate over 1 000 frames of 640x512 uint16 S1 frames (GPU box): frames/s and ms of one device.region_geometry call, the
algorithmic bytes (a shared map read once or a per-frame map read with each frame, the frames when they weigh, the outputs written once)
and their share of the 8 TB/s HBM peak, for
    shared maps  16 rectangles and 1 024 blobs, weighted by the frames
    per-frame    the hot-spot components of each frame above its 99.9th percentile, from label_images (K = the largest count), with and
                 without weights
and for comparison, on the same inputs,
    region_stats the seven statistics of device.region_stats over the same frames and maps
    torch        the same outputs with int64 scatter_add_ (count, five moments, three weighted sums) and scatter_reduce_ (the box), over
                 --torch-frames frames
    python tests/perf/region_geometry_time.py [--frames N] [--reps R] [--torch-frames T] [--no-torch] [--json out.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from librir_amd import device as D  # noqa: E402
from librir_amd.synthetic import s1_noisy_background  # noqa: E402

PEAK_BYTES_PER_S = 8.0e12
H, W = 512, 640
KINDS = ("rect16", "blob1024", "hotspots")


def rect_map(h, w, ny, nx):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((yy * ny // h) * nx + xx * nx // w).astype(np.int32)


def blob_map(h, w, k, seed):
    """k blobs: every pixel takes the nearest of k random centres (distances on the device)"""
    rng = np.random.default_rng(seed)
    c = torch.from_numpy(np.stack([rng.integers(0, h, k), rng.integers(0, w, k)], 1).astype(np.float32)).cuda()
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    p = torch.stack([yy.reshape(-1), xx.reshape(-1)], 1).float().cuda()
    lab = torch.cat([torch.cdist(p[i:i + 8192], c).argmin(1) for i in range(0, h * w, 8192)])
    return lab.view(h, w).to(torch.int32).cpu().numpy()


def algorithmic_bytes(n, npx, k, per_frame, weighted):
    return (n * npx * 2 if weighted else 0) + (n if per_frame else 1) * npx * 4 + n * k * (60 + (24 if weighted else 0))


def time_call(fn, reps):
    fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = 1e9
    for _ in range(reps):
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        best = min(best, start.elapsed_time(stop) * 1e-3)
    return best


def s1_frames(n):
    return torch.from_numpy(s1_noisy_background(n, H, W, seed=1).view(np.int16)).cuda().view(torch.uint16)


def hot_spot_maps(frames):
    """per-frame label maps: the components of each frame above its 99.9th percentile; -> (labels, K)"""
    n, npx = frames.shape[0], H * W
    v32 = frames.view(torch.int16).to(torch.int32) & 0xFFFF
    cut = torch.stack([f.reshape(-1).float().kthvalue(int(0.999 * npx)).values for f in v32])
    labels, _, _, counts = D.label_images(v32 > cut.view(n, 1, 1).to(torch.int32))
    return labels, int(counts.max())


def maps_of(kind, frames):
    if kind == "rect16":
        return torch.from_numpy(rect_map(H, W, 4, 4)).cuda(), 16
    if kind == "blob1024":
        return torch.from_numpy(blob_map(H, W, 1024, seed=1)).cuda(), 1024
    if kind == "hotspots":
        return hot_spot_maps(frames)
    raise ValueError(kind)


def measure(kind, weighted=True, n=1000, reps=10):
    """frames/s of one device.region_geometry call over n S1 frames: kind "rect16" or "blob1024" (a shared map; weighted only) or "hotspots"
    (per-frame maps from label_images; with the frames as weights or the maps alone)"""
    frames = s1_frames(n)
    labels, k = maps_of(kind, frames)
    if not weighted and labels.dim() != 3:
        raise ValueError("without weights a call takes per-frame maps")
    return n / time_call(lambda: D.region_geometry(labels, k, frames if weighted else None), reps)


def torch_route(frames64, labels, k, weighted):
    """count, box, moments and weighted sums per (frame, region) with int64 scatter_add_ and scatter_reduce_ (labels outside [0, k) go to a
    spill column).  A timing companion, not an oracle."""
    n = frames64.shape[0]
    lab = labels.reshape(labels.shape[0] if labels.dim() == 3 else 1, -1).long()
    lab = torch.where((lab >= 0) & (lab < k), lab, torch.full_like(lab, k)).expand(n, -1)
    idx = torch.arange(H * W, device=lab.device)
    x, y = (idx % W).expand(n, -1), (idx // W).expand(n, -1)
    v = frames64.reshape(n, -1)
    sums = [torch.ones_like(x), x, y, x * x, x * y, y * y] + ([v, v * x, v * y] if weighted else [])
    out = [torch.zeros((n, k + 1), dtype=torch.int64, device=lab.device).scatter_add_(1, lab, s)[:, :k] for s in sums]
    for src, op, init in [(x, "amin", 1 << 40), (y, "amin", 1 << 40), (x, "amax", -1), (y, "amax", -1)]:
        acc = torch.full((n, k + 1), init, dtype=torch.int64, device=lab.device)
        out.append(acc.scatter_reduce_(1, lab, src, op, include_self=True)[:, :k])
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
    frames64 = (frames[:tn].view(torch.int16).to(torch.int64) & 0xFFFF) if not a.no_torch else None
    rows = []
    print("%-28s %6s %12s %9s %8s %8s %14s %8s %16s" % ("workload", "K", "frames/s", "ms", "GB", "of peak", "torch frames/s", "speedup",
                                                       "region_stats f/s"))
    for kind in KINDS:
        labels, k = maps_of(kind, frames)
        per_frame = labels.dim() == 3
        t_stats = time_call(lambda: D.region_stats(frames, labels, k), a.reps)
        for weighted in (True, False) if per_frame else (True,):
            t = time_call(lambda: D.region_geometry(labels, k, frames if weighted else None), a.reps)
            nbytes = algorithmic_bytes(n, npx, k, per_frame, weighted)
            name = "%s, %s" % (kind, "weighted" if weighted else "labels only")
            row = {"workload": name, "K": k, "frames_per_s": n / t, "ms": t * 1e3, "bytes": nbytes, "fraction_of_peak": nbytes / t / PEAK_BYTES_PER_S,
                   "region_stats_frames_per_s": n / t_stats}
            tt = None
            if not a.no_torch:
                tl = labels[:tn] if per_frame else labels
                tt = time_call(lambda: torch_route(frames64, tl, k, weighted), max(1, a.reps // 3)) / tn
                row["torch_frames_per_s"] = 1 / tt
            rows.append(row)
            print("%-28s %6d %12.4g %9.3f %8.3f %8.3f %14s %8s %16.4g" % (name, k, n / t, t * 1e3, nbytes / 1e9, row["fraction_of_peak"],
                                                                         "%.4g" % (1 / tt) if tt else "-", "%.1fx" % (tt * n / t) if tt else "-",
                                                                         n / t_stats), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"frames": n, "shape": [H, W], "peak_bytes_per_s": PEAK_BYTES_PER_S, "torch_frames": tn, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
