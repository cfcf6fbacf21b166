"""Per-region quantile rate over 1 000 frames of 640x512 uint16 S1 frames (GPU box): frames/s and ms of one device.region_quantiles call at
percents (0.5,) and (0.25, 0.5, 0.75, 0.99), the algorithmic bytes (two passes over the frames, each with a shared map read once or a
per-frame map read with its frame, the outputs written once) and their share of the 8 TB/s HBM peak, for
    shared maps  K = 1, 16 rectangles and 1 024 blobs
    per-frame    the components of each frame above its 99.9th percentile, from label_images (K = the largest count)
and for comparison, on the same inputs,
    the loop     K device.find_median_pixel(frames, p, mask_r) calls with the masks built beforehand (16 rectangles, one percent)
    torch        one sort per frame of the keys label << 16 | value and a gather at each region's rank, over --torch-frames frames
    python tests/perf/region_quantiles_time.py [--frames N] [--reps R] [--torch-frames T] [--no-torch] [--no-loop] [--json out.json]"""
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
ONE, FOUR = (0.5,), (0.25, 0.5, 0.75, 0.99)


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


def algorithmic_bytes(n, npx, k, q, per_frame):
    return 2 * (n * npx * 2 + (n if per_frame else 1) * npx * 4) + n * k * 4 * (1 + q)


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


def measure(kind, percents, n=1000, reps=10):
    """frames/s of one device.region_quantiles call over n S1 frames: kind "rect16" (a shared map of 16 rectangles) or "hotspots" (per-frame
    maps from label_images)"""
    frames = s1_frames(n)
    if kind == "rect16":
        labels, k = torch.from_numpy(rect_map(H, W, 4, 4)).cuda(), 16
    elif kind == "hotspots":
        labels, k = hot_spot_maps(frames)
    else:
        raise ValueError(kind)
    return n / time_call(lambda: D.region_quantiles(frames, labels, percents, k), reps)


def torch_route(frames32, labels, k, percents):
    """values per (frame, region, percent) by one sort per frame of label << 16 | value (labels outside [0, k) sort last) and a gather at
    start + t - 1; the rank as the library computes it.  No 65535 rule: a timing companion, not an oracle."""
    n = frames32.shape[0]
    lab = labels.reshape(labels.shape[0] if labels.dim() == 3 else 1, -1).long()
    lab = torch.where((lab >= 0) & (lab < k), lab, torch.full_like(lab, k)).expand(n, -1)
    keys = (lab << 16 | frames32.reshape(n, -1)).sort(1).values
    count = torch.zeros((n, k + 1), dtype=torch.int64, device=keys.device).scatter_add_(1, lab, torch.ones_like(lab))[:, :k]
    start = count.cumsum(1) - count
    out = []
    for p in percents:
        t = torch.floor((count.float() * p).double() + 0.5).long()
        at = (start + t - 1).clamp(0, keys.shape[1] - 1)
        out.append(torch.where((t >= 1) & (t <= count), keys.gather(1, at) & 0xFFFF, torch.zeros_like(t)))
    return count, torch.stack(out, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-frames", type=int, default=100)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-loop", action="store_true")
    ap.add_argument("--json")
    a = ap.parse_args()
    assert torch.cuda.is_available() and D.device_available(), "needs a GPU"
    n, npx = a.frames, H * W
    frames = s1_frames(n)
    tn = min(n, a.torch_frames)
    frames32 = (frames[:tn].view(torch.int16).to(torch.int64) & 0xFFFF) if not a.no_torch else None
    hot, khot = hot_spot_maps(frames)
    work = [("shared, K=1", torch.zeros((H, W), dtype=torch.int32, device="cuda"), 1), ("shared, 16 rectangles", torch.from_numpy(rect_map(H, W, 4, 4)).cuda(), 16),
            ("shared, 1024 blobs", torch.from_numpy(blob_map(H, W, 1024, seed=1)).cuda(), 1024), ("per-frame, label_images", hot, khot)]
    rows = []
    print("%-26s %6s %2s %12s %9s %8s %8s %14s %8s" % ("workload", "K", "Q", "frames/s", "ms", "GB", "of peak", "torch frames/s", "speedup"))
    for name, labels, k in work:
        for pc in (ONE, FOUR):
            t = time_call(lambda: D.region_quantiles(frames, labels, pc, k), a.reps)
            nbytes = algorithmic_bytes(n, npx, k, len(pc), labels.dim() == 3)
            row = {"workload": name, "K": k, "percents": list(pc), "frames_per_s": n / t, "ms": t * 1e3, "bytes": nbytes,
                   "fraction_of_peak": nbytes / t / PEAK_BYTES_PER_S}
            tt = None
            if not a.no_torch:
                tl = labels[:tn] if labels.dim() == 3 else labels
                tt = time_call(lambda: torch_route(frames32, tl, k, pc), max(1, a.reps // 3)) / tn
                row["torch_frames_per_s"] = 1 / tt
            rows.append(row)
            print("%-26s %6d %2d %12.4g %9.3f %8.3f %8.3f %14s %8s" % (name, k, len(pc), n / t, t * 1e3, nbytes / 1e9, row["fraction_of_peak"],
                                                                      "%.4g" % (1 / tt) if tt else "-", "%.1fx" % (tt * n / t) if tt else "-"), flush=True)
    loop = None
    if not a.no_loop:
        labels = work[1][1]
        masks = [(labels == r).to(torch.uint8).expand(n, H, W).contiguous() for r in range(16)]
        t_loop = time_call(lambda: [D.find_median_pixel(frames, 0.5, m) for m in masks], max(1, a.reps // 3))
        t_new = time_call(lambda: D.region_quantiles(frames, labels, ONE, 16), a.reps)
        same = torch.equal(torch.stack([D.find_median_pixel(frames, 0.5, m) for m in masks], 1), D.region_quantiles(frames, labels, ONE, 16).values[:, :, 0])
        loop = {"find_median_pixel_loop_ms": t_loop * 1e3, "region_quantiles_ms": t_new * 1e3, "speedup": t_loop / t_new, "same_values": bool(same)}
        print("16 rectangles, p = 0.5: 16 find_median_pixel calls %.3f ms, one region_quantiles call %.3f ms (%.1fx), same values: %s"
              % (t_loop * 1e3, t_new * 1e3, t_loop / t_new, same))
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"frames": n, "shape": [H, W], "peak_bytes_per_s": PEAK_BYTES_PER_S, "torch_frames": tn, "rows": rows, "loop": loop}, f, indent=1)


if __name__ == "__main__":
    main()
