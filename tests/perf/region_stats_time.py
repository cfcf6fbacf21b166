"""Per-region statistics rate over 1 000 frames of 640x512 uint16 S1 frames (GPU box): frames/s and ms of one device.region_stats call,
the algorithmic bytes (the frames read once, a shared map read once or a per-frame map with each frame, the seven outputs written once) and
their share of the 8 TB/s HBM peak, for
    shared maps  K = 1, 16 rectangles, 1 024 and 4 096 blobs (LDS form), 4 097 and 8 192 blobs (above the form threshold: global form)
    per-frame    the components of each frame above its 99.9th percentile, from label_images (K = the largest count)
    recording    IRMovie.region_stats over a 1 000-frame recording with 16 rectangles, against IRMovie.to_tensor alone
and for comparison the torch route on the shared maps: int64 scatter_reduce of sum, sum of squares, amax and amin (no argmax).
    python tests/perf/region_stats_time.py [--frames N] [--reps R] [--no-torch] [--no-movie] [--json out.json]"""
import argparse
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from librir_amd import device as D  # noqa: E402
from librir_amd.synthetic import s1_noisy_background  # noqa: E402

PEAK_BYTES_PER_S = 8.0e12
H, W = 512, 640


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


def algorithmic_bytes(n, npx, k, per_frame):
    return n * npx * 2 + (n if per_frame else 1) * npx * 4 + n * k * 36


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


def torch_route(frames32, labels, k):
    """sum, sum of squares, max and min per (frame, region) with int64 scatter_reduce (labels outside [0, k) go to a spill column)"""
    n = frames32.shape[0]
    lab = labels.reshape(-1).long()
    lab = torch.where((lab >= 0) & (lab < k), lab, torch.full_like(lab, k)).expand(n, -1)
    v = frames32.reshape(n, -1)
    out = []
    for src, op, init in [(v, "sum", 0), (v * v, "sum", 0), (v, "amax", -1), (v, "amin", 1 << 40)]:
        acc = torch.full((n, k + 1), init, dtype=torch.int64, device=v.device)
        out.append(acc.scatter_reduce_(1, lab, src, op, include_self=True)[:, :k])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-movie", action="store_true")
    ap.add_argument("--json")
    a = ap.parse_args()
    assert torch.cuda.is_available() and D.device_available(), "needs a GPU"
    n, npx = a.frames, H * W
    host = s1_noisy_background(n, H, W, seed=1)
    frames = torch.from_numpy(host.view(np.int16)).cuda().view(torch.uint16)
    frames32 = torch.from_numpy(host.astype(np.int64)).cuda() if not a.no_torch else None
    shared = [("K=1", np.zeros((H, W), np.int32), 1), ("16 rectangles", rect_map(H, W, 4, 4), 16),
              ("1024 blobs", blob_map(H, W, 1024, seed=1), 1024), ("4096 blobs", blob_map(H, W, 4096, seed=2), 4096),
              ("4097 blobs", blob_map(H, W, 4097, seed=2), 4097), ("8192 blobs", blob_map(H, W, 8192, seed=3), 8192)]
    rows = []
    print("%-26s %6s %12s %9s %8s %8s %14s %8s" % ("workload", "K", "frames/s", "ms", "GB", "of peak", "torch frames/s", "speedup"))

    def report(name, k, t, nbytes, tt=None):
        row = {"workload": name, "K": k, "frames_per_s": n / t, "ms": t * 1e3, "bytes": nbytes, "fraction_of_peak": nbytes / t / PEAK_BYTES_PER_S}
        if tt is not None:
            row["torch_frames_per_s"] = n / tt
        rows.append(row)
        print("%-26s %6d %12.4g %9.3f %8.3f %8.3f %14s %8s" % (name, k, n / t, t * 1e3, nbytes / 1e9, row["fraction_of_peak"],
                                                              "%.4g" % (n / tt) if tt else "-", "%.1fx" % (tt / t) if tt else "-"), flush=True)

    for name, lab, k in shared:
        labels = torch.from_numpy(lab).cuda()
        t = time_call(lambda: D.region_stats(frames, labels, k), a.reps)
        tt = None
        if not a.no_torch:
            tt = time_call(lambda: torch_route(frames32, labels, k), max(1, a.reps // 3))
        report("shared, " + name, k, t, algorithmic_bytes(n, npx, k, False), tt)
    # per-frame maps: the components of each thresholded frame
    v32 = frames.view(torch.int16).to(torch.int32) & 0xFFFF
    cut = torch.stack([f.reshape(-1).float().kthvalue(int(0.999 * npx)).values for f in v32])  # each frame's 99.9th percentile
    hot = v32 > cut.view(n, 1, 1).to(torch.int32)
    del v32
    labels, _, _, counts = D.label_images(hot)
    k = int(counts.max())
    t = time_call(lambda: D.region_stats(frames, labels, k), a.reps)
    report("per-frame, label_images", k, t, algorithmic_bytes(n, npx, k, True))
    if not a.no_movie:
        from librir_amd.video_io import IRMovie, IRSaver

        lab = rect_map(H, W, 4, 4)
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "m.h264")
            with IRSaver(path, W, H, H) as s:
                s.add_images(frames, np.arange(n, dtype=np.int64) * 1000)
            with IRMovie.from_filename(path) as mov:
                labels = torch.from_numpy(lab).cuda()
                out = torch.empty((n, H, W), dtype=torch.uint16, device="cuda")
                t_read = time_call(lambda: mov.to_tensor(out=out), max(1, a.reps // 2))
                t = time_call(lambda: mov.region_stats(labels, nregions=16), max(1, a.reps // 2))
        report("recording, to_tensor only", 0, t_read, n * npx * 2)
        report("recording, region_stats", 16, t, algorithmic_bytes(n, npx, 16, False))
        rows[-1]["over_to_tensor"] = t / t_read
        print("IRMovie.region_stats / to_tensor alone: %.3f" % (t / t_read))
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"frames": n, "shape": [H, W], "peak_bytes_per_s": PEAK_BYTES_PER_S, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
