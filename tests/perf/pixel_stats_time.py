"""Per-pixel statistics rate over 1 000 frames of 640x512 uint16 S1 frames in one call (GPU box): frames/s and ms of device.pixel_stats
for the three forms (both groups, sums only, extremes only), the bytes moved (the frames read once, the partials of the slabs written and
read once where the stack is cut along time, the outputs of the form written once) and their share of the 8 TB/s HBM peak; then
    yardstick    device.region_stats with K = 1 and a shared map: the same five accumulators across space
    torch        f = frames.to(int32); f.amax(0), f.argmax(0), f.amin(0), f.argmin(0), f.sum(0, int64), (f.to(int64) ** 2).sum(0)
    thin         the forms that are cut into slabs: 5 000 x 64x80 and 70 001 x 3x5
    recording    IRMovie.pixel_stats over a 1 000-frame recording against IRMovie.to_tensor alone
    python tests/perf/pixel_stats_time.py [--frames N] [--reps R] [--no-torch] [--no-movie] [--only-kernels] [--json out.json]"""
import argparse
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from librir_amd import device as D  # noqa: E402
from librir_amd.low_level.misc import _lib  # noqa: E402
from librir_amd.synthetic import s1_noisy_background  # noqa: E402

PEAK_BYTES_PER_S = 8.0e12
H, W = 512, 640
FORMS = [("both groups", True, True), ("sums only", True, False), ("extremes only", False, True)]


def bytes_moved(n, h, w, sums, extremes):
    """the frames once, 2 x the partials (written, then read by the fold) where there is more than one slab, the outputs once"""
    npx = h * w
    work = _lib.rir_pixel_stats_workspace_bytes(w, h, n)
    slabs = work // (20 * npx) if work > 8 else 1
    per_px = (12 if sums else 0) + (8 if extremes else 0)
    out = (16 if sums else 0) + (16 if extremes else 0)
    return n * npx * 2 + (2 * slabs * npx * per_px if slabs > 1 else 0) + npx * out, slabs


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


def torch_route(frames):
    f = frames.to(torch.int32)
    return f.amax(0), f.argmax(0), f.amin(0), f.argmin(0), f.sum(0, dtype=torch.int64), (f.to(torch.int64) ** 2).sum(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-movie", action="store_true")
    ap.add_argument("--only-kernels", action="store_true", help="the three forms alone (for a profiler)")
    ap.add_argument("--json")
    a = ap.parse_args()
    assert torch.cuda.is_available() and D.device_available(), "needs a GPU"
    n = a.frames
    host = s1_noisy_background(n, H, W, seed=1)
    frames = torch.from_numpy(host.view(np.int16)).cuda().view(torch.uint16)
    rows = []
    print("%-34s %12s %9s %8s %8s %6s" % ("workload", "frames/s", "ms", "GB", "of peak", "slabs"))

    def report(name, nf, t, nbytes=None, slabs=None, **more):
        row = dict(workload=name, frames=nf, frames_per_s=nf / t, ms=t * 1e3, **more)
        if nbytes is not None:
            row.update(bytes=nbytes, fraction_of_peak=nbytes / t / PEAK_BYTES_PER_S, slabs=slabs)
        rows.append(row)
        print("%-34s %12.4g %9.3f %8s %8s %6s" % (name, nf / t, t * 1e3, "%.3f" % (nbytes / 1e9) if nbytes else "-",
                                                 "%.3f" % row["fraction_of_peak"] if nbytes else "-", slabs if slabs else "-"), flush=True)

    for name, sums, extremes in FORMS:
        t = time_call(lambda: D.pixel_stats(frames, sums, extremes), a.reps)
        nbytes, slabs = bytes_moved(n, H, W, sums, extremes)
        report("%d x %dx%d, %s" % (n, W, H, name), n, t, nbytes, slabs)
    if a.only_kernels:
        return
    labels = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    t = time_call(lambda: D.region_stats(frames, labels, 1), a.reps)
    report("region_stats, K = 1, shared map", n, t)
    if not a.no_torch:
        t = time_call(lambda: torch_route(frames), max(1, a.reps // 3))
        report("torch, int32 / int64 reductions", n, t)
    for nt, h, w in [(5000, 64, 80), (70001, 3, 5)]:
        thin = torch.randint(0, 65536, (nt, h, w), dtype=torch.int32, device="cuda").to(torch.int16).view(torch.uint16)
        for name, sums, extremes in FORMS:
            t = time_call(lambda: D.pixel_stats(thin, sums, extremes), a.reps)
            nbytes, slabs = bytes_moved(nt, h, w, sums, extremes)
            report("%d x %dx%d, %s" % (nt, w, h, name), nt, t, nbytes, slabs)
    if not a.no_movie:
        from librir_amd.video_io import IRMovie, IRSaver

        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "m.h264")
            with IRSaver(path, W, H, H) as s:
                s.add_images(frames, np.arange(n, dtype=np.int64) * 1000)
            with IRMovie.from_filename(path) as mov:
                out = torch.empty((n, H, W), dtype=torch.uint16, device="cuda")
                t_read = time_call(lambda: mov.to_tensor(out=out), max(1, a.reps // 2))
                t = time_call(lambda: mov.pixel_stats(), max(1, a.reps // 2))
        report("recording, to_tensor only", n, t_read)
        report("recording, pixel_stats", n, t, over_to_tensor=t / t_read)
        print("IRMovie.pixel_stats / to_tensor alone: %.3f" % (t / t_read))
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"frames": n, "shape": [H, W], "peak_bytes_per_s": PEAK_BYTES_PER_S, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
