"""Temporal median rate over 1 000 frames of 640x512 uint16 (GPU box): for windows 1, 3, 5, 9, 15, 31 and 63, frames/s of one
device.temporal_median call, the algorithmic bytes (each input frame read once per run of outputs it feeds - the run kernel's halo
included - and each output written once), the share of the 8 TB/s HBM peak, and for comparison the torch route
frames.unfold(0, W, 1).median(-1), timed on an int32 copy of the frames (interior outputs only; torch takes the lower median).
    python tests/perf/temporal_median_time.py [--frames N] [--reps R] [--windows 5,15] [--no-torch] [--json out.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from librir_amd import device as D  # noqa: E402

PEAK_BYTES_PER_S = 8.0e12
H, W = 512, 640


def algorithmic_bytes(n, window, npx):
    """bytes the launcher's plan moves (temporal_kernels.hip, launch_window): interior runs of `run` outputs read run + W - 1 frames,
    every other output reads its (truncated) window, every output is written once"""
    r = window // 2
    frame = 2 * npx
    if window == 1:
        return 2 * n * frame
    v = 4 if window <= 9 else 2 if window <= 31 else 1
    groups = (npx + 2 * v - 1) // (2 * v)
    interior = max(0, n - 2 * r)
    run = 64
    while run > 8 and groups * ((interior + run - 1) // run) < (1 << 18):
        run //= 2
    reads = 0
    for k in range(0, interior, run):
        reads += min(run, interior - k) + window - 1
    for t in list(range(0, min(r, n))) + list(range(max(r, n - r), n)):
        reads += min(n - 1, t + r) - max(0, t - r) + 1
    return (reads + n) * frame


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--windows", default="1,3,5,9,15,31,63")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--json")
    a = ap.parse_args()
    assert torch.cuda.is_available() and D.device_available(), "needs a GPU"
    n = a.frames
    src = torch.randint(0, 65536, (n, H, W), dtype=torch.int32, device="cuda")
    frames = src.to(torch.int16).view(torch.uint16)
    out = torch.empty_like(frames)
    rows = []
    print("%6s %12s %10s %10s %8s %14s" % ("window", "frames/s", "ms", "GB", "of peak", "torch frames/s"))
    for window in [int(x) for x in a.windows.split(",")]:
        t = time_call(lambda: D.temporal_median(frames, window, out=out), a.reps)
        nbytes = algorithmic_bytes(n, window, H * W)
        row = {"window": window, "frames_per_s": n / t, "ms": t * 1e3, "bytes": nbytes, "fraction_of_peak": nbytes / t / PEAK_BYTES_PER_S}
        if not a.no_torch and n >= window:
            tt = time_call(lambda: src.unfold(0, window, 1).median(-1), max(1, a.reps // 3))
            row["torch_unfold_frames_per_s"] = (n - window + 1) / tt
        rows.append(row)
        print("%6d %12.4g %10.3f %10.3f %8.3f %14s" % (window, row["frames_per_s"], row["ms"], nbytes / 1e9, row["fraction_of_peak"],
                                                     "%.4g" % row["torch_unfold_frames_per_s"] if "torch_unfold_frames_per_s" in row else "-"),
              flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"frames": n, "shape": [H, W], "peak_bytes_per_s": PEAK_BYTES_PER_S, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
