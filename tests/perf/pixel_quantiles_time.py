"""Per-pixel quantile rate over 1 000 frames of 640x512 uint16 S1 frames (GPU box), after warm-up, the median of repeated timed calls:
for Q = 1 (0.5), 3 (0.05, 0.5, 0.95) and 8 percents
    one call     device.pixel_quantiles over the resident stack: ms and frames/s
    streamed     a PixelQuantileSelector fed the same stack in pieces of 64 MiB, every pass
then, on the same stack in the same process,
    yardstick    device.pixel_stats(sums=False): one streaming read of the stack; call time / yardstick time is compared with R, the
                 number of times the design reads the frames (1 + 3 * ceil(Q / 4)) - near R: memory-bound, above 2 R: bound by something else
    torch        the fastest torch route to the same median, torch.sort(frames.to(int32), dim=0) or kthvalue, on as many frames as its
                 memory allows, scaled per frame; the Q = 1 call must be faster (asserted; the ratio is printed)
    python tests/perf/pixel_quantiles_time.py [--frames N] [--reps R] [--no-torch] [--only-kernels] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from librir_amd import device as D  # noqa: E402
from librir_amd.synthetic import s1_noisy_background  # noqa: E402

H, W = 512, 640
PIECE_BYTES = 64 << 20
SETS = [("Q = 1", (0.5,)), ("Q = 3", (0.05, 0.5, 0.95)), ("Q = 8", (0.0, 0.001, 0.25, 0.5, 0.75, 0.9, 0.99, 1.0))]


def reads(q):
    """R: pass 0 reads the frames once for all percents, passes 1 to 3 once per group of 4 percents"""
    return 1 + 3 * ((q + 3) // 4)


def time_call(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop) * 1e-3)
    return statistics.median(times)


def streamed(frames, pc, per_piece):
    sel = D.PixelQuantileSelector(pc, shape=tuple(frames.shape[1:]))
    for _ in range(sel.passes):
        for k in range(0, frames.shape[0], per_piece):
            sel.push(frames[k:k + per_piece])
        sel.next_pass()
    return sel.result()


def torch_median_sort(frames):
    return torch.sort(frames.to(torch.int32), dim=0).values[(frames.shape[0] + 1) // 2 - 1]


def torch_median_kth(frames):
    return torch.kthvalue(frames.to(torch.int32), (frames.shape[0] + 1) // 2, dim=0).values


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--torch-frames", type=int, default=250, help="frames the torch routes run on (scaled per frame)")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--only-kernels", action="store_true", help="the one-call forms alone (for a profiler)")
    ap.add_argument("--json")
    a = ap.parse_args()
    assert torch.cuda.is_available() and D.device_available(), "needs a GPU"
    n = a.frames
    host = s1_noisy_background(n, H, W, seed=1)
    frames = torch.from_numpy(host.view(np.int16)).cuda().view(torch.uint16)
    per_piece = max(1, PIECE_BYTES // (2 * H * W))
    rows = {}
    print("%-40s %12s %9s" % ("workload", "frames/s", "ms"))

    def report(name, nf, t, **more):
        rows[name] = dict(frames=nf, frames_per_s=nf / t, ms=t * 1e3, **more)
        print("%-40s %12.4g %9.3f %s" % (name, nf / t, t * 1e3, " ".join("%s=%.3g" % kv for kv in more.items())), flush=True)

    one = {}
    for name, pc in SETS:
        one[name] = time_call(lambda: D.pixel_quantiles(frames, pc), a.reps)
        report("%d x %dx%d, %s, one call" % (n, W, H, name), n, one[name], frame_reads=reads(len(pc)))
    if a.only_kernels:
        return
    for name, pc in SETS:
        t = time_call(lambda: streamed(frames, pc, per_piece), a.reps)
        report("%s, streamed in 64 MiB pieces" % name, n, t, over_one_call=t / one[name])
    t_stats = time_call(lambda: D.pixel_stats(frames, sums=False), a.reps)
    report("pixel_stats(sums=False), one read", n, t_stats)
    for name, pc in SETS:
        r = reads(len(pc))
        ratio = one[name] / t_stats
        rows["%s over one read" % name] = dict(ratio=ratio, frame_reads=r)
        print("%s: call / one read = %.2f, R = %d (%s)" % (name, ratio, r, "memory-streaming" if ratio <= 2 * r else "NOT bound by HBM: above 2 R"))
    if not a.no_torch:
        m = min(n, a.torch_frames)
        part = frames[:m]
        per_frame = {}
        for name, fn in (("torch.sort(int32, dim=0)", torch_median_sort), ("torch.kthvalue(int32, dim=0)", torch_median_kth)):
            t = time_call(lambda: fn(part), max(1, a.reps // 3), warm=1)
            per_frame[name] = t / m
            report("%s, %d frames" % (name, m), m, t)
        ours = D.pixel_quantiles(part, 0.5)[0]
        assert torch.equal(torch_median_sort(part), ours) and torch.equal(torch_median_kth(part), ours), "the S1 scene holds no 65535: the same median"
        best = min(per_frame, key=per_frame.get)
        speedup = per_frame[best] * n / one["Q = 1"]
        rows["Q = 1 over torch"] = dict(speedup=speedup, route=best)
        print("Q = 1 call against the fastest torch route (%s, scaled to %d frames): %.1f x faster" % (best, n, speedup))
        assert speedup > 1.0, "the Q = 1 call must be faster than the fastest torch route"
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"frames": n, "shape": [H, W], "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
