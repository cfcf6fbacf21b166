"""Flat morphology rate over 256 frames of 640x512 (GPU box): for every op at 3x3, 5x5, 7x7, 9x9 and 15x15 on uint16, and at 3x3 on uint8,
frames/s of one device.morphology call, the share of the 8 TB/s HBM peak on the 4WH bytes a uint16 frame costs (read once, written once;
2WH for uint8), the ratio to device.median_filter - the 3x3 rank filter that moves the same bytes - timed in the same process on the same
stack, and for comparison the torch route through float tensors (max_pool2d, and -max_pool2d(-x) for a min; its border is the clipped
window too).
    python tests/perf/morphology_time.py [--frames N] [--reps R] [--sizes 3,9] [--no-torch] [--json out.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from librir_amd import device as D  # noqa: E402

PEAK_BYTES_PER_S = 8.0e12
H, W = 512, 640
OPS = ("erode", "dilate", "open", "close", "tophat", "blackhat", "gradient")
_stacks = {}


def stack_of(n, dtype=torch.uint16):
    """one random stack (and an output of its shape) per length and type, shared by every measurement of the process"""
    if (n, dtype) not in _stacks:
        g = torch.Generator(device="cuda").manual_seed(3)
        src = torch.randint(0, 65536 if dtype == torch.uint16 else 256, (n, H, W), dtype=torch.int32, device="cuda", generator=g)
        frames = src.to(torch.int16).view(torch.uint16) if dtype == torch.uint16 else src.to(torch.uint8)
        _stacks[n, dtype] = (frames, torch.empty_like(frames))
    return _stacks[n, dtype]


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


def torch_route(x, op, size):
    """the same op on a float32 stack [n][1][h][w] with max_pool2d (padding with -inf: the clipped window)"""
    pool = lambda t: torch.nn.functional.max_pool2d(t, size, stride=1, padding=size // 2)  # noqa: E731
    dilate, erode = pool, lambda t: -pool(-t)  # noqa: E731
    return {"erode": lambda: erode(x), "dilate": lambda: dilate(x), "open": lambda: dilate(erode(x)), "close": lambda: erode(dilate(x)),
            "tophat": lambda: x - dilate(erode(x)), "blackhat": lambda: erode(dilate(x)) - x, "gradient": lambda: dilate(x) - erode(x)}[op]()


def measure(op, size, n, reps, dtype=torch.uint16):
    """frames/s of device.morphology(op, size) - or of device.median_filter for op "median_filter", of the torch route for "torch:<op>" -
    over n frames of 640x512, best of reps"""
    frames, out = stack_of(n, dtype)
    if op == "median_filter":
        return n / time_call(lambda: D.median_filter(frames), reps)
    if op.startswith("torch:"):
        x = frames.float().unsqueeze(1)
        return n / time_call(lambda: torch_route(x, op[6:], size), reps)
    return n / time_call(lambda: D.morphology(frames, op, size, out=out), reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="3,5,7,9,15")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--json")
    a = ap.parse_args()
    assert torch.cuda.is_available() and D.device_available(), "needs a GPU"
    n = a.frames
    median = measure("median_filter", 3, n, a.reps)
    print("median_filter 3x3: %.4g frames/s, %.3f of peak" % (median, median * 4 * H * W / PEAK_BYTES_PER_S))
    rows = []
    print("%6s %5s %9s %12s %8s %8s %10s %14s" % ("type", "size", "op", "frames/s", "ms", "of peak", "x median", "torch frames/s"))
    for dtype, sizes in ((torch.uint16, [int(s) for s in a.sizes.split(",")]), (torch.uint8, [3])):
        px = 2 if dtype == torch.uint16 else 1
        for size in sizes:
            for op in OPS:
                rate = measure(op, size, n, a.reps, dtype)
                row = {"dtype": str(dtype), "size": size, "op": op, "frames_per_s": rate, "ms": n / rate * 1e3,
                       "fraction_of_peak": rate * 2 * px * H * W / PEAK_BYTES_PER_S, "ratio_to_median_filter": rate / median}
                if not a.no_torch and dtype == torch.uint16:
                    row["torch_frames_per_s"] = measure("torch:" + op, size, n, max(1, a.reps // 4))
                rows.append(row)
                print("%6s %5d %9s %12.4g %8.3f %8.3f %10.2f %14s" % (str(dtype)[6:], size, op, rate, row["ms"], row["fraction_of_peak"],
                                                                   row["ratio_to_median_filter"],
                                                                   "%.4g" % row["torch_frames_per_s"] if "torch_frames_per_s" in row else "-"), flush=True)
    median_after = measure("median_filter", 3, n, a.reps)
    print("median_filter 3x3 again: %.4g frames/s" % median_after)
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"frames": n, "shape": [H, W], "peak_bytes_per_s": PEAK_BYTES_PER_S, "median_filter_frames_per_s": [median, median_after],
                       "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
