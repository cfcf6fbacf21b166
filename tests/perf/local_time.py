"""Local window statistics rate over 256 frames of 640x512 uint16 (GPU box), timed as morphology_time.py times its stack and on that stack:
frames/s of one device.local_threshold call (the mask form: 2 bytes read, 1 written a pixel) and of device.box_mean (2 + 2), box_sum (2 + 4)
and local_stats with all three outputs (2 + 14) at 3x3, 9x9 and 15x15, the share of the 8 TB/s HBM peak on those bytes, and the ratio to
device.median_filter - the reference's 3x3 filter - timed in the same process by morphology_time.measure.  For comparison the torch route
that the mask replaces: avg_pool2d of the frames and of their squares in float32 on a replicate-padded stack, then the compare - an
approximation of the same mask, not its equal.
    python tests/perf/local_time.py [--frames N] [--reps R] [--rounds K] [--sizes 3,9,15] [--no-torch] [--json out.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from librir_amd import device as D  # noqa: E402
from morphology_time import H, PEAK_BYTES_PER_S, W, measure, stack_of, time_call  # noqa: E402

FORMS = {"local_threshold": 3, "box_mean": 4, "box_sum": 6, "local_stats": 16}  # bytes a pixel: read once, every output written once
_outs = {}


def _out(n, dtype):
    if (n, dtype) not in _outs:
        _outs[n, dtype] = torch.empty((n, H, W), dtype=dtype, device="cuda")
    return _outs[n, dtype]


def measure_local(form, size, n, reps):
    """frames/s of the form at size x size over n frames of 640x512 uint16, best of reps; local_threshold at k = 4, delta = 20"""
    frames, _ = stack_of(n)
    if form == "local_threshold":
        out = _out(n, torch.bool)
        return n / time_call(lambda: D.local_threshold(frames, size, 4, 20, out=out), reps)
    if form == "box_mean":
        out = _out(n, torch.uint16)
        return n / time_call(lambda: D.box_mean(frames, size, out=out), reps)
    if form == "box_sum":
        out = _out(n, torch.int32)
        return n / time_call(lambda: D.box_sum(frames, size, out=out), reps)
    outs = (_out(n, torch.int32), _out(n, torch.int64), _out(n, torch.uint16))
    return n / time_call(lambda: D.local_stats(frames, size, None, True, True, True, out=outs), reps)


def torch_route(x, size, k=4.0, delta=20.0):
    """x: float32 [n][1][h][w] -> the mask, through two average pools of a replicate-padded stack"""
    pad = torch.nn.functional.pad(x, (size // 2,) * 4, mode="replicate")
    mean = torch.nn.functional.avg_pool2d(pad, size, stride=1)
    var = torch.nn.functional.avg_pool2d(pad * pad, size, stride=1) - mean * mean
    off = x - mean
    return (off > delta) & (off * off > k * k * var)


def measure_torch(size, n, reps):
    frames, _ = stack_of(n)
    x = frames.float().unsqueeze(1)
    return n / time_call(lambda: torch_route(x, size), reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", default="3,9,15")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--json")
    a = ap.parse_args()
    assert torch.cuda.is_available() and D.device_available(), "needs a GPU"
    n = a.frames
    rows = []
    print("%6s %16s %5s %12s %8s %8s %10s" % ("round", "form", "size", "frames/s", "ms", "of peak", "x median"))
    for k in range(a.rounds):  # (the yardstick again in every round: the ratio is taken within a round)
        median = measure("median_filter", 3, n, a.reps)
        print("%6d median_filter 3x3: %.4g frames/s, %.3f of peak" % (k, median, median * 4 * H * W / PEAK_BYTES_PER_S))
        for form, px_bytes in FORMS.items():
            for size in [int(s) for s in a.sizes.split(",")]:
                rate = measure_local(form, size, n, a.reps)
                row = {"round": k, "form": form, "size": size, "frames_per_s": rate, "ms": n / rate * 1e3,
                       "fraction_of_peak": rate * px_bytes * H * W / PEAK_BYTES_PER_S, "ratio_to_median_filter": rate / median}
                rows.append(row)
                print("%6d %16s %5d %12.4g %8.3f %8.3f %10.2f" % (k, form, size, rate, row["ms"], row["fraction_of_peak"], row["ratio_to_median_filter"]),
                      flush=True)
    if not a.no_torch:
        for size in [int(s) for s in a.sizes.split(",")]:
            rate = measure_torch(size, n, max(1, a.reps // 4))
            rows.append({"form": "torch", "size": size, "frames_per_s": rate})
            print("%6s %16s %5d %12.4g %8.3f" % ("-", "torch avg_pool2d", size, rate, n / rate * 1e3), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"frames": n, "shape": [H, W], "peak_bytes_per_s": PEAK_BYTES_PER_S, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
