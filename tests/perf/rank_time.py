"""Spatial rank filter rate over 256 frames of 640x512 uint16 (GPU box), timed as morphology_time.py times its stack and on that stack: frames/s
of one device.rank_filter call at the median rank of 3x3, 5x5 (the register kernels), 7x7, 9x9 and 15x15 (the LDS tile kernel), and of a
low percentile, the share of the 8 TB/s HBM peak on the 4WH bytes a frame costs, and the ratio to device.median_filter - the reference's 3x3
filter, which moves the same bytes - timed in the same process by morphology_time.measure.
    python tests/perf/rank_time.py [--frames N] [--reps R] [--rounds K] [--sizes 3,5,9] [--json out.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from librir_amd import device as D  # noqa: E402
from morphology_time import H, PEAK_BYTES_PER_S, W, measure, stack_of, time_call  # noqa: E402


def measure_rank(size, rank, n, reps):
    """frames/s of device.rank_filter(rank, size) - the median rank for rank None - over n frames of 640x512 uint16, best of reps"""
    frames, out = stack_of(n)
    rank = size * size // 2 if rank is None else rank
    return n / time_call(lambda: D.rank_filter(frames, rank, size, out=out), reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", default="3,5,7,9,15")
    ap.add_argument("--json")
    a = ap.parse_args()
    assert torch.cuda.is_available() and D.device_available(), "needs a GPU"
    n = a.frames
    rows = []
    print("%6s %5s %5s %12s %8s %8s %10s" % ("round", "size", "rank", "frames/s", "ms", "of peak", "x median"))
    for k in range(a.rounds):  # (the yardstick again in every round: the ratio is taken within a round)
        median = measure("median_filter", 3, n, a.reps)
        print("%6d median_filter 3x3: %.4g frames/s, %.3f of peak" % (k, median, median * 4 * H * W / PEAK_BYTES_PER_S))
        for size in [int(s) for s in a.sizes.split(",")]:
            cells = size * size
            for rank in (cells // 2, cells // 4):
                reps = a.reps if size <= 9 else max(2, a.reps // 4)
                rate = measure_rank(size, rank, n, reps)
                row = {"round": k, "size": size, "rank": rank, "frames_per_s": rate, "ms": n / rate * 1e3, "fraction_of_peak": rate * 4 * H * W / PEAK_BYTES_PER_S,
                       "ratio_to_median_filter": rate / median}
                rows.append(row)
                print("%6d %5d %5d %12.4g %8.3f %8.3f %10.2f" % (k, size, rank, rate, row["ms"], row["fraction_of_peak"], row["ratio_to_median_filter"]),
                      flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"frames": n, "shape": [H, W], "peak_bytes_per_s": PEAK_BYTES_PER_S, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
