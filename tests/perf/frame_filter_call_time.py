"""Host cost of a call of the Python forms of the frame filters in librir_amd.device (GPU box): microseconds per call over back-to-back
calls on a stack so small - (8, 64, 64) - that the wrapper and the launch, not the kernel, set the pace: morphology("open", 3),
local_threshold(3, 1) and h_dome(40) on uint16, distance_transform on bool.  Each figure is the wall clock of --calls calls with one
synchronise at the end, best of --reps.  h_dome waits for the stream between its rounds (it is synchronous with the host), so its figure holds
its kernels too.
    python tests/perf/frame_filter_call_time.py [--calls N] [--reps R] [--json out.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from librir_amd import device as D  # noqa: E402

N, H, W = 8, 64, 64


def forms():
    gen = torch.Generator(device="cuda").manual_seed(5)
    frames = torch.randint(1000, 1400, (N, H, W), dtype=torch.int32, device="cuda", generator=gen).to(torch.uint16)
    masks = torch.rand((N, H, W), device="cuda", generator=gen) < 0.9
    return {"morphology open 3": lambda: D.morphology(frames, "open", 3), "local_threshold 3, 1": lambda: D.local_threshold(frames, 3, 1),
            "h_dome 40": lambda: D.h_dome(frames, 40), "distance_transform": lambda: D.distance_transform(masks)}


def time_calls(call, calls, reps):
    """microseconds per call: `calls` of them back to back, one synchronise at the end, best of `reps`"""
    call()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(calls):
            call()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best / calls * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json")
    a = ap.parse_args()
    assert torch.cuda.is_available() and D.device_available(), "needs a GPU"
    rows = {}
    for name, call in forms().items():
        rows[name] = time_calls(call, a.calls, a.reps)
        print("%24s %8.2f us per call" % (name, rows[name]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"shape": [N, H, W], "calls": a.calls, "reps": a.reps, "us_per_call": rows}, f, indent=1)


if __name__ == "__main__":
    main()
