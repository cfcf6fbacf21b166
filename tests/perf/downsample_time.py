"""Adaptive temporal downsampling rate on 1 000 frames of 640x512 uint16 (GPU box): the S1 scene with a handful of block events, factor 10,
factor_std 0.9, both methods.  Printed per method:
    push          one Downsampler.push of the whole stack, host clock around the call and a synchronise: frames/s, ms (best and median of the
                  repeats, and their spread), and the floor of traffic 2 * 2WH * n + 2WH * kept bytes over that time against the 8 TB/s peak
    copy          a device-to-device copy of 2WH * n bytes (what either pass reads) timed the same way in the same run
    torch         the same job in plain torch: int32 differences, abs, the two sums per frame, a read-back, then the maximum over each
                  segment - what a user has without this feature (its segments are taken from the push's result)
    decide        the host recurrence alone (rir_downsample_decide over the same sums), part of the push's time
The time of each kernel alone comes from a kernel trace of this script (rocprofv3 --kernel-trace --stats -- python tests/perf/downsample_time.py):
ds_pair_sums and ds_max_hold each read the stack once, so either is compared with the copy of the same bytes.
    python tests/perf/downsample_time.py [--frames N] [--reps R] [--json out.json]"""
import argparse
import ctypes as ct
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import downsample_cases as DC  # noqa: E402
from librir_amd import device as D  # noqa: E402
from librir_amd.low_level.misc import _lib  # noqa: E402

PEAK_BYTES_PER_S = 8.0e12
H, W = 512, 640
EVENTS = {100: 300, 101: 300, 400: 200, 401: 400, 402: 100, 700: 500, 850: 250}


def scene(n, seed=1):
    """the S1 recipe of downsample_cases.scene, made on the device: bg * 1000 + 10 + N(0, sqrt(0.5)), block events"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    bg = torch.rand((H, W), device="cuda", generator=g) * 1000 + 10
    out = torch.empty((n, H, W), dtype=torch.uint16, device="cuda")
    for a in range(0, n, 50):
        b = min(n, a + 50)
        out[a:b] = (bg + torch.randn((b - a, H, W), device="cuda", generator=g) * 0.5 ** 0.5).to(torch.int32).to(torch.uint16)
    for i, level in EVENTS.items():
        if i < n:
            block = out[i, 2:H // 2, 3:W // 2]
            block.copy_((block.to(torch.int32) + level).to(torch.uint16))
    return out


def timed(fn, reps, warm=2):
    """host seconds of fn() + synchronise, every repeat -> sorted list"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return sorted(times)


def torch_job(fr, segments):
    v = fr.to(torch.int32)
    d = (v[1:] - v[:-1]).abs()
    x = d.sum((1, 2))
    q = (d * d).sum((1, 2), dtype=torch.int64)
    sums = torch.stack([x, q], 1).cpu()  # (the recurrence needs them on the host)
    out = torch.empty((len(segments), H, W), dtype=torch.uint16, device=fr.device)
    for k, (a, b) in enumerate(segments):
        out[k] = v[a:b + 1].amax(0).to(torch.uint16)
    return sums, out


def measure(method, n=1000, reps=10, factor=10, factor_std=.9, fr=None, with_torch=True):
    """-> dict of the figures of one method"""
    fr = scene(n) if fr is None else fr
    stamps = DC.stamps(n)
    out = torch.empty_like(fr)
    last = {}

    def push():
        d = D.Downsampler(W, H, factor, factor_std, None, method)
        last["r"] = d.push(fr, stamps, out=out)
        d.close()

    t_push = timed(push, reps)
    got = last["r"]
    kept = len(got.positions)
    copy_to = torch.empty_like(fr)
    t_copy = timed(lambda: copy_to.copy_(fr), reps)
    # the recurrence alone, from the exact sums of this scene
    v = fr.to(torch.int32)
    dd = (v[1:] - v[:-1]).abs()
    sums = np.zeros((n, 2), np.int64)
    sums[1:, 0] = dd.sum((1, 2)).cpu().numpy()
    sums[1:, 1] = (dd * dd).sum((1, 2), dtype=torch.int64).cpu().numpy()
    del v, dd
    keep = np.zeros(n, np.int32)
    stats = np.zeros(n, np.float64)
    t_decide = []
    for _ in range(reps):
        state = np.zeros(_lib.rir_downsample_state_bytes() // 8 + 1, np.int64)
        t0 = time.perf_counter()
        r = _lib.rir_downsample_decide(factor, ct.c_double(factor_std), method, ct.c_longlong(H * W), sums.ctypes.data, n, state.ctypes.data,
                                       keep.ctypes.data, stats.ctypes.data)
        t_decide.append(time.perf_counter() - t0)
    assert r == kept and np.array_equal(np.flatnonzero(keep), got.positions) and np.array_equal(stats.view(np.uint64), got.stats.view(np.uint64))
    res = {"method": method, "frames": n, "kept": kept, "push_s": t_push[0], "push_median_s": t_push[len(t_push) // 2], "push_worst_s": t_push[-1],
           "frames_per_s": n / t_push[0], "floor_bytes": 2 * 2 * W * H * n + 2 * W * H * kept, "copy_s": t_copy[0], "copy_median_s": t_copy[len(t_copy) // 2],
           "decide_s": min(t_decide)}
    res["fraction_of_peak"] = res["floor_bytes"] / t_push[0] / PEAK_BYTES_PER_S
    if with_torch:
        edges = [-1] + got.positions.tolist()
        segments = [(a + 1, b) for a, b in zip(edges[:-1], edges[1:])]
        t_torch = timed(lambda: torch_job(fr, segments), max(3, reps // 3), warm=1)
        res["torch_s"] = t_torch[0]
        _, images = torch_job(fr, segments)
        assert torch.equal(images.view(torch.int16), got.frames.view(torch.int16))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--json")
    a = ap.parse_args()
    assert torch.cuda.is_available() and D.device_available(), "needs a GPU"
    fr = scene(a.frames)
    rows = []
    print("%-8s %6s %5s %11s %8s %8s %8s %8s %8s %9s %9s %9s" % ("method", "frames", "kept", "frames/s", "ms", "median", "worst", "GB", "of peak", "copy ms",
                                                              "torch ms", "decide ms"))
    for method in (1, 2):
        r = measure(method, a.frames, a.reps, fr=fr, with_torch=not a.no_torch)
        rows.append(r)
        print("%-8d %6d %5d %11.5g %8.3f %8.3f %8.3f %8.3f %8.3f %9.3f %9.3f %9.3f" % (
            method, r["frames"], r["kept"], r["frames_per_s"], r["push_s"] * 1e3, r["push_median_s"] * 1e3, r["push_worst_s"] * 1e3, r["floor_bytes"] / 1e9,
            r["fraction_of_peak"], r["copy_s"] * 1e3, r.get("torch_s", float("nan")) * 1e3, r["decide_s"] * 1e3), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
