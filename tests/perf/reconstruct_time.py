"""h-dome rate over 256 frames of 640x512 uint16 (GPU box), for two scenes - (a) librir_amd.synthetic's hot-spot frames (discs of 8 000 on a
background of uniform noise), (b) smooth blobs plus noise of sigma 20 (reconstruct_cases.blobs_and_noise), where a value travels a long way -
at h = 50: frames/s and ms of one device.h_dome call, the rounds it took, and the ratio to the same result computed with what the library had
before: torch.minimum(device.dilate(F, 3), G) from F = G - h, repeated until torch.equal says that nothing changed - looked at every
`--check-every` iterations only, so that its host synchronisation is not what is compared - and a last subtraction.  Both are timed on the
host clock around a device synchronisation (h_dome waits for the stream between its rounds anyway), on the same stack in the same process, in
alternating rounds; the figures are medians over the rounds, with the spread of the ratio.
    python tests/perf/reconstruct_time.py [--frames N] [--rounds R] [--reps K] [--h H] [--check-every C] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from librir_amd import device as D  # noqa: E402
from librir_amd.synthetic import hot_spots  # noqa: E402
from reconstruct_cases import blobs_and_noise  # noqa: E402

H, W = 512, 640
SCENES = ("hot_spots", "blobs")
_scenes = {}


def scenes_of(n):
    """{scene: uint16 CUDA stack [n][512][640]}, shared by every measurement of the process; 32 different frames of each, repeated.  Every
    value is below 32 768, so the composed route may compare the frames as int16 (torch has no minimum for uint16)"""
    if n not in _scenes:
        hot = np.tile(hot_spots(32), ((n + 31) // 32, 1, 1))[:n]
        blobs = np.tile(np.stack([blobs_and_noise(seed=s) for s in range(8)]), ((n + 7) // 8, 1, 1))[:n]
        assert hot.max() < 32768 and blobs.max() < 32768
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda().view(torch.uint16)  # noqa: E731
        _scenes[n] = {"hot_spots": up(hot), "blobs": up(blobs), "out": torch.empty((n, H, W), dtype=torch.uint16, device="cuda"),
                      "f": torch.empty((n, H, W), dtype=torch.uint16, device="cuda"), "d": torch.empty((n, H, W), dtype=torch.uint16, device="cuda"),
                      "old": torch.empty((n, H, W), dtype=torch.uint16, device="cuda")}
    return _scenes[n]


def composed_h_dome(g, h, s, check_every):
    """the h-dome of g by the route that existed before: -> (result in s["d"], iterations)"""
    g16, f, d, old = g.view(torch.int16), s["f"], s["d"], s["old"]
    f16, d16 = f.view(torch.int16), d.view(torch.int16)
    torch.clamp(g16 - h, min=0, out=f16)  # (values below 32 768: no wrap)
    iterations = 0
    while True:
        for _ in range(check_every - 1):
            D.dilate(f, 3, out=d)
            torch.minimum(d16, g16, out=f16)
        old.copy_(f)
        D.dilate(f, 3, out=d)
        torch.minimum(d16, g16, out=f16)
        iterations += check_every
        if torch.equal(old.view(torch.int16), f16):
            break
    torch.sub(g16, f16, out=d16)
    return d, iterations


def wall(fn, reps):
    """seconds per call over reps calls on the host clock, the device idle before and after, after one warm-up call"""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def check(n, h, check_every):
    """both routes give the same bits; -> {scene: (rounds of h_dome, iterations of the composed route)}"""
    s = scenes_of(n)
    out = {}
    for scene in SCENES:
        _, rounds = D._reconstruct("h_dome", s[scene], None, "dilation", 8, None, s["out"], D.RECONSTRUCT_SHIFT, h, 1, return_rounds=True)
        d, iterations = composed_h_dome(s[scene], h, s, check_every)
        assert torch.equal(d.view(torch.int16), s["out"].view(torch.int16)), scene
        out[scene] = (rounds, iterations)
    return out


def rounds_of(n, rounds, reps, h=50, check_every=8, scenes=SCENES):
    """[{(scene, "h_dome"): frames/s, (scene, "composed"): frames/s} per round], the two routes alternating"""
    s = scenes_of(n)
    out = []
    for _ in range(rounds):
        r = {}
        for scene in scenes:
            r[scene, "composed"] = n / wall(lambda: composed_h_dome(s[scene], h, s, check_every), max(1, reps // 4))
            r[scene, "h_dome"] = n / wall(lambda: D.h_dome(s[scene], h, out=s["out"]), reps)
        out.append(r)
    return out


def summary(rs, scene):
    """(median frames/s of h_dome, of the composed route, median ratio, lowest and highest ratio of a round)"""
    ratios = [r[scene, "h_dome"] / r[scene, "composed"] for r in rs]
    return (statistics.median(r[scene, "h_dome"] for r in rs), statistics.median(r[scene, "composed"] for r in rs), statistics.median(ratios), min(ratios),
            max(ratios))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--h", type=int, default=50)
    ap.add_argument("--check-every", type=int, default=8)
    ap.add_argument("--json")
    a = ap.parse_args()
    assert torch.cuda.is_available() and D.device_available(), "needs a GPU"
    n = a.frames
    took = check(n, a.h, a.check_every)
    rs = rounds_of(n, a.rounds, a.reps, a.h, a.check_every)
    rows = []
    print("%10s %12s %8s %7s %14s %11s %9s %18s" % ("scene", "frames/s", "ms", "rounds", "composed f/s", "iterations", "ratio", "(lowest..highest)"))
    for scene in SCENES:
        rate, other, ratio, lo, hi = summary(rs, scene)
        row = {"scene": scene, "h": a.h, "frames_per_s": rate, "ms": n / rate * 1e3, "rounds": took[scene][0], "composed_frames_per_s": other,
               "composed_ms": n / other * 1e3, "composed_iterations": took[scene][1], "ratio": ratio, "ratio_lowest": lo, "ratio_highest": hi}
        rows.append(row)
        print("%10s %12.4g %8.3f %7d %14.4g %11d %9.2f %18s" % (scene, rate, row["ms"], row["rounds"], other, row["composed_iterations"], ratio,
                                                                 "%.2f..%.2f" % (lo, hi)), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"frames": n, "shape": [H, W], "rounds": a.rounds, "reps": a.reps, "check_every": a.check_every, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
