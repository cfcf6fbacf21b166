"""Polygon label map rate on 640x512 maps (GPU box): maps/s and ms of one device.polygon_map call on packed device tensors, the algorithmic
bytes (4 W H written per map; the polygons are noise beside them) over time against the 8 TB/s HBM peak, and beside each scene the time of
torch.full((n, h, w), -1, dtype=torch.int32), a write-only pass of the same bytes, for
    (a) octagons      n per-frame maps of 16 octagons covering about 0.4 of the image, moved by a shift table
    (b) quads         n maps of 1 024 small quadrilaterals (one set, shift table)
    (c) 1024 vertices n maps of one 1 024-vertex polygon (shift table)
    (d) shared        one map of the scene of (a): a call of a few microseconds of work, so 50 calls are timed together and the figure is
                      what a call costs in a queue of them (launches and the workspace's allocation), not a rate of the kernels
Both sides are timed as a caller meets them: a polygon_map call takes its workspace from torch's caching allocator, and torch.full
allocates its result from it, on every call.
    python tests/perf/polygon_map_time.py [--maps N] [--reps R] [--scenes abcd] [--json out.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import polygon_cases as PC  # noqa: E402
from librir_amd import device as D  # noqa: E402

PEAK_BYTES_PER_S = 8.0e12
H, W = 512, 640


def scene(kind, seed=1):
    """-> the polygons of a scene, as polygon_map takes them"""
    rng = np.random.default_rng(seed)
    if kind == "octagons":
        return PC.octagons(H, W)
    if kind == "quads":
        g = 32  # a 32 x 32 grid of jittered quadrilaterals, each about 12 x 10 pixels
        cells = [((i % g + 0.5) * W / g, (i // g + 0.5) * H / g) for i in range(g * g)]
        return [np.array([(cx - 6, cy - 5), (cx + 6, cy - 5), (cx + 6, cy + 5), (cx - 6, cy + 5)]) + rng.uniform(-2, 2, (4, 2)) for cx, cy in cells]
    if kind == "1024 vertices":
        return [PC.ring(1024, W / 2, H / 2, 0.45 * W, 0.45 * H) + rng.normal(0, 1.5, (1024, 2))]
    raise ValueError(kind)


def time_call(fn, reps, batch=1):
    """the best of `reps` timings of `batch` calls in a row, per call"""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = 1e9
    for _ in range(reps):
        start.record()
        for _ in range(batch):
            fn()
        stop.record()
        stop.synchronize()
        best = min(best, start.elapsed_time(stop) * 1e-3 / batch)
    return best


def measure(kind, n, reps, shifted=True, seed=1, batch=1):
    """-> (seconds of one polygon_map call, seconds of torch.full of the same maps, covered fraction of the first map)"""
    a = D._polygon_map_args(scene(kind, seed), (H, W), shifts=np.random.default_rng(seed).uniform(-20, 20, (n, 2)) if shifted else None)
    xy, npts, _, shifts = D._polygon_inputs(a, torch.device("cuda"))
    out = torch.empty(a.out_shape, dtype=torch.int32, device="cuda")
    t = time_call(lambda: D.polygon_map((xy, npts), (H, W), shifts=shifts, out=out), reps, batch)
    covered = float((out.view(-1, H, W)[0] >= 0).float().mean())
    t_fill = time_call(lambda: torch.full(a.out_shape, -1, dtype=torch.int32, device="cuda"), reps, batch)
    return t, t_fill, covered


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--scenes", default="abcd")
    ap.add_argument("--json")
    a = ap.parse_args()
    assert torch.cuda.is_available() and D.device_available(), "needs a GPU"
    rows = []
    print("%-28s %6s %12s %9s %8s %8s %9s %8s %8s" % ("scene", "maps", "maps/s", "ms", "GB", "of peak", "fill ms", "fill/map", "covered"))
    for name, kind, n, shifted in (("(a) 16 octagons, shifted", "octagons", a.maps, True), ("(b) 1024 quads, shifted", "quads", a.maps, True),
                                   ("(c) 1024 vertices, shifted", "1024 vertices", a.maps, True), ("(d) 16 octagons, one map", "octagons", 1, False)):
        if name[1] not in a.scenes:
            continue
        t, t_fill, covered = measure(kind, n, a.reps, shifted, batch=50 if n == 1 else 1)
        nbytes = n * H * W * 4
        rows.append({"scene": name, "maps": n, "maps_per_s": n / t, "ms": t * 1e3, "bytes": nbytes, "fraction_of_peak": nbytes / t / PEAK_BYTES_PER_S,
                     "torch_full_ms": t_fill * 1e3, "fill_over_map": t_fill / t, "covered": covered})
        print("%-28s %6d %12.4g %9.3f %8.3f %8.3f %9.3f %8.3f %8.3f" % (name, n, n / t, t * 1e3, nbytes / 1e9, nbytes / t / PEAK_BYTES_PER_S, t_fill * 1e3,
                                                                        t_fill / t, covered), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
