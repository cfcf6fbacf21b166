"""Component tracking rate over 1 000 label maps of 640x512 (GPU box): frames/s and ms of one device.track_components call, with the track
map (relabel, written to a preallocated stack) and without, the model bytes - the link pass reads every label frame 1 + 1/R times (runs of
R = 64 frame pairs), relabel reads and writes it once: 4 * W * H * (1 + 1/R) and 8 * W * H a frame; the node passes are left out - and their
share of the 8 TB/s HBM peak, for
    hot spots    synthetic.hot_spots above 4 000: a few large components a frame
    S1 99.9 %    every S1 frame above its own 99.9th percentile: a few hundred specks a frame (the per-frame case of region_stats_time.py)
    noise        a random mask at density 0.5: tens of thousands of components a frame, the worst case for unions
Yardsticks timed in the same run, none of them the code under test: an int32 copy of the label stack (dst.copy_(src): the 8 * W * H of
relabel), label_images on the same masks and, where scipy imports, scipy.ndimage.label with the 3-D structure on the first 100 frames on the
host, scaled to the stack.
    python tests/perf/track_time.py [--frames N] [--reps R] [--scenes hot,s1,noise] [--no-scipy] [--json out.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from librir_amd import device as D  # noqa: E402
from librir_amd.synthetic import hot_spots, s1_noisy_background  # noqa: E402

PEAK_BYTES_PER_S = 8.0e12
H, W = 512, 640
RUN = 64  # track_kernels.hip TK_RUN


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


def as_int32(frames):
    return frames.view(torch.int16).to(torch.int32) & 0xFFFF


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--scenes", default="hot,s1,noise")
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--json")
    a = ap.parse_args()
    assert torch.cuda.is_available() and D.device_available(), "needs a GPU"
    n, npx = a.frames, H * W
    try:
        import scipy.ndimage as ndi
    except ImportError:
        ndi = None
    if a.no_scipy:
        ndi = None

    scenes = a.scenes.split(",")

    def masks():
        if "hot" in scenes:
            f = torch.from_numpy(hot_spots(n, H, W).view(np.int16)).cuda().view(torch.uint16)
            yield "hot spots", as_int32(f) > 4000
        if "s1" in scenes:
            f = torch.from_numpy(s1_noisy_background(n, H, W, seed=1).view(np.int16)).cuda().view(torch.uint16)
            v32 = as_int32(f)
            cut = torch.stack([x.reshape(-1).float().kthvalue(int(0.999 * npx)).values for x in v32])
            yield "S1 99.9 %", v32 > cut.view(n, 1, 1).to(torch.int32)
        if "noise" in scenes:
            yield "noise", torch.rand((n, H, W), device="cuda", generator=torch.Generator("cuda").manual_seed(5)) < 0.5

    rows = []
    print("%-12s %7s %9s | %-22s %12s %9s %8s %8s" % ("scene", "K", "tracks", "what", "frames/s", "ms", "GB", "of peak"))
    for name, mask in masks():
        labels, _, _, counts = D.label_images(mask, table_entries=1)
        k = int(counts.max())
        dst = torch.empty_like(labels)
        ntracks = int(D.track_components(labels, counts, k, relabel=False).ntracks)
        link_bytes, relabel_bytes = n * npx * 4 * (1 + 1.0 / RUN), n * npx * 8
        timed = [("label_images", time_call(lambda: D.label_images(mask, table_entries=1), max(1, a.reps // 3)), None),
                 ("int32 copy", time_call(lambda: dst.copy_(labels), a.reps), relabel_bytes),
                 ("track, relabel off", time_call(lambda: D.track_components(labels, counts, k, relabel=False), a.reps), link_bytes),
                 ("track, relabel on", time_call(lambda: D.track_components(labels, counts, k, out=dst), a.reps), link_bytes + relabel_bytes)]
        if ndi is not None:
            m = min(n, 100)
            host = mask[:m].cpu().numpy()
            structure = np.zeros((3, 3, 3), int)
            structure[1] = [[0, 1, 0], [1, 1, 1], [0, 1, 0]]
            structure[:, 1, 1] = 1
            t0 = time.perf_counter()
            ndi.label(host, structure)
            timed.append(("scipy 3-D label, host", (time.perf_counter() - t0) * n / m, None))
        for what, t, nbytes in timed:
            row = {"scene": name, "K": k, "tracks": ntracks - 1, "what": what, "frames_per_s": n / t, "ms": t * 1e3}
            if nbytes is not None:
                row.update(bytes=nbytes, fraction_of_peak=nbytes / t / PEAK_BYTES_PER_S)
            rows.append(row)
            print("%-12s %7d %9d | %-22s %12.4g %9.3f %8s %8s" % (name, k, ntracks - 1, what, n / t, t * 1e3,
                                                                 "%.3f" % (nbytes / 1e9) if nbytes else "-",
                                                                 "%.3f" % row["fraction_of_peak"] if nbytes else "-"), flush=True)
        del labels, dst, mask
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"frames": n, "shape": [H, W], "peak_bytes_per_s": PEAK_BYTES_PER_S, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
