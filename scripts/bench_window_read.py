"""Windowed reads against the whole read followed by a crop, on one GPU: IRMovie.to_tensor(window=...) of a 1 000-image 640x512 S1
recording, for the windows of DESIGN.md section 4.  The forms of every case alternate, ROUNDS times each after a warm-up of each, a round
being REPS calls between two synchronisations (a single call of a millisecond is too short a timed window); the median and the range
over the rounds, in ms per call, are printed, one JSON line a case.  Read-back filters off, and the 64x64 window again with
bad-pixel repair on.

    python scripts/bench_window_read.py [--frames 1000] [--rounds 9] [--reps 20]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from librir_amd.synthetic import s1_noisy_background  # noqa: E402
from librir_amd.video_io import IRMovie, IRSaver  # noqa: E402

H, W = 512, 640
WINDOWS = [("64x64", (224, 288, 64, 64)), ("64 rows, full width", (224, 0, 64, 640)), ("whole frame", (0, 0, 512, 640)),
           ("61x59 unaligned", (225, 291, 61, 59))]


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def compare(mov, name, win, rounds, reps, filters):
    y0, x0, h, w = win
    forms = {"window": lambda: mov.to_tensor(window=win), "read+crop": lambda: mov.to_tensor()[:, y0:y0 + h, x0:x0 + w].contiguous(),
             "read": lambda: mov.to_tensor()}
    a, b = forms["window"](), forms["read+crop"]()
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)), name
    forms["read"]()
    ms = {k: [] for k in forms}
    for _ in range(rounds):  # alternating: a drift of the box falls on every form alike
        for k, fn in forms.items():
            ms[k].append(timed(fn, reps))
    out = {"case": name, "window": list(win), "filters": filters, "frames": mov.images, "rounds": rounds, "reps": reps}
    for k, v in ms.items():
        out[k + "_ms"] = {"median": round(float(np.median(v)), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    out["speedup_vs_read+crop"] = round(out["read+crop_ms"]["median"] / out["window_ms"]["median"], 2)
    out["speedup_vs_read"] = round(out["read_ms"]["median"] / out["window_ms"]["median"], 2)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    arr = s1_noisy_background(a.frames, H, W)
    frames = torch.from_numpy(arr.astype(np.int32)).to(torch.uint16).cuda()
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "s1.h264")
        with IRSaver(p, W, H, H) as s:
            s.add_images(frames, np.arange(a.frames, dtype=np.int64) * 20000000)
        del frames
        with IRMovie.from_filename(p) as mov:
            for name, win in WINDOWS:
                compare(mov, name, win, a.rounds, a.reps, "off")
            mov.bad_pixels_correction = True
            compare(mov, "64x64", WINDOWS[0][1], a.rounds, a.reps, "bad pixels")


if __name__ == "__main__":
    main()
