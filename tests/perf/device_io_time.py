"""Device I/O against the host route, one 1 000-image 640x512 S1 recording read and written in one process (GPU box):
    read:  IRMovie.to_tensor() against torch.from_numpy(mov.data).cuda(), uint16 and float32, read-back filters off and on
    write: IRSaver.add_images(t) against add_image(t.cpu().numpy()[i]) image by image
images/s, and the compressed bytes per image over the wall time against the 55 GB/s link.
    python tests/perf/device_io_time.py [--frames N] [--reps R] [--json out.json]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from librir_amd.synthetic import inject_bad_pixels, s1_noisy_background  # noqa: E402
from librir_amd.video_io import IRMovie, IRSaver  # noqa: E402

LINK_GBS = 55.0


def best(fn, reps):
    fn()
    torch.cuda.synchronize()
    t = 1e9
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t = min(t, time.perf_counter() - t0)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    n, h, w = a.frames, 512, 640
    arr = inject_bad_pixels(s1_noisy_background(n, h, w), 50)
    ts = np.arange(n, dtype=np.int64) * 20000000
    res = {"frames": n, "height": h, "width": w}
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "s1.h264")
        with IRSaver(src, w, h, h) as s:
            for i in range(n):
                s.add_image(arr[i], int(ts[i]))
        comp = os.path.getsize(src)
        res["compressed_bytes_per_image"] = comp / n
        with IRMovie.from_filename(src) as mov:
            for filt in (False, True):
                mov.bad_pixels_correction = filt
                tag = "filters_on" if filt else "filters_off"
                t_host = best(lambda: torch.from_numpy(mov.data).cuda(), a.reps)
                res["host_route_%s_s" % tag] = t_host
                for dt, name in ((torch.uint16, "u16"), (torch.float32, "f32")):
                    out = torch.empty((n, h, w), dtype=dt, device="cuda")
                    t = best(lambda: mov.to_tensor(dtype=dt, out=out), a.reps)
                    res["to_tensor_%s_%s_s" % (name, tag)] = t
                    res["to_tensor_%s_%s_images_per_s" % (name, tag)] = n / t
                    print("read %-11s %s: to_tensor %7.1f ms (%6.0f images/s, compressed %5.1f GB/s = %4.1f %% of the link), host route %7.1f ms: %.2fx"
                          % (tag, name, t * 1e3, n / t, comp / t / 1e9, 100 * comp / t / 1e9 / LINK_GBS, t_host * 1e3, t_host / t))
            mov.bad_pixels_correction = False
            t_dev = mov.to_tensor()
        k = [0]

        def write_dev():
            k[0] += 1
            with IRSaver(os.path.join(d, "w%d.h264" % k[0]), w, h, h) as s:
                s.add_images(t_dev, ts)

        def write_host():
            k[0] += 1
            with IRSaver(os.path.join(d, "w%d.h264" % k[0]), w, h, h) as s:
                host = t_dev.cpu().numpy()
                for i in range(n):
                    s.add_image(host[i], int(ts[i]))

        tw_dev, tw_host = best(write_dev, a.reps), best(write_host, a.reps)
        res.update(add_images_s=tw_dev, add_images_images_per_s=n / tw_dev, per_frame_add_image_s=tw_host, per_frame_add_image_images_per_s=n / tw_host)
        print("write: add_images %7.1f ms (%6.0f images/s, compressed %5.1f GB/s), cpu() + add_image per image %7.1f ms (%6.0f images/s): %.2fx"
              % (tw_dev * 1e3, n / tw_dev, comp / tw_dev / 1e9, tw_host * 1e3, n / tw_host, tw_host / tw_dev))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
