"""Seeded soak of the adaptive temporal downsampling (GPU box): random shapes, lossy heights, parameters, methods, stack lengths, value
ranges and splits into pushes, every result compared bit for bit with the oracle of tests/downsample_cases.py.  Prints one line per failure
and a last line "N cases, F failures"; the recorded run is in profiles/downsample_soak.txt.
    python tests/perf/soak_downsample.py [--cases N] [--seed S]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import downsample_cases as DC  # noqa: E402
from librir_amd import device as D  # noqa: E402


def one_case(rng):
    h, w = int(rng.integers(1, 70)), int(rng.integers(2, 200))
    if rng.random() < 0.4:
        w = (w + 7) // 8 * 8  # (the 16-byte form)
    lossy = int(rng.integers(1, h + 1))
    if w * lossy < 2:
        lossy = h = 2
    n = int(rng.integers(1, 330))
    factor = int(rng.choice([1, 2, 3, 4, 7, 10, 25]))
    factor_std = float(rng.choice([0., .25, .5, .75, .9, 1.]))
    method = int(rng.integers(1, 3))
    kind = rng.choice(["scene", "full", "four", "flip"])
    if kind == "scene":
        events = {int(i): int(rng.integers(50, 2000)) for i in rng.integers(0, n, 6)}
        f = DC.scene(n, h, w, seed=int(rng.integers(1 << 30)), events=events)
    elif kind == "full":
        f = rng.integers(0, 65536, (n, h, w), dtype=np.uint16)
    elif kind == "four":
        f = rng.integers(0, 4, (n, h, w)).astype(np.uint16) * np.uint16(21845)
    else:
        f = np.zeros((n, h, w), np.uint16)
        f[1::2] = 65535
        f[n // 2:, 0, 0] = 5
    cuts = sorted(set(rng.integers(1, n, int(rng.integers(0, 6))).tolist())) if n > 1 else []
    return dict(h=h, w=w, lossy=lossy, n=n, factor=factor, factor_std=factor_std, method=method, kind=str(kind), cuts=cuts), f


def run_case(p, f):
    stamps = DC.stamps(p["n"])
    exp = DC.oracle(f, stamps, p["factor"], p["factor_std"], p["lossy"], p["method"])
    fr = torch.from_numpy(f.view(np.int16)).cuda().view(torch.uint16)
    d = D.Downsampler(p["w"], p["h"], p["factor"], p["factor_std"], p["lossy"], p["method"])
    images, positions, stats = [], [], []
    edges = [0] + p["cuts"] + [p["n"]]
    for a, b in zip(edges[:-1], edges[1:]):
        got = d.push(fr[a:b], stamps[a:b])
        images.append(got.frames.cpu().numpy())
        positions.append(got.positions + a)
        stats.append(got.stats)
    positions = np.concatenate(positions).astype(np.int32)
    got = DC.Result(np.concatenate(images), positions, stamps[positions], np.concatenate(stats), None, None)
    assert d.close() == len(exp.positions)
    DC.same(got, exp, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=300)
    ap.add_argument("--seed", type=int, default=20261018)
    a = ap.parse_args()
    assert torch.cuda.is_available() and D.device_available(), "needs a GPU"
    rng = np.random.default_rng(a.seed)
    failures = 0
    for k in range(a.cases):
        p, f = one_case(rng)
        try:
            run_case(p, f)
        except AssertionError as e:
            failures += 1
            print("case %d %s: %s" % (k, p, str(e)[:300]), flush=True)
    print("seed %d: %d cases, %d failures" % (a.seed, a.cases, failures), flush=True)
    return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main())
