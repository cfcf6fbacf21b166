"""GPU, perf: rate floor of Downsampler.push over 1 000 frames of 640x512 (the S1 scene with block events, factor 10, factor_std 0.9, both
methods), timed as tests/perf/downsample_time.py times it: 0.7 of what that script measured when the feature was added, on one MI355X
(DESIGN.md section 7)."""
import os
import sys

import pytest

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.perf]

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "perf"))

FLOORS = {1: 0.476e6, 2: 0.776e6}  # frames/s; measured 0.680 M (1.471 ms a push, 165 kept) and 1.109 M (0.902 ms, 123 kept)


@pytest.mark.parametrize("method", [1, 2])
def test_rate_floor(method):
    from downsample_time import measure

    r = measure(method, 1000, 10, with_torch=False)
    print("downsample push, method %d: %.4g frames/s (floor %.4g), %d kept" % (method, r["frames_per_s"], FLOORS[method], r["kept"]))
    assert 100 <= r["kept"] <= 250  # the grid and the events
    assert r["frames_per_s"] >= FLOORS[method], "method %d: %.3g frames/s, floor %.3g" % (method, r["frames_per_s"], FLOORS[method])
