"""GPU, perf: device.h_dome over 256 frames of 640x512 uint16 at h = 50 against the same result computed with what the library had before -
torch.minimum(device.dilate(F, 3), G) repeated until nothing changes, looked at every 8 iterations - timed as tests/perf/reconstruct_time.py
times them: the same stack, the same process, alternating rounds, the median over the rounds of the ratio of the two rates.

The floor is a ratio of 1.0 on each scene, and it is a structural claim, not a measurement: a tile converges in LDS, where the composed route
crosses HBM twice per pixel of reach.  What was measured is in DESIGN.md section 7."""
import os
import sys

import pytest

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.perf]

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "perf"))

FLOOR = 1.0
N, ROUNDS, REPS, SHIFT, CHECK_EVERY = 256, 3, 4, 50, 8


@pytest.fixture(scope="module")
def rounds():
    from reconstruct_time import check, rounds_of

    check(N, SHIFT, CHECK_EVERY)  # the two routes agree bit for bit
    return rounds_of(N, ROUNDS, REPS, SHIFT, CHECK_EVERY)


@pytest.mark.parametrize("scene", ["hot_spots", "blobs"])
def test_h_dome_is_no_slower_than_the_composed_route(rounds, scene):
    from reconstruct_time import summary

    rate, other, ratio, lo, hi = summary(rounds, scene)
    print("h_dome %s: %.4g frames/s; composed route %.4g frames/s; ratio %.2f (%.2f..%.2f; floor %.1f)" % (scene, rate, other, ratio, lo, hi, FLOOR))
    assert ratio >= FLOOR, "h_dome %s: %.3g frames/s, %.2f of the composed route's %.3g (floor %.1f)" % (scene, rate, ratio, other, FLOOR)
