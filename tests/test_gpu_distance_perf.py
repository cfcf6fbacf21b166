"""GPU, perf: rate floors of device.distance_transform over 256 masks of 640x512 uint8, timed as tests/perf/distance_time.py times it.  The
yardstick is device.morphology(mask, "erode", 15) - the largest structuring element of the window filters - on the same stack in the same
process, in alternating rounds; the figure held is the median over five rounds of the ratio of the two rates.

Measured on one MI355X, 2026-10-21, medians of 5 alternating rounds of 5 calls in one session (lowest..highest ratio of a round; erode 15x15
on the same stacks: 0.254-0.256 M frames/s):

    scene (a) hot spots above a threshold   dist2 0.870 (0.865..0.913)   dist2 + index 0.766 (0.762..0.810)
    scene (b) its inversion                 dist2 1.342 (1.321..1.374)   dist2 + index 1.157 (1.144..1.195)

The floors are 0.8 of these ratios: 0.8 covers the +-10 % run-to-run spread of the rates in README.md.  Scene (b), the distance from
everywhere to a few spots, is the one that a search outward from each pixel would lose: it runs FASTER than scene (a) here, because rows
without a background cell never enter the envelope (DESIGN.md section 7 has the rates)."""
import os
import statistics
import sys

import pytest

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.perf]

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "perf"))

MEASURED = {("hot_spots", False): 0.870, ("hot_spots", True): 0.766, ("inverted", False): 1.342, ("inverted", True): 1.157}  # x erode 15
FLOORS = {k: 0.8 * v for k, v in MEASURED.items()}
N, ROUNDS, REPS = 256, 5, 5


@pytest.fixture(scope="module")
def rounds():
    from distance_time import rounds_of

    return rounds_of(N, ROUNDS, REPS, scenes=("hot_spots", "inverted"))


@pytest.mark.parametrize("scene,indices", sorted(FLOORS))
def test_rate_floor(rounds, scene, indices):
    from distance_time import summary

    rate, ratio, lo, hi = summary(rounds, scene, indices)
    yard = statistics.median(r["yardstick", scene] for r in rounds)
    what = "distance_transform %s%s" % (scene, " with indices" if indices else "")
    print("%s: %.4g frames/s; erode 15x15 %.4g frames/s; ratio %.3f (%.3f..%.3f; floor %.3f)" % (what, rate, yard, ratio, lo, hi, FLOORS[scene, indices]))
    assert ratio >= FLOORS[scene, indices], "%s: %.3g frames/s, %.3f of erode 15x15's %.3g (floor %.3f)" % (what, rate, ratio, yard, FLOORS[scene, indices])
