"""GPU, perf: rate floors of device.morphology at 3x3 over 256 frames of 640x512 uint16, timed as tests/perf/morphology_time.py times it.  The
yardstick is device.median_filter, the 3x3 rank filter that moves the same 4WH bytes a frame, timed in the same process on the same stack:
a separable 3x3 min needs about a fifth of its comparisons, so erode and dilate reach at least its rate; a fused 3x3 opening needs about
two fifths, so open and tophat reach at least 0.8 of it - which two passes over the stack cannot (DESIGN.md section 7 has the rates)."""
import os
import sys

import pytest

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.perf]

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "perf"))

FLOORS = {"erode": 1.0, "dilate": 1.0, "open": 0.8, "tophat": 0.8}  # of the rate of median_filter
N, REPS = 256, 20


@pytest.fixture(scope="module")
def median_rate():
    from morphology_time import measure

    return measure("median_filter", 3, N, REPS)


@pytest.mark.parametrize("op", sorted(FLOORS))
def test_rate_floor(median_rate, op):
    from morphology_time import measure

    rate = measure(op, 3, N, REPS)
    floor = FLOORS[op] * median_rate
    print("morphology %s 3x3: %.4g frames/s; median_filter %.4g frames/s; ratio %.2f (floor %.2f)" % (op, rate, median_rate, rate / median_rate, FLOORS[op]))
    assert rate >= floor, "%s 3x3: %.3g frames/s, %.2f of median_filter's %.3g (floor %.2f)" % (op, rate, rate / median_rate, median_rate, FLOORS[op])
