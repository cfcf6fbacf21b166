"""GPU, perf: rate floors of device.window_median at 3x3 and 5x5 over 256 frames of 640x512 uint16, timed as tests/perf/rank_time.py times it.
The yardstick is device.median_filter, the reference's 3x3 filter, which moves the same 4WH bytes a frame, timed in the same process on the
same stack (tests/perf/morphology_time.py's measure).

Measured on one MI355X (tests/perf/rank_time.py, rounds of best-of-20; DESIGN.md section 7 has the rates): ratios to median_filter
    3x3: 1.25, 1.27, 1.26, 1.19, 1.20, 1.22, 1.18, 1.21, 1.26   (2.76-2.96 M frames/s against 2.25-2.42 M; lowest 1.183)
    5x5: 0.33, 0.33, 0.32, 0.31, 0.32, 0.31, 0.32, 0.32, 0.29   (0.69-0.76 M frames/s; lowest 0.293)
Each floor is 0.85 of the lowest ratio seen - the box-to-box spread that the README's ranges show for kernels of this kind; timing both sides
in one process removes the rest."""
import os
import sys

import pytest

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.perf]

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "perf"))

LOWEST_RATIO_SEEN = {3: 1.183, 5: 0.293}  # of the rate of median_filter
FLOORS = {size: 0.85 * ratio for size, ratio in LOWEST_RATIO_SEEN.items()}
N, REPS = 256, 20


@pytest.fixture(scope="module")
def median_rate():
    from morphology_time import measure

    return measure("median_filter", 3, N, REPS)


@pytest.mark.parametrize("size", sorted(FLOORS))
def test_rate_floor(median_rate, size):
    from rank_time import measure_rank

    rate = measure_rank(size, None, N, REPS)
    floor = FLOORS[size] * median_rate
    print("window_median %dx%d: %.4g frames/s; median_filter %.4g frames/s; ratio %.2f (floor %.2f)" % (size, size, rate, median_rate, rate / median_rate,
                                                                                                       FLOORS[size]))
    assert rate >= floor, "%dx%d: %.3g frames/s, %.2f of median_filter's %.3g (floor %.2f)" % (size, size, rate, rate / median_rate, median_rate, FLOORS[size])
