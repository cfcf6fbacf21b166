"""GPU, perf: rate floors of device.local_threshold at 3x3, 9x9 and 15x15 and of device.box_mean at 9x9 over 256 frames of 640x512 uint16, timed
as tests/perf/local_time.py times them.  The yardstick is device.median_filter, the reference's 3x3 filter, timed in the same process on the
same stack (tests/perf/morphology_time.py's measure).

Measured on one MI355X (tests/perf/local_time.py, nine rounds of best-of-20; DESIGN.md section 7 has the rates): ratios to median_filter
    local_threshold 3x3:   0.61, 0.60, 0.61, 0.61, 0.61, 0.61, 0.62, 0.62, 0.59   (1.40-1.53 M frames/s against 2.32-2.51 M; lowest 0.593)
    local_threshold 9x9:   0.48, 0.48, 0.48, 0.48, 0.48, 0.48, 0.49, 0.48, 0.47   (1.12-1.20 M frames/s; lowest 0.471)
    local_threshold 15x15: 0.36, 0.35, 0.36, 0.36, 0.35, 0.36, 0.36, 0.35, 0.35   (0.84-0.88 M frames/s; lowest 0.345)
    box_mean 9x9:          0.75, 0.71, 0.72, 0.72, 0.71, 0.71, 0.73, 0.73, 0.71   (1.75-1.78 M frames/s; lowest 0.705)
Each floor is 0.85 of the lowest ratio seen - the box-to-box spread that the README's ranges show for kernels of this kind; timing both sides
in one process removes the rest."""
import os
import sys

import pytest

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.perf]

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "perf"))

LOWEST_RATIO_SEEN = {("local_threshold", 3): 0.593, ("local_threshold", 9): 0.471, ("local_threshold", 15): 0.345, ("box_mean", 9): 0.705}
FLOORS = {case: 0.85 * ratio for case, ratio in LOWEST_RATIO_SEEN.items()}  # of the rate of median_filter
N, REPS = 256, 20


@pytest.fixture(scope="module")
def median_rate():
    from morphology_time import measure

    return measure("median_filter", 3, N, REPS)


@pytest.mark.parametrize("form,size", sorted(FLOORS), ids=lambda v: str(v))
def test_rate_floor(median_rate, form, size):
    from local_time import measure_local

    rate = measure_local(form, size, N, REPS)
    floor = FLOORS[form, size] * median_rate
    print("%s %dx%d: %.4g frames/s; median_filter %.4g frames/s; ratio %.2f (floor %.2f)" % (form, size, size, rate, median_rate, rate / median_rate,
                                                                                            FLOORS[form, size]))
    assert rate >= floor, "%s %dx%d: %.3g frames/s, %.2f of median_filter's %.3g (floor %.2f)" % (form, size, size, rate, rate / median_rate, median_rate,
                                                                                                 FLOORS[form, size])
