"""GPU, perf: rate floors of device.region_quantiles over 1 000 frames of 640x512 (S1), on a shared map of 16 rectangles and on per-frame
hot-spot maps from label_images, at percents (0.5,) and (0.25, 0.5, 0.75, 0.99), timed as tests/perf/region_quantiles_time.py times it: 0.7
of what that script measured when the feature was added, on one MI355X."""
import os
import sys

import pytest

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.perf]

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "perf"))

ONE, FOUR = (0.5,), (0.25, 0.5, 0.75, 0.99)
FLOORS = {  # frames/s
    ("rect16", ONE): 1.00e6,  # measured 1.43-1.48 M (0.68-0.70 ms a call)
    ("rect16", FOUR): 0.63e6,  # measured 0.90-0.97 M (1.03-1.11 ms)
    ("hotspots", ONE): 0.40e6,  # measured 0.576 M (1.74 ms; K = 329)
    ("hotspots", FOUR): 0.30e6,  # measured 0.432 M (2.31 ms)
}


@pytest.mark.parametrize("kind,percents", sorted(FLOORS))
def test_rate_floor(kind, percents):
    from region_quantiles_time import measure

    rate = measure(kind, percents, 1000, 10)
    floor = FLOORS[kind, percents]
    print("region_quantiles, %s at %s: %.4g frames/s (floor %.4g)" % (kind, percents, rate, floor))
    assert rate >= floor, "%s at %s: %.3g frames/s, floor %.3g" % (kind, percents, rate, floor)
