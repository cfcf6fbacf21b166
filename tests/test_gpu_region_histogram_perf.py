"""GPU, perf: device.region_histogram / device.histogram over 1 000 frames of 640x512 (S1), timed as tests/perf/region_histogram_time.py
times it, on one MI355X.  Two kinds of check: with the bins (0, 256, 256) the call does the one counting pass that
region_quantiles at one percent does before a second pass and two scans, so in one run, on one stack and map, it may not take longer - no
margin; and rate floors, 0.7 of what the script measured when the feature was added."""
import os
import sys

import pytest

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.perf]

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "perf"))

COARSE, BACKGROUND, FINE = (0, 256, 256), (0, 4, 16384), (7000, 1, 2048)
FLOORS = {  # frames/s
    ("nomap", COARSE): 2.09e6,  # measured 2.98 M (0.335 ms a call)
    ("nomap", BACKGROUND): 0.94e6,  # measured 1.35 M (0.741 ms)
    ("nomap", FINE): 3.84e6,  # measured 5.49 M (0.182 ms)
    ("one", COARSE): 1.99e6,  # measured 2.85 M (0.351 ms)
    ("one", BACKGROUND): 0.95e6,  # measured 1.36 M (0.733 ms)
    ("one", FINE): 3.04e6,  # measured 4.34 M (0.230 ms)
    ("rect16", COARSE): 1.86e6,  # measured 2.66 M (0.376 ms)
    ("rect16", BACKGROUND): 0.060e6,  # measured 0.0855 M (11.7 ms: fifteen regions of sixteen are beyond the LDS limit)
    ("hotspots", COARSE): 0.89e6,  # measured 1.27 M (0.789 ms; K = 329)
    ("rect16", FINE): 0.39e6,  # measured 0.560 M (1.786 ms: half of the counters are beyond the LDS limit)
    ("hotspots", FINE): 0.73e6,  # measured 1.05 M (0.950 ms; K = 329)
}


@pytest.mark.parametrize("kind", ["one", "rect16"])
def test_one_counting_pass_is_not_slower_than_region_quantiles(kind):
    from region_histogram_time import measure_pair

    th, tq = measure_pair(kind, 1000, 10)
    print("%s: region_histogram(256, 0, 256) %.3f ms, region_quantiles(0.5) %.3f ms" % (kind, th * 1e3, tq * 1e3))
    assert th <= tq, "%s: region_histogram %.3f ms, region_quantiles %.3f ms" % (kind, th * 1e3, tq * 1e3)


@pytest.mark.parametrize("kind,bins", sorted(FLOORS))
def test_rate_floor(kind, bins):
    from region_histogram_time import measure

    rate = measure(kind, bins, 1000, 10)
    floor = FLOORS[kind, bins]
    print("region_histogram, %s at %s: %.4g frames/s (floor %.4g)" % (kind, bins, rate, floor))
    assert rate >= floor, "%s at %s: %.3g frames/s, floor %.3g" % (kind, bins, rate, floor)
