"""GPU, perf: rate floors of device.region_geometry over 1 000 frames of 640x512 (S1), weighted by the frames on shared maps of 16 rectangles
and of 1 024 blobs and on per-frame hot-spot maps from label_images, and on those hot-spot maps alone, timed as
tests/perf/region_geometry_time.py times it: 0.7 of what that script measured when the feature was added, on one MI355X."""
import os
import sys

import pytest

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.perf]

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "perf"))

FLOORS = {  # frames/s
    ("rect16", True): 0.64e6,  # measured 0.912-0.918 M (1.09-1.10 ms a call)
    ("blob1024", True): 0.46e6,  # measured 0.657-0.659 M (1.52 ms)
    ("hotspots", True): 1.33e6,  # measured 1.89-1.96 M (0.51-0.53 ms; K = 329)
    ("hotspots", False): 1.68e6,  # measured 2.40-2.45 M (0.41-0.42 ms)
}


@pytest.mark.parametrize("kind,weighted", sorted(FLOORS))
def test_rate_floor(kind, weighted):
    from region_geometry_time import measure

    rate = measure(kind, weighted, 1000, 10)
    floor = FLOORS[kind, weighted]
    print("region_geometry, %s, %s: %.4g frames/s (floor %.4g)" % (kind, "weighted" if weighted else "labels only", rate, floor))
    assert rate >= floor, "%s, weighted %s: %.3g frames/s, floor %.3g" % (kind, weighted, rate, floor)
