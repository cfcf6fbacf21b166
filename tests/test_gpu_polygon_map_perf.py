"""GPU, perf: rate floors of polygon_map over 1 000 shifted 640x512 maps - 16 octagons covering 0.4 of the image, and 1 024 small
quadrilaterals - timed as tests/perf/polygon_map_time.py times them: 0.7 of what that script measured when the feature was added, on one
MI355X."""
import os
import sys

import pytest

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.perf]

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "perf"))

FLOOR_OCTAGONS = 1.17e6  # measured 1.67 M maps/s (0.597 ms a call)
FLOOR_QUADS = 0.27e6  # measured 0.385 M (2.60 ms)


@pytest.mark.parametrize("kind,floor", [("octagons", FLOOR_OCTAGONS), ("quads", FLOOR_QUADS)])
def test_rate_floor(kind, floor):
    from polygon_map_time import measure

    n = 1000
    t, _, covered = measure(kind, n, 10)
    print("polygon_map, %s: %.4g maps/s (floor %.4g)" % (kind, n / t, floor))
    assert 0.35 < covered < 0.45
    assert n / t >= floor, "%s: %.3g maps/s, floor %.3g" % (kind, n / t, floor)
