"""GPU, perf: rate floors of track_components over 1 000 label maps of 640x512 from the hot-spot scene (synthetic.hot_spots above 4 000,
labelled by label_images), with the track map and without: 0.7 of what tests/perf/track_time.py measured when the feature was added, on
one MI355X."""
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.perf]

FLOOR_RELABEL_ON = 0.68e6  # measured 0.98 M frames/s (1.02 ms a call)
FLOOR_RELABEL_OFF = 1.15e6  # measured 1.65 M (0.61 ms)


@pytest.fixture(scope="module")
def hot_spot_labels():
    from librir_amd import device as D
    from librir_amd.synthetic import hot_spots

    f = torch.from_numpy(hot_spots(1000, 512, 640).view(np.int16)).cuda().view(torch.uint16)
    labels, _, _, counts = D.label_images((f.view(torch.int16).to(torch.int32) & 0xFFFF) > 4000, table_entries=1)
    return labels, counts, int(counts.max())


@pytest.mark.parametrize("relabel,floor", [(True, FLOOR_RELABEL_ON), (False, FLOOR_RELABEL_OFF)])
def test_rate_floor(hot_spot_labels, relabel, floor):
    from librir_amd import device as D

    labels, counts, k = hot_spot_labels
    n = labels.shape[0]
    out = torch.empty_like(labels) if relabel else None
    for _ in range(3):
        D.track_components(labels, counts, k, relabel=relabel, out=out)
    torch.cuda.synchronize()
    reps = 20
    t0 = time.perf_counter()
    for _ in range(reps):
        D.track_components(labels, counts, k, relabel=relabel, out=out)
    torch.cuda.synchronize()
    rate = reps * n / (time.perf_counter() - t0)
    print("track_components, relabel %s: %.4g frames/s (floor %.4g)" % (relabel, rate, floor))
    assert rate >= floor, "relabel %s: %.3g frames/s, floor %.3g" % (relabel, rate, floor)
