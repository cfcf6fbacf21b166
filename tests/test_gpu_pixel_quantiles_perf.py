"""GPU, perf: rate floors of pixel_quantiles over 1 000 frames of 640x512 of the S1 scene in one call, for the median alone and for three
percents: 0.7 of what tests/perf/pixel_quantiles_time.py measured when the feature was added, on one MI355X."""
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.perf]

FLOOR_Q1 = 1.03e6  # measured 1.47 M frames/s (0.680 ms a call; the frames are read 4 times)
FLOOR_Q3 = 0.46e6  # measured 0.646 M (1.548 ms; 4 reads, the three percents counted together)


@pytest.fixture(scope="module")
def s1_frames():
    from librir_amd.synthetic import s1_noisy_background

    return torch.from_numpy(s1_noisy_background(1000, 512, 640, seed=1).view(np.int16)).cuda().view(torch.uint16)


@pytest.mark.parametrize("percents,floor", [((0.5,), FLOOR_Q1), ((0.05, 0.5, 0.95), FLOOR_Q3)])
def test_rate_floor(s1_frames, percents, floor):
    from librir_amd import device as D

    n = s1_frames.shape[0]
    for _ in range(3):
        D.pixel_quantiles(s1_frames, percents)
    torch.cuda.synchronize()
    reps = 20
    t0 = time.perf_counter()
    for _ in range(reps):
        D.pixel_quantiles(s1_frames, percents)
    torch.cuda.synchronize()
    rate = reps * n / (time.perf_counter() - t0)
    print("pixel_quantiles, %d percents: %.4g frames/s (floor %.4g)" % (len(percents), rate, floor))
    assert rate >= floor, "%d percents: %.3g frames/s, floor %.3g" % (len(percents), rate, floor)
