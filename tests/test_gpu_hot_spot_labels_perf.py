"""GPU, perf: label_hot_spots over 1 000 frames of 640x512 (synthetic.hot_spots above 4 000) is not slower than what it replaces, timed in
the same run and in turns with it as tests/perf/hot_spot_label_time.py times it (the median of each over the turns, device events):
    (a) no filter: against the three torch passes of the mask and label_images on it.  Ratio >= 1.0; measured 1.34 (4.66-4.77 ms against 3.48-3.55)
    (b) high, min_area, max_area, clear_border: against the mask, label_images, scatter_reduce for the flags, cumsum and gather, after the
        two results were found equal bit for bit.  Ratio >= 1.0; measured 110-115 (440-450 ms against 3.87-4.05)
The bounds are the issue's: the new calls move strictly fewer bytes than the routes they are compared with."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.perf]

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "perf"))

TURNS = 7


@pytest.fixture(scope="module")
def hot_spot_frames():
    from librir_amd.synthetic import hot_spots

    return torch.from_numpy(hot_spots(1000, 512, 640).view(np.int16)).cuda().view(torch.uint16)


def test_no_filter_is_not_slower_than_mask_and_label_images(hot_spot_frames):
    import hot_spot_label_time as T

    old, new = T.no_filters(hot_spot_frames, TURNS)
    print("no filter: mask + label_images %.3f ms, label_hot_spots %.3f ms, ratio %.3f" % (old * 1e3, new * 1e3, old / new))
    assert old / new >= 1.0, "label_hot_spots %.3f ms, mask + label_images %.3f ms" % (new * 1e3, old * 1e3)


def test_four_filters_are_not_slower_than_the_torch_route(hot_spot_frames):
    import hot_spot_label_time as T

    old, new, kept = T.four_filters(hot_spot_frames, TURNS)  # (asserts the bit equality of the two results first)
    print("four filters: torch route %.3f ms, label_hot_spots %.3f ms, ratio %.3f (%.2f kept components a frame)" % (old * 1e3, new * 1e3, old / new, kept))
    assert old / new >= 1.0, "label_hot_spots %.3f ms, the torch route %.3f ms" % (new * 1e3, old * 1e3)
