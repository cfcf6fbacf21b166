"""GPU: a windowed read is faster than the whole read followed by a crop.  A condition, not a measurement: the windowed route does a
strict subset of the other route's file reads, link traffic, decode work and stores, so the bound is 1x and no more."""
import time

import numpy as np
import pytest

from librir_amd.synthetic import s1_noisy_background
from librir_amd.video_io import IRMovie, IRSaver

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.perf]


def test_window_read_beats_read_and_crop(tmp_path):
    n, h, w = 500, 512, 640
    win = (224, 288, 64, 64)
    arr = s1_noisy_background(n, h, w)
    frames = torch.from_numpy(arr.astype(np.int32)).to(torch.uint16).cuda()
    p = tmp_path / "s1.h264"
    with IRSaver(p, w, h, h) as s:
        s.add_images(frames, np.arange(n, dtype=np.int64) * 20000000)

    with IRMovie.from_filename(p) as mov:
        def windowed():
            return mov.to_tensor(window=win)

        def cropped():
            return mov.to_tensor()[:, 224:288, 288:352].contiguous()

        def best(fn):
            t = 1e9
            for _ in range(5):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                t = min(t, time.perf_counter() - t0)
            return t

        a, b = windowed(), cropped()  # the warm-up of each
        torch.cuda.synchronize()
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)) and torch.equal(a.view(torch.int16), frames[:, 224:288, 288:352].view(torch.int16))
        t_win, t_crop = best(windowed), best(cropped)
    print("to_tensor(window=%s) %.2f ms, to_tensor() + crop %.2f ms: %.2fx" % (win, t_win * 1e3, t_crop * 1e3, t_crop / t_win))
    assert t_win < t_crop
