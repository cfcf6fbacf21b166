"""CPU: the windowed device read (rir_load_window_device, IRMovie.to_tensor(window=...)) - exported, declared in the public header,
refusing bad arguments with -1 and the output untouched, failing loudly without a device; the window checked in Python before any
device call."""
import os
import re
import subprocess

import numpy as np
import pytest

from librir_amd.video_io import IRMovie
from librir_amd.video_io import rir_video_io as rv
from librir_amd.video_io.IRMovie import create_pcr_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "rir_load_window_device"
N, H, W = 3, 8, 16


def write_pcr(path, frames):
    n, h, w = frames.shape
    with open(path, "wb") as f:
        f.write(create_pcr_header(h, w, 50).astype(np.uint32).tobytes())
        f.write(frames.astype(np.uint16).tobytes())
    return path


def test_symbol_is_exported_and_declared():
    from librir_amd.low_level.misc import _video_io

    out = subprocess.run(["nm", "-D", "--defined-only", _video_io._name], stdout=subprocess.PIPE, check=True).stdout.decode()
    header = open(os.path.join(ROOT, "include", "rir_amd_video_io.h")).read()
    assert re.search(r"\bT %s$" % SYMBOL, out, re.M)
    assert re.search(r"\bint %s\(" % SYMBOL, header)
    assert hasattr(rv, "load_window_device") and rv._v.rir_load_window_device.argtypes is not None


def test_bad_arguments_return_minus_one(tmp_path):
    p = write_pcr(tmp_path / "m.pcr", np.arange(N * H * W, dtype=np.uint16).reshape(N, H, W))
    cam = rv.open_camera_file(p)
    buf = np.zeros((N, H, W), np.uint16)
    ptr, nb = buf.ctypes.data, buf.nbytes
    load = rv._v.rir_load_window_device
    code = ord("H")
    h, w = 4, 8
    assert load(0, 0, 1, 1, 0, 0, h, w, code, ptr, nb, None) == -1  # no such camera
    assert load(cam, 0, 1, 0, 0, 0, h, w, code, ptr, nb, None) == -1  # step 0
    assert load(cam, 0, 1, -1, 0, 0, h, w, code, ptr, nb, None) == -1
    assert load(cam, -1, 1, 1, 0, 0, h, w, code, ptr, nb, None) == -1  # images outside the file
    assert load(cam, 0, N + 1, 1, 0, 0, h, w, code, ptr, nb, None) == -1
    assert load(cam, 0, 3, 2, 0, 0, h, w, code, ptr, nb, None) == -1  # 0, 2, 4: past the end
    assert load(cam, 0, -1, 1, 0, 0, h, w, code, ptr, nb, None) == -1
    for y0, x0, hh, ww in ((-1, 0, 2, 2), (0, -1, 2, 2), (0, 0, 0, 4), (0, 0, 4, 0), (0, 0, -3, 4), (0, 0, H + 1, 1), (0, 0, 1, W + 1),
                           (H - 1, 0, 2, 1), (0, W - 1, 1, 2), (H, 0, 1, 1), (0, W, 1, 1), (2 ** 31 - 1, 0, 2, 2), (0, 0, 2 ** 31 - 1, 2)):
        assert load(cam, 0, 1, 1, y0, x0, hh, ww, code, ptr, nb, None) == -1, (y0, x0, hh, ww)  # a window outside the image, or empty
    assert load(cam, 0, N, 1, 0, 0, h, w, code, ptr, N * h * w * 2 - 1, None) == -1  # one byte short
    assert load(cam, 0, N, 1, 0, 0, h, w, ord("f"), ptr, N * h * w * 2, None) == -1  # float32 needs twice the bytes
    assert load(cam, 0, 1, 1, 0, 0, h, w, ord("d"), ptr, nb, None) == -1  # unknown dtype
    assert load(cam, 0, 1, 1, 0, 0, h, w, code, None, nb, None) == -1  # no output
    assert not buf.any()
    assert load(cam, 0, 0, 1, 0, 0, h, w, code, None, 0, None) == 0  # an empty selection
    assert load(cam, 1, 0, 3, 2, 3, 1, 1, ord("f"), ptr, 0, None) == 0
    assert not buf.any()
    rv.close_camera(cam)


def test_without_device_it_fails_and_logs(tmp_path):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from librir_amd.low_level.misc import last_error

    p = write_pcr(tmp_path / "m.pcr", np.ones((N, H, W), np.uint16))
    cam = rv.open_camera_file(p)
    buf = np.zeros((N, 2, 4), np.uint16)
    assert rv._v.rir_load_window_device(cam, 0, N, 1, 1, 2, 2, 4, ord("H"), buf.ctypes.data, buf.nbytes, None) == -1
    assert "no usable HIP device" in last_error()
    assert not buf.any()
    rv.close_camera(cam)


@pytest.mark.parametrize("method", ["to_tensor", "region_stats_window", "pixel_stats_window"])
def test_window_is_checked_before_any_device_call(tmp_path, method):
    """(the checks raise ValueError on a machine without a device too: nothing of the device is touched before them)"""
    p = write_pcr(tmp_path / "m.pcr", np.ones((N, H, W), np.uint16))
    with IRMovie.from_filename(p) as mov:
        def call(window):
            if method == "to_tensor":
                return mov.to_tensor(window=window)
            if method == "region_stats_window":
                return mov.region_stats_window(np.zeros((2, 2), np.int32), window)
            return mov.pixel_stats_window(window)

        for window in ((0, 0, 0, 4), (-1, 0, 2, 2), (0, 0, H + 1, 1), (0, W - 1, 1, 2), (0, 0, 4), (0.0, 0.0, 2.0, 2.0), (0, 0, 2, 2.0),
                       (0, -1, 2, 2), (0, 0, 4, 0), (H, 0, 1, 1), (0, 0, 1, W + 1), (0, 0, 2, 2, 2), "abcd", 5,
                       (np.int64(0), 0, 2, 2)):
            with pytest.raises(ValueError):
                call(window)
