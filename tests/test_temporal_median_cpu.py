"""CPU: the temporal median filter - its entry points are declared and exported, the Python API exists and checks its parameters without a
device, there is no CPU fallback, the oracle the GPU tests use agrees with a per-pixel restatement of the definition, and the kernels of
temporal_kernels.hip keep their window in registers (no scratch)."""
import ctypes as ct
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from librir_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def temporal_median_oracle(stack, window, threshold=0, rows=None, first=0, count=None, step=1):
    """the definition: output k = frame t = first + k * step; upper median of the window truncated at the stack's ends; threshold and rows rules"""
    n, h, w = stack.shape
    r = window // 2
    rows = h if rows is None else rows
    ts = list(range(first, n, step)) if count is None else [first + k * step for k in range(count)]
    out = np.empty((len(ts), h, w), np.uint16)
    for k, t in enumerate(ts):
        lo, hi = max(0, t - r), min(n - 1, t + r)
        m = np.sort(stack[lo:hi + 1], axis=0)[(hi - lo + 1) // 2]
        src = stack[t]
        res = np.where(np.abs(src.astype(np.int32) - m.astype(np.int32)) > threshold, m, src)
        res[rows:] = src[rows:]
        out[k] = res
    return out


def brute_force(stack, window, threshold, rows):
    n, h, w = stack.shape
    r = window // 2
    out = np.empty_like(stack)
    for t in range(n):
        for y in range(h):
            for x in range(w):
                vals = sorted(int(stack[u, y, x]) for u in range(max(0, t - r), min(n - 1, t + r) + 1))
                m, s = vals[len(vals) // 2], int(stack[t, y, x])
                out[t, y, x] = m if y < rows and abs(s - m) > threshold else s
    return out


@pytest.mark.parametrize("n,window,threshold,rows", [(1, 3, 0, 3), (2, 3, 0, 3), (5, 5, 0, 2), (6, 7, 1, 3), (9, 3, 1000, 3), (4, 63, 0, 0), (7, 1, 0, 3)])
def test_oracle_matches_the_definition_pixel_by_pixel(n, window, threshold, rows):
    rng = np.random.default_rng(n * 100 + window)
    stack = rng.integers(0, 65536, (n, 3, 4), dtype=np.uint16)
    stack[0, 0, 0], stack[-1, 0, 1] = 0, 65535
    assert np.array_equal(temporal_median_oracle(stack, window, threshold, rows), brute_force(stack, window, threshold, rows))
    assert np.array_equal(temporal_median_oracle(stack, window, threshold, rows, first=n - 1, count=1), brute_force(stack, window, threshold, rows)[-1:])


def test_entry_points_are_declared_and_exported(lib):
    dev = open(os.path.join(ROOT, "include", "rir_amd_device.h")).read()
    sp = open(os.path.join(ROOT, "include", "rir_amd_signal_processing.h")).read()
    assert re.search(r"int rir_temporal_median_device\(const unsigned short \*d_src, unsigned short \*d_dst, int w, int h, int nframes, int first, "
                     r"int count, int step,\s+int window, int threshold, int rows, void \*stream\);", dev)
    assert re.search(r"int rir_temporal_median\(const unsigned short \*src, unsigned short \*dst, int w, int h, int nframes, int window, "
                     r"int threshold, int rows\);", sp)
    assert hasattr(lib, "rir_temporal_median_device") and hasattr(lib, "rir_temporal_median")


def test_python_api_exists():
    from librir_amd import device as D
    from librir_amd import signal_processing as S

    assert callable(D.temporal_median) and callable(S.temporal_median) and "temporal_median" in S.__all__
    for m in ("push", "finish", "reset"):
        assert callable(getattr(D.TemporalMedian, m))
    from librir_amd.video_io import IRMovie
    import inspect

    params = inspect.signature(IRMovie.to_tensor).parameters
    assert "temporal_median" in params and "median_threshold" in params and params["temporal_median"].default is None


def test_no_cpu_fallback_without_device(lib):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from librir_amd.low_level.misc import last_error

    src = np.arange(3 * 4 * 5, dtype=np.uint16).reshape(3, 4, 5)
    dst = np.zeros_like(src)
    lib.rir_temporal_median.argtypes = [ct.c_void_p, ct.c_void_p] + [ct.c_int] * 6
    assert lib.rir_temporal_median(src.ctypes.data, dst.ctypes.data, 5, 4, 3, 3, 0, 4) == -1
    assert "no usable HIP device" in last_error()
    assert not dst.any()
    lib.rir_temporal_median_device.argtypes = [ct.c_void_p, ct.c_void_p] + [ct.c_int] * 9 + [ct.c_void_p]
    assert lib.rir_temporal_median_device(src.ctypes.data, dst.ctypes.data, 5, 4, 3, 0, 3, 1, 3, 0, 4, None) == -1
    assert not dst.any()
    from librir_amd import signal_processing as S

    with pytest.raises(RuntimeError):
        S.temporal_median(src, 3)


@pytest.mark.parametrize("kw", [dict(window=4), dict(window=65), dict(window=0), dict(window=3, threshold=65536), dict(window=3, threshold=-1),
                                dict(window=3, rows=5), dict(window=3, first=7), dict(window=3, first=-1), dict(window=3, count=7),
                                dict(window=3, first=2, count=3, step=2), dict(window=3, count=-1), dict(window=3, step=0)])
def test_device_entry_rejects_bad_parameters_without_a_device(kw):
    import torch

    from librir_amd import device as D

    frames = torch.zeros((6, 4, 5), dtype=torch.uint16)  # (a CPU tensor: the check comes before any device work)
    with pytest.raises(ValueError):
        D.temporal_median(frames, **kw)


@pytest.mark.parametrize("window", [4, 65, -1])
def test_host_entry_and_stream_reject_bad_windows_without_a_device(window):
    from librir_amd import device as D
    from librir_amd import signal_processing as S

    with pytest.raises(ValueError):
        S.temporal_median(np.zeros((6, 4, 5), np.uint16), window)
    with pytest.raises(ValueError):
        D.TemporalMedian(window)


HIPCC_FOUND = os.path.exists(B.HIPCC) or shutil.which(B.HIPCC) is not None


@pytest.mark.skipif(not HIPCC_FOUND, reason="hipcc not found")
def test_temporal_kernels_use_no_scratch(tmp_path):
    """every window's kernels keep their window in registers indexed by compile-time constants: no private segment"""
    asm = str(tmp_path / "temporal_kernels.s")
    flags = [f for f in B.COMMON if f != "-fPIC"]
    subprocess.check_call([B.HIPCC] + flags + ["-S", "--cuda-device-only", os.path.join(B.CSRC, "temporal_kernels.hip"), "-o", asm],
                          stderr=subprocess.DEVNULL)
    text = open(asm).read()
    meta = text[text.index("amdhsa.kernels:"):text.index(".end_amdgpu_metadata")]
    kernels = {}
    for block in re.split(r"\n  - ", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            kernels[name.group(1)] = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1))
    run = [k for k in kernels if k.startswith("_ZN3rir19temporal_median_run")]
    edge = [k for k in kernels if k.startswith("_ZN3rir20temporal_median_edge")]
    assert len(run) == 31 and len(edge) == 32, sorted(kernels)  # windows 3..63 (interior) and 1..63
    assert all(kernels[k] == 0 for k in run + edge), {k: v for k, v in kernels.items() if v}
