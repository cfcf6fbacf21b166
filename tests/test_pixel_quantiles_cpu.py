"""CPU: per-pixel quantiles over time - the numpy oracle the GPU tests use agrees with region_quantiles' oracle on the transposed view and
with find_median_pixel under a mask of ones (the definition), the entry points are declared and exported, the size queries follow the
formulas the header documents and refuse bad arguments, there is no CPU fallback, the Python API checks its arguments without a device,
and the kernels of pixel_quantile_kernels.hip use no scratch and no compare-and-swap loop."""
import ctypes as ct
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from librir_amd import build as B
from test_region_quantiles_cpu import PERCENTS, quantile_rank, region_quantiles_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pixel_quantiles_oracle(frames, percents):
    """the contract with a sort along time: element t - 1 of every pixel's sorted series, t = (int)roundf((float)n * p); -1 for no frames,
    0 where t == 0, t > n or the element is 65535.  frames (n, h, w) uint16 -> int32 (len(percents), h, w)"""
    frames = np.asarray(frames)
    if frames.ndim == 2:
        frames = frames[None]
    n, h, w = frames.shape
    percents = np.atleast_1d(np.asarray(percents, np.float32))
    out = np.full((percents.size, h, w), -1, np.int32)
    if n == 0:
        return out
    s = np.sort(frames, axis=0)
    for j, p in enumerate(percents):
        t = quantile_rank(n, p)
        if t < 1 or t > n:
            out[j] = 0
        else:
            out[j] = np.where(s[t - 1] == 65535, 0, s[t - 1])
    return out


def full_range_stack(seed, n, h, w):
    """full-range values with planted columns of 0 and of 65535 in time and one pixel that is 65535 throughout"""
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 65536, (n, h, w), dtype=np.uint16)
    flat = f.reshape(n, -1)
    flat[::3, 1::7] = 0
    flat[1::4, 2::5] = 65535
    flat[:, 3] = 0
    flat[:, 4] = 65535
    flat[:, -1] = 65535
    return f


STACKS = [(1, 3, 5), (2, 3, 5), (7, 5, 7), (257, 8, 9)]


@pytest.mark.parametrize("n,h,w", STACKS)
def test_oracle_is_region_quantiles_over_the_transposed_view(n, h, w):
    f = full_range_stack(n, n, h, w)
    exp = pixel_quantiles_oracle(f, PERCENTS)
    assert exp.dtype == np.int32 and exp.shape == (len(PERCENTS), h, w)
    labels = np.broadcast_to(np.arange(h * w, dtype=np.int32), (n, h * w))
    count, values = region_quantiles_oracle(f.reshape(1, n, h * w), labels, h * w, PERCENTS)
    assert (count == n).all()
    assert np.array_equal(values[0].T.reshape(len(PERCENTS), h, w), exp)
    assert (exp[:, -1, -1] == 0).all()  # 65535 throughout


def against_find_median_pixel(impl, f):
    n, h, w = f.shape
    exp = pixel_quantiles_oracle(f, PERCENTS)
    ones = np.ones((1, n), np.uint8)
    for y in range(h):
        for x in range(w):
            series = np.ascontiguousarray(f[:, y, x]).reshape(1, n)
            for j, p in enumerate(PERCENTS):
                assert exp[j, y, x] == impl.find_median_pixel(series, p, ones), (y, x, p)


@pytest.mark.parametrize("n,h,w", STACKS)
def test_oracle_is_find_median_pixel_of_each_series(oracle, n, h, w):
    against_find_median_pixel(oracle, full_range_stack(n, n, h, w))


@pytest.mark.parametrize("n,h,w", STACKS)
def test_oracle_is_the_compiled_reference_without_65535(ref, n, h, w):
    f = full_range_stack(n, n, h, w)
    f[f == 65535] = 65534
    against_find_median_pixel(ref, f)


def test_oracle_edges():
    assert (pixel_quantiles_oracle(np.zeros((0, 2, 3), np.uint16), (0.5, 1.0)) == -1).all()
    f = np.array([10, 20, 30, 40, 50, 60, 70], np.uint16).reshape(7, 1, 1)
    for c in (1, 2, 3, 5, 6, 7):
        got = pixel_quantiles_oracle(f[:c], (0.25, 0.5, 0.75))[:, 0, 0].tolist()
        assert got == [10 * quantile_rank(c, p) for p in (0.25, 0.5, 0.75)]
    assert pixel_quantiles_oracle(f, 0.0)[0, 0, 0] == 0 and pixel_quantiles_oracle(f, 1.0)[0, 0, 0] == 70
    assert pixel_quantiles_oracle(f[0], 0.5).shape == (1, 1, 1)  # one image: a stack of one


def test_entry_points_are_declared_and_exported(lib):
    dev = open(os.path.join(ROOT, "include", "rir_amd_device.h")).read()
    sp = open(os.path.join(ROOT, "include", "rir_amd_signal_processing.h")).read()
    assert re.search(r"int\s+rir_pixel_quantiles_passes\(void\);", dev)
    assert re.search(r"size_t\s+rir_pixel_quantiles_state_bytes\(int w, int h, int npercents\);", dev)
    assert re.search(r"size_t\s+rir_pixel_quantiles_workspace_bytes\(int w, int h, int nframes, int npercents\);", dev)
    assert re.search(r"int\s+rir_pixel_quantiles_device\(const unsigned short \*d_frames, int w, int h, int nframes,\s+"
                     r"const float \*percents /\* HOST \*/, int npercents, int \*d_values /\* \[npercents\]\[h\]\[w\] \*/,\s+"
                     r"void \*d_work, size_t work_bytes, void \*stream\);", dev)
    assert re.search(r"int\s+rir_pixel_quantiles_push_device\(const unsigned short \*d_frames, int w, int h, int nframes, int npercents, "
                     r"int pass,\s+void \*d_state, size_t state_bytes, void \*stream\);", dev)
    assert re.search(r"int\s+rir_pixel_quantiles_resolve_device\(int w, int h, const float \*percents /\* HOST \*/, int npercents, int pass,\s+"
                     r"long long total_frames, void \*d_state, size_t state_bytes,\s+int \*d_values /\*[^*]*\*/, void \*stream\);", dev)
    assert re.search(r"int\s+rir_pixel_quantiles\(const unsigned short \*frames, int w, int h, int nframes,\s+"
                     r"const float \*percents, int npercents, int \*values\);", sp)
    assert "ALL-ZERO state is the empty state" in dev
    for name in ("rir_pixel_quantiles_passes", "rir_pixel_quantiles_state_bytes", "rir_pixel_quantiles_workspace_bytes",
                 "rir_pixel_quantiles_device", "rir_pixel_quantiles_push_device", "rir_pixel_quantiles_resolve_device", "rir_pixel_quantiles"):
        assert hasattr(lib, name), name
    # both quantile units compile one rank expression
    rank = open(os.path.join(B.CSRC, "quantile_rank.h")).read()
    assert "roundf(__fmul_rn((float)c, percent))" in rank
    for unit in ("quantile_kernels.hip", "pixel_quantile_kernels.hip"):
        text = open(os.path.join(B.CSRC, unit)).read()
        assert '#include "quantile_rank.h"' in text and "__fmul_rn" not in text, unit


def size_queries(lib):
    state, work, passes = lib.rir_pixel_quantiles_state_bytes, lib.rir_pixel_quantiles_workspace_bytes, lib.rir_pixel_quantiles_passes
    state.argtypes, state.restype = [ct.c_int] * 3, ct.c_size_t
    work.argtypes, work.restype = [ct.c_int] * 4, ct.c_size_t
    passes.argtypes, passes.restype = [], ct.c_int
    return state, work, passes


def test_size_queries(lib):
    state, work, passes = size_queries(lib)
    assert 1 <= passes() <= 16
    for w, h, q in [(1, 1, 1), (5, 3, 8), (640, 512, 1), (640, 512, 3), (640, 512, 8), (65535, 32768, 1), (1024, 768, 2)]:
        got = state(w, h, q)
        assert got == 72 * q * w * h, (w, h, q)  # 16 counts, the prefix and the rank: 18 uint32 per percent and pixel
        assert got % 8 == 0 and got <= 128 * q * w * h + 4096
        for n in (0, 1, 1000, 2147483647):
            assert work(w, h, n, q) == got and work(w, h, n, q) > 0
    for bad in [(0, 5, 1), (5, 0, 1), (-1, 5, 1), (5, -1, 1), (65536, 32768, 1), (46341, 46341, 1), (5, 5, 0), (5, 5, 9), (5, 5, -1)]:
        assert state(*bad) == 0, bad
        assert work(bad[0], bad[1], 1, bad[2]) == 0, bad
    assert work(5, 5, -1, 1) == 0


def test_size_queries_do_not_depend_on_the_cut_along_time(lib):
    """the grid of test_pixel_stats_cpu.py's plan test: 72 bytes per (percent, pixel), however many slabs the counting launch has"""
    from test_pixel_stats_cpu import PLAN_LENGTHS, PLAN_SHAPES

    state, work, _ = size_queries(lib)
    for w, h in PLAN_SHAPES:
        for q in (1, 3, 8):
            assert state(w, h, q) == 72 * q * w * h, (w, h, q)
            for n in PLAN_LENGTHS:
                assert work(w, h, n, q) == 72 * q * w * h, (w, h, n, q)


PUSH_ARGS = [ct.c_void_p] + [ct.c_int] * 5 + [ct.c_void_p, ct.c_size_t, ct.c_void_p]
RESOLVE_ARGS = [ct.c_int, ct.c_int, ct.c_void_p, ct.c_int, ct.c_int, ct.c_longlong, ct.c_void_p, ct.c_size_t, ct.c_void_p, ct.c_void_p]
DEV_ARGS = [ct.c_void_p] + [ct.c_int] * 3 + [ct.c_void_p, ct.c_int, ct.c_void_p, ct.c_void_p, ct.c_size_t, ct.c_void_p]
HOST_ARGS = [ct.c_void_p] + [ct.c_int] * 3 + [ct.c_void_p, ct.c_int, ct.c_void_p]


def test_no_cpu_fallback_without_device(lib):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from librir_amd.low_level.misc import last_error

    frames = np.arange(2 * 3 * 5, dtype=np.uint16).reshape(2, 3, 5)
    pc = np.array([0.5, 1.0], np.float32)
    values = np.full((2, 3, 5), 7, np.int32)
    state = np.full(72 * 2 * 15 // 8, 5, np.int64)
    lib.rir_pixel_quantiles.argtypes = HOST_ARGS
    assert lib.rir_pixel_quantiles(frames.ctypes.data, 5, 3, 2, pc.ctypes.data, 2, values.ctypes.data) == -1
    assert "no usable HIP device" in last_error()
    lib.rir_pixel_quantiles_device.argtypes = DEV_ARGS
    assert lib.rir_pixel_quantiles_device(frames.ctypes.data, 5, 3, 2, pc.ctypes.data, 2, values.ctypes.data, state.ctypes.data, state.nbytes,
                                          None) == -1
    assert "no usable HIP device" in last_error()
    lib.rir_pixel_quantiles_push_device.argtypes = PUSH_ARGS
    assert lib.rir_pixel_quantiles_push_device(frames.ctypes.data, 5, 3, 2, 2, 0, state.ctypes.data, state.nbytes, None) == -1
    assert "no usable HIP device" in last_error()
    lib.rir_pixel_quantiles_resolve_device.argtypes = RESOLVE_ARGS
    assert lib.rir_pixel_quantiles_resolve_device(5, 3, pc.ctypes.data, 2, 3, 2, state.ctypes.data, state.nbytes, values.ctypes.data, None) == -1
    assert "no usable HIP device" in last_error()
    assert (values == 7).all() and (state == 5).all()
    from librir_amd import signal_processing as S

    with pytest.raises(RuntimeError):
        S.pixel_quantiles(frames, 0.5)


def test_python_api_exists():
    from librir_amd import device as D
    from librir_amd import signal_processing as S
    from librir_amd.video_io import IRMovie

    assert callable(D.pixel_quantiles) and callable(S.pixel_quantiles) and "pixel_quantiles" in S.__all__
    assert list(inspect.signature(D.pixel_quantiles).parameters) == ["frames", "percents"]
    assert list(inspect.signature(S.pixel_quantiles).parameters) == ["images", "percents"]
    params = inspect.signature(D.PixelQuantileSelector).parameters
    assert list(params) == ["percents", "shape", "device"] and params["shape"].default is None and params["device"].default is None
    for name in ("push", "next_pass", "result", "reset"):
        assert callable(getattr(D.PixelQuantileSelector, name))
    assert list(inspect.signature(D.PixelQuantileSelector.push).parameters) == ["self", "frames"]
    params = inspect.signature(IRMovie.pixel_quantiles).parameters
    assert list(params)[1:] == ["percents", "selection"] and params["selection"].default == slice(None)
    assert IRMovie._QUANTILE_RESIDENT_BYTES == 1 << 30
    assert "track_hot_spots" in IRMovie.pixel_quantiles.__doc__
    sel = D.PixelQuantileSelector((0.05, 0.5))
    assert sel.passes == 4
    with pytest.raises(RuntimeError):
        sel.result()  # asked too early: no pass is closed


@pytest.mark.parametrize("shape,dtype,percents,exc", [
    ((2, 4, 5), "int16", 0.5, RuntimeError),
    ((2, 4, 5), "float32", 0.5, RuntimeError),
    ((2, 4, 5), "int32", 0.5, RuntimeError),
    ((5,), "uint16", 0.5, ValueError),
    ((2, 2, 4, 5), "uint16", 0.5, ValueError),
    ((2, 0, 5), "uint16", 0.5, ValueError),
    ((2, 4, 5), "uint16", (), ValueError),
    ((2, 4, 5), "uint16", (0.1,) * 9, ValueError),
    ((2, 4, 5), "uint16", ((0.1, 0.2),), ValueError),
    ((2, 4, 5), "uint16", -0.01, ValueError),
    ((2, 4, 5), "uint16", (0.5, 1.01), ValueError),
    ((2, 4, 5), "uint16", (0.5, float("nan")), ValueError),
])
def test_python_checks_raise_without_a_device(shape, dtype, percents, exc):
    """CPU tensors: every check comes before any device work"""
    import torch

    from librir_amd import device as D
    from librir_amd import signal_processing as S

    fr = torch.zeros(shape, dtype=getattr(torch, dtype))
    with pytest.raises(exc):
        D.pixel_quantiles(fr, percents)
    with pytest.raises(exc):
        D.PixelQuantileSelector(percents).push(fr)
    with pytest.raises(exc):
        S.pixel_quantiles(np.zeros(shape, getattr(np, dtype)), percents)


def test_device_entry_refuses_cpu_tensors():
    import torch

    from librir_amd import device as D

    with pytest.raises(RuntimeError, match="CUDA"):
        D.pixel_quantiles(torch.zeros((2, 4, 5), dtype=torch.uint16), (0.5, 0.99))
    with pytest.raises(RuntimeError, match="CUDA"):
        D.PixelQuantileSelector(0.5).push(torch.zeros((2, 4, 5), dtype=torch.uint16))
    with pytest.raises(ValueError):
        D.PixelQuantileSelector(0.5, shape=(0, 5))


HIPCC_FOUND = os.path.exists(B.HIPCC) or shutil.which(B.HIPCC) is not None


@pytest.mark.skipif(not HIPCC_FOUND, reason="hipcc not found")
def test_pixel_quantile_kernels_use_no_scratch_and_no_cmpswap(tmp_path):
    """registers and LDS only: no private segment in any kernel of the unit, no compare-and-swap loop"""
    asm = str(tmp_path / "pixel_quantile_kernels.s")
    flags = [f for f in B.COMMON if f != "-fPIC"]
    subprocess.check_call([B.HIPCC] + flags + ["-S", "--cuda-device-only", os.path.join(B.CSRC, "pixel_quantile_kernels.hip"), "-o", asm],
                          stderr=subprocess.DEVNULL)
    text = open(asm).read()
    assert "cmpswap" not in text.lower()
    meta = text[text.index("amdhsa.kernels:"):text.index(".end_amdgpu_metadata")]
    kernels = {}
    for block in re.split(r"\n  - ", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            kernels[name.group(1)] = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1))
    assert any("pixel_quantiles_count" in k for k in kernels) and any("pixel_quantiles_resolve" in k for k in kernels), sorted(kernels)
    assert all(v == 0 for v in kernels.values()), kernels
