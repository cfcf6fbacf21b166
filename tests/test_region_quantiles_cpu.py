"""CPU: per-region quantiles - the numpy oracle the GPU tests use agrees with find_median_pixel under the mask labels == r (the definition),
the entry points are declared and exported and refuse bad arguments, there is no CPU fallback, the Python API checks its arguments without a
device, and the kernels of quantile_kernels.hip use no scratch and no compare-and-swap loop."""
import ctypes as ct
import inspect
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from librir_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PERCENTS = (0.0, 0.001, 0.25, 0.5, 0.75, 0.9, 0.99, 1.0)


def quantile_rank(c, p):
    """t = (int)roundf((float)c * p): the product in float32, rounded half away from zero (np.round rounds half to even: 0 for c = 1,
    p = 0.5, where roundf gives 1)"""
    return int(math.floor(float(np.float32(c) * np.float32(p)) + 0.5))


def region_quantiles_oracle(frames, labels, nregions, percents):
    """the contract with a sort: per frame the pixels ordered by (label, value), element t - 1 of each region's segment; -1 for an empty
    region, 0 where t == 0, t > count or the element is 65535.  -> (count [n][nregions], values [n][nregions][len(percents)]), int32"""
    frames = np.asarray(frames)
    if frames.ndim == 2:
        frames = frames[None]
    n, h, w = frames.shape
    percents = np.atleast_1d(np.asarray(percents, np.float32))
    lab = np.broadcast_to(np.asarray(labels, np.int64), (n, h, w)).reshape(n, -1)
    count = np.zeros((n, nregions), np.int32)
    values = np.zeros((n, nregions, percents.size), np.int32)
    for f in range(n):
        keep = (lab[f] >= 0) & (lab[f] < nregions)
        lf, vf = lab[f][keep], frames[f].reshape(-1)[keep].astype(np.int64)
        ordered = vf[np.lexsort((vf, lf))]
        c = np.bincount(lf, minlength=nregions).astype(np.int64)
        start = np.cumsum(c) - c
        count[f] = c
        for j, p in enumerate(percents):
            t = np.floor((c.astype(np.float32) * np.float32(p)).astype(np.float64) + 0.5).astype(np.int64)
            pick = (t >= 1) & (t <= c)
            s = np.zeros(nregions, np.int64)
            s[pick] = ordered[(start + t - 1)[pick]]
            s[s == 65535] = 0
            values[f, :, j] = np.where(c == 0, -1, s)
    return count, values


def full_range_case(seed, n, h, w, k, per_frame=False):
    """full-range values with planted 0s and 65535s; labels from -1 to k (both ends ignored)"""
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 65536, (n, h, w), dtype=np.uint16)
    frames.reshape(n, -1)[:, ::7] = 0
    frames.reshape(n, -1)[:, 3::11] = 65535
    labels = rng.integers(-1, k + 1, (n, h, w) if per_frame else (h, w)).astype(np.int32)
    return frames, labels


CASES = [(2, 5, 7, 3), (2, 17, 33, 9), (1, 64, 80, 40)]


def against_find_median_pixel(impl, frames, labels, k):
    count, values = region_quantiles_oracle(frames, labels, k, PERCENTS)
    checked = 0
    for f in range(frames.shape[0]):
        lab = labels[f] if labels.ndim == 3 else labels
        for r in range(k):
            mask = lab == r
            assert count[f, r] == mask.sum()
            if not mask.any():
                assert (values[f, r] == -1).all()
                continue
            for j, p in enumerate(PERCENTS):
                assert values[f, r, j] == impl.find_median_pixel(frames[f], p, mask.astype(np.uint8)), (f, r, p)
                checked += 1
    return checked


@pytest.mark.parametrize("n,h,w,k", CASES)
def test_oracle_is_find_median_pixel_under_each_region_mask(oracle, n, h, w, k):
    frames, labels = full_range_case(n * 100 + k, n, h, w, k, per_frame=k == 9)
    assert against_find_median_pixel(oracle, frames, labels, k) > 0


def test_oracle_with_whole_rows_of_65535(oracle):
    frames, labels = full_range_case(5, 2, 17, 33, 9)
    frames[:, 4:9] = 65535
    labels[5:8] = 2  # region 2: mostly 65535
    labels[8] = 3  # region 3: a row of 65535 and whatever the random map gave it
    assert against_find_median_pixel(oracle, frames, labels, 9) > 0
    count, values = region_quantiles_oracle(np.full((1, 3, 4), 65535, np.uint16), np.zeros((3, 4), np.int32), 2, PERCENTS)
    assert count.tolist() == [[12, 0]] and (values[0, 0] == 0).all() and (values[0, 1] == -1).all()


@pytest.mark.parametrize("n,h,w,k", CASES)
def test_oracle_is_the_compiled_reference_without_65535(ref, n, h, w, k):
    frames, labels = full_range_case(n * 100 + k, n, h, w, k)
    frames[frames == 65535] = 65534
    assert against_find_median_pixel(ref, frames, labels, k) > 0


def test_rank_rounds_half_away_from_zero():
    ties = [(1, 0.5), (2, 0.25), (2, 0.75), (3, 0.5), (5, 0.5), (6, 0.25), (6, 0.75), (7, 0.5)]
    assert [quantile_rank(c, p) for c, p in ties] == [1, 1, 2, 2, 3, 2, 5, 4]
    assert quantile_rank(1, 0.5) != int(np.round(np.float32(1) * np.float32(0.5)))
    assert quantile_rank(100, 0.0) == 0 and quantile_rank(100, 1.0) == 100 and quantile_rank(16777217, 1.0) == 16777216
    frames = np.array([[[10, 20, 30, 40, 50, 60, 70]]], np.uint16)
    for c in (1, 2, 3, 5, 6, 7):
        labels = np.full((1, 7), -1, np.int32)
        labels[0, :c] = 0
        _, values = region_quantiles_oracle(frames, labels, 1, (0.25, 0.5, 0.75))
        assert values[0, 0].tolist() == [10 * quantile_rank(c, p) for p in (0.25, 0.5, 0.75)]


def test_entry_points_are_declared_and_exported(lib):
    dev = open(os.path.join(ROOT, "include", "rir_amd_device.h")).read()
    sp = open(os.path.join(ROOT, "include", "rir_amd_signal_processing.h")).read()
    assert re.search(r"int rir_region_quantiles_device\(const unsigned short \*d_frames, const int \*d_labels, int w, int h, int nframes, "
                     r"int labels_per_frame,\s+int nregions, const float \*percents /\* HOST, npercents floats \*/, int npercents,\s+"
                     r"int \*d_count, int \*d_values, void \*d_work, size_t work_bytes, void \*stream\);", dev)
    assert re.search(r"size_t rir_region_quantiles_workspace_bytes\(int w, int h, int nframes, int labels_per_frame, int nregions, int npercents\);",
                     dev)
    assert re.search(r"int rir_region_quantiles\(const unsigned short \*frames, const int \*labels, int w, int h, int nframes, "
                     r"int labels_per_frame, int nregions,\s+const float \*percents, int npercents, int \*count, int \*values\);", sp)
    for name in ("rir_region_quantiles_device", "rir_region_quantiles_workspace_bytes", "rir_region_quantiles"):
        assert hasattr(lib, name), name
    header = open(os.path.join(B.CSRC, "quantile_kernels.h")).read()
    assert re.search(r"constexpr int QUANTILE_LDS_MAX = \d+;", header)


def frame_bytes(k, q):
    return k * (1040 + 1032 * q)  # B(nregions, npercents), as quantile_kernels.h and rir_amd_device.h document it


def test_workspace_query(lib):
    f = lib.rir_region_quantiles_workspace_bytes
    f.argtypes = [ct.c_int] * 6
    f.restype = ct.c_size_t
    cap = 256 << 20
    for w, h, n, per, k, q in [(640, 512, 10, 0, 16, 1), (640, 512, 1000, 1, 16, 4), (1, 1, 1, 0, 1, 1), (80, 64, 0, 0, 5, 8), (80, 64, 3, 0, 65536, 1),
                               (80, 64, 3, 1, 65536, 8), (640, 512, 100000, 0, 1024, 3)]:
        b = frame_bytes(k, q)
        got = f(w, h, n, per, k, q)
        assert got == b * min(max(n, 1), max(1, cap // b)), (w, h, n, per, k, q)
        assert 0 < got <= cap + b and got % 8 == 0
    for bad in [(0, 5, 1, 0, 1, 1), (5, 0, 1, 0, 1, 1), (5, 5, -1, 0, 1, 1), (5, 5, 1, 2, 1, 1), (5, 5, 1, -1, 1, 1), (5, 5, 1, 0, 0, 1),
                (5, 5, 1, 0, 65537, 1), (5, 5, 1, 0, 1, 0), (5, 5, 1, 0, 1, 9), (65536, 32768, 1, 0, 1, 1)]:
        assert f(*bad) == 0, bad


def test_no_cpu_fallback_without_device(lib):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from librir_amd.low_level.misc import last_error

    frames = np.arange(2 * 3 * 5, dtype=np.uint16).reshape(2, 3, 5)
    labels = np.zeros((3, 5), np.int32)
    pc = np.array([0.5, 1.0], np.float32)
    count, values = np.full((2, 1), 7, np.int32), np.full((2, 1, 2), 7, np.int32)
    lib.rir_region_quantiles.argtypes = [ct.c_void_p, ct.c_void_p] + [ct.c_int] * 5 + [ct.c_void_p, ct.c_int, ct.c_void_p, ct.c_void_p]
    assert lib.rir_region_quantiles(frames.ctypes.data, labels.ctypes.data, 5, 3, 2, 0, 1, pc.ctypes.data, 2, count.ctypes.data,
                                    values.ctypes.data) == -1
    assert "no usable HIP device" in last_error()
    assert (count == 7).all() and (values == 7).all()
    lib.rir_region_quantiles_device.argtypes = ([ct.c_void_p, ct.c_void_p] + [ct.c_int] * 5 + [ct.c_void_p, ct.c_int] + [ct.c_void_p] * 3
                                                + [ct.c_size_t, ct.c_void_p])
    work = np.zeros(frame_bytes(1, 2) // 8 * 2, np.int64)
    assert lib.rir_region_quantiles_device(frames.ctypes.data, labels.ctypes.data, 5, 3, 2, 0, 1, pc.ctypes.data, 2, count.ctypes.data,
                                           values.ctypes.data, work.ctypes.data, work.nbytes, None) == -1
    assert "no usable HIP device" in last_error()
    assert (count == 7).all() and (values == 7).all() and not work.any()
    from librir_amd import signal_processing as S

    with pytest.raises(RuntimeError):
        S.region_quantiles(frames, labels, 0.5, 1)


def test_python_api_exists():
    from librir_amd import device as D
    from librir_amd import signal_processing as S
    from librir_amd.video_io import IRMovie

    assert callable(D.region_quantiles) and callable(S.region_quantiles) and "region_quantiles" in S.__all__
    assert D.RegionQuantiles._fields == ("count", "values")
    assert list(inspect.signature(D.region_quantiles).parameters) == ["frames", "labels", "percents", "nregions"]
    assert list(inspect.signature(S.region_quantiles).parameters) == ["images", "labels", "percents", "nregions"]
    params = inspect.signature(IRMovie.region_quantiles).parameters
    assert list(params)[1:] == ["labels", "percents", "selection", "nregions"]
    assert params["selection"].default == slice(None) and params["nregions"].default is None


@pytest.mark.parametrize("frames_shape,frames_dtype,labels_shape,labels_dtype,percents,nregions,exc", [
    ((2, 4, 5), "uint16", (4, 5), "int64", 0.5, 3, RuntimeError),
    ((2, 4, 5), "int16", (4, 5), "int32", 0.5, 3, RuntimeError),
    ((2, 4, 5), "float32", (4, 5), "int32", 0.5, 3, RuntimeError),
    ((2, 4, 5), "uint16", (5, 4), "int32", 0.5, 3, ValueError),
    ((2, 4, 5), "uint16", (3, 4, 5), "int32", 0.5, 3, ValueError),
    ((4, 5), "uint16", (2, 4, 5), "int32", 0.5, 3, ValueError),
    ((2, 2, 4, 5), "uint16", (4, 5), "int32", 0.5, 3, ValueError),
    ((2, 4, 5), "uint16", (4, 5), "int32", 0.5, 0, ValueError),
    ((2, 4, 5), "uint16", (4, 5), "int32", 0.5, -3, ValueError),
    ((2, 4, 5), "uint16", (4, 5), "int32", 0.5, 65537, ValueError),
    ((2, 4, 5), "uint16", (4, 5), "int32", (), 3, ValueError),
    ((2, 4, 5), "uint16", (4, 5), "int32", (0.1,) * 9, 3, ValueError),
    ((2, 4, 5), "uint16", (4, 5), "int32", ((0.1, 0.2),), 3, ValueError),
    ((2, 4, 5), "uint16", (4, 5), "int32", -0.01, 3, ValueError),
    ((2, 4, 5), "uint16", (4, 5), "int32", (0.5, 1.01), 3, ValueError),
    ((2, 4, 5), "uint16", (4, 5), "int32", (0.5, float("nan")), 3, ValueError),
])
def test_python_checks_raise_without_a_device(frames_shape, frames_dtype, labels_shape, labels_dtype, percents, nregions, exc):
    """CPU tensors: every check comes before any device work"""
    import torch

    from librir_amd import device as D
    from librir_amd import signal_processing as S

    fr = torch.zeros(frames_shape, dtype=getattr(torch, frames_dtype))
    lab = torch.zeros(labels_shape, dtype=getattr(torch, labels_dtype))
    with pytest.raises(exc):
        D.region_quantiles(fr, lab, percents, nregions)
    np_dtype = {"uint16": np.uint16, "int16": np.int16, "float32": np.float32}[frames_dtype]
    with pytest.raises(exc):
        S.region_quantiles(np.zeros(frames_shape, np_dtype), np.zeros(labels_shape, getattr(np, labels_dtype)), percents, nregions)


def test_device_entry_refuses_cpu_tensors():
    import torch

    from librir_amd import device as D

    with pytest.raises(RuntimeError, match="CUDA"):
        D.region_quantiles(torch.zeros((2, 4, 5), dtype=torch.uint16), torch.zeros((4, 5), dtype=torch.int32), (0.5, 0.99), 3)


def test_region_stats_keeps_its_own_limits_and_messages():
    """the shared argument checks still speak for region_stats: 2^24 regions there, 65 536 here"""
    from librir_amd import signal_processing as S

    f, lab = np.zeros((1, 2, 2), np.uint16), np.zeros((2, 2), np.int32)
    with pytest.raises(ValueError, match=r"region_stats: nregions must be in 1\.\.2\^24"):
        S.region_stats(f, lab, 0)
    with pytest.raises(ValueError, match=r"region_quantiles: nregions must be in 1\.\.2\^16"):
        S.region_quantiles(f, lab, 0.5, 65537)


HIPCC_FOUND = os.path.exists(B.HIPCC) or shutil.which(B.HIPCC) is not None


@pytest.mark.skipif(not HIPCC_FOUND, reason="hipcc not found")
def test_quantile_kernels_use_no_scratch_and_no_cmpswap(tmp_path):
    """exact, order-free counting with native 32-bit atomic adds only: no compare-and-swap loop, no private segment"""
    asm = str(tmp_path / "quantile_kernels.s")
    flags = [f for f in B.COMMON if f != "-fPIC"]
    subprocess.check_call([B.HIPCC] + flags + ["-S", "--cuda-device-only", os.path.join(B.CSRC, "quantile_kernels.hip"), "-o", asm],
                          stderr=subprocess.DEVNULL)
    text = open(asm).read()
    assert "cmpswap" not in text.lower()
    for op in ("global_atomic_add", "ds_add_u32"):
        assert op in text, op
    meta = text[text.index("amdhsa.kernels:"):text.index(".end_amdgpu_metadata")]
    kernels = {}
    for block in re.split(r"\n  - ", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            kernels[name.group(1)] = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1))
    assert len([k for k in kernels if "region_quantiles" in k]) == 4, sorted(kernels)
    assert all(v == 0 for v in kernels.values()), kernels
