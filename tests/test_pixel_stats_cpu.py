"""CPU: per-pixel statistics over time - the numpy oracle the GPU tests use agrees with a per-pixel restatement of the contract and with
itself when batches are merged in any order, the entry points are declared and exported and refuse bad arguments, there is no CPU fallback,
the Python API checks its arguments without a device, and the kernels of pixel_kernels.hip use no scratch and no compare-and-swap loop."""
import ctypes as ct
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from librir_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIELDS = ("sum", "sumsq", "min", "max", "argmin", "argmax")
DTYPES = dict(sum=np.int64, sumsq=np.int64, min=np.int32, max=np.int32, argmin=np.int32, argmax=np.int32)
SUMS, EXTREMES = FIELDS[:2], FIELDS[2:]


def pixel_stats_oracle(frames, t0=0):
    """the contract in numpy: per pixel the exact sums and the extremes over time with t0 + the first frame that holds each; no frames: the
    empty state.  -> dict of [h][w] arrays"""
    frames = np.asarray(frames)
    if frames.ndim == 2:
        frames = frames[None]
    n, h, w = frames.shape
    if n == 0:
        return empty_state(h, w)
    v = frames.astype(np.int64)
    return {"sum": v.sum(0), "sumsq": (v * v).sum(0), "min": frames.min(0).astype(np.int32), "max": frames.max(0).astype(np.int32),
            "argmin": (frames.argmin(0) + t0).astype(np.int32), "argmax": (frames.argmax(0) + t0).astype(np.int32)}


def empty_state(h, w):
    return {k: np.full((h, w), 0 if k in SUMS else -1, DTYPES[k]) for k in FIELDS}


def merge_oracle(a, b):
    """the accumulating rule: sums add; the smaller minimum wins and, of equal minima, the lower time index; likewise for the maximum;
    -1 marks the empty state"""
    out = {"sum": a["sum"] + b["sum"], "sumsq": a["sumsq"] + b["sumsq"]}
    for val, arg, better in (("min", "argmin", np.less), ("max", "argmax", np.greater)):
        take = (b[val] >= 0) & ((a[val] < 0) | better(b[val], a[val]) | ((b[val] == a[val]) & (b[arg] < a[arg])))
        out[val] = np.where(take, b[val], a[val])
        out[arg] = np.where(take, b[arg], a[arg])
    return out


def brute_force(frames, t0):
    n, h, w = frames.shape
    res = {k: np.zeros((h, w), np.int64) for k in FIELDS}
    for y in range(h):
        for x in range(w):
            vals = [int(frames[f, y, x]) for f in range(n)]
            lo, hi = min(vals), max(vals)
            res["sum"][y, x] = sum(vals)
            res["sumsq"][y, x] = sum(v * v for v in vals)
            res["min"][y, x], res["max"][y, x] = lo, hi
            res["argmin"][y, x] = t0 + min(f for f in range(n) if vals[f] == lo)
            res["argmax"][y, x] = t0 + min(f for f in range(n) if vals[f] == hi)
    return res


def four_values(seed, n, h, w):
    """0, 21845, 43690, 65535 only: ties everywhere"""
    return np.random.default_rng(seed).integers(0, 4, (n, h, w)).astype(np.uint16) * np.uint16(21845)


CASES = [(0, 1, 1, 1, 5), (1, 2, 3, 5, 1), (2, 9, 4, 7, 1000), (3, 17, 5, 3, 7), (4, 6, 1, 9, 2147483000)]


@pytest.mark.parametrize("seed,n,h,w,t0", CASES)
def test_oracle_matches_the_definition_pixel_by_pixel(seed, n, h, w, t0):
    frames = four_values(seed, n, h, w)
    got = pixel_stats_oracle(frames, t0)
    exp = brute_force(frames, t0)
    for k in FIELDS:
        assert got[k].dtype == DTYPES[k] and got[k].shape == (h, w)
        assert np.array_equal(got[k], exp[k]), k


@pytest.mark.parametrize("seed,n,h,w,t0", CASES)
def test_batches_merged_in_any_order_equal_the_whole(seed, n, h, w, t0):
    frames = four_values(seed, n, h, w)
    whole = pixel_stats_oracle(frames, t0)
    rng = np.random.default_rng(seed)
    for _ in range(4):
        cuts = sorted(set(rng.integers(0, n + 1, 3).tolist()) | {0, n})
        batches = [(a, b) for a, b in zip(cuts, cuts[1:])]
        rng.shuffle(batches)
        acc = empty_state(h, w)
        for a, b in batches:
            acc = merge_oracle(acc, pixel_stats_oracle(frames[a:b], t0 + a))
        for k in FIELDS:
            assert np.array_equal(acc[k], whole[k]), (k, batches)
    assert all(np.array_equal(merge_oracle(whole, empty_state(h, w))[k], whole[k]) for k in FIELDS)


def test_entry_points_are_declared_and_exported(lib):
    dev = open(os.path.join(ROOT, "include", "rir_amd_device.h")).read()
    sp = open(os.path.join(ROOT, "include", "rir_amd_signal_processing.h")).read()
    assert re.search(r"int\s+rir_pixel_stats_device\(const unsigned short \*d_frames, int w, int h, int nframes, int t0, int accumulate,\s+"
                     r"long long \*d_sum, long long \*d_sumsq, int \*d_min, int \*d_max, int \*d_argmin, int \*d_argmax,\s+"
                     r"void \*d_work, size_t work_bytes, void \*stream\);", dev)
    assert re.search(r"size_t\s+rir_pixel_stats_workspace_bytes\(int w, int h, int nframes\);", dev)
    assert re.search(r"int\s+rir_pixel_stats\(const unsigned short \*frames, int w, int h, int nframes, long long \*sum, long long \*sumsq, "
                     r"int \*min, int \*max,\s+int \*argmin, int \*argmax\);", sp)
    assert "65535^2 * 2^31 < 2^63" in dev  # the overflow bound is stated
    for name in ("rir_pixel_stats_device", "rir_pixel_stats_workspace_bytes", "rir_pixel_stats"):
        assert hasattr(lib, name), name


def test_workspace_query(lib):
    f = lib.rir_pixel_stats_workspace_bytes
    f.argtypes = [ct.c_int] * 3
    f.restype = ct.c_size_t
    for bad in [(0, 5, 1), (5, 0, 1), (-1, 5, 1), (5, 5, -1), (65536, 32768, 1), (46341, 46341, 1)]:
        assert f(*bad) == 0, bad
    for good in [(1, 1, 0), (1, 1, 1), (640, 512, 1000), (5, 3, 70001), (1, 1, 2147483647), (65535, 32768, 1), (1024, 768, 3)]:
        assert f(*good) > 0, good
    assert f(1, 1, 70001) >= f(1, 1, 7)  # a long thin stack is cut along time: partials for every slab
    assert f(1024, 512, 65536) == 8 and f(1024, 512, 65537) == 2 * 20 * 1024 * 512  # a slab holds at most 65 536 frames: 16 bits of index


PLAN_SHAPES = [(1, 1), (5, 3), (511, 1), (512, 1), (513, 1), (80, 64), (640, 512)]  # w * h = 1, 15, 511, 512, 513, 5120, 327680
PLAN_LENGTHS = [1, 255, 256, 257, 5000, 65536, 65537, 70001]


@pytest.mark.parametrize("w,h", PLAN_SHAPES)
def test_workspace_follows_the_time_slab_plan(lib, w, h):
    """the cut along time in closed form: tiles of 512 pixels, slabs added while the grid stays within 1 024 workgroups, 256 to 65 536
    frames a slab; 20 bytes per (slab, pixel) when there is more than one slab, else 8"""
    f = lib.rir_pixel_stats_workspace_bytes
    f.argtypes = [ct.c_int] * 3
    f.restype = ct.c_size_t
    npx = w * h
    for n in PLAN_LENGTHS:
        tiles = (npx + 511) // 512
        want = max(1, 1024 // tiles)
        per_slab = min(max((n + want - 1) // want, 256), 65536)
        slabs = max(1, (n + per_slab - 1) // per_slab)
        assert f(w, h, n) == (slabs * npx * 20 if slabs > 1 else 8), (w, h, n, slabs, per_slab)


DEV_ARGS = [ct.c_void_p] + [ct.c_int] * 5 + [ct.c_void_p] * 7 + [ct.c_size_t, ct.c_void_p]
HOST_ARGS = [ct.c_void_p] + [ct.c_int] * 3 + [ct.c_void_p] * 6


def test_no_cpu_fallback_without_device(lib):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from librir_amd.low_level.misc import last_error

    frames = np.arange(2 * 3 * 5, dtype=np.uint16).reshape(2, 3, 5)
    outs = [np.zeros((3, 5), DTYPES[k]) for k in FIELDS]
    lib.rir_pixel_stats.argtypes = HOST_ARGS
    assert lib.rir_pixel_stats(frames.ctypes.data, 5, 3, 2, *(o.ctypes.data for o in outs)) == -1
    assert "no usable HIP device" in last_error()
    assert not any(o.any() for o in outs)
    lib.rir_pixel_stats_device.argtypes = DEV_ARGS
    work = np.zeros(64, np.int64)
    assert lib.rir_pixel_stats_device(frames.ctypes.data, 5, 3, 2, 0, 0, *(o.ctypes.data for o in outs), work.ctypes.data, work.nbytes, None) == -1
    assert "no usable HIP device" in last_error()
    assert not any(o.any() for o in outs)
    from librir_amd import signal_processing as S

    with pytest.raises(RuntimeError):
        S.pixel_stats(frames)


def test_python_api_exists():
    import inspect

    from librir_amd import device as D
    from librir_amd import signal_processing as S
    from librir_amd.video_io import IRMovie

    assert callable(D.pixel_stats) and callable(S.pixel_stats) and "pixel_stats" in S.__all__
    assert D.PixelStats._fields == FIELDS and callable(D.PixelStats.mean) and callable(D.PixelStats.std)
    assert list(inspect.signature(D.pixel_stats).parameters) == ["frames", "sums", "extremes", "t0"]
    assert list(inspect.signature(S.pixel_stats).parameters) == ["images", "sums", "extremes"]
    assert list(inspect.signature(D.PixelStatsAccumulator).parameters)[:2] == ["sums", "extremes"]
    assert list(inspect.signature(D.PixelStatsAccumulator.push).parameters) == ["self", "frames", "t0"]
    for name in ("push", "result", "reset", "merge"):
        assert callable(getattr(D.PixelStatsAccumulator, name))
    assert list(inspect.signature(IRMovie.pixel_stats).parameters)[1:] == ["selection", "sums", "extremes"]
    ps = D.PixelStats(1, 2, None, None, None, None, count=7)
    assert ps.count == 7 and ps.sum == 1 and ps.min is None and tuple(ps) == (1, 2, None, None, None, None)


def test_mean_and_std_from_exact_sums():
    import torch

    from librir_amd import device as D

    rng = np.random.default_rng(9)
    frames = four_values(9, 11, 6, 7)
    frames[:, ::2, ::3] = rng.integers(0, 65536, frames[:, ::2, ::3].shape)
    frames[:, 5, 6] = 65535  # a constant pixel: std 0
    o = pixel_stats_oracle(frames)
    ps = D.PixelStats(*(o[k] for k in FIELDS), count=11)
    mean, std = ps.mean(), ps.std()
    assert mean.dtype == np.float64 and std.dtype == np.float64 and mean.shape == (6, 7)
    ref = frames.astype(np.float64)
    for y in range(6):
        for x in range(7):
            assert mean[y, x] == pytest.approx(ref[:, y, x].mean(), rel=1e-12)
            assert std[y, x] == pytest.approx(ref[:, y, x].std(), rel=1e-9, abs=1e-6)
    pt = D.PixelStats(*(torch.from_numpy(o[k]) for k in FIELDS), count=11)
    assert pt.mean().dtype == torch.float64 and pt.std().dtype == torch.float64
    for y in range(6):
        for x in range(7):
            assert float(pt.mean()[y, x]) == pytest.approx(ref[:, y, x].mean(), rel=1e-12)
            assert float(pt.std()[y, x]) == pytest.approx(ref[:, y, x].std(), rel=1e-9, abs=1e-6)
    e = empty_state(2, 3)
    for none in (D.PixelStats(*(e[k] for k in FIELDS)), D.PixelStats(*(torch.from_numpy(e[k]) for k in FIELDS))):
        assert none.count == 0 and np.isnan(np.asarray(none.mean())).all() and np.isnan(np.asarray(none.std())).all()


@pytest.mark.parametrize("shape,dtype,kwargs,exc", [
    ((2, 4, 5), "int16", {}, RuntimeError),
    ((2, 4, 5), "float32", {}, RuntimeError),
    ((2, 4, 5), "int32", {}, RuntimeError),
    ((5,), "uint16", {}, ValueError),
    ((2, 2, 4, 5), "uint16", {}, ValueError),
    ((2, 0, 5), "uint16", {}, ValueError),
    ((2, 4, 5), "uint16", dict(sums=False, extremes=False), ValueError),
    ((2, 4, 5), "uint16", dict(t0=-1), ValueError),
    ((2, 4, 5), "uint16", dict(t0=(1 << 31) - 2), ValueError),
    ((2, 4, 5), "uint16", dict(t0=1.5), ValueError),
])
def test_python_checks_raise_without_a_device(shape, dtype, kwargs, exc):
    """CPU tensors: every check comes before any device work"""
    import torch

    from librir_amd import device as D
    from librir_amd import signal_processing as S

    fr = torch.zeros(shape, dtype=getattr(torch, dtype))
    with pytest.raises(exc):
        D.pixel_stats(fr, **kwargs)
    if "t0" in kwargs:
        with pytest.raises(exc):
            D.PixelStatsAccumulator().push(fr, kwargs["t0"])
    elif kwargs:
        with pytest.raises(exc):
            D.PixelStatsAccumulator(**kwargs)
    else:
        with pytest.raises(exc):
            D.PixelStatsAccumulator().push(fr)
    if "t0" not in kwargs:
        with pytest.raises(exc):
            S.pixel_stats(np.zeros(shape, getattr(np, dtype)), **kwargs)


def test_t0_at_the_int32_limit_is_accepted_by_the_checks():
    from librir_amd.signal_processing.rir_signal_processing import _pixel_stats_args

    assert _pixel_stats_args((2, 4, 5), True, False, (1 << 31) - 3) == (2, 4, 5)
    assert _pixel_stats_args((4, 5)) == (1, 4, 5)
    with pytest.raises(ValueError):
        _pixel_stats_args((2, 4, 5), True, True, (1 << 31) - 2)


def test_device_entry_refuses_cpu_tensors():
    import torch

    from librir_amd import device as D

    with pytest.raises(RuntimeError, match="CUDA"):
        D.pixel_stats(torch.zeros((2, 4, 5), dtype=torch.uint16))
    with pytest.raises(RuntimeError, match="CUDA"):
        D.PixelStatsAccumulator().push(torch.zeros((2, 4, 5), dtype=torch.uint16))


HIPCC_FOUND = os.path.exists(B.HIPCC) or shutil.which(B.HIPCC) is not None


@pytest.mark.skipif(not HIPCC_FOUND, reason="hipcc not found")
def test_pixel_kernels_use_no_scratch_and_no_cmpswap(tmp_path):
    """exact combination in registers, LDS and a fixed order: no private segment, no compare-and-swap loop"""
    asm = str(tmp_path / "pixel_kernels.s")
    flags = [f for f in B.COMMON if f != "-fPIC"]
    subprocess.check_call([B.HIPCC] + flags + ["-S", "--cuda-device-only", os.path.join(B.CSRC, "pixel_kernels.hip"), "-o", asm],
                          stderr=subprocess.DEVNULL)
    text = open(asm).read()
    assert "cmpswap" not in text.lower()
    meta = text[text.index("amdhsa.kernels:"):text.index(".end_amdgpu_metadata")]
    kernels = {}
    for block in re.split(r"\n  - ", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            kernels[name.group(1)] = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1))
    assert len([k for k in kernels if "pixel_stats" in k]) == 15, sorted(kernels)  # 3 forms x (4 slab kernels + 1 fold)
    assert all(v == 0 for v in kernels.values()), kernels
