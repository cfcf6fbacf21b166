"""CPU: per-region statistics - the numpy oracle the GPU tests use agrees with a per-pixel restatement of the contract, the entry points are
declared and exported and refuse bad arguments, there is no CPU fallback, the Python API checks its arguments without a device, and the kernels
of region_kernels.hip use no scratch and no compare-and-swap loop."""
import ctypes as ct
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from librir_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def region_stats_oracle(frames, labels, nregions):
    """the contract with int64 numpy scatter operations: per (frame, region) count, sum, sumsq, min, max and the lowest flat index of each;
    labels outside [0, nregions) ignored; empty regions 0, 0, 0, -1, -1, -1, -1.  -> dict of [n][nregions] arrays"""
    frames = np.asarray(frames)
    if frames.ndim == 2:
        frames = frames[None]
    n, h, w = frames.shape
    lab = np.broadcast_to(np.asarray(labels, np.int64), (n, h, w)).reshape(n, -1)
    v = frames.reshape(n, -1).astype(np.int64)
    idx = np.arange(h * w, dtype=np.int64)
    keep = (lab >= 0) & (lab < nregions)
    f = np.broadcast_to(np.arange(n, dtype=np.int64)[:, None], lab.shape)
    cell = (f * nregions + lab)[keep]
    vk, ik = v[keep], np.broadcast_to(idx, lab.shape)[keep]
    cells = n * nregions
    count = np.zeros(cells, np.int64)
    np.add.at(count, cell, 1)
    s = np.zeros(cells, np.int64)
    np.add.at(s, cell, vk)
    sq = np.zeros(cells, np.int64)
    np.add.at(sq, cell, vk * vk)
    # packed keys: value << 32 | index for the minimum (np.minimum), value << 32 | (2^32 - 1 - index) for the maximum (np.maximum)
    kmin = np.full(cells, np.iinfo(np.int64).max, np.int64)
    np.minimum.at(kmin, cell, vk << 32 | ik)
    kmax = np.full(cells, -1, np.int64)
    np.maximum.at(kmax, cell, vk << 32 | (0xFFFFFFFF - ik))
    empty = count == 0
    out = {
        "count": count.astype(np.int32),
        "sum": s,
        "sumsq": sq,
        "min": np.where(empty, -1, kmin >> 32).astype(np.int32),
        "argmin": np.where(empty, -1, kmin & 0xFFFFFFFF).astype(np.int32),
        "max": np.where(empty, -1, kmax >> 32).astype(np.int32),
        "argmax": np.where(empty, -1, 0xFFFFFFFF - (kmax & 0xFFFFFFFF)).astype(np.int32),
    }
    return {k: a.reshape(n, nregions) for k, a in out.items()}


FIELDS = ("count", "sum", "sumsq", "min", "max", "argmin", "argmax")
DTYPES = dict(count=np.int32, sum=np.int64, sumsq=np.int64, min=np.int32, max=np.int32, argmin=np.int32, argmax=np.int32)


def brute_force(frames, labels, nregions):
    n, h, w = frames.shape
    res = {k: np.zeros((n, nregions), np.int64) for k in FIELDS}
    for f in range(n):
        for r in range(nregions):
            px = [(int(frames[f, y, x]), y * w + x) for y in range(h) for x in range(w)
                  if (labels[f, y, x] if labels.ndim == 3 else labels[y, x]) == r]
            if not px:
                for k in ("min", "max", "argmin", "argmax"):
                    res[k][f, r] = -1
                continue
            vals = [p[0] for p in px]
            lo, hi = min(vals), max(vals)
            res["count"][f, r] = len(px)
            res["sum"][f, r] = sum(vals)
            res["sumsq"][f, r] = sum(x * x for x in vals)
            res["min"][f, r], res["max"][f, r] = lo, hi
            res["argmin"][f, r] = min(i for x, i in px if x == lo)
            res["argmax"][f, r] = min(i for x, i in px if x == hi)
    return res


def random_case(seed, n, h, w, nregions, per_frame):
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 4, (n, h, w)).astype(np.uint16) * np.uint16(21845)  # 0, 21845, 43690, 65535: many ties
    frames.reshape(n, -1)[:, ::5] = rng.integers(0, 65536, frames.reshape(n, -1)[:, ::5].shape)
    shape = (n, h, w) if per_frame else (h, w)
    labels = rng.integers(-2, nregions + 2, shape).astype(np.int32)  # below 0 and >= nregions: ignored; some regions left empty
    return frames, labels


@pytest.mark.parametrize("seed,n,h,w,nregions,per_frame", [(0, 1, 1, 1, 1, 0), (1, 2, 3, 5, 1, 0), (2, 3, 4, 7, 6, 0), (3, 3, 5, 3, 9, 1),
                                                           (4, 1, 6, 6, 40, 0), (5, 4, 2, 9, 3, 1), (6, 2, 7, 1, 5, 1)])
def test_oracle_matches_the_definition_pixel_by_pixel(seed, n, h, w, nregions, per_frame):
    frames, labels = random_case(seed, n, h, w, nregions, per_frame)
    got = region_stats_oracle(frames, labels, nregions)
    exp = brute_force(frames, labels, nregions)
    for k in FIELDS:
        assert got[k].dtype == DTYPES[k] and got[k].shape == (n, nregions)
        assert np.array_equal(got[k], exp[k]), k
    if nregions > 4:
        assert (got["count"] == 0).any() or nregions == 6  # empty regions are covered


def test_oracle_extremes():
    """values 0 and 65535 everywhere, ties at both ends fall to the lowest index, one region over a whole frame"""
    frames = np.full((2, 4, 5), 65535, np.uint16)
    frames[1] = 0
    labels = np.zeros((4, 5), np.int32)
    labels[0, 0] = -1
    o = region_stats_oracle(frames, labels, 1)
    assert o["count"].tolist() == [[19], [19]] and o["sum"][0, 0] == 19 * 65535 and o["sumsq"][0, 0] == 19 * 65535 ** 2
    assert o["argmin"].tolist() == [[1], [1]] and o["argmax"].tolist() == [[1], [1]]
    assert o["min"].tolist() == [[65535], [0]] and o["max"].tolist() == [[65535], [0]]


def test_entry_points_are_declared_and_exported(lib):
    dev = open(os.path.join(ROOT, "include", "rir_amd_device.h")).read()
    sp = open(os.path.join(ROOT, "include", "rir_amd_signal_processing.h")).read()
    assert re.search(r"int rir_region_stats_device\(const unsigned short \*d_frames, const int \*d_labels, int w, int h, int nframes, "
                     r"int labels_per_frame, int nregions,\s+int \*d_count, long long \*d_sum, long long \*d_sumsq, int \*d_min, int \*d_max, "
                     r"int \*d_argmin, int \*d_argmax,\s+void \*d_work, size_t work_bytes, void \*stream\);", dev)
    assert re.search(r"size_t rir_region_stats_workspace_bytes\(int w, int h, int nframes, int labels_per_frame, int nregions\);", dev)
    assert re.search(r"int rir_region_stats\(const unsigned short \*frames, const int \*labels, int w, int h, int nframes, int labels_per_frame, "
                     r"int nregions,\s+int \*count, long long \*sum, long long \*sumsq, int \*min, int \*max, int \*argmin, int \*argmax\);", sp)
    for name in ("rir_region_stats_device", "rir_region_stats_workspace_bytes", "rir_region_stats"):
        assert hasattr(lib, name), name


def test_workspace_query(lib):
    f = lib.rir_region_stats_workspace_bytes
    f.argtypes = [ct.c_int] * 5
    f.restype = ct.c_size_t
    assert f(640, 512, 10, 0, 16) == 10 * 16 * 32
    assert f(1, 1, 1, 1, 1 << 24) == 32 << 24
    for bad in [(0, 5, 1, 0, 1), (5, 0, 1, 0, 1), (5, 5, -1, 0, 1), (5, 5, 1, 2, 1), (5, 5, 1, 0, 0), (5, 5, 1, 0, (1 << 24) + 1), (65536, 32768, 1, 0, 1)]:
        assert f(*bad) == 0, bad


def test_no_cpu_fallback_without_device(lib):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from librir_amd.low_level.misc import last_error

    frames = np.arange(2 * 3 * 5, dtype=np.uint16).reshape(2, 3, 5)
    labels = np.zeros((3, 5), np.int32)
    outs = [np.zeros((2, 1), dt) for dt in (np.int32, np.int64, np.int64, np.int32, np.int32, np.int32, np.int32)]
    lib.rir_region_stats.argtypes = [ct.c_void_p, ct.c_void_p] + [ct.c_int] * 5 + [ct.c_void_p] * 7
    assert lib.rir_region_stats(frames.ctypes.data, labels.ctypes.data, 5, 3, 2, 0, 1, *(o.ctypes.data for o in outs)) == -1
    assert "no usable HIP device" in last_error()
    assert not any(o.any() for o in outs)
    lib.rir_region_stats_device.argtypes = [ct.c_void_p, ct.c_void_p] + [ct.c_int] * 5 + [ct.c_void_p] * 8 + [ct.c_size_t, ct.c_void_p]
    work = np.zeros(64, np.int64)
    assert lib.rir_region_stats_device(frames.ctypes.data, labels.ctypes.data, 5, 3, 2, 0, 1, *(o.ctypes.data for o in outs), work.ctypes.data,
                                       work.nbytes, None) == -1
    assert "no usable HIP device" in last_error()
    assert not any(o.any() for o in outs)
    from librir_amd import signal_processing as S

    with pytest.raises(RuntimeError):
        S.region_stats(frames, labels, 1)


def test_python_api_exists():
    import inspect

    from librir_amd import device as D
    from librir_amd import signal_processing as S
    from librir_amd.video_io import IRMovie

    assert callable(D.region_stats) and callable(S.region_stats) and "region_stats" in S.__all__
    assert D.RegionStats._fields == FIELDS and callable(D.RegionStats.mean) and callable(D.RegionStats.std)
    params = inspect.signature(IRMovie.region_stats).parameters
    assert list(params)[1:] == ["labels", "selection", "nregions"] and IRMovie._STATS_PIECE_BYTES == 64 << 20


def test_mean_and_std_from_exact_sums():
    from librir_amd import device as D

    frames, labels = random_case(9, 3, 6, 7, 5, 0)
    o = region_stats_oracle(frames, labels, 5)
    rs = D.RegionStats(*(o[k] for k in FIELDS))
    mean, std = rs.mean(), rs.std()
    assert mean.dtype == np.float64 and std.dtype == np.float64
    for f in range(3):
        for r in range(5):
            px = frames[f][labels == r].astype(np.float64)
            if px.size:
                assert mean[f, r] == pytest.approx(px.mean(), rel=1e-12) and std[f, r] == pytest.approx(px.std(), rel=1e-9, abs=1e-6)
            else:
                assert np.isnan(mean[f, r]) and np.isnan(std[f, r])
    import torch

    rt = D.RegionStats(*(torch.from_numpy(o[k]) for k in FIELDS))
    assert np.array_equal(rt.mean().numpy(), mean, equal_nan=True) and np.allclose(rt.std().numpy(), std, equal_nan=True)
    assert rt.mean().dtype == torch.float64 and rt.std().dtype == torch.float64


@pytest.mark.parametrize("frames_shape,frames_dtype,labels_shape,labels_dtype,nregions,exc", [
    ((2, 4, 5), "uint16", (4, 5), "int64", 3, RuntimeError),
    ((2, 4, 5), "int16", (4, 5), "int32", 3, RuntimeError),
    ((2, 4, 5), "float32", (4, 5), "int32", 3, RuntimeError),
    ((2, 4, 5), "uint16", (5, 4), "int32", 3, ValueError),
    ((2, 4, 5), "uint16", (3, 4, 5), "int32", 3, ValueError),
    ((2, 4, 5), "uint16", (2, 4, 5, 1), "int32", 3, ValueError),
    ((4, 5), "uint16", (2, 4, 5), "int32", 3, ValueError),
    ((2, 2, 4, 5), "uint16", (4, 5), "int32", 3, ValueError),
    ((2, 4, 5), "uint16", (4, 5), "int32", 0, ValueError),
    ((2, 4, 5), "uint16", (4, 5), "int32", -3, ValueError),
    ((2, 4, 5), "uint16", (4, 5), "int32", (1 << 24) + 1, ValueError),
])
def test_python_checks_raise_without_a_device(frames_shape, frames_dtype, labels_shape, labels_dtype, nregions, exc):
    """CPU tensors: every check comes before any device work"""
    import torch

    from librir_amd import device as D
    from librir_amd import signal_processing as S

    fr = torch.zeros(frames_shape, dtype=getattr(torch, frames_dtype))
    lab = torch.zeros(labels_shape, dtype=getattr(torch, labels_dtype))
    with pytest.raises(exc):
        D.region_stats(fr, lab, nregions)
    np_dtype = {"uint16": np.uint16, "int16": np.int16, "float32": np.float32}[frames_dtype]
    with pytest.raises(exc):
        S.region_stats(np.zeros(frames_shape, np_dtype), np.zeros(labels_shape, getattr(np, labels_dtype)), nregions)


def test_device_entry_refuses_cpu_tensors():
    import torch

    from librir_amd import device as D

    with pytest.raises(RuntimeError, match="CUDA"):
        D.region_stats(torch.zeros((2, 4, 5), dtype=torch.uint16), torch.zeros((4, 5), dtype=torch.int32), 3)


HIPCC_FOUND = os.path.exists(B.HIPCC) or shutil.which(B.HIPCC) is not None


@pytest.mark.skipif(not HIPCC_FOUND, reason="hipcc not found")
def test_region_kernels_use_no_scratch_and_no_cmpswap(tmp_path):
    """exact, order-free combination with native atomics only: no compare-and-swap loop, no private segment"""
    asm = str(tmp_path / "region_kernels.s")
    flags = [f for f in B.COMMON if f != "-fPIC"]
    subprocess.check_call([B.HIPCC] + flags + ["-S", "--cuda-device-only", os.path.join(B.CSRC, "region_kernels.hip"), "-o", asm],
                          stderr=subprocess.DEVNULL)
    text = open(asm).read()
    assert "cmpswap" not in text.lower()
    for op in ("global_atomic_add_x2", "global_atomic_umax_x2", "ds_add_u64", "ds_max_u64"):
        assert op in text, op
    meta = text[text.index("amdhsa.kernels:"):text.index(".end_amdgpu_metadata")]
    kernels = {}
    for block in re.split(r"\n  - ", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            kernels[name.group(1)] = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1))
    assert len([k for k in kernels if "region_stats" in k]) == 4, sorted(kernels)
    assert all(v == 0 for v in kernels.values()), kernels
