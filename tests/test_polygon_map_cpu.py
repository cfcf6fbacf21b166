"""CPU: polygon label maps - the numpy oracle the GPU tests use (polygon_cases.py, a row-local restatement of the reference's scanline fill)
equals the reference's own maps on every stored case (tests/golden/polygon_maps.npz, made by make_polygon_golden.py); the entry points are
declared and exported and refuse bad arguments, there is no CPU fallback, the Python API packs and checks its arguments without a device,
and the kernels of polygon_kernels.hip use no scratch."""
import ctypes as ct
import hashlib
import inspect
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import polygon_cases as PC
from librir_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = PC.cases()


@pytest.fixture(scope="module")
def stored():
    with open(os.path.join(GOLDEN, "polygon_maps_sha256.json")) as f:
        return np.load(os.path.join(GOLDEN, "polygon_maps.npz")), json.load(f)


def test_every_case_is_stored(stored):
    arrays, hashes = stored
    assert sorted(list(arrays.files) + list(hashes)) == sorted(CASES)
    assert all(name.endswith("_big") == (CASES[name]["shape"] == PC.BIG_SHAPE) for name in CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_equals_the_reference(stored, name):
    arrays, hashes = stored
    got = PC.oracle(CASES[name])
    assert got.dtype == np.int32 and got.shape == (PC.n_maps(CASES[name]),) + CASES[name]["shape"]
    if name.endswith("_big"):
        assert hashlib.sha256(got.tobytes()).hexdigest() == hashes[name]
    else:
        assert np.array_equal(got, arrays[name]), np.argwhere(got != arrays[name])[:5]


def test_degenerate_polygons_cover_what_the_reference_covers(stored):
    arrays, _ = stored
    for name, (_, pixels) in PC.DEGENERATES.items():
        assert int((arrays["degenerate_" + name] != 0).sum()) == pixels, name
    flat = arrays["degenerate_flat_to_column_0"][0]
    assert flat[3, 0] == 1 and flat.sum() == 1


def test_tie_triangle_row_starts_where_separate_rounding_puts_it(stored):
    """row 1: 7 + (1 / 10) * -45 rounds to 2.5 -> 3; a fused multiply-add gives 2.4999999999999996 -> 2"""
    row = stored[0]["tie_triangle"][0][1]
    assert np.flatnonzero(row)[0] == 3
    assert 7.0 + (1.0 / 10.0) * -45.0 == 2.5


def test_cases_cover_what_they_claim():
    shapes = {c["shape"] for c in CASES.values()}
    assert set(PC.SMALL_SHAPES + [PC.BIG_SHAPE]) <= shapes
    counts = {len(p) for c in CASES.values() if not c["per_map"] for p in c["sets"]}
    assert {0, 1, 2, 3, 64, 65, 200} <= counts
    assert {1, 3, 70} <= {PC.n_maps(c) for c in CASES.values() if c["shifts"] is not None and not c["per_map"]}
    assert {1, 3, 70} <= {PC.n_maps(c) for c in CASES.values() if c["per_map"]}
    assert any(c["per_map"] and c["shifts"] is not None for c in CASES.values())
    for name in ("nan", "inf", "1e30"):
        got = PC.oracle(CASES["out_of_range_" + name])[0]
        assert set(np.unique(got)) == {-1, 0, 2}, name  # polygons 1, 3 and 4 hold the bad vertex


def test_entry_points_are_declared_and_exported(lib):
    dev = open(os.path.join(ROOT, "include", "rir_amd_device.h")).read()
    sp = open(os.path.join(ROOT, "include", "rir_amd_signal_processing.h")).read()
    assert re.search(r"int rir_polygon_map_device\(const double \*d_xy, const int \*d_npts, const int \*d_values, int npoly, int max_pts, int nmaps, "
                     r"int sets_per_map,\s+const double \*d_shifts, int w, int h, int background, int \*d_dst, void \*d_work, size_t work_bytes, "
                     r"void \*stream\);", dev)
    assert re.search(r"size_t rir_polygon_map_workspace_bytes\(int w, int h, int nmaps, int npoly, int max_pts\);", dev)
    assert re.search(r"int rir_polygon_map\(const double \*xy, const int \*npts, const int \*values, int npoly, int max_pts, int nmaps, "
                     r"int sets_per_map,\s+const double \*shifts, int w, int h, int background, int \*dst\);", sp)
    assert "2^24" in dev[dev.index("Polygon regions of interest"):dev.index("int rir_polygon_map_device")]  # the deviation is documented
    for name in ("rir_polygon_map_device", "rir_polygon_map_workspace_bytes", "rir_polygon_map"):
        assert hasattr(lib, name), name
    assert not hasattr(lib, "draw_polygon")  # the geometry library stays the reference's


def test_workspace_query(lib):
    f = lib.rir_polygon_map_workspace_bytes
    f.argtypes = [ct.c_int] * 5
    f.restype = ct.c_size_t
    assert f(640, 512, 1000, 16, 8) == 1000 * 16 * (5 + 2 * 8) * 4 + 8
    assert f(640, 512, 3, 3, 4) == 3 * (3 * 13 + 1) * 4 + 8  # an odd number of ints per map is rounded up: 8-byte aligned maps
    assert f(5, 5, 0, 7, 3) == 8 and f(5, 5, 4, 0, 1) == 8  # no map, no polygon: not a refusal
    assert f(65536, 32767, 1, 4096, 1024) == 4096 * (5 + 2048) * 4 + 8  # w * h = 0x7FFF0000
    for bad in [(0, 5, 1, 1, 1), (5, 0, 1, 1, 1), (5, 5, -1, 1, 1), (5, 5, 1, -1, 1), (5, 5, 1, 1, 0), (5, 5, 1, 1, 1025), (5, 5, 1, 65537, 1),
                (65536, 32768, 1, 1, 1)]:
        assert f(*bad) == 0, bad


def _raw(lib):
    lib.rir_polygon_map_device.argtypes = [ct.c_void_p] * 3 + [ct.c_int] * 4 + [ct.c_void_p] + [ct.c_int] * 3 + [ct.c_void_p, ct.c_void_p, ct.c_size_t,
                                                                                                           ct.c_void_p]
    lib.rir_polygon_map.argtypes = [ct.c_void_p] * 3 + [ct.c_int] * 4 + [ct.c_void_p] + [ct.c_int] * 3 + [ct.c_void_p]
    return lib.rir_polygon_map_device, lib.rir_polygon_map


# Bad arguments get -1 as well, but without a device every call is refused before its arguments are looked at, so that is checked where
# there is one: tests/test_gpu_polygon_map.py::test_refused_arguments.  What can be told apart here is the workspace query's 0 (above).
def test_no_cpu_fallback_without_device(lib):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from librir_amd import signal_processing as S
    from librir_amd.low_level.misc import last_error

    dev_fn, host_fn = _raw(lib)
    xy = np.array([[[1, 1], [4, 1], [2, 3]]], np.float64)
    npts = np.array([3], np.int32)
    dst = np.full((1, 5, 6), 77, np.int32)
    work = np.zeros(64, np.int64)
    assert host_fn(xy.ctypes.data, npts.ctypes.data, None, 1, 3, 1, 0, None, 6, 5, -1, dst.ctypes.data) == -1
    assert "no usable HIP device" in last_error()
    assert dev_fn(xy.ctypes.data, npts.ctypes.data, None, 1, 3, 1, 0, None, 6, 5, -1, dst.ctypes.data, work.ctypes.data, work.nbytes, None) == -1
    assert "no usable HIP device" in last_error()
    assert (dst == 77).all()  # never a host result
    with pytest.raises(RuntimeError, match="polygon_map"):
        S.polygon_map([[(1, 1), (4, 1), (2, 3)]], (5, 6))


def test_python_api_exists():
    from librir_amd import device as D
    from librir_amd import signal_processing as S
    from librir_amd.video_io import IRMovie

    for fn in (D.polygon_map, S.polygon_map):
        params = inspect.signature(fn).parameters
        assert list(params) == ["polygons", "shape", "values", "background", "shifts", "out"]
        assert [params[k].default for k in list(params)[2:]] == [None, -1, None, None]
    assert "polygon_map" in S.__all__
    params = inspect.signature(IRMovie.polygon_stats).parameters
    assert list(params)[1:] == ["polygons", "selection", "shifts", "values"]
    assert params["selection"].default == slice(None) and params["shifts"].default is None and params["values"].default is None
    from librir_amd import low_level

    assert low_level._geometry is None  # geometry stays what it was (tests/test_host_io.py)
    assert not hasattr(D, "draw_polygon") and not hasattr(S, "draw_polygon")


def test_packing_needs_no_device():
    from librir_amd.device import _polygon_map_args as args

    tri, quad = [(1, 1), (4, 1), (2, 3)], np.array([(0, 0), (3, 0), (3, 3), (0, 3.5)])
    a = args([tri, quad, [], [(2, 2)]], (5, 6), values=[4, 4, 1, 0])
    assert a.xy.shape == (4, 4, 2) and a.xy.dtype == np.float64 and a.npts.tolist() == [3, 4, 0, 1] and a.npts.dtype == np.int32
    assert np.array_equal(a.xy[0, :3], tri) and not a.xy[0, 3:].any() and np.array_equal(a.xy[1], quad)
    assert (a.nmaps, a.per_map, a.npoly, a.max_pts, a.h, a.w, a.out_shape) == (1, 0, 4, 4, 5, 6, (5, 6))
    assert a.values.dtype == np.int32 and a.values.tolist() == [4, 4, 1, 0] and a.shifts is None
    a = args([tri], (5, 6), shifts=[(0, 0), (1.5, -2)])
    assert (a.nmaps, a.per_map, a.out_shape) == (2, 0, (2, 5, 6)) and a.shifts.dtype == np.float64 and a.shifts.shape == (2, 2)
    a = args([[tri, quad], [quad]], (5, 6))  # one set per map; the shorter set is filled up with a polygon of no point
    assert a.xy.shape == (2, 2, 4, 2) and a.npts.tolist() == [[3, 4], [4, 0]] and (a.nmaps, a.per_map, a.out_shape) == (2, 1, (2, 5, 6))
    a = args([[tri]], (5, 6))
    assert (a.nmaps, a.per_map, a.out_shape) == (1, 1, (1, 5, 6))
    a = args([], (5, 6))
    assert (a.nmaps, a.npoly, a.max_pts, a.out_shape) == (1, 0, 1, (5, 6))
    xy, npts = np.zeros((3, 2, 4, 2)), np.zeros((3, 2), np.int32)
    a = args((xy, npts), (5, 6), shifts=np.zeros((3, 2)))
    assert a.xy is xy and a.npts is npts and (a.nmaps, a.per_map, a.npoly, a.max_pts) == (3, 1, 2, 4)
    a = args((xy[0], npts[0]), (5, 6))
    assert (a.nmaps, a.per_map, a.out_shape) == (1, 0, (5, 6))


TRI = [(1, 1), (4, 1), (2, 3)]


@pytest.mark.parametrize("polygons,shape,kw,exc", [
    ([TRI], (5,), {}, ValueError),
    ([TRI], (0, 6), {}, ValueError),
    ([TRI], (5, 6.5), {}, ValueError),
    ([TRI], (65536, 32768), {}, ValueError),
    ([[(1, 1, 1), (2, 2, 2), (3, 3, 3)]], (5, 6), {}, ValueError),
    ([TRI, [TRI]], (5, 6), {}, ValueError),
    (7, (5, 6), {}, ValueError),
    ([np.zeros((1025, 2))], (5, 6), {}, ValueError),
    ([TRI], (5, 6), {"values": [1, 2]}, ValueError),
    ([TRI], (5, 6), {"values": [1.5]}, ValueError),
    ([TRI], (5, 6), {"values": [1 << 31]}, ValueError),
    ([TRI], (5, 6), {"background": 0.5}, ValueError),
    ([TRI], (5, 6), {"background": 1 << 31}, ValueError),
    ([TRI], (5, 6), {"shifts": [1, 2]}, ValueError),
    ([TRI], (5, 6), {"shifts": np.zeros((2, 3))}, ValueError),
    ([[TRI], [TRI]], (5, 6), {"shifts": np.zeros((3, 2))}, ValueError),
    ((np.zeros((2, 4, 2)), np.zeros((3,), np.int32)), (5, 6), {}, ValueError),
    ((np.zeros((2, 4, 3)), np.zeros((2,), np.int32)), (5, 6), {}, ValueError),
    ((np.zeros((2, 4, 2), np.float32), np.zeros((2,), np.int32)), (5, 6), {}, RuntimeError),
    ((np.zeros((2, 4, 2)), np.zeros((2,), np.int64)), (5, 6), {}, RuntimeError),
])
def test_python_checks_raise_without_a_device(polygons, shape, kw, exc):
    from librir_amd import device as D
    from librir_amd import signal_processing as S

    for fn in (D.polygon_map, S.polygon_map):
        with pytest.raises(exc, match="polygon_map"):
            fn(polygons, shape, **kw)


def test_device_api_checks_out_and_tensors_before_any_device_work():
    import torch

    from librir_amd import device as D

    for out in (torch.zeros((5, 6), dtype=torch.int64), torch.zeros((6, 5), dtype=torch.int32), torch.zeros((5, 6), dtype=torch.int32), np.zeros((5, 6))):
        with pytest.raises(RuntimeError, match="polygon_map"):
            D.polygon_map([TRI], (5, 6), out=out)
    with pytest.raises(ValueError, match="polygon_map"):
        D.polygon_map([TRI], (5, 6), shifts=torch.zeros((2, 3), dtype=torch.float64))
    with pytest.raises(RuntimeError, match="polygon_map"):  # packed polygons on the CPU
        D.polygon_map((torch.zeros((1, 3, 2), dtype=torch.float64), torch.zeros(1, dtype=torch.int32)), (5, 6))


HIPCC_FOUND = os.path.exists(B.HIPCC) or shutil.which(B.HIPCC) is not None


@pytest.mark.skipif(not HIPCC_FOUND, reason="hipcc not found")
def test_polygon_kernels_use_no_scratch(tmp_path):
    asm = str(tmp_path / "polygon_kernels.s")
    flags = [f for f in B.COMMON if f != "-fPIC"]
    subprocess.check_call([B.HIPCC] + flags + ["-S", "--cuda-device-only", os.path.join(B.CSRC, "polygon_kernels.hip"), "-o", asm],
                          stderr=subprocess.DEVNULL)
    text = open(asm).read()
    assert "global_store_dwordx4" in text  # finished rows go out 16 bytes a lane
    meta = text[text.index("amdhsa.kernels:"):text.index(".end_amdgpu_metadata")]
    kernels = {}
    for block in re.split(r"\n  - ", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            kernels[name.group(1)] = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1))
    for stage in ("prepare", "fill"):
        assert len([k for k in kernels if "polygon_%s_kernel" % stage in k]) == 1, (stage, sorted(kernels))
    assert len(kernels) == 2, sorted(kernels)
    assert all(v == 0 for v in kernels.values()), kernels
