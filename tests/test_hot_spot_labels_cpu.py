"""CPU: hot spots labelled straight from the frames - the numpy oracle the GPU tests use (hot_spot_cases.py) agrees with scipy's labelling
of the kept mask and with scenes worked by hand; the entry points are declared and exported, size their workspace and refuse bad
arguments; there is no CPU fallback; the Python API checks its arguments without a device, a float threshold stands for its floor."""
import ctypes as ct
import inspect
import os
import re

import numpy as np
import pytest

import hot_spot_cases as HC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("shape", HC.RANDOM_SHAPES)
@pytest.mark.parametrize("kw", [{}] + HC.RANDOM_FILTERS, ids=lambda kw: "+".join(kw) or "low")
def test_oracle_map_is_scipys_labelling_of_the_kept_mask(shape, kw):
    ndi = pytest.importorskip("scipy.ndimage")
    frames = HC.random_frames(shape)
    o = HC.oracle(frames, HC.RANDOM_LOW, **kw)
    for f in range(shape[0]):
        lab, k = ndi.label(o["labels"][f] > 0)
        assert np.array_equal(o["labels"][f], lab) and o["counts"][f] == k + 1
    if not kw:
        assert np.array_equal(o["labels"] > 0, frames > HC.RANDOM_LOW)


def test_oracle_on_a_scene_worked_by_hand():
    """low 5, high 8: A = {(0,0), (0,1), (1,1)} holds a 9 and touches the border; B = {(1,3), (2,3), (2,4), (3,3)} holds its only 9 in row 3,
    which rows = 3 cuts; C = {(2,0)} is a strong speck on the border"""
    f = np.array([[6, 9, 0, 0, 0, 0],
                  [0, 6, 0, 6, 0, 0],
                  [9, 0, 0, 6, 6, 0],
                  [0, 0, 0, 9, 0, 0],
                  [0, 0, 0, 0, 0, 0]], np.uint16)
    o = HC.oracle(f, 5)
    assert o["labels"][0].tolist() == [[1, 1, 0, 0, 0, 0], [0, 1, 0, 2, 0, 0], [3, 0, 0, 2, 2, 0], [0, 0, 0, 2, 0, 0], [0] * 6]
    assert o["counts"].tolist() == [4] and o["area"][0, :4].tolist() == [0, 3, 4, 1] and o["first"][0, :4].tolist() == [-1, 0, 9, 12]
    o = HC.oracle(f, 5, high=8)
    assert o["counts"].tolist() == [4]  # every component holds a 9
    o = HC.oracle(f, 5, high=8, rows=3)
    assert o["labels"][0].tolist() == [[1, 1, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0], [2, 0, 0, 0, 0, 0], [0] * 6, [0] * 6]  # (3,3) is cut: B is weak
    assert o["area"][0, :3].tolist() == [0, 3, 1] and o["first"][0, :3].tolist() == [-1, 0, 12]
    o = HC.oracle(f, 5, min_area=2, clear_border=True)
    assert o["counts"].tolist() == [2] and o["first"][0, :2].tolist() == [-1, 9] and o["area"][0, :2].tolist() == [0, 4]
    assert (o["labels"][0] > 0).sum() == 4
    o = HC.oracle(f, 5, clear_border=True, rows=3)  # row 2 is the last one: B touches it
    assert o["counts"].tolist() == [1] and not o["labels"].any()
    o = HC.oracle(f, 5, max_area=3, table_entries=2)
    assert o["counts"].tolist() == [3] and o["first"].tolist() == [[-1, 0]] and o["area"].tolist() == [[0, 3]]
    assert o["labels"][0].tolist() == [[1, 1, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0], [2, 0, 0, 0, 0, 0], [0] * 6, [0] * 6]


def test_random_scene_keeps_and_drops_components_across_tile_borders():
    """what makes the GPU test on (2, 70, 130) a test of the hand-over across tile borders, for each predicate on its own"""
    frames = HC.random_frames((2, 70, 130))
    want = [[(22, 11), (16, 14)], [(32, 1), (23, 7)], [(21, 12), (20, 10)], [(15, 18), (18, 12)]]
    for kw, exp in zip(HC.RANDOM_FILTERS, want):
        o = HC.oracle(frames, HC.RANDOM_LOW, **kw)
        assert [HC.spanning(o, f) for f in range(2)] == exp, kw


def test_scenes():
    for m, last in ((HC.spiral(64, 128), 63 * 128 + 127), (HC.comb(64, 128), 63 * 128 + 124)):
        r = HC.roots_of(m)
        assert np.unique(r).tolist() == [-1, 0] and np.flatnonzero(m.reshape(-1))[-1] == last  # one component from pixel 0 to the last tile


def test_entry_points_are_declared_and_exported(lib):
    dev = open(os.path.join(ROOT, "include", "rir_amd_device.h")).read()
    assert re.search(r"int rir_label_hot_spots_device\(const unsigned short \*d_frames, int w, int h, int nframes, int rows, int low, "
                     r"const int \*d_low_map, int use_high,\s+int high, const int \*d_high_map, int min_area, int max_area, int clear_border, "
                     r"int \*d_dst, int \*d_first, int \*d_area,\s+int table_entries, int \*d_count, void \*d_work, size_t work_bytes, "
                     r"void \*stream\);", dev)
    assert re.search(r"size_t rir_label_hot_spots_workspace_bytes\(int w, int h, int nframes\);", dev)
    for name in ("rir_label_hot_spots_device", "rir_label_hot_spots_workspace_bytes"):
        assert hasattr(lib, name), name
    assert not hasattr(lib, "rir_label_hot_spots") and not hasattr(lib, "label_hot_spots")  # label maps are born on the device


def test_workspace_query(lib):
    f = lib.rir_label_hot_spots_workspace_bytes
    f.argtypes = [ct.c_int] * 3
    f.restype = ct.c_size_t
    base = lib.rir_label_workspace_bytes_batch
    base.argtypes = [ct.c_int] * 3
    base.restype = ct.c_size_t

    def marks(w, h, n):  # two bitmaps - a 64-bit word per 64 pixels of each 256-pixel block, a multiple of 8 words per frame - and a byte a pixel
        words = ((w * h + 255) // 256 * 4 + 7) // 8 * 8
        plane = (w * h * 4 + 63) // 64 * 64 // 4
        return 2 * n * words * 8 + (n * plane + 63) // 64 * 64

    for w, h, n in [(640, 512, 1000), (1, 1, 1), (130, 70, 2), (65536, 32767, 1), (3, 5, 65535)]:
        assert f(w, h, n) == base(w, h, n) + marks(w, h, n) and base(w, h, n) > 0, (w, h, n)
    for bad in [(0, 5, 1), (5, 0, 1), (-1, 5, 1), (5, 5, 0), (5, 5, -1), (5, 5, 65536), (65536, 32768, 1)]:
        assert f(*bad) == 0, bad


def test_no_cpu_fallback_without_device(lib):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from librir_amd.low_level.misc import last_error

    frames = np.full((2, 3, 5), 9, np.uint16)
    dst = np.zeros((2, 3, 5), np.int32)
    first, area = np.zeros((2, 4), np.int32), np.zeros((2, 4), np.int32)
    count = np.zeros(2, np.int32)
    work = np.zeros(4096, np.int64)
    fn = lib.rir_label_hot_spots_device
    vp = ct.c_void_p
    fn.argtypes = [vp] + [ct.c_int] * 5 + [vp, ct.c_int, ct.c_int, vp] + [ct.c_int] * 3 + [vp] * 3 + [ct.c_int, vp, vp, ct.c_size_t, vp]
    assert fn(frames.ctypes.data, 5, 3, 2, 3, 1, None, 0, 0, None, 1, 15, 0, dst.ctypes.data, first.ctypes.data, area.ctypes.data, 4,
              count.ctypes.data, work.ctypes.data, work.nbytes, None) == -1
    assert "no usable HIP device" in last_error()
    assert not dst.any() and not first.any() and not area.any() and not count.any()


def test_python_api_exists():
    from librir_amd import device as D
    from librir_amd.video_io import IRMovie

    params = inspect.signature(D.label_hot_spots).parameters
    assert list(params) == ["frames", "low", "high", "min_area", "max_area", "clear_border", "rows", "table_entries"]
    assert [params[k].default for k in list(params)[2:]] == [None, 1, None, False, None, None]
    assert callable(D._label_hot_spots_into)
    # track_hot_spots and track_hot_spots_geometry keep their parameter lists (test_track_components_cpu.py and test_region_geometry_cpu.py
    # pin them); the filters of the kept components are a sibling's
    params = inspect.signature(IRMovie.track_kept_hot_spots).parameters
    assert list(params)[1:] == ["threshold", "selection", "table_entries", "stats", "geometry", "high", "min_area", "max_area", "clear_border"]
    assert [params[k].default for k in list(params)[2:]] == [slice(None), None, True, False, None, 1, None, False]
    doc = IRMovie.track_kept_hot_spots.__doc__
    assert "KEPT" in doc and "min_area <= area <= max_area" in doc and "> high" in doc and "row or column" in doc
    assert "track_kept_hot_spots" in IRMovie.track_hot_spots.__doc__


H, W = 4, 5


@pytest.mark.parametrize("kw,text", [
    (dict(low=np.zeros((W, H))), "low must be"),
    (dict(low=np.zeros(H * W)), "low must be"),
    (dict(low=1, high=np.zeros((H, W + 1))), "high must be"),
    (dict(low=1, high=np.zeros((1, H, W))), "high must be"),
    (dict(low=1, min_area=0), "min_area"),
    (dict(low=1, min_area=-3), "min_area"),
    (dict(low=1, min_area=1.5), "min_area"),
    (dict(low=1, min_area=4, max_area=3), "max_area"),
    (dict(low=1, max_area=0), "max_area"),
    (dict(low=1, rows=0), "rows"),
    (dict(low=1, rows=H + 1), "rows"),
    (dict(low=1, rows=-1), "rows"),
    (dict(low=float("nan")), "NaN"),
    (dict(low=1, high=float("nan")), "NaN"),
    (dict(low=np.full((H, W), np.nan)), "NaN"),
    (dict(low=1, high=np.where(np.eye(H, W) > 0, np.nan, 3.0)), "NaN"),
    (dict(low=1, table_entries=0), "table_entries"),
])
def test_python_checks_raise_without_a_device(kw, text):
    """CPU tensors: every check comes before any device work, for numpy and tensor thresholds alike"""
    import torch

    from librir_amd import device as D

    frames = torch.zeros((2, H, W), dtype=torch.uint16)
    with pytest.raises(ValueError, match="label_hot_spots.*" + text):
        D.label_hot_spots(frames, **kw)
    as_tensor = {k: torch.from_numpy(v) if isinstance(v, np.ndarray) else v for k, v in kw.items()}
    with pytest.raises(ValueError, match="label_hot_spots.*" + text):
        D.label_hot_spots(frames, **as_tensor)
    with pytest.raises(ValueError, match="label_hot_spots.*" + text):
        D._label_hot_spots_args((2, H, W), **kw)


def test_everything_in_order_but_the_device():
    import torch

    from librir_amd import device as D

    with pytest.raises(RuntimeError, match="CUDA"):
        D.label_hot_spots(torch.zeros((2, H, W), dtype=torch.uint16), 1, high=0, min_area=2, max_area=2, clear_border=True, rows=H)
    with pytest.raises(ValueError, match="label_hot_spots"):
        D._label_hot_spots_args((2, 2, H, W), 1)
    with pytest.raises(ValueError, match="label_hot_spots"):
        D._label_hot_spots_args((2, 0, W), 1)


def test_thresholds_are_floored_clamped_int32():
    """for an integer v, v > t == v > floor(t); thresholds are held as int32 in [-1, 65535]"""
    import torch

    from librir_amd import device as D

    def spec(low, high=None, **kw):
        return D._label_hot_spots_args((H, W), low, high, **kw)[3]

    for t, want in [(3, 3), (3.0, 3), (3.7, 3), (-0.5, -1), (-7, -1), (-1e30, -1), (float("-inf"), -1), (65534.9, 65534), (65535, 65535),
                    (1 << 40, 65535), (7e9, 65535), (float("inf"), 65535), (np.float32(2.5), 2), (np.int64(-9), -1), (np.uint16(65535), 65535)]:
        s = spec(t, t)
        assert (s.low, s.low_map, s.high, s.high_map, s.use_high) == (want, None, want, None, True), t
        v = np.arange(-2, 65538)
        if np.isfinite(t):
            assert np.array_equal(v[2:-2] > t, v[2:-2] > want), t  # every uint16 value answers alike
    m = np.array([[3.7, -0.5, -1e30, 65534.9, 7e9]] * H)
    want = np.array([[3, -1, -1, 65534, 65535]] * H, np.int32)
    for given in (m, m.astype(np.float32), torch.from_numpy(m)):
        s = spec(given, given)
        for got in (s.low_map, s.high_map):
            got = got.numpy() if isinstance(got, torch.Tensor) else got
            assert got.dtype == np.int32 and np.array_equal(got, want)
    big = np.array([[-5, 0, 65535, 65536, 1 << 40]] * H, np.int64)
    assert np.array_equal(spec(big).low_map, np.array([[-1, 0, 65535, 65535, 65535]] * H, np.int32))
    assert np.array_equal(spec(np.full((H, W), 65535, np.uint16)).low_map, np.full((H, W), 65535, np.int32))
    s = spec(5)
    assert (s.use_high, s.min_area, s.max_area, s.clear_border, s.rows, s.table_entries) == (False, 1, 0x7FFFFFFF, False, H, H * W + 1)
    s = spec(5, 2, min_area=3, max_area=3, clear_border=True, rows=1, table_entries=7)  # a high below low is legal
    assert (s.low, s.high, s.use_high, s.min_area, s.max_area, s.clear_border, s.rows, s.table_entries) == (5, 2, True, 3, 3, True, 1, 7)
    assert D._label_hot_spots_args((3, 40, 50), 1)[:3] == (3, 40, 50) and D._label_hot_spots_args((40, 50), 1)[3].table_entries == 1024
