"""CPU: spatial rank filters - the numpy reference the GPU tests use (rank_cases.py) agrees with scipy's rank, median and percentile filters
with mode="nearest", percentile_rank takes scipy's rank, the two extreme ranks are the morphology reference's erode and dilate, both entry
points are declared and exported, every refused argument is refused without a device, there is no CPU fallback, the Python forms exist and
check their parameters without a device, and the kernels of rank_kernels.hip use no scratch and at most 256 registers."""
import ctypes as ct
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import morphology_cases
from librir_amd import build as B
from rank_cases import CASES, case_id, make_stack, reference, reference_image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_reference_equals_scipy(case):
    ndi = pytest.importorskip("scipy.ndimage")
    stack = make_stack(case)
    size, cells = (case.size_y, case.size_x), case.size_y * case.size_x
    want = reference(stack, case.rank, case.size_y, case.size_x)
    work = stack.view(np.uint8) if stack.dtype == np.bool_ else stack
    got = np.stack([ndi.rank_filter(f, case.rank, size=size, mode="nearest") for f in work]).view(stack.dtype)
    assert got.dtype == want.dtype and np.array_equal(got, want)
    assert np.array_equal(reference(stack, case.rank - cells, case.size_y, case.size_x), want)  # a negative rank counts from the end
    if case.rank == cells // 2:
        assert np.array_equal(np.stack([ndi.median_filter(f, size=size, mode="nearest") for f in work]).view(stack.dtype), want)


PERCENTS = [0, 10, 25, 50, 75, 99.9, 100, -25]


@pytest.mark.parametrize("size_y,size_x", [(3, 3), (5, 5), (7, 3), (1, 5), (9, 9), (15, 15)])
def test_percentile_rank_is_scipys_choice(size_y, size_x):
    """on an image whose pixels all differ, every rank gives another image: the rank scipy's percentile_filter took is the one whose image it
    returned"""
    ndi = pytest.importorskip("scipy.ndimage")
    from librir_amd.signal_processing import percentile_rank

    img = np.random.default_rng(size_y * 16 + size_x).permutation(23 * 31).astype(np.uint16).reshape(23, 31)
    by_rank = [reference_image(img, r, size_y, size_x) for r in range(size_y * size_x)]
    for percent in PERCENTS:
        got = ndi.percentile_filter(img, percent, size=(size_y, size_x), mode="nearest")
        ranks = [r for r, image in enumerate(by_rank) if np.array_equal(image, got)]
        assert ranks == [percentile_rank(percent, size_y, size_x)], (percent, ranks)


def test_percentile_rank_rule():
    from librir_amd.signal_processing import percentile_rank

    assert percentile_rank(100, 3, 3) == 8 and percentile_rank(0, 3, 3) == 0 and percentile_rank(50, 3, 3) == 4 and percentile_rank(50, 5, 5) == 12
    assert percentile_rank(-100, 5, 5) == 0 and percentile_rank(-25, 3, 3) == percentile_rank(75, 3, 3) == 6 and percentile_rank(99.9, 15, 15) == 224
    for bad in (100.5, -100.5, 1000, float("nan")):
        with pytest.raises(ValueError):
            percentile_rank(bad, 3, 3)


@pytest.mark.parametrize("case", CASES[::6], ids=case_id)
def test_extreme_ranks_are_erode_and_dilate(case):
    stack = make_stack(case)
    cells = case.size_y * case.size_x
    assert np.array_equal(reference(stack, 0, case.size_y, case.size_x), morphology_cases.reference(stack, "erode", case.size_y, case.size_x))
    assert np.array_equal(reference(stack, cells - 1, case.size_y, case.size_x), morphology_cases.reference(stack, "dilate", case.size_y, case.size_x))
    work = stack.view(np.uint8) if stack.dtype == np.bool_ else stack
    assert np.array_equal(reference_image(work[0], 0, case.size_y, case.size_x), morphology_cases.reference_image(work[0], "erode", case.size_y, case.size_x))
    assert np.array_equal(reference_image(work[0], cells - 1, case.size_y, case.size_x),
                          morphology_cases.reference_image(work[0], "dilate", case.size_y, case.size_x))


def test_rows_and_size_one():
    stack = morphology_cases.spike_images(5, 6, np.uint16)
    top = stack.copy()
    top[:, 2:] = 65535  # what lies below the image must not be seen: the clamp goes to rows - 1
    for rank in (1, 7, 13):
        got = reference(top, rank, 3, 5, rows=2)
        assert np.array_equal(got[:, 2:], top[:, 2:]) and np.array_equal(got[:, :2], reference(stack[:, :2], rank, 3, 5))
        assert np.array_equal(reference(stack, rank, 3, 5, rows=0), stack)
    assert np.array_equal(reference(stack, 0, 1, 1), stack)


DEVICE_SIGNATURE = (r"int rir_rank_filter_device\(int type, const void \*d_src, void \*d_dst, int w, int h, int nframes, int rank, int size_x, int size_y, "
                    r"int rows,\s+void \*stream\);")
HOST_SIGNATURE = (r"int rir_rank_filter\(int type, const void \*src, void \*dst, int w, int h, int nframes, int rank, int size_x, int size_y,\s*"
                  r"int rows\);")


def test_entry_points_are_declared_and_exported(lib):
    dev = open(os.path.join(ROOT, "include", "rir_amd_device.h")).read()
    sp = open(os.path.join(ROOT, "include", "rir_amd_signal_processing.h")).read()
    assert re.search(DEVICE_SIGNATURE, dev) and re.search(HOST_SIGNATURE, sp)
    assert hasattr(lib, "rir_rank_filter_device") and hasattr(lib, "rir_rank_filter")


def _bind(lib):
    lib.rir_rank_filter_device.argtypes = [ct.c_int, ct.c_void_p, ct.c_void_p] + [ct.c_int] * 7 + [ct.c_void_p]
    lib.rir_rank_filter.argtypes = [ct.c_int, ct.c_void_p, ct.c_void_p] + [ct.c_int] * 7


GOOD = dict(type=ord("H"), w=5, h=4, nframes=3, rank=7, size_x=3, size_y=5, rows=4)
REFUSED = [dict(type=ord("h")), dict(type=ord("f")), dict(type=0), dict(rank=15), dict(rank=-1), dict(rank=225), dict(size_x=4), dict(size_y=2),
           dict(size_x=17), dict(size_y=0), dict(size_x=-3), dict(rows=5), dict(rows=-1), dict(w=0), dict(h=0), dict(nframes=-1), dict(src=None),
           dict(dst=None), dict(overlap=True)]


@pytest.mark.parametrize("change", REFUSED, ids=lambda c: "-".join("%s=%s" % kv for kv in c.items()))
def test_refused_arguments_do_not_need_a_device(lib, change):
    """both entry points refuse the call - and say why - whether or not there is a device: the check comes first"""
    from librir_amd.low_level.misc import last_error

    _bind(lib)
    buf = np.full(2 * 3 * 4 * 5, 7, np.uint16)
    a = dict(GOOD, src=buf.ctypes.data, dst=buf.ctypes.data + 3 * 4 * 5 * 2)
    overlap = change.get("overlap", False)
    a.update({k: v for k, v in change.items() if k != "overlap"})
    if overlap:
        a["dst"] = a["src"] + 2 * 4 * 5 * 2  # the last source frame is the first destination frame
    args = (a["type"], a["src"], a["dst"], a["w"], a["h"], a["nframes"], a["rank"], a["size_x"], a["size_y"], a["rows"])
    for name, call in (("rir_rank_filter_device", lambda: lib.rir_rank_filter_device(*args, None)), ("rir_rank_filter", lambda: lib.rir_rank_filter(*args))):
        assert call() == -1
        assert name + ":" in last_error() and "no usable HIP device" not in last_error(), last_error()
    assert (buf == 7).all()


def test_source_as_destination(lib):
    """the device entry refuses dst == src as an overlap; no frames is no work, whatever the pointers"""
    from librir_amd.low_level.misc import last_error

    _bind(lib)
    buf = np.zeros(3 * 4 * 5, np.uint16)
    assert lib.rir_rank_filter_device(ord("H"), buf.ctypes.data, buf.ctypes.data, 5, 4, 3, 4, 3, 3, 4, None) == -1
    assert "overlap" in last_error()
    assert lib.rir_rank_filter_device(ord("H"), buf.ctypes.data, buf.ctypes.data, 5, 4, 0, 4, 3, 3, 4, None) == 0
    assert lib.rir_rank_filter(ord("H"), buf.ctypes.data, buf.ctypes.data, 5, 4, 0, 4, 3, 3, 4) == 0


def test_no_cpu_fallback_without_device(lib):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from librir_amd import signal_processing as S
    from librir_amd.low_level.misc import last_error

    _bind(lib)
    src = np.arange(3 * 4 * 5, dtype=np.uint16).reshape(3, 4, 5)
    dst = np.zeros_like(src)
    for rank in (4, 0, 8):  # the median, and the two ranks that go to the morphology kernels
        assert lib.rir_rank_filter(ord("H"), src.ctypes.data, dst.ctypes.data, 5, 4, 3, rank, 3, 3, 4) == -1
        assert "no usable HIP device" in last_error()
        assert lib.rir_rank_filter_device(ord("H"), src.ctypes.data, dst.ctypes.data, 5, 4, 3, rank, 3, 3, 4, None) == -1
        assert "no usable HIP device" in last_error()
        assert not dst.any()
    with pytest.raises(RuntimeError):
        S.rank_filter(src, 4, 3)


def test_python_forms_exist():
    from librir_amd import device as D
    from librir_amd import signal_processing as S
    from librir_amd.video_io import IRMovie

    names = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    defaults = lambda f: {k: p.default for k, p in inspect.signature(f).parameters.items() if p.default is not inspect.Parameter.empty}  # noqa: E731
    none = {"rows": None, "out": None}
    assert names(D.rank_filter) == ["frames", "rank", "size", "rows", "out"] and defaults(D.rank_filter) == none
    assert names(D.window_median) == ["frames", "size", "rows", "out"] and defaults(D.window_median) == none
    assert names(D.percentile_filter) == ["frames", "percent", "size", "rows", "out"] and defaults(D.percentile_filter) == none
    assert names(S.rank_filter) == ["images", "rank", "size", "rows"] and defaults(S.rank_filter) == {"rows": None}
    assert names(S.percentile_rank) == ["percent", "size_y", "size_x"]
    assert names(S.rir_signal_processing._rank_filter_args) == ["shape", "dtype_name", "rank", "size", "rows"]
    assert "rank_filter" in S.__all__ and "percentile_rank" in S.__all__
    assert names(IRMovie.rank_filter) == ["self", "rank", "size", "selection", "rows", "out"]
    assert names(IRMovie.window_median) == ["self", "size", "selection", "rows", "out"]
    for f in (IRMovie.rank_filter, IRMovie.window_median):
        assert defaults(f) == {"selection": slice(None), "rows": None, "out": None}
    assert names(D.median_filter) == ["frames"]  # (the reference's 3x3 filter keeps its form)


def test_rank_filter_args():
    from librir_amd.signal_processing.rir_signal_processing import _rank_filter_args

    assert _rank_filter_args((2, 4, 5), "uint16", 7, (5, 3), None) == (ord("H"), 7, 5, 3, 4)
    assert _rank_filter_args((2, 4, 5), "uint8", -1, 3, 2) == (ord("B"), 8, 3, 3, 2)
    assert _rank_filter_args((0, 4, 5), "bool", -9, 3, 0) == (ord("?"), 0, 3, 3, 0)


BAD_PARAMETERS = [dict(size=4), dict(size=17), dict(size=0), dict(size=(3, 4)), dict(size=(3, 3, 3)), dict(size=(3,)), dict(size=3.0), dict(rank=9),
                  dict(rank=-10), dict(rank=4.0), dict(rank="median"), dict(rank=None), dict(rows=5), dict(rows=-1)]


@pytest.mark.parametrize("change", BAD_PARAMETERS, ids=lambda c: "-".join("%s=%s" % kv for kv in c.items()))
def test_python_forms_reject_bad_parameters_without_a_device(change):
    import torch

    from librir_amd import device as D
    from librir_amd import signal_processing as S

    kw = dict(dict(rank=4, size=3, rows=None), **change)
    frames = torch.zeros((6, 4, 5), dtype=torch.uint16)  # (a CPU tensor: the check comes before any device work)
    with pytest.raises(ValueError):
        D.rank_filter(frames, kw["rank"], kw["size"], kw["rows"])
    with pytest.raises(ValueError):
        D.rank_filter(frames[0], kw["rank"], kw["size"], kw["rows"])
    with pytest.raises(ValueError):
        S.rank_filter(np.zeros((6, 4, 5), np.uint16), kw["rank"], kw["size"], kw["rows"])
    if "rank" not in change:
        with pytest.raises(ValueError):
            D.window_median(frames, kw["size"], kw["rows"])
        with pytest.raises(ValueError):
            D.percentile_filter(frames, 25, kw["size"], rows=kw["rows"])


def test_python_forms_reject_wrong_percents_dtypes_and_outputs_without_a_device():
    import torch

    from librir_amd import device as D
    from librir_amd import signal_processing as S

    frames = torch.zeros((2, 4, 5), dtype=torch.uint16)
    for percent in (101, -100.5, float("nan")):
        with pytest.raises(ValueError):
            D.percentile_filter(frames, percent, 3)
    for dtype in (torch.int16, torch.float32, torch.int32):
        with pytest.raises(ValueError):
            D.rank_filter(torch.zeros((2, 4, 5), dtype=dtype), 4, 3)
    for dtype in (np.int16, np.float32, np.uint32):
        with pytest.raises(ValueError):
            S.rank_filter(np.zeros((2, 4, 5), dtype), 4, 3)
    with pytest.raises(ValueError):
        S.rank_filter(np.zeros((2, 2, 4, 5), np.uint16), 4, 3)
    for out in (torch.zeros((2, 4, 5), dtype=torch.uint8), torch.zeros((2, 4, 6), dtype=torch.uint16), torch.zeros((1, 4, 5), dtype=torch.uint16),
                torch.zeros((2, 4, 5), dtype=torch.uint16)):  # (the last one: right dtype and shape, but not a CUDA tensor)
        with pytest.raises(RuntimeError):
            D.rank_filter(frames, 4, 3, out=out)
        with pytest.raises(RuntimeError):
            D.window_median(frames, 3, out=out)


HIPCC_FOUND = os.path.exists(B.HIPCC) or shutil.which(B.HIPCC) is not None


@pytest.mark.skipif(not HIPCC_FOUND, reason="hipcc not found")
def test_rank_kernels_resources(tmp_path):
    """the unit compiles for gfx950; 20 kernels: the pair kernel for 2 pixel types (bool runs as uint8) x 2 sizes, and the LDS tile kernel for
    the 2 pixel types x 8 window heights; none has a private segment or more than 256 registers, the pair kernels use no LDS and the tile
    kernels the 16 bit planes of their tile with its halo (46 rows of 3 dwords each at most).  Looks at the kernels' resource metadata only."""
    asm = str(tmp_path / "rank_kernels.s")
    flags = [f for f in B.COMMON if f != "-fPIC"]
    done = subprocess.run([B.HIPCC] + flags + ["-S", "--cuda-device-only", os.path.join(B.CSRC, "rank_kernels.hip"), "-o", asm], stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0, done.stdout
    text = open(asm).read()
    meta = text[text.index("amdhsa.kernels:"):text.index(".end_amdgpu_metadata")]
    kernels = {}
    for block in re.split(r"\n  - ", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            field = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1))  # noqa: E731
            kernels[name.group(1)] = {"scratch": field("private_segment_fixed_size"), "lds": field("group_segment_fixed_size"), "vgpr": field("vgpr_count"),
                                      "spilled": field("vgpr_spill_count")}
    wave = {n: k for n, k in kernels.items() if "rank_median_wave_kernel" in n}
    tile = {n: k for n, k in kernels.items() if "rank_tile_kernel" in n}
    assert len(kernels) == 20 and len(wave) == 4 and len(tile) == 16, sorted(kernels)
    assert all(k["scratch"] == 0 and k["spilled"] == 0 for k in kernels.values()), {n: k for n, k in kernels.items() if k["scratch"] or k["spilled"]}
    assert all(k["vgpr"] <= 256 for k in kernels.values()), {n: k["vgpr"] for n, k in kernels.items()}
    assert all(k["lds"] == 0 for k in wave.values())
    assert sorted(k["lds"] for k in tile.values()) == sorted(2 * [16 * (32 + 2 * ry) * 3 * 4 for ry in range(8)])
