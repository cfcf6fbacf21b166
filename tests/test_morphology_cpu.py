"""CPU: flat morphology - the numpy reference the GPU tests use (morphology_cases.py) agrees with scipy's minimum / maximum filters composed
stage by stage and with a brute-force clipped window, the algebra the unsigned differences lean on holds, both entry points are declared and
exported, every refused argument is refused without a device, there is no CPU fallback, the Python forms exist and check their parameters
without a device, and the kernels of morphology_kernels.hip use no scratch."""
import ctypes as ct
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from librir_amd import build as B
from morphology_cases import CASES, OPS, case_id, make_stack, reference, reference_image, spike_images

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def scipy_composition(img, op, size_y, size_x):
    ndi = pytest.importorskip("scipy.ndimage")
    erode = lambda f: ndi.minimum_filter(f, size=(size_y, size_x), mode="nearest")  # noqa: E731
    dilate = lambda f: ndi.maximum_filter(f, size=(size_y, size_x), mode="nearest")  # noqa: E731
    return {"erode": lambda f: erode(f), "dilate": lambda f: dilate(f), "open": lambda f: dilate(erode(f)), "close": lambda f: erode(dilate(f)),
            "tophat": lambda f: f - dilate(erode(f)), "blackhat": lambda f: erode(dilate(f)) - f, "gradient": lambda f: dilate(f) - erode(f)}[op](img)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_reference_equals_the_scipy_composition(case):
    pytest.importorskip("scipy")
    stack = make_stack(case)
    want = reference(stack, case.op, case.size_y, case.size_x)
    work = stack.view(np.uint8) if stack.dtype == np.bool_ else stack
    got = np.stack([scipy_composition(f, case.op, case.size_y, case.size_x) for f in work]).view(stack.dtype)
    assert got.dtype == want.dtype and np.array_equal(got, want)


def brute_force(img, take_max, size_y, size_x):
    h, w = img.shape
    ry, rx = size_y // 2, size_x // 2
    out = np.empty_like(img)
    for y in range(h):
        for x in range(w):
            win = img[max(0, y - ry):y + ry + 1, max(0, x - rx):x + rx + 1]
            out[y, x] = win.max() if take_max else win.min()
    return out


@pytest.mark.parametrize("size_y,size_x", [(3, 3), (1, 5), (7, 3), (15, 15), (15, 1)])
def test_reference_equals_a_brute_force_clipped_window(size_y, size_x):
    rng = np.random.default_rng(size_y * 16 + size_x)
    img = rng.integers(0, 65536, (13, 17)).astype(np.uint16)
    img[0, 0], img[-1, -1], img[0, 5], img[7, 0] = 65535, 0, 0, 65535
    e, d = brute_force(img, False, size_y, size_x), brute_force(img, True, size_y, size_x)
    assert np.array_equal(reference_image(img, "erode", size_y, size_x), e)
    assert np.array_equal(reference_image(img, "dilate", size_y, size_x), d)
    assert np.array_equal(reference_image(img, "open", size_y, size_x), brute_force(e, True, size_y, size_x))
    assert np.array_equal(reference_image(img, "close", size_y, size_x), brute_force(d, False, size_y, size_x))
    assert np.array_equal(reference_image(img, "gradient", size_y, size_x), d - e)


@pytest.mark.parametrize("case", CASES[::5], ids=case_id)
def test_open_below_close_above_and_no_wrap(case):
    stack = make_stack(case)
    f = (stack.view(np.uint8) if stack.dtype == np.bool_ else stack).astype(np.int64)
    r = {op: reference(stack, op, case.size_y, case.size_x).astype(np.int64) for op in OPS}
    assert (r["open"] <= f).all() and (f <= r["close"]).all() and (r["erode"] <= r["open"]).all() and (r["close"] <= r["dilate"]).all()
    assert np.array_equal(r["tophat"], f - r["open"]) and np.array_equal(r["blackhat"], r["close"] - f)
    assert np.array_equal(r["gradient"], r["dilate"] - r["erode"])


def test_rows_and_size_one():
    stack = spike_images(5, 6, np.uint16)
    for op in OPS:
        got = reference(stack, op, 3, 5, rows=2)
        assert np.array_equal(got[:, 2:], stack[:, 2:]) and np.array_equal(got[:, :2], reference(stack[:, :2], op, 3, 5))
        assert np.array_equal(reference(stack, op, 3, 5, rows=0), stack)
        one = reference(stack, op, 1, 1)
        assert np.array_equal(one, stack if op in OPS[:4] else np.zeros_like(stack))


DEVICE_SIGNATURE = (r"int rir_morphology_device\(int type, const void \*d_src, void \*d_dst, int w, int h, int nframes, int op, int size_x, int size_y, "
                    r"int rows,\s+void \*stream\);")
HOST_SIGNATURE = (r"int rir_morphology\(int type, const void \*src, void \*dst, int w, int h, int nframes, int op, int size_x, int size_y,\s+"
                  r"int rows\);")


def test_entry_points_are_declared_and_exported(lib):
    dev = open(os.path.join(ROOT, "include", "rir_amd_device.h")).read()
    sp = open(os.path.join(ROOT, "include", "rir_amd_signal_processing.h")).read()
    assert re.search(DEVICE_SIGNATURE, dev) and re.search(HOST_SIGNATURE, sp)
    assert hasattr(lib, "rir_morphology_device") and hasattr(lib, "rir_morphology")


def _bind(lib):
    lib.rir_morphology_device.argtypes = [ct.c_int, ct.c_void_p, ct.c_void_p] + [ct.c_int] * 7 + [ct.c_void_p]
    lib.rir_morphology.argtypes = [ct.c_int, ct.c_void_p, ct.c_void_p] + [ct.c_int] * 7


GOOD = dict(type=ord("H"), w=5, h=4, nframes=3, op=2, size_x=3, size_y=5, rows=4)
REFUSED = [dict(type=ord("h")), dict(type=ord("f")), dict(type=0), dict(op=7), dict(op=-1), dict(size_x=4), dict(size_y=2), dict(size_x=17), dict(size_y=0),
           dict(size_x=-3), dict(rows=5), dict(rows=-1), dict(w=0), dict(h=0), dict(nframes=-1), dict(src=None), dict(dst=None), dict(overlap=True)]


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
    args = (a["type"], a["src"], a["dst"], a["w"], a["h"], a["nframes"], a["op"], a["size_x"], a["size_y"], a["rows"])
    for name, call in (("rir_morphology_device", lambda: lib.rir_morphology_device(*args, None)), ("rir_morphology", lambda: lib.rir_morphology(*args))):
        assert call() == -1
        assert name + ":" in last_error() and "no usable HIP device" not in last_error(), last_error()
    assert (buf == 7).all()


def test_source_as_destination(lib):
    """the device entry refuses dst == src as an overlap; no frames is no work, whatever the pointers"""
    from librir_amd.low_level.misc import last_error

    _bind(lib)
    buf = np.zeros(3 * 4 * 5, np.uint16)
    assert lib.rir_morphology_device(ord("H"), buf.ctypes.data, buf.ctypes.data, 5, 4, 3, 0, 3, 3, 4, None) == -1
    assert "overlap" in last_error()
    assert lib.rir_morphology_device(ord("H"), buf.ctypes.data, buf.ctypes.data, 5, 4, 0, 0, 3, 3, 4, None) == 0
    assert lib.rir_morphology(ord("H"), buf.ctypes.data, buf.ctypes.data, 5, 4, 0, 0, 3, 3, 4) == 0


def test_no_cpu_fallback_without_device(lib):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from librir_amd import signal_processing as S
    from librir_amd.low_level.misc import last_error

    _bind(lib)
    src = np.arange(3 * 4 * 5, dtype=np.uint16).reshape(3, 4, 5)
    dst = np.zeros_like(src)
    assert lib.rir_morphology(ord("H"), src.ctypes.data, dst.ctypes.data, 5, 4, 3, 0, 3, 3, 4) == -1
    assert "no usable HIP device" in last_error()
    assert not dst.any()
    assert lib.rir_morphology_device(ord("H"), src.ctypes.data, dst.ctypes.data, 5, 4, 3, 0, 3, 3, 4, None) == -1
    assert "no usable HIP device" in last_error()
    assert not dst.any()
    with pytest.raises(RuntimeError):
        S.morphology(src, "erode", 3)


def test_python_forms_exist():
    from librir_amd import device as D
    from librir_amd import signal_processing as S
    from librir_amd.video_io import IRMovie

    names = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    defaults = lambda f: {k: p.default for k, p in inspect.signature(f).parameters.items() if p.default is not inspect.Parameter.empty}  # noqa: E731
    assert names(D.morphology) == ["frames", "op", "size", "rows", "out"] and defaults(D.morphology) == {"rows": None, "out": None}
    for name in ("erode", "dilate", "morph_open", "morph_close", "top_hat", "black_hat", "morph_gradient"):
        f = getattr(D, name)
        assert names(f) == ["frames", "size", "rows", "out"] and defaults(f) == {"rows": None, "out": None}, name
    assert names(S.morphology) == ["images", "op", "size", "rows"] and defaults(S.morphology) == {"rows": None}
    assert "morphology" in S.__all__
    assert names(IRMovie.morphology) == ["self", "op", "size", "selection", "rows", "out"]
    assert defaults(IRMovie.morphology) == {"selection": slice(None), "rows": None, "out": None}
    assert "morph_open" in IRMovie.morphology.__doc__ and "label_images" in IRMovie.morphology.__doc__ and '"tophat", 9' in IRMovie.morphology.__doc__


BAD_PARAMETERS = [dict(size=4), dict(size=17), dict(size=0), dict(size=(3, 4)), dict(size=(3, 3, 3)), dict(size=(3,)), dict(size=3.0), dict(op="median"),
                  dict(op=2), dict(rows=5), dict(rows=-1)]


@pytest.mark.parametrize("change", BAD_PARAMETERS, ids=lambda c: "-".join("%s=%s" % kv for kv in c.items()))
def test_python_forms_reject_bad_parameters_without_a_device(change):
    import torch

    from librir_amd import device as D
    from librir_amd import signal_processing as S

    kw = dict(dict(op="open", size=3, rows=None), **change)
    frames = torch.zeros((6, 4, 5), dtype=torch.uint16)  # (a CPU tensor: the check comes before any device work)
    with pytest.raises(ValueError):
        D.morphology(frames, kw["op"], kw["size"], kw["rows"])
    with pytest.raises(ValueError):
        D.morphology(frames[0], kw["op"], kw["size"], kw["rows"])
    with pytest.raises(ValueError):
        S.morphology(np.zeros((6, 4, 5), np.uint16), kw["op"], kw["size"], kw["rows"])
    if "op" not in change:
        with pytest.raises(ValueError):
            D.morph_open(frames, kw["size"], kw["rows"])
        with pytest.raises(ValueError):
            D.top_hat(frames, kw["size"], rows=kw["rows"])


def test_python_forms_reject_wrong_dtypes_and_outputs_without_a_device():
    import torch

    from librir_amd import device as D
    from librir_amd import signal_processing as S

    for dtype in (torch.int16, torch.float32, torch.int32):
        with pytest.raises(ValueError):
            D.morphology(torch.zeros((2, 4, 5), dtype=dtype), "erode", 3)
    for dtype in (np.int16, np.float32, np.uint32):
        with pytest.raises(ValueError):
            S.morphology(np.zeros((2, 4, 5), dtype), "erode", 3)
    with pytest.raises(ValueError):
        S.morphology(np.zeros((2, 2, 4, 5), np.uint16), "erode", 3)
    frames = torch.zeros((2, 4, 5), dtype=torch.uint16)
    for out in (torch.zeros((2, 4, 5), dtype=torch.uint8), torch.zeros((2, 4, 6), dtype=torch.uint16), torch.zeros((1, 4, 5), dtype=torch.uint16),
                torch.zeros((2, 4, 5), dtype=torch.uint16)):  # (the last one: right dtype and shape, but not a CUDA tensor)
        with pytest.raises(RuntimeError):
            D.morphology(frames, "erode", 3, out=out)
        with pytest.raises(RuntimeError):
            D.dilate(frames, 3, out=out)


HIPCC_FOUND = os.path.exists(B.HIPCC) or shutil.which(B.HIPCC) is not None


@pytest.mark.skipif(not HIPCC_FOUND, reason="hipcc not found")
def test_morphology_kernels_resources(tmp_path):
    """the unit compiles for gfx950; 50 kernels: the pair kernel for 2 pixel types (bool runs as uint8) x 3 radii x 7 ops, and the LDS tile
    kernel for the 2 pixel types x 4 radius classes; none has a private segment, the pair kernels use no LDS and the tile kernels only
    the dynamic LDS their launch sizes (three buffers of the tile's region: 33 120 bytes at most).  Looks at the kernels' resource metadata
    only."""
    asm = str(tmp_path / "morphology_kernels.s")
    flags = [f for f in B.COMMON if f != "-fPIC"]
    done = subprocess.run([B.HIPCC] + flags + ["-S", "--cuda-device-only", os.path.join(B.CSRC, "morphology_kernels.hip"), "-o", asm], stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0, done.stdout
    text = open(asm).read()
    meta = text[text.index("amdhsa.kernels:"):text.index(".end_amdgpu_metadata")]
    kernels = {}
    for block in re.split(r"\n  - ", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            field = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1))  # noqa: E731
            kernels[name.group(1)] = {"scratch": field("private_segment_fixed_size"), "lds": field("group_segment_fixed_size"), "vgpr": field("vgpr_count")}
    wave = {n: k for n, k in kernels.items() if "morph_wave_kernel" in n}
    tile = {n: k for n, k in kernels.items() if "morph_tile_kernel" in n}
    assert len(kernels) == 50 and len(wave) == 42 and len(tile) == 8, sorted(kernels)
    assert all(k["scratch"] == 0 for k in kernels.values()), {n: k["scratch"] for n, k in kernels.items() if k["scratch"]}
    assert all(k["lds"] == 0 for k in kernels.values()), {n: k["lds"] for n, k in kernels.items() if k["lds"]}
    # (two workgroups of 256 threads per CU need at most 256 registers a lane; the 3x3 kernels are meant to run at four and more)
    assert all(k["vgpr"] <= 256 for k in wave.values())
    assert all(k["vgpr"] <= 128 for n, k in wave.items() if "Li1ELi" in n), {n: k["vgpr"] for n, k in wave.items() if "Li1ELi" in n}
