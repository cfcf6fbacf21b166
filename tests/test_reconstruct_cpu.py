"""CPU: grey-level morphological reconstruction - the numpy reference the GPU tests use (reconstruct_cases.py) agrees with an independent brute
force of the path definition, with scipy's binary_propagation and binary_fill_holes, and satisfies the operator's identities; both entry points
are declared with the documented signatures and exported, every refused argument is refused without a device, there is no CPU fallback, the
Python forms exist and check their parameters without a device, and the kernels of reconstruct_kernels.hip use no scratch."""
import ctypes as ct
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from librir_amd import build as B
from reconstruct_cases import (BORDER, CASES, MARKER, METHODS, SHIFT, TOP, TYPES, as_int, brute_force_image, case_id, diagonal, footprint, levels_image,
                               make_case, marker_image, reference, reference_image, serpentine, spiral)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("connectivity", [8, 4])
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("dtype", TYPES)
def test_reference_equals_the_brute_force_of_the_path_definition(dtype, method, connectivity):
    rng = np.random.default_rng(len(dtype) * 16 + connectivity + (method == "erosion"))
    top = TOP[dtype]
    for h, w in [(9, 11), (1, 1), (1, 7), (6, 1), (3, 2), (7, 8)]:
        mask = levels_image(rng, h, w, dtype)
        marker = marker_image(rng, mask, 0.15)
        g, f = as_int(mask), as_int(marker)
        if method == "erosion":
            f = top - f
        if h * w > 4:
            assert g.min() == 0 and g.max() == top  # values 0 and the type's maximum included
        want = brute_force_image(f, g, method, connectivity)
        assert np.array_equal(reference_image(f, g, method, connectivity)[0], want), (h, w)
        as_type = lambda a: a.astype(np.uint8).view(np.bool_) if dtype == "bool" else a.astype(dtype)  # noqa: E731
        assert np.array_equal(as_int(reference(mask, as_type(f), method, connectivity)), want)


@pytest.mark.parametrize("connectivity", [8, 4])
def test_bool_reference_equals_binary_propagation(connectivity):
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(connectivity)
    for _ in range(10):
        mask = rng.random((17, 23)) < 0.6
        marker = (rng.random((17, 23)) < 0.05) & mask
        assert np.array_equal(reference(mask, marker, "dilation", connectivity), ndi.binary_propagation(marker, structure=footprint(connectivity), mask=mask))


def test_fill_holes_equals_binary_fill_holes():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(3)
    for _ in range(10):
        mask = rng.random((17, 23)) < 0.55
        assert np.array_equal(reference(mask, None, "erosion", 4, BORDER), ndi.binary_fill_holes(mask))


@pytest.mark.parametrize("case", CASES[::3], ids=case_id)
def test_identities(case):
    mask, marker = make_case(case)
    top = TOP[case.dtype]
    far = np.full_like(mask, top if case.method == "erosion" else 0)
    kw = dict(method=case.method, connectivity=case.connectivity)
    assert np.array_equal(reference(mask, mask, **kw), mask)  # R(G, G) = G
    assert np.array_equal(reference(mask, far, **kw), far)  # R(0, G) = 0
    seed = marker if marker is not None else np.stack([marker_image(np.random.default_rng(1), m) for m in mask])
    r = reference(mask, seed, **kw)
    assert np.array_equal(reference(mask, r, **kw), r)  # idempotent
    assert not as_int(reference(mask, None, mode=SHIFT, param=0, output=1, **kw)).any()  # h_dome(f, 0) = 0
    flip = lambda a: ~a if a.dtype == np.bool_ else (top - a).astype(a.dtype)  # noqa: E731
    other = METHODS[1 - METHODS.index(case.method)]
    assert np.array_equal(flip(reference(flip(mask), flip(seed), other, case.connectivity)), r)  # erosion is dilation on the complements
    for mode, param in ((SHIFT, case.param), (BORDER, 0)):
        a = reference(mask, None, mode=mode, param=param, **kw)
        assert np.array_equal(flip(reference(flip(mask), None, other, case.connectivity, mode, param)), a)
        d = reference(mask, None, mode=mode, param=param, output=1, **kw)
        assert np.array_equal(as_int(d), np.abs(as_int(mask) - as_int(a)))


def test_rows_rule():
    mask, marker = make_case(CASES[0]._replace(h=9, w=11))
    for rows in (6, 1, 0):
        got = reference(mask, marker, rows=rows)
        assert np.array_equal(got[:, rows:], mask[:, rows:])
        if rows:
            assert np.array_equal(got[:, :rows], reference(mask[:, :rows], marker[:, :rows]))
        b = reference(mask, None, mode=BORDER, rows=rows)
        if rows:
            assert np.array_equal(b[:, rows - 1], mask[:, rows - 1])  # the border marker uses row rows - 1


def test_corridors():
    """the reach cases of the GPU test: the whole corridor fills, after as many iterations as it is long"""
    for maker in (serpentine, spiral):
        mask = maker(17, 64)
        marker = np.zeros_like(mask)
        marker[0, 0] = 700
        its = []
        got = reference(mask, marker, iterations=its)
        assert np.array_equal(got, np.where(mask > 0, 700, 0)) and its[0] == 567
    mask = diagonal(17, 64)
    marker = np.zeros_like(mask)
    marker[0, 0] = 700
    assert np.array_equal(reference(mask, marker, connectivity=8), np.where(mask > 0, 700, 0))
    assert np.array_equal(reference(mask, marker, connectivity=4), marker)


DEVICE_SIGNATURE = (r"int rir_reconstruct_device\(int type, const void \*d_mask, const void \*d_marker, void \*d_dst, int w, int h, int nframes, int method, "
                    r"int connectivity,\s+int marker_mode, int param, int output, int rows, void \*d_work, size_t work_bytes, int \*rounds, void \*stream\);")
WORKSPACE_SIGNATURE = r"size_t rir_reconstruct_workspace_bytes\(int type, int w, int h, int nframes\);"
HOST_SIGNATURE = (r"int rir_reconstruct\(int type, const void \*mask, const void \*marker, void \*dst, int w, int h, int nframes, int method, "
                  r"int connectivity,\s+int marker_mode, int param, int output, int rows, int \*rounds\);")


def test_entry_points_are_declared_and_exported(lib):
    dev = open(os.path.join(ROOT, "include", "rir_amd_device.h")).read()
    sp = open(os.path.join(ROOT, "include", "rir_amd_signal_processing.h")).read()
    assert re.search(DEVICE_SIGNATURE, dev) and re.search(WORKSPACE_SIGNATURE, dev) and re.search(HOST_SIGNATURE, sp)
    assert hasattr(lib, "rir_reconstruct_device") and hasattr(lib, "rir_reconstruct") and hasattr(lib, "rir_reconstruct_workspace_bytes")
    assert "did not converge" in dev and "SYNCHRONOUS" in dev and "cannot be captured into a graph" in dev


def _bind(lib):
    lib.rir_reconstruct_device.argtypes = [ct.c_int, ct.c_void_p, ct.c_void_p, ct.c_void_p] + [ct.c_int] * 9 + [ct.c_void_p, ct.c_size_t, ct.c_void_p, ct.c_void_p]
    lib.rir_reconstruct.argtypes = [ct.c_int, ct.c_void_p, ct.c_void_p, ct.c_void_p] + [ct.c_int] * 9 + [ct.c_void_p]
    lib.rir_reconstruct_workspace_bytes.argtypes = [ct.c_int] * 4
    lib.rir_reconstruct_workspace_bytes.restype = ct.c_size_t


GOOD = dict(type=ord("H"), w=5, h=4, nframes=3, method=0, connectivity=8, marker_mode=0, param=0, output=0, rows=4)
REFUSED = [dict(type=ord("h")), dict(type=ord("i")), dict(type=0), dict(method=2), dict(method=-1), dict(connectivity=6), dict(connectivity=0),
           dict(marker_mode=3), dict(marker_mode=-1), dict(output=2), dict(output=-1), dict(param=65536), dict(param=-1), dict(type=ord("B"), param=256),
           dict(type=ord("?"), param=2), dict(marker_mode=1, param=7), dict(marker_mode=2), dict(marker=None), dict(rows=5), dict(rows=-1), dict(w=0),
           dict(h=0), dict(nframes=-1), dict(mask=None), dict(dst=None), dict(overlap="mask"), dict(overlap="marker")]


@pytest.mark.parametrize("change", REFUSED, ids=lambda c: "-".join("%s=%s" % kv for kv in c.items()))
def test_refused_arguments_do_not_need_a_device(lib, change):
    """both entry points refuse the call - and say why - whether or not there is a device: the check comes first.  (marker_mode 1 or 2 with
    the marker of GOOD present, and mode 0 without one, are among them)"""
    from librir_amd.low_level.misc import last_error

    _bind(lib)
    frames = 3 * 4 * 5
    buf = np.full(4 * frames, 7, np.uint16)
    work = np.zeros(64, np.int64)
    a = dict(GOOD, mask=buf.ctypes.data, marker=buf.ctypes.data + frames * 2, dst=buf.ctypes.data + 2 * frames * 2)
    a.update({k: v for k, v in change.items() if k != "overlap"})
    if change.get("overlap") == "mask":
        a["dst"] = a["mask"] + 2 * 4 * 5 * 2  # the last mask frame is the first destination frame
    if change.get("overlap") == "marker":
        a["dst"] = a["marker"] - 4 * 5 * 2  # the last destination frame is the first marker frame (and the mask's too)
        a["mask"] = buf.ctypes.data + 3 * frames * 2
    args = (a["type"], a["mask"], a["marker"], a["dst"], a["w"], a["h"], a["nframes"], a["method"], a["connectivity"], a["marker_mode"], a["param"],
            a["output"], a["rows"])
    rounds = ct.c_int(-5)
    for name, call in (("rir_reconstruct_device", lambda: lib.rir_reconstruct_device(*args, work.ctypes.data, work.nbytes, ct.addressof(rounds), None)),
                       ("rir_reconstruct", lambda: lib.rir_reconstruct(*args, ct.addressof(rounds)))):
        assert call() == -1
        assert name + ":" in last_error() and "no usable HIP device" not in last_error(), last_error()
    assert (buf == 7).all() and rounds.value == -5


def test_workspace_and_no_frames(lib):
    """a workspace below one frame's share, a null or a misaligned one are refused; no frames is no work; the marker may be the mask"""
    from librir_amd.low_level.misc import last_error

    _bind(lib)
    buf = np.zeros(2 * 3 * 4 * 5, np.uint16)
    work = np.zeros(64, np.int64)
    src, dst = buf.ctypes.data, buf.ctypes.data + 3 * 4 * 5 * 2
    one = lib.rir_reconstruct_workspace_bytes(ord("H"), 5, 4, 1)
    assert one > 0 and lib.rir_reconstruct_workspace_bytes(ord("H"), 5, 4, 3) == 3 * one and lib.rir_reconstruct_workspace_bytes(ord("H"), 5, 4, 0) == one
    assert lib.rir_reconstruct_workspace_bytes(ord("f"), 5, 4, 3) == 0 and lib.rir_reconstruct_workspace_bytes(ord("H"), 0, 4, 3) == 0
    assert lib.rir_reconstruct_workspace_bytes(ord("H"), 5, 4, -1) == 0
    tail = (src, None, dst, 5, 4, 3, 0, 8, 1, 3, 1, 4)
    for ws, size in ((work.ctypes.data, one - 1), (work.ctypes.data, 0), (None, work.nbytes), (work.ctypes.data + 4, work.nbytes - 4)):
        assert lib.rir_reconstruct_device(ord("H"), *tail, ws, size, None, None) == -1
        assert "rir_reconstruct_device:" in last_error() and "workspace" in last_error() and "no usable HIP device" not in last_error()
    assert lib.rir_reconstruct_device(ord("H"), src, None, dst, 5, 4, 3, 0, 8, 1, 3, 1, 4, dst, 3 * one, None, None) == -1  # the workspace on dst
    assert "overlaps" in last_error()
    rounds = ct.c_int(-5)
    assert lib.rir_reconstruct_device(ord("H"), src, src, src, 5, 4, 0, 0, 8, 0, 0, 0, 4, work.ctypes.data, work.nbytes, ct.addressof(rounds), None) == 0
    assert rounds.value == 0
    assert lib.rir_reconstruct(ord("H"), src, src, src, 5, 4, 0, 0, 8, 0, 0, 0, 4, None) == 0
    import torch

    if not torch.cuda.is_available():  # marker == mask passes the checks: what fails is the device
        assert lib.rir_reconstruct_device(ord("H"), src, src, dst, 5, 4, 3, 0, 8, 0, 0, 0, 4, work.ctypes.data, work.nbytes, None, None) == -1
        assert "no usable HIP device" in last_error()


def test_no_cpu_fallback_without_device(lib):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from librir_amd import signal_processing as S
    from librir_amd.low_level.misc import last_error

    _bind(lib)
    src = np.arange(3 * 4 * 5, dtype=np.uint16).reshape(3, 4, 5)
    dst = np.zeros_like(src)
    work = np.zeros(64, np.int64)
    assert lib.rir_reconstruct(ord("H"), src.ctypes.data, None, dst.ctypes.data, 5, 4, 3, 0, 8, 1, 3, 1, 4, None) == -1
    assert "no usable HIP device" in last_error()
    assert not dst.any()
    assert lib.rir_reconstruct_device(ord("H"), src.ctypes.data, None, dst.ctypes.data, 5, 4, 3, 0, 8, 1, 3, 1, 4, work.ctypes.data, work.nbytes, None, None) == -1
    assert "no usable HIP device" in last_error()
    assert not dst.any()
    for call in (lambda: S.reconstruct(src, src), lambda: S.h_dome(src, 3), lambda: S.h_maxima(src, 3), lambda: S.fill_holes(src)):
        with pytest.raises(RuntimeError):
            call()


def test_python_forms_exist():
    from librir_amd import device as D
    from librir_amd import signal_processing as S
    from librir_amd.video_io import IRMovie

    names = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    defaults = lambda f: {k: p.default for k, p in inspect.signature(f).parameters.items() if p.default is not inspect.Parameter.empty}  # noqa: E731
    assert names(D.reconstruct) == ["marker", "mask", "method", "connectivity", "rows", "out", "return_rounds"]
    assert defaults(D.reconstruct) == {"method": "dilation", "connectivity": 8, "rows": None, "out": None, "return_rounds": False}
    for name in ("h_maxima", "h_dome", "h_minima", "h_basin"):
        f = getattr(D, name)
        assert names(f) == ["frames", "h", "connectivity", "rows", "out"] and defaults(f) == {"connectivity": 8, "rows": None, "out": None}, name
    for name, conn in (("regional_maxima", 8), ("regional_minima", 8), ("fill_holes", 4), ("clear_border", 8)):
        f = getattr(D, name)
        assert names(f) == ["frames", "connectivity", "rows", "out"] and defaults(f) == {"connectivity": conn, "rows": None, "out": None}, name
    assert "plateau of value 0 is no maximum" in D.regional_maxima.__doc__ and "maximum is no minimum" in D.regional_minima.__doc__
    assert "binary_fill_holes" in D.fill_holes.__doc__ and "graph" in D.reconstruct.__doc__
    assert names(S.reconstruct) == ["marker", "mask", "method", "connectivity", "rows"]
    assert names(S.h_maxima) == names(S.h_dome) == ["images", "h", "connectivity", "rows"] and names(S.fill_holes) == ["images", "connectivity", "rows"]
    assert defaults(S.fill_holes) == {"connectivity": 4, "rows": None} and defaults(S.h_dome) == {"connectivity": 8, "rows": None}
    assert all(n in S.__all__ for n in ("reconstruct", "h_maxima", "h_dome", "fill_holes"))
    for f in (IRMovie.h_dome, IRMovie.h_maxima):
        assert names(f) == ["self", "h", "selection", "connectivity", "rows", "out"]
        assert defaults(f) == {"selection": slice(None), "connectivity": 8, "rows": None, "out": None}
    assert "label_hot_spots(mov.h_dome(40), low=10, min_area=4)" in IRMovie.h_dome.__doc__


BAD_PARAMETERS = [dict(connectivity=6), dict(connectivity=0), dict(connectivity="8"), dict(connectivity=True), dict(rows=5), dict(rows=-1), dict(h=-1),
                  dict(h=65536), dict(h=2.0), dict(h=None), dict(h=True), dict(method="open"), dict(method=0)]


@pytest.mark.parametrize("change", BAD_PARAMETERS, ids=lambda c: "-".join("%s=%s" % kv for kv in c.items()))
def test_python_forms_reject_bad_parameters_without_a_device(change):
    import torch

    from librir_amd import device as D
    from librir_amd import signal_processing as S

    kw = dict(dict(method="dilation", connectivity=8, rows=None, h=3), **change)
    frames = torch.zeros((6, 4, 5), dtype=torch.uint16)  # (a CPU tensor: the check comes before any device work)
    images = np.zeros((6, 4, 5), np.uint16)
    if "h" not in change:
        for f in (frames, frames[0]):
            with pytest.raises(ValueError):
                D.reconstruct(f, f, kw["method"], kw["connectivity"], kw["rows"])
        with pytest.raises(ValueError):
            S.reconstruct(images, images, kw["method"], kw["connectivity"], kw["rows"])
    if "method" not in change:
        for form in (D.h_maxima, D.h_dome, D.h_minima, D.h_basin):
            with pytest.raises(ValueError):
                form(frames, kw["h"], kw["connectivity"], kw["rows"])
        for form in (S.h_maxima, S.h_dome):
            with pytest.raises(ValueError):
                form(images, kw["h"], kw["connectivity"], kw["rows"])
        if "h" not in change:
            for form in (D.regional_maxima, D.regional_minima, D.fill_holes, D.clear_border):
                with pytest.raises(ValueError):
                    form(frames, kw["connectivity"], rows=kw["rows"])
            with pytest.raises(ValueError):
                S.fill_holes(images, kw["connectivity"], kw["rows"])


def test_python_forms_reject_wrong_dtypes_markers_and_outputs_without_a_device():
    import torch

    from librir_amd import device as D
    from librir_amd import signal_processing as S

    for dtype in (torch.int16, torch.float32, torch.int32):
        z = torch.zeros((2, 4, 5), dtype=dtype)
        for call in (lambda: D.reconstruct(z, z), lambda: D.h_dome(z, 1), lambda: D.fill_holes(z), lambda: D.regional_maxima(z)):
            with pytest.raises(ValueError):
                call()
    for dtype in (np.int16, np.float32, np.uint32):
        z = np.zeros((2, 4, 5), dtype)
        for call in (lambda: S.reconstruct(z, z), lambda: S.h_dome(z, 1), lambda: S.fill_holes(z)):
            with pytest.raises(ValueError):
                call()
    with pytest.raises(ValueError):
        S.h_dome(np.zeros((2, 2, 4, 5), np.uint16), 1)
    with pytest.raises(ValueError):
        D.h_dome(torch.zeros((2, 4, 5), dtype=torch.uint8), 256)
    with pytest.raises(ValueError):
        D.h_dome(torch.zeros((2, 4, 5), dtype=torch.bool), 2)
    frames = torch.zeros((2, 4, 5), dtype=torch.uint16)
    for marker in (torch.zeros((2, 4, 5), dtype=torch.uint8), torch.zeros((2, 4, 6), dtype=torch.uint16), np.zeros((2, 4, 5), np.uint16)):
        with pytest.raises(ValueError):
            D.reconstruct(marker, frames)
    with pytest.raises(ValueError):
        S.reconstruct(np.zeros((2, 4, 5), np.uint8), np.zeros((2, 4, 5), np.uint16))
    for out in (torch.zeros((2, 4, 5), dtype=torch.uint8), torch.zeros((2, 4, 6), dtype=torch.uint16), torch.zeros((1, 4, 5), dtype=torch.uint16),
                torch.zeros((2, 4, 5), dtype=torch.uint16)):  # (the last one: right dtype and shape, but not a CUDA tensor)
        with pytest.raises(RuntimeError):
            D.reconstruct(frames, frames, out=out)
        with pytest.raises(RuntimeError):
            D.h_dome(frames, 3, out=out)
        with pytest.raises(RuntimeError):
            D.regional_maxima(frames, out=out)


HIPCC_FOUND = os.path.exists(B.HIPCC) or shutil.which(B.HIPCC) is not None


@pytest.mark.skipif(not HIPCC_FOUND, reason="hipcc not found")
def test_reconstruct_kernels_resources(tmp_path):
    """the unit compiles for gfx950; 18 kernels: the round kernel for 2 pixel types (bool runs as uint8) x 4 sources x 2 connectivities and the
    finish kernel for the 2 types; none has a private segment; a round keeps two uint16 planes of the 66 x 34 tile in LDS (under 10 KB, so
    that LDS never bounds residency) and stays at 64 registers a lane or below (8 waves per SIMD).  Looks at the kernels' resource metadata
    only."""
    asm = str(tmp_path / "reconstruct_kernels.s")
    flags = [f for f in B.COMMON if f != "-fPIC"]
    done = subprocess.run([B.HIPCC] + flags + ["-S", "--cuda-device-only", os.path.join(B.CSRC, "reconstruct_kernels.hip"), "-o", asm], stdout=subprocess.PIPE,
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
    rounds = {n: k for n, k in kernels.items() if "reconstruct_round_kernel" in n}
    finish = {n: k for n, k in kernels.items() if "reconstruct_finish_kernel" in n}
    assert len(kernels) == 18 and len(rounds) == 16 and len(finish) == 2, sorted(kernels)
    assert all(k["scratch"] == 0 for k in kernels.values()), {n: k["scratch"] for n, k in kernels.items() if k["scratch"]}
    assert all(2 * 66 * 34 * 2 <= k["lds"] < 10240 and k["vgpr"] <= 64 for k in rounds.values()), rounds
    assert all(k["lds"] == 0 for k in finish.values())
