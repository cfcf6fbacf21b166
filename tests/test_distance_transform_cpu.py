"""CPU: the exact Euclidean distance transform - the brute-force reference the GPU tests use (distance_cases.py) agrees with
round(scipy.ndimage.distance_transform_edt ** 2) wherever a background pixel exists, the separable reference equals the brute force, indices
included, the four disc identities hold against scipy's binary erosion and dilation, both entry points are declared and exported, every
refused argument is refused by both without a device, the workspace query refuses bad geometry and grows with the stack, there is no CPU
fallback, the Python forms exist and check their parameters without a device, and the kernels of distance_kernels.hip use no scratch."""
import ctypes as ct
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from librir_amd import build as B
from distance_cases import DIST2_NONE, SHAPES, brute_force, foregrounds, label_map, separable

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [s for s in SHAPES if s[0] * s[1] <= 37 * 70] + [(12, 17)]


@pytest.mark.parametrize("h,w", SMALL)
def test_reference_equals_scipy_edt_squared(h, w):
    ndi = pytest.importorskip("scipy.ndimage")
    for name, fg in foregrounds(h, w):
        dist2, _ = brute_force(fg)
        if fg.all():
            assert (dist2 == DIST2_NONE).all(), name
            continue
        assert np.array_equal(dist2, np.rint(ndi.distance_transform_edt(fg) ** 2).astype(np.int32)), name
        assert (dist2[~fg] == 0).all() and (dist2[fg] > 0).all(), name


@pytest.mark.parametrize("h,w", SHAPES)
def test_separable_reference_equals_the_brute_force(h, w):
    images = [fg for _, fg in foregrounds(h, w)] + [label_map(h, w) != 0, label_map(h, w) != 3]
    for i, fg in enumerate(images):
        for border, rows in [(False, h), (True, h)] + ([(True, max(0, h - 3)), (False, 1), (True, 0)] if i % 4 == 0 else []):
            want, got = brute_force(fg, 0, border, rows), separable(fg, 0, border, rows)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (i, border, rows)


def test_reference_properties():
    """the definition's corners: an index names a background pixel at exactly dist2, the lowest such; none gives DIST2_NONE and -1, with the
    border switch b^2 and -1; the rows outside the image get 0 and their own index; the background value is honoured"""
    h, w = 12, 17
    for name, fg in foregrounds(h, w):
        dist2, index = brute_force(fg)
        ys, xs = np.mgrid[:h, :w]
        if fg.all():
            assert (index == -1).all(), name
            d, i = brute_force(fg, border=True)
            b = np.minimum(np.minimum(xs + 1, w - xs), np.minimum(ys + 1, h - ys))
            assert np.array_equal(d, b * b) and (i == -1).all()
            continue
        qy, qx = index // w, index % w
        assert not fg[qy, qx].any() and np.array_equal((ys - qy) ** 2 + (xs - qx) ** 2, dist2), name
        flat = np.flatnonzero(~fg)
        for y, x in ((0, 0), (h // 2, w // 2), (h - 1, w - 1), (3, 11)):
            d = (y - flat // w) ** 2 + (x - flat % w) ** 2
            assert index[y, x] == flat[d == d.min()].min(), (name, y, x)
        d, i = brute_force(fg, border=True)
        assert (d <= dist2).all() and np.array_equal(i == -1, d < dist2) and np.array_equal(i[i >= 0], index[i >= 0]), name
    lab = label_map(h, w)
    assert np.array_equal(brute_force(lab, 3)[0], brute_force(lab != 3)[0]) and not np.array_equal(brute_force(lab, 3)[0], brute_force(lab, 0)[0])
    d, i = brute_force(lab, 0, False, 5)
    assert (d[5:] == 0).all() and np.array_equal(i[5:], np.arange(h * w).reshape(h, w)[5:]) and np.array_equal(d[:5], brute_force(lab[:5])[0])


def disc(radius):
    r = int(np.floor(radius))
    ys, xs = np.mgrid[-r:r + 1, -r:r + 1]
    return ys * ys + xs * xs <= radius * radius


@pytest.mark.parametrize("radius", [0, 1, 1.5, 2.3, 5, 20])
def test_disc_identities(radius):
    ndi = pytest.importorskip("scipy.ndimage")
    r2 = int(np.floor(radius * radius))
    for h, w in [(1, 1), (1, 7), (7, 1), (12, 17), (5, 65)]:
        for name, fg in foregrounds(h, w):
            st = disc(radius)
            assert np.array_equal(fg & (brute_force(fg)[0] > r2), ndi.binary_erosion(fg, st, border_value=1)), (name, h, w)
            assert np.array_equal(fg & (brute_force(fg, border=True)[0] > r2), ndi.binary_erosion(fg, st, border_value=0)), (name, h, w)
            assert np.array_equal(brute_force(~fg)[0] <= r2, ndi.binary_dilation(fg, st)), (name, h, w)


DEVICE_SIGNATURE = (r"int rir_distance_transform_device\(int type, const void \*d_src, int w, int h, int nframes, int background, int border, int rows, "
                    r"int \*d_dist2,\s+int \*d_index /\* may be NULL \*/, void \*d_work, size_t work_bytes, void \*stream\);")
WORKSPACE_SIGNATURE = r"size_t rir_distance_transform_workspace_bytes\(int w, int h, int nframes, int want_indices\);"
HOST_SIGNATURE = (r"int rir_distance_transform\(int type, const void \*src, int w, int h, int nframes, int background, int border, int rows, int \*dist2, "
                  r"int \*index\);")


def test_entry_points_are_declared_and_exported(lib):
    dev = open(os.path.join(ROOT, "include", "rir_amd_device.h")).read()
    sp = open(os.path.join(ROOT, "include", "rir_amd_signal_processing.h")).read()
    assert re.search(DEVICE_SIGNATURE, dev) and re.search(WORKSPACE_SIGNATURE, dev) and re.search(HOST_SIGNATURE, sp)
    assert re.search(r"#define RIR_DIST2_NONE 0x7fffffff\b", dev)
    for name in ("rir_distance_transform_device", "rir_distance_transform_workspace_bytes", "rir_distance_transform"):
        assert hasattr(lib, name), name


def _bind(lib):
    lib.rir_distance_transform_device.argtypes = [ct.c_int, ct.c_void_p] + [ct.c_int] * 6 + [ct.c_void_p] * 3 + [ct.c_size_t, ct.c_void_p]
    lib.rir_distance_transform.argtypes = [ct.c_int, ct.c_void_p] + [ct.c_int] * 6 + [ct.c_void_p] * 2
    lib.rir_distance_transform_workspace_bytes.argtypes = [ct.c_int] * 4
    lib.rir_distance_transform_workspace_bytes.restype = ct.c_size_t


GOOD = dict(type=ord("B"), w=5, h=4, nframes=3, background=0, border=0, rows=4)
REFUSED = [dict(type=ord("h")), dict(type=ord("f")), dict(type=ord("I")), dict(type=0), dict(background=256), dict(background=-1),
           dict(type=ord("?"), background=2), dict(type=ord("H"), background=65536), dict(border=2), dict(border=-1), dict(rows=5), dict(rows=-1),
           dict(w=0), dict(h=0), dict(w=16385), dict(h=16385), dict(nframes=-1), dict(src=None), dict(dist2=None), dict(overlap="dist2-src"),
           dict(overlap="index-src"), dict(overlap="index-dist2")]


@pytest.mark.parametrize("change", REFUSED, ids=lambda c: "-".join("%s=%s" % kv for kv in c.items()))
def test_refused_arguments_do_not_need_a_device(lib, change):
    """both entry points refuse the call - and say why - whether or not there is a device: the check comes first"""
    from librir_amd.low_level.misc import last_error

    _bind(lib)
    cells = 3 * 4 * 5
    src = np.full(cells * 4, 7, np.uint8)  # (room for every type)
    outs = np.full(3 * cells, 7, np.int32)
    work = np.zeros(3 * cells + 1, np.int64)
    a = dict(GOOD, src=src.ctypes.data, dist2=outs.ctypes.data, index=outs.ctypes.data + cells * 4)
    overlap = change.get("overlap")
    a.update({k: v for k, v in change.items() if k != "overlap"})
    if overlap == "dist2-src":
        a["dist2"] = a["src"] + cells - 1  # the input's last byte is the output's first
    elif overlap == "index-src":
        a["index"] = a["src"] - cells * 4 + 1
    elif overlap == "index-dist2":
        a["index"] = a["dist2"] + (cells - 1) * 4
    args = (a["type"], a["src"], a["w"], a["h"], a["nframes"], a["background"], a["border"], a["rows"], a["dist2"], a["index"])
    for name, call in (("rir_distance_transform_device", lambda: lib.rir_distance_transform_device(*args, work.ctypes.data, work.nbytes, None)),
                       ("rir_distance_transform", lambda: lib.rir_distance_transform(*args))):
        assert call() == -1
        assert name + ":" in last_error() and "no usable HIP device" not in last_error(), last_error()
    assert (src == 7).all() and (outs == 7).all()


def test_refused_workspaces_do_not_need_a_device(lib):
    from librir_amd.low_level.misc import last_error

    _bind(lib)
    cells = 3 * 4 * 5
    src, outs, work = np.zeros(cells, np.uint8), np.zeros(2 * cells, np.int32), np.zeros(3 * cells + 1, np.int64)
    one = lib.rir_distance_transform_workspace_bytes(5, 4, 1, 1)
    call = lambda s, d, i, wk, nbytes: lib.rir_distance_transform_device(ord("B"), s, 5, 4, 3, 0, 0, 4, d, i, wk, nbytes, None)  # noqa: E731
    s, d, i = src.ctypes.data, outs.ctypes.data, outs.ctypes.data + cells * 4
    for wk, nbytes, word in ((None, work.nbytes, "null"), (work.ctypes.data, one - 1, "workspace"), (work.ctypes.data, 0, "workspace"),
                             (work.ctypes.data + 4, work.nbytes - 4, "aligned"), (d + cells * 4 - 8, work.nbytes, "overlap"), (s - 8, one, "overlap")):
        assert call(s, d, i, wk, nbytes) == -1
        assert "rir_distance_transform_device:" in last_error() and word in last_error() and "no usable HIP device" not in last_error(), last_error()
    # no frames is no work, once the arguments are in order; the index is optional
    assert lib.rir_distance_transform_device(ord("B"), s, 5, 4, 0, 0, 0, 4, d, None, work.ctypes.data, work.nbytes, None) == 0
    assert lib.rir_distance_transform(ord("B"), s, 5, 4, 0, 0, 0, 4, d, None) == 0


def test_workspace_bytes(lib):
    _bind(lib)
    ws = lib.rir_distance_transform_workspace_bytes
    for bad in ((0, 4, 1, 0), (5, 0, 1, 0), (16385, 4, 1, 0), (5, 16385, 1, 1), (5, 4, -1, 0), (5, 4, 1, 2), (5, 4, 1, -1), (-5, 4, 1, 0)):
        assert ws(*bad) == 0, bad
    for w, h in ((5, 4), (640, 512), (16384, 16384), (1, 1)):
        for idx in (0, 1):
            sizes = [ws(w, h, n, idx) for n in (0, 1, 2, 5, 67, 300, 100000)]
            assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[0] == sizes[1], (w, h, sizes)  # (no frames: one frame's share)
            assert sizes[2] in (sizes[1], 2 * sizes[1]) and sizes[-1] <= max(sizes[1], 256 << 20)
    assert ws(640, 512, 2, 1) == 2 * ws(640, 512, 1, 1) and ws(640, 512, 100000, 0) > ws(640, 512, 2, 0)


def test_no_cpu_fallback_without_device(lib):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from librir_amd import signal_processing as S
    from librir_amd.low_level.misc import last_error

    _bind(lib)
    src = (np.arange(3 * 4 * 5) % 3).astype(np.uint8).reshape(3, 4, 5)
    outs, work = np.full((2, 3, 4, 5), -5, np.int32), np.zeros(3 * 4 * 5 * 3 + 1, np.int64)
    assert lib.rir_distance_transform(ord("B"), src.ctypes.data, 5, 4, 3, 0, 0, 4, outs[0].ctypes.data, outs[1].ctypes.data) == -1
    assert "no usable HIP device" in last_error() and (outs == -5).all()
    assert lib.rir_distance_transform_device(ord("B"), src.ctypes.data, 5, 4, 3, 0, 0, 4, outs[0].ctypes.data, outs[1].ctypes.data, work.ctypes.data,
                                             work.nbytes, None) == -1
    assert "no usable HIP device" in last_error() and (outs == -5).all()
    with pytest.raises(RuntimeError):
        S.distance_transform(src)


def test_python_forms_exist():
    from librir_amd import device as D
    from librir_amd import signal_processing as S
    from librir_amd.video_io import IRMovie

    names = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    defaults = lambda f: {k: p.default for k, p in inspect.signature(f).parameters.items() if p.default is not inspect.Parameter.empty}  # noqa: E731
    assert names(D.distance_transform) == ["masks", "background", "border", "rows", "return_indices", "out"]
    assert defaults(D.distance_transform) == {"background": 0, "border": False, "rows": None, "return_indices": False, "out": None}
    assert names(S.distance_transform) == ["images", "background", "border", "rows", "return_indices"]
    assert defaults(S.distance_transform) == {"background": 0, "border": False, "rows": None, "return_indices": False}
    assert "distance_transform" in S.__all__
    assert names(D.disc_erode) == ["mask", "radius", "border"] and defaults(D.disc_erode) == {"border": False}
    for f in (D.disc_dilate, D.disc_open, D.disc_close):
        assert names(f) == ["mask", "radius"] and defaults(f) == {}
    assert D.DIST2_NONE == DIST2_NONE == 0x7FFFFFFF
    assert names(IRMovie.distance_transform) == ["self", "threshold", "selection", "invert", "border", "rows", "return_indices"]
    assert defaults(IRMovie.distance_transform) == {"selection": slice(None), "invert": False, "border": False, "rows": None, "return_indices": False}
    doc = IRMovie.distance_transform.__doc__
    assert "disc_dilate" in doc and "label_images" in doc and "region_stats" in doc and "maximum of dist2" in doc


BAD_PARAMETERS = [dict(background=256), dict(background=-1), dict(background=1.0), dict(background=None), dict(border=2), dict(border="yes"),
                  dict(rows=5), dict(rows=-1)]


@pytest.mark.parametrize("change", BAD_PARAMETERS, ids=lambda c: "-".join("%s=%s" % kv for kv in c.items()))
def test_python_forms_reject_bad_parameters_without_a_device(change):
    import torch

    from librir_amd import device as D
    from librir_amd import signal_processing as S

    kw = dict(dict(background=0, border=False, rows=None), **change)
    masks = torch.zeros((6, 4, 5), dtype=torch.uint8)  # (a CPU tensor: the check comes before any device work)
    with pytest.raises(ValueError):
        D.distance_transform(masks, **kw)
    with pytest.raises(ValueError):
        D.distance_transform(masks[0], return_indices=True, **kw)
    with pytest.raises(ValueError):
        S.distance_transform(np.zeros((6, 4, 5), np.uint8), **kw)


def test_python_forms_reject_wrong_dtypes_shapes_and_outputs_without_a_device():
    import torch

    from librir_amd import device as D
    from librir_amd import signal_processing as S

    for dtype in (torch.int16, torch.float32, torch.int64):
        with pytest.raises(ValueError):
            D.distance_transform(torch.zeros((2, 4, 5), dtype=dtype))
    for dtype in (np.int16, np.float32, np.uint32, np.int64):
        with pytest.raises(ValueError):
            S.distance_transform(np.zeros((2, 4, 5), dtype))
    with pytest.raises(ValueError):
        S.distance_transform(np.zeros((2, 2, 4, 5), np.uint8))
    with pytest.raises(ValueError):
        S.distance_transform(np.zeros((2, 0, 5), np.uint8))
    with pytest.raises(ValueError):
        D.distance_transform(torch.zeros((2, 2, 4, 5), dtype=torch.uint8))
    with pytest.raises(ValueError):
        D.distance_transform(torch.zeros((2, 4, 0), dtype=torch.bool))
    masks = torch.zeros((2, 4, 5), dtype=torch.bool)
    good = torch.zeros((2, 4, 5), dtype=torch.int32)  # (right dtype and shape, but not a CUDA tensor)
    for out in (torch.zeros((2, 4, 5), dtype=torch.int64), torch.zeros((2, 4, 6), dtype=torch.int32), good, (good, good)):
        with pytest.raises(RuntimeError):
            D.distance_transform(masks, out=out)
    for out in (good, (good,), (good, good)):
        with pytest.raises(RuntimeError):
            D.distance_transform(masks, return_indices=True, out=out)
    for f in (D.disc_erode, D.disc_dilate, D.disc_open, D.disc_close):
        for radius in (-1, float("nan"), float("inf"), "3", None, True):
            with pytest.raises(ValueError):
                f(masks, radius)
        with pytest.raises(ValueError):
            f(torch.zeros((2, 4, 5), dtype=torch.uint16), 2)
        with pytest.raises(ValueError):
            f(torch.zeros((5,), dtype=torch.bool), 2)
    with pytest.raises(ValueError):
        D.disc_erode(masks, 2, border=3)
    # radius 0 copies, whatever the device
    for f in (D.disc_erode, D.disc_dilate, D.disc_open, D.disc_close):
        m = torch.tensor([[1, 0], [0, 1]], dtype=torch.uint8)
        got = f(m, 0)
        assert got is not m and got.dtype == m.dtype and torch.equal(got, m)


HIPCC_FOUND = os.path.exists(B.HIPCC) or shutil.which(B.HIPCC) is not None


@pytest.mark.skipif(not HIPCC_FOUND, reason="hipcc not found")
def test_distance_kernels_resources(tmp_path):
    """the unit compiles for gfx950; five kernels - the row pass for the three cell widths, the column pass with and without indices; none has
    a private segment, the row pass holds 3 KiB of LDS a wave, the column pass none.  Looks at the kernels' resource metadata only."""
    asm = str(tmp_path / "distance_kernels.s")
    flags = [f for f in B.COMMON if f != "-fPIC"]
    done = subprocess.run([B.HIPCC] + flags + ["-S", "--cuda-device-only", os.path.join(B.CSRC, "distance_kernels.hip"), "-o", asm], stdout=subprocess.PIPE,
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
    rows = {n: k for n, k in kernels.items() if "distance_rows_kernel" in n}
    columns = {n: k for n, k in kernels.items() if "distance_columns_kernel" in n}
    assert len(kernels) == 5 and len(rows) == 3 and len(columns) == 2, sorted(kernels)
    assert all(k["scratch"] == 0 for k in kernels.values()), {n: k["scratch"] for n, k in kernels.items() if k["scratch"]}
    assert all(k["lds"] == 4 * 256 * 12 for k in rows.values()) and all(k["lds"] == 0 for k in columns.values())
    assert all(k["vgpr"] <= 64 for k in kernels.values()), {n: k["vgpr"] for n, k in kernels.items()}  # (eight waves per SIMD)
