"""CPU: per-region geometry - the numpy oracle the GPU tests use agrees with a per-pixel restatement of the contract, the entry points are
declared and exported and refuse bad arguments, there is no CPU fallback, the Python API checks its arguments without a device, the float64
helpers of RegionGeometry agree with a direct computation on pixel coordinates, and the kernels of geometry_kernels.hip use no scratch."""
import ctypes as ct
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from librir_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("count", "bbox", "moments", "weighted")


def region_geometry_oracle(labels, nregions, frames=None):
    """the contract with int64 numpy scatter operations: per (frame, region) count, bbox (xmin, ymin, xmax, ymax; -1 when empty), moments
    (sums of x, y, x^2, x*y, y^2) and, with frames, weighted (sums of v, v*x, v*y; else None); labels outside [0, nregions) ignored.
    -> dict of [n][nregions] leading arrays"""
    lab = np.asarray(labels)
    if frames is not None:
        frames = np.asarray(frames)
        if frames.ndim == 2:
            frames = frames[None]
        n, h, w = frames.shape
    else:
        n, h, w = (lab[None] if lab.ndim == 2 else lab).shape
    lab = np.broadcast_to(lab.astype(np.int64), (n, h, w)).reshape(n, -1)
    idx = np.arange(h * w, dtype=np.int64)
    keep = (lab >= 0) & (lab < nregions)
    f = np.broadcast_to(np.arange(n, dtype=np.int64)[:, None], lab.shape)
    cell = (f * nregions + lab)[keep]
    x, y = np.broadcast_to(idx % w, lab.shape)[keep], np.broadcast_to(idx // w, lab.shape)[keep]
    cells = n * nregions

    def total(values):
        acc = np.zeros(cells, np.int64)
        np.add.at(acc, cell, values)
        return acc

    count = total(1)
    big = np.iinfo(np.int64).max
    lo_x, lo_y, hi_x, hi_y = np.full(cells, big), np.full(cells, big), np.full(cells, -1, np.int64), np.full(cells, -1, np.int64)
    np.minimum.at(lo_x, cell, x)
    np.minimum.at(lo_y, cell, y)
    np.maximum.at(hi_x, cell, x)
    np.maximum.at(hi_y, cell, y)
    empty = count == 0
    out = {
        "count": count.astype(np.int32).reshape(n, nregions),
        "bbox": np.stack([np.where(empty, -1, lo_x), np.where(empty, -1, lo_y), hi_x, hi_y], 1).astype(np.int32).reshape(n, nregions, 4),
        "moments": np.stack([total(x), total(y), total(x * x), total(x * y), total(y * y)], 1).reshape(n, nregions, 5),
        "weighted": None,
    }
    if frames is not None:
        v = frames.reshape(n, -1).astype(np.int64)[keep]
        out["weighted"] = np.stack([total(v), total(v * x), total(v * y)], 1).reshape(n, nregions, 3)
    return out


def brute_force(labels, nregions, frames, n, h, w):
    res = {"count": np.zeros((n, nregions), np.int32), "bbox": np.full((n, nregions, 4), -1, np.int32),
           "moments": np.zeros((n, nregions, 5), np.int64), "weighted": None if frames is None else np.zeros((n, nregions, 3), np.int64)}
    for f in range(n):
        for r in range(nregions):
            px = [(x, y) for y in range(h) for x in range(w) if (labels[f, y, x] if labels.ndim == 3 else labels[y, x]) == r]
            if not px:
                continue
            xs, ys = [p[0] for p in px], [p[1] for p in px]
            res["count"][f, r] = len(px)
            res["bbox"][f, r] = [min(xs), min(ys), max(xs), max(ys)]
            res["moments"][f, r] = [sum(xs), sum(ys), sum(x * x for x in xs), sum(x * y for x, y in px), sum(y * y for y in ys)]
            if frames is not None:
                vs = [int(frames[f, y, x]) for x, y in px]
                res["weighted"][f, r] = [sum(vs), sum(v * x for v, (x, y) in zip(vs, px)), sum(v * y for v, (x, y) in zip(vs, px))]
    return res


def random_case(seed, n, h, w, nregions, per_frame):
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 65536, (n, h, w)).astype(np.uint16)
    frames.reshape(n, -1)[:, ::5] = 65535
    labels = rng.integers(-2, nregions + 2, (n, h, w) if per_frame else (h, w)).astype(np.int32)  # below 0 and >= nregions: ignored
    return frames, labels


def same(got, exp, what=""):
    for k in FIELDS:
        if exp[k] is None:
            assert got[k] is None, (what, k)
            continue
        assert got[k].dtype == exp[k].dtype and got[k].shape == exp[k].shape, (what, k, got[k].dtype, got[k].shape)
        assert np.array_equal(got[k], exp[k]), (what, k)


@pytest.mark.parametrize("seed,n,h,w,nregions,per_frame", [(0, 1, 1, 1, 1, 0), (1, 2, 3, 5, 1, 0), (2, 3, 4, 7, 6, 0), (3, 3, 5, 3, 9, 1),
                                                           (4, 1, 6, 6, 40, 0), (5, 4, 2, 9, 3, 1), (6, 2, 7, 1, 5, 1), (7, 2, 7, 9, 4, 1)])
def test_oracle_matches_the_definition_pixel_by_pixel(seed, n, h, w, nregions, per_frame):
    frames, labels = random_case(seed, n, h, w, nregions, per_frame)
    got = region_geometry_oracle(labels, nregions, frames)
    same(got, brute_force(labels, nregions, frames, n, h, w), "weighted")
    assert got["count"].dtype == np.int32 and got["bbox"].dtype == np.int32 and got["moments"].dtype == np.int64 and got["weighted"].dtype == np.int64
    if nregions > 6:
        assert (got["count"] == 0).any()  # empty regions are covered
        assert (got["bbox"][got["count"] == 0] == -1).all() and not got["moments"][got["count"] == 0].any()
    # without frames: the label maps alone (a shared map is one map)
    m = n if per_frame else 1
    plain = region_geometry_oracle(labels, nregions)
    same(plain, brute_force(labels, nregions, None, m, h, w), "labels only")
    for k in ("count", "bbox", "moments"):
        assert np.array_equal(plain[k], got[k][:m] if not per_frame else got[k]), k


def test_oracle_largest_sums():
    """one region over a 2 x 32768 map of 65535: sum of x^2 of a row is 1.17e13, every field against the closed forms"""
    h, w = 2, 32768
    o = region_geometry_oracle(np.zeros((h, w), np.int32), 1, np.full((1, h, w), 65535, np.uint16))
    sx, sxx = w * (w - 1) // 2, (w - 1) * w * (2 * w - 1) // 6
    assert o["count"][0, 0] == h * w and o["bbox"][0, 0].tolist() == [0, 0, w - 1, 1]
    assert o["moments"][0, 0].tolist() == [2 * sx, w, 2 * sxx, sx, w]
    assert o["weighted"][0, 0].tolist() == [65535 * h * w, 65535 * 2 * sx, 65535 * w]


def test_entry_points_are_declared_and_exported(lib):
    dev = open(os.path.join(ROOT, "include", "rir_amd_device.h")).read()
    sp = open(os.path.join(ROOT, "include", "rir_amd_signal_processing.h")).read()
    flat = lambda s: re.sub(r"/\*.*?\*/", "", re.sub(r"\s+", " ", s))  # noqa: E731
    norm = lambda s: re.sub(r"\s+", " ", flat(s))  # noqa: E731
    assert ("int rir_region_geometry_device(const int *d_labels, const unsigned short *d_frames , int w, int h, int nframes, int labels_per_frame, "
            "int nregions, int *d_count, int *d_bbox, long long *d_moments, long long *d_weighted , void *d_work, size_t work_bytes, "
            "void *stream);") in norm(dev)
    assert "size_t rir_region_geometry_workspace_bytes(int w, int h, int nframes, int labels_per_frame, int nregions, int weighted);" in norm(dev)
    assert ("int rir_region_geometry(const int *labels, const unsigned short *frames , int w, int h, int nframes, int labels_per_frame, "
            "int nregions, int *count, int *bbox, long long *moments, long long *weighted );") in norm(sp)
    for name in ("rir_region_geometry_device", "rir_region_geometry_workspace_bytes", "rir_region_geometry"):
        assert hasattr(lib, name), name


def test_workspace_query(lib):
    f = lib.rir_region_geometry_workspace_bytes
    f.argtypes = [ct.c_int] * 6
    f.restype = ct.c_size_t
    for good in [(640, 512, 10, 0, 16, 1), (640, 512, 10, 1, 16, 0), (640, 512, 1, 0, 16, 0), (32768, 32768, 1, 0, 1 << 24, 1), (1, 1, 0, 0, 1, 1)]:
        assert f(*good) > 0, good
    for bad in [(0, 5, 1, 0, 1, 1), (5, 0, 1, 0, 1, 1), (32769, 5, 1, 0, 1, 1), (5, 32769, 1, 0, 1, 1), (65536, 32768, 1, 0, 1, 1),
                (46341, 46341, 1, 0, 1, 1), (5, 5, 1, 0, 0, 1), (5, 5, 1, 0, (1 << 24) + 1, 1), (5, 5, 1, 2, 1, 1), (5, 5, -1, 0, 1, 1),
                (5, 5, 1, 0, 1, 2), (5, 5, 3, 0, 1, 0)]:  # the last: several maps without weights need labels_per_frame 1
        assert f(*bad) == 0, bad


def test_no_cpu_fallback_without_device(lib):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from librir_amd.low_level.misc import last_error

    frames = np.arange(2 * 3 * 5, dtype=np.uint16).reshape(2, 3, 5)
    labels = np.zeros((3, 5), np.int32)
    outs = [np.zeros((2, 1), np.int32), np.zeros((2, 1, 4), np.int32), np.zeros((2, 1, 5), np.int64), np.zeros((2, 1, 3), np.int64)]
    lib.rir_region_geometry.argtypes = [ct.c_void_p, ct.c_void_p] + [ct.c_int] * 5 + [ct.c_void_p] * 4
    assert lib.rir_region_geometry(labels.ctypes.data, frames.ctypes.data, 5, 3, 2, 0, 1, *(o.ctypes.data for o in outs)) == -1
    assert "no usable HIP device" in last_error()
    assert not any(o.any() for o in outs)
    lib.rir_region_geometry_device.argtypes = [ct.c_void_p, ct.c_void_p] + [ct.c_int] * 5 + [ct.c_void_p] * 5 + [ct.c_size_t, ct.c_void_p]
    work = np.zeros(64, np.int64)
    assert lib.rir_region_geometry_device(labels.ctypes.data, frames.ctypes.data, 5, 3, 2, 0, 1, *(o.ctypes.data for o in outs), work.ctypes.data,
                                          work.nbytes, None) == -1
    assert "no usable HIP device" in last_error()
    assert not any(o.any() for o in outs)
    from librir_amd import signal_processing as S

    with pytest.raises(RuntimeError):
        S.region_geometry(labels, 1, frames)
    with pytest.raises(RuntimeError):
        S.region_geometry(labels, 1)


def test_python_api_exists():
    import inspect

    from librir_amd import device as D
    from librir_amd import signal_processing as S
    from librir_amd.video_io import IRMovie

    assert callable(D.region_geometry) and callable(S.region_geometry) and "region_geometry" in S.__all__
    assert list(inspect.signature(D.region_geometry).parameters) == ["labels", "nregions", "frames"]
    assert list(inspect.signature(S.region_geometry).parameters) == ["labels", "nregions", "frames"]
    assert D.RegionGeometry._fields == FIELDS
    for helper in ("centroid", "weighted_centroid", "covariance", "ellipse"):
        assert callable(getattr(D.RegionGeometry, helper)), helper
    assert list(inspect.signature(IRMovie.region_geometry).parameters)[1:] == ["labels", "selection", "nregions"]
    # the third element comes from a sibling of track_hot_spots, whose own parameters (pinned by test_track_components_cpu.py) stay
    p = inspect.signature(IRMovie.track_hot_spots_geometry).parameters
    assert list(p) == list(inspect.signature(IRMovie.track_hot_spots).parameters) and p["stats"].default is True


@pytest.mark.parametrize("labels_shape,labels_dtype,frames_shape,frames_dtype,nregions,exc", [
    ((4, 5), "int64", (2, 4, 5), "uint16", 3, RuntimeError),
    ((4, 5), "int32", (2, 4, 5), "int16", 3, RuntimeError),
    ((4, 5), "int32", (2, 4, 5), "float32", 3, RuntimeError),
    ((4, 5), "int64", None, None, 3, RuntimeError),
    ((5, 4), "int32", (2, 4, 5), "uint16", 3, ValueError),
    ((3, 4, 5), "int32", (2, 4, 5), "uint16", 3, ValueError),
    ((2, 4, 5, 1), "int32", (2, 4, 5), "uint16", 3, ValueError),
    ((2, 4, 5), "int32", (4, 5), "uint16", 3, ValueError),
    ((4, 5), "int32", (2, 2, 4, 5), "uint16", 3, ValueError),
    ((5,), "int32", None, None, 3, ValueError),
    ((1, 2, 4, 5), "int32", None, None, 3, ValueError),
    ((1, 32769), "int32", None, None, 3, ValueError),
    ((32769, 1), "int32", (32769, 1), "uint16", 3, ValueError),
    ((4, 5), "int32", (2, 4, 5), "uint16", 0, ValueError),
    ((4, 5), "int32", None, None, -3, ValueError),
    ((4, 5), "int32", (2, 4, 5), "uint16", (1 << 24) + 1, ValueError),
])
def test_python_checks_raise_without_a_device(labels_shape, labels_dtype, frames_shape, frames_dtype, nregions, exc):
    """CPU tensors: every check comes before any device work"""
    import torch

    from librir_amd import device as D
    from librir_amd import signal_processing as S

    lab = torch.zeros(labels_shape, dtype=getattr(torch, labels_dtype))
    fr = None if frames_shape is None else torch.zeros(frames_shape, dtype=getattr(torch, frames_dtype))
    with pytest.raises(exc):
        D.region_geometry(lab, nregions, fr)
    with pytest.raises(exc):
        S.region_geometry(np.zeros(labels_shape, getattr(np, labels_dtype)), nregions,
                          None if frames_shape is None else np.zeros(frames_shape, getattr(np, frames_dtype)))


def test_device_entry_refuses_cpu_tensors():
    import torch

    from librir_amd import device as D

    lab = torch.zeros((4, 5), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="CUDA"):
        D.region_geometry(lab, 3)
    with pytest.raises(RuntimeError, match="CUDA"):
        D.region_geometry(lab, 3, torch.zeros((2, 4, 5), dtype=torch.uint16))


# ---- the float64 helpers ---------------------------------------------------------------------------------------------------------------
# Tolerances: the covariance entries are within 4 * 2^-53 * (w^2 + h^2) of the exact value, 7.3e-10 for the 1024 x 768 maps used here, and a
# direct float64 computation on centred coordinates is far closer than that - abs 1e-8 for the covariance.  The eigenvalues l+- are a half
# sum and a root of such entries, so (axis / 4)^2 is compared at the same 1e-8; the axes themselves only after the square, because the root
# of a value near 0 magnifies its error.  The angle moves by about (error of an entry) / (l+ - l-): it is compared at 1e-6, modulo pi, where
# l+ - l- >= 0.01.

def direct(xs, ys):
    """centroid, covariance (cxx, cxy, cyy), eigenvalues (l+, l-) and angle from the pixel coordinates, centred first"""
    xs, ys = np.asarray(xs, np.float64), np.asarray(ys, np.float64)
    mx, my = xs.mean(), ys.mean()
    dx, dy = xs - mx, ys - my
    cxx, cxy, cyy = (dx * dx).mean(), (dx * dy).mean(), (dy * dy).mean()
    half, root = (cxx + cyy) / 2, math.hypot((cxx - cyy) / 2, cxy)
    return (mx, my), (cxx, cxy, cyy), (half + root, max(half - root, 0.0)), 0.5 * math.atan2(2 * cxy, cxx - cyy)


def helper_map():
    """768 x 1024, regions: 0 one pixel, 1 a horizontal line, 2 a vertical line, 3 a tilted band near the far corner, 4 a disc, 5 scattered
    pixels, 6 a diagonal of two pixels, 7 empty"""
    h, w = 768, 1024
    lab = np.full((h, w), -1, np.int32)
    yy, xx = np.mgrid[0:h, 0:w]
    lab[(np.abs((yy - 700) - 0.37 * (xx - 900)) < 6) & (xx > 800)] = 3
    lab[(yy - 300) ** 2 + (xx - 500) ** 2 <= 40 ** 2] = 4
    rng = np.random.default_rng(8)
    lab[rng.integers(0, h, 300), rng.integers(0, w, 300)] = 5
    lab[10, 1010], lab[11, 1011] = 6, 6
    lab[767, 1023] = 0
    lab[600, 17:430] = 1
    lab[5:760, 1001] = 2
    return lab


def as_geometry(o, to=lambda a: a):
    from librir_amd import device as D

    return D.RegionGeometry(*(None if o[k] is None else to(o[k]) for k in FIELDS))


@pytest.mark.parametrize("kind", ["numpy", "torch"])
def test_helpers_agree_with_a_direct_computation(kind):
    import torch

    lab = helper_map()
    rng = np.random.default_rng(3)
    frames = rng.integers(0, 65536, (2,) + lab.shape).astype(np.uint16)
    frames[1][lab == 4] = 0  # a region whose weights are all 0
    o = region_geometry_oracle(lab, 8, frames)
    g = as_geometry(o) if kind == "numpy" else as_geometry(o, torch.from_numpy)
    get = (lambda a: a) if kind == "numpy" else (lambda a: a.numpy())
    outs = [g.centroid(), g.weighted_centroid(), g.covariance(), g.ellipse()]
    for t, last in zip(outs, (2, 2, 3, 3)):
        assert (t.dtype == np.float64 if kind == "numpy" else t.dtype == torch.float64) and tuple(t.shape) == (2, 8, last)
    cen, wcen, cov, ell = (get(t) for t in outs)
    for f in range(2):
        for r in range(7):
            ys, xs = np.nonzero(lab == r)
            (mx, my), c, lam, ang = direct(xs, ys)
            assert cen[f, r] == pytest.approx([mx, my], rel=1e-14, abs=0)
            assert cov[f, r] == pytest.approx(c, rel=0, abs=1e-8), (r, cov[f, r], c)
            assert (ell[f, r, :2] / 4) ** 2 == pytest.approx(lam, rel=0, abs=1e-8), r
            if lam[0] - lam[1] >= 0.01:
                assert abs((ell[f, r, 2] - ang + math.pi / 2) % math.pi - math.pi / 2) < 1e-6, r
            v = frames[f][lab == r].astype(np.float64)
            if v.sum() > 0:
                assert wcen[f, r] == pytest.approx([(v * xs).sum() / v.sum(), (v * ys).sum() / v.sum()], rel=1e-12, abs=0)
            else:
                assert np.isnan(wcen[f, r]).all()
        # the one-pixel region, the lines and the empty region
        assert cen[f, 0].tolist() == [1023.0, 767.0] and cov[f, 0].tolist() == [0.0, 0.0, 0.0] and ell[f, 0].tolist() == [0.0, 0.0, 0.0]
        n1, n2 = 430 - 17, 760 - 5
        assert ell[f, 1, 0] == pytest.approx(4 * math.sqrt((n1 * n1 - 1) / 12), rel=1e-12) and ell[f, 1, 1] == 0.0 and ell[f, 1, 2] == 0.0
        assert ell[f, 2, 0] == pytest.approx(4 * math.sqrt((n2 * n2 - 1) / 12), rel=1e-12) and ell[f, 2, 1] == 0.0
        assert ell[f, 2, 2] == pytest.approx(math.pi / 2, rel=1e-15)
        assert ell[f, 6, 2] == pytest.approx(math.pi / 4, abs=1e-8)  # l+ - l- = 0.5: an entry's 7.3e-10 moves the angle by about 1.5e-9
        assert ell[f, 3, 2] == pytest.approx(math.atan(0.37), abs=0.02)  # the band's slope, from +x towards +y
        for t in (cen, cov, ell, wcen):
            assert np.isnan(t[f, 7]).all()
    assert np.isnan(wcen[1, 4]).all() and not np.isnan(wcen[0, 4]).any()


def test_weighted_centroid_needs_frames():
    o = region_geometry_oracle(helper_map(), 8)
    g = as_geometry(o)
    assert g.weighted is None and g.centroid().shape == (1, 8, 2)
    with pytest.raises(ValueError):
        g.weighted_centroid()


HIPCC_FOUND = os.path.exists(B.HIPCC) or shutil.which(B.HIPCC) is not None


@pytest.mark.skipif(not HIPCC_FOUND, reason="hipcc not found")
def test_geometry_kernels_use_no_scratch(tmp_path):
    """the five kernels (init, accumulate in LDS / global form, with and without weights) have no private segment"""
    asm = str(tmp_path / "geometry_kernels.s")
    flags = [f for f in B.COMMON if f != "-fPIC"]
    subprocess.check_call([B.HIPCC] + flags + ["-S", "--cuda-device-only", os.path.join(B.CSRC, "geometry_kernels.hip"), "-o", asm],
                          stderr=subprocess.DEVNULL)
    text = open(asm).read()
    meta = text[text.index("amdhsa.kernels:"):text.index(".end_amdgpu_metadata")]
    sizes = [int(m) for m in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", meta)]
    assert len(sizes) == 5 and all(v == 0 for v in sizes), sizes
