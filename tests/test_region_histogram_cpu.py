"""CPU: per-region histograms - the numpy oracle the GPU tests use, the entry points are declared and exported and refuse bad arguments
before a device is looked for, there is no CPU fallback, the Python API checks its arguments without a device, the reciprocal that replaces
the division is exact for every width, the kernels of histogram_kernels.hip use no scratch and no compare-and-swap loop, and the helpers
of the result (edges, mode, cumulative, otsu) on CPU tensors and numpy arrays."""
import ctypes as ct
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from librir_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(B.CSRC, "histogram_kernels.h")).read()


def region_histogram_oracle(frames, labels, k, lo, width, nbins, rows=None):
    """the contract with np.bincount: per frame the counted pixels with a label in [0, k) go to slot (v - lo) // width of their region, to
    a slot below for v < lo and one above for v >= lo + nbins * width.  labels None: one region.
    -> (count [n][k], hist [n][k][nbins], outside [n][k][2]), int32"""
    frames = np.asarray(frames)
    if frames.ndim == 2:
        frames = frames[None]
    n, h, w = frames.shape
    rows = h if rows is None else rows
    lab = np.zeros((h, w), np.int64) if labels is None else np.asarray(labels, np.int64)
    lab = np.broadcast_to(lab, (n, h, w))[:, :rows].reshape(n, -1)
    v = frames[:, :rows].reshape(n, -1).astype(np.int64)
    slot = np.where(v < lo, 0, np.minimum((v - lo) // width, nbins) + 1)  # 0: below, 1 .. nbins: the bins, nbins + 1: above
    count = np.zeros((n, k), np.int32)
    hist = np.zeros((n, k, nbins), np.int32)
    outside = np.zeros((n, k, 2), np.int32)
    for f in range(n):
        keep = (lab[f] >= 0) & (lab[f] < k)
        c = np.bincount(lab[f][keep] * (nbins + 2) + slot[f][keep], minlength=k * (nbins + 2)).reshape(k, nbins + 2)
        hist[f], outside[f, :, 0], outside[f, :, 1] = c[:, 1:-1], c[:, 0], c[:, -1]
        count[f] = c.sum(1)
    return count, hist, outside


def test_oracle_on_a_case_counted_by_hand():
    f = np.array([[[0, 5, 9, 10], [14, 15, 19, 20], [65535, 7, 12, 3]]], np.uint16)
    lab = np.array([[0, 0, 1, 1], [0, 1, 1, -1], [2, 0, 0, 0]], np.int32)
    count, hist, outside = region_histogram_oracle(f, lab, 2, 5, 5, 3)  # bins [5, 10) [10, 15) [15, 20)
    assert count.tolist() == [[6, 4]] and hist.tolist() == [[[2, 2, 0], [1, 1, 2]]] and outside.tolist() == [[[2, 0], [0, 0]]]
    count, hist, outside = region_histogram_oracle(f, lab, 2, 5, 5, 3, rows=2)  # the third row holds valid labels and does not count
    assert count.tolist() == [[3, 4]] and hist.tolist() == [[[1, 1, 0], [1, 1, 2]]] and outside.tolist() == [[[1, 0], [0, 0]]]
    count, hist, outside = region_histogram_oracle(f, None, 1, 10, 10, 1)
    assert count.tolist() == [[12]] and hist.tolist() == [[[5]]] and outside.tolist() == [[[5, 2]]]
    count, hist, outside = region_histogram_oracle(f, None, 1, 65535, 1, 1, rows=0)
    assert not count.any() and not hist.any() and not outside.any()


DEVICE_ARGS = [ct.c_void_p, ct.c_void_p] + [ct.c_int] * 9 + [ct.c_void_p] * 4 + [ct.c_size_t, ct.c_void_p]
HOST_ARGS = [ct.c_void_p, ct.c_void_p] + [ct.c_int] * 9 + [ct.c_void_p] * 3


def test_entry_points_are_declared_and_exported(lib):
    dev = open(os.path.join(ROOT, "include", "rir_amd_device.h")).read()
    sp = open(os.path.join(ROOT, "include", "rir_amd_signal_processing.h")).read()
    assert re.search(r"int rir_region_histogram_device\(const unsigned short \*d_frames, const int \*d_labels /\* or null \*/, int w, int h, int rows, "
                     r"int nframes,\s+int labels_per_frame, int nregions, int lo, int width, int nbins, int \*d_count /\* or null \*/, int \*d_hist,\s+"
                     r"int \*d_outside /\* or null \*/, void \*d_work, size_t work_bytes, void \*stream\);", dev)
    assert re.search(r"size_t rir_region_histogram_workspace_bytes\(int w, int h, int rows, int nframes, int labels_per_frame, int nregions, int nbins\);",
                     dev)
    assert re.search(r"int rir_region_histogram\(const unsigned short \*frames, const int \*labels /\* or null \*/, int w, int h, int rows, int nframes,\s+"
                     r"int labels_per_frame, int nregions, int lo, int width, int nbins, int \*count /\* or null \*/, int \*hist,\s+"
                     r"int \*outside /\* or null \*/\);", sp)
    for name in ("rir_region_histogram_device", "rir_region_histogram_workspace_bytes", "rir_region_histogram"):
        assert hasattr(lib, name), name
    for name in ("HISTOGRAM_LDS_MAX", "HISTOGRAM_COPY_MAX", "HISTOGRAM_MAX_COPIES"):
        assert re.search(r"constexpr int %s = \d+;" % name, HEADER), name


def test_workspace_query(lib):
    f = lib.rir_region_histogram_workspace_bytes
    f.argtypes = [ct.c_int] * 7
    f.restype = ct.c_size_t
    for good in [(640, 512, 512, 1000, 0, 16, 256), (640, 512, 0, 0, 1, 1, 65536), (1, 1, 1, 1, 0, 65536, 256), (80, 64, 61, 3, 1, 256, 65536)]:
        assert 0 < f(*good) <= 64 and f(*good) % 8 == 0, good
    for bad in [(0, 5, 1, 1, 0, 1, 1), (5, 0, 0, 1, 0, 1, 1), (5, 5, -1, 1, 0, 1, 1), (5, 5, 6, 1, 0, 1, 1), (5, 5, 5, -1, 0, 1, 1), (5, 5, 5, 1, 2, 1, 1),
                (5, 5, 5, 1, 0, 0, 1), (5, 5, 5, 1, 0, 65537, 1), (5, 5, 5, 1, 0, 1, 0), (5, 5, 5, 1, 0, 1, 65537), (5, 5, 5, 1, 0, 257, 65536),
                (65536, 32768, 1, 1, 0, 1, 1)]:
        assert f(*bad) == 0, bad


def calls(lib):
    """(device entry, host entry) over good arguments in host memory, each taking overrides by name"""
    frames = np.arange(2 * 3 * 5, dtype=np.uint16).reshape(2, 3, 5)
    labels = np.zeros((3, 5), np.int32)
    out = {"count": np.full((2, 2), 7, np.int32), "hist": np.full((2, 2, 4), 7, np.int32), "outside": np.full((2, 2, 2), 7, np.int32),
           "work": np.zeros(2, np.int64)}
    good = dict(fr=frames.ctypes.data, lab=labels.ctypes.data, w=5, h=3, rows=3, n=2, per=0, k=2, lo=0, width=8, nbins=4, count=out["count"].ctypes.data,
                hist=out["hist"].ctypes.data, outside=out["outside"].ctypes.data, work=out["work"].ctypes.data, wb=16)
    lib.rir_region_histogram_device.argtypes = DEVICE_ARGS
    lib.rir_region_histogram.argtypes = HOST_ARGS
    names = ("fr", "lab", "w", "h", "rows", "n", "per", "k", "lo", "width", "nbins", "count", "hist", "outside")

    def device(**kw):
        a = dict(good, **kw)
        return lib.rir_region_histogram_device(*(a[x] for x in names + ("work", "wb")), None)

    def host(**kw):
        a = dict(good, **kw)
        return lib.rir_region_histogram(*(a[x] for x in names))

    return device, host, out, (frames, labels)


BAD = [dict(w=0), dict(h=0), dict(rows=-1), dict(rows=4), dict(n=-1), dict(per=2), dict(per=-1), dict(k=0), dict(k=65537), dict(lo=-1), dict(lo=65536),
       dict(width=0), dict(width=65537), dict(nbins=0), dict(nbins=65537), dict(k=257, nbins=65536), dict(w=65536, h=32768),
       dict(lab=None, k=2), dict(lab=None, k=1, per=1)]


def test_bad_arguments_are_refused_before_the_device_is_looked_for(lib):
    """every bound of the contract, null pointers and overlaps: -1 with the entry's own reason, never "no usable HIP device", and nothing
    written - on a machine without a device as on one with"""
    from librir_amd.low_level.misc import last_error

    device, host, out, (frames, labels) = calls(lib)
    for fn in (device, host):
        for kw in BAD:
            assert fn(**kw) == -1, kw
            assert "invalid argument" in last_error() and "HIP device" not in last_error(), (kw, last_error())
        for null in ("fr", "hist"):
            assert fn(**{null: None}) == -1 and "null pointer" in last_error(), null
    assert device(work=None) == -1 and "null pointer" in last_error()
    assert device(wb=7) == -1 and "workspace" in last_error()
    assert device(work=out["work"].ctypes.data + 4) == -1 and "workspace" in last_error()
    for kw in (dict(count=out["hist"].ctypes.data + 8), dict(outside=out["hist"].ctypes.data), dict(hist=frames.ctypes.data),
               dict(work=out["count"].ctypes.data), dict(count=labels.ctypes.data)):
        assert device(**kw) == -1 and "overlap" in last_error(), kw
    assert all((a == 7).all() for name, a in out.items() if name != "work") and not out["work"].any()
    for fn in (device, host):
        assert fn(n=0) == 0  # nothing to do, with or without a device


def test_no_cpu_fallback_without_device(lib):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from librir_amd.low_level.misc import last_error

    device, host, out, (frames, labels) = calls(lib)
    for fn in (host, device):
        for kw in (dict(), dict(lab=None, k=1), dict(count=None, outside=None), dict(rows=0)):
            assert fn(**kw) == -1, kw
            assert "no usable HIP device" in last_error()
    assert all((a == 7).all() for name, a in out.items() if name != "work") and not out["work"].any()
    from librir_amd import signal_processing as S

    with pytest.raises(RuntimeError):
        S.region_histogram(frames, labels, 4, 0, 8, 2)
    with pytest.raises(RuntimeError):
        S.region_histogram(frames, None, 4)


def test_python_api_exists():
    from librir_amd import device as D
    from librir_amd import signal_processing as S
    from librir_amd.video_io import IRMovie

    assert callable(D.region_histogram) and callable(D.histogram) and callable(S.region_histogram) and "region_histogram" in S.__all__
    assert D.RegionHistogram._fields == ("count", "hist", "outside", "lo", "width")
    assert list(inspect.signature(D.region_histogram).parameters) == ["frames", "labels", "nbins", "lo", "width", "nregions", "rows"]
    assert list(inspect.signature(D.histogram).parameters) == ["frames", "nbins", "lo", "width", "rows"]
    assert list(inspect.signature(S.region_histogram).parameters) == ["images", "labels", "nbins", "lo", "width", "nregions", "rows"]
    params = inspect.signature(IRMovie.region_histogram).parameters
    assert list(params)[1:] == ["labels", "nbins", "lo", "width", "selection", "nregions", "rows"]
    assert params["selection"].default == slice(None) and params["nregions"].default is None and params["rows"].default is None
    assert list(inspect.signature(IRMovie.histogram).parameters)[1:] == ["nbins", "lo", "width", "selection", "rows"]
    assert list(inspect.signature(IRMovie.background_levels).parameters)[1:] == ["selection", "rows"]
    for name in ("_region_histogram_args", "_region_histogram_empty", "_region_histogram_into"):
        assert callable(getattr(D, name)), name


@pytest.mark.parametrize("frames_shape,labels_shape,kw", [
    ((2, 4, 5), (5, 4), dict(nbins=4)),
    ((2, 4, 5), (3, 4, 5), dict(nbins=4)),
    ((4, 5), (2, 4, 5), dict(nbins=4)),
    ((2, 2, 4, 5), (4, 5), dict(nbins=4)),
    ((2, 4, 5), (4, 5), dict(nbins=4, nregions=0)),
    ((2, 4, 5), (4, 5), dict(nbins=4, nregions=65537)),
    ((2, 4, 5), (4, 5), dict(nbins=65536, nregions=257)),
    ((2, 4, 5), (4, 5), dict(nbins=0)),
    ((2, 4, 5), (4, 5), dict(nbins=65537)),
    ((2, 4, 5), (4, 5), dict(nbins=4.0)),
    ((2, 4, 5), (4, 5), dict(nbins=4, lo=-1)),
    ((2, 4, 5), (4, 5), dict(nbins=4, lo=65536)),
    ((2, 4, 5), (4, 5), dict(nbins=4, width=0)),
    ((2, 4, 5), (4, 5), dict(nbins=4, width=65537)),
    ((2, 4, 5), (4, 5), dict(nbins=4, width=1.5)),
    ((2, 4, 5), (4, 5), dict(nbins=4, rows=-1)),
    ((2, 4, 5), (4, 5), dict(nbins=4, rows=5)),
    ((2, 4, 5), None, dict(nbins=4, nregions=2)),
    ((2, 4, 5), None, dict(nbins=4, rows=5)),
])
def test_args_reject_bad_shapes_and_bins_without_a_device(frames_shape, labels_shape, kw):
    import torch

    from librir_amd import device as D
    from librir_amd import signal_processing as S

    with pytest.raises(ValueError):
        D._region_histogram_args(frames_shape, labels_shape, **kw)
    fr = torch.zeros(frames_shape, dtype=torch.uint16)
    lab = None if labels_shape is None else torch.zeros(labels_shape, dtype=torch.int32)
    k = dict(kw)
    k.setdefault("nregions", 3 if lab is not None else None)
    with pytest.raises(ValueError):
        D.region_histogram(fr, lab, **k)
    with pytest.raises(ValueError):
        S.region_histogram(fr.numpy(), None if lab is None else lab.numpy(), **k)
    if lab is None:
        k.pop("nregions")
        if "rows" in kw:
            with pytest.raises(ValueError):
                D.histogram(fr, **k)


def test_args_accept_the_corners():
    from librir_amd import device as D

    assert D._region_histogram_args((2, 4, 5), (4, 5), 65536, 65535, 65536, 256, 0) == (2, 4, 5, 0, 65536, 65535, 65536, 0)
    assert D._region_histogram_args((4, 5), (4, 5), np.int64(7), rows=None) == (1, 4, 5, 0, 7, 0, 1, 4)
    assert D._region_histogram_args((3, 4, 5), (3, 4, 5), 1, nregions=65536) == (3, 4, 5, 1, 1, 0, 1, 4)
    assert D._region_histogram_args((3, 4, 5), None, 65536, 0, 1, None, 2) == (3, 4, 5, 0, 65536, 0, 1, 2)


def test_dtypes_and_cpu_tensors_are_refused():
    import torch

    from librir_amd import device as D
    from librir_amd import signal_processing as S

    f16, lab = torch.zeros((2, 4, 5), dtype=torch.uint16), torch.zeros((4, 5), dtype=torch.int32)
    for fr, lb in ((f16.to(torch.int16), lab), (f16.float(), lab), (f16, lab.long())):
        with pytest.raises(RuntimeError):
            D.region_histogram(fr, lb, 4, nregions=1)
        with pytest.raises(RuntimeError):
            S.region_histogram(fr.numpy(), lb.numpy(), 4, nregions=1)
    with pytest.raises(RuntimeError):
        D.histogram(f16.float(), 4)
    with pytest.raises(RuntimeError, match="CUDA"):
        D.region_histogram(f16, lab, 4, nregions=1)
    with pytest.raises(RuntimeError, match="CUDA"):
        D.histogram(f16, 4)


def test_the_reciprocal_is_exact_for_every_width():
    """the formula of histogram_div_magic, read from the header and restated: for every width 1..65536 the multiply-high equals v // width at
    both sides of every multiple of the width within 16 bits (1.5 M points) - and a power of two shifts"""
    assert re.search(r"constexpr uint32_t histogram_div_magic\(int width\) \{ return \(width & \(width - 1\)\) \? "
                     r"\(uint32_t\)\(0x100000000ull / \(uint32_t\)width\) \+ 1u : 0u; \}", HEADER)
    checked = 0
    for width in range(1, 65537):
        k = np.arange(0, 65535 // width + 2, dtype=np.uint64)
        v = np.concatenate([k * width, k[1:] * width - 1])
        v = v[v <= 65535]
        if width & (width - 1):
            magic = np.uint64((1 << 32) // width + 1)
            assert magic < 1 << 32
            q = (v * magic) >> np.uint64(32)
        else:
            q = v >> np.uint64(width.bit_length() - 1)
        assert np.array_equal(q, v // np.uint64(width)), width
        checked += v.size
    assert checked > 1400000


def helpers_case(xp):
    hist = np.zeros((2, 3, 8), np.int32)
    hist[0, 0] = [0, 5, 2, 5, 0, 5, 1, 0]  # three equally full bins: the lowest is 1
    hist[0, 1] = [0, 0, 0, 0, 0, 0, 0, 9]  # one occupied bin
    hist[1, 0] = [4, 6, 0, 0, 0, 3, 7, 2]  # two clusters: bins 0-1 and 5-7
    hist[1, 2] = [1, 0, 0, 0, 0, 0, 0, 1]  # two occupied bins at the ends
    count = hist.sum(-1).astype(np.int32)
    from librir_amd import device as D

    return D.RegionHistogram(xp(count), xp(hist), xp(np.zeros((2, 3, 2), np.int32)), 100, 10), hist


@pytest.mark.parametrize("kind", ["numpy", "torch"])
def test_helpers_of_the_result(kind):
    import torch

    r, hist = helpers_case((lambda a: a) if kind == "numpy" else torch.from_numpy)
    back = (lambda a: a) if kind == "numpy" else (lambda t: t.numpy())
    edges = back(r.edges())
    assert edges.dtype == np.int64 and edges.tolist() == list(range(100, 181, 10))
    mode = back(r.mode())
    assert mode.dtype == np.int32 and mode.tolist() == [[1, 7, -1], [6, -1, 0]]
    cum = back(r.cumulative())
    assert cum.dtype == np.int64 and np.array_equal(cum, np.cumsum(hist.astype(np.int64), -1))
    otsu = back(r.otsu())
    assert otsu.dtype == np.float64 and otsu.shape == (2, 3)
    assert otsu[0, 1] == -1 and otsu[0, 2] == -1 and otsu[1, 1] == -1  # one occupied bin, or none
    assert 1 <= otsu[1, 0] <= 4 and otsu[1, 0] == 1  # between the clusters, and the lowest of the equal ones
    assert otsu[1, 2] == 0
    # against the definition, bin by bin, in rational-free integer arithmetic scaled by the class sizes
    for f, k in ((0, 0), (1, 0), (1, 2)):
        h = hist[f, k].astype(object)
        best, at = -1, -1
        for t in range(7):
            w0, w1 = sum(h[:t + 1]), sum(h[t + 1:])
            if w0 == 0 or w1 == 0:
                continue
            m0, m1 = sum(b * h[b] for b in range(t + 1)), sum(b * h[b] for b in range(t + 1, 8))
            score = (m0 * w1 - m1 * w0) ** 2 * 1000000 // (w0 * w1)  # w0 * w1 * (mean0 - mean1)^2
            if score > best:
                best, at = score, t
        assert otsu[f, k] == at, (f, k)


def test_mode_of_wide_counts_and_a_single_bin():
    from librir_amd import device as D

    hist = np.array([[[327680]], [[0]]], np.int32)
    r = D.RegionHistogram(hist[..., 0], hist, np.zeros((2, 1, 2), np.int32), 0, 65536)
    assert r.mode().tolist() == [[0], [-1]] and r.otsu().tolist() == [[-1.0], [-1.0]] and r.edges().tolist() == [0, 65536]


HIPCC_FOUND = os.path.exists(B.HIPCC) or shutil.which(B.HIPCC) is not None


@pytest.mark.skipif(not HIPCC_FOUND, reason="hipcc not found")
def test_histogram_kernels_use_no_scratch_and_no_cmpswap(tmp_path):
    """exact, order-free counting with native 32-bit atomic adds only: no compare-and-swap loop, no private segment, by the compiler's own
    resource report and by the metadata of the code object"""
    asm = str(tmp_path / "histogram_kernels.s")
    flags = [f for f in B.COMMON if f != "-fPIC"]
    done = subprocess.run([B.HIPCC] + flags + ["-Rpass-analysis=kernel-resource-usage", "-S", "--cuda-device-only",
                                               os.path.join(B.CSRC, "histogram_kernels.hip"), "-o", asm], stderr=subprocess.PIPE, text=True, check=True)
    report = re.findall(r"Function Name: (\S+)|ScratchSize \[bytes/lane\]: (\d+)", done.stderr)
    names = [a for a, _ in report if a]
    scratch = [int(b) for _, b in report if b]
    assert len([x for x in names if "region_histogram_count" in x]) == 2 and len(scratch) == len(names) and not any(scratch), done.stderr
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
    assert len([k for k in kernels if "region_histogram_count" in k]) == 2, sorted(kernels)
    assert all(v == 0 for v in kernels.values()), kernels
