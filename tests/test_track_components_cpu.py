"""CPU: components tracked through time - the numpy oracle the GPU tests use agrees with a brute-force restatement of the definition and,
on boolean stacks, with scipy's 3-D labelling; the entry points are declared and exported and refuse bad arguments, there is no CPU
fallback, the Python API checks its arguments without a device, and the kernels of track_kernels.hip use no scratch."""
import ctypes as ct
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import track_cases as TC
from librir_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = ("track_of", "info", "tracks") + TC.TABLES


@pytest.mark.parametrize("seed,n,h,w,nlabels,with_counts,table", [
    (0, 1, 1, 1, 1, True, 1), (1, 1, 2, 3, 4, True, 3), (2, 2, 3, 5, 4, True, 9), (3, 3, 4, 7, 6, False, 16), (4, 5, 2, 2, 3, True, 2),
    (5, 4, 3, 3, 2, True, 5), (6, 6, 1, 9, 5, False, 25), (7, 3, 5, 1, 8, True, 1), (8, 7, 3, 4, 3, True, 15)])
def test_oracle_matches_the_definition_on_tiny_stacks(seed, n, h, w, nlabels, with_counts, table):
    labels, counts = TC.random_labels(seed, n, h, w, nlabels, with_counts)
    labels.reshape(-1)[::2] = np.random.default_rng(seed).integers(1, max(2, nlabels), labels.reshape(-1)[::2].shape)  # enough links
    got = TC.track_oracle(labels, counts, nlabels, table)
    exp = TC.brute_force(labels, counts, nlabels, table)
    for k in OUTPUTS:
        assert got[k].dtype == np.int32 and got[k].shape == exp[k].shape, k
        assert np.array_equal(got[k], exp[k]), (k, got[k], exp[k])
    assert got["volume"].sum() == labels.size and len(got["volume"]) == got["info"][0]


def test_oracle_on_a_scene_worked_by_hand():
    """frame 0: components 1 and 2; frame 1: one component over both; frame 2: nothing; frame 3: one component.  K = 3 (frame 1's
    count 2, frame 3's count 5 > K: its components 3 and 4 are dropped, its component 2 exists without a pixel)"""
    labels = np.array([[[1, 0, 2]], [[1, 1, 1]], [[0, 0, 0]], [[1, 4, 3]]], np.int32)
    counts = np.array([3, 2, 1, 5], np.int32)
    o = TC.track_oracle(labels, counts, 3, 8)
    assert o["track_of"].tolist() == [[0, 1, 1], [0, 1, 0], [0, 0, 0], [0, 2, 3]]
    assert o["info"].tolist() == [4, 1]
    assert o["first_frame"].tolist() == [-1, 0, 3, 3, 0, 0, 0, 0] and o["last_frame"].tolist() == [-1, 1, 3, 3, 0, 0, 0, 0]
    assert o["first_label"].tolist() == [0, 1, 1, 2, 0, 0, 0, 0] and o["components"].tolist() == [0, 3, 1, 1, 0, 0, 0, 0]
    assert o["tracks"].tolist() == [[[1, 0, 1]], [[1, 1, 1]], [[0, 0, 0]], [[2, 0, 0]]]
    short = TC.track_oracle(labels, counts, 3, 2)
    assert short["info"].tolist() == [4, 1] and short["first_frame"].tolist() == [-1, 0] and short["components"].tolist() == [0, 3]


@pytest.mark.parametrize("n,h,w", TC.RANDOM_SHAPES)
def test_oracle_track_map_is_scipys_3d_labelling(n, h, w):
    """boolean stacks labelled per frame with the 4-neighbour structure: the track map equals the 3-D labelling (4-connectivity inside a
    frame, the same pixel in adjacent frames) element for element"""
    ndi = pytest.importorskip("scipy.ndimage")
    mask = TC.random_mask(n * 1000 + w, n, h, w)
    cross = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    labels = np.zeros((n, h, w), np.int32)
    counts = np.zeros(n, np.int32)
    for t in range(n):
        labels[t], c = ndi.label(mask[t], cross)
        counts[t] = c + 1
    structure = np.zeros((3, 3, 3), int)
    structure[1] = cross
    structure[:, 1, 1] = 1
    exp, ntracks = ndi.label(mask, structure)
    got = TC.track_oracle(labels, counts, int(counts.max()))
    assert got["info"].tolist() == [ntracks + 1, 0]
    assert np.array_equal(got["tracks"], exp)
    assert np.array_equal(TC.track_oracle(labels, None, int(counts.max()), 1)["tracks"] > 0, mask)


def test_entry_points_are_declared_and_exported(lib):
    dev = open(os.path.join(ROOT, "include", "rir_amd_device.h")).read()
    assert re.search(r"int rir_track_components_device\(const int \*d_labels, const int \*d_counts, int w, int h, int nframes, int nlabels, "
                     r"int \*d_track_of, int \*d_info,\s+int \*d_first_frame, int \*d_last_frame, int \*d_first_label, int \*d_components, "
                     r"int table_entries, int \*d_dst,\s+void \*d_work, size_t work_bytes, void \*stream\);", dev)
    assert re.search(r"size_t rir_track_components_workspace_bytes\(int w, int h, int nframes, int nlabels\);", dev)
    for name in ("rir_track_components_device", "rir_track_components_workspace_bytes"):
        assert hasattr(lib, name), name
    assert not hasattr(lib, "rir_track_components")  # label maps are born on the device: there is no host-pointer entry


def test_workspace_query(lib):
    f = lib.rir_track_components_workspace_bytes
    f.argtypes = [ct.c_int] * 4
    f.restype = ct.c_size_t

    def up(b):
        return (b + 63) // 64 * 64

    def expect(n, k):
        nodes = n * k
        blocks = (nodes + 255) // 256
        return 2 * up(nodes * 4) + up(blocks * 4 * 8) + up(blocks * 4 * 4) + up(blocks * 4) + 64

    assert f(640, 512, 1000, 329) == expect(1000, 329)
    assert f(1, 1, 1, 1) == expect(1, 1) == 64 * 6
    assert f(5, 5, 0, 7) == 64  # no frame: nothing but the alignment slack, and not a refusal
    assert f(65536, 32767, 1, 1) == expect(1, 1)  # w * h = 0x7FFF0000
    assert f(1, 1, 0x7FFF, 0x10000) == expect(0x7FFF, 0x10000)  # n * K = 0x7FFF0000
    for bad in [(0, 5, 1, 1), (5, 0, 1, 1), (-1, 5, 1, 1), (5, 5, -1, 1), (5, 5, 1, 0), (5, 5, 1, -3), (65536, 32768, 1, 1), (1, 1, 0x7FFF, 0x10001),
                (1, 1, 0x7FFF0001, 1)]:
        assert f(*bad) == 0, bad


def test_no_cpu_fallback_without_device(lib):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from librir_amd.low_level.misc import last_error

    labels = np.ones((2, 3, 5), np.int32)
    track_of = np.zeros((2, 2), np.int32)
    info = np.zeros(2, np.int32)
    tables = [np.zeros(3, np.int32) for _ in range(4)]
    dst = np.zeros((2, 3, 5), np.int32)
    work = np.zeros(256, np.int64)
    fn = lib.rir_track_components_device
    fn.argtypes = [ct.c_void_p, ct.c_void_p] + [ct.c_int] * 4 + [ct.c_void_p] * 6 + [ct.c_int, ct.c_void_p, ct.c_void_p, ct.c_size_t, ct.c_void_p]
    assert fn(labels.ctypes.data, None, 5, 3, 2, 2, track_of.ctypes.data, info.ctypes.data, *(t.ctypes.data for t in tables), 3, dst.ctypes.data,
              work.ctypes.data, work.nbytes, None) == -1
    assert "no usable HIP device" in last_error()
    assert not track_of.any() and not info.any() and not dst.any() and not any(t.any() for t in tables)


def test_python_api_exists():
    from librir_amd import device as D
    from librir_amd import synthetic
    from librir_amd.video_io import IRMovie

    assert D.ComponentTracks._fields == ("tracks", "track_of", "ntracks", "truncated", "first_frame", "last_frame", "first_label", "components")
    params = inspect.signature(D.track_components).parameters
    assert list(params) == ["labels", "counts", "nlabels", "table_entries", "relabel", "out"]
    assert [params[k].default for k in list(params)[1:]] == [None, None, None, True, None]
    params = inspect.signature(IRMovie.track_hot_spots).parameters
    assert list(params)[1:] == ["threshold", "selection", "table_entries", "stats"]
    assert params["selection"].default == slice(None) and params["table_entries"].default is None and params["stats"].default is True
    assert list(inspect.signature(synthetic.hot_spots).parameters) == ["n", "h", "w", "seed"]


def test_hot_spots_scene_has_structure():
    """values <= 16 383, deterministic, and above a level between background and blobs: tracks that are born after the first frame, die
    before the last, and hold more components than frames they live (a split) or join two components of one frame (a merge)"""
    ndi = pytest.importorskip("scipy.ndimage")
    from librir_amd.synthetic import hot_spots

    f = hot_spots(40, 48, 64, 3)
    assert f.dtype == np.uint16 and f.shape == (40, 48, 64) and f.max() <= 16383 and np.array_equal(f, hot_spots(40, 48, 64, 3))
    mask = f > 4000
    labels = np.zeros(f.shape, np.int32)
    counts = np.zeros(40, np.int32)
    for t in range(40):
        labels[t], c = ndi.label(mask[t])
        counts[t] = c + 1
    o = TC.track_oracle(labels, counts, int(counts.max()))
    nt = o["info"][0]
    assert nt >= 3 and counts.max() >= 3
    assert (o["first_frame"][1:nt] > 0).any() and (o["last_frame"][1:nt] < 39).any()
    assert (o["components"][1:nt] > o["last_frame"][1:nt] - o["first_frame"][1:nt] + 1).any()


@pytest.mark.parametrize("labels_shape,labels_dtype,counts_shape,counts_dtype,nlabels,table,kw,exc", [
    ((2, 4, 5), "int64", None, None, 3, None, {}, RuntimeError),
    ((2, 4, 5), "uint16", None, None, 3, None, {}, RuntimeError),
    ((2, 4, 5), "float32", None, None, 3, None, {}, RuntimeError),
    ((2, 4, 5), "int32", (2,), "int64", 3, None, {}, RuntimeError),
    ((4, 5), "int32", None, None, 3, None, {}, ValueError),
    ((2, 2, 4, 5), "int32", None, None, 3, None, {}, ValueError),
    ((2, 0, 5), "int32", None, None, 3, None, {}, ValueError),
    ((2, 4, 5), "int32", (3,), "int32", 3, None, {}, ValueError),
    ((2, 4, 5), "int32", (2, 1), "int32", 3, None, {}, ValueError),
    ((2, 4, 5), "int32", None, None, 0, None, {}, ValueError),
    ((2, 4, 5), "int32", None, None, -2, None, {}, ValueError),
    ((2, 4, 5), "int32", None, None, 2.5, None, {}, ValueError),
    ((2, 4, 5), "int32", None, None, 0x7FFF0000 // 2 + 1, None, {}, ValueError),
    ((2, 4, 5), "int32", None, None, 3, 0, {}, ValueError),
    ((2, 4, 5), "int32", None, None, 3, -1, {}, ValueError),
    ((2, 4, 5), "int32", None, None, 3, None, {"relabel": False, "out": (2, 4, 5)}, ValueError),
    ((2, 4, 5), "int32", None, None, 3, None, {"out": (2, 5, 4)}, RuntimeError),
    ((2, 4, 5), "int32", None, None, 3, None, {}, RuntimeError),  # everything in order but the device: "CUDA"
])
def test_python_checks_raise_without_a_device(labels_shape, labels_dtype, counts_shape, counts_dtype, nlabels, table, kw, exc):
    """CPU tensors: every check comes before any device work"""
    import torch

    from librir_amd import device as D

    labels = torch.zeros(labels_shape, dtype=getattr(torch, labels_dtype))
    counts = None if counts_shape is None else torch.ones(counts_shape, dtype=getattr(torch, counts_dtype))
    kw = dict(kw)
    if "out" in kw:
        kw["out"] = torch.zeros(kw["out"], dtype=torch.int32)
    with pytest.raises(exc, match="track_components"):
        D.track_components(labels, counts, nlabels, table, **kw)


HIPCC_FOUND = os.path.exists(B.HIPCC) or shutil.which(B.HIPCC) is not None


@pytest.mark.skipif(not HIPCC_FOUND, reason="hipcc not found")
def test_track_kernels_use_no_scratch(tmp_path):
    asm = str(tmp_path / "track_kernels.s")
    flags = [f for f in B.COMMON if f != "-fPIC"]
    subprocess.check_call([B.HIPCC] + flags + ["-S", "--cuda-device-only", os.path.join(B.CSRC, "track_kernels.hip"), "-o", asm],
                          stderr=subprocess.DEVNULL)
    text = open(asm).read()
    assert "global_atomic_smin" in text  # the forest's links move by atomicMin
    meta = text[text.index("amdhsa.kernels:"):text.index(".end_amdgpu_metadata")]
    kernels = {}
    for block in re.split(r"\n  - ", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            kernels[name.group(1)] = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1))
    for stage in ("init", "link", "flatten", "scan", "number", "relabel"):
        assert len([k for k in kernels if "track_%s_kernel" % stage in k]) == 1, (stage, sorted(kernels))
    assert len(kernels) == 6, sorted(kernels)
    assert all(v == 0 for v in kernels.values()), kernels
