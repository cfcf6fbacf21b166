"""CPU: local window statistics - the numpy reference the GPU tests use (local_cases.py) agrees with scipy's correlate with mode="nearest",
the products of the z-score test stay inside int64 at the extremes of the parameters, the entry points are declared and exported, every
refused argument is refused without a device and in the recorded words (tests/golden/local_stats_messages.json), there is no CPU fallback,
the Python forms exist and check their parameters without a device, and the kernels of local_kernels.hip use no scratch and no LDS.

``PYTHONPATH=. python tests/test_local_stats_cpu.py`` writes the record of the messages anew from the library as it is."""
import ctypes as ct
import inspect
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from librir_amd import build as B
from local_cases import DELTA_MAX, INT64_MAX, K_DEN_MAX, K_NUM_MAX, checkerboard, largest_products, reference_mask, reference_mean, reference_sums
from morphology_cases import spike_images

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, "tests", "golden", "local_stats_messages.json")


@pytest.mark.parametrize("size_y,size_x", [(3, 3), (15, 15), (7, 3), (1, 5)])
def test_reference_equals_scipy(size_y, size_x):
    ndi = pytest.importorskip("scipy.ndimage")
    stack = np.random.default_rng(size_y * 16 + size_x).integers(0, 65536, (2, 9, 11)).astype(np.uint16)
    ones = np.ones((size_y, size_x), np.int64)
    for power in (1, 2):
        want = np.stack([ndi.correlate(f.astype(np.int64) ** power, ones, mode="nearest") for f in stack])
        got = reference_sums(stack, size_y, size_x, power=power)
        assert got.dtype == np.int64 and np.array_equal(got, want)
    n = size_y * size_x
    mean = reference_mean(stack, size_y, size_x)
    assert mean.dtype == np.uint16 and np.array_equal(mean, np.floor(reference_sums(stack, size_y, size_x) / n + 0.5).astype(np.uint16))


def test_reference_rows_and_mask():
    stack = spike_images(5, 6, np.uint16)
    top = stack.copy()
    top[:, 2:] = 65535  # what lies below the image must not be seen: the clamp goes to rows - 1
    assert np.array_equal(reference_sums(top, 3, 5, rows=2)[:, :2], reference_sums(stack[:, :2], 3, 5))
    assert not reference_sums(top, 3, 5, rows=2)[:, 2:].any() and not reference_sums(top, 3, 5, rows=0).any()
    assert np.array_equal(reference_mean(top, 3, 5, rows=2)[:, 2:], top[:, 2:]) and np.array_equal(reference_mean(stack, 1, 1), stack)
    # the spike of the first nine frames is the one hot pixel; k = 0 and delta = 0: above the local mean
    mask = reference_mask(stack[:9], 3, 3, 0)
    assert mask.sum() == 9 and all(mask[i].sum() == 1 for i in range(9))
    assert np.array_equal(reference_mask(stack, 3, 3, (5, 2), 20, "both"), reference_mask(stack, 3, 3, (5, 2), 20, "both", exact=True))
    assert not reference_mask(stack, 3, 3, 1, rows=0).any()
    # a constant window: d = 0 and V = 0, nothing is hot whatever the rule
    flat = np.full((1, 5, 6), 777, np.uint16)
    for polarity in ("above", "below", "both"):
        assert not reference_mask(flat, 3, 3, 0, -5, polarity).any() and not reference_mask(flat, 3, 3, 3, 0, polarity).any()


def test_int64_holds_every_product_at_the_limits():
    """the scenes with the largest terms at 15 x 15 - all 65535 (the largest S and Q), the 0 / 65535 checkerboard (the largest V), one 65535 on
    0 and one 0 on 65535 (the largest |d|) - with k_num 255 and k_den 64: both sides of the comparison stay below 2^63, and below the bounds
    that rir_amd_device.h and the kernel's comment state.  The limits leave headroom: with the bounds |d| <= 225 * 65535 and V <= 113 * 112 *
    65535^2 the left side first passes 2^63 at k_den = 206 and the right side at k_num = 412, so 64 (6 bits and one) and 255 (8 bits) are
    the round limits below them, not the last values that fit."""
    full = np.full((1, 31, 31), 65535, np.uint16)
    board = np.stack([checkerboard(31, 31, np.uint16), checkerboard(31, 31, np.uint16, 1)])
    spikes = spike_images(31, 31, np.uint16)
    spikes[:9][spikes[:9] != 65535] = 0
    spikes[9:][spikes[9:] != 0] = 65535
    S, Q = reference_sums(full, 15, 15), reference_sums(full, 15, 15, power=2)
    assert (S == 14745375).all() and (Q == 966338150625).all() and int(Q.max()) > 2 ** 32
    worst_d2 = worst_v = 0
    for stack in (full, board, spikes):
        left, right = largest_products(stack, 15, 15, K_DEN_MAX, K_NUM_MAX)
        assert left <= INT64_MAX and right <= INT64_MAX
        worst_d2, worst_v = max(worst_d2, left // K_DEN_MAX ** 2), max(worst_v, right // K_NUM_MAX ** 2)
    v_bound, d_bound = 113 * 112 * 65535 ** 2, 225 * 65535
    assert worst_v == v_bound and 5.43e13 < v_bound < 5.44e13  # the checkerboard
    assert worst_d2 == (224 * 65535) ** 2 <= d_bound ** 2  # one spike in a flat window
    assert d_bound ** 2 * K_DEN_MAX ** 2 < 8.91e17 and K_NUM_MAX ** 2 * v_bound < 3.6e18
    assert DELTA_MAX * 225 < 2 ** 31 and 225 * 966338150625 < INT64_MAX
    first_bad_den = next(k for k in range(1, 1000) if d_bound ** 2 * k * k > INT64_MAX)
    first_bad_num = next(k for k in range(1, 1000) if k * k * v_bound > INT64_MAX)
    assert (first_bad_den, first_bad_num) == (206, 412) and K_DEN_MAX < first_bad_den and K_NUM_MAX < first_bad_num
    # int64 numpy and Python integers agree on these scenes at the limits: nothing wrapped
    for stack in (board, spikes):
        for polarity in ("above", "below"):
            assert np.array_equal(reference_mask(stack, 15, 15, (K_NUM_MAX, K_DEN_MAX), 0, polarity),
                                  reference_mask(stack, 15, 15, (K_NUM_MAX, K_DEN_MAX), 0, polarity, exact=True))


def test_local_stats_args():
    from librir_amd.signal_processing.rir_signal_processing import _local_stats_args

    assert _local_stats_args("local_stats", (2, 4, 5), "uint16", (5, 3), None, outputs=(True, False, False)) == (ord("H"), 5, 3, 4)
    assert _local_stats_args("box_mean", (0, 4, 5), "bool", 15, 0, outputs=(False, False, True)) == (ord("?"), 15, 15, 0)
    assert _local_stats_args("local_threshold", (2, 4, 5), "uint8", 3, 2, k=4) == (ord("B"), 3, 3, 2, 4, 1, 0, 0)
    assert _local_stats_args("local_threshold", (2, 4, 5), "uint16", 3, None, k=(255, 64), delta=-65535, polarity="both") == (ord("H"), 3, 3, 4, 255, 64,
                                                                                                                          -65535, 2)
    assert _local_stats_args("local_threshold", (2, 4, 5), "uint16", 3, None, k=[0, 1], delta=65535, polarity="below")[4:] == (0, 1, 65535, 1)


BAD_SHARED = [dict(size=4), dict(size=0), dict(size=17), dict(size=(3, 4)), dict(size=(3, 3, 3)), dict(size=3.0), dict(rows=5), dict(rows=-1),
              dict(dtype="int16"), dict(dtype="float32"), dict(dtype="uint32")]
BAD_THRESHOLD = [dict(k=(1, 0)), dict(k=(1, 65)), dict(k=256), dict(k=-1), dict(k=(256, 64)), dict(k=2.5), dict(k=(1, 2, 3)), dict(k=None), dict(k=True),
                 dict(delta=65536), dict(delta=-65536), dict(delta=0.5), dict(polarity="up"), dict(polarity=0), dict(polarity=None)]


def label(change):
    return ",".join("%s=%s" % kv for kv in change.items())


@pytest.mark.parametrize("change", BAD_SHARED + BAD_THRESHOLD + [dict(outputs=(False, False, False))], ids=label)
def test_local_stats_args_refuses(change):
    from librir_amd.signal_processing.rir_signal_processing import _local_stats_args

    kw = dict(dict(size=3, rows=None, dtype="uint16", k=3, delta=0, polarity="above", outputs=(True, False, False)), **change)
    if change in BAD_SHARED or "outputs" in change:
        with pytest.raises(ValueError, match="^local_stats: "):
            _local_stats_args("local_stats", (2, 4, 5), kw["dtype"], kw["size"], kw["rows"], outputs=kw["outputs"])
    if "outputs" not in change:
        with pytest.raises(ValueError, match="^local_threshold: "):
            _local_stats_args("local_threshold", (2, 4, 5), kw["dtype"], kw["size"], kw["rows"], k=kw["k"], delta=kw["delta"], polarity=kw["polarity"])


@pytest.mark.parametrize("change", BAD_SHARED + BAD_THRESHOLD, ids=label)
def test_python_forms_reject_bad_parameters_without_a_device(change):
    import torch

    from librir_amd import device as D
    from librir_amd import signal_processing as S

    kw = dict(dict(size=3, rows=None, dtype="uint16", k=3, delta=0, polarity="above"), **change)
    images = np.zeros((6, 4, 5), kw["dtype"])
    frames = torch.from_numpy(images.view(np.int16) if images.dtype == np.uint16 else images)  # (a CPU tensor: the check comes before any device work)
    if images.dtype == np.uint16:
        frames = frames.view(torch.uint16)
    if change in BAD_SHARED:
        for call in (lambda: D.local_stats(frames, kw["size"], kw["rows"]), lambda: D.box_sum(frames[0], kw["size"], kw["rows"]),
                     lambda: D.box_mean(frames, kw["size"], kw["rows"]), lambda: S.local_stats(images, kw["size"], kw["rows"])):
            with pytest.raises(ValueError):
                call()
    for call in (lambda: D.local_threshold(frames, kw["size"], kw["k"], kw["delta"], kw["polarity"], kw["rows"]),
                 lambda: D.local_threshold(frames[0], kw["size"], kw["k"], kw["delta"], kw["polarity"], kw["rows"]),
                 lambda: S.local_threshold(images, kw["size"], kw["k"], kw["delta"], kw["polarity"], kw["rows"])):
        with pytest.raises(ValueError):
            call()


def test_python_forms_reject_no_output_and_wrong_outputs_without_a_device():
    import torch

    from librir_amd import device as D
    from librir_amd import signal_processing as S

    frames = torch.zeros((2, 4, 5), dtype=torch.uint16)
    with pytest.raises(ValueError, match="no output"):
        D.local_stats(frames, 3, sum=False)
    with pytest.raises(ValueError, match="no output"):
        S.local_stats(np.zeros((2, 4, 5), np.uint16), 3, sum=False)
    with pytest.raises(ValueError):
        S.local_stats(np.zeros((2, 2, 4, 5), np.uint16), 3)
    for out in (torch.zeros((2, 4, 5), dtype=torch.int64), torch.zeros((2, 4, 6), dtype=torch.int32), torch.zeros((2, 4, 5), dtype=torch.int32)):
        with pytest.raises(RuntimeError, match="out.sum"):  # (the last one: right dtype and shape, but not a CUDA tensor)
            D.local_stats(frames, 3, out=(out, None, None))
        with pytest.raises(RuntimeError):
            D.box_sum(frames, 3, out=out)
    with pytest.raises(RuntimeError):
        D.local_stats(frames, 3, out=torch.zeros((2, 4, 5), dtype=torch.int32))
    with pytest.raises(RuntimeError):
        D.box_mean(frames, 3, out=torch.zeros((2, 4, 5), dtype=torch.uint16))
    with pytest.raises(RuntimeError):
        D.local_threshold(frames, 3, 3, out=torch.zeros((2, 4, 5), dtype=torch.bool))
    with pytest.raises(ValueError):
        D.local_variance_terms(D.LocalStats(np.zeros(3, np.int32), None, None, 9))
    terms, n2 = D.local_variance_terms(D.LocalStats(np.array([9 * 65535, 5], np.int32), np.array([9 * 65535 ** 2, 13], np.int64), None, 9))
    assert n2 == 81 and terms.dtype == np.int64 and terms.tolist() == [0, 9 * 13 - 25]


def test_python_forms_exist():
    from librir_amd import device as D
    from librir_amd import signal_processing as S
    from librir_amd.video_io import IRMovie

    names = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    defaults = lambda f: {k: p.default for k, p in inspect.signature(f).parameters.items() if p.default is not inspect.Parameter.empty}  # noqa: E731
    assert names(D.local_stats) == ["frames", "size", "rows", "sum", "sumsq", "mean", "out"]
    assert defaults(D.local_stats) == {"rows": None, "sum": True, "sumsq": False, "mean": False, "out": None}
    assert names(D.box_sum) == names(D.box_mean) == ["frames", "size", "rows", "out"]
    assert names(D.local_threshold) == ["frames", "size", "k", "delta", "polarity", "rows", "out"]
    assert defaults(D.local_threshold) == {"delta": 0, "polarity": "above", "rows": None, "out": None}
    assert names(D.local_variance_terms) == ["stats"] and D.LocalStats._fields[:3] == ("sum", "sumsq", "mean")
    assert names(S.local_stats) == ["images", "size", "rows", "sum", "sumsq", "mean"] and names(S.local_threshold) == ["images", "size", "k", "delta",
                                                                                                                     "polarity", "rows"]
    assert "local_stats" in S.__all__ and "local_threshold" in S.__all__
    assert names(IRMovie.local_threshold) == ["self", "size", "k", "delta", "polarity", "selection", "rows", "out"]
    assert defaults(IRMovie.local_threshold) == {"delta": 0, "polarity": "above", "selection": slice(None), "rows": None, "out": None}
    assert names(IRMovie.box_mean) == ["self", "size", "selection", "rows", "out"]
    assert "label_images(mov.local_threshold(9, 4, delta=20))" in IRMovie.local_threshold.__doc__
    assert names(D.rank_filter) == ["frames", "rank", "size", "rows", "out"]  # (the neighbours keep their forms)


STATS_DEVICE = (r"int rir_local_stats_device\(int type, const void \*d_src, int w, int h, int nframes, int size_x, int size_y, int rows, int \*d_sum, "
                r"long long \*d_sumsq,\s+void \*d_mean, void \*stream\);")
THRESHOLD_DEVICE = (r"int rir_local_threshold_device\(int type, const void \*d_src, unsigned char \*d_mask, int w, int h, int nframes, int size_x, int size_y, "
                    r"int rows,\s+int k_num, int k_den, int delta, int polarity, void \*stream\);")
STATS_HOST = (r"int rir_local_stats\(int type, const void \*src, int w, int h, int nframes, int size_x, int size_y, int rows, int \*sum, long long \*sumsq, "
              r"void \*mean\);")
THRESHOLD_HOST = (r"int rir_local_threshold\(int type, const void \*src, unsigned char \*mask, int w, int h, int nframes, int size_x, int size_y, int rows, "
                  r"int k_num,\s+int k_den, int delta, int polarity\);")


def test_entry_points_are_declared_and_exported(lib):
    dev = open(os.path.join(ROOT, "include", "rir_amd_device.h")).read()
    sp = open(os.path.join(ROOT, "include", "rir_amd_signal_processing.h")).read()
    assert re.search(STATS_DEVICE, dev) and re.search(THRESHOLD_DEVICE, dev) and re.search(STATS_HOST, sp) and re.search(THRESHOLD_HOST, sp)
    for name in ("rir_local_stats_device", "rir_local_threshold_device", "rir_local_stats", "rir_local_threshold"):
        assert hasattr(lib, name)


def _bind(lib):
    lib.rir_local_stats_device.argtypes = [ct.c_int, ct.c_void_p] + [ct.c_int] * 6 + [ct.c_void_p] * 4
    lib.rir_local_stats.argtypes = [ct.c_int, ct.c_void_p] + [ct.c_int] * 6 + [ct.c_void_p] * 3
    lib.rir_local_threshold_device.argtypes = [ct.c_int, ct.c_void_p, ct.c_void_p] + [ct.c_int] * 10 + [ct.c_void_p]
    lib.rir_local_threshold.argtypes = [ct.c_int, ct.c_void_p, ct.c_void_p] + [ct.c_int] * 10


GOOD = dict(type=ord("H"), w=5, h=4, nframes=3, size_x=3, size_y=5, rows=4, k_num=3, k_den=1, delta=0, polarity=0)
REFUSED_SHARED = [dict(type=ord("h")), dict(type=ord("f")), dict(type=0), dict(size_x=4), dict(size_y=2), dict(size_x=17), dict(size_y=0), dict(size_x=-3),
                  dict(rows=5), dict(rows=-1), dict(w=0), dict(h=0), dict(nframes=-1), dict(src=None),
                  # wrong in two ways at once: what is reported is what is tested first
                  dict(type=ord("f"), size_x=4), dict(size_x=4, rows=9), dict(rows=9, src=None)]
REFUSED_STATS = [dict(sum=None, sumsq=None, mean=None), dict(overlap="sum"), dict(overlap="sumsq"), dict(overlap="mean"), dict(overlap="outputs"),
                 dict(src=None, sum=None, sumsq=None, mean=None), dict(rows=9, overlap="sum")]
REFUSED_THRESHOLD = [dict(k_num=256), dict(k_num=-1), dict(k_den=0), dict(k_den=65), dict(delta=65536), dict(delta=-65536), dict(polarity=3),
                     dict(polarity=-1), dict(mask=None), dict(overlap="mask"), dict(type=ord("f"), k_den=0), dict(size_x=4, k_num=256),
                     dict(k_num=256, delta=65536), dict(delta=65536, polarity=3), dict(polarity=3, rows=9), dict(k_den=65, mask=None)]


def c_answers(lib):
    """{"<entry> <change>": [return value, last error]} for the four C entries; no buffer is written"""
    from librir_amd.low_level.misc import last_error

    _bind(lib)
    out = {}
    px = 3 * 4 * 5
    src, sums, squares, means, masks = (np.full(px, 7, np.uint16), np.full(px, 7, np.int32), np.full(px, 7, np.int64), np.full(px, 7, np.uint16),
                                        np.full(px, 7, np.uint8))
    for change in REFUSED_SHARED + REFUSED_STATS:
        a = dict(GOOD, src=src.ctypes.data, sum=sums.ctypes.data, sumsq=squares.ctypes.data, mean=means.ctypes.data)
        a.update({k: v for k, v in change.items() if k != "overlap"})
        which = change.get("overlap")
        if which == "outputs":
            a["sumsq"] = a["sum"] + 4 * (px - 1)  # the last cell of the sums is the first of the squares
        elif which:
            a[which] = a["src"] + 2 * (px - 1)  # the last source pixel is the output's first cell
        args = (a["type"], a["src"], a["w"], a["h"], a["nframes"], a["size_x"], a["size_y"], a["rows"], a["sum"], a["sumsq"], a["mean"])
        out["rir_local_stats_device " + label(change)] = [lib.rir_local_stats_device(*args, None), last_error()]
        out["rir_local_stats " + label(change)] = [lib.rir_local_stats(*args), last_error()]
    for change in REFUSED_SHARED + REFUSED_THRESHOLD:
        a = dict(GOOD, src=src.ctypes.data, mask=masks.ctypes.data)
        a.update({k: v for k, v in change.items() if k != "overlap"})
        if change.get("overlap"):
            a["mask"] = a["src"] + 2 * px - 1
        args = (a["type"], a["src"], a["mask"], a["w"], a["h"], a["nframes"], a["size_x"], a["size_y"], a["rows"], a["k_num"], a["k_den"], a["delta"],
                a["polarity"])
        out["rir_local_threshold_device " + label(change)] = [lib.rir_local_threshold_device(*args, None), last_error()]
        out["rir_local_threshold " + label(change)] = [lib.rir_local_threshold(*args), last_error()]
    for a in (src, sums, squares, means, masks):
        assert (a == 7).all()
    return out


def test_refusals_need_no_device_and_are_worded_as_recorded(lib):
    """every entry refuses the call - and says why - whether or not there is a device: the checks come first, in one fixed order"""
    with open(RECORD) as f:
        recorded = json.load(f)
    got = c_answers(lib)
    assert sorted(got) == sorted(recorded)
    different = {k: (v, recorded[k]) for k, v in got.items() if v != recorded[k]}
    assert not different, different
    for key, (r, text) in got.items():
        assert r == -1 and text.startswith(key.split(" ")[0] + ": ") and "no usable HIP device" not in text, (key, text)


def test_no_frames_is_no_work_and_there_is_no_cpu_fallback(lib):
    import torch

    from librir_amd import signal_processing as S
    from librir_amd.low_level.misc import last_error

    _bind(lib)
    src = np.arange(3 * 4 * 5, dtype=np.uint16).reshape(3, 4, 5)
    sums, mask = np.zeros(src.shape, np.int32), np.zeros(src.shape, np.uint8)
    assert lib.rir_local_stats_device(ord("H"), src.ctypes.data, 5, 4, 0, 3, 3, 4, sums.ctypes.data, None, None, None) == 0
    assert lib.rir_local_stats(ord("H"), src.ctypes.data, 5, 4, 0, 3, 3, 4, sums.ctypes.data, None, None) == 0
    assert lib.rir_local_threshold_device(ord("H"), src.ctypes.data, mask.ctypes.data, 5, 4, 0, 3, 3, 4, 3, 1, 0, 0, None) == 0
    assert lib.rir_local_threshold(ord("H"), src.ctypes.data, mask.ctypes.data, 5, 4, 0, 3, 3, 4, 3, 1, 0, 0) == 0
    if torch.cuda.is_available():
        return
    for call in (lambda: lib.rir_local_stats_device(ord("H"), src.ctypes.data, 5, 4, 3, 3, 3, 4, sums.ctypes.data, None, None, None),
                 lambda: lib.rir_local_stats(ord("H"), src.ctypes.data, 5, 4, 3, 3, 3, 4, sums.ctypes.data, None, None),
                 lambda: lib.rir_local_threshold_device(ord("H"), src.ctypes.data, mask.ctypes.data, 5, 4, 3, 3, 3, 4, 3, 1, 0, 0, None),
                 lambda: lib.rir_local_threshold(ord("H"), src.ctypes.data, mask.ctypes.data, 5, 4, 3, 3, 3, 4, 3, 1, 0, 0)):
        assert call() == -1 and "no usable HIP device" in last_error()
    assert not sums.any() and not mask.any()
    with pytest.raises(RuntimeError):
        S.local_stats(src, 3)
    with pytest.raises(RuntimeError):
        S.local_threshold(src, 3, 3)


HIPCC_FOUND = os.path.exists(B.HIPCC) or shutil.which(B.HIPCC) is not None


@pytest.mark.skipif(not HIPCC_FOUND, reason="hipcc not found")
def test_local_kernels_resources(tmp_path):
    """the unit compiles for gfx950; 12 kernels: the statistics for 2 pixel types (bool runs as uint8) x the pair and the general form x with
    and without squares, the mask for 2 pixel types x the two forms; none has a private segment, a spilled register or - as DESIGN.md section
    7 states - any LDS, and all stay at 64 registers or fewer: 8 waves per SIMD.  Looks at the kernels' resource metadata only."""
    asm = str(tmp_path / "local_kernels.s")
    flags = [f for f in B.COMMON if f != "-fPIC"]
    done = subprocess.run([B.HIPCC] + flags + ["-S", "--cuda-device-only", os.path.join(B.CSRC, "local_kernels.hip"), "-o", asm], stdout=subprocess.PIPE,
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
                                      "spilled": field("vgpr_spill_count") + field("sgpr_spill_count")}
    stats = {n: k for n, k in kernels.items() if "local_stats_kernel" in n}
    mask = {n: k for n, k in kernels.items() if "local_threshold_kernel" in n}
    assert len(kernels) == 12 and len(stats) == 8 and len(mask) == 4, sorted(kernels)
    assert all(k["scratch"] == 0 and k["spilled"] == 0 and k["lds"] == 0 for k in kernels.values()), kernels
    assert all(k["vgpr"] <= 64 for k in kernels.values()), {n: k["vgpr"] for n, k in kernels.items()}


if __name__ == "__main__":
    from librir_amd.low_level.misc import _lib

    with open(RECORD, "w") as f:
        json.dump(c_answers(_lib), f, indent=1, sort_keys=True)
        f.write("\n")
