"""CPU: adaptive temporal downsampling (max-hold) - the oracle of downsample_cases.py agrees with a naive image-by-image restatement on the
seeded scenes; the library's host recurrence, rir_downsample_decide, fed the oracle's integer sums returns its keeps and statistics bit for
bit, whole and split across calls; the edges of the arithmetic; refused arguments; the entry points are declared and exported and fail
without a device; the Python API checks its arguments without one; the kernels of downsample_kernels.hip use no scratch."""
import ctypes as ct
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import downsample_cases as DC
from librir_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECIDE_ARGS = [ct.c_int, ct.c_double, ct.c_int, ct.c_longlong, ct.c_void_p, ct.c_int, ct.c_void_p, ct.c_void_p, ct.c_void_p]
PUSH_ARGS = [ct.c_int, ct.c_void_p, ct.c_int, ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_void_p]


@functools.lru_cache(maxsize=None)
def scene(h, w):
    f = DC.scene(DC.FRAMES, h, w, seed=h)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def expected(h, w, lossy, factor, factor_std, method):
    return DC.oracle(scene(h, w), DC.stamps(DC.FRAMES), factor, factor_std, lossy, method)


class Decide:
    """rir_downsample_decide with its state carried from call to call"""

    def __init__(self, lib, factor, factor_std, method, size):
        lib.rir_downsample_decide.argtypes = DECIDE_ARGS
        lib.rir_downsample_state_bytes.restype = ct.c_size_t
        self.lib, self.args = lib, (factor, factor_std, method, size)
        self.state = np.zeros(lib.rir_downsample_state_bytes() // 8 + 1, np.int64)

    def __call__(self, sums, stats=True):
        sums = np.ascontiguousarray(sums, np.int64).reshape(-1, 2)
        n = len(sums)
        keep = np.full(n, -7, np.int32)
        st = np.full(n, -7.0, np.float64)
        r = self.lib.rir_downsample_decide(*self.args, sums.ctypes.data, n, self.state.ctypes.data, keep.ctypes.data, st.ctypes.data if stats else None)
        assert r == int(keep.sum()), (r, keep)
        return keep.astype(bool), st


@pytest.mark.parametrize("method", DC.METHODS)
@pytest.mark.parametrize("factor,factor_std", DC.PARAMS)
@pytest.mark.parametrize("h,w,lossy", DC.SCENES)
def test_the_two_restatements_agree(h, w, lossy, factor, factor_std, method):
    exp = expected(h, w, lossy, factor, factor_std, method)
    DC.same(DC.naive(scene(h, w), DC.stamps(DC.FRAMES), factor, factor_std, lossy, method), exp, (h, w, lossy, factor, factor_std, method))
    on_grid = exp.positions % factor == 0
    assert on_grid.any() and (~on_grid).any(), "the scene exercises both the grid and the events"
    assert exp.positions[0] == 0 and np.array_equal(exp.images[0], scene(h, w)[0])
    if (factor, factor_std, method) == (10, 0., 1):  # (method 2 has no use for factor_std)
        assert len(exp.positions) > 100  # (nearly everything above the smallest statistic)
    if (factor, factor_std, method) == (10, 1., 1):
        assert 26 <= len(exp.positions) <= 40  # (the grid and the events)
    if factor == 10:
        assert {151, 152, 153} <= set(exp.positions.tolist())  # the event's rise, change and fall


@pytest.mark.parametrize("method", DC.METHODS)
@pytest.mark.parametrize("factor,factor_std", DC.PARAMS)
@pytest.mark.parametrize("h,w,lossy", DC.SCENES)
def test_decide_matches_the_oracle_bit_for_bit(lib, h, w, lossy, factor, factor_std, method):
    exp = expected(h, w, lossy, factor, factor_std, method)
    keep, stats = Decide(lib, factor, factor_std, method, w * lossy)(exp.sums)
    assert np.array_equal(keep, exp.keep)
    assert np.array_equal(DC.bits(stats), DC.bits(exp.stats))


@pytest.mark.parametrize("method", DC.METHODS)
def test_decide_split_at_every_cut(lib, method):
    h, w, lossy = DC.SCENES[1]
    exp = expected(h, w, lossy, 10, .9, method)
    for cut in range(DC.FRAMES + 1):
        d = Decide(lib, 10, .9, method, w * lossy)
        k0, s0 = d(exp.sums[:cut])
        k1, s1 = d(exp.sums[cut:], stats=cut % 2 == 0)
        assert np.array_equal(np.concatenate([k0, k1]), exp.keep), cut
        assert np.array_equal(DC.bits(s0), DC.bits(exp.stats[:cut])), cut
        if cut % 2 == 0:
            assert np.array_equal(DC.bits(s1), DC.bits(exp.stats[cut:])), cut
    d = Decide(lib, 10, .9, method, w * lossy)  # image by image
    keep = np.concatenate([d(exp.sums[i:i + 1])[0] for i in range(DC.FRAMES)])
    assert np.array_equal(keep, exp.keep)


def test_factor_one_passes_everything_through(lib):
    f = scene(12, 20)[:30]
    exp = DC.oracle(f, DC.stamps(30), 1, .5, 9, 1)
    assert np.array_equal(exp.positions, np.arange(30)) and np.array_equal(exp.images, f) and not exp.stats.any()
    DC.same(DC.naive(f, DC.stamps(30), 1, .5, 9, 1), exp)
    for method in DC.METHODS:
        keep, stats = Decide(lib, 1, .5, method, 180)(exp.sums)
        assert keep.all() and not stats.any()


@pytest.mark.parametrize("method", DC.METHODS)
@pytest.mark.parametrize("n", [0, 1, 2])
def test_short_sequences(lib, n, method):
    f = scene(12, 20)[:n]
    exp = DC.oracle(f, DC.stamps(n), 3, .5, 12, method)
    DC.same(DC.naive(f, DC.stamps(n), 3, .5, 12, method), exp)
    assert exp.positions.tolist() == [0][:n]
    keep, stats = Decide(lib, 3, .5, method, 240)(exp.sums)
    assert np.array_equal(keep, exp.keep) and np.array_equal(DC.bits(stats), DC.bits(exp.stats))


@pytest.mark.parametrize("method", DC.METHODS)
def test_static_scene_keeps_the_grid_only(lib, method):
    """all statistics are 0: std / mean is NaN in method 2, every comparison with it false"""
    f = np.repeat(scene(12, 20)[:1], 230, 0)
    exp = DC.oracle(f, DC.stamps(230), 10, .9, 12, method)
    assert not exp.stats.any() and not exp.sums.any()
    assert exp.positions.tolist() == list(range(0, 230, 10))
    DC.same(DC.naive(f, DC.stamps(230), 10, .9, 12, method), exp)
    keep, stats = Decide(lib, 10, .9, method, 240)(exp.sums)
    assert np.array_equal(keep, exp.keep) and not stats.any()


def test_uniform_step_where_x_squared_exceeds_2_53(lib):
    """+300 on every pixel of 512 x 640: x = 98 304 000, x * x > 2^53; the exact radicand is 0, the rounded one 0 or tiny - never NaN"""
    size = 512 * 640
    x, q = 300 * size, 300 * 300 * size
    assert x * x > 2 ** 53
    for step in (300, 299, 301, 46341, 65535):
        stat = DC.statistic(step * size, step * step * size, size)
        assert stat == stat and 0.0 <= stat < 1e-3, (step, stat)
    # a radicand that rounds below zero gives 0: q one less than x * x / size can be
    assert DC.statistic(x, q - 1, size) == 0.0 and DC.statistic(3, 1, 4) == 0.0
    sums = np.array([[0, 0], [x, q], [x, q - 1], [65535 * size, 65535 * 65535 * size], [size, 3 * size]], np.int64)
    for method in DC.METHODS:
        keep, stats = Decide(lib, 4, .5, method, size)(sums)
        exp_keep, exp_stats = DC.decide(sums, size, 4, .5, method)
        assert np.array_equal(keep, exp_keep) and np.array_equal(DC.bits(stats), DC.bits(exp_stats))
        assert not np.isnan(stats).any() and stats[2] == 0.0 and stats[4] > 0


def test_largest_differences_have_exact_squares(lib):
    """d = 65535 on every pixel: the reference's int square would overflow; the sums here are exact"""
    f = np.zeros((4, 6, 8), np.uint16)
    f[1::2] = 65535
    exp = DC.oracle(f, DC.stamps(4), 2, .5, 6, 1)
    assert exp.sums[1].tolist() == [65535 * 48, 65535 * 65535 * 48]
    assert not exp.stats.any()  # every pixel moves by the same amount: no spread
    keep, stats = Decide(lib, 2, .5, 1, 48)(exp.sums)
    assert np.array_equal(keep, exp.keep) and np.array_equal(DC.bits(stats), DC.bits(exp.stats))
    f[1, 0, 0] = 0  # one pixel stays: a spread
    exp = DC.oracle(f, DC.stamps(4), 2, .5, 6, 1)
    keep, stats = Decide(lib, 2, .5, 1, 48)(exp.sums)
    assert exp.stats[1] > 0 and np.array_equal(DC.bits(stats), DC.bits(exp.stats))


@pytest.mark.parametrize("factor_std,part", [(0., 0), (0.0104, 0), (0.99, 95), (1., 95)])
def test_part_at_its_ends(lib, factor_std, part):
    assert DC.Recurrence(10, factor_std, 1).part == part
    h, w, lossy = DC.SCENES[0]
    exp = DC.oracle(scene(h, w), DC.stamps(DC.FRAMES), 10, factor_std, lossy, 1)
    keep, stats = Decide(lib, 10, factor_std, 1, w * lossy)(exp.sums)
    assert np.array_equal(keep, exp.keep) and np.array_equal(DC.bits(stats), DC.bits(exp.stats))


def test_refused_arguments(lib):
    from librir_amd.low_level.misc import last_error

    lib.rir_downsample_decide.argtypes = DECIDE_ARGS
    lib.rir_downsample_state_bytes.restype = ct.c_size_t
    lib.rir_downsampler_create.argtypes = [ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_double, ct.c_int]
    state = np.zeros(lib.rir_downsample_state_bytes() // 8 + 1, np.int64)
    sums = np.zeros((3, 2), np.int64)
    keep = np.zeros(3, np.int32)

    def decide(factor, factor_std, method, size, n=3, st=state, sm=sums, kp=keep):
        return lib.rir_downsample_decide(factor, factor_std, method, size, sm.ctypes.data if sm is not None else None, n,
                                         st.ctypes.data if st is not None else None, kp.ctypes.data if kp is not None else None, None)

    assert decide(2, .5, 1, 100) >= 0
    state[:] = 0
    keep[:] = 0
    for bad in [(0, .5, 1, 100), (-1, .5, 1, 100), (2, -.01, 1, 100), (2, 1.01, 1, 100), (2, float("nan"), 1, 100), (2, .5, 0, 100), (2, .5, 3, 100),
                (2, .5, 1, 1), (2, .5, 1, 0), (2, .5, 1, 2 ** 31)]:
        assert decide(*bad) == -1, bad
        assert "rir_downsample_decide" in last_error()
    assert decide(2, .5, 1, 100, n=-1) == -1 and decide(2, .5, 1, 100, st=None) == -1
    assert decide(2, .5, 1, 100, sm=None) == -1 and decide(2, .5, 1, 100, kp=None) == -1
    assert not state.any() and not keep.any()  # nothing was done
    assert decide(2, .5, 1, 2 ** 31 - 1) >= 0 and decide(2, .5, 1, 100, n=0, sm=None, kp=None) == 0
    # the object: lossy_height 0 or > height, S < 2, factor 0, factor_std outside [0, 1], method 3 - refused as arguments, before any device
    for bad in [(20, 12, 0, 2, .5, 1), (20, 12, 13, 2, .5, 1), (1, 1, 1, 2, .5, 1), (1, 5, 1, 2, .5, 1), (20, 12, 12, 0, .5, 1), (20, 12, 12, 2, 1.5, 1),
                (20, 12, 12, 2, -.5, 1), (20, 12, 12, 2, .5, 3), (0, 12, 12, 2, .5, 1), (20, 0, 0, 2, .5, 1), (65536, 32768, 1, 2, .5, 1)]:
        assert lib.rir_downsampler_create(*bad) == 0, bad
        assert "rir_downsampler_create: invalid argument" in last_error(), bad


def test_entry_points_are_declared_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "rir_amd_device.h")).read()
    assert re.search(r"int\s+rir_downsampler_create\(int width, int height, int lossy_height, int factor, double factor_std, int method\);", hdr)
    assert re.search(r"int\s+rir_downsampler_push_device\(int handle, const unsigned short \*d_frames, int nframes, const long long \*timestamps, "
                     r"unsigned short \*d_out,\s+int \*positions, double \*stats, void \*stream\);", hdr)
    assert re.search(r"int\s+rir_downsampler_count\(int handle\);", hdr) and re.search(r"void\s+rir_downsampler_destroy\(int handle\);", hdr)
    assert re.search(r"int\s+rir_downsample_decide\(int factor, double factor_std, int method, long long size, const long long \*sums, int n, "
                     r"void \*state, int \*keep,\s+double \*stats\);", hdr)
    assert re.search(r"size_t\s+rir_downsample_state_bytes\(void\);", hdr)
    for name in ("rir_downsampler_create", "rir_downsampler_push_device", "rir_downsampler_count", "rir_downsampler_destroy", "rir_downsample_decide",
                 "rir_downsample_state_bytes"):
        assert hasattr(lib, name), name
    # the four deviations are stated where the contract is
    for words in ("exact int64", "gives 0 and not NaN", "refused as a whole", "never reads it"):
        assert words in hdr, words
        assert words in open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read(), words


def test_no_cpu_fallback_without_device(lib):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from librir_amd import device as D
    from librir_amd.low_level.misc import last_error

    lib.rir_downsampler_create.argtypes = [ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_double, ct.c_int]
    lib.rir_downsampler_push_device.argtypes = PUSH_ARGS
    assert lib.rir_downsampler_create(20, 12, 12, 2, .5, 1) == 0
    assert "no usable HIP device" in last_error()
    f = scene(12, 20)[:4]
    out = np.zeros_like(f)
    pos = np.zeros(4, np.int32)
    ts = DC.stamps(4)
    assert lib.rir_downsampler_push_device(1, f.ctypes.data, 4, ts.ctypes.data, out.ctypes.data, pos.ctypes.data, None, None) == -1
    assert lib.rir_downsampler_count(1) == -1
    lib.rir_downsampler_destroy(1)  # unknown handle: no-op
    assert not out.any() and not pos.any()
    with pytest.raises(RuntimeError, match="no usable HIP device"):
        D.Downsampler(20, 12, 2, .5)
    with pytest.raises(RuntimeError):
        D.downsample(torch.zeros((4, 12, 20), dtype=torch.uint16), ts, 2, .5)


def test_python_checks_need_no_device():
    import inspect

    import torch

    from librir_amd import device as D
    from librir_amd.video_io import IRMovie, IRSaver

    for bad in [dict(lossy_height=0), dict(lossy_height=13), dict(factor=0), dict(factor_std=-.1), dict(factor_std=1.1), dict(factor_std=float("nan")),
                dict(method=3), dict(method=0), dict(width=0), dict(height=0), dict(width=1, height=1)]:
        args = dict(width=20, height=12, factor=2, factor_std=.5)
        args.update(bad)
        with pytest.raises(ValueError):
            D.Downsampler(**args)
    assert D._downsample_args(20, 12, 3, 1, None, 2) == (20, 12, 12, 3, 1.0, 2)
    with pytest.raises(ValueError):
        D._downsample_stamps([1, 2, 2], 3, None)
    with pytest.raises(ValueError):
        D._downsample_stamps([3, 4], 2, 3)
    with pytest.raises(ValueError):
        D._downsample_stamps([3, 4], 3, None)
    assert D._downsample_stamps([4, 9], 2, 3).dtype == np.int64
    with pytest.raises(RuntimeError):
        D.downsample(torch.zeros((12, 20), dtype=torch.uint16), [1], 2, .5)
    assert D.Downsampled._fields == ("frames", "timestamps", "positions", "stats")
    assert inspect.signature(D.Downsampler.__init__).parameters["method"].default == 1
    assert inspect.signature(IRSaver.add_images).parameters["downsampler"].default is None
    assert inspect.signature(IRMovie.to_h264).parameters["downsample"].default is None


@pytest.mark.skipif(not (os.path.exists(B.HIPCC) or shutil.which(B.HIPCC)), reason="hipcc not found")
def test_downsample_kernels_use_no_scratch(tmp_path):
    asm = str(tmp_path / "downsample_kernels.s")
    flags = [f for f in B.COMMON if f != "-fPIC"]
    done = subprocess.run([B.HIPCC] + flags + ["-S", "--cuda-device-only", os.path.join(B.CSRC, "downsample_kernels.hip"), "-o", asm],
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0, done.stdout
    text = open(asm).read()
    meta = text[text.index("amdhsa.kernels:"):text.index(".end_amdgpu_metadata")]
    kernels = {}
    for block in re.split(r"\n  - ", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            kernels[name.group(1)] = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1))
    assert len(kernels) == 5, sorted(kernels)  # pair sums and max-hold in their 16-byte and ragged forms, and the fold
    assert all(v == 0 for v in kernels.values()), kernels
