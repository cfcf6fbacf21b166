"""GPU: the registration unit (ecc_kernels.hip, registration_abi.cpp) off the diagonal, at the sampling border and on ragged windows.

The suite's other registration tests move every frame by (i, i): a swap of x and y, of gx and gy, or a sign error that only a
negative or single-axis shift shows would leave them green.  Here (cases and references: tests/ecc_reference.py)
  1. ONE iteration from a chosen start - both signs, single axes, half-integers, -1 < t < 0 - on the smallest shapes at which each
     mechanism of the pixel loop can go wrong, through all three forms of the sums (one launch, two launches per iteration, several
     sequences), against the oracle, with a per-case bound max(8 x the oracle's own distance to a float64 reference, 1e-6 px / 1e-7);
  2. twelve fixed iterations on known off-diagonal translations, with and without a blocky mask;
  3. the fused crop + min-max normalisation + gradients against numpy float32, bit for bit, on windows of ragged sizes at the frame's edges;
  4. a tracked sequence that moves by (0.7, -0.4) px a frame, and its mirror image, through every route of the device and host classes.

Every test prints the worst distance it measured before it asserts (pytest -s).  Measured on the MI355X, worst over all cases, with the
bound that applied:
  1a/1b one iteration, one launch = two launches (same bits, 153 succeeding cases): 2.4e-7 px, 2.2e-9 on cc from the oracle (bound: the
        floors 1e-6 px / 1e-7, or 8 x the oracle's own distance to the float64 reference - at most 4.8e-7 px, 1.1e-8); 4.8e-7 px from the
        float64 reference - no farther than the oracle is; every listed failure raises;
  1c    three sequences, one iteration per image: 1.5e-7 px, 5.2e-10 on cc from the oracle's chain (floors); sequence 0 equals its solo run;
  2     twelve iterations: 1.8e-6 px, 3.3e-7 on cc from the oracle (1e-4 px, 1e-6); 0.064 px from the truth at the large shapes (0.1 px);
  3     crop + normalisation + gradients: equal bits in all 32 + 4 cases, sentinels untouched (the float32 division is correctly rounded);
  4     tracked sequence: 0.298 / 0.036 px, mirrored 0.122 / 0.026 px (0.5 px); the three device routes identical, host within 1e-5 px.
No kernel had to be changed.
"""
import ctypes as ct
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ecc_reference as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def grid(oracle):
    return E.reference_grid(oracle)


@pytest.fixture(scope="module")
def one_launch(dev):
    """the library's answers to the whole grid in this process: ecc_run_kernel (all iterations of an alignment in one launch)"""
    assert "RIR_ECC_LAUNCH_PER_ITERATION" not in os.environ
    return dict(zip(E.probe_cases(), E.device_probe_grid()))


def check_against_references(case, got, o, r, worst):
    """a succeeding case: `got` within the case's bound of the oracle's (tx, ty, rho); worst: running maxima for the report"""
    tol_t, tol_cc, d_t, d_cc = E.probe_bounds(o, r)
    e_t, e_cc = max(abs(got[0] - o[0]), abs(got[1] - o[1])), abs(got[2] - o[2])
    f_t, f_cc = max(abs(got[0] - r[0]), abs(got[1] - r[1])), abs(got[2] - r[2])
    worst["oracle_t"], worst["oracle_cc"] = max(worst.get("oracle_t", 0), e_t), max(worst.get("oracle_cc", 0), e_cc)
    worst["f64_t"], worst["f64_cc"] = max(worst.get("f64_t", 0), f_t), max(worst.get("f64_cc", 0), f_cc)
    worst["cpu_t"], worst["cpu_cc"] = max(worst.get("cpu_t", 0), d_t), max(worst.get("cpu_cc", 0), d_cc)
    worst["n"] = worst.get("n", 0) + 1
    return [] if e_t <= tol_t and e_cc <= tol_cc else ["%s: kernel-oracle %.3g px %.3g cc, bound %.3g / %.3g (oracle-float64 %.3g / %.3g); got %r oracle %r"
                                                      % (case, e_t, e_cc, tol_t, tol_cc, d_t, d_cc, got, o)]


# ---- 1a. one iteration, one launch ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", E.PROBE_SHAPES + E.DEGENERATE_SHAPES + [E.ILL_CONDITIONED_SHAPE], ids=lambda s: "%dx%d" % s)
def test_one_iteration_from_every_start_matches_the_oracle(grid, one_launch, shape):
    """find_transform_ecc_translation(T, I, start, 1, 0.0, mask): ecc_run_kernel, three pixels per round.  Every succeeding case of the grid
    within its bound of the oracle; every failing case (no overlap, a vanishing gradient) raises."""
    worst, bad = {}, []
    for case in [c for c in E.probe_cases() if c[0] == shape]:
        o, r = grid[case]
        got = one_launch[case]
        if (got is None) != (o is None):
            bad.append("%s: library %r, oracle %r" % (case, got, o))
        elif o is not None and shape != E.ILL_CONDITIONED_SHAPE:
            bad += check_against_references(case, got, o, r, worst)
    print("one launch %s: %s" % (shape, worst))
    assert not bad, "\n".join(bad)


# ---- 1b. two launches per iteration ------------------------------------------------------------------------------------------------
def test_two_launches_per_iteration_give_the_same_bits_on_the_whole_grid(one_launch):
    """RIR_ECC_LAUNCH_PER_ITERATION=1 in a fresh child process: ecc_sums_kernel + ecc_solve_kernel on the whole grid - the same bits as the
    one-launch form (and with them within the same bounds of the oracle), the same failures."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, os.path.join(root, "tests", "ecc_reference.py")], env=dict(os.environ, RIR_ECC_LAUNCH_PER_ITERATION="1"),
                       capture_output=True, text=True, timeout=300, cwd=root)
    assert p.returncode == 0, p.stderr[-2000:]
    child = json.loads(p.stdout.strip().splitlines()[-1])
    mine = E.to_hex([one_launch[c] for c in E.probe_cases()])
    assert len(child) == len(mine)
    diff = [(c, a, b) for c, a, b in zip(E.probe_cases(), mine, child) if a != b]
    assert not diff, diff[:5]


# ---- 1c. several sequences in one launch -------------------------------------------------------------------------------------------
MULTI_STARTS = [(2.5, -1.5), (-1.0, 0.0), (-2.6, 3.3)]
MULTI_FRAMES = [2, 1, 3]
MULTI_SEED = 80  # scenes MULTI_SEED + q: on these no image of a chain starts within 0.029 px of a rint tie at any of the four shapes (largest step 5.4 px)
MULTI_SHIFTS = [(2.75, -1.5), (-1.25, 2.0), (0.5, -0.75)]  # image k of a sequence is its scene sampled at x + MULTI_SHIFTS[k]


@pytest.mark.parametrize("shape", [(33, 65), (67, 83), (255, 257), (300, 701)], ids=lambda s: "%dx%d" % s)
def test_one_iteration_per_image_of_three_sequences_matches_the_oracle_chain(oracle, dev, shape):
    """rir_ecc_align_multi_device with max_iterations = 1 (ecc_run_multi_kernel: one pixel per round, slices, pairs - the last pair holds one
    sequence), gradients computed in numpy and uploaded: image k starts from the result of image k - 1, as the oracle's chain does; every
    image within its bound of the oracle, and sequence 0 bit for bit what rir_ecc_align_prepared_frames_device gives."""
    import torch

    from librir_amd.registration import device_registration as DR

    h, w = shape
    S, st = len(MULTI_FRAMES), DR._stream()
    templs, images = [], []
    for q in range(S):
        templs.append(E.scene(h, w, MULTI_SEED + q).astype(np.float32))
        images.append(np.stack([E.scene(h, w, MULTI_SEED + q, MULTI_SHIFTS[k]).astype(np.float32) for k in range(MULTI_FRAMES[q])]))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    d_t = [up(t) for t in templs]
    d_i = [up(i) for i in images]
    grads = [[E.gradients32(f) for f in i] for i in images]
    d_gx = [up(np.stack([g[0] for g in gs])) for gs in grads]
    d_gy = [up(np.stack([g[1] for g in gs])) for gs in grads]
    ptr = lambda ts: (ct.c_void_p * S)(*[x.data_ptr() for x in ts])  # noqa: E731
    stride = max(MULTI_FRAMES)
    res = np.full((S, stride, 4), -7.0, np.float64)
    warps = np.array(MULTI_STARTS, np.float32)
    counts, good = (ct.c_int * S)(*MULTI_FRAMES), (ct.c_int * S)()
    torch.cuda.synchronize()
    assert DR._lib.rir_ecc_align_multi_device(ptr(d_t), ptr(d_i), ptr(d_gx), ptr(d_gy), w, h, S, counts, warps.ctypes.data, 1, 0.0, res.ctypes.data,
                                             stride, good, st) == 0
    assert list(good) == MULTI_FRAMES
    worst, bad = {}, []
    for q in range(S):
        tx, ty = MULTI_STARTS[q]
        for k in range(MULTI_FRAMES[q]):
            for v in (tx, ty):  # (a condition of the inputs: no start of the chain on a rint tie unless it is one exactly)
                assert abs((v % 1.0) - 0.5) > 1e-3 or v % 1.0 == 0.5, (q, k, tx, ty)
            o = E.oracle_step(oracle, templs[q], images[q][k], tx, ty)
            r = E.ecc_step64(templs[q], images[q][k], tx, ty)
            assert o is not None and r is not None, (q, k)
            assert res[q, k, 3] == 1
            bad += check_against_references((shape, q, k), tuple(res[q, k, :3]), o, r, worst)
            tx, ty = o[0], o[1]
        assert np.all(res[q, MULTI_FRAMES[q]:] == -7.0)
        assert warps[q, 0] == np.float32(res[q, MULTI_FRAMES[q] - 1, 0]) and warps[q, 1] == np.float32(res[q, MULTI_FRAMES[q] - 1, 1])
    print("multi %s: %s" % (shape, worst))
    assert not bad, "\n".join(bad)
    own = np.full((MULTI_FRAMES[0], 4), -7.0, np.float64)
    w0 = np.array(MULTI_STARTS[0], np.float32)
    assert DR._lib.rir_ecc_align_prepared_frames_device(d_t[0].data_ptr(), d_i[0].data_ptr(), d_gx[0].data_ptr(), d_gy[0].data_ptr(), w, h, MULTI_FRAMES[0],
                                                       w0.ctypes.data, 1, 0.0, own.ctypes.data, st) == MULTI_FRAMES[0]
    assert np.array_equal(own, res[0, :MULTI_FRAMES[0]])


# ---- 2. fixed-iteration alignments off the diagonal ----------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("truth", E.TRUTHS, ids=lambda t: "%g,%g" % t)
@pytest.mark.parametrize("shape", E.TRUTH_SHAPES + [(67, 83), (33, 65)], ids=lambda s: "%dx%d" % s)
def test_twelve_iterations_on_a_known_translation(oracle, dev, shape, truth, masked):
    """max_iterations = 12, eps = 0: the same number of iterations in both implementations, no threshold to flake.  Against the oracle at
    the project's tolerances (1e-4 px, 1e-6 on cc); at the two large shapes within 0.1 px of the truth, with sign and axis."""
    t, i = E.truth_pair(shape, truth)
    m = E.blocky_mask(shape) if masked else None
    o = E.oracle_step(oracle, t, i, 0.0, 0.0, m, iterations=E.TRUTH_ITERATIONS)
    got = E.device_one_iteration(t, i, (0.0, 0.0), m, iterations=E.TRUTH_ITERATIONS)
    assert o is not None and got is not None
    print("12 iterations %s %s masked=%s: kernel-oracle %.3g px, %.3g cc; kernel-truth %.3g px"
          % (shape, truth, masked, max(abs(got[0] - o[0]), abs(got[1] - o[1])), abs(got[2] - o[2]), max(abs(got[0] - truth[0]), abs(got[1] - truth[1]))))
    assert abs(got[0] - o[0]) < 1e-4 and abs(got[1] - o[1]) < 1e-4 and abs(got[2] - o[2]) < 1e-6, (got, o)
    if shape in E.TRUTH_SHAPES:
        assert abs(got[0] - truth[0]) <= 0.1 and abs(got[1] - truth[1]) <= 0.1, (got, truth)


# ---- 3. the fused pre-processing against numpy, bit for bit ----------------------------------------------------------------------------
PREPARE_WINDOWS = {  # frame (h, w): windows (wx, wy, ww, wh)
    (40, 200): [(0, 0, 200, 40), (3, 5, 2, 2), (1, 1, 63, 7), (7, 2, 64, 8), (5, 3, 65, 9), (0, 31, 129, 9), (71, 0, 129, 17)],
    (150, 300): [(21, 11, 257, 131)],
}
PREPARE_CASES = [(f, win) for f, wins in PREPARE_WINDOWS.items() for win in wins]


def prepare_frames(frame_shape, win, dtype, nframes, flat=False):
    """nframes frames (a smooth scene that moves a little from frame to frame, + noise; integers for uint16) with the window's minimum and maximum on the window's own corners and
    more extreme values just outside every side of it: a crop or stride error changes the normalisation of every pixel"""
    h, w = frame_shape
    wx, wy, ww, wh = win
    rng = np.random.default_rng(wx * 1000 + wy * 10 + nframes)
    out = []
    for k in range(nframes):
        f = np.rint(E.unit_range(E.scene(h, w, 50, (0.3 * k, -0.2 * k))) * 40000 + 10000 + rng.normal(0, 30, (h, w)))  # in [9 800, 50 200]
        if dtype == "f":
            f = f + rng.random((h, w))  # (not integers)
        if flat:
            f[wy:wy + wh, wx:wx + ww] = 12345.0
        else:
            corners = [(wy, wx), (wy + wh - 1, wx + ww - 1), (wy, wx + ww - 1), (wy + wh - 1, wx)]
            f[corners[k % 4]] = 5000.0
            f[corners[(k + 1) % 4 if k % 2 == 0 else (k - 1) % 4]] = 60000.0
        ring = lambda k_: np.where(np.arange(k_) % 2 == 0, 100.0, 65000.0)  # noqa: E731  (both extremes on every side that has an outside)
        x0_, x1_, y0_, y1_ = max(wx - 1, 0), min(wx + ww + 1, w), max(wy - 1, 0), min(wy + wh + 1, h)
        if wy > 0:
            f[wy - 1, x0_:x1_] = ring(x1_ - x0_)
        if wy + wh < h:
            f[wy + wh, x0_:x1_] = ring(x1_ - x0_)[::-1]
        if wx > 0:
            f[y0_:y1_, wx - 1] = ring(y1_ - y0_)[::-1]
        if wx + ww < w:
            f[y0_:y1_, wx + ww] = ring(y1_ - y0_)
        out.append(f)
    return np.stack(out).astype(np.uint16 if dtype == "H" else np.float32)


def expected_prepare(full32, win):
    """numpy float32: crop, min-max normalisation, central differences with reflect-101 borders, of every frame"""
    wx, wy, ww, wh = win
    norms, gxs, gys = [], [], []
    for f in full32:
        w_ = f[wy:wy + wh, wx:wx + ww]
        assert w_.dtype == np.float32
        with np.errstate(all="ignore"):
            n = (w_ - w_.min()) / (w_.max() - w_.min())
            gx, gy = E.gradients32(n)
        assert n.dtype == np.float32
        norms.append(n), gxs.append(gx), gys.append(gy)
    return np.stack(norms), np.stack(gxs), np.stack(gys)


SENTINEL, PAD = -7.25, 64


def run_prepare(DR, frames_t, dtype, sigma, win, nframes):
    """rir_ecc_prepare_frames_device into buffers with sentinel words behind them -> (norm, gx, gy) as numpy (n, wh, ww)"""
    import torch

    n, h, w = frames_t.shape
    wx, wy, ww, wh = win
    outs = [torch.full((nframes * wh * ww + PAD,), SENTINEL, dtype=torch.float32, device="cuda") for _ in range(3)]
    assert DR._lib.rir_ecc_prepare_frames_device(frames_t.data_ptr(), ord(dtype), w, h, nframes, float(sigma), wx, wy, ww, wh, outs[0].data_ptr(),
                                                outs[1].data_ptr(), outs[2].data_ptr(), DR._stream()) == 0
    torch.cuda.synchronize()
    for o in outs:
        assert torch.all(o[nframes * wh * ww:] == SENTINEL).item(), "words behind the outputs were written"
    return outs, [o[:nframes * wh * ww].cpu().numpy().reshape(nframes, wh, ww) for o in outs]


@pytest.mark.parametrize("nframes", [1, 5])
@pytest.mark.parametrize("dtype", ["H", "f"])
@pytest.mark.parametrize("case", PREPARE_CASES, ids=lambda c: "%dx%d-%d,%d,%dx%d" % (c[0][1], c[0][0], c[1][0], c[1][1], c[1][2], c[1][3]))
def test_fused_pre_processing_equals_numpy_bit_for_bit(oracle, dev, case, dtype, nframes):
    """rir_ecc_prepare_frames_device, sigma = 0 (minmax_apply_grad_frames_kernel: 64 x 8 tiles, neighbours by lane shuffle, loads at the edges)
    against the same two float32 operations per value in numpy - equal bits in norm, gx and gy; rir_minmax_normalize_device on the strided
    window gives the same norm; rir_ecc_register_frame_device reports what rir_ecc_align_prepared_device gives on the prepared arrays."""
    import torch

    from librir_amd.registration import device_registration as DR

    frame_shape, win = case
    h, w = frame_shape
    wx, wy, ww, wh = win
    frames = prepare_frames(frame_shape, win, dtype, nframes)
    full32 = frames.astype(np.float32)
    outside = (wx, wy, ww, wh) != (0, 0, w, h)
    for f in full32:
        assert f[wy:wy + wh, wx:wx + ww].min() == 5000.0 and f[wy:wy + wh, wx:wx + ww].max() == 60000.0
        assert not outside or (f.min() == 100.0 and f.max() == 65000.0)
    exp = expected_prepare(full32, win)
    t = torch.from_numpy(frames).cuda()
    outs, got = run_prepare(DR, t, dtype, 0.0, win, nframes)
    for name, g, e in zip(("norm", "gx", "gy"), got, exp):
        assert np.array_equal(g, e, equal_nan=True), (name, np.argwhere(g != e)[:4], g[g != e][:4], e[g != e][:4])
    # the two-kernel normalisation of one strided window: the same bits
    t32 = torch.from_numpy(full32).cuda()
    for k in range(nframes):
        out = torch.full((wh * ww + PAD,), SENTINEL, dtype=torch.float32, device="cuda")
        assert DR._lib.rir_minmax_normalize_device(t32[k, wy:, wx:].data_ptr(), ww, wh, w, out.data_ptr(), DR._stream()) == 0
        torch.cuda.synchronize()
        assert np.array_equal(out[:wh * ww].cpu().numpy().reshape(wh, ww), exp[0][k]) and torch.all(out[wh * ww:] == SENTINEL).item(), k
    # one call per frame against the prepared arrays of the batch: frame 0's window is the reference, the last frame is aligned to it
    ref = torch.from_numpy(exp[0][0]).cuda()
    k, npx = nframes - 1, wh * ww
    res = []
    for prepared in (False, True):
        warp, cc, it = np.array([0.25, -0.5], np.float32), ct.c_double(0), ct.c_int(0)
        if prepared:
            rc = DR._lib.rir_ecc_align_prepared_device(ref.data_ptr(), outs[0][k * npx:].data_ptr(), outs[1][k * npx:].data_ptr(), outs[2][k * npx:].data_ptr(),
                                                      ww, wh, warp.ctypes.data, 3, 0.0, ct.byref(cc), ct.byref(it), DR._stream())
        else:
            rc = DR._lib.rir_ecc_register_frame_device(t[k].data_ptr(), ord(dtype), w, h, 0.0, wx, wy, ww, wh, ref.data_ptr(), warp.ctypes.data, 3, 0.0,
                                                      ct.byref(cc), ct.byref(it), DR._stream())
        res.append((rc, float(warp[0]).hex(), float(warp[1]).hex(), cc.value.hex() if rc == 0 else None))
    assert res[0] == res[1], res
    # ... and what the oracle gives on numpy's arrays, at the project's tolerances (2 x 2: both gradients vanish - the alignment fails everywhere)
    o = E.oracle_step(oracle, exp[0][0], exp[0][k], 0.25, -0.5, iterations=3)
    assert (res[0][0] == 0) == (o is not None) and (o is None) == (win == (3, 5, 2, 2)), (res[0], o)
    if o is not None:
        got = [float.fromhex(v) for v in res[0][1:]]
        assert abs(got[0] - o[0]) < 1e-4 and abs(got[1] - o[1]) < 1e-4 and abs(got[2] - o[2]) < 1e-6, (got, o)


@pytest.mark.parametrize("dtype", ["H", "f"])
def test_fused_pre_processing_of_a_flat_window_gives_nan_like_numpy(dev, dtype):
    """0 / 0 in every pixel of norm, and in every gradient, in the kernel as in numpy"""
    import torch

    from librir_amd.registration import device_registration as DR

    win = (5, 3, 65, 9)
    frames = prepare_frames((40, 200), win, dtype, 2, flat=True)
    exp = expected_prepare(frames.astype(np.float32), win)
    assert all(np.isnan(e).all() for e in exp)
    _, got = run_prepare(DR, torch.from_numpy(frames).cuda(), dtype, 0.0, win, 2)
    for g, e in zip(got, exp):
        assert np.array_equal(g, e, equal_nan=True)


@pytest.mark.parametrize("dtype", ["H", "f"])
def test_fused_pre_processing_behind_the_gaussian_filter_is_bit_exact(dev, dtype):
    """sigma = 0.5: dev.gaussian_filter's output through the numpy expectation - everything downstream of the filter, bit for bit"""
    import torch

    from librir_amd.registration import device_registration as DR

    win = (5, 3, 65, 9)
    frames = prepare_frames((40, 200), win, dtype, 3)
    t = torch.from_numpy(frames).cuda()
    filtered = dev.gaussian_filter(t, 0.5).cpu().numpy()
    assert filtered.dtype == np.float32 and filtered.shape == frames.shape
    exp = expected_prepare(filtered, win)
    _, got = run_prepare(DR, t, dtype, 0.5, win, 3)
    for name, g, e in zip(("norm", "gx", "gy"), got, exp):
        assert np.array_equal(g, e, equal_nan=True), name


# ---- 4. a tracked sequence whose motion is not diagonal ----------------------------------------------------------------------------------
TRACK_N, TRACK_SHAPE, TRACK_V = 24, (96, 160), (0.7, -0.4)


def track_frames(sign, dtype):
    """frame i moves by sign * (0.7 i, -0.4 i)"""
    h, w = TRACK_SHAPE
    rng = np.random.default_rng(5 if sign > 0 else 6)
    f = np.stack([E.scene(h, w, 11, (-sign * TRACK_V[0] * i, -sign * TRACK_V[1] * i)) + rng.normal(0, 0.01, (h, w)) for i in range(TRACK_N)])
    if dtype == "uint16":
        return np.rint((f - f.min()) / (f.max() - f.min()) * 60000 + 1000).astype(np.uint16)
    return f.astype(np.float32)


@pytest.mark.parametrize("dtype", ["float32", "uint16"])
def test_tracked_sequence_with_off_diagonal_motion(monkeypatch, dev, dtype):
    """compute, compute_many(chunk=7) and compute_many_multi (with the mirrored sequence beside it) give identical lists; x[i] within 0.5 px
    of 0.7 i and y[i] within 0.5 px of -0.4 i, signed (the last shift is about (16.1, -9.2): swapped axes or a wrong sign miss by pixels);
    the mirrored sequence gives the mirrored signs; the host class, step by step, agrees at 1e-5 px / 1e-7."""
    import torch

    from librir_amd.registration import DeviceRegistratorECC, MaskedRegistratorECC

    monkeypatch.setenv("RIR_REGISTRATION_STEP_BY_STEP", "1")
    h, w = TRACK_SHAPE
    fwd, back = track_frames(+1, dtype), track_frames(-1, dtype)
    t, tb = torch.from_numpy(fwd).cuda(), torch.from_numpy(back).cuda()
    new = lambda: DeviceRegistratorECC(1, 1, sigma=0, shape=TRACK_SHAPE)  # noqa: E731
    one = new()
    one.start(t[0])
    for i in range(1, TRACK_N):
        one.compute(t[i])
    many, many_b = new(), new()
    many.start(t[0]), many_b.start(tb[0])
    many.compute_many(t[1:], chunk=7)
    many_b.compute_many(tb[1:], chunk=7)
    multi = [new(), new()]
    multi[0].start(t[0]), multi[1].start(tb[0])
    DeviceRegistratorECC.compute_many_multi(multi, [t[1:], tb[1:]], chunk=7)
    tracks = lambda r: (r.x, r.y, r.confidences)  # noqa: E731
    assert len(one.x) == TRACK_N and tracks(one) == tracks(many) == tracks(multi[0])
    assert tracks(many_b) == tracks(multi[1])
    i = np.arange(TRACK_N)
    ex, ey = np.abs(np.array(one.x) - TRACK_V[0] * i), np.abs(np.array(one.y) - TRACK_V[1] * i)
    bx, by = np.abs(np.array(many_b.x) + TRACK_V[0] * i), np.abs(np.array(many_b.y) + TRACK_V[1] * i)
    print("track %s: worst error %.3f / %.3f px, mirrored %.3f / %.3f px; last shift (%.3f, %.3f)" % (dtype, ex.max(), ey.max(), bx.max(), by.max(), one.x[-1], one.y[-1]))
    assert ex.max() <= 0.5 and ey.max() <= 0.5, (one.x, one.y)
    assert bx.max() <= 0.5 and by.max() <= 0.5, (many_b.x, many_b.y)
    host = MaskedRegistratorECC(1, 1, sigma=0)
    host.subW, host.subH, host.startX, host.startY = w, h, 0, 0
    host.start(fwd[0])
    assert host._dev is None
    for k in range(1, TRACK_N):
        host.compute(fwd[k])
    assert np.allclose(one.x, host.x, rtol=0, atol=1e-5) and np.allclose(one.y, host.y, rtol=0, atol=1e-5)
    assert np.allclose(one.confidences, host.confidences, rtol=0, atol=1e-7)
