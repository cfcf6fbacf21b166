"""GPU: the frame-buffer filters over the whole 16-bit range (cases.FULL_RANGE_KINDS) and on frames under three rows or columns, against
the oracle bit for bit (the float32 gaussian within 2e-6 relative, bit for bit in the reference's order).  The oracle is pinned to the
compiled reference on the same grid by tests/test_oracle_golden.py.  What runs here and nowhere else: quantile answers beyond the first
quarter of the value range and the 65535 cut, 32-bit squares that wrap and the NaN deviation they lead to, clamp floors above 32767,
lists of thousands of flagged pixels, and the read-back repair of small frames, which repairs in list order."""
import ctypes as ct

import numpy as np
import pytest
from cases import FULL_RANGE_KINDS, FULL_RANGE_PERCENTS, FULL_RANGE_SHAPES, full_range_frames

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def u16_as_kernels(x):
    """float -> uint16 as the kernels convert (CastTo<uint16_t>: truncation through int32), not a clip: a wrap at the top shows"""
    return (np.trunc(np.asarray(x, np.float64)).astype(np.int64) & 0xFFFF).astype(np.uint16)


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def gaussian_close(g, r):
    """the float32 gaussian against the oracle's: within 2e-6 of the largest value (the order of the sums differs, not the terms)"""
    return np.abs(g - r).max() <= 2e-6 * np.abs(r).max()


# ---- find_median_pixel ---------------------------------------------------------------------------------------------------------------


def _median_batch_cases():
    """(name, frames (n, h, w), masks (n, h, w)) of full-range frames; h * w odd, so every frame after the first starts off a 16-byte
    boundary and ends in a scalar tail"""
    rng = np.random.default_rng(55)
    h, w = 67, 83
    kinds = np.stack([full_range_frames(k, h, w)[0] for k in FULL_RANGE_KINDS])
    # one frame per quarter of the value range: the answers at 0.5 lie in four different quarters of one batch
    quarters = np.stack([np.clip(q * 16384 + 8000 + rng.normal(0, 3000, (h, w)), 0, 65535).astype(np.uint16) for q in range(4)])
    tops = np.stack([np.full((h, w), 65535, np.uint16),  # every target reached only at 65535: 0
                     np.where(rng.random((h, w)) < 0.7, 65535, 65534).astype(np.uint16),  # 65534 up to 0.3, then 0
                     rng.integers(65500, 65536, (h, w)).astype(np.uint16)])
    masks = lambda n: (rng.random((n, h, w)) < 0.4).astype(np.uint8)
    return [("kinds", kinds, masks(len(kinds))), ("quarters", quarters, masks(4)), ("tops", tops, masks(3))]


def _oracle_medians(oracle, frames, masks, p):
    return [oracle.find_median_pixel(f, p) for f in frames], [oracle.find_median_pixel(f, p, m) for f, m in zip(frames, masks)]


def test_find_median_pixel_full_range_batches(dev, oracle):
    """device batch call: answers in every quarter, 65534, targets only 65535 reaches (answer 0), full / empty masks, percent 0 and 1"""
    seen = set()
    for name, fr, masks in _median_batch_cases():
        t, tm = cuda(fr), cuda(masks)
        for p in FULL_RANGE_PERCENTS:
            want, want_m = _oracle_medians(oracle, fr, masks, p)
            assert dev.find_median_pixel(t, p).cpu().tolist() == want, (name, p)
            assert dev.find_median_pixel(t, p, tm).cpu().tolist() == want_m, (name, p)
            seen.update(v >> 14 for v in want + want_m)
            seen.update("65534" for v in want if v == 65534)
        for full in (np.ones_like(masks), np.zeros_like(masks)):
            for p in (0.0, 0.5, 1.0):
                assert dev.find_median_pixel(t, p, cuda(full)).cpu().tolist() == [oracle.find_median_pixel(f, p, m) for f, m in zip(fr, full)], (name, p)
    assert {0, 1, 2, 3, "65534"} <= seen
    assert [oracle.find_median_pixel(np.full((3, 5), 65535, np.uint16), p) for p in (0.0, 0.5, 1.0)] == [0, 0, 0]


def test_find_median_pixel_quarter_per_frame(dev, oracle):
    """one batch, one percent, each frame answering in another quarter: the count carried from quarter to quarter is the frame's own"""
    _, fr, masks = _median_batch_cases()[1]
    want = [oracle.find_median_pixel(f, 0.5) for f in fr]
    assert [v >> 14 for v in want] == [0, 1, 2, 3]
    assert dev.find_median_pixel(cuda(fr), 0.5).cpu().tolist() == want
    rev = fr[::-1].copy()
    assert dev.find_median_pixel(cuda(rev), 0.5).cpu().tolist() == want[::-1]


@pytest.mark.parametrize("npx", [5561, 327680, 8 * 1024 * 4 + 3, 17])
def test_find_median_pixel_vector_and_scalar_paths(dev, oracle, npx):
    """one frame at an aligned start (16-byte loads, scalar tail when npx % 8) and the same frame one element further (scalar loads only):
    both answer as the oracle in every quarter, with and without a mask"""
    rng = np.random.default_rng(npx)
    img = rng.integers(0, 65536, npx).astype(np.uint16)
    img[: npx // 50] = 65535
    mask = (rng.random(npx) < 0.5).astype(np.uint8)
    base = torch.zeros(npx + 8, dtype=torch.uint16, device="cuda")
    for start in (0, 1):
        t = base[start:start + npx]
        t.copy_(cuda(img))
        assert (t.data_ptr() % 16 == 0) == (start == 0)
        for p in FULL_RANGE_PERCENTS:
            assert dev.find_median_pixel(t.view(1, 1, npx), p).item() == oracle.find_median_pixel(img, p), (start, p)
            assert dev.find_median_pixel(t.view(1, 1, npx), p, cuda(mask).view(1, 1, npx)).item() == oracle.find_median_pixel(img, p, mask), (start, p)


def test_find_median_pixel_host_full_range(oracle):
    """the reference's host entry point (signal_processing.find_median_pixel) on the same frames"""
    from librir_amd.signal_processing import find_median_pixel

    for name, fr, masks in _median_batch_cases():
        for f, m in zip(fr, masks):
            for p in FULL_RANGE_PERCENTS:
                assert find_median_pixel(f, p) == oracle.find_median_pixel(f, p), (name, p)
                assert find_median_pixel(f, p, m) == oracle.find_median_pixel(f, p, m), (name, p)
            assert find_median_pixel(f, 0.5, np.zeros_like(m)) == oracle.find_median_pixel(f, 0.5, np.zeros_like(m)) == 0


# ---- bad pixels: detector, floors, correct() -----------------------------------------------------------------------------------------


def _info(lib, handle, cap):
    info = (ct.c_int * 3)()
    xy = np.zeros((max(cap, 1), 2), np.int32)
    assert lib.rir_bad_pixels_info(handle, info, xy.ctypes.data_as(ct.c_void_p), cap) == 0
    return list(info), xy[: info[0]]


@pytest.mark.parametrize("shape", FULL_RANGE_SHAPES)
@pytest.mark.parametrize("kind", FULL_RANGE_KINDS)
def test_bad_pixels_full_range(dev, oracle, lib, kind, shape):
    """positions, floor_detect and floor_correct (the NaN deviation, floors above 32767, a threshold that wraps in 16 bits) and correct()
    of three later frames, on the whole frame and on its first h - 3 rows; and through the reference's host entry points"""
    from librir_amd.signal_processing import BadPixels as HostBadPixels

    h, w = shape
    first, later = full_range_frames(kind, h, w)
    tl = cuda(later)
    for rows in (h, h - 3):
        xy = oracle.bad_pixels_detect(first[:rows])
        fd, fc = oracle.bad_pixels_stats(first[:rows])
        bp = dev.BadPixels(cuda(first), rows=None if rows == h else rows)
        assert (bp.count, bp.floor_detect, bp.floor_correct) == (len(xy), fd, fc), (rows, bp.count, bp.floor_detect, bp.floor_correct, len(xy), fd, fc)
        info, got = _info(lib, bp.handle, len(xy))
        assert info == [len(xy), fc, fd] and np.array_equal(got, xy) and np.array_equal(bp.positions(), xy)
        if rows == h:
            exp = np.stack([oracle.bad_pixels_correct(f, xy, fc) for f in later])
            assert np.array_equal(bp.correct(tl).cpu().numpy(), exp)
            hb = HostBadPixels(first)
            info, got = _info(lib, hb.handle, len(xy))
            assert info == [len(xy), fc, fd] and np.array_equal(got, xy)
            for f, e in zip(later, exp):
                assert np.array_equal(hb.correct(f), e)
            del hb
        bp.close()


def test_bad_pixels_full_range_grid_reaches_its_paths(oracle):
    """what the grid above is for, at both sizes (the CPU suite checks the same of the oracle against the reference)"""
    for h, w in FULL_RANGE_SHAPES:
        first, _ = full_range_frames("saturated_blob", h, w)
        fd, fc = oracle.bad_pixels_stats(first)
        assert fc < -(1 << 30) and len(oracle.bad_pixels_detect(first)) > h * w // 3  # NaN deviation: dense list
        assert oracle.bad_pixels_stats(full_range_frames("high_dead", h, w)[0])[1] > 32767


# ---- dense lists: the fused chain and the read-back repair -------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def dense(dev):
    """the NaN case: about half of the frame flagged"""
    h, w = 67, 83
    first, later = full_range_frames("saturated_blob", h, w)
    frames = np.concatenate([first[None], later, full_range_frames("uniform", h, w)[1]])
    return first, frames


@pytest.mark.parametrize("sigma", [0.75, 1.0, 1.7, 2.0])  # radius 1, 2, 3, 4
def test_filter_chain_dense_list(dev, oracle, dense, sigma):
    first, frames = dense
    x = cuda(frames)
    bp = dev.BadPixels(x[0])
    assert bp.count > first.size // 3
    for off, strat in (((1.25, -2.5), "nearest"), ((-0.5, 0.75), "background"), ((0.0, 0.0), "nearest")):
        ref = dev.translate_to_u16(dev.gaussian_filter(bp.correct(x), sigma), off, strat, background=65535)
        out = dev.filter_chain(x, bp, sigma, off, strat, background=65535)
        assert torch.equal(out.view(torch.int16), ref.view(torch.int16)), (sigma, off, strat)
        # the whole chain on the oracle: within one level where the float32 gaussian sits next to an integer boundary.  At values up to
        # 65535 its error (2e-6 relative: up to 0.13 of a level) meets more boundaries than on the 10-bit scenes of test_gpu_filters.py
        xy = oracle.bad_pixels_detect(first)
        _, fc = oracle.bad_pixels_stats(first)
        o = out.cpu().numpy().astype(np.int64)
        for i in (1, 4):
            t = u16_as_kernels(oracle.translate(oracle.gaussian_filter(oracle.bad_pixels_correct(frames[i], xy, fc).astype(np.float32), sigma), off[0], off[1],
                                                strat, background=65535.0))
            d = np.abs(t.astype(np.int64) - o[i])
            assert d.max() <= 1 and (d != 0).mean() < 1e-2, (sigma, off, i, d.max(), (d != 0).mean())


@pytest.fixture
def reference_order(lib):
    lib.rir_set_gaussian_reference_order(1)
    yield
    lib.rir_set_gaussian_reference_order(0)


@pytest.mark.parametrize("sigma", [0.75, 1.0, 1.7, 2.0])
def test_filter_chain_dense_list_in_reference_order(dev, oracle, dense, sigma, reference_order):
    first, frames = dense
    x = cuda(frames)
    bp = dev.BadPixels(x[0])
    xy = oracle.bad_pixels_detect(first)
    _, fc = oracle.bad_pixels_stats(first)
    out = dev.filter_chain(x, bp, sigma, (1.25, -2.5), "nearest").cpu().numpy()
    for i in range(len(frames)):
        t = oracle.translate(oracle.gaussian_filter(oracle.bad_pixels_correct(frames[i], xy, fc).astype(np.float32), sigma), 1.25, -2.5, "nearest")
        assert np.array_equal(out[i], u16_as_kernels(t)), (sigma, i)


def _whole_window_flagged(xy, w, rows):
    """flagged pixels whose shifted 3x3 window holds only flagged pixels (IRFileLoader.cpp:760-790: the pixel is left as it is)"""
    bm = np.zeros((rows, w), bool)
    bm[xy[:, 1], xy[:, 0]] = True
    out = []
    for x, y in xy:
        x0 = min(max(x - 1, 0), w - 3)
        y0 = min(max(y - 1, 0), rows - 3)
        if bm[y0:y0 + 3, x0:x0 + 3].all():
            out.append((x, y))
    return out


def test_remove_bad_pixels_dense_list(dev, oracle, dense):
    first, frames = dense
    h, w = first.shape
    rows = h - 3
    bp = dev.BadPixels(cuda(first), rows=rows)
    xy = oracle.bad_pixels_detect(first[:rows])
    assert np.array_equal(bp.positions(), xy) and len(xy) > 1000
    assert len(_whole_window_flagged(xy, w, rows)) > 0
    t = cuda(frames)
    bp.remove_inplace(t, rows)
    assert np.array_equal(t.cpu().numpy(), np.stack([oracle.remove_bad_pixels(f, xy, rows=rows) for f in frames]))


# ---- small frames: the read-back repair in list order ------------------------------------------------------------------------------------


def _small_first(h, w, seed):
    """a cold scene with two saturated pixels in the detector's h - 3 rows: the deviation is NaN, floor_detect the median, about half of
    the pixels flagged - runs of adjacent flagged pixels in any shape"""
    rng = np.random.default_rng(seed)
    img = (120 + rng.integers(0, 40, (h, w))).astype(np.uint16)
    img.flat[rng.choice((h - 3) * w, 2, replace=False)] = 65535
    return img


SMALL_SHAPES = [(4, 24), (5, 24), (4, 400), (5, 131), (40, 1), (40, 2), (200, 2), (9, 1)]  # (h, w): rows = h - 3 on read-back


@pytest.mark.parametrize("shape", SMALL_SHAPES)
def test_remove_bad_pixels_small_frames(dev, oracle, shape):
    """frames under three rows (read-back uses h - 3) or columns: the reference repairs in list order, each repair reading the earlier ones
    (IRFileLoader.cpp:735-753).  Lists longer than one wave (4 x 400, 200 x 2) included; two runs give the same frames."""
    h, w = shape
    rows = h - 3
    first = _small_first(h, w, h * 1000 + w)
    xy = oracle.bad_pixels_detect(first[:rows])
    assert len(xy) >= 2
    rng = np.random.default_rng(w)
    frames = np.concatenate([first[None], rng.integers(0, 65536, (5, h, w)).astype(np.uint16)])
    exp = np.stack([oracle.remove_bad_pixels(f, xy, rows=rows) for f in frames])
    assert not np.array_equal(exp[1:], np.stack([_repair_all_at_once(f, xy, rows) for f in frames[1:]]))  # the order shows in these frames
    bp = dev.BadPixels(cuda(first), rows=rows)
    assert np.array_equal(bp.positions(), xy)
    runs = []
    for _ in range(2):
        t = cuda(frames)
        bp.remove_inplace(t, rows)
        runs.append(t.cpu().numpy())
    assert np.array_equal(runs[0], exp), (shape, int((runs[0] != exp).sum()))
    assert np.array_equal(runs[1], runs[0])
    if shape in ((4, 400), (200, 2)):
        assert len(xy) > 64


def _repair_all_at_once(img, xy, rows):
    """every repair from the unrepaired frame (what a parallel repair without order computes): to show the test frames tell the two apart"""
    out = img.copy()
    h, w = img.shape
    for x, y in xy:
        win = img[max(y - 1, 0):min(y + 2, rows), max(x - 1, 0):min(x + 2, w)].ravel()
        out[y, x] = np.sort(win)[win.size // 2]
    return out


@pytest.mark.parametrize("shape", [(4, 24), (5, 24), (40, 1), (40, 2), (4, 400)])
def test_read_back_small_frames(tmp_path, oracle, shape):
    """a recording of frames this small read back with bad_pixels_correction: load_pos and to_tensor repair as the reference does"""
    from librir_amd.video_io import IRMovie, IRSaver

    h, w = shape
    rows = h - 3
    first = _small_first(h, w, 7 * h + w)
    rng = np.random.default_rng(h + w)
    frames = np.concatenate([first[None], rng.integers(0, 65536, (6, h, w)).astype(np.uint16)])
    path = tmp_path / "small.h264"
    with IRSaver(path, w, h, h) as s:
        for i in range(len(frames)):
            s.add_image(frames[i], i * 20000000 + 7)
    xy = oracle.bad_pixels_detect(first[:rows])
    exp = np.stack([oracle.remove_bad_pixels(f, xy, rows=rows) for f in frames])
    with IRMovie.from_filename(path) as mov:
        assert np.array_equal(mov.to_tensor().cpu().numpy(), frames)
        mov.bad_pixels_correction = True
        for _ in range(2):
            assert np.array_equal(mov.to_tensor().cpu().numpy(), exp), shape
        assert np.array_equal(np.stack([mov.load_pos(i) for i in range(len(frames))]), exp), shape


# ---- 3x3 median filter ------------------------------------------------------------------------------------------------------------


MEDIAN_WIDTHS = [3, 4, 5, 59, 60, 61, 62, 63, 64, 65, 120, 121, 124, 640]
MEDIAN_HEIGHTS = [3, 4, 16, 17, 63, 64, 65, 129, 512]


def _median_frames(n, h, w, seed):
    """full-range noise with runs of 0 and 65535 along rows and columns"""
    rng = np.random.default_rng(seed)
    fr = rng.integers(0, 65536, (n, h, w)).astype(np.uint16)
    for f in fr:
        for v in (0, 65535):
            y, x = rng.integers(0, h), rng.integers(0, w)
            f[y, x:x + int(rng.integers(2, 9))] = v
            f[y:y + int(rng.integers(2, 9)), x] = v
        f[rng.random((h, w)) < 0.05] = rng.choice([0, 65535])
    return fr


@pytest.mark.parametrize("h", MEDIAN_HEIGHTS)
def test_median_filter_full_range_shapes(dev, oracle, h):
    """every width against this height: around the 60-column x 64-row tile and the w % 4 == 0 store path"""
    for w in MEDIAN_WIDTHS:
        n = 3 if h * w < 100000 else 2
        fr = _median_frames(n, h, w, h * 1000 + w)
        got = dev.median_filter(cuda(fr)).cpu().numpy()
        for i in range(n):
            assert np.array_equal(got[i], oracle.median_filter(fr[i])), (h, w, i)


# ---- translate, remove_motion, gaussian ------------------------------------------------------------------------------------------------


def _translate_frames():
    fr = [full_range_frames(k, 67, 83)[1][0] for k in ("ti_bits", "saturated_blob", "checkerboard", "uniform", "high_dead", "wide_normal")]
    return np.stack(fr + [np.full((67, 83), 65535, np.uint16), np.full((67, 83), 65534, np.uint16)])


OFFSETS = [(0.5, 0.25), (-1.25, 2.5), (3, -2), (0.3, -0.7), (-0.999, 0.001), (90.0, 0.5)]


def test_translate_full_range(dev, oracle):
    fr = _translate_frames()
    t = cuda(fr)
    f32 = fr.astype(np.float32)
    t32 = cuda(f32)
    for strat in ("", "background", "nearest", "wrap"):
        for dx, dy in OFFSETS:
            g = dev.translate(t, (dx, dy), strat, background=65535).cpu().numpy()
            assert np.array_equal(g, np.stack([oracle.translate(f, dx, dy, strat, background=65535) for f in fr])), (strat, dx, dy)
            if strat:  # (translate_to_u16 writes every pixel: no "noborder")
                g = dev.translate_to_u16(t32, (dx, dy), strat, background=65535).cpu().numpy()
                exp = np.stack([u16_as_kernels(oracle.translate(f, dx, dy, strat, background=65535)) for f in f32])
                assert np.array_equal(g, exp), (strat, dx, dy)
    offs = np.array(OFFSETS[:2] * 4, np.float32)[: len(fr)]
    g = dev.translate(t, cuda(offs), "nearest").cpu().numpy()
    assert np.array_equal(g, np.stack([oracle.translate(f, o[0], o[1], "nearest") for f, o in zip(fr, offs)]))


def test_remove_motion_full_range(dev, oracle):
    fr = _translate_frames()
    h = fr.shape[1]
    offs = np.array([OFFSETS[i % len(OFFSETS)] for i in range(len(fr))], np.float32)
    for rows in (h, h - 3):
        g = dev.remove_motion(cuda(fr), cuda(offs), rows=rows).cpu().numpy()
        assert np.array_equal(g, np.stack([oracle.remove_motion(f, o[0], o[1], rows=rows) for f, o in zip(fr, offs)])), rows


def test_gaussian_full_range(dev, oracle):
    fr = _translate_frames()
    for s in (0.5, 0.75, 1.0, 1.7, 2.0, 3.3):
        r = np.stack([oracle.gaussian_filter(f.astype(np.float32), s) for f in fr])
        inputs = (cuda(fr.astype(np.float32)),) + ((cuda(fr),) if s < 2.5 else ())
        for x in inputs:
            g = dev.gaussian_filter(x, s).cpu().numpy()
            assert gaussian_close(g, r), (s, x.dtype)


def test_gaussian_full_range_in_reference_order(dev, oracle, reference_order):
    fr = _translate_frames()
    for s in (0.5, 0.75, 1.0, 1.7, 2.0, 3.3):
        r = np.stack([oracle.gaussian_filter(f.astype(np.float32), s) for f in fr])
        inputs = (cuda(fr.astype(np.float32)),) + ((cuda(fr),) if s < 2.5 else ())
        for x in inputs:
            assert np.array_equal(dev.gaussian_filter(x, s).cpu().numpy().view(np.uint32), r.view(np.uint32)), (s, x.dtype)
