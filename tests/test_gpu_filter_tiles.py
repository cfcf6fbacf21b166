"""GPU: the three branches of the wave-tile kernels' column loader (filter_kernels.hip: load_column), at the smallest shapes that take them.

Frames of 40 x 130 and 40 x 132: tile column 1, wave 1 lies wholly inside the image for every radius (the branch with the row steps on the
scalar side: it needs w > 124 and h >= 36), every other tile takes the range-checked branch, the right tiles and the third row band are
ragged, the fourth wave exits; 130 leaves through 2-byte stores, 132 in 4-pixel pieces.  gaussian_filter, median_filter and filter_chain
against the oracle / against the three kernels, as tests/test_gpu_filters.py holds them at other shapes.

Frames of 2 GiB (a buffer descriptor does not cover them: plain clamped loads): one uint16 frame 32768 x 32768 and one float32 frame
16384 x 32768, made on the device.  Six windows of 96 x 160 pixels - the corners, one in the middle (every window is wider and taller than a
tile: it straddles tile seams), one at the bottom edge - are run again as small frames of their own, which take the other two branches: every
pixel whose taps lie inside the window, and every pixel at an edge the window shares with the image, has the same bits in both.  The two
compute the same expressions in the same order, so no tolerance."""
import numpy as np
import pytest

from librir_amd.synthetic import inject_bad_pixels, s1_noisy_background

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SHAPES = [(40, 130), (40, 132)]
SIGMAS = [0.75, 1.0, 1.7, 2.0]  # radius 1, 2, 3, 4


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture
def reference_order(lib):
    lib.rir_set_gaussian_reference_order(1)
    yield
    lib.rir_set_gaussian_reference_order(0)


# ---- 40 x 130 and 40 x 132 -----------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def small(oracle):
    """per shape: three float32 frames, their uint16 truncation, and the oracle's gaussian of both at every sigma (computed once)"""
    out = {}
    for h, w in SHAPES:
        f32 = (np.random.default_rng(h * 1000 + w).random((3, h, w)) * 16000).astype(np.float32)
        u16 = f32.astype(np.uint16)
        ref = {(s, kind): np.stack([oracle.gaussian_filter(f.astype(np.float32), s) for f in fr]) for s in SIGMAS for kind, fr in (("f32", f32), ("u16", u16))}
        out[(h, w)] = (f32, u16, ref)
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_gaussian_separable_small_tiles(dev, small, shape):
    f32, u16, ref = small[shape]
    for s in SIGMAS:
        for kind, x in (("f32", f32), ("u16", u16)):
            g = dev.gaussian_filter(cuda(x), s).cpu().numpy()
            assert g.dtype == np.float32 and np.allclose(g, ref[(s, kind)], rtol=1e-5, atol=0), (shape, s, kind)


@pytest.mark.parametrize("shape", SHAPES)
def test_gaussian_in_reference_order_small_tiles(dev, small, shape, reference_order):
    f32, u16, ref = small[shape]
    for s in SIGMAS:
        for kind, x in (("f32", f32), ("u16", u16)):
            g = dev.gaussian_filter(cuda(x), s).cpu().numpy()
            assert np.array_equal(g.view(np.uint32), ref[(s, kind)].view(np.uint32)), (shape, s, kind)


@pytest.mark.parametrize("shape", SHAPES)
def test_median_filter_small_tiles(dev, oracle, shape):
    h, w = shape
    fr = np.random.default_rng(h + w).integers(0, 65536, (3, h, w)).astype(np.uint16)
    fr[:, 5, 3:9] = 0
    fr[:, 7:12, w - 2] = 65535
    got = dev.median_filter(cuda(fr)).cpu().numpy()
    assert np.array_equal(got, np.stack([oracle.median_filter(f) for f in fr])), shape


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("sigma", SIGMAS)
def test_filter_chain_small_tiles(dev, shape, sigma):
    h, w = shape
    x = cuda(inject_bad_pixels(s1_noisy_background(3, h, w, seed=w), 40))
    bp = dev.BadPixels(x[0])
    assert bp.count > 0
    fixed = dev.gaussian_filter(bp.correct(x), sigma)
    for off in ((1.25, -2.5), (-3.5, 4.75)):
        for strat in ("nearest", "background"):
            ref = dev.translate_to_u16(fixed, off, strat, background=7)
            out = dev.filter_chain(x, bp, sigma, off, strat, background=7)
            assert torch.equal(out.view(torch.int16), ref.view(torch.int16)), (shape, sigma, off, strat)


# ---- frames of 2 GiB -----------------------------------------------------------------------------------------------------------------

WIN_H, WIN_W = 96, 160


def windows(h, w):
    """(top, left): the four corners, the middle, the bottom edge"""
    return [(0, 0), (0, w - WIN_W), (h - WIN_H, 0), (h - WIN_H, w - WIN_W), (h // 2 - WIN_H // 2, w // 2 - WIN_W // 2), (h - WIN_H, w // 3)]


def check_windows(frame, out, run, margin):
    """out = run(frame) on the whole frame (1, h, w); run on each window alone gives the same bits `margin` pixels inside the window, and up
    to the window's edge where that edge is the image's"""
    _, h, w = frame.shape
    as_bits = {2: torch.int16, 4: torch.int32}[out.element_size()]
    for top, left in windows(h, w):
        alone = run(frame[:, top:top + WIN_H, left:left + WIN_W].contiguous())
        y0, y1 = (0 if top == 0 else margin), (WIN_H if top + WIN_H == h else WIN_H - margin)
        x0, x1 = (0 if left == 0 else margin), (WIN_W if left + WIN_W == w else WIN_W - margin)
        a = out[0, top + y0:top + y1, left + x0:left + x1].contiguous().view(as_bits)
        b = alone[0, y0:y1, x0:x1].contiguous().view(as_bits)
        assert torch.equal(a, b), (top, left, int((a != b).sum()))


@pytest.fixture(scope="module")
def big_u16():
    """uint16 noise over the whole range, 32768 x 32768: w * h = 2^30 pixels, 2 GiB"""
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    x = torch.randint(-32768, 32768, (1, 32768, 32768), dtype=torch.int16, device="cuda", generator=g).view(torch.uint16)
    yield x
    del x
    torch.cuda.empty_cache()


def test_median_filter_2gib_frame(dev, big_u16):
    check_windows(big_u16, dev.median_filter(big_u16), dev.median_filter, margin=1)
    torch.cuda.empty_cache()


def test_filter_chain_2gib_frame(dev, big_u16):
    # taps of output (x, y): filtered columns x - 2, x - 1 and rows y + 2, y + 3, each with its 3 x 3 pixels
    run = lambda x: dev.filter_chain(x, None, 0.75, (1.25, -2.5), "nearest")
    check_windows(big_u16, run(big_u16), run, margin=5)
    torch.cuda.empty_cache()


@pytest.mark.parametrize("sigma,radius", [(0.75, 1), (2.0, 4)])
def test_gaussian_u16_2gib_frame(dev, lib, big_u16, sigma, radius):
    run = lambda x: dev.gaussian_filter(x, sigma)
    for order in (0, 1):
        lib.rir_set_gaussian_reference_order(order)
        try:
            out = run(big_u16)
            check_windows(big_u16, out, run, margin=radius)
        finally:
            lib.rir_set_gaussian_reference_order(0)
        del out
        torch.cuda.empty_cache()


@pytest.mark.parametrize("sigma,radius", [(0.75, 1), (2.0, 4)])
def test_gaussian_f32_2gib_frame(dev, lib, sigma, radius):
    g = torch.Generator(device="cuda")
    g.manual_seed(6)
    x = torch.rand((1, 16384, 32768), dtype=torch.float32, device="cuda", generator=g).mul_(16000.0)
    run = lambda x: dev.gaussian_filter(x, sigma)
    for order in (0, 1):
        lib.rir_set_gaussian_reference_order(order)
        try:
            out = run(x)
            check_windows(x, out, run, margin=radius)
        finally:
            lib.rir_set_gaussian_reference_order(0)
        del out
        torch.cuda.empty_cache()
