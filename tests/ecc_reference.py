"""Helper of the ECC probe tests (test_ecc_reference_cpu.py, test_gpu_registration_probe.py): a smooth deterministic scene that is
not symmetric in x and y, a float64 restatement of ONE iteration of translation-only ECC (independent of oracle/rir_oracle.c and
more precise than it: the distance between the two is the measured rounding sensitivity of a case), and the lists of cases - the
smallest shapes at which each mechanism of the kernels' pixel loop can go wrong, starts of both signs, on single axes, on
half-integers (rint ties) and in (-1, 0), blocky masks, and the cases in which the alignment must fail."""
import math

import numpy as np


def scene(h, w, seed, shift=(0.0, 0.0)):
    """float64; scene(.., shift=(-tx, -ty)) is the scene moved by (tx, ty)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    yy = yy + shift[1]
    xx = xx + shift[0]
    img = 0.3 * xx / w + 0.2 * yy / h
    for _ in range(6):
        cx, cy = rng.uniform(0, w), rng.uniform(0, h)
        s = rng.uniform(0.15, 0.4) * min(h, w) + 1.0
        a = rng.uniform(0.3, 1.0)
        img += a * np.exp(-((xx - cx) ** 2 / (2 * s * s) + (yy - cy) ** 2 / (2 * (0.7 * s) ** 2)))
    return img


def unit_range(a):
    """min-max normalisation, in the precision of `a`"""
    return (a - a.min()) / (a.max() - a.min())


def reflect101(n):
    """indices of the left / upper and right / lower neighbours with reflect-101 borders"""
    i = np.arange(n)
    lo = np.where(i > 0, i - 1, 1 if n > 1 else 0)
    hi = np.where(i < n - 1, i + 1, n - 2 if n > 1 else 0)
    return lo, hi


def gradients32(img):
    """central differences [-1/2 0 1/2] in float32 with reflect-101 borders -> (gx, gy)"""
    img = np.ascontiguousarray(img, dtype=np.float32)
    h, w = img.shape
    xl, xr = reflect101(w)
    yu, yd = reflect101(h)
    half = np.float32(0.5)
    gx = half * img[:, xr] - half * img[:, xl]
    gy = half * img[yd, :] - half * img[yu, :]
    assert gx.dtype == np.float32 and gy.dtype == np.float32
    return gx, gy


def _bilinear0(a, x0, y0, fx, fy):
    """float64 bilinear interpolation of the float32 array `a` at (x0 + fx, y0 + fy), taps outside the image are zero"""
    h, w = a.shape

    def tap(xi, yi):
        inside = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
        return np.where(inside, a[np.clip(yi, 0, h - 1), np.clip(xi, 0, w - 1)].astype(np.float64), 0.0)

    v00, v01, v10, v11 = tap(x0, y0), tap(x0 + 1, y0), tap(x0, y0 + 1), tap(x0 + 1, y0 + 1)
    top = v00 + fx * (v01 - v00)
    bot = v10 + fx * (v11 - v10)
    return top + fy * (bot - top)


def ecc_step64(templ, image, tx, ty, mask=None):
    """One iteration of the forward additive ECC scheme (translation only) from (tx, ty): gradients in float32, sample coordinates
    float32(x) + float32(tx), validity (and the mask) at np.rint of the sample coordinate, interpolation and the 15 sums in float64,
    the 2x2 solve of orc_ecc_translation.  -> (tx', ty', rho, n) with tx', ty' rounded to float32, or None where the oracle returns -1
    (n < 1, det == 0, NaN, lambda_d <= 0)."""
    templ = np.ascontiguousarray(templ, dtype=np.float32)
    image = np.ascontiguousarray(image, dtype=np.float32)
    h, w = image.shape
    gx, gy = gradients32(image)
    sx = np.arange(w, dtype=np.float32) + np.float32(tx)
    sy = np.arange(h, dtype=np.float32) + np.float32(ty)
    assert sx.dtype == np.float32 and sy.dtype == np.float32
    nx, ny = np.rint(sx).astype(np.int64), np.rint(sy).astype(np.int64)
    valid = ((ny >= 0) & (ny < h))[:, None] & ((nx >= 0) & (nx < w))[None, :]
    if mask is not None:
        m = np.asarray(mask)
        valid = valid & (m[np.clip(ny, 0, h - 1)][:, np.clip(nx, 0, w - 1)] != 0)
    flx, fly = np.floor(sx), np.floor(sy)
    x0 = np.broadcast_to(flx.astype(np.int64)[None, :], (h, w))
    y0 = np.broadcast_to(fly.astype(np.int64)[:, None], (h, w))
    fx = np.broadcast_to((sx - flx).astype(np.float64)[None, :], (h, w))
    fy = np.broadcast_to((sy - fly).astype(np.float64)[:, None], (h, w))
    sel = np.nonzero(valid)
    n = float(len(sel[0]))
    if n < 1.0:
        return None
    x0, y0, fx, fy = x0[sel], y0[sel], fx[sel], fy[sel]
    im = _bilinear0(image, x0, y0, fx, fy)
    dx = _bilinear0(gx, x0, y0, fx, fy)
    dy = _bilinear0(gy, x0, y0, fx, fy)
    t = templ[sel].astype(np.float64)
    S = lambda v: math.fsum(v.tolist())  # noqa: E731  (exactly rounded sums)
    s1, s2, s3, s4, s5 = S(im), S(im * im), S(t), S(t * t), S(t * im)
    s6, s7, s8, s9, s10 = S(dx), S(dy), S(dx * dx), S(dx * dy), S(dy * dy)
    s11, s12, s13, s14 = S(dx * im), S(dy * im), S(dx * t), S(dy * t)
    mi, mt = s1 / n, s3 / n
    img_norm2, tmp_norm2, corr = s2 - n * mi * mi, s4 - n * mt * mt, s5 - n * mt * mi
    h00, h01, h11 = s8, s9, s10
    ip0, ip1, tp0, tp1 = s11 - mi * s6, s12 - mi * s7, s13 - mt * s6, s14 - mt * s7
    det = h00 * h11 - h01 * h01
    with np.errstate(all="ignore"):  # (IEEE semantics as in C: sqrt of a negative is NaN, x / 0 is +-inf or NaN)
        rho = float(np.float64(corr) / (np.sqrt(np.float64(img_norm2)) * np.sqrt(np.float64(tmp_norm2))))
    if not (det != 0.0) or math.isnan(rho):
        return None
    i00, i01, i11 = h11 / det, -h01 / det, h00 / det
    iph0, iph1 = i00 * ip0 + i01 * ip1, i01 * ip0 + i11 * ip1
    lambda_n = img_norm2 - (ip0 * iph0 + ip1 * iph1)
    lambda_d = corr - (tp0 * iph0 + tp1 * iph1)
    if lambda_d <= 0.0:
        return None
    lam = lambda_n / lambda_d
    e0, e1 = lam * tp0 - ip0, lam * tp1 - ip1
    ntx = np.float32(float(np.float32(tx)) + (i00 * e0 + i01 * e1))
    nty = np.float32(float(np.float32(ty)) + (i01 * e0 + i11 * e1))
    return float(ntx), float(nty), rho, int(n)


def oracle_step(oracle, templ, image, tx, ty, mask=None, iterations=1):
    """`iterations` fixed iterations of the oracle from (tx, ty) -> (tx', ty', rho), or None where it fails"""
    try:
        r = oracle.ecc_translation(templ, image, (tx, ty), mask=mask, max_iter=iterations, eps=0.0)
    except RuntimeError:
        return None
    return r[0], r[1], r[2]


# ---- the cases -----------------------------------------------------------------------------------------------------------------
# (h, w): the smallest shapes at which each mechanism of the pixel loop can go wrong
PROBE_SHAPES = [
    (5, 3), (9, 13),                # fewer pixels than a wave / a workgroup; a wave spans many lines
    (4, 63), (17, 64), (33, 65),    # around a 64-pixel line
    (16, 257),                      # around a 256-pixel strip
    (255, 257),                     # 65 535 pixels: 256 workgroups, the last one short
    (256, 257),                     # just past 65 536 pixels: some threads take a second pixel
    (300, 701),                     # past 3 x 65 536 pixels: a second round with a tail
    (67, 83),                       # the shape the suite already uses
]
# both signs, single axes, integers, half-integers (rint ties), -1 < t < 0
STARTS = [(0.0, 0.0), (3.0, -2.0), (2.5, -1.5), (3.5, -0.5), (-0.25, 0.75), (-1.0, 0.0), (0.0, -1.0), (4.0, 0.0), (0.0, -3.0), (-2.6, 3.3)]
DEGENERATE_SHAPES = [(2, 2), (2, 7), (7, 2)]  # det == 0 at every start: one gradient vanishes everywhere
ILL_CONDITIONED_SHAPE = (3, 5)  # succeeds with a 21 px step: failure agreement only
# (shape, start) whose first step exceeds the 8 px conditioning cap on this scene - 22.6, 9.3 and 8.3 px, masked or not: far from the
# solution on a small image.  Both references agree on them to the last digit of float32; they stay in the grid and in every comparison,
# and the cap is asserted for everything else.
OVER_CAP = {((9, 13), (0.0, -3.0)), ((17, 64), (3.0, -2.0)), ((4, 63), (3.0, -2.0))}
STEP_CAP = 8.0
SCENE_SEED = 7
IMAGE_SHIFT = (2.75, -1.5)

_inputs = {}


def probe_inputs(shape):
    """(template, image) of a probe shape, float32 (computed once per shape, not to be written to)"""
    if shape not in _inputs:
        h, w = shape
        t = scene(h, w, SCENE_SEED).astype(np.float32)
        i = scene(h, w, SCENE_SEED, IMAGE_SHIFT).astype(np.float32)
        t.setflags(write=False), i.setflags(write=False)
        _inputs[shape] = (t, i)
    return _inputs[shape]


def has_mask(shape):
    return shape[0] >= 17 and shape[1] >= 64


_masks = {}


def blocky_mask(shape, seed=21):
    """uint8 (h, w): random 8x8 blocks, 70 % of them in; one masked-out block touches each of the four borders"""
    key = (shape, seed)
    if key not in _masks:
        h, w = shape
        rng = np.random.default_rng(seed)
        bh, bw = -(-h // 8), -(-w // 8)
        blocks = rng.random((bh, bw)) < 0.7
        blocks[0, bw // 3] = blocks[bh - 1, (2 * bw) // 3] = blocks[bh // 3, 0] = blocks[(2 * bh) // 3, bw - 1] = False
        m = np.kron(blocks, np.ones((8, 8)))[:h, :w].astype(np.uint8)
        m.setflags(write=False)
        _masks[key] = m
    return _masks[key]


def start_key(start):
    return "%g,%g" % start


def probe_cases():
    """every (shape, start, masked) of the grid: probe and degenerate shapes, the ill-conditioned one, and two starts without overlap"""
    cases = []
    for shape in PROBE_SHAPES + DEGENERATE_SHAPES + [ILL_CONDITIONED_SHAPE]:
        w = shape[1]
        for start in STARTS + [(float(w + 1), 0.0), (-float(w + 1), 0.5)]:
            cases.append((shape, start, False))
            if has_mask(shape):
                cases.append((shape, start, True))
    return cases


def listed_failure(shape, start):
    """the cases that must fail in both CPU references and in the library"""
    return shape in DEGENERATE_SHAPES or abs(start[0]) >= shape[1] + 1 or (shape == (4, 63) and start in ((0.0, -3.0), (-2.6, 3.3)))


_grid = {}


def reference_grid(oracle):
    """{(shape, start, masked): (oracle's (tx, ty, rho) or None, ecc_step64's (tx, ty, rho, n) or None)} over probe_cases(), once"""
    if not _grid:
        for shape, start, masked in probe_cases():
            t, i = probe_inputs(shape)
            m = blocky_mask(shape) if masked else None
            _grid[(shape, start, masked)] = (oracle_step(oracle, t, i, start[0], start[1], m), ecc_step64(t, i, start[0], start[1], m))
    return _grid


def probe_bounds(o, r):
    """the bound of a succeeding case from its oracle-to-float64 distance: (tol_t, tol_cc, d_cpu_t, d_cpu_cc)"""
    d_t = max(abs(o[0] - r[0]), abs(o[1] - r[1]))
    d_cc = abs(o[2] - r[2])
    return max(8 * d_t, FLOOR_T), max(8 * d_cc, FLOOR_CC), d_t, d_cc


FLOOR_T, FLOOR_CC = 1e-6, 1e-7  # px, correlation: the floors of the per-case bounds (and the most the two CPU references may differ)

# fixed-iteration alignments with a known answer: (h, w), true translation of the image against the template
TRUTH_SHAPES = [(129, 511), (300, 701)]
TRUTHS = [(2.75, -1.25), (-3.2, 0.3), (0.4, 4.1)]
TRUTH_ITERATIONS = 12


def truth_pair(shape, truth, seed=SCENE_SEED):
    """(template, image), min-max normalised float32: the image is the scene moved by `truth`"""
    h, w = shape
    t = unit_range(scene(h, w, seed)).astype(np.float32)
    i = unit_range(scene(h, w, seed, (-truth[0], -truth[1]))).astype(np.float32)
    return t, i


def device_one_iteration(templ, image, start, mask=None, iterations=1):
    """find_transform_ecc_translation from `start` with a fixed number of iterations -> (tx, ty, cc), or None where it raises"""
    from librir_amd.registration import find_transform_ecc_translation

    wm = np.eye(2, 3, dtype=np.float32)
    wm[0, 2], wm[1, 2] = start
    try:
        cc, out = find_transform_ecc_translation(templ, image, wm, iterations, 0.0, mask)
    except RuntimeError:
        return None
    return float(out[0, 2]), float(out[1, 2]), float(cc)


def device_probe_grid():
    """the library's answer to every case of probe_cases(), in that order (the process' environment decides which kernels give it)"""
    out = []
    for shape, start, masked in probe_cases():
        t, i = probe_inputs(shape)
        out.append(device_one_iteration(t, i, start, blocky_mask(shape) if masked else None))
    return out


def to_hex(results):
    return [None if r is None else [float(v).hex() for v in r] for r in results]


if __name__ == "__main__":  # the child process of the two-launches-per-iteration probe: the grid as one line of JSON
    import json
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print(json.dumps(to_hex(device_probe_grid())))
