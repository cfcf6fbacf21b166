"""Seeded scenes of the bounded-loss tests over the whole 16-bit range (test_lossy_reference_cpu.py, test_gpu_lossy_full_range.py,
hook_cases.py).  The scenes of the older tests stay below 1 300 levels: bits 13-15 of every pixel are zero, the integration-time
condition (h264.cpp:2402) never decides, no value goes through a packed 16-bit half with its top bit set, no square wraps, and no two
histogram bins tie.  These scenes are made so that all of that happens, and so that the reference's statistic stays a number (both
classes populated in every frame: tests/lossy_reference.py refuses a frame where it would not)."""
import numpy as np

_cache = {}


def _frozen(key, make):
    if key not in _cache:
        a = make()
        a.setflags(write=False)
        _cache[key] = a
    return _cache[key]


def surely_both_classes(lossy_rows):
    """pixels in bins strictly below AND strictly above the mode bin of the 16 384-bin histogram (the lowest of the largest bins,
    h264.cpp:1975-1984): neither class of the frame can be empty, wherever in its bin the background falls"""
    hist = np.bincount(np.asarray(lossy_rows).ravel() >> 2, minlength=16384)
    mode = int(np.argmax(hist))
    return bool(hist[:mode].sum() > 0 and hist[mode + 1:].sum() > 0)


def ti_edges(n, h, w, hl, seed):
    """uint16 [n, h, w] (computed once per argument list, not to be written to).

    rows [0, p)        a plateau at 900 .. 903 (one histogram bin: it holds the mode, and both classes), p = max(2, hl // 4)
    row  p             100 + 4 x + (0 .. 3): every pixel alone in a bin below the mode
    rows (p, h)        eight column bands centred on 8 192, 16 384, ... 57 344 and 65 532 (this one reaches 65 535 and clips): a static
                       offset of +-3 per pixel, +-2 of noise per frame and a drift of -1, 0, +1 with period 3 - pixels cross the boundary of
                       the top three bits while they stay within budgets of 6 / 2 of their reference
    rows hl - 2, hl - 1  rise by 47 000 from frame n // 2 on (clipped at 65 535): differences whose square wraps 32 bits, then values near
                       the top of the range for as long as any ring"""
    def make():
        assert hl >= 6 and w >= 8 and 100 + 4 * w + 3 < 880, "the scene's layout needs hl >= 6 and 8 <= w < 195"
        rng = np.random.default_rng(seed)
        p = max(2, hl // 4)
        band = np.arange(w) * 8 // w
        centre = np.where(band < 7, 8192 * (band + 1), 65532)
        static = centre[None, :] + rng.integers(-3, 4, (h, w))
        arr = static[None] + rng.integers(-2, 3, (n, h, w)) + (np.arange(n) % 3 - 1)[:, None, None]
        arr[:, :p] = 900 + rng.integers(0, 4, (n, p, w))
        arr[:, p] = 100 + 4 * np.arange(w)[None, :] + rng.integers(0, 4, (n, w))
        arr[n // 2:, hl - 2:hl] += 47000
        arr = np.clip(arr, 0, 65535).astype(np.uint16)
        # at every shape: the plateau holds the mode, with pixels on both sides of it (the precondition of the constant-budget form,
        # and what keeps the reference's statistic a number)
        assert all(np.argmax(np.bincount(f[:hl].ravel() >> 2)) == 900 >> 2 and surely_both_classes(f[:hl]) for f in arr), (n, h, w, hl, seed)
        return arr

    return _frozen(("ti_edges", n, h, w, hl, seed), make)


MODE_TIE_LOW, MODE_TIE_HIGH = 4000, 30000  # first levels of the two tied bins


def mode_tie(n, h, w, seed, hl=None):
    """uint16 [n, h, w] (computed once per argument list, not to be written to; with hl the scene is that of the first hl rows - the
    lossy ones - and the rows below them hold anything): h * w // 4 pixels at 4 000 .. 4 003 and as many at
    30 000 .. 30 003 (30 004 .. 30 007 in odd frames) - two bins that are the joint maximum of the histogram in every frame - and every
    other pixel alone in a bin of its own, below, between and above them; the populations are scattered over the frame, and every pixel
    moves inside its bin from frame to frame.  get_background keeps the LOWER bin (h264.cpp:1979): the background is 4 001, so with
    budgets 6 / 0 the pixels of the lower bin that stand at 4 002 or 4 003 are foreground and are refreshed whenever they move - with the
    tie broken the other way they would be background, within a budget of 6, and kept."""
    def make():
        rng = np.random.default_rng(seed)
        rows = h if hl is None else hl
        s, q = rows * w, rows * w // 4
        others = s - 2 * q
        lo_bin, hi_bin = MODE_TIE_LOW >> 2, MODE_TIE_HIGH >> 2
        free = np.array([b for b in range(8, 16384) if not (lo_bin - 1 <= b <= lo_bin + 1 or hi_bin - 1 <= b <= hi_bin + 2)])
        assert others <= len(free)
        bins = free[np.linspace(0, len(free) - 1, others).astype(np.int64)]
        assert len(set(bins.tolist())) == others and (bins < lo_bin).any() and (bins > hi_bin + 1).any() and ((bins > lo_bin) & (bins < hi_bin)).any()
        base = np.concatenate([np.full(q, MODE_TIE_LOW), np.full(q, MODE_TIE_HIGH), bins * 4])
        base = base[rng.permutation(s)]
        arr = base[None, :] + rng.integers(0, 4, (n, s))
        arr[1::2] += np.where(base == MODE_TIE_HIGH, 4, 0)[None, :]
        for i in range(n):  # the two bins tie, and nothing else comes near
            hist = np.bincount(arr[i] >> 2, minlength=16384)
            assert np.flatnonzero(hist == q).tolist() == [lo_bin, hi_bin + i % 2] and np.sort(hist)[-3] == 1, (n, h, w, seed, i)
        rest = rng.integers(0, 65536, (n, h - rows, w))
        return np.concatenate([arr.reshape(n, rows, w), rest], axis=1).astype(np.uint16)

    return _frozen(("mode_tie", n, h, w, seed, hl), make)
