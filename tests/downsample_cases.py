"""Adaptive temporal downsampling (max-hold): the oracle the CPU and GPU tests check against, a second, deliberately naive restatement to pin
it, and the seeded scenes.  Both restate the contract of include/rir_amd_device.h (rir_downsampler_push_device) - the reference's
VideoDownsampler with the documented deviations - in plain Python floats, one operation per statement, so that every rounding is the C
code's; numpy is used for integer work only (the exact sums and the maxima)."""
import math
from collections import namedtuple

import numpy as np

HISTORY = 96
EVENTS = {40: 300, 41: 300, 150: 200, 151: 400, 152: 100, 230: 500}  # frame -> levels added to a block
PARAMS = [(2, .5), (4, .75), (10, .9), (10, 0.), (10, 1.)]  # (factor, factor_std)
METHODS = (1, 2)
SCENES = [(12, 20, 12), (12, 20, 9), (33, 70, 33), (33, 70, 30)]  # (h, w, lossy_height)
FRAMES = 260  # method 1 leaves its warm-up only after 97 images

Result = namedtuple("Result", "images positions timestamps stats keep sums")


def scene(n, h, w, seed=5, events=EVENTS):
    """the S1 recipe without drift, bg * 1000 + 10 + N(0, sqrt(0.5)), plus block events on rows 2 .. h / 2, columns 3 .. w / 2"""
    rng = np.random.default_rng(seed)
    bg = rng.random((h, w)) * 1000
    out = np.empty((n, h, w), np.uint16)
    for i in range(n):
        out[i] = (bg + 10 + rng.normal(0, np.sqrt(0.5), (h, w))).astype(np.uint16)
        if i in events:
            out[i, 2:h // 2, 3:w // 2] += np.uint16(events[i])
    return out


def stamps(n, first=7, step=20000000):
    return np.arange(n, dtype=np.int64) * step + first


# ---- IEEE double operations that Python would raise on ------------------------------------------------------------------------------
def _sqrt(v):
    return math.sqrt(v) if v >= 0.0 else math.nan


def _div(a, b):
    if b != 0.0:
        return a / b
    if a == 0.0 or a != a:
        return math.nan
    return math.copysign(math.inf, a) * math.copysign(1.0, b)


def pair_sums(frames, size, prev=None):
    """[n][2] int64: sum |d| and sum d^2 over the first `size` pixels of every image and the one before it (prev ahead of the first; zeros
    without it)"""
    n = frames.shape[0]
    flat = frames.reshape(n, frames.shape[1] * frames.shape[2])[:, :size].astype(np.int64)
    out = np.zeros((n, 2), np.int64)
    before = None if prev is None else prev.reshape(-1)[:size].astype(np.int64)
    for i in range(n):
        if before is not None:
            d = np.abs(flat[i] - before)
            out[i, 0] = d.sum()
            out[i, 1] = (d * d).sum()
        before = flat[i]
    return out


def statistic(x, q, size):
    x = float(int(x))
    q = float(int(q))
    xx = x * x
    m = xx / float(size)
    r = q - m
    if r < 0.0:
        return 0.0
    v = r / float(size - 1)
    return math.sqrt(v)


def mean_std(p):
    x = 0.0
    x2 = 0.0
    for v in p:
        sq = v * v
        x = x + v
        x2 = x2 + sq
    n = float(len(p))
    mean = _div(x, n)
    xx = x * x
    m = _div(xx, n)
    r = x2 - m
    v = _div(r, float(len(p) - 1))
    return mean, _sqrt(v)


class Recurrence:
    """the keep / drop decision, image by image, from the statistics"""

    def __init__(self, factor, factor_std, method):
        self.factor, self.method = int(factor), int(method)
        self.part = min(max(int(factor_std * HISTORY), 0), HISTORY - 1)
        self.history = []
        self.i = 0
        self.last_added = 0
        self.count = 0

    def _slide(self, stat):
        if len(self.history) < HISTORY:
            self.history.append(stat)
        else:
            self.history = self.history[1:] + [stat]

    def _method1(self, stat):
        i, factor = self.i, self.factor
        if len(self.history) < HISTORY:
            if i > 0:
                self.history.append(stat)
            return i % factor == 0
        val = sorted(self.history)[self.part]
        mean, std = mean_std(self.history)
        half = 0.5 * std
        low = mean - half
        nothing = stat < low
        if i - self.last_added >= 2 * factor:
            nothing = False
        keep = (stat > val or i - self.last_added >= factor) and not nothing
        ten = 10 * std
        high = mean + ten
        if stat < high:
            self._slide(stat)
        return keep

    def _method2(self, stat):
        i, factor = self.i, self.factor
        if i == 0:
            return True
        grid = i % factor == 0
        if len(self.history) < 10:
            self.history.append(stat)
            return grid
        mean, std = mean_std(self.history)
        ratio = _div(std, mean)
        two = 2 * std
        quiet = mean + two
        nothing = ratio < 0.1 and stat < quiet
        half = 0.5 * std
        above = mean + half
        keep = grid or (not nothing and stat > above)
        five = 5 * std
        high = mean + five
        low = mean - std
        if (stat < high and stat > low) or grid:
            self._slide(stat)
        return keep

    def step(self, stat):
        if self.factor == 1:
            keep = True
        else:
            keep = self._method1(stat) if self.method == 1 else self._method2(stat)
            if keep:
                self.last_added = self.i
        self.i += 1
        self.count += int(keep)
        return keep


def decide(sums, size, factor, factor_std, method, rec=None):
    """keep flags and statistics of images whose pair sums are given -> (keep bool [n], stats float64 [n])"""
    rec = Recurrence(factor, factor_std, method) if rec is None else rec
    keep, stats = [], []
    for x, q in sums:
        stat = statistic(x, q, size) if rec.i > 0 and rec.factor != 1 else 0.0
        stats.append(stat)
        keep.append(rec.step(stat))
    return np.array(keep, bool), np.array(stats, np.float64)


def oracle(frames, timestamps, factor, factor_std, lossy_height=None, method=1):
    """one push of the whole sequence -> Result"""
    frames = np.asarray(frames)
    n, h, w = frames.shape
    lossy_height = h if lossy_height is None else lossy_height
    size = w * lossy_height
    sums = pair_sums(frames, size)
    keep, stats = decide(sums, size, factor, factor_std, method)
    positions = np.flatnonzero(keep).astype(np.int32)
    images = np.empty((len(positions), h, w), np.uint16)
    start = 0
    for k, at in enumerate(positions):
        images[k] = frames[at]
        if factor != 1:
            images[k, :lossy_height] = frames[start:at + 1, :lossy_height].max(0)
        start = at + 1
    return Result(images, positions, np.asarray(timestamps, np.int64)[positions], stats, keep, sums)


def naive(frames, timestamps, factor, factor_std, lossy_height=None, method=1):
    """The same contract written as the reference's loop is: image by image, with an explicit max_im, prev and a list the callback
    appends to; the history is a plain list, the part-th smallest entry found by repeated removal of the minimum."""
    frames = np.asarray(frames)
    n, h, w = frames.shape
    lossy_height = h if lossy_height is None else lossy_height
    size = w * lossy_height
    part = int(factor_std * 96)
    part = 0 if part < 0 else 95 if part > 95 else part
    emitted = []  # (image, time stamp, position)
    stats = []
    history = []
    max_im = np.zeros(h * w, np.uint16)
    prev = None
    last_added = 0

    def emit(image, i):
        emitted.append((image.reshape(h, w).copy(), int(timestamps[i]), i))

    def hold(img):
        max_im[:size] = np.maximum(max_im[:size], img[:size])
        max_im[size:] = img[size:]

    def moments(values):
        s = 0.0
        s2 = 0.0
        for v in values:
            s += v
            s2 += v * v
        count = len(values)
        inner = (s2 - _div(s * s, float(count)))
        return _div(s, float(count)), _sqrt(_div(inner, float(count - 1)))

    for i in range(n):
        img = frames[i].reshape(-1)
        if factor == 1:
            stats.append(0.0)
            emit(img, i)
            continue
        stat = 0.0
        if i > 0:
            d = np.abs(img[:size].astype(np.int64) - prev[:size].astype(np.int64))
            x = float(int(d.sum()))
            x_squared = float(int((d * d).sum()))
            radicand = (x_squared - (x * x) / size)
            stat = math.sqrt(radicand / (size - 1)) if radicand >= 0 else 0.0
        stats.append(stat)
        keep = False
        if method == 2 and i == 0:
            emit(img, i)
            prev = img
            continue
        hold(img)
        if method == 1:
            if len(history) < 96:
                if i > 0:
                    history.append(stat)
                keep = i % factor == 0
            else:
                pool = list(history)
                for _ in range(part):
                    pool.remove(min(pool))
                val = min(pool)
                mean, std = moments(history)
                nothing = stat < mean - 0.5 * std
                if i - last_added >= factor * 2:
                    nothing = False
                keep = (stat > val or i - last_added >= factor) and not nothing
                if stat < mean + 10 * std:
                    del history[0]
                    history.append(stat)
        else:
            if len(history) < 10:
                history.append(stat)
                keep = i % factor == 0
            else:
                mean, std = moments(history)
                nothing = _div(std, mean) < 0.1
                if nothing:
                    nothing = stat < mean + 2 * std
                keep = i % factor == 0 or (not nothing and stat > mean + 0.5 * std)
                if (stat < mean + 5 * std and stat > mean - std) or i % factor == 0:
                    if len(history) >= 96:
                        del history[0]
                    history.append(stat)
        if keep:
            emit(max_im, i)
            last_added = i
            max_im[:] = 0
        prev = img
    images = np.stack([e[0] for e in emitted]) if emitted else np.empty((0, h, w), np.uint16)
    return Result(images, np.array([e[2] for e in emitted], np.int32), np.array([e[1] for e in emitted], np.int64),
                  np.array(stats, np.float64), None, None)


def bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def same(got, exp, what=""):
    """two Results agree: positions, time stamps, statistics as raw bits, images"""
    assert np.array_equal(got.positions, exp.positions), (what, "positions", got.positions, exp.positions)
    assert np.array_equal(got.timestamps, exp.timestamps), (what, "timestamps")
    assert np.array_equal(bits(got.stats), bits(exp.stats)), (what, "stats", np.flatnonzero(bits(got.stats) != bits(exp.stats))[:5])
    assert got.images.shape == exp.images.shape and got.images.dtype == exp.images.dtype, (what, got.images.shape, exp.images.shape)
    if not np.array_equal(got.images, exp.images):
        bad = np.argwhere(got.images != exp.images)[:5]
        raise AssertionError("%s images differ at %s: got %s, expected %s" % (what, bad.tolist(), got.images[tuple(bad.T)], exp.images[tuple(bad.T)]))
