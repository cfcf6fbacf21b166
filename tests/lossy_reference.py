"""Helper of the bounded-loss tests (test_lossy_reference_cpu.py, test_gpu_lossy_full_range.py): a plain numpy restatement of the
reference's bounded-loss step, written from its text - h264.cpp:2253-2424 addImageLossyNoCamera, :2426-2607 addLoss, :1526-1615
RunningAverage2, :1955-2036 get_background and stdDev - and from nothing else: independent of oracle/rir_oracle.c and of the kernels,
and unlike both in structure.  Integers are int64, the statistics float64; the running average is a ring of EFFECTIVE values per pixel (a
reset overwrites the pixel's whole column), which is what RunningAverage2's sums / consts bookkeeping amounts to (:1572-1578: the
constant entries are always the oldest ones of the column).

An empty class or a negative radicand makes the reference's statistic NaN, and the conversion of that NaN to an integer is the
platform's business: outside this restatement's domain.  It REFUSES such a frame (OutOfDomain); the NaN tests of test_gpu_lossy.py and
test_gpu_lossy_spec.py keep that behaviour."""
import math

import numpy as np

WINDOW = 40  # running_average_frames (:2338): entries of the window of statistics; the statistic is split by class once it is full


class OutOfDomain(ValueError):
    """the frame makes the reference's statistic NaN"""


def wrap32(x):
    """int64 -> the value an int holds after a product that overflowed (two's complement, as `diff * diff` at :2003 does in practice)"""
    return ((x + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def round_half_away(x):
    """std::round of a double that is >= 0 (x - floor(x) is exact)"""
    f = math.floor(x)
    return int(f) + (1 if x - f >= 0.5 else 0)


class ReferenceLossy:
    """Stateful; the constructor's parameters, step(), last_errors() and set_errors() are those of oracle.pyoracle.OracleLossy.  The
    small methods below the constructor are the places where the deliberately wrong variants of test_lossy_reference_cpu.py differ."""

    def __init__(self, w, h, lossy_height=None, low_err=6, high_err=2, std_factor=5.0, running_average=32, subtract_min=False):
        self.w, self.h = int(w), int(h)
        self.hl = self.h if lossy_height is None else int(lossy_height)
        self.low_err, self.high_err, self.std_factor = int(low_err), int(high_err), float(std_factor)
        self.ra = min(int(running_average), 64)  # (:1774)
        self.subtract_min = bool(subtract_min)
        self.frames = 0
        self.min = 0
        self.ref = self.prev = self.last_dl = None  # refT, prevT (lossy rows, int64), lastDL (whole frame)
        self.ring = np.zeros((max(self.ra, 0), self.hl, self.w), np.int64)  # effective values; the oldest image is at `oldest`
        self.ring_len = self.oldest = 0
        self.first_std = None                       # firstStdDevs (one entry: :2339)
        self.window = []                            # stdDevs: (background, foreground) pairs
        self.last = (self.low_err, self.high_err, 0)
        # what the tests ask of a scene, counted here because only the step knows it
        self.by_top_bits = 0          # pixels within their budget that the integration-time condition alone refreshed
        self.both_sides_full_ring = 0  # frames, after the ring was full, in which some pixels were kept and some were not
        self.max_ring_sum = 0
        self.surely_both_classes = []  # per stepped frame: pixels in bins strictly below AND strictly above the mode bin
        self.backgrounds = []          # per stepped frame

    # ---- the places a wrong kernel could differ ------------------------------------------------------------------------------------
    def mode_bin(self, hist):
        return int(np.argmax(hist))  # the first of the largest: strict > at :1979

    def square(self, diff):
        return wrap32(diff * diff)  # int * int at :2003 / :2022 / :2028

    def same_integration_time(self, raw, t):
        return (self.last_dl[: self.hl] >> 13) == (raw >> 13)  # :2402

    def refresh_last_dl(self, frame, add_loss):
        self.last_dl = frame.copy()  # :2416 and :2593

    # ---- the step ------------------------------------------------------------------------------------------------------------------
    def _less_min(self, raw):
        return np.maximum(raw - self.min, 0) if self.subtract_min else raw.copy()  # :2320-2330

    def _stat(self, diff, sel, what):
        n = int(sel.sum())
        if n == 0:
            raise OutOfDomain("no pixel in the %s class" % what)
        a = np.float64(int(diff[sel].sum()))
        b = np.float64(int(self.square(diff[sel]).sum()))
        rad = a * a - b
        if rad < 0:
            raise OutOfDomain("negative radicand in the %s class" % what)
        return float(np.sqrt(rad) / n)

    def set_errors(self, low_err, high_err, std_factor=None):
        self.low_err, self.high_err = int(low_err), int(high_err)
        if std_factor is not None:
            self.std_factor = float(std_factor)

    def last_errors(self):
        return self.last

    def step(self, img, add_loss=False):
        frame = np.asarray(img).astype(np.int64).reshape(self.h, self.w)
        hl = self.hl
        raw = frame[:hl]
        out = frame.copy()
        if self.frames == 0:  # :2273-2312, :2446-2489
            self.last_dl = frame.copy()
            if self.subtract_min:
                self.min = int(raw.min())
            t = self._less_min(raw)
            self.ref, self.prev = t.copy(), t.copy()
            self.last = (self.low_err, self.high_err, 0)
            self.frames = 1
            out[:hl] = t
            return out.astype(np.uint16)
        t = self._less_min(raw)
        hist = np.bincount((raw >> 2).ravel(), minlength=16384)
        mb = self.mode_bin(hist)
        background = mb * 4 + 1  # :1990
        self.backgrounds.append(background)
        self.surely_both_classes.append(bool(hist[:mb].sum() > 0 and hist[mb + 1:].sum() > 0))
        fg = raw > background
        diff = np.abs(t - self.prev)
        if len(self.window) < WINDOW:  # :2340-2343
            s = self._stat(diff, np.ones_like(fg), "only")
            std = (s, s)
        else:
            std = (self._stat(diff, ~fg, "background"), self._stat(diff, fg, "foreground"))
        if self.first_std is None:
            self.first_std = std
        if len(self.window) == WINDOW:
            self.window.pop(0)
        self.window.append(std)
        mean = list(self.first_std)  # :2358-2370: the first statistic is in the sum twice
        for e in self.window:
            mean[0] += e[0]
            mean[1] += e[1]
        mean = [m / (len(self.window) + 1) for m in mean]
        if add_loss:  # :2549-2553
            d_low = 0.0 if std[0] < mean[0] else std[0] - mean[0]
            d_high = 0.0 if std[1] < mean[1] else std[1] - mean[1]
        else:  # :2372-2373
            d_low, d_high = abs(std[0] - mean[0]), abs(std[1] - mean[1])
        high = self.high_err - round_half_away(d_high * self.std_factor)
        low = self.low_err - round_half_away(d_low * self.std_factor)
        high = max(high, 0)
        low = max(low, high)
        self.last = (low, high, background)
        ring_was_full = self.ring_len == self.ra
        if self.ra > 0:  # addImage (:1559-1594): the new image joins, the oldest one leaves a full ring
            if ring_was_full:
                self.ring[self.oldest] = t
                self.oldest = (self.oldest + 1) % self.ra
            else:
                self.ring[self.ring_len] = t
                self.ring_len += 1
        within = np.abs(t - self.ref) <= np.where(fg, high, low)
        keep = within.copy()
        if not add_loss:
            keep &= self.same_integration_time(raw, t)
        self.by_top_bits += int((within & ~keep).sum())
        if keep.any() and not keep.all() and ring_was_full:
            self.both_sides_full_ring += 1
        self.ref = np.where(keep, self.ref, t)
        if self.ra > 0:
            ys, xs = np.nonzero(~keep)
            self.ring[: self.ring_len, ys, xs] = t[ys, xs]  # resetPixel (:1609-1614): the whole column
            sums = self.ring[: self.ring_len].sum(axis=0)
            self.max_ring_sum = max(self.max_ring_sum, int(sums.max()))
            res = sums // self.ring_len  # pixel (:1600-1603)
        else:
            res = self.ref  # (:2405 where kept, the pixel itself where not)
        self.prev = res.copy()  # :2415
        self.refresh_last_dl(frame, add_loss)
        out[:hl] = res
        self.frames += 1
        return out.astype(np.uint16)


def track(make, arr, pattern="lossy", changes=None):
    """frames, low and high errors of `make()` (a ReferenceLossy or an OracleLossy) over the frames of arr.  pattern: "lossy" (every
    frame through add_image_lossy), "loss" (add_loss from the second frame on) or "interleaved" (the entry point switches every 7
    frames); changes: {frame: (low, high, std_factor)} applied before that frame.  -> (frames [n,h,w] uint16, lows, highs, the object)"""
    L = make()
    exp, lo, hi = [], [], []
    for i in range(arr.shape[0]):
        if changes and i in changes:
            L.set_errors(*changes[i])
        exp.append(L.step(arr[i], add_loss=add_loss_at(pattern, i)))
        e = L.last_errors()
        lo.append(e[0])
        hi.append(e[1])
    return np.stack(exp), lo, hi, L


def add_loss_at(pattern, i):
    if i == 0 or pattern == "lossy":
        return False
    return True if pattern == "loss" else (i // 7) % 2 == 1
