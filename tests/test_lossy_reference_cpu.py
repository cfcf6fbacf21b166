"""CPU: a second opinion on the oracle's bounded-loss step.  tests/lossy_reference.py restates the reference (h264.cpp:2253-2607,
:1526-1615, :1955-2036) in numpy, from its text and in another structure than oracle/rir_oracle.c; the two must agree bit for bit,
frames and budgets, on the scenes of tests/lossy_cases.py - the scenes the GPU tests of test_gpu_lossy_full_range.py compare the
kernels with the oracle on.  The scenes' own conditions (what makes them worth running) are asserted from the numpy restatement alone,
and five deliberately wrong variants of it show that a kernel with one of these errors would not pass those GPU tests."""
import numpy as np
import pytest

from librir_amd.synthetic import s1_noisy_background
from lossy_cases import MODE_TIE_LOW, mode_tie, surely_both_classes, ti_edges
from lossy_reference import OutOfDomain, ReferenceLossy, track
from oracle.pyoracle import OracleLossy

N = 100
SHAPES = [(9, 13, 6), (35, 83, 32), (64, 96, 61)]
RINGS = [0, 1, 3, 32, 64]
PATTERNS = ["lossy", "loss", "interleaved"]
BUDGETS = {"ti_edges": (6, 2), "mode_tie": (6, 0)}
# budgets raised right after the rise of ti_edges: the statistic of the frame of the rise (differences of 47 000, whose squares wrap) is
# in the mean of the next 40 frames, and with budgets this wide what it adds to the mean decides the foreground budget of each of them
RAISED = {N // 2 + 1: (400, 380, 5.0)}


def scene_of(scene, shape, seed=5):
    h, w, hl = shape
    return ti_edges(N, h, w, hl, seed) if scene == "ti_edges" else mode_tie(N, h, w, seed, hl=hl)


def both(oracle, arr, shape, low, high, sf, ra, mn, pattern, changes=None, cls=ReferenceLossy):
    """-> the numpy restatement's (frames, lows, highs, object) and the oracle's"""
    h, w, hl = shape
    a = track(lambda: cls(w, h, hl, low, high, sf, ra, mn), arr, pattern, changes)
    b = track(lambda: OracleLossy(oracle, w, h, hl, low, high, sf, ra, mn), arr, pattern, changes)
    return a, b


def same(a, b):
    return np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2]


@pytest.mark.parametrize("subtract_min", [False, True], ids=["", "min"])
@pytest.mark.parametrize("sf", [0.0, 5.0])
@pytest.mark.parametrize("ra", RINGS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % (s[0], s[1]))
@pytest.mark.parametrize("scene", ["ti_edges", "mode_tie"])
def test_numpy_restatement_equals_the_oracle(oracle, scene, shape, ra, sf, subtract_min):
    arr = scene_of(scene, shape)
    low, high = BUDGETS[scene]
    for pattern in PATTERNS:
        a, b = both(oracle, arr, shape, low, high, sf, ra, subtract_min, pattern)
        assert same(a, b), pattern
        R = a[3]
        # the scene's conditions, from the restatement alone
        assert all(R.surely_both_classes) and len(R.surely_both_classes) == N - 1, pattern
        assert R.both_sides_full_ring >= 1, pattern
        if sf == 0.0:
            assert set(zip(a[1], a[2])) == {(low, high)}, pattern
        elif scene == "ti_edges":  # (mode_tie is about the background, and moves little: its budgets need not follow)
            assert len(set(zip(a[1], a[2])) - {(low, high)}) >= 1, pattern
        if scene == "mode_tie":
            assert set(R.backgrounds) == {MODE_TIE_LOW + 1}, pattern
        if ra == 64:
            assert R.max_ring_sum > 1 << 21, pattern
        if scene == "ti_edges" and pattern != "loss":
            assert R.by_top_bits >= 1, pattern
        if pattern == "loss":
            assert R.by_top_bits == 0  # (add_loss does not ask: h264.cpp:2579)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % (s[0], s[1]))
def test_parameter_change_in_mid_stream(oracle, shape):
    arr = scene_of("ti_edges", shape)
    for ra, mn, pattern in [(3, False, "lossy"), (32, True, "interleaved"), (32, False, "lossy")]:
        a, b = both(oracle, arr, shape, 6, 2, 5.0, ra, mn, pattern, RAISED)
        assert same(a, b), (ra, mn, pattern)
        assert max(a[1]) > 6  # (the change arrived)


# (h, w, hl, seed) of every other ti_edges scene the GPU tests name (test_gpu_lossy_full_range.py; hook_cases.py takes the shapes of
# test_gpu_lossy.CONST_CASES with seeds 47 and 53): many streams, the constant-budget form, odd sizes, the saver, pixels per thread
GPU_SCENES = ([(96, 128, 93, 20 + i) for i in range(5)] + [(64, 96, 61, 7), (40, 64, 38, 7), (35, 83, 32, 9), (9, 13, 6, 9), (35, 83, 32, 11), (64, 80, 61, 11)]
              + [(64, 96, 61, 47), (40, 64, 40, 47), (40, 64, 38, 47), (40, 64, 37, 47), (64, 96, 64, 53), (64, 96, 62, 53), (64, 96, 61, 53)])


@pytest.mark.parametrize("h,w,hl,seed", GPU_SCENES)
def test_conditions_of_the_scenes_the_gpu_tests_name(h, w, hl, seed):
    """from the restatement alone, with the reference's default parameters: inside its domain (it refuses a frame that is not), both
    classes surely there in every frame, decisions taken by the top bits alone, both sides of the decision with a full ring, budgets
    that move"""
    arr = ti_edges(N, h, w, hl, seed)
    _, lo, hi, R = track(lambda: ReferenceLossy(w, h, hl), arr)
    assert all(R.surely_both_classes) and R.by_top_bits >= 1 and R.both_sides_full_ring >= 1 and len(set(zip(lo, hi))) > 1
    assert all(surely_both_classes(f[:hl]) for f in arr[1:])  # (the scene's own check says the same)


def test_mode_tie_is_a_tie_and_the_lower_bin_is_the_background(oracle):
    for h, w in [(16, 64), (9, 13), (35, 83)]:
        arr = mode_tie(N, h, w, 5)
        for i in range(N):
            hist = np.bincount(arr[i].ravel() >> 2, minlength=16384)
            top = np.flatnonzero(hist == hist.max())
            assert top.tolist() == [MODE_TIE_LOW >> 2, 7500 + (i % 2)] and hist.max() == h * w // 4 and np.sort(hist)[-3] == 1, (h, w, i)
        R, L = ReferenceLossy(w, h, h, 6, 0, 0.0, 0), OracleLossy(oracle, w, h, h, 6, 0, 0.0, 0)
        for i in range(3):
            R.step(arr[i]), L.step(arr[i])
        assert R.last_errors() == L.last_errors() == (6, 0, MODE_TIE_LOW + 1)


def test_s1_stream_of_the_budget_test_through_both(oracle):
    """the stream of test_lossy_oracle.py::test_error_budget_shrinks_with_std_factor_and_splits_after_40_frames"""
    h, w = 32, 64
    arr = s1_noisy_background(60, h, w, seed=5)
    a, b = both(oracle, arr, (h, w, h), 6, 2, 5.0, 32, False, "lossy")
    assert same(a, b)
    assert len(set(zip(a[1], a[2]))) > 1


def test_restatement_refuses_what_makes_the_statistic_nan():
    h, w = 8, 16
    arr = ti_edges(50, h, w, 6, 3).copy()
    R = ReferenceLossy(w, h, 6, 6, 2, 5.0, 4)
    for i in range(45):
        R.step(arr[i])
    arr[45] = 1000  # a uniform frame once the statistic is split by class: no foreground
    with pytest.raises(OutOfDomain):
        R.step(arr[45])


# ---- the scenes discriminate ------------------------------------------------------------------------------------------------------
class NoIntegrationTimeCondition(ReferenceLossy):
    def same_integration_time(self, raw, t):
        return np.ones(raw.shape, bool)


class TopBitsOfTheReferencePixel(ReferenceLossy):
    def same_integration_time(self, raw, t):
        return ((self.ref + self.min) >> 13) == (raw >> 13)


class LastImageNotRefreshedByAddLoss(ReferenceLossy):
    def refresh_last_dl(self, frame, add_loss):
        if not add_loss:
            self.last_dl = frame.copy()


class SquaresNotWrapped(ReferenceLossy):
    def square(self, diff):
        return diff * diff


class TieToTheHighestBin(ReferenceLossy):
    def mode_bin(self, hist):
        return len(hist) - 1 - int(np.argmax(hist[::-1]))


# variant -> the case it must fail: scene, shape, (low, high, stdFactor, ring), entry points, parameter changes.  Each is a case of
# test_gpu_lossy_full_range.py (run paths with the default parameters; the budgets raised after the rise; the mode tie).
WRONG = {
    "top bits never asked": (NoIntegrationTimeCondition, "ti_edges", (64, 96, 61), (6, 2, 5.0, 32), "lossy", None),
    "top bits of ref + min instead of the last image": (TopBitsOfTheReferencePixel, "ti_edges", (64, 96, 61), (6, 2, 5.0, 32), "interleaved", None),
    "add_loss leaves the last image stale": (LastImageNotRefreshedByAddLoss, "ti_edges", (64, 96, 61), (6, 2, 5.0, 32), "interleaved", None),
    "squares not wrapped": (SquaresNotWrapped, "ti_edges", (64, 96, 61), (6, 2, 5.0, 32), "lossy", RAISED),
    "mode tie to the highest bin": (TieToTheHighestBin, "mode_tie", (16, 64, 16), (6, 0, 0.0, 0), "lossy", None),
}


@pytest.mark.parametrize("name", list(WRONG))
def test_a_wrong_step_does_not_pass(oracle, name):
    cls, scene, shape, (low, high, sf, ra), pattern, changes = WRONG[name]
    arr = scene_of(scene, shape)
    good, o = both(oracle, arr, shape, low, high, sf, ra, False, pattern, changes)
    assert same(good, o)
    wrong, _ = both(oracle, arr, shape, low, high, sf, ra, False, pattern, changes, cls=cls)
    assert not same(wrong, o)
