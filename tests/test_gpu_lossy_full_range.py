"""GPU: every form of the bounded-loss step on frames that use the whole 16-bit range (tests/lossy_cases.py) - pixels whose difference
is within their budget while their top three bits changed (h264.cpp:2402: the integration-time condition alone decides, and add_loss
does not ask while it still refreshes the last image, :2579 / :2593), values of 32 768 and more in every packed 16-bit half, differences
whose 32-bit square wraps, ring sums at their ceiling, and two histogram bins tied for the mode (:1979).  Everything is compared with
the oracle bit for bit: frames by array_equal, budgets as lists; there is no tolerance anywhere.  tests/test_lossy_reference_cpu.py
holds the oracle to a second restatement on these very scenes, and shows that a step with one of five plausible errors fails them."""
import numpy as np
import pytest

from librir_amd.video_io import IRMovie, IRSaver
from lossy_cases import MODE_TIE_LOW, mode_tie, ti_edges
from lossy_reference import add_loss_at, track
from oracle.pyoracle import OracleLossy
from test_gpu_lossy import run_path  # noqa: F401  (the fixture: every path a run of frames can take)

pytestmark = pytest.mark.gpu

N = 100
PATTERNS = ["lossy", "loss", "interleaved"]  # add_image_lossy, add_loss, the two switching every 7 frames
# budgets raised right after the rise of ti_edges: the statistic of the frame of the rise (differences of 47 000, whose squares wrap) is
# in the mean of the next 40 frames, and with budgets this wide what it adds to the mean decides the foreground budget of each of them
RAISED = {N // 2 + 1: (400, 380, 5.0)}
PARAMS = {
    "5_2_2.5_ring8": (dict(low=5, high=2, sf=2.5, ra=8), None),
    "defaults": (dict(low=6, high=2, sf=5.0, ra=32), None),
    "defaults_raised_after_the_rise": (dict(low=6, high=2, sf=5.0, ra=32), RAISED),
}
_ENV = ("RIR_LOSSY_LAUNCH_PER_FRAME", "RIR_LOSSY_RUN_MAX_WORKGROUPS", "RIR_LOSSY_NO_SPEC", "RIR_LOSSY_NO_CONST", "RIR_LOSSY_SPEC_PASSES", "RIR_LOSSY_RUN_FORM",
        "RIR_LOSSY_SPEC_FIRST_ONLY", "RIR_LOSSY_SPEC_NO_GIVE_UP", "RIR_LOSSY_SPEC_NO_PLANE")

_expected = {}


def expected(oracle, arr, key, shape, p, subtract_min=False, pattern="lossy", changes=None):
    """the oracle's (frames, lows, highs) for a scene (named by `key`), computed once and shared"""
    k = (key, shape, tuple(sorted(p.items())), subtract_min, pattern, None if changes is None else tuple(sorted(changes.items())))
    if k not in _expected:
        h, w, hl = shape
        e = track(lambda: OracleLossy(oracle, w, h, hl, p["low"], p["high"], p["sf"], p["ra"], subtract_min), arr, pattern, changes)[:3]
        e[0].setflags(write=False)
        _expected[k] = e
    return _expected[k]


def on_device(arr):
    import torch

    return torch.from_numpy(np.array(arr)).cuda()  # (a copy: the scenes are shared and write-protected)


def calls_of(cuts, pattern, changes=None, n=N):
    """the calls that step frames [0, n): cut at `cuts`, wherever the entry point switches and wherever a parameter changes"""
    b = set(cuts) | {0, n} | set(changes or ())
    if pattern != "lossy":
        b.add(1)  # (the first image goes through add_image_lossy)
    if pattern == "interleaved":
        b |= set(range(7, n, 7))
    b = sorted(b)
    return list(zip(b[:-1], b[1:]))


def step_calls(ls, t, cuts, pattern="lossy", changes=None, errors=True, after_call=None):
    """-> frames [n, h, w], lows, highs of the stream stepped call by call"""
    import torch

    got, lo, hi = [], [], []
    for c0, c1 in calls_of(cuts, pattern, changes, t.shape[0]):
        if changes and c0 in changes:
            ls.set_errors(*changes[c0])
        o, l_, h_ = ls.step(t[c0:c1], add_loss=add_loss_at(pattern, c0), errors=errors)
        got.append(o)
        if errors:
            lo.append(l_), hi.append(h_)
        if after_call:
            after_call(c0, c1)
    if not errors:
        ls.status()  # (queue-only calls leave the device-side verdict to this query)
        return torch.cat(got).cpu().numpy(), None, None
    return torch.cat(got).cpu().numpy(), np.concatenate(lo).tolist(), np.concatenate(hi).tolist()


def first_difference(got, exp):
    bad = [i for i in range(len(exp)) if not np.array_equal(got[i], exp[i])]
    if not bad:
        return None
    y, x = np.argwhere(got[bad[0]] != exp[bad[0]])[0]
    return dict(frames=bad[:8], frame=bad[0], y=int(y), x=int(x), got=int(got[bad[0], y, x]), expected=int(exp[bad[0], y, x]))


def check(got, exp, what):
    assert first_difference(got[0], exp[0]) is None, (what, first_difference(got[0], exp[0]))
    if got[1] is not None:
        assert got[1] == exp[1] and got[2] == exp[2], what


@pytest.fixture
def plain_paths(monkeypatch):
    for k in _ENV:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


# ---- the general form: the resident run kernel in its two forms, batches of streams, one launch per frame ---------------------------
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("name", list(PARAMS))
def test_run_paths_on_ti_edges(oracle, name, pattern, run_path, monkeypatch):
    """One stream through every run path, in two calls, queue-only, and cut into runs, single frames and pairs.  The speculative form is
    switched off: every frame is stepped by the general form the path names (the speculative form has its own test below)."""
    from librir_amd import device as D

    monkeypatch.setenv("RIR_LOSSY_NO_SPEC", "1")
    shape = h, w, hl = 64, 96, 61
    p, changes = PARAMS[name]
    arr = ti_edges(N, h, w, hl, 5)
    exp = expected(oracle, arr, "ti_edges5", shape, p, False, pattern, changes)
    t = on_device(arr)
    for what, cuts, errors in (("two calls", [0, 1, 40, N], True), ("queue only", [0, 1, N], False), ("cuts", [0, 1, 5, 6, 7, 30, 32, 33, N], True)):
        ls = D.LossyStream(w, h, hl, p["low"], p["high"], p["sf"], p["ra"])
        got = step_calls(ls, t, cuts, pattern, changes, errors)
        books = ls.path_stats(), ls.spec_stats()
        ls.close()
        check(got, exp, (run_path, what))
        assert books == ((0, 0), (0, 0, 0, 0)), books  # (neither streaming form was in it)


def test_many_streams_on_ti_edges(oracle, run_path, monkeypatch):
    """Five streams with their own scenes and parameters in shared launches, two calls; streams 1 and 3 subtract their minimum."""
    from librir_amd import device as D

    monkeypatch.setenv("RIR_LOSSY_NO_SPEC", "1")
    S, shape = 5, (96, 128, 93)
    h, w, hl = shape
    params = [dict(low=6, high=2, sf=5.0, ra=32), dict(low=3, high=3, sf=0.0, ra=4), dict(low=5, high=1, sf=2.5, ra=0),
              dict(low=9, high=4, sf=5.0, ra=7), dict(low=6, high=2, sf=5.0, ra=32)]
    data = [ti_edges(N, h, w, hl, 20 + i) for i in range(S)]
    mins = [i in (1, 3) for i in range(S)]
    streams = [D.LossyStream(w, h, hl, p["low"], p["high"], p["sf"], p["ra"], subtract_min=m) for p, m in zip(params, mins)]
    tens = [on_device(d) for d in data]
    cut = 13
    o1, lo1, hi1 = D.LossyStream.step_many(streams, [t[:cut] for t in tens])
    o2, lo2, hi2 = D.LossyStream.step_many(streams, [t[cut:] for t in tens])
    books = streams[0].path_stats(), streams[0].spec_stats()
    for i, p in enumerate(params):
        exp = expected(oracle, data[i], "ti_edges%d" % (20 + i), shape, p, mins[i])
        got = np.concatenate([o1[i].cpu().numpy(), o2[i].cpu().numpy()]), np.concatenate([lo1[i], lo2[i]]).tolist(), np.concatenate([hi1[i], hi2[i]]).tolist()
        check(got, exp, (run_path, i))
    for s in streams:
        s.close()
    assert books == ((0, 0), (0, 0, 0, 0)), books  # (stdFactor differs from 0 in four of them: the general form)


# ---- the constant-budget form -------------------------------------------------------------------------------------------------------
CONST_CUTS = {0: [0, 1, N], 1: [0, 1, 30, 31, N], 2: [0, 1, 3, N], 8: [0, 1, 50, N], 64: [0, 1, 20, 45, N]}  # (as in test_gpu_lossy.CONST_CASES)


@pytest.mark.parametrize("pattern", ["lossy", "loss"])
@pytest.mark.parametrize("subtract_min", [False, True], ids=["", "min"])
@pytest.mark.parametrize("ra", list(CONST_CUTS))
@pytest.mark.parametrize("shape", [(64, 96, 61), (40, 64, 38)], ids=["96x64", "64x40"])
def test_constant_budget_form_on_ti_edges(oracle, shape, ra, subtract_min, pattern, plain_paths):
    """stdFactor 0: every group of frames is taken by the streaming kernel (both classes are surely there in every frame of the scene),
    rings of every length, the ring of 64 with sums up to 64 x 65 535."""
    from librir_amd import device as D

    h, w, hl = shape
    p = dict(low=6, high=2, sf=0.0, ra=ra)
    arr = ti_edges(N, h, w, hl, 7)
    exp = expected(oracle, arr, "ti_edges7", shape, p, subtract_min, pattern)
    ls = D.LossyStream(w, h, hl, 6, 2, 0.0, ra, subtract_min=subtract_min)

    def taken(c0, c1):
        steps = (c1 - c0) - (1 if c0 == 0 else 0)
        if c1 - c0 >= 3 and steps >= 2:
            offered, took = ls.path_stats()
            assert offered >= 1 and took == offered, (c0, c1, offered, took)

    got = step_calls(ls, on_device(arr), CONST_CUTS[ra], pattern, after_call=taken)
    ls.close()
    check(got, exp, (shape, ra))


# ---- the speculative form -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["lossy", "loss"])
@pytest.mark.parametrize("name", ["defaults", "defaults_raised_after_the_rise"])
def test_speculative_form_on_ti_edges(oracle, name, pattern, plain_paths):
    """stdFactor 5 through the default route: groups are offered to the speculative form, which commits them or leaves them to the general
    form.  The rise of 47 000 levels does not fit the byte plane's 7 bits, and its squares wrap in the sums kernel's exact path: with the
    plane and without it, the oracle's frames and budgets and the same books (printed, not prescribed)."""
    from librir_amd import device as D

    plain_paths.setenv("RIR_LOSSY_SPEC_PASSES", "8")
    shape = h, w, hl = 64, 96, 61
    p, changes = PARAMS[name]
    arr = ti_edges(N, h, w, hl, 5)
    exp = expected(oracle, arr, "ti_edges5", shape, p, False, pattern, changes)
    t = on_device(arr)
    books = {}
    for plane in (True, False):
        if not plane:
            plain_paths.setenv("RIR_LOSSY_SPEC_NO_PLANE", "1")
        ls = D.LossyStream(w, h, hl, p["low"], p["high"], p["sf"], p["ra"])
        bk = []
        got = step_calls(ls, t, [0, 30, N], pattern, changes, after_call=lambda c0, c1: bk.append(((c0, c1), ls.spec_stats(), ls.path_stats())))
        ls.close()
        check(got, exp, (name, plane))
        books[plane] = bk
    print("spec_stats / path_stats per call:", books[True])
    assert books[True] == books[False], books
    assert any(b[1][0] >= 1 for b in books[True]), books  # (some group went through the speculative form's launches)


# ---- frames that are no multiple of 8 pixels: one pixel per thread, one launch per frame --------------------------------------------
@pytest.mark.parametrize("sf", [0.0, 5.0])
@pytest.mark.parametrize("subtract_min", [False, True], ids=["", "min"])
@pytest.mark.parametrize("ra", [0, 1, 3, 64])
@pytest.mark.parametrize("shape", [(35, 83, 32), (9, 13, 6)], ids=["83x35", "13x9"])
def test_odd_sizes_on_ti_edges(oracle, shape, ra, subtract_min, sf, plain_paths):
    from librir_amd import device as D

    h, w, hl = shape
    assert (w * hl) % 8 != 0 or (w * h) % 8 != 0
    p = dict(low=6, high=2, sf=sf, ra=ra)
    arr = ti_edges(N, h, w, hl, 9)
    t = on_device(arr)
    for pattern, cuts in (("lossy", [0, 1, 40, N]), ("interleaved", [0, N])):
        exp = expected(oracle, arr, "ti_edges9", shape, p, subtract_min, pattern)
        ls = D.LossyStream(w, h, hl, 6, 2, sf, ra, subtract_min=subtract_min)
        got = step_calls(ls, t, cuts, pattern)
        books = ls.path_stats(), ls.spec_stats()
        ls.close()
        check(got, exp, (shape, ra, pattern))
        assert books == ((0, 0), (0, 0, 0, 0)), books  # (no run of frames: each frame in launches of its own)


# ---- the saver ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,subtract_min", [((35, 83, 32), False), ((64, 80, 61), True)], ids=["83x35_defaults", "80x64_min"])
def test_saver_on_ti_edges(tmp_path, oracle, shape, subtract_min):
    """add_image_lossy, add_loss from frame 40 to 59 (images that do not reach the file but move the state, the last image included),
    add_image_lossy again: the file, read back, is the oracle's frames with MIN_T back on the lossy rows."""
    h, w, hl = shape
    arr = ti_edges(N, h, w, hl, 11)
    L = OracleLossy(oracle, w, h, hl, subtract_min=subtract_min)
    in_loss = lambda i: 40 <= i < 60  # noqa: E731
    exp, elo, ehi = [], [], []
    for i in range(N):
        exp.append(L.step(arr[i], add_loss=in_loss(i)))
        lo, hi, _ = L.last_errors()
        elo.append(lo), ehi.append(hi)
    dst = tmp_path / "full_range.h264"
    with IRSaver(dst, w, h, hl) as s:
        if subtract_min:
            s.set_parameter("subtractMin", 1)
        for i in range(N):
            if in_loss(i):
                assert np.array_equal(s.add_loss(arr[i]), exp[i]), i
            else:
                s.add_image_lossy(arr[i], i * 1000)
        assert list(s.get_low_errors()) == elo and list(s.get_high_errors()) == ehi
    recorded = [i for i in range(N) if not in_loss(i)]
    want = np.stack([exp[i] for i in recorded])
    if subtract_min:  # the loader adds MIN_T back on the first MIN_T_HEIGHT rows (IRFileLoader.cpp:1173-1179)
        want[:, :hl] += np.uint16(int(arr[0, :hl].min()))
    with IRMovie.from_filename(dst) as mov:
        assert mov.images == len(recorded)
        assert first_difference(mov.data, want) is None, first_difference(mov.data, want)


# ---- two bins tied for the mode ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["constant budgets", "general run", "launch per frame"])
@pytest.mark.parametrize("ra", [0, 4])
@pytest.mark.parametrize("shape", [(16, 64), (9, 13)], ids=["64x16", "13x9"])
def test_mode_tie_goes_to_the_lower_bin(oracle, shape, ra, form, plain_paths):
    """Budgets 6 / 0: with the lower of the two tied bins as background its pixels at 4 002 and 4 003 are foreground and refreshed whenever
    they move; a reduction that kept the higher bin would keep them.  (13x9 is no multiple of 8 pixels: a launch per frame whatever is asked.)"""
    from librir_amd import device as D

    h, w = shape
    if form == "general run":
        plain_paths.setenv("RIR_LOSSY_NO_CONST", "1")
        plain_paths.setenv("RIR_LOSSY_NO_SPEC", "1")
    elif form == "launch per frame":
        plain_paths.setenv("RIR_LOSSY_LAUNCH_PER_FRAME", "1")
    p = dict(low=6, high=0, sf=0.0, ra=ra)
    arr = mode_tie(N, h, w, 5)
    L = OracleLossy(oracle, w, h, h, 6, 0, 0.0, ra)
    L.step(arr[0]), L.step(arr[1])
    assert L.last_errors() == (6, 0, 4 * (MODE_TIE_LOW >> 2) + 1)
    exp = expected(oracle, arr, "mode_tie5", (h, w, h), p)
    ls = D.LossyStream(w, h, h, 6, 0, 0.0, ra)
    got = step_calls(ls, on_device(arr), [0, 1, 40, N])
    offered, took = ls.path_stats()
    ls.close()
    check(got, exp, (shape, ra, form))
    if form == "constant budgets" and (h * w) % 8 == 0:
        assert offered >= 1 and took == offered, (offered, took)
    else:
        assert (offered, took) == (0, 0)
