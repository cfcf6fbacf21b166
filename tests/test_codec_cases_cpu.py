"""CPU: the designed records of the codec record tests (codec_cases.py) are what the oracle makes of their frames - mode, widths and base
of every record, which is also a check of the oracle against the format text, stated nowhere else so far - and together they reach what
test_gpu_codec_records.py needs them to reach: every (mode, block, width) cell, the narrow tier with mixed widths, the step over the tier
edge and every uniform width in all three modes, every pattern at every frame position of a chunk, the tie of the key-mode rule.  The
same census over the frames of the older codec tests finds no LEFT record at all: that is why the new cases exist."""
import numpy as np
import pytest

import codec_cases as C

SEED = 11
KEYS = ("raw", "left")
KEY_MODE = {"raw": C.MODE_RAW, "left": C.MODE_LEFT}


def test_patterns_are_the_four_families():
    assert C.NPATTERNS == 47 and len({tuple(p) for p in C.PATTERNS}) == 47
    assert all(len(p) == 8 and 0 <= min(p) and max(p) <= 16 for p in C.PATTERNS)
    assert {(j, p[j]) for p in C.PATTERNS[:17] for j in range(8)} == {(j, w) for j in range(8) for w in range(17)}
    assert all(len(set(p)) > 1 for p in C.PATTERNS[:30])  # mixed
    assert {(j, p[j]) for p in C.PATTERNS[17:22] for j in range(8)} == {(j, w) for j in range(8) for w in range(5)}
    assert [C.tier_class(p) for p in C.PATTERNS[17:22]] == ["narrow_mixed"] * 5
    assert [C.tier_class(p) for p in C.PATTERNS[22:30]] == ["tier_edge"] * 8 and [p.index(5) for p in C.PATTERNS[22:30]] == list(range(8))
    assert [C.tier_class(p) for p in C.PATTERNS[30:]] == [("uniform", w) for w in range(17)]
    assert C.SCENE_H * C.SCENE_W == 47 * C.TILE_PX


def test_residuals_and_offsets_are_as_designed():
    rng = np.random.default_rng(1)
    bases = set()
    for p in C.PATTERNS + [C.LEFT_WIDEST]:
        for signed in (False, True):
            for _ in range(6):
                r = C.residuals(rng, p).reshape(64, 8)
                assert r.min() == 0 and [int(np.bitwise_or.reduce(r[:, j])).bit_length() for j in range(8)] == list(p)
                c = C.offset(rng, p, signed)
                lo, hi = (-32768, 32767) if signed else (0, 65535)
                assert lo <= c and c + r.max() <= c + (1 << max(p)) - 1 <= hi
                bases.add(c % 65536)
    assert {0, 0x8000} <= bases and all(any((b >> (4 * q)) & 15 == 15 for b in bases) for q in range(4))


def test_header_fields_reads_the_format_text():
    """a header put together bit by bit, as the text lists the fields"""
    widths, base, mode = [1, 16, 3, 4, 5, 6, 0, 9], 0xA5C3, 2
    h = 0
    for q in range(4):
        h |= (widths[q] | widths[4 + q] << 5 | ((base >> (4 * q)) & 15) << 10 | (mode << 14 if q == 0 else 0)) << (16 * q)
    m, w, b = C.header_fields(np.array([h], np.uint64))
    assert (int(m[0]), list(w[0]), int(b[0])) == (mode, widths, base)
    with pytest.raises(AssertionError):
        C.header_fields(np.array([1 << 30], np.uint64))


@pytest.mark.parametrize("key", KEYS)
def test_oracle_makes_the_designed_records(oracle, key):
    """every record of the record scene (one chunk of 48 frames) and of the key scene (GOP 1): the oracle's header is the designed mode,
    widths and base, and the oracle's decoder gives the frames back"""
    fr = C.record_scene(SEED, key)
    assert fr.shape == (48, 94, 256) and fr.dtype == np.uint16
    hdr, off, st = oracle.codec_encode_chunk(fr)
    mode, widths, base = C.header_fields(hdr)
    d_mode, d_widths, d_base = C.design("record", SEED, key)
    assert np.array_equal(mode, d_mode) and (mode[:, 0] == KEY_MODE[key]).all() and (mode[:, 1:] == C.MODE_TEMPORAL).all()
    assert np.array_equal(widths, d_widths) and np.array_equal(base, d_base)
    assert np.array_equal(np.diff(off.astype(np.int64)), d_widths.sum(axis=(1, 2))) and st.size == d_widths.sum()
    assert np.array_equal(oracle.codec_decode_chunk(hdr, off, st, 256, 94), fr)
    for t in range(47):  # the only record off its pattern: LEFT with eight widths of 16
        for f in range(48):
            want = C.LEFT_WIDEST if (key, f, min(C.PATTERNS[t])) == ("left", 0, 16) else C.PATTERNS[(t + f) % 47]
            assert list(widths[t, f]) == want, (t, f)
    kf = C.key_scene(SEED + 1, key)
    d_mode, d_widths, d_base = C.design("key", SEED + 1, key)
    for i in range(kf.shape[0]):
        hdr, off, st = oracle.codec_encode_chunk(kf[i:i + 1])
        mode, widths, base = C.header_fields(hdr[:, 0])
        assert np.array_equal(mode, d_mode[i]) and np.array_equal(widths, d_widths[i]) and np.array_equal(base, d_base[i]), i
        assert np.array_equal(oracle.codec_decode_chunk(hdr, off, st, 256, 94), kf[i:i + 1])


def test_census_reaches_every_cell_and_class(oracle):
    cells, classes = set(), set()
    for key in KEYS:
        for frames, gop in ((C.record_scene(SEED, key), 48), (C.key_scene(SEED + 1, key), 1)):
            for a, b in C.census(frames, gop, oracle):
                cells |= a
                classes |= b
    assert len(C.ALL_CELLS) == 3 * 8 * 17 == 408 and cells == C.ALL_CELLS
    for mode in (C.MODE_TEMPORAL, C.MODE_RAW, C.MODE_LEFT):
        assert (mode, "narrow_mixed") in classes and (mode, "tier_edge") in classes and (mode, "wide_mixed") in classes, mode
        for w in range(17):
            assert ((mode, ("uniform", w)) in classes) == ((mode, w) != (C.MODE_LEFT, 16)), (mode, w)
    # the key scene alone (GOP 1: what a stream of key frames meets) has every key-mode cell and class too
    for key in KEYS:
        got = [C.census(C.key_scene(SEED + 1, key), 1, oracle)]
        k_cells = set().union(*(a for chunk in got for a, _ in chunk))
        assert k_cells == {c for c in C.ALL_CELLS if c[0] == KEY_MODE[key]}


@pytest.mark.parametrize("key", KEYS)
def test_every_pattern_stands_at_every_frame_position(oracle, key):
    _, widths, _ = C.header_fields(oracle.codec_encode_chunk(C.record_scene(SEED, key))[0])
    every = {tuple(p) for p in C.PATTERNS}
    for f in range(1, 48):
        assert {tuple(int(x) for x in widths[t, f]) for t in range(47)} == every, f


def test_the_two_hand_tiles(oracle):
    """equal totals: RAW; LEFT smaller by one word: LEFT - by hand, by a plain numpy count and by the oracle"""
    assert C.TIE_WORDS == {"tie": (12, 12), "left_by_one": (31, 30)}
    assert C.mode_totals(C.TIE_TILE) == (12, 12) and C.mode_totals(C.LEFT_BY_ONE_TILE) == (31, 30)
    for tile, mode, words in ((C.TIE_TILE, C.MODE_RAW, 12), (C.LEFT_BY_ONE_TILE, C.MODE_LEFT, 30)):
        hdr, off, st = oracle.codec_encode_chunk(tile.astype(np.uint16).reshape(1, 1, 512))
        m, w, _ = C.header_fields(hdr)
        assert int(m[0, 0]) == mode and st.size == words == int(w.sum()) == off[1]
    fr = C.tie_frames()
    assert fr.shape == (3, 2, 1024)
    for i, want in ((0, [0, 2, 2, 0]), (1, [2, 0, 0, 2])):  # each beside a tile of the other kind, in both orders
        hdr, off, st = oracle.codec_encode_chunk(fr[i:i + 1])
        m, w, _ = C.header_fields(hdr[:, 0])
        assert list(m) == want and list(w.sum(axis=1)) == [12 if x == 0 else 30 for x in want]
    hdr, off, st = oracle.codec_encode_chunk(fr)
    assert np.array_equal(oracle.codec_decode_chunk(hdr, off, st, 1024, 2), fr)


def test_ragged_scenes(oracle):
    scenes = {name: (fr, off) for name, fr, off in C.ragged_scene(SEED)}
    assert set(scenes) == {"left_cut", "ramp", "raw_off1", "raw_off3", "left_off1", "left_off3"}
    cut, _ = scenes["left_cut"]
    assert cut.shape == (48, 3, 7937) and 3 * 7937 == 46 * 512 + 259 and (3 * 7937) % 8
    assert np.array_equal(cut.reshape(48, -1), C.record_scene(SEED, "left").reshape(48, -1)[:, :3 * 7937])
    m, w, _ = C.header_fields(oracle.codec_encode_chunk(cut)[0])
    d_mode, d_widths, _ = C.design("record", SEED, "left")
    assert np.array_equal(m[:46], d_mode[:46]) and np.array_equal(w[:46], d_widths[:46])  # the whole tiles keep their design
    ramp, _ = scenes["ramp"]
    assert ramp.shape == (3, 3, 2817) and 3 * 2817 == 16 * 512 + 259
    hdr, off, st = oracle.codec_encode_chunk(ramp)
    m, w, _ = C.header_fields(hdr)
    assert m.shape == (17, 3) and (m[:, 0] == C.MODE_LEFT).all() and list(w[-1, 0]) == [15, 7, 7, 14, 7, 7, 7, 7]
    assert np.array_equal(oracle.codec_decode_chunk(hdr, off, st, 2817, 3), ramp)
    for name, off_el in (("raw_off1", 1), ("raw_off3", 3), ("left_off1", 1), ("left_off3", 3)):
        assert scenes[name][1] == off_el and (2 * off_el) % 16 and scenes[name][0] is C.record_scene(SEED, name[:name.index("_")])


def test_the_older_codec_tests_never_make_a_left_record(oracle):
    """negative control: the frames of test_gpu_codec.CASES and the scenes of test_gpu_packed_mirrored hold no LEFT record.  If a scene
    with LEFT keys is added there one day, this test says so (and the case for this file's scenes changes, not disappears)."""
    import test_gpu_codec as T
    import test_gpu_packed_mirrored as M

    cells = set()
    for name, shape, gop in T.CASES:
        for a, _ in C.census(T._case_frames(name, shape), gop, oracle):
            cells |= a
    for name in M.SCENES:
        for a, _ in C.census(M._scene(name, 107, 32, 64, 50), 50, oracle):
            cells |= a
    assert cells and not {c for c in cells if c[0] == C.MODE_LEFT}
