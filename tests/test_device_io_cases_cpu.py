"""CPU: the case tables of the device I/O tests (device_io_cases.py) reach what test_gpu_device_io_full_range.py needs them to reach - a
MIN_T boundary inside a lane of a whole tile and of a cut one, reads of three batches with skipped chunks and single-frame jobs, MIN_T
that wraps - and the helper's restatements of the library's arithmetic hold against the numbers worked out by hand and the constants
in the source."""
import os
import re

import numpy as np

import device_io_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_batch_limits_are_the_library_s():
    src = open(os.path.join(ROOT, "librir_amd", "csrc", "video_io_abi.cpp")).read()
    assert int(re.search(r"kDioBatchChunks = (\d+);", src).group(1)) == C.BATCH_CHUNKS
    assert int(re.search(r"kDioBatchBytes = \(size_t\)(\d+) << 20;", src).group(1)) << 20 == C.BATCH_BYTES
    assert int(re.search(r"kDioScratchBytes = \(size_t\)(\d+) << 20;", src).group(1)) << 20 == C.SCRATCH_BYTES
    fmt = open(os.path.join(ROOT, "librir_amd", "csrc", "codec_format.h")).read()
    assert int(re.search(r"#define RIRB1_TILE_PX (\d+)", fmt).group(1)) == C.TILE_PX
    assert int(re.search(r"#define RIRB1_REC_MAX_WORDS (\d+)", fmt).group(1)) == 128  # batch_bytes_bound


def test_min_t_geometries_reach_partial_lanes():
    partial = set(range(1, 8))
    # 32x44: 1 408 pixels = 2 whole tiles + 384; the boundary 4 pixels into lane 5 of tile 0, lane 7 of tile 1, lane 31 of the cut tile
    assert C.lane_classes(32, 44, 1) == ({0, 4, 8}, {0}, 2) and 44 - (0 * 512 + 5 * 8) == 4
    assert C.lane_classes(32, 44, 13) == ({0, 4, 8}, {0}, 2) and 13 * 44 == 572 and 572 - (1 * 512 + 7 * 8) == 4
    assert C.lane_classes(32, 44, 29) == ({8}, {0, 4, 8}, 2) and 29 * 44 == 1276 and 1276 - (2 * 512 + 31 * 8) == 4
    assert C.lane_classes(9, 13, 4) == (set(), {0, 4, 8}, 0)  # 117 pixels: no multiple of 8, every tile ragged
    assert C.lane_classes(16, 32, 5) == ({0, 8}, set(), 1)  # one whole tile and nothing else; all-or-nothing lanes
    for g in ((32, 44, 1), (32, 44, 13), (32, 44, 29), (9, 13, 4), (16, 32, 5)):
        assert g in C.MIN_T_GEOMETRIES
    whole, cut = set(), set()
    for h, w, rows in C.MIN_T_GEOMETRIES:
        a, b, _ = C.lane_classes(h, w, rows)
        whole |= a
        cut |= b
    assert whole & partial and cut & partial and {0, 8} <= whole and {0, 8} <= cut
    # the MIN_T_HEIGHT variants the GPU test adds (absent: h - 3 rows; h; h + 8, clamped) end on a lane's edge or inside one - either is fine
    assert C.min_t_rows(32, 0) == 29 and C.min_t_rows(32, 32) == 32 and C.min_t_rows(32, 40) == 32 and C.min_t_rows(9, 4) == 4
    # the long MIN_T recording: a partial lane in a whole tile, in every one of three batches
    d = C.MIN_T_LONG
    assert C.lane_classes(d["h"], d["w"], d["rows"])[0] & partial
    assert [len(C.plan_of(d["n"], d["gop"], s)) for s in d["selections"]] == [3, 2]


def test_read_plan_batches_and_skipped_chunks():
    p = C.read_plan(37, 2, 0, 37, 1)
    assert [len(b) for b in p] == [8, 8, 3] and p[-1][-1] == (18, 0, 1, 36)
    assert p[1][0] == (8, 0, 2, 16)  # the second batch starts at output slot 16
    p = C.read_plan(37, 2, 0, 13, 3)
    jobs = [j for b in p for j in b]
    assert [len(b) for b in p] == [8, 5] and len(jobs) == 13
    assert [j[0] for j in jobs] == [c for c in range(19) if c % 3 != 2]  # chunks 2, 5, 8, ... have no selected frame
    assert [j[1] for j in jobs] == [0, 1] * 6 + [0] and [j[3] for j in jobs] == list(range(13))
    p = C.read_plan(37, 2, 0, 8, 5)
    assert [len(b) for b in p] == [8] and all(j[2] == 1 for j in p[0]) and [j[0] for j in p[0]] == [0, 2, 5, 7, 10, 12, 15, 17]
    p = C.read_plan(36, 3, 2, 12, 3)
    assert [len(b) for b in p] == [8, 4] and all(j[1:3] == (2, 1) for b in p for j in b)  # the last frame of every chunk, alone
    assert C.read_plan(7, 50, 0, 7, 1) == [[(0, 0, 7, 0)]] and C.read_plan(7, 50, 6, 1, 1) == [[(0, 6, 1, 0)]]  # one short chunk
    p = C.read_plan(9, 1, 0, 9, 1)
    assert [len(b) for b in p] == [8, 1] and [j for b in p for j in b] == [(c, 0, 1, c) for c in range(9)]
    # against a brute-force walk of every selection of a few recordings
    for n, gop in ((11, 3), (12, 4), (9, 1), (7, 50), (37, 2)):
        for first in range(n):
            for step in (1, 2, gop, gop + 1, 2 * gop + 1):
                count = (n - 1 - first) // step + 1
                want = {}
                for k in range(count):
                    want.setdefault((first + k * step) // gop, []).append(k)
                jobs = [j for b in C.read_plan(n, gop, first, count, step) for j in b]
                assert [j[0] for j in jobs] == sorted(want)
                for c, lf, cnt, of in jobs:
                    assert (lf, cnt, of) == (first + want[c][0] * step - c * gop, len(want[c]), want[c][0])


def test_selections_reach_their_chunk_edges():
    for gop, n in C.LOSSLESS_RECORDINGS + C.LOSSLESS_EXTRA_RECORDINGS:
        g = gop or C.DEFAULT_GOP
        sels = C.selections(n, g)
        steps = {s.step for s in sels if isinstance(s, slice) and s.step}
        assert {1, g, g + 1, 2 * g + 1} <= steps and (g == 1 or g - 1 in steps)
        ints = {s for s in sels if isinstance(s, int)}
        assert {0, min(g, n) - 1, n - 1} <= ints and (g >= n or g in ints)
        plans = [C.plan_of(n, g, s) for s in sels]
        assert [] in plans  # the empty selections
        last_alone = [j for p in plans for b in p for j in b if j[2] == 1 and j[1] == min(g, n - j[0] * g) - 1]
        assert last_alone  # a job whose only frame is its chunk's last
        assert any(j[0] == (n - 1) // g for j in last_alone)  # ... and the last chunk's
    recs = dict((gop, n) for gop, n in C.LOSSLESS_RECORDINGS + C.LOSSLESS_EXTRA_RECORDINGS)
    assert recs[3] % 3 and recs[4] % 4 == 0 and 1 in recs and recs[None] < C.DEFAULT_GOP  # short last chunk; none; GOP 1; GOP > recording
    assert len(C.plan_of(recs[1], 1, slice(None))) == 2  # GOP 1: nine jobs, two batches


def test_filtered_and_out_cases_leave_the_first_batch():
    d = C.FILTERED
    plans = [C.plan_of(d["n"], d["gop"], s) for s in d["selections"]]
    assert [len(p) for p in plans] == [3, 2, 2, 1]
    assert all(b[0][3] > 0 for p in plans[:3] for b in p[1:])  # k0 > 0 from the second batch on
    r = range(d["n"])[d["selections"][2]]
    assert r.start == 17 and r.start % d["gop"] == 1 and plans[2][1][0][3] not in (0, r.start)  # first != 0, k0 != 0, k0 != first
    assert all(j[2] == 1 for j in plans[3][0])
    assert [j[0] for b in plans[1] for j in b] == [c for c in range(18) if c % 3 != 1]  # skipped chunks, the last too
    gop, n = C.OUT_RECORDING
    skipped_before, skipped_between, skipped_chunk = False, False, False
    for step in C.OUT_STEPS:
        jobs = [j for b in C.read_plan(n, gop, 0, (n - 1) // step + 1, step) for j in b]
        skipped_before |= any(j[1] > 0 for j in jobs)
        skipped_between |= any(j[2] > 1 for j in jobs) and step > 1
        skipped_chunk |= len(jobs) < (n + gop - 1) // gop
    assert skipped_before and skipped_between and skipped_chunk
    for h, w in C.OUT_SHAPES:  # whole tiles to take the FAST form from when `out` is aligned
        assert (h * w) % 8 == 0 and h * w >= C.TILE_PX
    assert (32, 44) in C.OUT_SHAPES and 32 * 44 % C.TILE_PX  # ... and a cut tile behind them


def test_min_t_expected_is_the_definition():
    arr = C.with_ends(C.frames("uniform", 3, 9, 13, 5))
    flat = arr.reshape(3, -1)
    for half in (flat[:, 0::2], flat[:, 1::2]):  # the low and the high half of a packed pair of pixels
        assert (half == 65535).any() and (half < 5).any()
    assert len(np.unique(arr)) > arr.size // 2
    for min_t in C.MIN_T_VALUES:
        for mth in (0, 4, 9, 17):
            rows = 6 if mth == 0 else min(mth, 9)
            want = arr.copy()
            for i in range(3):
                for y in range(rows):
                    want[i, y] = [(int(v) + min_t) & 0xFFFF for v in arr[i, y]]
            got = C.min_t_expected(arr, min_t, mth)
            assert got.dtype == np.uint16 and np.array_equal(got, want)
            wrapped = (arr[:, :rows].astype(np.int64) + min_t < 0) | (arr[:, :rows].astype(np.int64) + min_t > 65535)
            assert wrapped.any() and not np.array_equal(got[:, :rows], arr[:, :rows]) and np.array_equal(got[:, rows:], arr[:, rows:])
    assert set(C.MIN_T_VALUES) == {1, 40000, 65535, -5}


def test_frames_kinds():
    for h, w in C.LOSSLESS_SHAPES:
        u, e, hi = (C.frames(k, 5, h, w, 1) for k in C.KINDS)
        assert all(a.dtype == np.uint16 and a.shape == (5, h, w) for a in (u, e, hi))
        assert set(np.unique(e)) <= {0, 65535} and (h * w == 1 or set(np.unique(e)) == {0, 65535})
        assert (np.abs(np.diff(e.astype(np.int64), axis=0)) == 65535).all()
        flat = hi.reshape(5, -1)
        npx = h * w
        edges = {0, npx - 1} | {p for t in range(0, npx, C.TILE_PX) for p in (t, min(t + C.TILE_PX, npx) - 1)}
        for p in edges:
            assert set(flat[:, p]) <= set(C.SPECIALS)
        rest = np.delete(flat, sorted(edges), axis=1)
        assert rest.size == 0 or (rest.min() >= 32768 and rest.max() < 32808)
        if npx >= 4:
            assert set(flat[:, sorted(edges)].ravel()) == set(C.SPECIALS)
    assert (C.frames("uniform", 11, 32, 44, 1) >= 49152).any() and (C.frames("uniform", 11, 32, 44, 1) < 16384).any()
    s = C.frames("s1_high", 37, 40, 72, 3)
    assert s.min() >= 64000 and s.max() < 65535


def test_small_recordings_stay_far_below_the_byte_and_scratch_limits():
    """why read_plan may ignore kDioBatchBytes and kDioScratchBytes: a whole small recording with its tables is a few hundred kilobytes"""
    recs = C.small_recordings()
    assert (37, 40, 72, 2) in recs and (37, 32, 44, 2) in recs and len(recs) >= 30
    for n, h, w, gop in recs:
        chunks = (n + gop - 1) // gop
        assert n * h * w * 2 + C.batch_bytes_bound(h, w, gop, chunks, 0) < C.BATCH_BYTES // 64
        assert C.batch_bytes_bound(h, w, gop, chunks, n) < C.BATCH_BYTES // 64
        assert 2 * n * h * w * 2 < C.SCRATCH_BYTES // 64  # float32 + motion: two scratch frames per image


def test_large_cases_cut_where_they_should():
    d = C.LARGE
    h, w, n, gop = d["h"], d["w"], d["n"], d["gop"]
    fbytes = h * w * 2
    assert n % d["base"] == 0 and len(C.read_plan(n, gop, 0, n, 1)) == 1 and len(C.read_plan(n, gop, 0, n, 1)[0]) == 5  # 5 chunks <= 8
    # the byte cut: incompressible chunks, payload between 95 % of the raw size (the test asserts it of the file) and the raw size
    assert C.batch_bytes_bound(h, w, gop, 2, 2 * gop) <= C.BATCH_BYTES < 0.95 * 3 * gop * fbytes  # 2 fit, a third does not: 2/2/1
    assert C.batch_bytes_bound(h, w, gop, 1, n - 4 * gop) <= C.BATCH_BYTES
    # the scratch cut: float32 + motion, two uint16 scratch frames per selected image
    assert 4 * gop * fbytes * 2 == 262144000 <= C.SCRATCH_BYTES < n * fbytes * 2  # 4 chunks fit, the fifth does not: 4/1
    assert gop * fbytes * 2 <= C.SCRATCH_BYTES  # a chunk alone: one batch (the reference read)
    arr = C.frames("uniform", 2, 8, 8, 0)
    assert not np.array_equal(arr[0], arr[1])
