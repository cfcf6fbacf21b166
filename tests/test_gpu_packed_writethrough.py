"""GPU: the packed encoder's copy-out of a segment by the 128-byte lines of memory, and the store policies of the packed step.

A segment no wave of which spilled leaves LDS as ONE run: the words in front of the first line boundary and behind the last whole line
as 8-byte stores, the lines between as 16 bytes per lane.  A segment with a spilled wave keeps the copy wave by wave.  Every case
compares EVERY header, segment length and segment word with the CPU restatement (oracle.codec_encode_chunk) and decodes the batch back
to the input (the helper of tests/test_gpu_packed_flush.py).  What the cases reach: segments that start and end on every word of a
line on both cursors, segments shorter than a line and empty ones, a stream buffer whose bytes outside the two extents must keep a
pattern, a spilled wave beside clean ones, a decoder output that is 16-byte but not 128-byte aligned, two encodes on one codec.

Two frame sizes throughout: 64 x 24 (three whole tiles of 512 pixels) and 37 x 35 (1295 pixels: no 16-byte rows, a ragged last tile)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(24, 64), (35, 37)]
SHAPE_IDS = ["64x24", "37x35"]
LINE_WORDS = 16  # 128 bytes
PATTERN = 0xA5


def _encode_and_compare(dev, oracle, fr, gop, pc=None):
    """Encode `fr` (n, h, w) uint16, compare all of it with the oracle, decode it back; returns (segments [chunk][tile], pos, seg,
    batch)."""
    import torch

    n, h, w = fr.shape
    if pc is None:
        pc = dev.PackedCodec(w, h, n, gop, stream_bytes="max", workspace_bytes="max")
    batch = pc.encode(torch.from_numpy(fr).cuda(), check=True)
    pos = batch.seg_pos.cpu().numpy().view(np.uint64)
    seg = batch.seg_words.cpu().numpy().view(np.uint32)
    st = batch.stream.cpu().numpy().view(np.uint64)
    hdr = batch.hdr.cpu().numpy().view(np.uint64)
    assert int(seg.astype(np.int64).sum()) == batch.words == batch.low + batch.high <= st.size
    segments = []
    for c in range(pc.P.nchunks):
        f0 = c * gop
        nf = min(gop, n - f0)
        h_o, o_o, st_o = oracle.codec_encode_chunk(fr[f0:f0 + nf])
        assert np.array_equal(hdr[c][:, :nf], h_o), ("headers", c)
        assert not hdr[c][:, nf:].any(), ("headers past a short chunk", c)
        assert np.array_equal(seg[c], np.diff(o_o)), ("segment lengths", c)
        row = []
        for tl in range(pc.P.ntiles):
            words = st[int(pos[c, tl]):int(pos[c, tl]) + int(seg[c, tl])]
            assert np.array_equal(words, st_o[o_o[tl]:o_o[tl + 1]]), ("segment words", c, tl)
            row.append(words.copy())
        segments.append(row)
    assert np.array_equal(pc.decode(batch).cpu().numpy(), fr), "decode differs from the input"
    return segments, pos, seg, batch


def _noise(rng, n, h, w):
    """full-range 16-bit noise: 128 words a record"""
    return rng.integers(0, 65536, (n, h, w)).astype(np.uint16)


def _quiet(rng, n, h, w):
    bg = rng.integers(1000, 30000, (h, w))
    return (bg[None] + rng.integers(0, 4, (n, h, w))).astype(np.uint16)


def _thirds(n, h, w, gop, outer_loud, seed):
    """every chunk in thirds: noise / quiet / noise (outer_loud) or quiet / noise / quiet"""
    rng = np.random.default_rng(seed)
    q, l = _quiet(rng, n, h, w), _noise(rng, n, h, w)
    in_chunk = np.arange(n) % gop
    middle = (in_chunk >= gop // 3) & (in_chunk < 2 * gop // 3)
    loud = ~middle if outer_loud else middle
    return np.where(loud[:, None, None], l, q)


def _exact_bits(rng, n, h, w, b):
    """frames whose successive differences are noise of exactly b bits in every slot of every tile, with a 0 in every tile (8 b words a
    temporal record)"""
    npx = h * w
    step = rng.integers(0, 1 << b, (n, npx)).astype(np.int64)
    for t0 in range(0, npx, 512):
        step[:, t0] = 0
        k = min(8, npx - t0 - 1)
        step[:, t0 + 1 + np.arange(k)] = (1 << b) - 1
    fr = np.cumsum(step, axis=0) & 0xFFFF
    return fr.astype(np.uint16).reshape(n, h, w)


def _varied_quiet(seed, n, h, w, gop):
    """a fixed background plus 0-4 bits of noise, the width drawn per (chunk, tile) and per slot of the record (pixel p of a tile is in
    slot p % 8; a record has one word per bit of each slot's width): segment lengths that differ word by word"""
    rng = np.random.default_rng(seed)
    npx = h * w
    bg = rng.integers(1000, 30000, npx)
    fr = np.empty((n, npx), np.int64)
    for c in range((n + gop - 1) // gop):
        f0, f1 = c * gop, min(n, (c + 1) * gop)
        for t0 in range(0, npx, 512):
            t1 = min(npx, t0 + 512)
            top = (1 << rng.integers(0, 5, 8))[np.arange(t1 - t0) % 8]  # (exclusive bound of every pixel's noise)
            fr[f0:f1, t0:t1] = bg[t0:t1] + rng.integers(0, top, (f1 - f0, t1 - t0))
    return fr.astype(np.uint16).reshape(n, h, w)


def _widths_in_turn(seed, n, h, w, gop):
    """_exact_bits with widths 1..7 in turn, one per chunk"""
    rng = np.random.default_rng(seed)
    return np.concatenate([_exact_bits(rng, min(gop, n - f0), h, w, 1 + (f0 // gop) % 7) for f0 in range(0, n, gop)])


def _line_positions(pos, seg, cap):
    """word-in-line of every segment's first word and of the word behind its last, per cursor (0: upwards from word 0, 1: downwards from
    the capacity); the stream tensor itself is 128-byte aligned (asserted by the caller)"""
    nchunks, ntiles = seg.shape
    starts, ends = (set(), set()), (set(), set())
    for c in range(nchunks):
        for t in range(ntiles):
            side = (c + t) & 1
            p, l = int(pos[c, t]), int(seg[c, t])
            assert p + l <= cap
            starts[side].add(p % LINE_WORDS)
            ends[side].add((p + l) % LINE_WORDS)
    return starts, ends


# ---- every alignment of a segment's two ends ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("gop,n", [(50, 7 * 50 + 13), (7, 16 * 7 + 3)], ids=["gop50", "gop7"])
def test_segments_start_and_end_on_every_word_of_a_line(dev, oracle, gop, n, shape):
    """Eight chunks (GOP 50) or seventeen (GOP 7), the last one short, three tiles: 12 or 25 segments on each cursor per scene, four
    scenes.  The lengths differ word by word (checked on the oracle's lengths: at least 12 of the 16 residues on each side - a condition
    on the input), so the segments of each extent, which has no holes, start on at least 12 of the 16 words of a line (asserted on what
    the device placed: the order of arrival is its own)."""
    h, w = shape
    scenes = [_varied_quiet(seed, n, h, w, gop) for seed in (101, 102, 103)] + [_widths_in_turn(104, n, h, w, gop)]
    starts, ends, residues = (set(), set()), (set(), set()), (set(), set())
    for fr in scenes:
        _, pos, seg, batch = _encode_and_compare(dev, oracle, fr, gop)
        assert batch.stream.data_ptr() % 128 == 0
        s, e = _line_positions(pos, seg, batch.stream.numel())
        for side in (0, 1):
            starts[side].update(s[side])
            ends[side].update(e[side])
        nchunks, ntiles = seg.shape
        for c in range(nchunks):
            for t in range(ntiles):
                residues[(c + t) & 1].add(int(seg[c, t]) % LINE_WORDS)  # (equal to the oracle's: compared above)
    print("start positions low/high %d/%d, end positions %d/%d, length residues %d/%d" % (
        len(starts[0]), len(starts[1]), len(ends[0]), len(ends[1]), len(residues[0]), len(residues[1])))
    assert len(residues[0]) >= 12 and len(residues[1]) >= 12, "the scenes' lengths do not vary word by word"
    assert len(starts[0]) >= 12 and len(starts[1]) >= 12, (sorted(starts[0]), sorted(starts[1]))


# ---- segments shorter than a line, and empty ones ----------------------------------------------------------------------------------
def _key_words_scene(n, h, w, gop):
    """constant frames whose tiles hold, chunk by chunk, a key record of k = 1 .. 15 words (width k // 8 + (j < k % 8) in slot j, a 0
    in every tile) and temporal records of 0 words"""
    npx = h * w
    ntiles = (npx + 511) // 512
    fr = np.zeros((n, npx), np.uint16)
    for c in range((n + gop - 1) // gop):
        for t in range(ntiles):
            k = 1 + (c * ntiles + t) % 15
            for j in range(8):
                wj = k // 8 + (1 if j < k % 8 else 0)
                if wj and t * 512 + 8 + j < npx:
                    fr[c * gop:(c + 1) * gop, t * 512 + 8 + j] = (1 << wj) - 1  # pixel p of a tile is in slot p % 8
    return fr.reshape(n, h, w)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("scene", ["constant", "zeros", "key_1_to_15_words"])
def test_segments_shorter_than_a_line_and_empty_ones(dev, oracle, scene, shape):
    """constant frames: temporal records of 0 words, a segment is its key record; an all-zero stack: every segment is empty; key records
    of 1 .. 15 words: only the 8-byte stores of the two ends.  GOP 7, five chunks and one of two frames."""
    h, w = shape
    n, gop = 37, 7
    if scene == "constant":
        fr = np.repeat(np.random.default_rng(111).integers(0, 65536, (1, h, w)).astype(np.uint16), n, axis=0)
    elif scene == "zeros":
        fr = np.zeros((n, h, w), np.uint16)
    else:
        fr = _key_words_scene(n, h, w, gop)
    _, _, seg, _ = _encode_and_compare(dev, oracle, fr, gop)
    if scene == "zeros":
        assert not seg.any()
    if scene == "key_1_to_15_words":
        assert seg.min() >= 1 and seg.max() <= 15 and len(set(seg.reshape(-1).tolist())) >= 12, sorted(set(seg.reshape(-1).tolist()))


# ---- nothing written outside the segments ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("scene", ["varied_quiet", "widths_in_turn", "noise_quiet_noise"])
def test_nothing_is_written_outside_the_two_extents(dev, oracle, scene, shape):
    """the stream buffer holds 0xA5 before the encode: every byte outside [0, low) and [cap - high, cap) still does afterwards, and
    inside - two extents without holes - every segment is the oracle's (a 16-byte store that runs over a neighbour's end, or over the
    end of an extent, shows in one or the other)"""
    import torch

    h, w = shape
    n, gop = (16 * 7 + 3, 7) if scene != "noise_quiet_noise" else (113, 50)
    fr = {"varied_quiet": lambda: _varied_quiet(121, n, h, w, gop), "widths_in_turn": lambda: _widths_in_turn(122, n, h, w, gop),
          "noise_quiet_noise": lambda: _thirds(n, h, w, gop, True, 123)}[scene]()
    pc = dev.PackedCodec(w, h, n, gop, stream_bytes="max", workspace_bytes="max")
    pc.stream.view(torch.uint8).fill_(PATTERN)
    _, _, _, batch = _encode_and_compare(dev, oracle, fr, gop, pc=pc)
    cap = pc.stream.numel()
    assert batch.low + batch.high < cap
    between = pc.stream[batch.low:cap - batch.high].view(torch.uint8)
    assert bool((between == PATTERN).all()), "wrote outside the two extents"


# ---- a spilled wave beside clean ones ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("scene", ["noise_quiet_noise", "quiet_noise_quiet", "only_wave_0"])
def test_a_spilled_wave_beside_clean_ones(dev, oracle, scene, shape):
    """GOP 50 in thirds: the outer waves (0 backwards, 3 forwards) or the inner ones (1 forwards, 2 backwards) spill, the others do not -
    the copy wave by wave under the new policy.  only_wave_0: frames 0 .. 11 of every chunk are noise (wave 0's share: the key record
    and 11 more, 1536 words for a region of 448), the rest is quiet.  Two full chunks and one of 13 frames, whose segments do not spill
    (waves of 3-4 records): both copies in one launch."""
    h, w = shape
    n, gop = 113, 50
    if scene == "only_wave_0":
        rng = np.random.default_rng(131)
        q, l = _quiet(rng, n, h, w), _noise(rng, n, h, w)
        fr = np.where((np.arange(n) % gop < 12)[:, None, None], l, q)
    else:
        fr = _thirds(n, h, w, gop, scene == "noise_quiet_noise", 132)
    _encode_and_compare(dev, oracle, fr, gop)


# ---- the decoder's frame stores -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_decode_into_a_view_that_is_not_line_aligned(dev, oracle, shape):
    """`out` begins 16 bytes into a larger tensor (16-byte, not 128-byte aligned) that holds a pattern: the frames are exact, the bytes
    in front and behind keep the pattern"""
    import torch

    h, w = shape
    n, gop = 23, 7
    fr = _varied_quiet(141, n, h, w, gop)
    pc = dev.PackedCodec(w, h, n, gop, stream_bytes="max", workspace_bytes="max")
    batch = pc.encode(torch.from_numpy(fr).cuda(), check=True)
    pad, count = 8, n * h * w  # uint16 elements
    big = torch.full(((pad + count + 64) * 2,), PATTERN, dtype=torch.uint8, device="cuda")
    assert big.data_ptr() % 128 == 0
    out = big[pad * 2:(pad + count) * 2].view(torch.uint16).view(n, h, w)
    assert out.data_ptr() % 16 == 0 and out.data_ptr() % 128 != 0
    pc.decode(batch, out=out)
    assert np.array_equal(out.cpu().numpy(), fr)
    assert bool((big[:pad * 2] == PATTERN).all()) and bool((big[(pad + count) * 2:] == PATTERN).all()), "wrote outside the output"


# ---- two encodes back to back ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_two_encodes_back_to_back_give_the_same_segments(dev, oracle, shape):
    """the control block is left clean: the second encode is the launch alone and places the same segments"""
    h, w = shape
    n, gop = 16 * 7 + 3, 7
    fr = _varied_quiet(151, n, h, w, gop)
    pc = dev.PackedCodec(w, h, n, gop, stream_bytes="max", workspace_bytes="max")
    first, _, _, _ = _encode_and_compare(dev, oracle, fr, gop, pc=pc)
    assert pc._clean_ws == pc.workspace.data_ptr(), "the second encode would not be the launch alone"
    second, _, _, _ = _encode_and_compare(dev, oracle, fr, gop, pc=pc)
    for row1, row2 in zip(first, second):
        for a, b in zip(row1, row2):
            assert np.array_equal(a, b)
