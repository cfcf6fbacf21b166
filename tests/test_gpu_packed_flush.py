"""GPU: the staged encoders' store-free sink.  A wave files every record in its LDS region; when a record does not fit, the region's
words - the records the wave produced first - are flushed to the wave's spill area and the region starts again, as often as it takes.

Every packed case compares EVERY header, segment length and segment word with the CPU restatement (oracle.codec_encode_chunk) and
decodes the batch back to the input, as tests/test_gpu_packed_mirrored.py does.  What the cases reach: several flushes per wave in
both directions (an even wave walks backwards, an odd one forwards), flushes that start and stop at different records, a wave whose
words fill its region exactly and one whose words exceed it by one record, header groups of 64 interleaved with flushes, waves with
0, 1 or 2 records, a full arena, and the dense single-pass encoder with its static spill area.

Two frame sizes throughout: 64 x 24 (three whole tiles of 512 pixels) and 37 x 35 (1295 pixels: no 16-byte rows, a ragged last tile)."""
import numpy as np
import pytest

from librir_amd.synthetic import s1_noisy_background

pytestmark = pytest.mark.gpu

SHAPES = [(24, 64), (35, 37)]
SHAPE_IDS = ["64x24", "37x35"]
REC_MAX_WORDS = 128  # RIRB1_REC_MAX_WORDS
WAVES = 4


def _encode_and_compare(dev, oracle, fr, gop, pc=None):
    """Encode `fr` (n, h, w) uint16, compare all of it with the oracle, decode it back; returns (segments [chunk][tile], headers
    [chunk] (ntiles, nf) from the oracle)."""
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
    segments, headers = [], []
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
        headers.append(h_o)
    assert np.array_equal(pc.decode(batch).cpu().numpy(), fr), "decode differs from the input"
    return segments, headers


def _noise(rng, n, h, w):
    """full-range 16-bit noise: 128 words a record, a region of 448 words holds three"""
    return rng.integers(0, 65536, (n, h, w)).astype(np.uint16)


def _quiet(rng, n, h, w):
    """a fixed background plus 2 bits of noise: a few words per record"""
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


# ---- several flushes per wave ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("scene", ["noise", "noise_quiet_noise", "quiet_noise_quiet"])
def test_several_flushes_per_wave(dev, oracle, scene, shape):
    """GOP 50: a wave has 12-13 records; on noise (128 words each) it fills its 448-word region three to four times.  The mixed scenes
    make the flushes start and stop at different records of a forward and of a backward wave.  Two full chunks and one of 13 frames."""
    h, w = shape
    n, gop = 113, 50
    if scene == "noise":
        fr = _noise(np.random.default_rng(41), n, h, w)
    else:
        fr = _thirds(n, h, w, gop, scene == "noise_quiet_noise", 42)
    _encode_and_compare(dev, oracle, fr, gop)


# ---- the boundary: a wave's words fill its region exactly / exceed it by one record ----------------------------------------------
def _staged_lds_words(gop, waves=WAVES):
    """the host's staged_lds_words (codec_kernels.hip): words of a wave's LDS region"""
    share = (gop + 1 + waves - 1) // waves + 1
    return min(448 * 4 // waves, share * REC_MAX_WORDS)


def _enc_split(w, waves, nf):
    if w <= 0:
        return 0
    if w >= waves:
        return nf
    b = (w * (nf + 1) + waves // 2) // waves - 1
    return (min(nf, 1) if b < 1 else min(b, nf))


def _cuts(nf, waves=WAVES):
    """the packed encoder's cuts (enc_split_mirrored): wave w packs records [cuts[w], cuts[w + 1])"""
    c = [_enc_split(w, waves, nf) for w in range(waves + 1)]
    if waves == 4:
        c[3] = min(nf, 2 * c[2] - c[1])
    return c


def _record_words(hdr):
    """payload words of each record from its header: field q (16 bits) = w_q | w_{4+q} << 5 | ..."""
    hdr = hdr.astype(np.uint64)
    tot = np.zeros(hdr.shape, np.int64)
    for q in range(4):
        f = (hdr >> np.uint64(16 * q)) & np.uint64(0xFFFF)
        tot += (f & np.uint64(31)).astype(np.int64) + ((f >> np.uint64(5)) & np.uint64(31)).astype(np.int64)
    return tot


def _exact_bits(rng, n, h, w, b):
    """frames whose successive differences are noise of exactly b bits in every slot of every tile, with a 0 in every tile: the
    temporal records have base 0, width b in all 8 slots and 8 b words"""
    npx = h * w
    step = rng.integers(0, 1 << b, (n, npx)).astype(np.int64)
    for t0 in range(0, npx, 512):
        step[:, t0] = 0  # the tile's minimum
        k = min(8, npx - t0 - 1)
        step[:, t0 + 1 + np.arange(k)] = (1 << b) - 1  # one pixel of full width in each of the 8 slots (pixel p of a tile is in slot p % 8)
    fr = np.cumsum(step, axis=0) & 0xFFFF  # (the codec's differences are modulo 2^16 as well)
    return fr.astype(np.uint16).reshape(n, h, w)


# (bits, GOP whose waves 1-3 hold exactly a region's words, GOP with one record more each): 8 x 56 = 14 x 32 = 448 words
BOUNDARY = [(7, 31, 35), (4, 55, 59)]


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("bits,gop_exact,gop_over", BOUNDARY, ids=["wide_7bit", "narrow_4bit"])
def test_region_filled_exactly_and_exceeded_by_one_record(dev, oracle, bits, gop_exact, gop_over, shape):
    """Every temporal record of every tile (the ragged one too: all 8 slots occur in it) has 8 * bits words.  With gop_exact, waves 1-3
    produce exactly the words their region holds (no flush); with gop_over one record more, which does not fit (one flush of the whole
    region).  The arithmetic is checked here from the oracle's headers and the encoder's cuts, the results against the oracle as
    everywhere."""
    h, w = shape
    for gop, extra in ((gop_exact, 0), (gop_over, 1)):
        cap = _staged_lds_words(gop)
        assert cap == 448
        fr = _exact_bits(np.random.default_rng(50 + gop), gop + 3, h, w, bits)
        _, headers = _encode_and_compare(dev, oracle, fr, gop)
        per_record = _record_words(headers[0])  # (ntiles, gop)
        assert (per_record[:, 1:] == 8 * bits).all(), "the scene does not give 8 b words a record"
        cuts = _cuts(gop)
        for wv in (1, 2, 3):
            total = per_record[:, cuts[wv]:cuts[wv + 1]].sum(axis=1)
            assert (total == cap + extra * 8 * bits).all(), ("wave total", gop, wv, total, cap)


# ---- more than 64 records per wave, and very few ----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("gop", [130, 260])
def test_header_groups_and_flushes_interleave(dev, oracle, gop, shape):
    """GOP 130: 32-33 records a wave; GOP 260: 65-66, so a wave's headers leave in two groups while it flushes every third record.  One
    full chunk and a short one of 9 frames."""
    h, w = shape
    n = gop + 9
    _encode_and_compare(dev, oracle, _noise(np.random.default_rng(60 + gop), n, h, w), gop)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_gops_1_to_8_on_noise(dev, oracle, shape):
    """waves with 0, 1 or 2 records; the region is the worst case of the wave's share there, so nothing is flushed"""
    h, w = shape
    for gop in range(1, 9):
        n = 2 * gop + 1  # two full chunks and one of a single frame
        _encode_and_compare(dev, oracle, _noise(np.random.default_rng(70 + gop), n, h, w), gop)


# ---- the arena --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_full_arena_is_reported_and_nothing_is_written_behind_the_workspace(dev, oracle, shape):
    """the default (minimal) workspace on noise: status bit 1, finish() raises, the bytes behind (and in front of) the workspace keep
    their pattern; after grow() the encode is exact and a second encode right after it gives the same segments (the control block
    was left clean)"""
    import torch

    h, w = shape
    n, gop = 113, 50
    fr = _noise(np.random.default_rng(80), n, h, w)
    t = torch.from_numpy(fr).cuda()
    pc = dev.PackedCodec(w, h, n, gop, stream_bytes="max")
    wcap, pad = pc.workspace.numel(), 4096
    wbig = torch.full((pad + wcap + pad,), 0xA5, dtype=torch.uint8, device="cuda")
    pc.workspace = wbig[pad:pad + wcap]
    pc.encode(t)
    code, _, _, arena = pc.status()
    assert code & 2, "the status does not name the arena"
    assert arena * 8 > wcap - 4096, "no more was asked for than the arena holds"
    with pytest.raises(RuntimeError, match="does not fit"):
        pc.finish()
    assert bool((wbig[:pad] == 0xA5).all()) and bool((wbig[pad + wcap:] == 0xA5).all()), "wrote outside the workspace"
    pc.grow()
    first, _ = _encode_and_compare(dev, oracle, fr, gop, pc=pc)
    assert pc._clean_ws == pc.workspace.data_ptr(), "the second encode would not be the launch alone"
    second, _ = _encode_and_compare(dev, oracle, fr, gop, pc=pc)
    for row1, row2 in zip(first, second):
        for a, b in zip(row1, row2):
            assert np.array_equal(a, b)


# ---- the dense single-pass encoder (static spill area, every wave forwards) ---------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("scene", ["noise", "s1"])
def test_dense_single_pass_equals_two_pass(dev, scene, shape):
    import torch

    h, w = shape
    n, gop = 113, 50
    fr = _noise(np.random.default_rng(90), n, h, w) if scene == "noise" else s1_noisy_background(n, h, w, seed=9)
    t = torch.from_numpy(fr).cuda()
    ctx = dev.CodecContext(w, h, n, gop)
    outs = []
    for single in (False, True):
        enc = ctx.encode(t, single_pass=single)
        torch.cuda.synchronize()
        coff = enc.chunk_off.cpu().numpy().copy()
        outs.append((enc.hdr.cpu().numpy().copy(), enc.tile_off.cpu().numpy().copy(), coff, enc.stream.cpu().numpy()[:int(coff[-1])].copy()))
        if single:
            assert np.array_equal(ctx.decode(enc).cpu().numpy(), fr)
    for a, b, what in zip(outs[0], outs[1], ("headers", "tile offsets", "chunk offsets", "stream")):
        assert np.array_equal(a, b), what
