"""GPU: the packed encoder whose waves walk a chunk in mirrored pairs (an even wave backwards, the odd wave after it forwards).

A record is frame f minus frame f - 1 whichever way a wave walks, so every header and every payload word must be what the CPU
restatement (oracle.pyoracle.Oracle.codec_encode_chunk) produces.  Every case below compares EVERY segment and EVERY header with
the oracle and then decodes the batch back to the input bit for bit; nothing is sampled.  The tests look at results only, not at
the order in which a wave produced them: an encoder that walks every wave forwards passes them too.

What the cases are chosen to reach: waves with 0, 1 and 2 records and short last chunks (small GOPs), runs of more than 64 records
in both directions (the header flush in groups of 64), the ragged kernel in both directions (odd frame sizes, an unaligned frame
pointer), waves that stage nothing (a constant scene), waves that all spill (noise), and waves that begin to spill at different
records so that a forward and a backward wave each leave a non-empty part in LDS and a non-empty part in their arena extent."""
import numpy as np
import pytest

from librir_amd.synthetic import s1_noisy_background

pytestmark = pytest.mark.gpu


def _encode_and_compare(dev, oracle, fr, gop, frames_tensor=None, pc=None):
    """Encode `fr` (n, h, w) uint16, compare all of it with the oracle, decode it back; returns the segments as a list of arrays
    indexed [chunk][tile]."""
    import torch

    n, h, w = fr.shape
    if pc is None:
        pc = dev.PackedCodec(w, h, n, gop, stream_bytes="max", workspace_bytes="max")
    t = torch.from_numpy(fr).cuda() if frames_tensor is None else frames_tensor
    batch = pc.encode(t, check=True)
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
    return segments


# ---- every GOP that changes which waves have records, with every kind of short last chunk -----------------------------------
GOPS = [1, 2, 3, 4, 5, 7, 8, 13, 50, 64, 65, 130, 260]
# last chunks of 1, 2 and gop - 1 frames, where the GOP has such a short chunk (GOP 1 has none)
GOP_CASES = [(g, r) for g in GOPS for r in (sorted({1, min(2, g - 1), g - 1}) if g > 1 else [0])]


@pytest.mark.parametrize("gop,last", GOP_CASES, ids=["gop%d_last%d" % c for c in GOP_CASES])
def test_every_gop_and_short_last_chunk(dev, oracle, gop, last):
    """two full chunks and a last chunk of `last` frames (GOP 1 has no short chunk: three chunks), 3 tiles of 512 pixels"""
    n = 2 * gop + last if gop > 1 else 3
    fr = s1_noisy_background(n, 24, 64, seed=100 + gop)
    _encode_and_compare(dev, oracle, fr, gop)


# ---- scenes ------------------------------------------------------------------------------------------------------------------
def _quiet(rng, n, h, w):
    """a fixed background plus 2 bits of noise: a few words per record"""
    bg = rng.integers(1000, 30000, (h, w))
    return (bg[None] + rng.integers(0, 4, (n, h, w))).astype(np.uint16)


def _loud(rng, n, h, w):
    """10 bits of noise: 80-odd words per record, a wave's LDS region holds five of them"""
    return rng.integers(20000, 21024, (n, h, w)).astype(np.uint16)


def _half_and_half(n, h, w, gop, loud_first, seed):
    rng = np.random.default_rng(seed)
    q, l = _quiet(rng, n, h, w), _loud(rng, n, h, w)
    in_second_half = (np.arange(n) % gop) >= gop // 2
    take_loud = ~in_second_half if loud_first else in_second_half
    return np.where(take_loud[:, None, None], l, q)


def _scene(name, n, h, w, gop):
    if name == "s1":
        return s1_noisy_background(n, h, w, seed=5)
    if name == "constant":
        return np.full((n, h, w), 1234, np.uint16)
    if name == "zero":
        return np.zeros((n, h, w), np.uint16)
    if name == "noise":
        return np.random.default_rng(21).integers(0, 65536, (n, h, w)).astype(np.uint16)
    if name == "quiet_then_loud":
        return _half_and_half(n, h, w, gop, False, 31)
    if name == "loud_then_quiet":
        return _half_and_half(n, h, w, gop, True, 32)
    raise KeyError(name)


SCENES = ["s1", "constant", "zero", "noise", "quiet_then_loud", "loud_then_quiet"]


@pytest.mark.parametrize("gop", [50, 130])
@pytest.mark.parametrize("scene", SCENES)
def test_scenes(dev, oracle, scene, gop):
    """two full chunks and a short one of 7 frames, 4 tiles of 512 pixels"""
    n, h, w = 2 * gop + 7, 32, 64
    _encode_and_compare(dev, oracle, _scene(scene, n, h, w, gop), gop)


# ---- the ragged kernel -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gop", [3, 7, 50, 130])
@pytest.mark.parametrize("shape", [(37, 53), (40, 50), (1, 1), (3, 171)], ids=["1961px", "2000px", "1px", "513px"])
@pytest.mark.parametrize("scene", ["s1", "loud_then_quiet", "quiet_then_loud"])
def test_frame_size_that_is_not_a_multiple_of_512_pixels(dev, oracle, scene, shape, gop):
    """1961 and 513 pixels: no 16-byte rows, every tile through the ragged kernel; 2000: three whole tiles and a ragged one"""
    h, w = shape
    n = 2 * gop + min(2, gop - 1)
    _encode_and_compare(dev, oracle, _scene(scene, n, h, w, gop), gop)


@pytest.mark.parametrize("gop", [3, 7, 50, 130])
@pytest.mark.parametrize("offset", [1, 4], ids=["2_bytes", "8_bytes"])
@pytest.mark.parametrize("scene", ["s1", "noise", "quiet_then_loud"])
def test_unaligned_frame_pointer(dev, oracle, scene, offset, gop):
    """frames of 4 whole tiles that do not start on a 16-byte boundary: the ragged kernel takes them all"""
    import torch

    n, h, w = 2 * gop + 1, 32, 64
    fr = _scene(scene, n, h, w, gop)
    flat = torch.zeros((fr.size + 8,), dtype=torch.uint16, device="cuda")
    t = flat[offset:offset + fr.size].view(n, h, w)
    t.copy_(torch.from_numpy(fr).cuda())
    assert t.data_ptr() % 16 != 0 and t.is_contiguous()
    _encode_and_compare(dev, oracle, fr, gop, frames_tensor=t)


# ---- the arena ---------------------------------------------------------------------------------------------------------------
def test_minimal_arena_with_incompressible_frames_reports_it_and_writes_nothing_out_of_bounds(dev, oracle):
    """every wave of every segment spills and the minimal arena has room for one workgroup in sixteen: the status names the arena,
    the canaries on both sides of the stream and of the workspace are intact, and with room for any data the same call succeeds
    and gives the oracle's words"""
    import torch

    n, h, w, gop = 107, 32, 64, 50
    fr = _scene("noise", n, h, w, gop)
    t = torch.from_numpy(fr).cuda()
    pc = dev.PackedCodec(w, h, n, gop, stream_bytes="max")
    cap, wcap = pc.stream.numel(), pc.workspace.numel()
    pad_w, pad_b = 512, 4096  # (the buffers stay 4 KiB aligned inside their canaries)
    big = torch.full((pad_w + cap + pad_w,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    wbig = torch.full((pad_b + wcap + pad_b,), 0xA5, dtype=torch.uint8, device="cuda")
    pc.stream = big[pad_w:pad_w + cap]
    pc.workspace = wbig[pad_b:pad_b + wcap]
    pc.encode(t)
    code, low, high, arena = pc.status()
    assert code & 2, "the status does not name the arena"
    assert arena * 8 > wcap - 4096, "more was asked for than the arena holds"
    with pytest.raises(RuntimeError, match="does not fit"):
        pc.finish()
    for canary, value in ((big[:pad_w], 0x5A5A5A5A5A5A5A5A), (big[pad_w + cap:], 0x5A5A5A5A5A5A5A5A), (wbig[:pad_b], 0xA5), (wbig[pad_b + wcap:], 0xA5)):
        assert bool((canary == value).all()), "wrote outside the buffers it was given"
    pc.grow()
    _encode_and_compare(dev, oracle, fr, gop, pc=pc)


@pytest.mark.parametrize("scene", ["s1", "noise", "loud_then_quiet"])
def test_two_encodes_in_a_row_give_the_same_segments(dev, oracle, scene):
    """the first launch leaves the control block zero: the second one, without a fill before it, places every segment again (wherever
    it arrives) with the same words"""
    n, h, w, gop = 107, 32, 64, 50
    fr = _scene(scene, n, h, w, gop)
    pc = dev.PackedCodec(w, h, n, gop, stream_bytes="max", workspace_bytes="max")
    first = _encode_and_compare(dev, oracle, fr, gop, pc=pc)
    assert pc._clean_ws == pc.workspace.data_ptr(), "the second encode would not be the launch alone"
    second = _encode_and_compare(dev, oracle, fr, gop, pc=pc)
    assert len(first) == len(second)
    for row1, row2 in zip(first, second):
        assert len(row1) == len(row2)
        for a, b in zip(row1, row2):
            assert np.array_equal(a, b)
