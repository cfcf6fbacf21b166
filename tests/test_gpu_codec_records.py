"""GPU: the codec on records the other codec tests never make (codec_cases.py): MODE_LEFT key records, widths that differ inside a
record, the step between the narrow and the wide tier at every block, every (mode, block, width) cell, the tie of the key-mode rule.

test_codec_cases_cpu.py shows on the CPU what these frames hold; here every encoder (two-pass, single-pass, slotted, packed) is compared
with the oracle word for word, every decoder (dense, slotted, packed, rir_codec_decode_chunks_device, the selective decode behind
IRMovie.to_tensor) gives the frames back, from the GPU's own output and from the oracle's laid out on the host.  Everything is exact
equality with the oracle or with the input frames: no tolerance, no measured number.  One oracle pass per (scene, GOP) serves all tests.

By hand, on a scratch copy, three breaks of codec_kernels.hip:
  - left_integrate without the carry across lanes: four tests in five of this file turn red (every decoder, decode_chunks and the
    recordings included); all of test_gpu_codec.py, the frozen-format hash too, stays green.
  - `use_left` computed with <=: 44 tests of this file turn red (the tie frame and every scene with a uniform-16 key record, in all
    four encoders).  test_gpu_codec.py sees this one as well, in its noise cases: an incompressible tile costs 128 words either way.
  - the tie given to LEFT only where 0 < words < 128: the tie frame turns red in all four encoders (8 tests); of test_gpu_codec.py only
    the frozen-format hash notices."""
import numpy as np
import pytest

import codec_cases as C
import device_io_cases as DC
from test_gpu_codec import _encode_and_compare_dense, _grid_reference, to_np

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SEED = 11


def _ragged(name):
    return {n: (fr, off) for n, fr, off in C.ragged_scene(SEED)}[name]


SCENES = {
    "raw": lambda: C.record_scene(SEED, "raw"),
    "left": lambda: C.record_scene(SEED, "left"),
    "key_raw": lambda: C.key_scene(SEED + 1, "raw"),
    "key_left": lambda: C.key_scene(SEED + 1, "left"),
    "tie": C.tie_frames,
    "left_cut": lambda: _ragged("left_cut")[0],
    "ramp": lambda: _ragged("ramp")[0],
}
# (scene, GOP, elements the frame pointer is off the 16-byte grid).  48 frames: GOP 48 is one chunk, GOP 7 six chunks and a short one of
# 6 frames whose later key frames are whatever the data gives, GOP 130 is larger than the stack; GOP 1: every record a key record.
CASES = [(s, g, 0) for s in ("raw", "left") for g in (48, 7, 130)]
CASES += [("key_raw", 1, 0), ("key_left", 1, 0), ("tie", 1, 0), ("tie", 3, 0)]
CASES += [("left_cut", 48, 0), ("left_cut", 7, 0), ("ramp", 3, 0), ("ramp", 2, 0), ("ramp", 1, 0)]
CASES += [("raw", 48, 1), ("raw", 7, 3), ("left", 7, 1), ("left", 48, 3)]
EVERY_CASE = pytest.mark.parametrize("scene,gop,offset", CASES, ids=["%s_gop%d_off%d" % c for c in CASES])


def _reference(oracle, scene, gop):
    """(frames, [(headers, tile offsets, stream) of the oracle per chunk])"""
    return _grid_reference(oracle, ("records", scene, gop), SCENES[scene], gop)


def _on_device(fr, offset=0, fill=None):
    """a contiguous uint16 device tensor shaped like `fr` that starts `offset` elements past a 16-byte boundary: holding `fr`, or `fill`"""
    flat = torch.from_numpy(np.full(fr.size + 8, 0 if fill is None else fill, np.uint16)).cuda()
    t = flat[offset:offset + fr.size].view(*fr.shape)
    if fill is None:
        t.copy_(torch.from_numpy(np.array(fr)).cuda())
    assert t.data_ptr() % 16 == 2 * offset and t.is_contiguous()
    return t


def _chunk_frames(n, gop):
    return [min(gop, n - f0) for f0 in range(0, n, gop)]


# ---- the four encoders against the oracle, each decoder on what its encoder wrote --------------------------------------------------
@pytest.mark.parametrize("single_pass", [False, True], ids=["two_pass", "single_pass"])
@EVERY_CASE
def test_dense_encoders_equal_oracle(dev, oracle, scene, gop, offset, single_pass):
    """rir_codec_encode_device and the single-pass encoder (status 0): headers, zero headers past a short chunk, tile and chunk offsets,
    every stream word; rir_codec_decode_device gives the input back"""
    fr, chunks = _reference(oracle, scene, gop)
    _encode_and_compare_dense(dev, fr, chunks, gop, single_pass, offset=offset)


@EVERY_CASE
def test_slotted_encoder_equals_oracle(dev, oracle, scene, gop, offset):
    """encode_tiles: headers, segment lengths and the words of every slot; decode_slots gives the input back; encode_compact makes the
    oracle's dense stream and tables of the same slots"""
    fr, chunks = _reference(oracle, scene, gop)
    n, h, w = fr.shape
    ctx = dev.CodecContext(w, h, n, gop)
    ctx.encode_tiles(_on_device(fr, offset))
    assert np.array_equal(ctx.decode_slots().cpu().numpy(), fr), "decode_slots differs from the input"
    seg_t, slots_t = ctx.slots()
    seg, slots = seg_t.cpu().numpy().view(np.uint32), slots_t.cpu().numpy().view(np.uint64)
    hdr = ctx.hdr.cpu().numpy().view(np.uint64)
    assert len(chunks) == ctx.layout.nchunks
    for c, ((h_o, o_o, st_o), nf) in enumerate(zip(chunks, _chunk_frames(n, gop))):
        assert np.array_equal(hdr[c][:, :nf], h_o), ("headers", c)
        assert not hdr[c][:, nf:].any(), ("headers past a short chunk", c)
        assert np.array_equal(seg[c], np.diff(o_o)), ("segment lengths", c)
        for tl in range(ctx.layout.ntiles):
            assert np.array_equal(slots[c, tl, :seg[c, tl]], st_o[o_o[tl]:o_o[tl + 1]]), ("slot words", c, tl)
    enc = ctx.encode_compact()
    _, toff, coff, st = to_np(enc)
    assert coff[0] == 0 and ctx.slots_payload_bytes() == enc.total_words() * 8
    for c, (h_o, o_o, st_o) in enumerate(chunks):
        assert np.array_equal(toff[c], o_o), ("tile offsets", c)
        assert coff[c + 1] - coff[c] == st_o.size, ("chunk offsets", c)
        assert np.array_equal(st[coff[c]:coff[c + 1]], st_o), ("stream words", c)
    assert np.array_equal(ctx.decode(enc).cpu().numpy(), fr), "decode of the compacted stream differs from the input"


@EVERY_CASE
def test_packed_encoder_equals_oracle(dev, oracle, scene, gop, offset):
    """rir_codec_encode_packed_device (waves that walk a chunk backwards keep their key frame in LDS): headers, segment lengths, the words
    of every segment, the two extents without holes; rir_codec_decode_packed_device gives the input back"""
    fr, chunks = _reference(oracle, scene, gop)
    n, h, w = fr.shape
    pc = dev.PackedCodec(w, h, n, gop, stream_bytes="max", workspace_bytes="max")
    batch = pc.encode(_on_device(fr, offset), check=True)
    pos = batch.seg_pos.cpu().numpy().view(np.uint64)
    seg = batch.seg_words.cpu().numpy().view(np.uint32)
    st = batch.stream.cpu().numpy().view(np.uint64)
    hdr = batch.hdr.cpu().numpy().view(np.uint64)
    assert int(seg.astype(np.int64).sum()) == batch.words == batch.low + batch.high <= st.size
    assert batch.words == sum(c[2].size for c in chunks) and len(chunks) == pc.P.nchunks
    order = np.argsort(pos.ravel(), kind="stable")
    p, s = pos.ravel()[order].astype(np.int64), seg.ravel()[order].astype(np.int64)
    p, s = p[s > 0], s[s > 0]  # (empty segments may share a position)
    nlow = int(np.searchsorted(p, batch.low))  # segments of the low extent [0, low); the rest fill [capacity - high, capacity)
    assert np.array_equal(p[:nlow], np.concatenate([[0], np.cumsum(s[:nlow])])[:nlow]) and int(s[:nlow].sum()) == batch.low, "holes in the low extent"
    assert np.array_equal(p[nlow:], st.size - batch.high + np.concatenate([[0], np.cumsum(s[nlow:])])[:p.size - nlow]), "holes in the high extent"
    for c, ((h_o, o_o, st_o), nf) in enumerate(zip(chunks, _chunk_frames(n, gop))):
        assert np.array_equal(hdr[c][:, :nf], h_o), ("headers", c)
        assert not hdr[c][:, nf:].any(), ("headers past a short chunk", c)
        assert np.array_equal(seg[c], np.diff(o_o)), ("segment lengths", c)
        for tl in range(pc.P.ntiles):
            assert np.array_equal(st[int(pos[c, tl]):int(pos[c, tl]) + int(seg[c, tl])], st_o[o_o[tl]:o_o[tl + 1]]), ("segment words", c, tl)
    assert np.array_equal(pc.decode(batch).cpu().numpy(), fr), "decode differs from the input"


# ---- the three decoders on what the oracle wrote --------------------------------------------------------------------------------------
def _as_int64(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


@pytest.mark.parametrize("layout", ["dense", "slots", "packed"])
@EVERY_CASE
def test_gpu_decodes_oracle_records(dev, oracle, scene, gop, offset, layout):
    """the oracle's chunks as a dense batch, scattered into slots and shuffled into a packed batch decode on the GPU to the input, into an
    output `offset` elements off the 16-byte grid (the decoders' ragged form takes whole tiles then)"""
    fr, chunks = _reference(oracle, scene, gop)
    n, h, w = fr.shape
    ctx = dev.CodecContext(w, h, n, gop)
    L = ctx.layout
    hdr = np.zeros((L.nchunks, L.ntiles, gop), np.uint64)
    for c, (h_o, _, _) in enumerate(chunks):
        hdr[c][:, :h_o.shape[1]] = h_o
    out = _on_device(fr, offset, fill=0xABCD)
    if layout == "dense":
        toff = np.stack([o_o for _, o_o, _ in chunks]).astype(np.uint32)
        coff = np.concatenate([[0], np.cumsum([s_o.size for _, _, s_o in chunks])]).astype(np.int64)
        st = np.concatenate([s_o for _, _, s_o in chunks] + [np.zeros(1, np.uint64)])
        enc = dev.EncodedBatch(L, _as_int64(hdr), torch.from_numpy(toff.view(np.int32)).cuda(), torch.from_numpy(coff).cuda(), _as_int64(st))
        ctx.decode(enc, out=out)
    elif layout == "slots":
        seg_t, slots_t = ctx.slots()
        seg = np.zeros(tuple(seg_t.shape), np.uint32)
        slots = np.full(tuple(slots_t.shape), 0xDEADBEEFDEADBEEF, np.uint64)
        for c, (_, o_o, s_o) in enumerate(chunks):
            seg[c] = np.diff(o_o)
            for tl in range(L.ntiles):
                slots[c, tl, :seg[c, tl]] = s_o[o_o[tl]:o_o[tl + 1]]
        ctx.hdr.copy_(_as_int64(hdr))
        seg_t.copy_(torch.from_numpy(seg.view(np.int32)))
        slots_t.copy_(_as_int64(slots))
        ctx.decode_slots(out=out)
    else:
        pc = dev.PackedCodec(w, h, n, gop, stream_bytes="max")
        keys = [(c, tl) for c in range(L.nchunks) for tl in range(L.ntiles)]
        np.random.default_rng(5).shuffle(keys)
        pos = np.zeros((L.nchunks, L.ntiles), np.uint64)
        seg = np.zeros((L.nchunks, L.ntiles), np.uint32)
        parts, at = [], 0
        for c, tl in keys:
            _, o_o, s_o = chunks[c]
            words = s_o[o_o[tl]:o_o[tl + 1]]
            pos[c, tl], seg[c, tl] = at, words.size
            parts.append(words)
            at += words.size
        st = np.concatenate(parts + [np.zeros(1, np.uint64)])
        batch = dev.PackedBatch(pc, _as_int64(hdr), _as_int64(pos), torch.from_numpy(seg.view(np.int32)).cuda(), _as_int64(st), at, 0)
        pc.decode(batch, out=out)
    assert np.array_equal(out.cpu().numpy(), fr)


# ---- rir_codec_decode_chunks_device -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,offset", [("left", 0), ("left", 3), ("left_cut", 0), ("raw", 1)])
def test_decode_chunks_places_permuted_chunks(dev, oracle, scene, offset):
    """the chunks of a record scene at GOP 7, in a permuted order and in two calls that each take a subset, their streams gathered behind a
    few foreign words: chunk_frames puts each chunk, the short last one included, at its frames of `out`; what a call does not name keeps
    the sentinel; `error` stays 0"""
    gop = 7
    fr, _ = _reference(oracle, scene, gop)
    n, h, w = fr.shape
    ctx = dev.CodecContext(w, h, n, gop)
    enc = ctx.encode(_on_device(fr))
    coff = enc.chunk_off.cpu().numpy()
    nchunks = ctx.layout.nchunks
    assert nchunks == 7 and n - 6 * gop == 6
    out = _on_device(fr, offset, fill=0xABCD)
    error = torch.zeros((1,), dtype=torch.int32, device="cuda")
    done = np.zeros(n, bool)
    for subset in ([4, 0, 6, 2], [5, 1, 3]):
        idx = torch.tensor(subset, device="cuda")
        parts = [torch.full((5,), 0x5A5A5A5A, dtype=torch.int64, device="cuda")] + [enc.stream[int(coff[c]):int(coff[c + 1])] for c in subset]
        sizes = [p.numel() for p in parts]
        chunk_off = torch.tensor(np.cumsum(sizes), dtype=torch.int64, device="cuda")
        chunk_frames = torch.tensor([[c * gop, min(gop, n - c * gop)] for c in subset], dtype=torch.int64, device="cuda")
        dev.decode_chunks(enc.hdr[idx].contiguous(), enc.tile_off[idx].contiguous(), chunk_off, torch.cat(parts), chunk_frames, out, gop, error)
        torch.cuda.synchronize()
        assert int(error.item()) == 0
        for c in subset:
            done[c * gop:(c + 1) * gop] = True
        got = out.cpu().numpy()
        assert np.array_equal(got[done], fr[done]), subset
        assert (got[~done] == 0xABCD).all(), "a frame no entry names was written"
    assert done.all() and np.array_equal(out.cpu().numpy(), fr)


# ---- recordings: the selective decode (rirb1_decode_select) on LEFT keys of wide and mixed widths, with walks that stop early ------------
@pytest.mark.parametrize("name,gop", [("left12", 5), ("raw12", 5), ("ramp", 2), ("ramp", None)])
def test_recordings_of_designed_records_read_back(tmp_path, oracle, name, gop):
    from librir_amd.video_io import IRMovie
    from test_gpu_device_io import record
    from test_gpu_device_io_full_range import check_numpy

    arr = C.ramp_frames() if name == "ramp" else np.array(C.record_scene(SEED, name[:-2])[:12])
    n = arr.shape[0]
    key_modes = C.header_fields(oracle.codec_encode_chunk(arr[:gop or n])[0])[0][:, 0]
    assert (key_modes == (C.MODE_RAW if name == "raw12" else C.MODE_LEFT)).all()  # (the first key records are all of one mode)
    with IRMovie.from_filename(record(tmp_path / "m.h264", arr, gop)) as mov:
        assert mov.images == n
        assert np.array_equal(mov.to_tensor().cpu().numpy(), arr)
        check_numpy(mov, arr, DC.selections(n, gop or DC.DEFAULT_GOP))
