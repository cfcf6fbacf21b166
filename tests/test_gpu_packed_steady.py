"""GPU: the packed form in steady state.

The packing kernel leaves its control block zero and its result on the status line, so encode after encode runs without a fill launch.
Covered here: many encodes in a row, each with its own status; a batch over its budget followed by one within it, with and without a
status() in between; and the packed decoder's kernels (FAST and ragged) refusing positions and lengths outside the stream and malformed
headers."""
import numpy as np
import pytest

from librir_amd.synthetic import s1_noisy_background

pytestmark = pytest.mark.gpu

# (n, h, w, gop): whole tiles only; a ragged last tile; the bench's frame size
SHAPES = [(12, 64, 128, 5), (9, 67, 83, 4), (60, 512, 640, 50)]


def _dense_words(dev, t, gop):
    n, h, w = t.shape
    return dev.CodecContext(w, h, n, gop).encode(t).total_words()


@pytest.mark.parametrize("n,h,w,gop", SHAPES)
def test_back_to_back_encodes_each_report_their_own_status(dev, n, h, w, gop):
    import torch

    a = torch.from_numpy(s1_noisy_background(n, h, w, seed=21)).cuda()
    b = torch.from_numpy((s1_noisy_background(n, h, w, seed=22) >> 3).astype(np.uint16)).cuda()  # (fewer words than `a`)
    words = {id(a): _dense_words(dev, a, gop), id(b): _dense_words(dev, b, gop)}
    assert words[id(a)] != words[id(b)]
    pc = dev.PackedCodec(w, h, n, gop)
    for i in range(24):
        t = a if i % 3 else b
        pc.encode(t)
        if i % 4 == 3:
            continue  # (no status in between: the next encode starts from the block this one left)
        code, low, high, arena = pc.status()
        assert code == 0 and low + high == words[id(t)], (i, code, low, high)
        out = pc.decode()
        assert torch.equal(out.view(torch.int16), t.view(torch.int16)), i
    # the same on frames that are not 16-byte aligned: every tile through the ragged kernels
    raw = torch.empty(n * h * w + 1, dtype=torch.uint16, device="cuda")
    u = raw[1:].view(n, h, w)
    u.copy_(a)
    for i in range(6):
        pc.encode(u)
        code, low, high, _ = pc.status()
        assert code == 0 and low + high == words[id(a)], i
        out = torch.empty(n * h * w + 1, dtype=torch.uint16, device="cuda")[1:].view(n, h, w)
        pc.decode(out=out)
        assert torch.equal(out.view(torch.int16), a.view(torch.int16)), i


@pytest.mark.parametrize("with_status", [True, False], ids=["status_between", "no_status_between"])
def test_over_budget_encode_then_a_good_one(dev, with_status):
    import torch

    n, h, w, gop = 12, 67, 83, 5
    bad = torch.from_numpy(np.random.default_rng(4).integers(0, 65536, (n, h, w)).astype(np.uint16)).cuda()
    good = torch.from_numpy(s1_noisy_background(n, h, w, seed=5)).cuda()
    want = _dense_words(dev, good, gop)
    pc = dev.PackedCodec(w, h, n, gop)  # the 8 bit-per-pixel budget and the minimal arena
    for _ in range(2):
        pc.encode(bad)
        if with_status:
            code, low, high, _ = pc.status()
            assert code & 1 and (low + high) > pc.stream.numel()
        # no status(): the codec still takes the block for clean - what the kernel left behind is all the next encode sees
        pc.encode(good, reset=with_status)
        code, low, high, arena = pc.status()
        assert code == 0 and low + high == want, (code, low, high, arena)
        out = pc.decode()
        assert torch.equal(out.view(torch.int16), good.view(torch.int16))


def _batch(dev, n, h, w, gop, seed):
    import torch

    t = torch.from_numpy(s1_noisy_background(n, h, w, seed=seed)).cuda()
    pc = dev.PackedCodec(w, h, n, gop)
    batch = pc.encode(t, check=True)
    return pc, batch, t


def _tampered(dev, pc, batch):
    return dev.PackedBatch(pc, batch.hdr.clone(), batch.seg_pos.clone(), batch.seg_words.clone(), batch.stream, batch.low, batch.high)


@pytest.mark.parametrize("n,h,w,gop", SHAPES[:2])
@pytest.mark.parametrize("aligned_out", [True, False], ids=["fast", "ragged_only"])
def test_packed_decoder_refuses_malformed_tables(dev, n, h, w, gop, aligned_out):
    import torch

    pc, batch, t = _batch(dev, n, h, w, gop, 31)
    P = pc.P
    cap = batch.stream.numel()

    def out():
        if aligned_out:
            return torch.empty((n, h, w), dtype=torch.uint16, device="cuda")
        return torch.empty(n * h * w + 1, dtype=torch.uint16, device="cuda")[1:].view(n, h, w)

    good = pc.decode(batch, out=out())
    assert torch.equal(good.view(torch.int16), t.view(torch.int16))
    pos = batch.seg_pos.cpu().numpy().view(np.uint64).astype(np.int64)
    seg = batch.seg_words.cpu().numpy().view(np.uint32).astype(np.int64)
    end = pos + seg
    last = np.unravel_index(int(np.argmax(end)), end.shape)  # the segment that ends at the end of the stream
    assert int(end[last]) == cap
    # a first tile (FAST kernel when the output is aligned) and the frame's last tile (ragged when the frame is)
    for c, tl in ((P.nchunks - 1, 0), (0, P.ntiles - 1)):
        for what in ("pos_past_end", "pos_huge", "pos_near_end"):
            b2 = _tampered(dev, pc, batch)
            v = {"pos_past_end": cap + 1, "pos_huge": 2 ** 63, "pos_near_end": cap - 1}[what]
            b2.seg_pos[c, tl] = np.array(v, np.uint64).view(np.int64).item()
            if what == "pos_near_end" and int(seg[c, tl]) <= 1:
                continue
            with pytest.raises(RuntimeError, match="malformed"):
                pc.decode(b2, out=out())
        b2 = _tampered(dev, pc, batch)
        b2.seg_words[c, tl] += 1  # (the walk no longer ends at the end of its segment)
        with pytest.raises(RuntimeError, match="malformed"):
            pc.decode(b2, out=out())
        b2 = _tampered(dev, pc, batch)
        b2.hdr[c, tl, 0] = b2.hdr[c, tl, 0] | (3 << 14)  # mode 3: no such mode
        with pytest.raises(RuntimeError, match="malformed"):
            pc.decode(b2, out=out())
    b2 = _tampered(dev, pc, batch)
    b2.seg_words[last] += 1  # a length that runs past the end of the stream
    with pytest.raises(RuntimeError, match="malformed"):
        pc.decode(b2, out=out())
    # and the untouched batch still decodes
    again = pc.decode(batch, out=out())
    assert torch.equal(again.view(torch.int16), t.view(torch.int16))
