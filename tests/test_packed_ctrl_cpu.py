"""CPU: when PackedCodec.encode zeroes the encoder's control block first (a fill launch) and when it launches the packing kernel alone.

The packing kernel leaves its control block zero when it runs to its end, so a workspace known to be clean needs no fill.  A block not
known to be clean is still zeroed: a new workspace, a workspace put in place of the old one, after grow(), after an encode whose status
was not 0.  The C entry points are replaced by a recorder here; what the kernel does is checked on the GPU
(tests/test_gpu_packed_steady.py)."""
import ctypes as ct

import pytest

from librir_amd import device as D


class Recorder:
    """stands in for the library: records which encode entry point is called, answers status() with a chosen code"""

    def __init__(self):
        self.calls = []
        self.code = 0

    def rir_codec_encode_packed_device(self, *a):
        self.calls.append("fill+pack")
        return 0

    def rir_codec_encode_packed_launch_device(self, *a):
        self.calls.append("pack")
        return 0

    def rir_codec_packed_reset_device(self, *a):
        self.calls.append("fill")
        return 0

    def rir_codec_encode_packed_status(self, ws, out, stream):
        out[0], out[1], out[2] = 10, 20, 0
        return self.code


@pytest.fixture
def pc(monkeypatch):
    import torch

    codec = D.PackedCodec(64, 32, 10, 4, device="cpu")  # (the layout query runs on the host)
    rec = Recorder()
    monkeypatch.setattr(D, "_lib", rec)
    monkeypatch.setattr(D, "_frames3", lambda t, dtype=None: t)
    monkeypatch.setattr(D, "_stream", lambda: ct.c_void_p(0))
    codec.frames = torch.zeros((10, 32, 64), dtype=torch.uint16)
    codec.rec = rec
    return codec


def test_steady_state_is_one_launch(pc):
    for _ in range(4):
        pc.encode(pc.frames)
    assert pc.rec.calls == ["fill+pack", "pack", "pack", "pack"]


def test_status_zero_keeps_the_block_clean(pc):
    pc.encode(pc.frames)
    assert pc.status() == (0, 10, 20, 0)
    pc.encode(pc.frames)
    assert pc.rec.calls == ["fill+pack", "pack"]


@pytest.mark.parametrize("code", [1, 2, 3])
def test_block_is_zeroed_after_a_failed_encode(pc, code):
    pc.encode(pc.frames)
    pc.rec.code = code
    with pytest.raises(RuntimeError, match="does not fit"):
        pc.finish()
    pc.rec.code = 0
    pc.encode(pc.frames)
    pc.encode(pc.frames)
    assert pc.rec.calls == ["fill+pack", "fill+pack", "pack"]


def test_block_is_zeroed_after_grow(pc):
    pc.encode(pc.frames)
    pc.grow()
    pc.encode(pc.frames)
    assert pc.rec.calls == ["fill+pack", "fill+pack"]


def test_block_is_zeroed_in_a_workspace_put_in_place(pc):
    import torch

    pc.encode(pc.frames)
    pc.workspace = torch.empty_like(pc.workspace)
    pc.encode(pc.frames)
    assert pc.rec.calls == ["fill+pack", "fill+pack"]


def test_reset_then_launch_alone(pc):
    """bench.py --full times the packing kernel alone: reset(), then encode(reset=False) - never a fill inside encode"""
    for _ in range(2):
        pc.reset()
        pc.encode(pc.frames, reset=False)
    pc.encode(pc.frames)
    assert pc.rec.calls == ["fill", "pack", "fill", "pack", "pack"]


def test_status_error_raises(pc):
    pc.rec.code = -1
    with pytest.raises(RuntimeError, match="status failed"):
        pc.status()
    pc.rec.code = 0
    pc.encode(pc.frames)
    assert pc.rec.calls == ["fill+pack"]
