import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")
    config.addinivalue_line("markers", "perf: asserts a rate floor (GPU box); not part of the parity run - select with -m 'gpu and perf'")


def pytest_collection_modifyitems(config, items):
    """Rate floors are not parity: on a loaded box a perf wobble must not turn the parity run red.  Tests marked `perf` run only
    when the marker expression names them (-m "gpu and perf")."""
    if "perf" in (config.option.markexpr or ""):
        return
    skip = pytest.mark.skip(reason="rate floor: run with -m 'gpu and perf'")
    for it in items:
        if "perf" in it.keywords:
            it.add_marker(skip)


@pytest.fixture(scope="session")
def oracle():
    """The CPU oracle (test infrastructure); built on demand with gcc."""
    so = os.path.join(ROOT, "oracle", "librir_oracle.so")
    src = os.path.join(ROOT, "oracle", "rir_oracle.c")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "librir_oracle.so"])
    from oracle.pyoracle import Oracle

    return Oracle()


@pytest.fixture(scope="session")
def ref():
    """The compiled reference (oracle/_ref) - only where it was built."""
    from oracle.pyoracle import Ref

    if not Ref.available():
        pytest.skip("oracle/_ref not built here (needs /root/reference)")
    return Ref()


REF_ANSWERS = os.path.join(ROOT, "tests", "golden", "reference_answers.json")


class RefAnswers:
    """The compiled reference's answer to each case: asked live where oracle/_ref was built, else as recorded in
    tests/golden/reference_answers.json (a sha256 of the answer's dtypes, shapes and bytes, per case).  With oracle/_ref built,
    RIR_RECORD_REF_ANSWERS=1 rewrites the recorded answers of the cases that ran from the live ones."""

    def __init__(self):
        from oracle.pyoracle import Ref

        self.ref = Ref() if Ref.available() else None
        with open(REF_ANSWERS) as f:
            self.recorded = json.load(f)
        self.record = {} if os.environ.get("RIR_RECORD_REF_ANSWERS") and self.ref is not None else None

    @staticmethod
    def digest(arrays):
        m = hashlib.sha256()
        for a in arrays:
            a = np.ascontiguousarray(a)
            m.update(("%s %s|" % (a.dtype.str, a.shape)).encode())
            m.update(a.tobytes())
        return m.hexdigest()[:32]

    def check(self, key, got, ask):
        """`got` (an array or a tuple of arrays) equals `ask(ref)`, the reference's answer; `key` names the case within the suite"""
        got = tuple(got) if isinstance(got, (tuple, list)) else (got,)
        if self.ref is None:
            assert key in self.recorded, "no recorded reference answer for %r" % key
            assert self.digest(got) == self.recorded[key], key
            return
        want = ask(self.ref)
        want = tuple(want) if isinstance(want, (tuple, list)) else (want,)
        assert len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want)), key
        if self.record is not None:
            assert self.digest(got) == self.digest(want), "equal but not bit for bit: %r" % key
            self.record[key] = self.digest(want)


@pytest.fixture(scope="session")
def ref_answers():
    r = RefAnswers()
    yield r
    if r.record:
        r.recorded.update(r.record)
        with open(REF_ANSWERS, "w") as f:
            json.dump(r.recorded, f, indent=0, sort_keys=True)
            f.write("\n")


@pytest.fixture(scope="session")
def golden():
    d = os.path.join(ROOT, "tests", "golden")
    arrays = np.load(os.path.join(d, "signal_processing.npz"))
    with open(os.path.join(d, "signal_processing_sha256.json")) as f:
        hashes = json.load(f)
    return arrays, hashes


@pytest.fixture(scope="session")
def lib():
    """The product shared object (must exist: built by __graft_entry__.build())."""
    from librir_amd.low_level.misc import _lib

    return _lib


@pytest.fixture(scope="session")
def dev():
    """Device batch API; GPU tests only."""
    import torch

    from librir_amd import device

    assert torch.cuda.is_available(), "GPU test started without a GPU"
    assert device.device_available()
    return device
