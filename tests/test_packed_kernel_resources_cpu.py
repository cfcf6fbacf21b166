"""CPU: the packed step's FAST kernels keep their state in registers.  rirb1_encode_packed<4, true> is built for 8 waves per SIMD
(amdgpu_waves_per_eu): a register beyond 64 there does not lower its occupancy, it becomes scratch - and its copy-out of a segment maps
words to waves through small arrays that must stay registers.  Looks at the kernels' resource metadata only."""
import os
import re
import shutil
import subprocess

import pytest

from librir_amd import build as B

HIPCC_FOUND = os.path.exists(B.HIPCC) or shutil.which(B.HIPCC) is not None


@pytest.mark.skipif(not HIPCC_FOUND, reason="hipcc not found")
def test_packed_fast_kernels_resources(tmp_path):
    asm = str(tmp_path / "codec_kernels.s")
    flags = [f for f in B.COMMON if f != "-fPIC"]
    done = subprocess.run([B.HIPCC] + flags + ["-S", "--cuda-device-only", os.path.join(B.CSRC, "codec_kernels.hip"), "-o", asm], stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0, done.stdout
    text = open(asm).read()
    meta = text[text.index("amdhsa.kernels:"):text.index(".end_amdgpu_metadata")]
    kernels = {}
    for block in re.split(r"\n  - ", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            field = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1))
            kernels[name.group(1)] = {"scratch": field("private_segment_fixed_size"), "vgpr": field("vgpr_count")}
    enc = [k for n, k in kernels.items() if n.startswith("_ZN3rir19rirb1_encode_packedILi4ELb1EEE")]
    dec = [k for n, k in kernels.items() if n.startswith("_ZN3rir19rirb1_decode_packedILb1EEE")]
    assert len(enc) == 1 and len(dec) == 1, sorted(kernels)
    assert enc[0]["scratch"] == 0 and enc[0]["vgpr"] <= 64, enc
    assert dec[0]["scratch"] == 0 and dec[0]["vgpr"] <= 64, dec
