"""CPU: the codec kernels of the bench step and of the saver are admitted at 8 workgroups of 256 threads per CU.

codec_kernels.hip is compiled device-only for gfx950 with the build's flags, and the resources each kernel records in its code object
metadata are read back.  The admission rule for 256-thread workgroups is min(8, floor(800 / (ceil(sgpr / 16) * 16 + 16))); the
compiler's own "Occupancy" remark does not apply it (it said 7 for a kernel admitted at 6), so the metadata is what is checked."""
import os
import re
import shutil
import subprocess

import pytest

from librir_amd import build as B

HIPCC_FOUND = os.path.exists(B.HIPCC) or shutil.which(B.HIPCC) is not None
pytestmark = pytest.mark.skipif(not HIPCC_FOUND, reason="hipcc not found")

# mangled-name prefixes of the kernels of the step
STEP_KERNELS = {
    "rirb1_decode_packed<true>": "_ZN3rir19rirb1_decode_packedILb1E",
    "rirb1_encode_packed<4,true>": "_ZN3rir19rirb1_encode_packedILi4ELb1E",
    "rirb1_encode_tiles<true>": "_ZN3rir18rirb1_encode_tilesILb1E",  # the saver's encoder (two-pass, stage 1)
}


@pytest.fixture(scope="module")
def metadata(tmp_path_factory):
    asm = str(tmp_path_factory.mktemp("codec_asm") / "codec_kernels.s")
    flags = [f for f in B.COMMON if f != "-fPIC"]
    subprocess.check_call([B.HIPCC] + flags + ["-S", "--cuda-device-only", os.path.join(B.CSRC, "codec_kernels.hip"), "-o", asm],
                          stderr=subprocess.DEVNULL)
    text = open(asm).read()
    meta = text[text.index("amdhsa.kernels:"):text.index(".end_amdgpu_metadata")]
    kernels = {}
    for block in re.split(r"\n  - ", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if not name:
            continue
        fields = dict(re.findall(r"\.(sgpr_count|vgpr_count|private_segment_fixed_size|group_segment_fixed_size):\s+(\d+)", block))
        kernels[name.group(1)] = {k: int(v) for k, v in fields.items()}
    return kernels


def workgroups_per_cu(sgpr):
    return min(8, 800 // ((sgpr + 15) // 16 * 16 + 16))


@pytest.mark.parametrize("kernel", sorted(STEP_KERNELS))
def test_step_kernel_fits_eight_workgroups_per_cu(metadata, kernel):
    found = [m for n, m in metadata.items() if n.startswith(STEP_KERNELS[kernel])]
    assert len(found) == 1, "%s: %d kernels match" % (kernel, len(found))
    m = found[0]
    assert m["sgpr_count"] <= 80, (kernel, m)
    assert m["vgpr_count"] <= 64, (kernel, m)
    assert m["private_segment_fixed_size"] == 0, (kernel, m)
    assert workgroups_per_cu(m["sgpr_count"]) >= 8, (kernel, m)


def test_packed_decoder_uses_no_lds(metadata):
    m = [m for n, m in metadata.items() if n.startswith(STEP_KERNELS["rirb1_decode_packed<true>"])][0]
    assert m["group_segment_fixed_size"] == 0


def test_admission_rule():
    # the general decoder's 106 SGPRs: 6 workgroups; 78 and 80: 8
    assert workgroups_per_cu(106) == 6 and workgroups_per_cu(80) == 8 and workgroups_per_cu(78) == 8 and workgroups_per_cu(81) == 7
