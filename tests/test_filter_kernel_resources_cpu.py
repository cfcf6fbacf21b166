"""CPU: the frame-buffer filter unit keeps every kernel's state in registers.  Its wave-tile kernels share their parts (tile decode, column
loader, border weight, wave shifts: filter_kernels.hip), inlined into kernels with very different register budgets - and the regular-tile
kernel of the fused chain is built for 8 waves per SIMD (amdgpu_waves_per_eu): a register beyond 64 there does not lower its occupancy, it
becomes scratch.  Looks at the kernels' resource metadata only."""
import os
import re
import shutil
import subprocess

import pytest

from librir_amd import build as B

HIPCC_FOUND = os.path.exists(B.HIPCC) or shutil.which(B.HIPCC) is not None


@pytest.mark.skipif(not HIPCC_FOUND, reason="hipcc not found")
def test_filter_kernels_resources(tmp_path):
    asm = str(tmp_path / "filter_kernels.s")
    flags = [f for f in B.COMMON if f != "-fPIC"]
    done = subprocess.run([B.HIPCC] + flags + ["-S", "--cuda-device-only", os.path.join(B.CSRC, "filter_kernels.hip"), "-o", asm], stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0, done.stdout
    text = open(asm).read()
    meta = text[text.index("amdhsa.kernels:"):text.index(".end_amdgpu_metadata")]
    kernels = {}
    for block in re.split(r"\n  - ", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            field = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1))
            kernels[name.group(1)] = {"scratch": field("private_segment_fixed_size"), "lds": field("group_segment_fixed_size"), "vgpr": field("vgpr_count")}
    assert len(kernels) == 48, sorted(kernels)
    assert all(k["scratch"] == 0 for k in kernels.values()), {n: k["scratch"] for n, k in kernels.items() if k["scratch"]}
    regular = [k for n, k in kernels.items() if "filter_chain_regular_kernel" in n]
    assert len(regular) == 1 and regular[0]["vgpr"] <= 64, regular
    chain = {n: k["lds"] for n, k in kernels.items() if "filter_chain" in n}
    # filter_chain_kernel<2 / 3 / 4>, and radius 1 as the regular and the listed kernel: one [4][16][64] float strip each
    assert len(chain) == 5 and all(v == 16384 for v in chain.values()), chain
    assert [k["lds"] for n, k in kernels.items() if "median3x3_kernel" in n] == [8192]
