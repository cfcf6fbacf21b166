"""CPU: the bounded-loss unit keeps every kernel's state in registers.  The two resident kernels are built for a fixed number of waves per SIMD
(amdgpu_waves_per_eu): a register too many does not lower their occupancy, it becomes scratch - and the shared per-pixel helpers are where
that has happened (two sides of a branch storing through one pointer).  Looks at the kernels' resource metadata only."""
import os
import re
import shutil
import subprocess

import pytest

from librir_amd import build as B

HIPCC_FOUND = os.path.exists(B.HIPCC) or shutil.which(B.HIPCC) is not None


@pytest.mark.skipif(not HIPCC_FOUND, reason="hipcc not found")
def test_lossy_kernels_use_no_scratch(tmp_path):
    asm = str(tmp_path / "lossy_kernels.s")
    flags = [f for f in B.COMMON if f != "-fPIC"]
    done = subprocess.run([B.HIPCC] + flags + ["-S", "--cuda-device-only", os.path.join(B.CSRC, "lossy_kernels.hip"), "-o", asm], stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0, done.stdout
    text = open(asm).read()
    meta = text[text.index("amdhsa.kernels:"):text.index(".end_amdgpu_metadata")]
    kernels = {}
    for block in re.split(r"\n  - ", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            kernels[name.group(1)] = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1))
    # 3 pair counts x (running average or none) x (addLoss or not) x (constant budgets, speculative)
    assert len([k for k in kernels if "lossy_const_run_kernel" in k]) == 24, sorted(kernels)
    assert any("lossy_run_kernel" in k for k in kernels) and any("lossy_run_parked_kernel" in k for k in kernels)
    assert all(v == 0 for v in kernels.values()), {k: v for k, v in kernels.items() if v}
