"""k_cc_front_a / b / c (cniic_amd/csrc/k_points.hip) each hold the bodies of several kernels, and a kernel's registers are those of
its hungriest role: the third one is launched with 1024 threads a block, which 128 VGPRs at most allow, and a scratch segment would
put a memory round trip into roles that are pure latency.  No GPU is needed to see it: the kernels are cross-compiled with the
release flags (tools/kernel_regs.sh) and the compiler's own resource remarks are read."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THREADS = {"k_cc_front_a": 256, "k_cc_front_b": 256, "k_cc_front_c": 1024}


@pytest.fixture(scope="module")
def remarks():
    return subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_regs.sh"), os.path.join(ROOT, "cniic_amd", "csrc", "k_points.hip"), "k_cc_front_"],
                          capture_output=True, text=True, check=True).stdout


@pytest.mark.parametrize("kernel", sorted(THREADS))
def test_front_kernels_have_no_scratch_and_fit_their_blocks(remarks, kernel):
    lines = [ln for ln in remarks.splitlines() if kernel in ln]
    assert len(lines) == 1, remarks
    print(lines[0])
    field = lambda name: int(re.search(re.escape(name) + r": (\d+)", lines[0]).group(1))
    assert field("ScratchSize [bytes/lane]") == 0
    assert field("VGPRs Spill") == 0
    if THREADS[kernel] == 1024:
        assert field("VGPRs") <= 128
