"""k_sp_pixpack (cniic_amd/csrc/k_points.hip) keeps a thread's 64 labels in 16 registers across its look-back, and that holds only because
the packed words pass through an empty `asm` the compiler cannot see through: without it the kernel needs 128 VGPRs and a scratch
segment.  No GPU is needed to see which it is: the kernel is cross-compiled with the release flags (tools/kernel_regs.sh) and the
compiler's own resource remarks are read."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pixpack_has_no_scratch_segment():
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_regs.sh"), os.path.join(ROOT, "cniic_amd", "csrc", "k_points.hip"), "k_sp_pixpack"],
                         capture_output=True, text=True, check=True).stdout
    lines = [ln for ln in out.splitlines() if "k_sp_pixpack" in ln]
    assert len(lines) == 1, out
    print(lines[0])
    field = lambda name: int(re.search(re.escape(name) + r": (\d+)", lines[0]).group(1))
    assert field("ScratchSize [bytes/lane]") == 0
    assert field("VGPRs Spill") == 0
    assert field("VGPRs") <= 128   # 1024 threads a block
