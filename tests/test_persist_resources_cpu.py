"""k_rgbw_persist (cniic_amd/csrc/k_kmeans_persist.hip) runs 1024 threads a block, so it has 128 vector registers a lane and not one more:
a version that needs more spills to a scratch segment, which this kernel once did (NOTES AC: 64 B a lane, 28 scratch accesses inside the
loop) and which nothing in the suite noticed.  Every loop-carried value added to its iteration loop can bring that back.  No GPU is needed
to see it: the kernel is cross-compiled with the release flags (tools/kernel_regs.sh) and the compiler's own resource remarks are read,
as tests/test_kernel_resources_cpu.py does for k_sp_pixpack.  profiles/persist_trips_resources.txt has the line beside the parent's."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_persist_has_no_scratch_segment_and_no_spilled_vector_register():
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_regs.sh"), os.path.join(ROOT, "cniic_amd", "csrc", "k_kmeans_persist.hip"), "k_rgbw_persist"],
                         capture_output=True, text=True, check=True).stdout
    lines = [ln for ln in out.splitlines() if "k_rgbw_persist" in ln]
    assert len(lines) == 1, out
    print(lines[0])
    field = lambda name: int(re.search(re.escape(name) + r": (\d+)", lines[0]).group(1))
    assert field("ScratchSize [bytes/lane]") == 0
    assert field("VGPRs Spill") == 0
    assert field("VGPRs") <= 128   # 1024 threads a block
