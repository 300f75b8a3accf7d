"""The kernels the staged points of a cluster-colors encode pass through (cniic_amd/csrc/k_points.hip: k_cc_front_b, whose cell scan
now names the persistent launch's chunk boundaries; k_cc_front_c, whose ranges role checks the fit; k_sp_partlab, with its staged
source; k_kmeans_persist.hip: k_rgbw_persist, whose set-up makes key and initial label of every point) keep no scratch segment and
spill no vector register; the two that run 1024 threads a block stay inside 128 VGPRs.  No GPU is needed to see it: the kernels are
cross-compiled with the release flags (tools/kernel_regs.sh) and the compiler's own resource remarks are read.
profiles/cc_points_resources.txt has the lines beside the parent's."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = {   # name as the remarks spell it -> (source file, threads a block)
    "k_cc_front_b": ("k_points.hip", 256),
    "k_cc_front_c": ("k_points.hip", 1024),
    "k_sp_partlabIh": ("k_points.hip", 1024),
    "k_sp_partlabIt": ("k_points.hip", 1024),
    "k_rgbw_persist": ("k_kmeans_persist.hip", 1024),
}


@pytest.fixture(scope="module")
def remarks():
    out = {}
    for src in sorted({s for s, _ in KERNELS.values()}):
        out[src] = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_regs.sh"), os.path.join(ROOT, "cniic_amd", "csrc", src), "k_cc_front_|k_sp_partlab|k_rgbw_persist"],
                                  capture_output=True, text=True, check=True).stdout
    return out


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_no_scratch_no_vector_spills_and_the_block_fits(remarks, kernel):
    src, threads = KERNELS[kernel]
    lines = [ln for ln in remarks[src].splitlines() if kernel in ln]
    assert len(lines) == 1, remarks[src]
    print(lines[0])
    field = lambda name: int(re.search(re.escape(name) + r": (\d+)", lines[0]).group(1))
    assert field("ScratchSize [bytes/lane]") == 0
    assert field("VGPRs Spill") == 0
    if threads == 1024:
        assert field("VGPRs") <= 128
