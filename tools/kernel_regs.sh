#!/bin/bash
# tools/kernel_regs.sh file.hip [pattern]: SGPRs, VGPRs, AGPRs, spills, scratch, LDS and occupancy of each kernel of one source file (gfx950),
# from the release flags; one line per kernel
f=$1; pat=${2:-.}
o=$(mktemp --suffix=.o) && trap 'rm -f "$o"' EXIT
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -x hip -c "$f" -o "$o" -Rpass-analysis=kernel-resource-usage 2>&1 \
 | grep -E "remark: +(Function Name|TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill|LDS Size \[bytes/block\]):" \
 | sed -E 's/.*remark: +//; s/ \[-Rpass.*//' \
 | awk '/^Function Name:/ {if (line) print line; line=$3; next} {line=line " | " $0} END {if (line) print line}' | grep -E "$pat"
