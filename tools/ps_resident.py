#!/usr/bin/env python3
"""How many points of an image the persistent colour K-means keeps in LDS (the rest stay in memory as packed words), from the
host model of its layout (cniic_amd/ps_layout.py): no GPU, no library.

    python3 tools/ps_resident.py [w [h [seed-offset [blocks [bytes of dynamic LDS to compare with]]]]]

Default: the headline image (4096 x 4096 photo, seed + 2) on 256 blocks, against the budget without the running sums in LDS."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from cniic_amd import ps_layout as L, synth

w = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
h = int(sys.argv[2]) if len(sys.argv) > 2 else w
so = int(sys.argv[3]) if len(sys.argv) > 3 else 2
G = int(sys.argv[4]) if len(sys.argv) > 4 else 256
other = int(sys.argv[5]) if len(sys.argv) > 5 else L.PS_BUDGET + L.PS_RUN_BYTES
img = synth.photo(w, h, synth.SEED0 + so).reshape(-1, 3).astype(np.uint32)
keys = np.unique((img[:, 0] << 16) | (img[:, 1] << 8) | img[:, 2])
cells = L.block_cells(keys, G)
print("%d x %d photo (seed + %d): %d distinct colours in %d cells on %d blocks; most cells in a block %d, most points %d"
      % (w, h, so, keys.size, sum(len(c) for c in cells), G, max(len(c) for c in cells), max(int(c.sum()) for c in cells)))
for name, budget in (("this layout", L.PS_BUDGET), ("compared with", other)):
    res, tot, refused = L.resident_points(keys, G, budget)
    print("%-14s %6d bytes of dynamic LDS a block: %d of %d points resident in LDS (%.2f %%), %d blocks refused"
          % (name, budget, res, tot, 100.0 * res / max(tot, 1), refused))
