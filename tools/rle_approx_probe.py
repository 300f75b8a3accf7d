"""cniic_hilbert_rle_approx_encode (hilbert(rle(d)), d != 0) with device buffers, against the exact `hilbert(rle)` encode of the same
image and against the single-core C restatement of the reference's walk (tests/rle_approx_ref.c, cc -O2 -ffp-contract=off, over the
image already in scan order).  Cases: the 4096^2 and 16384^2 photo-like synthetic images at d = 1, 2, 4, 8, 16; a flat image and
d = inf (all runs 255 long, no distance computed); uniform noise at d = 400 (every start tests 254 pixels).  Every GPU stream is
checked against the C one.  One JSON line per case; --out FILE also writes them there.
    python tools/rle_approx_probe.py [--out profiles/rle_approx_probe.json] [--reps 5] [--sizes 4096,16384] [--no-cpu]"""
import argparse
import json
import math
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import cniic_amd
import rle_approx_ref as R
from cniic_amd import _lib, synth


def best(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    return min(ts) * 1e3, sorted(ts)[len(ts) // 2] * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="4096,16384")
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    clib = None if a.no_cpu else R.compile_c(tempfile.mkdtemp())
    rows = []
    with cniic_amd.Context(0) as ctx:
        for s in [int(x) for x in a.sizes.split(",")]:
            n = s * s
            photo = torch.empty((s, s, 3), dtype=torch.uint8, device=dev)
            ctx.synth_image(_lib.SYNTH_PHOTO, synth.SEED0 + 77, s, s, photo)
            flat = torch.full((s, s, 3), 93, dtype=torch.uint8, device=dev)
            noise = torch.empty((s, s, 3), dtype=torch.uint8, device=dev)
            ctx.synth_image(_lib.SYNTH_UNIFORM, synth.SEED0 + 78, s, s, noise)
            out = torch.empty(8 + 12 * n, dtype=torch.uint8, device=dev)
            cases = [("photo", photo, d) for d in (1.0, 2.0, 4.0, 8.0, 16.0)] + [("flat", flat, 4.0), ("photo", photo, math.inf),
                                                                              ("noise", noise, 400.0)]
            exact_ms = {}
            for kind, img, d in cases:
                if kind not in exact_ms:
                    ctx.encode("hilbert(rle)", img, s, s, out=out)
                    exact_ms[kind] = best(lambda: ctx.encode("hilbert(rle)", img, s, s, out=out), a.reps)
                res = {}

                def run():
                    res["rc"], res["len"] = ctx.hilbert_rle_approx_encode(d, img, s, s, out=out)
                run()
                ms, med = best(run, a.reps)
                row = {"image": kind, "w": s, "h": s, "bytes": res["len"], "runs": (res["len"] - 8) // 12,
                       "gpu_ms_best": round(ms, 3), "gpu_ms_median": round(med, 3), "exact_hilbert_rle_ms": round(exact_ms[kind][0], 3)}
                if clib is not None:
                    lin = ctx.hilbert_linearize(img.cpu().numpy())
                    t = time.perf_counter()
                    exp = R.encode_c(clib, lin, s, s, d)
                    row["cpu_c_ms"] = round((time.perf_counter() - t) * 1e3, 1)
                    row["matches_c"] = out[:res["len"]].cpu().numpy().tobytes() == exp
                    row["speedup_vs_c"] = round(row["cpu_c_ms"] / ms, 1)
                row["d"] = "inf" if math.isinf(d) else d
                rows.append(row)
                print(json.dumps(row), flush=True)
            del photo, flat, noise, out
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
