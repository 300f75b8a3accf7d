"""cniic_codec_decode_batch against a loop of cniic_codec_decode, and cniic_mse_batch against a loop of cniic_mse, with device buffers
(the streams as cniic_codec_encode_batch wrote them).  One JSON line per case; --out FILE also writes them there.
    python tools/decode_batch_probe.py [--out profiles/decode_batch_probe.json] [--reps 3] [--only-batch]
--only-batch: the batched decode of the first case alone (for a profiler run of its own)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import cniic_amd
from cniic_amd import _lib, synth

CASES = [("cluster-colors(256)", 128, 1920, 1080), ("hufman", 256, 512, 512), ("delta", 16, 1024, 1024)]


def best(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    return min(ts) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only-batch", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    rows = []
    with cniic_amd.Context(0) as ctx:
        for expr, F, w, h in CASES[:1] if a.only_batch else CASES:
            fr = torch.empty((F, h, w, 3), dtype=torch.uint8, device=dev)
            for f in range(F):
                ctx.synth_image(_lib.SYNTH_PHOTO, synth.SEED0 + 3000 + f, w, h, fr[f])
            stride = w * h * (3 if expr.startswith("cluster") else 16) + (1 << 16)
            enc = torch.zeros(stride * F, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            rc, lens, _, _ = ctx.encode_batch(expr, fr, w, h, F, enc, stride)
            assert rc == 0, rc
            img = w * h * 3
            out = torch.zeros(img * F, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            batch = lambda: ctx.decode_batch(expr, enc, stride, lens, F, out, img)
            if a.only_batch:
                batch()
                return
            out1 = torch.zeros(img * F, dtype=torch.uint8, device=dev)

            def loop():
                for f in range(F):
                    ctx.decode_into(expr, enc[f * stride:], lens[f], out1[f * img:(f + 1) * img])
            t_batch, t_loop = best(batch, a.reps), best(loop, a.reps)
            row = dict(case="decode", codec=expr, frames=F, w=w, h=h, stream_mb=round(sum(lens) / 2 ** 20, 1), loop_ms=round(t_loop, 3),
                       batch_ms=round(t_batch, 3), same=bool(torch.equal(out, out1)))
            print(json.dumps(row), flush=True)
            rows.append(row)
            if expr.startswith("cluster"):
                src = fr.reshape(-1)
                mb = lambda: ctx.mse_batch(src, out, w * h, F)
                def mse1(f):
                    v = C.c_double(0)
                    ctx._L.cniic_mse(ctx.h, _lib._ptr(src[f * img:]), _lib._ptr(out[f * img:]), C.c_uint64(w * h), C.byref(v))
                    return v.value
                ml = lambda: [mse1(f) for f in range(F)]
                row = dict(case="mse", frames=F, w=w, h=h, loop_ms=round(best(ml, a.reps), 3), batch_ms=round(best(mb, a.reps), 3), same=mb() == ml())
                print(json.dumps(row), flush=True)
                rows.append(row)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
