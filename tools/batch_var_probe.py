"""The calls for batches of differently sized images against what there was before them, device buffers throughout:
  cniic_codec_encode_batch_var   against a loop of cniic_codec_encode on one context (100 images with sizes like DIV2K's validation set)
                                 and, on 64 equal 1920 x 1080 frames, against cniic_codec_encode_batch
  cniic_mse_batch_var            against a loop of cniic_mse, and its bytes per second against cniic_mse of ONE pair of the same total size
  cniic_codec_measure_batch      against the loop of cniic_codec_encode, cniic_codec_decode and cniic_mse
One JSON line per case (median / min / max of --reps timed runs after --warmup untimed ones); --out FILE also writes them there.
    python tools/batch_var_probe.py [--out profiles/batch_var_probe.json] [--reps 5] [--warmup 1] [--only mse|encode]
--only: one batched call and nothing else (for a profiler run of its own)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import cniic_amd
from cniic_amd import _lib, synth

CODECS = ("cluster-colors(256)", "hufman", "delta")


def div2k_like_sizes():
    """100 (w, h): the long side is 2040, six in ten have the commonest short side 1356, the rest spread over 665 ... 1982; one in seven
    is a portrait"""
    out = []
    for i in range(100):
        short = 1356 if i % 10 < 6 else 648 + (i * 7919) % 1393
        out.append((short, 2040) if i % 7 == 3 else (2040, short))
    return out


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return dict(median_ms=round(statistics.median(ts), 3), min_ms=round(min(ts), 3), max_ms=round(max(ts), 3))


def verdict(new, old):
    """new is not slower than old when its median is below old's median plus the run-to-run spread of both"""
    spread = (new["max_ms"] - new["min_ms"]) + (old["max_ms"] - old["min_ms"])
    return dict(ratio_old_over_new=round(old["median_ms"] / new["median_ms"], 3), not_slower=bool(new["median_ms"] <= old["median_ms"] + spread))


def mse1(ctx, a, b, npx):
    v = C.c_double(0)
    ctx._L.cniic_mse(ctx.h, _lib._ptr(a), _lib._ptr(b), C.c_uint64(npx), C.byref(v))
    return v.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only", choices=("mse", "encode"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    rows = []

    def emit(**row):
        print(json.dumps(row), flush=True)
        rows.append(row)

    sizes = div2k_like_sizes()
    F = len(sizes)
    ws, hs = [w for w, _ in sizes], [h for _, h in sizes]
    nbytes = [3 * w * h for w, h in sizes]
    offs = [sum(nbytes[:f]) for f in range(F)]            # back to back: most frames off the 16-byte boundaries
    offs16 = [0] * F
    for f in range(1, F):
        offs16[f] = (offs16[f - 1] + nbytes[f - 1] + 15) & ~15
    with cniic_amd.Context(0) as ctx:
        src = torch.empty(offs16[-1] + nbytes[-1] + 16, dtype=torch.uint8, device=dev)       # (room for either layout)
        src16 = torch.empty_like(src)
        for f, (w, h) in enumerate(sizes):
            ctx.synth_image(_lib.SYNTH_PHOTO, synth.SEED0 + 6000 + f, w, h, src[offs[f]:])
            src16[offs16[f]:offs16[f] + nbytes[f]] = src[offs[f]:offs[f] + nbytes[f]]
        back = torch.zeros_like(src)
        mpix = sum(w * h for w, h in sizes) / 1e6
        torch.cuda.synchronize()
        if a.only == "mse":
            ctx.mse_batch_var(src, offs, src16, offs16, [n // 3 for n in nbytes])
            return
        for expr in CODECS:
            stride = (max(nbytes) // 3 * (2 if expr.startswith("cluster") else 16) + (1 << 16) + 3) & ~3
            enc = torch.zeros(stride * F, dtype=torch.uint8, device=dev)
            enc1 = torch.zeros(stride * F, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            res = {}

            def batch():
                res["b"] = ctx.encode_batch_var(expr, src, offs, ws, hs, enc, stride)
            if a.only == "encode":
                batch()
                return

            def loop():
                res["l"] = [ctx.encode(expr, src[offs[f]:], w=ws[f], h=hs[f], out=enc1[f * stride:(f + 1) * stride])[1] for f in range(F)]
            t_b, t_l = timed(batch, a.reps, a.warmup), timed(loop, a.reps, a.warmup)
            lens = res["b"][1]
            same = res["b"][0] == 0 and lens == res["l"] and all(torch.equal(enc[f * stride:f * stride + lens[f]], enc1[f * stride:f * stride + lens[f]]) for f in range(F))
            emit(case="encode_batch_var vs loop of cniic_codec_encode", codec=expr, frames=F, mpix=round(mpix, 1), batch=t_b, loop=t_l, same=bool(same), **verdict(t_b, t_l))

            # the whole loop body: encode + decode + MSE
            def measure():
                res["m"] = ctx.measure_batch(expr, src, offs, ws, hs)

            def three():
                out = []
                for f in range(F):
                    n = ctx.encode(expr, src[offs[f]:], w=ws[f], h=hs[f], out=enc1[f * stride:(f + 1) * stride])[1]
                    ctx.decode_into(expr, enc1[f * stride:], n, back[offs[f]:offs[f] + nbytes[f]])
                    out.append((n, mse1(ctx, src[offs[f]:], back[offs[f]:], nbytes[f] // 3)))
                res["t"] = out
            t_m, t_t = timed(measure, a.reps, a.warmup), timed(three, a.reps, a.warmup)
            same = res["m"][0] == 0 and [(r["compressed_size"], r["error"]) for r in res["m"][1]] == res["t"]
            emit(case="measure_batch vs loop of encode + decode + mse", codec=expr, frames=F, mpix=round(mpix, 1), batch=t_m, loop=t_t, same=bool(same), **verdict(t_m, t_t))
            del enc, enc1

        # ---- the MSE alone: `back` holds the last codec's decoded images at the sources' offsets; src16 the sources, every pair aligned
        npx = [n // 3 for n in nbytes]
        back16 = torch.empty_like(src)
        for f in range(F):
            back16[offs16[f]:offs16[f] + nbytes[f]] = src[offs[f]:offs[f] + nbytes[f]]
        back16[::7] ^= 1
        torch.cuda.synchronize()
        total = sum(nbytes)
        res = {}

        def var_mis():
            res["v"] = ctx.mse_batch_var(src, offs, back16, offs16, npx)      # a off its boundaries, b on them: unrelated alignments

        def var_al():
            res["a"] = ctx.mse_batch_var(src16, offs16, back16, offs16, npx)

        def loop():
            res["l"] = [mse1(ctx, src[offs[f]:], back16[offs16[f]:], npx[f]) for f in range(F)]

        def one():
            res["o"] = mse1(ctx, src16, back16, total // 3)
        t_v, t_a, t_l, t_o = timed(var_mis, a.reps, a.warmup), timed(var_al, a.reps, a.warmup), timed(loop, a.reps, a.warmup), timed(one, a.reps, a.warmup)
        gbs = lambda t: round(2 * total / (t["median_ms"] * 1e-3) / 1e9, 1)
        emit(case="mse_batch_var vs loop of cniic_mse", frames=F, mbytes_per_side=round(total / 1e6, 1), batch_misaligned=t_v, batch_aligned=t_a, loop=t_l,
             one_pair_of_the_same_size_k_sqerr=t_o, gbytes_per_s=dict(batch_misaligned=gbs(t_v), batch_aligned=gbs(t_a), k_sqerr=gbs(t_o)),
             misaligned_over_aligned=round(t_v["median_ms"] / t_a["median_ms"], 3), same=bool(res["v"] == res["l"] == res["a"]), **verdict(t_v, t_l))
        del back, back16, src16

        # ---- equal frames: the new call against cniic_codec_encode_batch
        F2, w, h = 64, 1920, 1080
        fr = torch.empty((F2, h, w, 3), dtype=torch.uint8, device=dev)
        for f in range(F2):
            ctx.synth_image(_lib.SYNTH_PHOTO, synth.SEED0 + 7000 + f, w, h, fr[f])
        stride = w * h * 2 + (1 << 16)
        enc = torch.zeros(stride * F2, dtype=torch.uint8, device=dev)
        enc1 = torch.zeros(stride * F2, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        expr = "cluster-colors(256)"
        o2 = [f * w * h * 3 for f in range(F2)]

        def var():
            res["v"] = ctx.encode_batch_var(expr, fr, o2, [w] * F2, [h] * F2, enc, stride)

        def eq():
            res["e"] = ctx.encode_batch(expr, fr, w, h, F2, enc1, stride)
        t_v, t_e = timed(var, a.reps, a.warmup), timed(eq, a.reps, a.warmup)
        emit(case="encode_batch_var vs cniic_codec_encode_batch, equal frames", codec=expr, frames=F2, w=w, h=h, var=t_v, equal=t_e,
             same=bool(res["v"][1] == res["e"][1] and torch.equal(enc, enc1)), **verdict(t_v, t_e))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
