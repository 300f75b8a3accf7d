"""The calls for batches of differently sized images against what there was before them, device buffers throughout:
  cniic_codec_encode_batch_var   against a loop of cniic_codec_encode on one context (100 images with sizes like DIV2K's validation set)
                                 and, on 64 equal 1920 x 1080 frames, against cniic_codec_encode_batch
  cniic_mse_batch_var            against a loop of cniic_mse, and its bytes per second against cniic_mse of ONE pair of the same total size
  cniic_codec_measure_batch      against the loop of cniic_codec_encode, cniic_codec_decode and cniic_mse
One JSON line per case (median / min / max of --reps timed runs after --warmup untimed ones); --out FILE also writes them there.
    python tools/batch_var_probe.py [--out profiles/batch_var_probe.json] [--reps 5] [--warmup 1] [--only mse|encode|rle-decode]
--only: one batched call and nothing else (for a profiler run of its own).

  --hilbert [--against OTHER.so]   the Hilbert-RLE rules of the reference's Makefile on the same 100 images: cniic_codec_decode_batch of
                                 `hilbert(rle)`, `hilbert(rle(4))` and `hilbert(rle(16))` streams (the approximate ones written by
                                 cniic_hilbert_rle_approx_encode, decoded as `hilbert(rle)`: every build of the library takes that) and
                                 cniic_codec_measure_batch where the library takes the expression.  --against names another build of the
                                 library in cniic_amd/ (CNIIC_LIB_FILE): the two are then timed in child processes in alternation, --rounds
                                 times --reps runs each, and the medians compared."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if "--lib-file" in sys.argv:   # (before the package loads the library)
    os.environ["CNIIC_LIB_FILE"] = sys.argv[sys.argv.index("--lib-file") + 1]
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


HILBERT_D = (0.0, 4.0, 16.0)
SWEEP = ((64, 64, 256), (256, 256, 256), (512, 384, 256), (800, 600, 128), (1024, 1000, 100), (1024, 1024, 100), (1200, 900, 100), (2040, 1356, 100))


def hilbert_times(a):
    """this library's raw times (ms) per case, as one JSON line"""
    dev = torch.device("cuda", 0)
    out = {}
    if a.sweep:   # frames of ONE size per batch, d = 4 only: where the batched decode stops paying
        for w, h, F in SWEEP:
            hilbert_case(a, dev, "%dx%d x%d " % (w, h, F), [(w, h)] * F, (4.0,), out)
    else:
        hilbert_case(a, dev, "", div2k_like_sizes(), HILBERT_D, out)
    print("HILBERT " + json.dumps(out), flush=True)


def hilbert_case(a, dev, tag, sizes, ds, out):
    F = len(sizes)
    ws, hs = [w for w, _ in sizes], [h for _, h in sizes]
    nbytes = [3 * w * h for w, h in sizes]
    offs = [sum(nbytes[:f]) for f in range(F)]
    with cniic_amd.Context(0) as ctx:
        src = torch.empty(offs[-1] + nbytes[-1] + 16, dtype=torch.uint8, device=dev)
        for f, (w, h) in enumerate(sizes):
            ctx.synth_image(_lib.SYNTH_PHOTO, synth.SEED0 + 6000 + f, w, h, src[offs[f]:])
        img_stride = max(nbytes)
        back = torch.zeros(img_stride * F, dtype=torch.uint8, device=dev)
        for d in ds:
            name = "hilbert(rle)" if d == 0.0 else "hilbert(rle(%g))" % d
            lens, streams = [], []
            for f in range(F):
                one = torch.empty(8 + 4 * nbytes[f], dtype=torch.uint8, device=dev)
                rc, n = ctx.hilbert_rle_approx_encode(d, src[offs[f]:], ws[f], hs[f], out=one)
                lens.append(n); streams.append(one[:n])
            stride = (max(lens) + 3) & ~3
            enc = torch.zeros(stride * F, dtype=torch.uint8, device=dev)
            for f in range(F):
                enc[f * stride:f * stride + lens[f]] = streams[f]
            del streams
            torch.cuda.synchronize()
            res = {}

            def decode():
                res["d"] = ctx.decode_batch("hilbert(rle)", enc, stride, lens, F, back, img_stride)
            if a.only == "rle-decode":   # (with --sweep: the batches of small frames, which take the batched route)
                decode()
                continue
            out[tag + "decode_batch " + name] = raw_times(decode, a.reps, a.warmup)
            assert res["d"][0] == 0
            if a.sweep:
                continue
            if d == 0.0 or hasattr(_lib.lib(), "cniic_codec_parse_f64"):   # (a build from before hilbert(rle(d)) was an expression measures the exact codec only)
                def measure():
                    res["m"] = ctx.measure_batch(name, src, offs, ws, hs)
                out["measure_batch " + name] = raw_times(measure, a.reps, a.warmup)
                assert res["m"][0] == 0 and [r["compressed_size"] for r in res["m"][1]] == lens
            ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
            decode()
            out["rle_dec_batch frames " + name] = ctx.kernel_time("rle_dec_batch")[1]
            ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
            del enc


def raw_times(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(round((time.perf_counter() - t) * 1e3, 3))
    return ts


def stats(ts):
    return dict(median_ms=round(statistics.median(ts), 3), min_ms=round(min(ts), 3), max_ms=round(max(ts), 3), runs=len(ts))


def hilbert_ab(a):
    """children in alternation: this library, the other, this, the other, ..."""
    import subprocess
    got = {"this": {}, "other": {}}
    libs = [("this", None)] + ([("other", a.against)] if a.against else [])
    for _ in range(a.rounds):
        for who, lib in libs:
            cmd = [sys.executable, os.path.abspath(__file__), "--hilbert-child", "--reps", str(a.reps), "--warmup", str(a.warmup)] + (["--sweep"] if a.sweep else [])
            if lib:
                cmd += ["--lib-file", lib]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                raise SystemExit("child failed (%s): %s" % (who, r.stderr[-2000:]))
            line = [l for l in r.stdout.split("\n") if l.startswith("HILBERT ")][-1]
            for k, v in json.loads(line[8:]).items():
                if isinstance(v, list):
                    got[who].setdefault(k, []).extend(v)
                else:
                    got[who][k] = v
    rows = []
    for k, v in got["this"].items():
        if not isinstance(v, list):
            rows.append(dict(case=k, this=v, other=got["other"].get(k)))
            continue
        row = dict(case=k, this=stats(v))
        if isinstance(got["other"].get(k), list):
            row["other"] = stats(got["other"][k])
            sp = (row["this"]["max_ms"] - row["this"]["min_ms"]) + (row["other"]["max_ms"] - row["other"]["min_ms"])
            row.update(ratio_other_over_this=round(row["other"]["median_ms"] / row["this"]["median_ms"], 3), spreads_ms=round(sp, 3),
                       faster_by_more_than_the_spreads=bool(row["this"]["median_ms"] + sp < row["other"]["median_ms"]))
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only", choices=("mse", "encode", "rle-decode"))
    ap.add_argument("--hilbert", action="store_true")
    ap.add_argument("--hilbert-child", action="store_true")
    ap.add_argument("--against")
    ap.add_argument("--lib-file")
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--sweep", action="store_true", help="--hilbert: batches of one frame size each (SWEEP) instead of the 100 images")
    a = ap.parse_args()
    if a.hilbert:
        return hilbert_ab(a)
    if a.hilbert_child or a.only == "rle-decode":
        return hilbert_times(a)
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
