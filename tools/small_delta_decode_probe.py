"""Batches of SMALL `delta` frames through cniic_codec_decode_batch and cniic_codec_measure_batch: this build (the small-frame decode
route, k_delta_small_dec.hip, its decoders parsed on the GPU by k_small_trie.hip) against another build of the library, against this
build with the host's parse of the decoders and against this build with the route switched off, device buffers throughout.
    python tools/small_delta_decode_probe.py --against libcniic_hip_parent.so [--out profiles/small_delta_decode_probe.json] [--reps 5] [--rounds 1]
Batches of 256 and 4096 synthetic frames of 32 x 32, 64 x 64, 128 x 96 and 128 x 128, photo-like and uniform noise (noise: nearly every
symbol a leaf and codes of nearly one length, which settle slowest).  Every variant is timed in a child process of its own, the variants
in alternation (this, parse off, route off, other, this, ...), --rounds times --reps runs each after --warmup untimed ones; the medians are compared
with min - max beside them, and the digests of the decoded images (and of the measure rows) must agree.
  this        libcniic_hip_testing.so of this tree
  parse_off   the same library under CNIIC_TEST_DELTA_SMALL_DEC_PARSE_OFF=1: the decoders parsed on the host
  route_off   the same library under CNIIC_TEST_DELTA_SMALL_DEC_OFF=1: every frame's decode on a worker context
  other       --against FILE: another build in cniic_amd/ (CNIIC_LIB_FILE), e.g. the parent commit's library
A further child runs `this` with the stage timers on and records the duration of k_delta_small_dec ("delta_small_dec_batch") and of
k_small_trieparse ("delta_small_dec_parse", with the frames it parsed and, under "delta_small_dec_parse_host", those it handed back) of
both calls.  --sizes / --frames / --kinds / --calls narrow the sweep, --variants the builds."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = ((32, 32), (64, 64), (128, 96), (128, 128))
FRAMES = (256, 4096)
KINDS = ("photo", "uniform")
CALLS = ("decode_batch", "measure_batch")
STAGE = "delta_small_dec_batch"
PARSE_STAGE, PARSE_HOST_STAGE = "delta_small_dec_parse", "delta_small_dec_parse_host"
OFF = "CNIIC_TEST_DELTA_SMALL_DEC_OFF"
PARSE_OFF = "CNIIC_TEST_DELTA_SMALL_DEC_PARSE_OFF"


def cases(a):
    sizes = [tuple(int(x) for x in s.split("x")) for s in a.sizes.split(",")] if a.sizes else SIZES
    frames = [int(x) for x in a.frames.split(",")] if a.frames else FRAMES
    kinds = a.kinds.split(",") if a.kinds else KINDS
    calls = a.calls.split(",") if a.calls else CALLS
    return [(w, h, F, kind, call) for kind in kinds for (w, h) in sizes for F in frames for call in calls]


def child(a):
    import torch
    import cniic_amd
    from cniic_amd import _lib, synth
    dev = torch.device("cuda", 0)
    out = {}
    with cniic_amd.Context(0) as ctx:
        made = {}
        for w, h, F, kind, which in cases(a):
            nb = 3 * w * h
            if made.get("key") != (w, h, F, kind):
                made.clear()
                src = torch.empty(nb * F + 16, dtype=torch.uint8, device=dev)
                for f in range(F):
                    ctx.synth_image(_lib.SYNTH_PHOTO if kind == "photo" else _lib.SYNTH_UNIFORM, synth.SEED0 + 9700 + (f % 512) * 7 + f // 512, w, h, src[f * nb:])
                offs, ws, hs = [f * nb for f in range(F)], [w] * F, [h] * F
                stride = (8 + 8 * w * h + (19 * w * h + 7) // 8 + 3) & ~3     # no stream is longer (delta_small.hpp ds_stride)
                enc = torch.zeros(stride * F, dtype=torch.uint8, device=dev)
                img = torch.zeros(nb * F + 16, dtype=torch.uint8, device=dev)
                torch.cuda.synchronize()
                rc, lens, rcs, _ = ctx.encode_batch_var("delta", src, offs, ws, hs, enc, stride)
                assert rc == 0
                made.update(key=(w, h, F, kind), src=src, enc=enc, img=img, lens=lens)
            res = {}

            def call():
                if which == "decode_batch":
                    res["r"] = ctx.decode_batch("delta", enc, stride, lens, F, img, nb)
                else:
                    res["r"] = ctx.measure_batch("delta", src, offs, ws, hs)
            name = "%s %s %dx%d x%d" % (which, kind, w, h, F)
            if a.stages:
                call()
                ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
                call()
                out[name] = dict(ms=round(ctx.kernel_time(STAGE)[0], 3), launches=ctx.kernel_time(STAGE)[1], parse_ms=round(ctx.kernel_time(PARSE_STAGE)[0], 3),
                                 parsed=ctx.kernel_time(PARSE_STAGE)[1], handed_back=ctx.kernel_time(PARSE_HOST_STAGE)[1])
                ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
                continue
            img.zero_()
            for _ in range(a.warmup):
                call()
            ts = []
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t = time.perf_counter()
                call()
                torch.cuda.synchronize()
                ts.append(round((time.perf_counter() - t) * 1e3, 3))
            dg = hashlib.sha256()
            if which == "decode_batch":
                rc, dw, dh, rcs = res["r"]
                dg.update(repr((rc, dw, dh, rcs)).encode())
                dg.update(img[:nb * F].cpu().numpy().tobytes())
                failed = sum(r != 0 for r in rcs)
            else:
                rc, rows, mlens = res["r"]
                dg.update(repr((rc, [(r["compressed_size"], r["error"], r["rc"], r["lossless_mismatch"]) for r in rows])).encode())
                failed = sum(r["rc"] != 0 or r["error"] != 0.0 for r in rows)
            out[name] = dict(ms=ts, digest=dg.hexdigest()[:16], failed=failed)
    print("PROBE " + json.dumps(out), flush=True)


def stats(ts):
    return dict(median_ms=round(statistics.median(ts), 3), min_ms=round(min(ts), 3), max_ms=round(max(ts), 3), runs=len(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--against", help="another build of the library in cniic_amd/ (its file name)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--sizes")
    ap.add_argument("--frames")
    ap.add_argument("--kinds")
    ap.add_argument("--calls")
    ap.add_argument("--variants", help="of this,parse_off,route_off,other (this is always run)")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--stages", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    variants = [("this", {"CNIIC_USE_TESTING_LIB": "1"}), ("parse_off", {"CNIIC_USE_TESTING_LIB": "1", PARSE_OFF: "1"}),
                ("route_off", {"CNIIC_USE_TESTING_LIB": "1", OFF: "1"})]
    if a.against:
        variants.append(("other", {"CNIIC_LIB_FILE": a.against}))
    if a.variants:
        variants = [v for v in variants if v[0] == "this" or v[0] in a.variants.split(",")]
    base = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--warmup", str(a.warmup)]
    for k in ("sizes", "frames", "kinds", "calls"):
        if getattr(a, k):
            base += ["--" + k, getattr(a, k)]

    def run(env_add, extra=()):
        env = {k: v for k, v in os.environ.items() if k not in ("CNIIC_LIB_FILE", "CNIIC_USE_TESTING_LIB", OFF, PARSE_OFF)}
        env.update(env_add)
        r = subprocess.run(base + list(extra), capture_output=True, text=True, timeout=1100, env=env)
        if r.returncode != 0:
            raise SystemExit("child failed (%s): %s" % (env_add, r.stderr[-2000:]))
        return json.loads([l for l in r.stdout.split("\n") if l.startswith("PROBE ")][-1][6:])

    got = {v: {} for v, _ in variants}
    for _ in range(a.rounds):
        for who, env in variants:
            t0 = time.perf_counter()
            one = run(env)
            print("# %s: %d cases in %.0f s" % (who, len(one), time.perf_counter() - t0), file=sys.stderr, flush=True)
            for k, v in one.items():
                e = got[who].setdefault(k, dict(ms=[], digest=v["digest"], failed=v["failed"]))
                e["ms"].extend(v["ms"])
                assert e["digest"] == v["digest"], (who, k)
    stages = run(variants[0][1], ("--stages",))
    rows = []
    for k, v in got["this"].items():
        row = dict(case=k, failed_frames=v["failed"], this=stats(v["ms"]), kernel=stages.get(k))
        for who in ("parse_off", "route_off", "other"):
            if who not in got:
                continue
            o = got[who][k]
            row[who] = stats(o["ms"])
            sp = (row["this"]["max_ms"] - row["this"]["min_ms"]) + (row[who]["max_ms"] - row[who]["min_ms"])
            row[who].update(same_images=bool(o["digest"] == v["digest"]), ratio_over_this=round(row[who]["median_ms"] / row["this"]["median_ms"], 3),
                            spreads_ms=round(sp, 3), this_faster_by_more_than_the_spreads=bool(row["this"]["median_ms"] + sp < row[who]["median_ms"]))
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
