"""Batches of SMALL `zip(dict)` frames through cniic_codec_encode_batch_var and cniic_codec_measure_batch: this build (the small-frame
route, k_zd_small.hip) against another build of the library and against this build with the route switched off, device buffers throughout.
    python tools/small_zip_probe.py --against libcniic_hip_parent.so [--out profiles/small_zip_probe.json] [--reps 5] [--rounds 1]
Batches of 1, 4, 8, 32, 256 and 4096 synthetic frames of 32 x 32, 64 x 64, 128 x 96, 128 x 128 and 16384 x 1: photo-like, uniform noise,
flat, and photo-like with a flat band of a sixteenth of the frame.  Every variant is timed in a child process of its own, the variants in
alternation (this, route off, other, this, ...), --rounds times --reps runs each after --warmup untimed ones; the medians are compared
with min - max beside them, and the digests of the streams and of the measured rows must agree.
  this        libcniic_hip_testing.so of this tree under CNIIC_TEST_ZD_SMALL_FLOOR_OFF=1: every candidate takes the route, which is what
              the floor is set from (--floor keeps the floor: what a caller gets)
  route_off   the same library under CNIIC_TEST_ZD_SMALL_OFF=1
  other       --against FILE: another build in cniic_amd/ (CNIIC_LIB_FILE), e.g. the parent commit's library -- the yardstick
A further child runs `this` with the stage timers on and records the duration of k_zd_small ("zd_small_batch"), of the placing copy
("zd_small_place"), the frames handed back to the workers ("zd_small_handback") and the walks the commit wave finished
("zd_small_finished").  --sizes / --frames / --kinds narrow the sweep; --max-px skips the cases of more pixels in all (the workers need
seconds for 4096 frames of 16 384 pixels).

--calls decode times cniic_codec_decode_batch of the streams the encode wrote (the small-frame decode route, k_zd_small_dec.hip): `this` runs
under CNIIC_TEST_ZD_SMALL_DEC_FLOOR_OFF=1 as well, `route_off` under CNIIC_TEST_ZD_SMALL_DEC_OFF=1, the stage child records
"zd_small_dec_batch" and "zd_small_dec_handback", and a digest of all decoded images must agree between the variants.  --host decodes from
and into host memory.  `clear` in a decode cell: this build's slowest run beats the other's fastest -- the ranges do not overlap -- which
is what the route's floor is set from (`lost`: the other way round)."""
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

SIZES = ((32, 32), (64, 64), (128, 96), (128, 128), (16384, 1))
FRAMES = (1, 4, 8, 32, 256, 4096)
KINDS = ("photo", "uniform", "flat", "band")
STAGES = ("zd_small_batch", "zd_small_place", "zd_small_handback", "zd_small_finished", "zd_small_dec_batch", "zd_small_dec_handback")
OFF, FLOOR_OFF = "CNIIC_TEST_ZD_SMALL_OFF", "CNIIC_TEST_ZD_SMALL_FLOOR_OFF"
DEC_OFF, DEC_FLOOR_OFF = "CNIIC_TEST_ZD_SMALL_DEC_OFF", "CNIIC_TEST_ZD_SMALL_DEC_FLOOR_OFF"
CALLS = ("encode", "measure", "decode")
EXPR = "zip(dict)"


def cases(a):
    sizes = [tuple(int(x) for x in s.split("x")) for s in a.sizes.split(",")] if a.sizes else SIZES
    frames = [int(x) for x in a.frames.split(",")] if a.frames else FRAMES
    kinds = a.kinds.split(",") if a.kinds else KINDS
    return [(w, h, F, kind) for kind in kinds for (w, h) in sizes for F in frames if not a.max_px or w * h * F <= a.max_px]


def child(a):
    import torch
    import cniic_amd
    from cniic_amd import _lib, synth
    dev = torch.device("cuda", 0)
    out = {}
    with cniic_amd.Context(0) as ctx:
        for w, h, F, kind in cases(a):
            n, nb = w * h, 3 * w * h
            src = torch.empty(nb * F + 16, dtype=torch.uint8, device=dev)
            if kind == "flat":
                src.view(-1)[:nb * F].view(-1, 3)[:] = torch.tensor([93, 41, 200], dtype=torch.uint8, device=dev)
            else:
                for f in range(F):
                    ctx.synth_image(_lib.SYNTH_UNIFORM if kind == "uniform" else _lib.SYNTH_PHOTO, synth.SEED0 + 9950 + (f % 512) * 7 + f // 512, w, h, src[f * nb:])
                if kind == "band":          # a sixteenth of every frame, from its middle on, in one colour
                    px = src[:nb * F].view(F, n, 3)
                    px[:, n // 2:n // 2 + max(n // 16, 1)] = torch.tensor([93, 41, 200], dtype=torch.uint8, device=dev)
            offs, ws, hs = [f * nb for f in range(F)], [w] * F, [h] * F
            stride = (2 * (8 + 11 * n) + 2 + 15) & ~15          # 4 bytes a pair (zd_small.hpp)
            enc = torch.zeros(stride * F, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            res = {}

            def encode():
                res["e"] = ctx.encode_batch_var(EXPR, src, offs, ws, hs, enc, stride)

            def measure():
                res["m"] = ctx.measure_batch(EXPR, src, offs, ws, hs)

            def decode():
                if "img" not in res:
                    lens = res["e"][1]
                    if a.host:
                        import numpy as np
                        res["img"], res["streams"] = np.zeros(nb * F + 16, np.uint8), enc.cpu().numpy()
                    else:
                        res["img"], res["streams"] = torch.zeros(nb * F + 16, dtype=torch.uint8, device=dev), enc
                    res["lens"] = lens
                res["d"] = ctx.decode_batch(EXPR, res["streams"], stride, res["lens"], F, res["img"], nb)
            calls = dict(encode=encode, measure=measure, decode=decode)
            name = "%s %dx%d x%d" % (kind, w, h, F)
            if a.stages:
                got = {}
                encode()
                decode()
                ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
                for call in (encode, decode):
                    call()
                    for s in STAGES:
                        ms, cnt = ctx.kernel_time(s)
                        if cnt or ms:
                            got[s] = dict(ms=round(ms, 3), launches=cnt)
                ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
                out[name] = got
                continue
            row = {}
            timed = a.calls.split(",") if a.calls else CALLS[:2]
            for which in CALLS:
                if which not in timed:
                    if which == "encode":
                        encode()
                    row[which] = []
                    continue
                for _ in range(a.warmup):
                    calls[which]()
                ts = []
                for _ in range(a.reps):
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    calls[which]()
                    torch.cuda.synchronize()
                    ts.append(round((time.perf_counter() - t) * 1e3, 3))
                row[which] = ts
            rc, lens, rcs, sts = res["e"]
            host = enc.cpu().numpy()
            dg = hashlib.sha256()
            for f in range(F):
                dg.update(bytes([rcs[f] & 255]))
                dg.update(host[f * stride:f * stride + (lens[f] if rcs[f] == 0 else 0)].tobytes())
                if "m" in res:
                    dg.update(repr((res["m"][1][f]["compressed_size"], res["m"][1][f]["error"])).encode())
            if "d" in res:
                img = res["img"] if a.host else res["img"].cpu().numpy()
                dg.update(img[:nb * F].tobytes())
                dg.update(repr(res["d"]).encode())
            out[name] = dict(ms=row, digest=dg.hexdigest()[:16], failed=sum(r != 0 for r in rcs), pairs=sum(lens) // 4)
            print("[probe child] %s" % name, file=sys.stderr, flush=True)
            del enc, src
    print("PROBE " + json.dumps(out), flush=True)


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
    ap.add_argument("--max-px", type=int, default=0, help="skip the cases of more pixels in all")
    ap.add_argument("--calls", help="the calls to time, of encode,measure,decode (default: encode,measure)")
    ap.add_argument("--host", action="store_true", help="decode from and into host memory")
    ap.add_argument("--variants", help="of this,route_off,other (this is always run)")
    ap.add_argument("--floor", action="store_true", help="`this` keeps the route's floor")
    ap.add_argument("--timeout", type=int, default=1100)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--stages", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    this_env = {"CNIIC_USE_TESTING_LIB": "1"} if a.floor else {"CNIIC_USE_TESTING_LIB": "1", FLOOR_OFF: "1", DEC_FLOOR_OFF: "1"}
    variants = [("this", this_env), ("route_off", {"CNIIC_USE_TESTING_LIB": "1", OFF: "1", DEC_OFF: "1"})]
    if a.against:
        variants.append(("other", {"CNIIC_LIB_FILE": a.against}))
    if a.variants:
        variants = [v for v in variants if v[0] == "this" or v[0] in a.variants.split(",")]
    base = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--warmup", str(a.warmup), "--max-px", str(a.max_px)]
    for k in ("sizes", "frames", "kinds", "calls"):
        if getattr(a, k):
            base += ["--" + k, getattr(a, k)]
    if a.host:
        base.append("--host")

    def run(env_add, extra=()):
        env = {k: v for k, v in os.environ.items() if k not in ("CNIIC_LIB_FILE", "CNIIC_USE_TESTING_LIB", OFF, FLOOR_OFF, DEC_OFF, DEC_FLOOR_OFF)}
        env.update(env_add)
        r = subprocess.run(base + list(extra), stdout=subprocess.PIPE, text=True, timeout=a.timeout, env=env)   # (a child's progress lines go to stderr as they come)
        if r.returncode != 0:
            raise SystemExit("child failed (%s), status %d" % (env_add, r.returncode))
        print("[probe] a child is done: %s %s" % (env_add, list(extra)), file=sys.stderr, flush=True)
        return json.loads([l for l in r.stdout.split("\n") if l.startswith("PROBE ")][-1][6:])

    got = {v: {} for v, _ in variants}
    for _ in range(a.rounds):
        for who, env in variants:
            for k, v in run(env).items():
                e = got[who].setdefault(k, dict(ms={c: [] for c in CALLS}, digest=v["digest"], failed=v["failed"], pairs=v["pairs"]))
                for c in CALLS:
                    e["ms"][c].extend(v["ms"][c])
                assert e["digest"] == v["digest"], (who, k)
    stages = run(variants[0][1], ("--stages",))

    # a row per case, on one line: per call the [median, min, max] ms of this build and of `other`, the median of route_off,
    # x = the other's median over this build's, slower / faster = this build's median exceeds / beats the other's by more than the two
    # min - max spreads together
    def tri(ts):
        return [round(statistics.median(ts), 3), round(min(ts), 3), round(max(ts), 3)] if ts else None
    rows = []
    for k, v in got["this"].items():
        row = dict(case=k, failed_frames=v["failed"], pairs=v["pairs"], stages={s: [t["ms"], t["launches"]] for s, t in (stages.get(k) or {}).items()})
        for c in CALLS:
            if not v["ms"][c]:
                continue
            cell = dict(this=tri(v["ms"][c]))
            if "route_off" in got:
                cell["route_off"] = tri(got["route_off"][k]["ms"][c])[0]
            if "other" in got:
                o = tri(got["other"][k]["ms"][c])
                sp = (cell["this"][2] - cell["this"][1]) + (o[2] - o[1])
                cell.update(other=o, x=round(o[0] / cell["this"][0], 3), slower=bool(o[0] + sp < cell["this"][0]), faster=bool(cell["this"][0] + sp < o[0]))
                if c == "decode":
                    cell.update(clear=bool(cell["this"][2] < o[1]), lost=bool(o[2] < cell["this"][1]))
            row[c] = cell
        row["same"] = all(got[who][k]["digest"] == v["digest"] for who in ("route_off", "other") if who in got)
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("[\n" + ",\n".join(" " + json.dumps(r) for r in rows) + "\n]\n")


if __name__ == "__main__":
    main()
