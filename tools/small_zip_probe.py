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
is what the route's floor is set from (`lost`: the other way round).

--codec hilbert-zip probes Hilbert { compress: Zip } instead: cniic_hilbert_zip_encode_batch_var, cniic_hilbert_zip_measure_batch and
cniic_hilbert_zip_decode_batch (k_hz_small, k_hz_small_dec) under the CNIIC_TEST_HZ_SMALL_* knobs, the stages "hz_small_*".  A library that
has no such calls -- the parent commit's, which is the yardstick -- runs the loop of cniic_hilbert_zip_encode / cniic_hilbert_zip_decode
(and cniic_mse for measure) over the same device buffers on one context, which is all it can do.  Every cell carries `clear` / `lost` against that yardstick, and
`route_off_range` with `clear_of_route_off` / `lost_to_route_off` against this build's own workers, which is what the floors are set from."""
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
HZ_STAGES = ("hz_small_batch", "hz_small_place", "hz_small_handback", "hz_small_finished", "hz_small_dec_batch", "hz_small_dec_handback")
HZ_OFF, HZ_FLOOR_OFF = "CNIIC_TEST_HZ_SMALL_OFF", "CNIIC_TEST_HZ_SMALL_FLOOR_OFF"
HZ_DEC_OFF, HZ_DEC_FLOOR_OFF = "CNIIC_TEST_HZ_SMALL_DEC_OFF", "CNIIC_TEST_HZ_SMALL_DEC_FLOOR_OFF"


def cases(a):
    sizes = [tuple(int(x) for x in s.split("x")) for s in a.sizes.split(",")] if a.sizes else SIZES
    frames = [int(x) for x in a.frames.split(",")] if a.frames else FRAMES
    kinds = a.kinds.split(",") if a.kinds else KINDS
    return [(w, h, F, kind) for kind in kinds for (w, h) in sizes for F in frames if not a.max_px or w * h * F <= a.max_px]


def hz_calls(ctx, src, offs, ws, hs, enc, stride, res, host, dev):
    """encode / measure / decode of Hilbert { compress: Zip }: the batch calls where the library has them, else the loop of single calls"""
    import ctypes as C
    import numpy as np
    import torch
    L, F = ctx._L, len(offs)
    batched = hasattr(L, "cniic_hilbert_zip_encode_batch_var")
    nb = 3 * ws[0] * hs[0]
    p_src, p_enc = src.data_ptr(), enc.data_ptr()
    L.cniic_hilbert_zip_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]
    L.cniic_hilbert_zip_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]

    def encode_loop(dst, dst_stride):
        lens, rcs, ln = [], [], C.c_uint64(0)
        for f in range(F):
            rcs.append(L.cniic_hilbert_zip_encode(ctx.h, p_src + offs[f], ws[f], hs[f], dst + f * dst_stride, dst_stride, C.byref(ln)))
            lens.append(ln.value)
        return next((r for r in rcs if r), 0), lens, rcs, None

    def decode_loop(streams, lens, img, img_stride):
        cw, ch, rcs = C.c_uint32(0), C.c_uint32(0), []
        for f in range(F):
            rcs.append(L.cniic_hilbert_zip_decode(ctx.h, streams + f * stride, lens[f], img + f * img_stride, img_stride, C.byref(cw), C.byref(ch)))
        return next((r for r in rcs if r), 0), list(ws), list(hs), rcs

    def encode():
        res["e"] = ctx.hilbert_zip_encode_batch_var(src, offs, ws, hs, enc, stride) + (None,) if batched else encode_loop(p_enc, stride)

    def measure():
        if batched:
            res["m"] = ctx.hilbert_zip_measure_batch(src, offs, ws, hs)
            return
        if "mbuf" not in res:
            res["mbuf"] = (torch.zeros(stride * F, dtype=torch.uint8, device=dev), torch.zeros(nb * F + 16, dtype=torch.uint8, device=dev))
        sbuf, ibuf = res["mbuf"]
        rc, lens, rcs, _ = encode_loop(sbuf.data_ptr(), stride)
        decode_loop(sbuf.data_ptr(), lens, ibuf.data_ptr(), nb)
        rows = []
        for f in range(F):
            rows.append(dict(compressed_size=lens[f], error=ctx.mse(src[offs[f]:offs[f] + nb], ibuf[f * nb:(f + 1) * nb])))
        res["m"] = (rc, rows, lens)

    def decode():
        if "img" not in res:
            if host:
                res["img"], res["streams"] = np.zeros(nb * F + 16, np.uint8), enc.cpu().numpy()
            else:
                res["img"], res["streams"] = torch.zeros(nb * F + 16, dtype=torch.uint8, device=dev), enc
            res["lens"] = res["e"][1]
        if batched:
            res["d"] = ctx.hilbert_zip_decode_batch(res["streams"], stride, res["lens"], F, res["img"], nb)
        else:
            at = lambda x: x.ctypes.data if host else x.data_ptr()
            res["d"] = decode_loop(at(res["streams"]), res["lens"], at(res["img"]), nb)
    return dict(encode=encode, measure=measure, decode=decode)


def child(a):
    import torch
    import cniic_amd
    from cniic_amd import _lib, synth
    dev = torch.device("cuda", 0)
    out = {}
    hz = a.codec == "hilbert-zip"
    stage_names = HZ_STAGES if hz else STAGES
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
            calls = hz_calls(ctx, src, offs, ws, hs, enc, stride, res, a.host, dev) if hz else dict(encode=encode, measure=measure, decode=decode)
            encode, decode = calls["encode"], calls["decode"]
            name = "%s %dx%d x%d" % (kind, w, h, F)
            if a.stages:
                got = {}
                encode()
                decode()
                ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
                for call in (encode, decode):
                    call()
                    for s in stage_names:
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
            rc, lens, rcs = res["e"][:3]
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
    ap.add_argument("--codec", default="zip-dict", choices=("zip-dict", "hilbert-zip"), help="zip-dict: the expression zip(dict); hilbert-zip: Hilbert { compress: Zip }'s own calls")
    ap.add_argument("--variants", help="of this,route_off,other (this is always run)")
    ap.add_argument("--floor", action="store_true", help="`this` keeps the route's floor")
    ap.add_argument("--timeout", type=int, default=1100)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--stages", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    hz = a.codec == "hilbert-zip"
    off, floor_off, dec_off, dec_floor_off = (HZ_OFF, HZ_FLOOR_OFF, HZ_DEC_OFF, HZ_DEC_FLOOR_OFF) if hz else (OFF, FLOOR_OFF, DEC_OFF, DEC_FLOOR_OFF)
    this_env = {"CNIIC_USE_TESTING_LIB": "1"} if a.floor else {"CNIIC_USE_TESTING_LIB": "1", floor_off: "1", dec_floor_off: "1"}
    variants = [("this", this_env), ("route_off", {"CNIIC_USE_TESTING_LIB": "1", off: "1", dec_off: "1"})]
    if a.against:
        variants.append(("other", {"CNIIC_LIB_FILE": a.against}))
    if a.variants:
        variants = [v for v in variants if v[0] == "this" or v[0] in a.variants.split(",")]
    base = [sys.executable, os.path.abspath(__file__), "--child", "--codec", a.codec, "--reps", str(a.reps), "--warmup", str(a.warmup), "--max-px", str(a.max_px)]
    for k in ("sizes", "frames", "kinds", "calls"):
        if getattr(a, k):
            base += ["--" + k, getattr(a, k)]
    if a.host:
        base.append("--host")

    def run(env_add, extra=()):
        env = {k: v for k, v in os.environ.items() if k not in ("CNIIC_LIB_FILE", "CNIIC_USE_TESTING_LIB", OFF, FLOOR_OFF, DEC_OFF, DEC_FLOOR_OFF, HZ_OFF, HZ_FLOOR_OFF, HZ_DEC_OFF, HZ_DEC_FLOOR_OFF)}
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
                ro = tri(got["route_off"][k]["ms"][c])
                cell["route_off"] = ro[0]
                if hz:   # the floor of this codec is set against the workers of this build: the ranges, and whether they lie apart
                    cell.update(route_off_range=ro[1:], clear_of_route_off=bool(cell["this"][2] < ro[1]), lost_to_route_off=bool(ro[2] < cell["this"][1]))
            if "other" in got:
                o = tri(got["other"][k]["ms"][c])
                sp = (cell["this"][2] - cell["this"][1]) + (o[2] - o[1])
                cell.update(other=o, x=round(o[0] / cell["this"][0], 3), slower=bool(o[0] + sp < cell["this"][0]), faster=bool(cell["this"][0] + sp < o[0]))
                if c == "decode" or hz:
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
