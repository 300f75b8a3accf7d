"""Batches of SMALL `hufman` frames through cniic_codec_encode_batch_var, cniic_codec_decode_batch (of `hufman` streams and of
cluster-colors(256) streams, which are Hufman streams of palette colours) and cniic_codec_measure_batch: this build (the small-frame
routes, k_huf_small in k_delta_small.hip and k_huf_small_dec in k_delta_small_dec.hip) against another build of the library and against
this build with the routes switched off, device buffers throughout.
    python tools/small_hufman_probe.py --against libcniic_hip_parent.so [--out profiles/small_hufman_parse_probe.json] [--reps 5] [--rounds 1]
Batches of 1, 8, 256 and 4096 synthetic frames of 32 x 32, 64 x 64, 128 x 96, 128 x 128 and 16384 x 1, photo-like and uniform noise.
Every variant is timed in a child process of its own, the variants in alternation (this, routes off, other, this, ...), --rounds times
--reps runs each after --warmup untimed ones; the medians are compared with min - max beside them, and the digests of the streams and of
the decoded images must agree.  --variants narrows the variants, --calls the timed calls (the encodes still run once: the decodes need
their streams).
  this        libcniic_hip_testing.so of this tree
  route_off   the same library under CNIIC_TEST_HUF_SMALL_OFF=1 and CNIIC_TEST_HUF_SMALL_DEC_OFF=1
  parse_off   the same library under CNIIC_TEST_HUF_SMALL_DEC_PARSE_OFF=1: the decoders of device streams parsed on the host, as before
              k_small_trieparse_rgb
  other       --against FILE: another build in cniic_amd/ (CNIIC_LIB_FILE), e.g. the parent commit's library -- the yardstick
A fourth child runs `this` with the stage timers on and records the durations of k_huf_small ("huf_small_batch"), the placing copy
("huf_small_place"), k_huf_small_dec ("huf_small_dec_batch", of the `hufman` streams and of the cluster-colors ones) and, beside it,
k_small_trieparse_rgb ("huf_small_dec_parse": the launches' time and the frames parsed; "huf_small_dec_parse_host": the candidates handed
back).  --sizes / --frames / --kinds narrow the sweep."""
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
FRAMES = (1, 8, 256, 4096)
KINDS = ("photo", "uniform")
STAGES = ("huf_small_batch", "huf_small_place", "huf_small_dec_batch", "huf_small_dec_parse", "huf_small_dec_parse_host")
OFF = ("CNIIC_TEST_HUF_SMALL_OFF", "CNIIC_TEST_HUF_SMALL_DEC_OFF")
PARSE_OFF = "CNIIC_TEST_HUF_SMALL_DEC_PARSE_OFF"
CALLS = ("encode", "decode", "decode_cc", "measure")
CC = "cluster-colors(256)"


def cases(a):
    sizes = [tuple(int(x) for x in s.split("x")) for s in a.sizes.split(",")] if a.sizes else SIZES
    frames = [int(x) for x in a.frames.split(",")] if a.frames else FRAMES
    kinds = a.kinds.split(",") if a.kinds else KINDS
    return [(w, h, F, kind) for kind in kinds for (w, h) in sizes for F in frames]


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
            for f in range(F):
                ctx.synth_image(_lib.SYNTH_PHOTO if kind == "photo" else _lib.SYNTH_UNIFORM, synth.SEED0 + 9800 + (f % 512) * 7 + f // 512, w, h, src[f * nb:])
            offs, ws, hs = [f * nb for f in range(F)], [w] * F, [h] * F
            stride = (8 + 13 * n - 1 + (19 * n + 7) // 8 + 15) & ~15          # no stream of n pixels is longer (huf_small.hpp)
            cc_stride = (8 + 13 * 256 - 1 + 2 * n + 15) & ~15                   # 256 leaves; a Huffman code of 256 symbols averages below 9 bits
            enc = torch.zeros(stride * F, dtype=torch.uint8, device=dev)
            cc_enc = torch.zeros(cc_stride * F, dtype=torch.uint8, device=dev)
            back = torch.zeros(nb * F + 16, dtype=torch.uint8, device=dev)
            cc_back = torch.zeros(nb * F + 16, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            res = {}
            res["c"] = ctx.encode_batch_var(CC, src, offs, ws, hs, cc_enc, cc_stride, allow=(_lib.TOO_FEW_POINTS, _lib.FEW_ACTIVE))
            cc_lens = [l if r == 0 else 0 for l, r in zip(res["c"][1], res["c"][2])]

            def encode():
                res["e"] = ctx.encode_batch_var("hufman", src, offs, ws, hs, enc, stride)

            def decode():
                res["d"] = ctx.decode_batch("hufman", enc, stride, res["e"][1], F, back, nb)

            def decode_cc():
                res["dc"] = ctx.decode_batch(CC, cc_enc, cc_stride, cc_lens, F, cc_back, nb, allow=(_lib.DECODE,))

            def measure():
                res["m"] = ctx.measure_batch("hufman", src, offs, ws, hs)
            calls = dict(encode=encode, decode=decode, decode_cc=decode_cc, measure=measure)
            name = "%s %dx%d x%d" % (kind, w, h, F)
            if a.stages:
                got = {}
                for which in ("encode", "decode", "decode_cc"):
                    calls[which]()
                    ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
                    calls[which]()
                    for s in STAGES:
                        ms, cnt = ctx.kernel_time(s)
                        if cnt or ms:
                            got[s + ("_cc" if which == "decode_cc" else "")] = dict(ms=round(ms, 3), launches=cnt)
                    ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
                out[name] = got
                continue
            row = {}
            timed = a.calls.split(",") if a.calls else CALLS
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
            host, img, cc_img = enc.cpu().numpy(), back.cpu().numpy(), cc_back.cpu().numpy()
            dg = hashlib.sha256()
            for f in range(F):
                dg.update(bytes([rcs[f] & 255] + [res[c][3][f] & 255 for c in ("d", "dc") if c in res]))
                dg.update(host[f * stride:f * stride + (lens[f] if rcs[f] == 0 else 0)].tobytes())
                dg.update(img[f * nb:(f + 1) * nb].tobytes())
                if cc_lens[f]:
                    dg.update(cc_img[f * nb:(f + 1) * nb].tobytes())
                if "m" in res:
                    dg.update(repr((res["m"][1][f]["compressed_size"], res["m"][1][f]["error"])).encode())
            out[name] = dict(ms=row, digest=dg.hexdigest()[:16], failed=sum(r != 0 for r in rcs), cc_streams=sum(1 for l in cc_lens if l))
            print("[probe child] %s" % name, file=sys.stderr, flush=True)
            del src, enc, back, cc_enc, cc_back
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
    ap.add_argument("--calls", help="the calls to time, of encode,decode,decode_cc,measure")
    ap.add_argument("--variants", help="of this,route_off,parse_off,other (this is always run)")
    ap.add_argument("--timeout", type=int, default=1100)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--stages", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    variants = [("this", {"CNIIC_USE_TESTING_LIB": "1"}), ("route_off", dict({"CNIIC_USE_TESTING_LIB": "1"}, **{k: "1" for k in OFF})),
                ("parse_off", {"CNIIC_USE_TESTING_LIB": "1", PARSE_OFF: "1"})]
    if a.against:
        variants.append(("other", {"CNIIC_LIB_FILE": a.against}))
    if a.variants:
        variants = [v for v in variants if v[0] == "this" or v[0] in a.variants.split(",")]
    base = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--warmup", str(a.warmup)]
    for k in ("sizes", "frames", "kinds", "calls"):
        if getattr(a, k):
            base += ["--" + k, getattr(a, k)]

    def run(env_add, extra=()):
        env = {k: v for k, v in os.environ.items() if k not in ("CNIIC_LIB_FILE", "CNIIC_USE_TESTING_LIB", PARSE_OFF) + OFF}
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
                e = got[who].setdefault(k, dict(ms={c: [] for c in CALLS}, digest=v["digest"], failed=v["failed"], cc_streams=v["cc_streams"]))
                for c in CALLS:
                    e["ms"][c].extend(v["ms"][c])
                assert e["digest"] == v["digest"], (who, k)
    stages = run(variants[0][1], ("--stages",))

    # a row per case, on one line: per call the [median, min, max] ms of this build and of `other`, the medians of route_off and parse_off,
    # x = the other's median over this build's, slower / faster = this build's median exceeds / beats the other's by more than the two
    # min - max spreads together
    def tri(ts):
        return [round(statistics.median(ts), 3), round(min(ts), 3), round(max(ts), 3)] if ts else None
    rows = []
    for k, v in got["this"].items():
        row = dict(case=k, failed_frames=v["failed"], cc_streams=v["cc_streams"], stages={s: [t["ms"], t["launches"]] for s, t in (stages.get(k) or {}).items()})
        for c in CALLS:
            if not v["ms"][c]:
                continue
            cell = dict(this=tri(v["ms"][c]))
            for who in ("route_off", "parse_off"):
                if who in got:
                    cell[who] = tri(got[who][k]["ms"][c])[0]
            if "other" in got:
                o = tri(got["other"][k]["ms"][c])
                sp = (cell["this"][2] - cell["this"][1]) + (o[2] - o[1])
                cell.update(other=o, x=round(o[0] / cell["this"][0], 3), slower=bool(o[0] + sp < cell["this"][0]), faster=bool(cell["this"][0] + sp < o[0]))
            row[c] = cell
        row["same"] = all(got[who][k]["digest"] == v["digest"] for who in ("route_off", "parse_off", "other") if who in got)
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("[\n" + ",\n".join(" " + json.dumps(r) for r in rows) + "\n]\n")


if __name__ == "__main__":
    main()
