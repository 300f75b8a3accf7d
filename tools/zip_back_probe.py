"""zip(back) on the GPU -- one workgroup per stream -- against the single-core C restatement of the coder (tests/zip_back_ref.c), and the
batched calls against a loop of the single ones.
    python tools/zip_back_probe.py [--size 1024] [--scale 8] [--frames 100] [--reps 3] [--slices 65536,262144,1048576]
                                   [--out profiles/zip_back_probe.json]
Per image (photo-like and uniform noise, --size x --size, device buffers): the wall time of cniic_zip_back_image_encode / _decode
(median of --reps runs after a warm-up, stage timers off), one more run of each with the stage timers on, the restatement's encode and
decode of the same text, and the encode again with a launch's slice set to each of --slices (CNIIC_TEST_ZB_SLICE, testing build).
Then the folder: the --frames first of tools/batch_var_probe.py's 100 DIV2K-like sizes, each side divided by --scale (at full size a
loop of single encodes takes tens of minutes), encoded and decoded by the batched calls and by a loop of the single calls.
One JSON line per measurement; --out writes them to a file as well.

    python tools/zip_back_probe.py --against libcniic_hip_parent.so [--sizes 256,512,1024,2048] [--batches 8,32,100] [--scale 8]
                                   [--rounds 5] [--slices ...] [--out profiles/zip_back_probe.json]
measures the decode of this build -- the whole-GPU route (k_zipback_par.hip) taking every stream, CNIIC_TEST_ZB_PAR_MIN=0 -- against
another build in cniic_amd/ (CNIIC_LIB_FILE: the parent commit's library, the yardstick) and against this build with the route off
(CNIIC_TEST_ZB_PAR_OFF=1).  One child process encodes everything once with the GPU encoder (the first encode numbers: wall time at each
of --slices for the largest of --sizes that is at most 1024) and leaves the streams in a temporary file; then the three builds run in
alternating child processes, --rounds times, each timing every cell once after a warm-up.  Cells: cniic_zip_back_image_decode of a
photo-like and a noise image of each of --sizes; cniic_zip_back_image_decode_batch of the first 8 / 32 / 100 DIV2K-like sizes divided
by --scale; cniic_zip_back_image_measure_batch of the first 32 against the loop of the three single calls (all a build without the call
can do).  A cell reports [median, min, max] per build, `clear` (this build's slowest run beats the other's fastest) and `lost`, the
jump rounds and hand-backs of the route, and `same`: a digest of everything decoded agrees across the three."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

os.environ.setdefault("CNIIC_USE_TESTING_LIB", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

import cniic_amd
import zip_back_ref as Z
from batch_var_probe import div2k_like_sizes
from cniic_amd import _lib

ENC_STAGES = ("zb_serialize", "zb_encode")
DEC_STAGES = ("zb_decode", "zb_rebuild")
SLICE = "CNIIC_TEST_ZB_SLICE"


def wall(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return round(statistics.median(ts), 3)


def stages(ctx, fn, names):
    ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
    try:
        fn()
        return {k: dict(ms=round(ctx.kernel_time(k)[0], 3), launches=ctx.kernel_time(k)[1]) for k in names}
    finally:
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)


def single(ctx, clib, name, kind, n, reps, slices):
    img = torch.empty(n * n * 3, dtype=torch.uint8, device="cuda")
    ctx.synth_image(kind, 1, n, n, out=img)
    text_len = 8 + 11 * n * n
    stream = torch.empty(text_len + text_len // 4 + 16, dtype=torch.uint8, device="cuda")
    back = torch.empty(n * n * 3, dtype=torch.uint8, device="cuda")
    ln = [0]

    def enc():
        rc, ln[0] = ctx.zip_back_image_encode(img, w=n, h=n, out=stream)

    def dec():
        assert ctx.zip_back_image_decode_into(stream, ln[0], back) == (0, n, n)

    row = dict(what="single", image=name, size=n, text_bytes=text_len, encode_ms=wall(enc, reps), encode_stages=stages(ctx, enc, ENC_STAGES))
    row.update(stream_bytes=ln[0], decode_ms=wall(dec, reps), decode_stages=stages(ctx, dec, DEC_STAGES), lossless=bool(torch.equal(back, img)))
    text = np.frombuffer(Z.zip_text(img.cpu().numpy().reshape(n, n, 3)), np.uint8)
    info = {}
    t = time.perf_counter()
    ref = Z.encode_c(clib, text, info)
    row["c_encode_ms"] = round((time.perf_counter() - t) * 1e3, 1)
    t = time.perf_counter()
    out = Z.decode_c(clib, ref, cap=text_len)
    row["c_decode_ms"] = round((time.perf_counter() - t) * 1e3, 1)
    row.update(same_stream=stream[:ln[0]].cpu().numpy().tobytes() == ref and out == text.tobytes(), probes=info["probes"], longest=info["longest"])
    row["encode_ms_by_slice"] = {}
    for s in slices:
        os.environ[SLICE] = str(s)
        try:
            row["encode_ms_by_slice"][str(s)] = wall(enc, reps)
        finally:
            del os.environ[SLICE]
    return row


def folder(ctx, frames, scale, reps):
    sizes = [(max(w // scale, 1), max(h // scale, 1)) for w, h in div2k_like_sizes()[:frames]]
    F = len(sizes)
    ws, hs = [w for w, _ in sizes], [h for _, h in sizes]
    offs = np.concatenate([[0], np.cumsum([3 * w * h for w, h in sizes])]).astype(np.int64)
    imgs = torch.empty(int(offs[-1]), dtype=torch.uint8, device="cuda")
    for f, (w, h) in enumerate(sizes):
        ctx.synth_image(_lib.SYNTH_PHOTO, 100 + f, w, h, out=imgs[int(offs[f]):int(offs[f + 1])])
    stride = max(14 * w * h + 32 for w, h in sizes)
    img_stride = max(3 * w * h for w, h in sizes)
    out = torch.empty(stride * F, dtype=torch.uint8, device="cuda")
    out1 = torch.empty(stride * F, dtype=torch.uint8, device="cuda")
    px = torch.empty(img_stride * F, dtype=torch.uint8, device="cuda")
    lens = [[0] * F, [0] * F]

    def enc_batch():
        rc, lens[0], rcs = ctx.zip_back_encode_batch_var(imgs, offs[:-1], ws, hs, out, stride)

    def enc_loop():
        for f in range(F):
            rc, lens[1][f] = ctx.zip_back_image_encode(imgs[int(offs[f]):], w=ws[f], h=hs[f], out=out1[f * stride:(f + 1) * stride])

    def dec_batch():
        ctx.zip_back_decode_batch(out, stride, lens[0], F, px, img_stride)

    def dec_loop():
        for f in range(F):
            ctx.zip_back_image_decode_into(out[f * stride:], lens[0][f], px[f * img_stride:(f + 1) * img_stride])

    row = dict(what="folder", frames=F, scale=scale, megapixels=round(sum(w * h for w, h in sizes) / 1e6, 3))
    row.update(encode_batch_ms=wall(enc_batch, reps), encode_loop_ms=wall(enc_loop, reps))
    row["same_streams"] = lens[0] == lens[1] and all(torch.equal(out[f * stride:f * stride + lens[0][f]], out1[f * stride:f * stride + lens[0][f]]) for f in range(F))
    row.update(decode_batch_ms=wall(dec_batch, reps), decode_loop_ms=wall(dec_loop, reps))
    row["lossless"] = all(torch.equal(px[f * img_stride:f * img_stride + 3 * ws[f] * hs[f]], imgs[int(offs[f]):int(offs[f + 1])]) for f in range(F))
    return row


PAR_MIN, PAR_OFF = "CNIIC_TEST_ZB_PAR_MIN", "CNIIC_TEST_ZB_PAR_OFF"
KINDS = (("photo-like", _lib.SYNTH_PHOTO), ("noise", _lib.SYNTH_UNIFORM))


def once(fn):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return round((time.perf_counter() - t) * 1e3, 3)


def folder_sizes(frames, scale):
    return [(max(w // scale, 1), max(h // scale, 1)) for w, h in div2k_like_sizes()[:frames]]


def folder_images(ctx, sizes):
    offs = np.concatenate([[0], np.cumsum([3 * w * h for w, h in sizes])]).astype(np.int64)
    imgs = torch.empty(int(offs[-1]), dtype=torch.uint8, device="cuda")
    for f, (w, h) in enumerate(sizes):
        ctx.synth_image(_lib.SYNTH_PHOTO, 100 + f, w, h, out=imgs[int(offs[f]):int(offs[f + 1])])
    return imgs, offs


def prepare(a):
    """every stream of the run from the GPU encoder, into a.streams; the encode's times on stdout"""
    sizes = [int(x) for x in a.sizes.split(",")]
    store, rows = {}, []
    with cniic_amd.Context(0) as ctx:
        for name, kind in KINDS:
            for n in sizes:
                img = torch.empty(n * n * 3, dtype=torch.uint8, device="cuda")
                ctx.synth_image(kind, 1, n, n, out=img)
                out = torch.empty(14 * n * n + 32, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                t = time.perf_counter()
                rc, ln = ctx.zip_back_image_encode(img, w=n, h=n, out=out)
                torch.cuda.synchronize()
                rows.append(dict(what="encode", image=name, size=n, text_bytes=8 + 11 * n * n, stream_bytes=ln, encode_ms=round((time.perf_counter() - t) * 1e3, 1)))
                store["single/%s/%d" % (name, n)] = out[:ln].cpu().numpy()
                if n == max(x for x in sizes if x <= 1024):
                    rows[-1]["encode_ms_by_slice"] = {}
                    for sl in [int(x) for x in a.slices.split(",") if x]:
                        os.environ[SLICE] = str(sl)
                        try:
                            rows[-1]["encode_ms_by_slice"][str(sl)] = wall(lambda: ctx.zip_back_image_encode(img, w=n, h=n, out=out), 1)
                        finally:
                            del os.environ[SLICE]
        fsizes = folder_sizes(max(int(x) for x in a.batches.split(",")), a.scale)
        imgs, offs = folder_images(ctx, fsizes)
        stride = max(14 * w * h + 32 for w, h in fsizes)
        out = torch.empty(stride * len(fsizes), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        t = time.perf_counter()
        rc, lens, rcs = ctx.zip_back_encode_batch_var(imgs, offs[:-1], [w for w, _ in fsizes], [h for _, h in fsizes], out, stride)
        torch.cuda.synchronize()
        rows.append(dict(what="encode_batch", frames=len(fsizes), scale=a.scale, megapixels=round(sum(w * h for w, h in fsizes) / 1e6, 3),
                         encode_ms=round((time.perf_counter() - t) * 1e3, 1)))
        host = out.cpu().numpy()
        for f, ln in enumerate(lens):
            store["folder/%d" % f] = host[f * stride:f * stride + ln].copy()
    np.savez(a.streams, **store)
    print(json.dumps(rows))


def child(a):
    """every cell once on the build the environment names -> {cell: dict(ms, digest, rounds, handed)}"""
    sizes = [int(x) for x in a.sizes.split(",")]
    store = np.load(a.streams)
    cells = {}
    with cniic_amd.Context(0) as ctx:
        def marks(fn):
            ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
            try:
                fn()
                return dict(rounds=ctx.kernel_time("zb_par_rounds")[1], routed=ctx.kernel_time("zb_par_decode")[1], handed=ctx.kernel_time("zb_par_handback")[1],
                            serial_launches=ctx.kernel_time("zb_decode")[1])
            finally:
                ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)

        for name, kind in KINDS:
            for n in ([] if a.loop else sizes):      # (the loop's child times the measure cell only)
                stream = torch.from_numpy(store["single/%s/%d" % (name, n)]).cuda()
                back = torch.empty(n * n * 3, dtype=torch.uint8, device="cuda")
                fn = lambda: ctx.zip_back_image_decode_into(stream, stream.numel(), back)
                cells["single/%s/%d" % (name, n)] = dict(ms=once(fn), digest=hashlib.sha256(back.cpu().numpy().tobytes()).hexdigest()[:16], stream_bytes=stream.numel(), **marks(fn))
        for F in ([] if a.loop else [int(x) for x in a.batches.split(",")]):
            fsizes = folder_sizes(F, a.scale)
            lens = [len(store["folder/%d" % f]) for f in range(F)]
            stride, img_stride = max(lens), max(3 * w * h for w, h in fsizes)
            blob = np.zeros(stride * F, np.uint8)
            for f in range(F):
                blob[f * stride:f * stride + lens[f]] = store["folder/%d" % f]
            src = torch.from_numpy(blob).cuda()
            px = torch.zeros(img_stride * F, dtype=torch.uint8, device="cuda")
            fn = lambda: ctx.zip_back_decode_batch(src, stride, lens, F, px, img_stride)
            cells["batch/%d" % F] = dict(ms=once(fn), digest=hashlib.sha256(px.cpu().numpy().tobytes()).hexdigest()[:16], stream_bytes=[min(lens), max(lens)], **marks(fn))
        # the folder in one call against the loop of the three single calls
        F = min(32, max(int(x) for x in a.batches.split(",")))
        fsizes = folder_sizes(F, a.scale)
        imgs, offs = folder_images(ctx, fsizes)
        ws, hs = [w for w, _ in fsizes], [h for _, h in fsizes]
        got = []
        if hasattr(ctx._L, "cniic_zip_back_image_measure_batch") and not a.loop:
            def fn():
                rc, rows, lens = ctx.zip_back_measure_batch(imgs, offs[:-1], ws, hs)
                got[:] = [(r["compressed_size"], r["error"]) for r in rows]
        else:
            out = torch.empty(max(14 * w * h + 32 for w, h in fsizes), dtype=torch.uint8, device="cuda")
            px = torch.empty(max(3 * w * h for w, h in fsizes), dtype=torch.uint8, device="cuda")

            def fn():
                got[:] = []
                for f in range(F):
                    img = imgs[int(offs[f]):int(offs[f + 1])]
                    rc, ln = ctx.zip_back_image_encode(img, w=ws[f], h=hs[f], out=out)
                    ctx.zip_back_image_decode_into(out, ln, px[:img.numel()])
                    got.append((ln, ctx.mse(img, px[:img.numel()])))
        cells["measure/%d" % F] = dict(ms=once(fn), digest=hashlib.sha256(repr(got).encode()).hexdigest()[:16])
    print(json.dumps(cells))


def against(a):
    me = [sys.executable, os.path.abspath(__file__), "--sizes", a.sizes, "--batches", a.batches, "--scale", str(a.scale), "--slices", a.slices]
    tmp = tempfile.mkdtemp()
    streams = os.path.join(tmp, "streams.npz")
    clean = {k: v for k, v in os.environ.items() if k not in ("CNIIC_LIB_FILE", "CNIIC_USE_TESTING_LIB", PAR_MIN, PAR_OFF, SLICE)}
    r = subprocess.run(me + ["--prepare", "--streams", streams], stdout=subprocess.PIPE, text=True, timeout=a.timeout, env=dict(clean, CNIIC_USE_TESTING_LIB="1"), check=True)
    rows = json.loads(r.stdout.strip().split("\n")[-1])
    for row in rows:
        print(json.dumps(row), flush=True)
    variants = [("this", {"CNIIC_USE_TESTING_LIB": "1", PAR_MIN: "0"}, []), ("route_off", {"CNIIC_USE_TESTING_LIB": "1", PAR_OFF: "1"}, []),
                ("other", {"CNIIC_LIB_FILE": a.against}, []), ("this_loop", {"CNIIC_USE_TESTING_LIB": "1", PAR_OFF: "1"}, ["--loop"])]
    got = {}
    for rnd in range(a.rounds):
        for who, env, extra in variants:
            r = subprocess.run(me + ["--child", "--streams", streams] + extra, stdout=subprocess.PIPE, text=True, timeout=a.timeout, env=dict(clean, **env), check=True)
            for k, v in json.loads(r.stdout.strip().split("\n")[-1]).items():
                e = got.setdefault(k, {}).setdefault(who, dict(ms=[], digest=v["digest"], info={x: y for x, y in v.items() if x not in ("ms", "digest")}))
                e["ms"].append(v["ms"])
                assert e["digest"] == v["digest"], (who, k)
        report(a, rows, got, rnd + 1)


def report(a, head, got, rounds):
    """the cells after `rounds` rounds, printed and (--out) written: a run that is cut short leaves the rounds it finished"""
    rows = list(head)
    for k in sorted(got, key=lambda c: (c.split("/")[0], c.split("/")[1] if len(c.split("/")) == 3 else "", int(c.split("/")[-1]))):
        cell = dict(what=k, rounds_measured=rounds)
        for who, e in got[k].items():
            cell[who] = [round(statistics.median(e["ms"]), 3), min(e["ms"]), max(e["ms"])]
        cell.update(got[k]["this"]["info"])
        cell.update(clear=bool(cell["this"][2] < cell["other"][1]), lost=bool(cell["other"][2] < cell["this"][1]),
                    clear_of_route_off=bool(cell["this"][2] < cell["route_off"][1]), lost_to_route_off=bool(cell["route_off"][2] < cell["this"][1]),
                    same=len({e["digest"] for e in got[k].values()}) == 1)
        rows.append(cell)
        if rounds == a.rounds:
            print(json.dumps(cell), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--against", help="another build of the library in cniic_amd/ (its file name)")
    ap.add_argument("--sizes", default="256,512,1024,2048")
    ap.add_argument("--batches", default="8,32,100")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=1100)
    ap.add_argument("--prepare", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--loop", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--streams", help=argparse.SUPPRESS)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--scale", type=int, default=8)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--slices", default="65536,262144,1048576")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.prepare or a.child or a.against:
        return (prepare if a.prepare else child if a.child else against)(a)
    clib = Z.compile_c(tempfile.mkdtemp())
    rows = []
    with cniic_amd.Context(0) as ctx:
        for name, kind in (("photo-like", _lib.SYNTH_PHOTO), ("noise", _lib.SYNTH_UNIFORM)):
            rows.append(single(ctx, clib, name, kind, a.size, a.reps, [int(s) for s in a.slices.split(",") if s]))
            print(json.dumps(rows[-1]), flush=True)
        if a.frames:
            rows.append(folder(ctx, a.frames, a.scale, a.reps))
            print(json.dumps(rows[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
