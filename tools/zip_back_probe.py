"""zip(back) on the GPU -- one workgroup per stream -- against the single-core C restatement of the coder (tests/zip_back_ref.c), and the
batched calls against a loop of the single ones.
    python tools/zip_back_probe.py [--size 1024] [--scale 8] [--frames 100] [--reps 3] [--slices 65536,262144,1048576]
                                   [--out profiles/zip_back_probe.json]
Per image (photo-like and uniform noise, --size x --size, device buffers): the wall time of cniic_zip_back_image_encode / _decode
(median of --reps runs after a warm-up, stage timers off), one more run of each with the stage timers on, the restatement's encode and
decode of the same text, and the encode again with a launch's slice set to each of --slices (CNIIC_TEST_ZB_SLICE, testing build).
Then the folder: the --frames first of tools/batch_var_probe.py's 100 DIV2K-like sizes, each side divided by --scale (at full size a
loop of single encodes takes tens of minutes), encoded and decoded by the batched calls and by a loop of the single calls.
One JSON line per measurement; --out writes them to a file as well."""
import argparse
import json
import os
import statistics
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--scale", type=int, default=8)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--slices", default="65536,262144,1048576")
    ap.add_argument("--out")
    a = ap.parse_args()
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
