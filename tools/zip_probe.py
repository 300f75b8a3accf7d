"""zip(dict) encode and decode on the GPU, per phase, against the single-core C restatement of the coder (tests/zip_dict_ref.c) on the
same images: photo-like, uniform noise, "band" (that noise with the first row and the last four in one colour: an entry of 16 KB,
so the chain takes its plain route over the whole frozen phase) and flat, --size x --size (4096), device buffers.
    python tools/zip_probe.py [--size 4096] [--flat-size 4096] [--reps 3] [--out profiles/zip_probe.json]
The flat image never fills the dictionary and is coded on the host from end to end, a trie node per text byte: it is run once, with
the stage timers on.
Per image: the wall time of cniic_codec_encode / cniic_codec_decode (median of --reps runs after one warm-up, stage timers off), one more
run of each with the stage timers on -- host fill phase, table build, serialise, match, chain, compaction; host prefix, scan, copy --
and the restatement's encode and decode of the same text.  One JSON line per image; --out writes them to a file as well."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import cniic_amd
import zip_dict_ref as Z
from cniic_amd import _lib

EXPR = "zip(dict)"
ENC_STAGES = ("zd_serialize", "zd_fill_host", "zd_table_host", "zd_match", "zd_chain", "zd_chain_plain", "zd_compact")
DEC_STAGES = ("zd_prefix_host", "zd_scan", "zd_copy")


def images(ctx, n, nf):
    photo = torch.empty(n * n * 3, dtype=torch.uint8, device="cuda")
    noise = torch.empty(n * n * 3, dtype=torch.uint8, device="cuda")
    ctx.synth_image(_lib.SYNTH_PHOTO, 1, n, n, out=photo)
    ctx.synth_image(_lib.SYNTH_UNIFORM, 1, n, n, out=noise)
    flat = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(np.array((93, 41, 200), np.uint8), (nf * nf, 3))).reshape(-1)).cuda()
    band = noise.clone().view(n, n * 3)
    row = torch.tensor([93, 41, 200] * n, dtype=torch.uint8, device="cuda")
    band[:1] = row
    band[n - 4:] = row
    return (("photo-like", photo, n), ("noise", noise, n), ("band", band.view(-1), n), ("flat", flat, nf))


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
        return {k: round(ctx.kernel_time(k)[0], 3) for k in names if ctx.kernel_time(k)[1] or ctx.kernel_time(k)[0]}
    finally:
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--flat-size", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    clib = Z.compile_c(tempfile.mkdtemp())
    rows = []
    with cniic_amd.Context(0) as ctx:
        for name, img, n in images(ctx, a.size, a.flat_size):
            text_len = 8 + 11 * n * n
            stream = torch.empty(2 * text_len + 4, dtype=torch.uint8, device="cuda")
            back = torch.empty(n * n * 3, dtype=torch.uint8, device="cuda")
            ln = [0]

            def enc():
                rc, ln[0], _ = ctx.encode(EXPR, img, w=n, h=n, out=stream)

            def dec():
                rc, w, h = ctx.decode_into(EXPR, stream, ln[0], back)
                assert (rc, w, h) == (0, n, n)

            row = dict(image=name, size=n, text_bytes=text_len)
            if name == "flat":     # (never leaves the host's fill phase, seconds a run: once, the stage timers on)
                t = time.perf_counter()
                row["encode_stages_ms"] = stages(ctx, enc, ENC_STAGES)
                row["encode_ms"] = round((time.perf_counter() - t) * 1e3, 3)
            else:
                row["encode_ms"] = wall(enc, a.reps)
                row["encode_stages_ms"] = stages(ctx, enc, ENC_STAGES)
            row["stream_bytes"] = ln[0]
            reps = 1 if name == "flat" else a.reps
            row["decode_ms"] = wall(dec, reps)
            row["decode_stages_ms"] = stages(ctx, dec, DEC_STAGES)
            row["lossless"] = bool(torch.equal(back, img))
            if clib is not None:
                host = img.cpu().numpy().reshape(n, n, 3)
                text = np.frombuffer(Z.zip_text(host), np.uint8)
                info = {}
                t = time.perf_counter()
                ref = Z.encode_c(clib, text, info)
                row["c_encode_ms"] = round((time.perf_counter() - t) * 1e3, 1)
                t = time.perf_counter()
                out = Z.decode_c(clib, ref, cap=text_len)
                row["c_decode_ms"] = round((time.perf_counter() - t) * 1e3, 1)
                row["same_stream"] = stream[:ln[0]].cpu().numpy().tobytes() == ref and out == text.tobytes()
                row["fill_end"] = info["fill_end"]
                row["longest_entry"] = info["longest"]
                row["trie_nodes"] = info["nodes"]
            print(json.dumps(row), flush=True)
            rows.append(row)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
