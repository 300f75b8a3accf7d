"""zip(dict) encode and decode on the GPU, per phase, against the single-core C restatement of the coder (tests/zip_dict_ref.c) on the
same images: photo-like, uniform noise, "band" (that noise with the first row and the last four in one colour: an entry of 16 KB,
so the chain carries the parse across matches above 255 bytes: the hybrid chain of k_zipdict.hip) and flat, --size x --size (4096),
device buffers.
    python tools/zip_probe.py [--size 4096] [--flat-size 4096] [--reps 3] [--out profiles/zip_probe.json]
The flat image never fills the dictionary and is coded on the host from end to end, a trie node per text byte: it is run once, with
the stage timers on.
Per image: the wall time of cniic_codec_encode / cniic_codec_decode (median of --reps runs after one warm-up, stage timers off), one more
run of each with the stage timers on -- host fill phase, table build, serialise, match, chain, compaction; host prefix, scan, copy --
and the restatement's encode and decode of the same text.  One JSON line per image; --out writes them to a file as well.

    python tools/zip_probe.py --against libcniic_hip_parent.so [--size 4096] [--reps 5] [--out profiles/zip_chain_probe.json]
The chain of the frozen parse against another build of the library in cniic_amd/ (the parent commit's: the yardstick), in child processes
that alternate between the two builds: band, a photo-like image with a flat run of 96 pixels in its first row (an entry of 352 bytes: the
smallest trigger -- a run of 24 pixels makes one of 88 and stays on the windowed route; it is measured too), the same with a flat first
row -- three images with an entry above 255 bytes -- and photo-like and noise, whose route does not change.  Per image and build: the
encode's wall time and the chain's stage time as median [min, max] of --reps runs, the stages of the hybrid chain, a digest of the
stream; per image: whether the digests agree and whether the ranges lie apart (`clear`) or overlap.
    python tools/zip_probe.py --bound [--out FILE]
The fall-back bound: texts with a match of 256 bytes in every piece, every 4th, 16th and 64th piece of 65 536, through the hybrid chain
and through the one-block walk (CNIIC_TEST_ZD_CHAIN=walk) of the testing library: the chain's stage time, median [min, max] of --reps."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
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


HYBRID_STAGES = ("zd_chain_hybrid", "zd_hy_breaks", "zd_hy_maps", "zd_hy_scan", "zd_hy_table", "zd_hy_walk", "zd_hy_patch", "zd_hy_marks")
HYBRID_COUNTS = ("zd_chain_breaks", "zd_chain_entered")


def mmm(ts):
    return [round(statistics.median(ts), 3), round(min(ts), 3), round(max(ts), 3)]


def chain_images(ctx, n):
    photo = torch.empty(n * n * 3, dtype=torch.uint8, device="cuda")
    noise = torch.empty(n * n * 3, dtype=torch.uint8, device="cuda")
    ctx.synth_image(_lib.SYNTH_PHOTO, 1, n, n, out=photo)
    ctx.synth_image(_lib.SYNTH_UNIFORM, 1, n, n, out=noise)
    colour = torch.tensor([93, 41, 200], dtype=torch.uint8, device="cuda")
    band = noise.clone().view(n, n * 3)
    band[:1] = colour.repeat(n)
    band[n - 4:] = colour.repeat(n)
    run = photo.clone()
    run[:24 * 3] = colour.repeat(24)
    run96 = photo.clone()
    run96[:96 * 3] = colour.repeat(96)
    row = photo.clone()
    row[:n * 3] = colour.repeat(n)
    return (("band", band.view(-1)), ("photo-like + run of 24", run), ("photo-like + run of 96", run96), ("photo-like + flat row", row), ("photo-like", photo),
            ("noise", noise))


def chain_child(a):
    """one build, every image: --reps encodes timed by the wall clock, --reps with the stage timers on"""
    with cniic_amd.Context(0) as ctx:
        n = a.size
        for name, img in chain_images(ctx, n):
            stream = torch.empty(2 * (8 + 11 * n * n) + 4, dtype=torch.uint8, device="cuda")
            ln = [0]

            def enc():
                rc, ln[0], _ = ctx.encode(EXPR, img, w=n, h=n, out=stream)
                assert rc == 0

            enc()
            walls, chains, st = [], [], {}
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t = time.perf_counter()
                enc()
                torch.cuda.synchronize()
                walls.append((time.perf_counter() - t) * 1e3)
            ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
            for _ in range(a.reps):
                enc()
                chains.append(ctx.kernel_time("zd_chain")[0] + ctx.kernel_time("zd_chain_plain")[0])
                st = {k: round(ctx.kernel_time(k)[0], 4) for k in ENC_STAGES + HYBRID_STAGES if ctx.kernel_time(k)[1]}
                st.update({k: ctx.kernel_time(k)[1] for k in HYBRID_COUNTS if ctx.kernel_time("zd_chain_hybrid")[1]})
            ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
            print(json.dumps(dict(image=name, size=n, encode_ms=walls, chain_ms=chains, stages=st, stream_bytes=ln[0],
                                  sha256=hashlib.sha256(stream[:ln[0]].cpu().numpy().tobytes()).hexdigest())), flush=True)


def run_child(extra, env_add, timeout):
    env = {k: v for k, v in os.environ.items() if k not in ("CNIIC_LIB_FILE", "CNIIC_USE_TESTING_LIB", "CNIIC_TEST_ZD_CHAIN", "CNIIC_TEST_ZD_CHAIN_MAX_BREAKS")}
    env.update(env_add)
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + extra, stdout=subprocess.PIPE, text=True, timeout=timeout, env=env)
    if r.returncode != 0:
        raise SystemExit("the child ended with status %d" % r.returncode)
    return [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]


def apart(mine, other):
    return "clear" if mine[2] < other[1] else "lost" if mine[1] > other[2] else "overlap"


def chain_against(a):
    got = {"this": {}, "other": {}}
    for rnd in range(a.rounds):
        for who, env in (("this", {}), ("other", {"CNIIC_LIB_FILE": a.against})):
            for row in run_child(["--chain-child", "--size", str(a.size), "--reps", str(a.reps)], env, a.timeout):
                cell = got[who].setdefault(row["image"], dict(encode_ms=[], chain_ms=[], stages=row["stages"], sha256=row["sha256"], stream_bytes=row["stream_bytes"]))
                cell["encode_ms"] += row["encode_ms"]
                cell["chain_ms"] += row["chain_ms"]
    rows = []
    for name, mine in got["this"].items():
        other = got["other"][name]
        row = dict(image=name, size=a.size, reps=a.reps * a.rounds, stream_bytes=mine["stream_bytes"], same_stream=mine["sha256"] == other["sha256"],
                   encode_ms=mmm(mine["encode_ms"]), other_encode_ms=mmm(other["encode_ms"]), chain_ms=mmm(mine["chain_ms"]), other_chain_ms=mmm(other["chain_ms"]),
                   stages_ms=mine["stages"], other_stages_ms=other["stages"])
        row["encode"] = apart(row["encode_ms"], row["other_encode_ms"])
        row["chain"] = apart(row["chain_ms"], row["other_chain_ms"])
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def bound_texts(pieces=65536):
    """a head that makes the entries 2 .. 256 of one byte, noise in which the dictionary fills, then `pieces` pieces of noise with a stretch
    of 256 of that byte (behind a byte that occurs nowhere else) in every `every`-th piece"""
    rng = np.random.default_rng(1)
    alphabet = np.array([b for b in range(256) if b not in (7, 200)], np.uint8)
    head = np.concatenate([np.full(510, 7, np.uint8), alphabet[rng.integers(0, alphabet.size, 600000)]])
    for every in (1, 4, 16, 64):
        tail = alphabet[rng.integers(0, alphabet.size, pieces * 256)]
        if every == 1:       # a stretch and its stop byte every 257 bytes: a start in (almost) every piece
            at = np.arange(1, tail.size - 257, 257)
        else:
            at = np.arange(1, tail.size - 257, 256 * every)
        tail[at - 1] = 200
        for k in range(256):
            tail[at + k] = 7
        yield every, np.concatenate([head, tail])


def bound_probe(a):
    os.environ["CNIIC_USE_TESTING_LIB"] = "1"
    rows = []
    with cniic_amd.Context(0) as ctx:
        for every, text in bound_texts():
            t = torch.from_numpy(text).cuda()
            out = torch.empty(2 * text.size + 4, dtype=torch.uint8, device="cuda")
            row = dict(text="a match of 256 bytes every %d pieces" % every, bytes=int(text.size))
            digests = []
            ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
            for mode in ("hybrid", "walk"):
                if mode == "walk":
                    os.environ["CNIIC_TEST_ZD_CHAIN"] = "walk"
                ts = []
                for k in range(a.reps + 1):
                    rc, ln = ctx.zip_dict_encode(t, out=out)
                    assert rc == 0
                    if k:
                        ts.append(ctx.kernel_time("zd_chain_plain")[0])
                if mode == "hybrid":
                    assert ctx.kernel_time("zd_chain_hybrid")[1] == 1
                    row.update(breaks=ctx.kernel_time("zd_chain_breaks")[1], entered=ctx.kernel_time("zd_chain_entered")[1],
                               stages_ms={k: round(ctx.kernel_time(k)[0], 4) for k in HYBRID_STAGES if ctx.kernel_time(k)[1]})
                else:
                    assert ctx.kernel_time("zd_chain_hybrid")[1] == 0
                    del os.environ["CNIIC_TEST_ZD_CHAIN"]
                row[mode + "_chain_ms"] = mmm(ts)
                digests.append(hashlib.sha256(out[:ln].cpu().numpy().tobytes()).hexdigest())
            ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
            row["same_stream"] = digests[0] == digests[1]
            row["hybrid"] = apart(row["hybrid_chain_ms"], row["walk_chain_ms"])
            print(json.dumps(row), flush=True)
            rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--flat-size", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--against", help="another build of the library in cniic_amd/ (its file name)")
    ap.add_argument("--bound", action="store_true")
    ap.add_argument("--chain-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.reps is None:
        a.reps = 5 if a.against or a.bound or a.chain_child else 3
    if a.chain_child:
        return chain_child(a)
    if a.against or a.bound:
        rows = chain_against(a) if a.against else bound_probe(a)
        if a.out:
            with open(a.out, "w") as f:
                for r in rows:
                    f.write(json.dumps(r) + "\n")
        return
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
