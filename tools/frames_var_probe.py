"""cniic_cc_finish_frames_var (frames of different sizes, ONE palette) on the release library, device buffers throughout; one warm-up,
then medians of --reps runs with min - max.  Every run opens its own session (the shared K-means, untimed) and times the finishing call.
  (a) equal frames   128 frames of 1920 x 1080, K = 256: finish_frames_var against finish_frames, in alternation; the same bytes
  (b) the folder     the 100 synthetic images of DIV2K's sizes of tools/batch_var_probe.py under one palette: the finishing call, the
                     whole encode (session + K-means + finish), the call's stages with the stage timers on -- and, for scale, the same
                     build's cniic_codec_encode_batch_var of cluster-colors(256), which builds one palette PER IMAGE
    python tools/frames_var_probe.py [--out profiles/frames_var_probe.json] [--reps 5] [--only a|b]
  --c4 --against OTHER.so [--rounds 3]   the equal-size path itself, which shares device bodies with the new one: the `c4_one_gpu` block of
                     `bench.py --gpus 1 --full --cpu-sample 0` of this build and of another build of the library in cniic_amd/ (the parent
                     commit's), child processes in alternation; the row is added to --out beside (a) and (b)"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import cniic_amd
from batch_var_probe import div2k_like_sizes
from cniic_amd import _lib, synth
from cniic_amd.dist import ShardedClusterColors

STAGES = ("frames_var_labels", "frames_var_align", "frames_var_hist", "frames_var_trees", "frames_var_pack")


def stats(ts):
    return dict(median_ms=round(statistics.median(ts), 3), min_ms=round(min(ts), 3), max_ms=round(max(ts), 3), runs=len(ts))


def finish_time(scc, frames, npx, finish):
    """one session over `frames`, the finishing call alone timed -> (ms, what it returned)"""
    handle, _ = scc._cluster(frames, npx)
    try:
        torch.cuda.synchronize()
        t = time.perf_counter()
        res = finish(handle)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, res
    finally:
        scc.be.destroy(handle)


def find_key(obj, key):
    if isinstance(obj, dict):
        if key in obj:
            return obj[key]
        for v in obj.values():
            r = find_key(v, key)
            if r is not None:
                return r
    return None


def c4_against(a):
    """bench.py --full children, the other library first: the c4_one_gpu block's ms per step of each run"""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    runs = {"other": [], "this": []}
    for _ in range(a.rounds):
        for who in ("other", "this"):
            env = dict(os.environ)
            env.pop("CNIIC_LIB_FILE", None)
            if who == "other":
                env["CNIIC_LIB_FILE"] = a.against
            r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--full", "--cpu-sample", "0", "--steps", "5", "--warmup", "2"],
                               capture_output=True, text=True, timeout=a.child_timeout, env=env, cwd=root)
            lines = [l for l in r.stdout.split("\n") if l.startswith("{")]
            if r.returncode != 0 or not lines:
                raise SystemExit("bench.py failed (%s, exit %d): %s" % (who, r.returncode, (r.stderr or r.stdout)[-2000:]))
            blk = find_key(json.loads(lines[-1]), "c4_one_gpu")
            if not blk:
                raise SystemExit("bench.py --full gave no c4_one_gpu block (%s): %s" % (who, lines[-1][:1000]))
            runs[who].append(dict(ms_per_step=blk["ms_per_step"], mpixels_per_s=blk["value"], parity=(blk.get("parity") or {}).get("matches_oracle")))
            print(json.dumps({who: runs[who][-1]}), flush=True)
    st = {who: stats([x["ms_per_step"] for x in runs[who]]) for who in runs}
    row = dict(case="c4_one_gpu block of bench.py --full: this build against " + a.against, runs=runs, this=st["this"], other=st["other"],
               this_median_inside_other_min_max=bool(st["other"]["min_ms"] <= st["this"]["median_ms"] <= st["other"]["max_ms"]),
               this_median_not_above_other_max=bool(st["this"]["median_ms"] <= st["other"]["max_ms"]))
    print(json.dumps(row), flush=True)
    if a.out:
        rows = json.load(open(a.out)) if os.path.exists(a.out) else []
        rows = [r for r in rows if not r.get("case", "").startswith("c4_one_gpu")] + [row]
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=("a", "b"))
    ap.add_argument("--c4", action="store_true")
    ap.add_argument("--against")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child-timeout", type=int, default=170)
    a = ap.parse_args()
    if a.c4:
        return c4_against(a)
    assert os.environ.get("CNIIC_USE_TESTING_LIB") != "1", "the probe measures the release library"
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(device=dev))
    K = 256
    rows = []

    def emit(**row):
        print(json.dumps(row), flush=True)
        rows.append(row)

    with cniic_amd.Context(0, stream=torch.cuda.current_stream().cuda_stream) as ctx:
        scc = ShardedClusterColors(ctx, K, None, dev)
        if a.only != "b":
            F, w, h = 128, 1920, 1080
            fr = torch.empty((F, h, w, 3), dtype=torch.uint8, device=dev)
            for f in range(F):
                ctx.synth_image(_lib.SYNTH_PHOTO, synth.SEED0 + 4 + f, w, h, fr[f])
            stride = w * h
            out_v = torch.zeros(stride * F, dtype=torch.uint8, device=dev)
            out_e = torch.zeros(stride * F, dtype=torch.uint8, device=dev)
            flat, npx = fr.reshape(-1), F * w * h
            var = lambda hd: scc.be.finish_frames_var(hd, flat, [w] * F, [h] * F, out_v, stride)
            eq = lambda hd: scc.be.finish_frames(hd, fr, w, h, F, out_e, stride)
            t_v, t_e, res = [], [], {}
            for i in range(a.reps + 1):   # (the first pair is the warm-up)
                tv, res["v"] = finish_time(scc, flat, npx, var)
                te, res["e"] = finish_time(scc, flat, npx, eq)
                if i:
                    t_v.append(tv); t_e.append(te)
            sv, se = stats(t_v), stats(t_e)
            emit(case="(a) finish_frames_var vs finish_frames, equal frames", frames=F, w=w, h=h, K=K, var=sv, equal=se,
                 same=bool(list(res["v"][0]) == list(res["e"][0]) and torch.equal(out_v, out_e)),
                 var_median_inside_equal_min_max=bool(se["min_ms"] <= sv["median_ms"] <= se["max_ms"]), var_runs_ms=[round(t, 3) for t in t_v],
                 equal_runs_ms=[round(t, 3) for t in t_e])
            del fr, flat, out_v, out_e
        if a.only != "a":
            sizes = div2k_like_sizes()
            F = len(sizes)
            ws, hs = [w for w, _ in sizes], [h for _, h in sizes]
            nbytes = [3 * w * h for w, h in sizes]
            offs = [sum(nbytes[:f]) for f in range(F)]
            npx = sum(nbytes) // 3
            src = torch.empty(sum(nbytes) + 16, dtype=torch.uint8, device=dev)
            for f, (w, h) in enumerate(sizes):
                ctx.synth_image(_lib.SYNTH_PHOTO, synth.SEED0 + 6000 + f, w, h, src[offs[f]:])
            flat = src[:sum(nbytes)]
            stride = (max(nbytes) // 3 * 2 + (1 << 16) + 3) & ~3
            out = torch.zeros(stride * F, dtype=torch.uint8, device=dev)
            var = lambda hd: scc.be.finish_frames_var(hd, flat, ws, hs, out, stride)
            t_f, t_w, res = [], [], {}
            for i in range(a.reps + 1):
                tf, res["f"] = finish_time(scc, flat, npx, var)
                torch.cuda.synchronize()
                t = time.perf_counter()
                res["w"] = scc.encode_frames_var(flat, ws, hs, out, stride)
                torch.cuda.synchronize()
                if i:
                    t_f.append(tf); t_w.append((time.perf_counter() - t) * 1e3)
            lens = res["f"][0]
            rc, ws_b, hs_b, rcs = ctx.decode_batch("cluster-colors(%d)" % K, out, stride, lens, F, torch.empty(max(nbytes) * F, dtype=torch.uint8, device=dev), max(nbytes))
            # the stages, once, with the stage timers on (they synchronise: not part of the timings above)
            ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
            before = {s: ctx.kernel_time(s) for s in STAGES}
            finish_time(scc, flat, npx, var)
            stages = {s: dict(ms=round(ctx.kernel_time(s)[0] - before[s][0], 3), launches=ctx.kernel_time(s)[1] - before[s][1]) for s in STAGES}
            ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
            # for scale: one palette PER IMAGE (the reference's semantics) by the batched encode of the same build
            enc = torch.zeros(stride * F, dtype=torch.uint8, device=dev)
            t_b = []
            for i in range(a.reps + 1):
                torch.cuda.synchronize()
                t = time.perf_counter()
                rb = ctx.encode_batch_var("cluster-colors(%d)" % K, src, offs, ws, hs, enc, stride)
                torch.cuda.synchronize()
                if i:
                    t_b.append((time.perf_counter() - t) * 1e3)
            sf, sw = stats(t_f), stats(t_w)
            emit(case="(b) 100 images of DIV2K's sizes, one palette", frames=F, mpix=round(npx / 1e6, 1), K=K, finish_frames_var=sf, whole_encode=sw,
                 gpixels_per_s_whole=round(npx / (sw["median_ms"] * 1e-3) / 1e9, 2), stages=stages, kmeans_iterations=res["f"][1]["iterations"],
                 bytes_per_px=round(sum(lens) / npx, 4), decodes=bool(rc == 0 and ws_b == ws and hs_b == hs and not any(rcs)),
                 encode_batch_var_one_palette_per_image=stats(t_b), encode_batch_var_ok=bool(rb[0] == 0))
        scc.close()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
