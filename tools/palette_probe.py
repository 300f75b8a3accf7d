"""Frozen palettes (cniic_palette_*) on the release library, device buffers throughout; one warm-up, then medians of --reps runs with
min - max.
  (a) create   cniic_palette_create for K = 16, 256 and 2048 (entries drawn from a photograph's pixels): the whole call, and with the stage
               timers on the table kernel alone (pal_lut) and the cells that took the plain route; for K = 256 beside the kernel's floor, a
               16 MiB fill of the same buffer size
  (b) encode   the 100 synthetic images of DIV2K's sizes of tools/batch_var_probe.py, K = 256: every run opens a session (the shared K-means,
               untimed), takes its palette out (cniic_cc_palette), times the session's own finishing call (cniic_cc_finish_frames_var) and then
               Palette.encode_frames_var of a handle made of those centroids on the same frames -- the same tail with the label stage swapped
               for the gather; the stages of both, once, with the stage timers on
    python tools/palette_probe.py [--out profiles/palette_probe.json] [--reps 5] [--only a|b]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import cniic_amd
from batch_var_probe import div2k_like_sizes
from cniic_amd import _lib, synth
from cniic_amd.dist import ShardedClusterColors

STAGES_SESSION = ("frames_var_labels", "frames_var_align", "frames_var_hist", "frames_var_trees", "frames_var_pack")
STAGES_PALETTE = ("pal_labels", "frames_var_align", "frames_var_hist", "frames_var_trees", "frames_var_pack")


def stats(ts):
    return dict(median_ms=round(statistics.median(ts), 3), min_ms=round(min(ts), 3), max_ms=round(max(ts), 3), runs=len(ts))


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=("a", "b"))
    a = ap.parse_args()
    assert os.environ.get("CNIIC_USE_TESTING_LIB") != "1", "the probe measures the release library"
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(device=dev))
    rows = []

    def emit(**row):
        print(json.dumps(row), flush=True)
        rows.append(row)

    with cniic_amd.Context(0, stream=torch.cuda.current_stream().cuda_stream) as ctx:
        if a.only != "b":
            px = synth.photo(640, 480, synth.SEED0 + 77).reshape(-1, 3)
            fill = torch.empty(1 << 24, dtype=torch.uint8, device=dev)
            t_fill = []
            for i in range(a.reps + 1):
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record(); fill.fill_(i & 255); ev1.record()
                torch.cuda.synchronize()
                if i:
                    t_fill.append(ev0.elapsed_time(ev1))
            for K in (16, 256, 2048):
                cent = px[np.random.default_rng(K).choice(px.shape[0], K, replace=False)].copy()
                ts = []
                for i in range(a.reps + 1):
                    t, p = wall(lambda: cniic_amd.Palette.create(ctx, cent))
                    p.close()
                    if i:
                        ts.append(t)
                ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
                ks = []
                for i in range(a.reps + 1):
                    p = cniic_amd.Palette.create(ctx, cent)
                    k_ms, plain = ctx.kernel_time("pal_lut")[0], ctx.kernel_time("pal_lut_plain")[1]
                    p.close()
                    if i:
                        ks.append(k_ms)
                ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
                emit(case="(a) cniic_palette_create", K=K, label_bytes=1 if K <= 256 else 2, create=stats(ts), pal_lut_kernel=stats(ks), plain_cells=int(plain),
                     fill_16MiB_floor=stats(t_fill))
        if a.only != "a":
            K = 256
            scc = ShardedClusterColors(ctx, K, None, dev)
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
            out_s = torch.zeros(stride * F, dtype=torch.uint8, device=dev)
            out_p = torch.zeros(stride * F, dtype=torch.uint8, device=dev)
            t_s, t_p, t_c = [], [], []
            for i in range(a.reps + 2):   # (the first is the warm-up; the last runs with the stage timers on and is not timed)
                staged = i == a.reps + 1
                if staged:
                    ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
                handle, _ = scc._cluster(flat, npx)
                try:
                    cent, pixels = scc.be.palette(handle, K)
                    ts, (lens_s, st) = wall(lambda: scc.be.finish_frames_var(handle, flat, ws, hs, out_s, stride))
                    if staged:
                        stages_s = {s: dict(ms=round(ctx.kernel_time(s)[0], 3), launches=ctx.kernel_time(s)[1]) for s in STAGES_SESSION}
                finally:
                    scc.be.destroy(handle)
                tc, pal = wall(lambda: cniic_amd.Palette.create(ctx, cent))
                try:
                    tp, lens_p = wall(lambda: pal.encode_frames_var(flat, ws, hs, out_p, stride))
                    if staged:
                        stages_p = {s: dict(ms=round(ctx.kernel_time(s)[0], 3), launches=ctx.kernel_time(s)[1]) for s in STAGES_PALETTE}
                finally:
                    pal.close()
                if 0 < i <= a.reps:
                    t_s.append(ts); t_p.append(tp); t_c.append(tc)
            ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
            dec = torch.empty(max(nbytes) * F, dtype=torch.uint8, device=dev)
            rc, ws_b, hs_b, rcs = ctx.decode_batch("cluster-colors(%d)" % K, out_p, stride, lens_p, F, dec, max(nbytes))
            mse_p = ctx.mse_batch_var(flat, offs, dec, [f * max(nbytes) for f in range(F)], [n // 3 for n in nbytes])
            rc2, _, _, rcs2 = ctx.decode_batch("cluster-colors(%d)" % K, out_s, stride, lens_s, F, dec, max(nbytes))
            mse_s = ctx.mse_batch_var(flat, offs, dec, [f * max(nbytes) for f in range(F)], [n // 3 for n in nbytes])
            ss, sp = stats(t_s), stats(t_p)
            emit(case="(b) 100 images of DIV2K's sizes, K = 256: the session's finishing call against a frozen palette of its centroids", frames=F,
                 mpix=round(npx / 1e6, 1), K=K, session_finish_frames_var=ss, palette_encode_frames_var=sp, palette_create=stats(t_c),
                 gpixels_per_s_palette=round(npx / (sp["median_ms"] * 1e-3) / 1e9, 2), stages_session=stages_s, stages_palette=stages_p,
                 palette_median_inside_session_min_max=bool(ss["min_ms"] <= sp["median_ms"] <= ss["max_ms"]),
                 same_streams=bool(lens_s == lens_p and torch.equal(out_s, out_p)), streams_differing=int(sum(1 for x, y in zip(lens_s, lens_p) if x != y)),
                 bytes_per_px_session=round(sum(lens_s) / npx, 4), bytes_per_px_palette=round(sum(lens_p) / npx, 4),
                 decodes=bool(rc == 0 and ws_b == ws and hs_b == hs and not any(rcs) and rc2 == 0 and not any(rcs2)),
                 sse_palette=float(sum(m * (n // 3) for m, n in zip(mse_p, nbytes))), sse_session=float(sum(m * (n // 3) for m, n in zip(mse_s, nbytes))),
                 kmeans_iterations=st["iterations"], palette_runs_ms=[round(t, 3) for t in t_p], session_runs_ms=[round(t, 3) for t in t_s])
            scc.close()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
