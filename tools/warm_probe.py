"""K-means from given centroids and the fit of a frozen palette on the release library, device buffers throughout; medians of --reps runs
with min - max (one warm-up first).
  (a) the pan   1920 x 1080 windows that slide by (8, 4) pixels a frame over one 4096^2 photo-like image, 32 frames.  Per frame,
                cluster-colors(256) and voronoi(2048): cniic_codec_encode_warm fed the previous frame's centroids_out against
                cniic_codec_encode_opts (the cold call) on the same frame in the same run -- iterations, wall time, bytes per pixel, MSE.
                (Frame 0 has no previous frame: it is coded cold-equivalent from a grid of centroids and left out of the figures.)
  (b) refresh   one shared palette for frames 0 - 15; then frames 16 - 31: cniic_palette_fit_frames_var of the old palette on them, a session
                with cniic_cc_set_centroids(old palette) against a cold session -- iterations, the loop's time, the whole session's time.
  (c) pal_fit   beside pal_labels (the same gather) on the 100 images of DIV2K's sizes of tools/batch_var_probe.py, K = 256, and on a flat
                folder of the same sizes: the kernels through the stage timers, the calls by the wall clock.
    python tools/warm_probe.py [--out profiles/warm_probe.json] [--reps 5] [--only a|b|c] [--frames 32]"""
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
from cniic_amd.dist import HipBackend

W, H, STEP_X, STEP_Y, SIDE = 1920, 1080, 8, 4, 4096


def stats(ts):
    return dict(median_ms=round(statistics.median(ts), 3), min_ms=round(min(ts), 3), max_ms=round(max(ts), 3), runs=len(ts))


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, res


def spread(vs):
    return dict(median=round(statistics.median(vs), 4), min=round(min(vs), 4), max=round(max(vs), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--only", choices=("a", "b", "c"))
    a = ap.parse_args()
    assert os.environ.get("CNIIC_USE_TESTING_LIB") != "1", "the probe measures the release library"
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(device=dev))
    rows = []

    def emit(**row):
        print(json.dumps(row), flush=True)
        rows.append(row)

    with cniic_amd.Context(0, stream=torch.cuda.current_stream().cuda_stream) as ctx:
        F = a.frames
        big = torch.empty(SIDE * SIDE * 3, dtype=torch.uint8, device=dev)
        ctx.synth_image(_lib.SYNTH_PHOTO, synth.SEED0 + 4242, SIDE, SIDE, big)
        ctx.sync()
        pan = big.view(SIDE, SIDE, 3)
        frames = [pan[STEP_Y * f:STEP_Y * f + H, STEP_X * f:STEP_X * f + W].contiguous() for f in range(F)]
        torch.cuda.synchronize()
        npx = W * H

        if a.only in (None, "a"):
            for expr, K, xy in (("cluster-colors(256)", 256, False), ("voronoi(2048)", 2048, True)):
                cap = 64 + npx * 4 + 19 * K + (1 << 16)
                out_w = torch.empty(cap, dtype=torch.uint8, device=dev)
                out_c = torch.empty(cap, dtype=torch.uint8, device=dev)
                dec = torch.empty(npx * 3, dtype=torch.uint8, device=dev)
                if xy:   # frame 0: a grid of positions, mid grey
                    init = np.zeros(K, _lib.COLORPOS)
                    g = np.arange(K)
                    init["x"], init["y"], init["rgb"] = (g % 64) * (W // 64), (g // 64) * (H // 32), 128
                else:
                    init = np.repeat(np.arange(K, dtype=np.uint8)[:, None], 3, axis=1)
                per_frame = []
                for f in range(F):
                    tw, tc = [], []
                    for i in range(a.reps + 1):
                        t1, (rc, n_w, st_w, cent) = wall(lambda: ctx.encode_warm(expr, frames[f], init, w=W, h=H, out=out_w))
                        t2, (rc2, n_c, st_c) = wall(lambda: ctx.encode(expr, frames[f], w=W, h=H, out=out_c))
                        if i:
                            tw.append(t1); tc.append(t2)
                    mse = []
                    for buf, n in ((out_w, n_w), (out_c, n_c)):
                        rcd, dw, dh = ctx.decode_into(expr, buf, n, dec)
                        assert rcd == 0 and (dw, dh) == (W, H)
                        mse.append(ctx.mse(frames[f], dec))
                    per_frame.append(dict(frame=f, warm=stats(tw), cold=stats(tc), iterations_warm=st_w["iterations"], iterations_cold=st_c["iterations"],
                                          reseeds_warm=st_w["empty_reseeds"], bytes_warm=n_w, bytes_cold=n_c, mse_warm=round(mse[0], 4), mse_cold=round(mse[1], 4)))
                    init = cent
                fed = per_frame[1:]   # the frames that had a previous frame
                emit(case="(a) the pan: %s, warm (the previous frame's centroids) against cold, per frame" % expr, frames=len(fed), width=W, height=H,
                     step=[STEP_X, STEP_Y], iterations_warm=spread([r["iterations_warm"] for r in fed]), iterations_cold=spread([r["iterations_cold"] for r in fed]),
                     warm_ms=spread([r["warm"]["median_ms"] for r in fed]), cold_ms=spread([r["cold"]["median_ms"] for r in fed]),
                     speedup=spread([r["cold"]["median_ms"] / r["warm"]["median_ms"] for r in fed]),
                     bytes_per_px_warm=spread([r["bytes_warm"] / npx for r in fed]), bytes_per_px_cold=spread([r["bytes_cold"] / npx for r in fed]),
                     mse_warm=spread([r["mse_warm"] for r in fed]), mse_cold=spread([r["mse_cold"] for r in fed]),
                     mse_warm_over_cold=spread([r["mse_warm"] / r["mse_cold"] for r in fed if r["mse_cold"] > 0] or [0.0]),
                     frame0=per_frame[0], per_frame=fed)

        if a.only in (None, "b") and F >= 4:
            K, half = 256, F // 2
            be = HipBackend(ctx, dev)
            old_flat = torch.cat([fr.reshape(-1) for fr in frames[:half]])
            new_flat = torch.cat([fr.reshape(-1) for fr in frames[half:]])
            n_new = (F - half) * npx
            ws, hs = [W] * (F - half), [H] * (F - half)

            def session(flat, n, init):
                """-> (handle, stats, ms of the loop alone)"""
                h = be.image_begin(flat, n)
                occ = be.image_occupancy(h)
                partials = be.new_partials(K)
                be.image_create(h, occ, K, partials)
                if init is not None:
                    be.set_centroids(h, init)
                t, st = wall(lambda: be.run(h, None))
                return h, st, t

            h0, _, _ = session(old_flat, half * npx, None)
            old, _ = be.palette(h0, K)
            be.destroy(h0)
            t_fit, t_warm, t_cold, l_warm, l_cold = [], [], [], [], []
            with cniic_amd.Palette.create(ctx, old) as pal:
                for i in range(a.reps + 1):
                    t, (sse, pixels) = wall(lambda: pal.fit_frames_var(new_flat, ws, hs))
                    if i:
                        t_fit.append(t)
                sse_old_on_old, _ = pal.fit_frames_var(old_flat, [W] * half, [H] * half)
            res = {}
            for i in range(a.reps + 1):
                for name, init, tt, ll in (("warm", old, t_warm, l_warm), ("cold", None, t_cold, l_cold)):
                    t, (h, st, loop) = wall(lambda: session(new_flat, n_new, init))
                    cent, _ = be.palette(h, K)
                    be.destroy(h)
                    res[name] = (st, cent)
                    if i:
                        tt.append(t); ll.append(loop)
            fits = {}
            for name in ("warm", "cold"):
                with cniic_amd.Palette.create(ctx, res[name][1]) as p:
                    fits[name] = float(p.fit_frames_var(new_flat, ws, hs)[0].sum()) / (3.0 * n_new)
            emit(case="(b) a shared palette refreshed: K = 256 built on frames 0 - %d, then frames %d - %d" % (half - 1, half, F - 1), frames_new=F - half,
                 mpix_new=round(n_new / 1e6, 1), pal_fit_call=stats(t_fit), mse_old_palette_on_its_own_frames=round(float(sse_old_on_old.sum()) / (3.0 * half * npx), 4),
                 mse_old_palette_on_new_frames=round(float(sse.sum()) / (3.0 * n_new), 4), entries_without_pixels=int((pixels == 0).sum()),
                 iterations_warm=res["warm"][0]["iterations"], iterations_cold=res["cold"][0]["iterations"], loop_warm=stats(l_warm), loop_cold=stats(l_cold),
                 session_warm=stats(t_warm), session_cold=stats(t_cold), mse_warm_palette_under_the_rule=round(fits["warm"], 4),
                 mse_cold_palette_under_the_rule=round(fits["cold"], 4))

        if a.only in (None, "c"):
            K = 256
            sizes = div2k_like_sizes()
            Fd = len(sizes)
            ws, hs = [w for w, _ in sizes], [h for _, h in sizes]
            nbytes = [3 * w * h for w, h in sizes]
            offs = [sum(nbytes[:f]) for f in range(Fd)]
            n = sum(nbytes) // 3
            src = torch.empty(sum(nbytes) + 16, dtype=torch.uint8, device=dev)
            for f, (w, h) in enumerate(sizes):
                ctx.synth_image(_lib.SYNTH_PHOTO, synth.SEED0 + 6000 + f, w, h, src[offs[f]:])
            ctx.sync()
            flat = src[:sum(nbytes)]
            sample = flat[:3 * 640 * 480].cpu().numpy().reshape(-1, 3)
            cent = sample[np.random.default_rng(K).choice(sample.shape[0], K, replace=False)].copy()
            flat_folder = torch.empty_like(flat).view(-1, 3)
            flat_folder[:] = torch.tensor([int(v) for v in cent[7]], dtype=torch.uint8, device=dev)
            flat_folder = flat_folder.view(-1)
            labels = torch.empty(n + 16, dtype=torch.uint8, device=dev)
            with cniic_amd.Palette.create(ctx, cent) as pal:
                for name, data in (("photographs", flat), ("a flat folder", flat_folder)):
                    t_fit, t_lab, k_fit, k_lab = [], [], [], []
                    for i in range(a.reps + 1):
                        t1, _ = wall(lambda: pal.fit_frames_var(data, ws, hs))
                        t2, _ = wall(lambda: pal.labels(data, n, labels))
                        if i:
                            t_fit.append(t1); t_lab.append(t2)
                    ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
                    for i in range(a.reps + 1):
                        pal.fit_frames_var(data, ws, hs)
                        kf = ctx.kernel_time("pal_fit")
                        pal.fit_frames_var(data, ws, hs, want_pixels=False)
                        kn = ctx.kernel_time("pal_fit")
                        pal.labels(data, n, labels)
                        kl = ctx.kernel_time("pal_labels")
                        if i:
                            k_fit.append(kf[0]); k_lab.append(kl[0])
                    ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
                    emit(case="(c) pal_fit beside pal_labels, 100 images of DIV2K's sizes, K = 256: %s" % name, frames=Fd, mpix=round(n / 1e6, 1),
                         pal_fit_kernel=stats(k_fit), pal_labels_kernel=stats(k_lab), pal_fit_kernel_without_counts_ms=round(kn[0], 3), launches=int(kf[1]),
                         fit_call=stats(t_fit), labels_call=stats(t_lab), fit_over_labels_kernel=round(statistics.median(k_fit) / statistics.median(k_lab), 3))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
