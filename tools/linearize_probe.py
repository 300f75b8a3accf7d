#!/usr/bin/env python3
"""The three linearisations (cniic_hilbert_linearize_as: rect, small, large) and cniic_channel_diff_hist on device buffers, photo-like and
flat images, with cniic_hilbert_linearize of the same build beside them for scale.  One JSON line each: the call's wall time (median of
seven, the call waits for the GPU) and, where the call has a stage timer, the kernels' own time from it.  Tools only (NOTES.md, section M)."""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch, cniic_amd
from cniic_amd import _lib, synth
dev = torch.device("cuda", 0)
ctx = cniic_amd.Context(0)
C = _lib.C
def wall(fn, reps=7):
    fn(); fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)
shapes = [(4096, 4096), (4000, 3000)] if len(sys.argv) < 2 else [tuple(int(v) for v in a.split("x")) for a in sys.argv[1:]]
for w, h in shapes:
    for kind in ("photo", "flat"):
        img = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
        if kind == "photo": ctx.synth_image(_lib.SYNTH_PHOTO, synth.SEED0 + 21, w, h, out=img)
        else: img[:] = torch.tensor([9, 200, 77], dtype=torch.uint8, device=dev)
        out = torch.empty(w * h * 3, dtype=torch.uint8, device=dev)
        cnt = torch.zeros((3, 511), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        rows = {}
        rows["cniic_hilbert_linearize"] = (wall(lambda: ctx._check(ctx._L.cniic_hilbert_linearize(ctx.h, _lib._ptr(img), C.c_uint32(w), C.c_uint32(h), _lib._ptr(out)))), None)
        for m, stage in (("rect", None), ("small", "lin_small"), ("large", "lin_large")):
            ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
            ms = wall(lambda: ctx.hilbert_linearize_as(img, m, w, h, out))
            k = None
            if stage:
                ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
                ks = []
                for _ in range(5):
                    ctx.hilbert_linearize_as(img, m, w, h, out); ks.append(ctx.kernel_time(stage)[0])
                k = statistics.median(ks)
            rows["linearize_as " + m] = (ms, k)
        n = _lib.linearize_count("large", w, h)
        ctx.hilbert_linearize_as(img, "large", w, h, out)
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
        ms = wall(lambda: ctx.channel_diff_hist(out, npx=n, out=cnt))
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
        ks = []
        for _ in range(5):
            ctx.channel_diff_hist(out, npx=n, out=cnt); ks.append(ctx.kernel_time("chan_diff_hist")[0])
        rows["channel_diff_hist (of large)"] = (ms, statistics.median(ks))
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
        assert int(cnt.sum().item()) == 3 * (n - 1)
        for name, (ms, k) in rows.items():
            print(json.dumps(dict(w=w, h=h, image=kind, call=name, wall_ms=round(ms, 4), kernel_ms=None if k is None else round(k, 4))), flush=True)
