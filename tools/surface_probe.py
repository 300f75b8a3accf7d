"""cniic_frames_from_surfaces / cniic_frames_to_surfaces on the release library, device buffers throughout:
  pan       32 windows of 1920 x 1080 out of one 4096 x 4096 RGB8 image (tools/warm_probe.py's pan) as 32 descriptors in ONE call,
            against what a caller had to write before: a loop of 32 hipMemcpy2DAsync and one synchronise.  The two alternate.
  formats   the 100 DIV2K-sized frames of tools/batch_var_probe.py (273 Mpixels) as RGBA8, BGRA8, L8 and NV12 (709 limited) surfaces with
            256-byte pitches: import, and export where there is one; time and bytes read + written per second, beside a device-to-device
            hipMemcpyAsync that moves the same number of bytes (read + written) in the same run.
One warm-up, then medians of --reps with min and max.  One JSON line per case; --out FILE also writes them there.
    python tools/surface_probe.py [--out profiles/surface_probe.json] [--reps 5] [--only pan|import:rgba8|export:bgra8|import:nv12|...]
--only: that one call, once, and nothing else (for a profiler run of its own)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import cniic_amd
from cniic_amd import _lib
from cniic_amd._lib import Surface

from batch_var_probe import div2k_like_sizes

FORMATS = {"rgba8": _lib.PX_RGBA8, "bgra8": _lib.PX_BGRA8, "l8": _lib.PX_L8, "nv12": _lib.PX_NV12}
D2D = 3   # hipMemcpyDeviceToDevice


def hip():
    h = C.CDLL("libamdhip64.so")
    h.hipMemcpy2DAsync.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p]
    h.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    h.hipStreamSynchronize.argtypes = [C.c_void_p]
    h.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    return h


def clock(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def stats(ts):
    return dict(median_ms=round(statistics.median(ts), 3), min_ms=round(min(ts), 3), max_ms=round(max(ts), 3), runs=len(ts))


def alternate(fns, reps):
    """every function once untimed, then `reps` rounds of all of them in turn -> one stats dict per function"""
    for fn in fns:
        fn()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            ts[i].append(clock(fn))
    return [stats(t) for t in ts]


def pan(ctx, H, stream, a, emit):
    dev = torch.device("cuda", 0)
    side, w, h, n = 4096, 1920, 1080, 32
    img = torch.randint(0, 256, (side, side, 3), dtype=torch.uint8, device=dev)
    surfaces, offs = [], []
    for i in range(n):
        x, y = i * (side - w) // (n - 1), i * (side - h) // (n - 1)
        surfaces.append(Surface(off=(y * side + x) * 3, pitch=side * 3, w=w, h=h, format=_lib.PX_RGB8))
        offs.append(i * w * h * 3)
    out, out2 = torch.zeros(n * w * h * 3, dtype=torch.uint8, device=dev), torch.zeros(n * w * h * 3, dtype=torch.uint8, device=dev)

    def call():
        ctx.frames_from_surfaces(img, surfaces, out, offs)
        ctx.sync()

    def loop():
        for s, o in zip(surfaces, offs):
            rc = H.hipMemcpy2DAsync(out2.data_ptr() + o, w * 3, img.data_ptr() + s.off, s.pitch, w * 3, h, D2D, stream)
            assert rc == 0
        assert H.hipStreamSynchronize(stream) == 0
    if a.only:
        return call()
    t_call, t_loop = alternate([call, loop], a.reps)
    spread = t_loop["max_ms"] - t_loop["min_ms"]
    traffic = 2 * n * w * h * 3
    emit(case="pan: 32 windows of 1920x1080 out of 4096x4096 RGB8", one_call=t_call, loop_of_32_hipMemcpy2DAsync=t_loop, same=bool(torch.equal(out, out2)),
         gbytes_per_s=dict(one_call=round(traffic / t_call["median_ms"] / 1e6, 1), loop=round(traffic / t_loop["median_ms"] / 1e6, 1)),
         call_over_loop=round(t_call["median_ms"] / t_loop["median_ms"], 3), loop_spread_ms=round(spread, 3),
         slower_by_more_than_the_loops_spread=bool(t_call["median_ms"] > t_loop["median_ms"] + spread))


def up(x, m):
    return (x + m - 1) // m * m


def formats(ctx, H, stream, a, emit):
    dev = torch.device("cuda", 0)
    sizes = div2k_like_sizes()
    npx = sum(w * h for w, h in sizes)
    offs, at = [], 0
    for w, h in sizes:            # back to back: most frames off the 16-byte boundaries
        offs.append(at)
        at += 3 * w * h
    rgb = torch.randint(0, 256, (at,), dtype=torch.uint8, device=dev)
    back = torch.zeros_like(rgb)
    for name, fmt in FORMATS.items():
        if a.only and a.only.split(":")[1] != name:
            continue
        bpp = _lib.PX_BYTES[fmt]
        surfaces, end = [], 0
        for w, h in sizes:
            s = Surface(off=up(end, 256), pitch=up(w * bpp, 256), w=w, h=h, format=fmt)
            if fmt == _lib.PX_NV12:
                s.matrix, s.pitch_uv = _lib.YUV_709_LIMITED, s.pitch
                s.off_uv = s.off + h * s.pitch
            end = _lib.surface_span(s)[0]
            surfaces.append(s)
        surf = torch.randint(0, 256, (end,), dtype=torch.uint8, device=dev)
        moved_in = (npx * bpp + (npx // 2 if fmt == _lib.PX_NV12 else 0)) + 3 * npx     # the bytes the import reads + writes (NV12: chroma once)

        def imp():
            ctx.frames_from_surfaces(surf, surfaces, back, offs)
            ctx.sync()

        def exp():
            ctx.frames_to_surfaces(rgb, offs, surfaces, surf, alpha=255)
            ctx.sync()

        ncopy = min(moved_in // 2, rgb.numel())   # (per byte it makes no difference that the largest formats move a little more than the copy)

        def copy():   # the floor: hipMemcpyAsync device to device, which reads ncopy bytes and writes ncopy bytes
            assert H.hipMemcpyAsync(back.data_ptr(), rgb.data_ptr(), ncopy, D2D, stream) == 0
            assert H.hipStreamSynchronize(stream) == 0
        copied = 2 * ncopy
        writable = fmt in (_lib.PX_RGBA8, _lib.PX_BGRA8)
        if a.only:
            return imp() if a.only.startswith("import") else exp()
        fns = [imp, copy] + ([exp] if writable else [])
        ts = alternate(fns, a.reps)
        gbs = lambda nbytes, t: round(nbytes / t["median_ms"] / 1e6, 1)
        copy_per_byte = ts[1]["median_ms"] / copied
        row = dict(case="100 DIV2K-sized frames as %s surfaces, 256-byte pitches" % name.upper(), mpix=round(npx / 1e6, 1), import_=ts[0], mbytes_read_plus_written=round(moved_in / 1e6, 1),
                   import_gbytes_per_s=gbs(moved_in, ts[0]), d2d_copy=ts[1], d2d_copy_mbytes_read_plus_written=round(copied / 1e6, 1), d2d_copy_gbytes_per_s=gbs(copied, ts[1]),
                   import_over_copy_per_byte=round(ts[0]["median_ms"] / moved_in / copy_per_byte, 3))
        if writable:
            ctx.frames_from_surfaces(surf, surfaces, back, offs)    # (surf now holds the export of rgb)
            ctx.sync()
            row.update(export=ts[2], export_gbytes_per_s=gbs(moved_in, ts[2]), export_over_copy_per_byte=round(ts[2]["median_ms"] / moved_in / copy_per_byte, 3),
                       import_of_export_is_identity=bool(torch.equal(back, rgb)))
        emit(**row)
        del surf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only")
    a = ap.parse_args()
    rows = []

    def emit(**row):
        print(json.dumps(row), flush=True)
        rows.append(row)
    H = hip()
    stream = C.c_void_p()
    assert H.hipStreamCreate(C.byref(stream)) == 0
    with cniic_amd.Context(0) as ctx:
        assert ctx._L.cniic_is_testing_build() == 0, "measure on the release library"
        if not a.only or a.only == "pan":
            pan(ctx, H, stream, a, emit)
        if not a.only or ":" in a.only:
            formats(ctx, H, stream, a, emit)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
