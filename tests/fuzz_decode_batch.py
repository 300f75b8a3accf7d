#!/usr/bin/env python3
# tests/fuzz_decode_batch.py [seconds] -- random batches through cniic_codec_decode_batch against the oracle (tests/oracle_lib.py).
# A case is one batch: 1..40 frames (now and then more) of one codec -- mostly `hufman` and `cluster-colors(K)`, which take the batched
# device decode, sometimes `delta`, `hilbert(rle)` (exact and running-average streams) and `voronoi(K)`, which take the worker contexts.
# Frames are cut short, emptied, flipped, given trailing bytes or a header that claims other dimensions; stream and image strides are
# tight, odd, large or tiny; streams and images sit in host memory or in HBM, in all four combinations.  Every frame's status must be
# the single decode's, it must succeed exactly when the oracle does (and the image fits img_stride), and its dimensions and pixels must
# be the oracle's.  The output is filled with a sentinel and followed by a guard: the bytes of a decoded frame past w*h*3, and the
# guard, must come back untouched.  FUZZ_SEED picks the sequence.
import os, sys, time
os.environ.setdefault("CNIIC_USE_TESTING_LIB", "1")   # CNIIC_TEST_DECODE_BATCH_OFF exists in the testing build of the library only
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
import numpy as np
import oracle_lib as O

rng = np.random.default_rng(int(os.environ.get("FUZZ_SEED", "1")))
GUARD = 256
MUTATIONS = ("cut", "empty", "under8", "flip_decoder", "flip_payload", "trailing", "w_smaller", "h_smaller", "larger", "too_large")


def fib_counts(n):
    """Fibonacci counts 1, 1, 2, 3, 5, ... that add up to n (the remainder on the largest): the deepest Huffman tree n pixels allow"""
    c = [1, 1] if n >= 2 else [n]
    while n >= 2 and sum(c) + c[-1] + c[-2] <= n:
        c.append(c[-1] + c[-2])
    c[-1] += n - sum(c)
    return c


def image(h=None, w=None):
    r = rng.random()
    if h is not None:
        pass
    elif r < 0.25:
        s = int(2 ** rng.integers(0, 9)); h = w = s
    elif r < 0.85:
        h, w = int(rng.integers(1, 120)), int(rng.integers(1, 120))
    else:
        h, w = int(rng.integers(1, 301)), int(rng.integers(1, 301))
    y, x = np.mgrid[0:h, 0:w]
    kind = int(rng.integers(0, 5))
    if kind == 0:     # noise
        img = rng.integers(0, 256, (h, w, 3))
    elif kind == 1:   # smooth
        img = np.stack([x // 2 + y // 3, x // 3 + y, (x + y) // 4], axis=2) + rng.integers(-3, 4, (h, w, 3))
    elif kind == 2:   # flat: a one-leaf decoder
        img = np.zeros((h, w, 3), np.int64) + rng.integers(0, 256, 3)
    elif kind == 3:   # a few colours
        pal = rng.integers(0, 256, (int(rng.integers(2, 9)), 3))
        img = pal[rng.integers(0, len(pal), (h, w))]
    else:             # Fibonacci counts: the longest codes the size allows (22 bits at 300 x 300)
        c = fib_counts(h * w)
        cols = rng.choice(1 << 24, len(c), replace=False)
        keys = rng.permutation(np.repeat(cols, c))
        img = np.stack([keys >> 16, keys >> 8, keys], axis=1).reshape(h, w, 3)
    return np.ascontiguousarray(img & 255, np.uint8)


def codec():
    r = rng.random()
    if r < 0.4:
        return "hufman"
    if r < 0.8:
        return "cluster-colors(%d)" % int(rng.choice([1, 2, 3, 4, 16, 255, 256, 257, 300]) if rng.random() < 0.5 else rng.integers(1, 301))
    return str(rng.choice(["delta", "hilbert(rle)", "voronoi(%d)" % int(rng.integers(1, 301))]))


def encode(ctx, expr, img):
    """the frame's stream (GPU encoder), or a few random bytes where the image does not encode (too few points for K)"""
    from cniic_amd import _lib
    if expr == "hilbert(rle)" and rng.random() < 0.4:   # the lossy running-average encoder writes streams the exact decoder reads
        rc, data = ctx.hilbert_rle_approx_encode(float(rng.choice([0.5, 1.0, 3.0, 8.0, 40.0])), img)
    else:
        rc, data, _ = ctx.encode(expr, img, allow=(_lib.TOO_FEW_POINTS, _lib.FEW_ACTIVE))
    return data if rc == 0 else rng.integers(0, 256, int(rng.integers(0, 40)), dtype=np.uint8).tobytes()


def mutate(data, img_stride):
    """one of MUTATIONS (or none) applied to a stream -> (name, bytes)"""
    if rng.random() < 0.55 or not data:
        return "none", data
    m = str(rng.choice(MUTATIONS))
    b = bytearray(data)
    n = len(b)
    if m == "cut":
        return m, bytes(b[:int(rng.integers(0, n))])
    if m == "empty":
        return m, b""
    if m == "under8":
        return m, bytes(b[:int(rng.integers(1, 8))])
    if m in ("flip_decoder", "flip_payload"):
        lo, hi = (8, min(n, 8 + 16 + n // 8)) if m == "flip_decoder" else (n // 2, n)
        if hi <= lo:
            lo, hi = 0, n
        for _ in range(int(rng.integers(1, 4))):
            b[int(rng.integers(lo, hi))] ^= int(rng.integers(1, 256))
        return m, bytes(b)
    if m == "trailing":
        return m, bytes(b) + rng.integers(0, 256, int(rng.integers(1, 65)), dtype=np.uint8).tobytes()
    if n < 8:
        return m, data
    w, h = int.from_bytes(b[0:4], "little"), int.from_bytes(b[4:8], "little")
    if m == "w_smaller" and w > 1:   # fewer symbols than the payload holds: the rest must not be written
        w = int(rng.integers(1, w))
    elif m == "h_smaller" and h > 1:
        h = int(rng.integers(1, h))
    elif m == "larger":
        w += int(rng.integers(1, 9))
    elif m == "too_large":   # just past img_stride
        w = max(w, img_stride // (3 * max(h, 1)) + 1)
    b[0:4], b[4:8] = w.to_bytes(4, "little"), (h & 0xffffffff).to_bytes(4, "little")
    return m, bytes(b)


try:
    import torch as TORCH
    if not TORCH.cuda.is_available():
        TORCH = None
except Exception:
    TORCH = None


def _on_device(a, shift):
    """a copy of the numpy byte array `a` in HBM, starting `shift` bytes into an allocation of its own"""
    buf = TORCH.empty(a.size + shift + 16, dtype=TORCH.uint8, device="cuda")
    buf[shift:shift + a.size] = TORCH.from_numpy(a).cuda()
    return buf[shift:shift + a.size]


def one_case(ctx):
    """one random batch, checked frame by frame; returns a description of it"""
    from cniic_amd import _lib
    expr = codec()
    F = int(rng.integers(1, 41)) if rng.random() < 0.9 else int(rng.integers(41, 120))
    imgs = [image() for _ in range(F)]
    if rng.random() < 0.3:   # one size throughout, as in the benchmark's batches
        imgs = [image(*imgs[0].shape[:2]) for _ in range(F)]
    clean = [encode(ctx, expr, im) for im in imgs]
    tight = max(max(im.shape[0] * im.shape[1] * 3 for im in imgs), 1)
    img_stride = tight + int(rng.choice([0, 0, 1, 2, 3, 5, 4096 + int(rng.integers(0, 4096))]))
    muts, streams = zip(*[mutate(d, img_stride) for d in clean])
    streams = list(streams)
    lens = [len(s) for s in streams]
    r = rng.random()
    if r < 0.06:   # a stride below a header's 8 bytes: every frame fails, each on its own
        stride = int(rng.integers(0, 8))
        lens = [min(x, int(rng.integers(0, stride + 1))) for x in lens]
    elif r < 0.4:
        stride = max(lens)
    elif r < 0.7:
        stride = max(lens) + int(rng.integers(0, 8)) * 2 + 1
    else:
        stride = max(lens) + int(rng.integers(1, 70000))
    stride = max(stride, 0)
    buf = np.zeros(F * stride + max(lens + [0]) + 16, np.uint8)
    for f in range(F):
        buf[f * stride:f * stride + lens[f]] = np.frombuffer(streams[f][:lens[f]], np.uint8)
    data = [buf[f * stride:f * stride + lens[f]].tobytes() for f in range(F)]
    dev_in = TORCH is not None and rng.random() < 0.5
    dev_out = TORCH is not None and rng.random() < 0.5
    sentinel = int(rng.integers(0, 256))
    need = F * img_stride + GUARD
    out_h = np.full(need, sentinel, np.uint8)
    src = _on_device(buf, int(rng.integers(0, 4))) if dev_in else buf
    out = _on_device(out_h, int(rng.integers(0, 4))) if dev_out else out_h
    off = sorted(set(int(x) for x in rng.integers(0, F, int(rng.integers(1, 4))))) if rng.random() < 0.25 else []
    workers = rng.choice([-1, 1, 2, 3, 8, 16])
    what = dict(expr=expr, F=F, stride=stride, img_stride=img_stride, dev_in=dev_in, dev_out=dev_out, off=off, workers=int(workers),
                mutations=[(f, m) for f, m in enumerate(muts) if m != "none"])
    if TORCH is not None:
        TORCH.cuda.synchronize()   # (ctx may run on a stream of its own: torch's copies must have landed)
    saved = os.environ.get("CNIIC_TEST_DECODE_BATCH_OFF")
    if off:
        os.environ["CNIIC_TEST_DECODE_BATCH_OFF"] = ",".join(map(str, off))
    else:
        os.environ.pop("CNIIC_TEST_DECODE_BATCH_OFF", None)
    ctx.set_opt(_lib.OPT_BATCH_STREAMS, None if workers < 0 else int(workers))
    try:
        rc, ws, hs, rcs = ctx.decode_batch(expr, src, stride, lens, F, out, img_stride, allow=tuple(range(-1, -10, -1)))
    finally:
        ctx.set_opt(_lib.OPT_BATCH_STREAMS, None)
        if saved is None:
            os.environ.pop("CNIIC_TEST_DECODE_BATCH_OFF", None)
        else:
            os.environ["CNIIC_TEST_DECODE_BATCH_OFF"] = saved
    got = out.cpu().numpy() if dev_out else out_h
    assert rc != _lib.HIP, (what, "HIP error", rc)
    assert rc == next((x for x in rcs if x != 0), 0), (what, rc, rcs)
    for f in range(F):
        orc, oimg = O.decode(expr, data[f])
        single = np.zeros(max(img_stride, 1), np.uint8)
        raw = np.frombuffer(data[f] + b"\0", np.uint8)   # (a pointer even for an empty stream)
        src1, sw, sh = ctx.decode_into(expr, raw, lens[f], single, allow=tuple(range(-1, -10, -1)))
        at = (f, muts[f], lens[f], what)
        assert rcs[f] == src1, at + ("status", rcs[f], "single", src1)
        ok = orc == 0 and oimg.size <= img_stride
        assert (rcs[f] == 0) == ok, at + ("status", rcs[f], "oracle", orc, None if oimg is None else oimg.shape)
        if not ok:
            continue
        oh, ow = oimg.shape[:2]
        assert (ws[f], hs[f]) == (ow, oh) == (sw, sh), at + ("dimensions", ws[f], hs[f], ow, oh)
        frame = got[f * img_stride:(f + 1) * img_stride]
        assert np.array_equal(frame[:oimg.size], oimg.reshape(-1)), at + ("pixels",)
        assert np.array_equal(single[:oimg.size], oimg.reshape(-1)), at + ("single pixels",)
        assert (frame[oimg.size:] == sentinel).all(), at + ("a write past w*h*3 at", oimg.size + int(np.argmax(frame[oimg.size:] != sentinel)))
    assert (got[F * img_stride:F * img_stride + GUARD] == sentinel).all(), (what, "a write past the last frame")
    return what


def run(ctx, budget):
    """`budget` seconds of random batches on ctx; returns how many were checked (an assertion stops at the first difference)"""
    t0, cases, said = time.time(), 0, time.time()
    while time.time() - t0 < budget:
        if time.time() - said > 60:   # (a long run says that it is alive)
            said = time.time()
            sys.stderr.write("fuzz: %d batches after %.0f s\n" % (cases, said - t0)); sys.stderr.flush()
        one_case(ctx)
        cases += 1
    return cases


if __name__ == "__main__":
    import cniic_amd
    seconds = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
    if TORCH is not None:
        TORCH.cuda.set_stream(TORCH.cuda.Stream())   # (a context does not share the NULL stream)
    ctx = cniic_amd.Context(0, stream=TORCH.cuda.current_stream().cuda_stream) if TORCH is not None else cniic_amd.Context(0)
    n = run(ctx, seconds)
    print("fuzz_decode_batch: %d batches in %.0f s, every frame equal to the oracle and to its single decode" % (n, seconds))
