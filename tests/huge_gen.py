"""Integer-only generators of the huge test images (tests/golden/make_huge_digests.py, tests/test_gpu_huge.py).

Each is written once over an array module: `xp = numpy` gives the oracle's rows on the host, `xp = torch` the test's rows on the
device.  Only int64 adds, products below 2^63, xors, shifts, masks, compares and a sorted-table search are used, so both give the
same bytes (tests/test_huge_gen.py holds them to each other on crops).  The photo itself is synth.photo = cniic_synth_image kind 1
(numpy rows: make_fullsize_digests.photo_rows).  sha256_chunked and equal_chunked look at device buffers without ever holding a whole
image or stream on the host.

  tiles    32 x 32 tiles, each tile's colour from an integer hash of (x >> 5, y >> 5)
  ripple   the tiles plus a slow +-2 ripple per channel, (((x >> 2) + (y >> 2) + ch) % 5) - 2, clamped to 0..255
  bg       the tiles with about 55 % of them (141 of every 256 hash values) one background colour
  fib      45 colours with Fibonacci counts F(1..45), sum F(47) - 1 = 2 971 215 072 = 46368 x 64079 pixels; pixel i takes the
           colour whose cumulative range holds (i P) mod N, P prime: a permutation of the pixels, so the counts are exact
"""
M32 = 0xFFFFFFFF
TILE_SEED = 0x5EED7115
BG_RGB = (200, 180, 160)
BG_BELOW = 141                 # a tile is background when its second hash byte is below this: 141 / 256 = 55 %
FIB_N = 45
FIB_W, FIB_H = 46368, 64079
FIB_P = 1000000007             # prime, not a factor of F(47) - 1; (i P) < 2^62 for every i < 2^32


def fib_counts():
    f = [1, 1]
    while len(f) < FIB_N:
        f.append(f[-1] + f[-2])
    return f


def fib_palette():
    """45 distinct colours (37, 91 and 53 are odd: c -> c k mod 256 is one to one)"""
    return [((37 * c + 11) & 255, (91 * c + 7) & 255, (53 * c + 3) & 255) for c in range(FIB_N)]


def _h32(v):
    v = ((v ^ (v >> 16)) * 0x45D9F3B) & M32
    v = ((v ^ (v >> 16)) * 0x45D9F3B) & M32
    return v ^ (v >> 16)


def _grid(xp, w, y0, y1, device):
    if device is None:
        y = xp.arange(y0, y1, dtype=xp.int64).reshape(-1, 1)
        x = xp.arange(0, w, dtype=xp.int64).reshape(1, -1)
    else:
        y = xp.arange(y0, y1, dtype=xp.int64, device=device).reshape(-1, 1)
        x = xp.arange(0, w, dtype=xp.int64, device=device).reshape(1, -1)
    return x, y


def _is_torch(xp):
    return xp.__name__ == "torch"


def _i64(xp, b):
    return b.to(xp.int64) if _is_torch(xp) else b.astype(xp.int64)


def _stack_u8(xp, chans):
    if _is_torch(xp):
        return xp.stack([c.to(xp.uint8) for c in chans], dim=-1)
    return xp.stack([c.astype(xp.uint8) for c in chans], axis=-1)


def tiles_rows(xp, w, y0, y1, kind="tiles", device=None):
    """rows y0..y1 of a w-wide image of kind tiles / ripple / bg: (y1 - y0, w, 3) uint8"""
    x, y = _grid(xp, w, y0, y1, device)
    k = _h32((((y >> 5) << 16) | (x >> 5)) ^ TILE_SEED)
    ch = [(k >> 16) & 255, (k >> 8) & 255, k & 255]
    if kind == "bg":
        isbg = _i64(xp, (_h32(k ^ 0x5BD1E995) & 255) < BG_BELOW)
        ch = [c * (1 - isbg) + v * isbg for c, v in zip(ch, BG_RGB)]
    elif kind == "ripple":
        s = (x >> 2) + (y >> 2)
        ch = [c + ((s + i) % 5) - 2 for i, c in enumerate(ch)]
        ch = [c * _i64(xp, c > 0) for c in ch]
        ch = [c - (c - 255) * _i64(xp, c > 255) for c in ch]
    else:
        assert kind == "tiles", kind
    return _stack_u8(xp, ch)


def fib_rows(xp, y0, y1, device=None):
    """rows y0..y1 of the 46368 x 64079 Fibonacci image"""
    x, y = _grid(xp, FIB_W, y0, y1, device)
    j = ((y * FIB_W + x) * FIB_P) % (sum(fib_counts()))
    ends, acc = [], 0
    for c in fib_counts():
        acc += c
        ends.append(acc)
    pal = fib_palette()
    if device is None:
        idx = xp.searchsorted(xp.asarray(ends, dtype=xp.int64), j, side="right")
        lut = xp.asarray(pal, dtype=xp.uint8)
    else:
        idx = xp.searchsorted(xp.tensor(ends, dtype=xp.int64, device=device), j.contiguous(), right=True)
        lut = xp.tensor(pal, dtype=xp.uint8, device=device)
    return lut[idx]


def sha256_chunked(t, n=None, chunk=1 << 30):
    """SHA-256 of the first n bytes of a uint8 tensor (on the device or the host), copied to the host chunk bytes at a time"""
    import hashlib

    import torch
    flat = t.reshape(-1)
    n = flat.numel() if n is None else int(n)
    h = hashlib.sha256()
    buf = torch.empty(min(chunk, max(n, 1)), dtype=torch.uint8, pin_memory=flat.is_cuda)
    for at in range(0, n, chunk):
        m = min(n, at + chunk) - at
        buf[:m].copy_(flat[at:at + m])
        h.update(memoryview(buf[:m].numpy()))
    return h.hexdigest()


def equal_chunked(a, b, chunk=1 << 30):
    """torch.equal of two uint8 tensors of the same size, a chunk of bytes at a time (no temporary as large as the images)"""
    import torch
    a, b = a.reshape(-1), b.reshape(-1)
    if a.numel() != b.numel():
        return False
    return all(torch.equal(a[at:at + chunk], b[at:at + chunk]) for at in range(0, a.numel(), chunk))
