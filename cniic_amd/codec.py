"""Host-side mirror of the reference's Codec trait (src/codec.rs:14-19) and AnyCodec::from_str
(src/codec.rs:41-59) for the hot-path codecs, over the C ABI.

    codec = AnyCodec.from_str("cluster-colors(256)")
    data  = codec.encode(img)          # img: HxWx3 uint8
    img2  = codec.decode(data)         # None where the reference returns None / panics
    codec.name(), codec.is_lossless()

    HilbertRleApprox(4.0)               # hilbert(rle(4)): its own class, AnyCodec.from_str does not build it
"""
import math
from decimal import Decimal

from . import _lib


class Codec:
    """encode / decode / name / is_lossless, like `trait Codec` (src/codec.rs:14-19)."""

    def __init__(self, expr, ctx=None):
        if _lib.codec_parse(expr) is None:
            raise ValueError("Malformed codec argument: %r" % expr)  # main.rs:62-63
        self.expr = expr
        self._ctx = ctx
        self.last_stats = None

    @property
    def ctx(self):
        if self._ctx is None:
            self._ctx = _lib.Context(0)
        return self._ctx

    def encode(self, img, **kw):
        rc, data, st = self.ctx.encode(self.expr, img, **kw)
        self.last_stats = st
        return data

    def decode(self, data):
        rc, img = self.ctx.decode(self.expr, data, allow=(_lib.DECODE,))
        return img if rc == _lib.OK else None

    def decode_batch(self, streams):
        """decode of several streams at once (cniic_codec_decode_batch): a list of byte strings -> a list of images (None where the
        reference returns None / panics for that stream)"""
        import numpy as np
        F = len(streams)
        if F == 0:
            return []
        lens = [len(s) for s in streams]
        stride = max(max(lens), 1)
        buf = np.zeros(stride * F, np.uint8)
        for f, s in enumerate(streams):
            buf[f * stride:f * stride + len(s)] = np.frombuffer(bytes(s), np.uint8)
        npx = 0
        for s in streams:
            if len(s) >= 8:
                npx = max(npx, int.from_bytes(bytes(s[0:4]), "little") * int.from_bytes(bytes(s[4:8]), "little"))
        img_stride = max(min(npx, 1 << 28) * 3, 3)
        out = np.zeros(img_stride * F, np.uint8)
        rc, ws, hs, rcs = self.ctx.decode_batch(self.expr, buf, stride, lens, F, out, img_stride, allow=(_lib.DECODE, _lib.CAPACITY))
        imgs = []
        for f in range(F):
            if rcs[f] != _lib.OK:
                imgs.append(None)
                continue
            n = ws[f] * hs[f]
            imgs.append(out[f * img_stride:f * img_stride + n * 3].reshape(hs[f], ws[f], 3).copy())
        return imgs

    def name(self):
        return _lib.codec_name(self.expr)

    def is_lossless(self):
        return _lib.codec_is_lossless(self.expr)


class AnyCodec(Codec):
    @classmethod
    def from_str(cls, expr, ctx=None):
        return cls(expr, ctx)


def rust_f64_display(d):
    """f64's Display (format!("{}", d)): the shortest digits that read back as d, never an exponent ("1", "0.5", "0.0000001",
    "1000000000000000000000", "inf", "NaN", "-1", "-0")"""
    d = float(d)
    if math.isnan(d):
        return "NaN"
    if math.isinf(d):
        return "inf" if d > 0 else "-inf"
    s = format(Decimal(repr(d)), "f")   # repr: the shortest round-trip digits
    if "." in s:
        s = s.rstrip("0").rstrip(".")
    return s


class HilbertRleApprox(Codec):
    """Hilbert { compress: RLE(d) } (src/codec/hilbertc.rs:12-98, rle_approx :200-299) for any f64 d.  cniic_codec_parse takes only
    d == 0 (`hilbert(rle)`), so this codec has its own encode entry point; its streams decode as `hilbert(rle)` (same records)."""

    def __init__(self, d, ctx=None):
        self.d = float(d)
        self.expr = "hilbert(rle)"   # the decoder (RleDecoder, hilbertc.rs:304-335)
        self._ctx = ctx
        self.last_stats = None

    def encode(self, img, **kw):
        rc, data = self.ctx.hilbert_rle_approx_encode(self.d, img, **kw)
        return data

    def name(self):
        if self.d == 0.0:
            return "hilbert-rle"                                     # hilbertc.rs:83
        return "hilbert-rle-approx_%s" % rust_f64_display(self.d)   # :84

    def is_lossless(self):
        return self.d == 0.0
