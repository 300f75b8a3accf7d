"""Host-side mirror of the reference's Codec trait (src/codec.rs:14-19) and AnyCodec::from_str
(src/codec.rs:41-59) for the hot-path codecs, over the C ABI.

    codec = AnyCodec.from_str("cluster-colors(256)")
    data  = codec.encode(img)          # img: HxWx3 uint8
    img2  = codec.decode(data)         # None where the reference returns None / panics
    codec.name(), codec.is_lossless()
"""
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
