"""Host-side mirror of the reference's Codec trait (src/codec.rs:14-19) and AnyCodec::from_str
(src/codec.rs:41-59) for the hot-path codecs, over the C ABI.

    codec = AnyCodec.from_str("cluster-colors(256)")
    data  = codec.encode(img)          # img: HxWx3 uint8
    img2  = codec.decode(data)         # None where the reference returns None / panics
    codec.name(), codec.is_lossless()

    AnyCodec.from_str("hilbert(rle(4))")   # the lossy running-average RLE is an expression like the others
    HilbertRleApprox(4.0)                   # the same codec for a caller that holds d as a float
    AnyCodec.from_str("zip(dict)")          # the dictionary coder over the serialised image
    HilbertZip()                            # Hilbert { compress: Zip }: not an expression here, a class of its own
    ZipBack()                               # Zip::Back, the look-back coder: likewise
"""
import math
from decimal import Decimal

import numpy as np

from . import _lib


class Codec:
    """encode / decode / name / is_lossless, like `trait Codec` (src/codec.rs:14-19)."""

    def __init__(self, expr, ctx=None):
        if _lib.codec_parse_f64(expr) is None:
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

    def encode_warm(self, img, init, **kw):
        """cluster-colors(K) / voronoi(K) only: encode with the K-means started from init (the centroids of the previous frame of a video,
        of a neighbouring tile: (K, 3) uint8, or K _lib.COLORPOS entries) -> (stream, final centroids: the next call's init).  Any other
        codec raises CniicError(BAD_ARG)."""
        rc, data, st, cent = self.ctx.encode_warm(self.expr, img, init, **kw)
        self.last_stats = st
        return data, cent

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
            dims = _lib.stream_dims(self.expr, s)
            if dims is not None:
                npx = max(npx, dims[0] * dims[1])
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

    @staticmethod
    def _packed(imgs):
        """images of any sizes back to back in one host buffer -> (buffer, offsets, widths, heights)"""
        import numpy as np
        imgs = [np.ascontiguousarray(im, np.uint8) for im in imgs]
        for im in imgs:
            if im.ndim != 3 or im.shape[2] != 3:
                raise ValueError("images are HxWx3 uint8 arrays, not %r" % (im.shape,))
        offs = [0]
        for im in imgs:
            offs.append(offs[-1] + im.size)
        buf = np.concatenate([im.reshape(-1) for im in imgs] + [np.zeros(1, np.uint8)])
        return buf, offs[:-1], [im.shape[1] for im in imgs], [im.shape[0] for im in imgs]

    ENCODE_FAILURES = (_lib.BAD_ARG, _lib.TOO_FEW_POINTS, _lib.FEW_ACTIVE, _lib.CAPACITY)

    def encode_batch(self, imgs, **kw):
        """encode of several images of any sizes at once (cniic_codec_encode_batch_var): a list of HxWx3 uint8 arrays -> a list of byte
        strings (None where that image's encode failed); last_stats: the list of their stats"""
        import numpy as np
        if len(imgs) == 0:
            return []
        buf, offs, ws, hs = self._packed(imgs)
        F = len(offs)
        data, stats = [None] * F, [None] * F
        todo = list(range(F))
        stride = (max(max(w * h for w, h in zip(ws, hs)) * 2, 1 << 16) + 3) & ~3   # a first guess; a frame that needs more says how much
        while todo:
            out = np.empty(stride * len(todo), np.uint8)
            rc, lens, rcs, sts = self.ctx.encode_batch_var(self.expr, buf, [offs[f] for f in todo], [ws[f] for f in todo], [hs[f] for f in todo],
                                                           out, stride, allow=self.ENCODE_FAILURES, **kw)
            again = []
            for j, f in enumerate(todo):
                stats[f] = sts[j]
                if rcs[j] == _lib.OK:
                    data[f] = out[j * stride:j * stride + lens[j]].tobytes()
                elif rcs[j] == _lib.CAPACITY and lens[j] > stride:
                    again.append((f, lens[j]))
            todo = [f for f, _ in again]
            stride = (max([n for _, n in again], default=0) + 3) & ~3
        self.last_stats = stats
        return data

    def measure(self, imgs, **kw):
        """bench::measure_all's loop over a list of images of any sizes (cniic_codec_measure_batch): a list of dicts with the reference's
        CSV columns compressed_size, compression_ratio, error (bench.rs:68-75) plus rc (and lossless_mismatch, kmeans)"""
        if len(imgs) == 0:
            return []
        buf, offs, ws, hs = self._packed(imgs)
        rc, rows, _ = self.ctx.measure_batch(self.expr, buf, offs, ws, hs, allow=self.ENCODE_FAILURES + (_lib.DECODE,), **kw)
        return rows

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


def rust_f64_expr(d):
    """an <f64> that Rust's f64::from_str (and cniic_codec_parse_f64) reads back as exactly d: repr ("4.0", "1e-07", "inf", "nan")"""
    return repr(float(d))


class HilbertRleApprox(Codec):
    """Hilbert { compress: RLE(d) } (src/codec/hilbertc.rs:12-98, rle_approx :200-299) for any f64 d: the codec of the expression
    hilbert(rle(<d>)), built from the float.  encode goes through cniic_hilbert_rle_approx_encode (the same bytes), everything else
    through the expression."""

    def __init__(self, d, ctx=None):
        self.d = float(d)
        self.expr = "hilbert(rle(%s))" % rust_f64_expr(self.d)
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


class HilbertZip(Codec):
    """Hilbert { compress: Zip } (src/codec/hilbertc.rs:27-29,47-49,67-77): the dimensions, then the dictionary coder over the 11-byte
    records of the pixels in scan order.  `hilbert(zip)` is not an expression of this library: encode and decode go through
    cniic_hilbert_zip_encode / cniic_hilbert_zip_decode."""

    def __init__(self, ctx=None):
        self.expr = None
        self._ctx = ctx
        self.last_stats = None

    def encode(self, img, **kw):
        rc, data = self.ctx.hilbert_zip_encode(img, **kw)
        return data

    def decode(self, data):
        rc, img = self.ctx.hilbert_zip_decode(data, allow=(_lib.DECODE,))
        return img if rc == _lib.OK else None

    def decode_batch(self, streams):
        return [self.decode(s) for s in streams]

    def encode_batch(self, imgs, **kw):
        return [self.encode(im, **kw) for im in imgs]

    def measure(self, imgs, **kw):
        raise NotImplementedError("hilbert-zip has no expression: cniic_codec_measure_batch cannot name it")

    def name(self):
        return "hilbert-zip"      # hilbertc.rs:85

    def is_lossless(self):
        return True               # :92


class ZipBack(Codec):
    """Zip::Back (src/codec/zipc.rs:14-48): the look-back coder (src/zip/back.rs) over the dimensions and the 11-byte records of the
    pixels, row by row.  `zip(back)` is not an expression of this library: encode and decode go through cniic_zip_back_image_encode /
    cniic_zip_back_image_decode, batches through cniic_zip_back_image_encode_batch_var / _decode_batch (one workgroup per image).
    encode raises CniicError(UNSUPPORTED) for an image on which the reference panics (a flat stretch of about 3000 pixels)."""

    def __init__(self, ctx=None):
        self.expr = None
        self._ctx = ctx
        self.last_stats = None

    def encode(self, img, **kw):
        rc, data = self.ctx.zip_back_image_encode(img, **kw)
        return data

    def decode(self, data):
        rc, img = self.ctx.zip_back_image_decode(data, allow=(_lib.DECODE,))
        return img if rc == _lib.OK else None

    def encode_batch(self, imgs):
        """the streams of a list of HxWx3 images of any sizes, in one call; None for an image that cannot be encoded"""
        imgs = [np.ascontiguousarray(im, np.uint8) for im in imgs]
        if not imgs:
            return []
        offs = np.concatenate([[0], np.cumsum([im.size for im in imgs])])[:-1]
        blob = np.concatenate([im.reshape(-1) for im in imgs]) if sum(im.size for im in imgs) else np.zeros(1, np.uint8)
        stride = max(14 * im.shape[0] * im.shape[1] + 32 for im in imgs)
        out = np.empty(stride * len(imgs), np.uint8)
        rc, lens, rcs = self.ctx.zip_back_encode_batch_var(blob, offs, [im.shape[1] for im in imgs], [im.shape[0] for im in imgs], out, stride,
                                                           allow=(_lib.UNSUPPORTED,))
        return [out[f * stride:f * stride + lens[f]].tobytes() if rcs[f] == _lib.OK else None for f in range(len(imgs))]

    def decode_batch(self, streams):
        """the images of a list of streams, in one call; None where a stream does not decode"""
        streams = [bytes(s) for s in streams]
        if not streams:
            return []
        dims = [_lib.zip_back_dims(s) for s in streams]
        stride = max(max(len(s) for s in streams), 1)
        img_stride = max([3 * d[0] * d[1] for d in dims if d is not None and d[0] * d[1] <= (1 << 28)] + [1])
        blob = np.zeros(stride * len(streams), np.uint8)
        for f, s in enumerate(streams):
            blob[f * stride:f * stride + len(s)] = np.frombuffer(s, np.uint8)
        out = np.zeros(img_stride * len(streams), np.uint8)
        rc, ws, hs, rcs = self.ctx.zip_back_decode_batch(blob, stride, [len(s) for s in streams], len(streams), out, img_stride,
                                                         allow=(_lib.DECODE, _lib.CAPACITY))
        return [out[f * img_stride:f * img_stride + 3 * ws[f] * hs[f]].reshape(hs[f], ws[f], 3).copy() if rcs[f] == _lib.OK else None
                for f in range(len(streams))]

    def measure(self, imgs, **kw):
        raise NotImplementedError("zip-back has no expression: cniic_codec_measure_batch cannot name it")

    def name(self):
        return "zip-back"         # zipc.rs:53

    def is_lossless(self):
        return True               # :57-59
