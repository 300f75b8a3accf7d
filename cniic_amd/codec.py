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
    cniic_hilbert_zip_encode / cniic_hilbert_zip_decode, batches and measure through cniic_hilbert_zip_encode_batch_var / _decode_batch /
    _measure_batch."""

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

    DECODE_BATCH_BYTES = 256 << 20   # host memory one cniic_hilbert_zip_decode_batch call's images may take (a frame that claims more goes alone)

    def encode_batch(self, imgs, allow=(), **kw):
        """the streams of a list of HxWx3 images of any sizes, in one call (cniic_hilbert_zip_encode_batch_var); None for an image that
        cannot be encoded.  The per-image options of encode (w, h, out) make a loop of single calls, as before."""
        if len(imgs) == 0:
            return []
        if kw:
            return [self.encode(im, allow=allow, **kw) for im in imgs]
        buf, offs, ws, hs = self._packed(imgs)
        stride = (max(8 + 22 * w * h + 4 for w, h in zip(ws, hs)) + 3) & ~3   # (two symbols a byte of text at most)
        out = np.empty(stride * len(offs), np.uint8)
        rc, lens, rcs = self.ctx.hilbert_zip_encode_batch_var(buf, offs, ws, hs, out, stride, allow=self.ENCODE_FAILURES + tuple(allow))
        return [out[f * stride:f * stride + lens[f]].tobytes() if rcs[f] == _lib.OK else None for f in range(len(offs))]

    def decode_batch(self, streams):
        """the images of a list of streams (cniic_hilbert_zip_decode_batch); None where a stream does not decode.  The sizes are what the
        streams claim, so the list goes in calls whose images take at most DECODE_BATCH_BYTES of host memory together, smallest claims
        first; a stream that claims more than that on its own is decoded alone (one image's allocation, as the single call makes)."""
        streams = [bytes(s) for s in streams]
        if not streams:
            return []

        def claim(s):   # bytes of the image the stream's dimensions ask for; 1 where they ask for none that can be decoded
            if len(s) < 8:
                return 1
            n = int.from_bytes(s[0:4], "little") * int.from_bytes(s[4:8], "little")
            return 3 * n if 0 < n <= (1 << 28) else 1

        imgs = [None] * len(streams)
        order = sorted(range(len(streams)), key=lambda f: claim(streams[f]))
        at = 0
        while at < len(order):
            img_stride = claim(streams[order[at]])
            if img_stride > self.DECODE_BATCH_BYTES:
                imgs[order[at]] = self.decode(streams[order[at]])
                at += 1
                continue
            end = at + 1
            while end < len(order) and claim(streams[order[end]]) * (end + 1 - at) <= self.DECODE_BATCH_BYTES:
                end += 1
            part = [streams[f] for f in order[at:end]]
            img_stride = claim(part[-1])
            stride = max(max(len(s) for s in part), 1)
            blob = np.zeros(stride * len(part), np.uint8)
            for j, s in enumerate(part):
                blob[j * stride:j * stride + len(s)] = np.frombuffer(s, np.uint8)
            out = np.zeros(img_stride * len(part), np.uint8)
            rc, ws, hs, rcs = self.ctx.hilbert_zip_decode_batch(blob, stride, [len(s) for s in part], len(part), out, img_stride,
                                                                allow=(_lib.DECODE, _lib.CAPACITY))
            for j, f in enumerate(order[at:end]):
                if rcs[j] == _lib.OK:
                    imgs[f] = out[j * img_stride:j * img_stride + 3 * ws[j] * hs[j]].reshape(hs[j], ws[j], 3).copy()
            at = end
        return imgs

    def measure(self, imgs, seed=0, max_iters=0, flags=0, allow=()):
        """bench::measure_all's loop over a list of images of any sizes (cniic_hilbert_zip_measure_batch): a list of dicts with the
        reference's CSV columns compressed_size, compression_ratio, error (bench.rs:68-75) plus rc (and lossless_mismatch, kmeans).
        seed, max_iters and flags are Codec.measure's K-means options: taken, and without meaning for this codec."""
        if len(imgs) == 0:
            return []
        buf, offs, ws, hs = self._packed(imgs)
        rc, rows, _ = self.ctx.hilbert_zip_measure_batch(buf, offs, ws, hs, allow=self.ENCODE_FAILURES + (_lib.DECODE,) + tuple(allow))
        return rows

    def name(self):
        return "hilbert-zip"      # hilbertc.rs:85

    def is_lossless(self):
        return True               # :92


class ZipBack(Codec):
    """Zip::Back (src/codec/zipc.rs:14-48): the look-back coder (src/zip/back.rs) over the dimensions and the 11-byte records of the
    pixels, row by row.  `zip(back)` is not an expression of this library: encode and decode go through cniic_zip_back_image_encode /
    cniic_zip_back_image_decode, batches through cniic_zip_back_image_encode_batch_var / _decode_batch (one workgroup per image),
    measure through cniic_zip_back_image_measure_batch.
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

    def measure(self, imgs, seed=0, max_iters=0, flags=0, allow=()):
        """bench::measure_all's loop over a list of images of any sizes in ONE call (cniic_zip_back_image_measure_batch): a list of dicts
        with the reference's CSV columns compressed_size, compression_ratio, error (bench.rs:68-75) plus rc (and lossless_mismatch,
        kmeans).  seed, max_iters and flags are Codec.measure's K-means options: taken, and without meaning for this codec."""
        if len(imgs) == 0:
            return []
        buf, offs, ws, hs = self._packed(imgs)
        rc, rows, _ = self.ctx.zip_back_measure_batch(buf, offs, ws, hs, allow=(_lib.BAD_ARG, _lib.UNSUPPORTED, _lib.DECODE) + tuple(allow))
        return rows

    def name(self):
        return "zip-back"         # zipc.rs:53

    def is_lossless(self):
        return True               # :57-59
