"""The numpy restatement of cniic_frames_from_surfaces / cniic_frames_to_surfaces (include/cniic_hip.h): int64 arithmetic and
np.floor_divide for NV12's integer matrices, fancy indexing for the pitched rows.  Also here: the layout helper the surface tests and
tools/surface_probe.py share (surfaces placed at chosen residues with guard bytes between them)."""
import numpy as np

from cniic_amd import _lib
from cniic_amd._lib import PX_BGR8, PX_BGRA8, PX_BYTES, PX_L8, PX_LA8, PX_NV12, PX_RGB8, PX_RGBA8, Surface  # noqa: F401

POISON = 0xA5
# matrix -> (what Y loses, Y's factor, R's E, G's D, G's E, B's D): the header's table
YUV = {_lib.YUV_601_LIMITED: (16, 298, 409, -100, -208, 516), _lib.YUV_709_LIMITED: (16, 298, 459, -55, -136, 541),
       _lib.YUV_601_FULL: (0, 256, 359, -88, -183, 454), _lib.YUV_709_FULL: (0, 256, 403, -48, -120, 475)}
MATRICES = sorted(YUV)
Y_VALUES, C_VALUES = (0, 16, 17, 128, 235, 255), (0, 16, 128, 240, 255)


def yuv_unclipped(Y, U, V, matrix):
    """-> int64 (..., 3): the table's R, G, B before the clip"""
    ysub, cy, rv, gu, gv, bu = YUV[matrix]
    C, D, E = np.asarray(Y, np.int64) - ysub, np.asarray(U, np.int64) - 128, np.asarray(V, np.int64) - 128
    return np.stack([np.floor_divide(cy * C + rv * E + 128, 256), np.floor_divide(cy * C + gu * D + gv * E + 128, 256),
                     np.floor_divide(cy * C + bu * D + 128, 256)], axis=-1)


def yuv_to_rgb(Y, U, V, matrix):
    return np.clip(yuv_unclipped(Y, U, V, matrix), 0, 255).astype(np.uint8)


def rows(buf, off, pitch, row_bytes, h):
    """the index of every byte of h rows of row_bytes bytes, `pitch` apart, from `off` on: int64 (h, row_bytes)"""
    return int(off) + np.arange(h, dtype=np.int64)[:, None] * int(pitch) + np.arange(row_bytes, dtype=np.int64)[None, :]


def import_surface(buf, s):
    """surface s of the uint8 buffer buf -> uint8 (h, w, 3)"""
    w, h, fmt = int(s.w), int(s.h), int(s.format)
    if fmt == PX_NV12:
        Y = buf[rows(buf, s.off, s.pitch, w, h)]
        uv = buf[rows(buf, s.off_uv, s.pitch_uv, 2 * ((w + 1) // 2), (h + 1) // 2)]
        yy, xx = np.arange(h)[:, None] >> 1, np.arange(w)[None, :] >> 1
        return yuv_to_rgb(Y, uv[yy, 2 * xx], uv[yy, 2 * xx + 1], int(s.matrix))
    bpp = PX_BYTES[fmt]
    px = buf[rows(buf, s.off, s.pitch, w * bpp, h)].reshape(h, w, bpp)
    if fmt in (PX_L8, PX_LA8):
        return np.repeat(px[:, :, :1], 3, axis=2)
    return px[:, :, :3] if fmt in (PX_RGB8, PX_RGBA8) else px[:, :, 2::-1]


def export_surface(dst, s, rgb, alpha):
    """uint8 (h, w, 3) -> surface s of the uint8 buffer dst, in place; nothing else of dst changes"""
    w, h, fmt = int(s.w), int(s.h), int(s.format)
    bpp = PX_BYTES[fmt]
    px = np.empty((h, w, bpp), np.uint8)
    px[:, :, :3] = rgb if fmt in (PX_RGB8, PX_RGBA8) else rgb[:, :, ::-1]
    if bpp == 4:
        px[:, :, 3] = alpha
    dst[rows(dst, s.off, s.pitch, w * bpp, h)] = px.reshape(h, w * bpp)


def nv12_cross_product():
    """-> (Y plane (6, 50), UV plane (3, 50)): every Y of Y_VALUES against every (U, V) of C_VALUES x C_VALUES"""
    Y = np.repeat(np.array(Y_VALUES, np.uint8)[:, None], 50, axis=1)
    pairs = np.array([(u, v) for u in C_VALUES for v in C_VALUES], np.uint8)
    return Y, np.repeat(pairs.reshape(1, 50), 3, axis=0)


def at_residue(cursor, residue):
    """the first address >= cursor that is `residue` behind a multiple of 16"""
    return cursor + (residue - cursor) % 16


def span(s):
    got = _lib.surface_span(s)
    assert got is not None, "bad descriptor in a layout"
    return got


class Layout:
    """Surfaces and their packed frames laid out one behind the other, each at a chosen residue with `guard` bytes between two
    neighbours; sizes from cniic_surface_span."""

    def __init__(self, guard=16):
        self.guard, self.surfaces, self.img_off, self.src_bytes, self.rgb_bytes = guard, [], [], guard, guard

    def add(self, fmt, w, h, pad=0, src_res=0, rgb_res=0, matrix=0, pad_uv=0, uv_res=0):
        s = Surface(w=w, h=h, format=fmt, matrix=matrix)
        s.pitch = w * PX_BYTES[fmt] + pad
        s.off = at_residue(self.src_bytes, src_res)
        if fmt == PX_NV12:
            s.pitch_uv = 2 * ((w + 1) // 2) + pad_uv
            s.off_uv = at_residue(s.off + (h - 1) * s.pitch + w + self.guard, uv_res)
        end, nb = span(s)
        self.src_bytes = end + self.guard
        self.surfaces.append(s)
        self.img_off.append(at_residue(self.rgb_bytes, rgb_res))
        self.rgb_bytes = self.img_off[-1] + nb + self.guard
        return s

    def random_source(self, seed):
        """a source buffer: poison, the bytes of every surface's rows random"""
        rng = np.random.default_rng(seed)
        buf = np.full(self.src_bytes, POISON, np.uint8)
        for s in self.surfaces:
            idx = rows(buf, s.off, s.pitch, s.w * PX_BYTES[s.format], s.h)
            buf[idx] = rng.integers(0, 256, idx.shape, dtype=np.uint8)
            if s.format == PX_NV12:
                idx = rows(buf, s.off_uv, s.pitch_uv, 2 * ((s.w + 1) // 2), (s.h + 1) // 2)
                buf[idx] = rng.integers(0, 256, idx.shape, dtype=np.uint8)
        return buf

    def expected_import(self, src):
        out = np.full(self.rgb_bytes, POISON, np.uint8)
        for s, o in zip(self.surfaces, self.img_off):
            out[o:o + 3 * s.w * s.h] = import_surface(src, s).ravel()
        return out

    def expected_export(self, rgb, alpha):
        out = np.full(self.src_bytes, POISON, np.uint8)
        for s, o in zip(self.surfaces, self.img_off):
            export_surface(out, s, rgb[o:o + 3 * s.w * s.h].reshape(s.h, s.w, 3), alpha)
        return out

    def random_frames(self, seed):
        rng = np.random.default_rng(seed)
        buf = np.full(self.rgb_bytes, POISON, np.uint8)
        for s, o in zip(self.surfaces, self.img_off):
            buf[o:o + 3 * s.w * s.h] = rng.integers(0, 256, 3 * s.w * s.h, dtype=np.uint8)
        return buf
