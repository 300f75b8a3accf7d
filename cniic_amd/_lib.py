"""ctypes loader + thin wrappers of libcniic_hip.so (the C ABI of include/cniic_hip.h).

There is NO fallback: if the HIP extension is missing or no GPU is usable the calls raise.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))

OK = 0
ERR = {-1: "BAD_ARG", -2: "TOO_FEW_POINTS", -3: "FEW_ACTIVE", -4: "HIP", -5: "RCCL", -6: "DECODE", -7: "NOMEM",
       -8: "CAPACITY", -9: "UNSUPPORTED"}
BAD_ARG, TOO_FEW_POINTS, FEW_ACTIVE, HIP, RCCL, DECODE, NOMEM, CAPACITY, UNSUPPORTED = range(-1, -10, -1)
SYM_RGB, SYM_SIGNED = 1, 2
KIND_ZIP_DICT = 6   # cniic_codec_parse's kind of zip(dict)
SYNTH_UNIFORM, SYNTH_PHOTO = 0, 1
KM_BRUTE_FORCE, KM_PROFILE, KM_NO_SKIP = 1, 2, 4
LIN_RECT, LIN_SMALL, LIN_LARGE = 0, 1, 2
LIN_METHODS = {"rect": LIN_RECT, "small": LIN_SMALL, "large": LIN_LARGE}   # hilbert.rs:10-32
PX_L8, PX_LA8, PX_RGB8, PX_RGBA8, PX_BGR8, PX_BGRA8, PX_NV12 = range(1, 8)
PX_BYTES = {PX_L8: 1, PX_LA8: 2, PX_RGB8: 3, PX_RGBA8: 4, PX_BGR8: 3, PX_BGRA8: 4, PX_NV12: 1}   # per pixel (NV12: of the Y plane)
YUV_601_LIMITED, YUV_601_FULL, YUV_709_LIMITED, YUV_709_FULL = range(1, 5)
OPT_SP_MIN_PIXELS, OPT_HUF_GPU_CODES_MIN, OPT_GPU_DECODE_MIN, OPT_DELTA_ROUTE, OPT_STAGE_TIMERS, OPT_FRAME_TREES_HOST, OPT_BATCH_STREAMS, OPT_KM_MAX_BLOCKS, OPT_KM_LOOP = range(1, 10)

# every symbol include/cniic_hip.h declares (checked by tests/test_abi.py)
SYMBOLS = [
    "cniic_ctx_create", "cniic_ctx_destroy", "cniic_last_error", "cniic_version", "cniic_is_testing_build", "cniic_sync", "cniic_dev_alloc",
    "cniic_dev_free", "cniic_memcpy", "cniic_ctx_set_opt", "cniic_ctx_unset_opt", "cniic_ctx_get_opt", "cniic_ctx_set_scan", "cniic_last_kernel_time", "cniic_hist_rgb24", "cniic_hist_syms",
    "cniic_kmeans_rgbw", "cniic_kmeans_xyrgb", "cniic_kmeans_step_rgbw", "cniic_kmeans_step_xyrgb",
    "cniic_km_create_rgbw", "cniic_km_partial_words", "cniic_km_partials", "cniic_km_begin",
    "cniic_km_labels_internal", "cniic_km_assign", "cniic_km_update",
    "cniic_km_result", "cniic_km_time_assign", "cniic_km_destroy", "cniic_hist_rgb24_dense", "cniic_cc_create",
    "cniic_cc_unique", "cniic_cc_label_bytes", "cniic_cc_partials", "cniic_cc_assign", "cniic_cc_update", "cniic_cc_poll", "cniic_cc_poll_lagged",
    "cniic_cc_export_labels", "cniic_cc_import_labels", "cniic_cc_finish", "cniic_cc_finish_frames", "cniic_cc_destroy", "cniic_comm_unique_id",
    "cniic_comm_create", "cniic_comm_create_host", "cniic_comm_create_mailbox", "cniic_comm_connect_mailbox", "cniic_comm_destroy", "cniic_comm_all_reduce", "cniic_comm_set_timeout", "cniic_cc_run", "cniic_occupancy_pack",
    "cniic_cc_create_local", "cniic_cc_image_begin", "cniic_cc_image_occupancy", "cniic_cc_image_create", "cniic_remap_rgb", "cniic_hilbert_xy",
    "cniic_hilbert_linearize", "cniic_hilbert_delta", "cniic_hilbert_delta_hist", "cniic_huf_encode_all",
    "cniic_huf_size", "cniic_codec_parse", "cniic_codec_name", "cniic_codec_is_lossless", "cniic_codec_encode",
    "cniic_codec_encode_opts", "cniic_codec_encode_batch", "cniic_codec_decode", "cniic_codec_decode_batch", "cniic_mse", "cniic_mse_batch",
    "cniic_hilbert_rle_approx_encode", "cniic_synth_image",
    "cniic_codec_encode_batch_var", "cniic_mse_batch_var", "cniic_codec_measure_batch", "cniic_codec_parse_f64",
    "cniic_zip_dict_encode", "cniic_zip_dict_decode", "cniic_zip_dict_dims", "cniic_hilbert_zip_encode", "cniic_hilbert_zip_decode",
    "cniic_zip_back_encode", "cniic_zip_back_decode", "cniic_zip_back_dims", "cniic_zip_back_image_encode", "cniic_zip_back_image_decode",
    "cniic_zip_back_image_encode_batch_var", "cniic_zip_back_image_decode_batch",
    "cniic_hilbert_linearize_count", "cniic_hilbert_linearize_as", "cniic_channel_diff_hist",
    "cniic_cc_finish_frames_var",
    "cniic_cc_palette", "cniic_palette_create", "cniic_palette_destroy", "cniic_palette_label_bytes", "cniic_palette_labels",
    "cniic_palette_encode_frames_var",
    "cniic_kmeans_rgbw_from", "cniic_kmeans_xyrgb_from", "cniic_cc_set_centroids", "cniic_codec_encode_warm", "cniic_palette_fit_frames_var",
    "cniic_surface_span", "cniic_frames_from_surfaces", "cniic_frames_to_surfaces",
]


class CniicError(RuntimeError):
    def __init__(self, code, msg=""):
        self.code = code
        super().__init__("cniic error %d (%s): %s" % (code, ERR.get(code, "?"), msg))


class KmOpts(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("max_iters", C.c_uint64), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class KmStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("iterations", "moved_last", "empty_reseeds", "active", "pair_evals")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class MeasureRow(C.Structure):
    """cniic_measure_row: one row of bench::measure_all's CSV (bench.rs:68-75) + status"""
    _fields_ = [("compressed_size", C.c_uint64), ("compression_ratio", C.c_double), ("error", C.c_double), ("rc", C.c_int32),
                ("lossless_mismatch", C.c_uint32), ("kmeans", KmStats)]

    def as_dict(self):
        return dict(compressed_size=int(self.compressed_size), compression_ratio=float(self.compression_ratio), error=float(self.error),
                    rc=int(self.rc), lossless_mismatch=int(self.lossless_mismatch), kmeans=self.kmeans.as_dict())


class Surface(C.Structure):
    """cniic_surface: one pitched surface inside a larger buffer (offsets in bytes from the buffer's first byte)"""
    _fields_ = [("off", C.c_uint64), ("pitch", C.c_uint64), ("off_uv", C.c_uint64), ("pitch_uv", C.c_uint64), ("w", C.c_uint32), ("h", C.c_uint32),
                ("format", C.c_int32), ("matrix", C.c_int32)]


COLORPOS = np.dtype([("x", "<u4"), ("y", "<u4"), ("rgb", "u1", (3,)), ("pad", "u1")])


def lib_path():
    """libcniic_hip.so -- or, with CNIIC_USE_TESTING_LIB=1 (tests/conftest.py, tools/), libcniic_hip_testing.so: the same code built with
    -DCNIIC_TESTING, the only build in which the CNIIC_TEST_* / CNIIC_DBG_* / route-forcing environment knobs exist"""
    name = "libcniic_hip_testing.so" if os.environ.get("CNIIC_USE_TESTING_LIB") == "1" else "libcniic_hip.so"
    if os.environ.get("CNIIC_LIB_FILE"):   # a library built beside the shipped ones (another name in cniic_amd/), never a product path
        name = os.environ["CNIIC_LIB_FILE"]
    return os.path.join(_HERE, name)


_lib = None


HOST_SUM_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32)   # cniic_host_sum_fn


def lib():
    """Load libcniic_hip.so; raise loudly if it has not been built (no CPU fallback exists)."""
    global _lib
    if _lib is None:
        p = lib_path()
        if not os.path.exists(p):
            raise ImportError("%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                              "or `make -C cniic_amd/csrc` (hipcc --offload-arch=gfx950)" % p)
        L = C.CDLL(p)
        L.cniic_last_error.restype = C.c_char_p
        L.cniic_last_error.argtypes = [C.c_void_p]
        L.cniic_km_partial_words.restype = C.c_uint64
        L.cniic_km_partial_words.argtypes = [C.c_uint32, C.c_uint32]
        L.cniic_ctx_destroy.restype = None
        L.cniic_ctx_destroy.argtypes = [C.c_void_p]
        L.cniic_km_destroy.restype = None
        L.cniic_km_destroy.argtypes = [C.c_void_p]
        L.cniic_cc_destroy.restype = None
        L.cniic_cc_destroy.argtypes = [C.c_void_p]
        L.cniic_comm_destroy.restype = None
        L.cniic_comm_destroy.argtypes = [C.c_void_p]
        L.cniic_cc_unique.restype = C.c_uint64
        L.cniic_cc_unique.argtypes = [C.c_void_p]
        L.cniic_cc_label_bytes.restype = C.c_uint32
        L.cniic_cc_label_bytes.argtypes = [C.c_void_p]
        L.cniic_cc_finish_frames_var.restype = C.c_int32
        L.cniic_cc_finish_frames_var.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint32, C.c_void_p, C.c_uint64,
                                                 C.POINTER(C.c_uint64), C.c_void_p]
        if hasattr(L, "cniic_cc_palette"):   # (CNIIC_LIB_FILE may name an older build of the library, for a comparison: it has no palettes)
            _palette_prototypes(L)
        if hasattr(L, "cniic_cc_set_centroids"):   # (likewise: K-means from given centroids, the fit of a handle)
            _warm_prototypes(L)
        if hasattr(L, "cniic_surface_span"):   # (likewise: surfaces)
            _surface_prototypes(L)
        _lib = L
    return _lib


def _palette_prototypes(L):
    L.cniic_cc_palette.restype = C.c_int32
    L.cniic_cc_palette.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.cniic_palette_create.restype = C.c_int32
    L.cniic_palette_create.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]
    L.cniic_palette_destroy.restype = None
    L.cniic_palette_destroy.argtypes = [C.c_void_p]
    L.cniic_palette_label_bytes.restype = C.c_uint32
    L.cniic_palette_label_bytes.argtypes = [C.c_void_p]
    L.cniic_palette_labels.restype = C.c_int32
    L.cniic_palette_labels.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    L.cniic_palette_encode_frames_var.restype = C.c_int32
    L.cniic_palette_encode_frames_var.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint32, C.c_void_p, C.c_uint64,
                                                  C.POINTER(C.c_uint64)]


def _warm_prototypes(L):
    L.cniic_cc_set_centroids.restype = C.c_int32
    L.cniic_cc_set_centroids.argtypes = [C.c_void_p, C.c_void_p]
    L.cniic_palette_fit_frames_var.restype = C.c_int32
    L.cniic_palette_fit_frames_var.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint32, C.c_void_p, C.c_void_p]
    L.cniic_codec_encode_warm.restype = C.c_int32
    L.cniic_codec_encode_warm.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64,
                                          C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p]


def _surface_prototypes(L):
    L.cniic_surface_span.restype = C.c_int32
    L.cniic_surface_span.argtypes = [C.POINTER(Surface), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.cniic_frames_from_surfaces.restype = C.c_int32
    L.cniic_frames_from_surfaces.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Surface), C.c_uint32, C.c_void_p, C.POINTER(C.c_uint64)]
    L.cniic_frames_to_surfaces.restype = C.c_int32
    L.cniic_frames_to_surfaces.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(Surface), C.c_uint32, C.c_void_p, C.c_uint32]


def _ptr(x):
    """numpy array (host) / torch tensor (device or host) / int address / None -> c_void_p"""
    if x is None:
        return C.c_void_p(0)
    if isinstance(x, np.ndarray):
        assert x.flags["C_CONTIGUOUS"]
        return C.c_void_p(x.ctypes.data)
    if hasattr(x, "data_ptr"):
        assert x.is_contiguous()
        return C.c_void_p(x.data_ptr())
    if isinstance(x, (bytes, bytearray)):
        return C.cast(C.c_char_p(bytes(x)), C.c_void_p)
    return C.c_void_p(int(x))


class Context:
    """One cniic_ctx: a HIP stream + scratch HBM on one GPU.  Not shared between threads."""

    def __init__(self, device=0, stream=None):
        """stream: a hipStream_t handle to enqueue on (e.g. torch.cuda.current_stream().cuda_stream of a
        NON-default torch stream), or None for a private stream.  The NULL/default stream has handle 0
        and cannot be shared this way: make a torch.cuda.Stream() current first."""
        if stream is not None and int(stream) == 0:
            raise ValueError("cannot share the default (NULL) stream: use torch.cuda.set_stream(torch.cuda.Stream()) first")
        self._L = lib()
        h = C.c_void_p()
        rc = self._L.cniic_ctx_create(C.c_int32(device), C.c_void_p(stream or 0), C.byref(h))
        if rc != OK:
            raise CniicError(rc, "cniic_ctx_create(device=%d) failed: no usable gfx950 device?" % device)
        self.h = h
        self.device = device

    def close(self):
        if getattr(self, "h", None):
            self._L.cniic_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc, allow=()):
        if rc != OK and rc not in allow:
            raise CniicError(rc, (self._L.cniic_last_error(self.h) or b"").decode())
        return rc

    def set_opt(self, opt, value):
        """cniic_ctx_set_opt: a route switch / threshold for this context (value None: back to the environment's / the default)"""
        if value is None:
            self._check(self._L.cniic_ctx_unset_opt(self.h, C.c_int32(opt)))
        else:
            self._check(self._L.cniic_ctx_set_opt(self.h, C.c_int32(opt), C.c_uint64(value)))

    def set_scan(self, w, h, xy):
        """cniic_ctx_set_scan: inject the scan of w x h images (xy: (w h, 2) uint32 positions, or None for the built-in one)"""
        if xy is not None and isinstance(xy, np.ndarray):
            xy = np.ascontiguousarray(xy, np.uint32)
        self._check(self._L.cniic_ctx_set_scan(self.h, C.c_uint32(w), C.c_uint32(h), _ptr(xy)))

    def get_opt(self, opt):
        v = C.c_uint64(0)
        self._check(self._L.cniic_ctx_get_opt(self.h, C.c_int32(opt), C.byref(v)))
        return v.value

    def sync(self):
        self._check(self._L.cniic_sync(self.h))

    def kernel_time(self, which):
        ms, n = C.c_double(0), C.c_uint64(0)
        rc = self._L.cniic_last_kernel_time(self.h, which.encode(), C.byref(ms), C.byref(n))
        return (ms.value, n.value) if rc == OK else (0.0, 0)

    # ---- H1
    def hist_rgb24(self, rgb, npx=None):
        npx = int(npx if npx is not None else rgb.size // 3) if not hasattr(rgb, "numel") else int(npx or rgb.numel() // 3)
        nu = C.c_uint64(0)
        self._check(self._L.cniic_hist_rgb24(self.h, _ptr(rgb), C.c_uint64(npx), None, None, C.c_uint64(0), C.byref(nu)))
        keys = np.empty(max(nu.value, 1), np.uint32)
        counts = np.empty(max(nu.value, 1), np.uint64)
        self._check(self._L.cniic_hist_rgb24(self.h, _ptr(rgb), C.c_uint64(npx), _ptr(keys), _ptr(counts),
                                             C.c_uint64(keys.size), C.byref(nu)))
        return keys[:nu.value], counts[:nu.value]

    def hist_syms(self, kind, syms):
        syms = np.ascontiguousarray(syms, np.uint32)
        nu = C.c_uint64(0)
        self._check(self._L.cniic_hist_syms(self.h, kind, _ptr(syms), C.c_uint64(syms.size), None, None, C.c_uint64(0), C.byref(nu)))
        keys = np.empty(max(nu.value, 1), np.uint32)
        counts = np.empty(max(nu.value, 1), np.uint64)
        self._check(self._L.cniic_hist_syms(self.h, kind, _ptr(syms), C.c_uint64(syms.size), _ptr(keys), _ptr(counts),
                                            C.c_uint64(keys.size), C.byref(nu)))
        return keys[:nu.value], counts[:nu.value]

    # ---- K-means
    @staticmethod
    def _opts(seed=0, max_iters=0, flags=0):
        return KmOpts(seed, max_iters, flags, 0)

    def kmeans_rgbw(self, keys, weight, K, seed=0, max_iters=0, flags=0, allow=(), init=None):
        """init: None (init_centroids, kmeans.rs:101-108), or (K, 3) uint8 centroids to start from (cniic_kmeans_rgbw_from)"""
        keys = np.ascontiguousarray(keys, np.uint32)
        weight = np.ascontiguousarray(weight, np.uint32)
        U = keys.size
        cent = np.zeros((K, 3), np.uint8)
        labels = np.zeros(U, np.uint32)
        members = np.zeros(K, np.uint64)
        st = KmStats()
        o = self._opts(seed, max_iters, flags)
        if init is None:
            rc = self._L.cniic_kmeans_rgbw(self.h, _ptr(keys), _ptr(weight), C.c_uint64(U), C.c_uint32(K), C.byref(o),
                                           _ptr(cent), _ptr(labels), _ptr(members), C.byref(st))
        else:
            init = np.ascontiguousarray(init, np.uint8).reshape(K, 3)
            rc = self._L.cniic_kmeans_rgbw_from(self.h, _ptr(keys), _ptr(weight), C.c_uint64(U), C.c_uint32(K), C.byref(o), _ptr(init),
                                                _ptr(cent), _ptr(labels), _ptr(members), C.byref(st))
        rc = self._check(rc, allow)
        return rc, dict(centroids=cent, labels=labels, members=members, stats=st.as_dict())

    def kmeans_step_rgbw(self, keys, weight, K, centroids, labels):
        keys = np.ascontiguousarray(keys, np.uint32)
        weight = np.ascontiguousarray(weight, np.uint32)
        cent = np.ascontiguousarray(centroids, np.uint8).reshape(K, 3)
        labels = np.array(labels, np.uint32, copy=True)
        sums = np.zeros((K, 3), np.uint64)
        wsum = np.zeros(K, np.uint64)
        members = np.zeros(K, np.uint64)
        ch = C.c_uint64(0)
        self._check(self._L.cniic_kmeans_step_rgbw(self.h, _ptr(keys), _ptr(weight), C.c_uint64(keys.size), C.c_uint32(K),
                                                   _ptr(cent), _ptr(labels), _ptr(sums), _ptr(wsum), _ptr(members), C.byref(ch)))
        return dict(labels=labels, sums=sums, wsum=wsum, members=members, changed=ch.value)

    def kmeans_xyrgb(self, img, K, seed=0, max_iters=0, flags=0, want_labels=True, allow=(), init=None):
        """init: None (init_centroids, kmeans.rs:101-108), or K COLORPOS centroids inside the image to start from (cniic_kmeans_xyrgb_from)"""
        img = np.ascontiguousarray(img, np.uint8)
        h, w = img.shape[:2]
        cent = np.zeros(K, COLORPOS)
        labels = np.zeros(h * w, np.uint32) if want_labels else None
        members = np.zeros(K, np.uint64)
        st = KmStats()
        o = self._opts(seed, max_iters, flags)
        if init is None:
            rc = self._L.cniic_kmeans_xyrgb(self.h, _ptr(img), C.c_uint32(w), C.c_uint32(h), C.c_uint32(K), C.byref(o),
                                            _ptr(cent), _ptr(labels), _ptr(members), C.byref(st))
        else:
            init = np.ascontiguousarray(init, COLORPOS).reshape(K)
            rc = self._L.cniic_kmeans_xyrgb_from(self.h, _ptr(img), C.c_uint32(w), C.c_uint32(h), C.c_uint32(K), C.byref(o), _ptr(init),
                                                 _ptr(cent), _ptr(labels), _ptr(members), C.byref(st))
        rc = self._check(rc, allow)
        return rc, dict(centroids=cent, labels=labels, members=members, stats=st.as_dict())

    def kmeans_step_xyrgb(self, img, K, centroids, labels):
        img = np.ascontiguousarray(img, np.uint8)
        h, w = img.shape[:2]
        cent = np.ascontiguousarray(centroids, COLORPOS)
        labels = np.array(labels, np.uint32, copy=True)
        sums = np.zeros((K, 5), np.uint64)
        wsum = np.zeros(K, np.uint64)
        members = np.zeros(K, np.uint64)
        ch = C.c_uint64(0)
        self._check(self._L.cniic_kmeans_step_xyrgb(self.h, _ptr(img), C.c_uint32(w), C.c_uint32(h), C.c_uint32(K), _ptr(cent),
                                                    _ptr(labels), _ptr(sums), _ptr(wsum), _ptr(members), C.byref(ch)))
        return dict(labels=labels, sums=sums, wsum=wsum, members=members, changed=ch.value)

    def remap_rgb(self, img, keys, labels, centroids):
        img = np.ascontiguousarray(img, np.uint8)
        keys = np.ascontiguousarray(keys, np.uint32)
        labels = np.ascontiguousarray(labels, np.uint32)
        cent = np.ascontiguousarray(centroids, np.uint8)
        out = np.empty_like(img)
        self._check(self._L.cniic_remap_rgb(self.h, _ptr(img), C.c_uint64(img.size // 3), _ptr(keys), _ptr(labels),
                                            C.c_uint64(keys.size), _ptr(cent), C.c_uint32(cent.shape[0]), _ptr(out)))
        return out

    # ---- Hilbert
    def hilbert_xy(self, w, h):
        xy = np.zeros((max(w * h, 1), 2), np.uint32)
        self._check(self._L.cniic_hilbert_xy(self.h, C.c_uint32(w), C.c_uint32(h), _ptr(xy)))
        return xy[:w * h]

    def hilbert_linearize(self, img):
        img = np.ascontiguousarray(img, np.uint8)
        h, w = img.shape[:2]
        out = np.empty((h * w, 3), np.uint8)
        self._check(self._L.cniic_hilbert_linearize(self.h, _ptr(img), C.c_uint32(w), C.c_uint32(h), _ptr(out)))
        return out

    def hilbert_linearize_as(self, img, method, w=None, h=None, out=None, allow=()):
        """cniic_hilbert_linearize_as: method "rect" | "small" | "large" (or a CNIIC_LIN_* number).  img: HxWx3 uint8 numpy array, or a
        device tensor / address with w, h given.  -> the (npx, 3) pixels when out is None, else (rc, npx) with out (numpy array, device
        tensor) filled; with CAPACITY allowed: npx = the pixels needed"""
        if isinstance(img, np.ndarray):
            img = np.ascontiguousarray(img, np.uint8)
            h, w = img.shape[:2]
        m = LIN_METHODS[method] if isinstance(method, str) else int(method)
        own = out is None
        if own:
            out = np.empty((max(linearize_count(m, w, h), 1), 3), np.uint8)
        cap = (out.numel() if hasattr(out, "numel") else out.size) // 3
        n = C.c_uint64(0)
        rc = self._check(self._L.cniic_hilbert_linearize_as(self.h, C.c_int32(m), _ptr(img), C.c_uint32(w), C.c_uint32(h), _ptr(out), C.c_uint64(cap),
                                                            C.byref(n)), allow)
        if own:
            return out[:n.value]
        return rc, n.value

    def channel_diff_hist(self, lin, npx=None, out=None):
        """cniic_channel_diff_hist: lin = (n, 3) uint8 numpy array, or a device tensor / address (npx: its pixels, default all of it)
        -> int64 [3, 511] array, or `out` (a device tensor / numpy array of 3 x 511 64-bit words) filled"""
        if isinstance(lin, np.ndarray):
            lin = np.ascontiguousarray(lin, np.uint8)
        if npx is None:
            npx = (lin.numel() if hasattr(lin, "numel") else lin.size) // 3
        res = np.zeros((3, 511), np.int64) if out is None else out
        self._check(self._L.cniic_channel_diff_hist(self.h, _ptr(lin) if npx else None, C.c_uint64(npx), _ptr(res)))
        return res

    def hilbert_delta(self, img):
        img = np.ascontiguousarray(img, np.uint8)
        h, w = img.shape[:2]
        syms = np.empty(h * w, np.uint32)
        self._check(self._L.cniic_hilbert_delta(self.h, _ptr(img), C.c_uint32(w), C.c_uint32(h), _ptr(syms)))
        return syms

    def hilbert_delta_hist(self, img, want_syms=False, w=None, h=None):
        if isinstance(img, np.ndarray):
            img = np.ascontiguousarray(img, np.uint8)
            h, w = img.shape[:2]
        nu = C.c_uint64(0)
        self._check(self._L.cniic_hilbert_delta_hist(self.h, _ptr(img), C.c_uint32(w), C.c_uint32(h), None, None, C.c_uint64(0),
                                                     C.byref(nu), None))
        keys = np.empty(max(nu.value, 1), np.uint32)
        counts = np.empty(max(nu.value, 1), np.uint64)
        syms = np.empty(h * w, np.uint32) if want_syms else None
        self._check(self._L.cniic_hilbert_delta_hist(self.h, _ptr(img), C.c_uint32(w), C.c_uint32(h), _ptr(keys), _ptr(counts),
                                                     C.c_uint64(keys.size), C.byref(nu), _ptr(syms)))
        return keys[:nu.value], counts[:nu.value], syms

    # ---- Huffman
    def huf_encode_all(self, kind, syms):
        syms = np.ascontiguousarray(syms, np.uint32)
        cap = 64 + syms.size * 20
        out = np.empty(cap, np.uint8)
        ln = C.c_uint64(0)
        self._check(self._L.cniic_huf_encode_all(self.h, kind, _ptr(syms), C.c_uint64(syms.size), _ptr(out), C.c_uint64(cap), C.byref(ln)))
        return out[:ln.value].tobytes()

    def huf_size(self, kind, counts):
        counts = np.ascontiguousarray(counts, np.uint64)
        nb = C.c_uint64(0)
        rc = self._L.cniic_huf_size(kind, _ptr(counts), C.c_uint64(counts.size), C.byref(nb))
        if rc != OK:
            raise CniicError(rc)
        return nb.value

    # ---- codecs
    def encode(self, expr, img, w=None, h=None, out=None, seed=0, max_iters=0, flags=0, allow=()):
        """Codec::encode.  img: HxWx3 uint8 numpy array, or a device tensor / address with w,h given."""
        if isinstance(img, np.ndarray):
            img = np.ascontiguousarray(img, np.uint8)
            h, w = img.shape[:2]
        own = out is None
        if own:
            cap = 64 + w * h * 16 + (1 << 16)
            out = np.empty(cap, np.uint8)
        else:
            cap = out.numel() if hasattr(out, "numel") else out.size
        ln = C.c_uint64(0)
        st = KmStats()
        o = self._opts(seed, max_iters, flags)
        rc = self._check(self._L.cniic_codec_encode_opts(self.h, expr.encode(), C.byref(o), _ptr(img), C.c_uint32(w), C.c_uint32(h),
                                                         _ptr(out), C.c_uint64(cap), C.byref(ln), C.byref(st)), allow)
        if own:
            return rc, (out[:ln.value].tobytes() if rc == OK else b""), st.as_dict()
        return rc, ln.value, st.as_dict()

    def encode_warm(self, expr, img, init, w=None, h=None, out=None, seed=0, max_iters=0, flags=0, allow=()):
        """cniic_codec_encode_warm: Codec::encode of cluster-colors(K) / voronoi(K) with the K-means started from init ((K, 3) uint8, or K
        COLORPOS entries) -> (rc, stream or its length as encode, stats, final centroids in init's layout: the next frame's init)"""
        if isinstance(img, np.ndarray):
            img = np.ascontiguousarray(img, np.uint8)
            h, w = img.shape[:2]
        init = np.ascontiguousarray(init)
        if init.dtype != COLORPOS:
            init = np.ascontiguousarray(init, np.uint8).reshape(-1, 3)
        cent = np.zeros_like(init)
        own = out is None
        if own:
            cap = 64 + w * h * 16 + (1 << 16) + 19 * init.shape[0]
            out = np.empty(cap, np.uint8)
        else:
            cap = out.numel() if hasattr(out, "numel") else out.size
        ln = C.c_uint64(0)
        st = KmStats()
        o = self._opts(seed, max_iters, flags)
        rc = self._check(self._L.cniic_codec_encode_warm(self.h, expr.encode(), C.byref(o), _ptr(init), _ptr(img), C.c_uint32(w), C.c_uint32(h),
                                                         _ptr(out), C.c_uint64(cap), C.byref(ln), _ptr(cent), C.byref(st)), allow)
        if own:
            return rc, (out[:ln.value].tobytes() if rc == OK else b""), st.as_dict(), cent
        return rc, ln.value, st.as_dict(), cent

    def hilbert_rle_approx_encode(self, d, img, w=None, h=None, out=None, allow=()):
        """cniic_hilbert_rle_approx_encode: Hilbert { compress: RLE(d) }::encode for an f64 d (d == 0.0: the `hilbert(rle)` stream).
        img: HxWx3 uint8 numpy array, or a device tensor / address with w,h given.  -> (rc, bytes) when out is None, else (rc, length)"""
        if isinstance(img, np.ndarray):
            img = np.ascontiguousarray(img, np.uint8)
            h, w = img.shape[:2]
        own = out is None
        if own:
            cap = 8 + w * h * 12
            out = np.empty(cap, np.uint8)
        else:
            cap = out.numel() if hasattr(out, "numel") else out.size
        ln = C.c_uint64(0)
        rc = self._check(self._L.cniic_hilbert_rle_approx_encode(self.h, C.c_double(d), _ptr(img), C.c_uint32(w), C.c_uint32(h), _ptr(out),
                                                                 C.c_uint64(cap), C.byref(ln)), allow)
        if own:
            return rc, (out[:ln.value].tobytes() if rc == OK else b"")
        return rc, ln.value

    # ---- the dictionary coder
    def zip_dict_encode(self, data, n=None, out=None, allow=()):
        """cniic_zip_dict_encode: data = bytes / numpy array (host), or a device tensor / address with n given.
        -> (rc, bytes) when out is None, else (rc, length)"""
        if isinstance(data, (bytes, bytearray)):
            data = np.frombuffer(bytes(data), np.uint8)
        if n is None:
            n = data.numel() if hasattr(data, "numel") else data.size
        own = out is None
        if own:
            cap = 2 * n + 4
            out = np.empty(cap, np.uint8)
        else:
            cap = out.numel() if hasattr(out, "numel") else out.size
        ln = C.c_uint64(0)
        rc = self._check(self._L.cniic_zip_dict_encode(self.h, _ptr(data) if n else None, C.c_uint64(n), _ptr(out), C.c_uint64(cap), C.byref(ln)), allow)
        if own:
            return rc, (out[:ln.value].tobytes() if rc == OK else b"")
        return rc, ln.value

    def zip_dict_decode(self, data, n=None, out=None, cap=None, allow=()):
        """cniic_zip_dict_decode -> (rc, bytes) when out is None (cap: the most bytes the text may have, default 64 MiB), else (rc, length;
        with CAPACITY: the bytes needed)"""
        if isinstance(data, (bytes, bytearray)):
            data = np.frombuffer(bytes(data), np.uint8)
        if n is None:
            n = data.numel() if hasattr(data, "numel") else data.size
        own = out is None
        if own:
            cap = (64 << 20) if cap is None else cap
            out = np.empty(max(cap, 1), np.uint8)
        elif cap is None:
            cap = out.numel() if hasattr(out, "numel") else out.size
        ln = C.c_uint64(0)
        rc = self._check(self._L.cniic_zip_dict_decode(self.h, _ptr(data) if n else None, C.c_uint64(n), _ptr(out), C.c_uint64(cap), C.byref(ln)), allow)
        if own:
            return rc, (out[:ln.value].tobytes() if rc == OK else b"")
        return rc, ln.value

    def hilbert_zip_encode(self, img, w=None, h=None, out=None, allow=()):
        """cniic_hilbert_zip_encode.  img: HxWx3 uint8 numpy array, or a device tensor / address with w,h given.
        -> (rc, bytes) when out is None, else (rc, length)"""
        if isinstance(img, np.ndarray):
            img = np.ascontiguousarray(img, np.uint8)
            h, w = img.shape[:2]
        own = out is None
        if own:
            cap = 8 + w * h * 22 + 4
            out = np.empty(cap, np.uint8)
        else:
            cap = out.numel() if hasattr(out, "numel") else out.size
        ln = C.c_uint64(0)
        rc = self._check(self._L.cniic_hilbert_zip_encode(self.h, _ptr(img), C.c_uint32(w), C.c_uint32(h), _ptr(out), C.c_uint64(cap), C.byref(ln)), allow)
        if own:
            return rc, (out[:ln.value].tobytes() if rc == OK else b"")
        return rc, ln.value

    def hilbert_zip_decode(self, data, allow=()):
        """cniic_hilbert_zip_decode of a host stream -> (rc, HxWx3 image or None)"""
        raw = np.frombuffer(bytes(data), np.uint8)
        if raw.size < 8:
            return DECODE, None
        w = int.from_bytes(raw[0:4].tobytes(), "little")
        h = int.from_bytes(raw[4:8].tobytes(), "little")
        if w * h > (1 << 28):
            return CAPACITY, None
        out = np.zeros((max(w * h, 1), 3), np.uint8)
        cw, ch = C.c_uint32(0), C.c_uint32(0)
        rc = self._check(self._L.cniic_hilbert_zip_decode(self.h, _ptr(raw), C.c_uint64(raw.size), _ptr(out), C.c_uint64(out.size), C.byref(cw),
                                                          C.byref(ch)), allow)
        if rc != OK:
            return rc, None
        return rc, out[:w * h].reshape(h, w, 3)

    # ---- the look-back coder
    def zip_back_encode(self, data, n=None, out=None, allow=()):
        """cniic_zip_back_encode: data = bytes / numpy array (host), or a device tensor / address with n given.
        -> (rc, bytes) when out is None, else (rc, length; with CAPACITY: the bytes needed)"""
        if isinstance(data, (bytes, bytearray)):
            data = np.frombuffer(bytes(data), np.uint8)
        if n is None:
            n = data.numel() if hasattr(data, "numel") else data.size
        own = out is None
        if own:
            cap = n + n // 4 + 16
            out = np.empty(cap, np.uint8)
        else:
            cap = out.numel() if hasattr(out, "numel") else out.size
        ln = C.c_uint64(0)
        rc = self._check(self._L.cniic_zip_back_encode(self.h, _ptr(data) if n else None, C.c_uint64(n), _ptr(out), C.c_uint64(cap), C.byref(ln)), allow)
        if own:
            return rc, (out[:ln.value].tobytes() if rc == OK else b"")
        return rc, ln.value

    def zip_back_decode(self, data, n=None, out=None, cap=None, allow=()):
        """cniic_zip_back_decode -> (rc, bytes) when out is None (cap: the most bytes the text may have, default 64 MiB), else (rc, length;
        with CAPACITY: the bytes needed)"""
        if isinstance(data, (bytes, bytearray)):
            data = np.frombuffer(bytes(data), np.uint8)
        if n is None:
            n = data.numel() if hasattr(data, "numel") else data.size
        own = out is None
        if own:
            cap = (64 << 20) if cap is None else cap
            out = np.empty(max(cap, 1), np.uint8)
        elif cap is None:
            cap = out.numel() if hasattr(out, "numel") else out.size
        ln = C.c_uint64(0)
        rc = self._check(self._L.cniic_zip_back_decode(self.h, _ptr(data) if n else None, C.c_uint64(n), _ptr(out), C.c_uint64(cap), C.byref(ln)), allow)
        if own:
            return rc, (out[:ln.value].tobytes() if rc == OK else b"")
        return rc, ln.value

    def zip_back_image_encode(self, img, w=None, h=None, out=None, allow=()):
        """cniic_zip_back_image_encode.  img: HxWx3 uint8 numpy array, or a device tensor / address with w,h given.
        -> (rc, bytes) when out is None, else (rc, length)"""
        if isinstance(img, np.ndarray):
            img = np.ascontiguousarray(img, np.uint8)
            h, w = img.shape[:2]
        own = out is None
        if own:
            cap = 14 * w * h + 32
            out = np.empty(cap, np.uint8)
        else:
            cap = out.numel() if hasattr(out, "numel") else out.size
        ln = C.c_uint64(0)
        rc = self._check(self._L.cniic_zip_back_image_encode(self.h, _ptr(img), C.c_uint32(w), C.c_uint32(h), _ptr(out), C.c_uint64(cap), C.byref(ln)), allow)
        if own:
            return rc, (out[:ln.value].tobytes() if rc == OK else b"")
        return rc, ln.value

    def zip_back_image_decode(self, data, allow=()):
        """cniic_zip_back_image_decode of a host stream -> (rc, HxWx3 image or None)"""
        raw = np.frombuffer(bytes(data), np.uint8)
        dims = zip_back_dims(raw)
        if dims is None:
            return DECODE, None
        w, h = dims
        if w * h > (1 << 28):
            return CAPACITY, None
        out = np.zeros((max(w * h, 1), 3), np.uint8)
        cw, ch = C.c_uint32(0), C.c_uint32(0)
        rc = self._check(self._L.cniic_zip_back_image_decode(self.h, _ptr(raw), C.c_uint64(raw.size), _ptr(out), C.c_uint64(out.size), C.byref(cw),
                                                             C.byref(ch)), allow)
        if rc != OK:
            return rc, None
        return rc, out[:w * h].reshape(h, w, 3)

    def zip_back_image_decode_into(self, data, nbytes, out, allow=()):
        """cniic_zip_back_image_decode with caller-owned buffers (device tensors, numpy arrays or addresses) -> (rc, w, h)"""
        cap = out.numel() if hasattr(out, "numel") else out.size
        cw, ch = C.c_uint32(0), C.c_uint32(0)
        rc = self._check(self._L.cniic_zip_back_image_decode(self.h, _ptr(data), C.c_uint64(nbytes), _ptr(out), C.c_uint64(cap), C.byref(cw), C.byref(ch)), allow)
        return rc, cw.value, ch.value

    def zip_back_encode_batch_var(self, images, offs, ws, hs, out, stride, allow=()):
        """cniic_zip_back_image_encode_batch_var: the layout of encode_batch_var -> (rc, list of lengths, list of per-image status codes)"""
        F = len(offs)
        n = max(F, 1)
        off = (C.c_uint64 * n)(*[int(x) for x in offs])
        w = (C.c_uint32 * n)(*[int(x) for x in ws])
        h = (C.c_uint32 * n)(*[int(x) for x in hs])
        lens, rcs = (C.c_uint64 * n)(), (C.c_int32 * n)()
        rc = self._check(self._L.cniic_zip_back_image_encode_batch_var(self.h, _ptr(images), off, w, h, C.c_uint32(F), _ptr(out), C.c_uint64(stride), lens, rcs), allow)
        return rc, [int(lens[f]) for f in range(F)], [int(rcs[f]) for f in range(F)]

    def zip_back_decode_batch(self, streams, stride, lens, F, out, img_stride, allow=()):
        """cniic_zip_back_image_decode_batch: the layout of decode_batch -> (rc, list of widths, list of heights, list of per-frame status codes)"""
        n = max(F, 1)
        ln = (C.c_uint64 * n)(*[int(x) for x in lens])
        ws, hs, rcs = (C.c_uint32 * n)(), (C.c_uint32 * n)(), (C.c_int32 * n)()
        rc = self._check(self._L.cniic_zip_back_image_decode_batch(self.h, _ptr(streams), C.c_uint64(stride), ln, C.c_uint32(F), _ptr(out), C.c_uint64(img_stride),
                                                                   ws, hs, rcs), allow)
        return rc, [int(ws[f]) for f in range(F)], [int(hs[f]) for f in range(F)], [int(rcs[f]) for f in range(F)]

    def encode_batch(self, expr, frames, w, h, F, out, stride, seed=0, max_iters=0, flags=0, allow=()):
        """cniic_codec_encode_batch: F images (one contiguous [F][h][w][3] buffer), each encoded on its own (its own palette), image f's
        stream at out[f * stride:].  -> (rc, list of F lengths, list of F per-image status codes, list of F stats dicts)"""
        lens = (C.c_uint64 * F)()
        rcs = (C.c_int32 * F)()
        sts = (KmStats * F)()
        o = self._opts(seed, max_iters, flags)
        rc = self._check(self._L.cniic_codec_encode_batch(self.h, expr.encode(), C.byref(o), _ptr(frames), C.c_uint32(w), C.c_uint32(h), C.c_uint32(F),
                                                          _ptr(out), C.c_uint64(stride), lens, rcs, sts), allow)
        return rc, [int(x) for x in lens], [int(x) for x in rcs], [s.as_dict() for s in sts]

    def encode_batch_var(self, expr, images, offs, ws, hs, out, stride, seed=0, max_iters=0, flags=0, allow=()):
        """cniic_codec_encode_batch_var: len(offs) images of different sizes in one buffer (image f is ws[f] x hs[f] at images[offs[f]:]),
        each encoded on its own, image f's stream at out[f * stride:].  images / out: device tensors, numpy arrays or addresses.
        -> (rc, list of lengths, list of per-image status codes, list of stats dicts)"""
        F = len(offs)
        n = max(F, 1)
        off = (C.c_uint64 * n)(*[int(x) for x in offs])
        w = (C.c_uint32 * n)(*[int(x) for x in ws])
        h = (C.c_uint32 * n)(*[int(x) for x in hs])
        lens, rcs, sts = (C.c_uint64 * n)(), (C.c_int32 * n)(), (KmStats * n)()
        o = self._opts(seed, max_iters, flags)
        rc = self._check(self._L.cniic_codec_encode_batch_var(self.h, expr.encode(), C.byref(o), _ptr(images), off, w, h, C.c_uint32(F), _ptr(out),
                                                              C.c_uint64(stride), lens, rcs, sts), allow)
        return rc, [int(lens[f]) for f in range(F)], [int(rcs[f]) for f in range(F)], [sts[f].as_dict() for f in range(F)]

    def mse_batch_var(self, a, a_offs, b, b_offs, npx):
        """cniic_mse_batch_var: the MSE of len(npx) pairs of different sizes (pair f: npx[f] pixels at a[a_offs[f]:] and b[b_offs[f]:])
        -> list of floats"""
        F = len(npx)
        n = max(F, 1)
        ao = (C.c_uint64 * n)(*[int(x) for x in a_offs])
        bo = (C.c_uint64 * n)(*[int(x) for x in b_offs])
        px = (C.c_uint64 * n)(*[int(x) for x in npx])
        v = (C.c_double * n)()
        self._check(self._L.cniic_mse_batch_var(self.h, _ptr(a), ao, _ptr(b), bo, px, C.c_uint32(F), v))
        return [float(v[f]) for f in range(F)]

    def frames_from_surfaces(self, src, surfaces, rgb, img_offs, allow=()):
        """cniic_frames_from_surfaces: surface f of src (a list of Surface) -> packed RGB24 at rgb[img_offs[f]:], all frames in one launch.
        src / rgb: device tensors, numpy arrays or addresses.  With device memory on both sides the call is asynchronous on the
        context's stream (sync() waits).  -> rc"""
        F = len(surfaces)
        n = max(F, 1)
        return self._check(self._L.cniic_frames_from_surfaces(self.h, _ptr(src), (Surface * n)(*surfaces), C.c_uint32(F), _ptr(rgb),
                                                              (C.c_uint64 * n)(*[int(x) for x in img_offs])), allow)

    def frames_to_surfaces(self, rgb, img_offs, surfaces, dst, alpha=255, allow=()):
        """cniic_frames_to_surfaces: packed RGB24 at rgb[img_offs[f]:] -> surface f of dst (RGB8 / BGR8 / RGBA8 / BGRA8; the alpha byte
        written is `alpha`), the pitch's padding untouched.  -> rc"""
        F = len(surfaces)
        n = max(F, 1)
        return self._check(self._L.cniic_frames_to_surfaces(self.h, _ptr(rgb), (C.c_uint64 * n)(*[int(x) for x in img_offs]), (Surface * n)(*surfaces),
                                                            C.c_uint32(F), _ptr(dst), C.c_uint32(alpha)), allow)

    def measure_batch(self, expr, images, offs, ws, hs, out=None, stride=0, seed=0, max_iters=0, flags=0, allow=()):
        """cniic_codec_measure_batch: encode, size, ratio, decode, MSE and the lossless check of every image in one call (the body of
        bench::measure_all's loop).  out (optional): stream f is copied to out[f * stride:].
        -> (rc, list of row dicts, list of stream lengths)"""
        F = len(offs)
        n = max(F, 1)
        off = (C.c_uint64 * n)(*[int(x) for x in offs])
        w = (C.c_uint32 * n)(*[int(x) for x in ws])
        h = (C.c_uint32 * n)(*[int(x) for x in hs])
        rows, lens = (MeasureRow * n)(), (C.c_uint64 * n)()
        o = self._opts(seed, max_iters, flags)
        rc = self._check(self._L.cniic_codec_measure_batch(self.h, expr.encode(), C.byref(o), _ptr(images), off, w, h, C.c_uint32(F), rows, _ptr(out),
                                                           C.c_uint64(stride), lens), allow)
        return rc, [rows[f].as_dict() for f in range(F)], [int(lens[f]) for f in range(F)]

    def decode(self, expr, data, allow=()):
        raw = np.frombuffer(bytes(data), np.uint8)
        dims = stream_dims(expr, raw)
        if dims is None:
            return DECODE, None
        w, h = dims
        if w * h > (1 << 28):
            return CAPACITY, None
        out = np.zeros((max(w * h, 1), 3), np.uint8)
        cw, ch = C.c_uint32(0), C.c_uint32(0)
        rc = self._check(self._L.cniic_codec_decode(self.h, expr.encode(), _ptr(raw), C.c_uint64(raw.size), _ptr(out),
                                                    C.c_uint64(out.size), C.byref(cw), C.byref(ch)), allow)
        if rc != OK:
            return rc, None
        return rc, out[:w * h].reshape(h, w, 3)

    def decode_into(self, expr, data, nbytes, out, allow=()):
        """Codec::decode with caller-owned buffers: data = the stream (device tensor / address / numpy array), nbytes of it;
        out = a uint8 buffer (device tensor or numpy array) that receives the w x h x 3 image.  -> (rc, w, h)"""
        cap = out.numel() if hasattr(out, "numel") else out.size
        cw, ch = C.c_uint32(0), C.c_uint32(0)
        rc = self._check(self._L.cniic_codec_decode(self.h, expr.encode(), _ptr(data), C.c_uint64(nbytes), _ptr(out), C.c_uint64(cap),
                                                    C.byref(cw), C.byref(ch)), allow)
        return rc, cw.value, ch.value

    def decode_batch(self, expr, streams, stride, lens, F, out, img_stride, allow=()):
        """cniic_codec_decode_batch: F streams (stream f at streams[f * stride:], lens[f] bytes -- what encode_batch wrote), image f into
        out[f * img_stride:] (img_stride bytes at most).  streams / out: device tensors, numpy arrays or addresses.
        -> (rc, list of F widths, list of F heights, list of F per-frame status codes)"""
        ln = (C.c_uint64 * F)(*[int(x) for x in lens])
        ws, hs, rcs = (C.c_uint32 * F)(), (C.c_uint32 * F)(), (C.c_int32 * F)()
        rc = self._check(self._L.cniic_codec_decode_batch(self.h, expr.encode(), _ptr(streams), C.c_uint64(stride), ln, C.c_uint32(F), _ptr(out),
                                                          C.c_uint64(img_stride), ws, hs, rcs), allow)
        return rc, [int(x) for x in ws], [int(x) for x in hs], [int(x) for x in rcs]

    def mse_batch(self, a, b, npx, F):
        """cniic_mse_batch: the MSE of F image pairs of npx pixels each (pair f at a[f * npx * 3:], b[f * npx * 3:]) -> list of F floats"""
        if isinstance(a, np.ndarray):
            a = np.ascontiguousarray(a, np.uint8)
        if isinstance(b, np.ndarray):
            b = np.ascontiguousarray(b, np.uint8)
        v = (C.c_double * max(F, 1))()
        self._check(self._L.cniic_mse_batch(self.h, _ptr(a), _ptr(b), C.c_uint64(npx), C.c_uint32(F), v))
        return [float(v[i]) for i in range(F)]

    def mse(self, a, b):
        """cniic_mse of two RGB8 images of the same size: numpy arrays, or uint8 tensors (on the device: read in place, no copy)"""
        a = a.contiguous() if hasattr(a, "data_ptr") else np.ascontiguousarray(a, np.uint8)
        b = b.contiguous() if hasattr(b, "data_ptr") else np.ascontiguousarray(b, np.uint8)
        na = a.numel() if hasattr(a, "numel") else a.size
        nb = b.numel() if hasattr(b, "numel") else b.size
        if na != nb:
            raise ValueError("mse: images of %d and %d bytes" % (na, nb))
        v = C.c_double(0)
        self._check(self._L.cniic_mse(self.h, _ptr(a), _ptr(b), C.c_uint64(na // 3), C.byref(v)))
        return v.value

    def synth_image(self, kind, seed, w, h, out=None):
        if out is None:
            out = np.empty((h, w, 3), np.uint8)
        self._check(self._L.cniic_synth_image(self.h, kind, C.c_uint64(seed), C.c_uint32(w), C.c_uint32(h), _ptr(out)))
        return out


class Palette:
    """cniic_palette: a FROZEN palette of K colours on one Context -- every pixel's label is the nearest entry in squared integer distance,
    the lowest index among equals (include/cniic_hip.h).  Built once (the table of all 2^24 colours), used for any number of calls:

        pal = Palette.create(ctx, centroids)          # (K, 3) uint8: numpy array or device tensor
        lens = pal.encode_frames_var(flat, ws, hs, out, stride)
        pal.close()
    """

    def __init__(self, ctx, centroids, K=None):
        if isinstance(centroids, np.ndarray):
            centroids = np.ascontiguousarray(centroids, np.uint8)
        if K is None:
            K = (centroids.numel() if hasattr(centroids, "numel") else centroids.size) // 3
        self.ctx = ctx
        self.K = int(K)
        self.h = None
        h = C.c_void_p()
        ctx._check(ctx._L.cniic_palette_create(ctx.h, _ptr(centroids), C.c_uint32(self.K), C.byref(h)))
        self.h = h
        self.label_bytes = int(ctx._L.cniic_palette_label_bytes(h))

    @classmethod
    def create(cls, ctx, centroids, K=None):
        return cls(ctx, centroids, K)

    def close(self):
        if getattr(self, "h", None):
            self.ctx._L.cniic_palette_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            if getattr(self.ctx, "h", None):   # (a handle dies with its context)
                self.close()
        except Exception:
            pass

    def labels(self, rgb, npx=None, out=None):
        """cniic_palette_labels: the index image.  rgb: (..., 3) uint8 numpy array, or a device tensor / address with npx given; out: a
        buffer of npx labels of label_bytes bytes each (numpy array, device tensor), default a new numpy array -> out"""
        if isinstance(rgb, np.ndarray):
            rgb = np.ascontiguousarray(rgb, np.uint8)
        if npx is None:
            npx = (rgb.numel() if hasattr(rgb, "numel") else rgb.size) // 3
        if out is None:
            out = np.empty(max(npx, 1), np.uint8 if self.label_bytes == 1 else np.uint16)[:npx]
        self.ctx._check(self.ctx._L.cniic_palette_labels(self.h, _ptr(rgb) if npx else None, C.c_uint64(npx), _ptr(out)))
        return out

    def encode_frames_var(self, frames_flat, ws, hs, out, stride, allow=()):
        """cniic_palette_encode_frames_var: len(ws) frames of different sizes, back to back in frames_flat (device tensor, numpy array or
        address), frame f's stream at out[f * stride:] -> list of lengths; with a status in `allow`: (status, lengths)"""
        F = len(ws)
        n = max(F, 1)
        w = (C.c_uint32 * n)(*[int(x) for x in ws])
        hh = (C.c_uint32 * n)(*[int(x) for x in hs])
        lens = (C.c_uint64 * n)()
        rc = self.ctx._check(self.ctx._L.cniic_palette_encode_frames_var(self.h, _ptr(frames_flat), w, hh, C.c_uint32(F), _ptr(out), C.c_uint64(stride), lens), allow)
        if allow:
            return rc, [int(lens[f]) for f in range(F)]
        return [int(lens[f]) for f in range(F)]


    def fit_frames_var(self, frames_flat, ws, hs, want_pixels=True, allow=()):
        """cniic_palette_fit_frames_var: len(ws) frames of different sizes, back to back in frames_flat (device tensor, numpy array or
        address) -> (sse: uint64[F], the exact summed squared distance of every frame's pixels to their entries; pixels: uint64[K], the
        pixels of all frames per entry, or None); with a status in `allow`: (status, sse, pixels)"""
        F = len(ws)
        n = max(F, 1)
        w = (C.c_uint32 * n)(*[int(x) for x in ws])
        hh = (C.c_uint32 * n)(*[int(x) for x in hs])
        sse = np.zeros(n, np.uint64)
        pixels = np.zeros(self.K, np.uint64) if want_pixels else None
        rc = self.ctx._check(self.ctx._L.cniic_palette_fit_frames_var(self.h, _ptr(frames_flat), w, hh, C.c_uint32(F), _ptr(sse), _ptr(pixels)), allow)
        if allow:
            return rc, sse[:F], pixels
        return sse[:F], pixels


def surface_span(s):
    """cniic_surface_span (host only, no context): (one past the last byte of the buffer the surface spans, 3 w h), or None for a
    descriptor the calls refuse"""
    end, nb = C.c_uint64(0), C.c_uint64(0)
    rc = lib().cniic_surface_span(C.byref(s), C.byref(end), C.byref(nb))
    return (end.value, nb.value) if rc == OK else None


def linearize_count(method, w, h):
    """cniic_hilbert_linearize_count: pixels `method` ("rect" | "small" | "large", or a CNIIC_LIN_* number) yields for a w x h image"""
    m = LIN_METHODS[method] if isinstance(method, str) else int(method)
    n = C.c_uint64(0)
    rc = lib().cniic_hilbert_linearize_count(C.c_int32(m), C.c_uint32(w), C.c_uint32(h), C.byref(n))
    if rc != OK:
        raise CniicError(rc, "linearize_count(%r, %d, %d)" % (method, w, h))
    return n.value


def hilbert_linearize(img, method="rect", ctx=None):
    """hilbert::linearize_rect / linearize_small / linearize_large (hilbert.rs:10-32) of an HxWx3 uint8 image: a numpy array -> the
    (npx, 3) numpy array of its pixels in that order; a device tensor -> a device tensor.  ctx: a Context, or None for one on device 0"""
    own = ctx is None
    if own:
        ctx = Context(0)
    try:
        if isinstance(img, np.ndarray):
            return ctx.hilbert_linearize_as(img, method)
        import torch
        img = img.contiguous()
        h, w = int(img.shape[0]), int(img.shape[1])
        out = torch.empty((max(linearize_count(method, w, h), 1), 3), dtype=torch.uint8, device=img.device)
        torch.cuda.synchronize(img.device)   # (the context runs on a stream of its own)
        _, n = ctx.hilbert_linearize_as(img, method, w, h, out)
        return out[:n]
    finally:
        if own:
            ctx.close()


def channel_diff_hist(lin, ctx=None):
    """counts[c][v + 255] = how often channel c steps by v between neighbours of the linear RGB stream `lin` ((n, 3) uint8: numpy array or
    device tensor) -> int64 [3, 511] numpy array (scripts/experiments/hilbert_distribution.py)"""
    own = ctx is None
    if own:
        ctx = Context(0)
    try:
        if not isinstance(lin, np.ndarray):
            import torch
            lin = lin.contiguous()
            torch.cuda.synchronize(lin.device)
        return ctx.channel_diff_hist(lin)
    finally:
        if own:
            ctx.close()


def zip_dict_dims(data):
    """cniic_zip_dict_dims: (w, h) from the first pairs of a zip(dict) stream in host memory, or None"""
    raw = data if isinstance(data, np.ndarray) else np.frombuffer(bytes(data), np.uint8)
    w, h = C.c_uint32(0), C.c_uint32(0)
    rc = lib().cniic_zip_dict_dims(_ptr(raw) if raw.size else None, C.c_uint64(raw.size), C.byref(w), C.byref(h))
    return (w.value, h.value) if rc == OK else None


def zip_back_dims(data):
    """cniic_zip_back_dims: (w, h) from the first symbols of a zip-back stream in host memory, or None"""
    raw = data if isinstance(data, np.ndarray) else np.frombuffer(bytes(data), np.uint8)
    w, h = C.c_uint32(0), C.c_uint32(0)
    rc = lib().cniic_zip_back_dims(_ptr(raw) if raw.size else None, C.c_uint64(raw.size), C.byref(w), C.byref(h))
    return (w.value, h.value) if rc == OK else None


def stream_dims(expr, data):
    """(w, h) of a stream of codec `expr` in host memory, or None: its first 8 bytes -- for zip(dict), the first 8 bytes of its text"""
    p = codec_parse_f64(expr)
    if p is not None and p[0] == KIND_ZIP_DICT:
        return zip_dict_dims(data)
    if len(data) < 8:
        return None
    return int.from_bytes(bytes(data[0:4]), "little"), int.from_bytes(bytes(data[4:8]), "little")


def codec_parse(expr):
    kind, arg = C.c_int32(0), C.c_uint32(0)
    rc = lib().cniic_codec_parse(expr.encode(), C.byref(kind), C.byref(arg))
    if rc != OK:
        return None
    return kind.value, arg.value


def codec_parse_f64(expr):
    """cniic_codec_parse_f64: every expression, hilbert(rle(d)) included -> (kind, u32 argument, d), or None"""
    kind, arg, darg = C.c_int32(0), C.c_uint32(0), C.c_double(0.0)
    rc = lib().cniic_codec_parse_f64(expr.encode(), C.byref(kind), C.byref(arg), C.byref(darg))
    if rc != OK:
        return None
    return kind.value, arg.value, darg.value


def codec_name(expr):
    cap = 64
    while True:   # (hilbert-rle-approx_<d> spells d without an exponent: 5e-324 takes more than 330 characters)
        buf = C.create_string_buffer(cap)
        rc = lib().cniic_codec_name(expr.encode(), buf, C.c_uint64(cap))
        if rc != CAPACITY or cap >= 1 << 16:
            break
        cap *= 8
    if rc != OK:
        raise CniicError(rc, "Malformed codec argument: %s" % expr)
    return buf.value.decode()


def codec_is_lossless(expr):
    rc = lib().cniic_codec_is_lossless(expr.encode())
    if rc < 0:
        raise CniicError(rc, "Malformed codec argument: %s" % expr)
    return bool(rc)
