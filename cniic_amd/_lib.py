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

# The prototype of every function include/cniic_hip.h declares: name -> (restype, argtypes), held against the header by tests/test_abi.py.
# The mapping is fixed: int32_t / uint32_t / uint64_t / double by value -> _I32 / _U32 / _U64 / _F64; `const char *` -> _STR; every other
# pointer or array (data, out-parameters, structs, opaque handles, `char *buf`) -> _PTR, which takes None, an address, byref(...), a ctypes
# array and bytes alike; cniic_host_sum_fn -> HOST_SUM_FN; void -> None.  With these in place a bare Python int arrives in its full width.
_I32, _U32, _U64, _F64, _STR, _PTR = C.c_int32, C.c_uint32, C.c_uint64, C.c_double, C.c_char_p, C.c_void_p
PROTOTYPES = {
    "cniic_ctx_create": (_I32, [_I32, _PTR, _PTR]),
    "cniic_ctx_destroy": (None, [_PTR]),
    "cniic_last_error": (_STR, [_PTR]),
    "cniic_version": (_I32, []),
    "cniic_is_testing_build": (_I32, []),
    "cniic_sync": (_I32, [_PTR]),
    "cniic_dev_alloc": (_I32, [_PTR, _U64, _PTR]),
    "cniic_dev_free": (_I32, [_PTR, _PTR]),
    "cniic_memcpy": (_I32, [_PTR, _PTR, _PTR, _U64]),
    "cniic_ctx_set_opt": (_I32, [_PTR, _I32, _U64]),
    "cniic_ctx_unset_opt": (_I32, [_PTR, _I32]),
    "cniic_ctx_get_opt": (_I32, [_PTR, _I32, _PTR]),
    "cniic_ctx_set_scan": (_I32, [_PTR, _U32, _U32, _PTR]),
    "cniic_last_kernel_time": (_I32, [_PTR, _STR, _PTR, _PTR]),
    "cniic_hist_rgb24": (_I32, [_PTR, _PTR, _U64, _PTR, _PTR, _U64, _PTR]),
    "cniic_hist_syms": (_I32, [_PTR, _I32, _PTR, _U64, _PTR, _PTR, _U64, _PTR]),
    "cniic_kmeans_rgbw": (_I32, [_PTR, _PTR, _PTR, _U64, _U32, _PTR, _PTR, _PTR, _PTR, _PTR]),
    "cniic_kmeans_xyrgb": (_I32, [_PTR, _PTR, _U32, _U32, _U32, _PTR, _PTR, _PTR, _PTR, _PTR]),
    "cniic_kmeans_step_rgbw": (_I32, [_PTR, _PTR, _PTR, _U64, _U32, _PTR, _PTR, _PTR, _PTR, _PTR, _PTR]),
    "cniic_kmeans_step_xyrgb": (_I32, [_PTR, _PTR, _U32, _U32, _U32, _PTR, _PTR, _PTR, _PTR, _PTR, _PTR]),
    "cniic_km_create_rgbw": (_I32, [_PTR, _PTR, _PTR, _U64, _U32, _U32, _U32, _PTR, _PTR, _PTR]),
    "cniic_km_partial_words": (_U64, [_U32, _U32]),
    "cniic_km_partials": (_I32, [_PTR, _PTR]),
    "cniic_km_begin": (_I32, [_PTR]),
    "cniic_km_labels_internal": (_I32, [_PTR, _PTR, _PTR]),
    "cniic_km_assign": (_I32, [_PTR]),
    "cniic_km_update": (_I32, [_PTR, _PTR]),
    "cniic_km_result": (_I32, [_PTR, _PTR, _PTR, _PTR, _PTR]),
    "cniic_km_time_assign": (_I32, [_PTR, _I32, _PTR]),
    "cniic_km_destroy": (None, [_PTR]),
    "cniic_hist_rgb24_dense": (_I32, [_PTR, _PTR, _U64, _PTR]),
    "cniic_cc_create": (_I32, [_PTR, _PTR, _U32, _PTR, _U32, _U32, _PTR, _PTR]),
    "cniic_cc_unique": (_U64, [_PTR]),
    "cniic_cc_label_bytes": (_U32, [_PTR]),
    "cniic_cc_partials": (_I32, [_PTR, _PTR]),
    "cniic_cc_assign": (_I32, [_PTR]),
    "cniic_cc_update": (_I32, [_PTR, _PTR]),
    "cniic_cc_poll": (_I32, [_PTR, _PTR, _PTR]),
    "cniic_cc_poll_lagged": (_I32, [_PTR, _PTR, _PTR, _PTR]),
    "cniic_cc_export_labels": (_I32, [_PTR, _PTR]),
    "cniic_cc_import_labels": (_I32, [_PTR, _PTR]),
    "cniic_cc_finish": (_I32, [_PTR, _PTR, _U32, _U32, _PTR, _PTR, _U64, _PTR, _PTR]),
    "cniic_cc_finish_frames": (_I32, [_PTR, _PTR, _U32, _U32, _U32, _PTR, _U64, _PTR, _PTR]),
    "cniic_cc_destroy": (None, [_PTR]),
    "cniic_comm_unique_id": (_I32, [_PTR]),
    "cniic_comm_create": (_I32, [_PTR, _PTR, _U32, _U32, _PTR]),
    "cniic_comm_create_host": (_I32, [_PTR, _U32, _U32, HOST_SUM_FN, _PTR, _PTR]),
    "cniic_comm_create_mailbox": (_I32, [_PTR, _U32, _U32, _U64, _PTR, _PTR]),
    "cniic_comm_connect_mailbox": (_I32, [_PTR, _PTR]),
    "cniic_comm_destroy": (None, [_PTR]),
    "cniic_comm_all_reduce": (_I32, [_PTR, _PTR, _U64, _I32]),
    "cniic_comm_set_timeout": (_I32, [_PTR, _U64]),
    "cniic_cc_run": (_I32, [_PTR, _PTR, _PTR]),
    "cniic_occupancy_pack": (_I32, [_PTR, _PTR, _PTR]),
    "cniic_cc_create_local": (_I32, [_PTR, _PTR, _PTR, _U32, _PTR, _PTR, _PTR]),
    "cniic_cc_image_begin": (_I32, [_PTR, _PTR, _U64, _PTR]),
    "cniic_cc_image_occupancy": (_I32, [_PTR, _PTR]),
    "cniic_cc_image_create": (_I32, [_PTR, _PTR, _U32, _PTR, _PTR]),
    "cniic_remap_rgb": (_I32, [_PTR, _PTR, _U64, _PTR, _PTR, _U64, _PTR, _U32, _PTR]),
    "cniic_hilbert_xy": (_I32, [_PTR, _U32, _U32, _PTR]),
    "cniic_hilbert_linearize": (_I32, [_PTR, _PTR, _U32, _U32, _PTR]),
    "cniic_hilbert_delta": (_I32, [_PTR, _PTR, _U32, _U32, _PTR]),
    "cniic_hilbert_delta_hist": (_I32, [_PTR, _PTR, _U32, _U32, _PTR, _PTR, _U64, _PTR, _PTR]),
    "cniic_huf_encode_all": (_I32, [_PTR, _I32, _PTR, _U64, _PTR, _U64, _PTR]),
    "cniic_huf_size": (_I32, [_I32, _PTR, _U64, _PTR]),
    "cniic_codec_parse": (_I32, [_STR, _PTR, _PTR]),
    "cniic_codec_name": (_I32, [_STR, _PTR, _U64]),
    "cniic_codec_is_lossless": (_I32, [_STR]),
    "cniic_codec_encode": (_I32, [_PTR, _STR, _PTR, _U32, _U32, _PTR, _U64, _PTR, _PTR]),
    "cniic_codec_encode_opts": (_I32, [_PTR, _STR, _PTR, _PTR, _U32, _U32, _PTR, _U64, _PTR, _PTR]),
    "cniic_codec_encode_batch": (_I32, [_PTR, _STR, _PTR, _PTR, _U32, _U32, _U32, _PTR, _U64, _PTR, _PTR, _PTR]),
    "cniic_codec_decode": (_I32, [_PTR, _STR, _PTR, _U64, _PTR, _U64, _PTR, _PTR]),
    "cniic_codec_decode_batch": (_I32, [_PTR, _STR, _PTR, _U64, _PTR, _U32, _PTR, _U64, _PTR, _PTR, _PTR]),
    "cniic_mse": (_I32, [_PTR, _PTR, _PTR, _U64, _PTR]),
    "cniic_mse_batch": (_I32, [_PTR, _PTR, _PTR, _U64, _U32, _PTR]),
    "cniic_hilbert_rle_approx_encode": (_I32, [_PTR, _F64, _PTR, _U32, _U32, _PTR, _U64, _PTR]),
    "cniic_synth_image": (_I32, [_PTR, _I32, _U64, _U32, _U32, _PTR]),
    "cniic_codec_encode_batch_var": (_I32, [_PTR, _STR, _PTR, _PTR, _PTR, _PTR, _PTR, _U32, _PTR, _U64, _PTR, _PTR, _PTR]),
    "cniic_mse_batch_var": (_I32, [_PTR, _PTR, _PTR, _PTR, _PTR, _PTR, _U32, _PTR]),
    "cniic_codec_measure_batch": (_I32, [_PTR, _STR, _PTR, _PTR, _PTR, _PTR, _PTR, _U32, _PTR, _PTR, _U64, _PTR]),
    "cniic_codec_parse_f64": (_I32, [_STR, _PTR, _PTR, _PTR]),
    "cniic_zip_dict_encode": (_I32, [_PTR, _PTR, _U64, _PTR, _U64, _PTR]),
    "cniic_zip_dict_decode": (_I32, [_PTR, _PTR, _U64, _PTR, _U64, _PTR]),
    "cniic_zip_dict_dims": (_I32, [_PTR, _U64, _PTR, _PTR]),
    "cniic_hilbert_zip_encode": (_I32, [_PTR, _PTR, _U32, _U32, _PTR, _U64, _PTR]),
    "cniic_hilbert_zip_decode": (_I32, [_PTR, _PTR, _U64, _PTR, _U64, _PTR, _PTR]),
    "cniic_hilbert_zip_encode_batch_var": (_I32, [_PTR, _PTR, _PTR, _PTR, _PTR, _U32, _PTR, _U64, _PTR, _PTR]),
    "cniic_hilbert_zip_decode_batch": (_I32, [_PTR, _PTR, _U64, _PTR, _U32, _PTR, _U64, _PTR, _PTR, _PTR]),
    "cniic_hilbert_zip_measure_batch": (_I32, [_PTR, _PTR, _PTR, _PTR, _PTR, _U32, _PTR, _PTR, _U64, _PTR]),
    "cniic_zip_back_encode": (_I32, [_PTR, _PTR, _U64, _PTR, _U64, _PTR]),
    "cniic_zip_back_decode": (_I32, [_PTR, _PTR, _U64, _PTR, _U64, _PTR]),
    "cniic_zip_back_dims": (_I32, [_PTR, _U64, _PTR, _PTR]),
    "cniic_zip_back_image_encode": (_I32, [_PTR, _PTR, _U32, _U32, _PTR, _U64, _PTR]),
    "cniic_zip_back_image_decode": (_I32, [_PTR, _PTR, _U64, _PTR, _U64, _PTR, _PTR]),
    "cniic_zip_back_image_encode_batch_var": (_I32, [_PTR, _PTR, _PTR, _PTR, _PTR, _U32, _PTR, _U64, _PTR, _PTR]),
    "cniic_zip_back_image_decode_batch": (_I32, [_PTR, _PTR, _U64, _PTR, _U32, _PTR, _U64, _PTR, _PTR, _PTR]),
    "cniic_zip_back_image_measure_batch": (_I32, [_PTR, _PTR, _PTR, _PTR, _PTR, _U32, _PTR, _PTR, _U64, _PTR]),
    "cniic_hilbert_linearize_count": (_I32, [_I32, _U32, _U32, _PTR]),
    "cniic_hilbert_linearize_as": (_I32, [_PTR, _I32, _PTR, _U32, _U32, _PTR, _U64, _PTR]),
    "cniic_channel_diff_hist": (_I32, [_PTR, _PTR, _U64, _PTR]),
    "cniic_cc_finish_frames_var": (_I32, [_PTR, _PTR, _PTR, _PTR, _U32, _PTR, _U64, _PTR, _PTR]),
    "cniic_cc_palette": (_I32, [_PTR, _PTR, _PTR]),
    "cniic_palette_create": (_I32, [_PTR, _PTR, _U32, _PTR]),
    "cniic_palette_destroy": (None, [_PTR]),
    "cniic_palette_label_bytes": (_U32, [_PTR]),
    "cniic_palette_labels": (_I32, [_PTR, _PTR, _U64, _PTR]),
    "cniic_palette_encode_frames_var": (_I32, [_PTR, _PTR, _PTR, _PTR, _U32, _PTR, _U64, _PTR]),
    "cniic_kmeans_rgbw_from": (_I32, [_PTR, _PTR, _PTR, _U64, _U32, _PTR, _PTR, _PTR, _PTR, _PTR, _PTR]),
    "cniic_kmeans_xyrgb_from": (_I32, [_PTR, _PTR, _U32, _U32, _U32, _PTR, _PTR, _PTR, _PTR, _PTR, _PTR]),
    "cniic_cc_set_centroids": (_I32, [_PTR, _PTR]),
    "cniic_codec_encode_warm": (_I32, [_PTR, _STR, _PTR, _PTR, _PTR, _U32, _U32, _PTR, _U64, _PTR, _PTR, _PTR]),
    "cniic_palette_fit_frames_var": (_I32, [_PTR, _PTR, _PTR, _PTR, _U32, _PTR, _PTR]),
    "cniic_surface_span": (_I32, [_PTR, _PTR, _PTR]),
    "cniic_frames_from_surfaces": (_I32, [_PTR, _PTR, _PTR, _U32, _PTR, _PTR]),
    "cniic_frames_to_surfaces": (_I32, [_PTR, _PTR, _PTR, _PTR, _U32, _PTR, _U32]),
}
SYMBOLS = list(PROTOTYPES)


def lib():
    """Load libcniic_hip.so and declare every function of PROTOTYPES it exports; raise loudly if it has not been built (no CPU fallback
    exists)."""
    global _lib
    if _lib is None:
        p = lib_path()
        if not os.path.exists(p):
            raise ImportError("%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                              "or `make -C cniic_amd/csrc` (hipcc --offload-arch=gfx950)" % p)
        L = C.CDLL(p)
        for name, (restype, argtypes) in PROTOTYPES.items():
            if hasattr(L, name):   # (CNIIC_LIB_FILE may name an older build of the library, for a comparison: it lacks the newer calls)
                fn = getattr(L, name)
                fn.restype, fn.argtypes = restype, argtypes
        _lib = L
    return _lib


def _ptr(x):
    """numpy array (host) / torch tensor (device or host) / bytes / bytearray (its own buffer, not a copy) / int address / None -> c_void_p"""
    if x is None:
        return C.c_void_p(0)
    if isinstance(x, np.ndarray):
        assert x.flags["C_CONTIGUOUS"]
        return C.c_void_p(x.ctypes.data)
    if hasattr(x, "data_ptr"):
        assert x.is_contiguous()
        return C.c_void_p(x.data_ptr())
    if isinstance(x, bytes):
        return C.cast(C.c_char_p(x), C.c_void_p)
    if isinstance(x, bytearray):
        return C.c_void_p(C.addressof((C.c_char * len(x)).from_buffer(x)))
    return C.c_void_p(int(x))


def _count(x):
    """elements of a numpy array or a tensor"""
    return x.numel() if hasattr(x, "numel") else x.size


def _image(img, w, h):
    """an HxWx3 uint8 numpy array with its own w, h, or a device tensor / address with the w, h given -> (img, w, h)"""
    if isinstance(img, np.ndarray):
        img = np.ascontiguousarray(img, np.uint8)
        h, w = img.shape[:2]
    return img, w, h


def _host_bytes(data, n):
    """bytes / numpy array (host), or a device tensor / address with n given -> (data, n)"""
    if isinstance(data, (bytes, bytearray)):
        data = np.frombuffer(bytes(data), np.uint8)
    if n is None:
        n = _count(data)
    return data, n


def _array(ctype, xs, F):
    """the F numbers xs as a ctype[] the library reads (never of length 0)"""
    return (ctype * max(F, 1))(*[int(x) for x in xs])


def _out_buf(out, worst, cap=None):
    """where an encode-style call writes: the caller's `out` (cap bytes of it, default all) or, out None, a new buffer of `worst` bytes
    -> (out, cap, whether it is our own)"""
    if out is None:
        return np.empty(max(worst, 1), np.uint8), worst, True
    return out, (_count(out) if cap is None else cap), False


def _written(rc, out, ln, own):
    """what such a call returns beside rc: the bytes of our own buffer (none unless OK), or the length in the caller's"""
    if own:
        return out[:ln.value].tobytes() if rc == OK else b""
    return ln.value


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
        rc = self._L.cniic_ctx_create(device, stream or 0, C.byref(h))
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

    def _hist(self, fn, *head, tail=()):
        """count, then fill, of a histogram call fn(*head, keys, counts, cap, &n_unique, *tail) -> (keys, counts); what `tail` names is
        passed to the fill alone (the count gets NULL there)"""
        nu = C.c_uint64(0)
        self._check(fn(*head, None, None, 0, C.byref(nu), *[None] * len(tail)))
        keys = np.empty(max(nu.value, 1), np.uint32)
        counts = np.empty(max(nu.value, 1), np.uint64)
        self._check(fn(*head, _ptr(keys), _ptr(counts), keys.size, C.byref(nu), *tail))
        return keys[:nu.value], counts[:nu.value]

    def _decode_image(self, dims, allow, fn, *head):
        """the tail of a decode of a host stream into a new image: dims = the (w, h) the stream claims, or None; fn(*head, rgb, cap, &w, &h)
        decodes it -> (rc, HxWx3 image or None)"""
        if dims is None:
            return DECODE, None
        w, h = dims
        if w * h > (1 << 28):
            return CAPACITY, None
        out = np.zeros((max(w * h, 1), 3), np.uint8)
        cw, ch = C.c_uint32(0), C.c_uint32(0)
        rc = self._check(fn(*head, _ptr(out), out.size, C.byref(cw), C.byref(ch)), allow)
        if rc != OK:
            return rc, None
        return rc, out[:w * h].reshape(h, w, 3)

    def set_opt(self, opt, value):
        """cniic_ctx_set_opt: a route switch / threshold for this context (value None: back to the environment's / the default)"""
        if value is None:
            self._check(self._L.cniic_ctx_unset_opt(self.h, opt))
        else:
            self._check(self._L.cniic_ctx_set_opt(self.h, opt, value))

    def set_scan(self, w, h, xy):
        """cniic_ctx_set_scan: inject the scan of w x h images (xy: (w h, 2) uint32 positions, or None for the built-in one)"""
        if xy is not None and isinstance(xy, np.ndarray):
            xy = np.ascontiguousarray(xy, np.uint32)
        self._check(self._L.cniic_ctx_set_scan(self.h, w, h, _ptr(xy)))

    def get_opt(self, opt):
        v = C.c_uint64(0)
        self._check(self._L.cniic_ctx_get_opt(self.h, opt, C.byref(v)))
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
        return self._hist(self._L.cniic_hist_rgb24, self.h, _ptr(rgb), npx)

    def hist_syms(self, kind, syms):
        syms = np.ascontiguousarray(syms, np.uint32)
        return self._hist(self._L.cniic_hist_syms, self.h, kind, _ptr(syms), syms.size)

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
            rc = self._L.cniic_kmeans_rgbw(self.h, _ptr(keys), _ptr(weight), U, K, C.byref(o),
                                           _ptr(cent), _ptr(labels), _ptr(members), C.byref(st))
        else:
            init = np.ascontiguousarray(init, np.uint8).reshape(K, 3)
            rc = self._L.cniic_kmeans_rgbw_from(self.h, _ptr(keys), _ptr(weight), U, K, C.byref(o), _ptr(init),
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
        self._check(self._L.cniic_kmeans_step_rgbw(self.h, _ptr(keys), _ptr(weight), keys.size, K,
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
            rc = self._L.cniic_kmeans_xyrgb(self.h, _ptr(img), w, h, K, C.byref(o),
                                            _ptr(cent), _ptr(labels), _ptr(members), C.byref(st))
        else:
            init = np.ascontiguousarray(init, COLORPOS).reshape(K)
            rc = self._L.cniic_kmeans_xyrgb_from(self.h, _ptr(img), w, h, K, C.byref(o), _ptr(init),
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
        self._check(self._L.cniic_kmeans_step_xyrgb(self.h, _ptr(img), w, h, K, _ptr(cent),
                                                    _ptr(labels), _ptr(sums), _ptr(wsum), _ptr(members), C.byref(ch)))
        return dict(labels=labels, sums=sums, wsum=wsum, members=members, changed=ch.value)

    def remap_rgb(self, img, keys, labels, centroids):
        img = np.ascontiguousarray(img, np.uint8)
        keys = np.ascontiguousarray(keys, np.uint32)
        labels = np.ascontiguousarray(labels, np.uint32)
        cent = np.ascontiguousarray(centroids, np.uint8)
        out = np.empty_like(img)
        self._check(self._L.cniic_remap_rgb(self.h, _ptr(img), img.size // 3, _ptr(keys), _ptr(labels),
                                            keys.size, _ptr(cent), cent.shape[0], _ptr(out)))
        return out

    # ---- Hilbert
    def hilbert_xy(self, w, h):
        xy = np.zeros((max(w * h, 1), 2), np.uint32)
        self._check(self._L.cniic_hilbert_xy(self.h, w, h, _ptr(xy)))
        return xy[:w * h]

    def hilbert_linearize(self, img):
        img = np.ascontiguousarray(img, np.uint8)
        h, w = img.shape[:2]
        out = np.empty((h * w, 3), np.uint8)
        self._check(self._L.cniic_hilbert_linearize(self.h, _ptr(img), w, h, _ptr(out)))
        return out

    def hilbert_linearize_as(self, img, method, w=None, h=None, out=None, allow=()):
        """cniic_hilbert_linearize_as: method "rect" | "small" | "large" (or a CNIIC_LIN_* number).  img: HxWx3 uint8 numpy array, or a
        device tensor / address with w, h given.  -> the (npx, 3) pixels when out is None, else (rc, npx) with out (numpy array, device
        tensor) filled; with CAPACITY allowed: npx = the pixels needed"""
        img, w, h = _image(img, w, h)
        m = LIN_METHODS[method] if isinstance(method, str) else int(method)
        own = out is None
        if own:
            out = np.empty((max(linearize_count(m, w, h), 1), 3), np.uint8)
        n = C.c_uint64(0)
        rc = self._check(self._L.cniic_hilbert_linearize_as(self.h, m, _ptr(img), w, h, _ptr(out), _count(out) // 3, C.byref(n)), allow)
        if own:
            return out[:n.value]
        return rc, n.value

    def channel_diff_hist(self, lin, npx=None, out=None):
        """cniic_channel_diff_hist: lin = (n, 3) uint8 numpy array, or a device tensor / address (npx: its pixels, default all of it)
        -> int64 [3, 511] array, or `out` (a device tensor / numpy array of 3 x 511 64-bit words) filled"""
        if isinstance(lin, np.ndarray):
            lin = np.ascontiguousarray(lin, np.uint8)
        if npx is None:
            npx = _count(lin) // 3
        res = np.zeros((3, 511), np.int64) if out is None else out
        self._check(self._L.cniic_channel_diff_hist(self.h, _ptr(lin) if npx else None, npx, _ptr(res)))
        return res

    def hilbert_delta(self, img):
        img = np.ascontiguousarray(img, np.uint8)
        h, w = img.shape[:2]
        syms = np.empty(h * w, np.uint32)
        self._check(self._L.cniic_hilbert_delta(self.h, _ptr(img), w, h, _ptr(syms)))
        return syms

    def hilbert_delta_hist(self, img, want_syms=False, w=None, h=None):
        img, w, h = _image(img, w, h)
        syms = np.empty(h * w, np.uint32) if want_syms else None
        keys, counts = self._hist(self._L.cniic_hilbert_delta_hist, self.h, _ptr(img), w, h, tail=(_ptr(syms),))
        return keys, counts, syms

    # ---- Huffman
    def huf_encode_all(self, kind, syms):
        syms = np.ascontiguousarray(syms, np.uint32)
        out, cap, own = _out_buf(None, 64 + syms.size * 20)
        ln = C.c_uint64(0)
        rc = self._check(self._L.cniic_huf_encode_all(self.h, kind, _ptr(syms), syms.size, _ptr(out), cap, C.byref(ln)))
        return _written(rc, out, ln, own)

    def huf_size(self, kind, counts):
        counts = np.ascontiguousarray(counts, np.uint64)
        nb = C.c_uint64(0)
        rc = self._L.cniic_huf_size(kind, _ptr(counts), counts.size, C.byref(nb))
        if rc != OK:
            raise CniicError(rc)
        return nb.value

    # ---- codecs
    def encode(self, expr, img, w=None, h=None, out=None, seed=0, max_iters=0, flags=0, allow=()):
        """Codec::encode.  img: HxWx3 uint8 numpy array, or a device tensor / address with w,h given."""
        img, w, h = _image(img, w, h)
        out, cap, own = _out_buf(out, 64 + w * h * 16 + (1 << 16))
        ln = C.c_uint64(0)
        st = KmStats()
        o = self._opts(seed, max_iters, flags)
        rc = self._check(self._L.cniic_codec_encode_opts(self.h, expr.encode(), C.byref(o), _ptr(img), w, h,
                                                         _ptr(out), cap, C.byref(ln), C.byref(st)), allow)
        return rc, _written(rc, out, ln, own), st.as_dict()

    def encode_warm(self, expr, img, init, w=None, h=None, out=None, seed=0, max_iters=0, flags=0, allow=()):
        """cniic_codec_encode_warm: Codec::encode of cluster-colors(K) / voronoi(K) with the K-means started from init ((K, 3) uint8, or K
        COLORPOS entries) -> (rc, stream or its length as encode, stats, final centroids in init's layout: the next frame's init)"""
        img, w, h = _image(img, w, h)
        init = np.ascontiguousarray(init)
        if init.dtype != COLORPOS:
            init = np.ascontiguousarray(init, np.uint8).reshape(-1, 3)
        cent = np.zeros_like(init)
        out, cap, own = _out_buf(out, 64 + w * h * 16 + (1 << 16) + 19 * init.shape[0])
        ln = C.c_uint64(0)
        st = KmStats()
        o = self._opts(seed, max_iters, flags)
        rc = self._check(self._L.cniic_codec_encode_warm(self.h, expr.encode(), C.byref(o), _ptr(init), _ptr(img), w, h,
                                                         _ptr(out), cap, C.byref(ln), _ptr(cent), C.byref(st)), allow)
        return rc, _written(rc, out, ln, own), st.as_dict(), cent

    def hilbert_rle_approx_encode(self, d, img, w=None, h=None, out=None, allow=()):
        """cniic_hilbert_rle_approx_encode: Hilbert { compress: RLE(d) }::encode for an f64 d (d == 0.0: the `hilbert(rle)` stream).
        img: HxWx3 uint8 numpy array, or a device tensor / address with w,h given.  -> (rc, bytes) when out is None, else (rc, length)"""
        img, w, h = _image(img, w, h)
        out, cap, own = _out_buf(out, 8 + w * h * 12)
        ln = C.c_uint64(0)
        rc = self._check(self._L.cniic_hilbert_rle_approx_encode(self.h, d, _ptr(img), w, h, _ptr(out), cap, C.byref(ln)), allow)
        return rc, _written(rc, out, ln, own)

    # ---- the dictionary coder
    def zip_dict_encode(self, data, n=None, out=None, allow=()):
        """cniic_zip_dict_encode: data = bytes / numpy array (host), or a device tensor / address with n given.
        -> (rc, bytes) when out is None, else (rc, length)"""
        data, n = _host_bytes(data, n)
        out, cap, own = _out_buf(out, 2 * n + 4)
        ln = C.c_uint64(0)
        rc = self._check(self._L.cniic_zip_dict_encode(self.h, _ptr(data) if n else None, n, _ptr(out), cap, C.byref(ln)), allow)
        return rc, _written(rc, out, ln, own)

    def zip_dict_decode(self, data, n=None, out=None, cap=None, allow=()):
        """cniic_zip_dict_decode -> (rc, bytes) when out is None (cap: the most bytes the text may have, default 64 MiB), else (rc, length;
        with CAPACITY: the bytes needed)"""
        data, n = _host_bytes(data, n)
        out, cap, own = _out_buf(out, (64 << 20) if cap is None else cap, cap)
        ln = C.c_uint64(0)
        rc = self._check(self._L.cniic_zip_dict_decode(self.h, _ptr(data) if n else None, n, _ptr(out), cap, C.byref(ln)), allow)
        return rc, _written(rc, out, ln, own)

    def hilbert_zip_encode(self, img, w=None, h=None, out=None, allow=()):
        """cniic_hilbert_zip_encode.  img: HxWx3 uint8 numpy array, or a device tensor / address with w,h given.
        -> (rc, bytes) when out is None, else (rc, length)"""
        img, w, h = _image(img, w, h)
        out, cap, own = _out_buf(out, 8 + w * h * 22 + 4)
        ln = C.c_uint64(0)
        rc = self._check(self._L.cniic_hilbert_zip_encode(self.h, _ptr(img), w, h, _ptr(out), cap, C.byref(ln)), allow)
        return rc, _written(rc, out, ln, own)

    def hilbert_zip_decode(self, data, allow=()):
        """cniic_hilbert_zip_decode of a host stream -> (rc, HxWx3 image or None)"""
        raw = np.frombuffer(bytes(data), np.uint8)
        dims = None
        if raw.size >= 8:
            dims = int.from_bytes(raw[0:4].tobytes(), "little"), int.from_bytes(raw[4:8].tobytes(), "little")
        return self._decode_image(dims, allow, self._L.cniic_hilbert_zip_decode, self.h, _ptr(raw), raw.size)

    def hilbert_zip_decode_into(self, data, nbytes, out, cap=None, allow=()):
        """cniic_hilbert_zip_decode with caller-owned buffers (device tensors, numpy arrays or addresses) -> (rc, w, h)"""
        cw, ch = C.c_uint32(0), C.c_uint32(0)
        rc = self._check(self._L.cniic_hilbert_zip_decode(self.h, _ptr(data), nbytes, _ptr(out), _count(out) if cap is None else cap, C.byref(cw), C.byref(ch)), allow)
        return rc, cw.value, ch.value

    def hilbert_zip_encode_batch_var(self, images, offs, ws, hs, out, stride, allow=()):
        """cniic_hilbert_zip_encode_batch_var: the layout of encode_batch_var -> (rc, list of lengths, list of per-image status codes)"""
        F = len(offs)
        n = max(F, 1)
        lens, rcs = (C.c_uint64 * n)(), (C.c_int32 * n)()
        rc = self._check(self._L.cniic_hilbert_zip_encode_batch_var(self.h, _ptr(images), _array(C.c_uint64, offs, F), _array(C.c_uint32, ws, F),
                                                                    _array(C.c_uint32, hs, F), F, _ptr(out), stride, lens, rcs), allow)
        return rc, [int(lens[f]) for f in range(F)], [int(rcs[f]) for f in range(F)]

    def hilbert_zip_decode_batch(self, streams, stride, lens, F, out, img_stride, allow=()):
        """cniic_hilbert_zip_decode_batch: the layout of decode_batch -> (rc, list of widths, list of heights, list of per-frame status codes)"""
        n = max(F, 1)
        ws, hs, rcs = (C.c_uint32 * n)(), (C.c_uint32 * n)(), (C.c_int32 * n)()
        rc = self._check(self._L.cniic_hilbert_zip_decode_batch(self.h, _ptr(streams), stride, _array(C.c_uint64, lens, F), F, _ptr(out), img_stride,
                                                                ws, hs, rcs), allow)
        return rc, [int(ws[f]) for f in range(F)], [int(hs[f]) for f in range(F)], [int(rcs[f]) for f in range(F)]

    def hilbert_zip_measure_batch(self, images, offs, ws, hs, out=None, stride=0, allow=()):
        """cniic_hilbert_zip_measure_batch: measure_batch for Hilbert { compress: Zip } -> (rc, list of row dicts, list of stream lengths)"""
        F = len(offs)
        n = max(F, 1)
        rows, lens = (MeasureRow * n)(), (C.c_uint64 * n)()
        rc = self._check(self._L.cniic_hilbert_zip_measure_batch(self.h, _ptr(images), _array(C.c_uint64, offs, F), _array(C.c_uint32, ws, F),
                                                                 _array(C.c_uint32, hs, F), F, rows, _ptr(out), stride, lens), allow)
        return rc, [rows[f].as_dict() for f in range(F)], [int(lens[f]) for f in range(F)]

    # ---- the look-back coder
    def zip_back_encode(self, data, n=None, out=None, allow=()):
        """cniic_zip_back_encode: data = bytes / numpy array (host), or a device tensor / address with n given.
        -> (rc, bytes) when out is None, else (rc, length; with CAPACITY: the bytes needed)"""
        data, n = _host_bytes(data, n)
        out, cap, own = _out_buf(out, n + n // 4 + 16)
        ln = C.c_uint64(0)
        rc = self._check(self._L.cniic_zip_back_encode(self.h, _ptr(data) if n else None, n, _ptr(out), cap, C.byref(ln)), allow)
        return rc, _written(rc, out, ln, own)

    def zip_back_decode(self, data, n=None, out=None, cap=None, allow=()):
        """cniic_zip_back_decode -> (rc, bytes) when out is None (cap: the most bytes the text may have, default 64 MiB), else (rc, length;
        with CAPACITY: the bytes needed)"""
        data, n = _host_bytes(data, n)
        out, cap, own = _out_buf(out, (64 << 20) if cap is None else cap, cap)
        ln = C.c_uint64(0)
        rc = self._check(self._L.cniic_zip_back_decode(self.h, _ptr(data) if n else None, n, _ptr(out), cap, C.byref(ln)), allow)
        return rc, _written(rc, out, ln, own)

    def zip_back_image_encode(self, img, w=None, h=None, out=None, allow=()):
        """cniic_zip_back_image_encode.  img: HxWx3 uint8 numpy array, or a device tensor / address with w,h given.
        -> (rc, bytes) when out is None, else (rc, length)"""
        img, w, h = _image(img, w, h)
        out, cap, own = _out_buf(out, 14 * w * h + 32)
        ln = C.c_uint64(0)
        rc = self._check(self._L.cniic_zip_back_image_encode(self.h, _ptr(img), w, h, _ptr(out), cap, C.byref(ln)), allow)
        return rc, _written(rc, out, ln, own)

    def zip_back_image_decode(self, data, allow=()):
        """cniic_zip_back_image_decode of a host stream -> (rc, HxWx3 image or None)"""
        raw = np.frombuffer(bytes(data), np.uint8)
        return self._decode_image(zip_back_dims(raw), allow, self._L.cniic_zip_back_image_decode, self.h, _ptr(raw), raw.size)

    def zip_back_image_decode_into(self, data, nbytes, out, allow=()):
        """cniic_zip_back_image_decode with caller-owned buffers (device tensors, numpy arrays or addresses) -> (rc, w, h)"""
        cw, ch = C.c_uint32(0), C.c_uint32(0)
        rc = self._check(self._L.cniic_zip_back_image_decode(self.h, _ptr(data), nbytes, _ptr(out), _count(out), C.byref(cw), C.byref(ch)), allow)
        return rc, cw.value, ch.value

    def zip_back_encode_batch_var(self, images, offs, ws, hs, out, stride, allow=()):
        """cniic_zip_back_image_encode_batch_var: the layout of encode_batch_var -> (rc, list of lengths, list of per-image status codes)"""
        F = len(offs)
        n = max(F, 1)
        lens, rcs = (C.c_uint64 * n)(), (C.c_int32 * n)()
        rc = self._check(self._L.cniic_zip_back_image_encode_batch_var(self.h, _ptr(images), _array(C.c_uint64, offs, F), _array(C.c_uint32, ws, F),
                                                                       _array(C.c_uint32, hs, F), F, _ptr(out), stride, lens, rcs), allow)
        return rc, [int(lens[f]) for f in range(F)], [int(rcs[f]) for f in range(F)]

    def zip_back_decode_batch(self, streams, stride, lens, F, out, img_stride, allow=()):
        """cniic_zip_back_image_decode_batch: the layout of decode_batch -> (rc, list of widths, list of heights, list of per-frame status codes)"""
        n = max(F, 1)
        ws, hs, rcs = (C.c_uint32 * n)(), (C.c_uint32 * n)(), (C.c_int32 * n)()
        rc = self._check(self._L.cniic_zip_back_image_decode_batch(self.h, _ptr(streams), stride, _array(C.c_uint64, lens, F), F, _ptr(out), img_stride,
                                                                   ws, hs, rcs), allow)
        return rc, [int(ws[f]) for f in range(F)], [int(hs[f]) for f in range(F)], [int(rcs[f]) for f in range(F)]

    def zip_back_measure_batch(self, images, offs, ws, hs, out=None, stride=0, allow=()):
        """cniic_zip_back_image_measure_batch: measure_batch for Zip::Back -> (rc, list of row dicts, list of stream lengths)"""
        F = len(offs)
        n = max(F, 1)
        rows, lens = (MeasureRow * n)(), (C.c_uint64 * n)()
        rc = self._check(self._L.cniic_zip_back_image_measure_batch(self.h, _ptr(images), _array(C.c_uint64, offs, F), _array(C.c_uint32, ws, F),
                                                                    _array(C.c_uint32, hs, F), F, rows, _ptr(out), stride, lens), allow)
        return rc, [rows[f].as_dict() for f in range(F)], [int(lens[f]) for f in range(F)]

    def encode_batch(self, expr, frames, w, h, F, out, stride, seed=0, max_iters=0, flags=0, allow=()):
        """cniic_codec_encode_batch: F images (one contiguous [F][h][w][3] buffer), each encoded on its own (its own palette), image f's
        stream at out[f * stride:].  -> (rc, list of F lengths, list of F per-image status codes, list of F stats dicts)"""
        lens = (C.c_uint64 * F)()
        rcs = (C.c_int32 * F)()
        sts = (KmStats * F)()
        o = self._opts(seed, max_iters, flags)
        rc = self._check(self._L.cniic_codec_encode_batch(self.h, expr.encode(), C.byref(o), _ptr(frames), w, h, F,
                                                          _ptr(out), stride, lens, rcs, sts), allow)
        return rc, [int(x) for x in lens], [int(x) for x in rcs], [s.as_dict() for s in sts]

    def encode_batch_var(self, expr, images, offs, ws, hs, out, stride, seed=0, max_iters=0, flags=0, allow=()):
        """cniic_codec_encode_batch_var: len(offs) images of different sizes in one buffer (image f is ws[f] x hs[f] at images[offs[f]:]),
        each encoded on its own, image f's stream at out[f * stride:].  images / out: device tensors, numpy arrays or addresses.
        -> (rc, list of lengths, list of per-image status codes, list of stats dicts)"""
        F = len(offs)
        n = max(F, 1)
        lens, rcs, sts = (C.c_uint64 * n)(), (C.c_int32 * n)(), (KmStats * n)()
        o = self._opts(seed, max_iters, flags)
        rc = self._check(self._L.cniic_codec_encode_batch_var(self.h, expr.encode(), C.byref(o), _ptr(images), _array(C.c_uint64, offs, F),
                                                              _array(C.c_uint32, ws, F), _array(C.c_uint32, hs, F), F, _ptr(out),
                                                              stride, lens, rcs, sts), allow)
        return rc, [int(lens[f]) for f in range(F)], [int(rcs[f]) for f in range(F)], [sts[f].as_dict() for f in range(F)]

    def mse_batch_var(self, a, a_offs, b, b_offs, npx):
        """cniic_mse_batch_var: the MSE of len(npx) pairs of different sizes (pair f: npx[f] pixels at a[a_offs[f]:] and b[b_offs[f]:])
        -> list of floats"""
        F = len(npx)
        v = (C.c_double * max(F, 1))()
        self._check(self._L.cniic_mse_batch_var(self.h, _ptr(a), _array(C.c_uint64, a_offs, F), _ptr(b), _array(C.c_uint64, b_offs, F),
                                                _array(C.c_uint64, npx, F), F, v))
        return [float(v[f]) for f in range(F)]

    def frames_from_surfaces(self, src, surfaces, rgb, img_offs, allow=()):
        """cniic_frames_from_surfaces: surface f of src (a list of Surface) -> packed RGB24 at rgb[img_offs[f]:], all frames in one launch.
        src / rgb: device tensors, numpy arrays or addresses.  With device memory on both sides the call is asynchronous on the
        context's stream (sync() waits).  -> rc"""
        F = len(surfaces)
        return self._check(self._L.cniic_frames_from_surfaces(self.h, _ptr(src), (Surface * max(F, 1))(*surfaces), F, _ptr(rgb),
                                                              _array(C.c_uint64, img_offs, F)), allow)

    def frames_to_surfaces(self, rgb, img_offs, surfaces, dst, alpha=255, allow=()):
        """cniic_frames_to_surfaces: packed RGB24 at rgb[img_offs[f]:] -> surface f of dst (RGB8 / BGR8 / RGBA8 / BGRA8; the alpha byte
        written is `alpha`), the pitch's padding untouched.  -> rc"""
        F = len(surfaces)
        return self._check(self._L.cniic_frames_to_surfaces(self.h, _ptr(rgb), _array(C.c_uint64, img_offs, F), (Surface * max(F, 1))(*surfaces),
                                                            F, _ptr(dst), alpha), allow)

    def measure_batch(self, expr, images, offs, ws, hs, out=None, stride=0, seed=0, max_iters=0, flags=0, allow=()):
        """cniic_codec_measure_batch: encode, size, ratio, decode, MSE and the lossless check of every image in one call (the body of
        bench::measure_all's loop).  out (optional): stream f is copied to out[f * stride:].
        -> (rc, list of row dicts, list of stream lengths)"""
        F = len(offs)
        n = max(F, 1)
        rows, lens = (MeasureRow * n)(), (C.c_uint64 * n)()
        o = self._opts(seed, max_iters, flags)
        rc = self._check(self._L.cniic_codec_measure_batch(self.h, expr.encode(), C.byref(o), _ptr(images), _array(C.c_uint64, offs, F),
                                                           _array(C.c_uint32, ws, F), _array(C.c_uint32, hs, F), F, rows, _ptr(out),
                                                           stride, lens), allow)
        return rc, [rows[f].as_dict() for f in range(F)], [int(lens[f]) for f in range(F)]

    def decode(self, expr, data, allow=()):
        raw = np.frombuffer(bytes(data), np.uint8)
        return self._decode_image(stream_dims(expr, raw), allow, self._L.cniic_codec_decode, self.h, expr.encode(), _ptr(raw), raw.size)

    def decode_into(self, expr, data, nbytes, out, allow=()):
        """Codec::decode with caller-owned buffers: data = the stream (device tensor / address / numpy array), nbytes of it;
        out = a uint8 buffer (device tensor or numpy array) that receives the w x h x 3 image.  -> (rc, w, h)"""
        cw, ch = C.c_uint32(0), C.c_uint32(0)
        rc = self._check(self._L.cniic_codec_decode(self.h, expr.encode(), _ptr(data), nbytes, _ptr(out), _count(out),
                                                    C.byref(cw), C.byref(ch)), allow)
        return rc, cw.value, ch.value

    def decode_batch(self, expr, streams, stride, lens, F, out, img_stride, allow=()):
        """cniic_codec_decode_batch: F streams (stream f at streams[f * stride:], lens[f] bytes -- what encode_batch wrote), image f into
        out[f * img_stride:] (img_stride bytes at most).  streams / out: device tensors, numpy arrays or addresses.
        -> (rc, list of F widths, list of F heights, list of F per-frame status codes)"""
        ws, hs, rcs = (C.c_uint32 * F)(), (C.c_uint32 * F)(), (C.c_int32 * F)()
        rc = self._check(self._L.cniic_codec_decode_batch(self.h, expr.encode(), _ptr(streams), stride, _array(C.c_uint64, lens, F), F, _ptr(out),
                                                          img_stride, ws, hs, rcs), allow)
        return rc, [int(x) for x in ws], [int(x) for x in hs], [int(x) for x in rcs]

    def mse_batch(self, a, b, npx, F):
        """cniic_mse_batch: the MSE of F image pairs of npx pixels each (pair f at a[f * npx * 3:], b[f * npx * 3:]) -> list of F floats"""
        if isinstance(a, np.ndarray):
            a = np.ascontiguousarray(a, np.uint8)
        if isinstance(b, np.ndarray):
            b = np.ascontiguousarray(b, np.uint8)
        v = (C.c_double * max(F, 1))()
        self._check(self._L.cniic_mse_batch(self.h, _ptr(a), _ptr(b), npx, F, v))
        return [float(v[i]) for i in range(F)]

    def mse(self, a, b):
        """cniic_mse of two RGB8 images of the same size: numpy arrays, or uint8 tensors (on the device: read in place, no copy)"""
        a = a.contiguous() if hasattr(a, "data_ptr") else np.ascontiguousarray(a, np.uint8)
        b = b.contiguous() if hasattr(b, "data_ptr") else np.ascontiguousarray(b, np.uint8)
        na, nb = _count(a), _count(b)
        if na != nb:
            raise ValueError("mse: images of %d and %d bytes" % (na, nb))
        v = C.c_double(0)
        self._check(self._L.cniic_mse(self.h, _ptr(a), _ptr(b), na // 3, C.byref(v)))
        return v.value

    def synth_image(self, kind, seed, w, h, out=None):
        if out is None:
            out = np.empty((h, w, 3), np.uint8)
        self._check(self._L.cniic_synth_image(self.h, kind, seed, w, h, _ptr(out)))
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
            K = _count(centroids) // 3
        self.ctx = ctx
        self.K = int(K)
        self.h = None
        h = C.c_void_p()
        ctx._check(ctx._L.cniic_palette_create(ctx.h, _ptr(centroids), self.K, C.byref(h)))
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
            npx = _count(rgb) // 3
        if out is None:
            out = np.empty(max(npx, 1), np.uint8 if self.label_bytes == 1 else np.uint16)[:npx]
        self.ctx._check(self.ctx._L.cniic_palette_labels(self.h, _ptr(rgb) if npx else None, npx, _ptr(out)))
        return out

    def encode_frames_var(self, frames_flat, ws, hs, out, stride, allow=()):
        """cniic_palette_encode_frames_var: len(ws) frames of different sizes, back to back in frames_flat (device tensor, numpy array or
        address), frame f's stream at out[f * stride:] -> list of lengths; with a status in `allow`: (status, lengths)"""
        F = len(ws)
        lens = (C.c_uint64 * max(F, 1))()
        rc = self.ctx._check(self.ctx._L.cniic_palette_encode_frames_var(self.h, _ptr(frames_flat), _array(C.c_uint32, ws, F), _array(C.c_uint32, hs, F),
                                                                         F, _ptr(out), stride, lens), allow)
        if allow:
            return rc, [int(lens[f]) for f in range(F)]
        return [int(lens[f]) for f in range(F)]


    def fit_frames_var(self, frames_flat, ws, hs, want_pixels=True, allow=()):
        """cniic_palette_fit_frames_var: len(ws) frames of different sizes, back to back in frames_flat (device tensor, numpy array or
        address) -> (sse: uint64[F], the exact summed squared distance of every frame's pixels to their entries; pixels: uint64[K], the
        pixels of all frames per entry, or None); with a status in `allow`: (status, sse, pixels)"""
        F = len(ws)
        sse = np.zeros(max(F, 1), np.uint64)
        pixels = np.zeros(self.K, np.uint64) if want_pixels else None
        rc = self.ctx._check(self.ctx._L.cniic_palette_fit_frames_var(self.h, _ptr(frames_flat), _array(C.c_uint32, ws, F), _array(C.c_uint32, hs, F),
                                                                      F, _ptr(sse), _ptr(pixels)), allow)
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
    rc = lib().cniic_hilbert_linearize_count(m, w, h, C.byref(n))
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
    rc = lib().cniic_zip_dict_dims(_ptr(raw) if raw.size else None, raw.size, C.byref(w), C.byref(h))
    return (w.value, h.value) if rc == OK else None


def zip_back_dims(data):
    """cniic_zip_back_dims: (w, h) from the first symbols of a zip-back stream in host memory, or None"""
    raw = data if isinstance(data, np.ndarray) else np.frombuffer(bytes(data), np.uint8)
    w, h = C.c_uint32(0), C.c_uint32(0)
    rc = lib().cniic_zip_back_dims(_ptr(raw) if raw.size else None, raw.size, C.byref(w), C.byref(h))
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
        rc = lib().cniic_codec_name(expr.encode(), buf, cap)
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
