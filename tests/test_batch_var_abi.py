"""CPU-side checks of the calls for batches of differently sized images (cniic_codec_encode_batch_var, cniic_mse_batch_var,
cniic_codec_measure_batch): declared, exported by both libraries, mirrored by the Python loader with the C struct's layout, and the
Python mirror's empty batches never reach the library."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cniic_codec_encode_batch_var", "cniic_mse_batch_var", "cniic_codec_measure_batch")


def test_new_symbols_declared_exported_and_listed():
    from cniic_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cniic_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint32_t\s+%s\s*\(" % name, text), name
        assert name in _lib.SYMBOLS
    for so in ("libcniic_hip.so", "libcniic_hip_testing.so"):
        L = C.CDLL(os.path.join(ROOT, "cniic_amd", so))
        for name in NEW:
            assert hasattr(L, name), (so, name)
    # the sentence above cniic_codec_encode_batch no longer claims the whole folder
    head = open(os.path.join(ROOT, "include", "cniic_hip.h")).read()
    assert "EQUALLY SIZED" in head[:head.index("int32_t cniic_codec_encode_batch(")][-1500:]


def test_measure_row_layout_equals_the_c_struct(tmp_path):
    from cniic_amd import _lib
    src = tmp_path / "row.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cniic_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(cniic_measure_row), offsetof(cniic_measure_row, compressed_size),\n'
                   '  offsetof(cniic_measure_row, compression_ratio), offsetof(cniic_measure_row, error), offsetof(cniic_measure_row, rc),\n'
                   '  offsetof(cniic_measure_row, lossless_mismatch), offsetof(cniic_measure_row, kmeans)); return 0; }\n')
    exe = tmp_path / "row"
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    R = _lib.MeasureRow
    want = [C.sizeof(R)] + [getattr(R, f).offset for f in ("compressed_size", "compression_ratio", "error", "rc", "lossless_mismatch", "kmeans")]
    assert got == want
    assert C.sizeof(_lib.KmStats) == 40 and C.sizeof(R) == 72


def test_empty_batches_do_not_touch_the_library(monkeypatch):
    from cniic_amd import _lib
    from cniic_amd.codec import AnyCodec, HilbertRleApprox
    codec = AnyCodec.from_str("cluster-colors(16)")

    def no_context(*a, **k):
        raise AssertionError("an empty batch made a context")
    monkeypatch.setattr(_lib, "Context", no_context)
    assert codec.encode_batch([]) == []
    assert codec.measure([]) == []
    assert HilbertRleApprox(2.0).encode_batch([]) == []


def test_harness_usage_names_the_flag():
    exe = os.path.join(ROOT, "tools", "cniic_bench")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--one-call" in r.stderr
