"""bench.py --dump-outputs DIR: after the timed steps, what the timed path computed in its last step as DIR/<name>.npy -- float32 /
float64, at most 64 MB in all, a fixed seeded sample of a longer output -- so that two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_dump_keeps_short_arrays_whole_and_samples_long_ones_at_fixed_positions(tmp_path):
    short = torch.arange(1000).to(torch.uint8)
    long_ = torch.from_numpy(np.random.default_rng(7).integers(0, 256, bench.DUMP_SAMPLE + 12345, dtype=np.uint8))
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"short": short, "long": long_}, {"iterations": 5, "lengths": [1, 2, 3]})
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["iterations.npy", "lengths.npy", "long.npy", "long_length.npy", "short.npy", "short_length.npy"]
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), n
        total += a.nbytes
    assert total <= bench.DUMP_LIMIT_BYTES
    assert np.array_equal(np.load(tmp_path / "a" / "short.npy"), short.numpy())
    assert np.array_equal(np.load(tmp_path / "a" / "lengths.npy"), [1, 2, 3])
    # the sample: the elements at sorted positions drawn from the fixed seed and the length
    s = np.load(tmp_path / "a" / "long.npy")
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(long_.numel(), bench.DUMP_SAMPLE, replace=False))
    assert np.load(tmp_path / "a" / "long_length.npy")[0] == long_.numel()
    assert np.array_equal(s, long_.numpy()[idx])


def test_dump_over_the_limit_is_refused_before_anything_is_written(tmp_path):
    with pytest.raises(AssertionError):
        bench.dump_outputs(str(tmp_path / "d"), {}, {"x": np.zeros(bench.DUMP_LIMIT_BYTES // 8 + 1)})
    assert not os.path.exists(tmp_path / "d")


@pytest.mark.gpu
def test_bench_dumps_the_stream_of_its_last_timed_step(tmp_path):
    """the default path (configs[1]) at a small size: the line reports the steps it was given, and the dumped stream is the one
    the library makes of the same image"""
    import cniic_amd
    from cniic_amd import _lib, synth
    W = H = 512
    K = 16
    env = dict(os.environ, CNIIC_USE_TESTING_LIB="0")   # bench.py runs on the release library
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--size", str(W), "--k", str(K), "--steps", "3", "--warmup", "1",
                        "--no-extras", "--cpu-sample", "0", "--dump-outputs", str(tmp_path)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.strip()][0])
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    assert line["roofline"] is None and "parity" not in line   # a plain run: the timed steps and nothing else (roofline, parity: --full)
    stream = np.load(tmp_path / "stream.npy")
    assert stream.dtype == np.float32 and stream.size == np.load(tmp_path / "stream_length.npy")[0]
    with cniic_amd.Context(0) as ctx:
        img = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
        ctx.synth_image(_lib.SYNTH_PHOTO, synth.SEED0 + 2, W, H, out=img)
        rc, data, st = ctx.encode("cluster-colors(%d)" % K, img.cpu().numpy())
    assert rc == 0
    assert np.array_equal(stream, np.frombuffer(data, np.uint8))
    assert np.load(tmp_path / "kmeans_iterations.npy")[0] == st["iterations"] == line["config"]["kmeans_iterations"]
