"""bench.py --dump-outputs on CPU: what it writes (float32 .npy, bounded size, the same indices run after run) and which runs refuse it."""
import os
import subprocess
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def test_dump_outputs_is_a_fixed_float32_sample(tmp_path):
    import bench
    n = 3 * bench.DUMP_SAMPLE + 17
    params = torch.arange(n, dtype=torch.float32)
    store = types.SimpleNamespace(params=params, grads=-params)
    losses = torch.linspace(0, 1, 9)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), losses, store)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["grads_sample.npy", "losses.npy", "params_sample.npy"]
    total = 0
    for f in names:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == np.float32 and np.array_equal(a, b), f
        total += a.nbytes
    assert total <= 64 << 20
    p, g = np.load(tmp_path / "a" / "params_sample.npy"), np.load(tmp_path / "a" / "grads_sample.npy")
    assert p.shape == (bench.DUMP_SAMPLE,) and np.array_equal(g, -p)          # one index set for both buffers
    assert np.all(np.diff(p) >= 0) and p.max() > 2 * bench.DUMP_SAMPLE          # sorted, spread over the whole buffer
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "losses.npy"), losses.numpy())


def test_small_buffers_are_written_whole(tmp_path):
    import bench
    store = types.SimpleNamespace(params=torch.arange(1000.0), grads=torch.ones(1000))
    bench.dump_outputs(str(tmp_path), torch.zeros(9), store)
    np.testing.assert_array_equal(np.load(tmp_path / "params_sample.npy"), np.arange(1000.0, dtype=np.float32))


def test_dump_outputs_refused_outside_the_fixed_shape_step(tmp_path):
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    for extra in (["--shapes", "voc"], ["--config", "eval"]):
        r = subprocess.run([sys.executable, BENCH, "--dump-outputs", str(tmp_path / "x")] + extra, capture_output=True, text=True,
                           timeout=300, env=e)
        assert r.returncode == 2 and r.stdout == "" and "--dump-outputs" in r.stderr, (extra, r.stderr[-500:])
        assert not os.path.exists(tmp_path / "x")
