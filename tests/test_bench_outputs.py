"""``bench.py --dump-outputs DIR`` and the plain / ``--full`` split.

CPU: ``dump_outputs`` writes float32 ``.npy`` files and cuts arrays to a fixed, seeded sample when the
dump would pass its byte limit.  GPU: one plain run of the benchmark itself (3 timed steps) prints a
line with ``ms_per_step`` for exactly those steps, leaves the ``--full`` fields null and writes the
last timed step's loss, logits, parameters and buffers.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")


def _bench_module():
    import importlib.util

    spec = importlib.util.spec_from_file_location("dfd_bench", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_float32_and_seeded_sample(tmp_path, monkeypatch):
    bench = _bench_module()
    small = torch.arange(6, dtype=torch.float64).reshape(2, 3)
    big = torch.arange(100_000, dtype=torch.float32)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, {"small": small, "big": big})
    assert np.load(os.path.join(a, "small.npy")).dtype == np.float32
    np.testing.assert_array_equal(np.load(os.path.join(a, "small.npy")), small.numpy().astype(np.float32))
    np.testing.assert_array_equal(np.load(os.path.join(a, "big.npy")), big.numpy())  # under the limit: whole
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 64 << 10)
    bench.dump_outputs(a, {"small": small, "big": big})
    bench.dump_outputs(b, {"small": small, "big": big})
    sa, sb = np.load(os.path.join(a, "big.npy")), np.load(os.path.join(b, "big.npy"))
    assert sa.ndim == 1 and 0 < sa.size < big.numel()
    np.testing.assert_array_equal(sa, sb)  # the same sample every time
    assert np.all(np.diff(sa) > 0) and sa[-1] < 100_000  # distinct elements of the array, in order
    np.testing.assert_array_equal(np.load(os.path.join(a, "small.npy")), small.numpy().astype(np.float32))
    total = sum(os.path.getsize(os.path.join(a, f)) for f in os.listdir(a))
    assert total <= 64 << 10


@pytest.mark.gpu
def test_plain_bench_run_dumps_last_step(cuda, tmp_path):
    out = str(tmp_path / "dump")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", out],
                       capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["unit"] == "face-frames/s" and d["higher_is_better"] is True and d["dtype"] == "fp16"
    assert d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(256 * 1e3 / d["ms_per_step"], rel=1e-3)  # frames of one step / its time
    assert d["loss_finite"] is True
    assert d["pointwise"] is None and d["cpu_baseline"] is None  # measured only with --full
    got = {f[:-4]: np.load(os.path.join(out, f)) for f in os.listdir(out)}
    assert sorted(got) == ["buffers", "logits", "loss", "params"]
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())
    assert got["logits"].shape == (32, 2) and got["loss"].size == 1
    assert got["params"].size > 4_000_000  # the B0 trunk alone has 4,007,548 parameters
    assert sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out)) <= 64 << 20
