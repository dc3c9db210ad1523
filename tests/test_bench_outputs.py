"""bench.py's plain run, --full and --dump-outputs.

CPU: dump_outputs' file format and its size budget.  GPU: a small plain run prints the result
line without the figures that need runs of their own and writes the last step's arrays; the same
run with --full carries those figures.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (module import only: bench.main() is not called)

SMALL = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--ticks", "5", "--envs", "64"]


def test_dump_outputs_format_and_budget(tmp_path, monkeypatch):
    arrays = {"big": torch.arange(5000, dtype=torch.float64).reshape(50, 100),
              "small": torch.tensor([1, 2, 3], dtype=torch.uint8)}
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4096)
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), arrays)
    bench.dump_outputs(str(b), arrays)
    assert sorted(os.listdir(a)) == ["big.npy", "small.npy"]
    assert sum(os.path.getsize(a / f) for f in os.listdir(a)) <= 4096
    big, small = np.load(a / "big.npy"), np.load(a / "small.npy")
    assert big.dtype == np.float32 and small.dtype == np.float32
    assert small.tolist() == [1.0, 2.0, 3.0]
    # the sample: distinct elements of the array in their order, the same ones in every run
    assert big.ndim == 1 and 0 < big.size < 5000 and bool((np.diff(big) > 0).all())
    assert np.array_equal(big, np.load(b / "big.npy"))
    # an array within its share is written whole, in its shape; other ranks' files carry the rank
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 64 << 20)
    bench.dump_outputs(str(a), arrays, rank=1, world=2)
    assert np.array_equal(np.load(a / "big.rank1.npy"), arrays["big"].numpy().astype(np.float32))


def _bench(*extra):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, *extra], capture_output=True,
                       text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_its_last_step(tmp_path):
    line = _bench("--dump-outputs", str(tmp_path / "d"))
    assert line["steps"] == 2 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["ms_per_step"] > 0 and line["value"] > 0 and line["unit"] == "agent-steps/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f32"
    # value and ms_per_step describe the same timed steps: 64 envs x 8 agents x 5 ticks per step
    assert line["value"] == pytest.approx(64 * 8 * 5 / (line["ms_per_step"] * 1e-3), rel=1e-3)
    assert line["roofline"] is None and line["acting_only"] is None and line["cpu_baseline"] is None
    d = {f[:-4]: np.load(tmp_path / "d" / f) for f in os.listdir(tmp_path / "d")}
    assert {"state", "reward", "avg_dist", "hits", "params", "params_next", "adam_m", "adam_v", "target", "grad",
            "loss_gradnorm"} <= set(d)
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in d.values())
    assert d["state"].shape == (64, 8, 4) and d["reward"].shape == (64, 8) and d["params"].shape == (1673,)
    # three episodes of five ticks trained the weights away from the target's checkpoint values
    assert not np.array_equal(d["params"], d["target"]) and np.count_nonzero(d["adam_v"]) > 0
    assert d["loss_gradnorm"][0] == np.float32(line["loss"])


@pytest.mark.gpu
def test_full_run_carries_the_other_figures():
    line = _bench("--full", "--no-cpu-baseline")
    assert line["steps"] == 2 and line["ms_per_step"] > 0
    assert line["roofline"]["kernel_us"]["tick_kernel"] > 0
    assert line["acting_only"]["value"] > 0 and line["acting_only"]["training_graph"]["value"] > 0
    assert line["cpu_baseline"] is None
