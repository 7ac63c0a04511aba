"""bench.py's plain run, --full and --dump-outputs: the writer of the dumped arrays (size budget,
fixed sample) on the CPU, and one plain run end to end on the GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _dir_bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_dump_outputs_budget_and_fixed_sample(tmp_path, monkeypatch):
    """Arrays within their share of the budget are written whole, in fp32; a larger one is cut to the
    same elements in every call, and the files together stay within the budget."""
    b = _bench()
    monkeypatch.setattr(b, "DUMP_BUDGET_BYTES", 4 * 3000)  # 1000 elements per array
    big = torch.arange(5000, dtype=torch.float64).reshape(50, 100)
    arrays = {"loss": torch.tensor(1.5), "small": torch.arange(12.0).reshape(3, 4), "big": big}
    for d in ("a", "b"):
        b.dump_outputs(str(tmp_path / d), arrays)
    a = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in arrays}
    assert all(v.dtype == np.float32 for v in a.values())
    assert a["loss"].shape == () and a["loss"] == 1.5
    np.testing.assert_array_equal(a["small"], arrays["small"].numpy())
    assert a["big"].shape == (1000,)
    assert np.all(np.diff(a["big"]) > 0) and set(a["big"]) <= set(range(5000))  # distinct elements, in order
    np.testing.assert_array_equal(a["big"], np.load(tmp_path / "b" / "big.npy"))
    assert sum(v.nbytes for v in a.values()) <= 4 * 3000


def test_default_budget_is_under_64_mb():
    assert _bench().DUMP_BUDGET_BYTES + 4096 <= 64 * 10 ** 6  # .npy headers included


def test_flat_tensors_logical_order():
    """Nested states flatten in list order and in each tensor's logical (not memory) order; None skipped."""
    b = _bench()
    t = torch.arange(6.0).reshape(2, 3).t()  # non-contiguous view
    flat = b._flat_tensors([t, None, [torch.tensor([7.0])]])
    assert flat.tolist() == [0.0, 3.0, 1.0, 4.0, 2.0, 5.0, 7.0]
    assert b._flat_tensors([None]) is None


@pytest.mark.gpu
def test_plain_run_line_and_dump(tmp_path):
    """A plain run (no --full) at a small batch: the line holds the headline fields and ms_per_step,
    none of the --full measurements, and --dump-outputs writes the last timed step's loss, flows,
    states and parameters, finite, in fp32."""
    B, T, R, steps = 2, 10, 128, 3
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
           "--batch", str(B), "--pool", "2", "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    res = json.loads(lines[0])
    assert res["steps"] == steps and res["unit"] == "events/s" and res["higher_is_better"] and res["dtype"] == "fp32"
    assert res["ms_per_step"] > 0
    assert abs(res["value"] - B * T * 1000 / (res["ms_per_step"] * 1e-3)) <= 1e-3 * res["value"]
    assert res["roofline"] is None and res["kernels"] is None and res["cpu_baseline"] is None
    out = {f[:-4]: np.load(tmp_path / "out" / f) for f in os.listdir(tmp_path / "out")}
    assert set(out) == {"loss", "flow_0", "states", "params"}
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in out.values())
    assert out["loss"].shape == () and out["flow_0"].shape == (T, B, 2, R, R)
    assert np.abs(out["flow_0"]).max() > 0 and np.abs(out["states"]).max() > 0
    assert _dir_bytes(tmp_path / "out") <= 64 * 10 ** 6
