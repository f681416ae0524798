"""bench.py's command line: a plain run carries the headline only, --full the rest, and
--dump-outputs writes what the last timed step computed (bounded by bench.DUMP_BUDGET)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_dump_outputs_budget_and_fixed_sample(tmp_path, monkeypatch):
    """Within the budget every array is written whole; over it, the largest array alone is cut to
    a sample that is the same from call to call, and the files together stay within the budget."""
    g = torch.Generator().manual_seed(1)
    big = torch.randn(5000, 4, generator=g).to(torch.bfloat16)
    small = torch.randn(7, 3, generator=g)
    bench.dump_outputs(str(tmp_path / "whole"), {"pred": big, "param.w": small})
    a = _load(str(tmp_path / "whole"))
    assert a["pred"].dtype == np.float32 and a["pred"].shape == (5000, 4)
    assert np.array_equal(a["pred"], big.float().numpy()) and np.array_equal(a["param.w"], small.numpy())

    monkeypatch.setattr(bench, "DUMP_BUDGET", 40000)
    for name in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / name), {"pred": big, "param.w": small})
    s1, s2 = _load(str(tmp_path / "s1")), _load(str(tmp_path / "s2"))
    assert np.array_equal(s1["param.w"], small.numpy())
    assert s1["pred"].ndim == 1 and 0 < s1["pred"].size < big.numel()
    assert np.array_equal(s1["pred"], s2["pred"])
    assert np.isin(s1["pred"], big.float().numpy()).all()
    assert sum(os.path.getsize(tmp_path / "s1" / f) for f in os.listdir(tmp_path / "s1")) <= 40000


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_last_step(tmp_path):
    out = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--config", "small", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", out], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["warmup"] == 1 and d["full"] is False
    assert d["ms_per_step"] > 0 and d["value"] > 0 and d["dtype"] == "bf16" and d["higher_is_better"] is True
    assert d["value"] == pytest.approx(d["config"]["edge_updates_per_step_all_ranks"] / d["ms_per_step"] / 1e3, rel=1e-3)
    for k in ("kernels", "roofline", "c4_strong", "cpu_baseline"):
        assert k not in d, k
    a = _load(out)
    assert a["pred"].shape == (200 * 125, 4) and a["loss"].shape == (1,)
    params = [k for k in a if k.startswith("param.")]
    assert len(params) > 100 and all(a[k].dtype == np.float32 and np.isfinite(a[k]).all() for k in a)
    assert np.isfinite(a["loss"][0]) and a["loss"][0] > 0 and np.abs(a["pred"]).max() > 0
    assert sum(v.nbytes for v in a.values()) <= bench.DUMP_BUDGET
