"""The measurements of DESIGN.md 7g on one MI355X: agn_act_dropout_fwd / _bwd at 6,000,000 x 128 bf16
(time and the bytes they move per second), and the edge encoder's train step MLP(4, 128, 128, 2) bf16 on
the same rows at p = 0.1 against p = 0. HIP events around single launches (steps), warmed up, median
(min, max). Prints one JSON object.

Run:  python tools/dropout_micro.py
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "aero-gnn_amd")]
os.environ.setdefault("AEROGNN_MEMLOG", "0")
import torch
from aerognn import core, _lib as L
from models.mlp import MLP

dev = torch.device("cuda:0")
out = {}
rows, H = 6_000_000, 128
y = torch.randn(rows, H, device=dev, dtype=torch.bfloat16)
o = torch.empty_like(y)
mask = core.keep_mask_empty(y.numel(), dev)
g = torch.randn_like(y)


def timed(fn, warm=5, n=30):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ts.append(s.elapsed_time(e))
    return statistics.median(ts), min(ts), max(ts)


for act, name in ((L.ACT["relu"], "relu"), (L.ACT["gelu"], "gelu"), (L.ACT_NONE, "none")):
    med, lo, hi = timed(lambda: core.act_dropout_fwd(y, act, 0.1, 1234, 0, o, mask))
    nbytes = y.numel() * (2 + 2 + 1 / 8)
    out[f"fwd_{name}_ms"] = (med, lo, hi)
    out[f"fwd_{name}_TBps"] = nbytes / med / 1e9
    med, lo, hi = timed(lambda: core.act_dropout_bwd(y, act, 0.1, g, mask, o))
    out[f"bwd_{name}_ms"] = (med, lo, hi)
    out[f"bwd_{name}_TBps"] = y.numel() * ((4 if act != L.ACT_NONE else 2) + 2 + 1 / 8) / med / 1e9
del o, g, y, mask
torch.cuda.empty_cache()

x = torch.randn(rows, 4, device=dev, dtype=torch.bfloat16)
gy = torch.randn(rows, H, device=dev, dtype=torch.bfloat16)
for p in (0.0, 0.1):
    torch.manual_seed(0)
    m = MLP(4, H, H, 2, dropout=p).to(torch.bfloat16).to(dev).train()

    def step():
        m.zero_grad(set_to_none=True)
        m(x).backward(gy)
    med, lo, hi = timed(step, warm=3, n=10)
    out[f"edge_encoder_step_p{p}_ms"] = (med, lo, hi)
out["ratio_p0.1_over_p0"] = out["edge_encoder_step_p0.1_ms"][0] / out["edge_encoder_step_p0.0_ms"][0]
print(json.dumps(out, indent=1))
