"""N>1 data-parallel path on the GPU, rehearsed with 2 ranks sharing the box's one MI355X
(gloo staged through host memory; on the 8-GPU node the same code runs over RCCL).

1. DP gradients of the HIP model (each rank its own mesh, dist.mse_sum_loss + GradAllReduce)
   equal the single-process union-batch gradients of the same HIP model (fp32, summation-order
   tolerance).
2. `bench.py --gpus 2` under torchrun prints one JSON line with n_gpus == 2.
3. RCCL itself, once: a fresh torchrun child initialises the "nccl" backend (RCCL) before any GPU
   call at world size 1 (AEROGNN_DIST_FORCE=1), and GradAllReduce's armed path (bucket packing
   from the post-accumulate-grad hooks, async all-reduce on the RCCL communicator, wait, unpack)
   leaves the gradients bitwise unchanged; bench.py on the same setup prints its JSON line with
   the collective record.
"""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESHES = [(24, 16, 0), (20, 12, 1)]
KW = dict(processor_size=5, num_hidden_layers_node_processor=2, num_hidden_layers_edge_processor=2,
          num_hidden_layers_node_encoder=2, num_hidden_layers_edge_encoder=2, num_hidden_layers_decoder=2,
          hidden_dim_processor=128, hidden_dim_node_encoder=128, hidden_dim_edge_encoder=128,
          hidden_dim_decoder=128, aggregation="add", do_concat_trick=True, num_scales=3,
          layers_per_scale=1, stride=2)

WORKER = r'''
import os, sys, json
sys.path[:0] = [{root!r}, os.path.join({root!r}, "aero-gnn_amd")]
import numpy as np, torch
os.environ["AEROGNN_MEMLOG"] = "0"
from aerognn import dist as D
from aerognn.meshgen import ellipsoid
from models.bsms_mgn import BiStridedMeshGraphNet
rank, ws = D.init_from_env(backend="gloo")
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
torch.manual_seed(0)
model = BiStridedMeshGraphNet(6, 4, 4, **{kw!r}).to(dev).to(getattr(torch, {dt!r}))
nu, nv, seed = {meshes!r}[rank]
t = {{k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in ellipsoid(nu, nv, seed=seed).items()}}
for k in ("x", "edge_attr", "y"):
    t[k] = t[k].to(getattr(torch, {dt!r}))
n_glob = D.global_count(t["y"].numel(), dev)
pred = model(t["x"], t["edge_attr"], t["edge_index"], batch=None, pos=t["pos"])
D.mse_sum_loss(pred, t["y"], n_glob).backward()
D.GradAllReduce(model.parameters())()
if rank == 0:
    torch.save({{k: p.grad.cpu() for k, p in model.named_parameters()}}, {out!r})
torch.distributed.barrier()
torch.distributed.destroy_process_group()
'''


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _torchrun(script_args, timeout, nproc=2, backend="gloo", **extra_env):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", AEROGNN_DIST_BACKEND=backend, AEROGNN_MEMLOG="0",
               **extra_env)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
           "--master-addr=127.0.0.1", f"--master-port={_port()}"] + script_args
    return subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=timeout)


@pytest.mark.parametrize("dt", ["float32", "float64"])
def test_dp_grads_equal_union_batch_on_gpu(tmp_path, dt):
    """fp32: summation-order tolerance; float64 (train.py's "double" mode on the agn_f64_* path):
    the same gradients to ~1e-13, so the DP reduction itself is shown exact."""
    out = str(tmp_path / "g.pt")
    script = tmp_path / "worker.py"
    script.write_text(WORKER.format(root=ROOT, kw=KW, meshes=MESHES, out=out, dt=dt))
    r = _torchrun([str(script)], timeout=400)
    assert r.returncode == 0, r.stderr[-3000:]
    g_dp = torch.load(out, weights_only=True)

    from aerognn.meshgen import collate, ellipsoid
    from models.bsms_mgn import BiStridedMeshGraphNet
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = BiStridedMeshGraphNet(6, 4, 4, **KW).to(dev).to(getattr(torch, dt))
    u = collate([ellipsoid(*m[:2], seed=m[2]) for m in MESHES])
    u = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in u.items()}
    for k in ("x", "edge_attr", "y"):
        u[k] = u[k].to(getattr(torch, dt))
    pred = model(u["x"], u["edge_attr"], u["edge_index"], batch=u["batch"], pos=u["pos"])
    torch.nn.functional.mse_loss(pred, u["y"]).backward()
    errs = []
    for k, p in model.named_parameters():
        ref = p.grad.cpu().double()
        errs.append(float((g_dp[k].double() - ref).norm() / max(float(ref.norm()), 1e-30)))
    errs = np.array(errs)
    print(f"DP vs union batch ({dt}): param-grad rel-L2 median {np.median(errs):.3e}, worst {errs.max():.3e}")
    if dt == "float64":
        assert errs.max() < 1e-10, errs.max()
    else:
        # fp32 with different (valid) summation orders: measured median 6.9e-8, worst 1.3e-7
        # (profiles/r4_gpu_tests.log); the gate leaves room for a ReLU-kink flip
        assert np.median(errs) < 1e-6 and errs.max() < 1e-5, (np.median(errs), errs.max())


def test_bench_two_ranks_json():
    r = _torchrun(["bench.py", "--gpus", "2", "--config", "small", "--steps", "2", "--warmup", "1",
                   "--no-cpu-baseline"], timeout=500)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    assert d["n_gpus"] == 2 and d["value"] > 0 and d["scaling"] == "weak"
    assert d["config"]["parallelism"] == "dp2"


def test_bench_self_launch_two_ranks_json():
    """Plain `python bench.py --gpus 2` (no torchrun): bench starts its two ranks itself."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", AEROGNN_DIST_BACKEND="gloo", AEROGNN_MEMLOG="0")
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--config", "small", "--steps", "2", "--warmup", "1",
                        "--full", "--no-cpu-baseline", "--strong-config", "c4small"], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=500)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]  # rank 0 prints the only line
    d = json.loads(lines[0])
    print(d["value"], d["collective"])
    assert d["n_gpus"] == 2 and d["value"] > 0 and d["config"]["parallelism"] == "dp2"
    assert d["collective"]["world_size"] == 2 and d["collective"]["backend"] == "gloo"
    assert d["config"]["edge_updates_per_step_all_ranks"] > d["config"]["edge_updates_per_step_per_gpu"]
    # the strong-scaling leg reports per-rank times and the exposed all-reduce
    c4 = d["c4_strong"]
    print(c4)
    assert 0 < c4["rank_ms_min"] <= c4["rank_ms_max"] and c4["rank_ms_max"] == pytest.approx(c4["ms_per_step"], rel=1e-3)
    assert c4["allreduce_exposed_ms"] is not None and c4["allreduce_exposed_ms"] >= 0.0
    assert d["fault_word"] == 0


def test_bench_rejects_world_size_mismatch():
    r = _torchrun(["bench.py", "--gpus", "2", "--config", "small", "--steps", "1", "--warmup", "0",
                   "--no-cpu-baseline"], timeout=300, nproc=1)
    assert r.returncode != 0 and "WORLD_SIZE" in r.stderr, r.stderr[-2000:]


RCCL_WORKER = r'''
import os, sys, json
sys.path[:0] = [{root!r}, os.path.join({root!r}, "aero-gnn_amd")]
import numpy as np, torch
os.environ["AEROGNN_MEMLOG"] = "0"
from aerognn import dist as D
rank, ws = D.init_from_env()  # the RCCL process group, before any GPU call of this process
assert torch.distributed.get_backend() == "nccl" and ws == 1, (torch.distributed.get_backend(), ws)
from aerognn.meshgen import ellipsoid
from models.bsms_mgn import BiStridedMeshGraphNet
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
torch.manual_seed(0)
model = BiStridedMeshGraphNet(6, 4, 4, **{kw!r}).to(dev)
t = {{k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in ellipsoid(24, 16, seed=0).items()}}
n_glob = D.global_count(t["y"].numel(), dev)  # itself an RCCL all-reduce
def loss():
    return D.mse_sum_loss(model(t["x"], t["edge_attr"], t["edge_index"], batch=None, pos=t["pos"]), t["y"], n_glob)
loss().backward()
ref = {{k: p.grad.clone() for k, p in model.named_parameters()}}
model.zero_grad(set_to_none=True)
ar = D.GradAllReduce(model.parameters(), bucket_bytes=1 << 20)
ar.arm()
loss().backward()  # buckets pack and all-reduce from the hooks as their gradients land
in_hooks = ar.launched_in_hooks
ar()
torch.cuda.synchronize()
same = all(torch.equal(p.grad, ref[k]) for k, p in model.named_parameters())
json.dump({{"backend": torch.distributed.get_backend(), "buckets": len(ar.buckets), "in_hooks": in_hooks,
            "equal": same, "n_glob": n_glob}}, open({out!r}, "w"))
torch.distributed.destroy_process_group()
'''


def test_rccl_world_of_one_grad_allreduce(tmp_path):
    out = str(tmp_path / "r.json")
    script = tmp_path / "rccl_worker.py"
    script.write_text(RCCL_WORKER.format(root=ROOT, kw=KW, out=out))
    r = _torchrun([str(script)], timeout=300, nproc=1, backend="nccl", AEROGNN_DIST_FORCE="1")
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.load(open(out))
    print(d)
    assert d["backend"] == "nccl" and d["equal"], d
    assert d["buckets"] >= 2 and d["in_hooks"] >= 1, d  # the armed path ran, not only the tail call
    assert d["n_glob"] == 24 * 16 * 4  # y is [N, 4]


def test_bench_rccl_world_of_one_json():
    r = _torchrun(["bench.py", "--gpus", "1", "--config", "small", "--steps", "2", "--warmup", "1",
                   "--no-cpu-baseline"], timeout=400, nproc=1, backend="nccl", AEROGNN_DIST_FORCE="1")
    assert r.returncode == 0, r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    print(d["collective"], d["value"])
    assert d["n_gpus"] == 1 and d["value"] > 0
    assert d["collective"]["backend"] == "nccl" and d["collective"]["launched_in_hooks"] >= 1, d["collective"]
