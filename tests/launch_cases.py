"""The case table of the launch-trace test (test_gpu_launch_trace.py) and of the tool that records
its golden file (tools/record_launch_traces.py): one forward and one backward of every
autograd.Function mode in aerognn/functions.py, at shapes on both sides of the thresholds that pick a
kernel path (rows >= 64 * 1024 for the fused, 32-row and aggregation paths).

run_case(case, setenv) returns (trace, tensors): the [tag, cost] pair of every launch that core.PROF
recorded during the step, and every output and gradient by name. Inputs, weights and graphs come from
fixed seeds; the costs are functions of the shapes alone, so a trace compares exactly.
"""
import os

import torch

os.environ.setdefault("AEROGNN_MEMLOG", "0")
DEV = "cuda"
SMALL = (300, 1500)
LARGE = (65536, 131072)
F32, BF16 = torch.float32, torch.bfloat16


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _graph(N, E, seed=1):
    """A random edge list whose last node receives nothing (in-degree 0); the level in CSC order."""
    from aerognn.graph import Level
    g = _gen(seed)
    ei = torch.stack([torch.randint(0, N, (E,), generator=g), torch.randint(0, N - 1, (E,), generator=g)]).to(DEV)
    return ei, Level.from_edge_index(ei, N)


def _rand(shape, dt, seed, grad=True):
    return torch.randn(*shape, generator=_gen(seed)).to(dt).to(DEV).requires_grad_(grad)


def _module(make, pdt):
    torch.manual_seed(0)
    return make().to(DEV).to(pdt)


def _xe(N, E, H, dt, train=True):
    return _rand((N, H), dt, 2, train), _rand((E, H), dt, 3, train)


# --------------------------------------------------------------------------- builders
# Each returns (forward, leaves): forward() -> {name: output}, leaves = {name: tensor whose .grad counts}.
def _named(m):
    return {n: p for n, p in m.named_parameters()}


def b_gmp(shape, dt, H, aggregation="add", trick=True, train=True, pdt=F32):
    from models.mgnLayer import MeshGraphNetLayer
    N, E = shape
    _, lv = _graph(N, E)
    m = _module(lambda: MeshGraphNetLayer(H, H, H, 2, 2, "relu", True, aggregation, trick), pdt)
    x, e = _xe(N, E, H, dt, train)
    m.spec().pack.update(dt, x.device)
    return (lambda: dict(zip(("x'", "e'"), m.forward_level(x, e, lv)))), {"x": x, "e": e, **_named(m)}


def b_gmp_order(shape, dt, H):
    from models.bistride_ops import GMP
    N, E = shape
    _, lv = _graph(N, E)
    m = _module(lambda: GMP(H, H, H), F32)
    x, e = _xe(N, E, H, dt)
    m.spec().pack.update(dt, x.device)
    return (lambda: dict(zip(("x'", "e'"), m.forward_level(x, e, lv)))), {"x": x, "e": e, **_named(m)}


def b_edge_block(shape, dt, H, trick):
    from aerognn.functions import EdgeBlockFn
    from models.mgnLayer import EdgeBlock, EdgeBlockSum
    N, E = shape
    _, lv = _graph(N, E)
    m = _module(lambda: (EdgeBlockSum if trick else EdgeBlock)(H, H, H, 2, "relu", True), F32)
    x, e = _xe(N, E, H, dt)
    s = m.spec()
    s.pack.update(dt, x.device)
    return (lambda: {"e'": EdgeBlockFn.apply(x, e, lv, s, True, *s.edge_params())}), {"x": x, "e": e, **_named(m)}


def b_node_block(shape, dt, H, aggregation):
    from aerognn.functions import NodeBlockFn
    from models.mgnLayer import NodeBlock
    N, E = shape
    _, lv = _graph(N, E)
    m = _module(lambda: NodeBlock(H, H, H, 2, "relu", True, aggregation), F32)
    x, e = _xe(N, E, H, dt)
    s = m.spec()
    s.pack.update(dt, x.device)
    return (lambda: {"x'": NodeBlockFn.apply(x, e, lv, s, True, *s.node_params())}), {"x": x, "e": e, **_named(m)}


def b_v2(shape, dt, H, train=True, pdt=F32):
    from models.trial1 import MeshGraphNetLayer_v2
    N, E = shape
    _, lv = _graph(N, E)
    m = _module(lambda: MeshGraphNetLayer_v2(H), pdt)
    x, e = _xe(N, E, H, dt, train)
    m.spec().pack.update(dt, x.device)
    return (lambda: dict(zip(("x'", "e'"), m.forward_level(x, e, lv)))), {"x": x, "e": e, **_named(m)}


def b_mlp(nrow, k, dt, H, out, ln=True, rows=None, need_dx=False, pdt=F32):
    """rows: the chain runs on x[rows] for `rows` random row ids of the nrow-row input."""
    from models.mlp import MLP
    m = _module(lambda: MLP(k, H, out, 2, "relu", 0.0, ln), pdt)
    x = _rand((nrow, k), dt, 2, need_dx)
    idx = None if rows is None else torch.randint(0, nrow, (rows,), generator=_gen(5)).to(DEV)
    m.spec().pack.update(dt, x.device)
    fwd = (lambda: {"y": m(x)}) if idx is None else (lambda: {"y": m.forward_rows(x, idx)})
    return fwd, {**({"x": x} if need_dx else {}), **_named(m)}


def b_wec(shape, given):
    from models.bistride_ops import WeightedEdgeConv
    N, E = shape
    ei, lv = _graph(N, E)
    m = _module(lambda: WeightedEdgeConv(32, 64), F32)
    x = _rand((N, 32), F32, 2)
    pos = _rand((N, 3), F32, 3, False)
    m.spec().pack.update(F32, x.device)
    if not given:
        return (lambda: dict(zip(("out", "w"), m(x, ei, pos, level=lv)))), {"x": x, **_named(m)}
    w = torch.rand(E, 1, generator=_gen(4)).to(DEV).requires_grad_(True)
    return (lambda: {"out": m(x, ei, pos, edge_weights=w, compute_weights=False, level=lv)[0]}), \
        {"x": x, "w": w, "transform.weight": m.transform.weight, "transform.bias": m.transform.bias}


def b_pool(shape, H, boxed):
    """The U-Net's pooling step and its way back up (bsms_mgn.py:196-206) on one level."""
    from aerognn.functions import GradBox, PoolEdgeFn, PoolNodeFn, SkipFn, UnpoolFn
    from aerognn.graph import downsample_maps
    N, E = shape
    _, lv = _graph(N, E)
    P = downsample_maps(lv, None, None, 2, 1)
    x, e = _xe(N, E, H, F32)
    skip = x if boxed else _rand((N, H), F32, 4)

    def fwd():
        bn, be = (GradBox(), GradBox()) if boxed else (None, None)
        cn = PoolNodeFn.apply(x, P, bn)
        ce = PoolEdgeFn.apply(e, P, be)
        out = {"coarse_e": ce, "fine_x": UnpoolFn.apply(cn, skip, P, bn)}
        if boxed:
            out["fine_e"] = SkipFn.apply(e, be)
        return out
    return fwd, {"x": x, "e": e, "skip": skip}


# --------------------------------------------------------------------------- the table
# name -> (builder, kwargs, {AEROGNN_* switch: value})
CASES = {}


def _case(name, builder, env=None, **kw):
    assert name not in CASES
    CASES[name] = (builder, kw, env or {})


for _trick in (True, False):
    _eb = "sum" if _trick else "cat"
    for _agg in ("add", "mean"):
        for _train in (True, False):
            _case(f"gmp_f32_h32_{_eb}_{_agg}_{'train' if _train else 'infer'}", b_gmp, shape=SMALL, dt=F32, H=32,
                  aggregation=_agg, trick=_trick, train=_train)
    _case(f"gmp_bf16_h128_{_eb}", b_gmp, shape=SMALL, dt=BF16, H=128, trick=_trick, pdt=BF16)
    _case(f"edge_block_{_eb}", b_edge_block, shape=SMALL, dt=F32, H=32, trick=_trick)
_case("gmp_order", b_gmp_order, shape=SMALL, dt=F32, H=32)
for _agg in ("add", "mean"):
    _case(f"node_block_{_agg}", b_node_block, shape=SMALL, dt=F32, H=32, aggregation=_agg)
_case("v2_f32_h32", b_v2, shape=SMALL, dt=F32, H=32)
_case("mlp_encoder_k6", b_mlp, nrow=300, k=6, dt=F32, H=128, out=128)
_case("mlp_encoder_k6_rows_dx", b_mlp, nrow=300, k=6, dt=F32, H=128, out=128, rows=500, need_dx=True)
_case("mlp_decoder_no_ln", b_mlp, nrow=300, k=128, dt=F32, H=128, out=3, ln=False, need_dx=True)
_case("mlp_wide_h32", b_mlp, nrow=300, k=131, dt=F32, H=32, out=32, need_dx=True)
_case("wec", b_wec, shape=SMALL, given=False)
_case("wec_given", b_wec, shape=SMALL, given=True)
_case("pool_boxed", b_pool, shape=SMALL, H=32, boxed=True)
_case("pool_plain", b_pool, shape=SMALL, H=32, boxed=False)

_case("L_gmp_train", b_gmp, shape=LARGE, dt=BF16, H=128)
for _sw in ("EB_SAVED", "EDGE_AGG", "WG_DPD", "FUSED_EDGE_BWD", "PROJ_KERNEL"):
    _case(f"L_gmp_train_{_sw}_0", b_gmp, env={f"AEROGNN_{_sw}": "0"}, shape=LARGE, dt=BF16, H=128)
_case("L_gmp_infer", b_gmp, shape=LARGE, dt=BF16, H=128, train=False)
_case("L_v2_train", b_v2, shape=LARGE, dt=BF16, H=128)
_case("L_v2_infer", b_v2, shape=LARGE, dt=BF16, H=128, train=False)
_case("L_v2_train_V2_EDGE32_0", b_v2, env={"AEROGNN_V2_EDGE32": "0"}, shape=LARGE, dt=BF16, H=128)
_case("L_mlp_encoder_rows", b_mlp, nrow=70000, k=6, dt=BF16, H=128, out=128, rows=65536)
_case("L_mlp_encoder_rows_FUSED_ENC_BWD_0", b_mlp, env={"AEROGNN_FUSED_ENC_BWD": "0"}, nrow=70000, k=6, dt=BF16,
      H=128, out=128, rows=65536)
# the same fused paths with 16-bit parameters: every gradient is then rounded from its fp32 value
_case("L_gmp_train_bf16_params", b_gmp, shape=LARGE, dt=BF16, H=128, pdt=BF16)
_case("L_v2_train_bf16_params", b_v2, shape=LARGE, dt=BF16, H=128, pdt=BF16)
_case("L_mlp_encoder_rows_bf16_params", b_mlp, nrow=70000, k=6, dt=BF16, H=128, out=128, rows=65536, pdt=BF16)


def step(fwd, leaves, train=True):
    """One forward (and, in training, one backward from fixed-seed output gradients): every output by
    name and every leaf's gradient as "d <name>"."""
    if train:
        outs = fwd()
        gs = [torch.randn(o.shape, generator=_gen(7 + i)).to(o.dtype).to(DEV) for i, o in enumerate(outs.values())]
        torch.autograd.backward(list(outs.values()), gs)
    else:
        with torch.no_grad():
            outs = fwd()
    torch.cuda.synchronize()
    tensors = {k: v.detach() for k, v in outs.items()}
    if train:
        for k, t in leaves.items():
            assert t.grad is not None, k
            tensors["d " + k] = t.grad
    return tensors


def run_case(name, setenv):
    """One forward and one backward of a case with core.PROF on. setenv(key, value) sets the case's
    switches (monkeypatch.setenv in the test); the caller restores the environment."""
    from aerognn import core
    builder, kw, env = CASES[name]
    for k, v in env.items():
        setenv(k, v)
    fwd, leaves = builder(**kw)
    torch.cuda.synchronize()
    core.PROF = []
    try:
        tensors = step(fwd, leaves, kw.get("train", True))
        trace = [[tag, None if cost is None else list(cost)] for tag, cost, *_ in core.PROF]
    finally:
        core.PROF = None
    return trace, tensors
