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


def b_mlp_dropout(nrow, k, H, out, p):
    """models/mlp.py in training with dropout p: the chain Linear by Linear (LayeredSpec). The forward
    seeds torch's generator itself, so the Philox offsets of its masks are fixed."""
    from models.mlp import MLP
    m = _module(lambda: MLP(k, H, out, 2, "relu", p, True), F32).train()
    x = _rand((nrow, k), F32, 2, False)

    def fwd():
        torch.manual_seed(11)
        return {"y": m(x)}
    return fwd, _named(m)


def b_mlp_one_linear(nrow, k, H, out):
    """num_hidden_layers = 0 (the one-Linear quirk of mlp.py:31-32): `hidden` is the outputs rounded
    up to 32; with and without the LayerNorm."""
    from models.mlp import MLP
    ms = {tag: _module(lambda: MLP(k, H, out, 0, "relu", 0.0, ln), F32) for tag, ln in (("ln", True), ("plain", False))}
    x = _rand((nrow, k), F32, 2)
    leaves = {"x": x}
    for tag, m in ms.items():
        leaves.update({f"{tag}.{n}": p for n, p in m.named_parameters()})
    return (lambda: {f"y_{tag}": m(x) for tag, m in ms.items()}), leaves


def b_trial1_model(shape, H, layers):
    """One train step of a small MeshGraphNet_v2 on a batch of two graphs: every build_mlp Sequential and
    the bare linout as chains, the global pool and its broadcast, MGNv2Fn per layer."""
    from models.trial1 import MeshGraphNet_v2
    N, E = shape
    ei, _ = _graph(N, E)
    m = _module(lambda: MeshGraphNet_v2(6, 4, H, 3, layers), F32)
    x, ea = _rand((N, 6), F32, 2), _rand((E, 4), F32, 3)
    batch = (torch.arange(N) >= N // 2).long().to(DEV)
    return (lambda: {"y": m(x, ea, ei, batch)}), {"x": x, "edge_attr": ea, **_named(m)}


FOURIER = (2, -3, 7, True)  # d, freq_start, freq_len, with_input


def b_fourier(nrow, k, op):
    """[x | Fourier features] through the autograd Function or through torch.ops.aerognn.fourier_embed."""
    import aerognn.ops  # noqa: F401  (registers the operators)
    from aerognn.functions import FourierEmbedFn
    x = _rand((nrow, k), F32, 2)
    f = torch.ops.aerognn.fourier_embed if op else FourierEmbedFn.apply
    return (lambda: {"y": f(x, *FOURIER)}), {"x": x}


def b_act_dropout(nrow, k, p, op):
    """dropout_p(act(y)) for 'gelu' and 'none' through ActDropoutFn or through the registered operator,
    seeded alike inside the forward."""
    from aerognn import _lib as L
    from aerognn import ops
    from aerognn.functions import ActDropoutFn
    ys = {a: _rand((nrow, k), F32, 2 + i) for i, a in enumerate(("gelu", "none"))}

    def one(a):
        if op:
            return ops.act_dropout(ys[a], a, p)
        return ActDropoutFn.apply(ys[a], L.ACT_NONE if a == "none" else L.ACT[a], p)

    def fwd():
        torch.manual_seed(11)
        return {a: one(a) for a in ys}
    return fwd, {f"y_{a}": y for a, y in ys.items()}


def b_f64_mlp_rows(nrow, k, H, out, rows):
    """float64 MLP.forward_rows with an input gradient: the agn_f64_* kernels are not in the trace, the
    grouping and the segment sum of the scattered input gradient are."""
    from models.mlp import MLP
    m = _module(lambda: MLP(k, H, out, 2), torch.float64)
    x = _rand((nrow, k), torch.float64, 2)
    idx = torch.randint(0, nrow, (rows,), generator=_gen(5)).to(DEV)
    return (lambda: {"y": m.forward_rows(x, idx)}), {"x": x, **_named(m)}


def b_f64_gmp(shape, H):
    """A float64 MeshGraphNetLayer with the sum trick (aerognn/f64.py gmp_layer)."""
    from models.mgnLayer import MeshGraphNetLayer
    N, E = shape
    _, lv = _graph(N, E)
    m = _module(lambda: MeshGraphNetLayer(H, H, H, 2, 2, "relu", True, "add", True), torch.float64)
    x, e = _xe(N, E, H, torch.float64)
    return (lambda: dict(zip(("x'", "e'"), m.forward_level(x, e, lv)))), {"x": x, "e": e, **_named(m)}


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
# the routes that bind a reference module to a chain outside the layer Functions
_case("mlp_dropout_h32", b_mlp_dropout, nrow=300, k=6, H=32, out=32, p=0.1)
_case("mlp_one_linear", b_mlp_one_linear, nrow=300, k=6, H=32, out=20)
_case("trial1_model_h32", b_trial1_model, shape=SMALL, H=32, layers=2)
for _op in (False, True):
    _case("fourier_op" if _op else "fourier_fn", b_fourier, nrow=300, k=5, op=_op)
    _case("act_dropout_op" if _op else "act_dropout_fn", b_act_dropout, nrow=300, k=33, p=0.1, op=_op)
_case("f64_mlp_rows_dx", b_f64_mlp_rows, nrow=300, k=6, H=32, out=32, rows=500)
_case("f64_gmp_sum", b_f64_gmp, shape=SMALL, H=32)
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
