"""Every elementwise torch.nn.functional activation in the MLP chains (mlp.py:37 getattr(F, activation_fn))
on the MI355X: the fourteen names added to relu / gelu / silu / tanh (tests/actref.py NEW).

1. elementwise, through torch.ops.aerognn.act_dropout(y, name, 0.0) and its autograd on a fixed grid, in
   float64 (1e-10 relative, exact at the kinks), fp32 (ulps against float64, gated on torch's own fp32),
   bf16 / fp16 (within 1 ulp_T of the rounded float64 value); 256 B of sentinel behind every output.
2. models.mlp.MLP against the reference's goldens (tools/make_goldens_act.py): float64 1e-10; fp32 1e-5
   forward and input gradient, 5e-5 parameter gradients; bf16 / fp16 2e-2 against the float64 formula on
   the rounded operands.
3. the general kernels at rows 1 / 33 / 130 and three chain shapes, H = 32, fp32 and bf16: the
   instantiation reached, pre[l] saved, no ReLU-only fast kernel launched, the same bars.
4. with training-mode dropout (elu, hardswish), the mask reproduced from the generator state.
5. one MeshGraphNet training step with leaky_relu on the irregular `hub` graph against float64.
The reference is torch on the CPU in float64 throughout.
"""
import os

import pytest
import torch

import actref as A
import dropoutref as D
from chainref import ref_chain
from golden_util import load, max_rel, rel_l2

pytestmark = pytest.mark.gpu
os.environ.setdefault("AEROGNN_MEMLOG", "0")

DEV = "cuda"
FWD, GIN, GPAR, B16, F64 = 1e-5, 1e-5, 5e-5, 2e-2, 1e-10
M_VEC, M_GEN, M_NIN = 0, 1, 2
SENT = 0xA5
DTYPES = [torch.float64, torch.float32, torch.bfloat16, torch.float16]
IDS = ["fp64", "fp32", "bf16", "fp16"]
FAST = ["agn_debug_edge_agg_launches", "agn_debug_node32_launches", "agn_debug_enc32_launches",
        "agn_debug_dec32_launches", "agn_debug_node32_bwd_launches", "agn_debug_dec32_bwd_launches"]
pm = pytest.mark.parametrize


def _ops():
    import aerognn.ops  # noqa: F401  (registers torch.ops.aerognn.*)
    return torch.ops.aerognn


def _fast_counters():
    """The launch counters of the ReLU-only fast kernels. At the sizes of this file they cannot move
    whatever the activation (each of those kernels also declines below 64 * 1024 rows), so asserting
    them unchanged does NOT protect the kernels' `act_fn != AGN_ACT_RELU` guards: those stand by reading
    the code (csrc/mlp.hip res_fwd_ok / res_bwd_ok, node32_fwd / node32_bwd / enc32_fwd *_try,
    aerognn/core.py edge32_ok) and by tests/test_gpu_mask_matched.py's GELU chains at 70,001 rows."""
    from aerognn import _lib as L
    return [int(getattr(L.lib(), n)()) for n in FAST]


def _guarded(n, dtype):
    """A flat tensor of n elements of dtype with 256 B of sentinel behind it: (tensor, the sentinel bytes)."""
    nb = n * torch.empty(0, dtype=dtype).element_size()
    buf = torch.full((nb + 256,), SENT, dtype=torch.uint8, device=DEV)
    return buf[:nb].view(dtype), buf[nb:]


def _bits(t):
    return t.detach().cpu().contiguous().view(A.INT[t.dtype])


# ------------------------------------------------------------------------------ 1. elementwise
def _elementwise(name, dtype):
    """Ours on the grid through the operator and its autograd: (x, dy, y, gx) on the CPU. The same kernels
    called on guarded buffers must give the same bits and leave the sentinels alone."""
    from aerognn import _lib as L, core
    x, span = A.grid(dtype)
    n = x.numel()
    dy = A.upstream(n, dtype)
    xd = x.to(DEV).requires_grad_(True)
    out, mask = _ops().act_dropout(xd, name, 0.0)
    out.backward(dy.to(DEV))
    assert out.dtype == dtype and xd.grad.dtype == dtype
    (o, so), (m, sm), (g, sg) = _guarded(n, dtype), _guarded((n + 7) // 8, torch.uint8), _guarded(n, dtype)
    core.act_dropout_fwd(xd.detach(), L.ACT[name], 0.0, 0, 0, o, m)
    core.act_dropout_bwd(xd.detach(), L.ACT[name], 0.0, dy.to(DEV), m, g)
    torch.cuda.synchronize()
    assert all(bool((s == SENT).all()) for s in (so, sm, sg)), "sentinel overwritten"
    assert torch.equal(_bits(o), _bits(out)) and torch.equal(_bits(g), _bits(xd.grad)) and torch.equal(m, mask)
    return x, dy, span, out.detach().cpu(), xd.grad.cpu()


def _finite_where_torch_is(name, what, got, ref, dtype):
    ok = torch.isfinite(ref) & torch.isfinite(ref.to(dtype))
    assert bool(torch.isfinite(got[ok]).all()), f"{name} {what}: inf or NaN where torch is finite"


@pm("name", A.NEW)
def test_elementwise_float64(name):
    """Worst relative error |got - ref| / |ref| per function against torch's CPU float64 at 1e-10. tanhshrink is
    the one departure: torch's own x - tanh(x) and dy - dy (1 - tanh^2) cancel (0 at 1e-30), so its rounding
    noise, 4 eps |x| and 4 eps |dy| (actref.ref_noise), is taken off the difference first; and the kernels'
    result is also held to 1e-10, nothing taken off, against a reference that does not cancel
    (actref.tanhshrink_exact), which is what checks the series below 1/32."""
    x, dy, (k0, k1), y, gx = _elementwise(name, torch.float64)
    ry, rg = A.f64_ref(name, x, dy)
    refs = [("forward", y, ry, False, "torch"), ("backward", gx, rg, True, "torch")]
    if name == "tanhshrink":
        ey, eg = A.tanhshrink_exact(x, dy)
        refs += [("forward", y, ey, None, "exact"), ("backward", gx, eg, None, "exact")]
    for what, got, ref, back, which in refs:
        _finite_where_torch_is(name, what, got, ref, torch.float64)
        e = A.rel_err(got, ref, None if back is None else A.ref_noise(name, back, x, dy))
        i = int(e.argmax())
        print(f"{name} float64 {what} against {which}: worst relative error {float(e[i]):.3e} at x = {float(x[i])!r} "
              f"(gate {F64:.0e})")
        assert float(e.max()) <= F64, (name, what, which, float(e[i]), float(x[i]))
    # torch's side of every kink: on the point and on both neighbours, bit for bit (a zero of either sign)
    at = [k0 + 3 * j + q for j, k in enumerate(A.ALL_KINKS) if k in A.KINKS.get(name, ()) for q in range(3)]
    assert len(at) == 3 * len(A.KINKS.get(name, ()))
    if at:
        assert torch.equal(y[at], ry[at]), (name, x[at], y[at], ry[at])
        assert torch.equal(gx[at], rg[at]), (name, x[at], gx[at] / dy[at], rg[at] / dy[at])


# tanhshrink is the one function the kernels evaluate by another formula than torch (the series below 1/8), so
# 3 x torch's worst (1.2e7 ulps from its cancellation) is no measure of it. Its gate is capped by what the
# kernels' own formula allows with a tanhf within OpenCL's 5 ulps: forward, worst at the switch point 1/8,
# (5 + 1/2) ulp(tanh(1/8)) = 5.5 * 2^-27 over ulp(x^3 / 3 = 6.5e-4) = 2^-34, 704 ulps; backward dy t^2,
# 2 * 5 (the square) + 1/2 + 1/2 + 1/2 (three roundings) < 12 ulps.
FP32_CAP = {("tanhshrink", "forward"): 704.0, ("tanhshrink", "backward"): 12.0}


@pm("name", A.NEW)
def test_elementwise_fp32_in_ulps(name):
    """Worst error in fp32 ulps against float64, ours and torch's own fp32 CPU result; ours within 3 x
    torch's (test_gpu_train_tail.gate_fp32's margin: a different but equally good libm), never gated below
    1 ulp, which is a rounding, and for tanhshrink never above FP32_CAP. (tanhshrink's float64 value is
    actref.tanhshrink_exact: torch's float64 result is itself 2 fp32 ulps off at 1e-4.)"""
    import torch.nn.functional as F
    x, dy, _, y, gx = _elementwise(name, torch.float32)
    ry, rg = A.tanhshrink_exact(x.double(), dy.double()) if name == "tanhshrink" else A.f64_ref(name, x, dy)
    xt = x.clone().requires_grad_(True)
    ty = getattr(F, name)(xt)
    ty.backward(dy)
    for what, got, own, ref in (("forward", y, ty.detach(), ry), ("backward", gx, xt.grad, rg)):
        _finite_where_torch_is(name, what, got, ref, torch.float32)
        u = A.ulp(ref, torch.float32)
        eo, et = (got.double() - ref).abs() / u, (own.double() - ref).abs() / u
        i = int(eo.argmax())
        gate = min(max(3.0 * float(et.max()), 1.0), FP32_CAP.get((name, what), float("inf")))
        print(f"{name} fp32 {what}: worst ulps ours {float(eo[i]):.2f} (at x = {float(x[i])!r}), torch "
              f"{float(et.max()):.2f} (at x = {float(x[int(et.argmax())])!r}); gate {gate:.2f}")
        assert float(eo.max()) <= gate, (name, what, float(eo[i]), float(x[i]), float(et.max()))


@pm("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pm("name", A.NEW)
def test_elementwise_16bit_within_one_ulp(name, dtype):
    """Every element within 1 ulp_T of round_T(the float64 value): the fp32 evaluation is a few fp32 ulps
    off, which can flip one rounding, never two. sigmoid's derivative is taken from the stored output."""
    x, dy, _, y, gx = _elementwise(name, dtype)
    ry, rg = A.f64_ref(name, x, dy, y_stored=y if name == "sigmoid" else None)
    for what, got, ref in (("forward", y, ry), ("backward", gx, rg)):
        _finite_where_torch_is(name, what, got, ref, dtype)
        want = ref.to(dtype).double()
        e = (got.double() - want).abs() / A.ulp(want, dtype)
        i = int(e.argmax())
        print(f"{name} {dtype} {what}: worst {float(e[i]):.2f} ulp_T at x = {float(x[i])!r}")
        assert float(e.max()) <= 1.0, (name, what, float(e[i]), float(x[i]), float(got[i]), float(want[i]))


# ------------------------------------------------------------------------------ 2. modules against the goldens
def _gate(what, got, ref, tol, elem=True):
    r, mx = rel_l2(got.detach().cpu(), ref), max_rel(got.detach().cpu(), ref)
    print(f"{what}: rel-L2 {r:.2e}, max-elem {mx:.2e} (gate {tol:.0e})")
    assert r <= tol and (mx <= tol or not elem), (what, r, mx)


def _run(model, x, gy):
    model.zero_grad(set_to_none=True)
    xd = x.to(DEV).requires_grad_(True)
    y = model(xd)
    y.backward(gy.to(DEV))
    return y.detach(), xd.grad, {k: p.grad for k, p in model.named_parameters()}


def _golden_chain(name, tag):
    from models.mlp import MLP
    d, meta = load(f"act_{name}_f64")
    sd = {k[len(tag) + 3:]: v for k, v in d.items() if k.startswith(f"{tag}:p:")}
    m = MLP(activation_fn=name, **meta[tag]).double()  # (before loading: float32 parameters would round them)
    m.load_state_dict(sd, strict=True)
    return m, sd, {k[len(tag) + 1:]: v for k, v in d.items() if k.startswith(f"{tag}:") and ":p:" not in k}


@pm("tag", ["a", "b"], ids=["ln-nh2", "out4-nh1"])
@pm("name", A.NEW)
def test_mlp_matches_the_reference(name, tag):
    """models.mlp.MLP with the golden parameters, forward and backward with the golden upstream gradient, in
    float64 at 1e-10 and in fp32 at 1e-5 / 1e-5 / 5e-5 (rel-L2 and max-element) against the reference."""
    for dt, (fwd, gin, gpar) in ((torch.float64, (F64,) * 3), (torch.float32, (FWD, GIN, GPAR))):
        m, _, g = _golden_chain(name, tag)
        y, gx, gp = _run(m.to(dt).to(DEV), g["x"].to(dt), g["gy"].to(dt))
        assert y.dtype == dt
        _gate(f"{name} {tag} {dt} y", y, g["y"], fwd)
        _gate(f"{name} {tag} {dt} gx", gx, g["gx"], gin)
        for k, v in gp.items():
            _gate(f"{name} {tag} {dt} gp:{k}", v, g["gp:" + k], gpar)


@pm("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pm("tag", ["a", "b"], ids=["ln-nh2", "out4-nh1"])
@pm("name", A.NEW)
def test_mlp_16bit_against_float64_on_the_rounded_operands(name, tag, dtype):
    """The same chains with parameters, rows and upstream gradient rounded to the 16-bit type, against the
    float64 formula on those rounded operands, rel-L2 at 2e-2 (test_gpu_mlp_general.B16)."""
    m, sd, g = _golden_chain(name, tag)
    sd16 = {k: v.to(dtype) for k, v in sd.items()}
    x, gy = g["x"].to(dtype), g["gy"].to(dtype)
    ry, rgx, rgp = ref_chain(sd16, x, name, gy)
    y, gx, gp = _run(m.to(dtype).to(DEV), x, gy)
    assert y.dtype == dtype and gx.dtype == dtype
    _gate(f"{name} {tag} {dtype} y", y.float(), ry, B16, elem=False)
    _gate(f"{name} {tag} {dtype} gx", gx.float(), rgx, B16, elem=False)
    for k, v in gp.items():
        _gate(f"{name} {tag} {dtype} gp:{k}", v.float(), rgp[k], B16, elem=False)


# ------------------------------------------------------------------------------ 3. the general kernels' shapes
H = 32
ROWS = (1, 33, 130)
# (K, out, residual, forward mode, backward mode): K = 6 input; K = H with residual; out = H - 7 with LayerNorm
SHAPES = ((6, H, False, M_NIN, M_VEC), (H, H, True, M_VEC, M_VEC), (H, H - 7, False, M_GEN, M_GEN))


def _chain_sd(c):
    sd = {}
    for l, (w, b) in enumerate(zip(c.w, c.b)):
        sd[f"layers.{l}.weight"], sd[f"layers.{l}.bias"] = w.cpu(), b.cpu()
    sd["layer_norm.weight"], sd["layer_norm.bias"] = c.ln[0].cpu(), c.ln[1].cpu()
    return sd


def _direct(name, dtype, shape, rows):
    """One forward, backward and weight-gradient pass of a 3-Linear chain with LayerNorm through
    core.mlp_forward / core.mlp_backward on guarded buffers (test_gpu_mlp_general.run_chain's calls), every
    result against the float64 formula."""
    import test_gpu_mlp_general as T
    from aerognn import _lib as L
    from aerognn import core, functions as Fn
    from maskmatched import rows_of
    K, out_dim, resid, fwd_mode, bwd_mode = shape
    tag = f"{name} {dtype} K {K} out {out_dim} rows {rows}"
    c = T.Chain(H, dtype, K, 3, out_dim, True, act=name, seed=500 + K + out_dim)
    s, sd = c.spec, _chain_sd(c)
    sixteen = dtype != torch.float32
    cand = torch.randn(4 * rows + 256, K, generator=c.gen).to(dtype).float()
    xc = A.kink_free_select(sd, cand.double(), name, rows, rounded=(dtype,) if sixteen else ()).to(dtype)
    gyc = torch.randn(rows, out_dim, generator=c.gen).to(dtype)
    ry, rgx, rgp = ref_chain(sd, xc, name, gyc)
    _, rpre = ref_chain(sd, xc, name)
    if resid:
        ry, rgx = ry + xc.double(), rgx + gyc.double()
    fwd, gin, gpar = (B16,) * 3 if sixteen else (FWD, GIN, GPAR)
    G = T.Guards()
    x = xc.to(DEV)
    y = G.alloc(rows, out_dim, dtype)
    acts, hpre, stats = Fn._alloc_saves(s, rows, dtype, torch.device(DEV), True)
    acts, hpre, stats = [G.rehome(t) for t in acts], G.rehome(hpre), G.rehome(stats)
    for t in acts:  # pre[l] is written by the forward: a value no pre-activation has, until then
        core._pre_of(t).fill_(777.0)
    before = _fast_counters()
    core.mlp_forward(rows=rows, dtype=dtype, hidden=H, nlin=3, act_fn=s.act, out_dim=out_dim,
                     segs=[(L.SEG_PLAIN, K, x.stride(0), x, None, None)], wpk=s.wpk(), bias=s.biases(), ln=s.lnp(),
                     out=y, resid=x if resid else None, acts=acts, hpre=hpre, stats=stats)
    torch.cuda.synchronize()
    assert T._mode(0) == fwd_mode, (tag, "forward mode", T._mode(0))
    for l, t in enumerate(acts):
        pre = rows_of(core._pre_of(t), rows)
        _gate(f"{tag} pre[{l}]", pre.float(), rpre[l], fwd, elem=not sixteen)
    _gate(f"{tag} y", y.float(), ry, fwd, elem=not sixteen)
    g = gyc.to(DEV)
    gpre = [G.rehome(t) for t in Fn._alloc_gpre(s, rows, dtype, torch.device(DEV), rowmajor=range(3))]
    din = G.alloc(rows, K, dtype)
    nblk = core.bwd_nblocks(rows)
    part = G.alloc(nblk, 2 * out_dim, torch.float32)
    ln_rows = core.mlp_backward(rows=rows, dtype=dtype, hidden=H, nlin=3, act_fn=s.act, out_dim=out_dim, in_dim=K,
                                wtpk=s.wtpk(), acts=acts, g=g, gpre=gpre, ln_g=s.lnp()[0], hpre=hpre, stats=stats,
                                din=[(K, din, resid)], ln_partial=part)
    torch.cuda.synchronize()
    assert T._mode(1) == bwd_mode, (tag, "backward mode", T._mode(1))
    assert ln_rows == nblk
    _gate(f"{tag} gx", din.float(), rgx, gin, elem=not sixteen)
    grads = Fn._chain_param_grads(s, gpre, [x.contiguous()], acts, part, ln_rows)
    torch.cuda.synchronize()
    assert _fast_counters() == before, (tag, "a ReLU-only fast kernel was launched")
    keys = [f"layers.{l}.{p}" for l in range(3) for p in ("weight", "bias")] + ["layer_norm.weight", "layer_norm.bias"]
    assert len(grads) == len(keys)
    for k, v in zip(keys, grads):
        _gate(f"{tag} gp:{k}", v.float(), rgp[k], gpar, elem=not sixteen)
    G.check()


@pm("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pm("name", A.NEW)
def test_general_kernel_shapes(name, dtype):
    for shape in SHAPES:
        for rows in ROWS:
            _direct(name, dtype, shape, rows)


# ------------------------------------------------------------------------------ 4. with dropout
SEED = 0x1234ABCD5678


@pm("name", ["elu", "hardswish"])
def test_mlp_trains_with_dropout(name):
    """MLP(6, 32, 32, 2, activation_fn=name, dropout=0.25).train(): one forward and backward in fp32 against
    the float64 formula under the masks reproduced from the generator's (seed, offset), as
    tests/test_gpu_dropout.py does for gelu (LayerNorm parameters drawn off (1, 0), as its goldens)."""
    from models.mlp import MLP
    p, rows, offset = 0.25, 40, 4 * 12
    torch.manual_seed(31)
    m = MLP(6, 32, 32, 2, activation_fn=name, dropout=p)
    with torch.no_grad():
        m.layer_norm.weight.uniform_(0.5, 1.5)
        m.layer_norm.bias.normal_(0.0, 0.5)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    x = torch.randn(rows, 6, generator=torch.Generator().manual_seed(32))
    stream = D.MaskStream(SEED, offset, p)
    masks = [stream.next((rows, 32)) for _ in range(3)]
    ry, rgx, rgp = D.chain(sd, x, masks, p, act=name, dtype=torch.float64)
    m = m.to(DEV).train()
    torch.manual_seed(SEED)
    gen = torch.cuda.default_generators[torch.cuda.current_device()]
    gen.set_offset(offset)
    xd = x.to(DEV).requires_grad_(True)
    y = m(xd)
    y.square().mean().backward()
    assert gen.get_offset() == offset + 3 * D.advance(rows * 32)
    _gate(f"{name} dropout y", y, ry, FWD)
    _gate(f"{name} dropout gx", xd.grad, rgx, GIN)
    for k, v in m.named_parameters():
        _gate(f"{name} dropout gp:{k}", v.grad, rgp[k], GPAR)


# ------------------------------------------------------------------------------ 5. one model
def test_meshgraphnet_step_with_leaky_relu():
    """MeshGraphNet(hidden 32, 2 processor layers, activation_fn='leaky_relu') on the irregular `hub` graph:
    one fp32 training step (forward, MSE loss, backward) against the same step in float64 with plain torch
    (oracle/refcpu.py mgn_forward, F.leaky_relu) from the same state_dict, at the fp32 bars. The biases are
    conditioned off the kink at 0 as smoke() does (tests/kinkfree.py), the inputs are unchanged."""
    import torch.nn.functional as F
    import irregular_graphs as IG
    from kinkfree import kink_free_biases
    from models.mgn import MeshGraphNet
    from oracle import refcpu as R
    n, ei, _ = IG.family("hub")
    pos, _, _ = IG.features(n, ei.shape[1], 1, seed=21)
    g = torch.Generator().manual_seed(22)
    x, ea, tgt = torch.randn(n, 6, generator=g), R.compute_edge_attr(pos, ei), torch.randn(n, 4, generator=g)
    kw = dict(processor_size=2, activation_fn="leaky_relu", num_hidden_layers_node_processor=2,
              num_hidden_layers_edge_processor=2, hidden_dim_processor=32, num_hidden_layers_node_encoder=2,
              hidden_dim_node_encoder=32, num_hidden_layers_edge_encoder=2, hidden_dim_edge_encoder=32,
              aggregation="add", hidden_dim_decoder=32, num_hidden_layers_decoder=2)
    cfg = R.cfg_from_kwargs(**kw)
    torch.manual_seed(2)
    model = MeshGraphNet(6, 4, 4, **kw)
    for _ in range(4):
        p64 = {k: v.detach().double().clone() for k, v in model.state_dict().items()}
        if kink_free_biases(lambda: R.mgn_forward(p64, x.double(), ea.double(), ei, cfg), p64) == 0:
            break
        model.load_state_dict({k: v.float() for k, v in p64.items()})
    else:
        raise AssertionError("conditioned biases not kink-free after the fp32 round-trip")
    p64 = {k: v.detach().double().clone().requires_grad_(True) for k, v in model.state_dict().items()}
    r64 = R.mgn_forward(p64, x.double(), ea.double(), ei, cfg)
    rloss = F.mse_loss(r64, tgt.double())
    rloss.backward()
    before = _fast_counters()
    model = model.to(DEV).train()
    pred = model(x.to(DEV), ea.to(DEV), ei.to(DEV))
    loss = F.mse_loss(pred, tgt.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    assert _fast_counters() == before
    _gate("mgn leaky_relu pred", pred, r64.detach(), FWD)
    assert abs(float(loss) - float(rloss)) <= FWD * abs(float(rloss)), (float(loss), float(rloss))
    for k, v in model.named_parameters():
        _gate(f"mgn leaky_relu gp:{k}", v.grad, p64[k].grad, GPAR)
