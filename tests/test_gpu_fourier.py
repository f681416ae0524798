"""agn_fourier_embed / agn_fourier_embed_bwd, FourierMeshGraphNet and MLPNet on the MI355X against
golden vectors of the real reference (tools/make_goldens_fourier.py) and a float64 formula.

Gates (measured worst values: DESIGN.md "Fourier features"):
  kernel vs fourier_embed_f32: forward max|diff| <= 2^-22 (both sides within 1 ulp = 2^-24 of the
      exact trig of the same fp32 argument, so 2^-23 apart at most; the gate is twice that);
      gx rel-L2 <= 1e-5 (the project's input-gradient bar)
  kernel vs fourier_embed_f64: forward max|diff| <= 2^-50, gx rel-L2 <= 1e-10 (test_gpu_f64.py's gate)
  bf16 / f16 vs the float64 formula on the rounded input: max|diff| <= 2^-8 / 2^-11 (one ulp of the
      format below 1.0; a single correct rounding gives half of it)
  models, fp32: forward rel-L2 and max-element <= 1e-5, input grads 1e-5, parameter grads 5e-5
      (the project bars of test_gpu_parity.py); float64: 1e-10
  mlpnet_f32 forward: max(1e-5, 3 x rel-L2(pred, pred64)) of the fixture: LayerNorm over 4 features
      amplifies fp32 noise, so the reference's own distance from float64 is the yardstick
The shape sweep's elementwise bounds are derived in _bounds below from the formats' roundings alone.
"""
import math
import os

import pytest
import torch

from aerognn import _lib

from golden_util import load, max_rel, params, rel_l2

pytestmark = pytest.mark.gpu
os.environ.setdefault("AEROGNN_MEMLOG", "0")

DEV = "cuda"
FWD = 1e-5
GIN = 1e-5
GPAR = 5e-5
F64 = 1e-10
DTYPES = {"f32": torch.float32, "f64": torch.float64, "bf16": torch.bfloat16, "f16": torch.float16}


def _embed(x, d, fs, fl, with_input):
    from aerognn.functions import FourierEmbedFn
    return FourierEmbedFn.apply(x, d, fs, fl, with_input)


# ------------------------------------------------------------------ the float64 formula and its bounds
def _freqs(fs, fl):
    return (2.0 ** torch.arange(fs, fs + fl, dtype=torch.float64)) * math.pi


def _ref64(x, d, fs, fl, with_input):
    """fouriermgn.py:111-151 (+ the cat of :167-170) in float64 on the given (already rounded) input."""
    xd = x.double()
    a = xd[:, :d, None] * _freqs(fs, fl)
    emb = torch.cat([torch.cos(a), torch.sin(a)], -1).reshape(x.shape[0], -1)
    return torch.cat([xd, emb], -1) if with_input else emb


def _ref64_bwd(x, g, d, fs, fl, with_input):
    xd, gd = x.double(), g.double()
    n, k = x.shape
    f = _freqs(fs, fl)
    a = xd[:, :d, None] * f
    ge = gd[:, k if with_input else 0:].reshape(n, d, 2, fl)
    dx = gd[:, :k].clone() if with_input else torch.zeros(n, k, dtype=torch.float64)
    dx[:, :d] += (f * (torch.cos(a) * ge[:, :, 1] - torch.sin(a) * ge[:, :, 0])).sum(-1)
    return dx


def _bounds(dtype, x, g, d, fs, fl, with_input):
    """Elementwise error bounds of the kernel against the float64 formula, from the roundings only.

    Compute type C (fp32; fp64 for float64) with unit roundoff u; the stored type has unit roundoff
    us. The kernel's argument is fl(f_i' x) with f_i' = 2^i fl(pi): |a' - a| <= |a| (p + u), p =
    |fl(pi) - pi| / pi (2.8e-8 in fp32, 3.9e-17 in fp64); cos / sin are 1-Lipschitz and the device
    functions are taken as within 4u absolute of the exact value (documented: 1 ulp = u below 1.0).
    So every embedding column is within  e = |a| (p + u) 1.01 + 4u  of the formula, plus us (|ref| + e)
    for the store of a 16-bit row (fp16: plus its subnormal spacing 2^-24). The pass-through columns are
    copies: exact. Backward: term_i = f_i' (c gs - s gc) carries the trig error times f_i (|gs| + |gc|),
    the relative error p of f_i' and three roundings; the F + 1 ascending adds round partial sums
    bounded by S = |g_x| + sum_i f_i (|gs_i| + |gc_i|): (F + 4) u S + p S in all, plus the store's us (|ref| + that).
    For float64 the formula itself is computed in the kernel's precision and carries the same
    roundings, so both bounds are doubled there (4u + 4u = 2^-50 for the trig, the golden's gate)."""
    u, p = (2.0 ** -53, 3.9e-17) if dtype == torch.float64 else (2.0 ** -24, 2.8e-8)
    us = {torch.float64: 2.0 ** -53, torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}[dtype]
    sub = 2.0 ** -24 if dtype == torch.float16 else 0.0
    own = 2.0 if dtype == torch.float64 else 1.0
    n, k = x.shape
    f = _freqs(fs, fl)
    a = (x.double()[:, :d, None] * f).abs()
    trig = own * (a * (p + u) * 1.01 + 4 * u)                           # [n, d, F]
    ref = _ref64(x, d, fs, fl, with_input)
    emb_b = torch.cat([trig, trig], -1).reshape(n, -1)
    fwd_b = torch.cat([torch.zeros(n, k, dtype=torch.float64), emb_b], -1) if with_input else emb_b
    fwd_b = fwd_b + (us * (ref.abs() + fwd_b) + sub if dtype in (torch.bfloat16, torch.float16) else 0.0)
    gd = g.double()
    ge = gd[:, k if with_input else 0:].reshape(n, d, 2, fl).abs()
    w = f * (ge[:, :, 0] + ge[:, :, 1])                                  # f_i (|gc| + |gs|)
    S = gd[:, :k].abs().clone() if with_input else torch.zeros(n, k, dtype=torch.float64)
    S[:, :d] += w.sum(-1)
    bwd_b = own * ((fl + 4) * u + p) * S
    bwd_b[:, :d] += (w * trig).sum(-1)
    bwd_b = bwd_b + (us * (_ref64_bwd(x, g, d, fs, fl, with_input).abs() + bwd_b) + sub
                     if dtype in (torch.bfloat16, torch.float16) else 0.0)
    return fwd_b, bwd_b


def _inputs(n, k, dtype, seed, lim=4.0):
    g = torch.Generator().manual_seed(seed)
    x = ((torch.rand(n, k, generator=g, dtype=torch.float64) * 2 - 1) * lim).to(dtype)
    x.view(-1)[0] = 0.0
    x.view(-1)[-1] = -0.0
    return x, g


# ------------------------------------------------------------------ kernel against the reference's goldens
@pytest.mark.parametrize("name,fwd_gate,gx_gate", [("fourier_embed_f32", 2.0 ** -22, GIN),
                                                   ("fourier_embed_f64", 2.0 ** -50, F64)])
def test_kernel_vs_reference_golden(name, fwd_gate, gx_gate):
    d_, meta = load(name)
    fs, fl = meta["freq_start"], meta["freq_len"]
    for d in meta["dims"]:
        x = d_["x"].to(DEV).requires_grad_(True)
        out = _embed(x, d, fs, fl, True)
        assert out.dtype == d_["x"].dtype and out.shape == (257, 6 + 2 * d * fl)
        assert torch.equal(out[:, :6].cpu(), d_["x"])  # -0.0 == 0.0 here; the bit copy is checked in the sweep
        err = float((out[:, 6:].detach().cpu().double() - d_[f"emb_d{d}"].double()).abs().max())
        emb = _embed(x.detach(), d, fs, fl, False)
        assert torch.equal(emb, out[:, 6:])
        out.backward(d_[f"g_d{d}"].to(DEV))
        r = rel_l2(x.grad.cpu(), d_[f"gx_d{d}"])
        print(f"{name} d={d}: forward max|diff| {err:.3e} (gate {fwd_gate:.3e}), gx rel-L2 {r:.3e} (gate {gx_gate:.0e})")
        assert err <= fwd_gate, (d, err)
        assert r <= gx_gate, (d, r)


@pytest.mark.parametrize("dt,gate", [("bf16", 2.0 ** -8), ("f16", 2.0 ** -11)])
def test_kernel_16bit_single_rounding(dt, gate):
    """16-bit rows: fp32 math, one rounding on store; against the float64 formula on the rounded input."""
    d_, meta = load("fourier_embed_f32")
    fs, fl = meta["freq_start"], meta["freq_len"]
    x = d_["x"].to(DTYPES[dt])
    for d in meta["dims"]:
        out = _embed(x.to(DEV), d, fs, fl, True).cpu()
        assert out.dtype == DTYPES[dt]
        assert torch.equal(out[:, :6].view(torch.int16), x.view(torch.int16))
        err = float((out[:, 6:].double() - _ref64(x, d, fs, fl, False)).abs().max())
        print(f"fourier_embed {dt} d={d}: forward max|diff| {err:.3e} (gate {gate:.3e})")
        assert err <= gate, (d, err)


# ------------------------------------------------------------------ shape sweep
@pytest.mark.parametrize("n", [1, 63, 257, 4099])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_shape_sweep(dt, n):
    """Every (k, d) x freq_len x freq_start x with_input at this row count and dtype, forward and
    backward, elementwise within the derived bounds of the float64 formula; pass-through columns are
    bit copies."""
    dtype = DTYPES[dt]
    ibits = {2: torch.int16, 4: torch.int32, 8: torch.int64}[torch.empty(0, dtype=dtype).element_size()]
    worst_f = worst_b = 0.0
    for k, d in ((2, 2), (4, 2), (6, 3), (6, 1)):
        x, gen = _inputs(n, k, dtype, seed=100 * n + 10 * k + d)
        xg = x.to(DEV)
        for fl in (1, 7):
            for fs in (-3, 0):
                for with_input in (0, 1):
                    w = k * with_input + 2 * d * fl
                    g = torch.randn(n, w, generator=gen, dtype=torch.float64).to(dtype)
                    xr = xg.clone().requires_grad_(True)
                    out = _embed(xr, d, fs, fl, bool(with_input))
                    assert out.shape == (n, w) and out.dtype == dtype
                    out.backward(g.to(DEV))
                    out, dx = out.detach().cpu(), xr.grad.cpu()
                    fb, bb = _bounds(dtype, x, g, d, fs, fl, with_input)
                    ef = (out.double() - _ref64(x, d, fs, fl, with_input)).abs()
                    eb = (dx.double() - _ref64_bwd(x, g, d, fs, fl, with_input)).abs()
                    case = (k, d, fl, fs, with_input)
                    assert bool((ef <= fb).all()), (case, float((ef - fb).max()))
                    assert bool((eb <= bb).all()), (case, float((eb - bb).max()))
                    if with_input:
                        assert torch.equal(out[:, :k].view(ibits), x.view(ibits)), case
                        assert torch.equal(dx[:, d:].view(ibits), g[:, d:k].contiguous().view(ibits)), case
                    elif d < k:
                        assert not bool(dx[:, d:].any()), case
                    worst_f = max(worst_f, float((ef / fb.clamp(min=1e-300)).max()))
                    worst_b = max(worst_b, float((eb / bb.clamp(min=1e-300)).max()))
    print(f"sweep {dt} n={n}: worst error / bound forward {worst_f:.3f}, backward {worst_b:.3f}")


@pytest.mark.parametrize("dt", list(DTYPES))
def test_column_slice_input_is_read_in_place(dt):
    """An input that is a column slice of a wider tensor (ld > k) is read through its row stride:
    no copy, and the results are bitwise those of the contiguous copy."""
    from aerognn.functions import _rows_ld
    dtype = DTYPES[dt]
    wide, gen = _inputs(257, 9, dtype, seed=7)
    wide = wide.to(DEV)
    x = wide[:, 2:8]
    assert x.stride(0) == 9 and _rows_ld(x) is x
    g = torch.randn(257, 6 + 28, generator=gen, dtype=torch.float64).to(dtype).to(DEV)
    res = []
    for xin in (x, x.contiguous()):
        xr = xin.detach().requires_grad_(True)
        out = _embed(xr, 2, -3, 7, True)
        out.backward(g)
        res.append((out.detach(), xr.grad))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert res[0][1].shape == (257, 6)
    # the op takes the same path, and a strided gradient too
    import aerognn.ops  # noqa: F401
    assert torch.equal(torch.ops.aerognn.fourier_embed(x, 2, -3, 7, True), res[0][0])
    gw = torch.zeros(257, 40, dtype=dtype, device=DEV)
    gw[:, 3:37] = g
    assert torch.equal(torch.ops.aerognn.fourier_embed_backward(gw[:, 3:37], x, 2, -3, 7, True), res[0][1])


def test_two_runs_bitwise_equal():
    x, gen = _inputs(4099, 6, torch.float32, seed=3)
    x = x.to(DEV)
    g = torch.randn(4099, 6 + 42, generator=gen).to(DEV)
    runs = []
    for _ in range(2):
        xr = x.clone().requires_grad_(True)
        out = _embed(xr, 3, -3, 7, True)
        out.backward(g)
        runs.append((out.detach().clone(), xr.grad.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_backward_runs_only_when_the_input_needs_a_gradient():
    from aerognn import core
    x = torch.randn(63, 6, device=DEV)
    w = torch.ones(6 + 28, device=DEV, requires_grad=True)
    core.PROF = prof = []
    try:
        (_embed(x, 2, -3, 7, True) * w).sum().backward()
        no_grad = [t for t, *_ in prof]
        del prof[:]
        xr = x.clone().requires_grad_(True)
        (_embed(xr, 2, -3, 7, True) * w).sum().backward()
        with_grad = [t for t, *_ in prof]
    finally:
        core.PROF = None
    assert no_grad == ["fourier_embed"], no_grad
    assert with_grad == ["fourier_embed", "fourier_embed_bwd"], with_grad


def test_op_autograd_is_the_backward_op():
    import aerognn.ops  # noqa: F401
    x, gen = _inputs(63, 4, torch.float32, seed=5)
    g = torch.randn(63, 4 + 8, generator=gen).to(DEV)
    xr = x.to(DEV).requires_grad_(True)
    out = torch.ops.aerognn.fourier_embed(xr, 2, 0, 2, True)
    out.backward(g)
    x2 = x.to(DEV).requires_grad_(True)
    out2 = _embed(x2, 2, 0, 2, True)
    out2.backward(g)
    assert torch.equal(out, out2) and torch.equal(xr.grad, x2.grad)
    assert torch.equal(torch.ops.aerognn.fourier_embed_backward(g, x.to(DEV), 2, 0, 2, True), x2.grad)
    empty = torch.ops.aerognn.fourier_embed(torch.empty(0, 4, device=DEV), 2, 0, 2, False)
    assert empty.shape == (0, 8)


# ------------------------------------------------------------------ argument errors
E_ARG, E_DTYPE, E_SHAPE = _lib.E_ARG, _lib.E_DTYPE, _lib.E_SHAPE  # AGN_E_* of include/aerognn.h
# (field overrides, expected code) on a valid call: n = 5, k = 6, ld = 6, d = 2, freq -3 / 7, with_input = 1
BAD = [(dict(x=None), E_ARG), (dict(out=None), E_ARG), (dict(dtype=4), E_DTYPE), (dict(dtype=-1), E_DTYPE),
       (dict(d=0), E_SHAPE), (dict(d=7), E_SHAPE), (dict(freq_len=0), E_SHAPE), (dict(freq_len=33), E_SHAPE),
       (dict(freq_start=-31), E_SHAPE), (dict(freq_start=31, freq_len=1), E_SHAPE),
       (dict(freq_start=24, freq_len=7), E_SHAPE), (dict(ld=5), E_SHAPE), (dict(out_ld=33), E_SHAPE)]
BAD_BWD = [(dict(g=None), E_ARG), (dict(dx=None), E_ARG), (dict(g_ld=33), E_SHAPE), (dict(dx_ld=5), E_SHAPE)]


def test_argument_errors_return_codes_without_a_launch():
    from aerognn import _lib
    L = _lib.lib()
    x = torch.randn(5, 6, device=DEV)
    g = torch.randn(5, 34, device=DEV)
    out = torch.full((5, 34), 7.0, device=DEV)
    dx = torch.full((5, 6), 7.0, device=DEV)
    base = dict(dtype=_lib.F32, n=5, k=6, x=x.data_ptr(), ld=6, d=2, freq_start=-3, freq_len=7, with_input=1)
    names = {E_ARG: "invalid argument", E_DTYPE: "unsupported dtype (f32 / bf16 / f16)", E_SHAPE: "unsupported shape"}

    def fwd(**kw):
        a = {**base, "out": out.data_ptr(), "out_ld": 34, **kw}
        return L.agn_fourier_embed(a["dtype"], a["n"], a["k"], a["x"], a["ld"], a["d"], a["freq_start"], a["freq_len"],
                                   a["with_input"], a["out"], a["out_ld"], None)

    def bwd(**kw):
        a = {**base, "g": g.data_ptr(), "g_ld": 34, "dx": dx.data_ptr(), "dx_ld": 6, **kw}
        return L.agn_fourier_embed_bwd(a["dtype"], a["n"], a["k"], a["x"], a["ld"], a["d"], a["freq_start"],
                                       a["freq_len"], a["with_input"], a["g"], a["g_ld"], a["dx"], a["dx_ld"], None)

    for kw, code in BAD:
        assert fwd(**kw) == code, kw
        if "out" not in kw and "out_ld" not in kw:
            assert bwd(**kw) == code, kw
        assert L.agn_error_string(code).decode() == names[code]
    for kw, code in BAD_BWD:
        assert bwd(**kw) == code, kw
    assert fwd(n=0) == 0 and bwd(n=0) == 0
    assert fwd(n=-1) == E_ARG
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((dx == 7.0).all())  # nothing was launched
    # the Python layer turns a code into an exception carrying agn_error_string's text
    with pytest.raises(_lib.AeroGNNError, match="unsupported shape"):
        _embed(x, 7, -3, 7, True)
    with pytest.raises(_lib.AeroGNNError, match="unsupported shape"):
        _embed(x, 2, -3, 33, True)


# ------------------------------------------------------------------ models
def _fwd_ok(what, got, ref, tol=FWD):
    got = got.detach().float().cpu() if ref.dtype != torch.float64 else got.detach().cpu()
    r, m = rel_l2(got, ref), max_rel(got, ref)
    print(f"{what}: forward rel-L2 {r:.3e}, max-element {m:.3e} (gate {tol:.3e})")
    assert r <= tol and m <= tol, (what, r, m)


def _param_grads_ok(what, model, d, tol):
    worst = ("", 0.0)
    for name, p in model.named_parameters():
        assert p.grad is not None, name
        r = rel_l2(p.grad.cpu(), d["gp:" + name])
        if r > worst[1]:
            worst = (name, r)
    print(f"{what}: worst parameter-grad rel-L2 {worst[1]:.3e} ({worst[0]}; gate {tol:.0e})")
    assert worst[1] <= tol, worst


def _fourier_model(name):
    from models.fouriermgn import FourierMeshGraphNet
    d, meta = load(name)
    model = FourierMeshGraphNet(*meta["dims"], **meta["kwargs"])
    if d["x"].dtype == torch.float64:
        model = model.double()
    model.load_state_dict(params(d), strict=True)
    return model.to(DEV), d


@pytest.mark.parametrize("name,fwd,gin,gpar", [("fouriermgn3_f32", FWD, GIN, GPAR), ("fouriermgn3_f64", F64, F64, F64)])
def test_fouriermgn_train_step(name, fwd, gin, gpar):
    model, d = _fourier_model(name)
    x = d["x"].to(DEV).requires_grad_(True)
    pred = model(x, d["edge_attr"].to(DEV), d["edge_index"].to(DEV))
    assert pred.dtype == d["x"].dtype
    _fwd_ok(name, pred, d["pred"], fwd)
    loss = torch.nn.functional.mse_loss(pred, d["y"].to(DEV))
    loss.backward()
    lr = abs(float(loss.detach()) - float(d["loss"])) / float(d["loss"])
    r = rel_l2(x.grad.cpu(), d["gx"])
    print(f"{name}: loss rel {lr:.3e}, gx rel-L2 {r:.3e} (gate {gin:.0e})")
    assert lr <= fwd
    assert r <= gin, r
    _param_grads_ok(name, model, d, gpar)


def test_fourier_encoder_h128():
    """The H = 128 node encoder on [x | emb]: K = 34 in one input segment of the general MLP kernel."""
    from models.mlp import MLP
    d, m = load("fourier_enc_h128")
    enc = MLP(m["input_dim"], m["hidden_dim"], m["output_dim"], m["num_hidden_layers"],
              use_layer_norm=m["use_layer_norm"])
    enc.load_state_dict(params(d), strict=True)
    enc = enc.to(DEV)
    x = d["x"].to(DEV).requires_grad_(True)
    y = enc(_embed(x, m["fourier_features_dim"], m["freq_start"], m["freq_len"], True))
    _fwd_ok("fourier_enc_h128", y, d["y"])
    y.backward(d["gy"].to(DEV))
    r = rel_l2(x.grad.cpu(), d["gx"])
    print(f"fourier_enc_h128: gx rel-L2 {r:.3e} (gate {GIN:.0e})")
    assert r <= GIN, r
    _param_grads_ok("fourier_enc_h128", enc, d, GPAR)


def test_mlpnet():
    """MLPNet: the decoder's LayerNorm over output_dim = 4 (general kernel, masked columns)."""
    from models.mlpnet import MLPNet
    d, meta = load("mlpnet_f32")
    model = MLPNet(*meta["dims"], **meta["kwargs"])
    model.load_state_dict(params(d), strict=True)
    model = model.to(DEV)
    own = rel_l2(d["pred"], d["pred64"])
    gate = max(FWD, 3 * own)
    print(f"mlpnet_f32: the reference's fp32 forward is rel-L2 {own:.3e} from float64")
    pred = model(d["x"].to(DEV))
    assert pred.shape == d["pred"].shape
    _fwd_ok("mlpnet_f32", pred, d["pred"], gate)
    torch.nn.functional.mse_loss(pred, d["y"].to(DEV)).backward()
    _param_grads_ok("mlpnet_f32", model, d, GPAR)


def test_fourier_embedding_method_is_the_embedding_columns():
    model, d = _fourier_model("fouriermgn3_f32")
    x = d["x"].to(DEV)
    emb = model.fourier_embedding(x)
    assert emb.shape == (x.shape[0], 28)
    assert torch.equal(emb, _embed(x, 2, -3, 7, True)[:, 6:])


def test_bf16_model_is_the_composition_of_its_pieces():
    """bf16 wiring: forward equals, bitwise, node_encoder(fourier_embed(x)) -> edge_encoder.forward_rows
    -> forward_level per layer -> decoder on the kernel's embedded tensor. (The 16-bit accuracy of the
    embedding is gated above and that of the chains by the existing suite.)"""
    import aerognn.ops  # noqa: F401
    from aerognn.graph import Level
    model, d = _fourier_model("fouriermgn3_f32")
    model = model.to(torch.bfloat16)
    x = d["x"].to(DEV, torch.bfloat16)
    ea = d["edge_attr"].to(DEV, torch.bfloat16)
    ei = d["edge_index"].to(DEV)
    with torch.no_grad():
        pred = model(x, ea, ei)
        level = Level.from_edge_index(ei, x.shape[0])
        xe = torch.ops.aerognn.fourier_embed(x, 2, -3, 7, True)
        assert xe.dtype == torch.bfloat16 and xe.shape == (x.shape[0], 34)
        h = model.node_encoder(xe)
        e = model.edge_encoder.forward_rows(ea, level.perm)
        for layer in model.layers:
            h, e = layer.forward_level(h, e, level)
        manual = model.decoder(h)
    assert pred.dtype == torch.bfloat16 and bool(torch.isfinite(pred.float()).all())
    assert torch.equal(pred, manual)
