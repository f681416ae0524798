"""Training-mode dropout on the MI355X: the activation + dropout kernels (csrc/dropout.hip) through
torch.ops.aerognn.act_dropout, and the chains that use them (models/mlp.py, aerognn/f64.py) against the mask-matched goldens of the real reference (tools/make_goldens_dropout.py).

Gates:
  mask: bitwise the numpy restatement (tests/dropoutref.py) in every storage type
  ReLU / no activation: out and dy bitwise torch's CPU arithmetic through the same mask
  GELU / SiLU / Tanh: the per-element tolerance of the general-MLP sweep, tests/savechain.py
      (n - 1/2) ulp_T(|ref| + d) + d with its d for a non-ReLU forward and backward (imported, not
      copied; float64 takes the same form with a 53-bit significand and u = 2^-53)
  goldens: fp32 1e-5 rel-L2 for y and the input gradient, 5e-5 for the parameter gradients; float64 1e-10
  16-bit: 3 x the error of the fused chain at p = 0 against the same float64 restatement, measured
      in the same test on the same weights and inputs
"""
import os

import numpy as np
import pytest
import torch

import dropoutref as D
import savechain as S
from golden_util import load, params, rel_l2

pytestmark = pytest.mark.gpu
os.environ.setdefault("AEROGNN_MEMLOG", "0")

DEV = "cuda"
FWD, GIN, GPAR, F64 = 1e-5, 1e-5, 5e-5, 1e-10
DTYPES = [torch.float32, torch.bfloat16, torch.float16, torch.float64]
IDS = ["fp32", "bf16", "fp16", "fp64"]
SEED = 0x1234ABCD5678  # above 2^32: both key words are in use


def _ops():
    import aerognn.ops  # noqa: F401  (registers torch.ops.aerognn.*)
    return torch.ops.aerognn


def _gen():
    return torch.cuda.default_generators[torch.cuda.current_device()]


def _seed(seed, offset=0):
    torch.manual_seed(seed)
    _gen().set_offset(offset)


def _bits(t):
    return t.detach().cpu().contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _scaled(a, scale, dtype):
    """round_T(float(a) * (float)scale), fp64 in double: the kernel's product on the CPU."""
    if dtype == torch.float64:
        return a * scale
    return (a.float() * torch.tensor(scale, dtype=torch.float32)).to(dtype)


# ------------------------------------------------------------------------------ fails without the feature
def _mlp(dropout, dtype=torch.float32, seed=3, **kw):
    from models.mlp import MLP
    torch.manual_seed(seed)
    m = MLP(6, 32, 32, 2, dropout=dropout, **kw)
    return (m.double() if dtype == torch.float64 else m.to(dtype)).to(DEV)


@pytest.mark.parametrize("how", ["forward", "forward_rows", "float64", "no_grad"])
def test_mlp_trains_with_dropout(how):
    dt = torch.float64 if how == "float64" else torch.float32
    m = _mlp(0.25, dt).train()
    x = torch.randn(40, 6, dtype=dt, device=DEV)
    if how == "forward_rows":
        rows = torch.randperm(40, device=DEV)[:33]
        y = m.forward_rows(x, rows)
        assert y.shape == (33, 32)
    elif how == "no_grad":  # nn.Dropout drops under no_grad too: only eval() or p = 0 turns it off
        with torch.no_grad():
            y = m(x)
        assert not torch.equal(y, m.eval()(x))
        return
    else:
        y = m(x)
    y.square().mean().backward()
    assert bool(torch.isfinite(y).all())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())


# ------------------------------------------------------------------------------ the mask
def _pass_elems():
    from aerognn import _lib as L
    return int(L.lib().agn_act_dropout_pass_elems())


def _check_mask(y, p, offset=4 * 12):
    _seed(SEED, offset)
    out, mask = _ops().act_dropout(y, "relu", p)
    n = y.numel()
    assert _gen().get_offset() == offset + D.advance(n)
    want = D.pack_bits(D.keep_mask(SEED, offset, n, p))
    got = mask.cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got, want), (tuple(y.shape), p, offset)
    return out, mask


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_mask_is_the_restatement_s(dtype):
    g = torch.Generator().manual_seed(1)
    shapes = [(1,), (3,), (4,), (5,), (7,), (8,), (9,), (15,), (3, 5), (31, 32), (33, 64), (129, 128)]
    for p in (0.1, 0.25, 0.5, 0.9):
        for sh in shapes:
            _check_mask(torch.randn(*sh, generator=g).to(dtype).to(DEV), p)
    base = torch.randn(33 * 64 + 16, generator=g).to(dtype).to(DEV)
    for start in (1, 16):  # a view off the 16-B alignment by one element (scalar path), and an aligned one
        v = base[start:start + 33 * 64].view(33, 64)
        assert (v.data_ptr() % 16 == 0) == (start == 16)
        _check_mask(v, 0.25)
    # the 64-bit block counter carries across 2^32 (and an offset that is far from 0)
    _check_mask(torch.randn(32, generator=g).to(dtype).to(DEV), 0.5, offset=4 * (2 ** 32 - 2))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float64], ids=["bf16", "fp64"])
def test_mask_past_one_pass_of_the_grid(dtype):
    """The grid is capped (agn_act_dropout_pass_elems elements per pass): a tensor of one pass plus a
    few groups and a tail takes the grid-stride step."""
    n = _pass_elems() + 8 * 300 + 5
    y = torch.ones(n, dtype=dtype, device=DEV)
    out, mask = _check_mask(y, 0.25)
    kept = torch.from_numpy(D.keep_mask(SEED, 4 * 12, n, 0.25))
    want = torch.where(kept, _scaled(torch.ones(n, dtype=dtype), 1.0 / 0.75, dtype), torch.zeros(n, dtype=dtype))
    assert _same(out, want)


def test_mask_does_not_depend_on_the_storage_type():
    masks = []
    for dtype in DTYPES:
        _seed(SEED, 8)
        masks.append(_ops().act_dropout(torch.ones(129, 33, dtype=dtype, device=DEV), "none", 0.25)[1])
    assert all(torch.equal(m, masks[0]) for m in masks[1:])


def test_keep_fraction():
    n, p = 129 * 32, 0.25
    _seed(1234, 0)
    out, mask = _ops().act_dropout(torch.ones(129, 32, device=DEV), "none", p)
    kept = int(D.unpack_bits(mask.cpu().numpy(), n).sum())
    sigma = (n * p * (1 - p)) ** 0.5
    ref = int(D.keep_mask(1234, 0, n, p).sum())
    print(f"kept {kept} of {n} ({kept / n:.4f}), {abs(kept - n * (1 - p)) / sigma:.2f} sigma from the mean")
    assert abs(ref - n * (1 - p)) <= 4 * sigma and kept == ref
    assert int((out != 0).sum()) == kept


# ------------------------------------------------------------------------------ values
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("act", ["relu", "none"])
def test_relu_and_none_are_bitwise_torch_s(act, dtype):
    g = torch.Generator().manual_seed(2)
    for sh, p in (((33, 64), 0.25), ((7,), 0.5), ((129, 33), 0.1)):
        y0 = torch.randn(*sh, generator=g).to(dtype)
        g0 = torch.randn(*sh, generator=g).to(dtype)
        scale = 1.0 / (1.0 - p)
        _seed(SEED, 4)
        y = y0.to(DEV).requires_grad_(True)
        out, mask = _ops().act_dropout(y, act, p)
        out.backward(g0.to(DEV))
        kept = torch.from_numpy(D.keep_mask(SEED, 4, y0.numel(), p)).view(sh)
        a = torch.relu(y0) if act == "relu" else y0
        zero = torch.zeros(sh, dtype=dtype)
        assert _same(out, torch.where(kept, _scaled(a, scale, dtype), zero))
        da = torch.where(kept, _scaled(g0, scale, dtype), zero)
        assert _same(y.grad, torch.where(y0 > 0, da, zero) if act == "relu" else da)


def _ulp64(x):
    _, e = torch.frexp(x)
    e = torch.where(x > 0, e - 1, torch.full_like(e, -1022)).clamp_min(-1022)
    return torch.ldexp(torch.ones_like(x), e - 52)


def _check(name, got, ref, d, dtype, n):
    """tests/savechain.py's per-element tolerance; for float64 the same form with 53 bits."""
    if dtype != torch.float64:
        return S.check(name, got, ref, d, dtype, n=n)
    ratio = float(((got.detach().cpu() - ref).abs() / ((n - 0.5) * _ulp64(ref.abs() + d) + d)).max())
    print(f"  save-chain {name}: worst |got - ref| / tolerance {ratio:.3f} (n = {n}, float64)")
    assert ratio <= 1.0, (name, ratio)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("act", ["gelu", "silu", "tanh"])
def test_other_activations_within_the_sweep_s_tolerance(act, dtype):
    """Forward: a = round_T(f(y)) from the stored y (d = 8 u (|y| + |f|), savechain's non-ReLU forward),
    out = round_T(a * scale): two roundings, and the fp32 product adds u |ref|. Backward: da =
    round_T(g * scale) is the inner rounding of savechain's n = 2 non-ReLU backward, ref = g scale f'(y),
    d = u |g scale| |f'| + |g scale| 8 u A + 4 u |ref| (tanh: f' from the stored activation a)."""
    u = S.U if dtype != torch.float64 else 2.0 ** -53
    g = torch.Generator().manual_seed(5)
    sh, p = (65, 48), 0.25
    y0 = (2.0 * torch.randn(*sh, generator=g)).to(dtype)
    g0 = torch.randn(*sh, generator=g).to(dtype)
    scale = 1.0 / (1.0 - p) if dtype == torch.float64 else float(torch.tensor(1.0 / (1.0 - p), dtype=torch.float32))
    _seed(SEED, 4)
    y = y0.to(DEV).requires_grad_(True)
    out, mask = _ops().act_dropout(y, act, p)
    out.backward(g0.to(DEV))
    a_stored = S.f64(_ops().act_dropout(y.detach(), act, 0.0)[0])  # p = 0: act(y) as the kernel rounds it
    kept = torch.from_numpy(D.keep_mask(SEED, 4, y0.numel(), p)).view(sh).double()
    x = S.f64(y0)
    f = S.act_f(act, x)
    d_a = 8.0 * u * (x.abs() + f.abs())
    _check(f"{act} a", a_stored, f, d_a, dtype, 1)
    ref = f * scale * kept
    _check(f"{act} out", S.f64(out), ref, (d_a * scale + u * ref.abs()) * kept, dtype, 2)
    df, A = S.act_df(act, x, a_stored)
    gs = S.f64(g0) * scale * kept
    ref = gs * df
    _check(f"{act} dy", S.f64(y.grad), ref, u * gs.abs() * df.abs() + gs.abs() * 8.0 * u * A + 4.0 * u * ref.abs(),
           dtype, 2)
    assert bool((S.f64(out)[kept == 0] == 0).all()) and bool((S.f64(y.grad)[kept == 0] == 0).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_edge_probabilities(dtype):
    g = torch.Generator().manual_seed(6)
    y0 = torch.randn(33, 40, generator=g).to(dtype)
    y = y0.to(DEV).requires_grad_(True)
    from aerognn.ops import act_dropout
    out = act_dropout(y, "gelu", 1.0)
    out.backward(torch.ones_like(out))
    assert not bool(out.any()) and not bool(y.grad.any())
    _seed(SEED, 16)
    for act, want in (("relu", torch.relu(y0)), ("none", y0)):
        assert _same(act_dropout(y.detach(), act, 0.0), want)                  # p = 0: act(y), bitwise
        assert _same(act_dropout(y.detach(), act, 0.5, training=False), want)  # not training: the same
    assert _gen().get_offset() == 16  # neither draws


# ------------------------------------------------------------------------------ the generator
def _step(m, x, dt):
    m.zero_grad(set_to_none=True)
    xx = x.clone().requires_grad_(True)
    y = m(xx)
    y.float().square().mean().backward() if dt in (torch.bfloat16, torch.float16) else y.square().mean().backward()
    return [y.detach(), xx.grad] + [p.grad.clone() for p in m.parameters()]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_generator_replays_and_advances(dtype):
    m = _mlp(0.25, dtype).train()
    x = torch.randn(40, 6, generator=torch.Generator().manual_seed(7)).to(dtype).to(DEV)
    _seed(SEED, 40)
    a = _step(m, x, dtype)
    after = _gen().get_offset()
    assert after == 40 + 3 * D.advance(40 * 32)  # three dropouts over [40, 32] activations
    b = _step(m, x, dtype)  # not reseeded: the next counter range
    assert _gen().get_offset() == after + 3 * D.advance(40 * 32)
    assert not torch.equal(a[0], b[0])
    _seed(SEED, 40)
    c = _step(m, x, dtype)
    assert all(_same(s, t) for s, t in zip(a, c))
    _seed(SEED, after)      # the second call's masks are those at the advanced offset
    d = _step(m, x, dtype)
    assert all(_same(s, t) for s, t in zip(b, d))


def test_second_call_uses_the_advanced_offset():
    y = torch.ones(33, 5, device=DEV)
    _seed(SEED, 0)
    m1 = _ops().act_dropout(y, "none", 0.5)[1]
    m2 = _ops().act_dropout(y, "none", 0.5)[1]
    n = y.numel()
    assert np.array_equal(m1.cpu().numpy(), D.pack_bits(D.keep_mask(SEED, 0, n, 0.5)))
    assert np.array_equal(m2.cpu().numpy(), D.pack_bits(D.keep_mask(SEED, D.advance(n), n, 0.5)))
    assert D.advance(n) == 168 and not torch.equal(m1, m2)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_eval_and_p0_stay_on_the_fused_path(dtype):
    """eval() and p = 0 give bitwise what a module built with dropout=0.0 and the same weights gives."""
    drop, plain = _mlp(0.25, dtype), _mlp(0.0, dtype)
    plain.load_state_dict(drop.state_dict())
    x = torch.randn(40, 6, generator=torch.Generator().manual_seed(8)).to(dtype).to(DEV)
    ref = _step(plain.train(), x, dtype)
    off = _gen().get_offset()
    assert all(_same(s, t) for s, t in zip(_step(drop.eval(), x, dtype), ref))
    drop.train()
    drop.dropout.p = 0.0
    assert all(_same(s, t) for s, t in zip(_step(drop, x, dtype), ref))
    assert _gen().get_offset() == off
    rows = torch.randperm(40, device=DEV)[:17]
    assert _same(drop.forward_rows(x, rows), plain.forward_rows(x, rows))


# ------------------------------------------------------------------------------ the reference's goldens
CASES = ["drop_mlp_relu_ln", "drop_mlp_gelu", "drop_mlp_nh0"]


def _module(meta, dropout=None):
    from models.mlp import MLP
    kw = dict(meta["kwargs"])
    if dropout is not None:
        kw["dropout"] = dropout
    return MLP(**kw)


def _golden_step(m, d, dtype, loss32=False):
    x = d["x"].to(dtype).to(DEV).requires_grad_(True)
    y = m(x)
    (y.float() if loss32 else y).square().mean().backward()
    return y.detach(), x.grad, {k: p.grad for k, p in m.named_parameters()}


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("name", CASES)
def test_chain_matches_the_reference_through_the_same_masks(name, prec):
    d, meta = load(name)
    ref = d if prec == "f32" else load(name + "_f64")[0]
    dt = torch.float32 if prec == "f32" else torch.float64
    fwd, gin, gpar = (FWD, GIN, GPAR) if prec == "f32" else (F64,) * 3
    m = _module(meta)
    m.load_state_dict(params(d), strict=True)
    m = m.to(dt).to(DEV).train()
    _seed(meta["seed"], meta["offset"])
    y, gx, gp = _golden_step(m, d, dt)
    assert _gen().get_offset() == meta["offset"] + meta["dropout_calls"] * D.advance(meta["rows"] * 32)
    ey, egx = rel_l2(y.cpu(), ref["y"]), rel_l2(gx.cpu(), ref["gx"])
    egp = {k: rel_l2(g.cpu(), ref["gp:" + k]) for k, g in gp.items()}
    worst = max(egp.items(), key=lambda t: t[1])
    print("  " + ", ".join(f"{k} {v:.2e}" for k, v in egp.items()))
    print(f"{name} {prec}: y {ey:.3e} (gate {fwd:.0e}), gx {egx:.3e} ({gin:.0e}), worst gp {worst[1]:.3e} "
          f"({worst[0]}; {gpar:.0e})")
    assert ey <= fwd and egx <= gin and worst[1] <= gpar, (ey, egx, worst)
    if meta["dropout_calls"] == 0:  # one Linear: the p = 0 module's output, bit for bit
        m0 = _module(meta, dropout=0.0)
        m0.load_state_dict(params(d), strict=True)
        m0 = m0.to(dt).to(DEV).train()
        assert _same(m0(d["x"].to(dt).to(DEV)), y)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", ["drop_mlp_relu_ln", "drop_mlp_gelu"])
def test_16bit_chain_within_three_times_the_fused_chain_s_error(name, dtype):
    """Reference: the float64 restatement (dropoutref.chain) on the weights and inputs rounded to the
    storage type (the golden's weights; its inputs, conditioned away from ReLU kinks). Ours with dropout
    through the recorded masks against it; the existing fused chain at p = 0 against the same restatement
    with all-ones masks; the gate is 3 x the latter, per quantity."""
    d, meta = load(name)
    act = meta["kwargs"].get("activation_fn", "relu")
    sd16 = {k: v.to(dtype) for k, v in params(d).items()}
    shapes = D.mask_shapes(meta)
    s = D.MaskStream(meta["seed"], meta["offset"], meta["p"])
    masks = [s.next(sh) if sh is not None else None for sh in shapes]
    x16 = d["x"].to(dtype)
    if act == "relu":
        # rows within 2 eps_T of a ReLU kink re-drawn (dropoutref.kink_free_rows): the 16-bit pre-activations
        # are about eps_T from the float64 ones, and an element on the other side of 0 moves a gradient by
        # percents whichever code computes it, which is no measure of either code
        x16 = D.kink_free_rows(sd16, x16, [(masks, meta["p"]), ([None] * len(shapes), 0.0)],
                               torch.Generator().manual_seed(9), 2.0 * torch.finfo(dtype).eps)
    d16 = dict(d, x=x16)
    errs = {}
    for label, drop, mk, p in (("dropout", None, masks, meta["p"]), ("fused p=0", 0.0, [None] * len(shapes), 0.0)):
        m = _module(meta, dropout=drop)
        m.load_state_dict(params(d), strict=True)
        m = m.to(dtype).to(DEV).train()
        _seed(meta["seed"], meta["offset"])
        y, gx, gp = _golden_step(m, d16, dtype, loss32=True)
        ry, rgx, rgp = D.chain(sd16, d16["x"], mk, p, act=act, dtype=torch.float64)
        errs[label] = (rel_l2(y.cpu(), ry), rel_l2(gx.cpu(), rgx), max(rel_l2(g.cpu(), rgp[k]) for k, g in gp.items()))
    for i, what in enumerate(("y", "gx", "worst gp")):
        e, b = errs["dropout"][i], errs["fused p=0"][i]
        print(f"{name} {dtype} {what}: dropout {e:.3e}, fused p = 0 {b:.3e} (ratio {e / b:.2f}, gate 3)")
    for i, what in enumerate(("y", "gx", "worst gp")):
        assert errs["dropout"][i] <= 3.0 * errs["fused p=0"][i], (what, errs)


# ------------------------------------------------------------------------------ models
def _mesh(dtype):
    from aerognn.meshgen import collate, ellipsoid
    b = collate([ellipsoid(12, 8)])
    t = {k: torch.from_numpy(b[k]).to(dtype).to(DEV) for k in ("x", "edge_attr", "y", "pos")}
    t["edge_index"], t["batch"] = torch.from_numpy(b["edge_index"]).to(DEV), torch.from_numpy(b["batch"]).to(DEV)
    return t


def _build(name, dropout):
    mgn = dict(input_node_dim=6, input_edge_dim=4, output_node_dim=4, processor_size=2, activation_fn="relu",
               num_hidden_layers_node_processor=2, num_hidden_layers_edge_processor=2, hidden_dim_processor=32,
               num_hidden_layers_node_encoder=2, hidden_dim_node_encoder=32, num_hidden_layers_edge_encoder=2,
               hidden_dim_edge_encoder=32, aggregation="add", hidden_dim_decoder=32, num_hidden_layers_decoder=2,
               dropout=dropout)
    if name == "MeshGraphNet":
        from models.mgn import MeshGraphNet
        return MeshGraphNet(**mgn)
    if name == "BiStridedMeshGraphNet":
        from models.bsms_mgn import BiStridedMeshGraphNet
        return BiStridedMeshGraphNet(**mgn, num_scales=2, layers_per_scale=1, stride=2)
    if name == "poolMGN":
        from models.poolmgn import poolMGN
        return poolMGN(**mgn, global_pool_method="mean", num_hidden_layers_global_encoder=2, global_dim=32)
    if name == "FourierMeshGraphNet":
        from models.fouriermgn import FourierMeshGraphNet
        return FourierMeshGraphNet(**mgn, fourier_features_dim=2, fourier_freq_start=-3, fourier_freq_length=7)
    from models.mlpnet import MLPNet
    assert name == "MLPNet"
    return MLPNet(input_node_dim=6, output_node_dim=4, hidden_dim=32, num_hidden_layers_encoder=2,
                  num_hidden_layers_decoder=2, activation_fn="relu", dropout=dropout)


def _call(model, t):
    cls = model.__class__.__name__
    if cls == "poolMGN":
        return model(t["x"], t["edge_attr"], t["edge_index"], t["batch"])
    if cls == "BiStridedMeshGraphNet":
        return model(t["x"], t["edge_attr"], t["edge_index"], batch=t["batch"], pos=t["pos"])
    if cls == "MLPNet":
        return model(t["x"])
    return model(t["x"], t["edge_attr"], t["edge_index"])


def _model_step(model, t):
    model.zero_grad(set_to_none=True)
    pred = _call(model, t)
    loss = torch.nn.functional.mse_loss(pred.float() if pred.dtype != torch.float64 else pred,
                                        t["y"].float() if pred.dtype != torch.float64 else t["y"])
    loss.backward()
    assert bool(torch.isfinite(loss))
    grads = [p.grad.clone() for p in model.parameters() if p.grad is not None]
    assert grads and all(bool(torch.isfinite(g).all()) for g in grads)
    return [loss.detach().clone()] + grads


MODELS = [(n, torch.float32) for n in ("MeshGraphNet", "BiStridedMeshGraphNet", "poolMGN", "FourierMeshGraphNet",
                                       "MLPNet")] + \
    [("MeshGraphNet", torch.bfloat16), ("MeshGraphNet", torch.float64)]


@pytest.mark.parametrize("name,dtype", MODELS, ids=[f"{n}-{str(d).split('.')[1]}" for n, d in MODELS])
def test_model_train_step_with_dropout(name, dtype):
    t = _mesh(dtype)
    torch.manual_seed(11)
    drop = _build(name, 0.1)
    plain = _build(name, 0.0)
    plain.load_state_dict(drop.state_dict())
    drop, plain = (m.to(dtype).to(DEV).train() for m in (drop, plain))
    _seed(SEED, 0)
    a = _model_step(drop, t)
    assert _gen().get_offset() > 0
    _seed(SEED, 0)
    b = _model_step(drop, t)
    assert len(a) == len(b) and all(_same(s, u) for s, u in zip(a, b))  # bitwise repeatable after reseeding
    c = _model_step(plain, t)
    assert not torch.equal(a[0], c[0])  # and not the dropout = 0 step
