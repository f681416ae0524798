"""MeshGraphNet_v2 (models/trial1.py) on the MI355X: golden vectors of the real reference
(tools/make_goldens_trial1.py), the projection-free instantiation of agn_edge_forward32 and its
receiver means through the C ABI, and the layer's fast path against its general path.

Gates:
  goldens, fp32: forward rel-L2 and max-element <= 1e-5, loss 1e-5, input gradient 1e-5, parameter
      gradients 5e-5 (the project bars; the reference's own fp32 step is 2.8e-7 .. 6.3e-7 from float64 on
      these cases); float64: 1e-10
  kernel: bitwise (bf16 compared as int16) against agn_mlp_forward on the same operands, against the
      sum-trick instantiation fed P = [0 | b0], and agg against agn_segment_sum of the kernel's own e'
  layer, AEROGNN_V2_EDGE32 1 against 0: x', e', dx, de bitwise; parameter gradients rel-L2 <= 1e-5,
      the gate of test_gpu_fullsize.py::test_fused_edge_bwd_matches_split (fused backward against the
      split path: the fp32 order of the row sums differs)
  bf16 accuracy of the layer: see test_layer_bf16_accuracy
"""
import ctypes as C
import os

import pytest
import torch

from golden_util import load, max_rel, params, rel_l2

pytestmark = pytest.mark.gpu
os.environ.setdefault("AEROGNN_MEMLOG", "0")

DEV = "cuda"
H = 128
FWD, GIN, GPAR, F64 = 1e-5, 1e-5, 5e-5, 1e-10


def _i16(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_i16(a), _i16(b))


# --------------------------------------------------------------------------- goldens
def _fwd_ok(what, got, ref, tol):
    got = got.detach().cpu()
    assert got.dtype == ref.dtype and got.shape == ref.shape
    r, m = rel_l2(got, ref), max_rel(got, ref)
    print(f"{what}: forward rel-L2 {r:.3e}, max-element {m:.3e} (gate {tol:.0e})")
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


def _model(name):
    from models.trial1 import MeshGraphNet_v2
    d, meta = load(name)
    model = MeshGraphNet_v2(*meta["args"])
    if d["x"].dtype == torch.float64:
        model = model.double()
    model.load_state_dict(params(d), strict=True)
    return model.to(DEV), d


@pytest.mark.parametrize("name,fwd,gin,gpar", [("trial1_f32", FWD, GIN, GPAR), ("trial1_f64", F64, F64, F64)])
def test_train_step(name, fwd, gin, gpar):
    """H = 32, 3 layers, 5-Linear encoders, a two-graph batch: the general kernels (float64: aerognn/f64.py)."""
    model, d = _model(name)
    x = d["x"].to(DEV).requires_grad_(True)
    ea, ei, bt = d["edge_attr"].to(DEV), d["edge_index"].to(DEV), d["batch"].to(DEV)
    pred = model(x, ea, ei, bt)
    _fwd_ok(name, pred, d["pred"], fwd)
    loss = torch.nn.functional.mse_loss(pred, d["y"].to(DEV))
    loss.backward()
    lr = abs(float(loss.detach()) - float(d["loss"])) / float(d["loss"])
    r = rel_l2(x.grad.cpu(), d["gx"])
    print(f"{name}: loss rel {lr:.3e} (gate {fwd:.0e}), gx rel-L2 {r:.3e} (gate {gin:.0e})")
    assert lr <= fwd
    assert r <= gin, r
    _param_grads_ok(name, model, d, gpar)
    with torch.no_grad():  # batch = None: the two meshes pooled as one graph (trial1.py:104-106)
        _fwd_ok(name + " batch=None", model(x.detach(), ea, ei, None), d["pred_nobatch"], fwd)


def test_decoder_with_one_layer():
    """num_decoder_layers = 1 (Linear, ReLU, Linear) and 4-Linear encoders, batch = None."""
    model, d = _model("trial1_dec1")
    assert [type(m).__name__ for m in model.decoder] == ["Linear", "ReLU", "Linear"]
    with torch.no_grad():
        pred = model(d["x"].to(DEV), d["edge_attr"].to(DEV), d["edge_index"].to(DEV), None)
    _fwd_ok("trial1_dec1", pred, d["pred"], FWD)


def _layer_draws(seed, E, width):
    """tools/make_goldens_trial1.py layer_draws: the layer case's e and output gradient of e' are draws
    of one seeded generator instead of stored tensors (two files of < 1 MiB hold the rest)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(E, width, generator=g), torch.randn(E, width, generator=g)


def test_layer_h128():
    """One MeshGraphNetLayer_v2(128) through forward(x, edge_index, edge_attr): edges in shuffled order
    (the round trip through the level's order), receiver 5 and the last node without edges."""
    from models.trial1 import MeshGraphNetLayer_v2
    d, meta = load("trial1_layer_h128")
    dg, _ = load("trial1_layer_h128_g")
    layer = MeshGraphNetLayer_v2(meta["H"])
    layer.load_state_dict(params(d), strict=True)
    layer = layer.to(DEV)
    ei = d["edge_index"]
    deg = torch.bincount(ei[1], minlength=meta["N"])
    assert int(deg[5]) == 0 and int(deg[-1]) == 0 and bool((ei[1][1:] < ei[1][:-1]).any())
    e0, ge_out = _layer_draws(meta["seed"], meta["E"], meta["H"])
    x = d["x"].to(DEV).requires_grad_(True)
    e = e0.to(DEV).requires_grad_(True)
    xo, eo = layer(x, ei.to(DEV), e)
    _fwd_ok("trial1_layer_h128 x'", xo, dg["x_out"], FWD)
    _fwd_ok("trial1_layer_h128 e'", eo, d["e_out"], FWD)
    torch.autograd.backward([xo, eo], [dg["gx_out"].to(DEV), ge_out.to(DEV)])
    rx, re = rel_l2(x.grad.cpu(), dg["gx"]), rel_l2(e.grad.cpu(), dg["ge"])
    print(f"trial1_layer_h128: gx rel-L2 {rx:.3e}, ge rel-L2 {re:.3e} (gate {GIN:.0e})")
    assert rx <= GIN and re <= GIN, (rx, re)
    _param_grads_ok("trial1_layer_h128", layer, dg, GPAR)


# --------------------------------------------------------------------------- the global feature
def _compose(model, x, ea, ei, g_rows):
    """The model's forward from the broadcast global rows on, piece by piece."""
    from aerognn.graph import Level
    level = Level.from_edge_index(ei, x.shape[0])
    h = model.node_encoder(torch.cat((x, g_rows), dim=-1))
    e = model.edge_encoder.forward_rows(ea, level.perm)
    for layer in model.layers:
        h, e = layer.forward_level(h, e, level)
    return model.decode(h)


def test_unsorted_batch_follows_repeat_interleave():
    """trial1.py:102 broadcasts the pooled rows with repeat_interleave(bincount(batch)), which is
    g[batch] only for a non-decreasing batch. Expected pooled rows: the per-graph means (GraphGroups:
    graph g's members are the nodes with batch == g, G = batch.max() + 1) of the global encoder's rows,
    formed here in float64."""
    model, d = _model("trial1_f32")
    x, ea, ei = d["x"].to(DEV), d["edge_attr"].to(DEV), d["edge_index"].to(DEV)
    n = x.shape[0]
    batch = (torch.arange(n) % 3 == 1).long()
    batch[-1] = 2                      # three graphs, interleaved; graph 2 has one node
    bt = batch.to(DEV)
    with torch.no_grad():
        pooled = model.extract_feature(x, ei, bt)
        rows = model.extract_feature(x, ei, torch.arange(n, device=DEV))  # one graph per node: the rows themselves
        rows = rows.cpu().double()
        want = torch.stack([rows[batch == g].mean(0) for g in range(3)])
        assert pooled.shape == (3, 32)
        # an fp32 sum of n rows in any order and one division: |error| <= n 2^-24 mean|row| (first order)
        cnt = torch.bincount(batch).double()[:, None]
        bound = 1.01 * cnt * 2.0 ** -24 * torch.stack([rows[batch == g].abs().mean(0) for g in range(3)])
        err = (pooled.cpu().double() - want).abs()
        print(f"unsorted batch: pooled rows, worst error / bound {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all())
        pred = model(x, ea, ei, bt)
        ri = pooled.repeat_interleave(torch.bincount(bt), dim=0)
        assert not torch.equal(ri, pooled[bt])
        assert torch.equal(pred, _compose(model, x, ea, ei, ri))
        assert not torch.equal(pred, _compose(model, x, ea, ei, pooled[bt]))


def test_eval_mode_dropout_is_the_identity():
    from models.trial1 import MeshGraphNet_v2
    model, d = _model("trial1_f32")
    _, meta = load("trial1_f32")
    drop = MeshGraphNet_v2(*meta["args"], dropout=0.1)
    drop.load_state_dict(params(d), strict=True)
    drop = drop.to(DEV).eval()
    args = (d["x"].to(DEV), d["edge_attr"].to(DEV), d["edge_index"].to(DEV), d["batch"].to(DEV))
    with torch.no_grad():
        assert torch.equal(drop(*args), model.eval()(*args))
    drop.train()
    with pytest.raises(NotImplementedError, match="dropout"):
        drop(*args)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_bf16_model_is_the_composition_of_its_pieces(dtype):
    """16-bit wiring (general kernels at this size): forward equals, bitwise, global encoder -> mean pool ->
    broadcast -> node_encoder(cat) -> edge_encoder.forward_rows -> forward_level per layer -> decoder."""
    from aerognn.functions import BroadcastRowsFn, GlobalPoolFn, GraphGroups
    model, d = _model("trial1_f32")
    model = model.to(dtype)
    x, ea = d["x"].to(DEV, dtype), d["edge_attr"].to(DEV, dtype)
    ei, bt = d["edge_index"].to(DEV), d["batch"].to(DEV)
    with torch.no_grad():
        pred = model(x, ea, ei, bt)
        groups = GraphGroups(bt, x.shape[0], x.device)
        gf = model.extract_feature
        from models.trial1 import _run
        g = GlobalPoolFn.apply(_run(gf.linout, _run(gf.mlp, x)), groups, "mean")
        assert torch.equal(g, gf(x, ei, bt))
        manual = _compose(model, x, ea, ei, BroadcastRowsFn.apply(g, groups))
    assert pred.dtype == dtype and bool(torch.isfinite(pred.float()).all())
    assert torch.equal(pred, manual)


def test_layer_h64_against_float64():
    """Hidden width 64 (general kernels): the fp32 layer against the float64 path on the same weights and
    inputs, at the golden bars. Receiver 5 and the last node have no edges."""
    from models.trial1 import MeshGraphNetLayer_v2
    d, meta = load("trial1_layer_h128")
    ei = d["edge_index"].to(DEV)
    N, E, W = meta["N"], meta["E"], 64
    torch.manual_seed(3)
    layer = MeshGraphNetLayer_v2(W).to(DEV)
    g = torch.Generator().manual_seed(4)
    t = [torch.randn(r, W, generator=g) for r in (N, E, N, E)]
    res = {}
    for dt in (torch.float32, torch.float64):
        layer = layer.to(dt)
        x, e, gx, ge = (v.to(DEV, dt) for v in t)
        x.requires_grad_(True)
        e.requires_grad_(True)
        layer.zero_grad(set_to_none=True)
        xo, eo = layer(x, ei, e)
        torch.autograd.backward([xo, eo], [gx, ge])
        res[dt] = {"x'": xo.detach(), "e'": eo.detach(), "dx": x.grad, "de": e.grad,
                   **{n: p.grad.clone() for n, p in layer.named_parameters()}}
    lo, hi = res[torch.float32], res[torch.float64]
    assert not bool(hi["x'"][5].eq(t[0][5].to(DEV)).all())  # (the node chain still updates an edgeless node)
    for k in lo:
        r = rel_l2(lo[k].double(), hi[k])
        gate = GPAR if "mlp" in k else FWD
        print(f"v2 layer H=64 fp32 against float64: {k} rel-L2 {r:.3e} (gate {gate:.0e})")
        assert r <= gate, (k, r)


# --------------------------------------------------------------------------- the kernel through the C ABI
class FreeChain:
    """Random parameters of one projection-free edge chain (4 Linears with biases, LayerNorm), packed as
    the model packs them. b0 is bf16-representable, so the sum-trick instantiation fed P = [0 | b0] on
    every node row starts its accumulators from the same fp32 values (0 + b0, exact)."""

    def __init__(self, seed):
        from aerognn.core import Pack
        from aerognn.functions import ChainSpec
        g = torch.Generator(device="cpu").manual_seed(seed)
        s = H ** -0.5
        w = [(torch.randn(H, H, generator=g) * s).to(DEV) for _ in range(4)]
        b = [(torch.randn(H, generator=g) * 0.1).to(DEV) for _ in range(4)]
        b[0] = b[0].to(torch.bfloat16).float()
        self.b0 = b[0]
        self.params = (w, b, (1.0 + 0.1 * torch.randn(H, generator=g)).to(DEV), (0.1 * torch.randn(H, generator=g)).to(DEV))
        self.pack = Pack()
        self.spec = ChainSpec(list(zip(w, b)), (self.params[2], self.params[3]), H, self.pack, "e")
        self.pack.update(torch.bfloat16, torch.device(DEV))


_CHAIN = {}


def _chain():
    if "c" not in _CHAIN:
        _CHAIN["c"] = FreeChain(171)
    return _CHAIN["c"]


def _args(ch, e, out, nblk=None):
    from aerognn import _lib as L
    a = L.EdgeFwdArgs()
    a.rows = e.shape[0]
    a.nblk = int(L.lib().agn_edge_fwd32_blocks(e.shape[0])) if nblk is None else nblk
    wpk, bias = ch.spec.wpk(), ch.spec.biases()
    for i in range(4):
        a.wpk[i] = wpk[i]
        a.bias[i] = bias[i]
    a.ln_g, a.ln_b = ch.spec.lnp()
    a.e, a.out = L.ptr(e), L.ptr(out)
    return a


def _edge_launch(ch, e, dst, rowptr, N, agg, saves, nblk=None, P=None, src=None):
    """agn_edge_forward32 (+ agn_edge_agg_fixup) through the C ABI, so the grid can be chosen.
    agg: None, "sum" or "mean"; P / src: the sum-trick form (None: the projection-free chain)."""
    from aerognn import core, _lib as L
    lib = L.lib()
    E = e.shape[0]
    out = torch.full_like(e, float("nan"))
    a = _args(ch, e, out, nblk)
    a.proj, a.src = L.ptr(P), L.ptr(src)
    if P is not None or agg:
        a.dst = L.ptr(dst)
    a1 = st = ag = None
    if saves:
        a1 = core.tiled_empty(E, H, torch.bfloat16, e.device)
        a1.zero_()
        st = torch.zeros(E, 2, dtype=torch.float32, device=DEV)
        a.act[0], a.stats = L.ptr(a1), L.ptr(st)
    if agg:
        ag = torch.full((N, H), float("nan"), dtype=torch.bfloat16, device=DEV)  # unwritten rows stay NaN
        a.agg, a.rowptr, a.nodes, a.agg_mean = L.ptr(ag), L.ptr(rowptr), N, int(agg == "mean")
    n0 = lib.agn_debug_edge_agg_launches()
    L.check(lib.agn_edge_forward32(C.byref(a), core.stream()), "edge_forward32")
    if agg:
        L.check(lib.agn_edge_agg_fixup(C.byref(a), core.stream()), "edge_agg_fixup")
    torch.cuda.synchronize()
    assert lib.agn_debug_edge_agg_launches() - n0 == int(bool(agg))
    return out, a1, st, ag


def _general(ch, e, saves):
    """agn_mlp_forward on the same operands: one plain segment, bias[0] = b0, resid = e (the resident
    kernel from 65,536 rows on, the general one below)."""
    from aerognn import core, _lib as L
    from aerognn.functions import _alloc_saves
    E = e.shape[0]
    out = torch.full_like(e, float("nan"))
    acts, hpre, stats = _alloc_saves(ch.spec, E, torch.bfloat16, e.device, saves)
    core.mlp_forward(rows=E, dtype=torch.bfloat16, hidden=H, nlin=4, out_dim=H,
                     segs=[(L.SEG_PLAIN, H, e.stride(0), e, None, None)], wpk=ch.spec.wpk(), bias=ch.spec.biases(),
                     ln=ch.spec.lnp(), resid=e, out=out, acts=acts, hpre=hpre, stats=stats)
    torch.cuda.synchronize()
    return out, (acts[0] if saves else None), stats


def _tiled_rows(t, rows):
    from test_gpu_edge_chain import _decode_tiled
    return _decode_tiled(t, rows)


def _check_edge(deg, seed=0, nblk=None):
    """deg: edges per receiver, in receiver order."""
    from aerognn import core
    deg = torch.as_tensor(deg, dtype=torch.int64)
    N, E = deg.numel(), int(deg.sum())
    dst = torch.repeat_interleave(torch.arange(N), deg).to(torch.int32).to(DEV)
    rowptr = torch.zeros(N + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(deg, 0)
    rowptr = rowptr.to(torch.int32).to(DEV)
    g = torch.Generator(device="cpu").manual_seed(seed + 5)
    src = torch.randint(0, N, (E,), generator=g).to(torch.int32).to(DEV)
    e = torch.randn(E, H, generator=g).to(torch.bfloat16).to(DEV)
    ch = _chain()
    P = torch.zeros(N, 2 * H, dtype=torch.bfloat16, device=DEV)
    P[:, H:] = ch.b0.to(torch.bfloat16)
    for saves in (False, True):
        ref, ra1, rst = _general(ch, e, saves)
        assert bool(torch.isfinite(ref.float()).all())
        out, a1, st, _ = _edge_launch(ch, e, dst, rowptr, N, None, saves, nblk)
        old, oa1, ost, _ = _edge_launch(ch, e, dst, rowptr, N, None, saves, nblk, P=P, src=src)
        assert _same(out, ref), (N, E, saves)
        assert _same(out, old), (N, E, saves)
        if saves:
            assert _same(_tiled_rows(a1, E), _tiled_rows(ra1, E)) and torch.equal(st, rst)
            assert _same(a1, oa1) and torch.equal(st, ost)
        for mode in ("mean", "sum"):
            out2, a2, st2, agg = _edge_launch(ch, e, dst, rowptr, N, mode, saves, nblk)
            assert _same(out2, ref), (N, E, saves, mode)
            if saves:
                assert _same(a2, a1) and torch.equal(st2, st)
            want = core.segment_sum(N, H, rowptr, None, out2, torch.full_like(agg, float("nan")), mean=(mode == "mean"))
            torch.cuda.synchronize()
            assert _same(agg, want), (N, E, saves, mode, int((_i16(agg) != _i16(want)).any(1).sum()))
        # the means of the sum-trick form too (the flag is the argument struct's, not the new chain's)
        _, _, _, agg = _edge_launch(ch, e, dst, rowptr, N, "mean", saves, nblk, P=P, src=src)
        want = core.segment_sum(N, H, rowptr, None, old, torch.full_like(agg, float("nan")), mean=True)
        torch.cuda.synchronize()
        assert _same(agg, want), (N, E, saves, "sum-trick mean")


# the shapes of test_gpu_edge_agg.py (grids and runs explained there)
@pytest.mark.parametrize("E", [1, 31, 32, 33])
def test_free_single_tiles(E):
    g = torch.Generator(device="cpu").manual_seed(E)
    d = torch.bincount(torch.randint(0, 5, (E,), generator=g), minlength=5)
    _check_edge(d, seed=E)


def test_free_runs_of_at_most_one_tile():
    _check_edge([6] * 2000)


@pytest.mark.parametrize("nblk", [5, 13])
def test_free_grid_not_a_multiple_of_8(nblk):
    _check_edge([6] * 2000, seed=1, nblk=nblk)


def test_free_one_receiver_holds_all_edges():
    """Receiver 4 spans every run: the fix-up alone forms its mean over 5,000 edges."""
    _check_edge([0, 0, 0, 0, 5000, 0, 0, 0, 0, 0], seed=2)


def test_free_every_receiver_crosses_a_tile():
    _check_edge([40] * 300, seed=3)


def test_free_ragged_with_empty_receivers():
    g = torch.Generator(device="cpu").manual_seed(11)
    d = torch.randint(0, 13, (5000,), generator=g) * (torch.rand(5000, generator=g) >= 0.3)
    if int(d.sum()) % 32 == 0:
        d[0] += 1
    assert int((d == 0).sum()) > 1200
    _check_edge(d, seed=4)


def test_free_full_grid():
    """One block per CU, several tiles per run; agn_mlp_forward runs its resident kernel at this size."""
    _check_edge([6] * 70000, seed=6)


def test_free_arguments_are_checked():
    """Bad arguments return a code without a launch (out stays as it was)."""
    from aerognn import core, _lib as L
    lib = L.lib()
    ch = _chain()
    e = torch.randn(64, H, device=DEV).to(torch.bfloat16)
    out = torch.full_like(e, float("nan"))
    agg = torch.full((4, H), float("nan"), dtype=torch.bfloat16, device=DEV)
    dst = torch.arange(4, dtype=torch.int32, device=DEV).repeat_interleave(16)
    rowptr = (torch.arange(5, dtype=torch.int32, device=DEV) * 16).contiguous()

    def run(fn, **kw):
        a = _args(ch, e, out)
        a.dst, a.agg, a.rowptr, a.nodes = L.ptr(dst), L.ptr(agg), L.ptr(rowptr), 4
        for k, v in kw.items():
            setattr(a, k, v)
        return getattr(lib, fn)(C.byref(a), core.stream())

    fwd, fix = "agn_edge_forward32", "agn_edge_agg_fixup"
    assert run(fwd, agg_mean=2) != 0 and run(fix, agg_mean=2) != 0 and run(fwd, agg_mean=-1) != 0
    assert run(fwd, agg=None, agg_mean=1) != 0    # means need agg
    assert run(fwd, dst=None) != 0                # agg needs the receivers, with or without projections
    assert run(fwd, rowptr=None) != 0
    assert run(fwd, e=None) != 0
    src = torch.zeros(64, dtype=torch.int32, device=DEV)
    P = torch.zeros(4, 2 * H, dtype=torch.bfloat16, device=DEV)
    assert run(fwd, proj=L.ptr(P)) != 0           # the sum-trick form still needs src
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.float()).all()) and bool(torch.isnan(agg.float()).all())
    for kw in (dict(proj=L.ptr(P), src=L.ptr(src), agg_mean=1), dict(agg_mean=1)):
        assert run(fwd, **kw) == 0 and run(fix, **kw) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(agg.float()).all())


# --------------------------------------------------------------------------- the layer, fast path against general
def _graph(N, deg, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    E = N * deg
    # ~10 % of the receivers without edges, the rest ragged
    dst = torch.randint(0, N, (E,), generator=g)
    dst[dst % 10 == 3] += 1
    dst.clamp_(max=N - 1)
    return torch.stack([torch.randint(0, N, (E,), generator=g), dst]), g


def _v2_step(switch, monkeypatch, train=True, N=70000, deg=6, dtype=torch.bfloat16, layer=None):
    from aerognn import _lib as L
    from models.trial1 import MeshGraphNetLayer_v2
    monkeypatch.setenv("AEROGNN_V2_EDGE32", switch)
    lib = L.lib()
    if layer is None:
        torch.manual_seed(0)
        layer = MeshGraphNetLayer_v2(H).to(DEV)
    ei, g = _graph(N, deg, 4)
    E = ei.shape[1]
    ei = ei.to(DEV)
    x = torch.randn(N, H, generator=g).bfloat16().to(DEV, dtype).requires_grad_(train)
    e = torch.randn(E, H, generator=g).bfloat16().to(DEV, dtype).requires_grad_(train)
    n0 = lib.agn_debug_edge_agg_launches()
    if not train:
        with torch.no_grad():
            xo, eo = layer(x, ei, e)
        torch.cuda.synchronize()
        return {"x'": xo, "e'": eo}, lib.agn_debug_edge_agg_launches() - n0
    gx = torch.randn(N, H, generator=g).bfloat16().to(DEV, dtype)
    ge = torch.randn(E, H, generator=g).bfloat16().to(DEV, dtype)
    layer.zero_grad(set_to_none=True)
    xo, eo = layer(x, ei, e)
    torch.autograd.backward([xo, eo], [gx, ge])
    torch.cuda.synchronize()
    res = {"x'": xo.detach(), "e'": eo.detach(), "dx": x.grad, "de": e.grad,
           **{n: p.grad.clone() for n, p in layer.named_parameters()}}
    return res, lib.agn_debug_edge_agg_launches() - n0


@pytest.mark.parametrize("train", [True, False])
def test_layer_with_and_without(train, monkeypatch):
    """MGNv2Fn at N = 70,000 / E = 420,000, bf16 (fp32 master weights): the training step and the
    inference forward, AEROGNN_V2_EDGE32 on against off, and the switch on twice."""
    on, n_on = _v2_step("1", monkeypatch, train=train)
    off, n_off = _v2_step("0", monkeypatch, train=train)
    again, _ = _v2_step("1", monkeypatch, train=train)
    assert (n_on, n_off) == (1, 0)  # the edge kernel formed the means once per layer, or never
    assert on.keys() == off.keys() and len(on) == (4 + 20 if train else 2)
    worst = ("", 0.0)
    for k in on:
        assert on[k] is not None and bool(torch.isfinite(on[k].float()).all()), k
        assert _same(on[k], again[k]), k
        if k in ("x'", "e'", "dx", "de"):
            assert _same(on[k], off[k]), k
        else:
            r = rel_l2(on[k].float(), off[k].double())
            worst = max(worst, (k, r), key=lambda t: t[1])
    if train:
        print(f"v2 layer fast against general: worst parameter-grad rel-L2 {worst[1]:.3e} ({worst[0]}; gate 1e-5)")
        assert worst[1] <= 1e-5, worst


@pytest.mark.parametrize("env", ["AEROGNN_EB_SAVED", "AEROGNN_FUSED_EDGE_BWD"])
def test_training_without_saves_takes_the_general_path(env, monkeypatch):
    monkeypatch.setenv(env, "0")
    _, n = _v2_step("1", monkeypatch, train=True)
    assert n == 0
    _, n = _v2_step("1", monkeypatch, train=False)
    assert n == 1  # inference needs no backward


def test_small_level_takes_the_general_path(monkeypatch):
    _, n = _v2_step("1", monkeypatch, train=False, N=3000)
    assert n == 0


# bf16 against the layer's own fp32 run on the bf16-rounded weights and inputs, rel-L2, at
# N = 70,000 / E = 420,000 (_graph above), measured on the MI355X. Yardstick: the same distance of the
# existing MeshGraphNetLayer(128, 128, 128, 2, 2, 'relu', True, 'mean', do_concat_trick=True), whose
# code this model's addition does not touch; "params" is the worst parameter gradient.
YARDSTICK = {"x'": 2.528e-3, "e'": 2.537e-3, "dx": 4.739e-2, "de": 1.988e-2, "params": 6.977e-2}
MEASURED_V2 = {"x'": 2.602e-3, "e'": 2.469e-3, "dx": 2.476e-2, "de": 2.529e-2, "params": 6.309e-2}  # fast = general path


def bf16_distance(kind, monkeypatch=None):
    """rel-L2 of the bf16 training step from the fp32 step of the same layer on the same bf16-rounded
    weights and inputs. kind: "v2" (MeshGraphNetLayer_v2) or "mgn_mean" (the yardstick)."""
    from models.mgnLayer import MeshGraphNetLayer
    from models.trial1 import MeshGraphNetLayer_v2
    torch.manual_seed(0)
    layer = (MeshGraphNetLayer_v2(H) if kind == "v2" else
             MeshGraphNetLayer(H, H, H, 2, 2, "relu", True, "mean", True)).to(DEV)
    with torch.no_grad():
        for p in layer.parameters():
            p.copy_(p.to(torch.bfloat16).float())
    N, deg = 70000, 6
    ei, g = _graph(N, deg, 4)
    ei = ei.to(DEV)
    E = ei.shape[1]
    t = [torch.randn(r, H, generator=g).bfloat16() for r in (N, E, N, E)]
    res = {}
    for dtype in (torch.bfloat16, torch.float32):
        x, e, gx, ge = (v.to(DEV, dtype) for v in t)
        x.requires_grad_(True)
        e.requires_grad_(True)
        layer.zero_grad(set_to_none=True)
        xo, eo = layer(x, ei, e) if kind == "v2" else layer(x, e, ei)
        torch.autograd.backward([xo, eo], [gx, ge])
        torch.cuda.synchronize()
        res[dtype] = {"x'": xo.detach(), "e'": eo.detach(), "dx": x.grad, "de": e.grad,
                      **{n: p.grad.clone() for n, p in layer.named_parameters()}}
    lo, hi = res[torch.bfloat16], res[torch.float32]
    out = {k: rel_l2(lo[k].float(), hi[k].double()) for k in ("x'", "e'", "dx", "de")}
    out["params"] = max(rel_l2(lo[k].float(), hi[k].double()) for k in lo if k not in out)
    return out


def test_layer_bf16_accuracy():
    """The bf16 layer (fast path: N = 70,000, E = 420,000) against its own fp32 run on the bf16-rounded
    weights and inputs; each distance is gated at 3x the yardstick's (the project's convention for
    bf16 chains). Measured on the MI355X, rel-L2 (yardstick / this layer): x' 2.528e-3 / 2.602e-3,
    e' 2.537e-3 / 2.469e-3, dx 4.739e-2 / 2.476e-2, de 1.988e-2 / 2.529e-2, worst parameter gradient
    6.977e-2 / 6.309e-2 (the gradients carry the ReLU masks that differ between the two precisions).
    The general path (AEROGNN_V2_EDGE32=0) measures the same figures: its x', e', dx, de are bitwise
    the fast path's."""
    got = bf16_distance("v2")
    for k, v in got.items():
        print(f"v2 layer bf16 against fp32: {k} rel-L2 {v:.3e} (measured {MEASURED_V2[k]:.3e}; yardstick "
              f"{YARDSTICK[k]:.3e}, gate 3x)")
    bad = {k: v for k, v in got.items() if not v <= 3.0 * YARDSTICK[k]}
    assert not bad, bad
