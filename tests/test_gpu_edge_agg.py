"""The receiver sums formed inside the edge forward kernel (csrc/edge32_fwd.hip, the AGG
instantiation, with agn_edge_agg_fixup) and the node kernel's plain-agg variant
(csrc/node32_fwd.hip), mgnLayer.py:144-146's scatter_add fused into EdgeBlockSum's launch.

Everything is bitwise: agg against agn_segment_sum of the kernel's own e', the node kernel's variant
against its SUM walk and the general kernel, a layer and a BSMS-4 model step with AEROGNN_EDGE_AGG
1 against 0. bf16 tensors are compared as int16, so the sign of a zero counts.

The edge kernel's grid is tile_blocks(ceil(E / 32), 12) (csrc/host.hpp): 8 blocks up to 96 tiles, the
blocks needed rounded up to a multiple of 8 below one per CU, then every CU. The waves of an XCD
group (blocks g, g + 8, ...) split their eighth of the tiles into contiguous runs (tile32.hpp
RangeWalk); a grid that is no multiple of 8 splits all tiles over all waves."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
os.environ.setdefault("AEROGNN_MEMLOG", "0")
DEV = "cuda"
H = 128


def _i16(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_i16(a), _i16(b))


# --------------------------------------------------------------------------- a. the edge kernel
class EdgeChain:
    def __init__(self, seed):
        from aerognn.core import Pack
        from aerognn.functions import ChainSpec
        g = torch.Generator(device="cpu").manual_seed(seed)
        s = H ** -0.5
        we = (torch.randn(H, H, generator=g) * s).to(DEV)
        w = [(torch.randn(H, H, generator=g) * s).to(DEV) for _ in range(3)]
        b = [(torch.randn(H, generator=g) * 0.1).to(DEV) for _ in range(3)]
        self.params = (we, w, b, (1.0 + 0.1 * torch.randn(H, generator=g)).to(DEV), (0.1 * torch.randn(H, generator=g)).to(DEV))
        self.pack = Pack()
        self.spec = ChainSpec([(we, None)] + list(zip(w, b)), (self.params[3], self.params[4]), H, self.pack, "e")
        self.pack.update(torch.bfloat16, torch.device(DEV))


_CHAIN = {}


def _chain():
    if "c" not in _CHAIN:
        _CHAIN["c"] = EdgeChain(71)
    return _CHAIN["c"]


def _edge_launch(ch, e, P, src, dst, rowptr, N, agg, saves, nblk=None):
    """agn_edge_forward32 (+ agn_edge_agg_fixup) through the C ABI, so the grid can be chosen."""
    import ctypes as C
    from aerognn import core, _lib as L
    lib = L.lib()
    E = e.shape[0]
    a = L.EdgeFwdArgs()
    a.rows = E
    a.nblk = int(lib.agn_edge_fwd32_blocks(E)) if nblk is None else nblk
    wpk, bias = ch.spec.wpk(), ch.spec.biases()
    for i in range(4):
        a.wpk[i] = wpk[i]
        a.bias[i] = bias[i]
    a.ln_g, a.ln_b = ch.spec.lnp()
    out = torch.full_like(e, float("nan"))
    a.e, a.proj, a.src, a.dst, a.out = L.ptr(e), L.ptr(P), L.ptr(src), L.ptr(dst), L.ptr(out)
    a1 = st = ag = None
    if saves:
        a1 = core.tiled_empty(E, H, torch.bfloat16, e.device)
        a1.zero_()
        st = torch.zeros(E, 2, dtype=torch.float32, device=DEV)
        a.act[0], a.stats = L.ptr(a1), L.ptr(st)
    if agg:
        ag = torch.full((N, H), float("nan"), dtype=torch.bfloat16, device=DEV)  # unwritten rows stay NaN
        a.agg, a.rowptr, a.nodes = L.ptr(ag), L.ptr(rowptr), N
    n0 = lib.agn_debug_edge_agg_launches()
    L.check(lib.agn_edge_forward32(C.byref(a), core.stream()), "edge_forward32")
    if agg:
        L.check(lib.agn_edge_agg_fixup(C.byref(a), core.stream()), "edge_agg_fixup")
    torch.cuda.synchronize()
    assert lib.agn_debug_edge_agg_launches() - n0 == int(agg)
    return out, a1, st, ag


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
    P = torch.randn(N, 2 * H, generator=g).to(torch.bfloat16).to(DEV)
    ch = _chain()
    for saves in (False, True):
        ref, ra1, rst, _ = _edge_launch(ch, e, P, src, dst, rowptr, N, False, saves, nblk)
        out, a1, st, agg = _edge_launch(ch, e, P, src, dst, rowptr, N, True, saves, nblk)
        assert bool(torch.isfinite(ref.float()).all())
        assert _same(out, ref)
        if saves:
            assert _same(a1, ra1) and torch.equal(st, rst)
        want = core.segment_sum(N, H, rowptr, None, out, torch.full_like(agg, float("nan")))
        torch.cuda.synchronize()
        assert _same(agg, want), (N, E, saves, int((_i16(agg) != _i16(want)).any(1).sum()))


# 1 or 2 tiles on the 8-block grid: per eighth one tile at most, runs of 0 or 1 tile, most waves idle;
# 31 and 33: a partial last tile
@pytest.mark.parametrize("E", [1, 31, 32, 33])
def test_single_tiles(E):
    g = torch.Generator(device="cpu").manual_seed(E)
    d = torch.bincount(torch.randint(0, 5, (E,), generator=g), minlength=5)
    _check_edge(d, seed=E)


def test_runs_of_at_most_one_tile():
    """375 tiles on 32 blocks: an XCD group's 48 waves split 47 (46 in the last eighth) tiles, so every
    run is one tile or empty, and every tile end is a run end."""
    from aerognn import _lib as L
    assert L.lib().agn_edge_fwd32_blocks(12000) == 32
    _check_edge([6] * 2000)


@pytest.mark.parametrize("nblk", [5, 13])
def test_grid_not_a_multiple_of_8(nblk):
    """The walk's other branch: all 375 tiles split over nblk * 12 waves (6-7 and 2-3 tiles a run)."""
    _check_edge([6] * 2000, seed=1, nblk=nblk)


def test_one_receiver_holds_all_edges():
    """Receivers 0-3 and 5-9 are empty (before the first and after the last edge); receiver 4 spans
    every run of the 16-block grid, so no wave writes it and the fix-up sums it once."""
    _check_edge([0, 0, 0, 0, 5000, 0, 0, 0, 0, 0], seed=2)


def test_every_receiver_crosses_a_tile():
    """40 edges per receiver on 32-edge tiles, runs of one tile: most receivers cross a run end."""
    _check_edge([40] * 300, seed=3)


def test_ragged_with_empty_receivers():
    g = torch.Generator(device="cpu").manual_seed(11)
    d = torch.randint(0, 13, (5000,), generator=g) * (torch.rand(5000, generator=g) >= 0.3)
    if int(d.sum()) % 32 == 0:
        d[0] += 1
    assert int((d == 0).sum()) > 1200
    _check_edge(d, seed=4)


# the full grid (one block per CU), several tiles per run, the open sum carried from tile to tile
@pytest.mark.parametrize("N,deg", [(70000, 6), (12000, 36)])
def test_full_grid(N, deg):
    _check_edge([deg] * N, seed=6)


def test_agg_arguments_are_checked():
    import ctypes as C
    from aerognn import core, _lib as L
    lib = L.lib()
    a = L.EdgeFwdArgs()
    a.rows, a.nblk = 64, 8
    x = torch.zeros(64, H, dtype=torch.bfloat16, device=DEV)
    a.agg, a.nodes = L.ptr(x), 64  # no rowptr
    assert lib.agn_edge_agg_fixup(C.byref(a), core.stream()) != 0
    a.agg = None
    assert lib.agn_edge_agg_fixup(C.byref(a), core.stream()) != 0


# --------------------------------------------------------------------------- b. the node kernel
@pytest.mark.parametrize("N,nlin,saves", [(65537, 4, False), (65537, 3, True), (70000, 4, True), (70000, 3, False)])
def test_node_plain_agg_variant(N, nlin, saves):
    """node32_fwd_kernel's PLAIN variant on agg = segment_sum(e') against its SUM walk fed e' and
    against the general kernel on the same two plain segments: the output and every save."""
    from aerognn import core, _lib as L
    from aerognn.functions import _alloc_saves
    from test_gpu_node32 import NodeChain, _graph
    lib = L.lib()
    ch = NodeChain(81, nlin)
    E = N * 6
    rowptr = _graph(N, E, 82, 0.1)
    g = torch.Generator(device="cpu").manual_seed(83)
    x = torch.randn(N, H, generator=g).to(torch.bfloat16).to(DEV)
    ep = torch.randn(E, H, generator=g).to(torch.bfloat16).to(DEV)
    agg = core.segment_sum(N, H, rowptr, None, ep, torch.empty_like(x))

    def run(seg, resident):
        n0 = lib.agn_debug_node32_launches()
        old = lib.agn_set_option(L.OPT_RESIDENT, int(resident))
        try:
            out = torch.full_like(x, float("nan"))
            acts = hpre = stats = None
            if saves:
                acts, hpre, stats = _alloc_saves(ch.spec, N, torch.bfloat16, x.device, True)
                for t in acts + [hpre, stats]:
                    t.zero_()
                for t in acts:
                    t.agn_mask.zero_()
            core.mlp_forward(rows=N, dtype=torch.bfloat16, hidden=H, nlin=nlin, out_dim=H,
                             segs=[(L.SEG_PLAIN, H, H, x, None, None), seg], wpk=ch.spec.wpk(), bias=ch.spec.biases(),
                             ln=ch.spec.lnp(), resid=x, out=out, acts=acts, hpre=hpre, stats=stats)
            torch.cuda.synchronize()
        finally:
            lib.agn_set_option(L.OPT_RESIDENT, old)
        assert lib.agn_debug_node32_launches() - n0 == int(resident)
        return [out] + ([] if not saves else [t for a in acts for t in (a, a.agn_mask)] + [hpre, stats])

    plain = (L.SEG_PLAIN, H, H, agg, None, None)
    got = run(plain, True)
    walk = run((L.SEG_SUM, H, H, ep, rowptr, None), True)
    general = run(plain, False)
    assert len(got) == (1 + 2 * (nlin - 1) + 2 if saves else 1)
    assert bool(torch.isfinite(got[0].float()).all())
    for a, b, c in zip(got, walk, general):
        assert _same(a, b) and _same(a, c)


# --------------------------------------------------------------------------- c. the layer
def _layer_step(switch, monkeypatch, aggregation="add", trick=True, train=True, N=70000, deg=6):
    from aerognn import _lib as L
    from models.mgnLayer import MeshGraphNetLayer
    monkeypatch.setenv("AEROGNN_EDGE_AGG", switch)
    lib = L.lib()
    torch.manual_seed(0)
    layer = MeshGraphNetLayer(128, 128, 128, 2, 2, "relu", True, aggregation, trick).to(DEV)
    g = torch.Generator(device="cpu").manual_seed(4)
    E = N * deg
    ei = torch.stack([torch.randint(0, N, (E,), generator=g), torch.arange(N).repeat_interleave(deg)]).to(DEV)
    x = torch.randn(N, H, generator=g).bfloat16().to(DEV).requires_grad_(train)
    e = torch.randn(E, H, generator=g).bfloat16().to(DEV).requires_grad_(train)
    n0 = lib.agn_debug_edge_agg_launches()
    if not train:
        with torch.no_grad():
            xo, eo = layer(x, e, ei)
        torch.cuda.synchronize()
        return {"x'": xo, "e'": eo}, lib.agn_debug_edge_agg_launches() - n0
    gx = torch.randn(N, H, generator=g).bfloat16().to(DEV)
    ge = torch.randn(E, H, generator=g).bfloat16().to(DEV)
    xo, eo = layer(x, e, ei)
    torch.autograd.backward([xo, eo], [gx, ge])
    torch.cuda.synchronize()
    res = {"x'": xo.detach(), "e'": eo.detach(), "dx": x.grad, "de": e.grad, **{n: p.grad for n, p in layer.named_parameters()}}
    return res, lib.agn_debug_edge_agg_launches() - n0


@pytest.mark.parametrize("train", [True, False])
def test_layer_with_and_without(train, monkeypatch):
    """GMPFn at N = 70,000 / E = 420,000, bf16 sum-trick: the training step (forward, backward, every
    parameter gradient) and the inference forward, the switch on against off."""
    on, n_on = _layer_step("1", monkeypatch, train=train)
    off, n_off = _layer_step("0", monkeypatch, train=train)
    assert (n_on, n_off) == (1, 0)
    assert on.keys() == off.keys() and len(on) == 2 or len(on) > 14
    for k in on:
        assert on[k] is not None and _same(on[k], off[k]), k


@pytest.mark.parametrize("aggregation,trick", [("mean", True), ("add", False)])
def test_other_blocks_keep_the_walk(aggregation, trick, monkeypatch):
    """Mean aggregation and the concat edge block do not form the sums in the edge kernel."""
    _, n = _layer_step("1", monkeypatch, aggregation=aggregation, trick=trick, train=False)
    assert n == 0


def test_small_level_keeps_the_walk(monkeypatch):
    _, n = _layer_step("1", monkeypatch, train=False, N=3000)
    assert n == 0


# --------------------------------------------------------------------------- d. the model
_MESH = {}


def _model_step(switch, monkeypatch):
    from aerognn import _lib as L
    from aerognn.meshgen import ellipsoid
    from models.bsms_mgn import BiStridedMeshGraphNet
    monkeypatch.setenv("AEROGNN_EDGE_AGG", switch)
    if "m" not in _MESH:
        # 552,960 nodes: the coarsest of the four levels keeps >= 65,536 nodes, so all 15 processor
        # layers run the fused kernels
        _MESH["m"] = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in ellipsoid(1024, 540, seed=0).items()}
    t = _MESH["m"]
    torch.manual_seed(0)
    model = BiStridedMeshGraphNet(6, 4, 4, processor_size=15, num_hidden_layers_node_processor=2,
                                  num_hidden_layers_edge_processor=2, num_hidden_layers_node_encoder=2,
                                  num_hidden_layers_edge_encoder=2, num_hidden_layers_decoder=2,
                                  do_concat_trick=True, num_scales=4, layers_per_scale=2, stride=2).to(DEV)
    n0 = L.lib().agn_debug_edge_agg_launches()
    pred = model(t["x"].bfloat16(), t["edge_attr"].bfloat16(), t["edge_index"], batch=None, pos=t["pos"])
    loss = torch.nn.functional.mse_loss(pred.float(), t["y"])
    loss.backward()
    torch.cuda.synchronize()
    n = L.lib().agn_debug_edge_agg_launches() - n0
    return {"loss": loss.detach(), "pred": pred.detach(), **{k: p.grad for k, p in model.named_parameters()}}, n


def test_model_step_with_without_and_twice(monkeypatch):
    on, n_on = _model_step("1", monkeypatch)
    off, n_off = _model_step("0", monkeypatch)
    again, _ = _model_step("1", monkeypatch)
    assert (n_on, n_off) == (15, 0)
    assert bool(torch.isfinite(on["loss"]))
    for k in on:
        assert on[k] is not None and _same(on[k], off[k]), k
        assert _same(on[k], again[k]), k
