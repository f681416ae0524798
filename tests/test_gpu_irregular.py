"""Pooling, hierarchy and training on irregular graph topologies (tests/irregular_graphs.py).

Every other graph the suite pools is a degree-6 lattice, whose coarse receivers hold a dozen pooling
candidates. The hub, complete, multi and boundary(c) families put more than 256 candidates on a
receiver (the global-load fallback of pool_cand_sort_kernel), between 65 and 256 and exactly 63 /
64 / 65 / 255 / 256 / 257 (the 64-candidate chunks of pool_uniq_kernel / pool_emit_kernel and their
carry), none at all, all 5200 edges of a graph into one coarse edge (stride larger than the graph),
with parallel edges, self loops, one-way edges, isolated nodes, single-node graphs and a gap in the
batch ids. tests/test_irregular_graphs_cpu.py pins on the CPU that they do.

  a. the reference-format maps and pooled values of three successive model._downsample levels,
     bitwise against the oracle's R.downsample(..., stable=True);
  b. the intermediate maps of aerognn.graph.downsample_maps and Level.from_edge_index, each against
     plain torch on the CPU;
  c. PoolNodeFn / PoolEdgeFn / UnpoolFn forward and backward, bitwise against torch autograd on the
     CPU (fp32, float64) and against the rounding order of the kernels' contract (bf16, fp16);
  d. whole-model forward and parameter gradients against the float64 oracle, gated as smoke() is;
  e. the bf16 H = 128 layer under the AEROGNN_EDGE32 / AEROGNN_PROJ_KERNEL switches.
"""
import functools
import os

import pytest
import torch

import irregular_graphs as G

pytestmark = pytest.mark.gpu
os.environ.setdefault("AEROGNN_MEMLOG", "0")
DEV = "cuda"


def _eq(a, b):
    """Bitwise-equal values, NaN == NaN (the rule of _maps_equal in tests/test_gpu_configs.py)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.is_floating_point():
        return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())
    return torch.equal(a, b)


def _maps_equal(got, ref, what):
    cn, ce, cei, cb, cp, f2c = [None if t is None else t.cpu() for t in got]
    assert torch.equal(f2c, ref[5]), (what, "f2c")
    assert torch.equal(cei, ref[2]), (what, "c_edge_index")
    assert torch.equal(cb, ref[3]), (what, "c_batch")
    assert _eq(cn, ref[0]), (what, "pooled nodes")
    assert _eq(ce, ref[1]), (what, "pooled edges")
    if ref[4] is not None:
        assert _eq(cp, ref[4]), (what, "pooled pos")
    else:
        assert cp is None, what


def _ptr(idx, n):
    """CSR pointer [n + 1] of the groups of a group-index vector."""
    p = torch.zeros(n + 1, dtype=torch.long)
    p[1:] = torch.cumsum(torch.bincount(idx, minlength=n), 0)
    return p


def _i(t):
    return t.cpu().long()


@functools.lru_cache(maxsize=None)
def _pool_model(stride):
    from models.bsms_mgn import BiStridedMeshGraphNet
    return BiStridedMeshGraphNet(6, 4, 4, processor_size=1, num_scales=1, hidden_dim_processor=8, stride=stride).to(DEV)


# ------------------------------------------------------------------------------ a. maps, level by level
def _levels_vs_oracle(name, stride, with_pos=True, dtype=torch.float32):
    first, levels = G.oracle_levels(name, stride, 8, with_pos, dtype)
    model = _pool_model(stride)
    got = tuple(None if v is None else v.to(DEV) for v in first)
    fine = first
    for lev, ref in enumerate(levels):
        got = model._downsample(*got[:5])
        torch.cuda.synchronize()
        _maps_equal(got, ref, f"{name} stride {stride} level {lev + 1}")
        cc = G.candidate_counts(ref[5], fine[2], ref[0].shape[0])
        print(f"{name} stride {stride} level {lev + 1}: {ref[0].shape[0]} coarse nodes, {ref[2].shape[1]} coarse "
              f"edges, longest candidate list {int(cc.max())}: bit-exact")
        fine = ref


@pytest.mark.parametrize("name,stride", G.POOL_CASES)
def test_downsample_levels_bitexact(name, stride):
    _levels_vs_oracle(name, stride)


@pytest.mark.parametrize("name,stride", G.POOL_CASES)
def test_downsample_levels_bitexact_nopos(name, stride):
    """pos=None: nodes pool in id order (bsms_mgn.py:244-245), another f2c and other candidate lists."""
    _levels_vs_oracle(name, stride, with_pos=False)


@pytest.mark.parametrize("stride", [2, 1000])
def test_downsample_levels_bitexact_float64(stride):
    _levels_vs_oracle("hub", stride, dtype=torch.float64)


# ------------------------------------------------------------------------------ b. intermediate maps
def _check_level0(lv, ei, n):
    """Level.from_edge_index against torch: the stable receiver grouping of the caller's edges."""
    perm = torch.argsort(ei[1], stable=True)
    assert (lv.N, lv.E) == (n, ei.shape[1])
    assert torch.equal(lv.perm.cpu(), perm) and torch.equal(_i(lv.perm32), perm)
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(perm.numel())
    assert torch.equal(lv.perm_inv.cpu(), inv) and torch.equal(_i(lv.inv32), inv)
    assert torch.equal(_i(lv.src), ei[0][perm]) and torch.equal(_i(lv.dst), ei[1][perm])
    assert torch.equal(_i(lv.rowptr), _ptr(ei[1], n))
    assert torch.equal(lv.refkey.cpu(), perm)
    assert torch.equal(_i(lv.perm_src), torch.argsort(ei[0][perm], stable=True))
    assert torch.equal(_i(lv.rowptr_src), _ptr(ei[0], n))


def _check_pooling(lv, P, f2c, cbatch, what):
    """Every map of one downsample_maps step against torch on the CPU, from the fine level's CSC
    arrays, the expected assignment f2c and coarse batch."""
    src, dst, refkey = _i(lv.src), _i(lv.dst), lv.refkey.cpu()
    E, Nc = src.numel(), cbatch.numel()
    assert P.nc == Nc, what
    assert torch.equal(_i(P.f2c), f2c), (what, "f2c")
    # members of every coarse node: {v : f2c[v] = c} in ascending id
    assert torch.equal(_i(P.c2f), torch.argsort(f2c, stable=True)), (what, "c2f")
    assert torch.equal(_i(P.c2f_ptr), _ptr(f2c, Nc)), (what, "c2f_ptr")
    assert torch.equal(P.cbatch.cpu(), cbatch), (what, "cbatch")
    # coarse edges in CSC order: distinct (f2c[dst], f2c[src]), receiver-major
    uk, inv = torch.unique(f2c[dst] * max(Nc, 1) + f2c[src], return_inverse=True)
    Ec = uk.numel()
    C = P.coarse
    assert (C.N, C.E) == (Nc, Ec), what
    csrc, cdst = uk % max(Nc, 1), uk // max(Nc, 1)
    assert torch.equal(_i(C.src), csrc) and torch.equal(_i(C.dst), cdst), (what, "coarse edges")
    assert torch.equal(_i(P.inv), inv), (what, "inv")
    cmem = _i(P.cmem_ptr)
    assert int(cmem[Ec]) == E and torch.equal(cmem, _ptr(inv, Ec)), (what, "cmem_ptr")
    # the CSC positions of each coarse edge's fine edges, in ascending refkey (refkeys are distinct)
    assert torch.unique(refkey).numel() == E
    o = torch.argsort(refkey, stable=True)
    o = o[torch.argsort(inv[o], stable=True)]
    assert torch.equal(_i(P.cand_sorted), o), (what, "cand_sorted")
    assert torch.equal(C.refkey.cpu(), csrc * Nc + cdst), (what, "coarse refkey")
    assert torch.equal(_i(C.rowptr), _ptr(cdst, Nc)), (what, "coarse rowptr")
    assert torch.equal(_i(C.perm_src), torch.argsort(csrc, stable=True)), (what, "coarse perm_src")
    assert torch.equal(_i(C.rowptr_src), _ptr(csrc, Nc)), (what, "coarse rowptr_src")


@pytest.mark.parametrize("with_pos", [True, False])
@pytest.mark.parametrize("name,stride", G.POOL_CASES)
def test_downsample_maps_against_torch(name, stride, with_pos):
    from aerognn.graph import Level, downsample_maps
    first, levels = G.oracle_levels(name, stride, 8, with_pos)
    node, edge, ei, batch, pos = first
    n, ngraph = node.shape[0], int(batch[-1]) + 1
    lv = Level.from_edge_index(ei.to(DEV), n)
    torch.cuda.synchronize()
    _check_level0(lv, ei, n)
    b, p = batch.to(DEV), None if pos is None else pos.to(DEV)
    for lev, ref in enumerate(levels[:2]):  # level 1 sorts by the caller's order, level 2 by row * Nc + col
        P = downsample_maps(lv, b, p, stride, ngraph)
        torch.cuda.synchronize()
        _check_pooling(lv, P, ref[5], ref[3], f"{name} stride {stride} level {lev + 1}")
        # the oracle's coarse batch and pos (bitwise the kernels': test a) feed the next level
        lv, b, p = P.coarse, ref[3].to(DEV), None if ref[4] is None else ref[4].to(DEV)


# ------------------------------------------------------------------------------ c. autograd of the pooling Functions
AUTOGRAD_CASES = [("hub", 2), ("hub", 1000), ("multi", 3)]


@functools.lru_cache(maxsize=None)
def _pooling(name, stride):
    """(level 0, its Pooling, CPU copies of the maps the Functions read) of a case, built once."""
    from aerognn.graph import Level, downsample_maps
    first, levels = G.oracle_levels(name, stride)
    node, edge, ei, batch, pos = first
    lv = Level.from_edge_index(ei.to(DEV), node.shape[0])
    P = downsample_maps(lv, batch.to(DEV), pos.to(DEV), stride, int(batch[-1]) + 1)
    torch.cuda.synchronize()
    _check_pooling(lv, P, levels[0][5], levels[0][3], f"{name} stride {stride}")
    m = dict(f2c=_i(P.f2c), c2f=_i(P.c2f), c2f_ptr=_i(P.c2f_ptr), inv=_i(P.inv), cand=_i(P.cand_sorted),
             cmem_ptr=_i(P.cmem_ptr), refkey=lv.refkey.cpu(), n=node.shape[0], E=ei.shape[1], nc=P.nc, ec=P.coarse.E)
    return lv, P, m


def _pool_reference(x, g, add, inverse, visit, gptr, order, n_out):
    """(forward, d x) of out = scatter_mean(x, inverse) on the CPU, d x = g[inverse] / count (+ add).
    fp32 / float64: R.scatter_mean over the rows in the reference's visiting order `visit`, and torch
    autograd of it. 16-bit T: the kernels' contract: rows widened to fp32 and summed in order (group r =
    rows order[gptr[r] : gptr[r + 1]]), one division, one rounding; the backward in the rounding order
    of gather_rows_kernel, ((g / count) -> T) + add -> T."""
    from oracle import refcpu as R
    T = x.dtype
    if T in (torch.float32, torch.float64):
        xr = x.clone().requires_grad_(True)
        out = R.scatter_mean(xr[visit], inverse[visit], 0, n_out)
        if add is None:
            out.backward(g)
        else:
            torch.autograd.backward([out, xr.view_as(xr)], [g, add])
        return out.detach(), xr.grad
    cnt = (gptr[1:] - gptr[:-1]).clamp(min=1).float()[:, None]
    out = (G.seq_group_sum(x.float(), gptr, order) / cnt).to(T)
    dx = (g.float() / cnt)[inverse].to(T)
    if add is not None:
        dx = (dx.float() + add.float()).to(T)
    return out, dx


def _unpool_reference(coarse, skip, g, f2c, c2f_ptr, c2f):
    """(forward, d coarse) of coarse[f2c] + skip on the CPU (d skip = g): torch autograd in fp32 /
    float64; 16-bit: one rounded add, and the members' gradients summed in fp32 in ascending id.
    d coarse is a sum over a coarse node's members (all 600 nodes at stride 1000). torch's CPU backward
    of an index splits a long one over threads in an order of its own unless it is asked to be
    deterministic; then it adds the rows in ascending id, which is the kernels' contract."""
    T = coarse.dtype
    if T in (torch.float32, torch.float64):
        c, s = coarse.clone().requires_grad_(True), skip.clone().requires_grad_(True)
        out = c[f2c] + s
        was = torch.are_deterministic_algorithms_enabled()
        torch.use_deterministic_algorithms(True)
        try:
            out.backward(g)
        finally:
            torch.use_deterministic_algorithms(was)
        assert torch.equal(s.grad, g)
        assert torch.equal(c.grad, G.seq_group_sum(g, c2f_ptr, c2f))  # the reference's own order, pinned
        return out.detach(), c.grad
    return (coarse[f2c].float() + skip.float()).to(T), G.seq_group_sum(g.float(), c2f_ptr, c2f).to(T)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16, torch.float16],
                         ids=["fp32", "fp64", "bf16", "fp16"])
@pytest.mark.parametrize("width", [5, 128])
@pytest.mark.parametrize("name,stride", AUTOGRAD_CASES)
def test_pooling_functions_autograd(name, stride, width, dtype):
    from aerognn.functions import GradBox, PoolEdgeFn, PoolNodeFn, UnpoolFn
    lv, P, m = _pooling(name, stride)
    g = torch.Generator().manual_seed(1000 * width + stride)

    def draw(rows):
        return torch.randn(rows, width, generator=g).to(dtype)

    def run_pool(Fn, x, gout, add):
        xg = x.to(DEV).requires_grad_(True)
        box = None
        if add is not None:  # the up path's gradient of the skip tensor, parked before the pooling backward
            box = GradBox()
            box.put(add.to(DEV))
        y = Fn.apply(xg, P, box)
        y.backward(gout.to(DEV))
        torch.cuda.synchronize()
        assert box is None or box.g is None  # taken
        return y.detach().cpu(), xg.grad.cpu()

    what = f"{name} stride {stride} width {width} {dtype}"
    # nodes: groups c2f[c2f_ptr[c] : c2f_ptr[c + 1]], visited in id order
    x, gn, addn = draw(m["n"]), draw(m["nc"]), draw(m["n"])
    # edges (rows in the level's CSC order): groups cand[cmem_ptr[k] : cmem_ptr[k + 1]], visited in refkey order
    e, ge, adde = draw(m["E"]), draw(m["ec"]), draw(m["E"])
    for add_n, add_e in ((None, None), (addn, adde)):
        tag = (what, "plain" if add_n is None else "GradBox")
        want = _pool_reference(x, gn, add_n, m["f2c"], torch.arange(m["n"]), m["c2f_ptr"], m["c2f"], m["nc"])
        got = run_pool(PoolNodeFn, x, gn, add_n)
        assert _eq(got[0], want[0]), (tag, "PoolNodeFn forward")
        assert _eq(got[1], want[1]), (tag, "PoolNodeFn backward")
        want = _pool_reference(e, ge, add_e, m["inv"], torch.argsort(m["refkey"], stable=True), m["cmem_ptr"],
                               m["cand"], m["ec"])
        got = run_pool(PoolEdgeFn, e, ge, add_e)
        assert _eq(got[0], want[0]), (tag, "PoolEdgeFn forward")
        assert _eq(got[1], want[1]), (tag, "PoolEdgeFn backward")
    coarse, skip, gu = draw(m["nc"]), draw(m["n"]), draw(m["n"])
    want = _unpool_reference(coarse, skip, gu, m["f2c"], m["c2f_ptr"], m["c2f"])
    for boxed in (False, True):
        c, s = coarse.to(DEV).requires_grad_(True), skip.to(DEV).requires_grad_(True)
        box = GradBox() if boxed else None
        out = UnpoolFn.apply(c, s, P, box)
        out.backward(gu.to(DEV))
        torch.cuda.synchronize()
        assert _eq(out.detach().cpu(), want[0]), (what, boxed, "UnpoolFn forward")
        assert _eq(c.grad.cpu(), want[1]), (what, boxed, "UnpoolFn backward, coarse")
        if boxed:  # the skip's gradient goes to the box, not to autograd
            assert s.grad is None and box.armed and _eq(box.take().cpu(), gu), (what, "UnpoolFn GradBox")
        else:
            assert _eq(s.grad.cpu(), gu), (what, "UnpoolFn backward, skip")


# ------------------------------------------------------------------------------ d. a model against the float64 oracle
def _model_kw(stride, scales, aggregation, trick, H=32):
    return dict(processor_size=7, num_hidden_layers_node_processor=2, num_hidden_layers_edge_processor=2,
                num_hidden_layers_node_encoder=2, num_hidden_layers_edge_encoder=2, num_hidden_layers_decoder=2,
                hidden_dim_processor=H, hidden_dim_node_encoder=H, hidden_dim_edge_encoder=H, hidden_dim_decoder=H,
                aggregation=aggregation, do_concat_trick=trick, num_scales=scales, layers_per_scale=1, stride=stride)


def conditioned_model(name, stride, scales, aggregation, trick, seed=2):
    """The model of a case on the CPU, its biases conditioned off ReLU kinks as smoke() does
    (tests/kinkfree.py, repeated until a pass shifts nothing after the fp32 round-trip), with its
    inputs: (model, tensors, oracle cfg, bias columns shifted). seed draws the weights: at some seeds a
    deep edge column lies so close to 0 over thousands of rows that no bias shift of kinkfree's range
    clears it and the conditioning gives up (an AssertionError, never a silent pass); at 2 it
    converges on every case below."""
    from kinkfree import kink_free_biases
    from models.bsms_mgn import BiStridedMeshGraphNet
    from oracle import refcpu as R
    n, ei, batch = G.family(name)
    pos, _, _ = G.features(n, ei.shape[1], 1, seed=21)
    g = torch.Generator().manual_seed(22)
    t = dict(x=torch.randn(n, 6, generator=g), edge_attr=R.compute_edge_attr(pos, ei), edge_index=ei, batch=batch,
             pos=pos, y=torch.randn(n, 4, generator=g))
    kw = _model_kw(stride, scales, aggregation, trick)
    cfg = R.cfg_from_kwargs(**kw)
    torch.manual_seed(seed)
    model = BiStridedMeshGraphNet(6, 4, 4, **kw)
    shifted = 0
    for _ in range(4):
        p64 = {k: v.detach().double().clone() for k, v in model.state_dict().items()}
        k = kink_free_biases(lambda: R.bsms_forward(p64, t["x"].double(), t["edge_attr"].double(), ei, cfg, batch,
                                                    pos.double(), stable=True), p64)
        if k == 0:
            break
        shifted += k
        model.load_state_dict({k_: v.float() for k_, v in p64.items()})
    else:
        raise AssertionError("conditioned biases not kink-free after the fp32 round-trip")
    return model, t, cfg, shifted


MODEL_CASES = [("hub", 2, 3, "add", True), ("hub", 3, 3, "mean", True), ("complete", 8, 2, "add", True),
               ("multi", 3, 3, "add", True), ("hub", 2, 3, "add", False)]


@pytest.mark.parametrize("name,stride,scales,aggregation,trick", MODEL_CASES)
def test_model_gradients_vs_float64_oracle(name, stride, scales, aggregation, trick):
    """Forward against the fp32 oracle at 1e-5; every parameter gradient of the MSE loss against the
    float64 oracle, worst and median within 10x of the CPU fp32 oracle's own error measured here
    (floor 1e-6): the rule of smoke()."""
    from __graft_entry__ import _grad_errors
    model, t, cfg, shifted = conditioned_model(name, stride, scales, aggregation, trick)
    model = model.to(DEV)
    rel, ours, cpu, loss = _grad_errors(model, t, cfg, torch.device(DEV))
    print(f"{name} stride {stride} {scales} scales {aggregation} trick={trick}: {shifted} bias columns shifted; fwd "
          f"rel-L2 {rel:.2e}; param-grad rel-L2 vs fp64: ours median {float(ours.median()):.3e} max "
          f"{float(ours.max()):.3e}; cpu fp32 median {float(cpu.median()):.3e} max {float(cpu.max()):.3e}; loss "
          f"{loss:.6f}")
    assert rel <= 1e-5, rel
    assert float(ours.max()) <= max(10 * float(cpu.max()), 1e-6), (float(ours.max()), float(cpu.max()))
    assert float(ours.median()) <= max(10 * float(cpu.median()), 1e-6), (float(ours.median()), float(cpu.median()))


# ------------------------------------------------------------------------------ e. bf16 H = 128 kernel selection
def _layer_step(layer, x, e, lv):
    xg = x.clone().requires_grad_(True)
    eg = e.clone().requires_grad_(True)
    layer.zero_grad()
    xo, eo = layer.forward_level(xg, eg, lv)
    (xo.float().square().sum() + 0.5 * eo.float().square().sum()).backward()
    torch.cuda.synchronize()
    return xo.detach(), eo.detach(), xg.grad, eg.grad, {n: p.grad.clone() for n, p in layer.named_parameters()}


def test_bf16_layer_switches_bitwise_on_hub(monkeypatch):
    """One bf16 H = 128 sum-trick layer on the hub graph (600 nodes, 5200 edges: below the 65,536 rows
    of the fused backward and the in-kernel aggregation). AEROGNN_PROJ_KERNEL selects agn_proj_forward /
    agn_proj_backward or the general kernel; AEROGNN_EDGE32 the 32-row-tile edge forward or the
    resident general kernel, which GMPFn takes in inference and in the fused training step only, so
    on a level this small the switch moves the inference forward and leaves the training step alone.
    Every output and gradient is bitwise equal across the switches, and every switch is seen to move
    the launches it is documented to move (core.PROF tags, and calls counted at the Functions' own
    call sites: both edge paths carry the tag edge_fwd and both projection forwards the tag proj)."""
    from aerognn import core, functions
    from aerognn.graph import Level
    from models.mgnLayer import MeshGraphNetLayer
    n, ei, _ = G.hub()
    assert ei.shape[1] < 65536
    torch.manual_seed(0)
    layer = MeshGraphNetLayer(128, 128, 128, 2, 2, do_concat_trick=True).to(DEV)
    lv = Level.from_edge_index(ei.to(DEV), n)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(n, 128, generator=g).to(DEV, torch.bfloat16)
    e = torch.randn(ei.shape[1], 128, generator=g).to(DEV, torch.bfloat16)
    calls = {}
    for fn in ("edge_forward", "proj_forward", "proj_backward"):
        def counted(*a, _f=getattr(functions, fn), _n=fn, **k):
            calls[_n] = calls.get(_n, 0) + 1
            return _f(*a, **k)
        monkeypatch.setattr(functions, fn, counted)

    def run(edge32, proj):
        monkeypatch.setenv("AEROGNN_EDGE32", edge32)
        monkeypatch.setenv("AEROGNN_PROJ_KERNEL", proj)
        calls.clear()
        core.PROF = []
        try:
            step = _layer_step(layer, x, e, lv)
            train_calls = dict(calls)
            calls.clear()
            with torch.no_grad():
                xo, eo = layer.forward_level(x, e, lv)
            torch.cuda.synchronize()
            tags = [t for t, *_ in core.PROF]
        finally:
            core.PROF = None
        return step, (xo, eo), train_calls, dict(calls), tags

    base = run("1", "1")
    runs = {"EDGE32=0": run("0", "1"), "PROJ_KERNEL=0": run("1", "0")}
    # the paths taken
    assert base[2] == {"proj_forward": 1, "proj_backward": 1}, base[2]  # training: no 32-row-tile edge forward
    assert base[3] == {"proj_forward": 1, "edge_forward": 1}, base[3]  # inference: both fast kernels
    assert "proj" in base[4] and "proj_bwd" in base[4] and "edge_fwd" in base[4] and "edge_bwd" in base[4]
    r = runs["EDGE32=0"]
    assert r[2] == base[2] and r[3] == {"proj_forward": 1}, (r[2], r[3])
    assert "proj_bwd" in r[4]
    r = runs["PROJ_KERNEL=0"]
    assert r[2] == {} and r[3] == {"edge_forward": 1}, (r[2], r[3])
    assert "proj_bwd" not in r[4] and "proj" in r[4]  # the general kernel runs the backward product untagged
    # the values
    for what, r in runs.items():
        for nm, a, b in zip(("x'", "e'", "dx", "de"), base[0][:4], r[0][:4]):
            assert torch.equal(a, b), (what, "train", nm)
        for nm in base[0][4]:
            assert torch.equal(base[0][4][nm], r[0][4][nm]), (what, "train", nm)
        for nm, a, b in zip(("x'", "e'"), base[1], r[1]):
            assert torch.equal(a, b), (what, "inference", nm)
