"""agn_wgrad_segsum (csrc/dw.hip): dW_e = G0^T e and the receiver sums dP_d of the sum-trick edge
block (mgnLayer.py:97-99 under autograd) in one pass over G0.

Both outputs are bitwise those of the two launches the pass replaces, by construction: dW from the
plain agn_wgrad kernel's splits, stages and MFMA order, dP_d from agn_segment_sum's fp32 adds in
edge order with one rounding. So every comparison is torch.equal, with no tolerance. The cases are
the places where the walk over the staged rows changes path: a receiver across a 64-row stage, across
a split's end (its owner reads on from global memory), longer than a whole split, empty receivers
at every kind of position, splits without rows, and a single row.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
os.environ.setdefault("AEROGNN_MEMLOG", "0")
DEV = "cuda"
H = 128


def _plan(E):
    """(splits, rows per split) of a one-desc 128 x 128 agn_wgrad over E rows."""
    from aerognn import _lib as L
    ns = int(L.lib().agn_wgrad_nsplit(E, 1))
    per = ((E + ns - 1) // ns + 63) // 64 * 64
    return ns, per


def _rand_degs(E, N, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.bincount(torch.randint(0, N, (E,), generator=g), minlength=N).tolist()


def _check(degs, seed=0):
    """out against agn_segment_sum and dw against a plain WGrad run, bitwise; out starts as NaN, so
    a row nobody wrote shows."""
    from aerognn import core
    N, E = len(degs), int(sum(degs))
    rowptr = torch.zeros(N + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.tensor(degs, dtype=torch.int64), 0)
    rowptr = rowptr.to(torch.int32).to(DEV)
    dst = torch.repeat_interleave(torch.arange(N, dtype=torch.int32), torch.tensor(degs, dtype=torch.int64)).to(DEV)
    g = torch.Generator(device="cpu").manual_seed(seed)
    G = torch.randn(E, H, generator=g).to(torch.bfloat16).to(DEV)
    X = torch.randn(E, H, generator=g).to(torch.bfloat16).to(DEV)
    out = torch.full((N, H), float("nan"), dtype=torch.bfloat16, device=DEV)
    dw = torch.full((H, H), float("nan"), dtype=torch.float32, device=DEV)
    core.wgrad_segsum(G, X, dw, rowptr, dst, out)
    ref = core.segment_sum(N, H, rowptr, None, G, torch.empty(N, H, dtype=torch.bfloat16, device=DEV))
    dwr = torch.empty(H, H, dtype=torch.float32, device=DEV)
    wg = core.WGrad()
    wg.add(G, X, dwr)
    wg.run()
    torch.cuda.synchronize()
    assert not torch.isnan(out).any(), "a row of out that no workgroup wrote"
    assert torch.equal(out.view(torch.int16), ref.view(torch.int16))
    assert torch.equal(dw, dwr)
    return out, dw


@pytest.mark.parametrize("E", [1, 63, 64, 65, 128, 1000])
def test_sizes(E):
    if E == 1000:
        ns, per = _plan(E)
        assert ns > 1 and per < E, (ns, per)  # several splits: split ends inside the data
    _check(_rand_degs(E, max(1, E // 6), 1), seed=E)
    _check(_rand_degs(E, 3 * E + 2, 2), seed=E + 1)  # mostly empty receivers


def test_receiver_across_a_stage():
    assert _plan(128)[0] == 1
    _check([60, 10, 58])  # rows 60..69 cross the stage end at 64
    _check([3, 64, 61])   # a receiver of exactly one stage's length, shifted
    _check([64, 64])      # receivers that end exactly at the stage ends


def test_receiver_across_a_split():
    E = 1000
    ns, per = _plan(E)
    assert ns > 1 and 2 * per < E
    # rows per-3..per+3 cross the first split's end; the 70 rows 2per-30..2per+39 cross the second's
    # and, past it, run on into the next stage
    head = [per - 3, 7, per - 4 - 35, 5, 70]
    assert sum(head[:1]) < per < sum(head[:2]) and sum(head[:4]) == 2 * per - 30
    _check(head + _rand_degs(E - sum(head), 40, 3))
    # receivers that end exactly at a split's end
    _check([per, per] + _rand_degs(E - 2 * per, 50, 4))


def test_hub_longer_than_a_split():
    E = 2000
    ns, per = _plan(E)
    assert ns > 1 and per < 300
    _check([5] * 10 + [300] + _rand_degs(E - 350, 200, 5))
    _check([per + 1, 2 * per + 1] + _rand_degs(E - 3 * per - 2, 30, 6))


def test_all_edges_on_one_receiver():
    _check([0, 0, 1000, 0, 0])
    _check([1000])  # N = 1
    _check([1])     # N = 1, E = 1


def test_empty_receivers():
    E = 1000
    ns, per = _plan(E)
    assert ns > 1 and 2 * per < E
    mid = _rand_degs(E - 2 * per - 9, 60, 7)
    # empties at the start, in a row in the middle, exactly at a split's end (rowptr == per, and
    # again at 2 * per after a receiver that ends there), and several at the end (rowptr == E)
    degs = [0, 0, 0, per - 2, 2, 0, 0, 0, per] + [0, 0] + mid[:30] + [0, 0, 0, 0] + mid[30:] + [9, 0, 0, 0, 0, 0]
    _check(degs)
    # every receiver of some wave's share empty: walks that find nothing to add
    _check([0, 5, 0, 0] * 50 + [0] * 7)


def test_splits_without_rows():
    """rows-per-split is rounded up to 64, so the last splits of a plan can hold no rows."""
    from aerognn import _lib as L
    resident = int(L.lib().agn_wgrad_nsplit(1 << 30, 1))
    E = resident * 128 + 1
    ns, per = _plan(E)
    assert ns == resident and (ns - 1) * per >= E, (ns, per, E)
    _check(_rand_degs(E, E // 6, 8) + [0, 0, 0])


def test_no_edges():
    from aerognn import core
    N = 37
    rowptr = torch.zeros(N + 1, dtype=torch.int32, device=DEV)
    G = torch.empty(0, H, dtype=torch.bfloat16, device=DEV)
    out = torch.full((N, H), float("nan"), dtype=torch.bfloat16, device=DEV)
    dw = torch.full((H, H), float("nan"), dtype=torch.float32, device=DEV)
    core.wgrad_segsum(G, G.clone(), dw, rowptr, torch.empty(0, dtype=torch.int32, device=DEV), out)
    torch.cuda.synchronize()
    assert torch.equal(out, torch.zeros_like(out)) and torch.equal(dw, torch.zeros_like(dw))
    _check([0] * N)


def _mesh(nu, nv):
    from aerognn.meshgen import ellipsoid
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in ellipsoid(nu, nv).items()}


def test_mesh_rowptr():
    from aerognn.graph import Level
    m = _mesh(40, 25)
    lv = Level.from_edge_index(m["edge_index"].to(DEV), m["x"].shape[0])
    rp = lv.rowptr.cpu().long()
    _check((rp[1:] - rp[:-1]).tolist(), seed=9)


def test_unsupported_shapes_are_errors():
    from aerognn import core, _lib as L
    rowptr = torch.tensor([0, 64], dtype=torch.int32, device=DEV)
    dst = torch.zeros(64, dtype=torch.int32, device=DEV)
    G = torch.zeros(64, H, dtype=torch.float32, device=DEV)
    out = torch.empty(1, H, dtype=torch.float32, device=DEV)
    dw = torch.empty(H, H, dtype=torch.float32, device=DEV)
    with pytest.raises(L.AeroGNNError):
        core.wgrad_segsum(G, G, dw, rowptr, dst, out)  # 32-bit operands


def _layer_grads(m, switch, monkeypatch):
    from models.mgnLayer import MeshGraphNetLayer
    monkeypatch.setenv("AEROGNN_WG_DPD", switch)
    N, E = m["x"].shape[0], m["edge_index"].shape[1]
    torch.manual_seed(0)
    layer = MeshGraphNetLayer(128, 128, 128, 2, 2, do_concat_trick=True).to(DEV)
    g = torch.Generator(device="cpu").manual_seed(4)
    x = torch.randn(N, H, generator=g).bfloat16().to(DEV).requires_grad_(True)
    e = torch.randn(E, H, generator=g).bfloat16().to(DEV).requires_grad_(True)
    gx = torch.randn(N, H, generator=g).bfloat16().to(DEV)
    ge = torch.randn(E, H, generator=g).bfloat16().to(DEV)
    xo, eo = layer(x, e, m["edge_index"].to(DEV))
    torch.autograd.backward([xo, eo], [gx, ge])
    torch.cuda.synchronize()
    return {"dx": x.grad, "de": e.grad, **{n: p.grad for n, p in layer.named_parameters()}}


# ellipsoid(40, 25): 5,840 edges, the split bf16 backward (the switch must change nothing there);
# ellipsoid(150, 110): 98,400 edges, agn_edge_bwd_fused, where the one pass replaces the two launches
@pytest.mark.parametrize("nu,nv,fused", [(40, 25, False), (150, 110, True)])
def test_layer_gradients_bitwise_with_and_without(nu, nv, fused, monkeypatch):
    from aerognn import core
    m = _mesh(nu, nv)
    assert core.fused_edge_train_ok(m["edge_index"].shape[1], torch.bfloat16, 128, 4, True) == fused
    calls = []
    real = core.wgrad_segsum
    import aerognn.functions as F
    monkeypatch.setattr(F, "wgrad_segsum", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    on = _layer_grads(m, "1", monkeypatch)
    assert len(calls) == (1 if fused else 0)
    off = _layer_grads(m, "0", monkeypatch)
    assert len(calls) == (1 if fused else 0)
    assert on.keys() == off.keys() and len(on) > 10
    for k in on:
        a, b = on[k], off[k]
        assert a is not None and a.dtype == b.dtype, k
        assert torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a,
                           b.view(torch.int16) if b.dtype == torch.bfloat16 else b), k
