"""Golden vectors for MeshGraphNet_v2 (models/trial1.py) from the REAL reference (this container only).

Imports tools/make_goldens.py for its stand-ins and helpers (importing it runs no case), extends the
stand-ins at run time with the names models/trial1.py imports and never calls (four empty classes on
torch_geometric.nn, torch_scatter.scatter), then imports the reference's module. Writes
tests/golden/<case>.npz:

  trial1_f32 / _f64     MeshGraphNet_v2(6, 4, 32, 4, 3, num_encoder_layers=3, num_decoder_layers=2) on the
                        two-graph batch ellipsoid(12, 8) + ellipsoid(10, 7) (166 nodes / 908 edges): a train
                        step (pred, loss, input gradient, parameters, their gradients) and the forward with
                        batch=None on the same tensors (pred_nobatch)
  trial1_layer_h128     one MeshGraphNetLayer_v2(128) on the ellipsoid(12, 8) mesh with its edges shuffled,
  trial1_layer_h128_g   the edges into node 5 removed and one node without edges appended (receivers without
                        edges in the middle and at the end): x', e', the input gradients for random output
                        gradients, the parameter gradients. Two files, each below 1 MiB: the first holds
                        the parameters, x, edge_index and e', the second the gradients and x'. The edge
                        input e and the output gradient of e' are torch.randn draws of
                        torch.Generator().manual_seed(LAYER_SEED) in that order (layer_draws below, which
                        the test calls too) instead of stored tensors.
  trial1_dec1           MeshGraphNet_v2(6, 4, 32, 4, 2, num_encoder_layers=2, num_decoder_layers=1), forward

Run:  python tools/make_goldens_trial1.py
"""
from __future__ import annotations

import os
import sys
import types

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

import make_goldens as G  # noqa: E402  (installs the stand-ins, puts the reference first on sys.path)
from make_goldens import batch_tensors, grads, mesh_tensors, save, sd  # noqa: E402

_tgn, _ts = sys.modules["torch_geometric.nn"], sys.modules["torch_scatter"]
for _n in ("MessagePassing", "GCNConv", "GINEConv", "GraphSAGE"):  # imported by the module, never used
    if not hasattr(_tgn, _n):
        setattr(_tgn, _n, type(_n, (), {}))
if not hasattr(_ts, "scatter"):
    _ts.scatter = types.SimpleNamespace()  # a name only

from models.trial1 import MeshGraphNet_v2, MeshGraphNetLayer_v2  # noqa: E402
import models.trial1 as _refcheck  # noqa: E402
assert os.path.abspath(_refcheck.__file__).startswith(G.REF), _refcheck.__file__  # the REFERENCE's module

MODEL_SEED, LAYER_SEED, DEC1_SEED = 21, 22, 23
MODEL_ARGS = (6, 4, 32, 4, 3, 3, 2)
DEC1_ARGS = (6, 4, 32, 4, 2, 2, 1)


def layer_draws(E, H, dtype=torch.float32):
    """(e, ge_out) of the layer case."""
    g = torch.Generator().manual_seed(LAYER_SEED)
    return torch.randn(E, H, generator=g, dtype=dtype), torch.randn(E, H, generator=g, dtype=dtype)


def case_model(dtype, name):
    torch.manual_seed(MODEL_SEED)
    m = MeshGraphNet_v2(*MODEL_ARGS).to(dtype)
    t = batch_tensors([(12, 8, 0), (10, 7, 1)], dtype=dtype)
    x = t["x"].clone().requires_grad_(True)
    pred = m(x, t["edge_attr"], t["edge_index"], t["batch"])
    loss = torch.nn.MSELoss()(pred, t["y"])
    loss.backward()
    with torch.no_grad():
        pred_nobatch = m(t["x"], t["edge_attr"], t["edge_index"], None)
    save(name, dict(args=list(MODEL_ARGS), seed=MODEL_SEED, dtype=str(dtype)), x=t["x"], edge_attr=t["edge_attr"],
         edge_index=t["edge_index"], batch=t["batch"], y=t["y"], pred=pred, loss=loss, gx=x.grad,
         pred_nobatch=pred_nobatch, **sd(m), **grads(m))


def case_layer():
    H = 128
    torch.manual_seed(LAYER_SEED)
    layer = MeshGraphNetLayer_v2(H)
    t = mesh_tensors(12, 8, shuffle=True)
    ei = t["edge_index"]
    ei = ei[:, ei[1] != 5].contiguous()      # receiver 5 keeps no edge
    N, E = t["x"].shape[0] + 1, ei.shape[1]  # and the last node has none at all
    g = torch.Generator().manual_seed(LAYER_SEED + 100)
    x = torch.randn(N, H, generator=g).requires_grad_(True)
    gx_out = torch.randn(N, H, generator=g)
    e, ge_out = layer_draws(E, H)
    e.requires_grad_(True)
    xo, eo = layer(x, ei, e)
    torch.autograd.backward([xo, eo], [gx_out, ge_out])
    deg = torch.bincount(ei[1], minlength=N)
    assert int(deg[5]) == 0 and int(deg[N - 1]) == 0
    meta = dict(H=H, seed=LAYER_SEED, N=N, E=E)
    save("trial1_layer_h128", meta, x=x, edge_index=ei, e_out=eo, **sd(layer))
    save("trial1_layer_h128_g", meta, x_out=xo, gx_out=gx_out, gx=x.grad, ge=e.grad, **grads(layer))


def case_dec1():
    torch.manual_seed(DEC1_SEED)
    m = MeshGraphNet_v2(*DEC1_ARGS)
    t = mesh_tensors(10, 7, seed=1)
    with torch.no_grad():
        pred = m(t["x"], t["edge_attr"], t["edge_index"], None)
    save("trial1_dec1", dict(args=list(DEC1_ARGS), seed=DEC1_SEED), x=t["x"], edge_attr=t["edge_attr"],
         edge_index=t["edge_index"], pred=pred, **sd(m))


if __name__ == "__main__":
    torch.set_num_threads(8)
    case_model(torch.float32, "trial1_f32")
    case_model(torch.float64, "trial1_f64")
    case_layer()
    case_dec1()
