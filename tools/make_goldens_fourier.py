"""Golden vectors for FourierMeshGraphNet and MLPNet from the REAL reference (this container only).

Imports tools/make_goldens.py for its stand-ins and helpers (importing it runs no case), then the
reference's models/fouriermgn.py and models/mlpnet.py. Writes tests/golden/<case>.npz:

  fourier_embed_f32 / _f64  the feature map alone: x [257, 6] in +-4 with 0.0, -0.0 and +-4 planted;
                            per d in {2, 3}: emb, a random g for [x | emb], gx from the reference's autograd
  fouriermgn3_f32 / _f64    a 3-layer FourierMeshGraphNet (H = 32) train step with the input gradient
  fourier_enc_h128          the node encoder MLP(34, 128, 128, 2) alone on [x | emb]
  mlpnet_f32                MLPNet(6, 4, 32, 3, 3) with the same weights also run in float64 (pred64)

Run:  python tools/make_goldens_fourier.py
"""
from __future__ import annotations

import os
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

import make_goldens as G  # noqa: E402  (installs the stand-ins, puts the reference first on sys.path)
from make_goldens import MLP, grads, mesh_tensors, save, sd  # noqa: E402
from models.fouriermgn import FourierMeshGraphNet  # noqa: E402
from models.mlpnet import MLPNet  # noqa: E402
import models.fouriermgn as _refcheck  # noqa: E402
assert os.path.abspath(_refcheck.__file__).startswith(G.REF), _refcheck.__file__  # the REFERENCE's module

FREQ_START, FREQ_LEN = -3, 7


def _embedder(d):
    """The reference's fourier_embedding bound to its three attributes (no parameters involved)."""
    m = FourierMeshGraphNet(6, 4, 4, processor_size=1, hidden_dim_processor=8, hidden_dim_node_encoder=8,
                            hidden_dim_edge_encoder=8, hidden_dim_decoder=8, aggregation="add",
                            fourier_features_dim=d, fourier_freq_start=FREQ_START, fourier_freq_length=FREQ_LEN)
    return m.fourier_embedding


def case_embed(dtype, name):
    g = torch.Generator().manual_seed(10)
    x = (torch.rand(257, 6, generator=g, dtype=torch.float64) * 8 - 4).to(dtype)
    x[0, 0], x[0, 1], x[0, 2] = 0.0, -0.0, 4.0
    x[1, 0], x[1, 1], x[1, 2] = -4.0, 4.0, -0.0
    arrs = {"x": x}
    for d in (2, 3):
        emb_fn = _embedder(d)
        xr = x.clone().requires_grad_(True)
        emb = emb_fn(xr)
        out = torch.cat([xr, emb], dim=-1)  # fouriermgn.py:170
        gy = torch.randn(out.shape, generator=g, dtype=torch.float64).to(dtype)
        out.backward(gy)
        arrs.update({f"emb_d{d}": emb, f"g_d{d}": gy, f"gx_d{d}": xr.grad})
    save(name, dict(freq_start=FREQ_START, freq_len=FREQ_LEN, dims=[2, 3], dtype=str(dtype)), **arrs)


def _model_kw():
    kw = dict(G.MODEL_KW, processor_size=3, fourier_features_dim=2, fourier_freq_start=FREQ_START,
              fourier_freq_length=FREQ_LEN)
    kw.pop("do_concat_trick")
    return kw


def case_fouriermgn(dtype, name):
    torch.manual_seed(11)
    t = mesh_tensors(12, 8, dtype=dtype)
    kw = _model_kw()
    m = FourierMeshGraphNet(6, 4, 4, **kw).to(dtype)
    x = t["x"].clone().requires_grad_(True)
    pred = m(x, t["edge_attr"], t["edge_index"])
    loss = torch.nn.MSELoss()(pred, t["y"])
    loss.backward()
    save(name, dict(kwargs=kw, dims=[6, 4, 4], dtype=str(dtype)), x=t["x"], edge_attr=t["edge_attr"],
         edge_index=t["edge_index"], y=t["y"], pred=pred, loss=loss, gx=x.grad, **sd(m), **grads(m))


def case_enc_h128():
    """The node encoder of an H = 128 FourierMeshGraphNet alone: K = 34 in one input segment."""
    torch.manual_seed(12)
    t = mesh_tensors(12, 8)
    enc = MLP(34, 128, 128, num_hidden_layers=2)
    x = t["x"].clone().requires_grad_(True)
    xe = torch.cat([x, _embedder(2)(x)], dim=-1)
    y = enc(xe)
    gy = torch.randn_like(y)
    y.backward(gy)
    save("fourier_enc_h128", dict(input_dim=34, hidden_dim=128, output_dim=128, num_hidden_layers=2,
                                  use_layer_norm=True, fourier_features_dim=2, freq_start=FREQ_START,
                                  freq_len=FREQ_LEN),
         x=t["x"], y=y, gy=gy, gx=x.grad, **sd(enc), **grads(enc))


def case_mlpnet():
    torch.manual_seed(13)
    t = mesh_tensors(12, 8)
    kw = dict(hidden_dim=32, num_hidden_layers_encoder=3, num_hidden_layers_decoder=3)
    m = MLPNet(6, 4, **kw)
    pred = m(t["x"])
    loss = torch.nn.MSELoss()(pred, t["y"])
    loss.backward()
    m64 = MLPNet(6, 4, **kw).double()
    m64.load_state_dict({k: v.double() for k, v in m.state_dict().items()})
    pred64 = m64(t["x"].double())
    save("mlpnet_f32", dict(kwargs=kw, dims=[6, 4]), x=t["x"], y=t["y"], pred=pred, loss=loss, pred64=pred64,
         **sd(m), **grads(m))


if __name__ == "__main__":
    torch.set_num_threads(8)
    case_embed(torch.float32, "fourier_embed_f32")
    case_embed(torch.float64, "fourier_embed_f64")
    case_fouriermgn(torch.float32, "fouriermgn3_f32")
    case_fouriermgn(torch.float64, "fouriermgn3_f64")
    case_enc_h128()
    case_mlpnet()
