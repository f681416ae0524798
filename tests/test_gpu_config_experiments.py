"""Every experiment of the reference's config.yaml, built as train.py:60-200 builds it, takes one
train step on the device (forward, MSE, backward, Adam) on a tiny two-graph batch with the dataset's
feature counts. tests/golden/config_experiments.json (tools/make_goldens_wide.py) holds, per
experiment, the model name, the model kwargs after the override rule of utils.py:132-169 and
(d_n, d_e, d_out). `ahmedBody_pooling_mgn` (poolMGN, hidden_dim 32 with global_dim 128: a 142-wide
node encoder input at H = 32) is also compared with the reference's golden poolmgn_ahmed_h32.

The `missile3d1` entry names the dataset `missile_3d_1`; config.yaml's block is `missile_3d1` (a typo
in the reference, recorded in the entry's `note`), and the entry is built from that block.
"""
import json
import os

import pytest
import torch

from golden_util import GOLDEN, load, max_rel, params, rel_l2

pytestmark = pytest.mark.gpu
os.environ.setdefault("AEROGNN_MEMLOG", "0")

DEV = "cuda"
FWD, GIN, GPAR, F64TOL = 1e-5, 1e-5, 5e-5, 1e-10
with open(os.path.join(GOLDEN, "config_experiments.json")) as _f:
    CFG = json.load(_f)


def build(model_name, c, dims):
    """train.py:60-200: the model of `model_name` from the merged model block `c`."""
    d_n, d_e, d_out = dims
    g = c.get
    if model_name in ("MLP", "mlpnet"):
        from models.mlpnet import MLPNet
        return MLPNet(input_node_dim=d_n, output_node_dim=d_out, hidden_dim=g("hidden_dim"),
                      num_hidden_layers_encoder=g("num_hidden_layers_encoder"),
                      num_hidden_layers_decoder=g("num_hidden_layers_decoder"), activation_fn=g("activation"),
                      dropout=g("dropout"))
    mgn = dict(input_node_dim=d_n, input_edge_dim=d_e, output_node_dim=d_out, processor_size=g("processor_size"),
               activation_fn=g("activation_fn"), num_hidden_layers_node_processor=g("num_hidden_layers_node_processor"),
               num_hidden_layers_edge_processor=g("num_hidden_layers_edge_processor"),
               hidden_dim_processor=g("hidden_dim"), num_hidden_layers_node_encoder=g("num_hidden_layers_node_encoder"),
               hidden_dim_node_encoder=g("hidden_dim"), num_hidden_layers_edge_encoder=g("num_hidden_layers_edge_encoder"),
               hidden_dim_edge_encoder=g("hidden_dim"), aggregation=g("aggregation"), hidden_dim_decoder=g("hidden_dim"),
               num_hidden_layers_decoder=g("num_hidden_layers_decoder"))
    if model_name == "meshgraphnet":
        from models.mgn import MeshGraphNet
        return MeshGraphNet(**mgn, do_concat_trick=g("do_concat_trick"))
    if model_name in ("bsms_mgn", "bsms", "bsms-mgn"):
        from models.bsms_mgn import BiStridedMeshGraphNet
        return BiStridedMeshGraphNet(**mgn, dropout=g("dropout"), do_concat_trick=g("do_concat_trick", False),
                                     num_scales=g("num_scales", 3), layers_per_scale=g("layers_per_scale", 2),
                                     stride=g("stride", 2))
    if model_name == "poolMGN":
        from models.poolmgn import poolMGN
        return poolMGN(**mgn, global_pool_method=g("global_pool_method"),
                       num_hidden_layers_global_encoder=g("num_hidden_layers_global_encoder"),
                       global_dim=g("global_dim"), dropout=g("dropout"))
    if model_name == "fouriermgn":
        from models.fouriermgn import FourierMeshGraphNet
        return FourierMeshGraphNet(**mgn, dropout=g("dropout"), fourier_features_dim=g("fourier_features_dim"),
                                   fourier_freq_start=g("fourier_freq_start"),
                                   fourier_freq_length=g("fourier_freq_length"))
    if model_name in ("trial1", "Trial1"):
        from models.trial1 import MeshGraphNet_v2
        return MeshGraphNet_v2(node_input_size=d_n, edge_input_size=d_e, hidden_channels=g("hidden_dim"),
                               out_channels=d_out, num_graph_conv_layers=g("num_message_passing_layers"),
                               num_encoder_layers=g("number_of_encoding_layers"),
                               num_decoder_layers=g("number_of_decoding_layers"), dropout=g("dropout"))
    raise ValueError(model_name)


def run_model(model, t):
    """utils.py:171-190: the forward call of each model class."""
    cls = model.__class__.__name__
    if cls in ("poolMGN", "MeshGraphNet_v2"):
        return model(t["x"], t["edge_attr"], t["edge_index"], t["batch"])
    if cls == "BiStridedMeshGraphNet":
        return model(t["x"], t["edge_attr"], t["edge_index"], batch=t["batch"], pos=t["pos"])
    if cls == "MLPNet":
        return model(t["x"])
    return model(t["x"], t["edge_attr"], t["edge_index"])


def tiny_batch(dims, dtype=torch.float32):
    """Two small meshes with the dataset's feature layout (dataset.py:39-106): x = [pos, normals,
    per-graph constants for the var_keys], edge_attr = [pos[dst] - pos[src], its length]; a 2-D
    dataset takes the meshes' first two coordinates."""
    from aerognn.meshgen import collate, ellipsoid
    d_n, d_e, d_out = dims
    pd = d_e - 1
    b = collate([ellipsoid(8, 5, seed=0), ellipsoid(7, 6, seed=1)])
    gen = torch.Generator().manual_seed(17)
    pos = torch.from_numpy(b["pos"])[:, :pd]
    nrm = torch.from_numpy(b["x"])[:, 3:3 + pd]
    nrm = nrm / nrm.norm(dim=1, keepdim=True).clamp_min(1e-6)
    ei = torch.from_numpy(b["edge_index"])
    batch = torch.from_numpy(b["batch"])
    var = torch.randn(2, d_n - 2 * pd, generator=gen)
    vec = pos[ei[1]] - pos[ei[0]]
    t = dict(x=torch.cat([pos, nrm, var[batch]], 1), edge_attr=torch.cat([vec, vec.norm(dim=1, keepdim=True)], 1),
             y=torch.randn(pos.shape[0], d_out, generator=gen), pos=pos)
    assert t["x"].shape[1] == d_n and t["edge_attr"].shape[1] == d_e
    t = {k: v.to(dtype).contiguous().to(DEV) for k, v in t.items()}
    t["edge_index"], t["batch"] = ei.to(DEV), batch.to(DEV)
    return t


def train_step(model, t, step=True):
    model.train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=0.0)  # config.yaml training.default
    opt.zero_grad(set_to_none=True)
    loss = torch.nn.MSELoss()(run_model(model, t), t["y"])
    loss.backward()
    assert torch.isfinite(loss), float(loss.detach())
    for name, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    if not step:
        return float(loss.detach())
    opt.step()
    for name, p in model.named_parameters():
        assert bool(torch.isfinite(p).all()), name
    return float(loss.detach())


def test_config_covers_every_experiment():
    assert sorted(CFG) == ["ahmedBody_fourier_mgn", "ahmedBody_mgn", "ahmedBody_mgn_trial", "ahmedBody_pooling_mgn",
                           "airfoil_fourier_mgn", "airfoil_mgn", "airfoil_mlp", "airfoil_pooling_mgn", "missile3d1"]
    assert CFG["ahmedBody_pooling_mgn"]["dims"] == [14, 4, 4] and CFG["airfoil_mgn"]["dims"] == [6, 3, 4]
    assert CFG["missile3d1"]["dataset"] == "missile_3d1" and "missile_3d_1" in CFG["missile3d1"]["note"]
    assert CFG["missile3d1"]["dims"] == [9, 4, 5]
    a = CFG["ahmedBody_pooling_mgn"]["kwargs"]
    assert a["hidden_dim"] == 32 and a["global_dim"] == 128 and a["processor_size"] == 15


@pytest.mark.parametrize("name", sorted(CFG))
def test_experiment_train_step(name):
    e = CFG[name]
    torch.manual_seed(0)
    model = build(e["model"], e["kwargs"], e["dims"]).to(DEV)
    loss = train_step(model, tiny_batch(e["dims"]))
    print(f"{name}: {e['model']} dims {e['dims']} loss {loss:.4f}")


def _ahmed_model(meta):
    """ahmedBody_pooling_mgn as train.py builds it, processor_size cut to the golden's 3."""
    e = CFG["ahmedBody_pooling_mgn"]
    c = dict(e["kwargs"], processor_size=meta["kwargs"]["processor_size"])
    assert meta["dims"] == e["dims"]
    model = build(e["model"], c, e["dims"])
    for k, v in meta["kwargs"].items():  # the golden was generated with the same constructor arguments
        got = c.get("hidden_dim") if k.startswith("hidden_dim_") else c.get(k)
        assert got == v, (k, got, v)
    return model


def _gate(what, got, ref, tol):
    r, mx = rel_l2(got.detach().cpu(), ref), max_rel(got.detach().cpu(), ref)
    print(f"{what}: rel-L2 {r:.2e}, max-elem {mx:.2e} (gate {tol:.0e})")
    assert r <= tol and mx <= tol, (what, r, mx)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_ahmed_pooling_golden(prec):
    d, meta = load("poolmgn_ahmed_h32")
    ref = d if prec == "f32" else load("poolmgn_ahmed_h32_f64")[0]
    dt = torch.float32 if prec == "f32" else torch.float64
    fwd, gin, gpar = (FWD, GIN, GPAR) if prec == "f32" else (F64TOL,) * 3
    model = _ahmed_model(meta)
    model.load_state_dict(params(d))
    model = model.to(dt).to(DEV)
    assert model.node_encoder.layers[0].in_features == 142 and model.node_encoder.hidden_dim == 32
    x = d["x"].to(dt).to(DEV).requires_grad_(True)
    pred = model(x, d["edge_attr"].to(dt).to(DEV), d["edge_index"].to(DEV), d["batch"].to(DEV))
    loss = torch.nn.MSELoss()(pred, d["y"].to(dt).to(DEV))
    loss.backward()
    _gate("pred", pred, ref["pred"], fwd)
    assert abs(float(loss.detach()) - float(ref["loss"])) <= fwd * abs(float(ref["loss"]))
    _gate("gx", x.grad, ref["gx"], gin)
    for k, p in model.named_parameters():
        _gate("gp:" + k, p.grad, ref["gp:" + k], gpar)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_ahmed_pooling_16bit_trains(dtype):
    d, meta = load("poolmgn_ahmed_h32")
    model = _ahmed_model(meta)
    model.load_state_dict(params(d))
    model = model.to(dtype).to(DEV)
    t = {k: d[k].to(dtype).to(DEV) for k in ("x", "edge_attr", "y")}
    t["edge_index"], t["batch"] = d["edge_index"].to(DEV), d["batch"].to(DEV)
    model.eval()
    with torch.no_grad():
        pred = run_model(model, t)
    print(f"{dtype} pred rel-L2 vs the fp32 golden {rel_l2(pred.float().cpu(), d['pred']):.3e}")
    # train.py:20-40 offers bfloat16, not float16: Adam's eps = 1e-8 is 0 in float16 and a zero
    # gradient would step by 0 / 0, so the float16 case stops after the backward
    train_step(model, t, step=dtype != torch.float16)
