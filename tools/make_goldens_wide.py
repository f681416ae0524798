"""Golden vectors for MLP chains whose input is wider than 3 x hidden, from the REAL reference (needs
its checkout, as tools/make_goldens.py does), and the settings of every config.yaml experiment.

Imports tools/make_goldens.py for its stand-ins and helpers (importing it runs no case). Writes under
tests/golden/, tensors and settings only:

  mlp_wide_h32     MLP(142, 32, 32, num_hidden_layers=2) with LayerNorm on 130 rows
  mlp_wide_h128    MLP(450, 128, 128, 2) with LayerNorm on 33 rows
  mlp_wide_nh0     MLP(142, 32, 4, num_hidden_layers=0, use_layer_norm=False): the single-Linear quirk
  mlp_wide_dec     MLP(142, 32, 4, 2, use_layer_norm=False, activation_fn='gelu')
      <case>.npz     : x, gy (output gradient), the parameters (p:*), and the float32 y, gx, gp:*
      <case>_f64.npz : y, gx, gp:* of the same module in float64 on the same (upcast) tensors
  poolmgn_ahmed_h32  poolMGN as train.py:130-150 builds it for the ahmedBody_pooling_mgn experiment
      (dims 14 / 4 / 4, hidden_dim 32, global_dim 128, mean pooling, 'add' aggregation) with
      processor_size cut to 3, on a two-graph batch (ellipsoid(12, 8) + ellipsoid(10, 10), 196 nodes)
      whose node features are [pos, normals, 8 per-graph constants] (dataset.py:66-106): a train step
      (pred, MSE loss, gx, gp:*), the float64 results in poolmgn_ahmed_h32_f64.npz
  config_experiments.json  for each entry under config.yaml's `experiments:` the model name, the model
      kwargs merged by the override rule of utils.py:132-169 (an experiment key overrides the block that
      declares it) and the dataset's feature counts (d_n, d_e, d_out) by dataset.py:39-106:
      d_n = pos + normals + var_keys, d_e = pos + 1, d_out = output_features

Run:  python tools/make_goldens_wide.py
"""
from __future__ import annotations

import copy
import json
import os
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
import yaml  # noqa: E402

import make_goldens as G  # noqa: E402  (installs the stand-ins, puts the reference first on sys.path)
from make_goldens import MLP, batch_tensors, grads, poolMGN, save, sd  # noqa: E402

AHMED_KW = dict(processor_size=3, activation_fn="relu", num_hidden_layers_node_processor=2,
                num_hidden_layers_edge_processor=2, hidden_dim_processor=32, num_hidden_layers_node_encoder=2,
                hidden_dim_node_encoder=32, num_hidden_layers_edge_encoder=2, hidden_dim_edge_encoder=32,
                aggregation="add", hidden_dim_decoder=32, num_hidden_layers_decoder=2, global_pool_method="mean",
                num_hidden_layers_global_encoder=2, global_dim=128, dropout=0.0)
AHMED_DIMS = (14, 4, 4)
AHMED_MESHES = [(12, 8, 0), (10, 10, 1)]

MLP_CASES = {
    # name: (rows, seed, MLP kwargs)
    "mlp_wide_h32": (130, 31, dict(input_dim=142, hidden_dim=32, output_dim=32, num_hidden_layers=2,
                                   use_layer_norm=True)),
    "mlp_wide_h128": (33, 32, dict(input_dim=450, hidden_dim=128, output_dim=128, num_hidden_layers=2,
                                   use_layer_norm=True)),
    "mlp_wide_nh0": (130, 33, dict(input_dim=142, hidden_dim=32, output_dim=4, num_hidden_layers=0,
                                   use_layer_norm=False)),
    "mlp_wide_dec": (130, 34, dict(input_dim=142, hidden_dim=32, output_dim=4, num_hidden_layers=2,
                                   use_layer_norm=False, activation_fn="gelu")),
}


def case_mlp(name):
    rows, seed, kw = MLP_CASES[name]
    torch.manual_seed(seed)
    m = MLP(**kw)
    x = torch.randn(rows, kw["input_dim"])
    gy = torch.randn(rows, kw["output_dim"])
    out = {}
    for dtype in (torch.float32, torch.float64):
        md = copy.deepcopy(m).to(dtype)
        xd = x.detach().to(dtype).clone().requires_grad_(True)
        y = md(xd)
        y.backward(gy.to(dtype))
        out[dtype] = dict(y=y, gx=xd.grad, **grads(md))
    save(name, dict(kw, rows=rows, seed=seed), x=x, gy=gy, **sd(m), **out[torch.float32])
    save(name + "_f64", dict(kw, rows=rows, seed=seed), **out[torch.float64])


def ahmed_batch():
    """The two-graph batch with Ahmed-body node features: [pos, normals] of the meshes and 8 constants
    per graph in the var_keys' place (dataset.py:84-101 broadcasts each scalar to the graph's nodes)."""
    t = batch_tensors(AHMED_MESHES)
    g = torch.Generator().manual_seed(41)
    var = torch.randn(len(AHMED_MESHES), 8, generator=g)
    t["x"] = torch.cat([t["x"], var[t["batch"]]], 1)
    assert t["x"].shape[1] == AHMED_DIMS[0] and t["edge_attr"].shape[1] == AHMED_DIMS[1]
    return t


def case_poolmgn_ahmed():
    torch.manual_seed(40)
    m = poolMGN(*AHMED_DIMS, **AHMED_KW)
    assert m.node_encoder.layers[0].in_features == 142
    t = ahmed_batch()
    out = {}
    for dtype in (torch.float32, torch.float64):
        md = copy.deepcopy(m).to(dtype)
        x = t["x"].detach().to(dtype).clone().requires_grad_(True)
        pred = md(x, t["edge_attr"].to(dtype), t["edge_index"], batch=t["batch"])
        loss = torch.nn.MSELoss()(pred, t["y"].to(dtype))
        loss.backward()
        out[dtype] = dict(pred=pred, loss=loss, gx=x.grad, **grads(md))
    meta = dict(kwargs=AHMED_KW, dims=list(AHMED_DIMS), meshes=AHMED_MESHES)
    save("poolmgn_ahmed_h32", meta, x=t["x"], edge_attr=t["edge_attr"], edge_index=t["edge_index"], batch=t["batch"],
         y=t["y"], **sd(m), **out[torch.float32])
    save("poolmgn_ahmed_h32_f64", meta, **out[torch.float64])


def case_config():
    cfg = yaml.safe_load(open(os.path.join(G.REF, "config.yaml")))
    out = {}
    for name, exp in cfg["experiments"].items():
        exp = copy.deepcopy(exp)
        ds_key = exp["dataset"]
        note = None
        if ds_key not in cfg["dataset"]:  # missile3d1 names `missile_3d_1`; the block is `missile_3d1`
            fixed = ds_key.replace("_3d_", "_3d")
            assert fixed in cfg["dataset"], ds_key
            note = f"dataset key {ds_key!r} is not in config.yaml; built from {fixed!r}"
            ds_key = fixed
        ds = cfg["dataset"][ds_key]
        model = copy.deepcopy(cfg["model"][exp["model"]])
        # utils.py:144-158: the dataset block takes its keys first, then the model block, then training
        taken = {k for k in exp if k in ds}
        model.update({k: v for k, v in exp.items() if k in model and k not in taken})
        pos_dim = len(ds["input_features"]) // 2  # [coordinates, normals]
        dims = [2 * pos_dim + len(ds.get("var_keys", [])), pos_dim + 1, len(ds["output_features"])]
        out[name] = dict(model=exp["model"], kwargs=model, dataset=ds_key, dims=dims)
        if note:
            out[name]["note"] = note
    path = os.path.join(G.OUT, "config_experiments.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"config_experiments.json: {len(out)} experiments")


if __name__ == "__main__":
    torch.set_num_threads(8)
    for c in MLP_CASES:
        case_mlp(c)
    case_poolmgn_ahmed()
    case_config()
