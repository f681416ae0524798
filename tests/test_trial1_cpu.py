"""MeshGraphNet_v2 (models/trial1.py) without a GPU: names, state_dict keys and shapes against the
reference's golden parameters (tools/make_goldens_trial1.py), the initial weights of a seed, the
reference's parameter counts, the no-CPU-fallback rule and the dropout rule.
Numerics: tests/test_gpu_trial1.py."""
import inspect

import pytest
import torch

from golden_util import load, params


def _model(meta, **kw):
    from models.trial1 import MeshGraphNet_v2
    return MeshGraphNet_v2(*meta["args"], **kw)


def test_names_and_signatures():
    import models.trial1 as t1
    for n in ("build_mlp", "NodeEncoder", "EdgeEncoder", "GlobalEncoder", "MeshGraphNetLayer_v2", "MeshGraphNet_v2"):
        assert hasattr(t1, n), n
    assert t1.MeshGraphNet_v2(6, 4, 32, 4, 1).__class__.__name__ == "MeshGraphNet_v2"  # utils.py:179 dispatches on it
    p = inspect.signature(t1.MeshGraphNet_v2.__init__).parameters
    assert list(p)[1:] == ["node_input_size", "edge_input_size", "hidden_channels", "out_channels",
                           "num_graph_conv_layers", "num_encoder_layers", "num_decoder_layers", "dropout"]
    assert (p["num_encoder_layers"].default, p["num_decoder_layers"].default, p["dropout"].default) == (2, 2, 0.0)
    assert list(inspect.signature(t1.MeshGraphNet_v2.forward).parameters)[1:] == ["node_attr", "edge_attr", "edge_index",
                                                                                 "batch"]
    assert list(inspect.signature(t1.MeshGraphNetLayer_v2.forward).parameters)[1:] == ["x", "edge_index", "edge_attr"]
    q = inspect.signature(t1.build_mlp).parameters
    assert list(q) == ["input_dim", "hidden_dim", "output_dim", "num_hidden_layers", "lay_norm", "pooling", "dropout"]
    assert (q["num_hidden_layers"].default, q["lay_norm"].default, q["pooling"].default, q["dropout"].default) == \
        (2, True, False, 0.0)


@pytest.mark.parametrize("name", ["trial1_f32", "trial1_f64", "trial1_dec1"])
def test_golden_state_dict_loads_strict(name):
    """Keys, shapes and registration order are the reference's: its parameters load with strict=True."""
    d, meta = load(name)
    model = _model(meta)
    sd = params(d)
    if name == "trial1_f64":
        model = model.double()
    res = model.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    own = model.state_dict()
    assert list(own.keys()) == list(sd.keys())
    assert all(own[k].shape == sd[k].shape for k in sd)


def test_layer_golden_loads_strict():
    from models.trial1 import MeshGraphNetLayer_v2
    d, meta = load("trial1_layer_h128")
    layer = MeshGraphNetLayer_v2(meta["H"])
    sd = params(d)
    layer.load_state_dict(sd, strict=True)
    assert list(layer.state_dict().keys()) == list(sd.keys())
    assert layer.node_mlp[0].weight.shape == (128, 256)


def test_state_dict_keys_carry_the_sequential_indices():
    d, meta = load("trial1_f32")
    assert meta["args"][5:] == [3, 2]
    keys = set(params(d))
    for enc in ("node_encoder", "edge_encoder"):
        for i in (0, 2, 5, 8, 11, 12):
            assert {f"{enc}.mlp.{i}.weight", f"{enc}.mlp.{i}.bias"} <= keys
    for i in (0, 2, 5, 8, 11):
        assert f"extract_feature.mlp.{i}.weight" in keys
    assert "extract_feature.mlp.12.weight" not in keys and "extract_feature.linout.weight" in keys
    for chain in ("edge_mlp", "node_mlp"):
        for i in (0, 2, 5, 8, 9):
            assert f"layers.2.{chain}.{i}.bias" in keys
    assert {k for k in keys if k.startswith("decoder.")} == {f"decoder.{i}.{w}" for i in (0, 2, 5) for w in ("weight", "bias")}
    assert not any(k.startswith("dropout") for k in keys)
    # num_decoder_layers = 1: Linear, ReLU, Linear
    d1, _ = load("trial1_dec1")
    assert {k for k in params(d1) if k.startswith("decoder.")} == {f"decoder.{i}.{w}" for i in (0, 2) for w in ("weight", "bias")}


@pytest.mark.parametrize("name", ["trial1_f32", "trial1_dec1"])
def test_same_seed_gives_the_golden_initial_weights(name):
    d, meta = load(name)
    torch.manual_seed(meta["seed"])
    model = _model(meta)
    sd = params(d)
    for k, v in model.state_dict().items():
        assert torch.equal(v, sd[k]), k


def test_layer_seed_gives_the_golden_initial_weights():
    from models.trial1 import MeshGraphNetLayer_v2
    d, meta = load("trial1_layer_h128")
    torch.manual_seed(meta["seed"])
    layer = MeshGraphNetLayer_v2(meta["H"])
    sd = params(d)
    for k, v in layer.state_dict().items():
        assert torch.equal(v, sd[k]), k


@pytest.mark.parametrize("args,count", [((6, 4, 128, 4, 15, 3, 2), 2502404), ((6, 4, 32, 4, 15, 3, 2), 161732),
                                        ((14, 4, 32, 4, 15, 3, 2), 162244)])
def test_parameter_counts_are_the_reference_s(args, count):
    from models.trial1 import MeshGraphNet_v2
    assert sum(p.numel() for p in MeshGraphNet_v2(*args).parameters()) == count


def test_unused_dropout_attribute_exists():
    from models.trial1 import MeshGraphNet_v2
    m = MeshGraphNet_v2(6, 4, 32, 4, 1, dropout=0.25)
    assert isinstance(m.dropout, torch.nn.Dropout) and m.dropout.p == 0.25
    assert [mod.p for mod in m.decoder if isinstance(mod, torch.nn.Dropout)] == [0.25]
    assert all(mod.p == 0.0 for mod in m.node_encoder.mlp if isinstance(mod, torch.nn.Dropout))


def test_cpu_tensors_raise():
    from models.trial1 import MeshGraphNetLayer_v2
    d, meta = load("trial1_f32")
    model = _model(meta)
    with pytest.raises(RuntimeError, match="MI355X"):
        model(d["x"], d["edge_attr"], d["edge_index"], d["batch"])
    with pytest.raises(RuntimeError, match="MI355X"):
        model(d["x"], d["edge_attr"], d["edge_index"], None)
    with pytest.raises(RuntimeError, match="MI355X"):
        model.node_encoder(torch.ones(3, 38))
    with pytest.raises(RuntimeError, match="MI355X"):
        model.extract_feature(d["x"], d["edge_index"], d["batch"])
    with pytest.raises(RuntimeError, match="MI355X"):
        MeshGraphNetLayer_v2(32)(torch.ones(4, 32), torch.zeros(2, 3, dtype=torch.long), torch.ones(3, 32))


def test_training_dropout_raises():
    d, meta = load("trial1_f32")
    model = _model(meta, dropout=0.1)
    model.train()
    with pytest.raises(NotImplementedError, match="dropout"):
        model(d["x"], d["edge_attr"], d["edge_index"], d["batch"])
    model.eval()  # eval mode passes the dropout check (and then refuses the CPU tensors)
    with pytest.raises(RuntimeError, match="MI355X"):
        model(d["x"], d["edge_attr"], d["edge_index"], d["batch"])


def test_unsupported_hidden_width_raises():
    """Hidden widths other than 32 / 64 / 128 are refused when the chains are bound."""
    from models.trial1 import MeshGraphNetLayer_v2
    with pytest.raises(NotImplementedError, match="32/64/128"):
        MeshGraphNetLayer_v2(48).spec()


def test_edge_fwd_args_flag():
    """agn_edge_fwd_args keeps its layout: the trailing pad became the agg_mean flag."""
    import ctypes as C
    from aerognn import _lib as L
    names = [f for f, _ in L.EdgeFwdArgs._fields_]
    assert names[-2:] == ["nodes", "agg_mean"] and "_pad" not in names
    # 2 ints, 4 + 4 + 2 + 5 + 3 + 4 pointers, 2 ints
    assert C.sizeof(L.EdgeFwdArgs) == 8 + 22 * 8 + 8 and L.EdgeFwdArgs.agg_mean.offset == 8 + 22 * 8 + 4
