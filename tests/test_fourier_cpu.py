"""FourierMeshGraphNet / MLPNet drop-ins and torch.ops.aerognn.fourier_embed without a GPU:
imports, state_dict keys and shapes against the reference's golden parameters, the C-ABI symbols,
the no-CPU-fallback rule and the fake kernel's shape. Numerics: tests/test_gpu_fourier.py."""
import ctypes

import pytest
import torch

from golden_util import load, params


def _fourier_model(meta):
    from models.fouriermgn import FourierMeshGraphNet
    return FourierMeshGraphNet(*meta["dims"], **meta["kwargs"])


def _mlpnet(meta):
    from models.mlpnet import MLPNet
    return MLPNet(*meta["dims"], **meta["kwargs"])


def test_modules_import():
    from models.fouriermgn import FourierMeshGraphNet
    from models.mlpnet import MLPNet
    assert FourierMeshGraphNet.__name__ == "FourierMeshGraphNet" and MLPNet.__name__ == "MLPNet"


@pytest.mark.parametrize("name,build", [("fouriermgn3_f32", _fourier_model), ("fouriermgn3_f64", _fourier_model),
                                        ("mlpnet_f32", _mlpnet)])
def test_golden_state_dict_loads_strict(name, build):
    """Keys and shapes are the reference's: its parameters load with strict=True."""
    d, meta = load(name)
    model = build(meta)
    sd = params(d)
    res = model.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert list(model.state_dict().keys()) == list(sd.keys())  # registration (= init) order too


def test_node_encoder_input_width():
    d, meta = load("fouriermgn3_f32")
    model = _fourier_model(meta)
    assert model.node_encoder.layers[0].weight.shape[1] == 6 + 28
    from models.mgnLayer import EdgeBlock
    assert all(isinstance(layer.edge_block, EdgeBlock) for layer in model.layers)  # no do_concat_trick


def test_constructor_defaults_are_the_reference_s():
    import inspect
    from models.fouriermgn import FourierMeshGraphNet
    from models.mlpnet import MLPNet
    p = inspect.signature(FourierMeshGraphNet.__init__).parameters
    assert list(p)[1:4] == ["input_node_dim", "input_edge_dim", "output_node_dim"]
    assert (p["processor_size"].default, p["aggregation"].default, p["fourier_features_dim"].default,
            p["fourier_freq_start"].default, p["fourier_freq_length"].default) == (15, "sum", 2, -3, 7)
    q = inspect.signature(MLPNet.__init__).parameters
    assert (q["hidden_dim"].default, q["num_hidden_layers_encoder"].default,
            q["num_hidden_layers_decoder"].default) == (128, 2, 2)


def test_symbols_declared_and_exported():
    from aerognn import _lib
    names = _lib.exported_symbols()
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for sym in ("agn_fourier_embed", "agn_fourier_embed_bwd"):
        assert sym in names
        assert getattr(cdll, sym) is not None
        assert getattr(_lib.lib(), sym) is not None


def test_argument_errors_need_no_device():
    """The entries validate before they launch, so the codes come back on a machine without a GPU."""
    from aerognn import _lib
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.agn_fourier_embed(_lib.F32, 1, 2, None, 2, 2, -3, 7, 1, p, 30, None) == -1        # AGN_E_ARG
    assert L.agn_fourier_embed(7, 1, 2, p, 2, 2, -3, 7, 1, p, 30, None) == -2                  # AGN_E_DTYPE
    assert L.agn_fourier_embed(_lib.F32, 1, 2, p, 2, 3, -3, 7, 1, p, 30, None) == -4           # d > k
    assert L.agn_fourier_embed(_lib.F32, 0, 2, None, 2, 2, -3, 7, 1, None, 30, None) == 0      # n == 0
    assert L.agn_fourier_embed_bwd(_lib.F32, 1, 2, p, 2, 2, -3, 7, 1, p, 29, p, 2, None) == -4  # g_ld < row


def test_cpu_tensors_raise():
    import aerognn.ops  # noqa: F401
    from aerognn.functions import FourierEmbedFn
    x = torch.ones(3, 6)
    with pytest.raises(RuntimeError, match="MI355X"):
        torch.ops.aerognn.fourier_embed(x, 2, -3, 7, True)
    with pytest.raises(RuntimeError, match="MI355X"):
        torch.ops.aerognn.fourier_embed_backward(torch.ones(3, 34), x, 2, -3, 7, True)
    with pytest.raises(RuntimeError, match="MI355X"):
        FourierEmbedFn.apply(x, 2, -3, 7, True)
    d, meta = load("fouriermgn3_f32")
    model = _fourier_model(meta)
    with pytest.raises(RuntimeError, match="MI355X"):
        model.fourier_embedding(d["x"])
    with pytest.raises(RuntimeError):
        model(d["x"], d["edge_attr"], d["edge_index"])
    d, meta = load("mlpnet_f32")
    with pytest.raises(RuntimeError):
        _mlpnet(meta)(d["x"])


def test_op_schema_fake_kernel_and_autograd():
    import aerognn.ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    for name in ("fourier_embed", "fourier_embed_backward"):
        assert str(getattr(torch.ops.aerognn, name).default._schema).startswith(f"aerognn::{name}(")
    assert torch._C._dispatch_has_kernel_for_dispatch_key("aerognn::fourier_embed", "Autograd")
    with FakeTensorMode():
        x = torch.empty(10, 6, dtype=torch.bfloat16)
        y = torch.ops.aerognn.fourier_embed(x, 2, -3, 7, True)
        assert y.shape == (10, 6 + 28) and y.dtype == torch.bfloat16
        assert torch.ops.aerognn.fourier_embed(x, 3, 0, 1, False).shape == (10, 6)
        assert torch.ops.aerognn.fourier_embed(x, 3, -3, 7).shape == (10, 6 + 42)
        assert torch.ops.aerognn.fourier_embed_backward(y, x, 2, -3, 7, True).shape == (10, 6)
