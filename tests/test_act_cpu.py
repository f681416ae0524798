"""Every elementwise torch.nn.functional activation in the MLP chains (mlp.py:37 getattr(F, activation_fn)),
without a GPU: the names and codes of include/aerognn.h, the module bindings on both routes, what is
still refused, the argument errors of the entry points and the operator's fake kernels.
Numerics: tests/test_gpu_act.py."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

from actref import NEW, OLD, REFUSED

NAMES = OLD + NEW


def test_act_table_is_the_header_s():
    from aerognn import _lib as L
    assert len(NAMES) == 18 and tuple(L.ACT) == NAMES  # header order
    assert [L.ACT[n] for n in NAMES] == list(range(18))  # dense from 0: relu .. tanhshrink
    with open(L.HEADER) as f:
        text = f.read()
    codes = {m[1]: int(m[2]) for m in re.finditer(r"\b(AGN_ACT_[A-Z0-9_]+)\s*=\s*(\d+)", text)}
    assert codes == {"AGN_ACT_" + n.upper(): L.ACT[n] for n in NAMES}
    assert L.ACT_NONE == -1 and "none" not in L.ACT


@pytest.mark.parametrize("name", NAMES)
def test_name_is_an_elementwise_functional(name):
    f = getattr(F, name)
    x = torch.linspace(-4.0, 7.0, 12).view(3, 4)
    y = f(x)  # the input alone, as mlp.py:46 calls it
    assert y.shape == x.shape and y.dtype == x.dtype
    assert torch.equal(f(x[1:2, 2:3]), y[1:2, 2:3])  # elementwise: an element does not see its neighbours


@pytest.mark.parametrize("name", NAMES)
def test_mlp_binds_on_both_routes(name):
    from aerognn import _lib as L, f64, parts
    from models.mlp import MLP
    m = MLP(6, 32, 32, 2, activation_fn=name)
    s = m.spec()
    assert s.act == L.ACT[name] and s.nlin == 4
    c = f64.Chain.of(parts.read(m.double()))
    assert c.act == L.ACT[name]
    assert f64.mlp_chain(m).act == L.ACT[name]


@pytest.mark.parametrize("name", REFUSED)
def test_other_functionals_are_refused(name):
    from aerognn import f64
    from models.mlp import MLP
    m = MLP(6, 32, 32, 2, activation_fn=name)
    with pytest.raises(NotImplementedError, match="tanhshrink"):  # the message lists the set
        m.spec()
    with pytest.raises(NotImplementedError, match="tanhshrink"):
        f64.mlp_chain(m)


def test_model_constructs_with_a_new_activation():
    from models.mgn import MeshGraphNet
    m = MeshGraphNet(6, 4, 4, processor_size=2, activation_fn="leaky_relu", hidden_dim_processor=32,
                     hidden_dim_node_encoder=32, hidden_dim_edge_encoder=32, hidden_dim_decoder=32)
    for mlp in (m.node_encoder, m.edge_encoder, m.decoder, m.layers[0].node_block.mlp):
        assert mlp.spec().act == 6


def _fwd_args(L, act):
    buf = (ctypes.c_float * 1024)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    a = L.MlpFwdArgs()
    a.rows, a.dtype, a.hidden, a.nlin, a.out_dim, a.nseg, a.use_ln, a.out_ld = 1, L.F32, 32, 2, 32, 1, 0, 32
    a.seg[0].kind, a.seg[0].k, a.seg[0].ld, a.seg[0].ptr = L.SEG_PLAIN, 32, 32, p
    a.out, a.act_fn = p, act
    return a, buf


def _bwd_args(L, act):
    buf = (ctypes.c_float * 1024)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    a = L.MlpBwdArgs()
    a.rows, a.dtype, a.hidden, a.nlin, a.out_dim, a.in_dim, a.use_ln = 1, L.F32, 32, 2, 32, 32, 0
    a.g, a.din_nseg, a.act_fn = p, 1, act
    a.din_k[0], a.din[0], a.gpre[0], a.gpre[1], a.pre[0], a.mask[0] = 32, p, p, p, p, p
    return a, buf


def test_codes_out_of_range_are_argument_errors():
    """One past the last code, and -1 where AGN_ACT_NONE does not apply: AGN_E_ARG before any launch, so
    the codes come back on a machine without a GPU."""
    from aerognn import _lib as L
    lib = L.lib()
    last = max(L.ACT.values())
    assert last == L.ACT["tanhshrink"] == 17
    for act in (last + 1, -1, -2):
        a, keep = _fwd_args(L, act)
        assert lib.agn_mlp_forward(ctypes.byref(a), None) == L.E_ARG, act
        b, keep = _bwd_args(L, act)
        assert lib.agn_mlp_backward(ctypes.byref(b), None) == L.E_ARG, act
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    m = ctypes.cast((ctypes.c_ubyte * 8)(), ctypes.c_void_p)
    for act in (last + 1, -2):  # -1 is AGN_ACT_NONE here
        assert lib.agn_act_dropout_fwd(L.F32, act, 8, p, p, m, 0.0, 0, 0, None) == L.E_ARG, act
        assert lib.agn_act_dropout_bwd(L.F32, act, 8, p, p, m, p, 0.0, None) == L.E_ARG, act
    g = L.F64GemmArgs()
    g.rows, g.n, g.nseg, g.out = 1, 1, 0, ctypes.cast(buf, ctypes.c_void_p).value
    for field in ("relu", "mask_act"):  # the float64 epilogue codes are 1 + AGN_ACT_*
        setattr(g, field, last + 2)
        assert lib.agn_f64_gemm(ctypes.byref(g), None) == L.E_ARG, field
        setattr(g, field, 0)


def test_operator_names():
    import aerognn.ops as ops
    from aerognn import _lib as L
    for name in NAMES:
        assert ops._act_code(name) == L.ACT[name]
    assert ops._act_code("none") == L.ACT_NONE
    with pytest.raises(ValueError, match="tanhshrink"):
        ops._act_code("softmax")


@pytest.mark.parametrize("name", NEW)
def test_fake_kernels_accept_the_names(name):
    import aerognn.ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        y = torch.empty(5, 7, dtype=torch.bfloat16)
        out, mask = torch.ops.aerognn.act_dropout(y, name, 0.0)
        assert out.shape == y.shape and out.dtype == y.dtype and mask.shape == (5,) and mask.dtype == torch.uint8
        assert torch.ops.aerognn.act_dropout_backward(y, y, mask, name, 0.0).shape == y.shape


def test_no_reference_text_in_the_goldens():
    """The goldens hold arrays and a JSON meta string, no pickles (np.load's default refuses them)."""
    from golden_util import GOLDEN, load
    for name in NEW:
        d, meta = load(f"act_{name}_f64")
        assert meta["activation_fn"] == name and meta["rows"] == 37
        assert d["a:x"].shape == (37, 6) and d["b:y"].shape == (37, 4) and d["a:x"].dtype == torch.float64
        assert os.path.getsize(os.path.join(GOLDEN, f"act_{name}_f64.npz")) < 256 * 1024
