"""aerognn/parts.py on the CPU: the one reading of a reference module's Linears, LayerNorm and activation
hands out the module's own Parameters (identity, not equality), and the packed route (functions.ChainSpec)
and the float64 route (f64.Chain) bound from one record list the same Parameters in the same order."""
import pytest
import torch
from torch import nn


def _same(got, want):
    """Two (possibly nested) lists of tensors / None hold the same objects."""
    assert len(got) == len(want)
    for g, w in zip(got, want):
        if isinstance(w, (tuple, list)):
            _same(g, w)
        else:
            assert g is w


def test_mlp():
    from aerognn.parts import read
    from models.mlp import MLP
    m = MLP(10, 32, 8, 2)
    p = read(m)
    assert len(p.lins) == 4
    _same(p.lins, [(l.weight, l.bias) for l in m.layers])
    _same(p.ln, (m.layer_norm.weight, m.layer_norm.bias))
    assert p.eps == m.layer_norm.eps and p.act == "relu"
    q = read(MLP(10, 32, 8, 2, activation_fn="silu", use_layer_norm=False))
    assert q.ln is None and q.eps == 1e-5 and q.act == "silu"


def test_mlp_one_linear_quirk():
    """num_hidden_layers = 0 leaves one Linear input_dim -> output_dim (mlp.py:31-32)."""
    from aerognn.parts import read
    from models.mlp import MLP
    m = MLP(10, 32, 8, 0)
    p = read(m)
    _same(p.lins, [(m.layers[0].weight, m.layers[0].bias)])
    assert tuple(p.lins[0][0].shape) == (8, 10)
    _same(p.ln, (m.layer_norm.weight, m.layer_norm.bias))


def test_build_mlp_sequential_and_bare_linear():
    from aerognn.parts import read
    from models.trial1 import build_mlp
    seq = build_mlp(6, 32, 32, num_hidden_layers=2, dropout=0.1)
    assert any(isinstance(s, nn.Dropout) for s in seq)
    p = read(seq)
    lins = [s for s in seq if isinstance(s, nn.Linear)]
    assert len(lins) == 4
    _same(p.lins, [(l.weight, l.bias) for l in lins])
    _same(p.ln, (seq[-1].weight, seq[-1].bias))
    assert p.eps == seq[-1].eps and p.act == "relu"
    assert read(build_mlp(6, 32, 3, lay_norm=False)).ln is None
    lin = nn.Linear(32, 32)
    q = read(lin)
    _same(q.lins, [(lin.weight, lin.bias)])
    assert q.ln is None and q.eps == 1e-5 and q.act == "relu"


def test_edge_block_sum():
    from aerognn.parts import read
    from models.mgnLayer import EdgeBlockSum
    eb = EdgeBlockSum(32, 32, 32, 2, "silu", True)  # ReLU whatever activation_fn says (mgnLayer.py:81)
    p = read(eb)
    lins = [s for s in eb.mlp if isinstance(s, nn.Linear)]
    assert len(lins) == 3
    _same(p.lins, [(eb.edge_lin, None)] + [(l.weight, l.bias) for l in lins])
    _same(p.ln, (eb.mlp[-1].weight, eb.mlp[-1].bias))
    assert p.act == "relu"


def test_gmp_activation_names():
    from aerognn.parts import read
    from models.bistride_ops import GMP
    g = GMP(32, 32, 32, 'silu')
    for seq in (g.edge_mlp, g.node_mlp):
        p = read(seq)
        _same(p.lins, [(seq[0].weight, seq[0].bias), (seq[2].weight, seq[2].bias)])
        _same(p.ln, (seq[3].weight, seq[3].bias))
        assert p.act == "silu"
    assert g.spec().edge.act == g.spec().node.act != read(GMP(32, 32, 32).edge_mlp).act


def test_tanh_gelu_refused():
    from models.bistride_ops import GMP
    g = GMP(32, 32, 32)
    g.edge_mlp[1] = nn.GELU(approximate="tanh")
    with pytest.raises(NotImplementedError, match="aerognn GMP kernels implement ReLU / SiLU / GELU / Tanh MLPs"):
        g.spec()
    g.edge_mlp[1] = nn.GELU()
    g._spec = None
    assert g.spec().edge.params()[0] is g.edge_mlp[0].weight


def test_hidden_of():
    from aerognn.parts import hidden_of

    def lins(*outs):
        return [(torch.empty(o, 4), None) for o in outs]
    assert hidden_of(lins(8), 128) == 32
    assert hidden_of(lins(40), 128) == 64
    with pytest.raises(NotImplementedError, match="supports hidden_dim 32/64/128"):
        hidden_of(lins(200), 128)
    assert hidden_of(lins(64, 3), 64) == 64
    with pytest.raises(NotImplementedError, match="supports hidden_dim 32/64/128, got 48"):
        hidden_of(lins(48, 3), 48)


def _both_routes(parts, hidden):
    from aerognn import f64
    from aerognn.core import Pack
    from aerognn.functions import ChainSpec
    return ChainSpec.of(parts, hidden, Pack()).params(), f64.Chain.of(parts).params()


def test_both_routes_list_the_same_parameters():
    from aerognn.parts import read
    from models.mgnLayer import EdgeBlockSum
    from models.mlp import MLP
    m = MLP(10, 32, 8, 2)
    packed, f64 = _both_routes(read(m), 32)
    want = [t for l in m.layers for t in (l.weight, l.bias)] + [m.layer_norm.weight, m.layer_norm.bias]
    _same(packed, want)
    _same(f64, want)
    eb = EdgeBlockSum(32, 32, 32, 1)
    packed, f64 = _both_routes(read(eb), 32)
    lins = [s for s in eb.mlp if isinstance(s, nn.Linear)]
    want = [eb.edge_lin] + [t for l in lins for t in (l.weight, l.bias)] + [eb.mlp[-1].weight, eb.mlp[-1].bias]
    _same(packed, want)
    _same(f64, want)
