"""What a reference nn.Module gives the kernels: its Linears, LayerNorm and activation, read in ONE place.

read(module) -> Parts(lins, ln, eps, act) of
  * a models/mlp.py MLP (layers, use_layer_norm / layer_norm, activation_fn),
  * an nn.Sequential of Linear / activation / Dropout / LayerNorm modules or a bare nn.Linear (trial1's
    build_mlp and linout, EdgeBlockSum.mlp, GMP.edge_mlp / node_mlp),
  * an EdgeBlockSum (mgnLayer.py:72-105): (edge_lin, None) in front of its Sequential's Linears.
The tensors are the module's own Parameters. functions.ChainSpec (packed operands) and f64.Chain
(float64) are both built from this record, so a module binds the same way on either route.
hidden_of(lins, hidden_dim) is the `hidden` the fused MLP kernels run such a chain at.

Only torch.nn is imported here: this loads without the library, below functions.py and f64.py.
"""
from collections import namedtuple

from torch import nn

# lins: [(weight, bias or None)] in order; ln: (gamma, beta) or None; eps: the LayerNorm's (1e-5 without
# one); act: the activation between the Linears by its mlp.py:37 name
Parts = namedtuple("Parts", "lins ln eps act")

ACT_NAMES = {nn.ReLU: "relu", nn.SiLU: "silu", nn.GELU: "gelu", nn.Tanh: "tanh"}


def _parts(linears, ln, act):
    return Parts([(m.weight, m.bias) for m in linears], (ln.weight, ln.bias) if ln is not None else None,
                 ln.eps if ln is not None else 1e-5, act)


def read(m):
    if hasattr(m, "edge_lin"):
        # EdgeBlockSum: its chain is ReLU whatever activation_fn says (mgnLayer.py:81)
        p = read(m.mlp)
        return Parts([(m.edge_lin, None)] + p.lins, p.ln, p.eps, "relu")
    if hasattr(m, "activation_fn"):  # models/mlp.py (layer list: mlp.py:21-35)
        return _parts(m.layers, m.layer_norm if m.use_layer_norm else None, m.activation_fn)
    mods = [m] if isinstance(m, nn.Linear) else list(m)
    acts = [s for s in mods if not isinstance(s, (nn.Linear, nn.Dropout, nn.LayerNorm))]
    names = {ACT_NAMES.get(type(s)) for s in acts}
    # the kernels compute the exact (erf) GELU: a tanh-approximated one is refused
    if None in names or len(names) > 1 or any(isinstance(s, nn.GELU) and s.approximate != "none" for s in acts):
        raise NotImplementedError("aerognn GMP kernels implement ReLU / SiLU / GELU / Tanh MLPs")
    lns = [s for s in mods if isinstance(s, nn.LayerNorm)]
    return _parts([s for s in mods if isinstance(s, nn.Linear)], lns[0] if lns else None,
                  names.pop() if names else "relu")


def hidden_of(lins, hidden_dim):
    """The `hidden` of a chain: hidden_dim with more than one Linear, else the single Linear's outputs
    rounded up to 32."""
    H = hidden_dim if len(lins) > 1 else max(32, ((lins[0][0].shape[0] + 31) // 32) * 32)
    if H not in (32, 64, 128):
        raise NotImplementedError(f"aerognn fused MLP supports hidden_dim 32/64/128, got {H}")
    return H
