"""Golden vectors that pin WHERE the reference applies training-mode dropout, from the REAL reference
(needs its checkout, as tools/make_goldens.py does).

torch's random stream cannot be reproduced by another implementation, so the goldens are mask-matched:
the module's Dropout is replaced at run time (on the instance, nothing of the reference is edited) by a
module that is truthy like nn.Dropout (models/mlp.py:44 tests `if self.dropout:`) and returns
x * mask * (1 / (1 - p)), the masks being those of tests/dropoutref.py (the numpy restatement of
csrc/dropout.hip's Philox4x32-10) at a recorded (seed, starting offset, p), consumed in call order: what
the kernels draw when torch's generator stands at that seed and offset. Everything else (which
activations get a dropout, the order of the calls, the arithmetic around them) is the reference's.

Cases (40 rows each; <case>.npz float32, <case>_f64.npz the same module in float64 on the upcast tensors):
  drop_mlp_relu_ln   MLP(6, 32, 32, 2, 'relu', dropout=P) with LayerNorm
  drop_mlp_gelu      MLP(32, 32, 4, 2, 'gelu', dropout=P, use_layer_norm=False)
  drop_mlp_nh0       MLP(6, 32, 32, 0, dropout=P): one Linear, so no dropout is ever called; y equals
                     the p = 0 module's bit for bit (asserted here)
Stored: x, the parameters (p:*), y, and gx / gp:* of the loss y.square().mean(); meta holds seed, offset, p,
the constructor arguments and the number of dropout calls.

A LayerNorm gets gamma ~ U(0.5, 1.5) and beta ~ N(0, 0.5^2) in place of its initial (1, 0). With the initial
values sum(y^2) over a row is the constant M (up to eps), the gradient of this loss behind the LayerNorm is a
difference of nearly equal terms, and the reference's own float32 step is 1.6e-4 (MLP(6, 32, 32, 2)) and
1.4e-3 (MLP(6, 32, 32, 0)) rel-L2 from its float64 step in the input gradient: no float32 code could
meet 1e-5 there. Each case prints the reference's own float32-against-float64 figures.

Run:  python tools/make_goldens_dropout.py
"""
from __future__ import annotations

import copy
import os
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))

import torch  # noqa: E402
from torch import nn  # noqa: E402

from make_goldens import MLP, grads, save, sd  # noqa: E402  (installs the stand-ins; MLP is the reference's)
from dropoutref import MaskStream  # noqa: E402

P = 0.25
SEED = 0x5EED0DD5EED
OFFSET = 4 * 1000
ROWS = 40


class MaskedDropout(nn.Module):
    """nn.Dropout's place in the module, with the masks of a MaskStream (a Module is truthy)."""

    def __init__(self, stream):
        super().__init__()
        self.stream, self.calls = stream, 0

    def forward(self, x):
        self.calls += 1
        return x * self.stream.next(tuple(x.shape)).to(x.dtype) * (1.0 / (1.0 - self.stream.p))


def _install(m, stream):
    """Replace the instance's nn.Dropout by a MaskedDropout on `stream`."""
    assert isinstance(m.dropout, nn.Dropout) and m.dropout.p == P
    m.dropout = MaskedDropout(stream)
    return m.dropout


def case(name, seed, build, in_dim, meta):
    torch.manual_seed(seed)
    m = build()
    m.train()
    x = torch.randn(ROWS, in_dim)
    for mod in m.modules():
        if isinstance(mod, nn.LayerNorm):  # see the module docstring
            with torch.no_grad():
                mod.weight.copy_(0.5 + torch.rand(mod.weight.shape))
                mod.bias.copy_(0.5 * torch.randn(mod.bias.shape))
    out, calls = {}, None
    for dtype in (torch.float32, torch.float64):
        md = copy.deepcopy(m).to(dtype)
        drop = _install(md, MaskStream(SEED, OFFSET, P))
        xd = x.detach().to(dtype).clone().requires_grad_(True)
        y = md(xd)
        y.square().mean().backward()
        out[dtype] = dict(y=y, gx=xd.grad, **grads(md))
        assert calls in (None, drop.calls)
        calls = drop.calls
    meta = dict(meta, rows=ROWS, seed=SEED, offset=OFFSET, p=P, model_seed=seed, dropout_calls=calls)
    f32, f64 = out[torch.float32], out[torch.float64]
    rel = {k: float((f32[k].double() - f64[k]).norm() / f64[k].norm()) for k in f32}
    print(f"{name}: the reference's float32 against its float64: y {rel['y']:.2e}, gx {rel['gx']:.2e}, worst gp "
          f"{max(v for k, v in rel.items() if k.startswith('gp:')):.2e}")
    save(name, meta, x=x, **sd(m), **out[torch.float32])
    save(name + "_f64", meta, **out[torch.float64])
    return m, x, out, calls


if __name__ == "__main__":
    torch.set_num_threads(8)
    kw = dict(input_dim=6, hidden_dim=32, output_dim=32, num_hidden_layers=2, activation_fn="relu", dropout=P)
    _, _, _, n = case("drop_mlp_relu_ln", 51, lambda: MLP(**kw), 6, dict(kind="mlp", kwargs=kw))
    assert n == 3
    kw = dict(input_dim=32, hidden_dim=32, output_dim=4, num_hidden_layers=2, activation_fn="gelu", dropout=P,
              use_layer_norm=False)
    _, _, _, n = case("drop_mlp_gelu", 52, lambda: MLP(**kw), 32, dict(kind="mlp", kwargs=kw))
    assert n == 3
    kw = dict(input_dim=6, hidden_dim=32, output_dim=32, num_hidden_layers=0, dropout=P)
    m, x, out, n = case("drop_mlp_nh0", 53, lambda: MLP(**kw), 6, dict(kind="mlp", kwargs=kw))
    torch.manual_seed(53)
    m0 = MLP(**dict(kw, dropout=0.0)).train()
    m0.load_state_dict(m.state_dict())
    assert n == 0 and torch.equal(m0(x), out[torch.float32]["y"])
