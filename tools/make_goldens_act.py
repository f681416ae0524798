"""Golden vectors of the reference's MLP under every elementwise torch.nn.functional activation the
kernels added after relu / gelu / silu / tanh, from the REAL reference (needs its checkout, as
tools/make_goldens.py does): models/mlp.py:37 `getattr(F, activation_fn)` with the input alone.

One file per name, tests/golden/act_<name>_f64.npz, with two float64 chains:
  a:  MLP(6, 32, 32, num_hidden_layers=2, activation_fn=name)                       (LayerNorm)
  b:  MLP(6, 32, 4, num_hidden_layers=1, activation_fn=name, use_layer_norm=False)
Per chain (keys prefixed `a:` / `b:`): the parameters (p:*), 37 input rows x, the output y, an upstream
gradient gy, the input gradient gx and the parameter gradients (gp:*).

The rows are kink-free (tests/actref.py kink_free_select): of 512 N(0, 1) candidates the first 37 are kept
whose hidden pre-activations, by the float64 formula, stay outside the margin of tests/chainref.py
kink_free_rows (1e-5 of the pre-activations' spread) around every kink of the function (0; 0 and 6; +-1;
+-3), on the parameters as drawn; and, on parameters and rows rounded to bf16 and to fp16, outside
2 eps_T max(|kink|, spread) (a 16-bit chain's pre-activations are about eps_T of the spread from the
float64 formula's, so an element that close to a kink may lie on its other side in either code, and
the 16-bit comparison would count coin flips). The script fails if fewer than 37 are found; no row is
exempt from any comparison. A LayerNorm gets gamma ~ U(0.5, 1.5), beta ~ N(0, 0.5^2) (tools/make_goldens_dropout.py).

Run:  python tools/make_goldens_act.py
"""
from __future__ import annotations

import os
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))

import torch  # noqa: E402

from make_goldens import MLP, save  # noqa: E402  (installs the stand-ins; MLP is the reference's)
from actref import NEW, kink_free_select  # noqa: E402

ROWS, CANDIDATES = 37, 512
CHAINS = (("a", dict(input_dim=6, hidden_dim=32, output_dim=32, num_hidden_layers=2, use_layer_norm=True)),
          ("b", dict(input_dim=6, hidden_dim=32, output_dim=4, num_hidden_layers=1, use_layer_norm=False)))


def case(name, index):
    arrs, meta = {}, {"activation_fn": name, "rows": ROWS}
    for tag, kw in CHAINS:
        torch.manual_seed(1000 + 10 * index + (tag == "b"))
        m = MLP(activation_fn=name, **kw).double()
        if kw["use_layer_norm"]:
            with torch.no_grad():
                m.layer_norm.weight.uniform_(0.5, 1.5)
                m.layer_norm.bias.normal_(0.0, 0.5)
        g = torch.Generator().manual_seed(2000 + 10 * index + (tag == "b"))
        cand = torch.randn(CANDIDATES, kw["input_dim"], generator=g, dtype=torch.float64)
        state = {k: v.detach().clone() for k, v in m.state_dict().items()}
        x = kink_free_select(state, cand, name, ROWS).requires_grad_(True)
        y = m(x)
        gy = torch.randn(ROWS, kw["output_dim"], generator=g, dtype=torch.float64)
        y.backward(gy)
        assert all(bool(torch.isfinite(t).all()) for t in (y, x.grad))
        arrs.update({f"{tag}:x": x, f"{tag}:y": y, f"{tag}:gy": gy, f"{tag}:gx": x.grad})
        arrs.update({f"{tag}:p:{k}": v for k, v in m.state_dict().items()})
        arrs.update({f"{tag}:gp:{k}": p.grad for k, p in m.named_parameters()})
        meta[tag] = kw
    save(f"act_{name}_f64", meta, **arrs)


if __name__ == "__main__":
    torch.set_num_threads(8)
    for i, n in enumerate(NEW):
        if len(sys.argv) == 1 or n in sys.argv[1:]:
            case(n, i)
