"""References of one MLP chain (models/mlp.py:40-51) shared by the MLP tests: the float64 formula,
rows conditioned away from ReLU kinks, and torch's own 16-bit evaluation on the CPU (test
infrastructure, not product code)."""
import torch
import torch.nn.functional as F


def ref_chain(sd, x, act="relu", gy=None):
    """The float64 formula of models/mlp.py:40-51 on the parameters `sd` (any dtype, upcast):
    (y, pre-activations) or, with gy, (y, gx, {name: grad})."""
    p = {k: v.detach().cpu().double().requires_grad_(gy is not None) for k, v in sd.items()}
    x = x.detach().cpu().double().requires_grad_(gy is not None)
    n = sum(1 for k in p if k.startswith("layers.") and k.endswith(".weight"))
    h, pres = x, []
    for l in range(n):
        h = F.linear(h, p[f"layers.{l}.weight"], p[f"layers.{l}.bias"])
        if l < n - 1:
            pres.append(h)
            h = getattr(F, act)(h)
    if "layer_norm.weight" in p:
        h = F.layer_norm(h, (h.shape[1],), p["layer_norm.weight"], p["layer_norm.bias"], 1e-5)
    if gy is None:
        return h.detach(), [t.detach() for t in pres]
    h.backward(gy.detach().cpu().double())
    return h.detach(), x.grad, {k: v.grad for k, v in p.items()}


def kink_free_rows(sd, x, gen, act="relu", band=1e-5, rounds=8):
    """tests/kinkfree.py's rule for one chain: rows with a float64 ReLU input within band * std of 0 are
    re-drawn (a ReLU derivative jumps there, and two valid fp32 summation orders may take different
    sides), until none is. Decided by the float64 formula alone, never by the kernels."""
    if act != "relu":
        return x
    for _ in range(rounds):
        _, pres = ref_chain(sd, x)
        near = torch.zeros(x.shape[0], dtype=torch.bool)
        for t in pres:
            near |= (t.abs() < band * t.std()).any(1) if t.numel() > 1 else (t.abs() < band).any(1)
        if not near.any():
            return x
        x[near] = torch.randn(int(near.sum()), x.shape[1], generator=gen, dtype=x.dtype)
    raise AssertionError("rows not kink-free")


def torch_16bit(sd, x, act, gy):
    """torch's own evaluation of the chain in the 16-bit dtype on the CPU (the reference module's
    arithmetic, mlp.py:40-51): (y, gx, {name: grad})."""
    p = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    x = x.detach().clone().requires_grad_(True)
    n = sum(1 for k in p if k.startswith("layers.") and k.endswith(".weight"))
    h = x
    for l in range(n):
        h = F.linear(h, p[f"layers.{l}.weight"], p[f"layers.{l}.bias"])
        if l < n - 1:
            h = getattr(F, act)(h)
    if "layer_norm.weight" in p:
        h = F.layer_norm(h, (h.shape[1],), p["layer_norm.weight"], p["layer_norm.bias"], 1e-5)
    h.backward(gy)
    return h.detach(), x.grad, {k: v.grad for k, v in p.items()}
