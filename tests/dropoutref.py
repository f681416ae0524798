"""Restatements of training-mode dropout for the tests (test infrastructure, not product code):
Philox4x32-10 and the keep-mask of csrc/dropout.hip in numpy, and the reference's chain
(models/mlp.py:40-51) with given masks in torch on the CPU.

The mask of element e at (seed, offset, p): word e & 3 of the Philox block with key (lo32(seed),
hi32(seed)) and counter (lo32(c), hi32(c), 0, 0), c = offset / 4 + (e >> 2) (mod 2^64); kept iff
word >= min(2^32 - 1, round(p 2^32)); p >= 1 keeps nothing. A call over n elements advances the
offset by 4 ceil(n / 4).
"""
import numpy as np
import torch
import torch.nn.functional as F

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
LO = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """ctr: [..., 4] (any integer type, values < 2^32), key: two ints < 2^32 -> [..., 4] uint32."""
    ctr = np.asarray(ctr)
    c = [ctr[..., i].astype(np.uint64) for i in range(4)]
    k0, k1 = int(key[0]) & LO, int(key[1]) & LO
    m0, m1, lo = np.uint64(M0), np.uint64(M1), np.uint64(LO)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]  # 32 x 32 -> 64 bits: no overflow
        c = [(p1 >> s32) ^ c[1] ^ np.uint64(k0), p1 & lo, (p0 >> s32) ^ c[3] ^ np.uint64(k1), p0 & lo]
        k0, k1 = (k0 + W0) & LO, (k1 + W1) & LO
    return np.stack(c, -1).astype(np.uint32)


def threshold(p):
    return min(2 ** 32 - 1, int(round(p * 2.0 ** 32)))


def advance(n):
    """What a call over n elements adds to the offset."""
    return 4 * ((n + 3) // 4)


def keep_mask(seed, offset, n, p):
    """bool [n]: element e is kept."""
    if p >= 1.0:
        return np.zeros(n, dtype=bool)
    nb = (n + 3) // 4
    base = (offset // 4) & (2 ** 64 - 1)
    if base + nb < 2 ** 63:  # the usual case, vectorised
        blk = np.uint64(base) + np.arange(nb, dtype=np.uint64)
    else:                    # near 2^64: Python integers
        blk = np.array([(base + b) & (2 ** 64 - 1) for b in range(nb)], dtype=np.uint64)
    ctr = np.zeros((nb, 4), dtype=np.uint64)
    ctr[:, 0] = blk & np.uint64(LO)
    ctr[:, 1] = blk >> np.uint64(32)
    words = philox4x32_10(ctr, (seed & LO, (seed >> 32) & LO)).reshape(-1)[:n]
    return words >= np.uint32(threshold(p)) if threshold(p) > 0 else np.ones(n, dtype=bool)


def pack_bits(kept):
    """The kernel's mask bytes: bit e & 7 of byte e >> 3."""
    return np.packbits(np.asarray(kept, dtype=np.uint8), bitorder="little")


def unpack_bits(mask_bytes, n):
    return np.unpackbits(np.asarray(mask_bytes, dtype=np.uint8), bitorder="little")[:n].astype(bool)


class MaskStream:
    """Masks in call order from a starting (seed, offset), as successive kernel calls draw them."""

    def __init__(self, seed, offset, p):
        self.seed, self.offset, self.p = seed, offset, p

    def next(self, shape):
        n = int(np.prod(shape))
        m = keep_mask(self.seed, self.offset, n, self.p).reshape(shape)
        self.offset += advance(n)
        return torch.from_numpy(m)


def mask_shapes(meta):
    """Per hidden Linear of a golden case (tools/make_goldens_dropout.py meta), the shape of its
    dropout's mask: mlp.py:41-45 has one behind every hidden activation, none with a single Linear."""
    kw, rows = meta["kwargs"], meta["rows"]
    return [(rows, kw["hidden_dim"])] * (kw["num_hidden_layers"] + 1 if kw["num_hidden_layers"] > 0 else 0)


def parts_of(sd):
    """([(W, b)], (gamma, beta) or None) of a state dict of models/mlp.py MLP ('layers.N.weight',
    'layer_norm.weight')."""
    n = sum(1 for k in sd if k.startswith("layers.") and k.endswith(".weight"))
    lins = [(sd[f"layers.{l}.weight"], sd[f"layers.{l}.bias"]) for l in range(n)]
    ln = (sd["layer_norm.weight"], sd["layer_norm.bias"]) if "layer_norm.weight" in sd else None
    return lins, ln


def chain(sd, x, masks, p, act="relu", dtype=torch.float64, grad=True, pres=None):
    """The reference's chain in `dtype` on the CPU: per hidden Linear l, h = act(linear(h)), then
    h = h * masks[l] * scale where masks[l] is not None (scale = 1 / (1 - p), rounded to dtype by the
    product; a float32 chain thus multiplies by (float)(1 / (1 - p)) as the kernel does). The loss of the
    goldens is y.square().mean(): returns (y, gx, {name: grad}) with grad, else y. pres: a list that
    receives the hidden pre-activations."""
    sd = {k: v.detach().to(dtype).clone().requires_grad_(grad) for k, v in sd.items()}
    lins, ln = parts_of(sd)
    x = x.detach().to(dtype).clone().requires_grad_(grad)
    scale = 1.0 / (1.0 - p) if p < 1.0 else 0.0
    h = x
    for l, (w, b) in enumerate(lins):
        h = F.linear(h, w, b)
        if l < len(lins) - 1:
            if pres is not None:
                pres.append(h.detach())
            h = getattr(F, act)(h)
            if masks[l] is not None:
                h = h * masks[l].to(dtype) * scale
    if ln is not None:
        h = F.layer_norm(h, (h.shape[1],), ln[0], ln[1], 1e-5)
    if not grad:
        return h.detach()
    h.square().mean().backward()
    return h.detach(), x.grad, {k: v.grad for k, v in sd.items()}


def kink_free_rows(sd, x, configs, gen, band, rounds=200):
    """tests/chainref.py's kink_free_rows for a ReLU chain with masks: rows of x with a float64
    pre-activation within band * std of 0 under any of `configs` = [(masks, p), ...] are re-drawn
    (the masks stay with the row's position) until none is. A ReLU derivative jumps there, and a 16-bit
    chain whose pre-activations carry a relative error of the order of the type's epsilon may take the
    other side than float64 does. Decided by the float64 formula alone, never by the kernels."""
    x = x.clone()
    for _ in range(rounds):
        near = torch.zeros(x.shape[0], dtype=torch.bool)
        for masks, p in configs:
            pres = []
            chain(sd, x, masks, p, grad=False, pres=pres)
            for t in pres:
                near |= (t.abs() < band * t.std()).any(1)
        if not near.any():
            return x
        x[near] = torch.randn(int(near.sum()), x.shape[1], generator=gen, dtype=torch.float64).to(x.dtype)
    raise AssertionError("rows not kink-free")
