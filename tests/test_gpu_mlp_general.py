"""The general fused-MLP kernels (csrc/mlp.hip mlp_fwd_kernel / mlp_bwd_kernel) at every hidden width,
storage type and I/O mode, at small shapes: rows 1 / 33 / 130 (one row; a wave plus a row; a 128-row
block plus two, which leaves idle waves in the last block).

Section 3 of the sweep calls core.mlp_forward / core.mlp_backward / _chain_param_grads directly and
checks every stored tensor with the save-chain method (tests/savechain.py: float64 of each step from
the kernel's own stored operands, per-element tolerance (n - 1/2) ulp_T(|ref| + d) + d, nothing fitted,
no element exempt). Every case asserts the kernel instantiation it reached (agn_debug_mlp_mode) and that
256 B of sentinel after (and the padding inside) every output are intact. The module-level part runs
models.mlp.MLP and MeshGraphNetLayer at H = 64 against float64 at the project's fp32 bars.
"""
import os

import pytest
import torch

import savechain as S
from chainref import kink_free_rows, ref_chain, torch_16bit
from golden_util import max_rel, rel_l2
from maskmatched import rows_of

pytestmark = pytest.mark.gpu
os.environ.setdefault("AEROGNN_MEMLOG", "0")

DEV = "cuda"
FWD, GIN, GPAR, B16 = 1e-5, 1e-5, 5e-5, 2e-2
M_VEC, M_GEN, M_NIN, M_NOUT, M_WIDE = 0, 1, 2, 3, 4
ROWS = (1, 33, 130)
SENT = 0xA5
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ["fp32", "bf16", "fp16"]
HS = [32, 64, 128]
NODES = 17  # rows of a gathered operand (every index repeats at 33 and 130 rows)


# ------------------------------------------------------------------------------ guarded buffers
class Guards:
    """Outputs with 256 B of sentinel after the last valid element (and before the first, for an
    offset view); rows are not padded. check() asserts the sentinel and every padding column intact."""

    def __init__(self):
        self.items = []

    def alloc(self, rows, k, dtype, ld=None, offset=0):
        ld = ld or k
        es = torch.empty(0, dtype=dtype).element_size()
        n = (rows - 1) * ld + k
        buf = torch.full(((offset + n) * es + 256,), SENT, dtype=torch.uint8, device=DEV)
        flat = buf[offset * es:(offset + n) * es].view(dtype)
        self.items.append((buf, offset * es, (offset + n) * es, rows, k, ld, es))
        return torch.as_strided(flat, (rows, k), (ld, 1))

    def rehome(self, t):
        """A tensor of the project's allocators (Fn._alloc_saves / _alloc_gpre, tiled or a mask) moved
        into a guarded buffer of exactly its size, attributes kept."""
        if t is None:
            return None
        nb = t.numel() * t.element_size()
        buf = torch.full((nb + 256,), SENT, dtype=torch.uint8, device=DEV)
        out = buf[:nb].view(t.dtype).view(t.shape)
        for k in ("agn_tiled", "agn_rows"):
            if hasattr(t, k):
                setattr(out, k, getattr(t, k))
        for k in ("agn_mask", "agn_pre"):
            if hasattr(t, k):
                setattr(out, k, self.rehome(getattr(t, k)))
        self.items.append((buf, 0, nb, 1, nb, nb, 1))
        return out

    def check(self):
        assert self.items
        for buf, b0, b1, rows, k, ld, es in self.items:
            assert bool((buf[b1:] == SENT).all()) and bool((buf[:b0] == SENT).all()), "sentinel overwritten"
            if ld > k and rows > 1:
                pad = torch.as_strided(buf, (rows - 1, (ld - k) * es), (ld * es, 1), b0 + k * es)
                assert bool((pad == SENT).all()), "row padding overwritten"


def _mode(backward):
    from aerognn import _lib as L
    return int(L.lib().agn_debug_mlp_mode(int(backward)))


def _rounded(t, dtype):
    """fp32 values representable in dtype (parameters stay fp32 tensors: their gradients stay fp32)."""
    return t.to(dtype).float()


# ------------------------------------------------------------------------------ one chain, end to end
class Chain:
    """Random parameters of one chain, packed as the models pack them. Weights are N(0, 1) K^-1/2 rounded
    to the storage type, biases and LayerNorm parameters fp32."""

    def __init__(self, H, dtype, K, nlin, out, ln, act="relu", bias0=True, seed=0):
        from aerognn.core import Pack
        from aerognn.functions import ChainSpec
        g = torch.Generator().manual_seed(seed)
        dims = [K] + [H] * (nlin - 1) + [out]
        self.w = [_rounded(torch.randn(dims[l + 1], dims[l], generator=g) * dims[l] ** -0.5, dtype).to(DEV)
                  for l in range(nlin)]
        self.b = [(0.1 * torch.randn(dims[l + 1], generator=g)).to(DEV) if (l > 0 or bias0) else None
                  for l in range(nlin)]
        self.ln = ((1.0 + 0.1 * torch.randn(out, generator=g)).to(DEV), (0.1 * torch.randn(out, generator=g)).to(DEV)) \
            if ln else None
        self.H, self.dtype, self.K, self.nlin, self.out, self.act = H, dtype, K, nlin, out, act
        self.spec = ChainSpec(list(zip(self.w, self.b)), self.ln, H, Pack(), "c", act=act)
        self.spec.pack.update(dtype, torch.device(DEV))
        self.W64 = [S.f64(w) for w in self.w]
        self.b64 = [None if b is None else S.f64(b) for b in self.b]
        self.ln64 = None if self.ln is None else (S.f64(self.ln[0]), S.f64(self.ln[1]))
        self.gen = g


def _randn(gen, rows, k, dtype, ld=None, offset=0):
    """An input [rows, k] of N(0, 1) in dtype, row stride ld, optionally a view offset by `offset` elements."""
    ld = ld or k
    flat = torch.zeros(offset + rows * ld, dtype=dtype, device=DEV)
    v = torch.as_strided(flat, (rows, k), (ld, 1), offset)
    v.copy_(torch.randn(rows, k, generator=gen).to(dtype))
    return v


def _rowptr(rows):
    """Receivers with no members, one with more than 32, and ranges that cross the 32-row tiles."""
    pat = [40, 0, 3, 5, 0, 1, 7, 2, 13, 0, 0, 9]
    cnt = torch.tensor([pat[i % len(pat)] for i in range(rows)])
    return torch.cat([torch.zeros(1, dtype=torch.long), cnt.cumsum(0)]).to(torch.int32)


def run_chain(c, rows, segs, *, fwd_mode, bwd_mode=None, resid=None, out_ld=None, out_offset=0, proj=None,
              tiled=True, backward=True, g_offset=0, g2=False, g_none=False, din_resid=False, wgrad=False, label=None,
              tag=""):
    """One forward (+ backward, + weight gradients) of chain c on `rows` rows, everything checked.
    segs: list of dicts(kind, k, t, index (GATHER: int32 [rows]; SUM / MEAN: rowptr), mean). resid: None or
    the tensor added to the output. proj: (P [NODES, 2H], src, dst)."""
    from aerognn import _lib as L
    from aerognn import core, functions as Fn
    s, H, dt = c.spec, c.H, c.dtype
    G = Guards()
    kinds = {"plain": L.SEG_PLAIN, "gather": L.SEG_GATHER, "sum": L.SEG_SUM, "mean": L.SEG_MEAN}
    csegs, ops = [], []
    for sg in segs:
        store = None
        if sg["kind"] in ("sum", "mean"):
            store = sg["store"] = G.alloc(rows, sg["k"], dt)
        csegs.append((kinds[sg["kind"]], sg["k"], sg["t"].stride(0), sg["t"], sg.get("index"), store))
    out = G.alloc(rows, c.out, dt, ld=out_ld, offset=out_offset)
    acts, hpre, stats = Fn._alloc_saves(s, rows, dt, torch.device(DEV), True)
    if not tiled and s.tiled_saves:  # plain row-major saves at H = 128 (a.tiled = 0)
        def plain(t):
            p = torch.empty(rows, t.shape[1], dtype=dt, device=DEV)
            for k in ("agn_mask", "agn_pre"):
                if hasattr(t, k):
                    v = getattr(t, k)
                    setattr(p, k, plain(v) if k == "agn_pre" else v)
            return p
        acts, hpre = [plain(t) for t in acts], None if hpre is None else plain(hpre)
    assert any(core.is_tiled(t) for t in acts + [hpre]) == (tiled and s.tiled_saves and (c.nlin > 1 or hpre is not None))
    acts = [G.rehome(t) for t in acts]
    hpre, stats = G.rehome(hpre), G.rehome(stats)
    P = src = dst = None
    if proj is not None:
        P, src, dst = proj
    core.mlp_forward(rows=rows, dtype=dt, hidden=H, nlin=c.nlin, act_fn=s.act, out_dim=c.out, segs=csegs,
                     wpk=s.wpk(), bias=s.biases(), ln=s.lnp(), out=out, out_ld=out_ld, proj=P, src=src, dst=dst,
                     resid=resid, acts=acts, hpre=hpre, stats=stats)
    torch.cuda.synchronize()
    assert _mode(0) == fwd_mode, (tag, "forward mode", _mode(0), fwd_mode)
    # ---- the layer-0 operand rows as the kernel read them
    for sg in segs:
        t64 = S.f64(sg["t"])
        if sg["kind"] == "plain":
            ops.append(t64)
        elif sg["kind"] == "gather":
            ops.append(t64[sg["index"].cpu().long()])
        else:
            ref, d = S.segment_ref(t64, sg["index"], sg["kind"] == "mean")
            S.check(f"{tag}stored {sg['kind']}", sg["store"], ref, d, dt, label=label)
            ops.append(S.f64(sg["store"]))
    X64 = torch.cat(ops, 1)
    assert X64.shape == (rows, c.K)
    extra = ()
    if proj is not None:
        P64 = S.f64(P)
        extra = (P64[src.cpu().long(), :H], P64[dst.cpu().long(), H:])
    A = [rows_of(t, rows) for t in acts]
    PRE = [rows_of(core._pre_of(t), rows) for t in acts] if c.act != "relu" else None
    HP = None if hpre is None else rows_of(hpre, rows)
    S.check_forward(dt, c.act, X64, c.W64, c.b64, acts=A, pres=PRE, hpre=HP, stats=stats, out=out, ln=c.ln64,
                    resid=None if resid is None else S.f64(resid), extra=extra, tag=tag, label=label)
    if not backward:
        G.check()
        return
    # ---- backward
    g = None if g_none else _randn(c.gen, rows, c.out, dt, offset=g_offset)
    g64 = torch.zeros(rows, c.out, dtype=torch.float64) if g_none else S.f64(g)
    d_g = g2t = gidx = None
    if g2:
        g2t = torch.randn(NODES, c.out, generator=c.gen).to(dt).to(DEV)
        gidx = torch.randint(0, NODES, (rows,), generator=c.gen).to(torch.int32).to(DEV)
        g64 = g64 + S.f64(g2t)[gidx.cpu().long()]
        d_g = S.U * g64.abs()
    gpre = [G.rehome(t) for t in Fn._alloc_gpre(s, rows, dt, torch.device(DEV), rowmajor=range(c.nlin))]
    dins = [G.alloc(rows, sg["k"], dt) for sg in segs]
    nblk = core.bwd_nblocks(rows)
    part = G.alloc(nblk, 2 * c.out, torch.float32) if c.ln is not None else None
    ln_rows = core.mlp_backward(rows=rows, dtype=dt, hidden=H, nlin=c.nlin, act_fn=s.act, out_dim=c.out, in_dim=c.K,
                                wtpk=s.wtpk(), acts=acts, g=g, gpre=gpre, ln_g=s.lnp()[0] if c.ln is not None else None,
                                hpre=hpre, stats=stats, g2=g2t, gidx=gidx,
                                din=[(sg["k"], d, din_resid) for sg, d in zip(segs, dins)], ln_partial=part)
    torch.cuda.synchronize()
    assert _mode(1) == bwd_mode, (tag, "backward mode", _mode(1), bwd_mode)
    assert ln_rows == nblk
    if g_none:  # a zero gradient: every output is exactly zero
        for t in gpre + dins + ([part] if part is not None else []):
            assert bool((t == 0).all()), tag
        G.check()
        return
    S.check_backward(dt, c.act, c.W64, g64, acts=A, pres=PRE, hpre=HP, stats=stats,
                     ln_g=None if c.ln64 is None else c.ln64[0], gpre=gpre, din=[(d, din_resid) for d in dins],
                     lnp=None if part is None else S.f64(part).sum(0), d_g=d_g, tag=tag, label=label)
    if wgrad:
        in0 = []
        for sg in segs:  # contiguous operands: agn_wgrad is not the kernel under test here
            if sg["kind"] == "plain":
                in0.append(sg["t"].contiguous())
            elif sg["kind"] == "gather":
                in0.append((sg["t"].contiguous(), sg["index"]))
            else:
                in0.append(sg["store"])
        grads = Fn._chain_param_grads(s, gpre, in0, acts, part, ln_rows)
        torch.cuda.synchronize()
        ins, i = [X64] + [S.f64(a) for a in A], 0
        for l in range(c.nlin):
            G64 = S.f64(gpre[l])
            S.check_bar(f"{tag}dW{l}", grads[i], G64.T @ ins[l], GPAR)
            i += 1
            if c.b[l] is not None:
                S.check_bar(f"{tag}db{l}", grads[i], G64.sum(0), GPAR)
                i += 1
        assert len(grads) == i + (2 if c.ln is not None else 0)
    G.check()


def _plain(c, rows, k=None, ld=None, offset=0):
    k = k or c.H
    return {"kind": "plain", "k": k, "t": _randn(c.gen, rows, k, c.dtype, ld=ld, offset=offset)}


def _gather(c, rows, k=None, ld=None):
    k = k or c.H
    idx = torch.randint(0, NODES, (rows,), generator=c.gen).to(torch.int32).to(DEV)
    return {"kind": "gather", "k": k, "t": _randn(c.gen, NODES, k, c.dtype, ld=ld), "index": idx}


def _label(H, dtype):
    return f"{IDS[DTYPES.index(dtype)]} H={H}"


def _layouts(H):
    return (True, False) if H == 128 else (True,)


def _bwd_mode(c, aligned=True):
    if aligned and c.out == c.H:
        return M_VEC
    if aligned and c.out <= 32 and c.ln is None:
        return M_NOUT
    return M_GEN


pm = pytest.mark.parametrize


def sweep(f):
    return pm("dtype", DTYPES, ids=IDS)(pm("H", HS)(f))


# ------------------------------------------------------------------------------ the cases (a) to (m)
@sweep
def test_a_vec_residual(H, dtype):
    """(a) M_VEC: PLAIN K = H, nlin 3, out H, LayerNorm, resid = the input, din_resid."""
    for tiled in _layouts(H):
        c = Chain(H, dtype, H, 3, H, True, seed=10 + H)
        for rows in ROWS:
            x = _plain(c, rows)
            run_chain(c, rows, [x], fwd_mode=M_VEC, bwd_mode=M_VEC, resid=x["t"], tiled=tiled, din_resid=True,
                      wgrad=True, label=_label(H, dtype), tag=f"a rows {rows} tiled {tiled}: ")


@pm("mean", [False, True], ids=["sum", "mean"])
@sweep
def test_b_vec_segment_sum(H, dtype, mean):
    """(b) M_VEC: PLAIN H + SUM (MEAN) H with store; the stored sums against float64 index_add."""
    for tiled in _layouts(H):
        c = Chain(H, dtype, 2 * H, 3, H, True, seed=20 + H)
        for rows in ROWS:
            rp = _rowptr(rows)
            e = _randn(c.gen, int(rp[-1]), H, dtype)
            seg = {"kind": "mean" if mean else "sum", "k": H, "t": e, "index": rp.to(DEV)}
            x = _plain(c, rows)
            run_chain(c, rows, [x, seg], fwd_mode=M_VEC, bwd_mode=M_VEC, resid=x["t"], tiled=tiled,
                      label=_label(H, dtype), tag=f"b rows {rows} tiled {tiled}: ")


@sweep
def test_c_vec_concat_edge(H, dtype):
    """(c) M_VEC: PLAIN e + GATHER x[src] + GATHER x[dst], all H wide, repeated indices."""
    for tiled in _layouts(H):
        c = Chain(H, dtype, 3 * H, 3, H, True, seed=30 + H)
        for rows in ROWS:
            e = _plain(c, rows)
            xs = _gather(c, rows)
            xd = dict(xs, index=torch.randint(0, NODES, (rows,), generator=c.gen).to(torch.int32).to(DEV))
            run_chain(c, rows, [e, xs, xd], fwd_mode=M_VEC, bwd_mode=M_VEC, resid=e["t"], tiled=tiled,
                      label=_label(H, dtype), tag=f"c rows {rows} tiled {tiled}: ")


@sweep
def test_d_gen_narrow_last_segment(H, dtype):
    """(d) M_GEN: the concat chain with the last segment 5 wide."""
    for tiled in _layouts(H):
        c = Chain(H, dtype, 2 * H + 5, 3, H, True, seed=40 + H)
        for rows in ROWS:
            e = _plain(c, rows)
            run_chain(c, rows, [e, _gather(c, rows), _gather(c, rows, k=5)], fwd_mode=M_GEN, bwd_mode=M_VEC,
                      resid=e["t"], tiled=tiled, wgrad=True, label=_label(H, dtype),
                      tag=f"d rows {rows} tiled {tiled}: ")


@sweep
def test_e_gen_strides_and_alignment(H, dtype):
    """(e) M_GEN: case a with out_ld = H + 4 (input and residual on the same stride), and case a on views
    offset by one element (input = residual, output and gradient: rows not 16-B aligned)."""
    for tiled in _layouts(H):
        c = Chain(H, dtype, H, 3, H, True, seed=50 + H)
        for rows in ROWS:
            x = _plain(c, rows, ld=H + 4)
            run_chain(c, rows, [x], fwd_mode=M_GEN, bwd_mode=M_VEC, resid=x["t"], out_ld=H + 4, tiled=tiled,
                      din_resid=True, label=_label(H, dtype), tag=f"e out_ld rows {rows} tiled {tiled}: ")
            x = _plain(c, rows, offset=1)
            run_chain(c, rows, [x], fwd_mode=M_GEN, bwd_mode=M_GEN, resid=x["t"], out_offset=1, g_offset=1, tiled=tiled,
                      din_resid=True, label=_label(H, dtype), tag=f"e offset rows {rows} tiled {tiled}: ")


@sweep
def test_f_gen_narrow_layernorm(H, dtype):
    """(f) M_GEN: out = H - 7 and out = 4 with LayerNorm (feat_of(i, h) < outd in the LayerNorm sums)."""
    for out in (H - 7, 4):
        c = Chain(H, dtype, H, 3, out, True, seed=60 + H + out)
        for rows in ROWS:
            run_chain(c, rows, [_plain(c, rows)], fwd_mode=M_GEN, bwd_mode=M_GEN, label=_label(H, dtype),
                      tag=f"f out {out} rows {rows}: ")


@pm("K", [1, 6, 16])
@sweep
def test_g_nin(H, dtype, K):
    """(g) M_NIN: K in {1, 6, 16}, PLAIN with ld > K and GATHER, LayerNorm, out H."""
    for tiled in _layouts(H):
        c = Chain(H, dtype, K, 3, H, True, seed=70 + H + K)
        for rows in ROWS:
            run_chain(c, rows, [_plain(c, rows, k=K, ld=K + 3)], fwd_mode=M_NIN, bwd_mode=M_VEC, tiled=tiled, wgrad=True,
                      label=_label(H, dtype), tag=f"g plain K {K} rows {rows} tiled {tiled}: ")
            run_chain(c, rows, [_gather(c, rows, k=K, ld=K + 3)], fwd_mode=M_NIN, bwd_mode=M_VEC, tiled=tiled, wgrad=True,
                      label=_label(H, dtype), tag=f"g gather K {K} rows {rows} tiled {tiled}: ")


@pm("nlin", [3, 4])
@sweep
def test_h_nout(H, dtype, nlin):
    """(h) M_NOUT: K = H, out in {1, 4, 32}, no LayerNorm (out = 32 at H = 32 is H wide: M_VEC)."""
    for out in (1, 4, 32):
        for tiled in _layouts(H):
            c = Chain(H, dtype, H, nlin, out, False, seed=80 + H + out + nlin)
            mode = M_VEC if out == H else M_NOUT
            for rows in ROWS:
                run_chain(c, rows, [_plain(c, rows)], fwd_mode=mode, bwd_mode=mode, tiled=tiled, wgrad=True,
                          label=_label(H, dtype), tag=f"h out {out} rows {rows} tiled {tiled}: ")


@sweep
def test_i_single_linear(H, dtype):
    """(i) nlin = 1 forward: out = H (with LayerNorm), and out = 2 H with bias (ngrp = 2: the sum trick's
    projections off the fast path)."""
    for out, ln in ((H, True), (2 * H, False)):
        for tiled in (_layouts(H) if ln else (True,)):  # (out = 2 H has no saves: one layout)
            c = Chain(H, dtype, H, 1, out, ln, seed=90 + H + out)
            for rows in ROWS:
                run_chain(c, rows, [_plain(c, rows)], fwd_mode=M_VEC, backward=False, tiled=tiled,
                          label=_label(H, dtype), tag=f"i out {out} rows {rows} tiled {tiled}: ")


@sweep
def test_j_proj_prologue(H, dtype):
    """(j) the proj prologue: P [N][2H] gathered by src / dst, PLAIN e, nlin 3, LayerNorm, resid = e;
    backward with din_resid, gpre[0] checked (the operand of dP_s / dP_d and dW_e)."""
    for tiled in _layouts(H):
        c = Chain(H, dtype, H, 3, H, True, bias0=False, seed=100 + H)
        for rows in ROWS:
            P = _randn(c.gen, NODES, 2 * H, dtype)
            src, dst = (torch.randint(0, NODES, (rows,), generator=c.gen).to(torch.int32).to(DEV) for _ in range(2))
            e = _plain(c, rows)
            run_chain(c, rows, [e], fwd_mode=M_VEC, bwd_mode=M_VEC, resid=e["t"], proj=(P, src, dst), tiled=tiled,
                      din_resid=True, label=_label(H, dtype), tag=f"j rows {rows} tiled {tiled}: ")


@sweep
def test_k_gathered_gradient_add(H, dtype):
    """(k) backward with g2 / gidx: g + g2[gidx] ahead of the LayerNorm backward and in din_resid."""
    for tiled in _layouts(H):
        c = Chain(H, dtype, H, 3, H, True, seed=110 + H)
        for rows in ROWS:
            x = _plain(c, rows)
            run_chain(c, rows, [x], fwd_mode=M_VEC, bwd_mode=M_VEC, resid=x["t"], tiled=tiled, g2=True, din_resid=True,
                      label=_label(H, dtype), tag=f"k rows {rows} tiled {tiled}: ")
    c = Chain(H, dtype, H, 3, H - 7, True, seed=111 + H)  # the masked loads of g2
    for rows in ROWS:
        run_chain(c, rows, [_plain(c, rows)], fwd_mode=M_GEN, bwd_mode=M_GEN, g2=True, label=_label(H, dtype),
                  tag=f"k out H-7 rows {rows}: ")


@sweep
def test_l_zero_gradient(H, dtype):
    """(l) backward with g = None: every output is exactly zero."""
    for out, ln in ((H, True), (H - 7, True), (4, False)):
        for tiled in _layouts(H):
            c = Chain(H, dtype, H, 3, out, ln, seed=120 + H + out)
            if not c.spec.tiled_saves and not tiled:
                continue  # (out = H - 7 with LayerNorm saves row-major only: one layout)
            for rows in ROWS:
                x = _plain(c, rows)
                run_chain(c, rows, [x], fwd_mode=M_VEC if out == H else (M_GEN if ln else M_NOUT),
                          bwd_mode=_bwd_mode(c), tiled=tiled, g_none=True, din_resid=out == H, label=_label(H, dtype),
                          tag=f"l out {out} rows {rows} tiled {tiled}: ")


@pm("act", ["gelu", "silu", "tanh"])
@sweep
def test_m_other_activations(H, dtype, act):
    """(m) GACT: cases a, f (out = H - 7) and g (K = 6) under gelu / silu / tanh; pre[l] is the rounded
    Linear output, act[l] the rounded activation of the stored pre[l]."""
    lab = _label(H, dtype)
    for tiled in _layouts(H):
        c = Chain(H, dtype, H, 3, H, True, act=act, seed=130 + H)
        for rows in ROWS:
            x = _plain(c, rows)
            run_chain(c, rows, [x], fwd_mode=M_VEC, bwd_mode=M_VEC, resid=x["t"], tiled=tiled, din_resid=True, wgrad=True,
                      label=lab, tag=f"m/a {act} rows {rows} tiled {tiled}: ")
        c = Chain(H, dtype, 6, 3, H, True, act=act, seed=131 + H)
        for rows in ROWS:
            run_chain(c, rows, [_plain(c, rows, k=6, ld=9)], fwd_mode=M_NIN, bwd_mode=M_VEC, tiled=tiled, wgrad=True,
                      label=lab, tag=f"m/g {act} rows {rows} tiled {tiled}: ")
    c = Chain(H, dtype, H, 3, H - 7, True, act=act, seed=132 + H)
    for rows in ROWS:
        run_chain(c, rows, [_plain(c, rows)], fwd_mode=M_GEN, bwd_mode=M_GEN, wgrad=True, label=lab,
                  tag=f"m/f {act} rows {rows}: ")


@pytest.fixture(scope="module", autouse=True)
def _worst_ratio_table():
    """Prints, after the module's last test, the table of DESIGN.md §4 "save-chain": the worst ratio per
    type and hidden width over the cases that ran (a report, not a check: each case asserts its own)."""
    yield
    for k in sorted(S.WORST):
        print(f"save-chain worst ratio {k}: {S.WORST[k]:.3f}")


# ------------------------------------------------------------------------------ module level, H = 64
HM = 64
MLP_K = [1, 16, 17, HM - 1, HM, HM + 1, 2 * HM, 2 * HM + 5, 3 * HM]
MLP_CFG = [(0, HM, True), (1, 4, False), (2, HM, True), (2, HM - 7, True)]
CFG_IDS = ["nh0-outH-ln", "nh1-out4", "nh2-outH-ln", "nh2-outH-7-ln"]


def _gate(what, got, ref, tol):
    r, mx = rel_l2(got.detach().cpu(), ref), max_rel(got.detach().cpu(), ref)
    print(f"{what}: rel-L2 {r:.2e}, max-elem {mx:.2e} (gate {tol:.0e})")
    assert r <= tol and mx <= tol, (what, r, mx)


def _run(model, x, gy):
    model.zero_grad(set_to_none=True)
    xd = x.to(DEV).requires_grad_(True)
    y = model(xd)
    y.backward(gy.to(DEV))
    return y.detach(), xd.grad, {k: p.grad for k, p in model.named_parameters()}


@pm("cfg", MLP_CFG, ids=CFG_IDS)
@pm("K", MLP_K)
def test_mlp_h64_fp32(K, cfg):
    """models.mlp.MLP at H = 64 against the float64 formula (kink-free rows) at 1e-5 / 1e-5 / 5e-5."""
    from models.mlp import MLP
    nh, out, ln = cfg
    gen = torch.Generator().manual_seed(1000 * K + 10 * nh + out)
    torch.manual_seed(13 * K + nh)
    model = MLP(K, HM, out, nh, use_layer_norm=ln)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model = model.to(DEV)
    for rows in ROWS:
        x = kink_free_rows(sd, torch.randn(rows, K, generator=gen), gen)
        gy = torch.randn(rows, out, generator=gen)
        ry, rgx, rgp = ref_chain(sd, x, "relu", gy)
        y, gx, gp = _run(model, x, gy)
        _gate(f"rows {rows} y", y, ry, FWD)
        _gate(f"rows {rows} gx", gx, rgx, GIN)
        for k, g in gp.items():
            _gate(f"rows {rows} gp:{k}", g, rgp[k], GPAR)


@pm("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pm("cfg", MLP_CFG, ids=CFG_IDS)
@pm("K", MLP_K)
def test_mlp_h64_16bit(K, cfg, dtype):
    """The same modules with 16-bit parameters: a smoke test of the autograd wiring (the sharp 16-bit
    checks are the save-chain cases above). Reference: the float64 formula on the rounded values; gate:
    rel-L2 <= max(2e-2, 2 x the error of torch's own 16-bit CPU evaluation of the case), test_golden_16bit's
    rule for its LayerNorm chains."""
    from models.mlp import MLP
    nh, out, ln = cfg
    gen = torch.Generator().manual_seed(2000 * K + 10 * nh + out)
    torch.manual_seed(17 * K + nh)
    model = MLP(K, HM, out, nh, use_layer_norm=ln).to(dtype)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model = model.to(DEV)
    for rows in ROWS:
        x, gy = torch.randn(rows, K, generator=gen).to(dtype), torch.randn(rows, out, generator=gen).to(dtype)
        ry, rgx, rgp = ref_chain(sd, x, "relu", gy)
        ty, tgx, tgp = torch_16bit(sd, x, "relu", gy)
        y, gx, gp = _run(model, x, gy)
        assert y.dtype == dtype and gx.dtype == dtype
        for what, got, own, ref in [("y", y, ty, ry), ("gx", gx, tgx, rgx)] + [("gp:" + k, g, tgp[k], rgp[k])
                                                                               for k, g in gp.items()]:
            r, o = rel_l2(got.float().cpu(), ref), rel_l2(own.float(), ref)
            print(f"K {K} rows {rows} {what}: rel-L2 {r:.3e} (torch 16-bit {o:.3e})")
            assert r <= max(B16, 2 * o), (what, rows, r, o)


def _graph(gen, N=70, E=300):
    """About 70 nodes and 300 edges: node 5 isolated (neither sends nor receives), node 0 a hub that
    receives 48 edges (more than a 32-row tile)."""
    src = torch.randint(0, N, (E,), generator=gen)
    dst = torch.randint(0, N, (E,), generator=gen)
    dst[:48] = 0
    src[src == 5] = 6
    dst[dst == 5] = 7
    return torch.stack([src, dst])


@pm("nh", [1, 2])
@pm("trick,agg", [(True, "add"), (False, "add"), (False, "mean")], ids=["sum-add", "cat-add", "cat-mean"])
def test_layer_h64_fp32(trick, agg, nh):
    """MeshGraphNetLayer(64) in fp32 against oracle.refcpu in float64 on kink-free inputs
    (tests/kinkfree.py) at the project's bars."""
    from kinkfree import kink_free
    from models.mgnLayer import MeshGraphNetLayer
    from oracle import refcpu as R
    gen = torch.Generator().manual_seed(31 + nh)
    torch.manual_seed(7 + nh)
    layer = MeshGraphNetLayer(HM, HM, HM, nh, nh, "relu", True, agg, trick)
    ei = _graph(gen)
    N, E = 70, ei.shape[1]
    cfg = {"do_concat_trick": trick, "n_hid_edge": nh, "n_hid_node": nh, "aggregation": agg}
    p64 = {"L." + k: v.detach().double().requires_grad_(True) for k, v in layer.state_dict().items()}
    x, e = torch.randn(N, HM, generator=gen), torch.randn(E, HM, generator=gen)
    kink_free(lambda xx, ee: R.gmp_layer(p64, "L", xx, ee, ei, cfg), x, e, gen)
    gx, ge = torch.randn(N, HM, generator=gen), torch.randn(E, HM, generator=gen)
    x64, e64 = x.double().requires_grad_(True), e.double().requires_grad_(True)
    rx, re = R.gmp_layer(p64, "L", x64, e64, ei, cfg)
    torch.autograd.backward([rx, re], [gx.double(), ge.double()])
    layer = layer.to(DEV)
    xd, ed = x.to(DEV).requires_grad_(True), e.to(DEV).requires_grad_(True)
    xo, eo = layer(xd, ed, ei.to(DEV))
    torch.autograd.backward([xo, eo], [gx.to(DEV), ge.to(DEV)])
    assert not bool(xo[5].eq(xd[5]).all())  # (the node chain still updates the isolated node)
    _gate("x'", xo, rx.detach(), FWD)
    _gate("e'", eo, re.detach(), FWD)
    _gate("dx", xd.grad, x64.grad, GIN)
    _gate("de", ed.grad, e64.grad, GIN)
    for k, p in layer.named_parameters():
        _gate("gp:" + k, p.grad, p64["L." + k].grad, GPAR)
