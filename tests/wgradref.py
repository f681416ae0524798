"""Test infrastructure for the weight-gradient kernels (csrc/dw.hip: agn_wgrad, agn_wgrad_reduce,
agn_colsum; csrc/mlp.hip: agn_reduce_partials), shared by tests/test_gpu_wgrad.py and its CPU twin
tests/test_wgradref_cpu.py.

Two comparison modes.

Exact: the operands are integers in [-7, 7] (representable in fp32, bf16 and fp16). Every product is
an integer of magnitude <= 49 and every partial sum one of magnitude <= 49 * rows < 2^24, so each
fp32 addition is exact and dW = G^T X, db = colsum(G) come out the same in ANY summation order,
split count and MFMA association. The result must equal the int64 reference with no tolerance, and
everything a kernel must not read (pad rows of tiled buffers, columns outside a strided window,
table rows that xidx never names, slab entries nobody wrote) holds NaN, so a leak turns the output
non-finite; everything it must not write holds a sentinel bit pattern that is checked afterwards.

Rounded: randn operands against the float64 product with the elementwise accumulation bound
|got - ref| <= 2 (rows + nsplit + 16) 2^-24 S, S = |G|^T |X| (rounded_failures): this one catches an
accumulation in less than fp32, which the exact mode cannot see.

emulate_wgrad is a CPU stand-in for the kernel with injectable mistakes; the CPU test shows that the
comparison functions below reject each of them.
"""
import ctypes as C
import math

import torch

H = 128
NAN = float("nan")
SENTINEL = 0x7FC5A5A5  # a quiet NaN with a payload: compared as bits
RED_G = 8              # thread groups of wgrad_reduce_kernel / colsum_stage2 (csrc/dw.hip)
BUGS = ("drop_last_row", "repeat_stage_row", "swap_columns", "transpose_block", "leak_pad_row", "write_past_k")


# --------------------------------------------------------------------------- operands and layouts
def int_operand(rows, cols, seed, dtype=torch.float32):
    """[rows, cols] of integers drawn uniformly from [-7, 7] (CPU)."""
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(-7, 8, (rows, cols), generator=gen).to(dtype)


def encode_tiled(x, fill=NAN):
    """Row-major [rows, 128] (fp32 / bf16 / fp16) -> the AGN_TILED buffer of include/aerognn.h, rows
    padded to 32 with `fill`, tagged like core.tiled_empty; the inverse of maskmatched.decode_tiled.
    Unit (row r, i, half h) sits at 16-B index ((r / 32) U + i) 64 + r % 32 + 32 h; 16-bit units hold
    features 16i+4h+{0..3} | 16i+8+4h+{0..3} (U = 8), fp32 units features 8i+4h+{0..3} (U = 16)."""
    rows, width = x.shape
    assert width == H and x.dtype in (torch.float32, torch.bfloat16, torch.float16)
    rp = (rows + 31) // 32 * 32
    xp = torch.full((rp, H), fill, dtype=x.dtype, device=x.device)
    xp[:rows] = x
    if x.dtype == torch.float32:
        # feature 8i + 4h + e of row (t, c) -> [t][i][h][c][e]
        t = xp.reshape(-1, 32, 16, 2, 4).permute(0, 2, 3, 1, 4)
    else:
        # feature 16i + 8s + 4h + e of row (t, c) -> [t][i][h][c][4s + e]
        t = xp.reshape(-1, 32, 8, 2, 2, 4).permute(0, 2, 4, 1, 3, 5)
    t = t.contiguous().reshape(rp, H)
    t.agn_tiled = True
    t.agn_rows = rows
    return t


def strided(x, pad, off, poison=NAN):
    """x as the column window [:, off:off+cols] of a [rows, cols + off + pad] buffer whose other
    columns hold `poison`: row stride cols + off + pad, base `off` elements into the allocation."""
    rows, cols = x.shape
    buf = torch.full((rows, cols + off + pad), poison, dtype=x.dtype, device=x.device)
    buf[:, off:off + cols] = x
    return buf[:, off:off + cols]


def _sentinel(shape, device, sentinel=SENTINEL):
    return torch.full(shape, sentinel, dtype=torch.int32, device=device).view(torch.float32)


def window(M, K, ldw, col_off, sentinel=SENTINEL, device="cpu"):
    """(buf, view): an fp32 [M, K] dW view at rows 1..M, columns col_off.. of a sentinel-filled
    [M + 2][ldw] buffer."""
    assert ldw >= col_off + K
    buf = _sentinel((M + 2, ldw), device, sentinel)
    buf.agn_window = (slice(1, M + 1), slice(col_off, col_off + K))
    buf.agn_sentinel = sentinel
    return buf, buf[1:M + 1, col_off:col_off + K]


def vec_window(M, before=3, after=5, sentinel=SENTINEL, device="cpu"):
    """(buf, view): an fp32 [M] db view inside a longer sentinel-filled vector."""
    buf = _sentinel((before + M + after,), device, sentinel)
    buf.agn_window = (slice(before, before + M),)
    buf.agn_sentinel = sentinel
    return buf, buf[before:before + M]


def outside_untouched(buf):
    """Every element of a window / vec_window buffer outside its view still holds the sentinel bits."""
    out = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    out[buf.agn_window] = False
    return bool((buf.view(torch.int32)[out] == buf.agn_sentinel).all())


def all_sentinel(t, sentinel=SENTINEL):
    """Nothing wrote t (a view of a sentinel buffer, or the whole buffer)."""
    return bool((t.contiguous().view(torch.int32) == sentinel).all())


# --------------------------------------------------------------------------- references
def exact_ref(G, X, xidx=None):
    """(int64 G^T X[xidx], int64 colsum(G)) of integer-valued operands, on the CPU."""
    g, x = G.detach().cpu().long(), X.detach().cpu().long()
    if xidx is not None:
        x = x[xidx.detach().cpu().long()]
    return g.t() @ x, g.sum(0)


def bound_ref(G, X, rows, nsplit):
    """(ref, S, bound): the float64 product G^T X, S = |G|^T |X| and the elementwise bound
    2 (rows + nsplit + 16) 2^-24 S of a length-`rows` fp32 accumulation plus the split reduction
    (16-bit products are exact in fp32, fp32 products add one rounding; the factor 2 covers the
    unspecified association inside an MFMA)."""
    g, x = G.detach().cpu().double(), X.detach().cpu().double()
    ref, S = g.t() @ x, g.abs().t() @ x.abs()
    return ref, S, 2.0 * (rows + nsplit + 16) * 2.0 ** -24 * S


def reduce_order(partials):
    """fp32 emulation of wgrad_reduce_kernel / colsum_stage2 over partials [n, ...] (CPU fp32):
    group g = 0..7 adds entries g, g + 8, ... in ascending order from 0.f, then the eight group sums
    are added as ((p0 + p1) + p2) + ..."""
    p = partials.detach().cpu()
    assert p.dtype == torch.float32
    parts = []
    for g in range(RED_G):
        s = torch.zeros(p.shape[1:], dtype=torch.float32)
        for sp in range(g, p.shape[0], RED_G):
            s = s + p[sp]
        parts.append(s)
    r = parts[0]
    for g in range(1, RED_G):
        r = r + parts[g]
    return r


def partials_order(p):
    """fp32 emulation of reduce_partials_kernel over p [nw, n]: w = 0..nw-1 in order from 0.f."""
    p = p.detach().cpu()
    assert p.dtype == torch.float32
    s = torch.zeros(p.shape[1:], dtype=torch.float32)
    for w in range(p.shape[0]):
        s = s + p[w]
    return s


def colsum_order(p, scratch_rows):
    """fp32 emulation of agn_colsum over p [nw, n]: colsum_stage1 adds the rows of each chunk of
    ceil(nw / scratch_rows) rows in ascending order from 0.f, colsum_stage2 combines the chunk sums in
    reduce_order. nw == 0 gives zeros."""
    p = p.detach().cpu()
    nw = p.shape[0]
    if nw == 0:
        return torch.zeros(p.shape[1:], dtype=torch.float32)
    chunk = (nw + scratch_rows - 1) // scratch_rows
    return reduce_order(torch.stack([partials_order(p[r0:r0 + chunk]) for r0 in range(0, nw, chunk)]))


# --------------------------------------------------------------------------- comparisons
def exact_failures(name, got, ref):
    """Why fp32 `got` is not exactly the int64 `ref` (a list of strings, empty when it is)."""
    got = got.detach().cpu()
    if not bool(torch.isfinite(got).all()):
        return [f"{name}: {int((~torch.isfinite(got)).sum())} non-finite entries (a poison region leaked)"]
    if not torch.equal(got, got.round()):
        return [f"{name}: non-integer entries"]
    if not torch.equal(got.long(), ref):
        bad = (got.long() != ref).nonzero()
        return [f"{name}: {bad.shape[0]} entries differ from the int64 reference, first at {bad[0].tolist()}"]
    return []


def case_failures(name, dw, refw, db=None, refb=None, dw_buf=None, db_buf=None):
    """All exact-mode checks of one desc: dW, db, and nothing written outside their views."""
    f = exact_failures(f"{name} dW", dw, refw)
    if db is not None:
        f += exact_failures(f"{name} db", db, refb)
    if dw_buf is not None and not outside_untouched(dw_buf):
        f.append(f"{name}: a write outside the dW view")
    if db_buf is not None and not outside_untouched(db_buf):
        f.append(f"{name}: a write outside the db view")
    return f


def rounded_failures(name, got, ref, bound):
    """(failures, worst ratio |got - ref| / bound) of the rounded mode: the elementwise bound and the
    rel-L2 <= 1e-6 gate of tests/test_gpu_kernels.py."""
    got = got.detach().cpu().double()
    if not bool(torch.isfinite(got).all()):
        return [f"{name}: non-finite entries"], math.inf
    err = (got - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    f = []
    if ratio > 1.0:
        f.append(f"{name}: worst |got - ref| / bound = {ratio:.3f} > 1")
    rel = float((got - ref).norm() / ref.norm().clamp_min(1e-300))
    if rel > 1e-6:
        f.append(f"{name}: rel-L2 {rel:.3e} > 1e-6")
    return f, ratio


# --------------------------------------------------------------------------- CPU stand-in
def emulate_wgrad(G, X, dw, db=None, bug=None, pad_fill=NAN):
    """dw[:] = G^T X, db[:] = colsum(G) in fp32 on the CPU, written into the given views, with one
    injectable mistake (BUGS):
      drop_last_row     the last row is left out of the sums (a stage tail one row short)
      repeat_stage_row  row 64, the first of the second 64-row stage, is added twice
      swap_columns      output columns 0 and K - 1 swapped
      transpose_block   the leading 32 x 32 sub-block of dW transposed (a swapped MFMA operand pair)
      leak_pad_row      one pad row (holding pad_fill) joins the sums
      write_past_k      column K of every dW row is written as well
      lowprec           the running sum is rounded to bf16 after every 64-row stage (rounded mode)"""
    g, x = G.float(), X.float()
    rows, M, K = g.shape[0], g.shape[1], x.shape[1]
    if bug == "drop_last_row":
        g, x = g[:-1], x[:-1]
    elif bug == "repeat_stage_row":
        assert rows > 64
        g, x = torch.cat([g, g[64:65]]), torch.cat([x, x[64:65]])
    elif bug == "leak_pad_row":
        assert rows % 32
        g, x = torch.cat([g, torch.full((1, M), pad_fill)]), torch.cat([x, torch.full((1, K), pad_fill)])
    if bug == "lowprec":
        W = torch.zeros(M, K)
        for r0 in range(0, rows, 64):
            W = (W + g[r0:r0 + 64].t() @ x[r0:r0 + 64]).bfloat16().float()
    else:
        W = g.t() @ x
    b = g.sum(0)
    if bug == "swap_columns":
        assert K >= 2
        W[:, [0, K - 1]] = W[:, [K - 1, 0]]
    elif bug == "transpose_block":
        assert M >= 32 and K >= 32
        W[:32, :32] = W[:32, :32].t().clone()
    if bug == "write_past_k":
        torch.as_strided(dw, (M, K + 1), dw.stride(), dw.storage_offset())[:, K] = W[:, 0]
    dw.copy_(W)
    if db is not None:
        db.copy_(b)


# --------------------------------------------------------------------------- direct launch
class Desc:
    """One agn_wgrad_desc: G [rows, M], X [rows, K] (or a table gathered by xidx), the dW view and db.
    `over` overrides struct fields (m, k, rows, g_tiled, x_tiled, nsplit) for the argument checks."""

    def __init__(self, G, X, dw, db=None, xidx=None, **over):
        self.G, self.X, self.dw, self.db, self.xidx, self.over = G, X, dw, db, xidx, over


def launch(descs, dtype, nsplit, n=None, plan=False):
    """agn_wgrad on `descs` with the forced split count `nsplit` (0: each desc's own, from
    agn_wgrad_plan when `plan`, else from its override or 1). Slabs are sized as WGrad.run sizes them
    and NaN-filled, so an entry that is summed but never written shows. Returns (rc, batch, slabs);
    keep `slabs` alive until the stream has run. dtype: a torch dtype or an AGN_* code; n: b.n."""
    from aerognn import _lib as L
    from aerognn import core
    lib = L.lib()
    b = L.WgradBatch()
    b.n = len(descs) if n is None else n
    for j, d in enumerate(descs):
        f = dict(m=d.G.shape[1], k=d.X.shape[1], rows=core.logical_rows(d.G), g_tiled=int(core.is_tiled(d.G)),
                 x_tiled=int(core.is_tiled(d.X)), nsplit=0)
        f.update(d.over)
        b.d[j] = L.WgradDesc(L.ptr(d.G), L.ptr(d.X), d.G.stride(0), d.X.stride(0), f["m"], f["k"], f["rows"],
                             d.dw.stride(0), None, None, L.ptr(d.dw), L.ptr(d.db), f["g_tiled"], f["x_tiled"],
                             f["nsplit"], 0, L.ptr(d.xidx))
    if plan:
        L.check(lib.agn_wgrad_plan(C.byref(b)), "wgrad_plan")
    slabs = []
    for j, d in enumerate(descs):
        ns = max(1, nsplit if nsplit > 0 else b.d[j].nsplit)
        m, k = max(1, b.d[j].m), max(1, b.d[j].k)
        dwp = torch.full((int(lib.agn_wgrad_partial_floats(m, k, ns)),), NAN, dtype=torch.float32, device=d.dw.device)
        b.d[j].dw_partial = L.ptr(dwp)
        slabs.append(dwp)
        if d.db is not None:
            dbp = torch.full((ns * ((m + 127) // 128) * 128,), NAN, dtype=torch.float32, device=d.dw.device)
            b.d[j].db_partial = L.ptr(dbp)
            slabs.append(dbp)
    code = dtype if isinstance(dtype, int) else core.dt_code(dtype)
    rc = lib.agn_wgrad(C.byref(b), code, nsplit, core.stream())
    return rc, b, slabs
