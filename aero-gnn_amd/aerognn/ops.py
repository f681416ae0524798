"""torch.ops.aerognn.* — libaerognn's row-grouping kernels as registered PyTorch operators
(VERDICT r1 item 9).

The reference reaches these operations through third-party Python ops: torch_scatter's
scatter_add / scatter_mean / scatter_max along dim 0 (mgnLayer.py:144,146, bsms_mgn.py:265,270,
283) and torch_geometric's global pools (poolmgn.py:132-141). Registered here with
torch.library, they have a schema, fake (meta) kernels for shape propagation under
torch.compile / FakeTensorMode, and autograd formulas that are themselves torch.ops.aerognn ops:

  scatter_sum(src [n,k], index [n], dim_size, mean=False) -> [dim_size, k]
      out[r] = sum (or mean) of src[i] over index[i] == r, in increasing i (torch_scatter's CPU
      order; empty groups give 0). Grouping: agn_radix_sort_u64 + agn_row_ptr; sum:
      agn_segment_sum. Backward: gather_rows (mean: divided by the group size).
  group_ptr(index [n], dim_size) -> int32 [dim_size + 1] group offsets (radix sort + agn_row_ptr).
  gather_rows(src [m,k], index [n], rowptr=None) -> [n, k]
      out[i] = src[index[i]] (/ group size of index[i] when rowptr is given): agn_gather_rows.
      Backward: scatter_sum.
  scatter_max(src [n,k], index [n], dim_size) -> (out [dim_size,k], argmax [dim_size,k] int64)
      per column maximum and the first row attaining it (NaN wins, as in torch's max); empty
      groups give 0 and argmax = n (torch_scatter's convention): agn_segment_max. Backward:
      agn_segment_max_backward (gradient to the argmax row only).
  edge_features(pos [N,d], edge_index [2,E], mean=None, std=None) -> [E, d+1]
      [pos[dst] - pos[src], |.|] (dataset.py:52-62), optionally normalised: agn_edge_features.
  fourier_embed(x [n,k], d, freq_start, freq_len, with_input=True) -> [n, k * with_input + 2 * d * freq_len]
      [x | cos(f_i x_j), sin(f_i x_j)] of the first d columns, f_i = 2^(freq_start + i) pi
      (fouriermgn.py:111-151, :167-170): agn_fourier_embed. Backward: fourier_embed_backward
      (agn_fourier_embed_bwd, the trig recomputed from x).
  eval_sums(pred [n,f], y [n,f], mean [f], std [f], gptr int32 [G+1]) -> float64 [G, 2, f, 6]
      per graph, scale (normalised, physical) and feature: sum |d|, sum d^2, sum |t|, count of
      |t| > 1e-8, sum |d/t|, sum (d/t)^2 (inference.py:76-126, :337-350, :395-413): agn_eval_sums.
  aero_forces(pressure [n], shear [n,dim], normals [n,dim], pos?, areas?, edge_index?, gptr, center,
              length_scale=1e-2) -> (float64 [G, 4, 3] = sum F, sum M, sum |F|, sum |M|; areas float64 [n])
      surface integration of utils.py:385-448 / :451-559 with either the given element areas or
      the node areas of utils.py:510-520 from the mesh: agn_aero_forces. No autograd (evaluation).
  surface_forces(pos? [N,3], offsets? int64 [C+1], conn int64 [nconn] or [C,k], fields [N,4] x 0..4, mean?, std?,
                 cgptr int32 [G+1], want_cells=False)
      -> (float64 [G, nset, 2, 3] = sum F, sum |F|; areas float64 [C]; normals float64 [C, 3]; cells [nset, C, 4])
      cell areas, cell normals, point-to-cell means and the force sums of a 3-D surface given as points and
      a face list, one pass (inference.py:310-320 + utils.py:385-448): agn_surface_forces. No autograd.
  act_dropout(y, act, p, training=True) -> (out like y, keep-mask uint8 [ceil(n / 8)])
      dropout_p(act(y)) as mlp.py:44-45 applies it between two Linears, act a name of aerognn._lib.ACT
      ('relu', 'gelu', .. 'tanhshrink': include/aerognn.h AGN_ACT_*) or 'none'; Philox4x32-10 masks at the
      (seed, offset) of the device's default torch generator, which the call advances (read on the host:
      not under graph capture): agn_act_dropout_fwd.
      Backward: act_dropout_backward (agn_act_dropout_bwd). ops.act_dropout(...) returns out alone.

The fused MLP / MeshGraphNet-layer kernels are not registered as operators: their calls carry
packed-weight caches and a per-level CSC plan (Python objects), so they stay
torch.autograd.Functions behind the reference's nn.Module API (models/).

Every op requires device tensors and raises on CPU inputs: there is no CPU fallback.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor

from . import _lib as L
from . import functions as _fn
from .functions import _embed_rows
from .core import gather_rows as _gather_rows
from .core import require_device, segment_max as _segment_max
from .core import segment_max_backward as _segment_max_backward
from .core import segment_sum as _segment_sum

I32 = torch.int32


def _groups(index: Tensor, dim_size: int):
    from .graph import group_by
    idx = index.to(I32)
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= dim_size):
        raise IndexError(f"scatter index out of range [0, {dim_size})")
    return group_by(idx, dim_size)


def _rows2d(t: Tensor, what: str) -> Tensor:
    if t.dim() != 2:
        raise ValueError(f"{what}: expected a 2-D [rows, features] tensor, got shape {tuple(t.shape)}")
    return t.contiguous()


# ------------------------------------------------------------------------------- group_ptr
@torch.library.custom_op("aerognn::group_ptr", mutates_args=())
def group_ptr(index: Tensor, dim_size: int) -> Tensor:
    """int32 [dim_size + 1] offsets of the groups of `index` (group sizes = diff): the count a
    mean divides by, as a tensor op so autograd formulas stay traceable."""
    require_device(index)
    return _groups(index, dim_size)[1]


@group_ptr.register_fake
def _(index, dim_size):
    return index.new_empty(dim_size + 1, dtype=I32)


# ------------------------------------------------------------------------------- scatter_sum
@torch.library.custom_op("aerognn::scatter_sum", mutates_args=())
def scatter_sum(src: Tensor, index: Tensor, dim_size: int, mean: bool = False) -> Tensor:
    require_device(src, index)
    src = _rows2d(src, "scatter_sum")
    if index.numel() != src.shape[0]:
        raise ValueError("scatter_sum: index must have one entry per row of src")
    perm, rowptr = _groups(index, dim_size)
    out = torch.empty(dim_size, src.shape[1], dtype=src.dtype, device=src.device)
    if dim_size:
        _segment_sum(dim_size, src.shape[1], rowptr, perm, src, out, mean=mean)
    return out


@scatter_sum.register_fake
def _(src, index, dim_size, mean=False):
    return src.new_empty(dim_size, src.shape[1])


def _scatter_sum_ctx(ctx, inputs, output):
    src, index, dim_size, mean = inputs
    ctx.save_for_backward(index)
    ctx.mean = mean
    ctx.dim_size = dim_size


def _scatter_sum_bwd(ctx, g):
    (index,) = ctx.saved_tensors
    rowptr = torch.ops.aerognn.group_ptr(index, ctx.dim_size) if ctx.mean else None
    return torch.ops.aerognn.gather_rows(g, index, rowptr), None, None, None


torch.library.register_autograd("aerognn::scatter_sum", _scatter_sum_bwd, setup_context=_scatter_sum_ctx)


# ------------------------------------------------------------------------------- gather_rows
@torch.library.custom_op("aerognn::gather_rows", mutates_args=())
def gather_rows(src: Tensor, index: Tensor, rowptr: Optional[Tensor] = None) -> Tensor:
    require_device(src, index, rowptr)
    src = _rows2d(src, "gather_rows")
    idx = index.to(I32).contiguous()
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= src.shape[0]):
        raise IndexError(f"gather index out of range [0, {src.shape[0]})")
    out = torch.empty(idx.numel(), src.shape[1], dtype=src.dtype, device=src.device)
    if idx.numel():
        _gather_rows(idx.numel(), src.shape[1], idx, src, out,
                     cnt_ptr=rowptr.to(I32).contiguous() if rowptr is not None else None)
    return out


@gather_rows.register_fake
def _(src, index, rowptr=None):
    return src.new_empty(index.numel(), src.shape[1])


def _gather_ctx(ctx, inputs, output):
    src, index, rowptr = inputs
    ctx.save_for_backward(index, rowptr)
    ctx.n = src.shape[0]


def _gather_bwd(ctx, g):
    index, rowptr = ctx.saved_tensors
    # d src[r] = sum over i with index[i] == r of g[i], divided by the caller's group size
    # max(rowptr[r+1] - rowptr[r], 1) when the forward divided by it (any rowptr, not only
    # group_ptr(index))
    if rowptr is None:
        return torch.ops.aerognn.scatter_sum(g, index, ctx.n, False), None, None
    # sum and divide in fp32 and round once, as the forward's in-kernel fp32 division does (a bf16
    # count would round group sizes above 256, a bf16 sum would round before the division)
    # (16-bit types only: a float64 gradient stays float64, float32 is already fp32)
    gs = g.float() if g.dtype in (torch.bfloat16, torch.float16) else g
    d = torch.ops.aerognn.scatter_sum(gs, index, ctx.n, False)
    cnt = (rowptr[1:] - rowptr[:-1]).clamp(min=1).to(gs.dtype)
    return (d / cnt[:, None]).to(g.dtype), None, None


torch.library.register_autograd("aerognn::gather_rows", _gather_bwd, setup_context=_gather_ctx)


# ------------------------------------------------------------------------------- scatter_max
@torch.library.custom_op("aerognn::scatter_max", mutates_args=())
def scatter_max(src: Tensor, index: Tensor, dim_size: int) -> tuple[Tensor, Tensor]:
    require_device(src, index)
    src = _rows2d(src, "scatter_max")
    if index.numel() != src.shape[0]:
        raise ValueError("scatter_max: index must have one entry per row of src")
    perm, rowptr = _groups(index, dim_size)
    k = src.shape[1]
    out = torch.empty(dim_size, k, dtype=src.dtype, device=src.device)
    arg = torch.empty(dim_size, k, dtype=I32, device=src.device)
    if dim_size:
        _segment_max(dim_size, k, rowptr, perm, src, out, arg)
    arg64 = arg.to(torch.int64)
    return out, torch.where(arg64 < 0, torch.full_like(arg64, src.shape[0]), arg64)


@scatter_max.register_fake
def _(src, index, dim_size):
    return src.new_empty(dim_size, src.shape[1]), src.new_empty(dim_size, src.shape[1], dtype=torch.int64)


@torch.library.custom_op("aerognn::scatter_max_backward", mutates_args=())
def scatter_max_backward(grad: Tensor, argmax: Tensor, n: int) -> Tensor:
    require_device(grad, argmax)
    grad = _rows2d(grad, "scatter_max_backward")
    arg = torch.where(argmax >= n, torch.full_like(argmax, -1), argmax).to(I32).contiguous()
    dx = torch.zeros(n, grad.shape[1], dtype=grad.dtype, device=grad.device)
    if grad.shape[0]:
        _segment_max_backward(grad.shape[0], grad.shape[1], arg, grad, dx)
    return dx


@scatter_max_backward.register_fake
def _(grad, argmax, n):
    return grad.new_empty(n, grad.shape[1])


def _scatter_max_ctx(ctx, inputs, output):
    src, index, dim_size = inputs
    ctx.save_for_backward(output[1])
    ctx.n = src.shape[0]
    ctx.set_materialize_grads(True)


def _scatter_max_bwd(ctx, g_out, g_arg):
    (arg,) = ctx.saved_tensors
    return torch.ops.aerognn.scatter_max_backward(g_out, arg, ctx.n), None, None


torch.library.register_autograd("aerognn::scatter_max", _scatter_max_bwd, setup_context=_scatter_max_ctx)


# ------------------------------------------------------------------------------- edge_features
@torch.library.custom_op("aerognn::edge_features", mutates_args=())
def edge_features(pos: Tensor, edge_index: Tensor, mean: Optional[Tensor] = None,
                  std: Optional[Tensor] = None) -> Tensor:
    from .data import compute_edge_attr
    if (mean is None) != (std is None):
        raise ValueError("edge_features: give both mean and std, or neither")
    stats = None if mean is None else {"edge_mean": mean, "edge_std": std}
    return compute_edge_attr(pos=pos, edge_index=edge_index, stats=stats)


@edge_features.register_fake
def _(pos, edge_index, mean=None, std=None):
    return pos.new_empty(edge_index.shape[1], pos.shape[1] + 1, dtype=torch.float32)


# ------------------------------------------------------------------------------- fourier_embed
@torch.library.custom_op("aerognn::fourier_embed", mutates_args=())
def fourier_embed(x: Tensor, d: int, freq_start: int, freq_len: int, with_input: bool = True) -> Tensor:
    return _fn.fourier_forward(x, d, freq_start, freq_len, with_input)[1]


@fourier_embed.register_fake
def _(x, d, freq_start, freq_len, with_input=True):
    return x.new_empty(x.shape[0], (x.shape[1] if with_input else 0) + 2 * d * freq_len)


@torch.library.custom_op("aerognn::fourier_embed_backward", mutates_args=())
def fourier_embed_backward(grad: Tensor, x: Tensor, d: int, freq_start: int, freq_len: int,
                           with_input: bool) -> Tensor:
    return _fn.fourier_backward(grad, x, d, freq_start, freq_len, with_input)


@fourier_embed_backward.register_fake
def _(grad, x, d, freq_start, freq_len, with_input):
    return x.new_empty(x.shape[0], x.shape[1])


def _fourier_ctx(ctx, inputs, output):
    x, d, freq_start, freq_len, with_input = inputs
    ctx.save_for_backward(x)
    ctx.cfg = (d, freq_start, freq_len, with_input)


def _fourier_bwd(ctx, g):
    (x,) = ctx.saved_tensors
    return torch.ops.aerognn.fourier_embed_backward(g, x, *ctx.cfg), None, None, None, None


torch.library.register_autograd("aerognn::fourier_embed", _fourier_bwd, setup_context=_fourier_ctx)


# ------------------------------------------------------------------------------- activation + dropout
def _act_code(act: str) -> int:
    if act == "none":
        return L.ACT_NONE
    if act not in L.ACT:
        raise ValueError(f"act_dropout: act must be 'none' or one of {sorted(L.ACT)}, got {act!r}")
    return L.ACT[act]


def _check_p(p: float):
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"dropout probability has to be between 0 and 1, but got {p}")


@torch.library.custom_op("aerognn::act_dropout", mutates_args=())
def _act_dropout(y: Tensor, act: str, p: float, training: bool = True) -> tuple[Tensor, Tensor]:
    """(dropout_p(act(y)), keep-mask): the mask is one bit per element of y taken flat (bit e & 7 of byte
    e >> 3), Philox4x32-10 at the (seed, offset) of the device's default torch generator, which the
    call advances by 4 ceil(n / 4). Not training, or p = 0: act(y), all kept, nothing drawn."""
    require_device(y)
    _check_p(p)
    return _fn.act_dropout_forward(y, _act_code(act), float(p) if training else 0.0)[1:]


@_act_dropout.register_fake
def _(y, act, p, training=True):
    return torch.empty_like(y, memory_format=torch.contiguous_format), y.new_empty((y.numel() + 7) // 8,
                                                                                   dtype=torch.uint8)


@torch.library.custom_op("aerognn::act_dropout_backward", mutates_args=())
def act_dropout_backward(grad: Tensor, y: Tensor, mask: Tensor, act: str, p: float) -> Tensor:
    require_device(grad, y, mask)
    _check_p(p)
    return _fn.act_dropout_backward(grad, y, mask, _act_code(act), p)


@act_dropout_backward.register_fake
def _(grad, y, mask, act, p):
    return torch.empty_like(grad, memory_format=torch.contiguous_format)


def _act_dropout_ctx(ctx, inputs, output):
    y, act, p, training = inputs
    ctx.save_for_backward(y, output[1])
    ctx.cfg = (act, float(p) if training else 0.0)


def _act_dropout_bwd(ctx, g, g_mask):
    y, mask = ctx.saved_tensors
    return torch.ops.aerognn.act_dropout_backward(g, y, mask, *ctx.cfg), None, None, None


torch.library.register_autograd("aerognn::act_dropout", _act_dropout_bwd, setup_context=_act_dropout_ctx)


def act_dropout(y: Tensor, act: str, p: float, training: bool = True) -> Tensor:
    """dropout(act(y)) as the reference's MLP applies it between two Linears (mlp.py:44-45): act a name of
    aerognn._lib.ACT or 'none', training-mode dropout of probability p on torch's generator.
    torch.ops.aerognn.act_dropout returns the keep-mask bits as well."""
    return torch.ops.aerognn.act_dropout(y, act, p, training)[0]


# ------------------------------------------------------------------------------- evaluation
def _wide(t: Tensor, dtype=None) -> Tensor:
    """bf16 / fp16 widened to fp32 (exact); fp32 / fp64 kept; `dtype` forces the compute type."""
    if dtype is not None:
        return t if t.dtype == dtype else t.to(dtype)
    if t.dtype in (torch.float32, torch.float64):
        return t
    if t.dtype in (torch.bfloat16, torch.float16):
        return t.float()
    raise TypeError(f"aerognn evaluation ops take floating-point tensors, got {t.dtype}")


def _check_gptr(gptr: Tensor, what: str) -> Tensor:
    if gptr.dim() != 1 or gptr.numel() < 1 or gptr.dtype != I32:
        raise ValueError(f"{what}: gptr must be an int32 vector of ngraph + 1 row offsets")
    return gptr.contiguous()


@torch.library.custom_op("aerognn::eval_sums", mutates_args=())
def eval_sums(pred: Tensor, y: Tensor, mean: Tensor, std: Tensor, gptr: Tensor) -> Tensor:
    from ._lib import check, lib, ptr
    from .core import dt_code, stream
    require_device(pred, y, mean, std, gptr)
    if pred.dim() != 2 or y.shape != pred.shape:
        raise ValueError("eval_sums: pred and y must be 2-D [rows, features] tensors of one shape")
    n, f = pred.shape
    if mean.numel() != f or std.numel() != f:
        raise ValueError("eval_sums: mean and std must have one entry per feature")
    pred = _embed_rows(_wide(pred), "eval_sums")
    dt = pred.dtype
    y = _embed_rows(_wide(y, dt), "eval_sums")
    mean = _wide(mean, dt).reshape(-1).contiguous()
    std = _wide(std, dt).reshape(-1).contiguous()
    gptr = _check_gptr(gptr, "eval_sums")
    G = gptr.numel() - 1
    if n == 0 or G == 0:  # no launch: empty graphs give zeros
        return torch.zeros(G, 2, f, 6, dtype=torch.float64, device=pred.device)
    out = torch.empty(G, 2, f, 6, dtype=torch.float64, device=pred.device)  # the finishing pass writes every entry
    nb = int(lib().agn_eval_sums_temp_bytes(n, f, G))
    if nb == 0:
        raise ValueError(f"eval_sums: {f} features (the kernel takes 1..16)")
    scratch = torch.empty(nb, dtype=torch.uint8, device=pred.device)
    check(lib().agn_eval_sums(dt_code(dt), n, f, ptr(pred), pred.stride(0), ptr(y), y.stride(0), ptr(mean), ptr(std),
                              ptr(gptr), G, ptr(out), ptr(scratch), stream()), "eval_sums")
    return out


@eval_sums.register_fake
def _(pred, y, mean, std, gptr):
    return pred.new_empty(gptr.shape[0] - 1, 2, pred.shape[1], 6, dtype=torch.float64)


@torch.library.custom_op("aerognn::aero_forces", mutates_args=())
def aero_forces(pressure: Tensor, shear: Tensor, normals: Tensor, pos: Optional[Tensor], areas: Optional[Tensor],
                edge_index: Optional[Tensor], gptr: Tensor, center: list[float],
                length_scale: float = 1e-2) -> tuple[Tensor, Tensor]:
    """(sums [G, 4, 3] float64 = sum F, sum M, sum |F|, sum |M|; areas float64 [n] of the mesh rule, or
    [0] when the areas were given)."""
    import ctypes as C
    from ._lib import check, lib, ptr
    from .core import dt_code, stream
    from .graph import group_by
    require_device(pressure, shear, normals, pos, areas, edge_index, gptr)
    if shear.dim() != 2 or shear.shape[1] not in (2, 3):
        raise ValueError("aero_forces: shear must be [n, 2] or [n, 3]")
    n, dim = shear.shape
    if normals.shape != shear.shape or pressure.numel() != n or (pos is not None and pos.shape != shear.shape):
        raise ValueError("aero_forces: pressure [n], shear, normals and pos [n, dim] must agree")
    if (areas is None) == (edge_index is None):
        raise ValueError("aero_forces: give either the element areas or the mesh (edge_index), not both")
    if edge_index is not None and pos is None:
        raise ValueError("aero_forces: the mesh rule for the areas needs pos")
    if len(center) not in (0, dim):
        raise ValueError("aero_forces: center must have one entry per dimension")
    pressure = _wide(pressure).reshape(-1).contiguous()
    dt = pressure.dtype
    shear = _embed_rows(_wide(shear, dt), "aero_forces")
    normals = _embed_rows(_wide(normals, dt), "aero_forces")
    pos = None if pos is None else _embed_rows(_wide(pos, dt), "aero_forces")
    gptr = _check_gptr(gptr, "aero_forces")
    G = gptr.numel() - 1
    dev = pressure.device
    # the finishing pass writes every entry; without a launch (n == 0) empty graphs give zeros
    out = (torch.empty if n and G else torch.zeros)(G, 4, 3, dtype=torch.float64, device=dev)
    rowptr = perm = ei = None
    e = 0
    if edge_index is not None:
        if edge_index.dim() != 2 or edge_index.shape[0] != 2:
            raise ValueError("aero_forces: edge_index must be [2, E]")
        ei = edge_index.to(torch.int64).contiguous()
        e = ei.shape[1]
        if e and (int(ei.min()) < 0 or int(ei.max()) >= n):
            raise IndexError(f"aero_forces: edge_index out of range [0, {n})")
        perm, rowptr = group_by(ei[0], n)  # stable: a node's outgoing edges stay in the caller's order
        area_out = torch.zeros(n, dtype=torch.float64, device=dev)
    else:
        areas = areas.to(torch.float64).reshape(-1).contiguous()
        if areas.numel() != n:
            raise ValueError("aero_forces: areas must have one entry per element")
        area_out = torch.empty(0, dtype=torch.float64, device=dev)
    if n == 0 or G == 0:
        return out, area_out
    ctr = (C.c_double * dim)(*[float(c) for c in center]) if len(center) else None
    scratch = torch.empty(int(lib().agn_aero_forces_temp_bytes(n, G)), dtype=torch.uint8, device=dev)
    check(lib().agn_aero_forces(dt_code(dt), n, dim, ptr(pressure), ptr(shear), shear.stride(0), ptr(normals),
                                normals.stride(0), ptr(pos), 0 if pos is None else pos.stride(0), ptr(areas),
                                ptr(ei), e, ptr(rowptr), ptr(perm), float(length_scale),
                                ptr(area_out) if ei is not None else None, ctr, ptr(gptr), G, ptr(out), ptr(scratch),
                                stream()), "aero_forces")
    return out, area_out


@aero_forces.register_fake
def _(pressure, shear, normals, pos, areas, edge_index, gptr, center, length_scale=1e-2):
    n = shear.shape[0] if edge_index is not None else 0
    return (shear.new_empty(gptr.shape[0] - 1, 4, 3, dtype=torch.float64),
            shear.new_empty(n, dtype=torch.float64))


@torch.library.custom_op("aerognn::surface_forces", mutates_args=())
def surface_forces(pos: Optional[Tensor], offsets: Optional[Tensor], conn: Tensor, fields: list[Tensor],
                   mean: Optional[Tensor], std: Optional[Tensor], cgptr: Tensor,
                   want_cells: bool = False) -> tuple[Tensor, Tensor, Tensor, Tensor]:
    """(sums [G, nset, 2, 3] float64 = sum F, sum |F|; areas float64 [C]; normals float64 [C, 3]; cells
    [nset, C, 4] of the field dtype). Without want_cells the three cell outputs are empty ([0], [0, 3],
    [0, C, 4]); without pos the geometry is skipped (point-to-cell means alone) and areas / normals are
    empty. pos and the fields may be fp32 or fp64 independently (the geometry is fp64 either way: an fp32
    pos gives what its exact fp64 copy gives); bf16 / fp16 inputs are widened to fp32 first."""
    import ctypes as C
    from ._lib import check, lib, ptr
    from .core import dt_code, stream
    require_device(pos, offsets, conn, mean, std, cgptr, *fields)
    nset = len(fields)
    if nset > 4:
        raise ValueError("surface_forces: at most four field sets")
    if pos is None and nset == 0:
        raise ValueError("surface_forces: nothing to do without pos and without fields")
    if pos is not None and (pos.dim() != 2 or pos.shape[1] != 3):
        raise ValueError("surface_forces: pos must be [N, 3]")
    n = pos.shape[0] if pos is not None else fields[0].shape[0]
    if any(f.dim() != 2 or f.shape != (n, 4) for f in fields):
        raise ValueError("surface_forces: every field set must be [N, 4] (pressure, tau_x, tau_y, tau_z)")
    if (mean is None) != (std is None):
        raise ValueError("surface_forces: give mean and std together")
    if offsets is None:
        if conn.dim() != 2:
            raise ValueError("surface_forces: without offsets conn must be [C, k]")
        ncell, k = conn.shape
    else:
        if conn.dim() != 1 or offsets.dim() != 1 or offsets.numel() < 1:
            raise ValueError("surface_forces: the CSR form takes offsets [C + 1] and a flat conn")
        ncell, k = offsets.numel() - 1, 0
        offsets = offsets.to(torch.int64).contiguous()
    conn = conn.to(torch.int64).contiguous()
    nconn = conn.numel()
    if nconn:
        lo, hi = torch.stack(list(torch.aminmax(conn))).tolist()  # one copy to the host
        if lo < 0 or hi >= n:
            raise IndexError(f"surface_forces: face ids out of range [0, {n})")
    dev = conn.device
    pos = None if pos is None else _embed_rows(_wide(pos), "surface_forces")
    fields = [_embed_rows(_wide(f), "surface_forces") for f in fields]
    fdt = fields[0].dtype if nset else (pos.dtype if pos is not None else torch.float32)
    fields = [f if f.dtype == fdt else f.to(fdt) for f in fields]
    if mean is not None:
        mean, std = _wide(mean, fdt).reshape(-1).contiguous(), _wide(std, fdt).reshape(-1).contiguous()
        if mean.numel() != 4 or std.numel() != 4:
            raise ValueError("surface_forces: mean and std must have four entries")
    cgptr = _check_gptr(cgptr, "surface_forces")
    G = cgptr.numel() - 1
    launch = ncell > 0 and G > 0
    out = (torch.empty if launch and nset else torch.zeros)(G, nset, 2, 3, dtype=torch.float64, device=dev)
    geo = want_cells and pos is not None
    areas = torch.empty(ncell if geo else 0, dtype=torch.float64, device=dev)
    normals = torch.empty(ncell if geo else 0, 3, dtype=torch.float64, device=dev)
    cells = torch.empty(nset if want_cells else 0, ncell, 4, dtype=fdt, device=dev)
    if not launch:
        return out, areas, normals, cells
    scratch = torch.empty(int(lib().agn_surface_forces_temp_bytes(ncell, G, nset)), dtype=torch.uint8, device=dev)
    fptr = (C.c_void_p * max(nset, 1))(*[f.data_ptr() for f in fields])
    fld = (C.c_int * max(nset, 1))(*[max(f.stride(0), 4) for f in fields])
    check(lib().agn_surface_forces(dt_code(pos.dtype) if pos is not None else dt_code(fdt), n, ptr(pos),
                                   0 if pos is None else max(pos.stride(0), 3), ncell, ptr(offsets), ptr(conn), nconn, k,
                                   dt_code(fdt), nset, fptr, fld, ptr(mean), ptr(std), ptr(cgptr), G,
                                   ptr(out) if nset else None, ptr(areas) if geo else None,
                                   ptr(normals) if geo else None, ptr(cells) if want_cells and nset else None,
                                   ptr(scratch), stream()), "surface_forces")
    return out, areas, normals, cells


@surface_forces.register_fake
def _(pos, offsets, conn, fields, mean, std, cgptr, want_cells=False):
    ncell = conn.shape[0] if offsets is None else offsets.shape[0] - 1
    nset = len(fields)
    fdt = fields[0].dtype if nset else (pos.dtype if pos is not None else torch.float32)
    if fdt in (torch.bfloat16, torch.float16):
        fdt = torch.float32
    geo = want_cells and pos is not None
    return (conn.new_empty(cgptr.shape[0] - 1, nset, 2, 3, dtype=torch.float64),
            conn.new_empty(ncell if geo else 0, dtype=torch.float64),
            conn.new_empty(ncell if geo else 0, 3, dtype=torch.float64),
            conn.new_empty(nset if want_cells else 0, ncell, 4, dtype=fdt))


# ------------------------------------------------------------------------------- PyG-style pools
def global_add_pool(x: Tensor, batch: Optional[Tensor], size: Optional[int] = None) -> Tensor:
    """torch_geometric.nn.global_add_pool on torch.ops.aerognn.scatter_sum."""
    if batch is None:
        batch = torch.zeros(x.shape[0], dtype=torch.int64, device=x.device)
    size = int(batch.max()) + 1 if size is None else size
    return torch.ops.aerognn.scatter_sum(x, batch, size, False)


def global_mean_pool(x: Tensor, batch: Optional[Tensor], size: Optional[int] = None) -> Tensor:
    if batch is None:
        batch = torch.zeros(x.shape[0], dtype=torch.int64, device=x.device)
    size = int(batch.max()) + 1 if size is None else size
    return torch.ops.aerognn.scatter_sum(x, batch, size, True)


def global_max_pool(x: Tensor, batch: Optional[Tensor], size: Optional[int] = None) -> Tensor:
    if batch is None:
        batch = torch.zeros(x.shape[0], dtype=torch.int64, device=x.device)
    size = int(batch.max()) + 1 if size is None else size
    return torch.ops.aerognn.scatter_max(x, batch, size)[0]
