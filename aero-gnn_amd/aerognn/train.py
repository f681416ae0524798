"""The training step's tail on the device: what the reference does with the prediction after
`model(...)` (utils.py:171-196 train, :198-219 evaluate; train.py:222 nn.MSELoss()).

  mse_loss_grad(pred, y, n_global=None, acc=None) -> (loss, dpred)   one pass over pred and y
  MSELoss()                                   drop-in for nn.MSELoss() and dist.mse_sum_loss
  train(model, loader, optimizer, loss_fn, device)     utils.py:171-196, same signature and value
  evaluate(model, loader, loss_fn, device)             utils.py:198-219

The loss value is an fp64 sum in a fixed order (agn_mse_loss, csrc/train.hip: two calls give identical
bytes) and stays on the device: with this module's MSELoss, or an nn.MSELoss with mean reduction,
train() and evaluate() add each batch's loss to a device accumulator inside the loss kernel and read
it ONCE per epoch, where the reference's `total_loss += loss.item()` waits for the device once per
batch. Any other loss_fn runs the reference's loop as written, and so does a batch the kernel does not
cover (a CPU prediction, pred and y of different shapes, a y wider than pred's dtype and float32), where
nn.MSELoss broadcasts or promotes. Both work with any optimizer;
aerognn.optim.Adam is what removes the optimizer's launches.
"""
from __future__ import annotations

import torch
from torch import nn

from . import _lib as L
from .core import dt_code, require_device, stream


def chunk_rows() -> int:
    """Rows per first-stage chunk of the loss reduction (agn_mse_chunk_rows)."""
    return int(L.lib().agn_mse_chunk_rows())


def _rows(t):
    """t as [n, f] with unit column stride, without a copy where its layout allows."""
    if t.dim() == 2 and (t.stride(1) == 1 or t.shape[1] == 1) and t.stride(0) >= t.shape[1]:
        return t
    if t.dim() == 0:
        return t.reshape(1, 1)
    t = t.contiguous()
    return t.view(-1, t.shape[-1]) if t.dim() >= 2 else t.view(-1, 1)


def mse_loss_grad(pred, y, n_global=None, acc=None, need_grad=True):
    """(loss, dpred): loss = sum((pred - y)^2) / n_global as a 0-dim float64 device tensor, dpred =
    2 (pred - y) / n_global in pred's dtype and shape (None with need_grad=False); the caller runs
    pred.backward(dpred). n_global: the element count of the mean (default pred.numel(); the
    all-reduced count under data parallelism, dist.global_count). acc: a 0-dim float64 device tensor
    the loss is also added to (the epoch accumulator). y is in pred's dtype or float32."""
    require_device(pred, y, acc)
    if pred.shape != y.shape:
        raise ValueError(f"mse_loss_grad: pred {tuple(pred.shape)} and y {tuple(y.shape)} differ in shape")
    p2, y2 = _rows(pred.detach()), _rows(y.detach())
    n, f = p2.shape
    if n_global is None:
        n_global = float(n * f)
    if acc is not None and (acc.dtype != torch.float64 or acc.numel() != 1):
        raise TypeError("mse_loss_grad: acc must be a float64 scalar tensor on the device")
    dev = pred.device
    loss = torch.empty((), dtype=torch.float64, device=dev)
    dpred = torch.empty((n, f), dtype=pred.dtype, device=dev) if need_grad else None
    lib = L.lib()
    scratch = torch.empty(max(int(lib.agn_mse_loss_temp_bytes(n, f)), 16), dtype=torch.uint8, device=dev)
    L.check(lib.agn_mse_loss(dt_code(pred.dtype), dt_code(y.dtype), n, f, L.ptr(p2), p2.stride(0) if n > 1 else f,
                             L.ptr(y2), y2.stride(0) if n > 1 else f, float(n_global), L.ptr(loss), L.ptr(acc),
                             L.ptr(dpred), f, L.ptr(scratch), stream()), "mse_loss")
    return loss, (dpred.view(pred.shape) if need_grad else None)


class _MSE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, y, n_global):
        loss, dpred = mse_loss_grad(pred, y, n_global, need_grad=pred.requires_grad)
        ctx.dpred = dpred
        return loss

    @staticmethod
    def backward(ctx, grad_output):
        dpred = ctx.dpred
        return (None if dpred is None else dpred * grad_output.to(dpred.dtype)), None, None


class MSELoss(nn.Module):
    """nn.MSELoss() (mean reduction) on agn_mse_loss: a float64 0-dim loss whose backward hands the
    gradient formed in the same pass to pred. forward(pred, y, n_global=None): n_global as in
    mse_loss_grad (dist.mse_sum_loss's divisor)."""

    reduction = "mean"

    def forward(self, pred, y, n_global=None):
        return _MSE.apply(pred, y, n_global)


def _forward(model, batch):
    """The model-class dispatch of utils.py:178-189 / :206-215."""
    model_class = model.__class__.__name__
    if model_class in ("poolMGN", "MeshGraphNet_v2"):
        return model(batch.x, batch.edge_attr, batch.edge_index, batch.batch)
    if model_class in ("BiStridedMeshGraphNet",):
        pos = batch.pos if hasattr(batch, "pos") else None
        return model(batch.x, batch.edge_attr, batch.edge_index, batch=batch.batch, pos=pos)
    if model_class in ("MLPNet",):
        return model(batch.x)
    return model(batch.x, batch.edge_attr, batch.edge_index)


def _fused(loss_fn) -> bool:
    if isinstance(loss_fn, MSELoss):
        return True
    return isinstance(loss_fn, nn.MSELoss) and loss_fn.reduction == "mean"


_KERNEL_DTYPES = (torch.float32, torch.bfloat16, torch.float16, torch.float64)


def _kernel_applies(pred, y) -> bool:
    """agn_mse_loss covers this pair: both on the device, one shape (nn.MSELoss would broadcast
    otherwise), pred in a kernel dtype and y in pred's dtype or float32 (nn.MSELoss would promote
    otherwise). Anything else takes the reference's loop with the loss_fn as given."""
    return (torch.is_tensor(y) and pred.is_cuda and y.is_cuda and pred.shape == y.shape
            and pred.dtype in _KERNEL_DTYPES and (y.dtype == pred.dtype or y.dtype == torch.float32))


def train(model, loader, optimizer, loss_fn, device):
    """utils.py:171-196. The fused path (module docstring) needs the prediction on the device."""
    model.train()
    fused = _fused(loss_fn)
    total_loss = 0.0
    acc = None
    for batch in loader:
        batch = batch.to(device)
        pred = _forward(model, batch)
        if fused and _kernel_applies(pred, batch.y):
            if acc is None:
                acc = torch.zeros((), dtype=torch.float64, device=pred.device)
            _, dpred = mse_loss_grad(pred, batch.y, acc=acc)
            pred.backward(dpred)
            optimizer.step()
            optimizer.zero_grad()
            continue
        loss = loss_fn(pred, batch.y)
        loss.backward()
        optimizer.step()
        optimizer.zero_grad()
        total_loss += loss.item()
    if acc is not None:
        total_loss += float(acc)  # the one read of the epoch
    return total_loss / len(loader)


@torch.no_grad()
def evaluate(model, loader, loss_fn, device):
    """utils.py:198-219."""
    model.eval()
    fused = _fused(loss_fn)
    total_loss = 0.0
    acc = None
    for batch in loader:
        batch = batch.to(device)
        pred = _forward(model, batch)
        if fused and _kernel_applies(pred, batch.y):
            if acc is None:
                acc = torch.zeros((), dtype=torch.float64, device=pred.device)
            mse_loss_grad(pred, batch.y, acc=acc, need_grad=False)
            continue
        loss = loss_fn(pred, batch.y)
        total_loss += loss.item()
    if acc is not None:
        total_loss += float(acc)
    return total_loss / len(loader)
