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

  LossScaler(device=None, init_scale=2.**16, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000)

Dynamic loss scaling for the reference's `precision: float16` (train.py:35-38), whose gradients are fp16:
at n_global = 2^22 the unscaled dpred = 2 (pred - y) / n_global is under fp16's smallest subnormal wherever
|pred - y| < 2^-4. mse_loss_grad / MSELoss / train take `scaler=`: the loss kernel then multiplies the fp64
gradient by the scale S before it rounds to pred's dtype (agn_mse_loss_scaled; the loss value is never
scaled), scaler.step(optimizer) checks every gradient on the device and runs aerognn.optim.Adam's step on
g / S or skips it (aerognn.optim, "Loss scaling"), and scaler.update() is torch.amp.GradScaler's scale update
on the device. S, the found_inf flag, the growth tracker and the skipped-step count are 16 bytes of device
memory that the host does not read in a step. Under data parallelism the scaler steps after
GradAllReduce.__call__: a non-finite value on one rank reaches every rank through the sum, so all ranks
skip the same steps and keep the same scale.
"""
from __future__ import annotations

import math

import numpy as np
import torch
from torch import nn

from . import _lib as L
from .core import dt_code, require_device, stream
from .optim import Adam, _PendingStep


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


class LossScaler:
    """torch.amp.GradScaler's dynamic loss scale (its defaults, its update rule bit for bit, its
    state_dict keys: a checkpoint of either loads into the other) with the state on the device (module
    docstring). The 16 bytes are allocated at the first use, on `device` or on the device of the first
    tensor it meets. get_scale() and steps_skipped() read the device and may synchronise."""

    def __init__(self, device=None, init_scale=2.0 ** 16, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
        init_scale, growth_factor, backoff_factor = float(init_scale), float(growth_factor), float(backoff_factor)
        with np.errstate(over="ignore"):
            s32 = float(np.float32(init_scale))  # what the device holds
        if not (s32 > 0.0 and math.isfinite(s32)):
            raise ValueError(f"LossScaler: init_scale must be a positive finite float32, not {init_scale!r}")
        if not (growth_factor > 1.0 and math.isfinite(growth_factor)):
            raise ValueError(f"LossScaler: growth_factor must be > 1, not {growth_factor!r}")
        if not 0.0 < backoff_factor < 1.0:
            raise ValueError(f"LossScaler: backoff_factor must be in (0, 1), not {backoff_factor!r}")
        if isinstance(growth_interval, bool) or int(growth_interval) != growth_interval or growth_interval < 1:
            raise ValueError(f"LossScaler: growth_interval must be an integer >= 1, not {growth_interval!r}")
        if device is not None and torch.device(device).type != "cuda":
            raise ValueError(f"LossScaler: the state lives on a HIP device, not on {device!r}")
        self._device = None if device is None else torch.device(device)
        self._init_scale, self._init_tracker = init_scale, 0
        self._growth_factor, self._backoff_factor = growth_factor, backoff_factor
        self._growth_interval = int(growth_interval)
        self._state = None     # int32[4] on the device: agn_loss_scale_state
        self._pending = []     # scaled steps whose found_inf copy has not been read
        self._words = []       # free page-locked words

    def _device_state(self, device=None):
        """The state tensor, allocated on `device` at the first call."""
        if self._state is None:
            dev = self._device or (torch.device(device) if device is not None else torch.device("cuda"))
            if dev.type != "cuda":
                raise RuntimeError(f"LossScaler: the state lives on a HIP device, not on {dev}")
            host = np.zeros(1, dtype=np.dtype(L.LossScaleState))
            host["scale"], host["growth_tracker"] = self._init_scale, self._init_tracker
            self._state = torch.from_numpy(host.view(np.int32).copy()).to(dev)
        elif device is not None and torch.device(device).type == "cuda" and self._state.device != _indexed(device):
            raise RuntimeError(f"LossScaler: the state is on {self._state.device}, not on {device}")
        return self._state

    def _read(self):
        host = self._state.cpu().numpy().view(np.dtype(L.LossScaleState))[0]
        return float(host["scale"]), int(host["found_inf"]), int(host["growth_tracker"]), int(host["skipped"])

    def _watch(self, steps):
        """Enqueue the copy of found_inf to a page-locked word behind the check, guard it with an event
        and hand back the record of the step (optim._PendingStep) that the next step resolves."""
        word = self._words.pop() if self._words else torch.zeros(1, dtype=torch.int32, pin_memory=True)
        word.copy_(self._state[1:2], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        pend = _PendingStep(word, ev, steps, self._done)
        self._pending.append(pend)
        return pend

    def _done(self, pend):
        self._pending.remove(pend)
        self._words.append(pend.word)

    def _resolve(self):
        for pend in list(self._pending):
            pend.resolve()

    def get_scale(self) -> float:
        return self._init_scale if self._state is None else self._read()[0]

    def steps_skipped(self) -> int:
        return 0 if self._state is None else self._read()[3]

    def get_growth_factor(self) -> float:
        return self._growth_factor

    def get_backoff_factor(self) -> float:
        return self._backoff_factor

    def get_growth_interval(self) -> int:
        return self._growth_interval

    def step(self, optimizer, closure=None):
        """The optimizer's step on the scaled gradients, skipped as a whole when one of them is not finite.
        Needs an aerognn.optim.Adam; nothing is downgraded to torch's own step (RuntimeError instead)."""
        if not isinstance(optimizer, Adam):
            raise RuntimeError(f"LossScaler.step needs an aerognn.optim.Adam, not {type(optimizer).__module__}."
                               f"{type(optimizer).__name__}: another optimizer's step would apply the scaled gradients")
        if closure is not None:
            raise RuntimeError("LossScaler.step does not take a closure: step(closure) runs torch's own step, which "
                               "would apply the scaled gradients")
        return optimizer.step(scaler=self)

    def update(self):
        """torch.amp.GradScaler.update() on the device (agn_loss_scale_update); clears found_inf."""
        state = self._device_state()
        with torch.cuda.device(state.device):
            L.check(L.lib().agn_loss_scale_update(L.ptr(state), self._growth_factor, self._backoff_factor,
                                                  self._growth_interval, stream()), "loss_scale_update")

    def state_dict(self):
        """torch.amp.GradScaler.state_dict()'s keys. Resolves the last step first, so that an optimizer
        state_dict() taken next to it has its counters right."""
        self._resolve()
        scale, tracker = (self._init_scale, self._init_tracker) if self._state is None else self._read()[0:3:2]
        return {"scale": scale, "growth_factor": self._growth_factor, "backoff_factor": self._backoff_factor,
                "growth_interval": self._growth_interval, "_growth_tracker": tracker}

    def load_state_dict(self, state_dict):
        if len(state_dict) == 0:
            raise RuntimeError("LossScaler.load_state_dict: the source state dict is empty (a disabled GradScaler's)")
        self._resolve()
        self._init_scale = float(state_dict["scale"])
        self._growth_factor = float(state_dict["growth_factor"])
        self._backoff_factor = float(state_dict["backoff_factor"])
        self._growth_interval = int(state_dict["growth_interval"])
        self._init_tracker = int(state_dict["_growth_tracker"])
        if self._state is not None:
            host = self._state.cpu().numpy().view(np.dtype(L.LossScaleState))
            host["scale"], host["growth_tracker"] = self._init_scale, self._init_tracker
            self._state.copy_(torch.from_numpy(host.view(np.int32)))


def _indexed(device):
    d = torch.device(device)
    return torch.device("cuda", torch.cuda.current_device()) if d.index is None else d


def mse_loss_grad(pred, y, n_global=None, acc=None, need_grad=True, scaler=None):
    """(loss, dpred): loss = sum((pred - y)^2) / n_global as a 0-dim float64 device tensor, dpred =
    2 (pred - y) / n_global in pred's dtype and shape (None with need_grad=False); the caller runs
    pred.backward(dpred). n_global: the element count of the mean (default pred.numel(); the
    all-reduced count under data parallelism, dist.global_count). acc: a 0-dim float64 device tensor
    the loss is also added to (the epoch accumulator). y is in pred's dtype or float32. scaler: a
    LossScaler; dpred is then 2 (pred - y) / n_global * S, multiplied before it is rounded to pred's dtype,
    and the loss is the same bytes as without one."""
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
    args = (dt_code(pred.dtype), dt_code(y.dtype), n, f, L.ptr(p2), p2.stride(0) if n > 1 else f, L.ptr(y2),
            y2.stride(0) if n > 1 else f, float(n_global), L.ptr(loss), L.ptr(acc), L.ptr(dpred), f, L.ptr(scratch))
    if scaler is None:
        L.check(lib.agn_mse_loss(*args, stream()), "mse_loss")
    else:
        L.check(lib.agn_mse_loss_scaled(*args, L.ptr(scaler._device_state(dev)), stream()), "mse_loss_scaled")
    return loss, (dpred.view(pred.shape) if need_grad else None)


class _MSE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, y, n_global, scaler=None):
        loss, dpred = mse_loss_grad(pred, y, n_global, need_grad=pred.requires_grad, scaler=scaler)
        ctx.dpred = dpred
        return loss

    @staticmethod
    def backward(ctx, grad_output):
        dpred = ctx.dpred
        return (None if dpred is None else dpred * grad_output.to(dpred.dtype)), None, None, None


class MSELoss(nn.Module):
    """nn.MSELoss() (mean reduction) on agn_mse_loss: a float64 0-dim loss whose backward hands the
    gradient formed in the same pass to pred. forward(pred, y, n_global=None, scaler=None): n_global and
    scaler as in mse_loss_grad (dist.mse_sum_loss's divisor; the gradient scaled, the value not)."""

    reduction = "mean"

    def forward(self, pred, y, n_global=None, scaler=None):
        return _MSE.apply(pred, y, n_global, scaler)


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


def train(model, loader, optimizer, loss_fn, device, scaler=None):
    """utils.py:171-196. The fused path (module docstring) needs the prediction on the device. scaler: a
    LossScaler; the gradient is scaled inside the loss kernel, scaler.step(optimizer) and scaler.update()
    take optimizer.step()'s place, and the returned epoch loss is the unscaled one. A batch that would
    take the reference's loop then raises RuntimeError: its loss_fn cannot scale before it rounds."""
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
            _, dpred = mse_loss_grad(pred, batch.y, acc=acc, scaler=scaler)
            pred.backward(dpred)
            if scaler is None:
                optimizer.step()
            else:
                scaler.step(optimizer)
                scaler.update()
            optimizer.zero_grad()
            continue
        if scaler is not None:
            raise RuntimeError("aerognn.train.train: a LossScaler needs the fused loss (MSELoss or nn.MSELoss with mean "
                               "reduction, prediction and target on the device in dtypes agn_mse_loss covers)")
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
