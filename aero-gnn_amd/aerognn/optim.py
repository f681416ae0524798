"""Adam on the device in one launch per parameter dtype (agn_adam_step, csrc/train.hip): the
reference's torch.optim.Adam of train.py:207-212 as utils.py:193 steps it.

`Adam` IS torch.optim.Adam: the same constructor, param_groups, defaults, state layout (per parameter
`step` as a CPU float32 scalar tensor, `exp_avg`, `exp_avg_sq`) and state_dict(), so
ReduceLROnPlateau, the global optimizer-step hooks (aerognn.core's fault checkpoint) and checkpoints
of either class work with the other. Only step() differs: every parameter that qualifies (a HIP
tensor, float32 or float64, contiguous, with a dense gradient of the same dtype or with no gradient)
is updated by agn_adam_step from a device-resident descriptor table. Everything this module does not
cover runs torch.optim.Adam's own step() unchanged: parameters that do not qualify (CPU, 16-bit,
non-contiguous), and the whole step when any group sets amsgrad, maximize, capturable,
differentiable, decoupled_weight_decay, fused=True (torch then keeps `step` on the device) or a tensor
lr / beta, or when a closure is passed.

Per step the host writes the gradient pointers and the per-tensor scalars (lr is read from
param_groups every time; step_size and bc2_sqrt are formed in double from the tensor's own step
count, as torch's single-tensor Adam forms them) into a page-locked staging buffer and enqueues ONE
async copy on the current stream; nothing synchronises the device. The staging buffer is
double-buffered and each half guarded by an event (the way core._fault_enqueue guards its word), so a
host that runs ahead never overwrites a half whose copy is still in flight. The chunk map
((tensor, chunk) pairs of agn_adam_chunk_elems elements) is rebuilt only when the tensor list changes.
Once every parameter has its state, a step only checks that the parameters, their entries in
`self.state`, their state tensors and the gradients' layout are those of the last step (object by
object and pointer by pointer, before anything is changed) and
gathers the gradient pointers; anything that moved sends the step through the full partition again.
"""
from __future__ import annotations

import numpy as np
import torch
from torch.optim.adam import Adam as _TorchAdam

from . import _lib as L

_CODES = {torch.float32: L.F32, torch.float64: L.F64}
_DESC = np.dtype(L.AdamDesc)


def chunk_elems() -> int:
    """Elements per chunk-map entry (agn_adam_chunk_elems)."""
    return int(L.lib().agn_adam_chunk_elems())


def _step_dtype():
    """dtype of the per-parameter `step` counter: what torch.optim.Adam._init_group creates for a
    non-fused, non-capturable group (float32, or float64 when that is the default dtype)."""
    return torch.float64 if torch.get_default_dtype() == torch.float64 else torch.float32


def _base_step(opt, closure=None):
    """torch.optim.Adam.step itself, without a second round of the step hooks: torch wraps a class's
    step with its hook runner once an instance of that very class exists (it marks the wrapper
    `hooked` and functools.wraps keeps the original under `__wrapped__`)."""
    f = _TorchAdam.step
    if getattr(f, "hooked", False):
        f = getattr(f, "__wrapped__", None)
        if f is None:
            raise RuntimeError("aerognn.optim: this torch wraps Optimizer.step without keeping the original "
                               "(`__wrapped__`); torch.optim.Adam's own step cannot be reached without running "
                               "the step hooks twice")
    return f(opt, closure)


def _bump_versions(tensors):
    """The parameters changed in place behind autograd's back: tell its version counters."""
    inc = getattr(torch.autograd.graph, "increment_version", None)
    if inc is None:
        raise RuntimeError("aerognn.optim needs torch.autograd.graph.increment_version (torch >= 2.1)")
    try:
        inc(tensors)
    except TypeError:  # a torch whose increment_version takes one tensor
        for t in tensors:
            inc(t)


def build_chunk_map(numels, chunk) -> np.ndarray:
    """int32 [nchunk, 2] (tensor index, chunk index): every chunk of every tensor once, tensors in
    list order, chunks ascending."""
    numels = np.asarray(numels, dtype=np.int64)
    cnt = (numels + chunk - 1) // chunk
    ti = np.repeat(np.arange(len(numels), dtype=np.int64), cnt)
    first = np.cumsum(cnt) - cnt
    ci = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(first, cnt)
    return np.stack([ti, ci], axis=1).astype(np.int32).reshape(-1, 2)


class _Table:
    """The descriptor table, chunk map and staging buffers of one (device, dtype)."""

    def __init__(self, device, dtype):
        self.device, self.dtype, self.code = device, dtype, _CODES[dtype]
        self.sig = None
        self.flip = 0

    def rebuild(self, sig, pptr, mptr, vptr, numels):
        nt = len(pptr)
        self.nt = nt
        self.pin = [torch.zeros(nt * _DESC.itemsize, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
        self.host = [b.numpy().view(_DESC) for b in self.pin]
        self.events = [torch.cuda.Event(), torch.cuda.Event()]
        self.armed = [False, False]
        for h in self.host:
            h["p"], h["m"], h["v"] = pptr, mptr, vptr
            h["dtype"] = self.code
        self.dev = torch.empty(nt * _DESC.itemsize, dtype=torch.uint8, device=self.device)
        cmap = build_chunk_map(numels, chunk_elems())
        self.nchunk = int(cmap.shape[0])
        self.cmap = torch.from_numpy(np.ascontiguousarray(cmap).reshape(-1)).to(self.device)
        self.sig = sig

    def begin(self):
        """The free half of the staging buffer (a structured view of its descriptors), once the copy
        that last read it (two steps ago) has completed."""
        k = self.flip
        if self.armed[k]:
            self.events[k].synchronize()
        return self.host[k]

    def commit(self):
        """Enqueue the copy of the half begin() handed out on the current stream and guard it."""
        k = self.flip
        self.flip ^= 1
        self.dev.copy_(self.pin[k], non_blocking=True)
        self.events[k].record()
        self.armed[k] = True


class Adam(_TorchAdam):
    """torch.optim.Adam whose step() runs on agn_adam_step where it applies (module docstring).
    `replay = False` (class or instance) partitions the parameters afresh at every step (measurements)."""

    replay = True

    def _covered(self) -> bool:
        for g in self.param_groups:
            if (g.get("amsgrad") or g.get("maximize") or g.get("capturable") or g.get("differentiable")
                    or g.get("decoupled_weight_decay") or g.get("fused")):
                return False
            if torch.is_tensor(g["lr"]) or any(torch.is_tensor(b) for b in g["betas"]):
                return False
        return True

    def _qualifies(self, p) -> bool:
        if not (p.is_cuda and p.dtype in _CODES and p.is_contiguous()):
            return False
        g = p.grad
        if g is not None and (g.is_sparse or g.dtype != p.dtype or g.device != p.device or not g.is_contiguous()):
            return False
        st = self.state.get(p)
        if st:
            m, v, s = st.get("exp_avg"), st.get("exp_avg_sq"), st.get("step")
            for t in (m, v):
                if t is None or t.dtype != p.dtype or t.device != p.device or not t.is_contiguous() \
                        or t.numel() != p.numel():
                    return False
            if not torch.is_tensor(s) or s.is_cuda:
                return False
        return True

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None or not self._covered():
            return _base_step(self, closure)
        plan = self.__dict__.get("_agn_plan") if self.replay else None
        if plan is not None:
            work = self._replay(plan)
            if work is not None:
                for tab, recs, grads in work:
                    with torch.cuda.device(tab.device):
                        self._launch(tab, recs, grads)
                return None
            self._agn_plan = None
        ours, rest = [], False
        for gi, g in enumerate(self.param_groups):
            for p in g["params"]:
                if self._qualifies(p):
                    ours.append((p, gi))
                else:
                    rest = True
        if not ours:
            return _base_step(self)
        if rest:
            # torch's own step on the parameters this module does not cover, the groups otherwise as they are
            mine = {id(p) for p, _ in ours}
            saved = self.param_groups
            self.param_groups = [dict(g, params=[p for p in g["params"] if id(p) not in mine]) for g in saved]
            try:
                _base_step(self)
            finally:
                self.param_groups = saved
        self._device_step(ours, keep_plan=not rest)
        return None

    def _replay(self, plan):
        """The steady state: the parameter list, its storage, its entries in self.state and their tensors
        are those of the last step (checked one by one, before anything is changed), so only the
        gradients are gathered.
        None: something moved, and step() partitions the parameters afresh."""
        state_obj, count, tables = plan
        if state_obj is not self.state or count != sum(len(g["params"]) for g in self.param_groups):
            return None
        strided = torch.strided
        state_get = self.state.get
        work = []
        for tab, recs in tables:
            dt, device = tab.dtype, tab.device
            grads = [r[0].grad for r in recs]
            for (p, _, st, pptr, mptr, vptr, _), g in zip(recs, grads):
                if p.data_ptr() != pptr or p.dtype is not dt or state_get(p) is not st:
                    return None
                if g is None:
                    continue
                if (st is None or g.dtype is not dt or g.layout is not strided or g.device != device
                        or not g.is_contiguous() or st["exp_avg"].data_ptr() != mptr
                        or st["exp_avg_sq"].data_ptr() != vptr or st["step"].is_cuda):
                    return None
            work.append((tab, recs, grads))
        return work

    def _device_step(self, ours, keep_plan):
        tables = self.__dict__.setdefault("_agn_tables", {})
        by_key = {}
        for p, gi in ours:
            by_key.setdefault((p.device, p.dtype), []).append((p, gi))
        planned = []
        for (device, dtype), items in by_key.items():
            tab = tables.get((device, dtype))
            if tab is None:
                tab = tables[(device, dtype)] = _Table(device, dtype)
            with torch.cuda.device(device):
                recs = self._records(tab, items)
                self._launch(tab, recs, [r[0].grad for r in recs])
            planned.append((tab, recs))
        # replayed only when every parameter runs here and has its state (none without a gradient so far)
        if keep_plan and all(r[2] is not None for _, recs in planned for r in recs):
            self._agn_plan = (self.state, sum(len(g["params"]) for g in self.param_groups), planned)

    def _records(self, tab, items):
        """(p, group index, state dict, p / exp_avg / exp_avg_sq pointers, numel) per tensor, creating the
        state of a parameter that has its first gradient as torch.optim.Adam._init_group does; the
        table is rebuilt when the list differs from the one it was built for."""
        state = self.state
        recs = []
        for p, gi in items:
            st = state.get(p)  # no entry is created for a parameter without a gradient (torch creates none)
            if p.grad is not None and not st:
                st = state[p]
                st["step"] = torch.tensor(0.0, dtype=_step_dtype())
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            recs.append((p, gi, st if st else None, p.data_ptr(), st["exp_avg"].data_ptr() if st else 0,
                         st["exp_avg_sq"].data_ptr() if st else 0, p.numel()))
        sig = tuple(r[3:] for r in recs)
        if sig != tab.sig:
            tab.rebuild(sig, [r[3] for r in recs], [r[4] for r in recs], [r[5] for r in recs], [r[6] for r in recs])
        return recs

    def _launch(self, tab, recs, grads):
        live = [i for i, g in enumerate(grads) if g is not None]
        if not live:
            return
        steps = [recs[i][2]["step"] for i in live]
        torch._foreach_add_(steps, 1)
        ts = torch.stack(steps).tolist()
        nt = len(recs)
        same = {}
        for i, t in zip(live, ts):
            same.setdefault((recs[i][1], t), []).append(i)
        h = tab.begin()
        h["n"][...] = 0   # an entry without a gradient is skipped by the kernel
        h["g"][...] = 0
        for (gi, t), idx in same.items():
            g = self.param_groups[gi]
            beta1, beta2 = (float(b) for b in g["betas"])
            lr = float(g["lr"])
            # torch's _single_tensor_adam, in Python doubles
            bias_correction1 = 1 - beta1 ** t
            bias_correction2 = 1 - beta2 ** t
            vals = (beta1, beta2, float(g["eps"]), float(g["weight_decay"] or 0.0), lr / bias_correction1,
                    bias_correction2 ** 0.5)
            sel = slice(None) if len(idx) == nt else np.asarray(idx, dtype=np.int64)
            for name, val in zip(("beta1", "beta2", "eps", "weight_decay", "step_size", "bc2_sqrt"), vals):
                h[name][sel] = val
        li = slice(None) if len(live) == nt else np.asarray(live, dtype=np.int64)
        h["n"][li] = [recs[i][6] for i in live]
        h["g"][li] = [grads[i].data_ptr() for i in live]
        tab.commit()
        from .core import stream
        L.check(L.lib().agn_adam_step(tab.dev.data_ptr(), tab.nt, tab.cmap.data_ptr(), tab.nchunk, tab.code, stream()),
                "adam_step")
        _bump_versions([recs[i][0] for i in live])

    def add_param_group(self, param_group):
        self.__dict__["_agn_plan"] = None
        return super().add_param_group(param_group)
