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

Master weights. `Adam(params, ..., master_weights=True)` (a per-group option; the key is in `defaults`
and `param_groups` only when it is set) is for the reference's `precision: bf16` / `float16`
(train.py:30-38), whose parameters are 16-bit: torch's own step on them keeps p, exp_avg and exp_avg_sq
in 16 bits and rounds most updates away. In such a group a bf16 / fp16 HIP parameter runs on
agn_adam_step_master: its state holds `exp_avg` and `exp_avg_sq` in fp32 and `master_param`, an fp32 copy
of p that the step updates and rounds into p; an element of p that something else wrote restarts from
p (include/aerognn.h). fp32 / fp64 parameters of the group run agn_adam_step as always. Nothing is
downgraded silently: a 16-bit parameter of such a group that cannot run on the kernel and a closure raise
RuntimeError, and the options this module does not cover raise ValueError, at construction and at step().
load_state_dict() keeps the three tensors fp32 (torch's casts state to the parameter's dtype), upcasts
the 16-bit moments of a plain run's checkpoint, and keeps the optimizer's own master_weights flag when the
checkpoint's groups have none.

Loss scaling. `step(scaler=s)` (what aerognn.train.LossScaler.step(optimizer) calls; step() without it is
unchanged) is the step on scaled gradients, in two phases so that no tensor of any table moves unless every
gradient is finite: first every table's descriptors are written and copied, then agn_grad_check reads every
table's gradients and sets the scaler's found_inf flag on the device, then agn_adam_step_scaled /
agn_adam_step_master_scaled run, which return at once when the flag is set and otherwise multiply each
gradient by (float)(1 / S) in front of the unscaled step. Nothing falls back to torch's step, which would
apply the scaled gradients: a parameter with a gradient that does not qualify here (16-bit without
master_weights, CPU, non-contiguous), a closure and an uncovered option raise RuntimeError. The `step`
counters stay on the host, and the host never waits for the step it enqueues: they are incremented as
always, a copy of found_inf to a page-locked word is enqueued behind the check and guarded by an event, and
the NEXT step() (and state_dict() / load_state_dict()) waits for that event and takes the increments of a
skipped step back, by which time the next forward and backward are queued behind it.
"""
from __future__ import annotations

import numpy as np
import torch
from torch.optim.adam import Adam as _TorchAdam

from . import _lib as L

_CODES = {torch.float32: L.F32, torch.float64: L.F64}
_MASTER_CODES = {torch.bfloat16: L.BF16, torch.float16: L.F16}  # parameters of a master_weights group
_DESC = np.dtype(L.AdamDesc)
_MASTER_DESC = np.dtype(L.AdamMasterDesc)
_MASTER_KEYS = ("exp_avg", "exp_avg_sq", "master_param")


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
        self.device, self.dtype = device, dtype
        self.master = dtype in _MASTER_CODES  # agn_adam_master_desc entries, launched by agn_adam_step_master
        self.code = _MASTER_CODES[dtype] if self.master else _CODES[dtype]
        self.desc = _MASTER_DESC if self.master else _DESC
        self.sig = None
        self.flip = 0

    def rebuild(self, sig, pptr, mptr, vptr, numels, wptr):
        nt = len(pptr)
        self.nt = nt
        self.pin = [torch.zeros(nt * self.desc.itemsize, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
        self.host = [b.numpy().view(self.desc) for b in self.pin]
        self.events = [torch.cuda.Event(), torch.cuda.Event()]
        self.armed = [False, False]
        for h in self.host:
            h["p"], h["m"], h["v"] = pptr, mptr, vptr
            if self.master:
                h["w"] = wptr
            h["dtype"] = self.code
        self.dev = torch.empty(nt * self.desc.itemsize, dtype=torch.uint8, device=self.device)
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


def _master_state(p, st):
    """The state of a master-weight parameter as agn_adam_step_master reads it: exp_avg, exp_avg_sq and
    master_param contiguous fp32 on p's device; 16-bit moments are upcast (exact), a missing
    master_param is p in fp32."""
    if st.get("master_param") is None:
        st["master_param"] = p.detach().float()
    for k in _MASTER_KEYS:
        t = st[k]
        if t.dtype != torch.float32 or t.device != p.device or not t.is_contiguous():
            st[k] = t.detach().to(device=p.device, dtype=torch.float32).contiguous()


class _PendingStep:
    """A scaled step whose found_inf copy may still be in flight: the `step` tensors it incremented, the
    page-locked word the flag is copied to and the event behind the copy."""

    def __init__(self, word, event, steps, done):
        self.word, self.event, self.steps, self.done = word, event, steps, done

    def resolve(self):
        """Wait for the copy; a skipped step does not count."""
        if self.steps is None:
            return
        self.event.synchronize()
        if int(self.word[0]) != 0:
            torch._foreach_sub_(self.steps, 1)
        self.steps = None
        self.done(self)


class Adam(_TorchAdam):
    """torch.optim.Adam whose step() runs on agn_adam_step where it applies (module docstring).
    `replay = False` (class or instance) partitions the parameters afresh at every step (measurements)."""

    replay = True

    def __init__(self, params, *args, master_weights=False, **kwargs):
        super().__init__(params, *args, **kwargs)
        if master_weights:
            self.defaults["master_weights"] = True  # add_param_group hands the defaults to a new group
            for g in self.param_groups:
                g.setdefault("master_weights", True)
        self._check_master(None)

    @staticmethod
    def _uncovered(g):
        """The setting of group g that this module does not cover, or None."""
        for k in ("amsgrad", "maximize", "capturable", "differentiable", "decoupled_weight_decay", "fused"):
            if g.get(k):
                return f"{k}={g[k]!r}"
        if torch.is_tensor(g["lr"]):
            return "a tensor lr"
        if any(torch.is_tensor(b) for b in g["betas"]):
            return "a tensor beta"
        return None

    def _covered(self) -> bool:
        return all(self._uncovered(g) is None for g in self.param_groups)

    def _check_master(self, closure) -> bool:
        """True when a group sets master_weights. Such an optimizer never takes torch's step as a whole
        (that would step the 16-bit parameters in 16 bits): what would send it there raises instead."""
        if not any(g.get("master_weights") for g in self.param_groups):
            return False
        for gi, g in enumerate(self.param_groups):
            bad = self._uncovered(g)
            if bad:
                raise ValueError(f"aerognn.optim.Adam: master_weights=True cannot be combined with {bad} (param group "
                                 f"{gi}): that setting runs torch's own step, which keeps 16-bit parameters and "
                                 "their moments in 16 bits")
        if closure is not None:
            raise RuntimeError("aerognn.optim.Adam: master_weights=True does not take a closure: step(closure) runs "
                               "torch's own step, which keeps 16-bit parameters and their moments in 16 bits")
        return True

    def _master_reason(self, p):
        """Why the 16-bit parameter p of a master_weights group cannot run on agn_adam_step_master, or None."""
        if not p.is_cuda:
            return f"it is on {p.device}, not on a HIP device"
        if not p.is_contiguous():
            return "it is not contiguous"
        g = p.grad
        if g is not None:
            if g.is_sparse or g.layout is not torch.strided:
                return "its gradient is sparse"
            if g.dtype != p.dtype or g.device != p.device:
                return f"its gradient is {g.dtype} on {g.device}"
            if not g.is_contiguous():
                return "its gradient is not contiguous"
        st = self.state.get(p)
        if st:
            for k in ("exp_avg", "exp_avg_sq", "master_param"):
                t = st.get(k)
                if k == "master_param" and t is None:
                    continue  # a plain run's checkpoint: created from p at this step
                if not torch.is_tensor(t) or not t.is_floating_point() or t.numel() != p.numel():
                    return f"its state has no {k} of its size"
            if not torch.is_tensor(st.get("step")) or st["step"].is_cuda:
                return "its state's step is not a CPU tensor"
        return None

    def _qualifies(self, p, gi=0, master=False) -> bool:
        if master and p.dtype in _MASTER_CODES:
            why = self._master_reason(p)
            if why:
                g = self.param_groups[gi]
                i = next(i for i, q in enumerate(g["params"]) if q is p)
                name = repr(g["param_names"][i]) if "param_names" in g else f"{i}"
                raise RuntimeError(f"aerognn.optim.Adam(master_weights=True): parameter {name} of group {gi} "
                                   f"({p.dtype}, shape {tuple(p.shape)}) cannot take the master-weight step: {why}")
            return True
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

    def _resolve_pending(self):
        pend = self.__dict__.get("_agn_pending")
        if pend is not None:
            pend.resolve()
            self._agn_pending = None

    def state_dict(self):
        self._resolve_pending()  # the counters of a skipped scaled step are taken back first
        return super().state_dict()

    @torch.no_grad()
    def step(self, closure=None, *, scaler=None):
        self._resolve_pending()
        if scaler is not None:
            return self._scaled_step(closure, scaler)
        if not self._check_master(closure) and (closure is not None or not self._covered()):
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
            master = bool(g.get("master_weights"))
            for p in g["params"]:
                if self._qualifies(p, gi, master):
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

    def _scaled_step(self, closure, scaler):
        """step(scaler=...): module docstring, "Loss scaling". Everything that would run torch's own step
        raises before anything is changed."""
        if closure is not None:
            raise RuntimeError("aerognn.optim.Adam: a loss-scaled step does not take a closure: step(closure) runs "
                               "torch's own step, which would apply the scaled gradients")
        self._check_master(None)
        for gi, g in enumerate(self.param_groups):
            bad = self._uncovered(g)
            if bad:
                raise RuntimeError(f"aerognn.optim.Adam: a loss-scaled step cannot be combined with {bad} (param "
                                   f"group {gi}): that setting runs torch's own step, which would apply the scaled "
                                   "gradients")
        plan = self.__dict__.get("_agn_plan") if self.replay else None
        if plan is not None:
            work = self._replay(plan)
            if work is not None:
                self._scaled_launch(work, scaler)
                return None
            self._agn_plan = None
        ours, rest = [], False
        for gi, g in enumerate(self.param_groups):
            master = bool(g.get("master_weights"))
            for i, p in enumerate(g["params"]):
                if self._qualifies(p, gi, master):
                    ours.append((p, gi))
                elif p.grad is not None:
                    name = repr(g["param_names"][i]) if "param_names" in g else f"{i}"
                    raise RuntimeError(f"aerognn.optim.Adam: parameter {name} of group {gi} ({p.dtype} on {p.device}, "
                                       f"shape {tuple(p.shape)}) cannot take the loss-scaled step on the device "
                                       "(a 16-bit parameter needs master_weights=True; a parameter must be a "
                                       "contiguous HIP tensor with a dense gradient of its dtype), and torch's own "
                                       "step would apply the scaled gradient")
                else:
                    rest = True
        if ours:
            self._device_step(ours, keep_plan=not rest, scaler=scaler)
        return None

    def _replay(self, plan):
        """The steady state: the parameter list, its storage, its entries in self.state and their tensors
        are those of the last step (checked one by one, before anything is changed), so only the
        gradients are gathered.
        None: something moved, and step() partitions the parameters afresh."""
        state_obj, count, flags, tables = plan
        if (state_obj is not self.state or count != sum(len(g["params"]) for g in self.param_groups)
                or flags != [bool(g.get("master_weights")) for g in self.param_groups]):
            return None
        strided = torch.strided
        state_get = self.state.get
        work = []
        for tab, recs in tables:
            dt, device = tab.dtype, tab.device
            grads = [r[0].grad for r in recs]
            for (p, _, st, pptr, mptr, vptr, _, wptr), g in zip(recs, grads):
                if p.data_ptr() != pptr or p.dtype is not dt or state_get(p) is not st:
                    return None
                if g is None:
                    continue
                if (st is None or g.dtype is not dt or g.layout is not strided or g.device != device
                        or not g.is_contiguous() or st["exp_avg"].data_ptr() != mptr
                        or st["exp_avg_sq"].data_ptr() != vptr or st["step"].is_cuda):
                    return None
                if wptr:
                    w = st.get("master_param")
                    if w is None or w.data_ptr() != wptr:
                        return None
            work.append((tab, recs, grads))
        return work

    def _device_step(self, ours, keep_plan, scaler=None):
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
                if scaler is None:
                    self._launch(tab, recs, [r[0].grad for r in recs])
            planned.append((tab, recs))
        if scaler is not None:  # every table has its state and its records: check all, then step all
            self._scaled_launch([(tab, recs, [r[0].grad for r in recs]) for tab, recs in planned], scaler)
        # replayed only when every parameter runs here and has its state (none without a gradient so far)
        if keep_plan and all(r[2] is not None for _, recs in planned for r in recs):
            self._agn_plan = (self.state, sum(len(g["params"]) for g in self.param_groups),
                              [bool(g.get("master_weights")) for g in self.param_groups], planned)

    def _records(self, tab, items):
        """(p, group index, state dict, p / exp_avg / exp_avg_sq pointers, numel, master_param pointer or
        0) per tensor, creating the state of a parameter that has its first gradient as
        torch.optim.Adam._init_group does (a master table: fp32 moments and master_param = p in fp32; state
        that a plain run left is upcast, which is exact); the table is rebuilt when the list differs from
        the one it was built for."""
        state = self.state
        recs = []
        for p, gi in items:
            st = state.get(p)  # no entry is created for a parameter without a gradient (torch creates none)
            if p.grad is not None and not st:
                st = state[p]
                dt = torch.float32 if tab.master else p.dtype
                st["step"] = torch.tensor(0.0, dtype=_step_dtype())
                st["exp_avg"] = torch.zeros_like(p, dtype=dt, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, dtype=dt, memory_format=torch.preserve_format)
            if st and tab.master:
                _master_state(p, st)
            recs.append((p, gi, st if st else None, p.data_ptr(), st["exp_avg"].data_ptr() if st else 0,
                         st["exp_avg_sq"].data_ptr() if st else 0, p.numel(),
                         st["master_param"].data_ptr() if st and tab.master else 0))
        sig = tuple(r[3:] for r in recs)
        if sig != tab.sig:
            tab.rebuild(sig, *([r[k] for r in recs] for k in (3, 4, 5, 6, 7)))
        return recs

    def _scaled_launch(self, work, scaler):
        """The two phases of a loss-scaled step over `work` = [(table, records, gradients)]."""
        state = scaler._device_state(work[0][0].device)
        for tab, _, _ in work:
            if tab.device != state.device:
                raise RuntimeError(f"aerognn.optim.Adam: the LossScaler's state is on {state.device}, a parameter "
                                   f"table on {tab.device}")
        sp, lib = state.data_ptr(), L.lib()
        from .core import stream
        with torch.cuda.device(state.device):
            fired, steps = [], []
            for tab, recs, grads in work:
                live = self._fill(tab, recs, grads)
                if live:
                    fired.append((tab, recs, live))
                    steps += [recs[i][2]["step"] for i in live]
            if not fired:
                return
            for tab, _, _ in fired:
                L.check(lib.agn_grad_check(tab.dev.data_ptr(), int(tab.master), tab.nt, tab.cmap.data_ptr(), tab.nchunk,
                                           tab.code, sp, stream()), "grad_check")
            self._agn_pending = scaler._watch(steps)
            for tab, recs, live in fired:
                self._fire(tab, recs, live, sp)

    def _launch(self, tab, recs, grads):
        live = self._fill(tab, recs, grads)
        if live:
            self._fire(tab, recs, live)

    def _fill(self, tab, recs, grads):
        """The host half of a table's step: the counters of the tensors with a gradient go up by one, their
        descriptors are written and the copy is enqueued. Returns their indices (empty: nothing to run)."""
        live = [i for i, g in enumerate(grads) if g is not None]
        if not live:
            return live
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
        return live

    def _fire(self, tab, recs, live, scale_state=None):
        """The launch over a committed table; scale_state: the device address of a LossScaler's state."""
        from .core import stream
        lib = L.lib()
        args = (tab.dev.data_ptr(), tab.nt, tab.cmap.data_ptr(), tab.nchunk, tab.code)
        if scale_state is None:
            fn = lib.agn_adam_step_master if tab.master else lib.agn_adam_step
            L.check(fn(*args, stream()), "adam_step_master" if tab.master else "adam_step")
        else:
            fn = lib.agn_adam_step_master_scaled if tab.master else lib.agn_adam_step_scaled
            L.check(fn(*args, scale_state, stream()), "adam_step_master_scaled" if tab.master else "adam_step_scaled")
        _bump_versions([recs[i][0] for i in live])

    def add_param_group(self, param_group):
        self.__dict__["_agn_plan"] = None
        return super().add_param_group(param_group)

    def load_state_dict(self, state_dict):
        """torch's load_state_dict, then the fp32 state of master-weight parameters put back from
        `state_dict` itself: torch casts every floating state tensor but `step` to the parameter's dtype
        (through a call bound to Optimizer, which a subclass cannot replace). A group that had
        master_weights keeps it when the checkpoint's group has no such key (a plain run's)."""
        self._resolve_pending()
        had = [g.get("master_weights") for g in self.param_groups]
        super().load_state_dict(state_dict)
        for g, flag, saved in zip(self.param_groups, had, state_dict["param_groups"]):
            if flag is not None:
                g.setdefault("master_weights", flag)
            if not g.get("master_weights"):
                continue
            for p, pid in zip(g["params"], saved["params"]):
                src, st = state_dict["state"].get(pid), self.state.get(p)
                if not src or not st or p.dtype not in _MASTER_CODES:
                    continue
                for k in _MASTER_KEYS:
                    t = src.get(k)
                    if torch.is_tensor(t) and t.is_floating_point():
                        st[k] = t.detach().to(device=p.device, dtype=torch.float32)

    def master_parameters(self):
        """(param, master_param) of every parameter that has fp32 master weights so far: the weights to
        export from a 16-bit run."""
        for g in self.param_groups:
            if g.get("master_weights"):
                for p in g["params"]:
                    w = self.state.get(p, {}).get("master_param")
                    if w is not None:
                        yield p, w
