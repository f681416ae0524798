"""Dynamic loss scaling on the MI355X ("Loss scaling"): agn_mse_loss_scaled, agn_grad_check,
agn_adam_step_scaled / agn_adam_step_master_scaled, agn_loss_scale_update and aerognn.train.LossScaler.

Every comparison is exact (integer views), so there is no tolerance:
  loss     dpred is bitwise round_T(((2 d) / n_global) * S) of the fp64 formula (numpy); the loss value and the
           accumulator have the bytes of the unscaled call; a null state gives agn_mse_loss's bytes.
  check    one +inf, -inf or NaN at the first / last element, on both sides of a chunk edge, in the scalar
           tail and only in the last tensor sets found_inf; the largest finite value and subnormals do not;
           entries agn_adam_step skips are not read.
  skip     a step with one inf moves no tensor of any table and does not count.
  identity (master_param, exp_avg, exp_avg_sq) after scaled steps on g are bitwise the fp32 shadow's on
           g.float() * inv, inv = (float)(1 / S); fp32 / fp64 tables against their own unscaled run on g * inv.
  update   scale and tracker after every call are bitwise torch._amp_update_scale_'s.
Two cases differ from the wording of the request that asked for them, because its arithmetic does not hold:
  * pred - y = 2^10 with S = 2^16 overflows fp16 at n_global = n f = 2^8 (dpred = 2^19), not at 2^22 (2^5): the
    overflow case uses the default count.
  * from init_scale = 2^40 nothing is skipped at first: dpred = 2^-26 * 2^40 = 2^14 is finite in fp16. The
    described behaviour (the first steps skipped, the scale backs off until a step applies) is asserted from
    2^44 (2^18, 2^17 and 2^16 overflow, 2^15 applies: exactly three skips), and 2^40 is run with
    growth_interval = 1, where the scale grows into the overflow and backs off: steps_skipped() > 0 there too."""
import copy
import functools

import numpy as np
import pytest
import torch
from torch import nn

from aerognn import _lib as L
from aerognn import optim as agn_optim
from aerognn import train as agn_train
from aerognn.core import dt_code, stream
from test_gpu_config_experiments import CFG, build, run_model
from test_gpu_master_adam import (KEYS, LRS, SKIP_AT, SKIPPED, T16, bits, make_params, mixed_optimizer, mixed_problem,
                                  rounded, set_grads)
from test_gpu_train_tail import DTYPES, INT_VIEW, Batch, two_batches

pytestmark = pytest.mark.gpu

DEV = "cuda"
NG = 2 ** 22
STATE = np.dtype(L.LossScaleState)


def raw_state(scale=1.0, found_inf=0, tracker=0, skipped=0, rows=1):
    """`rows` agn_loss_scale_state on the device as int32 [rows, 4]."""
    h = np.zeros(rows, dtype=STATE)
    h["scale"], h["found_inf"], h["growth_tracker"], h["skipped"] = scale, found_inf, tracker, skipped
    return torch.from_numpy(h.view(np.int32).reshape(rows, 4).copy()).to(DEV)


def read_state(t):
    return t.cpu().numpy().reshape(-1).view(STATE)


def inv_of(S):
    """(float)(1 / (double)S) as a float32 device tensor: GradScaler's inv_scale."""
    return torch.tensor(float(S), dtype=torch.float64).reciprocal().float().to(DEV)


# ----------------------------------------------------------------------------- 1. the loss kernel
def ref_scaled_dpred(pred_cpu, y_cpu, n_global, S):
    d = pred_cpu.double().numpy() - y_cpu.double().numpy()
    q = ((2.0 * d) / np.float64(n_global)) * np.float64(np.float32(S))
    if pred_cpu.dtype == torch.float64:
        return torch.from_numpy(q)
    with np.errstate(over="ignore"):
        return torch.from_numpy(q.astype(np.float32)).to(pred_cpu.dtype)


def fp16_pair(delta):
    """64 x 4 fp16: y = m delta, m in [-32, 32), pred = y +- delta with alternating signs (all exact; delta a
    power of two)."""
    k = torch.arange(256).reshape(64, 4)
    y = ((k % 64) - 32).double() * delta
    sign = torch.where((k + k // 4) % 2 == 0, 1.0, -1.0).double()
    pred = y + sign * delta
    assert torch.equal(pred.half().double(), pred) and torch.equal(y.half().double(), y)
    return pred.half().to(DEV), y.half().to(DEV), sign


def test_loss_kernel_scales_before_it_rounds():
    pred, y, sign = fp16_pair(2.0 ** -5)
    acc0 = torch.zeros((), dtype=torch.float64, device=DEV)
    loss0, dp0 = agn_train.mse_loss_grad(pred, y, n_global=NG, acc=acc0)
    assert bool((dp0 == 0).all())  # the defect: 2^-26 is under half of fp16's smallest subnormal
    s = agn_train.LossScaler(init_scale=2.0 ** 16)
    acc1 = torch.zeros((), dtype=torch.float64, device=DEV)
    loss1, dp1 = agn_train.mse_loss_grad(pred, y, n_global=NG, acc=acc1, scaler=s)
    assert dp1.dtype == torch.float16 and torch.equal(dp1.cpu().double(), sign * 2.0 ** -10)
    assert torch.equal(bits(loss0), bits(loss1)) and torch.equal(bits(acc0), bits(acc1)) and float(loss0) > 0.0
    assert s.get_scale() == 65536.0 and s.steps_skipped() == 0  # the loss kernel only reads the state
    # MSELoss hands the same gradient to pred, and its value is the unscaled one
    leaf = pred.clone().requires_grad_(True)
    lm = agn_train.MSELoss()(leaf, y, NG, s)
    lm.backward()
    assert torch.equal(bits(lm), bits(loss0)) and torch.equal(bits(leaf.grad), bits(dp1))
    # overflow: (2 * 2^10 / 2^8) * 2^16 = 2^19 is +-inf in fp16 (module docstring: at the default count)
    pred, y, sign = fp16_pair(2.0 ** 10)
    lossu, dpu = agn_train.mse_loss_grad(pred, y)
    assert bool(torch.isfinite(dpu).all())
    losso, dpo = agn_train.mse_loss_grad(pred, y, scaler=s)
    assert bool(torch.isinf(dpo).all()) and torch.equal(torch.sign(dpo).cpu().double(), sign)
    assert torch.equal(bits(losso), bits(lossu))


def raw_mse(fn, pred, y, n_global, state):
    n, f = pred.shape
    loss = torch.empty((), dtype=torch.float64, device=DEV)
    acc = torch.zeros((), dtype=torch.float64, device=DEV)
    dp = torch.empty_like(pred)
    scr = torch.empty(max(int(L.lib().agn_mse_loss_temp_bytes(n, f)), 16), dtype=torch.uint8, device=DEV)
    args = (dt_code(pred.dtype), dt_code(y.dtype), n, f, L.ptr(pred), f, L.ptr(y), f, float(n_global), L.ptr(loss),
            L.ptr(acc), L.ptr(dp), f, L.ptr(scr))
    L.check(fn(*args, stream()) if state is None else fn(*args, state, stream()), "mse")
    return loss, acc, dp


@pytest.mark.parametrize("name", sorted(DTYPES))
def test_scaled_gradient_is_the_fp64_formula(name):
    dtype, iv = DTYPES[name], INT_VIEW[DTYPES[name]]
    lib = L.lib()
    c = agn_train.chunk_rows()
    assert c == 2048
    for i, n in enumerate((1, c - 1, c, c + 1)):
        g = torch.Generator().manual_seed(50 + i)
        pred_cpu, y_cpu = torch.randn(n, 4, generator=g).to(dtype), torch.randn(n, 4, generator=g).to(dtype)
        pred, y = pred_cpu.to(DEV), y_cpu.to(DEV)
        base = raw_mse(lib.agn_mse_loss, pred, y, 4 * n, None)
        null = raw_mse(lib.agn_mse_loss_scaled, pred, y, 4 * n, 0)  # a null state: agn_mse_loss's bytes
        for a, b in zip(base, null):
            assert torch.equal(bits(a), bits(b)), (name, n)
        for S in (1.0, 16.0):
            st = raw_state(S, tracker=3, skipped=2)
            loss, acc, dp = raw_mse(lib.agn_mse_loss_scaled, pred, y, 4 * n, st.data_ptr())
            want = ref_scaled_dpred(pred_cpu, y_cpu, 4 * n, S)
            assert torch.equal(dp.cpu().view(iv), want.view(iv)), (name, n, S)
            assert torch.equal(bits(loss), bits(base[0])) and torch.equal(bits(acc), bits(base[1])), (name, n, S)
            if S == 1.0:
                assert torch.equal(bits(dp), bits(base[2])), (name, n)
            assert read_state(st).tolist() == [(S, 0, 3, 2)]  # only read
            l2, d2 = agn_train.mse_loss_grad(pred, y, scaler=agn_train.LossScaler(init_scale=S))
            assert torch.equal(bits(d2), bits(dp)) and torch.equal(bits(l2), bits(loss))


# ----------------------------------------------------------------------------- 2. the check kernel
def check_sizes():
    c = agn_optim.chunk_elems()
    return [1, 7, 8, 9, c - 1, c, c + 1, 2 * c + 7]


def raw_table(master, code, grads, dummy):
    """A descriptor table over `grads` (None: an entry without a gradient) and its chunk map, on the device.
    p, m, v (and w) point at `dummy`, which agn_grad_check never reads."""
    h = np.zeros(len(grads), dtype=np.dtype(L.AdamMasterDesc if master else L.AdamDesc))
    for k in ("p", "m", "v") + (("w",) if master else ()):
        h[k] = dummy.data_ptr()
    h["dtype"] = code
    for i, g in enumerate(grads):
        if g is not None:
            h["g"][i], h["n"][i] = g.data_ptr(), g.numel()
    return h


def upload(h, numels):
    cmap = agn_optim.build_chunk_map(numels, agn_optim.chunk_elems())
    return (torch.from_numpy(h.view(np.uint8).copy()).to(DEV), torch.from_numpy(cmap.reshape(-1).copy()).to(DEV),
            int(cmap.shape[0]))


def run_check(tab, master, nt, cmap, nchunk, code, state_ptr):
    L.check(L.lib().agn_grad_check(tab.data_ptr(), int(master), nt, cmap.data_ptr(), nchunk, code, state_ptr, stream()),
            "grad_check")


def plant_positions(n, c, w):
    pos = {0, n - 1}
    for k in (1, 2):
        if n > k * c:
            pos |= {k * c - 1, k * c}  # the last element of a chunk and the first of the next
    if n % w:
        pos.add((n // w) * w)          # the first element of the scalar tail
    return sorted(pos)


@pytest.mark.parametrize("master", [False, True])
@pytest.mark.parametrize("name", sorted(DTYPES))
def test_check_finds_every_planted_value(name, master):
    dtype = DTYPES[name]
    code, c, w = dt_code(dtype), agn_optim.chunk_elems(), 16 // torch.empty((), dtype=dtype).element_size()
    gen = torch.Generator().manual_seed(7)
    grads, keep = [], []
    for n in check_sizes():
        grads.append(torch.randn(n, generator=gen).to(dtype).to(DEV))
    for off, n in ((1, 67), (4, 70)):  # views one and four elements into a buffer
        buf = torch.randn(off + n + 3, generator=gen).to(dtype).to(DEV)
        keep.append(buf)
        grads.append(buf[off:off + n])
        assert grads[-1].data_ptr() % 16 == (off * buf.element_size()) % 16
    grads.append(torch.randn(65, generator=gen).to(dtype).to(DEV))  # the last tensor of the table
    dummy = torch.zeros(16, dtype=torch.uint8, device=DEV)
    numels = [g.numel() for g in grads]
    tab, cmap, nchunk = upload(raw_table(master, code, grads, dummy), numels)
    plants = [(i, p, v) for i, g in enumerate(grads) for p in plant_positions(g.numel(), c, w)
              for v in (float("inf"), float("-inf"), float("nan"))]
    assert any(i == len(grads) - 1 for i, _, _ in plants)
    states = raw_state(4.0, tracker=5, skipped=9, rows=len(plants) + 1)
    base = states.data_ptr()
    run_check(tab, master, len(grads), cmap, nchunk, code, base)  # row 0: the clean gradients
    for r, (i, p, v) in enumerate(plants, start=1):
        old = grads[i][p].clone()
        grads[i][p] = v
        run_check(tab, master, len(grads), cmap, nchunk, code, base + 16 * r)
        grads[i][p] = old
    got = read_state(states)
    assert got[0].tolist() == (4.0, 0, 5, 9)
    for r, (i, p, v) in enumerate(plants, start=1):
        assert got[r].tolist() == (4.0, 1, 5, 9), (name, master, numels[i], p, v)  # the flag, and nothing else
    assert int(dummy.sum()) == 0


@pytest.mark.parametrize("master", [False, True])
@pytest.mark.parametrize("name", sorted(DTYPES))
def test_check_passes_finite_values_and_skips_dead_entries(name, master):
    dtype = DTYPES[name]
    code, c = dt_code(dtype), agn_optim.chunk_elems()
    fi = torch.finfo(dtype)
    edge = torch.tensor([fi.max, -fi.max, fi.smallest_normal, -fi.smallest_normal, 0.0, -0.0], dtype=torch.float64)
    sub = torch.tensor([1, 2, 3], dtype=INT_VIEW[dtype]).view(dtype)  # the three smallest subnormals, by pattern
    assert bool((sub.double() > 0).all()) and float(sub.double().max()) < fi.smallest_normal
    vals = torch.cat([edge.to(dtype), sub, -sub])
    assert bool(torch.isfinite(vals).all()) and float(vals.double().max()) == fi.max
    finite = [vals.repeat((n + len(vals) - 1) // len(vals))[:n].contiguous().to(DEV) for n in (1, 9, c + 1, 2 * c + 7)]
    dummy = torch.zeros(16, dtype=torch.uint8, device=DEV)
    states = raw_state(2.0, rows=4)
    tab, cmap, nchunk = upload(raw_table(master, code, finite, dummy), [g.numel() for g in finite])
    run_check(tab, master, len(finite), cmap, nchunk, code, states.data_ptr())
    # entries the step skips are not read: their buffers hold inf
    poison = [torch.full((n,), float("inf"), dtype=dtype, device=DEV) for n in (9, c + 1, 70, 33)]
    h = raw_table(master, code, [finite[1]] + poison, dummy)
    numels = [9, 9, c + 1, 70, 33]
    h["n"][1] = 0                                          # a parameter whose .grad is None: the stale pointer stays
    h["dtype"][2] = L.F32 if code != L.F32 else L.F64      # another dtype's entry
    h["m"][3] = 0                                          # a null pointer
    tab2, cmap2, nchunk2 = upload(h, numels)
    bad_map = cmap2.clone().view(-1, 2)
    assert bad_map[-1, 0] == 4
    bad_map[-1, 0] = 5                                     # tensor 4 only through a map entry outside the table
    run_check(tab2, master, 5, bad_map.view(-1), nchunk2, code, states.data_ptr() + 16)
    # a table with no live gradient
    tab3, cmap3, nchunk3 = upload(raw_table(master, code, [None, None], dummy), [9, c + 1])
    run_check(tab3, master, 2, cmap3, nchunk3, code, states.data_ptr() + 32)
    # the poisoned entries do count once they are live (the control for the three cases above)
    tab4, cmap4, nchunk4 = upload(raw_table(master, code, [finite[1]] + poison, dummy), numels)
    run_check(tab4, master, 5, cmap4, nchunk4, code, states.data_ptr() + 48)
    assert [int(r["found_inf"]) for r in read_state(states)] == [0, 0, 0, 1]


def test_a_parameter_without_a_gradient_is_not_read():
    """Through the optimizer: the gradient buffer of the step before holds inf now, and p.grad is None."""
    ps = [nn.Parameter(torch.ones(70, dtype=torch.float16, device=DEV)) for _ in range(2)]
    opt = agn_optim.Adam(ps, lr=1e-3, master_weights=True)
    s = agn_train.LossScaler(init_scale=4.0)
    stale = torch.ones(70, dtype=torch.float16, device=DEV)
    ps[0].grad, ps[1].grad = stale, torch.ones(70, dtype=torch.float16, device=DEV)
    s.step(opt)
    s.update()
    stale.fill_(float("inf"))
    before = ps[1].detach().clone()
    ps[0].grad, ps[1].grad = None, torch.ones(70, dtype=torch.float16, device=DEV)
    s.step(opt)
    s.update()
    assert s.steps_skipped() == 0 and bool((ps[1] != before).all())
    sd = opt.state_dict()
    assert float(sd["state"][0]["step"]) == 1.0 and float(sd["state"][1]["step"]) == 2.0


# ----------------------------------------------------------------------------- 3. a skipped step
def snapshot(params, opt):
    out = []
    for p in params:
        st = opt.state.get(p, {})
        out.append({"p": bits(p), **{k: bits(st[k]) for k in KEYS if k in st}})
    return out


def assert_unmoved(params, opt, before, steps):
    after = snapshot(params, opt)
    for i, (a, b) in enumerate(zip(before, after)):
        assert sorted(a) == sorted(b), i
        for k in a:
            assert torch.equal(a[k], b[k]), (i, k)
    sd = opt.state_dict()  # resolves the skipped step's counters
    for i, p in enumerate(params):
        assert float(opt.state[p]["step"]) == steps and float(sd["state"][i]["step"]) == steps, i
        assert opt.state[p]["step"].device.type == "cpu"


@pytest.mark.parametrize("first", [False, True])
def test_one_inf_skips_every_table(first):
    specs, start, grads = mixed_problem(2)
    ps, opt = mixed_optimizer(agn_optim.Adam, specs, start, lambda dt: dt, master_weights=True)
    s = agn_train.LossScaler(init_scale=2.0 ** 10)
    if not first:  # one clean step first: the skipped one then runs through the replayed plan
        set_grads(ps, grads, 0)
        s.step(opt)
        s.update()
        assert opt._agn_plan is not None
    victim = [i for i, sp in enumerate(specs) if sp[1] == torch.float16][-1]  # in the last fp16 tensor
    set_grads(ps, grads, 1)
    ps[victim].grad.view(-1)[specs[victim][2][0] // 2] = float("inf")
    if first:      # the state a first step creates (zeros, master_param = p) is what must stay
        before = [{"p": bits(p), "master_param": bits(p.detach().float()), "exp_avg": bits(torch.zeros_like(p).float()),
                   "exp_avg_sq": bits(torch.zeros_like(p).float())} if p.dtype in T16.values() else
                  {"p": bits(p), "exp_avg": bits(torch.zeros_like(p)), "exp_avg_sq": bits(torch.zeros_like(p))} for p in ps]
    else:
        before = snapshot(ps, opt)
    s.step(opt)
    s.update()
    tabs = opt.__dict__["_agn_tables"]
    assert {t.dtype: t.master for t in tabs.values()} == {torch.bfloat16: True, torch.float16: True,
                                                          torch.float32: False, torch.float64: False}
    assert_unmoved(ps, opt, before, 0.0 if first else 1.0)
    assert s.get_scale() == 2.0 ** 9 and s.steps_skipped() == 1
    assert s.state_dict()["_growth_tracker"] == 0
    assert int(read_state(s._device_state())["found_inf"][0]) == 0  # update() cleared it


# ----------------------------------------------------------------------------- 4. identity with the unscaled step
SCALES = (1.0, 0.25, 1024.0, 98304.0)


def scaled_grads(shape, i, nsteps, gen, dt, S):
    """T-exact gradients of magnitude ~ 10^(i % 5 - 3) * 2^-6 * S with exact zeros, |g| within dt's normal
    range or 0 (at most half the largest finite value)."""
    fi = torch.finfo(dt)
    out = []
    for _ in range(nsteps):
        t = torch.randn(shape, generator=gen).double() * 10.0 ** ((i % 5) - 3) * 2.0 ** -6 * S
        if t.numel() > 4:
            t.view(-1)[::5] = 0.0
        t = rounded(t.clamp(-fi.max / 2, fi.max / 2), dt)
        t[t.abs() < fi.smallest_normal] = 0.0
        out.append(t)
    return out


@functools.lru_cache(maxsize=None)
def scaled_problem(name, S):
    dt = T16[name]
    c = agn_optim.chunk_elems()
    specs = [((n,), "plain") for n in (1, 7, 8, 9, 63, c - 1, c, c + 1, 2 * c + 7)] + [((40, 40), "plain")]
    specs += [((67,), "view1"), ((70,), "view4"), ((9,), "nograd"), ((0,), "empty")]
    gen = torch.Generator().manual_seed(5)
    start, grads = [], []
    for i, (shape, kind) in enumerate(specs):
        start.append(rounded(torch.randn(shape, generator=gen), dt))
        gs = scaled_grads(shape, i, len(LRS), gen, dt, S)
        grads.append(None if kind == "nograd" else gs)
    return specs, start, grads


@pytest.mark.parametrize("S", SCALES)
@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("name", sorted(T16))
def test_identity_with_the_unscaled_step_on_g_times_inv(name, wd, S):
    dt = T16[name]
    specs, start, grads = scaled_problem(name, S)
    inv = inv_of(S)
    po, bufs = make_params(specs, start, dt)
    oo = agn_optim.Adam(po, lr=LRS[0], weight_decay=wd, master_weights=True)
    ps, _ = make_params(specs, start, torch.float32)
    os_ = agn_optim.Adam(ps, lr=LRS[0], weight_decay=wd)
    s = agn_train.LossScaler(init_scale=S)
    for k, lr in enumerate(LRS):
        skip = (SKIPPED,) if k == SKIP_AT else ()
        oo.param_groups[0]["lr"] = os_.param_groups[0]["lr"] = lr
        set_grads(po, grads, k, skip)
        for i, (q, gs) in enumerate(zip(ps, grads)):
            q.grad = None if (gs is None or i in skip) else gs[k].float().to(DEV) * inv
        s.step(oo)
        s.update()
        os_.step()
        for i, (p, q) in enumerate(zip(po, ps)):
            assert (p in oo.state) == (q in os_.state), (k, i)
            if p not in oo.state:
                continue
            st, ss = oo.state[p], os_.state[q]
            for key, y in zip(KEYS, (q, ss["exp_avg"], ss["exp_avg_sq"])):
                assert st[key].dtype == torch.float32 and torch.equal(bits(st[key]), bits(y)), (k, i, specs[i], key)
            assert torch.equal(bits(p), bits(st["master_param"].to(dt))), (k, i)
    assert s.steps_skipped() == 0 and s.get_scale() == S
    oo.state_dict()
    for i, (p, q) in enumerate(zip(po, ps)):
        if grads[i] is None:
            assert p not in oo.state and torch.equal(bits(p), bits(start[i].to(dt)))
        else:
            assert torch.equal(oo.state[p]["step"], os_.state[q]["step"])
            assert float(oo.state[p]["step"]) == len(LRS) - (1 if i == SKIPPED else 0)
    for i, (buf, off, n) in bufs.items():  # the elements around the two views are not written
        assert float(buf[:off].abs().max()) == 0.0 and float(buf[off + n:].abs().max()) == 0.0, specs[i]
    assert [(t.dtype, t.master) for t in oo._agn_tables.values()] == [(dt, True)]


@pytest.mark.parametrize("S", SCALES)
@pytest.mark.parametrize("name", ["f32", "f64"])
def test_fp32_and_fp64_tables_against_their_unscaled_run(name, S):
    dt = DTYPES[name]
    c = agn_optim.chunk_elems()
    gen = torch.Generator().manual_seed(11)
    shapes = [(1,), (3,), (4,), (5,), (65,), (c - 1,), (c + 1,), (2 * c + 7,)]
    start = [torch.randn(sh, generator=gen).to(dt) for sh in shapes]
    grads = [scaled_grads(sh, i, len(LRS), gen, dt, S) for i, sh in enumerate(shapes)]
    inv = inv_of(S).to(dt)  # the float32 value, exactly, in the table's compute type
    pa = [nn.Parameter(t.clone().to(DEV)) for t in start]
    pb = [nn.Parameter(t.clone().to(DEV)) for t in start]
    view = torch.zeros(68, dtype=dt, device=DEV)
    pa.append(nn.Parameter(view[1:]))  # the scalar path
    pb.append(nn.Parameter(torch.zeros(67, dtype=dt, device=DEV)))
    grads.append(scaled_grads((67,), 3, len(LRS), gen, dt, S))
    oa = agn_optim.Adam(pa, lr=LRS[0], weight_decay=1e-2)
    ob = agn_optim.Adam(pb, lr=LRS[0], weight_decay=1e-2)
    s = agn_train.LossScaler(init_scale=S)
    for k, lr in enumerate(LRS):
        oa.param_groups[0]["lr"] = ob.param_groups[0]["lr"] = lr
        for i, (a, b) in enumerate(zip(pa, pb)):
            skip = k == SKIP_AT and i == 2
            a.grad = None if skip else grads[i][k].to(dt).to(DEV)
            b.grad = None if skip else grads[i][k].to(dt).to(DEV) * inv
        s.step(oa)
        s.update()
        ob.step()
        for i, (a, b) in enumerate(zip(pa, pb)):
            assert torch.equal(bits(a), bits(b)), (k, i)
            for key in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(bits(oa.state[a][key]), bits(ob.state[b][key])), (k, i, key)
    oa.state_dict()
    for i, (a, b) in enumerate(zip(pa, pb)):
        assert torch.equal(oa.state[a]["step"], ob.state[b]["step"]), i
    assert float(view[0]) == 0.0 and s.steps_skipped() == 0


@pytest.mark.parametrize("replay", [True, False])
def test_five_steps_with_an_inf_at_the_third_are_the_four_clean_steps(replay):
    """Gradients are base_k * S_k with S_k the scale in force (2^4, and 2^3 after the skip): g * inv is base_k
    exactly, so the scaled run must leave the state of an unscaled run of the same class over the four clean
    steps, counters included."""
    specs, start, base = mixed_problem(5)
    po, oo = mixed_optimizer(agn_optim.Adam, specs, start, lambda dt: dt, master_weights=True)
    pc, oc = mixed_optimizer(agn_optim.Adam, specs, start, lambda dt: dt, master_weights=True)
    oo.replay = replay
    s = agn_train.LossScaler(init_scale=16.0)
    plans = []
    for k in range(5):
        S = 16.0 if k <= 2 else 8.0
        for p, gs in zip(po, base):
            p.grad = (gs[k] * S).to(p.dtype).to(DEV)
            assert bool(torch.isfinite(p.grad).all())
        if k == 2:
            po[0].grad.view(-1)[-1] = float("inf")
        s.step(oo)
        s.update()
        plans.append(oo.__dict__.get("_agn_plan"))
        if k != 2:
            set_grads(pc, base, k)
            oc.step()
    if replay:
        assert plans[0] is not None and all(p is plans[0] for p in plans)
    else:
        assert len({id(p) for p in plans}) == 5
    assert s.steps_skipped() == 1 and s.get_scale() == 8.0
    sd, sc = oo.state_dict(), oc.state_dict()
    for i, (p, q) in enumerate(zip(po, pc)):
        assert torch.equal(bits(p), bits(q)), i
        assert sorted(oo.state[p]) == sorted(oc.state[q])
        for key in oo.state[p]:
            assert torch.equal(bits(oo.state[p][key]), bits(oc.state[q][key])), (i, key)
        assert float(sd["state"][i]["step"]) == float(sc["state"][i]["step"]) == 4.0


# ----------------------------------------------------------------------------- 5. the scale update
@pytest.mark.parametrize("growth,backoff", [(2.0, 0.5), (1.5, 0.75)])
def test_scale_update_is_torchs(growth, backoff):
    lib = L.lib()
    seq = (0, 0, 1, 0, 0, 0, 1, 1, 0, 0)
    st = raw_state(2.0 ** 16)
    scale = torch.full((1,), 2.0 ** 16, device=DEV)
    tracker = torch.zeros(1, dtype=torch.int32, device=DEV)
    skipped, seen = 0, set()
    for k, f in enumerate(seq):
        st[0, 1] = f
        L.check(lib.agn_loss_scale_update(st.data_ptr(), growth, backoff, 2, stream()), "update")
        torch._amp_update_scale_(scale, tracker, torch.full((1,), float(f), device=DEV), growth, backoff, 2)
        skipped += f
        got = read_state(st)[0]
        assert np.float32(got["scale"]).view(np.int32) == int(bits(scale)[0]), (k, float(got["scale"]), float(scale))
        assert (int(got["growth_tracker"]), int(got["found_inf"]), int(got["skipped"])) == (int(tracker), 0, skipped), k
        seen.add(float(got["scale"]))
    assert min(seen) < 2.0 ** 16 < max(seen)  # the sequence grew and backed off
    # a growth that would overflow: the scale stays, the tracker goes to 0
    st = raw_state(3e38, tracker=1)
    scale, tracker = torch.full((1,), 3e38, device=DEV), torch.ones(1, dtype=torch.int32, device=DEV)
    L.check(lib.agn_loss_scale_update(st.data_ptr(), growth, backoff, 2, stream()), "update")
    torch._amp_update_scale_(scale, tracker, torch.zeros(1, device=DEV), growth, backoff, 2)
    got = read_state(st)[0]
    assert np.float32(got["scale"]) == np.float32(3e38) and int(got["growth_tracker"]) == 0 == int(tracker)
    assert np.float32(got["scale"]).view(np.int32) == int(bits(scale)[0])
    # LossScaler.update() is that call, and its state dict moves to a GradScaler and back
    s = agn_train.LossScaler(DEV, init_scale=8.0, growth_factor=growth, backoff_factor=backoff, growth_interval=2)
    s.update()
    s.update()
    assert s.get_scale() == 8.0 * growth and s.state_dict()["_growth_tracker"] == 0
    s.update()
    g = torch.amp.GradScaler("cuda")
    g.load_state_dict(s.state_dict())
    assert g.state_dict() == s.state_dict() and g.state_dict()["_growth_tracker"] == 1
    s2 = agn_train.LossScaler(DEV)
    s2.update()  # the device state exists before the load
    s2.load_state_dict(g.state_dict())
    assert s2.state_dict() == s.state_dict() and s2.get_scale() == 8.0 * growth


# ----------------------------------------------------------------------------- 6. it trains
def train_leaf(scaler, steps=20):
    pred0, y, _ = fp16_pair(2.0 ** -5)
    pred = nn.Parameter(pred0.clone())
    opt = agn_optim.Adam([pred], lr=1e-3, master_weights=True)
    for _ in range(steps):
        _, dpred = agn_train.mse_loss_grad(pred, y, n_global=NG, scaler=scaler)
        pred.backward(dpred)
        if scaler is None:
            opt.step()
        else:
            scaler.step(opt)
            scaler.update()
        opt.zero_grad()
    opt.state_dict()
    return pred0, pred.detach(), y, opt.state[pred]["step"]


def test_fp16_trains_only_with_a_scaler():
    pred0, pred, y, step = train_leaf(None)
    assert torch.equal(bits(pred), bits(pred0)) and float(step) == 20.0  # twenty steps on zeros
    s = agn_train.LossScaler()
    pred0, pred, y, step = train_leaf(s)
    d0, d = (pred0.double() - y.double()).abs(), (pred.double() - y.double()).abs()
    print(f"with a scaler: |pred - y| from {float(d0.max()):.6f} to [{float(d.min()):.6f}, {float(d.max()):.6f}]")
    # twenty Adam steps of lr 1e-3 move each element by up to 0.02: at least 2^-7 of the 2^-5 is asked for
    assert bool((d < d0).all()) and float(d.max()) <= 2.0 ** -5 - 2.0 ** -7 and float(step) == 20.0
    assert s.steps_skipped() == 0 and s.get_scale() == 65536.0


def test_a_scale_that_overflows_backs_off_until_a_step_applies():
    """Module docstring: 2^44, 2^43 and 2^42 overflow fp16 here (2^-26 S >= 2^16), 2^41 applies."""
    s = agn_train.LossScaler(init_scale=2.0 ** 44)
    pred0, pred, y, step = train_leaf(s)
    d0, d = (pred0.double() - y.double()).abs(), (pred.double() - y.double()).abs()
    assert s.steps_skipped() == 3 and s.get_scale() == 2.0 ** 41 and float(step) == 17.0
    assert bool(torch.isfinite(pred).all()) and bool((d < d0).all())
    # the scale of the request, 2^40, applies at once (2^14); with growth_interval = 1 it grows into the
    # overflow and backs off again
    s = agn_train.LossScaler(init_scale=2.0 ** 40, growth_interval=1)
    pred0, pred, y, step = train_leaf(s)
    d = (pred.double() - y.double()).abs()
    print(f"from 2^40 with growth_interval 1: {s.steps_skipped()} of 20 steps skipped, scale {s.get_scale():.4g}")
    assert s.steps_skipped() > 0 and float(step) == 20.0 - s.steps_skipped()
    assert bool(torch.isfinite(pred).all()) and bool((d < d0).all())


# ----------------------------------------------------------------------------- 7. the whole model
def fp16_model_and_batches():
    dt = torch.float16
    e = CFG["airfoil_mgn"]
    dims = e["dims"]
    torch.manual_seed(0)
    model = build(e["model"], dict(e["kwargs"], hidden_dim=32, processor_size=2), dims).to(dt).to(DEV)
    assert model.__class__.__name__ == "MeshGraphNet"
    batches = []
    for b in two_batches(dims):
        t = {k: (v.to(dt) if v.is_floating_point() else v) for k, v in b.__dict__.items()}
        assert t["x"].shape[0] == 64
        batches.append(t)
    return model, batches


def test_whole_model_in_fp16():
    dt = torch.float16
    ma, batches = fp16_model_and_batches()
    mb = copy.deepcopy(ma)
    pa, pb = list(ma.parameters()), list(mb.parameters())
    assert all(p.dtype == dt for p in pa)
    oa = agn_optim.Adam(pa, lr=1e-3, weight_decay=1e-2, master_weights=True)
    shadow = [nn.Parameter(p.detach().float()) for p in pb]
    ob = agn_optim.Adam(shadow, lr=1e-3, weight_decay=1e-2)
    s = agn_train.LossScaler()
    inv = inv_of(s.get_scale())
    ma.train()
    mb.train()
    for k in range(5):
        t = batches[k % 2]
        pred = run_model(ma, t)
        la, dpred = agn_train.mse_loss_grad(pred, t["y"], n_global=NG, scaler=s)
        pred.backward(dpred)
        if k == 0:  # unscaled, this gradient is zero where the scaled one is not
            _, plain = agn_train.mse_loss_grad(pred.detach(), t["y"], n_global=NG)
            assert int((plain == 0).sum()) > int((dpred == 0).sum()) and bool((dpred != 0).any())
            assert sum(int((p.grad != 0).sum()) for p in pa) > 0
        s.step(oa)
        s.update()
        oa.zero_grad()
        pred = run_model(mb, t)
        lb, dpred = agn_train.mse_loss_grad(pred, t["y"], n_global=NG, scaler=s)
        pred.backward(dpred)
        for p, q in zip(pb, shadow):
            assert p.grad is not None and p.grad.dtype == dt and bool(torch.isfinite(p.grad).all())
            q.grad = p.grad.float() * inv
        ob.step()
        with torch.no_grad():
            for p, q in zip(pb, shadow):
                p.copy_(q.to(dt))
        mb.zero_grad()
        assert torch.equal(bits(la), bits(lb)), (k, float(la), float(lb))
        for (n, p), q in zip(ma.named_parameters(), pb):
            assert torch.equal(bits(p), bits(q)), (k, n)
    assert s.steps_skipped() == 0 and [t.master for t in oa._agn_tables.values()] == [True]
    assert all(float(st["step"]) == 5.0 for st in oa.state_dict()["state"].values())


def test_train_returns_the_unscaled_loss():
    ma, batches = fp16_model_and_batches()
    mb = copy.deepcopy(ma)
    loader = [Batch(**batches[0])]
    oa = agn_optim.Adam(ma.parameters(), lr=1e-3, master_weights=True)
    ob = agn_optim.Adam(mb.parameters(), lr=1e-3, master_weights=True)
    s = agn_train.LossScaler()
    got = agn_train.train(ma, loader, oa, agn_train.MSELoss(), DEV, scaler=s)
    want = agn_train.train(mb, loader, ob, agn_train.MSELoss(), DEV)
    assert isinstance(got, float) and got == want and got > 0.0
    assert s.steps_skipped() == 0 and s.state_dict()["_growth_tracker"] == 1  # step and update ran
    assert all(p.grad is None for p in ma.parameters())
    assert all(float(st["step"]) == 1.0 for st in oa.state_dict()["state"].values())


# ----------------------------------------------------------------------------- 8. errors
def test_step_raises_instead_of_torchs_step():
    s = agn_train.LossScaler()

    def params(dt):
        ps = [nn.Parameter(torch.ones(9, dtype=dt, device=DEV)), nn.Parameter(torch.ones(5, device=DEV))]
        for p in ps:
            p.grad = torch.ones_like(p)
        return ps
    ps = params(torch.float16)
    plain = agn_optim.Adam(ps, lr=1e-3)  # a 16-bit parameter without master_weights
    with pytest.raises(RuntimeError, match=r"parameter 0 of group 0 \(torch.float16.*needs master_weights=True"):
        s.step(plain)
    with pytest.raises(RuntimeError, match="needs an aerognn.optim.Adam"):
        s.step(torch.optim.Adam(ps, lr=1e-3))
    ok = agn_optim.Adam(ps, lr=1e-3, master_weights=True)
    with pytest.raises(RuntimeError, match="closure"):
        s.step(ok, lambda: torch.tensor(1.0))
    strided = nn.Parameter(torch.ones(6, 4, device=DEV).t())
    strided.grad = torch.ones_like(strided)
    with pytest.raises(RuntimeError, match="cannot take the loss-scaled step"):
        s.step(agn_optim.Adam([strided], lr=1e-3))
    assert not plain.state and not ok.state and all(bool((p == 1).all()) for p in ps + [strided])
    # and step() without a scaler is what it was: torch's own step on the 16-bit parameter
    plain.step()
    assert plain.state[ps[0]]["exp_avg"].dtype == torch.float16 and float(plain.state[ps[0]]["step"]) == 1.0
