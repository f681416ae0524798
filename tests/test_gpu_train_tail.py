"""The training tail on the MI355X: agn_mse_loss (aerognn.train.mse_loss_grad / MSELoss / train /
evaluate) and agn_adam_step (aerognn.optim.Adam) against torch, which is the reference implementation
of both formulas.

Bounds:
  dpred    bitwise (2 * (pred.double() - y.double()) / n_global).float().to(T), compared on integer views.
           The fp64 part of the reference is formed on the host with numpy, whose division is the IEEE
           one (torch's device kernel multiplies by the reciprocal of a host scalar instead).
  loss     |loss - ref| <= (n f + 2) 2^-53 ref against the fp64 sum: all terms are positive, so the
           bound holds for any summation order ((k - 1) u for the sum, one u for the squares, one for
           the division). Two calls give identical bytes; acc after two calls is loss + loss exactly.
  Adam     fp32: separately for p, exp_avg and exp_avg_sq over the concatenation of all tensors, the
           rel-L2 and the max-abs error against torch.optim.Adam(foreach=False) in fp64 are each <= 3 x
           the same errors of torch.optim.Adam(foreach=False) in fp32, measured here. fp64: rel-L2
           <= 1e-10 against torch's fp64 run (the project's float64 tolerance).
  step     gradients of the first step bitwise the reference-style loop's (nn.MSELoss + torch.optim.Adam;
           the model kernels are deterministic), parameters within the Adam gate, the epoch loss
           within 2^-22 relative (a few fp32 roundings in torch's own loss). The batches hold 64 nodes x 4
           targets: nn.MSELoss's own backward equals the once-rounded fp64 formula bit for bit only
           when the element count is a power of two (two_batches). At another count (82 x 4) dpred is
           still bitwise the formula and within 5 * 2^-24 relative of torch's gradient per element
           (torch's three roundings plus this kernel's one).
  replay   the steady-state path of aerognn.optim.Adam (every step after the first of a real run): the
           same fp32 gate after five steps, and after state.clear() / del state[p].
Sizes are the smallest at which the kernels can go wrong: one element, the vector width +- 1, the
chunk sizes C - 1, C, C + 1 and 2 C + 5 / 2 C + 7, more than one block, an unaligned view."""
import ctypes
import types
import warnings

import numpy as np
import pytest
import torch
from torch import nn

from aerognn import _lib as L
from aerognn import optim as agn_optim
from aerognn import train as agn_train
from test_gpu_config_experiments import CFG, build, run_model

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -53
INT_VIEW = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16,
            torch.float64: torch.int64}
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "f64": torch.float64}


def mse_shapes():
    c = agn_train.chunk_rows()
    return [(1, 1), (1, 4), (c - 1, 4), (c, 4), (c + 1, 3), (2 * c + 5, 5)]


def make_pair(n, f, dtype, y_dtype, seed, ld=None):
    g = torch.Generator().manual_seed(seed)
    buf = torch.randn(n, ld or f, generator=g).to(dtype)
    y = torch.randn(n, f, generator=g).to(y_dtype)
    return buf, y


def ref_dpred(pred_cpu, y_cpu, n_global):
    d = pred_cpu.double().numpy() - y_cpu.double().numpy()
    q = (2.0 * d) / np.float64(n_global)
    if pred_cpu.dtype == torch.float64:
        return torch.from_numpy(q)
    return torch.from_numpy(q.astype(np.float32)).to(pred_cpu.dtype)


def ref_loss(pred_cpu, y_cpu, n_global):
    return float(((pred_cpu.double() - y_cpu.double()) ** 2).sum() / n_global)


def check_mse(pred_cpu, y_cpu, n_global=None, pred_dev=None):
    """pred_dev: the device tensor to pass (a column slice); default pred_cpu on the device."""
    n, f = pred_cpu.shape
    pred = pred_cpu.to(DEV) if pred_dev is None else pred_dev
    y = y_cpu.to(DEV)
    ng = float(n * f) if n_global is None else float(n_global)
    acc = torch.zeros((), dtype=torch.float64, device=DEV)
    loss1, dp1 = agn_train.mse_loss_grad(pred, y, n_global=n_global, acc=acc)
    loss2, dp2 = agn_train.mse_loss_grad(pred, y, n_global=n_global, acc=acc)
    loss3, none = agn_train.mse_loss_grad(pred, y, n_global=n_global, need_grad=False)
    assert none is None and dp1.shape == pred.shape and dp1.dtype == pred.dtype and loss1.dtype == torch.float64
    want = ref_dpred(pred_cpu, y_cpu, ng)
    iv = INT_VIEW[pred.dtype]
    what = (n, f, pred.dtype, y.dtype, n_global)
    assert torch.equal(dp1.cpu().view(iv), want.view(iv)), what
    assert torch.equal(dp2.view(iv), dp1.view(iv)), what
    l1, l2, l3, a = (t.cpu().view(torch.int64) for t in (loss1, loss2, loss3, acc))
    assert torch.equal(l1, l2) and torch.equal(l1, l3), what  # identical bytes; dpred = NULL too
    assert float(acc) == float(loss1) + float(loss1), what
    ref = ref_loss(pred_cpu, y_cpu, ng)
    err = abs(float(loss1) - ref)
    bound = (n * f + 2) * U * ref
    print(f"mse {what}: loss {float(loss1):.17g} ref {ref:.17g} err {err:.3e} bound {bound:.3e}")
    assert err <= bound, what


@pytest.mark.parametrize("name", sorted(DTYPES))
def test_mse_grad_bitwise_and_value(name):
    dtype = DTYPES[name]
    for i, (n, f) in enumerate(mse_shapes()):
        pred, y = make_pair(n, f, dtype, dtype, 10 + i)
        check_mse(pred, y)
        if dtype != torch.float32:  # y in float32 next to a 16-bit (or float64) prediction
            pred, y = make_pair(n, f, dtype, torch.float32, 20 + i)
            check_mse(pred, y)


@pytest.mark.parametrize("name", ["f32", "bf16"])
def test_mse_column_slice_and_global_count(name):
    dtype = DTYPES[name]
    c = agn_train.chunk_rows()
    buf, y = make_pair(c + 1, 3, dtype, dtype, 31, ld=7)  # pred = columns 2..4 of a 7-wide buffer
    dev_buf = buf.to(DEV)
    pred_dev = dev_buf[:, 2:5]
    assert pred_dev.stride(0) == 7 and not pred_dev.is_contiguous()
    check_mse(buf[:, 2:5].contiguous(), y, pred_dev=pred_dev)
    assert torch.equal(dev_buf.cpu().view(INT_VIEW[dtype]), buf.view(INT_VIEW[dtype]))  # pred is only read
    pred, y = make_pair(c + 1, 3, dtype, dtype, 32)
    check_mse(pred, y, n_global=3 * (c + 1) + 1001)  # the all-reduced count of a data-parallel run


def test_mse_empty_and_module():
    acc = torch.full((), 2.5, dtype=torch.float64, device=DEV)
    loss, dp = agn_train.mse_loss_grad(torch.zeros(0, 4, device=DEV), torch.zeros(0, 4, device=DEV), n_global=8.0,
                                       acc=acc)
    assert float(loss) == 0.0 and float(acc) == 2.5 and dp.shape == (0, 4)
    # MSELoss: the value of mse_loss_grad, and backward hands pred the gradient of the same pass
    pred_cpu, y_cpu = make_pair(65, 4, torch.float32, torch.float32, 40)
    pred = pred_cpu.to(DEV).requires_grad_(True)
    y = y_cpu.to(DEV)
    loss = agn_train.MSELoss()(pred, y)
    loss.backward()
    l0, d0 = agn_train.mse_loss_grad(pred, y)
    assert loss.dtype == torch.float64 and float(loss.detach()) == float(l0)
    assert torch.equal(pred.grad.view(torch.int32), d0.view(torch.int32))
    ref = nn.MSELoss()(pred_cpu, y_cpu)
    assert abs(float(loss.detach()) - float(ref)) <= 2.0 ** -22 * float(ref)
    with torch.no_grad():
        assert float(agn_train.MSELoss()(pred.detach(), y)) == float(l0)


def test_mse_argument_errors():
    lib = L.lib()
    pred = torch.zeros(8, 4, device=DEV)
    y = torch.zeros(8, 4, device=DEV)
    dp = torch.zeros(8, 4, device=DEV)
    loss = torch.zeros((), dtype=torch.float64, device=DEV)
    scr = torch.zeros(64, dtype=torch.uint8, device=DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: t.data_ptr()  # noqa: E731

    def call(dtype=L.F32, y_dtype=L.F32, n=8, f=4, p=P(pred), pld=4, yy=P(y), yld=4, ng=32.0, lo=P(loss), d=P(dp),
             dld=4, s=P(scr)):
        return lib.agn_mse_loss(dtype, y_dtype, n, f, p, pld, yy, yld, ng, lo, None, d, dld, s, st)
    assert call() == 0
    assert call(p=None) == -1 and call(yy=None) == -1 and call(lo=None) == -1 and call(s=None) == -1  # AGN_E_ARG
    assert call(n=-1) == -1
    assert call(f=0) == -4 and call(pld=3) == -4 and call(yld=3) == -4 and call(dld=3) == -4  # AGN_E_SHAPE
    assert call(ng=0.0) == -4 and call(ng=-1.0) == -4
    assert call(dtype=7) == -2 and call(y_dtype=L.BF16) == -2  # AGN_E_DTYPE
    torch.cuda.synchronize()
    tab = torch.zeros(96, dtype=torch.uint8, device=DEV)
    cmap = torch.zeros(2, dtype=torch.int32, device=DEV)
    assert lib.agn_adam_step(None, 1, P(cmap), 1, L.F32, st) == -1
    assert lib.agn_adam_step(P(tab), 1, None, 1, L.F32, st) == -1
    assert lib.agn_adam_step(P(tab), -1, P(cmap), 1, L.F32, st) == -1
    assert lib.agn_adam_step(P(tab), 1, P(cmap), -1, L.F32, st) == -1
    assert lib.agn_adam_step(P(tab), 1, P(cmap), 1, L.BF16, st) == -2
    assert lib.agn_adam_step(P(tab), 1, P(cmap), 1, L.F32, st) == 0  # a zeroed entry (n == 0) touches nothing
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- Adam
def adam_sizes():
    c = agn_optim.chunk_elems()
    return [1, 3, 4, 5, 63, 65, c - 1, c, c + 1, 2 * c + 7, (128, 128)]


LRS = (1e-3, 1e-3, 8e-4)  # a scheduler change before the third step


def make_problem(dtypes, nsteps=len(LRS), extras=True):
    """Start values (fp32-exact) and nsteps gradients per tensor, on the host in float64. specs:
    (shape, dtype, kind); kind 'view' = a view one element into a buffer, and with extras 'nograd'
    (never a gradient) and 'empty' (no elements)."""
    specs = [(s, dtypes[i % len(dtypes)], "plain") for i, s in enumerate(adam_sizes())]
    specs += [(67, dtypes[0], "view")]
    if extras:
        specs += [(9, dtypes[0], "nograd"), (0, dtypes[0], "empty")]
    g = torch.Generator().manual_seed(5)
    start, grads = [], []
    for i, (shape, _, kind) in enumerate(specs):
        shape = shape if isinstance(shape, tuple) else (shape,)
        start.append(torch.randn(shape, generator=g).float().double())
        gs = []
        for _ in range(nsteps):
            t = torch.randn(shape, generator=g) * 10.0 ** ((i % 5) - 3)  # down to 1e-3: the eps regime
            t = t.float()
            if t.numel() > 4:
                t.view(-1)[::5] = 0.0  # exact zeros
            gs.append(t.double())
        grads.append(None if kind == "nograd" else gs)
    return specs, start, grads


def make_params(specs, start, force=None):
    params = []
    for (shape, dtype, kind), s in zip(specs, start):
        dt = force or dtype
        if kind == "view":
            buf = torch.zeros(s.numel() + 1, dtype=dt, device=DEV)
            buf[1:] = s.to(dt)
            p = nn.Parameter(buf[1:])
            assert p.data_ptr() % 16 != 0 and p.is_contiguous()
        else:
            p = nn.Parameter(s.to(dt).to(DEV))
        params.append(p)
    return params


def run_adam(cls, specs, start, grads, wd, force=None, **kw):
    """Three steps of `cls` from `start`; tensors in their spec dtype, or all in `force`."""
    params = make_params(specs, start, force)
    opt = cls(params, lr=LRS[0], weight_decay=wd, **kw)
    for k, lr in enumerate(LRS):
        opt.param_groups[0]["lr"] = lr
        for p, gs in zip(params, grads):
            p.grad = None if gs is None else gs[k].to(p.dtype).to(DEV)
        opt.step()
    return params, opt


def cat_state(params, opt, idx):
    out = {}
    for key in ("p", "exp_avg", "exp_avg_sq"):
        out[key] = torch.cat([(params[i] if key == "p" else opt.state[params[i]][key]).detach().double().reshape(-1).cpu()
                              for i in idx])
    return out


def errs(a, ref):
    d = a - ref
    return float(d.norm() / ref.norm()), float(d.abs().max())


def gate_fp32(ours, t32, t64, what):
    """ours within 3 x torch's own fp32 error against the fp64 run, per quantity."""
    for key in ("p", "exp_avg", "exp_avg_sq"):
        (r_o, m_o), (r_t, m_t) = errs(ours[key], t64[key]), errs(t32[key], t64[key])
        print(f"adam {what} {key}: rel-L2 ours {r_o:.3e} torch {r_t:.3e} (x{r_o / max(r_t, 1e-300):.2f}); "
              f"max-abs ours {m_o:.3e} torch {m_t:.3e} (x{m_o / max(m_t, 1e-300):.2f})")
        assert r_o <= 3 * r_t and m_o <= 3 * m_t, (what, key, r_o, r_t, m_o, m_t)


@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_adam_fp32_against_torch(wd):
    specs, start, grads = make_problem([torch.float32])
    live = [i for i, gs in enumerate(grads) if gs is not None and start[i].numel() > 0]
    po, oo = run_adam(agn_optim.Adam, specs, start, grads, wd)
    p32, o32 = run_adam(torch.optim.Adam, specs, start, grads, wd, foreach=False)
    p64, o64 = run_adam(torch.optim.Adam, specs, start, grads, wd, force=torch.float64, foreach=False)
    assert "_agn_tables" in oo.__dict__  # the device path ran
    t64 = cat_state(p64, o64, live)
    assert errs(cat_state(p32, o32, live)["p"], t64["p"])[0] > 0.0  # torch's own error is not zero
    gate_fp32(cat_state(po, oo, live), cat_state(p32, o32, live), t64, f"wd={wd}")
    for i, (spec, gs) in enumerate(zip(specs, grads)):
        if gs is None:  # no gradient: parameter and state untouched, as torch leaves them
            assert torch.equal(po[i].detach().cpu().double(), start[i]) and po[i] not in oo.state and p32[i] not in o32.state
        else:
            so, st = oo.state[po[i]], o32.state[p32[i]]
            assert so["step"].device.type == "cpu" and so["step"].dtype == st["step"].dtype
            assert torch.equal(so["step"], st["step"]) and float(so["step"]) == len(LRS), spec
    sa, sb = oo.state_dict(), o32.state_dict()
    assert sorted(sa["state"]) == sorted(sb["state"])
    ga, gb = (dict(d["param_groups"][0], foreach=None) for d in (sa, sb))  # the torch runs set foreach=False
    assert ga == gb
    # the view's neighbour element (the buffer's first) is not written
    view = [i for i, s in enumerate(specs) if s[2] == "view"][0]
    assert po[view].storage_offset() == 1
    assert float(torch.as_strided(po[view].detach(), (1,), (1,), 0)) == 0.0


def test_adam_fp64_and_mixed_list():
    for dtypes in ([torch.float64], [torch.float32, torch.float64]):
        specs, start, grads = make_problem(dtypes)
        po, oo = run_adam(agn_optim.Adam, specs, start, grads, 1e-2)
        pt, ot = run_adam(torch.optim.Adam, specs, start, grads, 1e-2, foreach=False)
        p64, o64 = run_adam(torch.optim.Adam, specs, start, grads, 1e-2, force=torch.float64, foreach=False)
        assert set(t.dtype for t in oo.__dict__["_agn_tables"].values()) == set(dtypes)
        live = [i for i, gs in enumerate(grads) if gs is not None and start[i].numel() > 0]
        i64 = [i for i in live if specs[i][1] == torch.float64]
        i32 = [i for i in live if specs[i][1] == torch.float32]
        a, b = cat_state(po, oo, i64), cat_state(pt, ot, i64)
        for key in a:
            r = errs(a[key], b[key])[0]
            print(f"adam fp64 {key}: rel-L2 vs torch fp64 {r:.3e}")
            assert r <= 1e-10, (key, r)
        if i32:
            gate_fp32(cat_state(po, oo, i32), cat_state(pt, ot, i32), cat_state(p64, o64, i32), "mixed list")


def test_adam_state_dict_round_trip_on_device():
    """A torch.optim.Adam checkpoint continues on this class (and back) within the fp32 gate's terms:
    here simply the same step from the same state, compared with torch's step."""
    import copy
    specs, start, grads = make_problem([torch.float32])
    p32, o32 = run_adam(torch.optim.Adam, specs, start, grads, 1e-2, foreach=False)
    mine = [nn.Parameter(p.detach().clone()) for p in p32]
    opt = agn_optim.Adam(mine, lr=1.0)
    opt.load_state_dict(copy.deepcopy(o32.state_dict()))
    ref64 = [nn.Parameter(p.detach().double()) for p in p32]
    o64 = torch.optim.Adam(ref64, lr=1.0, foreach=False)
    o64.load_state_dict(copy.deepcopy(o32.state_dict()))
    for ps, o in ((mine, opt), (p32, o32), (ref64, o64)):
        for p, gs in zip(ps, grads):
            p.grad = None if gs is None else gs[0].to(p.dtype).to(DEV)
        o.step()
    live = [i for i, gs in enumerate(grads) if gs is not None and start[i].numel() > 0]
    assert float(opt.state[mine[live[0]]]["step"]) == len(LRS) + 1
    gate_fp32(cat_state(mine, opt, live), cat_state(p32, o32, live), cat_state(ref64, o64, live), "after load")


def test_adam_steady_state_replay():
    """The path every step after the first takes once all parameters have their state (Adam._replay):
    five steps with an lr change, one of them with one gradient set to None (that tensor's own step
    count then lags, as in torch), gated like the other Adam tests; then state.clear(), after which
    the cached plan must not be replayed: the next step starts new state, as torch's does."""
    lrs = (1e-3, 1e-3, 8e-4, 8e-4, 5e-4)
    skip_at, skipped = 2, 1
    specs, start, grads = make_problem([torch.float32], nsteps=len(lrs) + 1, extras=False)
    runs = []
    for cls, force, kw in ((agn_optim.Adam, None, {}), (torch.optim.Adam, None, dict(foreach=False)),
                           (torch.optim.Adam, torch.float64, dict(foreach=False))):
        ps = make_params(specs, start, force)
        runs.append((ps, cls(ps, lr=lrs[0], weight_decay=1e-2, **kw)))

    def one_step(k, lr, skip):
        for ps, o in runs:
            o.param_groups[0]["lr"] = lr
            for i, (p, gs) in enumerate(zip(ps, grads)):
                p.grad = None if (skip and i == skipped) else gs[k].to(p.dtype).to(DEV)
            o.step()
    (po, oo), (p32, o32), (p64, o64) = runs
    plan = None
    for k, lr in enumerate(lrs):
        one_step(k, lr, k == skip_at)
        now = oo.__dict__.get("_agn_plan")
        assert now is not None, k
        assert k == 0 or now is plan, k  # steps 1.. replayed the plan of step 0 (a fresh partition makes a new one)
        plan = now
    idx = list(range(len(specs)))
    gate_fp32(cat_state(po, oo, idx), cat_state(p32, o32, idx), cat_state(p64, o64, idx), "replay")
    for i in idx:
        so, st = oo.state[po[i]]["step"], o32.state[p32[i]]["step"]
        assert torch.equal(so, st) and float(so) == len(lrs) - (1 if i == skipped else 0), i
    # state.clear(): the tensors the plan holds are orphans now
    old_m = oo.state[po[0]]["exp_avg"]
    kept = old_m.clone()
    for _, o in runs:
        o.state.clear()
    one_step(len(lrs), lrs[-1], False)
    assert oo.__dict__.get("_agn_plan") is not None and oo._agn_plan is not plan
    assert torch.equal(old_m, kept) and oo.state[po[0]]["exp_avg"] is not old_m  # the orphan was not updated
    for i in idx:
        assert float(oo.state[po[i]]["step"]) == 1.0 == float(o32.state[p32[i]]["step"])
    assert sorted(oo.state_dict()["state"]) == sorted(o32.state_dict()["state"]) == idx
    gate_fp32(cat_state(po, oo, idx), cat_state(p32, o32, idx), cat_state(p64, o64, idx), "after state.clear()")
    # del of one entry is caught too: that parameter alone restarts
    for ps, o in runs:
        del o.state[ps[3]]
    one_step(0, lrs[-1], False)
    for i in idx:
        assert float(oo.state[po[i]]["step"]) == (1.0 if i == 3 else 2.0) == float(o32.state[p32[i]]["step"])
    gate_fp32(cat_state(po, oo, idx), cat_state(p32, o32, idx), cat_state(p64, o64, idx), "after del state[p]")


def test_adam_16bit_parameters_take_torch_step():
    """bf16 parameters do not qualify: torch's own step, bitwise; fp32 ones next to them still run here."""
    g = torch.Generator().manual_seed(9)
    vals = [torch.randn(33, generator=g), torch.randn(70, generator=g)]
    gr = [torch.randn(33, generator=g), torch.randn(70, generator=g)]

    def run(cls):
        ps = [nn.Parameter(vals[0].to(torch.bfloat16).to(DEV)), nn.Parameter(vals[1].to(DEV))]
        o = cls(ps, lr=1e-3, weight_decay=1e-2)
        for _ in range(2):
            ps[0].grad, ps[1].grad = gr[0].to(torch.bfloat16).to(DEV), gr[1].to(DEV)
            o.step()
        return ps, o
    (a, oa), (b, ob) = run(agn_optim.Adam), run(torch.optim.Adam)
    assert torch.equal(a[0].view(torch.int16), b[0].view(torch.int16))
    assert torch.equal(oa.state[a[0]]["exp_avg_sq"].view(torch.int16), ob.state[b[0]]["exp_avg_sq"].view(torch.int16))
    assert float(oa.state[a[0]]["step"]) == 2.0 and float(oa.state[a[1]]["step"]) == 2.0
    # |p| < 8 here: one fp32 ulp (2^-21 at most) per step is the most two correct evaluations differ by
    assert float(a[1].detach().abs().max()) < 8.0 and float((a[1] - b[1]).abs().max()) <= 2 * 2.0 ** -21


# ----------------------------------------------------------------------------- the whole step
BSMS_H32 = dict(processor_size=3, num_hidden_layers_node_processor=2, num_hidden_layers_edge_processor=2,
                num_hidden_layers_node_encoder=2, num_hidden_layers_edge_encoder=2, num_hidden_layers_decoder=2,
                hidden_dim_processor=32, hidden_dim_node_encoder=32, hidden_dim_edge_encoder=32, hidden_dim_decoder=32,
                aggregation="add", do_concat_trick=True, num_scales=2, layers_per_scale=1, stride=2)


def make_model(name):
    torch.manual_seed(0)
    if name == "bsms_h32":
        from models.bsms_mgn import BiStridedMeshGraphNet
        return BiStridedMeshGraphNet(6, 4, 4, **BSMS_H32).to(DEV), [6, 4, 4]
    e = CFG[name]
    return build(e["model"], e["kwargs"], e["dims"]).to(DEV), e["dims"]


class Batch(types.SimpleNamespace):
    def to(self, device):
        return self


def batch_of(dims, meshes, seed):
    """test_gpu_config_experiments.tiny_batch's feature layout (dataset.py:39-106) for the given
    ellipsoid meshes."""
    from aerognn.meshgen import collate, ellipsoid
    d_n, d_e, d_out = dims
    pd = d_e - 1
    b = collate([ellipsoid(nu, nv, seed=seed + i) for i, (nu, nv) in enumerate(meshes)])
    gen = torch.Generator().manual_seed(17 + seed)
    pos = torch.from_numpy(b["pos"])[:, :pd]
    nrm = torch.from_numpy(b["x"])[:, 3:3 + pd]
    nrm = nrm / nrm.norm(dim=1, keepdim=True).clamp_min(1e-6)
    ei = torch.from_numpy(b["edge_index"])
    batch = torch.from_numpy(b["batch"])
    var = torch.randn(len(meshes), d_n - 2 * pd, generator=gen)
    vec = pos[ei[1]] - pos[ei[0]]
    t = dict(x=torch.cat([pos, nrm, var[batch]], 1), edge_attr=torch.cat([vec, vec.norm(dim=1, keepdim=True)], 1),
             y=torch.randn(pos.shape[0], d_out, generator=gen), pos=pos)
    assert t["x"].shape[1] == d_n and t["edge_attr"].shape[1] == d_e
    t = {k: v.float().contiguous().to(DEV) for k, v in t.items()}
    t["edge_index"], t["batch"] = ei.to(DEV), batch.to(DEV)
    return Batch(**t)


def two_batches(dims):
    """Two batches of 64 nodes x 4 targets. The element count is a power of two on purpose: nn.MSELoss's
    backward rounds pred - y to fp32 and multiplies by fp32(2 / N), agn_mse_loss rounds the exact
    2 (pred - y) / N once; the two agree bit for bit exactly when N is a power of two (the scaling is
    then exact), and only then can the parameter gradients of the two loops be compared bitwise. For any
    other N the two dpred differ in the last bit of some elements (about a third of them)."""
    out = [batch_of(dims, [(8, 5), (6, 4)], 0), batch_of(dims, [(8, 4), (4, 8)], 3)]
    for b in out:
        n = b.y.numel()
        assert n & (n - 1) == 0, n
    return out


def as_dict(b):
    return b.__dict__


def record_steps(opt, params):
    rec = []
    opt.register_step_pre_hook(lambda o, a, k: rec.append(([p.detach().clone() for p in params],
                                                           [p.grad.detach().clone() for p in params])))
    return rec


def reference_loop(model, loader, opt, loss_fn):
    """utils.py:171-196 as written."""
    model.train()
    total = 0.0
    for batch in loader:
        pred = run_model(model, as_dict(batch))
        loss = loss_fn(pred, batch.y)
        loss.backward()
        opt.step()
        opt.zero_grad()
        total += loss.item()
    return total / len(loader)


@pytest.mark.parametrize("name", ["airfoil_mgn", "ahmedBody_pooling_mgn", "bsms_h32"])
def test_whole_step_against_reference_loop(name):
    ma, dims = make_model(name)
    mb, _ = make_model(name)
    for a, b in zip(ma.parameters(), mb.parameters()):
        assert torch.equal(a, b)
    loader = two_batches(dims)
    pa, pb = list(ma.parameters()), list(mb.parameters())
    oa = agn_optim.Adam(pa, lr=1e-3, weight_decay=0.0)
    ob = torch.optim.Adam(pb, lr=1e-3, weight_decay=0.0)
    ra, rb = record_steps(oa, pa), record_steps(ob, pb)
    got = agn_train.train(ma, loader, oa, nn.MSELoss(), DEV)
    want = reference_loop(mb, loader, ob, nn.MSELoss())
    assert "_agn_tables" in oa.__dict__ and len(ra) == len(rb) == 2
    # first step: the same gradients bit for bit, the parameters within the Adam gate
    for x, y, (k, _) in zip(ra[0][1], rb[0][1], ma.named_parameters()):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), k
    p64 = [nn.Parameter(p.double()) for p in ra[0][0]]
    o64 = torch.optim.Adam(p64, lr=1e-3, weight_decay=0.0, foreach=False)
    for p, g in zip(p64, ra[0][1]):
        p.grad = g.double()
    o64.step()
    cat = lambda ts: torch.cat([t.detach().double().reshape(-1).cpu() for t in ts])  # noqa: E731
    ref = cat(p64)
    (r_o, m_o), (r_t, m_t) = errs(cat(ra[1][0]), ref), errs(cat(rb[1][0]), ref)
    print(f"{name}: step-1 parameters rel-L2 ours {r_o:.3e} torch {r_t:.3e}; max-abs ours {m_o:.3e} torch {m_t:.3e}; "
          f"epoch loss ours {got:.9g} loop {want:.9g}")
    assert r_o <= 3 * r_t and m_o <= 3 * m_t
    assert abs(got - want) <= 2.0 ** -22 * abs(want)
    for p in pa:
        assert p.grad is None  # optimizer.zero_grad() ran
    # evaluate: the loop's value, parameters untouched
    before = [p.detach().clone() for p in pa]
    ev = agn_train.evaluate(ma, loader, nn.MSELoss(), DEV)
    ma.eval()
    with torch.no_grad():
        ref_ev = sum(nn.MSELoss()(run_model(ma, as_dict(b)), b.y).item() for b in loader) / len(loader)
    assert abs(ev - ref_ev) <= 2.0 ** -22 * abs(ref_ev)
    for p, q in zip(pa, before):
        assert torch.equal(p, q)
    assert agn_train.evaluate(ma, loader, agn_train.MSELoss(), DEV) == ev


def test_gradient_at_a_count_that_is_no_power_of_two():
    """82 nodes x 4 targets (test_gpu_config_experiments.tiny_batch), the kind of count real batches
    have. What train() hands to pred.backward is bitwise the fp64 formula rounded once, and it is
    within 5 * 2^-24 relative of nn.MSELoss's own gradient element by element: torch rounds pred - y,
    2 / N and their product (three roundings, (1 + u)^3 - 1 < 3.5 u), agn_mse_loss rounds the exact
    value once (u), so the two differ by less than 4.5 u of the exact value, u = 2^-24. The parameter
    gradients of the two are then compared through the same backward, only as a printed figure."""
    from test_gpu_config_experiments import tiny_batch
    model, dims = make_model("airfoil_mgn")
    t = tiny_batch(dims)
    n = t["y"].numel()
    assert n == 328 and n & (n - 1) != 0
    model.train()
    pred = run_model(model, t)
    _, dpred = agn_train.mse_loss_grad(pred, t["y"])
    want = ref_dpred(pred.detach().cpu(), t["y"].cpu(), float(n))
    assert torch.equal(dpred.cpu().view(torch.int32), want.view(torch.int32))
    leaf = pred.detach().clone().requires_grad_(True)
    nn.MSELoss()(leaf, t["y"]).backward()
    exact = 2.0 * (pred.detach().double() - t["y"].double()) / n
    diff = (dpred.double() - leaf.grad.double()).abs()
    nbits = int((dpred.view(torch.int32) != leaf.grad.view(torch.int32)).sum())
    print(f"dpred vs nn.MSELoss's gradient at N = {n}: {nbits} of {n} elements differ, max |diff| / |exact| "
          f"{float((diff / exact.abs().clamp_min(1e-300)).max()):.3e}")
    assert bool((diff <= 5 * 2.0 ** -24 * exact.abs()).all())
    pred.backward(dpred)
    ga = [p.grad.detach().clone() for p in model.parameters()]
    model.zero_grad(set_to_none=True)
    nn.MSELoss()(run_model(model, t), t["y"]).backward()
    num = torch.cat([(a.double() - p.grad.double()).reshape(-1) for a, p in zip(ga, model.parameters())]).norm()
    den = torch.cat([p.grad.double().reshape(-1) for p in model.parameters()]).norm()
    print(f"parameter gradients, this dpred against nn.MSELoss's: rel-L2 {float(num / den):.3e}")


def test_batches_the_kernel_does_not_cover_take_the_reference_loop():
    """nn.MSELoss promotes a float64 y next to a float32 prediction and broadcasts a [n, 1] y; agn_mse_loss
    does neither, so train() / evaluate() run the reference's loop on such batches: the same floats."""
    model, dims = make_model("airfoil_mgn")
    loader = two_batches(dims)
    wide = [Batch(**dict(b.__dict__, y=b.y.double())) for b in loader]
    col = [Batch(**dict(b.__dict__, y=b.y[:, :1].contiguous())) for b in loader]
    model.eval()
    for ld in (wide, col):
        with torch.no_grad(), warnings.catch_warnings():
            warnings.simplefilter("ignore")  # nn.MSELoss warns about the broadcast
            ref = sum(nn.MSELoss()(run_model(model, as_dict(b)), b.y).item() for b in ld) / len(ld)
            assert agn_train.evaluate(model, ld, nn.MSELoss(), DEV) == ref
    ma, _ = make_model("airfoil_mgn")
    mb, _ = make_model("airfoil_mgn")
    oa = torch.optim.Adam(ma.parameters(), lr=1e-3)
    ob = torch.optim.Adam(mb.parameters(), lr=1e-3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert agn_train.train(ma, col, oa, nn.MSELoss(), DEV) == reference_loop(mb, col, ob, nn.MSELoss())
    for a, b in zip(ma.parameters(), mb.parameters()):
        assert torch.equal(a, b)
