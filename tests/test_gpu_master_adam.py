"""aerognn.optim.Adam(master_weights=True) and agn_adam_step_master on the MI355X: bf16 / fp16 parameters
with an fp32 master copy and fp32 moments ("Master weights").

Bounds:
  identity  (master_param, exp_avg, exp_avg_sq) after every step are bitwise (int32 views) what
            agn_adam_step gives on fp32 tensors (a shadow aerognn.optim.Adam without the flag on fp32 clones,
            stepped with the upcast gradients); p is bitwise master_param.to(T) (int16 views).
  torch     the same three against torch.optim.Adam(foreach=False) in fp64 on the upcast values, within
            3 x the error of torch's own fp32 run, per quantity (test_gpu_train_tail.gate_fp32).
  follows   elements of p written between two steps restart from float(p) with their moments kept, the
            others continue from their masters: bitwise against a shadow built that way.
  model     a bf16 MeshGraphNet stepped by the master optimizer equals, bit for bit in parameters and
            losses, the same module whose parameters are overwritten from an fp32 shadow optimizer.
Sizes: one element, the wide path's 8 elements +- 1 and the fp32 kernel's 4 +- 1, 63 / 65, the chunk
size C - 1, C, C + 1 and 2 C + 7, more than one block, views one and four elements into a buffer (2-B and
8-B aligned: the scalar path), a parameter without a gradient and an empty one."""
import copy
import ctypes
import functools

import pytest
import torch
from torch import nn

from aerognn import _lib as L
from aerognn import optim as agn_optim
from aerognn import train as agn_train
from test_gpu_config_experiments import CFG, build, run_model
from test_gpu_train_tail import errs, gate_fp32, two_batches

pytestmark = pytest.mark.gpu

DEV = "cuda"
T16 = {"bf16": torch.bfloat16, "f16": torch.float16}
LRS = (1e-3, 1e-3, 8e-4)  # a scheduler change before the third step
KEYS = ("master_param", "exp_avg", "exp_avg_sq")
SKIPPED, SKIP_AT = 5, 1   # this tensor has no gradient at the second step
PAD = 3                   # untouched elements behind a view


def sizes():
    c = agn_optim.chunk_elems()
    return [1, 3, 4, 5, 7, 8, 9, 63, 65, c - 1, c, c + 1, 2 * c + 7, (128, 128)]


def rounded(t, dt):
    """t rounded to dt, as float64 on the host."""
    return t.to(dt).double()


def make_grads(shape, i, nsteps, gen, dt):
    """test_gpu_train_tail.make_problem's gradients (scales 1e-3 .. 10, exact zeros), rounded to dt."""
    gs = []
    for _ in range(nsteps):
        t = (torch.randn(shape, generator=gen) * 10.0 ** ((i % 5) - 3)).float()
        if t.numel() > 4:
            t.view(-1)[::5] = 0.0
        gs.append(rounded(t, dt))
    return gs


@functools.lru_cache(maxsize=None)
def problem(name):
    """specs (shape, kind), dt-exact start values and len(LRS) dt-exact gradients per tensor (float64, host)."""
    dt = T16[name]
    specs = [(s if isinstance(s, tuple) else (s,), "plain") for s in sizes()]
    specs += [((67,), "view1"), ((70,), "view4"), ((9,), "nograd"), ((0,), "empty")]
    gen = torch.Generator().manual_seed(5)
    start, grads = [], []
    for i, (shape, kind) in enumerate(specs):
        start.append(rounded(torch.randn(shape, generator=gen), dt))
        gs = make_grads(shape, i, len(LRS), gen, dt)
        grads.append(None if kind == "nograd" else gs)
    return specs, start, grads


def make_params(specs, start, dt):
    """Parameters in dt on the device; a view sits `off` elements into a zeroed buffer with PAD behind it."""
    params, bufs = [], {}
    for i, ((shape, kind), s) in enumerate(zip(specs, start)):
        if kind.startswith("view"):
            off, n = int(kind[4:]), s.numel()
            buf = torch.zeros(off + n + PAD, dtype=dt, device=DEV)
            buf[off:off + n] = s.to(dt)
            p = nn.Parameter(buf[off:off + n])
            assert p.is_contiguous() and p.data_ptr() % 16 == (off * buf.element_size()) % 16
            bufs[i] = (buf, off, n)
        else:
            p = nn.Parameter(s.to(dt).to(DEV))
        params.append(p)
    return params, bufs


def set_grads(params, grads, k, skip=()):
    for i, (p, gs) in enumerate(zip(params, grads)):
        p.grad = None if (gs is None or i in skip) else gs[k].to(p.dtype).to(DEV)


def bits(t):
    iv = {2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]
    return t.detach().contiguous().view(iv).cpu()


def snap_master(params, opt):
    return [None if p not in opt.state else tuple(bits(opt.state[p][k]) for k in KEYS) + (bits(p),) for p in params]


def snap_plain(params, opt):
    return [None if p not in opt.state else (bits(p), bits(opt.state[p]["exp_avg"]), bits(opt.state[p]["exp_avg_sq"]))
            for p in params]


def cat(ts):
    return torch.cat([t.detach().double().reshape(-1).cpu() for t in ts])


def cat_master(params, opt, idx):
    return {"p": cat([opt.state[params[i]]["master_param"] for i in idx]),
            "exp_avg": cat([opt.state[params[i]]["exp_avg"] for i in idx]),
            "exp_avg_sq": cat([opt.state[params[i]]["exp_avg_sq"] for i in idx])}


def cat_plain(params, opt, idx):
    return {"p": cat([params[i] for i in idx]), "exp_avg": cat([opt.state[params[i]]["exp_avg"] for i in idx]),
            "exp_avg_sq": cat([opt.state[params[i]]["exp_avg_sq"] for i in idx])}


@functools.lru_cache(maxsize=None)
def four_runs(name, wd):
    """The master optimizer in T, its fp32 shadow (this class without the flag) and torch.optim.Adam in
    fp32 and fp64, all from the same T-exact start values and gradients; one run shared by the tests."""
    dt = T16[name]
    specs, start, grads = problem(name)
    runs = {}
    for tag, cls, pdt, kw in (("ours", agn_optim.Adam, dt, dict(master_weights=True)),
                              ("shadow", agn_optim.Adam, torch.float32, {}),
                              ("t32", torch.optim.Adam, torch.float32, dict(foreach=False)),
                              ("t64", torch.optim.Adam, torch.float64, dict(foreach=False))):
        ps, bufs = make_params(specs, start, pdt)
        runs[tag] = dict(params=ps, bufs=bufs, opt=cls(ps, lr=LRS[0], weight_decay=wd, **kw), snaps=[])
    for k, lr in enumerate(LRS):
        for tag, r in runs.items():
            r["opt"].param_groups[0]["lr"] = lr
            set_grads(r["params"], grads, k, skip=(SKIPPED,) if k == SKIP_AT else ())
            r["opt"].step()
            if tag == "ours":
                r["snaps"].append(snap_master(r["params"], r["opt"]))
            elif tag == "shadow":
                r["snaps"].append(snap_plain(r["params"], r["opt"]))
    torch.cuda.synchronize()
    return specs, start, grads, runs


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("name", sorted(T16))
def test_identity_with_the_fp32_kernel(name, wd):
    dt = T16[name]
    specs, start, grads, runs = four_runs(name, wd)
    ours, shadow = runs["ours"], runs["shadow"]
    tabs = ours["opt"].__dict__["_agn_tables"]
    assert [(t.dtype, t.master) for t in tabs.values()] == [(dt, True)]  # the master kernel ran, and only it
    for k in range(len(LRS)):
        for i, (a, b) in enumerate(zip(ours["snaps"][k], shadow["snaps"][k])):
            assert (a is None) == (b is None), (k, i)
            if a is None:
                continue
            for key, x, y in zip(KEYS, a[:3], b):
                assert x.dtype == torch.int32 and torch.equal(x, y), (k, i, specs[i], key)
    for i, (p, q) in enumerate(zip(ours["params"], shadow["params"])):
        if grads[i] is None:  # never a gradient: no state, untouched
            assert p not in ours["opt"].state and torch.equal(bits(p), bits(start[i].to(dt)))
            continue
        st, ss = ours["opt"].state[p], shadow["opt"].state[q]
        assert sorted(st) == ["exp_avg", "exp_avg_sq", "master_param", "step"]
        for key in KEYS:
            assert st[key].dtype == torch.float32 and st[key].shape == p.shape and st[key].device == p.device
        assert torch.equal(bits(p), bits(st["master_param"].to(dt))), (i, specs[i])
        assert st["step"].device.type == "cpu" and st["step"].dtype == ss["step"].dtype
        assert torch.equal(st["step"], ss["step"]) and float(st["step"]) == len(LRS) - (1 if i == SKIPPED else 0)
    # p is the rounded master after every step, not only the last
    for k in range(len(LRS)):
        for i, a in enumerate(ours["snaps"][k]):
            if a is not None:
                w = a[0].view(torch.float32)
                assert torch.equal(a[3], bits(w.to(dt))), (k, i)
    # the elements around the two views are not written
    assert sorted(ours["bufs"]) == [i for i, s in enumerate(specs) if s[1].startswith("view")]
    for i, (buf, off, n) in ours["bufs"].items():
        assert ours["params"][i].data_ptr() % 16 != 0  # the scalar path
        assert float(buf[:off].abs().max()) == 0.0 and float(buf[off + n:].abs().max()) == 0.0, specs[i]
        assert float(buf[off:off + n].abs().max()) > 0.0
    got = dict(ours["opt"].master_parameters())
    assert all(got[p] is ours["opt"].state[p]["master_param"] for p in got)
    assert len(got) == sum(1 for g in grads if g is not None)


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("name", sorted(T16))
def test_against_torch(name, wd):
    specs, start, grads, runs = four_runs(name, wd)
    live = [i for i, gs in enumerate(grads) if gs is not None and start[i].numel() > 0]
    t64 = cat_plain(runs["t64"]["params"], runs["t64"]["opt"], live)
    t32 = cat_plain(runs["t32"]["params"], runs["t32"]["opt"], live)
    assert errs(t32["p"], t64["p"])[0] > 0.0  # torch's own error is not zero
    gate_fp32(cat_master(runs["ours"]["params"], runs["ours"]["opt"], live), t32, t64, f"master {name} wd={wd}")


@pytest.mark.parametrize("name", sorted(T16))
def test_master_follows_the_parameter(name):
    dt = T16[name]
    n = 2 * agn_optim.chunk_elems() + 7
    gen = torch.Generator().manual_seed(21)
    s = rounded(torch.randn(n, generator=gen), dt)
    gs = make_grads((n,), 2, 3, gen, dt)
    p = nn.Parameter(s.to(dt).to(DEV))
    q = nn.Parameter(s.float().to(DEV))
    opt = agn_optim.Adam([p], lr=1e-3, weight_decay=1e-2, master_weights=True)
    sh = agn_optim.Adam([q], lr=1e-3, weight_decay=1e-2)

    def step(k):
        p.grad, q.grad = gs[k].to(dt).to(DEV), gs[k].float().to(DEV)
        opt.step()
        sh.step()
    step(0)
    step(1)
    plan = opt._agn_plan
    touched = torch.zeros(n, dtype=torch.bool, device=DEV)
    touched[::2] = True  # half of the elements, across the wide path, both chunks and the tail
    old = p.detach().clone()
    new = torch.where(old >= 0, old.float() + 1.0, old.float() - 1.0).to(dt)  # other values, one away from 0-wards
    assert bool((bits(new) != bits(old)).all())
    with torch.no_grad():
        p.data[touched] = new[touched]
        q.data[touched] = new[touched].float()  # the shadow restarts there from float(p) and keeps its moments
    w_before = opt.state[p]["master_param"].clone()
    step(2)
    assert opt._agn_plan is plan  # the steady-state path: nothing moved, only values changed
    st, ss = opt.state[p], sh.state[q]
    assert torch.equal(bits(st["master_param"]), bits(q))
    assert torch.equal(bits(st["exp_avg"]), bits(ss["exp_avg"])) and torch.equal(bits(st["exp_avg_sq"]), bits(ss["exp_avg_sq"]))
    assert torch.equal(bits(p), bits(st["master_param"].to(dt)))
    # the untouched elements went on from masters that are not T-representable (else this shows nothing)
    keep = ~touched
    assert bool((w_before[keep].to(dt).float() != w_before[keep]).any())
    moved = (st["master_param"] - w_before).abs()
    assert float(moved[keep].max()) < 0.1 < float(moved[touched].min())


def mixed_problem(nsteps):
    c = agn_optim.chunk_elems()
    layout = [[(torch.bfloat16, (c + 1,)), (torch.float32, (65,)), (torch.float16, (9,))],
              [(torch.float64, (63,)), (torch.bfloat16, (40, 40)), (torch.float16, (2 * c + 7,)), (torch.float32, (7,))]]
    gen = torch.Generator().manual_seed(33)
    specs, start, grads = [], [], []
    for gi, group in enumerate(layout):
        for dt, shape in group:
            i = len(specs)
            specs.append((gi, dt, shape))
            start.append(rounded(torch.randn(shape, generator=gen), dt))
            grads.append(make_grads(shape, i, nsteps, gen, dt))
    return specs, start, grads


GROUP_KW = [dict(lr=1e-3, weight_decay=0.0), dict(lr=5e-4, weight_decay=1e-2)]


def mixed_optimizer(cls, specs, start, up, **kw):
    """The two groups; `up` maps a spec dtype to the dtype this run holds the tensor in."""
    ps = [nn.Parameter(s.to(up(dt)).to(DEV)) for (_, dt, _), s in zip(specs, start)]
    groups = [dict(GROUP_KW[gi], params=[p for p, sp in zip(ps, specs) if sp[0] == gi]) for gi in range(2)]
    return ps, cls(groups, **kw)


def shadow_dtype(dt):
    return torch.float32 if dt in T16.values() else dt


def assert_mixed_equal(specs, po, oo, ps, os_, what):
    """16-bit tensors: master state bitwise the fp32 shadow's, p the rounded master; fp32 / fp64 tensors:
    bitwise the flag-less run's (agn_adam_step unchanged next to the master tables)."""
    for i, (_, dt, _) in enumerate(specs):
        st, ss = oo.state[po[i]], os_.state[ps[i]]
        assert torch.equal(st["step"], ss["step"]), (what, i)
        w = st["master_param"] if dt in T16.values() else po[i]
        assert ("master_param" in st) == (dt in T16.values())
        for x, y in ((w, ps[i]), (st["exp_avg"], ss["exp_avg"]), (st["exp_avg_sq"], ss["exp_avg_sq"])):
            assert x.dtype == y.dtype == shadow_dtype(dt) and torch.equal(bits(x), bits(y)), (what, i, dt)
        assert torch.equal(bits(po[i]), bits(w.to(dt))), (what, i)


def test_mixed_list_groups_replay_and_checkpoint():
    nsteps, skip_at, skipped = 5, 2, 4
    specs, start, grads = mixed_problem(nsteps + 2)
    po, oo = mixed_optimizer(agn_optim.Adam, specs, start, lambda dt: dt, master_weights=True)
    ps, os_ = mixed_optimizer(agn_optim.Adam, specs, start, shadow_dtype)
    p32, o32 = mixed_optimizer(torch.optim.Adam, specs, start, shadow_dtype, foreach=False)
    p64, o64 = mixed_optimizer(torch.optim.Adam, specs, start, lambda dt: torch.float64, foreach=False)
    runs = [(po, oo), (ps, os_), (p32, o32), (p64, o64)]
    assert [g["master_weights"] for g in oo.param_groups] == [True, True]

    def one_step(k, todo, skip=()):
        for params, o in todo:
            set_grads(params, grads, k, skip)
            o.step()
    plan = None
    for k in range(nsteps):
        one_step(k, runs, (skipped,) if k == skip_at else ())
        now = oo.__dict__.get("_agn_plan")
        assert now is not None and (k == 0 or now is plan), k  # steps 1.. replay the plan of step 0
        plan = now
    tabs = oo.__dict__["_agn_tables"]
    assert {t.dtype: t.master for t in tabs.values()} == {torch.bfloat16: True, torch.float16: True,
                                                          torch.float32: False, torch.float64: False}
    assert_mixed_equal(specs, po, oo, ps, os_, "five steps")
    for i in range(len(specs)):
        assert float(oo.state[po[i]]["step"]) == nsteps - (1 if i == skipped else 0)
    i32 = [i for i, sp in enumerate(specs) if sp[1] != torch.float64]
    i64 = [i for i, sp in enumerate(specs) if sp[1] == torch.float64]
    gate_fp32(cat_plain(ps, os_, i32), cat_plain(p32, o32, i32), cat_plain(p64, o64, i32), "mixed list, fp32 side")
    a, b = cat_plain(po, oo, i64), cat_plain(p64, o64, i64)
    for key in a:
        assert errs(a[key], b[key])[0] <= 1e-10, key
    # state.clear(): the plan's tensors are orphans; new state starts from p (the shadow is told so)
    old_w = oo.state[po[0]]["master_param"]
    kept = old_w.clone()
    oo.state.clear()
    os_.state.clear()
    with torch.no_grad():
        for p, q in zip(po, ps):
            q.copy_(p.to(q.dtype))
    one_step(nsteps, runs[:2])
    assert oo._agn_plan is not None and oo._agn_plan is not plan
    assert torch.equal(old_w, kept) and oo.state[po[0]]["master_param"] is not old_w
    assert all(float(oo.state[p]["step"]) == 1.0 for p in po)
    assert_mixed_equal(specs, po, oo, ps, os_, "after state.clear()")
    # a deep copy of the state dict, loaded into a fresh master optimizer, continues bit for bit
    sd = copy.deepcopy(oo.state_dict())
    assert [g["master_weights"] for g in sd["param_groups"]] == [True, True]
    pn = [nn.Parameter(p.detach().clone()) for p in po]
    on = agn_optim.Adam([dict(GROUP_KW[gi], params=[p for p, sp in zip(pn, specs) if sp[0] == gi]) for gi in range(2)],
                        master_weights=True)
    on.load_state_dict(sd)
    for i, (_, dt, _) in enumerate(specs):
        for key in oo.state[po[i]]:
            x, y = on.state[pn[i]][key], oo.state[po[i]][key]
            assert x.dtype == y.dtype and x.device == y.device and torch.equal(bits(x), bits(y)), (i, key)
    one_step(nsteps + 1, [(po, oo), (pn, on)])
    for i in range(len(specs)):
        assert torch.equal(bits(pn[i]), bits(po[i])), i
        for key in oo.state[po[i]]:
            assert torch.equal(bits(on.state[pn[i]][key]), bits(oo.state[po[i]][key])), (i, key)
        assert float(on.state[pn[i]]["step"]) == 2.0


@pytest.mark.parametrize("name", sorted(T16))
def test_it_actually_trains(name):
    """ones(8), gradient ones, lr 1e-3, 200 steps: the flag-less step (torch's, in 16 bits) is printed, not
    asserted; with the flag p is the fp32 trajectory rounded."""
    dt = T16[name]
    p = nn.Parameter(torch.ones(8, dtype=dt, device=DEV))
    q = nn.Parameter(torch.ones(8, device=DEV))
    r = nn.Parameter(torch.ones(8, dtype=dt, device=DEV))
    opt = agn_optim.Adam([p], lr=1e-3, master_weights=True)
    sh = agn_optim.Adam([q], lr=1e-3)
    plain = agn_optim.Adam([r], lr=1e-3)
    hist_p, hist_q = [], []
    for _ in range(200):
        p.grad, q.grad, r.grad = torch.ones_like(p), torch.ones_like(q), torch.ones_like(r)
        opt.step()
        sh.step()
        plain.step()
        hist_p.append(p.detach().clone())
        hist_q.append(q.detach().clone())
    hp, hq = torch.stack(hist_p), torch.stack(hist_q)
    print(f"{name}: 200 steps of lr 1e-3 on 1.0: master weights {float(p.detach()[0]):.8f} (fp32 master "
          f"{float(opt.state[p]['master_param'][0]):.8f}), without the flag {float(r.detach()[0]):.8f}, "
          f"exp_avg_sq {float(plain.state[r]['exp_avg_sq'][0]):.5f} (fp32: {float(sh.state[q]['exp_avg_sq'][0]):.5f})")
    assert torch.equal(bits(hp), bits(hq.to(dt)))
    if dt == torch.bfloat16:  # the first update (1e-3) is under half an ulp (2^-9), the second is not
        assert bool((hp[0] == 1.0).all()) and bool((hp[1] == 0.99609375).all())
    assert bool((hp[1:] != 1.0).all())
    assert float((p.detach().float() - 0.8).abs().max()) <= 2.0 ** -8


def test_whole_model_in_bf16():
    dt = torch.bfloat16
    e = CFG["airfoil_mgn"]
    dims = e["dims"]
    torch.manual_seed(0)
    ma = build(e["model"], dict(e["kwargs"], hidden_dim=32, processor_size=2), dims).to(dt).to(DEV)
    assert ma.__class__.__name__ == "MeshGraphNet"
    mb = copy.deepcopy(ma)
    batches = []
    for b in two_batches(dims):  # 64 nodes each, tiny_batch's layout
        t = {k: (v.to(dt) if v.is_floating_point() else v) for k, v in b.__dict__.items()}
        assert t["x"].shape[0] == 64
        batches.append(t)
    pa, pb = list(ma.parameters()), list(mb.parameters())
    assert all(p.dtype == dt for p in pa)
    oa = agn_optim.Adam(pa, lr=1e-3, weight_decay=1e-2, master_weights=True)
    shadow = [nn.Parameter(p.detach().float()) for p in pb]
    ob = agn_optim.Adam(shadow, lr=1e-3, weight_decay=1e-2)
    loss_fn = agn_train.MSELoss()
    ma.train()
    mb.train()
    for k in range(5):
        t = batches[k % 2]
        la = loss_fn(run_model(ma, t), t["y"])
        la.backward()
        oa.step()
        oa.zero_grad()
        lb = loss_fn(run_model(mb, t), t["y"])
        lb.backward()
        for p, q in zip(pb, shadow):
            assert p.grad is not None and p.grad.dtype == dt
            q.grad = p.grad.float()
        ob.step()
        with torch.no_grad():
            for p, q in zip(pb, shadow):
                p.copy_(q.to(dt))
        mb.zero_grad()
        assert torch.equal(bits(la), bits(lb)), (k, float(la), float(lb))
        for (n, p), q in zip(ma.named_parameters(), pb):
            assert torch.equal(bits(p), bits(q)), (k, n)
    assert len(dict(oa.master_parameters())) == len(pa)
    assert [t.master for t in oa._agn_tables.values()] == [True]


def test_master_step_argument_errors():
    lib = L.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: t.data_ptr()  # noqa: E731
    tab = torch.zeros(ctypes.sizeof(L.AdamMasterDesc), dtype=torch.uint8, device=DEV)
    cmap = torch.zeros(2, dtype=torch.int32, device=DEV)
    f = lib.agn_adam_step_master
    assert f(None, 1, P(cmap), 1, L.BF16, st) == L.E_ARG == -1
    assert f(P(tab), 1, None, 1, L.BF16, st) == L.E_ARG
    assert f(P(tab), -1, P(cmap), 1, L.BF16, st) == L.E_ARG
    assert f(P(tab), 1, P(cmap), -1, L.F16, st) == L.E_ARG
    assert f(P(tab), 1, P(cmap), 1, L.F32, st) == L.E_DTYPE == -2
    assert f(P(tab), 1, P(cmap), 1, L.F64, st) == L.E_DTYPE
    assert f(P(tab), 1, P(cmap), 1, L.BF16, st) == 0  # a zeroed entry (n == 0, null pointers) touches nothing
    assert f(P(tab), 1, P(cmap), 1, L.F16, st) == 0
    assert f(P(tab), 0, P(cmap), 0, L.BF16, st) == 0
    torch.cuda.synchronize()
    assert int(tab.sum()) == 0 and int(cmap.sum()) == 0
