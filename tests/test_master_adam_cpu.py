"""CPU-only checks of the master-weight mode of aerognn.optim.Adam (`master_weights=True`) and of the
agn_adam_step_master block of include/aerognn.h: the header declares the entry and the ctypes twin of
agn_adam_master_desc matches the C layout; without the flag the class is torch.optim.Adam as before;
with it the flag is a group option, nothing is downgraded to torch's 16-bit step (RuntimeError /
ValueError instead), and load_state_dict keeps the fp32 state that torch's would cast to bf16."""
import copy
import ctypes

import numpy as np
import pytest
import torch
from torch import nn

from abi_layout import check_struct_layouts
from aerognn import _lib as L
from aerognn import optim as agn_optim


def _params(dtype=torch.float32):
    g = torch.Generator().manual_seed(3)
    return [nn.Parameter(torch.randn(s, generator=g).to(dtype)) for s in ((5, 3), (7,))]


def _set_grads(ps):
    g = torch.Generator().manual_seed(4)
    for p in ps:
        p.grad = torch.randn(p.shape, generator=g).to(p.dtype)


def test_header_declares_the_master_step():
    assert "agn_adam_step_master" in L.exported_symbols()
    assert "agn_adam_step_master" in L.LAUNCHES
    assert hasattr(L.lib(), "agn_adam_step_master")
    res, args = L.PROTOS["agn_adam_step_master"]
    # the table is a device address, not a ctypes pointer to a host struct
    assert res is ctypes.c_int and args == [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_void_p]


def test_master_desc_layout_matches_c(tmp_path):
    names = [f for f, _ in L.AdamMasterDesc._fields_]
    assert names == ["p", "g", "w", "m", "v", "n", "dtype", "_pad", "beta1", "beta2", "eps", "weight_decay", "step_size",
                     "bc2_sqrt"]
    seen = check_struct_layouts({"agn_adam_master_desc": L.AdamMasterDesc, "agn_adam_desc": L.AdamDesc}, tmp_path)
    assert seen == 2 + len(L.AdamMasterDesc._fields_) + len(L.AdamDesc._fields_) == 2 + 14 + 13
    assert np.dtype(L.AdamMasterDesc).itemsize == ctypes.sizeof(L.AdamMasterDesc)
    # the six scalars sit as in agn_adam_desc, one pointer further on
    for f in ("n", "dtype", "beta1", "beta2", "eps", "weight_decay", "step_size", "bc2_sqrt"):
        assert getattr(L.AdamMasterDesc, f).offset == getattr(L.AdamDesc, f).offset + 8, f


def test_without_the_flag_nothing_changes():
    pa, pb = _params(), _params()
    oa = agn_optim.Adam(pa, lr=1e-3, weight_decay=1e-2)
    ob = torch.optim.Adam(pb, lr=1e-3, weight_decay=1e-2)
    oe = agn_optim.Adam(_params(), lr=1e-3, weight_decay=1e-2, master_weights=False)
    for o in (oa, oe):
        assert o.defaults == ob.defaults and "master_weights" not in o.defaults
        assert [{k: v for k, v in g.items() if k != "params"} for g in o.param_groups] == \
               [{k: v for k, v in g.items() if k != "params"} for g in ob.param_groups]
        assert list(o.master_parameters()) == []
    _set_grads(pa)
    _set_grads(pb)
    oa.step()
    ob.step()
    sa, sb = oa.state_dict(), ob.state_dict()
    assert sa["param_groups"] == sb["param_groups"] and sorted(sa["state"]) == sorted(sb["state"])
    for k in sa["state"]:
        assert sorted(sa["state"][k]) == sorted(sb["state"][k]) == ["exp_avg", "exp_avg_sq", "step"]
        for name in sa["state"][k]:
            assert torch.equal(sa["state"][k][name], sb["state"][k][name]), (k, name)


def test_the_flag_is_a_group_option():
    ps = _params(torch.bfloat16)
    opt = agn_optim.Adam(ps, lr=1e-3, master_weights=True)
    assert opt.defaults["master_weights"] is True
    assert opt.state_dict()["param_groups"][0]["master_weights"] is True
    extra = nn.Parameter(torch.zeros(3, dtype=torch.bfloat16))
    opt.add_param_group({"params": [extra], "lr": 5e-4})
    assert opt.param_groups[1]["master_weights"] is True and opt.param_groups[1]["lr"] == 5e-4
    # per group: one group with it, one without
    a, b = _params(torch.bfloat16)
    mixed = agn_optim.Adam([{"params": [a], "master_weights": True}, {"params": [b]}], lr=1e-3)
    assert "master_weights" not in mixed.defaults
    assert mixed.param_groups[0]["master_weights"] is True and "master_weights" not in mixed.param_groups[1]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_cpu_16bit_parameter_raises_instead_of_torch_step(dtype):
    ps = _params(dtype)
    opt = agn_optim.Adam(ps, lr=1e-3, master_weights=True)
    _set_grads(ps)
    before = [p.detach().clone() for p in ps]
    with pytest.raises(RuntimeError, match=r"parameter 0 of group 0 .*cannot take the master-weight step.*cpu"):
        opt.step()
    assert not opt.state  # torch's 16-bit step did not run
    for p, q in zip(ps, before):
        assert torch.equal(p, q)


def test_closure_raises():
    ps = _params()
    opt = agn_optim.Adam(ps, lr=1e-3, master_weights=True)
    _set_grads(ps)
    with pytest.raises(RuntimeError, match="closure"):
        opt.step(lambda: torch.tensor(1.0))
    assert not opt.state


@pytest.mark.parametrize("kw", [dict(amsgrad=True), dict(maximize=True), dict(decoupled_weight_decay=True),
                                dict(lr=torch.tensor(1e-3))])
def test_uncovered_options_raise_at_construction(kw):
    with pytest.raises(ValueError, match="master_weights=True cannot be combined"):
        agn_optim.Adam(_params(torch.bfloat16), master_weights=True, **kw)


def test_uncovered_options_are_rechecked_at_step():
    ps = _params()
    opt = agn_optim.Adam(ps, lr=1e-3, master_weights=True)
    _set_grads(ps)
    opt.param_groups[0]["amsgrad"] = True
    with pytest.raises(ValueError, match="amsgrad"):
        opt.step()
    assert not opt.state


def test_fp32_cpu_parameters_of_a_master_group_take_torch_step():
    """Only 16-bit parameters have a master copy; an fp32 CPU parameter runs torch's step as before."""
    pa, pb = _params(), _params()
    oa = agn_optim.Adam(pa, lr=1e-3, weight_decay=1e-2, master_weights=True)
    ob = torch.optim.Adam(pb, lr=1e-3, weight_decay=1e-2)
    _set_grads(pa)
    _set_grads(pb)
    oa.step()
    ob.step()
    for a, b in zip(pa, pb):
        assert torch.equal(a, b)
    assert list(oa.master_parameters()) == []


def _hand_built_state():
    """A state dict for one bf16 parameter of 6 elements whose fp32 tensors are not bf16-representable."""
    g = torch.Generator().manual_seed(11)
    t = {k: torch.randn(6, generator=g) * s + 2.0 ** -20 for k, s in
         (("exp_avg", 1e-2), ("exp_avg_sq", 1e-4), ("master_param", 1.0))}
    t["exp_avg_sq"] = t["exp_avg_sq"].abs()
    for v in t.values():
        assert v.dtype == torch.float32 and not torch.equal(v.bfloat16().float(), v)
    return t


def _loaded(cls, master, tensors, group_has_flag):
    p = nn.Parameter(tensors["master_param"].bfloat16())
    kw = dict(master_weights=True) if master else {}
    opt = cls([p], lr=1e-3, **kw)
    sd = opt.state_dict()
    if not group_has_flag:
        sd["param_groups"][0].pop("master_weights", None)
    sd["state"] = {0: dict(step=torch.tensor(7.0), **{k: v.clone() for k, v in tensors.items()})}
    opt.load_state_dict(copy.deepcopy(sd))
    return p, opt


@pytest.mark.parametrize("group_has_flag", [True, False])
def test_load_state_dict_keeps_fp32_state(group_has_flag):
    tensors = _hand_built_state()
    p, opt = _loaded(agn_optim.Adam, True, tensors, group_has_flag)
    st = opt.state[p]
    assert opt.param_groups[0]["master_weights"] is True  # also when the checkpoint's group has no such key
    assert float(st["step"]) == 7.0 and st["step"].device.type == "cpu"
    for k, want in tensors.items():
        assert st[k].dtype == torch.float32 and st[k].device == p.device, k
        assert torch.equal(st[k].view(torch.int32), want.view(torch.int32)), k
    (q, w), = list(opt.master_parameters())
    assert q is p and w is st["master_param"]
    # the override is what keeps them: torch's own load casts the same dict to the parameter's dtype
    pt, ot = _loaded(torch.optim.Adam, False, tensors, False)
    for k in tensors:
        assert ot.state[pt][k].dtype == torch.bfloat16, k


def test_load_of_a_plain_checkpoint_upcasts_its_moments():
    """16-bit moments (a run without the flag) come out fp32 with the same values; master_param is made
    at the next step, so there is none yet."""
    m = torch.tensor([0.5, -0.25, 3.0], dtype=torch.bfloat16)
    v = torch.tensor([0.125, 2.0, 0.0], dtype=torch.bfloat16)
    p = nn.Parameter(torch.ones(3, dtype=torch.bfloat16))
    opt = agn_optim.Adam([p], lr=1e-3, master_weights=True)
    plain = torch.optim.Adam([nn.Parameter(torch.ones(3, dtype=torch.bfloat16))], lr=1e-3).state_dict()
    plain["state"] = {0: dict(step=torch.tensor(2.0), exp_avg=m, exp_avg_sq=v)}
    opt.load_state_dict(plain)
    st = opt.state[p]
    assert st["exp_avg"].dtype == st["exp_avg_sq"].dtype == torch.float32 and "master_param" not in st
    assert torch.equal(st["exp_avg"], m.float()) and torch.equal(st["exp_avg_sq"], v.float())
    assert opt.param_groups[0]["master_weights"] is True and list(opt.master_parameters()) == []
