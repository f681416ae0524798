"""CPU-only checks of the loss-scaling block of include/aerognn.h and of aerognn.train.LossScaler: the header
declares the five entry points with the types the binding needs (device tables and the device state as
plain addresses), agn_loss_scale_state has the C compiler's layout (16 bytes, offsets 0 / 4 / 8 / 12), every
argument error comes back before a launch, the constructor validates, and the state dict has
torch.amp.GradScaler's keys and moves between the two classes."""
import ctypes

import numpy as np
import pytest
import torch
from torch import nn

from abi_layout import check_struct_layouts
from aerognn import _lib as L
from aerognn import optim as agn_optim
from aerognn import train as agn_train

I, D, P = ctypes.c_int, ctypes.c_double, ctypes.c_void_p
MSE_ARGS = [I, I, I, I, P, I, P, I, D, P, P, P, I, P]
NEW = {
    "agn_mse_loss_scaled": MSE_ARGS + [P, P],
    "agn_grad_check": [P, I, I, P, I, I, P, P],
    "agn_adam_step_scaled": [P, I, P, I, I, P, P],
    "agn_adam_step_master_scaled": [P, I, P, I, I, P, P],
    "agn_loss_scale_update": [P, D, D, I, P],
}


def test_header_declares_the_loss_scale_entries():
    lib = L.lib()
    for name, args in NEW.items():
        assert name in L.exported_symbols() and name in L.LAUNCHES and hasattr(lib, name), name
        res, got = L.PROTOS[name]
        assert res is I and got == args, (name, got)
    # the scaled entries are the unscaled ones with the state in front of the stream
    for name in ("agn_mse_loss", "agn_adam_step", "agn_adam_step_master"):
        old, new = L.PROTOS[name][1], L.PROTOS[name + "_scaled"][1]
        assert new == old[:-1] + [P, P] and old[-1] is P, name


def test_state_layout_matches_c(tmp_path):
    S = L.LossScaleState
    assert [(f, t) for f, t in S._fields_] == [("scale", ctypes.c_float), ("found_inf", I), ("growth_tracker", I),
                                               ("skipped", I)]
    seen = check_struct_layouts({"agn_loss_scale_state": S}, tmp_path)
    assert seen == 5
    assert ctypes.sizeof(S) == 16 == np.dtype(S).itemsize
    assert [getattr(S, f).offset for f, _ in S._fields_] == [0, 4, 8, 12]
    assert all(getattr(S, f).size == 4 for f, _ in S._fields_)


def test_argument_errors_return_before_any_launch():
    """None of these calls reaches the device (this test runs without one): the addresses are host bytes
    that nothing dereferences."""
    lib = L.lib()
    buf = ctypes.create_string_buffer(256)
    a = ctypes.addressof(buf)
    assert (L.E_ARG, L.E_DTYPE, L.E_SHAPE) == (-1, -2, -4)

    def mse(dtype=L.F16, y_dtype=L.F16, n=8, f=4, p=a, pld=4, yy=a, yld=4, ng=32.0, lo=a, d=a, dld=4, s=a, state=a):
        return lib.agn_mse_loss_scaled(dtype, y_dtype, n, f, p, pld, yy, yld, ng, lo, None, d, dld, s, state, None)
    for state in (a, None):  # with and without a state: agn_mse_loss's checks
        assert mse(n=-1, state=state) == L.E_ARG and mse(lo=None, state=state) == L.E_ARG
        assert mse(dtype=7, state=state) == L.E_DTYPE and mse(y_dtype=L.BF16, state=state) == L.E_DTYPE
        assert mse(f=0, state=state) == L.E_SHAPE and mse(pld=3, state=state) == L.E_SHAPE
        assert mse(yld=3, state=state) == L.E_SHAPE and mse(dld=3, state=state) == L.E_SHAPE
        assert mse(ng=0.0, state=state) == L.E_SHAPE and mse(ng=-1.0, state=state) == L.E_SHAPE

    chk = lib.agn_grad_check
    for master in (0, 1):
        assert chk(None, master, 1, a, 1, L.F16, a, None) == L.E_ARG
        assert chk(a, master, 1, None, 1, L.F16, a, None) == L.E_ARG
        assert chk(a, master, 1, a, 1, L.F16, None, None) == L.E_ARG
        assert chk(a, master, 0, a, 0, L.F16, None, None) == L.E_ARG  # a null state also where nothing would run
        assert chk(a, master, -1, a, 1, L.F32, a, None) == L.E_ARG
        assert chk(a, master, 1, a, -1, L.F64, a, None) == L.E_ARG
        assert chk(a, master, 1, a, 1, 7, a, None) == L.E_DTYPE and chk(a, master, 1, a, 1, -1, a, None) == L.E_DTYPE
        for dt in (L.F32, L.F64, L.BF16, L.F16):  # an empty table or map: nothing to read, no launch
            assert chk(a, master, 0, a, 1, dt, a, None) == 0 and chk(a, master, 1, a, 0, dt, a, None) == 0

    for f, good, bad in ((lib.agn_adam_step_scaled, (L.F32, L.F64), (L.BF16, L.F16, 7)),
                         (lib.agn_adam_step_master_scaled, (L.BF16, L.F16), (L.F32, L.F64, 7))):
        for dt in good:
            assert f(None, 1, a, 1, dt, a, None) == L.E_ARG
            assert f(a, 1, None, 1, dt, a, None) == L.E_ARG
            assert f(a, 1, a, 1, dt, None, None) == L.E_ARG
            assert f(a, -1, a, 1, dt, a, None) == L.E_ARG and f(a, 1, a, -1, dt, a, None) == L.E_ARG
            assert f(a, 0, a, 0, dt, a, None) == 0
        for dt in bad:
            assert f(a, 1, a, 1, dt, a, None) == L.E_DTYPE

    upd = lib.agn_loss_scale_update
    assert upd(None, 2.0, 0.5, 2000, None) == L.E_ARG
    assert upd(a, 2.0, 0.5, 0, None) == L.E_SHAPE and upd(a, 2.0, 0.5, -3, None) == L.E_SHAPE
    assert upd(a, 0.0, 0.5, 2000, None) == L.E_SHAPE and upd(a, -2.0, 0.5, 2000, None) == L.E_SHAPE
    assert upd(a, 2.0, 0.0, 2000, None) == L.E_SHAPE and upd(a, 2.0, -0.5, 2000, None) == L.E_SHAPE
    assert upd(a, float("nan"), 0.5, 2000, None) == L.E_SHAPE
    assert bytes(buf) == bytes(256)


@pytest.mark.parametrize("kw", [dict(init_scale=0.0), dict(init_scale=-1.0), dict(init_scale=float("inf")),
                                dict(init_scale=float("nan")), dict(init_scale=1e39), dict(growth_factor=1.0),
                                dict(growth_factor=0.5), dict(growth_factor=float("inf")), dict(backoff_factor=1.0),
                                dict(backoff_factor=0.0), dict(backoff_factor=-0.5), dict(growth_interval=0),
                                dict(growth_interval=-1), dict(growth_interval=2.5), dict(device="cpu")])
def test_constructor_validates(kw):
    with pytest.raises(ValueError, match="LossScaler"):
        agn_train.LossScaler(**kw)


def test_defaults_and_state_dict_are_grad_scalers():
    ours, theirs = agn_train.LossScaler(), torch.amp.GradScaler("cpu")
    sa, sb = ours.state_dict(), theirs.state_dict()
    assert list(sa) == list(sb) == ["scale", "growth_factor", "backoff_factor", "growth_interval", "_growth_tracker"]
    assert sa == sb  # the defaults too: 2^16, 2, 0.5, 2000, tracker 0
    assert {k: type(v) for k, v in sa.items()} == {k: type(v) for k, v in sb.items()}
    assert ours.get_scale() == 65536.0 and ours.steps_skipped() == 0
    # a checkpoint of either loads into the other (no device state yet: the values are kept for its creation)
    src = dict(scale=4096.0, growth_factor=1.5, backoff_factor=0.75, growth_interval=7, _growth_tracker=3)
    ours.load_state_dict(dict(src))
    assert ours.state_dict() == src and ours.get_scale() == 4096.0
    theirs.load_state_dict(ours.state_dict())
    assert theirs.state_dict() == src
    fresh = agn_train.LossScaler(init_scale=2.0)
    fresh.load_state_dict(theirs.state_dict())
    assert fresh.state_dict() == src
    assert (fresh.get_growth_factor(), fresh.get_backoff_factor(), fresh.get_growth_interval()) == (1.5, 0.75, 7)
    with pytest.raises(RuntimeError, match="empty"):
        fresh.load_state_dict({})


def _params(dtype=torch.float32):
    g = torch.Generator().manual_seed(3)
    ps = [nn.Parameter(torch.randn(s, generator=g).to(dtype)) for s in ((5, 3), (7,))]
    for p in ps:
        p.grad = torch.randn(p.shape, generator=g).to(dtype)
    return ps


def test_step_refuses_what_would_take_torchs_step():
    """Before anything is changed: torch's own step would apply the scaled gradients."""
    s = agn_train.LossScaler()
    ps = _params()
    with pytest.raises(RuntimeError, match="needs an aerognn.optim.Adam"):
        s.step(torch.optim.Adam(ps, lr=1e-3))
    opt = agn_optim.Adam(ps, lr=1e-3)
    with pytest.raises(RuntimeError, match="closure"):
        s.step(opt, lambda: torch.tensor(1.0))
    with pytest.raises(RuntimeError, match="closure"):
        opt.step(lambda: torch.tensor(1.0), scaler=s)
    before = [p.detach().clone() for p in ps]
    with pytest.raises(RuntimeError, match=r"parameter 0 of group 0 .*cannot take the loss-scaled step"):
        s.step(opt)  # CPU parameters
    amsgrad = agn_optim.Adam(_params(), lr=1e-3, amsgrad=True)
    with pytest.raises(RuntimeError, match="amsgrad"):
        s.step(amsgrad)
    assert not opt.state and not amsgrad.state and all(torch.equal(p, q) for p, q in zip(ps, before))
    # without gradients nothing would be stepped by either: no error, no state, no device
    for p in ps:
        p.grad = None
    assert s.step(opt) is None and not opt.state
    # step() without a scaler is torch's on these CPU parameters, as before
    pa, pb = _params(), _params()
    oa, ob = agn_optim.Adam(pa, lr=1e-3), torch.optim.Adam(pb, lr=1e-3)
    oa.step()
    ob.step()
    assert all(torch.equal(a, b) for a, b in zip(pa, pb))


def test_train_with_a_scaler_needs_the_fused_loss():
    import types
    model = nn.Linear(5, 4)
    batch = types.SimpleNamespace(x=torch.zeros(3, 5), edge_attr=None, edge_index=None, y=torch.zeros(3, 4))
    batch.to = lambda device: batch
    model.__class__ = type("MLPNet", (nn.Linear,), {})
    opt = agn_optim.Adam(model.parameters(), lr=1e-3)
    before = [p.detach().clone() for p in model.parameters()]
    with pytest.raises(RuntimeError, match="LossScaler needs the fused loss"):
        agn_train.train(model, [batch], opt, nn.MSELoss(), "cpu", scaler=agn_train.LossScaler())
    assert all(torch.equal(p, q) for p, q in zip(model.parameters(), before)) and not opt.state
