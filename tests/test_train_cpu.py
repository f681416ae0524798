"""CPU-only checks of the training tail's boundary (aerognn.optim, aerognn.train, the agn_mse_loss /
agn_adam_step block of include/aerognn.h): the header declares the entries and the ctypes twin of
agn_adam_desc matches the C layout; on CPU parameters aerognn.optim.Adam IS torch.optim.Adam (the pure
fallback: bitwise steps, state dicts in both directions, ReduceLROnPlateau, the global step pre-hook);
train() / evaluate() with a generic loss_fn return the value of the reference's loop."""
import copy
import ctypes
import types

import numpy as np
import pytest
import torch
from torch import nn

from aerognn import _lib as L
from aerognn import optim as agn_optim
from aerognn import train as agn_train

from abi_layout import check_struct_layouts


def test_header_declares_train_entries():
    names = L.exported_symbols()
    for n in ("agn_mse_loss", "agn_mse_loss_temp_bytes", "agn_mse_chunk_rows", "agn_adam_step", "agn_adam_chunk_elems"):
        assert n in names, n
    lib = L.lib()
    for n in names:
        assert hasattr(lib, n), n
    assert lib.agn_mse_chunk_rows() > 0 and lib.agn_adam_chunk_elems() % 4 == 0
    r = lib.agn_mse_chunk_rows()
    assert lib.agn_mse_loss_temp_bytes(0, 4) >= 8
    assert lib.agn_mse_loss_temp_bytes(r, 4) >= 8 and lib.agn_mse_loss_temp_bytes(r + 1, 4) >= 16
    assert lib.agn_mse_loss_temp_bytes(5, 0) == 0


def test_new_struct_layouts_match_c(tmp_path):
    """The check of test_cpu_boundary.test_struct_layouts_match_c for the struct of this block: its size,
    every field's offset and size, and numpy's view of it, through which aerognn.optim fills the table."""
    seen = check_struct_layouts({"agn_adam_desc": L.AdamDesc}, tmp_path)
    assert seen == 1 + len(L.AdamDesc._fields_) == 14
    assert np.dtype(L.AdamDesc).itemsize == ctypes.sizeof(L.AdamDesc)


def test_chunk_map_covers_every_element_once():
    C = 4096
    numels = [0, 1, 3, C - 1, C, C + 1, 2 * C + 7, 0, 128 * 128]
    cmap = agn_optim.build_chunk_map(numels, C)
    assert cmap.dtype == np.int32 and cmap.shape[1] == 2
    assert len({tuple(r) for r in cmap.tolist()}) == cmap.shape[0]
    for i, n in enumerate(numels):
        cs = sorted(c for t, c in cmap.tolist() if t == i)
        assert cs == list(range((n + C - 1) // C)), (i, n, cs)
    assert agn_optim.build_chunk_map([], C).shape == (0, 2)


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [nn.Parameter(torch.randn(s, generator=g)) for s in ((5, 3), (7,), (2, 2, 2))]


def _set_grads(ps, seed):
    g = torch.Generator().manual_seed(100 + seed)
    for p in ps:
        p.grad = torch.randn(p.shape, generator=g)


def _assert_same(pa, pb, oa, ob):
    for a, b in zip(pa, pb):
        assert torch.equal(a, b)
        sa, sb = oa.state[a], ob.state[b]
        assert sorted(sa) == sorted(sb) == ["exp_avg", "exp_avg_sq", "step"]
        for k in sa:
            assert sa[k].dtype == sb[k].dtype and sa[k].device == sb[k].device and torch.equal(sa[k], sb[k]), k


def test_cpu_parameters_are_the_pure_fallback():
    pa, pb = _params(), _params()
    oa = agn_optim.Adam(pa, lr=1e-3, weight_decay=1e-2)
    ob = torch.optim.Adam(pb, lr=1e-3, weight_decay=1e-2)
    assert isinstance(oa, torch.optim.Adam) and oa.defaults == ob.defaults
    for s in range(3):
        _set_grads(pa, s)
        _set_grads(pb, s)
        oa.step()
        ob.step()
    _assert_same(pa, pb, oa, ob)
    assert oa.state[pa[0]]["step"].dtype == torch.float32 and float(oa.state[pa[0]]["step"]) == 3.0
    sa, sb = oa.state_dict(), ob.state_dict()
    assert sa["param_groups"] == sb["param_groups"] and sorted(sa["state"]) == sorted(sb["state"])


@pytest.mark.parametrize("direction", ["to_torch", "from_torch"])
def test_state_dict_moves_between_the_classes(direction):
    pa, pb = _params(), _params()
    src_cls, dst_cls = ((agn_optim.Adam, torch.optim.Adam) if direction == "to_torch"
                        else (torch.optim.Adam, agn_optim.Adam))
    oa = src_cls(pa, lr=2e-3, weight_decay=1e-2)
    for s in range(2):
        _set_grads(pa, s)
        oa.step()
    for a, b in zip(pa, pb):
        b.data.copy_(a.data)
    ob = dst_cls(pb, lr=1.0)
    ob.load_state_dict(copy.deepcopy(oa.state_dict()))  # as a checkpoint carries it: no tensor shared
    assert ob.param_groups[0]["lr"] == 2e-3
    _set_grads(pa, 7)
    _set_grads(pb, 7)
    oa.step()
    ob.step()
    _assert_same(pa, pb, oa, ob)


def test_reduce_lr_on_plateau_lowers_lr():
    opt = agn_optim.Adam(_params(), lr=1e-3)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", factor=0.8, patience=0, min_lr=1e-7)
    sched.step(1.0)
    sched.step(2.0)
    assert opt.param_groups[0]["lr"] == pytest.approx(8e-4, rel=1e-12)


@pytest.mark.parametrize("torch_first", [False, True])
def test_global_step_pre_hook_fires_once_per_step(torch_first):
    """Also with torch.optim.Adam's own step already wrapped by torch's hook runner (an instance of
    the base class exists), which the fallback must not run a second time."""
    from torch.optim.optimizer import register_optimizer_step_pre_hook
    if torch_first:
        torch.optim.Adam(_params(), lr=1e-3)
    ps = _params()
    opt = agn_optim.Adam(ps, lr=1e-3)
    calls = []
    h = register_optimizer_step_pre_hook(lambda o, a, k: calls.append(o))
    try:
        for s in range(2):
            _set_grads(ps, s)
            opt.step()
    finally:
        h.remove()
    assert calls == [opt, opt]


def test_uncovered_settings_run_torch_step():
    """amsgrad and a closure are torch.optim.Adam's own step, bitwise."""
    pa, pb = _params(), _params()
    oa = agn_optim.Adam(pa, lr=1e-3, amsgrad=True)
    ob = torch.optim.Adam(pb, lr=1e-3, amsgrad=True)
    _set_grads(pa, 0)
    _set_grads(pb, 0)
    assert oa.step(lambda: torch.tensor(3.0)) == ob.step(lambda: torch.tensor(3.0))
    for a, b in zip(pa, pb):
        assert torch.equal(a, b)
        assert torch.equal(oa.state[a]["max_exp_avg_sq"], ob.state[b]["max_exp_avg_sq"])


# ----------------------------------------------------------------------------- train / evaluate
class _Batch(types.SimpleNamespace):
    def to(self, device):
        return self


def _loader(with_pos=True):
    g = torch.Generator().manual_seed(3)
    out = []
    for n in (6, 9):
        b = _Batch(x=torch.randn(n, 5, generator=g), edge_attr=torch.randn(2 * n, 3, generator=g),
                   edge_index=torch.randint(0, n, (2, 2 * n), generator=g), batch=torch.zeros(n, dtype=torch.long),
                   y=torch.randn(n, 4, generator=g))
        if with_pos:
            b.pos = torch.randn(n, 3, generator=g)
        out.append(b)
    return out


def _stub(name, check):
    """A module class called `name` whose forward asserts the call utils.py:178-189 makes for it."""
    def forward(self, *a, **k):
        check(a, k)
        return self.lin(a[0])

    def init(self):
        nn.Module.__init__(self)
        torch.manual_seed(0)
        self.lin = nn.Linear(5, 4)
    return type(name, (nn.Module,), {"__init__": init, "forward": forward})()


def _is(a, n, keys):
    def check(args, kw):
        assert len(args) == n and sorted(kw) == sorted(keys), (len(args), sorted(kw))
    return check


STUBS = {"poolMGN": _is(None, 4, []), "MeshGraphNet_v2": _is(None, 4, []),
         "BiStridedMeshGraphNet": _is(None, 3, ["batch", "pos"]), "MLPNet": _is(None, 1, []),
         "MeshGraphNet": _is(None, 3, [])}


def _reference_forward(model, batch):
    model_class = model.__class__.__name__
    if model_class in ['poolMGN', 'MeshGraphNet_v2']:
        return model(batch.x, batch.edge_attr, batch.edge_index, batch.batch)
    elif model_class in ['BiStridedMeshGraphNet']:
        pos = batch.pos if hasattr(batch, 'pos') else None
        return model(batch.x, batch.edge_attr, batch.edge_index, batch=batch.batch, pos=pos)
    elif model_class in ['MLPNet']:
        return model(batch.x)
    return model(batch.x, batch.edge_attr, batch.edge_index)


def _reference_train(model, loader, optimizer, loss_fn, device):
    model.train()
    total_loss = 0.0
    for batch in loader:
        batch = batch.to(device)
        pred = _reference_forward(model, batch)
        loss = loss_fn(pred, batch.y)
        loss.backward()
        optimizer.step()
        optimizer.zero_grad()
        total_loss += loss.item()
    return total_loss / len(loader)


@torch.no_grad()
def _reference_evaluate(model, loader, loss_fn, device):
    model.eval()
    total_loss = 0.0
    for batch in loader:
        batch = batch.to(device)
        pred = _reference_forward(model, batch)
        loss = loss_fn(pred, batch.y)
        total_loss += loss.item()
    return total_loss / len(loader)


@pytest.mark.parametrize("name", sorted(STUBS))
@pytest.mark.parametrize("loss_name", ["l1", "mse"])
def test_train_and_evaluate_match_the_reference_loop_on_cpu(name, loss_name):
    """A generic loss_fn (and nn.MSELoss on a CPU model, which has no device path) runs the reference's
    loop as written: the same floats, the same parameters."""
    loss_fn = nn.L1Loss() if loss_name == "l1" else nn.MSELoss()
    loader = _loader()
    ma, mb = _stub(name, STUBS[name]), _stub(name, STUBS[name])
    assert ma.__class__.__name__ == name
    oa = agn_optim.Adam(ma.parameters(), lr=1e-2, weight_decay=1e-2)
    ob = torch.optim.Adam(mb.parameters(), lr=1e-2, weight_decay=1e-2)
    for _ in range(2):
        got = agn_train.train(ma, loader, oa, loss_fn, "cpu")
        want = _reference_train(mb, loader, ob, loss_fn, "cpu")
        assert isinstance(got, float) and got == want
    for a, b in zip(ma.parameters(), mb.parameters()):
        assert torch.equal(a, b) and a.grad is None
    assert agn_train.evaluate(ma, loader, loss_fn, "cpu") == _reference_evaluate(mb, loader, loss_fn, "cpu")
    assert not ma.training


def test_bistride_dispatch_without_pos():
    seen = {}

    def check(args, kw):
        seen.update(kw)
    m = _stub("BiStridedMeshGraphNet", check)
    agn_train.evaluate(m, _loader(with_pos=False), nn.L1Loss(), "cpu")
    assert seen["pos"] is None and seen["batch"] is not None


def test_device_entry_points_refuse_cpu_tensors():
    with pytest.raises(RuntimeError):
        agn_train.mse_loss_grad(torch.zeros(3, 4), torch.zeros(3, 4))
    with pytest.raises(RuntimeError):
        agn_train.MSELoss()(torch.zeros(3, 4, requires_grad=True), torch.zeros(3, 4))
