"""Every kernel off the default stream (tests/streamcheck.py has the method).

aerognn/core.py promises that every launch goes to the caller's current HIP stream and that nothing
synchronises. The library is deterministic, so no tolerance is needed: a call on a side stream must give
the bits of the same call on the default stream, also when its inputs arrive late on that stream and also
when the default stream is busy. The cases: every case of launch_cases.CASES (a), the table of
stream_cases.py for what those do not reach (b), two streams sharing the library's own state (c), the
exit status after a device fault word was set (d), and autograd handing our backward to the forward's
stream. The last test compares the entry points each case was seen calling with stream_cases.COVERED.

Each case prints its measured host time and the spins chosen from it (pytest -s shows them).
"""
import subprocess
import sys

import pytest
import torch

import launch_cases
import stream_cases
import streamcheck as SC

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def rate():
    """torch.cuda._sleep cycles per millisecond on this device, measured once."""
    return SC.cycles_per_ms()


@pytest.fixture(scope="module")
def side(rate):
    """One side stream for every case: one that the device runs next to the default stream."""
    return SC.concurrent_stream(rate)


# ------------------------------------------------------------------------------- a, b
@pytest.mark.parametrize("name", list(launch_cases.CASES))
def test_launch_case_off_the_default_stream(name, rate, side, monkeypatch):
    SC.check(name, SC.launch_case(name, monkeypatch.setenv), rate, side, monkeypatch)


@pytest.mark.parametrize("name", list(stream_cases.CASES))
def test_stream_case_off_the_default_stream(name, rate, side, monkeypatch):
    build, syncs = stream_cases.CASES[name]
    SC.check(name, build, rate, side, monkeypatch, syncs=syncs)


# ------------------------------------------------------------------------------- autograd hand-over
def _model_case():
    import irregular_graphs as G
    from aerognn.data import compute_edge_attr
    from models.bsms_mgn import BiStridedMeshGraphNet
    from test_gpu_irregular import _model_kw
    n, ei, batch = G.family("hub")
    pos, _, _ = G.features(n, ei.shape[1], 1, seed=21)
    g = torch.Generator().manual_seed(22)
    x, y = torch.randn(n, 6, generator=g).to(DEV), torch.randn(n, 4, generator=g).to(DEV)
    ei, batch, pos = ei.to(DEV), batch.to(DEV), pos.to(DEV)
    ea = compute_edge_attr(pos=pos, edge_index=ei)
    torch.manual_seed(2)
    model = BiStridedMeshGraphNet(6, 4, 4, **_model_kw(2, 3, "add", True)).to(DEV)
    return model, (x, ea, ei, batch, pos, y)


def _train_step(model, t, backward_inside, s=None):
    x, ea, ei, batch, pos, y = t
    model.zero_grad(set_to_none=True)
    if s is None:
        torch.nn.functional.mse_loss(model(x, ea, ei, batch=batch, pos=pos), y).backward()
        torch.cuda.synchronize()
    else:
        with torch.cuda.stream(s):
            loss = torch.nn.functional.mse_loss(model(x, ea, ei, batch=batch, pos=pos), y)
            if backward_inside:
                loss.backward()
        if not backward_inside:
            loss.backward()  # autograd runs every backward node on its forward's stream
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
    return {k: SC.bits(p.grad) for k, p in model.named_parameters()}


def test_autograd_runs_the_backward_on_the_forward_stream(monkeypatch):
    """One fp32 BSMS train step on the hub graph with the forward under torch.cuda.stream(s) and
    loss.backward() called outside it: the gradients are read after the current stream has waited for s
    and must be the bits of the step on the default stream. The model builds its pooling maps, which
    block the host, so no spin can be kept busy across the call: this compares results only."""
    from aerognn import _lib as L
    from aerognn import core
    monkeypatch.setattr(core, "CHECK_FAULTS", False)
    model, t = _model_case()
    torch.cuda.synchronize()
    with SC.recording("bsms_model_step"):
        ref = _train_step(model, t, True)
        s = torch.cuda.Stream()
        for inside in (True, False):
            got = _train_step(model, t, inside, s)
            bad = SC.differing(got, ref)
            assert not bad, f"backward {'inside' if inside else 'outside'} the stream block: {bad} differ"
    assert L.fault_status(reset=True) == 0


# ------------------------------------------------------------------------------- c
def test_two_streams_share_the_library_state(monkeypatch):
    """L_gmp_train (65,536 nodes) on s1 and the same builder at 70,000 nodes on s2 (the LayerNorm
    workspace of csrc/node32_bwd.hip grows), enqueued back to back without a host wait between them; then
    in the other order; then one of them on the default stream. Each result must be the bits of its solo
    run. This exercises the state the streams share (the workspace, the fault word, the kernel-mode
    record). It could not be made to fail deterministically before the workspace's reuse was ordered
    after its last user: the write and the read of the workspace are issued by one C call, so a
    missing wait shows only when the device happens to overlap the two calls. The ordering is verified
    by reading the code; this test runs once and repeats nothing to make a race show."""
    from aerognn import _lib as L
    from aerognn import core
    monkeypatch.setattr(core, "CHECK_FAULTS", False)
    for k, v in list(core._fault.items()):
        monkeypatch.setitem(core._fault, k, v)
    monkeypatch.setitem(core._fault, "hooked", True)
    builder, kw, _ = launch_cases.CASES["L_gmp_train"]
    cases = []
    for shape in (launch_cases.LARGE, (70000, 131072)):
        fwd, leaves = builder(**dict(kw, shape=shape))
        cases.append((fwd, leaves))
    gs = [None, None]

    def run(i):
        fwd, leaves = cases[i]
        for t in leaves.values():
            t.grad = None
        outs = fwd()
        if gs[i] is None:
            gs[i] = [torch.randn(o.shape, generator=launch_cases._gen(7 + j)).to(o.dtype).to(DEV)
                     for j, o in enumerate(outs.values())]
        torch.autograd.backward(list(outs.values()), gs[i])
        res = {k: v.detach() for k, v in outs.items()}
        res.update({"d " + k: t.grad for k, t in leaves.items()})
        return res

    def host(res):
        return {k: SC.bits(v) for k, v in res.items()}

    before = L.lib().agn_debug_node32_bwd_launches()
    solo = []
    for i in (0, 1):
        res = run(i)
        torch.cuda.synchronize()
        solo.append(host(res))
    assert L.lib().agn_debug_node32_bwd_launches() == before + 2  # the kernel that owns the workspace ran
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for order, streams in (((0, 1), (s1, s2)), ((1, 0), (s2, s1)), ((1, 0), (s1, None)), ((0, 1), (None, s2))):
        res = {}
        for i, s in zip(order, streams):
            if s is None:
                res[i] = run(i)
            else:
                with torch.cuda.stream(s):
                    res[i] = run(i)
        torch.cuda.synchronize()
        for i in order:
            bad = SC.differing(host(res[i]), solo[i])
            assert not bad, f"case {i} of order {order} on {streams}: {bad} differ from the solo run"
    assert L.fault_status(reset=True) == 0


# ------------------------------------------------------------------------------- d
_CHILD = """
import sys
sys.path[:0] = {paths!r}
from aerognn import _lib as L
from aerognn import core
core._poll_faults()
if {fault}:
    assert L.lib().agn_debug_set_fault(1) == 0
print("child done", flush=True)
"""


@pytest.mark.parametrize("fault", [True, False])
def test_exit_status_after_a_fault(fault):
    """A fresh process whose fault word is set after its last poll (agn_debug_set_fault only writes the
    word; no GPU fault is involved) and that returns normally must end with a nonzero status and name the
    device fault word on stderr; the same process without the word set exits 0."""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = _CHILD.format(paths=[root, os.path.join(root, "aero-gnn_amd")], fault=fault)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert "child done" in r.stdout, r.stderr
    if fault:
        assert r.returncode != 0, (r.returncode, r.stderr)
        assert "device fault word" in r.stderr, r.stderr
    else:
        assert r.returncode == 0, (r.returncode, r.stderr)
        assert "device fault word" not in r.stderr, r.stderr


# ------------------------------------------------------------------------------- completeness
def test_observed_entry_points_cover_the_declared_ones():
    """What the counting wrappers saw, over the cases run in this session, against stream_cases.COVERED:
    every case named for an entry point called it."""
    ran = [n for n in set(launch_cases.CASES) | set(stream_cases.CASES) if n in SC.OBSERVED]
    assert ran, "no stream case ran in this session"
    missing = {(e, c) for e, cases in stream_cases.COVERED.items() for c in cases
               if c in SC.OBSERVED and e not in SC.OBSERVED[c]}
    assert not missing, f"declared but not called: {sorted(missing)}"
