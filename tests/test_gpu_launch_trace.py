"""The launch sequence of every autograd.Function mode (aerognn/functions.py): which kernels run, in
which order, under which tag and with which cost tuple, for one forward and one backward of each case
of launch_cases.CASES, against tests/golden/launch_traces.json (tools/record_launch_traces.py).

The host layer only decides which kernel runs; a change there that keeps behaviour keeps every trace.
Costs are functions of the shapes alone, so they compare exactly (tuples and lists alike after JSON).
"""
import json
import os

import pytest
import torch

import launch_cases

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_traces.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_covers_the_case_table(golden):
    assert sorted(golden) == sorted(launch_cases.CASES)


@pytest.mark.parametrize("kernel", ["fourier", "act_dropout"])
def test_function_and_operator_agree(kernel, monkeypatch):
    """The autograd Function and the registered operator of one kernel: the same launches and the same bits."""
    (tf, xf), (to, xo) = (launch_cases.run_case(f"{kernel}_{via}", monkeypatch.setenv) for via in ("fn", "op"))
    assert tf and tf == to
    assert sorted(xf) == sorted(xo)
    for k in xf:
        assert torch.equal(xf[k], xo[k]), k


@pytest.mark.parametrize("name", list(launch_cases.CASES))
def test_launch_trace(name, golden, monkeypatch):
    trace, tensors = launch_cases.run_case(name, monkeypatch.setenv)
    assert trace, name
    assert all(t is not None for t in tensors.values())
    # (through JSON, as the golden file went: tuples become lists, the numbers stay what they are)
    assert json.loads(json.dumps(trace)) == golden[name], name
