"""Completeness of the stream cases (tests/test_gpu_streams.py), checked without a GPU: every entry
point of include/aerognn.h that takes a stream has a case that must call it, every case named exists, and
the poison the cases' inputs are overwritten with is the safe one."""
import pytest
import torch

import launch_cases
import stream_cases
import streamcheck as SC


def test_stream_entries_are_read_from_the_header():
    from aerognn import _lib as L
    entries = SC.stream_entries()
    assert len(entries) == len(set(entries)) and set(entries) <= set(L.PROTOS)
    assert {"agn_mlp_forward", "agn_fault_status_async", "agn_f64_gemm", "agn_radix_sort_u64"} <= set(entries)
    # the stream is the last parameter and a pointer; entry points without one are not listed
    assert all(L.PROTOS[e][1][-1] is L.vp for e in entries)
    assert not {"agn_fault_status", "agn_debug_set_fault", "agn_wgrad_plan", "agn_version"} & set(entries)
    # every launcher that core.PROF times takes a stream
    assert set(L.LAUNCHES) <= set(entries)


def test_every_stream_entry_point_has_a_case():
    assert set(stream_cases.COVERED) == set(SC.stream_entries())
    assert all(cases for cases in stream_cases.COVERED.values())


def test_every_covering_case_exists():
    assert not set(launch_cases.CASES) & set(stream_cases.CASES)
    known = set(launch_cases.CASES) | set(stream_cases.CASES)
    named = {c for cases in stream_cases.COVERED.values() for c in cases}
    assert named <= known, sorted(named - known)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32, torch.bfloat16, torch.float16, torch.int32, torch.int64])
def test_poison(dtype):
    """Floats become NaN, integers 0; shape, dtype and strides stay, and so does what lies between the
    elements of a strided tensor."""
    base = torch.arange(1, 41).reshape(5, 8).to(dtype)
    view = base[1:4, ::2]
    shape, strides = view.shape, view.stride()
    out = SC.poison_(view)
    assert out is view and view.shape == shape and view.stride() == strides and view.dtype == dtype
    if dtype.is_floating_point:
        assert torch.isnan(view).all()
    else:
        assert (view == 0).all()
    keep = torch.ones(5, 8, dtype=torch.bool)
    keep[1:4, ::2] = False
    assert torch.equal(base[keep], torch.arange(1, 41).reshape(5, 8).to(dtype)[keep])
    leaf = torch.ones(3, dtype=dtype, requires_grad=dtype.is_floating_point)
    SC.poison_(leaf)  # a leaf that requires a gradient is filled in place all the same
    assert leaf.requires_grad == dtype.is_floating_point


@pytest.mark.parametrize("dtype", [torch.uint8, torch.bool, torch.int8])
def test_poison_refuses_bytes(dtype):
    """Byte buffers hold packed weights and descriptor tables with addresses: no value is safe there."""
    with pytest.raises(TypeError):
        SC.poison_(torch.zeros(4, dtype=dtype))


def test_bits_tell_nan_payloads_and_signed_zeros_apart():
    a = torch.tensor([0.0, float("nan")])
    b = torch.tensor([-0.0, float("nan")])
    assert SC.same_bits(SC.bits(a), SC.bits(a.clone()))
    assert not SC.same_bits(SC.bits(a), SC.bits(b))
    c = a.clone()
    c.view(torch.int32)[1] += 1  # another NaN
    assert torch.isnan(c[1]) and not SC.same_bits(SC.bits(a), SC.bits(c))
    assert SC.differing({"x": SC.bits(a)}, {"x": SC.bits(a), "y": SC.bits(b)}) == ["y"]
    assert not SC.same_bits(SC.bits(a), SC.bits(a.double()))


def test_reachable_tensors_skip_bytes_and_the_host():
    """The inputs of a launch case are found through its closure; CPU tensors and byte buffers stay out.
    (On the CPU nothing is on the device: the walk itself is what runs here.)"""
    import types
    lv = types.SimpleNamespace(src=torch.zeros(3, dtype=torch.int32), table=torch.zeros(3, dtype=torch.uint8))
    m = torch.nn.Linear(2, 2)

    def fwd():
        return m, lv
    assert SC.reachable_tensors(fwd) == {}
