"""Gradients of 16-bit parameters: every autograd.Function forms its parameter gradients in fp32 and
rounds each once to the parameter's dtype (aerognn/functions.py, _to_param_dtypes).

The reference is the same step with fp32 parameters that hold the bf16 module's values (bf16 -> fp32 is
exact, and the packed bf16 weights and fp32 bias / LayerNorm vectors come out the same), so its fp32
gradients are the numbers the bf16 module rounds: the comparison is bitwise, outputs included. A
gradient cast before the launch that fills its fp32 buffer has run (the sum-trick layer's node chain
once did that: its dW products go out with the projection's in one later agn_wgrad launch) fails it.
"""
import pytest
import torch

import launch_cases

pytestmark = pytest.mark.gpu
CASES = ["gmp_bf16_h128_sum", "gmp_bf16_h128_cat", "L_gmp_train_bf16_params", "L_v2_train_bf16_params",
         "L_mlp_encoder_rows_bf16_params"]


@pytest.mark.parametrize("name", CASES)
def test_bf16_parameter_grads_are_the_fp32_grads_rounded_once(name):
    builder, kw, env = launch_cases.CASES[name]
    assert not env and kw["pdt"] == torch.bfloat16
    got = launch_cases.step(*builder(**kw))
    fwd, leaves = builder(**{**kw, "pdt": torch.float32})
    for t in leaves.values():
        t.data.copy_(t.data.bfloat16())
    want = launch_cases.step(fwd, leaves)
    assert got.keys() == want.keys() and any(k.startswith("d ") and want[k].dtype == torch.float32 for k in want)
    for k, w in want.items():
        assert got[k].dtype == torch.bfloat16
        assert torch.equal(got[k].view(torch.int16), w.bfloat16().view(torch.int16)), (name, k)
