"""Training-mode dropout without a GPU: the numpy Philox4x32-10 and keep-mask restatement
(tests/dropoutref.py) against known answers and its own invariants, and the chain restatement with those
masks against the goldens of the real reference (tools/make_goldens_dropout.py), which pin where the
reference applies dropout.

Gates: the float32 chain is the same torch CPU arithmetic as the generator's, so it is compared bitwise
where the GEMM order agrees and within 1e-6 rel-L2 otherwise (asserted: <= 1e-6); float64 within 1e-12.
"""
import numpy as np
import pytest
import torch

import dropoutref as D
from golden_util import load, params, rel_l2

CASES = ["drop_mlp_relu_ln", "drop_mlp_gelu", "drop_mlp_nh0"]


def _hex(words):
    return " ".join(f"{int(w):08x}" for w in words)


@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(ctr, key, want):
    assert _hex(D.philox4x32_10(np.array(ctr, dtype=np.uint64), key)) == want
    # a batch of counters gives the same block in every row
    batch = D.philox4x32_10(np.array([ctr, (1, 2, 3, 4), ctr], dtype=np.uint64), key)
    assert _hex(batch[0]) == want and _hex(batch[2]) == want and _hex(batch[1]) != want


def test_mask_is_word_e_and_3_of_block_e_shr_2():
    seed, offset, p = 0x0123456789ABCDEF, 4 * 77, 0.25
    m = D.keep_mask(seed, offset, 11, p)
    for e in range(11):
        c = offset // 4 + (e >> 2)
        w = D.philox4x32_10(np.array([c & D.LO, c >> 32, 0, 0], dtype=np.uint64), (seed & D.LO, seed >> 32))
        assert bool(m[e]) == (int(w[e & 3]) >= D.threshold(p))


def test_counter_carries_across_2_pow_32():
    """offset = 4 (2^32 - 2), n = 32: blocks 2^32 - 2 .. 2^32 + 5, the counter's second word goes 0 -> 1."""
    seed, p = 99, 0.5
    offset = 4 * (2 ** 32 - 2)
    m = D.keep_mask(seed, offset, 32, p)
    for b in range(8):
        c = 2 ** 32 - 2 + b
        ctr = np.array([c & D.LO, c >> 32, 0, 0], dtype=np.uint64)
        assert int(ctr[1]) == (0 if b < 2 else 1)
        w = D.philox4x32_10(ctr, (seed, 0))
        assert [bool(v) for v in m[4 * b:4 * b + 4]] == [int(v) >= D.threshold(p) for v in w]
    # the carry matters: without it blocks 2.. would repeat the counters 0.. of the low word
    wrong = D.keep_mask(seed, 0, 24, p)
    assert not np.array_equal(m[8:], wrong)


def test_edge_probabilities_and_threshold():
    assert D.threshold(0.0) == 0 and D.threshold(0.5) == 2 ** 31 and D.threshold(1.0) == 2 ** 32 - 1
    assert D.keep_mask(7, 0, 1000, 0.0).all()
    assert not D.keep_mask(7, 0, 1000, 1.0).any()


def test_mask_does_not_depend_on_the_split_into_calls():
    seed, offset, p, n = 1234, 4 * 10, 0.25, 4 * 61 + 3
    whole = D.keep_mask(seed, offset, n, p)
    for cut in (4, 8, 100, 4 * 60):
        a = D.keep_mask(seed, offset, cut, p)
        b = D.keep_mask(seed, offset + D.advance(cut), n - cut, p)
        assert np.array_equal(np.concatenate([a, b]), whole)
    s = D.MaskStream(seed, offset, p)
    parts = [s.next((3, 4)), s.next((4 * 61 + 3 - 12,))]
    assert np.array_equal(np.concatenate([t.reshape(-1).numpy() for t in parts]), whole)
    assert s.offset == offset + D.advance(12) + D.advance(n - 12)


def test_bits_round_trip():
    m = D.keep_mask(5, 0, 29, 0.5)
    b = D.pack_bits(m)
    assert b.dtype == np.uint8 and b.size == 4
    for e in range(29):
        assert bool((b[e >> 3] >> (e & 7)) & 1) == bool(m[e])
    assert np.array_equal(D.unpack_bits(b, 29), m)


def test_keep_fraction_of_the_gpu_test_s_seed():
    """The seed of tests/test_gpu_dropout.py's keep-fraction test meets the 4 sigma bound it asserts."""
    n, p = 129 * 32, 0.25
    kept = int(D.keep_mask(1234, 0, n, p).sum())
    sigma = (n * p * (1 - p)) ** 0.5
    assert abs(kept - n * (1 - p)) <= 4 * sigma
    assert abs(kept / n - 0.7602) < 5e-5


def _masks(d, meta, act_shapes):
    s = D.MaskStream(meta["seed"], meta["offset"], meta["p"])
    return [s.next(sh) if sh is not None else None for sh in act_shapes]


@pytest.mark.parametrize("name", CASES)
def test_chain_restatement_matches_the_reference(name):
    d, meta = load(name)
    d64, _ = load(name + "_f64")
    shapes = D.mask_shapes(meta)
    assert sum(s is not None for s in shapes) == meta["dropout_calls"]
    act = meta["kwargs"].get("activation_fn", "relu")
    for dtype, ref, tol in ((torch.float32, d, 1e-6), (torch.float64, d64, 1e-12)):
        y, gx, gp = D.chain(params(d), d["x"], _masks(d, meta, shapes), meta["p"], act=act, dtype=dtype)
        errs = {"y": rel_l2(y, ref["y"]), "gx": rel_l2(gx, ref["gx"])}
        for k, g in gp.items():
            errs["gp:" + k] = rel_l2(g, ref["gp:" + k])
        worst = max(errs, key=errs.get)
        bitwise = all(torch.equal(a, b) for a, b in [(y, ref["y"]), (gx, ref["gx"])] +
                      [(g, ref["gp:" + k]) for k, g in gp.items()])
        print(f"{name} {dtype}: bitwise {bitwise}, worst rel-L2 {errs[worst]:.3e} ({worst}; gate {tol:.0e})")
        assert errs[worst] <= tol, (worst, errs[worst])


def test_single_linear_has_no_dropout():
    d, meta = load("drop_mlp_nh0")
    assert meta["dropout_calls"] == 0 and D.mask_shapes(meta) == []
    y = D.chain(params(d), d["x"], [], 0.0, dtype=torch.float32, grad=False)
    assert rel_l2(y, d["y"]) <= 1e-6


def test_masks_are_needed():
    """The goldens do depend on the masks: the chain with all-ones masks (and the same scale) is far off."""
    d, meta = load("drop_mlp_relu_ln")
    ones = [torch.ones(s, dtype=torch.bool) for s in D.mask_shapes(meta)]
    y = D.chain(params(d), d["x"], ones, meta["p"], dtype=torch.float32, grad=False)
    assert rel_l2(y, d["y"]) > 1e-2
