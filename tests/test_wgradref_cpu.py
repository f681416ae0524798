"""tests/wgradref.py checked without a GPU: the tiled encoder against the decoder the other tests use,
the exactness of the integer inputs of tests/test_gpu_wgrad.py, the order emulations against float64,
and the evidence that the GPU tests would fail on a subtly wrong kernel: a CPU stand-in of agn_wgrad
with each of the mistakes wgradref.BUGS names is rejected by the same comparison functions the GPU
tests call, and the stand-in without a mistake passes them. Also WGrad.add's operand checks (it
launches nothing, so CPU tensors do)."""
import pytest
import torch

import wgradref as R
from maskmatched import decode_tiled

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ["fp32", "bf16", "fp16"]
MAX_ROWS = 1000  # the largest row count of tests/test_gpu_wgrad.py


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_encode_tiled_inverts_decode_tiled(dtype):
    for rows in (1, 31, 32, 33, 65, 97):
        x = torch.randn(rows, 128, generator=torch.Generator().manual_seed(rows)).to(dtype)
        t = R.encode_tiled(x, fill=R.NAN)
        assert t.shape == ((rows + 31) // 32 * 32, 128) and t.dtype == dtype and t.agn_tiled and t.agn_rows == rows
        assert torch.equal(decode_tiled(t, rows), x)
        # the pad rows, and only they, hold the fill
        full = decode_tiled(t, t.shape[0])
        assert bool(torch.isnan(full[rows:]).all()) and int(torch.isnan(full).sum()) == (t.shape[0] - rows) * 128
        # the documented address of a unit: (row r, i, half h) at 16-B index ((r / 32) U + i) 64 + r % 32 + 32 h
        per = 16 // x.element_size()
        U = 64 * x.element_size() // 16
        units = t.reshape(-1, per)
        for r, i, h in ((0, 0, 0), (rows - 1, U - 1, 1), (rows // 2, U // 2, 0)):
            u = units[((r // 32) * U + i) * 64 + r % 32 + 32 * h]
            if dtype == torch.float32:
                want = x[r, 8 * i + 4 * h:8 * i + 4 * h + 4]
            else:
                want = torch.cat([x[r, 16 * i + 4 * h:16 * i + 4 * h + 4], x[r, 16 * i + 8 + 4 * h:16 * i + 12 + 4 * h]])
            assert torch.equal(u, want)


def test_layout_helpers():
    x = R.int_operand(5, 7, 0)
    s = R.strided(x, 3, 1)
    assert torch.equal(s, x) and s.stride() == (11, 1) and s.storage_offset() == 1
    whole = torch.as_strided(s, (5, 11), (11, 1), 0)
    assert int(torch.isnan(whole).sum()) == 5 * 4
    buf, view = R.window(4, 3, 12, 6)
    assert view.shape == (4, 3) and view.stride() == (12, 1) and R.outside_untouched(buf) and R.all_sentinel(buf)
    view.zero_()
    assert R.outside_untouched(buf) and not R.all_sentinel(buf)
    for r, c in ((0, 6), (5, 8), (1, 5), (4, 9), (2, 0)):  # the rows above and below, the columns either side
        b2, _ = R.window(4, 3, 12, 6)
        b2[r, c] = 0.0
        assert not R.outside_untouched(b2)
    vb, vv = R.vec_window(4)
    vv.zero_()
    assert R.outside_untouched(vb)
    vb[2] = 1.0
    assert not R.outside_untouched(vb)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_integer_inputs_are_exact(dtype):
    """The operands survive the storage type, max |G^T X| < 2^24 at the largest row count used, and a
    float32 matmul (any order the BLAS picks) equals the int64 reference."""
    G, X = R.int_operand(MAX_ROWS, 128, 1), R.int_operand(MAX_ROWS, 200, 2)
    assert torch.equal(G.to(dtype).float(), G) and torch.equal(X.to(dtype).float(), X)
    assert int(G.min()) == -7 and int(G.max()) == 7
    assert 49 * MAX_ROWS < 2 ** 24
    refw, refb = R.exact_ref(G.to(dtype), X.to(dtype))
    assert int(refw.abs().max()) < 2 ** 24 and refw.dtype == torch.int64
    assert torch.equal((G.t() @ X).long(), refw) and torch.equal(G.sum(0).long(), refb)
    assert torch.equal((G.flip(0).t() @ X.flip(0)).long(), refw)  # another order
    idx = torch.randint(0, MAX_ROWS, (333,), generator=torch.Generator().manual_seed(3), dtype=torch.int32)
    rw, _ = R.exact_ref(G[:333], X, idx)
    assert torch.equal((G[:333].t() @ X[idx.long()]).long(), rw)


def _emulated(rows, M, K, bug, ldw_off=(9, 6)):
    G, X = R.int_operand(rows, M, 10 + rows), R.int_operand(rows, K, 20 + rows)
    dwb, dw = R.window(M, K, K + ldw_off[0], ldw_off[1])
    dbb, db = R.vec_window(M)
    R.emulate_wgrad(G, X, dw, db, bug=bug)
    refw, refb = R.exact_ref(G, X)
    return R.case_failures(f"{bug}", dw, refw, db, refb, dwb, dbb)


@pytest.mark.parametrize("rows,M,K", [(97, 128, 128), (65, 100, 100), (333, 200, 260)])
def test_unbugged_emulation_passes(rows, M, K):
    assert _emulated(rows, M, K, None) == []


@pytest.mark.parametrize("bug", R.BUGS)
@pytest.mark.parametrize("rows,M,K", [(97, 128, 128), (65, 100, 100), (333, 200, 260)])
def test_every_injected_bug_is_rejected(bug, rows, M, K):
    f = _emulated(rows, M, K, bug)
    assert f, f"{bug} at rows {rows}, ({M}, {K}) passed the exact comparison"


def test_pad_leak_of_a_finite_value_is_rejected_too():
    G, X = R.int_operand(33, 128, 1), R.int_operand(33, 128, 2)
    _, dw = R.window(128, 128, 128, 0)
    R.emulate_wgrad(G, X, dw, bug="leak_pad_row", pad_fill=1.0)
    assert R.exact_failures("dW", dw, R.exact_ref(G, X)[0])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_rounded_mode_rejects_a_low_precision_accumulation(dtype):
    """The bound passes an fp32 accumulation in two different orders and rejects a running sum that
    is kept in bf16 between the 64-row stages."""
    gen = torch.Generator().manual_seed(5)
    rows = 333
    G, X = torch.randn(rows, 128, generator=gen).to(dtype), torch.randn(rows, 128, generator=gen).to(dtype)
    ref, _, bound = R.bound_ref(G, X, rows, 3)
    dw = torch.empty(128, 128)
    R.emulate_wgrad(G, X, dw)
    f, ratio = R.rounded_failures("fp32", dw, ref, bound)
    assert f == [] and ratio <= 1.0
    seq = torch.zeros(128, 128)
    for r in range(rows):  # one row at a time: the longest dependent chain
        seq += torch.outer(G[r].float(), X[r].float())
    f, ratio = R.rounded_failures("sequential", seq, ref, bound)
    assert f == [] and ratio <= 1.0
    R.emulate_wgrad(G, X, dw, bug="lowprec")
    f, ratio = R.rounded_failures("lowprec", dw, ref, bound)
    assert f and ratio > 1.0


def test_order_emulations_agree_with_float64():
    """Sanity of reduce_order / colsum_order / partials_order: within fp32 accumulation error of the
    float64 sum, |err| <= n 2^-24 sum |p|."""
    gen = torch.Generator().manual_seed(0)
    for n in (1, 7, 8, 9, 33, 100):
        p = torch.randn(n, 6, 5, generator=gen)
        lim = n * 2.0 ** -24 * p.double().abs().sum(0)
        assert bool(((R.reduce_order(p).double() - p.double().sum(0)).abs() <= lim).all())
        assert bool(((R.partials_order(p).double() - p.double().sum(0)).abs() <= lim).all())
    assert torch.equal(R.reduce_order(torch.ones(40, 3)), torch.full((3,), 40.0))
    for nw, n, sr in ((1, 1, 1), (9, 65, 9), (513, 7, 512), (2049, 13, 512), (5, 3, 2)):
        p = torch.randn(nw, n, generator=gen)
        lim = nw * 2.0 ** -24 * p.double().abs().sum(0)
        assert bool(((R.colsum_order(p, sr).double() - p.double().sum(0)).abs() <= lim).all())
    assert torch.equal(R.colsum_order(torch.empty(0, 4), 1), torch.zeros(4))
    # the order is a different one from the plain sequential sum (else the bitwise GPU test pins nothing)
    p = torch.randn(33, 4096, generator=gen)
    assert not torch.equal(R.reduce_order(p), R.partials_order(p))


def test_wgrad_add_refuses_a_column_strided_operand():
    """WGrad.add hands stride(0) to the kernel as the leading dimension; a transposed view would be
    read silently wrong, so it is refused like a bad dw."""
    from aerognn.core import WGrad
    G, X = torch.zeros(8, 4), torch.zeros(8, 6)
    dw, db = torch.zeros(4, 6), torch.zeros(4)
    wg = WGrad()
    wg.add(G, X, dw, db)
    wg.add(G, torch.zeros(8, 12)[:, 3:9], dw)  # a column window is fine
    assert len(wg.items) == 2
    with pytest.raises(AssertionError):
        wg.add(torch.zeros(4, 8).t(), X, dw, db)
    with pytest.raises(AssertionError):
        wg.add(G, torch.zeros(6, 8).t(), dw, db)
    with pytest.raises(AssertionError):
        wg.add(G, torch.zeros(8, 12)[:, ::2], dw, db)
    with pytest.raises(AssertionError):
        wg.add(G, X, torch.zeros(6, 4).t(), db)
    assert len(wg.items) == 2
