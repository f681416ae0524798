"""The weight-gradient kernels of csrc/dw.hip (agn_wgrad, agn_wgrad_reduce, agn_colsum) and
agn_reduce_partials of csrc/mlp.hip at every operand layout, split count and batch shape
(tests/wgradref.py has the method).

Exact mode (every layout, indexing, tail, split and batch case): integer operands in [-7, 7], so dW
and db are the int64 reference in any summation order and are compared with torch.equal, no
tolerance; everything the kernel must not read holds NaN and everything it must not write a sentinel
bit pattern. Rounded mode (one randn case per dtype): the elementwise fp32 accumulation bound, which
catches an accumulation in less than fp32. The reductions are compared bitwise with fp32 CPU
emulations of their documented orders. Shapes are the smallest that reach each branch: the kernel
stages 64 rows, a tile is 32 rows, an output block is 128 x 128."""
import ctypes as C
import functools
import os

import pytest
import torch

from aerognn import _lib

import wgradref as R

pytestmark = pytest.mark.gpu
os.environ.setdefault("AEROGNN_MEMLOG", "0")
DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ["fp32", "bf16", "fp16"]
ROWS = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 200, 333]
MK = [(1, 1), (4, 128), (128, 4), (128, 6), (7, 12), (100, 100), (128, 129), (129, 128), (128, 256), (256, 128),
      (200, 260), (260, 6)]
E_ARG, E_DTYPE, E_SHAPE = _lib.E_ARG, _lib.E_DTYPE, _lib.E_SHAPE  # AGN_E_* of include/aerognn.h


# --------------------------------------------------------------------------- shared inputs (never modified)
@functools.lru_cache(maxsize=None)
def _g(rows, M):
    return R.int_operand(rows, M, 7 * rows + M)


@functools.lru_cache(maxsize=None)
def _x(rows, K):
    return R.int_operand(rows, K, 100003 + 11 * rows + K)


@functools.lru_cache(maxsize=None)
def _table(rows, K):
    """(table [rows + 5, K], xidx [rows] int32 with repeated indices); the rows xidx never names are NaN."""
    gen = torch.Generator().manual_seed(5 * rows + K)
    tab = R.int_operand(rows + 5, K, 200003 + 13 * rows + K)
    idx = torch.randint(0, rows + 5, (rows,), generator=gen, dtype=torch.int32)
    if rows > 1:
        idx[rows - 1] = idx[0]
    named = torch.zeros(rows + 5, dtype=torch.bool)
    named[idx.long()] = True
    assert int((~named).sum()) >= 5
    tab[~named] = R.NAN
    return tab, idx


@functools.lru_cache(maxsize=None)
def _ref(rows, M, K, gathered=False):
    if gathered:
        tab, idx = _table(rows, K)
        return R.exact_ref(_g(rows, M), torch.nan_to_num(tab), idx)
    return R.exact_ref(_g(rows, M), _x(rows, K))


def _layouts(x, dtype, tiled):
    xd = x.to(DEV, dtype)
    out = {"contiguous": xd, "pad3_off1": R.strided(xd, 3, 1), "pad8_off4": R.strided(xd, 8, 4),
           "pad8_off0": R.strided(xd, 8, 0)}
    if tiled:
        out["tiled"] = R.encode_tiled(xd)
    return out


class _Case:
    """One desc with its sentinel-framed outputs and its reference."""

    def __init__(self, name, G, X, ref, win=None, db=True, xidx=None):
        M, K = G.shape[1], X.shape[1]
        ldw, off = win if win is not None else (K, 0)
        self.name, self.ref = name, ref
        self.dwb, self.dw = R.window(M, K, ldw, off, device=DEV)
        self.dbb, self.db = R.vec_window(M, device=DEV) if db else (None, None)
        self.desc = R.Desc(G, X, self.dw, self.db, xidx)

    def failures(self):
        return R.case_failures(self.name, self.dw, self.ref[0], self.db, self.ref[1], self.dwb, self.dbb)


def _run(cases, dtype, nsplit, plan=False):
    """One agn_wgrad launch over up to 8 cases; the exact-mode failures of all of them."""
    assert 1 <= len(cases) <= 8
    rc, b, slabs = R.launch([c.desc for c in cases], dtype, nsplit, plan=plan)
    assert rc == 0, f"agn_wgrad returned {rc}"
    f = [m for c in cases for m in c.failures()]
    del slabs
    return f, b


# --------------------------------------------------------------------------- operand layouts
@pytest.mark.parametrize("nsplit", [1, 3])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_operand_layouts(dtype, nsplit):
    """M = K = 128: G in five layouts against X in the same five plus gathered, at every row count."""
    fails, n = [], 0
    for rows in ROWS:
        Gs = _layouts(_g(rows, 128), dtype, True)
        Xs = [(k, v, None, False) for k, v in _layouts(_x(rows, 128), dtype, True).items()]
        tab, idx = _table(rows, 128)
        tabd, idxd = tab.to(DEV, dtype), idx.to(DEV)
        Xs.append(("gathered", tabd, idxd, True))
        if dtype == torch.bfloat16:
            Xs.append(("gathered_pad3_off1", R.strided(tabd, 3, 1), idxd, True))
        for xname, X, xi, gath in Xs:
            for db in ((True, False) if rows == 65 else (True,)):
                cases = [_Case(f"rows {rows} G {gname} X {xname} db {db}", G, X, _ref(rows, 128, 128, gath), db=db, xidx=xi)
                         for gname, G in Gs.items()]
                fails += _run(cases, dtype, nsplit)[0]
                n += len(cases)
    assert n == (len(ROWS) + 1) * 5 * (7 if dtype == torch.bfloat16 else 6)  # nothing skipped
    assert not fails, "\n".join(fails[:20])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_row_major_operand_wider_than_a_block(dtype):
    """129 columns at row stride 136: the block at c0 = 0 has cols - c0 >= 128 (aligned 16-B rows), the
    block at c0 = 128 has one live column."""
    fails = []
    for rows in ROWS:
        g129, x129 = _g(rows, 129).to(DEV, dtype), _x(rows, 129).to(DEV, dtype)
        G, X = _g(rows, 128).to(DEV, dtype), _x(rows, 128).to(DEV, dtype)
        Gw, Xw = R.strided(g129, 7, 0), R.strided(x129, 7, 0)
        assert Gw.stride(0) == 136 and Xw.stride(0) == 136
        for nsplit in (1, 3):
            cases = [_Case(f"rows {rows} ns {nsplit} X wide", G, Xw, _ref(rows, 128, 129)),
                     _Case(f"rows {rows} ns {nsplit} G wide", Gw, X, _ref(rows, 129, 128)),
                     _Case(f"rows {rows} ns {nsplit} both wide", Gw, Xw, _ref(rows, 129, 129))]
            fails += _run(cases, dtype, nsplit)[0]
    assert not fails, "\n".join(fails[:20])


# --------------------------------------------------------------------------- shapes and dW windows
@pytest.mark.parametrize("nsplit", [1, 2])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_shapes_and_dw_windows(dtype, nsplit):
    """Every (M, K) at rows 1, 65, 200, contiguous and strided, dW written into four windows of a
    sentinel buffer (row strides K, K + 1, 2K + 1, K + 9; column offsets 0, K, 6), db inside a vector."""
    fails, n = [], 0
    for rows in (1, 65, 200):
        for M, K in MK:
            g, x = _g(rows, M).to(DEV, dtype), _x(rows, K).to(DEV, dtype)
            ops = {"contiguous": (g, x), "pad3_off1": (R.strided(g, 3, 1), R.strided(x, 3, 1))}
            cases = [_Case(f"rows {rows} ({M}, {K}) {lname} ldw {ldw} off {off}", G, X, _ref(rows, M, K), win=(ldw, off))
                     for lname, (G, X) in ops.items()
                     for ldw, off in ((K, 0), (K + 1, 0), (2 * K + 1, K), (K + 9, 6))]
            fails += _run(cases, dtype, nsplit)[0]
            n += len(cases)
    assert n == 3 * 12 * 8
    assert not fails, "\n".join(fails[:20])


# --------------------------------------------------------------------------- split counts
@pytest.mark.parametrize("rows,M,K", [(200, 128, 128), (1000, 128, 128), (1000, 256, 6)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_split_counts(dtype, rows, M, K):
    """Exact at every split count: around the 8 groups and the 4-in-flight loop of the reduction, and
    with trailing splits that own no rows."""
    G, X = _g(rows, M).to(DEV, dtype), _x(rows, K).to(DEV, dtype)
    fails = []
    for nsplit in (1, 2, 3, 7, 8, 9, 31, 32, 33, 40, (rows + 63) // 64 + 5):
        fails += _run([_Case(f"nsplit {nsplit}", G, X, _ref(rows, M, K))], dtype, nsplit)[0]
    assert not fails, "\n".join(fails[:20])


# --------------------------------------------------------------------------- mixed batches
def _mixed_cases(dtype):
    spec = [  # rows, (M, K), G layout, X layout, db
        (1, (4, 128), "contiguous", "tiled", True),
        (3, (128, 4), "tiled", "contiguous", False),
        (64, (128, 256), "tiled", "contiguous", True),
        (65, (7, 12), "pad3_off1", "pad3_off1", True),
        (700, (256, 128), "contiguous", "tiled", True),
        (700, (200, 260), "contiguous", "pad8_off4", False),
        (10, (128, 129), "pad8_off0", "contiguous", True),
        (333, (100, 100), "pad3_off1", "contiguous", False)]
    cases = []
    for rows, (M, K), gl, xl, db in spec:
        G = _layouts(_g(rows, M), dtype, M == 128)[gl]
        X = _layouts(_x(rows, K), dtype, K == 128)[xl]
        cases.append(_Case(f"rows {rows} ({M}, {K}) G {gl} X {xl}", G, X, _ref(rows, M, K), win=(K + 9, 6), db=db))
    return cases


@pytest.mark.parametrize("planned", [False, True], ids=["nsplit6", "planned"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_mixed_batch(dtype, planned):
    """Eight descs of very different row counts share one split count: the small ones run with most
    of their splits empty (as poolMGN's global encoder does next to its node-sized descs)."""
    cases = _mixed_cases(dtype)
    fails, b = _run(cases, dtype, 0 if planned else 6, plan=planned)
    if planned:
        ns = [b.d[j].nsplit for j in range(8)]
        assert len(set(ns)) == 1 and 1 <= ns[0] <= (700 + 127) // 128, ns
    assert not fails, "\n".join(fails[:20])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gathered_and_plain_descs_in_one_launch(dtype):
    """The gathered instantiation also serves descs without xidx (WGrad.run never builds this)."""
    def gath(rows, M, K):
        tab, idx = _table(rows, K)
        return _Case(f"gathered rows {rows} ({M}, {K})", _g(rows, M).to(DEV, dtype), tab.to(DEV, dtype),
                     _ref(rows, M, K, True), xidx=idx.to(DEV))
    for nsplit in (1, 2):
        cases = [_Case("plain rows 200", _g(200, 128).to(DEV, dtype), _x(200, 128).to(DEV, dtype), _ref(200, 128, 128)),
                 gath(65, 128, 6),
                 _Case("tiled rows 33", R.encode_tiled(_g(33, 128).to(DEV, dtype)), R.encode_tiled(_x(33, 128).to(DEV, dtype)),
                       _ref(33, 128, 128)),
                 gath(129, 100, 100)]
        fails, _ = _run(cases, dtype, nsplit)
        assert not fails, "\n".join(fails[:20])


def test_plan_properties():
    """agn_wgrad_plan returns 0, gives every desc the same split count, 1 <= nsplit <= ceil(max rows / 128)."""
    from aerognn import _lib as L
    lib = L.lib()
    for shapes in ([(1, 1, 1)], [(127, 128, 128)], [(129, 128, 128)], [(1, 4, 128), (700, 256, 128), (10, 128, 129)],
                   [(100000, 128, 128)] * 8, [(5000000, 256, 256), (3, 7, 12)], [(0, 128, 128), (64, 128, 128)]):
        b = L.WgradBatch()
        b.n = len(shapes)
        for j, (rows, m, k) in enumerate(shapes):
            b.d[j].rows, b.d[j].m, b.d[j].k = rows, m, k
        assert lib.agn_wgrad_plan(C.byref(b)) == 0
        ns = [b.d[j].nsplit for j in range(b.n)]
        top = max(1, (max(s[0] for s in shapes) + 127) // 128)
        assert len(set(ns)) == 1 and 1 <= ns[0] <= top, (shapes, ns)
    for n in (0, 9):
        b = L.WgradBatch()
        b.n = n
        assert lib.agn_wgrad_plan(C.byref(b)) == E_ARG


# --------------------------------------------------------------------------- WGrad.run host logic
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_wgrad_run_host_logic(dtype):
    """11 items in one WGrad (more than MAX_WGRAD): two with 0 rows, three gathered, two tiled, one dW
    shared by two column-slice items; every result exact, zero-row outputs zeroed from NaN."""
    from aerognn.core import WGrad

    def d(t):
        return t.to(DEV, dtype)

    def gath(rows, M, K, db, strided=False):
        tab, idx = _table(rows, K)
        T = R.strided(d(tab), 3, 1) if strided else d(tab)
        return _Case(f"gathered rows {rows} ({M}, {K})", d(_g(rows, M)), T, _ref(rows, M, K, True), win=(K + 1, 0), db=db,
                     xidx=idx.to(DEV))

    zero = (torch.zeros(128, 6, dtype=torch.int64), torch.zeros(128, dtype=torch.int64))
    cases = [
        _Case("rows 200", d(_g(200, 128)), d(_x(200, 128)), _ref(200, 128, 128), win=(137, 6)),
        _Case("rows 0", d(_g(0, 128)), d(_x(0, 6)), zero, win=(15, 6)),
        _Case("rows 65 tiled G, X", R.encode_tiled(d(_g(65, 128))), R.encode_tiled(d(_x(65, 128))), _ref(65, 128, 128)),
        _Case("rows 33 tiled X", d(_g(33, 7)), R.encode_tiled(d(_x(33, 128))), _ref(33, 7, 128), db=False),
        _Case("rows 1000 strided G", R.strided(d(_g(1000, 256)), 3, 1), d(_x(1000, 128)), _ref(1000, 256, 128)),
        _Case("rows 1", d(_g(1, 1)), d(_x(1, 1)), _ref(1, 1, 1)),
        gath(333, 128, 12, True),
        gath(64, 128, 128, False, strided=True),
        _Case("gathered rows 0", d(_g(0, 128)), d(_x(9, 6)), zero, win=(15, 6), xidx=torch.empty(0, dtype=torch.int32, device=DEV)),
    ]
    # one dW [100][134] shared by two column-slice items, as _chain_param_grads splits a concatenated input
    Gs, X1, X2 = d(_g(129, 100)), d(_x(129, 128)), d(_x(129, 6))
    sb, sv = R.window(100, 134, 140, 3, device=DEV)
    sdbb, sdb = R.vec_window(100, device=DEV)
    wg = WGrad()
    for c in cases[:4]:
        wg.add(c.desc.G, c.desc.X, c.dw, c.db, xidx=c.desc.xidx)
    wg.add(Gs, X1, sv[:, :128], sdb)
    wg.add(Gs, X2, sv[:, 128:])
    for c in cases[4:]:
        wg.add(c.desc.G, c.desc.X, c.dw, c.db, xidx=c.desc.xidx)
    assert len(wg.items) == 11 and sum(it[4] is not None for it in wg.items) == 3
    wg.run()
    assert wg.items == []
    fails = [m for c in cases for m in c.failures()]
    refs = torch.cat([R.exact_ref(_g(129, 100), _x(129, 128))[0], R.exact_ref(_g(129, 100), _x(129, 6))[0]], 1)
    fails += R.case_failures("shared dW", sv, refs, sdb, _g(129, 100).long().sum(0), sb, sdbb)
    assert not fails, "\n".join(fails[:20])


def test_wgrad_run_chunks_a_long_plain_group():
    """Nine plain items: two launches (8 + 1)."""
    from aerognn.core import WGrad
    shapes = [(r, M, K) for r, (M, K) in zip((1, 31, 33, 64, 65, 129, 200, 333, 63), MK)]
    cases = [_Case(f"rows {r} ({M}, {K})", _g(r, M).to(DEV), _x(r, K).to(DEV), _ref(r, M, K), win=(K + 9, 6)) for r, M, K in shapes]
    wg = WGrad()
    for c in cases:
        wg.add(c.desc.G, c.desc.X, c.dw, c.db)
    wg.run()
    fails = [m for c in cases for m in c.failures()]
    assert wg.items == [] and not fails, "\n".join(fails[:20])


# --------------------------------------------------------------------------- rounded mode
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_rounded_accumulation_bound(dtype):
    """randn operands: |got - ref64| <= 2 (rows + nsplit + 16) 2^-24 |G|^T |X| elementwise and rel-L2 <= 1e-6.
    Measured worst ratio to the bound on an MI355X: see DESIGN.md §4."""
    fails, worst = [], 0.0
    for rows in (200, 333):
        gen = torch.Generator().manual_seed(rows)
        G, X = torch.randn(rows, 128, generator=gen).to(dtype), torch.randn(rows, 128, generator=gen).to(dtype)
        for nsplit in (1, 3):
            dwb, dw = R.window(128, 128, 128, 0, device=DEV)
            dbb, db = R.vec_window(128, device=DEV)
            rc, _, slabs = R.launch([R.Desc(G.to(DEV), X.to(DEV), dw, db)], dtype, nsplit)
            assert rc == 0
            ref, _, bound = R.bound_ref(G, X, rows, nsplit)
            f, ratio = R.rounded_failures(f"dW rows {rows} nsplit {nsplit}", dw, ref, bound)
            g64 = G.double()
            fb, rb = R.rounded_failures(f"db rows {rows} nsplit {nsplit}", db, g64.sum(0),
                                        2.0 * (rows + nsplit + 16) * 2.0 ** -24 * g64.abs().sum(0))
            print(f"wgrad rounded {dtype} rows {rows} nsplit {nsplit}: worst |err| / bound dW {ratio:.4f} db {rb:.4f}")
            fails += f + fb
            worst = max(worst, ratio, rb)
            assert R.outside_untouched(dwb) and R.outside_untouched(dbb)
    print(f"wgrad rounded {dtype}: worst ratio to the bound {worst:.4f}")
    assert not fails, "\n".join(fails)


# --------------------------------------------------------------------------- the reductions, bitwise
def _bits_equal(a, b):
    return torch.equal(a.detach().cpu().contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("nsplit", [1, 7, 8, 9, 31, 32, 33, 40, 100])
def test_wgrad_reduce_alone(nsplit):
    """agn_wgrad_reduce on slabs the test writes (as core._reduce_slabs feeds it): bitwise the documented order."""
    from aerognn import _lib as L
    from aerognn.core import stream
    lib = L.lib()
    gen = torch.Generator().manual_seed(nsplit)
    dwp, dbp = torch.randn(3, nsplit, 128, 128, generator=gen), torch.randn(3, nsplit, 128, generator=gen)
    dwpd, dbpd = dwp.to(DEV), dbp.to(DEV)
    outs = [(R.window(128, 128, 128, 0, device=DEV), R.vec_window(128, device=DEV)) for _ in range(3)]
    b = L.WgradBatch()
    b.n = 3
    for l, ((_, dw), (_, db)) in enumerate(outs):
        b.d[l] = L.WgradDesc(None, None, 128, 128, 128, 128, 1000, 128, L.ptr(dwpd[l]), L.ptr(dbpd[l]), L.ptr(dw), L.ptr(db),
                             0, 0, nsplit, 0)
    assert lib.agn_wgrad_reduce(C.byref(b), nsplit, stream()) == 0
    for l, ((dwb, dw), (dbb, db)) in enumerate(outs):
        assert _bits_equal(dw, R.reduce_order(dwp[l])), f"dW{l}"
        assert _bits_equal(db, R.reduce_order(dbp[l])), f"db{l}"
        assert R.outside_untouched(dwb) and R.outside_untouched(dbb)
    # one desc with m = 100, k = 6 inside a padded 128 x 128 slab; dW beyond [m][k] stays untouched
    (dwb, dw), (dbb, db) = R.window(100, 6, 15, 6, device=DEV), R.vec_window(100, device=DEV)
    b = L.WgradBatch()
    b.n = 1
    b.d[0] = L.WgradDesc(None, None, 100, 6, 100, 6, 1000, 15, L.ptr(dwpd[0]), L.ptr(dbpd[0]), L.ptr(dw), L.ptr(db), 0, 0, 0, 0)
    assert lib.agn_wgrad_reduce(C.byref(b), nsplit, stream()) == 0
    assert _bits_equal(dw, R.reduce_order(dwp[0])[:100, :6].contiguous())
    assert _bits_equal(db, R.reduce_order(dbp[0])[:100].contiguous())
    assert R.outside_untouched(dwb) and R.outside_untouched(dbb)


@pytest.mark.parametrize("nw,n", [(1, 1), (3, 5), (8, 64), (9, 65), (511, 7), (512, 256), (513, 257), (2049, 130)])
def test_colsum_order(nw, n):
    from aerognn.core import colsum_rows
    p = torch.randn(nw, n, generator=torch.Generator().manual_seed(nw + n))
    buf, out = R.vec_window(n, device=DEV)
    colsum_rows(p.to(DEV), nw, n, out)
    assert _bits_equal(out, R.colsum_order(p, min(512, max(1, nw))))
    assert R.outside_untouched(buf)


def test_colsum_of_no_rows_is_zero():
    from aerognn.core import colsum_rows
    buf, out = R.vec_window(7, device=DEV)
    colsum_rows(torch.empty(0, 7, device=DEV), 0, 7, out)
    assert torch.equal(out.cpu(), torch.zeros(7)) and R.outside_untouched(buf)


@pytest.mark.parametrize("n", [1, 255, 256, 257])
@pytest.mark.parametrize("nw", [1, 2, 17])
def test_reduce_partials_order(nw, n):
    from aerognn.core import reduce_partials
    p = torch.randn(nw, n, generator=torch.Generator().manual_seed(31 * nw + n))
    buf, out = R.vec_window(n, device=DEV)
    reduce_partials(p.to(DEV), nw, n, out)
    assert _bits_equal(out, R.partials_order(p))
    assert R.outside_untouched(buf)


# --------------------------------------------------------------------------- argument checks
def test_argument_checks():
    """Each bad call returns its code before any launch: the outputs keep the sentinel."""
    from aerognn import _lib as L
    from aerognn.core import stream
    dtype = torch.bfloat16
    G, X = _g(65, 128).to(DEV, dtype), _x(65, 128).to(DEV, dtype)
    G100, X100 = _g(65, 100).to(DEV, dtype), _x(65, 100).to(DEV, dtype)
    Xt = R.encode_tiled(X)
    idx = torch.zeros(65, dtype=torch.int32, device=DEV)

    def outs(M=128, K=128):
        return R.window(M, K, K, 0, device=DEV), R.vec_window(M, device=DEV)

    def call(want, build, dt=dtype, nsplit=1, n=None):
        made = [outs(*mk) for mk in build["mk"]]
        descs = [R.Desc(g, x, w[1], v[1], xi, **over) for (g, x, xi, over), (w, v) in zip(build["descs"], made)]
        rc, _, slabs = R.launch(descs, dt, nsplit, n=n)
        torch.cuda.synchronize()
        assert rc == want, (build["name"], rc)
        for w, v in made:
            assert R.all_sentinel(w[0]) and R.all_sentinel(v[0]), build["name"]

    def one(name, g=G, x=X, xi=None, mk=(128, 128), **over):
        return dict(name=name, mk=[mk], descs=[(g, x, xi, over)])

    call(E_ARG, one("b.n = 0"), n=0)
    call(E_ARG, dict(name="b.n = 9", mk=[(128, 128)] * 8, descs=[(G, X, None, {})] * 8), n=9)
    call(E_ARG, one("m = 0", m=0))
    call(E_ARG, one("k = 0", k=0))
    call(E_ARG, one("rows = -1", rows=-1))
    call(E_SHAPE, one("g_tiled with m = 100", g=G100, mk=(100, 128), g_tiled=1))
    call(E_SHAPE, one("x_tiled with k = 100", x=X100, mk=(128, 100), x_tiled=1))
    call(E_ARG, one("xidx with x_tiled", x=Xt, xi=idx))
    call(E_ARG, dict(name="different nsplit, forced 0", mk=[(128, 128)] * 2,
                     descs=[(G, X, None, dict(nsplit=1)), (G, X, None, dict(nsplit=2))]), nsplit=0)
    call(E_ARG, one("nsplit 0 everywhere"), nsplit=0)
    call(E_DTYPE, one("float64"), dt=L.F64)
    (wb, w), (vb, v) = outs()
    slab = torch.zeros(128 * 128 + 128, device=DEV)
    b = L.WgradBatch()
    b.n = 1
    b.d[0] = L.WgradDesc(None, None, 128, 128, 128, 128, 65, 128, L.ptr(slab), L.ptr(slab[128 * 128:]), L.ptr(w), L.ptr(v), 0, 0, 0, 0)
    assert L.lib().agn_wgrad_reduce(C.byref(b), 0, stream()) == E_ARG
    b.n = 0
    assert L.lib().agn_wgrad_reduce(C.byref(b), 1, stream()) == E_ARG
    torch.cuda.synchronize()
    assert R.all_sentinel(wb) and R.all_sentinel(vb)
