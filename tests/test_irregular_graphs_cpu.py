"""The irregular graph families (tests/irregular_graphs.py) reach the pooling paths a lattice cannot.

CPU only and built from the oracle's R.downsample(..., stable=True) alone, never from the kernels:
for the (family, stride, level) cases tests/test_gpu_irregular.py runs, the candidate lists are long
enough for the global-load fallback of pool_cand_sort_kernel (more than 256), for the chunk carry
of pool_uniq_kernel / pool_emit_kernel (65 to 256, and a coarse-sender group lying across a
64-candidate chunk start), some receiver has no candidate at all, a coarse-edge group is at least 64
fine edges long, coarse self loops exist, and boundary(c) puts exactly c candidates on one receiver.
If a family is ever shrunk this fails, instead of the GPU tests quietly losing their coverage.
"""
import pytest
import torch

import irregular_graphs as G


def _stats(name, stride):
    """Per level of a case: (candidate counts, group sizes, coarse self loops, chunk seams)."""
    first, levels = G.oracle_levels(name, stride)
    out, ei = [], first[2]
    for cn, ce, cei, cb, cp, f2c in levels:
        Nc = cn.shape[0]
        out.append((G.candidate_counts(f2c, ei, Nc), G.group_sizes(f2c, ei, Nc), int((cei[0] == cei[1]).sum()),
                    G.chunk_seams(f2c, ei, Nc)))
        ei = cei
    return out


def _over(cc):
    return int((cc > 256).sum())


def _mid(cc):
    return int(((cc >= 65) & (cc <= 256)).sum())


def test_every_case_runs_all_levels():
    for name, stride in G.POOL_CASES:
        first, levels = G.oracle_levels(name, stride)
        assert len(levels) == G.NLEVELS, (name, stride)
        for lv in levels:
            assert lv[2].shape[1] > 0, (name, stride)  # coarse edges at every level: all three kernels run


def test_families_have_the_features_a_lattice_lacks():
    n, ei, batch = G.hub()
    assert (n, ei.shape[1]) == (600, 5200) and int(batch.max()) == 0
    assert int((ei[0] == ei[1]).sum()) > 0  # self loops in the input
    assert torch.unique(ei[0] * n + ei[1]).numel() < ei.shape[1]  # parallel edges
    deg = torch.bincount(ei[1], minlength=n)
    assert int(deg[0]) >= 400 and int(deg[299]) >= 400 and int(deg.median()) <= 10
    n, ei, batch = G.complete()
    assert (n, ei.shape[1]) == (48, 48 * 47) and torch.unique(ei[0] * n + ei[1]).numel() == ei.shape[1]
    n, ei, batch = G.multi()
    assert n == sum(G.MULTI_SIZES) and torch.unique(batch).tolist() == list(G.MULTI_IDS)
    assert torch.equal(torch.bincount(batch)[list(G.MULTI_IDS)], torch.tensor(G.MULTI_SIZES))
    assert bool((batch[1:] >= batch[:-1]).all())
    assert bool((batch[ei[0]] == batch[ei[1]]).all())  # no edge between graphs
    touched = torch.zeros(n, dtype=torch.bool)
    touched[ei[0]] = True
    touched[ei[1]] = True
    iso = (~touched).nonzero().flatten()
    last200 = int((batch <= 6).sum())  # end of the 200-node graph
    assert set(range(last200 - 10, last200)) <= set(iso.tolist()) and 0 in iso.tolist()
    assert int((ei[0] == ei[1]).sum()) > 0 and torch.unique(ei[0] * n + ei[1]).numel() < ei.shape[1]
    pairs = set(map(tuple, ei.t().tolist()))
    assert any((d, s) not in pairs for s, d in pairs)  # one-way edges


def test_hub_reaches_the_fallback_sort_and_the_chunk_carry():
    s1, s2, s3, s1000 = (_stats("hub", s) for s in (1, 2, 3, 1000))
    for st in (s1, s2, s3, s1000):
        assert _over(st[0][0]) >= 1  # level 1: the hubs' lists take the global-load rank loop
    assert _over(s2[1][0]) >= 1  # level 2 (coarse refkey) takes it too
    assert _mid(s2[2][0]) >= 1 and _mid(s3[1][0]) >= 1 and _mid(s3[2][0]) >= 1  # LDS sort, several chunks
    for cc, gs, loops, (same, differ) in s2 + s3:
        assert loops > 0 and same > 0 and differ > 0
    # a stride larger than the graph: one coarse node, every edge a candidate, one coarse self loop
    cc, gs, loops, (same, differ) = s1000[0]
    assert cc.tolist() == [5200] and gs.tolist() == [5200] and loops == 1 and same == 5200 // 64


def test_complete_graph_group_lengths():
    cc, gs, loops, (same, differ) = _stats("complete", 8)[0]
    assert cc.tolist() == [376] * 6 and int(gs.max()) == 64 and loops == 6 and same > 0
    cc, gs, loops, (same, differ) = _stats("complete", 2)[0]
    assert cc.tolist() == [94] * 24 and loops == 24 and same + differ == 24


@pytest.mark.parametrize("stride", [2, 3, 4, 5])
def test_multi_has_an_empty_receiver_at_every_level(stride):
    st = _stats("multi", stride)
    for cc, gs, loops, _ in st:
        assert int((cc == 0).sum()) >= 1 and loops > 0
    assert int(st[0][1].max()) >= 12  # parallel edges pool into long groups
    first, levels = G.oracle_levels("multi", stride)
    for lv in levels:  # the single-node graph 0 and the gap at id 5 survive every level
        assert lv[3][0] == 0 and int((lv[3] == 0).sum()) == 1 and 5 not in lv[3].tolist()


@pytest.mark.parametrize("c", G.BOUNDARY_COUNTS)
def test_boundary_counts_are_exact(c):
    for stride, want in ((1, c), (2, c + 1)):  # stride 2 pools node 0 with a node of one incoming edge
        first, levels = G.oracle_levels(f"boundary{c}", stride)
        f2c = levels[0][5]
        cc = G.candidate_counts(f2c, first[2], levels[0][0].shape[0])
        assert int(cc[f2c[0]]) == want and int(cc.max()) == want
        assert int((cc == want).sum()) == 1
    # stride 1 keeps the graph: the same count meets the coarse (row * Nc + col) order at levels 2, 3
    for cc, gs, loops, (same, differ) in _stats(f"boundary{c}", 1):
        assert int(cc.max()) == c and int(gs.max()) == 1 and same == 0 and differ == (c - 1) // 64


def test_pooled_means_are_sequential_sums():
    """The oracle's pooled means are bitwise a sequential sum in reference order and one division (the
    contract of agn_segment_sum): what makes exact equality the bar on the GPU, the 5200-long group
    included."""
    for name, stride in (("hub", 2), ("hub", 1000), ("complete", 8), ("multi", 3)):
        for dtype in (torch.float32, torch.float64):
            first, levels = G.oracle_levels(name, stride, dtype=dtype)
            node, edge, ei = first[:3]
            cn, ce, cei, cb, cp, f2c = levels[0]
            Nc = cn.shape[0]
            keys = f2c[ei[0]] * Nc + f2c[ei[1]]
            inv = torch.unique(keys, return_inverse=True)[1]
            for rows, idx, want in ((edge, inv, ce), (node, f2c, cn)):
                cnt = torch.bincount(idx, minlength=want.shape[0])
                ptr = torch.zeros(cnt.numel() + 1, dtype=torch.long)
                ptr[1:] = torch.cumsum(cnt, 0)
                s = G.seq_group_sum(rows, ptr, torch.argsort(idx, stable=True))
                assert torch.equal(s / cnt.clamp(min=1).to(dtype)[:, None], want), (name, stride, dtype)
