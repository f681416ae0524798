"""Irregular graph families for the pooling, hierarchy and model tests (pure torch, CPU, seeded).

Every graph the rest of the suite pools is an `aerognn.meshgen.ellipsoid` lattice: degree 6 everywhere,
candidate lists of a dozen edges, coarse-edge groups of at most 4. The families here reach what a
lattice cannot: receivers with more than 64 and more than 256 pooling candidates (the chunk carry of
pool_uniq / pool_emit and the global-load fallback of pool_cand_sort in csrc/graph.hip), receivers
with none, long coarse-edge groups, parallel edges, self loops, one-way edges, isolated nodes,
single-node graphs and a gap in the batch ids.

Each family returns (n, edge_index int64 [2, E], batch int64 [n]); the edge order is shuffled with the
seeded generator, because the caller's order is the level-0 reference order (Level.refkey).

tests/test_irregular_graphs_cpu.py pins, with the CPU oracle alone, that the cases below reach those
paths; tests/test_gpu_irregular.py runs them through the kernels.
"""
import functools

import torch

BOUNDARY_COUNTS = (63, 64, 65, 255, 256, 257)
NLEVELS = 3

# (family, stride) of every pooling case the GPU tests run (three successive levels each)
POOL_CASES = ([("hub", s) for s in (1, 2, 3, 1000)] + [("complete", s) for s in (2, 8)] +
              [("multi", s) for s in (2, 3, 4, 5)] +
              [(f"boundary{c}", s) for c in BOUNDARY_COUNTS for s in (1, 2)])


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _shuffled(ei, g):
    return ei[:, torch.randperm(ei.shape[1], generator=g)].contiguous()


def hub(n=600, hubs=(0, 299), spokes=400, base_deg=3, seed=1):
    """n * base_deg random pairs, each in both directions (parallel edges and a few self loops arise
    and stay), and per hub an edge to and from `spokes` distinct other nodes: one graph."""
    g = _gen(seed)
    a = torch.randint(n, (n * base_deg,), generator=g)
    b = torch.randint(n, (n * base_deg,), generator=g)
    src, dst = [a, b], [b, a]
    for h in hubs:
        others = torch.cat([torch.arange(h), torch.arange(h + 1, n)])
        s = others[torch.randperm(n - 1, generator=g)[:spokes]]
        hh = torch.full_like(s, h)
        src += [s, hh]
        dst += [hh, s]
    ei = torch.stack([torch.cat(src), torch.cat(dst)])
    return n, _shuffled(ei, g), torch.zeros(n, dtype=torch.long)


def complete(n=48, seed=3):
    """All ordered pairs s != d, one graph."""
    s, d = torch.meshgrid(torch.arange(n), torch.arange(n), indexing="ij")
    keep = s != d
    ei = torch.stack([s[keep], d[keep]])
    return n, _shuffled(ei, _gen(seed)), torch.zeros(n, dtype=torch.long)


MULTI_SIZES = (1, 2, 3, 4, 5, 200, 7)
MULTI_IDS = (0, 1, 2, 3, 4, 6, 7)  # graph id 5 is missing; graph 0 is one node without an edge


def multi(seed=2):
    """Seven graphs in one batch: per graph of more than one node 3 * size random directed edges, every
    2nd and every 3rd of them repeated (parallel edges), a self loop on every other node; the last 10
    nodes of the 200-node graph are isolated."""
    g = _gen(seed)
    srcs, dsts, batch = [], [], []
    off = 0
    for size, gid in zip(MULTI_SIZES, MULTI_IDS):
        batch.append(torch.full((size,), gid, dtype=torch.long))
        if size > 1:
            s = torch.randint(size, (3 * size,), generator=g)
            d = torch.randint(size, (3 * size,), generator=g)
            loops = torch.arange(0, size, 2)
            s = torch.cat([s, s[::2], s[::3], loops])
            d = torch.cat([d, d[::2], d[::3], loops])
            if size == 200:
                keep = (s < size - 10) & (d < size - 10)
                s, d = s[keep], d[keep]
            srcs.append(s + off)
            dsts.append(d + off)
        off += size
    ei = torch.stack([torch.cat(srcs), torch.cat(dsts)])
    return off, _shuffled(ei, g), torch.cat(batch)


def boundary(c, seed=4):
    """One graph of c + 2 nodes: a ring i -> i + 1 over all nodes, and as many spokes into node 0 from
    distinct senders (none of them the ring's) as bring node 0 to exactly c incoming edges. With
    stride 1 the coarse node of node 0 then has exactly c candidates."""
    n = c + 2
    ring = torch.stack([torch.arange(n), (torch.arange(n) + 1) % n])
    spokes = c - int((ring[1] == 0).sum())
    senders = torch.arange(1, 1 + spokes)  # 1 .. c - 1; the ring's sender into node 0 is n - 1
    assert senders.numel() == 0 or int(senders.max()) < n - 1
    ei = torch.cat([ring, torch.stack([senders, torch.zeros_like(senders)])], 1)
    assert int((ei[1] == 0).sum()) == c and ei[0][ei[1] == 0].unique().numel() == c
    return n, _shuffled(ei, _gen(seed + c)), torch.zeros(n, dtype=torch.long)


def family(name):
    if name.startswith("boundary"):
        return boundary(int(name[len("boundary"):]))
    return {"hub": hub, "complete": complete, "multi": multi}[name]()


def candidate_counts(f2c, edge_index, Nc):
    """Pooling candidates per coarse receiver: the fine edges whose receiver pools into it."""
    return torch.bincount(f2c[edge_index[1]], minlength=Nc)


def features(n, E, width, seed):
    """pos [n, 3] (randn, its x column a scaled random permutation: no ties, in fp32 too), node
    [n, width] and edge [E, width] (randn), fp32."""
    g = _gen(seed)
    pos = torch.randn(n, 3, generator=g)
    pos[:, 0] = (torch.randperm(n, generator=g).float() + 0.5) / n * 2 - 1
    return pos, torch.randn(n, width, generator=g), torch.randn(E, width, generator=g)


def group_sizes(f2c, edge_index, Nc):
    """Fine edges per coarse edge (the lengths of the groups the pooled edge means run over)."""
    keys = f2c[edge_index[0]] * max(Nc, 1) + f2c[edge_index[1]]
    return torch.unique(keys, return_counts=True)[1]


def chunk_seams(f2c, edge_index, Nc):
    """pool_uniq / pool_emit walk a receiver's candidates, sorted by coarse sender, 64 at a time and
    carry the last sender across chunks. Returns (same, differ): over all receivers, the chunk starts
    (positions 64, 128, ...) whose candidate has the same coarse sender as its predecessor (the carry
    must keep the group open) and those where it differs (a group opens on lane 0)."""
    cs, cd = f2c[edge_index[0]], f2c[edge_index[1]]
    order = torch.argsort(cd * max(Nc, 1) + cs, stable=True)
    cs, cd = cs[order], cd[order]
    start = torch.zeros(Nc + 1, dtype=torch.long)
    start[1:] = torch.cumsum(torch.bincount(cd, minlength=Nc), 0)
    at = torch.arange(cs.numel()) - start[cd]
    seam = ((at > 0) & (at % 64 == 0)).nonzero().flatten()
    same = int((cs[seam] == cs[seam - 1]).sum())
    return same, seam.numel() - same


@functools.lru_cache(maxsize=None)
def oracle_levels(name, stride, width=8, with_pos=True, dtype=torch.float32):
    """NLEVELS successive R.downsample(..., stable=True) steps of a case (fewer once no edge is left):
    ((node, edge, edge_index, batch, pos) of level 0, [the oracle's 6-tuple per level]). Computed once
    per case and shared; callers must not modify it."""
    from oracle import refcpu as R
    n, ei, batch = family(name)
    pos, node, edge = features(n, ei.shape[1], width, seed=11)
    first = (node.to(dtype), edge.to(dtype), ei, batch, pos if with_pos else None)
    out, cur = [], first
    for _ in range(NLEVELS):
        if cur[2].shape[1] == 0:
            break
        cur = R.downsample(*cur[:5], stride, stable=True)
        out.append(cur)
    return first, out


def seq_group_sum(rows, ptr, order=None):
    """Sequential sums in `rows`' dtype: out[g] = (((0 + r0) + r1) + ...) over the rows order[ptr[g] :
    ptr[g + 1]] (the fixed-order contract of agn_segment_sum, include/aerognn.h)."""
    ptr = ptr.long()
    cnt = ptr[1:] - ptr[:-1]
    out = torch.zeros(cnt.numel(), rows.shape[1], dtype=rows.dtype)
    for j in range(int(cnt.max()) if cnt.numel() else 0):
        live = (cnt > j).nonzero().flatten()
        at = ptr[live] + j
        out[live] = out[live] + rows[at if order is None else order.long()[at]]
    return out
