"""The stream cases that tests/launch_cases.py does not reach (graph build, scans, the registered
scatter operators, data preparation, evaluation, the training tail, bi-stride coarsening), and COVERED:
for every entry point of include/aerognn.h that takes a stream, the cases that must call it.

A case is a builder of (fn, inputs) as tests/streamcheck.py describes; CASES maps its name to
(builder, syncs). syncs=True: the wrapper blocks the host (it reads a count or an index range back, or
uploads a host table with a blocking copy), so only the "busy default stream" variant can say anything.
Shapes are the smallest that still take every code path named in the case's comment.

Importing this module needs neither a GPU nor the library: builders import what they use.
"""
import types

DEV = "cuda"
CASES = {}


def _case(name, syncs=False):
    def deco(f):
        assert name not in CASES
        CASES[name] = (f, syncs)
        return f
    return deco


def _gen(seed):
    import torch
    return torch.Generator(device="cpu").manual_seed(seed)


def _dev(t):
    import numpy as np
    import torch
    return (torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t).to(DEV)


def _level_fields(lv, pre):
    names = ("src", "dst", "rowptr", "refkey", "perm_src", "rowptr_src")
    return {f"{pre}{n}": getattr(lv, n) for n in names}


# --------------------------------------------------------------------------- graph build
def _hub():
    import irregular_graphs as G
    n, ei, batch = G.hub()  # 600 nodes, 5,200 edges, two receivers with more than 256 candidates
    pos, _, _ = G.features(n, ei.shape[1], 1, seed=11)
    return n, ei.to(DEV), batch.to(DEV), pos.to(DEV)


@_case("level_build")
def b_level_build():
    """Level.from_edge_index: iota_keys, the multi-pass radix sort with its copy-back, row_ptr_i64,
    level_index, and the sender grouping (int32 keys)."""
    from aerognn.graph import Level
    n, ei, _, _ = _hub()

    def fn():
        lv = Level.from_edge_index(ei, n)
        return {**_level_fields(lv, ""), "perm": lv.perm, "inv": lv.perm_inv, "perm32": lv.perm32, "inv32": lv.inv32}
    return fn, {"edge_index": ei}


@_case("graph_build", syncs=True)
def b_graph_build():
    """downsample_maps with pos and batch, stride 2: pool_sort_keys, the 32-bit-and-more radix sort,
    pool_assign, the candidate kernels with both scans, pool_edge_emit. Two counts are read with .item()."""
    from aerognn.graph import Level, downsample_maps
    n, ei, batch, pos = _hub()

    def fn():
        lv = Level.from_edge_index(ei, n)
        P = downsample_maps(lv, batch, pos, 2, 1)
        out = {k: getattr(P, k) for k in ("f2c", "c2f", "c2f_ptr", "cbatch", "cand_sorted", "cmem_ptr", "inv")}
        out.update(_level_fields(P.coarse, "coarse."))
        return out
    return fn, {"edge_index": ei, "batch": batch, "pos": pos}


@_case("scan_4097")
def b_scan():
    """exclusive_scan of 4,097 counts: the three-kernel path."""
    import torch
    from aerognn.graph import exclusive_scan
    x = torch.randint(0, 9, (4097,), generator=_gen(1), dtype=torch.int32).to(DEV)
    return (lambda: {"scan": exclusive_scan(x)}), {"x": x}


@_case("row_ptr_i32")
def b_row_ptr():
    """agn_row_ptr on sorted int32 keys (1,000 keys, 300 rows: rows without a key at both ends)."""
    import torch
    from aerognn import _lib as L
    from aerognn.core import stream
    keys = torch.sort(torch.randint(3, 290, (1000,), generator=_gen(2), dtype=torch.int32)).values.to(DEV)

    def fn():
        rp = torch.empty(301, dtype=torch.int32, device=DEV)
        L.check(L.lib().agn_row_ptr(L.ptr(keys), 1000, 300, L.ptr(rp), stream()), "row_ptr")
        return {"rowptr": rp}
    return fn, {"keys": keys}


@_case("index_map")
def b_index_map():
    """agn_index_map: fine id -> coarse id of a sorted selection (-1 elsewhere)."""
    import torch
    from aerognn import _lib as L
    from aerognn.core import stream
    n = 3001
    sel = torch.sort(torch.randperm(n, generator=_gen(3))[:1300]).values.to(torch.int32).to(DEV)

    def fn():
        imap = torch.empty(n, dtype=torch.int32, device=DEV)
        L.check(L.lib().agn_index_map(L.ptr(sel), sel.numel(), n, L.ptr(imap), stream()), "index_map")
        return {"map": imap}
    return fn, {"sel": sel}


# --------------------------------------------------------------------------- scatter operators
@_case("scatter_ops", syncs=True)
def b_scatter_ops():
    """torch.ops.aerognn.scatter_sum (sum and mean), gather_rows (plain and divided by a group size) and
    scatter_max, forward and backward, 3,000 rows of 24 into 700 groups (some empty). The operators check
    their index range on the host."""
    import torch
    import aerognn.ops  # noqa: F401  (registers the operators)
    ops = torch.ops.aerognn
    g = _gen(4)
    n, k, G = 3000, 24, 700
    src = torch.randn(n, k, generator=g).to(DEV).requires_grad_(True)
    tab = torch.randn(G, k, generator=g).to(DEV).requires_grad_(True)
    idx = torch.randint(0, G - 5, (n,), generator=g).to(DEV)
    gs = [torch.randn(G, k, generator=g).to(DEV) for _ in range(3)] + [torch.randn(n, k, generator=g).to(DEV) for _ in range(2)]

    def fn():
        src.grad = tab.grad = None
        outs = [ops.scatter_sum(src, idx, G, False), ops.scatter_sum(src, idx, G, True), ops.scatter_max(src, idx, G)[0],
                ops.gather_rows(tab, idx, None), ops.gather_rows(tab, idx, ops.group_ptr(idx, G))]
        torch.autograd.backward(outs, gs)
        res = {f"out{i}": o.detach() for i, o in enumerate(outs)}
        res.update({"d src": src.grad, "d tab": tab.grad})
        return res
    inputs = {"src": src, "tab": tab, "idx": idx}
    inputs.update({f"g{i}": t for i, t in enumerate(gs)})
    return fn, inputs


@_case("segment_sum2")
def b_segment_sum2():
    """core.segment_sum2: base + two grouped sums in one pass, 300 rows of 40."""
    import torch
    from aerognn import core
    from aerognn.graph import group_by
    g = _gen(5)
    N, k, E = 300, 40, 1500
    base = torch.randn(N, k, generator=g).to(DEV)
    sa, sb = (torch.randn(E, k, generator=g).to(DEV) for _ in range(2))
    (qa, pa), (qb, pb) = (group_by(torch.randint(0, N - 1, (E,), generator=g).to(torch.int32).to(DEV), N) for _ in range(2))

    def fn():
        out = torch.empty(N, k, device=DEV)
        return {"out": core.segment_sum2(N, k, base, (pa, qa, sa), (pb, qb, sb), out)}
    return fn, dict(base=base, sa=sa, sb=sb, pa=pa, qa=qa, pb=pb, qb=qb)


@_case("unpool")
def b_unpool():
    """models.bistride_ops.Unpool: scatter_rows forward, gather_rows backward."""
    import torch
    from models.bistride_ops import Unpool
    g = _gen(6)
    nf, nc, C = 1001, 400, 33
    xc = torch.randn(nc, C, generator=g).to(DEV).requires_grad_(True)
    idx = torch.sort(torch.randperm(nf, generator=g)[:nc]).values.to(DEV)
    go = torch.randn(nf, C, generator=g).to(DEV)
    m = Unpool()

    def fn():
        xc.grad = None
        out = m(xc, idx, nf)
        out.backward(go)
        return {"fine": out.detach(), "d xc": xc.grad}
    return fn, {"xc": xc, "idx": idx, "g": go}


# --------------------------------------------------------------------------- data preparation
def _meshes():
    from aerognn.meshgen import ellipsoid
    return [ellipsoid(nu, nv, seed=s) for s, (nu, nv) in enumerate(((12, 8), (10, 7), (9, 6)))]


@_case("edge_attr")
def b_edge_attr():
    """compute_edge_attr in the caller's order, in a level's CSC order (perm) and normalised."""
    import torch
    from aerognn.data import compute_edge_attr
    from aerognn.graph import Level
    m = _meshes()[0]
    pos, ei = _dev(m["pos"]), _dev(m["edge_index"])
    perm = Level.from_edge_index(ei, pos.shape[0]).perm.clone()
    g = _gen(7)
    stats = {"edge_mean": torch.randn(4, generator=g).to(DEV), "edge_std": (torch.rand(4, generator=g) + 0.5).to(DEV)}

    def fn():
        return {"plain": compute_edge_attr(pos=pos, edge_index=ei), "csc": compute_edge_attr(pos=pos, edge_index=ei, perm=perm),
                "scaled": compute_edge_attr(pos=pos, edge_index=ei, perm=perm, stats=stats)}
    return fn, {"pos": pos, "edge_index": ei, "perm": perm, **stats}


def _samples(rows):
    import torch
    g = _gen(8)
    return [types.SimpleNamespace(x=torch.randn(r, 6, generator=g).to(DEV), edge_attr=torch.randn(3 * r, 4, generator=g).to(DEV),
                                  y=torch.randn(r, 4, generator=g).to(DEV)) for r in rows]


@_case("norm_stats")
def b_norm_stats():
    """compute_normalization_stats over 4,097 node rows (two blocks of the column-sum kernel)."""
    from aerognn.data import compute_normalization_stats
    ds = _samples((4000, 97))
    inputs = {f"{k}{i}": getattr(d, k) for i, d in enumerate(ds) for k in ("x", "edge_attr", "y")}
    return (lambda: dict(compute_normalization_stats(ds))), inputs


@_case("normalize")
def b_normalize():
    """normalize_data on two samples and denormalize_predictions."""
    import torch
    from aerognn.data import denormalize_predictions, normalize_data
    src = _samples((300, 41))
    g = _gen(9)
    stats = {}
    for key, w in (("node", 6), ("edge", 4), ("target", 4)):
        stats[f"{key}_mean"] = torch.randn(w, generator=g).to(DEV)
        stats[f"{key}_std"] = (torch.rand(w, generator=g) + 0.5).to(DEV)

    def fn():
        ds = [types.SimpleNamespace(**vars(d)) for d in src]  # normalize_data rebinds the attributes
        normalize_data(ds, stats)
        out = {f"{k}{i}": getattr(d, k) for i, d in enumerate(ds) for k in ("x", "edge_attr", "y")}
        out["back"] = denormalize_predictions(out["y0"], stats)
        return out
    inputs = {f"{k}{i}": getattr(d, k) for i, d in enumerate(src) for k in ("x", "edge_attr", "y")}
    return fn, {**inputs, **stats}


@_case("collate", syncs=True)
def b_collate():
    """collate of three small meshes (the offsets are uploaded with blocking copies)."""
    from aerognn.data import collate
    ds = [types.SimpleNamespace(**{k: _dev(m[k]) for k in ("x", "edge_attr", "y", "pos", "edge_index")}) for m in _meshes()]

    def fn():
        b = collate(ds)
        return {k: getattr(b, k) for k in ("x", "edge_attr", "y", "pos", "edge_index", "batch")}
    return fn, {f"{k}{i}": getattr(d, k) for i, d in enumerate(ds) for k in ("x", "edge_attr", "y", "pos", "edge_index")}


# --------------------------------------------------------------------------- evaluation
def _one_graph(n):
    import torch
    return torch.tensor([0, n], dtype=torch.int32).to(DEV)


@_case("eval_sums")
def b_eval_sums():
    """agn_eval_sums on the smallest golden case (5 rows, 4 features)."""
    import torch
    import aerognn.ops  # noqa: F401
    from golden_util import load
    d, _ = load("evalmetrics_f32")
    t = {k: d[f"{k}2"].to(DEV) for k in ("pred", "y", "mean", "std")}
    gptr = _one_graph(5)
    return (lambda: {"sums": torch.ops.aerognn.eval_sums(t["pred"], t["y"], t["mean"], t["std"], gptr)}), t


@_case("aero_forces_areas")
def b_aero_forces_areas():
    """agn_aero_forces with given element areas (the 3-D golden, 168 elements)."""
    import torch
    import aerognn.ops  # noqa: F401
    from golden_util import load
    d, _ = load("aero3d_f32")
    t = {k: d[k].to(DEV) for k in ("p", "shear", "normals", "areas")}
    gptr = _one_graph(168)

    def fn():
        return {"sums": torch.ops.aerognn.aero_forces(t["p"], t["shear"], t["normals"], None, t["areas"], None, gptr, [])[0]}
    return fn, t


@_case("aero_forces_mesh", syncs=True)
def b_aero_forces_mesh():
    """agn_aero_forces with the areas from the mesh (the 96-node 2-D golden, moments about a centre);
    the operator checks the edge ids on the host."""
    import torch
    import aerognn.ops  # noqa: F401
    from golden_util import load
    d, meta = load("aero2d_f32")
    ph = d["phys_true1"]
    t = dict(p=ph[:, 0].contiguous().to(DEV), shear=ph[:, 1:3].contiguous().to(DEV), normals=d["normals1"].to(DEV),
             pos=d["pos1"].to(DEV), edge_index=d["edge_index1"].to(DEV))
    gptr = _one_graph(96)

    def fn():
        sums, areas = torch.ops.aerognn.aero_forces(t["p"], t["shear"], t["normals"], t["pos"], None, t["edge_index"], gptr,
                                                    list(meta["center"]))
        return {"sums": sums, "areas": areas}
    return fn, t


def _surface():
    from golden_util import load
    d, _ = load("aero3d_mesh_f32")  # 96 points, 147 cells of 3 and 4 corners
    return {k: d[k].to(DEV) for k in ("pos", "offsets", "conn", "true", "pred")}


@_case("surface_forces", syncs=True)
def b_surface_forces():
    """agn_surface_forces with the cell outputs; the operator reads the face-id range back."""
    import torch
    from aerognn import surface
    t = _surface()
    g = _gen(10)
    stats = {"target_mean": torch.randn(4, generator=g).to(DEV), "target_std": (torch.rand(4, generator=g) + 0.5).to(DEV)}

    def fn():
        ss = surface.integrate_surface(t["pos"], (t["offsets"], t["conn"]), [t["true"], t["pred"]], stats=stats,
                                       return_cells=True)
        return {"force": ss.force, "abs_force": ss.abs_force, "areas": ss.areas, "normals": ss.normals, "cells": ss.cells}
    return fn, {**t, **stats}


@_case("face_edges", syncs=True)
def b_face_edges():
    """edges_from_faces: agn_face_edges, whose edge count is read with .item()."""
    from aerognn import surface
    t = _surface()
    return (lambda: {"edge_index": surface.edges_from_faces((t["offsets"], t["conn"]), 96)}), \
        {"offsets": t["offsets"], "conn": t["conn"]}


# --------------------------------------------------------------------------- training tail
@_case("mse_loss")
def b_mse_loss():
    """train.mse_loss_grad (agn_mse_loss) in fp32 with an accumulator, and with a LossScaler on fp16
    predictions (agn_mse_loss_scaled); more rows than one first-stage chunk."""
    import torch
    from aerognn import train
    g = _gen(11)
    n = train.chunk_rows() + 37
    pred, y = (torch.randn(n, 4, generator=g).to(DEV) for _ in range(2))
    p16 = pred.half()
    acc0 = torch.tensor(1.5, dtype=torch.float64).to(DEV)
    scaler = train.LossScaler(DEV, init_scale=1024.0)
    state = scaler._device_state(DEV)

    def fn():
        acc = acc0.clone()
        loss, dp = train.mse_loss_grad(pred, y, acc=acc)
        loss16, dp16 = train.mse_loss_grad(p16, y, scaler=scaler)
        return {"loss": loss, "dpred": dp, "acc": acc, "loss16": loss16, "dpred16": dp16}
    return fn, {"pred": pred, "y": y, "pred16": p16, "acc0": acc0, "scale_state": state}


def _adam_case(dtype, master, scaled):
    """One aerognn.optim.Adam step over three tensors (5 elements, one chunk and 3, 1,000), from the same
    start at every call: parameters, moments, counters and the scaler's state are put back first. The
    optimizer has taken one step when the case starts, so that a call replays its plan and uploads
    nothing with a blocking copy."""
    import torch
    from aerognn import optim, train
    g = _gen(12)
    sizes = (5, optim.chunk_elems() + 3, 1000)
    p0 = [torch.randn(s, generator=g).to(dtype).to(DEV) for s in sizes]
    gr = [(torch.randn(s, generator=g) * (64.0 if scaled else 1.0)).to(dtype).to(DEV) for s in sizes]
    ps = [t.clone().requires_grad_(True) for t in p0]
    opt = optim.Adam(ps, lr=1e-2, weight_decay=1e-2, master_weights=master)
    scaler = train.LossScaler(DEV, init_scale=64.0, growth_interval=1) if scaled else None
    state0 = scaler._device_state(DEV).clone() if scaled else None
    inputs = {f"p0_{i}": t for i, t in enumerate(p0)}
    inputs.update({f"g{i}": t for i, t in enumerate(gr)})
    if scaled:
        inputs["scale_state0"] = state0

    def fn():
        opt.state_dict()  # a skipped scaled step of the call before is resolved before the counters are reset
        with torch.no_grad():
            for p, q, gq in zip(ps, p0, gr):
                p.copy_(q)
                p.grad = gq
                st = opt.state.get(p)
                if st:
                    st["exp_avg"].zero_()
                    st["exp_avg_sq"].zero_()
                    st["step"].fill_(0)
                    if master:
                        st["master_param"].copy_(q)
            if scaled:
                scaler._device_state(DEV).copy_(state0)
                scaler.step(opt)
                scaler.update()
            else:
                opt.step()
        out = {}
        for i, p in enumerate(ps):
            st = opt.state[p]
            out.update({f"p{i}": p.detach(), f"m{i}": st["exp_avg"], f"v{i}": st["exp_avg_sq"]})
            if master:
                out[f"w{i}"] = st["master_param"]
        if scaled:
            out["scale_state"] = scaler._device_state(DEV)
        return out

    fn()  # the first step: state, descriptor table and chunk map
    torch.cuda.synchronize()
    return fn, inputs


@_case("adam_f32")
def b_adam_f32():
    import torch
    return _adam_case(torch.float32, False, False)


@_case("adam_master_bf16")
def b_adam_master():
    import torch
    return _adam_case(torch.bfloat16, True, False)


@_case("adam_scaled_f32")
def b_adam_scaled():
    """LossScaler.step + update: agn_grad_check, agn_adam_step_scaled, agn_loss_scale_update."""
    import torch
    return _adam_case(torch.float32, False, True)


@_case("adam_master_scaled_f16")
def b_adam_master_scaled():
    import torch
    return _adam_case(torch.float16, True, True)


@_case("reduce_partials")
def b_reduce_partials():
    """core.reduce_partials: the fixed-order column sums of 37 partial rows."""
    import torch
    from aerognn import core
    p = torch.randn(37, 200, generator=_gen(13)).to(DEV)

    def fn():
        out = torch.empty(200, device=DEV)
        core.reduce_partials(p, 37, 200, out)
        return {"out": out}
    return fn, {"partial": p}


@_case("fault_poll", syncs=True)
def b_fault_poll():
    """agn_fault_status_async: the device fault word copied to page-locked memory on the stream. The
    word is library state (agn_debug_set_fault writes it from the host, no fault is involved): the true
    value is 5, the poison 0, and the word is 0 again when the case ends."""
    import ctypes as C
    import torch
    from aerognn import _lib as L
    from aerognn import core
    buf = torch.zeros(1, dtype=torch.int32, pin_memory=True)
    mark = torch.tensor([7], dtype=torch.int32).to(DEV)  # (every case has a tensor input)

    def fn():
        L.check(L.lib().agn_fault_status_async(C.c_void_p(buf.data_ptr()), core.stream()), "fault_status_async")
        return {"word": buf.to(DEV, non_blocking=True), "mark": mark + 0}
    fn.restore_state = lambda: L.check(L.lib().agn_debug_set_fault(5))
    fn.poison_state = lambda: L.check(L.lib().agn_debug_set_fault(0))
    return fn, {"mark": mark}


# --------------------------------------------------------------------------- bi-stride coarsening
@_case("bistride", syncs=True)
def b_bistride():
    """bfs_distance, both seeds, select_bistride_nodes, subgraph_edges and a two-level
    create_multiscale_graph on the 24 x 14 ellipsoid; all of them wait for the device (aerognn.h)."""
    import torch
    from aerognn import bistride as B
    from aerognn.meshgen import ellipsoid
    m = ellipsoid(24, 14)
    ei, pos = _dev(m["edge_index"]), _dev(m["pos"])
    n = pos.shape[0]

    def fn():
        adj = B.out_adjacency(ei, n)
        seeds = [B.bistride_seed(ei, n, pos, adj), B.bistride_seed(ei, n, None, adj)]
        sel = B.select_bistride_nodes(ei, n, pos)
        ms = B.create_multiscale_graph(ei, pos, n, 2)
        out = {"seeds": torch.tensor(seeds, device=DEV), "dist": B.bfs_distance(ei, n, seeds[1], adj), "sel": sel,
               "sub": B.subgraph_edges(ei, sel, n)}
        out.update({f"ms.ei{i}": t for i, t in enumerate(ms["edge_indices"])})
        out.update({f"ms.sel{i}": t for i, t in enumerate(ms["node_indices"])})
        return out
    return fn, {"edge_index": ei, "pos": pos}


# --------------------------------------------------------------------------- what must be called
# entry point -> the cases (of launch_cases.CASES or of CASES above) whose runs must call it; the last
# test of tests/test_gpu_streams.py compares this with what the counting wrappers saw.
COVERED = {
    "agn_wgrad": ["gmp_f32_h32_sum_add_train", "gmp_f32_h32_sum_mean_train", "gmp_bf16_h128_sum", "L_gmp_train",
                  "L_gmp_train_EB_SAVED_0"],
    "agn_wgrad_segsum": ["L_gmp_train", "L_gmp_train_EB_SAVED_0", "L_gmp_train_EDGE_AGG_0",
                         "L_gmp_train_PROJ_KERNEL_0", "L_gmp_train_bf16_params"],
    "agn_colsum": ["gmp_f32_h32_sum_add_train", "gmp_f32_h32_sum_mean_train", "gmp_bf16_h128_sum", "L_gmp_train",
                   "L_gmp_train_EB_SAVED_0"],
    "agn_pack": ["gmp_f32_h32_sum_add_train", "gmp_f32_h32_sum_add_infer", "gmp_f32_h32_sum_mean_train", "L_gmp_train",
                 "L_gmp_train_EB_SAVED_0"],
    "agn_mlp_forward": ["gmp_f32_h32_sum_add_train", "gmp_f32_h32_sum_add_infer", "gmp_f32_h32_sum_mean_train",
                        "L_gmp_train", "L_gmp_train_EB_SAVED_0"],
    "agn_mlp_backward": ["gmp_f32_h32_sum_add_train", "gmp_f32_h32_sum_mean_train", "gmp_bf16_h128_sum", "L_gmp_train",
                         "L_gmp_train_EB_SAVED_0"],
    "agn_reduce_partials": ["reduce_partials"],
    "agn_segment_sum": ["gmp_f32_h32_sum_add_train", "gmp_f32_h32_sum_mean_train", "gmp_bf16_h128_sum", "L_gmp_train",
                        "L_gmp_train_EB_SAVED_0", "scatter_ops"],
    "agn_segment_sum2": ["gmp_f32_h32_cat_add_train", "gmp_f32_h32_cat_mean_train", "gmp_bf16_h128_cat",
                         "edge_block_cat", "gmp_order", "segment_sum2"],
    "agn_segment_max": ["scatter_ops"],
    "agn_segment_max_backward": ["scatter_ops"],
    "agn_gather_rows": ["gmp_f32_h32_sum_mean_train", "gmp_f32_h32_cat_mean_train", "node_block_add", "L_v2_train",
                        "L_v2_train_V2_EDGE32_0", "scatter_ops", "unpool"],
    "agn_radix_sort_u64": ["mlp_encoder_k6_rows_dx", "trial1_model_h32", "f64_mlp_rows_dx", "f64_gmp_sum",
                           "level_build", "graph_build", "scatter_ops", "aero_forces_mesh", "bistride"],
    "agn_row_ptr": ["row_ptr_i32"],
    "agn_exclusive_scan_i32": ["graph_build", "scan_4097"],
    "agn_iota_keys": ["mlp_encoder_k6_rows_dx", "trial1_model_h32", "f64_mlp_rows_dx", "f64_gmp_sum", "level_build",
                      "graph_build", "scatter_ops", "aero_forces_mesh", "bistride"],
    "agn_level_index": ["trial1_model_h32", "level_build", "graph_build"],
    "agn_row_ptr_i64": ["mlp_encoder_k6_rows_dx", "trial1_model_h32", "f64_mlp_rows_dx", "f64_gmp_sum", "level_build",
                        "graph_build", "scatter_ops", "aero_forces_mesh", "bistride"],
    "agn_pool_sort_keys": ["graph_build"],
    "agn_pool_assign": ["graph_build"],
    "agn_pool_edge_candidates": ["graph_build"],
    "agn_pool_edge_sort": ["graph_build"],
    "agn_pool_edge_emit": ["graph_build"],
    "agn_bfs_distance": ["bistride"],
    "agn_center_seed": ["bistride"],
    "agn_maxdeg_seed": ["bistride"],
    "agn_bistride_select": ["bistride"],
    "agn_index_map": ["index_map", "bistride"],
    "agn_subgraph_edges": ["bistride"],
    "agn_scatter_rows": ["unpool"],
    "agn_wec_forward": ["wec", "wec_given"],
    "agn_wec_backward": ["wec", "wec_given"],
    "agn_edge_bwd_fused": ["L_gmp_train", "L_gmp_train_EB_SAVED_0"],
    "agn_encoder_bwd_fused": ["L_mlp_encoder_rows", "L_mlp_encoder_rows_bf16_params"],
    "agn_fault_status_async": ["fault_poll"],
    "agn_edge_forward32": ["L_gmp_train", "L_gmp_train_EB_SAVED_0"],
    "agn_edge_agg_fixup": ["L_gmp_train", "L_gmp_train_EB_SAVED_0"],
    "agn_wgrad_reduce": ["L_gmp_train", "L_gmp_train_EB_SAVED_0"],
    "agn_proj_forward": ["gmp_bf16_h128_sum", "L_gmp_train", "L_gmp_train_EB_SAVED_0"],
    "agn_proj_backward": ["gmp_bf16_h128_sum", "L_gmp_train", "L_gmp_train_EB_SAVED_0"],
    "agn_edge_features": ["edge_attr"],
    "agn_normalize": ["normalize"],
    "agn_col_stats": ["norm_stats"],
    "agn_collate": ["collate"],
    "agn_fourier_embed": ["fourier_fn", "fourier_op"],
    "agn_fourier_embed_bwd": ["fourier_fn", "fourier_op"],
    "agn_eval_sums": ["eval_sums"],
    "agn_aero_forces": ["aero_forces_areas", "aero_forces_mesh"],
    "agn_surface_forces": ["surface_forces"],
    "agn_face_edges": ["face_edges"],
    "agn_mse_loss": ["mse_loss"],
    "agn_adam_step": ["adam_f32"],
    "agn_adam_step_master": ["adam_master_bf16"],
    "agn_mse_loss_scaled": ["mse_loss"],
    "agn_grad_check": ["adam_scaled_f32", "adam_master_scaled_f16"],
    "agn_adam_step_scaled": ["adam_scaled_f32"],
    "agn_adam_step_master_scaled": ["adam_master_scaled_f16"],
    "agn_loss_scale_update": ["adam_scaled_f32", "adam_master_scaled_f16"],
    "agn_act_dropout_fwd": ["mlp_dropout_h32", "act_dropout_fn", "act_dropout_op"],
    "agn_act_dropout_bwd": ["mlp_dropout_h32", "act_dropout_fn", "act_dropout_op"],
    "agn_f64_gemm": ["f64_mlp_rows_dx", "f64_gmp_sum"],
    "agn_f64_wgrad": ["f64_mlp_rows_dx", "f64_gmp_sum"],
    "agn_f64_layernorm_fwd": ["f64_mlp_rows_dx", "f64_gmp_sum"],
    "agn_f64_layernorm_bwd": ["f64_mlp_rows_dx", "f64_gmp_sum"],
}
