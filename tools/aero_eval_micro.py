"""Micro-timing of the evaluation kernels at C3 size (1 M nodes / 6 M directed edges / 4 targets):
agn_eval_sums and agn_aero_forces against the same quantities composed from torch operators on the
device (the reference's own expressions of inference.py:76-126, :337-350 and utils.py:451-559, with the
per-edge Python loop of utils.py:516-520 replaced by index_add_), and against agn_col_stats and
agn_segment_sum as the bandwidth yardsticks of the same machine.

  python tools/aero_eval_micro.py [--n 1000] [--iters 20] [--surface-only]

The last rows are the 3-D surface passes (agn_surface_forces with two field sets and the geometry inline,
agn_face_edges) on ellipsoid(n, n) with meshgen.lattice_faces, beside the same quantities from torch
operators (gathers + linalg.cross for the forces, torch.unique for the edges); --surface-only runs
those alone.

Graph: an n x n triangulated grid (6 neighbours per interior node) with 2-D positions, edges in
(sender, receiver) order as to_undirected leaves them. Per pass: ms per call (HIP events on torch's
current stream), the bytes the pass must move, GB/s. The last line is one JSON object.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "aero-gnn_amd"))

from aerognn import _lib, aero  # noqa: E402
from aerognn.graph import group_by  # noqa: E402

dev = torch.device("cuda", 0)


def grid_mesh(n):
    ids = np.arange(n * n).reshape(n, n)
    src, dst = [], []
    for di, dj in ((0, 1), (1, 0), (1, 1)):
        a, b = ids[: n - di, : n - dj].ravel(), ids[di:, dj:].ravel()
        src += [a, b]
        dst += [b, a]
    src, dst = np.concatenate(src), np.concatenate(dst)
    o = np.lexsort((dst, src))
    rng = np.random.default_rng(0)
    jj, ii = np.meshgrid(np.arange(n), np.arange(n))
    pos = (np.stack([ii, jj], -1).reshape(-1, 2) + 0.3 * rng.random((n * n, 2))) / n
    return pos.astype(np.float32), np.stack([src[o], dst[o]]).astype(np.int64)


def timeit(f, it):
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(it):
        f()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / it


def torch_metrics(pred, y, mean, std):
    """What run_inference computes per case, as device tensors (no .item(): no host syncs timed)."""
    out = []
    pp, tp = pred * std + mean, y * std + mean
    for a, b in ((pred, y), (pp, tp)):
        for j in range(a.shape[1]):
            out.append(torch.mean(torch.abs(a[:, j] - b[:, j])))
            out.append(torch.mean((a[:, j] - b[:, j]) ** 2))
        out.append(torch.mean(torch.abs(a - b)))
        out.append(torch.mean((a - b) ** 2))
        nz = torch.abs(b) > 1e-8
        q = (a[nz] - b[nz]) / b[nz]
        out.append(torch.mean(torch.abs(q)))
        out.append(torch.sqrt(torch.mean(q ** 2)))
        rmse = torch.sqrt(torch.mean((a - b) ** 2, dim=0))
        mabs = torch.mean(torch.abs(b), dim=0)
        out.append(torch.mean(torch.where(mabs > 1e-8, rmse / mabs, torch.zeros_like(rmse))) * 100)
    return torch.stack(out)


def torch_forces(pos, ei, normals, pressure, shear):
    """calculate_aero_coefficients_2d's arithmetic on the device, the area loop as index_add_."""
    ln = torch.linalg.norm(pos[ei[1]] - pos[ei[0]], dim=1)
    areas = torch.zeros(pos.shape[0], dtype=torch.float64, device=pos.device)
    areas.index_add_(0, ei[0], ln.double() / 2 * 1e-2)
    F = (pressure[:, None] * normals).double() * areas[:, None] - shear.double() * areas[:, None]
    r = pos.double()
    M = r[:, 0] * F[:, 1] - r[:, 1] * F[:, 0]
    return torch.cat([F.sum(0), M.sum().reshape(1)])


def torch_surface(pos, tri, fields, mean, std):
    """inference.py:310-320 + utils.py:385-448 for triangles, composed from torch operators: cell areas
    and normals in fp64, point-to-cell means, F = p n A - tau A summed per set."""
    p = pos.double()
    p0 = p[tri[:, 0]]
    c = torch.linalg.cross(p[tri[:, 1]] - p0, p[tri[:, 2]] - p0)
    ln = torch.linalg.norm(c, dim=1, keepdim=True)
    area, nrm = 0.5 * ln, (c / ln).float()
    out = []
    for f in fields:
        cell = (f * std + mean)[tri].double().mean(1).float()
        out.append(((cell[:, :1] * nrm).double() * area - cell[:, 1:].double() * area).sum(0))
    return torch.stack(out)


def torch_edges(tri, n):
    """extract_all_edges + to_undirected from torch operators: both directions of every side, unique keys."""
    u = torch.cat([tri[:, 0], tri[:, 1], tri[:, 2]])
    v = torch.cat([tri[:, 1], tri[:, 2], tri[:, 0]])
    key = torch.unique(torch.cat([u * n + v, v * n + u]))
    return torch.stack([key // n, key % n])


def surface_rows(report, n, iters):
    """agn_surface_forces (two field sets, geometry inline) and agn_face_edges on ellipsoid(n, n) with its
    lattice_faces (n = 1000: 1 M points, about 2 M triangles), beside the torch compositions."""
    from aerognn import surface
    from aerognn.meshgen import ellipsoid, lattice_faces
    pos = torch.from_numpy(ellipsoid(n, n, unique_x=False)["pos"]).to(dev)
    tri = torch.from_numpy(lattice_faces(n, n)).to(dev)
    N, C = pos.shape[0], tri.shape[0]
    torch.manual_seed(1)
    y = torch.randn(N, 4, device=dev)
    pred = y + 0.1 * torch.randn(N, 4, device=dev)
    mean = torch.tensor([1e5, 3.0, -2.0, 1.5], device=dev)
    std = torch.tensor([3e4, 50.0, 40.0, 20.0], device=dev)
    gptr = torch.tensor([0, C], dtype=torch.int32, device=dev)
    print(f"surface: N={N} cells={C}", flush=True)
    # what the pass must move: the face list once, every point's position and two field rows once
    nbytes = C * 3 * 8 + N * (3 * 4 + 2 * 4 * 4)
    op = lambda: torch.ops.aerognn.surface_forces(pos, None, tri, [y, pred], mean, std, gptr, False)  # noqa: E731
    report("surface_forces (ours, op, ids checked)", timeit(op, iters), nbytes)
    L = _lib.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    out = torch.zeros(1, 2, 2, 3, dtype=torch.float64, device=dev)
    scratch = torch.empty(int(L.agn_surface_forces_temp_bytes(C, 1, 2)), dtype=torch.uint8, device=dev)
    fptr = (ctypes.c_void_p * 2)(y.data_ptr(), pred.data_ptr())
    fld = (ctypes.c_int * 2)(4, 4)

    def kern():
        rc = L.agn_surface_forces(_lib.F32, N, p(pos), 3, C, None, p(tri), tri.numel(), 3, _lib.F32, 2, fptr, fld, p(mean),
                                  p(std), p(gptr), 1, p(out), None, None, None, p(scratch), st)
        assert rc == 0, rc
    report("surface_forces (ours, kernels only)", timeit(kern, iters), nbytes)
    report("surface forces (torch composition)", timeit(lambda: torch_surface(pos, tri, [y, pred], mean, std), iters))
    ours = op()[0][0]
    ref = torch_surface(pos, tri, [y, pred], mean, std)
    print("surface: ours vs torch composition, |diff| / S:", ((ours[:, 0] - ref).abs() / ours[:, 1]).tolist(), flush=True)
    report("edges_from_faces (ours, count read back)", timeit(lambda: surface.edges_from_faces(tri, N), iters))
    report("edges (torch composition, unique)", timeit(lambda: torch_edges(tri, N), iters))
    assert torch.equal(surface.edges_from_faces(tri, N), torch_edges(tri, N))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--surface-only", action="store_true", help="only the 3-D surface rows")
    a = ap.parse_args()
    res = {}

    def report(name, ms, nbytes=None):
        gbs = None if nbytes is None else nbytes / ms / 1e6
        res[name] = {"ms": round(ms, 4), "bytes": nbytes, "GBps": None if gbs is None else round(gbs, 1)}
        tail = "" if nbytes is None else f"  {nbytes / 1e6:9.1f} MB  {gbs:8.1f} GB/s"
        print(f"{name:42s} {ms * 1e3:10.1f} us{tail}", flush=True)

    if a.surface_only:
        surface_rows(report, a.n, a.iters)
        print(json.dumps(res), flush=True)
        return
    pos_np, ei_np = grid_mesh(a.n)
    N, E, f, dim = pos_np.shape[0], ei_np.shape[1], 4, 2
    torch.manual_seed(0)
    pos, ei = torch.from_numpy(pos_np).to(dev), torch.from_numpy(ei_np).to(dev)
    y = torch.randn(N, f, device=dev)
    pred = y + 0.1 * torch.randn(N, f, device=dev)
    mean = torch.tensor([1e5, 3.0, -2.0, 300.0], device=dev)
    std = torch.tensor([3e4, 50.0, 50.0, 20.0], device=dev)
    normals = torch.nn.functional.normalize(torch.randn(N, dim, device=dev), dim=1)
    phys = y * std + mean
    pressure, shear = phys[:, 0].contiguous(), phys[:, 1:3].contiguous()
    gptr = torch.tensor([0, N], dtype=torch.int32, device=dev)
    L = _lib.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    print(f"N={N} E={E} f={f} dim={dim} chunk rows={aero.CHUNK_ROWS}", flush=True)
    res.update({"N": N, "E": E})

    # ---- error sums
    report("eval_sums (ours, op)", timeit(lambda: torch.ops.aerognn.eval_sums(pred, y, mean, std, gptr), a.iters),
           2 * N * f * 4)
    report("metrics (torch composition)", timeit(lambda: torch_metrics(pred, y, mean, std), a.iters))
    # ---- forces: the whole operator (groups the edges by sender on every call), then the kernel alone
    op = lambda: torch.ops.aerognn.aero_forces(pressure, shear, normals, pos, None, ei, gptr, [0.25, 0.0], 1e-2)  # noqa: E731
    force_bytes = N * (4 + 3 * dim * 4 + 8 + 8) + E * (4 + 8 + dim * 4)
    report("aero_forces (ours, op + grouping)", timeit(op, a.iters), force_bytes)
    perm, rowptr = group_by(ei[0], N)
    out = torch.zeros(1, 4, 3, dtype=torch.float64, device=dev)
    area = torch.zeros(N, dtype=torch.float64, device=dev)
    scratch = torch.empty(int(L.agn_aero_forces_temp_bytes(N, 1)), dtype=torch.uint8, device=dev)
    ctr = (ctypes.c_double * 2)(0.25, 0.0)

    def kern():
        rc = L.agn_aero_forces(_lib.F32, N, dim, p(pressure), p(shear), dim, p(normals), dim, p(pos), dim, None, p(ei), E,
                               p(rowptr), p(perm), 1e-2, p(area), ctr, p(gptr), 1, p(out), p(scratch), st)
        assert rc == 0, rc
    report("aero_forces (ours, kernels only)", timeit(kern, a.iters), force_bytes)
    areas_given = area.clone()

    def kern_areas():
        rc = L.agn_aero_forces(_lib.F32, N, dim, p(pressure), p(shear), dim, p(normals), dim, p(pos), dim,
                               p(areas_given), None, 0, None, None, 1e-2, None, ctr, p(gptr), 1, p(out), p(scratch), st)
        assert rc == 0, rc
    report("aero_forces (ours, given areas)", timeit(kern_areas, a.iters), N * (4 + 3 * dim * 4 + 8))
    report("forces (torch composition)", timeit(lambda: torch_forces(pos, ei, normals, pressure, shear), a.iters))
    ours = torch.ops.aerognn.aero_forces(pressure, shear, normals, pos, None, ei, gptr, [], 1e-2)[0][0]
    ref = torch_forces(pos, ei, normals, pressure, shear)
    S = torch.stack([ours[2, 0], ours[2, 1], ours[3, 0]])
    print("ours vs torch composition, |diff| / S:",
          ((torch.stack([ours[0, 0], ours[0, 1], ours[1, 0]]) - ref).abs() / S).tolist(), flush=True)
    # ---- yardsticks on the same machine
    mo, so = torch.empty(f, device=dev), torch.empty(f, device=dev)
    cs = torch.empty(int(L.agn_col_stats_temp_bytes(N, f)), dtype=torch.uint8, device=dev)
    report("agn_col_stats [N, 4] fp32", timeit(lambda: L.agn_col_stats(N, f, p(y), f, p(mo), p(so), 1e-8, p(cs), st), a.iters),
           2 * N * f * 4)
    H = 128
    g0 = torch.randn(E, H, device=dev).to(torch.bfloat16)
    so2 = torch.empty(N, H, dtype=torch.bfloat16, device=dev)
    report("agn_segment_sum [E, 128] bf16", timeit(
        lambda: L.agn_segment_sum(N, H, _lib.BF16, p(rowptr), None, p(g0), H, p(so2), H, 0, st), a.iters),
        (E + N) * H * 2 + N * 4)
    del g0, so2
    surface_rows(report, a.n, a.iters)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
