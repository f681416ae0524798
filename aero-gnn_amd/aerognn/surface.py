"""3-D surface evaluation from points and a face list, on the device.

For the Ahmed body the reference reads the case's .vtp again and runs three VTK filters on the host
(inference.py:310-320: compute_normals(cell_normals=True), compute_cell_sizes(area=True),
point_data_to_cell_data) before calculate_aero_coefficients_3d (utils.py:385-448); its readers build
the graph from the same surface with extract_all_edges + to_undirected (utils.py:75-81, :111-117).
Here a mesh that arrives as pos [N, 3] plus faces needs no host pass:

  faces_csr(faces, device)                      -> (offsets | None, conn, k) on the device
  cell_geometry(pos, faces)                     -> (areas float64 [C], normals float64 [C, 3])
  point_to_cell(values, faces)                  -> cell means [C, f] (a list for a list)
  integrate_surface(pos, faces, fields, ...)    -> SurfaceSums (force sums per graph and field set)
  edges_from_faces(faces, num_nodes)            -> int64 [2, E], to_undirected's coalesced order

All but faces_csr run torch.ops.aerognn.surface_forces (agn_surface_forces: ONE pass over the cells) or
agn_face_edges. Contract, rounding and the bitwise relation to aero_forces: include/aerognn.h and
DESIGN.md §7d.

Face lists come in three formats: an integer [C, k] tensor (k points per cell), an (offsets [C + 1],
connectivity) pair, or VTK's flat list [n0, i.., n1, i.., ...] (pyvista's `surface.faces`), which is
parsed with numpy on the host, once per mesh. Node ids are global: in a collated batch they already
carry the node offsets. The faces must be consistently wound; VTK's consistent_normals traversal,
point normals (which split points at sharp edges) and cell_data_to_point_data are not reproduced.
Tensors must live on the device: there is no CPU fallback.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch

from . import ops as _ops  # noqa: F401  (registers torch.ops.aerognn.*)
from .core import require_device

I64 = torch.int64

SurfaceSums = namedtuple("SurfaceSums", "force abs_force areas normals cells")


def _is_pair(faces) -> bool:
    return (isinstance(faces, (tuple, list)) and len(faces) == 2
            and all(torch.is_tensor(a) or isinstance(a, np.ndarray) for a in faces)
            and all(a.ndim == 1 for a in faces))


def _parse_vtk_flat(flat: np.ndarray):
    """[n0, i.., n1, i.., ...] -> (offsets [C + 1], conn) as int64 numpy arrays."""
    flat = np.asarray(flat).astype(np.int64, copy=False).reshape(-1)
    if flat.size == 0:
        return np.zeros(1, np.int64), np.zeros(0, np.int64)
    n0 = int(flat[0])
    if n0 >= 0 and flat.size % (n0 + 1) == 0 and np.all(flat.reshape(-1, n0 + 1)[:, 0] == n0):
        c = flat.size // (n0 + 1)  # one cell size throughout: no walk needed
        return np.arange(c + 1, dtype=np.int64) * n0, np.ascontiguousarray(flat.reshape(-1, n0 + 1)[:, 1:]).reshape(-1)
    starts, i = [], 0
    while i < flat.size:
        m = int(flat[i])
        if m < 0 or i + 1 + m > flat.size:
            raise ValueError("faces: malformed VTK face list")
        starts.append(i)
        i += 1 + m
    starts = np.asarray(starts, dtype=np.int64)
    counts = flat[starts]
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    keep = np.ones(flat.size, dtype=bool)
    keep[starts] = False
    return offsets, flat[keep]


def faces_csr(faces, device):
    """The three face-list formats as (offsets | None, conn, k) on `device`, int64: a [C, k] list gives
    (None, conn [C, k], k); an (offsets, connectivity) pair and a VTK flat list give (offsets [C + 1],
    conn [nconn], 0)."""
    if _is_pair(faces):
        off, conn = (torch.as_tensor(a).to(device=device, dtype=I64).contiguous() for a in faces)
        if off.numel() < 1:
            raise ValueError("faces: offsets must have C + 1 entries")
        return off, conn, 0
    t = torch.as_tensor(faces) if not torch.is_tensor(faces) else faces
    if t.is_floating_point() or t.dtype == torch.bool:
        raise TypeError("faces: an integer face list is required")
    if t.dim() == 2:
        return None, t.to(device=device, dtype=I64).contiguous(), int(t.shape[1])
    if t.dim() == 1:
        off, conn = _parse_vtk_flat(t.detach().cpu().numpy())
        return torch.from_numpy(off).to(device), torch.from_numpy(np.ascontiguousarray(conn)).to(device), 0
    raise ValueError("faces: expected [C, k], an (offsets, connectivity) pair or a VTK flat list")


def num_cells(offsets, conn) -> int:
    return int(conn.shape[0]) if offsets is None else int(offsets.numel()) - 1


def _device_faces(faces, device):
    """faces_csr after the no-CPU-fallback rule: tensors of the face list must already be on the device
    (a numpy array or a Python list is an input format and is uploaded)."""
    parts = faces if isinstance(faces, (tuple, list)) else (faces,)
    require_device(*[p for p in parts if torch.is_tensor(p)])
    return faces_csr(faces, device)


def _cell_ptr(cell_batch, ncell, device, ngraph):
    from .aero import graph_ptr
    return graph_ptr(cell_batch, ncell, device, ngraph)


def cell_geometry(pos, faces):
    """(areas float64 [C], normals float64 [C, 3]) of consistently wound faces: the fan-triangulation
    area of vtkCellSizeFilter and the unit normal in the direction of vtkPolygon::ComputeNormal, in fp64
    from pos (fp32 or fp64) widened exactly. Cells with fewer than three points, and cells whose cross
    products cancel, get area 0 / a zero normal."""
    require_device(pos)
    off, conn, _ = _device_faces(faces, pos.device)
    cg = _cell_ptr(None, num_cells(off, conn), pos.device, None)
    _, areas, normals, _ = torch.ops.aerognn.surface_forces(pos, off, conn, [], None, None, cg, True)
    return areas, normals


def _pad4(v):
    if v.dim() == 1:
        v = v[:, None]
    if v.dim() != 2 or not 1 <= v.shape[1] <= 4:
        raise ValueError("point fields must be [N, f] with f <= 4 per set")
    return v if v.shape[1] == 4 else torch.nn.functional.pad(v, (0, 4 - v.shape[1]))


def point_to_cell(values, faces):
    """vtkPointDataToCellData: per cell the mean of its points' values, sum_i (1 / n) v_i in fp64 in
    connectivity order, rounded once to the dtype of `values` ([N, f], f <= 4; or a list of up to four
    such tensors, which gives a list). A cell without points gets 0."""
    sets = list(values) if isinstance(values, (list, tuple)) else [values]
    require_device(*sets)
    dev = sets[0].device
    off, conn, _ = _device_faces(faces, dev)
    cg = _cell_ptr(None, num_cells(off, conn), dev, None)
    widths = [1 if v.dim() == 1 else v.shape[1] for v in sets]
    cells = torch.ops.aerognn.surface_forces(None, off, conn, [_pad4(v) for v in sets], None, None, cg, True)[3]
    out = [cells[s, :, :w] for s, w in enumerate(widths)]
    out = [o[:, 0] if v.dim() == 1 else o for o, v in zip(out, sets)]
    return out if isinstance(values, (list, tuple)) else out[0]


def integrate_surface(pos, faces, fields, stats=None, cell_batch=None, ngraph=None, return_cells=False) -> SurfaceSums:
    """Force sums of a 3-D surface given as points and faces, one pass over the cells.

    fields: one [N, 4] tensor (pressure, tau_x, tau_y, tau_z at the points) or a list of up to four; with
    stats (the reference's norm_stats: 'target_mean', 'target_std', the first four entries) the point
    values are de-normalised first, v * std + mean as inference.py:77-82. Per cell F = p n A - tau A from
    the point-to-cell means, the cell normal and the cell area. cell_batch (int64 [C], sorted) assigns the
    cells to graphs; None is one graph. Returns SurfaceSums: force and abs_force [G, nset, 3] float64
    (the sum of |F| is the scale an error of the signed sum is judged against) and, with return_cells,
    areas float64 [C], normals float64 [C, 3] and cells [nset, C, 4] (None otherwise)."""
    sets = list(fields) if isinstance(fields, (list, tuple)) else [fields]
    require_device(pos, cell_batch, *sets)
    dev = pos.device
    off, conn, _ = _device_faces(faces, dev)
    cg = _cell_ptr(cell_batch, num_cells(off, conn), dev, ngraph)
    mean = std = None
    if stats is not None:
        mean = torch.as_tensor(stats["target_mean"]).to(dev).reshape(-1)[:4]
        std = torch.as_tensor(stats["target_std"]).to(dev).reshape(-1)[:4]
    out, areas, normals, cells = torch.ops.aerognn.surface_forces(pos, off, conn, sets, mean, std, cg, bool(return_cells))
    if not return_cells:
        areas = normals = cells = None
    return SurfaceSums(out[:, :, 0], out[:, :, 1], areas, normals, cells)


def edges_from_faces(faces, num_nodes: int, device=None) -> torch.Tensor:
    """The reference readers' graph from a face list (utils.py:75-81, :111-117): every cell side in both
    directions, int64 [2, E] ascending by (row, col) without duplicates, which is what
    to_undirected(edge_index, num_nodes=N) returns. A two-point cell has one side, a repeated vertex
    gives one self-loop. Reads the edge count back once."""
    from ._lib import check, lib, ptr
    from .core import stream
    if device is None:
        first = faces[0] if isinstance(faces, (tuple, list)) and len(faces) else faces
        device = first.device if torch.is_tensor(first) else torch.device("cuda")
    off, conn, k = _device_faces(faces, device)
    require_device(conn)
    n, ncell, nconn = int(num_nodes), num_cells(off, conn), conn.numel()
    if nconn:
        lo, hi = torch.stack(list(torch.aminmax(conn))).tolist()
        if lo < 0 or hi >= n:
            raise IndexError(f"edges_from_faces: face ids out of range [0, {n})")
    if 2 * nconn > 2 ** 31 - 1:
        raise ValueError("edges_from_faces: more than 2^30 face corners")
    dev = conn.device
    m = 2 * nconn
    out = torch.empty(2, m, dtype=I64, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    scratch = torch.empty(int(lib().agn_face_edges_temp_bytes(nconn)), dtype=torch.uint8, device=dev)
    check(lib().agn_face_edges(n, ncell, ptr(off), ptr(conn), nconn, k, ptr(out), m, ptr(count), ptr(scratch),
                               stream()), "face_edges")
    e = int(count.item())
    return out[:, :e].contiguous()
