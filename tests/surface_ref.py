"""Plain numpy fp64 restatement of the surface contract (include/aerognn.h agn_surface_forces,
agn_face_edges): a helper for the tests, not a test. Same operation order as the kernel, every
operation one rounded fp64 + - * / or sqrt (no np.linalg.norm, no dot), per-cell Python loops. Only
the order of the fp64 force sums differs from the kernel's (compared by tolerance)."""
import numpy as np


def cells_of(offsets, conn, k=0):
    """List of per-cell id arrays from (offsets | None, conn, k)."""
    conn = np.asarray(conn)
    if offsets is None:
        return [row for row in conn.reshape(-1, k if k else conn.shape[-1])]
    offsets = np.asarray(offsets)
    return [conn[offsets[c]:offsets[c + 1]] for c in range(len(offsets) - 1)]


def cell_geometry(pos, cells):
    """(areas float64 [C], normals float64 [C, 3]): the fan cross products c_i = d_i x d_{i+1},
    d_i = p_i - p_0; area = sum 0.5 sqrt(c_i . c_i); normal = (sum c_i) / |sum c_i| or 0."""
    pos = np.asarray(pos).astype(np.float64)  # exact widening
    areas = np.zeros(len(cells))
    normals = np.zeros((len(cells), 3))
    for c, ids in enumerate(cells):
        S = [np.float64(0.0)] * 3
        area = np.float64(0.0)
        for i in range(1, len(ids) - 1):
            d1 = [pos[ids[i], x] - pos[ids[0], x] for x in range(3)]
            d2 = [pos[ids[i + 1], x] - pos[ids[0], x] for x in range(3)]
            cr = [d1[1] * d2[2] - d1[2] * d2[1], d1[2] * d2[0] - d1[0] * d2[2], d1[0] * d2[1] - d1[1] * d2[0]]
            area = area + np.float64(0.5) * np.sqrt(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2])
            S = [S[x] + cr[x] for x in range(3)]
        ln = np.sqrt(S[0] * S[0] + S[1] * S[1] + S[2] * S[2])
        areas[c] = area
        if ln != 0.0:
            normals[c] = [S[0] / ln, S[1] / ln, S[2] / ln]
    return areas, normals


def point_to_cell(values, cells, mean=None, std=None):
    """[C, f] in the dtype of values: sum_i (1 / n) v_i in fp64 in connectivity order from 0.0, rounded
    once; with mean / std the point value is v * std rounded, + mean rounded, in the dtype of values."""
    values = np.asarray(values)
    dt = values.dtype
    if mean is not None:
        values = values * np.asarray(std, dtype=dt)   # two separately rounded ops
        values = values + np.asarray(mean, dtype=dt)
    out = np.zeros((len(cells), values.shape[1]), dtype=dt)
    for c, ids in enumerate(cells):
        if len(ids) == 0:
            continue
        w = np.float64(1.0) / np.float64(len(ids))
        s = np.zeros(values.shape[1], dtype=np.float64)
        for v in ids:
            s = s + w * values[v].astype(np.float64)
        out[c] = s.astype(dt)
    return out


def cell_forces(cell, areas, normals):
    """Per cell F [C, 3] float64 from cell values [C, 4] (field dtype), areas and unrounded normals: the
    normal rounded to the field dtype, pn = p * normal rounded once there, F = pn A - tau A in fp64."""
    cell = np.asarray(cell)
    nT = np.asarray(normals).astype(cell.dtype)
    pn = cell[:, 0:1] * nT
    a = np.asarray(areas, dtype=np.float64)[:, None]
    return pn.astype(np.float64) * a - cell[:, 1:4].astype(np.float64) * a


def surface_forces(pos, cells, fields, mean=None, std=None, cgptr=None):
    """(out [G, nset, 2, 3] float64 = sum F, sum |F|; areas; normals; cell values [nset, C, 4])."""
    areas, normals = cell_geometry(pos, cells)
    C = len(cells)
    cgptr = [0, C] if cgptr is None else [int(v) for v in cgptr]
    out = np.zeros((len(cgptr) - 1, len(fields), 2, 3))
    vals = []
    for s, f in enumerate(fields):
        cv = point_to_cell(f, cells, mean, std)
        vals.append(cv)
        F = cell_forces(cv, areas, normals)
        for g in range(len(cgptr) - 1):
            sl = slice(cgptr[g], cgptr[g + 1])
            out[g, s, 0] = F[sl].sum(0)
            out[g, s, 1] = np.abs(F[sl]).sum(0)
    return out, areas, normals, (np.stack(vals) if vals else np.zeros((0, C, 4), np.float32))


def edges_from_faces(cells, n):
    """int64 [2, E]: every cell side in both directions, coalesced and sorted by (row, col)
    (extract_all_edges + to_undirected); a two-point cell has one side, smaller cells none."""
    keys = []
    for ids in cells:
        m = len(ids)
        sides = m if m >= 3 else (1 if m == 2 else 0)
        for i in range(sides):
            u, v = int(ids[i]), int(ids[(i + 1) % m])
            keys += [u * n + v, v * n + u]
    key = np.unique(np.asarray(keys, dtype=np.int64))
    return np.stack([key // n, key % n]).astype(np.int64).reshape(2, -1)


# ------------------------------------------------------------------ the golden, shared by the CPU and GPU tests
def golden_mesh():
    """(arrays, meta, cells) of tests/golden/aero3d_mesh_f32.npz (tools/make_goldens_surface.py)."""
    from golden_util import load
    d, meta = load("aero3d_mesh_f32")
    d = {k: v.numpy() for k, v in d.items()}
    return d, meta, cells_of(d["offsets"], d["conn"])


def check_golden_coefficients(sums_fn):
    """sums_fn(pos, offsets, conn, [true, pred]) -> [2 sets, 2, 3] float64 (sum F, sum |F|), against the
    reference's six numbers at aero_cases.COEF_TOL['f32']: |got - ref| <= 4 * 2^-24 * S, S the sum of the
    absolute contributions normalised like the coefficient."""
    import aero_cases
    d, meta, _ = golden_mesh()
    den = [meta["reference_area"] * meta["dynamic_pressure"]] * 3
    sums = np.asarray(sums_fn(d["pos"], d["offsets"], d["conn"], [d["true"], d["pred"]]))
    assert sums.shape == (2, 2, 3)
    for s, key in enumerate(("coef_true", "coef_pred")):
        out = np.zeros((4, 3))
        out[0], out[2] = sums[s, 0], sums[s, 1]
        aero_cases.assert_coef(out, d[key], den, aero_cases.COEF_TOL["f32"], (f"aero3d_mesh_f32 {key}", aero_cases.SLOTS_3D))


# ------------------------------------------------------------------ shared meshes
def box_mesh():
    """The box (0|2, 0|1, 0|0.5): four faces as quads, two split into triangles, outward winding, in CSR
    form. Dyadic coordinates: every area, normal and their products are exact in fp64."""
    X, Y, Z = 2.0, 1.0, 0.5
    pos = np.array([[x, y, z] for z in (0.0, Z) for y in (0.0, Y) for x in (0.0, X)])  # id = 4 z + 2 y + x
    cells = [np.array(c) for c in ([0, 2, 3, 1],            # z = 0, normal -z
                                   [4, 5, 7, 6],            # z = Z, normal +z
                                   [0, 1, 5, 4],            # y = 0, normal -y
                                   [2, 6, 7, 3],            # y = Y, normal +y
                                   [0, 4, 6], [0, 6, 2],    # x = 0, normal -x
                                   [1, 3, 7], [1, 7, 5])]   # x = X, normal +x
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in cells])]).astype(np.int64)
    return pos, offsets, np.concatenate(cells).astype(np.int64), cells


def merge_pairs(tri, every=4):
    """lattice_faces' triangle pairs with every `every`-th pair merged into the quad
    (nid, nid_below, right_below, right): a mixed list, CSR (offsets, conn)."""
    cells = []
    for q in range(tri.shape[0] // 2):
        t1, t2 = tri[2 * q], tri[2 * q + 1]
        if q % every == 0:
            cells.append(np.array([t1[0], t2[1], t2[2], t1[2]]))
        else:
            cells += [t1, t2]
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in cells])]).astype(np.int64)
    return offsets, np.concatenate(cells).astype(np.int64)
