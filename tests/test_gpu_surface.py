"""The surface kernels on the MI355X (agn_surface_forces, agn_face_edges through
torch.ops.aerognn.surface_forces and aerognn.surface / aerognn.aero) against tests/surface_ref.py, against
aero_forces on the cell arrays they emit, and against the reference's golden.

Bounds:
  geometry    per cell within 4 * 2^-52, areas relative to the area, normal components relative to 1.
              Every operation is a correctly rounded fp64 + - * / or sqrt in a fixed order with
              contraction off, so 0 is expected; the margin covers a compiler's sqrt / division sequence.
              The measured difference is printed.
  cell values bitwise.
  force sums  within 1e-12 of the absolute-sum scale against the restatement (fp64 sums of the same terms
              in another order); BITWISE against aero_forces on the emitted cell arrays (the same
              reduction); a graph of a batch bitwise the graph alone; two calls identical bytes.
  golden      4 * 2^-24 * S (aero_cases.COEF_TOL['f32']).
  edges       integers: exact.
Shapes: cells of 1, 2, 3, 4, 5 and 7 points and a zero-area triangle; lattice_faces(64, 33) = 4096 cells =
two reduction chunks and 24,576 sort keys; per-graph cell counts R + 1, 0, 65, 0 for the chunk size R."""
import functools
import re
import types

import numpy as np
import pytest
import torch

import aero_cases
import surface_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
GEO_TOL = 4 * 2.0 ** -52
SUM_TOL = 1e-12
MEAN = (1e5, 3.0, -2.0, 1.5)
STD = (3e4, 50.0, 40.0, 20.0)


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def bits(t):
    return t.contiguous().view(torch.int64 if t.element_size() == 8 else torch.int32)


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def run(pos, faces_dev, fields, stats=False, cgptr=None, cells=True):
    """torch.ops.aerognn.surface_forces on device tensors; faces_dev = (offsets | None, conn)."""
    import aerognn.ops  # noqa: F401  (registers the operators)
    off, conn = faces_dev
    ncell = conn.shape[0] if off is None else off.numel() - 1
    g = torch.tensor([0, ncell] if cgptr is None else list(cgptr), dtype=torch.int32, device=DEV)
    mean = std = None
    if stats:
        dt = fields[0].dtype
        mean, std = torch.tensor(MEAN, dtype=dt, device=DEV), torch.tensor(STD, dtype=dt, device=DEV)
    return torch.ops.aerognn.surface_forces(pos, off, conn, list(fields), mean, std, g, cells)


def point_fields(n, nset, np_dtype, seed, physical=True):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(nset):
        f = rng.standard_normal((n, 4))
        if physical:
            f = f * np.array([100.0, 2.0, 2.0, 2.0]) - np.array([20.0, 0, 0, 0])
        out.append(f.astype(np_dtype))
    return out


@functools.lru_cache(maxsize=None)
def mixed_mesh():
    """40 random points; cells of 1, 2, 3, 4, 5 and 7 points, a zero-area triangle (collinear points), an
    empty cell, a cell that repeats a point. CSR."""
    rng = np.random.default_rng(3)
    pos = rng.standard_normal((40, 3))
    pos[10], pos[11], pos[12] = [0, 0, 0], [1, 1, 1], [2, 2, 2]
    cells = [np.array(c, dtype=np.int64) for c in ([5], [6, 7], [0, 1, 2], [3, 4, 8, 9], [13, 14, 15, 16, 17],
                                                    [18, 19, 20, 21, 22, 23, 24], [10, 11, 12], [], [25, 26, 26, 27],
                                                    [39, 0, 38], [30, 31, 32, 33], [1])]
    cells += [rng.choice(40, size=m, replace=False).astype(np.int64) for m in (3, 4, 5, 7, 3, 4)]
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in cells])]).astype(np.int64)
    return pos, offsets, np.concatenate(cells).astype(np.int64), cells


@functools.lru_cache(maxsize=None)
def lattice():
    """ellipsoid(64, 33) and its 4096 triangles."""
    from aerognn.meshgen import ellipsoid, lattice_faces
    m = ellipsoid(64, 33)
    return m, lattice_faces(64, 33)


def check_vs_ref(got, ref, what):
    """(out, areas, normals, cells) of the kernel against surface_ref.surface_forces."""
    out, areas, normals, cells = (t.cpu().numpy() for t in got)
    r_out, r_areas, r_normals, r_cells = ref
    da = np.abs(areas - r_areas) / np.where(r_areas > 0, r_areas, 1.0)
    dn = np.abs(normals - r_normals)
    print(f"{what}: max area rel diff {da.max():.3e}, max normal diff {dn.max():.3e} (bound {GEO_TOL:.3e})")
    assert np.all(da <= GEO_TOL) and np.all(dn <= GEO_TOL), what
    np.testing.assert_array_equal(areas == 0, r_areas == 0, err_msg=what)
    assert cells.dtype == r_cells.dtype and cells.shape == r_cells.shape
    np.testing.assert_array_equal(cells.view(np.uint8), r_cells.view(np.uint8), err_msg=f"{what}: cell values")
    S = r_out[:, :, 1:2, :]
    err = np.abs(out - r_out)
    print(f"{what}: max force err / S {np.max(err / np.maximum(S, 1e-300)):.3e} (bound {SUM_TOL:.0e})")
    assert np.all(err <= SUM_TOL * S), what


# ------------------------------------------------------------------ the kernel against the restatement
@pytest.mark.parametrize("pos_dt,fld_dt,stats", [(np.float32, np.float32, True), (np.float64, np.float64, False),
                                                 (np.float32, np.float64, True), (np.float64, np.float32, False)])
def test_mixed_cells_vs_restatement(pos_dt, fld_dt, stats):
    pos, offsets, conn, cells = mixed_mesh()
    pos = pos.astype(pos_dt)
    fields = point_fields(40, 2, fld_dt, 5, physical=not stats)
    got = run(dev(pos), (dev(offsets), dev(conn)), [dev(f) for f in fields], stats=stats)
    ms = (np.array(MEAN, fld_dt), np.array(STD, fld_dt)) if stats else (None, None)
    ref = surface_ref.surface_forces(pos, cells, fields, *ms)
    check_vs_ref(got, ref, f"mixed cells pos {np.dtype(pos_dt).name} fields {np.dtype(fld_dt).name} stats {stats}")
    areas, normals = got[1].cpu().numpy(), got[2].cpu().numpy()
    for c in (0, 1, 6, 7, 11):                                    # one and two points, collinear, empty
        assert areas[c] == 0 and not normals[c].any()
    assert np.all(areas[[2, 3, 4, 5]] > 0)


def test_box_is_exact_on_the_device():
    from aerognn import surface
    pos, offsets, conn, _ = surface_ref.box_mesh()
    for dt in (torch.float32, torch.float64):
        areas, normals = surface.cell_geometry(dev(pos, dt), (dev(offsets), dev(conn)))
        assert areas.dtype == normals.dtype == torch.float64
        assert float(areas.sum()) == 7.0
        assert not (areas[:, None] * normals).sum(0).any()
        assert torch.equal(normals.abs().sum(1), torch.ones(8, dtype=torch.float64, device=DEV))


def test_lattice_two_chunks_vs_restatement():
    m, tri = lattice()
    fields = point_fields(m["pos"].shape[0], 1, np.float32, 7)
    got = run(dev(m["pos"]), (None, dev(tri)), [dev(f) for f in fields])
    check_vs_ref(got, surface_ref.surface_forces(m["pos"], list(tri), fields), "lattice 4096 cells")


# ------------------------------------------------------------------ the defining equality
def aero_rows(got, s, cgptr, ncell):
    """Rows 0 and 2 of aero_forces on the cell arrays `got` holds for set s: [G, 2, 3]."""
    out, areas, normals, cells = got
    g = torch.tensor([0, ncell] if cgptr is None else list(cgptr), dtype=torch.int32, device=DEV)
    cv = cells[s]
    res = torch.ops.aerognn.aero_forces(cv[:, 0].contiguous(), cv[:, 1:4], normals.to(cv.dtype), None, areas, None, g,
                                        [], 1e-2)[0]
    return res[:, [0, 2]]


@pytest.mark.parametrize("fld_dt", [np.float32, np.float64])
@pytest.mark.parametrize("stats", [False, True])
def test_sums_are_bitwise_aero_forces_on_the_emitted_cells(fld_dt, stats):
    m, tri = lattice()
    R = aero_chunk()
    sizes = [R + 1, 0, 65, 0]
    cgptr = np.concatenate([[0], np.cumsum(sizes)])
    fields = [dev(f) for f in point_fields(m["pos"].shape[0], 2, fld_dt, 11, physical=not stats)]
    for faces, gp, what in (((None, dev(tri)), None, "one graph, 4096 cells"),
                            ((None, dev(tri[:cgptr[-1]])), cgptr, "batch R + 1, 0, 65, 0")):
        got = run(dev(m["pos"]), faces, fields, stats=stats, cgptr=gp)
        ncell = faces[1].shape[0]
        for s in range(2):
            assert same_bytes(got[0][:, s], aero_rows(got, s, gp, ncell)), f"{what}, set {s}"
    # mixed cells too: the equality does not depend on the cell shapes
    pos, offsets, conn, cells = mixed_mesh()
    f = [dev(x) for x in point_fields(40, 1, fld_dt, 13, physical=not stats)]
    got = run(dev(pos), (dev(offsets), dev(conn)), f, stats=stats)
    assert same_bytes(got[0][:, 0], aero_rows(got, 0, None, len(cells)))


def aero_chunk():
    from aerognn import aero
    return aero.CHUNK_ROWS


# ------------------------------------------------------------------ shapes
def test_regular_and_csr_forms_give_identical_bytes():
    m, tri = lattice()
    pos = dev(m["pos"])
    fields = [dev(f) for f in point_fields(pos.shape[0], 2, np.float32, 17)]
    quads = np.stack([tri[0::2, 0], tri[1::2, 1], tri[1::2, 2], tri[0::2, 2]], 1)   # every pair merged
    for reg in (tri, quads):
        k = reg.shape[1]
        a = run(pos, (None, dev(reg)), fields, stats=True)
        b = run(pos, (dev(np.arange(reg.shape[0] + 1, dtype=np.int64) * k), dev(reg.reshape(-1))), fields, stats=True)
        for x, y in zip(a, b):
            assert same_bytes(x, y), f"[C, {k}] against CSR"
    # a quad is its two triangles: the same total area
    ta = run(pos, (None, dev(tri)), [], cells=True)[1]
    qa = run(pos, (None, dev(quads)), [], cells=True)[1]
    assert torch.equal(qa, ta[0::2] + ta[1::2])


def test_strided_pos_mixed_dtypes_and_16_bit():
    pos, offsets, conn, cells = mixed_mesh()
    faces = (dev(offsets), dev(conn))
    f32 = [dev(f) for f in point_fields(40, 1, np.float32, 19)]
    f64 = [f.double() for f in f32]
    wide = torch.zeros(40, 6, device=DEV)
    wide[:, 2:5] = dev(pos, torch.float32)
    sl = wide[:, 2:5]
    assert not sl.is_contiguous() and sl.stride(0) == 6
    ref = run(sl.contiguous(), faces, f32)
    for x, y in zip(run(sl, faces, f32), ref):
        assert same_bytes(x, y), "pos_ld = 6"
    # a column slice of a wider field tensor
    fw = torch.zeros(40, 9, device=DEV)
    fw[:, 3:7] = f32[0]
    for x, y in zip(run(sl, faces, [fw[:, 3:7]]), ref):
        assert same_bytes(x, y), "field_ld = 9"
    # fp32 positions with fp64 fields: taken as they are; the geometry is fp64 from the exact widening
    for x, y in zip(run(sl, faces, f64), run(sl.double(), faces, f64)):
        assert same_bytes(x, y), "fp32 pos, fp64 fields"
    # bf16 inputs are widened to fp32 (exact)
    pb, fb = sl.bfloat16(), f32[0].bfloat16()
    for x, y in zip(run(pb, faces, [fb]), run(pb.float(), faces, [fb.float()])):
        assert same_bytes(x, y), "bf16 widened"
    with pytest.raises(IndexError):
        run(sl, (None, torch.tensor([[0, 1, 40]], device=DEV)), f32)
    with pytest.raises(IndexError):
        run(sl, (None, torch.tensor([[0, -1, 2]], device=DEV)), f32)


def test_batch_independent_and_repeatable():
    """Per-graph cell counts R + 1, 0, 65, 0 cut from the 4096 triangles: every graph's sums are bitwise
    the sums of its cells alone, empty graphs give zeros, two calls give identical bytes."""
    from aerognn import surface
    m, tri = lattice()
    R = aero_chunk()
    sizes = [R + 1, 0, 65, 0]
    cgptr = np.concatenate([[0], np.cumsum(sizes)])
    pos = dev(m["pos"])
    fields = [dev(f) for f in point_fields(pos.shape[0], 2, np.float32, 23, physical=False)]
    faces = dev(tri[:cgptr[-1]])
    got = run(pos, (None, faces), fields, stats=True, cgptr=cgptr)
    again = run(pos, (None, faces), fields, stats=True, cgptr=cgptr)
    for x, y in zip(got, again):
        assert same_bytes(x, y)
    assert not got[0][1].any() and not got[0][3].any()
    for g in (0, 2):
        a, b = int(cgptr[g]), int(cgptr[g + 1])
        alone = run(pos, (None, faces[a:b]), fields, stats=True)
        assert same_bytes(got[0][g], alone[0][0]), f"graph {g} differs from the graph alone"
        assert same_bytes(got[1][a:b], alone[1]) and same_bytes(got[3][:, a:b], alone[3])
    # the same through the public entry, from a cell batch vector
    batch = torch.repeat_interleave(torch.arange(4, device=DEV), torch.tensor(sizes, device=DEV))
    stats = {"target_mean": torch.tensor(MEAN), "target_std": torch.tensor(STD)}
    ss = surface.integrate_surface(pos, faces, fields, stats=stats, cell_batch=batch, ngraph=4, return_cells=True)
    assert same_bytes(ss.force, got[0][:, :, 0]) and same_bytes(ss.abs_force, got[0][:, :, 1])
    assert same_bytes(ss.areas, got[1]) and same_bytes(ss.normals, got[2]) and same_bytes(ss.cells, got[3])
    assert surface.integrate_surface(pos, faces, fields[0], stats=stats).areas is None


def test_zero_and_four_sets_and_the_helpers():
    from aerognn import surface
    pos, offsets, conn, cells = mixed_mesh()
    faces = (dev(offsets), dev(conn))
    p = dev(pos)
    out, areas, normals, cv = run(p, faces, [])
    assert out.shape == (1, 0, 2, 3) and cv.shape == (0, len(cells), 4)
    r_areas, r_normals = surface_ref.cell_geometry(pos, cells)
    assert np.all(np.abs(areas.cpu().numpy() - r_areas) <= GEO_TOL * np.maximum(r_areas, 1e-300))
    assert np.all(np.abs(normals.cpu().numpy() - r_normals) <= GEO_TOL)
    ga, gn = surface.cell_geometry(p, faces)
    assert same_bytes(ga, areas) and same_bytes(gn, normals)
    fields = point_fields(40, 4, np.float64, 29)
    got = run(p, faces, [dev(f) for f in fields])
    assert got[0].shape == (1, 4, 2, 3) and got[3].shape == (4, len(cells), 4)
    check_vs_ref(got, surface_ref.surface_forces(pos, cells, fields), "four sets")
    # set s of a four-set call is the one-set call, bitwise
    for s in (0, 3):
        one = run(p, faces, [dev(fields[s])])
        assert same_bytes(one[0][:, 0], got[0][:, s]) and same_bytes(one[3][0], got[3][s])
    # point_to_cell: the means alone, narrower sets padded
    v3 = dev(fields[1][:, :3])
    c3, c1 = surface.point_to_cell([v3, dev(fields[2][:, 0])], faces)
    assert c3.shape == (len(cells), 3) and c1.shape == (len(cells),)
    np.testing.assert_array_equal(c3.cpu().numpy(), surface_ref.point_to_cell(fields[1][:, :3], cells))
    np.testing.assert_array_equal(c1.cpu().numpy(), surface_ref.point_to_cell(fields[2][:, :1], cells)[:, 0])
    assert same_bytes(surface.point_to_cell(dev(fields[0]), faces), got[3][0])
    # no cells: zeros, no launch
    e = run(p, (None, torch.zeros(0, 3, dtype=torch.int64, device=DEV)), [dev(fields[0])])
    assert e[0].shape == (1, 1, 2, 3) and not e[0].any() and e[1].numel() == 0


# ------------------------------------------------------------------ the reference's golden
def test_coefficients_3d_mesh_vs_golden():
    from aerognn import aero
    d, meta, _ = surface_ref.golden_mesh()
    kw = dict(reference_area=meta["reference_area"], dynamic_pressure=meta["dynamic_pressure"])

    def sums(pos, off, conn, fields):
        c = aero.coefficients_3d_mesh(dev(pos), (dev(off), dev(conn)), [dev(f) for f in fields], **kw)
        den = kw["reference_area"] * kw["dynamic_pressure"]
        F = np.stack([c["CA"][0], c["CN"][0], c["CY"][0]], 1) * den          # [nset, 3]
        S = np.stack([c["S_CA"][0], c["S_CN"][0], c["S_CY"][0]], 1) * den
        return np.stack([F, S], 1)
    surface_ref.check_golden_coefficients(sums)
    # the reference-named function: its six keys, the golden's numbers at the same bound
    faces = (dev(d["offsets"]), dev(d["conn"]))
    c = aero.calculate_aero_coefficients_3d_mesh(dev(d["pos"]), faces, dev(d["true"]), dev(d["pred"]), **kw)
    assert list(c) == ["CA_true", "CN_true", "CY_true", "CA_pred", "CN_pred", "CY_pred"]
    assert all(isinstance(v, float) for v in c.values())
    s = aero.coefficients_3d_mesh(dev(d["pos"]), faces, [dev(d["true"]), dev(d["pred"])], **kw)
    for j, nm in enumerate(("true", "pred")):
        for k, key in enumerate(("CA", "CN", "CY")):
            assert abs(c[f"{key}_{nm}"] - float(d[f"coef_{nm}"][k])) <= aero_cases.COEF_TOL["f32"] * s["S_" + key][0, j]
    # the VTK flat list of the same mesh gives the same bytes
    flat = np.concatenate([np.concatenate([[len(x)], x]) for x in surface_ref.cells_of(d["offsets"], d["conn"])])
    assert c == aero.calculate_aero_coefficients_3d_mesh(dev(d["pos"]), flat, dev(d["true"]), dev(d["pred"]), **kw)
    # normalised fields + stats = the physical fields, when the de-normalisation is exact
    stats = {"target_mean": torch.zeros(4), "target_std": torch.full((4,), 4.0)}
    c4 = aero.calculate_aero_coefficients_3d_mesh(dev(d["pos"]), faces, dev(d["true"] / 4), dev(d["pred"] / 4),
                                                  stats=stats, **kw)
    assert c4 == c


# ------------------------------------------------------------------ edges_from_faces
def test_edges_from_faces():
    from aerognn import surface
    m, tri = lattice()

    def check(cells, n, faces, what):
        got = surface.edges_from_faces(faces, n)
        assert got.dtype == torch.int64 and got.dim() == 2 and got.shape[0] == 2 and got.is_contiguous(), what
        np.testing.assert_array_equal(got.cpu().numpy(), surface_ref.edges_from_faces(cells, n), err_msg=what)
        return got
    pos, offsets, conn, cells = surface_ref.box_mesh()
    check(cells, 8, (dev(offsets), dev(conn)), "box")
    d, _, gcells = surface_ref.golden_mesh()
    check(gcells, d["pos"].shape[0], (dev(d["offsets"]), dev(d["conn"])), "golden mixed list")
    odd = [np.array(c, dtype=np.int64) for c in ([0, 1, 2], [2, 1, 0], [0, 1, 2], [3, 4], [4], [], [1, 1, 3], [5, 6, 7, 8, 9])]
    off = np.concatenate([[0], np.cumsum([len(c) for c in odd])]).astype(np.int64)
    got = check(odd, 11, (dev(off), dev(np.concatenate(odd))), "duplicated, reversed, repeated vertex")
    assert [1, 1] in got.T.tolist() and [3, 4] in got.T.tolist() and 10 not in got
    # 24,576 keys: more than one block of the sort; the generator's own graph
    got = check(list(tri), 64 * 33, dev(tri), "lattice_faces(64, 33)")
    np.testing.assert_array_equal(got.cpu().numpy(), m["edge_index"])
    assert same_bytes(got, surface.edges_from_faces(dev(tri), 64 * 33))
    # the regular form and the VTK flat list of the same cells
    flat = np.concatenate([np.full((tri.shape[0], 1), 3), tri], 1).reshape(-1)
    assert same_bytes(got, surface.edges_from_faces(flat, 64 * 33))
    e = surface.edges_from_faces(torch.zeros(0, 3, dtype=torch.int64, device=DEV), 5)
    assert e.shape == (2, 0) and e.dtype == torch.int64
    with pytest.raises(IndexError):
        surface.edges_from_faces(dev(tri), 64 * 33 - 1)


# ------------------------------------------------------------------ DeviceEvaluator, ahmed_body
class _Case(types.SimpleNamespace):
    def to(self, device):
        return _Case(**{k: (v.to(device) if torch.is_tensor(v) else v) for k, v in vars(self).items()})


NUM = aero_cases.NUM
AHMED_RE = (rf" \| CA:(?P<ca_p>{NUM}) \((?P<ca_t>{NUM})\) \| CN:(?P<cn_p>{NUM}) \((?P<cn_t>{NUM})\) "
            rf"\| CY:(?P<cy_p>{NUM}) \((?P<cy_t>{NUM})\)")


def fmt(c):
    return (f" | CA:{c['CA_pred']:7.4f} ({c['CA_true']:7.4f}) | CN:{c['CN_pred']:7.4f} ({c['CN_true']:7.4f}) "
            f"| CY:{c['CY_pred']:7.4f} ({c['CY_true']:7.4f})")


def test_device_evaluator_ahmed_body():
    from aerognn import aero, surface
    from aerognn.meshgen import ellipsoid, lattice_faces
    from models.mgn import MeshGraphNet
    m = ellipsoid(12, 8)
    tri = torch.from_numpy(lattice_faces(12, 8))
    torch.manual_seed(0)
    model = MeshGraphNet(6, 4, 4, processor_size=1, hidden_dim_processor=32, hidden_dim_node_encoder=32,
                         hidden_dim_edge_encoder=32, hidden_dim_decoder=32, aggregation="add").to(DEV)
    stats = {"target_mean": torch.tensor(MEAN), "target_std": torch.tensor(STD)}
    params = {"dataset": {"name": "ahmed_body", "output_features": ["p", "tau_x", "tau_y", "tau_z"]}}
    base = dict(x=torch.from_numpy(m["x"]), edge_attr=torch.from_numpy(m["edge_attr"]),
                edge_index=torch.from_numpy(m["edge_index"]), pos=torch.from_numpy(m["pos"]), y=torch.from_numpy(m["y"]),
                Velocity=40.0, Height=288.0, Width=389.0, case_no="run_7")
    kw = dict(reference_area=288.0 * 389.0 * 1e-6 / 2, dynamic_pressure=0.5 * 1.225 * 40.0 * 40.0)
    ev = aero.DeviceEvaluator(model, stats, params)
    pos, y = base["pos"].to(DEV), base["y"].to(DEV)
    dstats = {k: v.to(DEV) for k, v in stats.items()}

    # with faces, without cell_y: the true fields are the point-to-cell means of the de-normalised y
    case = _Case(faces=tri, **base)
    pred = ev.predict(case)
    info = ev.evaluate_case(case)
    assert re.fullmatch(AHMED_RE, info["coeff_str"]), info["coeff_str"]
    c = aero.calculate_aero_coefficients_3d_mesh(pos, tri.to(DEV), y, pred, stats=dstats, **kw)
    assert info["coeff_str"] == fmt(c)
    assert info["case_no"] == "run_7"

    # with cell_y: the file's own cell data for the true fields
    rng = np.random.default_rng(41)
    cell_y = torch.from_numpy((rng.standard_normal((tri.shape[0], 4)) * [100, 2, 2, 2]).astype(np.float32))
    info2 = ev.evaluate_case(_Case(faces=tri, cell_y=cell_y, **base))
    assert re.fullmatch(AHMED_RE, info2["coeff_str"]), info2["coeff_str"]
    areas, normals = surface.cell_geometry(pos, tri.to(DEV))
    cy = cell_y.to(DEV)
    ct = aero.calculate_aero_coefficients_3d(areas, normals.float(), cy[:, 0], cy[:, 1:4], **kw)
    c2 = dict(c, CA_true=ct["CA"], CN_true=ct["CN"], CY_true=ct["CY"])
    assert info2["coeff_str"] == fmt(c2) and info2["coeff_str"] != info["coeff_str"]

    # without faces: exactly as before
    info3 = ev.evaluate_case(_Case(**base))
    assert info3["coeff_str"] == ""
    assert info3["rrmse_percent"] == info["rrmse_percent"]
    lines = ev.errors_txt().split("\n")
    assert lines[2].endswith(info["coeff_str"] + " | run_7") and lines[4].endswith(" | run_7")
