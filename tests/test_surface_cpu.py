"""3-D surface evaluation from a face list (aerognn.surface, torch.ops.aerognn.surface_forces,
agn_surface_forces / agn_face_edges) without a GPU: tests/surface_ref.py (the numpy fp64 restatement of
the contract) on shapes whose answers are known exactly and against the reference's golden, the face-list
formats, meshgen.lattice_faces, the C-ABI symbols and their argument errors, the operator's schema and
fake kernel, the no-CPU-fallback rule and the public signatures.
Numerics of the kernels: tests/test_gpu_surface.py."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import surface_ref

NEW_SYMBOLS = ("agn_surface_forces_temp_bytes", "agn_surface_forces", "agn_face_edges_temp_bytes", "agn_face_edges")


# ------------------------------------------------------------------ the restatement on known shapes
def test_box_is_exact():
    """Dyadic coordinates: total area exactly 7, sum area * normal exactly 0, every normal exactly +-e_i."""
    pos, offsets, conn, cells = surface_ref.box_mesh()
    for dt in (np.float64, np.float32):
        areas, normals = surface_ref.cell_geometry(pos.astype(dt), cells)
        assert areas.sum() == 7.0
        np.testing.assert_array_equal((areas[:, None] * normals).sum(0), np.zeros(3))
        expect = np.array([[0, 0, -1], [0, 0, 1], [0, -1, 0], [0, 1, 0], [-1, 0, 0], [-1, 0, 0], [1, 0, 0], [1, 0, 0]], float)
        np.testing.assert_array_equal(normals, expect)
        np.testing.assert_array_equal(areas, [2.0, 2.0, 1.0, 1.0, 0.25, 0.25, 0.25, 0.25])
    assert [len(c) for c in surface_ref.cells_of(offsets, conn)] == [4, 4, 4, 4, 3, 3, 3, 3]


def test_fan_area_is_half_the_newell_norm_on_planar_quads():
    rng = np.random.default_rng(0)
    for _ in range(20):
        o, u, v = rng.standard_normal((3, 3))
        ab = np.array([[0, 0], [1 + rng.random(), 0.1 * rng.random()], [1 + rng.random(), 1 + rng.random()],
                       [0.1 * rng.random(), 1 + rng.random()]])   # a convex quad in plane coordinates
        p = o + ab[:, :1] * u + ab[:, 1:] * v
        area, normal = surface_ref.cell_geometry(p, [np.arange(4)])
        newell = sum(np.cross(p[i], p[(i + 1) % 4]) for i in range(4))
        half = 0.5 * np.sqrt((newell * newell).sum())
        assert abs(area[0] - half) <= 1e-12 * half
        np.testing.assert_allclose(normal[0], newell / np.sqrt((newell * newell).sum()), atol=1e-12)


def test_degenerate_cells():
    """A zero-area triangle and cells of one and two points: area 0 and a zero normal; their cell values
    are still the means of their points; an empty cell gives 0."""
    pos = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2], [0, 1, 0]], dtype=np.float64)
    cells = [np.array([0, 1, 2]), np.array([3]), np.array([0, 3]), np.array([], dtype=np.int64), np.array([0, 1, 3])]
    areas, normals = surface_ref.cell_geometry(pos, cells)
    np.testing.assert_array_equal(areas[:4], 0.0)
    np.testing.assert_array_equal(normals[:4], 0.0)
    assert areas[4] > 0 and abs((normals[4] ** 2).sum() - 1) < 1e-15
    vals = np.array([[1.0], [2.0], [6.0], [5.0]], dtype=np.float32)
    cv = surface_ref.point_to_cell(vals, cells)
    assert cv.dtype == np.float32
    np.testing.assert_array_equal(cv[:, 0], np.array([3.0, 5.0, 3.0, 0.0, (1 / 3 + 2 / 3) + 5 / 3], dtype=np.float32))
    out = surface_ref.surface_forces(pos, cells[:4], [np.ones((4, 4), np.float32)])[0]
    assert not out.any()


# ------------------------------------------------------------------ the golden
def test_golden_cell_arrays_are_the_restatement_s_bitwise():
    d, meta, cells = surface_ref.golden_mesh()
    assert sorted(set(len(c) for c in cells)) == [3, 4]                      # a mixed list
    assert d["areas"].dtype == np.float64 and d["normals"].dtype == np.float32 and d["p"].dtype == np.float32
    areas, normals = surface_ref.cell_geometry(d["pos"], cells)
    np.testing.assert_array_equal(areas, d["areas"])
    np.testing.assert_array_equal(normals.astype(np.float32), d["normals"])
    for fld, p, sh in (("true", "p", "shear"), ("pred", "p_pred", "shear_pred")):
        cv = surface_ref.point_to_cell(d[fld], cells)
        np.testing.assert_array_equal(cv[:, 0], d[p])
        np.testing.assert_array_equal(cv[:, 1:4], d[sh])


def test_restatement_coefficients_vs_golden():
    surface_ref.check_golden_coefficients(
        lambda pos, off, conn, fields: surface_ref.surface_forces(pos, surface_ref.cells_of(off, conn), fields)[0][0])


# ------------------------------------------------------------------ meshgen.lattice_faces, faces_csr
@pytest.mark.parametrize("nu,nv", [(12, 8), (7, 3), (5, 2)])
def test_lattice_faces_edges_are_the_generator_s_graph(nu, nv):
    from aerognn.meshgen import ellipsoid, lattice_faces
    m = ellipsoid(nu, nv)
    tri = lattice_faces(nu, nv)
    assert tri.shape == (2 * nu * (nv - 1), 3) and tri.dtype == np.int64
    np.testing.assert_array_equal(surface_ref.edges_from_faces(list(tri), nu * nv), m["edge_index"])
    areas, normals = surface_ref.cell_geometry(m["pos"], list(tri))
    assert np.all(areas > 0)
    node_n = m["normals"].astype(np.float64)
    for j in range(3):                                                       # outward: along the node normals
        assert np.all((normals * node_n[tri[:, j]]).sum(1) > 0.5)


def test_faces_csr_formats_agree():
    from aerognn.surface import faces_csr, num_cells
    tri = np.array([[0, 1, 2], [2, 1, 3], [3, 1, 4]], dtype=np.int64)
    offsets = np.array([0, 3, 6, 9], dtype=np.int64)
    flat = np.concatenate([np.concatenate([[3], t]) for t in tri])
    o_reg, c_reg, k = faces_csr(torch.from_numpy(tri).int(), "cpu")
    assert o_reg is None and k == 3 and c_reg.dtype == torch.int64 and num_cells(o_reg, c_reg) == 3
    for faces in ((torch.from_numpy(offsets), torch.from_numpy(tri.reshape(-1))), (offsets, tri.reshape(-1)), flat,
                  torch.from_numpy(flat), flat.tolist()):
        o, c, kk = faces_csr(faces, "cpu")
        assert kk == 0 and o.dtype == torch.int64 and c.dtype == torch.int64 and num_cells(o, c) == 3
        np.testing.assert_array_equal(o.numpy(), np.arange(4) * k)           # what the regular form means
        np.testing.assert_array_equal(c.numpy(), c_reg.reshape(-1).numpy())
    # a mixed VTK list (the walk, not the uniform shortcut), the golden's list among them
    d, _, cells = surface_ref.golden_mesh()
    flat = np.concatenate([np.concatenate([[len(c)], c]) for c in cells])
    o, c, _ = faces_csr(flat, "cpu")
    np.testing.assert_array_equal(o.numpy(), d["offsets"])
    np.testing.assert_array_equal(c.numpy(), d["conn"])
    mixed = [2, 0, 1, 1, 5, 4, 0, 1, 2, 3, 0]
    o, c, _ = faces_csr(mixed, "cpu")
    assert o.tolist() == [0, 2, 3, 7, 7] and c.tolist() == [0, 1, 5, 0, 1, 2, 3]
    with pytest.raises(ValueError):
        faces_csr([3, 0, 1], "cpu")
    with pytest.raises(TypeError):
        faces_csr(torch.zeros(3, 3), "cpu")


def test_edges_restatement_rules():
    """One side for a two-point cell, none below, one self-loop for a repeated vertex, duplicates and
    reversed cells coalesced."""
    cells = [np.array([0, 1, 2]), np.array([2, 1, 0]), np.array([0, 1, 2]), np.array([3, 4]), np.array([4]),
             np.array([], dtype=np.int64), np.array([1, 1, 3])]
    e = surface_ref.edges_from_faces(cells, 5)
    assert [tuple(c) for c in e.T] == [(0, 1), (0, 2), (1, 0), (1, 1), (1, 2), (1, 3), (2, 0), (2, 1), (3, 1), (3, 4), (4, 3)]
    assert surface_ref.edges_from_faces([], 5).shape == (2, 0)


# ------------------------------------------------------------------ the C ABI
def test_symbols_declared_and_exported():
    from aerognn import _lib
    names = _lib.exported_symbols()
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for sym in NEW_SYMBOLS:
        assert sym in names
        assert getattr(cdll, sym) is not None
        assert getattr(_lib.lib(), sym) is not None
    hdr = open(os.path.join(os.path.dirname(_lib.__file__), "..", "..", "include", "aerognn.h")).read()
    for ref in ("inference.py:310-320", "utils.py:75-81", "utils.py:385-448"):
        assert ref in hdr


def test_scratch_sizes():
    from aerognn import _lib
    L = _lib.lib()
    R = L.agn_aero_chunk_rows()
    for c, g, s in ((1, 1, 1), (R, 1, 2), (R + 1, 3, 4), (10 * R + 7, 4, 0)):
        cap = (c + R - 1) // R + g
        assert L.agn_surface_forces_temp_bytes(c, g, s) >= 8 * cap * 6 * s + 4 * (2 * g + 1)
    assert L.agn_surface_forces_temp_bytes(10, 1, 5) == 0 and L.agn_surface_forces_temp_bytes(-1, 1, 1) == 0
    for nconn in (0, 3, 12288):
        assert L.agn_face_edges_temp_bytes(nconn) >= 2 * nconn * (8 + 8 + 4 + 4)
    assert L.agn_face_edges_temp_bytes(2 ** 30) == 0 and L.agn_face_edges_temp_bytes(-1) == 0


def test_argument_errors_need_no_device():
    from aerognn import _lib
    L = _lib.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    fields = (ctypes.c_void_p * 4)(p.value, p.value, p.value, p.value)
    lds = (ctypes.c_int * 4)(4, 4, 4, 4)

    def sf(pdt=_lib.F32, n=4, pos=p, pos_ld=3, ncell=1, offsets=None, conn=p, nconn=3, k=3, fdt=_lib.F32, nset=1,
           fl=fields, ld=lds, mean=None, std=None, cgptr=p, out=p, area=None, scratch=p):
        return L.agn_surface_forces(pdt, n, pos, pos_ld, ncell, offsets, conn, nconn, k, fdt, nset, fl, ld, mean, std,
                                    cgptr, 1, out, area, None, None, scratch, None)
    assert sf(n=-1) == -1 and sf(ncell=-1) == -1 and sf(nconn=-1) == -1      # AGN_E_ARG: negative counts
    assert sf(cgptr=None) == -1 and sf(conn=None) == -1 and sf(out=None) == -1 and sf(scratch=None) == -1
    assert sf(fl=None) == -1                                                 # field sets named, none given
    assert sf(fl=(ctypes.c_void_p * 4)(p.value, None, None, None), nset=2) == -1
    assert sf(pos=None, area=p) == -1                                        # areas asked for without pos
    assert sf(pdt=_lib.BF16) == -2 and sf(fdt=_lib.F16) == -2 and sf(pdt=_lib.F16, fdt=_lib.BF16) == -2
    assert sf(nset=5) == -4 and sf(nset=-1) == -4                            # AGN_E_SHAPE
    assert sf(pos_ld=2) == -4
    assert sf(ld=(ctypes.c_int * 4)(3, 4, 4, 4)) == -4                       # a field row narrower than 4
    assert sf(mean=p) == -4                                                  # mean without std
    assert sf(ncell=2) == -4                                                 # ncell * k > nconn
    assert sf(n=0) == -4                                                     # points named, none given
    assert sf(ncell=0, cgptr=None, conn=None, nconn=0, scratch=None) == 0    # C == 0: no launch

    def fe(n=4, ncell=1, conn=p, nconn=3, k=3, out=p, out_ld=6, ecount=p, scratch=p):
        return L.agn_face_edges(n, ncell, None, conn, nconn, k, out, out_ld, ecount, scratch, None)
    assert fe(n=-1) == -1 and fe(ncell=-1) == -1 and fe(nconn=-1) == -1 and fe(ecount=None) == -1
    assert fe(conn=None) == -1 and fe(out=None) == -1 and fe(scratch=None) == -1
    assert fe(nconn=2 ** 30) == -4 and fe(ncell=2) == -4 and fe(out_ld=5) == -4


# ------------------------------------------------------------------ the operator and the public functions
def test_op_schema_and_fake_kernel():
    import aerognn.ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert str(torch.ops.aerognn.surface_forces.default._schema).startswith("aerognn::surface_forces(")
    with FakeTensorMode():
        pos = torch.empty(10, 3)
        f = torch.empty(10, 4, dtype=torch.float64)
        tri = torch.empty(7, 3, dtype=torch.int64)
        gptr = torch.empty(3, dtype=torch.int32)
        out, a, nrm, cells = torch.ops.aerognn.surface_forces(pos, None, tri, [f, f], None, None, gptr, True)
        assert out.shape == (2, 2, 2, 3) and out.dtype == torch.float64
        assert a.shape == (7,) and nrm.shape == (7, 3) and a.dtype == nrm.dtype == torch.float64
        assert cells.shape == (2, 7, 4) and cells.dtype == torch.float64
        off, conn = torch.empty(6, dtype=torch.int64), torch.empty(17, dtype=torch.int64)
        out, a, nrm, cells = torch.ops.aerognn.surface_forces(pos, off, conn, [pos.new_empty(10, 4).bfloat16()], None,
                                                              None, gptr, False)
        assert out.shape == (2, 1, 2, 3) and a.shape == (0,) and nrm.shape == (0, 3) and cells.shape == (0, 5, 4)
        assert cells.dtype == torch.float32
        out, a, nrm, cells = torch.ops.aerognn.surface_forces(None, off, conn, [f], None, None, gptr, True)
        assert a.shape == (0,) and cells.shape == (1, 5, 4)
        out, a, nrm, cells = torch.ops.aerognn.surface_forces(pos, off, conn, [], None, None, gptr, True)
        assert out.shape == (2, 0, 2, 3) and a.shape == (5,) and cells.shape == (0, 5, 4)


def test_cpu_tensors_raise():
    from aerognn import aero, surface
    pos = torch.rand(5, 3)
    tri = torch.tensor([[0, 1, 2], [2, 1, 3], [3, 1, 4]])
    f = torch.rand(5, 4)
    gptr = torch.tensor([0, 3], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="MI355X"):
        torch.ops.aerognn.surface_forces(pos, None, tri, [f], None, None, gptr, False)
    with pytest.raises(RuntimeError, match="MI355X"):
        surface.cell_geometry(pos, tri)
    with pytest.raises(RuntimeError, match="MI355X"):
        surface.point_to_cell(f, tri)
    with pytest.raises(RuntimeError, match="MI355X"):
        surface.integrate_surface(pos, tri, [f, f])
    with pytest.raises(RuntimeError, match="MI355X"):
        surface.edges_from_faces(tri, 5)
    with pytest.raises(RuntimeError, match="MI355X"):
        surface.edges_from_faces((torch.tensor([0, 3]), torch.tensor([0, 1, 2])), 5)
    with pytest.raises(RuntimeError, match="MI355X"):
        aero.calculate_aero_coefficients_3d_mesh(pos, tri, f, f)


def test_public_signatures():
    from aerognn import aero, meshgen, surface
    sig = lambda fn: list(inspect.signature(fn).parameters)  # noqa: E731
    assert sig(surface.faces_csr) == ["faces", "device"]
    assert sig(surface.cell_geometry) == ["pos", "faces"]
    assert sig(surface.point_to_cell) == ["values", "faces"]
    assert sig(surface.integrate_surface)[:6] == ["pos", "faces", "fields", "stats", "cell_batch", "ngraph"]
    assert sig(surface.edges_from_faces)[:2] == ["faces", "num_nodes"]
    p = inspect.signature(aero.calculate_aero_coefficients_3d_mesh).parameters
    assert list(p) == ["pos", "faces", "true_fields", "pred_fields", "reference_area", "dynamic_pressure", "stats"]
    assert [p[k].default for k in list(p)[4:]] == [1.0, 1.0, None]
    q = inspect.signature(aero.calculate_aero_coefficients_3d).parameters                 # unchanged
    assert list(q) == ["areas", "normals", "pressure", "shear_stress", "reference_area", "dynamic_pressure"]
    assert sig(meshgen.lattice_faces) == ["nu", "nv"] and "lattice_faces" in meshgen.__all__
