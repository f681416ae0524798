"""Golden vector for the 3-D surface evaluation from a face list, from the REAL reference (this
container only).

Imports tools/make_goldens_aero.py for its stand-ins (the names the reference's utils.py imports and
never calls on this path: pyvista, torch_geometric.utils / .loader / .data) and for the reference's own
calculate_aero_coefficients_3d; importing it runs no case. Writes tests/golden/aero3d_mesh_f32.npz:

  mesh     ellipsoid(12, 8) with meshgen.lattice_faces, every fourth triangle pair merged into a quad:
           a mixed triangle / quad list in CSR form (offsets, conn)
  fields   fp32 true and predicted point fields [N, 4] (p, tau_x, tau_y, tau_z)
  cells    what the three VTK filters of inference.py:310-320 hand the reference, from the numpy fp64
           restatement tests/surface_ref.py (pyvista / VTK are not available): Area float64, Normals,
           p, wallShearStress, p_pred, wallShearStress_pred float32
  coef     the six numbers the reference's calculate_aero_coefficients_3d returns on a
           SimpleNamespace(cell_data=...) stand-in surface

Run:  python tools/make_goldens_surface.py
"""
from __future__ import annotations

import os
import sys
import types

sys.dont_write_bytecode = True
_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, _HERE)

import numpy as np  # noqa: E402

import make_goldens_aero as A  # noqa: E402  (installs the stand-ins, imports the reference's utils.py)

sys.path.insert(0, os.path.join(_HERE, "..", "tests"))
import surface_ref  # noqa: E402

from aerognn.meshgen import ellipsoid, lattice_faces  # noqa: E402


def case_aero3d_mesh():
    m = ellipsoid(12, 8)
    pos = m["pos"].astype(np.float32)
    offsets, conn = surface_ref.merge_pairs(lattice_faces(12, 8), every=4)
    cells = surface_ref.cells_of(offsets, conn)
    rng = np.random.default_rng(37)
    n = pos.shape[0]
    true = np.concatenate([100.0 * rng.standard_normal((n, 1)) - 20.0, 2.0 * rng.standard_normal((n, 3))], 1)
    pred = true + np.concatenate([5.0 * rng.standard_normal((n, 1)), 0.2 * rng.standard_normal((n, 3))], 1)
    true, pred = true.astype(np.float32), pred.astype(np.float32)
    area, normals = surface_ref.cell_geometry(pos, cells)
    ct, cp = surface_ref.point_to_cell(true, cells), surface_ref.point_to_cell(pred, cells)
    cd = {"Area": area, "Normals": normals.astype(np.float32),          # the dtypes VTK hands the reference
          "p": np.ascontiguousarray(ct[:, 0]), "wallShearStress": np.ascontiguousarray(ct[:, 1:4]),
          "p_pred": np.ascontiguousarray(cp[:, 0]), "wallShearStress_pred": np.ascontiguousarray(cp[:, 1:4])}
    assert cd["Area"].dtype == np.float64 and all(cd[k].dtype == np.float32 for k in cd if k != "Area")
    ref_area, q = 0.389 * 0.288 / 2, 0.5 * 1.225 * 40.0 * 40.0
    c = A.calculate_aero_coefficients_3d(types.SimpleNamespace(cell_data=cd), reference_area=ref_area,
                                         reference_length=1.0, dynamic_pressure=q)
    A.save("aero3d_mesh_f32", dict(reference_area=ref_area, dynamic_pressure=q, nu=12, nv=8, merge_every=4),
           pos=pos, offsets=offsets, conn=conn, true=true, pred=pred, areas=cd["Area"], normals=cd["Normals"],
           p=cd["p"], shear=cd["wallShearStress"], p_pred=cd["p_pred"], shear_pred=cd["wallShearStress_pred"],
           coef_true=np.array([c["CA_true"], c["CN_true"], c["CY_true"]]),
           coef_pred=np.array([c["CA_pred"], c["CN_pred"], c["CY_pred"]]))


if __name__ == "__main__":
    case_aero3d_mesh()
