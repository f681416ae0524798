"""Golden vectors for the evaluation stage from the REAL reference (this container only).

Imports tools/make_goldens.py for its stand-ins and helpers (importing it runs no case), extends the
stand-ins with the names the reference's utils.py and inference.py import and never call on these
paths (pyvista, torch_geometric.utils / .loader / .data), then imports those two modules. Writes
tests/golden/<case>.npz:

  aero2d_f32 / _f64       a two-case airfoil_2d set: closed airfoil-like loops of 257 and 96 nodes, both
                          edge directions, edges shuffled, one node of the second loop without outgoing
                          edges; normalised targets y and predictions pred [N, 4] (p, tau_x, tau_y, T), the
                          statistics, the de-normalised fields (inference.py:77-82 on the CPU). Expected:
                          calculate_aero_coefficients_2d for the true and the predicted fields with
                          reference_area = 1e-2 and dynamic_pressure = 0.5 * 1.4 * 101325 * 0.3^2, once more
                          with moment_center = (0.25, 0); compute_rrmse_percent; the per-feature and pooled
                          torch.mean expressions of run_inference
  aero3d_f32              calculate_aero_coefficients_3d on a SimpleNamespace(cell_data=...) stand-in
                          surface made of the triangles of the ellipsoid(12, 8) lattice (areas, normals)
  evalmetrics_f32 / _f64  pred, y of [1000, 4] and [37, 4] (one target column of the second all zeros, a
                          few exact zeros scattered in another) and a [5, 4] case whose targets are zero
                          in both scales. Expected: AeroInference.compute_errors and compute_rrmse_percent
                          in both scales, the per-feature and pooled torch.mean expressions

Run:  python tools/make_goldens_aero.py
"""
from __future__ import annotations

import os
import sys
import types

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_goldens as G  # noqa: E402  (installs the stand-ins, puts the reference first on sys.path)
from make_goldens import save  # noqa: E402

# names only: imported by utils.py / inference.py at module level, never called on the paths used here
_tg = sys.modules["torch_geometric"]
for _name, _attrs in (("torch_geometric.utils", ("is_undirected", "to_undirected")),
                      ("torch_geometric.loader", ("DataLoader",)),
                      ("torch_geometric.data", ("Data",))):
    _m = types.ModuleType(_name)
    for _a in _attrs:
        setattr(_m, _a, type(_a, (), {}))
    sys.modules[_name] = _m
    setattr(_tg, _name.rsplit(".", 1)[1], _m)
sys.modules["pyvista"] = types.ModuleType("pyvista")

import utils as _refutils  # noqa: E402
import inference as _refinf  # noqa: E402
assert os.path.abspath(_refutils.__file__).startswith(G.REF), _refutils.__file__    # the REFERENCE's modules
assert os.path.abspath(_refinf.__file__).startswith(G.REF), _refinf.__file__
from utils import calculate_aero_coefficients_2d, calculate_aero_coefficients_3d  # noqa: E402
from inference import AeroInference  # noqa: E402

from aerognn.meshgen import ellipsoid  # noqa: E402  (sys.modules still holds the package make_goldens imported)

INF = AeroInference.__new__(AeroInference)  # compute_errors / compute_rrmse_percent read nothing of self

MEAN = (1e5, 3.0, -2.0, 300.0)
STD = (3e4, 50.0, 50.0, 20.0)
REF_AREA = 1e-2
MACH = 0.3
Q2D = 0.5 * 1.4 * 101325 * MACH * MACH
CENTER = (0.25, 0.0)


def loop_mesh(n, seed, drop_node=None):
    """Closed airfoil-like loop of n nodes: pos, unit outward normals (float64), edge_index with both
    directions, shuffled; drop_node keeps no outgoing edge."""
    rng = np.random.default_rng(seed)
    th = 2 * np.pi * (np.arange(n) + 0.25 * rng.random(n)) / n
    x = 0.5 * (1 + np.cos(th))
    yy = 0.06 * np.sin(th) * (1.6 - np.cos(th)) + 0.01 * np.sin(2 * th)
    pos = np.stack([x, yy], 1)
    tan = np.roll(pos, -1, 0) - np.roll(pos, 1, 0)
    nrm = np.stack([tan[:, 1], -tan[:, 0]], 1)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    a = np.arange(n)
    b = (a + 1) % n
    ei = np.concatenate([np.stack([a, b]), np.stack([b, a])], 1)
    ei = ei[:, rng.permutation(ei.shape[1])]
    if drop_node is not None:
        ei = ei[:, ei[0] != drop_node]
    return pos, nrm, ei.astype(np.int64)


def feature_errors(pred, target):
    """[f, 2] (mae, mse): the torch.mean expressions of inference.py:343-349 / :406-412."""
    out = []
    for j in range(pred.shape[1]):
        out.append([torch.mean(torch.abs(pred[:, j] - target[:, j])).item(),
                    torch.mean((pred[:, j] - target[:, j]) ** 2).item()])
    return np.array(out, dtype=np.float64)


def denorm(t, std, mean):
    return t * std + mean  # inference.py:77-82 (two torch ops)


def case_aero2d(dtype, name):
    rng = np.random.default_rng(31)
    mean = torch.tensor(MEAN, dtype=dtype)
    std = torch.tensor(STD, dtype=dtype)
    arrs = dict(target_mean=mean, target_std=std)
    coef_true, coef_pred, coef_true_c, rrmse, f_phys, f_norm = [], [], [], [], [], []
    all_p, all_t, all_pn, all_tn = [], [], [], []
    for i, (n, drop) in enumerate(((257, None), (96, 17))):
        pos, nrm, ei = loop_mesh(n, 40 + i, drop)
        pos_t, nrm_t, ei_t = torch.from_numpy(pos).to(dtype), torch.from_numpy(nrm).to(dtype), torch.from_numpy(ei)
        y = torch.from_numpy(rng.standard_normal((n, 4))).to(dtype)
        pred = (y.double() + 0.1 * torch.from_numpy(rng.standard_normal((n, 4)))).to(dtype)
        tp, pp = denorm(y, std, mean), denorm(pred, std, mean)
        data = types.SimpleNamespace(pos=pos_t, normals=nrm_t, edge_index=ei_t)
        kw = dict(reference_area=REF_AREA, reference_length=1.0, dynamic_pressure=Q2D)
        ct = calculate_aero_coefficients_2d(data, pressure=tp[:, 0:1], shear_stress=tp[:, 1:3], **kw)
        cp = calculate_aero_coefficients_2d(data, pressure=pp[:, 0:1], shear_stress=pp[:, 1:3], **kw)
        cc = calculate_aero_coefficients_2d(data, pressure=tp[:, 0:1], shear_stress=tp[:, 1:3],
                                            moment_center=np.array(CENTER), **kw)
        for lst, c in ((coef_true, ct), (coef_pred, cp), (coef_true_c, cc)):
            lst.append([c["CA"], c["CN"], c["Cm"]])
        rrmse.append(INF.compute_rrmse_percent(pp, tp))
        f_phys.append(feature_errors(pp, tp))
        f_norm.append(feature_errors(pred, y))
        all_p.append(pp), all_t.append(tp), all_pn.append(pred), all_tn.append(y)
        arrs.update({f"pos{i}": pos_t, f"normals{i}": nrm_t, f"edge_index{i}": ei_t, f"y{i}": y, f"pred{i}": pred,
                     f"phys_true{i}": tp, f"phys_pred{i}": pp})
    save(name, dict(dtype=str(dtype), reference_area=REF_AREA, mach=MACH, dynamic_pressure=Q2D, center=list(CENTER),
                    alpha=[2.0, -1.5], airfoil=["loop257", "loop96"], dropped_node=17,
                    output_features=["p", "tau_x", "tau_y", "T"]),
         coef_true=np.array(coef_true), coef_pred=np.array(coef_pred), coef_true_center=np.array(coef_true_c),
         rrmse=np.array(rrmse), feat_phys=np.array(f_phys), feat_norm=np.array(f_norm),
         pooled_phys=feature_errors(torch.cat(all_p), torch.cat(all_t)),
         pooled_norm=feature_errors(torch.cat(all_pn), torch.cat(all_tn)), **arrs)


def lattice_triangles(nu, nv):
    """The triangles of meshgen.ellipsoid's lat-long lattice (node id = j * nu + i)."""
    i, j = np.arange(nu), np.arange(nv)
    nid = j[:, None] * nu + i[None, :]
    right = j[:, None] * nu + (i[None, :] + 1) % nu
    t1 = np.stack([nid[:-1].ravel(), right[:-1].ravel(), nid[1:].ravel()], 1)
    t2 = np.stack([right[:-1].ravel(), right[1:].ravel(), nid[1:].ravel()], 1)
    return np.concatenate([t1, t2], 0)


def case_aero3d():
    m = ellipsoid(12, 8)
    tri = lattice_triangles(12, 8)
    p = m["pos"].astype(np.float64)
    cr = np.cross(p[tri[:, 1]] - p[tri[:, 0]], p[tri[:, 2]] - p[tri[:, 0]])
    area = 0.5 * np.linalg.norm(cr, axis=1)                                  # float64, as pyvista's Area
    normals = (cr / np.linalg.norm(cr, axis=1, keepdims=True)).astype(np.float32)
    rng = np.random.default_rng(33)
    nc = tri.shape[0]
    cd = {"Area": area, "Normals": normals,
          "p": (100.0 * rng.standard_normal(nc) - 20.0).astype(np.float32),
          "wallShearStress": (2.0 * rng.standard_normal((nc, 3))).astype(np.float32)}
    cd["p_pred"] = (cd["p"] + 5.0 * rng.standard_normal(nc)).astype(np.float32)
    cd["wallShearStress_pred"] = (cd["wallShearStress"] + 0.2 * rng.standard_normal((nc, 3))).astype(np.float32)
    ref_area, q = 0.389 * 0.288 / 2, 0.5 * 1.225 * 40.0 * 40.0
    c = calculate_aero_coefficients_3d(types.SimpleNamespace(cell_data=cd), reference_area=ref_area,
                                       reference_length=1.0, dynamic_pressure=q)
    save("aero3d_f32", dict(reference_area=ref_area, dynamic_pressure=q), areas=area, normals=normals, p=cd["p"],
         shear=cd["wallShearStress"], p_pred=cd["p_pred"], shear_pred=cd["wallShearStress_pred"],
         coef_true=np.array([c["CA_true"], c["CN_true"], c["CY_true"]]),
         coef_pred=np.array([c["CA_pred"], c["CN_pred"], c["CY_pred"]]))


ERR_KEYS = ("mae", "mse", "rmse", "relative_mae", "relative_rmse")


def case_metrics(dtype, name):
    rng = np.random.default_rng(35)
    arrs, meta_cases = {}, []
    pooled = [[], [], [], []]
    for i, n in enumerate((1000, 37, 5)):
        mean = torch.tensor(MEAN if i < 2 else (0.0, 0.0, 0.0, 0.0), dtype=dtype)
        std = torch.tensor(STD, dtype=dtype)
        y = torch.from_numpy(rng.standard_normal((n, 4))).to(dtype)
        if i == 1:
            y[:, 2] = 0.0                      # one target column all zeros
            y[[3, 11, 30], 0] = 0.0            # a few exact zeros in another
        if i == 2:
            y[:] = 0.0                         # zero in both scales (mean = 0): no |t| > 1e-8 anywhere
        pred = (y.double() + 0.1 * torch.from_numpy(rng.standard_normal((n, 4)))).to(dtype)
        tp, pp = denorm(y, std, mean), denorm(pred, std, mean)
        for s, (a, b) in enumerate(((pred, y), (pp, tp))):  # scale 0 normalised, 1 physical
            e = INF.compute_errors(a, b)
            arrs[f"errors{i}_s{s}"] = np.array([e[k] for k in ERR_KEYS], dtype=np.float64)
            arrs[f"rrmse{i}_s{s}"] = np.array(INF.compute_rrmse_percent(a, b), dtype=np.float64)
            arrs[f"feat{i}_s{s}"] = feature_errors(a, b)
        if i < 2:
            for lst, t in zip(pooled, (pred, y, pp, tp)):
                lst.append(t)
        arrs.update({f"pred{i}": pred, f"y{i}": y, f"mean{i}": mean, f"std{i}": std})
        meta_cases.append(n)
    arrs["pooled_s0"] = feature_errors(torch.cat(pooled[0]), torch.cat(pooled[1]))
    arrs["pooled_s1"] = feature_errors(torch.cat(pooled[2]), torch.cat(pooled[3]))
    save(name, dict(dtype=str(dtype), rows=meta_cases, error_keys=list(ERR_KEYS), pooled_cases=[0, 1]), **arrs)


if __name__ == "__main__":
    torch.set_num_threads(8)
    case_aero2d(torch.float32, "aero2d_f32")
    case_aero2d(torch.float64, "aero2d_f64")
    case_aero3d()
    case_metrics(torch.float32, "evalmetrics_f32")
    case_metrics(torch.float64, "evalmetrics_f64")
