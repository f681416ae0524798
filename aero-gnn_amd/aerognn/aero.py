"""Evaluation on the device: the stage the reference runs after `model(...)` (inference.py
AeroInference.run_inference; utils.py calculate_aero_coefficients_2d / _3d).

The reference copies every prediction to the host, runs about twenty torch.mean passes per case and
builds the 2-D node areas in a Python loop over every directed edge. Here the error sums of a case
are ONE pass over pred and y (torch.ops.aerognn.eval_sums -> agn_eval_sums) and the force / moment
integration, node areas included, is ONE pass over the surface (torch.ops.aerognn.aero_forces ->
agn_aero_forces); only a few dozen doubles per case travel to the host.

  prediction_errors(pred_scaled, y_scaled, stats, batch=None) -> ErrorSums (device) -> .cpu() -> ErrorReport
  node_areas(pos, edge_index, length_scale=1e-2)              -> float64 [n]
  integrate_forces(pressure, shear, normals, ...)             -> ForceSums of [G, ...] tensors
  calculate_aero_coefficients_2d / _3d                        -> the reference's names and keys
  calculate_aero_coefficients_3d_mesh(pos, faces, true, pred) -> CA_true .. CY_pred from points and faces:
                                                                 cell areas, normals, point-to-cell means and
                                                                 force sums in ONE pass (aerognn.surface,
                                                                 torch.ops.aerognn.surface_forces)
  DeviceEvaluator(model, norm_stats, params)                  -> AeroInference without host copies

Sums are fp64, deterministic (fixed-order two-stage reductions, no atomics) and batch independent:
graph g of a batch gives bitwise the numbers of graph g evaluated alone.
"""
from __future__ import annotations

from collections import namedtuple
from typing import Optional

import numpy as np
import torch

from . import ops as _ops  # noqa: F401  (registers torch.ops.aerognn.*)
from .core import require_device

I32 = torch.int32
REL_EPS = 1e-8  # inference.py:97, :120
SUM_NAMES = ("abs_err", "sq_err", "abs_target", "count", "abs_rel", "sq_rel")


def chunk_rows() -> int:
    """Rows per reduction chunk of the two kernels (agn_aero_chunk_rows)."""
    from ._lib import lib
    return int(lib().agn_aero_chunk_rows())


def __getattr__(name):
    if name == "CHUNK_ROWS":
        return chunk_rows()
    raise AttributeError(name)


def graph_ptr(batch: Optional[torch.Tensor], n: int, device, ngraph: Optional[int] = None) -> torch.Tensor:
    """int32 [G + 1] row range of each graph of a PyG `batch` vector (sorted, as collate leaves it);
    None = one graph of n rows."""
    if batch is None:
        return torch.tensor([0, n], dtype=I32, device=device)
    from ._lib import check, lib, ptr
    from .core import stream
    require_device(batch)
    b = batch.to(torch.int64).contiguous()
    if b.numel() != n:
        raise ValueError("batch must have one entry per row")
    if ngraph is None:
        ngraph = int(b.max()) + 1 if n else 0
    gptr = torch.empty(ngraph + 1, dtype=I32, device=b.device)
    check(lib().agn_row_ptr_i64(ptr(b), n, ngraph, ptr(gptr), stream()), "row_ptr_i64")
    return gptr


# ----------------------------------------------------------------------------- error metrics
class ErrorReport:
    """Host side of ErrorSums: sums [G, 2, f, 6] float64 (scale 0 normalised, 1 physical; SUM_NAMES)
    and rows [G]. Every metric the reference prints is a ratio of these."""

    SCALES = {"normalized": 0, "physical": 1}

    def __init__(self, sums: np.ndarray, rows: np.ndarray):
        self.sums = np.asarray(sums, dtype=np.float64)
        self.rows = np.asarray(rows, dtype=np.float64)

    @property
    def num_graphs(self) -> int:
        return self.sums.shape[0]

    def _s(self, scale) -> int:
        return self.SCALES[scale] if isinstance(scale, str) else int(scale)

    def _pick(self, g):
        """(sums [2, f, 6], rows) of graph g, or of the whole set (g None: graph order, fp64)."""
        if g is None:
            s = np.zeros(self.sums.shape[1:], dtype=np.float64)
            for i in range(self.num_graphs):
                s = s + self.sums[i]
            return s, float(self.rows.sum())
        return self.sums[g], float(self.rows[g])

    def feature_errors(self, g=0, scale="physical", names=None) -> dict:
        """{feature: {'mae', 'mse'}} of inference.py:341-350 (g None: :404-413 over the test set)."""
        s, n = self._pick(g)
        s = s[self._s(scale)]
        names = list(names) if names is not None else [f"feature_{j}" for j in range(s.shape[0])]
        with np.errstate(divide="ignore", invalid="ignore"):
            return {nm: {"mae": float(s[j, 0] / n), "mse": float(s[j, 1] / n)} for j, nm in enumerate(names)}

    def compute_errors(self, g=0, scale="physical") -> dict:
        """AeroInference.compute_errors over all features of graph g (inference.py:90-111)."""
        s, n = self._pick(g)
        s = s[self._s(scale)].sum(axis=0)  # features in column order
        tot = n * self.sums.shape[2]
        with np.errstate(divide="ignore", invalid="ignore"):
            mae, mse = float(s[0] / tot), float(s[1] / tot)
            if s[3] > 0:
                rmae, rrmse = float(s[4] / s[3]), float(np.sqrt(s[5] / s[3]))
            else:
                rmae = rrmse = float("nan")
        # rmse as the reference forms it (inference.py:94): torch.sqrt(torch.tensor(mse)) is a float32
        # tensor whatever the input dtype, so the value is the fp32 square root of the fp32-rounded mse
        return {"mae": mae, "mse": mse, "rmse": float(np.sqrt(np.float32(mse))), "relative_mae": rmae,
                "relative_rmse": rrmse}

    def rrmse_percent(self, g=0, scale="physical") -> float:
        """AeroInference.compute_rrmse_percent (inference.py:113-126): a feature whose mean |t| is
        <= 1e-8 contributes 0."""
        s, n = self._pick(g)
        s = s[self._s(scale)]
        with np.errstate(divide="ignore", invalid="ignore"):
            rmse = np.sqrt(s[:, 1] / n)
            mean_abs = s[:, 2] / n
            rr = np.where(mean_abs > REL_EPS, rmse / mean_abs, 0.0)
            return float(np.mean(rr) * 100)

    def pooled(self, names=None) -> dict:
        """The test-set means of inference.py:395-413: the per-graph sums added in fp64 in graph order."""
        return {"errors_physical": self.feature_errors(None, "physical", names),
                "errors_normalized": self.feature_errors(None, "normalized", names)}

    @staticmethod
    def concat(reports) -> "ErrorReport":
        reports = list(reports)
        return ErrorReport(np.concatenate([r.sums for r in reports], 0), np.concatenate([r.rows for r in reports], 0))


class ErrorSums:
    """The [G, 2, f, 6] sums of prediction_errors, still on the device."""

    def __init__(self, sums: torch.Tensor, gptr: torch.Tensor):
        self.sums, self.gptr = sums, gptr

    def cpu(self) -> ErrorReport:
        """One device-to-host copy: the sums and the graph sizes in one buffer."""
        G = self.sums.shape[0]
        rows = (self.gptr[1:] - self.gptr[:-1]).to(torch.float64)
        h = torch.cat([self.sums.reshape(-1), rows]).cpu().numpy()
        return ErrorReport(h[:h.size - G].reshape(tuple(self.sums.shape)), h[h.size - G:])


def prediction_errors(pred_scaled, y_scaled, stats, batch=None, ngraph=None) -> ErrorSums:
    """Error sums of a batch in both scales, one pass: stats is the reference's norm_stats dict
    ('target_mean', 'target_std'); physical values are pred * std + mean as inference.py:77-82."""
    require_device(pred_scaled, y_scaled, batch)
    dev = pred_scaled.device
    mean = torch.as_tensor(stats["target_mean"]).to(dev)
    std = torch.as_tensor(stats["target_std"]).to(dev)
    gptr = graph_ptr(batch, pred_scaled.shape[0], dev, ngraph)
    return ErrorSums(torch.ops.aerognn.eval_sums(pred_scaled, y_scaled, mean, std, gptr), gptr)


# ----------------------------------------------------------------------------- forces
ForceSums = namedtuple("ForceSums", "force moment abs_force abs_moment areas")


def integrate_forces(pressure, shear_stress, normals, pos=None, areas=None, edge_index=None, batch=None,
                     moment_center=None, length_scale=1e-2, ngraph=None) -> ForceSums:
    """Per graph: sum F [G, dim], sum M [G, 1] (2-D) or [G, 3] (None without pos), and the sums of the
    absolute contributions, F = p n A - tau A, M = r x F about moment_center. Element areas are
    either given or the 2-D rule of utils.py:510-520 from (pos, edge_index); `areas` of the result is
    then the float64 [n] node areas."""
    require_device(pressure, shear_stress, normals)
    dev = shear_stress.device
    n, dim = shear_stress.shape
    gptr = graph_ptr(batch, n, dev, ngraph)
    if moment_center is None:
        center = []
    else:
        center = [float(c) for c in (moment_center.detach().cpu().reshape(-1).tolist()
                                     if torch.is_tensor(moment_center) else np.asarray(moment_center).reshape(-1))]
    out, a = torch.ops.aerognn.aero_forces(pressure, shear_stress, normals, pos, areas, edge_index, gptr, center,
                                           float(length_scale))
    nm = 1 if dim == 2 else 3
    return ForceSums(out[:, 0, :dim], out[:, 1, :nm] if pos is not None else None, out[:, 2, :dim],
                     out[:, 3, :nm] if pos is not None else None, a if edge_index is not None else areas)


def node_areas(pos, edge_index, length_scale=1e-2) -> torch.Tensor:
    """utils.py:510-520 on the device: float64 [n], half the length of every outgoing edge times
    length_scale, summed per sender in edge order; a node without outgoing edges has area 0."""
    require_device(pos, edge_index)
    n = pos.shape[0]
    zero = torch.zeros(n, dtype=pos.dtype, device=pos.device)
    return integrate_forces(zero, pos, pos, pos=pos, edge_index=edge_index, length_scale=length_scale).areas


def _coefficients(fs: ForceSums, ref_area, ref_length, q) -> np.ndarray:
    """[G, 2 * (dim + nm)] on the host: coefficients then their absolute-contribution scales."""
    cols = [fs.force, fs.moment, fs.abs_force, fs.abs_moment]
    h = torch.cat([c for c in cols if c is not None], dim=1).cpu().numpy()
    dim = fs.force.shape[1]
    nm = 0 if fs.moment is None else fs.moment.shape[1]
    # F / reference_area / q and M / (reference_area * reference_length) / q, as utils.py:551-553
    den = np.concatenate([np.full(dim, float(ref_area)), np.full(nm, float(ref_area) * float(ref_length))] * 2)
    return h / den / float(q)


def calculate_aero_coefficients_2d(test_data, pressure, shear_stress, reference_area: float = 1.0,
                                   reference_length: float = 1.0, moment_center=None,
                                   dynamic_pressure: float = 1.0) -> dict:
    """utils.py:451-559 with the reference's signature and keys; test_data carries pos, normals and
    edge_index on the device. Also usable on a PyG batch through coefficients_2d_batch."""
    c = coefficients_2d_batch(test_data, pressure, shear_stress, reference_area, reference_length, moment_center,
                              dynamic_pressure)
    return {"CA": float(c["CA"][0]), "CN": float(c["CN"][0]), "Cm": float(c["Cm"][0])}


def coefficients_2d_batch(test_data, pressure, shear_stress, reference_area=1.0, reference_length=1.0,
                          moment_center=None, dynamic_pressure=1.0, batch=None) -> dict:
    """numpy [G] arrays CA, CN, Cm and their scales S_CA, S_CN, S_Cm (the sums of absolute
    contributions, normalised like the coefficient)."""
    fs = integrate_forces(pressure, shear_stress, test_data.normals, pos=test_data.pos,
                          edge_index=test_data.edge_index, batch=batch, moment_center=moment_center)
    c = _coefficients(fs, reference_area, reference_length, dynamic_pressure)
    return {"CA": c[:, 0], "CN": c[:, 1], "Cm": c[:, 2], "S_CA": c[:, 3], "S_CN": c[:, 4], "S_Cm": c[:, 5]}


def calculate_aero_coefficients_3d(areas, normals, pressure, shear_stress, reference_area: float = 1.0,
                                   dynamic_pressure: float = 1.0) -> dict:
    """utils.py:385-448 for one set of fields: the reference reads Area, Normals, p and wallShearStress
    from a pyvista surface's cell data; this takes those four cell arrays (call it once for the true and
    once for the predicted fields)."""
    fs = integrate_forces(pressure, shear_stress, normals, areas=areas)
    c = _coefficients(fs, reference_area, 1.0, dynamic_pressure)
    return {"CA": float(c[0, 0]), "CN": float(c[0, 1]), "CY": float(c[0, 2])}


def calculate_aero_coefficients_3d_mesh(pos, faces, true_fields, pred_fields, reference_area: float = 1.0,
                                        dynamic_pressure: float = 1.0, stats=None) -> dict:
    """inference.py:310-320 followed by utils.py:385-448 from the mesh itself: pos [N, 3], a face list
    (aerognn.surface.faces_csr's formats; consistently wound) and the true and predicted point fields
    [N, 4] (pressure, tau_x, tau_y, tau_z). Cell areas, cell normals, the point-to-cell means of both
    sets and the force sums are ONE surface_forces pass. With stats (norm_stats) both sets are
    de-normalised first. Returns the reference's six keys CA_true .. CY_pred (utils.py:441-448)."""
    c = coefficients_3d_mesh(pos, faces, [true_fields, pred_fields], reference_area, dynamic_pressure, stats)
    return {f"{k}_{nm}": float(c[k][0, s]) for s, nm in enumerate(("true", "pred")) for k in ("CA", "CN", "CY")}


def coefficients_3d_mesh(pos, faces, fields, reference_area=1.0, dynamic_pressure=1.0, stats=None, cell_batch=None,
                         ngraph=None) -> dict:
    """numpy [G, nset] arrays CA, CN, CY and their scales S_CA, S_CN, S_CY (the sums of absolute
    contributions, normalised like the coefficient) for up to four field sets in one pass."""
    from .surface import integrate_surface
    ss = integrate_surface(pos, faces, fields, stats=stats, cell_batch=cell_batch, ngraph=ngraph)
    h = torch.stack([ss.force, ss.abs_force]).cpu().numpy() / float(reference_area) / float(dynamic_pressure)
    return {"CA": h[0, :, :, 0], "CN": h[0, :, :, 1], "CY": h[0, :, :, 2],
            "S_CA": h[1, :, :, 0], "S_CN": h[1, :, :, 1], "S_CY": h[1, :, :, 2]}


# ----------------------------------------------------------------------------- AeroInference
class DeviceEvaluator:
    """AeroInference (inference.py:29-473) without host copies, plots or VTU export: evaluate_case
    returns the reference's case_error_info dictionary, errors_txt the text of errors.txt."""

    def __init__(self, model, norm_stats, params):
        self.model = model
        self.norm_stats = norm_stats
        self.params = params
        self.model.eval()
        try:
            self.device = next(model.parameters()).device
        except (StopIteration, AttributeError):
            self.device = torch.device("cuda")
        self.device_norm_stats = {k: (v.to(self.device) if torch.is_tensor(v) else v) for k, v in norm_stats.items()}
        self.cases = []
        self._reports = []

    def _ds(self):
        return self.params.get("dataset", {})

    @torch.no_grad()
    def predict(self, data) -> torch.Tensor:
        """The model-class dispatch of predict_single (inference.py:52-74)."""
        data = data.to(self.device)
        name = self.model.__class__.__name__
        if name in ("poolMGN", "MeshGraphNet_v2"):
            batch = torch.zeros(data.x.size(0), dtype=torch.long, device=self.device)
            return self.model(data.x, data.edge_attr, data.edge_index, batch)
        if name == "BiStridedMeshGraphNet":
            batch = torch.zeros(data.x.size(0), dtype=torch.long, device=self.device)
            return self.model(data.x, data.edge_attr, data.edge_index, batch=batch,
                              pos=data.pos if hasattr(data, "pos") else None)
        if name == "MLPNet":
            return self.model(data.x)
        return self.model(data.x, data.edge_attr, data.edge_index)

    @torch.no_grad()
    def evaluate_case(self, data) -> dict:
        data = data.to(self.device)
        pred = self.predict(data)
        y = data.y
        names = self._ds().get("output_features", [f"feature_{j}" for j in range(y.shape[1])])
        rep = prediction_errors(pred, y, self.device_norm_stats).cpu()
        coeff_str = ""
        if self._ds().get("name", "dataset") == "airfoil_2d":
            mean, std = self.device_norm_stats["target_mean"], self.device_norm_stats["target_std"]
            mach = float(data.mach)
            q = 0.5 * 1.4 * 101325 * mach * mach
            co = []
            for t in (y, pred):  # true, predicted (inference.py:266-289)
                phys = t * std + mean
                co.append(calculate_aero_coefficients_2d(data, pressure=phys[:, 0:1], shear_stress=phys[:, 1:3],
                                                         reference_area=1e-2, reference_length=1.0,
                                                         dynamic_pressure=q))
            tc, pc = co
            coeff_str = (f" | CA:{pc['CA']:7.4f} ({tc['CA']:7.4f}) "
                         f"| CN:{pc['CN']:7.4f} ({tc['CN']:7.4f}) "
                         f"| Cm:{pc['Cm']:7.4f} ({tc['Cm']:7.4f})")
        elif self._ds().get("name", "dataset") == "ahmed_body" and getattr(data, "faces", None) is not None:
            c = self._ahmed_coefficients(data, y, pred)
            coeff_str = (f" | CA:{c['CA_pred']:7.4f} ({c['CA_true']:7.4f}) "
                         f"| CN:{c['CN_pred']:7.4f} ({c['CN_true']:7.4f}) "
                         f"| CY:{c['CY_pred']:7.4f} ({c['CY_true']:7.4f})")
        info = {"case_id": len(self.cases),
                "rrmse_percent": rep.rrmse_percent(0, "physical"),
                "errors_physical": rep.feature_errors(0, "physical", names),
                "errors_normalized": rep.feature_errors(0, "normalized", names),
                "coeff_str": coeff_str}
        for key in ("airfoil", "mach", "alpha", "case_no"):
            if hasattr(data, key):
                v = getattr(data, key)
                info[key] = v.item() if torch.is_tensor(v) else v
        self.cases.append(info)
        self._reports.append(rep)
        return info

    def _ahmed_coefficients(self, data, y, pred) -> dict:
        """inference.py:298-327 from data.pos and data.faces instead of the case's .vtp: the six
        coefficients with q = 0.5 * 1.225 * Velocity^2 and reference_area = Height * Width * 1e-6 / 2.
        The reference's "true" fields are the file's own cell data: data.cell_y ([C, 4], physical) is
        used when the case carries it, otherwise the point-to-cell mean of the de-normalised y."""
        from .surface import integrate_surface
        num = lambda v: float(v.reshape(-1)[0]) if torch.is_tensor(v) else float(v)  # noqa: E731
        velocity, height, width = num(data.Velocity), num(data.Height), num(data.Width)
        kw = dict(reference_area=height * width * 1e-6 / 2, dynamic_pressure=0.5 * 1.225 * velocity * velocity)
        cell_y = getattr(data, "cell_y", None)
        if cell_y is None:
            return calculate_aero_coefficients_3d_mesh(data.pos, data.faces, y[:, :4], pred[:, :4],
                                                       stats=self.device_norm_stats, **kw)
        ss = integrate_surface(data.pos, data.faces, pred[:, :4], stats=self.device_norm_stats, return_cells=True)
        cp = ss.force[0, 0].cpu().numpy() / kw["reference_area"] / kw["dynamic_pressure"]
        cell_y = cell_y.to(self.device)
        ct = calculate_aero_coefficients_3d(ss.areas, ss.normals.to(cell_y.dtype), cell_y[:, 0], cell_y[:, 1:4], **kw)
        return {"CA_true": ct["CA"], "CN_true": ct["CN"], "CY_true": ct["CY"],
                "CA_pred": float(cp[0]), "CN_pred": float(cp[1]), "CY_pred": float(cp[2])}

    def test_set_mean(self) -> dict:
        names = self._ds().get("output_features", None)
        return ErrorReport.concat(self._reports).pooled(names)

    def errors_txt(self) -> str:
        """errors.txt of inference.py:424-470 for the cases evaluated so far."""
        pooled = self.test_set_mean()
        feats = list(pooled["errors_physical"].keys())
        mean_of = lambda d, k: float(np.mean([d[f][k] for f in feats]))  # noqa: E731
        rr = float(np.mean([c["rrmse_percent"] for c in self.cases]))
        lines = [f"TEST_MEAN | rrmse:{rr:6.2f} | nmae:{mean_of(pooled['errors_normalized'], 'mae'):8.6f} | "
                 f"nmse:{mean_of(pooled['errors_normalized'], 'mse'):8.6f} | "
                 f"mae:{mean_of(pooled['errors_physical'], 'mae'):7.2f} | "
                 f"mse:{mean_of(pooled['errors_physical'], 'mse'):12.2f}", ""]
        ds = self._ds().get("name", "dataset")
        for c in self.cases:
            head = (f"case_{c['case_id']:03d} | rrmse:{c['rrmse_percent']:6.2f} | "
                    f"nmae:{mean_of(c['errors_normalized'], 'mae'):8.6f} | "
                    f"nmse:{mean_of(c['errors_normalized'], 'mse'):8.6f} | "
                    f"mae:{mean_of(c['errors_physical'], 'mae'):7.2f} | "
                    f"mse:{mean_of(c['errors_physical'], 'mse'):12.2f}{c.get('coeff_str', '')}")
            if ds == "airfoil_2d":
                airfoil, mach, alpha = c.get("airfoil", "N/A"), c.get("mach", "N/A"), c.get("alpha", "N/A")
                if isinstance(mach, (int, float)):
                    mach = f"{mach:.2f}"
                if isinstance(alpha, (int, float)):
                    alpha = f"{alpha:.2f}"
                lines.append(f"{head} | {airfoil:8s} | {str(mach):4s} | {str(alpha):5s}")
            elif ds == "ahmed_body":
                lines.append(f"{head} | {str(c.get('case_no', 'N/A')):5s}")
        return "\n".join(lines) + "\n"
