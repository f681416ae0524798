"""Plain numpy restatement of the two evaluation contracts (include/aerognn.h agn_eval_sums,
agn_aero_forces): a helper for the tests, not a test. It carries the kernels' roundings in the input
dtype (p = pred * std then + mean, d = p - t, d / t, pressure * normal, the coordinate differences of
the area rule) and forms everything after them in float64; only the order of the fp64 sums differs
from the kernels'."""
import numpy as np

REL_EPS = 1e-8


def _scale_terms(p, t):
    """[f, 6] float64 of one graph and one scale; p, t in the input dtype."""
    d = p - t                                   # rounded once in the input dtype
    dd = d.astype(np.float64)
    at = np.abs(t.astype(np.float64))
    nz = at > REL_EPS
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(nz, (d / t).astype(np.float64), 0.0)   # the division in the input dtype
    return np.stack([np.abs(dd).sum(0), (dd * dd).sum(0), at.sum(0), nz.sum(0).astype(np.float64),
                     np.abs(q).sum(0), (q * q).sum(0)], axis=1)


def eval_sums(pred, y, mean, std, gptr=None):
    """[G, 2, f, 6] float64."""
    pred, y = np.asarray(pred), np.asarray(y)
    dt = pred.dtype
    mean, std = np.asarray(mean, dtype=dt), np.asarray(std, dtype=dt)
    gptr = [0, pred.shape[0]] if gptr is None else [int(v) for v in gptr]
    out = np.zeros((len(gptr) - 1, 2, pred.shape[1], 6))
    for g in range(len(gptr) - 1):
        p, t = pred[gptr[g]:gptr[g + 1]], y[gptr[g]:gptr[g + 1]]
        out[g, 0] = _scale_terms(p, t)
        pp = p * std                            # two separately rounded ops
        pp = pp + mean
        tp = t * std
        tp = tp + mean
        out[g, 1] = _scale_terms(pp, tp)
    return out


def node_areas(pos, edge_index, length_scale=1e-2):
    """float64 [n]: sum over a node's outgoing edges of |pos[dst] - pos[v]| * (0.5 * length_scale)."""
    pos, ei = np.asarray(pos), np.asarray(edge_index)
    diff = pos[ei[1]] - pos[ei[0]]              # in the input dtype
    ln = np.sqrt((diff.astype(np.float64) ** 2).sum(1)) * (0.5 * length_scale)
    area = np.zeros(pos.shape[0])
    np.add.at(area, ei[0], ln)                  # unbuffered, in edge order
    return area


def forces(pressure, shear, normals, areas, pos=None, center=None, gptr=None):
    """[G, 4, 3] float64: sum F, sum M, sum |F|, sum |M| (2-D: M in slot 0)."""
    pressure, shear, normals = np.asarray(pressure).reshape(-1), np.asarray(shear), np.asarray(normals)
    n, dim = shear.shape
    pn = pressure[:, None] * normals            # rounded once in the input dtype
    a = np.asarray(areas, dtype=np.float64)[:, None]
    F = pn.astype(np.float64) * a - shear.astype(np.float64) * a
    M = np.zeros((n, 3))
    if pos is not None:
        c = np.zeros(dim) if center is None else np.asarray(center, dtype=np.float64)
        r = np.asarray(pos).astype(np.float64) - c
        if dim == 2:
            M[:, 0] = r[:, 0] * F[:, 1] - r[:, 1] * F[:, 0]
        else:
            M[:, 0] = r[:, 1] * F[:, 2] - r[:, 2] * F[:, 1]
            M[:, 1] = r[:, 2] * F[:, 0] - r[:, 0] * F[:, 2]
            M[:, 2] = r[:, 0] * F[:, 1] - r[:, 1] * F[:, 0]
    gptr = [0, n] if gptr is None else [int(v) for v in gptr]
    out = np.zeros((len(gptr) - 1, 4, 3))
    for g in range(len(gptr) - 1):
        s = slice(gptr[g], gptr[g + 1])
        out[g, 0, :dim] = F[s].sum(0)
        out[g, 1] = M[s].sum(0)
        out[g, 2, :dim] = np.abs(F[s]).sum(0)
        out[g, 3] = np.abs(M[s]).sum(0)
    return out


def metrics(sums, rows):
    """The reference's metrics of one graph and one scale from sums [f, 6]: (compute_errors' five
    values, rrmse_percent, per-feature [f, 2] mae / mse)."""
    f = sums.shape[0]
    tot = sums.sum(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        mae, mse = tot[0] / (rows * f), tot[1] / (rows * f)
        rel = (tot[4] / tot[3], np.sqrt(tot[5] / tot[3])) if tot[3] > 0 else (np.nan, np.nan)
        rmse_j, mabs_j = np.sqrt(sums[:, 1] / rows), sums[:, 2] / rows
        rr = np.where(mabs_j > REL_EPS, rmse_j / mabs_j, 0.0).mean() * 100
        feat = np.stack([sums[:, 0] / rows, sums[:, 1] / rows], 1)
    # rmse as the reference forms it: torch.sqrt(torch.tensor(mse)), a float32 tensor whatever the input dtype
    return np.array([mae, mse, float(np.sqrt(np.float32(mse))), rel[0], rel[1]]), float(rr), feat
