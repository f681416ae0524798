"""Golden comparisons of the evaluation stage, shared by tests/test_aero_cpu.py (which runs them on
tests/aero_ref.py: the reference alone stays inside the bounds) and tests/test_gpu_aero.py (which runs
them on the kernels). A helper, not a test.

Bounds:
  coefficients  |got - ref| <= 4 * 2^-24 * S for the f32 goldens, 1e-12 * S for f64, S the sum of the
                absolute contributions (sum |F_el| or sum |M_el|) normalised like the coefficient: the only
                fp32 roundings that differ from the reference's are its fp32 edge length (<= 3 roundings)
                and the / 2 * 1e-2 scalar (fp32 or fp64 depending on the NumPy version); the rest is fp64
                on both sides.
  metrics       relative 16 * 2^-24 (f32) / 1e-12 (f64): d is bitwise the reference's and every summed term
                is non-negative, so the difference is the reference's fp32 squares and fp32 summation.
  NaN and 0 of the zero-target rules are matched exactly.
"""
import numpy as np

import aero_ref
from golden_util import load

EPS32 = 2.0 ** -24
COEF_TOL = {"f32": 4 * EPS32, "f64": 1e-12}
METRIC_TOL = {"f32": 16 * EPS32, "f64": 1e-12}


def _np(d):
    return {k: v.numpy() for k, v in d.items()}


def assert_metric(got, ref, tol, what):
    """NaN and exact zeros match exactly, everything else within the relative bound."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaN pattern {got} vs {ref}"
    assert np.array_equal(got == 0, ref == 0), f"{what}: zero pattern {got} vs {ref}"
    ok = ~np.isnan(ref)
    err = np.abs(got[ok] - ref[ok])
    rel = err / np.where(ref[ok] == 0, 1.0, np.abs(ref[ok]))
    print(f"{what}: max rel err {rel.max() if rel.size else 0.0:.3e} (bound {tol:.3e})")
    assert np.all(rel <= tol), f"{what}: rel err {rel.max():.3e} > {tol:.3e}"


def check_metrics_golden(prec, sums_fn):
    """sums_fn(pred, y, mean, std) -> [2, f, 6] float64 of one graph."""
    d, meta = load(f"evalmetrics_{prec}")
    d = _np(d)
    tol = METRIC_TOL[prec]
    all_sums, all_rows = [], []
    for i, rows in enumerate(meta["rows"]):
        sums = np.asarray(sums_fn(d[f"pred{i}"], d[f"y{i}"], d[f"mean{i}"], d[f"std{i}"]))
        assert sums.shape == (2, 4, 6)
        for s in (0, 1):
            errs, rr, feat = aero_ref.metrics(sums[s], rows)
            assert_metric(errs, d[f"errors{i}_s{s}"], tol, f"evalmetrics_{prec} case {i} scale {s} compute_errors")
            assert_metric(rr, d[f"rrmse{i}_s{s}"], tol, f"evalmetrics_{prec} case {i} scale {s} rrmse_percent")
            assert_metric(feat, d[f"feat{i}_s{s}"], tol, f"evalmetrics_{prec} case {i} scale {s} feature mae/mse")
        if i in meta["pooled_cases"]:
            all_sums.append(sums)
            all_rows.append(rows)
    tot = all_sums[0] + all_sums[1]  # graph order, fp64
    for s in (0, 1):
        feat = aero_ref.metrics(tot[s], float(sum(all_rows)))[2]
        assert_metric(feat, d[f"pooled_s{s}"], tol, f"evalmetrics_{prec} pooled scale {s}")
    # the zero-target rules of the cases built for them
    assert d["rrmse1_s0"] > 0 and np.all(d["feat1_s0"] > 0)           # a zero column only drops that feature
    assert np.isnan(d["errors2_s0"][3:]).all() and np.isnan(d["errors2_s1"][3:]).all()
    assert d["rrmse2_s0"] == 0 and d["rrmse2_s1"] == 0


def assert_coef(out, ref, den, tol, what):
    """out [4, 3] sums; ref the reference's coefficients in column order; den per coefficient."""
    for k, (slot, comp) in enumerate(what[1]):
        got = out[slot, comp] / den[k]
        S = out[slot + 2, comp] / den[k]
        err = abs(got - ref[k])
        print(f"{what[0]} coef {k}: got {got:.9e} ref {ref[k]:.9e} err {err:.3e} = {err / S / EPS32:.4f} * 2^-24 * S "
              f"(bound {tol * S:.3e})")
        assert err <= tol * S, f"{what[0]} coef {k}: |{got} - {ref[k]}| = {err:.3e} > {tol:.3e} * S = {tol * S:.3e}"


SLOTS_2D = ((0, 0), (0, 1), (1, 0))  # CA = Fx, CN = Fy, Cm = Mz
SLOTS_3D = ((0, 0), (0, 1), (0, 2))  # CA, CN, CY


def check_aero2d_golden(prec, forces_fn):
    """forces_fn(pressure [n], shear, normals, pos, edge_index, center or None) -> [4, 3] float64."""
    d, meta = load(f"aero2d_{prec}")
    d = _np(d)
    tol = COEF_TOL[prec]
    q, A = meta["dynamic_pressure"], meta["reference_area"]
    den = [A * q, A * q, A * 1.0 * q]
    for i in range(2):
        geo = (d[f"normals{i}"], d[f"pos{i}"], d[f"edge_index{i}"])
        for key, fld, ctr in (("coef_true", "phys_true", None), ("coef_pred", "phys_pred", None),
                              ("coef_true_center", "phys_true", meta["center"])):
            ph = d[f"{fld}{i}"]
            out = np.asarray(forces_fn(np.ascontiguousarray(ph[:, 0]), ph[:, 1:3], *geo, ctr))
            assert_coef(out, d[key][i], den, tol, (f"aero2d_{prec} case {i} {key}", SLOTS_2D))


def check_aero3d_golden(forces_fn):
    """forces_fn(pressure, shear, normals, areas) -> [4, 3] float64."""
    d, meta = load("aero3d_f32")
    d = _np(d)
    den = [meta["reference_area"] * meta["dynamic_pressure"]] * 3
    for key, p, sh in (("coef_true", "p", "shear"), ("coef_pred", "p_pred", "shear_pred")):
        out = np.asarray(forces_fn(d[p], d[sh], d["normals"], d["areas"]))
        assert_coef(out, d[key], den, COEF_TOL["f32"], (f"aero3d_f32 {key}", SLOTS_3D))


# the line patterns of errors.txt (inference.py:437, :461)
NUM = r"\s*-?\d+\.\d+"
TEST_MEAN_RE = (rf"TEST_MEAN \| rrmse:(?P<rrmse>{NUM}) \| nmae:(?P<nmae>{NUM}) \| nmse:(?P<nmse>{NUM}) \| "
                rf"mae:(?P<mae>{NUM}) \| mse:(?P<mse>{NUM})")
CASE_RE = (rf"case_(?P<id>\d{{3}}) \| rrmse:(?P<rrmse>{NUM}) \| nmae:(?P<nmae>{NUM}) \| nmse:(?P<nmse>{NUM}) \| "
           rf"mae:(?P<mae>{NUM}) \| mse:(?P<mse>{NUM})"
           rf" \| CA:(?P<ca_p>{NUM}) \((?P<ca_t>{NUM})\) \| CN:(?P<cn_p>{NUM}) \((?P<cn_t>{NUM})\) "
           rf"\| Cm:(?P<cm_p>{NUM}) \((?P<cm_t>{NUM})\)"
           rf" \| (?P<airfoil>.{{8,}}) \| (?P<mach>\S+\s*) \| (?P<alpha>\S+\s*)")
