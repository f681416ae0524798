"""The evaluation kernels on the MI355X (agn_eval_sums, agn_aero_forces through torch.ops.aerognn and
aerognn.aero) against tests/aero_ref.py and the reference's goldens.

Bounds (tests/aero_cases.py): against aero_ref 1e-12 of the absolute-sum scale (both
sides are fp64 sums of the same rounded terms, only the order differs); against the goldens
4 * 2^-24 * S (coefficients, f32), 16 * 2^-24 relative (metrics, f32), 1e-12 for f64; NaN and 0 of the
zero-target rules exactly; two calls bitwise equal; a graph of a batch bitwise equal to the graph alone.
Shapes are the smallest at which the chunk layout can go wrong: 1, 63, 65 rows, R - 1, R, R + 1 and
2 R + 7 for the kernels' chunk size R, empty graphs in the middle and at the end of a batch, a graph
boundary inside a chunk."""
import re
import types

import numpy as np
import pytest
import torch

import aero_cases
import aero_ref
from golden_util import load
from aero_cases import CASE_RE, TEST_MEAN_RE

pytestmark = pytest.mark.gpu

DEV = "cuda"
REF_TOL = 1e-12
MEAN = (1e5, 3.0, -2.0, 300.0)
STD = (3e4, 50.0, 50.0, 20.0)


def R():
    from aerognn import aero
    return aero.CHUNK_ROWS


def row_counts():
    r = R()
    return [1, 63, 65, r - 1, r, r + 1, 2 * r + 7]


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def stats_for(f, np_dtype):
    mean = np.resize(np.array(MEAN), f).astype(np_dtype)
    std = np.resize(np.array(STD), f).astype(np_dtype)
    return mean, std


def make_fields(n, f, np_dtype, seed):
    rng = np.random.default_rng(seed)
    y = rng.standard_normal((n, f)).astype(np_dtype)
    if n > 4:
        y[rng.integers(0, n, 3), 0] = 0.0  # exact zero targets: excluded from the relative sums
    pred = (y + 0.1 * rng.standard_normal((n, f))).astype(np_dtype)
    return pred, y


def gpu_sums(pred, y, mean, std, gptr=None):
    n = pred.shape[0]
    g = torch.tensor([0, n] if gptr is None else list(gptr), dtype=torch.int32, device=DEV)
    return torch.ops.aerognn.eval_sums(pred, y, mean, std, g)


def assert_sums_close(got, ref, what):
    """Non-negative sums: the value is its own absolute-sum scale; counts are exact."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, what
    np.testing.assert_array_equal(got[..., 3], ref[..., 3], err_msg=f"{what}: counts")
    err = np.abs(got - ref)
    assert np.all(err <= REF_TOL * np.abs(ref)), f"{what}: max rel err {np.max(err / np.maximum(np.abs(ref), 1e-300)):.3e}"


# ------------------------------------------------------------------ agn_eval_sums
def test_eval_sums_row_counts_vs_ref():
    mean, std = stats_for(4, np.float32)
    for n in row_counts():
        pred, y = make_fields(n, 4, np.float32, n)
        got = gpu_sums(dev(pred), dev(y), dev(mean), dev(std)).cpu().numpy()
        assert_sums_close(got, aero_ref.eval_sums(pred, y, mean, std), f"rows {n}")


@pytest.mark.parametrize("f", [1, 5, 16])
def test_eval_sums_feature_counts_vs_ref(f):
    n = 2 * R() + 7
    mean, std = stats_for(f, np.float32)
    pred, y = make_fields(n, f, np.float32, 100 + f)
    got = gpu_sums(dev(pred), dev(y), dev(mean), dev(std)).cpu().numpy()
    assert got.shape == (1, 2, f, 6)
    assert_sums_close(got, aero_ref.eval_sums(pred, y, mean, std), f"f {f}")


def test_eval_sums_fp64_vs_ref():
    n = R() + 1
    mean, std = stats_for(4, np.float64)
    pred, y = make_fields(n, 4, np.float64, 7)
    got = gpu_sums(dev(pred), dev(y), dev(mean), dev(std)).cpu().numpy()
    assert_sums_close(got, aero_ref.eval_sums(pred, y, mean, std), "fp64")


def test_eval_sums_batch_independent_and_repeatable():
    """Sizes R + 1, 0, 65, 0: an empty graph in the middle and one at the end, the third graph's first
    row inside what a batch-wide chunk layout would make chunk 1. Each graph's sums are bitwise the
    single-graph call's; a second call gives identical bytes; empty graphs give zeros."""
    sizes = [R() + 1, 0, 65, 0]
    gptr = np.concatenate([[0], np.cumsum(sizes)])
    n = int(gptr[-1])
    mean, std = stats_for(4, np.float32)
    pred, y = make_fields(n, 4, np.float32, 11)
    dp, dy, dm, ds = dev(pred), dev(y), dev(mean), dev(std)
    got = gpu_sums(dp, dy, dm, ds, gptr)
    again = gpu_sums(dp, dy, dm, ds, gptr)
    assert torch.equal(got.view(torch.int64), again.view(torch.int64))
    assert_sums_close(got.cpu().numpy(), aero_ref.eval_sums(pred, y, mean, std, gptr), "batch")
    for g, sz in enumerate(sizes):
        a, b = int(gptr[g]), int(gptr[g + 1])
        if sz == 0:
            assert not got[g].any()
            continue
        alone = gpu_sums(dp[a:b], dy[a:b], dm, ds)
        assert torch.equal(got[g].view(torch.int64), alone[0].view(torch.int64)), f"graph {g} differs from the graph alone"
    # the same through the public entry, from a PyG batch vector
    from aerognn import aero
    batch = torch.repeat_interleave(torch.arange(4, device=DEV), torch.tensor(sizes, device=DEV))
    es = aero.prediction_errors(dp, dy, {"target_mean": dm, "target_std": ds}, batch=batch, ngraph=4)
    assert torch.equal(es.sums.view(torch.int64), got.view(torch.int64))
    np.testing.assert_array_equal(es.cpu().rows, np.array(sizes, dtype=np.float64))


def test_eval_sums_strided_slice_and_bf16():
    n = 65
    mean, std = stats_for(4, np.float32)
    pred, y = make_fields(n, 4, np.float32, 13)
    wide = torch.zeros(n, 9, device=DEV)
    wide[:, 2:6] = dev(pred)
    sl = wide[:, 2:6]
    assert not sl.is_contiguous()
    got = gpu_sums(sl, dev(y), dev(mean), dev(std))
    ref = gpu_sums(dev(pred), dev(y), dev(mean), dev(std))
    assert torch.equal(got.view(torch.int64), ref.view(torch.int64))
    # bf16 inputs are widened to fp32 (exact): the sums of the widened values, bitwise
    pb, yb = dev(pred).bfloat16(), dev(y).bfloat16()
    got = gpu_sums(pb, yb, dev(mean), dev(std))
    ref = gpu_sums(pb.float(), yb.float(), dev(mean), dev(std))
    assert torch.equal(got.view(torch.int64), ref.view(torch.int64))
    assert_sums_close(got.cpu().numpy(), aero_ref.eval_sums(pb.float().cpu().numpy(), yb.float().cpu().numpy(), mean, std),
                      "bf16 widened")


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_eval_sums_vs_golden(prec):
    """The reference's compute_errors, compute_rrmse_percent and torch.mean expressions, zero-target
    NaN / 0 included."""
    aero_cases.check_metrics_golden(
        prec, lambda pred, y, mean, std: gpu_sums(dev(pred), dev(y), dev(mean), dev(std))[0].cpu().numpy())


# ------------------------------------------------------------------ agn_aero_forces
def loop_mesh(n, seed, np_dtype=np.float32, drop=None):
    """Closed loop of n nodes (n = 1: a single node, e = 0), both edge directions, shuffled."""
    rng = np.random.default_rng(seed)
    th = 2 * np.pi * (np.arange(n) + 0.25 * rng.random(n)) / n
    pos = np.stack([0.5 * (1 + np.cos(th)), 0.06 * np.sin(th) * (1.6 - np.cos(th))], 1)
    tan = np.roll(pos, -1, 0) - np.roll(pos, 1, 0)
    nrm = np.stack([tan[:, 1], -tan[:, 0]], 1) + 1e-9
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    if n < 3:
        ei = np.zeros((2, 0), dtype=np.int64)
    else:
        a = np.arange(n)
        b = (a + 1) % n
        ei = np.concatenate([np.stack([a, b]), np.stack([b, a])], 1)
        ei = ei[:, rng.permutation(ei.shape[1])]
        if drop is not None:
            ei = ei[:, ei[0] != drop]
    p = (1e5 + 3e4 * rng.standard_normal(n)).astype(np_dtype)
    sh = (50.0 * rng.standard_normal((n, 2))).astype(np_dtype)
    return pos.astype(np_dtype), nrm.astype(np_dtype), ei.astype(np.int64), p, sh


def gpu_forces(p, sh, nrm, pos=None, ei=None, areas=None, center=None, gptr=None):
    n = sh.shape[0]
    g = torch.tensor([0, n] if gptr is None else list(gptr), dtype=torch.int32, device=DEV)
    return torch.ops.aerognn.aero_forces(p, sh, nrm, pos, areas, ei, g, [] if center is None else list(center), 1e-2)


def assert_forces_close(got, ref, what):
    """Signed sums (rows 0, 1) within 1e-12 of their absolute-contribution sums (rows 2, 3)."""
    got, ref = np.asarray(got), np.asarray(ref)
    S = np.concatenate([ref[:, 2:4], ref[:, 2:4]], axis=1)
    err = np.abs(got - ref)
    assert np.all(err <= REF_TOL * S), f"{what}: max err / S {np.max(err / np.maximum(S, 1e-300)):.3e}"


def test_forces_2d_row_counts_vs_ref():
    for n in row_counts():
        pos, nrm, ei, p, sh = loop_mesh(n, n, drop=5 if n > 10 else None)
        out, area = gpu_forces(dev(p), dev(sh), dev(nrm), dev(pos), dev(ei), center=(0.25, 0.0))
        ra = aero_ref.node_areas(pos, ei)
        np.testing.assert_allclose(area.cpu().numpy(), ra, rtol=REF_TOL, atol=0, err_msg=f"areas, {n} nodes")
        if n > 10:
            assert area[5].item() == 0.0           # a node with no outgoing edge
        if n == 1:
            assert ei.shape[1] == 0 and not out.any()  # e = 0: no area, no force
        assert_forces_close(out.cpu().numpy(), aero_ref.forces(p, sh, nrm, ra, pos, (0.25, 0.0)), f"{n} nodes")


def test_forces_fp64_and_bf16():
    n = 65
    pos, nrm, ei, p, sh = loop_mesh(n, 3, np.float64)
    out, area = gpu_forces(dev(p), dev(sh), dev(nrm), dev(pos), dev(ei))
    ra = aero_ref.node_areas(pos, ei)
    np.testing.assert_allclose(area.cpu().numpy(), ra, rtol=REF_TOL, atol=0)
    assert_forces_close(out.cpu().numpy(), aero_ref.forces(p, sh, nrm, ra, pos), "fp64")
    tb = [dev(a).bfloat16() for a in (p, sh, nrm, pos)]
    got, ga = gpu_forces(*tb, dev(ei))
    ref, fa = gpu_forces(*[t.float() for t in tb], dev(ei))
    assert torch.equal(got.view(torch.int64), ref.view(torch.int64)) and torch.equal(ga, fa)


def test_forces_3d_given_areas_with_and_without_pos():
    rng = np.random.default_rng(5)
    n = R() + 1
    p = (100 * rng.standard_normal(n)).astype(np.float32)
    sh = rng.standard_normal((n, 3)).astype(np.float32)
    nrm = rng.standard_normal((n, 3)).astype(np.float32)
    pos = rng.standard_normal((n, 3)).astype(np.float32)
    areas = rng.random(n)
    ctr = (0.1, -0.2, 0.3)
    with_pos, a = gpu_forces(dev(p), dev(sh), dev(nrm), dev(pos), areas=dev(areas), center=ctr)
    assert a.numel() == 0
    assert_forces_close(with_pos.cpu().numpy(), aero_ref.forces(p, sh, nrm, areas, pos, ctr), "3-D with moments")
    out, _ = gpu_forces(dev(p), dev(sh), dev(nrm), None, areas=dev(areas))
    assert_forces_close(out.cpu().numpy(), aero_ref.forces(p, sh, nrm, areas), "3-D, pos=None")
    assert not out[:, 1].any() and not out[:, 3].any()
    from aerognn import aero
    fs = aero.integrate_forces(dev(p), dev(sh), dev(nrm), areas=dev(areas))
    assert fs.moment is None and fs.abs_moment is None and fs.force.shape == (1, 3)
    fs = aero.integrate_forces(dev(p), dev(sh), dev(nrm), pos=dev(pos), areas=dev(areas), moment_center=ctr)
    assert fs.moment.shape == (1, 3) and torch.equal(fs.moment, with_pos[:, 1]) and torch.equal(fs.abs_force, with_pos[:, 2])


def test_forces_batch_independent_and_repeatable():
    """Graphs of R + 1, 0, 65 and 0 nodes collated into one batch (node ids offset): every graph's row
    is bitwise the single-graph call's, the node areas too."""
    sizes = [R() + 1, 0, 65, 0]
    gptr = np.concatenate([[0], np.cumsum(sizes)])
    meshes = [loop_mesh(sz, 20 + g, drop=7) for g, sz in enumerate(sizes) if sz]
    offs = [int(gptr[0]), int(gptr[2])]
    pos = np.concatenate([m[0] for m in meshes])
    nrm = np.concatenate([m[1] for m in meshes])
    ei = np.concatenate([m[2] + o for m, o in zip(meshes, offs)], 1)
    ei = ei[:, np.random.default_rng(1).permutation(ei.shape[1])]  # the graphs' edges interleaved
    p = np.concatenate([m[3] for m in meshes])
    sh = np.concatenate([m[4] for m in meshes])
    args = (dev(p), dev(sh), dev(nrm), dev(pos), dev(ei))
    out, area = gpu_forces(*args, center=(0.25, 0.0), gptr=gptr)
    out2, area2 = gpu_forces(*args, center=(0.25, 0.0), gptr=gptr)
    assert torch.equal(out.view(torch.int64), out2.view(torch.int64)) and torch.equal(area, area2)
    assert not out[1].any() and not out[3].any()
    for g, o in zip((0, 2), offs):
        a, b = int(gptr[g]), int(gptr[g + 1])
        m_ei = ei[:, (ei[0] >= a) & (ei[0] < b)] - o  # the graph's edges in their batch order
        alone, area1 = gpu_forces(dev(p[a:b]), dev(sh[a:b]), dev(nrm[a:b]), dev(pos[a:b]), dev(m_ei), center=(0.25, 0.0))
        assert torch.equal(out[g].view(torch.int64), alone[0].view(torch.int64)), f"graph {g} differs from the graph alone"
        assert torch.equal(area[a:b], area1)
    from aerognn import aero
    np.testing.assert_array_equal(aero.node_areas(dev(pos), dev(ei)).cpu().numpy(), area.cpu().numpy())


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_coefficients_2d_vs_golden(prec):
    def forces(pressure, shear, normals, pos, ei, center):
        return gpu_forces(dev(pressure), dev(shear), dev(normals), dev(pos), dev(ei), center=center)[0][0].cpu().numpy()
    aero_cases.check_aero2d_golden(prec, forces)


def test_coefficients_3d_vs_golden():
    aero_cases.check_aero3d_golden(
        lambda p, sh, nrm, areas: gpu_forces(dev(p), dev(sh), dev(nrm), None, areas=dev(areas))[0][0].cpu().numpy())


def test_reference_named_functions_vs_golden():
    """calculate_aero_coefficients_2d / _3d with the reference's keys, the numbers of the goldens."""
    from aerognn import aero
    d, meta = load("aero2d_f32")
    data = types.SimpleNamespace(pos=d["pos0"].to(DEV), normals=d["normals0"].to(DEV), edge_index=d["edge_index0"].to(DEV))
    ph = d["phys_true0"].to(DEV)
    kw = dict(reference_area=meta["reference_area"], dynamic_pressure=meta["dynamic_pressure"])
    c = aero.calculate_aero_coefficients_2d(data, pressure=ph[:, 0:1], shear_stress=ph[:, 1:3], **kw)
    assert list(c) == ["CA", "CN", "Cm"] and all(isinstance(v, float) for v in c.values())
    s = aero.coefficients_2d_batch(data, ph[:, 0:1], ph[:, 1:3], **kw)
    for k, key in enumerate(("CA", "CN", "Cm")):
        assert abs(c[key] - float(d["coef_true"][0, k])) <= aero_cases.COEF_TOL["f32"] * s["S_" + key][0]
    ctr = np.array(meta["center"])
    cc = aero.calculate_aero_coefficients_2d(data, ph[:, 0:1], ph[:, 1:3], moment_center=ctr, **kw)
    sc = aero.coefficients_2d_batch(data, ph[:, 0:1], ph[:, 1:3], moment_center=ctr, **kw)
    assert abs(cc["Cm"] - float(d["coef_true_center"][0, 2])) <= aero_cases.COEF_TOL["f32"] * sc["S_Cm"][0]
    d3, m3 = load("aero3d_f32")
    c3 = aero.calculate_aero_coefficients_3d(d3["areas"].to(DEV), d3["normals"].to(DEV), d3["p_pred"].to(DEV),
                                             d3["shear_pred"].to(DEV), reference_area=m3["reference_area"],
                                             dynamic_pressure=m3["dynamic_pressure"])
    assert list(c3) == ["CA", "CN", "CY"]
    np.testing.assert_allclose([c3[k] for k in c3], d3["coef_pred"].numpy(), rtol=1e-6)


# ------------------------------------------------------------------ DeviceEvaluator
class _Stored(torch.nn.Module):
    """Stub model: returns the stored prediction of the case whose node features it is given."""

    def __init__(self, table):
        super().__init__()
        self.table = table
        self.anchor = torch.nn.Parameter(torch.zeros(1))

    def forward(self, x, edge_attr, edge_index):
        return self.table[x.shape[0]]


class _Case(types.SimpleNamespace):
    def to(self, device):
        return _Case(**{k: (v.to(device) if torch.is_tensor(v) else v) for k, v in vars(self).items()})


def test_device_evaluator_matches_the_reference_s_report():
    from aerognn.aero import DeviceEvaluator
    d, meta = load("aero2d_f32")
    feats = meta["output_features"]
    cases = [_Case(x=d[f"pos{i}"], edge_attr=None, edge_index=d[f"edge_index{i}"], pos=d[f"pos{i}"],
                   normals=d[f"normals{i}"], y=d[f"y{i}"], mach=meta["mach"], alpha=meta["alpha"][i],
                   airfoil=meta["airfoil"][i]) for i in range(2)]
    model = _Stored({c.x.shape[0]: d[f"pred{i}"].to(DEV) for i, c in enumerate(cases)}).to(DEV)
    ev = DeviceEvaluator(model, {"target_mean": d["target_mean"], "target_std": d["target_std"]},
                         {"dataset": {"name": "airfoil_2d", "output_features": feats}})
    mt, ct = aero_cases.METRIC_TOL["f32"], aero_cases.COEF_TOL["f32"]
    for i, c in enumerate(cases):
        info = ev.evaluate_case(c)
        assert list(info)[:5] == ["case_id", "rrmse_percent", "errors_physical", "errors_normalized", "coeff_str"]
        assert info["case_id"] == i and info["airfoil"] == meta["airfoil"][i] and info["mach"] == meta["mach"]
        assert list(info["errors_physical"]) == feats and list(info["errors_physical"]["p"]) == ["mae", "mse"]
        aero_cases.assert_metric(info["rrmse_percent"], d["rrmse"][i].numpy(), mt, f"case {i} rrmse")
        for key, g in (("errors_physical", "feat_phys"), ("errors_normalized", "feat_norm")):
            got = np.array([[info[key][f]["mae"], info[key][f]["mse"]] for f in feats])
            aero_cases.assert_metric(got, d[g][i].numpy(), mt, f"case {i} {key}")
    pooled = ev.test_set_mean()
    for key, g in (("errors_physical", "pooled_phys"), ("errors_normalized", "pooled_norm")):
        got = np.array([[pooled[key][f]["mae"], pooled[key][f]["mse"]] for f in feats])
        aero_cases.assert_metric(got, d[g].numpy(), mt, f"pooled {key}")
    # errors.txt: the reference's line pattern; numbers parsed back and compared as numbers, each within
    # the bound of its quantity plus half a unit of the last printed digit
    lines = ev.errors_txt().split("\n")
    m = re.fullmatch(TEST_MEAN_RE, lines[0])
    assert m and lines[1] == "" and len(lines) == 5 and lines[4] == ""

    def near(txt, ref, tol_abs, digits):
        assert abs(float(txt) - ref) <= tol_abs + 0.5 * 10.0 ** -digits + 1e-12 * abs(ref), (txt, ref)

    mean_of = lambda a, k: float(np.mean(a[:, k]))  # noqa: E731
    near(m.group("rrmse"), float(d["rrmse"].mean()), mt * float(d["rrmse"].mean()), 2)
    for name, arr, k, dig in (("nmae", "pooled_norm", 0, 6), ("nmse", "pooled_norm", 1, 6), ("mae", "pooled_phys", 0, 2),
                              ("mse", "pooled_phys", 1, 2)):
        ref = mean_of(d[arr].numpy(), k)
        near(m.group(name), ref, mt * ref, dig)
    q, A = meta["dynamic_pressure"], meta["reference_area"]
    for i in range(2):
        m = re.fullmatch(CASE_RE, lines[2 + i])
        assert m, lines[2 + i]
        assert int(m.group("id")) == i and m.group("airfoil").strip() == meta["airfoil"][i]
        assert m.group("mach").strip() == f"{meta['mach']:.2f}" and m.group("alpha").strip() == f"{meta['alpha'][i]:.2f}"
        near(m.group("rrmse"), float(d["rrmse"][i]), mt * float(d["rrmse"][i]), 2)
        for name, arr, k, dig in (("nmae", "feat_norm", 0, 6), ("nmse", "feat_norm", 1, 6), ("mae", "feat_phys", 0, 2),
                                  ("mse", "feat_phys", 1, 2)):
            ref = mean_of(d[arr][i].numpy(), k)
            near(m.group(name), ref, mt * ref, dig)
        St = ev_scales(cases[i], d[f"phys_true{i}"].to(DEV), A, q)
        Sp = ev_scales(cases[i], d[f"phys_pred{i}"].to(DEV), A, q)
        for k, nm in enumerate(("ca", "cn", "cm")):
            near(m.group(nm + "_t"), float(d["coef_true"][i, k]), ct * St[k], 4)
            near(m.group(nm + "_p"), float(d["coef_pred"][i, k]), ct * Sp[k], 4)


def ev_scales(case, phys, A, q):
    """Absolute-contribution scales of CA, CN, Cm for a case's physical fields."""
    from aerognn import aero
    c = case.to(DEV)
    s = aero.coefficients_2d_batch(c, phys[:, 0:1], phys[:, 1:3], reference_area=A, dynamic_pressure=q)
    return [float(s["S_CA"][0]), float(s["S_CN"][0]), float(s["S_Cm"][0])]
