"""The evaluation stage (aerognn.aero, torch.ops.aerognn.eval_sums / aero_forces) without a GPU: the
C-ABI symbols and their argument errors, the operators' fake kernels, the no-CPU-fallback rule, the
reference's signature, and tests/aero_ref.py against every golden (the numpy restatement of the
kernels' contracts alone stays inside the bounds the GPU tests hold the kernels to).
Numerics of the kernels: tests/test_gpu_aero.py."""
import ctypes
import inspect
import re
import types

import numpy as np
import pytest
import torch

import aero_cases
import aero_ref
from aero_cases import CASE_RE, TEST_MEAN_RE

NEW_SYMBOLS = ("agn_aero_chunk_rows", "agn_eval_sums_temp_bytes", "agn_eval_sums", "agn_aero_forces_temp_bytes",
               "agn_aero_forces")


def test_symbols_declared_and_exported():
    from aerognn import _lib
    names = _lib.exported_symbols()
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for sym in NEW_SYMBOLS:
        assert sym in names
        assert getattr(cdll, sym) is not None
        assert getattr(_lib.lib(), sym) is not None


def test_header_and_library_agree():
    """The chunk size the module exposes is the library's, the scratch helpers count what the header
    says (partials for ceil(n / R) + ngraph chunks), and the header names what each entry replaces."""
    import os
    from aerognn import _lib, aero
    L = _lib.lib()
    R = L.agn_aero_chunk_rows()
    assert R > 0 and aero.CHUNK_ROWS == R == aero.chunk_rows()
    for n, f, g in ((1, 1, 1), (R, 4, 1), (R + 1, 16, 3), (10 * R + 7, 5, 4)):
        cap = (n + R - 1) // R + g
        assert L.agn_eval_sums_temp_bytes(n, f, g) >= 8 * cap * 12 * f + 4 * (2 * g + 1)
        assert L.agn_aero_forces_temp_bytes(n, g) >= 8 * cap * 12 + 4 * (2 * g + 1)
    assert L.agn_eval_sums_temp_bytes(10, 17, 1) == 0
    hdr = open(os.path.join(os.path.dirname(_lib.__file__), "..", "..", "include", "aerognn.h")).read()
    for ref in ("inference.py:76-126", ":337-350", ":395-413", "utils.py:385-448", ":451-559"):
        assert ref in hdr


def test_argument_errors_need_no_device():
    from aerognn import _lib
    L = _lib.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ev = lambda dtype, n, f, ld, ptr=p, g=1: L.agn_eval_sums(dtype, n, f, ptr, ld, p, ld, p, p, p, g, p, p, None)  # noqa: E731
    assert ev(_lib.F32, -1, 4, 4) == -1          # AGN_E_ARG
    assert ev(_lib.F32, 1, 4, 4, None) == -1     # null pointer
    assert ev(_lib.BF16, 1, 4, 4) == -2          # AGN_E_DTYPE
    assert ev(_lib.F32, 1, 0, 4) == -4           # f outside 1..16
    assert ev(_lib.F32, 1, 17, 17) == -4
    assert ev(_lib.F32, 1, 4, 3) == -4           # row stride narrower than the row
    assert ev(_lib.F32, 0, 4, 4, None) == 0      # n == 0: no launch

    def fo(dtype=_lib.F32, n=1, dim=2, ld=2, areas=p, rowptr=None, pressure=p):
        return L.agn_aero_forces(dtype, n, dim, pressure, p, ld, p, ld, p, ld, areas, p, 0, rowptr, p, 1e-2, None, None,
                                 p, 1, p, p, None)
    assert fo(n=-1) == -1
    assert fo(pressure=None) == -1
    assert fo(dtype=_lib.F16) == -2
    assert fo(dim=4, ld=4) == -4                 # dim outside {2, 3}
    assert fo(dim=3, ld=2) == -4                 # row stride narrower than the row
    assert fo(areas=p, rowptr=p) == -4           # areas and mesh both given
    assert fo(areas=None, rowptr=None) == -4     # both missing
    assert fo(n=0) == 0


def test_op_schemas_and_fake_kernels():
    import aerognn.ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    for name in ("eval_sums", "aero_forces"):
        assert str(getattr(torch.ops.aerognn, name).default._schema).startswith(f"aerognn::{name}(")
    with FakeTensorMode():
        pred = torch.empty(10, 5, dtype=torch.bfloat16)
        gptr = torch.empty(4, dtype=torch.int32)
        s = torch.ops.aerognn.eval_sums(pred, pred, torch.empty(5), torch.empty(5), gptr)
        assert s.shape == (3, 2, 5, 6) and s.dtype == torch.float64
        p, sh = torch.empty(10), torch.empty(10, 2)
        ei = torch.empty(2, 30, dtype=torch.int64)
        out, area = torch.ops.aerognn.aero_forces(p, sh, sh, sh, None, ei, gptr, [0.25, 0.0], 1e-2)
        assert out.shape == (3, 4, 3) and out.dtype == torch.float64 and area.shape == (10,)
        sh3 = torch.empty(10, 3)
        out, area = torch.ops.aerognn.aero_forces(p, sh3, sh3, None, torch.empty(10, dtype=torch.float64), None, gptr,
                                                  [], 1e-2)
        assert out.shape == (3, 4, 3) and area.shape == (0,)


def test_cpu_tensors_raise():
    from aerognn import aero
    x = torch.ones(6, 4)
    stats = {"target_mean": torch.zeros(4), "target_std": torch.ones(4)}
    gptr = torch.tensor([0, 6], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="MI355X"):
        torch.ops.aerognn.eval_sums(x, x, stats["target_mean"], stats["target_std"], gptr)
    with pytest.raises(RuntimeError, match="MI355X"):
        aero.prediction_errors(x, x, stats)
    pos = torch.rand(6, 2)
    ei = torch.tensor([[0, 1, 2], [1, 2, 0]])
    with pytest.raises(RuntimeError, match="MI355X"):
        torch.ops.aerognn.aero_forces(torch.ones(6), pos, pos, pos, None, ei, gptr, [], 1e-2)
    with pytest.raises(RuntimeError, match="MI355X"):
        aero.node_areas(pos, ei)
    data = types.SimpleNamespace(pos=pos, normals=pos, edge_index=ei)
    with pytest.raises(RuntimeError, match="MI355X"):
        aero.calculate_aero_coefficients_2d(data, torch.ones(6, 1), pos)
    with pytest.raises(RuntimeError, match="MI355X"):
        aero.calculate_aero_coefficients_3d(torch.ones(6), torch.rand(6, 3), torch.ones(6), torch.rand(6, 3))


def test_coefficient_signatures_are_the_reference_s():
    """calculate_aero_coefficients_2d: the reference's parameters and defaults (utils.py:451-459)."""
    from aerognn import aero
    p = inspect.signature(aero.calculate_aero_coefficients_2d).parameters
    assert list(p) == ["test_data", "pressure", "shear_stress", "reference_area", "reference_length", "moment_center",
                       "dynamic_pressure"]
    assert [p[k].default for k in list(p)[3:]] == [1.0, 1.0, None, 1.0]
    assert all(p[k].default is inspect.Parameter.empty for k in list(p)[:3])
    q = inspect.signature(aero.calculate_aero_coefficients_3d).parameters
    assert list(q) == ["areas", "normals", "pressure", "shear_stress", "reference_area", "dynamic_pressure"]
    assert (q["reference_area"].default, q["dynamic_pressure"].default) == (1.0, 1.0)


def test_error_report_matches_aero_ref_and_handles_zero_targets():
    """ErrorReport (the host side of prediction_errors) on sums from aero_ref: the same numbers as
    aero_ref.metrics, NaN for relative metrics without a nonzero target, pooled = sums added."""
    from aerognn.aero import ErrorReport
    rng = np.random.default_rng(0)
    y = rng.standard_normal((40, 3)).astype(np.float32)
    y[25:, :] = 0
    pred = y + 0.1 * rng.standard_normal((40, 3)).astype(np.float32)
    mean, std = np.zeros(3, np.float32), np.array([2, 3, 4], np.float32)
    sums = aero_ref.eval_sums(pred, y, mean, std, [0, 25, 40])
    rep = ErrorReport(sums, np.array([25, 15]))
    for g, rows in ((0, 25), (1, 15)):
        for s, scale in ((0, "normalized"), (1, "physical")):
            errs, rr, feat = aero_ref.metrics(sums[g, s], rows)
            e = rep.compute_errors(g, scale)
            np.testing.assert_array_equal(np.array([e[k] for k in ("mae", "mse", "rmse", "relative_mae",
                                                                   "relative_rmse")]), errs)
            assert rep.rrmse_percent(g, scale) == rr
            fe = rep.feature_errors(g, scale, ["a", "b", "c"])
            np.testing.assert_array_equal(np.array([[fe[k]["mae"], fe[k]["mse"]] for k in "abc"]), feat)
    assert np.isnan(rep.compute_errors(1)["relative_mae"]) and rep.rrmse_percent(1) == 0.0
    pooled = rep.pooled(["a", "b", "c"])
    feat = aero_ref.metrics((sums[0] + sums[1])[1], 40.0)[2]
    np.testing.assert_array_equal(np.array([[pooled["errors_physical"][k]["mae"], pooled["errors_physical"][k]["mse"]]
                                            for k in "abc"]), feat)


# ------------------------------------------------------------------ aero_ref against the goldens
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_aero_ref_metrics_vs_golden(prec):
    aero_cases.check_metrics_golden(prec, lambda pred, y, mean, std: aero_ref.eval_sums(pred, y, mean, std)[0])


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_aero_ref_coefficients_2d_vs_golden(prec):
    def forces(pressure, shear, normals, pos, ei, center):
        return aero_ref.forces(pressure, shear, normals, aero_ref.node_areas(pos, ei), pos, center)[0]
    aero_cases.check_aero2d_golden(prec, forces)


def test_aero_ref_coefficients_3d_vs_golden():
    aero_cases.check_aero3d_golden(lambda p, sh, nrm, areas: aero_ref.forces(p, sh, nrm, areas)[0])


def test_golden_mesh_has_the_edge_cases():
    """Shuffled edges, both directions, one node without outgoing edges."""
    from golden_util import load
    d, meta = load("aero2d_f32")
    ei = d["edge_index1"].numpy()
    assert meta["dropped_node"] not in ei[0] and meta["dropped_node"] in ei[1]
    assert not np.all(np.diff(ei[0]) >= 0)
    assert aero_ref.node_areas(d["pos1"].numpy(), ei)[meta["dropped_node"]] == 0.0
    e0 = d["edge_index0"].numpy()
    assert {(int(a), int(b)) for a, b in e0.T} == {(int(b), int(a)) for a, b in e0.T}


def test_errors_txt_line_pattern():
    """DeviceEvaluator.errors_txt formats the reference's lines (inference.py:437-470); the numbers are
    checked on the GPU, the format here from stored case dictionaries."""
    from aerognn.aero import DeviceEvaluator, ErrorReport
    ev = DeviceEvaluator.__new__(DeviceEvaluator)
    ev.params = {"dataset": {"name": "airfoil_2d", "output_features": ["p", "t"]}}
    sums = aero_ref.eval_sums(np.ones((3, 2), np.float32), np.zeros((3, 2), np.float32) + 2, np.zeros(2, np.float32),
                              np.ones(2, np.float32))
    rep = ErrorReport(sums, np.array([3]))
    ev._reports = [rep]
    ev.cases = [{"case_id": 0, "rrmse_percent": rep.rrmse_percent(0), "coeff_str": " | CA: 0.1000 ( 0.2000) "
                 "| CN: 0.1000 ( 0.2000) | Cm:-0.1000 (-0.2000)",
                 "errors_physical": rep.feature_errors(0, "physical", ["p", "t"]),
                 "errors_normalized": rep.feature_errors(0, "normalized", ["p", "t"]),
                 "airfoil": "naca0012", "mach": 0.3, "alpha": 2.0}]
    lines = ev.errors_txt().split("\n")
    assert re.fullmatch(TEST_MEAN_RE, lines[0]) and lines[1] == ""
    m = re.fullmatch(CASE_RE, lines[2])
    assert m and float(m.group("rrmse")) == 50.0 and float(m.group("mae")) == 1.0 and m.group("mach") == "0.30"

