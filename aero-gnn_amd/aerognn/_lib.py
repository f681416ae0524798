"""ctypes binding of libaerognn.so (C-ABI declared in include/aerognn.h).

This is the drop-in boundary: every hot-path op of the reference's models/*.py is a call
through these entry points. There is deliberately NO fallback: if the shared library is
missing or a call fails, we raise.
"""
from __future__ import annotations

import ctypes as C
import os

from . import _header

_HERE = os.path.dirname(os.path.abspath(__file__))
# AEROGNN_LIB: an alternative build of the same library (A/B measurements only)
LIB_PATH = os.environ.get("AEROGNN_LIB") or os.path.join(_HERE, "libaerognn.so")

# The single definition of the boundary: constants, structs and prototypes are read from it at import.
HEADER = os.path.join(_HERE, "..", "..", "include", "aerognn.h")


class AeroGNNError(RuntimeError):
    pass


if not os.path.exists(HEADER):
    raise AeroGNNError(f"{HEADER} not found: the ctypes binding is derived from it")
with open(HEADER) as _f:
    CONSTS, STRUCTS, PROTOS = _header.parse(_f.read(), HEADER)

# Every AGN_X of the header as X (F32 .. F64, SEG_*, E_*, OPT_RESIDENT, MAX_LIN, MAX_SEG, MAX_WGRAD,
# ACT_NONE, ..) and every struct agn_x_y as the class XY (Seg, MlpFwdArgs, WgradDesc, ..): fields,
# order and pads are the header's, so positional construction follows the C declaration.
globals().update({k[4:]: v for k, v in CONSTS.items()})
globals().update({cls.__name__: cls for cls in STRUCTS.values()})
# the MLP hidden activation by its mlp.py:37 name
ACT = {k[8:].lower(): v for k, v in CONSTS.items() if k.startswith("AGN_ACT_") and v >= 0}

vp = C.c_void_p
i32 = C.c_int

_lib = None

# Entry points that enqueue device work on a stream. When core.PROF is a list, every call of one
# of them is bracketed by HIP events on the caller's current stream (the stream the launch goes
# to) and recorded under its name, unless an enclosing core.timed(...) already times it under a
# finer tag (edge_fwd, node_bwd, ...). Nothing is recorded when PROF is None.
LAUNCHES = ("agn_pack", "agn_mlp_forward", "agn_mlp_backward", "agn_reduce_partials", "agn_wgrad", "agn_wgrad_segsum", "agn_colsum",
            "agn_segment_sum", "agn_segment_sum2", "agn_gather_rows", "agn_radix_sort_u64", "agn_row_ptr", "agn_row_ptr_i64",
            "agn_iota_keys", "agn_level_index",
            "agn_exclusive_scan_i32", "agn_pool_sort_keys", "agn_pool_assign", "agn_pool_edge_candidates",
            "agn_pool_edge_sort", "agn_pool_edge_emit", "agn_bfs_distance", "agn_center_seed", "agn_maxdeg_seed",
            "agn_bistride_select", "agn_index_map", "agn_subgraph_edges", "agn_scatter_rows", "agn_wec_forward",
            "agn_wec_backward", "agn_edge_features", "agn_normalize", "agn_col_stats", "agn_collate",
            "agn_segment_max", "agn_segment_max_backward", "agn_edge_bwd_fused", "agn_encoder_bwd_fused", "agn_wgrad_reduce",
            "agn_edge_forward32", "agn_edge_agg_fixup",
            "agn_proj_forward", "agn_proj_backward", "agn_fourier_embed", "agn_fourier_embed_bwd", "agn_eval_sums",
            "agn_aero_forces", "agn_surface_forces", "agn_face_edges", "agn_mse_loss", "agn_adam_step", "agn_adam_step_master",
            "agn_act_dropout_fwd", "agn_act_dropout_bwd", "agn_mse_loss_scaled", "agn_grad_check", "agn_adam_step_scaled",
            "agn_adam_step_master_scaled", "agn_loss_scale_update")


class _Lib:
    """The loaded CDLL; launch entry points go through the optional event timer."""

    def __init__(self, cdll):
        self._cdll = cdll
        for name in LAUNCHES:
            if hasattr(cdll, name):
                setattr(self, name, _timed_launch(getattr(cdll, name), name[4:]))

    def __getattr__(self, name):
        return getattr(self._cdll, name)


def _timed_launch(f, tag):
    from . import core

    def call(*args):
        prof = core.PROF
        if prof is None or core._TIMED_DEPTH:
            return f(*args)
        import torch
        s = torch.cuda.Event(enable_timing=True)
        s.record()
        rc = f(*args)
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        prof.append((tag, None, s, e))
        return rc
    return call


def lib():
    """Load libaerognn.so (raises if it has not been built: no CPU fallback exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise AeroGNNError(
                f"{LIB_PATH} not found: build it with `make -C aero-gnn_amd/csrc` "
                "(or __graft_entry__.build()); the aerognn hot path has no CPU fallback")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in PROTOS.items():
            if os.environ.get("AEROGNN_LIB") and name.startswith("agn_debug_") and not hasattr(L, name):
                continue  # an older A/B build without a newer kernel's debug counter
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = _Lib(L)
    return _lib


def exported_symbols():
    """Names of every function include/aerognn.h declares (checked by the CPU test suite)."""
    return sorted(PROTOS)


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = lib().agn_error_string(rc).decode()
        raise AeroGNNError(f"aerognn {what} failed: {msg} (code {rc})")


def fault_status(reset=True) -> int:
    """The device fault word (include/aerognn.h agn_fault_status): nonzero if a bounded LDS-ring
    wait of agn_edge_bwd_fused gave up since the last reset. Synchronises the device."""
    v = i32(0)
    check(lib().agn_fault_status(C.byref(v), 1 if reset else 0), "fault_status")
    return int(v.value)


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()
