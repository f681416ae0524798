// Fused MLP chains on MFMA for the MeshGraphNet hot path (gfx950): agn_mlp_forward / agn_mlp_backward.
//
// One kernel evaluates a whole reference MLP — models/mlp.py:40-51 (Linear -> ReLU -> ... ->
// Linear -> LayerNorm) — for 32 rows per wave, with the layer-0 input assembled on the fly:
//   * EdgeBlockSum (models/mgnLayer.py:93-105): acc0 = P_s[src] + P_d[dst], input e, K = H,
//     then ReLU/Linear chain, LN, and the residual e' = e + LN(..) of mgnLayer.py:205;
//   * EdgeBlock    (mgnLayer.py:32-49): input cat[e, x[row], x[col]] via GATHER segments;
//   * NodeBlock    (mgnLayer.py:134-153): input cat[x, scatter_add(e', col)] where the SUM
//     segment reduces the receiver-grouped (CSC) rows of e' in edge order (bitwise the
//     torch_scatter summation order for fp32), residual x' = x + .. (mgnLayer.py:211);
//   * encoders / decoder / node projections: plain inputs.
// Activations never leave registers between layers (see common.hpp for the layout); only
// the block output (and, when training, the per-layer activations) are written to HBM.
//
// This file holds the two entry points: check the call, choose the I/O mode, offer the chain to
// the 32-row tile kernels and to the resident kernels, else launch the general kernel. The general
// kernels are in mlp_general.hpp, compiled per storage type in mlp_general_{f32,bf16,f16}.hip (the
// bf16 one also holds the resident kernels); the weight packer is in pack.hip.
#include "mlp_general.hpp"

namespace {

int g_opt_resident = 1;  // AGN_OPT_RESIDENT
// the chains the resident kernels (mlp_general_bf16.hip) run
bool res_fwd_ok(const agn_mlp_fwd_args* a, bool vec) {
  return g_opt_resident && vec && a->act_fn == AGN_ACT_RELU && a->dtype == AGN_BF16 && a->hidden == 128 && a->nlin <= RES_MAXL && a->nseg == 1 &&
         a->seg[0].kind == AGN_SEG_PLAIN && a->seg[0].k == 128 && a->out_dim == 128 && a->out_ld == 128 &&
         a->seg[0].ld % 8 == 0 && a->rows >= 64 * 1024;
}
bool res_bwd_ok(const agn_mlp_bwd_args* a, bool vec) {
  // edge/node chains with an H-wide dX, or any chain without dX (the edge encoder: d_e = 4 in)
  bool need_dx = false;
  for (int s = 0; s < a->din_nseg; ++s) need_dx |= a->din[s] != nullptr;
  // nlin == 1 with LayerNorm and no dX: the LayerNorm backward alone (G3 for agn_edge_bwd_fused)
  const bool din_ok = need_dx ? (a->din_nseg == 1 && a->in_dim == 128 && a->din_k[0] == 128)
                              : (a->nlin > 1 || a->use_ln);
  return g_opt_resident && vec && a->act_fn == AGN_ACT_RELU && a->dtype == AGN_BF16 && a->hidden == 128 &&
         a->nlin <= RES_MAXL && a->out_dim == 128 && din_ok && a->rows >= 64 * 1024;
}

// ------------------------------------------------------------------------- checks and mode choice
bool fwd_ptrs_aligned(const agn_mlp_fwd_args* a) {
  bool ok = al16(a->out) && al16(a->resid) && al16(a->proj) && al16(a->hpre);
  for (int s = 0; s < a->nseg; ++s) ok = ok && al16(a->seg[s].ptr) && al16(a->seg[s].store);
  for (int l = 0; l < a->nlin; ++l) ok = ok && al16(a->act[l]);
  return ok;
}
bool bwd_ptrs_aligned(const agn_mlp_bwd_args* a) {
  bool ok = al16(a->g) && al16(a->g2) && al16(a->hpre);
  for (int s = 0; s < a->din_nseg; ++s) ok = ok && al16(a->din[s]);
  for (int l = 0; l < a->nlin; ++l) ok = ok && al16(a->gpre[l]);
  return ok;
}

// The I/O mode (M_*) of a forward call with rows > 0 and valid counts, or the AGN_E_* code (< 0) of
// a chain no kernel runs.
int fwd_mode(const agn_mlp_fwd_args* a) {
  const bool out_full =
      (a->out_ld % 8 == 0) && (a->nlin == 1 ? (a->out_dim % a->hidden == 0) : (a->out_dim == a->hidden));
  bool in_full = true;
  bool wide = false;
  for (int s = 0; s < a->nseg; ++s) {
    if (a->seg[s].k < 1 || a->seg[s].ld < a->seg[s].k) return AGN_E_SHAPE;
    if (a->seg[s].k > a->hidden) {
      // wider than hidden: a PLAIN / GATHER row walked in column blocks (never next to the projections)
      if ((a->seg[s].kind != AGN_SEG_PLAIN && a->seg[s].kind != AGN_SEG_GATHER) || a->proj) return AGN_E_SHAPE;
      wide = true;
    }
    if (s + 1 < a->nseg && (a->seg[s].k % 32) != 0) return AGN_E_SHAPE;
    if (a->seg[s].k != a->hidden || a->seg[s].ld % 8 != 0) in_full = false;
  }
  if (a->nlin > 1 && a->out_dim > a->hidden) return AGN_E_SHAPE;
  if (a->use_ln && a->out_dim > a->hidden) return AGN_E_SHAPE;
  if (a->act_fn < AGN_ACT_RELU || a->act_fn > AGN_ACT_TANHSHRINK) return AGN_E_ARG;
  for (int l = 0; l < a->nlin; ++l)
    if (!al16(a->act[l]) || !al16(a->pre[l])) return AGN_E_ARG;  // activation buffers are always 16-B accessed
  if (wide) return M_WIDE;  // (never in_full, never M_NIN: always the masked-I/O mode)
  if (!fwd_ptrs_aligned(a)) return M_GEN;
  if (in_full && out_full) return M_VEC;
  if (out_full && a->nseg == 1 && (a->seg[0].kind == AGN_SEG_PLAIN || a->seg[0].kind == AGN_SEG_GATHER) &&
      a->seg[0].k <= 16)
    return M_NIN;
  if (in_full && a->nlin > 1 && a->out_dim <= 32 && !a->use_ln) return M_NOUT;
  return M_GEN;
}

// The same for a backward call. M_WIDE: a dX wider than hidden that is wanted.
int bwd_mode(const agn_mlp_bwd_args* a) {
  if (a->out_dim > a->hidden) return AGN_E_SHAPE;
  long kin = 0;
  bool wide = false;
  for (int s = 0; s < a->din_nseg; ++s) {
    if (a->din_k[s] < 1) return AGN_E_SHAPE;
    if (a->din_k[s] > a->hidden) {
      // wider than hidden: dX in column blocks into one [rows][k] buffer (no residual form)
      if (a->din_resid[s]) return AGN_E_SHAPE;
      wide = wide || a->din[s] != nullptr;
    }
    if (s + 1 < a->din_nseg && (a->din_k[s] % 32) != 0) return AGN_E_SHAPE;
    kin += a->din_k[s];
  }
  if (wide && kin > a->in_dim) return AGN_E_SHAPE;  // the blocks index W0^T's packed rows
  if (a->act_fn < AGN_ACT_RELU || a->act_fn > AGN_ACT_TANHSHRINK) return AGN_E_ARG;
  for (int l = 0; l + 1 < a->nlin; ++l) {
    // the ReLU backward reads the sign bits (AGN_RELU_MASK), the others the saved pre-activation
    if (a->act_fn == AGN_ACT_RELU ? !a->mask[l] : (!a->pre[l] || !al16(a->pre[l]))) return AGN_E_ARG;
    if (a->act_fn != AGN_ACT_RELU && a->tiled == 0 && a->hidden % 4) return AGN_E_SHAPE;
  }
  if (wide) return M_WIDE;  // the masked-I/O mode's WIDE instantiation
  if (!bwd_ptrs_aligned(a)) return M_GEN;
  if (a->out_dim == a->hidden) return M_VEC;
  if (a->out_dim <= 32 && !a->use_ln) return M_NOUT;
  return M_GEN;
}
}  // namespace

namespace agn {
int g_last_mode[2] = {-1, -1};  // mlp_general.hpp

int cu_count() {  // host.hpp
  static int cus = 0;
  if (cus == 0) {
    int dev = 0;
    hipDeviceProp_t p;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&p, dev) == hipSuccess) cus = p.multiProcessorCount;
    if (cus <= 0) cus = 256;
  }
  return cus;
}

bool node32_fwd_try(const agn_mlp_fwd_args* a, void* stream, int* rc);  // node32_fwd.hip
bool enc32_fwd_try(const agn_mlp_fwd_args* a, void* stream, int* rc);   // enc32_fwd.hip
bool dec32_fwd_try(const agn_mlp_fwd_args* a, void* stream, int* rc);   // enc32_fwd.hip
bool node32_bwd_try(const agn_mlp_bwd_args* a, void* stream, int* rc, int* ln_rows);  // node32_bwd.hip
bool dec32_bwd_try(const agn_mlp_bwd_args* a, void* stream, int* rc);                  // node32_bwd.hip
}  // namespace agn

extern "C" {

int agn_version(void) { return 1; }

int agn_set_option(int key, int value) {
  if (key == AGN_OPT_RESIDENT) {
    const int old = g_opt_resident;
    g_opt_resident = value ? 1 : 0;
    return old;
  }
  return AGN_E_ARG;
}

const char* agn_error_string(int code) {
  switch (code) {
    case 0: return "success";
    case AGN_E_ARG: return "invalid argument";
    case AGN_E_DTYPE: return "unsupported dtype (f32 / bf16 / f16)";
    case AGN_E_HIDDEN: return "unsupported hidden size (32, 64, 128)";
    case AGN_E_SHAPE: return "unsupported shape";
    default: return code > 0 ? hipGetErrorString((hipError_t)code) : "unknown error";
  }
}

int agn_debug_mlp_mode(int backward) { return g_last_mode[backward ? 1 : 0]; }

int agn_mlp_bwd_nwaves(int rows) {
  const int waves = (rows + 31) / 32;
  return (waves + WPB - 1) / WPB;
}

int agn_mlp_forward(const agn_mlp_fwd_args* a, void* stream) {
  if (!a || a->rows < 0 || a->nlin < 1 || a->nlin > AGN_MAX_LIN || a->nseg < 1 || a->nseg > AGN_MAX_SEG)
    return AGN_E_ARG;
  if (a->rows == 0) return 0;
  const int mode = fwd_mode(a);
  if (mode < 0) return mode;
  g_last_mode[0] = -1;
  int rc = 0;
  if (g_opt_resident) {  // the 32-row tile kernels, resident weights:
    // a processor layer's node MLP (aggregation walked in), an encoder on narrow rows, the decoder to <= 32 outputs
    if (mode == M_VEC && node32_fwd_try(a, stream, &rc)) return rc;
    if (mode == M_NIN && enc32_fwd_try(a, stream, &rc)) return rc;
    if (mode == M_NOUT && dec32_fwd_try(a, stream, &rc)) return rc;
  }
  if (res_fwd_ok(a, mode == M_VEC)) return mlp_resident_fwd(*a, stream);
  switch (a->dtype) {
    case AGN_F32: return mlp_general_fwd_f32(*a, mode, stream);
    case AGN_BF16: return mlp_general_fwd_bf16(*a, mode, stream);
    case AGN_F16: return mlp_general_fwd_f16(*a, mode, stream);
    default: return AGN_E_DTYPE;
  }
}

int agn_mlp_backward(const agn_mlp_bwd_args* a, void* stream) {
  if (!a || a->rows < 0 || a->nlin < 1 || a->nlin > AGN_MAX_LIN || a->din_nseg < 0 || a->din_nseg > AGN_MAX_SEG)
    return AGN_E_ARG;
  if (a->rows == 0) return 0;
  const int mode = bwd_mode(a);
  if (mode < 0) return mode;
  // ln_rows (the rows of ln_partial the kernel wrote) is the call's one output field
  agn_mlp_bwd_args* am = const_cast<agn_mlp_bwd_args*>(a);
  g_last_mode[1] = -1;
  int rc = 0, lr = 0;
  if (g_opt_resident && mode == M_VEC && node32_bwd_try(a, stream, &rc, &lr)) {  // a processor layer's node MLP
    am->ln_rows = lr;
    return rc;
  }
  if (g_opt_resident && mode == M_NOUT && dec32_bwd_try(a, stream, &rc)) {  // the decoder from H-wide rows
    am->ln_rows = agn_mlp_bwd_nwaves(a->rows);
    return rc;
  }
  if (res_bwd_ok(a, mode == M_VEC)) return mlp_resident_bwd(*a, stream, &am->ln_rows);
  am->ln_rows = agn_mlp_bwd_nwaves(a->rows);
  switch (a->dtype) {
    case AGN_F32: return mlp_general_bwd_f32(*a, mode, stream);
    case AGN_BF16: return mlp_general_bwd_bf16(*a, mode, stream);
    case AGN_F16: return mlp_general_bwd_f16(*a, mode, stream);
    default: return AGN_E_DTYPE;
  }
}

}  // extern "C"
