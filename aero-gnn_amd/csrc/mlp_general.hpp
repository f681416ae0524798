// The general fused-MLP kernels (mlp_fwd_kernel / mlp_bwd_kernel): any hidden width of 32, 64 or
// 128, float32 / bfloat16 / float16 storage, every I/O mode and activation. One kernel evaluates a
// whole reference MLP (models/mlp.py:40-51) for 32 rows per wave, 4 waves (128 rows) per block, with
// each layer's packed weights staged in LDS once per block; mlp.hip describes the chain and chooses
// the mode.
//
// 162 instantiations make this the slowest code of the library to compile, so each storage type is
// a translation unit of its own (mlp_general_{f32,bf16,f16}.hip), which instantiates launch_fwd /
// launch_bwd below for its type and exports them as agn::mlp_general_{fwd,bwd}_<type>. mlp.hip
// includes this header for those declarations and for the helpers its resident kernels share.
#pragma once
#include <type_traits>
#include "tile32.hpp"
#include "aerognn.h"

namespace agn {
// The general kernel of a chain in one storage type (mlp_general_<type>.hip), `mode` as chosen by
// mlp.hip: the launch status, or AGN_E_HIDDEN for a width other than 32 / 64 / 128. Hidden: the
// library's exported symbols stay those of include/aerognn.h.
#define AGN_HIDDEN __attribute__((visibility("hidden")))
AGN_HIDDEN int mlp_general_fwd_f32(const agn_mlp_fwd_args& a, int mode, void* stream);
AGN_HIDDEN int mlp_general_bwd_f32(const agn_mlp_bwd_args& a, int mode, void* stream);
AGN_HIDDEN int mlp_general_fwd_bf16(const agn_mlp_fwd_args& a, int mode, void* stream);
AGN_HIDDEN int mlp_general_bwd_bf16(const agn_mlp_bwd_args& a, int mode, void* stream);
AGN_HIDDEN int mlp_general_fwd_f16(const agn_mlp_fwd_args& a, int mode, void* stream);
AGN_HIDDEN int mlp_general_bwd_f16(const agn_mlp_bwd_args& a, int mode, void* stream);
// The resident-weight kernels (mlp_general_bf16.hip) for the chains mlp.hip found eligible: bf16,
// H = 128, every layer H -> H, at most RES_MAXL Linears. ln_rows: the rows of ln_partial written.
constexpr int RES_MAXL = 4;
AGN_HIDDEN int mlp_resident_fwd(const agn_mlp_fwd_args& a, void* stream);
AGN_HIDDEN int mlp_resident_bwd(const agn_mlp_bwd_args& a, void* stream, int* ln_rows);
// agn_debug_mlp_mode: the I/O mode of the last general-kernel launch per direction ([0] forward,
// [1] backward), -1 after a call that went to another kernel. Host-side only; defined in mlp.hip.
AGN_HIDDEN extern int g_last_mode[2];
#undef AGN_HIDDEN
}  // namespace agn

using namespace agn;

namespace {

constexpr int WPB = 4;           // waves per block
constexpr int BLOCK = 64 * WPB;  // 128 data rows per block

template <typename T, int NT>
constexpr int lds_units() { return NT * (nrk(32 * NT) / BOp<T, 16>::RPU) * 64; }

// Stage the packed A fragments of out tiles [ot0, ot0+otn) x K units [unit0, unit0+nu) of a
// packed matrix with `ku_total` units per tile into LDS as [otn][nu][64] (16 B each).
AGN_DEV void stage_block(uint4* lds, const void* gw, int ku_total, int ot0, int otn, int unit0, int nu) {
  const uint4* g = reinterpret_cast<const uint4*>(gw);
  const int per = nu * 64;
  const int n = otn * per;
  for (int i = threadIdx.x; i < n; i += BLOCK) {
    const int ot = i / per, rem = i - ot * per;
    lds[i] = g[((size_t)(ot0 + ot) * ku_total + unit0) * 64 + rem];
  }
}

// Row I/O in acc layout. VEC: k == 32*NT features, 16-B aligned rows -> 16-B per-lane
// accesses through lane-half exchanges (common.hpp load8_w/store8_w; all lanes of a row pair
// must be active together). !VEC: masked 4-feature chunks.
template <typename T, int NR, bool VEC>
AGN_DEV void load_row(float (&v)[NR], const T* rowp, int k, int h) {
  if constexpr (VEC) {
    load_row_w<T, NR>(v, rowp, h);
  } else {
#pragma unroll
    for (int q = 0; q < NR / 4; ++q) {
      const f32x4 x = load4_masked(rowp, 8 * q + 4 * h, k, false);
      v[4 * q] = x[0]; v[4 * q + 1] = x[1]; v[4 * q + 2] = x[2]; v[4 * q + 3] = x[3];
    }
  }
}
template <typename T, int NR, bool VEC>
AGN_DEV void add_row(float (&v)[NR], const T* rowp, int k, int h) {
  if constexpr (VEC) {
    add_row_w<T, NR>(v, rowp, h);
  } else {
#pragma unroll
    for (int q = 0; q < NR / 4; ++q) {
      const f32x4 x = load4_masked(rowp, 8 * q + 4 * h, k, false);
      v[4 * q] += x[0]; v[4 * q + 1] += x[1]; v[4 * q + 2] += x[2]; v[4 * q + 3] += x[3];
    }
  }
}
template <typename T, int NR, bool VEC>
AGN_DEV void store_row(T* rowp, int k, const float (&v)[NR], int h, bool valid) {
  if constexpr (VEC) {
    store_row_w<T, NR>(rowp, v, h, valid);
  } else if (valid) {
#pragma unroll
    for (int q = 0; q < NR / 4; ++q) {
      const f32x4 x = {v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
      store4_masked(rowp, 8 * q + 4 * h, k, false, x);
    }
  }
}

template <int NT, int NR>
AGN_DEV void acc_to_regs(float (&v)[NR], const f32x16 (&acc)[NT]) {
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) v[16 * t + r] = acc[t][r];
}

template <int NT, bool FULL>
AGN_DEV void acc_bias(f32x16 (&acc)[NT], const float* b, int nvalid, int h) {
  float v[16 * NT];
  if (FULL && b) load_param<16 * NT, true>(v, b, nvalid, h);
  else load_param<16 * NT, false>(v, b, nvalid, h);
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = v[16 * t + r];
}

// Load one input segment for data row `rr` into acc-layout registers.
template <typename T, int NR, bool VEC>
AGN_DEV void load_segment(float (&in)[NR], const agn_seg& s, int rr, bool valid, int h) {
  const T* base = reinterpret_cast<const T*>(s.ptr);
  if (s.kind == AGN_SEG_PLAIN || s.kind == AGN_SEG_GATHER) {
    const int r = (s.kind == AGN_SEG_GATHER) ? s.index[rr] : rr;
    load_row<T, NR, VEC>(in, base + (size_t)r * s.ld, s.k, h);
  } else {  // SUM / MEAN over rows index[rr] .. index[rr+1]-1 (receiver-grouped edges)
#pragma unroll
    for (int i = 0; i < NR; ++i) in[i] = 0.f;
    const int beg = s.index[rr], end = s.index[rr + 1];
    for (int j = beg; j < end; ++j) add_row<T, NR, VEC>(in, base + (size_t)j * s.ld, s.k, h);
    if (s.kind == AGN_SEG_MEAN) {
      const float cnt = (float)max(end - beg, 1);
#pragma unroll
      for (int i = 0; i < NR; ++i) in[i] = in[i] / cnt;
    }
#pragma unroll
    for (int i = 0; i < NR; ++i) in[i] = round_t<T>(in[i]);
    if (s.store) store_row<T, NR, VEC>(reinterpret_cast<T*>(s.store) + (size_t)rr * s.k, s.k, in, h, valid);
  }
}

// Columns [c0, c0 + kb) of a PLAIN / GATHER segment wider than the hidden size (kb <= NR * 2
// features, masked: neither c0 nor the row stride need keep the row 16-B aligned).
template <typename T, int NR>
AGN_DEV void load_segment_block(float (&in)[NR], const agn_seg& s, int rr, int h, int c0, int kb) {
  const int r = (s.kind == AGN_SEG_GATHER) ? s.index[rr] : rr;
  load_row<T, NR, false>(in, reinterpret_cast<const T*>(s.ptr) + (size_t)r * s.ld + c0, kb, h);
}

// ------------------------------------------------------------------------- forward
// I/O modes of the general kernels (compile-time, chosen on the host per call):
//   M_VEC : every input segment and the output are H wide (16-B row I/O everywhere)
//   M_NIN : one PLAIN or GATHER input of k <= 16 features (encoders: d_n = 6, d_e = 4), output H wide
//   M_NOUT: H-wide inputs, nlin > 1, output of <= 32 features, no LayerNorm (decoder: d_out = 4)
//   M_GEN : anything else (masked 4-feature chunks)
// M_WIDE (host-side only) selects the WIDE instantiations of M_GEN: a PLAIN / GATHER input segment
// (forward) or a dX segment (backward) wider than H, walked in H-wide column blocks. They are
// instantiations of their own so that the code of every other shape stays what it was.
enum { M_VEC = 0, M_GEN = 1, M_NIN = 2, M_NOUT = 3, M_WIDE = 4 };

// k <= 16 features of one row into acc-layout registers (features >= k and >= 16 are zero)
template <typename T, int NR>
AGN_DEV void load_row_narrow(float (&v)[NR], const T* rowp, int k, int h) {
#pragma unroll
  for (int i = 0; i < NR; ++i) v[i] = 0.f;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const f32x4 x = load4_masked(rowp, 8 * q + 4 * h, k, false);
    v[4 * q] = x[0]; v[4 * q + 1] = x[1]; v[4 * q + 2] = x[2]; v[4 * q + 3] = x[3];
  }
}

// load_segment's SUM / MEAN walk with two member rows' loads in flight per step (adds in edge
// order, one rounding: the same values). Run before anything else of the wave is live.
template <int NR>
AGN_DEV void walk2_segment(float (&in)[NR], const agn_seg& s, int rr, bool valid, int h) {
  const bf16* base = reinterpret_cast<const bf16*>(s.ptr);
#pragma unroll
  for (int i = 0; i < NR; ++i) in[i] = 0.f;
  const int beg = s.index[rr], end = s.index[rr + 1];
  int j = beg;
  for (; j + 1 < end; j += 2) {
    uint4 r0[NR / 8], r1[NR / 8];
    const bf16* p0 = base + (size_t)j * s.ld;
    const bf16* p1 = p0 + s.ld;
#pragma unroll
    for (int i = 0; i < NR / 8; ++i) r0[i] = *reinterpret_cast<const uint4*>(p0 + 16 * i + 8 * h);
#pragma unroll
    for (int i = 0; i < NR / 8; ++i) r1[i] = *reinterpret_cast<const uint4*>(p1 + 16 * i + 8 * h);
#pragma unroll
    for (int i = 0; i < NR / 8; ++i) {
      float o[8];
      unpack8_w(o, r0[i]);  // load8_w's exchange + conversion
#pragma unroll
      for (int e = 0; e < 8; ++e) in[8 * i + e] += o[e];
    }
#pragma unroll
    for (int i = 0; i < NR / 8; ++i) {
      float o[8];
      unpack8_w(o, r1[i]);
#pragma unroll
      for (int e = 0; e < 8; ++e) in[8 * i + e] += o[e];
    }
  }
  if (j < end) add_row_w<bf16, NR>(in, base + (size_t)j * s.ld, h);
  if (s.kind == AGN_SEG_MEAN) {
    const float cnt = (float)max(end - beg, 1);
#pragma unroll
    for (int i = 0; i < NR; ++i) in[i] = in[i] / cnt;
  }
#pragma unroll
  for (int i = 0; i < NR; ++i) in[i] = round_t<bf16>(in[i]);
  if (s.store) store_row<bf16, NR, true>(reinterpret_cast<bf16*>(s.store) + (size_t)rr * s.k, s.k, in, h, valid);
}

// A hidden activation other than ReLU (AGN_ACT_*): the Linear output rounded to T, saved to pre
// (the backward's x) when given, the activation applied in fp32 and packed (rounded) into b
template <typename T, int NT, int NR, bool MORE>
AGN_DEV void set_act(BOp<T, NR>& b, const f32x16 (&acc)[NT], int k, T* pre, int tiled, int row, int h, bool valid) {
  constexpr int H = 32 * NT;
  float v[NR];
#pragma unroll
  for (int i = 0; i < NR; ++i) v[i] = round_t<T>(acc[i / 16][i % 16]);
  if (pre) {
    BOp<T, NR> pb;
    pb.set(v);
    if (tiled) pb.store_tiled(pre, row, h, valid);
    else pb.store(pre + (size_t)row * H, h, valid);
  }
#pragma unroll
  for (int i = 0; i < NR; ++i) v[i] = act_fwd<MORE>(k, v[i]);
  b.set(v);
}

// GACT: a hidden activation other than ReLU (agn_mlp_*_args.act_fn): 1 = gelu / silu / tanh, 2 = any
// later code (gact_of); the ReLU instantiations carry none of its registers, and the GACT = 1 ones
// none of the later functions' code
template <typename T, int NT, int MODE, int GACT, bool WIDE = false>
__global__ __launch_bounds__(BLOCK, 2) void mlp_fwd_kernel(const agn_mlp_fwd_args a) {
  static_assert(!WIDE || MODE == M_GEN, "wide segments run on the masked-I/O mode");
  constexpr int H = 32 * NT;
  constexpr int NR = 16 * NT;
  constexpr int NUH = nrk(H) / BOp<T, NR>::RPU;  // K units of an H-wide input
  constexpr bool IN_FULL = (MODE == M_VEC || MODE == M_NOUT);
  constexpr bool OUT_FULL = (MODE == M_VEC || MODE == M_NIN);
  __shared__ uint4 wl[lds_units<T, NT>()];
  const int lane = threadIdx.x & 63;
  const int c = lane & 31, h = lane >> 5;
  const int wave = blockIdx.x * WPB + (threadIdx.x >> 6);
  const int row = wave * 32 + c;
  const bool valid = row < a.rows;
  const int rr = valid ? row : a.rows - 1;

  f32x16 acc[NT];
  float v[NR];
  BOp<T, NR> b;

  int k0 = 0;
  for (int s = 0; s < a.nseg; ++s) k0 += a.seg[s].k;
  const int ku0 = units_k<T>(k0);
  // a node MLP's SUM / MEAN input is walked first, while nothing else of the wave is live, and
  // kept packed until its GEMM (the layer-0 GEMM order, hence every sum, is unchanged)
  constexpr bool W2 = MODE == M_VEC && std::is_same<T, bf16>::value && NT == 4;
  const bool walk2 = W2 && a.nseg == 2 && (a.seg[1].kind == AGN_SEG_SUM || a.seg[1].kind == AGN_SEG_MEAN) &&
                     a.seg[1].k == H;
  BOp<T, NR> bagg;
  if constexpr (W2) {
    if (walk2) {
      walk2_segment<NR>(v, a.seg[1], rr, valid, h);
      bagg.set(v);
    }
  }
  const int ngrp = (a.nlin == 1) ? (a.out_dim + H - 1) / H : 1;

  for (int grp = 0; grp < ngrp; ++grp) {
    const int out0 = (a.nlin == 1) ? a.out_dim : H;
    const int gofs = grp * H;
    const int nv0 = min(H, out0 - gofs);
    const int otn0 = (nv0 + 31) / 32;
    // ---- layer-0 accumulator init: bias, or the EdgeBlockSum projections gathered by src/dst
    if (a.proj) {
      const T* P = reinterpret_cast<const T*>(a.proj);
      const T* ps = P + (size_t)a.src[rr] * (2 * H);
      const T* pd = P + (size_t)a.dst[rr] * (2 * H) + H;
      // one 16-feature pair per round: keeps the gathered rows from all being live at once
#pragma unroll
      for (int i = 0; i < NR / 8; ++i) {
        cbarrier();
        float x[8], y[8];
        load8_w(x, ps, i, h);
        load8_w(y, pd, i, h);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[(8 * i + e) / 16][(8 * i + e) % 16] = x[e] + y[e];
      }
    } else {
      acc_bias<NT, OUT_FULL || MODE == M_NOUT>(acc, a.bias[0] ? a.bias[0] + gofs : nullptr, nv0, h);
    }
    // ---- layer 0: sum over input segments. WIDE: a PLAIN / GATHER segment wider than H is walked
    // in H-wide column blocks (the last may be narrow), one stage_block of W0 per block: the
    // products and their order are those of consecutive H-wide segments
    int unit = 0;
    for (int s = 0; s < a.nseg; ++s) {
      for (int c0 = 0; c0 < (WIDE ? a.seg[s].k : 1); c0 += H) {
        const int kb = WIDE ? min(H, a.seg[s].k - c0) : a.seg[s].k;
        const int nu = units_k<T>(kb);
        __syncthreads();
        stage_block(wl, a.wpk[0], ku0, grp * NT, otn0, unit, nu);
        if constexpr (MODE == M_NIN) {  // PLAIN, or GATHER (the caller's row order permuted in the load)
          const int src_row = a.seg[s].kind == AGN_SEG_GATHER ? a.seg[s].index[rr] : rr;
          load_row_narrow<T, NR>(v, reinterpret_cast<const T*>(a.seg[s].ptr) + (size_t)src_row * a.seg[s].ld, a.seg[s].k, h);
        } else {
          // (the two flags are what is left of a removed staging path: a tidier spelling of this
          // site changes the assembly of the walk2 instantiations, so its statements stay)
          bool staged = false;
          if (!staged) {
            if (W2 && walk2 && s == 1) staged = true;
            else if (WIDE && a.seg[s].k > H) load_segment_block<T, NR>(v, a.seg[s], rr, h, c0, kb);
            else load_segment<T, NR, IN_FULL>(v, a.seg[s], rr, valid, h);
          }
        }
        bool staged_b = false;
        if (W2 && walk2 && s == 1) b = bagg;
        else if (!staged_b) b.set(v);
        __syncthreads();
        if constexpr (IN_FULL) gemm<T, NT, NR, true>(acc, b, NUH, wl, NUH, NT, lane);
        else if constexpr (MODE == M_NIN) gemm<T, NT, NR, true>(acc, b, nu, wl, nu, NT, lane);
        else gemm<T, NT, NR>(acc, b, nu, wl, nu, otn0, lane);
        unit += nu;
      }
    }
    // ---- hidden layers: relu(acc) -> packed operand -> next Linear (registers only)
    for (int l = 1; l < a.nlin; ++l) {
      const bool last = (l == a.nlin - 1);
      const int outl = last ? a.out_dim : H;
      const int otn = (outl + 31) / 32;
      __syncthreads();
      stage_block(wl, a.wpk[l], NUH, 0, otn, 0, NUH);
      if constexpr (GACT != 0) set_act<T, NT, NR, GACT == 2>(b, acc, a.act_fn, reinterpret_cast<T*>(a.pre[l - 1]), a.tiled, row, h, valid);
      else b.template set_relu<NT>(acc);
      if (a.act[l - 1]) {
        if (a.tiled) b.store_tiled(reinterpret_cast<T*>(a.act[l - 1]), row, h, valid);
        else b.store(reinterpret_cast<T*>(a.act[l - 1]) + (size_t)row * H, h, valid);
      }
      // waves past the last 32-row tile (the grid rounds up to WPB waves) own no mask tile
      if (!GACT && a.mask[l - 1] && wave * 32 < a.rows)
        store_relu_mask<T, NR>(a.mask[l - 1], b, wave, lane);
      if (OUT_FULL || !last) acc_bias<NT, true>(acc, a.bias[l], H, h);
      else acc_bias<NT, false>(acc, a.bias[l], outl, h);
      __syncthreads();
      if (OUT_FULL || !last) gemm<T, NT, NR, true>(acc, b, NUH, wl, NUH, NT, lane);
      else gemm<T, NT, NR>(acc, b, NUH, wl, NUH, otn, lane);
    }
    // ---- epilogue: LayerNorm, residual, store
    const int outd = (a.nlin == 1) ? nv0 : a.out_dim;
    float mean = 0.f, rstd = 1.f;
    if (MODE != M_NOUT && a.use_ln) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < NR; ++i) s += (OUT_FULL || feat_of(i, h) < outd) ? acc[i / 16][i % 16] : 0.f;
      s = sum32(s);
      mean = s / (float)outd;
      float q = 0.f;
#pragma unroll
      for (int i = 0; i < NR; ++i) {
        const float d = acc[i / 16][i % 16] - mean;
        if (OUT_FULL || feat_of(i, h) < outd) q = ln_sq_acc(q, d);
      }
      q = sum32(q);
      rstd = 1.0f / sqrtf(q / (float)outd + 1e-5f);
      if (a.stats && valid && h == 0) {
        a.stats[2 * (size_t)row] = mean;
        a.stats[2 * (size_t)row + 1] = rstd;
      }
    }
    T* hp = a.hpre ? reinterpret_cast<T*>(a.hpre) + (size_t)row * outd : nullptr;
    const T* rp = a.resid ? reinterpret_cast<const T*>(a.resid) + (size_t)rr * a.out_ld + gofs : nullptr;
    T* op = reinterpret_cast<T*>(a.out) + (size_t)row * a.out_ld + gofs;
    if constexpr (OUT_FULL) {
#pragma unroll
      for (int i = 0; i < NR / 8; ++i) {
        float v8[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v8[e] = acc[(8 * i + e) / 16][(8 * i + e) % 16];
        if (a.use_ln) {
          if (hp) {
            if (a.tiled) store8_tiled<T, NR>(reinterpret_cast<T*>(a.hpre), i, row, h, v8, valid);
            else store8_w(hp, i, h, v8, valid);
          }
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const int f0 = 16 * i + 8 * j + 4 * h;
            const f32x4 g4 = *reinterpret_cast<const f32x4*>(a.ln_g + f0);
            const f32x4 b4 = *reinterpret_cast<const f32x4*>(a.ln_b + f0);
#pragma unroll
            for (int e = 0; e < 4; ++e) v8[4 * j + e] = ln_out(v8[4 * j + e], mean, rstd, g4[e], b4[e]);
          }
        }
        if (rp) {
          float r8[8];
          load8_w(r8, rp, i, h);
#pragma unroll
          for (int e = 0; e < 8; ++e) v8[e] = round_t<T>(v8[e]) + r8[e];
        }
        store8_w(op, i, h, v8, valid);
      }
    } else {
      // M_NOUT: only the first 32 features (acc tile 0) exist; M_GEN: all, masked
      constexpr int NQ = (MODE == M_NOUT) ? 4 : NR / 4;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int f0 = 8 * q + 4 * h;
        f32x4 v = {acc[q / 4][4 * (q % 4)], acc[q / 4][4 * (q % 4) + 1], acc[q / 4][4 * (q % 4) + 2],
                   acc[q / 4][4 * (q % 4) + 3]};
        if (MODE != M_NOUT && a.use_ln) {
          if (hp && valid) {
            if (a.tiled) store4_tiled<T, NR>(reinterpret_cast<T*>(a.hpre), q, row, h, v);  // outd == H
            else store4_masked(hp, f0, outd, false, v);
          }
          f32x4 g4 = {1.f, 1.f, 1.f, 1.f}, b4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (f0 + e < outd) { g4[e] = a.ln_g[f0 + e]; b4[e] = a.ln_b[f0 + e]; }
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = ln_out(v[e], mean, rstd, g4[e], b4[e]);
        }
        if (rp) {
          const f32x4 r = load4_masked(rp, f0, outd, false);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = round_t<T>(v[e]) + r[e];
        }
        if (valid) store4_masked(op, f0, outd, false, v);
      }
    }
  }
}

// ------------------------------------------------------------------------- backward
// row rr of the second incoming gradient (gathered through gidx when given)
template <typename T>
AGN_DEV const T* g2_row(const agn_mlp_bwd_args& a, int rr) {
  return reinterpret_cast<const T*>(a.g2) + (size_t)(a.gidx ? a.gidx[rr] : rr) * a.out_dim;
}

template <typename T, int NR, int MODE>
AGN_DEV void load_grad(float (&g)[NR], const agn_mlp_bwd_args& a, int rr, bool valid, int h) {
  const T* g1 = a.g ? reinterpret_cast<const T*>(a.g) + (size_t)rr * a.out_dim : nullptr;
  const T* g2 = a.g2 ? g2_row<T>(a, rr) : nullptr;
  if constexpr (MODE == M_NOUT) {  // out_dim <= 32: acc tile 0 only
#pragma unroll
    for (int i = 0; i < NR; ++i) g[i] = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      f32x4 x = g1 ? load4_masked(g1, 8 * q + 4 * h, a.out_dim, false) : f32x4{0.f, 0.f, 0.f, 0.f};
      if (g2) {
        const f32x4 y = load4_masked(g2, 8 * q + 4 * h, a.out_dim, false);
        x[0] += y[0]; x[1] += y[1]; x[2] += y[2]; x[3] += y[3];
      }
      g[4 * q] = x[0]; g[4 * q + 1] = x[1]; g[4 * q + 2] = x[2]; g[4 * q + 3] = x[3];
    }
  } else {
    if (g1) {
      load_row<T, NR, MODE == M_VEC>(g, g1, a.out_dim, h);
    } else {
#pragma unroll
      for (int i = 0; i < NR; ++i) g[i] = 0.f;
    }
    if (g2) add_row<T, NR, MODE == M_VEC>(g, g2, a.out_dim, h);
  }
  if (!valid) {
#pragma unroll
    for (int i = 0; i < NR; ++i) g[i] = 0.f;
  }
}

// GACT: a hidden activation other than ReLU (agn_mlp_*_args.act_fn): 1 = gelu / silu / tanh, 2 = any
// later code (gact_of); the ReLU instantiations carry none of its registers, and the GACT = 1 ones
// none of the later functions' code
template <typename T, int NT, int MODE, int GACT, bool WIDE = false>
__global__ __launch_bounds__(BLOCK, 2) void mlp_bwd_kernel(const agn_mlp_bwd_args a) {
  static_assert(!WIDE || MODE == M_GEN, "wide segments run on the masked-I/O mode");
  constexpr bool VEC = (MODE == M_VEC);
  constexpr int H = 32 * NT;
  constexpr int NR = 16 * NT;
  constexpr int NP = (NR >= 32) ? NR / 32 : 1;
  __shared__ uint4 wl[lds_units<T, NT>()];
  __shared__ float lnp[WPB][2][H];
  const int lane = threadIdx.x & 63;
  const int c = lane & 31, h = lane >> 5;
  const int wid = threadIdx.x >> 6;
  const int wave = blockIdx.x * WPB + wid;
  const int row = wave * 32 + c;
  const bool valid = row < a.rows;
  const int rr = valid ? row : a.rows - 1;
  const int M = a.out_dim;

  float A[NR];  // current dL/d(pre-activation)
  load_grad<T, NR, MODE>(A, a, rr, valid, h);
  if (MODE != M_NOUT && a.use_ln) {
    // LayerNorm backward, streamed 4 features at a time (hpre, gamma re-read per chunk: the loads
    // are written out in both passes, behind a helper or a lambda they change the assembly)
    const float mean = a.stats[2 * (size_t)rr], rstd = a.stats[2 * (size_t)rr + 1];
    const T* hp = reinterpret_cast<const T*>(a.hpre) + (size_t)rr * M;
    float B[NR];
    float c1 = 0.f, c2 = 0.f;
#pragma unroll
    for (int q = 0; q < NR / 4; ++q) {
      const int f0 = 8 * q + 4 * h;
      const f32x4 hv = a.tiled ? load4_tiled<T, NR>(reinterpret_cast<const T*>(a.hpre), q, rr, h)  // M == H
                       : VEC ? load4(hp + f0) : load4_masked(hp, f0, M, false);
      f32x4 gm = {0.f, 0.f, 0.f, 0.f};
      if (VEC) gm = *reinterpret_cast<const f32x4*>(a.ln_g + f0);
      else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (f0 + e < M) gm[e] = a.ln_g[f0 + e];
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool in = VEC || f0 + e < M;
        const float xh = in ? (hv[e] - mean) * rstd : 0.f;
        ln_bwd_acc(c1, c2, A[4 * q + e], gm[e], xh);
        B[4 * q + e] = A[4 * q + e] * xh;  // g * xhat (LN weight-grad partial)
      }
    }
    c1 = sum32(c1);
    c2 = sum32(c2);
    c1 /= (float)M;
    c2 /= (float)M;
    if (a.ln_partial) {  // LayerNorm parameter partials over the wave's 32 rows (butterfly)
      butterfly_reduce<NR>(B, lane);
      float pg[NP];
#pragma unroll
      for (int i = 0; i < NP; ++i) pg[i] = B[i];
#pragma unroll
      for (int i = 0; i < NR; ++i) B[i] = A[i];
      butterfly_reduce<NR>(B, lane);
      // (these stores and the final sum are the resident backward's too, mlp_general_bf16.hip: one
      // helper for both changes the assembly of either, so each keeps its statements)
      const bool canon = (NR >= 32) || ((c % (32 / (NR < 32 ? NR : 32))) == 0);
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        const int f = feat_of((c * NR) / 32 + i, h);
        if (canon) { lnp[wid][0][f] = pg[i]; lnp[wid][1][f] = B[i]; }
      }
    }
#pragma unroll
    for (int q = 0; q < NR / 4; ++q) {
      const int f0 = 8 * q + 4 * h;
      const f32x4 hv = a.tiled ? load4_tiled<T, NR>(reinterpret_cast<const T*>(a.hpre), q, rr, h)  // M == H
                       : VEC ? load4(hp + f0) : load4_masked(hp, f0, M, false);
      f32x4 gm = {0.f, 0.f, 0.f, 0.f};
      if (VEC) gm = *reinterpret_cast<const f32x4*>(a.ln_g + f0);
      else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (f0 + e < M) gm[e] = a.ln_g[f0 + e];
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool in = VEC || f0 + e < M;
        const float xh = (hv[e] - mean) * rstd;
        A[4 * q + e] = in ? ln_bwd_out(A[4 * q + e], gm[e], c1, c2, xh, rstd) : 0.f;
      }
    }
  }
  // chain rule through the Linear / ReLU stack
  f32x16 acc[NT];
  BOp<T, NR> b;
  for (int l = a.nlin - 1; l >= 0; --l) {
    const int Ml = (l == a.nlin - 1) ? M : H;
    const int kuM = units_k<T>(Ml);
    if (a.gpre[l] && ((a.gpre_tiled >> l) & 1)) {
      store_row_tiled<T, NR>(reinterpret_cast<T*>(a.gpre[l]), A, row, h, valid);
    } else if (a.gpre[l]) {
      T* gp = reinterpret_cast<T*>(a.gpre[l]) + (size_t)row * Ml;
      if (VEC || (MODE == M_NOUT && l < a.nlin - 1)) store_row<T, NR, true>(gp, Ml, A, h, valid);
      else store_row<T, NR, false>(gp, Ml, A, h, valid);
    }
    b.set(A);
    if (l > 0) {
      __syncthreads();
      stage_block(wl, a.wtpk[l], kuM, 0, NT, 0, kuM);
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = f32x16{};
      __syncthreads();
      gemm<T, NT, NR, true>(acc, b, kuM, wl, kuM, NT, lane);
      cbarrier();
      acc_to_regs<NT, NR>(A, acc);
      if constexpr (!GACT) {
        // AGN_RELU_MASK sign bits (8 B per lane instead of the activation row)
        uint32_t mk[mask_dwords<NR>()];
        load_relu_mask<NR>(mk, a.mask[l - 1], min(wave, (a.rows - 1) / 32), lane);  // clamp: idle waves
#pragma unroll
        for (int i = 0; i < NR; ++i) A[i] = mask_sel(mk, i, A[i]);
      } else {
        // dL/dy rounded to T (the Linear backward's output in the storage type), times f'(x) at
        // the forward's saved pre-activation x
        const T* pb = reinterpret_cast<const T*>(a.pre[l - 1]);
#pragma unroll
        for (int q = 0; q < NR / 4; ++q) {
          const f32x4 x = a.tiled ? load4_tiled<T, NR>(pb, q, rr, h) : load4(pb + (size_t)rr * H + 8 * q + 4 * h);
#pragma unroll
          for (int e = 0; e < 4; ++e) A[4 * q + e] = act_bwd<T, GACT == 2>(a.act_fn, x[e], round_t<T>(A[4 * q + e]));
        }
      }
    } else {
      int koff = 0;
      for (int s = 0; s < a.din_nseg; ++s) {
        const int ks = a.din_k[s];
        if (WIDE && a.din[s] && ks > H) {
          // a segment wider than H (no residual form): dX[:, blk] = dh0 . W0[:, blk] per H-wide
          // column block from the packed W0^T, written straight into the one [rows][ks] buffer
          // (row stride ks: the rows need not be 16-B aligned, so the stores are masked)
          for (int c0 = 0; c0 < ks; c0 += H) {
            const int kb = min(H, ks - c0);
            const int otn = (kb + 31) / 32;
            __syncthreads();
            stage_block(wl, a.wtpk[0], kuM, (koff + c0) / 32, otn, 0, kuM);
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = f32x16{};
            __syncthreads();
            gemm<T, NT, NR>(acc, b, kuM, wl, kuM, otn, lane);
            float v[NR];
            acc_to_regs<NT, NR>(v, acc);
            store_row<T, NR, false>(reinterpret_cast<T*>(a.din[s]) + (size_t)row * ks + c0, kb, v, h, valid);
          }
        } else if (a.din[s]) {
          const int otn = (ks + 31) / 32;
          __syncthreads();
          stage_block(wl, a.wtpk[0], kuM, koff / 32, otn, 0, kuM);
#pragma unroll
          for (int t = 0; t < NT; ++t) acc[t] = f32x16{};
          __syncthreads();
          gemm<T, NT, NR>(acc, b, kuM, wl, kuM, otn, lane);
          float v[NR];
          acc_to_regs<NT, NR>(v, acc);
          if (a.din_resid[s]) {
            cbarrier();
            float g[NR];
            load_grad<T, NR, MODE>(g, a, rr, valid, h);
#pragma unroll
            for (int i = 0; i < NR; ++i) v[i] += g[i];
          }
          T* dp = reinterpret_cast<T*>(a.din[s]) + (size_t)row * ks;
          if (MODE != M_GEN && ks == H) store_row<T, NR, true>(dp, ks, v, h, valid);
          else store_row<T, NR, false>(dp, ks, v, h, valid);
        }
        koff += ks;
      }
    }
  }
  if (a.use_ln && a.ln_partial) {
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * M; i += BLOCK) {
      const int q = i / M, f = i - q * M;
      float s = 0.f;
#pragma unroll
      for (int w = 0; w < WPB; ++w) s += lnp[w][q][f];
      a.ln_partial[(size_t)blockIdx.x * 2 * M + i] = s;
    }
  }
}

// ------------------------------------------------------------------------- launch
// f(std::integral_constant<int, V>) for the V among Vs that equals v; false if none does
template <int... Vs, typename F>
bool with_const(int v, F&& f) {
  return ((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}

// the kernels' GACT of an AGN_ACT_* code
inline int gact_of(int act_fn) { return act_fn == AGN_ACT_RELU ? 0 : (act_fn <= AGN_ACT_TANH ? 1 : 2); }

// The one place each direction's general kernel is launched: width, mode and activation become
// template arguments, and g_last_mode records the instantiation that ran.
template <typename T>
int launch_fwd(const agn_mlp_fwd_args& a, int mode, void* stream) {
  const bool ran = with_const<32, 64, 128>(a.hidden, [&](auto hid) {
    with_const<M_VEC, M_GEN, M_NIN, M_NOUT, M_WIDE>(mode, [&](auto m) {
      with_const<0, 1, 2>(gact_of(a.act_fn), [&](auto gact) {
        constexpr bool WIDE = decltype(m)::value == M_WIDE;
        constexpr int MODE = WIDE ? M_GEN : decltype(m)::value;
        hipLaunchKernelGGL((mlp_fwd_kernel<T, decltype(hid)::value / 32, MODE, decltype(gact)::value, WIDE>),
                           dim3(agn_mlp_bwd_nwaves(a.rows)), dim3(BLOCK), 0, (hipStream_t)stream, a);
        g_last_mode[0] = WIDE ? M_WIDE : MODE;
      });
    });
  });
  return ran ? launch_status() : AGN_E_HIDDEN;
}

template <typename T>
int launch_bwd(const agn_mlp_bwd_args& a, int mode, void* stream) {
  const bool ran = with_const<32, 64, 128>(a.hidden, [&](auto hid) {
    with_const<M_VEC, M_GEN, M_NOUT, M_WIDE>(mode, [&](auto m) {  // (no narrow-input mode: dX is masked)
      with_const<0, 1, 2>(gact_of(a.act_fn), [&](auto gact) {
        constexpr bool WIDE = decltype(m)::value == M_WIDE;
        constexpr int MODE = WIDE ? M_GEN : decltype(m)::value;
        hipLaunchKernelGGL((mlp_bwd_kernel<T, decltype(hid)::value / 32, MODE, decltype(gact)::value, WIDE>),
                           dim3(agn_mlp_bwd_nwaves(a.rows)), dim3(BLOCK), 0, (hipStream_t)stream, a);
        g_last_mode[1] = WIDE ? M_WIDE : MODE;
      });
    });
  });
  return ran ? launch_status() : AGN_E_HIDDEN;
}

}  // namespace
