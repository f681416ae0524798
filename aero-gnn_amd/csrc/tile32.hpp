// Shared code of the persistent "32-row tile" kernels (gfx950, bf16, H = 128): edge32_fwd.hip,
// enc32_fwd.hip, node32_fwd.hip, node32_bwd.hip and edge_bwd.hip; the tile walk also serves the
// resident kernels of mlp_general_bf16.hip and proj.hip. Each wave of these kernels streams 32-row tiles in
// the acc layout of common.hpp and must stay bitwise equal to the general kernel (mlp_general.hpp) on the same
// operands, so the sequences that pin that equality (the MFMA order of a streamed product, the
// LayerNorm output steps) are written once here.
//
// These kernels are register-tight, and a sequence moved behind a helper is not always compiled as
// it was in place (the helper is optimised on its own before it is inlined). A helper is used only
// where the kernel's instruction stream stayed identical; where it did not, the call site keeps
// the sequence written out and says so. Check the device assembly before moving one.
#pragma once
#include "common.hpp"
#include "host.hpp"

namespace agn {
namespace t32 {

constexpr int H = 128;
constexpr int NT = 4;                       // 32-feature output tiles per row
constexpr int NR = 64;                      // acc registers per lane (the features of its row half)
constexpr int NU = 8;                       // k-steps of 16 per 128 input features
constexpr int LAYER_UNITS = NT * NU * 64;   // packed units (16 B) of a 128 x 128 weight image

// XCD-aware tile walk: blocks b and b + 8 share an XCD (and its 4 MB L2), so each group of
// blocks {g, g+8, ...} walks one contiguous eighth of the tiles. Consecutive CSC edge tiles
// share receivers and nearby senders: their P_s/P_d rows are re-read from the same L2.
// nw = the waves of a block that walk, w = this wave's index among them (nw = 1, w = 0: the block
// walks as one, edge_bwd.hip's rounds).
struct Walk {
  int first, end, step;
  AGN_DEV Walk(int ntiles, int w, int nw) {
    if (gridDim.x >= 8 && (gridDim.x & 7) == 0) {
      const int g = blockIdx.x & 7, bi = blockIdx.x >> 3, nb = gridDim.x >> 3;
      const int per = (ntiles + 7) / 8;
      first = g * per + bi * nw + w;
      end = min(ntiles, (g + 1) * per);
      step = nb * nw;
    } else {
      first = blockIdx.x * nw + w;
      end = ntiles;
      step = gridDim.x * nw;
    }
  }
};

// The same tiles as contiguous ranges: the waves of an XCD group split their eighth of the tiles
// (all tiles when the grid is no multiple of 8) into one run each, the first `cnt % waves` runs one
// tile longer. A wave that walks its run in order can carry a sum over the rows from tile to tile
// (edge32_fwd.hip's receiver sums). The split is a function of (ntiles, grid, block, w, nw) alone, so
// another launch can recompute every run's ends (agn_edge_agg_fixup).
struct RangeWalk {
  int first, end, step;
  // the tiles [base, base + cnt) that block blk's group splits over n runs, and this wave's run i
  static AGN_DEV void group(int ntiles, int grid, int blk, int w, int nw, int& base, int& cnt, int& i, int& n) {
    if (grid >= 8 && (grid & 7) == 0) {
      const int per = (ntiles + 7) / 8;
      base = (blk & 7) * per;
      cnt = max(0, min(ntiles, base + per) - base);
      i = (blk >> 3) * nw + w;
      n = (grid >> 3) * nw;
    } else {
      base = 0;
      cnt = ntiles;
      i = blk * nw + w;
      n = grid * nw;
    }
  }
  AGN_DEV RangeWalk(int ntiles, int grid, int blk, int w, int nw) {
    int base, cnt, i, n;
    group(ntiles, grid, blk, w, nw, base, cnt, i, n);
    const int q = cnt / n, r = cnt - q * n;
    first = base + i * q + min(i, r);
    end = first + q + (i < r ? 1 : 0);
    step = 1;
  }
  AGN_DEV RangeWalk(int ntiles, int w, int nw) : RangeWalk(ntiles, (int)gridDim.x, (int)blockIdx.x, w, nw) {}
  // the first tile of the run that holds tile t < ntiles
  static AGN_DEV int first_of(int ntiles, int grid, int nw, int t) {
    int base, cnt, i, n;
    const bool xcd = grid >= 8 && (grid & 7) == 0;
    group(ntiles, grid, xcd ? t / ((ntiles + 7) / 8) : 0, 0, nw, base, cnt, i, n);
    const int q = cnt / n, r = cnt - q * n, o = t - base;
    const int k = o < r * (q + 1) ? o / (q + 1) : r + (o - r * (q + 1)) / q;  // (q >= 1 here: o < cnt)
    return base + k * q + min(k, r);
  }
};

// acc[ot] += W[output tile ot0 + ot, k-units u0 .. u0 + 7] . b over the k-steps in order (the
// per-accumulator sequence of common.hpp gemm, so the sums are bitwise the general kernel's). w is
// a packed image of ku_total k-units per output tile, in LDS or in global memory (L2); its
// fragments (u, ot) stream PF deep, ot inner. FENCE: a scheduling fence per step, which keeps the
// scheduler from hoisting all 32 fragment loads.
template <int PF, bool FENCE = false>
AGN_DEV void gemm_stream(f32x16 (&acc)[NT], const BOp<bf16, NR>& b, const uint4* w, int ku_total, int ot0, int u0,
                         int lane) {
  uint4 f[PF];
#pragma unroll
  for (int i = 0; i < PF; ++i) f[i] = w[((ot0 + i % NT) * ku_total + u0 + i / NT) * 64 + lane];
#pragma unroll
  for (int idx = 0; idx < NT * NU; ++idx) {
    const uint4 cur = f[idx % PF];
    const int nx = idx + PF;
    if (nx < NT * NU) f[idx % PF] = w[((ot0 + nx % NT) * ku_total + u0 + nx / NT) * 64 + lane];
    b.mfma(acc[idx % NT], cur, idx / NT);
    if (FENCE) __builtin_amdgcn_sched_barrier(0);
  }
}

// acc = bias (fp32 [H] in LDS), acc layout
// the same for one bias (fp32 [H])
AGN_DEV void acc_bias(f32x16 (&acc)[NT], const float* pv, int h) {
#pragma unroll
  for (int q = 0; q < 4 * NT; ++q) {
    const f32x4 x = *reinterpret_cast<const f32x4*>(pv + 8 * q + 4 * h);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[q / 4][4 * (q % 4) + e] = x[e];
  }
}

// registers 8i .. 8i + 7 of the lane's row half (one 16-B unit of the row once packed)
AGN_DEV void acc_get8(float (&v)[8], const f32x16 (&acc)[NT], int i) {
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = acc[(8 * i + e) / 16][(8 * i + e) % 16];
}

// v = LN(v) for registers 8i .. 8i + 7 (acc_get8), gamma and beta fp32 [H] in LDS
AGN_DEV void ln_out8(float (&v)[8], const float* gam, const float* bet, int i, int h, float mean, float rstd) {
#pragma unroll
  for (int jj = 0; jj < 2; ++jj) {
    const int f0 = 16 * i + 8 * jj + 4 * h;
    const f32x4 g4 = *reinterpret_cast<const f32x4*>(gam + f0);
    const f32x4 b4 = *reinterpret_cast<const f32x4*>(bet + f0);
#pragma unroll
    for (int e = 0; e < 4; e += 2) {
      const f32x2 o = ln_out2(f2(v[4 * jj + e], v[4 * jj + e + 1]), mean, rstd, f2(g4[e], g4[e + 1]),
                              f2(b4[e], b4[e + 1]));
      v[4 * jj + e] = o[0];
      v[4 * jj + e + 1] = o[1];
    }
  }
}

}  // namespace t32
}  // namespace agn
