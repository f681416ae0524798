// The bfloat16 translation unit of the fused MLP chains: the general kernels for bfloat16 storage
// (mlp_general.hpp, 54 instantiations) and the two resident-weight kernels, which are bf16-only.
// They share this file because the compiler allocates the registers of the H = 128 general kernels
// differently once the resident kernels leave their translation unit.
#include "mlp_general.hpp"

using namespace agn::t32;

namespace {

// ------------------------------------------------------------------------- resident-weight kernels
// Persistent variants for the hot edge MLP (bf16, H = 128, every layer H -> H, <= 4 Linears): all
// packed weights of the chain live in LDS for the whole launch (4 x 32 KB), so the 8 waves of
// a block never synchronise after the prologue and each wave streams its own 32-row tiles —
// one wave's gathers overlap the other waves' MFMA chains. One block per CU.
constexpr int RES_WPB = 8;
constexpr int RES_BLOCK = 64 * RES_WPB;

// Stage the per-feature fp32 parameter vectors of a resident chain into LDS:
// pv[l] = bias of Linear l (0 if absent), pv[RES_MAXL] = LN gamma, pv[RES_MAXL + 1] = LN beta.
template <int H, int NV>
AGN_DEV void stage_params(float (*pv)[H], const float* const* bias, int nlin, const float* g, const float* b,
                          int nthreads) {
  for (int i = threadIdx.x; i < NV * H; i += nthreads) {
    const int l = i / H, f = i - l * H;
    const float* src = l < NV - 2 ? (l < nlin ? bias[l] : nullptr) : (l == NV - 2 ? g : b);
    pv[l][f] = src ? src[f] : 0.f;
  }
}

// Diagnostic phase clocks of the resident edge forward (built with -DAGN_FWD_STAMPS into the
// separate stamps library only): the 8 waves of block 0 record s_memtime at 10 points of their
// first 8 tiles into agn_fwd_stamps[(wave * 8 + tile) * 16 + point].
#ifdef AGN_FWD_STAMPS
__device__ unsigned long long* agn_fwd_stamps;
#define FWD_STAMP(k)                                                                                   \
  do {                                                                                                 \
    if (agn_fwd_stamps && blockIdx.x == 0 && lane == 0 && ntile < 8)                                   \
      agn_fwd_stamps[((threadIdx.x >> 6) * 8 + ntile) * 16 + (k)] = __builtin_amdgcn_s_memtime();      \
  } while (0)
#else
#define FWD_STAMP(k) \
  do {               \
  } while (0)
#endif

__global__ __launch_bounds__(RES_BLOCK, 2) void mlp_fwd_res_kernel(const agn_mlp_fwd_args a) {
  __shared__ uint4 wres[RES_MAXL * LAYER_UNITS];
  __shared__ __attribute__((aligned(16))) float pv[RES_MAXL + 2][H];  // biases, LN gamma, LN beta
  __shared__ uint4 stg[RES_WPB][8][H / 8 + STG_PAD];  // per-wave 8-row staging: coalesced e loads
  __shared__ int ids[RES_WPB][64];                     // per-wave next-tile src (lanes 0-31) / dst
  for (int l = 0; l < a.nlin; ++l) stage_block(wres + l * LAYER_UNITS, a.wpk[l], NU, 0, NT, 0, NU);
  stage_params<H, RES_MAXL + 2>(pv, a.bias, a.nlin, a.ln_g, a.ln_b, RES_BLOCK);
  __syncthreads();
  const int lane0 = threadIdx.x & 63;
  const int ntiles = (a.rows + 31) / 32;
  const agn_seg& sg = a.seg[0];
  const Walk tw(ntiles, threadIdx.x >> 6, RES_WPB);
  // The sender / receiver ids of the wave's next tile are loaded one tile ahead, so a tile's
  // projection-row gathers issue together with its e loads (one memory latency per tile, not two).
  // They reach the next tile through the wave's LDS slot, not a loop-carried register: a
  // loop-carried load result makes the compiler wait vmcnt(0) at the loop head, i.e. also for the
  // previous tile's e' stores. Lane l loads the src (l < 32) or dst (l >= 32) of row l & 31.
  int* wids = ids[threadIdx.x >> 6];
  const int32_t* const srcp = a.src;
  const int32_t* const dstp = a.dst;
  // (without projections the load reads the input rows instead: always a valid address, so the
  // next-id load below needs no branch - a conditional load leaves a register write at the loop
  // head that the compiler guards with vmcnt(0))
  const int32_t* const idp = a.proj ? (lane0 < 32 ? srcp : dstp) : reinterpret_cast<const int32_t*>(sg.ptr);
  auto tile_id = [&](int t) { return idp[min(t * 32 + (lane0 & 31), a.rows - 1)]; };
  if (a.proj && tw.first < tw.end) wids[lane0] = tile_id(tw.first);
#ifdef AGN_FWD_STAMPS
  int ntile = 0;
#endif
  // the previous tile's e' row, stored once this tile's loads have been consumed (PendingRow)
  PendingRow<NR / 8> pend;
  for (int tile = tw.first; tile < tw.end; tile += tw.step) {
    cbarrier();  // keep the (loop-invariant) LDS weight reads inside the loop: no LICM into VGPRs
    // the lane id behind a barrier each tile: lane-derived offsets (row addresses, staging and
    // weight-fragment offsets) are recomputed per tile instead of being hoisted and kept live
    const int lane = opaque_v(lane0);
    const int c = lane & 31, h = lane >> 5;
    FWD_STAMP(0);
    const int row = tile * 32 + c;
    const bool valid = row < a.rows;
    const int rr = valid ? row : a.rows - 1;
    f32x16 acc[NT];
    BOp<bf16, NR> b;
    // the projection rows are gathered and summed first, then the e tile goes through the staging
    // rows (issuing the e loads ahead of the gathers measured slower: DESIGN.md §9, round 3)
    const bool staged_in = sg.ld == H;
    uint4 eraw[NR / 8];
    const bool more = a.proj && tile + tw.step < tw.end;
    const int nid = tile_id(more ? tile + tw.step : tile);  // (unconditional: see tile_id)
    if (a.proj) {
      const int cs = wids[c], cd = wids[32 + c];
      const bf16* P = reinterpret_cast<const bf16*>(a.proj);
      // acc = P_s[src] + P_d[dst] on the matrix cores (exact fp32 add, common.hpp acc_add2_mfma)
      BOp<bf16, NR> xs, xd;
      {
        // gathers issued, then the previous tile's stores, then the gathered data used: the wait
        // for the gathers does not include the stores (PendingRow)
        uint4 rs[NR / 8], rd[NR / 8];
        const bf16* ps = P + (size_t)cs * (2 * H) + 8 * h;
        const bf16* pd = P + (size_t)cd * (2 * H) + H + 8 * h;
#pragma unroll
        for (int i = 0; i < NR / 8; ++i) {
          rs[i] = *reinterpret_cast<const uint4*>(ps + 16 * i);
          rd[i] = *reinterpret_cast<const uint4*>(pd + 16 * i);
        }
        xs.set_w(rs);
        xd.set_w(rd);
      }
      bf16x8 f0, f1;
      ident_frags(f0, f1, lane);
      acc_add2_mfma<NT, NR>(acc, xs, xd, f0, f1);
    } else {
      t32::acc_bias(acc, pv[0], h);
    }
    FWD_STAMP(1);
    {
      if (staged_in) {  // coalesced 1-KB loads through the wave's LDS staging rows
        tile_load_issue<H / 8>(eraw, reinterpret_cast<const bf16*>(sg.ptr) + (size_t)tile * 32 * H, a.rows - tile * 32,
                               lane);
        uint4 mine[NR / 8];
        tile_load_finish<H / 8>(mine, eraw, stg[threadIdx.x >> 6], lane);
        b.set_w(mine);
      } else {
        b.load_w(reinterpret_cast<const bf16*>(sg.ptr) + (size_t)rr * sg.ld, h);
      }
    }
    // the residual is the layer input itself (e' = e + .., mgnLayer.py:205): keep the packed
    // operand instead of re-reading the row in the epilogue
    const bool res_in = a.resid == sg.ptr && a.out_ld == sg.ld;
    const BOp<bf16, NR> e0 = b;
    FWD_STAMP(2);
    gemm<bf16, NT, NR, true>(acc, b, NU, wres, NU, NT, lane);
    FWD_STAMP(3);
    // the previous tile's e' stores issue here, after this tile's loads have been consumed:
    // the next wait on a load is the next tile's, ~3/4 of a tile later, when they have completed
    cbarrier();
    pend.flush(h);
    for (int l = 1; l < a.nlin; ++l) {
      cbarrier();
      b.template set_relu<NT>(acc);
      if (a.act[l - 1]) {
        if (a.tiled) b.store_tiled(reinterpret_cast<bf16*>(a.act[l - 1]), row, h, valid);
        else b.store(reinterpret_cast<bf16*>(a.act[l - 1]) + (size_t)row * H, h, valid);
      }
      if (a.mask[l - 1]) store_relu_mask<bf16, NR>(a.mask[l - 1], b, tile, lane);
      cbarrier();
      t32::acc_bias(acc, pv[l], h);
      FWD_STAMP(4 + 2 * (l - 1));
      gemm<bf16, NT, NR, true>(acc, b, NU, wres + l * LAYER_UNITS, NU, NT, lane);
      FWD_STAMP(5 + 2 * (l - 1));
    }
    // epilogue: LayerNorm, residual, store (8 features per lane at a time)
    float rstd = 1.f, mean = 0.f;  // (declared in this order, ln_out8 below leaves the assembly as it was)
    if (a.use_ln) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < NR; ++i) s += acc[i / 16][i % 16];
      s = sum32(s);
      mean = s / (float)H;
      float q = 0.f;
#pragma unroll
      for (int i = 0; i < NR; i += 2) q = ln_sq_acc2(q, acc[i / 16][i % 16], acc[(i + 1) / 16][(i + 1) % 16], mean);
      q = sum32(q);
      rstd = 1.0f / sqrtf(q / (float)H + 1e-5f);
      if (a.stats && valid && h == 0) {
        a.stats[2 * (size_t)row] = mean;
        a.stats[2 * (size_t)row + 1] = rstd;
      }
    }
    FWD_STAMP(10);
    bf16* hp = a.hpre ? reinterpret_cast<bf16*>(a.hpre) + (size_t)row * H : nullptr;
    const bf16* rp = a.resid ? reinterpret_cast<const bf16*>(a.resid) + (size_t)rr * a.out_ld : nullptr;
    bf16* op = reinterpret_cast<bf16*>(a.out) + (size_t)row * a.out_ld;
#pragma unroll
    for (int i = 0; i < NR / 8; ++i) {
      float v[8];
      acc_get8(v, acc, i);
      if (a.use_ln) {
        if (hp) {
          if (a.tiled) store8_tiled<bf16, NR>(reinterpret_cast<bf16*>(a.hpre), i, row, h, v, valid);
          else store8_w(hp, i, h, v, valid);
        }
        ln_out8(v, pv[RES_MAXL], pv[RES_MAXL + 1], i, h, mean, rstd);
      }
      if (rp) {
        float r[8];
        if (res_in) e0.get8(r, i);
        else load8_w(r, rp, i, h);
#pragma unroll
        for (int e = 0; e < 8; e += 2) {  // round_t(v) + r, the add packed
          const uint32_t p = pack2t<bf16>(v[e], v[e + 1]);
          const f32x2 o = f2(lo16<bf16>(p), hi16<bf16>(p)) + f2(r[e], r[e + 1]);
          v[e] = o[0];
          v[e + 1] = o[1];
        }
      }
      if (i == 0 && more) wids[lane] = nid;  // (the slot's reads are done: LDS is in order per wave)
      pend.set(i, v);  // direct 16-B stores, deferred (the staged 1-KB store measured slower)
    }
    pend.p = op;
    pend.valid = valid;
    FWD_STAMP(11);
#ifdef AGN_FWD_STAMPS
    ++ntile;
#endif
  }
  pend.flush(lane0 >> 5);
}

AGN_DEV void load_grad_w(float (&g)[NR], const agn_mlp_bwd_args& a, int rr, bool valid, int h) {
  if (a.g) {
    load_row_w<bf16, NR>(g, reinterpret_cast<const bf16*>(a.g) + (size_t)rr * a.out_dim, h);
  } else {  // unused output: zero incoming gradient (no materialised zeros)
#pragma unroll
    for (int i = 0; i < NR; ++i) g[i] = 0.f;
  }
  if (a.g2) add_row_w<bf16, NR>(g, g2_row<bf16>(a, rr), h);
  if (!valid) {
#pragma unroll
    for (int i = 0; i < NR; ++i) g[i] = 0.f;
  }
}

AGN_DEV void add_grad_w(float (&v)[NR], const agn_mlp_bwd_args& a, int rr, int h) {
  // v += (g + g2): the incoming gradient is summed first, as autograd accumulates it
  const bf16* g = reinterpret_cast<const bf16*>(a.g) + (size_t)rr * a.out_dim;
  if (!a.g2 || !a.g) {
    if (a.g) add_row_w<bf16, NR>(v, g, h);
    else if (a.g2) add_row_w<bf16, NR>(v, g2_row<bf16>(a, rr), h);
    return;
  }
  const bf16* g2 = g2_row<bf16>(a, rr);
#pragma unroll
  for (int i = 0; i < NR / 8; ++i) {
    float x[8], y[8];
    load8_w(x, g, i, h);
    load8_w(y, g2, i, h);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[8 * i + e] += x[e] + y[e];
  }
}

__global__ __launch_bounds__(RES_BLOCK, 2) void mlp_bwd_res_kernel(const agn_mlp_bwd_args a) {
  constexpr int NP = NR / 32;
  __shared__ uint4 wres[RES_MAXL * LAYER_UNITS];
  __shared__ float lnp[RES_WPB][2][H];
  __shared__ __attribute__((aligned(16))) float pg_lds[H];  // LN gamma
  // layer 0's weights only serve dX: an encoder (narrow input, no input gradient) skips them
  // (res_bwd_ok: without dX every din pointer is NULL; with dX there is exactly one segment)
  for (int l = a.din[0] ? 0 : 1; l < a.nlin; ++l) stage_block(wres + l * LAYER_UNITS, a.wtpk[l], NU, 0, NT, 0, NU);
  for (int i = threadIdx.x; i < H; i += RES_BLOCK) pg_lds[i] = a.use_ln ? a.ln_g[i] : 0.f;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int c = lane & 31, h = lane >> 5;
  const int wid = threadIdx.x >> 6;
  const int ntiles = (a.rows + 31) / 32;
  float pg[NP], pb[NP];
#pragma unroll
  for (int i = 0; i < NP; ++i) { pg[i] = 0.f; pb[i] = 0.f; }
  const Walk tw(ntiles, wid, RES_WPB);
  for (int tile = tw.first; tile < tw.end; tile += tw.step) {
    cbarrier();
    const int row = tile * 32 + c;
    const bool valid = row < a.rows;
    const int rr = valid ? row : a.rows - 1;
    float A[NR];
    load_grad_w(A, a, rr, valid, h);
    if (a.use_ln) {
      const float mean = a.stats[2 * (size_t)rr], rstd = a.stats[2 * (size_t)rr + 1];
      const bf16* hp = reinterpret_cast<const bf16*>(a.hpre) + (size_t)rr * H;
      float B[NR];
      float c1 = 0.f, c2 = 0.f;
      // the pre-LN row is read once and kept packed (32 VGPRs) for both LN passes
      uint4 hraw[NR / 8];
#pragma unroll
      for (int i = 0; i < NR / 8; ++i) {
        if (a.tiled) {
          hraw[i] = reinterpret_cast<const uint4*>(a.hpre)[tiled_unit<bf16, NR>(rr, i, h)];
        } else {
          float t8[8];
          load8_w(t8, hp, i, h);
          hraw[i] = __builtin_bit_cast(uint4, u32x4{pack2(t8[0], t8[1]), pack2(t8[2], t8[3]), pack2(t8[4], t8[5]),
                                                    pack2(t8[6], t8[7])});
        }
      }
#pragma unroll
      for (int i = 0; i < NR / 8; ++i) {
        float hv[8];
        unpack8(hv, hraw[i]);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const f32x4 gm = *reinterpret_cast<const f32x4*>(pg_lds + 16 * i + 8 * j + 4 * h);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int r = 8 * i + 4 * j + e;
            const float xh = (hv[4 * j + e] - mean) * rstd;
            ln_bwd_acc(c1, c2, A[r], gm[e], xh);
            B[r] = A[r] * xh;
          }
        }
      }
      c1 = sum32(c1);
      c2 = sum32(c2);
      c1 /= (float)H;
      c2 /= (float)H;
      if (a.ln_partial) {
        butterfly_reduce<NR>(B, lane);
#pragma unroll
        for (int i = 0; i < NP; ++i) pg[i] += B[i];
#pragma unroll
        for (int i = 0; i < NR; ++i) B[i] = A[i];
        butterfly_reduce<NR>(B, lane);
#pragma unroll
        for (int i = 0; i < NP; ++i) pb[i] += B[i];
      }
#pragma unroll
      for (int i = 0; i < NR / 8; ++i) {
        float hv[8];
        unpack8(hv, hraw[i]);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const f32x4 gm = *reinterpret_cast<const f32x4*>(pg_lds + 16 * i + 8 * j + 4 * h);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int r = 8 * i + 4 * j + e;
            const float xh = (hv[4 * j + e] - mean) * rstd;
            A[r] = ln_bwd_out(A[r], gm[e], c1, c2, xh, rstd);
          }
        }
      }
    }
    f32x16 acc[NT];
    BOp<bf16, NR> b;
    for (int l = a.nlin - 1; l >= 0; --l) {
      cbarrier();
      // AGN_RELU_MASK sign bits (res_bwd_ok: always given), issued before this layer's gpre store:
      // vmcnt retires in order, so a load issued after the store would wait for it to complete
      uint32_t mk[mask_dwords<NR>()];
      if (l > 0) load_relu_mask<NR>(mk, a.mask[l - 1], tile, lane);
      if (a.gpre[l]) {
        if ((a.gpre_tiled >> l) & 1) store_row_tiled<bf16, NR>(reinterpret_cast<bf16*>(a.gpre[l]), A, row, h, valid);
        else store_row_w<bf16, NR>(reinterpret_cast<bf16*>(a.gpre[l]) + (size_t)row * H, A, h, valid);
      }
      b.set(A);
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = f32x16{};
      if (l > 0) {
        gemm<bf16, NT, NR, true>(acc, b, NU, wres + l * LAYER_UNITS, NU, NT, lane);
#pragma unroll
        for (int i = 0; i < NR; ++i) A[i] = mask_sel(mk, i, acc[i / 16][i % 16]);
      } else if (a.din[0]) {
        // de = W0^T gpre0 (+ g + g2), direct 16-B stores
        gemm<bf16, NT, NR, true>(acc, b, NU, wres, NU, NT, lane);
        float v[NR];
        acc_to_regs<NT, NR>(v, acc);
        if (a.din_resid[0]) add_grad_w(v, a, rr, h);
        store_row_w<bf16, NR>(reinterpret_cast<bf16*>(a.din[0]) + (size_t)row * H, v, h, valid);
      }
    }
  }
  if (a.use_ln && a.ln_partial) {
    // (mlp_bwd_kernel's stores and sum, written out here as there: see its note)
    const bool canon = (NR >= 32) || ((c % (32 / (NR < 32 ? NR : 32))) == 0);
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int f = feat_of((c * NR) / 32 + i, h);
      if (canon) { lnp[wid][0][f] = pg[i]; lnp[wid][1][f] = pb[i]; }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * H; i += RES_BLOCK) {
      const int q = i / H, f = i - q * H;
      float s = 0.f;
#pragma unroll
      for (int w = 0; w < RES_WPB; ++w) s += lnp[w][q][f];
      a.ln_partial[(size_t)blockIdx.x * 2 * H + i] = s;
    }
  }
}

int res_blocks(int rows) {
  const int tiles = (rows + 31) / 32;
  const int need = (tiles + RES_WPB - 1) / RES_WPB;
  const int cap = cu_count();  // 128 KB of resident weights: one block per CU
  return need < cap ? (need > 0 ? need : 1) : cap;
}

}  // namespace

#ifdef AGN_FWD_STAMPS
extern "C" int agn_debug_fwd_stamps(void* p) {
  return hipMemcpyToSymbol(HIP_SYMBOL(agn_fwd_stamps), &p, sizeof(p)) == hipSuccess ? 0 : -1;
}
#endif

namespace agn {
int mlp_general_fwd_bf16(const agn_mlp_fwd_args& a, int mode, void* stream) { return launch_fwd<bf16>(a, mode, stream); }
int mlp_general_bwd_bf16(const agn_mlp_bwd_args& a, int mode, void* stream) { return launch_bwd<bf16>(a, mode, stream); }

int mlp_resident_fwd(const agn_mlp_fwd_args& a, void* stream) {
  hipLaunchKernelGGL(mlp_fwd_res_kernel, dim3(res_blocks(a.rows)), dim3(RES_BLOCK), 0, (hipStream_t)stream, a);
  return launch_status();
}
int mlp_resident_bwd(const agn_mlp_bwd_args& a, void* stream, int* ln_rows) {
  *ln_rows = res_blocks(a.rows);
  hipLaunchKernelGGL(mlp_bwd_res_kernel, dim3(*ln_rows), dim3(RES_BLOCK), 0, (hipStream_t)stream, a);
  return launch_status();
}
}  // namespace agn
