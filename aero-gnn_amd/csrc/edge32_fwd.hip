// Forward of the sum-trick edge MLP on 32-row tiles with 32x32x16 MFMAs (gfx950, bf16, H = 128):
//   e' = e + LN(W3 relu(W2 relu(W1 relu(e W_e^T + P_s[src] + P_d[dst]) + b1) + b2) + b3)
// (models/mgnLayer.py:72-105 EdgeBlockSum, residual :205), bitwise agn_mlp_forward's resident
// kernel on the same operands (mlp.hip mlp_fwd_res_kernel: the same MFMA sequence per accumulator,
// the same exact MFMA row sum P_s + P_d, the same LayerNorm and residual steps), so the 32-row
// fused backward (edge_bwd.hip), which recomputes that kernel's chain, pairs with it unchanged.
//
// The residual add round(LN(h3)) + e runs on the matrix cores like the row sum (round 6: 160 VALU
// fewer per tile, -1 % per launch).
//
// Why a second kernel: the chain is vector-issue-bound on the SIMD, not HBM- or MFMA-bound
// (DESIGN.md §9 round 5). A v_mfma_f32_32x32x16_bf16 holds the SIMD's vector issue for 8 of its
// 32 cycles; the exact MFMA row sum replaces ~190 VALU unpack/add instructions per tile. Against the
// resident kernel (two waves per SIMD at <= 256 registers, the previous tile's stores deferred in
// registers) this one runs three waves per SIMD at <= 168 registers, keeping the residual
// operand; the weight fragments stream two deep instead of a whole k-step ahead. (16 waves at
// <= 128 registers, re-reading the residual, spilled and ran 0.94 -> 1.64 ms per C3 launch;
// static per-SIMD wave priorities changed nothing: both removed in round 6.)
//
// Training saves (SAVE): the first ReLU output a1 in AGN_TILED (the packed operand as it stands, one
// 1-KB store per unit) and the LayerNorm (mean, rstd). The fused backward (edge_bwd.hip) starts its
// recompute at Lin1 from them: 264 B per edge written here against e, P_s[src], P_d[dst], W_e and the
// statistics recomputed there.
//
// Persistent: one workgroup per CU, the four packed weight images resident in LDS (128 KB), each
// wave streaming 32-row tiles in CSC order over an XCD-grouped walk; a tile's node ids are loaded
// one tile ahead through the wave's LDS slot (a loop-carried load result would make the compiler
// wait vmcnt(0) at the loop head, i.e. for the previous tile's stores too).
//
// Receiver sums (AGG, agn_edge_fwd_args.agg): agg[n] = sum of e' rows rowptr[n] .. rowptr[n+1]-1, formed
// from the finished tile instead of by the node kernel re-reading all of e' from HBM. Each wave walks
// one contiguous run of tiles (tile32.hpp RangeWalk) in place of the strided walk. The rounded tile
// goes through a 2-KB LDS buffer of the wave in four 8-row batches beside its global stores; lane l
// then adds columns 2l, 2l + 1 of the rows in edge order: per receiver and column the fp32 adds of
// segment_sum4_kernel (graph.hip) from +0, one rounding, a 256-B row store when the receiver's run
// of edges ends. Where a receiver opens is wave-uniform (one ballot per tile over the dst ids the
// tile loaded), and the open sum goes from tile to tile. One writer per agg row, nothing passes
// between waves: a wave writes the receivers whose whole edge range lies inside its run (it reads
// the dst of the rows next to the run's ends to tell) and zeros for the empty receivers at a row of
// its run (those past the last edge: the wave with the last tile); a receiver that crosses the end of
// a run is summed from e' by edge_agg_fixup_kernel, which recomputes the runs from (rows, grid).
// Receiver means (MEAN, agn_edge_fwd_args.agg_mean): the same sums divided by (float)max(deg, 1) before
// their one rounding, by the kernel and by the fix-up: bitwise agn_segment_sum(out, mean = 1).
//
// The projection-free chain (PROJ = false, agn_edge_fwd_args.proj == NULL):
//   e' = e + LN(W3 relu(W2 relu(W1 relu(e W0^T + b0) + b1) + b2) + b3)
// (models/trial1.py:61-65 MeshGraphNetLayer_v2), the same kernel with the accumulators started from b0
// instead of the row sum; see the template's comment. DESIGN.md §7c has the register counts of every
// instantiation (<= 168, none spills).
#include <type_traits>
#include "tile32.hpp"
#include "aerognn.h"

using namespace agn;
using namespace agn::t32;

namespace {

constexpr int LAYER = LAYER_UNITS;      // packed units (16 B) per weight image
#ifndef AGN_E32_PF
#define AGN_E32_PF 2
#endif
constexpr int PF = AGN_E32_PF;          // weight fragments in flight
#ifndef AGN_E32_DIAG
#define AGN_E32_DIAG 0  // timing diagnostics only (outputs wrong): 1 no LayerNorm statistics, 3 no row sum
#endif

#ifndef AGN_E32_AGG_DIAG
#define AGN_E32_AGG_DIAG 0  // timing diagnostics of AGG only (agg wrong): 1 the contiguous walk alone (no stage, no
#endif                      // sums), 2 everything but the agg stores
constexpr int NW = 12;  // waves per CU (three per SIMD)

struct Smem {
  uint4 w[4 * LAYER];   // packed A units [layer][ot][ku][lane] (agn_pack trans = 0 layout, as is)
  float pv[5][H];       // b1, b2, b3, LN gamma, LN beta
  int ids[NW][64];      // per wave: next tile's src (lanes 0-31) / dst (32-63)
};
static_assert(sizeof(Smem) <= 160 * 1024, "LDS budget");
struct SmemAgg : Smem {
  uint4 stage[NW][8 * 16];  // per wave: 8 rows of the rounded tile, chunk k of row r at [r][k ^ r]
};
static_assert(sizeof(SmemAgg) <= 160 * 1024, "LDS budget");
template <class Base>
struct SmemB0 : Base {
  float pv0[H];  // the projection-free chain: b0, the bias of the first Linear
};
static_assert(sizeof(SmemB0<SmemAgg>) <= 160 * 1024, "LDS budget");
typedef const __attribute__((address_space(4))) int32_t* cidx_t;  // index reads as scalar loads

// Lin l's product: the resident kernel's per-accumulator sequence, fragments PF deep (tile32.hpp)
AGN_DEV void gemm4(f32x16 (&acc)[NT], const BOp<bf16, NR>& b, const uint4* w, int lane) {
  gemm_stream<PF>(acc, b, w, NU, 0, 0, lane);
}

// Diagnostic phase clocks (built with -DAGN_E32_STAMPS into a separate library only,
// tools/e32_stamps.py): the waves of block 0 record s_memtime at 8 points of their first 16 tiles
// into agn_e32_stamps[(wave * 16 + tile) * 16 + point], s_memrealtime (100 MHz) at point 15.
#ifdef AGN_E32_STAMPS
__device__ unsigned long long* agn_e32_stamps;
#define E32_STAMP(k)                                                                                   \
  do {                                                                                                 \
    if (agn_e32_stamps && blockIdx.x == 0 && lane0 == 0 && ntile < 16)                                 \
      agn_e32_stamps[((threadIdx.x >> 6) * 16 + ntile) * 16 + (k)] =                                    \
          (k) == 15 ? __builtin_amdgcn_s_memrealtime() : __builtin_amdgcn_s_memtime();                   \
  } while (0)
#else
#define E32_STAMP(k) \
  do {               \
  } while (0)
#endif

// PROJ = false: the projection-free chain e' = e + LN(W3 relu(W2 relu(W1 relu(e W0^T + b0) + b1) + b2) + b3)
// (models/trial1.py MeshGraphNetLayer_v2's edge update): the accumulators start from b0 as the
// resident kernel's do without projections (mlp.hip: the bias first, then the products), there are no
// src ids and no P rows, and the dst ids are loaded only for the receiver aggregates.
// MEAN (with AGG): a receiver's fp32 column sums are divided by (float)max(deg, 1), deg from rowptr,
// before the one rounding (scatter_mean; segment_sum4_kernel's mean step).
template <bool SAVE, bool AGG, bool PROJ = true, bool MEAN = false>
__global__ __launch_bounds__(64 * NW) void edge32_fwd_kernel(const agn_edge_fwd_args a) {
  static_assert(AGG || !MEAN, "means are receiver aggregates");
  constexpr bool IDS = PROJ || AGG;  // the tile's node ids go through the wave's LDS slot
  constexpr int NTHR = 64 * NW;
  using SmemT = std::conditional_t<AGG, SmemAgg, Smem>;
  __shared__ std::conditional_t<PROJ, SmemT, SmemB0<SmemT>> sm;
  {
    const uint4* const* wp = reinterpret_cast<const uint4* const*>(a.wpk);
    for (int i = threadIdx.x; i < 4 * LAYER; i += NTHR) sm.w[i] = wp[i / LAYER][i % LAYER];
    for (int i = threadIdx.x; i < 5 * H; i += NTHR) {
      const int l = i / H, f = i - l * H;
      sm.pv[l][f] = l < 3 ? (a.bias[l + 1] ? a.bias[l + 1][f] : 0.f) : (l == 3 ? a.ln_g[f] : a.ln_b[f]);
    }
    if constexpr (!PROJ) {
      for (int i = threadIdx.x; i < H; i += NTHR) sm.pv0[i] = a.bias[0] ? a.bias[0][i] : 0.f;
    }
  }
  __syncthreads();
  const int lane0 = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int ntiles = (a.rows + 31) / 32;
  const std::conditional_t<AGG, RangeWalk, Walk> walk(ntiles, w, NW);
  int* wids = sm.ids[w];
  // (!PROJ: both lane halves load dst, so the slot's upper half holds it as with projections)
  const int32_t* const idp = PROJ && lane0 < 32 ? a.src : a.dst;
  auto tile_id = [&](int t) { return idp[min(t * 32 + (lane0 & 31), a.rows - 1)]; };
  if constexpr (IDS) {
    if (walk.first < walk.end) wids[lane0] = tile_id(walk.first);
  }
  const bf16* P = reinterpret_cast<const bf16*>(a.proj);
  const bf16* E = reinterpret_cast<const bf16*>(a.e);
#ifdef AGN_E32_STAMPS
  int ntile = 0;
#endif
  // AGG: the open receiver (wave-uniform; the one before the run's first row is not this wave's to
  // write: closed by the previous run, or crossing into this one). Its two column sums and the
  // tile's dst ids wait in the wave's stage buffer while the chain runs (the buffer is idle then,
  // and the chain has no three registers to spare): dwords 0-31 dst, 64-127 / 128-191 the sums.
  int cur = -1;
  bool skip = true;
  char* const aggp = reinterpret_cast<char*>(a.agg);
  auto agg_put = [&](int n, uint32_t v, int l) {
    if (AGN_E32_AGG_DIAG == 0 && (unsigned)n < (unsigned)a.nodes)
      *reinterpret_cast<uint32_t*>(aggp + (size_t)n * (2 * H) + (uint32_t)(4 * l)) = v;
  };
  // MEAN: receiver n's two column sums over its degree, rounded once (the sums' instantiations keep
  // their statements as they were: routed through this helper their instruction stream moved)
  auto mean2 = [&](int n, float s0, float s1) {
    float cnt = 1.f;
    if ((unsigned)n < (unsigned)a.nodes) {
      const cidx_t ptr = (cidx_t)(uintptr_t)a.rowptr;
      cnt = (float)max(ptr[n + 1] - ptr[n], 1);
    }
    return pack2(s0 / cnt, s1 / cnt);
  };
  uint32_t* park = nullptr;
  if constexpr (AGG && AGN_E32_AGG_DIAG != 1) {
    park = reinterpret_cast<uint32_t*>(sm.stage[w]);
    if (walk.first < walk.end && walk.first > 0) cur = ((cidx_t)(uintptr_t)a.dst)[walk.first * 32 - 1];
    park[64 + lane0] = 0u;
    park[128 + lane0] = 0u;
  }
  for (int tile = walk.first; tile < walk.end; tile += walk.step) {
    cbarrier();
    E32_STAMP(0);
    E32_STAMP(15);
    // lane-derived offsets recomputed per tile, not hoisted and kept live (common.hpp opaque_v)
    const int lane = opaque_v(lane0);
    const int c = lane & 31, h = lane >> 5;
    const int row = tile * 32 + c;
    const bool valid = row < a.rows;
    const int rr = valid ? row : a.rows - 1;
    const bool more = tile + walk.step < walk.end;
    int nid = 0;
    if constexpr (IDS) nid = tile_id(more ? tile + walk.step : tile);
    f32x16 acc[NT];
    BOp<bf16, NR> b;
    if constexpr (!PROJ) {
      if constexpr (AGG) {
        const int cd = wids[32 + c];
        if constexpr (AGN_E32_AGG_DIAG != 1) park[c] = cd;
        if (more) wids[lane] = nid;  // (this tile's reads of the slot are done: LDS is in order per wave)
      }
      b.load_w(E + (size_t)rr * H, h);
      acc_bias(acc, sm.pv0, h);  // acc = b0: the resident kernel's start without projections
    } else {
      const int cs = wids[c], cd = wids[32 + c];
      if constexpr (AGG && AGN_E32_AGG_DIAG != 1) park[c] = cd;
      if (more) wids[lane] = nid;  // (this tile's reads of the slot are done: LDS is in order per wave)
      // acc = P_s[src] + P_d[dst] on the matrix cores (exact fp32 add, common.hpp acc_add2_mfma)
      uint4 rs[NR / 8], rd[NR / 8];
      const bf16* ps = P + (size_t)cs * (2 * H) + 8 * h;
      const bf16* pd = P + (size_t)cd * (2 * H) + H + 8 * h;
#pragma unroll
      for (int i = 0; i < NR / 8; ++i) {
        rs[i] = *reinterpret_cast<const uint4*>(ps + 16 * i);
        rd[i] = *reinterpret_cast<const uint4*>(pd + 16 * i);
      }
      b.load_w(E + (size_t)rr * H, h);
      // all 24 row loads in flight before the first use: without this fence the scheduler of the
      // SAVE instantiation (a1 / statistics stores, 152 registers) issued the P_d rows two at a time
      // behind vmcnt(0) waits (1.01 -> 1.46 ms per C3 launch)
      __builtin_amdgcn_sched_barrier(0);
      bf16x8 f0, f1;
      ident_frags_rows(f0, f1, lane);
      if (AGN_E32_DIAG == 3) {
#pragma unroll
        for (int ot = 0; ot < NT; ++ot) acc[ot] = f32x16{};
      } else {
        acc_add2_mfma_rows<NT, NR / 8>(acc, rs, rd, f0, f1);  // rows as loaded: no lane-half exchange
      }
    }
    E32_STAMP(1);
    const BOp<bf16, NR> e0 = b;  // the residual operand
    gemm4(acc, b, sm.w, lane);
    E32_STAMP(2);
#pragma unroll
    for (int l = 1; l < 4; ++l) {
      cbarrier();
      b.template set_relu<NT>(acc);
      if constexpr (SAVE) {  // a1 (AGN_TILED); behind Lin1's MFMAs or non-temporal: no faster (round 6)
        if (l == 1) b.store_tiled(reinterpret_cast<bf16*>(a.act[0]), row, h, valid);
      }
      acc_bias(acc, sm.pv[l - 1], h);  // the bias of Linear l
      gemm4(acc, b, sm.w + l * LAYER, lane);
      E32_STAMP(2 + l);
    }
    cbarrier();
    // LayerNorm statistics over the row's 128 features (two lanes per row), resident kernel order
    // (written out: as a shared helper the 63 adds below come out with their operands swapped)
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < (AGN_E32_DIAG == 1 ? 1 : NR); ++i) s += acc[i / 16][i % 16];
    s = sum32(s);
    const float mean = s / (float)H;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < (AGN_E32_DIAG == 1 ? 2 : NR); i += 2) q = ln_sq_acc2(q, acc[i / 16][i % 16], acc[(i + 1) / 16][(i + 1) % 16], mean);
    q = sum32(q);
    const float rstd = 1.0f / sqrtf(q / (float)H + 1e-5f);
    if constexpr (SAVE) {
      if (h == 0 && valid) *reinterpret_cast<f32x2*>(a.stats + 2 * (size_t)row) = f32x2{mean, rstd};
    }
    E32_STAMP(6);
    bf16* op = reinterpret_cast<bf16*>(a.out) + (size_t)row * H;
    {
      // LN(h3) rounded to bf16 (the operand's packing), then round(LN) + e on the matrix cores: the
      // identity-fragment sum of two bf16 rows is the VALU path's fp32 add bit for bit (a -0 sum
      // comes out +0), and it replaces 160 unpack / add VALU per tile
      float v[NR];
#pragma unroll
      for (int i = 0; i < NR / 8; ++i) {
        float v8[8];
        acc_get8(v8, acc, i);
        ln_out8(v8, sm.pv[3], sm.pv[4], i, h, mean, rstd);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[8 * i + e] = v8[e];
      }
      BOp<bf16, NR> lnb;
      lnb.set(v);
      bf16x8 f0, f1;
      ident_frags(f0, f1, lane);
      acc_add2_mfma<NT, NR>(acc, lnb, e0, f0, f1);
    }
    if constexpr (!AGG || AGN_E32_AGG_DIAG == 1) {
#pragma unroll
      for (int i = 0; i < NR / 8; ++i) {
        float v[8];
        acc_get8(v, acc, i);
        store8_w(op, i, h, v, valid);
      }
    } else {
      u32x4 pk[NR / 8];  // chunk 2i + h of row c, as stored
#pragma unroll
      for (int i = 0; i < NR / 8; ++i) {
        float v[8];
        acc_get8(v, acc, i);
        pk[i] = __builtin_bit_cast(u32x4, pack8_w(v, h));
        if (valid) *reinterpret_cast<u32x4*>(op + 16 * i + 8 * h) = pk[i];
      }
      char* const stg = reinterpret_cast<char*>(sm.stage[w]);
      const int rcv = (int)park[c];  // the receiver of row c
      // bit c of brk: row c opens another receiver than the row before it (row 0: than the open one);
      // bit c of live: row c is a row of the matrix (a partial last tile)
      const int before = c > 0 ? (int)park[c - 1] : cur;
      const int nrow = min(32, a.rows - tile * 32);
      const uint32_t live = nrow >= 32 ? ~0u : (1u << nrow) - 1u;
      const uint32_t brk = (uint32_t)__ballot(rcv != before) & live;
      f32x2 s = {__uint_as_float(park[64 + lane]), __uint_as_float(park[128 + lane])};
      const uint32_t wr = (uint32_t)(c & 7) * 256u, wx = (uint32_t)(c & 7) << 4;
      const uint32_t rd = (uint32_t)lane << 2;  // dword `lane` of a row: chunk lane / 4
#pragma unroll 1
      for (int p = 0; p < 4; ++p) {
        // (LDS is in order per wave: the batch's reads see its writes, the next batch's writes
        // come after these reads)
        if ((c >> 3) == p) {
#pragma unroll
          for (int i = 0; i < NR / 8; ++i)
            *reinterpret_cast<u32x4*>(stg + wr + (((uint32_t)(2 * i + h) << 4) ^ wx)) = pk[i];
        }
        uint32_t x[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) x[r] = *reinterpret_cast<const uint32_t*>(stg + r * 256 + (rd ^ (uint32_t)(r << 4)));
        const uint32_t bb = (brk >> (8 * p)) & 0xffu, lb = (live >> (8 * p)) & 0xffu;
        if (bb == 0u && lb == 0xffu) {  // eight rows of the open receiver
#pragma unroll
          for (int r = 0; r < 8; ++r) s += f32x2{lo_bf16(x[r]), hi_bf16(x[r])};
        } else {
#pragma unroll
          for (int r = 0; r < 8; ++r) {
            if ((lb >> r) & 1u) {
              if ((bb >> r) & 1u) {
                const int d = __builtin_amdgcn_readlane(rcv, 8 * p + r);
                if constexpr (MEAN) {
                  if (!skip) agg_put(cur, mean2(cur, s[0], s[1]), lane);
                } else {
                  if (!skip) agg_put(cur, pack2(s[0], s[1]), lane);
                }
                for (int n = cur + 1; n < d; ++n) agg_put(n, 0u, lane);  // the empty receivers at this row
                cur = d;
                skip = false;
                s = f32x2{0.f, 0.f};
              }
              s += f32x2{lo_bf16(x[r]), hi_bf16(x[r])};
            }
          }
        }
      }
      park[64 + lane] = __float_as_uint(s[0]);
      park[128 + lane] = __float_as_uint(s[1]);
    }

    E32_STAMP(7);
#ifdef AGN_E32_STAMPS
    ++ntile;
#endif
  }
  if constexpr (AGG && AGN_E32_AGG_DIAG != 1) {
    if (walk.first < walk.end) {
      cbarrier();
      uint32_t sum;
      if constexpr (MEAN) sum = skip ? 0u : mean2(cur, __uint_as_float(park[64 + lane0]), __uint_as_float(park[128 + lane0]));
      else sum = pack2(__uint_as_float(park[64 + lane0]), __uint_as_float(park[128 + lane0]));
      const int rend = min(walk.end * 32, a.rows);
      if (rend == a.rows) {  // the last edge: its receiver ends here, the rest are empty
        if (!skip) agg_put(cur, sum, lane0);
        for (int n = cur + 1; n < a.nodes; ++n) agg_put(n, 0u, lane0);
      } else if (!skip && ((cidx_t)(uintptr_t)a.dst)[rend] != cur) {
        agg_put(cur, sum, lane0);  // ends with the run (the empty ones after it: the next run's)
      }
    }
  }
}

// The receivers edge32_fwd_kernel<., true> left out: one wave per wave of that grid. A run that
// starts inside a receiver's edge range (the rows on both sides of its first row have one dst) makes
// that receiver a crossing one; the first such run of a receiver sums it from e' over its whole
// rowptr range, lane l columns 2l, 2l + 1 in edge order (segment_sum4_kernel's adds), 4 rows in flight.
__global__ __launch_bounds__(256) void edge_agg_fixup_kernel(const agn_edge_fwd_args a) {
  const int lane = threadIdx.x & 63;
  const int gw = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (gw >= a.nblk * NW) return;
  const int ntiles = (a.rows + 31) / 32;
  const RangeWalk run(ntiles, a.nblk, gw / NW, gw % NW, NW);
  if (run.first >= run.end || run.first == 0) return;
  const cidx_t dst = (cidx_t)(uintptr_t)a.dst, ptr = (cidx_t)(uintptr_t)a.rowptr;
  const int p = run.first * 32;
  const int n = dst[p];
  if (dst[p - 1] != n || (unsigned)n >= (unsigned)a.nodes) return;
  const int beg = min(max(ptr[n], 0), a.rows), end = min(max(ptr[n + 1], beg), a.rows);
  // an earlier run that also starts inside n has it
  if (RangeWalk::first_of(ntiles, a.nblk, NW, run.first - 1) * 32 > beg) return;
  const char* ep = reinterpret_cast<const char*>(a.out) + (uint32_t)(4 * lane);
  float s0 = 0.f, s1 = 0.f;
  for (int j = beg; j < end; j += 4) {
    uint32_t v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = *reinterpret_cast<const uint32_t*>(ep + (size_t)min(j + q, end - 1) * (2 * H));
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (j + q < end) {
        s0 += lo_bf16(v[q]);
        s1 += hi_bf16(v[q]);
      }
  }
  if (a.agg_mean) {  // (a crossing receiver has edges: end > beg)
    const float cnt = (float)max(end - beg, 1);
    s0 = s0 / cnt;
    s1 = s1 / cnt;
  }
  *reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(a.agg) + (size_t)n * (2 * H) + (uint32_t)(4 * lane)) = pack2(s0, s1);
}

long g_agg_launches = 0;  // launches that formed the receiver sums (agn_debug_edge_agg_launches: tests check the dispatch)

}  // namespace

extern "C" {

long agn_debug_edge_agg_launches(void) { return g_agg_launches; }

#ifdef AGN_E32_STAMPS
int agn_debug_e32_stamps(void* p) {
  return hipMemcpyToSymbol(HIP_SYMBOL(agn_e32_stamps), &p, sizeof(p)) == hipSuccess ? 0 : -1;
}
#endif

int agn_edge_fwd32_blocks(int rows) {
  return tile_blocks((rows + 31) / 32, NW);
}

int agn_edge_forward32(const agn_edge_fwd_args* a, void* stream) {
  if (!a || a->rows < 0 || a->nblk < 1) return AGN_E_ARG;
  if (a->rows == 0) {  // no edge: every receiver is empty
    if (a->agg && a->nodes > 0 && hipMemsetAsync(a->agg, 0, (size_t)a->nodes * (2 * H), (hipStream_t)stream) != hipSuccess)
      return launch_status();
    return 0;
  }
  // proj == NULL: the projection-free chain (no src; dst only for the receiver aggregates)
  const bool proj = a->proj != nullptr;
  if (!a->e || !a->out || !a->ln_g || !a->ln_b) return AGN_E_ARG;
  if (proj ? (!a->src || !a->dst) : (a->agg && !a->dst)) return AGN_E_ARG;
  if (a->agg_mean != 0 && (a->agg_mean != 1 || !a->agg)) return AGN_E_ARG;
  if (a->act[1] || a->act[2] || a->hpre) return AGN_E_ARG;  // a1 and the statistics are the only saves
  const bool save = a->act[0] != nullptr;
  if (save != (a->stats != nullptr) || (save && (!al16(a->act[0]) || (reinterpret_cast<uintptr_t>(a->stats) & 7))))
    return AGN_E_ARG;
  for (int l = 0; l < 4; ++l)
    if (!a->wpk[l] || !al16(a->wpk[l])) return AGN_E_ARG;
  if (!al16(a->e) || !al16(a->proj) || !al16(a->out)) return AGN_E_ARG;
  if (!proj && a->bias[0] && (reinterpret_cast<uintptr_t>(a->bias[0]) & 3)) return AGN_E_ARG;
  if (a->agg && (!a->rowptr || a->nodes < 1 || !al16(a->agg))) return AGN_E_ARG;
  const dim3 g(a->nblk), blk(64 * NW);
  hipStream_t st = (hipStream_t)stream;
  if (a->agg) ++g_agg_launches;
  // (SAVE, AGG, PROJ, MEAN) -> the instantiation; the sum-trick ones with sums are the four of before
#define E32_LAUNCH(S, A, P, M) hipLaunchKernelGGL((edge32_fwd_kernel<S, A, P, M>), g, blk, 0, st, *a)
#define E32_BY_SAVE(A, P, M)     \
  do {                           \
    if (save) E32_LAUNCH(true, A, P, M); \
    else E32_LAUNCH(false, A, P, M);     \
  } while (0)
  if (proj) {
    if (!a->agg) E32_BY_SAVE(false, true, false);
    else if (!a->agg_mean) E32_BY_SAVE(true, true, false);
    else E32_BY_SAVE(true, true, true);
  } else {
    if (!a->agg) E32_BY_SAVE(false, false, false);
    else if (!a->agg_mean) E32_BY_SAVE(true, false, false);
    else E32_BY_SAVE(true, false, true);
  }
#undef E32_BY_SAVE
#undef E32_LAUNCH
  return launch_status();
}

int agn_edge_agg_fixup(const agn_edge_fwd_args* a, void* stream) {
  if (!a || a->rows < 0 || a->nblk < 1 || a->nblk > (1 << 20)) return AGN_E_ARG;
  if (!a->agg || !a->rowptr || a->nodes < 1 || !al16(a->agg)) return AGN_E_ARG;
  if (a->agg_mean != 0 && a->agg_mean != 1) return AGN_E_ARG;
  if (a->rows == 0) return 0;
  if (!a->dst || !a->out || !al16(a->out)) return AGN_E_ARG;
  hipLaunchKernelGGL(edge_agg_fixup_kernel, dim3((a->nblk * NW + 3) / 4), dim3(256), 0, (hipStream_t)stream, *a);
  return launch_status();
}

}  // extern "C"
