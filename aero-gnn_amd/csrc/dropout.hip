// Training-mode dropout of the MLP chains (models/mlp.py:40-51 `x = dropout(act(layer(x)))`) as one
// elementwise pass between two Linears: activation + dropout forward and its backward, for bf16 /
// fp16 / fp32 / fp64 storage. The fused chain kernels are not involved: a chain with dropout runs
// Linear by Linear and calls these kernels in between.
//
//   forward   a   = round_T(act(float(y)))             (act < 0: a = y, no activation)
//             out = kept ? round_T(float(a) * scale) : 0,   scale = (float)(1 / (1 - p))
//             mask: one bit per element, bit e & 7 of byte e >> 3, ceil(n / 8) bytes
//   backward  da  = kept ? round_T(float(dout) * scale) : 0
//             dy  = round_T(act_bwd(act, float(y), float(da)))      (act < 0: dy = da)
//   fp64 computes in double throughout.
//
// The mask is Philox4x32-10 (standard constants, ten rounds): key = (lo32(seed), hi32(seed)), element
// e reads word e & 3 of the block with counter (lo32(c), hi32(c), 0, 0), c = offset / 4 + (e >> 2), and
// is kept iff word >= min(2^32 - 1, round(p 2^32)). p >= 1 drops everything. The mask of an element
// depends on (seed, offset, e, p) alone: not on the grid, the access width or the storage type.
//
// One thread owns eight consecutive elements = one mask byte = two Philox blocks, and walks the
// groups with a grid stride. Where every pointer is 16-B aligned a full group moves in 16-B
// accesses (one for 16-bit storage, two for fp32, four for fp64); the last partial group and
// unaligned views take the scalar path. No atomics: two calls with the same arguments give the same
// bytes. out may be y itself (each thread reads its group before it writes it).
#include "common.hpp"
#include "act64.hpp"
#include "host.hpp"
#include "aerognn.h"

using namespace agn;

namespace {

constexpr int DR_THREADS = 256;
constexpr int DR_BLOCKS_PER_CU = 8;

AGN_DEV void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
  // one 32 x 32 -> 64 multiply per product (v_mad_u64_u32) instead of a high and a low one, both at
  // a quarter of the VALU rate: 6 % off the forward at 6,000,000 x 128 bf16
  const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
  const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
  const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
  c[0] = hi1 ^ c[1] ^ k0;
  c[1] = lo1;
  c[2] = hi0 ^ c[3] ^ k1;
  c[3] = lo0;
}

// Philox4x32-10 of the counter (lo32(ctr), hi32(ctr), 0, 0)
AGN_DEV void philox4x32_10(uint64_t ctr, uint32_t k0, uint32_t k1, uint32_t (&c)[4]) {
  c[0] = (uint32_t)ctr;
  c[1] = (uint32_t)(ctr >> 32);
  c[2] = 0u;
  c[3] = 0u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

// the arithmetic of one element in the compute type of T (float; double for fp64)
template <typename T> struct Arith {
  typedef float S;
  static AGN_DEV T act(int k, T y) { return k < 0 ? y : from_f<T>(act_fwd(k, to_f(y))); }
  static AGN_DEV T mul(T a, S s) { return from_f<T>(to_f(a) * s); }
  static AGN_DEV T dact(int k, T y, T da) { return k < 0 ? da : from_f<T>(act_bwd<T>(k, to_f(y), to_f(da))); }
  static AGN_DEV T zero() { return from_f<T>(0.f); }
};
template <> struct Arith<double> {
  typedef double S;
  static AGN_DEV double act(int k, double y) { return k < 0 ? y : act_fwd64(k, y); }
  static AGN_DEV double mul(double a, S s) { return a * s; }
  static AGN_DEV double dact(int k, double y, double da) { return k < 0 ? da : act_bwd64(k, y, da); }
  static AGN_DEV double zero() { return 0.0; }
};

template <typename T> struct alignas(16) Chunk16 { T v[16 / sizeof(T)]; };

// elements [e0, e0 + cnt) of p into v; a full group of an aligned tensor in 16-B accesses
template <typename T>
AGN_DEV void load_group(T (&v)[8], const T* p, int64_t e0, int cnt, bool vec) {
  constexpr int W = 16 / sizeof(T);
  if (vec && cnt == 8) {
#pragma unroll
    for (int c = 0; c < 8 / W; ++c) {
      const Chunk16<T> x = *reinterpret_cast<const Chunk16<T>*>(p + e0 + c * W);
#pragma unroll
      for (int q = 0; q < W; ++q) v[c * W + q] = x.v[q];
    }
    return;
  }
#pragma unroll
  for (int q = 0; q < 8; ++q) v[q] = q < cnt ? p[e0 + q] : Arith<T>::zero();
}

template <typename T>
AGN_DEV void store_group(const T (&v)[8], T* p, int64_t e0, int cnt, bool vec) {
  constexpr int W = 16 / sizeof(T);
  if (vec && cnt == 8) {
#pragma unroll
    for (int c = 0; c < 8 / W; ++c) {
      Chunk16<T> x;
#pragma unroll
      for (int q = 0; q < W; ++q) x.v[q] = v[c * W + q];
      *reinterpret_cast<Chunk16<T>*>(p + e0 + c * W) = x;
    }
    return;
  }
#pragma unroll
  for (int q = 0; q < 8; ++q)
    if (q < cnt) p[e0 + q] = v[q];
}

// y and out may be the same buffer: no __restrict__ on them
template <typename T>
__global__ void __launch_bounds__(DR_THREADS)
act_dropout_fwd_kernel(int64_t n, int act, const T* y, T* out, uint8_t* __restrict__ mask, uint32_t thr,
                       int drop_all, typename Arith<T>::S scale, uint32_t k0, uint32_t k1, uint64_t ctr0, int vec) {
  const int64_t ngroup = (n + 7) >> 3;
  const int64_t stride = (int64_t)gridDim.x * DR_THREADS;
  for (int64_t g = (int64_t)blockIdx.x * DR_THREADS + threadIdx.x; g < ngroup; g += stride) {
    const int64_t e0 = g << 3;
    const int cnt = (int)min((int64_t)8, n - e0);
    T v[8];
    load_group<T>(v, y, e0, cnt, vec != 0);
    uint32_t bits = 0u;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      uint32_t w[4];
      philox4x32_10(ctr0 + 2u * (uint64_t)g + (uint64_t)h, k0, k1, w);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = 4 * h + q;
        const bool kept = !drop_all && w[q] >= thr && i < cnt;
        bits |= (kept ? 1u : 0u) << i;
        const T a = Arith<T>::act(act, v[i]);
        v[i] = kept ? Arith<T>::mul(a, scale) : Arith<T>::zero();
      }
    }
    store_group<T>(v, out, e0, cnt, vec != 0);
    mask[g] = (uint8_t)bits;
  }
}

// y: the forward's input (unused and may be NULL when act < 0); dy may be dout itself
template <typename T>
__global__ void __launch_bounds__(DR_THREADS)
act_dropout_bwd_kernel(int64_t n, int act, const T* __restrict__ y, const T* dout, const uint8_t* __restrict__ mask,
                       T* dy, typename Arith<T>::S scale, int vec) {
  const int64_t ngroup = (n + 7) >> 3;
  const int64_t stride = (int64_t)gridDim.x * DR_THREADS;
  for (int64_t g = (int64_t)blockIdx.x * DR_THREADS + threadIdx.x; g < ngroup; g += stride) {
    const int64_t e0 = g << 3;
    const int cnt = (int)min((int64_t)8, n - e0);
    T d[8], x[8];
    load_group<T>(d, dout, e0, cnt, vec != 0);
    if (act >= 0) load_group<T>(x, y, e0, cnt, vec != 0);
    const uint32_t bits = mask[g];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const T da = ((bits >> i) & 1u) ? Arith<T>::mul(d[i], scale) : Arith<T>::zero();
      d[i] = act >= 0 ? Arith<T>::dact(act, x[i], da) : da;
    }
    store_group<T>(d, dy, e0, cnt, vec != 0);
  }
}

int grid_for(int64_t n) {
  const int64_t need = ((n + 7) / 8 + DR_THREADS - 1) / DR_THREADS;
  const int64_t cap = (int64_t)cu_count() * DR_BLOCKS_PER_CU;
  return (int)(need < cap ? need : cap);
}

bool act_ok(int act) { return act == AGN_ACT_NONE || (act >= AGN_ACT_RELU && act <= AGN_ACT_TANHSHRINK); }

template <typename T>
void launch_fwd(int64_t n, int act, const void* y, void* out, uint8_t* mask, double p, uint64_t seed, uint64_t offset,
                hipStream_t st) {
  const bool all = !(p < 1.0);
  double t = p * 4294967296.0;
  t = t < 0.0 ? 0.0 : rint(t);
  const uint32_t thr = t >= 4294967295.0 ? 0xffffffffu : (uint32_t)t;
  const typename Arith<T>::S scale = all ? (typename Arith<T>::S)0 : (typename Arith<T>::S)(1.0 / (1.0 - p));
  const int vec = al16(y) && al16(out);
  hipLaunchKernelGGL(act_dropout_fwd_kernel<T>, dim3(grid_for(n)), dim3(DR_THREADS), 0, st, n, act, (const T*)y,
                     (T*)out, mask, thr, all ? 1 : 0, scale, (uint32_t)seed, (uint32_t)(seed >> 32), offset / 4, vec);
}

template <typename T>
void launch_bwd(int64_t n, int act, const void* y, const void* dout, const uint8_t* mask, void* dy, double p,
                hipStream_t st) {
  const typename Arith<T>::S scale = !(p < 1.0) ? (typename Arith<T>::S)0 : (typename Arith<T>::S)(1.0 / (1.0 - p));
  const int vec = (act < 0 || al16(y)) && al16(dout) && al16(dy);
  hipLaunchKernelGGL(act_dropout_bwd_kernel<T>, dim3(grid_for(n)), dim3(DR_THREADS), 0, st, n, act, (const T*)y,
                     (const T*)dout, mask, (T*)dy, scale, vec);
}

}  // namespace

extern "C" {

int64_t agn_act_dropout_pass_elems(void) { return (int64_t)cu_count() * DR_BLOCKS_PER_CU * DR_THREADS * 8; }

int agn_act_dropout_fwd(int dtype, int act, int64_t n, const void* y, void* out, uint8_t* mask, double p,
                        uint64_t seed, uint64_t offset, void* stream) {
  if (n < 0 || !(p >= 0.0) || p > 1.0 || !act_ok(act)) return AGN_E_ARG;
  if (n == 0) return 0;
  if (!y || !out || !mask) return AGN_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  switch (dtype) {
    case AGN_F32: launch_fwd<float>(n, act, y, out, mask, p, seed, offset, st); break;
    case AGN_BF16: launch_fwd<bf16>(n, act, y, out, mask, p, seed, offset, st); break;
    case AGN_F16: launch_fwd<f16>(n, act, y, out, mask, p, seed, offset, st); break;
    case AGN_F64: launch_fwd<double>(n, act, y, out, mask, p, seed, offset, st); break;
    default: return AGN_E_DTYPE;
  }
  return launch_status();
}

int agn_act_dropout_bwd(int dtype, int act, int64_t n, const void* y, const void* dout, const uint8_t* mask, void* dy,
                        double p, void* stream) {
  if (n < 0 || !(p >= 0.0) || p > 1.0 || !act_ok(act)) return AGN_E_ARG;
  if (n == 0) return 0;
  if (!dout || !dy || !mask || (act >= 0 && !y)) return AGN_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  switch (dtype) {
    case AGN_F32: launch_bwd<float>(n, act, y, dout, mask, dy, p, st); break;
    case AGN_BF16: launch_bwd<bf16>(n, act, y, dout, mask, dy, p, st); break;
    case AGN_F16: launch_bwd<f16>(n, act, y, dout, mask, dy, p, st); break;
    case AGN_F64: launch_bwd<double>(n, act, y, dout, mask, dy, p, st); break;
    default: return AGN_E_DTYPE;
  }
  return launch_status();
}

}  // extern "C"
