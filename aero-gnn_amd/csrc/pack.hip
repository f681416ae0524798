// Weight packing (agn_pack): row-major Linear weights into the MFMA A-fragment order the fused MLP
// kernels read with one 16-B load per lane (common.hpp), and parameter vectors to fp32. Also the
// column sum of per-block partials (agn_reduce_partials).
#include "common.hpp"
#include "host.hpp"
#include "aerognn.h"

using namespace agn;

namespace {

// A operand of Y^T = A * X^T: A[r][k] = trans ? W[k][r] : W[r][k]  (W row-major, ld)
template <typename S>
AGN_DEV float wat(const S* w, int ld, int M, int K, int trans, int r, int k) {
  if (r >= M || k >= K) return 0.f;
  return trans ? to_f(w[(size_t)k * ld + r]) : to_f(w[(size_t)r * ld + k]);
}

template <typename S>
AGN_DEV void pack_one(const agn_pack_desc& d, int tid) {
  const S* w = reinterpret_cast<const S*>(d.src);
  if (d.rows == 0) {  // vector -> fp32
    if (tid < d.cols) reinterpret_cast<float*>(d.dst)[d.col_off + tid] = to_f(w[(size_t)tid * d.ld]);
    return;
  }
  const int OT = (d.rows + 31) / 32;
  const int lane = tid & 63;
  const int i = lane & 31, hh = lane >> 5;
  const int unit = tid >> 6;
  const int ot0 = d.row_off / 32;
  if (d.dst_dtype == AGN_BF16 || d.dst_dtype == AGN_F16) {
    const int KU = (d.cols + 15) / 16, KUT = (d.dst_cols + 15) / 16, ku0 = d.col_off / 16;
    if (unit >= OT * KU) return;
    const int ot = unit / KU, ku = unit % KU;
    const size_t at = ((size_t)(ot0 + ot) * KUT + ku0 + ku) * 64 + lane;
    if (d.dst_dtype == AGN_BF16) {
      bf16x8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        o[j] = (bf16)wat(w, d.ld, d.rows, d.cols, d.trans, 32 * ot + i, 16 * ku + 8 * (j >> 2) + 4 * hh + (j & 3));
      reinterpret_cast<bf16x8*>(d.dst)[at] = o;
    } else {
      f16x8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        o[j] = (f16)wat(w, d.ld, d.rows, d.cols, d.trans, 32 * ot + i, 16 * ku + 8 * (j >> 2) + 4 * hh + (j & 3));
      reinterpret_cast<f16x8*>(d.dst)[at] = o;
    }
  } else {
    const int KU = 2 * ((d.cols + 15) / 16), KUT = 2 * ((d.dst_cols + 15) / 16), ku0 = d.col_off / 8;
    if (unit >= OT * KU) return;
    const int ot = unit / KU, ku = unit % KU;
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = wat(w, d.ld, d.rows, d.cols, d.trans, 32 * ot + i, 8 * ku + 4 * hh + e);
    reinterpret_cast<f32x4*>(d.dst)[((size_t)(ot0 + ot) * KUT + ku0 + ku) * 64 + lane] = o;
  }
}

__global__ void pack_kernel(const agn_pack_desc* __restrict__ descs) {
  const agn_pack_desc d = descs[blockIdx.y];
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  // only float32 / bfloat16 / float16 operands are packed (the descriptors live in device memory, so
  // the host wrapper (aerognn.core.Pack) rejects others; a stray one writes nothing here instead of
  // reinterpreting its bits)
  const auto ok = [](int t) { return t == AGN_F32 || t == AGN_BF16 || t == AGN_F16; };
  if (!ok(d.src_dtype) || !ok(d.dst_dtype)) return;
  if (d.src_dtype == AGN_BF16) pack_one<bf16>(d, tid);
  else if (d.src_dtype == AGN_F16) pack_one<f16>(d, tid);
  else pack_one<float>(d, tid);
}

__global__ void reduce_partials_kernel(const float* __restrict__ p, int nw, int n, float* __restrict__ out) {
  const int cidx = blockIdx.x * blockDim.x + threadIdx.x;
  if (cidx >= n) return;
  float s = 0.f;
  for (int w = 0; w < nw; ++w) s += p[(size_t)w * n + cidx];
  out[cidx] = s;
}

}  // namespace

extern "C" {

size_t agn_packed_bytes(int m, int k, int dtype) {
  return (size_t)((m + 31) / 32) * ((k + 15) / 16) * 1024 * (dtype == AGN_F32 ? 2 : 1);
}

int agn_pack(const agn_pack_desc* descs_device, int n, int max_threads, void* stream) {
  if (n <= 0) return 0;
  if (max_threads <= 0) return AGN_E_ARG;
  dim3 grid((max_threads + 255) / 256, n);
  hipLaunchKernelGGL(pack_kernel, grid, dim3(256), 0, (hipStream_t)stream, descs_device);
  return launch_status();
}

int agn_reduce_partials(const float* partial, int nw, int n, float* out, void* stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(reduce_partials_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                     partial, nw, n, out);
  return launch_status();
}

}  // extern "C"
