// Fourier feature map of FourierMeshGraphNet (fouriermgn.py:111-151 fourier_embedding, and the
// torch.cat of :167-170): out[r] = [x[r] | cos(f_i x_j), sin(f_i x_j)], f_i = 2^(freq_start + i) pi.
// The reference builds it from arange / pow / mul / cos / sin and two cats; here it is one pass
// forward and one pass backward, with the reference's rounding sequence in the compute type C
// (fp32, or fp64 for AGN_F64; 16-bit rows are converted to fp32 and rounded once on store):
//   f_i = ldexp(C(pi), freq_start + i)   exact scaling of the rounded pi (torch: (2.0 ** i) * pi)
//   a   = f_i * x_j                      one rounding, never contracted into an FMA
//   cos(a), sin(a)                       the device library's accurate sincos
#include "common.hpp"
#include "host.hpp"
#include "aerognn.h"

using namespace agn;

// nothing in this file is contracted into an FMA: a = f_i * x_j is rounded on its own before the
// range reduction, and the backward's sums are the written sequence of multiplies and adds
#pragma clang fp contract(off)

namespace {

constexpr int FE_MAX_FREQ = 32;  // freq_len
constexpr int FE_MAX_EXP = 30;   // |freq_start|, |freq_start + freq_len|
constexpr int FE_THREADS = 256;
constexpr int FE_MAX_BLOCKS = 1 << 20;  // grid-stride beyond this many blocks

template <typename C> struct Trig;
template <> struct Trig<float> {
  static AGN_DEV float freq(int e) { return ldexpf(3.14159265358979323846f, e); }
  static AGN_DEV float arg(float f, float x) { return f * x; }
  static AGN_DEV void sc(float a, float* s, float* c) { sincosf(a, s, c); }
};
template <> struct Trig<double> {
  static AGN_DEV double freq(int e) { return ldexp(3.14159265358979323846, e); }
  static AGN_DEV double arg(double f, double x) { return f * x; }
  static AGN_DEV void sc(double a, double* s, double* c) { sincos(a, s, c); }
};

// one thread per output element (consecutive threads write consecutive columns of a row)
template <typename T, typename C>
__global__ void fourier_embed_kernel(int64_t total, int w, int koff, int F, int freq_start,
                                     const T* __restrict__ x, int ld, T* __restrict__ out, int out_ld) {
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += step) {
    const int64_t r = t / w;
    const int c = (int)(t - r * w);
    const T* xr = x + r * ld;
    T* o = out + r * out_ld + c;
    if (c < koff) {
      *o = xr[c];
      continue;
    }
    const int e = c - koff;
    const int j = e / (2 * F), q = e - j * 2 * F;
    const int i = q < F ? q : q - F;
    const C a = Trig<C>::arg(Trig<C>::freq(freq_start + i), (C)xr[j]);
    C s, cs;
    Trig<C>::sc(a, &s, &cs);
    *o = (T)(q < F ? cs : s);
  }
}

// one thread per input element: dx[r][j] = pass-through + sum_i f_i (cos(a) g_sin - sin(a) g_cos),
// i ascending, accumulated in C, one rounding
template <typename T, typename C>
__global__ void fourier_embed_bwd_kernel(int64_t total, int k, int d, int koff, int F, int freq_start,
                                         const T* __restrict__ x, int ld, const T* __restrict__ g, int g_ld,
                                         T* __restrict__ dx, int dx_ld) {
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += step) {
    const int64_t r = t / k;
    const int j = (int)(t - r * k);
    const T* gr = g + r * g_ld;
    C acc = koff ? (C)gr[j] : (C)0;
    if (j < d) {
      const C xv = (C)x[r * ld + j];
      const T* gc = gr + koff + j * 2 * F;
      for (int i = 0; i < F; ++i) {
        const C f = Trig<C>::freq(freq_start + i);
        C s, cs;
        Trig<C>::sc(Trig<C>::arg(f, xv), &s, &cs);
        acc += f * (cs * (C)gc[F + i] - s * (C)gc[i]);
      }
    }
    dx[r * dx_ld + j] = (T)acc;
  }
}

int blocks_for(int64_t total) {
  const int64_t b = (total + FE_THREADS - 1) / FE_THREADS;
  return (int)(b < FE_MAX_BLOCKS ? b : FE_MAX_BLOCKS);
}

// argument checks shared by both entries; row = the width of [x | emb] or emb
int check_args(int dtype, int n, int k, int ld, int d, int freq_start, int freq_len, int with_input, int* row) {
  if (n < 0) return AGN_E_ARG;
  if (dtype != AGN_F32 && dtype != AGN_BF16 && dtype != AGN_F16 && dtype != AGN_F64) return AGN_E_DTYPE;
  if (d < 1 || d > k || freq_len < 1 || freq_len > FE_MAX_FREQ) return AGN_E_SHAPE;
  if (freq_start < -FE_MAX_EXP || freq_start > FE_MAX_EXP || freq_start + freq_len < -FE_MAX_EXP ||
      freq_start + freq_len > FE_MAX_EXP)
    return AGN_E_SHAPE;
  if (ld < k) return AGN_E_SHAPE;
  const int64_t w = (int64_t)(with_input ? k : 0) + 2 * (int64_t)d * freq_len;
  if (w > INT32_MAX) return AGN_E_SHAPE;
  *row = (int)w;
  return 0;
}

template <typename T, typename C>
void launch_fwd(int n, int k, const void* x, int ld, int freq_start, int F, int with_input, int w, void* out,
                int out_ld, hipStream_t st) {
  const int64_t total = (int64_t)n * w;
  hipLaunchKernelGGL((fourier_embed_kernel<T, C>), dim3(blocks_for(total)), dim3(FE_THREADS), 0, st, total, w,
                     with_input ? k : 0, F, freq_start, (const T*)x, ld, (T*)out, out_ld);
}

template <typename T, typename C>
void launch_bwd(int n, int k, int d, const void* x, int ld, int freq_start, int F, int with_input, const void* g,
                int g_ld, void* dx, int dx_ld, hipStream_t st) {
  const int64_t total = (int64_t)n * k;
  hipLaunchKernelGGL((fourier_embed_bwd_kernel<T, C>), dim3(blocks_for(total)), dim3(FE_THREADS), 0, st, total, k, d,
                     with_input ? k : 0, F, freq_start, (const T*)x, ld, (const T*)g, g_ld, (T*)dx, dx_ld);
}

}  // namespace

extern "C" {

int agn_fourier_embed(int dtype, int n, int k, const void* x, int ld, int d, int freq_start, int freq_len,
                      int with_input, void* out, int out_ld, void* stream) {
  if (n > 0 && (!x || !out)) return AGN_E_ARG;
  int w = 0;
  const int rc = check_args(dtype, n, k, ld, d, freq_start, freq_len, with_input, &w);
  if (rc) return rc;
  if (out_ld < w) return AGN_E_SHAPE;
  if (n == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  switch (dtype) {
    case AGN_F32: launch_fwd<float, float>(n, k, x, ld, freq_start, freq_len, with_input, w, out, out_ld, st); break;
    case AGN_BF16: launch_fwd<bf16, float>(n, k, x, ld, freq_start, freq_len, with_input, w, out, out_ld, st); break;
    case AGN_F16: launch_fwd<f16, float>(n, k, x, ld, freq_start, freq_len, with_input, w, out, out_ld, st); break;
    default: launch_fwd<double, double>(n, k, x, ld, freq_start, freq_len, with_input, w, out, out_ld, st); break;
  }
  return launch_status();
}

int agn_fourier_embed_bwd(int dtype, int n, int k, const void* x, int ld, int d, int freq_start, int freq_len,
                          int with_input, const void* g, int g_ld, void* dx, int dx_ld, void* stream) {
  if (n > 0 && (!x || !g || !dx)) return AGN_E_ARG;
  int w = 0;
  const int rc = check_args(dtype, n, k, ld, d, freq_start, freq_len, with_input, &w);
  if (rc) return rc;
  if (g_ld < w || dx_ld < k) return AGN_E_SHAPE;
  if (n == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const int F = freq_len;
  switch (dtype) {
    case AGN_F32: launch_bwd<float, float>(n, k, d, x, ld, freq_start, F, with_input, g, g_ld, dx, dx_ld, st); break;
    case AGN_BF16: launch_bwd<bf16, float>(n, k, d, x, ld, freq_start, F, with_input, g, g_ld, dx, dx_ld, st); break;
    case AGN_F16: launch_bwd<f16, float>(n, k, d, x, ld, freq_start, F, with_input, g, g_ld, dx, dx_ld, st); break;
    default: launch_bwd<double, double>(n, k, d, x, ld, freq_start, F, with_input, g, g_ld, dx, dx_ld, st); break;
  }
  return launch_status();
}

}  // extern "C"
