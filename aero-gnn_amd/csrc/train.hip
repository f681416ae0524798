// The training tail on the device: what the reference does with the prediction after `model(...)`
// (utils.py:191-195 loss_fn(pred, y), loss.backward()'s first step, total_loss += loss.item();
// train.py:207-212 with utils.py:193 torch.optim.Adam.step()).
//
// agn_mse_loss: ONE pass over pred and y gives the MSE value and its gradient. d = (double)pred -
// (double)y; the squares and every sum are fp64. The reduction has two stages with a fixed tree
// shape and no atomics (the manner of aero.hip): stage 1, one block per chunk of MSE_ROWS rows,
// thread t takes the chunk's elements t, t + 256, ... in ascending order and the block adds its 256
// threads in a halving tree; stage 2, one block, thread t adds the chunk partials t, t + 256, ... in
// ascending order, the same tree adds the threads, and thread 0 alone writes S / n_global and adds it
// to the epoch accumulator. The shape depends on (n, f) only: two calls give identical bytes.
// dpred = (2 d) / n_global in fp64 with an IEEE division, rounded fp64 -> fp32 -> pred's dtype (RNE
// at each step; once for fp64): the roundings of torch.Tensor.to() applied to the fp64 value.
//
// agn_adam_step: torch's single-tensor Adam (L2 weight decay, no amsgrad) for a whole parameter list
// in one launch. A device-resident descriptor table holds one entry per tensor, a device-resident
// chunk map cuts the list into (tensor, chunk) pairs of ADAM_CHUNK elements; the grid is capped and
// walks the map with a grid stride. 16-B loads and stores where the tensor's four pointers allow it,
// scalar otherwise. Every elementwise step is one correctly rounded operation in the tensor dtype, in
// torch's order (the whole file is compiled with `#pragma clang fp contract(off)`: nothing is fused).
//
// agn_adam_step_master: the same step for bf16 / fp16 parameters (train.py:30-38 makes them 16-bit,
// train.py:207-212 steps them) with an fp32 master copy w and fp32 moments per tensor. Per element
// w = (bits(round_T(w)) == bits(p)) ? w : (float)p, then adam_elem<float> on (w, (float)g, m, v) exactly
// as agn_adam_step runs it on an fp32 tensor, then p = round_T(w). 8 elements per thread where the
// five pointers are 16-B aligned (one 16-B access for p and g, two for w, m, v), scalar otherwise.
//
// Loss scaling (the reference's `precision: float16`, train.py:35-38): a 16-byte agn_loss_scale_state in
// device memory holds the scale S, the found_inf flag, the growth tracker and the skipped-step count.
// agn_mse_loss_scaled multiplies the fp64 gradient by S before its one rounding chain; agn_grad_check reads
// every live gradient of a table once (exponent bits all ones = inf / NaN) and sets found_inf;
// agn_adam_step_scaled / agn_adam_step_master_scaled are the two Adam kernels with g * (float)(1 / S) in front of
// adam_elem, and return at once when found_inf is set; agn_loss_scale_update is torch._amp_update_scale_ on
// the state, by one thread. The unscaled entry points launch the same templates without a state.
#include "common.hpp"
#include "host.hpp"
#include "aerognn.h"

using namespace agn;

#pragma clang fp contract(off)

namespace {

constexpr int MSE_ROWS = 2048;     // rows per stage-1 chunk
constexpr int TR_THREADS = 256;
constexpr int ADAM_CHUNK = 4096;   // elements per chunk-map entry (a multiple of 4: chunk starts keep the tensor's alignment)
constexpr int ADAM_MAX_BLOCKS = 2048;

// the sum of the block's 256 values in a fixed halving tree; thread 0 holds it on return
AGN_DEV double block_tree_sum(double v, double* sh, int t) {
  sh[t] = v;
  __syncthreads();
#pragma unroll
  for (int h = TR_THREADS / 2; h >= 1; h >>= 1) {
    if (t < h) sh[t] += sh[t + h];
    __syncthreads();
  }
  return sh[0];
}

// fp64 -> fp32 -> T with RNE at each step (fp64: one rounding, none)
template <typename T> AGN_DEV T round_from_f64(double v) { return from_f<T>((float)v); }
template <> AGN_DEV double round_from_f64<double>(double v) { return v; }
template <> AGN_DEV float round_from_f64<float>(double v) { return (float)v; }

// stage 1: part[b] = sum of d^2 over rows [b * MSE_ROWS, ...), dpred written on the way
template <typename T, typename TY>
__global__ void __launch_bounds__(TR_THREADS)
mse_chunk_kernel(int n, int f, const T* __restrict__ pred, int pred_ld, const TY* __restrict__ y, int y_ld,
                 double n_global, T* __restrict__ dpred, int dpred_ld, double* __restrict__ part,
                 const agn_loss_scale_state* __restrict__ state) {
  __shared__ double sh[TR_THREADS];
  const double scale = state ? (double)state->scale : 1.0;
  const int t = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * MSE_ROWS;
  const int rows = (int)min((int64_t)MSE_ROWS, (int64_t)n - r0);  // >= 1: the grid is ceil(n / MSE_ROWS)
  const int cnt = rows * f;                                       // <= MSE_ROWS * f, checked by the host
  double s = 0.0;
  for (int e = t; e < cnt; e += TR_THREADS) {
    const int r = e / f, j = e - r * f;
    const size_t row = (size_t)(r0 + r);
    const double d = (double)pred[row * pred_ld + j] - (double)y[row * y_ld + j];
    s += d * d;
    if (dpred) {
      double q = (2.0 * d) / n_global;
      if (state) q = q * scale;  // before the rounding to T: what T cannot hold unscaled survives
      dpred[row * dpred_ld + j] = round_from_f64<T>(q);
    }
  }
  s = block_tree_sum(s, sh, t);
  if (t == 0) part[blockIdx.x] = s;
}

// stage 2: loss = (sum of the partials, fixed order) / n_global; *acc += loss by thread 0 alone
__global__ void __launch_bounds__(TR_THREADS)
mse_finish_kernel(int nchunk, const double* __restrict__ part, double n_global, double* __restrict__ loss_out,
                  double* __restrict__ acc) {
  __shared__ double sh[TR_THREADS];
  const int t = threadIdx.x;
  double s = 0.0;
  for (int c = t; c < nchunk; c += TR_THREADS) s += part[c];
  s = block_tree_sum(s, sh, t);
  if (t == 0) {
    const double loss = s / n_global;
    *loss_out = loss;
    if (acc) *acc += loss;
  }
}

template <typename T, typename TY>
void launch_mse(int n, int f, const void* pred, int pred_ld, const void* y, int y_ld, double n_global, void* dpred,
                int dpred_ld, double* part, const agn_loss_scale_state* state, hipStream_t st) {
  const int nchunk = (int)(((int64_t)n + MSE_ROWS - 1) / MSE_ROWS);
  hipLaunchKernelGGL((mse_chunk_kernel<T, TY>), dim3(nchunk), dim3(TR_THREADS), 0, st, n, f, (const T*)pred, pred_ld,
                     (const TY*)y, y_ld, n_global, (T*)dpred, dpred_ld, part, state);
}

// ---------------------------------------------------------------------------- Adam
template <typename T> AGN_DEV T sqrt_rn(T a);
template <> AGN_DEV float sqrt_rn<float>(float a) { return __fsqrt_rn(a); }
template <> AGN_DEV double sqrt_rn<double>(double a) { return sqrt(a); }
template <typename T> AGN_DEV T quot_rn(T a, T b);
template <> AGN_DEV float quot_rn<float>(float a, float b) { return __fdiv_rn(a, b); }
template <> AGN_DEV double quot_rn<double>(double a, double b) { return a / b; }

// the per-tensor scalars rounded to the tensor dtype (torch passes 1 - beta as one Python double)
template <typename T>
struct AdamK {
  T omb1, beta1, beta2, omb2, eps, wd, step_size, bc2_sqrt;
  bool decay, lerp_lo;  // lerp_lo: 1 - beta1 < 0.5, the branch of torch's lerp that starts from exp_avg
};

// one element, torch's _single_tensor_adam in its order:
//   grad.add(param, alpha=wd); exp_avg.lerp_(grad, 1 - beta1); exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
//   denom = (exp_avg_sq.sqrt() / bc2_sqrt).add_(eps); param.addcdiv_(exp_avg, denom, value=-step_size)
template <typename T>
AGN_DEV void adam_elem(T& p, T g, T& m, T& v, const AdamK<T>& k) {
  if (k.decay) g = g + k.wd * p;
  m = k.lerp_lo ? m + k.omb1 * (g - m) : g - (g - m) * k.beta1;
  v = v * k.beta2 + k.omb2 * (g * g);
  const T denom = quot_rn<T>(sqrt_rn<T>(v), k.bc2_sqrt) + k.eps;
  p = p - k.step_size * quot_rn<T>(m, denom);
}

// D: agn_adam_desc or agn_adam_master_desc (the same six doubles)
template <typename T, typename D>
AGN_DEV AdamK<T> adam_scalars(const D& d) {
  AdamK<T> k;
  k.omb1 = (T)(1.0 - d.beta1);
  k.beta1 = (T)1 - k.omb1;
  k.lerp_lo = fabs((double)k.omb1) < 0.5;  // torch's lerp tests the weight as rounded to the tensor dtype
  k.beta2 = (T)d.beta2;
  k.omb2 = (T)(1.0 - d.beta2);
  k.eps = (T)d.eps;
  k.wd = (T)d.weight_decay;
  k.decay = d.weight_decay != 0.0;
  k.step_size = (T)d.step_size;
  k.bc2_sqrt = (T)d.bc2_sqrt;
  return k;
}

template <typename T> struct Vec16;
template <> struct Vec16<float> { typedef f32x4 type; static constexpr int W = 4; };
typedef double f64x2 __attribute__((ext_vector_type(2)));
template <> struct Vec16<double> { typedef f64x2 type; static constexpr int W = 2; };

// SC: the loss-scaled step. found_inf set: nothing is touched; else g * inv in front of adam_elem, one
// rounding in T, inv = (float)(1 / (double)S) as torch.amp.GradScaler forms it
template <bool SC, typename T>
AGN_DEV T unscaled(T g, T inv) { return SC ? g * inv : g; }

template <typename T, bool SC>
__global__ void __launch_bounds__(TR_THREADS)
adam_kernel(const agn_adam_desc* __restrict__ descs, int ntensor, const int32_t* __restrict__ cmap, int nchunk,
            int dtype, const agn_loss_scale_state* __restrict__ state) {
  typedef typename Vec16<T>::type V;
  constexpr int W = Vec16<T>::W;
  const int t = threadIdx.x;
  T inv = (T)1;
  if (SC) {
    if (state->found_inf != 0) return;
    inv = (T)(float)(1.0 / (double)state->scale);
  }
  for (int c = blockIdx.x; c < nchunk; c += gridDim.x) {  // block-uniform walk of the chunk map
    const int ti = cmap[2 * c], ci = cmap[2 * c + 1];
    if (ti < 0 || ti >= ntensor || ci < 0) continue;     // a malformed map entry touches nothing
    const agn_adam_desc d = descs[ti];
    if (d.dtype != dtype || !d.p || !d.g || !d.m || !d.v) continue;
    const int64_t e0 = (int64_t)ci * ADAM_CHUNK;
    if (e0 >= d.n) continue;                              // n == 0: a parameter without a gradient
    const int len = (int)min((int64_t)ADAM_CHUNK, d.n - e0);
    const AdamK<T> k = adam_scalars<T>(d);
    T* p = (T*)d.p + e0;
    const T* g = (const T*)d.g + e0;
    T* m = (T*)d.m + e0;
    T* v = (T*)d.v + e0;
    // e0 * sizeof(T) is a multiple of 16, so the chunk is aligned exactly when the tensor is
    const bool vec = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                       reinterpret_cast<uintptr_t>(v)) & 15) == 0;
    const int nv = vec ? len / W : 0;
    for (int i = t; i < nv; i += TR_THREADS) {
      V pv = reinterpret_cast<V*>(p)[i], mv = reinterpret_cast<V*>(m)[i], vv = reinterpret_cast<V*>(v)[i];
      const V gv = reinterpret_cast<const V*>(g)[i];
#pragma unroll
      for (int q = 0; q < W; ++q) {
        T pe = pv[q], me = mv[q], ve = vv[q];
        adam_elem<T>(pe, unscaled<SC, T>(gv[q], inv), me, ve, k);
        pv[q] = pe; mv[q] = me; vv[q] = ve;
      }
      reinterpret_cast<V*>(p)[i] = pv;
      reinterpret_cast<V*>(m)[i] = mv;
      reinterpret_cast<V*>(v)[i] = vv;
    }
    for (int i = nv * W + t; i < len; i += TR_THREADS) adam_elem<T>(p[i], unscaled<SC, T>(g[i], inv), m[i], v[i], k);
  }
}

// ---------------------------------------------------------------------------- Adam with fp32 master weights
typedef uint16_t u16x8 __attribute__((ext_vector_type(8)));
constexpr int MW = 8;  // elements per thread on the wide path: 16 B of p and of g, 2 x 16 B of w, m and v

// one element: pb / gb are the 16-bit patterns of p and g (T = bf16 or f16). The master follows the
// parameter: an element whose p is not round_T(w) (something wrote p since the last step) restarts from
// (float)p and keeps its moments; the patterns are compared, so +-0 and NaN need no case of their own.
template <typename T, bool SC>
AGN_DEV void adam_master_elem(uint16_t& pb, uint16_t gb, float& w, float& m, float& v, const AdamK<float>& k,
                              float inv) {
  if (__builtin_bit_cast(uint16_t, from_f<T>(w)) != pb) w = to_f(__builtin_bit_cast(T, pb));
  adam_elem<float>(w, unscaled<SC, float>(to_f(__builtin_bit_cast(T, gb)), inv), m, v, k);
  pb = __builtin_bit_cast(uint16_t, from_f<T>(w));
}

template <typename T, bool SC>
__global__ void __launch_bounds__(TR_THREADS)
adam_master_kernel(const agn_adam_master_desc* __restrict__ descs, int ntensor, const int32_t* __restrict__ cmap,
                   int nchunk, int dtype, const agn_loss_scale_state* __restrict__ state) {
  const int t = threadIdx.x;
  float inv = 1.0f;
  if (SC) {
    if (state->found_inf != 0) return;
    inv = (float)(1.0 / (double)state->scale);
  }
  for (int c = blockIdx.x; c < nchunk; c += gridDim.x) {  // block-uniform walk of the chunk map
    const int ti = cmap[2 * c], ci = cmap[2 * c + 1];
    if (ti < 0 || ti >= ntensor || ci < 0) continue;     // a malformed map entry touches nothing
    const agn_adam_master_desc d = descs[ti];
    if (d.dtype != dtype || !d.p || !d.g || !d.w || !d.m || !d.v) continue;
    const int64_t e0 = (int64_t)ci * ADAM_CHUNK;
    if (e0 >= d.n) continue;                              // n == 0: a parameter without a gradient
    const int len = (int)min((int64_t)ADAM_CHUNK, d.n - e0);
    const AdamK<float> k = adam_scalars<float>(d);
    uint16_t* p = (uint16_t*)d.p + e0;
    const uint16_t* g = (const uint16_t*)d.g + e0;
    float* w = (float*)d.w + e0;
    float* m = (float*)d.m + e0;
    float* v = (float*)d.v + e0;
    // e0 * 2 is a multiple of 16, so the chunk is aligned exactly when the tensor is
    const bool vec = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(w) |
                       reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v)) & 15) == 0;
    const int nv = vec ? len / MW : 0;
    for (int i = t; i < nv; i += TR_THREADS) {
      u16x8 pv = reinterpret_cast<u16x8*>(p)[i];
      const u16x8 gv = reinterpret_cast<const u16x8*>(g)[i];
      f32x4 wv[2], mv[2], vv[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        wv[h] = reinterpret_cast<f32x4*>(w)[2 * i + h];
        mv[h] = reinterpret_cast<f32x4*>(m)[2 * i + h];
        vv[h] = reinterpret_cast<f32x4*>(v)[2 * i + h];
      }
#pragma unroll
      for (int q = 0; q < MW; ++q) {
        uint16_t pb = pv[q];
        float we = wv[q / 4][q % 4], me = mv[q / 4][q % 4], ve = vv[q / 4][q % 4];
        adam_master_elem<T, SC>(pb, gv[q], we, me, ve, k, inv);
        pv[q] = pb; wv[q / 4][q % 4] = we; mv[q / 4][q % 4] = me; vv[q / 4][q % 4] = ve;
      }
      reinterpret_cast<u16x8*>(p)[i] = pv;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        reinterpret_cast<f32x4*>(w)[2 * i + h] = wv[h];
        reinterpret_cast<f32x4*>(m)[2 * i + h] = mv[h];
        reinterpret_cast<f32x4*>(v)[2 * i + h] = vv[h];
      }
    }
    for (int i = nv * MW + t; i < len; i += TR_THREADS)
      adam_master_elem<T, SC>(p[i], g[i], w[i], m[i], v[i], k, inv);
  }
}

// ---------------------------------------------------------------------------- loss scaling: check and update
AGN_DEV bool adam_entry_live(const agn_adam_desc& d) { return d.p && d.g && d.m && d.v; }
AGN_DEV bool adam_entry_live(const agn_adam_master_desc& d) { return d.p && d.g && d.w && d.m && d.v; }

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));
template <typename U> struct Chk16;  // 16 B of the element's bit pattern
template <> struct Chk16<uint16_t> { typedef u16x8 type; };
template <> struct Chk16<uint32_t> { typedef u32x4 type; };
template <> struct Chk16<uint64_t> { typedef u64x2 type; };

// Read-only pass over the gradients agn_adam_step / agn_adam_step_master would step: the same walk of the
// chunk map and the same skipped entries. U: the element's bit pattern, EXP: its exponent field; all ones
// there is +-inf or NaN. A thread that saw one stores the flag (every writer stores the same 1).
template <typename D, typename U, U EXP>
__global__ void __launch_bounds__(TR_THREADS)
grad_check_kernel(const D* __restrict__ descs, int ntensor, const int32_t* __restrict__ cmap, int nchunk, int dtype,
                  agn_loss_scale_state* __restrict__ state) {
  typedef typename Chk16<U>::type V;
  constexpr int W = 16 / (int)sizeof(U);
  const int t = threadIdx.x;
  bool bad = false;
  for (int c = blockIdx.x; c < nchunk; c += gridDim.x) {  // block-uniform walk of the chunk map
    const int ti = cmap[2 * c], ci = cmap[2 * c + 1];
    if (ti < 0 || ti >= ntensor || ci < 0) continue;
    const D d = descs[ti];
    if (d.dtype != dtype || !adam_entry_live(d)) continue;
    const int64_t e0 = (int64_t)ci * ADAM_CHUNK;
    if (e0 >= d.n) continue;
    const int len = (int)min((int64_t)ADAM_CHUNK, d.n - e0);
    const U* g = (const U*)d.g + e0;
    const int nv = (reinterpret_cast<uintptr_t>(g) & 15) == 0 ? len / W : 0;
    for (int i = t; i < nv; i += TR_THREADS) {
      const V gv = reinterpret_cast<const V*>(g)[i];
#pragma unroll
      for (int q = 0; q < W; ++q) bad |= (gv[q] & EXP) == EXP;
    }
    for (int i = nv * W + t; i < len; i += TR_THREADS) bad |= (g[i] & EXP) == EXP;
  }
  if (bad) state->found_inf = 1;
}

template <typename D>
void launch_grad_check(const void* descs, int ntensor, const int32_t* cmap, int nchunk, int dtype,
                       agn_loss_scale_state* state, hipStream_t st) {
  const dim3 grid(nchunk < ADAM_MAX_BLOCKS ? nchunk : ADAM_MAX_BLOCKS), block(TR_THREADS);
  const D* d = (const D*)descs;
  switch (dtype) {
    case AGN_F32:
      hipLaunchKernelGGL((grad_check_kernel<D, uint32_t, 0x7f800000u>), grid, block, 0, st, d, ntensor, cmap, nchunk,
                         dtype, state);
      break;
    case AGN_F64:
      hipLaunchKernelGGL((grad_check_kernel<D, uint64_t, 0x7ff0000000000000ull>), grid, block, 0, st, d, ntensor, cmap,
                         nchunk, dtype, state);
      break;
    case AGN_BF16:
      hipLaunchKernelGGL((grad_check_kernel<D, uint16_t, (uint16_t)0x7f80>), grid, block, 0, st, d, ntensor, cmap,
                         nchunk, dtype, state);
      break;
    default:
      hipLaunchKernelGGL((grad_check_kernel<D, uint16_t, (uint16_t)0x7c00>), grid, block, 0, st, d, ntensor, cmap,
                         nchunk, dtype, state);
      break;
  }
}

// torch._amp_update_scale_ (amp_update_scale_cuda_kernel) on the state, then the flag is cleared
__global__ void loss_scale_update_kernel(agn_loss_scale_state* __restrict__ state, double growth, double backoff,
                                         int interval) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (state->found_inf != 0) {
    state->scale = (float)((double)state->scale * backoff);
    state->growth_tracker = 0;
    state->skipped = state->skipped + 1;
  } else {
    const int successful = state->growth_tracker + 1;
    if (successful == interval) {
      const float grown = (float)((double)state->scale * growth);
      if (isfinite(grown)) state->scale = grown;
      state->growth_tracker = 0;
    } else {
      state->growth_tracker = successful;
    }
  }
  state->found_inf = 0;
}

int mse_loss_impl(int dtype, int y_dtype, int n, int f, const void* pred, int pred_ld, const void* y, int y_ld,
                  double n_global, double* loss_out, double* acc, void* dpred, int dpred_ld, void* scratch,
                  const agn_loss_scale_state* state, void* stream) {
  if (n < 0) return AGN_E_ARG;
  if (dtype != AGN_F32 && dtype != AGN_BF16 && dtype != AGN_F16 && dtype != AGN_F64) return AGN_E_DTYPE;
  if (y_dtype != dtype && y_dtype != AGN_F32) return AGN_E_DTYPE;
  // f <= 2^31 / MSE_ROWS keeps a chunk's element count in an int
  if (f < 1 || f > (1 << 19) || pred_ld < f || y_ld < f || (dpred && dpred_ld < f)) return AGN_E_SHAPE;
  if (!(n_global > 0.0)) return AGN_E_SHAPE;
  if (!loss_out) return AGN_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) {  // loss 0, acc unchanged: a plain memset of the 8 bytes, no kernel
    const hipError_t e = hipMemsetAsync(loss_out, 0, sizeof(double), st);
    return e == hipSuccess ? 0 : (int)e;
  }
  if (!pred || !y || !scratch) return AGN_E_ARG;
  double* part = reinterpret_cast<double*>(scratch);
  const bool ysame = y_dtype == dtype;
#define AGN_MSE(T, TY) launch_mse<T, TY>(n, f, pred, pred_ld, y, y_ld, n_global, dpred, dpred_ld, part, state, st)
  switch (dtype) {
    case AGN_F32: AGN_MSE(float, float); break;
    case AGN_F64:
      if (ysame) AGN_MSE(double, double);
      else AGN_MSE(double, float);
      break;
    case AGN_BF16:
      if (ysame) AGN_MSE(bf16, bf16);
      else AGN_MSE(bf16, float);
      break;
    default:
      if (ysame) AGN_MSE(f16, f16);
      else AGN_MSE(f16, float);
      break;
  }
#undef AGN_MSE
  const int nchunk = (int)(((int64_t)n + MSE_ROWS - 1) / MSE_ROWS);
  hipLaunchKernelGGL(mse_finish_kernel, dim3(1), dim3(TR_THREADS), 0, st, nchunk, part, n_global, loss_out, acc);
  return launch_status();
}

// state == nullptr: the unscaled step
int adam_step_impl(const agn_adam_desc* descs, int ntensor, const int32_t* cmap, int nchunk, int dtype,
                   const agn_loss_scale_state* state, void* stream) {
  if (ntensor < 0 || nchunk < 0) return AGN_E_ARG;
  if (dtype != AGN_F32 && dtype != AGN_F64) return AGN_E_DTYPE;
  if (ntensor == 0 || nchunk == 0) return 0;
  if (!descs || !cmap) return AGN_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(nchunk < ADAM_MAX_BLOCKS ? nchunk : ADAM_MAX_BLOCKS), block(TR_THREADS);
#define AGN_ADAM(T, SC) \
  hipLaunchKernelGGL((adam_kernel<T, SC>), grid, block, 0, st, descs, ntensor, cmap, nchunk, dtype, state)
  if (dtype == AGN_F32) {
    if (state) AGN_ADAM(float, true);
    else AGN_ADAM(float, false);
  } else {
    if (state) AGN_ADAM(double, true);
    else AGN_ADAM(double, false);
  }
#undef AGN_ADAM
  return launch_status();
}

int adam_step_master_impl(const agn_adam_master_desc* descs, int ntensor, const int32_t* cmap, int nchunk, int dtype,
                          const agn_loss_scale_state* state, void* stream) {
  if (ntensor < 0 || nchunk < 0) return AGN_E_ARG;
  if (dtype != AGN_BF16 && dtype != AGN_F16) return AGN_E_DTYPE;
  if (ntensor == 0 || nchunk == 0) return 0;
  if (!descs || !cmap) return AGN_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(nchunk < ADAM_MAX_BLOCKS ? nchunk : ADAM_MAX_BLOCKS), block(TR_THREADS);
#define AGN_ADAM(T, SC) \
  hipLaunchKernelGGL((adam_master_kernel<T, SC>), grid, block, 0, st, descs, ntensor, cmap, nchunk, dtype, state)
  if (dtype == AGN_BF16) {
    if (state) AGN_ADAM(bf16, true);
    else AGN_ADAM(bf16, false);
  } else {
    if (state) AGN_ADAM(f16, true);
    else AGN_ADAM(f16, false);
  }
#undef AGN_ADAM
  return launch_status();
}

}  // namespace

extern "C" {

int agn_mse_chunk_rows(void) { return MSE_ROWS; }

size_t agn_mse_loss_temp_bytes(int n, int f) {
  if (n < 0 || f < 1) return 0;
  const size_t nchunk = (size_t)(((int64_t)n + MSE_ROWS - 1) / MSE_ROWS);
  return (sizeof(double) * (nchunk > 0 ? nchunk : 1) + 15) & ~(size_t)15;
}

int agn_mse_loss(int dtype, int y_dtype, int n, int f, const void* pred, int pred_ld, const void* y, int y_ld,
                 double n_global, double* loss_out, double* acc, void* dpred, int dpred_ld, void* scratch,
                 void* stream) {
  return mse_loss_impl(dtype, y_dtype, n, f, pred, pred_ld, y, y_ld, n_global, loss_out, acc, dpred, dpred_ld, scratch,
                       nullptr, stream);
}

int agn_mse_loss_scaled(int dtype, int y_dtype, int n, int f, const void* pred, int pred_ld, const void* y, int y_ld,
                        double n_global, double* loss_out, double* acc, void* dpred, int dpred_ld, void* scratch,
                        const agn_loss_scale_state* state_device, void* stream) {
  return mse_loss_impl(dtype, y_dtype, n, f, pred, pred_ld, y, y_ld, n_global, loss_out, acc, dpred, dpred_ld, scratch,
                       state_device, stream);
}

int agn_adam_chunk_elems(void) { return ADAM_CHUNK; }

int agn_adam_step(const agn_adam_desc* descs_device, int ntensor, const int32_t* chunk_map_device, int nchunk,
                  int dtype, void* stream) {
  return adam_step_impl(descs_device, ntensor, chunk_map_device, nchunk, dtype, nullptr, stream);
}

int agn_adam_step_master(const agn_adam_master_desc* descs_device, int ntensor, const int32_t* chunk_map_device,
                         int nchunk, int dtype, void* stream) {
  return adam_step_master_impl(descs_device, ntensor, chunk_map_device, nchunk, dtype, nullptr, stream);
}

int agn_adam_step_scaled(const agn_adam_desc* descs_device, int ntensor, const int32_t* chunk_map_device, int nchunk,
                         int dtype, const agn_loss_scale_state* state_device, void* stream) {
  if (!state_device) return AGN_E_ARG;
  return adam_step_impl(descs_device, ntensor, chunk_map_device, nchunk, dtype, state_device, stream);
}

int agn_adam_step_master_scaled(const agn_adam_master_desc* descs_device, int ntensor,
                                const int32_t* chunk_map_device, int nchunk, int dtype,
                                const agn_loss_scale_state* state_device, void* stream) {
  if (!state_device) return AGN_E_ARG;
  return adam_step_master_impl(descs_device, ntensor, chunk_map_device, nchunk, dtype, state_device, stream);
}

int agn_grad_check(const void* descs_device, int master, int ntensor, const int32_t* chunk_map_device, int nchunk,
                   int dtype, agn_loss_scale_state* state_device, void* stream) {
  if (ntensor < 0 || nchunk < 0 || !state_device) return AGN_E_ARG;
  if (dtype != AGN_F32 && dtype != AGN_F64 && dtype != AGN_BF16 && dtype != AGN_F16) return AGN_E_DTYPE;
  if (ntensor == 0 || nchunk == 0) return 0;
  if (!descs_device || !chunk_map_device) return AGN_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (master) launch_grad_check<agn_adam_master_desc>(descs_device, ntensor, chunk_map_device, nchunk, dtype,
                                                      state_device, st);
  else launch_grad_check<agn_adam_desc>(descs_device, ntensor, chunk_map_device, nchunk, dtype, state_device, st);
  return launch_status();
}

int agn_loss_scale_update(agn_loss_scale_state* state_device, double growth_factor, double backoff_factor,
                          int growth_interval, void* stream) {
  if (!state_device) return AGN_E_ARG;
  if (growth_interval < 1 || !(growth_factor > 0.0) || !(backoff_factor > 0.0)) return AGN_E_SHAPE;
  hipLaunchKernelGGL(loss_scale_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state_device, growth_factor,
                     backoff_factor, growth_interval);
  return launch_status();
}

}  // extern "C"
