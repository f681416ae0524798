// Evaluation on the device: the prediction-error sums behind MAE / MSE / RRMSE in both scales
// (inference.py:76-126 predict_single's de-normalisation, compute_errors, compute_rrmse_percent;
// :337-350 and :395-413 the per-case and test-set torch.mean passes) and the surface integration
// of pressure and wall shear into forces and moments (utils.py:385-448, :451-559, with the
// per-edge Python loop of :510-520 that builds the 2-D node areas). The reference copies every
// prediction to the host and runs ~20 torch.mean passes per case; here each quantity is one pass
// over the device arrays plus one finishing pass.
//
// Reductions (both entries; the code is in aero_reduce.hpp, shared with surface.hip): fp64
// accumulators, two stages, no atomics and nothing passed between workgroups. Stage 1: one block per chunk of AERO_ROWS rows; chunks are laid out from each graph's
// first row (not from row 0 of the batch), so graph g of a batch is cut exactly as it is when it
// is evaluated alone. Thread t owns one column j = t % f and takes the chunk's elements t, t + S,
// t + 2 S, ... (S = the largest multiple of f <= 256) in ascending order; the block then adds the
// S / f threads of a column in a fixed halving tree. Stage 2: one block per graph adds that graph's
// chunk partials in ascending chunk order. Every sum therefore has a fixed shape that depends on
// the graph's own row count only: results are bitwise reproducible and batch independent.
// A block finds its (graph, chunk) by binary search in the exclusive scan of the per-graph chunk
// counts (agn_exclusive_scan_i32); the launch has the host-known bound ceil(n / R) + ngraph blocks
// and blocks past the real total exit.
//
// Rounding contract: every elementwise step up to and including d = p - t and d / t is ONE
// correctly rounded operation in the input type (fp32 or fp64), in the reference's order:
//   physical scale  p = pred * std (rounded), then + mean (rounded): two torch ops, never an FMA
//   d = p - t; q = d / t (IEEE division); pn = pressure * normal (utils.py:524, fp32 x fp32)
//   coordinate differences pos[dst] - pos[v] of the area rule
// and everything after (|d|, d^2, |q|, q^2, norms, areas, forces, moments, the sums) is fp64 formed
// from those rounded values. The whole file is compiled with `#pragma clang fp contract(off)`:
// no multiply-add written here is fused, in either precision.
#include "common.hpp"
#include "host.hpp"
#include "aerognn.h"

#pragma clang fp contract(off)

#include "aero_reduce.hpp"  // chunk layout, the block tree and the finishing pass (shared with surface.hip)

using namespace agn;
using namespace agn::red;

namespace {

constexpr int AERO_NACC = 12;     // fp64 accumulators per thread, both entries
constexpr int AERO_MAX_F = 16;

template <typename T> AGN_DEV T div_rn(T a, T b);
template <> AGN_DEV float div_rn<float>(float a, float b) { return __fdiv_rn(a, b); }
template <> AGN_DEV double div_rn<double>(double a, double b) { return a / b; }

// the six sums of one scale for one element: a[0..5] += |d|, d^2, |t|, [|t| > 1e-8], |d/t|, (d/t)^2
template <typename T>
AGN_DEV void error_terms(double* a, T p, T t) {
  const T d = p - t;
  const double dd = (double)d, at = fabs((double)t);
  a[0] += fabs(dd);
  a[1] += dd * dd;
  a[2] += at;
  if (at > 1e-8) {
    const double qq = (double)div_rn<T>(d, t);
    a[3] += 1.0;
    a[4] += fabs(qq);
    a[5] += qq * qq;
  }
}

// stage 1 of agn_eval_sums: part[b][s][j][6] for chunk b
template <typename T>
__global__ void __launch_bounds__(AERO_THREADS)
eval_chunk_kernel(int n, int f, int ngraph, const T* __restrict__ pred, int pred_ld, const T* __restrict__ y, int y_ld,
                  const T* __restrict__ mean, const T* __restrict__ std, const int32_t* __restrict__ gptr,
                  const int32_t* __restrict__ coff, double* __restrict__ part) {
  __shared__ double sh[AERO_NACC][AERO_THREADS];
  int g, r0, r1;
  if (!find_chunk(blockIdx.x, n, ngraph, gptr, coff, &g, &r0, &r1)) return;  // block-uniform
  const int t = threadIdx.x;
  const int Q = AERO_THREADS / f;  // threads per column; S = Q * f
  const int q = t / f, j = t - q * f;
  double a[AERO_NACC];
#pragma unroll
  for (int k = 0; k < AERO_NACC; ++k) a[k] = 0.0;
  if (q < Q) {
    const T sd = std[j], mu = mean[j];
    for (int r = r0 + q; r < r1; r += Q) {
      const T pv = pred[(size_t)r * pred_ld + j], tv = y[(size_t)r * y_ld + j];
      error_terms<T>(a, pv, tv);                               // normalised scale
      const T pp = pv * sd + mu, tp = tv * sd + mu;            // two roundings each (contract off)
      error_terms<T>(a + 6, pp, tp);                           // physical scale
    }
  }
  column_tree_reduce<AERO_NACC>(a, sh, t, f, Q);
  if (t < f) {
    double* o = part + (size_t)blockIdx.x * (AERO_NACC * f);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      o[(size_t)t * 6 + k] = a[k];
      o[((size_t)f + t) * 6 + k] = a[6 + k];
    }
  }
}

struct ForceArgs {
  int n, dim, ngraph;
  int shear_ld, normals_ld, pos_ld;
  const void *pressure, *shear, *normals, *pos;
  const double* areas;
  const int64_t* edge_index;
  int64_t e;
  const int32_t *rowptr, *perm;
  double half_scale;  // 0.5 * length_scale
  double* area_out;
  double center[3];
  const int32_t *gptr, *coff;
  double* part;
};

// stage 1 of agn_aero_forces: one thread per element, part[b] = [F(3) | M(3) | |F|(3) | |M|(3)]
// (2-D: F = (Fx, Fy, 0), M = (Mz, 0, 0))
template <typename T>
__global__ void __launch_bounds__(AERO_THREADS) force_chunk_kernel(const ForceArgs A) {
  __shared__ double sh[AERO_NACC][AERO_THREADS];
  int g, r0, r1;
  if (!find_chunk(blockIdx.x, A.n, A.ngraph, A.gptr, A.coff, &g, &r0, &r1)) return;  // block-uniform
  const int t = threadIdx.x, dim = A.dim;
  const T* pressure = (const T*)A.pressure;
  const T* shear = (const T*)A.shear;
  const T* normals = (const T*)A.normals;
  const T* pos = (const T*)A.pos;
  double a[AERO_NACC];
#pragma unroll
  for (int k = 0; k < AERO_NACC; ++k) a[k] = 0.0;
  for (int v = r0 + t; v < r1; v += AERO_THREADS) {
    double area;
    if (A.areas) {
      area = A.areas[v];
    } else {
      // utils.py:510-520: the node's outgoing edges in the caller's edge order (stable sender grouping)
      area = 0.0;
      T pv[3] = {0, 0, 0};
      for (int c = 0; c < dim; ++c) pv[c] = pos[(size_t)v * A.pos_ld + c];
      const int k0 = max(A.rowptr[v], 0);
      const int64_t k1 = min((int64_t)A.rowptr[v + 1], A.e);
      for (int64_t k = k0; k < k1; ++k) {
        const int32_t ed = A.perm[k];
        if (ed < 0 || ed >= A.e) continue;
        const int64_t d = A.edge_index[A.e + ed];
        if (d < 0 || d >= A.n) continue;
        double ss = 0.0;
        for (int c = 0; c < dim; ++c) {
          const T df = pos[(size_t)d * A.pos_ld + c] - pv[c];  // in the input type
          ss += (double)df * (double)df;
        }
        area += sqrt(ss) * A.half_scale;
      }
      if (A.area_out) A.area_out[v] = area;
    }
    const T p = pressure[v];
    double F[3] = {0.0, 0.0, 0.0}, r[3] = {0.0, 0.0, 0.0};
    for (int c = 0; c < dim; ++c) {
      const T pn = p * normals[(size_t)v * A.normals_ld + c];  // one rounding in the input type
      F[c] = (double)pn * area - (double)shear[(size_t)v * A.shear_ld + c] * area;
      if (pos) r[c] = (double)pos[(size_t)v * A.pos_ld + c] - A.center[c];
    }
    double M[3] = {0.0, 0.0, 0.0};
    if (pos) {
      if (dim == 2) {
        M[0] = r[0] * F[1] - r[1] * F[0];
      } else {
        M[0] = r[1] * F[2] - r[2] * F[1];
        M[1] = r[2] * F[0] - r[0] * F[2];
        M[2] = r[0] * F[1] - r[1] * F[0];
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      a[c] += F[c];
      a[3 + c] += M[c];
      a[6 + c] += fabs(F[c]);
      a[9 + c] += fabs(M[c]);
    }
  }
  column_tree_reduce<AERO_NACC>(a, sh, t, 1, AERO_THREADS);
  if (t == 0) {
    double* o = A.part + (size_t)blockIdx.x * AERO_NACC;
#pragma unroll
    for (int k = 0; k < AERO_NACC; ++k) o[k] = a[k];
  }
}

}  // namespace

extern "C" {

int agn_aero_chunk_rows(void) { return AERO_ROWS; }

size_t agn_eval_sums_temp_bytes(int n, int f, int ngraph) {
  if (n < 0 || ngraph < 0 || f < 1 || f > AERO_MAX_F) return 0;
  return carve(nullptr, n, ngraph, AERO_NACC * f).bytes;
}

int agn_eval_sums(int dtype, int n, int f, const void* pred, int pred_ld, const void* y, int y_ld, const void* mean,
                  const void* std, const int32_t* gptr, int ngraph, double* out, void* scratch, void* stream) {
  if (n < 0 || ngraph < 0) return AGN_E_ARG;
  if (dtype != AGN_F32 && dtype != AGN_F64) return AGN_E_DTYPE;
  if (f < 1 || f > AERO_MAX_F || pred_ld < f || y_ld < f) return AGN_E_SHAPE;
  if (n == 0 || ngraph == 0) return 0;
  if (!pred || !y || !mean || !std || !gptr || !out || !scratch) return AGN_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int width = AERO_NACC * f, cap = chunk_cap(n, ngraph);
  const Scratch s = carve(scratch, n, ngraph, width);
  const int rc = plan_chunks(s, n, ngraph, gptr, st);
  if (rc) return rc;
  if (dtype == AGN_F32)
    hipLaunchKernelGGL(eval_chunk_kernel<float>, dim3(cap), dim3(AERO_THREADS), 0, st, n, f, ngraph, (const float*)pred,
                       pred_ld, (const float*)y, y_ld, (const float*)mean, (const float*)std, gptr, s.coff, s.part);
  else
    hipLaunchKernelGGL(eval_chunk_kernel<double>, dim3(cap), dim3(AERO_THREADS), 0, st, n, f, ngraph,
                       (const double*)pred, pred_ld, (const double*)y, y_ld, (const double*)mean, (const double*)std,
                       gptr, s.coff, s.part);
  hipLaunchKernelGGL(finish_kernel, dim3(ngraph), dim3(AERO_THREADS), 0, st, ngraph, width, cap, s.coff, s.part, out);
  return launch_status();
}

size_t agn_aero_forces_temp_bytes(int n, int ngraph) {
  if (n < 0 || ngraph < 0) return 0;
  return carve(nullptr, n, ngraph, AERO_NACC).bytes;
}

int agn_aero_forces(int dtype, int n, int dim, const void* pressure, const void* shear, int shear_ld,
                    const void* normals, int normals_ld, const void* pos, int pos_ld, const double* areas,
                    const int64_t* edge_index, int64_t e, const int32_t* rowptr, const int32_t* perm,
                    double length_scale, double* area_out, const double* center, const int32_t* gptr, int ngraph,
                    double* out, void* scratch, void* stream) {
  if (n < 0 || ngraph < 0 || e < 0) return AGN_E_ARG;
  if (dtype != AGN_F32 && dtype != AGN_F64) return AGN_E_DTYPE;
  if (dim != 2 && dim != 3) return AGN_E_SHAPE;
  if (shear_ld < dim || normals_ld < dim || (pos && pos_ld < dim)) return AGN_E_SHAPE;
  const bool mesh = rowptr != nullptr;
  if (mesh == (areas != nullptr)) return AGN_E_SHAPE;  // areas and mesh both given, or both missing
  if (n == 0 || ngraph == 0) return 0;
  if (!pressure || !shear || !normals || !gptr || !out || !scratch) return AGN_E_ARG;
  if (mesh && (!pos || (e > 0 && (!edge_index || !perm)))) return AGN_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int cap = chunk_cap(n, ngraph);
  const Scratch s = carve(scratch, n, ngraph, AERO_NACC);
  const int rc = plan_chunks(s, n, ngraph, gptr, st);
  if (rc) return rc;
  ForceArgs A;
  A.n = n; A.dim = dim; A.ngraph = ngraph;
  A.shear_ld = shear_ld; A.normals_ld = normals_ld; A.pos_ld = pos_ld;
  A.pressure = pressure; A.shear = shear; A.normals = normals; A.pos = pos;
  A.areas = areas;
  A.edge_index = edge_index; A.e = e; A.rowptr = rowptr; A.perm = perm;
  A.half_scale = 0.5 * length_scale;
  A.area_out = mesh ? area_out : nullptr;
  for (int c = 0; c < 3; ++c) A.center[c] = (center && c < dim) ? center[c] : 0.0;
  A.gptr = gptr; A.coff = s.coff; A.part = s.part;
  if (dtype == AGN_F32) hipLaunchKernelGGL(force_chunk_kernel<float>, dim3(cap), dim3(AERO_THREADS), 0, st, A);
  else hipLaunchKernelGGL(force_chunk_kernel<double>, dim3(cap), dim3(AERO_THREADS), 0, st, A);
  hipLaunchKernelGGL(finish_kernel, dim3(ngraph), dim3(AERO_THREADS), 0, st, ngraph, AERO_NACC, cap, s.coff, s.part,
                     out);
  return launch_status();
}

}  // extern "C"
