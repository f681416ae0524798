// The two-stage fixed-order fp64 reduction of the evaluation kernels (aero.hip: agn_eval_sums,
// agn_aero_forces; surface.hip: agn_surface_forces), written once so that the three entries cut a
// graph into the same chunks and add in the same trees: agn_surface_forces is bitwise
// agn_aero_forces on the cell arrays it emits because both run this code.
//
// Stage 1: one block of AERO_THREADS threads per chunk of AERO_ROWS rows; chunks are laid out from
// each graph's first row (not from row 0 of the batch), so graph g of a batch is cut exactly as it
// is when it is evaluated alone. A block finds its (graph, chunk) by binary search in the exclusive
// scan of the per-graph chunk counts (find_chunk); its threads accumulate in registers and
// column_tree_reduce adds them in a fixed halving tree. Stage 2 (finish_kernel): one block per graph
// adds that graph's chunk partials in ascending chunk order. No atomics, nothing passed between
// workgroups. Include after `#pragma clang fp contract(off)`.
#pragma once
#include "common.hpp"
#include "host.hpp"
#include "aerognn.h"

namespace agn {
namespace red {

constexpr int AERO_ROWS = 2048;   // rows (or elements) per chunk
constexpr int AERO_THREADS = 256;

// the chunk-count prefix `coff` [ngraph + 1] -> (graph, first row, end row) of block b; false past the total.
// Row ranges are clamped to [0, n], so a malformed gptr cannot send a read out of the arrays.
AGN_DEV bool find_chunk(int b, int n, int ngraph, const int32_t* __restrict__ gptr, const int32_t* __restrict__ coff,
                        int* g_out, int* r0_out, int* r1_out) {
  if (b >= coff[ngraph]) return false;
  int lo = 0, hi = ngraph;  // last g with coff[g] <= b (empty graphs share an offset: the last one wins)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (coff[mid] <= b) lo = mid;
    else hi = mid;
  }
  const int g = lo;
  const int a = max(gptr[g], 0), e = min(gptr[g + 1], n);
  const int64_t r0 = (int64_t)a + (int64_t)(b - coff[g]) * AERO_ROWS;
  if (r0 >= e) return false;
  *g_out = g;
  *r0_out = (int)r0;
  *r1_out = (int)min((int64_t)e, r0 + AERO_ROWS);
  return true;
}

// cnt[g] = chunks of graph g
static __global__ void chunk_count_kernel(int n, int ngraph, const int32_t* __restrict__ gptr, int32_t* __restrict__ cnt) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= ngraph) return;
  const int a = max(gptr[g], 0), e = min(gptr[g + 1], n);
  cnt[g] = e > a ? (e - a + AERO_ROWS - 1) / AERO_ROWS : 0;
}

// Adds, per column j, the accumulators of the Q threads t = q * f + j (q < Q) in a halving tree over
// q; on return the threads with q == 0 hold the sums. sh: [NACC][AERO_THREADS] doubles. Each of the
// NACC accumulators goes through the same tree on its own: the result of one does not depend on NACC.
template <int NACC>
AGN_DEV void column_tree_reduce(double (&a)[NACC], double (*sh)[AERO_THREADS], int t, int f, int Q) {
  const int q = t / f;
  const bool live = q < Q;
#pragma unroll
  for (int k = 0; k < NACC; ++k)
    if (live) sh[k][t] = a[k];
  __syncthreads();
  int P = 1;
  while (P < Q) P <<= 1;
  for (int h = P >> 1; h >= 1; h >>= 1) {
    if (live && q < h && q + h < Q) {
#pragma unroll
      for (int k = 0; k < NACC; ++k) sh[k][t] += sh[k][t + h * f];
    }
    __syncthreads();
  }
  if (live && q == 0) {
#pragma unroll
    for (int k = 0; k < NACC; ++k) a[k] = sh[k][t];
  }
}

// stage 2: out[g][o] = sum over the graph's chunks, ascending, of part[chunk][o]; o < width
static __global__ void finish_kernel(int ngraph, int width, int cap, const int32_t* __restrict__ coff,
                                     const double* __restrict__ part, double* __restrict__ out) {
  const int g = blockIdx.x, o = threadIdx.x;
  if (o >= width) return;
  const int c0 = max(coff[g], 0), c1 = min(coff[g + 1], cap);  // cap = chunks the partials hold
  double s = 0.0;
  int c = c0;
  // eight loads in flight, then their adds in ascending chunk order (the order of the plain loop)
  for (; c + 8 <= c1; c += 8) {
    double v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = part[(size_t)(c + i) * width + o];
#pragma unroll
    for (int i = 0; i < 8; ++i) s += v[i];
  }
  for (; c < c1; ++c) s += part[(size_t)c * width + o];
  out[(size_t)g * width + o] = s;
}

static inline size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

static inline int chunk_cap(int n, int ngraph) { return (int)(((int64_t)n + AERO_ROWS - 1) / AERO_ROWS) + ngraph; }

// scratch: [cnt int32 ngraph][coff int32 ngraph + 1][scan scratch][partials double cap * width]
struct Scratch {
  int32_t *cnt, *coff, *scan;
  double* part;
  size_t bytes;
};
static inline Scratch carve(void* base, int n, int ngraph, int width) {
  Scratch s;
  char* p = reinterpret_cast<char*>(base);
  size_t o = 0;
  s.cnt = reinterpret_cast<int32_t*>(p + o);
  o += up16(sizeof(int32_t) * (size_t)ngraph);
  s.coff = reinterpret_cast<int32_t*>(p + o);
  o += up16(sizeof(int32_t) * ((size_t)ngraph + 1));
  s.scan = reinterpret_cast<int32_t*>(p + o);
  o += up16(agn_scan_temp_bytes(ngraph));
  s.part = reinterpret_cast<double*>(p + o);
  o += up16(sizeof(double) * (size_t)chunk_cap(n, ngraph) * width);
  s.bytes = o;
  return s;
}

// per-graph chunk counts and their exclusive scan (coff[ngraph] = the total)
static inline int plan_chunks(const Scratch& s, int n, int ngraph, const int32_t* gptr, hipStream_t st) {
  hipLaunchKernelGGL(chunk_count_kernel, dim3((ngraph + 255) / 256), dim3(256), 0, st, n, ngraph, gptr, s.cnt);
  return agn_exclusive_scan_i32(s.cnt, s.coff, ngraph, s.coff + ngraph, s.scan, st);
}

}  // namespace red
}  // namespace agn
