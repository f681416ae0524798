// 3-D surface evaluation from a face list, on the device: what the reference gets from three VTK
// filters on the host (inference.py:310-320: compute_normals(cell_normals=True),
// compute_cell_sizes(area=True), point_data_to_cell_data) followed by calculate_aero_coefficients_3d
// (utils.py:385-448), and the readers' graph from the same faces (utils.py:75-81, :111-117:
// extract_all_edges + to_undirected).
//
// agn_surface_forces: one pass over the cells, one thread per cell. A thread walks the cell's points
// in connectivity order once: the fan cross products c_i = (p_i - p_0) x (p_{i+1} - p_0) give the
// area (sum of 0.5 |c_i|, vtkCellSizeFilter's fan triangulation) and the normal (sum of c_i,
// normalised: the direction of vtkPolygon::ComputeNormal), and the point fields are averaged with the
// weight 1 / n (vtkPointDataToCellData). All geometry is fp64 from positions widened exactly; every
// operation is one correctly rounded fp64 + - * / or sqrt in the order written (contraction is off for
// the whole file). The force of a cell is the element rule of agn_aero_forces (aero.hip) on the cell
// values rounded to the field dtype, and the per-graph sums run through the chunk layout, the block
// tree and the finishing pass of aero_reduce.hpp with agn_aero_forces' element-to-thread map: the
// sums are bitwise agn_aero_forces on the cell arrays this kernel emits.
//
// agn_face_edges: every cell side as two directed keys u * N + v, radix-sorted, run-flagged, scanned
// and compacted: the coalesced (row, col) order to_undirected returns.
#include "common.hpp"
#include "host.hpp"
#include "aerognn.h"

#pragma clang fp contract(off)

#include "aero_reduce.hpp"

using namespace agn;
using namespace agn::red;

namespace {

constexpr int SURF_MAX_SET = 4;
constexpr int SURF_NACC = 6;  // per set: sum F (3), sum |F| (3)

struct SurfArgs {
  int n, ncell, ngraph, k, nset, pos_ld;
  int64_t nconn;
  const void* pos;
  const int64_t *offsets, *conn;
  const void* field[SURF_MAX_SET];
  int field_ld[SURF_MAX_SET];
  const void *mean, *std;
  const int32_t *cgptr, *coff;
  double *part, *area_out, *normal_out;
  void* cell_out;
};

// P: dtype of pos, T: dtype of the point fields, of mean / std and of cell_out
template <typename P, typename T>
__global__ void __launch_bounds__(AERO_THREADS) surface_chunk_kernel(const SurfArgs A) {
  __shared__ double sh[SURF_NACC][AERO_THREADS];
  int g, r0, r1;
  if (!find_chunk(blockIdx.x, A.ncell, A.ngraph, A.cgptr, A.coff, &g, &r0, &r1)) return;  // block-uniform
  const int t = threadIdx.x, nset = A.nset;
  const P* pos = (const P*)A.pos;
  const bool scale = A.mean != nullptr;
  T mu[4] = {0, 0, 0, 0}, sd[4] = {1, 1, 1, 1};
  if (scale) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      mu[j] = ((const T*)A.mean)[j];
      sd[j] = ((const T*)A.std)[j];
    }
  }
  double a[SURF_MAX_SET][SURF_NACC];
#pragma unroll
  for (int s = 0; s < SURF_MAX_SET; ++s)
#pragma unroll
    for (int k = 0; k < SURF_NACC; ++k) a[s][k] = 0.0;

  for (int c = r0 + t; c < r1; c += AERO_THREADS) {  // agn_aero_forces' element-to-thread map
    // the cell's slice of conn, clamped to the array
    int64_t o0, o1;
    if (A.offsets) {
      o0 = A.offsets[c];
      o1 = A.offsets[c + 1];
    } else {
      o0 = (int64_t)c * A.k;
      o1 = o0 + A.k;
    }
    o0 = min(max(o0, (int64_t)0), A.nconn);
    o1 = min(max(o1, o0), A.nconn);
    const int np = (int)min(o1 - o0, (int64_t)INT32_MAX);
    const double w = 1.0 / (double)np;

    double p0[3] = {0.0, 0.0, 0.0}, dp[3] = {0.0, 0.0, 0.0}, S[3] = {0.0, 0.0, 0.0};
    double area = 0.0;
    double cv[SURF_MAX_SET][4];
#pragma unroll
    for (int s = 0; s < SURF_MAX_SET; ++s)
#pragma unroll
      for (int j = 0; j < 4; ++j) cv[s][j] = 0.0;

    for (int i = 0; i < np; ++i) {
      int64_t v = A.conn[o0 + i];
      v = min(max(v, (int64_t)0), (int64_t)A.n - 1);  // the caller validated the ids; never read outside
      if (pos) {
        double d[3];
#pragma unroll
        for (int x = 0; x < 3; ++x) d[x] = (double)pos[(size_t)v * A.pos_ld + x];
        if (i == 0) {
#pragma unroll
          for (int x = 0; x < 3; ++x) p0[x] = d[x];
        } else {
#pragma unroll
          for (int x = 0; x < 3; ++x) d[x] = d[x] - p0[x];
          if (i >= 2) {  // c_{i-1} = d_{i-1} x d_i: two rounded products and one rounded difference each
            double cr[3];
            cr[0] = dp[1] * d[2] - dp[2] * d[1];
            cr[1] = dp[2] * d[0] - dp[0] * d[2];
            cr[2] = dp[0] * d[1] - dp[1] * d[0];
            area += 0.5 * sqrt(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2]);
#pragma unroll
            for (int x = 0; x < 3; ++x) S[x] += cr[x];
          }
#pragma unroll
          for (int x = 0; x < 3; ++x) dp[x] = d[x];
        }
      }
#pragma unroll
      for (int s = 0; s < SURF_MAX_SET; ++s) {
        if (s < nset) {
          const T* row = (const T*)A.field[s] + (size_t)v * A.field_ld[s];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            T f = row[j];
            if (scale) {
              f = f * sd[j];  // two roundings in the field dtype (inference.py:77-82), never an FMA
              f = f + mu[j];
            }
            cv[s][j] += w * (double)f;
          }
        }
      }
    }

    double nrm[3] = {0.0, 0.0, 0.0};
    const double len = sqrt(S[0] * S[0] + S[1] * S[1] + S[2] * S[2]);
    if (len != 0.0) {
#pragma unroll
      for (int x = 0; x < 3; ++x) nrm[x] = S[x] / len;
    }
    if (A.area_out) A.area_out[c] = area;
    if (A.normal_out) {
#pragma unroll
      for (int x = 0; x < 3; ++x) A.normal_out[(size_t)c * 3 + x] = nrm[x];
    }
    T nT[3];
#pragma unroll
    for (int x = 0; x < 3; ++x) nT[x] = (T)nrm[x];  // VTK stores Normals as float
#pragma unroll
    for (int s = 0; s < SURF_MAX_SET; ++s) {
      if (s < nset) {
        T cell[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) cell[j] = (T)cv[s][j];  // the mean is rounded once, as the filter stores it
        if (A.cell_out) {
          T* o = (T*)A.cell_out + ((size_t)s * A.ncell + c) * 4;
#pragma unroll
          for (int j = 0; j < 4; ++j) o[j] = cell[j];
        }
#pragma unroll
        for (int x = 0; x < 3; ++x) {
          const T pn = cell[0] * nT[x];  // one rounding in the field dtype
          const double F = (double)pn * area - (double)cell[1 + x] * area;
          a[s][x] += F;
          a[s][3 + x] += fabs(F);
        }
      }
    }
  }

  for (int s = 0; s < nset; ++s) {  // block-uniform
    double r[SURF_NACC];
#pragma unroll
    for (int q = 0; q < SURF_MAX_SET; ++q)
      if (q == s) {
#pragma unroll
        for (int k = 0; k < SURF_NACC; ++k) r[k] = a[q][k];
      }
    column_tree_reduce<SURF_NACC>(r, sh, t, 1, AERO_THREADS);
    if (t == 0) {
      double* o = A.part + ((size_t)blockIdx.x * nset + s) * SURF_NACC;
#pragma unroll
      for (int k = 0; k < SURF_NACC; ++k) o[k] = r[k];
    }
    __syncthreads();  // sh is reused by the next set
  }
}

// ---- agn_face_edges
// One thread per cell: side i = (v_i, v_{(i+1) mod n}) fills the key slots 2 (o0 + i) and + 1; a slot
// without a side (n < 2, the second point of a two-point cell) holds `none` = N * N, above every key.
__global__ void face_keys_kernel(int ncell, int k, int64_t nconn, uint64_t nnode, const int64_t* __restrict__ offsets,
                                 const int64_t* __restrict__ conn, uint64_t* __restrict__ keys) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncell) return;
  int64_t o0, o1;
  if (offsets) {
    o0 = offsets[c];
    o1 = offsets[c + 1];
  } else {
    o0 = (int64_t)c * k;
    o1 = o0 + k;
  }
  o0 = min(max(o0, (int64_t)0), nconn);
  o1 = min(max(o1, o0), nconn);
  const int64_t np = o1 - o0;
  const uint64_t none = nnode * nnode;
  const int64_t sides = np >= 3 ? np : (np == 2 ? 1 : 0);
  const uint64_t first = np > 0 ? (uint64_t)conn[o0] : 0;
  uint64_t u = first;
  for (int64_t i = 0; i < np; ++i) {
    const uint64_t v = i + 1 < np ? (uint64_t)conn[o0 + i + 1] : first;
    const bool side = i < sides;
    keys[2 * (o0 + i)] = side ? u * nnode + v : none;
    keys[2 * (o0 + i) + 1] = side ? v * nnode + u : none;
    u = v;
  }
}

// flag[i] = key i is a side's key and differs from its predecessor (the keys are sorted)
__global__ void face_flags_kernel(int m, uint64_t none, const uint64_t* __restrict__ keys, int32_t* __restrict__ flag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const uint64_t key = keys[i];
  flag[i] = (key < none && (i == 0 || key != keys[i - 1])) ? 1 : 0;
}

__global__ void face_emit_kernel(int m, uint64_t nnode, const uint64_t* __restrict__ keys,
                                 const int32_t* __restrict__ flag, const int32_t* __restrict__ at,
                                 int64_t* __restrict__ out, int64_t out_ld) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m || !flag[i]) return;
  const int64_t p = at[i];
  if (p < 0 || p >= out_ld) return;
  const uint64_t key = keys[i];
  out[p] = (int64_t)(key / nnode);
  out[out_ld + p] = (int64_t)(key % nnode);
}

struct EdgeScratch {
  uint64_t *keys, *keys_tmp;
  int32_t *vals, *vals_tmp, *scan;
  void* sort;
  size_t bytes;
};
EdgeScratch carve_edges(void* base, int m) {
  EdgeScratch s;
  char* p = reinterpret_cast<char*>(base);
  size_t o = 0;
  s.keys = reinterpret_cast<uint64_t*>(p + o);
  o += up16(sizeof(uint64_t) * (size_t)m);
  s.keys_tmp = reinterpret_cast<uint64_t*>(p + o);
  o += up16(sizeof(uint64_t) * (size_t)m);
  s.vals = reinterpret_cast<int32_t*>(p + o);  // the sort's payload; afterwards the run flags
  o += up16(sizeof(int32_t) * (size_t)m);
  s.vals_tmp = reinterpret_cast<int32_t*>(p + o);  // afterwards the output positions
  o += up16(sizeof(int32_t) * (size_t)m);
  s.scan = reinterpret_cast<int32_t*>(p + o);
  o += up16(agn_scan_temp_bytes(m));
  s.sort = p + o;
  o += up16(agn_radix_sort_temp_bytes(m));
  s.bytes = o;
  return s;
}

bool float_dtype(int d) { return d == AGN_F32 || d == AGN_F64; }

}  // namespace

extern "C" {

size_t agn_surface_forces_temp_bytes(int ncell, int ngraph, int nset) {
  if (ncell < 0 || ngraph < 0 || nset < 0 || nset > SURF_MAX_SET) return 0;
  return carve(nullptr, ncell, ngraph, SURF_NACC * (nset > 0 ? nset : 1)).bytes;
}

int agn_surface_forces(int pos_dtype, int n, const void* pos, int pos_ld, int ncell, const int64_t* offsets,
                       const int64_t* conn, int64_t nconn, int k, int field_dtype, int nset, const void* const* fields,
                       const int* field_ld, const void* mean, const void* std, const int32_t* cgptr, int ngraph,
                       double* out, double* area_out, double* normal_out, void* cell_out, void* scratch,
                       void* stream) {
  if (n < 0 || ncell < 0 || ngraph < 0 || nconn < 0) return AGN_E_ARG;
  if (!float_dtype(pos_dtype) || !float_dtype(field_dtype)) return AGN_E_DTYPE;
  if (nset < 0 || nset > SURF_MAX_SET || (pos && pos_ld < 3) || (!offsets && k < 0)) return AGN_E_SHAPE;
  if ((mean == nullptr) != (std == nullptr)) return AGN_E_SHAPE;
  if (!offsets && (int64_t)ncell * k > nconn) return AGN_E_SHAPE;
  if (nset > 0) {
    if (!fields || !field_ld) return AGN_E_ARG;
    for (int s = 0; s < nset; ++s) {
      if (!fields[s]) return AGN_E_ARG;
      if (field_ld[s] < 4) return AGN_E_SHAPE;
    }
  }
  if (!pos && (area_out || normal_out)) return AGN_E_ARG;
  if (ncell == 0 || ngraph == 0) return 0;
  if (!cgptr || !scratch || (nconn > 0 && !conn) || (nset > 0 && !out)) return AGN_E_ARG;
  if (nconn > 0 && n == 0) return AGN_E_SHAPE;  // points named, none given
  hipStream_t st = (hipStream_t)stream;
  const int width = SURF_NACC * (nset > 0 ? nset : 1), cap = chunk_cap(ncell, ngraph);
  const Scratch s = carve(scratch, ncell, ngraph, width);
  const int rc = plan_chunks(s, ncell, ngraph, cgptr, st);
  if (rc) return rc;
  SurfArgs A;
  A.n = n; A.ncell = ncell; A.ngraph = ngraph; A.k = k; A.nset = nset; A.pos_ld = pos_ld;
  A.nconn = nconn;
  A.pos = pos; A.offsets = offsets; A.conn = conn;
  for (int i = 0; i < SURF_MAX_SET; ++i) {
    A.field[i] = i < nset ? fields[i] : nullptr;
    A.field_ld[i] = i < nset ? field_ld[i] : 0;
  }
  A.mean = mean; A.std = std;
  A.cgptr = cgptr; A.coff = s.coff;
  A.part = s.part; A.area_out = area_out; A.normal_out = normal_out; A.cell_out = cell_out;
  const dim3 grid(cap), block(AERO_THREADS);
  if (pos_dtype == AGN_F32 && field_dtype == AGN_F32)
    hipLaunchKernelGGL((surface_chunk_kernel<float, float>), grid, block, 0, st, A);
  else if (pos_dtype == AGN_F32)
    hipLaunchKernelGGL((surface_chunk_kernel<float, double>), grid, block, 0, st, A);
  else if (field_dtype == AGN_F32)
    hipLaunchKernelGGL((surface_chunk_kernel<double, float>), grid, block, 0, st, A);
  else
    hipLaunchKernelGGL((surface_chunk_kernel<double, double>), grid, block, 0, st, A);
  if (nset > 0)
    hipLaunchKernelGGL(finish_kernel, dim3(ngraph), dim3(AERO_THREADS), 0, st, ngraph, width, cap, s.coff, s.part, out);
  return launch_status();
}

size_t agn_face_edges_temp_bytes(int64_t nconn) {
  if (nconn < 0 || 2 * nconn > INT32_MAX) return 0;
  return carve_edges(nullptr, (int)(2 * nconn)).bytes;
}

int agn_face_edges(int n, int ncell, const int64_t* offsets, const int64_t* conn, int64_t nconn, int k, int64_t* out,
                   int64_t out_ld, int32_t* ecount, void* scratch, void* stream) {
  if (n < 0 || ncell < 0 || nconn < 0 || !ecount) return AGN_E_ARG;
  if (2 * nconn > INT32_MAX || (!offsets && (k < 0 || (int64_t)ncell * k > nconn))) return AGN_E_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  const int m = (int)(2 * nconn);
  if (ncell == 0 || m == 0 || n == 0) {
    const hipError_t e = hipMemsetAsync(ecount, 0, sizeof(int32_t), st);
    return e == hipSuccess ? launch_status() : (int)e;
  }
  if (!conn || !out || !scratch) return AGN_E_ARG;
  if (out_ld < m) return AGN_E_SHAPE;  // the edge count is not known before the pass: room for every key
  const EdgeScratch s = carve_edges(scratch, m);
  const uint64_t nnode = (uint64_t)n, none = nnode * nnode;
  int bits = 0;
  while (bits < 64 && (none >> bits) != 0) ++bits;
  // slots no cell covers (a malformed offsets array) must not hold stale keys
  hipError_t e = hipMemsetAsync(s.keys, 0xff, sizeof(uint64_t) * (size_t)m, st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(face_keys_kernel, dim3((ncell + 255) / 256), dim3(256), 0, st, ncell, k, nconn, nnode, offsets, conn,
                     s.keys);
  int rc = agn_radix_sort_u64(s.keys, s.vals, m, bits, s.keys_tmp, s.vals_tmp, s.sort, stream);
  if (rc) return rc;
  const dim3 grid((m + 255) / 256);
  hipLaunchKernelGGL(face_flags_kernel, grid, dim3(256), 0, st, m, none, s.keys, s.vals);
  rc = agn_exclusive_scan_i32(s.vals, s.vals_tmp, m, ecount, s.scan, stream);
  if (rc) return rc;
  hipLaunchKernelGGL(face_emit_kernel, grid, dim3(256), 0, st, m, nnode, s.keys, s.vals, s.vals_tmp, out, out_ld);
  return launch_status();
}

}  // extern "C"
