// Row gather / expand / compact-and-sum (gfx950): what lets a transformer encoder run on the samples that HAVE its modality
// (Modal3Classifier(..., present=); IEMOCAP missing-modality training).  Such an encoder has no BatchNorm and no dropout, so all
// samples whose modality is absent share one input (zeros) and one feature f(0):
//
//   mla_rows_gather       inputs:            dst[j] = src[idx[j]] (j < P), then `zero_tail_rows` rows of +0.0 (the one absent input)
//   mla_rows_expand       features:          dst[b] = src[map[b]]  (b < B): a present sample's row, or the zero row's feature f(0)
//   mla_rows_compact_sum  feature gradients: dst[j] = src[idx[j]] (j < P), dst[P] = sum_a src[absent[a]], fp32, in the order of `absent`
//
// Pure bandwidth, plain C++: blockIdx.y is the destination row, so the row's source is uniform over a workgroup; a thread moves
// one unit per turn of a grid-stride loop over the row.  A unit is 16 bytes when every row starts on a 16-byte boundary (both
// bases aligned, the row a whole number of units), else one 4-byte word: rows of 257 floats start at different offsets mod 16 in
// source and destination, so there is no common vector body to peel a scalar tail from.  Every destination row is written exactly
// once; no atomics, no LDS, and the one sum is a serial fp32 chain per element.
//
// The index tables are built on the host.  The host copy is checked (rows_args.h) before anything is launched; the device copy is
// the caller's upload of the same table, and the kernels write zeros for (never read through) an entry that leaves the source.
#include "common.h"
#include "rows_args.h"

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <typename U>
__device__ __forceinline__ void rows_copy_row(const U* __restrict__ src, int64_t s, int64_t src_rows, U* __restrict__ out, size_t units) {
  const bool copy = (uint64_t)s < (uint64_t)src_rows;
  const U* in = src + (copy ? (size_t)s : 0) * units;
  const U zero = {};
  const size_t stride = (size_t)gridDim.x * ROWS_THREADS;
  for (size_t u = (size_t)blockIdx.x * ROWS_THREADS + threadIdx.x; u < units; u += stride) out[u] = copy ? in[u] : zero;
}

// dst row r = src row map[r] for r < n_map, zeros for the rows behind (gather: the zero tail; expand: n_map == gridDim.y)
template <typename U>
__global__ __launch_bounds__(ROWS_THREADS) void rows_move_kernel(const U* __restrict__ src, const int64_t* __restrict__ map, int n_map,
                                                                 int64_t src_rows, U* __restrict__ dst, size_t units) {
  const int r = blockIdx.y;
  rows_copy_row(src, r < n_map ? map[r] : -1, src_rows, dst + (size_t)r * units, units);
}

// dst rows 0..P-1 = src rows idx[.]; dst row P = src[absent[0]] + src[absent[1]] + ... from +0.0, in that order (A == 0: +0.0)
template <typename V>
__global__ __launch_bounds__(ROWS_THREADS) void rows_compact_sum_kernel(const V* __restrict__ src, const int64_t* __restrict__ idx,
                                                                        const int64_t* __restrict__ absent, int P, int A,
                                                                        int64_t src_rows, V* __restrict__ dst, size_t units) {
  const int r = blockIdx.y;
  V* out = dst + (size_t)r * units;
  if (r < P) {
    rows_copy_row(src, idx[r], src_rows, out, units);
    return;
  }
  const size_t stride = (size_t)gridDim.x * ROWS_THREADS;
  for (size_t u = (size_t)blockIdx.x * ROWS_THREADS + threadIdx.x; u < units; u += stride) {
    V acc = {};
    for (int a = 0; a < A; ++a) {
      const int64_t s = absent[a];
      if ((uint64_t)s < (uint64_t)src_rows) acc += src[(size_t)s * units + u];
    }
    out[u] = acc;
  }
}

// ---- entry points: rows_args.h checks everything and plans the launch --------------------------------------------------
static dim3 rows_grid(const RowsPlan& p) { return dim3(p.blocks_x, (unsigned)p.rows); }

static void rows_move_launch(const RowsPlan& p, const void* src, const int64_t* map, int n_map, int64_t src_rows, void* dst, hipStream_t st) {
  if (p.vec16)
    hipLaunchKernelGGL(rows_move_kernel<u32x4>, rows_grid(p), dim3(ROWS_THREADS), 0, st, (const u32x4*)src, map, n_map, src_rows, (u32x4*)dst,
                       p.units);
  else
    hipLaunchKernelGGL(rows_move_kernel<uint32_t>, rows_grid(p), dim3(ROWS_THREADS), 0, st, (const uint32_t*)src, map, n_map, src_rows,
                       (uint32_t*)dst, p.units);
}

extern "C" int mla_rows_gather(const void* src, const int64_t* idx, const int64_t* idx_host, void* dst, int B, int P, size_t row_elems,
                               int elem_bytes, int zero_tail_rows, void* stream) {
  RowsPlan p;
  if (int rc = rows_gather_plan(src, idx, idx_host, dst, B, P, row_elems, elem_bytes, zero_tail_rows, &p)) return rc;
  rows_move_launch(p, src, idx, P, B, dst, (hipStream_t)stream);
  MLA_CHECK_LAUNCH("rows_move_kernel (gather)");
  return MLA_OK;
}

extern "C" int mla_rows_expand(const void* src, const int64_t* map, const int64_t* map_host, void* dst, int B, int src_rows,
                               size_t row_elems, int elem_bytes, void* stream) {
  RowsPlan p;
  if (int rc = rows_expand_plan(src, map, map_host, dst, B, src_rows, row_elems, elem_bytes, &p)) return rc;
  rows_move_launch(p, src, map, B, src_rows, dst, (hipStream_t)stream);
  MLA_CHECK_LAUNCH("rows_move_kernel (expand)");
  return MLA_OK;
}

extern "C" int mla_rows_compact_sum(const float* src, const int64_t* idx, const int64_t* idx_host, const int64_t* absent_idx,
                                    const int64_t* absent_host, float* dst, int B, int P, int A, size_t row_elems, void* stream) {
  RowsPlan p;
  if (int rc = rows_compact_sum_plan(src, idx, idx_host, absent_idx, absent_host, dst, B, P, A, row_elems, &p)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (p.vec16)
    hipLaunchKernelGGL(rows_compact_sum_kernel<f32x4>, rows_grid(p), dim3(ROWS_THREADS), 0, st, (const f32x4*)src, idx, absent_idx, P, A,
                       (int64_t)B, (f32x4*)dst, p.units);
  else
    hipLaunchKernelGGL(rows_compact_sum_kernel<float>, rows_grid(p), dim3(ROWS_THREADS), 0, st, src, idx, absent_idx, P, A, (int64_t)B, dst,
                       p.units);
  MLA_CHECK_LAUNCH("rows_compact_sum_kernel");
  return MLA_OK;
}
