// Fused multi-head attention, forward and backward, exact fp32 on v_mfma_f32_32x32x2_f32: the kernels of attention_kernels.h (outline,
// remainder rows, masking: see there) with the arithmetic AttF32 below, and the three stand-alone vector kernels for sequences shorter
// than one tile, which both arithmetics use.
//
// What AttF32 supplies: a walked tile is its fp32 image in LDS, 32 rows of ATT_LD floats, read along rows as b128 fragments
// (mma_tile_own) and element-wise down a column (mma_tileT_acc); an owned row block is 32 fp32 registers per lane, which feed the MFMA
// and the vector code of the remainder loop alike; the accumulator registers of a score tile are the B operand of the next product
// as they stand.
#include "attention_kernels.h"

namespace {

struct AttF32 {
  typedef float Elem;
  static constexpr int TILE = 32 * ATT_LD;       // [32][ATT_LD]
  typedef float Own[32];                         // lane (row = lane % 32, half) holds X[row][half * 32 + kk]

  // (with remainder rows the forward needs ~190 VGPRs: at three 4-wave workgroups per CU it spilled 11 registers whose reloads wait `vmcnt(0)`
  //  inside the key loop; two workgroups per CU and no scratch is faster -- n = 257: 170 -> see DESIGN 8)
  static constexpr int fwd_wgs(int W, int TAIL) { return (W >= 3 && !TAIL) ? 3 : 2; }
  static constexpr int dq_wgs(int) { return 2; }
  static constexpr int dkv_wgs(int) { return 2; }

  template <int NT>
  static __device__ __forceinline__ void tile_store(float* tile, const TileRegs<NT>& t, int tid) { t.store(tile, tid); }

  // 32 registers of the B operand of a wave-owned row block
  static __device__ __forceinline__ void own_load(Own& x, const float* base, size_t row_stride, int row, int n, int half) {
    if (row < n) {
      const f32x4* p = reinterpret_cast<const f32x4*>(base + (size_t)row * row_stride + half * 32);
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const f32x4 v = p[c];
        x[4 * c + 0] = v[0]; x[4 * c + 1] = v[1]; x[4 * c + 2] = v[2]; x[4 * c + 3] = v[3];
      }
    } else {
#pragma unroll
      for (int c = 0; c < 32; ++c) x[c] = 0.f;
    }
  }
  // the fp32 view of an owned block: the registers it is held in
  static __device__ __forceinline__ void own_rows_f32(float (&x)[32], const Own& own, const float*, size_t, int, int, int) {
#pragma unroll
    for (int c = 0; c < 32; ++c) x[c] = own[c];
  }
  // The dQ kernel's owned rows and dsum = rowsum(dO * O): the rows are loaded up front, the sum is formed where the kernel asks for it.
  static __device__ __forceinline__ float dq_own_load(Own& q, Own& d_o, const float* Qb, size_t rs, const float* dOb, const float*, size_t os,
                                                      int row, int n, int half) {
    own_load(q, Qb, rs, row, n, half);
    own_load(d_o, dOb, os, row, n, half);
    return 0.f;
  }
  static __device__ __forceinline__ float dq_dsum(float dsum, const Own& d_o, const float* Ob, size_t os, int row, int n, int half) {
    Own oreg;
    own_load(oreg, Ob, os, row, n, half);
#pragma unroll
    for (int c = 0; c < 32; ++c) dsum += d_o[c] * oreg[c];
    return dsum + __shfl_xor(dsum, 32, 64);
  }
  static __device__ __forceinline__ int tile_lane(int lane) { return lane; }

  // acc(32 x 32) = T(32 rows from LDS, b128 fragments) x own^T : acc[e] <-> (tile row acc_row(e, half), own row lane % 32)
  static __device__ __forceinline__ void mma_tile_own(f32x16& acc, const float* tile, const Own& own, int lane) {
    const float* rowp = tile + (lane & 31) * ATT_LD + (lane >> 5) * 32;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(rowp + 4 * c);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], own[4 * c + j], acc, 0, 0, 0);
    }
  }

  // out^T(64 x 32, two 32-row blocks) += tile^T (64 x 32 tile rows) x w(32 tile rows x 32 own rows, accumulator layout)
  static __device__ __forceinline__ void mma_tileT_acc(f32x16& o0, f32x16& o1, const float* tile, const float (&w)[16], int lane) {
    const int half = lane >> 5, c = lane & 31;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const float* rowp = tile + acc_row(e, half) * ATT_LD;
      o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(rowp[c], w[e], o0, 0, 0, 0);
      o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(rowp[32 + c], w[e], o1, 0, 0, 0);
    }
  }

  // dot product of a wave-owned row (lane: row lane % 32, dims half * 32 ..) with one broadcast row of 64 floats
  static __device__ __forceinline__ float own_dot(const float (&own)[32], const float* __restrict__ row, int half) {
    const f32x4* p = reinterpret_cast<const f32x4*>(row + half * 32);
    float d = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const f32x4 v = p[c];
      d += own[4 * c] * v[0] + own[4 * c + 1] * v[1] + own[4 * c + 2] * v[2] + own[4 * c + 3] * v[3];
    }
    return d + __shfl_xor(d, 32, 64);
  }

  // ---- vector code for OWNED remainder rows, run by one wave per tile on the tiles in LDS: a dot product per tile row (lane = row,
  // half = dim half), softmax statistics by wave reductions, weighted row sums with the weights broadcast by v_readlane.
  static __device__ __forceinline__ float vec_row_dot(const float* __restrict__ tile, const float* __restrict__ vec, int lane) {
    const f32x4* rowp = reinterpret_cast<const f32x4*>(tile + (lane & 31) * ATT_LD + (lane >> 5) * 32);
    const f32x4* vp = reinterpret_cast<const f32x4*>(vec + (lane >> 5) * 32);
    float d = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const f32x4 a = rowp[c], v = vp[c];
      d += a[0] * v[0] + a[1] * v[1] + a[2] * v[2] + a[3] * v[3];
    }
    return d + __shfl_xor(d, 32, 64);
  }
  // sum_{r < 32} w_r * tile[r][lane], w_r = the value lane r holds
  static __device__ __forceinline__ float vec_wsum(const float* __restrict__ tile, float w, int lane) {
    float a = 0.f;
#pragma unroll
    for (int r = 0; r < 32; ++r)
      a += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(w), r)) * tile[r * ATT_LD + lane];
    return a;
  }
};

// ---------------------------------------------------------------------------------------------------------------------
// Stand-alone vector kernels for sequences shorter than one tile (n <= ATT_TAIL_MAX, nm == 0; otherwise the vector wave of the
// tiled kernels owns the remainder rows): one 4-wave workgroup per (b, h, row), plain vector code over the whole sequence (scores of one
// row against n keys / queries in LDS, lanes over the other axis for the dot products, lanes over the 64 features for the
// weighted sums).  ~n x 128 FMAs per wave: microseconds for the whole grid.
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float row_dot(const float* __restrict__ row, const float* __restrict__ vec_lds) {
  const f32x4* p = reinterpret_cast<const f32x4*>(row);
  float d = 0.f;
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    const f32x4 v = p[c];
    d += v[0] * vec_lds[4 * c] + v[1] * vec_lds[4 * c + 1] + v[2] * vec_lds[4 * c + 2] + v[3] * vec_lds[4 * c + 3];
  }
  return d;
}

// weighted sum over the sequence: out[d] = sum_j w[j] * rows[j][d]; ATT_TW waves = ATT_TW row lanes x 64 features, 16 independent
// loads per lane in flight per round (a tail kernel is a few dependent memory round trips, nothing else), lanes combined through
// LDS in a fixed order.  Result in threads 0..63 (feature = tid).
#define ATT_TW 4
__device__ __forceinline__ float tail_wsum(const float* __restrict__ rows, size_t row_stride, const float* __restrict__ w, int n,
                                            float (*red)[ATT_HD]) {
  const int d = threadIdx.x & 63, rl = threadIdx.x >> 6;
  float acc = 0.f;
  for (int j0 = rl; j0 < n; j0 += 16 * ATT_TW) {
    float v[16], ww[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int j = j0 + k * ATT_TW;
      v[k] = j < n ? rows[(size_t)j * row_stride + d] : 0.f;
      ww[k] = j < n ? w[j] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) acc += ww[k] * v[k];
  }
  red[rl][d] = acc;
  __syncthreads();
  float t = 0.f;
  if (threadIdx.x < 64)
#pragma unroll
    for (int k = 0; k < ATT_TW; ++k) t += red[k][d];
  return t;
}
__device__ __forceinline__ float block_reduce_max(float v, float* redw) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) redw[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = redw[0];
#pragma unroll
  for (int k = 1; k < ATT_TW; ++k) t = fmaxf(t, redw[k]);
  __syncthreads();
  return t;
}
__device__ __forceinline__ float block_reduce_sum(float v, float* redw) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) redw[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = 0.f;
#pragma unroll
  for (int k = 0; k < ATT_TW; ++k) t += redw[k];
  __syncthreads();
  return t;
}

__global__ __launch_bounds__(64 * ATT_TW) void attn_fwd_tail_kernel(const AttGeom g, float* __restrict__ O, float* __restrict__ LSE) {
  __shared__ float qs[ATT_HD], ps[ATT_TAIL_N], red[ATT_TW][ATT_HD], red4[ATT_TW];
  const int tid = threadIdx.x, bh = blockIdx.x, b = bh / g.H, h = bh - b * g.H, q = g.nm + blockIdx.y;
  const size_t rs = (size_t)3 * g.H * ATT_HD, os = (size_t)g.H * ATT_HD;
  const float* Kb = g.qkv + qkv_off(g, b, 0, 1, h);
  const float* Vb = g.qkv + qkv_off(g, b, 0, 2, h);
  if (tid < ATT_HD) qs[tid] = g.qkv[qkv_off(g, b, q, 0, h) + tid];
  __syncthreads();
  float mx = -INFINITY;
  for (int j = tid; j < g.n; j += 64 * ATT_TW) {
    const float sj = key_state(g, b, j, g.n) == 0.f ? row_dot(Kb + (size_t)j * rs, qs) * g.scale : -1e7f;
    ps[j] = sj;
    mx = fmaxf(mx, sj);
  }
  mx = block_reduce_max(mx, red4);
  float sum = 0.f;
  for (int j = tid; j < g.n; j += 64 * ATT_TW) {
    const float pj = fast_exp(ps[j] - mx);
    ps[j] = pj;
    sum += pj;
  }
  sum = block_reduce_sum(sum, red4);
  const float acc = tail_wsum(Vb, rs, ps, g.n, red);
  if (tid < ATT_HD) O[((size_t)b * g.n + q) * os + (size_t)h * ATT_HD + tid] = acc / sum;
  if (tid == 0) LSE[(size_t)bh * g.n + q] = mx + logf(sum);
}

__global__ __launch_bounds__(64 * ATT_TW) void attn_bwd_dq_tail_kernel(const AttGeom g, const float* __restrict__ dO, const float* __restrict__ O,
                                                                const float* __restrict__ LSE, float* __restrict__ Dvec,
                                                                float* __restrict__ dqkv) {
  __shared__ float qs[ATT_HD], dos[ATT_HD], dss[ATT_TAIL_N], red[ATT_TW][ATT_HD], red4[ATT_TW];
  const int tid = threadIdx.x, bh = blockIdx.x, b = bh / g.H, h = bh - b * g.H, q = g.nm + blockIdx.y;
  const size_t rs = (size_t)3 * g.H * ATT_HD, os = (size_t)g.H * ATT_HD;
  const float* Kb = g.qkv + qkv_off(g, b, 0, 1, h);
  const float* Vb = g.qkv + qkv_off(g, b, 0, 2, h);
  const size_t orow = ((size_t)b * g.n + q) * os + (size_t)h * ATT_HD;
  float prod = 0.f;
  if (tid < ATT_HD) {
    const float dov = dO[orow + tid];
    qs[tid] = g.qkv[qkv_off(g, b, q, 0, h) + tid];
    dos[tid] = dov;
    prod = dov * O[orow + tid];
  }
  const float dsum = block_reduce_sum(prod, red4);              // also orders the LDS writes above before the reads below
  const float lse = LSE[(size_t)bh * g.n + q];
  for (int j = tid; j < g.n; j += 64 * ATT_TW) {
    const float sj = row_dot(Kb + (size_t)j * rs, qs), dpj = row_dot(Vb + (size_t)j * rs, dos);
    const float pj = key_state(g, b, j, g.n) == 0.f ? fast_exp(sj * g.scale - lse) : 0.f;
    dss[j] = pj * (dpj - dsum) * g.scale;
  }
  __syncthreads();
  const float acc = tail_wsum(Kb, rs, dss, g.n, red);
  if (tid < ATT_HD) dqkv[qkv_off(g, b, q, 0, h) + tid] = acc;
  if (tid == 0) Dvec[(size_t)bh * g.n + q] = dsum;
}

__global__ __launch_bounds__(64 * ATT_TW) void attn_bwd_dkv_tail_kernel(const AttGeom g, const float* __restrict__ dO, const float* __restrict__ LSE,
                                                                 const float* __restrict__ Dvec, float* __restrict__ dqkv) {
  __shared__ float ks[ATT_HD], vs[ATT_HD], ps[ATT_TAIL_N], dss[ATT_TAIL_N], red[ATT_TW][ATT_HD];
  const int tid = threadIdx.x, bh = blockIdx.x, b = bh / g.H, h = bh - b * g.H, key = g.nm + blockIdx.y;
  const size_t rs = (size_t)3 * g.H * ATT_HD, os = (size_t)g.H * ATT_HD;
  const float* Qb = g.qkv + qkv_off(g, b, 0, 0, h);
  const float* dOb = dO + (size_t)b * g.n * os + (size_t)h * ATT_HD;
  if (tid < ATT_HD) {
    ks[tid] = g.qkv[qkv_off(g, b, key, 1, h) + tid];
    vs[tid] = g.qkv[qkv_off(g, b, key, 2, h) + tid];
  }
  const bool attend = key_state(g, b, key, g.n) == 0.f;
  __syncthreads();
  for (int qq = tid; qq < g.n; qq += 64 * ATT_TW) {
    const float sq = row_dot(Qb + (size_t)qq * rs, ks), dpq = row_dot(dOb + (size_t)qq * os, vs);
    const float pq = attend ? fast_exp(sq * g.scale - LSE[(size_t)bh * g.n + qq]) : 0.f;
    ps[qq] = pq;
    dss[qq] = pq * (dpq - Dvec[(size_t)bh * g.n + qq]) * g.scale;
  }
  __syncthreads();
  const float dv = tail_wsum(dOb, os, ps, g.n, red);
  __syncthreads();
  const float dk = tail_wsum(Qb, rs, dss, g.n, red);
  if (tid < ATT_HD) {
    dqkv[qkv_off(g, b, key, 1, h) + tid] = dk;
    dqkv[qkv_off(g, b, key, 2, h) + tid] = dv;
  }
}

}  // namespace

extern "C" int mla_attention_fwd(const float* qkv, const float* pad_mask, float* o, float* lse, int B, int H, int n, int hd,
                                 void* stream) {
  MLA_REQUIRE(qkv && o && lse, "mla_attention_fwd: null pointer");
  if (int rc = check_att("mla_attention_fwd", B, H, n, hd)) return rc;
  const int nm = att_main_rows(n);
  AttGeom g{qkv, pad_mask, B, H, n, nm, 1.0f / sqrtf((float)hd)};
  hipStream_t st = (hipStream_t)stream;
  if (nm > 0) {
    att_launch(nm, n, B * H, [&](auto w, auto tail, dim3 grid, dim3 block) {
      attn_fwd_kernel<AttF32, decltype(w)::value, decltype(tail)::value><<<grid, block, 0, st>>>(g, o, lse);
    });
  } else {                // n <= ATT_TAIL_MAX: nothing for the MFMA kernels, the stand-alone vector kernel does all rows
    attn_fwd_tail_kernel<<<dim3(B * H, n - nm), 64 * ATT_TW, 0, st>>>(g, o, lse);
  }
  MLA_CHECK_LAUNCH("attn_fwd_kernel");
  return MLA_OK;
}

extern "C" int mla_attention_bwd(const float* d_o, const float* qkv, const float* o, const float* lse, const float* pad_mask,
                                 float* dqkv, float* dvec, int B, int H, int n, int hd, void* stream) {
  MLA_REQUIRE(d_o && qkv && o && lse && dqkv && dvec, "mla_attention_bwd: null pointer");
  if (int rc = check_att("mla_attention_bwd", B, H, n, hd)) return rc;
  const int nm = att_main_rows(n);
  AttGeom g{qkv, pad_mask, B, H, n, nm, 1.0f / sqrtf((float)hd)};
  hipStream_t st = (hipStream_t)stream;
  // order matters: the query-side kernel writes dvec (rowsum(d_o * o)) for every row before the key-side kernel reads it
  if (nm > 0) {
    att_launch(nm, n, B * H, [&](auto w, auto tail, dim3 grid, dim3 block) {
      attn_bwd_dq_kernel<AttF32, decltype(w)::value, decltype(tail)::value><<<grid, block, 0, st>>>(g, d_o, o, lse, dvec, dqkv);
    });
    MLA_CHECK_LAUNCH("attn_bwd_dq_kernel");
    att_launch(nm, n, B * H, [&](auto w, auto tail, dim3 grid, dim3 block) {
      attn_bwd_dkv_kernel<AttF32, decltype(w)::value, decltype(tail)::value><<<grid, block, 0, st>>>(g, d_o, lse, dvec, dqkv);
    });
  } else {                // n <= ATT_TAIL_MAX: the stand-alone vector kernels do all rows
    const dim3 tail(B * H, n - nm);
    attn_bwd_dq_tail_kernel<<<tail, 64 * ATT_TW, 0, st>>>(g, d_o, o, lse, dvec, dqkv);
    MLA_CHECK_LAUNCH("attn_bwd_dq_tail_kernel");
    attn_bwd_dkv_tail_kernel<<<tail, 64 * ATT_TW, 0, st>>>(g, d_o, lse, dvec, dqkv);
  }
  MLA_CHECK_LAUNCH("attn_bwd_dkv_kernel");
  return MLA_OK;
}
