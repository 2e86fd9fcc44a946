// Fused multi-head attention, forward and backward, on the split-bf16 arithmetic: fp32 in, out and accumulate, every product formed
// on v_mfma_f32_32x32x16_bf16 from the exact three-way bf16 split of BOTH operands (split_pair) and the six kept products of
// TERM_A / TERM_B (split_mma<6>) -- the arithmetic of the Linear and convolution kernels (split_common.h).
//
// The kernels are those of attention_kernels.h (outline, remainder rows, masking, softmax, host selection: see there) with the
// arithmetic AttSplit below.  The three tail-only kernels (n <= 3) hold no MFMA: the entry points here call mla_attention_fwd /
// mla_attention_bwd for those lengths.
//
// What AttSplit supplies is how the five products are fed:
//   * OWN rows (Q in the forward, Q and dO in the dQ kernel, K and V in the dK / dV kernel) are split once into register fragments,
//     [4 k-steps][3 planes] x 4 VGPRs: lane (row r, half h) holds dims 16 s + 8 h .. + 7 of its row in k-step s.
//   * WALKED tiles (32 rows x 64 dims) are split once when staged: global fp32 -> registers -> three bf16 planes in LDS, 128-byte
//     rows, double-buffered.  A tile is read two ways from the one image:
//       along rows (ds_read_b128), as the A operand of S^T = K Q^T, dP^T = V dO^T (S = Q K^T, dP = dO V^T on the key side), and
//       transposed (ds_read_b64_tr_b16), as the A operand of O^T += V^T P^T, dQ^T += K^T dS^T, dV^T += dO^T P, dK^T += Q^T dS.
//     Image: 16-byte chunk ch (0..7) of row `row` lies at 128 row + 16 (ch ^ x(row)), x(row) = ((row >> 1) & 1) << 2 | (row >> 2) & 3
//     -- the XOR image of the programming guide for 32x32x16 operands, restated for 128-byte rows.  Row reads: the 16 lanes of a
//     ds_read_b128 group take rows of which the 8 even (odd) ones have 8 different (row >> 1) & 7, hence 8 different chunks, and the
//     row parity picks the 128-byte half of the 64 banks.  Transposed reads: a 32-lane half takes 4 consecutive rows x 64 bytes; row
//     parity picks the bank half, bit 1 of the row flips chunk bit 2.  Both are conflict-free.
//   * P and dS are split in registers from the accumulator: the score tile is produced transposed to the rows the wave owns, its
//     column (the owned row) on the lane and its 32 rows in the 16 registers, so registers 8 s .. 8 s + 7 are the B fragment of
//     k-step s of the next product.  Element j of lane half h is tile row 16 s + 8 (j >> 2) + 4 h + (j & 3); the transposed reads
//     of the other operand fetch exactly those rows (two reads of 4 rows per fragment), so both operands enumerate k alike.
//
// Remainder rows read the staged tiles as vector code.  The tiles are bf16 planes now; that code rebuilds x = (hi + mid) + lo, which
// is exact, instead of keeping an fp32 image beside the planes: 2 x 2 tiles x 12 KiB of planes is 48 KiB per workgroup, an fp32 image
// of each would add 34 KiB and push two 4-wave workgroups (the budget of every kernel here) past the CU's 160 KiB.
//
// Budget: two 4-wave workgroups per CU, i.e. 256 registers per wave and <= 59 KiB of LDS per workgroup.  The forward (221 - 253 VGPRs)
// and the dQ kernel hold no scratch (dQ<3, 3>: 36 bytes per lane); the dK / dV kernel does not fit and says so at AttSplit::dkv_wgs.
// Measured against the fp32-MFMA kernels (forward + backward, same process): 0.68 - 0.72 of their time at n = 256, 288, 512, 0.95 at
// n = 257, 1.16 at n = 258 (profiles/r07_attention_math.txt).
#include "attention_kernels.h"
#include "split_common.h"

#define ATS_PLANE 1024                 // dwords of one bf16 plane of a tile: 32 rows x 128 B
#define ATS_TILE (3 * ATS_PLANE)       // hi | mid | lo

namespace {

// dword offset of 16-byte chunk ch of row `row` inside a plane
__device__ __forceinline__ int ats_off(int row, int ch) { return row * 32 + ((ch ^ ((((row >> 1) & 1) << 2) | ((row >> 2) & 3))) << 2); }

__device__ __forceinline__ float bf_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf_hi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }

struct AttSplit {
  typedef unsigned Elem;
  static constexpr int TILE = ATS_TILE;          // [3 planes][32][32 dwords]
  typedef u32x4 Own[4][3];                       // [k-step][plane]

  static constexpr int fwd_wgs(int, int) { return 2; }
  // (two-wave workgroups: one wave per SIMD, see dkv_wgs)
  static constexpr int dq_wgs(int W) { return W == 2 ? 1 : 2; }
  // dK / dV registers: two own operands (96) + four accumulators (64) + S, dP / P, dS (32) + the split P / dS planes and the transposed
  // fragments (24) + the staged tile leave no slack in 256.  W >= 3 is compiled for two workgroups per CU and spills 48 ... 168 bytes
  // per lane (addresses and a few staging values; two workgroups with them measured 10 ... 15 % faster on the backward than one
  // workgroup per CU without); a two-wave workgroup takes one wave per SIMD and 512 registers, which still seats two per CU.
  static constexpr int dkv_wgs(int W) { return W == 2 ? 1 : 2; }

  // registers -> the three planes of a tile image (split once per staged tile)
  template <int NT>
  static __device__ __forceinline__ void tile_store(unsigned* tile, const TileRegs<NT>& t, int tid) {
#pragma unroll
    for (int p = 0; p < TileRegs<NT>::P; ++p) {
      const int idx = tid + NT * p, row = (idx >> 4) & 31, c4 = idx & 15;
      if (idx < 512) split_store4(tile + ats_off(row, c4 >> 1) + 2 * (c4 & 1), ATS_PLANE, t.r[p]);
    }
  }

  // fp32 copy of a wave-owned row block in fragment order: x[8 s + j] = X[row][16 s + 8 half + j] (zero beyond n).
  // The vector code of the remainder keys after the tile loop wants the own rows in fp32 again.  It reloads them: rebuilding them
  // from the fragments is loop-invariant, so the compiler formed all 32 / 64 values BEFORE the loop and spilled them across it.
  static __device__ __forceinline__ void own_rows_f32(float (&x)[32], const Own&, const float* base, size_t row_stride, int row, int n, int half) {
    if (row < n) {
      const float* p = base + (size_t)row * row_stride + half * 8;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const f32x4 v0 = *reinterpret_cast<const f32x4*>(p + 16 * s), v1 = *reinterpret_cast<const f32x4*>(p + 16 * s + 4);
        x[8 * s + 0] = v0[0]; x[8 * s + 1] = v0[1]; x[8 * s + 2] = v0[2]; x[8 * s + 3] = v0[3];
        x[8 * s + 4] = v1[0]; x[8 * s + 5] = v1[1]; x[8 * s + 6] = v1[2]; x[8 * s + 7] = v1[3];
      }
    } else {
#pragma unroll
      for (int c = 0; c < 32; ++c) x[c] = 0.f;
    }
  }
  static __device__ __forceinline__ void own_split(Own& f, const float (&x)[32]) {
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        unsigned hi, mid, lo;
        split_pair<true>(x[8 * s + 2 * i], x[8 * s + 2 * i + 1], hi, mid, lo);
        f[s][0][i] = hi;
        f[s][1][i] = mid;
        f[s][2][i] = lo;
      }
  }
  static __device__ __forceinline__ void own_load(Own& f, const float* base, size_t row_stride, int row, int n, int half) {
    float x[32];
    own_rows_f32(x, f, base, row_stride, row, n, half);
    own_split(f, x);
  }
  // The dQ kernel's owned rows and dsum = rowsum(dO * O).  dsum is formed here, before the splits, while the fp32 dO rows are live
  // (once they are fragments it would take a second fp32 copy of them beside the fragments); dq_dsum has nothing left to do.
  static __device__ __forceinline__ float dq_own_load(Own& q, Own& d_o, const float* Qb, size_t rs, const float* dOb, const float* Ob, size_t os,
                                                      int row, int n, int half) {
    float dsum = 0.f;
    float x[32], oreg[32];
    own_rows_f32(x, d_o, dOb, os, row, n, half);
    own_rows_f32(oreg, d_o, Ob, os, row, n, half);
#pragma unroll
    for (int c = 0; c < 32; ++c) dsum += x[c] * oreg[c];
    own_split(d_o, x);
    own_rows_f32(x, q, Qb, rs, row, n, half);
    own_split(q, x);
    return dsum + __shfl_xor(dsum, 32, 64);
  }
  static __device__ __forceinline__ float dq_dsum(float dsum, const Own&, const float*, size_t, int, int, int) { return dsum; }
  // dK / dV kernel, once per tile: the lane plus an opaque 0, so that the fragment addresses are formed per tile, not held across the loop
  static __device__ __forceinline__ int tile_lane(int lane) {
    int pz = 0;
    asm volatile("" : "+v"(pz));
    return lane + pz;
  }

  // acc(32 x 32) += T(32 tile rows, row reads) x own^T : acc[e] <-> (tile row acc_row(e, half), own row lane % 32)
  static __device__ __forceinline__ void mma_tile_own(f32x16& acc, const unsigned* tile, const Own& own, int lane) {
    const int r = lane & 31, h = lane >> 5;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const unsigned* p = tile + ats_off(r, 2 * s + h);
      u32x4 a[3];
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) a[pl] = *reinterpret_cast<const u32x4*>(p + pl * ATS_PLANE);
      split_mma<6>(a, own[s], acc);
    }
  }

  // out^T(64 x 32, two 32-row blocks) += tile^T (transposed reads) x w (32 tile rows x 32 own rows, accumulator layout, split here).
  // Every lane of the wave must be active (ds_read_b64_tr_b16).
  static __device__ __forceinline__ void mma_tileT_acc(f32x16& o0, f32x16& o1, const unsigned* tile, const float (&w)[16], int lane) {
    const int h = lane >> 5, g16 = (lane >> 4) & 1, q = (lane & 15) >> 2, p = lane & 3;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      u32x4 b[3];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        unsigned hi, mid, lo;
        split_pair<true>(w[8 * s + 2 * i], w[8 * s + 2 * i + 1], hi, mid, lo);
        b[0][i] = hi;
        b[1][i] = mid;
        b[2][i] = lo;
      }
#pragma unroll
      for (int blk = 0; blk < 2; ++blk) {
        u32x4 a[3];
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
          // elements 4 jj .. 4 jj + 3 of the fragment: tile rows 16 s + 8 jj + 4 h + (0..3), column = dim 32 blk + lane % 32
          const unsigned* ap = tile + ats_off(16 * s + 8 * jj + 4 * h + q, 4 * blk + 2 * g16 + (p >> 1)) + 2 * (p & 1);
#pragma unroll
          for (int pl = 0; pl < 3; ++pl) {
            const u32x2 t = __builtin_bit_cast(u32x2, lds_tr(ap + pl * ATS_PLANE));
            a[pl][2 * jj] = t[0];
            a[pl][2 * jj + 1] = t[1];
          }
        }
        split_mma<6>(a, b, blk ? o1 : o0);
      }
    }
  }

  // dot product of a wave-owned row (fragment order, see own_rows_f32) with one broadcast row of 64 floats
  static __device__ __forceinline__ float own_dot(const float (&own)[32], const float* __restrict__ row, int half) {
    float d = 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const f32x4 v0 = *reinterpret_cast<const f32x4*>(row + 16 * s + 8 * half), v1 = *reinterpret_cast<const f32x4*>(row + 16 * s + 8 * half + 4);
      d += own[8 * s] * v0[0] + own[8 * s + 1] * v0[1] + own[8 * s + 2] * v0[2] + own[8 * s + 3] * v0[3];
      d += own[8 * s + 4] * v1[0] + own[8 * s + 5] * v1[1] + own[8 * s + 6] * v1[2] + own[8 * s + 7] * v1[3];
    }
    return d + __shfl_xor(d, 32, 64);
  }

  // ---- vector code for OWNED remainder rows on the plane images (AttF32: vec_row_dot, vec_wsum); values rebuilt exactly
  static __device__ __forceinline__ float vec_row_dot(const unsigned* __restrict__ tile, const float* __restrict__ vec, int lane) {
    const int r = lane & 31, half = lane >> 5;
    float d = 0.f;
#pragma unroll 1
    for (int c = 0; c < 4; ++c) {
      const unsigned* p = tile + ats_off(r, 4 * half + c);
      const u32x4 a = *reinterpret_cast<const u32x4*>(p), m = *reinterpret_cast<const u32x4*>(p + ATS_PLANE),
                  l = *reinterpret_cast<const u32x4*>(p + 2 * ATS_PLANE);
      const float* vp = vec + half * 32 + 8 * c;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        d += ((bf_lo(a[i]) + bf_lo(m[i])) + bf_lo(l[i])) * vp[2 * i];
        d += ((bf_hi(a[i]) + bf_hi(m[i])) + bf_hi(l[i])) * vp[2 * i + 1];
      }
    }
    return d + __shfl_xor(d, 32, 64);
  }
  // sum_{r < 32} w_r * tile[r][lane], w_r = the value lane r holds.  Lane (k = lane % 32, rh = lane / 32) takes dword k -- dims 2 k and
  // 2 k + 1 -- of rows 16 rh .. 16 rh + 15 (half the reads of a lane per dim, both halves of every dword used, packed fp32 math); the
  // two row halves are added across lanes and lane L fetches dim L from lane L / 2.  8 rows per trip of a rolled loop: fully unrolled,
  // the scheduler puts every read in flight, which pushes the own-row fragments of the MFMA code out to scratch around each vector step.
  static __device__ __forceinline__ float vec_wsum(const unsigned* __restrict__ tile, float w, int lane) {
    const int k = lane & 31, rh = lane >> 5;
    f32x2 a = {0.f, 0.f};
#pragma unroll 1
    for (int i0 = 0; i0 < 16; i0 += 8)
#pragma unroll
      for (int i = i0; i < i0 + 8; ++i) {
        const unsigned* p = tile + 512 * rh + ats_off(i, k >> 2) + (k & 3);        // row 16 rh + i: x(row) does not depend on rh
        const unsigned hi = p[0], mid = p[ATS_PLANE], lo = p[2 * ATS_PLANE];
        const float w0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(w), i));
        const float w1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(w), 16 + i));
        const float wr = rh ? w1 : w0;
        const f32x2 x = (f32x2{bf_lo(hi), bf_hi(hi)} + f32x2{bf_lo(mid), bf_hi(mid)}) + f32x2{bf_lo(lo), bf_hi(lo)};
        a += x * f32x2{wr, wr};
      }
    a[0] += __shfl_xor(a[0], 32, 64);
    a[1] += __shfl_xor(a[1], 32, 64);
    const float b0 = __shfl(a[0], lane >> 1, 64), b1 = __shfl(a[1], lane >> 1, 64);
    return (lane & 1) ? b1 : b0;
  }
};

}  // namespace

extern "C" int mla_attention_fwd_split(const float* qkv, const float* pad_mask, float* o, float* lse, int B, int H, int n, int hd,
                                       void* stream) {
  MLA_REQUIRE(qkv && o && lse, "mla_attention_fwd_split: null pointer");
  if (int rc = check_att("mla_attention_fwd_split", B, H, n, hd)) return rc;
  const int nm = att_main_rows(n);
  if (nm == 0) return mla_attention_fwd(qkv, pad_mask, o, lse, B, H, n, hd, stream);   // n <= ATT_TAIL_MAX: vector kernels, no product on an MFMA
  AttGeom g{qkv, pad_mask, B, H, n, nm, 1.0f / sqrtf((float)hd)};
  hipStream_t st = (hipStream_t)stream;
  att_launch(nm, n, B * H, [&](auto w, auto tail, dim3 grid, dim3 block) {
    attn_fwd_kernel<AttSplit, decltype(w)::value, decltype(tail)::value><<<grid, block, 0, st>>>(g, o, lse);
  });
  MLA_CHECK_LAUNCH("attn_fwd_kernel<AttSplit>");
  return MLA_OK;
}

extern "C" int mla_attention_bwd_split(const float* d_o, const float* qkv, const float* o, const float* lse, const float* pad_mask,
                                       float* dqkv, float* dvec, int B, int H, int n, int hd, void* stream) {
  MLA_REQUIRE(d_o && qkv && o && lse && dqkv && dvec, "mla_attention_bwd_split: null pointer");
  if (int rc = check_att("mla_attention_bwd_split", B, H, n, hd)) return rc;
  const int nm = att_main_rows(n);
  if (nm == 0) return mla_attention_bwd(d_o, qkv, o, lse, pad_mask, dqkv, dvec, B, H, n, hd, stream);
  AttGeom g{qkv, pad_mask, B, H, n, nm, 1.0f / sqrtf((float)hd)};
  hipStream_t st = (hipStream_t)stream;
  // order matters: the query-side kernel writes dvec (rowsum(d_o * o)) for every row before the key-side kernel reads it
  att_launch(nm, n, B * H, [&](auto w, auto tail, dim3 grid, dim3 block) {
    attn_bwd_dq_kernel<AttSplit, decltype(w)::value, decltype(tail)::value><<<grid, block, 0, st>>>(g, d_o, o, lse, dvec, dqkv);
  });
  MLA_CHECK_LAUNCH("attn_bwd_dq_kernel<AttSplit>");
  att_launch(nm, n, B * H, [&](auto w, auto tail, dim3 grid, dim3 block) {
    attn_bwd_dkv_kernel<AttSplit, decltype(w)::value, decltype(tail)::value><<<grid, block, 0, st>>>(g, d_o, lse, dvec, dqkv);
  });
  MLA_CHECK_LAUNCH("attn_bwd_dkv_kernel<AttSplit>");
  return MLA_OK;
}
