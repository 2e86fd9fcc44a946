// Fused multi-head attention, forward and backward, on the split-bf16 arithmetic: fp32 in, out and accumulate, every product formed
// on v_mfma_f32_32x32x16_bf16 from the exact three-way bf16 split of BOTH operands (split_pair) and the six kept products of
// TERM_A / TERM_B (split_mma<6>) -- the arithmetic of the Linear and convolution kernels (split_common.h).
//
//   reference: Attention.forward, models/m3ae.py:102-125 (and timm's Attention inside cav_mae.py:93); see attention.hip.
//
// The outline is attention.hip's, kernel for kernel: head dim 64, qkv (B, n, 3, H, 64) read in place, online softmax forward, a
// backward of two kernels that recompute P from the saved log-sum-exp (dQ owns query rows and writes dvec, dK / dV own key rows), no
// atomics.  Scale, the mask rule, fast_exp, the softmax statistics, 1 / l and m + logf(l) are that file's; so are the remainder-row
// scheme (n = 32 m + r, r <= 3), the (W, TAIL) instantiations and their host selection (attention_common.h).  The three tail-only
// kernels (n <= 3) hold no MFMA: the entry points here call mla_attention_fwd / mla_attention_bwd for those lengths.
//
// What differs is how the five products are fed:
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
// and the dQ kernel hold no scratch (dQ<3, 3>: 36 bytes per lane); the dK / dV kernel does not fit and says so where it is declared.
// Measured against the fp32-MFMA kernels (forward + backward, same process): 0.68 - 0.72 of their time at n = 256, 288, 512, 0.95 at
// n = 257, 1.16 at n = 258 (profiles/r07_attention_math.txt).
#include "attention_common.h"
#include "split_common.h"

#define ATS_PLANE 1024                 // dwords of one bf16 plane of a tile: 32 rows x 128 B
#define ATS_TILE (3 * ATS_PLANE)       // hi | mid | lo

namespace {

// dword offset of 16-byte chunk ch of row `row` inside a plane
__device__ __forceinline__ int ats_off(int row, int ch) { return row * 32 + ((ch ^ ((((row >> 1) & 1) << 2) | ((row >> 2) & 3))) << 2); }

__device__ __forceinline__ float bf_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf_hi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }

typedef u32x4 OwnFrag[4][3];           // [k-step][plane]

// fp32 copy of a wave-owned row block in fragment order: x[8 s + j] = X[row][16 s + 8 half + j] (zero beyond n)
__device__ __forceinline__ void own_rows_load_k(float (&x)[32], const float* base, size_t row_stride, int row, int n, int half) {
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
__device__ __forceinline__ void own_split(OwnFrag& f, const float (&x)[32]) {
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
// (The vector code of the remainder keys after the tile loop wants the own rows in fp32 again.  It reloads them: rebuilding them
//  from the fragments is loop-invariant, so the compiler formed all 32 / 64 values BEFORE the loop and spilled them across it.)

// registers -> the three planes of a tile image (split once per staged tile)
template <int NT>
__device__ __forceinline__ void split_tile_store(unsigned* tile, const TileRegs<NT>& t, int tid) {
#pragma unroll
  for (int p = 0; p < TileRegs<NT>::P; ++p) {
    const int idx = tid + NT * p, row = (idx >> 4) & 31, c4 = idx & 15;
    if (idx < 512) split_store4(tile + ats_off(row, c4 >> 1) + 2 * (c4 & 1), ATS_PLANE, t.r[p]);
  }
}

// acc(32 x 32) += T(32 tile rows, row reads) x own^T : acc[e] <-> (tile row acc_row(e, half), own row lane % 32)
__device__ __forceinline__ void mma_tile_own(f32x16& acc, const unsigned* tile, const OwnFrag& own, int lane) {
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
__device__ __forceinline__ void mma_tileT_acc(f32x16& o0, f32x16& o1, const unsigned* tile, const float (&w)[16], int lane) {
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

// dot product of a wave-owned row (fragment order, see own_rows_load_k) with one broadcast row of 64 floats
__device__ __forceinline__ float own_dot(const float (&own)[32], const float* __restrict__ row, int half) {
  float d = 0.f;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const f32x4 v0 = *reinterpret_cast<const f32x4*>(row + 16 * s + 8 * half), v1 = *reinterpret_cast<const f32x4*>(row + 16 * s + 8 * half + 4);
    d += own[8 * s] * v0[0] + own[8 * s + 1] * v0[1] + own[8 * s + 2] * v0[2] + own[8 * s + 3] * v0[3];
    d += own[8 * s + 4] * v1[0] + own[8 * s + 5] * v1[1] + own[8 * s + 6] * v1[2] + own[8 * s + 7] * v1[3];
  }
  return d + __shfl_xor(d, 32, 64);
}

// ---- vector code for OWNED remainder rows on the plane images (attention.hip: vec_row_dot, vec_wsum); values rebuilt exactly
__device__ __forceinline__ float vec_row_dot(const unsigned* __restrict__ tile, const float* __restrict__ vec, int lane) {
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
__device__ __forceinline__ float vec_wsum(const unsigned* __restrict__ tile, float w, int lane) {
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

// ---------------------------------------------------------------------------------------------------------------------
// forward: workgroup = 32 W queries of one (b, h); loop over key tiles of 32.  o (B, n, H*64), lse (B, H, n).
// ---------------------------------------------------------------------------------------------------------------------
template <int W, int TAIL>
__global__ __launch_bounds__(64 * W, 2) void attn_fwd_split_kernel(const AttGeom g, float* __restrict__ O, float* __restrict__ LSE) {
  constexpr int TMAX = TAIL > 0 ? TAIL : 1;
  __shared__ __attribute__((aligned(16))) unsigned smem[2 * 2 * ATS_TILE + 2 * 32];
  unsigned* Ks = smem;                      // [2][3 planes][32][32 dwords]
  unsigned* Vs = smem + 2 * ATS_TILE;
  float* Kst = reinterpret_cast<float*>(smem + 4 * ATS_TILE);    // [2][32] key states
  __shared__ __attribute__((aligned(16))) float tailK[ATT_TAIL_MAX][ATT_HD], tailV[ATT_TAIL_MAX][ATT_HD];   // the remainder keys [nm, n), fp32
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5;
  const int bh = blockIdx.y, b = bh / g.H, h = bh - b * g.H;
  const int q = blockIdx.x * (32 * W) + wave * 32 + (lane & 31);
  const bool vec = TAIL && blockIdx.x == 0;       // workgroup 0 also owns the remainder queries (attention.hip: attn_fwd_kernel)
  const bool wave_active = blockIdx.x * (32 * W) + wave * 32 < g.nm;
  __shared__ __attribute__((aligned(16))) float vecQ[ATT_TAIL_MAX][ATT_HD];
  __shared__ float vred[W][ATT_TAIL_MAX][ATT_HD + 2], tailSt[ATT_TAIL_MAX];
  const int nt = g.n - g.nm;
  float vm[TMAX], vl[TMAX], vo[TMAX];
#pragma unroll
  for (int t = 0; t < TMAX; ++t) { vm[t] = -INFINITY; vl[t] = 0.f; vo[t] = 0.f; }
  const size_t rs = (size_t)3 * g.H * ATT_HD;                  // token stride inside qkv
  const float* Qb = g.qkv + qkv_off(g, b, 0, 0, h);
  const float* Kb = g.qkv + qkv_off(g, b, 0, 1, h);
  const float* Vb = g.qkv + qkv_off(g, b, 0, 2, h);

  OwnFrag qf;
  {
    float qreg[32];
    own_rows_load_k(qreg, Qb, rs, q, g.nm, half);
    own_split(qf, qreg);
  }
  if (vec && wave == 0)
    for (int t = 0; t < nt; ++t) vecQ[t][lane] = Qb[(size_t)(g.nm + t) * rs + lane];
  if (tid < nt) tailSt[tid] = key_state(g, b, g.nm + tid, g.n);
  f32x16 o0, o1;
  zero_acc(o0);
  zero_acc(o1);
  float m_i = -INFINITY, l_i = 0.f;

  const int ntiles = (g.nm + 31) / 32;
  TileRegs<64 * W> kr, vr;
  kr.load(Kb, rs, 0, g.nm, tid);
  vr.load(Vb, rs, 0, g.nm, tid);
  split_tile_store(Ks, kr, tid);
  split_tile_store(Vs, vr, tid);
  if (tid < 32) Kst[tid] = key_state(g, b, tid, g.nm);
  for (int i = tid; i < (g.n - g.nm) * ATT_HD; i += 64 * W) {
    tailK[i >> 6][i & 63] = Kb[(size_t)(g.nm + (i >> 6)) * rs + (i & 63)];
    tailV[i >> 6][i & 63] = Vb[(size_t)(g.nm + (i >> 6)) * rs + (i & 63)];
  }
  __syncthreads();
  for (int jt = 0; jt < ntiles; ++jt) {
    const int cur = jt & 1, nxt = cur ^ 1;
    const bool more = jt + 1 < ntiles;
    float kst_next = 0.f;
    if (more) {
      kr.load(Kb, rs, (jt + 1) * 32, g.nm, tid);
      vr.load(Vb, rs, (jt + 1) * 32, g.nm, tid);
      if (tid < 32) kst_next = key_state(g, b, (jt + 1) * 32 + tid, g.nm);    // pad-mask load issued here, consumed after the tile's work
    }
    const unsigned* kt = Ks + cur * ATS_TILE;
    const unsigned* vt = Vs + cur * ATS_TILE;
    if (vec && jt % W == wave) {
      const float st = Kst[cur * 32 + (lane & 31)];
#pragma unroll
      for (int t = 0; t < TMAX; ++t)
        if (t < nt) {
          float sv = vec_row_dot(kt, vecQ[t], lane);
          sv = st == 0.f ? sv * g.scale : (st == 1.f ? -1e7f : -INFINITY);
          const float m_new = fmaxf(vm[t], wave_max(sv));
          const float alpha = fast_exp(vm[t] - m_new), pv = fast_exp(sv - m_new);
          vl[t] = vl[t] * alpha + wave_sum(half == 0 ? pv : 0.f);
          vm[t] = m_new;
          vo[t] = vo[t] * alpha + vec_wsum(vt, pv, lane);
        }
    }
    if (wave_active) {
      f32x16 s;
      zero_acc(s);
      mma_tile_own(s, kt, qf, lane);                            // S^T = K Q^T: s[e] <-> (key acc_row(e, half), query lane)
      float p[16];
      float mt = -INFINITY;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const float st = Kst[cur * 32 + acc_row(e, half)];
        p[e] = st == 0.f ? s[e] * g.scale : (st == 1.f ? -1e7f : -INFINITY);
        mt = fmaxf(mt, p[e]);
      }
      mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
      const float m_new = fmaxf(m_i, mt);
      const float alpha = fast_exp(m_i - m_new);                     // first tile: exp(-inf) = 0
      float lt = 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        p[e] = fast_exp(p[e] - m_new);
        lt += p[e];
      }
      lt += __shfl_xor(lt, 32, 64);
      l_i = l_i * alpha + lt;
      m_i = m_new;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        o0[e] *= alpha;
        o1[e] *= alpha;
      }
      mma_tileT_acc(o0, o1, vt, p, lane);                       // O^T += V^T P^T
    }
    if (more) {
      split_tile_store(Ks + nxt * ATS_TILE, kr, tid);
      split_tile_store(Vs + nxt * ATS_TILE, vr, tid);
      if (tid < 32) Kst[nxt * 32 + tid] = kst_next;
    }
    __syncthreads();
  }
  if (vec) {        // remainder queries: wave 0 adds the remainder keys to its partial, all partials are merged, wave 0 writes the rows
#pragma unroll
    for (int t = 0; t < TMAX; ++t)
      if (t < nt) {
        if (wave == 0)
          for (int j = g.nm; j < g.n; ++j) {
            const float dot = wave_sum(vecQ[t][lane] * tailK[j - g.nm][lane]);
            const float sj = tailSt[j - g.nm] == 0.f ? dot * g.scale : -1e7f;
            const float m_new = fmaxf(vm[t], sj);
            const float alpha = fast_exp(vm[t] - m_new), pj = fast_exp(sj - m_new);
            vl[t] = vl[t] * alpha + pj;
            vm[t] = m_new;
            vo[t] = vo[t] * alpha + pj * tailV[j - g.nm][lane];
          }
        vred[wave][t][lane] = vo[t];
        if (lane == 0) {
          vred[wave][t][ATT_HD] = vm[t];
          vred[wave][t][ATT_HD + 1] = vl[t];
        }
      }
    __syncthreads();
    if (wave == 0)
#pragma unroll
      for (int t = 0; t < TMAX; ++t)
        if (t < nt) {
          float m = -INFINITY;
#pragma unroll
          for (int w = 0; w < W; ++w) m = fmaxf(m, vred[w][t][ATT_HD]);
          float l = 0.f, o = 0.f;
#pragma unroll
          for (int w = 0; w < W; ++w) {
            const float sc = fast_exp(vred[w][t][ATT_HD] - m);          // a wave that saw no tile: exp(-inf) = 0
            l += vred[w][t][ATT_HD + 1] * sc;
            o += vred[w][t][lane] * sc;
          }
          O[((size_t)b * g.n + g.nm + t) * (g.H * ATT_HD) + (size_t)h * ATT_HD + lane] = o / l;
          if (lane == 0) LSE[(size_t)bh * g.n + g.nm + t] = m + logf(l);
        }
    __syncthreads();
  }
  if (!wave_active) return;
  if (nt > 0) {                                                  // remainder keys (e.g. the 257th token): vector code
    float qreg[32];
    own_rows_load_k(qreg, Qb, rs, q, g.nm, half);
    for (int j = g.nm; j < g.n; ++j) {
      const float sj = tailSt[j - g.nm] == 0.f ? own_dot(qreg, tailK[j - g.nm], half) * g.scale : -1e7f;
      const float m_new = fmaxf(m_i, sj);
      const float alpha = fast_exp(m_i - m_new), pj = fast_exp(sj - m_new);
      l_i = l_i * alpha + pj;
      m_i = m_new;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        o0[e] *= alpha;
        o1[e] *= alpha;
      }
      own_axpy(o0, o1, tailV[j - g.nm], pj, half);
    }
  }
  // all waves have passed the last barrier: the K/V buffers are free, reuse them as per-wave staging
  float* stage = reinterpret_cast<float*>(smem) + wave * 32 * ATT_LD;
  store_ownT(stage, o0, o1, O + (size_t)b * g.n * (g.H * ATT_HD) + (size_t)h * ATT_HD, (size_t)g.H * ATT_HD,
             blockIdx.x * (32 * W) + wave * 32, g.nm, lane, 1.0f / l_i);
  if (half == 0 && q < g.nm) LSE[(size_t)bh * g.n + q] = m_i + logf(l_i);
}

// ---------------------------------------------------------------------------------------------------------------------
// backward, query side: recomputes P^T from LSE, writes dQ and Dvec[b, h, q] = sum_d dO * O (consumed by the key-side kernel).
// ---------------------------------------------------------------------------------------------------------------------
// (two-wave workgroups: one wave per SIMD, see attn_bwd_dkv_split_kernel)
template <int W, int TAIL>
__global__ __launch_bounds__(64 * W, W == 2 ? 1 : 2) void attn_bwd_dq_split_kernel(const AttGeom g, const float* __restrict__ dO, const float* __restrict__ O,
                                                                 const float* __restrict__ LSE, float* __restrict__ Dvec,
                                                                 float* __restrict__ dqkv) {
  constexpr int TMAX = TAIL > 0 ? TAIL : 1;
  __shared__ __attribute__((aligned(16))) unsigned smem[2 * 2 * ATS_TILE + 2 * 32];
  unsigned* Ks = smem;
  unsigned* Vs = smem + 2 * ATS_TILE;
  float* Kst = reinterpret_cast<float*>(smem + 4 * ATS_TILE);
  __shared__ __attribute__((aligned(16))) float tailK[ATT_TAIL_MAX][ATT_HD], tailV[ATT_TAIL_MAX][ATT_HD];   // the remainder keys [nm, n), fp32
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5;
  const int bh = blockIdx.y, b = bh / g.H, h = bh - b * g.H;
  const int q0 = blockIdx.x * (32 * W) + wave * 32, q = q0 + (lane & 31);
  const bool vec = TAIL && blockIdx.x == 0;                   // this workgroup also owns the remainder queries [nm, n)
  const bool wave_active = q0 < g.nm;
  __shared__ __attribute__((aligned(16))) float vecQ[ATT_TAIL_MAX][ATT_HD], vecD[ATT_TAIL_MAX][ATT_HD];
  __shared__ float vred[W][ATT_TAIL_MAX][ATT_HD], tailSt[ATT_TAIL_MAX];
  const int nt = g.n - g.nm;
  float vlse[TMAX], vD[TMAX], vdq[TMAX];
#pragma unroll
  for (int t = 0; t < TMAX; ++t) { vlse[t] = INFINITY; vD[t] = 0.f; vdq[t] = 0.f; }
  const size_t rs = (size_t)3 * g.H * ATT_HD, os = (size_t)g.H * ATT_HD;
  const float* Qb = g.qkv + qkv_off(g, b, 0, 0, h);
  const float* Kb = g.qkv + qkv_off(g, b, 0, 1, h);
  const float* Vb = g.qkv + qkv_off(g, b, 0, 2, h);
  const float* dOb = dO + (size_t)b * g.n * os + (size_t)h * ATT_HD;
  const float* Ob = O + (size_t)b * g.n * os + (size_t)h * ATT_HD;

  OwnFrag qf, dof;
  float dsum = 0.f;
  {
    float x[32], oreg[32];
    own_rows_load_k(x, dOb, os, q, g.nm, half);
    own_rows_load_k(oreg, Ob, os, q, g.nm, half);
#pragma unroll
    for (int c = 0; c < 32; ++c) dsum += x[c] * oreg[c];
    own_split(dof, x);
    own_rows_load_k(x, Qb, rs, q, g.nm, half);
    own_split(qf, x);
  }
  dsum += __shfl_xor(dsum, 32, 64);
  if (tid < nt) tailSt[tid] = key_state(g, b, g.nm + tid, g.n);
  if (vec)
#pragma unroll
    for (int t = 0; t < TMAX; ++t)
      if (t < nt) {
        const float dv = dOb[(size_t)(g.nm + t) * os + lane];
        if (wave == 0) {
          vecQ[t][lane] = Qb[(size_t)(g.nm + t) * rs + lane];
          vecD[t][lane] = dv;
        }
        vD[t] = wave_sum(dv * Ob[(size_t)(g.nm + t) * os + lane]);
        vlse[t] = LSE[(size_t)bh * g.n + g.nm + t];
      }
  const float lse = q < g.nm ? LSE[(size_t)bh * g.n + q] : INFINITY;   // rows beyond nm: p = exp(s - inf) = 0
  if (half == 0 && q < g.nm) Dvec[(size_t)bh * g.n + q] = dsum;
  f32x16 dq0, dq1;
  zero_acc(dq0);
  zero_acc(dq1);

  const int ntiles = (g.nm + 31) / 32;
  TileRegs<64 * W> kr, vr;
  kr.load(Kb, rs, 0, g.nm, tid);
  vr.load(Vb, rs, 0, g.nm, tid);
  split_tile_store(Ks, kr, tid);
  split_tile_store(Vs, vr, tid);
  if (tid < 32) Kst[tid] = key_state(g, b, tid, g.nm);
  for (int i = tid; i < (g.n - g.nm) * ATT_HD; i += 64 * W) {
    tailK[i >> 6][i & 63] = Kb[(size_t)(g.nm + (i >> 6)) * rs + (i & 63)];
    tailV[i >> 6][i & 63] = Vb[(size_t)(g.nm + (i >> 6)) * rs + (i & 63)];
  }
  __syncthreads();
  for (int jt = 0; jt < ntiles; ++jt) {
    const int cur = jt & 1, nxt = cur ^ 1;
    const bool more = jt + 1 < ntiles;
    float kst_next = 0.f;
    if (more) {
      kr.load(Kb, rs, (jt + 1) * 32, g.nm, tid);
      vr.load(Vb, rs, (jt + 1) * 32, g.nm, tid);
      if (tid < 32) kst_next = key_state(g, b, (jt + 1) * 32 + tid, g.nm);
    }
    const unsigned* kt = Ks + cur * ATS_TILE;
    const unsigned* vt = Vs + cur * ATS_TILE;
    if (vec && jt % W == wave) {
      const bool att = Kst[cur * 32 + (lane & 31)] == 0.f;
#pragma unroll
      for (int t = 0; t < TMAX; ++t)
        if (t < nt) {
          const float sv = vec_row_dot(kt, vecQ[t], lane), dpv = vec_row_dot(vt, vecD[t], lane);
          const float pv = att ? fast_exp(sv * g.scale - vlse[t]) : 0.f;
          vdq[t] += vec_wsum(kt, pv * (dpv - vD[t]) * g.scale, lane);
        }
    }
    if (wave_active) {
      f32x16 s, dp;
      zero_acc(s);
      zero_acc(dp);
      mma_tile_own(s, kt, qf, lane);                            // S^T  = K Q^T
      mma_tile_own(dp, vt, dof, lane);                          // dP^T = V dO^T
      float ds[16];
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const float st = Kst[cur * 32 + acc_row(e, half)];
        const float pe = st == 0.f ? fast_exp(s[e] * g.scale - lse) : 0.f;   // padded keys: exp(-1e7 - lse) == 0 exactly
        ds[e] = pe * (dp[e] - dsum) * g.scale;
      }
      mma_tileT_acc(dq0, dq1, kt, ds, lane);                    // dQ^T += K^T dS^T
    }
    if (more) {
      split_tile_store(Ks + nxt * ATS_TILE, kr, tid);
      split_tile_store(Vs + nxt * ATS_TILE, vr, tid);
      if (tid < 32) Kst[nxt * 32 + tid] = kst_next;
    }
    __syncthreads();
  }
  if (vec) {        // remainder queries: wave 0 adds the remainder keys, the waves' partial dQ rows are summed, wave 0 writes
#pragma unroll
    for (int t = 0; t < TMAX; ++t)
      if (t < nt) {
        if (wave == 0)
          for (int j = g.nm; j < g.n; ++j) {
            const float sj = wave_sum(vecQ[t][lane] * tailK[j - g.nm][lane]), dpj = wave_sum(vecD[t][lane] * tailV[j - g.nm][lane]);
            const float pj = tailSt[j - g.nm] == 0.f ? fast_exp(sj * g.scale - vlse[t]) : 0.f;
            vdq[t] += pj * (dpj - vD[t]) * g.scale * tailK[j - g.nm][lane];
          }
        vred[wave][t][lane] = vdq[t];
      }
    __syncthreads();
    if (wave == 0)
#pragma unroll
      for (int t = 0; t < TMAX; ++t)
        if (t < nt) {
          float a = 0.f;
#pragma unroll
          for (int w = 0; w < W; ++w) a += vred[w][t][lane];
          dqkv[qkv_off(g, b, g.nm + t, 0, h) + lane] = a;
          if (lane == 0) Dvec[(size_t)bh * g.n + g.nm + t] = vD[t];
        }
    __syncthreads();
  }
  if (!wave_active) return;
  if (nt > 0) {                                                  // remainder keys: vector code
    float qreg[32], doreg[32];
    own_rows_load_k(qreg, Qb, rs, q, g.nm, half);
    own_rows_load_k(doreg, dOb, os, q, g.nm, half);
    for (int j = g.nm; j < g.n; ++j) {
      const float sj = own_dot(qreg, tailK[j - g.nm], half), dpj = own_dot(doreg, tailV[j - g.nm], half);
      const float pj = tailSt[j - g.nm] == 0.f ? fast_exp(sj * g.scale - lse) : 0.f;
      own_axpy(dq0, dq1, tailK[j - g.nm], pj * (dpj - dsum) * g.scale, half);
    }
  }
  float* stage = reinterpret_cast<float*>(smem) + wave * 32 * ATT_LD;
  store_ownT(stage, dq0, dq1, dqkv + qkv_off(g, b, 0, 0, h), rs, q0, g.nm, lane, 1.0f);
}

// ---------------------------------------------------------------------------------------------------------------------
// backward, key side: workgroup = 32 W keys; loop over query tiles of 32 (Q, dO, LSE, Dvec through LDS).  Writes dK, dV.
// ---------------------------------------------------------------------------------------------------------------------
// Registers: two own operands (96) + four accumulators (64) + S, dP / P, dS (32) + the split P / dS planes and the transposed
// fragments (24) + the staged tile leave no slack in 256.  W >= 3 is compiled for two workgroups per CU and spills 48 ... 168 bytes
// per lane (addresses and a few staging values; two workgroups with them measured 10 ... 15 % faster on the backward than one
// workgroup per CU without); a two-wave workgroup takes one wave per SIMD and 512 registers, which still seats two per CU.
template <int W, int TAIL>
__global__ __launch_bounds__(64 * W, W == 2 ? 1 : 2) void attn_bwd_dkv_split_kernel(const AttGeom g, const float* __restrict__ dO, const float* __restrict__ LSE,
                                                                  const float* __restrict__ Dvec, float* __restrict__ dqkv) {
  constexpr int TMAX = TAIL > 0 ? TAIL : 1;
  __shared__ __attribute__((aligned(16))) unsigned smem[2 * 2 * ATS_TILE + 2 * 64];
  unsigned* Qs = smem;
  unsigned* dOs = smem + 2 * ATS_TILE;
  float* Rs = reinterpret_cast<float*>(smem + 4 * ATS_TILE);      // [2][64]: lse (32) | Dvec (32) of the query tile
  __shared__ __attribute__((aligned(16))) float tailQ[ATT_TAIL_MAX][ATT_HD], tailD[ATT_TAIL_MAX][ATT_HD];   // remainder queries: Q, dO rows, fp32
  __shared__ float tailS[ATT_TAIL_MAX][2];                                                                  // their lse, rowsum(dO * O)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5;
  const int bh = blockIdx.y, b = bh / g.H, h = bh - b * g.H;
  const int k0 = blockIdx.x * (32 * W) + wave * 32, key = k0 + (lane & 31);
  const bool vec = TAIL && blockIdx.x == 0;                   // this workgroup also owns the remainder keys [nm, n)
  const bool wave_active = k0 < g.nm;
  __shared__ __attribute__((aligned(16))) float vecK[ATT_TAIL_MAX][ATT_HD], vecV[ATT_TAIL_MAX][ATT_HD];
  __shared__ float vred[W][ATT_TAIL_MAX][2][ATT_HD];
  const int nt = g.n - g.nm;
  float vdk[TMAX], vdv[TMAX];
  bool vatt[TMAX];
#pragma unroll
  for (int t = 0; t < TMAX; ++t) { vdk[t] = 0.f; vdv[t] = 0.f; vatt[t] = false; }
  const size_t rs = (size_t)3 * g.H * ATT_HD, os = (size_t)g.H * ATT_HD;
  const float* Qb = g.qkv + qkv_off(g, b, 0, 0, h);
  const float* Kb = g.qkv + qkv_off(g, b, 0, 1, h);
  const float* Vb = g.qkv + qkv_off(g, b, 0, 2, h);
  const float* dOb = dO + (size_t)b * g.n * os + (size_t)h * ATT_HD;

  OwnFrag kf, vf;
  {
    float x[32];
    own_rows_load_k(x, Kb, rs, key, g.nm, half);
    own_split(kf, x);
    own_rows_load_k(x, Vb, rs, key, g.nm, half);
    own_split(vf, x);
  }
  if (vec)
#pragma unroll
    for (int t = 0; t < TMAX; ++t)
      if (t < nt) {
        if (wave == 0) {
          vecK[t][lane] = Kb[(size_t)(g.nm + t) * rs + lane];
          vecV[t][lane] = Vb[(size_t)(g.nm + t) * rs + lane];
        }
        vatt[t] = key_state(g, b, g.nm + t, g.n) == 0.f;
      }
  const bool attend = key_state(g, b, key, g.nm) == 0.f;               // padded / missing keys: P == 0, so dK = dV = 0
  f32x16 dk0, dk1, dv0, dv1;
  zero_acc(dk0);
  zero_acc(dk1);
  zero_acc(dv0);
  zero_acc(dv1);

  const int ntiles = (g.nm + 31) / 32;
  auto row_stat = [&](int t0) -> float {                        // lse (tid < 32) / rowsum(dO * O) (tid 32..63) of query t0 + tid % 32
    float v = tid < 32 ? INFINITY : 0.f;                         // queries beyond nm: lse = +inf -> p = 0
    if (tid < 64) {
      const int qq = t0 + (tid & 31);
      if (qq < g.nm) v = tid < 32 ? LSE[(size_t)bh * g.n + qq] : Dvec[(size_t)bh * g.n + qq];
    }
    return v;
  };
  TileRegs<64 * W> qr, dr;
  qr.load(Qb, rs, 0, g.nm, tid);
  dr.load(dOb, os, 0, g.nm, tid);
  split_tile_store(Qs, qr, tid);
  split_tile_store(dOs, dr, tid);
  if (tid < 64) Rs[tid] = row_stat(0);
  for (int i = tid; i < (g.n - g.nm) * ATT_HD; i += 64 * W) {
    tailQ[i >> 6][i & 63] = Qb[(size_t)(g.nm + (i >> 6)) * rs + (i & 63)];
    tailD[i >> 6][i & 63] = dOb[(size_t)(g.nm + (i >> 6)) * os + (i & 63)];
  }
  if (tid < 2 * (g.n - g.nm)) tailS[tid >> 1][tid & 1] = (tid & 1) ? Dvec[(size_t)bh * g.n + g.nm + (tid >> 1)] : LSE[(size_t)bh * g.n + g.nm + (tid >> 1)];
  __syncthreads();
  for (int it = 0; it < ntiles; ++it) {
    const int cur = it & 1, nxt = cur ^ 1;
    const bool more = it + 1 < ntiles;
    float stat_next = 0.f;
    if (more) {
      qr.load(Qb, rs, (it + 1) * 32, g.nm, tid);
      dr.load(dOb, os, (it + 1) * 32, g.nm, tid);
      stat_next = row_stat((it + 1) * 32);                      // issued with the tile loads, consumed after the tile's work
    }
    int pz = 0;                                                 // an opaque 0: the fragment addresses are formed per tile, not held across the loop
    asm volatile("" : "+v"(pz));
    const int ln = lane + pz;
    const unsigned* qt = Qs + cur * ATS_TILE;
    const unsigned* dt = dOs + cur * ATS_TILE;
    if (vec && it % W == wave) {
      const float lse_q = Rs[cur * 64 + (lane & 31)], d_q = Rs[cur * 64 + 32 + (lane & 31)];
#pragma unroll
      for (int t = 0; t < TMAX; ++t)
        if (t < nt) {
          const float sv = vec_row_dot(qt, vecK[t], lane), dpv = vec_row_dot(dt, vecV[t], lane);
          const float pv = vatt[t] ? fast_exp(sv * g.scale - lse_q) : 0.f;
          vdv[t] += vec_wsum(dt, pv, lane);
          vdk[t] += vec_wsum(qt, pv * (dpv - d_q) * g.scale, lane);
        }
    }
    if (wave_active) {
      const float* st = Rs + cur * 64;
      f32x16 s, dp;
      zero_acc(s);
      zero_acc(dp);
      mma_tile_own(s, qt, kf, ln);                            // S  = Q K^T : s[e] <-> (query acc_row(e, half), key lane)
      mma_tile_own(dp, dt, vf, ln);                           // dP = dO V^T
      float p[16], ds[16];
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int r = acc_row(e, half);
        p[e] = attend ? fast_exp(s[e] * g.scale - st[r]) : 0.f;
        ds[e] = p[e] * (dp[e] - st[32 + r]) * g.scale;
      }
      mma_tileT_acc(dv0, dv1, dt, p, ln);                     // dV^T += dO^T P
      mma_tileT_acc(dk0, dk1, qt, ds, ln);                    // dK^T += Q^T dS
    }
    if (more) {
      split_tile_store(Qs + nxt * ATS_TILE, qr, tid);
      split_tile_store(dOs + nxt * ATS_TILE, dr, tid);
      if (tid < 64) Rs[nxt * 64 + tid] = stat_next;
    }
    __syncthreads();
  }
  if (vec) {        // remainder keys: wave 0 adds the remainder queries, the waves' partial dK / dV rows are summed, wave 0 writes
#pragma unroll
    for (int t = 0; t < TMAX; ++t)
      if (t < nt) {
        if (wave == 0)
          for (int qq = g.nm; qq < g.n; ++qq) {
            const float sq = wave_sum(vecK[t][lane] * tailQ[qq - g.nm][lane]), dpq = wave_sum(vecV[t][lane] * tailD[qq - g.nm][lane]);
            const float pq = vatt[t] ? fast_exp(sq * g.scale - tailS[qq - g.nm][0]) : 0.f;
            vdv[t] += pq * tailD[qq - g.nm][lane];
            vdk[t] += pq * (dpq - tailS[qq - g.nm][1]) * g.scale * tailQ[qq - g.nm][lane];
          }
        vred[wave][t][0][lane] = vdk[t];
        vred[wave][t][1][lane] = vdv[t];
      }
    __syncthreads();
    if (wave == 0)
#pragma unroll
      for (int t = 0; t < TMAX; ++t)
        if (t < nt) {
          float a = 0.f, c = 0.f;
#pragma unroll
          for (int w = 0; w < W; ++w) {
            a += vred[w][t][0][lane];
            c += vred[w][t][1][lane];
          }
          dqkv[qkv_off(g, b, g.nm + t, 1, h) + lane] = a;
          dqkv[qkv_off(g, b, g.nm + t, 2, h) + lane] = c;
        }
    __syncthreads();
  }
  if (!wave_active) return;
  if (nt > 0) {                                                  // remainder queries: vector code
    float kreg[32], vreg[32];
    own_rows_load_k(kreg, Kb, rs, key, g.nm, half);
    own_rows_load_k(vreg, Vb, rs, key, g.nm, half);
    for (int qq = g.nm; qq < g.n; ++qq) {
      const float* qrow = tailQ[qq - g.nm];
      const float* drow = tailD[qq - g.nm];
      const float sq = own_dot(kreg, qrow, half), dpq = own_dot(vreg, drow, half);
      const float pq = attend ? fast_exp(sq * g.scale - tailS[qq - g.nm][0]) : 0.f;
      own_axpy(dv0, dv1, drow, pq, half);
      own_axpy(dk0, dk1, qrow, pq * (dpq - tailS[qq - g.nm][1]) * g.scale, half);
    }
  }
  float* stage = reinterpret_cast<float*>(smem) + wave * 32 * ATT_LD;
  store_ownT(stage, dk0, dk1, dqkv + qkv_off(g, b, 0, 1, h), rs, k0, g.nm, lane, 1.0f);
  __builtin_amdgcn_wave_barrier();
  store_ownT(stage, dv0, dv1, dqkv + qkv_off(g, b, 0, 2, h), rs, k0, g.nm, lane, 1.0f);
}

// the (W, TAIL) instantiation attention.hip's host code picks for (nm, n): TAIL = 1 for [cls] + 32 m, ATT_TAIL_MAX for any other
// remainder, 0 for none
#define ATS_LAUNCH(KERNEL, ...)                                                                       \
  do {                                                                                                \
    if (nm + 1 == n) {                                                                                \
      if (W == 4) KERNEL<4, 1><<<grid, 256, 0, st>>>(__VA_ARGS__);                                    \
      else if (W == 3) KERNEL<3, 1><<<grid, 192, 0, st>>>(__VA_ARGS__);                               \
      else KERNEL<2, 1><<<grid, 128, 0, st>>>(__VA_ARGS__);                                           \
    } else if (nm < n) {                                                                              \
      if (W == 4) KERNEL<4, ATT_TAIL_MAX><<<grid, 256, 0, st>>>(__VA_ARGS__);                         \
      else if (W == 3) KERNEL<3, ATT_TAIL_MAX><<<grid, 192, 0, st>>>(__VA_ARGS__);                    \
      else KERNEL<2, ATT_TAIL_MAX><<<grid, 128, 0, st>>>(__VA_ARGS__);                                \
    } else {                                                                                          \
      if (W == 4) KERNEL<4, 0><<<grid, 256, 0, st>>>(__VA_ARGS__);                                    \
      else if (W == 3) KERNEL<3, 0><<<grid, 192, 0, st>>>(__VA_ARGS__);                               \
      else KERNEL<2, 0><<<grid, 128, 0, st>>>(__VA_ARGS__);                                           \
    }                                                                                                 \
  } while (0)

}  // namespace

extern "C" int mla_attention_fwd_split(const float* qkv, const float* pad_mask, float* o, float* lse, int B, int H, int n, int hd,
                                       void* stream) {
  MLA_REQUIRE(qkv && o && lse, "mla_attention_fwd_split: null pointer");
  if (int rc = check_att("mla_attention_fwd_split", B, H, n, hd)) return rc;
  const int nm = att_main_rows(n);
  if (nm == 0) return mla_attention_fwd(qkv, pad_mask, o, lse, B, H, n, hd, stream);   // n <= ATT_TAIL_MAX: vector kernels, no product on an MFMA
  AttGeom g{qkv, pad_mask, B, H, n, nm, 1.0f / sqrtf((float)hd)};
  hipStream_t st = (hipStream_t)stream;
  const int W = att_waves(nm);
  const dim3 grid(cdiv(nm, 32 * W), B * H);
  ATS_LAUNCH(attn_fwd_split_kernel, g, o, lse);
  MLA_CHECK_LAUNCH("attn_fwd_split_kernel");
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
  const int W = att_waves(nm);
  const dim3 grid(cdiv(nm, 32 * W), B * H);
  // order matters: the query-side kernel writes dvec (rowsum(d_o * o)) for every row before the key-side kernel reads it
  ATS_LAUNCH(attn_bwd_dq_split_kernel, g, d_o, o, lse, dvec, dqkv);
  MLA_CHECK_LAUNCH("attn_bwd_dq_split_kernel");
  ATS_LAUNCH(attn_bwd_dkv_split_kernel, g, d_o, lse, dvec, dqkv);
  MLA_CHECK_LAUNCH("attn_bwd_dkv_split_kernel");
  return MLA_OK;
}
