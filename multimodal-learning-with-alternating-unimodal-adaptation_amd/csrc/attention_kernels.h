// Fused multi-head attention for the transformer rows, forward and backward: the three MFMA kernels, written once for every
// arithmetic.  attention.hip instantiates them with AttF32 (exact fp32 on v_mfma_f32_32x32x2_f32), attention_split.hip with AttSplit
// (the exact three-way bf16 split on v_mfma_f32_32x32x16_bf16); each of those files says what its arithmetic supplies.
//
//   reference: Attention.forward, models/m3ae.py:102-125 (and timm's Attention inside cav_mae.py:93):
//     attention = (q @ k^T) * scale;  attention = where(padding_mask > 0, -1e7, attention)  (m3ae.py:109-117)
//     attention = softmax(attention, -1);  x = attention @ v  -> (B, n, H*hd)                  (m3ae.py:118-122)
//
// q, k, v are read in place from the (B, n, 3, H, 64) buffer the fused qkv Linear writes; the output lands in (B, n, H*64).
// The n x n score / probability matrices never reach HBM (the materialised form moved 2 x 203 MB per layer at B = 64 and
// ran its batched GEMMs at 43 TFLOP/s): forward keeps an online softmax, backward recomputes the probabilities from the
// saved log-sum-exp.  Everything is deterministic (no atomics): the backward is two kernels, one that owns query rows
// (dQ) and one that owns key rows (dK, dV).
//
// Wave-level formulation (64-wide wavefronts, 32 x 32 MFMA tiles): every wave owns 32 rows of its output operand and walks the
// other sequence dimension in tiles of 32 through LDS.  Scores are produced TRANSPOSED to the operand the wave owns
// (forward / dQ: S^T = K Q^T, so a lane holds 16 keys of ONE query), which makes the softmax statistics per-lane scalars
// (one cross-half shuffle per tile instead of 32-lane reductions) and -- because the k index of an MFMA contraction may
// be enumerated in any order as long as A and B agree -- lets the probability accumulator registers be fed straight back
// as the B operand of the next product (P^T as [key][query]) without a round trip through LDS.
//
// Ragged lengths: a sequence of n = 32 m + r tokens with r <= 3 (M3AE: 257 = [cls] + 256) is split into m full tiles for the
// MFMA kernels and r remainder rows that are handled by vector code -- as extra keys / queries at the end of each MFMA wave's
// loop (a dot product and a rank-1 update per row) and, as OWNED rows, by workgroup 0 of every (b, h), which runs plain
// vector code on the tiles it has in LDS anyway, next to its own MFMA rows; a ninth 32-wide tile and a ninth wave block for one row made
// n = 257 cost 1.6x of n = 256.  TAIL is the number of remainder rows an instantiation can own: 0, 1 (the [cls] + 32 m case:
// 3 instead of 9 state registers) or ATT_TAIL_MAX; W is the number of waves (att_launch picks both).
//
// Masking: keys beyond n do not exist (-inf, probability exactly 0); padded keys (mask > 0) have their score REPLACED by
// -1e7 like the reference, which underflows to probability exactly 0 in fp32 unless a whole row is padded (never: the
// [cls] key is always present, m3ae.py:347).
//
// What a Math type supplies (everything else -- staging loop, double buffer, mask rule, softmax, remainder rows, epilogue -- is here):
//   Elem, TILE                       element type and elements per 32 x 64 tile image in LDS
//   tile_store                       TileRegs -> tile image
//   Own, own_load                    a wave-owned block of 32 rows as the B operand of mma_tile_own
//   own_rows_f32, own_dot            the fp32 view of an owned block for the remainder loop after the tile loop, and a dot product on it
//   mma_tile_own, mma_tileT_acc      the products: tile x own^T and tile^T x accumulator-layout weights
//   vec_row_dot, vec_wsum            vector code on a staged tile, for the OWNED remainder rows
//   fwd_wgs, dq_wgs, dkv_wgs         second argument of __launch_bounds__ per role
//   dq_own_load, dq_dsum, tile_lane  where register allocation wants a statement placed (see AttSplit; free in AttF32)
#pragma once
#include "attention_common.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// forward: workgroup = 32 W queries of one (b, h); loop over key tiles of 32.  o (B, n, H*64), lse (B, H, n).
// ---------------------------------------------------------------------------------------------------------------------
template <class Math, int W, int TAIL>
__global__ __launch_bounds__(64 * W, Math::fwd_wgs(W, TAIL)) void attn_fwd_kernel(const AttGeom g, float* __restrict__ O, float* __restrict__ LSE) {
  typedef typename Math::Elem Elem;
  constexpr int TMAX = TAIL > 0 ? TAIL : 1;      // remainder rows this instantiation can own (TAIL = 1: the [cls] + 256 case, 3: any)
  __shared__ __attribute__((aligned(16))) Elem smem[2 * 2 * Math::TILE + 2 * 32];
  Elem* Ks = smem;                               // [2] tile images
  Elem* Vs = smem + 2 * Math::TILE;              // [2] tile images
  float* Kst = reinterpret_cast<float*>(smem + 4 * Math::TILE);    // [2][32] key states
  __shared__ __attribute__((aligned(16))) float tailK[ATT_TAIL_MAX][ATT_HD], tailV[ATT_TAIL_MAX][ATT_HD];   // the remainder keys [nm, n), fp32
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5;
  const int bh = blockIdx.y, b = bh / g.H, h = bh - b * g.H;
  const int q = blockIdx.x * (32 * W) + wave * 32 + (lane & 31);
  // With remainder rows (TAIL) workgroup 0 of every (b, h) owns them IN ADDITION to its MFMA rows (see vec_row_dot): tile jt is
  // handled by wave jt % W, each wave keeps a partial (max, sum, weighted row) state, wave 0 merges them at the end -- ~7 % more
  // work per wave of that workgroup.  Measured alternatives at n = 257 (fp32 forward, us; n = 256 takes 124): everything on wave 0
  // (155), a fifth wave per workgroup (192), one more workgroup per (b, h) that only stages tiles and runs the vector code (173),
  // stand-alone vector kernels reading global memory (164, and 2 x 40 in the backward), a ninth padded tile / wave block (202).
  const bool vec = TAIL && blockIdx.x == 0;
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

  typename Math::Own qown;
  Math::own_load(qown, Qb, rs, q, g.nm, half);
  if (vec && wave == 0)
    for (int t = 0; t < nt; ++t) vecQ[t][lane] = Qb[(size_t)(g.nm + t) * rs + lane];
  if (tid < nt) tailSt[tid] = key_state(g, b, g.nm + tid, g.n);
  f32x16 o0, o1;
  att_zero(o0);
  att_zero(o1);
  float m_i = -INFINITY, l_i = 0.f;

  const int ntiles = (g.nm + 31) / 32;
  TileRegs<64 * W> kr, vr;
  kr.load(Kb, rs, 0, g.nm, tid);
  vr.load(Vb, rs, 0, g.nm, tid);
  Math::tile_store(Ks, kr, tid);
  Math::tile_store(Vs, vr, tid);
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
    const Elem* kt = Ks + cur * Math::TILE;
    const Elem* vt = Vs + cur * Math::TILE;
    if (vec && jt % W == wave) {
      const float st = Kst[cur * 32 + (lane & 31)];
#pragma unroll
      for (int t = 0; t < TMAX; ++t)
        if (t < nt) {
          float sv = Math::vec_row_dot(kt, vecQ[t], lane);
          sv = st == 0.f ? sv * g.scale : (st == 1.f ? -1e7f : -INFINITY);
          const float m_new = fmaxf(vm[t], wave_max(sv));
          const float alpha = fast_exp(vm[t] - m_new), pv = fast_exp(sv - m_new);
          vl[t] = vl[t] * alpha + wave_sum(half == 0 ? pv : 0.f);
          vm[t] = m_new;
          vo[t] = vo[t] * alpha + Math::vec_wsum(vt, pv, lane);
        }
    }
    if (wave_active) {
      f32x16 s;
      att_zero(s);
      Math::mma_tile_own(s, kt, qown, lane);                    // S^T = K Q^T: s[e] <-> (key acc_row(e, half), query lane)
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
      Math::mma_tileT_acc(o0, o1, vt, p, lane);                 // O^T += V^T P^T
    }
    if (more) {
      Math::tile_store(Ks + nxt * Math::TILE, kr, tid);
      Math::tile_store(Vs + nxt * Math::TILE, vr, tid);
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
    __syncthreads();                                               // vred shares nothing with the staging below, but keep the waves together
  }
  if (!wave_active) return;
  if (nt > 0) {                                                  // remainder keys (e.g. the 257th token): vector code
    float qreg[32];
    Math::own_rows_f32(qreg, qown, Qb, rs, q, g.nm, half);
    for (int j = g.nm; j < g.n; ++j) {
      const float sj = tailSt[j - g.nm] == 0.f ? Math::own_dot(qreg, tailK[j - g.nm], half) * g.scale : -1e7f;
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
// backward, query side: workgroup = 32 W queries; loop over key tiles.  Recomputes P^T from LSE, writes dQ and
// Dvec[b, h, q] = sum_d dO * O (consumed by the key-side kernel).
// ---------------------------------------------------------------------------------------------------------------------
template <class Math, int W, int TAIL>
__global__ __launch_bounds__(64 * W, Math::dq_wgs(W)) void attn_bwd_dq_kernel(const AttGeom g, const float* __restrict__ dO, const float* __restrict__ O,
                                                                          const float* __restrict__ LSE, float* __restrict__ Dvec,
                                                                          float* __restrict__ dqkv) {
  typedef typename Math::Elem Elem;
  constexpr int TMAX = TAIL > 0 ? TAIL : 1;
  __shared__ __attribute__((aligned(16))) Elem smem[2 * 2 * Math::TILE + 2 * 32];
  Elem* Ks = smem;
  Elem* Vs = smem + 2 * Math::TILE;
  float* Kst = reinterpret_cast<float*>(smem + 4 * Math::TILE);
  __shared__ __attribute__((aligned(16))) float tailK[ATT_TAIL_MAX][ATT_HD], tailV[ATT_TAIL_MAX][ATT_HD];   // the remainder keys [nm, n), fp32
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5;
  const int bh = blockIdx.y, b = bh / g.H, h = bh - b * g.H;
  const int q0 = blockIdx.x * (32 * W) + wave * 32, q = q0 + (lane & 31);
  const bool vec = TAIL && blockIdx.x == 0;                   // this workgroup also owns the remainder queries [nm, n) (see attn_fwd_kernel)
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

  typename Math::Own qown, doown;
  float dsum = Math::dq_own_load(qown, doown, Qb, rs, dOb, Ob, os, q, g.nm, half);
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
  dsum = Math::dq_dsum(dsum, doown, Ob, os, q, g.nm, half);       // rowsum(dO * O) of the owned query, on both lanes of its row
  const float lse = q < g.nm ? LSE[(size_t)bh * g.n + q] : INFINITY;   // rows beyond nm: p = exp(s - inf) = 0
  if (half == 0 && q < g.nm) Dvec[(size_t)bh * g.n + q] = dsum;
  f32x16 dq0, dq1;
  att_zero(dq0);
  att_zero(dq1);

  const int ntiles = (g.nm + 31) / 32;
  TileRegs<64 * W> kr, vr;
  kr.load(Kb, rs, 0, g.nm, tid);
  vr.load(Vb, rs, 0, g.nm, tid);
  Math::tile_store(Ks, kr, tid);
  Math::tile_store(Vs, vr, tid);
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
    const Elem* kt = Ks + cur * Math::TILE;
    const Elem* vt = Vs + cur * Math::TILE;
    if (vec && jt % W == wave) {
      const bool att = Kst[cur * 32 + (lane & 31)] == 0.f;
#pragma unroll
      for (int t = 0; t < TMAX; ++t)
        if (t < nt) {
          const float sv = Math::vec_row_dot(kt, vecQ[t], lane), dpv = Math::vec_row_dot(vt, vecD[t], lane);
          const float pv = att ? fast_exp(sv * g.scale - vlse[t]) : 0.f;
          vdq[t] += Math::vec_wsum(kt, pv * (dpv - vD[t]) * g.scale, lane);
        }
    }
    if (wave_active) {
      f32x16 s, dp;
      att_zero(s);
      att_zero(dp);
      Math::mma_tile_own(s, kt, qown, lane);                    // S^T  = K Q^T
      Math::mma_tile_own(dp, vt, doown, lane);                  // dP^T = V dO^T
      float ds[16];
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const float st = Kst[cur * 32 + acc_row(e, half)];
        const float pe = st == 0.f ? fast_exp(s[e] * g.scale - lse) : 0.f;   // padded keys: exp(-1e7 - lse) == 0 exactly
        ds[e] = pe * (dp[e] - dsum) * g.scale;
      }
      Math::mma_tileT_acc(dq0, dq1, kt, ds, lane);              // dQ^T += K^T dS^T
    }
    if (more) {
      Math::tile_store(Ks + nxt * Math::TILE, kr, tid);
      Math::tile_store(Vs + nxt * Math::TILE, vr, tid);
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
    Math::own_rows_f32(qreg, qown, Qb, rs, q, g.nm, half);
    Math::own_rows_f32(doreg, doown, dOb, os, q, g.nm, half);
    for (int j = g.nm; j < g.n; ++j) {
      const float sj = Math::own_dot(qreg, tailK[j - g.nm], half), dpj = Math::own_dot(doreg, tailV[j - g.nm], half);
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
template <class Math, int W, int TAIL>
__global__ __launch_bounds__(64 * W, Math::dkv_wgs(W)) void attn_bwd_dkv_kernel(const AttGeom g, const float* __restrict__ dO, const float* __restrict__ LSE,
                                                                            const float* __restrict__ Dvec, float* __restrict__ dqkv) {
  typedef typename Math::Elem Elem;
  constexpr int TMAX = TAIL > 0 ? TAIL : 1;
  __shared__ __attribute__((aligned(16))) Elem smem[2 * 2 * Math::TILE + 2 * 64];
  Elem* Qs = smem;
  Elem* dOs = smem + 2 * Math::TILE;
  float* Rs = reinterpret_cast<float*>(smem + 4 * Math::TILE);      // [2][64]: lse (32) | Dvec (32) of the query tile
  __shared__ __attribute__((aligned(16))) float tailQ[ATT_TAIL_MAX][ATT_HD], tailD[ATT_TAIL_MAX][ATT_HD];   // remainder queries: Q, dO rows, fp32
  __shared__ float tailS[ATT_TAIL_MAX][2];                                                                  // their lse, rowsum(dO * O)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5;
  const int bh = blockIdx.y, b = bh / g.H, h = bh - b * g.H;
  const int k0 = blockIdx.x * (32 * W) + wave * 32, key = k0 + (lane & 31);
  const bool vec = TAIL && blockIdx.x == 0;                   // this workgroup also owns the remainder keys [nm, n) (see attn_fwd_kernel)
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

  typename Math::Own kown, vown;
  Math::own_load(kown, Kb, rs, key, g.nm, half);
  Math::own_load(vown, Vb, rs, key, g.nm, half);
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
  att_zero(dk0);
  att_zero(dk1);
  att_zero(dv0);
  att_zero(dv1);

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
  Math::tile_store(Qs, qr, tid);
  Math::tile_store(dOs, dr, tid);
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
    const int ln = Math::tile_lane(lane);                       // the lane the products of this tile address LDS with
    const Elem* qt = Qs + cur * Math::TILE;
    const Elem* dt = dOs + cur * Math::TILE;
    if (vec && it % W == wave) {
      const float lse_q = Rs[cur * 64 + (lane & 31)], d_q = Rs[cur * 64 + 32 + (lane & 31)];
#pragma unroll
      for (int t = 0; t < TMAX; ++t)
        if (t < nt) {
          const float sv = Math::vec_row_dot(qt, vecK[t], lane), dpv = Math::vec_row_dot(dt, vecV[t], lane);
          const float pv = vatt[t] ? fast_exp(sv * g.scale - lse_q) : 0.f;
          vdv[t] += Math::vec_wsum(dt, pv, lane);
          vdk[t] += Math::vec_wsum(qt, pv * (dpv - d_q) * g.scale, lane);
        }
    }
    if (wave_active) {
      const float* st = Rs + cur * 64;
      f32x16 s, dp;
      att_zero(s);
      att_zero(dp);
      Math::mma_tile_own(s, qt, kown, ln);                      // S  = Q K^T : s[e] <-> (query acc_row(e, half), key lane)
      Math::mma_tile_own(dp, dt, vown, ln);                     // dP = dO V^T
      float p[16], ds[16];
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int r = acc_row(e, half);
        p[e] = attend ? fast_exp(s[e] * g.scale - st[r]) : 0.f;
        ds[e] = p[e] * (dp[e] - st[32 + r]) * g.scale;
      }
      Math::mma_tileT_acc(dv0, dv1, dt, p, ln);                 // dV^T += dO^T P
      Math::mma_tileT_acc(dk0, dk1, qt, ds, ln);                // dK^T += Q^T dS
    }
    if (more) {
      Math::tile_store(Qs + nxt * Math::TILE, qr, tid);
      Math::tile_store(dOs + nxt * Math::TILE, dr, tid);
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
    Math::own_rows_f32(kreg, kown, Kb, rs, key, g.nm, half);
    Math::own_rows_f32(vreg, vown, Vb, rs, key, g.nm, half);
    for (int qq = g.nm; qq < g.n; ++qq) {
      const float* qrow = tailQ[qq - g.nm];
      const float* drow = tailD[qq - g.nm];
      const float sq = Math::own_dot(kreg, qrow, half), dpq = Math::own_dot(vreg, drow, half);
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

}  // namespace
