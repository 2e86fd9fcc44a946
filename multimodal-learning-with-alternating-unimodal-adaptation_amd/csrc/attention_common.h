// Pieces the fused-attention kernels (attention_kernels.h) and their arithmetics (attention.hip: fp32 MFMA, attention_split.hip: split
// bf16) share: the geometry, the global -> register tile loads, the accumulator-layout helpers, the mask rule, fast_exp and the
// host-side kernel selection.  Everything here is independent of how a product is formed.
#pragma once
#include <type_traits>
#include "common.h"

#define ATT_HD 64          // head dim (ViT-B: 768 / 12)
#define ATT_LD 68          // padded LDS row (floats): 17 x 16 B -> conflict-free ds_read_b128 across 32 rows
#define ATT_TAIL_MAX 3     // n % 32 <= this: the remainder rows take the vector path
#define ATT_TAIL_N 4096    // longest sequence the one-wave tail kernels hold in LDS

namespace {

// exp via v_exp_f32 (2^x): the accurate expf expands to ~20 VALU instructions, 16 of them per lane and key tile were a
// quarter of the forward's issue slots.  Relative error <= |x| 2^-23 (the rounding of x * log2 e), i.e. < 3e-6 for the
// score range a softmax row can hold before the result underflows anyway; arguments of -inf / -1e7 give exactly 0.
__device__ __forceinline__ float fast_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896340736f); }

__device__ __forceinline__ int acc_row(int e, int half) { return (e & 3) + 8 * (e >> 2) + 4 * half; }
__device__ __forceinline__ void att_zero(f32x16& acc) {
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
}

struct AttGeom {
  const float* qkv;        // (B, n, 3, H, 64)
  const float* pm;         // (B, n) or null
  int B, H, n;
  int nm;                  // rows [0, nm) are handled by the MFMA kernels (nm % 32 == 0 or nm == n); rows [nm, n) -- at most
                           // ATT_TAIL_MAX of them -- by vector code: the [cls] token makes n = 257 = 8 tiles + 1, and a ninth
                           // 32-wide tile / a ninth wave block for that one row cost 60 % more time than n = 256
  float scale;
};

// byte-free helpers: element offset of (b, t, which, h, 0)
__device__ __forceinline__ size_t qkv_off(const AttGeom& g, int b, int t, int which, int h) {
  return (((size_t)b * g.n + t) * 3 + which) * (size_t)(g.H * ATT_HD) + (size_t)h * ATT_HD;
}

// One 32 x 64 tile (rows t0.., zero-filled beyond n) from global into registers / from registers into padded LDS.
// NT threads: float4 slot idx = tid + NT p of the 512 (row = idx / 16, float4 column idx % 16).
template <int NT>
struct TileRegs {
  static constexpr int P = (512 + NT - 1) / NT;
  f32x4 r[P];
  __device__ __forceinline__ void load(const float* base, size_t row_stride, int t0, int n, int tid) {
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const int idx = tid + NT * p, row = idx >> 4;
      r[p] = (idx < 512 && t0 + row < n) ? *reinterpret_cast<const f32x4*>(base + (size_t)(t0 + row) * row_stride + (idx & 15) * 4)
                                         : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
  __device__ __forceinline__ void store(float* lds, int tid) const {
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const int idx = tid + NT * p;
      if (idx < 512) *reinterpret_cast<f32x4*>(&lds[(idx >> 4) * ATT_LD + (idx & 15) * 4]) = r[p];
    }
  }
};

// Write a wave's transposed 64 x 32 result (o0 / o1: row = feature, column = own row) to global rows of 64 floats.
// stage: this wave's 32 x ATT_LD floats of LDS.
__device__ __forceinline__ void store_ownT(float* stage, const f32x16& o0, const f32x16& o1, float* dst, size_t row_stride,
                                            int row0, int n, int lane, float mul) {
  const int half = lane >> 5, c = lane & 31;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    stage[c * ATT_LD + acc_row(e, half)] = o0[e] * mul;
    stage[c * ATT_LD + 32 + acc_row(e, half)] = o1[e] * mul;
  }
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    const int idx = p * 64 + lane, r = idx >> 4, c4 = idx & 15;
    if (row0 + r < n)
      *reinterpret_cast<f32x4*>(dst + (size_t)(row0 + r) * row_stride + c4 * 4) = *reinterpret_cast<const f32x4*>(&stage[r * ATT_LD + c4 * 4]);
  }
}

// key state of a tile: 0 = attend, 1 = padded (score := -1e7), 2 = beyond n
__device__ __forceinline__ float key_state(const AttGeom& g, int b, int key, int limit) {
  if (key >= limit) return 2.f;
  return (g.pm && g.pm[(size_t)b * g.n + key] > 0.f) ? 1.f : 0.f;
}

// out^T (+)= row (x) w : rank-1 update of a transposed 64 x 32 accumulator pair with one broadcast row and a per-lane weight
__device__ __forceinline__ void own_axpy(f32x16& o0, f32x16& o1, const float* __restrict__ row, float w, int half) {
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    o0[e] += row[acc_row(e, half)] * w;
    o1[e] += row[32 + acc_row(e, half)] * w;
  }
}

// rows the MFMA kernels own: everything, unless the last partial tile holds <= ATT_TAIL_MAX rows
inline int att_main_rows(int n) {
  const int r = n % 32;
  return (r > 0 && r <= ATT_TAIL_MAX && n <= ATT_TAIL_N) ? n - r : n;
}

// Waves (= blocks of 32 owned rows) per workgroup: the sequence is cut into ceil(n / 32) wave blocks and a workgroup whose
// last waves have no rows keeps its CU slot for the whole key loop, so pick the width that leaves the fewest idle waves
// (n = 257 = cls + 256: nine blocks -> three workgroups of three waves instead of 4 + 4 + 1; n = 512: four).
inline int att_waves(int n) {
  const int blocks = (n + 31) / 32;
  int best = 4, best_idle = 1 << 30;
  for (int w = 4; w >= 2; --w) {
    const int idle = ((blocks + w - 1) / w) * w - blocks;
    if (idle < best_idle) { best = w; best_idle = idle; }
  }
  return best;
}

// The one place that maps a length to an instantiation, nm = att_main_rows(n) > 0: W = att_waves(nm) waves; TAIL = 1 for [cls] + 32 m
// (one remainder row: 3 instead of 9 state registers), ATT_TAIL_MAX for any other remainder, 0 for none.
// launch(W, TAIL, grid, block) receives both as std::integral_constant and starts its kernel<.., W, TAIL>.
template <class Launch>
inline void att_launch(int nm, int n, int BH, Launch&& launch) {
  const int W = att_waves(nm);
  const dim3 grid(cdiv(nm, 32 * W), BH), block(64 * W);
  auto with_tail = [&](auto w) {
    if (nm + 1 == n) launch(w, std::integral_constant<int, 1>{}, grid, block);
    else if (nm < n) launch(w, std::integral_constant<int, ATT_TAIL_MAX>{}, grid, block);
    else launch(w, std::integral_constant<int, 0>{}, grid, block);
  };
  if (W == 4) with_tail(std::integral_constant<int, 4>{});
  else if (W == 3) with_tail(std::integral_constant<int, 3>{});
  else with_tail(std::integral_constant<int, 2>{});
}

inline int check_att(const char* who, int B, int H, int n, int hd) {
  MLA_REQUIRE(B > 0 && H > 0 && n > 0, "%s: non-positive dims", who);
  MLA_REQUIRE(hd == ATT_HD, "%s: head dim %d unsupported (64)", who, hd);
  MLA_REQUIRE((long)B * H < 65536 && (long)B * n * 3 * H * hd < (1L << 31), "%s: problem too large", who);
  return MLA_OK;
}

}  // namespace
