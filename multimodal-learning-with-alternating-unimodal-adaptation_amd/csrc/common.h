// Shared helpers for the gfx950 kernels of libmla_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "args_common.h"

#define MLA_WAVE 64

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define MLA_CHECK_LAUNCH(name)                                             \
  do {                                                                     \
    hipError_t e__ = hipGetLastError();                                    \
    if (e__ != hipSuccess) {                                               \
      mla_set_error("%s: launch failed: %s", name, hipGetErrorString(e__)); \
      return MLA_ERR_LAUNCH;                                               \
    }                                                                      \
  } while (0)

static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// CU count of the device current at the first call (the persistent grids and the tile-round models of every planner).  256 -- the
// MI355X's -- when no device answers, so the host-side size and support queries stay usable without a GPU.
inline int mla_cu_count() {
  static const int cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    return n;
  }();
  return cus;
}

// An int setting with an environment default, behind a measurement hook.  The variable is read once, at the first use: its first
// character when that is a digit in [lo, hi] (numeric: atoi, clamped to [lo, hi]), else dflt.  hook(x) sets x when lo <= x <= hi and
// answers the current value either way (out-of-range arguments are queries); internal code reads get().
struct EnvInt {
  const char* name;
  int lo, hi, dflt;
  bool numeric = false;
  int v = INT_MIN;               // INT_MIN: neither set nor read yet
  int get() {
    if (v == INT_MIN) {
      const char* e = getenv(name);
      v = dflt;
      if (e && numeric) { const int x = atoi(e); v = x < lo ? lo : (x > hi ? hi : x); }
      else if (e && e[0] >= '0' + lo && e[0] <= '0' + hi) v = e[0] - '0';
    }
    return v;
  }
  int hook(int x) {
    if (x >= lo && x <= hi) v = x;
    return get();
  }
};

// wave-level reductions (64 lanes)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_min_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double wave_max_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// the one BatchNorm expression (explicit fma) every kernel that forms or re-forms bn(x) uses: identical rounding everywhere
// (bn.hip: bn_val; the convolution kernels that fold relu(bn(.)) into their operand staging)
__device__ __forceinline__ float bn_val1(float x, float mu, float is, float ga, float be) { return fmaf((x - mu) * is, ga, be); }

// The stem's BatchNorm backward fed by the POOLED gradient (bn.hip: bn_bwd_pooled_apply_kernel; stem_split.hip: the weight-gradient
// kernel that forms conv1's gradient while it loads it).  Both call these two, with the one contraction written out, so the two
// paths agree bit for bit.
//   pool_pick: g += the pooled gradient w of a window whose selected position `sel` is this pixel's position `code` in it; the
//              windows of a pixel are visited in (wy, wx) order starting from g = 0.
//   bn_bwd_pooled_dy1: dy = gamma * invstd * ([bn(y) > 0] g - dbeta / M - xhat * dgamma / M); dg = dgamma / M, db = dbeta / M.
//   bn_inv_count, bn_bwd_scale: the 1 / M both use, and dg / db from the reduced sums -- a product the compiler must not contract
//              into the subtraction that consumes it (it would, in one kernel and not in the other).
__device__ __forceinline__ float pool_pick(float g, int sel, int code, float w) { return g + (sel == code ? w : 0.f); }
__device__ __forceinline__ float bn_bwd_pooled_dy1(float y, float g, float mu, float is, float ga, float be, float dg, float db) {
  const float gm = bn_val1(y, mu, is, ga, be) > 0.f ? g : 0.f;
  const float xhat = (y - mu) * is;
  return (ga * is) * fmaf(-xhat, dg, gm - db);
}
__device__ __forceinline__ float bn_inv_count(int N, int H, int W) { return 1.0f / ((float)N * (float)H * (float)W); }
__device__ __forceinline__ float bn_bwd_scale(float sum, float invM) { return __fmul_rn(sum, invM); }

// Logical tile id -> (tm, tn).  Narrow outputs (gridN <= 8: every ResNet conv) keep the row-major order.  Wide outputs
// (transformer Linears: N = 768..3072, up to 48 column tiles) are walked in column PANELS of 8 tiles: all row tiles of a
// panel before the next panel, so the panel's B operand (8 x BN x K x 4 B <= 3 MB) stays in the 4 MB per-XCD L2 while A
// streams through once per panel.  Row-major order re-read the whole weight matrix (7-9 MB) from the fabric for every row
// of tiles: 1.8 GB per 16448 x 2304 x 768 GEMM, which held the Linear layers at 76 TFLOP/s (profiles/r02_m3ae_*).
__device__ __forceinline__ void tile_coords(int wg, int gridM, int gridN, int& tm, int& tn) {
  if (gridN <= 8) {
    tm = wg / gridN;
    tn = wg - tm * gridN;
    return;
  }
  const int per_panel = gridM * 8;
  int panel = wg / per_panel;
  const int full = gridN >> 3;                     // panels of width 8; a narrower one follows if gridN % 8 != 0
  if (panel > full) panel = full;
  const int rem = wg - panel * per_panel;
  const int pw = panel < full ? 8 : gridN - full * 8;
  tm = rem / pw;
  tn = panel * 8 + (rem - tm * pw);
}

// Bijective XCD-aware remap of a flat workgroup id: consecutive logical ids land on the same XCD
// (blocks b and b+8 share an XCD/L2 under round-robin dispatch).  Speed only, never correctness.
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7, x = bid & 7, l = bid >> 3;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + l;
}
