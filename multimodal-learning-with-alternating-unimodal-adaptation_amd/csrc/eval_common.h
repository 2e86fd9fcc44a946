// What the four evaluation kernels -- eval_fuse_kernel and eval_head_kernel (eval_head.hip), scores_append_kernel (metrics.hip),
// fusion_sweep_kernel (fusion_sweep.hip) -- and their host halves (eval_args.h, metrics_args.h, sweep_args.h) are written on.  The
// path promises bit-for-bit agreement between its kernels: a grid row of the sweep equal to an evaluator's alphas predicts what that
// evaluator predicts, head 0 of the score store is the fused row eval_fuse_kernel took its arg-max of.  Each expression those promises
// rest on is defined once, below.  Two kernels keep sites written out, each with a comment naming the helper, because the call
// changed their instruction stream and the A/B run came out slower (profiles/eval_common_ab.json):
// eval_head_kernel's eligibility, fixed-alpha rule and fused sum, and scores_append_kernel's fused sum.
#pragma once
#include "head_common.h"

// Host-safe part (the *_host_check.cpp programs build it without HIP).

// M = 2 or 3 and the null test.  M first: it says which of the per-modality pointers p[] are required.  `others`: every other
// required pointer is there.
static inline int eval_check_modalities(const char* who, int M, const float* const* p, bool others) {
  MLA_REQUIRE(M == 2 || M == 3, "%s: need M = 2 or 3 (got %d)", who, M);
  MLA_REQUIRE(p[0] && p[1] && (M != 3 || p[2]) && others, "%s: null pointer", who);
  return MLA_OK;
}

static inline uintptr_t eval_or_ptrs(const float* const* p, int n) {
  uintptr_t words = 0;
  for (int i = 0; i < n; ++i) words |= (uintptr_t)p[i];
  return words;
}

// `words`: every float / int32 pointer or-ed together (a null optional one adds nothing); any 4-byte offset passes (slices of flat
// buffers)
static inline int eval_check_aligned(const char* who, uintptr_t words, const int64_t* labels) {
  MLA_REQUIRE(!(words & 3) && !((uintptr_t)labels & 7), "%s: float / int32 buffers must be 4-byte and labels 8-byte aligned", who);
  return MLA_OK;
}

#ifdef __HIPCC__
__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}

// First slot that holds the row maximum mx (numpy.argmax), a lane holding the slots lane and lane + 64: NaN slots never win, and a
// row in which no slot equals mx (non-finite logits, outside the contract) answers 0: always inside [0, C).
__device__ __forceinline__ int eval_first_max2(float v0, float v1, float mx, int C, int lane) {
  int i = INT_MAX;
  if (lane + 64 < C && v1 == mx) i = lane + 64;
  if (lane < C && v0 == mx) i = lane;
  i = wave_min_i(i);
  return i < C ? i : 0;
}

// The same first maximum by one thread over the C classes of a row, v(c) the value of class c.
template <class V>
__device__ __forceinline__ int eval_scan_first_max(int C, V v) {
  float best = -INFINITY;
  int arg = 0;
  for (int c = 0; c < C; ++c) {
    const float x = v(c);
    if (x > best) { best = x; arg = c; }
  }
  return arg;
}

// The fused value of one class slot, sum_m w[m] * l(m) with the modalities in order, l(m) modality m's logit of the slot.  A plain C
// expression: every call site contracts it the same way.
template <class W, class L>
__device__ __forceinline__ float eval_fused_slot(int M, const W& w, L l) {
  float v = 0.f;
#pragma unroll
  for (int m = 0; m < MLA_HEAD_MAXM; ++m)
    if (m < M) v += w[m] * l(m);
  return v;
}

// A label no counter may be indexed with: the row is counted nowhere.
__device__ __forceinline__ bool eval_bad_label(long lab, int C) { return lab < 0 || lab >= C; }

// Bit k: the row has modality k.  present: (B, M) bytes, or null: every modality present.
__device__ __forceinline__ int eval_present_mask(const uint8_t* present, size_t row, int M) {
  int e = 0;
#pragma unroll
  for (int k = 0; k < MLA_HEAD_MAXM; ++k)
    if (k < M && (!present || present[row * M + k] != 0)) e |= 1 << k;
  return e;
}

// The fixed-alpha weights of a row (main.py:647-651): the alphas as they are when every modality is present, otherwise renormalised
// over what the row has, +0.0 for what it lacks.  False: the remaining share is not > 0, the row is to be counted nowhere and w[]
// is undefined (it was divided by that share).
__device__ __forceinline__ bool eval_fixed_weights(const float* alpha, int mask, int M, float* w) {
  if (mask == (1 << M) - 1) {
#pragma unroll
    for (int k = 0; k < MLA_HEAD_MAXM; ++k) w[k] = k < M ? alpha[k] : 0.f;
    return true;
  }
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < MLA_HEAD_MAXM; ++k)
    if ((mask >> k) & 1) s += alpha[k];
#pragma unroll
  for (int k = 0; k < MLA_HEAD_MAXM; ++k) w[k] = ((mask >> k) & 1) ? alpha[k] / s : 0.f;
  return s > 0.f;
}
#endif
