// The one Linear head + cross entropy every head family is written on: the shared head (head_gs_sgd.hip), the concat head
// (concat_head.hip), the QMF heads (qmf_head.hip) and the fused feature phase (feature_step.hip).  Their logits, losses and
// losses agree bit for bit because each sum below exists once, in one order.
// Not here: the two row-sequential gradient loops, dW[c][d] = sum_r dl[r][c] x[r][d] (rows in order) and dX[d] = sum_c dl[c] W[c][d]
// (classes in order).  They stay written out in their kernels: as inlined functions the loops compile to other instruction streams
// than the kernels had (scripts/head_isa.py), and the shared head's pair of weight-gradient kernels shares them through
// head_dw_block (head_gs_sgd.hip) instead.
#pragma once

// Host-safe part (feature_args.h builds without HIP).
#include "args_common.h"

#define MLA_HEAD_MAXC 128       // classes: the two-slot softmax holds a row of logits in one wave, two per lane
#define MLA_HEAD_MAXM 3         // modalities

// the shape rule of every head that holds a row of logits in the two-slot softmax (eval_args.h, feature_args.h, fusion_args.h)
static inline int head_check_shape(const char* who, int B, int D, int C) {
  MLA_REQUIRE(B > 0 && D > 0 && C > 0, "%s: need B, D, C > 0 (got %d, %d, %d)", who, B, D, C);
  MLA_REQUIRE(C <= MLA_HEAD_MAXC, "%s: need 0 < C <= %d (got %d)", who, MLA_HEAD_MAXC, C);
  return MLA_OK;
}

#ifdef __HIPCC__
#include "common.h"

// x . w by ONE wave, lanes striding the features; every lane gets the sum.  The caller adds the bias.
__device__ __forceinline__ float head_row_dot(const float* x, const float* w, int D, int lane) {
  float s = 0.f;
  for (int d = lane; d < D; d += 64) s += x[d] * w[d];
  return wave_sum(s);
}

// Softmax of a row of C <= MLA_HEAD_MAXC logits by one wave: lane holds the slots lane and lane + 64 (-inf / 0 past C).
struct Softmax2 {
  float l0, l1, e0, e1, s, mx, logs;      // mx: the row maximum; s = sum exp(l - mx); logs = logf(s)
};
__device__ __forceinline__ Softmax2 head_softmax2(const float* l, int C, int lane) {
  Softmax2 r;
  r.l0 = lane < C ? l[lane] : -INFINITY;
  r.l1 = lane + 64 < C ? l[lane + 64] : -INFINITY;
  r.mx = wave_max(fmaxf(r.l0, r.l1));
  r.e0 = lane < C ? expf(r.l0 - r.mx) : 0.f;
  r.e1 = lane + 64 < C ? expf(r.l1 - r.mx) : 0.f;
  r.s = wave_sum(r.e0 + r.e1);
  r.logs = logf(r.s);
  return r;
}

// -log softmax(l)[label] of a row with maximum mx and logs = log sum exp(l - mx), as log_softmax forms it: both terms are of the
// size of the loss.  (mx + logs) - l_label rounds at the size of the LOGITS instead: at logits near -1e4 and a loss near 1 that is
// an error of 1e-4 of the loss (tests/test_head_exact_gpu.py, the `low` family).
__device__ __forceinline__ float head_ce_loss(float logs, float mx, float l_label) { return logs - (l_label - mx); }

// d CE / d logit of one slot (mean reduction).  What a bad label does to the row is the caller's policy.
__device__ __forceinline__ float head_ce_grad(float e, float s, bool hit, float inv_batch) {
  return (e / s - (hit ? 1.f : 0.f)) * inv_batch;
}

// sum_r v[r * stride + col] over n rows by the first wave of a workgroup (tid < 64): 64-strided rows, then the wave reduction.
// The bias gradient (v = dl, stride C, col c) and every loss sum (stride 1, col 0).
__device__ __forceinline__ float head_col_sum(const float* v, int n, int stride, int col, int tid) {
  float a = 0.f;
  for (int r = tid; r < n; r += 64) a += v[(size_t)r * stride + col];
  return wave_sum(a);
}

// torch.optim.SGD on one element
__device__ __forceinline__ void sgd_elem(float* __restrict__ p, float* __restrict__ buf, float g, float lr, float momentum, float wd,
                                         int first) {
  const float pv = *p;
  const float d = g + wd * pv;
  const float b = first ? d : momentum * *buf + d;
  *buf = b;
  *p = pv - lr * b;
}
#endif
