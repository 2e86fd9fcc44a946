// Host half of mla_adam_step: argument checks, the bias corrections (in double, as torch.optim.Adam computes them) and the split of
// a 4-byte-aligned range into scalar head / 16-byte body / scalar tail (range_plan, which mla_sgd_step plans with too).  Plain C++
// with no HIP in it, so adam_host_check.cpp builds it with the host sanitizers.
#pragma once
#include <math.h>
#include "args_common.h"

// The split of one flat range for a float4 kernel, shared by mla_adam_step and mla_sgd_step: `p` is the written tensor that sets the
// 16-byte grid, s0 and s1 (s1 nullable) are the state tensors walked with it, g (nullable) the gradient.
struct RangePlan {
  size_t head;         // leading elements before p reaches a 16-byte boundary (all of n when n is shorter)
  size_t n4;           // float4 groups of the body
  int vec;             // 1: p and the state reach 16-byte alignment together (the body runs on float4); 0: all-scalar launch
  int gvec;            // 1: g is aligned with p as well (float4 gradient loads)
};

// False when a pointer is not 4-byte aligned (nothing is planned then).
static inline bool range_plan(const float* p, const float* g, const float* s0, const float* s1, size_t n, RangePlan* out) {
  const uintptr_t ap = (uintptr_t)p, ag = (uintptr_t)g, a0 = (uintptr_t)s0, a1 = s1 ? (uintptr_t)s1 : ap;
  if ((ap | ag | a0 | a1) & 3) return false;
  size_t head = ((16 - (ap & 15)) & 15) >> 2;
  if (head > n) head = n;
  out->head = head;
  out->vec = ((a0 & 15) == (ap & 15)) && ((a1 & 15) == (ap & 15));
  out->gvec = out->vec && (!g || (ag & 15) == (ap & 15));
  out->n4 = out->vec ? (n - head) >> 2 : 0;
  if (!out->vec) out->head = 0;      // scalar launch: one range [0, n)
  return true;
}

struct AdamPlan {
  float step_size;     // lr / (1 - beta1^step)
  float bc2_sqrt;      // sqrt(1 - beta2^step)
  size_t head;         // leading elements before p reaches a 16-byte boundary (all of n when n is shorter)
  size_t n4;           // float4 groups of the body
  int vec;             // 1: p, m and v reach 16-byte alignment together (the body runs on float4); 0: all-scalar launch
  int gvec;            // 1: g is aligned with p as well (float4 gradient loads)
};

static inline int adam_plan(const float* p, const float* g, const float* m, const float* v, size_t n, float lr, float beta1,
                            float beta2, int step, AdamPlan* out) {
  MLA_REQUIRE(p && m && v, "mla_adam_step: null pointer");
  MLA_REQUIRE(n != 0, "mla_adam_step: n == 0");
  MLA_REQUIRE(step >= 1, "mla_adam_step: step must be >= 1 (got %d)", step);
  RangePlan r;
  MLA_REQUIRE(range_plan(p, g, m, v, n, &r), "mla_adam_step: buffers must be 4-byte aligned");
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  out->step_size = (float)((double)lr / bc1);
  out->bc2_sqrt = (float)sqrt(bc2);
  out->head = r.head;
  out->n4 = r.n4;
  out->vec = r.vec;
  out->gvec = r.gvec;
  return MLA_OK;
}
