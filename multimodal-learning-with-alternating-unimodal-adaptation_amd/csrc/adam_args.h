// Host half of mla_adam_step: argument checks, the bias corrections (in double, as torch.optim.Adam computes them) and the split of
// a 4-byte-aligned range into scalar head / 16-byte body / scalar tail.  Plain C++ with no HIP in it, so adam_host_check.cpp
// builds it with the host sanitizers.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "../../include/mla_hip.h"

void mla_set_error(const char* fmt, ...);

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
  if (!p || !m || !v) {
    mla_set_error("mla_adam_step: null pointer");
    return MLA_ERR_INVALID_ARG;
  }
  if (n == 0) {
    mla_set_error("mla_adam_step: n == 0");
    return MLA_ERR_INVALID_ARG;
  }
  if (step < 1) {
    mla_set_error("mla_adam_step: step must be >= 1 (got %d)", step);
    return MLA_ERR_INVALID_ARG;
  }
  const uintptr_t ap = (uintptr_t)p, ag = (uintptr_t)g, am = (uintptr_t)m, av = (uintptr_t)v;
  if ((ap | ag | am | av) & 3) {
    mla_set_error("mla_adam_step: buffers must be 4-byte aligned");
    return MLA_ERR_INVALID_ARG;
  }
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  out->step_size = (float)((double)lr / bc1);
  out->bc2_sqrt = (float)sqrt(bc2);
  size_t head = ((16 - (ap & 15)) & 15) >> 2;
  if (head > n) head = n;
  out->head = head;
  out->vec = ((am & 15) == (ap & 15)) && ((av & 15) == (ap & 15));
  out->gvec = out->vec && (!g || (ag & 15) == (ap & 15));
  out->n4 = out->vec ? (n - head) >> 2 : 0;
  if (!out->vec) out->head = 0;      // scalar launch: one range [0, n)
  return MLA_OK;
}
