// Host half of mla_eval_head (eval_head.hip): argument checks and the launch plan.  Plain C++ with no HIP in it, so
// eval_host_check.cpp builds it with the host sanitizers.
#pragma once
#include "head_common.h"

#define EVAL_ROWS 2             // rows per workgroup: one wave per (row, modality), 64 * M * EVAL_ROWS threads

struct EvalHeadArgs {
  const float* x[MLA_HEAD_MAXM];     // features per modality (B, D)
  const float *W, *bias;             // the shared head (C, D), (C)
  const int64_t* labels;             // (B)
  const uint8_t* present;            // (B, M) or null: every modality present
  int* counts;                       // C * (2 + M), accumulated
  float* logits_out;                 // (M, B, C)
  float* fused_out;                  // (B, C) or null
  float* weights_out;                // (B, M) or null
  int* pred_out;                     // (B, 1 + M) or null
  float alpha[MLA_HEAD_MAXM];
  int M, B, D, C, mode;
};

struct EvalPlan {
  int threads, blocks;               // 64 * M * EVAL_ROWS threads; ceil(B / EVAL_ROWS) workgroups
};

static inline int eval_head_plan(const EvalHeadArgs* a, EvalPlan* out) {
  MLA_REQUIRE(a->M == 2 || a->M == 3, "mla_eval_head: need M = 2 or 3 (got %d)", a->M);      // first: M says which x[] are required
  MLA_REQUIRE(a->x[0] && a->x[1] && (a->M != 3 || a->x[2]) && a->W && a->bias && a->labels && a->counts && a->logits_out,
              "mla_eval_head: null pointer");
  MLA_TRY(head_check_shape("mla_eval_head", a->B, a->D, a->C));
  MLA_REQUIRE(a->mode == 0 || a->mode == 1, "mla_eval_head: need mode = 0 (fixed alphas) or 1 (per-sample entropy gating) (got %d)", a->mode);
  uintptr_t words = (uintptr_t)a->W | (uintptr_t)a->bias | (uintptr_t)a->counts | (uintptr_t)a->logits_out | (uintptr_t)a->fused_out |
                    (uintptr_t)a->weights_out | (uintptr_t)a->pred_out;
  for (int m = 0; m < a->M; ++m) words |= (uintptr_t)a->x[m];
  MLA_REQUIRE(!(words & 3) && !((uintptr_t)a->labels & 7), "mla_eval_head: float / int32 buffers must be 4-byte and labels 8-byte aligned");
  out->threads = 64 * a->M * EVAL_ROWS;
  out->blocks = (int)(((long)a->B + EVAL_ROWS - 1) / EVAL_ROWS);
  return MLA_OK;
}
