// Host halves of mla_eval_head and mla_eval_fuse (eval_head.hip): argument checks and the launch plans.  Plain C++ with no HIP in
// it, so eval_host_check.cpp builds it with the host sanitizers.
#pragma once
#include "eval_common.h"

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
  int threads, blocks;               // mla_eval_head: 64 * M * EVAL_ROWS threads, ceil(B / EVAL_ROWS) workgroups; mla_eval_fuse: 256, 1
};

static inline int eval_head_plan(const EvalHeadArgs* a, EvalPlan* out) {
  MLA_TRY(eval_check_modalities("mla_eval_head", a->M, a->x, a->W && a->bias && a->labels && a->counts && a->logits_out));
  MLA_TRY(head_check_shape("mla_eval_head", a->B, a->D, a->C));
  MLA_REQUIRE(a->mode == 0 || a->mode == 1, "mla_eval_head: need mode = 0 (fixed alphas) or 1 (per-sample entropy gating) (got %d)", a->mode);
  const uintptr_t words = (uintptr_t)a->W | (uintptr_t)a->bias | (uintptr_t)a->counts | (uintptr_t)a->logits_out | (uintptr_t)a->fused_out |
                          (uintptr_t)a->weights_out | (uintptr_t)a->pred_out | eval_or_ptrs(a->x, a->M);
  MLA_TRY(eval_check_aligned("mla_eval_head", words, a->labels));
  out->threads = 64 * a->M * EVAL_ROWS;
  out->blocks = (int)(((long)a->B + EVAL_ROWS - 1) / EVAL_ROWS);
  return MLA_OK;
}

// mla_eval_fuse, the published batch-level chain: one workgroup.  labels (B), counts C * (2 + M) and weights_out (M, or null) are
// kernel arguments of their own.
struct EvalFuseArgs {
  const float* out[MLA_HEAD_MAXM];   // logits per modality (B, C)
  float alpha[MLA_HEAD_MAXM];        // fixed fusion weights (used when dynamic == 0)
  int M, B, C, dynamic;
};

static inline int eval_fuse_plan(const EvalFuseArgs* a, const int64_t* labels, const int* counts, EvalPlan* out) {
  MLA_REQUIRE(a->out[0] && a->out[1] && labels && counts && (a->M == 2 || (a->M == 3 && a->out[2])) && a->B > 0 && a->C > 0,
              "mla_eval_fuse: bad argument");
  out->threads = 256;
  out->blocks = 1;
  return MLA_OK;
}
