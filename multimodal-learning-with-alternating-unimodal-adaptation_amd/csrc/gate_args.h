// Host halves of mla_gate_sweep and mla_eval_head_gated (gate_sweep.hip): argument checks, the contract on a gate and the launch
// plans; below them, for the kernels only, the two expressions the gated family w_m ~ a_m exp(-beta H_m) is written on.  The host
// part is plain C++ with no HIP in it, so gate_host_check.cpp builds it with the host sanitizers.
#pragma once
#include <math.h>
#include "eval_args.h"
#include "sweep_args.h"

// The contract on a gate (include/mla_hip.h): hmax - H_k <= ln 128, so x_k <= 16 ln 128 = 77.6 < 88.7 = ln FLT_MAX, and
// 1024 e^77.6 = 5e36 < FLT_MAX / 3: neither g_k nor the three-term sum overflows.
#define GATE_MAX_PRIOR 1024.f
#define GATE_MAX_BETA 16.f
#define GATE_MAX_ROWS 4                 // the largest row tile the sweep kernel is instantiated at (1, 2, 4)

static inline int gate_check_gate(const char* who, const float* prior, float beta, int M) {
  for (int k = 0; k < M; ++k)
    MLA_REQUIRE(isfinite(prior[k]) && prior[k] >= 0.f && prior[k] <= GATE_MAX_PRIOR,
                "%s: need a finite prior%d in [0, %g] (got %g)", who, k, (double)GATE_MAX_PRIOR, (double)prior[k]);
  MLA_REQUIRE(isfinite(beta) && beta >= 0.f && beta <= GATE_MAX_BETA, "%s: need a finite beta in [0, %g] (got %g)", who,
              (double)GATE_MAX_BETA, (double)beta);
  return MLA_OK;
}

struct GateSweepArgs {
  const float* l[MLA_HEAD_MAXM];        // logits per modality (B, C)
  const int64_t* labels;                // (B)
  const uint8_t* present;               // (B, M) or null: every modality present
  const float* grid;                    // (G, M + 1) on the device: a_0 .. a_{M-1}, beta
  int *tp, *pp;                         // (G, C) each, accumulated
  int* num;                             // (C), accumulated, or null
  float* ent_out;                       // (B, M) or null: the entropies the gates were formed from
  int M, B, C, G;
};

// `rows`: the row tile (1, 2 or 4); the plan is fusion_sweep_plan's with that tile
static inline int gate_sweep_plan(const GateSweepArgs* a, int rows, SweepPlan* out) {
  const char* who = "mla_gate_sweep";
  MLA_TRY(eval_check_modalities(who, a->M, a->l, a->labels && a->grid && a->tp && a->pp));
  MLA_TRY(head_check_shape(who, a->B, 1, a->C));
  MLA_REQUIRE(a->G > 0 && a->G <= SWEEP_MAXG, "%s: need 0 < G <= %d gates (got %d)", who, SWEEP_MAXG, a->G);
  MLA_REQUIRE(rows == 1 || rows == 2 || rows == GATE_MAX_ROWS, "%s: need a row tile of 1, 2 or %d (got %d)", who, GATE_MAX_ROWS, rows);
  const uintptr_t words = (uintptr_t)a->grid | (uintptr_t)a->tp | (uintptr_t)a->pp | (uintptr_t)a->num | (uintptr_t)a->ent_out |
                          eval_or_ptrs(a->l, a->M);
  MLA_TRY(eval_check_aligned(who, words, a->labels));
  out->threads = SWEEP_LANES;
  out->row_tiles = ((long)a->B + rows - 1) / rows;
  out->blocks_x = (int)(out->row_tiles < SWEEP_MAX_ROW_BLOCKS ? out->row_tiles : SWEEP_MAX_ROW_BLOCKS);
  out->blocks_y = (a->G + SWEEP_LANES - 1) / SWEEP_LANES;
  return MLA_OK;
}

// mla_eval_head_gated: EvalHeadArgs with alpha[] = the prior (mode is not read) and beta; the plan is mla_eval_head's
static inline int eval_head_gated_plan(const EvalHeadArgs* a, float beta, EvalPlan* out) {
  const char* who = "mla_eval_head_gated";
  MLA_TRY(eval_check_modalities(who, a->M, a->x, a->W && a->bias && a->labels && a->counts && a->logits_out));
  MLA_TRY(head_check_shape(who, a->B, a->D, a->C));
  MLA_TRY(gate_check_gate(who, a->alpha, beta, a->M));
  const uintptr_t words = (uintptr_t)a->W | (uintptr_t)a->bias | (uintptr_t)a->counts | (uintptr_t)a->logits_out | (uintptr_t)a->fused_out |
                          (uintptr_t)a->weights_out | (uintptr_t)a->pred_out | eval_or_ptrs(a->x, a->M);
  MLA_TRY(eval_check_aligned(who, words, a->labels));
  out->threads = 64 * a->M * EVAL_ROWS;
  out->blocks = (int)(((long)a->B + EVAL_ROWS - 1) / EVAL_ROWS);
  return MLA_OK;
}

#ifdef __HIPCC__
// H = - sum_c p_c lp_c of a row of C logits by one wave, every lane gets it: the expression of eval_head_kernel's mode 1, term
// for term (a slot whose exp underflowed to 0 contributes its limit 0, slots past C hold e = 0).
__device__ __forceinline__ float gate_row_entropy(const Softmax2& sm) {
  const float t0 = sm.e0 != 0.f ? (sm.e0 / sm.s) * ((sm.l0 - sm.mx) - sm.logs) : 0.f;
  const float t1 = sm.e1 != 0.f ? (sm.e1 / sm.s) * ((sm.l1 - sm.mx) - sm.logs) : 0.f;
  return 0.f - wave_sum(t0 + t1);
}

// The weights of one (row, gate) pair from the row's entropies H[0..M) (include/mla_hip.h, the rule of the gated family):
// x_k = beta (hmax - H_k), g_k = a_k expf(x_k), s = (float) sum_k (double) g_k, w_k = g_k / s over the eligible modalities (bit k of
// mask), +0.0 for the others.  False: !(s > 0), the pair is left out and w[] is undefined.  At a = 1, beta = 1 both products are
// exact and the weights are eval_head_kernel's mode 1; at beta = 0 with s == 1 they are the priors.
__device__ __forceinline__ bool gate_weights(const float* prior, float beta, const float* H, int mask, int M, float* w) {
  float hmax = -INFINITY;
#pragma unroll
  for (int k = 0; k < MLA_HEAD_MAXM; ++k)
    if (k < M && ((mask >> k) & 1)) hmax = fmaxf(hmax, H[k]);
  float g[MLA_HEAD_MAXM];
  double sum = 0.0;
#pragma unroll
  for (int k = 0; k < MLA_HEAD_MAXM; ++k) {
    const bool el = k < M && ((mask >> k) & 1);
    const float x = beta * (hmax - (el ? H[k] : hmax));
    g[k] = el ? prior[k] * expf(x) : 0.f;
    sum += (double)g[k];
  }
  const float s = (float)sum;
#pragma unroll
  for (int k = 0; k < MLA_HEAD_MAXM; ++k) w[k] = (k < M && ((mask >> k) & 1)) ? g[k] / s : 0.f;
  return s > 0.f;
}
#endif
