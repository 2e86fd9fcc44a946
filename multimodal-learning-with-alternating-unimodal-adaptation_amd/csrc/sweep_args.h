// Host half of mla_fusion_sweep (fusion_sweep.hip): argument checks and the launch plan.  Plain C++ with no HIP in it, so
// sweep_host_check.cpp builds it with the host sanitizers.
#pragma once
#include "eval_common.h"

#define SWEEP_MAXG 4096                 // grid points of one call: a three-modality lattice at step 1/80 has 3 321
#define SWEEP_LANES 256                 // one lane per grid point: a workgroup owns a tile of SWEEP_LANES grid points ...
#define SWEEP_ROWS 1                    // ... and stages a tile of SWEEP_ROWS rows in LDS.  A lane scans its rows one after the other, a
                                        // latency-bound loop: at (M, B, C, G) = (2, 64, 101, 101) tiles of 4, 2, 1 rows took 45.8, 24.4, 13.6 us
#define SWEEP_MAX_ROW_BLOCKS 256        // grid.x: one workgroup per CU; a workgroup strides over the row tiles past that

struct SweepArgs {
  const float* l[MLA_HEAD_MAXM];        // logits per modality (B, C)
  const int64_t* labels;                // (B)
  const uint8_t* present;               // (B, M) or null: every modality present
  const float* grid;                    // (G, M) on the device
  int *tp, *pp;                         // (G, C) each, accumulated
  int* num;                             // (C), accumulated, or null
  int M, B, C, G;
};

struct SweepPlan {
  int threads;                          // SWEEP_LANES
  int blocks_x;                         // workgroups along the rows: min(row tiles, SWEEP_MAX_ROW_BLOCKS)
  int blocks_y;                         // tiles of grid points: ceil(G / SWEEP_LANES)
  long row_tiles;                       // ceil(B / SWEEP_ROWS)
};

static inline int fusion_sweep_plan(const SweepArgs* a, SweepPlan* out) {
  const char* who = "mla_fusion_sweep";
  MLA_TRY(eval_check_modalities(who, a->M, a->l, a->labels && a->grid && a->tp && a->pp));
  MLA_TRY(head_check_shape(who, a->B, 1, a->C));
  MLA_REQUIRE(a->G > 0 && a->G <= SWEEP_MAXG, "%s: need 0 < G <= %d grid points (got %d)", who, SWEEP_MAXG, a->G);
  const uintptr_t words = (uintptr_t)a->grid | (uintptr_t)a->tp | (uintptr_t)a->pp | (uintptr_t)a->num | eval_or_ptrs(a->l, a->M);
  MLA_TRY(eval_check_aligned(who, words, a->labels));
  out->threads = SWEEP_LANES;
  out->row_tiles = ((long)a->B + SWEEP_ROWS - 1) / SWEEP_ROWS;
  out->blocks_x = (int)(out->row_tiles < SWEEP_MAX_ROW_BLOCKS ? out->row_tiles : SWEEP_MAX_ROW_BLOCKS);
  out->blocks_y = (a->G + SWEEP_LANES - 1) / SWEEP_LANES;
  return MLA_OK;
}
