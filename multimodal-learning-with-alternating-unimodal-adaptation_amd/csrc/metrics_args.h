// Host halves of the evaluation metrics (metrics.hip): argument checks and launch plans of mla_scores_append,
// mla_average_precision and mla_confusion_count.  Plain C++ with no HIP in it, so metrics_host_check.cpp builds it with the host
// sanitizers.
#pragma once
#include "eval_common.h"

#define METRICS_MAXH 4                  // heads of a store: the fused one, then up to MLA_HEAD_MAXM modalities
#define METRICS_MAXCAP (1 << 26)        // rows of a store: H * cap waves and every (h, row) index stay far inside an int
#define METRICS_WAVES 4                 // waves per workgroup of the wave-per-unit kernels

struct ScoresAppendArgs {
  const float* logits[METRICS_MAXH];    // (B, C) each: fused first, then each modality; logits[0] null when `weights` is given
  const float* weights;                 // null, or H - 1 floats on the device: head 0 is formed as sum_m weights[m] logits[1 + m]
  const int64_t* labels;                // (B)
  float* scores;                        // (H, C, cap), class-major
  int* pred;                            // (H, cap)
  int* labels_out;                      // (cap)
  int H, B, C, pos, cap;
};

struct AvgPrecisionArgs {
  const float* scores;                  // (H, C, cap)
  const int* labels;                    // (cap)
  double* ap;                           // (H, C)
  int* npos;                            // (C)
  double* ws;                           // (H, cap): the per-row terms
  int N, cap, H, C;
};

struct ConfusionArgs {
  const int* pred;                      // (H, cap)
  const int* labels;                    // (cap)
  int* conf;                            // (H, C, C), accumulated
  int N, cap, H, C;
};

struct MetricsPlan {
  int threads, blocks;                  // first launch
  int blocks2;                          // mla_average_precision: the finalize launch (one wave per (h, c))
};

static inline size_t metrics_ws_bytes(int cap, int H) {
  return cap > 0 && H > 0 ? (size_t)cap * (size_t)H * sizeof(double) : 0;
}

// what the three entry points ask of the store's shape
static inline int metrics_check_store(const char* who, int H, int C, int cap) {
  MLA_REQUIRE(H >= 1 && H <= METRICS_MAXH, "%s: need 1 <= H <= %d heads (got %d)", who, METRICS_MAXH, H);
  MLA_TRY(head_check_shape(who, 1, 1, C));
  MLA_REQUIRE(cap > 0 && cap <= METRICS_MAXCAP, "%s: need 0 < cap <= %d rows (got %d)", who, METRICS_MAXCAP, cap);
  return MLA_OK;
}

static inline int metrics_wave_blocks(long waves) { return (int)((waves + METRICS_WAVES - 1) / METRICS_WAVES); }

static inline int scores_append_plan(const ScoresAppendArgs* a, MetricsPlan* out) {
  const char* who = "mla_scores_append";
  MLA_TRY(metrics_check_store(who, a->H, a->C, a->cap));
  MLA_REQUIRE(a->B > 0, "%s: need B > 0 (got %d)", who, a->B);
  MLA_REQUIRE(a->pos >= 0 && (long)a->pos + a->B <= (long)a->cap, "%s: rows %d .. %ld do not fit a store of cap = %d rows", who, a->pos,
              (long)a->pos + a->B - 1, a->cap);
  MLA_REQUIRE(!a->weights || (a->H >= 2 && !a->logits[0]),
              "%s: with a weight vector head 0 is formed from the H - 1 >= 1 modality matrices: pass no fused matrix (H = %d)", who, a->H);
  // no eval_check_modalities: the store has H = 1 .. 4 heads, and which logits[] are required depends on `weights`, not on M alone
  uintptr_t words = (uintptr_t)a->weights | (uintptr_t)a->scores | (uintptr_t)a->pred | (uintptr_t)a->labels_out;
  bool have = a->labels && a->scores && a->pred && a->labels_out;
  for (int h = a->weights ? 1 : 0; h < a->H; ++h) {
    have = have && a->logits[h];
    words |= (uintptr_t)a->logits[h];
  }
  MLA_REQUIRE(have, "%s: null pointer", who);
  MLA_TRY(eval_check_aligned(who, words, a->labels));
  out->threads = 64 * METRICS_WAVES;
  out->blocks = metrics_wave_blocks((long)a->B * a->H);          // one wave per (row, head)
  out->blocks2 = 0;
  return MLA_OK;
}

static inline int metrics_check_rows(const char* who, int N, int cap) {
  MLA_REQUIRE(N > 0 && N <= cap, "%s: need 0 < N <= cap rows (got N = %d, cap = %d)", who, N, cap);
  return MLA_OK;
}

static inline int average_precision_plan(const AvgPrecisionArgs* a, MetricsPlan* out) {
  const char* who = "mla_average_precision";
  MLA_TRY(metrics_check_store(who, a->H, a->C, a->cap));
  MLA_TRY(metrics_check_rows(who, a->N, a->cap));
  MLA_REQUIRE(a->scores && a->labels && a->ap && a->npos && a->ws, "%s: null pointer", who);
  MLA_REQUIRE(!(((uintptr_t)a->scores | (uintptr_t)a->labels | (uintptr_t)a->npos) & 3) && !(((uintptr_t)a->ap | (uintptr_t)a->ws) & 7),
              "%s: float / int32 buffers must be 4-byte and double buffers 8-byte aligned", who);
  out->threads = 64 * METRICS_WAVES;
  out->blocks = metrics_wave_blocks((long)a->N * a->H);          // terms: one wave per (head, row)
  out->blocks2 = metrics_wave_blocks((long)a->H * a->C);         // finalize: one wave per (head, class)
  return MLA_OK;
}

static inline int confusion_plan(const ConfusionArgs* a, MetricsPlan* out) {
  const char* who = "mla_confusion_count";
  MLA_TRY(metrics_check_store(who, a->H, a->C, a->cap));
  MLA_TRY(metrics_check_rows(who, a->N, a->cap));
  MLA_REQUIRE(a->pred && a->labels && a->conf, "%s: null pointer", who);
  MLA_REQUIRE(!(((uintptr_t)a->pred | (uintptr_t)a->labels | (uintptr_t)a->conf) & 3), "%s: int32 buffers must be 4-byte aligned", who);
  out->threads = 256;
  const long units = (long)a->N * a->H, bx = (units + 255) / 256;
  out->blocks = (int)(bx < 1024 ? bx : 1024);                    // one thread per (head, row), grid-stride past 1024 workgroups
  out->blocks2 = 0;
  return MLA_OK;
}
