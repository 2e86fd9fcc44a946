// Host half of the sum / FiLM / gated fusion heads (fusion_head.hip): argument checks, the workspace layout and the block plan of
// the gradient launch.  Plain C++ with no HIP in it, so fusion_host_check.cpp builds it with the host sanitizers.
#pragma once
#include "head_common.h"

#define FUSION_MAXD 4096        // one row of the fused feature z in LDS: 16 KB
#define FUSION_MAXJOBS 3        // Linear layers of one head: gated has fc_x, fc_y, fc_out
#define FUSION_NLOSS 3          // loss rows: the training loss, then (sum only) the reported losses of out_a and out_v

// Workspace (floats): dlogits (B, C) | rowloss (FUSION_NLOSS, B) | dh (B, 2 D), the gradient at the hidden Linear outputs
// (FiLM: d(gamma | beta); gated: dhx (B, D) then dhy (B, D); sum: unused).  One size for the three methods.
struct FusionWs {
  size_t dlogits, rowloss, dh, total;
};

static inline size_t fusion_ws_elems(int B, int D, int C) {
  if (B <= 0 || D <= 0 || C <= 0) return 0;
  return (size_t)B * C + (size_t)FUSION_NLOSS * B + 2 * (size_t)B * D;
}

static inline FusionWs fusion_ws_layout(int B, int D, int C) {
  FusionWs w;
  w.dlogits = 0;
  w.rowloss = (size_t)B * C;
  w.dh = w.rowloss + (size_t)FUSION_NLOSS * B;
  w.total = w.dh + 2 * (size_t)B * D;
  return w;
}

// Shapes every entry point accepts: D a multiple of 64 (the 64-lane dot products have no tail and a 256-column block never straddles
// the gamma | beta boundary of FiLM's hidden layer), C within the two-slot softmax.
static inline int fusion_check_shape(const char* who, int B, int D, int C) {
  MLA_TRY(head_check_shape(who, B, D, C));
  MLA_REQUIRE(D % 64 == 0 && D <= FUSION_MAXD, "%s: need D a multiple of 64 and D <= %d (got %d)", who, FUSION_MAXD, D);
  return MLA_OK;
}

static inline int fusion_check_ptrs(const char* who, const void* const* ptrs, int n) {
  for (int i = 0; i < n; ++i) {
    MLA_REQUIRE(ptrs[i], "%s: null pointer (argument %d)", who, i);
    MLA_REQUIRE(!((uintptr_t)ptrs[i] & 3), "%s: argument %d is not 4-byte aligned", who, i);
  }
  return MLA_OK;
}

static inline int fusion_check_labels(const char* who, const void* labels) {
  MLA_REQUIRE(labels && !((uintptr_t)labels & 7), "%s: labels must be a non-null 8-byte aligned int64 buffer", who);
  return MLA_OK;
}

// One Linear layer's backward in the gradient launch: g (B, N) the gradient at its output, in (B, K) its input, W (N, K).
// Blocks [first, first + w_blocks): dW (N, K) = g^T in, one block per (n, 256 columns of K); the first of them per n also db[n].
// Blocks [first + w_blocks, first + w_blocks + x_blocks): din (B, K) = g W, one block per (row, 256 columns); none when din is null.
struct FusionJob {
  const float* g;
  const float* in;
  const float* W;
  float* dW;
  float* db;
  float* din;
  int N, K;
  int first, w_blocks, x_blocks, kchunks;
};

struct FusionJobs {
  FusionJob job[FUSION_MAXJOBS];
  int n, blocks;
};

static inline void fusion_jobs_init(FusionJobs* js) {
  js->n = 0;
  js->blocks = 0;
}

static inline int fusion_jobs_add(FusionJobs* js, const float* g, const float* in, const float* W, float* dW, float* db, float* din,
                                  int B, int N, int K) {
  MLA_REQUIRE(js->n < FUSION_MAXJOBS && g && in && dW && db && (!din || W) && B > 0 && N > 0 && K > 0, "fusion_jobs_add: bad job");
  FusionJob* j = &js->job[js->n++];
  j->g = g; j->in = in; j->W = W; j->dW = dW; j->db = db; j->din = din;
  j->N = N; j->K = K;
  j->kchunks = (K + 255) / 256;
  j->first = js->blocks;
  j->w_blocks = N * j->kchunks;
  j->x_blocks = din ? B * j->kchunks : 0;
  js->blocks += j->w_blocks + j->x_blocks;
  return MLA_OK;
}
