// Host half of mla_feature_phase / mla_gather_rows2 (feature_step.hip): argument checks, the workspace layout and the launch
// plan.  Plain C++ with no HIP in it, so feature_host_check.cpp builds it with the host sanitizers.
#pragma once
#include "head_common.h"

#define FEATURE_MAXD 4096       // the feature mean (fp64) / one row of Pl in LDS: 32 KB
#define FEATURE_KROWS 8         // rows of Pl one workgroup of the gradient launch forms k for

// Workspace (floats): dlogits (B, C) | rowloss (B) | pad to 16 bytes | fp64 r (D), k (D), rowsq (D) | G (C, D), the raw head gradient
// of a projecting phase.  mla_feature_phase_owm keeps fp32 r (D), k (D) at the head of the fp64 region and the rest of it unused.
struct FeaturePlan {
  size_t dlogits, rowloss, f64, G, total;            // offsets into ws (floats; f64: the 3 D doubles, 16-byte aligned), and its size
  int dchunks;                                       // ceil(D / 256): column blocks of the weight gradient
  int grad_blocks;                                   // C * dchunks weight-gradient blocks ...
  int k_blocks;                                      // ... + ceil(D / FEATURE_KROWS) blocks for r and k when projecting (else 0)
  size_t lds_bytes;                                  // D floats
};

static inline size_t feature_ws_elems(int B, int D, int C) {
  if (B <= 0 || D <= 0 || C <= 0) return 0;
  return (((size_t)B * C + (size_t)B + 3) & ~(size_t)3) + 6 * (size_t)D + (size_t)C * D;
}

// `who`: the entry point the messages name (mla_feature_phase, or mla_feature_phase_owm: the same arguments, workspace and plan)
static inline int feature_phase_plan_for(const char* who, const void* X, const void* labels, const void* W, const void* b,
                                         const void* buf, const void* Pl, const void* logits, const void* loss, const void* ws, int B,
                                         int D, int C, int project, FeaturePlan* out) {
  MLA_REQUIRE(X && labels && W && b && buf && logits && loss && ws && (!project || Pl), "%s: null pointer", who);
  MLA_TRY(head_check_shape(who, B, D, C));
  MLA_REQUIRE(D <= FEATURE_MAXD, "%s: need D <= %d (got %d)", who, FEATURE_MAXD, D);
  // the flat bases as the allocator hands them out; b = W + C*D and its momentum only need float alignment (C*D is arbitrary)
  MLA_REQUIRE(!(((uintptr_t)X | (uintptr_t)W | (uintptr_t)buf | (uintptr_t)Pl | (uintptr_t)ws | (uintptr_t)logits) & 15),
              "%s: buffers must be 16-byte aligned", who);
  MLA_REQUIRE(!(((uintptr_t)b | (uintptr_t)loss) & 3) && !((uintptr_t)labels & 7),
              "%s: bias / loss must be 4-byte and labels 8-byte aligned", who);
  out->dlogits = 0;
  out->rowloss = (size_t)B * C;
  out->f64 = (out->rowloss + (size_t)B + 3) & ~(size_t)3;
  out->G = out->f64 + 6 * (size_t)D;
  out->total = out->G + (size_t)C * D;
  out->dchunks = (D + 255) / 256;
  out->grad_blocks = C * out->dchunks;
  out->k_blocks = project ? (D + FEATURE_KROWS - 1) / FEATURE_KROWS : 0;
  out->lds_bytes = (size_t)D * sizeof(float);
  return MLA_OK;
}

static inline int feature_phase_plan(const void* X, const void* labels, const void* W, const void* b, const void* buf,
                                     const void* Pl, const void* logits, const void* loss, const void* ws, int B, int D, int C,
                                     int project, FeaturePlan* out) {
  return feature_phase_plan_for("mla_feature_phase", X, labels, W, b, buf, Pl, logits, loss, ws, B, D, C, project, out);
}

// vec: 1 when rows move as 16-byte accesses (D % 4 == 0 and every table / output 16-byte aligned), else the scalar path
static inline int gather_rows2_plan(const void* T0, const void* T1, const void* labels, const void* idx, const void* out0,
                                    const void* out1, const void* out_label, const void* out_idx, long N, int D, int B, int* vec) {
  MLA_REQUIRE(T0 && T1 && labels && idx && out0 && out1 && out_label && out_idx, "mla_gather_rows2: null pointer");
  MLA_REQUIRE(N > 0 && D > 0 && B > 0, "mla_gather_rows2: need N, D, B > 0 (got %ld, %d, %d)", N, D, B);
  MLA_REQUIRE(!(((uintptr_t)T0 | (uintptr_t)T1 | (uintptr_t)out0 | (uintptr_t)out1) & 3) &&
                  !(((uintptr_t)labels | (uintptr_t)idx | (uintptr_t)out_label | (uintptr_t)out_idx) & 7),
              "mla_gather_rows2: tables must be 4-byte and index / label buffers 8-byte aligned");
  *vec = (D % 4 == 0) && !(((uintptr_t)T0 | (uintptr_t)T1 | (uintptr_t)out0 | (uintptr_t)out1) & 15);
  return MLA_OK;
}

// The index vector is produced on the host (the epoch's permutation): refuse anything outside [0, N) before it is uploaded.
static inline int gather_index_check(const int64_t* idx_host, long n, long N) {
  MLA_REQUIRE(idx_host && n > 0 && N > 0, "mla_gather_index_check: bad argument");
  for (long i = 0; i < n; ++i)
    MLA_REQUIRE(idx_host[i] >= 0 && idx_host[i] < N, "mla_gather_index_check: index %ld at position %ld is outside [0, %ld)",
                (long)idx_host[i], i, N);
  return MLA_OK;
}
