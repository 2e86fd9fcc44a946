// Host half of mla_gs_project_owm (gs_owm.hip): argument checks, the workspace layout and the launch plan.  Plain C++ with no HIP
// in it, so gs_host_check.cpp builds it with the host sanitizers.
#pragma once
#include "args_common.h"

#define GS_OWM_MAXD 8192        // one row of Pl (fp32) in LDS: 32 KB
#define GS_OWM_WAVES 4          // waves per workgroup of both launches: a wave per row of Pl (A), a wave per class (B)

// Workspace (floats): k (D) | the copy of G (C, D) the projection reads while it writes G in place
struct GsOwmPlan {
  size_t k, G, total;           // offsets into ws (floats), and its size
  int k_blocks;                 // ceil(D / GS_OWM_WAVES) workgroups of launch A; they also copy G, striding over its C * D elements
  size_t lds_bytes;             // D floats
};

static inline size_t gs_owm_ws_elems(int D, int C) {
  if (D <= 0 || C <= 0) return 0;
  return (size_t)D + (size_t)C * D;
}

static inline int gs_owm_plan(const void* Pl, const void* r, const void* G, const void* ws, int D, int C, GsOwmPlan* out) {
  MLA_REQUIRE(Pl && r && G && ws, "mla_gs_project_owm: null pointer");
  MLA_REQUIRE(D > 0 && C > 0, "mla_gs_project_owm: need D, C > 0 (got %d, %d)", D, C);
  MLA_REQUIRE(D <= GS_OWM_MAXD, "mla_gs_project_owm: need D <= %d (got %d): a row of Pl is kept in LDS", GS_OWM_MAXD, D);
  MLA_REQUIRE(!(((uintptr_t)Pl | (uintptr_t)r | (uintptr_t)G | (uintptr_t)ws) & 3), "mla_gs_project_owm: buffers must be 4-byte aligned");
  out->k = 0;
  out->G = (size_t)D;
  out->total = out->G + (size_t)C * D;
  const size_t n = out->total * sizeof(float);
  MLA_REQUIRE(!mla_overlap(ws, n, Pl, (size_t)D * D * sizeof(float)) && !mla_overlap(ws, n, G, (size_t)C * D * sizeof(float)) &&
                  !mla_overlap(ws, n, r, (size_t)D * sizeof(float)),
              "mla_gs_project_owm: the workspace overlaps Pl, r or G");
  out->k_blocks = (D + GS_OWM_WAVES - 1) / GS_OWM_WAVES;
  out->lds_bytes = (size_t)D * sizeof(float);
  return MLA_OK;
}
