// Stand-alone host check of mla_gs_project_owm's argument validation, workspace layout and launch plan (gs_args.h) with util.cpp's
// error reporting.  No GPU, no HIP: `make host-check` builds it with -fsanitize=address,undefined and runs it.
#include "gs_args.h"
#include "host_check.h"

int main() {
  alignas(16) static float buf[4][64];
  float *Pl = buf[0], *r = buf[1], *G = buf[2], *ws = buf[3];
  GsOwmPlan p;
  // D = 4, C = 3: Pl 16, r 4, G 12 and ws 16 floats, each inside its own 64-float row
  EXPECT(gs_owm_plan(Pl, r, G, ws, 4, 3, &p) == MLA_OK);
  // null pointers, one at a time
  const void* args[4] = {Pl, r, G, ws};
  for (int z = 0; z < 4; ++z) {
    const void* a[4];
    memcpy(a, args, sizeof(a));
    a[z] = nullptr;
    REFUSED(gs_owm_plan(a[0], a[1], a[2], a[3], 4, 3, &p), "mla_gs_project_owm: null pointer");
  }
  // sizes
  REFUSED(gs_owm_plan(Pl, r, G, ws, 0, 3, &p), "need D, C > 0 (got 0, 3)");
  REFUSED(gs_owm_plan(Pl, r, G, ws, -1, 3, &p), "need D, C > 0");
  REFUSED(gs_owm_plan(Pl, r, G, ws, 4, 0, &p), "need D, C > 0 (got 4, 0)");
  REFUSED(gs_owm_plan(Pl, r, G, ws, GS_OWM_MAXD + 1, 3, &p), "need D <= 8192 (got 8193)");
  EXPECT((size_t)GS_OWM_MAXD * sizeof(float) <= 32768);
  // alignment
  REFUSED(gs_owm_plan((const char*)Pl + 2, r, G, ws, 4, 3, &p), "4-byte aligned");
  REFUSED(gs_owm_plan(Pl, r, G, (const char*)ws + 1, 4, 3, &p), "4-byte aligned");
  EXPECT(gs_owm_plan(Pl + 1, r + 3, G + 1, ws + 1, 4, 3, &p) == MLA_OK);
  // the workspace may share no byte with Pl, r or G: the projection reads its copy of G while it writes G
  REFUSED(gs_owm_plan(Pl, r, G, Pl + 15, 4, 3, &p), "overlaps");
  REFUSED(gs_owm_plan(Pl, r, G, r + 3, 4, 3, &p), "overlaps");
  REFUSED(gs_owm_plan(Pl, r, G, G + 11, 4, 3, &p), "overlaps");
  REFUSED(gs_owm_plan(Pl, r, ws + 15, ws, 4, 3, &p), "overlaps");
  EXPECT(gs_owm_plan(Pl, r, ws + 16, ws, 4, 3, &p) == MLA_OK);           // ... and may touch them
  // the plan: k then the copy of G, ending at mla_gs_owm_ws_elems; one wave of launch A per row of Pl
  const int shapes[][2] = {{1, 1}, {4, 1}, {63, 3}, {64, 4}, {65, 5}, {70, 130}, {257, 101}, {768, 101}, {8192, 128}};
  const float* far = reinterpret_cast<const float*>((uintptr_t)1 << 40);     // never dereferenced
  for (const auto& s : shapes) {
    const int D = s[0], C = s[1];
    EXPECT(gs_owm_plan(Pl, r, G, far, D, C, &p) == MLA_OK);
    EXPECT(p.k == 0 && p.G == (size_t)D && p.total == (size_t)D + (size_t)C * D && p.total == gs_owm_ws_elems(D, C));
    EXPECT(p.k_blocks * GS_OWM_WAVES >= D && (p.k_blocks - 1) * GS_OWM_WAVES < D);
    EXPECT(p.lds_bytes == (size_t)D * 4 && p.lds_bytes <= 32768);
  }
  EXPECT(gs_owm_ws_elems(0, 3) == 0 && gs_owm_ws_elems(4, -1) == 0);
  return host_check_done("gs");
}
