// Stand-alone host check of mla_feature_phase's / mla_gather_rows2's argument validation, workspace layout and launch plan
// (feature_args.h) with util.cpp's error reporting.  No GPU, no HIP: `make host-check` builds it with -fsanitize=address,undefined
// and runs it.
#include "feature_args.h"
#include "host_check.h"

int main() {
  alignas(16) static float buf[8][64];
  alignas(16) static int64_t ibuf[4][16];
  float *X = buf[0], *W = buf[1], *m = buf[2], *Pl = buf[3], *lg = buf[4], *loss = buf[5], *ws = buf[6];
  int64_t* lab = ibuf[0];
  FeaturePlan p;
  auto plan = [&](const void* x, const void* l, const void* w, const void* b, const void* mo, const void* pl, const void* lo,
                  const void* ls, const void* wk, int B, int D, int C, int project) {
    return feature_phase_plan(x, l, w, b, mo, pl, lo, ls, wk, B, D, C, project, &p);
  };
  // null pointers, one at a time; Pl may be null only when the projection does not fire
  const void* args[9] = {X, lab, W, W + 8, m, Pl, lg, loss, ws};
  for (int z = 0; z < 9; ++z) {
    const void* a[9];
    memcpy(a, args, sizeof(a));
    a[z] = nullptr;
    EXPECT(plan(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], 2, 4, 2, 1) == MLA_ERR_INVALID_ARG);
    EXPECT(strstr(mla_last_error(), "null pointer"));
  }
  EXPECT(plan(X, lab, W, W + 8, m, nullptr, lg, loss, ws, 2, 4, 2, 0) == MLA_OK);
  // sizes
  EXPECT(plan(X, lab, W, W + 8, m, Pl, lg, loss, ws, 0, 4, 2, 1) == MLA_ERR_INVALID_ARG);
  EXPECT(plan(X, lab, W, W + 8, m, Pl, lg, loss, ws, 2, -1, 2, 1) == MLA_ERR_INVALID_ARG);
  EXPECT(strstr(mla_last_error(), "B, D, C > 0"));
  EXPECT(plan(X, lab, W, W + 8, m, Pl, lg, loss, ws, 2, 4, 0, 1) == MLA_ERR_INVALID_ARG);
  EXPECT(plan(X, lab, W, W + 8, m, Pl, lg, loss, ws, 2, 4, 129, 1) == MLA_ERR_INVALID_ARG);
  EXPECT(strstr(mla_last_error(), "need 0 < C <= 128 (got 129)"));
  EXPECT(plan(X, lab, W, W + 8, m, Pl, lg, loss, ws, 2, 4, 128, 1) == MLA_OK);
  EXPECT(plan(X, lab, W, W + 8, m, Pl, lg, loss, ws, 2, FEATURE_MAXD + 1, 2, 1) == MLA_ERR_INVALID_ARG);
  EXPECT(strstr(mla_last_error(), "need D <="));
  // alignment: the flat bases at 16 bytes, the bias (W + C*D, any C*D) at 4
  EXPECT(plan(X, lab, W + 1, W + 9, m, Pl, lg, loss, ws, 2, 4, 2, 1) == MLA_ERR_INVALID_ARG);
  EXPECT(strstr(mla_last_error(), "16-byte aligned"));
  EXPECT(plan(X, lab, W, W + 8, m + 2, Pl, lg, loss, ws, 2, 4, 2, 1) == MLA_ERR_INVALID_ARG);
  EXPECT(plan(X, lab, W, W + 8, m, Pl + 3, lg, loss, ws, 2, 4, 2, 1) == MLA_ERR_INVALID_ARG);
  EXPECT(plan(X, lab, W, (const char*)(W + 8) + 2, m, Pl, lg, loss, ws, 2, 4, 2, 1) == MLA_ERR_INVALID_ARG);
  EXPECT(strstr(mla_last_error(), "4-byte"));
  EXPECT(plan(X, (const char*)lab + 4, W, W + 8, m, Pl, lg, loss, ws, 2, 4, 2, 1) == MLA_ERR_INVALID_ARG);
  for (int o = 0; o < 4; ++o) EXPECT(plan(X, lab, W, W + 8 + o, m, Pl, lg, loss, ws, 2, 4, 2, 1) == MLA_OK);   // D = 70, C = 65: C*D % 4 = 2
  // the plan: regions tile the workspace in order without overlap and end at mla_feature_ws_elems; every D, multiple of 4 / 64 or not
  const int shapes[][3] = {{64, 512, 101}, {5, 768, 128}, {1, 512, 3}, {8, 70, 65}, {3, 64, 64}, {2, 1, 1}, {7, 257, 2}, {1, 4096, 128}};
  for (const auto& s : shapes)
    for (int project = 0; project < 2; ++project) {
      const int B = s[0], D = s[1], C = s[2];
      EXPECT(plan(X, lab, W, W + 8, m, Pl, lg, loss, ws, B, D, C, project) == MLA_OK);
      EXPECT(p.dlogits == 0 && p.rowloss == (size_t)B * C && p.f64 >= p.rowloss + B && p.f64 < p.rowloss + B + 4 && p.f64 % 4 == 0 &&
             p.G == p.f64 + 6 * (size_t)D);
      EXPECT(p.total == p.G + (size_t)C * D && p.total == feature_ws_elems(B, D, C));
      EXPECT(p.dchunks * 256 >= D && (p.dchunks - 1) * 256 < D && p.grad_blocks == C * p.dchunks);
      EXPECT(project ? (p.k_blocks * FEATURE_KROWS >= D && (p.k_blocks - 1) * FEATURE_KROWS < D) : p.k_blocks == 0);
      EXPECT(p.lds_bytes == (size_t)D * 4 && 2 * p.lds_bytes <= 32768);
    }
  EXPECT(feature_ws_elems(0, 4, 2) == 0 && feature_ws_elems(2, 4, -1) == 0);
  // mla_feature_phase_owm: the same checks and plan under its own name
  const char* owm = "mla_feature_phase_owm";
  REFUSED(feature_phase_plan_for(owm, X, lab, W, W + 8, m, nullptr, lg, loss, ws, 2, 4, 2, 1, &p), "mla_feature_phase_owm: null pointer");
  REFUSED(feature_phase_plan_for(owm, X, lab, W, W + 8, m, Pl, lg, loss, ws, 2, 0, 2, 1, &p), "mla_feature_phase_owm: need B, D, C > 0");
  REFUSED(feature_phase_plan_for(owm, X, lab, W, W + 8, m, Pl, lg, loss, ws, 2, FEATURE_MAXD + 1, 2, 1, &p),
          "mla_feature_phase_owm: need D <= 4096 (got 4097)");
  REFUSED(feature_phase_plan_for(owm, X, lab, W, W + 8, m, Pl + 3, lg, loss, ws, 2, 4, 2, 1, &p), "mla_feature_phase_owm: buffers must be");
  EXPECT(feature_phase_plan_for(owm, X, lab, W, W + 8, m, Pl, lg, loss, ws, 7, 257, 2, 1, &p) == MLA_OK && p.total == feature_ws_elems(7, 257, 2));

  // gather: null pointers, sizes, alignment, and the vector / scalar choice
  int64_t *idx = ibuf[1], *ol = ibuf[2], *oi = ibuf[3];
  float *T0 = buf[0], *T1 = buf[1], *o0 = buf[2], *o1 = buf[3];
  int vec = -1;
  EXPECT(gather_rows2_plan(nullptr, T1, lab, idx, o0, o1, ol, oi, 4, 8, 2, &vec) == MLA_ERR_INVALID_ARG);
  EXPECT(strstr(mla_last_error(), "null pointer"));
  EXPECT(gather_rows2_plan(T0, T1, lab, idx, o0, o1, ol, nullptr, 4, 8, 2, &vec) == MLA_ERR_INVALID_ARG);
  EXPECT(gather_rows2_plan(T0, T1, lab, idx, o0, o1, ol, oi, 0, 8, 2, &vec) == MLA_ERR_INVALID_ARG);
  EXPECT(gather_rows2_plan(T0, T1, lab, idx, o0, o1, ol, oi, 4, 0, 2, &vec) == MLA_ERR_INVALID_ARG);
  EXPECT(gather_rows2_plan(T0, T1, lab, idx, o0, o1, ol, oi, 4, 8, 0, &vec) == MLA_ERR_INVALID_ARG);
  EXPECT(gather_rows2_plan((const char*)T0 + 1, T1, lab, idx, o0, o1, ol, oi, 4, 8, 2, &vec) == MLA_ERR_INVALID_ARG);
  EXPECT(gather_rows2_plan(T0, T1, lab, (const char*)idx + 4, o0, o1, ol, oi, 4, 8, 2, &vec) == MLA_ERR_INVALID_ARG);
  EXPECT(gather_rows2_plan(T0, T1, lab, idx, o0, o1, ol, oi, 4, 8, 2, &vec) == MLA_OK && vec == 1);
  EXPECT(gather_rows2_plan(T0, T1, lab, idx, o0, o1, ol, oi, 4, 70, 2, &vec) == MLA_OK && vec == 0);     // D % 4 != 0
  EXPECT(gather_rows2_plan(T0, T1 + 1, lab, idx, o0, o1, ol, oi, 4, 8, 2, &vec) == MLA_OK && vec == 0);  // a table off 16 bytes
  EXPECT(gather_rows2_plan(T0, T1, lab, idx, o0, o1 + 2, ol, oi, 4, 8, 2, &vec) == MLA_OK && vec == 0);
  // the index range check, where the index is produced
  for (int i = 0; i < 16; ++i) idx[i] = i;
  EXPECT(gather_index_check(idx, 16, 16) == MLA_OK);
  EXPECT(gather_index_check(idx, 16, 15) == MLA_ERR_INVALID_ARG);
  EXPECT(strstr(mla_last_error(), "index 15 at position 15 is outside [0, 15)"));
  idx[3] = -1;
  EXPECT(gather_index_check(idx, 16, 16) == MLA_ERR_INVALID_ARG);
  EXPECT(strstr(mla_last_error(), "index -1 at position 3"));
  EXPECT(gather_index_check(nullptr, 16, 16) == MLA_ERR_INVALID_ARG);
  EXPECT(gather_index_check(idx, 0, 16) == MLA_ERR_INVALID_ARG);
  return host_check_done("feature");
}
