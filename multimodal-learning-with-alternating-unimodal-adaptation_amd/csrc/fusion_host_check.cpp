// Stand-alone host check of the fusion heads' argument validation, workspace layout and gradient-launch block plan (fusion_args.h) with
// util.cpp's error reporting.  No GPU, no HIP: `make host-check` builds it with -fsanitize=address,undefined and runs it.
#include "fusion_args.h"
#include "host_check.h"

int main() {
  alignas(16) static float buf[8][64];
  alignas(16) static int64_t lab[8];
  // shapes: B, D, C > 0; C within the two-slot softmax; D a multiple of 64 up to FUSION_MAXD
  EXPECT(fusion_check_shape("who", 64, 512, 6) == MLA_OK);
  EXPECT(fusion_check_shape("who", 1, 64, 1) == MLA_OK);
  EXPECT(fusion_check_shape("who", 5, 768, MLA_HEAD_MAXC) == MLA_OK);
  EXPECT(fusion_check_shape("who", 5, FUSION_MAXD, 3) == MLA_OK);
  EXPECT(fusion_check_shape("who", 0, 512, 6) == MLA_ERR_INVALID_ARG);
  EXPECT(strstr(mla_last_error(), "who: need B, D, C > 0 (got 0, 512, 6)"));
  EXPECT(fusion_check_shape("who", 4, -64, 6) == MLA_ERR_INVALID_ARG);
  EXPECT(fusion_check_shape("who", 4, 512, 0) == MLA_ERR_INVALID_ARG);
  EXPECT(fusion_check_shape("who", 4, 512, MLA_HEAD_MAXC + 1) == MLA_ERR_INVALID_ARG);
  EXPECT(strstr(mla_last_error(), "need 0 < C <= 128 (got 129)"));
  const int bad_d[] = {1, 63, 65, 70, 100, 257, 320 + 32, FUSION_MAXD + 64};
  for (int d : bad_d) {
    EXPECT(fusion_check_shape("who", 4, d, 6) == MLA_ERR_INVALID_ARG);
    EXPECT(strstr(mla_last_error(), "multiple of 64"));
  }
  // pointers: null and misaligned, one at a time, named by position
  const void* ptrs[4] = {buf[0], buf[1], buf[2] + 1, buf[3]};
  EXPECT(fusion_check_ptrs("who", ptrs, 4) == MLA_OK);
  for (int z = 0; z < 4; ++z) {
    const void* a[4];
    memcpy(a, ptrs, sizeof(a));
    a[z] = nullptr;
    EXPECT(fusion_check_ptrs("who", a, 4) == MLA_ERR_INVALID_ARG);
    char want[64];
    snprintf(want, sizeof(want), "who: null pointer (argument %d)", z);
    EXPECT(strstr(mla_last_error(), want));
    a[z] = (const char*)ptrs[z] + 2;
    EXPECT(fusion_check_ptrs("who", a, 4) == MLA_ERR_INVALID_ARG);
    EXPECT(strstr(mla_last_error(), "4-byte aligned"));
  }
  EXPECT(fusion_check_labels("who", lab) == MLA_OK);
  EXPECT(fusion_check_labels("who", nullptr) == MLA_ERR_INVALID_ARG);
  EXPECT(fusion_check_labels("who", (const char*)lab + 4) == MLA_ERR_INVALID_ARG);
  EXPECT(strstr(mla_last_error(), "8-byte aligned"));

  // workspace: the regions tile it in order without overlap and end at fusion_ws_elems
  const int shapes[][3] = {{64, 512, 6}, {64, 768, 101}, {1, 64, 1}, {5, 320, 65}, {5, 128, 6}, {3, 4096, 128}};
  for (const auto& s : shapes) {
    const int B = s[0], D = s[1], C = s[2];
    const FusionWs w = fusion_ws_layout(B, D, C);
    EXPECT(w.dlogits == 0 && w.rowloss == (size_t)B * C && w.dh == w.rowloss + (size_t)FUSION_NLOSS * B);
    EXPECT(w.total == w.dh + 2 * (size_t)B * D && w.total == fusion_ws_elems(B, D, C));
  }
  EXPECT(fusion_ws_elems(0, 512, 6) == 0 && fusion_ws_elems(4, 512, -1) == 0);

  // the gradient launch: blocks of every job are consecutive, cover (N, K) and (B, K) in 256-column chunks, and add up
  for (const auto& s : shapes) {
    const int B = s[0], D = s[1], C = s[2];
    float *g = buf[0], *in = buf[1], *W = buf[2], *dW = buf[3], *db = buf[4], *din = buf[5];
    FusionJobs js;
    fusion_jobs_init(&js);
    EXPECT(js.n == 0 && js.blocks == 0);
    EXPECT(fusion_jobs_add(&js, g, in, nullptr, dW, db, nullptr, B, C, D) == MLA_OK);         // fc_out: no input gradient
    EXPECT(fusion_jobs_add(&js, g, in, W, dW, db, din, B, 2 * D, D) == MLA_OK);               // FiLM's fc
    EXPECT(fusion_jobs_add(&js, g, in, W, dW, db, din, B, D, D) == MLA_OK);                   // a gated hidden layer
    EXPECT(js.n == 3);
    int next = 0;
    const int N[3] = {C, 2 * D, D};
    for (int i = 0; i < 3; ++i) {
      const FusionJob& j = js.job[i];
      EXPECT(j.first == next && j.N == N[i] && j.K == D);
      EXPECT(j.kchunks * 256 >= D && (j.kchunks - 1) * 256 < D);
      EXPECT(j.w_blocks == N[i] * j.kchunks);
      EXPECT(j.x_blocks == (j.din ? B * j.kchunks : 0));
      next += j.w_blocks + j.x_blocks;
    }
    EXPECT(js.blocks == next && js.job[0].x_blocks == 0);
    EXPECT(fusion_jobs_add(&js, g, in, W, dW, db, din, B, D, D) == MLA_ERR_INVALID_ARG);      // a fourth job
    EXPECT(js.n == 3 && js.blocks == next);
  }
  {
    float *g = buf[0], *in = buf[1], *W = buf[2], *dW = buf[3], *db = buf[4], *din = buf[5];
    FusionJobs js;
    fusion_jobs_init(&js);
    EXPECT(fusion_jobs_add(&js, nullptr, in, W, dW, db, din, 4, 6, 64) == MLA_ERR_INVALID_ARG);
    EXPECT(fusion_jobs_add(&js, g, in, nullptr, dW, db, din, 4, 6, 64) == MLA_ERR_INVALID_ARG);  // an input gradient needs W
    EXPECT(fusion_jobs_add(&js, g, in, W, dW, nullptr, din, 4, 6, 64) == MLA_ERR_INVALID_ARG);
    EXPECT(fusion_jobs_add(&js, g, in, W, dW, db, din, 0, 6, 64) == MLA_ERR_INVALID_ARG);
    EXPECT(fusion_jobs_add(&js, g, in, W, dW, db, din, 4, 0, 64) == MLA_ERR_INVALID_ARG);
    EXPECT(strstr(mla_last_error(), "bad job"));
    EXPECT(js.n == 0 && js.blocks == 0);
  }
  return host_check_done("fusion");
}
