// Stand-alone host check of mla_adam_step's argument validation and launch plan (adam_args.h) with util.cpp's error reporting.
// No GPU, no HIP: `make host-check` builds it with -fsanitize=address,undefined and runs it.
#include <math.h>
#include "adam_args.h"
#include "host_check.h"

int main() {
  alignas(16) static float buf[4][64];
  float *p = buf[0], *g = buf[1], *m = buf[2], *v = buf[3];
  AdamPlan pl;
  // invalid arguments: every one answers MLA_ERR_INVALID_ARG with a message, before anything else is looked at
  EXPECT(adam_plan(nullptr, g, m, v, 8, 1e-3f, 0.9f, 0.999f, 1, &pl) == MLA_ERR_INVALID_ARG);
  EXPECT(strstr(mla_last_error(), "null pointer"));
  EXPECT(adam_plan(p, g, nullptr, v, 8, 1e-3f, 0.9f, 0.999f, 1, &pl) == MLA_ERR_INVALID_ARG);
  EXPECT(adam_plan(p, g, m, nullptr, 8, 1e-3f, 0.9f, 0.999f, 1, &pl) == MLA_ERR_INVALID_ARG);
  EXPECT(adam_plan(p, g, m, v, 0, 1e-3f, 0.9f, 0.999f, 1, &pl) == MLA_ERR_INVALID_ARG);
  EXPECT(strstr(mla_last_error(), "n == 0"));
  EXPECT(adam_plan(p, g, m, v, 8, 1e-3f, 0.9f, 0.999f, 0, &pl) == MLA_ERR_INVALID_ARG);
  EXPECT(strstr(mla_last_error(), "step must be >= 1 (got 0)"));
  EXPECT(adam_plan(p, g, m, v, 8, 1e-3f, 0.9f, 0.999f, -7, &pl) == MLA_ERR_INVALID_ARG);
  EXPECT(adam_plan((float*)((char*)p + 2), g, m, v, 8, 1e-3f, 0.9f, 0.999f, 1, &pl) == MLA_ERR_INVALID_ARG);
  EXPECT(strstr(mla_last_error(), "4-byte aligned"));
  // a null gradient is legal (zeroed gradients)
  EXPECT(adam_plan(p, nullptr, m, v, 8, 1e-3f, 0.9f, 0.999f, 1, &pl) == MLA_OK);
  EXPECT(pl.vec == 1 && pl.gvec == 1 && pl.head == 0 && pl.n4 == 2);
  // bias corrections in double
  EXPECT(adam_plan(p, g, m, v, 8, 1e-3f, 0.95f, 0.999f, 3, &pl) == MLA_OK);
  EXPECT(pl.step_size == (float)((double)1e-3f / (1.0 - pow((double)0.95f, 3.0))));
  EXPECT(pl.bc2_sqrt == (float)sqrt(1.0 - pow((double)0.999f, 3.0)));
  // every start offset and length: head + 4 n4 + tail covers [0, n) exactly and the body is 16-byte aligned
  for (int o = 0; o < 4; ++o)
    for (int og = 0; og < 4; ++og)
      for (size_t n = 1; n <= 40; ++n) {
        EXPECT(adam_plan(p + o, g + og, m + o, v + o, n, 1e-3f, 0.9f, 0.999f, 1, &pl) == MLA_OK);
        EXPECT(pl.vec == 1 && pl.gvec == (o == og));
        EXPECT(pl.head <= 3 && pl.head <= n && pl.head + 4 * pl.n4 <= n && n - pl.head - 4 * pl.n4 <= 3);
        EXPECT(pl.n4 == 0 || ((uintptr_t)(p + o + pl.head) & 15) == 0);
      }
  // m off p's alignment: the all-scalar launch
  EXPECT(adam_plan(p + 1, g + 1, m + 2, v + 1, 9, 1e-3f, 0.9f, 0.999f, 1, &pl) == MLA_OK);
  EXPECT(pl.vec == 0 && pl.gvec == 0 && pl.head == 0 && pl.n4 == 0);
  // mla_sgd_step's use of the same split: one state tensor (s1 null), a nullable gradient
  RangePlan rp;
  for (int o = 0; o < 4; ++o)
    for (int og = 0; og < 4; ++og)
      for (size_t n = 1; n <= 40; ++n) {
        EXPECT(range_plan(p + o, g + og, m + o, nullptr, n, &rp));
        EXPECT(rp.vec == 1 && rp.gvec == (o == og) && rp.head <= 3 && rp.head <= n && n - rp.head - 4 * rp.n4 <= 3);
        EXPECT(rp.n4 == 0 || ((uintptr_t)(p + o + rp.head) & 15) == 0);
      }
  EXPECT(range_plan(p + 1, nullptr, m + 1, nullptr, 9, &rp) && rp.vec == 1 && rp.gvec == 1 && rp.head == 3 && rp.n4 == 1);
  EXPECT(range_plan(p + 1, g + 1, m + 3, nullptr, 9, &rp) && rp.vec == 0 && rp.gvec == 0 && rp.head == 0 && rp.n4 == 0);
  EXPECT(!range_plan((float*)((char*)p + 2), g, m, nullptr, 9, &rp) && !range_plan(p, g, (float*)((char*)m + 1), nullptr, 9, &rp));
  return host_check_done("adam");
}
