// Stand-alone host check of the metrics entry points' argument validation and launch plans (metrics_args.h) with util.cpp's error
// reporting.  No GPU, no HIP: `make host-check` builds it with -fsanitize=address,undefined and runs it.
#include <initializer_list>
#include "metrics_args.h"
#include "host_check.h"

int main() {
  alignas(16) static float fbuf[6][64];
  alignas(16) static double dbuf[2][64];
  alignas(16) static int64_t lab64[16];
  alignas(16) static int ibuf[4][64];
  MetricsPlan p;

  // ---- mla_scores_append
  ScoresAppendArgs good;
  memset(&good, 0, sizeof(good));
  for (int h = 0; h < METRICS_MAXH; ++h) good.logits[h] = fbuf[h];
  good.labels = lab64; good.scores = fbuf[4]; good.pred = ibuf[0]; good.labels_out = ibuf[1];
  good.H = 3; good.B = 2; good.C = 2; good.pos = 1; good.cap = 4;
  EXPECT(scores_append_plan(&good, &p) == MLA_OK);
  for (int H : {0, -1, 5}) {
    ScoresAppendArgs a = good;
    a.H = H;
    REFUSED(scores_append_plan(&a, &p), "need 1 <= H <= 4 heads");
  }
  for (int H = 1; H <= 4; ++H) {
    ScoresAppendArgs a = good;
    a.H = H;
    EXPECT(scores_append_plan(&a, &p) == MLA_OK);
    for (int h = 0; h < METRICS_MAXH; ++h) {                  // the first H matrices are required, the others never looked at
      a = good;
      a.H = H;
      a.logits[h] = nullptr;
      if (h < H) REFUSED(scores_append_plan(&a, &p), "mla_scores_append: null pointer");
      else EXPECT(scores_append_plan(&a, &p) == MLA_OK);
    }
  }
  {
    ScoresAppendArgs a = good;
    a.C = MLA_HEAD_MAXC + 1;
    REFUSED(scores_append_plan(&a, &p), "mla_scores_append: need 0 < C <= 128 (got 129)");
    a.C = MLA_HEAD_MAXC;
    EXPECT(scores_append_plan(&a, &p) == MLA_OK);
    a.C = 0;
    REFUSED(scores_append_plan(&a, &p), "B, D, C > 0");
    a = good; a.B = 0;
    REFUSED(scores_append_plan(&a, &p), "need B > 0");
    a = good; a.cap = 0;
    REFUSED(scores_append_plan(&a, &p), "need 0 < cap");
    a = good; a.cap = METRICS_MAXCAP + 1;
    REFUSED(scores_append_plan(&a, &p), "need 0 < cap");
  }
  // the row range: pos .. pos + B - 1 inside [0, cap), without int overflow
  for (int pos : {0, 1, 2}) {
    ScoresAppendArgs a = good;
    a.pos = pos;
    EXPECT(scores_append_plan(&a, &p) == MLA_OK);
  }
  {
    ScoresAppendArgs a = good;
    a.pos = 3;
    REFUSED(scores_append_plan(&a, &p), "rows 3 .. 4 do not fit a store of cap = 4 rows");
    a.pos = -1;
    REFUSED(scores_append_plan(&a, &p), "do not fit");
    a.pos = METRICS_MAXCAP; a.cap = METRICS_MAXCAP; a.B = 0x7fffffff;
    REFUSED(scores_append_plan(&a, &p), "do not fit");
  }
  // the weight vector: head 0 is formed, not passed
  {
    ScoresAppendArgs a = good;
    a.weights = fbuf[5]; a.logits[0] = nullptr;
    EXPECT(scores_append_plan(&a, &p) == MLA_OK);
    a.logits[0] = fbuf[0];
    REFUSED(scores_append_plan(&a, &p), "pass no fused matrix");
    a.logits[0] = nullptr; a.H = 1;
    REFUSED(scores_append_plan(&a, &p), "pass no fused matrix");
    a.H = 3; a.logits[2] = nullptr;
    REFUSED(scores_append_plan(&a, &p), "null pointer");
    a = good; a.weights = (const float*)((const char*)fbuf[5] + 2); a.logits[0] = nullptr;
    REFUSED(scores_append_plan(&a, &p), "4-byte");
  }
  {
    ScoresAppendArgs a = good;
    a.labels = nullptr;
    REFUSED(scores_append_plan(&a, &p), "null pointer");
    a = good; a.scores = nullptr;
    REFUSED(scores_append_plan(&a, &p), "null pointer");
    a = good; a.pred = nullptr;
    REFUSED(scores_append_plan(&a, &p), "null pointer");
    a = good; a.labels_out = nullptr;
    REFUSED(scores_append_plan(&a, &p), "null pointer");
    a = good; a.labels = (const int64_t*)((const char*)lab64 + 4);
    REFUSED(scores_append_plan(&a, &p), "8-byte");
    a = good; a.scores = (float*)((char*)fbuf[4] + 2);
    REFUSED(scores_append_plan(&a, &p), "4-byte");
    a = good; a.scores = fbuf[4] + 1;
    EXPECT(scores_append_plan(&a, &p) == MLA_OK);
  }
  // the plan: one wave per (row, head), every unit covered once
  for (int H = 1; H <= 4; ++H)
    for (int B : {1, 2, 3, 5, 64, 65, 22716}) {
      ScoresAppendArgs a = good;
      a.H = H; a.B = B; a.pos = 0; a.cap = 22716;
      EXPECT(scores_append_plan(&a, &p) == MLA_OK);
      EXPECT(p.threads == 64 * METRICS_WAVES && p.threads <= 1024);
      EXPECT((long)p.blocks * METRICS_WAVES >= (long)B * H && (long)(p.blocks - 1) * METRICS_WAVES < (long)B * H);
    }

  // ---- mla_average_precision
  AvgPrecisionArgs ag;
  memset(&ag, 0, sizeof(ag));
  ag.scores = fbuf[0]; ag.labels = ibuf[0]; ag.ap = dbuf[0]; ag.npos = ibuf[1]; ag.ws = dbuf[1];
  ag.N = 3; ag.cap = 4; ag.H = 2; ag.C = 2;
  EXPECT(average_precision_plan(&ag, &p) == MLA_OK);
  EXPECT(p.blocks == 2 && p.blocks2 == 1);
  for (int H : {0, 5}) {
    AvgPrecisionArgs a = ag;
    a.H = H;
    REFUSED(average_precision_plan(&a, &p), "mla_average_precision: need 1 <= H <= 4 heads");
  }
  {
    AvgPrecisionArgs a = ag;
    a.C = 129;
    REFUSED(average_precision_plan(&a, &p), "mla_average_precision: need 0 < C <= 128 (got 129)");
    a = ag; a.N = 5;
    REFUSED(average_precision_plan(&a, &p), "need 0 < N <= cap rows (got N = 5, cap = 4)");
    a = ag; a.N = 0;
    REFUSED(average_precision_plan(&a, &p), "need 0 < N <= cap");
    a = ag; a.N = 4;
    EXPECT(average_precision_plan(&a, &p) == MLA_OK);
    for (int f = 0; f < 5; ++f) {
      a = ag;
      (f == 0 ? *(const void**)&a.scores : f == 1 ? *(const void**)&a.labels : f == 2 ? *(const void**)&a.ap
       : f == 3 ? *(const void**)&a.npos : *(const void**)&a.ws) = nullptr;
      REFUSED(average_precision_plan(&a, &p), "mla_average_precision: null pointer");
    }
    a = ag; a.ws = (double*)((char*)dbuf[1] + 4);
    REFUSED(average_precision_plan(&a, &p), "8-byte");
    a = ag; a.ap = (double*)((char*)dbuf[0] + 4);
    REFUSED(average_precision_plan(&a, &p), "8-byte");
    a = ag; a.scores = (const float*)((const char*)fbuf[0] + 2);
    REFUSED(average_precision_plan(&a, &p), "4-byte");
  }
  for (int H = 1; H <= 4; ++H)
    for (int N : {1, 63, 64, 65, 744, 22716})
      for (int C : {1, 6, 101, 128}) {
        AvgPrecisionArgs a = ag;
        a.H = H; a.N = N; a.cap = N + 3; a.C = C;
        EXPECT(average_precision_plan(&a, &p) == MLA_OK);
        EXPECT((long)p.blocks * METRICS_WAVES >= (long)N * H && (long)(p.blocks - 1) * METRICS_WAVES < (long)N * H);
        EXPECT(p.blocks2 * METRICS_WAVES >= H * C && (p.blocks2 - 1) * METRICS_WAVES < H * C);
      }
  EXPECT(metrics_ws_bytes(4, 2) == 64 && metrics_ws_bytes(0, 2) == 0 && metrics_ws_bytes(4, 0) == 0);
  EXPECT(metrics_ws_bytes(METRICS_MAXCAP, METRICS_MAXH) == (size_t)METRICS_MAXCAP * METRICS_MAXH * 8);

  // ---- mla_confusion_count
  ConfusionArgs cg;
  memset(&cg, 0, sizeof(cg));
  cg.pred = ibuf[0]; cg.labels = ibuf[1]; cg.conf = ibuf[2];
  cg.N = 3; cg.cap = 4; cg.H = 2; cg.C = 2;
  EXPECT(confusion_plan(&cg, &p) == MLA_OK);
  EXPECT(p.blocks == 1 && p.threads == 256);
  {
    ConfusionArgs a = cg;
    a.H = 0;
    REFUSED(confusion_plan(&a, &p), "mla_confusion_count: need 1 <= H <= 4 heads");
    a.H = 5;
    REFUSED(confusion_plan(&a, &p), "mla_confusion_count: need 1 <= H <= 4 heads");
    a = cg; a.C = 129;
    REFUSED(confusion_plan(&a, &p), "mla_confusion_count: need 0 < C <= 128 (got 129)");
    a = cg; a.N = 5;
    REFUSED(confusion_plan(&a, &p), "need 0 < N <= cap rows");
    a = cg; a.pred = nullptr;
    REFUSED(confusion_plan(&a, &p), "mla_confusion_count: null pointer");
    a = cg; a.labels = nullptr;
    REFUSED(confusion_plan(&a, &p), "mla_confusion_count: null pointer");
    a = cg; a.conf = nullptr;
    REFUSED(confusion_plan(&a, &p), "mla_confusion_count: null pointer");
    a = cg; a.conf = (int*)((char*)ibuf[2] + 2);
    REFUSED(confusion_plan(&a, &p), "4-byte");
    a = cg; a.N = METRICS_MAXCAP; a.cap = METRICS_MAXCAP; a.H = 4;
    EXPECT(confusion_plan(&a, &p) == MLA_OK);
    EXPECT(p.blocks == 1024);
  }
  return host_check_done("metrics");
}
