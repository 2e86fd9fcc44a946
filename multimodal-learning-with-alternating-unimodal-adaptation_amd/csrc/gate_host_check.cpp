// Stand-alone host check of mla_gate_sweep's and mla_eval_head_gated's argument validation, the contract on a gate and the launch
// plans (gate_args.h) with util.cpp's error reporting.
// No GPU, no HIP: `make host-check` builds it with -fsanitize=address,undefined and runs it.
#include <float.h>
#include <initializer_list>
#include "gate_args.h"
#include "host_check.h"

int main() {
  alignas(16) static float fbuf[9][64];
  alignas(16) static int64_t lab64[16];
  alignas(16) static int ibuf[3][64];
  alignas(16) static uint8_t have[64];
  SweepPlan p;

  // ---- the contract on a gate: the caps keep every intermediate finite in fp32 at the largest entropy gap, ln 128
  {
    const float xmax = GATE_MAX_BETA * logf((float)MLA_HEAD_MAXC);
    EXPECT(xmax < logf(FLT_MAX));
    const float gmax = GATE_MAX_PRIOR * expf(xmax);
    EXPECT(isfinite(gmax) && (double)gmax * MLA_HEAD_MAXM < (double)FLT_MAX);
    const float good[3] = {0.f, GATE_MAX_PRIOR, 0.55f};
    EXPECT(gate_check_gate("who", good, 0.f, 3) == MLA_OK && gate_check_gate("who", good, GATE_MAX_BETA, 3) == MLA_OK);
    for (float v : {-1e-30f, -1.f, nextafterf(GATE_MAX_PRIOR, INFINITY), INFINITY, -INFINITY, NAN})
      for (int k = 0; k < 3; ++k) {
        float pr[3] = {1.f, 1.f, 1.f};
        pr[k] = v;
        REFUSED(gate_check_gate("who", pr, 1.f, 3), "who: need a finite prior");
        if (k == 2) EXPECT(gate_check_gate("who", pr, 1.f, 2) == MLA_OK);      // not read with two modalities
      }
    for (float v : {-1e-30f, -1.f, nextafterf(GATE_MAX_BETA, INFINITY), INFINITY, NAN})
      REFUSED(gate_check_gate("who", good, v, 3), "who: need a finite beta in [0, 16]");
    EXPECT(gate_check_gate("who", good, -0.f, 3) == MLA_OK);
  }

  // ---- mla_gate_sweep
  GateSweepArgs good;
  memset(&good, 0, sizeof(good));
  for (int m = 0; m < MLA_HEAD_MAXM; ++m) good.l[m] = fbuf[m];
  good.labels = lab64; good.present = have; good.grid = fbuf[3]; good.ent_out = fbuf[4];
  good.tp = ibuf[0]; good.pp = ibuf[1]; good.num = ibuf[2];
  good.M = 3; good.B = 5; good.C = 6; good.G = 7;
  EXPECT(gate_sweep_plan(&good, 1, &p) == MLA_OK);
  EXPECT(p.threads == SWEEP_LANES && p.blocks_x == 5 && p.blocks_y == 1 && p.row_tiles == 5);
  for (int rows : {-1, 0, 3, 5, 8}) REFUSED(gate_sweep_plan(&good, rows, &p), "mla_gate_sweep: need a row tile of 1, 2 or 4");

  for (int M : {-1, 0, 1, 4}) {
    GateSweepArgs a = good;
    a.M = M;
    REFUSED(gate_sweep_plan(&a, 1, &p), "mla_gate_sweep: need M = 2 or 3");
  }
  // the required pointers: l2 only with three modalities; present, num and ent_out may be null
  for (int M : {2, 3})
    for (int f = 0; f < 10; ++f) {
      GateSweepArgs a = good;
      a.M = M;
      const void** field = f < 3 ? (const void**)&a.l[f] : f == 3 ? (const void**)&a.labels : f == 4 ? (const void**)&a.grid
                         : f == 5 ? (const void**)&a.tp : f == 6 ? (const void**)&a.pp : f == 7 ? (const void**)&a.present
                         : f == 8 ? (const void**)&a.num : (const void**)&a.ent_out;
      *field = nullptr;
      if (f >= 7 || (f == 2 && M == 2)) EXPECT(gate_sweep_plan(&a, 1, &p) == MLA_OK);
      else REFUSED(gate_sweep_plan(&a, 1, &p), "mla_gate_sweep: null pointer");
    }
  {
    GateSweepArgs a = good;
    a.B = 0;
    REFUSED(gate_sweep_plan(&a, 1, &p), "mla_gate_sweep: need B, D, C > 0");
    a.B = -3;
    REFUSED(gate_sweep_plan(&a, 1, &p), "need B, D, C > 0");
    a = good; a.C = 0;
    REFUSED(gate_sweep_plan(&a, 1, &p), "need B, D, C > 0");
    a.C = MLA_HEAD_MAXC + 1;
    REFUSED(gate_sweep_plan(&a, 1, &p), "mla_gate_sweep: need 0 < C <= 128 (got 129)");
    a.C = MLA_HEAD_MAXC;
    EXPECT(gate_sweep_plan(&a, 1, &p) == MLA_OK);
    a = good; a.G = 0;
    REFUSED(gate_sweep_plan(&a, 1, &p), "mla_gate_sweep: need 0 < G <= 4096 gates (got 0)");
    a.G = -1;
    REFUSED(gate_sweep_plan(&a, 1, &p), "need 0 < G <= 4096");
    a.G = SWEEP_MAXG + 1;
    REFUSED(gate_sweep_plan(&a, 1, &p), "need 0 < G <= 4096 gates (got 4097)");
    a.G = SWEEP_MAXG;
    EXPECT(gate_sweep_plan(&a, 1, &p) == MLA_OK);
  }
  // alignment: every float / int32 buffer the call reads or writes, l2 only when it is read
  for (int f = 0; f < 9; ++f) {
    GateSweepArgs a = good;
    const char** field = f < 3 ? (const char**)&a.l[f] : f == 3 ? (const char**)&a.grid : f == 4 ? (const char**)&a.tp
                       : f == 5 ? (const char**)&a.pp : f == 6 ? (const char**)&a.num : f == 7 ? (const char**)&a.ent_out
                       : (const char**)&a.present;
    *field += 2;
    if (f == 8) EXPECT(gate_sweep_plan(&a, 1, &p) == MLA_OK);           // bytes: any address
    else REFUSED(gate_sweep_plan(&a, 1, &p), "4-byte");
    *field += 2;
    EXPECT(gate_sweep_plan(&a, 1, &p) == MLA_OK);
  }
  {
    GateSweepArgs a = good;
    a.M = 2; a.l[2] = (const float*)((const char*)fbuf[2] + 1);          // not read with two modalities
    EXPECT(gate_sweep_plan(&a, 1, &p) == MLA_OK);
    a = good; a.labels = (const int64_t*)((const char*)lab64 + 4);
    REFUSED(gate_sweep_plan(&a, 1, &p), "8-byte");
  }
  // the plan at every tile: every row tile and every gate covered once, the remainders included; the kernel's LDS
  for (int rows : {1, 2, GATE_MAX_ROWS})
    for (int B : {1, 3, 4, 5, 7, 64, 65, 257, 600, 22714, rows * SWEEP_MAX_ROW_BLOCKS, rows * SWEEP_MAX_ROW_BLOCKS + 1})
      for (int G : {1, 63, 64, 65, 255, 256, 257, 861, 3321, 4096}) {
        GateSweepArgs a = good;
        a.B = B; a.G = G;
        EXPECT(gate_sweep_plan(&a, rows, &p) == MLA_OK);
        EXPECT(p.threads == SWEEP_LANES && p.threads <= 1024 && p.threads % 64 == 0);
        EXPECT(p.row_tiles * rows >= B && (p.row_tiles - 1) * rows < B);
        EXPECT(p.blocks_x >= 1 && p.blocks_x <= SWEEP_MAX_ROW_BLOCKS && (p.blocks_x == p.row_tiles || p.blocks_x == SWEEP_MAX_ROW_BLOCKS));
        EXPECT(p.blocks_y * SWEEP_LANES >= G && (p.blocks_y - 1) * SWEEP_LANES < G && p.blocks_y <= 65535);
      }
  EXPECT(sizeof(float) * GATE_MAX_ROWS * MLA_HEAD_MAXM * (MLA_HEAD_MAXC + 1) + 8 * GATE_MAX_ROWS <= 65536);
  {
    GateSweepArgs a = good;
    a.B = 0x7fffffff; a.G = SWEEP_MAXG; a.C = MLA_HEAD_MAXC;
    for (int rows : {1, 2, GATE_MAX_ROWS}) {
      EXPECT(gate_sweep_plan(&a, rows, &p) == MLA_OK);
      EXPECT(p.row_tiles == (0x7fffffffL + rows - 1) / rows && p.blocks_x == SWEEP_MAX_ROW_BLOCKS && p.blocks_y == SWEEP_MAXG / SWEEP_LANES);
    }
  }

  // ---- mla_eval_head_gated
  EvalHeadArgs head;
  memset(&head, 0, sizeof(head));
  head.x[0] = fbuf[0]; head.x[1] = fbuf[1]; head.x[2] = fbuf[2];
  head.W = fbuf[3]; head.bias = fbuf[4]; head.labels = lab64; head.present = have;
  head.counts = ibuf[0]; head.logits_out = fbuf[5]; head.fused_out = fbuf[6]; head.weights_out = fbuf[7]; head.pred_out = ibuf[1];
  head.alpha[0] = 0.55f; head.alpha[1] = 0.45f; head.alpha[2] = 0.f;
  head.M = 3; head.B = 2; head.D = 4; head.C = 2; head.mode = 7;          // the mode is not read
  EvalPlan ep;
  EXPECT(eval_head_gated_plan(&head, 2.f, &ep) == MLA_OK && ep.threads == 64 * 3 * EVAL_ROWS && ep.blocks == 1);
  for (int f = 0; f < 8; ++f) {
    EvalHeadArgs a = head;
    const void** field = f < 3 ? (const void**)&a.x[f] : f == 3 ? (const void**)&a.W : f == 4 ? (const void**)&a.bias
                       : f == 5 ? (const void**)&a.labels : f == 6 ? (const void**)&a.counts : (const void**)&a.logits_out;
    *field = nullptr;
    REFUSED(eval_head_gated_plan(&a, 2.f, &ep), "mla_eval_head_gated: null pointer");
  }
  {
    EvalHeadArgs a = head;
    a.M = 2; a.x[2] = nullptr; a.present = nullptr; a.fused_out = nullptr; a.weights_out = nullptr; a.pred_out = nullptr;
    a.alpha[2] = NAN;                                                      // not read with two modalities
    EXPECT(eval_head_gated_plan(&a, 2.f, &ep) == MLA_OK && ep.threads == 64 * 2 * EVAL_ROWS);
    a = head; a.M = 1;
    REFUSED(eval_head_gated_plan(&a, 2.f, &ep), "mla_eval_head_gated: need M = 2 or 3");
    a.M = 4;
    REFUSED(eval_head_gated_plan(&a, 2.f, &ep), "need M = 2 or 3");
    a = head; a.C = MLA_HEAD_MAXC + 1;
    REFUSED(eval_head_gated_plan(&a, 2.f, &ep), "mla_eval_head_gated: need 0 < C <= 128 (got 129)");
    a = head; a.D = 0;
    REFUSED(eval_head_gated_plan(&a, 2.f, &ep), "B, D, C > 0");
    a = head; a.alpha[1] = -0.5f;
    REFUSED(eval_head_gated_plan(&a, 2.f, &ep), "mla_eval_head_gated: need a finite prior1 in [0, 1024]");
    a = head; a.alpha[2] = 1025.f;
    REFUSED(eval_head_gated_plan(&a, 2.f, &ep), "need a finite prior2");
    a = head; a.alpha[0] = NAN;
    REFUSED(eval_head_gated_plan(&a, 2.f, &ep), "need a finite prior0");
    a = head;
    REFUSED(eval_head_gated_plan(&a, 16.5f, &ep), "mla_eval_head_gated: need a finite beta in [0, 16]");
    REFUSED(eval_head_gated_plan(&a, -1.f, &ep), "need a finite beta");
    REFUSED(eval_head_gated_plan(&a, INFINITY, &ep), "need a finite beta");
    a.fused_out = (float*)((char*)fbuf[6] + 2);
    REFUSED(eval_head_gated_plan(&a, 2.f, &ep), "4-byte");
    a = head; a.labels = (const int64_t*)((const char*)lab64 + 4);
    REFUSED(eval_head_gated_plan(&a, 2.f, &ep), "8-byte");
  }
  for (int M = 2; M <= 3; ++M)
    for (int B : {1, 2, 3, 5, 64, 65, 130, 22714}) {
      EvalHeadArgs a = head;
      a.M = M; a.B = B;
      EXPECT(eval_head_gated_plan(&a, 0.f, &ep) == MLA_OK);
      EXPECT(ep.threads == 64 * M * EVAL_ROWS && ep.threads <= 64 * MLA_HEAD_MAXM * EVAL_ROWS && ep.threads <= 1024);
      EXPECT((long)ep.blocks * EVAL_ROWS >= B && (long)(ep.blocks - 1) * EVAL_ROWS < B);
    }
  return host_check_done("gate");
}
