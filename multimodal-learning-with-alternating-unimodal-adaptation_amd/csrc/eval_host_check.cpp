// Stand-alone host check of mla_eval_head's and mla_eval_fuse's argument validation and launch plans (eval_args.h) with util.cpp's
// error reporting.
// No GPU, no HIP: `make host-check` builds it with -fsanitize=address,undefined and runs it.
#include <initializer_list>
#include "eval_args.h"
#include "host_check.h"

// op 0: null; 1: two bytes on; 2: four bytes on
template <class T>
static void shift(T*& p, int op) {
  p = op == 0 ? nullptr : (T*)((uintptr_t)p + (op == 1 ? 2 : 4));
}
// fields 0..7 are required (x[2] with M = 3), 8..10 optional
static void poke(EvalHeadArgs& a, int field, int op) {
  switch (field) {
    case 0: shift(a.x[0], op); break;
    case 1: shift(a.x[1], op); break;
    case 2: shift(a.x[2], op); break;
    case 3: shift(a.W, op); break;
    case 4: shift(a.bias, op); break;
    case 5: shift(a.labels, op); break;
    case 6: shift(a.counts, op); break;
    case 7: shift(a.logits_out, op); break;
    case 8: shift(a.fused_out, op); break;
    case 9: shift(a.weights_out, op); break;
    default: shift(a.pred_out, op); break;
  }
}

int main() {
  alignas(16) static float buf[8][64];
  alignas(16) static int64_t lab[16];
  alignas(16) static int ibuf[2][64];
  static uint8_t present[64];
  EvalHeadArgs good;
  memset(&good, 0, sizeof(good));
  good.x[0] = buf[0]; good.x[1] = buf[1]; good.x[2] = buf[2];
  good.W = buf[3]; good.bias = buf[4]; good.labels = lab; good.present = present;
  good.counts = ibuf[0]; good.logits_out = buf[5]; good.fused_out = buf[6]; good.weights_out = buf[7]; good.pred_out = ibuf[1];
  good.M = 3; good.B = 2; good.D = 4; good.C = 2; good.mode = 1;
  EvalPlan p;
  EXPECT(eval_head_plan(&good, &p) == MLA_OK);

  // null pointers, one at a time; x[2] is required with three modalities only; present and the per-row outputs may be null
  for (int f = 0; f < 8; ++f) {
    EvalHeadArgs a = good;
    poke(a, f, 0);
    EXPECT(eval_head_plan(&a, &p) == MLA_ERR_INVALID_ARG);
    EXPECT(strstr(mla_last_error(), "mla_eval_head: null pointer"));
  }
  {
    EvalHeadArgs a = good;
    a.M = 2; a.x[2] = nullptr; a.present = nullptr; a.fused_out = nullptr; a.weights_out = nullptr; a.pred_out = nullptr;
    EXPECT(eval_head_plan(&a, &p) == MLA_OK);
  }
  // modalities, sizes, mode
  for (int M : {-1, 0, 1, 4}) {
    EvalHeadArgs a = good;
    a.M = M;
    EXPECT(eval_head_plan(&a, &p) == MLA_ERR_INVALID_ARG);
    EXPECT(strstr(mla_last_error(), "need M = 2 or 3"));
  }
  for (int z = 0; z < 3; ++z)
    for (int v : {0, -1}) {
      EvalHeadArgs a = good;
      (z == 0 ? a.B : z == 1 ? a.D : a.C) = v;
      EXPECT(eval_head_plan(&a, &p) == MLA_ERR_INVALID_ARG);
      EXPECT(strstr(mla_last_error(), "B, D, C > 0"));
    }
  {
    EvalHeadArgs a = good;
    a.C = MLA_HEAD_MAXC + 1;
    EXPECT(eval_head_plan(&a, &p) == MLA_ERR_INVALID_ARG);
    EXPECT(strstr(mla_last_error(), "need 0 < C <= 128 (got 129)"));
    a.C = MLA_HEAD_MAXC;
    EXPECT(eval_head_plan(&a, &p) == MLA_OK);
    a.mode = 0;
    EXPECT(eval_head_plan(&a, &p) == MLA_OK);
    for (int mode : {-1, 2}) {
      a.mode = mode;
      EXPECT(eval_head_plan(&a, &p) == MLA_ERR_INVALID_ARG);
      EXPECT(strstr(mla_last_error(), "need mode = 0"));
    }
  }
  // alignment: every float / int32 buffer at 4 bytes, the labels at 8; any 4-byte offset passes (slices of flat buffers)
  for (int f = 0; f < 11; ++f) {
    if (f == 5) continue;                       // the labels: below
    EvalHeadArgs a = good;
    poke(a, f, 1);
    EXPECT(eval_head_plan(&a, &p) == MLA_ERR_INVALID_ARG);
    EXPECT(strstr(mla_last_error(), "4-byte"));
    a = good;
    poke(a, f, 2);
    EXPECT(eval_head_plan(&a, &p) == MLA_OK);
  }
  {
    EvalHeadArgs a = good;
    a.labels = (const int64_t*)((const char*)lab + 4);
    EXPECT(eval_head_plan(&a, &p) == MLA_ERR_INVALID_ARG);
    a = good;
    a.present = present + 1;                    // bytes: no alignment asked
    EXPECT(eval_head_plan(&a, &p) == MLA_OK);
  }
  // the plan: one wave per (row, modality), every row covered once, the workgroup inside the kernel's launch bound and its LDS
  for (int M = 2; M <= 3; ++M)
    for (int B : {1, 2, 3, 5, 64, 65, 130, 22714}) {
      EvalHeadArgs a = good;
      a.M = M; a.B = B;
      EXPECT(eval_head_plan(&a, &p) == MLA_OK);
      EXPECT(p.threads == 64 * M * EVAL_ROWS && p.threads <= 64 * MLA_HEAD_MAXM * EVAL_ROWS && p.threads <= 1024);
      EXPECT((long)p.blocks * EVAL_ROWS >= B && (long)(p.blocks - 1) * EVAL_ROWS < B);
    }
  EXPECT(sizeof(float) * EVAL_ROWS * MLA_HEAD_MAXM * MLA_HEAD_MAXC <= 6144);

  // mla_eval_fuse: one message for every refusal; out[2] is required with three modalities only; one workgroup of 256 threads
  EvalFuseArgs fuse;
  memset(&fuse, 0, sizeof(fuse));
  fuse.out[0] = buf[0]; fuse.out[1] = buf[1]; fuse.out[2] = buf[2];
  fuse.M = 3; fuse.B = 2; fuse.C = 2;
  EXPECT(eval_fuse_plan(&fuse, lab, ibuf[0], &p) == MLA_OK && p.threads == 256 && p.blocks == 1);
  for (int f = 0; f < 3; ++f) {
    EvalFuseArgs a = fuse;
    a.out[f] = nullptr;
    REFUSED(eval_fuse_plan(&a, lab, ibuf[0], &p), "mla_eval_fuse: bad argument");
    a.M = 2;
    EXPECT((eval_fuse_plan(&a, lab, ibuf[0], &p) == MLA_OK) == (f == 2));
  }
  REFUSED(eval_fuse_plan(&fuse, nullptr, ibuf[0], &p), "mla_eval_fuse: bad argument");
  REFUSED(eval_fuse_plan(&fuse, lab, nullptr, &p), "mla_eval_fuse: bad argument");
  for (int M : {-1, 0, 1, 4}) {
    EvalFuseArgs a = fuse;
    a.M = M;
    REFUSED(eval_fuse_plan(&a, lab, ibuf[0], &p), "mla_eval_fuse: bad argument");
  }
  for (int z = 0; z < 2; ++z)
    for (int v : {0, -1}) {
      EvalFuseArgs a = fuse;
      (z == 0 ? a.B : a.C) = v;
      REFUSED(eval_fuse_plan(&a, lab, ibuf[0], &p), "mla_eval_fuse: bad argument");
    }
  return host_check_done("eval");
}
