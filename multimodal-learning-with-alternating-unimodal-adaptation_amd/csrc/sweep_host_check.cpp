// Stand-alone host check of mla_fusion_sweep's argument validation and launch plan (sweep_args.h) with util.cpp's error reporting.
// No GPU, no HIP: `make host-check` builds it with -fsanitize=address,undefined and runs it.
#include <initializer_list>
#include "sweep_args.h"
#include "host_check.h"

int main() {
  alignas(16) static float fbuf[4][64];
  alignas(16) static int64_t lab64[16];
  alignas(16) static int ibuf[3][64];
  alignas(16) static uint8_t have[64];
  SweepPlan p;

  SweepArgs good;
  memset(&good, 0, sizeof(good));
  for (int m = 0; m < MLA_HEAD_MAXM; ++m) good.l[m] = fbuf[m];
  good.labels = lab64; good.present = have; good.grid = fbuf[3];
  good.tp = ibuf[0]; good.pp = ibuf[1]; good.num = ibuf[2];
  good.M = 3; good.B = 5; good.C = 6; good.G = 7;
  EXPECT(fusion_sweep_plan(&good, &p) == MLA_OK);
  EXPECT(p.threads == SWEEP_LANES && p.blocks_x == (5 + SWEEP_ROWS - 1) / SWEEP_ROWS && p.blocks_y == 1 && p.row_tiles == p.blocks_x);

  for (int M : {-1, 0, 1, 4}) {
    SweepArgs a = good;
    a.M = M;
    REFUSED(fusion_sweep_plan(&a, &p), "mla_fusion_sweep: need M = 2 or 3");
  }
  // the required pointers: l2 only with three modalities; present and num may be null
  for (int M : {2, 3})
    for (int f = 0; f < 9; ++f) {
      SweepArgs a = good;
      a.M = M;
      const void** field = f < 3 ? (const void**)&a.l[f] : f == 3 ? (const void**)&a.labels : f == 4 ? (const void**)&a.grid
                         : f == 5 ? (const void**)&a.tp : f == 6 ? (const void**)&a.pp : f == 7 ? (const void**)&a.present
                         : (const void**)&a.num;
      *field = nullptr;
      if (f >= 7 || (f == 2 && M == 2)) EXPECT(fusion_sweep_plan(&a, &p) == MLA_OK);
      else REFUSED(fusion_sweep_plan(&a, &p), "mla_fusion_sweep: null pointer");
    }
  {
    SweepArgs a = good;
    a.B = 0;
    REFUSED(fusion_sweep_plan(&a, &p), "mla_fusion_sweep: need B, D, C > 0");
    a.B = -3;
    REFUSED(fusion_sweep_plan(&a, &p), "need B, D, C > 0");
    a = good; a.C = 0;
    REFUSED(fusion_sweep_plan(&a, &p), "need B, D, C > 0");
    a.C = MLA_HEAD_MAXC + 1;
    REFUSED(fusion_sweep_plan(&a, &p), "mla_fusion_sweep: need 0 < C <= 128 (got 129)");
    a.C = MLA_HEAD_MAXC;
    EXPECT(fusion_sweep_plan(&a, &p) == MLA_OK);
    a = good; a.G = 0;
    REFUSED(fusion_sweep_plan(&a, &p), "mla_fusion_sweep: need 0 < G <= 4096 grid points (got 0)");
    a.G = -1;
    REFUSED(fusion_sweep_plan(&a, &p), "need 0 < G <= 4096");
    a.G = SWEEP_MAXG + 1;
    REFUSED(fusion_sweep_plan(&a, &p), "need 0 < G <= 4096 grid points (got 4097)");
    a.G = SWEEP_MAXG;
    EXPECT(fusion_sweep_plan(&a, &p) == MLA_OK);
  }
  // alignment: every float / int32 buffer the call reads, l2 only when it is read
  for (int f = 0; f < 8; ++f) {
    SweepArgs a = good;
    const char** field = f < 3 ? (const char**)&a.l[f] : f == 3 ? (const char**)&a.grid : f == 4 ? (const char**)&a.tp
                       : f == 5 ? (const char**)&a.pp : f == 6 ? (const char**)&a.num : (const char**)&a.present;
    *field += 2;
    if (f == 7) EXPECT(fusion_sweep_plan(&a, &p) == MLA_OK);            // bytes: any address
    else REFUSED(fusion_sweep_plan(&a, &p), "4-byte");
    *field += 2;
    EXPECT(fusion_sweep_plan(&a, &p) == MLA_OK);
  }
  {
    SweepArgs a = good;
    a.M = 2; a.l[2] = (const float*)((const char*)fbuf[2] + 1);          // not read with two modalities
    EXPECT(fusion_sweep_plan(&a, &p) == MLA_OK);
    a = good; a.labels = (const int64_t*)((const char*)lab64 + 4);
    REFUSED(fusion_sweep_plan(&a, &p), "8-byte");
  }
  // the plan: every row tile and every grid point covered once, the remainders included
  for (int B : {1, 3, 4, 5, 7, 64, 65, 257, 22714, SWEEP_ROWS * SWEEP_MAX_ROW_BLOCKS, SWEEP_ROWS * SWEEP_MAX_ROW_BLOCKS + 1})
    for (int G : {1, 63, 64, 65, 255, 256, 257, 861, 3321, 4096}) {
      SweepArgs a = good;
      a.B = B; a.G = G;
      EXPECT(fusion_sweep_plan(&a, &p) == MLA_OK);
      EXPECT(p.threads == SWEEP_LANES && p.threads <= 1024);
      EXPECT(p.row_tiles * SWEEP_ROWS >= B && (p.row_tiles - 1) * SWEEP_ROWS < B);
      EXPECT(p.blocks_x >= 1 && p.blocks_x <= SWEEP_MAX_ROW_BLOCKS && (p.blocks_x == p.row_tiles || p.blocks_x == SWEEP_MAX_ROW_BLOCKS));
      EXPECT(p.blocks_y * SWEEP_LANES >= G && (p.blocks_y - 1) * SWEEP_LANES < G && p.blocks_y <= 65535);
    }
  // long arithmetic: a million rows against the largest grid, and the largest B an int holds
  {
    SweepArgs a = good;
    a.B = 1 << 20; a.G = SWEEP_MAXG; a.C = MLA_HEAD_MAXC;
    EXPECT(fusion_sweep_plan(&a, &p) == MLA_OK);
    EXPECT(p.row_tiles == (1L << 20) / SWEEP_ROWS && p.blocks_x == SWEEP_MAX_ROW_BLOCKS && p.blocks_y == SWEEP_MAXG / SWEEP_LANES);
    EXPECT((long)p.blocks_x * p.blocks_y * p.threads < (1L << 31));      // threads of the whole launch
    a.B = 0x7fffffff;
    EXPECT(fusion_sweep_plan(&a, &p) == MLA_OK);
    EXPECT(p.row_tiles == (0x7fffffffL + SWEEP_ROWS - 1) / SWEEP_ROWS && p.blocks_x == SWEEP_MAX_ROW_BLOCKS);
  }
  return host_check_done("sweep");
}
