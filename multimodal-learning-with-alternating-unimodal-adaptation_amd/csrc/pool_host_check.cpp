// Stand-alone host check of the pooling / layout entry points' host half and of the pooled stem backward's tile plan (pool_args.h)
// with util.cpp's error reporting.  No GPU, no HIP: `make host-check` builds it with -fsanitize=address,undefined and runs it.
#include <initializer_list>
#include "pool_args.h"
#include "host_check.h"

// the tile plan before bn_pooled_tiles: the tile rule applied to the pooled rows alone
static long old_pooled_tiles(int MP) { return pool_cdiv(MP, bn_tile_rows(MP)); }

static void plan_of(int N, int H, int W, int* M, int* MP, int* tr, int* tiles) {
  *M = N * H * W;
  *MP = N * pool_out(H) * pool_out(W);
  bn_pooled_tiles(*M, *MP, tr, tiles);
}

int main() {
  const void* q = (const void*)0x1000;                    // stands for device memory: only looked at for null
  int M, MP, tr, tiles;

  // ---- the pooled reduction never writes more partial rows than mla_bn_bwd_ws_elems(M, C) holds
  EXPECT(bn_ws_tiles(245760) == 1024 && bn_ws_tiles(245761) == 961);       // rows held are not monotone in M
  long old_over = 0, changed = 0;
  for (int H = 1; H <= 12; ++H)
    for (int W = 1; W <= 12; ++W)
      for (int N = 1; N <= 70000; ++N) {                  // M <= 70000 * 144 < 2^31
        plan_of(N, H, W, &M, &MP, &tr, &tiles);
        const int held = bn_ws_tiles(M);
        if (tiles > held || tiles < 1 || tr % 16 != 0 || (long)tiles * tr < MP || (long)(tiles - 1) * tr >= MP) {
          fprintf(stderr, "N=%d H=%d W=%d: %d tiles of %d rows for %d pooled rows, %d rows held\n", N, H, W, tiles, tr, MP, held);
          ++failures;
          return 1;
        }
        const long old = old_pooled_tiles(MP);
        old_over += old > held;
        changed += tr != bn_tile_rows(MP);
        if (old <= held) EXPECT(tr == bn_tile_rows(MP) && tiles == old);   // the plan changes only where it has to
      }
  EXPECT(old_over > 0 && changed == old_over);            // the sweep does tell the two plans apart
  // the two named shapes: the old plan's rows against the rows held (the second one ran past the scratch tail as well)
  plan_of(2341, 5, 7, &M, &MP, &tr, &tiles);
  EXPECT(old_pooled_tiles(MP) == 878 && bn_ws_tiles(M) == 854 && tiles <= 854 && tr > bn_tile_rows(MP));
  plan_of(10891, 1, 5, &M, &MP, &tr, &tiles);
  EXPECT(old_pooled_tiles(MP) == 1022 && bn_ws_tiles(M) == 851 && tiles <= 851);
  EXPECT((1022 - 851) * 2 > 256);                         // 171 rows of 2 C floats: more than the 256 C + 2 floats of the tail
  // unchanged where the workload and the existing tests run
  const int keep[5][3] = {{64 * 3, 112, 112}, {1, 2, 2}, {3, 9, 7}, {2, 16, 12}, {8, 112, 40}};
  for (const auto& k : keep) {
    plan_of(k[0], k[1], k[2], &M, &MP, &tr, &tiles);
    EXPECT(tr == bn_tile_rows(MP) && tiles == old_pooled_tiles(MP) && tiles <= bn_ws_tiles(M));
  }
  plan_of(64 * 3, 112, 112, &M, &MP, &tr, &tiles);
  EXPECT(MP == 602112 && tr == 304 && tiles == 1981);

  // ---- the full plan and its refusals
  PooledBwdPlan bp;
  auto pooled = [&](const void* dpool, const void* idx, const void* y, const void* ch, const void* dg, const void* ws, int N, int H, int W,
                    int C) { return bn_bwd_pooled_plan(dpool, idx, y, ch, ch, ch, ch, dg, dg, ws, N, H, W, C, &bp); };
  EXPECT(pooled(q, q, q, q, q, q, 42, 112, 112, 64) == MLA_OK);
  EXPECT(bp.M == 526848 && bp.OH == 56 && bp.OW == 56 && bp.MP == 131712 && bp.quads == 2107392 && bp.grid == BN_EW_MAX_BLOCKS);
  EXPECT(pooled(q, q, q, q, q, q, 1, 1, 1, 4) == MLA_OK && bp.MP == 1 && bp.tiles == 1 && bp.quads == 1 && bp.grid == 1);
  REFUSED(pooled(nullptr, q, q, q, q, q, 2, 9, 7, 64), "null pointer");
  REFUSED(pooled(q, nullptr, q, q, q, q, 2, 9, 7, 64), "null pointer");
  REFUSED(pooled(q, q, nullptr, q, q, q, 2, 9, 7, 64), "null pointer");
  REFUSED(pooled(q, q, q, nullptr, q, q, 2, 9, 7, 64), "null pointer");
  REFUSED(pooled(q, q, q, q, nullptr, q, 2, 9, 7, 64), "null pointer");
  REFUSED(pooled(q, q, q, q, q, nullptr, 2, 9, 7, 64), "null pointer");
  REFUSED(pooled(q, q, q, q, q, q, 0, 9, 7, 64), "bad dims");
  REFUSED(pooled(q, q, q, q, q, q, -2, -9, 7, 64), "bad dims");
  REFUSED(pooled(q, q, q, q, q, q, 65536, 256, 128, 64), "bad dims");      // M = 2^31
  REFUSED(pooled(q, q, q, q, q, q, 2, 9, 7, 6), "must be 4*2^k");
  REFUSED(pooled(q, q, q, q, q, q, 2, 9, 7, 12), "must be 4*2^k");
  REFUSED(pooled(q, q, q, q, q, q, 2, 9, 7, 2048), "must be 4*2^k");
  REFUSED(pooled(q, q, q, q, q, q, 2, 9, 7, 0), "non-positive dims");

  PoolPlan p;
  auto fused = [&](const void* y, const void* ch, const void* out, const void* idx, int N, int H, int W, int C) {
    return bn_relu_maxpool_fwd_plan(y, ch, ch, ch, ch, out, idx, N, H, W, C, &p);
  };
  EXPECT(fused(q, q, q, q, 168, 112, 112, 64) == MLA_OK && p.OH == 56 && p.OW == 56 && p.units == 2107392 && p.grid == BN_EW_MAX_BLOCKS);
  EXPECT(fused(q, q, q, q, 2, 9, 7, 8) == MLA_OK && p.OH == 5 && p.OW == 4 && p.units == 2 * 3 * 2 * 2 && p.grid == 1);
  REFUSED(fused(nullptr, q, q, q, 2, 9, 7, 8), "bad argument");
  REFUSED(fused(q, nullptr, q, q, 2, 9, 7, 8), "bad argument");
  REFUSED(fused(q, q, nullptr, q, 2, 9, 7, 8), "bad argument");
  REFUSED(fused(q, q, q, nullptr, 2, 9, 7, 8), "bad argument");
  REFUSED(fused(q, q, q, q, 0, 9, 7, 8), "non-positive dims");
  REFUSED(fused(q, q, q, q, -2, -9, 7, 8), "bad argument");
  REFUSED(fused(q, q, q, q, 2, 9, 7, 10), "must be 4*2^k");
  REFUSED(fused(q, q, q, q, 65536, 256, 128, 64), "bad dims");

  // ---- max-pool
  for (int n = 1; n <= 9; ++n) EXPECT(pool_out(n) == (n - 1) / 2 + 1);
  EXPECT(pool_out(112) == 56 && pool_out(1025) == 513);
  EXPECT(maxpool_fwd_plan(q, q, q, 1, 1025, 1025, 64, &p) == MLA_OK && p.units == 4210704 && p.grid == POOL_MAX_BLOCKS);
  EXPECT(maxpool_fwd_plan(q, q, q, 2, 9, 7, 8, &p) == MLA_OK && p.OH == 5 && p.OW == 4 && p.units == 80 && p.grid == 1);
  EXPECT(maxpool_bwd_plan(q, q, q, 1, 1025, 1025, 64, &p) == MLA_OK && p.units == 16810000 && p.OH == 513);
  EXPECT(pool_grid_trips(p.units, POOL_MAX_BLOCKS) == 5);                  // four trips past the first
  REFUSED(maxpool_fwd_plan(nullptr, q, q, 2, 9, 7, 8, &p), "mla_maxpool3x3s2_fwd: bad argument");
  REFUSED(maxpool_fwd_plan(q, nullptr, q, 2, 9, 7, 8, &p), "bad argument");
  REFUSED(maxpool_fwd_plan(q, q, nullptr, 2, 9, 7, 8, &p), "bad argument");
  REFUSED(maxpool_fwd_plan(q, q, q, 2, 9, 7, 6, &p), "bad argument");
  REFUSED(maxpool_fwd_plan(q, q, q, 2, 0, 7, 8, &p), "bad argument");
  REFUSED(maxpool_bwd_plan(nullptr, q, q, 2, 9, 7, 8, &p), "mla_maxpool3x3s2_bwd: bad argument");
  REFUSED(maxpool_bwd_plan(q, nullptr, q, 2, 9, 7, 8, &p), "bad argument");
  REFUSED(maxpool_bwd_plan(q, q, nullptr, 2, 9, 7, 8, &p), "bad argument");
  REFUSED(maxpool_bwd_plan(q, q, q, 2, 9, 7, 9, &p), "bad argument");
  REFUSED(maxpool_bwd_plan(q, q, q, 2, 9, -7, 8, &p), "bad argument");

  // ---- average pool: cgpb is a power of two >= 4 that divides C / 4 and is the largest such <= 256, or the call is refused
  AvgPlan a;
  for (int C = 4; C <= 4096; C += 4) {
    const int c4n = C / 4, rc = avgpool_fwd_plan(q, q, 3, 49, C, &a);
    int best = 1;
    for (int k = 2; k <= 256; k *= 2)
      if (c4n % k == 0) best = k;
    if (best < 4) {
      EXPECT(rc == MLA_ERR_INVALID_ARG && strstr(mla_last_error(), "unsupported"));
    } else {
      EXPECT(rc == MLA_OK && a.cgpb == best && (a.cgpb & (a.cgpb - 1)) == 0 && a.cgpb >= 4 && c4n % a.cgpb == 0);
      EXPECT(a.nrl * a.cgpb == 256 && a.grid_x == 3 && (int)a.grid_y * a.cgpb == c4n);
    }
  }
  const int layouts[8][4] = {{16, 4, 64, 1}, {32, 8, 32, 1}, {64, 16, 16, 1}, {128, 32, 8, 1}, {512, 128, 2, 1}, {768, 64, 4, 3},
                             {1024, 256, 1, 1}, {2048, 256, 1, 2}};         // C -> cgpb, nrl, grid.y
  for (const auto& l : layouts)
    EXPECT(avgpool_fwd_plan(q, q, 1, 1, l[0], &a) == MLA_OK && a.cgpb == l[1] && a.nrl == l[2] && (int)a.grid_y == l[3]);
  for (int C : {4, 8, 12, 24}) REFUSED(avgpool_fwd_plan(q, q, 3, 49, C, &a), "unsupported");
  REFUSED(avgpool_fwd_plan(q, q, 3, 49, 18, &a), "mla_avgpool_fwd: bad argument");
  REFUSED(avgpool_fwd_plan(nullptr, q, 3, 49, 64, &a), "bad argument");
  REFUSED(avgpool_fwd_plan(q, nullptr, 3, 49, 64, &a), "bad argument");
  REFUSED(avgpool_fwd_plan(q, q, 0, 49, 64, &a), "bad argument");
  REFUSED(avgpool_fwd_plan(q, q, 3, 0, 64, &a), "bad argument");
  EXPECT(avgpool_bwd_plan(q, q, 33, 1024, 512, &p) == MLA_OK && p.units == 4325376 && p.grid == POOL_MAX_BLOCKS);
  EXPECT(avgpool_bwd_plan(q, q, 3, 49, 4, &p) == MLA_OK && p.units == 147 && p.grid == 1);         // the backward takes any C % 4 == 0
  REFUSED(avgpool_bwd_plan(nullptr, q, 3, 49, 64, &p), "mla_avgpool_bwd: bad argument");
  REFUSED(avgpool_bwd_plan(q, nullptr, 3, 49, 64, &p), "bad argument");
  REFUSED(avgpool_bwd_plan(q, q, 3, 49, 66, &p), "bad argument");
  REFUSED(avgpool_bwd_plan(q, q, 3, -1, 64, &p), "bad argument");

  // ---- layout
  EXPECT(video_to_nhwc_plan(q, q, 28, 3, 3, 224, 224, &p) == MLA_OK && p.units == 4214784 && p.grid == POOL_MAX_BLOCKS);
  EXPECT(video_to_nhwc_plan(q, q, 64, 3, 3, 224, 224, &p) == MLA_OK && p.units == 9633792 && p.grid == POOL_MAX_BLOCKS);
  EXPECT(video_to_nhwc_plan(q, q, 1, 8, 1, 1, 1, &p) == MLA_OK && p.grid == 1);
  REFUSED(video_to_nhwc_plan(q, q, 2, 9, 3, 5, 7, &p), "mla_video_to_nhwc: bad argument");
  REFUSED(video_to_nhwc_plan(q, q, 2, 0, 3, 5, 7, &p), "bad argument");
  REFUSED(video_to_nhwc_plan(nullptr, q, 2, 3, 3, 5, 7, &p), "bad argument");
  REFUSED(video_to_nhwc_plan(q, nullptr, 2, 3, 3, 5, 7, &p), "bad argument");
  REFUSED(video_to_nhwc_plan(q, q, 2, 3, 0, 5, 7, &p), "bad argument");
  TransposePlan t;
  EXPECT(transpose_plan(q, q, 3, 33, 70, &t) == MLA_OK && t.gx == 3 && t.gy == 2 && t.gz == 3);
  EXPECT(transpose_plan(q, q, 65535, 1, 32, &t) == MLA_OK && t.gx == 1 && t.gy == 1 && t.gz == 65535);
  REFUSED(transpose_plan(q, q, 65536, 33, 70, &t), "transpose: bad argument");
  REFUSED(transpose_plan(q, q, 0, 33, 70, &t), "bad argument");
  REFUSED(transpose_plan(nullptr, q, 3, 33, 70, &t), "bad argument");
  REFUSED(transpose_plan(q, nullptr, 3, 33, 70, &t), "bad argument");
  REFUSED(transpose_plan(q, q, 3, 0, 70, &t), "bad argument");
  REFUSED(transpose_plan(q, q, 3, 32 * 65535 + 1, 70, &t), "too many rows");
  EXPECT(transpose_plan(q, q, 3, 32 * 65535, 70, &t) == MLA_OK && t.gy == 65535);

  // ---- each capped grid covers n units in ceil(n / (cap * 256)) trips, with at least one workgroup and no workgroup without work
  for (unsigned cap : {(unsigned)POOL_MAX_BLOCKS, (unsigned)BN_EW_MAX_BLOCKS}) {
    const size_t per = (size_t)cap * POOL_THREADS;
    const size_t ns[] = {1, 255, 256, 257, per - 256, per - 255, per - 1, per, per + 1, 2 * per, 2 * per + 1, 5 * per - 3, ((size_t)1 << 33) + 5};
    for (size_t n : ns) {
      const size_t g = (size_t)pool_capped_grid(n, cap), trips = pool_grid_trips(n, cap);
      EXPECT(g >= 1 && g <= cap && (g - 1) * POOL_THREADS < n);
      EXPECT(trips == (n + per - 1) / per && g * POOL_THREADS * trips >= n && (trips == 1 || g == cap));
    }
    EXPECT(pool_capped_grid(0, cap) == 1);
  }
  // the first cases past a cap by less than one trip, and the cases just below them
  EXPECT(pool_grid_trips(4210704, POOL_MAX_BLOCKS) == 2 && pool_grid_trips((size_t)512 * 512 * 16, POOL_MAX_BLOCKS) == 1);
  EXPECT(pool_grid_trips(4214784, POOL_MAX_BLOCKS) == 2 && pool_grid_trips((size_t)27 * 3 * 224 * 224, POOL_MAX_BLOCKS) == 1);
  EXPECT(pool_grid_trips(4325376, POOL_MAX_BLOCKS) == 2 && pool_grid_trips((size_t)32 * 1024 * 128, POOL_MAX_BLOCKS) == 1);
  EXPECT(pool_grid_trips(2107392, BN_EW_MAX_BLOCKS) == 2 && pool_grid_trips((size_t)167 * 28 * 28 * 16, BN_EW_MAX_BLOCKS) == 1);
  return host_check_done("pool");
}
