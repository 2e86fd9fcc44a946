// Host half of the pooling and layout entry points (pool.hip) and of the two stem entry points that fuse BatchNorm into the max-pool
// (bn.hip: mla_bn_relu_maxpool_fwd, mla_bn_bwd_pooled): output sizes, capped grids, the avgpool layout, the argument checks and the
// tile plan of the pooled reduction -- with the BatchNorm tile rule that sizes its workspace.  Plain C++ with no HIP in it, so
// pool_host_check.cpp builds it with the host sanitizers.
#pragma once
#include "args_common.h"

#define POOL_THREADS 256
#define POOL_MAX_BLOCKS 16384     // pool.hip's grid-stride kernels
#define BN_EW_MAX_BLOCKS 8192     // bn.hip's elementwise kernels, the two fused stem kernels among them

static inline long pool_cdiv(long a, long b) { return (a + b - 1) / b; }

// max-pool 3x3, stride 2, padding 1
static inline int pool_out(int n) { return (n + 2 - 3) / 2 + 1; }

// workgroups of a grid-stride launch over n units: one thread per unit, at most max_blocks workgroups, at least one
static inline int pool_capped_grid(size_t n, unsigned max_blocks) {
  const unsigned b = mla_strided_blocks(n, POOL_THREADS, max_blocks, 1);
  return (int)(b < 1 ? 1 : b);
}
// how often the grid-stride loop of that launch runs for its busiest thread
static inline size_t pool_grid_trips(size_t n, unsigned max_blocks) {
  const size_t per_trip = (size_t)pool_capped_grid(n, max_blocks) * POOL_THREADS;
  return (n + per_trip - 1) / per_trip;
}

// ---- BatchNorm tiling (statistics, backward sums, the pooled reduction) -------------------------------------------------------------
static inline int bn_tile_rows(int M) {
  // aim at ~2048 workgroups for the big activations (stem, layer1: > 256 K rows), ~1024 below (then the statistics are
  // finalized by ONE launch, bn_finalize_tiles_kernel)
  long t = M > (1 << 18) ? ((long)M + 2047) / 2048 : ((long)M + 1023) / 1024;
  t = ((t + 15) / 16) * 16;
  if (t < 32) t = 32;
  if (t > 1024) t = 1024;
  return (int)t;
}
// partial rows [2][C] of M activation rows: what mla_bn_stats_partial_elems / mla_bn_bwd_ws_elems hold in front of their scratch tail
static inline int bn_ws_tiles(int M) { return (int)pool_cdiv(M, bn_tile_rows(M)); }

static inline int bn_check(const char* who, long M, int C) {
  MLA_REQUIRE(M > 0 && C > 0, "%s: non-positive dims", who);
  MLA_REQUIRE(C % 4 == 0 && C <= 1024 && 256 % (C / 4) == 0, "%s: C=%d must be 4*2^k, <= 1024", who, C);
  return MLA_OK;
}

// The pooled reduction tiles its MP = N * OH * OW pooled rows and writes one partial row per tile into a workspace the caller sized
// for the M = N * H * W pixels (mla_bn_bwd_ws_elems).  The tile rule of MP is kept wherever its tiles fit the bn_ws_tiles(M) rows of
// that workspace -- always at the stem's shapes, whose dgamma / dbeta bits depend on it.  They need not: cdiv(M, bn_tile_rows(M)) is
// not monotone in M (245760 rows: 1024 tiles, 245761 rows: 961), and small H, W bring MP close to M.  Then the tile grows to the
// smallest multiple of 16 rows with which they fit.
static inline void bn_pooled_tiles(int M, int MP, int* tile_rows, int* tiles) {
  const long held = bn_ws_tiles(M);
  long tr = bn_tile_rows(MP);
  if (pool_cdiv(MP, tr) > held) tr = pool_cdiv(pool_cdiv(MP, held), 16) * 16;
  *tile_rows = (int)tr;
  *tiles = (int)pool_cdiv(MP, tr);
}

// ---- launch plans --------------------------------------------------------------------------------------------------------------------
struct PoolPlan {        // a grid-stride launch of `grid` workgroups over `units` threads' worth of work
  int OH, OW;            // pooled size (max-pool entry points)
  size_t units;
  int grid;
};

static inline void pool_plan_fill(PoolPlan* p, int H, int W, size_t units, unsigned max_blocks) {
  p->OH = pool_out(H);
  p->OW = pool_out(W);
  p->units = units;
  p->grid = pool_capped_grid(units, max_blocks);
}

// one thread per pooled output and 4 channels
static inline int maxpool_fwd_plan(const void* x, const void* y, const void* idx, int N, int H, int W, int C, PoolPlan* p) {
  MLA_REQUIRE(x && y && idx && N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "mla_maxpool3x3s2_fwd: bad argument");
  pool_plan_fill(p, H, W, (size_t)N * pool_out(H) * pool_out(W) * (C / 4), POOL_MAX_BLOCKS);
  return MLA_OK;
}

// one thread per input pixel and 4 channels
static inline int maxpool_bwd_plan(const void* dy, const void* idx, const void* dx, int N, int H, int W, int C, PoolPlan* p) {
  MLA_REQUIRE(dy && idx && dx && N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "mla_maxpool3x3s2_bwd: bad argument");
  pool_plan_fill(p, H, W, (size_t)N * H * W * (C / 4), POOL_MAX_BLOCKS);
  return MLA_OK;
}

struct AvgPlan {         // block = cgpb float4 column groups x nrl row lanes; grid = (NB, (C / 4) / cgpb)
  int cgpb, nrl;
  unsigned grid_x, grid_y;
};

static inline int avgpool_fwd_plan(const void* x, const void* y, int NB, int P, int C, AvgPlan* p) {
  MLA_REQUIRE(x && y && NB > 0 && P > 0 && C > 0 && C % 4 == 0, "mla_avgpool_fwd: bad argument");
  const int c4n = C / 4;
  int cgpb = 256;
  while (cgpb > 1 && c4n % cgpb != 0) cgpb >>= 1;     // largest power of two <= 256 dividing C/4 (C=768 -> 64)
  MLA_REQUIRE(cgpb >= 4, "mla_avgpool_fwd: C=%d unsupported", C);
  p->cgpb = cgpb;
  p->nrl = 256 / cgpb;
  p->grid_x = (unsigned)NB;
  p->grid_y = (unsigned)(c4n / cgpb);
  return MLA_OK;
}

static inline int avgpool_bwd_plan(const void* dy, const void* dx, int NB, int P, int C, PoolPlan* p) {
  MLA_REQUIRE(dy && dx && NB > 0 && P > 0 && C > 0 && C % 4 == 0, "mla_avgpool_bwd: bad argument");
  pool_plan_fill(p, 1, 1, (size_t)NB * P * (C / 4), POOL_MAX_BLOCKS);
  return MLA_OK;
}

// one thread per output pixel, all (<= 8) channels
static inline int video_to_nhwc_plan(const void* src, const void* dst, int B, int C, int T, int H, int W, PoolPlan* p) {
  MLA_REQUIRE(src && dst && B > 0 && C > 0 && C <= 8 && T > 0 && H > 0 && W > 0, "mla_video_to_nhwc: bad argument");
  pool_plan_fill(p, H, W, (size_t)B * T * H * W, POOL_MAX_BLOCKS);
  return MLA_OK;
}

struct TransposePlan {   // 32 x 32 tiles: grid = (cdiv(S, 32), cdiv(R, 32), batch)
  unsigned gx, gy, gz;
};

static inline int transpose_plan(const void* src, const void* dst, int batch, int R, int S, TransposePlan* p) {
  MLA_REQUIRE(src && dst && batch > 0 && batch < 65536 && R > 0 && S > 0, "transpose: bad argument");
  MLA_REQUIRE(pool_cdiv(R, 32) < 65536, "transpose: too many rows");
  p->gx = (unsigned)pool_cdiv(S, 32);
  p->gy = (unsigned)pool_cdiv(R, 32);
  p->gz = (unsigned)batch;
  return MLA_OK;
}

// one thread per 2x2 block of pooled outputs and 4 channels
static inline int bn_relu_maxpool_fwd_plan(const void* y, const void* mean, const void* invstd, const void* gamma, const void* beta,
                                           const void* out, const void* idx, int N, int H, int W, int C, PoolPlan* p) {
  const long Ml = (long)N * H * W;
  MLA_TRY(bn_check("mla_bn_relu_maxpool_fwd", Ml, C));
  MLA_REQUIRE(y && mean && invstd && gamma && beta && out && idx && N > 0 && H > 0 && W > 0, "mla_bn_relu_maxpool_fwd: bad argument");
  MLA_REQUIRE(Ml < (1L << 31), "mla_bn_relu_maxpool_fwd: bad dims");
  const int OH = pool_out(H), OW = pool_out(W);
  pool_plan_fill(p, H, W, (size_t)N * ((OH + 1) / 2) * ((OW + 1) / 2) * (C / 4), BN_EW_MAX_BLOCKS);
  return MLA_OK;
}

struct PooledBwdPlan {
  int M, OH, OW, MP;
  int tile_rows, tiles;  // the reduction over pooled rows: tiles <= bn_ws_tiles(M)
  size_t quads;          // the apply pass: one thread per 2x2 pixel quad and 4 channels
  int grid;
};

static inline int bn_bwd_pooled_plan(const void* dpool, const void* idx, const void* y, const void* mean, const void* invstd,
                                     const void* gamma, const void* beta, const void* dgamma, const void* dbeta, const void* ws, int N,
                                     int H, int W, int C, PooledBwdPlan* p) {
  const long Ml = (long)N * H * W;
  MLA_REQUIRE(Ml > 0 && Ml < (1L << 31), "mla_bn_bwd_pooled: bad dims");
  MLA_TRY(bn_check("mla_bn_bwd_pooled", Ml, C));
  MLA_REQUIRE(dpool && idx && y && mean && invstd && gamma && beta && dgamma && dbeta && ws, "mla_bn_bwd_pooled: null pointer");
  MLA_REQUIRE(N > 0 && H > 0 && W > 0, "mla_bn_bwd_pooled: bad dims");      // (two negative sizes have a positive product)
  p->M = (int)Ml;
  p->OH = pool_out(H);
  p->OW = pool_out(W);
  p->MP = N * p->OH * p->OW;
  bn_pooled_tiles(p->M, p->MP, &p->tile_rows, &p->tiles);
  p->quads = (size_t)N * ((H + 1) / 2) * ((W + 1) / 2) * (C / 4);
  p->grid = pool_capped_grid(p->quads, BN_EW_MAX_BLOCKS);
  return MLA_OK;
}
