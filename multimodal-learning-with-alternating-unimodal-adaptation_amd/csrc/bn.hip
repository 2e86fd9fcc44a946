// BatchNorm2d (training mode) over pixel-major [M][C] fp32 activations, gfx950.
//
// Replaces the ATen batch_norm forward/backward that nn.BatchNorm2d triggers in the reference
// (models/backbone.py:29, 32, 86, 128; momentum 0.1, eps 1e-5, biased batch variance for the
// normalisation, unbiased for running_var) together with the in-place ReLU and the residual add
// of BasicBlock.forward (backbone.py:41, 49-50), which are fused into the apply pass.
//
// HBM-bound: every pass is float4-vectorised with channels on the fast axis, so a wave reads
// whole 256-B..1-KiB pixel rows; per-channel reductions are thread-private over a row stripe,
// then LDS across row lanes, then fp64 across tiles -- no atomics, results are bitwise reproducible.
// Statistics normally arrive pre-reduced from the conv epilogue (conv_igemm.hip), saving one full
// read of the activation.
//
// The fp64 step over the tile partials [tiles][2][C] is one family for both directions
// (bn_finalize_partials picks the regime): bn_finalize_tiles_kernel<PT, FWD, CL, KL> in one launch
// (<16, 16> or <4, 64>), or bn_tiles_stage1_kernel + bn_finalize_chunks_kernel<FWD>; the closing
// arithmetic is written once (bn_close_fwd, bn_close_bwd).
#include "common.h"
#include "pool_args.h"

static size_t bn_red_scratch_floats(int C);
// ---- tiling shared by the stats and backward-reduce kernels --------------------------------
// bn_tile_rows / bn_ws_tiles: pool_args.h (the host half the pooled stem entry points share with their host check)

// Every partial buffer carries a scratch tail for the two-stage reduction (declared in bn.hip, used by the conv too).
extern "C" size_t mla_bn_partial_scratch_elems(int C) { return bn_red_scratch_floats(C); }
extern "C" size_t mla_bn_stats_partial_elems(int M, int C) {
  return (size_t)bn_ws_tiles(M) * 2 * C * 2 + bn_red_scratch_floats(C);     // forward statistics: fp64 partials
}
extern "C" size_t mla_bn_bwd_ws_elems(int M, int C) { return (size_t)bn_ws_tiles(M) * 2 * C + bn_red_scratch_floats(C); }

// one per-channel float4 (mean, invstd, gamma, beta, dgamma, dbeta) of column group cg
__device__ __forceinline__ f32x4 chan4(const float* __restrict__ p, int cg) { return reinterpret_cast<const f32x4*>(p)[cg]; }

// The tail of the fp32 tile reductions (bn_reduce_kernel<1>, bn_bwd_pooled_reduce_kernel): row lane 0 of every column group adds
// the sums of lanes 1..nrl-1 in that order through LDS and stores the partial row partial[tile][0|1][C] of this workgroup.
__device__ __forceinline__ void bn_store_tile_sums(f32x4 s0, f32x4 s1, float* __restrict__ partial, int C, int cg, int rl, int nrl) {
  __shared__ f32x4 red[2][256];
  const int c4n = C >> 2;
  red[0][threadIdx.x] = s0;
  red[1][threadIdx.x] = s1;
  __syncthreads();
  if (rl == 0) {
    for (int k = 1; k < nrl; ++k) {
      s0 += red[0][k * c4n + cg];
      s1 += red[1][k * c4n + cg];
    }
    reinterpret_cast<f32x4*>(partial + ((size_t)blockIdx.x * 2 + 0) * C)[cg] = s0;
    reinterpret_cast<f32x4*>(partial + ((size_t)blockIdx.x * 2 + 1) * C)[cg] = s1;
  }
}

// Reduce two per-channel quantities over a tile of rows.  MODE 0: (x, x^2), fp64 partials.  MODE 1: (g, g*xhat), fp32 partials.
// Block: 256 threads = (C/4 column groups) x (row lanes); C/4 <= 256 and divides 256.
template <int MODE>
__global__ __launch_bounds__(256) void bn_reduce_kernel(const float* __restrict__ x, const float* __restrict__ dout,
                                                         const float* __restrict__ relu_out,
                                                         const float* __restrict__ mean, const float* __restrict__ invstd,
                                                         float* __restrict__ partial, int M, int C, int tile_rows) {
  const int c4n = C >> 2;
  const int cg = threadIdx.x % c4n, rl = threadIdx.x / c4n, nrl = 256 / c4n;
  const int r0 = blockIdx.x * tile_rows, r1 = min(M, r0 + tile_rows);
  if (MODE == 0) {   // forward statistics: everything in fp64 (x * x is exact there), see the conv epilogue in igemm_common.h
    double d0[4] = {0.0, 0.0, 0.0, 0.0}, d1[4] = {0.0, 0.0, 0.0, 0.0};
    for (int r = r0 + rl; r < r1; r += nrl) {
      const f32x4 xv = reinterpret_cast<const f32x4*>(x)[(size_t)r * c4n + cg];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double v = (double)xv[e];
        d0[e] += v;
        d1[e] += v * v;
      }
    }
    __shared__ double redd[2][4][256];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      redd[0][e][threadIdx.x] = d0[e];
      redd[1][e][threadIdx.x] = d1[e];
    }
    __syncthreads();
    if (rl == 0) {
      double* pd = reinterpret_cast<double*>(partial);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        double a = d0[e], q = d1[e];
        for (int k = 1; k < nrl; ++k) {
          a += redd[0][e][k * c4n + cg];
          q += redd[1][e][k * c4n + cg];
        }
        pd[((size_t)blockIdx.x * 2 + 0) * C + cg * 4 + e] = a;
        pd[((size_t)blockIdx.x * 2 + 1) * C + cg * 4 + e] = q;
      }
    }
    return;
  }
  const f32x4 mu = chan4(mean, cg), is = chan4(invstd, cg);
  f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
  for (int r = r0 + rl; r < r1; r += nrl) {
    const size_t idx = (size_t)r * c4n + cg;
    const f32x4 xv = reinterpret_cast<const f32x4*>(x)[idx];
    f32x4 g = reinterpret_cast<const f32x4*>(dout)[idx];
    if (relu_out) {
      const f32x4 o = reinterpret_cast<const f32x4*>(relu_out)[idx];
#pragma unroll
      for (int e = 0; e < 4; ++e) g[e] = o[e] > 0.f ? g[e] : 0.f;
    }
    s0 += g;
    s1 += g * ((xv - mu) * is);
  }
  bn_store_tile_sums(s0, s1, partial, C, cg, rl, nrl);
}

// Two-stage fp64 reduction of the per-tile partials partial[t][0|1][c] (up to 9408 tiles at the 64x64 conv tile).
// Stage 1: grid (C/64, S <= 64): a block = 64 channels (lanes: coalesced 256-B rows) x 4 waves striding over its chunk
// of >= 64 tiles -> fp64 chunk sums in `scratch[s][0|1][c]`.  Stage 2: one block per 64 channels = 64 channels x 4
// chunk lanes, each lane loads its <= 16 chunk sums at once (no serial load chain) and the lanes are combined through
// LDS in a fixed order.  Deterministic.
#define BN_RED_MAXS 64
static int bn_red_chunks(int tiles) { int s = cdiv(tiles, 64); return s < 1 ? 1 : (s > BN_RED_MAXS ? BN_RED_MAXS : s); }
static size_t bn_red_scratch_floats(int C) { return (size_t)BN_RED_MAXS * 2 * C * 2 + 2; }   // doubles, as floats (+ alignment)

template <typename PT>   // PT = double: forward statistics partials; float: backward (sum g, sum g * xhat) partials
__global__ __launch_bounds__(256) void bn_tiles_stage1_kernel(const PT* __restrict__ partial, int tiles, int C,
                                                               double* __restrict__ scratch) {
  __shared__ double red[2][4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  const int S = gridDim.y, per = (tiles + S - 1) / S;
  const int t0 = blockIdx.y * per, t1 = min(tiles, t0 + per);
  double s = 0.0, q = 0.0;
  if (c < C)
    for (int t = t0 + wave; t < t1; t += 4) {
      s += (double)partial[((size_t)t * 2 + 0) * C + c];
      q += (double)partial[((size_t)t * 2 + 1) * C + c];
    }
  red[0][wave][lane] = s;
  red[1][wave][lane] = q;
  __syncthreads();
  if (wave == 0 && c < C) {
    for (int w = 1; w < 4; ++w) {
      s += red[0][w][lane];
      q += red[1][w][lane];
    }
    scratch[((size_t)blockIdx.y * 2 + 0) * C + c] = s;
    scratch[((size_t)blockIdx.y * 2 + 1) * C + c] = q;
  }
}

// sums of the S chunk sums for channel c = blockIdx.x*64 + lane; valid in wave 0
__device__ __forceinline__ void chunk_sums(const double* __restrict__ scratch, int S, int C, double& s, double& q) {
  __shared__ double red2[2][4][64];
  const int lane = threadIdx.x & 63, kl = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  double sv[BN_RED_MAXS / 4], qv[BN_RED_MAXS / 4];
#pragma unroll
  for (int j = 0; j < BN_RED_MAXS / 4; ++j) {        // all loads of this lane in flight at once
    const int k = kl + 4 * j;
    const bool ok = k < S && c < C;
    sv[j] = ok ? scratch[((size_t)k * 2 + 0) * C + c] : 0.0;
    qv[j] = ok ? scratch[((size_t)k * 2 + 1) * C + c] : 0.0;
  }
  s = 0.0;
  q = 0.0;
#pragma unroll
  for (int j = 0; j < BN_RED_MAXS / 4; ++j) {
    s += sv[j];
    q += qv[j];
  }
  red2[0][kl][lane] = s;
  red2[1][kl][lane] = q;
  __syncthreads();
  if (kl == 0)
    for (int w = 1; w < 4; ++w) {
      s += red2[0][w][lane];
      q += red2[1][w][lane];
    }
}

// The closing arithmetic of every finalize regime, from the fp64 channel totals s (slot 0) and q (slot 1).
// Forward: mean, invstd from the clamped biased variance, running statistics with the unbiased one.
__device__ __forceinline__ void bn_close_fwd(double s, double q, int M, float eps, float momentum, int c, float* __restrict__ mean,
                                             float* __restrict__ invstd, float* running_mean, float* running_var) {
  const double m = s / M;
  double var = q / M - m * m;
  if (var < 0.0) var = 0.0;
  mean[c] = (float)m;
  invstd[c] = (float)(1.0 / sqrt(var + (double)eps));
  if (running_mean) {
    const double unb = var * ((double)M / (double)(M > 1 ? M - 1 : 1));
    running_mean[c] = (float)((1.0 - momentum) * (double)running_mean[c] + momentum * m);
    running_var[c] = (float)((1.0 - momentum) * (double)running_var[c] + momentum * unb);
  }
}
// Backward: slot 0 is sum g = dbeta, slot 1 is sum g * xhat = dgamma.
__device__ __forceinline__ void bn_close_bwd(double s, double q, int c, float* __restrict__ dgamma, float* __restrict__ dbeta) {
  dbeta[c] = (float)s;
  dgamma[c] = (float)q;
}

// Stage 2.  FWD 1: out0 = mean, out1 = invstd.  FWD 0: out0 = dgamma, out1 = dbeta (the other arguments are unused).
template <int FWD>
__global__ __launch_bounds__(256) void bn_finalize_chunks_kernel(const double* __restrict__ scratch, int S, int M, int C, float eps,
                                                                  float momentum, float* __restrict__ out0, float* __restrict__ out1,
                                                                  float* running_mean, float* running_var) {
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  double s, q;
  chunk_sums(scratch, S, C, s, q);
  if ((threadIdx.x >> 6) != 0 || c >= C) return;
  if (FWD) bn_close_fwd(s, q, M, eps, momentum, c, out0, out1, running_mean, running_var);
  else bn_close_bwd(s, q, c, out0, out1);
}

// One-launch finalize, instead of the stage-1 + stage-2 pair (two dependent 5-8 us launches on the serial conv -> statistics ->
// apply chain): a block owns CL channels x KL tile lanes; lane k sums tiles k, k + KL, ... (four loads in flight, then a tail of
// single tiles), lane 0 adds the other lanes through LDS in ascending order, then the closing arithmetic above.  Two shapes:
//   <16, 16>  up to BN_ONE_MAXT tiles (every layer but the stem and layer1 forward);
//   <4, 64>   up to BN_WIDE_MAXT (layer1: 2048 / 2352 conv tiles, the pooled stem backward: <= 37 values per lane at 2352 tiles).
// The order of the fp64 additions is part of the contract: tests/exact.py restates it and test_finalize_order holds every regime to it.
template <typename PT, int FWD, int CL, int KL>
__global__ __launch_bounds__(256) void bn_finalize_tiles_kernel(const PT* __restrict__ partial, int tiles, int M, int C, float eps,
                                                                 float momentum, float* __restrict__ out0, float* __restrict__ out1,
                                                                 float* running_mean, float* running_var) {
  static_assert(CL * KL == 256, "a block is CL channels x KL tile lanes");
  __shared__ double red[2][KL][CL];
  const int cl = threadIdx.x % CL, kl = threadIdx.x / CL;
  const int c = blockIdx.x * CL + cl;
  double s = 0.0, q = 0.0;
  if (c < C) {
    int t = kl;
    for (; t + 3 * KL < tiles; t += 4 * KL) {
      const double a0 = (double)partial[((size_t)t * 2 + 0) * C + c], b0 = (double)partial[((size_t)t * 2 + 1) * C + c];
      const double a1 = (double)partial[((size_t)(t + KL) * 2 + 0) * C + c], b1 = (double)partial[((size_t)(t + KL) * 2 + 1) * C + c];
      const double a2 = (double)partial[((size_t)(t + 2 * KL) * 2 + 0) * C + c], b2 = (double)partial[((size_t)(t + 2 * KL) * 2 + 1) * C + c];
      const double a3 = (double)partial[((size_t)(t + 3 * KL) * 2 + 0) * C + c], b3 = (double)partial[((size_t)(t + 3 * KL) * 2 + 1) * C + c];
      s += (a0 + a1) + (a2 + a3);
      q += (b0 + b1) + (b2 + b3);
    }
    for (; t < tiles; t += KL) {
      s += (double)partial[((size_t)t * 2 + 0) * C + c];
      q += (double)partial[((size_t)t * 2 + 1) * C + c];
    }
  }
  red[0][kl][cl] = s;
  red[1][kl][cl] = q;
  __syncthreads();
  if (kl != 0 || c >= C) return;
  for (int k = 1; k < KL; ++k) {
    s += red[0][k][cl];
    q += red[1][k][cl];
  }
  if (FWD) bn_close_fwd(s, q, M, eps, momentum, c, out0, out1, running_mean, running_var);
  else bn_close_bwd(s, q, c, out0, out1);
}

// The one place that picks the finalize regime for `tiles` partial rows partial[tiles][2][C] (PT = double, FWD = 1: forward
// statistics -> out0 = mean, out1 = invstd and the running statistics; PT = float, FWD = 0: backward sums -> out0 = dgamma,
// out1 = dbeta).  Beyond BN_WIDE_MAXT tiles the two-stage pair runs through the scratch tail that follows the tiles.
constexpr int BN_ONE_MAXT = 1024, BN_WIDE_MAXT = 16384;
template <typename PT, int FWD>
static int bn_finalize_partials(const PT* partial, int tiles, int M, int C, float eps, float momentum, float* out0, float* out1,
                                float* running_mean, float* running_var, hipStream_t st) {
  if (tiles <= BN_ONE_MAXT) {
    bn_finalize_tiles_kernel<PT, FWD, 16, 16><<<cdiv(C, 16), 256, 0, st>>>(partial, tiles, M, C, eps, momentum, out0, out1, running_mean, running_var);
    MLA_CHECK_LAUNCH("bn_finalize_tiles_kernel<16, 16>");
  } else if (tiles <= BN_WIDE_MAXT) {
    bn_finalize_tiles_kernel<PT, FWD, 4, 64><<<cdiv(C, 4), 256, 0, st>>>(partial, tiles, M, C, eps, momentum, out0, out1, running_mean, running_var);
    MLA_CHECK_LAUNCH("bn_finalize_tiles_kernel<4, 64>");
  } else {
    double* scratch = reinterpret_cast<double*>(const_cast<PT*>(partial) + (size_t)tiles * 2 * C);
    const int S = bn_red_chunks(tiles);
    bn_tiles_stage1_kernel<PT><<<dim3(cdiv(C, 64), S), 256, 0, st>>>(partial, tiles, C, scratch);
    MLA_CHECK_LAUNCH("bn_tiles_stage1_kernel");
    bn_finalize_chunks_kernel<FWD><<<cdiv(C, 64), 256, 0, st>>>(scratch, S, M, C, eps, momentum, out0, out1, running_mean, running_var);
    MLA_CHECK_LAUNCH("bn_finalize_chunks_kernel");
  }
  return MLA_OK;
}

// the one BN expression (explicit fma) every kernel that forms or re-forms bn(x) uses: identical rounding everywhere
__device__ __forceinline__ f32x4 bn_val(const f32x4 x, const f32x4 mu, const f32x4 is, const f32x4 ga, const f32x4 be) {
  f32x4 r;
#pragma unroll
  for (int e = 0; e < 4; ++e) r[e] = bn_val1(x[e], mu[e], is[e], ga[e], be[e]);
  return r;
}

__global__ __launch_bounds__(256) void bn_apply_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                        const float* __restrict__ invstd,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        const float* residual, float* out, size_t n4, int c4n, int relu) {
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n4; idx += (size_t)gridDim.x * blockDim.x) {
    const int cg = (int)(idx % c4n);
    const f32x4 mu = chan4(mean, cg), is = chan4(invstd, cg), ga = chan4(gamma, cg), be = chan4(beta, cg);
    f32x4 v = bn_val(reinterpret_cast<const f32x4*>(x)[idx], mu, is, ga, be);
    if (residual) v += reinterpret_cast<const f32x4*>(residual)[idx];
    if (relu) {   // NaN kept, as torch.relu and bn_relu_maxpool_fwd_kernel keep it (fmaxf alone answers 0)
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = v[e] != v[e] ? v[e] : fmaxf(v[e], 0.f);
    }
    reinterpret_cast<f32x4*>(out)[idx] = v;
  }
}

// dx may alias dout (in place): every element is read before it is written by the same thread.
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* dout, const float* __restrict__ relu_out,
                                                            const float* __restrict__ x, const float* __restrict__ mean,
                                                            const float* __restrict__ invstd,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ dgamma,
                                                            const float* __restrict__ dbeta, float* dx, float* g_out,
                                                            size_t n4, int c4n, float invM) {
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n4; idx += (size_t)gridDim.x * blockDim.x) {
    const int cg = (int)(idx % c4n);
    const f32x4 mu = chan4(mean, cg), is = chan4(invstd, cg), ga = chan4(gamma, cg);
    const f32x4 dg = chan4(dgamma, cg) * invM, db = chan4(dbeta, cg) * invM;
    f32x4 g = reinterpret_cast<const f32x4*>(dout)[idx];
    if (relu_out) {
      const f32x4 o = reinterpret_cast<const f32x4*>(relu_out)[idx];
#pragma unroll
      for (int e = 0; e < 4; ++e) g[e] = o[e] > 0.f ? g[e] : 0.f;
    }
    const f32x4 xhat = (reinterpret_cast<const f32x4*>(x)[idx] - mu) * is;
    if (g_out) reinterpret_cast<f32x4*>(g_out)[idx] = g;
    reinterpret_cast<f32x4*>(dx)[idx] = ga * is * (g - db - xhat * dg);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Stem: conv1 -> bn1 -> relu -> maxpool(3, 2, 1) (backbone.py:149-152).  The stem activations are the largest tensors of the
// network (N x 112 x 112 x 64 resp. N x 512 x 64 x 64: 1.15 GB per pass at batch 64), and everything around them is
// HBM-bound, so the ReLU output is never materialised:
//   forward   mla_bn_relu_maxpool_fwd: the max-pool reads y (the conv output) and applies BN + ReLU on the fly
//             (saves writing and re-reading a_stem: 2.3 GB per step);
//   backward  mla_bn_bwd_pooled: the BatchNorm backward takes its upstream gradient straight from the POOLED gradient --
//             g[pixel] = [bn(y) > 0] * sum over the <= 4 windows that selected this pixel -- in its reduction pass (as a sum
//             over pooled outputs) and in its apply pass (saves writing and twice re-reading the scattered gradient and reading a_stem: 4.2 GB per step).
// bn_val (above) is the one expression both directions use, so the recomputed ReLU mask and the max-pool decisions agree
// bit for bit.
// ---------------------------------------------------------------------------------------------------------------------

// idx = kh*3+kw of the FIRST maximum in row-major window order (ATen: `val > maxval || isnan(val)`), as maxpool_fwd_kernel.
// A thread forms a 2x2 block of pooled outputs from the 5x5 input pixels they cover (25 loads and BN evaluations instead of
// 36), walking the input rows top to bottom so that every output still sees its window in row-major order.
__global__ __launch_bounds__(256) void bn_relu_maxpool_fwd_kernel(const float* __restrict__ y, const float* __restrict__ mean,
                                                                   const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                                   const float* __restrict__ beta, float* __restrict__ out,
                                                                   uint8_t* __restrict__ idx, int N, int H, int W, int C, int OH, int OW) {
  const int c4n = C >> 2, QH = (OH + 1) >> 1, QW = (OW + 1) >> 1;
  const size_t total = (size_t)N * QH * QW * c4n;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int cg = (int)(i % c4n);
    size_t p = i / c4n;
    const int oxq = (int)(p % QW); p /= QW;
    const int oyq = (int)(p % QH);
    const int n = (int)(p / QH);
    const f32x4 mu = chan4(mean, cg), is = chan4(invstd, cg), ga = chan4(gamma, cg), be = chan4(beta, cg);
    f32x4 best[2][2];
    int bi[2][2][4];
    bool first[2][2];
#pragma unroll
    for (int qy = 0; qy < 2; ++qy)
#pragma unroll
      for (int qx = 0; qx < 2; ++qx) {
        best[qy][qx] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        first[qy][qx] = true;
#pragma unroll
        for (int e = 0; e < 4; ++e) bi[qy][qx][e] = 0;
      }
    const int iy0 = oyq * 4 - 1, ix0 = oxq * 4 - 1;          // first input row / column of the 5x5 patch
#pragma unroll
    for (int r = 0; r < 5; ++r) {
      const int iy = iy0 + r;
      if ((unsigned)iy >= (unsigned)H) continue;
      f32x4 v[5];
      bool ok[5];
#pragma unroll
      for (int c = 0; c < 5; ++c) {
        const int ix = ix0 + c;
        ok[c] = (unsigned)ix < (unsigned)W;
        v[c] = ok[c] ? reinterpret_cast<const f32x4*>(y)[((size_t)(n * H + iy) * W + ix) * c4n + cg] : f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int c = 0; c < 5; ++c) {
        v[c] = bn_val(v[c], mu, is, ga, be);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[c][e] = v[c][e] != v[c][e] ? v[c][e] : fmaxf(v[c][e], 0.f);   // relu, NaN kept
      }
#pragma unroll
      for (int qy = 0; qy < 2; ++qy) {
        const int kh = r - 2 * qy;                            // row of output qy's window
        if (kh < 0 || kh > 2) continue;
#pragma unroll
        for (int qx = 0; qx < 2; ++qx)
#pragma unroll
          for (int kw = 0; kw < 3; ++kw) {
            const int c = 2 * qx + kw;
            if (!ok[c]) continue;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float ve = v[c][e];
              if (first[qy][qx] || ve > best[qy][qx][e] || ve != ve) {
                best[qy][qx][e] = ve;
                bi[qy][qx][e] = kh * 3 + kw;
              }
            }
            first[qy][qx] = false;
          }
      }
    }
#pragma unroll
    for (int qy = 0; qy < 2; ++qy)
#pragma unroll
      for (int qx = 0; qx < 2; ++qx) {
        const int oy = oyq * 2 + qy, ox = oxq * 2 + qx;
        if (oy >= OH || ox >= OW) continue;
        const size_t o = ((size_t)(n * OH + oy) * OW + ox) * c4n + cg;
        reinterpret_cast<f32x4*>(out)[o] = best[qy][qx];
        reinterpret_cast<uchar4*>(idx)[o] = make_uchar4(bi[qy][qx][0], bi[qy][qx][1], bi[qy][qx][2], bi[qy][qx][3]);
      }
  }
}

// The reduction pass in scatter form: sum_pixels g = sum over POOLED outputs o of dpool[o] * [bn(y[sel(o)]) > 0] (every pooled output
// selected exactly one pixel per channel), likewise sum g * xhat -- a quarter of the iterations of the per-pixel gather form and
// 6 loads per thread instead of 9.  Tiles are rows of pooled pixels; partial layout as bn_reduce_kernel<1>.
__global__ __launch_bounds__(256) void bn_bwd_pooled_reduce_kernel(const float* __restrict__ dpool, const uint8_t* __restrict__ idx,
                                                                    const float* __restrict__ y, const float* __restrict__ mean,
                                                                    const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                                    const float* __restrict__ beta, float* __restrict__ out, int N, int H,
                                                                    int W, int C, int OH, int OW, int tile_rows) {
  const int c4n = C >> 2, MP = N * OH * OW;
  const int cg = threadIdx.x % c4n, rl = threadIdx.x / c4n, nrl = 256 / c4n;
  const int r0 = blockIdx.x * tile_rows, r1 = min(MP, r0 + tile_rows);
  const f32x4 mu = chan4(mean, cg), is = chan4(invstd, cg), ga = chan4(gamma, cg), be = chan4(beta, cg);
  f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
  for (int r = r0 + rl; r < r1; r += nrl) {
    const int ox = r % OW, t = r / OW, oy = t % OH, n = t / OH;
    const size_t o = (size_t)r * c4n + cg;
    const f32x4 g = reinterpret_cast<const f32x4*>(dpool)[o];
    const uchar4 sel = reinterpret_cast<const uchar4*>(idx)[o];
    const int code[4] = {sel.x, sel.y, sel.z, sel.w};
    f32x4 xv;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int kh = (code[e] * 11) >> 5, kw = code[e] - 3 * kh;      // code = kh * 3 + kw, 0..8
      xv[e] = y[((size_t)(n * H + oy * 2 - 1 + kh) * W + (ox * 2 - 1 + kw)) * C + cg * 4 + e];
    }
    const f32x4 a = bn_val(xv, mu, is, ga, be);
    const f32x4 xhat = (xv - mu) * is;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float ge = a[e] > 0.f ? g[e] : 0.f;
      s0[e] += ge;
      s1[e] += ge * xhat[e];
    }
  }
  bn_store_tile_sums(s0, s1, out, C, cg, rl, nrl);
}

// The apply pass: dy = gamma * invstd * (g - db/M - xhat * dg/M).  A thread owns the 2x2 pixel quad (2a + py, 2b + px): its
// pixels lie in the four windows (a | a+1, b | b+1) only, at window positions that are compile-time constants --
//   (0,0): (a,b) code 4;   (0,1): (a,b) 5, (a,b+1) 3;   (1,0): (a,b) 7, (a+1,b) 1;   (1,1): (a,b) 8, (a,b+1) 6, (a+1,b) 2, (a+1,b+1) 0
// -- so the pooled gradient and the index bytes of each window are loaded once per quad (4 + 4 loads for 4 pixels instead of
// up to 8 per pixel in the per-pixel gather form).
__global__ __launch_bounds__(256) void bn_bwd_pooled_apply_kernel(const float* __restrict__ dpool, const uint8_t* __restrict__ idx,
                                                                   const float* __restrict__ y, const float* __restrict__ mean,
                                                                   const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                                   const float* __restrict__ beta, const float* __restrict__ dgamma,
                                                                   const float* __restrict__ dbeta, float* __restrict__ out, int N, int H,
                                                                   int W, int C, int OH, int OW) {
  const int c4n = C >> 2, QH = (H + 1) >> 1, QW = (W + 1) >> 1;
  const size_t total = (size_t)N * QH * QW * c4n;
  const float invM = bn_inv_count(N, H, W);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int cg = (int)(i % c4n);
    size_t p = i / c4n;
    const int b = (int)(p % QW); p /= QW;
    const int a = (int)(p % QH);
    const int n = (int)(p / QH);
    const f32x4 mu = chan4(mean, cg), is = chan4(invstd, cg), ga = chan4(gamma, cg), be = chan4(beta, cg);
    const f32x4 dgs = chan4(dgamma, cg), dbs = chan4(dbeta, cg);
    f32x4 dg, db;
#pragma unroll
    for (int e = 0; e < 4; ++e) { dg[e] = bn_bwd_scale(dgs[e], invM); db[e] = bn_bwd_scale(dbs[e], invM); }
    f32x4 wg[2][2];                    // pooled gradient of window (a + wy, b + wx); zero outside the pooled grid
    int ws[2][2][4];                   // its selected positions; -1 outside
#pragma unroll
    for (int wy = 0; wy < 2; ++wy)
#pragma unroll
      for (int wx = 0; wx < 2; ++wx) {
        const int oy = a + wy, ox = b + wx;
        if (oy < OH && ox < OW) {
          const size_t o = ((size_t)(n * OH + oy) * OW + ox) * c4n + cg;
          wg[wy][wx] = reinterpret_cast<const f32x4*>(dpool)[o];
          const uchar4 s = reinterpret_cast<const uchar4*>(idx)[o];
          ws[wy][wx][0] = s.x; ws[wy][wx][1] = s.y; ws[wy][wx][2] = s.z; ws[wy][wx][3] = s.w;
        } else {
          wg[wy][wx] = f32x4{0.f, 0.f, 0.f, 0.f};
          ws[wy][wx][0] = ws[wy][wx][1] = ws[wy][wx][2] = ws[wy][wx][3] = -1;
        }
      }
#pragma unroll
    for (int py = 0; py < 2; ++py)
#pragma unroll
      for (int px = 0; px < 2; ++px) {
        const int iy = 2 * a + py, ix = 2 * b + px;
        if (iy >= H || ix >= W) continue;
        f32x4 g = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int wy = 0; wy <= py; ++wy)             // window row a + wy covers pixel row 2a + py at kh = py + 1 - 2 wy
#pragma unroll
          for (int wx = 0; wx <= px; ++wx) {
            const int code = (py + 1 - 2 * wy) * 3 + (px + 1 - 2 * wx);
#pragma unroll
            for (int e = 0; e < 4; ++e) g[e] = pool_pick(g[e], ws[wy][wx][e], code, wg[wy][wx][e]);
          }
        const size_t o = ((size_t)(n * H + iy) * W + ix) * c4n + cg;
        const f32x4 xv = reinterpret_cast<const f32x4*>(y)[o];
        f32x4 r;                       // (the shared expression: the fused stem weight gradient forms the same bits)
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = bn_bwd_pooled_dy1(xv[e], g[e], mu[e], is[e], ga[e], be[e], dg[e], db[e]);
        reinterpret_cast<f32x4*>(out)[o] = r;
      }
  }
}

// bn_check: pool_args.h
static int ew_grid(size_t n4) { return pool_capped_grid(n4, BN_EW_MAX_BLOCKS); }

// the backward sums partial[tiles][2][C] (fp32, scratch tail behind them) -> dgamma, dbeta
static int bn_bwd_finalize(const float* partial, int tiles, int M, int C, float* dgamma, float* dbeta, hipStream_t st) {
  return bn_finalize_partials<float, 0>(partial, tiles, M, C, 0.f, 0.f, dgamma, dbeta, nullptr, nullptr, st);
}

// the apply pass of the two plain backward entry points
static int bn_bwd_apply(const float* dout, const float* relu_out, const float* x, const float* mean, const float* invstd,
                        const float* gamma, const float* dgamma, const float* dbeta, float* dx, float* g_out, int M, int C,
                        hipStream_t st) {
  const size_t n4 = (size_t)M * C / 4;
  bn_bwd_apply_kernel<<<ew_grid(n4), 256, 0, st>>>(dout, relu_out, x, mean, invstd, gamma, dgamma, dbeta, dx, g_out, n4, C / 4,
                                                   1.0f / (float)M);
  MLA_CHECK_LAUNCH("bn_bwd_apply_kernel");
  return MLA_OK;
}

extern "C" int mla_bn_stats_partial(const float* x, int M, int C, float* partial, int* tiles, void* stream) {
  if (int rc = bn_check("mla_bn_stats_partial", M, C)) return rc;
  MLA_REQUIRE(x && partial, "mla_bn_stats_partial: null pointer");
  const int tr = bn_tile_rows(M), nt = cdiv(M, tr);
  bn_reduce_kernel<0><<<nt, 256, 0, (hipStream_t)stream>>>(x, nullptr, nullptr, nullptr, nullptr, partial, M, C, tr);
  MLA_CHECK_LAUNCH("bn_reduce_kernel<0>");
  if (tiles) *tiles = nt;
  return MLA_OK;
}

extern "C" int mla_bn_finalize(const float* partial, int tiles, int M, int C, float eps, float momentum, float* mean,
                               float* invstd, float* running_mean, float* running_var, void* stream) {
  MLA_REQUIRE(partial && mean && invstd && tiles > 0 && M > 0 && C > 0, "mla_bn_finalize: bad argument");
  MLA_REQUIRE((running_mean == nullptr) == (running_var == nullptr), "mla_bn_finalize: running stats must come in pairs");
  MLA_REQUIRE(((uintptr_t)partial % 8) == 0, "mla_bn_finalize: partial must be 8-byte aligned");
  const double* pd = reinterpret_cast<const double*>(partial);                     // fp64 [tiles][2][C] (conv epilogue / bn_stats_partial)
  return bn_finalize_partials<double, 1>(pd, tiles, M, C, eps, momentum, mean, invstd, running_mean, running_var, (hipStream_t)stream);
}

extern "C" int mla_bn_apply(const float* x, const float* mean, const float* invstd, const float* gamma,
                            const float* beta, const float* residual, float* out, int M, int C, int relu, void* stream) {
  if (int rc = bn_check("mla_bn_apply", M, C)) return rc;
  MLA_REQUIRE(x && mean && invstd && gamma && beta && out, "mla_bn_apply: null pointer");
  const size_t n4 = (size_t)M * C / 4;
  bn_apply_kernel<<<ew_grid(n4), 256, 0, (hipStream_t)stream>>>(x, mean, invstd, gamma, beta, residual, out, n4, C / 4, relu);
  MLA_CHECK_LAUNCH("bn_apply_kernel");
  return MLA_OK;
}

extern "C" int mla_bn_bwd(const float* dout, const float* relu_out, const float* x, const float* mean,
                          const float* invstd, const float* gamma, float* dx, float* dgamma, float* dbeta, float* g_out,
                          float* ws, int M, int C, void* stream) {
  if (int rc = bn_check("mla_bn_bwd", M, C)) return rc;
  MLA_REQUIRE(dout && x && mean && invstd && gamma && dx && dgamma && dbeta && ws, "mla_bn_bwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int tr = bn_tile_rows(M), nt = cdiv(M, tr);
  bn_reduce_kernel<1><<<nt, 256, 0, st>>>(x, dout, relu_out, mean, invstd, ws, M, C, tr);
  MLA_CHECK_LAUNCH("bn_reduce_kernel<1>");
  if (int rc = bn_bwd_finalize(ws, nt, M, C, dgamma, dbeta, st)) return rc;
  return bn_bwd_apply(dout, relu_out, x, mean, invstd, gamma, dgamma, dbeta, dx, g_out, M, C, st);
}

// BatchNorm backward whose reduction pass was done by the producer of dout (mla_conv2d_dgrad[_split]_bn): finalize the
// `tiles` per-tile sums of `partial` (its scratch tail follows the tiles) into dgamma / dbeta, then the apply pass.
extern "C" int mla_bn_bwd_from_partial(const float* dout, const float* x, const float* mean, const float* invstd,
                                       const float* gamma, float* dx, float* dgamma, float* dbeta, float* partial, int tiles,
                                       int M, int C, void* stream) {
  if (int rc = bn_check("mla_bn_bwd_from_partial", M, C)) return rc;
  MLA_REQUIRE(dout && x && mean && invstd && gamma && dx && dgamma && dbeta && partial && tiles > 0,
              "mla_bn_bwd_from_partial: null pointer or no tiles");
  hipStream_t st = (hipStream_t)stream;
  if (int rc = bn_bwd_finalize(partial, tiles, M, C, dgamma, dbeta, st)) return rc;
  return bn_bwd_apply(dout, nullptr, x, mean, invstd, gamma, dgamma, dbeta, dx, nullptr, M, C, st);
}

extern "C" int mla_bn_relu_maxpool_fwd(const float* y, const float* mean, const float* invstd, const float* gamma, const float* beta,
                                       float* out, uint8_t* idx, int N, int H, int W, int C, void* stream) {
  PoolPlan p;
  MLA_TRY(bn_relu_maxpool_fwd_plan(y, mean, invstd, gamma, beta, out, idx, N, H, W, C, &p));
  bn_relu_maxpool_fwd_kernel<<<p.grid, 256, 0, (hipStream_t)stream>>>(y, mean, invstd, gamma, beta, out, idx, N, H, W, C, p.OH, p.OW);
  MLA_CHECK_LAUNCH("bn_relu_maxpool_fwd_kernel");
  return MLA_OK;
}

extern "C" int mla_bn_bwd_pooled(const float* dpool, const uint8_t* idx, const float* y, const float* mean, const float* invstd,
                                 const float* gamma, const float* beta, float* dy, float* dgamma, float* dbeta, float* ws, int N,
                                 int H, int W, int C, void* stream) {
  PooledBwdPlan p;
  MLA_TRY(bn_bwd_pooled_plan(dpool, idx, y, mean, invstd, gamma, beta, dgamma, dbeta, ws, N, H, W, C, &p));
  hipStream_t st = (hipStream_t)stream;
  // reduction: p.tiles tiles of pooled pixels, one partial row each -- never more than the bn_ws_tiles(M) rows that ws holds
  // (bn_pooled_tiles enlarges the tile where the tile rule of MP alone would give more)
  bn_bwd_pooled_reduce_kernel<<<p.tiles, 256, 0, st>>>(dpool, idx, y, mean, invstd, gamma, beta, ws, N, H, W, C, p.OH, p.OW, p.tile_rows);
  MLA_CHECK_LAUNCH("bn_bwd_pooled_reduce_kernel");
  if (int rc = bn_bwd_finalize(ws, p.tiles, p.M, C, dgamma, dbeta, st)) return rc;
  if (!dy) return MLA_OK;            // reduction half only: the consumer of dy forms it itself (mla_conv2d_stem_wgrad_split_bnpool)
  bn_bwd_pooled_apply_kernel<<<p.grid, 256, 0, st>>>(dpool, idx, y, mean, invstd, gamma, beta, dgamma, dbeta, dy, N, H, W, C, p.OH, p.OW);
  MLA_CHECK_LAUNCH("bn_bwd_pooled_apply_kernel");
  return MLA_OK;
}
