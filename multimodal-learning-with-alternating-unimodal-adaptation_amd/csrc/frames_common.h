// What frames.hip (descriptors made and checked on the host) and resident.hip (descriptors drawn on the device) share: Pillow's
// coefficient arithmetic, the LDS plan and the resample body.  The first half is plain C++ with no HIP in it, so the host halves
// (resident_args.h, resident_host_check.cpp) build it with the host sanitizers; the kernels' half needs hipcc.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define FR_HD __host__ __device__
#else
#define FR_HD
#endif

#define FR_THREADS 256
#define FR_BAND 16                 // output rows per workgroup (halved by the planner until the LDS budget fits)
#define FR_LDS_MAX 65536
#define FR_DIM_MAX 65536

#define FR_BILINEAR 0
#define FR_BICUBIC 1

// Pillow's filters (libImaging/Resample.c bilinear_filter / bicubic_filter), same expressions
template <int FILTER>
FR_HD static inline double fr_filter(double x) {
#pragma clang fp contract(off)
  if (x < 0.0) x = -x;
  if (FILTER == FR_BILINEAR) return x < 1.0 ? 1.0 - x : 0.0;
  const double a = -0.5;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

// Pillow precompute_coeffs() bounds and (optionally) normalize_coeffs_8bpc() weights of output index xx for a resize of `in`
// samples to `out` (box = the whole input: torchvision crops first, so the filter clamps to the crop).
template <int FILTER>
FR_HD static inline void fr_coeffs(int in, int out, int xx, int* xmin_out, int* xmax_out, int* k) {
#pragma clang fp contract(off)
  const double scale = (double)in / out;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = (FILTER == FR_BICUBIC ? 2.0 : 1.0) * filterscale;
  const double center = (xx + 0.5) * scale;
  const double ss = 1.0 / filterscale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > in) xmax = in;
  xmax -= xmin;
  *xmin_out = xmin;
  *xmax_out = xmax;
  if (!k) return;
  // two sweeps instead of Pillow's stored double array: the weights are recomputed bit-identically (same expression)
  double ww = 0.0;
  for (int x = 0; x < xmax; ++x) ww += fr_filter<FILTER>((x + xmin - center + 0.5) * ss);
  for (int x = 0; x < xmax; ++x) {
    double w = fr_filter<FILTER>((x + xmin - center + 0.5) * ss);
    if (ww != 0.0) w /= ww;
    k[x] = (int)(w < 0.0 ? -0.5 + w * (1 << 22) : 0.5 + w * (1 << 22));
  }
}
static inline void fr_bounds(int filter, int in, int out, int xx, int* xmin, int* xmax) {
  if (filter == FR_BICUBIC) fr_coeffs<FR_BICUBIC>(in, out, xx, xmin, xmax, nullptr);
  else fr_coeffs<FR_BILINEAR>(in, out, xx, xmin, xmax, nullptr);
}

static inline int fr_ksize(int filter, int in, int out) {   // Pillow: (int)ceil(support) * 2 + 1
  const double scale = (double)in / out;
  return (int)ceil((filter == FR_BICUBIC ? 2.0 : 1.0) * (scale < 1.0 ? 1.0 : scale)) * 2 + 1;
}

struct FramePlan {
  int band, rows_cap, kh, kv;
  size_t lds;
};

// LDS layout (bytes, each part 16-byte aligned): lut f32[3*256] | hk i32[OW*kh] | hb i32[OW*2] | vk i32[band*kv] |
// vb i32[band*2] | tmp u8[rows_cap*OW*3]
FR_HD static inline size_t fr_al(size_t b) { return (b + 15) & ~(size_t)15; }
static inline size_t fr_lds(int OW, int band, int rows_cap, int kh, int kv) {
  return fr_al(3 * 256 * 4) + fr_al((size_t)OW * kh * 4) + fr_al((size_t)OW * 8) + fr_al((size_t)band * kv * 4) +
         fr_al((size_t)band * 8) + fr_al((size_t)rows_cap * OW * 3);
}

#ifdef __HIPCC__
#include "common.h"

__device__ __forceinline__ int fr_clip8(int acc) {
  acc >>= 22;
  return acc < 0 ? 0 : (acc > 255 ? 255 : acc);
}

// ---- ColorJitter (mla_image_augment): Pillow's ImageEnhance on one pixel ----------------------------------------------------
#define FR_JIT_COLS 7              // jitter descriptor: n_ops, op0, op1, op2, brightness / contrast / saturation factor bits
#define FR_BRIGHTNESS 0            // operation ids: torchvision ColorJitter's fn_id
#define FR_CONTRAST 1
#define FR_SATURATION 2

struct FrJitter {
  int n, op[3];
  float f[3];                      // f[q] = the factor of op[q]
};

__device__ __forceinline__ FrJitter fr_jitter_load(const int64_t* __restrict__ j) {
  FrJitter jt;
  jt.n = min(max((int)j[0], 0), 3);               // the host checked the table; the clamps only bound a corrupted one
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    jt.op[q] = min(max((int)j[1 + q], 0), 2);
    jt.f[q] = __uint_as_float((unsigned)j[4 + jt.op[q]]);
  }
  return jt;
}

// index of contrast in the operation list, n when it is absent: operations [0, at) run before the reduction, [at, n) after
__device__ __forceinline__ int fr_contrast_at(const FrJitter& jt) {
  int at = jt.n;
#pragma unroll
  for (int q = 2; q >= 0; --q)
    if (q < jt.n && jt.op[q] == FR_CONTRAST) at = q;
  return at;
}

__device__ __forceinline__ int fr_luma(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

// Pillow ImagingBlend on one byte: (uint8)(d + a * (x - d)) in fp32, product and sum rounded separately: contraction is switched
// off here (hipcc's __fmul_rn / __fadd_rn are plain operators and fuse into v_fma_f32, which changes bytes); clipped when a leaves
// [0, 1].  For a in [0, 1] t lies between d and x, so the clip is the plain truncation.
__device__ __forceinline__ int fr_blend(int d, int x, float a) {
#pragma clang fp contract(off)
  const float p = a * (float)(x - d);
  const float t = (float)d + p;
  return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}

// m: the mean luma (contrast only)
__device__ __forceinline__ void fr_enhance(int op, float a, int m, int& r, int& g, int& b) {
  const int d = op == FR_BRIGHTNESS ? 0 : (op == FR_CONTRAST ? m : fr_luma(r, g, b));
  r = fr_blend(d, r, a);
  g = fr_blend(d, g, a);
  b = fr_blend(d, b, a);
}

// DW = descriptor columns: 8 (offset, H, W, top, left, ch, cw, flip; full = out, window at 0) or 12 (+ full_h, full_w, win_top,
// win_left)
// AUG: the epilogue of mla_image_augment's first launch (jit / staging / partials; lut and out unused) instead of the LUT
template <int FILTER, int DW, bool AUG>
__device__ __forceinline__ void fr_body(const uint8_t* __restrict__ src, const int64_t* __restrict__ desc,
                                        const float* __restrict__ lut, float* __restrict__ out, const int64_t* __restrict__ jit,
                                        uint8_t* __restrict__ staging, int64_t* __restrict__ partials, int T, int OH, int OW,
                                        int band, int rows_cap, int kh, int kv) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fr_smem[];
  float* s_lut = reinterpret_cast<float*>(fr_smem);
  int* hk = reinterpret_cast<int*>(fr_smem + fr_al(3 * 256 * 4));
  int* hb = reinterpret_cast<int*>(reinterpret_cast<unsigned char*>(hk) + fr_al((size_t)OW * kh * 4));
  int* vk = reinterpret_cast<int*>(reinterpret_cast<unsigned char*>(hb) + fr_al((size_t)OW * 8));
  int* vb = reinterpret_cast<int*>(reinterpret_cast<unsigned char*>(vk) + fr_al((size_t)band * kv * 4));
  uint8_t* tmp = reinterpret_cast<uint8_t*>(vb) + fr_al((size_t)band * 8);

  const int tid = threadIdx.x;
  const int n = blockIdx.y;
  const int y0 = blockIdx.x * band;
  const int nb = min(band, OH - y0);
  const int64_t* d = desc + (size_t)n * DW;
  const size_t off = (size_t)d[0];
  const int W = (int)d[2], top = (int)d[3], left = (int)d[4], ch = (int)d[5], cw = (int)d[6];
  const bool flip = d[7] != 0;
  const int full_h = DW == 12 ? (int)d[8] : OH, full_w = DW == 12 ? (int)d[9] : OW;
  const int win_top = DW == 12 ? (int)d[10] : 0, win_left = DW == 12 ? (int)d[11] : 0;

  if (!AUG)
    for (int i = tid; i < 3 * 256; i += FR_THREADS) s_lut[i] = lut[i];
  for (int xx = tid; xx < OW; xx += FR_THREADS)
    fr_coeffs<FILTER>(cw, full_w, win_left + xx, &hb[2 * xx], &hb[2 * xx + 1], hk + (size_t)xx * kh);
  for (int yy = tid; yy < nb; yy += FR_THREADS)
    fr_coeffs<FILTER>(ch, full_h, win_top + y0 + yy, &vb[2 * yy], &vb[2 * yy + 1], vk + (size_t)yy * kv);
  __syncthreads();

  // source rows [r0, r0 + nrows) of the crop feed this band (bounds are monotone in the output index); the host planner
  // sized rows_cap from the same bounds, the min() only keeps a corrupted descriptor inside LDS
  const int r0 = vb[0];
  const int nrows = min(vb[2 * (nb - 1)] + vb[2 * (nb - 1) + 1] - r0, rows_cap);

  // horizontal pass -> tmp[r][xx][c] (uint8, Pillow's intermediate image)
  for (int i = tid; i < nrows * OW; i += FR_THREADS) {
    const int r = i / OW, xx = i - r * OW;
    const uint8_t* row = src + off + ((size_t)(top + r0 + r) * W + left) * 3;
    const int xmin = hb[2 * xx], xmax = hb[2 * xx + 1];
    const int* k = hk + (size_t)xx * kh;
    int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
    const uint8_t* p = row + (size_t)xmin * 3;
    for (int x = 0; x < xmax; ++x, p += 3) {
      const int w = k[x];
      a0 += (int)p[0] * w;
      a1 += (int)p[1] * w;
      a2 += (int)p[2] * w;
    }
    uint8_t* t = tmp + (size_t)i * 3;
    t[0] = (uint8_t)fr_clip8(a0);
    t[1] = (uint8_t)fr_clip8(a1);
    t[2] = (uint8_t)fr_clip8(a2);
  }
  __syncthreads();

  // vertical pass, flip, LUT; consecutive threads write consecutive (or, flipped, mirrored) columns of one row
  const int b = n / T, tt = n - b * T;
  const size_t plane = (size_t)OH * OW, cstride = (size_t)T * plane;
  float* o = AUG ? nullptr : out + (size_t)b * 3 * cstride + (size_t)tt * plane;
  FrJitter jt;
  int npre = 0, lsum = 0;
  if (AUG) {
    jt = fr_jitter_load(jit + (size_t)n * FR_JIT_COLS);
    npre = fr_contrast_at(jt);
  }
  for (int i = tid; i < nb * OW; i += FR_THREADS) {
    const int yy = i / OW, xx = i - yy * OW;
    const int ymin = vb[2 * yy] - r0, ymax = vb[2 * yy + 1];
    const int* k = vk + (size_t)yy * kv;
    int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
    const uint8_t* p = tmp + ((size_t)ymin * OW + xx) * 3;
    for (int y = 0; y < ymax; ++y, p += (size_t)OW * 3) {
      const int w = k[y];
      a0 += (int)p[0] * w;
      a1 += (int)p[1] * w;
      a2 += (int)p[2] * w;
    }
    const size_t po = (size_t)(y0 + yy) * OW + (flip ? OW - 1 - xx : xx);
    if (AUG) {
      int r = fr_clip8(a0), g = fr_clip8(a1), bl = fr_clip8(a2);
#pragma unroll
      for (int q = 0; q < 3; ++q)
        if (q < npre) fr_enhance(jt.op[q], jt.f[q], 0, r, g, bl);
      lsum += fr_luma(r, g, bl);
      uint8_t* s = staging + ((size_t)n * plane + po) * 3;
      s[0] = (uint8_t)r;
      s[1] = (uint8_t)g;
      s[2] = (uint8_t)bl;
    } else {
      o[po] = s_lut[fr_clip8(a0)];
      o[cstride + po] = s_lut[256 + fr_clip8(a1)];
      o[2 * cstride + po] = s_lut[512 + fr_clip8(a2)];
    }
  }
  if (AUG) {
    // luma sum of the band: a thread holds at most band * OW / 256 <= 256 pixels of <= 255, a workgroup < 2^24; hk is free since
    // the horizontal pass (the barrier above) and holds at least 5 ints
#pragma unroll
    for (int o2 = 32; o2 > 0; o2 >>= 1) lsum += __shfl_xor(lsum, o2, 64);
    if ((tid & 63) == 0) hk[tid >> 6] = lsum;
    __syncthreads();
    if (tid == 0) {
      int64_t sum = 0;
      for (int w = 0; w < FR_THREADS / 64; ++w) sum += hk[w];
      partials[(size_t)n * gridDim.x + blockIdx.x] = sum;
    }
  }
}
#endif  // __HIPCC__
