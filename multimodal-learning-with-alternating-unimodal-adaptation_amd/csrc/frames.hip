// CREMA-D frame augmentation (dataset/dataset.py:128-153), gfx950: crop -> bilinear resize -> horizontal flip -> ToTensor +
// Normalize of a batch of decoded uint8 RGB frames, bit-identical to PIL + torchvision on the host.
//
//   PIL  img.crop((left, top, left+cw, top+ch)).resize((OW, OH), BILINEAR)      RandomResizedCrop / Resize((224, 224))
//   PIL  .transpose(FLIP_LEFT_RIGHT) if flip                                     RandomHorizontalFlip
//   LUT  lut[c][u8] = (u8 / 255 - mean[c]) / std[c], built with torch's CPU ops  ToTensor + Normalize
//
// Pillow's 8-bit resample (libImaging/Resample.c) is separable: a horizontal pass over every source row the vertical pass
// needs, clipped to uint8, then a vertical pass, both in 22-bit fixed point (acc = 2^21 + sum u8 * k; clamp(acc >> 22)).
// The integer coefficients come from double-precision triangle weights normalised by their sum; they are recomputed here
// with the exact operation order of Pillow's precompute_coeffs / normalize_coeffs_8bpc and FP contraction off (an FMA in
// `(xx + 0.5) * scale` or `0.5 + w * 2^22` changes the last bit and with it some pixels).
//
// One workgroup per (frame, band of output rows): coefficients of all output columns and of the band's rows into LDS, the
// horizontal pass of the source rows the band reads into LDS (uint8), then the vertical pass, flip and LUT, written as
// coalesced fp32 rows straight into the (B, 3, T, OH, OW) batch (frame n = sample n / T, time slot n % T).  No atomics.
//
// mla_image_resample is the same kernel with two more degrees of freedom (CAVDataset, dataset/dataset.py:251-256, and the
// M3AE / Food-101 eval transform, dataset.py:413-420: Resize(size, BICUBIC) + CenterCrop(size)):
//   filter   0 = bilinear (support 1), 1 = Pillow's bicubic (a = -0.5, support 2; negative coefficients round away from zero)
//   window   the crop is resized to full_h x full_w and only the out_h x out_w window at (win_top, win_left) of that image is
//            computed: the coefficients are those of output indices win_left + xx / win_top + yy of a cw -> full_w /
//            ch -> full_h resize, so a CenterCrop costs nothing and reads only the source rows its window needs.
// mla_frames_resample is the instantiation <bilinear, 8-column descriptor> with full = out and a zero window offset.
//
// mla_image_augment is the M3AE / Food-101 TRAIN transform (dataset/dataset.py:401-412: timm create_transform with
// color_jitter=True, i.e. torchvision ColorJitter(1, 1, 1) between the flip and ToTensor).  Brightness, saturation and contrast
// are Pillow's ImageEnhance: Image.blend(degenerate, image, factor) per byte in fp32 without contraction, truncated (clipped
// when the factor leaves [0, 1]) to uint8 after EACH operation, applied in a drawn order.  The degenerate image is 0
// (brightness), the pixel's own luma L = (R*19595 + G*38470 + B*7471 + 0x8000) >> 16 (saturation) or the rounded mean luma m
// of the whole image as it is when contrast is applied.  Two launches, integer reductions only:
//   frames_augment_kernel   the bicubic instantiation of the resample body; its epilogue applies the flip and the operations that
//                           precede contrast, writes the uint8 image to a staging buffer (N, OH, OW, 3) and the int64 luma sum of
//                           its band into partials[n * bands + band] (one slot per workgroup: no atomics, no grid-order dependence)
//   frames_jitter_kernel    one pixel per thread: m = (2 S + n) / (2 n) from the image's partials (= int(S / n + 0.5)), contrast and
//                           the operations after it, LUT, coalesced fp32 stores
#include <algorithm>
#include <math.h>
#include <string.h>
#include <cmath>
#include "common.h"
#include "frames_common.h"        // fr_body, fr_bounds, fr_ksize, fr_lds, FramePlan: shared with resident.hip

template <int FILTER, int DW>
__global__ __launch_bounds__(FR_THREADS) void frames_resample_kernel(const uint8_t* __restrict__ src,
                                                                      const int64_t* __restrict__ desc,
                                                                      const float* __restrict__ lut, float* __restrict__ out,
                                                                      int T, int OH, int OW, int band, int rows_cap, int kh,
                                                                      int kv) {
  fr_body<FILTER, DW, false>(src, desc, lut, out, nullptr, nullptr, nullptr, T, OH, OW, band, rows_cap, kh, kv);
}

__global__ __launch_bounds__(FR_THREADS) void frames_augment_kernel(const uint8_t* __restrict__ src,
                                                                     const int64_t* __restrict__ desc,
                                                                     const int64_t* __restrict__ jit, uint8_t* __restrict__ staging,
                                                                     int64_t* __restrict__ partials, int OH, int OW, int band,
                                                                     int rows_cap, int kh, int kv) {
  fr_body<FR_BICUBIC, 12, true>(src, desc, nullptr, nullptr, jit, staging, partials, 1, OH, OW, band, rows_cap, kh, kv);
}

__global__ __launch_bounds__(FR_THREADS) void frames_jitter_kernel(const uint8_t* __restrict__ staging,
                                                                    const int64_t* __restrict__ partials,
                                                                    const int64_t* __restrict__ jit, const float* __restrict__ lut,
                                                                    float* __restrict__ out, int OH, int OW, int bands) {
  __shared__ float s_lut[3 * 256];
  const int tid = threadIdx.x, n = blockIdx.y;
  for (int i = tid; i < 3 * 256; i += FR_THREADS) s_lut[i] = lut[i];
  __syncthreads();
  const FrJitter jt = fr_jitter_load(jit + (size_t)n * FR_JIT_COLS);
  const int at = fr_contrast_at(jt);
  const int64_t npix = (int64_t)OH * OW;
  int m = 0;
  if (at < jt.n) {               // uniform per workgroup: scalar loads
    int64_t S = 0;
    for (int i = 0; i < bands; ++i) S += partials[(size_t)n * bands + i];
    m = (int)((2 * S + npix) / (2 * npix));
  }
  const int64_t p = (int64_t)blockIdx.x * FR_THREADS + tid;
  if (p >= npix) return;
  const uint8_t* s = staging + ((size_t)n * npix + p) * 3;
  int r = s[0], g = s[1], b = s[2];
#pragma unroll
  for (int q = 0; q < 3; ++q)
    if (q >= at && q < jt.n) fr_enhance(jt.op[q], jt.f[q], m, r, g, b);
  float* o = out + (size_t)n * 3 * npix + p;
  o[0] = s_lut[r];
  o[npix] = s_lut[256 + g];
  o[2 * npix] = s_lut[512 + b];
}

// Host checks of one launch + the LDS plan.  Every descriptor is read from host memory: offset, H, W, crop top, crop left,
// crop h, crop w, flip (DW = 8) + full_h, full_w, win_top, win_left (DW = 12; with 8 columns full = out and the window is at 0).
static int fr_plan(const char* who, const int64_t* desc_host, int DW, int filter, int N, int B, int T, size_t frames_bytes, int OH,
                   int OW, FramePlan* plan) {
  MLA_REQUIRE(desc_host, "%s: null descriptor table", who);
  MLA_REQUIRE(filter == FR_BILINEAR || filter == FR_BICUBIC, "%s: unknown filter %d (0 = bilinear, 1 = bicubic)", who, filter);
  MLA_REQUIRE(B > 0 && T > 0 && N > 0, "%s: B=%d T=%d N=%d must be > 0", who, B, T, N);
  MLA_REQUIRE((long long)B * T == N, "%s: N=%d frames but B*T = %d*%d", who, N, B, T);
  MLA_REQUIRE(N < 65536, "%s: N=%d frames per launch (max 65535)", who, N);
  MLA_REQUIRE(OH > 0 && OW > 0 && OH <= 4096 && OW <= 4096, "%s: output size %dx%d out of range", who, OH, OW);
  int kh = 1, kv = 1;
  double sy_max = 0.0;
  for (int n = 0; n < N; ++n) {
    const int64_t* d = desc_host + (size_t)n * DW;
    const int64_t off = d[0], H = d[1], W = d[2], top = d[3], left = d[4], ch = d[5], cw = d[6], flip = d[7];
    const int64_t full_h = DW == 12 ? d[8] : OH, full_w = DW == 12 ? d[9] : OW, win_top = DW == 12 ? d[10] : 0,
                  win_left = DW == 12 ? d[11] : 0;
    MLA_REQUIRE(H > 0 && W > 0 && H <= FR_DIM_MAX && W <= FR_DIM_MAX, "%s: frame %d: size %lldx%lld out of range", who, n,
                (long long)H, (long long)W);
    MLA_REQUIRE(ch > 0 && cw > 0, "%s: frame %d: empty crop %lldx%lld", who, n, (long long)ch, (long long)cw);
    MLA_REQUIRE(top >= 0 && left >= 0 && top + ch <= H && left + cw <= W,
                "%s: frame %d: crop (top %lld, left %lld, h %lld, w %lld) leaves the %lldx%lld frame", who, n, (long long)top,
                (long long)left, (long long)ch, (long long)cw, (long long)H, (long long)W);
    MLA_REQUIRE(flip == 0 || flip == 1, "%s: frame %d: flip flag %lld", who, n, (long long)flip);
    MLA_REQUIRE(off >= 0 && (uint64_t)off + (uint64_t)(H * W * 3) <= (uint64_t)frames_bytes,
                "%s: frame %d: bytes [%lld, %lld) lie outside the %zu-byte buffer", who, n, (long long)off,
                (long long)(off + H * W * 3), frames_bytes);
    MLA_REQUIRE(full_h > 0 && full_w > 0 && full_h <= FR_DIM_MAX && full_w <= FR_DIM_MAX,
                "%s: frame %d: resized size %lldx%lld out of range", who, n, (long long)full_h, (long long)full_w);
    MLA_REQUIRE(win_top >= 0 && win_left >= 0 && win_top + OH <= full_h && win_left + OW <= full_w,
                "%s: frame %d: window (top %lld, left %lld, %dx%d) leaves the %lldx%lld resized image", who, n, (long long)win_top,
                (long long)win_left, OH, OW, (long long)full_h, (long long)full_w);
    kh = std::max(kh, fr_ksize(filter, (int)cw, (int)full_w));
    kv = std::max(kv, fr_ksize(filter, (int)ch, (int)full_h));
    sy_max = fmax(sy_max, (double)ch / full_h);
  }
  // exact number of source rows a band of `band` output rows reads, maximised over frames and bands
  for (int band = FR_BAND; band >= 1; band >>= 1) {
    int rows_cap = 1;
    for (int n = 0; n < N; ++n) {
      const int64_t* d = desc_host + (size_t)n * DW;
      const int ch = (int)d[5], full_h = DW == 12 ? (int)d[8] : OH, win_top = DW == 12 ? (int)d[10] : 0;
      for (int y0 = 0; y0 < OH; y0 += band) {
        const int y1 = std::min(y0 + band, OH) - 1;
        int a0, a1, b0, b1;
        fr_bounds(filter, ch, full_h, win_top + y0, &a0, &a1);
        fr_bounds(filter, ch, full_h, win_top + y1, &b0, &b1);
        rows_cap = std::max(rows_cap, b0 + b1 - a0);
      }
    }
    const size_t lds = fr_lds(OW, band, rows_cap, kh, kv);
    if (lds <= FR_LDS_MAX) {
      *plan = FramePlan{band, rows_cap, kh, kv, lds};
      return MLA_OK;
    }
  }
  MLA_REQUIRE(false, "%s: a %dx%d output of crops up to %.1fx its height needs more than %d bytes of LDS", who, OH, OW, sy_max,
              FR_LDS_MAX);
  return MLA_ERR_INVALID_ARG;
}

template <int FILTER, int DW>
static void fr_launch(const FramePlan& plan, const uint8_t* frames, const int64_t* desc, const float* lut, float* out, int N, int T,
                      int out_h, int out_w, void* stream) {
  dim3 grid((unsigned)cdiv(out_h, plan.band), (unsigned)N);
  hipLaunchKernelGGL((frames_resample_kernel<FILTER, DW>), grid, dim3(FR_THREADS), plan.lds, (hipStream_t)stream, frames, desc, lut,
                     out, T, out_h, out_w, plan.band, plan.rows_cap, plan.kh, plan.kv);
}

extern "C" int mla_frames_check(const int64_t* desc_host, int N, int B, int T, size_t frames_bytes, int out_h, int out_w) {
  FramePlan plan;
  return fr_plan("mla_frames", desc_host, 8, FR_BILINEAR, N, B, T, frames_bytes, out_h, out_w, &plan);
}

extern "C" int mla_frames_resample(const uint8_t* frames, size_t frames_bytes, const int64_t* desc, const int64_t* desc_host,
                                   const float* lut, float* out, int N, int B, int T, int out_h, int out_w, void* stream) {
  MLA_REQUIRE(frames && desc && lut && out, "mla_frames_resample: null pointer");
  FramePlan plan;
  const int rc = fr_plan("mla_frames", desc_host, 8, FR_BILINEAR, N, B, T, frames_bytes, out_h, out_w, &plan);
  if (rc != MLA_OK) return rc;
  fr_launch<FR_BILINEAR, 8>(plan, frames, desc, lut, out, N, T, out_h, out_w, stream);
  MLA_CHECK_LAUNCH("mla_frames_resample");
  return MLA_OK;
}

extern "C" int mla_image_check(const int64_t* desc_host, int N, int B, int T, size_t frames_bytes, int out_h, int out_w,
                               int filter) {
  FramePlan plan;
  return fr_plan("mla_image", desc_host, 12, filter, N, B, T, frames_bytes, out_h, out_w, &plan);
}

extern "C" int mla_image_resample(const uint8_t* frames, size_t frames_bytes, const int64_t* desc, const int64_t* desc_host,
                                  const float* lut, float* out, int N, int B, int T, int out_h, int out_w, int filter,
                                  void* stream) {
  MLA_REQUIRE(frames && desc && lut && out, "mla_image_resample: null pointer");
  FramePlan plan;
  const int rc = fr_plan("mla_image", desc_host, 12, filter, N, B, T, frames_bytes, out_h, out_w, &plan);
  if (rc != MLA_OK) return rc;
  if (filter == FR_BICUBIC) fr_launch<FR_BICUBIC, 12>(plan, frames, desc, lut, out, N, T, out_h, out_w, stream);
  else fr_launch<FR_BILINEAR, 12>(plan, frames, desc, lut, out, N, T, out_h, out_w, stream);
  MLA_CHECK_LAUNCH("mla_image_resample");
  return MLA_OK;
}

// Host checks of the jitter table: int64 (N, 7) rows (n_ops, op0, op1, op2, brightness bits, contrast bits, saturation bits)
static int fr_jitter_check(const int64_t* jit_host, int N) {
  MLA_REQUIRE(jit_host, "mla_image_augment: null jitter table");
  for (int n = 0; n < N; ++n) {
    const int64_t* j = jit_host + (size_t)n * FR_JIT_COLS;
    MLA_REQUIRE(j[0] >= 0 && j[0] <= 3, "mla_image_augment: image %d: %lld operations (0..3)", n, (long long)j[0]);
    unsigned seen = 0;
    for (int q = 0; q < (int)j[0]; ++q) {
      const int64_t op = j[1 + q];
      MLA_REQUIRE(op >= 0 && op <= 2, "mla_image_augment: image %d: unknown operation id %lld (0 = brightness, 1 = contrast, 2 = saturation)",
                  n, (long long)op);
      MLA_REQUIRE(!(seen & (1u << op)), "mla_image_augment: image %d: operation %lld is repeated", n, (long long)op);
      seen |= 1u << op;
    }
    for (int q = 0; q < 3; ++q) {
      const int64_t bits = j[4 + q];
      MLA_REQUIRE(bits >= 0 && bits <= 0xFFFFFFFFll, "mla_image_augment: image %d: factor %d is not an fp32 bit pattern", n, q);
      const uint32_t u = (uint32_t)bits;
      float a;
      memcpy(&a, &u, sizeof a);
      MLA_REQUIRE(std::isfinite(a) && a >= 0.f, "mla_image_augment: image %d: factor %d is %g (must be finite and >= 0)", n, q, (double)a);
    }
  }
  return MLA_OK;
}

static int fr_augment_plan(const int64_t* desc_host, const int64_t* jit_host, int N, size_t frames_bytes, int OH, int OW,
                           size_t staging_bytes, size_t partials_count, FramePlan* plan) {
  int rc = fr_plan("mla_image_augment", desc_host, 12, FR_BICUBIC, N, N, 1, frames_bytes, OH, OW, plan);
  if (rc != MLA_OK) return rc;
  rc = fr_jitter_check(jit_host, N);
  if (rc != MLA_OK) return rc;
  const size_t need_s = (size_t)N * OH * OW * 3, need_p = (size_t)N * cdiv(OH, plan->band);
  MLA_REQUIRE(staging_bytes >= need_s, "mla_image_augment: staging buffer of %zu bytes, %zu needed (N * out_h * out_w * 3)", staging_bytes,
              need_s);
  MLA_REQUIRE(partials_count >= need_p, "mla_image_augment: partials buffer of %zu int64 slots, %zu needed (N * bands of %d rows)",
              partials_count, need_p, plan->band);
  return MLA_OK;
}

extern "C" int mla_image_augment_check(const int64_t* desc_host, const int64_t* jit_host, int N, size_t frames_bytes, int out_h,
                                       int out_w, size_t staging_bytes, size_t partials_count) {
  FramePlan plan;
  return fr_augment_plan(desc_host, jit_host, N, frames_bytes, out_h, out_w, staging_bytes, partials_count, &plan);
}

static inline bool fr_disjoint(const void* a, size_t an, const void* b, size_t bn) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x + an <= y || y + bn <= x;
}

extern "C" int mla_image_augment(const uint8_t* frames, size_t frames_bytes, const int64_t* desc, const int64_t* desc_host,
                                 const int64_t* jit, const int64_t* jit_host, const float* lut, float* out, uint8_t* staging,
                                 size_t staging_bytes, int64_t* partials, size_t partials_count, int N, int out_h, int out_w,
                                 void* stream) {
  MLA_REQUIRE(frames && desc && jit && lut && out && staging && partials, "mla_image_augment: null pointer");
  FramePlan plan;
  const int rc = fr_augment_plan(desc_host, jit_host, N, frames_bytes, out_h, out_w, staging_bytes, partials_count, &plan);
  if (rc != MLA_OK) return rc;
  const size_t out_bytes = (size_t)N * 3 * out_h * out_w * sizeof(float), part_bytes = partials_count * sizeof(int64_t);
  MLA_REQUIRE(fr_disjoint(out, out_bytes, staging, staging_bytes) && fr_disjoint(out, out_bytes, partials, part_bytes) &&
                  fr_disjoint(staging, staging_bytes, partials, part_bytes),
              "mla_image_augment: out, staging and partials overlap");
  MLA_REQUIRE((uintptr_t)partials % 8 == 0, "mla_image_augment: partials must be 8-byte aligned");
  const int bands = cdiv(out_h, plan.band);
  hipLaunchKernelGGL(frames_augment_kernel, dim3((unsigned)bands, (unsigned)N), dim3(FR_THREADS), plan.lds, (hipStream_t)stream, frames,
                     desc, jit, staging, partials, out_h, out_w, plan.band, plan.rows_cap, plan.kh, plan.kv);
  MLA_CHECK_LAUNCH("mla_image_augment (resample)");
  hipLaunchKernelGGL(frames_jitter_kernel, dim3((unsigned)cdiv((long)out_h * out_w, FR_THREADS), (unsigned)N), dim3(FR_THREADS), 0,
                     (hipStream_t)stream, staging, partials, jit, lut, out, out_h, out_w, bands);
  MLA_CHECK_LAUNCH("mla_image_augment (jitter)");
  return MLA_OK;
}
