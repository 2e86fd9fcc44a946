// CAVDataset's spectrogram path (dataset/dataset.py:281-294, 303-321; --cav_augnois), gfx950: SpecAug frequency / time mask ->
// normalise -> scaled uniform noise -> roll along time of a batch of (T, F) fbanks, bit-identical to the reference's torch CPU
// expressions
//
//   fbank[:, f0:f0+fw] = 0; fbank[t0:t0+tw, :] = 0           torchaudio FrequencyMasking(48) / TimeMasking(192), mask value 0.0
//   fbank = (fbank - norm_mean) / norm_std                    always (skip_norm = False), so a masked cell is (0 - mean) / std
//   fbank = fbank + torch.rand(T, F) * s / 10                 s = np.random.rand(), cast to fp32 by the tensor-scalar product
//   fbank = torch.roll(fbank, r, 0)                           out[(t + r) mod T] = fbank[t]
//
// in fp32 with a true IEEE division and no contraction (multiplying by 1 / std instead changes 4 % of the elements).  The masks,
// s and r are drawn on the host (cav_feed.sample_fbank_aug) and arrive in one descriptor row per sample; the T * F uniforms are
// drawn here, counter-based: element i = t * F + f of sample b is word i % 4 of philox4x32(i / 4, stream_id[b], seed), mapped
// to [0, 1) as torch.rand maps its 24 random bits.  A sample with flags = 0 is only normalised, so augmented and plain samples
// share a launch.  One thread per 4 consecutive bins (one Philox block, one 16-byte load and store); x and out are distinct
// buffers (the roll makes in-place unsafe).  No atomics.
#include <math.h>
#include "common.h"
#include "philox.h"

#define FB_THREADS 256
#define FB_DESC 8            // flags, f0, fw, t0, tw, roll, scale_bits, stream_id

__device__ __forceinline__ float fb_u01(uint32_t x) { return (float)(x >> 8) * (1.0f / 16777216.0f); }   // [0, 1): torch.rand

// host: F % 4 == 0 and 16-byte aligned buffers, so a thread's 4 elements lie in one row and are one Philox block
__global__ __launch_bounds__(FB_THREADS) void fbank_augment_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                                    const int64_t* __restrict__ desc, int T, int F, float mean,
                                                                    float std, uint64_t seed) {
#pragma clang fp contract(off)
  const int b = blockIdx.y;
  const int64_t* d = desc + (size_t)b * FB_DESC;
  const bool aug = (d[0] & 1) != 0;
  const int f0 = (int)d[1], f1 = f0 + (int)d[2], t0 = (int)d[3], t1 = t0 + (int)d[4], roll = (int)d[5];
  const float s = __uint_as_float((uint32_t)d[6]);
  const uint64_t stream_id = (uint64_t)d[7];
  const int per = T * F / 4;                                     // host: T * F < 2^31
  const int i = blockIdx.x * FB_THREADS + threadIdx.x;           // group of 4 consecutive elements of sample b
  if (i >= per) return;
  const int e = i * 4, t = e / F, f = e - t * F;
  int tt = aug ? t + roll : t;                                   // host: |roll| <= T
  if (tt < 0) tt += T;
  if (tt >= T) tt -= T;
  const size_t base = (size_t)b * T * F;
  f32x4 v = *reinterpret_cast<const f32x4*>(x + base + e);
  uint32_t r[4] = {0u, 0u, 0u, 0u};
  if (aug) philox4x32((uint64_t)i, stream_id, seed, r);
  const bool trow = aug && t >= t0 && t < t1;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float w = (trow || (aug && f + j >= f0 && f + j < f1)) ? 0.0f : v[j];
    w = (w - mean) / std;
    if (aug) w = w + (fb_u01(r[j]) * s) / 10.0f;
    v[j] = w;
  }
  *reinterpret_cast<f32x4*>(out + base + (size_t)tt * F + f) = v;
}

// Host checks of one launch: the descriptor rows are read from host memory.
static int fb_check(const int64_t* desc_host, int B, int T, int F) {
  MLA_REQUIRE(desc_host, "mla_fbank: null descriptor table");
  MLA_REQUIRE(B > 0 && T > 0 && F > 0, "mla_fbank: B=%d T=%d F=%d must be > 0", B, T, F);
  MLA_REQUIRE(F % 4 == 0, "mla_fbank: F=%d is no multiple of 4 (the kernel moves 4 bins per thread)", F);
  MLA_REQUIRE(B < 65536 && (long long)T * F < (1ll << 31), "mla_fbank: B=%d or T*F=%lld too large (max 65535, 2^31 - 1)", B,
              (long long)T * F);
  for (int b = 0; b < B; ++b) {
    const int64_t* d = desc_host + (size_t)b * FB_DESC;
    const int64_t flags = d[0], f0 = d[1], fw = d[2], t0 = d[3], tw = d[4], roll = d[5], bits = d[6];
    MLA_REQUIRE(flags == 0 || flags == 1, "mla_fbank: sample %d: flags %lld", b, (long long)flags);
    MLA_REQUIRE(fw >= 0 && tw >= 0, "mla_fbank: sample %d: negative mask width (freq %lld, time %lld)", b, (long long)fw,
                (long long)tw);
    MLA_REQUIRE(f0 >= 0 && f0 + fw <= F, "mla_fbank: sample %d: frequency mask [%lld, %lld) leaves the %d bins", b, (long long)f0,
                (long long)(f0 + fw), F);
    MLA_REQUIRE(t0 >= 0 && t0 + tw <= T, "mla_fbank: sample %d: time mask [%lld, %lld) leaves the %d frames", b, (long long)t0,
                (long long)(t0 + tw), T);
    MLA_REQUIRE(roll >= -(int64_t)T && roll <= (int64_t)T, "mla_fbank: sample %d: roll %lld beyond +-%d", b, (long long)roll, T);
    MLA_REQUIRE(bits >= 0 && bits <= 0xFFFFFFFFll, "mla_fbank: sample %d: noise scale is not an fp32 bit pattern", b);
  }
  return MLA_OK;
}

extern "C" int mla_fbank_check(const int64_t* desc_host, int B, int T, int F) { return fb_check(desc_host, B, T, F); }

extern "C" int mla_fbank_augment(const float* x, float* out, const int64_t* desc, const int64_t* desc_host, int B, int T, int F,
                                 float mean, float std, uint64_t seed, void* stream) {
  MLA_REQUIRE(x && out && desc, "mla_fbank_augment: null pointer");
  MLA_REQUIRE(std != 0.0f && std == std && mean == mean, "mla_fbank_augment: std %g / mean %g (std == 0 or NaN)", (double)std,
              (double)mean);
  const int rc = fb_check(desc_host, B, T, F);
  if (rc != MLA_OK) return rc;
  const size_t bytes = (size_t)B * T * F * sizeof(float);
  const uintptr_t xa = (uintptr_t)x, oa = (uintptr_t)out;
  MLA_REQUIRE(xa + bytes <= oa || oa + bytes <= xa, "mla_fbank_augment: x and out overlap (the roll cannot run in place)");
  MLA_REQUIRE(xa % 16 == 0 && oa % 16 == 0, "mla_fbank_augment: x and out must be 16-byte aligned");
  dim3 grid((unsigned)cdiv((long)T * F / 4, FB_THREADS), (unsigned)B);
  hipLaunchKernelGGL(fbank_augment_kernel, grid, dim3(FB_THREADS), 0, (hipStream_t)stream, x, out, desc, T, F, mean, std, seed);
  MLA_CHECK_LAUNCH("mla_fbank_augment");
  return MLA_OK;
}
