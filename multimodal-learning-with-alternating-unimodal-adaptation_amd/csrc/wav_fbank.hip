// Kaldi log-mel filterbank from packed PCM16 clips (data/extract_fbank.py:8-54), gfx950.  Per clip the reference runs
//
//   waveform = waveform - waveform.mean()
//   fbank = torchaudio.compliance.kaldi.fbank(waveform, htk_compat=True, sample_frequency=16000, use_energy=False,
//                                             window_type='hanning', num_mel_bins=128, dither=0.0, frame_shift=10)
//
// and pads with zeros or cuts to target_length rows.  With torchaudio 0.8.1's other defaults a frame is 400 samples every 160
// (snip_edges), minus its own mean, pre-emphasised (0.97, sample 0 against itself), times a symmetric Hann window, zero-padded to
// 512; the power spectrum of its real FFT goes through 128 triangular mel banks over the bins 0..255 and log(max(E, 2^-23)).
//
// One wave per frame, WAVFB_FRAMES frames per workgroup, grid (frame block, clip).  The 512-point real FFT is a 256-point complex
// radix-4 decimation-in-frequency FFT of z[n] = x[2n] + i x[2n+1] in LDS (four stages, one butterfly per lane and stage, output
// in base-4 digit-reversed order) and the split post-pass.  Twiddles come from a table the host computed in fp64; no sincos here.
// Real and imaginary parts live in separate fp32 arrays, four words of padding after every 16 (PADI): unpadded, the stride-16 and
// stride-4 stages put a half-wave's ds_read_b32 / ds_write_b32 on 16 and on 8 of the 32 banks; padded, both are conflict-free,
// the stride-64 stage is 2-way for 4 lanes of 32, and the last stage moves a lane's four consecutive words (16-byte aligned under
// this padding) as one ds_read_b128 / ds_write_b128.
// Every reduction has a fixed order (per-lane ascending, then the xor butterfly; a bank's bins ascending) and there are no
// atomics: a clip's rows depend on that clip's samples and descriptor row alone.
#include "common.h"
#include "wav_fbank_args.h"

#define PADI(i) ((i) + (((i) >> 4) << 2))
#define WAVFB_LDS 320                             // PADI(255) + 1 = 316, rounded up

// position of Z[k] after the four in-place radix-4 DIF stages: k's base-4 digits reversed
__device__ __forceinline__ int digit_reverse4(int k) { return ((k & 3) << 6) | ((k & 12) << 2) | ((k >> 2) & 12) | (k >> 6); }

struct cplx {
  float re, im;
};
__device__ __forceinline__ cplx cadd(cplx a, cplx b) { return {a.re + b.re, a.im + b.im}; }
__device__ __forceinline__ cplx csub(cplx a, cplx b) { return {a.re - b.re, a.im - b.im}; }
__device__ __forceinline__ cplx cmul(cplx a, cplx b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__device__ __forceinline__ cplx mul_neg_i(cplx a) { return {a.im, -a.re}; }
// exp(-2 pi i j / 512), j in [0, 512)
__device__ __forceinline__ cplx twiddle512(const float* __restrict__ tw, int j) { return {tw[2 * j], tw[2 * j + 1]}; }

// one radix-4 DIF stage over 256 points in LDS: Q = quarter length (64, 16, 4, 1), one butterfly per lane
template <int Q>
__device__ __forceinline__ void radix4_stage(float* re, float* im, const float* __restrict__ tw, int lane) {
  const int k = lane & (Q - 1), base = ((lane - k) << 2) + k;
  cplx x[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) x[m] = {re[PADI(base + m * Q)], im[PADI(base + m * Q)]};
  const cplx a0 = cadd(x[0], x[2]), a1 = csub(x[0], x[2]), a2 = cadd(x[1], x[3]), a3 = mul_neg_i(csub(x[1], x[3]));
  cplx y[4] = {cadd(a0, a2), cadd(a1, a3), csub(a0, a2), csub(a1, a3)};
  if (Q > 1) {
#pragma unroll
    for (int m = 1; m < 4; ++m) y[m] = cmul(y[m], twiddle512(tw, m * k * (128 / Q)));       // W_{4Q}^{mk}
  }
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    re[PADI(base + m * Q)] = y[m].re;
    im[PADI(base + m * Q)] = y[m].im;
  }
}

// sample j of the frame lives at z[j / 2]: even samples in re, odd ones in im
__device__ __forceinline__ float& frame_at(float* re, float* im, int j) { return ((j & 1) ? im : re)[PADI(j >> 1)]; }

// host (wavfb_plan): clips inside the buffer, mel runs inside [0, 256) and as long as mel_weight, out 16-byte aligned.  The kernel
// repeats the range tests on what it reads from the device tables, so that a device table that differs from the host's cannot
// make it read outside wav, the power spectrum or mel_weight.
__global__ __launch_bounds__(WAVFB_THREADS) void wav_fbank_kernel(const int16_t* __restrict__ wav, long long wav_samples,
                                                                   const int64_t* __restrict__ desc, const float* __restrict__ window,
                                                                   const float* __restrict__ tw, const int* __restrict__ mel_start,
                                                                   const int* __restrict__ mel_len, const float* __restrict__ mel_weight,
                                                                   int mel_weights, f32x4* __restrict__ out, int T) {
  __shared__ float s_re[WAVFB_FRAMES][WAVFB_LDS], s_im[WAVFB_FRAMES][WAVFB_LDS], s_pw[WAVFB_FRAMES][WAVFB_BINS];
  const int b = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * WAVFB_FRAMES + wave;
  const int64_t* d = desc + (size_t)b * WAVFB_DESC;
  const long long off = d[0], sum = d[2];
  long long n = d[1];
  if (off < 0 || off > wav_samples || n > wav_samples - off) n = 0;
  const long long frames = n < WAVFB_WINDOW ? 0 : 1 + (n - WAVFB_WINDOW) / WAVFB_SHIFT;
  const int valid = (int)(frames < T ? frames : T);
  f32x4* orow = out + ((size_t)b * T + row) * (WAVFB_MEL / 4);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  if ((int)blockIdx.x * WAVFB_FRAMES >= valid) {             // uniform over the workgroup: rows beyond the clip are +0.0
    if (row < T && lane < WAVFB_MEL / 4) orow[lane] = zero;
    return;
  }
  // a workgroup that straddles the clip's end: the waves beyond it run the last frame again (every wave meets every barrier, no
  // read leaves the clip) and write zeros
  const bool live = row < valid;
  const int frame = live ? row : valid - 1;
  float* re = s_re[wave];
  float* im = s_im[wave];
  float* pw = s_pw[wave];

  // samples as torchaudio.load gives them (s / 32768, exact) minus the clip mean, which is exact up to its one rounding
  const float mean = (float)((double)sum / (32768.0 * (double)n));
  const int16_t* src = wav + off + (long long)frame * WAVFB_SHIFT;
  float x[7];
  float acc = 0.f;
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    const int j = lane + 64 * i;
    x[i] = j < WAVFB_WINDOW ? __fsub_rn((float)src[j] * (1.0f / 32768.0f), mean) : 0.f;
    acc += x[i];
  }
  const float frame_mean = wave_sum(acc) / (float)WAVFB_WINDOW;          // remove_dc_offset
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    const int j = lane + 64 * i;
    x[i] = __fsub_rn(x[i], frame_mean);
    if (j < WAVFB_WINDOW) frame_at(re, im, j) = x[i];
  }
  __syncthreads();
  // x[j] - 0.97 x[max(j - 1, 0)], then the window: the reference's three roundings, not contracted
  float y[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    const int j = lane + 64 * i;
    y[i] = 0.f;
    if (j < WAVFB_WINDOW) {
      const float prev = frame_at(re, im, j > 0 ? j - 1 : 0);
      y[i] = __fmul_rn(__fsub_rn(x[i], __fmul_rn(0.97f, prev)), window[j]);
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 7; ++i) frame_at(re, im, lane + 64 * i) = y[i];
  frame_at(re, im, lane + 448) = 0.f;
  __syncthreads();

  radix4_stage<64>(re, im, tw, lane);
  __syncthreads();
  radix4_stage<16>(re, im, tw, lane);
  __syncthreads();
  radix4_stage<4>(re, im, tw, lane);
  __syncthreads();
  radix4_stage<1>(re, im, tw, lane);
  __syncthreads();

  // split post-pass: X[k] = (Z[k] + conj Z[256 - k]) / 2 + W_512^k (Z[k] - conj Z[256 - k]) / (2i), k = 0..255; |X[k]|^2
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int k = lane + 64 * i, pa = PADI(digit_reverse4(k)), pb = PADI(digit_reverse4((256 - k) & 255));
    const cplx A = {re[pa], im[pa]}, Bc = {re[pb], -im[pb]};
    const cplx E = cadd(A, Bc), D = csub(A, Bc);
    const cplx O = cmul(twiddle512(tw, k), mul_neg_i(D));
    const cplx X = {0.5f * (E.re + O.re), 0.5f * (E.im + O.im)};
    pw[k] = X.re * X.re + X.im * X.im;
  }
  __syncthreads();

  // mel banks 2 * lane and 2 * lane + 1: their weights start at the sum of the run lengths before them
  int s0 = mel_start[2 * lane], l0 = mel_len[2 * lane], s1 = mel_start[2 * lane + 1], l1 = mel_len[2 * lane + 1];
  if (s0 < 0 || s0 > WAVFB_BINS || l0 < 0 || l0 > WAVFB_BINS - s0) l0 = 0;
  if (s1 < 0 || s1 > WAVFB_BINS || l1 < 0 || l1 > WAVFB_BINS - s1) l1 = 0;
  int incl = l0 + l1;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(incl, o, 64);
    if (lane >= o) incl += t;
  }
  const int o0 = incl - l0 - l1, o1 = o0 + l0;
  if (incl > mel_weights) l0 = l1 = 0;
  float e0 = 0.f, e1 = 0.f;
  for (int i = 0; i < l0; ++i) e0 = fmaf(mel_weight[o0 + i], pw[s0 + i], e0);
  for (int i = 0; i < l1; ++i) e1 = fmaf(mel_weight[o1 + i], pw[s1 + i], e1);
  const float eps = 0x1p-23f;                                 // torch.finfo(torch.float).eps
  // log in fp64, rounded once: the device logf is within 1 ulp, and at eps itself (every silent element) it returns the neighbour
  // of the correctly rounded -15.942385 that torch's CPU log gives.  Two fp64 logs per lane and frame are nothing here.
  const float v0 = (float)log((double)fmaxf(e0, eps)), v1 = (float)log((double)fmaxf(e1, eps));
  const float v2 = __shfl_down(v0, 1, 64), v3 = __shfl_down(v1, 1, 64);
  if (row < T && !(lane & 1)) {
    const f32x4 v = {v0, v1, v2, v3};
    orow[lane >> 1] = live ? v : zero;
  }
}

extern "C" int mla_wav_fbank_check(const int64_t* desc_host, int B, size_t wav_samples, int target_length, const int32_t* mel_start_host,
                                   const int32_t* mel_len_host, size_t mel_weights) {
  WavFbankPlan p;
  return wavfb_check(desc_host, B, wav_samples, target_length, mel_start_host, mel_len_host, mel_weights, &p);
}

extern "C" int mla_wav_fbank(const int16_t* wav, size_t wav_samples, const int64_t* desc, const int64_t* desc_host, const float* window,
                             const float* twiddle, const int32_t* mel_start, const int32_t* mel_len, const int32_t* mel_start_host,
                             const int32_t* mel_len_host, const float* mel_weight, size_t mel_weights, float* out, int B, int target_length,
                             void* stream) {
  WavFbankPlan p;
  const int rc = wavfb_plan(wav, wav_samples, desc, desc_host, window, twiddle, mel_start, mel_len, mel_start_host, mel_len_host, mel_weight,
                            mel_weights, out, B, target_length, &p);
  if (rc != MLA_OK) return rc;
  hipLaunchKernelGGL(wav_fbank_kernel, dim3((unsigned)p.blocks_x, (unsigned)B), dim3(WAVFB_THREADS), 0, (hipStream_t)stream, wav,
                     (long long)wav_samples, desc, window, twiddle, mel_start, mel_len, mel_weight, (int)mel_weights,
                     reinterpret_cast<f32x4*>(out), target_length);
  MLA_CHECK_LAUNCH("mla_wav_fbank");
  return MLA_OK;
}
