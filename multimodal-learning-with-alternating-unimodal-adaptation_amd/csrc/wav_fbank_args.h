// Host half of mla_wav_fbank (wav_fbank.hip): the checks of the clip table, which the batcher builds on the host, of the sparse mel
// matrix and of the buffers, and the launch plan.  Plain C++ with no HIP in it, so wav_fbank_host_check.cpp builds it with the host
// sanitizers.
#pragma once
#include <limits.h>
#include "args_common.h"

#define WAVFB_DESC 4            // offset_samples, n_samples, sample_sum, reserved (0)
#define WAVFB_WINDOW 400        // 25 ms at 16 kHz
#define WAVFB_SHIFT 160         // 10 ms
#define WAVFB_PADDED 512        // round_to_power_of_two
#define WAVFB_BINS 256          // FFT bins 0..255 carry mel weight; the Nyquist bin has weight 0
#define WAVFB_MEL 128
#define WAVFB_THREADS 256
#define WAVFB_FRAMES 4          // frames per workgroup: one wave each

struct WavFbankPlan {
  int blocks_x;                 // grid = (blocks_x, B): blocks_x * WAVFB_FRAMES >= target_length
};

// frames of an n-sample clip with snip_edges=True
static inline int64_t wavfb_frames(int64_t n) { return n < WAVFB_WINDOW ? 0 : 1 + (n - WAVFB_WINDOW) / WAVFB_SHIFT; }

// desc_host int64 (B, 4): every clip inside the buffer, n_samples 0 (an absent clip) or >= 400, a sum that n int16 samples can have
static inline int wavfb_table_check(const int64_t* desc_host, int B, size_t wav_samples) {
  MLA_REQUIRE(desc_host, "mla_wav_fbank: null clip table");
  MLA_REQUIRE(B > 0 && B < 65536, "mla_wav_fbank: need 0 < B < 65536 (got B=%d)", B);
  // 32768 * n below stays inside int64
  MLA_REQUIRE(wav_samples <= (size_t)INT64_MAX / 32768, "mla_wav_fbank: a buffer of %zu samples is too large", wav_samples);
  const int64_t total = (int64_t)wav_samples;
  for (int b = 0; b < B; ++b) {
    const int64_t* d = desc_host + (size_t)b * WAVFB_DESC;
    const int64_t off = d[0], n = d[1], sum = d[2];
    MLA_REQUIRE(n == 0 || n >= WAVFB_WINDOW, "mla_wav_fbank: clip %d: n_samples %lld is neither 0 nor >= %d (one 25 ms frame)", b,
                (long long)n, WAVFB_WINDOW);
    MLA_REQUIRE(off >= 0 && off <= total && n <= total - off, "mla_wav_fbank: clip %d: samples [%lld, %lld + %lld) leave the buffer of %lld",
                b, (long long)off, (long long)off, (long long)n, (long long)total);
    MLA_REQUIRE(sum <= 32767 * n && sum >= -32768 * n, "mla_wav_fbank: clip %d: sample_sum %lld is not a sum of %lld int16 samples", b,
                (long long)sum, (long long)n);
    MLA_REQUIRE(d[3] == 0, "mla_wav_fbank: clip %d: the reserved column is %lld, not 0", b, (long long)d[3]);
  }
  return MLA_OK;
}

// the sparse mel matrix: bank i weighs the FFT bins [start[i], start[i] + len[i]) with the next len[i] entries of mel_weight
static inline int wavfb_mel_check(const int32_t* mel_start_host, const int32_t* mel_len_host, size_t mel_weights) {
  MLA_REQUIRE(mel_start_host && mel_len_host, "mla_wav_fbank: null mel table");
  size_t total = 0;
  for (int i = 0; i < WAVFB_MEL; ++i) {
    const int32_t s = mel_start_host[i], l = mel_len_host[i];
    MLA_REQUIRE(s >= 0 && l >= 0 && s <= WAVFB_BINS && l <= WAVFB_BINS - s,
                "mla_wav_fbank: mel bank %d: bins [%d, %d + %d) are outside [0, %d)", i, s, s, l, WAVFB_BINS);
    total += (size_t)l;
  }
  MLA_REQUIRE(total == mel_weights, "mla_wav_fbank: the mel runs hold %zu weights but mel_weight has %zu", total, mel_weights);
  return MLA_OK;
}

static inline int wavfb_shape_plan(int B, int target_length, WavFbankPlan* out) {
  MLA_REQUIRE(B > 0 && B < 65536 && target_length > 0, "mla_wav_fbank: need 0 < B < 65536 and target_length > 0 (got B=%d, target_length=%d)",
              B, target_length);
  MLA_REQUIRE((long long)target_length * WAVFB_MEL <= INT_MAX && (long long)B * target_length <= INT_MAX,
              "mla_wav_fbank: target_length * %d and B * target_length must fit an int (got B=%d, target_length=%d)", WAVFB_MEL, B,
              target_length);
  out->blocks_x = (target_length + WAVFB_FRAMES - 1) / WAVFB_FRAMES;
  return MLA_OK;
}

static inline int wavfb_check(const int64_t* desc_host, int B, size_t wav_samples, int target_length, const int32_t* mel_start_host,
                              const int32_t* mel_len_host, size_t mel_weights, WavFbankPlan* out) {
  MLA_TRY(wavfb_shape_plan(B, target_length, out));
  MLA_TRY(wavfb_table_check(desc_host, B, wav_samples));
  return wavfb_mel_check(mel_start_host, mel_len_host, mel_weights);
}

static inline int wavfb_plan(const void* wav, size_t wav_samples, const void* desc, const int64_t* desc_host, const void* window,
                             const void* twiddle, const void* mel_start, const void* mel_len, const int32_t* mel_start_host,
                             const int32_t* mel_len_host, const void* mel_weight, size_t mel_weights, const void* out, int B,
                             int target_length, WavFbankPlan* plan) {
  // an empty buffer (every clip absent) may come as a null pointer
  MLA_REQUIRE((wav_samples == 0 || wav) && desc && desc_host && window && twiddle && mel_start && mel_len && mel_start_host &&
                  mel_len_host && mel_weight && out,
              "mla_wav_fbank: null pointer");
  MLA_TRY(wavfb_check(desc_host, B, wav_samples, target_length, mel_start_host, mel_len_host, mel_weights, plan));
  MLA_REQUIRE(!((uintptr_t)out & 15), "mla_wav_fbank: out must be 16-byte aligned (rows are written as 16-byte units)");
  MLA_REQUIRE(!((uintptr_t)wav & 1) && !((uintptr_t)desc & 7) &&
                  !(((uintptr_t)window | (uintptr_t)twiddle | (uintptr_t)mel_start | (uintptr_t)mel_len | (uintptr_t)mel_weight) & 3),
              "mla_wav_fbank: wav must be 2-byte, the clip table 8-byte and the constant tables 4-byte aligned");
  return MLA_OK;
}
