// Stand-alone host check of mla_wav_fbank's argument validation and launch plan (wav_fbank_args.h) with util.cpp's error
// reporting.  No GPU, no HIP: `make host-check` builds it with -fsanitize=address,undefined and runs it.
#include "wav_fbank_args.h"
#include "host_check.h"

int main() {
  // three clips in a buffer of 2000 samples: 400 at 0, an absent one, 1599 at the odd offset 401 (to the buffer's last sample)
  enum { B = 3, N = 2000, T = 8, NW = 2 * WAVFB_MEL };
  alignas(16) static int16_t wav[N];
  alignas(16) static float out[B * T * WAVFB_MEL + 4], window[WAVFB_WINDOW], tw[2 * WAVFB_PADDED], weight[NW];
  alignas(16) static int64_t dev[B * WAVFB_DESC];
  alignas(16) static int32_t start[WAVFB_MEL], len[WAVFB_MEL];
  const int64_t ok[B * WAVFB_DESC] = {0, 400, -1234, 0, 400, 0, 0, 0, 401, 1599, 32767ll * 1599, 0};
  for (int i = 0; i < WAVFB_MEL; ++i) { start[i] = 2 * i; len[i] = 2; }          // the last run ends at bin 256
  int64_t t[B * WAVFB_DESC];
  int32_t ms[WAVFB_MEL], ml[WAVFB_MEL];
  WavFbankPlan p;
  auto plan = [&](const void* w, size_t n, const void* d, const int64_t* dh, const void* o, int b, int tl) {
    return wavfb_plan(w, n, d, dh, window, tw, start, len, start, len, weight, NW, o, b, tl, &p);
  };
  EXPECT(plan(wav, N, dev, ok, out, B, T) == MLA_OK);
  EXPECT(p.blocks_x == 2);
  EXPECT(plan(wav, N, dev, ok, out, B, 1024) == MLA_OK && p.blocks_x == 256);
  EXPECT(plan(wav, N, dev, ok, out, B, 5) == MLA_OK && p.blocks_x == 2);
  EXPECT(wavfb_frames(399) == 0 && wavfb_frames(400) == 1 && wavfb_frames(559) == 1 && wavfb_frames(560) == 2 &&
         wavfb_frames(400 + 160 * 7) == 8 && wavfb_frames(16000) == 98);

  // null pointers; the sample buffer may be null only when it is empty
  REFUSED(plan(nullptr, N, dev, ok, out, B, T), "null pointer");
  REFUSED(plan(wav, N, nullptr, ok, out, B, T), "null pointer");
  REFUSED(plan(wav, N, dev, nullptr, out, B, T), "null pointer");
  REFUSED(plan(wav, N, dev, ok, nullptr, B, T), "null pointer");
  REFUSED(wavfb_plan(wav, N, dev, ok, nullptr, tw, start, len, start, len, weight, NW, out, B, T, &p), "null pointer");
  REFUSED(wavfb_plan(wav, N, dev, ok, window, nullptr, start, len, start, len, weight, NW, out, B, T, &p), "null pointer");
  REFUSED(wavfb_plan(wav, N, dev, ok, window, tw, nullptr, len, start, len, weight, NW, out, B, T, &p), "null pointer");
  REFUSED(wavfb_plan(wav, N, dev, ok, window, tw, start, len, start, nullptr, weight, NW, out, B, T, &p), "null pointer");
  REFUSED(wavfb_plan(wav, N, dev, ok, window, tw, start, len, start, len, nullptr, NW, out, B, T, &p), "null pointer");
  REFUSED(wavfb_table_check(nullptr, B, N), "null clip table");
  REFUSED(wavfb_mel_check(nullptr, len, NW), "null mel table");
  memset(t, 0, sizeof(t));
  EXPECT(plan(nullptr, 0, dev, t, out, B, T) == MLA_OK);                          // every clip absent

  // sizes: B, target_length and the int ranges of target_length * 128 and B * target_length
  REFUSED(plan(wav, N, dev, ok, out, 0, T), "0 < B < 65536");
  REFUSED(plan(wav, N, dev, ok, out, 65536, T), "0 < B < 65536");
  REFUSED(plan(wav, N, dev, ok, out, B, 0), "target_length > 0");
  REFUSED(plan(wav, N, dev, ok, out, B, -8), "target_length > 0");
  REFUSED(wavfb_shape_plan(1, (1 << 24), &p), "fit an int");                      // 2^24 * 128 = 2^31
  EXPECT(wavfb_shape_plan(1, (1 << 24) - 1, &p) == MLA_OK);
  REFUSED(wavfb_shape_plan(65535, 32769, &p), "fit an int");                      // 65535 * 32769 = 2^31 + 32767
  EXPECT(wavfb_shape_plan(65535, 32768, &p) == MLA_OK);                           // 2^31 - 32768

  // alignment
  REFUSED(plan(wav, N, dev, ok, out + 1, B, T), "16-byte aligned");
  REFUSED(plan(wav, N, dev, ok, out + 2, B, T), "16-byte aligned");
  EXPECT(plan(wav, N, dev, ok, out + 4, B, T) == MLA_OK);
  REFUSED(plan((const char*)wav + 1, N, dev, ok, out, B, T), "2-byte");
  EXPECT(plan(wav + 1, N, dev, ok, out, B, T) == MLA_OK);                         // never dereferenced here: any 2-byte boundary
  REFUSED(plan(wav, N, (const char*)dev + 4, ok, out, B, T), "8-byte");
  REFUSED(wavfb_plan(wav, N, dev, ok, (const char*)window + 2, tw, start, len, start, len, weight, NW, out, B, T, &p), "4-byte");

  // the clip table
  auto table = [&](int row, int col, int64_t v, size_t n) {
    memcpy(t, ok, sizeof(t));
    if (row >= 0) t[WAVFB_DESC * row + col] = v;
    return wavfb_table_check(t, B, n);
  };
  EXPECT(table(-1, 0, 0, N) == MLA_OK);
  REFUSED(table(-1, 0, 0, N - 1), "leave the buffer");                            // the last clip ends one sample past it
  REFUSED(table(0, 0, -1, N), "leave the buffer");
  REFUSED(table(0, 0, N + 1, N), "leave the buffer");                             // an offset past the buffer
  REFUSED(table(0, 0, N - 399, N), "leave the buffer");
  EXPECT(table(0, 0, N - 400, N) == MLA_OK);
  REFUSED(table(0, 0, INT64_MAX, N), "leave the buffer");                         // offset + n would overflow
  REFUSED(table(2, 1, INT64_MAX, N), "leave the buffer");
  REFUSED(table(0, 1, 399, N), "neither 0 nor >= 400");
  REFUSED(table(0, 1, 1, N), "neither 0 nor >= 400");
  REFUSED(table(0, 1, -400, N), "neither 0 nor >= 400");
  EXPECT(table(1, 0, N, N) == MLA_OK);                                            // an absent clip at the buffer's very end
  REFUSED(table(1, 2, 1, N), "not a sum");                                        // no samples, so no sum
  REFUSED(table(0, 2, 32767ll * 400 + 1, N), "not a sum");
  REFUSED(table(0, 2, -32768ll * 400 - 1, N), "not a sum");
  EXPECT(table(0, 2, -32768ll * 400, N) == MLA_OK);
  REFUSED(table(2, 3, 7, N), "reserved");
  REFUSED(wavfb_table_check(ok, B, (size_t)-1), "too large");
  REFUSED(wavfb_table_check(ok, B, (size_t)(INT64_MAX / 32768) + 1), "too large");
  const int64_t huge = INT64_MAX / 32768;                                          // the largest buffer: 32768 * n_samples fits int64
  EXPECT(table(2, 1, huge - ok[WAVFB_DESC * 2], (size_t)huge) == MLA_OK);

  // sparse mel runs inside [0, 256), and as many weights as they hold
  auto mel = [&](int bank, int32_t s, int32_t l, size_t n) {
    memcpy(ms, start, sizeof(ms));
    memcpy(ml, len, sizeof(ml));
    if (bank >= 0) { ms[bank] = s; ml[bank] = l; }
    return wavfb_mel_check(ms, ml, n);
  };
  EXPECT(mel(-1, 0, 0, NW) == MLA_OK);
  REFUSED(mel(5, -1, 2, NW), "outside [0, 256)");
  REFUSED(mel(5, 10, -1, NW), "outside [0, 256)");
  REFUSED(mel(127, 255, 2, NW), "outside [0, 256)");                              // would read the Nyquist bin
  REFUSED(mel(127, 257, 0, NW - 2), "outside [0, 256)");
  REFUSED(mel(0, INT32_MAX, INT32_MAX, NW), "outside [0, 256)");
  EXPECT(mel(3, 256, 0, NW - 2) == MLA_OK);                                       // an empty bank
  EXPECT(mel(3, 0, 256, NW + 254) == MLA_OK);
  REFUSED(mel(-1, 0, 0, NW - 1), "hold 256 weights");
  REFUSED(mel(-1, 0, 0, NW + 1), "hold 256 weights");
  return host_check_done("wav fbank");
}
