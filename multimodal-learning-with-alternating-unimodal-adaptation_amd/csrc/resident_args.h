// Host half of mla_resident_plan / mla_resident_batch (resident.hip): the checks of the frame table, which the store builds on the
// host once, the worst-case LDS plan over every crop the device draw can produce, and the per-batch argument checks.  Plain C++
// with no HIP in it, so resident_host_check.cpp builds it with the host sanitizers.
//
// The draw (resident_draw_kernel) is RandomResizedCrop.get_params + RandomHorizontalFlip on Philox4x32-10 (philox.h):
//     philox4x32(counter, stream_id, key)   key       = (epoch << 32) | seed      seed, epoch < 2^32: distinct pairs, distinct keys
//                                           stream_id = dataset index i           (64 bits)
//                                           counter   = (frame slot t << 4) | k   k = 0..9: try k;  k = 10: the flip
// so a frame's draw is a function of (seed, epoch, i, t) alone.  Try k reads the words a, b, c, d of its block:
//     target_area = H * W * (0.08 + 0.92 * (a * 2^-32));   aspect = exp(L0 + (L1 - L0) * (b * 2^-32))
//     w = rint(sqrt(target_area * aspect));  h = rint(sqrt(target_area / aspect))              fp64, no contraction
//     accepted when 0 < w <= W and 0 < h <= H:  top = (c * (H - h + 1)) >> 32,  left = (d * (W - w + 1)) >> 32
// after ten refusals the central crop of frames.sample_crop; flip = word 0 of block k = 10 < 2^31.
#pragma once
#include <limits.h>
#include <algorithm>
#include <utility>
#include <vector>
#include "args_common.h"
#include "frames_common.h"

#define RES_TABLE_COLS 3                          // frame table row: byte offset, H, W
#define RES_DESC_COLS 8                           // mla_frames_resample's descriptor row
#define RES_SPEC_ROW (1024 * 128)                 // floats per spectrogram
#define RES_TRIES 10
#define RES_FLIP_SLOT 10
#define RES_SCALE_LO 0.08                         // RandomResizedCrop(scale=(0.08, 1.0))
#define RES_SCALE_SPAN 0.92
#define RES_L0 (-0x1.269621134db92p-2)            // log(3 / 4) = -0.2876820724517809
#define RES_L1 (0x1.269621134db91p-2)             // log(4 / 3) =  0.28768207245178085
#define RES_RATIO_LO 0.75
#define RES_RATIO_HI (4.0 / 3.0)
#define RES_DRAW_THREADS 64
#define RES_GATHER_THREADS 256
#define RES_GATHER_UNITS 4                        // 16-byte units per thread

FR_HD static inline uint64_t res_key(uint64_t seed, uint64_t epoch) { return (epoch << 32) | seed; }
FR_HD static inline uint64_t res_counter(int t, int k) { return ((uint64_t)(uint32_t)t << 4) | (uint64_t)k; }

// table_host int64 (rows, 3): every frame inside the buffer, rows a whole number of samples of T frames
static inline int res_table_check(const int64_t* table_host, int64_t rows, int T, size_t frames_bytes) {
  MLA_REQUIRE(table_host, "mla_resident_plan: null frame table");
  MLA_REQUIRE(T > 0 && T < 65536, "mla_resident_plan: T=%d frames per sample out of range", T);
  MLA_REQUIRE(rows > 0 && rows % T == 0 && rows / T <= INT_MAX,
              "mla_resident_plan: %lld table rows are not N * T rows of N <= 2^31 - 1 samples with T=%d", (long long)rows, T);
  MLA_REQUIRE(frames_bytes <= (size_t)INT64_MAX, "mla_resident_plan: a buffer of %zu bytes is too large", frames_bytes);
  for (int64_t n = 0; n < rows; ++n) {
    const int64_t* d = table_host + (size_t)n * RES_TABLE_COLS;
    const int64_t off = d[0], H = d[1], W = d[2];
    MLA_REQUIRE(H > 0 && W > 0 && H <= FR_DIM_MAX && W <= FR_DIM_MAX, "mla_resident_plan: frame %lld: size %lldx%lld out of range",
                (long long)n, (long long)H, (long long)W);
    // H * W * 3 <= 3 * 2^32: no overflow; compared without forming off + size
    MLA_REQUIRE(off >= 0 && H * W * 3 <= (int64_t)frames_bytes && off <= (int64_t)frames_bytes - H * W * 3,
                "mla_resident_plan: frame %lld: bytes [%lld, %lld + %lld) lie outside the %zu-byte buffer", (long long)n, (long long)off,
                (long long)off, (long long)(H * W * 3), frames_bytes);
  }
  return MLA_OK;
}

static inline int res_out_check(const char* who, int out_h, int out_w) {
  MLA_REQUIRE(out_h > 0 && out_w > 0 && out_h <= 4096 && out_w <= 4096, "%s: output size %dx%d out of range", who, out_h, out_w);
  return MLA_OK;
}

// most source rows any band of `band` output rows reads when ch rows are resized to OH
static inline int res_band_rows(int ch, int OH, int band) {
  int rows = 1;
  for (int y0 = 0; y0 < OH; y0 += band) {
    const int y1 = std::min(y0 + band, OH) - 1;
    int a0, a1, b0, b1;
    fr_bounds(FR_BILINEAR, ch, OH, y0, &a0, &a1);
    fr_bounds(FR_BILINEAR, ch, OH, y1, &b0, &b1);
    rows = std::max(rows, b0 + b1 - a0);
  }
  return rows;
}

// The plan that holds for every crop the draw can make of the table's frames: ch in 1..H, cw in 1..W of every distinct shape
// (train), or the whole frames only (eval).  The coefficient counts grow with the crop; the rows a band reads are maximised
// over every ch, as they need not.
static inline int res_plan(const int64_t* table_host, int64_t rows, int T, size_t frames_bytes, int OH, int OW, int train,
                           FramePlan* plan) {
  MLA_TRY(res_out_check("mla_resident_plan", OH, OW));
  MLA_TRY(res_table_check(table_host, rows, T, frames_bytes));
  std::vector<std::pair<int, int>> shapes;
  for (int64_t n = 0; n < rows; ++n)
    shapes.emplace_back((int)table_host[(size_t)n * RES_TABLE_COLS + 1], (int)table_host[(size_t)n * RES_TABLE_COLS + 2]);
  std::sort(shapes.begin(), shapes.end());
  shapes.erase(std::unique(shapes.begin(), shapes.end()), shapes.end());
  int kh = 1, kv = 1;
  for (const auto& s : shapes) {
    kv = std::max(kv, fr_ksize(FR_BILINEAR, s.first, OH));
    kh = std::max(kh, fr_ksize(FR_BILINEAR, s.second, OW));
  }
  int worst_h = shapes[0].first, worst_w = shapes[0].second;
  for (int band = FR_BAND; band >= 1; band >>= 1) {
    // the whole frames first: when they do not fit, no maximisation is needed to know it
    int rows_cap = 1;
    for (const auto& s : shapes) {
      const int r = res_band_rows(s.first, OH, band);
      if (r > rows_cap) {
        rows_cap = r;
        worst_h = s.first;
        worst_w = s.second;
      }
    }
    if (fr_lds(OW, band, rows_cap, kh, kv) > FR_LDS_MAX) continue;
    if (train) {                                    // the crops of all shapes together have every height up to the tallest frame's
      const auto& tall = shapes.back();
      for (int ch = 1; ch < tall.first; ++ch) {
        const int r = res_band_rows(ch, OH, band);
        if (r > rows_cap) {
          rows_cap = r;
          worst_h = tall.first;
          worst_w = tall.second;
        }
      }
    }
    const size_t lds = fr_lds(OW, band, rows_cap, kh, kv);
    if (lds <= FR_LDS_MAX) {
      *plan = FramePlan{band, rows_cap, kh, kv, lds};
      return MLA_OK;
    }
  }
  MLA_REQUIRE(false, "mla_resident_plan: a %dx%d frame resized to %dx%d needs more than %d bytes of LDS in every band", worst_h, worst_w,
              OH, OW, FR_LDS_MAX);
  return MLA_ERR_INVALID_ARG;
}

// a plan5 (band, rows_cap, kh, kv, lds) as res_plan returns them for this output size
static inline int res_plan5_check(const int* plan5, int OH, int OW, FramePlan* plan) {
  MLA_REQUIRE(plan5, "mla_resident_batch: null plan");
  const int band = plan5[0], rows_cap = plan5[1], kh = plan5[2], kv = plan5[3];
  MLA_REQUIRE(band >= 1 && band <= FR_BAND && (band & (band - 1)) == 0, "mla_resident_batch: plan: band %d is not 16, 8, 4, 2 or 1", band);
  MLA_REQUIRE(rows_cap >= 1 && rows_cap <= FR_DIM_MAX, "mla_resident_batch: plan: rows_cap %d out of range", rows_cap);
  MLA_REQUIRE(kh >= 3 && kv >= 3 && (kh & 1) && (kv & 1) && kh <= 2 * FR_DIM_MAX + 1 && kv <= 2 * FR_DIM_MAX + 1,
              "mla_resident_batch: plan: %d / %d coefficients per output are not filter sizes", kh, kv);
  const size_t lds = fr_lds(OW, band, rows_cap, kh, kv);
  MLA_REQUIRE(lds <= FR_LDS_MAX, "mla_resident_batch: plan: needs %zu bytes of LDS (max %d)", lds, FR_LDS_MAX);
  MLA_REQUIRE(plan5[4] >= 0 && (size_t)plan5[4] == lds, "mla_resident_batch: plan: says %d bytes of LDS where its sizes need %zu", plan5[4], lds);
  *plan = FramePlan{band, rows_cap, kh, kv, lds};
  return MLA_OK;
}

static inline int res_batch_check(const void* frames, size_t frames_bytes, const void* table, const void* spec_table, const void* labels,
                                  const void* order, int N, int T, int pos, int b, uint64_t seed, uint64_t epoch, const int* plan5,
                                  const void* lut, const void* desc_out, const void* image_out, const void* spec_out,
                                  const void* label_out, const void* idx_out, int OH, int OW, FramePlan* plan) {
  MLA_REQUIRE(frames && table && labels && order && lut && desc_out && image_out && label_out && idx_out,
              "mla_resident_batch: null pointer");
  MLA_REQUIRE(!spec_table || spec_out, "mla_resident_batch: a spec table but no spec_out");
  MLA_REQUIRE(N > 0 && T > 0 && b > 0 && pos >= 0, "mla_resident_batch: need N, T, b > 0 and pos >= 0 (got N=%d T=%d b=%d pos=%d)", N, T, b,
              pos);
  MLA_REQUIRE((long long)pos + b <= N, "mla_resident_batch: batch [%d, %d + %d) leaves the order of N=%d", pos, pos, b, N);
  MLA_REQUIRE((long long)b * T < 65536, "mla_resident_batch: b * T = %d * %d frames per launch (max 65535)", b, T);
  MLA_REQUIRE(seed < (1ull << 32) && epoch < (1ull << 32), "mla_resident_batch: seed %llu and epoch %llu must be below 2^32",
              (unsigned long long)seed, (unsigned long long)epoch);
  MLA_REQUIRE(frames_bytes >= 3 && frames_bytes <= (size_t)INT64_MAX, "mla_resident_batch: a frame buffer of %zu bytes", frames_bytes);
  MLA_TRY(res_out_check("mla_resident_batch", OH, OW));
  MLA_TRY(res_plan5_check(plan5, OH, OW, plan));
  MLA_REQUIRE(!(((uintptr_t)table | (uintptr_t)labels | (uintptr_t)order | (uintptr_t)desc_out | (uintptr_t)label_out | (uintptr_t)idx_out) & 7),
              "mla_resident_batch: the frame table, labels, order, desc_out, label_out and idx_out must be 8-byte aligned");
  MLA_REQUIRE(!(((uintptr_t)lut | (uintptr_t)image_out) & 3), "mla_resident_batch: lut and image_out must be 4-byte aligned");
  MLA_REQUIRE(!(((uintptr_t)spec_table | (uintptr_t)(spec_table ? spec_out : nullptr)) & 15),
              "mla_resident_batch: spec_table and spec_out must be 16-byte aligned (rows move as 16-byte units)");
  return MLA_OK;
}
