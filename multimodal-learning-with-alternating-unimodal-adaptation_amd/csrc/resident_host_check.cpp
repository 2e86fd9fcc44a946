// Stand-alone host check of mla_resident_plan's table checks and worst-case plan and of mla_resident_batch's argument validation
// (resident_args.h) with util.cpp's error reporting.  No GPU, no HIP: `make host-check` builds it with
// -fsanitize=address,undefined and runs it.
#include "resident_args.h"
#include "host_check.h"

int main() {
  // two samples of T = 3 frames, sizes mixed, packed back to back
  enum { T = 3, ROWS = 6 };
  const int sizes[ROWS][2] = {{36, 48}, {36, 48}, {50, 40}, {8, 200}, {90, 120}, {36, 48}};
  int64_t table[ROWS * RES_TABLE_COLS], t[ROWS * RES_TABLE_COLS];
  int64_t total = 0;
  for (int n = 0; n < ROWS; ++n) {
    table[3 * n] = total;
    table[3 * n + 1] = sizes[n][0];
    table[3 * n + 2] = sizes[n][1];
    total += (int64_t)sizes[n][0] * sizes[n][1] * 3;
  }
  FramePlan p, q;
  EXPECT(res_plan(table, ROWS, T, (size_t)total, 40, 40, 1, &p) == MLA_OK);
  EXPECT(p.band == 16 && p.lds == fr_lds(40, p.band, p.rows_cap, p.kh, p.kv) && p.lds <= FR_LDS_MAX);
  EXPECT(p.kh == fr_ksize(FR_BILINEAR, 200, 40) && p.kv == fr_ksize(FR_BILINEAR, 90, 40));
  // the train plan covers every crop height: it is at least the eval plan, and at least any single crop's need
  EXPECT(res_plan(table, ROWS, T, (size_t)total, 40, 40, 0, &q) == MLA_OK);
  EXPECT(q.band == p.band && q.kh == p.kh && q.kv == p.kv && q.rows_cap <= p.rows_cap);
  for (int ch = 1; ch <= 90; ++ch) EXPECT(res_band_rows(ch, 40, p.band) <= p.rows_cap);
  EXPECT(res_band_rows(90, 40, q.band) == q.rows_cap);
  // 480x360 -> 224: about 30 source rows per band of 16
  const int64_t crema[3] = {0, 360, 480};
  EXPECT(res_plan(crema, 1, 1, 360 * 480 * 3, 224, 224, 1, &p) == MLA_OK);
  EXPECT(p.band == 16 && p.rows_cap >= 26 && p.rows_cap <= 32 && p.kh == 7 && p.kv == 5);

  // the frame table
  auto plan = [&](int row, int col, int64_t v, int64_t rows, int tt, size_t bytes) {
    memcpy(t, table, sizeof(t));
    if (row >= 0) t[3 * row + col] = v;
    return res_plan(t, rows, tt, bytes, 40, 40, 1, &q);
  };
  EXPECT(plan(-1, 0, 0, ROWS, T, (size_t)total) == MLA_OK);
  REFUSED(plan(-1, 0, 0, ROWS, T, (size_t)total - 1), "lie outside");                // the last frame ends one byte past it
  REFUSED(plan(0, 0, -1, ROWS, T, (size_t)total), "lie outside");
  REFUSED(plan(5, 0, INT64_MAX, ROWS, T, (size_t)total), "lie outside");             // offset + size would overflow
  REFUSED(plan(2, 1, 0, ROWS, T, (size_t)total), "out of range");
  REFUSED(plan(2, 2, FR_DIM_MAX + 1, ROWS, T, (size_t)total), "out of range");
  REFUSED(plan(-1, 0, 0, ROWS - 1, T, (size_t)total), "are not N * T rows");
  REFUSED(plan(-1, 0, 0, 0, T, (size_t)total), "are not N * T rows");
  REFUSED(plan(-1, 0, 0, ROWS, 0, (size_t)total), "frames per sample");
  REFUSED(res_plan(nullptr, ROWS, T, (size_t)total, 40, 40, 1, &q), "null frame table");
  REFUSED(res_plan(table, ROWS, T, (size_t)total, 0, 40, 1, &q), "output size");
  REFUSED(res_plan(table, ROWS, T, (size_t)total, 40, 4097, 1, &q), "output size");
  // an offset above 2^32: accepted when the buffer is that large, refused by one byte when it is not
  const int64_t far_off = (5ll << 32) + 7;
  const int64_t far_row[3] = {far_off, 36, 48};
  EXPECT(res_plan(far_row, 1, 1, (size_t)(far_off + 36 * 48 * 3), 40, 40, 1, &q) == MLA_OK);
  REFUSED(res_plan(far_row, 1, 1, (size_t)(far_off + 36 * 48 * 3 - 1), 40, 40, 1, &q), "lie outside");
  // a frame no band of which fits 64 KB of LDS: the message names it
  const int64_t tall[3] = {0, 65536, 2};
  REFUSED(res_plan(tall, 1, 1, 65536 * 2 * 3, 4, 4096, 0, &q), "65536x2 frame");

  // the per-batch checks
  EXPECT(res_plan(table, ROWS, T, (size_t)total, 40, 40, 1, &p) == MLA_OK);
  int plan5[5] = {p.band, p.rows_cap, p.kh, p.kv, (int)p.lds};
  alignas(16) static char buf[64];
  const void* a = buf;
  auto batch = [&](const void* frames, const void* spec, const void* spec_out, int N, int pos, int b, uint64_t seed, uint64_t epoch,
                   const int* pl, int oh, int ow) {
    return res_batch_check(frames, (size_t)total, a, spec, a, a, N, T, pos, b, seed, epoch, pl, a, a, a, spec_out, a, a, oh, ow, &q);
  };
  EXPECT(batch(a, a, a, 2, 0, 2, 0, 0, plan5, 40, 40) == MLA_OK);
  EXPECT(q.band == p.band && q.rows_cap == p.rows_cap && q.lds == p.lds);
  EXPECT(batch(a, nullptr, nullptr, 2, 1, 1, 0xFFFFFFFFull, 0xFFFFFFFFull, plan5, 40, 40) == MLA_OK);
  REFUSED(batch(nullptr, a, a, 2, 0, 2, 0, 0, plan5, 40, 40), "null pointer");
  REFUSED(batch(a, a, nullptr, 2, 0, 2, 0, 0, plan5, 40, 40), "no spec_out");
  REFUSED(batch(a, a, a, 2, 1, 2, 0, 0, plan5, 40, 40), "leaves the order");
  REFUSED(batch(a, a, a, 2, -1, 2, 0, 0, plan5, 40, 40), "pos >= 0");
  REFUSED(batch(a, a, a, 2, 0, 0, 0, 0, plan5, 40, 40), "b > 0");
  REFUSED(batch(a, a, a, INT_MAX, INT_MAX - 1, 2, 0, 0, plan5, 40, 40), "leaves the order");   // pos + b does not wrap
  REFUSED(batch(a, a, a, 100000, 0, 21846, 0, 0, plan5, 40, 40), "max 65535");                 // 21846 * 3 = 65538
  EXPECT(batch(a, a, a, 100000, 0, 21845, 0, 0, plan5, 40, 40) == MLA_OK);                     // 65535
  REFUSED(batch(a, a, a, 2, 0, 2, 1ull << 32, 0, plan5, 40, 40), "below 2^32");
  REFUSED(batch(a, a, a, 2, 0, 2, 0, 1ull << 32, plan5, 40, 40), "below 2^32");
  REFUSED(batch(a, a, a, 2, 0, 2, 0, 0, nullptr, 40, 40), "null plan");
  REFUSED(batch((const char*)a + 0, (const char*)a + 8, a, 2, 0, 2, 0, 0, plan5, 40, 40), "16-byte aligned");
  REFUSED(batch(a, a, (const char*)a + 4, 2, 0, 2, 0, 0, plan5, 40, 40), "16-byte aligned");
  REFUSED(res_batch_check(a, (size_t)total, (const char*)a + 4, a, a, a, 2, T, 0, 2, 0, 0, plan5, a, a, a, a, a, a, 40, 40, &q), "8-byte aligned");
  REFUSED(res_batch_check(a, (size_t)total, a, a, a, a, 2, T, 0, 2, 0, 0, plan5, (const char*)a + 2, a, a, a, a, a, 40, 40, &q), "4-byte aligned");
  // forged plans
  auto forged = [&](int k, int v, int ow) {
    int f[5];
    memcpy(f, plan5, sizeof(f));
    f[k] = v;
    return batch(a, a, a, 2, 0, 2, 0, 0, f, 40, ow);
  };
  REFUSED(forged(0, 12, 40), "band 12");
  REFUSED(forged(0, 32, 40), "band 32");
  REFUSED(forged(0, 0, 40), "band 0");
  REFUSED(forged(1, 0, 40), "rows_cap");
  REFUSED(forged(2, 4, 40), "filter sizes");
  REFUSED(forged(3, 1, 40), "filter sizes");
  REFUSED(forged(4, (int)p.lds - 16, 40), "bytes of LDS where");
  REFUSED(forged(1, p.rows_cap + 1, 40), "bytes of LDS where");              // a larger cap with the old byte count
  REFUSED(forged(1, 60000, 40), "bytes of LDS (max");
  REFUSED(forged(4, (int)p.lds, 48), "bytes of LDS where");                  // the same plan at another output width
  return host_check_done("resident");
}
