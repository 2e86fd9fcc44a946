// Stand-alone host check of the argument validation and launch plans of mla_rows_gather / mla_rows_expand / mla_rows_compact_sum
// (rows_args.h) with util.cpp's error reporting.  No GPU, no HIP: `make host-check` builds it with -fsanitize=address,undefined and
// runs it.
#include "rows_args.h"
#include "host_check.h"

int main() {
  enum { B = 5, ROW = 8 };                               // rows of 32 bytes
  alignas(16) static float src[B * ROW], dst[(B + 1) * ROW];
  alignas(16) static int64_t dev[B];                     // stands for the device tables: only its address is looked at
  const int64_t idx[2] = {4, 0}, all[B] = {0, 1, 2, 3, 4}, map[B] = {2, 0, 2, 1, 2}, absent[3] = {1, 3, 2};
  RowsPlan p;

  // ---- gather
  auto gather = [&](const void* s, const int64_t* d, const int64_t* h, const void* o, int b, int P, size_t row, int eb, int tail) {
    return rows_gather_plan(s, d, h, o, b, P, row, eb, tail, &p);
  };
  EXPECT(gather(src, dev, idx, dst, B, 2, ROW, 4, 1) == MLA_OK);
  EXPECT(p.vec16 == 1 && p.units == 2 && p.blocks_x == 1 && p.rows == 3);
  EXPECT(gather(src, dev, idx, dst, B, 2, ROW / 2, 8, 1) == MLA_OK && p.vec16 == 1 && p.units == 2);      // int64 rows of the same bytes
  EXPECT(gather(src, dev, idx, dst, B, 2, 3, 4, 1) == MLA_OK && p.vec16 == 0 && p.units == 3);             // rows of 12 bytes: words
  EXPECT(gather(src + 1, dev, idx, dst, 4, 2, ROW, 4, 0) == MLA_ERR_INVALID_ARG);                          // idx[0] = 4 of 4 rows
  EXPECT(gather(src + 1, dev, all, dst, 4, 4, ROW, 4, 0) == MLA_OK && p.vec16 == 0 && p.units == 8);       // a base off 16 bytes: words
  EXPECT(gather(src, dev, all, dst, B, B, ROW, 4, 1) == MLA_OK && p.rows == B + 1);
  EXPECT(gather(nullptr, nullptr, nullptr, dst, B, 0, ROW, 4, 1) == MLA_OK && p.rows == 1);                // the zero row alone
  REFUSED(gather(nullptr, dev, idx, dst, B, 2, ROW, 4, 1), "null pointer");
  REFUSED(gather(src, nullptr, idx, dst, B, 2, ROW, 4, 1), "null pointer");
  REFUSED(gather(src, dev, nullptr, dst, B, 2, ROW, 4, 1), "null pointer");
  REFUSED(gather(src, dev, idx, nullptr, B, 2, ROW, 4, 1), "null pointer");
  REFUSED(gather(src, dev, idx, dst, B, -1, ROW, 4, 1), "0 <= P <= B");
  REFUSED(gather(src, dev, all, dst, 4, 5, ROW, 4, 1), "0 <= P <= B");
  REFUSED(gather(src, dev, idx, dst, B, 2, ROW, 4, -1), "zero_tail_rows >= 0");
  REFUSED(gather(src, dev, idx, dst, 0, 0, ROW, 4, 1), "B > 0");
  REFUSED(gather(src, dev, idx, dst, B, 2, 0, 4, 1), "row_elems");
  REFUSED(gather(src, dev, idx, dst, B, 2, ((size_t)1 << 40) + 1, 4, 1), "row_elems");
  REFUSED(gather(src, dev, idx, dst, B, 0, ROW, 4, 0), "0 destination rows");
  REFUSED(gather(src, dev, idx, dst, B, 2, ROW, 4, ROWS_MAX_ROWS), "destination rows");
  REFUSED(gather(src, dev, idx, dst, B, 2, ROW, 2, 1), "2 bytes");
  REFUSED(gather((const char*)src + 2, dev, idx, dst, B, 2, ROW, 4, 1), "4-byte aligned");
  REFUSED(gather(src, (const int64_t*)((const char*)dev + 4), idx, dst, B, 2, ROW, 4, 1), "8-byte aligned");
  REFUSED(gather(src, dev, idx, src + 4 * ROW, B, 2, ROW, 4, 1), "overlaps");                              // dst = the last source row
  EXPECT(gather(dst, dev, idx, dst + B * ROW, B, 0, ROW, 4, 1) == MLA_OK);                                 // directly behind: apart
  const int64_t low[2] = {0, -1}, high[2] = {5, 0};
  REFUSED(gather(src, dev, low, dst, B, 2, ROW, 4, 1), "idx[1] = -1");
  REFUSED(gather(src, dev, high, dst, B, 2, ROW, 4, 1), "idx[0] = 5 is outside [0, 5)");

  // ---- expand: B destination rows from 3 source rows
  auto expand = [&](const void* s, const int64_t* d, const int64_t* h, const void* o, int b, int S, size_t row, int eb) {
    return rows_expand_plan(s, d, h, o, b, S, row, eb, &p);
  };
  EXPECT(expand(src, dev, map, dst, B, 3, ROW, 4) == MLA_OK && p.rows == B && p.vec16 == 1);
  REFUSED(expand(nullptr, dev, map, dst, B, 3, ROW, 4), "null pointer");
  REFUSED(expand(src, nullptr, map, dst, B, 3, ROW, 4), "null pointer");
  REFUSED(expand(src, dev, nullptr, dst, B, 3, ROW, 4), "null pointer");
  REFUSED(expand(src, dev, map, nullptr, B, 3, ROW, 4), "null pointer");
  REFUSED(expand(src, dev, map, dst, 0, 3, ROW, 4), "0 destination rows");
  REFUSED(expand(src, dev, map, dst, B, 0, ROW, 4), "src_rows = 0");
  REFUSED(expand(src, dev, map, dst, B, 3, 0, 4), "row_elems");
  REFUSED(expand(src, dev, map, dst, B, 2, ROW, 4), "map[0] = 2 is outside [0, 2)");
  REFUSED(expand(src, dev, map, src + ROW, B, 3, ROW, 4), "overlaps");

  // ---- compact_sum: 2 present rows, 3 absent ones
  auto csum = [&](const void* s, const int64_t* d, const int64_t* h, const int64_t* ad, const int64_t* ah, const void* o, int b, int P, int A,
                  size_t row) { return rows_compact_sum_plan(s, d, h, ad, ah, o, b, P, A, row, &p); };
  EXPECT(csum(src, dev, idx, dev, absent, dst, B, 2, 3, ROW) == MLA_OK && p.rows == 3);
  EXPECT(csum(src, nullptr, nullptr, dev, all, dst, B, 0, B, ROW) == MLA_OK && p.rows == 1);               // nothing present
  EXPECT(csum(src, dev, all, nullptr, nullptr, dst, B, B, 0, ROW) == MLA_OK && p.rows == B + 1);           // nothing absent
  REFUSED(csum(nullptr, dev, idx, dev, absent, dst, B, 2, 3, ROW), "null pointer");
  REFUSED(csum(src, dev, idx, dev, nullptr, dst, B, 2, 3, ROW), "null pointer");
  REFUSED(csum(src, nullptr, idx, dev, absent, dst, B, 2, 3, ROW), "null pointer");
  REFUSED(csum(src, dev, all, dev, absent, dst, 4, 5, 3, ROW), "0 <= P <= B");
  REFUSED(csum(src, dev, idx, dev, absent, dst, B, 2, -1, ROW), "A >= 0");
  REFUSED(csum(src, dev, idx, dev, absent, dst, B, 2, 3, 0), "row_elems");
  REFUSED(csum(src, dev, idx, dev, absent, dst, 3, 2, 3, ROW), "idx[0] = 4");
  REFUSED(csum(src, dev, all, dev, absent, dst, 3, 3, 3, ROW), "absent_idx[1] = 3 is outside [0, 3)");
  REFUSED(csum(src, dev, idx, dev, absent, src, B, 2, 3, ROW), "overlaps");

  // the plan at the training shapes: one 3 x 256 x 256 image row per sample, B = 32 -- units and the capped grid
  EXPECT(gather((const void*)0x1000000, dev, all, (const void*)0x40000000, 32, 5, 196608, 4, 1) == MLA_OK);
  EXPECT(p.vec16 == 1 && p.units == 49152 && p.blocks_x == 192 && (size_t)p.blocks_x * p.rows <= ROWS_MAX_BLOCKS);
  EXPECT(expand((const void*)0x1000000, dev, map, (const void*)0x40000000, 5, 3, 768, 4) == MLA_OK && p.units == 192 && p.blocks_x == 1);
  return host_check_done("rows");
}
