// Host half of mla_rows_gather / mla_rows_expand / mla_rows_compact_sum (rows.hip): the checks of the index tables, which the caller
// builds on the host, and of the buffers, and the launch plan.  Plain C++ with no HIP in it, so rows_host_check.cpp builds it with
// the host sanitizers.
#pragma once
#include "args_common.h"

#define ROWS_THREADS 256
#define ROWS_MAX_BLOCKS 2048     // 8 workgroups of 256 on each of 256 CUs; the grid-stride loop takes the rest
#define ROWS_MAX_ROWS 65535      // gridDim.y

// One launch: grid = (blocks_x, rows), a thread strides over the `units` of its row by blocks_x * ROWS_THREADS.  A unit is 16 bytes
// when both bases and the row size are multiples of 16 (every row then starts on a 16-byte boundary), else one 4-byte word.
struct RowsPlan {
  int vec16;
  size_t units;
  unsigned blocks_x;
  int rows;
};

static inline int rows_table_check(const char* who, const char* what, const int64_t* host, int n, int64_t bound) {
  for (int j = 0; j < n; ++j)
    MLA_REQUIRE(host[j] >= 0 && host[j] < bound, "%s: %s[%d] = %lld is outside [0, %lld)", who, what, j, (long long)host[j], (long long)bound);
  return MLA_OK;
}

// what every entry point shares: B source rows and `out_rows` destination rows of row_elems elements of elem_bytes each, src and
// dst 4-byte aligned and apart; fills the plan
static inline int rows_buffers_plan(const char* who, const void* src, const void* dst, int B, int out_rows, size_t row_elems,
                                    int elem_bytes, RowsPlan* out) {
  MLA_REQUIRE(elem_bytes == 4 || elem_bytes == 8, "%s: elements of %d bytes (4 or 8)", who, elem_bytes);
  MLA_REQUIRE(B > 0 && row_elems > 0 && row_elems <= ((size_t)1 << 40), "%s: need B > 0 and 0 < row_elems <= 2^40 (got B=%d, row_elems=%zu)",
              who, B, row_elems);
  MLA_REQUIRE(out_rows > 0 && out_rows <= ROWS_MAX_ROWS, "%s: %d destination rows (1 .. %d)", who, out_rows, ROWS_MAX_ROWS);
  MLA_REQUIRE((((uintptr_t)src | (uintptr_t)dst) & 3) == 0, "%s: src / dst must be 4-byte aligned", who);
  const size_t row_bytes = row_elems * (size_t)elem_bytes;
  MLA_REQUIRE(!mla_overlap(dst, (size_t)out_rows * row_bytes, src, (size_t)B * row_bytes), "%s: dst overlaps src", who);
  out->vec16 = (((uintptr_t)src | (uintptr_t)dst | row_bytes) & 15) == 0;
  out->units = row_bytes / (out->vec16 ? 16 : 4);
  out->blocks_x = mla_strided_blocks(out->units, ROWS_THREADS, ROWS_MAX_BLOCKS, (unsigned)out_rows);
  out->rows = out_rows;
  return MLA_OK;
}

static inline int rows_gather_plan(const void* src, const int64_t* idx, const int64_t* idx_host, const void* dst, int B, int P,
                                   size_t row_elems, int elem_bytes, int zero_tail_rows, RowsPlan* out) {
  const char* who = "mla_rows_gather";
  MLA_REQUIRE(dst && (P <= 0 || (src && idx && idx_host)), "%s: null pointer", who);
  MLA_REQUIRE(P >= 0 && P <= B && zero_tail_rows >= 0 && zero_tail_rows <= ROWS_MAX_ROWS,
              "%s: need 0 <= P <= B and zero_tail_rows >= 0 (got P=%d, B=%d, zero_tail_rows=%d)", who, P, B, zero_tail_rows);
  MLA_REQUIRE(((uintptr_t)idx & 7) == 0, "%s: idx must be 8-byte aligned", who);
  MLA_TRY(rows_buffers_plan(who, src, dst, B, P + zero_tail_rows, row_elems, elem_bytes, out));
  return rows_table_check(who, "idx", idx_host, P, B);
}

static inline int rows_expand_plan(const void* src, const int64_t* map, const int64_t* map_host, const void* dst, int B, int src_rows,
                                   size_t row_elems, int elem_bytes, RowsPlan* out) {
  const char* who = "mla_rows_expand";
  MLA_REQUIRE(src && map && map_host && dst, "%s: null pointer", who);
  MLA_REQUIRE(src_rows > 0, "%s: src_rows = %d", who, src_rows);
  MLA_REQUIRE(((uintptr_t)map & 7) == 0, "%s: map must be 8-byte aligned", who);
  MLA_TRY(rows_buffers_plan(who, src, dst, src_rows, B, row_elems, elem_bytes, out));
  return rows_table_check(who, "map", map_host, B, src_rows);
}

static inline int rows_compact_sum_plan(const void* src, const int64_t* idx, const int64_t* idx_host, const int64_t* absent_idx,
                                        const int64_t* absent_host, const void* dst, int B, int P, int A, size_t row_elems, RowsPlan* out) {
  const char* who = "mla_rows_compact_sum";
  MLA_REQUIRE(src && dst && (P <= 0 || (idx && idx_host)) && (A <= 0 || (absent_idx && absent_host)), "%s: null pointer", who);
  MLA_REQUIRE(P >= 0 && P <= B && P < ROWS_MAX_ROWS && A >= 0, "%s: need 0 <= P <= B and A >= 0 (got P=%d, B=%d, A=%d)", who, P, B, A);
  MLA_REQUIRE((((uintptr_t)idx | (uintptr_t)absent_idx) & 7) == 0, "%s: the index tables must be 8-byte aligned", who);
  MLA_TRY(rows_buffers_plan(who, src, dst, B, P + 1, row_elems, 4, out));
  MLA_TRY(rows_table_check(who, "idx", idx_host, P, B));
  return rows_table_check(who, "absent_idx", absent_host, A, B);
}
