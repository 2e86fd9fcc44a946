// What every host half (*_args.h) and every wrapper checks its arguments with.  Plain C++ with no HIP in it: common.h includes it for
// the kernels' files, the *_host_check.cpp programs reach it through their *_args.h and build with the host sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/mla_hip.h"

void mla_set_error(const char* fmt, ...);      // util.cpp; mla_last_error() answers the text

// refuse with a message unless cond holds
#define MLA_REQUIRE(cond, ...)              \
  do {                                      \
    if (!(cond)) {                          \
      mla_set_error(__VA_ARGS__);           \
      return MLA_ERR_INVALID_ARG;           \
    }                                       \
  } while (0)

// pass a failed status on (its message is set already)
#define MLA_TRY(expr)                       \
  do {                                      \
    const int rc__ = (expr);                \
    if (rc__ != MLA_OK) return rc__;        \
  } while (0)

// do the byte ranges [a, a + na) and [b, b + nb) share a byte?  Null or empty ranges share none.
static inline int mla_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return a && b && na && nb && x < y + nb && y < x + na;
}

// grid.x of a (blocks_x, rows) launch whose threads stride over the `units` of their row: enough blocks to give every unit a thread,
// but no more than max_blocks workgroups in the whole grid (the grid-stride loop takes the rest), and at least one
static inline unsigned mla_strided_blocks(size_t units, unsigned threads, unsigned max_blocks, unsigned rows) {
  const size_t bx = (units + threads - 1) / threads, cap = max_blocks / rows < 1 ? 1 : max_blocks / rows;
  return (unsigned)(bx < cap ? bx : cap);
}
