// What the stand-alone *_host_check.cpp programs share: they check a host half (*_args.h) with util.cpp's error reporting, no GPU
// and no HIP, and `make host-check` builds them with -fsanitize=address,undefined and runs them.  One program, one translation unit.
#pragma once
#include <stdio.h>
#include <string.h>
#include "../../include/mla_hip.h"

extern "C" const char* mla_last_error(void);

static int failures = 0;
#define EXPECT(cond)                                               \
  do {                                                             \
    if (!(cond)) {                                                 \
      fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                  \
    }                                                              \
  } while (0)
// the call answers MLA_ERR_INVALID_ARG and leaves a message that holds `text`
#define REFUSED(call, text) \
  do {                      \
    EXPECT((call) == MLA_ERR_INVALID_ARG); \
    EXPECT(strstr(mla_last_error(), text)); \
  } while (0)

// what main returns: 1 after a failed EXPECT, else "<name> host check ok" and 0
static inline int host_check_done(const char* name) {
  if (failures) return 1;
  printf("%s host check ok\n", name);
  return 0;
}
