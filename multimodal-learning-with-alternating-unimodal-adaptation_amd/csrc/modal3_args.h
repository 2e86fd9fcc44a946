// Host half of mla_modal3_assemble (modal3.hip): the checks of the mask table, which the batcher builds on the host, and of the
// buffers, and the launch plan.  Plain C++ with no HIP in it, so modal3_host_check.cpp builds it with the host sanitizers.
#pragma once
#include <vector>
#include "args_common.h"

#define MODAL3_DESC 4           // audio present, image present, text present, image slot
#define MODAL3_THREADS 256
#define MODAL3_MAX_BLOCKS 2048  // 8 workgroups of 256 on each of 256 CUs; the grid-stride loop takes the rest

// One sample's work in 16-byte units: [0, image) the image row, then the spectrogram, token and padding-mask rows.
struct Modal3Plan {
  int image, spec, token, pm, total;     // units per sample of each range, and their sum
  int blocks_x;                          // grid = (blocks_x, B); a thread strides over `total` by blocks_x * MODAL3_THREADS
};

// mdesc_host int64 (B, 4): flags in {0, 1}; the slots of the rows with an image are a permutation of 0..P-1 (so no two rows read, and
// no row reads beyond, the P compact images), the other rows hold -1; P is the number of rows with an image.
static inline int modal3_table_check(const int64_t* mdesc_host, int B, int P) {
  MLA_REQUIRE(mdesc_host, "mla_modal3_assemble: null mask table");
  MLA_REQUIRE(B > 0 && B < 65536 && P >= 0 && P <= B, "mla_modal3_assemble: need 0 < B < 65536 and 0 <= P <= B (got B=%d, P=%d)", B, P);
  std::vector<uint8_t> seen((size_t)P, 0);
  int present = 0;
  for (int b = 0; b < B; ++b) {
    const int64_t* d = mdesc_host + (size_t)b * MODAL3_DESC;
    for (int c = 0; c < 3; ++c)
      MLA_REQUIRE(d[c] == 0 || d[c] == 1, "mla_modal3_assemble: sample %d: flag %d is %lld, not 0 or 1", b, c, (long long)d[c]);
    const int64_t slot = d[3];
    if (!d[1]) {
      MLA_REQUIRE(slot == -1, "mla_modal3_assemble: sample %d has no image but slot %lld (want -1)", b, (long long)slot);
      continue;
    }
    ++present;
    MLA_REQUIRE(slot >= 0 && slot < P, "mla_modal3_assemble: sample %d: image slot %lld is outside [0, %d)", b, (long long)slot, P);
    MLA_REQUIRE(!seen[(size_t)slot], "mla_modal3_assemble: sample %d: image slot %lld is used twice", b, (long long)slot);
    seen[(size_t)slot] = 1;
  }
  MLA_REQUIRE(present == P, "mla_modal3_assemble: %d samples have an image but P=%d", present, P);
  return MLA_OK;
}

// Sizes: every row a whole number of 16-byte units (3*S*S and T*F multiples of 4 floats, L a multiple of 4 so that the fp32
// padding-mask row is; the int64 token row then is too).
static inline int modal3_shape_plan(int B, int S, int TF, int L, Modal3Plan* out) {
  MLA_REQUIRE(B > 0 && S > 0 && TF > 0 && L > 0, "mla_modal3_assemble: need B, S, T*F, L > 0 (got %d, %d, %d, %d)", B, S, TF, L);
  const long long img = 3ll * S * S;
  MLA_REQUIRE(img % 4 == 0 && TF % 4 == 0 && L % 4 == 0,
              "mla_modal3_assemble: 3*S*S=%lld, T*F=%d and L=%d must be multiples of 4 (rows move as 16-byte units)", img, TF, L);
  const long long total = img / 4 + TF / 4 + L / 2 + L / 4;
  MLA_REQUIRE(total < (1ll << 31), "mla_modal3_assemble: a sample of %lld 16-byte units is too large (max 2^31 - 1)", total);
  out->image = (int)(img / 4);
  out->spec = TF / 4;
  out->token = L / 2;
  out->pm = L / 4;
  out->total = (int)total;
  out->blocks_x = (int)mla_strided_blocks((size_t)total, MODAL3_THREADS, MODAL3_MAX_BLOCKS, (unsigned)B);
  return MLA_OK;
}

static inline int modal3_plan(const void* image_compact, const void* spec, const void* token, const void* pm, const void* mdesc,
                              const int64_t* mdesc_host, const void* image_out, int B, int P, int S, int TF, int L,
                              Modal3Plan* out) {
  MLA_REQUIRE(spec && token && pm && mdesc && mdesc_host && image_out && (P <= 0 || image_compact), "mla_modal3_assemble: null pointer");
  MLA_TRY(modal3_shape_plan(B, S, TF, L, out));
  MLA_REQUIRE(!(((uintptr_t)image_compact | (uintptr_t)spec | (uintptr_t)token | (uintptr_t)pm | (uintptr_t)image_out) & 15),
              "mla_modal3_assemble: image, spec, token and padding-mask buffers must be 16-byte aligned");
  MLA_REQUIRE(!((uintptr_t)mdesc & 7), "mla_modal3_assemble: the mask table must be 8-byte aligned");
  MLA_TRY(modal3_table_check(mdesc_host, B, P));
  const size_t img = (size_t)out->image * 16, nout = (size_t)B * img;
  MLA_REQUIRE(!mla_overlap(image_out, nout, image_compact, (size_t)P * img) && !mla_overlap(image_out, nout, spec, (size_t)B * TF * 4) &&
                  !mla_overlap(image_out, nout, token, (size_t)B * L * 8) && !mla_overlap(image_out, nout, pm, (size_t)B * L * 4) &&
                  !mla_overlap(image_out, nout, mdesc, (size_t)B * MODAL3_DESC * 8),
              "mla_modal3_assemble: image_out overlaps an input");
  return MLA_OK;
}
