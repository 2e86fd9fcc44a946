// Stand-alone host check of mla_modal3_assemble's argument validation and launch plan (modal3_args.h) with util.cpp's error
// reporting.  No GPU, no HIP: `make host-check` builds it with -fsanitize=address,undefined and runs it.
#include "modal3_args.h"
#include "host_check.h"

int main() {
  // B = 7, S = 2, T*F = 8, L = 4: image rows of 48 B, spectrogram rows of 32 B, token rows of 32 B, padding-mask rows of 16 B
  enum { B = 7, S = 2, TF = 8, L = 4 };
  alignas(16) static float compact[B * 12], out[B * 12], spec[B * TF], pm[B * L];
  alignas(16) static int64_t token[B * L], dev[B * MODAL3_DESC];
  // every non-zero mask row; the slots of the four rows with an image are not in batch order
  const int64_t ok[B * MODAL3_DESC] = {1, 0, 0, -1, 0, 1, 0, 2, 0, 0, 1, -1, 1, 1, 0, 0, 1, 0, 1, -1, 0, 1, 1, 3, 1, 1, 1, 1};
  int64_t t[B * MODAL3_DESC];
  Modal3Plan p;
  auto plan = [&](const void* ic, const void* sp, const void* tk, const void* pk, const void* md, const int64_t* mh, const void* io,
                  int b, int P, int s, int tf, int l) { return modal3_plan(ic, sp, tk, pk, md, mh, io, b, P, s, tf, l, &p); };
  EXPECT(plan(compact, spec, token, pm, dev, ok, out, B, 4, S, TF, L) == MLA_OK);
  EXPECT(p.image == 3 && p.spec == 2 && p.token == 2 && p.pm == 1 && p.total == 8 && p.blocks_x == 1);

  // null pointers, one at a time; image_compact may be null only when no sample has an image
  const void* args[7] = {compact, spec, token, pm, dev, ok, out};
  for (int z = 0; z < 7; ++z) {
    const void* a[7];
    memcpy(a, args, sizeof(a));
    a[z] = nullptr;
    REFUSED(plan(a[0], a[1], a[2], a[3], a[4], (const int64_t*)a[5], a[6], B, 4, S, TF, L), "null pointer");
  }
  for (int i = 0; i < B; ++i) { t[4 * i] = 1; t[4 * i + 1] = 0; t[4 * i + 2] = i & 1; t[4 * i + 3] = -1; }
  EXPECT(plan(nullptr, spec, token, pm, dev, t, out, B, 0, S, TF, L) == MLA_OK);
  REFUSED(modal3_table_check(nullptr, B, 4), "null mask table");

  // sizes
  REFUSED(plan(compact, spec, token, pm, dev, ok, out, 0, 4, S, TF, L), "> 0");
  REFUSED(plan(compact, spec, token, pm, dev, ok, out, B, 4, 0, TF, L), "> 0");
  REFUSED(plan(compact, spec, token, pm, dev, ok, out, B, 4, S, -8, L), "> 0");
  REFUSED(plan(compact, spec, token, pm, dev, ok, out, B, 4, S, TF, 0), "> 0");
  REFUSED(plan(compact, spec, token, pm, dev, ok, out, B, 4, 3, TF, L), "multiples of 4");      // 3 * 3 * 3 = 27 floats
  REFUSED(plan(compact, spec, token, pm, dev, ok, out, B, 4, S, 6, L), "multiples of 4");
  REFUSED(plan(compact, spec, token, pm, dev, ok, out, B, 4, S, TF, 6), "multiples of 4");      // token row whole, padding-mask row not
  REFUSED(modal3_shape_plan(B, 60000, TF, L, &p), "too large");
  REFUSED(modal3_table_check(ok, 65536, 4), "B < 65536");
  REFUSED(modal3_table_check(ok, B, -1), "0 <= P <= B");
  REFUSED(modal3_table_check(ok, B, B + 1), "0 <= P <= B");

  // alignment
  REFUSED(plan(compact + 1, spec, token, pm, dev, ok, out, B, 4, S, TF, L), "16-byte aligned");
  REFUSED(plan(compact, spec + 2, token, pm, dev, ok, out, B, 4, S, TF, L), "16-byte aligned");
  REFUSED(plan(compact, spec, token + 1, pm, dev, ok, out, B, 4, S, TF, L), "16-byte aligned");
  REFUSED(plan(compact, spec, token, pm + 3, dev, ok, out, B, 4, S, TF, L), "16-byte aligned");
  REFUSED(plan(compact, spec, token, pm, dev, ok, out + 1, B, 4, S, TF, L), "16-byte aligned");
  REFUSED(plan(compact, spec, token, pm, (const char*)dev + 4, ok, out, B, 4, S, TF, L), "8-byte aligned");

  // image_out overlapping an input: its first and its last unit, and each input in turn
  REFUSED(plan(out, spec, token, pm, dev, ok, out, B, 4, S, TF, L), "overlaps");
  REFUSED(plan(out + B * 12 - 4, spec, token, pm, dev, ok, out, B, 4, S, TF, L), "overlaps");
  REFUSED(plan(compact, spec, token, pm, dev, ok, (float*)spec, B, 4, S, TF, L), "overlaps");
  REFUSED(plan(compact, spec, token, pm, dev, ok, (float*)token, B, 4, S, TF, L), "overlaps");
  REFUSED(plan(compact, spec, token, pm, dev, ok, (float*)dev, B, 4, S, TF, L), "overlaps");
  {
    alignas(16) static float both[B * 12 + B * L];                // the padding mask directly behind image_out: adjacent is fine
    EXPECT(plan(compact, spec, token, both + B * 12, dev, ok, both, B, 4, S, TF, L) == MLA_OK);
    REFUSED(plan(compact, spec, token, both + B * 12 - 4, dev, ok, both, B, 4, S, TF, L), "overlaps");
  }

  // the table: flags, slots, P
  auto table = [&](int row, int col, int64_t v, int P) {
    memcpy(t, ok, sizeof(t));
    if (row >= 0) t[4 * row + col] = v;
    return modal3_table_check(t, B, P);
  };
  EXPECT(table(-1, 0, 0, 4) == MLA_OK);
  REFUSED(table(0, 0, 2, 4), "not 0 or 1");
  REFUSED(table(2, 2, -1, 4), "not 0 or 1");
  REFUSED(table(3, 1, 7, 4), "not 0 or 1");
  REFUSED(table(0, 3, 0, 4), "has no image but slot 0");
  REFUSED(table(1, 3, -1, 4), "outside [0, 4)");
  REFUSED(table(1, 3, 4, 4), "outside [0, 4)");
  REFUSED(table(1, 3, 3, 4), "used twice");
  REFUSED(table(-1, 0, 0, 5), "4 samples have an image but P=5");
  REFUSED(table(-1, 0, 0, 3), "outside [0, 3)");                  // P too small: slot 3 no longer fits
  REFUSED(table(0, 1, 1, 4), "outside [0, 4)");                   // a fifth image with slot -1
  memcpy(t, ok, sizeof(t));
  t[4 * 0 + 1] = 1;
  t[4 * 0 + 3] = 4;
  EXPECT(modal3_table_check(t, B, 5) == MLA_OK);

  // the plan at the training shapes: B = 32, S = 256, 1024 x 128, L = 256 -- units and the capped grid
  EXPECT(modal3_shape_plan(32, 256, 1024 * 128, 256, &p) == MLA_OK);
  EXPECT(p.image == 49152 && p.spec == 32768 && p.token == 128 && p.pm == 64 && p.total == 82112);
  EXPECT(p.blocks_x == MODAL3_MAX_BLOCKS / 32 && (long long)p.blocks_x * 32 <= MODAL3_MAX_BLOCKS);
  EXPECT(modal3_shape_plan(5000, 2, 8, 4, &p) == MLA_OK && p.blocks_x == 1);
  return host_check_done("modal3");
}
