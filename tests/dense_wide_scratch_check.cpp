// Host check of sosvo_dense_stereo_wide's layout in csrc/dense_wide_scratch.h (tests/test_dense_wide_reference.py compiles and
// runs it), against the sizes include/sosvo_dense_wide.h and DESIGN.md section 42 state.  Prints "ok" and returns 0, or says
// what failed.
#include <stdint.h>
#include <stdio.h>

#include "dense_scratch.h"
#include "dense_wide_scratch.h"

static int failures = 0;
#define CHECK(cond)                                               \
  do {                                                            \
    if (!(cond)) {                                                \
      printf("line %d: %s does not hold\n", __LINE__, #cond);     \
      ++failures;                                                 \
    }                                                             \
  } while (0)

int main() {
  // n = 2, rows = 3, cols = 5, D = 48: 30 pixels.  By hand, each rounded up to 256: a plane of census words 30 * 8 = 240 -> 256;
  // C 30 * 48 = 1440 -> 1536; S 2880 -> 3072; k* 30 * 2 = 60 -> 256; the left-right keys 120 -> 256
  static char arena[8192];
  const size_t total = 2 * 3 * 5, D = 48;
  for (int s_given = 0; s_given < 2; ++s_given)
    for (int want_lr = 0; want_lr < 2; ++want_lr) {
      Carver m{nullptr};
      const sosvo_dense_wide_scratch z = sosvo_dense_wide_carve(m, total, D, s_given != 0, want_lr != 0);
      CHECK(!z.census_top && !z.census_bot && !z.C && !z.S && !z.kstar && !z.best);
      Carver p{arena};
      const sosvo_dense_wide_scratch b = sosvo_dense_wide_carve(p, total, D, s_given != 0, want_lr != 0);
      CHECK((char*)b.census_top == arena && (char*)b.census_bot == arena + 256 && (char*)b.C == arena + 512);
      CHECK((char*)b.S == arena + 2048);  // (where it lies when it is carved)
      const size_t after_S = s_given ? 2048 : 5120;
      CHECK((char*)b.kstar == arena + after_S && (char*)b.best == arena + after_S + 256);
      const size_t want = after_S + 256 + (want_lr ? 256 : 0);
      CHECK(m.off == want && p.off == want && want <= sizeof(arena));
    }
  // the working size, 64 frames of 146 x 1440: 22 + 3 D bytes per pixel, D + 18 with the caller's S and no left-right check
  const size_t px = (size_t)64 * 146 * 1440;
  for (size_t d = 16; d <= 256; d += 16) {
    Carver all{nullptr}, least{nullptr};
    sosvo_dense_wide_carve(all, px, d, false, true);
    sosvo_dense_wide_carve(least, px, d, true, false);
    CHECK(all.off == (22 + 3 * d) * px && least.off == (18 + d) * px);
  }
  // one byte per pixel more than the 64-disparity layout of dense_scratch.h (213 -> 214 at D = 64): k* is 16 bits wide
  Carver old64{nullptr}, wide64{nullptr};
  sosvo_dense_carve(old64, px, 64, false, true);
  sosvo_dense_wide_carve(wide64, px, 64, false, true);
  CHECK(old64.off == 213 * px && wide64.off == 214 * px);

  if (failures == 0) printf("ok\n");
  return failures == 0 ? 0 : 1;
}
