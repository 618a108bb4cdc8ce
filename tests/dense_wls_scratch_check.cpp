// Host check of sosvo_dense_wls's layout in csrc/dense_wls_scratch.h (tests/test_wls_scratch.py compiles and runs it), against
// the sizes include/sosvo_dense_filter.h and DESIGN.md section 41 state.  Prints "ok" and returns 0, or says what failed.
#include <stdint.h>
#include <stdio.h>

#include "dense_wls_scratch.h"

static int failures = 0;
#define CHECK(cond)                                               \
  do {                                                            \
    if (!(cond)) {                                                \
      printf("line %d: %s does not hold\n", __LINE__, #cond);     \
      ++failures;                                                 \
    }                                                             \
  } while (0)

int main() {
  // n = 2, rows = 3, cols = 5: 30 pixels, 6 rows.  By hand, each rounded up to 256: the table 256 * 8 = 2048; a plane of doubles
  // 30 * 8 = 240 -> 256, five of them (N, D, c', two f'); in the cyclic form a sixth and 6 * 2 * 8 = 96 -> 256 for the rows' vy / vz
  static char arena[8192];
  const size_t total = 2 * 3 * 5, lines = 2 * 3;
  for (int cyclic = 0; cyclic < 2; ++cyclic) {
    Carver m{nullptr};
    const sosvo_dense_wls_scratch z = sosvo_dense_wls_carve(m, total, lines, cyclic != 0);
    CHECK(!z.weights && !z.N && !z.D && !z.cp && !z.fN && !z.fD && !z.fz && !z.ratio);
    Carver p{arena};
    const sosvo_dense_wls_scratch b = sosvo_dense_wls_carve(p, total, lines, cyclic != 0);
    CHECK((char*)b.weights == arena);
    CHECK((char*)b.N == arena + 2048 && (char*)b.D == arena + 2304 && (char*)b.cp == arena + 2560);
    CHECK((char*)b.fN == arena + 2816 && (char*)b.fD == arena + 3072);
    CHECK((char*)b.fz == arena + 3328);  // (where it lies when it is carved)
    CHECK((char*)b.ratio == arena + (cyclic ? 3584 : 3328));
    const size_t want = cyclic ? 3840 : 3328;
    CHECK(m.off == want && p.off == want && want <= sizeof(arena));
  }
  // the working size, 64 frames of 146 x 1440: 40 bytes per pixel, 48 and 16 per row in the cyclic form, and the table; no more
  // than the 56 per pixel the definition allows, at the narrowest cyclic map as well (3 columns: 48 + 16 / 3)
  const size_t px = (size_t)64 * 146 * 1440, ln = (size_t)64 * 146;
  Carver big{nullptr}, big_cyclic{nullptr}, narrow{nullptr};
  sosvo_dense_wls_carve(big, px, ln, false);
  sosvo_dense_wls_carve(big_cyclic, px, ln, true);
  sosvo_dense_wls_carve(narrow, ln * 3, ln, true);
  CHECK(big.off == 2048 + 40 * px && big_cyclic.off == 2048 + 48 * px + 16 * ln);
  CHECK(big_cyclic.off <= 56 * px && narrow.off <= 56 * (ln * 3));

  if (failures == 0) printf("ok\n");
  return failures == 0 ? 0 : 1;
}
