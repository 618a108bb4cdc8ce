// Host check of csrc/scratch_carver.h and of sosvo_dense_stereo's layout in csrc/dense_scratch.h (tests/test_scratch_carver.py
// compiles and runs it).  Prints "ok" and returns 0, or says what failed.
#include <stdint.h>
#include <stdio.h>

#include "dense_scratch.h"
#include "scratch_carver.h"

static int failures = 0;
#define CHECK(cond)                                               \
  do {                                                            \
    if (!(cond)) {                                                \
      printf("line %d: %s does not hold\n", __LINE__, #cond);     \
      ++failures;                                                 \
    }                                                             \
  } while (0)

// a layout of mixed types and sizes, one of them empty: the offsets each take starts at, and the total
struct Mixed {
  uint8_t* a;
  double* b;
  uint16_t* none;
  uint32_t* c;
  uint64_t* d;
  size_t at[5], total;
};
static Mixed mixed(Carver& cv) {
  Mixed m;
  m.at[0] = cv.off;
  m.a = cv.take<uint8_t>(1);        // 1 byte -> 256
  m.at[1] = cv.off;
  m.b = cv.take<double>(33);        // 264 bytes -> 512
  m.at[2] = cv.off;
  m.none = cv.take<uint16_t>(0);    // nothing
  m.at[3] = cv.off;
  m.c = cv.take<uint32_t>(64);      // 256 bytes -> 256
  m.at[4] = cv.off;
  m.d = cv.take<uint64_t>(1000);    // 8000 bytes -> 8192
  m.total = cv.off;
  return m;
}

int main() {
  CHECK(sosvo_round256(0) == 0 && sosvo_round256(1) == 256 && sosvo_round256(255) == 256 && sosvo_round256(256) == 256 &&
        sosvo_round256(257) == 512);

  Carver measure{nullptr};
  const Mixed m = mixed(measure);
  CHECK(m.a == nullptr && m.b == nullptr && m.none == nullptr && m.c == nullptr && m.d == nullptr);  // null while measuring
  const size_t want[5] = {0, 256, 768, 768, 1024};
  for (int i = 0; i < 5; ++i) CHECK(m.at[i] == want[i] && m.at[i] % 256 == 0);
  CHECK(m.at[3] == m.at[2]);  // take<T>(0) advances by nothing
  CHECK(m.total == 1024 + 8192);

  static char arena[16384];
  Carver place{arena};
  const Mixed p = mixed(place);
  for (int i = 0; i < 5; ++i) CHECK(p.at[i] == m.at[i]);  // the placing pass: the same offsets and total
  CHECK(p.total == m.total && p.total <= sizeof(arena));
  CHECK((char*)p.a == arena + want[0] && (char*)p.b == arena + want[1] && (char*)p.none == arena + want[2] &&
        (char*)p.c == arena + want[3] && (char*)p.d == arena + want[4]);  // typed pointers at base + offset

  // sosvo_dense_stereo at n = 2, rows = 3, cols = 5: 30 pixels, 64 disparities.  By hand, each rounded up to 256:
  //   census words 30 * 8 = 240 -> 256 per view; C 30 * 64 = 1920 -> 2048; S 30 * 64 * 2 = 3840 -> 3840 (unless S_out is
  //   given); k* 30 -> 256; left-right keys 30 * 4 = 120 -> 256 (only with lr_max >= 0)
  const size_t total = 2 * 3 * 5;
  for (int s_given = 0; s_given < 2; ++s_given)
    for (int want_lr = 0; want_lr < 2; ++want_lr) {
      Carver dm{nullptr};
      const sosvo_dense_scratch z = sosvo_dense_carve(dm, total, 64, s_given != 0, want_lr != 0);
      CHECK(!z.census_top && !z.census_bot && !z.C && !z.S && !z.kstar && !z.best);
      Carver dp{arena};
      const sosvo_dense_scratch b = sosvo_dense_carve(dp, total, 64, s_given != 0, want_lr != 0);
      const size_t o_k = s_given ? 2560 : 2560 + 3840;
      CHECK((char*)b.census_top == arena);
      CHECK((char*)b.census_bot == arena + 256);
      CHECK((char*)b.C == arena + 512);
      CHECK((char*)b.S == arena + 2560);  // (where S lies when it is carved; with S_out the entry point never uses it)
      CHECK((char*)b.kstar == arena + o_k);
      CHECK((char*)b.best == arena + o_k + 256);
      const size_t want_total = o_k + 256 + (want_lr ? 256 : 0);
      CHECK(dm.off == want_total && dp.off == want_total && want_total <= sizeof(arena));
    }
  Carver all{nullptr};
  sosvo_dense_carve(all, total, 64, false, true);
  CHECK(all.off == 6912);  // 256 + 256 + 2048 + 3840 + 256 + 256

  if (failures == 0) printf("ok\n");
  return failures == 0 ? 0 : 1;
}
